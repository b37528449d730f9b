"""CPU: the inputs of tests/test_gpu_dict_anchors.py are what their names say (anchor_inputs): per job the anchor the content was built for has
the promised number of dictionary members in its bucket, the promised member wins (or none), and the runs are the promised ones — by the
witness, which is oracle/pyref.py::lz_anchors and a plain bucket count; and the oracle runs a dictionary job for every one of them."""
import numpy as np
import pytest

import anchor_inputs as A
import edge_inputs as E


@pytest.fixture(scope="module")
def groups():
    return A.groups()


@pytest.fixture(scope="module")
def seen(groups):
    return {name: A.witness(job) for name, job in groups.items()}


NAMES = ("candidates", "buckets", "counts", "worst", "distance", "padding", "runs")


def test_the_groups_are_the_named_ones(groups):
    assert tuple(groups) == NAMES
    assert all(int(t) <= 65536 for j in groups.values() for t in j["T"]) and all(len(j["ids"]) <= 64 for j in groups.values())


@pytest.mark.parametrize("name", NAMES)
def test_every_job_is_what_it_was_built_to_be(name, groups, seen):
    job = groups[name]
    for j, (w, ex) in enumerate(zip(seen[name], job["expect"])):
        if ex is None:
            continue
        a, members, d, run, back = ex
        print(name, j, "expect", ex, "witness", w.get(a))
        assert a in w, (name, j)
        assert (w[a][0] == members or members is None) and w[a][1] == d, (name, j, ex, w[a])
        if d and run is not None:
            assert w[a][2] == run, (name, j, ex, w[a])
        if d and back is not None:
            assert w[a][3] == back, (name, j, ex, w[a])


def test_candidates_cover_the_member_counts_and_the_edges_of_the_64(groups, seen):
    ex = groups["candidates"]["expect"]
    assert {e[1] for e in ex} >= {0, 1, 63, 64, 65, 200}
    assert {e[1] for e in ex if e[2] == 0} >= {0, 1, 63, 64, 65, 200}          # no member agrees
    assert {e[1] for e in ex if e[2] == len(groups["candidates"]["parts"][1])} >= {1, 63, 64, 65, 200}   # the nearest does (one chunk length back)
    # the winner's place in its bucket, counted from the nearest: 0, the last of the 64, and both sides of the steps of 16 between them
    w = seen["candidates"]
    assert all(x[0][0] == e[1] for x, e in zip(w, ex))


def test_buckets_are_0_4095_and_1(groups):
    parts, ids = groups["buckets"]["parts"], groups["buckets"]["ids"]
    hs = [A.hash4(bytes(parts[int(i)][:4])) for i in ids]
    assert hs == [0, 0, 4095, 4095, 1, 1] and bytes(parts[int(ids[0])][:4]) == bytes(4)
    assert A.hash4(A.gram_of_bucket(4095)) == 4095


def test_counts_cover_the_lengths_the_anchor_numbers_and_the_dictionaries(groups, seen):
    job = groups["counts"]
    Ls = [int(job["parts"][int(i)].size) for i in job["ids"]]
    Ds = {int(job["parts"][int(b)].size) for b in job["base"]}
    assert set(A.COUNT_LENGTHS) <= set(Ls) and {1, 3, 4, 63, 64, 65, 67, 127, 128} <= set(A.COUNT_LENGTHS)
    assert {(L + 63) // 64 for L in Ls} >= set(A.COUNT_ANCHORS) | {1, 2, 3, 4, 5}
    assert Ds >= {3, 1024, 2048}
    for L, w in zip(Ls, seen["counts"]):
        n = (L + 63) // 64
        # the last block's anchor position has four bytes left unless L mod 64 is 1, 2 or 3
        assert (n - 1 in w) == (L % 64 not in (1, 2, 3)), L
        assert set(w) == set(range(n if n - 1 in w else n - 1))
    # near-duplicates: most anchors exist (behind a dictionary of 3 bytes none can)
    for L, b, w in zip(Ls, job["base"], seen["counts"]):
        if int(job["parts"][int(b)].size) >= L >= 64:
            assert sum(1 for v in w.values() if v[1]) >= len(w) // 2, L


def test_worst_case_every_anchor_has_64_agreeing_members_and_the_window_is_the_cap(groups, seen):
    job = groups["worst"]
    assert tuple(int(t) for t in job["T"]) == A.CAPS
    for w in seen["worst"]:
        assert all(v[0] >= 64 and v[1] == 64 * (a + 1) for a, v in w.items())     # (block a's nearest dictionary member: a + 1 periods back)


def test_distance_jobs_are_class_b_and_their_controls_sg3(groups):
    T = [int(t) for t in groups["distance"]["T"]]
    assert T == [32968, 32768, 32968, 32768]
    assert [e[2] for e in groups["distance"]["expect"]] == [32768, 32568, 0, 32569]


def test_the_oracle_runs_a_dictionary_job_for_every_one(groups, orc):
    from dataclasses import asdict
    from hmse_amd import IngestConfig
    for name, job in groups.items():
        odata, ocuts, obase, rows = E.oracle_view(job)
        assert (obase[rows] >= 0).all()
        _, off, kind = orc.deflate_chunks(odata, ocuts, orc.default_cfg(**asdict(IngestConfig())), None, obase)
        assert set(np.unique(kind[rows])) <= {0, 2}, name
        assert (np.diff(off.astype(np.int64))[rows] > 0).all(), name
        # where the content was built so that the anchor's member is followed by the whole chunk, the delta is accepted
        for j, ex in enumerate(job["expect"]):
            if name in ("candidates", "buckets", "worst", "runs") and ex is not None and ex[2]:
                assert kind[rows[j]] == 2, (name, j)
