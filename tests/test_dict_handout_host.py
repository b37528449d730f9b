"""CPU: the inputs of tests/test_gpu_dict_handout.py keep the promises their names make (dict_handout_inputs: "all" hinted, "none"
hinted, "mixed"), by the witness written from the definition of rules 2b / 2c; and the oracle runs a dictionary job for every one of them."""
import numpy as np
import pytest

import dict_handout_inputs as H
import edge_inputs as E


def _jobs():
    return list(H.groups().items()) + [("depths", H.depth_job())]


def test_the_caps_are_the_libraries():
    from hmse_amd import ops
    assert tuple(ops.DEFLATE_CLASS_CAPS) == H.CAPS


@pytest.mark.parametrize("name,job", _jobs(), ids=[n for n, _ in _jobs()])
def test_every_job_keeps_its_promise(name, job):
    unhinted = H.witness(job)
    seen = set()
    for j, (u, pr) in enumerate(zip(unhinted, job["promise"])):
        L = int(job["parts"][int(job["ids"][j])].size)
        hashed = max(L - 3, 0)
        print(name, j, "L", L, "T", int(job["T"][j]), pr, "unhinted", u, "of", hashed)
        assert 0 <= u <= hashed
        if pr == "all":
            assert u == 12, (name, j, u)              # the window's last 15 positions have fewer than 16 bytes left: 12 of them are hashed
        elif pr == "none":
            assert u == hashed, (name, j, u, hashed)
        elif pr == "mixed":
            assert 0.05 * hashed <= u <= 0.60 * hashed, (name, j, u, hashed)
        seen.add(pr)
    if name == "contents":
        assert seen >= {"all", "none", "mixed", None}
    if name in ("caps", "depths"):
        assert seen == {"mixed"}


def test_the_groups_cover_what_they_are_for():
    g = H.groups()
    T = g["caps"]["T"]
    assert {int(t) for t in T} == {c + k for c in H.CAPS for k in (-1, 0, 1)}
    assert all(int(t) <= 65536 for j in g.values() for t in j["T"]) and all(len(j["ids"]) <= 64 for j in g.values())
    Ls = {int(g["lengths"]["parts"][int(i)].size) for i in g["lengths"]["ids"]}
    Ds = {int(g["lengths"]["parts"][int(b)].size) for b in g["lengths"]["base"]}
    assert Ls == set(H.LENGTHS) and Ds == set(H.DICT_LENGTHS) and 3 in Ds and any(d % 1024 == 0 for d in Ds) and any(d % 1024 for d in Ds)
    ld = g["long_dictionary"]
    assert sorted(int(t) for t in ld["T"][:3]) == [32768, 32769, 35768] and int(ld["parts"][int(ld["base"][2])].size) > 32768


@pytest.mark.parametrize("name,job", _jobs(), ids=[n for n, _ in _jobs()])
def test_the_oracle_runs_a_dictionary_job_for_every_one(name, job, orc):
    """A record that can be a DELTA: the chunk has a base, the oracle answers with a DELTA record (kind 2) or — where the delta was refused
    as too large — with the FULL record of the second pass (kind 0), never with a pointer."""
    from dataclasses import asdict
    from hmse_amd import IngestConfig
    odata, ocuts, obase, rows = E.oracle_view(job)
    assert (obase[rows] >= 0).all()
    _, off, kind = orc.deflate_chunks(odata, ocuts, orc.default_cfg(**asdict(IngestConfig())), None, obase)
    assert set(np.unique(kind[rows])) <= {0, 2}
    assert (np.diff(off.astype(np.int64))[rows] > 0).all()
    if name in ("caps", "depths"):
        assert (kind[rows] == 2).all()               # near-duplicates: the delta is accepted
