"""CPU: the order of search results (hmse_amd.find sort / sort_regex / order_ranges; include/hmse_order.h) without a GPU — the plain-Python
reference of tests/order_ref.py against sorted(), its key against the kernels' own keys (tools/order_emu.py runs order.hip's kernels on
CPU threads), the rounds of find.order_ranges on CPU tensors with plain-Python stand-ins for the two ops calls, with the skip on and
off, then the new header against _lib (prototypes, exported symbols, the ISA audit), the entry points' own refusals (HMSE_EINVAL in
front of every HIP call) and the wrappers' and methods' refusals."""
import itertools
import os
import random
import re
import subprocess
import sys

import pytest

import order_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmse_order.h")
CALLS = ("hmse_order_keys", "hmse_order_lcp")
FIELDS = ("ptr", "index", "start", "end", "first", "count", "distinct", "total", "rank_of")


def _random_case(rnd, n_max=60):
    """a corpus over a few words in both cases, zero and 0xFF bytes and bytes whose | 0x20 form is another byte; ranges in 1..3 groups,
    some empty, many equal texts at different starts"""
    words = [b"ab", b"AB", b"aB", b"abc", b"@", b"`", b"[", b"{", b"\xc1", b"\xe1", b"z", b"Z", b"", b"\x00", b"\xff", b"abcabcab"]
    corpus = b"".join(rnd.choice(words) for _ in range(rnd.randint(0, 40)))
    N = len(corpus)
    n = rnd.randint(0, n_max)
    starts, ends = [], []
    for _ in range(n):
        s = rnd.randint(0, N)
        e = s if rnd.random() < 0.1 else min(N, s + rnd.randint(0, rnd.choice([3, 3, 20])))
        starts.append(s); ends.append(e)
    G = rnd.randint(1, 3)
    ptr = [0] + sorted(rnd.randint(0, n) for _ in range(G - 1)) + [n]
    return corpus, starts, ends, ptr


# ---- the reference against sorted() ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ic", [False, True])
def test_reference_equals_sorted_over_slices_with_ties_runs_and_ranks(ic):
    rnd = random.Random(21 + ic)
    ties = empties = 0
    low = lambda b: bytes(c + 32 if 65 <= c <= 90 else c for c in b)
    assert low(b"AZ@[\xc1") == b"az@[\xc1" == b"AZ@[\xc1".lower()
    for _ in range(300):
        corpus, starts, ends, ptr = _random_case(rnd)
        full, uniq = ref.order(corpus, starts, ends, ptr, ic), ref.order(corpus, starts, ends, ptr, ic, unique=True)
        for j in range(len(ptr) - 1):
            texts = {i: low(corpus[starts[i]:ends[i]]) if ic else corpus[starts[i]:ends[i]] for i in range(ptr[j], ptr[j + 1])}
            want = sorted(texts, key=lambda i: (texts[i], starts[i], i))
            lo, hi = full["ptr"][j], full["ptr"][j + 1]
            assert (lo, hi) == (ptr[j], ptr[j + 1]) and full["index"][lo:hi] == want
            assert [texts[i] for i in want] == sorted(texts.values())                  # as Python orders bytes: a prefix first, the empty text first of all
            assert [full["rank_of"][i] for i in want] == list(range(hi - lo)) and full["count"][lo:hi] == [1] * (hi - lo)
            distinct = sorted(set(texts.values()))
            assert full["distinct"][j] == uniq["distinct"][j] == len(distinct) and full["total"][j] == uniq["total"][j] == hi - lo
            assert [texts[i] for i, f in zip(want, full["first"][lo:hi]) if f] == distinct
            ulo, uhi = uniq["ptr"][j], uniq["ptr"][j + 1]
            assert [texts[i] for i in uniq["index"][ulo:uhi]] == distinct and uniq["first"][ulo:uhi] == [True] * len(distinct)
            assert uniq["count"][ulo:uhi] == [sum(1 for t in texts.values() if t == v) for v in distinct]
            for i, c in zip(uniq["index"][ulo:uhi], uniq["count"][ulo:uhi]):            # a run's head is its member with the smallest (start, index)
                assert (starts[i], i) == min((starts[k], k) for k in texts if texts[k] == texts[i])
            ties += len(distinct) < len(texts)
            empties += b"" in distinct
        assert full["start"] == [starts[i] for i in full["index"]] and uniq["end"] == [ends[i] for i in uniq["index"]] and uniq["rank_of"] == full["rank_of"]
    assert ties > 100 and empties > 50


def test_reference_key_orders_texts_and_tells_padding_from_zero_bytes():
    """key_a < key_b implies text_a < text_b for texts that agree in front of the depth; equal keys with r <= 7 mean equal texts; with r = 8
    they agree through depth + 7.  Over the alphabets {0, 'a'}, {0, 0xFF} and a sample of all 256 values, at lengths around 0, 6, 7, 8, 9."""
    header = open(HEADER).read()
    assert int(re.search(r"#define HMSE_ORDER_KEY_BYTES (\d+)u", header).group(1)) == ref.KEY_BYTES == 7
    assert int(re.search(r"#define HMSE_ORDER_R_MORE\s+(\d+)u", header).group(1)) == ref.R_MORE == 8
    rnd = random.Random(3)
    for alpha in (b"\x00a", b"\x00\xff", bytes(range(256))):
        texts = {bytes(rnd.choice(alpha) for _ in range(L)) for L in (0, 1, 5, 6, 7, 8, 9, 14, 15) for _ in range(40)}
        texts |= {t[:k] for t in list(texts)[:60] for k in range(len(t))}
        for d in (0, 1, 7):
            pool = [t for t in texts if len(t) >= d]
            for a, b in itertools.islice(itertools.combinations(sorted(pool), 2), 40000):
                if a[:d] != b[:d]:
                    continue
                ka, kb = ref.key_of_text(a, d), ref.key_of_text(b, d)
                assert ka < 1 << 60 and kb < 1 << 60
                if ka != kb:
                    assert (ka < kb) == (a < b), (a, b, d)
                elif ka & 15 <= 7:
                    assert a == b
                else:
                    assert a[: d + 7] == b[: d + 7] and ka & 15 == 8
    assert ref.key_of_text(b"", 0) == 0 and ref.key_of_text(b"\x00", 0) == 1 and ref.key_of_text(b"\x00" * 9, 0) == 8 and ref.key_of_text(b"\x00" * 9, 2) == 7
    assert ref.key_of_text(b"abcdefgh", 0) == (int.from_bytes(b"abcdefg", "big") << 4) | 8 and ref.key_of_text(b"abcdefgh", 8) == 0
    assert ref.key(b"xABCx", 1, 4, 0, True) == ref.key_of_text(b"abc", 0) != ref.key(b"xABCx", 1, 4, 0)
    assert ref.text_of(b"@[`{\xc1AZ", 0, 7, True) == b"@[`{\xc1az"
    assert ref.lcp(b"abcXabcY", [0, 4, 0], [4, 8, 4], [1, 0, 2], [0, 1, 0]) == [3, 3, 4] and ref.lcp(b"qbcXabcY", [0], [4], [0], [0]) == [4]
    assert ref.lcp(b"qbcXabcX", [0, 4], [4, 8], [1, 0], [1, 1]) == [4, 4]                   # the bytes in front of from are not looked at


# ---- the kernels on the CPU ------------------------------------------------------------------------------------------------------------------
def test_the_emulator_passes_and_its_keys_equal_the_python_restatement_bit_for_bit():
    """A short unsanitised pass of tools/order_emu.py (the kernels of order.hip, one std::thread per lane, against the definition on random
    chunk maps), then its KEY lines: ranges of length 0, 1, 6, 7, 8, 9, 15, 16 and 64 of the corpus C[q] = (37 q + 11) & 0xFF (0x00 and 0xFF
    planted where windows end, 5-byte chunks) at depths 0, 1, L and L - 6 .. L - 9, folded and not."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "order_emu.py"), "--iters", "12"], capture_output=True, text=True)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    c = bytearray((q * 37 + 11) & 0xFF for q in range(300))
    c[7 + 6], c[49 + 6], c[172 + 7], c[172 + 8] = 0x00, 0xFF, 0x00, 0xFF
    corpus = bytes(c)
    assert any(65 <= b <= 90 for b in corpus[:64])
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("KEY ")]
    seen, last = set(), set()
    for _, s, e, d, fold, key in rows:
        s, e, d, fold = int(s), int(e), int(d), int(fold)
        assert int(key, 16) == ref.key(corpus, s, e, d, bool(fold)), (s, e, d, fold)
        L = e - s
        seen.add((L - d, "0" if d == 0 else "L" if d == L else "1" if d == 1 else "in", fold))
        if L - d >= 7:
            last.add(corpus[s + d + 6])                                                 # the byte at the end of the window
    for fold in (0, 1):
        assert {(left, fold) for left, _, f in seen if f == fold} >= {(x, fold) for x in (0, 6, 7, 8, 9)}
        assert {w for _, w, f in seen if f == fold} == {"0", "1", "L", "in"}
    assert {0x00, 0xFF} <= last and len(rows) == 2 * sum(r_[4] == "0" for r_ in rows) >= 300
    assert len({r_[5] for r_ in rows if r_[4] == "0"}) > 60


# ---- the rounds on CPU tensors -----------------------------------------------------------------------------------------------------------------
def _stand_ins(corpus, ic, calls):
    import torch
    def keys(s, e, d):
        calls.append(("keys", s.numel()))
        assert s.is_contiguous() and e.is_contiguous() and d.is_contiguous() and d.dtype == torch.int64
        return torch.tensor(ref.keys(corpus, s.tolist(), e.tolist(), d.tolist(), ic), dtype=torch.int64)
    def lcp(s, e, rep, frm):
        calls.append(("lcp", s.numel()))
        assert s.is_contiguous() and rep.is_contiguous() and frm.is_contiguous() and rep.dtype == torch.int64 and s.numel() >= 2
        assert int(rep.min()) >= 0 and int(rep.max()) < s.numel()
        return torch.tensor(ref.lcp(corpus, s.tolist(), e.tolist(), rep.tolist(), frm.tolist(), ic), dtype=torch.int64)
    return keys, lcp


def _run_rounds(corpus, starts, ends, ptr, ic=False, unique=False, max_rounds=64, skip=True):
    import torch
    from hmse_amd import find
    i64 = lambda v: torch.tensor(v, dtype=torch.int64)
    G = len(ptr) - 1
    group = torch.repeat_interleave(torch.arange(G), i64(ptr[1:]) - i64(ptr[:-1]))
    calls = []
    keys, lcp = _stand_ins(corpus, ic, calls)
    s = find.order_ranges(i64(starts), i64(ends), group, G, keys, lcp, unique, max_rounds, skip)
    return s, calls


def _same(got, want):
    import torch
    for f in FIELDS:
        t = getattr(got, f)
        assert t.dtype == (torch.bool if f == "first" else torch.int64) and t.tolist() == want[f], f


@pytest.mark.parametrize("skip", [True, False])
def test_rounds_on_cpu_tensors_give_the_reference_order(skip):
    rnd = random.Random(6)
    most = 0
    for it in range(80):
        corpus, starts, ends, ptr = _random_case(rnd, n_max=80)
        ic, unique = bool(it & 1), bool(it & 2)
        s, calls = _run_rounds(corpus, starts, ends, ptr, ic, unique, skip=skip)
        _same(s, ref.order(corpus, starts, ends, ptr, ic, unique))
        assert s.rounds == sum(c[0] == "keys" for c in calls) and (len(starts) == 0) == (s.rounds == 0)
        assert (sum(c[0] == "lcp" for c in calls) == 0) if not skip else True
        sizes = [c[1] for c in calls if c[0] == "keys"]
        assert sizes == sorted(sizes, reverse=True) and (not sizes or sizes[0] == len(starts))     # fewer ranges keyed every round
        most = max(most, s.rounds)
    assert most >= 2


def test_the_chain_of_prefixes_and_its_runtime_error():
    """a, aa, ..., a^40 (and a second copy of every one): eight lengths finish per round — the known bad case max_rounds is for"""
    corpus = b"a" * 40
    starts, ends = [0] * 40 + [0] * 40, list(range(1, 41)) * 2
    want = ref.order(corpus, starts, ends, [0, 80])
    assert want["index"] == [i for k in range(40) for i in (k, k + 40)]
    for skip in (True, False):
        s, calls = _run_rounds(corpus, starts, ends, [0, 80], skip=skip)
        _same(s, want)
        assert 5 <= s.rounds <= 7
    _same(_run_rounds(corpus, starts, ends, [0, 80], unique=True)[0], ref.order(corpus, starts, ends, [0, 80], unique=True))
    with pytest.raises(RuntimeError, match=r"sort: \d+ of 80 ranges are unresolved after max_rounds = 2 rounds \(their buckets stand at depths \d+\.\.\d+\)"):
        _run_rounds(corpus, starts, ends, [0, 80], max_rounds=2)


def test_fifty_equal_long_texts_take_two_rounds_with_the_skip():
    text = bytes(random.Random(9).randrange(97, 123) for _ in range(300))
    near = [text[:299] + b"!", text[:150] + b"!" + text[151:], text[:8] + b"!" + text[9:]]
    corpus = text * 50 + b"".join(near)
    starts = [300 * k for k in range(53)]
    ends = [s + 300 for s in starts]
    s, calls = _run_rounds(corpus, starts[:50], ends[:50], [0, 50])
    assert s.rounds <= 2 and s.index.tolist() == list(range(50)) and s.first.tolist() == [True] + [False] * 49 and s.distinct.tolist() == [1]
    assert [c[0] for c in calls] == ["keys", "lcp", "keys"]
    u, _ = _run_rounds(corpus, starts[:50], ends[:50], [0, 50], unique=True)
    assert (u.index.tolist(), u.count.tolist(), u.ptr.tolist(), u.rank_of.tolist()) == ([0], [50], [0, 1], list(range(50)))
    want = ref.order(corpus, starts, ends, [0, 53])
    a, _ = _run_rounds(corpus, starts, ends, [0, 53])
    b, _ = _run_rounds(corpus, starts, ends, [0, 53], skip=False)
    _same(a, want); _same(b, want)
    assert a.rounds <= 5 < 40 <= b.rounds                                                  # 300 / 7 rounds without the skip


# ---- the header, the library, the entry points -------------------------------------------------------------------------------------------------
def test_signatures_equal_the_header():
    import test_abi
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    header = open(HEADER).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = re.findall(r"^(\w+) (hmse_[a-z0-9_]+)\(([^;]*)\);", plain, re.M)
    assert [name for _, name, _ in protos] == list(_lib.ORDER_SIGNATURES) == list(CALLS)
    others = set(_lib.PARSED) | set(_lib.PARSED_REGEXA) | set(_lib.PARSED_TALLY) | set(_lib.PARSED_SUBST)
    assert not set(_lib.ORDER_SIGNATURES) & others and set(_lib.PARSED_ORDER) == set(CALLS)
    for ret, name, params in protos:
        t_ret, _, t_params = _lib.ORDER_SIGNATURES[name].partition(":")
        entries = [e.split() if e.strip() != "stream" else ["stream", "stream"] for e in t_params.split(",")]
        decls = [re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*", d).groups() for d in params.split(",")]
        assert test_abi._C_RETURN[t_ret] == ret and [e[1] for e in entries] == [d[2] for d in decls], name
        assert all(test_abi.kind_agrees(kind, ty, bool(star)) for (kind, _), (ty, star, _) in zip(entries, decls)), name
        fn = getattr(lib, name)
        assert fn.restype is _lib.PARSED_ORDER[name][0] and list(fn.argtypes) == [q.ctype for q in _lib.PARSED_ORDER[name][1]], name
    # the tables are hmse_lines_gather's, the ABI version stays
    assert _lib.ORDER_SIGNATURES["hmse_order_keys"].split(" u64*? start")[0] == _lib.SIGNATURES["hmse_lines_gather"].split(" u64*? start")[0]
    assert _lib.ORDER_SIGNATURES["hmse_order_lcp"].split(" u64*? start")[0] == _lib.SIGNATURES["hmse_lines_gather"].split(" u64*? start")[0]
    assert lib.hmse_abi_version() == 3
    assert "Out of scope" in header and "bit 1" in header and "descending order" in header


def test_a_missing_library_is_an_import_error_like_the_tally_s(monkeypatch, tmp_path):
    from hmse_amd import _lib
    gone = str(tmp_path / "libhmse_order.so")
    monkeypatch.setattr(_lib, "_hip", None)
    monkeypatch.setattr(_lib, "ORDER_LIB_PATH", gone)
    with pytest.raises(ImportError) as e:
        _lib.hip_lib()
    monkeypatch.setattr(_lib, "TALLY_LIB_PATH", str(tmp_path / "libhmse_tally.so"))
    with pytest.raises(ImportError) as t:
        _lib.hip_lib()
    assert str(e.value).replace("order", "tally") == str(t.value) and gone in str(e.value) and "g.build()" in str(e.value)
    assert _lib._hip is None


def test_the_library_exports_its_header_and_passes_the_isa_audit():
    """libhmse_order.so beside libhmse_hip.so: exported == declared in include/hmse_order.h; no divergent loop in the LCP kernel, which
    holds the one cross-lane operation, and no cross-lane instruction inside a divergent loop anywhere (the keys kernel's loops are
    divergent: a thread per range); no Async / Graph import, no import the pinned list does not allow.  The other libraries gain no
    symbol."""
    import json
    from hmse_amd import _lib
    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return sorted(x for x in (ln.split()[-1] for ln in out.splitlines() if ln.split()[1:2] and ln.split()[1] in "TW") if not x.startswith("_"))
    assert exported(_lib.ORDER_LIB_PATH) == sorted(CALLS)
    assert exported(_lib.TALLY_LIB_PATH) == sorted(_lib.TALLY_SIGNATURES) and exported(_lib.SUBST_LIB_PATH) == sorted(_lib.SUBST_SIGNATURES)
    assert not [x for x in exported(_lib.HIP_LIB_PATH) if "order" in x] and not set(CALLS) & set(_lib.EXPORTED_SYMBOLS)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    rep = isa_audit.audit(_lib.ORDER_LIB_PATH)
    assert {"order_ranges_kernel", "order_keys_kernel", "order_lcp_kernel"} <= set(rep)
    assert rep["order_lcp_kernel"]["loops"] >= 2 and rep["order_lcp_kernel"]["divergent_loops"] == 0, rep["order_lcp_kernel"]
    assert rep["order_keys_kernel"]["loops"] >= 1, rep["order_keys_kernel"]
    assert isa_audit.summary(rep) == {}
    pin = json.load(open(os.path.join(ROOT, "tests", "golden", "isa_audit.json")))
    imports = isa_audit.imported_hip_calls(_lib.ORDER_LIB_PATH)
    assert not [x for x in imports if "Async" in x or "Graph" in x], imports
    assert set(imports) <= set(pin["hip_imports_allowed"]), sorted(set(imports) - set(pin["hip_imports_allowed"]))


def test_the_new_sources_cap_no_grid_and_stride_by_none():
    """every launch of order.hip covers its n directly: the audit of tests/grid_caps.py finds nothing in it, and nothing to exempt"""
    import grid_caps as G
    sites = [s for s in G.capped_sites() if s[0] == "order.hip"]
    assert sites == [] and not [k for k in G.EXEMPT if k[0] == "order.hip"] and not [k for k in G.NOT_A_GRID if k[0] == "order.hip"]
    src = open(os.path.join(ROOT, "hmse_amd", "csrc", "order.hip")).read()
    assert src.count("<<<") == 3 and "__shared__" not in src


def test_entry_points_refuse_bad_arguments_with_no_gpu_present():
    """HMSE_EINVAL (-1), never HMSE_EHIP (-3): refused in front of every clear and launch (the pointers are host addresses)"""
    import torch
    from hmse_amd import _lib
    lib = _lib.hip_lib()
    mem = torch.zeros(1 << 12, dtype=torch.uint8)
    b = mem.data_ptr() + (-mem.data_ptr()) % 256
    keys_names = ("raw", "raw_bytes", "raw_off", "n_rec", "cuts", "slot", "n_chunks", "start", "end", "depth", "n", "flags", "key", "status")
    lcp_names = ("raw", "raw_bytes", "raw_off", "n_rec", "cuts", "slot", "n_chunks", "start", "end", "rep", "from", "n", "flags", "lcp", "status")
    assert keys_names == tuple(p.name for p in _lib.PARSED_ORDER["hmse_order_keys"][1][:-1]) and lcp_names == tuple(p.name for p in _lib.PARSED_ORDER["hmse_order_lcp"][1][:-1])
    dflt = {"raw": b, "raw_bytes": 64, "raw_off": b, "n_rec": 1, "cuts": b, "slot": b, "n_chunks": 1, "start": b, "end": b, "depth": b, "rep": b, "from": b,
            "n": 2, "flags": 0, "key": b, "lcp": b, "status": b}

    def call(fn, names, **kw):
        a = {**dflt, **kw}
        return fn(*[a[k] for k in names], None)
    both = ((lib.hmse_order_keys, keys_names), (lib.hmse_order_lcp, lcp_names))
    for fn, names in both:
        for kw in (dict(status=None), dict(raw=None), dict(raw_off=None), dict(cuts=None), dict(slot=None), dict(start=None), dict(end=None),
                   dict(n=1 << 31), dict(n=1 << 33), dict(n=(1 << 64) - 1), dict(flags=2), dict(flags=3), dict(flags=1 << 31),
                   dict(raw_off=None, n_chunks=0, n=0), dict(status=None, n=0)):
            assert call(fn, names, **kw) == -1, (names[9], kw)
    for kw in (dict(depth=None), dict(key=None)):
        assert call(*both[0], **kw) == -1, kw
    for kw in (dict(rep=None), {"from": None}, dict(lcp=None)):
        assert call(*both[1], **kw) == -1, kw
    assert mem.sum().item() == 0


def test_wrappers_and_methods_refuse_what_they_should(monkeypatch):
    import torch
    from hmse_amd import find, ops
    u8 = torch.zeros(8, dtype=torch.uint8)
    z = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.order_keys(u8, z, z, z[:1], z, z, z)
    with pytest.raises(ops.HmseError, match="must live in HBM"):
        ops.order_lcp(u8, z, z, z[:1], z, z, z, z)
    with pytest.raises(ops.HmseError, match="depth must be torch.int64"):
        ops.order_keys(u8, z, z, z[:1], z, z, z.to(torch.int32))
    with pytest.raises(ops.HmseError, match="from must be torch.int64"):
        ops.order_lcp(u8, z, z, z[:1], z, z, z, z.to(torch.int32))
    with pytest.raises(ops.HmseError, match="rep must be torch.int64"):
        ops.order_lcp(u8, z, z, z[:1], z, z, z.to(torch.int32), z)
    with pytest.raises(ops.HmseError, match="raw must be torch.uint8"):
        ops.order_keys(u8.to(torch.int8), z, z, z[:1], z, z, z)
    with pytest.raises(ops.HmseError, match="start / end / depth do not match"):
        ops.order_keys(u8, z, z, z[:1], z, z, z[:1])
    with pytest.raises(ops.HmseError, match="start / end / rep / from do not match"):
        ops.order_lcp(u8, z, z, z[:1], z, z, z, z[:1])
    with pytest.raises(TypeError, match="takes 14 arguments"):
        ops._call("hmse_order_keys", 1, 2, 3)
    with pytest.raises(KeyError):
        ops._call("hmse_order_nothing")
    # the methods, on a finder that no device work made: the refusals come in front of every launch
    fd = find.StoreFinder.__new__(find.StoreFinder)
    fd.dev = torch.device("cpu")
    fd.raw, fd.raw_off, fd.cuts, fd.slot, fd.n_bytes = u8, z, z, z[:1], 8
    pair = (torch.tensor([0, 1]), torch.tensor([1, 2]))
    with pytest.raises(ValueError, match=r"sort: what is a Found, which has offsets but no lengths.*spans\(\)"):
        fd.sort(find.Found(z, z[:0], z[:1]))
    with pytest.raises(ValueError, match=r"sort: what is a ApproxFound, which has offsets but no lengths.*\(start, end\) pair"):
        fd.sort(find.ApproxFound(z, z[:0], z[:1], z[:0]))
    with pytest.raises(ValueError, match="int64 tensors on the finder's device"):
        fd.sort((pair[0].to(torch.int32), pair[1]))
    with pytest.raises(ValueError, match="one length"):
        fd.sort((pair[0], pair[1][:1]))
    with pytest.raises(ValueError, match="what is a RegexFound, a Lines, a Tally"):
        fd.sort([1, 2])
    with pytest.raises(ValueError, match="descends or leaves the corpus of n_bytes = 8"):
        fd.sort((pair[0], torch.tensor([1, 9])))
    with pytest.raises(ValueError, match="descends or leaves"):
        fd.sort((torch.tensor([2, 1]), torch.tensor([1, 2])))
    with pytest.raises(ValueError, match="ptr does not split the 2 ranges"):
        fd.sort((pair[0], pair[1], torch.tensor([0, 1])))
    with pytest.raises(ValueError, match="ptr does not split"):
        fd.sort((pair[0], pair[1], torch.tensor([0, 3, 2])))
    # no ranges, no groups: empty results of the right shapes, no launch (the library is never asked)
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail("a launch"))
    e = torch.zeros(0, dtype=torch.int64)
    empty_tally = find.Tally(torch.zeros(3, dtype=torch.int64), e, e, e, z, z, e, 0)
    for what, G in (((e, e), 1), ((e, e, torch.tensor([0, 0, 0])), 2), ((e, e, torch.tensor([0])), 0),
                    (find.RegexFound(torch.zeros(4, dtype=torch.int64), e, z.new_zeros(3), e), 3), (empty_tally, 2)):
        for unique in (False, True):
            s = fd.sort(what, unique=unique)
            assert s.ptr.tolist() == [0] * (G + 1) and s.distinct.tolist() == [0] * G == s.total.tolist() and s.rounds == 0
            assert all(getattr(s, f).numel() == 0 and getattr(s, f).dtype == torch.int64 for f in ("index", "start", "end", "count", "rank_of"))
            assert s.first.numel() == 0 and s.first.dtype == torch.bool
            assert fd.text(s)[0].numel() == 0 and fd.text(s)[1].tolist() == [0]
    with pytest.raises(pytest.fail.Exception, match="a launch"):                  # a host tensor reaches the one call path, which would refuse it
        fd.sort(pair)
