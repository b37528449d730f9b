"""Static guard for the match kernels' register budget: tools/spill_audit.py on the shipped library, CPU only.

The DEFLATE match kernels are bound by the vector instructions they issue, and until round 8 one in six of the static vector instructions
outside the matcher's trip loop was a `v_readlane_b32` / `v_writelane_b32` that moved a spilled SGPR; the two-per-CU dictionary kernels
spilled vector registers to scratch on top.  The conditions asserted here are what keeps that from coming back unnoticed."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _library():
    lib = os.path.join(ROOT, "hmse_amd", "csrc", "libhmse_hip.so")
    if not os.path.exists(lib):
        import __graft_entry__ as g
        g.build()
    return lib


def test_spill_audit_tells_spill_traffic_from_cross_lane_reads():
    import spill_audit
    # v9 is only ever written by v_writelane (SGPR spill space): its lane moves are spill traffic, inside the loop 4..16.
    # v2 is written by an ordinary vector instruction: the v_readlane from it is a genuine cross-lane read.
    ins = [(0, "v_writelane_b32", "v9, s4, 0", None), (4, "v_mov_b32_e32", "v2, v0", None), (8, "v_readlane_b32", "s6, v9, 0", None),
           (12, "v_readlane_b32", "s7, v2, 3", None), (16, "s_cbranch_scc1", "65533", 4), (20, "scratch_store_dword", "off, v3, s32", None),
           (24, "s_endpgm", "", None)]
    assert spill_audit.spill_vgprs(ins) == {"v9"}
    rep = spill_audit.audit_function(ins)
    assert rep["total"]["reload"] == 1 and rep["total"]["spill_write"] == 1 and rep["total"]["cross_lane"] == 1 and rep["total"]["scratch_st"] == 1
    assert len(rep["loops"]) == 1 and rep["loops"][0]["depth"] == 0
    assert rep["loops"][0]["all"]["reload"] == 1 and rep["loops"][0]["all"]["spill_write"] == 0 and rep["loops"][0]["all"]["valu"] == 3
    assert spill_audit.two_per_cu("l1_deflate_kernel<1024, 22976, 22976, true, true, true, true, true>")
    assert not spill_audit.two_per_cu("l1_deflate_kernel<1024, 32768, 32768, true, true, true, true, true>")
    assert not spill_audit.two_per_cu("l1_deflate_kernel<1024, 65536, 32768, false, false, false, false, true>")


def test_match_kernels_keep_their_register_budget():
    """Every two-per-CU instantiation of the match kernel (classes S .. SG2, plain and dictionary: 1024 threads, eight wavefronts per SIMD)
    stays within 64 VGPRs WITHOUT spilling a vector register — no scratch at all —, and in every match kernel no natural loop below the
    per-job loop carries SGPR spill traffic (a reload there is a vector instruction per trip in vector-issue-bound code).  A loop that
    cannot be made clean is pinned, with its reason, in tests/golden/spill_audit.json."""
    import spill_audit
    pin = json.load(open(os.path.join(ROOT, "tests", "golden", "spill_audit.json")))
    rep = spill_audit.audit(_library())
    match = {k: v for k, v in rep.items() if k.startswith("l1_deflate_kernel<")}
    two = {k: v for k, v in match.items() if spill_audit.two_per_cu(k)}
    assert len(match) >= 12 and len(two) == 8, sorted(match)        # six classes, four of them two per CU, plain and dictionary
    bad = []
    for k, v in sorted(two.items()):
        m = v["meta"]
        if m["vgpr_spill_count"] != 0 or m["private_segment_fixed_size"] != 0 or m["vgpr_count"] > 64:
            bad.append((k, "vgpr", m["vgpr_count"], "vgpr spills", m["vgpr_spill_count"], "scratch bytes", m["private_segment_fixed_size"]))
        if v["total"]["scratch_ld"] or v["total"]["scratch_st"]:
            bad.append((k, "scratch instructions", v["total"]["scratch_ld"], v["total"]["scratch_st"]))
    for k, v in sorted(match.items()):
        outer = [l for l in v["loops"] if l["depth"] == 0]
        assert outer and max(l["all"]["instructions"] for l in outer) > v["total"]["instructions"] // 2, (k, "per-job loop not found")
        dirty = [l for l in v["loops"] if l["depth"] >= 1 and (l["all"]["reload"] or l["all"]["spill_write"])]
        fam = [p for p in pin["allowed"] if k == p or (p.endswith("<") and k.startswith(p))]
        allowed = max([pin["allowed"][p]["loops"] for p in fam] or [0])
        if len(dirty) > allowed:
            bad.append((k, "loops with spill traffic", [(hex(l["header"]), l["all"]["reload"], l["all"]["spill_write"]) for l in dirty], "pinned: %d" % allowed))
    assert not bad, bad
