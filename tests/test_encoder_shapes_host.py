"""CPU: every input of tests/encoder_shapes.py reaches the branch of the encoder's Huffman stage it was built for (asserted from the
witness, which uses oracle/pyref.py only), and on every one of them the two restatements of the encoder — oracle/hmse_oracle_deflate.c
and oracle/pyref.py — agree byte for byte, stock zlib inflates the stream, and the witness's restated costs predict its block type
and length.  No GPU."""
import zlib

import pytest

import encoder_shapes as es
from oracle import pyref

W = es.witnesses
NAMES = list(es.cases())


def dynamic(*names):
    ws = [W()[n] for n in names]
    assert all(w["block"] == 2 for w in ws), [(n, w["block"]) for n, w in zip(names, ws)]
    return ws if len(ws) > 1 else ws[0]


def used(freq):
    return [s for s, f in enumerate(freq) if f]


def inflate(stream, zdict):
    d = zlib.decompressobj(-15, zdict=zdict) if zdict else zlib.decompressobj(-15)
    raw = d.decompress(stream)
    assert d.eof and not d.unused_data
    return raw


@pytest.mark.parametrize("name", NAMES)
def test_both_restatements_agree_and_the_witness_predicts_the_stream(orc, name):
    chunk, zdict = es.cases()[name]
    w = W()[name]
    got = pyref.deflate(chunk, zdict or b"")
    assert orc.deflate(chunk, orc.default_cfg(), zdict) == got
    assert inflate(got, zdict) == chunk
    assert ((got[0] >> 1) & 3, len(got)) == (w["block"], w["stream_len"])


def test_w1_literal_length_tree_deeper_than_15():
    w = dynamic("w1-litlen-depth-16")
    assert sorted(f for f in w["lf"] if f) == sorted(es.FIB17) and used(w["lf"])[0] == 256       # no stray literal: lengths and EOB only
    assert w["depth"][0] == 16 and max(w["ll"]) == 15 and w["repairs"][0] == 1
    assert w["tokens"] == w["matches"] == 4179 and len(es.cases()["w1-litlen-depth-16"][0]) == 23700


def test_w2_distance_tree_deeper_than_15():
    w = dynamic("w2-dist-depth-16")
    assert w["df"] == [0] * 13 + list(es.FIB17)
    assert w["depth"][1] == 16 and max(w["dl"]) == 15 and w["repairs"][1] == 1
    both = dynamic("w9-both-trees-deep")
    assert both["depth"][:2] == (12, 16) and both["repairs"][1] == 1


def test_w3_code_length_tree_deeper_than_7_in_both_encode_lists():
    for name, depth, longer in (("w3-cl-depth-8", 8, False), ("w3-cl-depth-8-long", 8, True), ("w3-cl-depth-9", 9, False), ("w3-cl-depth-9-long", 9, True)):
        w = dynamic(name)
        assert w["depth"][2] == depth and max(w["cl"]) == 7 and w["matches"] == 0, name
        assert sorted(f for f in w["cf"] if f) == list(es.FIB17[:depth + 1]), name
        assert (len(es.cases()[name][0]) > 12288) == longer                      # l1_encode_kernel<0, 12288> | <12288, 32768>


def test_w4_the_repair_loop_runs_once_and_twice():
    runs = {name: W()[name]["repairs"] for name in NAMES}
    assert runs["w1-litlen-depth-16"] == (1, 0, 0) and runs["w2-dist-depth-16"] == (0, 1, 0)
    assert runs["w3-cl-depth-8"] == runs["w3-cl-depth-8-long"] == (0, 0, 1)
    assert runs["w3-cl-depth-9"] == runs["w3-cl-depth-9-long"] == (0, 0, 2)
    # nothing else repairs: the cases above are the only ones that pin the loop
    assert all(not any(r) for n, r in runs.items() if n[:2] not in ("w1", "w2", "w3") and n != "w9-both-trees-deep")


def test_w5_distance_trees_with_fewer_than_two_used_codes():
    none, zero, five = dynamic("w7-rle-a", "w5-only-distance-code-0", "w5-one-distance-code-5")
    assert used(none["df"]) == [] and none["dl"][:2] == [1, 1] and none["ndist"] == 2          # dummies 0 and 1
    assert used(zero["df"]) == [0] and zero["dl"][:2] == [1, 1] and zero["ndist"] == 2         # dummy 1
    assert used(five["df"]) == [5] and five["dl"][:6] == [1, 0, 0, 0, 0, 1] and five["ndist"] == 6   # dummy 0
    assert five["matches"] == 1


def test_w6_header_ends():
    assert dynamic("w7-rle-a")["nlit"] == 257
    assert dynamic("w5-only-distance-code-0")["nlit"] == 286
    assert dynamic("w1-litlen-depth-16")["ndist"] == 30 and dynamic("w1-litlen-depth-16")["ncl"] == 19
    # the smallest ncl: a complete distance tree over at most 30 codes has a length of 4 or less, and 4 is the 12th in the header's order
    w = dynamic("w6-ncl-12")
    assert w["ncl"] == 12 == min(x["ncl"] for x in W().values() if x["block"] == 2)
    assert set(w["dl"][14:30]) == {4} and not {1, 2, 3, 12, 13, 14, 15} & set(w["ll"])


def test_w7_code_length_rle_coverage():
    ws = [w for w in W().values() if w["block"] == 2]
    runs = [r for w in ws for r in w["runs"]]
    zero = {n for _, _, v, n in runs if v == 0}
    other = {n for _, _, v, n in runs if v}
    assert {1, 2, 3, 10, 11, 138, 139, 140, 141, 148, 149} <= zero
    # the end-of-block code is always used, so no zero run is longer than 256 (a job without a literal): two full 18s never occur
    assert max(zero) == 256 and {1, 2, 3, 4, 6, 7, 8, 9, 10} <= other
    assert {n % 138 for n in zero if n >= 138} >= {0, 1, 2, 3, 10, 11} and {(n - 1) % 6 for n in other} == set(range(6))
    starts = {(i, v != 0) for t, i, v, n in runs if t == 0}
    assert {(63, False), (63, True), (64, False), (64, True)} <= starts
    for edge in (64, 128, 192, 256):
        assert edge == 256 or any(t == 0 and i < edge < i + n and v == 0 for t, i, v, n in runs), edge   # (256 is never zero)
        assert any(t == 0 and i < edge < i + n and v != 0 for t, i, v, n in runs), edge
    assert any(t == 0 and i == 257 and v == 0 for t, i, v, n in runs)                           # 257 (length 3) is never used
    # the tokens themselves, with the symbols the closed form has to pick
    toks = [t for w in ws for t in w["rle"]]
    assert {(s, ev) for _, _, s, _, ev in toks if s == 18} >= {(18, 0), (18, 127), (18, 138 - 11)} and any(s == 17 and ev == 7 for _, _, s, _, ev in toks)
    assert {ev for _, _, s, _, ev in toks if s == 16} == {0, 1, 2, 3} and {ev for _, _, s, _, ev in toks if s == 17} >= {0, 7}
    # the second call: a distance tree whose runs take 18, 16 and plain tokens behind a non-zero token base
    w2 = W()["w2-dist-depth-16"]
    dist = [(s, i) for t, i, s, _, _ in w2["rle"] if t == 1]
    assert w2["dist_token_base"] > 0 and dist[0] == (18, 0) and {16, 15} <= {s for s, _ in dist} and len(dist) >= 10


def test_w8_ties_in_bits():
    a, b, c = (W()[n] for n in ("w8-stored-eq-fixed", "w8-stored-eq-dynamic", "w8-fixed-eq-dynamic"))
    assert a["stored_bits"] == a["fixed_bits"] <= a["dyn_bits"] and a["block"] == 0
    assert b["stored_bits"] == b["dyn_bits"] < b["fixed_bits"] and b["block"] == 0
    assert c["fixed_bits"] == c["dyn_bits"] < c["stored_bits"] and c["block"] == 1


def test_w9_tokens_wider_than_a_dword():
    one, two, deep = dynamic("w9-wide-38", "w9-wide-36-twice", "w9-both-trees-deep")
    assert (one["widest_token"], one["three_dword_puts"]) == (38, 1)
    assert (two["widest_token"], two["three_dword_puts"]) == (36, 2)
    assert deep["widest_token"] == 34 and len(es.cases()["w9-both-trees-deep"][0]) > 12288     # wider than a dword in the second list too
