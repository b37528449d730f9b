"""GPU: hmse_l1_deflate on the inputs of tests/encoder_shapes.py — the Kraft repair of each of the three trees, every remainder class of the
closed-form code-length RLE, distance trees with dummy symbols, the ends of nlit / ndist / ncl, block types tied in bits and tokens whose put
touches three dwords of the bit image — against the CPU oracle, byte for byte: one call per configuration with every case in it.  What each
case reaches is asserted on the CPU (tests/test_encoder_shapes_host.py); the witnesses hold at the default configuration, level 1 and a
chain depth of 200 are parity only.  tests/enc_spill_check.py runs the same selection through the forced spill path."""
import zlib
from dataclasses import replace

import numpy as np
import pytest

import encoder_shapes as es
from test_gpu_parity import dev, ocfg, to_dev  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("change", [dict(), dict(level=1), dict(chain_depth=200)], ids=["default", "level-1", "chain-depth-200"])
def test_encoder_shapes_equal_the_oracle(orc, dev, change):
    from hmse_amd import IngestConfig, ops
    cfg = replace(IngestConfig(), **change)
    data, cuts, base, names = es.batch()
    assert data.size < 2 << 20
    want_out, want_off, want_kind = orc.deflate_chunks(data, cuts, ocfg(orc, cfg), None, base)
    out, off, kind = ops.l1_deflate(to_dev(data, dev), to_dev(cuts.astype(np.int64), dev), cfg, None, to_dev(base, dev))
    off, kind, out = off.cpu().numpy().astype(np.uint64), kind.cpu().numpy(), out.cpu().numpy()
    sizes = lambda o: dict(zip(names, np.diff(o.astype(np.int64)).tolist()))
    assert np.array_equal(off, want_off), [(n, s, sizes(want_off)[n]) for n, s in sizes(off).items() if s != sizes(want_off)[n]][:10]
    assert np.array_equal(kind, want_kind), [n for n, a, b in zip(names, kind, want_kind) if a != b]
    wrong = [n for k, n in enumerate(names) if not np.array_equal(out[int(off[k]):int(off[k + 1])], want_out[int(off[k]):int(off[k + 1])])]
    assert not wrong and np.array_equal(out, want_out), wrong
    for k, name in enumerate(names):
        raw = data[int(cuts[k]):int(cuts[k + 1])].tobytes()
        zd = data[int(cuts[base[k]]):int(cuts[base[k] + 1])].tobytes() if kind[k] == 2 else None
        d = zlib.decompressobj(-15, zdict=zd) if zd else zlib.decompressobj(-15)
        assert d.decompress(out[int(off[k]):int(off[k + 1])].tobytes()) == raw and d.eof, name
    if not change:
        # the witnesses are about these very streams: the dictionary jobs built for a tree's repair are kept as DELTA records, and every
        # record is the stream whose block type and length the witness predicts
        at = {n: k for k, n in enumerate(names)}
        for name, w in es.witnesses().items():
            k, zdict = at[name], es.cases()[name][1]
            assert kind[k] == (2 if zdict else 0), name
            assert ((int(out[int(off[k])]) >> 1) & 3, int(off[k + 1] - off[k])) == (w["block"], w["stream_len"]), name
        assert kind[at["w1-litlen-depth-16"]] == kind[at["w2-dist-depth-16"]] == 2
