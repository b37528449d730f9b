"""GPU: the matcher's hand-out list written by the ordered sort (plain DEFLATE jobs of classes S and S2).  A list
with a missing, doubled or misplaced entry leaves positions unmatched or matched with the wrong candidate count, so every record is held
byte for byte against the CPU oracle and inflated through stock zlib; the check build of the library (libhmse_hip_dflcheck.so) also
compares, job by job, the entries the sort appended per class with the totals taken from the bucket sizes, in a child process.

  lengths    nh = 0, 1, 4; on and around one scatter step (1024 positions) and two; both class caps and one byte either side
  contents   one repeated byte (one bucket, all four classes), random (lists nearly empty), periods 5 and 7 (a few buckets of
             hundreds of members), text
  depths     2 (level 1), 3, 4, 12, 24 (on and beside the class thresholds 4 / 12 / 24), 32, and the largest accepted one
"""
import os
import subprocess
import sys

import pytest

import handout_inputs as H
from test_gpu_edges import run_jobs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def max_chain_depth() -> int:
    """The largest chain_depth hmse_cfg_validate accepts (the accepted depths are 1 .. max)."""
    from hmse_amd import IngestConfig, ops
    ok = lambda d: ops._host("hmse_cfg_validate", cfg=IngestConfig(chain_depth=d)) == 0
    lo, hi = 1, 1 << 24
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


@pytest.mark.parametrize("kind", H.CONTENTS)
def test_lengths_around_the_scatter_steps_and_the_class_caps(kind, orc, dev):
    from hmse_amd import IngestConfig
    run_jobs(orc, dev, H.plain_jobs(H.LENGTHS, (kind,)), IngestConfig(), kind)


@pytest.mark.parametrize("which", range(7), ids=["level1", "depth3", "depth4", "depth12", "depth24", "default", "deepest"])
def test_depths_on_and_beside_the_class_thresholds(which, orc, dev):
    deepest = max_chain_depth()
    name, cfg = H.depth_cfgs(deepest)[which]
    if which == 6:
        print("largest accepted chain_depth:", deepest, "(above 62: saturated counts, recomputed at the pull)" if deepest > 62 else "")
    run_jobs(orc, dev, H.plain_jobs(H.DEPTH_LENGTHS), cfg, name)


def test_entry_counts_equal_the_class_totals_in_the_check_build():
    """Every job above again, in a child process that loads the check build: a class whose appended entries differ from its total raises
    status bit 5 and the call fails — also where the stream would have survived the hole."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HMSE_LIB_VARIANT="dflcheck")
    r = subprocess.run([sys.executable, os.path.join(here, "handout_check.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "hand-out lists OK" in r.stdout
