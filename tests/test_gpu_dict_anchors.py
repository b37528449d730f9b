"""GPU: the anchor phase of the DICTIONARY DEFLATE jobs in three stages (one lane per anchor finds the bucket's dictionary members, groups of
lanes choose the nearest one that agrees on 32 bytes, one wavefront per chosen anchor measures the runs).  A wrong
boundary, a member outside the 64 nearest, a farther member chosen before a nearer one, or a wrong run or backward extent changes a record
or is caught by the check build, so every stream is held byte for byte against the CPU oracle and inflated through stock zlib; the check
build of the library (libhmse_hip_dflcheck.so) also computes every anchor by the one-wavefront-per-anchor form and compares the words, in a
child process.  What each group is for: tests/anchor_inputs.py; that the inputs are what they claim to be:
tests/test_anchor_inputs_host.py."""
import os
import subprocess
import sys

import pytest

import anchor_inputs as A
from test_gpu_edges import run_jobs

pytestmark = pytest.mark.gpu

GROUPS = ("candidates", "buckets", "counts", "worst", "distance", "padding", "runs")


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def groups():
    return A.groups()


@pytest.mark.parametrize("name", GROUPS)
def test_streams_equal_the_oracles(name, groups, orc, dev):
    from hmse_amd import IngestConfig
    assert tuple(groups) == GROUPS
    kinds = run_jobs(orc, dev, groups[name], IngestConfig(), name)
    if name == "worst":
        assert (kinds == 2).all()     # copies of the dictionary: every record is the dictionary job's


def test_anchors_equal_those_of_one_wavefront_per_anchor_in_the_check_build():
    """Every job above again, in a child process that loads the check build: an anchor word or a backward extent that differs from the one
    the form without stages computes raises status bit 6 and the call fails — also where the stream would have survived it."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HMSE_LIB_VARIANT="dflcheck")
    r = subprocess.run([sys.executable, os.path.join(here, "dict_anchor_check.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "dictionary anchors OK" in r.stdout
