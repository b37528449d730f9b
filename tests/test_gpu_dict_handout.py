"""GPU: the hand-out list of the DICTIONARY DEFLATE jobs of the LDS classes, built by one pass over the chunk positions from the ranks the
ordered sort left in the match-distance array.  A list with a missing, doubled or foreign entry, a rank read from a
slot that holds none, or a hinted position written wrongly changes a record, so every stream is held byte for byte against the CPU oracle
and inflated through stock zlib; the check build of the library (libhmse_hip_dflcheck.so) also counts, job by job, the list's classes over
the sorted ranks as the two passes did and compares, in a child process.  What each group is for: tests/dict_handout_inputs.py; that the
inputs are what they claim to be: tests/test_dict_handout_host.py."""
import os
import subprocess
import sys

import pytest

import dict_handout_inputs as H
import handout_inputs as HP
from test_gpu_edges import run_jobs
from test_gpu_handout_in_sort import max_chain_depth

pytestmark = pytest.mark.gpu

GROUPS = ("contents", "lengths", "caps", "long_dictionary")


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def groups():
    return H.groups()


@pytest.mark.parametrize("name", GROUPS)
def test_streams_equal_the_oracles(name, groups, orc, dev):
    from hmse_amd import IngestConfig
    kinds = run_jobs(orc, dev, groups[name], IngestConfig(), name)
    if name == "caps":
        assert (kinds == 2).all()     # near-duplicates: every record is the dictionary job's


@pytest.mark.parametrize("which", range(7), ids=["level1", "depth3", "depth4", "depth12", "depth24", "default", "deepest"])
def test_depths_on_and_beside_the_class_thresholds(which, orc, dev):
    name, cfg = HP.depth_cfgs(max_chain_depth())[which]
    run_jobs(orc, dev, H.depth_job(), cfg, name)


def test_class_counts_equal_those_of_the_pass_over_the_ranks_in_the_check_build():
    """Every job above again, in a child process that loads the check build: a class of the list whose size differs from the count over
    the sorted ranks raises status bit 5 and the call fails — also where the stream would have survived it."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HMSE_LIB_VARIANT="dflcheck")
    r = subprocess.run([sys.executable, os.path.join(here, "dict_handout_check.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "dictionary hand-out lists OK" in r.stdout
