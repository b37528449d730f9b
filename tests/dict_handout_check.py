"""Run by tests/test_gpu_dict_handout.py in a child process with HMSE_LIB_VARIANT=dflcheck (the library is chosen once per process): the
dictionary kernels of that build also count the hand-out list's four classes over the sorted ranks, the way the two passes over the ranks
classified them, and raise status bit 5 where a class of the list built from the chunk positions has another size — ops.l1_deflate then
fails.  Same jobs, same comparison with the oracle and zlib as in the parent."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import oracle as orc   # noqa: E402  (test infrastructure)
from hmse_amd import IngestConfig, _lib   # noqa: E402
import dict_handout_inputs as H   # noqa: E402
import handout_inputs as HP   # noqa: E402
from test_gpu_edges import run_jobs   # noqa: E402
from test_gpu_handout_in_sort import max_chain_depth   # noqa: E402

assert os.environ.get("HMSE_LIB_VARIANT") == "dflcheck" and _lib.HIP_LIB_PATH.endswith("libhmse_hip_dflcheck.so")
orc.build()
dev = torch.device("cuda:0")
n = 0
for name, job in H.groups().items():
    run_jobs(orc, dev, job, IngestConfig(), name)
    n += len(job["ids"])
job = H.depth_job()
for name, cfg in HP.depth_cfgs(max_chain_depth()):
    run_jobs(orc, dev, job, cfg, name)
    n += len(job["ids"])
print(f"dictionary hand-out lists OK: {n} jobs")
