"""Run by tests/test_gpu_handout_in_sort.py in a child process with HMSE_LIB_VARIANT=dflcheck (the library is chosen once per process):
the DEFLATE match kernel of that build compares, behind every sort that wrote a hand-out list, the entries appended per class with the
class totals computed from the bucket sizes, and raises status bit 5 on a difference — ops.l1_deflate then fails.  Same jobs, same
comparison with the oracle and zlib as in the parent."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import oracle as orc   # noqa: E402  (test infrastructure)
from hmse_amd import IngestConfig, _lib   # noqa: E402
import handout_inputs as H   # noqa: E402
from test_gpu_edges import run_jobs   # noqa: E402
from test_gpu_handout_in_sort import max_chain_depth   # noqa: E402

assert os.environ.get("HMSE_LIB_VARIANT") == "dflcheck" and _lib.HIP_LIB_PATH.endswith("libhmse_hip_dflcheck.so")
orc.build()
dev = torch.device("cuda:0")
n = 0
job = H.plain_jobs(H.LENGTHS)
run_jobs(orc, dev, job, IngestConfig(), "lengths")
n += len(job["parts"])
job = H.plain_jobs(H.DEPTH_LENGTHS)
for name, cfg in H.depth_cfgs(max_chain_depth()):
    run_jobs(orc, dev, job, cfg, name)
    n += len(job["parts"])
print(f"hand-out lists OK: {n} jobs")
