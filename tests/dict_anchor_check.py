"""Run by tests/test_gpu_dict_anchors.py in a child process with HMSE_LIB_VARIANT=dflcheck (the library is chosen once per process): the
dictionary kernels of that build also compute every anchor the way one wavefront per anchor did — bucket search, exact common prefixes, the
longest-then-nearest key, the runs — and raise status bit 6 where an anchor word or a backward extent of the three stages differs;
ops.l1_deflate then fails.  Same jobs, same comparison with the oracle and zlib as in the parent."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import oracle as orc   # noqa: E402  (test infrastructure)
from hmse_amd import IngestConfig, _lib   # noqa: E402
import anchor_inputs as A   # noqa: E402
from test_gpu_edges import run_jobs   # noqa: E402

assert os.environ.get("HMSE_LIB_VARIANT") == "dflcheck" and _lib.HIP_LIB_PATH.endswith("libhmse_hip_dflcheck.so")
orc.build()
dev = torch.device("cuda:0")
n = 0
for name, job in A.groups().items():
    run_jobs(orc, dev, job, IngestConfig(), name)
    n += len(job["ids"])
print(f"dictionary anchors OK: {n} jobs")
