"""Two count-only launches of approx_scan_kernel<8> (m = 16, k = 2, 64 MiB) for a counters-only run:
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --output-format csv -- python tools/approx_pmc.py
(A) a text of one byte value — every Peq lookup of a wavefront is one address, a broadcast, so what conflicts remain are the tile's;
(B) random text over 64 byte values.  The two dispatches of approx_scan_kernel<8> in the CSV are A and B, in that order."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hmse_amd import ops
dev = torch.device("cuda:0")
n = 64 << 20
rng = np.random.default_rng(1)
pats = [bytes(rng.integers(48, 112, 16, dtype=np.uint8)) for _ in range(8)]
pat = torch.from_numpy(np.frombuffer(b"".join(pats), np.uint8).copy()).to(dev)
off = [16 * i for i in range(9)]
ro = torch.tensor([0, n], dtype=torch.int64, device=dev)
for name, raw in (("A", np.full(n, ord("a"), np.uint8)), ("B", rng.integers(48, 112, n, dtype=np.uint8))):
    h, nh, c = ops.approx_scan(torch.from_numpy(raw).to(dev), ro, None, pat, off, [2] * 8, hits_cap=0)
    torch.cuda.synchronize()
    print(name, nh, c.tolist(), flush=True)
