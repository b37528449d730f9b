"""Two launches of crc32_kernel (64 MiB in ranges of 8192 bytes) for a counters-only run:
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --output-format csv -- python tools/export_pmc.py
(A) data of one byte value — what it does to the table lookups depends on the register, not on the byte: the lanes of full strips hold
equal registers, so their lookups are broadcasts; (B) random data: every lookup of a wavefront is 64 random entries of a 256-entry table.
The two dispatches of crc32_kernel in the CSV are A and B, in that order."""
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hmse_amd import ops
dev = torch.device("cuda:0")
n = 64 << 20
rng = np.random.default_rng(1)
cuts = torch.arange(0, n + 1, 8192, dtype=torch.int64, device=dev)
for name, raw in (("A", np.full(n, ord("a"), np.uint8)), ("B", rng.integers(0, 256, n, dtype=np.uint8))):
    crc = ops.crc32(torch.from_numpy(raw).to(dev), cuts)
    torch.cuda.synchronize()
    print(name, hex(int(crc[0]) & 0xFFFFFFFF), hex(zlib.crc32(raw[:8192].tobytes())), flush=True)
