"""Fixed small workload of the launch comparison (profiles/abi3/README.md): three 1 MiB batches through StreamIngest(graph=True), then three global batches through
stream_shards_local_gl4_graph at two emulated ranks.  Imports hmse_amd from the current directory (this tree, or the parent's copy)."""
import os, sys
sys.path.insert(0, os.getcwd())
import torch
from hmse_amd import IngestConfig, corpus, stream, stream_gl4
import hmse_amd
print("hmse_amd from", hmse_amd.__file__, flush=True)
MIB = 1 << 20
dev = torch.device("cuda:0")
cfg = IngestConfig(seg_size=MIB)
data = corpus.wiki_synth(3 * MIB, seed=23)
s = stream.StreamIngest(cfg, data.size, dev, graph=True)
for a in range(0, data.size, MIB):
    s.push(torch.from_numpy(data[a: a + MIB].copy()))
res = s.finish()
torch.cuda.synchronize()
print("one rank:", res.stats, flush=True)
d2 = corpus.wiki_synth(6 * MIB, seed=29)
d2[4 * MIB + 1000: 5 * MIB] = d2[1000: MIB]          # the last batch repeats bytes of the first: pointers and remote dictionaries
d2[4 * MIB + 5000: 5 * MIB: 1500] ^= 0x20
batches = [torch.from_numpy(d2[a: a + 2 * MIB].copy()) for a in range(0, d2.size, 2 * MIB)]
out = stream_gl4.stream_shards_local_gl4_graph(batches, cfg, 2, dev)
torch.cuda.synchronize()
print("two ranks:", [r.stats for r in out], flush=True)
