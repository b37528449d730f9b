"""GPU: a plain `bench.py` run times the steps it is asked for, prints the headline without the side measurements of --full,
and its --dump-outputs are the arrays the timed path returns for the same input."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_times_k_steps_and_dumps_what_the_step_returns(tmp_path):
    import torch
    import bench
    from hmse_amd import IngestConfig, corpus, ingest
    assert torch.cuda.is_available()
    nbytes = 64 << 20
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--bytes", str(nbytes),
                        "--dump-outputs", str(tmp_path / "bench")], capture_output=True, timeout=600)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stderr.decode()[-2000:])
    out = json.loads(lines[0])
    assert out["metric"] == "ingest_GiB_per_s" and out["unit"] == "GiB/s" and out["higher_is_better"] is True and out["dtype"] == "u8"
    assert out["steps"] == 3 and len(out["step_ms_host"]) == 3 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["config"]["total_bytes"] == nbytes
    assert not {"cpu_baseline", "stage_roofline", "roofline", "read_path", "manifest", "other_configs"} & set(out)
    host, _ = corpus.load("wikipedia", nbytes)
    res = ingest.ingest_shard(torch.from_numpy(host).to("cuda:0"), IngestConfig(), want_stats=False)
    bench.dump_outputs(res, str(tmp_path / "direct"))
    names = sorted(os.listdir(tmp_path / "direct"))
    assert names == sorted(os.listdir(tmp_path / "bench")) and {"cuts.npy", "digests.npy", "sig.npy", "streams.npy"} <= set(names)
    for n in names:
        assert np.array_equal(np.load(tmp_path / "bench" / n), np.load(tmp_path / "direct" / n)), n
