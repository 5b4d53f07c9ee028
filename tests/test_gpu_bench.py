"""bench.py end to end on the GPU: a plain run prints the one headline line (nothing that needs passes of its own), and
--dump-outputs writes what the last timed step computed — checked here against the oracle on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    import bench
    from oracle import fq_oracle as O
    out = tmp_path / "out"
    steps = 7
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                        "--dump-outputs", str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["unit"] == "Melem/s" and rec["higher_is_better"] is True and rec["dtype"] == "f16" and rec["metric"]
    assert rec["steps"] == steps and rec["warmup"] == 2 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert not {"roofline", "cpu_baseline", "strong", "c4"} & set(rec), sorted(rec)     # those come with --full

    q, s = np.load(out / "q_int4.npy"), np.load(out / "scales.npy")
    assert sorted(os.listdir(out)) == ["q_int4.npy", "scales.npy"]
    assert q.dtype == s.dtype == np.float32 and q.shape == (bench.DUMP_ROWS, bench.D) and s.shape == (bench.ROWS,)
    # the last timed step read input buffer (steps - 1) % N_BUF; the dump holds a seeded sample of its rows
    x = bench.make_inputs(torch.device("cuda", 0), seed=0)[(steps - 1) % bench.N_BUF].cpu().numpy()
    rows = torch.randperm(bench.ROWS, generator=torch.Generator().manual_seed(0))[:bench.DUMP_ROWS].sort().values.numpy()
    mats = bench.make_matrices("cpu")
    ref = O.kron_quant(x[rows], mats["left"].numpy(), mats["right"].numpy(), bench.SIG4, bench.SIG4, clamp0=False)
    flips = float(np.mean(q != ref["q"]))
    assert flips <= 1e-3 and np.max(np.abs(q - ref["q"])) <= 1, flips
    assert np.allclose(s[rows], ref["scale16"].astype(np.float32), rtol=2e-3, atol=0)
