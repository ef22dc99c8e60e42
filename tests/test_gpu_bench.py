"""-m gpu: a plain run of bench.py at a small size -- --steps sets the number of timed steps, the result line carries
ms_per_step, and --dump-outputs writes what the last timed step computed: what the pipeline returns for the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from world_class_amd.synth import make_utterance

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_what_the_last_timed_step_computed(tmp_path):
    out_dir = tmp_path / "out"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--utts", "3", "--distinct", "2",
           "--seconds", "1.0", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert abs(out["value"] - out["config"]["frames_per_gpu"] / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    assert out["roofline"] is None and not {"stages", "with_transfers", "cpu_baseline"} & set(out)  # (those are --full's)

    import world_class_amd as w
    w.lib().wc_set_device(0)
    xs = [make_utterance(48000, 1.0, 3000 + i % 2) for i in range(3)]  # bench.py's workload: seed 3000 + i % distinct
    want = w.Pipeline(48000).run_batch(xs)
    cat = {k: np.concatenate([o[k] for o in want]) for k in ("tpos", "f0", "sp", "ap", "y")}
    got = {f[:-4]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert set(got) == {"tpos", "f0", "sp_rowsum", "ap_rowsum", "sp_rows", "ap_rows", "y"}
    assert all(v.dtype == np.float64 for v in got.values())
    # a batch this small is below every sampling limit: every frame, row and sample, in order
    assert np.array_equal(got["tpos"], cat["tpos"]) and np.array_equal(got["f0"], cat["f0"])
    assert np.array_equal(got["sp_rows"], cat["sp"]) and np.array_equal(got["ap_rows"], cat["ap"])
    assert np.allclose(got["sp_rowsum"], cat["sp"].sum(1), rtol=1e-12, atol=0) and np.allclose(got["ap_rowsum"], cat["ap"].sum(1), rtol=1e-12, atol=0)
    assert got["y"].shape == cat["y"].shape and np.abs(got["y"] - cat["y"]).max() < 1e-12
