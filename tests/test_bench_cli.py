"""bench.py's command line: a plain run is lean (no CPU baseline without --full), --steps sets the timed steps, --dump-outputs writes
what the last timed step computed as .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_helpers_and_step_count_check(tmp_path):
    """step_outputs on a CPU model: the step's scalars in float64, ids in float32, the variables whole when they fit the sample size;
    the same call gives the same arrays; write_outputs writes DIR/<name>.npy.  --steps 0 is refused before anything runs."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from s2vt_amd import model as M
    m = M.Video_Caption_Generator(24, 50, 8, 16, 2, 8, 3, 5, device="cpu")
    st = M.StepStats(torch.tensor(1.5), torch.tensor([2.0]), torch.tensor(3.0))
    st.samples = torch.randint(0, 50, (4, 5), dtype=torch.int32)
    st.greedy = torch.randint(0, 50, (2, 5), dtype=torch.int32)
    st.attr_loss = None
    a, b = bench.step_outputs(st, m, {}), bench.step_outputs(st, m, {})
    assert set(a) == {"loss", "grad_sumsq", "mask_sum", "sampled_ids", "greedy_ids", "params_sample"}
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert a["loss"].dtype == np.float64 and float(a["loss"][0]) == 1.5 and float(a["mask_sum"][0]) == 3.0
    assert a["sampled_ids"].dtype == np.float32 and np.array_equal(a["sampled_ids"], st.samples.numpy())
    assert np.array_equal(a["params_sample"], m.store.theta.numpy())          # small buffer: all of it
    bench.write_outputs(str(tmp_path / "out"), a)
    assert sorted(os.listdir(tmp_path / "out")) == sorted(k + ".npy" for k in a)
    assert np.array_equal(np.load(tmp_path / "out" / "greedy_ids.npy"), a["greedy_ids"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path):
    """`bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs DIR`: one line with the headline keys, exactly the steps asked for, no CPU
    baseline (that is --full's), and the last step's ids, scalars and variable sample as finite arrays within 64 MB."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0 and out["unit"] == "tokens/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f32" and "cpu_baseline" not in out
    arrs = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert set(arrs) == {"loss", "grad_sumsq", "mask_sum", "sampled_ids", "greedy_ids", "params_sample"}
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrs.values())
    assert arrs["sampled_ids"].shape == (5 * 64, 20) and arrs["greedy_ids"].shape == (64, 20) and arrs["params_sample"].shape == (1 << 20,)
    assert float(arrs["loss"][0]) == pytest.approx(out["config"]["loss"], rel=1e-6)
