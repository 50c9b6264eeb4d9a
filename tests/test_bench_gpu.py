"""GPU: the single-GPU bench line as the driver runs it (a fresh child process, never an exec from this one).  `--full`: ONE JSON line that carries the headline
with `roofline` and -- measured in the same invocation, each in a child process of its own -- BASELINE.json's other single-GPU configurations under
`other_configs`: configs[1] (1 000 landmarks, unknown correspondence, the device-resident measure loop) and the whole configs[4] workload on one GPU
(40 000 -> 50 000 landmarks, float tiles, the pass in F32 arithmetic and in split arithmetic).  Short legs here (the figures to quote come from the default run); no CPU baseline.
A plain run: the headline alone, exactly K timed steps once, and with --dump-outputs the state its last timed step left."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_bench_line_carries_the_other_single_gpu_configurations():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "64", "--warmup", "16", "--deferred-steps", "80",
                        "--no-cpu-baseline"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    b = json.loads(lines[0])
    assert b["n_gpus"] == 1 and b["unit"] == "update-steps/s" and b["value"] > 0 and b["config"]["state_finite"]
    assert b["roofline"]["bound"] == "hbm" and 0.5 < b["roofline"]["frac"] < 1.0 and "k_downdate_w" in b["roofline"]["kernel"]
    # a timed region under 0.2 s: the block is repeated, the median quoted, and the line says so
    assert "note" in b["config"] and b["repeats"] >= 3 and b["repeats"] % 2 == 1
    assert b["ms_per_step_min"] <= b["ms_per_step"] <= b["ms_per_step_max"]
    assert b["deferred"]["deferred_batch"] == 20 and b["deferred_b32"]["deferred_batch"] == 32
    oc = b["other_configs"]
    c1, c4 = oc["configs[1]"], oc["configs[4] on one GPU"]
    assert "error" not in c1 and "error" not in c4, oc
    assert c1["value"] > 5e4 and c1["config"]["state_finite"] and "device-resident loop" in c1["config"]["device_association"]
    assert c4["value"] > 1e3 and c4["config"]["state_finite"] and c4["roofline"]["kernel"].startswith("k_flush_strip32<")
    r4 = c4["roofline"]
    assert r4["bound"] in ("hbm", "mfma") and r4["frac"] == max(r4["roofs"]["hbm"]["frac"], r4["roofs"]["mfma"]["frac"])
    assert r4["pairs_per_launch"] == 64 and 0.3 < r4["roofs"]["hbm"]["frac"] < 1.0 and 0.4 < r4["roofs"]["mfma"]["frac"] < 1.0
    assert c4["steps"] == 9936 and "50000 landmarks" in c4["config"]["workload"]
    # the same workload with the pass in split arithmetic: bound by HBM, and faster than the F32-arithmetic leg
    c4s = oc["configs[4] on one GPU, split arithmetic"]
    assert "error" not in c4s, oc
    r4s = c4s["roofline"]
    assert c4s["config"]["state_finite"] and r4s["kernel"] == "k_flush_split3<2>" and r4s["pairs_per_launch"] == 64
    assert r4s["bound"] == "hbm" and r4s["roofs"]["mfma"]["executed_over_algorithmic_flops"] == 6.0 and r4s["roofs"]["mfma"]["peak"] == 2500.0
    assert c4s["steps"] == 9936 and c4s["value"] > 1.1 * c4["value"]
    # both once more with the pass beside the next batch's appends and corrections (cfg.async_flush): present, finite, not slower than 0.9 x
    for key, syn in (("configs[4] on one GPU, asynchronous pass", c4), ("configs[4] on one GPU, split arithmetic, asynchronous pass", c4s)):
        ca = oc[key]
        assert "error" not in ca, oc
        assert ca["config"]["async_flush"] and ca["config"]["state_finite"] and ca["steps"] == 9936 and ca["value"] > 0.9 * syn["value"]


def test_plain_bench_line_is_the_headline_alone_and_dumps_the_last_state(tmp_path):
    """No --full: the headline leg only, its K timed steps timed once; --dump-outputs writes what the timed path's last step left
    (float64, under 64 MB), and that is what the same W + K steps give through the plain methods, bit for bit."""
    N, K, W = 1000, 40, 8
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--landmarks", str(N), "--steps", str(K), "--warmup", str(W),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    b = json.loads(lines[0])
    assert b["steps"] == K and b["warmup"] == W and b["repeats"] == 1 and b["ms_per_step"] > 0 and b["value"] > 0
    assert b["unit"] == "update-steps/s" and b["higher_is_better"] and b["dtype"] == "f64" and b["config"]["state_finite"]
    for key in ("deferred", "deferred_b32", "cpu_baseline", "cpu_baselines", "other_configs", "breakdown_us_per_step"):
        assert key not in b, key
    got = {p.name: np.load(p) for p in out.iterdir()}
    assert set(got) == {"x.npy", "P_digest.npy", "P_diag_blocks.npy", "P_rows.npy"}
    assert all(a.dtype == np.float64 for a in got.values()) and sum(a.nbytes for a in got.values()) <= 64 << 20
    np.testing.assert_array_equal(got["P_digest.npy"], np.array(b["config"]["state_digest"]))

    sys.path.insert(0, ROOT)
    import bench
    from ekf_slam_amd import Engine
    n = 3 + 2 * N
    w, x, s, d, U = bench.make_state(N, 20260101 + 3)
    e = Engine(mode="known", capacity=N, tile=128, batch=1)
    e.load_lowrank_state(x, s, d, U)
    for (u, z, R, k) in bench.make_steps(w, N, W + K, [.01, 5.0]):
        e.predict(u); e.correct(z, R, k)
    np.testing.assert_array_equal(got["x.npy"], e.get_x())
    np.testing.assert_array_equal(got["P_diag_blocks.npy"], e.get_P_diag_blocks())
    np.testing.assert_array_equal(got["P_rows.npy"], e.get_P()[bench.dump_rows(n)])
    np.testing.assert_array_equal(got["P_digest.npy"], e.digest())
    e.close()
