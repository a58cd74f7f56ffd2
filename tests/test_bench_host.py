"""bench.py's host-side pieces that need no GPU: the CPU baseline (the reference's
fp32 CPU forward at a given batch, 1 warm-up + timed iterations, CPU model recorded) and the
int8-fused floors it reports beside the roofline, its options; and one small plain run on the GPU
(result line, --steps, --dump-outputs)."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def test_cpu_baseline_shape_and_fields():
    import bench
    r = bench.cpu_baseline("resnet18", "r18_u8", 2, iters=1)
    assert r["unit"] == "images/s" and r["kind"] == "port" and r["value"] > 0
    assert r["cores"] >= 1 and r["cpu_model"] and "batch 2" in r["sample"] and "1 warm-up" in r["sample"]


def test_int8_fused_floors_match_baseline_md():
    import bench
    # BASELINE.md 3, int8-fused bound column
    assert bench.INT8_FUSED_FLOOR_MS == {"r50_mixed": (256, 0.666), "r18_u8": (256, 0.179), "r34_4bit": (512, 0.742)}
    assert set(bench.INT8_FUSED_FLOOR_MS) == set(bench.CONFIGS)


def test_plain_run_options(monkeypatch, capsys):
    """--full and --dump-outputs exist; what only a --full run produces (--layers) is refused
    without it, before anything touches a GPU."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--help"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--full" in out and "--dump-outputs DIR" in out
    for argv in (["--layers"], ["--steps", "0"]):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        with pytest.raises(SystemExit) as e:
            bench.main()
        assert e.value.code == 2


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_its_outputs(gpu, tmp_path):
    """A plain run (small config, in a child process as it is used): the result line holds the
    headline fields and no --full section, --steps sets the timed steps, and --dump-outputs writes
    the last step's logits, identical from run to run."""
    import json
    import subprocess
    import numpy as np
    outs = []
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
               "--config", "r18_u8", "--batch", "8", "--dump-outputs", str(tmp_path / d)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, p.stdout
        r = json.loads(lines[0])
        assert r["steps"] == 3 and r["warmup"] == 2 and r["full"] is False
        assert r["unit"] == "images/s" and r["higher_is_better"] is True and r["dtype"] == "i8"
        assert r["ms_per_step"] > 0 and abs(r["value"] * r["ms_per_step"] * 1e-3 / 8 - 1) < 1e-3
        assert "roofline" not in r and "cpu_baseline" not in r
        assert os.listdir(tmp_path / d) == ["logits.npy"]
        y = np.load(tmp_path / d / "logits.npy")
        assert y.shape == (8, 1000) and y.dtype == np.float32 and np.isfinite(y).all() and np.abs(y).max() > 0
        outs.append(y)
    assert np.array_equal(outs[0], outs[1])
