"""bench.py's two kinds of run: a plain run does what the headline figure needs and nothing else; the percentiles,
roofline, per-kernel table, config 3, data-parallel rehearsal and CPU baseline are behind --full."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernels", "kernel_us_per_step", "config3", "dp_world1", "cpu_baseline")


def check_headline(out, steps, warmup):
    for k in HEADLINE:
        assert k in out, k
    assert out["steps"] == steps and out["warmup"] == warmup
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["higher_is_better"] is True and out["dtype"] == "f32" and out["unit"] == "caption-tokens/s"
    assert out["config"]["final_loss"] > 0


def test_full_is_an_option():
    p = subprocess.run([sys.executable, BENCH, "--help"], stdout=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0
    assert "--full" in p.stdout


@pytest.mark.gpu
def test_plain_run_does_only_the_headline(monkeypatch, capsys):
    """In process, with every --full measurement replaced by one that fails: a plain run must not call them, nor build
    the config-3 model, and its line carries the headline fields and none of theirs."""
    import bench

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"a plain run called bench.{name}")
        return f
    for name in ("step_percentiles", "kernel_breakdown", "dp_world1_rehearsal", "cpu_baseline"):
        monkeypatch.setattr(bench, name, refuse(name))
    made, make_model = [], bench.make_model
    monkeypatch.setattr(bench, "make_model", lambda wl, *a, **k: made.append(wl) or make_model(wl, *a, **k))
    monkeypatch.setattr(sys, "argv", [BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1"])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert made == ["dense"]
    check_headline(out, 3, 1)
    for k in FULL_ONLY:
        assert k not in out, k
    assert "step_ms_p10_p50_p90" not in out["config"]


@pytest.mark.gpu
def test_full_run_reports_what_moved():
    """--full (without the data-parallel rehearsal, which starts three more processes) still reports the percentiles,
    the roofline and per-kernel table of both configs, config 3's timing and the CPU baseline."""
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "10", "--warmup", "2", "--full", "--no-dp-world1"],
                       stdout=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    check_headline(out, 10, 2)
    pct = out["config"]["step_ms_p10_p50_p90"]
    assert len(pct) == 3 and 0 < pct[0] <= pct[1] <= pct[2]
    assert out["roofline"]["frac"] > 0 and out["kernels"] and out["kernel_us_per_step"] > 0
    c3 = out["config3"]
    assert c3["steps"] == 10 and c3["ms_per_step"] > 0 and c3["value"] > 0 and c3["roofline"]["frac"] > 0 and c3["kernels"]
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["unit"] == "caption-tokens/s"
    assert "dp_world1" not in out
