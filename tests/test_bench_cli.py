"""bench.py's command line: the plain run (headline only, --dump-outputs) and --full (every other block)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "kernel_ms_per_step", "latency", "ingest", "cpu_baseline", "cpu_baseline_cpu_share",
             "parity_vs_ref", "feature_masks", "pose_rmse_vs_ref", "exact_voxel_order")


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_defaults_leave_everything_else_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.profile, a.dump_outputs) == (7, 2, False, "off", None)
    a = _parse(monkeypatch, "--full")
    assert a.full and a.profile == "all"
    a = _parse(monkeypatch, "--full", "--profile", "off", "--dump-outputs", "d")
    assert a.profile == "off" and a.dump_outputs == "d"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--profile", "dominant"]])
def test_parse_rejects(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, *argv)


def test_dump_outputs_writes_float_arrays(tmp_path):
    import bench
    from feature_base_pointcloud_registration_amd.fbr_types import REG_STATS, REG_STATS_FIELDS
    poses = np.arange(18, dtype=np.float32).reshape(3, 6) / 7
    stats = np.zeros(3, REG_STATS)
    for i, f in enumerate(REG_STATS_FIELDS):
        stats[f] = [i, 2 * i, -i]
    d = tmp_path / "a" / "b"  # created on demand
    bench.dump_outputs(str(d), poses, stats)
    assert sorted(os.listdir(d)) == sorted(["poses.npy"] + [f"stats_{f}.npy" for f in REG_STATS_FIELDS])
    p = np.load(d / "poses.npy")
    assert p.dtype == np.float32 and np.array_equal(p, poses)
    for i, f in enumerate(REG_STATS_FIELDS):
        s = np.load(d / f"stats_{f}.npy")
        assert s.dtype == np.float64 and s.tolist() == [i, 2 * i, -i]


def _bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *argv], capture_output=True, text=True,
                       timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_steps_results(tmp_path):
    """A plain run carries the headline and none of the --full blocks; --dump-outputs holds what
    fbr_batch_results returns for the same seeded jobs, bit for bit."""
    from feature_base_pointcloud_registration_amd import api, synth
    d = tmp_path / "out"
    res = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "C1", "--batch", "8",
                 "--dump-outputs", str(d))
    assert all(k in res for k in HEADLINE) and not any(k in res for k in FULL_ONLY)
    assert res["steps"] == 3 and res["warmup"] == 1 and res["unit"] == "scans/s" and res["dtype"] == "f32"
    assert res["higher_is_better"] is True and res["registration_status_ok"] == 8
    assert res["value"] == pytest.approx(8 * 1000.0 / res["ms_per_step"], rel=1e-3)
    jobs = synth.make_jobs("C1", 8, base_seed=1000)
    with api.Context(synth.config_params("C1", max_batch=8)) as ctx:
        ctx.set_map(*synth.config_map("C1"))
        ctx.batch_stage([j[0] for j in jobs], np.stack([j[1] for j in jobs]).astype(np.float32))
        ctx.batch_launch()
        ctx.batch_wait()
        poses, stats = ctx.batch_results()
    got = np.load(d / "poses.npy")
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), poses.view(np.int32))
    for f in stats.dtype.names:
        assert np.array_equal(np.load(d / f"stats_{f}.npy"), stats[f].astype(np.float64)), f


@pytest.mark.gpu
def test_full_run_carries_every_other_block():
    res = _bench("--full", "--gpus", "1", "--steps", "2", "--warmup", "1", "--config", "C1", "--batch", "8",
                 "--cpu-sample", "4", "--latency", "10", "--ingest", "1")
    assert all(k in res for k in HEADLINE + FULL_ONLY)
    assert res["parity_vs_ref"]["n"] == 4 and res["feature_masks"]["mask_bit_equal"] == 4
    assert res["roofline"]["kernel"] in res["roofline"]["kernels"]
