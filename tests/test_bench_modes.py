"""bench.py's two kinds of run at N=1.  A plain run (the driver's `bench.py --gpus 1 --steps K --warmup W`) times the headline
and prints ONE JSON line; `--full` adds the measurements that take runs of their own and prints the full line, then the
compact one.  `--sections` only selects sub-objects of `--full`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--views", "3", "--workload", "c1_256x256_plumbing"]


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    return [l for l in p.stdout.splitlines() if l.startswith("{")]


def test_sections_need_full():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--sections", "train"], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 2 and "--full" in p.stderr, p.stderr[-2000:]


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone(hip_device, tmp_path):
    import bench
    lines = _bench(SMALL + ["--dump-outputs", str(tmp_path)])
    assert len(lines) == 1 and len(lines[0]) <= bench.HEADLINE_MAX_BYTES, lines
    d = json.loads(lines[0])
    assert d["unit"] == "views/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["n_gpus"] == 1
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] == pytest.approx(3 * 1e3 / d["ms_per_step"], rel=1e-9)
    assert d["metric"].startswith("rendered views/sec @ 256x256") and d["config"]["workload"] == "c1_256x256_plumbing"
    # the timed region's own roofline stays; nothing that needs extra steps, the CPU oracle or other workloads
    assert d["roofline"]["launches"] == 2 * 3 * len(d["timed_regions_ms"]) and "isolated_launch_ms" not in d["roofline"]
    for k in ("cpu_baseline", "parity", "hipgraph_replay", "kernel_ms_per_view", "roofline_valu", "fast_exp", "train", "c2"):
        assert k not in d, k
    assert set(d["dump_outputs"]) == {"color", "depth"}
    assert np.load(tmp_path / "color.npy").shape == (3, 3, 256, 256) and np.load(tmp_path / "depth.npy").shape == (3, 1, 256, 256)


@pytest.mark.gpu
def test_full_run_adds_the_extra_measurements(hip_device):
    lines = _bench(SMALL + ["--full", "--sections", "raster"])
    d, compact = json.loads(lines[-2]), json.loads(lines[-1])      # the full line, then the compact one the driver parses
    assert compact["value"] == pytest.approx(d["value"], rel=1e-4) and compact["cpu_baseline"]["kind"] == "port"
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["value"] > 0 and "max_abs_err_vs_oracle" in d["parity"]
    assert d["hipgraph_replay"]["same_image_as_eager"] is True and d["hipgraph_replay"]["value"] > 0
    assert d["kernel_ms_per_view"]["render"] > 0 and d["roofline"]["isolated_launch_ms"] > 0
