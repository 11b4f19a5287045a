"""bench.py's plain run on a reduced C3 frame: --steps sets the number of timed frames, the line
carries ms_per_step, the CPU baseline and `parity` stay behind --full, and --dump-outputs writes
the last timed frame, colour and depth, bit-identical to a single render of the same scene."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rt_amd as R
from cases import compare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_timed_frame(gpu, tmp_path):
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--width", "100", "--height", "54", "--spp", "6", "--dump-outputs", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0.0
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["cpu_baseline"] is None and line["parity"] is None  # --full only
    sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 10_000, width=100, height=54, spp=6)
    g, gd, gst = R.render(sc)
    assert line["rays_per_step"] == gst["segments"]  # the counters cover exactly the 3 timed frames
    # Mrays/s = rays of the timed frames / their time (both figures are rounded to 3 decimals in the
    # line: 0.0005 ms of a frame of 0.1 ms or more is within 1%)
    assert line["ms_per_step"] >= 0.1
    assert line["value"] == pytest.approx(gst["segments"] / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    assert sorted(os.listdir(out)) == ["depth.npy", "rgba.npy"]
    rgba, depth = np.load(os.path.join(out, "rgba.npy")), np.load(os.path.join(out, "depth.npy"))
    assert rgba.dtype == np.float32 and rgba.shape == (54, 100, 4)
    assert depth.dtype == np.float32 and depth.shape == (54, 100)
    assert compare(rgba, g)["exact_frac"] == 1.0
    assert compare(depth, gd)["exact_frac"] == 1.0
