"""bench.py's plain run (no --full): the headline fields with every side field null, and --dump-outputs - the same arrays
from two runs with the same arguments, and they are what the last timed step's scene gives when it is run on its own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, SCENES = 6, 4            # the last timed step is k = 5: scene 5 % 4 = 1

# the last timed step's scene alone, in a fresh process, under the timed region's launch sizing and the dump writer of bench.py
ONE_SCENE = """
import sys
import torch
sys.path.insert(0, sys.argv[1])
import bench
from canonicalvoting_amd import dist as cvd, hv_cuda, me as ME, pipeline
from canonicalvoting_amd.hough import HoughVoting
from canonicalvoting_amd.minkunet import MinkUNet34C
steps, scenes, path = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
dev = torch.device("cuda", 0)
hv_cuda.set_algorithm(0)
ME.set_compute_dtype("fp32")
torch.manual_seed(0)
model = MinkUNet34C(3, 6 * 9 + 9 + 1).cuda().eval()
s = bench.ResidentScene(cvd.scene_seeds(0, scenes)[(steps - 1) % scenes], bench.N_POINTS, dev)
bench.POLICY = pipeline.policy_for_scenes_in_flight(bench.scene_threads(7))
out = {}
dets, raw = bench.run_step(model, HoughVoting(bench.RES, bench.NUM_ROTS), s, teacher=True, out=out)
torch.cuda.synchronize()
out.update(dets=dets, raw=raw)
bench.dump_outputs(path, out)
"""


def _bench(out):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "2",
                        "--scenes", str(SCENES), "--min-warm-seconds", "0", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {p.name: np.load(p) for p in d.iterdir()}


def test_plain_run_prints_the_headline_and_dumps_the_last_step(cuda, built_lib, tmp_path):
    line = _bench(tmp_path / "a")
    assert line["steps"] == STEPS and line["full"] is False and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "scenes/s"
    for k in ("cpu_baseline", "parity", "parity_one_in_flight", "train_step_ms", "steady_state", "stage_ms_isolated",
              "roofline", "roofline_conv", "in_flight_counters"):
        assert line[k] is None, k
    a = _load(tmp_path / "a")
    assert {"det_class.npy", "det_box.npy", "det_score.npy", "raw_boxes.npy", "raw_scores.npy", "raw_classes.npy",
            "raw_cand_idx.npy", "raw_verdict.npy", "y.npy"} == set(a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["y.npy"].shape == (80000, 64) and np.isfinite(a["y.npy"]).all()
    n = len(a["det_class.npy"])
    assert n > 0 and a["det_box.npy"].shape == (n, 8, 3) and a["det_score.npy"].shape == (n,)

    # the same arguments: the same arrays, bit for bit
    _bench(tmp_path / "b")
    b = _load(tmp_path / "b")
    assert set(b) == set(a)
    for name in a:
        assert np.array_equal(a[name], b[name]), name

    # and they are the last step's: its scene run on its own gives the same detections and decode arrays
    r = subprocess.run([sys.executable, "-c", ONE_SCENE, ROOT, str(STEPS), str(SCENES), str(tmp_path / "one")], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    one = _load(tmp_path / "one")
    assert set(one) == set(a)
    for name in a:
        if name == "y.npy":         # (fp32 summation order only: one scene in flight on another stream)
            np.testing.assert_allclose(a[name], one[name], rtol=0, atol=1e-6)
        else:
            assert np.array_equal(a[name], one[name]), name
