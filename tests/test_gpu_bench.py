"""GPU: a plain `bench.py` run -- exactly K timed steps, the headline keys, nothing of --full -- and --dump-outputs: two
runs with the same arguments hand back the same outputs, bit for bit (the settle phase before the warm-up may differ in
length from run to run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps, warmup):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_plain_run_and_dumped_outputs(tmp_path):
    K, W = 10, 5
    runs = [_bench(tmp_path / ("run%d" % i), K, W) for i in range(2)]
    for line in runs:
        assert line["metric"] == "frame_pairs_per_sec" and line["unit"] == "frame-pairs/s" and line["higher_is_better"]
        assert line["steps"] == K and line["warmup"] == W and line["pairs_launched_in_timed_region"] == K
        assert not line["pairs_mismatch"] and line["value"] > 0 and line["ms_per_step"] > 0
        assert line["segments_archived_in_timed_region"] == line["segments_expected"] > 0
        assert abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-6 * 1e3
        assert line["full"] is False
        assert not {"cpu_baseline", "roofline", "kernel_rooflines", "iterations_per_feature"} & set(line)
    names = sorted(os.listdir(tmp_path / "run0"))
    assert names == ["live_trackquality.npy", "live_tracks.npy", "trackquality.npy", "tracks.npy"]
    assert names == sorted(os.listdir(tmp_path / "run1"))
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "run0" / n), np.load(tmp_path / "run1" / n)
        assert a.dtype == np.float32 and a.shape == b.shape, n
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), n
        total += a.nbytes
    assert total <= 64 << 20
    tracks, quality = np.load(tmp_path / "run0" / "tracks.npy"), np.load(tmp_path / "run0" / "trackquality.npy")
    # the np.savez payload of one finished segment: track_len + 1 = 3 vertices per track, 2 quality values
    assert tracks.ndim == 3 and tracks.shape[1:] == (3, 2) and quality.shape == (len(tracks), 2) and len(tracks) > 1000
    assert np.isfinite(tracks).all() and np.isfinite(quality).all()
