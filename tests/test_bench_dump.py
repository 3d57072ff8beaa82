"""bench.py --dump-outputs / --full contract: one timed step, then the
PRELOAD keys read back from the final primary and sync land as float64
``.npy`` files whose content is fixed by the benchmark's inputs."""

import json
import os
import subprocess
import sys

import numpy as np

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_dump_outputs(tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    dump = tmp_path / "dump"
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"),
         "--gpus", "1", "--steps", "1", "--warmup", "0", "--full",
         "--dump-outputs", str(dump)],
        capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 1 and out["ms_per_step"] > 0
    assert sorted(os.listdir(dump)) == [
        "lost_acked_writes.npy", "readback_primary.npy",
        "readback_sync.npy"]
    want = np.arange(bench.PRELOAD, dtype=np.float64)
    for name in ("readback_primary", "readback_sync"):
        got = np.load(dump / (name + ".npy"))
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, want)
    lost = np.load(dump / "lost_acked_writes.npy")
    assert lost.dtype == np.float64 and lost.tolist() == [0.0]
