"""Dedicated-box (gpu-marked) tier for the coordination servers'
disconnect grace: the chaos soak with ``--zk-disconnect-grace-ms 500``,
against the standalone server and against a three-member ensemble.

The soak's fault families split on exactly the line the grace draws:
kills and proxy partitions close connections, SIGSTOP does not.  Each
cycle is a real fault on a live shard (failover, exact acked-write
verification, heal), so like tests/test_gpu_zk_ensemble.py these run as
child processes with their own timeouts and not in "a few seconds".
"""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SEED = 7
CYCLES = 10
MINUTES = 6
GRACE_MS = 500


def _soak(*extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(
        [sys.executable, "-m", "manatee_amd.tools.soak",
         "--cycles", str(CYCLES), "--minutes", str(MINUTES),
         "--seed", str(SEED), "--zk-disconnect-grace-ms", str(GRACE_MS)]
        + list(extra),
        capture_output=True, text=True, timeout=MINUTES * 60 + 120, env=env,
        cwd=REPO)
    tail = "\n".join(r.stderr.splitlines()[-12:])
    assert r.returncode == 0, tail + "\n" + r.stdout
    stats = json.loads(r.stdout.splitlines()[-1])
    print(json.dumps(stats))
    assert stats["ok"], stats
    assert stats["lost"] == 0, stats
    assert not stats["failures"], stats
    assert stats["acked"] > 0, stats
    assert stats["cycles"] >= 1, stats
    assert stats["zk_disconnect_grace_ms"] == GRACE_MS, stats
    return stats


@pytest.mark.timeout(MINUTES * 60 + 180)
def test_soak_with_disconnect_grace_zero_acked_loss():
    _soak()


@pytest.mark.timeout(MINUTES * 60 + 180)
def test_soak_with_disconnect_grace_and_ensemble_zero_acked_loss():
    stats = _soak("--zk-ensemble", "3")
    assert stats["zk_ensemble"] == 3, stats
