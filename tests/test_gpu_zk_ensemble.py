"""Dedicated-box (gpu-marked) tier for the replicated coordination
ensemble: the chaos soak with ``--zk-ensemble 3``."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# Under seed 5 the soak's first four draws (11 actions in ensemble mode)
# are kill_zk_leader, zk_outage, kill_zk_follower, kill_db_only: both
# new families, plus a full outage and restart of all three members.
SEED = 5
CYCLES = 4


@pytest.mark.timeout(600)
def test_soak_with_coordination_ensemble_zero_acked_loss():
    """A handful of soak cycles over a three-member coordination
    ensemble, run as a child process the way the 50-cycle soak is.

    Unlike every other new test this one cannot take "a few seconds":
    each cycle is a real fault on a live shard — seconds of failover,
    an exact acked-write verification and a heal back to full shape —
    and formation comes first.  It is kept to four cycles and has its
    own timeout."""
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(
        [sys.executable, "-m", "manatee_amd.tools.soak",
         "--zk-ensemble", "3", "--cycles", str(CYCLES), "--minutes", "8",
         "--seed", str(SEED)],
        capture_output=True, text=True, timeout=540, env=env, cwd=REPO)
    tail = "\n".join(r.stderr.splitlines()[-12:])
    assert r.returncode == 0, tail + "\n" + r.stdout
    stats = json.loads(r.stdout.splitlines()[-1])
    assert stats["ok"], stats
    assert stats["cycles"] == CYCLES, stats
    assert stats["kills"].get("kill_zk_leader", 0) >= 1, stats["kills"]
    assert stats["kills"].get("kill_zk_follower", 0) >= 1, stats["kills"]
    assert stats["lost"] == 0, stats
    assert not stats["failures"], stats
    assert stats["acked"] > 0, stats
    assert "max_zk_failover_s" in stats, stats
    assert stats["max_zk_failover_s"] > 0.0, stats
