"""Process-level: a real shard whose coordination plane is a
three-member ensemble — ``DevCluster(zk_ensemble=3)``.  The same tier as
test_failover_matrix.py, and the smallest shapes that show the point:
losing one coordination member costs the shard nothing."""

import asyncio
import glob
import os
import subprocess
import sys

from manatee_amd.tools.devcluster import DevCluster

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADM_BIN = os.path.join(REPO, "bin", "manatee-adm")


def run(coro, timeout=240):
    return asyncio.run(asyncio.wait_for(coro, timeout))


def _sitter_logs(c):
    out = ""
    for p in c.peers:
        for path in glob.glob(os.path.join(p.dir, "sitter.log*")):
            with open(path, errors="replace") as f:
                out += f.read()
    return out


async def _formed(c):
    await c.start()
    s = await c.wait_cluster(
        lambda s: s.get("sync") and len(s.get("async", [])) == 1,
        timeout_s=90, what="formation")
    await c.wait_writable(timeout_s=60)
    return s


def test_default_mode_is_unchanged(tmp_path):
    c = DevCluster(str(tmp_path / "d"))
    assert c.zk_ensemble == 1 and c.zk_members == []
    assert c.zk_conn_str == "%s:%d" % (c.ip, c.zk_port)
    assert "," not in c.zk_conn_str
    # the peers' port blocks follow the single coordination block, as ever
    assert [p.index for p in c.peers] == [0, 1, 2]
    assert c.peers[0].pg_port > c.zk_port

    e = DevCluster(str(tmp_path / "e"), zk_ensemble=3)
    addrs = e.zk_conn_str.split(",")
    assert len(addrs) == 3 and len(set(addrs)) == 3
    assert [p.index for p in e.peers] == [0, 1, 2]
    assert e.peers[0].sitter_config()["zkCfg"]["connStr"] == e.zk_conn_str
    ports = [m["client_port"] for m in e.zk_members] + \
        [m["quorum_port"] for m in e.zk_members]
    assert len(set(ports)) == 6
    assert len({m["dir"] for m in e.zk_members}) == 3


def test_coordination_leader_kill_does_not_disturb_the_shard(tmp_path):
    async def go():
        c = DevCluster(str(tmp_path / "c"), n_peers=3,
                       shard_name="1.zkens", zk_ensemble=3)
        try:
            s = await _formed(c)
            roles = await c.zk_roles()
            assert sorted(roles) == ["follower", "follower", "leader"]
            lead = await c.zk_leader_index()
            assert roles[lead] == "leader"

            prim = c.peer_by_id(s["primary"]["id"])
            acked = []
            stop = False

            async def load():
                cli = prim.db_client()
                try:
                    k = 0
                    while not stop:
                        await cli.put("k%d" % k, k, timeout_s=5.0)
                        acked.append(k)
                        k += 1
                        await asyncio.sleep(0.005)
                finally:
                    await cli.close()
            task = asyncio.get_running_loop().create_task(load())
            while len(acked) < 20:
                await asyncio.sleep(0.02)

            c.kill_zk_member(lead)
            n_at_kill = len(acked)
            new_lead = await c.wait_zk_leader(timeout_s=30)
            assert new_lead != lead
            roles = await c.zk_roles()
            assert roles[lead] is None
            # two session timeouts of quiet: anything the loss of the
            # leader was going to upset has happened by now
            await asyncio.sleep(2 * c.session_timeout_ms / 1000.0)
            stop = True
            await task                      # raises if a write failed
            assert len(acked) > n_at_kill + 20

            s2 = await c.cluster_state()
            assert s2["generation"] == s["generation"]
            assert s2["primary"]["id"] == s["primary"]["id"]
            assert s2["sync"]["id"] == s["sync"]["id"]
            assert "session expired" not in _sitter_logs(c)
            cli = prim.db_client()
            for k in acked[-50:]:
                assert await cli.get("k%d" % k) == k
            await cli.close()

            # the dead member comes back as a follower and catches up
            c.start_zk_member(lead)
            for _ in range(200):
                roles = await c.zk_roles()
                if roles[lead] == "follower":
                    break
                await asyncio.sleep(0.05)
            assert sorted(roles) == ["follower", "follower", "leader"]
        finally:
            c.stop()
    run(go())


def test_failover_with_one_coordination_member_down(tmp_path):
    """Impossible with the standalone server, which was itself a single
    point of failure: a database failover while part of the coordination
    plane is dead."""
    async def go():
        c = DevCluster(str(tmp_path / "c"), n_peers=3,
                       shard_name="1.zkdown", zk_ensemble=3)
        try:
            s = await _formed(c)
            c.kill_zk_member(await c.zk_leader_index())
            await c.wait_zk_leader(timeout_s=30)
            prim = c.peer_by_id(s["primary"]["id"])
            cli = prim.db_client()
            for k in range(40):
                await cli.put("f%d" % k, k, timeout_s=5.0)
            await cli.close()

            prim.kill9()
            s2 = await c.wait_cluster(
                lambda st: st["generation"] > s["generation"],
                timeout_s=60, what="takeover with a zk member down")
            assert s2["primary"]["id"] == s["sync"]["id"]
            newp = await c.wait_writable(timeout_s=60)
            cli = newp.db_client()
            for k in range(40):
                assert await cli.get("f%d" % k) == k
            await cli.put("after", 1, timeout_s=5.0)
            await cli.close()
            assert (await c.zk_roles()).count(None) == 1
        finally:
            c.stop()
    run(go())


def test_adm_show_with_three_address_zk_ips(tmp_path):
    async def go():
        c = DevCluster(str(tmp_path / "c"), n_peers=1, singleton=True,
                       shard_name="1.zkadm", zk_ensemble=3,
                       run_snapshotter=False)
        try:
            await c.start()
            await c.wait_cluster(lambda s: s.get("primary"),
                                 timeout_s=60, what="formation")
            env = dict(os.environ)
            env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
            env["ZK_IPS"] = c.zk_conn_str
            env["SHARD"] = c.shard_path
            env.pop("MANATEE_ADM_TEST_STATE", None)
            assert c.zk_conn_str.count(",") == 2
            r = subprocess.run([sys.executable, ADM_BIN, "show"], env=env,
                               capture_output=True, text=True, timeout=60)
            assert r.returncode == 0, r.stdout + r.stderr
            assert c.peers[0].ip in r.stdout
            assert "primary" in r.stdout
            # ...and with one member (the leader) dead
            c.kill_zk_member(await c.zk_leader_index())
            await c.wait_zk_leader(timeout_s=30)
            r = subprocess.run([sys.executable, ADM_BIN, "show"], env=env,
                               capture_output=True, text=True, timeout=60)
            assert r.returncode == 0, r.stdout + r.stderr
            assert "primary" in r.stdout
        finally:
            c.stop()
    run(go())
