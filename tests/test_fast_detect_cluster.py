"""Process-level: a real shard on 20 s coordination sessions whose
coordination server runs with a 0.5 s disconnect grace —
``DevCluster(zk_disconnect_grace_ms=500)``.

kill -9 closes the sitter's connection at once, so the primary's death
is detected within the grace and not after the session timeout.  At
2 s sessions a failover measures about 2.1 s, i.e. everything after
detection costs a fraction of a second; the cap here is half the session
timeout, which detection by timeout (20 s or more) cannot meet.
"""

import asyncio
import time

from manatee_amd.tools.devcluster import DevCluster

SESSION_MS = 20000
GRACE_MS = 500
FAILOVER_CAP_S = SESSION_MS / 2000.0


def run(coro, timeout=240):
    return asyncio.run(asyncio.wait_for(coro, timeout))


def test_grace_reaches_the_coordination_processes(tmp_path, monkeypatch):
    monkeypatch.delenv("MANATEE_ZK_DISCONNECT_GRACE_MS", raising=False)
    c = DevCluster(str(tmp_path / "a"))
    assert c.zk_disconnect_grace_ms is None and c._zk_grace_args() == []
    c = DevCluster(str(tmp_path / "b"), zk_disconnect_grace_ms=GRACE_MS)
    assert c._zk_grace_args() == ["--disconnect-grace-ms", str(GRACE_MS)]
    # the environment decides only when the argument is not given
    monkeypatch.setenv("MANATEE_ZK_DISCONNECT_GRACE_MS", "3000")
    assert DevCluster(str(tmp_path / "c")).zk_disconnect_grace_ms == 3000
    assert DevCluster(str(tmp_path / "d"), zk_ensemble=3,
                      zk_disconnect_grace_ms=GRACE_MS) \
        .zk_disconnect_grace_ms == GRACE_MS
    assert DevCluster(str(tmp_path / "e"),
                      zk_disconnect_grace_ms=0).zk_disconnect_grace_ms is None


def test_killed_primary_is_detected_within_the_grace(tmp_path):
    async def go():
        c = DevCluster(str(tmp_path / "c"), n_peers=3,
                       shard_name="1.fastdetect",
                       session_timeout_ms=SESSION_MS,
                       zk_disconnect_grace_ms=GRACE_MS)
        try:
            await c.start()
            s = await c.wait_cluster(
                lambda s: s.get("sync") and len(s.get("async", [])) == 1,
                timeout_s=90, what="formation")
            prim = await c.wait_writable(timeout_s=60)
            assert prim.id == s["primary"]["id"]

            acked = []
            stop = False

            async def load():
                cli = prim.db_client()
                try:
                    k = 0
                    while not stop:
                        try:
                            await cli.put("k%d" % k, k, timeout_s=5.0)
                        except Exception:
                            return      # the primary died under us
                        acked.append(k)
                        k += 1
                        await asyncio.sleep(0.005)
                finally:
                    await cli.close()
            task = asyncio.get_running_loop().create_task(load())
            while len(acked) < 50:
                await asyncio.sleep(0.02)

            t0 = time.monotonic()
            prim.kill9()
            newp = await c.wait_writable(timeout_s=FAILOVER_CAP_S)
            took = time.monotonic() - t0
            print("writable again %.2f s after kill -9 (session %d ms, "
                  "grace %d ms)" % (took, SESSION_MS, GRACE_MS))
            assert took <= FAILOVER_CAP_S
            stop = True
            await task

            s2 = await c.cluster_state()
            assert newp.id == s["sync"]["id"] == s2["primary"]["id"]
            assert s2["generation"] > s["generation"]
            assert any(d["id"] == prim.id for d in s2["deposed"])
            assert len(acked) >= 50
            cli = newp.db_client()
            try:
                for k in acked:
                    assert await cli.get("k%d" % k) == k, \
                        "acknowledged write k%d lost" % k
            finally:
                await cli.close()
            with open(c.base_dir + "/zk.log", errors="replace") as f:
                assert "session expired after disconnect" in f.read()

            await c.rebuild_peer(prim)
            s3 = await c.wait_cluster(
                lambda st: st.get("sync") and len(st.get("async", [])) == 1
                and not st.get("deposed"),
                timeout_s=90, what="heal to primary, sync and async")
            assert s3["primary"]["id"] == newp.id
            assert prim.id in (s3["sync"]["id"], s3["async"][0]["id"])
        finally:
            c.stop()
    run(go())
