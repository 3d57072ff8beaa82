"""Transactions across failover on a 3-peer engine=postgres shard: two
tpcb writers run until the primary is SIGKILLed; on the new primary,
and on the deposed peer once it is rebuilt, every writer's balances,
history rows and sequence stamps must describe a whole number of
transactions that includes every acknowledged one.
"""

import asyncio
import time

from manatee_amd.tools.devcluster import DevCluster
from manatee_amd.tools.wrbench import TpcbWriter, check_tpcb


def run(coro, timeout=240):
    return asyncio.run(asyncio.wait_for(coro, timeout))


async def _until(what, probe, timeout_s=30.0):
    deadline = time.monotonic() + timeout_s
    last = None
    while True:
        try:
            if await probe():
                return
        except Exception as exc:
            last = exc
        assert time.monotonic() < deadline, "%s: %r" % (what, last)
        await asyncio.sleep(0.1)


def test_tpcb_invariants_across_primary_death(tmp_path):
    async def go():
        c = DevCluster(str(tmp_path / "c"), n_peers=3,
                       shard_name="1.pgtxn", engine="postgres",
                       run_snapshotter=False)
        writers = []
        try:
            await c.start()
            s = await c.wait_cluster(
                lambda s: s.get("sync") and len(s.get("async", [])) == 1,
                timeout_s=120, what="3-peer formation (engine=postgres)")
            prim = await c.wait_writable(timeout_s=120)

            # an atomic batch reaches the async standby as a whole
            items = [("atom-%d" % i, i) for i in range(30)]
            cli = prim.db_client()
            assert await cli.put_many_atomic(items) == 30
            await cli.close()
            acli = c.peer_by_id(s["async"][0]["id"]).db_client()
            seen = set()

            async def replicated():
                n = await acli.count(prefix="atom-")
                seen.add(n)
                return n == 30
            await _until("atomic batch on the async", replicated)
            assert seen <= {0, 30}, "a partial batch was visible: %r" % seen
            assert await acli.get_many([k for k, _ in items]) == \
                [v for _, v in items]
            await acli.close()

            writers = [TpcbWriter(prim, w, n_accounts=4) for w in range(2)]
            for w in writers:
                await w.setup()
            stop = asyncio.Event()
            tasks = [asyncio.ensure_future(w.run(stop)) for w in writers]
            await _until("both writers committing",
                         lambda: _true(all(w.acked >= 20 for w in writers)))
            prim.kill9()
            # the writers die with their connections, mid-transaction
            done = await asyncio.gather(*tasks, return_exceptions=True)
            assert all(isinstance(d, Exception) for d in done), done
            acked = [w.acked for w in writers]
            assert min(acked) >= 20

            await c.wait_cluster(
                lambda st: st["generation"] > s["generation"] and
                st["primary"]["id"] == s["sync"]["id"],
                timeout_s=60, what="sync takeover")
            newp = await c.wait_writable(timeout_s=60)
            assert newp.id != prim.id
            ncli = newp.db_client()
            last = [await check_tpcb(ncli, w.label, w.n_accounts, w.acked)
                    for w in writers]
            await ncli.close()
            # at most the one COMMIT in flight at the kill is unacked
            assert all(a <= m <= a + 1 for a, m in zip(acked, last)), \
                (acked, last)

            await c.rebuild_peer(prim)
            rcli = prim.db_client()

            async def caught_up():
                return [await rcli.count(prefix="hist-%s-" % w.label)
                        for w in writers] == [m + 1 for m in last]
            await _until("rebuilt peer replaying the history", caught_up)
            assert [await check_tpcb(rcli, w.label, w.n_accounts, w.acked)
                    for w in writers] == last
            await rcli.close()
        finally:
            for w in writers:
                await w.close()
            c.stop()
    run(go())


async def _true(value):
    return value
