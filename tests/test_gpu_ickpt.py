"""Dedicated-box (gpu-marked) tier for incremental checkpoints: a
50k-key dataset, a 100-key hot set overwritten under load, the primary
killed mid-load."""

import asyncio
import time

import pytest

from manatee_amd.common import lsn
from tests.ickpt_cluster import (TUNABLES, ckpt_info, formed, read_back,
                                 run, wait_for)

pytestmark = pytest.mark.gpu

PRELOAD = 50000
HOT = 100
HOT_SECONDS = 3.0
# wait_writable writes one probe key of its own into the shard
OTHER_KEYS = 1


@pytest.fixture
def cluster_dir(tmp_path):
    return str(tmp_path / "cluster")


@pytest.mark.timeout(120)
def test_hot_set_deltas_and_zero_loss_across_primary_kill(cluster_dir):
    """The dataset is 500x the hot set.  Once the preload has been
    checkpointed, every delta the survivor writes holds at most the hot
    set: the layer's record count and the checkpointer's own counters
    say so, whatever the timing was.  No acknowledged write is lost."""
    async def go():
        c, s, prim = await formed(cluster_dir, "1.gpuickpt")
        try:
            sync = c.peer_by_id(s["sync"]["id"])
            acked = {}
            cli = prim.db_client()
            for at in range(0, PRELOAD, 2000):
                items = [("pre%05d" % i, "p" * 100)
                         for i in range(at, min(at + 2000, PRELOAD))]
                assert await cli.put_many(items, timeout_s=60) == len(items)
                acked.update(items)

            # the preload is in layers on both and no checkpoint is due
            # or running: less than checkpoint_wal_bytes of WAL is past
            # the manifest.  What is dirty now is all of the preload that
            # a later delta can still hold.
            async def settled():
                for peer in (prim, sync):
                    info = await ckpt_info(peer)
                    pcli = peer.db_client()
                    try:
                        st = await pcli.status()
                    finally:
                        await pcli.close()
                    gap = lsn.parse(st["replay_lsn"]) - lsn.parse(info["lsn"])
                    if not info["layers"] or \
                            gap >= TUNABLES["checkpoint_wal_bytes"]:
                        return False
                return True
            await wait_for(settled, 30, "preload checkpointed")
            before = await ckpt_info(sync)

            # overwrite the hot set, pipelined, and kill mid-load
            hot = {}
            stop = asyncio.Event()

            async def load():
                seq = 0
                try:
                    while not stop.is_set():
                        items = []
                        for i in range(HOT):
                            seq += 1
                            items.append(("hot%03d" % i, seq))
                        await cli.put_many(items, timeout_s=10)
                        hot.update(items)        # acknowledged, all of it
                except Exception:
                    pass                         # the primary died under us
            task = asyncio.get_running_loop().create_task(load())
            t0 = time.monotonic()
            await asyncio.sleep(HOT_SECONDS)
            assert not task.done(), "the load stopped before the kill"
            prim.kill9()
            stop.set()
            await task
            await cli.close()
            assert hot, "nothing was acknowledged in %.1fs" % (
                time.monotonic() - t0)

            new_prim = await c.wait_writable(timeout_s=60)
            assert new_prim.id == sync.id
            await read_back(new_prim, acked)
            ncli = new_prim.db_client()
            try:
                for k, seq in hot.items():
                    # an unacknowledged newer write may have landed too
                    got = await ncli.get(k)
                    assert got is not None and got >= seq, (k, got, seq)
            finally:
                await ncli.close()

            info = await ckpt_info(new_prim)
            print("ckpt before the hot phase: %r" % (before,))
            print("ckpt on the survivor:      %r" % (info,))
            assert info["mode"] == "incremental"
            assert info["checkpoints"] > before["checkpoints"]
            assert info["compactions"] >= 1
            bound = HOT + OTHER_KEYS + before["dirty_keys"]
            # each preload record is longer than its 100-byte value and
            # less than checkpoint_wal_bytes of them were outstanding
            assert before["dirty_keys"] <= \
                TUNABLES["checkpoint_wal_bytes"] // 100, before
            deltas = [layer for layer in info["layers"]
                      if layer["kind"] == "delta"
                      and lsn.parse(layer["lsn"]) > lsn.parse(before["lsn"])]
            for layer in deltas:
                assert layer["records"] <= bound, layer
            # the last checkpoint wrote what was dirty, no more
            assert info["last_checkpoint_records"] <= \
                info["last_checkpoint_dirty"] <= bound, info
            assert info["dirty_keys"] <= bound
            base = info["layers"][0]
            assert base["kind"] == "base" and base["records"] >= PRELOAD
        finally:
            c.stop()
    run(go())
