"""A 3-peer DevCluster on the ``dir`` store with every waldb in
``checkpoint_mode = incremental`` and thresholds of a few KB, for
tests/test_ickpt_cluster.py and tests/test_gpu_ickpt.py."""

import asyncio
import os
import time

from manatee_amd.common import confparser
from manatee_amd.tools.devcluster import DevCluster

TUNABLES = {"checkpoint_mode": "incremental",
            "checkpoint_wal_bytes": 4096,
            "wal_segment_bytes": 16384,
            "wal_keep_bytes": 65536}


def run(coro, timeout=240):
    return asyncio.run(asyncio.wait_for(coro, timeout))


async def formed(cluster_dir: str, shard: str, tunables=None):
    """Start the cluster; returns (cluster, state, primary peer)."""
    c = DevCluster(cluster_dir, n_peers=3, shard_name=shard,
                   run_snapshotter=False,
                   waldb_tunables=dict(TUNABLES if tunables is None
                                       else tunables))
    try:
        await c.start()
        s = await c.wait_cluster(
            lambda s: s.get("sync") and len(s.get("async", [])) == 1,
            timeout_s=60, what="3-peer formation")
        prim = await c.wait_writable(timeout_s=60)
        assert prim.id == s["primary"]["id"]
    except BaseException:
        c.stop()
        raise
    return c, s, prim


async def ckpt_info(peer) -> dict:
    cli = peer.db_client()
    try:
        return await cli.checkpoint_info()
    finally:
        await cli.close()


def peer_conf(peer) -> dict:
    return confparser.read(os.path.join(peer.store_dir, "live", "data",
                                        "waldb.conf"))


async def wait_for(pred, timeout_s: float, what: str, every_s: float = 0.1):
    """Poll the coroutine function ``pred`` until it returns a truthy
    value; returns it."""
    deadline = time.monotonic() + timeout_s
    last = None
    while True:
        try:
            got = await pred()
            if got:
                return got
        except Exception as exc:
            last = exc
        if time.monotonic() > deadline:
            raise AssertionError("timeout waiting for %s; last error %r"
                                 % (what, last))
        await asyncio.sleep(every_s)


async def read_back(peer, acked: dict) -> None:
    """Every acknowledged key reads back from ``peer`` with its last
    acknowledged value."""
    cli = peer.db_client()
    try:
        keys = sorted(acked)
        for at in range(0, len(keys), 500):
            part = keys[at:at + 500]
            resps = await cli.pipeline({"q": "get", "k": k} for k in part)
            for k, r in zip(part, resps):
                assert r.get("ok") and r.get("found") and \
                    r.get("v") == acked[k], \
                    "acknowledged write %s lost: %r" % (k, r)
    finally:
        await cli.close()
