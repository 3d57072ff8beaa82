"""Shared steps of the rewind cluster tests: a 3-peer DevCluster whose
primary is killed holding WAL the sync never saw, and the real
``manatee-adm rebuild`` run against the deposed peer."""

import asyncio
import json
import os
import signal
import sys
import time

from manatee_amd.common import lsn as lsnmod
from manatee_amd.tools.devcluster import DevCluster

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADM_BIN = os.path.join(REPO, "bin", "manatee-adm")


async def formed(cluster_dir, shard_name, **kw):
    c = DevCluster(cluster_dir, n_peers=3, shard_name=shard_name,
                   rewind_on_divergence=True, **kw)
    await c.start()
    await c.wait_cluster(
        lambda s: s.get("sync") and len(s.get("async", [])) == 1,
        timeout_s=60, what="formation")
    return c


async def put_acked(peer, prefix, n, value_bytes=8):
    """``n`` acknowledged puts; returns ``{key: value}``."""
    cli = peer.db_client()
    acked = {}
    try:
        for lo in range(0, n, 64):
            items = [("%s%05d" % (prefix, i), "%d:" % i + "v" * value_bytes)
                     for i in range(lo, min(n, lo + 64))]
            await cli.put_many(items, timeout_s=30)
            acked.update(items)
    finally:
        await cli.close()
    return acked


async def depose_primary(c, prim, divergent=0, value_bytes=8, settle_s=0.3,
                         ckpt_fraction=0.0):
    """Kill the primary so that it is deposed.  With ``divergent`` > 0
    it dies holding that many records the sync never received: the sync
    is frozen, the puts are pipelined and never awaited (the commit gate
    holds their acks), the primary is killed, the sync thawed.  With
    ``ckpt_fraction`` the primary is killed only once its checkpoint
    covers that fraction of the unacknowledged bytes."""
    s = await c.cluster_state()
    gen = s["generation"]
    sync = c.peer_by_id(s["sync"]["id"])
    writer = None
    if divergent:
        pc = prim.db_client()
        before = lsnmod.parse((await pc.status())["current_lsn"])
        sync.pause()
        _reader, writer = await asyncio.open_connection(prim.ip,
                                                        prim.pg_port)
        writer.write(b"".join(
            json.dumps({"q": "put", "k": "unacked%05d" % i,
                        "v": "u" * value_bytes}).encode() + b"\n"
            for i in range(divergent)))
        await writer.drain()
        deadline = time.monotonic() + 30
        while lsnmod.parse((await pc.status())["current_lsn"]) - before \
                < divergent * value_bytes:
            assert time.monotonic() < deadline, "puts never appended"
            await asyncio.sleep(0.02)
        while ckpt_fraction and lsnmod.parse(
                (await pc.status())["checkpoint_lsn"]) - before \
                < ckpt_fraction * divergent * value_bytes:
            assert time.monotonic() < deadline, "never checkpointed"
            await asyncio.sleep(0.02)
        await pc.close()
        # the flush loop writes the append buffer out every 50 ms
        await asyncio.sleep(settle_s)
    prim.kill9()
    if writer is not None:
        writer.close()
        sync.resume()
    await c.wait_cluster(
        lambda st: st["generation"] > gen
        and any(d["id"] == prim.id for d in st["deposed"]),
        timeout_s=90, what="takeover deposing the old primary")
    return await c.wait_writable(timeout_s=90)


async def adm_rebuild(c, peer, *flags, timeout=120):
    """``manatee-adm rebuild -y`` for ``peer`` with a --start-cmd that
    restarts its sitter.  Returns ``(returncode, output)``."""
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    env.pop("MANATEE_ADM_TEST_STATE", None)
    cfg = os.path.join(peer.dir, "sitter.json")
    start_cmd = (
        "setsid %s -m manatee_amd.daemons.sitter -f %s "
        "--log-file %s >/dev/null 2>&1 & echo $! > %s"
        % (sys.executable, cfg,
           os.path.join(peer.dir, "sitter-rebuilt.log.json"),
           os.path.join(peer.dir, "sitter-rebuilt.pid")))
    proc = await asyncio.create_subprocess_exec(
        sys.executable, ADM_BIN, "rebuild", "-c", cfg, "-y", *flags,
        "--start-cmd", start_cmd, "--timeout", str(timeout),
        env=env, stdout=asyncio.subprocess.PIPE,
        stderr=asyncio.subprocess.STDOUT)
    out, _ = await asyncio.wait_for(proc.communicate(), timeout + 60)
    return proc.returncode, out.decode()


def kill_rebuilt_sitter(peer):
    """The sitter the CLI's --start-cmd spawned (devcluster does not
    track it), then the peer's database."""
    try:
        with open(os.path.join(peer.dir, "sitter-rebuilt.pid")) as f:
            os.killpg(int(f.read().strip()), signal.SIGKILL)
    except (OSError, ValueError):
        pass
    peer.kill9()


async def assert_same_data(prim, peer, acked, timeout_s=60):
    """``peer`` catches up with ``prim``, serves every acknowledged key
    with the primary's value and no key of the deposed tail."""
    pc, rc = prim.db_client(), peer.db_client()
    try:
        deadline = time.monotonic() + timeout_s
        while True:
            try:
                if await rc.count() == await pc.count() and \
                        (await rc.status())["replay_lsn"] == \
                        (await pc.status())["current_lsn"]:
                    break
            except Exception:
                pass
            assert time.monotonic() < deadline, "peer never caught up"
            await asyncio.sleep(0.2)
        lost = 0
        keys = sorted(acked)
        for lo in range(0, len(keys), 256):
            chunk = keys[lo:lo + 256]
            reqs = [{"q": "get", "k": k} for k in chunk]
            mine = await rc.pipeline(reqs, timeout_s=30)
            theirs = await pc.pipeline(reqs, timeout_s=30)
            for k, m, t in zip(chunk, mine, theirs):
                assert m.get("v") == t.get("v"), k
                lost += not (m.get("found") and m["v"] == acked[k])
        assert lost == 0, "%d acknowledged writes lost" % lost
        # of the puts nobody acknowledged, exactly those the new primary
        # had received before the old one died
        assert await rc.count("unacked") == await pc.count("unacked")
        assert await rc.count() == await pc.count()
    finally:
        await pc.close()
        await rc.close()


async def metrics(peer):
    """The peer's /metrics as ``{sample name with labels: value}``."""
    code, body = await peer.http_status("/metrics")
    assert code == 200, body
    out = {}
    for line in body.splitlines():
        if line and not line.startswith("#"):
            name, _, value = line.rpartition(" ")
            out[name] = float(value)
    return out
