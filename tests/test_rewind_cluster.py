"""``manatee-adm rebuild --rewind`` on a live 3-peer shard: a deposed
ex-primary with a genuinely divergent WAL tail rejoins without a
restore; an idle one is a noop; a checkpoint past the fork refuses and
changes nothing."""

import asyncio
import os
import re

import pytest

from manatee_amd.adm import core as adm
from tests import crashfs
from tests.rewind_cluster import (adm_rebuild, assert_same_data,
                                  depose_primary, formed,
                                  kill_rebuilt_sitter, metrics, put_acked)

# more than a frozen receiver's socket buffers and the sender's can hold
# between them, so the killed primary keeps records nobody else has
DIVERGENT, VALUE_BYTES = 384, 64 * 1024


def run(coro, timeout=300):
    return asyncio.run(asyncio.wait_for(coro, timeout))


@pytest.fixture
def cluster_dir(tmp_path):
    return str(tmp_path / "cluster")


async def _assert_rejoined_without_restore(c, peer, newp, acked, result):
    s = await c.cluster_state()
    assert s["deposed"] == []
    assert any(a["id"] == peer.id for a in s["async"])
    await assert_same_data(newp, peer, acked)
    m = await metrics(peer)
    rewinds = {k: v for k, v in m.items()
               if k.startswith("manatee_rewinds_total")}
    assert rewinds.pop('manatee_rewinds_total{result="%s"}' % result) == 1
    assert set(rewinds.values()) == {0}, rewinds
    assert m["manatee_restores_total"] == 0
    code, body = await peer.http_status("/restore")
    assert code == 200 and body == {"active": False, "done": False}
    code, body = await peer.http_status("/ping")
    assert body["status"]["rewind"]["result"] == result
    assert not os.path.exists(os.path.join(peer.store_dir, "isolated"))


def test_rebuild_rewind_of_a_divergent_ex_primary(cluster_dir):
    async def go():
        # no checkpoint while the test runs: one taken over the divergent
        # tail is the refusal of the third test
        c = await formed(cluster_dir, "1.rwd",
                         waldb_tunables={"checkpoint_wal_bytes": 1 << 30})
        prim = None
        try:
            prim = await c.wait_writable(timeout_s=60)
            acked = await put_acked(prim, "acked", 200)
            newp = await depose_primary(c, prim, DIVERGENT, VALUE_BYTES)
            acked.update(await put_acked(newp, "later", 50))

            rc, text = await adm_rebuild(c, prim, "--rewind")
            assert rc == 0, text
            m = re.search(r"rewound to the fork point (\S+) "
                          r"\((\d+) bytes cut", text)
            assert m, text
            assert int(m.group(2)) > 0
            assert "removed %s from the deposed list" % prim.id in text
            assert "rejoined the cluster" in text
            await _assert_rejoined_without_restore(c, prim, newp, acked,
                                                   "ok")
        finally:
            if prim is not None:
                kill_rebuilt_sitter(prim)
            c.stop()
    run(go())


def test_rebuild_rewind_of_an_idle_ex_primary_is_a_noop(cluster_dir):
    async def go():
        c = await formed(cluster_dir, "1.rwi")
        prim = None
        try:
            prim = await c.wait_writable(timeout_s=60)
            acked = await put_acked(prim, "acked", 50)
            newp = await depose_primary(c, prim)
            rc, text = await adm_rebuild(c, prim, "--rewind")
            assert rc == 0, text
            assert "rewind: noop" in text and "(0 bytes cut)" in text
            assert "rejoined the cluster" in text
            await _assert_rejoined_without_restore(c, prim, newp, acked,
                                                   "noop")
        finally:
            if prim is not None:
                kill_rebuilt_sitter(prim)
            c.stop()
    run(go())


async def _reap_and_restart(c, peer):
    """Let the deposed peer back in WITHOUT a rebuild: its sitter finds
    the database refused as diverged."""
    zk = await adm.create_zk_client(c.zk_conn_str)
    try:
        await adm.reap(zk, c.shard_path, peer_id=peer.id)
    finally:
        await zk.close()
    peer.start()
    await c.wait_cluster(
        lambda s: any(a["id"] == peer.id for a in s.get("async", [])),
        timeout_s=60, what="peer back as async")


@pytest.mark.parametrize("refused", [False, True])
def test_manager_rewinds_a_diverged_standby_before_restoring(cluster_dir,
                                                             refused):
    """``rewindOnDivergence``: a standby refused as diverged is rewound
    by its own sitter; a rewind that refuses falls through to the
    restore."""
    async def go():
        c = await formed(
            cluster_dir, "1.rwm",
            waldb_tunables={"checkpoint_wal_bytes":
                            64 if refused else 1 << 30})
        try:
            prim = await c.wait_writable(timeout_s=60)
            acked = await put_acked(prim, "acked", 100)
            newp = await depose_primary(
                c, prim, DIVERGENT, VALUE_BYTES,
                ckpt_fraction=0.6 if refused else 0.0)
            await _reap_and_restart(c, prim)
            await assert_same_data(newp, prim, acked)
            m = await metrics(prim)
            code, body = await prim.http_status("/ping")
            last = body["status"]["rewind"]
            if refused:
                assert m['manatee_rewinds_total{result="refused"}'] == 1
                assert m['manatee_rewinds_total{result="ok"}'] == 0
                assert m["manatee_restores_total"] == 1
                assert last["reason"] == "checkpoint-past-fork"
            else:
                assert m['manatee_rewinds_total{result="ok"}'] == 1
                assert m['manatee_rewinds_total{result="refused"}'] == 0
                assert m["manatee_restores_total"] == 0
                assert last["result"] == "ok" and last["bytes_cut"] > 0
                assert body["status"]["restore"] is None
        finally:
            c.stop()
    run(go())


def test_rebuild_rewind_refuses_a_checkpoint_past_the_fork(cluster_dir):
    async def go():
        # full mode, a checkpoint every few KB of WAL: the primary
        # checkpoints its divergent tail before it dies
        c = await formed(cluster_dir, "1.rwr",
                         waldb_tunables={"checkpoint_wal_bytes": 64})
        prim = None
        try:
            prim = await c.wait_writable(timeout_s=60)
            await put_acked(prim, "acked", 50)
            # a full checkpoint is due once new WAL reaches half the last
            # image, so the last one covers over 2/3 of the tail: far
            # past what the frozen sync's socket buffers held
            await depose_primary(c, prim, DIVERGENT, VALUE_BYTES,
                                 ckpt_fraction=0.6)
            data_dir = os.path.join(prim.store_dir, "live", "data")
            before = crashfs.snapshot(data_dir)
            deposed = (await c.cluster_state())["deposed"]
            rc, text = await adm_rebuild(c, prim, "--rewind")
            assert rc != 0, text
            assert "rewind refused: checkpoint-past-fork" in text
            assert "rerun without --rewind" in text
            assert crashfs.snapshot(data_dir) == before
            assert (await c.cluster_state())["deposed"] == deposed
            assert any(d["id"] == prim.id for d in deposed)
            assert not os.path.exists(os.path.join(prim.store_dir,
                                                   "isolated"))
            assert not os.path.exists(os.path.join(prim.dir,
                                                   "sitter-rebuilt.pid"))
        finally:
            if prim is not None:
                kill_rebuilt_sitter(prim)
            c.stop()
    run(go())
