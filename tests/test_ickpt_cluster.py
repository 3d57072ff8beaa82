"""Incremental checkpoints through a whole shard of real subprocesses:
``postgresMgrCfg.waldbTunables`` reaches every peer's ``waldb.conf``,
primary and standbys write layers and compact them, a peer rebuilt from
a snapshot of a layered data dir starts and keeps the knob, and no
acknowledged write is lost when the primary is then killed.
"""

import json
import os

import pytest

from manatee_amd.storage import open_store
from tests.ickpt_cluster import (ckpt_info, formed, peer_conf, read_back,
                                 run, wait_for)


@pytest.fixture
def cluster_dir(tmp_path):
    return str(tmp_path / "cluster")


def test_layers_through_snapshot_rebuild_and_failover(cluster_dir):
    async def go():
        c, s, prim = await formed(cluster_dir, "1.ickpt")
        try:
            sync = c.peer_by_id(s["sync"]["id"])
            asy = c.peer_by_id(s["async"][0]["id"])
            for peer in c.peers:
                assert peer_conf(peer)["checkpoint_mode"] == "incremental"

            # overwrite a fixed key set: the base stays small, the deltas
            # pile up, compaction fires on primary and standby alike
            acked = {}
            seen = {prim.id: 0, sync.id: 0}
            cli = prim.db_client()
            rnd = 0

            async def layered():
                nonlocal rnd
                rnd += 1
                items = [("row%03d" % i, "r%d-" % rnd + "x" * 100)
                         for i in range(40)]
                assert await cli.put_many(items) == len(items)
                acked.update(items)
                done = True
                for peer in (prim, sync):
                    info = await ckpt_info(peer)
                    assert info["mode"] == "incremental"
                    seen[peer.id] = max(seen[peer.id], len(info["layers"]))
                    done = done and seen[peer.id] >= 2 and \
                        info["compactions"] >= 1
                return done
            await wait_for(layered, 60, "layers and a compaction on the "
                           "primary and the sync", every_s=0.06)
            await cli.close()

            # the sitter's /metrics carries the checkpointer's gauges
            info = await ckpt_info(prim)
            code, text = await prim.http_status("/metrics")
            assert code == 200
            gauges = dict(line.split(" ", 1) for line in text.splitlines()
                          if line.startswith("manatee_checkpoint"))
            assert int(gauges["manatee_checkpoints"]) >= \
                info["checkpoints"] >= 2
            assert int(gauges["manatee_checkpoint_compactions"]) >= \
                info["compactions"] >= 1
            assert int(gauges["manatee_checkpoint_last_bytes"]) > 0
            assert int(gauges["manatee_checkpoint_dirty_keys"]) >= 0

            # quiesced: the snapshot every restore peer would send
            for peer in (prim, sync):
                await open_store(peer.storage_cfg(), log=None).snapshot()
            await c.rebuild_peer(asy)
            # (it never left the cluster state, so that returns at once)
            await wait_for(lambda: _caught_up(asy, prim), 60,
                           "rebuilt peer streaming and caught up")
            conf = peer_conf(asy)
            assert conf["checkpoint_mode"] == "incremental"
            assert conf["checkpoint_wal_bytes"] == "4096"
            assert conf["port"] == str(asy.pg_port)
            # it started from the snapshot's layers, not from an image
            # (its log is the restored database's alone: the fixup after
            # a restore deletes the one that rode in)
            loaded = [r for r in _db_log(asy)
                      if r["msg"] == "checkpoint loaded"]
            assert loaded and loaded[-1]["layers"] >= 1, loaded
            info = await ckpt_info(asy)
            assert info["layers"] and info["layers"][0]["kind"] == "base"
            await read_back(asy, acked)

            prim.kill9()
            new_prim = await c.wait_writable(timeout_s=60)
            assert new_prim.id != prim.id
            await read_back(new_prim, acked)
            assert peer_conf(asy)["checkpoint_mode"] == "incremental"
            assert (await ckpt_info(new_prim))["mode"] == "incremental"
        finally:
            c.stop()
    run(go())


def _db_log(peer) -> list:
    with open(os.path.join(peer.store_dir, "live", "waldb.log")) as f:
        return [json.loads(line) for line in f if line.startswith("{")]


async def _caught_up(peer, primary) -> bool:
    cli, pcli = peer.db_client(), primary.db_client()
    try:
        st = await cli.status()
        return st["upstream_status"] == "streaming" and \
            st["replay_lsn"] == (await pcli.status())["current_lsn"]
    finally:
        await cli.close()
        await pcli.close()
