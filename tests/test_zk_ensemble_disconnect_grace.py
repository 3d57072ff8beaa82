"""The disconnect grace in a three-member coordination ensemble.

Only the serving leader talks to clients, so only it sees a client
close; what it saw is never replicated, and a new leader starts every
session on one full timeout.  The expiry itself is the ordinary
``session_close`` entry, so the replicas stay identical.
"""

import asyncio
import time

from manatee_amd.coord import jute
from manatee_amd.coord.zkquorum import ZkQuorumServer
from tests.test_zk_ensemble import (EL_MAX_MS, EL_MIN_MS, HEARTBEAT_MS, IDS,
                                    Ensemble, _client, _retry_until, run)
from tests.zkraw import RawSession

GRACE_MS = 500
GRACE_S = GRACE_MS / 1000.0
SESSION_MS = 20000
MARGIN_S = 1.0
EPH = "/grace/owner"


class GraceEnsemble(Ensemble):
    """``Ensemble`` whose members run with a disconnect grace."""

    async def start_member(self, i):
        peers = {}
        for j in IDS:
            if j == i:
                peers[j] = ("127.0.0.1", self.quorum_port[j])
            else:
                peers[j] = ("127.0.0.1", self.links[(i, j)].port)
        srv = ZkQuorumServer(
            i, client_host="127.0.0.1", client_port=self.client_port[i],
            peers=peers, data_dir=self.data_dir(i),
            election_timeout_ms=(EL_MIN_MS, EL_MAX_MS),
            heartbeat_ms=HEARTBEAT_MS,
            snapshot_entries=self.snapshot_entries,
            disconnect_grace_ms=GRACE_MS)
        await srv.start()
        self.members[i] = srv
        return srv


async def _owner(ens, lead, timeout_ms):
    """A raw session on the leader that owns EPH."""
    admin = await _client(ens.conn_str, timeout_ms=SESSION_MS)
    await admin.mkdirp("/grace")
    await admin.close()
    owner = await RawSession.open(ens.addr(lead), timeout_ms)
    assert owner.sid != 0 and owner.timeout_ms == timeout_ms
    await owner.create_ephemeral(EPH)
    return owner


def test_early_expiry_through_the_leader(tmp_path):
    async def go():
        ens = await GraceEnsemble(tmp_path).start()
        watcher = None
        try:
            lead = await ens.wait_leader()
            owner = await _owner(ens, lead, SESSION_MS)
            watcher = await _client(ens.conn_str, timeout_ms=SESSION_MS)
            gone = asyncio.get_running_loop().create_future()

            def on_event(etype, _path):
                if etype == jute.EVENT_NODE_DELETED and not gone.done():
                    gone.set_result(time.monotonic())
            assert await watcher.exists(EPH, watch=on_event) is not None
            t0 = time.monotonic()
            owner.abort()
            took = await asyncio.wait_for(gone, GRACE_S + MARGIN_S + 1.0) - t0
            print("delete seen %.3f s after the abort" % took)
            assert GRACE_S <= took <= GRACE_S + MARGIN_S
            assert await ens.wait_leader() == lead
            stats = ens.members[lead].stats
            assert stats["expired_on_disconnect"] == 1
            assert stats["expired_sessions"] == 1
            for i in IDS:
                if i != lead:
                    assert ens.members[i].stats["expired_on_disconnect"] == 0
            await watcher.close()
            watcher = None
            await ens.settled()
            full = ens.assert_identical()
            assert len(ens.members) == 3
            assert EPH not in full["nodes"]
            assert "0x%x" % owner.sid not in full["sessions"]
        finally:
            if watcher is not None:
                await watcher.close()
            await ens.stop()
    run(go())


def test_leader_change_during_the_grace_restores_the_full_timeout(tmp_path):
    """The new leader saw nobody close anything: the session of a client
    that is in fact gone gets one full timeout (6 s) there."""
    session_ms = 6000

    async def go():
        ens = await GraceEnsemble(tmp_path).start()
        try:
            lead = await ens.wait_leader()
            owner = await _owner(ens, lead, session_ms)
            await ens.settled()
            t0 = time.monotonic()
            owner.abort()
            await ens.stop_member(lead)
            assert time.monotonic() - t0 < GRACE_S, \
                "the old leader was not stopped within the grace"
            new = await ens.wait_leader()
            srv = ens.members[new]
            t_serving = time.monotonic()
            assert EPH in srv.nodes
            assert srv.sessions[owner.sid].detached_at is None
            await asyncio.sleep(4 * GRACE_S)
            assert EPH in srv.nodes and owner.sid in srv.sessions
            assert srv.stats["expired_sessions"] == 0
            # ... and then goes by the ordinary path
            await _retry_until(lambda: EPH not in srv.nodes,
                               session_ms / 1000.0 + MARGIN_S)
            took = time.monotonic() - t_serving
            print("expired %.3f s after the new leader began serving" % took)
            # the session's clock restarted when the new leader began
            # serving; wait_leader() polls every 10 ms, and the half
            # second allows for a loaded machine between the two
            assert took >= session_ms / 1000.0 - 0.5
            assert srv.stats["expired_sessions"] == 1
            assert srv.stats["expired_on_disconnect"] == 0
            await ens.settled()
            ens.assert_identical()
        finally:
            await ens.stop()
    run(go())


def test_follower_restart_during_the_grace_converges(tmp_path):
    async def go():
        ens = await GraceEnsemble(tmp_path).start()
        try:
            lead = await ens.wait_leader()
            follower = [i for i in IDS if i != lead][0]
            owner = await _owner(ens, lead, SESSION_MS)
            await ens.settled()
            t0 = time.monotonic()
            owner.abort()
            await ens.stop_member(follower)
            assert EPH in ens.members[lead].nodes, \
                "the follower was not stopped within the grace"
            await ens.start_member(follower)
            await _retry_until(lambda: EPH not in ens.members[lead].nodes,
                               GRACE_S + MARGIN_S)
            assert time.monotonic() - t0 >= GRACE_S
            assert await ens.wait_leader() == lead
            assert ens.members[lead].stats["expired_on_disconnect"] == 1
            await ens.settled()
            full = ens.assert_identical()
            assert len(ens.members) == 3
            assert EPH not in full["nodes"]
            assert "0x%x" % owner.sid not in full["sessions"]
        finally:
            await ens.stop()
    run(go())
