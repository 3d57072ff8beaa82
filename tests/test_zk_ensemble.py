"""Three in-process ``ZkQuorumServer``s and the real ``ZkClient``.

Every directed member-to-member link runs through a ``LinkProxy`` (each
server's peer table simply holds the proxies' addresses), and clients
that must be cut off are given proxy addresses too — so links are cut
without any seam in production code.
"""

import asyncio
import os
import random
import shutil
import socket
import time

import pytest

from manatee_amd.common.logging import null_logger
from manatee_amd.coord import jute
from manatee_amd.coord.jute import MultiOp, ZkError
from manatee_amd.coord.zkclient import ZkClient
from manatee_amd.coord.zkquorum import MemberDisk, ZkQuorumServer
from manatee_amd.tools.devcluster import _EPHEMERAL_LOW
from manatee_amd.tools.netproxy import LinkProxy

EL_MIN_MS, EL_MAX_MS = 200, 400
HEARTBEAT_MS = 40
SESSION_MS = 1500
IDS = (1, 2, 3)


def free_port():
    """A listen port BELOW the kernel's ephemeral range: a member is
    stopped and started again on the same port, and no outgoing socket
    of anybody's may take it in between."""
    rng = random.Random()
    while True:
        port = rng.randrange(12000, min(_EPHEMERAL_LOW, 32768) - 1)
        s = socket.socket()
        s.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        try:
            s.bind(("127.0.0.1", port))
            return port
        except OSError:
            continue
        finally:
            s.close()


def run(coro, timeout=60):
    return asyncio.run(asyncio.wait_for(coro, timeout))


class Ensemble:
    def __init__(self, base_dir, snapshot_entries=1000):
        self.base_dir = str(base_dir)
        self.snapshot_entries = snapshot_entries
        ports = set()
        while len(ports) < 2 * len(IDS):
            ports.add(free_port())
        ports = sorted(ports)
        self.client_port = dict(zip(IDS, ports[:len(IDS)]))
        self.quorum_port = dict(zip(IDS, ports[len(IDS):]))
        self.links = {}          # (src, dst) -> LinkProxy to dst's quorum
        self.client_proxy = {}   # member -> LinkProxy to its client port
        self.members = {}

    async def start(self):
        for src in IDS:
            for dst in IDS:
                if src != dst:
                    p = LinkProxy("127.0.0.1", self.quorum_port[dst],
                                  name="m%d->m%d" % (src, dst))
                    await p.start()
                    self.links[(src, dst)] = p
        for i in IDS:
            p = LinkProxy("127.0.0.1", self.client_port[i],
                          name="client->m%d" % i)
            await p.start()
            self.client_proxy[i] = p
        for i in IDS:
            await self.start_member(i)
        return self

    def data_dir(self, i):
        return os.path.join(self.base_dir, "m%d" % i)

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
            snapshot_entries=self.snapshot_entries)
        await srv.start()
        self.members[i] = srv
        return srv

    async def stop_member(self, i):
        srv = self.members.pop(i)
        await srv.stop()

    async def stop(self):
        for i in list(self.members):
            await self.stop_member(i)
        for p in list(self.links.values()) + list(self.client_proxy.values()):
            await p.close()

    def addr(self, i):
        return "127.0.0.1:%d" % self.client_port[i]

    @property
    def conn_str(self):
        return ",".join(self.addr(i) for i in IDS)

    @property
    def proxied_conn_str(self):
        return ",".join(self.client_proxy[i].addr for i in IDS)

    def hold_off_clients(self):
        for p in self.client_proxy.values():
            p.set_drops(to_server=True, to_client=True)

    def admit_clients(self):
        for p in self.client_proxy.values():
            p.heal()

    def cut_member(self, i):
        for (src, dst), p in self.links.items():
            if i in (src, dst):
                p.set_drops(to_server=True, to_client=True)

    def heal_members(self):
        for p in self.links.values():
            p.heal()

    def serving(self):
        return [i for i, s in self.members.items() if s.serving]

    async def wait_leader(self, timeout_s=10.0, among=None):
        deadline = time.monotonic() + timeout_s
        while time.monotonic() < deadline:
            live = [i for i in self.serving()
                    if among is None or i in among]
            if live:
                return max(live, key=lambda i: self.members[i].epoch)
            await asyncio.sleep(0.01)
        raise AssertionError("no serving leader; roles=%r" % {
            i: (s.role, s.epoch) for i, s in self.members.items()})

    async def settled(self, timeout_s=10.0):
        """Wait until every running member has applied the same log."""
        deadline = time.monotonic() + timeout_s
        while time.monotonic() < deadline:
            lead = self.serving()
            if len(lead) == 1:
                top = self.members[lead[0]].core.last_index
                if all(s.applied_index == top and
                       s.core.last_index == top
                       for s in self.members.values()):
                    return
            await asyncio.sleep(0.02)
        raise AssertionError("ensemble did not settle: %r" % {
            i: (s.role, s.epoch, s.applied_index, s.core.last_index)
            for i, s in self.members.items()})

    def dumps(self):
        return {i: s.dump_full() for i, s in self.members.items()}

    def assert_identical(self):
        dumps = list(self.dumps().values())
        assert len(dumps) >= 2
        for d in dumps[1:]:
            assert d == dumps[0]
        return dumps[0]


async def _client(conn_str, timeout_ms=SESSION_MS, events=None):
    cli = ZkClient(conn_str, session_timeout_ms=timeout_ms,
                   on_session=(events.append if events is not None
                               else None))
    await cli.connect(timeout_s=10.0)
    return cli


async def _retry(op, timeout_s):
    """Run ``op`` until it stops failing with a ZkError."""
    deadline = time.monotonic() + timeout_s
    while True:
        try:
            return await op()
        except ZkError:
            if time.monotonic() > deadline:
                raise
            await asyncio.sleep(0.01)


async def _four_letter(addr, word):
    host, _, port = addr.rpartition(":")
    r, w = await asyncio.open_connection(host, int(port))
    w.write(word)
    await w.drain()
    out = await asyncio.wait_for(r.read(), 5.0)      # until the server closes
    w.close()
    return out


def test_crud_and_replica_identity(tmp_path):
    async def go():
        ens = await Ensemble(tmp_path).start()
        clis = []
        try:
            await ens.wait_leader()
            cli = await _client(ens.conn_str)
            cli2 = await _client(ens.conn_str)
            clis += [cli, cli2]
            assert cli.session_id != cli2.session_id
            await cli.mkdirp("/manatee/1.moray/election")
            assert await cli.create("/manatee/1.moray/state",
                                    b'{"generation":1}') \
                == "/manatee/1.moray/state"
            data, stat = await cli.get_data("/manatee/1.moray/state")
            assert data == b'{"generation":1}' and stat.version == 0
            # zxid = (epoch << 32) | counter
            assert stat.czxid >> 32 == ens.members[
                await ens.wait_leader()].epoch
            # CAS
            st2 = await cli.set_data("/manatee/1.moray/state",
                                     b'{"generation":2}', version=0)
            assert st2.version == 1 and st2.mzxid > stat.mzxid
            with pytest.raises(ZkError) as ei:
                await cli.set_data("/manatee/1.moray/state", b"x", version=0)
            assert ei.value.code == jute.ZBADVERSION
            with pytest.raises(ZkError) as ei:
                await cli.create("/manatee/1.moray/state", b"")
            assert ei.value.code == jute.ZNODEEXISTS
            with pytest.raises(ZkError) as ei:
                await cli.delete("/manatee/1.moray")
            assert ei.value.code == jute.ZNOTEMPTY
            # multi: history node + versioned state write, atomically
            res = await cli.multi([
                MultiOp.create("/manatee/1.moray/history", b""),
                MultiOp.create("/manatee/1.moray/history/2-", b"h",
                               jute.PERSISTENT_SEQUENTIAL),
                MultiOp.set_data("/manatee/1.moray/state",
                                 b'{"generation":3}', version=1)])
            assert res[1] == ("create",
                              "/manatee/1.moray/history/2-0000000000")
            hist, hstat = await cli.get_data(
                "/manatee/1.moray/history/2-0000000000")
            _d, sstat = await cli.get_data("/manatee/1.moray/state")
            assert hstat.czxid == sstat.mzxid      # one zxid for the multi
            # a failing multi changes nothing
            with pytest.raises(ZkError) as ei:
                await cli.multi([
                    MultiOp.create("/manatee/1.moray/other", b""),
                    MultiOp.set_data("/manatee/1.moray/state", b"no",
                                     version=0)])
            assert ei.value.code == jute.ZBADVERSION
            assert await cli.exists("/manatee/1.moray/other") is None
            # ephemeral-sequential election
            p1 = await cli.create("/manatee/1.moray/election/a-", b"1",
                                  mode=jute.EPHEMERAL_SEQUENTIAL)
            p2 = await cli2.create("/manatee/1.moray/election/b-", b"2",
                                   mode=jute.EPHEMERAL_SEQUENTIAL)
            assert p1.endswith("a-0000000000")
            assert p2.endswith("b-0000000001")
            fired = []
            kids, _ = await cli.get_children(
                "/manatee/1.moray/election",
                watch=lambda e, p: fired.append((e, p)))
            assert len(kids) == 2
            await cli2.close()
            clis.remove(cli2)
            await _retry_until(lambda: fired, 5.0)
            kids, _ = await cli.get_children("/manatee/1.moray/election")
            assert kids == [p1.rsplit("/", 1)[1]]
            await cli.delete("/manatee/1.moray/history/2-0000000000")

            await ens.settled()
            full = ens.assert_identical()
            assert len(ens.members) == 3
            node = full["nodes"]["/manatee/1.moray/election"]
            assert node["next_seq"] == 2
            assert full["nodes"][p1]["ephemeralOwner"] == cli.session_id
        finally:
            for c in clis:
                await c.close()
            await ens.stop()
    run(go())


async def _retry_until(pred, timeout_s):
    deadline = time.monotonic() + timeout_s
    while not pred():
        assert time.monotonic() < deadline, "condition never became true"
        await asyncio.sleep(0.01)


def test_followers_do_not_serve(tmp_path):
    async def go():
        ens = await Ensemble(tmp_path).start()
        try:
            lead = await ens.wait_leader()
            follower = [i for i in IDS if i != lead][0]
            lone = ZkClient(ens.addr(follower), session_timeout_ms=SESSION_MS)
            with pytest.raises(asyncio.TimeoutError):
                await lone.connect(timeout_s=1.0)
            assert lone.session_id == 0
            await lone.close()
            assert ens.members[follower].stats["requests"] == 0
            cli = await _client(ens.conn_str)
            try:
                await cli.create("/x", b"1")
                assert ens.members[lead].sessions[cli.session_id].conn \
                    is not None
                for i in IDS:
                    if i != lead:
                        assert ens.members[i].stats["requests"] == 0
            finally:
                await cli.close()
        finally:
            await ens.stop()
    run(go())


def test_leader_stop_without_session_loss(tmp_path):
    async def go():
        ens = await Ensemble(tmp_path).start()
        events = []
        cli = other = None
        try:
            lead = await ens.wait_leader()
            cli = await _client(ens.conn_str, events=events)
            sid = cli.session_id
            await cli.create("/watched", b"0")
            eph = await cli.create("/eph-", b"", mode=jute.EPHEMERAL_SEQUENTIAL)
            fired = []
            await cli.get_data("/watched",
                               watch=lambda e, p: fired.append((e, p)))

            # one timeout to notice, three election rounds, plus the
            # client's 1.0 s reconnect back-off cap
            bound = 4 * EL_MAX_MS / 1000.0 + 1.0
            t0 = time.monotonic()
            await ens.stop_member(lead)
            await _retry(lambda: cli.exists("/watched"), bound)
            usable_after = time.monotonic() - t0
            print("client usable again after %.3fs (bound %.3fs)"
                  % (usable_after, bound))
            assert usable_after < bound
            assert cli.session_id == sid
            assert await cli.exists(eph) is not None
            new_lead = await ens.wait_leader()
            assert new_lead != lead

            # the watch from before the stop fires for a change after it
            other = await _client(ens.conn_str)
            await other.set_data("/watched", b"1")
            await _retry_until(lambda: fired, 5.0)
            assert fired == [(jute.EVENT_NODE_DATA_CHANGED, "/watched")]
            assert "expired" not in events
            assert cli.state == "connected"
        finally:
            for c in (cli, other):
                if c is not None:
                    await c.close()
            await ens.stop()
    run(go())


def test_missed_event_fires_on_rearm(tmp_path):
    async def go():
        ens = await Ensemble(tmp_path).start()
        a = b = None
        try:
            await ens.wait_leader()
            a_events = []
            a = await _client(ens.proxied_conn_str, timeout_ms=6000,
                              events=a_events)
            b = await _client(ens.conn_str)
            await a.create("/n", b"0")
            await a.create("/kids", b"")
            got = []
            await a.get_data("/n", watch=lambda e, p: got.append((e, p)))
            await a.get_children("/kids",
                                 watch=lambda e, p: got.append((e, p)))
            await a.exists("/later", watch=lambda e, p: got.append((e, p)))
            await a.get_data("/kids", watch=lambda e, p: got.append(
                ("unchanged", e, p)))
            ens.hold_off_clients()
            await b.set_data("/n", b"1")
            await b.create("/kids/c", b"")
            await b.create("/later", b"")
            await asyncio.sleep(0.2)
            assert got == []           # A is cut off: it heard nothing
            ens.admit_clients()
            await _retry_until(lambda: len(got) >= 3, 8.0)
            assert sorted(got) == sorted([
                (jute.EVENT_NODE_DATA_CHANGED, "/n"),
                (jute.EVENT_NODE_CHILDREN_CHANGED, "/kids"),
                (jute.EVENT_NODE_CREATED, "/later")])
            assert "expired" not in a_events
            # the watch on unchanged data was registered, not fired
            await b.set_data("/kids", b"x")
            await _retry_until(lambda: len(got) >= 4, 5.0)
            assert got[-1] == ("unchanged", jute.EVENT_NODE_DATA_CHANGED,
                               "/kids")
        finally:
            for c in (a, b):
                if c is not None:
                    await c.close()
            await ens.stop()
    run(go())


def test_expiry_is_replicated_and_not_early(tmp_path):
    async def go():
        ens = await Ensemble(tmp_path).start()
        a = None
        try:
            lead = await ens.wait_leader()
            timeout_s = SESSION_MS / 1000.0
            a_events = []
            a = await _client(ens.proxied_conn_str, events=a_events)
            sid = a.session_id
            eph = await a.create("/eph", b"", mode=jute.EPHEMERAL)
            await ens.settled()
            # A goes silent (no close), and 0.6 timeouts later the leader
            # — the only member that knew how long A had been silent —
            # is stopped
            ens.hold_off_clients()
            await asyncio.sleep(0.6 * timeout_s)
            await ens.stop_member(lead)
            new_lead = await ens.wait_leader()
            t1 = time.monotonic()
            # 0.7 timeouts into the new reign A has been silent for more
            # than a whole timeout, yet must not be expired: its clock
            # restarted when the new leader began serving
            await asyncio.sleep(0.7 * timeout_s)
            assert time.monotonic() - t1 < timeout_s
            for s in ens.members.values():
                assert sid in s.sessions
                assert eph in s.nodes
            # ...and after a full timeout it is, on every replica
            deadline = t1 + timeout_s + 2.0
            while any(eph in s.nodes or sid in s.sessions
                      for s in ens.members.values()):
                assert time.monotonic() < deadline, "session never expired"
                await asyncio.sleep(0.02)
            assert time.monotonic() - t1 >= timeout_s
            assert ens.members[new_lead].stats["expired_sessions"] == 1
            await ens.settled()
            ens.assert_identical()
            # the client learns it from a server, on reconnect
            ens.admit_clients()
            await _retry_until(lambda: "expired" in a_events, 8.0)
        finally:
            if a is not None:
                await a.close()
            await ens.stop()
    run(go())


def test_minority_serves_nothing(tmp_path):
    async def go():
        ens = await Ensemble(tmp_path).start()
        cli = c2 = None
        try:
            lead = await ens.wait_leader()
            cli = await _client(ens.addr(lead), timeout_ms=6000)
            acked = []
            for k in range(5):
                await cli.create("/w%d" % k, b"%d" % k)
                acked.append("/w%d" % k)
            others = [i for i in IDS if i != lead]
            for i in others:
                await ens.stop_member(i)
            # a write through the survivor gets no ack
            with pytest.raises(ZkError) as ei:
                await cli.create("/minority", b"")
            assert ei.value.code in (jute.ZCONNECTIONLOSS,
                                     jute.ZOPERATIONTIMEOUT)
            await asyncio.sleep(EL_MAX_MS / 1000.0)
            assert ens.serving() == []
            lone = ZkClient(ens.addr(lead), session_timeout_ms=SESSION_MS)
            with pytest.raises(asyncio.TimeoutError):
                await lone.connect(timeout_s=1.0)
            await lone.close()
            assert cli.state != "connected"
            # a majority again: everything acked is there, writes work
            await ens.start_member(others[0])
            await ens.wait_leader()
            c2 = await _client(ens.conn_str)
            for path in acked:
                assert await c2.exists(path) is not None
            await c2.create("/after", b"")
            await ens.settled()
            ens.assert_identical()
        finally:
            for c in (cli, c2):
                if c is not None:
                    await c.close()
            await ens.stop()
    run(go())


def test_stale_leader_steps_down_and_loses_its_write(tmp_path):
    async def go():
        ens = await Ensemble(tmp_path).start()
        c_old = c_new = None
        try:
            old = await ens.wait_leader()
            others = [i for i in IDS if i != old]
            events = []
            c_old = await _client(ens.addr(old), timeout_ms=6000)
            c_old.on_session = lambda ev: events.append(
                (ev, time.monotonic()))
            await c_old.create("/base", b"")
            await ens.settled()

            # record, at the very calls, when the old leader severs its
            # clients and when a successor first serves — and what the
            # old leader looked like at that moment
            marks = {}
            old_srv = ens.members[old]

            def on_stop(orig=old_srv._stop_serving):
                marks.setdefault("old_stopped", time.monotonic())
                orig()
            old_srv._stop_serving = on_stop
            for i in others:
                def on_begin(epoch, orig=ens.members[i]._begin_serving):
                    if "new_serving" not in marks:
                        marks["new_serving"] = time.monotonic()
                        marks["old_serving_then"] = old_srv.serving
                        # (a bare TCP connection may exist: the client
                        # keeps knocking and is turned away unanswered)
                        marks["old_conns_then"] = sum(
                            1 for sess in old_srv.sessions.values()
                            if sess.conn is not None)
                        marks["old_role_then"] = old_srv.role
                    orig(epoch)
                ens.members[i]._begin_serving = on_begin

            epoch_before = old_srv.epoch
            ens.cut_member(old)
            t_cut = time.monotonic()
            with pytest.raises(ZkError) as ei:
                await c_old.create("/stale", b"")
            assert ei.value.code == jute.ZCONNECTIONLOSS
            t_closed = [t for ev, t in events if ev == "disconnected"][0]
            # the lease is the MINIMUM election timeout, counted from the
            # send time of the last acknowledged heartbeat — which is
            # before the cut.  On top of it: the member's tick period
            # (10 ms here: min(heartbeat, el_min / 10) / 2), a few of
            # them for event-loop scheduling.  Well under EL_MAX, so a
            # lease keyed to anything longer than the minimum fails here.
            lease = EL_MIN_MS / 1000.0
            tick = 0.010
            print("old leader closed its clients %.3fs after the cut "
                  "(lease %.3fs)" % (t_closed - t_cut, lease))
            assert t_closed - t_cut < lease + 5 * tick
            assert lease + 5 * tick < EL_MAX_MS / 1000.0
            assert not old_srv.serving

            new = await ens.wait_leader(among=others)
            # nobody served while the old leader still could: it had
            # stopped, and dropped every client, BEFORE the successor's
            # first moment of serving.  Pure ordering — no slack.
            assert marks["old_stopped"] < marks["new_serving"]
            assert marks["old_serving_then"] is False
            assert marks["old_conns_then"] == 0
            assert marks["old_role_then"] != "leader"
            assert ens.members[new].epoch > epoch_before
            c_new = await _client(",".join(ens.addr(i) for i in others))
            await c_new.create("/fresh", b"")

            ens.heal_members()
            await ens.settled()
            full = ens.assert_identical()
            assert len(ens.members) == 3
            assert "/fresh" in full["nodes"] and "/base" in full["nodes"]
            assert "/stale" not in full["nodes"]
            assert ens.members[old].role == "follower"
        finally:
            for c in (c_old, c_new):
                if c is not None:
                    await c.close()
            await ens.stop()
    run(go())


def test_restart_and_compaction(tmp_path):
    async def go():
        ens = await Ensemble(tmp_path, snapshot_entries=10).start()
        cli = None
        try:
            await ens.wait_leader()
            cli = await _client(ens.conn_str)
            await cli.mkdirp("/shard/election")
            await cli.create("/shard/state", b"0")
            for k in range(12):
                p = await cli.create("/shard/election/p-", b"%d" % k,
                                     mode=jute.EPHEMERAL_SEQUENTIAL)
                assert p.endswith("%010d" % k)
                await cli.set_data("/shard/state", b"%d" % k)
                if k % 2:
                    await cli.delete(p)
            q = [await cli.create("/shard/q-", b"",
                                  mode=jute.PERSISTENT_SEQUENTIAL)
                 for _ in range(5)]
            for p in q:
                await cli.delete(p)
            await cli.close()       # its ephemerals go, by a logged txn
            cli = None
            await ens.settled()
            before = ens.assert_identical()
            assert before["sessions"] == {}
            assert before["nodes"]["/shard/election"]["children"] == []
            assert before["nodes"]["/shard/election"]["next_seq"] == 12
            for s in ens.members.values():
                # truncated several times, on every member
                assert s.stats["snapshots_written"] >= 3
                assert len(s.core.log) <= 11

            for i in IDS:
                await ens.stop_member(i)
            for i in IDS:
                await ens.start_member(i)
            await ens.wait_leader()
            await ens.settled()
            after = ens.assert_identical()
            assert after["nodes"] == before["nodes"]
            cli = await _client(ens.conn_str)
            assert (await cli.create("/shard/q-", b"",
                                     mode=jute.PERSISTENT_SEQUENTIAL)) \
                == "/shard/q-0000000005"
            assert (await cli.create("/shard/election/p-", b"",
                                     mode=jute.EPHEMERAL_SEQUENTIAL)) \
                .endswith("p-0000000012")

            # a member replaced with an empty data directory is caught
            # up by snapshot (the log it would need is truncated)
            lead = await ens.wait_leader()
            victim = [i for i in IDS if i != lead][0]
            await ens.stop_member(victim)
            shutil.rmtree(ens.data_dir(victim))
            fresh = await ens.start_member(victim)
            await ens.settled()
            assert fresh.stats["snapshots_installed"] >= 1
            ens.assert_identical()

            # a torn last entry (kill -9 mid-append) is cut away
            await cli.close()
            cli = None
            await ens.settled()
            whole = ens.assert_identical()
            for i in IDS:
                await ens.stop_member(i)
            with open(os.path.join(ens.data_dir(victim), "log.jsonl"),
                      "ab") as f:
                f.write(b'[99999,1,{"op":"create","zxid":1,"pa')
            for i in IDS:
                await ens.start_member(i)
            await ens.wait_leader()
            await ens.settled()
            assert ens.assert_identical()["nodes"] == whole["nodes"]
        finally:
            if cli is not None:
                await cli.close()
            await ens.stop()
    run(go())


def test_torn_log_tail_recovers_to_last_whole_entry(tmp_path):
    d = str(tmp_path / "m")
    disk = MemberDisk(d, null_logger())
    assert disk.load()["log"] == []
    disk.save_meta(3, 2)
    disk.append(1, [(1, None), (1, {"op": "delete", "zxid": 5,
                                    "path": "/a"})])
    disk.append(3, [(2, {"op": "delete", "zxid": 6, "path": "/b"})])
    # a conflicting suffix from a deposed leader is cut before appending
    disk.append(2, [(3, None)])
    disk.close()
    with open(os.path.join(d, "log.jsonl"), "ab") as f:
        f.write(b'[3,3,{"op":"del')
    disk = MemberDisk(d, null_logger())
    st = disk.load()
    assert (st["epoch"], st["voted_for"]) == (3, 2)
    assert st["log"] == [(1, None), (3, None)]
    # and the file is whole again: appending after recovery works
    disk.append(3, [(3, {"op": "delete", "zxid": 7, "path": "/c"})])
    disk.close()
    st = MemberDisk(d, null_logger()).load()
    assert [e for e, _p in st["log"]] == [1, 3, 3]
    assert st["log"][2][1]["path"] == "/c"


def test_four_letter_words(tmp_path):
    async def go():
        ens = await Ensemble(tmp_path).start()
        cli = None
        try:
            lead = await ens.wait_leader()
            cli = await _client(ens.conn_str)
            await cli.create("/x", b"")
            await ens.settled()
            modes = {}
            for i in IDS:
                assert await _four_letter(ens.addr(i), b"ruok") == b"imok"
                text = (await _four_letter(ens.addr(i), b"srvr")).decode()
                fields = dict(line.split(": ", 1)
                              for line in text.splitlines() if ": " in line)
                modes[i] = fields["Mode"]
                assert int(fields["Epoch"]) == ens.members[lead].epoch
                assert int(fields["Zxid"], 16) == ens.members[lead].zxid
                assert int(fields["Sessions"]) == 1
            assert modes[lead] == "leader"
            assert sorted(modes.values()) == ["follower", "follower",
                                              "leader"]
        finally:
            if cli is not None:
                await cli.close()
            await ens.stop()
    run(go())


def test_multi_ops_see_each_other_in_order(tmp_path):
    """Validation inside a multi follows sequential semantics."""
    async def go():
        ens = await Ensemble(tmp_path).start()
        cli = None
        try:
            await ens.wait_leader()
            cli = await _client(ens.conn_str)
            await cli.mkdirp("/p/c1")
            await cli.create("/p/c2", b"")
            # children first, then the parent, in one transaction
            await cli.multi([MultiOp.delete("/p/c1"),
                             MultiOp.delete("/p/c2"),
                             MultiOp.delete("/p")])
            assert await cli.exists("/p") is None
            # a node made here: its version moves with each setData
            await cli.multi([MultiOp.create("/n", b"0"),
                             MultiOp.set_data("/n", b"1", version=0),
                             MultiOp.set_data("/n", b"2", version=1),
                             MultiOp.check("/n", version=2)])
            data, stat = await cli.get_data("/n")
            assert data == b"2" and stat.version == 2
            with pytest.raises(ZkError) as ei:
                await cli.multi([MultiOp.set_data("/n", b"3", version=2),
                                 MultiOp.set_data("/n", b"4", version=2)])
            assert ei.value.code == jute.ZBADVERSION
            with pytest.raises(ZkError) as ei:
                await cli.multi([MultiOp.create("/q", b""),
                                 MultiOp.create("/q/k", b""),
                                 MultiOp.delete("/q")])
            assert ei.value.code == jute.ZNOTEMPTY
            assert await cli.exists("/q") is None
            assert (await cli.get_data("/n"))[0] == b"2"
            await ens.settled()
            ens.assert_identical()
        finally:
            if cli is not None:
                await cli.close()
            await ens.stop()
    run(go())


def test_failed_multi_fires_no_watch(tmp_path):
    """A multi whose second op fails is never logged: no watcher hears
    of its first op and the node reads back unchanged, on every member.
    Then a multi that makes a parent and its child is accepted."""
    async def go():
        ens = await Ensemble(tmp_path).start()
        cli = watcher = None
        events = []
        try:
            lead = ens.members[await ens.wait_leader()]
            cli = await _client(ens.conn_str)
            watcher = await _client(ens.conn_str)
            await cli.create("/x", b"0")
            root_children = asyncio.get_running_loop().create_future()

            def on_event(etype, path):
                events.append((etype, path))
                if (etype, path) == (jute.EVENT_NODE_CHILDREN_CHANGED, "/") \
                        and not root_children.done():
                    root_children.set_result(None)

            for path in ("/x", "/"):
                await watcher.get_data(path, watch=on_event)
                await watcher.get_children(path, watch=on_event)
            fired = lead.stats["watch_events"]
            proposals = lead.stats["proposals"]
            with pytest.raises(ZkError) as ei:
                await cli.multi([MultiOp.set_data("/x", b"1", version=0),
                                 MultiOp.set_data("/x", b"2", version=0)])
            assert ei.value.code == jute.ZBADVERSION
            # an event is written to the watcher's connection when the
            # write is applied, so one would be ahead of this reply
            data, stat = await watcher.get_data("/x")
            assert events == []
            assert lead.stats["watch_events"] == fired
            assert lead.stats["proposals"] == proposals
            assert (data, stat.version, stat.mzxid) == (b"0", 0, stat.czxid)

            res = await cli.multi([MultiOp.create("/p", b"P"),
                                   MultiOp.create("/p/c", b"C")])
            assert res == [("create", "/p"), ("create", "/p/c")]
            assert (await cli.get_data("/p"))[0] == b"P"
            assert (await cli.get_data("/p/c"))[0] == b"C"
            assert (await cli.get_children("/p"))[0] == ["c"]
            await asyncio.wait_for(root_children, 5)
            assert events == [(jute.EVENT_NODE_CHILDREN_CHANGED, "/")]
            await ens.settled()
            full = ens.assert_identical()
            assert full["nodes"]["/x"]["version"] == 0
        finally:
            for c in (cli, watcher):
                if c is not None:
                    await c.close()
            await ens.stop()
    run(go())


def test_no_ephemeral_for_a_session_whose_close_is_already_logged(tmp_path):
    """A create that reaches the head of the proposal queue after its own
    session's close must not leave an ownerless ephemeral behind."""
    async def go():
        ens = await Ensemble(tmp_path).start()
        cli = None
        try:
            lead = ens.members[await ens.wait_leader()]
            cli = await _client(ens.conn_str)
            sid = cli.session_id
            await cli.create("/own", b"", mode=jute.EPHEMERAL)
            # queue, back to back: the expiry of cli's session, then an
            # ephemeral create and a multi from that same session
            closing = asyncio.ensure_future(lead._submit(
                lambda zxid, _now: {"op": "session_close", "zxid": zxid,
                                    "sid": sid}))

            def prep_create(zxid, now_ms):
                txn = lead._prep_create("/ghost", b"", jute.EPHEMERAL, sid)
                txn.update(zxid=zxid, time=now_ms)
                return txn

            def prep_multi(zxid, now_ms):
                return {"op": "multi", "zxid": zxid, "time": now_ms,
                        "ops": lead._prep_multi(
                            [MultiOp.create("/ghost2", b"", jute.EPHEMERAL)],
                            sid)}
            late = [asyncio.ensure_future(lead._submit(p))
                    for p in (prep_create, prep_multi)]
            await closing
            for fut in late:
                with pytest.raises(ZkError) as ei:
                    await fut
                assert ei.value.code == jute.ZSESSIONEXPIRED
            await ens.settled()
            full = ens.assert_identical()
            assert full["sessions"] == {}
            assert not [p for p, n in full["nodes"].items()
                        if n["ephemeralOwner"]]
        finally:
            if cli is not None:
                await cli.close()
            await ens.stop()
    run(go())


def test_member_that_cannot_persist_halts_and_run_member_exits_nonzero(
        tmp_path):
    from manatee_amd.coord.zkquorum import run_member

    async def go():
        ens = await Ensemble(tmp_path).start()
        cli = None
        try:
            lead = await ens.wait_leader()
            victim = [i for i in IDS if i != lead][0]
            cli = await _client(ens.conn_str)
            await cli.create("/a", b"")
            await ens.settled()

            def full_disk(start, entries):
                raise OSError(28, "No space left on device")
            ens.members[victim].disk.append = full_disk
            await cli.create("/b", b"")          # the other two still agree
            srv = ens.members[victim]
            await asyncio.wait_for(srv.halted.wait(), 5.0)
            assert srv.role == "halted" and not srv.serving
            assert await _four_letter(ens.addr(victim), b"ruok") != b"imok"
            text = (await _four_letter(ens.addr(victim), b"srvr")).decode()
            assert "Mode: halted" in text
            assert "/b" not in srv.nodes
            await cli.create("/c", b"")
            assert await _four_letter(ens.addr(lead), b"ruok") == b"imok"
        finally:
            if cli is not None:
                await cli.close()
            await ens.stop()

        # the process entry point turns the halt into a non-zero exit
        port, qport = free_port(), free_port()
        solo = ZkQuorumServer(
            1, client_port=port, peers={1: ("127.0.0.1", qport)},
            data_dir=str(tmp_path / "solo"),
            election_timeout_ms=(EL_MIN_MS, EL_MAX_MS),
            heartbeat_ms=HEARTBEAT_MS)

        def read_only(start, entries):
            raise OSError(30, "Read-only file system")
        solo.disk.append = read_only     # hit by its first election no-op
        assert await asyncio.wait_for(run_member(solo), 10.0) == 1
    run(go())
