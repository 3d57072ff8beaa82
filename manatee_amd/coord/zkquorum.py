"""Replicated coordination server: N ``ZkServer``s that agree on one log.

``ZkQuorumServer`` is the ZooKeeper client front-end and znode tree of
``zkserver.ZkServer`` driven by the consensus core in ``quorum.py``.
An odd, static set of members (three is the tested shape) elects a
leader; only the leader serves clients — reads included — and every
write is a log entry that a majority has fsynced before the client sees
the reply.  A member that is not the serving leader accepts a client's
TCP connection and closes it at once, so ``ZkClient`` (or any stock
ZooKeeper client) moves on to the next address of its connection string.

The log carries OUTCOMES, not requests: a create with its final,
already-sequenced path, its ctime and its zxid; a setData with its mtime;
session open/close (close is also expiry, and applying it deletes the
session's ephemerals on every replica alike).  Every ``Stat`` field and
sequence counter comes out of the entry, never from a replica's own
clock or counter, so the replicas stay byte-identical (``dump_full()``).

Sessions are replicated; their liveness is known to the leader only, and
a new leader restarts every session's clock at one full timeout.
With ``disconnect_grace_ms`` set, the serving leader also expires a
session whose client closed its connection (FIN or RST) and did not
re-attach within the grace; that observation is leader-local, never
logged or snapshotted, and a new leader starts without it.
Watches belong to a connection and die with it; a reconnecting client
re-arms them with SetWatches and its last seen zxid, and whatever it
missed fires at once.

Each member keeps, in its data directory: ``meta.json`` (epoch + vote),
``log.jsonl`` (append-only, fsynced before any acknowledgement) and
``snapshot.json`` (tree + sessions, written tmp/fsync/rename; the log is
cut behind it once it grows past ``snapshot_entries``).

    python -m manatee_amd.coord.zkquorum --id 1 --client 10.0.0.1:2181 \\
        --peers 1=10.0.0.1:2888,2=10.0.0.2:2888,3=10.0.0.3:2888 \\
        --data-dir /var/lib/manatee-zk
"""

from __future__ import annotations

import asyncio
import json
import os
import random
import struct
import time
from typing import Any, Callable, Dict, List, Optional, Set, Tuple

from ..common import dial
from ..common.logging import Logger, null_logger
from . import jute
from .jute import Reader, ZkError, ZOK, ZSESSIONEXPIRED, ZMARSHALLINGERROR
from .quorum import LEADER, QuorumCore
from .zkserver import ZkServer, _Node, _Session, _parent

FOUR_LETTER_WORDS = (b"ruok", b"srvr")
_WRITE_OPS = (jute.OP_CREATE, jute.OP_DELETE, jute.OP_SETDATA,
              jute.OP_MULTI)
_MAX_PEER_FRAME = 64 * 1024 * 1024


class _NotServing(Exception):
    """This member cannot (or can no longer) answer: drop the client
    connection WITHOUT a reply — the outcome is unknown to the client,
    which is what connection loss means."""


def _fsync_dir(path: str) -> None:
    try:
        fd = os.open(path, os.O_RDONLY)
    except OSError:
        return
    try:
        os.fsync(fd)
    except OSError:
        pass
    finally:
        os.close(fd)


class MemberDisk:
    """One member's data directory."""

    def __init__(self, data_dir: str, log: Logger):
        self.dir = data_dir
        self.log = log
        self.meta_path = os.path.join(data_dir, "meta.json")
        self.log_path = os.path.join(data_dir, "log.jsonl")
        self.snap_path = os.path.join(data_dir, "snapshot.json")
        self._f = None
        self._offsets: List[int] = []    # byte offset of each held entry
        self.base_index = 0

    def _write_atomic(self, path: str, obj: Any) -> None:
        tmp = path + ".tmp"
        with open(tmp, "w") as f:
            json.dump(obj, f, separators=(",", ":"))
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
        _fsync_dir(self.dir)

    def load(self) -> dict:
        os.makedirs(self.dir, exist_ok=True)
        epoch, voted = 0, None
        try:
            with open(self.meta_path) as f:
                m = json.load(f)
            epoch, voted = int(m["epoch"]), m.get("voted_for")
        except FileNotFoundError:
            pass
        snapshot = None
        try:
            with open(self.snap_path) as f:
                snapshot = json.load(f)
        except FileNotFoundError:
            pass
        base = snapshot["index"] if snapshot else 0
        base_epoch = snapshot["epoch"] if snapshot else 0
        entries: List[tuple] = []
        raw = b""
        try:
            with open(self.log_path, "rb") as f:
                raw = f.read()
        except FileNotFoundError:
            pass
        good = 0            # bytes of the file that parsed
        pos = 0
        while True:
            nl = raw.find(b"\n", pos)
            if nl < 0:
                break       # torn tail (no newline): a kill -9 mid-append
            try:
                idx, e, payload = json.loads(raw[pos:nl])
            except (ValueError, TypeError):
                break       # nothing after a bad line can be trusted
            if idx > base:
                if idx != base + len(entries) + 1:
                    break
                entries.append((int(e), payload))
            pos = good = nl + 1
        if good != len(raw):
            self.log.warn("log tail unparseable; cut at the last whole "
                          "entry", kept=len(entries),
                          dropped_bytes=len(raw) - good)
        self.base_index = base
        self._rewrite(entries)
        return {"epoch": epoch, "voted_for": voted, "base_index": base,
                "base_epoch": base_epoch, "log": entries,
                "snapshot": snapshot}

    def _rewrite(self, entries: List[tuple]) -> None:
        """Replace the log file with exactly ``entries`` (which start at
        base_index + 1)."""
        if self._f is not None:
            self._f.close()
        tmp = self.log_path + ".tmp"
        self._offsets = []
        with open(tmp, "wb") as f:
            off = 0
            for k, (e, payload) in enumerate(entries):
                line = self._line(self.base_index + 1 + k, e, payload)
                self._offsets.append(off)
                f.write(line)
                off += len(line)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, self.log_path)
        _fsync_dir(self.dir)
        self._f = open(self.log_path, "r+b")
        self._f.seek(0, os.SEEK_END)

    @staticmethod
    def _line(index: int, epoch: int, payload: Any) -> bytes:
        return json.dumps([index, epoch, payload],
                          separators=(",", ":")).encode() + b"\n"

    def save_meta(self, epoch: int, voted_for: Optional[int]) -> None:
        self._write_atomic(self.meta_path,
                           {"epoch": epoch, "voted_for": voted_for})

    def append(self, start: int, entries: List[tuple]) -> None:
        k = start - self.base_index - 1
        if k < len(self._offsets):
            # a deposed leader's uncommitted suffix: cut it
            self._f.truncate(self._offsets[k])
            del self._offsets[k:]
        self._f.seek(0, os.SEEK_END)
        off = self._f.tell()
        for j, (e, payload) in enumerate(entries):
            line = self._line(start + j, e, payload)
            self._offsets.append(off)
            self._f.write(line)
            off += len(line)
        self._f.flush()
        os.fsync(self._f.fileno())

    def save_snapshot(self, snapshot: dict, remaining: List[tuple]) -> None:
        """Snapshot first, then cut the log: a crash in between leaves
        entries the snapshot already covers, which load() skips."""
        self._write_atomic(self.snap_path, snapshot)
        self.base_index = snapshot["index"]
        self._rewrite(remaining)

    def close(self) -> None:
        if self._f is not None:
            self._f.close()
            self._f = None


class _PeerLink:
    """Outbound half of one member-to-member link: frames are written
    if the connection is up and DROPPED otherwise (the core re-sends on
    its own clock); a background task redials through common/dial."""

    def __init__(self, server: "ZkQuorumServer", peer_id: int,
                 host: str, port: int):
        self.server = server
        self.peer_id = peer_id
        self.host, self.port = host, port
        self.writer: Optional[asyncio.StreamWriter] = None
        self._task: Optional[asyncio.Task] = None

    def send(self, msg: dict) -> None:
        w = self.writer
        if w is None:
            if self._task is None or self._task.done():
                self._task = asyncio.get_running_loop().create_task(
                    self._connect())
            return
        body = json.dumps(msg, separators=(",", ":")).encode()
        try:
            if w.transport.get_write_buffer_size() > 8 * 1024 * 1024:
                raise ConnectionError("peer not draining")
            w.write(struct.pack(">I", len(body)) + body)
        except (ConnectionError, OSError, RuntimeError):
            self._drop(w)

    def _drop(self, w) -> None:
        if self.writer is w:
            self.writer = None
        try:
            w.transport.abort()
        except Exception:
            pass

    async def _connect(self) -> None:
        backoff = 0.05
        while self.server._running and self.writer is None:
            w = None
            try:
                r, w = await asyncio.wait_for(
                    dial.open_connection(self.host, self.port), 2.0)
                hello = json.dumps({"hello": self.server.server_id}).encode()
                w.write(struct.pack(">I", len(hello)) + hello)
                self.writer = w
            except (OSError, asyncio.TimeoutError):
                if w is not None:
                    w.close()
                await asyncio.sleep(backoff)
                backoff = min(backoff * 2, 0.5)
                continue
            # the peer never writes on this connection: a read returns
            # only when it is gone
            try:
                while await r.read(4096):
                    pass
            except (ConnectionError, OSError):
                pass
            self._drop(w)
            return

    def close(self) -> None:
        if self._task is not None:
            self._task.cancel()
        if self.writer is not None:
            self._drop(self.writer)


class ZkQuorumServer(ZkServer):
    """One member of a replicated coordination ensemble."""

    def __init__(self, server_id: int,
                 client_host: str = "127.0.0.1", client_port: int = 0,
                 peers: Optional[Dict[int, Tuple[str, int]]] = None,
                 data_dir: Optional[str] = None,
                 election_timeout_ms: Tuple[int, int] = (1000, 2000),
                 heartbeat_ms: int = 100,
                 snapshot_entries: int = 1000,
                 log: Optional[Logger] = None,
                 min_session_timeout_ms: int = 1000,
                 max_session_timeout_ms: int = 120000,
                 disconnect_grace_ms: Optional[int] = None):
        super().__init__(host=client_host, port=client_port, log=log,
                         min_session_timeout_ms=min_session_timeout_ms,
                         max_session_timeout_ms=max_session_timeout_ms,
                         disconnect_grace_ms=disconnect_grace_ms)
        if not peers or server_id not in peers:
            raise ValueError("peers must list every member, this one "
                             "included")
        if len(peers) % 2 == 0:
            raise ValueError("an ensemble has an odd number of members")
        if not data_dir:
            raise ValueError("data_dir is required")
        if not 0 < election_timeout_ms[0] <= election_timeout_ms[1]:
            raise ValueError("election_timeout_ms is (min, max)")
        self.server_id = server_id
        self.peers = {int(k): (v[0], int(v[1])) for k, v in peers.items()}
        self.data_dir = data_dir
        self.election_timeout_ms = tuple(election_timeout_ms)
        self.heartbeat_ms = heartbeat_ms
        self.snapshot_entries = snapshot_entries
        self.log = (log or null_logger()).child(
            component="ZkQuorumServer", member=server_id)
        self.disk = MemberDisk(data_dir, self.log)
        self.core: Optional[QuorumCore] = None
        self.applied_index = 0
        self._running = False
        self._serving_epoch = 0         # 0 = not serving
        self._last_zxid_assigned = 0
        self._plock: Optional[asyncio.Lock] = None
        self._waiting: Dict[int, Tuple[int, asyncio.Future]] = {}
        self._client_conns: Set[asyncio.StreamWriter] = set()
        self._peer_conns: Set[asyncio.StreamWriter] = set()
        self._links: Dict[int, _PeerLink] = {}
        self._quorum_server: Optional[asyncio.AbstractServer] = None
        self._ticker: Optional[asyncio.Task] = None
        self._closing_sids: Set[int] = set()
        # set when the member can no longer persist and has stopped
        # taking part (see _pump); created in start()
        self.halted: Optional[asyncio.Event] = None
        self.halt_reason: Optional[str] = None
        self.stats.update({"proposals": 0, "elections_won": 0,
                           "snapshots_written": 0,
                           "snapshots_installed": 0})

    # ------------------------------------------------------------ lifecycle
    async def start(self) -> None:
        loop = asyncio.get_running_loop()
        st = self.disk.load()
        self._restore(st["snapshot"])
        self.applied_index = st["base_index"]
        self.core = QuorumCore(
            self.server_id, list(self.peers),
            random.Random(), time.monotonic(),
            election_timeout=(self.election_timeout_ms[0] / 1000.0,
                              self.election_timeout_ms[1] / 1000.0),
            heartbeat=self.heartbeat_ms / 1000.0,
            epoch=st["epoch"], voted_for=st["voted_for"], log=st["log"],
            base_index=st["base_index"], base_epoch=st["base_epoch"],
            snapshot=st["snapshot"])
        self._plock = asyncio.Lock()
        self.halted = asyncio.Event()
        self.halt_reason = None
        self._running = True
        qhost, qport = self.peers[self.server_id]
        self._quorum_server = await asyncio.start_server(
            self._handle_peer, qhost, qport)
        for pid, (h, p) in self.peers.items():
            if pid != self.server_id:
                self._links[pid] = _PeerLink(self, pid, h, p)
        self._server = await asyncio.start_server(
            self._handle_conn, self.host, self.port)
        self.port = self._server.sockets[0].getsockname()[1]
        self._ticker = loop.create_task(self._tick_loop())
        self._sweeper = loop.create_task(self._sweep_sessions())
        self.log.info("quorum member started", client=self.conn_str,
                      quorum="%s:%d" % (qhost, qport), epoch=st["epoch"],
                      log_entries=len(st["log"]),
                      snapshot_index=st["base_index"])

    async def stop(self) -> None:
        self._running = False
        self._stop_serving()
        for task in (self._ticker, self._sweeper):
            if task is not None:
                task.cancel()
                await asyncio.wait({task}, timeout=2.0)
        self._ticker = self._sweeper = None
        for link in self._links.values():
            link.close()
        self._links.clear()
        for w in list(self._peer_conns) + list(self._client_conns):
            try:
                w.transport.abort()
            except Exception:
                pass
        for srv in (self._server, self._quorum_server):
            if srv is not None:
                srv.close()
                try:
                    await asyncio.wait_for(srv.wait_closed(), 2.0)
                except (asyncio.TimeoutError, Exception):
                    pass
        self._server = self._quorum_server = None
        self.disk.close()

    # ----------------------------------------------------------- inspection
    @property
    def role(self) -> str:
        if self.halt_reason is not None:
            return "halted"
        return self.core.role if self.core is not None else "follower"

    @property
    def epoch(self) -> int:
        return self.core.epoch if self.core is not None else 0

    @property
    def last_applied_zxid(self) -> int:
        return self.zxid

    @property
    def serving(self) -> bool:
        return bool(self._serving_epoch) and self.core is not None and \
            self.core.role == LEADER and \
            self.core.epoch == self._serving_epoch and \
            self.core.has_lease(time.monotonic())

    def dump_full(self) -> dict:
        """The whole replicated state, Stats and sequence counters
        included — equal on every member once the ensemble is quiet."""
        nodes = {}
        for path, n in sorted(self.nodes.items()):
            nodes[path] = {
                "data": n.data.hex(), "czxid": n.stat_czxid,
                "mzxid": n.stat_mzxid, "pzxid": n.pzxid, "ctime": n.ctime,
                "mtime": n.mtime, "version": n.version,
                "cversion": n.cversion, "ephemeralOwner": n.ephemeral_owner,
                "next_seq": n.next_seq, "children": sorted(n.children)}
        sessions = {"0x%x" % s.sid: {"timeout_ms": s.timeout_ms,
                                     "ephemerals": sorted(s.ephemerals)}
                    for s in self.sessions.values()}
        return {"zxid": self.zxid, "nodes": nodes, "sessions": sessions}

    # ------------------------------------------------------------ snapshots
    def _make_snapshot(self) -> dict:
        nodes = {}
        for path, n in self.nodes.items():
            nodes[path] = [n.data.hex(), n.stat_czxid, n.stat_mzxid, n.pzxid,
                           n.ctime, n.mtime, n.version, n.cversion,
                           n.ephemeral_owner, n.next_seq]
        sessions = {str(s.sid): [s.passwd.hex(), s.timeout_ms]
                    for s in self.sessions.values()}
        return {"index": self.applied_index,
                "epoch": self.core.epoch_at(self.applied_index),
                "zxid": self.zxid, "nodes": nodes, "sessions": sessions}

    def _restore(self, snap: Optional[dict]) -> None:
        self.nodes = {"/": _Node(b"", 0, now_ms=0)}
        self.sessions = {}
        self.zxid = 0
        self.data_watches.clear()
        self.child_watches.clear()
        if not snap:
            return
        self.zxid = snap["zxid"]
        for sid, (passwd, timeout_ms) in snap["sessions"].items():
            self.sessions[int(sid)] = _Session(
                int(sid), bytes.fromhex(passwd), timeout_ms)
        self.nodes = {}
        for path, v in snap["nodes"].items():
            n = _Node(bytes.fromhex(v[0]), v[1], ephemeral_owner=v[8],
                      now_ms=v[4])
            (n.stat_mzxid, n.pzxid, n.mtime, n.version, n.cversion,
             n.next_seq) = v[2], v[3], v[5], v[6], v[7], v[9]
            self.nodes[path] = n
        for path, n in self.nodes.items():
            if path != "/":
                pp = _parent(path)
                self.nodes[pp].children.add(path[len(pp):].lstrip("/"))
            if n.ephemeral_owner in self.sessions:
                self.sessions[n.ephemeral_owner].ephemerals.add(path)

    # ---------------------------------------------------------- core driver
    async def _tick_loop(self) -> None:
        period = max(0.005, min(self.heartbeat_ms,
                                self.election_timeout_ms[0] / 10.0) / 2000.0)
        while self._running:
            await asyncio.sleep(period)
            if not self._running:
                return
            try:
                self.core.tick(time.monotonic())
                self._pump()
            except Exception as exc:
                self.log.error("quorum tick failed", err=exc)

    def _pump(self) -> None:
        """Carry out the core's effects, in order."""
        try:
            self._pump_effects()
        except OSError as exc:
            # the core is now ahead of the disk; a member that cannot
            # persist must not vote, acknowledge or serve again.  Halt:
            # `halted` is set (run_member exits non-zero on it, so the
            # service manager restarts the process), `ruok` stops
            # answering `imok` and `srvr` says `Mode: halted`.
            self.log.error("data directory write failed; member halted",
                           err=exc)
            self.halt_reason = "%s: %s" % (type(exc).__name__, exc)
            if self.halted is not None:
                self.halted.set()
            self._running = False
            self.core.drain()
            self._stop_serving()
            for w in list(self._peer_conns):
                try:
                    w.transport.abort()
                except Exception:
                    pass

    def _pump_effects(self) -> None:
        core = self.core
        for eff in core.drain():
            kind = eff[0]
            if kind == "send":
                link = self._links.get(eff[1])
                if link is not None:
                    link.send(eff[2])
            elif kind == "meta":
                self.disk.save_meta(eff[1], eff[2])
            elif kind == "append":
                self.disk.append(eff[1], eff[2])
            elif kind == "apply":
                self._apply(eff[1], eff[2], eff[3])
            elif kind == "role":
                self._on_role(eff[1], eff[2])
            elif kind == "serving":
                self._begin_serving(eff[1])
            elif kind == "snapshot":
                _k, index, _epoch, snap = eff
                self.disk.save_snapshot(snap, [])
                self._drop_all_clients()
                self._restore(snap)
                self.applied_index = index
                self.stats["snapshots_installed"] += 1
                self.log.info("snapshot installed", index=index)
        if len(core.log) > self.snapshot_entries and \
                self.applied_index > core.base_index:
            snap = self._make_snapshot()
            core.compact(self.applied_index, snap)
            self.disk.save_snapshot(snap, list(core.log))
            self.stats["snapshots_written"] += 1
            self.log.info("snapshot written; log truncated",
                          index=self.applied_index, kept=len(core.log))

    def _on_role(self, role: str, epoch: int) -> None:
        self.log.info("role change", role=role, epoch=epoch)
        if role == LEADER:
            self.stats["elections_won"] += 1
        else:
            self._stop_serving()

    def _begin_serving(self, epoch: int) -> None:
        # everything up to this epoch's no-op is applied: no client has
        # seen a zxid this member does not have.  Liveness was the old
        # leader's knowledge — every session gets one full timeout, and
        # this member has seen no client close anything.
        now = time.monotonic()
        for sess in self.sessions.values():
            sess.last_seen = now
            sess.conn = None
            sess.detached_at = None
        self._closing_sids.clear()
        self._last_zxid_assigned = self.zxid
        self._serving_epoch = epoch
        self.log.info("serving clients", epoch=epoch,
                      zxid="0x%x" % self.zxid, sessions=len(self.sessions))

    def _stop_serving(self) -> None:
        """Sever everything a leader owes its clients.  Does not rely on
        task cancellation: handlers re-check ``_serving_epoch`` after
        every await, and their transports are aborted here."""
        self._serving_epoch = 0
        waiting, self._waiting = self._waiting, {}
        for _epoch, fut in waiting.values():
            if not fut.done():
                fut.set_exception(_NotServing())
        self._drop_all_clients()

    def _drop_all_clients(self) -> None:
        for w in list(self._client_conns):
            try:
                w.transport.abort()
            except Exception:
                pass
        self._client_conns.clear()
        for sess in self.sessions.values():
            sess.conn = None
        self.data_watches.clear()
        self.child_watches.clear()

    # --------------------------------------------------------- peer traffic
    async def _handle_peer(self, reader: asyncio.StreamReader,
                           writer: asyncio.StreamWriter) -> None:
        self._peer_conns.add(writer)
        try:
            peer = None
            while self._running:
                hdr = await reader.readexactly(4)
                (n,) = struct.unpack(">I", hdr)
                if n > _MAX_PEER_FRAME:
                    return
                msg = json.loads(await reader.readexactly(n))
                if peer is None:
                    peer = msg.get("hello")
                    if peer not in self.peers or peer == self.server_id:
                        self.log.warn("quorum hello from a stranger",
                                      hello=peer)
                        return
                    continue
                if msg.get("from") != peer or not self._running:
                    return
                self.core.handle(msg, time.monotonic())
                self._pump()
        except (asyncio.IncompleteReadError, ConnectionError, OSError,
                ValueError):
            pass
        except Exception as exc:
            self.log.error("peer connection handler error", err=exc)
        finally:
            self._peer_conns.discard(writer)
            try:
                writer.close()
            except Exception:
                pass

    # ------------------------------------------------------------ proposals
    def _next_zxid(self) -> int:
        epoch = self.core.epoch
        last = max(self.zxid, self._last_zxid_assigned)
        zxid = last + 1 if (last >> 32) == epoch else (epoch << 32) | 1
        self._last_zxid_assigned = zxid
        return zxid

    async def _submit(self, prepare: Callable[[int, int], dict]) -> Any:
        """One proposal at a time: validate against applied state, log,
        replicate, wait for the majority, apply, return the outcome.
        ``prepare(zxid, now_ms)`` raises ZkError for a request that fails
        validation (nothing is logged then)."""
        async with self._plock:
            if not self.serving:
                raise _NotServing()
            epoch = self._serving_epoch
            assigned = self._last_zxid_assigned
            try:
                txn = prepare(self._next_zxid(), int(time.time() * 1000))
            except ZkError:
                self._last_zxid_assigned = assigned     # nothing was logged
                raise
            fut = asyncio.get_running_loop().create_future()
            index = self.core.last_index + 1
            self._waiting[index] = (epoch, fut)
            got = self.core.propose(txn, time.monotonic())
            if got is None:
                self._waiting.pop(index, None)
                self._pump()
                raise _NotServing()
            self.stats["proposals"] += 1
            self._pump()
            # resolved by _apply, or failed by _stop_serving — check-
            # quorum bounds the wait by the minimum election timeout
            return await fut

    def _apply(self, index: int, epoch: int, txn: Optional[dict]) -> None:
        result: Any = None
        if txn is not None:
            try:
                result = self._apply_txn(txn)
            except ZkError as exc:
                # cannot happen for a validated txn; identical on every
                # replica if it does
                self.log.error("txn failed to apply", index=index,
                               op=txn.get("op"), err=exc)
                result = exc
        self.applied_index = index
        waiter = self._waiting.pop(index, None)
        if waiter is not None and not waiter[1].done():
            if waiter[0] == epoch == self._serving_epoch and \
                    not isinstance(result, ZkError):
                waiter[1].set_result(result)
            else:
                waiter[1].set_exception(_NotServing())

    def _apply_txn(self, txn: dict) -> Any:
        op = txn["op"]
        zxid = txn["zxid"]
        if op == "multi":
            return [self._apply_one(sub, zxid, txn["time"])
                    for sub in txn["ops"]]
        if op == "session_open":
            self.zxid = zxid
            sess = _Session(txn["sid"], bytes.fromhex(txn["passwd"]),
                            txn["timeout"])
            self.sessions[sess.sid] = sess
            return sess
        if op == "session_close":
            self.zxid = zxid
            sess = self.sessions.pop(txn["sid"], None)
            if sess is None:
                return None
            sess.closed = True
            for path in sorted(sess.ephemerals):
                try:
                    self._do_delete(path, -1, force=True, journal=False,
                                    zxid=zxid)
                except ZkError:
                    pass
            self._forget_watches(sess.sid)
            self._closing_sids.discard(sess.sid)
            if sess.conn is not None:
                try:
                    sess.conn.close()
                except Exception:
                    pass
                sess.conn = None
            return None
        res = self._apply_one(txn, zxid, txn.get("time", 0))
        return res[1] if len(res) > 1 else None

    # ----------------------------------------- validation (leader, pre-log)
    # Requests are checked against the applied tree, under the proposal
    # lock, by ZkServer._prep_create / _prep_versioned / _prep_multi: the
    # one statement of the tree's rules, which the standalone server's
    # multi goes through as well.
    def _check_owner(self, sid: int) -> None:
        """The session a write comes from must still be alive HERE, at
        the head of the proposal queue: its close or expiry may have been
        logged while the request waited, and an ephemeral created after
        that would have no owner to be deleted with."""
        if sid not in self.sessions or sid in self._closing_sids:
            raise ZkError(ZSESSIONEXPIRED)

    # ------------------------------------------------------ client handling
    def _four_letter(self, word: bytes) -> bytes:
        if word == b"ruok":
            # "are you ok": not after a data-directory write failure
            return b"imok" if self.halt_reason is None else b"halt"
        core = self.core
        leader = core.leader_id if core is not None else None
        return ("Manatee coordination ensemble member %d\n"
                "Mode: %s\n"
                "Serving: %s\n"
                "Zxid: 0x%x\n"
                "Epoch: %d\n"
                "Leader: %s\n"
                "Sessions: %d\n"
                "Node count: %d\n"
                % (self.server_id, self.role,
                   "yes" if self.serving else "no", self.zxid, self.epoch,
                   leader if leader is not None else "none",
                   len(self.sessions), len(self.nodes))).encode()

    def _forget_watches(self, sid: int) -> None:
        for watchmap in (self.data_watches, self.child_watches):
            for path in [p for p, s in watchmap.items() if sid in s]:
                watchmap[path].discard(sid)
                if not watchmap[path]:
                    del watchmap[path]

    async def _handle_conn(self, reader: asyncio.StreamReader,
                           writer: asyncio.StreamWriter) -> None:
        sess: Optional[_Session] = None
        self._client_conns.add(writer)
        try:
            # bounded wait on a plain future — no wait_for around a read
            # whose cancellation could be lost
            first = asyncio.ensure_future(reader.readexactly(4))
            done, _ = await asyncio.wait({first}, timeout=10.0)
            if not done:
                first.cancel()
                return
            hdr = first.result()
            if hdr in FOUR_LETTER_WORDS:
                writer.write(self._four_letter(hdr))
                await writer.drain()
                return
            if not self.serving:
                return      # not the leader: the client tries the next
            epoch = self._serving_epoch
            (n,) = struct.unpack(">i", hdr)
            if n < 0 or n > 8 * 1024 * 1024:
                return
            body = await reader.readexactly(n)
            _zxid, timeout_ms, sid, passwd = jute.decode_connect_request(body)
            if not self.serving or self._serving_epoch != epoch:
                return
            if sid != 0:
                old = self.sessions.get(sid)
                if old is None or old.passwd != passwd or old.closed \
                        or sid in self._closing_sids:
                    # expired / unknown: sessionId 0 tells the client
                    writer.write(jute.encode_connect_response(
                        timeout_ms, 0, b"\x00" * 16))
                    await writer.drain()
                    return
                sess = old
            else:
                timeout_ms = max(self.min_to, min(self.max_to, timeout_ms))
                passwd = os.urandom(16).hex()

                def prep(zxid, _now, timeout_ms=timeout_ms, passwd=passwd):
                    # the txn's own zxid is unique across leaders and
                    # restarts: it is the session id
                    return {"op": "session_open", "zxid": zxid,
                            "sid": zxid, "passwd": passwd,
                            "timeout": timeout_ms}
                sess = await self._submit(prep)
                self.log.debug("session created", sid="0x%x" % sess.sid,
                               timeout_ms=timeout_ms)
            if self._serving_epoch != epoch:
                return
            if sess.conn is not None and sess.conn is not writer:
                self._forget_watches(sess.sid)
                try:
                    sess.conn.transport.abort()
                except Exception:
                    pass
            sess.conn = writer
            sess.detached_at = None
            sess.last_seen = time.monotonic()
            writer.write(jute.encode_connect_response(
                sess.timeout_ms, sess.sid, sess.passwd))
            await writer.drain()

            while True:
                hdr = await reader.readexactly(4)
                (n,) = struct.unpack(">i", hdr)
                if n < 0 or n > 8 * 1024 * 1024:
                    break
                body = await reader.readexactly(n)
                if sess.closed or sess.conn is not writer or \
                        self._serving_epoch != epoch or not self.serving:
                    break
                sess.last_seen = time.monotonic()
                r = Reader(body)
                xid, opcode = jute.decode_request_header(r)
                self.stats["requests"] += 1
                if opcode == jute.OP_CLOSE_SESSION:
                    sid = sess.sid
                    self._closing_sids.add(sid)
                    await self._submit(lambda zxid, _now: {
                        "op": "session_close", "zxid": zxid, "sid": sid})
                    writer.write(jute.encode_reply_header(
                        xid, self.zxid, ZOK).framed())
                    await writer.drain()
                    break
                if opcode in _WRITE_OPS:
                    frame = await self._dispatch_write(sess, xid, opcode, r)
                    if self._serving_epoch != epoch:
                        break       # deposed meanwhile: never ack
                else:
                    frame = self._dispatch(sess, xid, opcode, r)
                writer.write(frame)
                await writer.drain()
        except (_NotServing, asyncio.IncompleteReadError, ConnectionError,
                OSError, asyncio.CancelledError):
            pass
        except Exception as exc:  # never let one conn kill the server
            self.log.error("connection handler error", err=exc)
        finally:
            self._client_conns.discard(writer)
            if sess is not None and sess.conn is writer:
                # the session lives on until its timeout; its watches
                # belonged to this connection and go with it
                sess.conn = None
                self._forget_watches(sess.sid)
                # ... or until the disconnect grace, when it was the
                # CLIENT that closed.  A leader that was deposed or is
                # stopping aborted the connection itself, which says
                # nothing about the client.
                if not sess.closed and sess.sid not in self._closing_sids \
                        and self._running and self.serving \
                        and self._serving_epoch == epoch \
                        and self._peer_closed(reader):
                    self._mark_detached(sess)
            try:
                writer.transport.abort()
            except Exception:
                pass

    async def _dispatch_write(self, sess: _Session, xid: int, opcode: int,
                              r: Reader) -> bytes:
        try:
            if opcode == jute.OP_CREATE:
                path = r.ustring() or ""
                data = r.buffer() or b""
                jute.read_acls(r)
                flags = r.int32()

                def prep(zxid, now_ms):
                    txn = self._prep_create(path, data, flags, sess.sid)
                    txn.update(zxid=zxid, time=now_ms)
                    return txn
                created = await self._submit(prep)
                w = jute.encode_reply_header(xid, self.zxid, ZOK)
                w.ustring(created)
                return w.framed()
            if opcode == jute.OP_DELETE:
                path = r.ustring() or ""
                version = r.int32()

                def prep(zxid, _now):
                    txn = self._prep_versioned("delete", path, version)
                    txn["zxid"] = zxid
                    return txn
                await self._submit(prep)
                return jute.encode_reply_header(xid, self.zxid, ZOK).framed()
            if opcode == jute.OP_SETDATA:
                path = r.ustring() or ""
                data = r.buffer() or b""
                version = r.int32()

                def prep(zxid, now_ms):
                    txn = self._prep_versioned("setData", path, version,
                                               data)
                    txn.update(zxid=zxid, time=now_ms)
                    return txn
                stat = await self._submit(prep)
                w = jute.encode_reply_header(xid, self.zxid, ZOK)
                stat.write(w)
                return w.framed()
            if opcode == jute.OP_MULTI:
                ops = jute.read_multi_request(r)

                def prep(zxid, now_ms):
                    return {"op": "multi", "zxid": zxid, "time": now_ms,
                            "ops": self._prep_multi(ops, sess.sid)}
                try:
                    results = await self._submit(prep)
                except ZkError as exc:
                    results = [("error", exc.code)]
                w = jute.encode_reply_header(xid, self.zxid, ZOK)
                jute.write_multi_response(w, results)
                return w.framed()
            raise ZkError(jute.ZUNIMPLEMENTED)
        except ZkError as exc:
            return jute.encode_reply_header(xid, self.zxid, exc.code).framed()
        except (ValueError, struct.error):
            return jute.encode_reply_header(xid, self.zxid,
                                            ZMARSHALLINGERROR).framed()

    def _dispatch(self, sess: _Session, xid: int, opcode: int,
                  r: Reader) -> bytes:
        if opcode != jute.OP_SETWATCHES:
            return super()._dispatch(sess, xid, opcode, r)
        # ZooKeeper's SetWatches: whatever already happened after the
        # client's last seen zxid fires at once; the rest is registered
        try:
            rel = r.int64()
            lists = []
            for _ in range(3):
                n = r.int32()
                lists.append([r.ustring() or "" for _ in range(max(n, 0))])
        except (ValueError, struct.error):
            return jute.encode_reply_header(jute.XID_SET_WATCHES, self.zxid,
                                            ZMARSHALLINGERROR).framed()
        out = []

        def fire(etype, path):
            out.append(jute.encode_watcher_event(
                etype, jute.STATE_SYNC_CONNECTED, path))
            self.stats["watch_events"] += 1
        for path in lists[0]:                           # data watches
            node = self.nodes.get(path)
            if node is None:
                fire(jute.EVENT_NODE_DELETED, path)
            elif node.stat_mzxid > rel:
                fire(jute.EVENT_NODE_DATA_CHANGED, path)
            else:
                self.data_watches.setdefault(path, set()).add(sess.sid)
        for path in lists[1]:                           # exists watches
            if path in self.nodes:
                fire(jute.EVENT_NODE_CREATED, path)
            else:
                self.data_watches.setdefault(path, set()).add(sess.sid)
        for path in lists[2]:                           # child watches
            node = self.nodes.get(path)
            if node is None:
                fire(jute.EVENT_NODE_DELETED, path)
            elif node.pzxid > rel:
                fire(jute.EVENT_NODE_CHILDREN_CHANGED, path)
            else:
                self.child_watches.setdefault(path, set()).add(sess.sid)
        out.append(jute.encode_reply_header(jute.XID_SET_WATCHES, self.zxid,
                                            ZOK).framed())
        return b"".join(out)

    # ------------------------------------------------------- session expiry
    async def _sweep_sessions(self) -> None:
        period = max(0.02, self.tick_ms / 4000.0)
        while self._running:
            await asyncio.sleep(period)
            if not self.serving:
                continue
            epoch = self._serving_epoch
            now = time.monotonic()
            for sess in list(self.sessions.values()):
                if self._serving_epoch != epoch:
                    break
                if sess.closed or sess.sid in self._closing_sids:
                    continue
                if (now - sess.last_seen) * 1000.0 > sess.timeout_ms:
                    self.log.info("session expired", sid="0x%x" % sess.sid,
                                  timeout_ms=sess.timeout_ms)
                    on_disconnect = False
                elif self._grace_elapsed(sess, now):
                    self._log_disconnect_expiry(sess, now)
                    on_disconnect = True
                else:
                    continue
                self._closing_sids.add(sess.sid)
                sid = sess.sid
                try:
                    await self._submit(lambda zxid, _now, sid=sid: {
                        "op": "session_close", "zxid": zxid, "sid": sid})
                    self.stats["expired_sessions"] += 1
                    if on_disconnect:
                        self.stats["expired_on_disconnect"] += 1
                except _NotServing:
                    break
                except Exception as exc:
                    self.log.error("session expiry failed", err=exc)


def parse_peers(spec: str) -> Dict[int, Tuple[str, int]]:
    """``1=host:port,2=host:port,3=host:port``"""
    out: Dict[int, Tuple[str, int]] = {}
    for part in spec.split(","):
        part = part.strip()
        if not part:
            continue
        sid, _, addr = part.partition("=")
        host, _, port = addr.rpartition(":")
        if not sid or not host or not port:
            raise ValueError("bad peer %r (want ID=HOST:PORT)" % part)
        out[int(sid)] = (host, int(port))
    return out


async def run_member(srv: ZkQuorumServer) -> int:
    """Run one member until SIGINT/SIGTERM (returns 0) or until it halts
    because its data directory cannot be written (returns 1, so that a
    service manager restarts it)."""
    import signal
    stop = asyncio.Event()
    loop = asyncio.get_running_loop()
    for sig in (signal.SIGINT, signal.SIGTERM):
        try:
            loop.add_signal_handler(sig, stop.set)
        except (NotImplementedError, RuntimeError):
            pass
    await srv.start()
    try:
        waits = [asyncio.ensure_future(stop.wait()),
                 asyncio.ensure_future(srv.halted.wait())]
        await asyncio.wait(waits, return_when=asyncio.FIRST_COMPLETED)
        for w in waits:
            w.cancel()
        return 1 if srv.halted.is_set() else 0
    finally:
        await srv.stop()


def main(argv=None) -> int:
    import argparse

    from ..common.logging import Logger as _Logger, level_from_verbosity
    ap = argparse.ArgumentParser(
        prog="manatee-zkquorum",
        description="One member of a replicated coordination ensemble")
    ap.add_argument("--id", type=int, required=True)
    ap.add_argument("--client", required=True, metavar="HOST:PORT",
                    help="address clients connect to")
    ap.add_argument("--peers", required=True,
                    metavar="1=H:P,2=H:P,3=H:P",
                    help="quorum address of EVERY member, this one included")
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--election-timeout-ms", default="1000,2000",
                    metavar="MIN,MAX")
    ap.add_argument("--heartbeat-ms", type=int, default=100)
    ap.add_argument("--snapshot-entries", type=int, default=1000)
    ap.add_argument("--disconnect-grace-ms", type=int, default=None,
                    metavar="MS",
                    help="as leader, expire a session this long after its "
                         "client closed the connection without "
                         "re-attaching (default: off)")
    ap.add_argument("-v", "--verbose", action="count", default=0)
    ns = ap.parse_args(argv)
    log = _Logger("manatee-zkquorum", level=level_from_verbosity(ns.verbose))
    host, _, port = ns.client.rpartition(":")
    lo, _, hi = ns.election_timeout_ms.partition(",")
    srv = ZkQuorumServer(
        ns.id, client_host=host, client_port=int(port),
        peers=parse_peers(ns.peers), data_dir=ns.data_dir,
        election_timeout_ms=(int(lo), int(hi or lo)),
        heartbeat_ms=ns.heartbeat_ms,
        snapshot_entries=ns.snapshot_entries, log=log,
        disconnect_grace_ms=ns.disconnect_grace_ms)
    try:
        return asyncio.run(run_member(srv))
    except KeyboardInterrupt:
        return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
