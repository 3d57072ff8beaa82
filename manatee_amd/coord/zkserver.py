"""Embedded ZooKeeper-protocol coordination server.

The reference assumes an external ZooKeeper 3.4.x ensemble (docs/user-guide.md
"Zookeeper", lib/zookeeperMgr.js).  This image (and many deploy targets) has
no Java, so the framework ships its own coordination server speaking the same
client wire protocol (``jute.py``): sessions with timeouts, ephemeral and
sequential znodes, one-shot data/child watches, versioned setData (CAS) and
atomic multi-op transactions — the exact feature set ``zookeeperMgr.js``
consumes (ephemeral-sequential election at :452-456, one-shot watch
re-registration at :204-264, transaction with versioned setData at :605-630).

A real ZooKeeper ensemble can be substituted 1:1 — the client side
(``zkclient.py``) speaks the standard protocol and never imports this module.

The store is in-memory with an optional append-only journal for restart
durability (``journal_path``).  Coordination data is tiny (one state JSON +
election nodes + history); the journal replays in milliseconds.

This server is one process and therefore a single point of failure for
failover.  ``zkquorum.py`` runs the same tree and front-end as a
replicated three-member ensemble.
"""

from __future__ import annotations

import asyncio
import json
import os
import random
import re
import struct
import time
from typing import Dict, List, Optional, Set, Tuple

from ..common.logging import Logger, null_logger
from . import jute
from .jute import (MultiOp, Reader, Stat, Writer, ZkError, ZOK, ZNONODE,
                   ZNODEEXISTS, ZBADVERSION, ZNOTEMPTY, ZSESSIONEXPIRED,
                   ZNOCHILDRENFOREPHEMERALS, ZUNIMPLEMENTED, ZMARSHALLINGERROR,
                   ZBADARGUMENTS)


def _now_ms() -> int:
    return int(time.time() * 1000)


class _Node:
    __slots__ = ("data", "children", "stat_czxid", "stat_mzxid", "ctime",
                 "mtime", "version", "cversion", "ephemeral_owner", "next_seq",
                 "pzxid")

    def __init__(self, data: bytes, czxid: int, ephemeral_owner: int = 0,
                 now_ms: Optional[int] = None):
        self.data = data
        self.children: Set[str] = set()
        self.stat_czxid = czxid
        self.stat_mzxid = czxid
        self.ctime = _now_ms() if now_ms is None else now_ms
        self.mtime = self.ctime
        self.version = 0
        self.cversion = 0
        self.ephemeral_owner = ephemeral_owner
        self.next_seq = 0
        self.pzxid = czxid

    def stat(self) -> Stat:
        return Stat(czxid=self.stat_czxid, mzxid=self.stat_mzxid,
                    ctime=self.ctime, mtime=self.mtime, version=self.version,
                    cversion=self.cversion, aversion=0,
                    ephemeralOwner=self.ephemeral_owner,
                    dataLength=len(self.data), numChildren=len(self.children),
                    pzxid=self.pzxid)


class _Session:
    __slots__ = ("sid", "passwd", "timeout_ms", "last_seen", "ephemerals",
                 "conn", "closed", "detached_at")

    def __init__(self, sid: int, passwd: bytes, timeout_ms: int):
        self.sid = sid
        self.passwd = passwd
        self.timeout_ms = timeout_ms
        self.last_seen = time.monotonic()
        self.ephemerals: Set[str] = set()
        self.conn: Optional[asyncio.StreamWriter] = None
        self.closed = False
        # monotonic time at which the CLIENT's side closed the session's
        # connection; None while attached, after silence without a close,
        # or when this server dropped the connection itself
        self.detached_at: Optional[float] = None


_TRAILING_SEQ = re.compile(r"(\d{10})$")


def _parent(path: str) -> str:
    i = path.rfind("/")
    return path[:i] if i > 0 else "/"


def _validate_path(path: str) -> str:
    if not path.startswith("/") or (len(path) > 1 and path.endswith("/")):
        raise ZkError(jute.ZAPIERROR, path)
    return path


def _child_name(parent_path: str, path: str) -> str:
    return path[len(parent_path):].lstrip("/")


class _Shadow:
    """One znode as the later ops of a transaction see it: only what
    validation reads."""

    __slots__ = ("ephemeral", "version", "next_seq", "children")

    def __init__(self, ephemeral: bool, version: int = 0, next_seq: int = 0,
                 children: Optional[Set[str]] = None):
        self.ephemeral = ephemeral
        self.version = version
        self.next_seq = next_seq
        self.children: Set[str] = children if children is not None else set()


class _MultiView:
    """The tree as one transaction sees it while it is validated: the
    applied tree, overlaid with what the transaction's earlier ops have
    done.  A path is copied into the overlay when it is first looked at;
    ``None`` there means deleted (or never there)."""

    __slots__ = ("_nodes", "_seen")

    def __init__(self, nodes: Dict[str, _Node]):
        self._nodes = nodes
        self._seen: Dict[str, Optional[_Shadow]] = {}

    def get(self, path: str) -> Optional[_Shadow]:
        if path not in self._seen:
            n = self._nodes.get(path)
            self._seen[path] = None if n is None else _Shadow(
                bool(n.ephemeral_owner), n.version, n.next_seq,
                set(n.children))
        return self._seen[path]

    def put(self, path: str, shadow: Optional[_Shadow]) -> None:
        self._seen[path] = shadow


class ZkServer:
    """One standalone coordination server (the test/dev substitute for a
    3-node ZK ensemble)."""

    def __init__(self, host: str = "127.0.0.1", port: int = 0,
                 log: Optional[Logger] = None,
                 tick_ms: int = 200,
                 min_session_timeout_ms: int = 1000,
                 max_session_timeout_ms: int = 120000,
                 journal_path: Optional[str] = None,
                 disconnect_grace_ms: Optional[int] = None):
        self.host = host
        self.port = port
        self.log = (log or null_logger()).child(component="ZkServer")
        self.tick_ms = tick_ms
        self.min_to = min_session_timeout_ms
        self.max_to = max_session_timeout_ms
        self.journal_path = journal_path
        # opt-in: a session whose client closed its connection (FIN/RST)
        # and did not re-attach within this long is expired then, not at
        # its timeout.  None or <= 0 is off; silence never counts.
        self.disconnect_grace_ms = disconnect_grace_ms \
            if disconnect_grace_ms and disconnect_grace_ms > 0 else None
        self._stopping = False
        self._journal = None
        self._journal_entries = 0
        self.journal_compact_entries = 5000

        self.nodes: Dict[str, _Node] = {"/": _Node(b"", 0)}
        self.sessions: Dict[int, _Session] = {}
        self.zxid = 0
        self._next_sid = (random.getrandbits(24) << 24) | 1
        self.data_watches: Dict[str, Set[int]] = {}
        self.child_watches: Dict[str, Set[int]] = {}
        self._server: Optional[asyncio.AbstractServer] = None
        self._sweeper: Optional[asyncio.Task] = None
        self.stats = {"requests": 0, "watch_events": 0, "expired_sessions": 0,
                      "expired_on_disconnect": 0}

    # ------------------------------------------------------------ lifecycle
    async def start(self) -> None:
        if self.journal_path and os.path.exists(self.journal_path):
            self._replay_journal()
        if self.journal_path:
            self._journal = open(self.journal_path, "a", buffering=1)
        self._server = await asyncio.start_server(
            self._handle_conn, self.host, self.port)
        self.port = self._server.sockets[0].getsockname()[1]
        self._sweeper = asyncio.get_running_loop().create_task(
            self._sweep_sessions())
        self.log.info("zk server listening", host=self.host, port=self.port)

    async def stop(self) -> None:
        self._stopping = True
        if self._sweeper:
            self._sweeper.cancel()
            try:
                await self._sweeper
            except asyncio.CancelledError:
                pass
        if self._server:
            self._server.close()
            await self._server.wait_closed()
        for sess in list(self.sessions.values()):
            if sess.conn is not None:
                try:
                    sess.conn.close()
                except Exception:
                    pass
        if self._journal:
            self._journal.close()
            self._journal = None

    @property
    def conn_str(self) -> str:
        return "%s:%d" % (self.host, self.port)

    # ------------------------------------------------------------- journal
    def _journal_write(self, op: dict) -> None:
        if self._journal is not None:
            self._journal.write(json.dumps(op, separators=(",", ":")) + "\n")
            self._journal_entries += 1
            if self._journal_entries >= self.journal_compact_entries and \
                    self._journal_entries >= 2 * max(1, len(self.nodes)):
                try:
                    self._compact_journal()
                except OSError as exc:
                    self.log.error("journal compaction failed", err=exc)

    def _replay_journal(self) -> None:
        n = 0
        with open(self.journal_path, "r") as f:
            for line in f:
                line = line.strip()
                if not line:
                    continue
                try:
                    op = json.loads(line)
                except ValueError:
                    # torn tail from a dirty kill mid-append; nothing
                    # after it can be valid either
                    self.log.warn("journal line unparseable; stopping "
                                  "replay", entries=n)
                    break
                try:
                    if op["op"] == "create":
                        # journaled paths are FINAL (already sequenced):
                        # always replay as plain persistent creates, then
                        # restore the parent's sequence counter so new
                        # sequential nodes continue after the replayed ones
                        self._do_create(op["path"],
                                        bytes.fromhex(op["data"]),
                                        jute.PERSISTENT, 0,
                                        journal=False)
                        m = _TRAILING_SEQ.search(op["path"])
                        if m:
                            parent = self.nodes.get(_parent(op["path"]))
                            if parent is not None:
                                parent.next_seq = max(
                                    parent.next_seq, int(m.group(1)) + 1)
                    elif op["op"] == "setData":
                        self._do_set_data(op["path"],
                                          bytes.fromhex(op["data"]), -1,
                                          journal=False)
                    elif op["op"] == "delete":
                        self._do_delete(op["path"], -1, journal=False)
                except ZkError:
                    pass
                n += 1
        self._journal_entries = n
        self.log.info("journal replayed", entries=n)

    def _compact_journal(self) -> None:
        """Rewrite the journal as a snapshot of the current persistent
        tree (one create per node) — bounds the append-only journal,
        which otherwise grows with every cluster-state write forever."""
        tmp = self.journal_path + ".tmp"
        count = 0
        with open(tmp, "w") as f:
            for path in sorted(self.nodes):
                node = self.nodes[path]
                if path == "/" or node.ephemeral_owner:
                    continue
                f.write(json.dumps(
                    {"op": "create", "path": path,
                     "data": node.data.hex(), "flags": jute.PERSISTENT},
                    separators=(",", ":")) + "\n")
                count += 1
            f.flush()
            os.fsync(f.fileno())
        if self._journal is not None:
            self._journal.close()
        os.replace(tmp, self.journal_path)
        self._journal = open(self.journal_path, "a", buffering=1)
        self._journal_entries = count
        self.log.info("journal compacted", nodes=count)

    # ------------------------------------------------------- session sweeper
    async def _sweep_sessions(self) -> None:
        # sweep at tick/4 (min 20 ms): expiry granularity is pure added
        # failover-detection latency and the scan is O(sessions), tiny
        while True:
            await asyncio.sleep(max(0.02, self.tick_ms / 4000.0))
            now = time.monotonic()
            for sess in list(self.sessions.values()):
                if sess.closed:
                    continue
                if (now - sess.last_seen) * 1000.0 > sess.timeout_ms:
                    self.log.info("session expired", sid="0x%x" % sess.sid,
                                  timeout_ms=sess.timeout_ms)
                    self.stats["expired_sessions"] += 1
                    self._expire_session(sess)
                elif self._grace_elapsed(sess, now):
                    self._log_disconnect_expiry(sess, now)
                    self.stats["expired_on_disconnect"] += 1
                    self.stats["expired_sessions"] += 1
                    self._expire_session(sess)

    def _grace_elapsed(self, sess: _Session, now: float) -> bool:
        return self.disconnect_grace_ms is not None and \
            sess.detached_at is not None and \
            (now - sess.detached_at) * 1000.0 > self.disconnect_grace_ms

    def _log_disconnect_expiry(self, sess: _Session, now: float) -> None:
        self.log.info("session expired after disconnect",
                      sid="0x%x" % sess.sid,
                      grace_ms=self.disconnect_grace_ms,
                      detached_ms=int((now - sess.detached_at) * 1000.0),
                      timeout_ms=sess.timeout_ms)

    def _expire_session(self, sess: _Session) -> None:
        sess.closed = True
        self.sessions.pop(sess.sid, None)
        for path in sorted(sess.ephemerals):
            try:
                self._do_delete(path, -1, force=True)
            except ZkError:
                pass
        for watchset in list(self.data_watches.values()):
            watchset.discard(sess.sid)
        for watchset in list(self.child_watches.values()):
            watchset.discard(sess.sid)
        if sess.conn is not None:
            try:
                sess.conn.close()
            except Exception:
                pass
            sess.conn = None

    # --------------------------------------------------------- watch firing
    def _fire_data_watch(self, path: str, etype: int) -> None:
        sids = self.data_watches.pop(path, None)
        if sids:
            self._deliver(sids, etype, path)

    def _fire_child_watch(self, path: str, etype: int = jute.EVENT_NODE_CHILDREN_CHANGED) -> None:
        sids = self.child_watches.pop(path, None)
        if sids:
            self._deliver(sids, etype, path)

    def _deliver(self, sids: Set[int], etype: int, path: str) -> None:
        frame = jute.encode_watcher_event(etype, jute.STATE_SYNC_CONNECTED,
                                          path)
        for sid in sids:
            sess = self.sessions.get(sid)
            if sess is not None and sess.conn is not None:
                try:
                    sess.conn.write(frame)
                    self.stats["watch_events"] += 1
                except Exception:
                    pass

    # ------------------------------------------------------------- core ops
    # zxid / now_ms: the standalone server draws both locally (None).  The
    # quorum server (zkquorum.py) passes the values its replicated txn
    # carries, so every replica builds byte-identical Stats.
    def _do_create(self, path: str, data: bytes, flags: int, owner_sid: int,
                   journal: bool = True, zxid: Optional[int] = None,
                   now_ms: Optional[int] = None) -> str:
        _validate_path(path)
        parent_path = _parent(path)
        parent = self.nodes.get(parent_path)
        if parent is None:
            raise ZkError(ZNONODE, parent_path)
        if parent.ephemeral_owner:
            raise ZkError(ZNOCHILDRENFOREPHEMERALS, parent_path)
        sequential = flags in (jute.PERSISTENT_SEQUENTIAL,
                               jute.EPHEMERAL_SEQUENTIAL)
        if sequential:
            path = "%s%010d" % (path, parent.next_seq)
        if path in self.nodes:
            raise ZkError(ZNODEEXISTS, path)
        if sequential:
            # only a create that succeeds consumes a sequence number
            parent.next_seq += 1
        self.zxid = self.zxid + 1 if zxid is None else zxid
        ephemeral = flags in (jute.EPHEMERAL, jute.EPHEMERAL_SEQUENTIAL)
        node = _Node(data, self.zxid,
                     ephemeral_owner=owner_sid if ephemeral else 0,
                     now_ms=now_ms)
        self.nodes[path] = node
        parent.children.add(_child_name(parent_path, path))
        parent.cversion += 1
        parent.pzxid = self.zxid
        if ephemeral and owner_sid in self.sessions:
            self.sessions[owner_sid].ephemerals.add(path)
        if journal and not ephemeral:
            self._journal_write({"op": "create", "path": path,
                                 "data": data.hex(), "flags": flags})
        self._fire_data_watch(path, jute.EVENT_NODE_CREATED)
        self._fire_child_watch(parent_path)
        return path

    def _do_delete(self, path: str, version: int, force: bool = False,
                   journal: bool = True, zxid: Optional[int] = None) -> None:
        if path == "/":
            # the root is not a znode anybody made; without it every
            # later create would answer ZNONODE
            raise ZkError(ZBADARGUMENTS, path)
        node = self.nodes.get(path)
        if node is None:
            raise ZkError(ZNONODE, path)
        if node.children:
            raise ZkError(ZNOTEMPTY, path)
        if version != -1 and version != node.version and not force:
            raise ZkError(ZBADVERSION, path)
        self.zxid = self.zxid + 1 if zxid is None else zxid
        del self.nodes[path]
        parent_path = _parent(path)
        parent = self.nodes.get(parent_path)
        if parent is not None:
            parent.children.discard(_child_name(parent_path, path))
            parent.cversion += 1
            parent.pzxid = self.zxid
        if node.ephemeral_owner and node.ephemeral_owner in self.sessions:
            self.sessions[node.ephemeral_owner].ephemerals.discard(path)
        if journal and not node.ephemeral_owner:
            self._journal_write({"op": "delete", "path": path})
        self._fire_data_watch(path, jute.EVENT_NODE_DELETED)
        self._fire_child_watch(path, jute.EVENT_NODE_DELETED)
        self._fire_child_watch(parent_path)

    def _do_set_data(self, path: str, data: bytes, version: int,
                     journal: bool = True, zxid: Optional[int] = None,
                     now_ms: Optional[int] = None) -> Stat:
        node = self.nodes.get(path)
        if node is None:
            raise ZkError(ZNONODE, path)
        if version != -1 and version != node.version:
            raise ZkError(ZBADVERSION, path)
        self.zxid = self.zxid + 1 if zxid is None else zxid
        node.data = data
        node.version += 1
        node.mtime = _now_ms() if now_ms is None else now_ms
        node.stat_mzxid = self.zxid
        if journal and not node.ephemeral_owner:
            self._journal_write({"op": "setData", "path": path,
                                 "data": data.hex()})
        self._fire_data_watch(path, jute.EVENT_NODE_DATA_CHANGED)
        return node.stat()

    def _do_multi(self, ops: List[MultiOp], owner_sid: int) -> List[tuple]:
        # validate the whole transaction first, every op seeing the
        # effects of the earlier ones; a failure raises from here with
        # nothing applied, journaled, fired or numbered
        # (ref zookeeperMgr.js:605-630 relies on this for putClusterState CAS)
        txns = self._prep_multi(ops, owner_sid)
        return [self._apply_one(txn, None, None, journal=True)
                for txn in txns]

    # ------------------------------------------------ validation and apply
    # A write is validated into its OUTCOME (a create with its final,
    # already-sequenced path), then applied.  The standalone server does
    # this for a multi; the quorum server (zkquorum.py) for every write,
    # with the log between the two halves.  Inside a multi the ops see
    # each other's effects, in order, through a _MultiView.
    def _check_owner(self, sid: int) -> None:
        """An ephemeral needs a live session to be deleted with."""
        if sid not in self.sessions:
            raise ZkError(ZSESSIONEXPIRED)

    def _prep_create(self, path: str, data: bytes, flags: int, sid: int,
                     view: Optional[_MultiView] = None) -> dict:
        view = view or _MultiView(self.nodes)
        _validate_path(path)
        pp = _parent(path)
        parent = view.get(pp)
        if parent is None:
            raise ZkError(ZNONODE, pp)
        if parent.ephemeral:
            raise ZkError(ZNOCHILDRENFOREPHEMERALS, pp)
        seq = None
        if flags in (jute.PERSISTENT_SEQUENTIAL, jute.EPHEMERAL_SEQUENTIAL):
            seq = parent.next_seq
            path = "%s%010d" % (path, seq)
        if view.get(path) is not None:
            raise ZkError(ZNODEEXISTS, path)
        ephemeral = flags in (jute.EPHEMERAL, jute.EPHEMERAL_SEQUENTIAL)
        if ephemeral:
            self._check_owner(sid)
        if seq is not None:
            parent.next_seq = seq + 1
        parent.children.add(_child_name(pp, path))
        view.put(path, _Shadow(ephemeral))
        return {"op": "create", "path": path, "data": data.hex(),
                "owner": sid if ephemeral else 0, "seq": seq}

    def _prep_versioned(self, op: str, path: str, version: int,
                        data: bytes = b"",
                        view: Optional[_MultiView] = None) -> dict:
        view = view or _MultiView(self.nodes)
        if op == "delete" and path == "/":
            raise ZkError(ZBADARGUMENTS, path)
        node = view.get(path)
        if node is None:
            raise ZkError(ZNONODE, path)
        if op == "delete" and node.children:
            raise ZkError(ZNOTEMPTY, path)
        if version != -1 and version != node.version:
            raise ZkError(ZBADVERSION, path)
        if op == "setData":
            node.version += 1
            return {"op": op, "path": path, "data": data.hex()}
        if op == "delete":
            view.put(path, None)
            pp = _parent(path)
            parent = view.get(pp)
            if parent is not None:
                parent.children.discard(_child_name(pp, path))
        return {"op": op, "path": path}

    def _prep_multi(self, ops: List[MultiOp], sid: int) -> List[dict]:
        view = _MultiView(self.nodes)
        out = []
        for op in ops:
            if op.kind == "create":
                out.append(self._prep_create(op.path, op.data or b"",
                                             op.flags, sid, view))
            else:
                out.append(self._prep_versioned(op.kind, op.path,
                                                op.version, op.data or b"",
                                                view))
        return out

    def _apply_one(self, txn: dict, zxid: Optional[int],
                   now_ms: Optional[int], journal: bool = False) -> tuple:
        """Apply one validated outcome; cannot fail for a txn that
        ``_prep_*`` produced against this tree."""
        op = txn["op"]
        if op == "create":
            owner = txn["owner"]
            path = self._do_create(
                txn["path"], bytes.fromhex(txn["data"]),
                jute.EPHEMERAL if owner else jute.PERSISTENT, owner,
                journal=journal, zxid=zxid, now_ms=now_ms)
            if txn.get("seq") is not None:
                self.nodes[_parent(path)].next_seq = txn["seq"] + 1
            return ("create", path)
        if op == "setData":
            return ("setData", self._do_set_data(
                txn["path"], bytes.fromhex(txn["data"]), -1, journal=journal,
                zxid=zxid, now_ms=now_ms))
        if op == "delete":
            self._do_delete(txn["path"], -1, force=True, journal=journal,
                            zxid=zxid)
            return ("delete",)
        return ("check",)

    # -------------------------------------------------------- conn handling
    async def _read_frame(self, reader: asyncio.StreamReader) -> Optional[bytes]:
        try:
            hdr = await reader.readexactly(4)
        except (asyncio.IncompleteReadError, ConnectionError, OSError):
            return None
        (n,) = struct.unpack(">i", hdr)
        if n < 0 or n > 8 * 1024 * 1024:
            return None
        try:
            return await reader.readexactly(n)
        except (asyncio.IncompleteReadError, ConnectionError, OSError):
            return None

    @staticmethod
    def _peer_closed(reader: asyncio.StreamReader) -> bool:
        """The stream ended (FIN) or failed (RST, or an error the kernel
        reported) — as opposed to a handler that stopped reading on its
        own.  A transport this server closed itself ends the stream too;
        callers rule that out by ``sess.conn is writer`` and their own
        stopping/serving state."""
        return reader.at_eof() or reader.exception() is not None

    def _mark_detached(self, sess: _Session) -> None:
        if self.disconnect_grace_ms is not None:
            sess.detached_at = time.monotonic()

    async def _handle_conn(self, reader: asyncio.StreamReader,
                           writer: asyncio.StreamWriter) -> None:
        sess: Optional[_Session] = None
        try:
            body = await self._read_frame(reader)
            if body is None:
                return
            _zxid, timeout_ms, sid, passwd = jute.decode_connect_request(body)
            if sid != 0:
                old = self.sessions.get(sid)
                if old is not None and old.passwd == passwd and not old.closed:
                    sess = old
                    if sess.conn is not None and sess.conn is not writer:
                        try:
                            sess.conn.close()
                        except Exception:
                            pass
                    sess.conn = writer
                    sess.detached_at = None
                    sess.last_seen = time.monotonic()
                    writer.write(jute.encode_connect_response(
                        sess.timeout_ms, sess.sid, sess.passwd))
                else:
                    # expired / unknown session: sessionId 0 tells the client
                    writer.write(jute.encode_connect_response(
                        timeout_ms, 0, b"\x00" * 16))
                    await writer.drain()
                    return
            else:
                timeout_ms = max(self.min_to, min(self.max_to, timeout_ms))
                sid = self._next_sid
                self._next_sid += 1
                sess = _Session(sid, os.urandom(16), timeout_ms)
                sess.conn = writer
                self.sessions[sid] = sess
                self.log.debug("session created", sid="0x%x" % sid,
                               timeout_ms=timeout_ms)
                writer.write(jute.encode_connect_response(
                    timeout_ms, sid, sess.passwd))
            await writer.drain()

            while True:
                body = await self._read_frame(reader)
                if body is None:
                    break
                if sess.closed:
                    break
                sess.last_seen = time.monotonic()
                r = Reader(body)
                xid, opcode = jute.decode_request_header(r)
                self.stats["requests"] += 1
                if opcode == jute.OP_CLOSE_SESSION:
                    w = jute.encode_reply_header(xid, self.zxid, ZOK)
                    writer.write(w.framed())
                    await writer.drain()
                    sess.closed = True
                    self.sessions.pop(sess.sid, None)
                    for path in sorted(sess.ephemerals):
                        try:
                            self._do_delete(path, -1, force=True)
                        except ZkError:
                            pass
                    for ws in list(self.data_watches.values()):
                        ws.discard(sess.sid)
                    for ws in list(self.child_watches.values()):
                        ws.discard(sess.sid)
                    break
                frame = self._dispatch(sess, xid, opcode, r)
                writer.write(frame)
                await writer.drain()
        except (ConnectionError, asyncio.CancelledError):
            pass
        except Exception as exc:  # never let one conn kill the server
            self.log.error("connection handler error", err=exc)
        finally:
            if sess is not None and sess.conn is writer:
                # the session stays until its timeout (disconnect !=
                # expiry) — unless the CLIENT closed and the disconnect
                # grace is on: then the sweeper gives it that long to
                # re-attach.  A close or abort of our own proves nothing.
                sess.conn = None
                if not sess.closed and not self._stopping and \
                        self._peer_closed(reader):
                    self._mark_detached(sess)
            try:
                writer.close()
            except Exception:
                pass

    def _dispatch(self, sess: _Session, xid: int, opcode: int,
                  r: Reader) -> bytes:
        try:
            if opcode == jute.OP_PING:
                return jute.encode_reply_header(jute.XID_PING, self.zxid,
                                                ZOK).framed()
            if opcode == jute.OP_CREATE:
                path = r.ustring() or ""
                data = r.buffer() or b""
                jute.read_acls(r)
                flags = r.int32()
                created = self._do_create(path, data, flags, sess.sid)
                w = jute.encode_reply_header(xid, self.zxid, ZOK)
                w.ustring(created)
                return w.framed()
            if opcode == jute.OP_DELETE:
                path = r.ustring() or ""
                version = r.int32()
                self._do_delete(path, version)
                return jute.encode_reply_header(xid, self.zxid, ZOK).framed()
            if opcode == jute.OP_EXISTS:
                path = r.ustring() or ""
                watch = r.boolean()
                node = self.nodes.get(path)
                if watch:
                    # exists watches register even on missing nodes
                    self.data_watches.setdefault(path, set()).add(sess.sid)
                if node is None:
                    raise ZkError(ZNONODE, path)
                w = jute.encode_reply_header(xid, self.zxid, ZOK)
                node.stat().write(w)
                return w.framed()
            if opcode == jute.OP_GETDATA:
                path = r.ustring() or ""
                watch = r.boolean()
                node = self.nodes.get(path)
                if node is None:
                    # a getData watch on a missing node is NOT registered
                    raise ZkError(ZNONODE, path)
                if watch:
                    self.data_watches.setdefault(path, set()).add(sess.sid)
                w = jute.encode_reply_header(xid, self.zxid, ZOK)
                w.buffer(node.data)
                node.stat().write(w)
                return w.framed()
            if opcode == jute.OP_SETDATA:
                path = r.ustring() or ""
                data = r.buffer() or b""
                version = r.int32()
                stat = self._do_set_data(path, data, version)
                w = jute.encode_reply_header(xid, self.zxid, ZOK)
                stat.write(w)
                return w.framed()
            if opcode in (jute.OP_GETCHILDREN, jute.OP_GETCHILDREN2):
                path = r.ustring() or ""
                watch = r.boolean()
                node = self.nodes.get(path)
                if node is None:
                    raise ZkError(ZNONODE, path)
                if watch:
                    self.child_watches.setdefault(path, set()).add(sess.sid)
                w = jute.encode_reply_header(xid, self.zxid, ZOK)
                children = sorted(node.children)
                w.int32(len(children))
                for c in children:
                    w.ustring(c)
                if opcode == jute.OP_GETCHILDREN2:
                    node.stat().write(w)
                return w.framed()
            if opcode == jute.OP_MULTI:
                ops = jute.read_multi_request(r)
                try:
                    results = self._do_multi(ops, sess.sid)
                except ZkError as exc:
                    w = jute.encode_reply_header(xid, self.zxid, ZOK)
                    jute.write_multi_response(w, [("error", exc.code)])
                    return w.framed()
                w = jute.encode_reply_header(xid, self.zxid, ZOK)
                jute.write_multi_response(w, results)
                return w.framed()
            if opcode == jute.OP_SYNC:
                path = r.ustring() or ""
                w = jute.encode_reply_header(xid, self.zxid, ZOK)
                w.ustring(path)
                return w.framed()
            if opcode == jute.OP_AUTH:
                return jute.encode_reply_header(jute.XID_AUTH, self.zxid,
                                                ZOK).framed()
            if opcode == jute.OP_SETWATCHES:
                # relativeZxid, then 3 vectors of paths
                r.int64()
                for watchmap in (self.data_watches, self.data_watches,
                                 self.child_watches):
                    n = r.int32()
                    for _ in range(max(n, 0)):
                        p = r.ustring() or ""
                        watchmap.setdefault(p, set()).add(sess.sid)
                return jute.encode_reply_header(jute.XID_SET_WATCHES,
                                                self.zxid, ZOK).framed()
            raise ZkError(ZUNIMPLEMENTED)
        except ZkError as exc:
            return jute.encode_reply_header(xid, self.zxid, exc.code).framed()
        except (ValueError, struct.error):
            return jute.encode_reply_header(xid, self.zxid,
                                            ZMARSHALLINGERROR).framed()

    # ------------------------------------------------------------ test aid
    def dump_tree(self) -> Dict[str, dict]:
        out = {}
        for path, node in sorted(self.nodes.items()):
            out[path] = {"data": node.data.decode("utf-8", "replace"),
                         "version": node.version,
                         "ephemeralOwner": node.ephemeral_owner,
                         "children": sorted(node.children)}
        return out


async def run_standalone(host: str, port: int, log: Logger,
                         journal_path: Optional[str] = None,
                         disconnect_grace_ms: Optional[int] = None) -> None:
    srv = ZkServer(host=host, port=port, log=log, journal_path=journal_path,
                   disconnect_grace_ms=disconnect_grace_ms)
    await srv.start()
    try:
        while True:
            await asyncio.sleep(3600)
    finally:
        await srv.stop()


def main(argv=None) -> int:
    import argparse

    from ..common.logging import Logger as _Logger, level_from_verbosity
    ap = argparse.ArgumentParser(prog="manatee-zk")
    ap.add_argument("-H", "--host", default="127.0.0.1")
    ap.add_argument("-p", "--port", type=int, default=2181)
    ap.add_argument("-j", "--journal", default=None)
    ap.add_argument("-g", "--disconnect-grace-ms", type=int, default=None,
                    metavar="MS",
                    help="expire a session this long after its client "
                         "closed the connection without re-attaching "
                         "(default: off, the session timeout alone decides)")
    ap.add_argument("-v", "--verbose", action="count", default=0)
    ns = ap.parse_args(argv)
    log = _Logger("manatee-zk", level=level_from_verbosity(ns.verbose))
    try:
        asyncio.run(run_standalone(
            ns.host, ns.port, log, journal_path=ns.journal,
            disconnect_grace_ms=ns.disconnect_grace_ms))
    except KeyboardInterrupt:
        pass
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
