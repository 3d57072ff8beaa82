"""minipg server — PostgreSQL process conventions + libpq v3 frontend
over the waldb replication core.

See package docstring for the fidelity contract.  The process is
managed by db/postgres.py + db/manager.py exactly as the reference
manages a real ``postgres`` child (ref lib/postgresMgr.js:1653-1795):
spawned as ``postgres -D dataDir``, killed dirty, reloaded with SIGHUP,
promoted via trigger file, configured only through regenerated conf
files.

Peer replication is multiplexed on the listen port by first byte:
``{`` starts a waldb JSON/replication exchange (PostgreSQL likewise
multiplexes walsender connections on its port), anything else is
parsed as a libpq startup packet.
"""

from __future__ import annotations

import argparse
import asyncio
import dataclasses
import datetime
import os
import re
import struct
import sys
from typing import Dict, List, Optional, Tuple

from ...common import confparser
from ...common import lsn as lsnmod
from ...common.logging import Logger, level_from_verbosity
from ...common.lsn import pg_strip_minor
from ..waldb.core import (Settings, conf_value, init_data_dir as waldb_init,
                          parse_knobs, run_server)
from ..waldb.server import WaldbServer
from ..waldb.wal import encode_op

_I32 = struct.Struct(">i")
_I16 = struct.Struct(">h")

SSL_REQUEST = 80877103
CANCEL_REQUEST = 80877102
GSSENC_REQUEST = 80877104
PROTOCOL_V3 = 196608

# largest libpq message accepted; also the cap on one transaction
# block's buffered (encoded) writes
MAX_MSG = 16 * 1024 * 1024

CONF_NAME = "postgresql.conf"
RECOVERY_NAME = "recovery.conf"
SIGNAL_NAME = "standby.signal"


def parse_conninfo(text: str) -> Dict[str, str]:
    """'host=H port=P user=U application_name=A ...' → dict."""
    out: Dict[str, str] = {}
    for part in text.strip().strip("'\"").split():
        k, _, v = part.partition("=")
        if k:
            out[k] = v
    return out


def sql_unquote(text: str) -> str:
    return text.replace("''", "'")


def split_statements(sql: str) -> List[str]:
    """Split a simple-Query string on ';' outside single quotes (the
    multi-statement form of the simple protocol)."""
    out, cur, inq = [], [], False
    for ch in sql:
        if ch == "'":
            inq = not inq
            cur.append(ch)
        elif ch == ";" and not inq:
            out.append("".join(cur))
            cur = []
        else:
            cur.append(ch)
    out.append("".join(cur))
    return [s.strip() for s in out if s.strip()]


# a whole single-quoted literal ('' is an escaped quote)
_RE_LITERAL = re.compile(r"'(?:[^']|'')*'")
# a literal (an unterminated one runs to the end) or a $n placeholder
_RE_PARAM = re.compile(r"'(?:[^']|'')*(?:'|$)|\$(\d+)")


def count_params(sql: str) -> int:
    """The highest ``$n`` outside single-quoted literals."""
    top = 0
    for m in _RE_PARAM.finditer(sql):
        if m.group(1) is not None:
            n = int(m.group(1))
            if n < 1:
                raise PgSqlError("42P02", "there is no parameter $0")
            top = max(top, n)
    return top


def bind_params(sql: str, params: List[Optional[str]]) -> str:
    """Lexical parameter substitution: every ``$n`` outside a literal
    becomes a quoted literal with ``'`` doubled (``NULL`` for None).  One
    pass, so a ``$1`` inside a substituted VALUE is never looked at
    again, and a value cannot close its own literal."""
    def rep(m):
        if m.group(1) is None:
            return m.group(0)
        v = params[int(m.group(1)) - 1]
        return "NULL" if v is None else "'" + v.replace("'", "''") + "'"
    return _RE_PARAM.sub(rep, sql)


def _cstr(buf: bytes, pos: int) -> Tuple[str, int]:
    end = buf.index(b"\x00", pos)
    return buf[pos:end].decode("utf-8"), end + 1


class PgSqlError(Exception):
    def __init__(self, code: str, msg: str):
        self.code = code
        self.msg = msg
        super().__init__(msg)


_TOMBSTONE = object()       # a key deleted inside the open block


class _Portal:
    __slots__ = ("stmt", "kind", "cols", "arg", "rows", "pos")

    def __init__(self, stmt: str, kind: str, cols, arg):
        self.stmt = stmt            # name of the statement it was bound to
        self.kind = kind
        self.cols = cols
        self.arg = arg
        self.rows: Optional[List[list]] = None      # None until executed
        self.pos = 0


class _Session:
    """Per-connection state: the transaction block with its buffered
    writes, and the extended-query protocol's statements, portals and
    staged output.  It dies with the connection, so a client that drops
    mid-block leaves no trace."""

    __slots__ = ("txn", "ops", "ops_bytes", "pending", "stmts", "portals",
                 "staged", "max_lsn", "skip")

    def __init__(self):
        self.txn = "I"              # ReadyForQuery status: I, T or E
        self.ops: List[dict] = []
        self.ops_bytes = 0
        self.pending: Dict[str, object] = {}
        self.stmts: Dict[str, Tuple[str, int, Optional[List[str]]]] = {}
        self.portals: Dict[str, _Portal] = {}
        self.staged: List[bytes] = []
        self.max_lsn: Optional[int] = None
        self.skip = False           # discarding until the next Sync

    def end_txn(self) -> None:
        self.txn = "I"
        self.ops = []
        self.ops_bytes = 0
        self.pending = {}
        self.portals.clear()

    def fail(self) -> None:
        """An error inside a block fails the block."""
        if self.txn == "T":
            self.txn = "E"


class MinipgServer(WaldbServer):
    PID_FILE = "postmaster.pid"
    CONF_FILE = CONF_NAME

    def __init__(self, data_dir: str, log: Logger):
        super().__init__(data_dir, log)
        self.log = log.child(component="minipg")
        try:
            with open(os.path.join(self.data_dir, "PG_VERSION")) as f:
                self.pg_major = f.read().strip() or "12"
        except OSError:
            self.pg_major = "12"
        self.lsn_word = "lsn" if float(self.pg_major) >= 10 else "location"

    # -------------------------------------------------- postgres conf model
    def read_settings(self, prev: Settings) -> Settings:
        raw = confparser.read(os.path.join(self.data_dir, CONF_NAME))
        s = conf_value
        standby, conninfo_s, trigger = False, None, None
        rec_path = os.path.join(self.data_dir, RECOVERY_NAME)
        if os.path.exists(os.path.join(self.data_dir, SIGNAL_NAME)):
            # PG ≥12 style: standby.signal + settings in postgresql.conf
            standby = True
            conninfo_s = s(raw.get("primary_conninfo", ""))
            trigger = s(raw.get("promote_trigger_file", ""))
        elif os.path.exists(rec_path):
            # pre-12 style: recovery.conf with standby_mode=on
            rec = confparser.read(rec_path)
            if s(rec.get("standby_mode", "")) == "on":
                standby = True
                conninfo_s = s(rec.get("primary_conninfo", ""))
                trigger = s(rec.get("trigger_file", ""))
        ci = parse_conninfo(conninfo_s) if conninfo_s else {}

        listen = s(raw.get("listen_addresses", "127.0.0.1"))
        if listen in ("*", ""):
            listen = "0.0.0.0"
        upstream = None
        if standby and ci.get("host"):
            upstream = "%s:%s" % (ci["host"], ci.get("port", "5432"))
        # absent knobs keep their value; PG writes wal_sender_timeout in ms
        return parse_knobs(raw, dataclasses.replace(
            prev,
            role="standby" if standby else "primary",
            listen_ip=listen,
            port=s(raw.get("port", "5432")),
            name=ci.get("application_name", "standby"),
            read_only=s(raw.get("default_transaction_read_only",
                                "off")) == "on",
            sync_standby=s(raw.get("synchronous_standby_names", "")) or None,
            upstream=upstream,
            trigger_path=trigger or os.path.join(
                os.path.dirname(self.data_dir), "promote")), 0.001)

    # ------------------------------------------------- connection multiplex
    async def _handle_conn(self, reader: asyncio.StreamReader,
                           writer: asyncio.StreamWriter) -> None:
        try:
            first = await reader.readexactly(1)
        except (asyncio.IncompleteReadError, ConnectionError):
            writer.close()
            return
        if first == b"{":
            # waldb JSON exchange (peer replication / internal probes)
            return await self._serve_json(reader, writer, first)
        await self._serve_libpq(first, reader, writer)

    # ----------------------------------------------------- libpq v3 backend
    @staticmethod
    def _msg(t: bytes, payload: bytes = b"") -> bytes:
        return t + _I32.pack(len(payload) + 4) + payload

    def _row_desc(self, cols: List[str]) -> bytes:
        body = [_I16.pack(len(cols))]
        for c in cols:
            body.append(c.encode() + b"\x00")
            body.append(struct.pack(">ihihih", 0, 0, 25, -1, -1, 0))
        return self._msg(b"T", b"".join(body))

    def _data_row(self, vals: List[Optional[str]]) -> bytes:
        body = [_I16.pack(len(vals))]
        for v in vals:
            if v is None:
                body.append(_I32.pack(-1))
            else:
                b = v.encode("utf-8")
                body.append(_I32.pack(len(b)) + b)
        return self._msg(b"D", b"".join(body))

    # the CommandComplete frames of the fixed tags, built once
    _COMPLETE = {
        tag: b"C" + _I32.pack(len(tag) + 5) + tag.encode() + b"\x00"
        for tag in ("INSERT 0 1", "DELETE 1", "DELETE 0", "UPDATE 1",
                    "UPDATE 0", "SELECT 1", "SELECT 0", "BEGIN", "COMMIT",
                    "ROLLBACK", "CREATE TABLE")}

    def _complete(self, tag: str) -> bytes:
        return self._COMPLETE.get(tag) or \
            self._msg(b"C", tag.encode() + b"\x00")

    def _result(self, cols: List[str], rows: List[list]) -> List[bytes]:
        """A whole SELECT answer: description, rows, completion tag."""
        return ([self._row_desc(cols)] + [self._data_row(r) for r in rows]
                + [self._complete("SELECT %d" % len(rows))])

    def _error(self, code: str, msg: str) -> bytes:
        fields = b"SERROR\x00" + b"C" + code.encode() + b"\x00" + \
            b"M" + msg.encode() + b"\x00" + b"\x00"
        return self._msg(b"E", fields)

    def _ready(self, status: str = "I") -> bytes:
        return self._msg(b"Z", status.encode())

    async def _serve_libpq(self, first: bytes,
                           reader: asyncio.StreamReader,
                           writer: asyncio.StreamWriter) -> None:
        try:
            while True:     # startup negotiation (SSL probe then startup)
                rest = await reader.readexactly(3)
                (length,) = struct.unpack(">I", first + rest)
                if length < 4 or length - 4 > MAX_MSG:
                    writer.close()
                    return
                payload = await reader.readexactly(length - 4)
                (code,) = struct.unpack_from(">i", payload)
                if code in (SSL_REQUEST, GSSENC_REQUEST):
                    writer.write(b"N")      # no TLS; client retries plain
                    await writer.drain()
                    first = await reader.readexactly(1)
                    continue
                if code == CANCEL_REQUEST:
                    writer.close()
                    return
                if code != PROTOCOL_V3:
                    writer.write(self._error(
                        "08P01", "unsupported protocol %d" % code))
                    await writer.drain()
                    writer.close()
                    return
                break
            # AuthenticationOk + parameters + ReadyForQuery
            out = [self._msg(b"R", _I32.pack(0))]
            for k, v in (("server_version", self.pg_major + ".0 (minipg)"),
                         ("client_encoding", "UTF8"),
                         ("server_encoding", "UTF8"),
                         ("integer_datetimes", "on")):
                out.append(self._msg(
                    b"S", k.encode() + b"\x00" + v.encode() + b"\x00"))
            out.append(self._msg(b"K", struct.pack(">ii", os.getpid(), 0)))
            out.append(self._ready())
            writer.write(b"".join(out))
            await writer.drain()

            sess = _Session()
            while True:
                hdr = await reader.readexactly(5)
                t = hdr[:1]
                (ln,) = struct.unpack(">I", hdr[1:])
                if ln < 4 or ln - 4 > MAX_MSG:
                    writer.write(self._error(
                        "08P01", "invalid message length %d" % ln))
                    await writer.drain()
                    return
                payload = await reader.readexactly(ln - 4)
                if t == b"X":
                    return
                if t == b"Q":
                    if sess.staged or sess.skip:
                        # a simple query ends an unsynced extended sequence
                        await self._flush_staged(sess, writer, sync=False)
                        sess.skip = False
                    sql = payload.rstrip(b"\x00").decode("utf-8")
                    await self._run_query_cycle(sql, writer, sess)
                elif t in self._EXTENDED:
                    await self._extended(t, payload, sess, writer)
                else:
                    writer.write(self._error(
                        "0A000", "unsupported frontend message %r"
                        % t.decode("latin-1")))
                    writer.write(self._ready(sess.txn))
                    await writer.drain()
        except (asyncio.IncompleteReadError, ConnectionError,
                asyncio.CancelledError):
            pass
        except Exception as exc:
            self.log.error("libpq connection error", err=exc)
        finally:
            try:
                writer.close()
            except Exception:
                pass

    async def _run_query_cycle(self, sql: str,
                               writer: asyncio.StreamWriter,
                               sess: _Session) -> None:
        """One simple-Query cycle: possibly multiple statements, one
        ReadyForQuery at the end; an error aborts the rest (as the real
        backend does).  GROUP COMMIT: every write in the statement list
        is appended immediately and the whole cycle waits once for the
        highest LSN's sync ack, so a multi-statement INSERT batch pays
        one replication round trip, not one per row."""
        staged: List[bytes] = []
        max_lsn = None
        err: Optional[PgSqlError] = None
        for stmt in split_statements(sql) or [""]:
            try:
                chunks, lsn = self._execute_staged(stmt, sess)
            except PgSqlError as exc:
                err = exc
                break
            staged.extend(chunks)
            if lsn is not None:
                max_lsn = lsn
        if max_lsn is not None:
            res = await self._await_commit(max_lsn)
            if not res.get("ok"):
                # gate broke while waiting (e.g. read-only flipped):
                # nothing in this cycle may be acknowledged
                staged = []
                err = err or PgSqlError("25006", res.get("error",
                                                         "commit failed"))
        for chunk in staged:
            writer.write(chunk)
        if err is not None:
            sess.fail()
            writer.write(self._error(err.code, err.msg))
        writer.write(self._ready(sess.txn))
        await writer.drain()

    def _execute_staged(self, stmt: str, sess: _Session
                        ) -> Tuple[List[bytes], Optional[int]]:
        """One statement of a simple-Query cycle as wire chunks.  Writes
        append-without-waiting (their acks are withheld until the
        cycle's single commit gate); everything else executes
        directly."""
        kind, cols, arg = self._plan(stmt)
        rows, tag, lsn = self._run(kind, arg, sess)
        if cols is not None:
            return self._result(cols, rows), lsn
        if tag is None:
            return [self._msg(b"I")], lsn       # EmptyQueryResponse
        return [self._complete(tag)], lsn

    def _append_sql(self, op: dict, verb: str) -> int:
        lsn, err = self._append_write(op)
        if err is not None:
            msg = err.get("error", "")
            if "read-only" in msg:
                raise PgSqlError(
                    "25006",
                    "cannot execute %s in a read-only transaction" % verb)
            raise PgSqlError("XX000", msg or "write failed")
        return lsn

    # --------------------------------------------- extended-query protocol
    _EXTENDED = frozenset((b"P", b"B", b"D", b"E", b"C", b"S", b"H"))

    async def _extended(self, t: bytes, payload: bytes, sess: _Session,
                        writer: asyncio.StreamWriter) -> None:
        """One extended-protocol message.  All output is STAGED in the
        session and reaches the socket only at Sync or Flush, behind one
        commit gate for the highest LSN appended so far — the simple
        path's durability rule: no CommandComplete for a write is sent
        before its WAL record passed ``_await_commit``.  After an error
        every message up to the next Sync is discarded."""
        if t == b"S":
            return await self._flush_staged(sess, writer, sync=True)
        if t == b"H":
            return await self._flush_staged(sess, writer, sync=False)
        if sess.skip:
            return
        try:
            try:
                if t == b"P":
                    self._on_parse(payload, sess)
                elif t == b"B":
                    self._on_bind(payload, sess)
                elif t == b"D":
                    self._on_describe(payload, sess)
                elif t == b"E":
                    self._on_execute(payload, sess)
                else:
                    self._on_close(payload, sess)
            except (struct.error, ValueError, IndexError) as exc:
                raise PgSqlError("08P01", "malformed %s message: %s"
                                 % (t.decode(), exc))
        except PgSqlError as exc:
            sess.fail()
            sess.staged.append(self._error(exc.code, exc.msg))
            sess.skip = True

    async def _flush_staged(self, sess: _Session,
                            writer: asyncio.StreamWriter,
                            sync: bool) -> None:
        if sess.max_lsn is not None:
            lsn, sess.max_lsn = sess.max_lsn, None
            res = await self._await_commit(lsn)
            if not res.get("ok"):
                # as in _run_query_cycle: nothing staged may be
                # acknowledged once the gate broke
                sess.fail()
                sess.staged = [self._error(
                    "25006", res.get("error", "commit failed"))]
                sess.skip = True
        if sess.staged:
            writer.write(b"".join(sess.staged))
            sess.staged = []
        if sync:
            sess.skip = False
            if sess.txn == "I":
                sess.portals.clear()    # portals end with the transaction
            writer.write(self._ready(sess.txn))
        await writer.drain()

    def _check_failed(self, sess: _Session, kind: str) -> None:
        if sess.txn == "E" and kind not in ("commit", "rollback"):
            raise PgSqlError(
                "25P02", "current transaction is aborted, commands "
                "ignored until end of transaction block")

    def _on_parse(self, p: bytes, sess: _Session) -> None:
        name, pos = _cstr(p, 0)
        sql, pos = _cstr(p, pos)
        # declared parameter type oids are ignored: everything is text
        (ntypes,) = _I16.unpack_from(p, pos)
        if ntypes < 0 or pos + 2 + 4 * ntypes > len(p):
            raise ValueError("parameter type list runs past the message")
        if name and name in sess.stmts:
            raise PgSqlError("42P05", 'prepared statement "%s" already '
                             'exists' % name)
        parts = split_statements(sql)
        if len(parts) > 1:
            raise PgSqlError("42601", "cannot insert multiple commands "
                             "into a prepared statement")
        text = parts[0] if parts else ""
        nparams = count_params(text)
        # plan with empty literals in the parameters' places: what kind
        # of statement this is never depends on a literal's content
        kind, cols, _ = self._plan(bind_params(text, [""] * nparams))
        self._check_failed(sess, kind)
        sess.stmts[name] = (text, nparams, cols)
        sess.staged.append(self._msg(b"1"))

    def _on_bind(self, p: bytes, sess: _Session) -> None:
        portal, pos = _cstr(p, 0)
        stmt, pos = _cstr(p, pos)
        (nfmt,) = _I16.unpack_from(p, pos)
        fmts = struct.unpack_from(">%dh" % nfmt, p, pos + 2)
        pos += 2 + 2 * nfmt
        (nparams,) = _I16.unpack_from(p, pos)
        pos += 2
        raw: List[Optional[bytes]] = []
        for _ in range(nparams):
            (ln,) = _I32.unpack_from(p, pos)
            pos += 4
            if ln < 0:
                raw.append(None)
            else:
                if pos + ln > len(p):
                    raise ValueError("parameter runs past the message")
                raw.append(p[pos:pos + ln])
                pos += ln
        (nres,) = _I16.unpack_from(p, pos)
        fmts += struct.unpack_from(">%dh" % nres, p, pos + 2)
        if stmt not in sess.stmts:
            raise PgSqlError("26000", 'prepared statement "%s" does not '
                             'exist' % stmt)
        text, want, _cols = sess.stmts[stmt]
        if nparams != want:
            raise PgSqlError(
                "08P01", 'bind message supplies %d parameters, but prepared '
                'statement "%s" requires %d' % (nparams, stmt, want))
        if any(fmts):
            raise PgSqlError("0A000", "binary parameter and result "
                             "formats are not supported")
        if portal and portal in sess.portals:
            raise PgSqlError("42P03", 'cursor "%s" already exists' % portal)
        try:
            params = [None if b is None else b.decode("utf-8") for b in raw]
        except UnicodeDecodeError:
            raise PgSqlError("22021", "invalid byte sequence for encoding "
                             '"UTF8"')
        kind, cols, arg = self._plan(bind_params(text, params))
        self._check_failed(sess, kind)
        sess.portals[portal] = _Portal(stmt, kind, cols, arg)
        sess.staged.append(self._msg(b"2"))

    def _on_describe(self, p: bytes, sess: _Session) -> None:
        """Answered from the plan alone: nothing executes."""
        what = p[:1]
        name, _ = _cstr(p, 1)
        if what == b"S":
            if name not in sess.stmts:
                raise PgSqlError("26000", 'prepared statement "%s" does '
                                 'not exist' % name)
            _text, nparams, cols = sess.stmts[name]
            sess.staged.append(self._msg(
                b"t", _I16.pack(nparams) + _I32.pack(25) * nparams))
        elif what == b"P":
            if name not in sess.portals:
                raise PgSqlError("34000", 'portal "%s" does not exist'
                                 % name)
            cols = sess.portals[name].cols
        else:
            raise ValueError("describe target %r" % what)
        sess.staged.append(self._row_desc(cols) if cols is not None
                           else self._msg(b"n"))

    def _on_execute(self, p: bytes, sess: _Session) -> None:
        name, pos = _cstr(p, 0)
        (max_rows,) = _I32.unpack_from(p, pos)
        portal = sess.portals.get(name)
        if portal is None:
            raise PgSqlError("34000", 'portal "%s" does not exist' % name)
        if portal.cols is None:
            if portal.rows is not None:
                raise PgSqlError("55000", 'portal "%s" cannot be run'
                                 % name)
            portal.rows = []
            _rows, tag, lsn = self._run(portal.kind, portal.arg, sess)
            if lsn is not None:
                sess.max_lsn = lsn
            sess.staged.append(self._complete(tag) if tag is not None
                               else self._msg(b"I"))
            return
        if portal.rows is None:
            portal.rows, _tag, _lsn = self._run(portal.kind, portal.arg,
                                                sess)
        left = len(portal.rows) - portal.pos
        n = min(left, max_rows) if max_rows > 0 else left
        for row in portal.rows[portal.pos:portal.pos + n]:
            sess.staged.append(self._data_row(row))
        portal.pos += n
        if n < left:
            sess.staged.append(self._msg(b"s"))     # PortalSuspended
        else:
            # the tag counts the rows of THIS Execute, as PostgreSQL's
            sess.staged.append(self._complete("SELECT %d" % n))

    def _on_close(self, p: bytes, sess: _Session) -> None:
        what = p[:1]
        name, _ = _cstr(p, 1)
        if what == b"S":
            if sess.stmts.pop(name, None) is not None:
                for pname in [n for n, po in sess.portals.items()
                              if po.stmt == name]:
                    del sess.portals[pname]
        elif what == b"P":
            sess.portals.pop(name, None)
        else:
            raise ValueError("close target %r" % what)
        sess.staged.append(self._msg(b"3"))

    # ------------------------------------------------------------ SQL layer
    _RE_INSERT = re.compile(
        r"insert\s+into\s+kv\s*\(\s*k\s*,\s*v\s*\)\s*values\s*\(\s*"
        r"'((?:[^']|'')*)'\s*,\s*'((?:[^']|'')*)'\s*\)", re.I)
    _RE_SELECT_V = re.compile(
        r"select\s+v\s+from\s+kv\s+where\s+k\s*=\s*'((?:[^']|'')*)'", re.I)
    _RE_COUNT = re.compile(
        r"select\s+count\(\*\)\s+(?:as\s+\w+\s+)?from\s+kv"
        r"(?:\s+where\s+k\s+like\s+'((?:[^']|'')*)%')?", re.I)
    _RE_DELETE = re.compile(
        r"delete\s+from\s+kv\s+where\s+k\s*=\s*'((?:[^']|'')*)'", re.I)
    _RE_UPDATE = re.compile(
        r"update\s+kv\s+set\s+v\s*=\s*'((?:[^']|'')*)'\s*"
        r"where\s+k\s*=\s*'((?:[^']|'')*)'", re.I)

    _TXN_WORDS = {"begin": "begin", "commit": "commit", "end": "commit",
                  "rollback": "rollback", "abort": "rollback"}

    @staticmethod
    def _verb(rx, stmt: str):
        """``rx`` found in ``stmt`` as the statement itself.  A match
        with a quote before it lies inside or behind a literal — the
        TEXT of a key or value, never the command."""
        m = rx.search(stmt)
        if m is not None and m.start() and "'" in stmt[:m.start()]:
            return None
        return m

    def _plan(self, stmt: str):
        """What a statement is, without running it:
        ``(kind, columns, arg)``.  ``columns`` is None for a statement
        that returns no rows, otherwise exactly the column names
        ``_run``'s rows come with — Describe answers from here."""
        if stmt[:1] in "sS":
            # the read hot path: a statement that BEGINS as a key lookup
            # is one, without a look at the other patterns
            m = self._RE_SELECT_V.match(stmt)
            if m:
                return "select_v", ["v"], sql_unquote(m.group(1))
        m = self._RE_INSERT.search(stmt)        # _verb, inlined: hot
        if m and not (m.start() and "'" in stmt[:m.start()]):
            return "insert", None, (sql_unquote(m.group(1)),
                                    sql_unquote(m.group(2)))
        m = self._verb(self._RE_DELETE, stmt)
        if m:
            return "delete", None, sql_unquote(m.group(1))
        m = self._verb(self._RE_UPDATE, stmt)
        if m:
            return "update", None, (sql_unquote(m.group(2)),
                                    sql_unquote(m.group(1)))

        # keywords are looked for outside literals only
        low = stmt.lower()
        if "'" in low:
            low = _RE_LITERAL.sub("''", low)
        low = " ".join(low.split())
        if not low:
            return "empty", None, None

        word = low.split(" ", 1)[0]
        if word in self._TXN_WORDS or low.startswith("start transaction"):
            if "savepoint" in low or low.startswith("rollback to"):
                raise PgSqlError("0A000", "savepoints are not supported")
            return self._TXN_WORDS.get(word, "begin"), None, None

        if low.startswith("create table"):
            return "create", None, None

        if "current_time" in low and "from" not in low:
            return "current_time", ["current_time"], None

        if "pg_is_in_recovery" in low:
            return "in_recovery", ["r"], None

        if "pg_current_wal_lsn" in low or "pg_current_xlog_location" in low:
            return "current_lsn", ["loc"], None

        if "pg_last_wal_replay_lsn" in low or \
                "pg_last_xlog_replay_location" in low:
            return "replay_lsn", ["loc"], None

        if "pg_last_xact_replay_timestamp" in low:
            return "replay_ts", ["t"], None

        if "pg_stat_wal_receiver" in low:
            return "wal_receiver", ["status", "conninfo"], None

        if "pg_stat_replication" in low:
            w = self.lsn_word
            return "stat_replication", [
                "pid", "application_name", "client_addr", "state",
                "sent_" + w, "write_" + w, "flush_" + w, "replay_" + w,
                "sync_state"], None

        m = self._verb(self._RE_SELECT_V, stmt)
        if m:
            return "select_v", ["v"], sql_unquote(m.group(1))
        m = self._verb(self._RE_COUNT, stmt)
        if m:
            return "count", ["count"], sql_unquote(m.group(1) or "")
        raise PgSqlError("42601", 'syntax error at or near "%s"'
                         % stmt.split()[0][:40])

    def _run(self, kind: str, arg, sess: _Session
             ) -> Tuple[Optional[List[list]], Optional[str], Optional[int]]:
        """Execute a planned statement: ``(rows, tag, lsn)``.  ``rows``
        is None unless the plan has columns; ``tag`` is None for the
        empty query and for row-returning statements (their tag is the
        row count); ``lsn`` is the WAL position a write still has to
        pass the commit gate for."""
        if kind == "insert":
            op = {"op": "put", "k": arg[0], "v": arg[1]}
            if sess.txn == "I":
                return None, "INSERT 0 1", self._append_sql(op, "INSERT")
            self._buffer(sess, op, "INSERT")
            return None, "INSERT 0 1", None

        if kind == "select_v":
            if sess.txn != "I":
                self._check_failed(sess, kind)
            found, v = self._txn_get(sess, arg)
            return ([[str(v)]] if found else []), None, None

        if sess.txn == "E":
            self._check_failed(sess, kind)

        if kind == "delete":
            if not self._txn_get(sess, arg)[0]:
                return None, "DELETE 0", None
            op = {"op": "del", "k": arg}
            if sess.txn == "I":
                return None, "DELETE 1", self._append_sql(op, "DELETE")
            self._buffer(sess, op, "DELETE")
            return None, "DELETE 1", None

        if kind == "update":
            if not self._txn_get(sess, arg[0])[0]:
                return None, "UPDATE 0", None
            op = {"op": "put", "k": arg[0], "v": arg[1]}
            if sess.txn == "I":
                return None, "UPDATE 1", self._append_sql(op, "UPDATE")
            self._buffer(sess, op, "UPDATE")
            return None, "UPDATE 1", None

        if kind == "count":
            return [[str(self._txn_count(sess, arg))]], None, None

        if kind == "begin":
            if sess.txn == "I":
                sess.txn = "T"
            return None, "BEGIN", None

        if kind == "commit":
            was, ops = sess.txn, sess.ops
            sess.end_txn()
            if was == "E":
                return None, "ROLLBACK", None
            if not ops:
                return None, "COMMIT", None
            # the whole block is ONE WAL record: all-or-nothing across
            # a crash and across replication
            return None, "COMMIT", self._append_sql(
                {"op": "batch", "ops": ops}, "COMMIT")

        if kind == "rollback":
            sess.end_txn()
            return None, "ROLLBACK", None

        if kind == "empty":
            return None, None, None

        if kind == "create":
            return None, "CREATE TABLE", None

        if kind == "current_time":
            now = datetime.datetime.now(datetime.timezone.utc)
            return [[now.strftime("%H:%M:%S.%f%z")]], None, None

        if kind == "in_recovery":
            return [["t" if self.role == "standby" else "f"]], None, None

        if kind == "current_lsn":
            if self.role == "standby":
                raise PgSqlError("55000", "recovery is in progress")
            return [[lsnmod.format_lsn(self.wal.end)]], None, None

        if kind == "replay_lsn":
            val = (lsnmod.format_lsn(self.replay_lsn)
                   if self.role == "standby" else None)
            return [[val]], None, None

        if kind == "replay_ts":
            val = ("%f" % self.last_replay_time
                   if (self.role == "standby" and self.last_replay_time)
                   else None)
            return [[val]], None, None

        if kind == "wal_receiver":
            # the standby-side receiver status (real PG ≥9.6): one row
            # while this server is a standby.  'diverged' is a minipg
            # extension (real PG surfaces divergence only in its log);
            # the manager uses it to trigger the restore-on-divergence
            # path (ref standby-failure ⇒ restore :1339-1373).
            rows = []
            if self.role == "standby":
                status = {"streaming": "streaming",
                          "diverged": "diverged"}.get(
                              self.upstream_status, "stopped")
                rows.append([status, "host=%s" % (self.upstream or "")])
            return rows, None, None

        if kind == "stat_replication":
            return self._stat_replication(), None, None

        raise PgSqlError("XX000", "unplanned statement kind %r" % kind)

    # ---------------------------------------------------- transaction block
    def _buffer(self, sess: _Session, op: dict, verb: str) -> None:
        """A write inside a block: nothing reaches the WAL before
        COMMIT.  The read-only check is made here too, so the statement
        fails where PostgreSQL's would, not only at COMMIT."""
        if sess.txn == "E":
            self._check_failed(sess, "write")
        settings = self.settings
        if settings.role != "primary" or settings.read_only:
            raise PgSqlError(
                "25006",
                "cannot execute %s in a read-only transaction" % verb)
        sess.ops_bytes += len(encode_op(op))
        if sess.ops_bytes > MAX_MSG:
            raise PgSqlError(
                "54000", "transaction exceeds %d bytes of buffered writes"
                % MAX_MSG)
        sess.ops.append(op)
        sess.pending[op["k"]] = op["v"] if op["op"] == "put" else _TOMBSTONE

    def _txn_get(self, sess: _Session, k: str) -> Tuple[bool, object]:
        """Committed state overlaid with the block's own writes."""
        if sess.pending and k in sess.pending:
            v = sess.pending[k]
            return (False, None) if v is _TOMBSTONE else (True, v)
        return self.get(k)

    def _txn_count(self, sess: _Session, prefix: str) -> int:
        n = self.count(prefix)
        for k, v in sess.pending.items():
            if prefix and not k.startswith(prefix):
                continue
            if v is _TOMBSTONE:
                n -= k in self.kv
            else:
                n += k not in self.kv
        return n

    def _stat_replication(self) -> List[list]:
        rows = []
        for rep, row in self.replica_rows():
            addr = None
            try:
                peer = rep.writer.get_extra_info("peername")
                addr = peer[0] if peer else None
            except Exception:
                pass
            rows.append([
                str(os.getpid()), row["application_name"], addr,
                row["state"], row["sent_lsn"], row["write_lsn"],
                row["flush_lsn"], row["replay_lsn"], row["sync_state"]])
        return rows


# ---------------------------------------------------------------- binaries

def init_data_dir(data_dir: str, version: str) -> None:
    """The initdb analogue: PG_VERSION (major), system identity,
    timeline 1 (ref _prepareDatabase lib/postgresMgr.js:1806-1987)."""
    waldb_init(data_dir)
    with open(os.path.join(data_dir, "PG_VERSION"), "w") as f:
        f.write(pg_strip_minor(version) + "\n")


def initdb_main(version: str, argv=None) -> int:
    ap = argparse.ArgumentParser(prog="initdb (minipg)")
    ap.add_argument("-D", "--pgdata", required=True)
    ap.add_argument("-E", "--encoding", default="UTF8")
    ap.add_argument("-U", "--username", default=None)
    ns, _ = ap.parse_known_args(argv)
    if os.path.exists(os.path.join(ns.pgdata, "PG_VERSION")):
        print("initdb: directory %s is not empty" % ns.pgdata,
              file=sys.stderr)
        return 1
    init_data_dir(ns.pgdata, version)
    print("Success. You can now start the database server.")
    return 0


def postgres_main(version: str, argv=None) -> int:
    ap = argparse.ArgumentParser(prog="postgres (minipg)")
    ap.add_argument("-D", "--pgdata", required=True)
    ns, _ = ap.parse_known_args(argv)
    data_dir = os.path.abspath(ns.pgdata)
    log = Logger("minipg", level=level_from_verbosity(1),
                 path=os.path.join(os.path.dirname(data_dir),
                                   "minipg.log"))
    return run_server(MinipgServer(data_dir, log))


def main(argv=None) -> int:
    """module entry: ``python -m manatee_amd.db.minipg -D dir
    [--init] [--pg-version 12.0]``."""
    ap = argparse.ArgumentParser(prog="minipg")
    ap.add_argument("-D", "--pgdata", required=True)
    ap.add_argument("--init", action="store_true")
    ap.add_argument("--pg-version", default="12.0")
    ns = ap.parse_args(argv)
    if ns.init:
        return initdb_main(ns.pg_version, ["-D", ns.pgdata])
    return postgres_main(ns.pg_version, ["-D", ns.pgdata])


if __name__ == "__main__":
    sys.exit(main())
