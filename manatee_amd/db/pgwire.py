"""Minimal PostgreSQL v3 wire-protocol client (asyncio).

The admin/health paths need exactly what the reference uses the ``pg``
module for (ref lib/postgresMgr.js:1990-2172, lib/adm.js:348-427): a
single connection running simple queries (``SELECT current_time``,
``pg_stat_replication``, LSN functions) serially.  This speaks the v3
protocol directly — StartupMessage, trust/ident auth (no password
flows), simple Query, row decoding as text — with a serialized query
queue like the reference's (one query in flight per connection,
working around node-postgres #718).

The write-load drivers additionally use the extended-query protocol:
bound parameters (text format only), named prepared statements,
pipelines of many Bind/Execute pairs under one Sync, and transaction
blocks.  Every call, simple or extended, holds the same lock for its
whole request/response cycle and tears the connection down on a
transport error.
"""

from __future__ import annotations

import asyncio
import struct
from typing import Dict, List, Optional, Sequence, Tuple

from ..common import dial

_I32 = struct.Struct(">i")
_I16 = struct.Struct(">h")
_HDR = struct.Struct(">cI")     # type byte + length (len includes itself)

PROTOCOL_VERSION = 196608       # 3.0

# ReadyForQuery payload -> transaction status
_TXN_STATUS = {b"I": "I", b"T": "T", b"E": "E"}


class PgError(RuntimeError):
    def __init__(self, fields: Dict[str, str]):
        self.fields = fields
        # set when raised out of pipeline(): the entry that failed and
        # the results of the entries before it
        self.pipeline_index: Optional[int] = None
        self.pipeline_results: List["PgResult"] = []
        super().__init__(fields.get("M", "postgres error"))

    @property
    def code(self) -> str:
        return self.fields.get("C", "")


class PgResult:
    def __init__(self, columns: List[str], rows: List[Tuple],
                 command: str = ""):
        self.columns = columns
        self.rows = rows
        self.command = command

    def dicts(self) -> List[dict]:
        return [dict(zip(self.columns, r)) for r in self.rows]


def _cstr(b: bytes, pos: int) -> Tuple[str, int]:
    end = b.index(b"\x00", pos)
    return b[pos:end].decode("utf-8"), end + 1


def _frame(t: bytes, body: bytes) -> bytes:
    return t + _I32.pack(len(body) + 4) + body


def _row_description(payload: bytes) -> List[str]:
    (n,) = struct.unpack_from(">h", payload)
    pos = 2
    columns = []
    for _ in range(n):
        name, pos = _cstr(payload, pos)
        pos += 18    # table oid, attnum, type oid, len, mod, fmt
        columns.append(name)
    return columns


def _data_row(payload: bytes) -> Tuple:
    (n,) = struct.unpack_from(">h", payload)
    pos = 2
    row = []
    for _ in range(n):
        (ln,) = struct.unpack_from(">i", payload, pos)
        pos += 4
        if ln == -1:
            row.append(None)
        else:
            row.append(payload[pos:pos + ln].decode("utf-8"))
            pos += ln
    return tuple(row)


# ------------------------------------------- extended-protocol frontend
def _parse_msg(name: str, sql: str) -> bytes:
    return _frame(b"P", name.encode("utf-8") + b"\x00"
                  + sql.encode("utf-8") + b"\x00" + _I16.pack(0))


def _bind_msg(portal: str, stmt: str, params: Sequence) -> bytes:
    """Bind with every parameter and every result column in text format
    (no format codes = all text).  None is sent as SQL NULL; anything
    that is not a string goes through ``str()``."""
    body = [portal.encode("utf-8"), b"\x00", stmt.encode("utf-8"), b"\x00",
            _I16.pack(0), _I16.pack(len(params))]
    for p in params:
        if p is None:
            body.append(_I32.pack(-1))
        else:
            b = (p if isinstance(p, str) else str(p)).encode("utf-8")
            body.append(_I32.pack(len(b)))
            body.append(b)
    body.append(_I16.pack(0))
    return _frame(b"B", b"".join(body))


_DESCRIBE_PORTAL = _frame(b"D", b"P\x00")
_EXECUTE_ALL = _frame(b"E", b"\x00" + _I32.pack(0))
_SYNC = _frame(b"S", b"")


class PgClient:
    """One serialized connection (queries run one at a time)."""

    def __init__(self, host: str, port: int, user: str,
                 database: str = "postgres",
                 connect_timeout_s: float = 10.0):
        self.host = host
        self.port = port
        self.user = user
        self.database = database
        self.connect_timeout_s = connect_timeout_s
        self._reader: Optional[asyncio.StreamReader] = None
        self._writer: Optional[asyncio.StreamWriter] = None
        self._lock = asyncio.Lock()
        self.parameters: Dict[str, str] = {}
        # transaction status of the last ReadyForQuery: I idle, T in a
        # block, E in a failed block
        self.txn_status = "I"
        # named statements prepared on THIS connection (name -> sql)
        self._prepared: Dict[str, str] = {}

    # ------------------------------------------------------------ lifecycle
    async def connect(self) -> None:
        """TCP connect + startup/auth handshake, ALL bounded by
        connect_timeout_s: a backend that accepts the connection but
        never answers the startup packet (dying process, half-open
        socket after a partition) must not hang the caller forever."""
        try:
            await asyncio.wait_for(self._connect(),
                                   self.connect_timeout_s)
        except BaseException:
            self._teardown()
            raise

    def _teardown(self) -> None:
        """Forget the connection, and with it everything that lived on
        it: the open transaction block and the prepared statements."""
        writer = self._writer
        self._writer = None
        self._reader = None
        self.txn_status = "I"
        self._prepared = {}
        if writer is not None:
            try:
                writer.close()
            except Exception:
                pass

    async def _connect(self) -> None:
        self._reader, self._writer = await dial.open_connection(
            self.host, self.port)
        params = ("user\x00%s\x00database\x00%s\x00\x00"
                  % (self.user, self.database)).encode("utf-8")
        body = _I32.pack(PROTOCOL_VERSION) + params
        self._writer.write(_I32.pack(len(body) + 4) + body)
        await self._writer.drain()
        # authentication + parameter flow until ReadyForQuery
        while True:
            t, payload = await self._recv()
            if t == b"R":
                (auth,) = _I32.unpack_from(payload)
                if auth != 0:
                    raise PgError({"M": "unsupported auth method %d (only "
                                        "trust/ident)" % auth})
            elif t == b"S":
                key, pos = _cstr(payload, 0)
                val, _ = _cstr(payload, pos)
                self.parameters[key] = val
            elif t == b"K":      # BackendKeyData
                pass
            elif t == b"Z":      # ReadyForQuery
                self.txn_status = _TXN_STATUS.get(payload, "I")
                return
            elif t == b"E":
                raise PgError(self._err_fields(payload))

    async def close(self) -> None:
        if self._writer is not None:
            try:
                self._writer.write(b"X" + _I32.pack(4))  # Terminate
                await self._writer.drain()
            except (ConnectionError, OSError):
                pass
            self._teardown()

    @property
    def connected(self) -> bool:
        return self._writer is not None

    # --------------------------------------------------------------- query
    async def _guarded(self, coro, timeout_s: float):
        """One request/response cycle: serialized on the connection,
        bounded by ``timeout_s``.  Any transport-level failure (EOF
        from a dead backend, timeout, reset) tears the connection down
        so the next use reconnects — a stale cached connection must
        never masquerade as a live one."""
        try:
            async with self._lock:   # serialized, ref :1990-2172
                try:
                    return await asyncio.wait_for(coro, timeout_s)
                except (asyncio.IncompleteReadError, EOFError,
                        ConnectionError, OSError, asyncio.TimeoutError):
                    self._teardown()
                    raise
        finally:
            coro.close()    # never started (cancelled at the lock)

    async def query(self, sql: str,
                    timeout_s: float = 30.0) -> PgResult:
        """Simple-protocol query; returns the LAST result set.  Any
        transport-level failure (EOF from a dead backend, timeout,
        reset) tears the connection down so the next use reconnects —
        a stale cached connection must never masquerade as a live one."""
        # _guarded, spelled out: this is the hot path of every driver
        async with self._lock:   # serialized, ref :1990-2172
            try:
                return await asyncio.wait_for(self._query(sql), timeout_s)
            except (asyncio.IncompleteReadError, EOFError,
                    ConnectionError, OSError, asyncio.TimeoutError):
                self._teardown()
                raise

    async def _query(self, sql: str) -> PgResult:
        if self._writer is None:
            raise PgError({"M": "not connected"})
        body = sql.encode("utf-8") + b"\x00"
        self._writer.write(b"Q" + _I32.pack(len(body) + 4) + body)
        await self._writer.drain()
        columns: List[str] = []
        rows: List[Tuple] = []
        command = ""
        error: Optional[PgError] = None
        while True:
            t, payload = await self._recv()
            if t == b"T":        # RowDescription
                (n,) = struct.unpack_from(">h", payload)
                pos = 2
                columns = []
                for _ in range(n):
                    name, pos = _cstr(payload, pos)
                    pos += 18    # table oid, attnum, type oid, len, mod, fmt
                    columns.append(name)
                rows = []
            elif t == b"D":      # DataRow
                (n,) = struct.unpack_from(">h", payload)
                pos = 2
                row = []
                for _ in range(n):
                    (ln,) = struct.unpack_from(">i", payload, pos)
                    pos += 4
                    if ln == -1:
                        row.append(None)
                    else:
                        row.append(payload[pos:pos + ln].decode("utf-8"))
                        pos += ln
                rows.append(tuple(row))
            elif t == b"C":      # CommandComplete
                command, _ = _cstr(payload, 0)
            elif t == b"E":
                error = PgError(self._err_fields(payload))
            elif t == b"Z":      # ReadyForQuery — end of cycle
                self.txn_status = _TXN_STATUS.get(payload, "I")
                if error is not None:
                    raise error
                return PgResult(columns, rows, command)
            # 'N' (notice), 'S' (parameter), 'I' (empty) are ignored

    # ------------------------------------------------------ extended query
    async def query_params(self, sql: str, params: Sequence = (),
                           timeout_s: float = 30.0) -> PgResult:
        """One parameterised statement: unnamed Parse, Bind, Describe
        (portal), Execute and Sync in one write."""
        return (await self._guarded(
            self._extended([("", sql, params)]), timeout_s))[0]

    async def prepare(self, name: str, sql: str,
                      timeout_s: float = 30.0) -> None:
        """Create the named prepared statement ``name`` on this
        connection (it is gone when the connection is)."""
        if not name:
            raise ValueError("a prepared statement needs a name")
        await self._guarded(self._prepare(name, sql), timeout_s)

    async def _prepare(self, name: str, sql: str) -> None:
        if self._writer is None:
            raise PgError({"M": "not connected"})
        self._writer.write(_parse_msg(name, sql) + _SYNC)
        await self._writer.drain()
        _results, error = await self._read_extended()
        if error is not None:
            raise error
        self._prepared[name] = sql

    def is_prepared(self, name: str) -> bool:
        return name in self._prepared

    async def execute_prepared(self, name: str, params: Sequence = (),
                               timeout_s: float = 30.0) -> PgResult:
        return (await self._guarded(
            self._extended([(name, None, params)]), timeout_s))[0]

    async def pipeline(self, entries, timeout_s: float = 30.0
                       ) -> List[PgResult]:
        """Many statements, one round trip: a Bind/Describe/Execute
        group per ``(name_or_sql, params)`` entry, ONE Sync at the end.
        An entry naming a statement prepared on this connection is
        bound to it; any other string is SQL for the unnamed statement.
        Returns one result per entry.  The server stops at the first
        failing entry and runs none after it; that error is raised with
        ``pipeline_index`` and ``pipeline_results`` (the entries that
        completed before it) set."""
        plan = []
        for what, params in entries:
            if what in self._prepared:
                plan.append((what, None, params))
            else:
                plan.append(("", what, params))
        if not plan:
            return []
        return await self._guarded(self._extended(plan), timeout_s)

    async def _extended(self, plan) -> List[PgResult]:
        if self._writer is None:
            raise PgError({"M": "not connected"})
        out = []
        for name, sql, params in plan:
            if sql is not None:
                out.append(_parse_msg(name, sql))
            out.append(_bind_msg("", name, params))
            out.append(_DESCRIBE_PORTAL)
            out.append(_EXECUTE_ALL)
        out.append(_SYNC)
        self._writer.write(b"".join(out))
        await self._writer.drain()
        results, error = await self._read_extended()
        if error is not None:
            error.pipeline_index = len(results)
            error.pipeline_results = results
            raise error
        return results

    async def _read_extended(self
                             ) -> Tuple[List[PgResult], Optional[PgError]]:
        """Read up to the ReadyForQuery that answers our Sync: one
        result per CommandComplete / EmptyQueryResponse /
        PortalSuspended, and the error that cut the sequence short."""
        results: List[PgResult] = []
        columns: List[str] = []
        rows: List[Tuple] = []
        error: Optional[PgError] = None
        while True:
            t, payload = await self._recv()
            if t == b"T":
                columns = _row_description(payload)
            elif t == b"n":      # NoData
                columns = []
            elif t == b"D":
                rows.append(_data_row(payload))
            elif t in (b"C", b"I", b"s"):
                command = _cstr(payload, 0)[0] if t == b"C" else ""
                results.append(PgResult(columns, rows, command))
                columns, rows = [], []
            elif t == b"E":
                if error is None:
                    error = PgError(self._err_fields(payload))
            elif t == b"Z":
                self.txn_status = _TXN_STATUS.get(payload, "I")
                return results, error
            # '1' '2' '3' (parse/bind/close complete), 't', notices: skipped

    def transaction(self, timeout_s: float = 30.0) -> "_Transaction":
        """``async with cli.transaction():`` — BEGIN on entry, COMMIT on
        a clean exit, ROLLBACK when the body raises.  The block belongs
        to the connection: while it is open, use the client from one
        task only."""
        return _Transaction(self, timeout_s)

    # ------------------------------------------------------------- framing
    async def _recv(self) -> Tuple[bytes, bytes]:
        hdr = await self._reader.readexactly(5)
        t, ln = _HDR.unpack(hdr)
        payload = await self._reader.readexactly(ln - 4)
        return t, payload

    @staticmethod
    def _err_fields(payload: bytes) -> Dict[str, str]:
        fields = {}
        pos = 0
        while pos < len(payload) and payload[pos:pos + 1] != b"\x00":
            code = payload[pos:pos + 1].decode()
            val, pos = _cstr(payload, pos + 1)
            fields[code] = val
        return fields


class _Transaction:
    def __init__(self, cli: PgClient, timeout_s: float):
        self._cli = cli
        self._timeout_s = timeout_s

    async def __aenter__(self) -> PgClient:
        await self._cli.query("BEGIN", timeout_s=self._timeout_s)
        return self._cli

    async def __aexit__(self, exc_type, exc, tb) -> bool:
        cli = self._cli
        if exc_type is None:
            res = await cli.query("COMMIT", timeout_s=self._timeout_s)
            if res.command != "COMMIT":
                # the block had failed and the body swallowed the error
                raise PgError({"C": "25P02", "M": "transaction was rolled "
                               "back (%s)" % res.command})
            return False
        # a torn-down connection took its block with it
        if cli.connected and cli.txn_status != "I":
            try:
                await cli.query("ROLLBACK", timeout_s=self._timeout_s)
            except Exception:
                pass
        return False
