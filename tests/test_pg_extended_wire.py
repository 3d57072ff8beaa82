"""Extended-query protocol golden vectors for minipg.

The server and ``PgClient`` are a matched pair — a shared framing bug
would be invisible to their round-trip tests.  Here every frontend
message is assembled BYTE BY BYTE from the PostgreSQL protocol
documentation ("Message Formats", protocol 3.0: Parse, Bind, Describe,
Execute, Close, Sync, Flush) with ``struct`` only, sent over a plain
socket, and the backend's answer is compared with bytes assembled the
same way (ParseComplete, BindComplete, CloseComplete,
ParameterDescription, NoData, RowDescription, DataRow, CommandComplete,
EmptyQueryResponse, PortalSuspended, ErrorResponse, ReadyForQuery).
``PgClient`` is never used.
"""

import asyncio
import os
import struct

from tests.minipg_inproc import run, start_minipg, stop_minipg

i16 = lambda v: struct.pack(">h", v)        # noqa: E731
i32 = lambda v: struct.pack(">i", v)        # noqa: E731
cs = lambda s: s.encode("utf-8") + b"\x00"  # noqa: E731


def msg(t: bytes, body: bytes = b"") -> bytes:
    return t + i32(len(body) + 4) + body


# ------------------------------------------------------------- frontend
def parse(name, sql, oids=()):
    return msg(b"P", cs(name) + cs(sql) + i16(len(oids))
               + b"".join(i32(o) for o in oids))


def bind(portal, stmt, params, pfmts=(), rfmts=()):
    body = cs(portal) + cs(stmt)
    body += i16(len(pfmts)) + b"".join(i16(f) for f in pfmts)
    body += i16(len(params))
    for p in params:
        if p is None:
            body += i32(-1)
        else:
            b = p.encode("utf-8")
            body += i32(len(b)) + b
    body += i16(len(rfmts)) + b"".join(i16(f) for f in rfmts)
    return msg(b"B", body)


def describe(kind, name):
    return msg(b"D", kind + cs(name))


def execute(portal, max_rows=0):
    return msg(b"E", cs(portal) + i32(max_rows))


def close(kind, name):
    return msg(b"C", kind + cs(name))


def query(sql):
    return msg(b"Q", cs(sql))


SYNC = msg(b"S")
FLUSH = msg(b"H")
TERMINATE = msg(b"X")

# -------------------------------------------------------------- backend
PARSE_OK = b"1\x00\x00\x00\x04"
BIND_OK = b"2\x00\x00\x00\x04"
CLOSE_OK = b"3\x00\x00\x00\x04"
NO_DATA = b"n\x00\x00\x00\x04"
SUSPENDED = b"s\x00\x00\x00\x04"
EMPTY_QUERY = b"I\x00\x00\x00\x04"


def ready(status: bytes) -> bytes:
    return b"Z\x00\x00\x00\x05" + status


def param_desc(n):
    return msg(b"t", i16(n) + i32(25) * n)      # every parameter is text


def row_desc(*cols):
    body = i16(len(cols))
    for c in cols:
        # name, table oid, attnum, type oid (25 text), typlen, typmod,
        # format (0 text)
        body += cs(c) + i32(0) + i16(0) + i32(25) + i16(-1) + i32(-1) + i16(0)
    return msg(b"T", body)


def data_row(*vals):
    body = i16(len(vals))
    for v in vals:
        if v is None:
            body += i32(-1)
        else:
            b = v.encode("utf-8")
            body += i32(len(b)) + b
    return msg(b"D", body)


def complete(tag):
    return msg(b"C", cs(tag))


def error(code, message):
    return msg(b"E", b"S" + cs("ERROR") + b"C" + cs(code)
               + b"M" + cs(message) + b"\x00")


INSERT = "INSERT INTO kv (k, v) VALUES ($1, $2)"
SELECT = "SELECT v FROM kv WHERE k = $1"
ABORTED = ("current transaction is aborted, commands ignored until end "
           "of transaction block")


class Wire:
    """A raw libpq connection past its startup exchange."""

    def __init__(self, reader, writer):
        self.reader = reader
        self.writer = writer

    @classmethod
    async def open(cls, port):
        reader, writer = await asyncio.open_connection("127.0.0.1", port)
        self = cls(reader, writer)
        body = i32(196608) + cs("user") + cs("postgres") + \
            cs("database") + cs("postgres") + b"\x00"
        writer.write(i32(len(body) + 4) + body)
        want = msg(b"R", i32(0))
        for k, v in (("server_version", "12.0 (minipg)"),
                     ("client_encoding", "UTF8"),
                     ("server_encoding", "UTF8"),
                     ("integer_datetimes", "on")):
            want += msg(b"S", cs(k) + cs(v))
        # the server runs in this process
        want += msg(b"K", i32(os.getpid()) + i32(0)) + ready(b"I")
        assert await self.recv(b"Z") == want
        return self

    async def recv(self, last: bytes) -> bytes:
        """Whole messages up to and including the first of type
        ``last``."""
        out = b""
        while True:
            hdr = await self.reader.readexactly(5)
            (ln,) = struct.unpack(">I", hdr[1:])
            out += hdr + await self.reader.readexactly(ln - 4)
            if hdr[:1] == last:
                return out

    async def roundtrip(self, sent: bytes, last: bytes = b"Z") -> bytes:
        self.writer.write(sent)
        await self.writer.drain()
        return await self.recv(last)

    async def finish(self) -> None:
        """Nothing stray may be pending: a bare Sync is answered by
        exactly one ReadyForQuery, and after Terminate the server sends
        nothing more."""
        assert await self.roundtrip(SYNC) in (ready(b"I"), ready(b"T"),
                                              ready(b"E"))
        self.writer.write(TERMINATE)
        await self.writer.drain()
        assert await self.reader.read() == b""
        self.writer.close()


def wire_test(scenario, tmp_path):
    async def go():
        srv, port = await start_minipg(str(tmp_path / "pg"))
        try:
            w = await Wire.open(port)
            await scenario(srv, w)
            await w.finish()
        finally:
            stop_minipg(srv)
    run(go())


def test_parameterised_insert_and_select(tmp_path):
    async def scenario(srv, w):
        got = await w.roundtrip(
            parse("", INSERT, oids=(25, 25)) + bind("", "", ["k1", "it's"])
            + describe(b"P", "") + execute("") + SYNC)
        assert got == (PARSE_OK + BIND_OK + NO_DATA
                       + complete("INSERT 0 1") + ready(b"I"))
        assert srv.kv == {"k1": "it's"}

        got = await w.roundtrip(
            parse("", SELECT) + bind("", "", ["k1"]) + describe(b"P", "")
            + execute("") + SYNC)
        assert got == (PARSE_OK + BIND_OK + row_desc("v")
                       + data_row("it's") + complete("SELECT 1")
                       + ready(b"I"))

        # a key that is not there; explicit all-text format codes
        got = await w.roundtrip(
            parse("", SELECT) + bind("", "", ["nope"], pfmts=(0,),
                                     rfmts=(0,))
            + describe(b"P", "") + execute("") + SYNC)
        assert got == (PARSE_OK + BIND_OK + row_desc("v")
                       + complete("SELECT 0") + ready(b"I"))

        # the empty statement, and Flush: output without ReadyForQuery
        got = await w.roundtrip(
            parse("", "") + bind("", "", []) + execute("") + FLUSH,
            last=b"I")
        assert got == PARSE_OK + BIND_OK + EMPTY_QUERY
        assert await w.roundtrip(SYNC) == ready(b"I")
    wire_test(scenario, tmp_path)


def test_describe_statement_does_not_execute(tmp_path):
    async def scenario(srv, w):
        got = await w.roundtrip(
            parse("sel", SELECT) + describe(b"S", "sel") + SYNC)
        assert got == (PARSE_OK + param_desc(1) + row_desc("v")
                       + ready(b"I"))
        got = await w.roundtrip(
            parse("ins", INSERT) + describe(b"S", "ins") + SYNC)
        assert got == PARSE_OK + param_desc(2) + NO_DATA + ready(b"I")
        for sql in ("BEGIN", "COMMIT", "ROLLBACK",
                    "UPDATE kv SET v = $1 WHERE k = $2",
                    "DELETE FROM kv WHERE k = $1",
                    "CREATE TABLE IF NOT EXISTS kv (k text, v text)"):
            n = sql.count("$")
            got = await w.roundtrip(
                parse("", sql) + describe(b"S", "") + SYNC)
            assert got == (PARSE_OK + param_desc(n) + NO_DATA
                           + ready(b"I")), sql
        # a portal bound to the INSERT is described, never run
        end = srv.wal.end
        got = await w.roundtrip(
            bind("p", "ins", ["a", "b"]) + describe(b"P", "p") + SYNC)
        assert got == BIND_OK + NO_DATA + ready(b"I")
        assert srv.kv == {} and srv.wal.end == end
        # the count's column is what Execute's row will carry
        got = await w.roundtrip(
            parse("", "SELECT count(*) AS n FROM kv") + bind("", "", [])
            + describe(b"P", "") + execute("") + SYNC)
        assert got == (PARSE_OK + BIND_OK + row_desc("count")
                       + data_row("0") + complete("SELECT 1")
                       + ready(b"I"))
        # Close of a statement and of a portal, present or not
        got = await w.roundtrip(
            close(b"S", "sel") + close(b"P", "never") + SYNC)
        assert got == CLOSE_OK + CLOSE_OK + ready(b"I")
        got = await w.roundtrip(describe(b"S", "sel") + SYNC)
        assert got == error(
            "26000", 'prepared statement "sel" does not exist') \
            + ready(b"I")
    wire_test(scenario, tmp_path)


def test_execute_row_limit_suspends_the_portal(tmp_path):
    async def scenario(srv, w):
        from manatee_amd.db.waldb.core import ReplicaConn
        # two pg_stat_replication rows without two standbys
        srv.replicas.extend([ReplicaConn("s1", None),
                             ReplicaConn("s2", None)])
        cols = ["pid", "application_name", "client_addr", "state",
                "sent_lsn", "write_lsn", "flush_lsn", "replay_lsn",
                "sync_state"]
        zero = "0/00000000"
        rows = [data_row(str(os.getpid()), name, None, "streaming",
                         zero, zero, zero, zero, "async")
                for name in ("s1", "s2")]
        # portals live until the end of the transaction: hold one open
        got = await w.roundtrip(query("BEGIN"))
        assert got == complete("BEGIN") + ready(b"T")
        got = await w.roundtrip(
            parse("", "SELECT * FROM pg_stat_replication")
            + bind("cur", "", []) + describe(b"P", "cur")
            + execute("cur", 1) + SYNC)
        assert got == (PARSE_OK + BIND_OK + row_desc(*cols) + rows[0]
                       + SUSPENDED + ready(b"T"))
        # the remainder; Execute never repeats the RowDescription
        got = await w.roundtrip(execute("cur", 1) + SYNC)
        assert got == rows[1] + complete("SELECT 1") + ready(b"T")
        got = await w.roundtrip(execute("cur", 1) + SYNC)
        assert got == complete("SELECT 0") + ready(b"T")
        # the limit above what is left, and no limit
        got = await w.roundtrip(
            bind("c2", "", []) + execute("c2", 5) + bind("c3", "", [])
            + execute("c3", 0) + SYNC)
        assert got == (BIND_OK + rows[0] + rows[1] + complete("SELECT 2")
                       + BIND_OK + rows[0] + rows[1]
                       + complete("SELECT 2") + ready(b"T"))
        got = await w.roundtrip(query("COMMIT"))
        assert got == complete("COMMIT") + ready(b"I")
        # the transaction's end dropped the portal
        got = await w.roundtrip(execute("cur", 1) + SYNC)
        assert got == error("34000", 'portal "cur" does not exist') \
            + ready(b"I")
        del srv.replicas[:]
    wire_test(scenario, tmp_path)


def test_error_skips_to_sync(tmp_path):
    async def scenario(srv, w):
        got = await w.roundtrip(
            parse("", INSERT) + bind("", "", ["e1", "1"]) + execute("")
            + parse("", "FROB") + bind("", "", []) + execute("")
            + parse("", INSERT) + bind("", "", ["e2", "2"]) + execute("")
            + SYNC)
        assert got == (PARSE_OK + BIND_OK + complete("INSERT 0 1")
                       + error("42601", 'syntax error at or near "FROB"')
                       + ready(b"I"))
        assert srv.kv == {"e1": "1"}
        # outside a block every Sync drops the portals
        got = await w.roundtrip(execute("") + SYNC)
        assert got == error("34000", 'portal "" does not exist') \
            + ready(b"I")
        # Flush after an error does not end the skipping; Sync does
        got = await w.roundtrip(
            parse("", "FROB") + FLUSH + parse("", SELECT) + SYNC)
        assert got == error("42601", 'syntax error at or near "FROB"') \
            + ready(b"I")
        got = await w.roundtrip(parse("", SELECT) + SYNC)
        assert got == PARSE_OK + ready(b"I")
    wire_test(scenario, tmp_path)


def test_ready_for_query_transaction_status(tmp_path):
    async def scenario(srv, w):
        got = await w.roundtrip(
            parse("", "BEGIN") + bind("", "", []) + execute("") + SYNC)
        assert got == (PARSE_OK + BIND_OK + complete("BEGIN")
                       + ready(b"T"))
        got = await w.roundtrip(
            parse("", INSERT) + bind("", "", ["t1", "1"]) + execute("")
            + SYNC)
        assert got == (PARSE_OK + BIND_OK + complete("INSERT 0 1")
                       + ready(b"T"))
        got = await w.roundtrip(parse("", "FROB") + SYNC)
        assert got == error("42601", 'syntax error at or near "FROB"') \
            + ready(b"E")
        got = await w.roundtrip(
            parse("", SELECT) + bind("", "", ["t1"]) + execute("") + SYNC)
        assert got == error("25P02", ABORTED) + ready(b"E")
        got = await w.roundtrip(query("SELECT v FROM kv WHERE k = 't1'"))
        assert got == error("25P02", ABORTED) + ready(b"E")
        got = await w.roundtrip(
            parse("", "ROLLBACK") + bind("", "", []) + execute("") + SYNC)
        assert got == (PARSE_OK + BIND_OK + complete("ROLLBACK")
                       + ready(b"I"))
        assert srv.kv == {}
        # COMMIT of a failed block answers ROLLBACK
        got = await w.roundtrip(query("BEGIN; FROB"))
        assert got == (complete("BEGIN")
                       + error("42601", 'syntax error at or near "FROB"')
                       + ready(b"E"))
        got = await w.roundtrip(query("COMMIT"))
        assert got == complete("ROLLBACK") + ready(b"I")
    wire_test(scenario, tmp_path)


def test_bind_errors(tmp_path):
    async def scenario(srv, w):
        unsupported = error("0A000", "binary parameter and result formats "
                            "are not supported")
        got = await w.roundtrip(
            parse("", INSERT) + bind("", "", ["b1", "1"], pfmts=(1,))
            + execute("") + SYNC)
        assert got == PARSE_OK + unsupported + ready(b"I")
        got = await w.roundtrip(
            parse("", SELECT) + bind("", "", ["b1"], rfmts=(1,))
            + execute("") + SYNC)
        assert got == PARSE_OK + unsupported + ready(b"I")
        got = await w.roundtrip(
            parse("", SELECT) + bind("", "", ["b1"], pfmts=(0, 1))
            + execute("") + SYNC)
        assert got == PARSE_OK + unsupported + ready(b"I")

        got = await w.roundtrip(bind("", "nosuch", []) + execute("") + SYNC)
        assert got == error(
            "26000", 'prepared statement "nosuch" does not exist') \
            + ready(b"I")
        got = await w.roundtrip(describe(b"P", "nosuch") + SYNC)
        assert got == error("34000", 'portal "nosuch" does not exist') \
            + ready(b"I")

        got = await w.roundtrip(
            parse("", INSERT) + bind("", "", ["only-one"]) + execute("")
            + SYNC)
        assert got == PARSE_OK + error(
            "08P01", 'bind message supplies 1 parameters, but prepared '
            'statement "" requires 2') + ready(b"I")

        # NULL where the statement cannot take one: the SQL layer's error
        got = await w.roundtrip(
            parse("", INSERT) + bind("", "", ["k", None]) + execute("")
            + SYNC)
        assert got == PARSE_OK + error(
            "42601", 'syntax error at or near "INSERT"') + ready(b"I")
        assert srv.kv == {}
    wire_test(scenario, tmp_path)


def test_named_statements(tmp_path):
    async def scenario(srv, w):
        got = await w.roundtrip(parse("dup", INSERT) + SYNC)
        assert got == PARSE_OK + ready(b"I")
        got = await w.roundtrip(parse("dup", SELECT) + SYNC)
        assert got == error(
            "42P05", 'prepared statement "dup" already exists') \
            + ready(b"I")
        # the unnamed statement is simply replaced
        got = await w.roundtrip(
            parse("", INSERT) + parse("", SELECT) + bind("", "", ["x"])
            + execute("") + SYNC)
        assert got == (PARSE_OK + PARSE_OK + BIND_OK
                       + complete("SELECT 0") + ready(b"I"))
        # a named statement outlives Sync and is bound again and again
        got = await w.roundtrip(
            bind("", "dup", ["n1", "1"]) + execute("")
            + bind("", "dup", ["n2", "$1;'\n"]) + execute("") + SYNC)
        assert got == (BIND_OK + complete("INSERT 0 1")
                       + BIND_OK + complete("INSERT 0 1") + ready(b"I"))
        assert srv.kv == {"n1": "1", "n2": "$1;'\n"}
        got = await w.roundtrip(
            parse("", "SELECT 1; SELECT 2") + SYNC)
        assert got == error(
            "42601", "cannot insert multiple commands into a prepared "
            "statement") + ready(b"I")
    wire_test(scenario, tmp_path)
