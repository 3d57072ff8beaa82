"""Golden wire transcripts for the two database front-ends.

One fixed script is played against an in-process primary (no sync
standby) through each client protocol and the answers are compared with
committed recordings:

- the JSON line protocol of ``WaldbServer`` as RAW response bytes
  (``tests/golden/waldb_transcript.out``) — only ``pid``, ``ident``,
  ``uptime_s`` and ``last_replay_time`` of ``status`` and ``ts`` of
  ``ping`` are masked; LSNs are not, they pin the WAL framing;
- the libpq front-end of ``MinipgServer`` through ``PgClient`` as
  ``(columns, rows, command tag, error code)`` per statement, for
  PG_VERSION 12 and 9.6, plus one JSON line on the same port
  (``tests/golden/minipg_transcript.json``).

The recordings pin behaviour across refactors of the servers.
Regenerate after an intentional protocol change with:
    REGEN_GOLDEN=1 python -m pytest tests/test_waldb_transcript.py -q
"""

import asyncio
import json
import os
import re

import pytest

from manatee_amd.common import confparser
from manatee_amd.common.logging import null_logger
from manatee_amd.db.pgwire import PgClient, PgError

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          "golden")
WALDB_GOLDEN = os.path.join(GOLDEN_DIR, "waldb_transcript.out")
MINIPG_GOLDEN = os.path.join(GOLDEN_DIR, "minipg_transcript.json")
REGEN = bool(os.environ.get("REGEN_GOLDEN"))


def run(coro, timeout=30):
    return asyncio.run(asyncio.wait_for(coro, timeout))


def _stop(srv) -> None:
    if srv._server is not None:
        srv._server.close()
    if srv._flusher is not None:
        srv._flusher.cancel()
    srv.wal.close()


def _listen_port(data: str, pid_file: str) -> int:
    with open(os.path.join(data, pid_file)) as f:
        return int(f.read().split()[1])


# ------------------------------------------------------------------ waldb

# every line newline-terminated; answered strictly in order
WALDB_SCRIPT = [
    b'{"q":"ping"}',
    b'{"q":"put","k":"a","v":{"x":[1,2],"s":"\\u00e9"}}',
    b'{"q":"get","k":"a"}',
    b'{"q":"del","k":"a"}',
    b'{"q":"get","k":"a"}',
    b'{"q":"del","k":"never-there"}',
    b'{"q":"batch","ops":[{"op":"put","k":"p1","v":1},'
    b'{"op":"put","k":"p2","v":"two"},{"op":"put","k":"p3","v":null},'
    b'{"op":"put","k":"q1","v":[]},{"op":"del","k":"p3"}]}',
    b'{"q":"batch","ops":[]}',
    b'{"q":"batch"}',
    b'{"q":"batch","ops":[{"op":"put","k":"z1","v":1},{"op":"frob","k":"z2"}]}',
    b'{"q":"batch","ops":[{"op":"put","v":1}]}',
    b'{"q":"put","k":"p4","v":4}',
    b'{"q":"put","k":"p5","v":5}',
    b'{"q":"scan","prefix":"p","after":"p1","limit":2}',
    b'{"q":"scan","prefix":"p","after":"p2"}',
    b'{"q":"scan"}',
    b'{"q":"count"}',
    b'{"q":"count","prefix":"p"}',
    b'{"q":"count","prefix":"nope"}',
    b'{"q":"xlog"}',
    b'{nope',
    b'{"q":"frob"}',
    b'{"k":"no-q"}',
    b'{"q":"status"}',
]
# sent WITHOUT a newline, followed by EOF
WALDB_FINAL = b'{"q":"put","k":"eof","v":"unterminated"}'
# a second connection observes what the unterminated line did
WALDB_AFTER = [
    b'{"q":"get","k":"eof"}',
    b'{"q":"count"}',
    b'{"q":"xlog"}',
]

_MASKS = [
    (re.compile(rb'"pid":\d+'), b'"pid":0'),
    (re.compile(rb'"ident":"[0-9a-f]+"'), b'"ident":"X"'),
    (re.compile(rb'"uptime_s":[0-9.e+-]+'), b'"uptime_s":0'),
    (re.compile(rb'"last_replay_time":[0-9.e+-]+'),
     b'"last_replay_time":0'),
    (re.compile(rb'"ts":[0-9.e+-]+'), b'"ts":0'),
]


def _mask(raw: bytes) -> bytes:
    for rx, repl in _MASKS:
        raw = rx.sub(repl, raw)
    return raw


async def _read_lines(reader, n: int) -> bytes:
    out = b""
    for _ in range(n):
        line = await reader.readline()
        assert line.endswith(b"\n"), "connection closed early: %r" % out
        out += line
    return out


async def _waldb_transcript(tmp_path) -> bytes:
    from manatee_amd.db.waldb.server import WaldbServer, init_data_dir

    data = str(tmp_path / "db")
    init_data_dir(data)
    confparser.write(os.path.join(data, "waldb.conf"), {
        "role": "primary", "listen_ip": "127.0.0.1", "port": "0",
        "name": "n1"})
    srv = WaldbServer(data, null_logger())
    await srv.start()
    try:
        port = _listen_port(data, "waldb.pid")
        reader, writer = await asyncio.open_connection("127.0.0.1", port)
        # the whole script in ONE write: pipelined
        writer.write(b"".join(line + b"\n" for line in WALDB_SCRIPT))
        await writer.drain()
        raw = await _read_lines(reader, len(WALDB_SCRIPT))
        writer.write(WALDB_FINAL)
        writer.write_eof()
        raw += b"--- unterminated final line, then EOF\n"
        raw += await reader.read()
        writer.close()
        raw += b"--- second connection\n"
        reader, writer = await asyncio.open_connection("127.0.0.1", port)
        writer.write(b"".join(line + b"\n" for line in WALDB_AFTER))
        await writer.drain()
        raw += await _read_lines(reader, len(WALDB_AFTER))
        writer.close()
        return _mask(raw)
    finally:
        _stop(srv)


def test_waldb_json_transcript(tmp_path):
    got = run(_waldb_transcript(tmp_path))
    if REGEN:
        with open(WALDB_GOLDEN, "wb") as f:
            f.write(got)
    with open(WALDB_GOLDEN, "rb") as f:
        want = f.read()
    assert got == want


# ----------------------------------------------------------------- minipg

def _pg_statements(w: str):
    """The statement list; ``w`` is the LSN word of the PG major
    (``lsn`` from 10 on, ``location`` before)."""
    cur = ("pg_current_wal_lsn()" if w == "lsn"
           else "pg_current_xlog_location()")
    return [
        "CREATE TABLE IF NOT EXISTS kv (k text primary key, v text);",
        "INSERT INTO kv (k, v) VALUES ('a', 'one');",
        "INSERT INTO kv (k, v) VALUES ('it''s', 'quo''ted');",
        "SELECT v FROM kv WHERE k = 'a';",
        "SELECT v FROM kv WHERE k = 'it''s';",
        "SELECT v FROM kv WHERE k = 'missing';",
        "DELETE FROM kv WHERE k = 'a';",
        "DELETE FROM kv WHERE k = 'a';",
        "INSERT INTO kv (k, v) VALUES ('p1', '1'); "
        "INSERT INTO kv (k, v) VALUES ('p2', '2'); "
        "INSERT INTO kv (k, v) VALUES ('q1', '3');",
        "SELECT count(*) FROM kv WHERE k LIKE 'p%';",
        "SELECT count(*) AS n FROM kv;",
        "SELECT pg_is_in_recovery() as r;",
        "SELECT %s as loc;" % cur,
        "SELECT * FROM pg_stat_replication;",
        "SELECT * FROM pg_stat_wal_receiver;",
        "SELECT pg_last_%s_replay_%s() as loc;"
        % ("wal" if w == "lsn" else "xlog", w),
        # an error in the middle aborts the rest of the cycle
        "INSERT INTO kv (k, v) VALUES ('m1', '1'); FROB; "
        "INSERT INTO kv (k, v) VALUES ('m2', '2');",
        "SELECT count(*) FROM kv WHERE k LIKE 'm%';",
        "SELEKT 1;",
        "",
        "SELECT %s as loc;" % cur,
    ]


async def _minipg_transcript(tmp_path, version: str) -> dict:
    from manatee_amd.db.minipg.server import MinipgServer, init_data_dir

    data = str(tmp_path / ("pg" + version))
    init_data_dir(data, version)
    confparser.write(os.path.join(data, "postgresql.conf"), {
        "listen_addresses": "'127.0.0.1'", "port": "0"})
    srv = MinipgServer(data, null_logger())
    await srv.start()
    try:
        port = _listen_port(data, "postmaster.pid")
        cli = PgClient("127.0.0.1", port, "postgres")
        await cli.connect()
        sql = []
        for stmt in _pg_statements(srv.lsn_word):
            try:
                r = await cli.query(stmt)
                sql.append([stmt, r.columns, [list(row) for row in r.rows],
                            r.command, None])
            except PgError as exc:
                sql.append([stmt, None, None, None, exc.code])
        await cli.close()
        # first-byte multiplexing: a JSON line on the libpq port
        reader, writer = await asyncio.open_connection("127.0.0.1", port)
        writer.write(b'{"q":"xlog"}\n')
        await writer.drain()
        line = await reader.readline()
        writer.close()
        return {"pg_major": srv.pg_major, "sql": sql,
                "json_xlog": line.decode()}
    finally:
        _stop(srv)


@pytest.mark.parametrize("version", ["12.0", "9.6.3"])
def test_minipg_libpq_transcript(tmp_path, version):
    got = run(_minipg_transcript(tmp_path, version))
    golden = {}
    if os.path.exists(MINIPG_GOLDEN):
        with open(MINIPG_GOLDEN) as f:
            golden = json.load(f)
    if REGEN:
        golden[version] = got
        with open(MINIPG_GOLDEN, "w") as f:
            json.dump(golden, f, indent=1, sort_keys=True)
            f.write("\n")
    assert got == golden[version]
    w = "lsn" if version == "12.0" else "location"
    cols = [row[1] for row in got["sql"]
            if "pg_stat_replication" in row[0]][0]
    assert "sent_" + w in cols and "replay_" + w in cols
