"""Transaction blocks and bound parameters on minipg, through
``PgClient`` and ``PgKvClient`` against an in-process server (no
cluster): quoting, read-your-writes, isolation from other connections,
one WAL record per COMMIT, rollback, failed blocks, read-only, the
buffer cap, UPDATE, pipelines, and all-or-nothing recovery after a
crash inside the COMMIT record.
"""

import os

import pytest

from manatee_amd.db.pgkv import PgKvClient, PgKvError
from manatee_amd.db.pgwire import PgClient, PgError
from manatee_amd.db.waldb.wal import decode_op, encode_op
from tests.minipg_inproc import run, start_minipg, stop_minipg

INSERT = "INSERT INTO kv (k, v) VALUES ($1, $2)"
SELECT = "SELECT v FROM kv WHERE k = $1"
UPDATE = "UPDATE kv SET v = $1 WHERE k = $2"

AWKWARD = ["it's", "a;b", "$1", "$2 and '$1'", "line\nbreak", "", "''",
           "';DELETE FROM kv WHERE k = 'x", "pg_is_in_recovery",
           "current_time", "DELETE FROM kv WHERE k = ''x''", "é☃"]


def with_server(scenario, tmp_path, conf=None):
    async def go():
        srv, port = await start_minipg(str(tmp_path / "pg"), conf)
        clients = []

        async def connect():
            cli = PgClient("127.0.0.1", port, "postgres")
            await cli.connect()
            clients.append(cli)
            return cli
        try:
            await scenario(srv, port, connect)
        finally:
            for cli in clients:
                await cli.close()
            stop_minipg(srv)
    run(go())


def test_parameter_quoting_round_trip(tmp_path):
    async def scenario(srv, port, connect):
        cli = await connect()
        # every awkward string as a key AND as a value, outside a block
        for i, s in enumerate(AWKWARD):
            r = await cli.query_params(INSERT, [s, AWKWARD[-1 - i]])
            assert r.command == "INSERT 0 1"
        assert srv.kv == {s: AWKWARD[-1 - i]
                          for i, s in enumerate(AWKWARD)}
        for i, s in enumerate(AWKWARD):
            r = await cli.query_params(SELECT, [s])
            assert r.columns == ["v"] and r.rows == [(AWKWARD[-1 - i],)], s
        # ... and inside one, through the key/value client
        kv = PgKvClient("127.0.0.1", port)
        try:
            async with kv.transaction() as tx:
                for s in AWKWARD:
                    await tx.put("tx:" + s, {"s": s})
                for s in AWKWARD:
                    assert await tx.get("tx:" + s) == {"s": s}
            for s in AWKWARD:
                assert await kv.get("tx:" + s) == {"s": s}
            assert await kv.count() == 2 * len(AWKWARD)
            async with kv.transaction() as tx:
                for s in AWKWARD:
                    assert await tx.delete("tx:" + s) == "DELETE 1"
            assert await kv.count() == len(AWKWARD)
        finally:
            await kv.close()
        # NULL where a literal is required is the SQL layer's error
        with pytest.raises(PgError) as ei:
            await cli.query_params(INSERT, ["k", None])
        assert ei.value.code == "42601"
        assert "k" not in srv.kv
    with_server(scenario, tmp_path)


def test_read_your_writes_and_isolation(tmp_path):
    async def scenario(srv, port, connect):
        a, b = await connect(), await connect()
        await a.query_params(INSERT, ["p-old", "0"])
        await a.query_params(INSERT, ["q-old", "0"])
        start = srv.wal.end

        async def counts(cli):
            return (int((await cli.query(
                        "SELECT count(*) FROM kv")).rows[0][0]),
                    int((await cli.query_params(
                        "SELECT count(*) FROM kv WHERE k LIKE $1",
                        ["p-%"])).rows[0][0]),
                    int((await cli.query(
                        "SELECT count(*) AS n FROM kv WHERE k LIKE 'q-%'"
                    )).rows[0][0]))

        async with a.transaction():
            assert a.txn_status == "T"
            await a.query_params(INSERT, ["p-new", "1"])
            await a.query("INSERT INTO kv (k, v) VALUES ('q-new', '1')")
            await a.query_params(UPDATE, ["2", "p-old"])
            assert (await a.query_params(
                "DELETE FROM kv WHERE k = $1", ["q-old"])).command \
                == "DELETE 1"
            # deleting what this block already deleted finds nothing
            assert (await a.query_params(
                "DELETE FROM kv WHERE k = $1", ["q-old"])).command \
                == "DELETE 0"
            # the block reads its own writes ...
            assert (await a.query_params(SELECT, ["p-new"])).rows == [("1",)]
            assert (await a.query_params(SELECT, ["p-old"])).rows == [("2",)]
            assert (await a.query_params(SELECT, ["q-old"])).rows == []
            assert await counts(a) == (3, 2, 1)
            # ... nobody else does, and nothing is in the WAL yet
            assert (await b.query_params(SELECT, ["p-new"])).rows == []
            assert (await b.query_params(SELECT, ["p-old"])).rows == [("0",)]
            assert (await b.query_params(SELECT, ["q-old"])).rows == [("0",)]
            assert await counts(b) == (2, 1, 1)
            assert srv.wal.end == start
            assert srv.kv == {"p-old": "0", "q-old": "0"}
        assert a.txn_status == "I"
        # COMMIT: everything visible, as exactly ONE WAL record
        assert await counts(b) == (3, 2, 1)
        assert (await b.query_params(SELECT, ["p-old"])).rows == [("2",)]
        records = list(srv.wal.iter_records(start))
        assert len(records) == 1 and records[0][0] == srv.wal.end
        assert decode_op(records[0][1]) == {"op": "batch", "ops": [
            {"op": "put", "k": "p-new", "v": "1"},
            {"op": "put", "k": "q-new", "v": "1"},
            {"op": "put", "k": "p-old", "v": "2"},
            {"op": "del", "k": "q-old"}]}
        # an empty block writes nothing
        end = srv.wal.end
        async with a.transaction():
            assert (await a.query_params(SELECT, ["p-new"])).rows == [("1",)]
        assert srv.wal.end == end
        # BEGIN inside a block, COMMIT/ROLLBACK outside one: no-ops
        assert (await a.query("COMMIT")).command == "COMMIT"
        assert (await a.query("ROLLBACK")).command == "ROLLBACK"
        assert (await a.query("START TRANSACTION")).command == "BEGIN"
        assert (await a.query("BEGIN")).command == "BEGIN"
        assert a.txn_status == "T"
        assert (await a.query("END")).command == "COMMIT"
        assert a.txn_status == "I" and srv.wal.end == end
    with_server(scenario, tmp_path)


def test_rollback_and_dropped_connection_leave_no_trace(tmp_path):
    async def scenario(srv, port, connect):
        a, b = await connect(), await connect()
        await a.query_params(INSERT, ["keep", "0"])
        end = srv.wal.end
        before = dict(srv.kv)

        with pytest.raises(ZeroDivisionError):
            async with a.transaction():
                await a.query_params(INSERT, ["gone1", "1"])
                await a.query_params("DELETE FROM kv WHERE k = $1", ["keep"])
                1 / 0
        assert a.txn_status == "I"
        await a.query("BEGIN")
        await a.query_params(UPDATE, ["9", "keep"])
        assert (await a.query("ABORT")).command == "ROLLBACK"
        assert srv.wal.end == end and srv.kv == before

        # a connection that vanishes mid-block
        await b.query("BEGIN")
        await b.query_params(INSERT, ["gone2", "2"])
        await b.query_params(UPDATE, ["9", "keep"])
        b._writer.transport.abort()
        await b.close()
        assert (await a.query_params(SELECT, ["gone2"])).rows == []
        assert (await a.query_params(SELECT, ["keep"])).rows == [("0",)]
        assert srv.wal.end == end and srv.kv == before
    with_server(scenario, tmp_path)


def test_failed_block(tmp_path):
    async def scenario(srv, port, connect):
        cli = await connect()
        end = srv.wal.end
        await cli.query("BEGIN")
        await cli.query_params(INSERT, ["f1", "1"])
        with pytest.raises(PgError) as ei:
            await cli.query("FROB")
        assert ei.value.code == "42601" and cli.txn_status == "E"
        for attempt in (cli.query("SELECT v FROM kv WHERE k = 'f1'"),
                        cli.query_params(INSERT, ["f2", "2"]),
                        cli.query("SELECT count(*) FROM kv"),
                        cli.query("BEGIN")):
            with pytest.raises(PgError) as ei:
                await attempt
            assert ei.value.code == "25P02" and cli.txn_status == "E"
        r = await cli.query("COMMIT")
        assert r.command == "ROLLBACK" and cli.txn_status == "I"
        assert srv.kv == {} and srv.wal.end == end

        # the context manager turns that answer into an error
        with pytest.raises(PgError) as ei:
            async with cli.transaction():
                await cli.query_params(INSERT, ["f3", "3"])
                with pytest.raises(PgError):
                    await cli.query_params("SELEKT $1", ["x"])
        assert ei.value.code == "25P02" and cli.txn_status == "I"
        assert srv.kv == {} and srv.wal.end == end
        # savepoints are out of scope, and say so
        with pytest.raises(PgError) as ei:
            await cli.query("SAVEPOINT a")
        assert ei.value.code == "42601"
        with pytest.raises(PgError) as ei:
            await cli.query("ROLLBACK TO SAVEPOINT a")
        assert ei.value.code == "0A000"
    with_server(scenario, tmp_path)


def test_write_in_block_on_read_only_server(tmp_path):
    async def scenario(srv, port, connect):
        cli = await connect()
        assert (await cli.query("BEGIN")).command == "BEGIN"
        assert (await cli.query_params(SELECT, ["x"])).rows == []
        # the statement fails, not only the COMMIT
        with pytest.raises(PgError) as ei:
            await cli.query_params(INSERT, ["x", "1"])
        assert ei.value.code == "25006" and cli.txn_status == "E"
        assert (await cli.query("COMMIT")).command == "ROLLBACK"
        await cli.query("BEGIN")
        with pytest.raises(PgError) as ei:
            await cli.query("INSERT INTO kv (k, v) VALUES ('x', '1')")
        assert ei.value.code == "25006" and cli.txn_status == "E"
        await cli.query("ROLLBACK")
        # a statement that finds nothing to write is not a write
        async with cli.transaction():
            r = await cli.query("UPDATE kv SET v = '1' WHERE k = 'x'")
            assert r.command == "UPDATE 0"
            r = await cli.query("DELETE FROM kv WHERE k = 'x'")
            assert r.command == "DELETE 0"
        assert srv.kv == {} and srv.wal.end == 0
    with_server(scenario, tmp_path,
                conf={"default_transaction_read_only": "on"})


def test_transaction_buffer_cap(tmp_path):
    async def scenario(srv, port, connect):
        from manatee_amd.db.minipg.server import MAX_MSG
        assert MAX_MSG == 16 * 1024 * 1024
        cli = await connect()
        # the cap counts ENCODED ops; a character outside the BMP takes
        # 12 bytes there (two \uXXXX escapes), which keeps the strings
        # that have to cross the wire and the SQL layer short
        big = "\U0001F418" * (MAX_MSG // 24 + 64)
        assert len(encode_op({"op": "put", "k": "big1", "v": big})) \
            < MAX_MSG < 2 * len(encode_op({"op": "put", "k": "", "v": big}))
        await cli.query("BEGIN")
        await cli.query_params(INSERT, ["big1", big])
        assert (await cli.query_params(SELECT, ["big1"])).rows == [(big,)]
        with pytest.raises(PgError) as ei:
            await cli.query_params(INSERT, ["big2", big])
        assert ei.value.code == "54000" and cli.txn_status == "E"
        assert (await cli.query("COMMIT")).command == "ROLLBACK"
        assert srv.kv == {} and srv.wal.end == 0
    with_server(scenario, tmp_path)


def test_update(tmp_path):
    async def scenario(srv, port, connect):
        cli = await connect()
        await cli.query_params(INSERT, ["u", "1"])
        r = await cli.query("UPDATE kv SET v = 'two' WHERE k = 'u'")
        assert r.command == "UPDATE 1" and srv.kv["u"] == "two"
        end = srv.wal.end
        r = await cli.query("UPDATE kv SET v = 'x' WHERE k = 'absent'")
        assert r.command == "UPDATE 0"
        r = await cli.query_params(UPDATE, ["x", "absent"])
        assert r.command == "UPDATE 0"
        assert srv.wal.end == end and "absent" not in srv.kv
        r = await cli.query_params(UPDATE, ["it's $2", "u"])
        assert r.command == "UPDATE 1" and r.columns == []
        assert srv.kv == {"u": "it's $2"}
        await cli.prepare("upd", UPDATE)
        r = await cli.execute_prepared("upd", ["3", "u"])
        assert r.command == "UPDATE 1" and srv.kv == {"u": "3"}
        # inside a block it sees the block's own insert
        async with cli.transaction():
            assert (await cli.execute_prepared(
                "upd", ["1", "fresh"])).command == "UPDATE 0"
            await cli.query_params(INSERT, ["fresh", "0"])
            assert (await cli.execute_prepared(
                "upd", ["1", "fresh"])).command == "UPDATE 1"
        assert srv.kv == {"u": "3", "fresh": "1"}
    with_server(scenario, tmp_path)


def test_pipeline(tmp_path):
    async def scenario(srv, port, connect):
        cli = await connect()
        await cli.prepare("ins", INSERT)
        await cli.prepare("sel", SELECT)
        with pytest.raises(PgError) as ei:
            await cli.prepare("ins", SELECT)
        assert ei.value.code == "42P05"
        res = await cli.pipeline(
            [("ins", ("a", "1")), ("sel", ("a",)), (SELECT, ("zz",)),
             ("ins", ("b", "2")), ("SELECT count(*) FROM kv", ()),
             ("sel", ("b",)), ("", ())])
        assert [(r.columns, r.rows, r.command) for r in res] == [
            ([], [], "INSERT 0 1"), (["v"], [("1",)], "SELECT 1"),
            (["v"], [], "SELECT 0"), ([], [], "INSERT 0 1"),
            (["count"], [("2",)], "SELECT 1"),
            (["v"], [("2",)], "SELECT 1"), ([], [], "")]
        assert await cli.pipeline([]) == []

        # an entry that fails: the ones after it never run
        end = srv.wal.end
        with pytest.raises(PgError) as ei:
            await cli.pipeline(
                [("ins", ("c", "3")), ("sel", ("c",)), ("FROB", ()),
                 ("ins", ("d", "4")), ("sel", ("d",))])
        assert ei.value.code == "42601"
        assert ei.value.pipeline_index == 2
        assert [r.command for r in ei.value.pipeline_results] == \
            ["INSERT 0 1", "SELECT 1"]
        assert srv.kv == {"a": "1", "b": "2", "c": "3"}
        assert cli.txn_status == "I" and cli.connected
        assert len(list(srv.wal.iter_records(end))) == 1

        # the key/value client's atomic batch is one record, or nothing
        kv = PgKvClient("127.0.0.1", port)
        try:
            end = srv.wal.end
            items = [("m%d" % i, {"i": i, "s": "it's"}) for i in range(20)]
            assert await kv.put_many_atomic(items) == 20
            assert len(list(srv.wal.iter_records(end))) == 1
            assert await kv.get_many(["m0", "m19", "nope"]) == \
                [{"i": 0, "s": "it's"}, {"i": 19, "s": "it's"}, None]
            assert await kv.count(prefix="m") == 20
            # a second batch reuses the prepared statement
            assert await kv.put_many_atomic([("m20", 20)]) == 1
            assert await kv.get("m20") == 20
        finally:
            await kv.close()
    with_server(scenario, tmp_path)


def test_atomic_batch_fails_as_a_whole_when_read_only(tmp_path):
    async def scenario(srv, port, connect):
        kv = PgKvClient("127.0.0.1", port)
        try:
            with pytest.raises(PgKvError) as ei:
                await kv.put_many_atomic([("a", 1), ("b", 2)])
            assert "read-only" in str(ei.value)
            # the failed block was closed: the connection is usable
            assert await kv.count() == 0
            assert kv._cli.txn_status == "I"
        finally:
            await kv.close()
        assert srv.kv == {} and srv.wal.end == 0
    with_server(scenario, tmp_path,
                conf={"default_transaction_read_only": "on"})


def test_commit_is_all_or_nothing_across_a_crash(tmp_path):
    """A transaction is one WAL record.  Stop the server with no
    checkpoint and restart: all three keys.  Cut the WAL file inside
    that record (the torn tail a crash leaves) and restart: none."""
    data = str(tmp_path / "pg")
    keys = {"t1": "one", "t2": "two", "t3": "three"}

    async def commit():
        srv, port = await start_minipg(data)
        try:
            cli = PgClient("127.0.0.1", port, "postgres")
            await cli.connect()
            await cli.query_params(INSERT, ["before", "0"])
            mark = srv.wal.end
            async with cli.transaction():
                for k, v in keys.items():
                    await cli.query_params(INSERT, [k, v])
            await cli.close()
            return mark, srv.wal.end
        finally:
            stop_minipg(srv)

    async def recovered():
        srv, _port = await start_minipg(data)
        try:
            return dict(srv.kv), srv.wal.end
        finally:
            stop_minipg(srv)

    mark, end = run(commit())
    assert not os.path.exists(os.path.join(data, "checkpoint.json"))
    kv, got_end = run(recovered())
    assert kv == dict(keys, before="0") and got_end == end

    seg = os.path.join(data, "wal-%016x.seg" % 0)
    assert os.path.getsize(seg) == end
    with open(seg, "r+b") as f:
        f.truncate(end - 5)         # inside the COMMIT record
    kv, got_end = run(recovered())
    assert kv == {"before": "0"} and got_end == mark


def test_tpcb_profile_needs_the_postgres_engine(tmp_path):
    from manatee_amd.tools import wrbench
    with pytest.raises(ValueError):
        run(wrbench.run([1], 1.0, str(tmp_path / "w"), engine="waldb",
                        profile="tpcb"))
    with pytest.raises(SystemExit):
        wrbench.main(["--profile", "tpcb"])
