"""Unit tests for the replication core's settings handling and
timeline switch (db/waldb/core.py) through both front-ends."""

import asyncio
import dataclasses
import io
import json
import os

from manatee_amd.common import confparser
from manatee_amd.common.logging import Logger, null_logger
from manatee_amd.db.minipg.server import MinipgServer
from manatee_amd.db.minipg.server import init_data_dir as pg_init
from manatee_amd.db.waldb.core import (DEFAULT_CKPT_WAL_BYTES,
                                       DEFAULT_WAL_KEEP_BYTES, Settings,
                                       parse_knobs)
from manatee_amd.db.waldb.server import WaldbServer, init_data_dir

KNOBS = {"checkpoint_wal_bytes": "1000", "wal_keep_bytes": "2000",
         "wal_segment_bytes": "3000", "wal_sender_timeout": "1500"}


def run(coro, timeout=30):
    return asyncio.run(asyncio.wait_for(coro, timeout))


def _waldb(tmp_path, log=None, **conf):
    data = str(tmp_path / "db")
    if not os.path.exists(data):
        init_data_dir(data)
    base = {"role": "primary", "listen_ip": "127.0.0.1", "port": "0",
            "name": "n1"}
    base.update(conf)
    confparser.write(os.path.join(data, "waldb.conf"), base)
    return WaldbServer(data, log or null_logger())


def _minipg(tmp_path, **conf):
    data = str(tmp_path / "pg" / "data")
    if not os.path.exists(data):
        pg_init(data, "12.0")
    base = {"listen_addresses": "'127.0.0.1'", "port": "0"}
    base.update(conf)
    confparser.write(os.path.join(data, "postgresql.conf"), base)
    return MinipgServer(data, null_logger())


def _stop(srv) -> None:
    srv._sever_repl()
    if srv._server is not None:
        srv._server.close()
    if srv._flusher is not None:
        srv._flusher.cancel()
    srv.wal.close()


def _knobs(s: Settings):
    return (s.ckpt_wal_bytes, s.wal_keep_bytes, s.wal_segment_bytes,
            s.wal_sender_timeout_s)


# ------------------------------------------------------------ parse_knobs

def test_knobs_absent_keys_waldb_resets_sizes_minipg_keeps_all(tmp_path):
    first = _waldb(tmp_path, **KNOBS).read_settings(Settings())
    assert _knobs(first) == (1000, 2000, 3000, 1500.0)
    again = _waldb(tmp_path).read_settings(first)
    assert _knobs(again) == (DEFAULT_CKPT_WAL_BYTES, DEFAULT_WAL_KEEP_BYTES,
                             3000, 1500.0)

    first = _minipg(tmp_path, **KNOBS).read_settings(Settings())
    assert _knobs(first) == (1000, 2000, 3000, 1.5)
    again = _minipg(tmp_path).read_settings(first)
    assert _knobs(again) == (1000, 2000, 3000, 1.5)


def test_knobs_sender_timeout_units(tmp_path):
    raw = {"wal_sender_timeout": "1500"}
    assert parse_knobs(raw, Settings(), 1.0).wal_sender_timeout_s == 1500.0
    assert parse_knobs(raw, Settings(), 0.001).wal_sender_timeout_s == 1.5
    assert _waldb(tmp_path, **raw).read_settings(
        Settings()).wal_sender_timeout_s == 1500.0
    assert _minipg(tmp_path, **raw).read_settings(
        Settings()).wal_sender_timeout_s == 1.5


def test_knobs_stop_at_first_unparsable_value(tmp_path):
    raw = dict(KNOBS, wal_keep_bytes="lots")
    prev = Settings(ckpt_wal_bytes=11, wal_keep_bytes=22,
                    wal_segment_bytes=33, wal_sender_timeout_s=44.0)
    assert _knobs(parse_knobs(raw, prev, 1.0)) == (1000, 22, 33, 44.0)
    # quoted values parse like bare ones
    assert parse_knobs({"wal_keep_bytes": "'5'"}, prev, 1.0) \
        .wal_keep_bytes == 5
    # waldb falls back to the default size and the previous rest ...
    got = _waldb(tmp_path, **raw).read_settings(prev)
    assert _knobs(got) == (1000, DEFAULT_WAL_KEEP_BYTES, 33, 44.0)
    # ... minipg to the previous values throughout
    got = _minipg(tmp_path, **raw).read_settings(prev)
    assert _knobs(got) == (1000, 22, 33, 44.0)


# ------------------------------------------------- minipg read_settings

def test_minipg_settings_standby_signal(tmp_path):
    srv = _minipg(
        tmp_path,
        primary_conninfo="'host=10.0.0.7 port=6000 user=u "
                         "application_name=peer2'",
        promote_trigger_file="'/some/where/go'",
        synchronous_standby_names="'peer3'",
        default_transaction_read_only="on")
    open(os.path.join(srv.data_dir, "standby.signal"), "w").close()
    s = srv.read_settings(Settings())
    assert (s.role, s.upstream, s.name) == \
        ("standby", "10.0.0.7:6000", "peer2")
    assert s.trigger_path == "/some/where/go"
    assert (s.sync_standby, s.read_only) == ("peer3", True)
    assert (s.listen_ip, s.port) == ("127.0.0.1", "0")


def test_minipg_settings_recovery_conf(tmp_path):
    srv = _minipg(tmp_path, promote_trigger_file="'/ignored/pre12'")
    rec = os.path.join(srv.data_dir, "recovery.conf")
    confparser.write(rec, {
        "standby_mode": "on",
        "primary_conninfo": "'host=10.0.0.8 application_name=peer9'",
        "trigger_file": "'/old/style/trigger'"})
    s = srv.read_settings(Settings())
    assert (s.role, s.upstream, s.name) == \
        ("standby", "10.0.0.8:5432", "peer9")
    assert s.trigger_path == "/old/style/trigger"
    # standby_mode off: recovery.conf does not make a standby
    confparser.write(rec, {"standby_mode": "off",
                           "trigger_file": "'/old/style/trigger'"})
    assert srv.read_settings(Settings()).role == "primary"


def test_minipg_settings_plain_primary(tmp_path):
    srv = _minipg(tmp_path, listen_addresses="'*'", port="5433")
    s = srv.read_settings(Settings())
    assert (s.role, s.upstream, s.sync_standby) == ("primary", None, None)
    assert s.trigger_path == os.path.join(
        os.path.dirname(srv.data_dir), "promote")
    assert (s.listen_ip, s.port) == ("0.0.0.0", "5433")
    assert not s.read_only


# ---------------------------------------------------------------- reload

def test_reload_refuses_foreign_port_and_keeps_settings(tmp_path):
    async def go():
        out = io.StringIO()
        srv = _waldb(tmp_path, log=Logger("t", stream=out),
                     synchronous_standby_names="'ours'")
        await srv.start()
        try:
            old = srv.settings
            segment = srv.wal.segment_bytes
            _waldb(tmp_path, port="5999", role="standby",
                   synchronous_standby_names="'theirs'",
                   default_transaction_read_only="on",
                   wal_segment_bytes="4096")
            srv._on_sighup()
            assert srv.settings is old
            assert (srv.role, srv.sync_standby, srv.read_only) == \
                ("primary", "ours", False)
            assert srv.wal.segment_bytes == segment
            errors = [json.loads(line) for line in
                      out.getvalue().splitlines()]
            errors = [r for r in errors if r["level"] >= 50]
            assert len(errors) == 1
            assert "different port" in errors[0]["msg"]
            assert errors[0]["conf_port"] == "5999"
            # the same port with other values IS adopted, as a new object
            _waldb(tmp_path, synchronous_standby_names="'next'")
            srv._on_sighup()
            assert srv.settings is not old
            assert srv.sync_standby == "next"
            assert dataclasses.replace(
                srv.settings, sync_standby="ours") == old
        finally:
            _stop(srv)
    run(go())


# ------------------------------------------------------- _bump_timeline

async def _write_some(srv, n=5):
    for i in range(n):
        res = await srv._do_write({"op": "put", "k": "k%d" % i, "v": i})
        assert res["ok"]
    return srv.wal.end


def test_bump_timeline_at_start_with_trigger(tmp_path):
    async def go():
        srv = _waldb(tmp_path)
        await srv.start()
        try:
            end = await _write_some(srv)
            assert (srv.timeline, end > 0) == (1, True)
        finally:
            _stop(srv)
        trigger = os.path.join(srv.data_dir, "promote")
        open(trigger, "w").close()
        srv = _waldb(tmp_path)
        await srv.start()
        try:
            assert srv.timeline == 2
            assert srv.history[-1] == {"tl": 2, "at": end}
            assert srv.history[0] == {"tl": 1, "at": 0}
            assert not os.path.exists(trigger)
            with open(os.path.join(srv.data_dir,
                                   "waldb_ident.json")) as f:
                assert json.load(f)["history"] == srv.history
        finally:
            _stop(srv)
    run(go())


def test_bump_timeline_on_online_promote(tmp_path):
    async def go():
        srv = _waldb(tmp_path)
        await srv.start()
        try:
            end = await _write_some(srv)
        finally:
            _stop(srv)
        srv = _waldb(tmp_path, role="standby")
        await srv.start()
        try:
            assert (srv.role, srv.timeline, srv.wal.end) == \
                ("standby", 1, end)
            trigger = os.path.join(srv.data_dir, "promote")
            open(trigger, "w").close()
            _waldb(tmp_path, role="primary")
            srv._on_sighup()
            assert (srv.role, srv.upstream) == ("primary", None)
            assert srv.timeline == 2
            assert srv.history[-1] == {"tl": 2, "at": end}
            assert not os.path.exists(trigger)
            with open(os.path.join(srv.data_dir,
                                   "waldb_ident.json")) as f:
                assert json.load(f)["history"] == srv.history
            res = await srv._do_write({"op": "put", "k": "after", "v": 1})
            assert res["ok"]
        finally:
            _stop(srv)
    run(go())
