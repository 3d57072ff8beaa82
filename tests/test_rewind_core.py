"""waldb rewind: fork-point arithmetic, the offline rewind of a diverged
data directory against a live upstream, its refusals, and the intent
marker.  Real waldb subprocesses, no cluster."""

import asyncio
import json
import os
import struct
import subprocess
import sys
import zlib

import pytest

from manatee_amd.common.logging import null_logger
from manatee_amd.db.waldb import ckpt as ckptmod
from manatee_amd.db.waldb import rewind
from tests import crashfs
from tests.rewind_util import (DIVERGENT, assert_converged, build_pair,
                               knobs, read_json, records_past,
                               segment_starts, start_as_standby, wal_bytes)
from tests.test_waldb import Node, REPO, free_port, wait_async

T1 = {"tl": 1, "at": 0}


def run(coro):
    return asyncio.run(asyncio.wait_for(coro, 60))


# ------------------------------------------------------------ arithmetic
@pytest.mark.parametrize("name,f,u,want", [
    ("equal histories, follower ahead",
     (1, [T1], 500), (1, [T1], 300), (1, 300)),
    ("follower one timeline behind, WAL past the switch",
     (1, [T1], 900), (2, [T1, {"tl": 2, "at": 700}], 1200), (1, 700)),
    ("both promoted 1->2 at different offsets",
     (2, [T1, {"tl": 2, "at": 600}], 800),
     (2, [T1, {"tl": 2, "at": 700}], 1200), (1, 600)),
    ("follower on a newer timeline than the upstream",
     (2, [T1, {"tl": 2, "at": 600}], 800), (1, [T1], 650), (1, 600)),
    ("newer follower, upstream short of the follower's switch",
     (2, [T1, {"tl": 2, "at": 600}], 800), (1, [T1], 550), (1, 550)),
    ("follower exactly at the switch point (noop)",
     (1, [T1], 700), (2, [T1, {"tl": 2, "at": 700}], 1200), (1, 700)),
    ("common timeline 2, third switch on the upstream only",
     (2, [T1, {"tl": 2, "at": 600}], 950),
     (3, [T1, {"tl": 2, "at": 600}, {"tl": 3, "at": 900}], 1000), (2, 900)),
    ("no common entry at all",
     (1, [], 100), (1, [T1], 300), (1, 0)),
])
def test_fork_point(name, f, u, want):
    assert rewind.fork_point(*f, *u) == want, name


def test_common_prefix_compares_entries_whole():
    a = [T1, {"tl": 2, "at": 600}, {"tl": 3, "at": 900}]
    b = [T1, {"tl": 2, "at": 600}, {"tl": 3, "at": 901}]
    assert rewind.common_prefix(a, b) == a[:2]
    assert rewind.common_prefix(a, a) == a
    assert rewind.common_prefix([], a) == []


# --------------------------------------------------------------- success
def _rewind(pair, data_dir=None):
    return rewind.rewind_data_dir(data_dir or pair.a.data_dir, "127.0.0.1",
                                  pair.b.port, null_logger())


def _assert_rewound(pair, res):
    d = pair.fork_lsn
    assert res.ok and res.fork_lsn == d, res
    a_start, a_wal = wal_bytes(pair.a.data_dir)
    b_start, b_wal = wal_bytes(pair.b.data_dir)
    assert a_start == b_start == 0
    assert a_wal == b_wal[:d]
    assert records_past(pair.a.data_dir, d) == 0
    ident = read_json(pair.a.data_dir, "waldb_ident.json")
    assert (ident["timeline"], ident["history"]) == (1, [T1])
    assert ident["ident"] == read_json(pair.b.data_dir,
                                       "waldb_ident.json")["ident"]
    assert not os.path.exists(os.path.join(pair.a.data_dir,
                                           rewind.MARKER_NAME))
    assert not os.path.exists(os.path.join(pair.a.data_dir, "promote"))


@pytest.mark.parametrize("position", ["mid", "segstart", "end"])
def test_rewind_then_stream(tmp_path, position):
    pair = build_pair(tmp_path, position)
    try:
        d = pair.fork_lsn
        starts = segment_starts(pair.a.data_dir)
        _, before = wal_bytes(pair.a.data_dir)
        assert len([s for s in starts if s < d]) >= 4, starts
        if position == "mid":
            assert d not in starts
            # the tail to cut spans more than one segment
            assert len([s for s in starts if s > d]) >= 2, starts
        elif position == "segstart":
            assert d in starts
        if position == "end":
            assert len(before) == d
        else:
            assert records_past(pair.a.data_dir, d) == DIVERGENT
        # a stale trigger must not survive into the standby
        open(os.path.join(pair.a.data_dir, "promote"), "w").close()

        res = _rewind(pair)
        assert res.result == ("noop" if position == "end" else "ok"), res
        assert res.bytes_cut == len(before) - d
        _assert_rewound(pair, res)
        # nothing left to do the second time
        assert _rewind(pair).result == "noop"

        start_as_standby(pair)
        run(assert_converged(pair))
        ident = read_json(pair.a.data_dir, "waldb_ident.json")
        assert ident["timeline"] == 2
        assert ident["history"] == [T1, {"tl": 2, "at": d}]
    finally:
        pair.stop()


def test_layered_rewind_drops_the_layers_past_the_fork(tmp_path):
    pair = build_pair(tmp_path, "mid", layered=True)
    try:
        d = pair.fork_lsn
        before = read_json(pair.a.data_dir, "checkpoint.json")
        lsns = [ckptmod.parse_layer_name(n)[0] for n in before["layers"]]
        assert lsns[0] <= d and before["layers"][0].endswith(".base")
        assert len([x for x in lsns if x > d]) >= 2, before
        res = _rewind(pair)
        assert res.result == "ok", res
        assert res.layers_dropped == len([x for x in lsns if x > d])
        _assert_rewound(pair, res)
        after = read_json(pair.a.data_dir, "checkpoint.json")
        assert after["layers"] == [n for n, x in zip(before["layers"], lsns)
                                   if x <= d]
        assert after["lsn"] <= d
        # the recovered kv is the upstream's at D: no key of the tail
        kv, _layers = ckptmod.load_layers(pair.a.data_dir, after)
        assert not set(pair.divergent_keys) & set(kv)
        start_as_standby(pair)
        run(assert_converged(pair))
    finally:
        pair.stop()


# -------------------------------------------------------------- refusals
@pytest.fixture(scope="module")
def diverged(tmp_path_factory):
    pair = build_pair(tmp_path_factory.mktemp("diverged"), "mid")
    yield pair
    pair.stop()


@pytest.fixture(scope="module")
def diverged_layered(tmp_path_factory):
    pair = build_pair(tmp_path_factory.mktemp("layered"), "mid",
                      layered=True)
    yield pair
    pair.stop()


def _assert_refused(pair, data_dir, reason):
    before = crashfs.snapshot(data_dir)
    res = _rewind(pair, data_dir)
    assert not res.ok and res.result == "refused", res
    assert res.reason == reason, res
    assert crashfs.snapshot(data_dir) == before
    return res


def test_refuses_a_full_checkpoint_past_the_fork(diverged, tmp_path):
    # a server on a copy of the diverged directory checkpoints at once
    node = Node(tmp_path, "ckpt")
    diverged.copy_of_a(node.data_dir)
    node.write_conf(role="primary", extra=knobs(1))
    node.start()
    try:
        async def go():
            cli = node.client()

            async def done():
                st = await cli.status()
                return st["checkpoint_lsn"] == st["current_lsn"]
            await wait_async(done, what="checkpoint")
            await cli.close()
        run(go())
        node.kill9()
    finally:
        node.stop()
    assert read_json(node.data_dir, "checkpoint.json")["lsn"] \
        > diverged.fork_lsn
    _assert_refused(diverged, node.data_dir, "checkpoint-past-fork")


def test_refuses_a_base_layer_past_the_fork(diverged_layered, tmp_path):
    d = diverged_layered.copy_of_a(str(tmp_path / "compacted"))
    names = read_json(d, "checkpoint.json")["layers"]
    # a forced compaction: every layer folded into one base at the top
    base = ckptmod.merge_layers(d, names)
    assert base["lsn"] > diverged_layered.fork_lsn
    with open(os.path.join(d, "checkpoint.json"), "w") as f:
        json.dump(ckptmod.dump_manifest(base["lsn"], [base]), f)
    _assert_refused(diverged_layered, d, "checkpoint-past-fork")


def test_refuses_wal_recycled_below_the_surviving_image(diverged, tmp_path):
    d = diverged.copy_of_a(str(tmp_path / "recycled"))
    os.unlink(os.path.join(d, "wal-%016x.seg" % 0))
    _assert_refused(diverged, d, "checkpoint-past-fork")


def test_refuses_history_that_differs_below_the_fork(diverged, tmp_path):
    d = diverged.copy_of_a(str(tmp_path / "flipped"))
    # one payload byte of the first record, its frame CRC recomputed:
    # every frame still validates, the bytes are not the upstream's
    path = os.path.join(d, "wal-%016x.seg" % 0)
    with open(path, "rb") as f:
        buf = bytearray(f.read())
    length, _crc = struct.unpack_from(">II", buf, 0)
    assert 8 + length < diverged.fork_lsn
    buf[8 + length - 3] ^= 0x01
    struct.pack_into(">I", buf, 4, zlib.crc32(bytes(buf[8:8 + length])))
    with open(path, "wb") as f:
        f.write(buf)
    _assert_refused(diverged, d, "history-mismatch")


def test_refuses_a_fork_inside_a_record(diverged, tmp_path):
    d = diverged.copy_of_a(str(tmp_path / "inside"))

    def probe(req):
        resp = rewind.probe_upstream("127.0.0.1", diverged.b.port, req)
        _, wal = wal_bytes(diverged.b.data_dir)
        lsn = resp["fork_lsn"] - 3
        return dict(resp, fork_lsn=lsn,
                    crc32=zlib.crc32(wal[resp["window_start"]:lsn]))
    before = crashfs.snapshot(d)
    res = rewind.rewind_data_dir(d, "127.0.0.1", 1, null_logger(),
                                 probe=probe)
    assert (res.result, res.reason) == ("refused", "not-a-boundary")
    assert crashfs.snapshot(d) == before


def test_refuses_a_foreign_ident(diverged, tmp_path):
    d = diverged.copy_of_a(str(tmp_path / "foreign"))
    ident = read_json(d, "waldb_ident.json")
    ident["ident"] = "0" * 32
    with open(os.path.join(d, "waldb_ident.json"), "w") as f:
        json.dump(ident, f)
    _assert_refused(diverged, d, "ident-mismatch")


def test_refuses_an_unreachable_upstream_and_a_running_db(diverged,
                                                          tmp_path):
    d = diverged.copy_of_a(str(tmp_path / "alone"))
    before = crashfs.snapshot(d)
    res = rewind.rewind_data_dir(d, "127.0.0.1", free_port(), null_logger())
    assert res.result == "refused" and \
        res.reason.startswith("connection-failed"), res
    assert crashfs.snapshot(d) == before
    with open(os.path.join(d, "waldb.pid"), "w") as f:
        f.write("%d 1\n" % os.getpid())
    res = _rewind(diverged, d)
    assert res.result == "refused" and res.reason.startswith("running"), res


def test_probe_is_unverifiable_without_overlap(diverged):
    ident = read_json(diverged.b.data_dir, "waldb_ident.json")
    d = diverged.fork_lsn
    req = {"ident": ident["ident"], "timeline": 1, "history": [T1],
           "wal_start": d, "wal_end": d + 100}
    resp = rewind.probe_upstream("127.0.0.1", diverged.b.port, req)
    assert resp == {"ok": False, "error": "unverifiable"}
    resp = rewind.probe_upstream("127.0.0.1", diverged.b.port,
                                 dict(req, wal_start=0))
    _, wal = wal_bytes(diverged.b.data_dir)
    assert resp == {"ok": True, "timeline": 2, "history": ident["history"],
                    "fork_lsn": d, "window_start": 0,
                    "crc32": zlib.crc32(wal[:d])}


def test_minipg_answers_the_probe_on_its_json_passthrough(tmp_path):
    """The PostgreSQL-shaped front-end hands a connection that begins
    with ``{`` to the same core."""
    from tests.minipg_inproc import start_minipg, stop_minipg

    async def go():
        data = str(tmp_path / "pg")
        srv, port = await start_minipg(data)
        try:
            for i in range(5):
                lsn, err = srv._append_write({"op": "put", "k": "k%d" % i,
                                              "v": i})
                assert err is None
            srv.wal.flush_buffer()
            end = srv.wal.end
            req = {"ident": srv.ident["ident"], "timeline": 1,
                   "history": srv.history, "wal_start": 0,
                   "wal_end": end + 77}
            loop = asyncio.get_running_loop()
            resp = await loop.run_in_executor(
                None, rewind.probe_upstream, "127.0.0.1", port, req)
            assert resp == {"ok": True, "timeline": 1,
                            "history": srv.history, "fork_lsn": end,
                            "window_start": 0,
                            "crc32": zlib.crc32(srv.wal.read(0, end))}
            resp = await loop.run_in_executor(
                None, rewind.probe_upstream, "127.0.0.1", port,
                dict(req, ident="someone else"))
            assert resp == {"ok": False, "error": "ident-mismatch"}
        finally:
            stop_minipg(srv)
    run(go())


# ---------------------------------------------------------------- marker
def test_server_refuses_to_start_on_an_unfinished_rewind(diverged,
                                                         tmp_path):
    node = Node(tmp_path, "marked")
    diverged.copy_of_a(node.data_dir)
    node.write_conf(role="primary", extra=knobs())
    with open(os.path.join(node.data_dir, rewind.MARKER_NAME), "w") as f:
        json.dump({"fork_lsn": diverged.fork_lsn, "timeline": 1,
                   "history": [T1], "replay_from": 0, "manifest": None}, f)
    proc = subprocess.run(
        [sys.executable, "-m", "manatee_amd.db.waldb.server",
         "-D", node.data_dir], env=dict(os.environ, PYTHONPATH=REPO),
        stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=30)
    assert proc.returncode != 0
    assert b"unfinished rewind" in proc.stderr
    assert not os.path.exists(os.path.join(node.data_dir, "waldb.pid"))
    # a second rewind finishes the first one, without the upstream
    res = rewind.rewind_data_dir(node.data_dir, "127.0.0.1", free_port(),
                                 null_logger())
    assert res.result == "ok" and res.resumed
    _, wal = wal_bytes(node.data_dir)
    assert wal == wal_bytes(diverged.b.data_dir)[1][:diverged.fork_lsn]
    assert not os.path.exists(os.path.join(node.data_dir,
                                           rewind.MARKER_NAME))


def test_command_line_entry_point(diverged, tmp_path):
    d = diverged.copy_of_a(str(tmp_path / "cli"))
    proc = subprocess.run(
        [sys.executable, "-m", "manatee_amd.db.waldb.rewind", "-D", d,
         "--upstream", "127.0.0.1:%d" % diverged.b.port],
        env=dict(os.environ, PYTHONPATH=REPO), stdout=subprocess.PIPE,
        stderr=subprocess.DEVNULL, timeout=30)
    assert proc.returncode == 0
    out = json.loads(proc.stdout)
    assert out["result"] == "ok"
    assert out["fork_lsn_bytes"] == diverged.fork_lsn
    assert records_past(d, diverged.fork_lsn) == 0
