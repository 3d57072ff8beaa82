"""Incremental layered checkpoints (``checkpoint_mode = incremental``,
db/waldb/ckpt.py): hermetic, in-process.  A ``WaldbServer`` object is
driven through ``_do_write`` and ``_checkpoint()``; ``checkpoint_wal_bytes``
stays at its default unless a test is about spacing, so the flush loop
never starts a checkpoint of its own.
"""

import asyncio
import io
import json
import os
import random
import shutil
import threading

import pytest

from manatee_amd.common import confparser
from manatee_amd.common.logging import Logger, null_logger
from manatee_amd.db.engine import WaldbEngine
from manatee_amd.db.waldb import ckpt as ckptmod
from manatee_amd.db.waldb.ckpt import CheckpointCorrupt, CheckpointFormatError
from manatee_amd.db.waldb.client import WaldbClient
from manatee_amd.db.waldb.core import Settings, parse_knobs
from manatee_amd.db.waldb.server import (CKPT_NAME, WaldbServer,
                                         init_data_dir)
from manatee_amd.db.waldb.wal import decode_op
from tests.minipg_inproc import start_minipg, stop_minipg

INCR = {"checkpoint_mode": "incremental"}


def run(coro, timeout=60):
    return asyncio.run(asyncio.wait_for(coro, timeout))


def _server(data, log=None, **conf):
    if not os.path.exists(data):
        init_data_dir(data)
    base = {"role": "primary", "listen_ip": "127.0.0.1", "port": "0",
            "name": "n1"}
    base.update(conf)
    confparser.write(os.path.join(data, "waldb.conf"), base)
    return WaldbServer(data, log or null_logger())


async def _start(data, **conf):
    srv = _server(data, **conf)
    await srv.start()
    return srv


def _crash(srv) -> None:
    """Abandon the server object without a checkpoint or a clean stop,
    as tests/minipg_inproc.py does."""
    if srv._server is not None:
        srv._server.close()
    if srv._flusher is not None:
        srv._flusher.cancel()
    srv.wal.close()


async def _put(srv, k, v):
    assert (await srv._do_write({"op": "put", "k": k, "v": v}))["ok"]


async def _del(srv, k):
    assert (await srv._do_write({"op": "del", "k": k}))["ok"]


def _manifest(data) -> dict:
    with open(os.path.join(data, CKPT_NAME)) as f:
        return json.load(f)


def _layer_files(data):
    try:
        return sorted(os.listdir(os.path.join(data, ckptmod.CKPT_DIR)))
    except FileNotFoundError:
        return []


def _subops(data, name):
    """Every put/del record of one layer file, in order."""
    _header, ops = ckptmod.read_layer(
        os.path.join(data, ckptmod.CKPT_DIR), name)
    return [sub for op in ops for sub in op["ops"]]


# ---------------------------------------------------------- delta is O(dirty)

def test_delta_holds_only_the_dirty_keys(tmp_path):
    data = str(tmp_path / "n1")

    async def go():
        srv = await _start(data, **INCR)
        try:
            for i in range(300):
                await _put(srv, "k%03d" % i, "x" * 100)
            await srv._checkpoint()
            man = _manifest(data)
            assert man["format"] == 2 and len(man["layers"]) == 1
            base = os.path.join(data, ckptmod.CKPT_DIR, man["layers"][0])
            before = os.stat(base)

            for i in (5, 50, 150):
                await _put(srv, "k%03d" % i, "y" * 100)
            await _del(srv, "k299")
            await srv._checkpoint()
            man = _manifest(data)
            assert "kv" not in man
            assert len(man["layers"]) == 2
            assert man["layers"][0].endswith(".base")
            assert man["layers"][1].endswith(".delta")
            assert man["lsn"] == srv.ckpt_lsn == srv.replay_lsn
            after = os.stat(base)
            assert (after.st_ino, after.st_mtime_ns, after.st_size) == \
                (before.st_ino, before.st_mtime_ns, before.st_size)
            subs = _subops(data, man["layers"][1])
            assert sorted((s["op"], s["k"]) for s in subs) == [
                ("del", "k299"), ("put", "k005"), ("put", "k050"),
                ("put", "k150")]
            delta = os.path.join(data, ckptmod.CKPT_DIR, man["layers"][1])
            assert os.path.getsize(delta) * 10 < after.st_size
            assert len(_subops(data, man["layers"][0])) == 300
            assert srv._dirty == set()
        finally:
            _crash(srv)
    run(go())


def test_large_layers_are_chunked_into_several_frames(tmp_path, monkeypatch):
    """No frame may approach the record cap: a layer is cut into batches
    by record count and by bytes."""
    monkeypatch.setattr(ckptmod, "CHUNK_KEYS", 7)
    d = str(tmp_path)
    items = [("k%d" % i, i) for i in range(30)] + [("t", ckptmod.TOMBSTONE)]
    info = ckptmod.write_layer(os.path.join(d, "ckpt"), "base", 9, 0,
                               items, 31)
    header, ops = ckptmod.read_layer(os.path.join(d, "ckpt"), info["name"])
    assert header["count"] == 31 == info["records"]
    assert [len(op["ops"]) for op in ops] == [7, 7, 7, 7, 3]
    monkeypatch.setattr(ckptmod, "CHUNK_BYTES", 64)
    ckptmod.write_layer(os.path.join(d, "ckpt"), "base", 9, 0,
                        [("a", "v" * 100), ("b", "v" * 100)], 2)
    _h, ops = ckptmod.read_layer(os.path.join(d, "ckpt"), info["name"])
    assert [len(op["ops"]) for op in ops] == [1, 1]
    with pytest.raises(ValueError):
        ckptmod.write_layer(os.path.join(d, "ckpt"), "base", 10, 0, items, 5)


@pytest.mark.parametrize("window", [16, 300, 1 << 20])
def test_layer_validation_in_windows(tmp_path, monkeypatch, window):
    """A layer is scanned a window at a time (the scanner keeps the GIL):
    frames that straddle a window edge, a frame larger than the window,
    and damage anywhere are all seen as in one pass."""
    monkeypatch.setattr(ckptmod, "CHUNK_KEYS", 10)
    d = str(tmp_path)
    items = [("k%03d" % i, "v" * (i % 37)) for i in range(200)]
    info = ckptmod.write_layer(d, "base", 5, 0, items, len(items))
    monkeypatch.setattr(ckptmod, "SCAN_WINDOW", window)
    _header, ops = ckptmod.read_layer(d, info["name"])
    assert [(s["k"], s["v"]) for op in ops for s in op["ops"]] == items
    path = os.path.join(d, info["name"])
    with open(path, "rb") as f:
        good = f.read()
    for off in (0, 9, len(good) // 2, len(good) - 1):
        bad = bytearray(good)
        bad[off] ^= 0x10
        with open(path, "wb") as f:
            f.write(bad)
        with pytest.raises(CheckpointCorrupt):
            ckptmod.read_layer(d, info["name"])


# ------------------------------------------------------- recovery equivalence

def test_recovery_equals_the_model_at_every_crash_point(tmp_path):
    data = str(tmp_path / "n1")
    rng = random.Random(20240607)
    model = {}
    keys = ["key%02d" % i for i in range(40)]

    async def step(srv, i):
        r = rng.random()
        if r < 0.55:
            k = rng.choice(keys)
            model[k] = "v%d-%s" % (i, "p" * rng.randrange(60))
            await _put(srv, k, model[k])
        elif r < 0.8:
            k = rng.choice(keys)
            model.pop(k, None)
            await _del(srv, k)
        else:
            ops = []
            for _ in range(rng.randrange(1, 6)):
                k = rng.choice(keys)
                if rng.random() < 0.6:
                    ops.append({"op": "put", "k": k, "v": "b%d" % i})
                    model[k] = "b%d" % i
                else:
                    ops.append({"op": "del", "k": k})
                    model.pop(k, None)
            assert (await srv._do_write({"op": "batch", "ops": ops}))["ok"]

    async def go():
        compactions = crashes = 0
        srv = await _start(data, **INCR)
        try:
            # a batch that puts and deletes the same key, both ways round
            assert (await srv._do_write({"op": "batch", "ops": [
                {"op": "put", "k": "both", "v": 1},
                {"op": "del", "k": "both"},
                {"op": "del", "k": "back"},
                {"op": "put", "k": "back", "v": 2}]}))["ok"]
            model["back"] = 2
            # a key deleted in one layer and put again in a later one
            await _put(srv, "phoenix", "first")
            await srv._checkpoint()
            await _del(srv, "phoenix")
            await srv._checkpoint()
            assert {"op": "del", "k": "phoenix"} in _subops(
                data, _manifest(data)["layers"][-1])
            await _put(srv, "phoenix", "second")
            model["phoenix"] = "second"
            await srv._checkpoint()

            for i in range(400):
                await step(srv, i)
                if rng.random() < 0.12:
                    await srv._checkpoint()
                    assert srv.ckpt_lsn == srv.replay_lsn
                if i % 45 == 44:
                    # crash, sometimes straight after a checkpoint
                    assert srv.kv == model
                    want = (srv.ckpt_lsn, srv.replay_lsn)
                    compactions += srv._compact_count
                    _crash(srv)
                    srv = await _start(data, **INCR)
                    crashes += 1
                    assert srv.kv == model
                    assert (srv.ckpt_lsn, srv.replay_lsn) == want
                    assert srv.wal.end == want[1]
            compactions += srv._compact_count
        finally:
            _crash(srv)
        assert crashes >= 5
        assert compactions >= 3, compactions
    run(go())


def test_minipg_commit_then_checkpoint_survives_restart(tmp_path):
    from manatee_amd.db.pgwire import PgClient
    data = str(tmp_path / "pg")
    insert = "INSERT INTO kv (k, v) VALUES ($1, $2)"

    async def go():
        srv, port = await start_minipg(data, INCR)
        try:
            assert srv.settings.ckpt_mode == "incremental"
            cli = PgClient("127.0.0.1", port, "postgres")
            await cli.connect()
            await cli.query_params(insert, ["before", "0"])
            for i in range(30):     # a base the delta stays smaller than
                await cli.query_params(insert, ["pad%d" % i, "x" * 50])
            await srv._checkpoint()
            async with cli.transaction():
                for k in ("t1", "t2", "t3"):
                    await cli.query_params(insert, [k, k.upper()])
                await cli.query_params(
                    "DELETE FROM kv WHERE k = $1", ["before"])
            await cli.close()
            await srv._checkpoint()
            man = _manifest(data)
            assert man["format"] == 2 and len(man["layers"]) == 2
            assert len(_subops(data, man["layers"][1])) == 4
            want = dict(srv.kv)
            end = srv.wal.end
        finally:
            stop_minipg(srv)
        assert want == dict({"pad%d" % i: "x" * 50 for i in range(30)},
                            t1="T1", t2="T2", t3="T3")
        # make the WAL useless: only the layers can bring the keys back
        for name in os.listdir(data):
            if name.startswith("wal-"):
                os.unlink(os.path.join(data, name))
        srv, _port = await start_minipg(data, INCR)
        try:
            assert srv.kv == want
            assert (srv.ckpt_lsn, srv.replay_lsn, srv.wal.end) == \
                (end, end, end)
        finally:
            stop_minipg(srv)
    run(go())


# ------------------------------------------------------------------ tombstones

def test_tombstone_outlives_the_wal_and_compaction_drops_it(tmp_path):
    data = str(tmp_path / "n1")
    small = dict(INCR, wal_keep_bytes="512", wal_segment_bytes="1024")

    async def go():
        srv = await _start(data, **small)
        try:
            for i in range(30):
                await _put(srv, "k%02d" % i, "x" * 100)
            await _put(srv, "gone", "soon")
            await srv._checkpoint()
            await _del(srv, "gone")
            del_lsn = srv.replay_lsn
            for i in range(20):           # roll several segments
                await _put(srv, "k%02d" % i, "y" * 100)
            await srv._checkpoint()
            assert srv.wal.start > del_lsn, "the delete is still in the WAL"
            man = _manifest(data)
            assert len(man["layers"]) == 2
            assert {"op": "del", "k": "gone"} in _subops(data,
                                                         man["layers"][1])
            want = dict(srv.kv)
        finally:
            _crash(srv)
        assert "gone" not in want

        srv = await _start(data, **small)
        try:
            assert srv.kv == want and "gone" not in srv.kv
            n = 0
            while srv._compact_count == 0:
                await _put(srv, "k%02d" % (n % 30), "z" * 100)
                n += 1
                if n % 10 == 0:
                    await srv._checkpoint()
                assert n < 1000
            man = _manifest(data)
            assert len(man["layers"]) == 1
            subs = _subops(data, man["layers"][0])
            assert all(s["op"] == "put" for s in subs)
            assert len(subs) == len(srv.kv) == 30
            assert {s["k"]: s["v"] for s in subs} == srv.kv
            want = dict(srv.kv)
        finally:
            _crash(srv)
        srv = await _start(data, **small)
        try:
            assert srv.kv == want
        finally:
            _crash(srv)
    run(go())


# ---------------------------------------------------- compaction under writes

def test_writes_during_a_compaction_go_into_the_next_delta(tmp_path,
                                                           monkeypatch):
    data = str(tmp_path / "n1")
    entered, release = threading.Event(), threading.Event()
    real_merge = ckptmod.merge_layers

    def slow_merge(data_dir, names):
        entered.set()
        assert release.wait(30)
        return real_merge(data_dir, names)

    async def go():
        model = {}
        srv = await _start(data, **INCR)
        try:
            for i in range(20):
                model["k%02d" % i] = "a"
                await _put(srv, "k%02d" % i, "a")
            await srv._checkpoint()
            for i in range(20):
                model["k%02d" % i] = "b" * 50
                await _put(srv, "k%02d" % i, "b" * 50)
            assert srv._compact_count == 0
            monkeypatch.setattr(ckptmod, "merge_layers", slow_merge)
            task = asyncio.get_running_loop().create_task(srv._checkpoint())
            while not entered.is_set():
                await asyncio.sleep(0.001)
            # the merge is running in the executor: keep writing
            assert srv._ckpt_running
            for i in range(10, 30):
                model["k%02d" % i] = "during"
                await _put(srv, "k%02d" % i, "during")
            model.pop("k00")
            await _del(srv, "k00")
            release.set()
            await task
            monkeypatch.setattr(ckptmod, "merge_layers", real_merge)
            assert srv._compact_count == 1 and not srv._ckpt_running
            man = _manifest(data)
            assert len(man["layers"]) == 1
            assert man["layers"][0].endswith(".base")
            # the base is the state at the checkpoint, not the live kv
            merged = {s["k"]: s["v"] for s in _subops(data,
                                                      man["layers"][0])}
            assert merged == {"k%02d" % i: "b" * 50 for i in range(20)}
            assert srv._dirty == {"k%02d" % i for i in range(10, 30)} \
                | {"k00"}
            assert srv.kv == model
            want = (srv.ckpt_lsn, srv.replay_lsn)
        finally:
            release.set()
            _crash(srv)
        srv = await _start(data, **INCR)
        try:
            assert srv.kv == model
            assert (srv.ckpt_lsn, srv.replay_lsn) == want
            await srv._checkpoint()
            assert len(_manifest(data)["layers"]) == 2
        finally:
            _crash(srv)
        srv = await _start(data, **INCR)
        try:
            assert srv.kv == model
        finally:
            _crash(srv)
    run(go())


def test_large_merges_run_in_a_child_process(tmp_path, monkeypatch):
    """Past ``MERGE_IN_CHILD_BYTES`` the merge is a child process; the
    result is the one the in-thread merge gives, and a merge that fails
    there leaves the layers and the manifest as they were."""
    data = str(tmp_path / "n1")

    async def go():
        out = io.StringIO()
        srv = _server(data, log=Logger("t", stream=out), **INCR)
        await srv.start()
        try:
            for i in range(20):
                await _put(srv, "k%02d" % i, "a" * 30)
            await srv._checkpoint()
            await _del(srv, "k00")
            for i in range(1, 20):
                await _put(srv, "k%02d" % i, "b" * 60)
            in_thread = []
            real_merge = ckptmod.merge_layers
            monkeypatch.setattr(ckptmod, "merge_layers", lambda *a: (
                in_thread.append(a), real_merge(*a))[1])
            monkeypatch.setattr(ckptmod, "MERGE_IN_CHILD_BYTES", 0)
            await srv._checkpoint()
            assert srv._compact_count == 1 and not in_thread
            man = _manifest(data)
            assert len(man["layers"]) == 1
            assert srv._layers[0] == {
                "name": man["layers"][0], "kind": "base",
                "lsn": man["lsn"], "records": 19,
                "bytes": os.path.getsize(os.path.join(
                    data, ckptmod.CKPT_DIR, man["layers"][0]))}
            assert {s["k"]: s["v"] for s in _subops(
                data, man["layers"][0])} == srv.kv

            # damage the base, then make a compaction due
            path = os.path.join(data, ckptmod.CKPT_DIR, man["layers"][0])
            with open(path, "r+b") as f:
                f.seek(40)
                f.write(b"\xff")
            for i in range(1, 20):
                await _put(srv, "k%02d" % i, "c" * 90)
            await srv._checkpoint()
            assert srv._compact_count == 1
            assert "checkpoint compaction failed" in out.getvalue()
            assert "layer merge failed" in out.getvalue()
            assert len(_manifest(data)["layers"]) == 2 == len(srv._layers)
        finally:
            _crash(srv)
    run(go())


def test_failed_layer_write_keeps_the_keys_dirty(tmp_path, monkeypatch):
    data = str(tmp_path / "n1")

    async def go():
        out = io.StringIO()
        srv = _server(data, log=Logger("t", stream=out), **INCR)
        await srv.start()
        try:
            await _put(srv, "a", 1)
            for i in range(20):     # a base the delta stays smaller than
                await _put(srv, "pad%d" % i, "x" * 50)
            await srv._checkpoint()
            await _put(srv, "b", 2)
            await _del(srv, "a")
            lsn = srv.ckpt_lsn

            def boom(*a, **kw):
                raise OSError("disk full")
            monkeypatch.setattr(ckptmod, "write_layer", boom)
            await srv._checkpoint()
            monkeypatch.undo()
            assert srv._dirty == {"a", "b"} and srv.ckpt_lsn == lsn
            assert "checkpoint failed" in out.getvalue()
            assert len(_manifest(data)["layers"]) == 1
            await srv._checkpoint()
            assert srv._dirty == set() and srv.ckpt_lsn > lsn
            assert len(_subops(data, _manifest(data)["layers"][1])) == 2
        finally:
            _crash(srv)
    run(go())


# ------------------------------------------------------------ deferred deletion

async def _until_compactions(srv, n, tag):
    i = 0
    while srv._compact_count < n:
        await _put(srv, "k%02d" % (i % 10), "%s%d" % (tag, i) + "x" * 40)
        i += 1
        if i % 5 == 0:
            await srv._checkpoint()
        assert i < 1000


def test_superseded_layers_are_unlinked_one_compaction_late(tmp_path):
    data = str(tmp_path / "n1")
    copy = str(tmp_path / "copy")

    async def go():
        srv = await _start(data, **INCR)
        try:
            for i in range(10):
                await _put(srv, "k%02d" % i, "x" * 40)
            await srv._checkpoint()
            await _until_compactions(srv, 1, "a")
            first_gen = set(_layer_files(data))
            man1 = _manifest(data)
            assert len(man1["layers"]) == 1
            superseded = first_gen - set(man1["layers"])
            assert len(superseded) >= 2, "merged layers must still exist"

            # between compactions layers are only ever added; remember
            # the manifest and state before the checkpoint that compacts
            i = 0
            prev, prev_kv, prev_files = man1, dict(srv.kv), first_gen
            while srv._compact_count < 2:
                await _put(srv, "k%02d" % (i % 10), "b%d" % i + "x" * 40)
                i += 1
                if i % 5 == 0:
                    await srv._checkpoint()
                    if srv._compact_count < 2:
                        assert prev_files <= set(_layer_files(data))
                        prev, prev_kv = _manifest(data), dict(srv.kv)
                        prev_files = set(_layer_files(data))
                assert i < 1000
            assert len(prev["layers"]) > 1
            man2 = _manifest(data)
            now = set(_layer_files(data))
            assert len(man2["layers"]) == 1
            assert not (superseded & now), "first generation must be gone"
            second_gen = now - set(man2["layers"])
            # the merged layers: that manifest's, and the delta the last
            # checkpoint added before it compacted
            assert second_gen > set(prev["layers"])
            assert len(second_gen) == len(prev["layers"]) + 1
            model = dict(srv.kv)
            end = srv.replay_lsn
        finally:
            _crash(srv)

        # a copy whose manifest is one generation behind its files
        shutil.copytree(data, copy)
        with open(os.path.join(copy, CKPT_NAME), "w") as f:
            json.dump(prev, f)
        kv, layers = ckptmod.load_layers(copy, prev)
        assert kv == prev_kv and len(layers) == len(prev["layers"]) > 1
        srv = await _start(copy, **INCR)
        try:
            # WAL tail replay brings it to the model
            assert srv.ckpt_lsn == prev["lsn"] < end
            assert srv.kv == model and srv.replay_lsn == end
            # what that manifest does not name was swept at start-up
            assert set(_layer_files(copy)) == set(prev["layers"])
        finally:
            _crash(srv)
    run(go())


# ---------------------------------------------------------------------- damage

def _damaged_dir(tmp_path):
    """A data dir with a base and one delta; returns (dir, manifest, kv,
    path of the newest layer, its bytes)."""
    data = str(tmp_path / "n1")

    async def go():
        srv = await _start(data, **INCR)
        try:
            for i in range(6):
                await _put(srv, "k%d" % i, "v%d" % i)
            await srv._checkpoint()
            await _put(srv, "k1", "new")
            await _del(srv, "k2")
            await _put(srv, "k9", [1, {"a": None}])
            await srv._checkpoint()
            return dict(srv.kv)
        finally:
            _crash(srv)
    kv = run(go())
    man = _manifest(data)
    path = os.path.join(data, ckptmod.CKPT_DIR, man["layers"][-1])
    with open(path, "rb") as f:
        good = f.read()
    return data, man, kv, path, good


def test_loader_refuses_every_truncation_and_byte_flip(tmp_path):
    data, man, kv, path, good = _damaged_dir(tmp_path)
    assert ckptmod.load_layers(data, man)[0] == kv
    assert len(good) > 100
    for n in range(len(good)):
        with open(path, "wb") as f:
            f.write(good[:n])
        with pytest.raises(CheckpointCorrupt):
            ckptmod.load_layers(data, man)
    for off in range(len(good)):
        bad = bytearray(good)
        bad[off] ^= 0x41
        with open(path, "wb") as f:
            f.write(bad)
        with pytest.raises(CheckpointCorrupt):
            ckptmod.load_layers(data, man)
    os.unlink(path)
    with pytest.raises(CheckpointCorrupt):
        ckptmod.load_layers(data, man)
    # the base alone is just as fatal, and so is a swapped order
    with open(path, "wb") as f:
        f.write(good)
    assert ckptmod.load_layers(data, man)[0] == kv
    with pytest.raises(CheckpointCorrupt):
        ckptmod.load_layers(data, dict(man, layers=man["layers"][::-1]))
    with pytest.raises(CheckpointCorrupt):
        ckptmod.load_layers(data, dict(man, layers=man["layers"][1:]))
    with pytest.raises(CheckpointCorrupt):
        ckptmod.load_layers(data, dict(man, layers=[]))
    # a delta copied under another layer's name disagrees with its header
    other = os.path.join(data, ckptmod.CKPT_DIR,
                         ckptmod.layer_name(man["lsn"] + 7, "delta"))
    shutil.copy(path, other)
    with pytest.raises(CheckpointCorrupt):
        ckptmod.load_layers(data, dict(
            man, lsn=man["lsn"] + 7,
            layers=[man["layers"][0], os.path.basename(other)]))


def test_start_refuses_a_damaged_layer_and_opens_no_listener(tmp_path):
    data, man, kv, path, good = _damaged_dir(tmp_path)

    async def go():
        with open(path, "wb") as f:
            f.write(good[:-3])
        os.unlink(os.path.join(data, "waldb.pid"))   # the last run's
        out = io.StringIO()
        srv = _server(data, log=Logger("t", stream=out), **INCR)
        with pytest.raises(CheckpointCorrupt):
            await srv.start()
        assert srv._server is None and srv._flusher is None
        assert not os.path.exists(os.path.join(data, "waldb.pid"))
        assert srv.kv == {}
        errors = [json.loads(line) for line in out.getvalue().splitlines()]
        assert [e for e in errors if e["level"] >= 50
                and "checkpoint layer corrupt" in e["msg"]]
        # the configured mode does not matter: what is on disk decides
        srv = _server(data)
        with pytest.raises(CheckpointCorrupt):
            await srv.start()
        assert srv._server is None

        # an unknown format refuses too, with its own exception
        with open(path, "wb") as f:
            f.write(good)
        with open(os.path.join(data, CKPT_NAME), "w") as f:
            json.dump(dict(man, format=3), f)
        srv = _server(data, **INCR)
        with pytest.raises(CheckpointFormatError):
            await srv.start()
        assert srv._server is None
    run(go())


def test_start_sweeps_tmp_and_unreferenced_files(tmp_path):
    data, man, kv, path, good = _damaged_dir(tmp_path)
    ckpt_dir = os.path.join(data, ckptmod.CKPT_DIR)
    strays = ["%016x.delta.tmp" % 5, "%016x.base" % 3, "%016x.delta" % 4,
              "notes.txt"]
    for name in strays:
        with open(os.path.join(ckpt_dir, name), "wb") as f:
            f.write(b"junk that would fail every check")

    async def go():
        srv = await _start(data, **INCR)
        try:
            assert srv.kv == kv
            assert _layer_files(data) == sorted(man["layers"])
        finally:
            _crash(srv)
    run(go())


# --------------------------------------------------------------- mode switching

def test_switching_modes_and_back(tmp_path):
    data = str(tmp_path / "n1")

    async def go():
        model = {}

        async def write(srv, tag, n=20):
            for i in range(n):
                model["k%02d" % i] = tag
                await _put(srv, "k%02d" % i, tag)

        srv = await _start(data)                     # full
        try:
            assert srv.settings.ckpt_mode == "full"
            await write(srv, "full-1")
            await srv._checkpoint()
            assert "kv" in _manifest(data) and _layer_files(data) == []
        finally:
            _crash(srv)

        srv = await _start(data, **INCR)             # classic image loads
        try:
            assert srv.kv == model and srv._layers == []
            await write(srv, "incr-1", 5)
            await srv._checkpoint()                  # first: a base
            man = _manifest(data)
            assert "kv" not in man and len(man["layers"]) == 1
            assert len(_subops(data, man["layers"][0])) == len(model)
            model.pop("k07")
            await _del(srv, "k07")
            await srv._checkpoint()
            assert len(_manifest(data)["layers"]) == 2
        finally:
            _crash(srv)

        srv = await _start(data)                     # layers load under full
        try:
            assert srv.kv == model and len(srv._layers) == 2
            layers = _layer_files(data)
            await write(srv, "full-2", 3)
            await srv._checkpoint()
            man = _manifest(data)
            assert man["kv"] == model and "format" not in man
            assert sorted(man) == ["kv", "lsn"]
            # deferred: still there after the superseding image ...
            assert _layer_files(data) == layers
            await write(srv, "full-3", 3)
            await srv._checkpoint()
            # ... gone after the next
            assert _layer_files(data) == []
            assert srv._layers == [] and srv._ckpt_garbage == []
        finally:
            _crash(srv)

        srv = await _start(data, **INCR)
        try:
            assert srv.kv == model
            # a reload adopts the mode for the NEXT checkpoint
            _server(data)
            srv._on_sighup()
            assert srv.settings.ckpt_mode == "full"
            await srv._checkpoint()
            assert "kv" in _manifest(data)
            _server(data, **INCR)
            srv._on_sighup()
            assert srv.settings.ckpt_mode == "incremental"
            await srv._checkpoint()
            assert _manifest(data)["format"] == 2
        finally:
            _crash(srv)

        srv = await _start(data)
        try:
            assert srv.kv == model
        finally:
            _crash(srv)
    run(go())


# ---------------------------------------------------------------------- spacing

def test_incremental_checkpoints_are_due_at_checkpoint_wal_bytes(tmp_path):
    data = str(tmp_path / "n1")

    async def go():
        srv = await _start(data, checkpoint_wal_bytes="4096", **INCR)
        try:
            srv._ckpt_running = True        # hold the flush loop off
            for i in range(300):
                await _put(srv, "k%03d" % i, "x" * 100)
            await srv._checkpoint()
            first = srv.ckpt_lsn
            base = srv._layers[0]["bytes"]
            assert base > 2 * 4096
            assert srv._ckpt_due_bytes() == 4096
            # full mode on the same state would wait for half the image
            full = Settings(ckpt_mode="full", ckpt_wal_bytes=4096)
            srv._last_ckpt_bytes, saved = base, srv._last_ckpt_bytes
            srv.settings, incr = full, srv.settings
            assert srv._ckpt_due_bytes() == base // 2 > 4096
            srv.settings, srv._last_ckpt_bytes = incr, saved

            srv._ckpt_running = True
            while srv.replay_lsn - first < 4096:
                await _put(srv, "k000", "y" * 100)
            assert srv.replay_lsn - first < base // 2
            assert srv.ckpt_lsn == first
            srv._ckpt_running = False       # the flush loop's own decision
            deadline = asyncio.get_running_loop().time() + 10
            while srv.ckpt_lsn == first or srv._ckpt_running:
                assert asyncio.get_running_loop().time() < deadline, \
                    "the flush loop never started the due checkpoint"
                await asyncio.sleep(0.01)
            man = _manifest(data)
            assert len(man["layers"]) == 2
            assert len(_subops(data, man["layers"][1])) == 1
        finally:
            _crash(srv)
    run(go())


# ------------------------------------------------------------------------ knobs

def test_checkpoint_mode_knob_in_both_front_ends(tmp_path):
    from tests.test_waldb_core import _minipg, _waldb
    assert Settings().ckpt_mode == "full"
    for front in (_waldb, _minipg):
        assert front(tmp_path).read_settings(Settings()).ckpt_mode == "full"
        s = front(tmp_path, checkpoint_mode="incremental") \
            .read_settings(Settings())
        assert s.ckpt_mode == "incremental"
        s = front(tmp_path, checkpoint_mode="'incremental'") \
            .read_settings(Settings())
        assert s.ckpt_mode == "incremental"
    # a bad value is unparsable: the pass ends there, earlier knobs hold
    prev = Settings(ckpt_wal_bytes=11, wal_keep_bytes=22,
                    ckpt_mode="incremental")
    got = parse_knobs({"checkpoint_wal_bytes": "1000",
                       "checkpoint_mode": "sometimes"}, prev, 1.0)
    assert (got.ckpt_wal_bytes, got.wal_keep_bytes, got.ckpt_mode) == \
        (1000, 22, "incremental")
    # ... and a bad knob before it keeps the mode from being applied
    got = parse_knobs({"wal_keep_bytes": "lots",
                       "checkpoint_mode": "full"}, prev, 1.0)
    assert (got.wal_keep_bytes, got.ckpt_mode) == (22, "incremental")
    # minipg keeps the previous value for an absent or bad knob
    assert _minipg(tmp_path).read_settings(prev).ckpt_mode == "incremental"
    assert _minipg(tmp_path, checkpoint_mode="never") \
        .read_settings(prev).ckpt_mode == "incremental"
    # waldb.conf is regenerated whole: absent means the default
    assert _waldb(tmp_path).read_settings(prev).ckpt_mode == "full"


# --------------------------------------------------------------------- plumbing

def _conf(data) -> dict:
    return confparser.read(os.path.join(data, "waldb.conf"))


def test_engine_tunables_reach_every_regenerated_conf(tmp_path):
    data = str(tmp_path / "data")
    os.makedirs(data)
    eng = WaldbEngine(data, "127.0.0.1", 5000, "peer1",
                      tunables={"checkpoint_mode": "incremental",
                                "checkpoint_wal_bytes": 4096})
    eng.write_conf("primary", sync_name="peer2")
    conf = _conf(data)
    assert conf["checkpoint_mode"] == "incremental"
    assert conf["checkpoint_wal_bytes"] == "4096"
    assert conf["role"] == "primary"
    eng.write_conf("standby", upstream_url="tcp://postgres@10.0.0.1:5432/p")
    assert _conf(data)["checkpoint_mode"] == "incremental"
    # a restore brings the SOURCE peer's conf; the fixup deletes it and
    # the regenerated one carries the tunables again
    confparser.write(os.path.join(data, "waldb.conf"),
                     {"role": "primary", "port": "1"})
    eng.post_restore_fixup()
    assert not os.path.exists(os.path.join(data, "waldb.conf"))
    eng.write_conf("standby", upstream_url="tcp://postgres@10.0.0.1:5432/p")
    conf = _conf(data)
    assert conf["checkpoint_mode"] == "incremental"
    assert conf["port"] == "5000"
    # the server reads what the engine wrote
    init_data_dir(data)
    s = WaldbServer(data, null_logger()).read_settings(Settings())
    assert (s.ckpt_mode, s.ckpt_wal_bytes) == ("incremental", 4096)
    # no tunables: the conf is what it always was
    plain = WaldbEngine(data, "127.0.0.1", 5000, "peer1")
    plain.write_conf("primary")
    assert "checkpoint_mode" not in _conf(data)

    with pytest.raises(ValueError):
        WaldbEngine(data, "127.0.0.1", 5000, "peer1",
                    tunables={"checkpoint_mod": "incremental"})
    with pytest.raises(ValueError):
        WaldbEngine(data, "127.0.0.1", 5000, "peer1",
                    tunables={"role": "primary"})


def test_build_engine_passes_waldb_tunables(tmp_path):
    from manatee_amd.shard import build_engine
    from manatee_amd.tools.devcluster import DevCluster
    eng = build_engine({"engine": "waldb",
                        "waldbTunables": {"checkpoint_mode": "incremental"}},
                       "127.0.0.1", 5000, "p", str(tmp_path), null_logger())
    assert eng.tunables == {"checkpoint_mode": "incremental"}
    assert build_engine({}, "127.0.0.1", 5000, "p", str(tmp_path),
                        null_logger()).tunables == {}
    with pytest.raises(ValueError):
        build_engine({"waldbTunables": {"nope": 1}}, "127.0.0.1", 5000,
                     "p", str(tmp_path), null_logger())
    c = DevCluster(str(tmp_path / "c"), n_peers=1,
                   waldb_tunables={"checkpoint_mode": "incremental"})
    assert c.peers[0].sitter_config()["postgresMgrCfg"]["waldbTunables"] \
        == {"checkpoint_mode": "incremental"}
    c = DevCluster(str(tmp_path / "d"), n_peers=1)
    assert "waldbTunables" not in c.peers[0].sitter_config()["postgresMgrCfg"]


# ------------------------------------------------------------------- ckpt query

def test_ckpt_query_and_client_method(tmp_path):
    data = str(tmp_path / "n1")

    async def go():
        srv = await _start(data, **INCR)
        cli = None
        try:
            with open(os.path.join(data, "waldb.pid")) as f:
                port = int(f.read().split()[1])
            cli = WaldbClient("127.0.0.1", port)
            info = await cli.checkpoint_info()
            assert info == {"ok": True, "mode": "incremental",
                            "lsn": "0/00000000", "layers": [],
                            "dirty_keys": 0, "last_checkpoint_bytes": 0,
                            "last_checkpoint_dirty": 0,
                            "last_checkpoint_records": 0,
                            "checkpoints": 0, "compactions": 0}
            for i in range(10):
                await cli.put("k%d" % i, "x" * 50)
            assert (await cli.checkpoint_info())["dirty_keys"] == 10
            await srv._checkpoint()
            await cli.put("k3", "y")
            await cli.delete("k4")
            await cli.put("extra", 1)
            await srv._checkpoint()
            await cli.put("k5", "z")
            info = await cli.query({"q": "ckpt"})
            assert info == await cli.checkpoint_info()
            status = await cli.status()
            assert info["lsn"] == status["checkpoint_lsn"]
            assert (info["checkpoints"], info["compactions"]) == (2, 0)
            assert info["dirty_keys"] == 1
            assert (info["last_checkpoint_dirty"],
                    info["last_checkpoint_records"]) == (3, 3)
            man = _manifest(data)
            assert [layer["name"] for layer in info["layers"]] == \
                man["layers"]
            assert [(layer["kind"], layer["records"])
                    for layer in info["layers"]] == [("base", 10),
                                                     ("delta", 3)]
            for layer in info["layers"]:
                assert layer["bytes"] == os.path.getsize(
                    os.path.join(data, ckptmod.CKPT_DIR, layer["name"]))
            assert info["layers"][1]["lsn"] == info["lsn"]
            assert info["last_checkpoint_bytes"] == \
                info["layers"][1]["bytes"] + os.path.getsize(
                    os.path.join(data, CKPT_NAME))
            # the pinned status reply gained no field
            assert "layers" not in status and "dirty_keys" not in status
        finally:
            if cli is not None:
                await cli.close()
            _crash(srv)
    run(go())


def test_layer_frames_are_wal_frames(tmp_path):
    """A layer is readable with the WAL's own scanner and op decoder."""
    from manatee_amd.db.waldb.wal import _scan
    info = ckptmod.write_layer(str(tmp_path), "delta", 77, 33,
                               [("a", 1), ("b", ckptmod.TOMBSTONE)], 2)
    assert info == {"name": "%016x.delta" % 77, "kind": "delta", "lsn": 77,
                    "bytes": info["bytes"], "records": 2}
    assert os.listdir(str(tmp_path)) == [info["name"]]      # no *.tmp left
    with open(os.path.join(str(tmp_path), info["name"]), "rb") as f:
        buf = f.read()
    valid, records = _scan(buf)
    assert valid == len(buf) == info["bytes"]
    frames = [decode_op(buf[o:o + n]) for o, n in records]
    assert frames == [
        {"ckpt": "header", "kind": "delta", "lsn": 77, "parent": 33,
         "count": 2},
        {"op": "batch", "ops": [{"op": "put", "k": "a", "v": 1},
                                {"op": "del", "k": "b"}]},
        {"ckpt": "trailer", "count": 2}]
