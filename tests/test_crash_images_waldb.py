"""Crash images of a waldb data directory (tests/crashfs.py).

A ``WaldbServer`` is driven in-process while every file operation under
its data directory is recorded.  From the trace every directory a
``kill -9`` or a power loss could have left is rebuilt, recovered with
``WaldbServer.start()`` and held against the model:

1. ``start()`` succeeds;
2. ``replay_lsn`` is the LSN of some write and ``kv`` is the model's
   state at that LSN (prefix consistency: batches whole, nothing
   resurrected);
3. ``wal.end == replay_lsn >= ckpt_lsn``;
4. ``replay_lsn`` is at least the floor — under ``process`` the last
   write whose ``pwrite`` returned, under ``powerloss`` the last write
   before the most recent WAL fsync;
5. one more put and a second restart still equal the model.

Every scenario first passes the recorder's self-check and asserts that
its trace holds the operations the images are about (a roll, a
``drop_below``, layers, compactions, ...), so none passes emptily.  The
seeded-fault tests at the end break one ordering rule at a time and
expect the same checker to object.
"""

import asyncio
import collections
import json
import os
import random
import re

import pytest

from manatee_amd.common import confparser
from manatee_amd.common.logging import null_logger
from manatee_amd.db.waldb import ckpt as ckptmod
from manatee_amd.db.waldb import core as coremod
from manatee_amd.db.waldb.server import (CKPT_NAME, PROMOTE_TRIGGER,
                                         WaldbServer, init_data_dir)
from manatee_amd.db.waldb.wal import LEGACY_NAME, Wal
from tests import crashfs

SMALL = {"wal_segment_bytes": "1024", "wal_keep_bytes": "512"}
FULL = dict(SMALL)
INCR = dict(SMALL, checkpoint_mode="incremental")
KEYS = ["key%02d" % i for i in range(12)]
SEG_RE = re.compile(r"^wal-([0-9a-f]{16})\.seg$")


def run(coro, timeout=120):
    return asyncio.run(asyncio.wait_for(coro, timeout))


def _write_conf(data, conf, durably=True):
    """``durably``: the way the manager regenerates the conf, fsync and
    all.  The thousands of images being recovered do without."""
    base = {"role": "primary", "listen_ip": "127.0.0.1", "port": "0",
            "name": "n1"}
    base.update(conf)
    path = os.path.join(data, "waldb.conf")
    if durably:
        confparser.write(path, base)
    else:
        with open(path, "w") as f:
            f.write(confparser.dump_string(base))


def _crash(srv):
    """Abandon the server object, as tests/test_waldb_ickpt.py does."""
    if srv._server is not None:
        srv._server.close()
    if srv._flusher is not None:
        srv._flusher.cancel()
    srv.wal.close()


async def _start(data, conf, durably=True):
    """Start a server whose WAL is fsynced only where the test says so:
    the 50 ms flush loop is stopped, ``Workload.fsync`` stands in."""
    _write_conf(data, conf, durably)
    srv = WaldbServer(data, null_logger())
    try:
        await srv.start()
    except BaseException:
        _crash(srv)
        raise
    srv._flusher.cancel()
    return srv


class Workload:
    """Random puts, deletes and batches over a dozen keys, with the
    model's state remembered at every LSN."""

    def __init__(self, data, rec, seed):
        self.data, self.rec = data, rec
        self.rng = random.Random(seed)
        self.kv = {}
        self.model = {0: {}}
        self.srv = None
        self.writes = 0
        self.compactions = 0

    async def start(self, conf):
        self.srv = await _start(self.data, conf)
        assert self.srv.kv == self.kv

    def crash(self):
        self.compactions += self.srv._compact_count
        _crash(self.srv)
        self.srv = None

    def _op(self):
        rng, n = self.rng, self.writes
        r = rng.random()
        if r < 0.55:
            return {"op": "put", "k": rng.choice(KEYS),
                    "v": "v%d-%s" % (n, "p" * rng.randrange(60))}
        if r < 0.8:
            return {"op": "del", "k": rng.choice(KEYS)}
        ops = []
        for _ in range(rng.randrange(1, 6)):
            if rng.random() < 0.6:
                ops.append({"op": "put", "k": rng.choice(KEYS),
                            "v": "b%d" % n})
            else:
                ops.append({"op": "del", "k": rng.choice(KEYS)})
        return {"op": "batch", "ops": ops}

    async def write(self, group=1):
        """``group`` records, then ONE flush of the WAL buffer (group
        commit) and a mark."""
        for _ in range(group):
            op = self._op()
            ckptmod.apply_op(self.kv, op)
            assert (await self.srv._do_write(op))["ok"]
            self.model[self.srv.replay_lsn] = dict(self.kv)
            self.writes += 1
        self.srv.wal.flush_buffer()
        self.rec.mark(("lsn", self.srv.replay_lsn))

    def fsync(self):
        """What the flush loop does every 50 ms."""
        self.srv.wal.fsync()

    async def checkpoint(self):
        self.rec.mark(("ckpt",))
        await self.srv._checkpoint()
        # _checkpoint logs a failure and carries on; here it is one
        assert self.srv.ckpt_lsn == self.srv.replay_lsn

    async def steps(self, n, ckpt_every=9):
        for i in range(n):
            await self.write(group=3 if i % 11 == 10 else 1)
            if i % 7 == 6:
                self.fsync()
            if i % ckpt_every == ckpt_every - 1:
                await self.checkpoint()


def coverage(ops):
    """What a trace exercised, by counting its operations."""
    c = collections.Counter()
    unsynced = False
    for op in ops:
        kind, path = op[0], op[1]
        seg = SEG_RE.match(path) if isinstance(path, str) else None
        if kind == "create" and seg and int(seg.group(1), 16) > 0:
            c["roll"] += 1
        elif kind == "unlink" and seg:
            c["drop_below"] += 1
        elif kind == "rename" and op[2].startswith("ckpt" + os.sep):
            c["layer"] += 1
            c[op[2].rsplit(".", 1)[1]] += 1
        elif kind == "unlink" and path.startswith("ckpt" + os.sep) \
                and not path.endswith(".tmp"):
            c["layer_unlink"] += 1
        elif kind == "pwrite" and seg:
            unsynced = True
        elif kind == "fsync" and seg:
            unsynced = False
        elif kind == "mark" and path == ("ckpt",) and unsynced:
            c["ckpt_over_unsynced_wal"] += 1
    return c


# ------------------------------------------------------------------ scenarios

async def _full(w):
    await w.start(FULL)
    await w.steps(150)
    w.crash()


async def _incremental(w):
    await w.start(INCR)
    await w.steps(160)
    w.crash()


async def _switch(w):
    await w.start(FULL)
    await w.steps(40)
    w.crash()
    await w.start(INCR)
    await w.steps(70)
    w.crash()
    await w.start(FULL)             # the image supersedes the layers,
    await w.steps(40)               # which go one checkpoint later
    w.crash()


async def _promote(w):
    """The trigger is there before the first start (``record`` puts it
    into the starting image): ``_bump_timeline`` saves the identity,
    then unlinks it."""
    await w.start(FULL)
    assert w.srv.timeline == 2
    await w.steps(45)
    w.crash()


SCENARIOS = {
    # name: (workload, conf to recover with, needs layers)
    "full": (_full, FULL, False),
    "incremental": (_incremental, INCR, True),
    "switch": (_switch, INCR, True),
    "promote": (_promote, FULL, False),
}
_TRACES = {}


def record(data, body, seed=20250611):
    """Run ``body(workload)`` on a fresh data directory under the
    recorder; self-check; returns ``(recorder, workload)``."""
    init_data_dir(data)
    _write_conf(data, FULL)
    if body is _promote:
        with open(os.path.join(data, PROMOTE_TRIGGER), "w"):
            pass
    big = []
    real_merge = ckptmod.merge_layers_offloaded

    def merge(data_dir, names):
        # a merge in a child process would write behind the recorder
        size = sum(os.path.getsize(os.path.join(data_dir, ckptmod.CKPT_DIR,
                                                n)) for n in names)
        if size >= ckptmod.MERGE_IN_CHILD_BYTES:
            big.append(size)
        return real_merge(data_dir, names)

    with crashfs.Recorder(data) as rec:
        w = Workload(data, rec, seed)
        ckptmod.merge_layers_offloaded = merge
        try:
            run(body(w))
        finally:
            ckptmod.merge_layers_offloaded = real_merge
            if w.srv is not None:
                w.crash()
    assert not big, "layers reached MERGE_IN_CHILD_BYTES: %r" % big
    rec.verify()
    return rec, w


def scenario(name, tmp_path_factory):
    """The recorded trace of one scenario (run once per session), with
    its coverage conditions asserted."""
    if name not in _TRACES:
        body, conf, layered = SCENARIOS[name]
        data = str(tmp_path_factory.mktemp("crash-" + name) / "n1")
        rec, w = record(data, body)
        c = coverage(rec.ops)
        assert c["roll"] >= 1 and c["drop_below"] >= 1, c
        assert c["ckpt_over_unsynced_wal"] >= 1, c
        if layered:
            assert c["layer"] >= 1 and c["layer_unlink"] >= 1, c
        if name == "incremental":
            assert c["delta"] >= 1 and c["base"] >= 3, c
            assert w.compactions >= 2, w.compactions
        if name == "promote":
            assert ("unlink", PROMOTE_TRIGGER) in rec.ops
        _TRACES[name] = (rec, w, conf)
    return _TRACES[name]


# -------------------------------------------------------------------- checker

def process_floor(ops, i):
    """LSN of the last write whose pwrite returned before crash point i."""
    for op in reversed(ops[:i]):
        if op[0] == "mark" and op[1][0] == "lsn":
            return op[1][1]
    return 0


def powerloss_floor(ops, i):
    """LSN of the last write before the most recent WAL fsync."""
    synced = False
    for op in reversed(ops[:i]):
        if op[0] == "fsync" and SEG_RE.match(op[1]):
            synced = True
        elif synced and op[0] == "mark" and op[1][0] == "lsn":
            return op[1][1]
    return 0


async def recover_image(img, model, conf, dest, promoted=False):
    """Recover one image in ``dest``; returns ``(replay_lsn, broken
    invariants)`` — all but the floor, which depends on the crash point
    and not on the bytes."""
    img.materialize(dest)
    try:
        srv = await _start(dest, conf, durably=False)
    except Exception as exc:
        return None, ["1: start() raised %s: %s" % (type(exc).__name__, exc)]
    bad = []
    try:
        lsn = srv.replay_lsn
        if lsn not in model:
            bad.append("2: replay_lsn %d is no write's LSN" % lsn)
        elif srv.kv != model[lsn]:
            bad.append("2: kv at %d is not the model's" % lsn)
        if not srv.wal.end == srv.replay_lsn >= srv.ckpt_lsn:
            bad.append("3: wal.end %d, replay_lsn %d, ckpt_lsn %d"
                       % (srv.wal.end, srv.replay_lsn, srv.ckpt_lsn))
        tls = [h["tl"] for h in srv.history]
        ats = [h["at"] for h in srv.history]
        if tls != sorted(set(tls)) or ats != sorted(ats) \
                or srv.timeline != tls[-1] or ats[-1] > lsn:
            bad.append("timeline %d with history %r at %d"
                       % (srv.timeline, srv.history, lsn))
        if promoted and (srv.timeline not in (2, 3) or os.path.exists(
                os.path.join(dest, PROMOTE_TRIGGER))):
            bad.append("promote trigger not consumed once: timeline %d"
                       % srv.timeline)
        want = dict(srv.kv, **{"after-crash": lsn})
        assert (await srv._do_write({"op": "put", "k": "after-crash",
                                     "v": lsn}))["ok"]
        end = srv.replay_lsn
        timeline = srv.timeline
    finally:
        _crash(srv)
    try:
        srv = await _start(dest, conf, durably=False)
    except Exception as exc:
        return lsn, bad + ["5: restart raised %s: %s"
                           % (type(exc).__name__, exc)]
    try:
        if srv.kv != want or srv.replay_lsn != end or srv.wal.end != end \
                or srv.timeline != timeline:
            bad.append("5: after one more put and a restart: replay_lsn "
                       "%d for %d" % (srv.replay_lsn, end))
    finally:
        _crash(srv)
    return lsn, bad


def check_images(images, floor_of, ops, model, conf, dest, promoted=False,
                 stop_after=None):
    """Check every image; returns ``(images checked, violations)``.  The
    same bytes at a later crash point are not recovered twice: only the
    floor is held against the earlier result again."""
    async def go():
        count, violations, known = 0, [], {}
        for i, img in images:
            count += 1
            fp = img.fingerprint()
            if fp not in known:
                known[fp] = await recover_image(img, model, conf, dest,
                                                promoted)
            lsn, bad = known[fp]
            floor = floor_of(ops, i)
            if lsn is not None and lsn < floor:
                bad = bad + ["4: replay_lsn %d below the floor %d"
                             % (lsn, floor)]
            violations += ["%s: %s" % (img.label, what) for what in bad]
            if stop_after and len(violations) >= stop_after:
                break
        return count, violations
    return run(go())


def _images(rec, model_name):
    if model_name == "process":
        return crashfs.process_images(rec.start, rec.ops), process_floor
    return (crashfs.powerloss_images(rec.start, rec.ops,
                                     model_name == "powerloss-journalled"),
            powerloss_floor)


MODELS = ["process", "powerloss-journalled", "powerloss-strict"]


@pytest.mark.parametrize("model_name", MODELS)
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_every_crash_image_recovers_to_the_model(name, model_name, tmp_path,
                                                 tmp_path_factory):
    rec, w, conf = scenario(name, tmp_path_factory)
    images, floor_of = _images(rec, model_name)
    count, violations = check_images(
        images, floor_of, rec.ops, w.model, conf, str(tmp_path / "img"),
        promoted=name == "promote")
    print("%s/%s: %d operations, %d images, %d violations"
          % (name, model_name, len(rec.ops), count, len(violations)))
    assert count > len(crashfs.powerloss_points(rec.ops)) // 2
    assert not violations, "%d of %d images:\n%s" % (
        len(violations), count, "\n".join(violations[:20]))


def test_process_images_with_the_python_codec(tmp_path, monkeypatch):
    """The same check with ``wal._scan``'s fallback instead of the
    native scanner."""
    import manatee_amd.native
    monkeypatch.setattr(manatee_amd.native, "codec", None)
    rec, w = record(str(tmp_path / "n1"), _promote)
    count, violations = check_images(
        crashfs.process_images(rec.start, rec.ops), process_floor, rec.ops,
        w.model, FULL, str(tmp_path / "img"), promoted=True)
    assert count > 100 and not violations, violations[:20]


# ------------------------------------------------------ crash during recovery

def _unreferenced(img):
    try:
        named = json.loads(img.files[CKPT_NAME]).get("layers", [])
    except (KeyError, ValueError):
        named = []
    return [p for p in img.files if p.startswith("ckpt" + os.sep)
            and os.path.basename(p) not in named]


PICKS = 6


def _mutating_recoveries(rec):
    """Images of the incremental trace whose recovery itself changes the
    directory, ``{kind: [(crash point, image), ...]}``: a torn tail that
    ``Wal.open`` cuts, files in ``ckpt/`` that the start-up sweep
    removes, and the single-file WAL of before segmentation.  There are
    hundreds of the first two; ``PICKS`` of each, spread evenly over the
    trace (the first and the last among them), stand for them."""
    found = collections.defaultdict(list)
    for i, img in crashfs.process_images(rec.start, rec.ops):
        if "bytes of the write to wal-" in img.label:
            found["ftruncate"].append((i, img))
        if _unreferenced(img):
            found["sweep"].append((i, img))
        segs = [p for p in img.files if SEG_RE.match(p)]
        if segs == ["wal-%016x.seg" % 0] and len(img.files[segs[0]]) > 300:
            # the single-file layout of before segmentation
            img = crashfs.Image(img.dirs, img.files,
                                img.label + ", as legacy wal.log")
            img.files[LEGACY_NAME] = img.files.pop(segs[0])
            found["legacy"].append((i, img))
    return {kind: [imgs[k * (len(imgs) - 1) // (PICKS - 1)]
                   for k in range(PICKS)] if len(imgs) > PICKS else imgs
            for kind, imgs in found.items()}


def test_crash_during_recovery_of_incremental_images(tmp_path,
                                                     tmp_path_factory):
    rec, w, conf = scenario("incremental", tmp_path_factory)
    chosen = _mutating_recoveries(rec)
    assert sorted(chosen) == ["ftruncate", "legacy", "sweep"]
    expect = {"ftruncate": lambda op: op[0] == "truncate"
              and SEG_RE.match(op[1]),
              "sweep": lambda op: op[0] == "unlink"
              and op[1].startswith("ckpt" + os.sep),
              "legacy": lambda op: op[:2] == ("rename", LEGACY_NAME)}
    total = 0
    for kind, picks in sorted(chosen.items()):
        for i, img in picks:
            floor = process_floor(rec.ops, i)
            data = str(tmp_path / "recovering")
            img.materialize(data)
            _write_conf(data, conf)
            with crashfs.Recorder(data) as inner:
                async def recover():
                    _crash(await _start(data, conf))
                run(recover())
            inner.verify()
            assert any(expect[kind](op) for op in inner.ops), \
                (kind, img.label, inner.ops)
            for images in (
                    crashfs.process_images(inner.start, inner.ops),
                    crashfs.powerloss_images(inner.start, inner.ops, False)):
                count, violations = check_images(
                    images, lambda ops, j: floor, inner.ops, w.model, conf,
                    str(tmp_path / "img"))
                total += count
                assert not violations, "recovery of [%s]:\n%s" % (
                    img.label, "\n".join(violations[:20]))
    print("crash during recovery: %d recoveries recorded, %d images"
          % (sum(len(p) for p in chosen.values()), total))
    assert total > 200


# --------------------------------------------------------------- seeded faults
#
# One ordering rule broken at a time, on a short trace: the checker must
# find an image that violates an invariant, or it proves nothing above.

async def _short_incremental(w):
    await w.start(INCR)
    await w.steps(42, ckpt_every=6)
    w.crash()


def _violations(tmp_path, *model_names):
    rec, w = record(str(tmp_path / "n1"), _short_incremental)
    assert w.compactions >= 2
    found = []
    for model_name in model_names:
        images, floor_of = _images(rec, model_name)
        _count, violations = check_images(images, floor_of, rec.ops, w.model,
                                          INCR, str(tmp_path / "img"),
                                          stop_after=3)
        found.append(violations)
    return found


def test_the_short_trace_is_clean_without_a_fault(tmp_path):
    assert _violations(tmp_path, *MODELS) == [[], [], []]


def test_seeded_layer_directory_never_fsynced(tmp_path, monkeypatch):
    monkeypatch.setattr(ckptmod, "_fsync_dir", lambda path: None)
    violations, = _violations(tmp_path, "powerloss-strict")
    assert any("CheckpointCorrupt" in v for v in violations), violations


def test_seeded_manifest_published_before_its_layer(tmp_path, monkeypatch):
    """``write_layer`` holds its rename back until the manifest that
    names the layer has been published."""
    held = []
    real_layer, real_json = ckptmod.write_layer, coremod._write_json_atomic

    def write_layer(ckpt_dir, kind, lsn, *rest):
        layer = real_layer(ckpt_dir, kind, lsn, *rest)
        path = os.path.join(ckpt_dir, layer["name"])
        os.rename(path, path + ".held")
        held.append(path)
        return layer

    def write_json_atomic(path, obj, **kw):
        size = real_json(path, obj, **kw)
        while held:
            os.rename(held[-1] + ".held", held.pop())
        return size

    monkeypatch.setattr(ckptmod, "write_layer", write_layer)
    monkeypatch.setattr(coremod, "_write_json_atomic", write_json_atomic)
    violations, = _violations(tmp_path, "process")
    assert any("CheckpointCorrupt" in v for v in violations), violations


def test_seeded_checkpoint_without_the_wal_fsync(tmp_path, monkeypatch):
    """``Wal.fsync`` does nothing while ``_checkpoint`` runs: the image
    can be ahead of the durable WAL."""
    in_ckpt = []
    real_fsync, real_ckpt = Wal.fsync, WaldbServer._checkpoint

    def fsync(self):
        if in_ckpt:
            self.flush_buffer()
        else:
            real_fsync(self)

    async def checkpoint(self):
        in_ckpt.append(1)
        try:
            await real_ckpt(self)
        finally:
            in_ckpt.pop()

    monkeypatch.setattr(Wal, "fsync", fsync)
    monkeypatch.setattr(WaldbServer, "_checkpoint", checkpoint)
    for violations in _violations(tmp_path, *MODELS[1:]):
        assert any(": 3: " in v for v in violations), violations


def test_seeded_layers_unlinked_before_the_manifest_is_durable(tmp_path,
                                                               monkeypatch):
    """Superseded layers go at once instead of one generation late, and
    the manifest's rename is not made durable first."""
    def retire(self, superseded):
        live = {layer["name"] for layer in self._layers}
        ckptmod.unlink_layers(self.data_dir,
                              [n for n in superseded if n not in live])

    monkeypatch.setattr(WaldbServer, "_retire_layers", retire)
    monkeypatch.setattr(coremod, "_fsync_dir", lambda path: None)
    violations, = _violations(tmp_path, "powerloss-strict")
    assert any("CheckpointCorrupt" in v for v in violations), violations
