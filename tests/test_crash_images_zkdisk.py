"""Crash images of a quorum member's data directory (tests/crashfs.py):
``zkquorum.MemberDisk`` is driven through votes, appends (the cut of a
deposed suffix included), snapshots and ``load()``'s own rewrite, and
every image a ``kill -9`` or a power loss could leave is loaded again.

After ``load()`` of any image:

* ``epoch`` and ``voted_for`` are those of the last ``save_meta`` that
  returned, or of the one in flight — never older: a forgotten vote is
  a double vote;
* the entries are contiguous from ``base_index + 1``, a prefix of what
  was appended, and include every entry whose ``append`` returned;
* the snapshot is the last one saved or the one in flight, and its
  index never exceeds what was ever appended.

This class fsyncs its directory after every rename, so the strict
power-loss model holds as well as the journalled one.
"""

import json
import os

import pytest

from manatee_amd.common.logging import null_logger
from manatee_amd.coord.zkquorum import MemberDisk
from tests import crashfs


class Driver:
    """Calls bracketed by marks, from which ``expected_at`` rebuilds
    what the disk had promised at a crash point."""

    def __init__(self, d, rec):
        self.d, self.rec = d, rec
        self.disk = MemberDisk(d, null_logger())

    def _call(self, what, fn, *args):
        self.rec.mark((what, "begin") + args)
        fn(*args)
        self.rec.mark((what, "done") + args)

    def load(self):
        self._call("load", lambda: self.disk.load())

    def reopen(self):
        self.disk.close()
        self.disk = MemberDisk(self.d, null_logger())
        self.load()

    def meta(self, epoch, voted_for):
        self._call("meta", self.disk.save_meta, epoch, voted_for)

    def append(self, start, entries):
        self._call("append", self.disk.append, start, entries)

    def snapshot(self, index, epoch, remaining):
        self._call("snapshot", lambda i, e, r: self.disk.save_snapshot(
            {"index": i, "epoch": e, "tree": {"n": i}}, r),
            index, epoch, remaining)


def entry(epoch, n):
    return (epoch, {"op": "set", "path": "/n%d" % n, "data": "x" * n})


def workload(d):
    d.load()                                        # an empty directory
    d.meta(1, 2)
    d.append(1, [entry(1, 1), entry(1, 2), entry(1, 3)])
    d.meta(2, None)
    d.meta(2, 3)
    d.append(4, [entry(2, 4), entry(2, 5)])
    # a new leader overwrites from index 3: the deposed suffix is cut
    d.append(3, [entry(3, 13), entry(3, 14)])
    d.snapshot(2, 1, [entry(3, 13), entry(3, 14)])
    d.append(5, [entry(3, 15)])
    d.meta(4, 1)
    d.reopen()                                      # load()'s own _rewrite
    d.append(6, [entry(4, 16)])
    d.snapshot(6, 4, [])
    d.append(7, [entry(4, 17), entry(4, 18)])
    d.meta(5, None)
    d.disk.close()


def expected_at(ops, i):
    """What the calls before crash point ``i`` promised: the meta, log
    and snapshot index of the calls that returned, and of a call in
    flight (else None)."""
    done = {"meta": (0, None), "log": [], "snapshot": 0}
    flying = {"meta": None, "log": None, "snapshot": None, "cut": None}
    ever = 0
    for op in ops[:i]:
        if op[0] != "mark":
            continue
        what, phase = op[1][:2]
        args = op[1][2:]
        if what == "meta":
            new = tuple(args)
        elif what == "append":
            start, entries = args
            new = done["log"][:start - 1] + [list(e) for e in entries]
            ever = max(ever, len(new))
            what = "log"
            if phase == "begin":
                flying["cut"] = start - 1
        elif what == "snapshot":
            new = args[0]
        else:
            continue
        if phase == "begin":
            flying[what] = new
        else:
            done[what], flying[what] = new, None
            if what == "log":
                flying["cut"] = None
    return done, flying, ever


def check_image(i, img, ops, dest):
    img.materialize(dest)
    done, flying, ever = expected_at(ops, i)
    disk = MemberDisk(dest, null_logger())
    try:
        st = disk.load()
    except Exception as exc:
        return ["load() raised %s: %s" % (type(exc).__name__, exc)]
    bad = []
    try:
        meta = (st["epoch"], st["voted_for"])
        if meta not in (done["meta"], flying["meta"]):
            bad.append("meta %r, promised %r (in flight %r)"
                       % (meta, done["meta"], flying["meta"]))
        base = st["base_index"]
        snap = st["snapshot"]["index"] if st["snapshot"] else 0
        if base != snap or base not in (done["snapshot"],
                                        flying["snapshot"]):
            bad.append("base_index %d, snapshot %d, promised %r (in "
                       "flight %r)" % (base, snap, done["snapshot"],
                                       flying["snapshot"]))
        if base > ever:
            bad.append("snapshot at %d, but only %d entries ever existed"
                       % (base, ever))
        got = [list(e) for e in st["log"]]
        last = base + len(got)
        if not any(log is not None and log[base:last] == got
                   and len(log) >= last
                   for log in (done["log"], flying["log"])):
            bad.append("entries %d..%d are no prefix of what was appended"
                       % (base + 1, last))
        need = len(done["log"]) if flying["cut"] is None else \
            min(len(done["log"]), flying["cut"])
        if last < need:
            bad.append("entries end at %d, but appends returned up to %d"
                       % (last, need))
        # load() leaves the canonical file: contiguous from base + 1,
        # and a further append lands behind it
        disk.append(last + 1, [entry(9, 99)])
        disk.close()
        with open(os.path.join(dest, "log.jsonl"), "rb") as f:
            lines = [json.loads(line) for line in f.read().splitlines()]
        if [line[0] for line in lines] != list(range(base + 1, last + 2)) \
                or [line[1:] for line in lines] != got + [list(entry(9, 99))]:
            bad.append("log.jsonl after load() and one append is not "
                       "%d..%d" % (base + 1, last + 1))
        again = MemberDisk(dest, null_logger())
        st2 = again.load()
        again.close()
        if (st2["epoch"], st2["voted_for"], st2["base_index"]) != \
                meta + (base,) or len(st2["log"]) != len(got) + 1:
            bad.append("a second load() disagrees with the first")
    finally:
        disk.close()
    return bad


@pytest.fixture(scope="module")
def trace(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("zkdisk") / "member")
    os.makedirs(root)
    with crashfs.Recorder(root) as rec:
        workload(Driver(root, rec))
    rec.verify(exclude=())
    kinds = [op[0] for op in rec.ops]
    assert kinds.count("truncate") >= 1, "no deposed suffix was cut"
    assert sum(op[:3] == ("fsync", "", True) for op in rec.ops) >= 10
    assert ("rename", "snapshot.json.tmp", "snapshot.json") in rec.ops
    assert ("rename", "meta.json.tmp", "meta.json") in rec.ops
    assert rec.ops.count(("rename", "log.jsonl.tmp", "log.jsonl")) >= 4
    return rec


@pytest.mark.parametrize("model_name", ["process", "powerloss-journalled",
                                        "powerloss-strict"])
def test_every_crash_image_loads_to_what_was_promised(trace, model_name,
                                                      tmp_path):
    if model_name == "process":
        images = crashfs.process_images(trace.start, trace.ops)
    else:
        images = crashfs.powerloss_images(
            trace.start, trace.ops, model_name == "powerloss-journalled")
    count, wrong = 0, []
    for i, img in images:
        count += 1
        wrong += ["%s: %s" % (img.label, what)
                  for what in check_image(i, img, trace.ops,
                                          str(tmp_path / "img"))]
    print("zkdisk/%s: %d operations, %d images, %d violations"
          % (model_name, len(trace.ops), count, len(wrong)))
    assert count > 60
    assert not wrong, "%d:\n%s" % (len(wrong), "\n".join(wrong[:20]))


def test_seeded_vote_not_made_durable(tmp_path, monkeypatch):
    """The checker can fail: without the directory fsync a vote that
    ``save_meta`` returned from is forgotten under strict power loss."""
    from manatee_amd.coord import zkquorum
    monkeypatch.setattr(zkquorum, "_fsync_dir", lambda path: None)
    root = str(tmp_path / "member")
    os.makedirs(root)
    with crashfs.Recorder(root) as rec:
        workload(Driver(root, rec))
    rec.verify(exclude=())
    wrong = []
    for i, img in crashfs.powerloss_images(rec.start, rec.ops, False):
        wrong += check_image(i, img, rec.ops, str(tmp_path / "img"))
    assert any(w.startswith("meta ") for w in wrong), wrong[:10]
