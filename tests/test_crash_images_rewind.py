"""Every directory a crash can leave behind during a waldb rewind.

One successful rewind — fork point inside a segment, the tail to cut
spanning several segments, a stale promote trigger present — is recorded
under ``crashfs.Recorder``, once on a full-mode directory and once on a
layered one that loses two delta layers.  The upstream's answer is taken
from a live server beforehand and replayed by a stub, so the recorded
process does all its own I/O and ``Recorder.verify()`` holds.

For every ``kill -9`` image and every power-loss image (both readings of
what a file fsync does for its directory entry):

* without the intent marker the tree is the original one or the final
  one, so a database can only start on one of those two;
* with the marker a second rewind — which must not need the upstream —
  ends with the final tree's WAL bytes, manifest and ident;
* the WAL never has a hole;
* an image without the marker that is not the original holds no record
  past the fork point.

The marker's own ``rewind.json.tmp`` (written, not yet renamed) is the
one stray file tolerated next to the original tree: nothing reads it,
and the next rewind overwrites it.
"""

import os

import pytest

from manatee_amd.common.logging import null_logger
from manatee_amd.db.waldb import rewind
from tests import crashfs
from tests.rewind_util import build_pair, records_past, wal_bytes

STRAY = rewind.MARKER_NAME + ".tmp"
COMPARED = ("checkpoint.json", "waldb_ident.json")


class Recorded:
    pass


@pytest.fixture(scope="module", params=["full", "layered"])
def recorded(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rewind-" + request.param)
    pair = build_pair(tmp, "mid", layered=request.param == "layered")
    try:
        open(os.path.join(pair.a.data_dir, "promote"), "w").close()
        answers = []

        def live(req):
            answers.append(rewind.probe_upstream("127.0.0.1", pair.b.port,
                                                 req))
            return answers[-1]
        # the upstream's answer, from a run on a throw-away copy
        dry = pair.copy_of_a(str(tmp / "dry"))
        assert rewind.rewind_data_dir(dry, "", 0, null_logger(),
                                      probe=live).result == "ok"
    finally:
        pair.stop()
    r = Recorded()
    r.fork_lsn = pair.fork_lsn
    r.work = pair.copy_of_a(str(tmp / "work"))
    with crashfs.Recorder(r.work) as rec:
        res = rewind.rewind_data_dir(r.work, "", 0, null_logger(),
                                     probe=lambda req: answers[0])
    assert res.result == "ok" and res.bytes_cut > 0
    assert res.layers_dropped >= 2 if pair.layered \
        else res.layers_dropped == 0
    rec.verify()
    r.rec = rec
    r.original = crashfs.Image(*rec.start)
    r.final = crashfs.Image(*crashfs.snapshot(r.work))
    assert crashfs.snapshot(dry) == crashfs.snapshot(r.work)
    r.dest = str(tmp / "image")
    return r


def _no_probe(req):
    raise AssertionError("finishing a rewind must not ask the upstream")


def _check(r, img):
    img.materialize(r.dest)
    wal_bytes(r.dest)               # asserts that the segments abut
    if rewind.MARKER_NAME not in img.files:
        tree = crashfs.Image(img.dirs, {p: d for p, d in img.files.items()
                                        if p != STRAY})
        fp = tree.fingerprint()
        assert fp in (r.original.fingerprint(), r.final.fingerprint()), \
            img.label
        if fp != r.original.fingerprint():
            assert records_past(r.dest, r.fork_lsn) == 0, img.label
        return "original" if fp == r.original.fingerprint() else "final"
    res = rewind.rewind_data_dir(r.dest, "", 0, null_logger(),
                                 probe=_no_probe)
    assert res.result == "ok" and res.resumed, img.label
    _dirs, files = crashfs.snapshot(r.dest)
    assert rewind.MARKER_NAME not in files, img.label
    assert "promote" not in files, img.label
    assert wal_bytes(r.dest) == wal_bytes(r.work), img.label
    assert records_past(r.dest, r.fork_lsn) == 0, img.label
    for name in COMPARED:
        assert files.get(name) == r.final.files.get(name), \
            "%s: %s" % (img.label, name)
    return "marker"


def test_the_recorded_rewind_is_the_interesting_one(recorded):
    kinds = [op[0] for op in recorded.rec.ops]
    # several whole segments dropped, one shortened
    assert kinds.count("unlink") >= 2 + 2
    assert kinds.count("truncate") >= 1
    assert recorded.final.fingerprint() != recorded.original.fingerprint()


def test_every_process_crash_image(recorded):
    seen = set()
    for _i, img in crashfs.process_images(recorded.rec.start,
                                          recorded.rec.ops):
        seen.add(_check(recorded, img))
    assert seen == {"original", "marker", "final"}


@pytest.mark.parametrize("file_fsync_persists_entry", [True, False])
def test_every_powerloss_image(recorded, file_fsync_persists_entry):
    seen = set()
    for _i, img in crashfs.powerloss_images(recorded.rec.start,
                                            recorded.rec.ops,
                                            file_fsync_persists_entry):
        seen.add(_check(recorded, img))
    assert seen == {"original", "marker", "final"}
