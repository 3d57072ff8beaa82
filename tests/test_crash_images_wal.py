"""Crash images of a bare ``Wal`` directory (tests/crashfs.py), process
model: after ``kill -9`` at any file operation — a torn ``pwrite``
included — ``open()`` yields a byte-exact prefix of the logical stream
that held at some point of the trace, or raises.  And a directory whose
segments do not abut must make ``open()`` raise.
"""

import os
import shutil

import pytest

from manatee_amd.db.waldb.wal import Wal, encode_frame
from tests import crashfs

SEGMENT = 256


class Driver:
    """A ``Wal`` under the recorder, with the logical stream it should
    hold.  ``versions`` are the streams that ever held: a truncation
    starts a new one."""

    def __init__(self, d, rec):
        self.rec = rec
        self.wal = Wal(d, segment_bytes=SEGMENT)
        self.stream = b""
        self.versions = []
        self.n = 0
        self.wal.open()
        self.mark()

    def mark(self):
        assert self.wal.end == len(self.stream)
        self.rec.mark(("end", self.wal.end))

    def payload(self):
        self.n += 1
        return (b"rec-%03d-" % self.n) * (1 + self.n % 5)

    def append(self):
        p = self.payload()
        self.stream += encode_frame(p)
        assert self.wal.append(p) == len(self.stream)
        self.mark()

    def append_buffered(self, count):
        for _ in range(count):
            p = self.payload()
            self.stream += encode_frame(p)
            self.wal.append_buffered(p)
        self.wal.flush_buffer()
        self.mark()

    def append_raw(self, count):
        chunk = b"".join(encode_frame(self.payload()) for _ in range(count))
        self.wal.append_raw(chunk, len(self.stream))
        self.stream += chunk
        self.mark()

    def truncate_to(self, lsn):
        self.versions.append(self.stream)
        self.stream = self.stream[:lsn]
        self.wal.truncate_to(lsn)
        self.mark()

    def finish(self):
        self.wal.fsync()
        self.wal.close()
        self.versions.append(self.stream)


def boundaries(stream):
    """Offsets at which a record of ``stream`` ends, and 0."""
    out, pos = {0}, 0
    while pos < len(stream):
        pos += 8 + int.from_bytes(stream[pos:pos + 4], "big")
        out.add(pos)
    assert pos == len(stream)
    return out


def _appends(d):
    for i in range(30):
        if i % 3 == 2:
            d.append_buffered(1 + i % 4)
        else:
            d.append()
        if i % 8 == 7:
            d.wal.fsync()


def _raw(d):
    for i in range(30):
        d.append_raw(1 + i % 3)


def _drop(d):
    for i in range(45):
        d.append()
        if i in (20, 35, 44):
            start = d.wal.start
            d.wal.drop_below(len(d.stream) - 300)
            assert d.wal.start > start
            d.mark()


def _truncate(d):
    """Timeline fencing: cut in the middle of a segment several
    segments back, then at a segment's first byte, each followed by
    appends that roll again."""
    for _ in range(60):
        d.append()
    segs = list(d.wal._segs)
    assert len(segs) >= 6
    cut = min(b for b in boundaries(d.stream) if b > segs[-4])
    assert segs[-4] < cut < segs[-3]
    d.truncate_to(cut)
    assert d.wal._segs == segs[:-3]
    for _ in range(20):
        d.append()
    segs = list(d.wal._segs)
    assert len(segs) >= 4
    d.truncate_to(segs[-2])
    for _ in range(12):
        d.append()


WORKLOADS = {"appends": _appends, "append_raw": _raw, "drop_below": _drop,
             "truncate_to": _truncate}


def check_image(i, img, ops, versions, dest):
    """Open one image; returns what is wrong with the result, if
    anything, and whether ``open()`` refused."""
    img.materialize(dest)
    ends = [op[1][1] for op in ops[:i] if op[0] == "mark"][-1:] + \
        [op[1][1] for op in ops[i:] if op[0] == "mark"][:1]
    wal = Wal(dest, segment_bytes=SEGMENT)
    seen = []
    try:
        end = wal.open(replay=lambda lsn, p: seen.append((lsn, p)))
    except IOError:
        return None, True
    try:
        start = wal.start
        data = wal.read(start, 1 << 30)
        if len(data) != end - start:
            return "read %d bytes of [%d, %d)" % (len(data), start, end), False
        if not min(ends) <= end <= max(ends):
            return "end %d, but the calls around the crash had %r" % (
                end, ends), False
        for stream in versions:
            if len(stream) >= end and stream[start:end] == data \
                    and {start, end} <= boundaries(stream):
                break
        else:
            return "[%d, %d) is no prefix of a stream that held" % (
                start, end), False
        frames = b"".join(encode_frame(p) for _lsn, p in seen)
        if frames != data or [lsn for lsn, _p in seen] != sorted(
                boundaries(stream[:end]) - boundaries(stream[:start])):
            return "replay handed out other records than the file holds", \
                False
        # usable: one more record, and it is there after a reopen
        last = wal.append(b"after-crash")
    finally:
        wal.close()
    again = Wal(dest, segment_bytes=SEGMENT)
    try:
        if again.open() != last or again.read(start, 1 << 30) != \
                data + encode_frame(b"after-crash"):
            return "append after recovery did not survive a reopen", False
    finally:
        again.close()
    return None, False


@pytest.mark.parametrize("name", sorted(WORKLOADS))
def test_every_process_crash_image_opens_to_a_prefix(name, tmp_path):
    root = str(tmp_path / "wal")
    os.makedirs(root)
    with crashfs.Recorder(root) as rec:
        d = Driver(root, rec)
        WORKLOADS[name](d)
        d.finish()
    rec.verify()
    kinds = [op[0] for op in rec.ops]
    assert kinds.count("create") >= 4, "no segment rolls"
    if name == "drop_below":
        assert kinds.count("unlink") >= 3
    if name == "truncate_to":
        assert kinds.count("unlink") >= 4 and kinds.count("truncate") >= 2
    count = refused = 0
    wrong = []
    for i, img in crashfs.process_images(rec.start, rec.ops):
        count += 1
        what, raised = check_image(i, img, rec.ops, d.versions,
                                   str(tmp_path / "img"))
        refused += raised
        if what:
            wrong.append("%s: %s" % (img.label, what))
    print("wal/%s: %d operations, %d images, %d refused, %d wrong"
          % (name, len(rec.ops), count, refused, len(wrong)))
    assert count > len(rec.ops) // 2
    assert not wrong, "\n".join(wrong[:20])
    # open() may refuse an image, but no crash of these calls needs it to
    assert refused == 0


# ----------------------------------------------------------------------- gaps

@pytest.fixture
def six_segments(tmp_path):
    d = str(tmp_path / "wal")
    w = Wal(d, segment_bytes=SEGMENT)
    w.open()
    lsns = [w.append((b"rec-%03d-" % i) * 4) for i in range(40)]
    w.fsync()
    w.close()
    segs = w._segs
    assert len(segs) >= 6
    return d, segs, lsns


def _opens(d, replay_from):
    w = Wal(d, segment_bytes=SEGMENT)
    seen = []
    try:
        return w.open(replay=lambda lsn, p: seen.append(lsn),
                      replay_from=replay_from), seen
    finally:
        w.close()


@pytest.mark.parametrize("beyond", [False, True])
def test_open_refuses_a_missing_middle_segment(six_segments, beyond):
    """``beyond``: the hole lies below ``replay_from``, where segments
    are not scanned."""
    d, segs, lsns = six_segments
    replay_from = segs[4] if beyond else 0
    assert _opens(d, replay_from)[0] == lsns[-1]
    os.unlink(os.path.join(d, "wal-%016x.seg" % segs[2]))
    with pytest.raises(IOError) as exc:
        end, seen = _opens(d, replay_from)
        print("open() returned end %d after replaying %d of %d records"
              % (end, len(seen), len(lsns)))
    assert str(segs[2]) in str(exc.value) and str(segs[3]) in str(exc.value)


@pytest.mark.parametrize("beyond", [False, True])
def test_open_refuses_a_segment_shorter_than_the_next_start(six_segments,
                                                            beyond):
    d, segs, lsns = six_segments
    replay_from = segs[4] if beyond else 0
    # cut at a record boundary: every frame left in the file is valid
    short = max(lsn for lsn in lsns if segs[2] < lsn < segs[3])
    assert short > segs[2]
    with open(os.path.join(d, "wal-%016x.seg" % segs[2]), "r+b") as f:
        f.truncate(short - segs[2])
    with pytest.raises(IOError) as exc:
        end, seen = _opens(d, replay_from)
        print("open() returned end %d after replaying %d of %d records"
              % (end, len(seen), len(lsns)))
    assert str(short) in str(exc.value) and str(segs[3]) in str(exc.value)


def test_a_half_done_truncation_never_leaves_a_hole(six_segments, tmp_path):
    """Stop ``truncate_to`` after each of its unlinks in turn: what is
    left may hold more WAL than asked for, never a gap."""
    d, segs, lsns = six_segments
    cut = min(lsn for lsn in lsns if lsn > segs[1])
    dropped = [s for s in segs if s > cut]
    assert len(dropped) >= 4
    for done in range(1, len(dropped)):
        copy = str(tmp_path / ("copy%d" % done))
        shutil.copytree(d, copy)
        w = Wal(copy, segment_bytes=SEGMENT)
        w.open()
        real_unlink, calls = os.unlink, []

        def unlink(path, *a, **kw):
            if len(calls) == done:
                raise KeyboardInterrupt("kill -9")
            calls.append(path)
            real_unlink(path, *a, **kw)

        os.unlink = unlink
        try:
            with pytest.raises(KeyboardInterrupt):
                w.truncate_to(cut)
        finally:
            os.unlink = real_unlink
            os.close(w._fd)
        end, seen = _opens(copy, 0)
        assert end in segs and end > cut
        assert seen == [lsn for lsn in lsns if lsn <= end]
