"""Rewind a diverged waldb data directory to the fork point.

A peer whose WAL ran past the point where the shard's history switched
timelines (a deposed primary, a standby refused as ``diverged``) does
not need its whole dataset replaced.  WAL is replicated byte for byte,
so LSNs are byte offsets every peer shares, and the WAL that makes the
peer unusable is the tail past the fork point ``D``.  A rewind

1. asks the upstream for ``D`` and a CRC of its own WAL just below it
   (the ``rewind-probe`` request, ``ReplCore.rewind_probe``),
2. checks that ``D`` is a record boundary here and that the local bytes
   below it match,
3. makes sure the checkpoint image on disk is at or before ``D``
   (dropping delta layers that are past it),
4. cuts the WAL at ``D`` and rewrites the ident to the common history.

Ordinary recovery and streaming do the rest.  PostgreSQL's ``pg_rewind``
solves the same problem by copying changed blocks; here the checkpoint
is logical and replay is idempotent, so cutting the log is enough.

``fork_point`` is pure.  ``rewind_data_dir`` runs on a STOPPED database
only and is synchronous (the engine runs it in the executor).  Steps
3-4 run under a durable intent marker, ``rewind.json``: the database
refuses to start while it exists, and a second ``rewind_data_dir``
finishes the interrupted one and reaches the same bytes.
"""

from __future__ import annotations

import argparse
import dataclasses
import json
import os
import socket
import sys
import zlib
from typing import Callable, Iterator, List, Optional, Tuple

from ...common import dial
from ...common import lsn as lsnmod
from ...common.logging import Logger, level_from_verbosity
from . import ckpt as ckptmod
from .wal import _SEG_RE, Wal, _scan, fsync_dir

MARKER_NAME = "rewind.json"
# how far below the fork point the two sides compare bytes: the window
# of one ``Wal.read``
PROBE_WINDOW = 1 << 20
# bytes hashed between two yields to the event loop (upstream) and per
# file read (here)
CRC_CHUNK = 64 * 1024
PID_FILES = ("waldb.pid", "db_child.pid")


class RewindPending(Exception):
    """The data directory holds an unfinished rewind (``rewind.json``).
    The database must not start on it: the WAL, the checkpoint and the
    ident may belong to different histories."""


# ------------------------------------------------------------ arithmetic
def common_prefix(f_history: List[dict], u_history: List[dict]
                  ) -> List[dict]:
    """The longest common prefix of two timeline histories, entries
    compared whole (``tl`` and ``at``)."""
    out = []
    for a, b in zip(f_history or [], u_history or []):
        if (a.get("tl"), a.get("at")) != (b.get("tl"), b.get("at")):
            break
        out.append({"tl": a["tl"], "at": a["at"]})
    return out


def fork_point(f_timeline: int, f_history: List[dict], f_end: int,
               u_timeline: int, u_history: List[dict], u_end: int
               ) -> Tuple[int, int]:
    """Where a follower's history and an upstream's part ways.

    Returns ``(common_timeline, D)``.  The common timeline is the one
    the longest common prefix of the histories ends on (1 for an empty
    prefix).  Each side's extent on it is the ``at`` of its next switch
    point if it has one, else its WAL end; ``D`` is the smaller extent.
    Two peers that both went 1→2 at different offsets share only
    timeline 1.  The timelines themselves are implied by the histories;
    they are part of the signature because the handshake carries them."""
    prefix = common_prefix(f_history, u_history)
    n = len(prefix)
    common_tl = prefix[-1]["tl"] if prefix else 1

    def extent(history: List[dict], end: int) -> int:
        history = history or []
        return int(history[n]["at"]) if n < len(history) else int(end)

    return common_tl, min(extent(f_history, f_end), extent(u_history, u_end))


def probe_window(f_start: int, u_start: int, fork_lsn: int) -> int:
    """Start of the byte range both sides hash: as far below the fork
    point as both still have WAL, one read window at the most."""
    return max(int(f_start), int(u_start), fork_lsn - PROBE_WINDOW)


def crc_slices(read: Callable[[int, int], bytes], lo: int, hi: int
               ) -> Iterator[int]:
    """CRC-32 of the bytes ``[lo, hi)`` that ``read(lo, hi)`` returns,
    ``CRC_CHUNK`` at a time: yields the running value after every slice
    (a caller on an event loop yields to it in between), the last one is
    the CRC of the whole range.  Nothing is yielded for an empty range;
    a read that comes back short raises ``IOError``."""
    crc, pos = 0, lo
    while pos < hi:
        data = read(pos, min(pos + CRC_CHUNK, hi))
        if not data:
            raise IOError("no WAL bytes at %d" % pos)
        crc = zlib.crc32(data, crc)
        pos += len(data)
        yield crc


def range_crc(read: Callable[[int, int], bytes], lo: int, hi: int) -> int:
    crc = 0
    for crc in crc_slices(read, lo, hi):
        pass
    return crc


# ------------------------------------------------- replication handshake
# A follower may stream from ``start_lsn`` (its WAL end) only if its WAL
# is a byte prefix of the upstream's.  The histories can rule that out
# (``check_follower``); they cannot confirm it: two peers promoted at
# the same offset have identical histories and different bytes after
# it, and so has a primary that lost an unsynced tail its follower
# holds.  So an accepted follower gets the CRC of the upstream's bytes
# just below ``start_lsn`` (``handshake_offer``) and compares it with
# its own before it appends or acks anything (``handshake_verify``).
def check_follower(f_timeline: int, f_history: Optional[List[dict]],
                   start_lsn: int, u_timeline: int, u_history: List[dict],
                   u_start: int, u_end: int) -> Optional[str]:
    """May a follower at ``(f_timeline, start_lsn)`` with history
    ``f_history`` stream from an upstream with WAL ``[u_start, u_end)``?
    Returns the refusal (``timeline-mismatch``, ``diverged``,
    ``wal-gone``) or None.  ``f_history`` is None for a follower that
    does not send one: then only the upstream's own switch points to
    timelines above the follower's are held against it."""
    if f_timeline > u_timeline:
        return "timeline-mismatch"
    # the follower must not have WAL past our switch to any later
    # timeline: that WAL belongs to a deposed line of history
    for h in u_history or []:
        if h["tl"] > f_timeline and start_lsn > h["at"]:
            return "diverged"
    if start_lsn > u_end:
        return "diverged"
    if f_history is not None:
        # ... nor past the point where the two histories part ways: two
        # peers promoted apart share nothing above the lower switch
        _tl, fork = fork_point(f_timeline, f_history, start_lsn,
                               u_timeline, u_history, u_end)
        if fork < start_lsn:
            return "diverged"
    if start_lsn < u_start:
        # the WAL this follower needs was recycled by a checkpoint; it
        # must bootstrap from a snapshot instead
        return "wal-gone"
    return None


def handshake_offer(f_start: int, u_start: int, start_lsn: int,
                    read: Callable[[int, int], bytes]) -> dict:
    """What the upstream's OK answer carries for an accepted follower:
    ``{window_start, crc32}`` of ITS bytes in ``[W, start_lsn)``,
    ``W = probe_window(...)``.  ``W >= start_lsn`` is an empty window (a
    freshly restored follower has no WAL below its end): CRC 0."""
    window = probe_window(f_start, u_start, start_lsn)
    return {"window_start": window,
            "crc32": range_crc(read, window, start_lsn)}


def offered_window(resp: dict, start_lsn: int) -> Optional[Tuple[int, int]]:
    """``(W, crc)`` the follower has to check, or None when the answer
    carries none (an upstream that does not send one) or an empty one."""
    if "window_start" not in resp or "crc32" not in resp:
        return None
    window, crc = int(resp["window_start"]), int(resp["crc32"])
    if window >= start_lsn:
        return None
    return window, crc


def handshake_verify(resp: dict, start_lsn: int,
                     read: Callable[[int, int], bytes]) -> bool:
    """The follower's half: are its own bytes in the offered window the
    upstream's?  True as well when there is nothing to compare."""
    offered = offered_window(resp, start_lsn)
    if offered is None:
        return True
    return range_crc(read, offered[0], start_lsn) == offered[1]


# ---------------------------------------------------------------- result
@dataclasses.dataclass
class RewindResult:
    """``result`` is ``ok`` (WAL cut), ``noop`` (nothing to cut) or
    ``refused`` (directory untouched; ``reason`` says why)."""
    result: str
    reason: Optional[str] = None
    fork_lsn: Optional[int] = None
    timeline: Optional[int] = None
    bytes_cut: int = 0
    layers_dropped: int = 0
    resumed: bool = False

    @property
    def ok(self) -> bool:
        return self.result in ("ok", "noop")

    def as_dict(self) -> dict:
        return {"ok": self.ok, "result": self.result, "reason": self.reason,
                "fork_lsn": (lsnmod.format_lsn(self.fork_lsn)
                             if self.fork_lsn is not None else None),
                "fork_lsn_bytes": self.fork_lsn,
                "timeline": self.timeline, "bytes_cut": self.bytes_cut,
                "layers_dropped": self.layers_dropped,
                "resumed": self.resumed}


def _refused(reason: str, **kw) -> RewindResult:
    return RewindResult("refused", reason=reason, **kw)


# ------------------------------------------------------- read-only views
def _live_pid(data_dir: str) -> Optional[int]:
    for name in PID_FILES:
        try:
            with open(os.path.join(data_dir, name)) as f:
                pid = int(f.read().split()[0])
        except (OSError, ValueError, IndexError):
            continue
        try:
            os.kill(pid, 0)
        except ProcessLookupError:
            continue
        except PermissionError:
            pass
        # a zombie (killed, not yet reaped by its parent) holds no files
        try:
            with open("/proc/%d/stat" % pid) as f:
                if f.read().rpartition(")")[2].split()[0] == "Z":
                    continue
        except (OSError, IndexError):
            pass
        return pid
    return None


def _segments(data_dir: str) -> List[Tuple[int, int]]:
    """``[(start LSN, size)]`` of the WAL segment files, sorted."""
    out = []
    for name in os.listdir(data_dir):
        m = _SEG_RE.match(name)
        if m:
            out.append((int(m.group(1), 16),
                        os.path.getsize(os.path.join(data_dir, name))))
    return sorted(out)


class _LocalWal:
    """The WAL of a stopped database, read without changing a byte
    (``Wal.open`` would cut a torn tail)."""

    def __init__(self, data_dir: str):
        self.dir = data_dir
        self.segs = _segments(data_dir)
        if not self.segs:
            raise IOError("no WAL segments")
        pos = self.segs[0][0]
        for start, size in self.segs[:-1]:
            if start != pos:
                raise IOError("WAL segments do not abut at %d" % pos)
            pos = start + size
        if self.segs[-1][0] != pos:
            raise IOError("WAL segments do not abut at %d" % pos)
        self.start = self.segs[0][0]

    def _path(self, start: int) -> str:
        return os.path.join(self.dir, "wal-%016x.seg" % start)

    def scan(self, from_lsn: int, boundary: Optional[int]
             ) -> Tuple[int, bool]:
        """Validate records from ``from_lsn`` (a record boundary, as is
        every segment start).  Returns ``(end, hit)``: the end of the
        last whole record, and whether ``boundary`` is a record
        boundary at or above ``from_lsn``."""
        hit = boundary == from_lsn
        end = max(from_lsn, self.start)
        for i, (start, size) in enumerate(self.segs):
            last = i == len(self.segs) - 1
            if start + size <= from_lsn and not last:
                continue
            skip = max(0, from_lsn - start)
            with open(self._path(start), "rb") as f:
                f.seek(skip)
                buf = f.read()
            valid, records = _scan(buf)
            base = start + skip
            if boundary is not None and base <= boundary <= base + valid:
                want = boundary - base
                hit = hit or want == 0 or any(
                    off + length == want for off, length in records)
            end = base + valid
            if valid != len(buf):
                if not last:
                    raise IOError("corrupt interior WAL segment at %d"
                                  % (base + valid))
                break
        return end, hit

    def crc32(self, lo: int, hi: int) -> int:
        """CRC-32 of the raw bytes ``[lo, hi)``."""
        crc = 0
        for start, size in self.segs:
            a, b = max(lo, start), min(hi, start + size)
            if a >= b:
                continue
            with open(self._path(start), "rb") as f:
                f.seek(a - start)
                left = b - a
                while left > 0:
                    data = f.read(min(left, CRC_CHUNK))
                    if not data:
                        raise IOError("short WAL segment at %d" % start)
                    crc = zlib.crc32(data, crc)
                    left -= len(data)
        return crc


def _checkpoint_plan(data_dir: str, fork_lsn: int, wal_start: int):
    """What the checkpoint image needs so that it is at or before
    ``fork_lsn``.  Returns ``(replay_from, manifest, dropped)``:
    the LSN recovery will replay from, the manifest to publish (None if
    the file on disk can stay) and how many layers that drops — or
    raises ``ValueError`` when no image at or before the fork exists."""
    from .core import CKPT_NAME
    path = os.path.join(data_dir, CKPT_NAME)
    try:
        with open(path) as f:
            ckpt = json.load(f)
    except FileNotFoundError:
        ckpt = None
    manifest, dropped = None, 0
    if ckpt is None:
        replay_from = 0
    elif "kv" not in ckpt and "format" in ckpt:
        if ckpt["format"] != ckptmod.MANIFEST_FORMAT:
            raise ValueError("checkpoint-format")
        names = ckptmod.manifest_layers(ckpt)
        keep = [n for n in names
                if ckptmod.parse_layer_name(n)[0] <= fork_lsn]
        if not keep:
            raise ValueError("checkpoint-past-fork")
        replay_from = int(ckpt.get("lsn", 0))
        if len(keep) != len(names) or replay_from > fork_lsn:
            # the image is consistent at its top layer's LSN
            replay_from = ckptmod.parse_layer_name(keep[-1])[0]
            manifest = {"format": ckptmod.MANIFEST_FORMAT,
                        "lsn": replay_from, "layers": keep}
            dropped = len(names) - len(keep)
    else:
        replay_from = int(ckpt.get("lsn", 0))
        if replay_from > fork_lsn:
            raise ValueError("checkpoint-past-fork")
    if wal_start > replay_from:
        # the WAL between the surviving image and the fork is recycled
        raise ValueError("checkpoint-past-fork")
    return replay_from, manifest, dropped


# ----------------------------------------------------------------- probe
def probe_upstream(host: str, port: int, req: dict,
                   timeout_s: float = 10.0) -> dict:
    """One ``rewind-probe`` exchange with the upstream's replication
    port."""
    h, p = dial.resolve(host, port)
    with socket.create_connection((h, p), timeout=timeout_s) as sock:
        sock.sendall((json.dumps(dict(req, q="rewind-probe"))
                      + "\n").encode())
        buf = b""
        while not buf.endswith(b"\n"):
            data = sock.recv(65536)
            if not data:
                break
            buf += data
    if not buf:
        raise ConnectionError("upstream closed the connection")
    return json.loads(buf)


# ---------------------------------------------------------------- rewind
def _apply(data_dir: str, marker: dict, log: Logger) -> None:
    """Steps 3-5 from the marker alone.  Every step is idempotent and
    durable before the next begins, so this can be run again after a
    crash at any point."""
    from .core import (CKPT_NAME, IDENT_NAME, PROMOTE_TRIGGER,
                       _write_json_atomic)
    fork_lsn = int(marker["fork_lsn"])
    if marker.get("manifest") is not None:
        _write_json_atomic(os.path.join(data_dir, CKPT_NAME),
                           marker["manifest"], separators=(",", ":"))
    wal = Wal(data_dir)
    wal.open(replay=None, replay_from=int(marker["replay_from"]))
    try:
        if wal.end < fork_lsn:
            raise IOError("WAL ends at %d, below the fork point %d"
                          % (wal.end, fork_lsn))
        wal.truncate_to(fork_lsn)
    finally:
        wal.close()
    ident_path = os.path.join(data_dir, IDENT_NAME)
    with open(ident_path) as f:
        ident = json.load(f)
    ident["timeline"] = marker["timeline"]
    ident["history"] = marker["history"]
    _write_json_atomic(ident_path, ident)
    _unlink_durably(data_dir, PROMOTE_TRIGGER)
    _unlink_durably(data_dir, MARKER_NAME)
    log.info("rewind complete", fork=lsnmod.format_lsn(fork_lsn),
             timeline=marker["timeline"])


def _unlink_durably(data_dir: str, name: str) -> None:
    try:
        os.unlink(os.path.join(data_dir, name))
    except FileNotFoundError:
        return
    fsync_dir(data_dir)


def read_marker(data_dir: str) -> Optional[dict]:
    try:
        with open(os.path.join(data_dir, MARKER_NAME)) as f:
            return json.load(f)
    except FileNotFoundError:
        return None


def rewind_data_dir(data_dir: str, upstream_host: str, upstream_port: int,
                    log: Logger,
                    probe: Optional[Callable[[dict], dict]] = None
                    ) -> RewindResult:
    """Rewind the stopped database in ``data_dir`` to where its history
    and the upstream's part ways.  A refusal leaves the directory as it
    was.  ``probe`` replaces the network exchange (request dict in,
    response dict out)."""
    from .core import IDENT_NAME, PROMOTE_TRIGGER, _write_json_atomic
    data_dir = os.path.abspath(data_dir)
    pid = _live_pid(data_dir)
    if pid is not None:
        return _refused("running (pid %d)" % pid)

    marker = read_marker(data_dir)
    if marker is not None:
        # an earlier rewind was interrupted: it had passed every check
        log.warn("finishing an interrupted rewind",
                 fork=lsnmod.format_lsn(int(marker["fork_lsn"])))
        _apply(data_dir, marker, log)
        return RewindResult("ok", fork_lsn=int(marker["fork_lsn"]),
                            timeline=marker["timeline"], resumed=True)

    try:
        with open(os.path.join(data_dir, IDENT_NAME)) as f:
            ident = json.load(f)
        local = _LocalWal(data_dir)
        local_end, _ = local.scan(local.start, None)
    except (OSError, ValueError) as exc:
        return _refused("local-unreadable: %s" % exc)
    timeline = int(ident.get("timeline", 1))
    history = ident.get("history", [])

    # 1. probe
    req = {"ident": ident.get("ident"), "timeline": timeline,
           "history": history, "wal_start": local.start,
           "wal_end": local_end}
    try:
        resp = probe(req) if probe is not None else \
            probe_upstream(upstream_host, upstream_port, req)
    except (OSError, ValueError) as exc:
        return _refused("connection-failed: %s" % exc)
    if not resp.get("ok"):
        return _refused(str(resp.get("error") or "probe-refused"))
    try:
        fork_lsn = int(resp["fork_lsn"])
        window = int(resp["window_start"])
        want_crc = int(resp["crc32"])
        u_history = list(resp.get("history") or [])
    except (KeyError, TypeError, ValueError):
        return _refused("bad-probe-response")
    prefix = common_prefix(history, u_history)
    common_tl = prefix[-1]["tl"] if prefix else 1
    where = dict(fork_lsn=fork_lsn, timeline=common_tl)
    if not local.start <= window < fork_lsn <= local_end:
        return _refused("unverifiable", **where)

    # 3 (decided first: it fixes where the boundary scan may begin)
    try:
        replay_from, manifest, dropped = _checkpoint_plan(
            data_dir, fork_lsn, local.start)
    except ValueError as exc:
        return _refused(str(exc), **where)
    except (OSError, ckptmod.CheckpointCorrupt) as exc:
        return _refused("local-unreadable: %s" % exc, **where)

    # 2. verify
    try:
        _end, hit = local.scan(replay_from, fork_lsn)
        if not hit:
            return _refused("not-a-boundary", **where)
        if local.crc32(window, fork_lsn) != want_crc:
            return _refused("history-mismatch", **where)
    except OSError as exc:
        return _refused("local-unreadable: %s" % exc, **where)

    # 6. nothing to cut
    if fork_lsn == local_end and prefix == history and manifest is None:
        _unlink_durably(data_dir, PROMOTE_TRIGGER)
        log.info("rewind: nothing to cut",
                 fork=lsnmod.format_lsn(fork_lsn))
        return RewindResult("noop", **where)

    # 3-5 under the intent marker
    marker = {"fork_lsn": fork_lsn, "timeline": common_tl,
              "history": prefix, "replay_from": replay_from,
              "manifest": manifest}
    _write_json_atomic(os.path.join(data_dir, MARKER_NAME), marker)
    log.info("rewinding", fork=lsnmod.format_lsn(fork_lsn),
             bytes_cut=local_end - fork_lsn, layers_dropped=dropped,
             timeline=common_tl)
    _apply(data_dir, marker, log)
    return RewindResult("ok", bytes_cut=local_end - fork_lsn,
                        layers_dropped=dropped, **where)


# ------------------------------------------------------------------ main
def main(argv=None) -> int:
    ap = argparse.ArgumentParser(
        prog="waldb-rewind",
        description="Rewind a stopped waldb data directory to the point "
                    "where its WAL and the upstream's part ways")
    ap.add_argument("-D", "--data-dir", required=True)
    ap.add_argument("--upstream", required=True, metavar="HOST:PORT")
    ap.add_argument("-v", "--verbose", action="count", default=0)
    ns = ap.parse_args(argv)
    host, _, port = ns.upstream.rpartition(":")
    log = Logger("waldb-rewind", level=level_from_verbosity(ns.verbose))
    res = rewind_data_dir(ns.data_dir, host, int(port), log)
    print(json.dumps(res.as_dict()))
    return 0 if res.ok else 1


if __name__ == "__main__":
    sys.exit(main())
