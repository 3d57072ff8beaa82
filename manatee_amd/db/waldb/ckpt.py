"""Layered checkpoint files for ``checkpoint_mode = incremental``.

A checkpoint in this mode writes only the keys touched since the previous
one, as an immutable *layer* file under ``<data_dir>/ckpt/``.  The
manifest ``checkpoint.json`` names the layers that make up the image,
oldest first: one ``base`` and any number of ``delta`` layers on top.

A layer is a stream of WAL-format frames (``u32 len | u32 crc32 |
payload``, see ``wal.py``), validated with the same native scanner:

    frame 0      {"ckpt":"header","kind":K,"lsn":L,"parent":P,"count":N}
    frame 1..    ordinary ``batch`` ops of ``put`` / ``del`` (tombstone)
    last frame   {"ckpt":"trailer","count":N}

``L`` is the LSN the layer is consistent at, ``P`` the LSN of the layer
below it (0 for a base) and ``N`` the number of put/del records.  The
trailer makes a copy that was cut at a frame boundary detectable.  The
file name repeats ``L`` and ``K``: ``<%016x L>.<K>``.

Everything here is synchronous and touches no server state, so the
writers run in the executor and the loader can be called on a bare
directory.
"""

from __future__ import annotations

import json
import os
import re
import subprocess
import sys
from typing import Dict, Iterable, Iterator, List, Tuple

from .wal import _scan, decode_op, encode_frame, encode_op

CKPT_DIR = "ckpt"
MANIFEST_FORMAT = 2
# records per batch frame, and a byte bound for large values: no frame
# may come near the 64 MiB record cap of the scanner
CHUNK_KEYS = 4096
CHUNK_BYTES = 4 * 1024 * 1024
# a layer is validated this many bytes per scanner call: the native
# scanner keeps the GIL, and one call over a whole base would stall the
# event loop for as long as its CRCs take
SCAN_WINDOW = 8 * 1024 * 1024
# layers of at least this many bytes together are merged in a child
# process, see merge_layers_offloaded
MERGE_IN_CHILD_BYTES = 1024 * 1024
# merge when the deltas together reach the base's size, or past this
# many layers
MAX_LAYERS = 8

TOMBSTONE = object()
_NAME_RE = re.compile(r"^([0-9a-f]{16})\.(base|delta)$")


class CheckpointCorrupt(Exception):
    """A layer the manifest names is missing or damaged.  The database
    must not start: serving the kv without that layer would silently
    lose or resurrect keys."""


class CheckpointFormatError(Exception):
    """``checkpoint.json`` has a format this build does not know."""


def layer_name(lsn: int, kind: str) -> str:
    return "%016x.%s" % (lsn, kind)


def parse_layer_name(name: str) -> Tuple[int, str]:
    m = _NAME_RE.match(name)
    if not m:
        raise CheckpointCorrupt("bad layer name %r" % (name,))
    return int(m.group(1), 16), m.group(2)


def apply_op(kv: dict, op: dict) -> None:
    """``ReplCore._apply_op`` on a bare dict."""
    kind = op.get("op")
    if kind == "put":
        kv[op["k"]] = op["v"]
    elif kind == "del":
        kv.pop(op["k"], None)
    elif kind == "batch":
        for sub in op.get("ops") or []:
            apply_op(kv, sub)


def _fsync_dir(path: str) -> None:
    fd = os.open(path, os.O_RDONLY)
    try:
        os.fsync(fd)
    finally:
        os.close(fd)


def write_layer(ckpt_dir: str, kind: str, lsn: int, parent: int,
                items: Iterable[Tuple[object, object]], count: int) -> dict:
    """Write one layer: ``items`` yields ``count`` pairs ``(key, value)``
    with ``TOMBSTONE`` as the value of a deleted key.  tmp + fsync +
    rename + directory fsync.  Returns the layer's description
    ``{name, kind, lsn, bytes, records}``."""
    os.makedirs(ckpt_dir, exist_ok=True)
    name = layer_name(lsn, kind)
    path = os.path.join(ckpt_dir, name)
    tmp = path + ".tmp"
    written = 0
    with open(tmp, "wb") as f:
        f.write(encode_frame(encode_op(
            {"ckpt": "header", "kind": kind, "lsn": lsn, "parent": parent,
             "count": count})))
        chunk: List[bytes] = []
        chunk_bytes = 0

        def flush_chunk() -> None:
            f.write(encode_frame(
                b'{"op":"batch","ops":[' + b",".join(chunk) + b"]}"))

        for k, v in items:
            sub = encode_op({"op": "del", "k": k} if v is TOMBSTONE
                            else {"op": "put", "k": k, "v": v})
            chunk.append(sub)
            chunk_bytes += len(sub)
            written += 1
            if len(chunk) >= CHUNK_KEYS or chunk_bytes >= CHUNK_BYTES:
                flush_chunk()
                chunk, chunk_bytes = [], 0
        if chunk:
            flush_chunk()
        if written != count:
            raise ValueError("layer %s: %d records for a header of %d"
                             % (name, written, count))
        f.write(encode_frame(encode_op({"ckpt": "trailer",
                                        "count": count})))
        f.flush()
        os.fsync(f.fileno())
        size = os.fstat(f.fileno()).st_size
    os.replace(tmp, path)
    _fsync_dir(ckpt_dir)
    return {"name": name, "kind": kind, "lsn": lsn, "bytes": size,
            "records": count}


def _scan_windowed(buf: bytes) -> Tuple[int, List[Tuple[int, int]]]:
    """``wal._scan`` over ``buf`` in windows of ``SCAN_WINDOW``."""
    view = memoryview(buf)
    records: List[Tuple[int, int]] = []
    pos, window = 0, SCAN_WINDOW
    while pos < len(buf):
        valid, found = _scan(view[pos:pos + window])
        if valid == 0:
            if pos + window >= len(buf):
                break
            window *= 2         # one frame larger than the window
            continue
        records.extend((pos + off, length) for off, length in found)
        pos += valid
        window = SCAN_WINDOW
    return pos, records


def open_layer(ckpt_dir: str, name: str) -> Tuple[dict, Iterator[dict]]:
    """Validate one layer file; returns ``(header, batch ops)``.  Raises
    ``CheckpointCorrupt`` for a missing file, a frame that fails its
    CRC, a missing trailer, or a header that disagrees with the file
    name or the records.

    Every CRC, the header and the trailer are checked before this
    returns.  The batch ops are decoded one frame at a time as the
    iterator is consumed, so that a base of millions of records never
    has them all alive at once (a cyclic-GC pass over that many dicts
    stops every thread, the event loop's too); the record count is
    checked against the header when the iterator is exhausted."""
    lsn, kind = parse_layer_name(name)
    path = os.path.join(ckpt_dir, name)
    try:
        with open(path, "rb") as f:
            buf = f.read()
    except OSError as exc:
        raise CheckpointCorrupt("layer %s unreadable: %s" % (name, exc))
    valid, records = _scan_windowed(buf)
    if valid != len(buf):
        raise CheckpointCorrupt("layer %s: bad frame at byte %d of %d"
                                % (name, valid, len(buf)))
    if len(records) < 2:
        raise CheckpointCorrupt("layer %s: no header and trailer" % name)

    def frame(i: int):
        off, length = records[i]
        try:
            return decode_op(buf[off:off + length])
        except ValueError:
            raise CheckpointCorrupt("layer %s: undecodable frame" % name)

    header, trailer = frame(0), frame(-1)
    if not isinstance(header, dict) or header.get("ckpt") != "header":
        raise CheckpointCorrupt("layer %s: no header" % name)
    if not isinstance(trailer, dict) or trailer.get("ckpt") != "trailer":
        raise CheckpointCorrupt("layer %s: no trailer (truncated)" % name)
    if (header.get("lsn"), header.get("kind")) != (lsn, kind):
        raise CheckpointCorrupt("layer %s: header says %r at %r"
                                % (name, header.get("kind"),
                                   header.get("lsn")))
    if header.get("count") != trailer.get("count"):
        raise CheckpointCorrupt("layer %s: header counts %r, trailer %r"
                                % (name, header.get("count"),
                                   trailer.get("count")))

    def ops() -> Iterator[dict]:
        count = 0
        for i in range(1, len(records) - 1):
            op = frame(i)
            if not isinstance(op, dict) or op.get("op") != "batch" \
                    or not isinstance(op.get("ops"), list):
                raise CheckpointCorrupt("layer %s: unexpected frame" % name)
            count += len(op["ops"])
            yield op
        if count != header["count"]:
            raise CheckpointCorrupt("layer %s: header counts %r, file "
                                    "holds %d" % (name, header["count"],
                                                  count))
    return header, ops()


def read_layer(ckpt_dir: str, name: str) -> Tuple[dict, List[dict]]:
    """``open_layer`` with every batch op decoded and checked."""
    header, ops = open_layer(ckpt_dir, name)
    return header, list(ops)


def manifest_layers(manifest: dict) -> List[str]:
    """The layer names of a format-2 manifest, shape-checked."""
    names = manifest.get("layers")
    if not isinstance(names, list) or not names or \
            not all(isinstance(n, str) for n in names):
        raise CheckpointCorrupt("manifest names no layers")
    return names


def load_layers(data_dir: str, manifest: dict
                ) -> Tuple[Dict[str, object], List[dict]]:
    """The kv a format-2 ``manifest`` describes, read from
    ``<data_dir>/ckpt/``: the base, then each delta in order.  Pure: it
    reads files and raises ``CheckpointCorrupt`` rather than returning
    anything partial.  Also returns the layers' descriptions."""
    ckpt_dir = os.path.join(data_dir, CKPT_DIR)
    kv: Dict[str, object] = {}
    layers: List[dict] = []
    below = 0
    for i, name in enumerate(manifest_layers(manifest)):
        header, ops = open_layer(ckpt_dir, name)
        if header["kind"] != ("base" if i == 0 else "delta"):
            raise CheckpointCorrupt("layer %s: a %s at position %d"
                                    % (name, header["kind"], i))
        if header.get("parent") != below or (i and header["lsn"] <= below):
            raise CheckpointCorrupt(
                "layer %s: parent %r, but the layer below is at %d"
                % (name, header.get("parent"), below))
        below = header["lsn"]
        try:
            for op in ops:
                apply_op(kv, op)
        except (KeyError, TypeError, AttributeError):
            raise CheckpointCorrupt("layer %s: malformed record" % name)
        layers.append({"name": name, "kind": header["kind"],
                       "lsn": header["lsn"], "records": header["count"],
                       "bytes": os.path.getsize(
                           os.path.join(ckpt_dir, name))})
    if below > int(manifest.get("lsn", 0)):
        raise CheckpointCorrupt("layer %s is past the manifest's lsn"
                                % layers[-1]["name"])
    return kv, layers


def merge_layers(data_dir: str, names: List[str]) -> dict:
    """Compaction: fold the named layer FILES (never the live kv) into
    one new base at the newest layer's LSN.  The last writer wins and
    tombstones are dropped, so the base holds exactly the live keys.
    Returns the new base's description; publishing it is the caller's."""
    kv, layers = load_layers(data_dir, {"lsn": parse_layer_name(names[-1])[0],
                                        "layers": names})
    return write_layer(os.path.join(data_dir, CKPT_DIR), "base",
                       layers[-1]["lsn"], 0, kv.items(), len(kv))


def merge_layers_offloaded(data_dir: str, names: List[str]) -> dict:
    """``merge_layers``, in a child process once the layers are large.

    A merge is a pure function of files, and for a big base it is
    seconds of interpreter work: decoding and re-encoding every record.
    In an executor thread that work holds the GIL in slices and sets off
    cyclic-GC passes that stop the event loop's thread too, for longer
    the larger the database.  A child process shares neither.  Small
    merges stay in the calling thread: they cost less than the spawn."""
    ckpt_dir = os.path.join(data_dir, CKPT_DIR)
    total = 0
    for name in names:
        try:
            total += os.path.getsize(os.path.join(ckpt_dir, name))
        except OSError:
            pass                # merge_layers reports the missing layer
    if total < MERGE_IN_CHILD_BYTES:
        return merge_layers(data_dir, names)
    env = dict(os.environ)
    root = os.path.dirname(os.path.dirname(os.path.dirname(
        os.path.dirname(os.path.abspath(__file__)))))
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    res = subprocess.run(
        [sys.executable, "-m", "manatee_amd.db.waldb.ckpt", "merge",
         data_dir] + list(names),
        stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
        stderr=subprocess.PIPE, env=env)
    if res.returncode != 0:
        err = res.stderr.decode("utf-8", "replace").strip().splitlines()
        raise CheckpointCorrupt("layer merge failed (exit %d): %s"
                                % (res.returncode,
                                   err[-1] if err else "no output"))
    return json.loads(res.stdout)


def remove_unreferenced(data_dir: str, keep: Iterable[str]) -> List[str]:
    """Start-up sweep of ``ckpt/``: whatever the manifest does not name
    — superseded layers, the ``*.tmp`` of an interrupted write — goes."""
    ckpt_dir = os.path.join(data_dir, CKPT_DIR)
    keep = set(keep)
    removed = []
    try:
        names = os.listdir(ckpt_dir)
    except OSError:
        return removed
    for name in names:
        if name not in keep:
            try:
                os.unlink(os.path.join(ckpt_dir, name))
                removed.append(name)
            except OSError:
                pass
    return removed


def unlink_layers(data_dir: str, names: Iterable[str]) -> None:
    for name in names:
        try:
            os.unlink(os.path.join(data_dir, CKPT_DIR, name))
        except OSError:
            pass


def dump_manifest(lsn: int, layers: List[dict]) -> dict:
    return {"format": MANIFEST_FORMAT, "lsn": lsn,
            "layers": [layer["name"] for layer in layers]}



def main(argv=None) -> int:
    """``python -m manatee_amd.db.waldb.ckpt merge DATA_DIR LAYER...`` —
    the child side of ``merge_layers_offloaded``: prints the new base's
    description as JSON."""
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) < 3 or argv[0] != "merge":
        sys.stderr.write("usage: ckpt merge DATA_DIR LAYER...\n")
        return 2
    print(json.dumps(merge_layers(argv[1], argv[2:])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
