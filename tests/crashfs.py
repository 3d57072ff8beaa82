"""Record the file operations of in-process code and rebuild the
directories a crash could have left behind.

``Recorder(root)`` is a context manager.  While it is active every
mutation under ``root`` is appended to ``ops``, in order and from all
threads: file creation and truncation (``os.open`` with ``O_CREAT`` or
``O_TRUNC``, the builtin ``open`` in a writing mode), ``os.pwrite``,
writes / truncates / flushes through file objects opened for writing
(the builtin ``open`` and ``os.fdopen`` return a thin proxy for those),
``os.ftruncate``, ``os.fsync`` (of a file or of a directory;
descriptors are resolved through ``/proc/self/fd``), ``os.replace`` /
``os.rename`` / ``os.unlink`` and ``os.mkdir`` (``os.makedirs`` creates
through the patched ``os.mkdir``).  ``mark(label)`` adds an entry of
the test's own, which is how a model is tied to a position in the
trace.  Everything patched is restored on exit; product code is not
touched.

A file object's writes are logged when they reach the descriptor — at
``flush``, ``close``, ``fileno``, ``seek`` or ``truncate`` — as ONE
write, which is what the interpreter's buffer does with them.

``Recorder.verify()`` is the self-check every scenario must pass:
applying the whole trace to the starting image gives a tree
byte-identical to the real directory.  It proves the recorder missed no
write path (a child process that wrote would fail it).

Operations (tuples; paths relative to the root, ``""`` is the root):

    ("create", path, truncated)     ("pwrite", path, offset, bytes)
    ("truncate", path, size)        ("fsync", path, is_dir)
    ("rename", src, dst)            ("unlink", path)
    ("mkdir", path)                 ("mark", label)

Crash models
------------

``process_images`` — ``kill -9``.  The kernel has everything a system
call returned from, so the image at crash point ``i`` is the starting
image plus the first ``i`` operations, for every ``i`` from 0 to N.
Marks and fsyncs change nothing on disk, so the crash points before
them are folded into the next one that precedes a mutation (the same
bytes, and the later point has the stricter floor).  A write of ``n``
bytes is also cut to its first ``m`` bytes, ``m`` in ``{1, 7, 8, n//2,
n-1}`` clipped to ``0 < m < n``.

``powerloss_images`` — the machine loses power.

* A file's content is what it was at its last ``fsync`` (files of the
  starting image: what they held then), or, as the other choice,
  everything written.
* A directory's operations — link, rename, unlink, mkdir — up to its
  last directory fsync are durable.
* Of its later operations any prefix of that directory's own sequence
  may have survived, independently per directory.  The builder
  enumerates none or all per directory, crossed with the two content
  choices: at most ``2^dirs * 2`` images per crash point (identical
  ones are folded).
* ``file_fsync_persists_entry``: ``True`` is what journalled file
  systems do — an fsync of a file also makes every earlier operation in
  its directory durable; ``False`` is the strict reading — only a
  directory fsync does.

Power-loss crash points are the operations that change durability: just
before and just after every fsync, plus the start and the end of the
trace.  The starting image is taken as durable.
"""

import builtins
import hashlib
import itertools
import os
import shutil
import threading

MUTATING = ("create", "pwrite", "truncate", "rename", "unlink", "mkdir")
NAMESPACE = ("create", "rename", "unlink", "mkdir")
TORN = (1, 7, 8)


def snapshot(root, exclude=()):
    """``(dirs, files)`` of a real directory: relative directory names
    (the root is ``""``) and ``{relative path: bytes}``."""
    dirs, files = {""}, {}
    for base, dnames, fnames in os.walk(root):
        rel = os.path.relpath(base, root)
        rel = "" if rel == "." else rel
        for d in dnames:
            dirs.add(os.path.join(rel, d))
        for name in fnames:
            path = os.path.join(rel, name)
            if path in exclude:
                continue
            with open(os.path.join(base, name), "rb") as f:
                files[path] = f.read()
    return dirs, files


class Image:
    """One directory tree in memory."""

    def __init__(self, dirs, files, label=""):
        self.dirs, self.files, self.label = set(dirs), dict(files), label

    def fingerprint(self):
        h = hashlib.sha1()
        for d in sorted(self.dirs):
            h.update(b"d" + d.encode() + b"\0")
        for path in sorted(self.files):
            data = self.files[path]
            h.update(b"f" + path.encode() + b"\0%d\0" % len(data) + data)
        return h.digest()

    def materialize(self, dest):
        """Make ``dest`` exactly this tree."""
        shutil.rmtree(dest, ignore_errors=True)
        os.makedirs(dest)
        for d in sorted(self.dirs):
            if d:
                os.makedirs(os.path.join(dest, d), exist_ok=True)
        for path, data in self.files.items():
            with open(os.path.join(dest, path), "wb") as f:
                f.write(data)


def _splice(old, off, data):
    if off > len(old):
        old = old + b"\0" * (off - len(old))
    return old[:off] + data + old[off + len(data):]


def _resize(old, size):
    return old[:size] + b"\0" * (size - len(old))


class _Tree:
    """The true history: names, inodes, their bytes, and the bytes each
    inode had at its last fsync."""

    def __init__(self, start):
        dirs, files = start
        self.dirs = set(dirs)
        self.names = {}
        self.data = {}
        self.durable = {}
        for path, data in files.items():
            ino = len(self.data)
            self.names[path] = ino
            self.data[ino] = self.durable[ino] = data

    def apply(self, op):
        """Apply one operation; returns the inode a ``create`` made (or
        None if the file existed)."""
        kind = op[0]
        if kind == "create":
            _k, path, truncated = op
            if path not in self.names:
                ino = len(self.data)
                self.names[path] = ino
                self.data[ino] = b""
                return ino
            if truncated:
                self.data[self.names[path]] = b""
        elif kind == "pwrite":
            ino = self.names[op[1]]
            self.data[ino] = _splice(self.data[ino], op[2], op[3])
        elif kind == "truncate":
            ino = self.names[op[1]]
            self.data[ino] = _resize(self.data[ino], op[2])
        elif kind == "rename":
            if op[1] in self.dirs:
                raise NotImplementedError("directory rename %r" % (op,))
            self.names[op[2]] = self.names.pop(op[1])
        elif kind == "unlink":
            del self.names[op[1]]
        elif kind == "mkdir":
            self.dirs.add(op[1])
        elif kind == "fsync" and not op[2]:
            ino = self.names[op[1]]
            self.durable[ino] = self.data[ino]
        return None

    def image(self, label=""):
        return Image(self.dirs, {p: self.data[i]
                                 for p, i in self.names.items()}, label)


def apply_all(start, ops):
    tree = _Tree(start)
    for op in ops:
        tree.apply(op)
    return tree.image("whole trace")


def process_images(start, ops):
    """Every ``kill -9`` image of the trace: yields ``(i, image)`` where
    ``i`` operations were complete (``image.label`` says how much of the
    next one, if any)."""
    tree = _Tree(start)
    for i, op in enumerate(ops):
        if op[0] in MUTATING:
            yield i, tree.image("process @%d before %s" % (i, op[0]))
            if op[0] == "pwrite":
                n = len(op[3])
                for m in sorted(set(TORN + (n // 2, n - 1))):
                    if 0 < m < n:
                        img = tree.image("process @%d, %d of %d bytes of "
                                         "the write to %s" % (i, m, n, op[1]))
                        img.files[op[1]] = _splice(img.files[op[1]], op[2],
                                                   op[3][:m])
                        yield i, img
        tree.apply(op)
    yield len(ops), tree.image("process @%d, end of trace" % len(ops))


def _parent(path):
    return os.path.dirname(path)


def powerloss_points(ops):
    """Crash points (count of completed operations) where durability
    changes: around every fsync, plus both ends of the trace."""
    points = {0, len(ops)}
    for i, op in enumerate(ops):
        if op[0] == "fsync":
            points.update((i, i + 1))
    return sorted(points)


def powerloss_images(start, ops, file_fsync_persists_entry):
    """Every power-loss image of the trace under the module's model:
    yields ``(i, image)``."""
    points = set(powerloss_points(ops))
    tree = _Tree(start)
    cutoff = {}                 # directory -> ops below this are durable
    created = {}                # op index of a create -> its new inode
    for i in range(len(ops) + 1):
        if i in points:
            for img in _powerloss_at(start, ops, i, tree, cutoff, created):
                yield i, img
        if i == len(ops):
            break
        op = ops[i]
        ino = tree.apply(op)
        if ino is not None:
            created[i] = ino
        if op[0] == "fsync":
            if op[2]:
                cutoff[op[1]] = i
            elif file_fsync_persists_entry:
                cutoff[_parent(op[1])] = i


def _powerloss_at(start, ops, i, tree, cutoff, created):
    pending = set()             # directories with operations in doubt
    for k in range(i):
        op = ops[k]
        if op[0] in NAMESPACE:
            d = _parent(op[2] if op[0] == "rename" else op[1])
            if op[0] == "rename" and _parent(op[1]) != d:
                raise NotImplementedError("rename across directories")
            if k >= cutoff.get(d, 0) and not (
                    op[0] == "create" and k not in created):
                pending.add(d)
    pending = sorted(pending)
    start_names = _Tree(start).names    # the starting image's inodes
    seen = set()
    for keep in itertools.product((False, True), repeat=len(pending)):
        kept = {d for d, yes in zip(pending, keep) if yes}
        dirs = set(start[0])
        names = dict(start_names)
        for k in range(i):
            op = ops[k]
            if op[0] not in NAMESPACE:
                continue
            d = _parent(op[2] if op[0] == "rename" else op[1])
            if not (k < cutoff.get(d, 0) or d in kept):
                continue
            if op[0] == "create":
                if k in created:
                    names[op[1]] = created[k]
            elif op[0] == "rename":
                if op[1] in names:
                    names[op[2]] = names.pop(op[1])
            elif op[0] == "unlink":
                names.pop(op[1], None)
            else:
                dirs.add(op[1])
        # a directory whose own mkdir did not survive takes its files along
        dirs = {d for d in dirs if all(
            d[:n] in dirs for n, c in enumerate(d) if c == os.sep)}
        names = {p: ino for p, ino in names.items() if _parent(p) in dirs}
        for everything in (False, True):
            content = tree.data if everything else tree.durable
            img = Image(dirs, {p: content.get(ino, b"")
                               for p, ino in names.items()},
                        "powerloss @%d, kept directory operations of %r, "
                        "%s" % (i, sorted(kept), "all written bytes"
                                if everything else "fsynced bytes"))
            fp = img.fingerprint()
            if fp not in seen:
                seen.add(fp)
                yield img


class _FileProxy:
    """A file object opened for writing under the root: what it writes
    is logged when it reaches the descriptor."""

    def __init__(self, rec, f, binary, pos):
        self._rec, self._f, self._binary = rec, f, binary
        self._pos = pos
        self._pending = bytearray()
        self._pending_at = pos

    def _log_pending(self):
        if self._pending:
            self._rec._log_fd(self._f.fileno(), "pwrite", self._pending_at,
                              bytes(self._pending))
            self._pending = bytearray()
        self._pending_at = self._pos

    def write(self, data):
        raw = bytes(data) if self._binary else \
            data.encode(self._f.encoding or "utf-8")
        with self._rec._lock:
            n = self._f.write(data)
            self._pending += raw
            self._pos += len(raw)
        return n

    def flush(self):
        with self._rec._lock:
            self._f.flush()
            self._log_pending()

    def fileno(self):
        self.flush()
        return self._f.fileno()

    def seek(self, offset, whence=0):
        self.flush()
        self._pos = self._pending_at = self._f.seek(offset, whence)
        return self._pos

    def truncate(self, size=None):
        self.flush()
        with self._rec._lock:
            size = self._f.truncate(self._pos if size is None else size)
            self._rec._log_fd(self._f.fileno(), "truncate", size)
        return size

    def close(self):
        if not self._f.closed:
            self.flush()
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __iter__(self):
        return iter(self._f)

    def __getattr__(self, name):
        return getattr(self._f, name)


class Recorder:
    PATCHED = ("open", "fdopen", "pwrite", "ftruncate", "fsync", "replace",
               "rename", "unlink", "mkdir")

    def __init__(self, root):
        self.root = os.path.realpath(root)
        self.ops = []
        self.start = None
        self._lock = threading.RLock()
        self._real = {}

    # ------------------------------------------------------------ plumbing
    def _rel(self, path):
        """``path`` relative to the root, or None if it is elsewhere."""
        if not isinstance(path, (str, bytes, os.PathLike)):
            return None
        path = os.fsdecode(os.fspath(path))
        path = os.path.abspath(path)
        if path != self.root and not path.startswith(self.root + os.sep):
            path = os.path.join(os.path.realpath(os.path.dirname(path)),
                                os.path.basename(path))
        if path == self.root:
            return ""
        if path.startswith(self.root + os.sep):
            return path[len(self.root) + 1:]
        return None

    def _fd_rel(self, fd):
        try:
            return self._rel(os.readlink("/proc/self/fd/%d" % fd))
        except OSError:
            return None

    def _log(self, *op):
        with self._lock:
            self.ops.append(op)

    def _log_fd(self, fd, kind, *rest):
        rel = self._fd_rel(fd)
        if rel is not None and not rel.endswith(" (deleted)"):
            self._log(kind, rel, *rest)

    def mark(self, label):
        self._log("mark", label)

    # ------------------------------------------------------------- patches
    def _os_open(self, path, flags, mode=0o777, *, dir_fd=None):
        real = self._real["open"]
        rel = self._rel(path) if dir_fd is None else None
        if rel is None or not flags & (os.O_CREAT | os.O_TRUNC):
            return real(path, flags, mode, dir_fd=dir_fd)
        with self._lock:
            existed = os.path.lexists(path)
            fd = real(path, flags, mode)
            if not existed or flags & os.O_TRUNC:
                self._log("create", rel, bool(flags & os.O_TRUNC))
            return fd

    def _os_pwrite(self, fd, data, offset):
        with self._lock:
            n = self._real["pwrite"](fd, data, offset)
            self._log_fd(fd, "pwrite", offset, bytes(data)[:n])
            return n

    def _os_ftruncate(self, fd, length):
        with self._lock:
            self._real["ftruncate"](fd, length)
            self._log_fd(fd, "truncate", length)

    def _os_fsync(self, fd):
        if hasattr(fd, "fileno"):
            fd = fd.fileno()
        with self._lock:
            self._real["fsync"](fd)
            rel = self._fd_rel(fd)
            if rel is not None:
                self._log("fsync", rel, os.path.isdir(
                    os.path.join(self.root, rel)))

    def _os_rename(self, which, src, dst, **kw):
        with self._lock:
            self._real[which](src, dst, **kw)
            rsrc, rdst = self._rel(src), self._rel(dst)
            if rsrc is None and rdst is None:
                return
            if kw or rsrc is None or rdst is None:
                raise NotImplementedError("rename across the root: %r -> %r"
                                          % (src, dst))
            self._log("rename", rsrc, rdst)

    def _os_unlink(self, path, *, dir_fd=None):
        with self._lock:
            self._real["unlink"](path, dir_fd=dir_fd)
            rel = self._rel(path) if dir_fd is None else None
            if rel is not None:
                self._log("unlink", rel)

    def _os_mkdir(self, path, mode=0o777, *, dir_fd=None):
        with self._lock:
            self._real["mkdir"](path, mode, dir_fd=dir_fd)
            rel = self._rel(path) if dir_fd is None else None
            if rel is not None:
                self._log("mkdir", rel)

    def _builtin_open(self, file, mode="r", *args, **kw):
        real = self._real["builtins.open"]
        rel = self._rel(file)
        if rel is None or not set(mode) & set("wax+"):
            return real(file, mode, *args, **kw)
        with self._lock:
            existed = os.path.lexists(file)
            f = real(file, mode, *args, **kw)
            if not existed or "w" in mode:
                self._log("create", rel, "w" in mode)
            pos = os.fstat(f.fileno()).st_size if "a" in mode else 0
            return _FileProxy(self, f, "b" in mode, pos)

    def _os_fdopen(self, fd, mode="r", *args, **kw):
        f = self._real["fdopen"](fd, mode, *args, **kw)
        if set(mode) & set("wax+") and self._fd_rel(fd) is not None:
            pos = os.fstat(fd).st_size if "a" in mode else 0
            return _FileProxy(self, f, "b" in mode, pos)
        return f

    def __enter__(self):
        self.start = snapshot(self.root)
        for name in self.PATCHED:
            self._real[name] = getattr(os, name)
        self._real["builtins.open"] = builtins.open
        os.open = self._os_open
        os.fdopen = self._os_fdopen
        os.pwrite = self._os_pwrite
        os.ftruncate = self._os_ftruncate
        os.fsync = self._os_fsync
        os.replace = lambda s, d, **kw: self._os_rename("replace", s, d, **kw)
        os.rename = lambda s, d, **kw: self._os_rename("rename", s, d, **kw)
        os.unlink = self._os_unlink
        os.mkdir = self._os_mkdir
        builtins.open = self._builtin_open
        return self

    def __exit__(self, *exc):
        for name in self.PATCHED:
            setattr(os, name, self._real[name])
        builtins.open = self._real["builtins.open"]

    # ---------------------------------------------------------- self-check
    def verify(self, exclude=("waldb.pid",)):
        """The trace applied to the starting image must be the directory
        as it is now, byte for byte (``exclude`` left out)."""
        want = apply_all(self.start, self.ops)
        dirs, files = snapshot(self.root, exclude)
        got = {p: d for p, d in want.files.items() if p not in exclude}
        assert want.dirs == dirs, (sorted(want.dirs), sorted(dirs))
        assert sorted(got) == sorted(files), (sorted(got), sorted(files))
        for path in files:
            assert got[path] == files[path], \
                "the trace does not reproduce %s" % path
