"""Replication core shared by the database front-ends.

``ReplCore`` is everything about a waldb process that is not a client
wire protocol: identity and timelines, crash recovery, checkpoints, the
WAL flush loop, the synchronous-commit gate, streaming replication in
and out, online promote and conf reload.  ``db/waldb/server.py`` and
``db/minipg/server.py`` put a protocol in front of it.

Durability/replication semantics mirror the reference's PostgreSQL setup:
``synchronous_commit=remote_write`` — a put is acknowledged only once the
named synchronous standby reports the record *written* (etc/postgresql.conf;
SURVEY.md §6).  A promote trigger file bumps the timeline and records the
switch point, which is how divergence of a deposed primary is detected
(the xlog-divergence problem, ref docs/xlog-diverge.md).
"""

from __future__ import annotations

import asyncio
import dataclasses
import json
import os
import signal
import struct
import sys
import time
import uuid
from typing import Dict, Iterator, List, Optional, Tuple

from ...common import dial
from ...common import lsn as lsnmod
from ...common.logging import Logger
from . import ckpt as ckptmod
from . import rewind as rewindmod
from .ckpt import CheckpointCorrupt, CheckpointFormatError  # noqa: F401
from .wal import (DEFAULT_SEGMENT_BYTES, Wal, WalGone, _codec, encode_op,
                  decode_op, parse_frames)
from .wal import fsync_dir as _fsync_dir

CONF_NAME = "waldb.conf"
IDENT_NAME = "waldb_ident.json"
CKPT_NAME = "checkpoint.json"
PROMOTE_TRIGGER = "promote"
_U32 = struct.Struct(">I")

# checkpoint + WAL-retention defaults (overridable in the conf — the
# pg_overrides analogue, ref lib/postgresMgr.js:118-161)
DEFAULT_CKPT_WAL_BYTES = 8 * 1024 * 1024
DEFAULT_WAL_KEEP_BYTES = 32 * 1024 * 1024
# disconnect a replica that accepts no bytes for this long (the
# PostgreSQL wal_sender_timeout defense: a SIGSTOPped/partitioned
# standby must not pin WAL retention and a replica slot forever)
DEFAULT_WAL_SENDER_TIMEOUT_S = 60.0
CKPT_MODES = ("full", "incremental")


@dataclasses.dataclass(frozen=True)
class Settings:
    """What a front-end reads from its conf files.  Immutable: a reload
    builds a new object and the core adopts it whole, or keeps the old."""
    role: str = "primary"
    listen_ip: str = "127.0.0.1"
    port: str = "0"
    name: str = "standby"
    read_only: bool = False
    sync_standby: Optional[str] = None
    upstream: Optional[str] = None          # "host:port"
    trigger_path: str = ""
    ckpt_wal_bytes: int = DEFAULT_CKPT_WAL_BYTES
    wal_keep_bytes: int = DEFAULT_WAL_KEEP_BYTES
    wal_segment_bytes: int = DEFAULT_SEGMENT_BYTES
    wal_sender_timeout_s: float = DEFAULT_WAL_SENDER_TIMEOUT_S
    ckpt_mode: str = "full"                 # "full" | "incremental"


def conf_value(v: str) -> str:
    """A conf value without surrounding blanks and quotes."""
    return v.strip().strip("'").strip('"')


def _ckpt_mode(v: str) -> str:
    if v not in CKPT_MODES:
        raise ValueError("checkpoint_mode %r" % (v,))
    return v


# conf key, Settings field, parser — applied in this order
_KNOBS = (("checkpoint_wal_bytes", "ckpt_wal_bytes", int),
          ("wal_keep_bytes", "wal_keep_bytes", int),
          ("wal_segment_bytes", "wal_segment_bytes", int),
          ("wal_sender_timeout", "wal_sender_timeout_s", float),
          ("checkpoint_mode", "ckpt_mode", _ckpt_mode))
KNOB_NAMES = tuple(key for key, _field, _parse in _KNOBS)


def parse_knobs(raw: Dict[str, str], fallback: Settings,
                sender_timeout_unit_s: float) -> Settings:
    """``fallback`` with the tuning knobs present in ``raw`` applied.  An
    absent knob keeps the fallback's value; the first unparsable value
    ends the pass, so the knobs after it keep the fallback's too.
    ``wal_sender_timeout`` counts units of ``sender_timeout_unit_s``
    seconds (PostgreSQL writes milliseconds)."""
    applied = {}
    for key, field, parse in _KNOBS:
        if key in raw:
            try:
                applied[field] = parse(conf_value(raw[key]))
            except ValueError:
                break
    if "wal_sender_timeout_s" in applied:
        applied["wal_sender_timeout_s"] *= sender_timeout_unit_s
    return dataclasses.replace(fallback, **applied)


class _BufferedReader:
    """readline() view over leftover pipelined bytes + the stream —
    used when the chunked request framing of a front-end has read past
    a ``repl`` request before handing the socket to the replication
    path (the leftover bytes are the standby's first acks)."""

    def __init__(self, leftover: bytes, reader: asyncio.StreamReader):
        self._left = leftover
        self._reader = reader

    async def readline(self) -> bytes:
        if self._left:
            nl = self._left.find(b"\n")
            if nl >= 0:
                line = self._left[:nl + 1]
                self._left = self._left[nl + 1:]
                return line
            line, self._left = self._left, b""
            return line + await self._reader.readline()
        return await self._reader.readline()


class ReplicaConn:
    """Server-side state for one downstream replication connection
    (one row of pg_stat_replication, ref lib/adm.js:348-427)."""

    __slots__ = ("name", "sent_lsn", "write_lsn", "flush_lsn", "replay_lsn",
                 "writer", "wake")

    def __init__(self, name: str, writer):
        self.name = name
        self.sent_lsn = 0
        self.write_lsn = 0
        self.flush_lsn = 0
        self.replay_lsn = 0
        self.writer = writer
        self.wake = asyncio.Event()


class ReplCore:
    """One database process minus its client protocol.

    A front-end subclass supplies exactly three things:

    ``PID_FILE`` (with ``CONF_FILE``)
        file names in the data dir: the readiness marker written once
        the listener is up, and the conf file whose mtime is watched as
        a reload trigger.
    ``read_settings(prev) -> Settings``
        read the conf files; ``prev`` is the object in force (defaults
        on first load).  Must not touch ``self``: the core decides
        whether the result is adopted, and swaps ``self.settings`` whole.
    ``_handle_conn(reader, writer)``
        serve one accepted connection: commit through ``_append_write``
        + ``_await_commit``, read through ``get``/``count``/``scan``/
        ``replica_rows``/``_status``, hand ``repl`` to ``_handle_repl``.
    """

    def __init__(self, data_dir: str, log: Logger):
        self.data_dir = os.path.abspath(data_dir)
        self.log = log.child(component="waldb")
        self.kv: Dict[str, object] = {}
        self.wal = Wal(self.data_dir)
        self.settings = Settings()
        self.ckpt_lsn = 0
        self._last_ckpt_bytes = 0
        self._ckpt_running = False
        # keys touched since the last checkpoint (what an incremental
        # checkpoint writes), the layers the manifest on disk names, and
        # layer files a compaction superseded: those are unlinked one
        # generation late, see _retire_layers
        self._dirty: set = set()
        self._layers: List[dict] = []
        self._ckpt_garbage: List[str] = []
        self._ckpt_count = 0
        # of the last checkpoint: dirty keys it captured, records it wrote
        self._last_ckpt_dirty = 0
        self._last_ckpt_records = 0
        self._compact_count = 0
        self.ident: dict = {}
        self.replay_lsn = 0
        self.last_replay_time: Optional[float] = None
        self.upstream_status = "n/a"
        self.replicas: List[ReplicaConn] = []
        # last acked flush LSN per follower NAME, kept across disconnects:
        # a sync standby that blips while the primary writes past the keep
        # window must not be forced into a full restore (read-only storm)
        self._peer_acked: Dict[str, int] = {}
        self.commit_cond: Optional[asyncio.Condition] = None
        self._server: Optional[asyncio.AbstractServer] = None
        self._repl_task: Optional[asyncio.Task] = None
        self._repl_writer: Optional[asyncio.StreamWriter] = None
        self._repl_gen = 0
        self._flusher: Optional[asyncio.Task] = None
        self._start_time = time.time()

    # ------------------------------------------------------- settings/ident
    role = property(lambda self: self.settings.role)
    read_only = property(lambda self: self.settings.read_only)
    sync_standby = property(lambda self: self.settings.sync_standby)
    upstream = property(lambda self: self.settings.upstream)
    ckpt_wal_bytes = property(lambda self: self.settings.ckpt_wal_bytes)

    def _adopt(self, settings: Settings) -> None:
        self.settings = settings
        self.wal.segment_bytes = settings.wal_segment_bytes

    def load_ident(self) -> None:
        with open(os.path.join(self.data_dir, IDENT_NAME)) as f:
            self.ident = json.load(f)

    def save_ident(self) -> None:
        _write_json_atomic(os.path.join(self.data_dir, IDENT_NAME),
                           self.ident)

    timeline = property(lambda self: self.ident.get("timeline", 1))

    @property
    def history(self) -> List[dict]:
        """[{tl, at}] — timeline switch points (tl began at WAL offset at)."""
        return self.ident.get("history", [])

    def _bump_timeline(self, at: int) -> bool:
        """Consume the promote trigger, if present: start a new timeline
        at WAL offset ``at`` and record the switch point durably (pg_ctl
        promote analogue).  This is what fences a deposed primary: WAL it
        wrote past ``at`` is on a dead line of history and
        ``_check_follower`` refuses it."""
        trigger = self.settings.trigger_path
        if not os.path.exists(trigger):
            return False
        self.ident["timeline"] = self.timeline + 1
        self.ident["history"] = list(self.history) + [
            {"tl": self.ident["timeline"], "at": at}]
        self.save_ident()
        os.unlink(trigger)
        return True

    # -------------------------------------------------------------- startup
    async def start(self) -> None:
        self._adopt(self.read_settings(self.settings))
        if os.path.exists(os.path.join(self.data_dir,
                                       rewindmod.MARKER_NAME)):
            # a rewind was interrupted: WAL, checkpoint and ident may
            # belong to different histories until it is finished
            self.log.error("data directory holds an unfinished rewind; "
                           "REFUSING to start (run the rewind again)",
                           marker=rewindmod.MARKER_NAME)
            raise rewindmod.RewindPending(rewindmod.MARKER_NAME)
        self.load_ident()

        # recover: checkpoint (if any) + WAL tail replay
        self._load_checkpoint()
        end = self.wal.open(replay=self._apply_replay,
                            replay_from=self.ckpt_lsn)
        self.replay_lsn = max(end, self.replay_lsn)
        if self.role == "primary" and self._bump_timeline(end):
            self.log.info("promoted: timeline bumped",
                          timeline=self.timeline, at=end)

        self.commit_cond = asyncio.Condition()
        ip = self.settings.listen_ip
        self._server = await asyncio.start_server(
            self._handle_conn, ip, int(self.settings.port or "0"))
        port = self._server.sockets[0].getsockname()[1]
        self.log.info("waldb listening", ip=ip, port=port, role=self.role,
                      timeline=self.timeline,
                      wal_end=lsnmod.format_lsn(self.wal.end),
                      native_codec=_codec() is not None)
        # readiness marker for the manager (postmaster.pid analogue)
        with open(os.path.join(self.data_dir, self.PID_FILE), "w") as f:
            f.write("%d %d\n" % (os.getpid(), port))

        loop = asyncio.get_running_loop()
        loop.add_signal_handler(signal.SIGHUP, self._on_sighup)
        self._flusher = loop.create_task(self._flush_loop())
        if self.role == "standby":
            self._start_repl_client()

    def _on_sighup(self) -> None:
        """Reload the knobs that can change without a restart (sync names,
        read-only) — pg_ctl reload analogue (ref lib/postgresMgr.js
        _updateStandby :1195-1260 uses conf + SIGHUP only).  A
        standby→primary role change with the promote trigger present is
        an ONLINE promote (pg_ctl promote analogue): stop following the
        upstream, bump the timeline at the current WAL end, and start
        taking writes — no restart."""
        old = self.settings
        try:
            new = self.read_settings(old)
        except Exception as exc:
            self.log.error("conf reload failed", err=exc)
            return
        if old.port and new.port != old.port:
            # a conf naming a different port is not OURS (e.g. a foreign
            # conf that rode in with a dataset restore under a process
            # that should be dead) — never adopt another peer's identity
            self.log.error("conf reload names a different port; "
                           "REFUSING to adopt it",
                           our_port=old.port, conf_port=new.port)
            return
        self.log.info("conf reloaded", role=new.role,
                      sync_standby=new.sync_standby,
                      read_only=new.read_only)
        if old.role == "standby" and new.role == "primary":
            self._adopt(new)
            self._online_promote()
            return
        if old.role == "primary" and new.role == "standby":
            # demotion cannot be done online safely; the manager always
            # restarts for this path — stay primary until it does
            self.log.warn("primary->standby reload ignored (needs restart)")
            self._adopt(dataclasses.replace(new, role="primary"))
            return
        self._adopt(new)
        if (old.sync_standby, old.read_only) != \
                (new.sync_standby, new.read_only):
            # wake commit waiters to re-evaluate against the new rules
            asyncio.get_running_loop().create_task(self._notify_commits())
        if new.role == "standby" and old.upstream != new.upstream:
            self._sever_repl()
            self._start_repl_client()

    def _start_repl_client(self) -> None:
        self._repl_gen += 1
        self._repl_task = asyncio.get_running_loop().create_task(
            self._replication_client(self._repl_gen))

    @staticmethod
    def _abort(writer) -> None:
        """Drop a connection NOW: nothing buffered is flushed."""
        try:
            writer.transport.abort()
        except Exception:
            pass

    def _sever_repl(self) -> None:
        """Stop following the upstream NOW — synchronously.

        task.cancel() alone is NOT enough: Python 3.10's asyncio.wait_for
        can lose a cancellation that races the inner read's completion
        (bpo-42130, fixed in 3.12).  A lost cancel at promote left the
        promoted sync STREAMING FROM AND ACKING the deposed primary, which
        went on acknowledging writes the new timeline will never contain
        (docs/troubleshooting.md, "A deposed primary keeps acknowledging
        writes").  So: bump the generation (a cancel-surviving loop exits
        at its next iteration instead of reconnecting) and abort the live
        transport (an aborted socket carries no further acks — the old
        primary's gate closes at the promote instant)."""
        self._repl_gen += 1
        if self._repl_task is not None:
            # test seam: simulate bpo-42130 eating the cancel — the
            # regression test proves the gen+abort path alone severs
            if not os.environ.get("WALDB_TEST_EAT_REPL_CANCEL"):
                self._repl_task.cancel()
            self._repl_task = None
        w, self._repl_writer = self._repl_writer, None
        if w is not None:
            self._abort(w)

    def _online_promote(self) -> None:
        self._sever_repl()
        self.settings = dataclasses.replace(self.settings, upstream=None)
        self.upstream_status = "n/a"
        self._bump_timeline(self.wal.end)
        self.replay_lsn = self.wal.end
        # disconnect downstream replicas: they must re-handshake to adopt
        # the new timeline/history before consuming post-switch WAL
        for rep in list(self.replicas):
            try:
                rep.writer.close()
            except Exception:
                pass
        self.log.info("promoted online", timeline=self.timeline,
                      at=lsnmod.format_lsn(self.wal.end))
        asyncio.get_running_loop().create_task(self._notify_commits())

    async def _notify_commits(self) -> None:
        async with self.commit_cond:
            self.commit_cond.notify_all()

    def _conf_mtime(self) -> float:
        try:
            return os.stat(os.path.join(self.data_dir,
                                        self.CONF_FILE)).st_mtime
        except OSError:
            return 0.0

    async def _flush_loop(self) -> None:
        """Background fsync every 50 ms — local flush is decoupled from
        commit ack (remote_write semantics).  Also drives checkpoints and
        watches the conf file's mtime as a reload safety net (a SIGHUP
        delivered during interpreter startup is ignored by design)."""
        last = 0
        conf_mtime = self._conf_mtime()
        conf_tick = 0
        while True:
            await asyncio.sleep(0.05)
            if self.wal.end != last:
                try:
                    self.wal.fsync()
                    last = self.wal.end
                except OSError as exc:
                    # An fsync failure means durability is gone — the one
                    # property this engine exists to provide.  Crash loudly:
                    # the manager sees the unexpected exit and raises a
                    # fatal error event (like an unexpected postgres death,
                    # ref lib/postgresMgr.js:1736-1753).
                    self.log.error("WAL fsync failed; aborting", err=exc)
                    os._exit(2)
            conf_tick += 1
            if conf_tick >= 4:      # every 200 ms
                conf_tick = 0
                m = self._conf_mtime()
                if m != conf_mtime:
                    conf_mtime = m
                    self._on_sighup()
            if self.replay_lsn - self.ckpt_lsn >= self._ckpt_due_bytes() \
                    and not self._ckpt_running:
                asyncio.get_running_loop().create_task(self._checkpoint())

    # ---------------------------------------------------------- checkpoints
    def _load_checkpoint(self) -> None:
        path = os.path.join(self.data_dir, CKPT_NAME)
        try:
            with open(path) as f:
                ckpt = json.load(f)
        except FileNotFoundError:
            ckptmod.remove_unreferenced(self.data_dir, ())
            return
        except (OSError, ValueError):
            return
        # what is on disk decides, never the configured mode
        if "kv" not in ckpt and "format" in ckpt:
            if ckpt["format"] != ckptmod.MANIFEST_FORMAT:
                self.log.error("checkpoint.json has an unknown format; "
                               "REFUSING to start", format=ckpt["format"])
                raise CheckpointFormatError(
                    "checkpoint format %r" % (ckpt["format"],))
            try:
                self.kv, self._layers = ckptmod.load_layers(self.data_dir,
                                                            ckpt)
            except CheckpointCorrupt as exc:
                # never serve the kv without a layer the manifest names
                self.log.error("checkpoint layer corrupt; REFUSING to "
                               "start (rebuild this peer)", err=exc)
                raise
        else:
            self.kv = ckpt.get("kv", {})
        removed = ckptmod.remove_unreferenced(
            self.data_dir, [layer["name"] for layer in self._layers])
        if removed:
            self.log.info("removed unreferenced checkpoint files",
                          files=sorted(removed))
        self.ckpt_lsn = int(ckpt.get("lsn", 0))
        self.replay_lsn = self.ckpt_lsn
        try:
            self._last_ckpt_bytes = os.path.getsize(path)
        except OSError:
            pass
        self.log.info("checkpoint loaded",
                      lsn=lsnmod.format_lsn(self.ckpt_lsn),
                      keys=len(self.kv), layers=len(self._layers))

    def _ckpt_due_bytes(self) -> int:
        """New WAL after which the next checkpoint is due.

        Full mode, adaptive spacing: a checkpoint serializes the WHOLE
        kv, so requiring at least half the last image's size in new WAL
        keeps checkpoint I/O amortized O(1) per WAL byte — a big database
        no longer re-dumps hundreds of MB every 8 MB of appends (recovery
        stays bounded by ~2x the image size).  An incremental checkpoint
        costs O(dirty keys), so the configured spacing holds."""
        if self.settings.ckpt_mode == "incremental":
            return self.ckpt_wal_bytes
        return max(self.ckpt_wal_bytes, self._last_ckpt_bytes // 2)

    async def _checkpoint(self) -> None:
        """Write an atomic point-in-time image of the kv state at the
        current replay LSN, then recycle WAL segments no consumer can
        still need (bounded crash recovery + bounded snapshots — the
        PostgreSQL CHECKPOINT analogue)."""
        self._ckpt_running = True
        try:
            # fsync WAL BEFORE capturing the checkpoint LSN (PostgreSQL's
            # ordering): the background flush loop can lag appends by up to
            # 50 ms, and a checkpoint.lsn beyond the durable WAL end would
            # let post-crash recovery hand out LSNs below already-streamed
            # positions on the same timeline.
            self.wal.fsync()
            at = self.replay_lsn
            if self.settings.ckpt_mode == "incremental":
                await self._checkpoint_incremental(at)
            else:
                await self._checkpoint_full(at)
            self.ckpt_lsn = at
            self._ckpt_count += 1
            # retention floor: the checkpoint, minus the keep window,
            # and never past what a connected replica still needs
            keep = self.settings.wal_keep_bytes
            floor = at - keep
            for rep in self.replicas:
                floor = min(floor, rep.sent_lsn)
            # ... nor past what the NAMED sync standby last acked, even if
            # it is briefly disconnected (restart, network blip) — capped
            # at 8× the keep window so a long-dead sync cannot pin WAL
            # forever (it takes the restore path instead)
            if self.sync_standby and self._sync_replica() is None:
                acked = self._peer_acked.get(self.sync_standby)
                if acked is not None:
                    floor = min(floor, max(acked, at - 8 * keep))
            if floor > self.wal.start:
                self.wal.drop_below(floor)
            self.log.debug("checkpoint complete",
                           lsn=lsnmod.format_lsn(at),
                           wal_start=lsnmod.format_lsn(self.wal.start))
        except Exception as exc:
            self.log.error("checkpoint failed", err=exc)
        else:
            if self._compaction_due():
                try:
                    await self._compact()
                except Exception as exc:
                    # the layers and the manifest are as they were
                    self.log.error("checkpoint compaction failed", err=exc)
        finally:
            self._ckpt_running = False

    async def _checkpoint_full(self, at: int) -> None:
        """The classic image: the whole kv in ``checkpoint.json``."""
        captured, self._dirty = self._dirty, set()
        snap = dict(self.kv)   # single-threaded: consistent at `at`
        path = os.path.join(self.data_dir, CKPT_NAME)
        try:
            self._last_ckpt_bytes = \
                await asyncio.get_running_loop().run_in_executor(
                    None, lambda: _write_json_atomic(
                        path, {"lsn": at, "kv": snap},
                        separators=(",", ":")))
        except BaseException:
            self._dirty |= captured
            raise
        self._last_ckpt_dirty = len(captured)
        self._last_ckpt_records = len(snap)
        if self._layers or self._ckpt_garbage:
            # switched back from incremental: the image supersedes the
            # layers like a compaction does
            names = [layer["name"] for layer in self._layers]
            self._layers = []
            await asyncio.get_running_loop().run_in_executor(
                None, self._retire_layers, names)

    async def _checkpoint_incremental(self, at: int) -> None:
        """Write the keys touched since the last checkpoint as a delta
        layer and publish a manifest that names it.  The event loop does
        O(dirty keys) work; encoding and I/O happen in the executor.

        The exception is the first checkpoint after the mode is turned
        on (or after a classic image was loaded): there is no base yet,
        so one is written from the live kv — once, O(dataset)."""
        loop = asyncio.get_running_loop()
        ckpt_dir = os.path.join(self.data_dir, ckptmod.CKPT_DIR)
        captured, self._dirty = self._dirty, set()
        try:
            layers = list(self._layers)
            written = 0
            if not layers:
                items = list(self.kv.items())
                kind, parent = "base", 0
            else:
                kv, tomb = self.kv, ckptmod.TOMBSTONE
                items = [(k, kv.get(k, tomb)) for k in captured]
                kind, parent = "delta", layers[-1]["lsn"]
            if kind == "base" or items:
                if at <= parent and kind == "delta":
                    raise RuntimeError("delta at %d not above layer at %d"
                                       % (at, parent))
                layer = await loop.run_in_executor(
                    None, lambda: ckptmod.write_layer(
                        ckpt_dir, kind, at, parent, items, len(items)))
                layers.append(layer)
                written = layer["bytes"]
            path = os.path.join(self.data_dir, CKPT_NAME)
            manifest = ckptmod.dump_manifest(at, layers)
            written += await loop.run_in_executor(
                None, lambda: _write_json_atomic(
                    path, manifest, separators=(",", ":")))
        except BaseException:
            # nothing was published: these keys are still unsaved
            self._dirty |= captured
            raise
        if kind == "base":
            # a base written over a name that waits for deletion is live
            self._ckpt_garbage = [n for n in self._ckpt_garbage
                                  if n != layers[0]["name"]]
        self._layers = layers
        self._last_ckpt_bytes = written
        self._last_ckpt_dirty = len(captured)
        self._last_ckpt_records = len(items)

    def _compaction_due(self) -> bool:
        layers = self._layers
        if len(layers) < 2:
            return False
        return len(layers) > ckptmod.MAX_LAYERS or \
            sum(layer["bytes"] for layer in layers[1:]) >= layers[0]["bytes"]

    async def _compact(self) -> None:
        """Merge the layer FILES into one new base in the executor and
        publish a manifest that names only it.  Runs under
        ``_ckpt_running``; writes that arrive meanwhile are in the dirty
        set and go into the next delta.  Merging once the deltas reach
        the base's size keeps layer bytes written amortized O(1) per
        WAL byte."""
        loop = asyncio.get_running_loop()
        names = [layer["name"] for layer in self._layers]
        data_dir, at = self.data_dir, self.ckpt_lsn
        base = await loop.run_in_executor(
            None, lambda: ckptmod.merge_layers_offloaded(data_dir, names))
        path = os.path.join(data_dir, CKPT_NAME)
        await loop.run_in_executor(
            None, lambda: _write_json_atomic(
                path, ckptmod.dump_manifest(at, [base]),
                separators=(",", ":")))
        self._layers = [base]
        await loop.run_in_executor(None, self._retire_layers, names)
        self._compact_count += 1
        self.log.debug("checkpoint layers compacted", merged=len(names),
                       base=base["name"], bytes=base["bytes"])

    def _retire_layers(self, superseded: List[str]) -> None:
        """Deferred deletion.  A snapshot on the ``dir`` provider is a
        tar of the LIVE directory, so a copy can pair the previous
        manifest with the current files.  What the publication before
        this one superseded is unlinked now; what this one supersedes
        waits for the next.  Between such publications layers are only
        ever added.  Called in the executor, under ``_ckpt_running``:
        unlinking a large file takes the file system a while."""
        live = {layer["name"] for layer in self._layers}
        ckptmod.unlink_layers(self.data_dir,
                              [n for n in self._ckpt_garbage
                               if n not in live])
        self._ckpt_garbage = [n for n in superseded if n not in live]

    def checkpoint_info(self) -> dict:
        """The ``ckpt`` query: what the checkpointer has on disk and what
        it has done since start."""
        return {
            "ok": True,
            "mode": self.settings.ckpt_mode,
            "lsn": lsnmod.format_lsn(self.ckpt_lsn),
            "layers": [dict(layer, lsn=lsnmod.format_lsn(layer["lsn"]))
                       for layer in self._layers],
            "dirty_keys": len(self._dirty),
            "last_checkpoint_bytes": self._last_ckpt_bytes,
            "last_checkpoint_dirty": self._last_ckpt_dirty,
            "last_checkpoint_records": self._last_ckpt_records,
            "checkpoints": self._ckpt_count,
            "compactions": self._compact_count,
        }

    # -------------------------------------------------------------- replay
    def _apply_op(self, op: dict) -> None:
        kind = op.get("op")
        if kind == "put":
            self.kv[op["k"]] = op["v"]
            self._dirty.add(op["k"])
        elif kind == "del":
            self.kv.pop(op["k"], None)
            self._dirty.add(op["k"])
        elif kind == "batch":
            for sub in op.get("ops") or []:
                self._apply_op(sub)

    def _apply_replay(self, commit_lsn: int, payload: bytes) -> None:
        try:
            op = decode_op(payload)
        except ValueError:
            # a crc-valid record that fails to decode is corruption of a
            # kind recovery cannot repair — scream, never skip silently
            self.log.error("undecodable WAL record skipped",
                           lsn=lsnmod.format_lsn(commit_lsn))
            return
        self._apply_op(op)
        self.replay_lsn = commit_lsn
        self.last_replay_time = time.time()

    # ----------------------------------------------------- replication out
    async def _handle_repl(self, req: dict, reader, writer) -> None:
        if req.get("ident") != self.ident.get("ident"):
            writer.write(b'{"ok":false,"error":"ident-mismatch"}\n')
            await writer.drain()
            return
        # a follower that sends neither is judged, and answered, by the
        # rule from before the handshake carried them
        f_history = req.get("history")
        if not isinstance(f_history, list):
            f_history = None
        start = int(req.get("start_lsn", 0))
        err = self._check_follower(int(req.get("timeline", 0)), start,
                                   f_history)
        offer = None
        if not err and "wal_start" in req:
            offer, err = await self._handshake_offer(
                int(req["wal_start"]), int(req.get("timeline", 0)), start,
                f_history)
        if err:
            writer.write(json.dumps({"ok": False, "error": err})
                         .encode() + b"\n")
            await writer.drain()
            self.log.warn("refused replication request", error=err,
                          follower=req.get("name"))
            return
        resp = {"ok": True, "timeline": self.timeline,
                "history": self.history}
        resp.update(offer or {})
        writer.write((json.dumps(resp) + "\n").encode())
        await writer.drain()
        # A reconnect under the same name supersedes any stale sender:
        # after a partition/SIGSTOP the old TCP connection can sit
        # wedged (keepalives vanishing into retransmit) for up to
        # wal_sender_timeout, and while its row is first in
        # self.replicas the commit gate and pg_stat_replication read
        # its frozen ack LSNs — failovers then stall ~60 s for no
        # reason.  Abort the old transport and drop the row now.
        name = str(req.get("name", "?"))
        for old in [r for r in self.replicas if r.name == name]:
            self.log.warn("superseding stale replica connection",
                          name=name)
            self._abort(old.writer)
            if old in self.replicas:
                self.replicas.remove(old)
            old.wake.set()
        rep = ReplicaConn(name, writer)
        rep.sent_lsn = start = int(req["start_lsn"])
        self.log.info("replica connected", name=rep.name,
                      start=lsnmod.format_lsn(start))
        await self._stream_to_replica(rep, start, reader)
        self.log.info("replica disconnected", name=rep.name)

    async def _stream_to_replica(self, rep: ReplicaConn, start: int,
                                 reader: asyncio.StreamReader) -> None:
        """Pump WAL [start..∞) to a downstream, consuming its JSON acks."""
        self.replicas.append(rep)
        ack_task = asyncio.get_running_loop().create_task(
            self._consume_acks(rep, reader))

        async def drain() -> None:
            # wal_sender_timeout: a replica that stops reading would
            # otherwise block this drain forever, pinning the WAL
            # retention floor and a replica slot
            await asyncio.wait_for(rep.writer.drain(),
                                   self.settings.wal_sender_timeout_s)

        try:
            pos = start
            while True:
                # record-ALIGNED windows only: a raw byte window can cut
                # a record at the boundary, and the receiver applies
                # whole chunks (WalGone cannot happen: a connected
                # replica's sent_lsn pins the retention floor)
                chunk = self.wal.read_aligned(pos)
                if chunk:
                    rep.writer.write(_U32.pack(len(chunk)) + chunk)
                    await drain()
                    pos += len(chunk)
                    rep.sent_lsn = pos
                else:
                    rep.wake.clear()
                    try:
                        await asyncio.wait_for(rep.wake.wait(), 5.0)
                    except asyncio.TimeoutError:
                        # keepalive so a silent link is detected
                        rep.writer.write(_U32.pack(0))
                        await drain()
        except WalGone:
            self.log.warn("replica outlived WAL retention; disconnecting",
                          name=rep.name)
        except asyncio.TimeoutError:
            self.log.warn("replica accepted no bytes within the sender "
                          "timeout; disconnecting", name=rep.name,
                          timeout_s=self.settings.wal_sender_timeout_s)
        except (ConnectionError, OSError, asyncio.CancelledError):
            pass
        finally:
            ack_task.cancel()
            if rep in self.replicas:
                self.replicas.remove(rep)
            await self._notify_commits()

    async def _consume_acks(self, rep: ReplicaConn,
                            reader: asyncio.StreamReader) -> None:
        try:
            while True:
                line = await reader.readline()
                if not line:
                    return
                try:
                    ack = json.loads(line)
                except ValueError:
                    continue
                rep.write_lsn = int(ack.get("write_lsn", rep.write_lsn))
                rep.flush_lsn = int(ack.get("flush_lsn", rep.flush_lsn))
                rep.replay_lsn = int(ack.get("replay_lsn", rep.replay_lsn))
                self._peer_acked[rep.name] = max(
                    self._peer_acked.get(rep.name, 0), rep.flush_lsn)
                await self._notify_commits()
        except (ConnectionError, asyncio.CancelledError):
            return

    def _wake_replicas(self) -> None:
        for rep in self.replicas:
            rep.wake.set()

    def _sync_replica(self) -> Optional[ReplicaConn]:
        """The connected replica named by synchronous_standby_names."""
        name = self.settings.sync_standby
        return next((r for r in self.replicas if r.name == name), None)

    def _check_follower(self, timeline: int, start_lsn: int,
                        history: Optional[List[dict]] = None
                        ) -> Optional[str]:
        """May a follower at (timeline, start_lsn) with ``history`` (None:
        it sent none) stream from us?  Returns an error string or None;
        the rules are ``rewind.check_follower``."""
        return rewindmod.check_follower(
            timeline, history, start_lsn, self.timeline, self.history,
            self.wal.start, self.wal.end)

    def _wal_range(self, lo: int, hi: int) -> bytes:
        return self.wal.read(lo, hi - lo)

    async def _handshake_offer(self, f_start: int, timeline: int,
                               start_lsn: int,
                               history: Optional[List[dict]]):
        """``(offer, None)`` for a follower ``_check_follower`` accepted —
        the CRC-32 of our WAL in the window below ``start_lsn``, which it
        compares with its own bytes (``rewind.handshake_offer``) — or
        ``(None, error)`` if a checkpoint recycled what it needs while
        the window was read."""
        while True:
            window = rewindmod.probe_window(f_start, self.wal.start,
                                            start_lsn)
            crc = 0
            try:
                # a slice at a time, like rewind_probe
                for crc in rewindmod.crc_slices(self._wal_range, window,
                                                start_lsn):
                    await asyncio.sleep(0)
            except (WalGone, IOError):
                err = self._check_follower(timeline, start_lsn, history)
                if err or window >= self.wal.start:
                    return None, err or "wal-gone"
                continue
            return {"window_start": window, "crc32": crc}, None

    async def rewind_probe(self, req: dict) -> dict:
        """Answer a diverged peer that wants to rewind (``rewind.py``):
        where its history and ours part ways, and the CRC-32 of our WAL
        in the window just below that point, which it compares with its
        own bytes.  Changes no state."""
        if req.get("ident") != self.ident.get("ident"):
            return {"ok": False, "error": "ident-mismatch"}
        try:
            _tl, fork = rewindmod.fork_point(
                int(req.get("timeline", 0)), req.get("history") or [],
                int(req["wal_end"]), self.timeline, self.history,
                self.wal.end)
            start = rewindmod.probe_window(int(req["wal_start"]),
                                           self.wal.start, fork)
        except (KeyError, TypeError, ValueError):
            return {"ok": False, "error": "bad rewind-probe request"}
        if start >= fork:
            return {"ok": False, "error": "unverifiable"}
        # a slice at a time: one CRC over the whole window would hold
        # the event loop (and every commit ack) for its duration
        crc = 0
        try:
            for crc in rewindmod.crc_slices(self._wal_range, start, fork):
                await asyncio.sleep(0)
        except (WalGone, IOError):
            # a checkpoint recycled the window while we were reading it
            return {"ok": False, "error": "unverifiable"}
        return {"ok": True, "timeline": self.timeline,
                "history": self.history, "fork_lsn": fork,
                "window_start": start, "crc32": crc}

    # ------------------------------------------------------ replication in
    async def _replication_client(self, gen: int) -> None:
        """Standby: follow primary_conninfo, append + apply, ack.

        ``gen`` guards against a cancellation this task never saw
        (bpo-42130, see _sever_repl): a superseded generation must stop
        — reconnecting would re-open the ack channel a promote or
        reconfigure just severed."""
        while self._repl_gen == gen:
            try:
                await self._follow_upstream_once(gen)
            except asyncio.CancelledError:
                return
            except Exception as exc:
                if self.upstream_status != "diverged":
                    self.upstream_status = "disconnected"
                self.log.warn("replication connection failed", err=exc,
                              status=self.upstream_status)
            # diverged is unrecoverable without a restore; keep serving
            # reads and let the manager notice via status
            await asyncio.sleep(
                1.0 if self.upstream_status == "diverged" else 0.2)

    def _ack_payload(self) -> bytes:
        return (json.dumps({"write_lsn": self.wal.end,
                            "flush_lsn": self.wal.end,
                            "replay_lsn": self.replay_lsn})
                + "\n").encode()

    async def _verify_handshake(self, resp: dict) -> bool:
        """``rewind.handshake_verify`` a slice at a time: a standby
        serves reads while it hashes.  An answer without a window (an
        upstream that sends none, or a follower with no WAL below its
        end) verifies nothing and passes."""
        end = self.wal.end
        offered = rewindmod.offered_window(resp, end)
        if offered is None:
            return True
        crc = 0
        for crc in rewindmod.crc_slices(self._wal_range, offered[0], end):
            await asyncio.sleep(0)
        return crc == offered[1]

    async def _follow_upstream_once(self, gen: int) -> None:
        if not self.upstream:
            return
        host, _, port = self.upstream.partition(":")
        reader, writer = await asyncio.wait_for(
            dial.open_connection(host, int(port)), 5.0)
        if self._repl_gen != gen:
            # superseded while connecting: never register or stream
            self._abort(writer)
            return
        self._repl_writer = writer
        try:
            req = {"q": "repl",
                   "name": self.settings.name,
                   "ident": self.ident.get("ident"),
                   "timeline": self.timeline,
                   "start_lsn": self.wal.end,
                   "history": self.history,
                   "wal_start": self.wal.start}
            writer.write((json.dumps(req) + "\n").encode())
            await writer.drain()
            line = await asyncio.wait_for(reader.readline(), 5.0)
            resp = json.loads(line)
            if not resp.get("ok"):
                err = resp.get("error", "repl refused")
                if err in ("diverged", "timeline-mismatch",
                           "ident-mismatch", "wal-gone"):
                    self.upstream_status = "diverged"
                    self.log.error("cannot stream from upstream; "
                                   "restore required", error=err)
                raise RuntimeError("upstream refused replication: " + err)
            # the histories did not rule us out; the bytes decide.  Before
            # anything is adopted, appended or acked: a follower found
            # diverged here has changed no file and opened no write gate
            if not await self._verify_handshake(resp):
                self.upstream_status = "diverged"
                self.log.error("cannot stream from upstream; restore "
                               "required", error="diverged",
                               detail="WAL below our end differs from "
                                      "the upstream's")
                raise RuntimeError("WAL is not a prefix of the upstream's")
            # adopt upstream's timeline/history (we are a consistent prefix)
            if resp.get("timeline", self.timeline) != self.timeline or \
                    resp.get("history") != self.history:
                self.ident["timeline"] = resp.get("timeline", self.timeline)
                self.ident["history"] = resp.get("history", self.history)
                self.save_ident()
            self.upstream_status = "streaming"
            self.log.info("streaming from upstream", upstream=self.upstream,
                          start=lsnmod.format_lsn(self.wal.end))
            # initial ack so an already-caught-up follower reports its
            # position immediately (the primary's write-enable gate needs it)
            writer.write(self._ack_payload())
            await writer.drain()
            while True:
                if self._repl_gen != gen:
                    # superseded (promote/reconfigure whose cancel we
                    # never saw — bpo-42130): one more ack from here
                    # would reopen the deposed primary's commit gate
                    raise ConnectionError("superseded replication client")
                # the primary keepalives every 5 s; a silent link for 3×
                # that is a dead upstream (e.g. network partition with
                # the TCP connection still "open") — reconnect rather
                # than hang in a read forever
                hdr = await asyncio.wait_for(reader.readexactly(4), 15.0)
                (n,) = _U32.unpack(hdr)
                if n == 0:
                    writer.write(self._ack_payload())  # keepalive → re-ack
                    await writer.drain()
                    continue
                chunk = await reader.readexactly(n)
                # validate/split BEFORE touching the WAL: bytes that are
                # appended but fail to parse would never be applied to
                # the kv, leaving this standby acking data it does not
                # serve (and a later promote would lose it)
                frames = list(parse_frames(chunk))
                at = self.wal.end
                self.wal.append_raw(chunk, at)
                for frame_len, payload in frames:
                    at += frame_len
                    self._apply_replay(at, payload)
                self._wake_replicas()  # cascade downstream
                writer.write(self._ack_payload())
                await writer.drain()
        except asyncio.CancelledError:
            # the follower is being STOPPED (promote, reconfigure,
            # shutdown): sever abruptly.  A graceful close would flush a
            # buffered ack, which could let the old upstream acknowledge
            # one more client write while THIS node is already taking
            # over — shrink that window to nothing.
            self._abort(writer)
            raise
        finally:
            self.upstream_status = "disconnected" \
                if self.upstream_status == "streaming" else self.upstream_status
            if self._repl_writer is writer:
                self._repl_writer = None
            writer.close()

    # ------------------------------------------------------------- commits
    async def _do_write(self, op: dict) -> dict:
        """Commit one WAL record (a put, a delete, or an atomic batch —
        one record ⇒ all-or-nothing across crash recovery AND
        replication) under the synchronous-commit gate."""
        lsn, err = self._append_write(op)
        if err is not None:
            return err
        return await self._await_commit(lsn)

    def _append_write(self, op: dict):
        """Validate + append + apply ONE record without waiting.
        Returns (lsn, None) or (None, error_response)."""
        settings = self.settings
        if settings.role != "primary":
            return None, {"ok": False, "error": "read-only: not the "
                                                "primary"}
        if settings.read_only:
            return None, {"ok": False, "error":
                          "cannot execute in a read-only transaction"}
        lsn = self.wal.append_buffered(encode_op(op))
        self._apply_op(op)
        self.replay_lsn = lsn
        self.last_replay_time = time.time()
        self._wake_replicas()
        return lsn, None

    async def _await_commit(self, lsn: int) -> dict:
        """synchronous_commit=remote_write: wait until the named sync
        standby reports the record written (ref etc/postgresql.conf,
        SURVEY.md §6)."""
        if self.settings.sync_standby:
            # fast path — the sync already acked this LSN (common under
            # group commit once an ack lands): no Condition round trip.
            # Safe without the lock: single-threaded event loop, no
            # await between the check and the return.
            rep = self._sync_replica()
            if (rep is None or rep.write_lsn < lsn
                    or self.settings.read_only) \
                    and not await self._wait_sync_written(lsn):
                return {"ok": False, "error":
                        "read-only set while awaiting sync standby"}
        return {"ok": True, "lsn": lsnmod.format_lsn(lsn)}

    async def _wait_sync_written(self, lsn: int) -> bool:
        """Sleep on commit_cond until the sync standby has written
        ``lsn`` or none is required any more (True), or read-only is set
        (False: nothing still waiting may be acknowledged)."""
        async with self.commit_cond:
            while True:
                if self.settings.read_only:
                    return False
                rep = self._sync_replica()
                if not self.settings.sync_standby or \
                        (rep is not None and rep.write_lsn >= lsn):
                    return True
                await self.commit_cond.wait()

    # ---------------------------------------------------------------- reads
    def get(self, k) -> Tuple[bool, object]:
        """(found, value)."""
        return k in self.kv, self.kv.get(k)

    def count(self, prefix: Optional[str] = None) -> int:
        if prefix:
            return sum(1 for k in self.kv if k.startswith(prefix))
        return len(self.kv)

    def scan(self, prefix: str, after: Optional[str],
             limit: int) -> List[str]:
        """Up to ``limit`` keys with ``prefix`` above ``after``, sorted."""
        keys = sorted(k for k in self.kv if k.startswith(prefix)
                      and (after is None or k > after))
        return keys[:limit]

    def replica_rows(self) -> Iterator[Tuple[ReplicaConn, dict]]:
        """One pg_stat_replication row per connected replica, LSNs
        formatted (ref lib/adm.js:348-427)."""
        sync = self.settings.sync_standby
        for rep in self.replicas:
            yield rep, {
                "application_name": rep.name,
                "state": "streaming",
                "sync_state": "sync" if rep.name == sync else "async",
                "sent_lsn": lsnmod.format_lsn(rep.sent_lsn),
                "write_lsn": lsnmod.format_lsn(rep.write_lsn),
                "flush_lsn": lsnmod.format_lsn(rep.flush_lsn),
                "replay_lsn": lsnmod.format_lsn(rep.replay_lsn),
            }

    def _status(self) -> dict:
        return {
            "ok": True,
            "pid": os.getpid(),
            "role": self.role,
            "timeline": self.timeline,
            "ident": self.ident.get("ident"),
            "current_lsn": lsnmod.format_lsn(self.wal.end),
            "replay_lsn": lsnmod.format_lsn(self.replay_lsn),
            "checkpoint_lsn": lsnmod.format_lsn(self.ckpt_lsn),
            "wal_start_lsn": lsnmod.format_lsn(self.wal.start),
            "wal_retained_bytes": self.wal.end - self.wal.start,
            "last_replay_time": self.last_replay_time,
            "read_only": self.read_only,
            "sync_standby": self.sync_standby,
            "upstream": self.upstream,
            "upstream_status": (self.upstream_status
                                if self.role == "standby" else "n/a"),
            "replication": [row for _, row in self.replica_rows()],
            "uptime_s": time.time() - self._start_time,
            "keys": len(self.kv),
        }


def _write_json_atomic(path: str, obj, **dump_kw) -> int:
    """tmp + fsync + rename + directory fsync: readers see the old file
    or the new one, and once this returns a power loss cannot bring the
    old one back (what is deleted next — WAL below a checkpoint, layers
    a manifest superseded, the promote trigger — relies on that).
    Returns the size written."""
    tmp = path + ".tmp"
    with open(tmp, "w") as f:
        json.dump(obj, f, **dump_kw)
        f.flush()
        os.fsync(f.fileno())
        size = os.fstat(f.fileno()).st_size
    os.replace(tmp, path)
    _fsync_dir(os.path.dirname(path))
    return size


def init_data_dir(data_dir: str) -> None:
    """initdb analogue: fresh system identifier, timeline 1."""
    os.makedirs(data_dir, exist_ok=True)
    ident = {"ident": uuid.uuid4().hex, "timeline": 1,
             "history": [{"tl": 1, "at": 0}]}
    with open(os.path.join(data_dir, IDENT_NAME), "w") as f:
        json.dump(ident, f)
    os.chmod(data_dir, 0o700)


def run_server(server: ReplCore) -> int:
    """Start, serve until SIGINT/SIGTERM/SIGQUIT, exit 0."""
    async def run():
        await server.start()
        stop = asyncio.Event()
        loop = asyncio.get_running_loop()
        for sig in (signal.SIGINT, signal.SIGTERM, signal.SIGQUIT):
            loop.add_signal_handler(sig, stop.set)
        await stop.wait()
        # MANATEE-188: a DIRTY exit, by design — durability comes from
        # the crash-safe WAL and checkpoints are atomic tmp+replace, so
        # a graceful unwind adds nothing.  And it WAITS for the default
        # executor, where a whole-kv checkpoint write can be in flight
        # for tens of seconds: that stalled failovers ~60 s
        # (docs/troubleshooting.md).  os._exit skips all that.
        if os.environ.get("WALDB_CLEAN_EXIT"):
            return 0            # profiling/debug: full unwind on signal
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)

    return asyncio.run(run())
