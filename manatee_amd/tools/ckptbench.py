"""ckptbench — what a checkpoint costs in each ``checkpoint_mode``.

For every dataset size N and each mode, in a fresh data dir and an
in-process ``WaldbServer`` (no cluster, no sync standby):

1. load N keys of ``--value-bytes`` and take the first checkpoint (a
   whole image in ``full`` mode, the one-off base in ``incremental``);
2. overwrite a hot set of ``--hot-keys`` for ``--seconds`` while the
   server's own flush loop decides when a checkpoint is due, and a 1 ms
   ticker task records how long the event loop went without running it;
3. abandon the server without a clean stop and time a restart until it
   listens.

Per mode it reports the bytes each checkpoint wrote, the longest
event-loop stall, the data-dir size at the end and the restart time.
One JSON document on stdout; ``full`` is the yardstick for
``incremental`` on the same tree.

    python -m manatee_amd.tools.ckptbench --keys 100000,1000000
"""

from __future__ import annotations

import argparse
import asyncio
import json
import os
import shutil
import sys
import tempfile
import time

from ..common import confparser
from ..common.logging import null_logger
from ..db.waldb.server import WaldbServer, init_data_dir

TICK_S = 0.001


def _dir_bytes(path: str) -> int:
    total = 0
    for root, _dirs, files in os.walk(path):
        for name in files:
            try:
                total += os.path.getsize(os.path.join(root, name))
            except OSError:
                pass
    return total


class _Ticker:
    """A task that sleeps ``TICK_S`` in a loop; ``worst`` is the longest
    it was kept from running past that, i.e. the longest stall of the
    event loop since ``reset()``."""

    def __init__(self):
        self.worst = 0.0
        self._task = asyncio.get_running_loop().create_task(self._run())

    async def _run(self) -> None:
        while True:
            t0 = time.perf_counter()
            await asyncio.sleep(TICK_S)
            late = time.perf_counter() - t0 - TICK_S
            if late > self.worst:
                self.worst = late

    def reset(self) -> None:
        self.worst = 0.0

    def stop(self) -> None:
        self._task.cancel()


def _abandon(srv) -> None:
    if srv._server is not None:
        srv._server.close()
    if srv._flusher is not None:
        srv._flusher.cancel()
    srv.wal.close()


def _record_checkpoints(srv, out: list, merged: list) -> None:
    """Wrap ``srv._checkpoint`` so every checkpoint, the flush loop's
    included, leaves (bytes written, seconds, compactions so far), and
    ``srv._compact`` so every compaction leaves the new base's bytes."""
    inner = srv._checkpoint
    inner_compact = srv._compact

    async def compact():
        await inner_compact()
        merged.append(srv._layers[0]["bytes"])
    srv._compact = compact

    async def recorded():
        before = srv._ckpt_count
        t0 = time.perf_counter()
        await inner()
        if srv._ckpt_count > before:
            out.append({"bytes": srv._last_ckpt_bytes,
                        "records": srv._last_ckpt_records,
                        "seconds": round(time.perf_counter() - t0, 4),
                        "compactions": srv._compact_count})
    srv._checkpoint = recorded


async def run_mode(mode: str, keys: int, value_bytes: int, hot_keys: int,
                   seconds: float, ckpt_wal_bytes: int, workdir: str) -> dict:
    data = os.path.join(workdir, "%s-%d" % (mode, keys))
    init_data_dir(data)
    confparser.write(os.path.join(data, "waldb.conf"), {
        "role": "primary", "listen_ip": "127.0.0.1", "port": "0",
        "name": "bench", "checkpoint_mode": mode,
        "checkpoint_wal_bytes": str(ckpt_wal_bytes),
        # keep no more WAL than the checkpoints need, in small segments:
        # the data-dir size then shows what each mode has to retain
        "wal_keep_bytes": str(ckpt_wal_bytes),
        "wal_segment_bytes": str(max(65536, ckpt_wal_bytes // 4))})
    srv = WaldbServer(data, null_logger())
    await srv.start()
    ticker = _Ticker()
    ckpts: list = []
    merged: list = []
    try:
        # load with the flush loop's checkpoints held off, so both modes
        # start the measured phase from one first checkpoint
        srv._ckpt_running = True
        value = "v" * value_bytes
        for i in range(keys):
            srv._append_write({"op": "put", "k": "key%08d" % i, "v": value})
            if i % 2000 == 1999:
                await asyncio.sleep(0)
        srv.wal.fsync()
        _record_checkpoints(srv, ckpts, merged)
        ticker.reset()
        await srv._checkpoint()
        first = dict(ckpts.pop(), stall_ms=round(ticker.worst * 1e3, 2))
        del merged[:]

        ticker.reset()
        writes = 0
        hot_from = srv.wal.end
        deadline = time.perf_counter() + seconds
        while time.perf_counter() < deadline:
            for _ in range(50):
                srv._append_write({"op": "put",
                                   "k": "key%08d" % (writes % hot_keys),
                                   "v": value})
                writes += 1
            await asyncio.sleep(0)
        while srv._ckpt_running:
            await asyncio.sleep(0.01)
        forced = not ckpts
        if forced:
            # not one was due within the time: measure one all the same
            await srv._checkpoint()
        stall = ticker.worst
        size = _dir_bytes(data)
        wal_bytes = srv.wal.end - srv.wal.start
        hot_wal = srv.wal.end - hot_from
        want = (len(srv.kv), srv.replay_lsn)
    finally:
        ticker.stop()
        _abandon(srv)

    t0 = time.perf_counter()
    srv = WaldbServer(data, null_logger())
    await srv.start()
    restart = time.perf_counter() - t0
    try:
        if (len(srv.kv), srv.replay_lsn) != want:
            raise RuntimeError("%s mode: restart recovered %r, wanted %r"
                               % (mode, (len(srv.kv), srv.replay_lsn), want))
    finally:
        _abandon(srv)
    sizes = [c["bytes"] for c in ckpts]
    return {
        "first_checkpoint": first,
        "hot_writes": writes,
        "checkpoints": len(ckpts),
        "checkpoint_forced": forced,
        "compactions": len(merged),
        "compaction_bytes_total": sum(merged),
        "layer_bytes_per_wal_byte": round(
            (sum(sizes) + sum(merged)) / max(1, hot_wal), 3),
        "bytes_per_checkpoint_mean": sum(sizes) // len(sizes),
        "bytes_per_checkpoint_max": max(sizes),
        "checkpoint_seconds_max": max(c["seconds"] for c in ckpts),
        "max_loop_stall_ms": round(stall * 1e3, 2),
        "retained_wal_bytes": wal_bytes,
        "data_dir_bytes": size,
        "restart_to_listening_s": round(restart, 3),
    }


async def run(keys_list, value_bytes: int, hot_keys: int, seconds: float,
              ckpt_wal_bytes: int, workdir: str) -> dict:
    results = []
    for keys in keys_list:
        row = {"keys": keys, "modes": {}}
        for mode in ("full", "incremental"):
            row["modes"][mode] = await run_mode(
                mode, keys, value_bytes, hot_keys, seconds, ckpt_wal_bytes,
                workdir)
            shutil.rmtree(os.path.join(workdir, "%s-%d" % (mode, keys)),
                          ignore_errors=True)
        results.append(row)
    return {"bench": "ckptbench", "value_bytes": value_bytes,
            "hot_keys": hot_keys, "seconds": seconds,
            "checkpoint_wal_bytes": ckpt_wal_bytes, "results": results}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="manatee-ckptbench",
                                 description=__doc__.split("\n\n")[0])
    ap.add_argument("--keys", default="100000",
                    help="dataset sizes, comma-separated")
    ap.add_argument("--value-bytes", type=int, default=100)
    ap.add_argument("--hot-keys", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=5.0,
                    help="hot-set overwrite time per mode and size")
    ap.add_argument("--checkpoint-wal-bytes", type=int, default=1 << 20)
    ap.add_argument("-d", "--dir", default=None)
    ns = ap.parse_args(argv)
    keys_list = [int(k) for k in ns.keys.split(",") if k]
    workdir = ns.dir or tempfile.mkdtemp(prefix="manatee-ckptbench-")
    try:
        out = asyncio.run(run(keys_list, ns.value_bytes, ns.hot_keys,
                              ns.seconds, ns.checkpoint_wal_bytes, workdir))
    finally:
        if ns.dir is None:
            shutil.rmtree(workdir, ignore_errors=True)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
