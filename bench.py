#!/usr/bin/env python3
"""bench.py — the north-star benchmark (BASELINE.json).

Metric: **failover-to-writable seconds** on a 3-peer shard under continuous
acknowledged write load, with **zero acknowledged-write loss**, measured
around ``kill -9`` of the primary.

One *step* = one full failover cycle:
  1. a background writer issues synchronously-replicated writes against the
     primary, recording every acknowledged key;
  2. ``kill -9`` the primary peer (sitter + database + backupserver);
  3. wait until a NEW primary acknowledges a write  → failover-to-writable;
  4. verify every previously-acknowledged write is present (write loss = 0);
  5. rebuild the deposed ex-primary (manatee-adm rebuild flow) so the shard
     is back to primary/sync/async for the next step.

``value`` is the p50 failover-to-writable over the timed steps
(lower is better).  ``vs_baseline`` divides by the reference's own
integration-suite convergence bound of 30 s on one host
(/root/reference/test/integ.test.js:53) — the only comparable number the
reference publishes.

Driver contract: ``python bench.py --gpus N --steps K --warmup W``; under
torchrun each rank runs an independent shard (weak scaling) and rank 0
reports the worst rank's p50.

A plain run sets up the shard, warms up, times the K steps and prints the
result line — nothing else.  ``--dump-outputs DIR`` additionally reads
back, after the timed steps, the PRELOAD keys from the final primary and
sync and saves them (plus the last step's lost-write count) as
``DIR/<name>.npy``; the keys and values written are the same in every
run, so two builds can be compared array for array.  ``--full`` is where
any measurement beyond the headline figure belongs (none exists yet).
"""

import argparse
import asyncio
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from manatee_amd.tools.devcluster import DevCluster  # noqa: E402

# bench timing tier: detection is bounded by the ZK session timeout.  The
# reference's own test tier uses 2000 ms sessions
# (/root/reference/test/zookeeperMgr.test.js:52-56); we use the same.
SESSION_TIMEOUT_MS = 2000

# writes acknowledged before the first kill of every run (keys
# bench-0 .. bench-(PRELOAD-1)); --dump-outputs reads exactly these back
PRELOAD = 50


class Writer:
    """Continuous acknowledged-write load against the current primary.

    Tracks every acknowledged write by COUNT (verified with a server-side
    count of the key prefix — any lost write changes it) plus a rolling
    window of recent (key, value) pairs verified individually; keys are
    unique so the count check is exact while verification stays O(window)
    instead of O(total writes) per failover step."""

    WINDOW = 4000

    def __init__(self, cluster: DevCluster):
        self.cluster = cluster
        self.acked = {}           # rolling window of recent acked writes
        self.acked_count = 0      # total acknowledged writes
        self.seq = 0
        self.task = None
        self.stop_flag = False
        self.pause_flag = False
        self._paused = asyncio.Event()
        self.last_ack_time = None

    async def _run(self):
        cli = None
        peer = None
        while not self.stop_flag:
            if self.pause_flag:
                # quiescent point: no put is in flight while paused, so
                # acked_count is exact and frozen for the loss check
                self._paused.set()
                await asyncio.sleep(0.01)
                continue
            try:
                if cli is None:
                    s = await self.cluster.cluster_state()
                    if s is None:
                        await asyncio.sleep(0.05)
                        continue
                    peer = self.cluster.peer_by_id(s["primary"]["id"])
                    cli = peer.db_client()
                key = "bench-%d" % self.seq
                await cli.put(key, self.seq, timeout_s=1.0)
                self.acked[key] = self.seq
                self.acked_count += 1
                if len(self.acked) > self.WINDOW:
                    self.acked.pop(next(iter(self.acked)))
                self.last_ack_time = time.monotonic()
                self.seq += 1
            except Exception:
                if cli is not None:
                    await cli.close()
                cli = None
                await asyncio.sleep(0.02)
        if cli is not None:
            await cli.close()

    def start(self):
        self.stop_flag = False
        self.task = asyncio.get_running_loop().create_task(self._run())

    async def pause(self):
        """Freeze the writer at an iteration boundary (no in-flight put).
        While paused no new acks can arrive, so a server-side count
        compared against ``acked_count`` is exact — post-failover acks
        cannot pad over a lost write."""
        self._paused.clear()
        self.pause_flag = True
        await self._paused.wait()

    def resume(self):
        self.pause_flag = False

    async def stop(self):
        self.stop_flag = True
        self.pause_flag = False
        if self.task is not None:
            await self.task
            self.task = None


# test seam: called with (cluster, state) after failover completes and
# BEFORE the loss verification — the injected-loss regression test uses it
# to delete an acknowledged key and prove the check catches it
_pre_verify_hook = None


async def verify_no_loss(cluster: DevCluster, state: dict,
                         writer: Writer) -> dict:
    """Exact zero-acknowledged-write-loss check.

    The writer is FROZEN first (no in-flight put, no new acks), so the
    acked set is exactly ``bench-0 .. bench-(seq-1)`` — the writer only
    advances ``seq`` after an ack and retries the same key otherwise.
    A server-side count of the prefix therefore detects ANY lost key;
    the rolling window (the writes nearest the kill) is additionally
    read back value-by-value.  The new SYNC must converge to hold every
    acked write as well (it replicates from the new primary)."""
    await writer.pause()
    try:
        acked_total = writer.acked_count
        window = dict(writer.acked)
        assert acked_total == writer.seq, \
            "writer invariant broken: acked_count != seq while paused"

        # at most ONE committed-but-unacked key can exist (the writer has a
        # single in-flight put and retries the same seq until acked): it is
        # exactly bench-<seq>.  Probe it and exclude it from the count so it
        # cannot pad over a lost acked key.
        probe_key = "bench-%d" % acked_total

        newp = cluster.peer_by_id(state["primary"]["id"])
        cli = newp.db_client()
        lost = 0
        try:
            present = await cli.count(prefix="bench-")
            if await cli.get(probe_key) is not None:
                present -= 1
            if present < acked_total:
                lost += acked_total - present
            for key, val in window.items():
                got = await cli.get(key)
                if got != val:
                    lost += 1
        finally:
            await cli.close()

        # the sync must CONVERGE to contain every acked write (it may be
        # the old async, still replaying) — poll with a deadline
        sync_lost = 0
        if state.get("sync"):
            syncp = cluster.peer_by_id(state["sync"]["id"])
            scli = syncp.db_client()
            try:
                deadline = time.monotonic() + 15.0
                sync_present = 0
                while time.monotonic() < deadline:
                    try:
                        sync_present = await scli.count(prefix="bench-")
                        if await scli.get(probe_key) is not None:
                            sync_present -= 1
                    except Exception:
                        sync_present = 0
                    if sync_present >= acked_total:
                        break
                    await asyncio.sleep(0.05)
                if sync_present < acked_total:
                    sync_lost = acked_total - sync_present
            finally:
                await scli.close()
        return {"lost": lost + sync_lost, "checked": acked_total}
    finally:
        writer.resume()


async def one_failover(cluster: DevCluster, writer: Writer) -> dict:
    """Kill the primary; measure kill→writable; verify zero write loss."""
    s = await cluster.cluster_state()
    prim = cluster.peer_by_id(s["primary"]["id"])
    old_gen = s["generation"]

    t_kill = time.monotonic()
    prim.kill9()
    # writable == a brand-new write acknowledged by the NEW primary
    deadline = t_kill + 120
    t_writable = None
    while time.monotonic() < deadline:
        s2 = await cluster.cluster_state()
        if s2 and s2["generation"] > old_gen and \
                s2["primary"]["id"] != prim.id:
            newp = cluster.peer_by_id(s2["primary"]["id"])
            cli = newp.db_client()
            try:
                await cli.put("__failover_probe__", time.time(),
                              timeout_s=1.0)
                t_writable = time.monotonic()
                await cli.close()
                break
            except Exception:
                await cli.close()
        await asyncio.sleep(0.02)
    if t_writable is None:
        raise RuntimeError("failover did not complete within 120 s")

    s2 = await cluster.cluster_state()
    if _pre_verify_hook is not None:
        await _pre_verify_hook(cluster, s2)
    v = await verify_no_loss(cluster, s2, writer)

    # heal: rebuild the deposed ex-primary so the next step starts from a
    # full primary/sync/async shard
    await cluster.rebuild_peer(prim)
    await cluster.wait_writable(timeout_s=60)
    return {"failover_s": t_writable - t_kill,
            "lost_acked_writes": v["lost"], "acked_checked": v["checked"]}


async def read_back_preload(cluster: DevCluster) -> dict:
    """What a caller is left with after the last timed step: the current
    primary's (and sync's) values for the PRELOAD keys.  These keys are
    acknowledged before the first kill in every run, so the arrays have
    the same shape and — absent write loss — the same content from run
    to run; a missing key reads back as NaN."""
    s = await cluster.cluster_state()
    out = {}
    for role in ("primary", "sync"):
        vals = []
        if s.get(role):
            cli = cluster.peer_by_id(s[role]["id"]).db_client()
            try:
                for i in range(PRELOAD):
                    v = await cli.get("bench-%d" % i)
                    vals.append(float("nan") if v is None else float(v))
            finally:
                await cli.close()
        out["readback_%s" % role] = vals
    return out


def dump_outputs(dump_dir: str, arrays: dict) -> None:
    """Write each array as ``<dump_dir>/<name>.npy`` (float64)."""
    import numpy as np
    os.makedirs(dump_dir, exist_ok=True)
    for name, vals in arrays.items():
        np.save(os.path.join(dump_dir, name + ".npy"),
                np.asarray(vals, dtype=np.float64))


async def run_rank(rank: int, steps: int, warmup: int, base_dir: str,
                   engine: str = "waldb",
                   session_timeout_ms: int = SESSION_TIMEOUT_MS,
                   want_outputs: bool = False) -> dict:
    cluster = DevCluster(os.path.join(base_dir, "rank%d" % rank),
                         n_peers=3, shard_name="%d.bench" % (rank + 1),
                         engine=engine,
                         session_timeout_ms=session_timeout_ms)
    # SIGTERM (e.g. `timeout`-bounded runs) must unwind through the
    # finally below — a hard exit would orphan the whole cluster, and a
    # leaked db squatting a port poisons later runs on the same host
    loop = asyncio.get_running_loop()
    me = asyncio.current_task()
    import signal as _signal
    for _sig in (_signal.SIGTERM, _signal.SIGINT):
        try:
            loop.add_signal_handler(_sig, me.cancel)
        except (NotImplementedError, RuntimeError):
            pass
    results = []
    total_lost = 0
    total_checked = 0
    try:
        await cluster.start()
        await cluster.wait_cluster(
            lambda s: s.get("sync") and len(s.get("async", [])) == 1,
            timeout_s=120, what="formation")
        await cluster.wait_writable(timeout_s=120)
        writer = Writer(cluster)
        writer.start()
        # let some write load accumulate
        while writer.seq < PRELOAD:
            await asyncio.sleep(0.05)

        for i in range(warmup):
            r = await one_failover(cluster, writer)
            print("# rank %d warmup %d: %.3fs (lost=%d)"
                  % (rank, i, r["failover_s"], r["lost_acked_writes"]),
                  file=sys.stderr)
        t0 = time.monotonic()
        for i in range(steps):
            r = await one_failover(cluster, writer)
            results.append(r)
            total_lost += r["lost_acked_writes"]
            total_checked += r["acked_checked"]
            print("# rank %d step %d: failover %.3fs (lost=%d/%d)"
                  % (rank, i, r["failover_s"], r["lost_acked_writes"],
                     r["acked_checked"]), file=sys.stderr)
        elapsed = time.monotonic() - t0
        await writer.stop()
        outputs = None
        if want_outputs:
            outputs = await read_back_preload(cluster)
            outputs["lost_acked_writes"] = \
                [results[-1]["lost_acked_writes"]]
    finally:
        cluster.stop()

    times = sorted(r["failover_s"] for r in results)
    return {
        "p50": statistics.median(times),
        "p99": times[min(len(times) - 1, int(len(times) * 0.99))],
        "mean": statistics.fmean(times),
        "max": times[-1],
        "min": times[0],
        "lost": total_lost,
        "checked": total_checked,
        "writes_acked": sum(r["acked_checked"] for r in results[-1:]),
        "elapsed_s": elapsed,
        "outputs": outputs,
    }


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--engine", choices=("waldb", "postgres"),
                    default="waldb",
                    help="postgres = the engine=postgres management path "
                         "(minipg binaries, libpq writes)")
    ap.add_argument("--session-timeout-ms", type=int,
                    default=SESSION_TIMEOUT_MS,
                    help="ZK session timeout (failure-detection bound); "
                         "2000 matches the reference's test tier, 60000 "
                         "its production tier")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last step "
                         "left behind as DIR/<name>.npy (float64): the "
                         "PRELOAD keys read back from the primary and the "
                         "sync, and the last step's lost-write count")
    ap.add_argument("--full", action="store_true",
                    help="also run measurements beyond the headline "
                         "figure (none at present: a plain run already "
                         "does only setup, warmup and the timed steps)")
    ns = ap.parse_args()
    if ns.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))

    base_dir = ns.workdir or tempfile.mkdtemp(prefix="manatee-bench-")
    try:
        res = asyncio.run(run_rank(
            rank, ns.steps, ns.warmup, base_dir, engine=ns.engine,
            session_timeout_ms=ns.session_timeout_ms,
            want_outputs=ns.dump_outputs is not None))
    finally:
        if ns.workdir is None:   # keep logs when an explicit workdir is given
            shutil.rmtree(base_dir, ignore_errors=True)

    if ns.dump_outputs is not None:
        # one shard per rank: rank 0 owns the plain names
        dump_outputs(ns.dump_outputs if rank == 0 else
                     os.path.join(ns.dump_outputs, "rank%d" % rank),
                     res.pop("outputs"))

    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo")
        gathered = [None] * world
        dist.all_gather_object(gathered, res)
        dist.barrier()
        if rank != 0:
            return 0
        # whole-job view: worst rank's p50 (time metric, weak scaling)
        res = {
            "p50": max(r["p50"] for r in gathered),
            "p99": max(r["p99"] for r in gathered),
            "mean": statistics.fmean(r["mean"] for r in gathered),
            "max": max(r["max"] for r in gathered),
            "min": min(r["min"] for r in gathered),
            "lost": sum(r["lost"] for r in gathered),
            "checked": sum(r["checked"] for r in gathered),
            "elapsed_s": max(r["elapsed_s"] for r in gathered),
        }

    baseline_s = 30.0   # reference integ-suite convergence bound
    out = {
        "metric": "failover-to-writable seconds (p50/p99) + ack'd-write "
                  "loss, 3-node shard",
        "value": round(res["p50"], 4),
        "unit": "s",
        "n_gpus": ns.gpus,
        "steps": ns.steps,
        "warmup": ns.warmup,
        "ms_per_step": round(res["elapsed_s"] / ns.steps * 1000.0, 1),
        "higher_is_better": False,
        "scaling": "weak",
        "vs_baseline": round(res["p50"] / baseline_s, 4),
        "dtype": "n/a",
        "data": "synthetic",
        "config": {
            "model": "manatee shard (primary/sync/async)",
            "engine": ns.engine,
            "peers_per_shard": 3,
            "shards": world,
            "parallelism": "one shard per rank",
            "workload": "continuous synchronously-replicated writes",
            "session_timeout_ms": ns.session_timeout_ms,
            "kill_mode": "SIGKILL of primary sitter+db+backupserver",
            "p99_s": round(res["p99"], 4),
            "mean_s": round(res["mean"], 4),
            "min_s": round(res["min"], 4),
            "max_s": round(res["max"], 4),
            "acked_writes_checked": res["checked"],
            "acked_writes_lost": res["lost"],
            "baseline_note": "reference's own integ bound: topology "
                             "convergence <= 30 s after SIGKILL "
                             "(test/integ.test.js:53)",
        },
    }
    if res["lost"] != 0:
        out["config"]["INVALID"] = "acknowledged writes were lost"
    print(json.dumps(out))
    return 0 if res["lost"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
