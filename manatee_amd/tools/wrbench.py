"""Write/read throughput micro-benchmark for the replicated engine.

    python -m manatee_amd.tools.wrbench [--seconds 10] [--writers 1,8,32]
        [--engine waldb|postgres] [--profile kv|tpcb]

Spins a local 3-peer shard (primary -> sync -> async) and measures,
for each writer count, the rate of *synchronously acknowledged* puts
(every put waits for the sync standby's write-ack, the shard's
durability contract) plus standby read throughput.  One JSON line on
stdout.

``--profile tpcb`` (engine=postgres only) runs a pgbench-style
transactional load instead: every writer moves amounts between its own
accounts in BEGIN..COMMIT blocks over prepared statements, the run
reports transactions per second, and afterwards the balance, history
and sequence invariants are verified on the primary and on the sync
standby (``check_tpcb``)."""

from __future__ import annotations

import argparse
import asyncio
import json
import shutil
import sys
import tempfile
import time

from ..db.pgwire import PgClient
from .devcluster import DevCluster


async def writer_task(peer, label, stop, counter, pipeline=0):
    cli = peer.db_client()
    i = 0
    try:
        while not stop.is_set():
            if pipeline > 1:
                n = await cli.put_many(
                    (("w-%s-%d" % (label, i + j), i + j)
                     for j in range(pipeline)))
                counter[0] += n
                i += pipeline
            else:
                await cli.put("w-%s-%d" % (label, i), i)
                counter[0] += 1
                i += 1
    finally:
        await cli.close()


async def reader_task(peer, stop, counter):
    cli = peer.db_client()
    i = 0
    try:
        while not stop.is_set():
            await cli.get("w-0-%d" % (i % 1000))
            counter[0] += 1
            i += 1
    finally:
        await cli.close()


async def measure(c: DevCluster, n_writers: int, seconds: float,
                  pipeline: int = 0) -> dict:
    s = await c.cluster_state()
    prim = c.peer_by_id(s["primary"]["id"])
    sync = c.peer_by_id(s["sync"]["id"])
    stop = asyncio.Event()
    wcount = [0]
    rcount = [0]
    tasks = [asyncio.ensure_future(
        writer_task(prim, "%d.%d" % (pipeline, w),
                    stop, wcount, pipeline=pipeline))
        for w in range(n_writers)]
    tasks += [asyncio.ensure_future(
        reader_task(sync, stop, rcount))
        for _ in range(4)]
    t0 = time.monotonic()
    await asyncio.sleep(seconds)
    stop.set()
    await asyncio.gather(*tasks, return_exceptions=True)
    dt = time.monotonic() - t0
    return {"writers": n_writers, "pipeline": pipeline,
            "acked_puts_per_s": round(wcount[0] / dt, 1),
            "standby_reads_per_s": round(rcount[0] / dt, 1)}


# ------------------------------------------------------- the tpcb profile

TPCB_ACCOUNTS = 4
TPCB_BALANCE = 1000
_TPCB_STMTS = {
    "tpcb_begin": "BEGIN",
    "tpcb_sel": "SELECT v FROM kv WHERE k = $1",
    "tpcb_upd": "UPDATE kv SET v = $1 WHERE k = $2",
    "tpcb_ins": "INSERT INTO kv (k, v) VALUES ($1, $2)",
    "tpcb_commit": "COMMIT",
}


class InvariantError(AssertionError):
    pass


class TpcbWriter:
    """One pgbench-style (TPC-B-like) writer over prepared statements.

    It owns the accounts ``acct-<label>-<i>`` — there are no row locks,
    so writers never share a key.  Transaction ``k`` moves an amount
    between two of them, stamps ``k`` into both values and inserts
    ``hist-<label>-<k>``, all in one BEGIN..COMMIT block; ``acked`` is
    the last ``k`` whose COMMIT was acknowledged."""

    def __init__(self, peer, label, n_accounts: int = TPCB_ACCOUNTS):
        if n_accounts < 2:
            raise ValueError("a tpcb writer needs at least two accounts")
        self.cli = PgClient(peer.ip, peer.pg_port, "postgres",
                            connect_timeout_s=5.0)
        self.label = str(label)
        self.n_accounts = n_accounts
        self.acked = -1

    def account(self, i: int) -> str:
        return "acct-%s-%d" % (self.label, i)

    async def setup(self) -> None:
        await self.cli.connect()
        for name, sql in _TPCB_STMTS.items():
            await self.cli.prepare(name, sql)
        start = json.dumps({"bal": TPCB_BALANCE, "k": -1})
        res = await self.cli.pipeline(
            [("tpcb_begin", ())]
            + [("tpcb_ins", (self.account(i), start))
               for i in range(self.n_accounts)]
            + [("tpcb_commit", ())])
        if res[-1].command != "COMMIT":
            raise RuntimeError("account setup ended with %r"
                               % res[-1].command)

    async def transact(self, timeout_s: float = 30.0) -> int:
        """Run the next transaction; returns its ``k`` once COMMIT is
        acknowledged."""
        k = self.acked + 1
        a, b = k % self.n_accounts, (k + 1) % self.n_accounts
        amount = 1 + k % 7
        ka, kb = self.account(a), self.account(b)
        res = await self.cli.pipeline(
            [("tpcb_begin", ()), ("tpcb_sel", (ka,)), ("tpcb_sel", (kb,))],
            timeout_s=timeout_s)
        va = json.loads(res[1].rows[0][0])
        vb = json.loads(res[2].rows[0][0])
        va = {"bal": va["bal"] - amount, "k": k}
        vb = {"bal": vb["bal"] + amount, "k": k}
        res = await self.cli.pipeline(
            [("tpcb_upd", (json.dumps(va), ka)),
             ("tpcb_upd", (json.dumps(vb), kb)),
             ("tpcb_ins", ("hist-%s-%d" % (self.label, k),
                           json.dumps({"from": a, "to": b, "amt": amount}))),
             ("tpcb_commit", ())], timeout_s=timeout_s)
        tags = [r.command for r in res]
        if tags != ["UPDATE 1", "UPDATE 1", "INSERT 0 1", "COMMIT"]:
            raise RuntimeError("tpcb transaction %d answered %r"
                               % (k, tags))
        self.acked = k
        return k

    async def run(self, stop: asyncio.Event) -> None:
        while not stop.is_set():
            await self.transact()

    async def close(self) -> None:
        await self.cli.close()


async def check_tpcb(kv, label, n_accounts: int, acked: int) -> int:
    """Verify one writer's invariants through the key/value client
    ``kv`` of any peer; returns ``m``, the last transaction present.

    (a) the balances sum to the starting total; (b) the
    ``hist-<label>-*`` rows are exactly ``0..m`` with ``m >= acked``
    (one more than ``acked`` is legal: a COMMIT that was applied but
    whose acknowledgement never reached the writer); (c) the largest
    sequence number stamped into any account is ``m``."""
    n_hist = await kv.count(prefix="hist-%s-" % label)
    m = n_hist - 1
    if m < acked:
        raise InvariantError(
            "writer %s: %d history rows, but transaction %d was "
            "acknowledged" % (label, n_hist, acked))
    for lo in range(0, n_hist, 500):
        keys = ["hist-%s-%d" % (label, k)
                for k in range(lo, min(lo + 500, n_hist))]
        for key, v in zip(keys, await kv.get_many(keys)):
            if v is None:
                raise InvariantError(
                    "writer %s: %d history rows but %s is missing"
                    % (label, n_hist, key))
    accts = await kv.get_many(["acct-%s-%d" % (label, i)
                               for i in range(n_accounts)])
    if any(v is None for v in accts):
        raise InvariantError("writer %s: an account is missing" % label)
    total = sum(v["bal"] for v in accts)
    if total != n_accounts * TPCB_BALANCE:
        raise InvariantError(
            "writer %s: balances sum to %d, started with %d"
            % (label, total, n_accounts * TPCB_BALANCE))
    stamped = max(v["k"] for v in accts)
    if stamped != m:
        raise InvariantError(
            "writer %s: accounts are stamped up to %d but history ends "
            "at %d" % (label, stamped, m))
    return m


async def check_tpcb_on(peer, writers, wait_s: float = 10.0) -> int:
    """``check_tpcb`` for every writer on ``peer``; returns the number
    of history rows.  A standby is given ``wait_s`` to replay what the
    writers had acknowledged."""
    kv = peer.db_client()
    try:
        deadline = time.monotonic() + wait_s
        rows = 0
        for w in writers:
            while await kv.count(prefix="hist-%s-" % w.label) <= w.acked \
                    and time.monotonic() < deadline:
                await asyncio.sleep(0.05)
            rows += 1 + await check_tpcb(kv, w.label, w.n_accounts,
                                         w.acked)
        return rows
    finally:
        await kv.close()


async def measure_tpcb(c: DevCluster, n_writers: int, seconds: float,
                       accounts: int = TPCB_ACCOUNTS) -> dict:
    s = await c.cluster_state()
    prim = c.peer_by_id(s["primary"]["id"])
    sync = c.peer_by_id(s["sync"]["id"])
    writers = [TpcbWriter(prim, "%d.%d" % (n_writers, w), accounts)
               for w in range(n_writers)]
    try:
        for w in writers:
            await w.setup()
        stop = asyncio.Event()
        tasks = [asyncio.ensure_future(w.run(stop)) for w in writers]
        t0 = time.monotonic()
        await asyncio.sleep(seconds)
        stop.set()
        done = await asyncio.gather(*tasks, return_exceptions=True)
        dt = time.monotonic() - t0
    finally:
        for w in writers:
            await w.close()
    for exc in done:
        if isinstance(exc, BaseException):
            raise exc
    rows = await check_tpcb_on(prim, writers)
    rows_sync = await check_tpcb_on(sync, writers)
    if rows_sync != rows:
        raise InvariantError("sync standby holds %d history rows, the "
                             "primary %d" % (rows_sync, rows))
    return {"writers": n_writers, "profile": "tpcb",
            "txns_per_s": round(sum(w.acked + 1 for w in writers) / dt, 1),
            "accounts": n_writers * accounts, "history_rows": rows,
            "invariants_ok": True}


async def run(writers, seconds, workdir, engine="waldb", profile="kv",
              accounts=TPCB_ACCOUNTS) -> dict:
    if profile not in ("kv", "tpcb"):
        raise ValueError("unknown profile %r" % profile)
    if profile == "tpcb" and engine != "postgres":
        raise ValueError("the tpcb profile needs engine=postgres")
    c = DevCluster(workdir, n_peers=3, shard_name="1.wrbench",
                   engine=engine)
    try:
        await c.start()
        await c.wait_cluster(
            lambda s: s.get("sync") and len(s.get("async", [])) == 1,
            timeout_s=120, what="formation")
        await c.wait_writable(timeout_s=120)
        results = []
        if profile == "tpcb":
            for w in writers:
                r = await measure_tpcb(c, w, seconds, accounts)
                results.append(r)
                print("# writers=%d: %.0f txns/s" % (w, r["txns_per_s"]),
                      file=sys.stderr)
            s = await c.cluster_state()
            cli = c.peer_by_id(s["primary"]["id"]).db_client()
            total = await cli.count(prefix="acct-") + \
                await cli.count(prefix="hist-")
            await cli.close()
            return {"engine": engine, "profile": profile,
                    "results": results, "total_keys": total}
        for w in writers:
            r = await measure(c, w, seconds)
            results.append(r)
            print("# writers=%d: %.0f acked puts/s, %.0f standby reads/s"
                  % (w, r["acked_puts_per_s"], r["standby_reads_per_s"]),
                  file=sys.stderr)
        # pipelined bulk mode: batches of 50 per round trip
        r = await measure(c, 4, seconds, pipeline=50)
        results.append(r)
        print("# writers=4 pipeline=50: %.0f acked puts/s"
              % r["acked_puts_per_s"], file=sys.stderr)
        # durability sanity: everything acked must be present
        s = await c.cluster_state()
        cli = c.peer_by_id(s["primary"]["id"]).db_client()
        total = await cli.count(prefix="w-")
        await cli.close()
        return {"engine": engine, "results": results, "total_keys": total}
    finally:
        c.stop()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="manatee-wrbench")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--engine", choices=("waldb", "postgres"),
                    default="waldb")
    ap.add_argument("--writers", default="1,8,32")
    ap.add_argument("--profile", choices=("kv", "tpcb"), default="kv",
                    help="kv: single acked puts (default); tpcb: "
                    "BEGIN/SELECT/UPDATE/INSERT/COMMIT transactions over "
                    "prepared statements (needs --engine postgres)")
    ap.add_argument("--accounts", type=int, default=TPCB_ACCOUNTS,
                    help="tpcb: accounts per writer")
    ap.add_argument("-d", "--dir", default=None)
    ns = ap.parse_args(argv)
    if ns.profile == "tpcb" and ns.engine != "postgres":
        ap.error("--profile tpcb requires --engine postgres")
    writers = [int(w) for w in ns.writers.split(",")]
    workdir = ns.dir or tempfile.mkdtemp(prefix="manatee-wrbench-")
    try:
        out = asyncio.run(run(writers, ns.seconds, workdir,
                              engine=ns.engine, profile=ns.profile,
                              accounts=ns.accounts))
    finally:
        if ns.dir is None:
            shutil.rmtree(workdir, ignore_errors=True)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
