"""Seeded discrete-event simulator for the consensus core (quorum.py).

In the manner of ``fsm/sim.py``: N ``QuorumCore``s, one event heap, one
seeded RNG — a failing seed replays exactly.  The network drops, delays
(and thereby reorders) and partitions messages; members crash and
restart from what they had PERSISTED (epoch, vote, log, snapshot) and
nothing else; a client proposes writes at whichever member will take
them and records the acknowledged ones.

Checked after every event:

- at most one leader per epoch;
- log matching: two logs that agree on the epoch at an index agree on
  everything before it;
- no two members ever apply different entries at one index (and an
  installed snapshot matches the history it claims to summarise);
- every acknowledged write is in the log of every later leader;
- a member never votes for two candidates in one epoch, restarts
  included.

    python -m manatee_amd.coord.quorumsim --seed 7 [--seconds 12] [-v]
"""

from __future__ import annotations

import argparse
import hashlib
import heapq
import json
import random
import sys
from typing import Any, Dict, List, Optional, Set, Tuple

from .quorum import LEADER, QuorumCore


class InvariantViolation(AssertionError):
    pass


def _chain(prev: str, entry) -> str:
    return hashlib.sha1((prev + json.dumps(entry, sort_keys=True))
                        .encode()).hexdigest()[:16]


class _Store:
    """What one member has on disk."""

    def __init__(self):
        self.epoch = 0
        self.voted_for: Optional[int] = None
        self.base_index = 0
        self.base_epoch = 0
        self.log: List[tuple] = []
        self.snapshot: Any = None


class _Member:
    def __init__(self, node_id: int):
        self.id = node_id
        self.store = _Store()
        self.core: Optional[QuorumCore] = None
        self.applied = 0            # state machine position
        self.digest = ""            # hash chain over applied entries
        self.incarnation = 0


class QuorumSim:
    def __init__(self, seed: int, n: int = 3,
                 election_timeout: Tuple[float, float] = (0.15, 0.30),
                 heartbeat: float = 0.03, tick: float = 0.01,
                 drop: float = 0.0, delay: Tuple[float, float] = (0.001, 0.004),
                 snapshot_entries: int = 0, chaos: bool = False,
                 client: bool = False, verbose: bool = False):
        self.seed = seed
        self.rng = random.Random(seed)
        self.now = 0.0
        self.election_timeout = election_timeout
        self.heartbeat = heartbeat
        self.tick_s = tick
        self.drop = drop
        self.delay = delay
        self.snapshot_entries = snapshot_entries
        self.verbose = verbose
        self.members: Dict[int, _Member] = {i: _Member(i)
                                            for i in range(1, n + 1)}
        self.blocked: Set[Tuple[int, int]] = set()     # directed links
        self._heap: List[tuple] = []
        self._seq = 0
        # global history for the invariants
        self.leaders: Dict[int, int] = {}               # epoch -> member
        self.leader_history: List[Tuple[int, int]] = []  # (epoch, member)
        self.votes: Dict[Tuple[int, int], int] = {}
        self.applied: Dict[int, tuple] = {}             # index -> entry
        self.digests: Dict[int, str] = {0: ""}
        self.acked: Dict[int, tuple] = {}               # index -> entry
        self.pending: Dict[Tuple[int, int], tuple] = {}
        self.failed: List[Any] = []                     # payloads never acked
        self.stats = {"events": 0, "sent": 0, "dropped": 0, "crashes": 0,
                      "partitions": 0, "snapshots_installed": 0,
                      "compactions": 0, "proposed": 0}
        self._next_write = 0
        for m in self.members.values():
            self._boot(m)
        if chaos:
            self._push(self.rng.uniform(0.5, 1.0), "chaos", None)
        if client:
            self._push(0.05, "client", None)

    # ------------------------------------------------------------ plumbing
    def _push(self, at: float, kind: str, arg) -> None:
        self._seq += 1
        heapq.heappush(self._heap, (at, self._seq, kind, arg))

    def _log(self, *a) -> None:
        if self.verbose:
            print("[%8.3f]" % self.now, *a, file=sys.stderr)

    def _boot(self, m: _Member) -> None:
        s = m.store
        m.incarnation += 1
        m.core = QuorumCore(
            m.id, list(self.members), random.Random(
                "%d/%d/%d" % (self.seed, m.id, m.incarnation)),
            self.now, election_timeout=self.election_timeout,
            heartbeat=self.heartbeat, epoch=s.epoch, voted_for=s.voted_for,
            log=list(s.log), base_index=s.base_index,
            base_epoch=s.base_epoch, snapshot=s.snapshot)
        # the state machine restarts from the snapshot
        m.applied = s.base_index
        m.digest = s.snapshot["digest"] if s.snapshot else ""
        self._push(self.now + self.tick_s, "tick", (m.id, m.incarnation))

    # ------------------------------------------------------ fault injection
    def crash(self, node: int) -> None:
        m = self.members[node]
        if m.core is not None:
            self._log("crash", node)
            m.core = None
            self.stats["crashes"] += 1
            self._fail_pending(node)

    def restart(self, node: int) -> None:
        m = self.members[node]
        if m.core is None:
            self._log("restart", node)
            self._boot(m)

    def cut(self, a: int, b: int) -> None:
        self.blocked.add((a, b))
        self.blocked.add((b, a))

    def isolate(self, node: int) -> None:
        self.stats["partitions"] += 1
        for other in self.members:
            if other != node:
                self.cut(node, other)

    def heal(self) -> None:
        self.blocked.clear()

    # -------------------------------------------------------------- queries
    def leader(self) -> Optional[int]:
        """The serving leader with the highest epoch, if any."""
        best = None
        for m in self.members.values():
            c = m.core
            if c is not None and c.role == LEADER and c.serving:
                if best is None or c.epoch > self.members[best].core.epoch:
                    best = m.id
        return best

    def core(self, node: int) -> QuorumCore:
        return self.members[node].core

    # -------------------------------------------------------------- driving
    def propose(self, node: int, payload) -> Optional[int]:
        m = self.members[node]
        if m.core is None:
            return None
        idx = m.core.propose(payload, self.now)
        if idx is not None:
            self.stats["proposed"] += 1
            self.pending[(node, idx)] = (m.core.epoch, payload)
        self._effects(m)
        self._check()
        return idx

    def run_for(self, seconds: float) -> None:
        self.run_until(self.now + seconds)

    def run_until(self, t_end: float, stop=None) -> bool:
        while self._heap and self._heap[0][0] <= t_end:
            at, _seq, kind, arg = heapq.heappop(self._heap)
            self.now = max(self.now, at)
            self.stats["events"] += 1
            getattr(self, "_ev_" + kind)(arg)
            self._check()
            if stop is not None and stop():
                return True
        self.now = max(self.now, t_end)
        return False

    def _ev_tick(self, arg) -> None:
        node, inc = arg
        m = self.members[node]
        if m.core is None or m.incarnation != inc:
            return
        m.core.tick(self.now)
        self._effects(m)
        self._push(self.now + self.tick_s, "tick", arg)

    def _ev_deliver(self, arg) -> None:
        to, msg = arg
        m = self.members[to]
        if m.core is None or (msg["from"], to) in self.blocked:
            self.stats["dropped"] += 1
            return
        m.core.handle(msg, self.now)
        self._effects(m)

    def _ev_client(self, _arg) -> None:
        live = [m.id for m in self.members.values() if m.core is not None]
        if live:
            node = self.leader() if self.rng.random() < 0.8 else None
            if node is None:
                node = self.rng.choice(live)
            payload = {"w": self._next_write}
            m = self.members[node]
            idx = m.core.propose(payload, self.now)
            if idx is not None:
                self._next_write += 1
                self.stats["proposed"] += 1
                self.pending[(node, idx)] = (m.core.epoch, payload)
            self._effects(m)
        self._push(self.now + self.rng.uniform(0.01, 0.05), "client", None)

    def _ev_chaos(self, _arg) -> None:
        r = self.rng.random()
        lead = self.leader()
        victim = lead if (lead is not None and self.rng.random() < 0.6) \
            else self.rng.choice(list(self.members))
        down = [m.id for m in self.members.values() if m.core is None]
        if r < 0.35 and not down and not self.blocked:
            self.crash(victim)
            self._push(self.now + self.rng.uniform(0.2, 0.8), "restart",
                       victim)
        elif r < 0.70 and not down and not self.blocked:
            self._log("isolate", victim)
            self.isolate(victim)
            self._push(self.now + self.rng.uniform(0.3, 0.9), "heal", None)
        elif r < 0.85:
            self.drop = self.rng.choice([0.0, 0.05, 0.2])
        self._push(self.now + self.rng.uniform(0.4, 1.2), "chaos", None)

    def _ev_restart(self, node) -> None:
        self.restart(node)

    def _ev_heal(self, _arg) -> None:
        self._log("heal")
        self.heal()

    # -------------------------------------------------------------- effects
    def _fail_pending(self, node: int) -> None:
        for key in [k for k in self.pending if k[0] == node]:
            self.failed.append(self.pending.pop(key)[1])

    def _effects(self, m: _Member) -> None:
        core, s = m.core, m.store
        for eff in core.drain():
            kind = eff[0]
            if kind == "meta":
                _k, epoch, voted = eff
                if epoch < s.epoch:
                    raise InvariantViolation("epoch went backwards")
                s.epoch, s.voted_for = epoch, voted
                if voted is not None:
                    prior = self.votes.setdefault((m.id, epoch), voted)
                    if prior != voted:
                        raise InvariantViolation(
                            "member %d voted for %d and %d in epoch %d"
                            % (m.id, prior, voted, epoch))
            elif kind == "append":
                _k, start, entries = eff
                del s.log[start - s.base_index - 1:]
                s.log.extend(entries)
            elif kind == "snapshot":
                _k, index, epoch, data = eff
                s.log = []
                s.base_index, s.base_epoch, s.snapshot = index, epoch, data
                if self.digests.get(index) != data["digest"]:
                    raise InvariantViolation(
                        "member %d installed a snapshot at %d that does "
                        "not match the applied history" % (m.id, index))
                m.applied, m.digest = index, data["digest"]
                self.stats["snapshots_installed"] += 1
            elif kind == "send":
                _k, to, msg = eff
                if msg["t"] == "vote_resp" and msg["granted"]:
                    if self.votes.get((m.id, msg["epoch"])) != to:
                        raise InvariantViolation(
                            "member %d granted an unpersisted vote" % m.id)
                self.stats["sent"] += 1
                if (m.id, to) in self.blocked or \
                        self.rng.random() < self.drop:
                    self.stats["dropped"] += 1
                    continue
                d = self.rng.uniform(*self.delay)
                if self.rng.random() < 0.02:
                    d *= 10        # a straggler: arrives out of order
                # the wire carries JSON: no aliasing between members
                self._push(self.now + d, "deliver",
                           (to, json.loads(json.dumps(msg))))
            elif kind == "apply":
                _k, index, epoch, payload = eff
                self._applied(m, index, (epoch, payload))
            elif kind == "role":
                _k, role, epoch = eff
                self._log("member", m.id, role, "epoch", epoch)
                if role == LEADER:
                    prior = self.leaders.setdefault(epoch, m.id)
                    if prior != m.id:
                        raise InvariantViolation(
                            "two leaders in epoch %d: %d and %d"
                            % (epoch, prior, m.id))
                    self.leader_history.append((epoch, m.id))
                    self._check_leader_completeness(m)
                else:
                    self._fail_pending(m.id)
            elif kind == "serving":
                pass
        if self.snapshot_entries and core is m.core and \
                len(core.log) > self.snapshot_entries and \
                m.applied > core.base_index:
            snap = {"index": m.applied, "digest": m.digest}
            s.snapshot = snap
            drop = m.applied - s.base_index
            s.base_epoch = s.log[drop - 1][0]
            del s.log[:drop]
            s.base_index = m.applied
            core.compact(m.applied, snap)
            self.stats["compactions"] += 1

    def _applied(self, m: _Member, index: int, entry: tuple) -> None:
        if index != m.applied + 1:
            raise InvariantViolation("member %d applied %d after %d"
                                     % (m.id, index, m.applied))
        entry = (entry[0], entry[1])
        prior = self.applied.setdefault(index, entry)
        if prior != entry:
            raise InvariantViolation(
                "index %d applied as %r and as %r" % (index, prior, entry))
        m.applied = index
        m.digest = _chain(m.digest, entry)
        self.digests.setdefault(index, m.digest)
        if self.digests[index] != m.digest:
            raise InvariantViolation("history diverged at %d" % index)
        want = self.pending.pop((m.id, index), None)
        if want is not None:
            if want == entry and m.core.role == LEADER and \
                    m.core.epoch == entry[0]:
                self.acked[index] = entry
            else:
                self.failed.append(want[1])

    def _check_leader_completeness(self, m: _Member) -> None:
        core = m.core
        for index, entry in self.acked.items():
            if index <= core.base_index:
                continue
            if index > core.last_index or \
                    tuple(core.entry_at(index)) != entry:
                raise InvariantViolation(
                    "leader %d of epoch %d lacks acked entry %d"
                    % (m.id, core.epoch, index))

    def _check(self) -> None:
        cores = [m.core for m in self.members.values()
                 if m.core is not None]
        # log matching, pairwise, over the common index range
        for i in range(len(cores)):
            for j in range(i + 1, len(cores)):
                a, b = cores[i], cores[j]
                lo = max(a.base_index, b.base_index) + 1
                hi = min(a.last_index, b.last_index)
                agree = False
                for idx in range(hi, lo - 1, -1):
                    ea, eb = a.entry_at(idx), b.entry_at(idx)
                    if agree:
                        if tuple(ea) != tuple(eb):
                            raise InvariantViolation(
                                "log matching broken at %d between %d "
                                "and %d" % (idx, a.id, b.id))
                    elif ea[0] == eb[0]:
                        agree = True
                        if ea[1] != eb[1]:
                            raise InvariantViolation(
                                "same epoch, different entry at %d" % idx)
        # the disk mirrors the core
        for m in self.members.values():
            if m.core is not None:
                s = m.store
                if (s.epoch, s.voted_for, s.base_index) != \
                        (m.core.epoch, m.core.voted_for,
                         m.core.base_index) or \
                        len(s.log) != len(m.core.log):
                    raise InvariantViolation(
                        "member %d: persisted state lags the core" % m.id)

    # -------------------------------------------------------------- summary
    def settle(self, seconds: float = 3.0) -> None:
        """End of a chaos run: heal, restart everybody, stop dropping,
        and let the ensemble converge."""
        self._heap = [e for e in self._heap
                      if e[2] not in ("chaos", "heal", "restart", "client")]
        heapq.heapify(self._heap)
        self.heal()
        self.drop = 0.0
        for node in self.members:
            self.restart(node)
        self.run_for(seconds)

    def summary(self) -> dict:
        return {"seed": self.seed, "sim_seconds": round(self.now, 3),
                "acked": len(self.acked), "failed": len(self.failed),
                "leaders": len(set(self.leader_history)),
                "distinct_leader_members":
                    len({m for _e, m in self.leader_history}),
                "max_epoch": max([0] + list(self.leaders)),
                "applied": max([0] + list(self.applied)),
                **self.stats}


def run_seed(seed: int, seconds: float = 10.0, verbose: bool = False,
             n: int = 3) -> dict:
    sim = QuorumSim(seed, n=n, chaos=True, client=True, drop=0.02,
                    snapshot_entries=25, verbose=verbose)
    sim.run_for(seconds)
    sim.settle()
    # after settling every member holds the same applied history
    tops = {m.applied for m in sim.members.values()}
    digs = {m.digest for m in sim.members.values()}
    if len(tops) != 1 or len(digs) != 1:
        raise InvariantViolation("members did not converge: %r" % (tops,))
    return sim.summary()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="manatee-quorumsim")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--seeds", type=int, default=1,
                    help="run this many consecutive seeds")
    ap.add_argument("--seconds", type=float, default=10.0,
                    help="simulated seconds of chaos per seed")
    ap.add_argument("--nodes", type=int, default=3)
    ap.add_argument("-v", "--verbose", action="store_true")
    ns = ap.parse_args(argv)
    rc = 0
    for seed in range(ns.seed, ns.seed + ns.seeds):
        try:
            out = run_seed(seed, ns.seconds, ns.verbose, ns.nodes)
            out["ok"] = True
        except InvariantViolation as exc:
            out = {"seed": seed, "ok": False, "violation": str(exc)}
            rc = 1
        print(json.dumps(out))
    return rc


if __name__ == "__main__":
    sys.exit(main())
