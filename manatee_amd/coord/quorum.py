"""Consensus core for the replicated coordination server — sans-IO.

A pure state machine in the style of ``db/waldb/core.py`` and
``fsm/peer.py``: inputs are peer messages, clock ticks (the clock is an
argument, never read here) and local proposals; outputs are *effects*
the driver must carry out IN ORDER.  No sockets, no files, no ``time``.

The algorithm is leader-based log replication in the Raft shape, with
terms called *epochs*:

- one persisted vote per epoch, and a ``(lastEpoch, lastIndex)``
  up-to-date check before any vote is granted;
- AppendEntries with a prev-entry check, heartbeats, commit by majority
  match — and an entry of an older epoch is never committed by counting
  replicas, only together with an entry of the leader's own epoch;
- a new leader appends a no-op of its own epoch and reports itself
  *serving* only once that no-op is committed and applied;
- check-quorum and a leader lease: a leader that has no majority
  acknowledgement younger than the MINIMUM election timeout steps down,
  and a follower ignores vote requests for that same span after it last
  heard from a leader — so by the time a successor can be elected the
  old leader has already stopped serving.  Lease age is measured from
  the leader's SEND time (echoed back in the acknowledgement), which is
  never later than the moment the follower heard it.

Static membership, no pre-vote, no pipelining (coordination traffic is
tiny).

Effects (tuples, returned by ``drain()``; the driver performs each
before looking at the next one, so anything that must be durable before
a message leaves simply precedes that message):

``("meta", epoch, voted_for)``
    persist the epoch and vote (fsync) — precedes any vote reply.
``("append", start_index, entries)``
    make the durable log end with ``entries`` starting at
    ``start_index``: cut whatever it holds from there on, append, fsync.
    ``entries`` is a list of ``(epoch, payload)``.
``("snapshot", index, epoch, data)``
    install a snapshot received from the leader: persist it, drop the
    whole log, reset the state machine to ``data``.
``("send", peer_id, message)``
    message is a JSON-able dict.
``("apply", index, epoch, payload)``
    entry is committed; apply it.  ``payload`` None is a leader no-op.
``("role", role, epoch)``
    role changed.  Leaving ``leader`` means: stop serving NOW, fail
    whatever proposals are pending (never acknowledge them).
``("serving", epoch)``
    this leader's no-op is committed and applied: clients may be served.
"""

from __future__ import annotations

from typing import Any, Dict, Iterable, List, Optional, Tuple

FOLLOWER = "follower"
CANDIDATE = "candidate"
LEADER = "leader"

Entry = Tuple[int, Any]     # (epoch, payload)


class QuorumCore:
    def __init__(self, node_id: int, members: Iterable[int], rng,
                 now: float,
                 election_timeout: Tuple[float, float] = (0.3, 0.6),
                 heartbeat: float = 0.05,
                 epoch: int = 0, voted_for: Optional[int] = None,
                 log: Iterable[Entry] = (),
                 base_index: int = 0, base_epoch: int = 0,
                 snapshot: Any = None, max_batch: int = 256):
        self.id = node_id
        self.members = sorted(set(members))
        if node_id not in self.members:
            raise ValueError("node %r is not a member" % (node_id,))
        self.peers = [m for m in self.members if m != node_id]
        self.majority = len(self.members) // 2 + 1
        self.rng = rng
        self.el_min, self.el_max = election_timeout
        self.heartbeat = heartbeat
        self.max_batch = max_batch

        # persistent (mirrors what the driver has on disk)
        self.epoch = epoch
        self.voted_for = voted_for
        self.log: List[Entry] = [(e, p) for e, p in log]
        self.base_index = base_index
        self.base_epoch = base_epoch
        self.snapshot = snapshot

        # volatile
        self.role = FOLLOWER
        self.leader_id: Optional[int] = None
        self.commit_index = base_index
        self.serving = False
        # a restarted member has forgotten when it last heard a leader;
        # assume "just now" so the vote embargo still covers the lease
        self.leader_contact = now
        self.election_deadline = now + self._draw()
        self.votes: set = set()
        self.next_index: Dict[int, int] = {}
        self.match_index: Dict[int, int] = {}
        self.heard: Dict[int, float] = {}
        self.next_heartbeat = 0.0
        self.noop_index = 0
        self._out: List[tuple] = []

    # -------------------------------------------------------------- helpers
    def _draw(self) -> float:
        return self.rng.uniform(self.el_min, self.el_max)

    @property
    def last_index(self) -> int:
        return self.base_index + len(self.log)

    @property
    def last_epoch(self) -> int:
        return self.log[-1][0] if self.log else self.base_epoch

    def epoch_at(self, index: int) -> int:
        if index == self.base_index:
            return self.base_epoch
        return self.log[index - self.base_index - 1][0]

    def entry_at(self, index: int) -> Entry:
        return self.log[index - self.base_index - 1]

    def drain(self) -> List[tuple]:
        out, self._out = self._out, []
        return out

    def _send(self, to: int, msg: dict) -> None:
        msg["from"] = self.id
        msg["epoch"] = self.epoch
        self._out.append(("send", to, msg))

    def _quorum_ts(self, now: float) -> float:
        """The youngest instant at which a majority (self included) is
        known to have followed this leader."""
        ts = sorted([now] + [self.heard[p] for p in self.peers],
                    reverse=True)
        return ts[self.majority - 1]

    def has_lease(self, now: float) -> bool:
        return self.role == LEADER and \
            now - self._quorum_ts(now) < self.el_min

    # ---------------------------------------------------------- transitions
    def _set_role(self, role: str) -> None:
        if role != self.role:
            self.role = role
            if role != LEADER:
                self.serving = False
            self._out.append(("role", role, self.epoch))

    def _become_follower(self, epoch: int, now: float) -> None:
        if epoch > self.epoch:
            self.epoch = epoch
            self.voted_for = None
            self.leader_id = None
            self._out.append(("meta", self.epoch, self.voted_for))
        if self.role != FOLLOWER:
            self.election_deadline = now + self._draw()
        self._set_role(FOLLOWER)

    def _start_election(self, now: float) -> None:
        self.epoch += 1
        self.voted_for = self.id
        self.leader_id = None
        self.votes = {self.id}
        self._out.append(("meta", self.epoch, self.voted_for))
        self.election_deadline = now + self._draw()
        if self.role != CANDIDATE:
            self.role = CANDIDATE
            self.serving = False
        # report every new candidacy: the epoch moved
        self._out.append(("role", CANDIDATE, self.epoch))
        for p in self.peers:
            self._send(p, {"t": "vote_req", "last_index": self.last_index,
                           "last_epoch": self.last_epoch})
        if len(self.votes) >= self.majority:
            self._become_leader(now)

    def _become_leader(self, now: float) -> None:
        self.role = LEADER
        self.leader_id = self.id
        self.serving = False
        self.next_index = {p: self.last_index + 1 for p in self.peers}
        self.match_index = {p: 0 for p in self.peers}
        self.heard = {p: now for p in self.peers}
        self._out.append(("role", LEADER, self.epoch))
        self.log.append((self.epoch, None))
        self.noop_index = self.last_index
        self._out.append(("append", self.last_index, [(self.epoch, None)]))
        self._broadcast(now)
        self._advance_commit()

    # --------------------------------------------------------------- inputs
    def tick(self, now: float) -> None:
        if self.role == LEADER:
            if now - self._quorum_ts(now) >= self.el_min:
                # check-quorum: no majority has acknowledged anything
                # sent within the lease; somebody else may be elected
                self.election_deadline = now + self._draw()
                self.leader_id = None
                self._set_role(FOLLOWER)
            elif now >= self.next_heartbeat:
                self._broadcast(now)
        elif now >= self.election_deadline:
            self._start_election(now)

    def propose(self, payload: Any, now: float) -> Optional[int]:
        """Append a client entry; returns its index, or None when this
        member may not accept it (not a serving leader, or lease lost)."""
        if payload is None:
            raise ValueError("None is reserved for the leader no-op")
        if self.role != LEADER or not self.serving or \
                not self.has_lease(now):
            return None
        self.log.append((self.epoch, payload))
        self._out.append(("append", self.last_index,
                          [(self.epoch, payload)]))
        self._broadcast(now)
        self._advance_commit()
        return self.last_index

    def compact(self, index: int, snapshot: Any) -> None:
        """The driver has durably written ``snapshot`` covering
        everything up to and including ``index`` (applied): forget the
        log up to there."""
        if index <= self.base_index:
            return
        if index > self.commit_index:
            raise ValueError("cannot compact past the commit index")
        epoch = self.epoch_at(index)
        del self.log[:index - self.base_index]
        self.base_index = index
        self.base_epoch = epoch
        self.snapshot = snapshot

    def handle(self, msg: dict, now: float) -> None:
        t = msg.get("t")
        if msg.get("from") not in self.peers:
            return
        if t == "vote_req":
            self._on_vote_req(msg, now)
        elif t == "vote_resp":
            self._on_vote_resp(msg, now)
        elif t == "append":
            self._on_append(msg, now)
        elif t == "snap":
            self._on_snap(msg, now)
        elif t == "append_resp":
            self._on_append_resp(msg, now)

    # ---------------------------------------------------------------- votes
    def _on_vote_req(self, msg: dict, now: float) -> None:
        if msg["epoch"] < self.epoch:
            self._send(msg["from"], {"t": "vote_resp", "granted": False})
            return
        # lease: a live leader was heard less than one minimum election
        # timeout ago (or this member IS the leader and check-quorum has
        # not fired): the request is ignored outright — not even the
        # epoch is adopted
        if self.role == LEADER:
            return
        if self.role == FOLLOWER and now - self.leader_contact < self.el_min:
            return
        if msg["epoch"] > self.epoch:
            self._become_follower(msg["epoch"], now)
        up_to_date = (msg["last_epoch"], msg["last_index"]) >= \
            (self.last_epoch, self.last_index)
        grant = up_to_date and self.voted_for in (None, msg["from"]) \
            and self.role == FOLLOWER
        if grant:
            if self.voted_for is None:
                self.voted_for = msg["from"]
                self._out.append(("meta", self.epoch, self.voted_for))
            self.election_deadline = now + self._draw()
        self._send(msg["from"], {"t": "vote_resp", "granted": grant})

    def _on_vote_resp(self, msg: dict, now: float) -> None:
        if msg["epoch"] > self.epoch:
            self._become_follower(msg["epoch"], now)
            return
        if self.role != CANDIDATE or msg["epoch"] != self.epoch:
            return
        if msg.get("granted"):
            self.votes.add(msg["from"])
            if len(self.votes) >= self.majority:
                self._become_leader(now)

    # ---------------------------------------------------------- replication
    def _broadcast(self, now: float) -> None:
        self.next_heartbeat = now + self.heartbeat
        for p in self.peers:
            self._send_append(p, now)

    def _send_append(self, p: int, now: float) -> None:
        nxt = self.next_index[p]
        if nxt <= self.base_index:
            # the entries this follower needs are compacted away
            self._send(p, {"t": "snap", "last_index": self.base_index,
                           "last_epoch": self.base_epoch,
                           "data": self.snapshot, "ts": now})
            return
        prev = nxt - 1
        lo = prev - self.base_index
        entries = [[e, pl] for e, pl in self.log[lo:lo + self.max_batch]]
        self._send(p, {"t": "append", "prev_index": prev,
                       "prev_epoch": self.epoch_at(prev),
                       "entries": entries, "commit": self.commit_index,
                       "ts": now})

    def _follow_leader(self, msg: dict, now: float) -> bool:
        """Common head of append/snap handling; False = stale sender."""
        if msg["epoch"] < self.epoch:
            self._send(msg["from"], {"t": "append_resp", "ok": False,
                                     "match": 0, "hint": 0,
                                     "ts": msg.get("ts", 0.0)})
            return False
        if msg["epoch"] > self.epoch or self.role != FOLLOWER:
            # same epoch + leader role cannot happen (one leader per
            # epoch); a candidate of this epoch yields to its winner
            if self.role == LEADER and msg["epoch"] == self.epoch:
                raise AssertionError("two leaders in epoch %d" % self.epoch)
            self._become_follower(msg["epoch"], now)
        self.leader_id = msg["from"]
        self.leader_contact = now
        self.election_deadline = now + self._draw()
        return True

    def _on_append(self, msg: dict, now: float) -> None:
        if not self._follow_leader(msg, now):
            return
        prev = msg["prev_index"]
        entries = [(e, p) for e, p in msg["entries"]]
        if prev < self.base_index:
            # the head of this batch is already inside our snapshot
            skip = self.base_index - prev
            entries = entries[skip:]
            prev = self.base_index
            if skip > len(msg["entries"]):
                self._ack(msg, True, self.base_index)
                return
        elif prev > self.last_index or \
                self.epoch_at(prev) != msg["prev_epoch"]:
            hint = min(prev - 1, self.last_index)
            self._ack(msg, False, 0, max(hint, self.commit_index))
            return
        # find the first entry that is new or conflicts
        idx = prev
        new_from = None
        for k, (e, _p) in enumerate(entries):
            idx = prev + 1 + k
            if idx > self.last_index or self.epoch_at(idx) != e:
                new_from = k
                break
        if new_from is not None:
            start = prev + 1 + new_from
            if start <= self.commit_index:
                raise AssertionError("leader asks to rewrite committed "
                                     "entry %d" % start)
            del self.log[start - self.base_index - 1:]
            fresh = entries[new_from:]
            self.log.extend(fresh)
            self._out.append(("append", start, list(fresh)))
        matched = prev + len(entries)
        self._commit_to(min(msg["commit"], matched))
        self._ack(msg, True, matched)

    def _on_snap(self, msg: dict, now: float) -> None:
        if not self._follow_leader(msg, now):
            return
        idx = msg["last_index"]
        if self.commit_index < idx <= self.last_index and \
                self.epoch_at(idx) == msg["last_epoch"]:
            # this member already holds the snapshot's last entry, so by
            # log matching everything up to it: keep the durable log —
            # entries beyond idx may be acknowledged and counted — and
            # take from the snapshot only the news that idx is committed
            self._commit_to(idx)
            self._ack(msg, True, idx)
        elif idx > self.commit_index:
            self.log = []
            self.base_index = idx
            self.base_epoch = msg["last_epoch"]
            self.snapshot = msg["data"]
            self.commit_index = idx
            self._out.append(("snapshot", idx, msg["last_epoch"],
                              msg["data"]))
            self._ack(msg, True, idx)
        else:
            self._ack(msg, True, self.commit_index)

    def _ack(self, msg: dict, ok: bool, match: int, hint: int = 0) -> None:
        self._send(msg["from"], {"t": "append_resp", "ok": ok,
                                 "match": match, "hint": hint,
                                 "ts": msg.get("ts", 0.0)})

    def _on_append_resp(self, msg: dict, now: float) -> None:
        if msg["epoch"] > self.epoch:
            self._become_follower(msg["epoch"], now)
            return
        if self.role != LEADER or msg["epoch"] != self.epoch:
            return
        p = msg["from"]
        self.heard[p] = max(self.heard[p], min(msg.get("ts", 0.0), now))
        if msg["ok"]:
            advanced = msg["match"] > self.match_index[p]
            if advanced:
                self.match_index[p] = msg["match"]
            self.next_index[p] = max(self.next_index[p],
                                     self.match_index[p] + 1)
            self._advance_commit()
            if advanced and self.next_index[p] <= self.last_index:
                self._send_append(p, now)     # catch-up: keep going
        else:
            # the follower's own account of its log wins over what it
            # acknowledged earlier: a member replaced with an empty data
            # directory really is behind its old match.  (A stale,
            # reordered reject only makes the leader re-send; lowering
            # match is always safe.)
            nxt = max(1, min(msg["hint"] + 1, self.next_index[p]))
            self.match_index[p] = min(self.match_index[p], nxt - 1)
            if nxt != self.next_index[p]:
                self.next_index[p] = nxt
                self._send_append(p, now)

    def _advance_commit(self) -> None:
        matches = sorted([self.last_index] +
                         [self.match_index[p] for p in self.peers],
                         reverse=True)
        n = matches[self.majority - 1]
        # only an entry of the CURRENT epoch commits by counting; older
        # ones ride along with it
        if n > self.commit_index and self.epoch_at(n) == self.epoch:
            self._commit_to(n)
            if not self.serving and self.commit_index >= self.noop_index:
                self.serving = True
                self._out.append(("serving", self.epoch))

    def _commit_to(self, n: int) -> None:
        while self.commit_index < n:
            self.commit_index += 1
            e, p = self.entry_at(self.commit_index)
            self._out.append(("apply", self.commit_index, e, p))
