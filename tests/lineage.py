"""A model of WAL lineage: who may stream from whom, stated from bytes.

Plain Python, no server code (``tests/zkmodel.py`` is the same idea for
the coordination tree).  A model peer is a list of records, a WAL start,
a timeline and a history; the operations are the ones that move real
peers apart and together: write, copy, follow, promote, recycle and a
crash that loses an unsynced tail.

The truth about an ordered pair ``(f, u)`` of one lineage is read off
the bytes alone:

``prefix(f, u)``
    ``f``'s bytes in ``[max(starts), f.end)`` are ``u``'s at the same
    offsets and ``f.end <= u.end``.
``lcp(f, u)``
    the greatest record boundary of both below which their bytes agree.

and so is the verdict the replication handshake owes the pair
(``expected``).  ``docs/wal-divergence.md`` promises it;
``tests/test_wal_lineage.py`` holds the handshake and the rewind
arithmetic against it.

Payloads are WAL ops a waldb server replays (puts and deletes over eight
keys), every one unique, most of ONE size: the record boundaries of two
branches then coincide, which is what lets a diverged follower's end
look like a boundary of its upstream.
"""

import json
import random
import struct
import zlib

_HDR = struct.Struct(">II")
KEYS = 8
# padding of a put's value: most records come out the same size
PADS = (0, 0, 0, 0, 0, 3, 16)

REFUSALS = ("timeline-mismatch", "diverged", "wal-gone")


def frame(payload: bytes) -> bytes:
    return _HDR.pack(len(payload), zlib.crc32(payload)) + payload


class Peer:
    """``records`` is the whole log from offset 0; ``wal_start`` says how
    much of it is still on disk.  What was recycled stays in the list so
    that offsets are list arithmetic, and is never read."""

    def __init__(self, name, records=(), wal_start=0, timeline=1,
                 history=({"tl": 1, "at": 0},)):
        self.name = name
        self.records = list(records)
        self.wal_start = wal_start
        self.timeline = timeline
        self.history = [dict(h) for h in history]
        self.upstream = None     # whom it followed last
        self._touch()

    # ---------------------------------------------------------- bytes
    def _touch(self):
        """After every change of ``records``."""
        self._bytes = None
        marks, pos = [0], 0
        for r in self.records:
            pos += _HDR.size + len(r)
            marks.append(pos)
        self._marks, self.end = marks, pos
        self.markset = frozenset(marks)

    @property
    def bytes(self) -> bytes:
        if self._bytes is None:
            self._bytes = b"".join(frame(r) for r in self.records)
        return self._bytes

    def boundaries(self):
        """Every record boundary from 0 to ``end``."""
        return self._marks

    def read(self, lo: int, hi: int) -> bytes:
        assert self.wal_start <= lo <= hi <= self.end, \
            "%s: read [%d, %d) outside [%d, %d)" % (
                self.name, lo, hi, self.wal_start, self.end)
        return self.bytes[lo:hi]

    def records_upto(self, lsn: int):
        out, pos = [], 0
        for r in self.records:
            pos += _HDR.size + len(r)
            if pos > lsn:
                break
            out.append(r)
        return out

    def kv_at(self, lsn: int) -> dict:
        """What a server that replayed the log up to ``lsn`` serves."""
        kv = {}
        for r in self.records_upto(lsn):
            op = json.loads(r)
            if op["op"] == "put":
                kv[op["k"]] = op["v"]
            else:
                kv.pop(op["k"], None)
        return kv

    def describe(self) -> str:
        return "%s tl=%d wal=[%d,%d) history=%s" % (
            self.name, self.timeline, self.wal_start, self.end,
            [(h["tl"], h["at"]) for h in self.history])


# ------------------------------------------------------------------ truth
def prefix(f: Peer, u: Peer) -> bool:
    lo = max(f.wal_start, u.wal_start)
    if f.end > u.end:
        return False
    return lo >= f.end or f.bytes[lo:f.end] == u.bytes[lo:f.end]


def whole_prefix(f: Peer, u: Peer) -> bool:
    """``prefix`` over everything either ever wrote, recycled or not:
    tells a follower that merely fell behind from one that also forked."""
    return f.end <= u.end and u.bytes.startswith(f.bytes)


def lcp(f: Peer, u: Peer) -> int:
    n = 0
    for a, b in zip(f.records, u.records):
        if a != b:
            break
        n += 1
    return f.boundaries()[n]


def reasons(f: Peer, u: Peer) -> set:
    """Every reason the handshake has to refuse ``f`` as a follower of
    ``u``; empty means it must accept."""
    out = set()
    if f.timeline > u.timeline:
        out.add("timeline-mismatch")
    if not prefix(f, u):
        out.add("diverged")
    elif f.end < u.wal_start:
        # prefix() held on an empty overlap
        out.add("wal-gone")
        if not whole_prefix(f, u):
            out.add("diverged")
    return out


def blind(f: Peer, u: Peer) -> bool:
    """The two logs forked, and no byte that would show it is on disk
    on both sides: ``f`` has no WAL left below its end, or ends exactly
    where ``u``'s begins.  ``prefix`` holds on the empty overlap, so by
    the bytes on disk the handshake may accept, and it cannot do better
    unless the histories happen to show the fork.  The one kind of pair
    whose verdict the model does not pin."""
    return f.end >= u.wal_start and f.end <= u.end and \
        max(f.wal_start, u.wal_start) >= f.end and not whole_prefix(f, u)


def expected(f: Peer, u: Peer):
    """``None`` (accept), the one refusal that applies, ``"refused"``
    where more than one does and the word is not pinned, or ``"any"``
    for a ``blind`` pair."""
    if blind(f, u):
        return "any"
    why = reasons(f, u)
    if not why:
        return None
    return why.pop() if len(why) == 1 else "refused"


def agrees(verdict, want) -> bool:
    """Does the handshake's ``verdict`` (None or a refusal) meet what
    ``expected`` returned?"""
    if want == "any":
        return verdict is None or verdict in REFUSALS
    if want == "refused":
        return verdict in REFUSALS
    return verdict == want


def switch_above(f: Peer, u: Peer):
    """``at`` of ``u``'s first switch to a timeline above ``f``'s."""
    for h in u.history:
        if h["tl"] > f.timeline:
            return h["at"]
    return None


# --------------------------------------------------------------- programs
class World:
    """Up to ``max_peers`` peers of one lineage and a seeded stream of
    operations over them.  ``step()`` applies one and returns its
    description."""

    def __init__(self, seed: int, max_peers: int = 5):
        self.rng = random.Random(seed)
        self.max_peers = max_peers
        self.serial = 0
        self.names = 0
        self.peers = []
        self.last_copy = None    # (new, source) while the step is the copy
        first = self._new_peer()
        self.write(first, 3)

    def _new_peer(self, like: Peer = None) -> Peer:
        name = "p%d" % self.names
        self.names += 1
        p = Peer(name) if like is None else Peer(
            name, like.records, like.wal_start, like.timeline, like.history)
        self.peers.append(p)
        return p

    def peer(self, name: str) -> Peer:
        return next(p for p in self.peers if p.name == name)

    # ------------------------------------------------------ operations
    def _payload(self, pad: int = None) -> bytes:
        self.serial += 1
        rng = self.rng
        key = "k%d" % rng.randrange(KEYS)
        if pad is not None:
            op = {"op": "put", "k": key, "v": "%05d" % self.serial + "x" * pad}
        elif rng.random() < 0.1:
            op = {"op": "del", "k": key, "n": "%05d" % self.serial}
        else:
            op = {"op": "put", "k": key,
                  "v": "%05d" % self.serial + "x" * rng.choice(PADS)}
        return json.dumps(op, separators=(",", ":")).encode()

    def write(self, p: Peer, n: int, pad: int = None) -> None:
        """``pad`` fixes the kind and size of the records (a put with
        that much padding); the default draws both."""
        for _ in range(n):
            p.records.append(self._payload(pad))
        p._touch()

    def copy(self, p: Peer) -> Peer:
        q = self._new_peer(p)
        self.last_copy = (q.name, p.name)
        return q

    def follow(self, f: Peer, u: Peer, upto: int) -> None:
        """``f`` streams from ``u`` up to ``u``'s boundary ``upto`` and
        adopts its timeline and history, as the handshake does whatever
        ``upto`` is.  Only for a pair that may."""
        assert not reasons(f, u) and whole_prefix(f, u) and upto >= f.end
        f.records = u.records_upto(upto)
        f.timeline = u.timeline
        f.history = [dict(h) for h in u.history]
        f.upstream = u.name
        f._touch()
        assert f.end == upto

    def promote(self, p: Peer) -> None:
        p.timeline += 1
        p.history.append({"tl": p.timeline, "at": p.end})

    def recycle(self, p: Peer, lsn: int) -> None:
        assert p.wal_start <= lsn <= p.end and lsn in p.boundaries()
        p.wal_start = lsn

    def crash_truncate(self, p: Peer, n: int) -> None:
        """Lose the last ``n`` records.  The floor is the last switch
        point (a promotion makes the WAL below it durable first) and
        the WAL start."""
        floor = max(p.wal_start, p.history[-1]["at"])
        while n > 0 and p.records and \
                p.end - _HDR.size - len(p.records[-1]) >= floor:
            p.records.pop()
            p._touch()
            n -= 1

    # ------------------------------------------------------- generator
    OPS = (("write", 30), ("copy", 12), ("follow", 22), ("promote", 14),
           ("recycle", 8), ("crash_truncate", 8), ("twin", 6))

    def step(self) -> str:
        rng = self.rng
        self.last_copy = None
        names, weights = zip(*self.OPS)
        for _ in range(20):
            op = rng.choices(names, weights)[0]
            done = getattr(self, "_gen_" + op)()
            if done:
                return done
        return self._gen_write()

    def _gen_write(self):
        p = rng_choice(self.rng, self.peers)
        n = self.rng.randint(1, 3)
        self.write(p, n)
        return "write(%s, %d)" % (p.name, n)

    def _gen_copy(self):
        if len(self.peers) >= self.max_peers:
            return None
        p = rng_choice(self.rng, self.peers)
        q = self.copy(p)
        return "copy(%s -> %s)" % (p.name, q.name)

    def _gen_twin(self):
        """A copy and a promotion of both sides: two peers that went to
        the same timeline number at the same offset, then wrote."""
        if len(self.peers) >= self.max_peers:
            return None
        p = rng_choice(self.rng, self.peers)
        q = self.copy(p)
        self.promote(p)
        self.promote(q)
        self.write(p, self.rng.randint(1, 3))
        self.write(q, self.rng.randint(1, 2))
        return "twin(%s, %s)" % (p.name, q.name)

    def _gen_follow(self):
        rng = self.rng
        pairs = [(f, u) for f in self.peers for u in self.peers
                 if f is not u and not reasons(f, u) and whole_prefix(f, u)
                 and (u.end > f.end or u.history != f.history)]
        if not pairs:
            return None
        f, u = rng_choice(rng, pairs)
        marks = [b for b in u.boundaries() if b >= f.end]
        # mostly all the way; sometimes exactly to a switch point or short
        upto = marks[-1]
        roll = rng.random()
        at = switch_above(f, u)
        if roll < 0.25 and at in marks:
            upto = at
        elif roll < 0.45:
            upto = rng_choice(rng, marks)
        self.follow(f, u, upto)
        return "follow(%s <- %s, %d)" % (f.name, u.name, upto)

    def _gen_promote(self):
        p = rng_choice(self.rng, self.peers)
        if p.timeline >= 4:
            return None
        self.promote(p)
        return "promote(%s)" % p.name

    def _gen_recycle(self):
        p = rng_choice(self.rng, self.peers)
        # recycling drops whole segments and keeps the last: never all
        marks = [b for b in p.boundaries() if p.wal_start < b < p.end]
        if not marks:
            return None
        lsn = rng_choice(self.rng, marks)
        self.recycle(p, lsn)
        return "recycle(%s, %d)" % (p.name, lsn)

    def _gen_crash_truncate(self):
        p = rng_choice(self.rng, self.peers)
        before = p.end
        self.crash_truncate(p, self.rng.randint(1, 3))
        if p.end == before:
            return None
        return "crash_truncate(%s) %d -> %d" % (p.name, before, p.end)


def rng_choice(rng, seq):
    return seq[rng.randrange(len(seq))]


def run_program(seed: int, steps: int = 30, max_peers: int = 5):
    """Yield ``(step number, description, world)`` after every step of
    the seeded program; the world is live, look before the next step."""
    world = World(seed, max_peers)
    yield 0, "init", world
    for i in range(1, steps + 1):
        yield i, world.step(), world
