"""The replication handshake and the rewind arithmetic against a model
of WAL lineage (``tests/lineage.py``).

``docs/wal-divergence.md`` promises that a standby whose WAL is not a
byte prefix of its upstream's is refused at the handshake.  The rules,
one test each below, then for every ordered pair of peers after every
step of 300 seeded programs:

* **safety**: not a prefix ⇒ refused;
* **no spurious restore**: the model says accept ⇒ accepted; and where
  exactly one refusal applies, that word;
* **rewind**: ``fork_point`` is at or below the greatest common record
  boundary, or else the rewind refuses (the CRC over the probe window
  differs, or there is no window to probe).

Level 1 calls the handshake's pure functions (``rewind.check_follower``,
``handshake_offer``, ``handshake_verify``: what ``ReplCore`` calls) with
the model's byte strings.  Level 2 writes model peers out as data
directories and lets real servers shake hands, stream, refuse and
rewind.  A failure names seed, step and pair; ``lineage.run_program``
replays it.
"""

import asyncio
import collections
import json
import os
import shutil
import zlib

import pytest

from manatee_amd.common import confparser
from manatee_amd.common.logging import null_logger
from manatee_amd.db.waldb import rewind
from manatee_amd.db.waldb.server import WaldbServer
from manatee_amd.db.waldb.wal import Wal
from tests import lineage
from tests.lineage import Peer, World
from tests.minipg_inproc import start_minipg, stop_minipg
from tests.rewind_util import SEGMENT_BYTES, wal_bytes

N_PROGRAMS = 300
N_STEPS = 30

# what the 300 programs have to reach, each at least once
MUST_OCCUR = (
    "accept",
    "diverged on a lower timeline",
    "twin promotion, different at",
    "twin promotion, same at, different bytes after it",
    "follower end is no record boundary of the upstream",
    "follower ahead of the upstream",
    "timeline-mismatch",
    "wal-gone",
    "accept at end == at",
    "accept two timelines behind",
    "accept of a cascaded follower",
    "accept of a fresh copy",
)


# ====================================================================
# the code under test, without sockets
# ====================================================================
def handshake(f: Peer, u: Peer):
    """What happens when ``f`` asks to stream from ``u``: None (it
    streams) or the refusal.  Upstream's half, the answer as JSON on the
    wire, then the follower's half."""
    err = rewind.check_follower(f.timeline, f.history, f.end,
                                u.timeline, u.history, u.wal_start, u.end)
    if err:
        return err
    answer = json.loads(json.dumps(
        rewind.handshake_offer(f.wal_start, u.wal_start, f.end, u.read)))
    if not rewind.handshake_verify(answer, f.end, f.read):
        return "diverged"
    return None


def model_says(f: Peer, u: Peer):
    """The handshake stubbed to the model's own answer: the guard test
    must hold on this alone."""
    want = lineage.expected(f, u)
    if want == "any":
        return None
    return "diverged" if want == "refused" else want


def rewind_goes_ahead(f: Peer, u: Peer, fork: int) -> bool:
    """Would ``rewind_data_dir`` cut ``f`` at ``fork``?  Its checks:
    a non-empty probe window inside both WALs, a record boundary of
    ``f``, equal CRCs."""
    window = rewind.probe_window(f.wal_start, u.wal_start, fork)
    if not window < fork <= min(f.end, u.end):
        return False
    if fork not in f.markset:
        return False
    return zlib.crc32(f.read(window, fork)) == \
        zlib.crc32(u.read(window, fork))


def _extent(peer: Peer, n: int) -> int:
    """The peer's extent on the timeline the first ``n`` history entries
    end on: its next switch point, else its WAL end."""
    return peer.history[n]["at"] if n < len(peer.history) else peer.end


def check_rewind(f: Peer, u: Peer):
    """None, or what is wrong with ``fork_point`` for this pair."""
    _tl, fork = rewind.fork_point(f.timeline, f.history, f.end,
                                  u.timeline, u.history, u.end)
    common = lineage.lcp(f, u)
    if fork > common and rewind_goes_ahead(f, u, fork):
        return "fork point %d is above the common bytes (%d) and the " \
               "probe does not notice" % (fork, common)
    if f.history != u.history:
        n = len(rewind.common_prefix(f.history, u.history))
        if common in (_extent(f, n), _extent(u, n)) and fork != common:
            return "fork point %d, but the common bytes end on a switch " \
                   "point or WAL end, %d" % (fork, common)
    return None


def classify(world: World, f: Peer, u: Peer, want) -> list:
    """Which of ``MUST_OCCUR`` this pair is, from the model alone."""
    out = []
    same_tl = f.timeline == u.timeline and f.timeline > 1
    if want is None:
        out.append("accept")
        if f.timeline < u.timeline and \
                f.end == lineage.switch_above(f, u):
            out.append("accept at end == at")
        if f.timeline + 2 <= u.timeline:
            out.append("accept two timelines behind")
        if f.upstream == u.name and u.upstream is not None \
                and f.end < u.end:
            out.append("accept of a cascaded follower")
        if world.last_copy == (f.name, u.name):
            out.append("accept of a fresh copy")
    elif want in ("timeline-mismatch", "wal-gone"):
        out.append(want)
    if want == "diverged" and f.timeline < u.timeline:
        out.append("diverged on a lower timeline")
    if want == "diverged" and same_tl and f.history != u.history \
            and [h["tl"] for h in f.history] == [h["tl"] for h in u.history]:
        out.append("twin promotion, different at")
    if want == "diverged" and same_tl and f.history == u.history \
            and lineage.lcp(f, u) == f.history[-1]["at"] \
            and min(f.end, u.end) > f.history[-1]["at"]:
        out.append("twin promotion, same at, different bytes after it")
    if f.end < u.end and f.end not in u.markset:
        out.append("follower end is no record boundary of the upstream")
    if f.end > u.end:
        out.append("follower ahead of the upstream")
    return out


class Report:
    def __init__(self):
        self.pairs = self.blind = 0
        self.seen = collections.Counter()
        self.unsafe, self.spurious, self.rewind = [], [], []


def _where(seed, step, what, f, u, verdict, want):
    return "seed %d step %d (%s): %s -> %s\n    f: %s\n    u: %s\n    " \
           "handshake: %r  model: %r" % (
               seed, step, what, f.name, u.name, f.describe(), u.describe(),
               verdict, want)


def sweep(seeds, decide=handshake, arithmetic=True) -> Report:
    """Every ordered pair after every step of every program.  No pair
    is skipped; ``Report.blind`` counts those whose verdict the model
    does not pin (``lineage.blind``)."""
    rep = Report()
    for seed in seeds:
        for step, what, world in lineage.run_program(seed, N_STEPS):
            for f in world.peers:
                for u in world.peers:
                    if f is u:
                        continue
                    rep.pairs += 1
                    want = lineage.expected(f, u)
                    verdict = decide(f, u)
                    rep.blind += want == "any"
                    for kind in classify(world, f, u, want):
                        rep.seen[kind] += 1
                    if verdict is None and not lineage.prefix(f, u):
                        rep.unsafe.append(_where(seed, step, what, f, u,
                                                 verdict, want))
                    elif not lineage.agrees(verdict, want):
                        rep.spurious.append(_where(seed, step, what, f, u,
                                                   verdict, want))
                    wrong = arithmetic and check_rewind(f, u)
                    if wrong:
                        rep.rewind.append(
                            _where(seed, step, what, f, u, verdict, want)
                            + "\n    " + wrong)
    return rep


def _show(failures) -> str:
    return "%d pairs, the first:\n%s" % (len(failures),
                                         "\n".join(failures[:3]))


# ====================================================================
# the rules, one by one
# ====================================================================
def _world(n=5) -> tuple:
    """A world whose one peer ``a`` holds ``n`` records of one size."""
    world = World(0)
    a = world.peers[0]
    a.records.clear()
    world.write(a, n, pad=0)
    return world, a


def case_fresh_copy():
    world, a = _world()
    return world.copy(a), a, None


def case_behind_on_the_same_timeline():
    world, a = _world()
    f = world.copy(a)
    world.write(a, 3)
    return f, a, None


def case_lower_timeline_end_at_the_switch():
    world, a = _world()
    f = world.copy(a)
    world.promote(a)
    world.write(a, 2, pad=0)
    assert f.end == a.history[-1]["at"]
    return f, a, None


def case_two_timelines_behind():
    world, a = _world()
    f = world.copy(a)
    world.write(a, 1, pad=0)
    world.promote(a)
    world.write(a, 2, pad=0)
    world.promote(a)
    world.write(a, 1, pad=0)
    return f, a, None


def case_cascaded_follower():
    world, a = _world()
    b, c = world.copy(a), world.copy(a)
    world.promote(a)
    world.write(a, 3, pad=0)
    world.follow(b, a, a.boundaries()[-2])
    assert c.timeline < b.timeline and b.end < a.end
    return c, b, None


def case_promoted_apart_nothing_written():
    """Twin promotions at different offsets, but the follower wrote
    nothing on its timeline: still a prefix."""
    world, a = _world()
    f = world.copy(a)
    world.write(a, 2, pad=0)
    world.promote(f)
    world.promote(a)
    world.write(a, 1, pad=0)
    return f, a, None


def case_freshly_restored():
    """No WAL below its end: nothing to compare, accepted."""
    world, a = _world()
    f = world.copy(a)
    f.wal_start = f.end
    world.write(a, 2, pad=0)
    return f, a, None


def case_wal_past_the_switch():
    world, a = _world()
    b = world.copy(a)
    world.write(a, 2, pad=0)
    world.promote(b)
    world.write(b, 3, pad=0)
    return a, b, "diverged"


def case_twin_promotion_same_at():
    """Both went 1→2 at the same offset and wrote records of one size:
    equal histories, ends on each other's boundaries."""
    world, a = _world()
    b, c = world.copy(a), world.copy(a)
    world.promote(b)
    world.write(b, 3, pad=0)
    world.promote(c)
    world.write(c, 1, pad=0)
    assert b.history == c.history and c.end in b.boundaries()
    return c, b, "diverged"


def case_twin_promotion_different_at():
    world, a = _world()
    b = world.copy(a)
    world.write(a, 1, pad=0)
    c = world.copy(a)
    world.promote(b)
    world.write(b, 4, pad=0)
    world.promote(c)
    world.write(c, 1, pad=0)
    assert b.timeline == c.timeline and b.history != c.history
    assert b.history[-1]["at"] < c.history[-1]["at"] < c.end < b.end
    return c, b, "diverged"


def case_follower_ahead():
    world, a = _world()
    f = world.copy(a)
    world.write(f, 1, pad=0)
    return f, a, "diverged"


def case_end_inside_a_record():
    """Same timeline, same history, the follower's end is inside a
    record of the upstream."""
    world, a = _world()
    f = world.copy(a)
    world.write(f, 1, pad=3)
    world.write(a, 2, pad=0)
    assert f.end < a.end and f.end not in a.boundaries()
    return f, a, "diverged"


def case_upstream_lost_a_tail():
    """The upstream crashed, lost records the follower holds and wrote
    others over them.  Nothing in the histories shows it."""
    world, a = _world()
    f = world.copy(a)
    world.crash_truncate(a, 2)
    world.write(a, 3, pad=0)
    assert f.history == a.history and f.end in a.boundaries()
    return f, a, "diverged"


def case_follower_promoted():
    world, a = _world()
    f = world.copy(a)
    world.promote(f)
    world.write(a, 1, pad=0)
    return f, a, "timeline-mismatch"


def case_behind_recycled_wal():
    world, a = _world()
    f = world.copy(a)
    world.write(a, 4, pad=0)
    world.recycle(a, a.boundaries()[-3])
    assert f.end < a.wal_start
    return f, a, "wal-gone"


CASES = [fn for name, fn in sorted(globals().items())
         if name.startswith("case_")]


@pytest.mark.parametrize("case", CASES, ids=lambda fn: fn.__name__[5:])
def test_rule(case):
    f, u, want = case()
    assert lineage.expected(f, u) == want, "the model disagrees with the " \
        "case's own label"
    assert handshake(f, u) == want, "\n    f: %s\n    u: %s" % (
        f.describe(), u.describe())
    assert check_rewind(f, u) is None


def test_a_follower_that_sends_no_history_is_judged_as_before():
    """Mixed versions: without ``history`` only the upstream's own
    switch points count, with no window offered nothing is compared."""
    f, u, _ = case_twin_promotion_different_at()
    assert rewind.check_follower(f.timeline, None, f.end, u.timeline,
                                 u.history, u.wal_start, u.end) is None
    assert rewind.handshake_verify({"ok": True}, f.end, f.read)
    f, u, _ = case_wal_past_the_switch()
    assert rewind.check_follower(f.timeline, None, f.end, u.timeline,
                                 u.history, u.wal_start, u.end) == "diverged"


def test_crc_slices_cover_a_range_longer_than_one_slice():
    data = bytes(range(256)) * 1000
    reads = []

    def read(lo, hi):
        reads.append((lo, hi))
        return data[lo:hi]

    assert rewind.range_crc(read, 5, len(data)) == zlib.crc32(data[5:])
    assert len(reads) > 1 and all(hi - lo <= rewind.CRC_CHUNK
                                  for lo, hi in reads)
    assert rewind.range_crc(read, 7, 7) == 0
    with pytest.raises(IOError):
        rewind.range_crc(lambda lo, hi: b"", 0, 10)


# ====================================================================
# Level 1: seeded programs
# ====================================================================
@pytest.fixture(scope="module")
def programs() -> Report:
    return sweep(range(N_PROGRAMS))


def test_programs_reach_every_kind_of_pair_on_the_model_alone():
    """The guard, with the code under test replaced by the model's own
    answers: what the programs reach does not depend on the handshake."""
    rep = sweep(range(N_PROGRAMS), decide=model_says, arithmetic=False)
    assert not rep.unsafe and not rep.spurious
    missing = [kind for kind in MUST_OCCUR if not rep.seen[kind]]
    assert not missing, "never produced: %s (of %d pairs)" % (
        missing, rep.pairs)
    # the model pins all but a sliver of the pairs
    assert rep.blind * 100 < rep.pairs
    print("\n%d pairs, %d blind; " % (rep.pairs, rep.blind) + ", ".join(
        "%s: %d" % (kind, rep.seen[kind]) for kind in MUST_OCCUR))


def test_safety_a_follower_that_is_no_prefix_is_refused(programs):
    assert not programs.unsafe, _show(programs.unsafe)


def test_no_spurious_refusal_and_the_refusal_says_why(programs):
    assert not programs.spurious, _show(programs.spurious)


def test_fork_point_is_at_or_below_the_common_bytes(programs):
    assert not programs.rewind, _show(programs.rewind)


@pytest.mark.gpu
@pytest.mark.parametrize("first", range(300, 3000, 300))
def test_wider_sweep(first):
    rep = sweep(range(first, first + 300))
    assert not rep.unsafe, _show(rep.unsafe)
    assert not rep.spurious, _show(rep.spurious)
    assert not rep.rewind, _show(rep.rewind)


# ====================================================================
# Level 2: real bytes, real handshake
# ====================================================================
IDENT = "5ca1ab1e" * 4
KNOBS = {"wal_segment_bytes": str(SEGMENT_BYTES),
         "checkpoint_wal_bytes": str(1 << 30)}
# the seeded programs whose final pairs are started as servers: with the
# named cases at most MAX_PAIRS pairs in all, so the count bounds the time
LEVEL2_SEEDS = (1, 5, 8)
PAIRS_PER_SEED = 6
MAX_PAIRS = 40


def materialise(peer: Peer, data_dir: str, minipg: bool = False) -> str:
    """The model peer as a stopped database: its records through
    ``Wal.append`` from its WAL start, a checkpoint image at the start
    if WAL below it is gone, and its ident."""
    os.makedirs(data_dir)
    os.chmod(data_dir, 0o700)
    wal = Wal(data_dir, SEGMENT_BYTES)
    wal.open(replay_from=peer.wal_start)
    for r in peer.records[len(peer.records_upto(peer.wal_start)):]:
        wal.append(r)
    wal.fsync()
    assert (wal.start, wal.end) == (peer.wal_start, peer.end)
    wal.close()
    if peer.wal_start:
        with open(os.path.join(data_dir, "checkpoint.json"), "w") as f:
            json.dump({"lsn": peer.wal_start,
                       "kv": peer.kv_at(peer.wal_start)}, f)
    with open(os.path.join(data_dir, "waldb_ident.json"), "w") as f:
        json.dump({"ident": IDENT, "timeline": peer.timeline,
                   "history": peer.history}, f)
    if minipg:
        with open(os.path.join(data_dir, "PG_VERSION"), "w") as f:
            f.write("12\n")
    return data_dir


def lineage_files(data_dir: str) -> dict:
    """The WAL segments and the ident, name → bytes."""
    out = {}
    for name in sorted(os.listdir(data_dir)):
        if name.startswith("wal-") or name == "waldb_ident.json":
            with open(os.path.join(data_dir, name), "rb") as f:
                out[name] = f.read()
    return out


async def _start_waldb(data_dir: str, name: str, upstream_port=None):
    conf = dict(KNOBS, listen_ip="127.0.0.1", port="0", name=name,
                role="standby" if upstream_port else "primary")
    if upstream_port:
        conf["primary_conninfo"] = "'127.0.0.1:%d'" % upstream_port
    confparser.write(os.path.join(data_dir, "waldb.conf"), conf)
    srv = WaldbServer(data_dir, null_logger())
    await srv.start()
    return srv


def _port(srv) -> int:
    return srv._server.sockets[0].getsockname()[1]


def _stop(srv) -> None:
    """No checkpoint, no clean stop (``tests/minipg_inproc.py``); the
    pid file goes, so that the directory reads as stopped."""
    srv._sever_repl()
    for rep in list(srv.replicas):
        srv._abort(rep.writer)
    stop_minipg(srv)
    os.unlink(os.path.join(srv.data_dir, srv.PID_FILE))


async def _until(pred, what: str, timeout: float = 10.0) -> None:
    deadline = asyncio.get_running_loop().time() + timeout
    while not pred():
        assert asyncio.get_running_loop().time() < deadline, \
            "timeout: " + what
        await asyncio.sleep(0.01)


def _is_prefix(f_dir: str, u_dir: str) -> bool:
    f_start, f_buf = wal_bytes(f_dir)
    u_start, u_buf = wal_bytes(u_dir)
    lo = max(f_start, u_start)
    hi = f_start + len(f_buf)
    return hi <= u_start + len(u_buf) and \
        f_buf[lo - f_start:] == u_buf[lo - u_start:hi - u_start]


async def _converges(f_dir: str, usrv, u: Peer, extra: list) -> None:
    """A standby on ``f_dir`` streams from ``usrv``, reaches its end
    after one more write there, holds a prefix of its bytes and serves
    the model's kv at that LSN."""
    fsrv = await _start_waldb(f_dir, "f", _port(usrv))
    try:
        await _until(lambda: fsrv.upstream_status in ("streaming",
                                                      "diverged"),
                     "handshake answered")
        assert fsrv.upstream_status == "streaming"
        op = {"op": "put", "k": "extra", "v": len(extra)}
        assert (await usrv._do_write(op))["ok"]
        extra.append(op)
        await _until(lambda: fsrv.replay_lsn == usrv.wal.end,
                     "follower caught up")
        assert fsrv.wal.end == usrv.wal.end
        fsrv.wal.flush_buffer()
        usrv.wal.flush_buffer()
        assert _is_prefix(f_dir, usrv.data_dir)
        want = u.kv_at(u.end)
        for op in extra:
            want[op["k"]] = op["v"]
        assert fsrv.kv == want
        assert (fsrv.timeline, fsrv.history) == (usrv.timeline,
                                                 usrv.history)
    finally:
        _stop(fsrv)


async def _level2(tmp, f: Peer, u: Peer, minipg: bool = False) -> str:
    """One pair, end to end; returns what happened, for the caller to
    hold against the case's own expectation."""
    want = lineage.expected(f, u)
    assert want != "any"
    f_dir = materialise(f, os.path.join(tmp, "f"))
    u_dir = materialise(u, os.path.join(tmp, "u"), minipg)
    if minipg:
        usrv, _ = await start_minipg(u_dir, KNOBS)
    else:
        usrv = await _start_waldb(u_dir, "u")
    extra = []
    try:
        assert usrv.wal.end == u.end and usrv.kv == u.kv_at(u.end)
        if want is None:
            await _converges(f_dir, usrv, u, extra)
            return "accepted"

        # refused: flagged, and not a byte changed
        before = lineage_files(f_dir)
        fsrv = await _start_waldb(f_dir, "f", _port(usrv))
        try:
            await _until(lambda: fsrv.upstream_status in ("streaming",
                                                          "diverged"),
                         "handshake answered")
            assert fsrv.upstream_status == "diverged"
            assert not usrv.replicas or \
                all(rep.write_lsn == 0 for rep in usrv.replicas), \
                "a refused follower acked"
            assert fsrv.kv == f.kv_at(f.end)
        finally:
            _stop(fsrv)
        assert lineage_files(f_dir) == before

        # a rewind of a copy: a prefix that then streams, or untouched
        copy = os.path.join(tmp, "rewound")
        shutil.copytree(f_dir, copy)
        res = await asyncio.get_running_loop().run_in_executor(
            None, lambda: rewind.rewind_data_dir(
                copy, "127.0.0.1", _port(usrv), null_logger()))
        if res.result == "refused":
            assert lineage_files(copy) == before, res
            return "refused, rewind refused: " + res.reason
        assert res.result in ("ok", "noop")
        assert res.fork_lsn <= lineage.lcp(f, u)
        assert _is_prefix(copy, u_dir)
        await _converges(copy, usrv, u, extra)
        return "refused, rewind " + res.result
    finally:
        for rep in list(usrv.replicas):
            usrv._abort(rep.writer)
        stop_minipg(usrv)


def _run(coro, timeout=30):
    return asyncio.run(asyncio.wait_for(coro, timeout))


def _seeded_pairs():
    """From each seed's final world a fixed, small, mixed handful: the
    pairs are sorted into kinds by what the model says of them (verdict,
    which timeline is higher, equal histories or not) and drawn from
    the kinds in turn."""
    out = []
    for seed in LEVEL2_SEEDS:
        for _step, _what, world in lineage.run_program(seed, N_STEPS):
            pass
        kinds = collections.defaultdict(list)
        for f in world.peers:
            for u in world.peers:
                want = lineage.expected(f, u)
                if f is not u and want != "any":
                    kinds[(str(want), f.history == u.history,
                           (f.timeline > u.timeline)
                           - (f.timeline < u.timeline))].append((f, u))
        picked = []
        while len(picked) < PAIRS_PER_SEED and any(kinds.values()):
            for kind in sorted(kinds):
                if kinds[kind] and len(picked) < PAIRS_PER_SEED:
                    picked.append(kinds[kind].pop(0))
        out += [pytest.param(f, u, id="seed%d-%s-%s" % (seed, f.name,
                                                        u.name))
                for f, u in picked]
    return out


def test_level2_stays_within_its_budget():
    assert len(CASES) + len(_seeded_pairs()) + 2 <= MAX_PAIRS


@pytest.mark.parametrize("case", CASES, ids=lambda fn: fn.__name__[5:])
def test_rule_between_servers(case, tmp_path):
    f, u, want = case()
    outcome = _run(_level2(str(tmp_path), f, u))
    assert outcome.startswith("accepted" if want is None else "refused"), \
        outcome
    if case is case_twin_promotion_same_at:
        # equal histories: the fork point is the shorter end, and only
        # the bytes below it say that it is none
        assert outcome == "refused, rewind refused: history-mismatch"
    if case in (case_wal_past_the_switch, case_twin_promotion_different_at,
                case_follower_ahead):
        assert outcome == "refused, rewind ok"


@pytest.mark.parametrize("f,u", _seeded_pairs())
def test_seeded_pair_between_servers(f, u, tmp_path):
    _run(_level2(str(tmp_path), f, u))


def test_twin_promotion_is_refused_by_a_minipg_upstream(tmp_path):
    """``MinipgServer`` inherits the core: same handshake."""
    f, u, _ = case_twin_promotion_same_at()
    assert _run(_level2(str(tmp_path), f, u, minipg=True)) == \
        "refused, rewind refused: history-mismatch"


def test_twin_promotion_with_the_python_codec(tmp_path, monkeypatch):
    import manatee_amd.native
    monkeypatch.setattr(manatee_amd.native, "codec", None)
    f, u, _ = case_twin_promotion_different_at()
    assert _run(_level2(str(tmp_path), f, u)) == "refused, rewind ok"
