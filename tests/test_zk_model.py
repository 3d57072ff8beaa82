"""Both coordination servers against a plain model of the data tree.

``tests/zkmodel.py`` states the rules of create / delete / setData /
check / multi / session close once, in a dictionary.  Here seeded random
programs over a deliberately tiny namespace (so that collisions are the
norm) run on the model, on the standalone ``ZkServer`` and on the
replicated ``ZkQuorumServer``, without sockets or an event loop, and
after EVERY step the outcome and the whole tree must agree.  The same
programs then check that a quorum follower (log replay) and a restored
member (snapshot) are identical to the leader, and that the standalone
journal replays to the model's persistent tree.

A failing program prints its seed and its steps; ``run_program`` replays
any step list.
"""

import functools
import json
import pprint
import random

import pytest

from manatee_amd.coord import jute
from manatee_amd.coord.jute import MultiOp, ZkError
from manatee_amd.coord.quorum import QuorumCore
from manatee_amd.coord.zkquorum import ZkQuorumServer
from manatee_amd.coord.zkserver import ZkServer, _Session
from tests import zkmodel
from tests.zkmodel import ModelError, ZkModel

N_PROGRAMS = 300
N_STEPS = 40
FIXED_TIME_MS = 1700000000000

# two names per level, depth <= 3, the root, one relative path and one
# with a trailing slash
NAMES = ("a", "b")


def _name_space():
    paths, level = ["/"], [""]
    for _ in range(3):
        level = ["%s/%s" % (p, n) for p in level for n in NAMES]
        paths += level
    return paths + ["a/b", "/a/"]


SPACE = _name_space()
DATA = (b"", b"x", b"yy", b"zzz")


# ====================================================================
# programs
# ====================================================================
# A program is a list of concrete steps:
#   ("open", sid) | ("close", sid)
#   ("create", sid, path, data, flags)
#   ("delete", sid, path, version)
#   ("setData", sid, path, data, version)
#   ("multi", sid, [op, ...])       ops as ZkModel.multi takes them

def _pick_path(rng, nodes, touched):
    r = rng.random()
    if touched and r < 0.5:
        base = rng.choice(touched)
        k = rng.random()
        if k < 0.5:
            return base
        if k < 0.75:
            return zkmodel.parent_of(base) if base.startswith("/") else base
        return "%s/%s" % ("" if base == "/" else base, rng.choice(NAMES))
    if r < 0.7:
        return rng.choice(sorted(nodes))
    return rng.choice(SPACE)


def _pick_version(rng, nodes, path):
    node = nodes.get(path)
    current = node.version if node is not None else 0
    return rng.choice((-1, -1, current, current, current, current + 1,
                       current - 1))


def _pick_op(rng, nodes, touched, in_multi):
    path = _pick_path(rng, nodes, touched)
    r = rng.random()
    if r < 0.45:
        return ("create", path, rng.choice(DATA), rng.choice(zkmodel.FLAGS))
    if r < 0.70:
        return ("delete", path, _pick_version(rng, nodes, path))
    if r < 0.90 or not in_multi:
        return ("setData", path, rng.choice(DATA),
                _pick_version(rng, nodes, path))
    return ("check", path, _pick_version(rng, nodes, path))


def _apply_single(model, sid, op):
    if op[0] == "create":
        return model.create(op[1], op[2], op[3], sid)
    if op[0] == "delete":
        return model.delete(op[1], op[2])
    if op[0] == "setData":
        return model.set_data(op[1], op[2], op[3])
    model._check(model.nodes, op[1], op[2])


def _gen_multi(rng, model, sid):
    """2-5 ops, each drawn against what the earlier ones left behind, so
    that later ops often name paths the earlier ones touched."""
    scratch = ZkModel()
    scratch.nodes = {p: n.copy() for p, n in model.nodes.items()}
    scratch.sessions = set(model.sessions)
    ops, touched = [], []
    for _ in range(rng.randint(2, 5)):
        for attempt in range(2):
            op = _pick_op(rng, scratch.nodes, touched, True)
            trial = ZkModel()
            trial.nodes = {p: n.copy() for p, n in scratch.nodes.items()}
            trial.sessions = scratch.sessions
            try:
                _apply_single(trial, sid, op)
                break
            except ModelError:
                # keep about half of the ops that fail
                if rng.random() < 0.5:
                    break
        try:
            made = _apply_single(scratch, sid, op)
        except ModelError:
            made = None
        ops.append(op)
        touched.append(made if op[0] == "create" and made else op[1])
    return ops


@functools.lru_cache(maxsize=None)
def gen_program(seed, dead_sessions):
    """Returns (steps, counts): the program and how often the model fired
    each rule while running it.  With ``dead_sessions`` requests also
    come from sessions that were closed."""
    rng = random.Random(seed * 2 + int(dead_sessions))
    model = ZkModel()
    steps = []
    slots = [None, None]            # [sid, live]
    next_sid = [0x100]

    def open_slot(i):
        sid = next_sid[0]
        next_sid[0] += 1
        slots[i] = [sid, True]
        model.open_session(sid)
        steps.append(("open", sid))

    open_slot(0)
    open_slot(1)
    while len(steps) < N_STEPS + 2:
        r = rng.random()
        if r < 0.08:
            i = rng.randrange(2)
            if slots[i][1]:
                slots[i][1] = False
                model.close_session(slots[i][0])
                steps.append(("close", slots[i][0]))
            else:
                open_slot(i)
            continue
        usable = [s for s in slots if s[1] or dead_sessions]
        if not usable:
            open_slot(rng.randrange(2))
            continue
        sid = rng.choice(usable)[0]
        if r < 0.08 + 0.31:
            ops = _gen_multi(rng, model, sid)
            steps.append(("multi", sid, ops))
            try:
                model.multi(ops, sid)
            except ModelError:
                pass
        else:
            op = _pick_op(rng, model.nodes, [], False)
            steps.append((op[0], sid) + op[1:])
            try:
                _apply_single(model, sid, op)
            except ModelError:
                pass
    return tuple(steps), model.counts


# ====================================================================
# adapters: the real servers, driven without sockets
# ====================================================================

def _multi_ops(ops):
    out = []
    for op in ops:
        if op[0] == "create":
            out.append(MultiOp.create(op[1], op[2], op[3]))
        elif op[0] == "delete":
            out.append(MultiOp.delete(op[1], op[2]))
        elif op[0] == "setData":
            out.append(MultiOp.set_data(op[1], op[2], op[3]))
        else:
            out.append(MultiOp.check(op[1], op[2]))
    return out


def _multi_results(results):
    out = []
    for res in results:
        if res[0] == "setData":
            out.append(("setData", res[1].version, res[1].dataLength))
        else:
            out.append(tuple(res))
    return out


class Standalone:
    name = "standalone"

    def __init__(self, tmp_path, journal=False):
        self.srv = ZkServer()
        self.journal_path = None
        if journal:
            self.journal_path = str(tmp_path / "journal.jsonl")
            self.srv.journal_path = self.journal_path
            self.srv._journal = open(self.journal_path, "a", buffering=1)

    def close(self):
        if self.srv._journal is not None:
            self.srv._journal.close()
            self.srv._journal = None

    def consumed(self):
        """Everything a failed request must leave alone besides the tree."""
        return (self.srv.zxid, self.srv._journal_entries)

    def open_session(self, sid):
        self.srv.sessions[sid] = _Session(sid, b"\x00" * 16, 30000)

    def close_session(self, sid):
        self.srv._expire_session(self.srv.sessions[sid])

    def create(self, sid, path, data, flags):
        return self.srv._do_create(path, data, flags, sid)

    def delete(self, sid, path, version):
        self.srv._do_delete(path, version)

    def set_data(self, sid, path, data, version):
        st = self.srv._do_set_data(path, data, version)
        return st.version, st.dataLength

    def multi(self, sid, ops):
        return _multi_results(self.srv._do_multi(_multi_ops(ops), sid))


def _quorum_member(tmp_path, name):
    """A member that is never started: no sockets, no disk, an empty
    tree as start() leaves it."""
    srv = ZkQuorumServer(1, peers={1: ("127.0.0.1", 1)},
                         data_dir=str(tmp_path / name))
    srv.core = QuorumCore(1, [1], random.Random(0), 0.0)
    srv._restore(None)
    return srv


class Quorum:
    name = "quorum"

    def __init__(self, tmp_path):
        self.tmp_path = tmp_path
        self.srv = _quorum_member(tmp_path, "leader")
        self.log = []

    def close(self):
        pass

    def consumed(self):
        return (self.srv.zxid, self.srv._last_zxid_assigned, len(self.log))

    def _submit(self, prepare):
        """What ZkQuorumServer._submit does around the consensus round:
        draw a zxid, validate into a txn (rolling the zxid back when
        validation refuses), log, apply."""
        srv = self.srv
        assigned = srv._last_zxid_assigned
        try:
            txn = prepare(srv._next_zxid(), FIXED_TIME_MS)
        except ZkError:
            srv._last_zxid_assigned = assigned
            raise
        # the log is JSON on disk and on the wire
        txn = json.loads(json.dumps(txn))
        self.log.append(txn)
        return srv._apply_txn(txn)

    def open_session(self, sid):
        self._submit(lambda zxid, _now: {
            "op": "session_open", "zxid": zxid, "sid": sid,
            "passwd": "00" * 16, "timeout": 30000})

    def close_session(self, sid):
        self._submit(lambda zxid, _now: {
            "op": "session_close", "zxid": zxid, "sid": sid})

    def create(self, sid, path, data, flags):
        def prep(zxid, now_ms):
            txn = self.srv._prep_create(path, data, flags, sid)
            txn.update(zxid=zxid, time=now_ms)
            return txn
        return self._submit(prep)

    def delete(self, sid, path, version):
        def prep(zxid, _now):
            txn = self.srv._prep_versioned("delete", path, version)
            txn["zxid"] = zxid
            return txn
        self._submit(prep)

    def set_data(self, sid, path, data, version):
        def prep(zxid, now_ms):
            txn = self.srv._prep_versioned("setData", path, version, data)
            txn.update(zxid=zxid, time=now_ms)
            return txn
        st = self._submit(prep)
        return st.version, st.dataLength

    def multi(self, sid, ops):
        mops = _multi_ops(ops)

        def prep(zxid, now_ms):
            return {"op": "multi", "zxid": zxid, "time": now_ms,
                    "ops": self.srv._prep_multi(mops, sid)}
        return _multi_results(self._submit(prep))

    # ---------------------------------------------------- replica identity
    def assert_replicas_identical(self):
        follower = _quorum_member(self.tmp_path, "follower")
        for txn in self.log:
            follower._apply_txn(txn)        # no _prep_*: the follower path
        restored = _quorum_member(self.tmp_path, "restored")
        restored._restore(json.loads(json.dumps(self.srv._make_snapshot())))
        lead = self.srv.dump_full()
        assert follower.dump_full() == lead, "log replay diverged"
        assert restored.dump_full() == lead, "snapshot restore diverged"


# ====================================================================
# the comparison
# ====================================================================

def server_tree(srv):
    return {p: {"data": n.data, "version": n.version,
                "cversion": n.cversion, "children": sorted(n.children),
                "owner": n.ephemeral_owner, "next_seq": n.next_seq}
            for p, n in srv.nodes.items()}


def _model_step(model, step):
    kind = step[0]
    try:
        if kind == "open":
            return ("ok", model.open_session(step[1]))
        if kind == "close":
            return ("ok", model.close_session(step[1]))
        if kind == "multi":
            return ("ok", model.multi(step[2], step[1]))
        return ("ok", _apply_single(model, step[1], (kind,) + step[2:]))
    except ModelError as exc:
        return ("err", exc.code)


def _server_step(adapter, step):
    kind = step[0]
    try:
        if kind == "open":
            return ("ok", adapter.open_session(step[1]))
        if kind == "close":
            return ("ok", adapter.close_session(step[1]))
        if kind == "multi":
            return ("ok", adapter.multi(step[1], step[2]))
        if kind == "create":
            return ("ok", adapter.create(*step[1:]))
        if kind == "delete":
            return ("ok", adapter.delete(*step[1:]))
        return ("ok", adapter.set_data(*step[1:]))
    except ZkError as exc:
        return ("err", exc.code)


def _assert_same_tree(adapter, want):
    tree = server_tree(adapter.srv)
    for path in sorted(set(tree) | set(want)):
        assert tree.get(path) == want.get(path), \
            "%s has %s = %r, expected %r" % (
                adapter.name, path, tree.get(path), want.get(path))
    return want


def _describe(outcome):
    if outcome[0] == "err":
        return "error %s" % jute.ERROR_NAMES.get(outcome[1], outcome[1])
    return "ok %r" % (outcome[1],)


def run_program(steps, adapter, label="", model=None):
    """Run ``steps`` on the model (a fresh one by default) and on
    ``adapter``, comparing after every step.  Returns the model and the
    list of outcomes."""
    model = model or ZkModel()
    srv = adapter.srv
    outcomes = []
    i = -1
    try:
        for i, step in enumerate(steps):
            before = model.tree()
            consumed = adapter.consumed()
            zxid = srv.zxid
            want = _model_step(model, step)
            got = _server_step(adapter, step)
            assert got == want, "%s answered %s, the model says %s" % (
                adapter.name, _describe(got), _describe(want))
            mtree = _assert_same_tree(adapter, model.tree())
            assert {sid: sorted(s.ephemerals)
                    for sid, s in srv.sessions.items()} == \
                {sid: sorted(p for p, n in model.nodes.items()
                             if n.owner == sid)
                 for sid in model.sessions}, "sessions' ephemerals"
            # zxids: nothing absolute, the servers number differently
            for path, n in srv.nodes.items():
                assert n.stat_czxid <= n.stat_mzxid, path
                assert n.pzxid >= n.stat_czxid, path
            if want[0] == "err":
                assert adapter.consumed() == consumed, \
                    "a failed request consumed (zxid, ...): %r -> %r" % (
                        consumed, adapter.consumed())
            elif mtree != before:
                assert srv.zxid > zxid, "a write did not advance the zxid"
            else:
                assert srv.zxid >= zxid
            outcomes.append(want)
    except AssertionError as exc:
        raise AssertionError(
            "%s %s, step %d: %s\nprogram up to there:\n%s" % (
                adapter.name, label, i, exc,
                pprint.pformat(list(steps[:i + 1])))) from None
    return model, outcomes


# ====================================================================
# tests
# ====================================================================

def _required_counts():
    keys = []
    for ctx in ("single", "multi"):
        keys += [(ctx, "create", c) for c in (
            jute.ZAPIERROR, jute.ZNONODE, jute.ZNOCHILDRENFOREPHEMERALS,
            jute.ZNODEEXISTS, jute.ZSESSIONEXPIRED)]
        keys += [(ctx, "delete", c) for c in (
            jute.ZBADARGUMENTS, jute.ZNONODE, jute.ZNOTEMPTY,
            jute.ZBADVERSION)]
        keys += [(ctx, "setData", c) for c in (jute.ZNONODE,
                                               jute.ZBADVERSION)]
    keys += [("multi", "check", c) for c in (jute.ZNONODE, jute.ZBADVERSION)]
    keys += [zkmodel.PARENT_MADE_IN_MULTI, zkmodel.DELETE_THEN_RECREATE]
    return keys


def test_programs_reach_every_rule():
    """The model alone: over the programs below, every error of the rule
    list fires, as a single request and inside a multi, and so do the two
    successful multi shapes the standalone server used to refuse."""
    total = {}
    for seed in range(N_PROGRAMS):
        for dead in (False, True):
            _steps, counts = gen_program(seed, dead)
            for k, v in counts.items():
                total[k] = total.get(k, 0) + v
    report = {k: total.get(k, 0) for k in _required_counts()}
    print(pprint.pformat(report))
    missing = [k for k, v in report.items() if not v]
    assert not missing, missing
    # the standalone server is never sent a dead session
    alive = {}
    for seed in range(N_PROGRAMS):
        for k, v in gen_program(seed, False)[1].items():
            alive[k] = alive.get(k, 0) + v
    assert not [k for k in alive if isinstance(k, tuple)
                and k[2] == jute.ZSESSIONEXPIRED]
    missing = [k for k in _required_counts() if not alive.get(k)
               and not (isinstance(k, tuple)
                        and k[2] == jute.ZSESSIONEXPIRED)]
    assert not missing, missing


def test_standalone_matches_model(tmp_path):
    for seed in range(N_PROGRAMS):
        steps, _ = gen_program(seed, False)
        journaled = seed % 10 == 0
        d = tmp_path / ("s%d" % seed)
        d.mkdir()
        adapter = Standalone(d, journal=journaled)
        try:
            model, _ = run_program(steps, adapter, "seed=%d" % seed)
        finally:
            adapter.close()
        if journaled:
            _assert_journal_replays(adapter.journal_path, model,
                                    "seed=%d" % seed)


def _assert_journal_replays(journal_path, model, label):
    fresh = ZkServer(journal_path=journal_path)
    fresh._replay_journal()
    got = {p: (n.data, sorted(n.children)) for p, n in fresh.nodes.items()}
    assert got == model.persistent(), \
        "journal replay differs from the model's persistent tree, %s" % label


def test_quorum_matches_model_and_replicas_are_identical(tmp_path):
    for seed in range(N_PROGRAMS):
        steps, _ = gen_program(seed, True)
        adapter = Quorum(tmp_path / ("q%d" % seed))
        run_program(steps, adapter, "seed=%d" % seed)
        try:
            adapter.assert_replicas_identical()
        except AssertionError as exc:
            raise AssertionError("quorum seed=%d: %s\nprogram:\n%s" % (
                seed, exc, pprint.pformat(list(steps)))) from None


# ------------------------------------------------------------ named cases
S = 0x100
_X = [("open", S), ("create", S, "/x", b"0", 0)]
_P = [("open", S), ("create", S, "/p", b"", 0)]

NAMED = {
    # a failing multi must leave nothing behind ...
    "partial_setdata_twice_at_one_version": (
        _X, ("multi", S, [("setData", "/x", b"1", 0),
                          ("setData", "/x", b"2", 0)]),
        ("err", jute.ZBADVERSION)),
    "partial_create_twice": (
        [("open", S)], ("multi", S, [("create", "/a", b"", 0),
                                     ("create", "/a", b"", 0)]),
        ("err", jute.ZNODEEXISTS)),
    "partial_delete_then_setdata": (
        _X, ("multi", S, [("delete", "/x", -1),
                          ("setData", "/x", b"1", -1)]),
        ("err", jute.ZNONODE)),
    "partial_create_child_then_delete_parent": (
        _P, ("multi", S, [("create", "/p/c", b"", 0),
                          ("delete", "/p", -1)]),
        ("err", jute.ZNOTEMPTY)),
    # ... and a legal one must be accepted
    "refused_create_parent_then_child": (
        [("open", S)], ("multi", S, [("create", "/p", b"", 0),
                                     ("create", "/p/c", b"", 0)]),
        ("ok", [("create", "/p"), ("create", "/p/c")])),
    "refused_delete_then_recreate": (
        _X, ("multi", S, [("delete", "/x", 0),
                          ("create", "/x", b"new", 0)]),
        ("ok", [("delete",), ("create", "/x")])),
    # the root is not deletable
    "delete_root": (
        [("open", S)], ("delete", S, "/", -1), ("err", jute.ZBADARGUMENTS)),
    "delete_root_in_multi": (
        [("open", S)], ("multi", S, [("delete", "/", -1)]),
        ("err", jute.ZBADARGUMENTS)),
}


def _adapter(kind, tmp_path):
    return Standalone(tmp_path, journal=True) if kind == "standalone" \
        else Quorum(tmp_path)


@pytest.mark.parametrize("kind", ["standalone", "quorum"])
@pytest.mark.parametrize("case", sorted(NAMED))
def test_named_case(case, kind, tmp_path):
    setup, step, expected = NAMED[case]
    adapter = _adapter(kind, tmp_path)
    srv = adapter.srv
    try:
        # a watcher on everything the step names: a failed request fires
        # nothing, so the watches must still be armed afterwards
        watcher = 0x999
        adapter.open_session(watcher)
        model = ZkModel()
        model.open_session(watcher)
        run_program(setup, adapter, case, model)
        paths = {"/"} | ({op[1] for op in step[2]} if step[0] == "multi"
                         else {step[2]})
        for p in paths:
            srv.data_watches[p] = {watcher}
            srv.child_watches[p] = {watcher}
        armed = ({p: set(s) for p, s in srv.data_watches.items()},
                 {p: set(s) for p, s in srv.child_watches.items()})
        before = server_tree(srv)
        journal = srv._journal_entries

        want = _model_step(model, step)
        assert want == expected, "the model itself: %s" % _describe(want)
        got = _server_step(adapter, step)
        assert got == expected, "%s answered %s, expected %s" % (
            kind, _describe(got), _describe(expected))
        _assert_same_tree(adapter, model.tree())
        if expected[0] == "err":
            _assert_same_tree(adapter, before)
            assert (srv.data_watches, srv.child_watches) == armed, \
                "a failed request fired a watch"
            assert srv._journal_entries == journal, \
                "a failed request wrote to the journal"
        # the tree still works afterwards
        after = ("create", S, "/after", b"", 0)
        assert _server_step(adapter, after) == _model_step(model, after) \
            == ("ok", "/after")
    finally:
        adapter.close()
    if kind == "standalone":
        _assert_journal_replays(adapter.journal_path, model, case)
    else:
        adapter.assert_replicas_identical()
