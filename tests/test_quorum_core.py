"""The consensus core (coord/quorum.py) and its simulator — no sockets,
no files, no clock: directed cases on hand-driven cores and on a
fault-free simulator, then a seeded sweep with drops, partitions and
crash-restarts under which every invariant must hold."""

import random

from manatee_amd.coord.quorum import (CANDIDATE, FOLLOWER, LEADER,
                                      QuorumCore)
from manatee_amd.coord.quorumsim import QuorumSim, run_seed

EL = (0.3, 0.6)


def _core(node=1, now=0.0, **kw):
    return QuorumCore(node, [1, 2, 3], random.Random(node), now,
                      election_timeout=EL, heartbeat=0.05, **kw)


def _sends(effects, t=None):
    return [e[2] for e in effects
            if e[0] == "send" and (t is None or e[2]["t"] == t)]


def _vote_req(frm, epoch, last_index, last_epoch):
    return {"t": "vote_req", "from": frm, "epoch": epoch,
            "last_index": last_index, "last_epoch": last_epoch}


def _steady_sim(seed=1, **kw):
    sim = QuorumSim(seed, **kw)
    sim.run_until(5.0, stop=lambda: sim.leader() is not None)
    assert sim.leader() is not None
    return sim


def _commit(sim, payloads):
    for p in payloads:
        lead = sim.leader()
        idx = sim.propose(lead, p)
        assert idx is not None
        sim.run_until(sim.now + 2.0, stop=lambda: idx in sim.acked)
        assert sim.acked[idx][1] == p


# ------------------------------------------------------------- directed
def test_shorter_or_older_log_cannot_win():
    log = [(1, "a"), (2, "b")]
    # long after any leader was heard, so the request is considered
    now = 10.0
    for last_index, last_epoch, want in (
            (1, 2, False),      # same last epoch, shorter
            (5, 1, False),      # longer, but its last entry is older
            (2, 2, True),       # as up to date
            (1, 3, True)):      # newer last epoch beats length
        core = _core(epoch=2, log=log)
        core.handle(_vote_req(2, 3, last_index, last_epoch), now)
        eff = core.drain()
        (resp,) = _sends(eff, "vote_resp")
        assert resp["granted"] is want, (last_index, last_epoch)
        # the epoch is adopted either way, and a granted vote is
        # persisted BEFORE the reply leaves
        kinds = [e[0] for e in eff]
        assert ("meta", 3, 2 if want else None) in eff
        assert kinds.index("meta") < kinds.index("send")

    # end to end: the member that missed committed writes never leads
    sim = _steady_sim()
    lead = sim.leader()
    behind = [m for m in sim.members if m != lead][0]
    sim.isolate(behind)
    _commit(sim, [{"w": k} for k in range(3)])
    sim.run_for(2.0)          # the isolated member campaigns, epoch after epoch
    assert sim.core(behind).epoch > sim.core(lead).epoch
    n_before = len(sim.leader_history)
    last_acked = max(sim.acked)
    assert sim.core(behind).last_index < last_acked
    sim.heal()
    # for as long as its log lacks an acknowledged write it is never a
    # leader, in any epoch — however high its own epoch has climbed
    t_end = sim.now + 5.0
    while sim.core(behind).last_index < last_acked:
        assert sim.now < t_end, "the stale member never caught up"
        sim.run_for(0.002)
        assert sim.core(behind).role != LEADER
        assert all(m != behind for _e, m in sim.leader_history[n_before:])
    # its campaigning did depose the old leader's epoch: somebody with a
    # complete log leads the new one
    sim.run_until(sim.now + 3.0, stop=lambda: sim.leader() is not None
                  and sim.core(sim.leader()).epoch
                  >= sim.core(behind).epoch)
    assert sim.leader() is not None
    assert sim.core(sim.leader()).epoch >= sim.core(behind).epoch
    sim.run_for(0.5)
    assert sim.core(behind).last_index == sim.core(sim.leader()).last_index


def test_deposed_leaders_uncommitted_entry_is_overwritten():
    sim = _steady_sim()
    old = sim.leader()
    _commit(sim, [{"w": "kept"}])
    sim.isolate(old)
    idx = sim.propose(old, {"w": "doomed"})     # lease still valid: taken
    assert idx is not None
    assert sim.core(old).entry_at(idx)[1] == {"w": "doomed"}
    sim.run_until(sim.now + 5.0,
                  stop=lambda: sim.leader() not in (None, old))
    new = sim.leader()
    assert new not in (None, old)
    _commit(sim, [{"w": "fresh"}])
    sim.heal()
    sim.run_for(2.0)
    assert sim.core(old).role == FOLLOWER
    assert sim.core(old).entry_at(idx) == sim.core(new).entry_at(idx)
    assert sim.core(old).entry_at(idx)[1] != {"w": "doomed"}
    assert all(p != {"w": "doomed"} for _e, p in sim.applied.values())
    assert {"w": "doomed"} in sim.failed
    assert idx not in sim.acked or sim.acked[idx][1] != {"w": "doomed"}
    assert sim.members[old].applied == sim.members[new].applied


def test_old_epoch_entry_commits_only_with_a_current_epoch_entry():
    # member 1 restarts holding an epoch-2 entry nobody committed
    core = _core(epoch=2, voted_for=1, log=[(1, None), (2, "x")])
    core.tick(10.0)                              # election timeout
    assert core.role == CANDIDATE and core.epoch == 3
    core.drain()
    core.handle({"t": "vote_resp", "from": 2, "epoch": 3,
                 "granted": True}, 10.01)
    eff = core.drain()
    assert core.role == LEADER
    assert ("append", 3, [(3, None)]) in eff     # the no-op of its epoch
    # the old-epoch entry reaches a majority — the no-op has not yet
    core.handle({"t": "append_resp", "from": 2, "epoch": 3, "ok": True,
                 "match": 2, "ts": 10.01}, 10.02)
    eff = core.drain()
    assert core.commit_index == 0
    assert not [e for e in eff if e[0] in ("apply", "serving")]
    assert core.propose("y", 10.02) is None      # not serving yet
    # ...now it has: everything commits together, in order
    core.handle({"t": "append_resp", "from": 2, "epoch": 3, "ok": True,
                 "match": 3, "ts": 10.02}, 10.03)
    eff = core.drain()
    assert [e[1:] for e in eff if e[0] == "apply"] == [
        (1, 1, None), (2, 2, "x"), (3, 3, None)]
    assert ("serving", 3) in eff
    assert core.propose("y", 10.03) == 4


def test_restarted_member_refuses_a_second_vote_in_the_same_epoch():
    core = _core(epoch=4)
    core.handle(_vote_req(2, 5, 0, 0), 10.0)
    eff = core.drain()
    assert ("meta", 5, 2) in eff
    assert _sends(eff, "vote_resp")[0]["granted"] is True
    # kill -9; what was persisted is all that comes back
    core = _core(now=20.0, epoch=5, voted_for=2)
    core.handle(_vote_req(3, 5, 7, 4), 30.0)     # a far better log: still no
    (resp,) = _sends(core.drain(), "vote_resp")
    assert resp["granted"] is False
    assert core.voted_for == 2
    core.handle(_vote_req(2, 5, 0, 0), 30.0)     # the same candidate again
    (resp,) = _sends(core.drain(), "vote_resp")
    assert resp["granted"] is True


def test_vote_requests_are_ignored_while_a_leader_is_heard():
    core = _core(epoch=1)
    core.handle({"t": "append", "from": 2, "epoch": 1, "prev_index": 0,
                 "prev_epoch": 0, "entries": [], "commit": 0, "ts": 5.0},
                5.0)
    core.drain()
    core.handle(_vote_req(3, 9, 99, 9), 5.0 + EL[0] - 0.01)
    assert core.drain() == [] and core.epoch == 1
    core.handle(_vote_req(3, 9, 99, 9), 5.0 + EL[0] + 0.001)
    assert _sends(core.drain(), "vote_resp")[0]["granted"] is True


def test_member_behind_truncation_is_caught_up_by_snapshot_then_log():
    sim = _steady_sim(snapshot_entries=5)
    lead = sim.leader()
    lagger = [m for m in sim.members if m != lead][0]
    sim.crash(lagger)
    _commit(sim, [{"w": k} for k in range(20)])
    assert sim.core(lead).base_index > sim.members[lagger].store.base_index \
        + len(sim.members[lagger].store.log)
    sim.restart(lagger)
    sim.run_for(2.0)
    assert sim.stats["snapshots_installed"] == 1
    snap_at = sim.core(lagger).base_index
    assert snap_at > 0
    _commit(sim, [{"w": "after-%d" % k} for k in range(3)])
    sim.run_for(0.5)
    top = sim.members[sim.leader()].applied
    assert sim.members[lagger].applied == top > snap_at
    assert sim.members[lagger].digest == sim.members[sim.leader()].digest
    assert sim.stats["snapshots_installed"] == 1     # the rest came by log


def test_cut_off_leader_stops_accepting_within_min_election_timeout():
    sim = _steady_sim(election_timeout=EL, heartbeat=0.05)
    lead = sim.leader()
    _commit(sim, [{"w": 0}])
    sim.isolate(lead)
    t_cut = sim.now
    taken = []
    refused_at = None
    while sim.now < t_cut + 2 * EL[0]:
        idx = sim.propose(lead, {"w": "late-%d" % len(taken)})
        if idx is None:
            refused_at = sim.now
            break
        taken.append(idx)
        sim.run_for(0.002)
    assert refused_at is not None
    assert refused_at - t_cut <= EL[0]
    sim.run_until(t_cut + EL[0] + sim.tick_s)
    assert sim.core(lead).role != LEADER
    assert sim.propose(lead, {"w": "later"}) is None
    # nothing it took while cut off was ever acknowledged
    acked_payloads = [p for _e, p in sim.acked.values()]
    assert not [p for p in acked_payloads
                if p is not None and str(p["w"]).startswith("late")]
    assert len(sim.failed) == len(taken)


# ----------------------------------------------------------- seed sweep
N_SEEDS = 40        # ~0.15 s each: 8 simulated seconds of chaos + settling


def test_seed_sweep_invariants_hold_under_faults():
    """Drops, partitions and crash-restarts, aimed at the leader more
    often than not; run_seed raises InvariantViolation on the first
    breach.  Not vacuous: every seed commits client writes and at least
    half the seeds see two or more distinct members lead."""
    rows = [run_seed(seed, seconds=8.0) for seed in range(N_SEEDS)]
    for r in rows:
        assert r["acked"] >= 1, r
        assert r["crashes"] + r["partitions"] >= 1, r
    multi = [r for r in rows if r["distinct_leader_members"] >= 2]
    assert 2 * len(multi) >= N_SEEDS, len(multi)
    assert sum(r["dropped"] for r in rows) > 0
    assert any(r["snapshots_installed"] for r in rows)
    assert any(r["failed"] for r in rows)


def test_simulator_cli_replays_a_seed(capsys):
    import json

    from manatee_amd.coord import quorumsim
    assert quorumsim.main(["--seed", "3", "--seconds", "3"]) == 0
    first = json.loads(capsys.readouterr().out.splitlines()[-1])
    assert first["ok"] and first["seed"] == 3 and first["acked"] >= 1
    assert quorumsim.main(["--seed", "3", "--seconds", "3"]) == 0
    assert json.loads(capsys.readouterr().out.splitlines()[-1]) == first


def test_snapshot_never_discards_a_matching_log_suffix():
    """A snapshot that arrives at a member already holding its last
    entry (late, reordered, or to a member whose commit index fell back
    on restart) must keep the durable log: entries beyond the snapshot
    may be acknowledged and counted toward a majority."""
    log = [(1, "e%d" % k) for k in range(1, 11)]
    core = _core(epoch=1, log=log)              # restarted: commit 0
    core.handle({"t": "snap", "from": 2, "epoch": 1, "last_index": 5,
                 "last_epoch": 1, "data": {"any": "thing"}, "ts": 1.0}, 1.0)
    eff = core.drain()
    assert core.last_index == 10 and core.base_index == 0
    assert not [e for e in eff if e[0] in ("snapshot", "append")]
    assert [e[1] for e in eff if e[0] == "apply"] == [1, 2, 3, 4, 5]
    (ack,) = _sends(eff, "append_resp")
    assert ack["ok"] and ack["match"] == 5
    # a snapshot whose last entry this member does NOT hold (another
    # epoch at that index) still replaces everything
    core = _core(epoch=1, log=log)
    core.handle({"t": "snap", "from": 2, "epoch": 3, "last_index": 5,
                 "last_epoch": 2, "data": {"any": "thing"}, "ts": 1.0}, 1.0)
    eff = core.drain()
    assert ("snapshot", 5, 2, {"any": "thing"}) in eff
    assert core.last_index == 5 and core.base_index == 5
