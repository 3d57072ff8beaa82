"""Dedicated-box tier: the transactional (tpcb) write load of
``tools/wrbench`` against a 3-peer engine=postgres shard.  No
throughput is asserted — the run's own invariant check (balances,
history rows, sequence stamps, on the primary and on the sync standby)
is what must hold, at 1 and at 8 writers.
"""

import asyncio

import pytest

from manatee_amd.tools import wrbench

pytestmark = pytest.mark.gpu


def test_wrbench_tpcb_invariants(tmp_path):
    out = asyncio.run(asyncio.wait_for(
        wrbench.run([1, 8], 3.0, str(tmp_path / "wrbench"),
                    engine="postgres", profile="tpcb"), 300))
    assert out["engine"] == "postgres" and out["profile"] == "tpcb"
    assert [r["writers"] for r in out["results"]] == [1, 8]
    for r in out["results"]:
        assert r["invariants_ok"] is True
        assert r["accounts"] == r["writers"] * wrbench.TPCB_ACCOUNTS
        assert r["txns_per_s"] > 0
        # every acknowledged transaction left its history row
        assert r["history_rows"] >= r["txns_per_s"] * 3.0 * 0.99
    assert out["total_keys"] == sum(r["accounts"] + r["history_rows"]
                                    for r in out["results"])

