"""Dedicated-box (gpu-marked) tier for the rewind: the divergent
ex-primary scenario of ``test_rewind_cluster`` at a resident size where
a restore is visible, then a plain ``rebuild`` of the same peer on the
same cluster for comparison.

Asserted: the rewind path started no restore and no backup job, and no
acknowledged write was lost.  Recorded, NOT asserted: how long each
rejoin took and how many bytes each moved (both rejoin times are
dominated by session expiry at this tier).  The figures are printed,
and written as JSON to ``$MANATEE_REWIND_PROFILE`` when that is set —
``profiles/rewind_rebuild.json`` is one such run."""

import asyncio
import json
import os
import re
import time

import pytest

from manatee_amd.common import lsn as lsnmod
from tests.rewind_cluster import (adm_rebuild, assert_same_data,
                                  depose_primary, formed,
                                  kill_rebuilt_sitter, metrics, put_acked)

pytestmark = pytest.mark.gpu

RESIDENT, DIVERGENT, VALUE_BYTES = 640, 384, 64 * 1024   # 40 MiB, 24 MiB


def _backup_jobs(c):
    """Backup jobs every peer's backup server has accepted so far."""
    n = 0
    for p in c.peers:
        try:
            with open(os.path.join(p.dir, "backupserver.log.json")) as f:
                n += sum('"backup requested"' in line for line in f)
        except OSError:
            pass
    return n


@pytest.mark.timeout(300)
def test_rewind_against_full_rebuild_of_the_same_peer(tmp_path):
    async def go():
        c = await formed(str(tmp_path / "cluster"), "1.gpurwd",
                         waldb_tunables={"checkpoint_wal_bytes": 1 << 30})
        prim = None
        try:
            prim = await c.wait_writable(timeout_s=60)
            acked = await put_acked(prim, "res", RESIDENT, VALUE_BYTES)
            newp = await depose_primary(c, prim, DIVERGENT, VALUE_BYTES)
            acked.update(await put_acked(newp, "later", 50))
            jobs = _backup_jobs(c)

            t0 = time.monotonic()
            rc, text = await adm_rebuild(c, prim, "--rewind")
            rewind_s = time.monotonic() - t0
            assert rc == 0, text
            m = re.search(r"rewound to the fork point (\S+) "
                          r"\((\d+) bytes cut", text)
            assert m, text
            fork, cut = lsnmod.parse(m.group(1)), int(m.group(2))
            assert cut > 0
            await assert_same_data(newp, prim, acked)
            mt = await metrics(prim)
            assert mt['manatee_rewinds_total{result="ok"}'] == 1
            assert mt["manatee_restores_total"] == 0
            code, body = await prim.http_status("/restore")
            assert body == {"active": False, "done": False}
            assert _backup_jobs(c) == jobs
            assert not os.path.exists(os.path.join(prim.store_dir,
                                                   "isolated"))
            cli = prim.db_client()
            streamed = lsnmod.parse(
                (await cli.status())["current_lsn"]) - fork
            await cli.close()

            # the same peer again, the classic way
            kill_rebuilt_sitter(prim)
            t0 = time.monotonic()
            rc, text = await adm_rebuild(c, prim)
            rebuild_s = time.monotonic() - t0
            assert rc == 0, text
            await assert_same_data(newp, prim, acked)
            assert _backup_jobs(c) == jobs + 1
            code, restore = await prim.http_status("/restore")
            assert restore.get("done") and not restore.get("failed")

            report = {
                "resident_value_bytes": RESIDENT * VALUE_BYTES,
                "divergent_value_bytes": DIVERGENT * VALUE_BYTES,
                "rewind": {"rejoin_s": round(rewind_s, 2),
                           "wal_bytes_cut": cut,
                           "wal_bytes_streamed": streamed},
                "rebuild": {"rejoin_s": round(rebuild_s, 2),
                            "restore_bytes": restore.get("completed")},
                "note": "recorded, not asserted; one run",
            }
            print("rewind vs rebuild: %s" % json.dumps(report))
            out = os.environ.get("MANATEE_REWIND_PROFILE")
            if out:
                with open(out, "w") as f:
                    json.dump(report, f, indent=2)
                    f.write("\n")
        finally:
            if prim is not None:
                kill_rebuilt_sitter(prim)
            c.stop()
    asyncio.run(asyncio.wait_for(go(), 290))
