"""An in-process MinipgServer on port 0 for protocol tests (no cluster,
no sync standby), set up as tests/test_waldb_transcript.py does."""

import asyncio
import os

from manatee_amd.common import confparser
from manatee_amd.common.logging import null_logger


def run(coro, timeout=60):
    return asyncio.run(asyncio.wait_for(coro, timeout))


async def start_minipg(data: str, conf: dict = None):
    """Start a primary on ``data`` (initialised on first use); returns
    ``(server, port)``."""
    from manatee_amd.db.minipg.server import MinipgServer, init_data_dir

    if not os.path.exists(os.path.join(data, "PG_VERSION")):
        init_data_dir(data, "12.0")
    settings = {"listen_addresses": "'127.0.0.1'", "port": "0"}
    settings.update(conf or {})
    confparser.write(os.path.join(data, "postgresql.conf"), settings)
    srv = MinipgServer(data, null_logger())
    await srv.start()
    with open(os.path.join(data, "postmaster.pid")) as f:
        port = int(f.read().split()[1])
    return srv, port


def stop_minipg(srv) -> None:
    """Stop WITHOUT a checkpoint: what is on disk afterwards is the WAL
    alone, as after a crash."""
    if srv._server is not None:
        srv._server.close()
    if srv._flusher is not None:
        srv._flusher.cancel()
    srv.wal.close()
