"""The standalone coordination server's opt-in disconnect grace.

A session whose CLIENT closed the connection (FIN or RST) and did not
re-attach within ``disconnect_grace_ms`` is expired then; silence, a
connection this server dropped itself, and the default configuration all
keep the full session timeout.

The contrast is a 0.5 s grace against a 20 s session (40-fold), so
nothing here can pass by the ordinary timeout.  MARGIN is what a loaded
machine may add to the grace; the sweeper itself runs every 50 ms.
"""

import asyncio
import time

import pytest

from manatee_amd.coord import jute
from manatee_amd.coord.zkclient import ZkClient
from manatee_amd.coord.zkserver import ZkServer
from tests.zkraw import RawSession

GRACE_MS = 500
GRACE_S = GRACE_MS / 1000.0
SESSION_MS = 20000
MARGIN_S = 1.0
EPH = "/grace/owner"


def run(coro, timeout=30):
    return asyncio.run(asyncio.wait_for(coro, timeout))


async def _server(**kw):
    srv = ZkServer(**kw)
    await srv.start()
    admin = ZkClient(srv.conn_str, session_timeout_ms=SESSION_MS)
    await admin.connect()
    await admin.mkdirp("/grace")
    return srv, admin


async def _watch_delete(cli, path):
    """A future resolving to the monotonic time ``cli`` was told that
    ``path`` is gone."""
    fut = asyncio.get_running_loop().create_future()

    def on_event(etype, _path):
        if etype == jute.EVENT_NODE_DELETED and not fut.done():
            fut.set_result(time.monotonic())
    assert await cli.exists(path, watch=on_event) is not None
    return fut


def test_client_close_expires_the_session_after_the_grace():
    async def go():
        srv, watcher = await _server(disconnect_grace_ms=GRACE_MS)
        try:
            owner = await RawSession.open(srv.conn_str, SESSION_MS)
            assert owner.timeout_ms == SESSION_MS
            await owner.create_ephemeral(EPH)
            gone = await _watch_delete(watcher, EPH)
            t0 = time.monotonic()
            owner.abort()
            took = await asyncio.wait_for(gone, GRACE_S + MARGIN_S + 1.0) - t0
            print("delete seen %.3f s after the abort" % took)
            assert GRACE_S <= took <= GRACE_S + MARGIN_S
            assert srv.stats["expired_on_disconnect"] == 1
            assert srv.stats["expired_sessions"] == 1
            assert owner.sid not in srv.sessions
        finally:
            await watcher.close()
            await srv.stop()
    run(go())


def test_orderly_close_counts_like_a_reset():
    """A killed process's kernel sends FIN when nothing is unread."""
    async def go():
        srv, watcher = await _server(disconnect_grace_ms=GRACE_MS)
        try:
            owner = await RawSession.open(srv.conn_str, SESSION_MS)
            await owner.create_ephemeral(EPH)
            gone = await _watch_delete(watcher, EPH)
            t0 = time.monotonic()
            await owner.fin()
            took = await asyncio.wait_for(gone, GRACE_S + MARGIN_S + 1.0) - t0
            print("delete seen %.3f s after the close" % took)
            assert GRACE_S <= took <= GRACE_S + MARGIN_S
            assert srv.stats["expired_on_disconnect"] == 1
        finally:
            await watcher.close()
            await srv.stop()
    run(go())


def test_reconnecting_client_keeps_its_session():
    async def go():
        srv, admin = await _server(disconnect_grace_ms=GRACE_MS)
        events = []
        cli = ZkClient(srv.conn_str, session_timeout_ms=SESSION_MS,
                       on_session=events.append)
        try:
            await cli.connect()
            sid = cli.session_id
            await cli.create(EPH, b"", mode=jute.EPHEMERAL)
            cli._writer.transport.abort()
            await asyncio.sleep(4 * GRACE_S)
            assert events == ["connected", "disconnected", "connected"]
            assert cli.session_id == sid
            stat = await admin.exists(EPH)
            assert stat is not None and stat.ephemeralOwner == sid
            await cli.set_data(EPH, b"still mine")
            assert srv.sessions[sid].detached_at is None
            assert srv.stats["expired_on_disconnect"] == 0
            assert srv.stats["expired_sessions"] == 0
        finally:
            await cli.close()
            await admin.close()
            await srv.stop()
    run(go())


def test_silence_is_not_a_close():
    async def go():
        srv, watcher = await _server(disconnect_grace_ms=GRACE_MS)
        try:
            owner = await RawSession.open(srv.conn_str, SESSION_MS)
            await owner.create_ephemeral(EPH)
            await asyncio.sleep(4 * GRACE_S)        # not a byte, not a FIN
            assert await watcher.exists(EPH) is not None
            assert srv.stats["expired_on_disconnect"] == 0
            assert srv.sessions[owner.sid].detached_at is None
            gone = await _watch_delete(watcher, EPH)
            t0 = time.monotonic()
            await owner.fin()
            took = await asyncio.wait_for(gone, GRACE_S + MARGIN_S + 1.0) - t0
            print("delete seen %.3f s after the close" % took)
            assert GRACE_S <= took <= GRACE_S + MARGIN_S
            assert srv.stats["expired_on_disconnect"] == 1
        finally:
            await watcher.close()
            await srv.stop()
    run(go())


def test_default_has_no_grace():
    """Pins that default construction changes nothing (passes before the
    feature too): the session outlives its connection."""
    async def go():
        srv, admin = await _server()
        try:
            owner = await RawSession.open(srv.conn_str, 8000)
            await owner.create_ephemeral(EPH)
            owner.abort()
            await asyncio.sleep(2.0)
            assert await admin.exists(EPH) is not None
            assert owner.sid in srv.sessions
            assert srv.stats["expired_sessions"] == 0
            assert srv.stats.get("expired_on_disconnect", 0) == 0
        finally:
            await admin.close()
            await srv.stop()
    run(go())


def test_zero_and_negative_grace_mean_off():
    assert ZkServer().disconnect_grace_ms is None
    assert ZkServer(disconnect_grace_ms=0).disconnect_grace_ms is None
    assert ZkServer(disconnect_grace_ms=-5).disconnect_grace_ms is None
    assert ZkServer(disconnect_grace_ms=250).disconnect_grace_ms == 250


def test_late_return_is_told_the_session_is_gone():
    async def go():
        srv, watcher = await _server(disconnect_grace_ms=GRACE_MS)
        try:
            owner = await RawSession.open(srv.conn_str, SESSION_MS)
            await owner.create_ephemeral(EPH)
            gone = await _watch_delete(watcher, EPH)
            owner.abort()
            await asyncio.wait_for(gone, GRACE_S + MARGIN_S + 1.0)
            back = await RawSession.open(srv.conn_str, SESSION_MS,
                                         sid=owner.sid, passwd=owner.passwd)
            assert back.sid == 0
            await back.fin()
            # and the real client turns that into 'expired', which is
            # what zkmgr rebuilds its session on
            events = []
            cli = ZkClient(srv.conn_str, session_timeout_ms=SESSION_MS,
                           on_session=events.append)
            cli.session_id, cli.session_passwd = owner.sid, owner.passwd
            with pytest.raises(asyncio.TimeoutError):
                await cli.connect(timeout_s=0.5)    # never 'connected'
            assert cli.state == "expired" and events == ["expired"]
            await cli.close()
        finally:
            await watcher.close()
            await srv.stop()
    run(go())


def test_takeover_by_a_second_connection_is_not_a_client_close():
    """The server aborts the first connection itself when a second one
    presents the same session: no evidence about the client."""
    async def go():
        srv, admin = await _server(disconnect_grace_ms=GRACE_MS)
        try:
            first = await RawSession.open(srv.conn_str, SESSION_MS)
            await first.create_ephemeral(EPH)
            second = await RawSession.open(srv.conn_str, SESSION_MS,
                                           sid=first.sid,
                                           passwd=first.passwd)
            assert second.sid == first.sid
            assert await first.at_eof()
            await asyncio.sleep(4 * GRACE_S)
            assert first.sid in srv.sessions
            assert srv.sessions[first.sid].detached_at is None
            assert await admin.exists(EPH) is not None
            assert srv.stats["expired_on_disconnect"] == 0
            assert srv.stats["expired_sessions"] == 0
            await second.fin()
            await first.fin()
        finally:
            await admin.close()
            await srv.stop()
    run(go())


def test_grace_at_or_above_the_timeout_leaves_the_timeout_in_charge():
    async def go():
        srv, watcher = await _server(disconnect_grace_ms=5000)
        try:
            owner = await RawSession.open(srv.conn_str, 1000)
            assert owner.timeout_ms == 1000
            await owner.create_ephemeral(EPH)
            gone = await _watch_delete(watcher, EPH)
            t0 = time.monotonic()
            owner.abort()
            took = await asyncio.wait_for(gone, 1.0 + MARGIN_S + 1.0) - t0
            print("delete seen %.3f s after the abort" % took)
            # the session's clock started at its last request, a moment
            # before t0 (the exists() that armed the watch ran between)
            assert 0.8 <= took <= 1.0 + MARGIN_S
            assert srv.stats["expired_sessions"] == 1
            assert srv.stats["expired_on_disconnect"] == 0
        finally:
            await watcher.close()
            await srv.stop()
    run(go())
