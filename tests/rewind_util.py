"""A diverged pair of waldb data directories for the rewind tests.

``build_pair`` follows the recipe of
``test_waldb.test_cascading_replication_and_promote_divergence``: a
primary ``a`` is seeded, its directory is copied to ``b`` while it runs,
``b`` follows it for some shared records and is then promoted (timeline
2 at ``P``); both sides go on writing.  ``a`` is left STOPPED with WAL
past ``P`` on timeline 1, ``b`` RUNNING as the upstream a rewind of
``a`` talks to.

Segments are tiny (``SEGMENT_BYTES``), so the 40 seed records already
span several and the divergent tail spans more than one.
"""

import asyncio
import json
import os
import shutil
import struct
import zlib

from manatee_amd.db.waldb.wal import _SEG_RE
from tests.test_waldb import Node, wait_async

SEGMENT_BYTES = 256
SEED, SHARED, DIVERGENT = 40, 10, 5
HUGE = str(1 << 30)
_HDR = struct.Struct(">II")


def knobs(ckpt_bytes=HUGE, mode="full"):
    return {"wal_segment_bytes": str(SEGMENT_BYTES),
            "checkpoint_wal_bytes": str(ckpt_bytes),
            "checkpoint_mode": mode}


def wal_bytes(data_dir):
    """``(start, bytes)``: the segment files of a directory, joined."""
    segs = sorted((int(m.group(1), 16), name)
                  for name, m in ((n, _SEG_RE.match(n))
                                  for n in os.listdir(data_dir)) if m)
    out = b""
    for start, name in segs:
        assert start == segs[0][0] + len(out), "hole before %s" % name
        with open(os.path.join(data_dir, name), "rb") as f:
            out += f.read()
    return segs[0][0], out


def segment_starts(data_dir):
    return sorted(int(m.group(1), 16) for m in
                  (_SEG_RE.match(n) for n in os.listdir(data_dir)) if m)


def read_json(data_dir, name):
    with open(os.path.join(data_dir, name)) as f:
        return json.load(f)


def records_past(data_dir, lsn):
    """How many whole records of the directory's WAL end above ``lsn``."""
    start, buf = wal_bytes(data_dir)
    pos, n = 0, 0
    while pos + _HDR.size <= len(buf):
        length, crc = _HDR.unpack_from(buf, pos)
        payload = buf[pos + _HDR.size:pos + _HDR.size + length]
        if len(payload) != length or zlib.crc32(payload) != crc:
            break
        pos += _HDR.size + length
        n += start + pos > lsn
    return n


async def _checkpointed(cli):
    st = await cli.status()
    return st["checkpoint_lsn"] == st["current_lsn"]


class Pair:
    def __init__(self, a, b, fork_lsn, divergent_keys, layered):
        self.a, self.b = a, b
        self.fork_lsn = fork_lsn
        self.divergent_keys = divergent_keys
        self.layered = layered

    def stop(self):
        self.a.stop()
        self.b.stop()

    def copy_of_a(self, dest):
        """A fresh copy of the stopped peer's directory to mutate."""
        shutil.copytree(self.a.data_dir, dest)
        return dest


def build_pair(tmp_path, position="mid", layered=False):
    """``position``: where the fork point falls in ``a``'s WAL — ``mid``
    (inside a segment), ``segstart`` (exactly on a segment start) or
    ``end`` (``a`` wrote nothing after it).  ``layered``: ``a`` runs
    ``checkpoint_mode = incremental`` with its base below the fork and
    two delta layers above it."""
    mode = "incremental" if layered else "full"
    a, b = Node(tmp_path, "a"), Node(tmp_path, "b")
    a.init()
    a.write_conf(role="primary", extra=knobs(mode=mode))
    a.start()
    pair = Pair(a, b, None, [], layered)
    try:
        asyncio.run(asyncio.wait_for(_drive(pair, position, mode), 60))
    except BaseException:
        pair.stop()
        raise
    return pair


async def _drive(pair, position, mode):
    a, b = pair.a, pair.b
    ac = a.client()
    for i in range(SEED):
        await ac.put("seed%d" % i, i)
    shutil.copytree(a.data_dir, b.data_dir,
                    ignore=shutil.ignore_patterns("waldb.pid", "waldb.conf"))
    b.write_conf(role="standby", upstream="127.0.0.1:%d" % a.port,
                 extra=knobs())
    b.start()
    bc = b.client()
    for i in range(SHARED):
        await ac.put("shared%d" % i, i)
    # a record as long as a segment makes the NEXT append roll, so the
    # record after it starts a segment; one short record after that
    # leaves the end of the WAL inside a segment
    pad = "x" * SEGMENT_BYTES
    if position == "segstart":
        await ac.put("short", 0)
        await ac.put("pad", pad)
    else:
        await ac.put("pad", pad)
        await ac.put("short", 0)
    if pair.layered:
        # the base, below the fork
        a.write_conf(role="primary", extra=knobs(1, mode))
        a.sighup()
        await wait_async(lambda: _checkpointed(ac), what="base layer")
        a.write_conf(role="primary", extra=knobs(mode=mode))
        a.sighup()
        await asyncio.sleep(0.3)

    async def caught_up():
        return (await bc.status())["current_lsn"] == \
            (await ac.status())["current_lsn"]
    await wait_async(caught_up, what="copy caught up")
    await bc.close()

    # promote the copy: timeline 2 begins at its WAL end
    b.kill9()
    b.promote_trigger()
    b.write_conf(role="primary", extra=knobs())
    b.start()
    bc = b.client()
    for i in range(DIVERGENT):
        await bc.put("new%d" % i, i)
    await bc.close()
    hist = read_json(b.data_dir, "waldb_ident.json")["history"]
    assert [h["tl"] for h in hist] == [1, 2]
    pair.fork_lsn = hist[-1]["at"]

    if position != "end":
        if pair.layered:
            a.write_conf(role="primary", extra=knobs(1, mode))
            a.sighup()
            await asyncio.sleep(0.3)
        for i in range(DIVERGENT):
            key = "lost%d" % i
            await ac.put(key, "d" * 100)
            pair.divergent_keys.append(key)
            if pair.layered and i in (1, DIVERGENT - 1):
                # two delta layers above the fork
                await wait_async(lambda: _checkpointed(ac),
                                 what="delta layer")
    await ac.close()
    a.kill9()


def start_as_standby(pair):
    """Start the (rewound) peer following the upstream."""
    pair.a.write_conf(role="standby",
                      upstream="127.0.0.1:%d" % pair.b.port,
                      extra=knobs(mode="incremental" if pair.layered
                                  else "full"))
    pair.a.start()


async def assert_converged(pair):
    """The peer streams from the upstream and serves exactly its keys."""
    ac, bc = pair.a.client(), pair.b.client()
    try:
        async def streaming():
            return (await ac.status())["upstream_status"] == "streaming"
        await wait_async(streaming, what="rewound peer streaming")

        async def caught_up():
            return (await ac.status())["replay_lsn"] == \
                (await bc.status())["current_lsn"]
        await wait_async(caught_up, what="rewound peer caught up")
        assert await ac.count() == await bc.count()
        want = await bc.scan("", limit=10000)
        assert await ac.scan("", limit=10000) == want
        assert len(want) >= SEED + SHARED + DIVERGENT
        for key in pair.divergent_keys:
            assert await ac.get(key) is None
    finally:
        await ac.close()
        await bc.close()
