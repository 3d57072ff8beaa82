"""A coordination client with no life of its own, for tests that need a
connection to die (or fall silent) exactly when the test says so: it
never pings, never reconnects and never sends CloseSession unless told
to.  ``ZkClient`` does all three by itself."""

import asyncio
import struct

from manatee_amd.coord import jute
from manatee_amd.coord.jute import Reader

NO_PASSWD = b"\x00" * 16


class RawSession:
    def __init__(self, reader, writer, timeout_ms, sid, passwd):
        self.reader = reader
        self.writer = writer
        self.timeout_ms = timeout_ms
        self.sid = sid
        self.passwd = passwd
        self._xid = 0

    @classmethod
    async def open(cls, addr, timeout_ms, sid=0, passwd=NO_PASSWD):
        """Connect handshake with one ``HOST:PORT``.  ``sid == 0`` on the
        result means the server refused the session presented."""
        host, _, port = addr.rpartition(":")
        reader, writer = await asyncio.open_connection(host, int(port))
        writer.write(jute.encode_connect_request(0, timeout_ms, sid, passwd))
        await writer.drain()
        body = await asyncio.wait_for(_read_frame(reader), 5.0)
        got_timeout, got_sid, got_passwd = jute.decode_connect_response(body)
        return cls(reader, writer, got_timeout, got_sid, got_passwd)

    async def create_ephemeral(self, path, data=b""):
        self._xid += 1
        w = jute.encode_request_header(self._xid, jute.OP_CREATE)
        w.ustring(path).buffer(data)
        jute.write_acls(w)
        w.int32(jute.EPHEMERAL)
        self.writer.write(w.framed())
        await self.writer.drain()
        while True:
            r = Reader(await asyncio.wait_for(_read_frame(self.reader), 5.0))
            xid, _zxid, err = jute.decode_reply_header(r)
            if xid == self._xid:
                break
        if err != jute.ZOK:
            raise jute.ZkError(err, path)
        return r.ustring()

    def abort(self):
        """RST, no CloseSession: what the kernel does for a killed
        process with unread data, or a rebooted host."""
        self.writer.transport.abort()

    async def fin(self):
        """Orderly close of the socket (FIN), still no CloseSession: what
        the kernel does for a killed process."""
        self.writer.close()
        try:
            await self.writer.wait_closed()
        except (ConnectionError, OSError):
            pass

    async def at_eof(self, timeout_s=2.0):
        """True once the server has closed this connection."""
        try:
            return await asyncio.wait_for(self.reader.read(1 << 16),
                                          timeout_s) == b""
        except (ConnectionError, OSError):
            return True
        except asyncio.TimeoutError:
            return False


async def _read_frame(reader):
    (n,) = struct.unpack(">i", await reader.readexactly(4))
    return await reader.readexactly(n)
