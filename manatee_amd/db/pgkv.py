"""PgKvClient — the WaldbClient API over the libpq wire protocol.

Write-load drivers (bench.py, soak, the integ tests) speak to whichever
engine a peer runs through one key/value client interface.  For
``engine=postgres`` (minipg) that means real SQL over libpq: INSERTs
acknowledged under synchronous_commit=remote_write, reads on standbys,
server-side counts — the pgbench-writes analogue of BASELINE.json's
headline config.

Values are JSON-encoded into the ``v`` column so callers get their
types back, exactly as with WaldbClient.
"""

from __future__ import annotations

import json
from typing import Optional

from .pgwire import PgClient, PgError


class PgKvError(RuntimeError):
    pass


def _q(text: str) -> str:
    """SQL single-quote escape."""
    return text.replace("'", "''")


# the parameterised forms (values travel as bound parameters)
PUT_STMT = "kv_put"
PUT_SQL = "INSERT INTO kv (k, v) VALUES ($1, $2)"
GET_SQL = "SELECT v FROM kv WHERE k = $1"
DELETE_SQL = "DELETE FROM kv WHERE k = $1"


class PgKvClient:
    def __init__(self, host: str, port: int, user: str = "postgres",
                 connect_timeout_s: float = 5.0,
                 query_timeout_s: float = 30.0):
        self.host = host
        self.port = port
        self.query_timeout_s = query_timeout_s
        self._cli = PgClient(host, port, user,
                             connect_timeout_s=connect_timeout_s)

    async def _query(self, sql: str, timeout_s: Optional[float] = None):
        try:
            if not self._cli.connected:
                await self._cli.connect()
            return await self._cli.query(
                sql, timeout_s=timeout_s if timeout_s is not None
                else self.query_timeout_s)
        except PgError as exc:
            # connection state is fine after a server-reported error;
            # anything transport-level invalidates the connection
            raise PgKvError(str(exc)) from exc
        except Exception:
            await self.close()
            raise

    # ------------------------------------------------------------- the API
    async def ping(self, timeout_s: float = 5.0) -> bool:
        try:
            await self._query("SELECT current_time;", timeout_s=timeout_s)
            return True
        except Exception:
            await self.close()
            return False

    async def put(self, key: str, value, timeout_s: Optional[float] = None
                  ) -> str:
        res = await self._query(
            "INSERT INTO kv (k, v) VALUES ('%s', '%s')"
            % (_q(key), _q(json.dumps(value))), timeout_s=timeout_s)
        if not res.command.startswith("INSERT"):
            raise PgKvError("unexpected result %r" % res.command)
        return res.command

    async def put_many(self, items, timeout_s: Optional[float] = None
                       ) -> int:
        """Multi-statement simple query: one round trip, N INSERTs (the
        libpq batch form); the server aborts the rest on any error."""
        items = list(items)
        sql = ";".join(
            "INSERT INTO kv (k, v) VALUES ('%s', '%s')"
            % (_q(k), _q(json.dumps(v))) for k, v in items)
        res = await self._query(sql, timeout_s=timeout_s)
        if not res.command.startswith("INSERT"):
            raise PgKvError("batch aborted at %r" % res.command)
        return len(items)

    async def get(self, key: str, timeout_s: Optional[float] = None):
        res = await self._query(
            "SELECT v FROM kv WHERE k = '%s'" % _q(key),
            timeout_s=timeout_s)
        if not res.rows:
            return None
        return json.loads(res.rows[0][0])

    async def delete(self, key: str,
                     timeout_s: Optional[float] = None) -> str:
        res = await self._query("DELETE FROM kv WHERE k = '%s'" % _q(key),
                                timeout_s=timeout_s)
        return res.command

    async def count(self, prefix: Optional[str] = None,
                    timeout_s: Optional[float] = None) -> int:
        if prefix:
            sql = "SELECT count(*) AS n FROM kv WHERE k LIKE '%s%%'" \
                % _q(prefix)
        else:
            sql = "SELECT count(*) AS n FROM kv"
        res = await self._query(sql, timeout_s=timeout_s)
        return int(res.rows[0][0])

    # ------------------------------------------------------- transactions
    async def _extended(self, call, *args,
                        timeout_s: Optional[float] = None):
        """``_query``'s connection and error handling for the
        extended-protocol calls of PgClient."""
        try:
            if not self._cli.connected:
                await self._cli.connect()
            return await call(
                *args, timeout_s=timeout_s if timeout_s is not None
                else self.query_timeout_s)
        except PgError as exc:
            raise PgKvError(str(exc)) from exc
        except Exception:
            await self.close()
            raise

    async def put_many_atomic(self, items,
                              timeout_s: Optional[float] = None) -> int:
        """All of ``items`` or none of them: one transaction block of
        parameterised INSERTs, sent as ONE pipeline (one round trip) and
        committed by the server as one WAL record."""
        items = list(items)
        if not self._cli.is_prepared(PUT_STMT):
            await self._extended(self._cli.prepare, PUT_STMT, PUT_SQL,
                                 timeout_s=timeout_s)
        entries = [("BEGIN", ())]
        entries += [(PUT_STMT, (k, json.dumps(v))) for k, v in items]
        entries.append(("COMMIT", ()))
        try:
            res = await self._extended(self._cli.pipeline, entries,
                                       timeout_s=timeout_s)
        except PgKvError:
            # the server skipped the rest, COMMIT included: the block
            # is still open (and failed) on this connection
            if self._cli.connected and self._cli.txn_status != "I":
                await self._query("ROLLBACK", timeout_s=timeout_s)
            raise
        if res[-1].command != "COMMIT":
            raise PgKvError("transaction ended with %r" % res[-1].command)
        return len(items)

    async def get_many(self, keys, timeout_s: Optional[float] = None
                       ) -> list:
        """The values of ``keys`` (None where absent) in one round trip:
        a pipeline of parameterised SELECTs."""
        res = await self._extended(
            self._cli.pipeline, [(GET_SQL, (k,)) for k in keys],
            timeout_s=timeout_s)
        return [json.loads(r.rows[0][0]) if r.rows else None for r in res]

    def transaction(self) -> "PgKvTransaction":
        """``async with kv.transaction() as tx:`` — ``tx.get``,
        ``tx.put`` and ``tx.delete`` run inside one block;
        it commits on a clean exit and rolls back when the body raises.
        Read-committed, no row locks: see docs/working-on.md."""
        return PgKvTransaction(self)

    async def status(self) -> dict:
        in_rec = (await self._query(
            "SELECT pg_is_in_recovery() as r;")).rows[0][0] in ("t", "true")
        repl = []
        res = await self._query("SELECT * FROM pg_stat_replication;")
        for row in res.dicts():
            repl.append({
                "application_name": row.get("application_name"),
                "state": row.get("state"),
                "sync_state": row.get("sync_state"),
                "sent_lsn": row.get("sent_lsn") or row.get("sent_location"),
                "write_lsn": (row.get("write_lsn")
                              or row.get("write_location")),
                "flush_lsn": (row.get("flush_lsn")
                              or row.get("flush_location")),
                "replay_lsn": (row.get("replay_lsn")
                               or row.get("replay_location")),
            })
        return {"ok": True,
                "role": "standby" if in_rec else "primary",
                "replication": repl}

    async def xlog(self) -> str:
        in_rec = (await self._query(
            "SELECT pg_is_in_recovery() as r;")).rows[0][0] in ("t", "true")
        sql = ("SELECT pg_last_wal_replay_lsn() as loc;" if in_rec
               else "SELECT pg_current_wal_lsn() as loc;")
        return (await self._query(sql)).rows[0][0]

    async def close(self) -> None:
        try:
            await self._cli.close()
        except Exception:
            pass


class PgKvTransaction:
    """The key/value calls inside one transaction block, with bound
    parameters.  Reads see committed state plus this block's own
    writes; nothing is visible to other connections, or in the WAL,
    before the block commits."""

    def __init__(self, kv: PgKvClient):
        self._kv = kv
        self._block = None

    async def __aenter__(self) -> "PgKvTransaction":
        kv = self._kv
        try:
            if not kv._cli.connected:
                await kv._cli.connect()
            self._block = kv._cli.transaction(timeout_s=kv.query_timeout_s)
            await self._block.__aenter__()
        except PgError as exc:
            raise PgKvError(str(exc)) from exc
        except Exception:
            await kv.close()
            raise
        return self

    async def __aexit__(self, exc_type, exc, tb) -> bool:
        try:
            return await self._block.__aexit__(exc_type, exc, tb)
        except PgError as err:
            raise PgKvError(str(err)) from err
        except Exception:
            await self._kv.close()
            raise

    async def _run(self, sql: str, params,
                   timeout_s: Optional[float] = None):
        if not self._kv._cli.connected:
            # never reconnect mid-block: the block died with the link
            raise PgKvError("connection lost inside a transaction")
        return await self._kv._extended(self._kv._cli.query_params, sql,
                                        params, timeout_s=timeout_s)

    async def put(self, key: str, value,
                  timeout_s: Optional[float] = None) -> str:
        res = await self._run(PUT_SQL, (key, json.dumps(value)), timeout_s)
        return res.command

    async def get(self, key: str, timeout_s: Optional[float] = None):
        res = await self._run(GET_SQL, (key,), timeout_s)
        if not res.rows:
            return None
        return json.loads(res.rows[0][0])

    async def delete(self, key: str,
                     timeout_s: Optional[float] = None) -> str:
        return (await self._run(DELETE_SQL, (key,), timeout_s)).command
