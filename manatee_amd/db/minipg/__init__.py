"""minipg — a PostgreSQL-shaped database engine process.

There is no PostgreSQL distribution (and no network to fetch one) in
this environment, so the ``engine=postgres`` management path
(db/postgres.py — conf regeneration, recovery.conf/standby.signal,
promote trigger files, initdb/postgres binaries, libpq probes,
pg_stat_replication gating; ref lib/postgresMgr.js) is proven against
THIS engine instead: a separate binary with PostgreSQL's process
conventions and wire protocol, backed by the waldb replication core.

What is postgres-faithful:
- ``initdb -D dir`` / ``postgres -D dir`` binaries (installed under
  ``<pgBaseDir>/<version>/bin`` by tools/devcluster);
- ``postgresql.conf`` / ``recovery.conf`` (pre-12) / ``standby.signal``
  (12+), ``primary_conninfo``, ``synchronous_standby_names``,
  ``default_transaction_read_only``, promote trigger files, SIGHUP
  reload, ``PG_VERSION``, ``postmaster.pid``, dirty-kill semantics;
- the libpq v3 wire protocol (startup/auth/simple query) serving the
  introspection surface the manager and adm use —
  ``pg_is_in_recovery()``, LSN functions, ``pg_stat_replication``,
  ``pg_last_xact_replay_timestamp()`` — plus a small SQL table surface
  (INSERT/SELECT/UPDATE/DELETE on ``kv``) for write-load benchmarks;
- the extended-query protocol: Parse, Bind, Describe, Execute, Close,
  Sync and Flush, with named and unnamed statements and portals,
  ``$n`` parameters, Execute row limits (PortalSuspended) and
  skip-to-Sync after an error.  Describe answers without executing;
- transaction blocks over both protocols: ``BEGIN``/``START
  TRANSACTION``, ``COMMIT``/``END``, ``ROLLBACK``/``ABORT``, the real
  transaction status (I/T/E) in every ReadyForQuery, ``25P02`` in a
  failed block.  A block's writes are buffered in the connection and
  reach the WAL at COMMIT as ONE record, so a transaction is
  all-or-nothing across a crash and across replication; inside the
  block reads see the connection's own pending writes;
- synchronous_commit=remote_write semantics: an INSERT, or a COMMIT, is
  acknowledged only after the named sync standby reports it written.

What is not: it is a KV store, not SQL PostgreSQL, and peer-to-peer
WAL shipping uses waldb's stream (multiplexed on the same port, as
PostgreSQL multiplexes replication connections on its port).  In the
extended protocol:
- parameters and results are text only (a binary format code is
  ``0A000``); every parameter is reported as type ``text`` (oid 25);
- parameter substitution is lexical: a bound value becomes a quoted
  literal (``'`` doubled, NULL the keyword) in the statement text,
  which then goes through the same SQL layer as a simple query.  A
  value can never end its literal, let alone the statement;
- the CommandComplete of a portal executed in several steps counts the
  rows of the last step;
- outside a block every statement commits on its own, in both
  protocols: an error between two Syncs (or in a multi-statement simple
  query) stops the rest but does not undo the writes before it, where
  PostgreSQL would roll the implicit transaction back.  Use a block.
And in transactions:
- isolation is READ COMMITTED with NO row locks and NO write-write
  conflict detection: every statement reads the latest committed state
  (plus its own block's writes), and two connections that update the
  same key race — the last COMMIT wins, silently.  Writers that need
  more must not share keys (``tools/wrbench --profile tpcb`` gives
  every writer its own accounts);
- a block buffers at most 16 MiB of encoded writes (``54000`` beyond);
- no savepoints, no ``SET TRANSACTION``: the words after ``BEGIN`` are
  accepted and ignored.
"""

from .server import MinipgServer, init_data_dir, main  # noqa: F401
