"""A plain model of the coordination servers' data tree.

One dictionary of nodes and the rules of create / delete / setData /
check / multi / close_session, written down from the protocol's rules
and from nothing in ``zkserver`` or ``zkquorum``: ``test_zk_model.py``
drives both servers and this model with the same programs and compares
outcome and tree after every step.

An operation either succeeds or raises ``ModelError(code)`` and changes
nothing.  ``counts`` records how often each rule fired, keyed
``(context, kind, code)`` with context ``"single"`` or ``"multi"``, and
how often the two notable successful multi shapes occurred, so that a
test can tell that its programs reached every rule.
"""

import collections

from manatee_amd.coord import jute

PERSISTENT, EPHEMERAL, PERSISTENT_SEQUENTIAL, EPHEMERAL_SEQUENTIAL = 0, 1, 2, 3
FLAGS = (PERSISTENT, EPHEMERAL, PERSISTENT_SEQUENTIAL, EPHEMERAL_SEQUENTIAL)

# successful shapes counted besides the error rules
PARENT_MADE_IN_MULTI = "create under a parent made earlier in the multi"
DELETE_THEN_RECREATE = "delete then recreate of one path in the multi"


class ModelError(Exception):
    def __init__(self, code, path=""):
        self.code = code
        self.path = path
        super().__init__("%s %s" % (jute.ERROR_NAMES.get(code, code), path))


class Node:
    __slots__ = ("data", "version", "cversion", "owner", "children",
                 "next_seq")

    def __init__(self, data=b"", owner=0):
        self.data = data
        self.version = 0        # bumped by setData
        self.cversion = 0       # bumped by a create or delete of a child
        self.owner = owner      # session id of an ephemeral, else 0
        self.children = set()   # child NAMES
        self.next_seq = 0       # what the next sequential child is given

    def copy(self):
        n = Node(self.data, self.owner)
        n.version, n.cversion, n.next_seq = \
            self.version, self.cversion, self.next_seq
        n.children = set(self.children)
        return n


def parent_of(path):
    head = path.rsplit("/", 1)[0]
    return head if head else "/"


def name_of(path):
    return path.rsplit("/", 1)[1]


class ZkModel:
    def __init__(self):
        self.nodes = {"/": Node()}
        self.sessions = set()
        self.counts = collections.Counter()

    # ------------------------------------------------------------ sessions
    def open_session(self, sid):
        self.sessions.add(sid)

    def close_session(self, sid):
        self.sessions.discard(sid)
        for path in sorted(p for p, n in self.nodes.items()
                           if n.owner == sid):
            self._delete(self.nodes, path, -1)

    # ----------------------------------------------------- the rules proper
    # Each works on the node dictionary it is given, raises before it
    # changes anything, and is used for single requests and multis alike.
    def _create(self, nodes, path, data, flags, sid):
        if not path.startswith("/") or (len(path) > 1 and path.endswith("/")):
            raise ModelError(jute.ZAPIERROR, path)
        pp = parent_of(path)
        parent = nodes.get(pp)
        if parent is None:
            raise ModelError(jute.ZNONODE, pp)
        if parent.owner:
            raise ModelError(jute.ZNOCHILDRENFOREPHEMERALS, pp)
        sequential = flags in (PERSISTENT_SEQUENTIAL, EPHEMERAL_SEQUENTIAL)
        if sequential:
            path = "%s%010d" % (path, parent.next_seq)
        if path in nodes:
            raise ModelError(jute.ZNODEEXISTS, path)
        ephemeral = flags in (EPHEMERAL, EPHEMERAL_SEQUENTIAL)
        if ephemeral and sid not in self.sessions:
            raise ModelError(jute.ZSESSIONEXPIRED, path)
        if sequential:
            parent.next_seq += 1
        nodes[path] = Node(data, sid if ephemeral else 0)
        parent.children.add(name_of(path))
        parent.cversion += 1
        return path

    def _delete(self, nodes, path, version):
        if path == "/":
            raise ModelError(jute.ZBADARGUMENTS, path)
        node = nodes.get(path)
        if node is None:
            raise ModelError(jute.ZNONODE, path)
        # real ZooKeeper tests the version before the child count; both
        # servers here test the children first, and this pins their order
        if node.children:
            raise ModelError(jute.ZNOTEMPTY, path)
        if version != -1 and version != node.version:
            raise ModelError(jute.ZBADVERSION, path)
        del nodes[path]
        parent = nodes[parent_of(path)]
        parent.children.discard(name_of(path))
        parent.cversion += 1

    def _check(self, nodes, path, version):
        node = nodes.get(path)
        if node is None:
            raise ModelError(jute.ZNONODE, path)
        if version != -1 and version != node.version:
            raise ModelError(jute.ZBADVERSION, path)
        return node

    def _set_data(self, nodes, path, data, version):
        node = self._check(nodes, path, version)
        node.data = data
        node.version += 1
        return node

    # ------------------------------------------------------ single requests
    def _counted(self, context, kind, fn, *args):
        try:
            return fn(*args)
        except ModelError as exc:
            self.counts[(context, kind, exc.code)] += 1
            raise

    def create(self, path, data, flags, sid):
        return self._counted("single", "create", self._create, self.nodes,
                             path, data, flags, sid)

    def delete(self, path, version):
        return self._counted("single", "delete", self._delete, self.nodes,
                             path, version)

    def set_data(self, path, data, version):
        """Returns (version, dataLength) of the node afterwards."""
        node = self._counted("single", "setData", self._set_data, self.nodes,
                             path, data, version)
        return node.version, len(node.data)

    # --------------------------------------------------------------- multi
    def multi(self, ops, sid):
        """``ops``: ("create", path, data, flags) | ("delete", path,
        version) | ("setData", path, data, version) | ("check", path,
        version).  Runs them in order on a copy of the tree, each seeing
        the earlier ones; commits the copy only if all succeed, else
        raises the first failure and changes nothing.  Returns per op
        ("create", path) | ("setData", version, dataLength) | ("delete",)
        | ("check",)."""
        nodes = {p: n.copy() for p, n in self.nodes.items()}
        results = []
        made, deleted, shapes = set(), set(), set()
        for op in ops:
            kind = op[0]
            if kind == "create":
                path = self._counted("multi", kind, self._create, nodes,
                                     op[1], op[2], op[3], sid)
                if parent_of(path) in made:
                    shapes.add(PARENT_MADE_IN_MULTI)
                if path in deleted:
                    shapes.add(DELETE_THEN_RECREATE)
                made.add(path)
                results.append(("create", path))
            elif kind == "delete":
                self._counted("multi", kind, self._delete, nodes, op[1],
                              op[2])
                deleted.add(op[1])
                made.discard(op[1])
                results.append(("delete",))
            elif kind == "setData":
                node = self._counted("multi", kind, self._set_data, nodes,
                                     op[1], op[2], op[3])
                results.append(("setData", node.version, len(node.data)))
            elif kind == "check":
                self._counted("multi", kind, self._check, nodes, op[1],
                              op[2])
                results.append(("check",))
            else:
                raise ValueError(kind)
        self.nodes = nodes
        for shape in shapes:
            self.counts[shape] += 1
        return results

    # ---------------------------------------------------------------- view
    def tree(self):
        """path -> everything compared with a server's tree."""
        return {p: {"data": n.data, "version": n.version,
                    "cversion": n.cversion, "children": sorted(n.children),
                    "owner": n.owner, "next_seq": n.next_seq}
                for p, n in self.nodes.items()}

    def persistent(self):
        """path -> (data, sorted persistent children): what survives a
        restart of the standalone server."""
        out = {}
        for p, n in self.nodes.items():
            if n.owner:
                continue
            base = "" if p == "/" else p
            out[p] = (n.data, sorted(
                c for c in n.children
                if not self.nodes["%s/%s" % (base, c)].owner))
        return out
