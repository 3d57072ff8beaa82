"""The crash-image helper itself (tests/crashfs.py): what the recorder
sees, what its self-check refuses, and what the two crash models make
of a handful of operations whose outcome can be worked out by hand."""

import os
import subprocess
import sys

import pytest

from tests import crashfs


def _root(tmp_path):
    root = str(tmp_path / "root")
    os.makedirs(root)
    with open(os.path.join(root, "old"), "wb") as f:
        f.write(b"old bytes")
    return root


def test_recorder_sees_every_kind_of_operation_and_restores(tmp_path):
    root = _root(tmp_path)
    before = (os.open, os.fsync, os.replace, open)
    outside = str(tmp_path / "elsewhere")
    with crashfs.Recorder(root) as rec:
        os.makedirs(os.path.join(root, "a", "b"))
        fd = os.open(os.path.join(root, "a", "f"), os.O_RDWR | os.O_CREAT)
        os.pwrite(fd, b"0123456789", 4)
        os.ftruncate(fd, 9)
        os.fsync(fd)
        os.close(fd)
        with open(os.path.join(root, "t.tmp"), "w") as f:
            f.write("one ")
            f.write("two")
            f.flush()
            os.fsync(f.fileno())
        os.replace(os.path.join(root, "t.tmp"), os.path.join(root, "t"))
        dfd = os.open(root, os.O_RDONLY)
        os.fsync(dfd)
        os.close(dfd)
        rec.mark("here")
        with open(os.path.join(root, "old"), "r+b") as f:
            f.seek(0, os.SEEK_END)
            f.write(b"+more")
            f.truncate(11)
        with open(os.path.join(root, "old"), "ab") as f:
            f.write(b"!")
        os.unlink(os.path.join(root, "a", "f"))
        with open(outside, "w") as f:        # not under the root
            f.write("x")
        with open(os.path.join(root, "old"), "rb") as f:
            assert f.read() == b"old bytes+m!"
    assert (os.open, os.fsync, os.replace, open) == before
    rec.verify()
    j = os.path.join
    assert rec.ops == [
        ("mkdir", "a"), ("mkdir", j("a", "b")),
        ("create", j("a", "f"), False),
        ("pwrite", j("a", "f"), 4, b"0123456789"),
        ("truncate", j("a", "f"), 9), ("fsync", j("a", "f"), False),
        ("create", "t.tmp", True), ("pwrite", "t.tmp", 0, b"one two"),
        ("fsync", "t.tmp", False), ("rename", "t.tmp", "t"),
        ("fsync", "", True), ("mark", "here"),
        ("pwrite", "old", 9, b"+more"), ("truncate", "old", 11),
        ("pwrite", "old", 11, b"!"), ("unlink", j("a", "f"))]


def test_self_check_fails_for_a_write_the_recorder_cannot_see(tmp_path):
    root = _root(tmp_path)
    with crashfs.Recorder(root) as rec:
        subprocess.run([sys.executable, "-c",
                        "open(%r, 'w').write('child')"
                        % os.path.join(root, "old")], check=True)
    with pytest.raises(AssertionError):
        rec.verify()


def test_process_images_are_every_prefix_and_torn_writes(tmp_path):
    start = ({""}, {})
    ops = [("create", "f", True), ("pwrite", "f", 0, b"x" * 20),
           ("mark", "m"), ("fsync", "f", False), ("unlink", "f")]
    got = [(i, img.files.get("f"))
           for i, img in crashfs.process_images(start, ops)]
    assert got == [(0, None), (1, b"")] + \
        [(1, b"x" * m) for m in (1, 7, 8, 10, 19)] + \
        [(4, b"x" * 20), (5, None)]
    # a write of two bytes can only be cut to one
    ops = [("create", "f", True), ("pwrite", "f", 0, b"ab")]
    assert [img.files.get("f") for _i, img in
            crashfs.process_images(start, ops)] == [None, b"", b"a", b"ab"]


def _outcomes(start, ops, journalled):
    out = {}
    for i, img in crashfs.powerloss_images(start, ops, journalled):
        out.setdefault(i, set()).add(
            tuple(sorted(img.files.items())))
    return out


def test_powerloss_directory_and_content_rules(tmp_path):
    start = ({""}, {"old": b"1"})
    ops = [("create", "t", True), ("pwrite", "t", 0, b"new"),
           ("fsync", "t", False), ("rename", "t", "old"),
           ("mkdir", "d"), ("create", os.path.join("d", "x"), True),
           ("fsync", "", True), ("pwrite", "old", 3, b"er")]
    old, new = ("old", b"1"), ("old", b"new")
    strict = _outcomes(start, ops, False)
    # before the file's fsync: nothing, an empty file, or all of it
    assert strict[2] == {(old,), (old, ("t", b"")), (old, ("t", b"new"))}
    # after it, strict: the NAME is still in doubt, the bytes are not
    assert strict[3] == {(old,), (old, ("t", b"new"))}
    # the rename is in doubt until the directory is fsynced, and d/x
    # needs both d's entry and d's own fsync, which never comes
    dx = (os.path.join("d", "x"), b"")
    assert strict[6] == {(old,), (new,), (dx, new)}
    assert strict[7] == {(new,), (dx, new)}
    assert strict[8] == {(new,), (dx, new), (("old", b"newer"),),
                         (dx, ("old", b"newer"))}
    # journalled: the file's fsync made its name durable too
    journalled = _outcomes(start, ops, True)
    assert journalled[3] == {(old, ("t", b"new"))}
    assert journalled[6] == {(old, ("t", b"new")), (new,), (dx, new)}
    assert sorted(strict) == sorted(journalled) == [0, 2, 3, 6, 7, 8]


def test_powerloss_drops_a_directory_whose_mkdir_did_not_survive():
    start = ({""}, {})
    sub = os.path.join("d", "f")
    ops = [("mkdir", "d"), ("create", sub, True), ("pwrite", sub, 0, b"x"),
           ("fsync", sub, False), ("fsync", "d", True)]
    images = [img for i, img in crashfs.powerloss_images(start, ops, False)
              if i == len(ops)]
    assert sorted((sorted(img.dirs), sorted(img.files.items()))
                  for img in images) == [
        ([""], []), (["", "d"], [(sub, b"x")])]
