"""CPU: the shard group's surface without a GPU -- it exists, it refuses loudly where there is no device (no fall-back to
one index or to the CPU), `ANRAG_DEVICES` parses as documented and the block bounds are `sharded.shard_bounds`."""
import ctypes as C

import numpy as np
import pytest


def _no_gpu():
    import torch

    return not torch.cuda.is_available()


def test_group_create_without_a_device_is_nodevice():
    from anrag import _native as nat

    if not _no_gpu():
        pytest.skip("a GPU is present")
    lib = nat.load_library()
    dev = (C.c_int32 * 2)(0, 0)
    g = C.c_void_p()
    assert lib.anrag_shard_group_create(C.cast(dev, C.c_void_p), 2, C.byref(g)) == -5  # ANRAG_ERR_NODEVICE
    assert b"no CPU fallback" in lib.anrag_last_error()
    assert not g.value


def test_group_create_rejects_bad_arguments():
    from anrag import _native as nat

    lib = nat.load_library()
    dev = (C.c_int32 * 17)(*([0] * 17))
    g = C.c_void_p()
    assert lib.anrag_shard_group_create(C.cast(dev, C.c_void_p), 0, C.byref(g)) == -1
    assert lib.anrag_shard_group_create(C.cast(dev, C.c_void_p), 17, C.byref(g)) == -1
    assert lib.anrag_shard_group_create(None, 2, C.byref(g)) == -1
    assert lib.anrag_shard_group_destroy(None) == 0
    assert nat.ERR_UNSUPPORTED == -6


def test_database_manager_with_devices_raises_without_a_gpu(monkeypatch, tmp_path):
    """With ANRAG_DEVICES the loaders go to anrag_shard_group_create and its refusal comes up; no single index is ever
    constructed on the way (constructing one fails this test), let alone a CPU path."""
    import sqlite3

    from anrag import _native as nat
    from anrag import database_manager as dbm
    from anrag.bm25_index import Bm25Index

    if not _no_gpu():
        pytest.skip("a GPU is present")

    def no_single_index(*a, **k):
        pytest.fail("fell back to one anrag_index")

    created = []
    real = dbm.ShardGroup

    class Spy(real):
        def __init__(self, devices):
            created.append(list(devices))
            super().__init__(devices)

    monkeypatch.setattr(dbm, "Index", no_single_index)
    monkeypatch.setattr(dbm, "ShardGroup", Spy)
    monkeypatch.setenv("ANRAG_DEVICES", "0,0")
    db = str(tmp_path / "m.db")
    conn = sqlite3.connect(db)
    conn.execute("CREATE TABLE chunks (id TEXT PRIMARY KEY, content TEXT, source TEXT, embedding BLOB, url TEXT)")
    for i in range(4):
        conn.execute("INSERT INTO chunks VALUES (?,?,?,?,?)", (f"c{i}", "x", "CG1", np.ones(8, np.float32).tobytes(), None))
    conn.commit()
    conn.close()
    with pytest.raises(nat.AnragError) as e:
        dbm.DatabaseManager().load_embeddings_from_sql(db)
    assert e.value.code == -5 and "no CPU fallback" in str(e.value)
    with pytest.raises(nat.AnragError) as e:
        dbm.Bm25Proxy(Bm25Index([["a", "b"], ["b", "c"], ["c"]]), ["s", "s", "t"])
    assert e.value.code == -5
    assert created == [[0, 0], [0, 0]]  # both refusals came through the group


def test_database_manager_rejects_a_bad_device_list(monkeypatch):
    from anrag.database_manager import DenseHandle

    monkeypatch.setenv("ANRAG_DEVICES", "0,x")
    with pytest.raises(ValueError):
        DenseHandle(np.ones((4, 8), np.float32), ["a", "b", "a", "b"])


def test_devices_parsing():
    from anrag.index import parse_devices

    assert parse_devices("0, 1,1") == [0, 1, 1]
    assert parse_devices("3") == [3]
    assert parse_devices(",".join(["0"] * 16)) == [0] * 16
    for bad in ("", " ", "0,,1", "0,", "-1", "0,-2", "a", "0,b", "1.5", ",".join(["0"] * 17)):
        with pytest.raises(ValueError):
            parse_devices(bad)


def test_group_bounds_are_shard_bounds():
    from anrag.index import group_bounds
    from anrag.sharded import shard_bounds

    for n in (1, 7, 1003, 9609):
        for s in range(1, 9):
            lo = group_bounds(n, s)
            assert len(lo) == s + 1 and lo[0] == 0 and lo[-1] == n
            for r in range(s):
                assert (lo[r], lo[r + 1]) == shard_bounds(n, s, r), (n, s, r)
