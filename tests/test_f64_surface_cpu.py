"""CPU: the float64-query entry points exist at every layer -- header, library, ctypes table, Index -- and the host layer
routes by them (no compute: there is no GPU in this container)."""
import inspect
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("anrag_hybrid_search_f64", "anrag_set_dense_f64_scan", "anrag_dense_f64_stats")


def test_new_entry_points_are_declared_exported_and_bound():
    from anrag import _native as nat
    from anrag.index import Index, ShardGroup

    header = open(os.path.join(REPO, "include", "anrag.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = nat.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared in include/anrag.h"
        assert name in nat.EXPORTS and hasattr(lib, name), f"{name} not exported / bound"
    # the fused fp64 call takes anrag_hybrid_search's arguments, with a double query
    assert nat._SIGNATURES["anrag_hybrid_search_f64"] == nat._SIGNATURES["anrag_hybrid_search"]
    for method in ("hybrid_search_f64", "set_dense_f64_scan", "dense_f64_stats", "dense_f64_scan_serves"):
        assert callable(getattr(Index, method, None)), f"Index.{method} missing"
    assert not hasattr(ShardGroup, "hybrid_search_f64")  # a group form is out of scope: the host layer must not find one
    assert (inspect.signature(Index.hybrid_search_f64).parameters.keys()
            == inspect.signature(Index.hybrid_search).parameters.keys())


def test_served_dimensions():
    from anrag.index import Index

    probe = Index.__new__(Index)
    for dim, served in ((8, True), (100, True), (384, True), (3072, True), (6, False), (3076, False), (4096, False)):
        probe.n_rows, probe.dim = 10, dim
        assert probe.dense_f64_scan_serves() == served, dim
    probe.n_rows = 0
    assert not probe.dense_f64_scan_serves()
    probe._h = None  # (never created: nothing to destroy)
