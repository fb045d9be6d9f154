"""GPU: the int8 shadow scan's pair pass (dense_prefilter.hip, DESIGN.md §3 "K1F8 pair pass") and the pairing of single
fused calls (api.hip, anrag_hybrid_search_device).

A pair pass takes two queries through one walk of the image; per query every value it writes must be the single pass's,
bit for bit.  The single pass is the reference throughout: a launch of ONE query never pairs.
  1. hi rows (as uint32: NaN patterns included) and T of each query alone against groups of 2 (both positions), 3
     (pair + odd) and 16, with and without the source filter, over the row geometries that take a path of their own;
  2. no cross-talk inside a pair: partner q, -q, all-zero, NaN / inf;
  3. the group entry points end to end against prefilter mode 0;
  4. single calls in pairing mode 2 (deterministic): burst counts, parameter changes, every flush point;
  5. single calls in auto mode.
The corpora are far below the 1 GiB gate, where single fused queries would take the one-stream lanes: the indexes of 4 and 5
are created with ANRAG_SCAN_LANES=0, which leaves the three-stream pipeline as the only route (so "a lane query" among the
flush points is a single dense query through the pipeline here; the lanes and a held query cannot coexist below the gate).
The CPU-side check at the end holds the pair kernels to the register budget of the single ones."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "a-nice-rag_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"

SENTINEL = np.uint32(0x7FA5A5A5)
RW = {256: 24, 768: 8, 1024: 6, 2048: 3}  # rows per batch of the int8 scan


def _gauss(n, d, rng):
    e = rng.standard_normal((n, d), dtype=np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    return e


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---------------------------------------------------------------- 1. pair equals single, row by row
# n = 1,000 leaves waves without rows; 40,001 gives blocks of 40 rows at 768-d (a ragged last batch, a clamped last wave,
# every hi row leaving in flush); 100,003 gives blocks of 104 rows at 768-d and 120 at 256-d, longer than the 64-row hi
# store and no multiple of it, so that the store inside reduce and the carry into the next 64 rows run as well
CASES = [(d, n) for d in (256, 768, 1024, 2048) for n in (1, 1000, 40_001)] + [(256, 100_003), (768, 100_003)]


@pytest.mark.gpu
@pytest.mark.parametrize("dim,n", CASES)
def test_pair_pass_writes_the_single_pass_bits(dim, n):
    from anrag.index import Index

    rng = np.random.default_rng(100 * dim + n)
    q = _gauss(16, dim, rng)
    q[5] *= np.float32(1e3)
    q[6] *= np.float32(1e-3)
    with Index(0) as idx:
        idx.set_dense_prefilter(2)
        e = _gauss(n, dim, rng)
        idx.dense_load(e)
        geo = idx.debug_prefilter_read(data=False)
        rpw, rw = geo["rows_per_wave"], geo["batch_rows"]
        assert geo["form"] == 2 and rw == RW[dim] and rpw % rw == 0
        # the top rows of queries 0 .. 3: first and last row of a wave's block, both sides of its first 64-row hi store,
        # the corpus's first and last row
        planted = []
        for j in range(4):
            w = 2 * j + 1
            for t, at in enumerate((w * rpw, (w + 1) * rpw - 1, w * rpw + 63, w * rpw + 64, 0 if j == 0 else -1,
                                    n - 1 if j == 1 else -1)):
                if 0 <= at < n and (t < 2 or rpw > 64 or at in (0, n - 1)):
                    e[at] = q[j] * np.float32(1.0 - 0.01 * t)
                    planted.append(at)
        if n == 100_003:
            assert rpw > 64 and rpw % 64 != 0 and len(planted) >= 18, (rpw, planted)
        if n > 1000:
            assert len(planted) >= 10, (rpw, planted)
            e[n // 2, 3] = np.nan
            e[n // 2 + 1] = 0.0
        src = (np.arange(n) % 5).astype(np.uint16)
        idx.dense_load(e, source_id=src)
        assert idx.debug_prefilter_read(data=False)["rows_per_wave"] == rpw
        print(f"D={dim} n={n}: rows_per_wave {rpw}, batch_rows {rw}, {len(planted)} planted rows")
        for allow in (None, np.array([1, 1, 0, 1, 1], np.uint8)):
            for k in (25, 1, 64):
                members = list(range(16)) if k == 25 else [0, 1, 2]
                idx.set_scan_pairing(1)
                p0, s0, _ = idx.scan_pair_stats()
                alone = {i: idx.debug_prefilter_bounds(q[i], k, allow_source=allow) for i in members}
                p1, s1, pend = idx.scan_pair_stats()
                assert (p1 - p0, s1 - s0, pend) == (0, len(members), 0)
                for i in members:
                    assert not (_u32(alone[i][0]) == SENTINEL).any(), "the single pass left rows unwritten"
                groups = [[0, 1], [1, 0], [0, 1, 2], [2, 0, 1]] + ([list(range(16)), list(range(15, -1, -1))] if k == 25 else [])
                for g in groups:
                    p0, s0, _ = idx.scan_pair_stats()
                    hi, thr = idx.debug_prefilter_bounds(q[g], k, allow_source=allow)
                    p1, s1, _ = idx.scan_pair_stats()
                    assert (p1 - p0, s1 - s0) == (len(g) // 2, len(g) % 2), "the group did not take the pair form"
                    for pos, i in enumerate(g):
                        tag = f"D={dim} n={n} k={k} filter={allow is not None} group={g} position {pos}"
                        diff = np.flatnonzero(_u32(hi[pos]) != _u32(alone[i][0][0]))
                        assert diff.size == 0, f"{tag}: hi differs from the single pass on rows {diff[:8]}"
                        assert _u32(thr[pos:pos + 1])[0] == _u32(alone[i][1])[0], f"{tag}: T differs"
                # pairing off: the same group in single passes
                idx.set_scan_pairing(0)
                p0, s0, _ = idx.scan_pair_stats()
                hi, thr = idx.debug_prefilter_bounds(q[[0, 1, 2]], k, allow_source=allow)
                p1, s1, _ = idx.scan_pair_stats()
                assert (p1 - p0, s1 - s0) == (0, 3)
                for pos in range(3):
                    assert np.array_equal(_u32(hi[pos]), _u32(alone[pos][0][0])) and _u32(thr[pos:pos + 1])[0] == _u32(alone[pos][1])[0]


# ---------------------------------------------------------------- shared corpus of 2 .. 5
N, D, VOCAB = 40_001, 768, 300
NQ = 113
K, TOP_N = 25, 10


@pytest.fixture(scope="module")
def data():
    from anrag.bm25_index import Bm25Index

    rng = np.random.default_rng(2024)
    e = _gauss(N, D, rng)
    p = 1.0 / np.arange(1, VOCAB + 1) ** 1.07
    p /= p.sum()
    lens = rng.integers(5, 20, N)
    toks = rng.choice(VOCAB, size=int(lens.sum()), p=p)
    cuts = np.cumsum(lens)[:-1]
    corpus = [[f"t{j}" for j in part] for part in np.split(toks, cuts)]
    bi = Bm25Index(corpus, k1=1.7, b=0.83, epsilon=0.05)
    rows = rng.choice(N, NQ, replace=False)
    q = e[rows] + 0.05 * rng.standard_normal((NQ, D), dtype=np.float32)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    terms = [bi.term_ids([str(t) for t in rng.choice(corpus[r], size=int(rng.integers(1, 7)))]) for r in rows]
    src = (np.arange(N) % 5).astype(np.uint16)
    return e, bi, q, terms, src


def _index(data, lanes_off=False):
    from anrag.index import Index

    e, bi, _, _, src = data
    old = os.environ.get("ANRAG_SCAN_LANES")
    if lanes_off:
        os.environ["ANRAG_SCAN_LANES"] = "0"  # read by anrag_index_create
    try:
        idx = Index(0)
    finally:
        if lanes_off:
            if old is None:
                del os.environ["ANRAG_SCAN_LANES"]
            else:
                os.environ["ANRAG_SCAN_LANES"] = old
    idx.set_dense_prefilter(2)
    idx.dense_load(e, source_id=src)
    idx.bm25_load(bi.indptr, bi.post_doc, bi.post_tf, bi.idf, bi.doc_len, bi.avgdl, bi.k1, bi.b, source_id=src)
    return idx


class _Device:
    def __init__(self, data, queries=None):
        import torch
        from anrag import _native as nat

        self.torch, self.nat, self.lib = torch, nat, nat.load_library()
        _, _, q, terms, _ = data
        if queries is not None:
            q = queries
        dev = torch.device("cuda", 0)
        nq = len(q)
        self.nq = nq
        self.n_terms = [len(terms[i % len(terms)]) for i in range(nq)]
        self.Q = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(dev)
        self.T = torch.full((nq, 8), -1, dtype=torch.int32, device=dev)
        for i in range(nq):
            t = terms[i % len(terms)]
            self.T[i, : len(t)] = torch.from_numpy(np.asarray(t, dtype=np.int32)).to(dev)
        self.out_f = torch.zeros((nq, 2 * 64, 2), dtype=torch.int64, device=dev)
        self.cnt_f = torch.zeros(nq, dtype=torch.int32, device=dev)
        self.out_c = torch.zeros((nq, 2 * 64, 2), dtype=torch.int64, device=dev)
        self.out_d = torch.zeros((nq, 64, 2), dtype=torch.int64, device=dev)
        bits = np.zeros(2048, np.uint32)
        for s in (0, 1, 3, 4):
            bits[s >> 5] |= np.uint32(1 << (s & 31))
        self.allow = torch.from_numpy(bits.view(np.int32)).to(dev)
        torch.cuda.synchronize()

    def clear(self):
        self.out_f.zero_(); self.cnt_f.zero_(); self.out_c.zero_(); self.out_d.zero_()
        self.torch.cuda.synchronize()

    def fused(self, idx, qs, k=K, top_n=TOP_N, allow=False):
        a = self.allow.data_ptr() if allow else None
        for i in qs:
            self.nat.check(self.lib.anrag_hybrid_search_device(
                idx.handle, self.Q[i].data_ptr(), self.T[i].data_ptr(), self.n_terms[i], k, 5.0, 1.0, 40.0, top_n, a, a,
                self.out_f[i].data_ptr(), self.cnt_f[i:].data_ptr()))

    def candidate_group(self, idx, g, k, allow=False):
        a = self.allow.data_ptr() if allow else None
        pq = (C.c_void_p * len(g))(*[self.Q[i].data_ptr() for i in g])
        pt = (C.c_void_p * len(g))(*[self.T[i].data_ptr() for i in g])
        nt = (C.c_int32 * len(g))(*[self.n_terms[i] for i in g])
        po = (C.c_void_p * len(g))(*[self.out_c[i].data_ptr() for i in g])
        self.nat.check(self.lib.anrag_hybrid_candidates_group_device(idx.handle, pq, pt, nt, len(g), k, a, a, po))

    def dense_group(self, idx, first, n, k, allow=False):
        # n consecutive queries, k records each, packed from out_d[first]
        idx.dense_search_device(self.Q[first].data_ptr(), n, k, self.allow.data_ptr() if allow else 0,
                                self.out_d[first].data_ptr())

    def results(self, idx):
        idx.sync()
        return [x.cpu().numpy().copy() for x in (self.out_f, self.cnt_f, self.out_c, self.out_d)]


def _equal(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


# ---------------------------------------------------------------- 2. no cross-talk
@pytest.mark.gpu
def test_a_partner_changes_nothing(data):
    e, _, q, _, _ = data
    odd = q[1].copy()
    odd[7], odd[100] = np.nan, np.inf
    partners = {"same": q[0], "negated": -q[0], "zero": np.zeros(D, np.float32), "nan-inf": odd}
    qs = np.stack([q[0]] + list(partners.values())).astype(np.float32)
    dv = _Device(data, queries=qs)
    with _index(data) as idx:
        alone_b = [idx.debug_prefilter_bounds(x, K) for x in qs]
        # each query alone, end to end: a call of one query (the lanes here) never pairs
        dv.clear()
        p0, s0, _ = idx.scan_pair_stats()
        for i in range(len(qs)):
            dv.dense_group(idx, i, 1, K)
        alone_r = dv.results(idx)[3]
        assert idx.scan_pair_stats()[0] == p0
        for j, name in enumerate(partners, start=1):
            for order in ([0, j], [j, 0]):
                hi, thr = idx.debug_prefilter_bounds(qs[order], K)
                for pos, i in enumerate(order):
                    assert np.array_equal(_u32(hi[pos]), _u32(alone_b[i][0][0])), f"partner {name}: hi of query {i} differs"
                    assert _u32(thr[pos:pos + 1])[0] == _u32(alone_b[i][1])[0], f"partner {name}: T of query {i} differs"
                # the final records through the pipeline's group of 2
                pair = self_pair = dv.torch.stack([dv.Q[order[0]], dv.Q[order[1]]]).contiguous()
                out = dv.torch.zeros((2, K, 2), dtype=dv.torch.int64, device="cuda")
                dv.torch.cuda.synchronize()
                p0 = idx.scan_pair_stats()[0]
                idx.dense_search_device(pair.data_ptr(), 2, K, 0, out.data_ptr())
                idx.sync()
                assert idx.scan_pair_stats()[0] == p0 + 1
                got = out.cpu().numpy()
                for pos, i in enumerate(order):
                    assert np.array_equal(got[pos], alone_r[i, :K]), f"partner {name}: records of query {i} differ"
                del pair, self_pair


# ---------------------------------------------------------------- 3. the group entry points end to end
@pytest.mark.gpu
@pytest.mark.parametrize("allow", [False, True])
def test_groups_end_to_end_against_the_fp32_scan(data, allow):
    dv = _Device(data)
    with _index(data) as idx:
        got = {}
        for mode in (0, 2):
            idx.set_dense_prefilter(mode)
            p0, s0, _ = idx.scan_pair_stats()
            res = []
            for k in (1, 25, 64):
                dv.clear()
                at = 0
                for n in (2, 3, 8):
                    dv.candidate_group(idx, list(range(at, at + n)), k, allow)
                    dv.dense_group(idx, 32 + at, n, k, allow)
                    at += n
                r = dv.results(idx)
                assert (r[2][:13, :k, 1] >= 0).all() and (r[3][32:45].reshape(-1, 2)[: 13 * k, 1] >= 0).all()
                res.append(r)
            got[mode] = res
            p1, s1, _ = idx.scan_pair_stats()
            # per k and entry point: 2 -> 1 pair, 3 -> 1 pair + 1 single, 8 -> 4 pairs
            assert (p1 - p0, s1 - s0) == ((36, 6) if mode == 2 else (0, 0))
        for a, b in zip(got[0], got[2]):
            _equal(a, b)


# ---------------------------------------------------------------- 4. pairing of single calls, mode 2
@pytest.fixture(scope="module")
def want(data):
    """the fp32 scan's answers to the fused single calls, per (k, top_n, allow)"""
    dv = _Device(data)
    out = {}
    with _index(data, lanes_off=True) as idx:
        idx.set_dense_prefilter(0)
        for key in ((K, TOP_N, False), (K - 1, TOP_N, False), (K, TOP_N + 3, False), (K, TOP_N, True)):
            dv.clear()
            dv.fused(idx, range(NQ), k=key[0], top_n=key[1], allow=key[2])
            r = dv.results(idx)
            assert (r[1] == key[1]).all()
            assert idx.scan_pair_stats() == (0, 0, 0)
            out[key] = r[:2]
    return out


@pytest.mark.gpu
def test_burst_of_single_calls_pairs_up(data, want):
    dv = _Device(data)
    with _index(data, lanes_off=True) as idx:
        idx.set_scan_pairing(2)
        for rep in range(2):  # the second burst starts on used slots
            dv.clear()
            p0, s0, pend = idx.scan_pair_stats()
            assert pend == 0
            dv.fused(idx, range(NQ))
            assert idx.scan_pair_stats()[2] == 1  # the 113th waits for a partner
            r = dv.results(idx)
            p1, s1, pend = idx.scan_pair_stats()
            assert (p1 - p0, s1 - s0, pend) == (56, 1, 0)
            _equal(want[K, TOP_N, False], r[:2])


@pytest.mark.gpu
def test_calls_with_other_parameters_never_pair(data, want):
    dv = _Device(data)
    variants = {"similarity_k": (K - 1, TOP_N, False), "top_n": (K, TOP_N + 3, False), "filter": (K, TOP_N, True)}
    with _index(data, lanes_off=True) as idx:
        idx.set_scan_pairing(2)
        for name, other in variants.items():
            dv.clear()
            p0, s0, _ = idx.scan_pair_stats()
            for i in range(16):
                key = other if i % 2 else (K, TOP_N, False)
                dv.fused(idx, [i], k=key[0], top_n=key[1], allow=key[2])
                assert idx.scan_pair_stats()[2] == 1
            r = dv.results(idx)
            p1, s1, pend = idx.scan_pair_stats()
            assert (p1 - p0, s1 - s0, pend) == (0, 16, 0), name
            for i in range(16):
                key = other if i % 2 else (K, TOP_N, False)
                assert np.array_equal(r[0][i], want[key][0][i]) and r[1][i] == want[key][1][i], (name, i)


@pytest.mark.gpu
def test_every_other_entry_point_launches_the_held_query(data, want):
    import torch
    from anrag.index import rank_batch

    e, bi, q, terms, _ = data
    dv = _Device(data)
    side = torch.cuda.Stream(device="cuda")
    seen = {}
    with _index(data, lanes_off=True) as idx:
        idx.set_scan_pairing(2)
        legs = [dict(index=idx, weight=5.0, queries=q[:2]), dict(index=idx, weight=1.0, term_lists=terms[:2])]
        one = torch.zeros((K, 2), dtype=torch.int64, device="cuda")

        def via_signal():
            idx.signal_stream(side.cuda_stream)
            with torch.cuda.stream(side):
                seen["records"], seen["count"] = dv.out_f.clone(), dv.cnt_f.clone()
            side.synchronize()

        def via_mode_change():
            idx.set_dense_prefilter(0)
            idx.set_dense_prefilter(2)

        def via_host_query():
            ids, _ = idx.hybrid_search(q[3], terms[3], K, 5.0, 1.0, 40, TOP_N)
            assert np.array_equal(ids, want[K, TOP_N, False][0][3, :TOP_N, 1])

        points = {
            "sync": idx.sync,
            "signal_stream": via_signal,
            "wait_stream": lambda: idx.wait_stream(side.cuda_stream),
            "prefilter mode change": via_mode_change,
            "single dense query": lambda: idx.dense_search_device(dv.Q[5].data_ptr(), 1, K, 0, one.data_ptr()),
            "rank_batch": lambda: rank_batch(legs, 2, 500, 40, 500, id_space=N, want_scores=True),
            "host-pointer query": via_host_query,
        }
        for i, (name, call) in enumerate(points.items()):
            dv.clear()
            p0, s0, _ = idx.scan_pair_stats()
            dv.fused(idx, [i])
            assert idx.scan_pair_stats()[2] == 1, name
            call()
            assert idx.scan_pair_stats()[2] == 0, f"{name} left the query held"
            if name == "signal_stream":
                assert np.array_equal(seen["records"].cpu().numpy()[i], want[K, TOP_N, False][0][i]), name
                assert int(seen["count"][i]) == TOP_N
            r = dv.results(idx)
            assert np.array_equal(r[0][i], want[K, TOP_N, False][0][i]) and r[1][i] == TOP_N, f"{name}: the held query's answer"
            p1, s1, _ = idx.scan_pair_stats()
            assert p1 == p0 and s1 - s0 >= 1, name
        # caller-owned streams: nothing is ever held
        streams = [torch.cuda.Stream(device="cuda") for _ in range(3)]
        idx.set_streams(*(s.cuda_stream for s in streams))
        dv.clear()
        for i in range(5):
            dv.fused(idx, [i])
            assert idx.scan_pair_stats()[2] == 0
        r = dv.results(idx)
        _equal([want[K, TOP_N, False][0][:5], want[K, TOP_N, False][1][:5]], [r[0][:5], r[1][:5]])
        idx.set_streams(0, 0, 0)
    # destroy
    idx = _index(data, lanes_off=True)
    idx.set_scan_pairing(2)
    dv.clear()
    dv.fused(idx, [9])
    assert idx.scan_pair_stats()[2] == 1
    idx.close()
    torch.cuda.synchronize()
    assert np.array_equal(dv.out_f[9].cpu().numpy(), want[K, TOP_N, False][0][9]) and int(dv.cnt_f[9]) == TOP_N


# ---------------------------------------------------------------- 5. auto mode
@pytest.mark.gpu
def test_auto_mode_never_holds_a_lone_query_and_loses_none(data, want):
    dv = _Device(data)
    with _index(data, lanes_off=True) as idx:
        assert idx.scan_pair_stats() == (0, 0, 0)
        dv.clear()
        dv.fused(idx, [0])
        assert idx.scan_pair_stats() == (0, 1, 0), "one query on an idle index must be launched at once"
        r = dv.results(idx)
        assert np.array_equal(r[0][0], want[K, TOP_N, False][0][0])
        dv.clear()
        p0, s0, _ = idx.scan_pair_stats()
        dv.fused(idx, range(112))
        r = dv.results(idx)
        p1, s1, pend = idx.scan_pair_stats()
        print(f"auto mode, burst of 112: {p1 - p0} pair passes, {s1 - s0} single passes")
        assert 2 * (p1 - p0) + (s1 - s0) == 112 and pend == 0
        _equal([want[K, TOP_N, False][0][:112], want[K, TOP_N, False][1][:112]], [r[0][:112], r[1][:112]])


# ---------------------------------------------------------------- CPU: the pair kernels' registers
def _kernels(obj, tmp):
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
    subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(tmp, "x.o")],
                   check=True, capture_output=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fat}", f"--output={co}", "--unbundle"], check=True, capture_output=True)
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out, cur = [], {}
    for line in notes.splitlines():
        m = re.match(r"\s+-?\s*\.(name|vgpr_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\S+)", line)
        if m:
            k, v = m.groups()
            if k != "name" or v.lstrip("'").startswith("_Z"):
                cur[k] = v.strip("'")
        if ".wavefront_size" in line:
            if "name" in cur:
                out.append(cur)
            cur = {}
    return out


@pytest.mark.skipif(not (os.path.exists(f"{LLVM}/llvm-readelf") and shutil.which("c++filt")), reason="needs the ROCm LLVM tools")
def test_pair_kernels_fit_beside_k3():
    """The single kernels are held to 128 VGPRs by name (test_int8_scan_kernels_fit_beside_k3); the pair kernels have a
    name of their own and the same budget: <= 128 VGPRs, no spills, no scratch, and their LDS (both queries' codes, the
    allow bitmap) leaves K3's workgroups their share of the CU's 160 KiB."""
    obj = os.path.join(CSRC, "dense_prefilter.o")
    if not os.path.exists(obj):
        subprocess.run(["make", "-C", CSRC, "-j", "8"], check=True, capture_output=True)
    pairs = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k in _kernels(obj, tmp):
            name = subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip()
            if "i8_pair_kernel" in name:
                pairs[name] = k
    assert len(pairs) == 12, sorted(pairs)  # six dimensions, with and without the source filter
    for name, k in pairs.items():
        print(name, k["vgpr_count"], k["group_segment_fixed_size"])
        assert int(k["vgpr_count"]) <= 128, f"{name}: {k['vgpr_count']} VGPRs"
        assert int(k.get("vgpr_spill_count", 0)) == 0, name
        assert int(k.get("private_segment_fixed_size", 0)) == 0, name
        assert int(k["group_segment_fixed_size"]) <= 40 * 1024, f"{name}: {k['group_segment_fixed_size']} B of LDS"
