"""The float64 leg of `rank_batch` without a GPU: how `_fill_leg` fills the C struct for `queries_f64` and `queries`, and
a numpy model of K1TD's transposed lane reduction (a-nice-rag_amd/csrc/dense_tile_f64.hip).

The model moves whole 64-lane vectors exactly as the kernel's exchanges do (v_permlane32_swap, v_permlane16_swap, the
lane ^ d moves of wave_topk.hpp) and merges them in the kernel's binary-counter order.  It is run twice: on symbols, to
show that every value is summed by exactly the tree "distance 32, then 16, 8, 4, 2, 1" of K1D (the two operands of an
addition may come in either order: IEEE addition commutes), and on random doubles, where the bits must equal the plain
butterfly's.  It reports which lane ends up with which value; the kernel's store indexing is held to that."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(REPO, "a-nice-rag_amd", "csrc", "dense_tile_f64.hip")

from anrag import _native as nat
from anrag import index as index_mod


# ------------------------------------------------------------------ _fill_leg
class _StubIndex:
    dim = 8
    handle = None


def _filled(leg, n_queries):
    slot, keep = nat.RankLeg(), []
    index_mod._fill_leg(slot, leg, 0, n_queries, keep)
    return slot, keep


def test_fill_leg_queries_f64_is_kind_2_and_keeps_the_bits():
    rng = np.random.default_rng(5)
    q32 = rng.standard_normal((3, 8)).astype(np.float32)
    q = q32.astype(np.float64) + 1e-9 * rng.standard_normal((3, 8))
    assert (q.astype(np.float32).astype(np.float64) != q).any()  # a cast down would show
    slot, keep = _filled(dict(index=_StubIndex(), weight=0.5, queries_f64=q), 3)
    assert nat.LEG_DENSE_F64 == 2 and slot.kind == 2
    assert slot.weight == 0.5 and not slot.term_ids and not slot.term_offsets
    back = np.frombuffer((C.c_double * 24).from_address(slot.queries), dtype=np.float64)
    assert back.tobytes() == q.tobytes()
    # a strided view is made contiguous, still float64
    wide = np.zeros((3, 16))
    wide[:, ::2] = q
    slot, keep = _filled(dict(index=_StubIndex(), weight=1.0, queries_f64=wide[:, ::2]), 3)
    assert np.frombuffer((C.c_double * 24).from_address(slot.queries), dtype=np.float64).tobytes() == q.tobytes()
    # one query as a vector
    slot, keep = _filled(dict(index=_StubIndex(), weight=1.0, queries_f64=q[0]), 1)
    assert slot.kind == 2
    assert np.frombuffer((C.c_double * 8).from_address(slot.queries), dtype=np.float64).tobytes() == q[0].tobytes()


def test_fill_leg_queries_f64_is_never_cast():
    q = np.ones((2, 8), np.float32)
    with pytest.raises(AssertionError):
        _filled(dict(index=_StubIndex(), weight=1.0, queries_f64=q), 2)
    with pytest.raises(AssertionError):  # the two keys name two kinds of leg
        _filled(dict(index=_StubIndex(), weight=1.0, queries_f64=q.astype(np.float64), queries=q), 2)


def test_fill_leg_queries_still_casts_to_fp32():
    rng = np.random.default_rng(6)
    q = rng.standard_normal((2, 8)) + 1e-9
    slot, keep = _filled(dict(index=_StubIndex(), weight=1.0, queries=q), 2)
    assert nat.LEG_DENSE == 0 and slot.kind == 0
    back = np.frombuffer((C.c_float * 16).from_address(slot.queries), dtype=np.float32)
    assert back.tobytes() == q.astype(np.float32).tobytes()


def test_fill_leg_term_lists_is_kind_1():
    slot, keep = _filled(dict(index=_StubIndex(), weight=1.0, term_lists=[[1, 2], []]), 2)
    assert nat.LEG_BM25 == 1 and slot.kind == 1


def test_exports_name_the_tile_stats():
    assert "anrag_rank_f64_tile_stats" in nat.EXPORTS


# ------------------------------------------------------------------ the transposed reduction
LANES = np.arange(64)


def permlane32_swap(a, b):
    """v_permlane32_swap a, b: lanes 32..63 of a <-> lanes 0..31 of b."""
    a, b = a.copy(), b.copy()
    a[32:], b[:32] = b[:32].copy(), a[32:].copy()
    return a, b


def permlane16_swap(a, b):
    """v_permlane16_swap a, b: rows 1 and 3 (of 16 lanes) of a <-> rows 0 and 2 of b."""
    a, b = a.copy(), b.copy()
    for ra, rb in ((1, 0), (3, 2)):
        sa, sb = slice(16 * ra, 16 * ra + 16), slice(16 * rb, 16 * rb + 16)
        a[sa], b[sb] = b[sb].copy(), a[sa].copy()
    return a, b


def lane_xor(v, d):
    return v[LANES ^ d]


def merge(x, y, dist, add):
    """One level of the kernel's tile64_merge: x the earlier vector, y the later."""
    if dist == 32:
        a, b = permlane32_swap(x, y)
        return add(a, b)
    if dist == 16:
        a, b = permlane16_swap(x, y)
        return add(a, b)
    second = (LANES & dist) != 0
    own = np.where(second, y, x)
    send = np.where(second, x, y)
    return add(own, lane_xor(send, dist))


def transposed(values, levels, add):
    """values: 2^levels vectors of 64 per-lane accumulators, in the kernel's order -> the finished vector."""
    st = [None] * 6
    out = None
    for t, v in enumerate(values):
        done = True
        for lev in range(levels):
            if ((t >> lev) & 1) == 0:
                st[lev] = v
                done = False
                break
            v = merge(st[lev], v, 32 >> lev, add)
        if done:
            out = v
    assert out is not None
    for d in (4, 2, 1):  # the distances the transposed levels did not cover: the plain butterfly
        if d < (32 >> (levels - 1)):
            out = add(out, lane_xor(out, d))
    return out


def butterfly(v, add):
    for d in (32, 16, 8, 4, 2, 1):
        v = add(v, lane_xor(v, d))
    return v


def t_lane(levels):
    """The kernel's store indexing: the value (within its vector) that a lane holds."""
    t = np.zeros(64, dtype=np.int64)
    for j in range(levels):
        t |= ((LANES >> (5 - j)) & 1) << j
    return t


def storing(levels):
    return (LANES & ((1 << (6 - levels)) - 1)) == 0


def sym_add(a, b):
    out = np.empty(64, dtype=object)
    for i in range(64):
        assert a[i] != b[i]
        out[i] = frozenset((a[i], b[i]))  # an addition of two operands, in either order
    return out


@pytest.mark.parametrize("levels", [3, 4, 5, 6])
def test_transposed_reduction_is_the_tree_32_16_8_4_2_1(levels):
    n = 1 << levels
    values = []
    for t in range(n):
        v = np.empty(64, dtype=object)
        for i in range(64):
            v[i] = (t, i)  # value t's accumulator of lane i
        values.append(v)
    got = transposed(values, levels, sym_add)
    want = [butterfly(v, sym_add) for v in values]
    tl = t_lane(levels)
    holder = {}
    for lane in range(64):
        # whatever the lane holds is the complete tree of exactly one value, as the same lane of the butterfly has it
        t = tl[lane]
        assert got[lane] == want[t][lane], f"lane {lane} does not hold value {t}'s tree"
        if storing(levels)[lane]:
            assert t not in holder
            holder[t] = lane
    assert sorted(holder) == list(range(n))  # every value is stored once
    # bit (5 - j) of the lane = bit j of the value: a bit reversal of the lane's upper bits
    for t, lane in holder.items():
        assert lane == sum(((t >> j) & 1) << (5 - j) for j in range(levels))


@pytest.mark.parametrize("levels", [3, 4, 5, 6])
def test_transposed_reduction_bits_equal_the_butterfly(levels):
    rng = np.random.default_rng(levels)
    n = 1 << levels
    values = [rng.standard_normal(64) * 10.0 ** rng.integers(-8, 8, 64) for _ in range(n)]
    got = transposed(values, levels, np.add)
    tl, st = t_lane(levels), storing(levels)
    differs = 0
    for lane in np.nonzero(st)[0]:
        want = butterfly(values[tl[lane]], np.add)[0]
        assert got[lane].tobytes() == want.tobytes()
        differs += float(np.sum(values[tl[lane]])) != float(want)
    assert differs  # the order of the additions shows in the bits: the comparison means something


def test_kernel_store_indexing_is_the_models():
    src = open(KERNEL).read()
    # the lane -> value map and the storing lanes, as modelled by t_lane() and storing() above
    assert re.search(r"t_lane \|= \(\(lane >> \(5 - j\)\) & 1\) << j;", src)
    assert re.search(r"stores = \(lane & \(\(1 << \(6 - L\)\) - 1\)\) == 0;", src)
    # values in query-major order (t = query * R + row), merged at distance 32 >> level
    assert re.search(r"const int t = i \* R \+ r;", src)
    assert re.search(r"const int qi = tv / R, r_l = tv % R;", src)
    assert re.search(r"tile64_merge<\(32 >> LEVEL\)>", src)
    # geometry: (rows per batch) x (queries per group) is a whole number of vectors of 8, 16, 32 or 64 values
    r = {1: 8, 2: 4, 3: 2, 4: 2, 8: 1}
    nq = {1: 16, 2: 16, 3: 16, 4: 16, 8: 8}
    assert "return CH == 1 ? 8 : (CH == 2 ? 4 : (CH <= 4 ? 2 : 1));" in src
    assert "return CH <= 4 ? 16 : 8;" in src
    for ch in r:
        v = min(64, r[ch] * nq[ch])
        assert v in (8, 16, 32, 64) and (r[ch] * nq[ch]) % v == 0
        assert nq[ch] * ch * 256 * 8 + 8192 <= 160 * 1024  # the group's queries and the allow bitmap fit the LDS
