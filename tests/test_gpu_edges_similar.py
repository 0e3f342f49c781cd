"""Cosine neighbour search (K12, csrc/similar.hip) at its edges: every rank class of the sweep
and every float4 tail mask against the fp64 reference, the log cuts of sim_compact (cut every
few tiles, cut among equal score words, keys with a clear top bit), the merge at its stage
and slice-count boundaries, scaling and the no-direction contract, als_similar_unit_rows at
its word / block / grid edges, and the engine's switch between the two routes.

Inputs come from test_similar_edges_cpu.py, which pins them on the CPU.  Tables are built on
the host as fp32; the reference is similar_ref.py (fp64 numpy on the same fp32 values).
Tolerance: similar_ref.check (an index may differ only where fp64 scores tie within 1e-5,
scores at rtol = atol = 1e-5); on top of it the grid asserts that the tie rule has to excuse
at most 0.1 % of the listed positions — the CPU file shows that 1.2 % of the positions have
their next fp64 score inside that window, so a kernel scrambling near-equal scores fails it.
"""
import functools

import numpy as np
import pytest
import torch

import similar_ref as R
import test_similar_edges_cpu as C
from als_mi355x import _lib
from als_mi355x import engine as E
from als_mi355x import filters as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(M, ld, fill=float("nan")):
    """M [m, k] as a device table of leading dimension ld, columns [k, ld) holding `fill`."""
    M = np.array(M, np.float32)
    out = torch.full((M.shape[0], ld), fill, device=DEV)
    out[:, :M.shape[1]] = torch.as_tensor(M).to(DEV)
    return out.contiguous()


def _bits(allow):
    return None if allow is None else F.pack_allow_bits(
        torch.as_tensor(np.nonzero(allow)[0]).to(DEV), len(allow))


def _i32(a):
    return None if a is None else torch.as_tensor(np.array(a, np.int32)).to(DEV)


def _run(Q, T, top, self_rows=None, allow=None, slices=0, ld=None, ldq=None):
    rank = T.shape[1]
    Td = _dev(T, E.ld_for(rank) if ld is None else ld)
    Qd = _dev(Q, E.ld_for(rank) + 4 if ldq is None else ldq)   # ldq != ld throughout
    idx, sc = E.similar_rows(Qd, len(Q), Td, len(T), rank, top, _i32(self_rows), _bits(allow),
                             slices)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sc.cpu().numpy()


def _same(a, b, msg=""):
    np.testing.assert_array_equal(a[0], b[0], err_msg=msg)
    np.testing.assert_array_equal(a[1].view(np.int32), b[1].view(np.int32), err_msg=msg)


def _score_err(idx, sc, S):
    """Largest |score - fp64 score| over the listed pairs."""
    live = idx >= 0
    ref = np.take_along_axis(S, np.where(live, idx, 0), 1)
    return float(np.abs(sc.astype(np.float64) - ref)[live].max()) if live.any() else 0.0


# ------------------------------------------------------------------ 1. rank and layout grid
def test_grid_covers_every_value():
    cases = C.grid_cases()
    assert {(r, t) for r, t, _ in cases} == {(r, t) for r in C.RANKS for t in C.TOPS}
    assert {(C.sweep_of(r), q) for r, _, q in cases} == {(c, q) for c in C.SWEEPS for q in C.NQS}


@functools.lru_cache(maxsize=None)
def _grid_case(rank, top, n_q):
    T, rows = C.grid_table(rank), C.grid_queries(rank)[:n_q]
    Q, ld = T[rows], E.ld_for(rank)
    a = _run(Q, T, top, rows, slices=C.GRID_SLICES, ld=ld, ldq=ld + 4)
    b = _run(Q, T, top, rows, slices=C.GRID_SLICES, ld=ld + 8, ldq=ld)
    _same(a, b, "the two strides")
    S, adm = R.cosine(Q, T), R.admissible(Q, T, rows)
    R.check(a[0], a[1], S, adm, top)
    return a, S, adm


@pytest.mark.parametrize("rank,top,n_q", C.grid_cases())
def test_rank_and_layout_grid(rank, top, n_q):
    (idx, sc), S, adm = _grid_case(rank, top, n_q)
    for r in range(n_q):                       # the exact tie 10 / 20: the lower index first
        lst = list(idx[r])
        if 10 in lst and 20 in lst:            # (rank 1: every row of that sign ties with them)
            i10, i20 = lst.index(10), lst.index(20)
            assert i10 < i20 and (rank < 3 or i20 == i10 + 1)
        assert not {C.ZERO, C.NAN, C.INF} & set(lst)
    if rank >= 2:
        assert idx[0, 0] == 20 and abs(sc[0, 0] - 1) <= 1e-6             # query 10: its twin
        if n_q > 1:
            assert idx[1, 0] == 40 and abs(sc[1, 0] - 1) <= 1e-6         # query 30 = 3 x row 40
    err = _score_err(idx, sc, S)
    print(f"grid rank {rank} top {top} n_q {n_q}: score err {err:.2e}, "
          f"excused {C.excused(idx, S, adm, top)}")


def test_grid_excused_share_is_capped():
    """Pooled over every grid case of rank >= 3: the positions whose index departs from the
    fp64 ranking (all inside the 1e-5 window, or check fails) are at most 0.1 % of the listed
    ones.  Measured: 10 of 94,012 (0.0106 %, the fp32 emulation of the CPU file gives the
    same count); the worst score error per instantiation is printed alongside."""
    bad = listed = 0
    worst = {}
    for rank, top, n_q in C.grid_cases():
        if rank < 3:
            continue
        (idx, sc), S, adm = _grid_case(rank, top, n_q)
        e, m = C.excused(idx, S, adm, top)
        bad += e
        listed += m
        cls = C.sweep_of(rank)
        worst[cls] = max(worst.get(cls, 0.0), _score_err(idx, sc, S))
    print(f"excused {bad} of {listed} = {bad / listed:.4%}; worst score error {worst}")
    assert bad <= 0.001 * listed, (bad, listed)


@pytest.mark.parametrize("rank", [1, 2])
@pytest.mark.parametrize("top,n_q", [(10, 17), (256, 33)])
def test_ranks_one_and_two(rank, top, n_q):
    """All cosines are +-1 (rank 1) or densely tied (rank 2), so the index rule says nothing:
    every listed score within 1e-6 of its fp64 value, no negative-cosine row before a
    positive one, the direction-less rows absent."""
    T = C.grid_table(rank)[:200]               # 196 neighbours: top 256 lists both signs
    rows = np.arange(100, 100 + n_q)
    idx, sc = _run(T[rows], T, top, rows, slices=C.GRID_SLICES)
    S = R.cosine(T[rows], T)
    R.check(idx, sc, S, R.admissible(T[rows], T, rows), top)
    live = idx >= 0
    assert (live.sum(axis=1) == min(top, 196)).all()
    ref = np.take_along_axis(S, np.where(live, idx, rows[:, None]), 1)
    assert np.abs(sc - ref)[live].max() <= 1e-6
    sign = np.where(live, np.sign(ref), -2)    # open slots last
    assert (np.diff(sign, axis=1) <= 0).all()
    assert top < 196 or ((sign == 1).any(axis=1) & (sign == -1).any(axis=1)).all()
    assert not np.isin(idx, [C.ZERO, C.NAN, C.INF]).any()
    assert (idx != rows[:, None]).all()


# ------------------------------------------------------------------ 2. log cuts
@pytest.mark.parametrize("top", C.RISING_TOPS)
@pytest.mark.parametrize("rank", C.CUT_RANKS)
def test_rising_scores_cut_every_few_tiles(rank, top):
    """One slice; query 0's scores rise with the row index, so every tile's 16 keys pass its
    threshold and its log is cut every (cap - top) / 16 tiles to the end, while the other 15
    logs fill at their own pace."""
    T, Q, self_rows = C.rising_table(rank)
    idx, sc = _run(Q, T, top, self_rows, slices=1)
    S, adm = R.cosine(Q, T), R.admissible(Q, T, self_rows)
    R.check(idx, sc, S, adm, top)
    assert idx[0, 0] >= C.CUT_N - 3            # neighbours of the last row, within the tie rule
    print(f"rising rank {rank} top {top}: score err {_score_err(idx, sc, S):.2e}")


@pytest.mark.parametrize("top", [1, 256])
@pytest.mark.parametrize("rank", C.CUT_RANKS)
def test_falling_scores_pass_nothing_after_the_first_cut(rank, top):
    T, Q, self_rows = C.rising_table(rank)
    T = np.ascontiguousarray(T[::-1])
    self_rows = np.where(self_rows >= 0, C.CUT_N - 1 - self_rows, -1)
    idx, sc = _run(Q, T, top, self_rows, slices=1)
    R.check(idx, sc, R.cosine(Q, T), R.admissible(Q, T, self_rows), top)
    assert idx[0, 0] <= 2


def _check_floods(idx, sc, floods, adm):
    """Of each flood, every list holds exactly the lowest-index admissible copies, in ascending
    index order, with identical score bits; a flood listed only in part ends the list."""
    for r in range(len(idx)):
        for pos in floods:
            at = np.nonzero(np.isin(idx[r], pos))[0]
            if len(at) == 0:
                continue
            want = pos[adm[r, pos]]
            np.testing.assert_array_equal(idx[r, at], want[:len(at)], err_msg=f"query {r}")
            assert (np.diff(at) == 1).all(), (r, at)
            assert len(set(sc[r, at].view(np.int32).tolist())) == 1, (r, sc[r, at])
            if len(at) < len(want):
                assert at[-1] == idx.shape[1] - 1, (r, at)


@pytest.mark.parametrize("top", C.FLOOD_TOPS)
@pytest.mark.parametrize("rank", C.CUT_RANKS)
def test_tie_floods_are_cut_by_index(rank, top):
    """300 exact copies of query 0 and 70 of query 1 (every third scaled by a power of two:
    the same score bits), one slice: whenever a cut falls inside a flood, sim_compact's
    second search has to pick the lowest indices among equal score words.  Plain, with an
    allow mask clearing every third copy, and with self_rows naming a copy."""
    T, Q, posA, posB, self_rows = C.flood_table(rank)
    S = R.cosine(Q, T)
    named = self_rows.copy()
    named[0], named[1], named[2] = posA[0], posB[3], posA[1]
    for allow, sr in ((None, self_rows), (C.flood_allow(len(T), posA, posB), self_rows),
                      (None, named)):
        idx, sc = _run(Q, T, top, sr, allow, slices=1)
        adm = R.admissible(Q, T, sr, allow)
        _check_floods(idx, sc, (posA, posB), adm)
        R.check(idx, sc, S, adm, top)
        assert idx[0, 0] == posA[adm[0, posA]][0] and idx[1, 0] == posB[adm[1, posB]][0]
        assert abs(sc[0, 0] - 1) <= 1e-6
        if top >= 64:
            assert np.isin(idx[2], posA).sum() >= top - 64     # the mid-list query cuts in A


@pytest.mark.parametrize("top", [10, 256])
@pytest.mark.parametrize("rank", C.CUT_RANKS)
def test_all_negative_lists(rank, top):
    """Every key has a clear top bit: the 32-step search of the score word ends in its low
    half."""
    T, Q = C.negative_table(rank)
    idx, sc = _run(Q, T, top, slices=1)
    R.check(idx, sc, R.cosine(Q, T), R.admissible(Q, T), top)
    assert (idx >= 0).all() and (sc < 0).all()


# ------------------------------------------------------------------ 3. merge
MERGE_SLICES = (63, 64, 65, 96, 97, 2049, 4096)


@pytest.mark.parametrize("top", [1, 256])
@pytest.mark.parametrize("rank", C.CUT_RANKS)
def test_merge_boundaries_are_bit_identical_to_one_slice(rank, top):
    """The flood table at 5000 rows, 17 queries (a second pass of one): 63 / 64 one merge
    stage, 65 the first two-stage count, 97 a last first-stage group of one list, 2049 and
    4096 slices of 3 and 2 rows (4096: the second stage streams 128 x top keys); the floods
    make both stages cut among equal score words."""
    n = 5000
    T, Q, posA, posB, self_rows = C.flood_table(rank, n, 14)
    assert len(Q) == 17
    base = _run(Q, T, top, self_rows, slices=1)
    adm = R.admissible(Q, T, self_rows)
    R.check(base[0], base[1], R.cosine(Q, T), adm, top)
    _check_floods(base[0], base[1], (posA, posB), adm)
    ws = _lib.lib().als_similar_workspace_bytes
    for s in MERGE_SLICES:
        assert ws(n, 16, top, s) >= 16 * s * top * 8 > 0
        _same(base, _run(Q, T, top, self_rows, slices=s), f"slices={s}")


@pytest.mark.parametrize("n,slices", [(5, 8), (1, 3)])
def test_more_slices_than_rows(n, slices):
    rng = np.random.default_rng(n)
    T = rng.standard_normal((n, 10)).astype(np.float32)
    rows = np.array([0, n - 1])
    assert _lib.lib().als_similar_workspace_bytes(n, 2, 10, slices) > 0
    for sr in (rows, [-1, -1]):
        idx, sc = _run(T[rows], T, 10, sr, slices=slices)
        adm = R.admissible(T[rows], T, sr)
        R.check(idx, sc, R.cosine(T[rows], T), adm, 10)
        m = int(adm[0].sum())
        assert (idx[:, m:] == -1).all() and np.isneginf(sc[:, m:]).all() and (idx[:, :m] >= 0).all()


# ------------------------------------------------------------------ 4. scaling, no direction
@pytest.mark.parametrize("rank", C.CUT_RANKS)
def test_power_of_two_scaling_to_2_pow_40(rank):
    """|t|^2 k stays finite and normal inside 2^+-40, so dot, norm and quotient scale exactly."""
    T = C.grid_table(rank)
    rows = C.grid_queries(rank)[:17]
    rng = np.random.default_rng(40 + rank)
    et = np.ldexp(np.float32(1), rng.integers(-40, 41, len(T))).astype(np.float32)
    eq = np.ldexp(np.float32(1), rng.integers(-40, 41, len(rows))).astype(np.float32)
    with np.errstate(invalid="ignore"):
        Ts, Qs = T * et[:, None], T[rows] * eq[:, None]
    a = _run(T[rows], T, 100, rows, slices=3)
    b = _run(Qs, Ts, 100, rows, slices=3)
    _same(a, b)
    assert et.min() == 2.0 ** -40 and et.max() == 2.0 ** 40


def _extreme_report(idx, sc, S, extreme):
    """{row: (times listed, largest score error where listed)}."""
    out = {}
    for j in extreme:
        at = idx == j
        err = np.abs(sc.astype(np.float64) - S[:, j][:, None])[at]
        out[int(j)] = (int(at.sum()), float(err.max()) if at.any() else 0.0)
    return out


@pytest.mark.parametrize("rank", C.CUT_RANKS)
def test_rows_whose_norm_under_or_overflows(rank):
    """The contract, not the kernel: a row whose fp32 |t|^2 is subnormal, zero or Inf (norms
    2^-70, 2^-76, 2^+70) is either absent or listed with a score within 1e-5 of its fp64
    cosine, never with another score.  Three of the six rows are exact multiples of query 0
    (true cosine 1: a wrong score shows at position 0).  The sweep leaves every such row
    out (|t|^2 below 2^-100 or not finite: no direction); the unit copy + K5 route takes
    fp64 norms and lists them, accurately — a documented difference between the routes."""
    T, rows, extreme = C.extreme_table(rank)
    Q = T[rows]
    S = R.cosine(Q, T)
    for top in (10, 256):
        idx, sc = _run(Q, T, top, rows, slices=3)
        rep = _extreme_report(idx, sc, S, extreme)
        print(f"sweep rank {rank} top {top}: extreme rows (listed, err) {rep}")
        assert all(err <= 1e-5 for _, err in rep.values()), rep
        adm = R.admissible(Q, T, rows)
        for r in range(len(rows)):                 # what is absent is not expected
            gone = np.setdiff1d(extreme, idx[r])
            adm[r, gone] = False
        R.check(idx, sc, S, adm, top)
        assert idx[0, 0] in extreme[::2] or abs(sc[0, 0]) < 0.99
    # the other route: fp64 norms, so these rows have a direction and are listed
    Td = _dev(T, E.ld_for(rank), 0.0)
    i2, s2 = E.similar_rows_unit(torch.as_tensor(np.array(rows)).to(DEV), Td, len(T), rank, 10)
    torch.cuda.synchronize()
    i2, s2 = i2.cpu().numpy(), s2.cpu().numpy()
    R.check(i2, s2, S, R.admissible(Q, T, rows), 10)
    np.testing.assert_array_equal(i2[0, :3], extreme[::2])


# ------------------------------------------------------------------ 5. als_similar_unit_rows
UNIT_RANKS = (1, 3, 4, 5, 63, 64, 65, 127, 128)     # l steps by 64 columns: 65 = a second trip
UNIT_ROWS = (1, 31, 32, 33, 127, 128, 129)          # a wavefront = 32 rows, a block = 4 words


def _unit_case(rank, n, seed):
    """Gaussian rows; a zero, a NaN and an Inf row among the first and the last 32 rows."""
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((n, rank)).astype(np.float32)
    for base, sign in ((1, 1), (n - 2, -1)):
        for i, kind in enumerate((0.0, np.nan, np.inf)):
            j = base + sign * 2 * i
            if 0 <= j < n:
                if kind == 0.0:
                    T[j] = 0
                else:
                    T[j, (rank - 1) * (i % 2)] = kind
    allow = rng.random(n) < 0.6
    return T, allow


def _words(bits_bool):
    """bool [n] -> the int32 mask words, unused bits of the last word 0."""
    n_words = max((len(bits_bool) + 31) // 32, 1)
    padded = np.zeros(32 * n_words, np.uint8)
    padded[:len(bits_bool)] = bits_bool
    return np.packbits(padded, bitorder="little").view(np.uint32).view(np.int32)


def _check_unit(T, allow, rank):
    n = len(T)
    Td = _dev(T, E.ld_for(rank) + 4)                 # NaN in [k, ld) of the input
    Tn, bits, valid = E.unit_rows(Td, n, rank, _bits(allow))
    _, bits1, _ = E.unit_rows(Td, n, rank, None)
    torch.cuda.synchronize()
    ok = R.has_direction(T)
    np.testing.assert_array_equal(valid.cpu().numpy(), ok.astype(np.int32))
    want = np.where(ok[:, None], T.astype(np.float64), 0)
    want = want / np.where(ok, np.sqrt((want * want).sum(1)), 1)[:, None]
    got = Tn.cpu().numpy()
    assert got.shape == (n, E.ld_for(rank) + 4)
    np.testing.assert_allclose(got[:, :rank], want, rtol=0, atol=6e-8)   # one fp32 rounding
    assert (got[:, rank:] == 0).all()
    np.testing.assert_array_equal(bits.cpu().numpy(), _words(allow & ok))
    np.testing.assert_array_equal(bits1.cpu().numpy(), _words(ok))
    return float(np.abs(got[:, :rank] - want).max())


@pytest.mark.parametrize("rank", UNIT_RANKS)
def test_unit_rows_word_and_block_edges(rank):
    """Unit copy within one fp32 rounding of the fp64 quotient (6e-8 absolute on unit rows),
    columns [k, ld) exactly 0, valid exact, and the returned mask equal to allow &
    has_direction word for word.  The unused bits of the last word are expected to be 0:
    filters.pack_allow_bits drops rows >= n, so they come in clear, and the kernel ANDs each
    word with a mask that holds a bit only for a row < n with a direction — which also
    clears them in the all-ones mask the binding passes for allow = None."""
    worst = 0.0
    for n in UNIT_ROWS:
        T, allow = _unit_case(rank, n, 100 * rank + n)
        worst = max(worst, _check_unit(T, allow, rank))
    print(f"unit rows rank {rank}: worst error {worst:.2e}")


def test_unit_rows_grid_stride_second_trip():
    """262,177 rows: 8,194 mask words > 4 x 2048 blocks, so the first two wavefronts take a
    second trip of the grid-stride loop; the last word holds one row."""
    n = 262_177
    assert (n + 31) // 32 > 4 * 2048 and n % 32 == 1
    T, allow = _unit_case(3, n, 7)
    _check_unit(T, allow, 3)


# ------------------------------------------------------------------ 6. the route switch
def test_route_switch_keeps_the_contract():
    rank, n, top = 33, 1500, 10
    rng = np.random.default_rng(6)
    V = rng.standard_normal((n, rank)).astype(np.float32)
    V[3], V[5] = 0, V[4]
    core = E.ALSCore.from_factors(np.arange(4), np.ones((4, rank), np.float32), np.arange(n), V)
    S = R.cosine(V, V)
    m0 = E.SIMILAR_SWEEP_MIN_ROWS
    got = {}
    for m in (m0 - 1, m0, m0 + 1):
        keys, ids, sc = core.similar(np.arange(m), top)
        torch.cuda.synchronize()
        assert keys.cpu().numpy().tolist() == list(range(m))
        rows = np.arange(m)
        idx = ids.cpu().numpy()
        idx = np.where(np.isneginf(sc.cpu().numpy()), -1, idx)
        got[m] = (idx, sc.cpu().numpy())
        R.check(idx, got[m][1], S[:m], R.admissible(V[:m], V, rows), top)
    (ia, sa), common = got[m0 - 1], m0 - 1           # the sweep; the other two: unit copy + K5
    for m in (m0, m0 + 1):
        ib, sb = got[m][0][:common], got[m][1][:common]
        live = ia >= 0
        assert np.array_equal(live, ib >= 0)
        assert np.abs(sa[live] - sb[live]).max() <= 1e-5
        for r, p in zip(*np.nonzero(ia != ib)):      # only where fp64 scores tie within 1e-5
            assert abs(S[r, ia[r, p]] - S[r, ib[r, p]]) <= 1e-5, (m, r, p)
