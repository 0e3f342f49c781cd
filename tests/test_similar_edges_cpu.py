"""CPU side of test_gpu_edges_similar.py (K12, als_similar; no GPU, nothing launched): the
input builders the GPU file imports, and tests that pin them and the reference.

* Grid: every rank meets both tops, every query count meets every sweep instantiation.
* The 0.1 % cap of the GPU file on tie-excused positions is not vacuous: on the grid's own
  inputs the next fp64 score lies within 1e-5 on >= 0.3 % of the top-256 positions, and a
  plain numpy fp32 evaluation of the cosines departs from the fp64 order on <= 0.05 %.
* Rising / falling tables: the fp64 cosine to query 0 is strictly monotone in the row index.
* Tie floods: 300 + 70 exact copies (a third scaled by powers of two), irregular gaps over
  the whole index range, the mid-list query's flood inside the first 64 places.
* cap(top) as restated here steps at 64 / 65 and 192 / 193.
"""
import functools

import numpy as np
import pytest

import similar_ref as R

# ------------------------------------------------------------------ 1. the rank grid
SWEEPS = {(4, 1): (1, 3, 4, 5, 15, 16), (8, 1): (17, 20, 31, 32), (16, 1): (33, 63, 64),
          (16, 2): (65, 67, 68, 127, 128)}        # sim_sweep_kernel<LPR, C>: its ranks
RANKS = tuple(k for ks in SWEEPS.values() for k in ks)
TOPS = (10, 256)
NQS = (1, 15, 16, 17, 32, 33)
GRID_N, GRID_SLICES = 1000, 7                     # 143 rows a slice: off the 16-row grid
ZERO, NAN, INF = 70, 80, 90                       # planted rows without a direction
N_QROWS = 33                                      # queries: rows of the table (grid_queries)


def sweep_of(rank):
    return (4, 1) if rank <= 16 else (8, 1) if rank <= 32 else (16, 1) if rank <= 64 else (16, 2)


def grid_cases():
    """(rank, top, n_q): within a class the query counts go round, so with >= 6 (rank, top)
    pairs per class every count meets every instantiation."""
    out = []
    for ranks in SWEEPS.values():
        i = 0
        for rank in ranks:
            for top in TOPS:
                out.append((rank, top, NQS[i % len(NQS)]))
                i += 1
    return out


@functools.lru_cache(maxsize=None)
def grid_table(rank, n=GRID_N):
    """Gaussian rows with the planted rows of test_gpu_similar._table; the NaN inside [0, k)."""
    rng = np.random.default_rng(1200 + rank)
    T = rng.standard_normal((n, rank)).astype(np.float32)
    T[10] = T[20]            # an exact tie: the lower index first
    T[30] = 3 * T[40]        # cosine 1 across different norms
    T[50] = -T[60]           # cosine -1
    T[ZERO] = 0
    T[NAN, rank // 2] = np.nan
    T[INF, 0] = np.inf
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def grid_queries(rank):
    """The 33 query rows: the planted rows 10, 30 and 50, then the first 30 rows from 100 on
    whose fp64 cosine to row 40 is negative.  Rows 30 and 40 score within an fp32 rounding of
    each other for every query, in an order no fp32 evaluation can settle; wherever both are
    listed the tie rule has two positions to excuse, and in the top 256 of 1000 rows that pair
    alone would use up the GPU file's cap (measured with cosine_fp32: all of 0.11 % of the
    positions).  A query on the far side of row 40 never lists the pair, so the cap measures
    the ordinary rows; the planted queries still list it (query 30 at score 1)."""
    T = grid_table(rank)
    c = R.cosine(T[40:41], T)[0]
    rest = [j for j in range(100, len(T)) if c[j] < 0][:N_QROWS - 3]
    rows = np.array([10, 30, 50] + rest)
    rows.setflags(write=False)
    return rows


def excused(idx, S, adm, top):
    """(positions where idx departs from the fp64 ranking, listed positions): what
    similar_ref.check's tie rule has to excuse."""
    ref_i, _ = R.neighbours(S, adm, top)
    live = ref_i >= 0
    return int(((np.asarray(idx) != ref_i) & live).sum()), int(live.sum())


def cosine_fp32(Q, T):
    """The same cosines in plain numpy fp32 (an emulation: not the kernel's order of sums)."""
    Q, T = np.asarray(Q, np.float32), np.asarray(T, np.float32)
    ok = R.has_direction(T)
    Tz = np.where(ok[:, None], T, np.float32(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        S = (Q @ Tz.T) / (np.sqrt((Q * Q).sum(1))[:, None] * np.sqrt((Tz * Tz).sum(1))[None, :])
    return S.astype(np.float32)


# ------------------------------------------------------------------ 2. log cuts
def sim_cap(top):
    """similar.hip's sim_cap restated: keys of a query's log."""
    return 64 * ((top + 64 + 63) // 64)


CUT_N = 3000
CUT_RANKS = (20, 128)
RISING_TOPS = (1, 63, 64, 65, 192, 193, 255, 256)
FLOOD_TOPS = (1, 10, 64, 100, 256)
N_FLOOD_A, N_FLOOD_B = 300, 70


@functools.lru_cache(maxsize=None)
def rising_table(rank, n=CUT_N):
    """(T, Q, self_rows): the fp64 cosine of row j to query 0 (a vector outside the table)
    rises strictly with j; queries 1-15 are rows of the table."""
    rng = np.random.default_rng(2200 + rank)
    G = rng.standard_normal((n, rank)).astype(np.float32)
    q0 = rng.standard_normal((1, rank)).astype(np.float32)
    T = G[np.argsort(R.cosine(q0, G)[0], kind="stable")]
    rows = np.sort(rng.choice(n, 15, replace=False))
    Q = np.concatenate([q0, T[rows]])
    self_rows = np.concatenate([[-1], rows]).astype(np.int32)
    for a in (T, Q, self_rows):
        a.setflags(write=False)
    return T, Q, self_rows


@functools.lru_cache(maxsize=None)
def flood_table(rank, n=CUT_N, n_gauss=1):
    """(T, Q, posA, posB): Gaussian rows, 300 exact copies of a vector a at posA and 70 of b at
    posB (ascending, drawn over the whole range: irregular gaps), every third copy scaled by
    a power of two.  Q = [a, b, mid, n_gauss Gaussian rows of T], mid = g + lambda a with
    lambda bisected so that about 40 ordinary rows score above the flood."""
    rng = np.random.default_rng(3200 + rank + n)
    T = rng.standard_normal((n, rank)).astype(np.float32)
    a, b, g = rng.standard_normal((3, rank)).astype(np.float32)
    pos = rng.choice(n, N_FLOOD_A + N_FLOOD_B, replace=False)
    posA, posB = np.sort(pos[:N_FLOOD_A]), np.sort(pos[N_FLOOD_A:])
    for p, v in ((posA, a), (posB, b)):
        scale = np.ones(len(p), np.float32)
        scale[::3] = np.ldexp(np.float32(1), rng.integers(-8, 9, len(scale[::3]))).astype(np.float32)
        T[p] = v[None, :] * scale[:, None]
    plain = np.ones(n, bool)
    plain[pos] = False
    lo, hi = 0.0, 4.0
    for _ in range(40):
        lam = 0.5 * (lo + hi)
        mid = (g + np.float32(lam) * a).astype(np.float32)
        c = R.cosine(mid[None], T)[0]
        above = int((c[plain] > c[posA[0]]).sum())
        if above > 40:
            lo = lam
        else:
            hi = lam
    gauss = np.nonzero(plain)[0][np.linspace(5, plain.sum() - 5, n_gauss).astype(int)]
    Q = np.concatenate([a[None], b[None], mid[None], T[gauss]])
    self_rows = np.concatenate([[-1, -1, -1], gauss]).astype(np.int32)
    for x in (T, Q, posA, posB, self_rows):
        x.setflags(write=False)
    return T, Q, posA, posB, self_rows


def flood_allow(n, posA, posB):
    """Every third copy of either flood cleared."""
    allow = np.ones(n, bool)
    allow[posA[1::3]] = False
    allow[posB[1::3]] = False
    return allow


@functools.lru_cache(maxsize=None)
def negative_table(rank, n=CUT_N):
    """Componentwise positive queries against a componentwise negative table."""
    rng = np.random.default_rng(4200 + rank)
    T = -np.abs(rng.standard_normal((n, rank))).astype(np.float32) - np.float32(0.01)
    Q = np.abs(rng.standard_normal((4, rank))).astype(np.float32) + np.float32(0.01)
    T.setflags(write=False)
    Q.setflags(write=False)
    return T, Q


# ------------------------------------------------------------------ 4. under- and overflow
EXTREME_EXP = (-70, -76, 70)      # norms whose fp32 |t|^2 is subnormal, subnormal or 0, Inf


@functools.lru_cache(maxsize=None)
def extreme_table(rank, n=1000):
    """(T, rows, extreme): a Gaussian table whose rows n-6 .. n-1 are, for each norm of
    EXTREME_EXP, an exact power-of-two multiple of query 0's row (true cosine 1) and a row
    of its own direction; rows: the query rows (self-excluded)."""
    rng = np.random.default_rng(5200 + rank)
    T = rng.standard_normal((n, rank)).astype(np.float32)
    rows = np.array([7, 100, 101, 102, 103], np.int32)
    extreme = np.arange(n - 6, n)
    for i, e in enumerate(EXTREME_EXP):
        for j, src in enumerate((T[rows[0]], rng.standard_normal(rank).astype(np.float32))):
            shift = e - int(np.round(np.log2(np.linalg.norm(src.astype(np.float64)))))
            T[extreme[2 * i + j]] = np.ldexp(src, shift)
    T.setflags(write=False)
    return T, rows, extreme


# ================================================================== the pins
def test_grid_covers_every_value():
    cases = grid_cases()
    assert len(cases) == len(set(cases)) == 2 * len(RANKS)
    assert {(r, t) for r, t, _ in cases} == {(r, t) for r in RANKS for t in TOPS}
    assert {(sweep_of(r), q) for r, _, q in cases} == {(c, q) for c in SWEEPS for q in NQS}
    for cls, ranks in SWEEPS.items():
        assert all(sweep_of(r) == cls for r in ranks)
        lpr, c = cls
        tails = {(r - 1) % 4 for r in ranks}            # last live column of the float4 mask:
        assert tails >= {0, 2, 3}                       # x only, xyz, full (xy: rank 10 of
        assert max(ranks) == 4 * lpr * c                # test_gpu_similar.test_parity_grid)
    assert [sweep_of(r) for r in (16, 17, 32, 33, 64, 65)] == \
        [(4, 1), (8, 1), (8, 1), (16, 1), (16, 1), (16, 2)]
    assert GRID_N // GRID_SLICES + 1 == 143 and 143 % 16 != 0
    assert max(NQS) == N_QROWS
    for rank in RANKS:
        rows = grid_queries(rank)
        assert len(rows) == len(set(rows.tolist())) == N_QROWS and rows.max() < 400


def test_grid_planted_rows():
    for rank in RANKS:
        T = grid_table(rank)
        ok = R.has_direction(T)
        assert list(np.nonzero(~ok)[0]) == [ZERO, NAN, INF]
        assert np.isnan(T[NAN, :rank]).sum() == 1 and np.isinf(T[INF, 0])
        S = R.cosine(T[[10, 30, 50]], T)
        assert S[0, 20] == pytest.approx(1, abs=1e-12) and S[1, 40] == pytest.approx(1, abs=1e-7)
        assert S[2, 60] == pytest.approx(-1, abs=1e-12)


def test_tie_window_and_fp32_emulation_shares():
    """Why the GPU file's 0.1 % cap means something: ties within the checker's window are
    several times more frequent than the cap, an honest fp32 evaluation is well below it."""
    near = pos256 = swapped = listed = 0
    for rank, top, n_q in grid_cases():
        if rank < 3:
            continue
        T = grid_table(rank)
        rows = grid_queries(rank)[:n_q]
        S, adm = R.cosine(T[rows], T), R.admissible(T[rows], T, rows)
        if top == 256:
            _, sc = R.neighbours(S, adm, top + 1)
            near += int((sc[:, :-1] - sc[:, 1:] <= 1e-5).sum())
            pos256 += sc[:, :-1].size
        idx32, _ = R.neighbours(cosine_fp32(T[rows], T).astype(np.float64), adm, top)
        e, m = excused(idx32, S, adm, top)
        swapped += e
        listed += m
    print(f"window share {near / pos256:.4%} of {pos256}; fp32 emulation {swapped} / {listed} "
          f"= {swapped / listed:.4%}")
    assert near / pos256 >= 0.003
    assert swapped / listed <= 0.0005


def test_cap_steps():
    assert [sim_cap(t) for t in (1, 63, 64, 65, 192, 193, 255, 256)] == \
        [128, 128, 128, 192, 256, 320, 320, 320]
    assert sim_cap(64) < sim_cap(65) and sim_cap(192) < sim_cap(193)
    assert {64, 65, 192, 193} <= set(RISING_TOPS)
    for t in RISING_TOPS + FLOOD_TOPS:
        assert sim_cap(t) - t >= 64 and sim_cap(t) % 64 == 0   # room for a 16-row tile, J whole


@pytest.mark.parametrize("rank", CUT_RANKS)
def test_rising_order_is_strict(rank):
    T, Q, self_rows = rising_table(rank)
    c = R.cosine(Q[:1], T)[0]
    assert (np.diff(c) > 0).all()
    assert len(Q) == 16 and self_rows[0] == -1 and len(set(self_rows[1:])) == 15
    np.testing.assert_array_equal(Q[1:], T[self_rows[1:]])
    # the reference list of query 0 is the table's tail, backwards
    idx, _ = R.neighbours(R.cosine(Q[:1], T), R.admissible(Q[:1], T), 256)
    np.testing.assert_array_equal(idx[0], np.arange(CUT_N - 1, CUT_N - 257, -1))


@pytest.mark.parametrize("n,n_gauss", [(CUT_N, 1), (5000, 14)])
@pytest.mark.parametrize("rank", CUT_RANKS)
def test_flood_positions(rank, n, n_gauss):
    T, Q, posA, posB, self_rows = flood_table(rank, n, n_gauss)
    assert len(posA) == N_FLOOD_A > 256 and len(posB) == N_FLOOD_B > 64
    assert not set(posA) & set(posB) and (np.diff(posA) > 0).all() and (np.diff(posB) > 0).all()
    for p in (posA, posB):
        gaps = np.diff(p)
        assert len(set(gaps.tolist())) > 10                       # irregular
        assert p[0] < n // 10 and p[-1] > n - n // 10             # the whole range
        unit = T[p] / np.abs(T[p]).max(axis=1, keepdims=True)
        assert (unit == unit[0]).all()                            # exact copies up to 2^e
        scaled = (np.abs(T[p]).max(axis=1) != np.abs(T[p[1]]).max())
        assert 0 < scaled.sum() <= len(p) // 3 + 1
    S = R.cosine(Q, T)
    assert np.ptp(S[0, posA]) == 0 and np.ptp(S[1, posB]) == 0    # fp64 scores tie exactly
    assert S[0, posA[0]] == pytest.approx(1, abs=1e-12)
    idx, _ = R.neighbours(S, R.admissible(Q, T, self_rows), 256)
    first = list(idx[2]).index(posA[0])                           # the mid-list query
    assert 16 <= first < 64, first
    np.testing.assert_array_equal(idx[2, first:256], posA[:256 - first])
    assert len(Q) == 3 + n_gauss and (self_rows[3:] >= 0).all()
    allow = flood_allow(n, posA, posB)
    assert (~allow).sum() == 100 + 23


@pytest.mark.parametrize("rank", CUT_RANKS)
def test_negative_table_and_extreme_rows(rank):
    T, Q = negative_table(rank)
    assert (R.cosine(Q, T) < 0).all()
    T, rows, extreme = extreme_table(rank)
    assert R.has_direction(T).all()                               # in fp64 every row has one
    norms = np.log2(np.linalg.norm(T[extreme].astype(np.float64), axis=1))
    np.testing.assert_allclose(norms, np.repeat(EXTREME_EXP, 2), atol=0.51)
    S = R.cosine(T[rows], T)
    np.testing.assert_allclose(S[0, extreme[::2]], 1, atol=1e-12)  # exact multiples of query 0
    with np.errstate(over="ignore", under="ignore"):
        ss = (T[extreme] * T[extreme]).sum(axis=1, dtype=np.float32)
    tiny = np.finfo(np.float32).tiny
    assert (ss[:4] < tiny).all() and np.isinf(ss[4:]).all()       # subnormal or 0, and Inf
