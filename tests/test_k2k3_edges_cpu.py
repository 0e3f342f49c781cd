"""CPU side of the K2/K3 edge grid (tests/test_gpu_edges_k2_k3.py): the generators, the
fp32 textbook yardstick and the reasons no grid row may reach the fp64 rescue, all without
a GPU.

The GPU file asserts `max GPU error <= 8 x max textbook error` per case; here the same
textbook errors are pinned to (0, 1.25e-5], so that bar is neither vacuous (a zero
yardstick) nor looser than the project's 1e-4."""
import numpy as np
import pytest

from oracle import als_oracle as O
from helpers import (K2K3_N_SRC, K2K3_REG, degree_rows, fp32_textbook_half_sweep, k2k3_grid_case,
                     k2k3_grid_degrees, k2k3_grid_refs, k2k3_special_rows, rel_row_errs)

CPU_RANKS = [1, 16, 33, 64, 65, 128]


# ---------------------------------------------------------------- degree_rows
@pytest.mark.parametrize("ratings", ["stars", "signed"])
def test_degree_rows_exact_degrees_distinct_ids(ratings):
    degrees = [1, 2, 31, 32, 33, 64, 65, 200, 1, 200]
    dst, src, r = degree_rows(degrees, 200, seed=4, ratings=ratings)
    assert dst.dtype == np.int32 and src.dtype == np.int32 and r.dtype == np.float32
    assert np.bincount(dst).tolist() == degrees + [200]
    for t in range(len(degrees) + 1):
        ids = src[dst == t]
        assert len(np.unique(ids)) == len(ids) and ids.min() >= 0 and ids.max() < 200
    assert np.array_equal(src[dst == len(degrees)], np.arange(200))  # the row rating everything
    assert np.all(np.diff(dst) >= 0)  # rows in order: CSR positions are input positions
    lo = 0.5 if ratings == "stars" else -2.0
    assert r.min() >= lo and r.max() <= lo + 4.5 and np.all(r * 2 == np.round(r * 2))


def test_degree_rows_deterministic_per_seed():
    a = degree_rows([5, 40, 7], 64, seed=9)
    b = degree_rows([5, 40, 7], 64, seed=9)
    c = degree_rows([5, 40, 7], 64, seed=10)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[1], c[1])
    # the same degree twice gets different source ids
    d, s, _ = degree_rows([40, 40], 64, seed=9)
    assert not np.array_equal(s[d == 0], s[d == 1])


def test_degree_rows_signed_has_all_three_signs():
    _, _, r = degree_rows([64, 65, 129], 256, seed=2, ratings="signed")
    assert (r > 0).any() and (r < 0).any() and (r == 0).any()
    _, _, rs = degree_rows([64, 65, 129], 256, seed=2, ratings="stars")
    assert np.array_equal(rs - np.float32(2.5), r)


def test_degree_rows_rejects_bad_input():
    with pytest.raises(ValueError):
        degree_rows([0, 3], 10, seed=0)
    with pytest.raises(ValueError):
        degree_rows([11], 10, seed=0)
    with pytest.raises(ValueError):
        degree_rows([3], 10, seed=0, ratings="counts")


@pytest.mark.parametrize("rank", [1, 64])
def test_grid_degrees(rank):
    deg = k2k3_grid_degrees(rank)
    assert min(deg) >= 1 and max(deg) == K2K3_N_SRC
    for d in (1, 33, 129, 513, 1024, rank, rank + 1):
        assert deg.count(d) >= 3
    c = k2k3_grid_case(rank, False)
    assert np.diff(c["indptr"]).tolist() == deg + [K2K3_N_SRC]
    assert np.allclose(np.linalg.norm(c["Y"].astype(np.float64), axis=1), 1.0, atol=1e-6)


# ---------------------------------------------------------------- the yardstick
def test_textbook_is_fp32_and_ordered():
    """One row by hand: the Gram summed rating by rating in fp32 differs from the fp64 sum
    rounded once, and the result is float32 all the way."""
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((50, 5)).astype(np.float32)
    indptr, idx = np.array([0, 50]), np.arange(50, dtype=np.int32)
    r = rng.integers(1, 11, 50).astype(np.float32) / 2
    X = fp32_textbook_half_sweep(indptr, idx, r, Y, 0.1)
    assert X.dtype == np.float32 and X.shape == (1, 5)
    A = np.zeros((5, 5), np.float32)
    b = np.zeros(5, np.float32)
    for j in range(50):
        A += np.outer(Y[j], Y[j])
        b += r[j] * Y[j]
    A[np.arange(5), np.arange(5)] += np.float32(0.1) * np.float32(50)
    x = np.linalg.solve(A.astype(np.float64), b.astype(np.float64))
    assert np.abs(X[0] - x).max() <= 1e-5 * np.abs(x).max()
    e = rel_row_errs(X, O.half_sweep(indptr, idx, r, Y, 0.1))
    assert 0 < e[0] <= 1e-5


@pytest.mark.parametrize("mode", ["explicit", "alpha4", "alpha40"])
@pytest.mark.parametrize("rank", CPU_RANKS)
def test_textbook_error_on_the_grid(rank, mode):
    """8 x the yardstick stays within the project's 1e-4 and above 0 on the §1 inputs."""
    implicit = mode != "explicit"
    alpha = {"explicit": 1.0, "alpha4": 4.0, "alpha40": 40.0}[mode]
    X, e = k2k3_grid_refs(rank, implicit, alpha)
    assert np.isfinite(X).all() and (np.linalg.norm(X, axis=1) > 0).mean() > 0.95
    assert 0 < e.max() <= 1.25e-5, e.max()
    assert 8 * e.max() <= 1e-4


# ---------------------------------------------------------------- the rescue criteria
def _split_exponent(m):
    """The Gram's power-of-two scale: the launch's largest operand lands in [2^14, 2^15)."""
    return 14 - int(np.floor(np.log2(m)))


def rescue_candidates(indptr, indices, vals, Y, reg, rank):
    """Explicit rows that DESIGN's a-priori rescue tests would flag, evaluated in fp64:
    the split window (largest scaled Gram diagonal entry < n T^2, or the row's largest
    scaled |rating| in (0, T), T = 2^-4) and the rank-deficiency test (4 n <= k and
    trace(G) > 63 lambda n)."""
    Y = np.asarray(Y, np.float64)
    T = 2.0 ** -4
    sy = 2.0 ** _split_exponent(np.abs(Y).max())
    sr = 2.0 ** _split_exponent(np.abs(vals).max())
    flagged = []
    for row in range(len(indptr) - 1):
        p0, p1 = int(indptr[row]), int(indptr[row + 1])
        n = p1 - p0
        diag = ((sy * Y[indices[p0:p1]]) ** 2).sum(0)
        rmax = sr * np.abs(vals[p0:p1]).max()
        window = (0 < diag.max() < n * T * T) or (0 < rmax < T)
        rank_def = 4 * n <= rank and diag.sum() / sy ** 2 > 63 * reg * n
        if window or rank_def:
            flagged.append(row)
    return flagged


def pivot_spread(A, k):
    """max / min LDL^T pivot of A (fp64) with the dims in the solve kernels' order (block c
    holds dims m CN + c, m = 0..15): what the a-posteriori rescue test compares with
    kCondMax = 32 (8 for the implicit rows of the rank 65-128 kernel)."""
    cn = 1 if k <= 16 else 2 if k <= 32 else 4 if k <= 64 else 8
    perm = [m * cn + c for c in range(cn) for m in range(16) if m * cn + c < k]
    d = np.diag(np.linalg.cholesky(A[np.ix_(perm, perm)])) ** 2
    return d.max() / d.min()


@pytest.mark.parametrize("mode", ["explicit", "alpha4", "alpha40"])
@pytest.mark.parametrize("rank", CPU_RANKS)
def test_grid_pivot_spreads_are_far_from_the_rescue_limit(rank, mode):
    """The third rescue test looks at the fp32 pivots.  In fp64 an explicit system's pivots
    spread by at most its condition number, <= 1 + 1 / lambda = 11 for unit-norm rows
    (reached by the 1-rating rows), against a limit of 32; the implicit ones by less than
    4 against 8: rounding cannot carry a row past its limit."""
    implicit = mode != "explicit"
    alpha = {"explicit": 1.0, "alpha4": 4.0, "alpha40": 40.0}[mode]
    c = k2k3_grid_case(rank, implicit)
    A, _, ne = O.normal_equations(c["indptr"], c["indices"], c["vals"], c["Y"], implicit, alpha)
    if implicit:
        A += O.yty(c["Y"])[None]
    A[:, np.arange(rank), np.arange(rank)] += K2K3_REG * ne[:, None]
    assert max(pivot_spread(a, rank) for a in A) < (4.0 if implicit else 11.5)


@pytest.mark.parametrize("rank", CPU_RANKS)
def test_no_grid_row_qualifies_for_the_rescue(rank):
    """Unit-norm source factors at regParam 0.1: trace(G) / (lambda n) = 10 < 63 and every
    operand sits within 2^-4 of the launch maximum — the grid measures the fp32 kernels."""
    c = k2k3_grid_case(rank, False)
    assert rescue_candidates(c["indptr"], c["indices"], c["vals"], c["Y"], K2K3_REG, rank) == []
    # and the criteria do see what they are meant to: tiny factor rows, a tiny rating,
    # a very short row at a small regParam
    Y = c["Y"].copy()
    row = 5 * len(c["degrees"]) // 7
    p0, p1 = c["indptr"][row], c["indptr"][row + 1]
    Y[c["indices"][p0:p1]] *= 1e-7
    assert row in rescue_candidates(c["indptr"], c["indices"], c["vals"], Y, K2K3_REG, rank)
    v = c["vals"].copy()
    v[c["indptr"][0]:c["indptr"][1]] = 1e-6
    assert 0 in rescue_candidates(c["indptr"], c["indices"], v, c["Y"], K2K3_REG, rank)
    if rank >= 4:
        assert 0 in rescue_candidates(c["indptr"], c["indices"], c["vals"], c["Y"], 1e-3, rank)


# ---------------------------------------------------------------- §2: special implicit rows
@pytest.mark.parametrize("rank", [16, 32, 64, 128])
def test_special_implicit_rows_on_the_oracle(rank):
    """Rows with no positive rating have a zero right-hand side and no lambda n term: the
    system is YtY + sum c y y^T, positive definite through YtY alone (n_src >= 4 rank),
    and the oracle's solution is exactly zero."""
    s = k2k3_special_rows(rank)
    assert K2K3_N_SRC >= 4 * rank
    G = O.yty(s["Y"])
    ev = np.linalg.eigvalsh(G)
    assert ev[0] > 0 and ev[-1] / ev[0] < 8
    np.linalg.cholesky(G)
    A, b, ne = O.normal_equations(s["indptr"], s["indices"], s["vals"], s["Y"], True, 4.0)
    np.linalg.cholesky(A + G[None])  # with numExplicits = 0 nothing else is added
    X = O.half_sweep(s["indptr"], s["indices"], s["vals"], s["Y"], K2K3_REG, True, 4.0)
    deg = np.diff(s["indptr"])
    for kind, rows in s["rows"].items():
        assert deg[rows].tolist() == list(s["degrees"])
        for row in rows:
            v = s["vals"][s["indptr"][row]:s["indptr"][row + 1]]
            if kind == "nonpositive":
                assert (v <= 0).all() and (v < 0).any() and ne[row] == 0
                assert np.all(X[row] == 0) and np.all(b[row] == 0)
            elif kind == "zero":
                assert (v == 0).all() and ne[row] == 0 and np.all(A[row] == 0)
                assert np.all(X[row] == 0)
            else:  # one positive rating, the row's last
                assert v[-1] > 0 and (v[:-1] <= 0).all() and ne[row] == 1
                assert np.linalg.norm(X[row]) > 0
