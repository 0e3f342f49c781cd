"""fp64 numpy reference of the MMR re-ranking and the intra-list similarity (K14,
als_diversify / als_list_similarity) and the checkers the GPU tests share.

The contract is the one in include/als_hip.h.  Per row: a pool of m slots (idx, score); a
slot is live iff 0 <= idx < n_v and its score is finite; rel = (s - s_min) / (s_max - s_min)
over the live slots (1 for all when they are equal); unit vectors from an fp64 norm over
columns [0, k), the zero vector for a row with zero norm or a non-finite entry; step 0 picks
the largest rel, step t >= 1 the largest lam * rel - (1 - lam) * max cos to the picked,
ties to the lowest slot position.

mmr(...) follows that literally.  check_greedy(...) replays the picks of the code under test
instead of comparing whole lists: at each step it computes the fp64 value of every live
unpicked slot GIVEN the earlier picks under test, and asserts that the pick is such a slot
with a value within tol of the best, and that its score is the slot's, bit for bit.  One
near-tie can therefore not make the rest of a list "wrong", and no row is ever left out.

Why tol = 2e-5: the cosine of two fp32-stored unit vectors summed in fp32 in any order over
k <= 128 terms errs by at most about (k + 2) 2^-24 <= 7.8e-6 (far less in fp64); rel is exact
to fp64 rounding; each value therefore errs by at most (1 - lam) 7.8e-6 and the comparison of
two values by twice that.  The library takes lam as a float: for a lam that fp32 does not hold
exactly that moves a value by at most 2^-24 (|rel| + |cos|) <= 1.2e-7, inside the bound.
Derived, not measured; the same reasoning as the 1e-5 of similar_ref.py.  ILS is compared
with atol = 1e-5 by the same bound (a mean of cosines errs no more than one of them).
"""
import numpy as np

TOL = 2e-5
ILS_ATOL = 1e-5


def unit_rows(V, k):
    """fp64 unit vectors of V[:, :k]; zero rows where the norm is zero or an entry is not
    finite."""
    A = np.asarray(V, np.float64)[:, :k]
    ok = np.isfinite(A).all(axis=1)
    A = np.where(ok[:, None], A, 0.0)
    nrm = np.sqrt((A * A).sum(axis=1))
    ok &= nrm > 0
    return np.where(ok[:, None], A / np.where(ok, nrm, 1.0)[:, None], 0.0)


def live_slots(idx, sc, n_v):
    idx = np.asarray(idx, np.int64)
    return (idx >= 0) & (idx < n_v) & np.isfinite(np.asarray(sc, np.float64))


def relevance(sc, live):
    """rel of one row's slots (fp64; 0 in dead slots, which are never read)."""
    s = np.where(live, np.asarray(sc, np.float32).astype(np.float64), 0.0)
    if not live.any():
        return np.zeros_like(s)
    lo, hi = s[live].min(), s[live].max()
    if hi == lo:
        return np.ones_like(s)
    return np.where(live, (s - lo) / (hi - lo), 0.0)


def _mean_pairs(C):
    n = C.shape[0]
    if n < 2:
        return np.nan
    iu = np.triu_indices(n, 1)
    return float(C[iu].sum() / len(iu[0]))


def mmr(idx, sc, V, k, top, lam):
    """(out_idx int64 [n_q, top], out_score f32 [n_q, top], ils f64 [n_q], picked slots: a
    list of lists), the contract followed literally in fp64."""
    idx = np.asarray(idx, np.int64)
    sc = np.asarray(sc, np.float32)
    n_q, m = idx.shape
    n_v = len(V)
    Vn = unit_rows(V, k)
    out_i = np.full((n_q, top), -1, np.int64)
    out_s = np.full((n_q, top), -np.inf, np.float32)
    ils = np.full(n_q, np.nan)
    slots = []
    for r in range(n_q):
        live = live_slots(idx[r], sc[r], n_v)
        rel = relevance(sc[r], live)
        X = np.where(live[:, None], Vn[np.where(live, idx[r], 0)], 0.0)
        free = live.copy()
        mx = np.zeros(m)
        picked = []
        while len(picked) < top and free.any():
            val = rel.copy() if not picked else lam * rel - (1.0 - lam) * mx
            val[~free] = -np.inf
            j = int(np.argmax(val))             # the first of equal values: the lowest slot
            c = X @ X[j]
            mx = c if not picked else np.maximum(mx, c)
            picked.append(j)
            free[j] = False
        out_i[r, :len(picked)] = idx[r, picked]
        out_s[r, :len(picked)] = sc[r, picked]
        ils[r] = _mean_pairs(X[picked] @ X[picked].T)
        slots.append(picked)
    return out_i, out_s, ils, slots


def list_similarity(idx, V, k):
    """f64 [n_q]: mean cosine over the unordered pairs of the slots with 0 <= idx < n_v."""
    idx = np.asarray(idx, np.int64)
    Vn = unit_rows(V, k)
    out = np.full(idx.shape[0], np.nan)
    for r in range(idx.shape[0]):
        ok = (idx[r] >= 0) & (idx[r] < len(V))
        X = Vn[idx[r][ok]]
        out[r] = _mean_pairs(X @ X.T)
    return out


def check_greedy(pool_idx, pool_sc, V, k, lam, got_idx, got_sc, top, tol=TOL):
    """Replays the picks under test (see the module docstring).  Returns the fp64 ILS of
    the lists under test, f64 [n_q]."""
    pool_idx = np.asarray(pool_idx, np.int64)
    pool_sc = np.asarray(pool_sc, np.float32)
    got_idx = np.asarray(got_idx, np.int64)
    got_sc = np.asarray(got_sc, np.float32)
    n_q, m = pool_idx.shape
    assert got_idx.shape == got_sc.shape == (n_q, top), (got_idx.shape, got_sc.shape, n_q, top)
    n_v = len(V)
    Vn = unit_rows(V, k)
    ils = np.full(n_q, np.nan)
    for r in range(n_q):
        live = live_slots(pool_idx[r], pool_sc[r], n_v)
        want = min(top, int(live.sum()))
        assert (got_idx[r, want:] == -1).all() and np.isneginf(got_sc[r, want:]).all(), \
            (r, want, got_idx[r], got_sc[r])
        rel = relevance(pool_sc[r], live)
        X = np.where(live[:, None], Vn[np.where(live, pool_idx[r], 0)], 0.0)
        free = live.copy()
        mx = np.zeros(m)
        picked = []
        for t in range(want):
            val = rel.copy() if t == 0 else lam * rel - (1.0 - lam) * mx
            val[~free] = -np.inf
            best = val.max()
            # the slot under test: a free slot holding this index and these score bits whose
            # value is the largest such (duplicates of an index are separate candidates)
            match = free & (pool_idx[r] == got_idx[r, t]) & \
                (pool_sc[r].view(np.int32) == got_sc[r, t].view(np.int32))
            assert match.any(), f"row {r} step {t}: pick {got_idx[r, t]} / {got_sc[r, t]!r} " \
                                f"is no live unpicked slot with that score"
            j = int(np.argmax(np.where(match, val, -np.inf)))
            assert val[j] >= best - tol, \
                f"row {r} step {t}: picked value {val[j]!r} < best {best!r} - {tol}"
            c = X @ X[j]
            mx = c if t == 0 else np.maximum(mx, c)
            picked.append(j)
            free[j] = False
        ils[r] = _mean_pairs(X[picked] @ X[picked].T)
    return ils


def planted_clusters(rank=8, clusters=4, per=10, noise=1e-3, seed=0):
    """(V f32 [clusters * per, rank], user vector f32 [rank]): items of cluster c sit around
    the axis e_{c+1}; the user likes cluster 1 most, then 2, 3, 4."""
    rng = np.random.default_rng(seed)
    V = np.zeros((clusters * per, rank))
    for c in range(clusters):
        V[c * per:(c + 1) * per, c] = 1.0
    V += noise * rng.standard_normal(V.shape)
    u = np.zeros(rank)
    u[:clusters] = [1.0, 0.9, 0.8, 0.7][:clusters]
    return V.astype(np.float32), u.astype(np.float32)


def pool_of(u, V, k, pool):
    """The score-descending pool K5 would list for one user: (idx int32 [1, pool], score
    f32 [1, pool]), ties at lower rows first."""
    s = (np.asarray(V, np.float64)[:, :k] @ np.asarray(u, np.float64)[:k]).astype(np.float32)
    order = np.argsort(-s, kind="stable")[:pool]
    return order.astype(np.int32)[None, :], s[order][None, :]
