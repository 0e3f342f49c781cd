"""fp64 numpy reference of the cosine neighbour search (K12, als_similar) and the checker
the GPU tests share.

cosine(Q, T): the full cosine matrix in fp64, NaN where either vector has no direction
(zero norm, a NaN or an Inf).  admissible(...): which table rows a query may list — not
its own row (by index), allowed by the mask, and with a direction.  neighbours(...): stable
argsort(-S) over the admissible entries, padded to idx -1 / score -inf.  check(...): the
house rule of test_gpu_topk_filtered._check — an index may differ from the reference only
where the fp64 scores tie within 1e-5, scores are compared at rtol = atol = 1e-5.

The tolerance is derivable: the fp32 dot of k <= 128 terms errs by at most k 2^-24 ~ 7.6e-6
of |q||t| in the worst summation order (far less with a tree), the norms add ~1e-7.
"""
import numpy as np


def has_direction(M):
    """Rows of M that are finite and not all zero."""
    M = np.asarray(M, np.float64)
    return np.isfinite(M).all(axis=1) & (np.abs(M).sum(axis=1) > 0)


def cosine(Q, T):
    Q = np.asarray(Q, np.float64)
    T = np.asarray(T, np.float64)
    qok, tok = has_direction(Q), has_direction(T)
    Qz = np.where(qok[:, None], Q, 0.0)
    Tz = np.where(tok[:, None], T, 0.0)
    qn = np.sqrt((Qz * Qz).sum(axis=1))
    tn = np.sqrt((Tz * Tz).sum(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        S = (Qz @ Tz.T) / (qn[:, None] * tn[None, :])
    S[~qok, :] = np.nan
    S[:, ~tok] = np.nan
    return S


def admissible(Q, T, self_rows=None, allow=None):
    """bool [n_q, n]: table row j may be listed by query r."""
    n_q, n = len(Q), len(T)
    adm = np.ones((n_q, n), bool)
    adm &= has_direction(T)[None, :]
    adm &= has_direction(Q)[:, None]
    if allow is not None:
        adm &= np.asarray(allow, bool)[None, :]
    if self_rows is not None:
        for r, s in enumerate(np.asarray(self_rows, np.int64)):
            if 0 <= s < n:
                adm[r, s] = False
    return adm


def neighbours(S, adm, top):
    """(idx int64 [n_q, top], score f64 [n_q, top]): score descending, ties by ascending
    row (stable argsort), inadmissible and NaN entries never listed, open slots -1 / -inf."""
    Sm = np.where(adm & ~np.isnan(S), S, -np.inf)
    order = np.argsort(-Sm, axis=1, kind="stable")[:, :top]
    sc = np.take_along_axis(Sm, order, 1)
    idx = np.where(np.isneginf(sc), -1, order)
    if idx.shape[1] < top:
        pad = top - idx.shape[1]
        idx = np.pad(idx, ((0, 0), (0, pad)), constant_values=-1)
        sc = np.pad(sc, ((0, 0), (0, pad)), constant_values=-np.inf)
    return idx, sc


def check(idx, sc, S, adm, top):
    """idx / sc: the lists under test for the rows of S / adm."""
    idx, sc = np.asarray(idx), np.asarray(sc)
    assert idx.shape == sc.shape == (S.shape[0], top), (idx.shape, sc.shape, S.shape, top)
    ref_i, ref_s = neighbours(S, adm, top)
    for r in range(S.shape[0]):
        n = int((ref_i[r] >= 0).sum())
        assert (idx[r, n:] == -1).all() and np.isneginf(sc[r, n:]).all(), (r, n, idx[r], sc[r])
        got = idx[r, :n]
        assert (got >= 0).all() and len(set(got.tolist())) == n, (r, got)
        assert adm[r, got].all(), f"row {r}: inadmissible row listed: {got[~adm[r, got]]}"
        for p in np.nonzero(got != ref_i[r, :n])[0]:  # only where fp64 scores tie within 1e-5
            assert abs(S[r, got[p]] - ref_s[r, p]) <= 1e-5 * max(1, abs(ref_s[r, p])), (r, p)
        np.testing.assert_allclose(sc[r, :n], ref_s[r, :n], rtol=1e-5, atol=1e-5)
