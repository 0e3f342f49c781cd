"""Seeded synthetic rating sets for tests (planted low-rank model, SURVEY §8d shape rules)."""
import numpy as np


def planted(n_users, n_items, density=0.05, k_true=8, seed=0, heavy_items=(), heavy_users=(),
            half_stars=True, dup=0, id_gap=1):
    """Return (users, items, ratings) int32/int32/float32 with optional heavy rows,
    duplicate (u,i) pairs (`dup` extra copies) and sparse ids (ids multiplied by id_gap)."""
    rng = np.random.default_rng(seed)
    mask = rng.random((n_users, n_items)) < density
    for i in heavy_items:
        mask[:, i] = True
    for u in heavy_users:
        mask[u, :] = True
    mask[np.arange(n_users), rng.integers(0, n_items, n_users)] = True  # every user rates
    mask[rng.integers(0, n_users, n_items), np.arange(n_items)] = True  # every item rated
    u, i = np.nonzero(mask)
    perm = rng.permutation(len(u))
    u, i = u[perm], i[perm]
    us = rng.normal(0, 0.35, (n_users, k_true))
    vs = rng.normal(0, 0.35, (n_items, k_true))
    r = 3.6 + (us[u] * vs[i]).sum(1) + rng.normal(0, 0.8, len(u))
    r = np.round(r * 2) / 2 if half_stars else np.round(r)
    r = np.clip(r, 0.5 if half_stars else 1, 5)
    if dup:
        sel = rng.integers(0, len(u), dup)
        u = np.concatenate([u, u[sel]])
        i = np.concatenate([i, i[sel]])
        r = np.concatenate([r, np.clip(r[sel] - 1, 0.5, 5)])
    return (u * id_gap).astype(np.int32), (i * id_gap).astype(np.int32), r.astype(np.float32)


def degree_rows(degrees, n_src, seed, ratings="stars"):
    """Destination rows with exactly the given degrees (>= 1; distinct source ids each,
    `rng.choice`) plus one row rating every source id, so both id maps are dense and
    destination row t has degrees[t] ratings in the order returned here (the CSR build is
    a stable sort).  "stars": planted half-star ratings in [0.5, 5]; "signed": the same
    minus 2.5 (implicit preferences: positive, negative and exactly zero all occur).
    Returns (dst, src, r) int32 / int32 / float32."""
    if ratings not in ("stars", "signed"):
        raise ValueError(f"ratings must be 'stars' or 'signed', got {ratings!r}")
    degrees = [int(d) for d in degrees]
    if min(degrees) < 1 or max(degrees) > n_src:
        raise ValueError("degrees must lie in [1, n_src]")
    rng = np.random.default_rng(seed)
    dst = [np.full(d, t) for t, d in enumerate(degrees)]
    src = [rng.choice(n_src, d, replace=False) for d in degrees]
    dst.append(np.full(n_src, len(degrees)))
    src.append(np.arange(n_src))
    dst = np.concatenate(dst).astype(np.int32)
    src = np.concatenate(src).astype(np.int32)
    df = rng.normal(0, 0.35, (len(degrees) + 1, 8))
    sf = rng.normal(0, 0.35, (n_src, 8))
    r = np.clip(np.round((3.6 + (df[dst] * sf[src]).sum(1) + rng.normal(0, 0.8, len(dst))) * 2) / 2,
                0.5, 5)
    if ratings == "signed":
        r = r - 2.5
    return dst, src, r.astype(np.float32)


def fp32_textbook_half_sweep(indptr, indices, vals, Y, reg, implicit=False, alpha=1.0, yty=None):
    """computeFactors in textbook fp32 (the yardstick of DESIGN §2): per destination row
    the normal equations accumulated one rating at a time with every product and sum in
    np.float32 (NormalEquation.add: explicit ata += y y^T, atb += r y; implicit
    c1 = alpha |r|, ata += c1 y y^T, atb += (1 + c1) y if r > 0, numExplicits = ratings
    > 0, ata starting from YtY), ata_ii += regParam * numExplicits, LAPACK spotrf
    (np.linalg.cholesky of a float32 matrix) and two fp32 triangular solves.
    yty: [k, k] (implicit; rounded to fp32).  Returns X [n, k] float32."""
    f32 = np.float32
    Y = np.asarray(Y, f32)
    vals = np.asarray(vals, f32)
    n, k = len(indptr) - 1, Y.shape[1]
    X = np.zeros((n, k), f32)
    G0 = np.asarray(yty, np.float64).astype(f32) if implicit else np.zeros((k, k), f32)
    tmp = np.empty((k, k), f32)
    dg = np.arange(k)
    for row in range(n):
        A = G0.copy()
        b = np.zeros(k, f32)
        n_exp = 0
        for p in range(int(indptr[row]), int(indptr[row + 1])):
            y = Y[indices[p]]
            r = vals[p]
            if implicit:
                c1 = f32(alpha) * np.abs(r)
                np.multiply((c1 * y)[:, None], y[None, :], out=tmp)
                if r > 0:
                    b += (f32(1) + c1) * y
                    n_exp += 1
            else:
                np.multiply(y[:, None], y[None, :], out=tmp)
                b += r * y
                n_exp += 1
            A += tmp
        A[dg, dg] += f32(reg) * f32(n_exp)
        L = np.linalg.cholesky(A)
        assert L.dtype == f32
        z = np.zeros(k, f32)
        for i in range(k):  # L z = b
            z[i] = (b[i] - np.dot(L[i, :i], z[:i])) / L[i, i]
        x = np.zeros(k, f32)
        for i in range(k - 1, -1, -1):  # L^T x = z
            x[i] = (z[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
        X[row] = x
    return X


# The K2/K3 edge grid (test_gpu_edges_k2_k3.py, test_k2k3_edges_cpu.py): task lengths around
# every 32-rating MFMA step, 64-rating staging block and 128 / 512-rating task boundary.
K2K3_DEGREES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 63, 64, 65, 95, 96, 97, 127, 128,
                129, 159, 160, 161, 191, 192, 193, 255, 256, 257, 287, 288, 289, 383, 384, 385,
                511, 512, 513, 769, 1024)
K2K3_RANKS = (1, 3, 15, 16, 17, 31, 32, 33, 47, 63, 64, 65, 97, 127, 128)
K2K3_N_SRC = 1024
K2K3_REG = 0.1
K2K3_REPEATS = 3


def k2k3_grid_degrees(rank):
    """Every grid degree K2K3_REPEATS times (different source ids), with rank - 1, rank,
    rank + 1 (a row has at least one rating)."""
    return [d for d in K2K3_DEGREES + (rank - 1, rank, rank + 1) if d >= 1] * K2K3_REPEATS


def unit_source_factors(n, k, seed):
    """Seeded unit-norm Gaussian rows, fp32 (Spark's ALS.initialize shape)."""
    x = np.random.default_rng(seed).standard_normal((n, k)).astype(np.float32)
    return (x / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)


_K2K3_CASES = {}


def k2k3_grid_case(rank, implicit):
    """The §1 inputs of one rank, shared (and left unchanged) by every test that needs
    them: (dst, src, r) of degree_rows, the destination side's CSR, unit-norm source
    factors Y.  The chunk, the dual switch and alpha do not change them."""
    key = (rank, bool(implicit))
    if key not in _K2K3_CASES:
        from oracle import als_oracle as O
        degrees = k2k3_grid_degrees(rank)
        dst, src, r = degree_rows(degrees, K2K3_N_SRC, seed=rank,
                                  ratings="signed" if implicit else "stars")
        indptr, indices, vals = O.csr_build(dst, src, r, len(degrees) + 1)
        Y = unit_source_factors(K2K3_N_SRC, rank, seed=1000 + rank)
        _K2K3_CASES[key] = dict(degrees=degrees, dst=dst, src=src, r=r, indptr=indptr,
                                indices=indices, vals=vals, Y=Y)
    return _K2K3_CASES[key]


_K2K3_REFS = {}


def k2k3_grid_refs(rank, implicit, alpha=1.0):
    """(fp64 oracle X, per-row relative errors of the fp32 textbook solve against it) on
    the §1 inputs, computed once per (rank, mode)."""
    key = (rank, bool(implicit), float(alpha) if implicit else 1.0)
    if key not in _K2K3_REFS:
        from oracle import als_oracle as O
        c = k2k3_grid_case(rank, implicit)
        a = (c["indptr"], c["indices"], c["vals"], c["Y"], K2K3_REG, implicit, alpha)
        X = O.half_sweep(*a)
        Xt = fp32_textbook_half_sweep(*a, yty=O.yty(c["Y"]) if implicit else None)
        _K2K3_REFS[key] = (X, rel_row_errs(Xt, X))
    return _K2K3_REFS[key]


K2K3_SPECIAL_DEGREES = (1, 32, 33, 64, 65, 129)
_K2K3_SPECIAL = {}


def k2k3_special_rows(rank):
    """Implicit rows that random data meets only by chance, one per degree of
    K2K3_SPECIAL_DEGREES and kind: "nonpositive" (every rating <= 0: numExplicits = 0, a
    zero right-hand side), "zero" (every rating exactly 0: confidence 0 as well) and
    "last_positive" (one rating > 0, in the row's last position — alone in its staging
    block at 65 and 129 ratings), among ordinary signed rows.  rows[kind][j] is the row of
    degree K2K3_SPECIAL_DEGREES[j]."""
    if rank not in _K2K3_SPECIAL:
        from oracle import als_oracle as O
        kinds = ("nonpositive", "zero", "last_positive", "ordinary")
        degrees = list(K2K3_SPECIAL_DEGREES) * len(kinds)
        dst, src, r = degree_rows(degrees, K2K3_N_SRC, seed=2000 + rank, ratings="signed")
        nd = len(K2K3_SPECIAL_DEGREES)
        rows = {kind: list(range(j * nd, (j + 1) * nd)) for j, kind in enumerate(kinds)}
        for row in rows["nonpositive"] + rows["last_positive"]:
            sel = np.nonzero(dst == row)[0]
            r[sel] = -np.abs(r[sel])
            r[sel[0]] = -1.5
        for row in rows["zero"]:
            r[dst == row] = 0.0
        for row in rows["last_positive"]:
            r[np.nonzero(dst == row)[0][-1]] = 2.0
        del rows["ordinary"]
        indptr, indices, vals = O.csr_build(dst, src, r, len(degrees) + 1)
        Y = unit_source_factors(K2K3_N_SRC, rank, seed=3000 + rank)
        _K2K3_SPECIAL[rank] = dict(degrees=K2K3_SPECIAL_DEGREES, rows=rows, dst=dst, src=src, r=r,
                                   indptr=indptr, indices=indices, vals=vals, Y=Y)
    return _K2K3_SPECIAL[rank]


def rel_row_err(x, ref):
    x = np.asarray(x, np.float64)
    ref = np.asarray(ref, np.float64)
    num = np.linalg.norm(x - ref, axis=1)
    den = np.maximum(np.linalg.norm(ref, axis=1), 1e-6)
    return float((num / den).max())


def row_len_buckets(indptr, err_rows, edges=(32, 128, 512, 2048)):
    """Max per-row relative error bucketed by row length (ratings per row):
    {"<=32": e, "33-128": e, ..., ">2048": e} (">2048" = heavy rows, chunked)."""
    deg = np.diff(np.asarray(indptr))
    lo = 0
    out = {}
    for hi in list(edges) + [None]:
        sel = deg > lo if hi is None else (deg > lo) & (deg <= hi)
        name = f">{lo}" if hi is None else (f"<={hi}" if lo == 0 else f"{lo + 1}-{hi}")
        out[name] = {"rows": int(sel.sum()), "max_rel_err": float(err_rows[sel].max()) if sel.any()
                     else None}
        lo = hi if hi is not None else lo
    return out


def rel_row_errs(x, ref):
    """Per-row ||x - ref|| / ||ref|| (vector)."""
    x = np.asarray(x, np.float64)
    ref = np.asarray(ref, np.float64)
    return np.linalg.norm(x - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-6)


def report(name, value):
    """Append a measured error to $ALS_TEST_REPORT (JSON lines) when set."""
    import json
    import os
    path = os.environ.get("ALS_TEST_REPORT")
    if path:
        with open(path, "a") as f:
            v = value if isinstance(value, (dict, list)) else float(value)
            f.write(json.dumps({"test": name, "value": v}) + "\n")


def oracle_train_c(users, items, ratings, rank, iterations, reg, U0, implicit=False, alpha=1.0):
    """ALS.train restated (oracle.als_oracle's loop) with the C half-sweeps
    (oracle/als_oracle.c, OpenMP) for the larger parity cases.
    Returns (U, V, umap, imap, uids, iids)."""
    from oracle import als_oracle as O
    from oracle import c_oracle as C
    users = np.asarray(users, np.int64)
    items = np.asarray(items, np.int64)
    ratings = np.asarray(ratings, np.float32)
    umap, uids = O.index_build(users, int(users.max()) + 1)
    imap, iids = O.index_build(items, int(items.max()) + 1)
    ip = O.csr_build(imap[items], umap[users], ratings, len(iids))
    up = O.csr_build(umap[users], imap[items], ratings, len(uids))
    U = np.asarray(U0, np.float32)
    V = np.zeros((len(iids), rank), np.float32)
    for _ in range(iterations):
        V, st = C.half_sweep(*ip, U, reg, implicit=implicit, alpha=alpha)
        assert not st.any()
        U, st = C.half_sweep(*up, V, reg, implicit=implicit, alpha=alpha)
        assert not st.any()
    return U, V, umap, imap, uids, iids


# ---------------------------------------------------------------- K5 checks and the row-group cases
def topk_check(Q, Vm, idx, sc, top, tol=1e-5):
    """idx/sc vs the fp64 oracle: identical except where fp64 scores tie within tol."""
    from oracle import als_oracle as O
    ref_i, ref_s = O.topk(Q, Vm, top)
    S = Q.astype(np.float64) @ Vm.astype(np.float64).T
    for row in range(Q.shape[0]):
        if not np.array_equal(idx[row], ref_i[row]):
            bad = np.nonzero(idx[row] != ref_i[row])[0]
            for p_ in bad:
                assert abs(S[row, idx[row, p_]] - ref_s[row, p_]) <= tol * max(1, abs(ref_s[row, p_])), \
                    (row, p_, idx[row, p_], ref_i[row, p_])
        np.testing.assert_allclose(sc[row], ref_s[row], rtol=1e-5, atol=1e-5)
    return ref_i, ref_s


def topk_ref_ranking(S, adm, top):
    """The reference lists of fp64 scores S under the admissibility mask adm: inadmissible
    and NaN entries out, ranked by (score descending, index ascending), open slots
    -1 / -inf."""
    Sm = np.where(adm & ~np.isnan(S), S, -np.inf)
    order = np.argsort(-Sm, axis=1, kind="stable")[:, :top]  # ties: lower index first
    sc = np.take_along_axis(Sm, order, 1)
    idx = np.where(np.isneginf(sc), -1, order)
    if idx.shape[1] < top:
        pad = top - idx.shape[1]
        idx = np.pad(idx, ((0, 0), (0, pad)), constant_values=-1)
        sc = np.pad(sc, ((0, 0), (0, pad)), constant_values=-np.inf)
    return idx, sc


def topk_ranking_check(idx, sc, S, adm, top, rows=None, skip=None):
    """idx / sc: the kernel's lists of the rows of S / adm (all rows, or `rows` of them).
    Returns the number of positions whose index differs from the reference's (each one
    excused by the 1e-5 tie rule, or the check has failed); positions where both indices
    are V rows of `skip` (bool [n_v]) are checked alike but not counted."""
    ref_i, ref_s = topk_ref_ranking(S, adm, top)
    excused = 0
    for r in range(S.shape[0]):
        n = int((ref_i[r] >= 0).sum())
        assert (idx[r, n:] == -1).all() and np.isneginf(sc[r, n:]).all(), (r, n, idx[r], sc[r])
        got = idx[r, :n]
        assert (got >= 0).all() and len(set(got.tolist())) == n, (r, got)
        assert adm[r, got].all(), f"row {r}: inadmissible row listed: {got[~adm[r, got]]}"
        for p in np.nonzero(got != ref_i[r, :n])[0]:  # only where fp64 scores tie within 1e-5
            assert abs(S[r, got[p]] - ref_s[r, p]) <= 1e-5 * max(1, abs(ref_s[r, p])), (r, p)
            excused += not (skip is not None and skip[got[p]] and skip[ref_i[r, p]])
        np.testing.assert_allclose(sc[r, :n], ref_s[r, :n], rtol=1e-5, atol=1e-5)
    return excused


def topk_sample_check(idx, sc, S, top, adm=None, skip=None):
    """topk_ranking_check on whole arrays (the same assertions, no loop over the rows), for
    the samples of test_gpu_topk_row_groups.py.  Returns {"positions": listed positions of
    the reference, "excused": those whose index differs from the reference's under the
    1e-5 tie rule (outside `skip`, as above), "max_score_err": the largest
    |score - ref| / max(1, |ref|)}."""
    n_r, n_v = S.shape
    if adm is None:
        adm = np.ones(S.shape, bool)
    ref_i, ref_s = topk_ref_ranking(S, adm, top)
    real = ref_i >= 0
    assert (idx[~real] == -1).all() and np.isneginf(sc[~real]).all(), \
        np.nonzero((~real & ((idx != -1) | ~np.isneginf(sc))).any(1))[0][:10]
    assert (idx[real] >= 0).all() and (idx[real] < n_v).all(), \
        np.nonzero((real & ((idx < 0) | (idx >= n_v))).any(1))[0][:10]
    # distinct per row (open slots get distinct negative stand-ins)
    srt = np.sort(np.where(real, idx, -1 - np.arange(top)[None, :]), axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), np.nonzero((srt[:, 1:] == srt[:, :-1]).any(1))[0][:10]
    got = np.where(real, idx, 0).astype(np.int64)
    rr = np.arange(n_r)[:, None]
    assert adm[rr, got][real].all(), "an inadmissible row is listed"
    bad = real & (idx != ref_i)
    refs = np.where(real, ref_s, 0.0)
    scale = np.maximum(1.0, np.abs(refs))
    off = np.abs(S[rr, got] - refs)
    assert (off[bad] <= 1e-5 * scale[bad]).all(), \
        [(int(r), int(p), int(idx[r, p]), int(ref_i[r, p])) for r, p in
         zip(*np.nonzero(bad & (off > 1e-5 * scale)))][:10]
    np.testing.assert_allclose(sc[real], ref_s[real], rtol=1e-5, atol=1e-5)
    if skip is not None:
        bad &= ~(skip[got] & skip[np.where(real, ref_i, 0)])
    err = np.abs(np.where(real, sc, 0.0).astype(np.float64) - refs) / scale
    return {"positions": int(real.sum()), "excused": int(bad.sum()),
            "max_score_err": float(err.max()) if err.size else 0.0}


# The two-row-group cases of K5 (test_gpu_topk_row_groups.py, test_topk_row_groups_cpu.py).
# csrc/topk.hip's topk_split_rg takes two row groups (256 query rows per workgroup) for
# register lists and key logs from kTkRg2MinRows = 262,144 query rows; a key-log launch
# covers kTkLogBlocks = 512 blocks, 131,072 rows at two groups.
K5RG_MIN_ROWS = 262144
K5RG_SLICE_ROWS = 131072
K5RG_NQ = K5RG_MIN_ROWS + 130   # 1,025 blocks; the last: group 0 full, 2 rows of group 1
K5RG_NV = 1159                  # 3 x 384 + 7 = 6 x 192 + 7
K5RG_RANKS = (24, 40, 100)      # NK = 1, 2, 4
K5RG_TOPS = (8, 11, 16, 17, 64, 99, 128)  # TOPR 8 / 12 / 16 / 32 / 64 / 100 / 128
K5RG_FILTERED = tuple((k, t) for k in (40, 100) for t in (11, 17, 99))
K5RG_SPLIT = K5RG_SLICE_ROWS + 65   # the one-group calls: rows [0, SPLIT) and [SPLIT, n_q)
K5RG_BIG_ROWS = (0, K5RG_SPLIT)     # Q[row, 0] = K5RG_BIG: max |Q| of the call and of each half
K5RG_BIG = 6.0
K5RG_ZERO_ROWS = (200, 300, K5RG_SLICE_ROWS + 130, K5RG_NQ - 1)  # 200: group 1, 300: group 0
K5RG_TIE = (10, 1100)               # Vm[1100] = Vm[10]
K5RG_COPIES = 300
K5RG_EXCUSED_CAP = 0.005            # share of sampled positions the tie rule may excuse
K5RG_WINDOW_CAP = 0.0015            # ... and what random data of these shapes can offer it

_K5RG_ITEMS = {}


def k5rg_items(rank):
    """(Vm [K5RG_NV, rank] float32, copies): N(0, 1) rows times uniform(0.2, 2.0), the
    exact-tie pair K5RG_TIE, and K5RG_COPIES exact copies of one strong row (3 x a N(0, 1)
    row) at the sorted indices `copies`, scattered over the index range."""
    if rank not in _K5RG_ITEMS:
        rng = np.random.default_rng(5000 + rank)
        Vm = rng.standard_normal((K5RG_NV, rank)).astype(np.float32)
        Vm *= rng.uniform(0.2, 2.0, (K5RG_NV, 1)).astype(np.float32)
        lo, hi = K5RG_TIE
        ends = [3, K5RG_NV - 2]  # one in the first tile, one in the ragged last tile
        free = np.setdiff1d(np.arange(K5RG_NV), [lo, hi] + ends)
        copies = np.sort(np.concatenate([ends, rng.choice(free, K5RG_COPIES - 2, replace=False)]))
        Vm[copies] = 3.0 * rng.standard_normal(rank).astype(np.float32)
        Vm[lo] = 1.75 * rng.standard_normal(rank).astype(np.float32)  # (strong enough to be listed)
        Vm[hi] = Vm[lo]
        Vm.setflags(write=False)
        copies.setflags(write=False)
        _K5RG_ITEMS[rank] = (Vm, copies)
    return _K5RG_ITEMS[rank]


def k5rg_sample_rows(n_q=K5RG_NQ, seam=K5RG_SLICE_ROWS):
    """The rows compared with fp64: the first 512 (two workgroups), the launch seam of the
    key-log path +- 256, the last 400 and 300 drawn ones (sorted, unique)."""
    drawn = np.random.default_rng(77).choice(n_q, 300, replace=False)
    return np.unique(np.concatenate([np.arange(512), np.arange(seam - 256, seam + 257),
                                     np.arange(n_q - 400, n_q), drawn]))


def k5rg_scores(Q, Vm, copies):
    """fp64 Q Vm^T with the planted ties exact by construction: bit-identical fp32 rows
    have one true score, whatever the matrix product's blocking makes of the columns."""
    S = Q.astype(np.float64) @ Vm.astype(np.float64).T
    S[:, copies[1:]] = S[:, copies[:1]]
    S[:, K5RG_TIE[1]] = S[:, K5RG_TIE[0]]
    return S


def k5rg_window_share(S, top, planted):
    """Share of the top `top` positions of each row of S whose fp64 score lies within the
    1e-5 tie window of the next one down (top + 1 scores per row; the planted columns left
    out): the most the tie rule could excuse on such data."""
    s = -np.sort(-S[:, ~planted], axis=1)[:, :top + 1]
    close = (s[:, :-1] - s[:, 1:]) <= 1e-5 * np.maximum(1.0, np.abs(s[:, :-1]))
    return float(close.mean())
