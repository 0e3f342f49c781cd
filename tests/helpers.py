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
# covers kTkLogBlocks = 512 blocks (csrc/topk_sweep.h), 131,072 rows at two groups.
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


# ---------------------------------------------------------------- ragged rows and the references of K7 / K11 / K13
def ragged_csr(rows):
    """(row_ptr int64 [n + 1], col int32, val float32) of a list of (cols, vals) rows."""
    lens = np.array([len(c) for c, _ in rows], np.int64)
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    col = np.concatenate([np.asarray(c, np.int64) for c, _ in rows] + [np.zeros(0, np.int64)])
    val = np.concatenate([np.asarray(v, np.float32) for _, v in rows] + [np.zeros(0, np.float32)])
    return ptr, col.astype(np.int32), val.astype(np.float32)


def ragged_ptr(lists):
    """(ptr int64 [n + 1], flat int32) of a list of integer lists (K11's targets)."""
    ptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    return ptr, np.concatenate([np.asarray(x, np.int64) for x in lists]
                               + [np.zeros(0, np.int64)]).astype(np.int32)


def known_entries(rows, n_src):
    """The rows with the entries whose column lies outside [0, n_src) removed."""
    out = []
    for c, v in rows:
        c, v = np.asarray(c), np.asarray(v)
        ok = (c >= 0) & (c < n_src)
        out.append((c[ok], v[ok]))
    return out


def fold_in_oracle(rows, V, reg, implicit, alpha):
    """K7's reference: oracle.als_oracle.half_sweep over the rows' ratings with the unknown
    items removed (rows left without a rating are not given to it: their result is defined
    as zero).  Returns (X_ref [n, k] float32, n_used [n])."""
    from oracle import als_oracle as O
    known = known_entries(rows, len(V))
    n_used = np.array([len(c) for c, _ in known], np.int64)
    full = np.nonzero(n_used > 0)[0]
    ref = np.zeros((len(rows), V.shape[1]), np.float32)
    if len(full):
        ptr, col, val = ragged_csr([known[r] for r in full])
        ref[full] = O.half_sweep(ptr, col, val, V, reg, implicit, alpha)
    return ref, n_used


def explain_reference(rows, targets, V, reg, implicit, alpha, yty=None):
    """K11's reference (tests/explain_ref.py): per slot (row, target, score, pos, contrib)
    with the full ordered list.  yty: the [k, k] fp64 Gram to use (the one a kernel call was
    given); None = V^T V in fp64."""
    import explain_ref as R
    if yty is None:
        yty = V.astype(np.float64).T @ V.astype(np.float64)
    out = []
    for r, ((c, v), tg) in enumerate(zip(rows, targets)):
        for t, (s, pos, con) in zip(tg, R.explain_row(c, v, V, tg, reg, implicit, alpha, yty)):
            out.append((r, int(t), s, pos, con))
    return out


def explain_check_slots(ref, rows, V, k, reg, implicit, alpha, sc, pos, con, top_n):
    """Compare one als_explain call's outputs with the reference slots of explain_reference;
    returns (max contribution error, max score error): ||c - c_ref||_2 / ||c_ref||_2 over
    the contribution vector (the whole of it when it fits top_n, the listed head otherwise)
    and |score - score_ref| / (||x_ref|| ||y_t||)."""
    import explain_ref as R
    Vd, sc = V.astype(np.float64), sc.astype(np.float64)
    xs = [R.solve_row(c, v, V, reg, implicit, alpha) for c, v in rows]
    e_c = e_s = 0.0
    for s, (r, t, s_ref, p_ref, c_ref) in enumerate(ref):
        n = min(top_n, len(p_ref))
        np.testing.assert_array_equal(pos[s, :n], p_ref[:n], err_msg=f"slot {s} row {r}")
        assert (pos[s, n:] == -1).all() and (con[s, n:] == 0).all()
        if len(p_ref) == 0:
            assert sc[s] == 0
            continue
        whole = len(p_ref) <= top_n      # the full vector, or the listed head of a longer row
        den = np.linalg.norm(c_ref if whole else c_ref[:n])
        e_c = max(e_c, np.linalg.norm(con[s, :n] - c_ref[:n]) / max(den, 1e-300))
        e_s = max(e_s, abs(sc[s] - s_ref) / (np.linalg.norm(xs[r]) * np.linalg.norm(Vd[t])))
    return e_c, e_s


def nnls_sources(k, signed, seed=0, n_src=200):
    """Unit-norm source rows: signed (about half of a solution's coordinates end on the wall)
    or their absolute values (few do)."""
    rng = np.random.default_rng(3000 + 7 * k + seed)
    Y = rng.standard_normal((n_src, k))
    Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    return (Y if signed else np.abs(Y)).astype(np.float32)


# ---------------------------------------------------------------- the K7 / K11 / K13 edge cases
# (test_gpu_edges_row_kernels.py, test_row_kernel_edges_cpu.py).  csrc/row_system.h takes a
# row's ratings kRowBatch = 32 at a time; row_dispatch picks NB = k_pad / 16 in {1, 2, 4, 8};
# past kRowMaxBlocks = 65,536 rows a workgroup takes a second row.
ROWK_N_SRC = 200
ROWK_REG = 0.1
ROWK_ALPHA = 40.0
ROWK_BATCH = 32
ROWK_LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97)
ROWK_UNKNOWN_ROWS = (("unknown_at_32", 33), ("nsrc_at_64", 65), ("unknown_batch", 64),
                     ("known_last", 33))
ROWK_IMPLICIT_ROWS = (("last_positive_33", 33), ("last_positive_65", 65),
                      ("nonpositive_33", 33), ("nonpositive_65", 65))
ROWK_TOP_N = 10
ROWK_MAX_BLOCKS = 65536
ROWK2_N = ROWK_MAX_BLOCKS + 64
ROWK2_RANK = 8


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def rowk_grid_lengths(rank):
    return [d for d in ROWK_LENGTHS + (rank - 1, rank, rank + 1) if d >= 1]


_ROWK_GRID = {}


def rowk_grid_case(rank, implicit):
    """The §1 rows of one rank and mode, shared (and left unchanged) by every test: the
    grid lengths (distinct source ids per row, half-star ratings; implicit: the same minus
    2.5), then the special rows — `special[name]` is the row's index:
      unknown_at_32     33 entries, entry 32 has col = -1 (alone in the last batch)
      nsrc_at_64        65 entries, entry 64 has col = n_src
      unknown_batch     64 entries, entries 32..63 unknown (a whole batch)
      known_last        33 entries, entries 0..31 unknown, only entry 32 known
      last_positive_d   implicit: every rating <= 0 but the last, which is 2.0 (d = 33, 65)
      nonpositive_d     implicit: no positive rating at all (a zero right-hand side)
    `trimmed[name]`: the four rows with unknown entries, those entries deleted.
    `targets17` / `targets1`: K11's targets per row (17 with a -1, n_src, a rated item and a
    repeat among them; 1)."""
    key = (rank, bool(implicit))
    if key not in _ROWK_GRID:
        lengths = rowk_grid_lengths(rank)
        special = ROWK_UNKNOWN_ROWS + (ROWK_IMPLICIT_ROWS if implicit else ())
        # one draw for both modes (the implicit rows come last and are dropped when explicit)
        degrees = lengths + [d for _, d in ROWK_UNKNOWN_ROWS + ROWK_IMPLICIT_ROWS]
        dst, src, r = degree_rows(degrees, ROWK_N_SRC, seed=6000 + rank,
                                  ratings="signed" if implicit else "stars")
        rows = [(src[dst == t].astype(np.int64), r[dst == t].copy())
                for t in range(len(lengths) + len(special))]
        at = {name: len(lengths) + j for j, (name, _) in enumerate(special)}
        rows[at["unknown_at_32"]][0][32] = -1
        rows[at["nsrc_at_64"]][0][64] = ROWK_N_SRC
        rows[at["unknown_batch"]][0][32:] = -1
        rows[at["known_last"]][0][:32] = -1
        if implicit:
            for name, _ in ROWK_IMPLICIT_ROWS:
                v = rows[at[name]][1]
                v[:] = -np.abs(v) + np.float32(0.0)
                v[0] = -1.5
                if name.startswith("last_positive"):
                    v[-1] = 2.0
        trimmed = {name: known_entries([rows[at[name]]], ROWK_N_SRC)[0]
                   for name, _ in ROWK_UNKNOWN_ROWS}
        rng = np.random.default_rng(6500 + rank)
        targets17 = []
        for c, _ in rows:
            tg = rng.integers(0, ROWK_N_SRC, 17)
            tg[0], tg[4], tg[3] = -1, ROWK_N_SRC, tg[2]
            tg[1] = c[(c >= 0) & (c < ROWK_N_SRC)][0]
            targets17.append(tg)
        targets1 = [tg[5:6] for tg in targets17]
        Y = unit_source_factors(ROWK_N_SRC, rank, seed=6100 + rank)
        for c, v in rows + list(trimmed.values()):
            _freeze(c, v)
        _freeze(Y, *targets17)
        _ROWK_GRID[key] = dict(rank=rank, implicit=bool(implicit), lengths=lengths, special=at,
                               rows=tuple(rows), trimmed=trimmed, Y=Y,
                               targets17=tuple(targets17), targets1=tuple(targets1))
    return _ROWK_GRID[key]


def rowk_zero_rhs_rows(case):
    """Indices of the rows of a grid case whose right-hand side is zero (implicit, no
    positive rating among the used entries): their result is exactly zero."""
    if not case["implicit"]:
        return []
    return [i for i, (c, v) in enumerate(known_entries(case["rows"], ROWK_N_SRC))
            if len(c) and not (v > 0).any()]


_ROWK_REFS = {}


def rowk_grid_refs(rank, implicit):
    """The references of rowk_grid_case, computed once: "fold" = (X fp32, n_used) of
    fold_in_oracle, "explain17" / "explain1" = explain_reference's slots (asserted
    well separated: the order of every list is decided by the values), "nnls" = (A, b,
    n_used, X fp32) of nnls_ref."""
    key = (rank, bool(implicit))
    if key not in _ROWK_REFS:
        import explain_ref as XR
        import nnls_ref as NR
        c = rowk_grid_case(rank, implicit)
        rows, Y = list(c["rows"]), c["Y"]
        out = {"fold": fold_in_oracle(rows, Y, ROWK_REG, implicit, ROWK_ALPHA)}
        for name in ("targets17", "targets1"):
            ref = explain_reference(rows, c[name], Y, ROWK_REG, implicit, ROWK_ALPHA)
            for r, t, _, pos, con in ref:
                assert XR.well_separated(con, pos), (rank, implicit, r, t)
            out["explain" + name[7:]] = ref
        ptr, col, val = ragged_csr(rows)
        A, b, used = NR.systems(ptr, col, val, Y, ROWK_REG, implicit, ROWK_ALPHA)
        X = np.stack([NR.nnls_solve(A[r], b[r]).astype(np.float32) for r in range(len(rows))])
        _freeze(A, b, used, X, *out["fold"])
        out["nnls"] = (A, b, used, X)
        _ROWK_REFS[key] = out
    return _ROWK_REFS[key]


# ---- §2: a workgroup's second row (rank 8, 65,600 rows)
def small_rows_systems(cols, vals, lens, Y, reg, implicit, alpha, yty=None):
    """The normal equations of many rows of <= 3 entries at once, in fp64 and with K7's
    rules: cols / vals [n, 3] (all ids known), lens [n]; yty: the implicit Gram to use
    (None = Y^T Y in fp64).  Returns (A [n, k, k], wb [n, 3] with zeros past a row's
    length, Yj [n, 3, k] likewise, m [n, 3] bool)."""
    Yd = np.asarray(Y, np.float32).astype(np.float64)
    k = Yd.shape[1]
    m = np.arange(cols.shape[1])[None, :] < np.asarray(lens)[:, None]
    Yj = Yd[cols] * m[:, :, None]
    r = np.asarray(vals, np.float64) * m
    if implicit:
        c1 = alpha * np.abs(r)
        pos = (r > 0) & m
        wa, wb, n_reg = c1, np.where(pos, 1.0 + c1, 0.0), pos.sum(1)
        base = Yd.T @ Yd if yty is None else np.asarray(yty, np.float64)
    else:
        wa, wb, n_reg = m.astype(np.float64), r, m.sum(1)
        base = np.zeros((k, k))
    A = np.einsum("nj,nja,njb->nab", wa, Yj, Yj) + base[None]
    A += (reg * n_reg)[:, None, None] * np.eye(k)[None]
    return A, wb, Yj, m


def _assemble(n, lens3, cols3, vals3, designed):
    """CSR of n rows: row i is the first lens3[i] entries of cols3[i] / vals3[i], or
    designed[i] = (cols, vals) when present."""
    lens = np.asarray(lens3, np.int64).copy()
    for i, (c, _) in designed.items():
        lens[i] = len(c)
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    col = np.zeros(ptr[-1], np.int32)
    val = np.zeros(ptr[-1], np.float32)
    m = np.arange(cols3.shape[1])[None, :] < np.asarray(lens3)[:, None]
    m[list(designed)] = False
    at = (ptr[:-1, None] + np.arange(cols3.shape[1])[None, :])[m]
    col[at] = cols3[m]
    val[at] = vals3[m]
    for i, (c, v) in designed.items():
        col[ptr[i]:ptr[i + 1]] = c
        val[ptr[i]:ptr[i + 1]] = v
    return ptr, col, val


def _ratings(rng, n, implicit):
    """Integer ratings 1..5; implicit: minus 3, so -2..2."""
    return (rng.integers(1, 6, n) - (3 if implicit else 0)).astype(np.float32)


_ROWK2 = {}


def rowk_second_row_case(implicit):
    """K7 / K11: ROWK2_N rows at rank ROWK2_RANK.  Workgroup b < 64 takes the rows b and
    b + 65,536; `pairs[name] = (first, second)`:
      empty_then_ordinary    no entry at all -> 20 ratings
      ordinary_then_empty    20 ratings -> no entry
      long_then_short        300 ratings -> 1
      short_then_long        1 rating -> 300
      unknown_then_ordinary  5 entries, none of them a known column -> 20 ratings
      nonpositive_then_ordinary  12 ratings <= 0 (implicit: a zero right-hand side) -> 20
      no_targets_then_17     K11: 0 targets -> 17 targets (20 ratings each)
    Every other row is a filler of 1-3 ratings (cols3 / vals3 / lens3) with one target
    (`tg`).  `designed`: {row: (cols, vals)}; `targets`: K11's ragged targets per row."""
    key = bool(implicit)
    if key not in _ROWK2:
        n, N, B = ROWK2_N, ROWK_N_SRC, ROWK_MAX_BLOCKS
        rng = np.random.default_rng(7100)
        lens3 = rng.integers(1, 4, n)
        cols3 = rng.integers(0, N, (n, 3))
        vals3 = _ratings(rng, n * 3, implicit).reshape(n, 3)
        tg = rng.integers(0, N, n)

        def row(d):
            return rng.integers(0, N, d), _ratings(rng, d, implicit)

        empty = (np.zeros(0, np.int64), np.zeros(0, np.float32))
        unknown = (np.array([-1, N, -1, N + 7, -5]), _ratings(rng, 5, implicit))
        nonpos = row(12)
        nonpos = (nonpos[0], -np.abs(nonpos[1]) - np.float32(0.5))
        names = ("empty_then_ordinary", "ordinary_then_empty", "long_then_short",
                 "short_then_long", "unknown_then_ordinary", "nonpositive_then_ordinary",
                 "no_targets_then_17")
        firsts = (empty, row(20), row(300), row(1), unknown, nonpos, row(20))
        seconds = (row(20), empty, row(1), row(300), row(20), row(20), row(20))
        pairs = {name: (b, b + B) for b, name in enumerate(names)}
        designed = {}
        for b, (f, s) in enumerate(zip(firsts, seconds)):
            designed[b], designed[b + B] = f, s
        ptr, col, val = _assemble(n, lens3, cols3, vals3, designed)
        targets = [tg[i:i + 1] for i in range(n)]
        a, b2 = pairs["no_targets_then_17"]
        targets[a] = np.zeros(0, np.int64)
        targets[b2] = rng.integers(0, N, 17)
        Y = unit_source_factors(N, ROWK2_RANK, seed=7101)
        _freeze(lens3, cols3, vals3, tg, ptr, col, val, Y)
        _ROWK2[key] = dict(n=n, Y=Y, lens3=lens3, cols3=cols3, vals3=vals3, tg=tg, ptr=ptr,
                           col=col, val=val, designed=designed, pairs=pairs, targets=targets)
    return _ROWK2[key]


def nnls_solve_order(row_ptr):
    """The order in which als_nnls_rows' solve launch walks the rows: a stable sort on
    descending degree (ties in index order); workgroup w % 65,536 takes order[w]."""
    return np.argsort(-np.diff(np.asarray(row_ptr)), kind="stable")


_ROWK2_NNLS = {}
ROWK2_POOL = 16


def rowk_second_row_case_nnls(implicit):
    """K13: ROWK2_N rows at rank ROWK2_RANK.  The solve launch walks the rows longest
    first, so a workgroup's second row is one of the 64 shortest and never longer than its
    first; a row without any entry can only come second.  The rows 65,537..65,599 have one
    rating each and row 9 none: with nnls_solve_order they are the second rows of the
    workgroups 0..62 and 63.  The first rows are the rows 10..14, the longest of the call
    in this order; `pairs[name] = (first, second)`:
      long_then_short        300 ratings -> 1
      unknown_then_ordinary  40 entries, none known (the n = 0 exit) -> 1 rating
      nonpositive_then_ordinary  30 ratings <= 0 (implicit: b = 0) -> 1 rating
      zero_rhs_then_ordinary 25 ratings of 0: b = 0 in both modes, the solver stops at
                             iteration 0 -> 1 rating
      ordinary_then_ordinary 20 ratings -> 1
      ordinary_then_empty    workgroup 63's filler of 3 ratings -> row 9
    Every other row is one of ROWK2_POOL filler rows of 1-3 ratings (`pool`, `which`)."""
    key = bool(implicit)
    if key not in _ROWK2_NNLS:
        n, N, B, P = ROWK2_N, ROWK_N_SRC, ROWK_MAX_BLOCKS, ROWK2_POOL
        rng = np.random.default_rng(7200)
        pool_lens = np.array([1 + j % 3 for j in range(P)])
        pool_cols = rng.integers(0, N, (P, 3))
        pool_vals = _ratings(rng, P * 3, implicit).reshape(P, 3)
        if implicit:
            pool_vals[:, 0] = np.abs(pool_vals[:, 0]) + 1   # every filler has a positive rating
        which = rng.integers(0, P, n)
        ones = np.nonzero(pool_lens == 1)[0]
        which[B + 1:] = ones[rng.integers(0, len(ones), n - B - 1)]

        def row(d):
            return rng.integers(0, N, d), _ratings(rng, d, implicit)

        unknown = (np.where(np.arange(40) % 2 == 0, -1, N), _ratings(rng, 40, implicit))
        nonpos = row(30)
        nonpos = (nonpos[0], -np.abs(nonpos[1]) - np.float32(0.5))
        zero = (rng.integers(0, N, 25), np.zeros(25, np.float32))
        designed = {9: (np.zeros(0, np.int64), np.zeros(0, np.float32)), 10: row(300),
                    11: unknown, 12: nonpos, 13: zero, 14: row(20)}
        ptr, col, val = _assemble(n, pool_lens[which], pool_cols[which], pool_vals[which],
                                  designed)
        order = nnls_solve_order(ptr)
        names = ("long_then_short", "unknown_then_ordinary", "nonpositive_then_ordinary",
                 "zero_rhs_then_ordinary", "ordinary_then_ordinary")
        pairs = {name: (int(order[w]), int(order[w + B])) for w, name in enumerate(names)}
        pairs["ordinary_then_empty"] = (int(order[63]), int(order[63 + B]))
        Y = nnls_sources(ROWK2_RANK, True, seed=5, n_src=N)
        pool = [(pool_cols[j, :pool_lens[j]], pool_vals[j, :pool_lens[j]]) for j in range(P)]
        _freeze(which, ptr, col, val, Y, order)
        _ROWK2_NNLS[key] = dict(n=n, Y=Y, pool=pool, which=which, ptr=ptr, col=col, val=val,
                                designed=designed, pairs=pairs, order=order)
    return _ROWK2_NNLS[key]


ROWK_PIVOT_RANK = 4
_ROWK_PIVOT = {}


def rowk_failed_pivot_case():
    """K7 / K11, explicit, reg = 0, rank 4, ROWK2_N rows: fillers of 6 distinct items (a
    positive definite A: redrawn until the smallest eigenvalue exceeds 1e-5 of the largest;
    `eig_ratio` holds every filler's), and two rows of 2 ratings whose A has rank 2:
    `failing` = (0, 65,537), i.e. the pairs (failed pivot -> ordinary) in workgroup 0 and
    (ordinary -> failed pivot) in workgroup 1.  cols / vals: [n, 6]; the failing rows use
    the first 2 entries."""
    if not _ROWK_PIVOT:
        n, N, k = ROWK2_N, ROWK_N_SRC, ROWK_PIVOT_RANK
        rng = np.random.default_rng(7300)
        Y = unit_source_factors(N, k, seed=7301)
        Yd = Y.astype(np.float64)
        cols = np.argsort(rng.random((n, N)), axis=1)[:, :6]      # 6 distinct items per row
        ratio = np.zeros(n)
        todo = np.arange(n)
        for _ in range(50):
            Yj = Yd[cols[todo]]
            ev = np.linalg.eigvalsh(np.einsum("nja,njb->nab", Yj, Yj))
            ratio[todo] = ev[:, 0] / ev[:, -1]
            todo = todo[ratio[todo] <= 1e-5]
            if not len(todo):
                break
            cols[todo] = np.argsort(rng.random((len(todo), N)), axis=1)[:, :6]
        assert not len(todo)
        vals = rng.integers(1, 6, (n, 6)).astype(np.float32)
        failing = (0, ROWK_MAX_BLOCKS + 1)
        lens = np.full(n, 6)
        lens[list(failing)] = 2
        ptr = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=ptr[1:])
        m = np.arange(6)[None, :] < lens[:, None]
        _freeze(Y, cols, vals, lens, ptr, ratio)
        _ROWK_PIVOT.update(n=n, Y=Y, cols=cols, vals=vals, lens=lens, ptr=ptr, m=m,
                           col=cols[m].astype(np.int32), val=vals[m], failing=failing,
                           eig_ratio=ratio, tg=rng.integers(0, N, n))
    return _ROWK_PIVOT


# ---- §3: K13's task boundaries and the short workspace
ROWK3_RANKS = (16, 128)
ROWK3_CHUNKS = (33, 1)


def rowk3_lengths(chunk):
    """c - 1, c, c + 1, 2c, 2c + 1, 3c - 1 and a 200-rating row with every fifth column
    unknown; chunk = 1: the lengths <= 5 of those, one of 40, and the 200-rating row."""
    c = chunk
    lens = [c - 1, c, c + 1, 2 * c, 2 * c + 1, 3 * c - 1]
    if chunk == 1:
        lens = [d for d in lens if d <= 5] + [40]
    return lens + [200]


def nnls_task_counts(lens, chunk):
    """Tasks per row as nnls_keys_kernel counts them: ceil(d / chunk) for d > chunk, else 0."""
    return [-(-d // chunk) if d > chunk else 0 for d in lens]


def nnls_slot_bytes(k):
    """One task's workspace slot: (nb (nb + 1) / 2 + 1) x 256 + 2 doubles, nb = k_pad / 16."""
    k_pad = 16 if k <= 16 else 32 if k <= 32 else 64 if k <= 64 else 128
    nb = k_pad // 16
    return 8 * ((nb * (nb + 1) // 2 + 1) * 256 + 2)


def nnls_wall_margin(A, b, seed=0, eps=1e-13):
    """How far nnls_ref's solution moves (relative 2-norm) when A and b are perturbed by eps
    relative, entry by entry (A kept symmetric): a row whose solution sits on a wall decision
    moves by far more than eps."""
    import nnls_ref as NR
    rng = np.random.default_rng(seed)
    x = NR.nnls_solve(A, b)
    E = rng.uniform(-1, 1, A.shape)
    E = (E + E.T) / 2
    xp = NR.nnls_solve(A * (1 + eps * E), b * (1 + eps * rng.uniform(-1, 1, b.shape)))
    return float(np.linalg.norm(xp - x) / max(np.linalg.norm(x), 1e-30))


ROWK3_MARGIN = 1e-8
_ROWK3 = {}


def rowk3_case(rank, signed, implicit, chunk):
    """The §3 rows of one (rank, sources, mode, chunk): rowk3_lengths(chunk), ids drawn with
    repetition, ratings 1..5, every fifth column of the last row unknown.  A row whose
    reference solution moves by ROWK3_MARGIN or more under nnls_wall_margin's 1e-13
    perturbation is redrawn (`redrawn` counts them), so the 1e-6 bar between two summation
    orders is one the reference alone keeps.  Returns dict(Y, rows, lens, ref = nnls_ref's
    fp32 rows, margins)."""
    key = (rank, bool(signed), bool(implicit), chunk)
    if key not in _ROWK3:
        import nnls_ref as NR
        Y = nnls_sources(rank, signed, seed=1, n_src=ROWK_N_SRC)
        lens = rowk3_lengths(chunk)
        rows, margins, redrawn = [], [], 0
        for j, d in enumerate(lens):
            for attempt in range(20):
                rng = np.random.default_rng(8000 + 100 * rank + 10 * j + 1000 * attempt + chunk)
                c, v = rng.integers(0, ROWK_N_SRC, d), rng.integers(1, 6, d).astype(np.float32)
                if j == len(lens) - 1:
                    c[::5] = -1
                ptr, col, val = ragged_csr([(c, v)])
                A, b, _ = NR.systems(ptr, col, val, Y, ROWK_REG, implicit, ROWK_ALPHA)
                mg = nnls_wall_margin(A[0], b[0], seed=j) if d else 0.0
                if mg < ROWK3_MARGIN:
                    break
                redrawn += 1
            else:
                raise AssertionError(f"no stable row of {d} ratings found: {key}")
            rows.append((c, v))
            margins.append(mg)
        ptr, col, val = ragged_csr(rows)
        ref = NR.solve_rows(ptr, col, val, Y, ROWK_REG, implicit, ROWK_ALPHA)
        for c, v in rows:
            _freeze(c, v)
        _freeze(Y, ref)
        _ROWK3[key] = dict(Y=Y, rows=tuple(rows), lens=lens, ref=ref, margins=margins,
                           redrawn=redrawn)
    return _ROWK3[key]
