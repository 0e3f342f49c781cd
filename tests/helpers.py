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
