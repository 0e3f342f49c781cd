"""Shared helpers of the fp64 rescue tests (test_rescue_cpu.py, test_gpu_rescue64.py): where
als_solve_half keeps the rescue list, thin views over it, the fp64 reference of a row before
any rounding to fp32, the conditioning of the systems the tests use, and a block whose
Cholesky failure is exact in fp64.

The bar of the GPU file is derived here, not measured.  rescue64_kernel (csrc/rescue64.h)
forms exact fp64 products of fp32 values, sums them in fp64, factorises in fp64 and rounds
once, to fp32, at the store:

  * the final cast is at most 2^-24 relative per entry, so 2^-24 norm-wise;
  * the fp64 part differs from the reference below by summation order and elimination order
    only: at most a small multiple of rank * cond(A) * 2^-53, which COND_BAR keeps at or below
    2^-30 on every case (test_rescue_cpu.py), three orders of magnitude below the cast;
  * the ABI carries regParam as a float, so the kernel's lambda is (double)(float)0.1, 2^-26
    off 0.1: the references below take the same value (abi_reg), which leaves no such term;
  * a factor 2 of margin covers all of it: BAR = 2^-23.
"""
import numpy as np

from oracle import als_oracle as O
from helpers import (K2K3_RANKS, K2K3_REG, fp32_textbook_half_sweep, k2k3_grid_case,
                     k2k3_special_rows, ragged_csr)

BAR = 2.0 ** -23        # per listed row, ||x - ref|| / ||ref||
COND_BAR = 2.0 ** -30   # rank * cond(A) * 2^-53 of every system a GPU test solves
RESCUE_GRID = 64        # csrc/solve_config.h kRescueGrid: workgroups walking the list
RESCUE_BATCH = 32       # csrc/rescue64.h kRescueBatch: ratings staged per step
YARDSTICK_FACTOR = 8.0  # 2^-21 / 2^-24: the split-f16 product against an fp32 one


def abi_reg(reg):
    """regParam as als_solve_half receives it (a C float), widened back to a double."""
    return float(np.float32(reg))


REG = abi_reg(K2K3_REG)  # what every reference of the reg = 0.1 cases uses


# ---------------------------------------------------------------- the list in the workspace
def align256(n):
    return (int(n) + 255) & ~255


def table_offset(ws_bytes, n_src, k_pad):
    """Byte offset of the split table: (n_src + 1) x k_pad words that end at the workspace
    end, their start rounded down to 256 B (csrc/gram_solve.hip, als_solve_half)."""
    return (int(ws_bytes) - align256(4 * int(k_pad) * (int(n_src) + 1))) & ~255


def list_region(ws_bytes, rank, n_src, n_rows, k_pad):
    """Byte offset of the rescue list (int32 [n_rows]) in a workspace of ws_bytes: right
    below the split table.  int32 word 2 of the workspace is the list count, word 3 the
    rescue launch's finished-block counter.  k_pad: als_k_pad(rank)."""
    if not (1 <= rank <= k_pad and k_pad % 16 == 0 and k_pad - rank < max(16, k_pad // 2)):
        raise ValueError(f"k_pad {k_pad} is not the padded rank of {rank}")
    if n_src < 0 or n_rows < 0:
        raise ValueError("negative sizes")
    return table_offset(ws_bytes, n_src, k_pad) - align256(4 * int(n_rows))


def _list_view(ws, rank, n_src, n_rows):
    import torch
    import als_mi355x.engine as E
    nbytes = int(ws.buf.numel())
    kp = E.k_pad(rank)
    off = list_region(nbytes, rank, n_src, n_rows, kp)
    end = off + 4 * n_rows
    if off < 256 or off % 256 or end > table_offset(nbytes, n_src, kp):
        raise ValueError(f"the list [{off}, {end}) does not fit a workspace of {nbytes} bytes")
    return ws.buf[off:end].view(torch.int32)


def count_words(ws):
    """(list count, finished-block counter): int32 words 2 and 3 of the workspace."""
    import torch
    torch.cuda.synchronize()
    w = ws.buf[8:16].view(torch.int32).cpu()
    return int(w[0]), int(w[1])


def write_list(ws, rows, rank, n_src, n_rows):
    """Put `rows` (dense destination rows, each in [0, n_rows), at most n_rows of them) on
    the rescue list of a call with these sizes and set the count; the finished-block
    counter is set to 0, as the prep leaves it."""
    import torch
    rows = np.asarray(rows, np.int64).reshape(-1)
    if len(rows) > n_rows or (len(rows) and (rows.min() < 0 or rows.max() >= n_rows)):
        raise ValueError("listed rows must lie in [0, n_rows) and fit the list")
    view = _list_view(ws, rank, n_src, n_rows)
    view[:len(rows)] = torch.as_tensor(rows.astype(np.int32)).to(view.device)
    ws.buf[8:16].view(torch.int32).copy_(torch.tensor([len(rows), 0], dtype=torch.int32))


def read_list(ws, rank, n_src, n_rows):
    """The listed rows, in list order (int64 [count])."""
    n = count_words(ws)[0]
    if not 0 <= n <= n_rows:
        raise ValueError(f"list count {n} outside [0, {n_rows}]")
    return _list_view(ws, rank, n_src, n_rows)[:n].cpu().numpy().astype(np.int64)


# ---------------------------------------------------------------- fp64 references
def systems(indptr, indices, vals, Y, reg, implicit=False, alpha=1.0, rows=None):
    """(A [n, k, k], b [n, k]) of CholeskySolver.solve in fp64: NormalEquation.add
    (oracle.als_oracle.normal_equations), + YtY for implicit, + reg * numExplicits on the
    diagonal."""
    A, b, ne = O.normal_equations(indptr, indices, vals, Y, implicit, alpha, rows)
    if implicit:
        A += O.yty(Y)[None]
    dg = np.arange(A.shape[1])
    A[:, dg, dg] += float(reg) * ne.astype(np.float64)[:, None]
    return A, b


def system_conds(indptr, indices, vals, Y, reg, implicit=False, alpha=1.0, rows=None):
    """fp64 2-norm condition number of every row's A."""
    A, _ = systems(indptr, indices, vals, Y, reg, implicit, alpha, rows)
    return np.linalg.cond(A, 2)


def exact_ref(indptr, indices, vals, Y, reg, implicit=False, alpha=1.0, rows=None):
    """The fp64 solution of every row, before any rounding to fp32 ([n, k] float64)."""
    A, b = systems(indptr, indices, vals, Y, reg, implicit, alpha, rows)
    return np.linalg.solve(A, b[..., None])[..., 0]


def row_errs(x, ref):
    """Per row ||x - ref|| / ||ref||; absolute where ref is zero."""
    x = np.asarray(x, np.float64)
    ref = np.asarray(ref, np.float64)
    nr = np.linalg.norm(ref, axis=1)
    e = np.linalg.norm(x - ref, axis=1) / np.where(nr > 0, nr, 1.0)
    e[nr == 0] = np.linalg.norm(x[nr == 0], axis=1)
    return e


def packed_yty(Y, k_pad):
    """oracle.als_oracle.yty(Y), exact fp64, in the lower-packed layout rescue64_kernel
    reads (entry i (i + 1) / 2 + j, j <= i < k); the entries of padded dims hold NaN: the
    kernel reads the first k (k + 1) / 2 only.  (als_yty's own Gram runs on the f16 matrix
    cores with fp32-grade products; with it the implicit cases would measure K2b.)"""
    G = O.yty(Y)
    out = np.full(k_pad * (k_pad + 1) // 2, np.nan)
    i, j = np.tril_indices(G.shape[0])
    out[i * (i + 1) // 2 + j] = G[i, j]
    return out


def cond_term(rank, conds):
    """rank * cond * 2^-53, the fp64 term of the error bound (largest over the rows)."""
    return float(rank * np.max(conds) * 2.0 ** -53)


# ---------------------------------------------------------------- the cases of the GPU file
GRID_MODES = {"explicit": (False, 1.0), "implicit_a4": (True, 4.0), "implicit_a40": (True, 40.0)}
GRID_CASES = [(rank, mode) for rank in K2K3_RANKS for mode in GRID_MODES]
PARTIAL_CASES = [(rank, mode) for rank in (3, 33, 128) for mode in ("explicit", "implicit_a4")]
SPECIAL_RANKS = (1, 16, 33, 64, 128)
SPECIAL_ALPHA = 4.0
FAIL_RANKS = (4, 33, 128)
GUARD_RANKS = (16, 32, 64, 128)
GUARD_SCALE = 2.0 ** -30
_REFS = {}


def _refs(key, case, reg, implicit, alpha, rows=None):
    if key not in _REFS:
        a = (case["indptr"], case["indices"], case["vals"], case["Y"], reg, implicit, alpha, rows)
        A, b = systems(*a)
        X = np.linalg.solve(A, b[..., None])[..., 0]
        conds = np.linalg.cond(A, 2)
        X.setflags(write=False)
        conds.setflags(write=False)
        _REFS[key] = (X, conds)
    return _REFS[key]


def grid_refs(rank, mode):
    """(exact_ref, system_conds) of helpers.k2k3_grid_case(rank, implicit) in one mode of
    GRID_MODES, computed once and left unchanged."""
    implicit, alpha = GRID_MODES[mode]
    return _refs(("grid", rank, mode), k2k3_grid_case(rank, implicit), REG, implicit, alpha)


def special_refs(rank):
    """The same of helpers.k2k3_special_rows(rank), implicit at SPECIAL_ALPHA."""
    return _refs(("special", rank), k2k3_special_rows(rank), REG, True, SPECIAL_ALPHA)


# ---- (d): a block whose failure is exact in fp64
FAIL_ROWS = 3 * RESCUE_GRID
_FAIL_COEF = (1, 1, 1, 1, 2, 4)                      # source a + rank * j is _FAIL_COEF[j] e_a
_FAIL_CHOICES = ((0,), (4,), (0, 1, 2, 3), (5,))     # sum of squares 1, 4, 4, 16
_FAILING = {}


def failing_row(t):
    """Row t of failing_case fails iff t and t // RESCUE_GRID have the same parity: with every
    row listed in order, workgroup w of RESCUE_GRID takes the rows w, w + 64, w + 128, i.e.
    failing -> full rank -> failing for even w and the reverse for odd w."""
    return ((t & 1) ^ ((t // RESCUE_GRID) & 1)) == 0


def fail_columns(rank):
    return (1, max(1, rank // 2), rank - 1)


def failing_case(rank):
    """An explicit block for reg = 0, FAIL_ROWS destination rows over 6 rank one-hot integer
    sources (source a + rank j = c_j e_a, c = 1, 1, 1, 1, 2, 4), so every A is diagonal with
    small integer entries and every sum is exact in any order.

    A full-rank row rates, on every axis a, one of the source sets _FAIL_CHOICES: A_aa is 1,
    4 or 16, its square root and both divisions are exact, and x_a = b_a / A_aa is a
    half-integer multiple of 1/16 that fp32 holds exactly (`X` [n, rank] float64; NaN rows
    for the failing ones).  A failing row rates every axis below `fail_col[row]` (one of
    fail_columns(rank), all >= 1), no source on that axis and about half of the axes above:
    the kernel's right-looking Cholesky meets a pivot of exactly 0.0 at that column, in the
    middle of the factorisation.  Ratings are half stars; every row has at least one and
    every source id is rated by some row (dense ids = ids)."""
    if rank < 2:
        raise ValueError("failing_case needs rank >= 2 (a pivot at a column >= 1)")
    if rank not in _FAILING:
        rng = np.random.default_rng(9000 + rank)
        n_src = len(_FAIL_COEF) * rank
        Y = np.zeros((n_src, rank), np.float32)
        for j, c in enumerate(_FAIL_COEF):
            Y[np.arange(rank) + rank * j, np.arange(rank)] = c
        cols_of = {}
        fail_col = np.full(FAIL_ROWS, -1)
        q_fail = q_full = 0
        for t in range(FAIL_ROWS):
            if failing_row(t):
                jc = fail_columns(rank)[q_fail % 3]
                axes = list(range(jc)) + [a for a in range(jc + 1, rank) if rng.random() < 0.5]
                fail_col[t] = jc
                q = q_fail
                q_fail += 1
            else:
                axes = list(range(rank))
                q = q_full
                q_full += 1
            ids = [a + rank * j for a in axes for j in _FAIL_CHOICES[(q + a) % 4]]
            cols_of[t] = rng.permutation(np.array(ids))
        dst = np.concatenate([np.full(len(cols_of[t]), t) for t in range(FAIL_ROWS)]).astype(np.int32)
        src = np.concatenate([cols_of[t] for t in range(FAIL_ROWS)]).astype(np.int32)
        r = (rng.integers(1, 11, len(src)) / 2).astype(np.float32)
        assert np.array_equal(np.unique(src), np.arange(n_src)) and np.bincount(dst).min() >= 1
        indptr, indices, vals = O.csr_build(dst, src, r, FAIL_ROWS)
        failing = np.nonzero(fail_col >= 0)[0]
        full = np.nonzero(fail_col < 0)[0]
        A, b, _ = O.normal_equations(indptr, indices, vals, Y, rows=full)
        X = np.full((FAIL_ROWS, rank), np.nan)
        X[full] = b / np.diagonal(A, axis1=1, axis2=2)
        for a in (Y, fail_col, failing, full, indptr, indices, vals, X):
            a.setflags(write=False)
        _FAILING[rank] = dict(rank=rank, n_src=n_src, dst=dst, src=src, r=r, indptr=indptr,
                              indices=indices, vals=vals, Y=Y, fail_col=fail_col,
                              failing=failing, full=full, X=X)
    return _FAILING[rank]


def cholesky_replay(A):
    """rescue64_kernel's factorisation, step by step in fp64 (right-looking, in place on the
    lower triangle: pivot test `!(dd > 0)`, sqrt, column / l, trailing update).  Returns the
    column at which it breaks, or -1 when every pivot is positive."""
    L = np.array(A, np.float64)
    k = L.shape[0]
    for jc in range(k):
        dd = L[jc, jc]
        if not dd > 0.0:
            return jc
        l = np.sqrt(dd)
        L[jc, jc] = l
        L[jc + 1:, jc] /= l
        c = L[jc + 1:, jc]
        L[jc + 1:, jc + 1:] -= np.tril(np.outer(c, c))
    return -1


# ---- (e): ratings the explicit guards must send to the rescue
_GUARD = {}


def guard_case(rank):
    """helpers.k2k3_grid_case(rank, explicit) with every rating times GUARD_SCALE (exact: the
    fp64 solution scales exactly) plus one anchor destination row, the last, with a single
    rating of 1.0 on source 0: the launch's rating scale is the anchor's, and every other
    row's scaled ratings sit 2^-28 and more below the split window."""
    if rank not in _GUARD:
        c = k2k3_grid_case(rank, False)
        n = len(c["indptr"]) - 1
        small = (c["r"].astype(np.float64) * GUARD_SCALE).astype(np.float32)
        assert np.array_equal(small.astype(np.float64), c["r"].astype(np.float64) * GUARD_SCALE)
        dst = np.concatenate([c["dst"], [n]]).astype(np.int32)
        src = np.concatenate([c["src"], [0]]).astype(np.int32)
        r = np.concatenate([small, [1.0]]).astype(np.float32)
        indptr, indices, vals = O.csr_build(dst, src, r, n + 1)
        _GUARD[rank] = dict(dst=dst, src=src, r=r, indptr=indptr, indices=indices, vals=vals,
                            Y=c["Y"], anchor=n)
    return _GUARD[rank]


def guard_refs(rank):
    """(exact_ref [n + 1, rank], system_conds [n + 1]) of guard_case(rank): the grid's own
    references scaled (A does not see the ratings), the anchor row solved here."""
    g = guard_case(rank)
    X, conds = grid_refs(rank, "explicit")
    xa, ca = _refs(("anchor", rank), g, REG, False, 1.0, rows=[g["anchor"]])
    return np.concatenate([X * GUARD_SCALE, xa]), np.concatenate([conds, ca])


def guard_unlisted(rank, dual):
    """(dual-path rows, rows the guards leave off the list) of guard_case(rank): with the
    dual path on, the rows of <= dual_limit(rank) ratings; always the anchor."""
    import als_mi355x.engine as E
    g = guard_case(rank)
    deg = np.diff(g["indptr"])
    dual_rows = np.nonzero(deg <= E.dual_limit(rank))[0] if dual else np.zeros(0, np.int64)
    return dual_rows, np.union1d(dual_rows, [g["anchor"]]).astype(np.int64)


GUARD_CASES = [(rank, dual) for rank in GUARD_RANKS
               for dual in ((True, False) if rank > 32 else (True,))]  # dual path: rank >= 33
_GUARD_YARD = {}


def guard_textbook_errs(rank, rows):
    """Per-row errors, against guard_refs, of the fp32 textbook solve
    (helpers.fp32_textbook_half_sweep) of the given rows of guard_case(rank): the yardstick
    of the rows that the fp32-grade path keeps (the anchor, the dual-path rows), as in
    test_gpu_edges_k2_k3.py: the GPU may be YARDSTICK_FACTOR times worse, no more."""
    key = (rank, tuple(int(r) for r in rows))
    if key not in _GUARD_YARD:
        g = guard_case(rank)
        p, idx, v = g["indptr"], g["indices"], g["vals"]
        ptr, col, val = ragged_csr([(idx[p[r]:p[r + 1]], v[p[r]:p[r + 1]]) for r in key[1]])
        Xt = fp32_textbook_half_sweep(ptr, col, val, g["Y"], K2K3_REG)
        _GUARD_YARD[key] = row_errs(Xt, guard_refs(rank)[0][list(key[1])])
    return _GUARD_YARD[key]
