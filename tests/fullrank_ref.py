"""numpy fp64 oracle of the full-ranking kernel K9 (als_rank_positions / als_full_rank_metrics).

Scores are s*(r, v) = the fp64 dot product of the fp32 factor rows; the kernel's contract is
|s^ - s*| <= tau(r, v) = 2 * rank * 2^-24 * sum_d |q_d v_d|.  For every relevant entry j of
query row r, over the admissible rows v != j, counts() gives

    lo    = #{s*_v >  s*_j + tau_v + tau_j}     (rows above j whatever the rounding did)
    above = #{s*_v >  s*_j}
    tied  = #{s*_v == s*_j}
    hi    = #{s*_v >= s*_j - tau_v - tau_j}     (rows that can be above or level with j)

so a conforming kernel has lo <= above^ and above^ + tied^ <= hi.  An entry that is itself
inadmissible (excluded for its row, outside `allow`, or with a NaN score) has -1 everywhere.
metrics() is the reduction als_full_rank_metrics performs, from given counts.
"""
import numpy as np

SUMS = ("sum_w_pr", "sum_w", "sum_row_pr", "sum_auc", "auc_rows", "sum_rr", "rr_rows", "rows",
        "pairs", "inadmissible", "pr_rows")
U24 = 2.0 ** -24


def score_matrix(Q, V):
    """(s* [n_q, n_v], tau [n_q, n_v]) in fp64 from fp32 factors."""
    q, v = np.asarray(Q, np.float64), np.asarray(V, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = q @ v.T
        tau = 2.0 * q.shape[1] * U24 * (np.abs(q) @ np.abs(v).T)
    return s, tau


def admissible_mask(n_q, n_v, ex=None, allow=None):
    """bool [n_q, n_v]: allowed and not excluded.  ex: per-row arrays of V rows (duplicates
    fine) or None; allow: iterable of allowed V rows or None."""
    ok = np.ones((n_q, n_v), bool)
    if allow is not None:
        col = np.zeros(n_v, bool)
        a = np.asarray(list(allow), np.int64)
        col[a[(a >= 0) & (a < n_v)]] = True
        ok &= col[None, :]
    if ex is not None:
        for r, e in enumerate(ex):
            e = np.asarray(e, np.int64)
            ok[r, e[(e >= 0) & (e < n_v)]] = False
    return ok


def counts(Q, V, rel, ex=None, allow=None):
    """rel: per-row ascending arrays of V rows.  Returns a dict of int64 arrays aligned with
    np.concatenate(rel) — lo, above, tied, hi, row — plus n_adm [n_q], `banded` = the
    (entry, other row) comparisons that fall inside the band (sum of hi - lo) and
    `compared` = all comparisons made."""
    n_q, n_v = len(rel), len(V)
    s, tau = score_matrix(Q, V)
    adm = admissible_mask(n_q, n_v, ex, allow) & ~np.isnan(s)
    lo, above, tied, hi, row = [], [], [], [], []
    compared = 0
    for r in range(n_q):
        sr, tr, ar = s[r], tau[r], adm[r]
        for j in np.asarray(rel[r], np.int64):
            row.append(r)
            if j < 0 or j >= n_v or not ar[j]:
                for x in (lo, above, tied, hi):
                    x.append(-1)
                continue
            other = ar.copy()
            other[j] = False
            so, to = sr[other], tr[other]
            lo.append(int((so > sr[j] + to + tr[j]).sum()))
            above.append(int((so > sr[j]).sum()))
            tied.append(int((so == sr[j]).sum()))
            hi.append(int((so >= sr[j] - to - tr[j]).sum()))
            compared += int(other.sum())
    out = {k: np.asarray(x, np.int64) for k, x in
           (("lo", lo), ("above", above), ("tied", tied), ("hi", hi), ("row", row))}
    out["n_adm"] = adm.sum(1).astype(np.int64)
    valid = out["above"] >= 0
    # comparisons the bound does not decide: s*_v within tau_v + tau_j of s*_j
    out["banded"] = int((out["hi"][valid] - out["lo"][valid]).sum())
    out["compared"] = compared
    return out


def sums(above, tied, n_adm, row, weights=None):
    """als_full_rank_metrics' 11 sums (SUMS order) in fp64 from per-entry counts."""
    above, tied = np.asarray(above, np.float64), np.asarray(tied, np.float64)
    row = np.asarray(row, np.int64)
    w = np.ones(len(above)) if weights is None else np.asarray(weights, np.float64)
    s = dict.fromkeys(SUMS, 0.0)
    for r in range(len(n_adm)):
        mine = row == r
        s["inadmissible"] += float((mine & (above < 0)).sum())
        sel = mine & (above >= 0)
        m = float(sel.sum())
        if m == 0:
            continue
        N = float(n_adm[r])
        p = above[sel] + 0.5 * tied[sel]
        s["rows"] += 1
        s["pairs"] += m
        s["sum_rr"] += 1.0 / (1.0 + p.min())
        s["rr_rows"] += 1
        if N > 1:
            s["sum_w_pr"] += float((w[sel] * p).sum()) / (N - 1)
            s["sum_w"] += float(w[sel].sum())
            s["sum_row_pr"] += float(p.sum()) / (N - 1) / m
            s["pr_rows"] += 1
        if N > m:
            s["sum_auc"] += 1.0 - (float(p.sum()) - 0.5 * m * (m - 1)) / (m * (N - m))
            s["auc_rows"] += 1
    return [s[k] for k in SUMS]


def metrics(above, tied, n_adm, row, weights=None):
    s = sums(above, tied, n_adm, row, weights)

    def ratio(a, b):
        return a / b if b > 0 else float("nan")
    return {"expectedPercentileRank": ratio(s[0], s[1]), "meanPercentileRank": ratio(s[2], s[10]),
            "auc": ratio(s[3], s[4]), "mrr": ratio(s[5], s[6]), "rows": int(s[7]),
            "pairs": int(s[8]), "inadmissible": int(s[9])}


def brute_force(Q, V, rel, ex=None, allow=None):
    """above per entry by a full descending argsort of each row's admissible scores; valid
    only when no two admissible scores of a row are equal (the caller checks)."""
    n_q, n_v = len(rel), len(V)
    s, _ = score_matrix(Q, V)
    adm = admissible_mask(n_q, n_v, ex, allow) & ~np.isnan(s)
    out = []
    for r in range(n_q):
        cols = np.nonzero(adm[r])[0]
        order = cols[np.argsort(-s[r, cols], kind="stable")]
        pos = {int(c): p for p, c in enumerate(order)}
        out.extend(pos.get(int(j), -1) for j in rel[r])
    return np.asarray(out, np.int64)


# ---------------------------------------------------------------- shared test inputs
def integer_factors(rng, n, rank):
    return rng.integers(-8, 9, (n, rank)).astype(np.float32)


def random_relevant(rng, n_q, n_v, sizes):
    """Per-row ascending relevant sets; sizes: per-row sizes (clamped to n_v)."""
    return [np.sort(rng.choice(n_v, min(int(m), n_v), replace=False)).astype(np.int64)
            for m in sizes]


def random_exclusions(rng, n_q, n_v, rel, mean=6):
    """Per-row ascending exclusion lists with duplicates; every third row also excludes one
    of its own relevant rows (when it has any)."""
    ex = []
    for r in range(n_q):
        e = rng.integers(0, n_v, int(rng.integers(0, 2 * mean + 1)))
        e = np.concatenate([e, e[: len(e) // 3]])  # duplicates
        if r % 3 == 0 and len(rel[r]):
            e = np.concatenate([e, rel[r][:1]])
        ex.append(np.sort(e).astype(np.int64))
    return ex


def ranges(lists):
    """Per-row lists -> (begin int64 [n], end int64 [n], col int32 [>= 1])."""
    lens = np.array([len(x) for x in lists], np.int64)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    col = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)])
    if col.size == 0:
        col = np.zeros(1, np.int64)
    return ptr[:-1].copy(), ptr[1:].copy(), col.astype(np.int32)
