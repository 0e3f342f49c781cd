"""numpy fp64 restatement of the K15 contracts (include/als_hip.h): als_list_exposure,
als_list_concentration and als_list_novelty, skip rules and NaN rules included, plus the
dictionary engine.list_metrics_dict forms from their sums."""
import math

import numpy as np


def unpack_bits(bits, n_v):
    """bool [n_v] of a mask in the form filters.pack_allow_bits writes (int32 words holding
    uint32 patterns; bits past n_v are ignored); None = every row."""
    if bits is None:
        return np.ones(n_v, bool)
    w = np.asarray(bits).astype(np.int64) & 0xFFFFFFFF
    j = np.arange(n_v)
    return ((w[j >> 5] >> (j & 31)) & 1).astype(bool)


def pack_bits(mask):
    """The inverse: bool [n_v] -> int32 words (at least one)."""
    mask = np.asarray(mask, bool)
    n_words = max((len(mask) + 31) // 32, 1)
    w = np.zeros(n_words, np.int64)
    j = np.nonzero(mask)[0]
    np.add.at(w, j >> 5, np.int64(1) << (j & 31))
    return np.where(w >= 2 ** 31, w - 2 ** 32, w).astype(np.int32)


def valid_entries(idx, at, n_v, allow=None):
    """bool [n_q, at]: which of the first `at` positions of every row count."""
    idx = np.asarray(idx)[:, :at].astype(np.int64)
    ok = (idx >= 0) & (idx < n_v)
    if allow is not None and n_v > 0:
        ok &= unpack_bits(allow, n_v)[np.clip(idx, 0, n_v - 1)]
    return ok


def exposure(idx, at, n_v, allow=None):
    """(counts int64 [n_v], skipped entries)."""
    idx = np.asarray(idx)[:, :at].astype(np.int64)
    ok = valid_entries(idx, at, n_v, allow)
    counts = np.bincount(idx[ok], minlength=n_v)[:n_v] if n_v else np.zeros(0, np.int64)
    return counts.astype(np.int64), int(ok.size - ok.sum())


def gini_sorted(c):
    """sum_j (2j - n - 1) c_(j) / (n T) over the ascending counts, j = 1 .. n."""
    c = np.sort(np.asarray(c, np.float64))
    n, t = len(c), c.sum()
    if n == 0 or t == 0:
        return float("nan")
    j = np.arange(1, n + 1, dtype=np.float64)
    return float(((2 * j - n - 1) * c).sum() / (n * t))


def gini_pairs(c):
    """The mean-absolute-difference form, sum_ij |c_i - c_j| / (2 n T): O(n^2), small n."""
    c = np.asarray(c, np.float64)
    n, t = len(c), c.sum()
    if n == 0 or t == 0:
        return float("nan")
    return float(np.abs(c[:, None] - c[None, :]).sum() / (2 * n * t))


def gini_leading_zeros(counts, in_cat):
    """The form the kernel uses: rows outside the catalogue keyed 0 and sorted with the rest;
    a count at 0-based position i of the full sort has catalogue rank i + 1 - (n_v - n)."""
    counts = np.asarray(counts, np.float64)
    in_cat = np.asarray(in_cat, bool)
    n_v, n = len(counts), int(in_cat.sum())
    keys = np.sort(np.where(in_cat, counts, 0.0))
    t = keys.sum()
    if n == 0 or t == 0:
        return float("nan")
    rank = np.arange(1, n_v + 1, dtype=np.float64) - (n_v - n)
    return float((np.where(keys > 0, (2 * rank - n - 1) * keys, 0.0)).sum() / (n * t))


def concentration(counts, allow=None):
    """out[7] of als_list_concentration as a list of Python floats."""
    counts = np.asarray(counts, np.int64)
    n_v = len(counts)
    nan = float("nan")
    if n_v == 0:
        return [0.0, 0.0, 0.0, nan, nan, 0.0, 0.0]
    c = np.maximum(counts[unpack_bits(allow, n_v)], 0)
    n, t = len(c), int(c.sum())
    pos = c[c > 0].astype(np.float64)
    ent = float(-((pos / t) * np.log2(pos / t)).sum()) if t > 0 else nan
    return [float(n), float(len(pos)), float(t), gini_sorted(c) if t > 0 else nan, ent,
            float((c * (c - 1) // 2).sum()), float(c.max()) if n else 0.0]


def overlap_pairs(lists):
    """sum over unordered pairs of lists of |A ∩ B| (lists without duplicates)."""
    sets = [set(int(x) for x in l) for l in lists]
    return sum(len(sets[a] & sets[b]) for a in range(len(sets)) for b in range(a + 1, len(sets)))


def novelty(idx, at, n_v, pop, n_pop, allow=None, tail=None):
    """(sums [7], per_row float64 [n_q, 3]) of als_list_novelty."""
    idx = np.asarray(idx)[:, :at].astype(np.int64)
    pop = np.asarray(pop, np.int64)
    ok = valid_entries(idx, at, n_v, allow)
    tail_m = None if tail is None else unpack_bits(tail, n_v)
    n_q = idx.shape[0]
    rows = np.full((n_q, 3), np.nan)
    for r in range(n_q):
        js = idx[r][ok[r]]
        if len(js) == 0:
            continue
        p = pop[js]
        has = p > 0
        if has.any():
            s = 0.0
            for v in p[has]:            # position order
                s += math.log2(n_pop / float(v))
            rows[r, 0] = s / int(has.sum())
        rows[r, 1] = float(p.sum()) / len(js)
        if tail_m is not None:
            rows[r, 2] = float(tail_m[js].sum()) / len(js)
    sums = [float(np.nansum(rows[:, 0])), float((~np.isnan(rows[:, 0])).sum()),
            float(np.nansum(rows[:, 1])), float((~np.isnan(rows[:, 1])).sum()),
            float(np.nansum(rows[:, 2])), float(ok.sum()), float(ok.size - ok.sum())]
    return sums, rows


def long_tail(pop, n_v, head_fraction, in_cat=None):
    """bool [n_v]: the catalogue rows outside the floor(head_fraction n) most-rated ones, ties
    at the cut to the head by ascending row."""
    pop = np.asarray(pop, np.int64)
    cat = np.arange(n_v) if in_cat is None else np.nonzero(np.asarray(in_cat, bool))[0]
    n_head = int(math.floor(head_fraction * len(cat)))
    order = np.argsort(-pop[cat], kind="stable")
    out = np.zeros(n_v, bool)
    out[cat[order[n_head:]]] = True
    return out


def metrics_dict(idx, at, n_v, allow=None, pop=None, n_pop=None, head_fraction=0.2):
    """What engine.list_metrics_rows returns for the same inputs."""
    nan = float("nan")
    counts, skipped = exposure(idx, at, n_v, allow)
    c = concentration(counts, allow)
    n_lists = int(np.asarray(idx).shape[0])
    pairs = n_lists * (n_lists - 1) // 2
    out = {"coverage": c[1] / c[0] if c[0] > 0 else nan, "gini": c[3], "entropy": c[4],
           "effectiveItems": 2.0 ** c[4] if c[4] == c[4] else nan,
           "personalization": 1.0 - c[5] / (pairs * at) if pairs > 0 else nan,
           "topItemShare": c[6] / n_lists if n_lists > 0 else nan,
           "novelty": nan, "averagePopularity": nan, "longTailShare": nan,
           "lists": n_lists, "entries": int(c[2]), "skipped": skipped}
    if pop is not None:
        in_cat = None if allow is None else unpack_bits(allow, n_v)
        tail = pack_bits(long_tail(pop, n_v, head_fraction, in_cat))
        s, _ = novelty(idx, at, n_v, pop, n_pop, allow, tail)
        out["novelty"] = s[0] / s[1] if s[1] > 0 else nan
        out["averagePopularity"] = s[2] / s[3] if s[3] > 0 else nan
        out["longTailShare"] = s[4] / s[3] if s[3] > 0 else nan
    return out
