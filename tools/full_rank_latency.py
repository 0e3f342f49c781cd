#!/usr/bin/env python3
"""Latency of the full-ranking metrics: ALSCore.full_rank_metrics (K9) against the only way
to get the same numbers without it — plain torch on the same GPU: Q_chunk @ V.T in fp32,
chunked to fit memory, the training pairs masked out, then a compare-and-sum per held-out
pair.

Data has the MovieLens-25M shape (datasets.synthetic_config("ml25m")), one pair in five held
out, rank 64, a short implicit fit on the rest; both paths rank every held-out pair among
the items its user has no training pair with (exclude="train").  Each path is warmed up,
then timed with device events around the whole call (both end in a host read, so the events
bracket host work too); the figure is the median of the repeats with the minimum and
maximum beside it.  The two dicts are compared, so that a faster figure is a figure for the
same answer.  One JSON line per path on stdout.

    python tools/full_rank_latency.py [--users 0] [--rank 64] [--repeats 3] [--warmup 1]
                                      [--chunk 4096] [--pair-chunk 2048]

--users N > 0 scores the held-out pairs of the first N users only (both paths).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload  # noqa: E402

_pkgload.load()
from als_mi355x import datasets as D  # noqa: E402
from als_mi355x import engine as E  # noqa: E402
from als_mi355x import filters as F  # noqa: E402

PCT = ("expectedPercentileRank", "meanPercentileRank", "auc", "mrr")


def torch_path(core, hu, hi, chunk, pair_chunk):
    """full_rank_metrics(hu, hi, exclude="train") in plain torch."""
    dev = core.device
    q, o = core.uidx.rows_of(hu).long(), core.iidx.rows_of(hi).long()
    keep = (q >= 0) & (o >= 0)
    dropped = int(hu.numel()) - int(keep.sum().item())
    rows, inv = torch.unique(q[keep], return_inverse=True)
    n, n_v, k = int(rows.numel()), core.n_items, core.rank
    beg, end, col = F.relevance_lists(inv, o[keep], n)
    prow = torch.repeat_interleave(torch.arange(n, device=dev), end - beg)
    pcol = col.long()
    rp, ex = core.train_exclusion(True)
    Q, V = core.U[:, :k].index_select(0, rows), core.V[:, :k]
    above = torch.empty(pcol.numel(), dtype=torch.int64, device=dev)
    tied = torch.empty_like(above)
    n_adm = torch.empty(n, dtype=torch.int64, device=dev)
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        S = Q[r0:r1] @ V.T
        b, e = rp[rows[r0:r1]], rp[rows[r0:r1] + 1]
        er = torch.repeat_interleave(torch.arange(r1 - r0, device=dev), e - b)
        pos = torch.arange(er.numel(), device=dev) - torch.repeat_interleave(
            torch.cumsum(e - b, 0) - (e - b), e - b) + torch.repeat_interleave(b, e - b)
        S[er, ex[pos].long()] = float("-inf")
        n_adm[r0:r1] = n_v - (S == float("-inf")).sum(1)
        p0, p1 = int(beg[r0]), int(end[r1 - 1])
        for a in range(p0, p1, pair_chunk):
            z = min(p1, a + pair_chunk)
            rr, cc = prow[a:z] - r0, pcol[a:z]
            mine = S[rr, cc]
            rowsS = S[rr]
            above[a:z] = (rowsS > mine[:, None]).sum(1)
            tied[a:z] = (rowsS == mine[:, None]).sum(1) - 1
    ok = S.new_ones(pcol.numel(), dtype=torch.bool)  # no training pair is held out
    p = above.double() + 0.5 * tied.double()
    N = n_adm.double()
    m = torch.bincount(prow, minlength=n).double()
    sp = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, prow, p)
    pmin = torch.full((n,), float("inf"), dtype=torch.float64, device=dev).scatter_reduce_(
        0, prow, p, "amin")
    has_pr, has_auc = N > 1, N > m
    pr = p / (N[prow] - 1)
    row_pr = sp / (N - 1) / m
    auc = 1 - (sp - 0.5 * m * (m - 1)) / (m * (N - m))
    return {"expectedPercentileRank": float(pr[has_pr[prow]].mean()),
            "meanPercentileRank": float(row_pr[has_pr].mean()),
            "auc": float(auc[has_auc].mean()), "mrr": float((1 / (1 + pmin)).mean()),
            "rows": n, "pairs": int(ok.sum()), "inadmissible": 0, "dropped": dropped}


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ml25m", choices=sorted(D.CONFIGS))
    ap.add_argument("--users", type=int, default=0)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--pair-chunk", type=int, default=2048)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("full_rank_latency.py needs a HIP GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda")
    u, i, r = D.synthetic_config(a.config, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    held = torch.rand(u.numel(), device=dev, generator=g) < 0.2
    core = E.ALSCore(u[~held], i[~held], r[~held], device=dev)
    core.fit(a.rank, 3, 0.1, implicit=True, alpha=1.0, seed=5)
    hu, hi = u[held], i[held]
    if a.users > 0:
        first = core.uidx.ids()[:a.users].max()
        sel = hu <= first
        hu, hi = hu[sel], hi[sel]
    core.train_exclusion(True)   # built once and cached: not part of either figure
    torch.cuda.synchronize()
    shape = {"users": core.n_users, "items": core.n_items, "train": core.nnz,
             "held_out": int(hu.numel()), "rank": a.rank}
    res = {}
    for name, fn in (("full_rank_metrics (K9)",
                      lambda: core.full_rank_metrics(hu, hi, exclude="train")),
                     ("torch matmul + compare-and-sum",
                      lambda: torch_path(core, hu, hi, a.chunk, a.pair_chunk))):
        out, ms = timed(fn, a.warmup, a.repeats)
        res[name] = out
        print(json.dumps({"path": name, **shape, "repeats": a.repeats,
                          "median_ms": round(statistics.median(ms), 2),
                          "min_ms": round(min(ms), 2), "max_ms": round(max(ms), 2),
                          "result": out}), flush=True)
    x, y = res.values()
    diff = {k: abs(x[k] - y[k]) for k in PCT}
    print(json.dumps({"max_abs_diff_between_paths": diff,
                      "same_counts": all(x[k] == y[k] for k in ("rows", "pairs", "dropped")),
                      "agree_to_1e-6": all(diff[k] <= 1e-6 for k in PCT[:3])}), flush=True)


if __name__ == "__main__":
    main()
