#!/usr/bin/env python3
"""Cost of explaining recommendations (K11, als_explain) in units of K7: als_fold_in of the
same rows, on the same device, in the same run — one factorisation per row either way.

Factors have the MovieLens-25M shape (59,047 items; the row lengths of the K7 cost run,
tools/fold_in_latency.py: 100 ratings per user, explicit feedback).  The job is 4,096 new
users x the 10 items recommend_new lists for each, at ranks 64 and 128.  Two levels:
  kernel  engine.fold_in_rows / engine.explain_rows over the same ragged rows (one launch
          each), timed with device events;
  engine  ALSCore.fold_in / ALSCore.explain(ratings=) from ids to device tensors (grouping,
          id maps and the status read included).
Each is warmed up, then repeated; the figures are median, minimum and maximum, the two
calls alternating inside one loop so that drift hits both alike.  The explained scores are
checked against the folded factors before anything is timed.

    python tools/explain_cost.py [--users 4096] [--ratings 100] [--targets 10]
                                 [--ranks 64,128] [--repeats 30] [--warmup 3] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload  # noqa: E402

_pkgload.load()
from als_mi355x import engine as E  # noqa: E402
from als_mi355x import filters as F  # noqa: E402

REG = 0.1


def timed_pair(fa, fb, warmup, repeats):
    """Alternate fa and fb; per-call device-event times of each, in ms."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(repeats):
        for ms, fn in zip(out, (fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
    return out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=59047)
    ap.add_argument("--users", type=int, default=4096)
    ap.add_argument("--ratings", type=int, default=100)
    ap.add_argument("--targets", type=int, default=10)
    ap.add_argument("--ranks", default="64,128")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("explain_cost.py needs a HIP GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda")
    results = []
    for rank in (int(x) for x in a.ranks.split(",")):
        rng = np.random.default_rng(rank)
        V = (rng.standard_normal((a.items, rank)) / np.sqrt(rank)).astype(np.float32)
        U = (rng.standard_normal((8, rank)) / np.sqrt(rank)).astype(np.float32)
        core = E.ALSCore.from_factors(np.arange(8), U, np.arange(a.items), V)
        u = torch.as_tensor(np.repeat(np.arange(a.users, dtype=np.int32), a.ratings)).to(dev)
        i = torch.as_tensor(rng.integers(0, a.items, a.users * a.ratings).astype(np.int32)).to(dev)
        r = torch.as_tensor(rng.integers(1, 11, a.users * a.ratings).astype(np.float32) / 2).to(dev)
        keys, rec, _ = core.recommend_new(u, i, r, a.targets, reg=REG)
        pu = keys.repeat_interleave(rec.shape[1])
        pi = rec.reshape(-1)

        # kernel level: the same ragged rows into both entry points
        _, row_ptr, col, val = F.ragged_rows(u, core.iidx.rows_of(i), r)
        order, tgt_ptr = E.group_pairs(torch.searchsorted(keys, pu), int(keys.numel()))
        tgt = core.iidx.rows_of(pi)[order].to(torch.int32).contiguous()
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        args = (row_ptr, col, val, core.V, core.n_items, rank, REG, False, 1.0, None)
        fold = lambda: E.fold_in_rows(*args, status, core.ws)
        expl = lambda: E.explain_rows(*args, tgt_ptr, tgt, a.targets, status, core.ws)
        X, _ = fold()
        sc, _, con, _ = expl()
        want = (X[:, :rank].double().repeat_interleave(a.targets, 0)
                * core.V[tgt.long(), :rank].double()).sum(1)
        diff = float((sc.double() - want).abs().max())
        assert int(status.item()) == 0 and diff < 1e-5, diff
        k_fold, k_expl = timed_pair(fold, expl, a.warmup, a.repeats)
        e_fold, e_expl = timed_pair(
            lambda: core.fold_in(u, i, r, reg=REG),
            lambda: core.explain(pu, pi, a.targets, reg=REG, ratings=(u, i, r)),
            a.warmup, a.repeats)
        res = {"rank": rank, "users": a.users, "ratings_per_user": a.ratings,
               "targets_per_user": a.targets, "top_n": a.targets, "items": a.items,
               "repeats": a.repeats, "max_abs_score_diff_vs_fold_in": diff,
               "kernel": {"fold_in": stats(k_fold), "explain": stats(k_expl),
                          "explain_over_fold_in": round(statistics.median(k_expl)
                                                        / statistics.median(k_fold), 3)},
               "engine": {"fold_in": stats(e_fold), "explain": stats(e_expl),
                          "explain_over_fold_in": round(statistics.median(e_expl)
                                                        / statistics.median(e_fold), 3)}}
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.json:
        doc = {"tool": "tools/explain_cost.py " + " ".join(sys.argv[1:]),
               "device": torch.cuda.get_device_name(0),
               "method": "device events around each call, fold_in and explain alternating in "
                         "one loop; median / min / max of the repeats after the warm-up",
               "results": results}
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
