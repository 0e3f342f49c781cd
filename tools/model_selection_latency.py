#!/usr/bin/env python3
"""Latency of the reference's rank sweep: TrainValidationSplit (one engine per training
split, K8 scoring) against the hand loop a caller had before it — ALS.fit per rank, which
rebuilds both rating blocks (K1) every time, plus ALSModel.rmse.

The sweep is the reference's (RecommenderSystem.py:136-159): ranks 4 / 8 / 12, 5 iterations,
lambda 0.1, on the script-as-written shape (6,040 x 3,706, 292,716 ratings from
datasets.synthetic).  Both paths get the same train / validation split, made once outside
the timed region (the tuner's own split); each path is timed end to end with a host clock
around work that ends in a device synchronise — the frames start on the host in both, so
uploads, K1, the fits and the scoring are all inside.  The tuner's final refit of the best
rank on the whole dataset has no counterpart in the hand loop and is timed separately
(`tvs_with_refit`).  The figure is the median of the repeats after a warm-up, with the
minimum and maximum beside it.  The validation RMSEs of the two paths are compared, so that
a faster figure is a figure for the same answer.  One JSON line per path on stdout.

    python tools/model_selection_latency.py [--ranks 4,8,12] [--iters 5] [--reg 0.1]
                                            [--repeats 7] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload  # noqa: E402

_pkgload.load()
from als_mi355x import datasets  # noqa: E402
from als_mi355x.ml import tuning as T  # noqa: E402
from als_mi355x.ml.evaluation import RegressionEvaluator  # noqa: E402
from als_mi355x.ml.recommendation import ALS  # noqa: E402


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def main():
    import pandas as pd
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="4,8,12")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reg", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("model_selection_latency.py needs a HIP GPU: a timing taken anywhere else says "
                 "nothing")
    if a.repeats < 5:
        sys.exit("--repeats must be at least 5")
    ranks = [int(x) for x in a.ranks.split(",")]
    n_u, n_i, nnz, half, seed = datasets.CONFIGS["ml1m_lab4"]
    u, i, r = datasets.synthetic(n_u, n_i, nnz, seed=seed, half_stars=half)
    df = pd.DataFrame({"user": u.cpu().numpy(), "item": i.cpu().numpy(),
                       "rating": r.cpu().numpy()})
    base = dict(maxIter=a.iters, regParam=a.reg, seed=5, coldStartStrategy="drop")
    grid = T.ParamGridBuilder().addGrid(ALS.rank, ranks).build()
    ev = RegressionEvaluator(labelCol="rating")
    tvs = T.TrainValidationSplit(ALS(**base), grid, ev, trainRatio=0.75, seed=0)
    tr, va = tvs.split(len(df))
    train, valid = T._take(df, tr), T._take(df, va)

    def shared():   # what TrainValidationSplit.fit does before its refit
        return T._fit_and_score(tvs.estimator, grid, ev, train, valid, False)[0]

    def hand():
        return [ALS(rank=k, **base).fit(train).rmse(valid) for k in ranks]

    def with_refit():
        return tvs.fit(df).validationMetrics

    res = {}
    for name, fn in (("tvs_shared_engine", shared), ("hand_loop", hand),
                     ("tvs_with_refit", with_refit)):
        out, ms = timed(fn, a.warmup, a.repeats)
        res[name] = (out, statistics.median(ms))
        print(json.dumps({"path": name, "ranks": ranks, "iters": a.iters, "reg": a.reg,
                          "train": len(train), "valid": len(valid), "repeats": a.repeats,
                          "median_ms": round(statistics.median(ms), 3),
                          "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                          "validation_rmse": [round(x, 9) for x in out]}), flush=True)
    x, y = np.array(res["tvs_shared_engine"][0]), np.array(res["hand_loop"][0])
    print(json.dumps({"max_rel_rmse_diff_between_paths": float(np.abs(x / y - 1).max()),
                      "hand_over_shared": round(res["hand_loop"][1] / res["tvs_shared_engine"][1],
                                                4)}), flush=True)


if __name__ == "__main__":
    main()
