#!/usr/bin/env python3
"""Cost of the training objective (K10) beside the ALS iteration it observes.

On the ML-25M-shaped synthetic ratings (datasets.synthetic_config("ml25m")), for the rank-64
explicit configuration and the rank-128 implicit (alpha 40) one:
  * ms per ALS iteration (core.iterate, device events around `iters` iterations),
  * ms per ALSCore.objective() evaluation (its two rating passes, the Gram product when
    implicit, and the one host sync; host clock around a call that ends in that sync),
  * ms per iteration of fit(..., objective_every=1) against fit(...) with the option off.
The runs of the two fit variants alternate; the figure is the median of the repeats after a
warm-up, with minimum and maximum beside it.  One JSON line per configuration on stdout;
--out writes the list to a file too.

    python tools/objective_cost.py [--iters 3] [--repeats 5] [--warmup 1] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload  # noqa: E402

_pkgload.load()
from als_mi355x import datasets as D  # noqa: E402
from als_mi355x import engine as E  # noqa: E402

CONFIGS = (("ml25m explicit rank 64", 64, False, 1.0), ("ml25m implicit alpha=40 rank 128", 128,
                                                        True, 40.0))


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
            "max_ms": round(max(ms), 3)}


def fit_ms(core, k, iters, imp, alpha, every):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    core.fit(k, iters, 0.1, imp, alpha, seed=1, objective_every=every)   # ends in a sync
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("objective_cost.py needs a HIP GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    u, i, r = D.synthetic_config("ml25m", device=dev)
    core = E.ALSCore(u, i, r, device=dev)
    del u, i, r
    rows = []
    for name, k, imp, alpha in CONFIGS:
        for _ in range(a.warmup):
            fit_ms(core, k, 1, imp, alpha, 1)
        off, on, ev = [], [], []
        for _ in range(a.repeats):           # interleaved: off, on, off, on, ...
            off.append(fit_ms(core, k, a.iters, imp, alpha, 0))
            on.append(fit_ms(core, k, a.iters, imp, alpha, 1))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            val = core.objective(0.1, imp, alpha)
            ev.append((time.perf_counter() - t0) * 1e3)
        row = {"config": name, "rank": k, "implicit": imp, "alpha": alpha, "nnz": core.nnz,
               "n_users": core.n_users, "n_items": core.n_items, "iters": a.iters,
               "repeats": a.repeats, "ms_per_iteration_off": stats(off),
               "ms_per_iteration_every_1": stats(on), "ms_per_evaluation": stats(ev),
               "evaluation_over_iteration": round(statistics.median(ev) / statistics.median(off),
                                                  4),
               "objective": val["objective"], "history": core.objective_history}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
