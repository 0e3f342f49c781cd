#!/usr/bin/env python3
"""Cost of the nonnegative half-sweeps (K13, als_nnls_rows) at the flagship shape.

Data has the MovieLens-25M shape (datasets.synthetic_config("ml25m")), rank 64, explicit
feedback, regParam 0.1.  The factors are those of a short nonnegative fit, so the solver sees
the systems a fit gives it; each half-sweep is then repeated from the same other-side factors
(a half-sweep reads one table and writes the other, so repeats do the same work).  Reported:
ms per item and per user half-sweep with nonnegative=True, the mean and maximum of the solver's
iteration counts, and — for context only: it solves a different problem — the same half-sweeps
of the Cholesky path on the factors of a Cholesky fit of the same length.  Each figure is the
median of the repeats after the warm-ups, timed with device events.  One JSON document on stdout
and, with --out, in a file.

    python tools/nnls_cost.py [--config ml25m] [--rank 64] [--fit-iters 2] [--repeats 20]
                              [--warmup 3] [--out profiles/k13_nnls_cost.json]
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

REG = 0.1


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
            "max_ms": round(max(ms), 3)}


def iteration_counts(core, block, Y, n_src):
    ws = E.Workspace(core.device)
    _, _, it = E.nnls_rows(block.row_ptr, block.col, block.val, Y, n_src, core.rank, REG, False,
                           1.0, None, ws, E.DEFAULT_CHUNK, iters=True)
    it = it.double()
    return {"mean": round(float(it.mean()), 3), "max": int(it.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ml25m", choices=sorted(D.CONFIGS))
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--fit-iters", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nnls_cost.py needs a HIP GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    u, i, r = D.synthetic_config(a.config, device=dev)
    core = E.ALSCore(u, i, r, device=dev)
    del u, i, r
    k = a.rank
    out = {"shape": a.config, "n_users": core.n_users, "n_items": core.n_items, "nnz": core.nnz,
           "rank": k, "reg": REG, "feedback": "explicit", "fit_iters": a.fit_iters,
           "repeats": a.repeats, "warmup": a.warmup, "chunk": E.DEFAULT_CHUNK,
           "device": torch.cuda.get_device_name(dev)}

    core.fit(k, a.fit_iters, REG, seed=5, nonnegative=True)
    out["nnls"] = {
        "item_half_sweep": timed(lambda: core.half_sweep_items(REG, nonnegative=True), a.warmup,
                                 a.repeats),
        "user_half_sweep": timed(lambda: core.half_sweep_users(REG, nonnegative=True), a.warmup,
                                 a.repeats),
        "item_iterations": iteration_counts(core, core.item_block, core.U, core.n_users),
        "user_iterations": iteration_counts(core, core.user_block, core.V, core.n_items),
        "zero_fraction_U": round(float((core.U[:, :k] == 0).double().mean()), 4),
        "zero_fraction_V": round(float((core.V[:, :k] == 0).double().mean()), 4)}

    core.fit(k, a.fit_iters, REG, seed=5)
    out["cholesky_context"] = {
        "item_half_sweep": timed(lambda: core.half_sweep_items(REG), a.warmup, a.repeats),
        "user_half_sweep": timed(lambda: core.half_sweep_users(REG), a.warmup, a.repeats)}
    core.check_status()
    doc = json.dumps(out, indent=1)
    print(doc, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
