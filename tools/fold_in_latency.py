#!/usr/bin/env python3
"""Latency of serving new users: ALSCore.fold_in (K7) against the path a caller had before
it — build_index + build_block + solve_half over the new rows with V as Y_src.

Factors have the MovieLens-25M shape (59,047 items, rank 64, explicit feedback); the jobs
are 1 new user x 100 ratings and 10,000 new users x 100 ratings.  Each (job, path) is
warmed up, then timed with device events around the whole call (both paths end in a host
read of a device word, so the events bracket host work too); the figure is the median of
the repeats, with the minimum and maximum beside it.  The two paths' results are compared
per row, so that a faster figure is a figure for the same answer.  One JSON line per
(job, path) on stdout.

    python tools/fold_in_latency.py [--items 59047] [--rank 64] [--ratings 100]
                                    [--users 1,10000] [--repeats 20] [--warmup 3]
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

REG = 0.1


def new_users(n_users, n_ratings, n_items, seed):
    rng = np.random.default_rng(seed)
    u = np.repeat(np.arange(n_users, dtype=np.int32), n_ratings)
    i = rng.integers(0, n_items, n_users * n_ratings).astype(np.int32)
    r = rng.integers(1, 11, n_users * n_ratings).astype(np.float32) / 2
    dev = torch.device("cuda")
    return tuple(torch.as_tensor(x).to(dev) for x in (u, i, r))


def fold_in_path(core, u, i, r):
    _, X, _ = core.fold_in(u, i, r, reg=REG)
    return X


def solve_half_path(core, u, i, r):
    """The same rows through K1 + K2/K3: a user index and CSR block over the new ratings,
    then one half-sweep with the model's V as the source factors."""
    ws = E.Workspace(core.device)
    uidx = E.build_index(u, int(u.max()) + 1, ws)
    block = E.build_block(u, uidx, core.iidx.keys(i), core.iidx, r, ws,
                          E.chunk_for(core.rank, False))
    X = torch.empty((uidx.n, E.ld_for(core.rank)), dtype=torch.float32, device=core.device)
    status = torch.zeros(1, dtype=torch.int32, device=core.device)
    E.solve_half(block, core.V, X, core.rank, REG, False, 1.0, None, status, ws)
    E.raise_status(int(status.item()))
    return X[:, :core.rank]


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
    ap.add_argument("--items", type=int, default=59047)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--ratings", type=int, default=100)
    ap.add_argument("--users", default="1,10000")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fold_in_latency.py needs a HIP GPU: a timing taken anywhere else says nothing")
    rng = np.random.default_rng(0)
    V = (rng.standard_normal((a.items, a.rank)) / np.sqrt(a.rank)).astype(np.float32)
    U = (rng.standard_normal((8, a.rank)) / np.sqrt(a.rank)).astype(np.float32)
    core = E.ALSCore.from_factors(np.arange(8), U, np.arange(a.items), V)
    for n_users in (int(x) for x in a.users.split(",")):
        u, i, r = new_users(n_users, a.ratings, a.items, seed=n_users)
        res = {}
        for name, path in (("fold_in", fold_in_path), ("index+block+solve_half", solve_half_path)):
            X, ms = timed(lambda: path(core, u, i, r), a.warmup, a.repeats)
            res[name] = X.double()
            print(json.dumps({"job": f"{n_users} users x {a.ratings} ratings", "path": name,
                              "items": a.items, "rank": a.rank, "repeats": a.repeats,
                              "median_ms": round(statistics.median(ms), 4),
                              "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}),
                  flush=True)
        x, y = res.values()
        err = (torch.linalg.vector_norm(x - y, dim=1)
               / torch.linalg.vector_norm(y, dim=1).clamp(min=1e-6)).max()
        print(json.dumps({"job": f"{n_users} users x {a.ratings} ratings",
                          "max_rel_row_diff_between_paths": float(err)}), flush=True)


if __name__ == "__main__":
    main()
