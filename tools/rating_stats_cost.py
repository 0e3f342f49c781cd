#!/usr/bin/env python3
"""Cost of the rating statistics and of the bias baseline (K16) beside what they stand next to
(DESIGN.md section K16).

On the ML-25M-shaped synthetic ratings (datasets.synthetic_config("ml25m")), after a warm-up of
every call, device-event times of
  * als_row_moments without a gather table on the user side and on the item side,
  * als_row_moments with one (fp64, the other side's rows), both sides,
  * the same numbers from torch on the same device: n, sum and M2 per row by index_add_ in fp64
    over an expanded row-id vector (torch.repeat_interleave of the row lengths, built outside
    the timed window) and min / max by segment_reduce; with the gather, `val - other[col]` first,
  * one ALSCore.fit_baseline("bias", sweeps=10) (20 sweeps with gather, their updates, the
    objective and the host syncs of the history; host clock around a call that ends in a sync),
  * one explicit rank-64 ALS iteration (core.iterate),
  * a device-to-device copy of 1 GiB, whose bytes read + written over its time is the copy
    bandwidth of this run.
The byte floor of a sweep is nnz * 4 bytes (val alone) without a gather and nnz * 8 (val and col)
with one, over that bandwidth.  A timed window is `inner` back-to-back calls, the calls
alternate inside every repeat, and the figure is the median of the repeats with minimum and
maximum beside it.  Clocks are taken as found.  Writes one JSON document.

    python tools/rating_stats_cost.py --out profiles/k16_rating_stats_cost.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload  # noqa: E402

_pkgload.load()
from als_mi355x import datasets as D  # noqa: E402
from als_mi355x import engine as E  # noqa: E402


def _time(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def _stats(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(min(ts)), 4),
            "max_ms": round(float(max(ts)), 4)}


def torch_moments(block, rows, other=None):
    """n, sum, M2, min, max per row with torch ops, fp64."""
    e = block.val.double()
    if other is not None:
        e = e - other[block.col.long()]
    n_rows = block.n_rows
    lengths = block.row_ptr[1:] - block.row_ptr[:-1]
    n = lengths.double()
    s = torch.zeros(n_rows, dtype=torch.float64, device=e.device).index_add_(0, rows, e)
    mean = s / n.clamp(min=1)
    d = e - mean[rows]
    m2 = torch.zeros(n_rows, dtype=torch.float64, device=e.device).index_add_(0, rows, d * d)
    lo = torch.segment_reduce(e, "min", lengths=lengths)
    hi = torch.segment_reduce(e, "max", lengths=lengths)
    return n, s, m2, lo, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--config", default="ml25m")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rating_stats_cost.py needs a HIP GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    u, i, r = D.synthetic_config(args.config, device=dev)
    core = E.ALSCore(u, i, r, device=dev)
    del u, i, r
    ws = E.Workspace(dev)
    g = torch.Generator(device="cuda").manual_seed(1)
    sides = {"user": (core.user_block, core.n_items), "item": (core.item_block, core.n_users)}
    calls, checks = {}, []
    for name, (block, n_cols) in sides.items():
        other = torch.randn(n_cols, dtype=torch.float64, device=dev, generator=g)
        rows = torch.repeat_interleave(torch.arange(block.n_rows, device=dev),
                                       block.row_ptr[1:] - block.row_ptr[:-1])
        mom = torch.empty((block.n_rows, 5), dtype=torch.float64, device=dev)
        tot = torch.empty(5, dtype=torch.float64, device=dev)
        calls[f"row_moments_{name}"] = (
            lambda b=block, c=n_cols, m=mom, t=tot: E.row_moments(b, c, ws, moments=m, total=t))
        calls[f"row_moments_{name}_gather"] = (
            lambda b=block, c=n_cols, o=other, m=mom, t=tot:
            E.row_moments(b, c, ws, other=o, moments=m, total=t))
        calls[f"torch_{name}"] = lambda b=block, rw=rows: torch_moments(b, rw)
        calls[f"torch_{name}_gather"] = lambda b=block, rw=rows, o=other: torch_moments(b, rw, o)
        checks.append((name, block, n_cols, other, rows))
    src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    calls["copy_1GiB"] = lambda: dst.copy_(src)
    core.init_factors(64, seed=1)
    core.schedule_for(False)
    calls["als_iteration_rank64"] = lambda: core.iterate(0.1)

    agreement = {}
    for name, block, n_cols, other, rows in checks:      # the two forms compute one thing
        for tag, o in (("", None), ("_gather", other)):
            mom, _ = E.row_moments(block, n_cols, ws, other=o)
            n, s, m2, lo, hi = torch_moments(block, rows, o)
            has = n > 0
            agreement[f"{name}{tag}"] = {
                "count_equal": bool(torch.equal(mom[:, 0], n)),
                "min_max_equal": bool(torch.equal(mom[has][:, 3], lo[has])
                                      and torch.equal(mom[has][:, 4], hi[has])),
                "sum_max_abs_diff": float((mom[:, 1] - s).abs().max()),
                "m2_max_rel_diff": float(((mom[:, 2] - m2).abs() / m2.clamp(min=1e-300))[has]
                                         .max())}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    ts = {key: [] for key in calls}
    fit_ms = []
    core.fit_baseline("bias", sweeps=10)
    for _ in range(args.repeats):
        for key, fn in calls.items():
            ts[key].append(_time(fn, 2 if key.startswith(("als_", "torch_")) else args.inner))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        base = core.fit_baseline("bias", sweeps=10)     # ends in the history's host syncs
        torch.cuda.synchronize()
        fit_ms.append((time.perf_counter() - t0) * 1e3)
    med = lambda k: float(np.median(ts[k]))
    bw = 2 * src.numel() / (med("copy_1GiB") * 1e-3)          # bytes read + written per second
    doc = {"tool": "tools/rating_stats_cost.py", "device": "MI355X (gfx950), one GPU",
           "config": args.config, "nnz": core.nnz, "n_users": core.n_users,
           "n_items": core.n_items, "task_ratings": E.rating_stats_task(),
           "rows_per_workgroup": E.rating_stats_group_rows(), "repeats": args.repeats,
           "calls_per_window": args.inner,
           "method": "device events around back-to-back calls (2 per window for the torch forms "
                     "and the ALS iteration), per-call time = window / calls; median / min / max "
                     "of the repeats after a warm-up of each call; the calls alternate inside a "
                     "repeat; fit_baseline by the host clock around a call that ends in a sync; "
                     "clocks as found",
           "copy_bandwidth_TB_per_s": round(bw / 1e12, 3),
           "agreement_with_torch": agreement,
           **{key: _stats(t) for key, t in ts.items()},
           "fit_baseline_bias_10_sweeps": _stats(fit_ms),
           "baseline_history": base.history}
    for name in sides:
        for tag, bytes_per in (("", 4), ("_gather", 8)):
            key = f"row_moments_{name}{tag}"
            floor_ms = core.nnz * bytes_per / bw * 1e3
            doc[key]["byte_floor_ms"] = round(floor_ms, 4)
            doc[key]["over_byte_floor"] = round(med(key) / floor_ms, 2)
            doc[key]["over_torch"] = round(med(key) / med(f"torch_{name}{tag}"), 4)
    doc["fit_baseline_over_als_iteration"] = round(
        float(np.median(fit_ms)) / med("als_iteration_rank64"), 3)
    print(json.dumps(doc), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
