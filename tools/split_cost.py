#!/usr/bin/env python3
"""Cost of the per-user holdout (K20, ALSCore.split) beside the host split it replaces
(DESIGN.md section K20).

On the ML-25M-shaped synthetic ratings (datasets.synthetic_config("ml25m")), for a count-1
holdout, a 0.2 fraction and one fold of 3, after a warm-up of every call:
  (a) the K20 kernels alone, per side (device events): als_split_anchor and
      als_split_eligible on either side, als_split_thresholds on either side as the selecting
      one, als_split_mark on both sides of a user-side split;
  (b) ALSCore.split in full (host clock: it reads the kept count back and shrinks id maps);
  (c) the route without K20 for a validation part of the same size: TrainValidationSplit.split
      (datasets.random_split on the host) + tuning._take of both parts from a dict of numpy
      columns + make_engine of the training part (host copy to the device, K1);
  (d) the bytes each kernel must move at the least — anchor / eligible / thresholds: 4 B per
      stored entry, the row pointer, the id and anchor tables and the per-row outputs; mark:
      the same plus one bit per entry and the threshold table — over the bandwidth of a 1 GiB
      device-to-device copy in this run, and the ratio of (a) to that floor.
Figures are the median of the repeats with minimum and maximum beside it.  Clocks are taken as
found.  Writes one JSON document.

    python tools/split_cost.py --out profiles/k20_split_cost.json
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

SEED = 7
MODES = {"count1": dict(count=1), "fraction0.2": dict(fraction=0.2), "fold0of3": dict(fold=(0, 3))}


def _events(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner, out


def _host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _stats(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(min(ts)), 4),
            "max_ms": round(float(max(ts)), 4)}


def _repeat(timer, fn, repeats):
    ts, out = [], None
    for rep in range(repeats + 1):     # the first pass warms everything up
        t, out = timer(fn)
        if rep:
            ts.append(t)
    return ts, out


def kernels(core, kw, repeats, bw):
    """(a) and (d): every K20 entry point alone, on the side(s) it can run on."""
    ws = core.ws
    mode, value = E.check_split_args(**kw)
    uids, iids = core.uidx.ids().contiguous(), core.iidx.ids().contiguous()
    side = {"user": (core.user_block, core.item_block, uids, iids, True),
            "item": (core.item_block, core.user_block, iids, uids, False)}
    out = {}
    anchors, thr_user = {}, None
    for name, (b, o, ids, oids, are_users) in side.items():
        n, m, nnz = b.n_rows, o.n_rows, b.nnz
        ts, anchors[name] = _repeat(_events, lambda: E.split_anchor(
            b.row_ptr, b.col, m, ids, oids, are_users, SEED, ws), repeats)
        out[f"anchor_{name}"] = dict(_stats(ts), floor_bytes=4 * nnz + 8 * (n + 1) + 8 * n + 4 * m)
    for name, (b, o, ids, oids, are_users) in side.items():
        n, m, nnz = b.n_rows, o.n_rows, b.nnz
        anchor = anchors["item" if name == "user" else "user"]   # of the other side
        ts, e = _repeat(_events, lambda: E.split_eligible(b.row_ptr, b.col, m, anchor), repeats)
        out[f"eligible_{name}"] = dict(_stats(ts), floor_bytes=4 * nnz + 8 * (n + 1) + 4 * m + 4 * n)
        lo, hi = E.split_windows(e, mode, value, 1)
        ts, thr = _repeat(_events, lambda: E.split_thresholds(
            b.row_ptr, b.col, m, ids, oids, are_users, SEED, anchor, lo, hi, ws), repeats)
        lens = b.row_ptr[1:] - b.row_ptr[:-1]
        cap = E.split_row_cap()
        out[f"thresholds_{name}"] = dict(
            _stats(ts), floor_bytes=4 * nnz + 8 * (n + 1) + 4 * n + 8 * m + 8 * n + 24 * n,
            rows_over_cap=int((lens > cap).sum()), entries_over_cap=int(lens[lens > cap].sum()),
            longest_row=int(lens.max()))
        if name == "user":
            thr_user = thr
    anchor = anchors["item"]
    for name, (b, o, ids, oids, are_users) in side.items():
        n, m, nnz = b.n_rows, o.n_rows, b.nnz
        ts, _ = _repeat(_events, lambda: E.split_mark(
            b.row_ptr, b.col, m, ids, oids, are_users, SEED, are_users, thr_user, anchor, ws),
            repeats)
        out[f"mark_{name}"] = dict(_stats(ts), floor_bytes=4 * nnz + nnz // 8 + 16 * (n + 1)
                                   + 4 * (n + m) + 24 * core.n_users + 4 * core.n_items)
    for v in out.values():
        v["byte_floor_ms"] = round(v["floor_bytes"] / bw * 1e3, 4)
        v["over_byte_floor"] = round(v["median_ms"] / v["byte_floor_ms"], 2)
    out["selection_user_side_sum_ms"] = round(sum(out[k]["median_ms"] for k in (
        "anchor_item", "eligible_user", "thresholds_user", "mark_user", "mark_item")), 4)
    return out


def host_route(cols, train_ratio, repeats):
    """(c): the split every tuner makes without K20, step by step (host clock)."""
    from als_mi355x.ml.recommendation import ALS
    from als_mi355x.ml.tuning import TrainValidationSplit, _take
    est = ALS()
    tv = TrainValidationSplit(est, [{}], None, trainRatio=train_ratio, seed=SEED)
    n = len(cols["user"])
    names = ("random_split", "take", "make_engine", "total")
    ts = {k: [] for k in names}
    held = 0
    for rep in range(repeats + 1):
        t_s, (tr, va) = _host(lambda: tv.split(n))
        t_t, (train, val) = _host(lambda: (_take(cols, tr), _take(cols, va)))
        t_e, core = _host(lambda: E.make_engine(*est._columns(train)))
        held = len(va)
        if rep:
            for k, v in zip(names, (t_s, t_t, t_e, t_s + t_t + t_e)):
                ts[k].append(v)
        del core, train, val
    return dict({k: _stats(v) for k, v in ts.items()}, held_out=held, train_ratio=train_ratio)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--config", default="ml25m")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("split_cost.py needs a HIP GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    u, i, r = D.synthetic_config(args.config, device=dev)
    core = E.ALSCore(u, i, r, device=dev)
    cols = {"user": u.cpu().numpy(), "item": i.cpu().numpy(), "rating": r.cpu().numpy()}
    del u, i, r
    src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    cp = [_events(lambda: dst.copy_(src), 4)[0] for _ in range(args.repeats)]
    bw = 2 * src.numel() / (float(np.median(cp)) * 1e-3)
    del src, dst
    doc = {"tool": "tools/split_cost.py", "device": "MI355X (gfx950), one GPU",
           "config": args.config, "nnz": core.nnz, "n_users": core.n_users,
           "n_items": core.n_items, "row_cap": E.split_row_cap(), "repeats": args.repeats,
           "host_repeats": args.host_repeats,
           "method": "device events around each K20 entry point, host clock around ALSCore.split "
                     "and around the host route's steps; median / min / max of the repeats "
                     "after one warm-up pass; clocks as found",
           "copy_bandwidth_TB_per_s": round(bw / 1e12, 3), "modes": {}}
    for name, kw in MODES.items():
        entry = {"kernels": kernels(core, kw, args.repeats, bw)}
        ts, (train, held) = _repeat(_host, lambda: core.split(seed=SEED, **kw), args.repeats)
        n_held = int(held[0].numel())
        entry["core_split_call"] = dict(_stats(ts), held_out=n_held, kept=train.nnz)
        del train, held
        entry["host_route"] = host_route(cols, 1.0 - n_held / core.nnz, args.host_repeats)
        entry["host_route_over_core_split"] = round(
            entry["host_route"]["total"]["median_ms"] / entry["core_split_call"]["median_ms"], 1)
        doc["modes"][name] = entry
        print(json.dumps({name: entry}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
