#!/usr/bin/env python3
"""Cost of adding ratings to a fitted core (K17, ALSCore.add_ratings / refresh / refit) beside
what it replaces.

On the ML-25M-shaped synthetic ratings (datasets.synthetic_config("ml25m")), for batches of 12,
1e4 and 1e6 ratings (12: one new user; the others: random users, one in a hundred of them new,
and random known items), after a warm-up of every call:
  * the steps of add_ratings, each by the host clock around a step that ends in a sync, because
    each holds host syncs of its own: growing both id maps, K1 on the batch (both sides),
    K17 on each side (device events: it has no sync), scheduling both sides again;
  * against them the parent's way: ALSCore(concat(old, batch)) from device tensors, and K1
    alone (als_csr_build of one side of the concatenation, device events);
  * K17 against its byte floor: 8 B read and 8 B written per output entry plus the three row
    pointers, over the bandwidth of a 1 GiB device-to-device copy in this run;
  * refresh (the touched rows only) against one full iteration, rank 64, explicit;
  * the objective (K10) after one and two warm iterations (add the 1e6 batch to a core fitted
    --fit-iters iterations, then refit) against the history of a cold fit on the merged data.
Figures are the median of the repeats with minimum and maximum beside it; the calls alternate
inside a repeat.  Clocks are taken as found.  Writes one JSON document.

    python tools/update_cost.py --out profiles/k17_update_cost.json
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


def make_batch(core, n, gen):
    dev = core.device
    uids, iids = core.uidx.ids(), core.iidx.ids()
    if n <= 100:   # the reference's case: one new user
        u = torch.full((n,), int(uids.max()) + 1, dtype=torch.int32, device=dev)
    else:
        u = uids[torch.randint(0, uids.numel(), (n,), device=dev, generator=gen)].clone()
        fresh = torch.rand(n, device=dev, generator=gen) < 0.01
        u[fresh] = int(uids.max()) + 1 + torch.randint(0, max(n // 200, 1), (int(fresh.sum()),),
                                                       device=dev, generator=gen).int()
    i = iids[torch.randint(0, iids.numel(), (n,), device=dev, generator=gen)]
    r = (torch.randint(1, 11, (n,), device=dev, generator=gen) * 0.5).float()
    return u, i, r


def steps(core, batch, repeats):
    """add_ratings taken apart on a core that is left as it is."""
    u, i, r = batch
    ws = core.ws
    ub, ib = core.user_block, core.item_block
    ts = {k: [] for k in ("grow_index", "k1_batch", "k17_user", "k17_item", "reschedule",
                          "add_ratings_sum")}
    for rep in range(repeats + 1):
        t_idx, (gu, gi) = _host(lambda: (E.grow_index(core.uidx, u, ws),
                                         E.grow_index(core.iidx, i, ws)))
        (uidx, umap, _), (iidx, imap, _) = gu, gi
        uk, ik = uidx.keys(u), iidx.keys(i)
        t_k1, (au, ai) = _host(lambda: (E.build_csr(uk, uidx, ik, iidx, r, ws),
                                        E.build_csr(ik, iidx, uk, uidx, r, ws)))
        t_mu, mu = _events(lambda: E.merge_csr(ub.row_ptr, ub.col, ub.val, ib.n_rows, umap, imap,
                                               *au))
        t_mi, mi = _events(lambda: E.merge_csr(ib.row_ptr, ib.col, ib.val, ub.n_rows, imap, umap,
                                               *ai))
        nnz = core.nnz + int(u.numel())
        t_s, _ = _host(lambda: (E.schedule_block(uidx.n, nnz, *mu, ws, ub.chunk),
                                E.schedule_block(iidx.n, nnz, *mi, ws, ib.chunk)))
        if rep:   # the first pass warms everything up
            for k, v in zip(ts, (t_idx, t_k1, t_mu, t_mi, t_s, t_idx + t_k1 + t_mu + t_mi + t_s)):
                ts[k].append(v)
        del mu, mi
    return ts, (ub.n_rows, uidx.n, ib.n_rows, iidx.n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--config", default="ml25m")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--fit-iters", type=int, default=10)
    ap.add_argument("--batches", default="12,10000,1000000")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("update_cost.py needs a HIP GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    u, i, r = D.synthetic_config(args.config, device=dev)
    core = E.ALSCore(u, i, r, device=dev)
    gen = torch.Generator(device="cuda").manual_seed(1)
    src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    copy = [_events(lambda: dst.copy_(src), 4)[0] for _ in range(args.repeats)]
    bw = 2 * src.numel() / (float(np.median(copy)) * 1e-3)
    del src, dst
    doc = {"tool": "tools/update_cost.py", "device": "MI355X (gfx950), one GPU",
           "config": args.config, "nnz": core.nnz, "n_users": core.n_users,
           "n_items": core.n_items, "merge_tile": E.csr_merge_tile(), "repeats": args.repeats,
           "method": "host clock around steps that end in a sync (they hold host syncs), device "
                     "events around K17 and K1 alone; median / min / max of the repeats after "
                     "one warm-up pass; clocks as found",
           "copy_bandwidth_TB_per_s": round(bw / 1e12, 3), "batches": {}}
    batches = {}
    for n in (int(x) for x in args.batches.split(",")):
        batch = make_batch(core, n, gen)
        batches[n] = batch
        ts, (nu0, nu1, ni0, ni1) = steps(core, batch, args.repeats)
        cat = [torch.cat([a, b]) for a, b in zip((u, i, r), batch)]
        rebuild, k1_side = [], []
        for rep in range(args.repeats + 1):
            t, fresh = _host(lambda: E.ALSCore(*cat, device=dev))
            t1, _ = _events(lambda: E.build_csr(fresh.uidx.keys(cat[0]), fresh.uidx,
                                                fresh.iidx.keys(cat[1]), fresh.iidx, cat[2],
                                                fresh.ws))
            if rep:
                rebuild.append(t)
                k1_side.append(t1)
            del fresh
        nnz_out = core.nnz + n
        entry = {k: _stats(v) for k, v in ts.items()}
        entry["rebuild_core_from_concat"] = _stats(rebuild)
        entry["k1_one_side_of_concat"] = _stats(k1_side)
        for side, (n0, n1) in (("user", (nu0, nu1)), ("item", (ni0, ni1))):
            floor = (16 * nnz_out + 8 * (n0 + 1) + 16 * (n1 + 1)) / bw * 1e3
            key = f"k17_{side}"
            entry[key]["byte_floor_ms"] = round(floor, 4)
            entry[key]["over_byte_floor"] = round(entry[key]["median_ms"] / floor, 2)
            entry[key]["k1_over_k17"] = round(float(np.median(k1_side))
                                              / entry[key]["median_ms"], 2)
        entry["rebuild_over_add_ratings"] = round(
            float(np.median(rebuild)) / entry["add_ratings_sum"]["median_ms"], 2)
        entry["new_users"], entry["new_items"] = nu1 - nu0, ni1 - ni0
        doc["batches"][str(n)] = entry
        del cat
        print(json.dumps({str(n): entry}), flush=True)

    # refresh against an iteration, and the warm start against a cold fit
    reg = 0.1
    n_big = max(batches)
    del core
    for n in sorted(batches):   # a core of its own per batch: the touched rows are the batch's
        core = E.ALSCore(u, i, r, device=dev)
        core.fit(args.rank, args.fit_iters, reg, seed=1, objective_every=1)
        entry = doc["batches"][str(n)]
        if n == n_big:
            doc["first_fit_history"] = [v for _, v in core.objective_history]
        it_ms = [_events(lambda: core.iterate(reg), 2)[0] for _ in range(args.repeats)]
        entry[f"als_iteration_rank{args.rank}"] = _stats(it_ms)
        core.fit(args.rank, args.fit_iters, reg, seed=1)
        t_add, info = _host(lambda: core.add_ratings(*batches[n], seed=1))
        entry["add_ratings_with_factors_ms"] = round(t_add, 3)
        entry["touched_users"], entry["touched_items"] = (int(info["touched_users"].numel()),
                                                          int(info["touched_items"].numel()))
        keep = (core.U.clone(), core.V.clone())
        core.refresh()
        ref_ms = []
        for _ in range(args.repeats):
            core.U.copy_(keep[0])
            core.V.copy_(keep[1])
            ref_ms.append(_host(core.refresh)[0])
        core.U.copy_(keep[0])
        core.V.copy_(keep[1])
        entry["refresh"] = _stats(ref_ms)
        entry["refresh_over_iteration"] = round(float(np.median(ref_ms))
                                                / float(np.median(it_ms)), 3)
        if n != n_big:
            del core
    doc["objective_after_add"] = core.objective(reg)["objective"]
    core.refit(2, objective_every=1)
    doc["warm_history"] = [v for _, v in core.objective_history]
    cat = [torch.cat([a, b]) for a, b in zip((u, i, r), batches[n_big])]
    del core
    cold = E.ALSCore(*cat, device=dev)
    cold.fit(args.rank, args.fit_iters, reg, seed=1, objective_every=1)
    doc["cold_history"] = [v for _, v in cold.objective_history]
    doc["cold_iterations_to_reach_warm_1"] = next(
        (k + 1 for k, v in enumerate(doc["cold_history"]) if v <= doc["warm_history"][0]), None)
    print(json.dumps(doc), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
