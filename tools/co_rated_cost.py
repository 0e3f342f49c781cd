#!/usr/bin/env python3
"""Cost of the co-rated neighbours (K19) beside the routes they stand next to (DESIGN.md
section K19).

On the ML-25M-shaped synthetic ratings (datasets.synthetic_config("ml25m")), item side, top 10,
measure "count" (the measure changes one fp64 expression per candidate row, not the traffic),
device-event times after a warm-up of every call of
  * ALSCore.co_rated for 1, 16 and 256 queries drawn from the most-rated, the median and the
    least-rated items,
  * the same answer from torch.sparse on the same device: the queries' rows of B^T (a sparse
    COO slice, built outside the timed window) times B by torch.sparse.mm, densified, the
    query's own column cleared, then torch.topk; idx and counts are compared with K19's,
  * K12's ALSCore.similar (rank 64 factors) for the same queries,
  * ALSCore.co_rated_all(10): a uniform sample of `--sample` rows first; the whole catalogue
    is run when the sample predicts less than `--all-budget-s` seconds, otherwise the
    prediction is recorded and marked as extrapolated.  The torch route is treated alike,
    in chunks of 256 rows.
The figure is the median of the repeats with minimum and maximum beside it.  Clocks are taken
as found.  Writes one JSON document.

    python tools/co_rated_cost.py --out profiles/k19_co_rated_cost.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload  # noqa: E402

_pkgload.load()
from als_mi355x import datasets as D  # noqa: E402
from als_mi355x import engine as E  # noqa: E402

TOP = 10


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _stats(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(min(ts)), 4),
            "max_ms": round(float(max(ts)), 4), "repeats": len(ts)}


def _say(*a):
    print(*a, file=sys.stderr, flush=True)


def _finish(doc, out):
    print(json.dumps(doc), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--config", default="ml25m")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=1024)
    ap.add_argument("--all-budget-s", type=float, default=90.0)
    ap.add_argument("--only", default="", help="comma-separated query tags; skips the rest "
                                               "and the all-items part")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("co_rated_cost.py needs a HIP GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    u, i, r = D.synthetic_config(args.config, device=dev)
    core = E.ALSCore(u, i, r, device=dev)
    del u, i, r
    core.init_factors(64, seed=1)
    ib, ub = core.item_block, core.user_block
    n_i, n_u = core.n_items, core.n_users
    ids = core.iidx.ids()
    lens = (ib.row_ptr[1:] - ib.row_ptr[:-1])
    ulen = (ub.row_ptr[1:] - ub.row_ptr[:-1]).double()
    order = torch.argsort(lens, descending=True, stable=True)
    doc = {"tool": "tools/co_rated_cost.py", "device": "MI355X (gfx950), one GPU",
           "config": args.config, "nnz": core.nnz, "n_users": n_u, "n_items": n_i, "top": TOP,
           "measure": "count", "task_entries": E.co_rated_task(),
           "cache_window": E.co_rated_window(), "pass_queries": E.CO_RATED_PASS,
           "sum_user_len_squared": float((ulen * ulen).sum()),
           "item_ratings_max_median_min": [int(lens.max()), int(lens.median()), int(lens.min())],
           "method": "device events around one call, median / min / max of the repeats after a "
                     "warm-up of each call; clocks as found",
           "queries": {}}

    # B [users, items] and B^T [items, users] as sparse fp32 matrices of ones (duplicates add)
    ones = torch.ones(core.nnz, dtype=torch.float32, device=dev)
    # (through a coalesced COO: K1 keeps a row's columns in input order and keeps duplicates,
    # and rocSPARSE's SpGEMM wants the second factor's rows sorted)
    user_of = torch.repeat_interleave(torch.arange(n_u, device=dev),
                                      ub.row_ptr[1:] - ub.row_ptr[:-1])
    B = torch.sparse_coo_tensor(torch.stack([user_of, ub.col.long()]), ones,
                                size=(n_u, n_i)).coalesce().to_sparse_csr()
    del user_of
    item_of = torch.repeat_interleave(torch.arange(n_i, device=dev), lens)
    Bt = torch.sparse_coo_tensor(torch.stack([item_of, ib.col.long()]), ones,
                                 size=(n_i, n_u)).coalesce()

    def torch_route(rows):
        sel = Bt.index_select(0, rows).to_sparse_csr()

        def run():
            C = torch.sparse.mm(sel, B).to_dense()
            C[torch.arange(rows.numel(), device=dev), rows] = 0
            return torch.topk(C, TOP, dim=1)
        return run

    def exact_counts(a):
        """Row a of B^T B in int64 by index_add_ over the user-side entries."""
        mult = torch.zeros(n_u, dtype=torch.int64, device=dev).index_add_(
            0, ib.col[ib.row_ptr[a]:ib.row_ptr[a + 1]].long(),
            torch.ones(int(lens[a]), dtype=torch.int64, device=dev))
        w = torch.repeat_interleave(mult, ub.row_ptr[1:] - ub.row_ptr[:-1])
        c = torch.zeros(n_i, dtype=torch.int64, device=dev).index_add_(0, ub.col.long(), w)
        c[a] = 0
        return c

    def measure(tag, rows):
        if args.only and tag not in args.only.split(","):
            return
        _say("start", tag)
        q_ids = ids[rows]
        entry = {"query_ratings_max_min": [int(lens[rows].max()), int(lens[rows].min())],
                 "walked_entries": float(sum(
                     float(ulen[ib.col[ib.row_ptr[a]:ib.row_ptr[a + 1]].long()].sum())
                     for a in rows.tolist()))}
        ours = lambda: core.co_rated(q_ids, TOP, measure="count")
        sim = lambda: core.similar(q_ids, TOP)
        ours(), sim()
        torch.cuda.synchronize()
        if rows.numel() == 1:
            c = exact_counts(int(rows[0]))
            got = ours()[3][0].long()
            entry["counts_equal_index_add"] = bool(torch.equal(got, torch.topk(c, TOP).values))
        _say(tag, "co_rated and similar warm")
        entry["co_rated"] = _stats([_time(ours)[0] for _ in range(args.repeats)])
        entry["similar_k12_rank64"] = _stats([_time(sim)[0] for _ in range(args.repeats)])
        try:
            srows = torch.sort(rows).values         # co_rated answers in ascending id order
            tr = torch_route(srows)
            _say(tag, "torch rows selected")
            tr()
            torch.cuda.synchronize()
            _say(tag, "torch warm")
            ts, val = [], None
            for _ in range(max(2, args.repeats // 2)):
                t, val = _time(tr)
                ts.append(t)
            entry["torch_sparse_mm_topk"] = _stats(ts)
            _, _, _, common = ours()
            entry["counts_equal_torch"] = bool(torch.equal(common.long(), val.values.long()))
            entry["co_rated_over_torch"] = round(
                entry["co_rated"]["median_ms"] / entry["torch_sparse_mm_topk"]["median_ms"], 4)
        except Exception as ex:  # the torch route is a comparison: record why it has no figure
            entry["torch_sparse_mm_topk"] = {"error": f"{type(ex).__name__}: {str(ex)[:300]}"}
        doc["queries"][tag] = entry
        _say(tag, json.dumps(entry))

    mid = n_i // 2
    for m in (1, 16, 256):
        measure(f"most_rated_{m}", order[:m].contiguous())
        measure(f"median_{m}", order[mid - m // 2: mid - m // 2 + m].contiguous())
        measure(f"least_rated_{m}", order[n_i - m:].contiguous())

    if args.only:
        return _finish(doc, args.out)
    # every item: a uniform sample first, the catalogue when the sample says it fits
    g = torch.Generator(device="cpu").manual_seed(7)
    samp = torch.sort(torch.randperm(n_i, generator=g)[:args.sample]).values.to(dev)
    samp_ids = ids[samp]
    allq = {"sample_rows": int(samp.numel())}
    core.co_rated(samp_ids[:64], TOP, measure="count")
    t_s = [_time(lambda: core.co_rated(samp_ids, TOP, measure="count"))[0] for _ in range(3)]
    allq["co_rated_sample"] = _stats(t_s)
    pred_s = float(np.median(t_s)) * 1e-3 * n_i / samp.numel()
    allq["co_rated_all_predicted_s"] = round(pred_s, 3)
    _say("co_rated_all predicted s", pred_s)
    doc["all_items"] = allq
    if args.out:      # what is known so far, should a later step not finish
        _finish(doc, args.out + ".partial")
    if pred_s < args.all_budget_s:
        if pred_s < 10:
            core.co_rated_all(TOP, measure="count")      # (a warm-up, where it is cheap)
        t_a =[_time(lambda: core.co_rated_all(TOP, measure="count"))[0]
               for _ in range(3 if pred_s < 10 else 1)]
        allq["co_rated_all"] = _stats(t_a)
        allq["co_rated_all_extrapolated"] = False
    else:
        allq["co_rated_all_extrapolated"] = True
    try:
        chunks = [samp[c:c + 256] for c in range(0, samp.numel(), 256)]
        runs = [torch_route(c) for c in chunks]
        runs[0]()
        torch.cuda.synchronize()
        t_t = [sum(_time(rn)[0] for rn in runs) for _ in range(2)]
        allq["torch_sample_chunks_of_256"] = _stats(t_t)
        allq["torch_all_predicted_s"] = round(float(np.median(t_t)) * 1e-3 * n_i / samp.numel(),
                                              3)
    except Exception as ex:
        allq["torch_sample_chunks_of_256"] = {"error": f"{type(ex).__name__}: {str(ex)[:300]}"}
    t_k = [_time(lambda: core.similar_all(TOP))[0] for _ in range(3)]
    allq["similar_all_k12_rank64"] = _stats(t_k)
    doc["all_items"] = allq
    _finish(doc, args.out)


if __name__ == "__main__":
    main()
