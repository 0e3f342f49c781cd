"""Cost of the list measures (K15) beside the lists they measure.

Two cases:
  * "ml25m": the ML-25M shape (162,541 users x 59,047 items, rank 64, random factors with a
    shared direction), the lists K5 makes at top 10;
  * "zipf": a synthetic catalogue of 1M rows and as many 100-slot lists as fit (at most
    --zipf-lists), ids drawn from datasets._zipf_probs and scattered over the rows.
For each: device-event times, after a warm-up of every call, of als_list_exposure,
als_list_concentration, als_list_novelty, torch.bincount over the same flattened valid entries
(the baseline the counting kernel has to beat; once over entries already filtered and cast to
int64, once with the filter and the cast a caller would have to run first) and, for ml25m, the
K5 call that makes the lists (what a user already pays).  A timed window is `inner`
back-to-back calls (so that short kernels are not a measurement of the clock), the calls
alternate inside every repeat, and the counts are checked against torch.bincount.  Each timed
exposure call goes through engine.list_exposure_rows, so it includes the allocation of the
counts and of the skipped word (torch.empty + torch.zeros) beside the memset and the kernel.
Writes one JSON document (profiles/k15_list_metrics_cost.json is a run of this, with the
figures of the two counting forms that were measured during development and not kept recorded
beside it).

    python tools/list_metrics_cost.py --out profiles/k15_list_metrics_cost.json
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


def measure(name, idx, at, n_v, pop, n_pop, repeats, inner, extra=None):
    ws = E.Workspace(idx.device)
    flat = idx[:, :at].reshape(-1)
    flat = flat[(flat >= 0) & (flat < n_v)].long()
    want = torch.bincount(flat, minlength=n_v)
    counts, _ = E.list_exposure_rows(idx, at, n_v)
    tail = E.long_tail_bits(pop, n_v, 0.2)

    def bincount_from_lists():
        e = idx[:, :at].reshape(-1)
        return torch.bincount(e[(e >= 0) & (e < n_v)].long(), minlength=n_v)

    calls = {
        "exposure": lambda: E.list_exposure_rows(idx, at, n_v),
        "torch_bincount": lambda: torch.bincount(flat, minlength=n_v),
        "torch_bincount_with_filter_and_cast": bincount_from_lists,
        "concentration": lambda: E.list_concentration(counts, n_v, None, idx.shape[0], at, ws),
        "novelty": lambda: E.list_novelty_rows(idx, at, n_v, pop, n_pop, ws, None, tail),
    }
    calls.update(extra or {})
    for key, fn in calls.items():              # warm-up of each, and the counts checked
        out = fn()
        if key == "exposure":
            assert torch.equal(out[0].long(), want), key
    torch.cuda.synchronize()
    ts = {key: [] for key in calls}
    for _ in range(repeats):
        for key, fn in calls.items():
            ts[key].append(_time(fn, inner))
    conc = E.list_concentration(counts, n_v, None, idx.shape[0], at, ws).tolist()
    r = {"case": name, "lists": int(idx.shape[0]), "at": at, "catalogue_rows": n_v,
         "entries": int(flat.numel()), "repeats": repeats, "calls_per_window": inner,
         "exposure_window_rows": E.list_exposure_window(),
         **{key: _stats(t) for key, t in ts.items()},
         "coverage": round(conc[1] / conc[0], 5), "gini": round(conc[3], 5),
         "top_item_share_of_entries": round(conc[6] / max(conc[2], 1.0), 5)}
    med = lambda k: float(np.median(ts[k]))
    r["exposure_over_bincount"] = round(med("exposure") / med("torch_bincount"), 3)
    r["exposure_G_entries_per_s"] = round(flat.numel() / med("exposure") / 1e6, 2)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--shape", default="162541x59047x64")
    ap.add_argument("--zipf-rows", type=int, default=1_000_000)
    ap.add_argument("--zipf-lists", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("list_metrics_cost.py needs a HIP GPU: nothing is measured without one")
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    doc = {"tool": "tools/list_metrics_cost.py", "device": "MI355X (gfx950), one GPU",
           "method": "device events around `calls_per_window` back-to-back calls, per-call "
                     "time = window / calls; median / min / max of the repeats after a warm-up "
                     "of each call; the calls alternate inside a repeat; the counts equal "
                     "torch.bincount's; an exposure call includes the allocation of its two "
                     "outputs (engine.list_exposure_rows)",
           "results": []}

    def flush():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")

    # ---- the ML-25M shape, lists from K5
    n_u, n_i, rank = (int(x) for x in args.shape.split("x"))

    def factors(n):
        return (torch.randn((n, rank), device="cuda", generator=g)
                + 1.5 * torch.rand((n, 1), device="cuda", generator=g)) / rank ** 0.5

    core = E.ALSCore.from_factors(torch.arange(n_u), factors(n_u), torch.arange(n_i),
                                  factors(n_i))
    idx, _ = E.topk_rows(core.U, n_u, core.V, n_i, rank, 10)
    p = D._zipf_probs(n_i, 0.9, 1.0).to(dev)
    pop = (p * 25_000_000).round().to(torch.int32)[torch.randperm(n_i, device=dev, generator=g)]
    r = measure("ml25m", idx, 10, n_i, pop.contiguous(), n_u, args.repeats, 20,
                {"k5_top10": lambda: E.topk_rows(core.U, n_u, core.V, n_i, rank, 10)})
    doc["results"].append(r)
    print(json.dumps(r), flush=True)
    flush()
    del core, idx

    # ---- a Zipf-skewed catalogue of 1M rows, 100-slot lists
    n_v, at = args.zipf_rows, 100
    free, _ = torch.cuda.mem_get_info()
    # per entry: the int32 list, bincount's int64 copy and its filter temporaries
    n_q = int(min(args.zipf_lists, free // (at * 40)))
    cdf = torch.cumsum(D._zipf_probs(n_v, 0.9, 1.0), 0)
    cdf = (cdf / cdf[-1]).to(torch.float32).to(dev)
    perm = torch.randperm(n_v, device=dev, generator=g).to(torch.int32)
    idx = torch.empty((n_q, at), dtype=torch.int32, device=dev)
    step = 1 << 20
    for r0 in range(0, n_q, step):
        r1 = min(n_q, r0 + step)
        u = torch.rand(((r1 - r0) * at,), device=dev, generator=g)
        draw = torch.searchsorted(cdf, u).clamp_(max=n_v - 1)
        idx[r0:r1] = perm[draw].view(r1 - r0, at)
    pop = torch.bincount(idx.reshape(-1).long(), minlength=n_v).to(torch.int32)
    r = measure("zipf", idx, at, n_v, pop, n_q, args.repeats, 1)
    doc["results"].append(r)
    print(json.dumps(r), flush=True)
    flush()


if __name__ == "__main__":
    main()
