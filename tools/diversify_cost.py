"""Cost of diversified lists beside the plain ones.

At one model shape (default: the ML-25M shape, 162,541 users x 59,047 items, rank 64, random
factors with a shared direction) and for each (top, pool): device-event medians, after a
warm-up of every call, of
  * recommend_all(top) alone (K5 at `top`),
  * K5 at `pool` alone (the candidate pools of every user),
  * K14 alone on those pools (engine.diversify_rows), with its gathered bytes per second
    (live slots x rank x 4 B; the pool arrays and outputs are not counted),
  * K5 at `pool` + K14 as ALSCore.recommend_diverse runs them (chunked),
and the mean intra-list similarity of the plain top lists (als_list_similarity) and of the
diversified ones at trade-off 0.7.  Writes one JSON document
(profiles/k14_diversify_cost.json is a run of this).

    python tools/diversify_cost.py --out profiles/k14_diversify_cost.json
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
from als_mi355x import engine as E  # noqa: E402


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ts):
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(min(ts)), 3),
            "max_ms": round(float(max(ts)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--shape", default="162541x59047x64")
    ap.add_argument("--cases", default="10:50,10:100,100:256", help="top:pool, comma separated")
    ap.add_argument("--trade-off", type=float, default=0.7)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diversify_cost.py needs a HIP GPU: nothing is measured without one")
    n_u, n_i, rank = (int(x) for x in args.shape.split("x"))
    lam = args.trade_off
    g = torch.Generator(device="cuda").manual_seed(1)

    def factors(n):
        return (torch.randn((n, rank), device="cuda", generator=g)
                + 1.5 * torch.rand((n, 1), device="cuda", generator=g)) / rank ** 0.5

    core = E.ALSCore.from_factors(torch.arange(n_u), factors(n_u), torch.arange(n_i),
                                  factors(n_i))
    doc = {"tool": "tools/diversify_cost.py", "device": "MI355X (gfx950), one GPU",
           "shape": {"users": n_u, "items": n_i, "rank": rank}, "trade_off": lam,
           "method": "device events around each engine call, every user in one call; median / "
                     "min / max of the repeats after a warm-up of each; random factors "
                     "N(0, 1) + a shared direction",
           "results": []}

    def flush():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")

    for case in args.cases.split(","):
        top, pool = (int(x) for x in case.split(":"))
        pi, ps = E.topk_rows(core.U, n_u, core.V, n_i, rank, pool)

        calls = {
            "recommend_all_top": lambda: core.recommend_all(top),
            "k5_pool": lambda: E.topk_rows(core.U, n_u, core.V, n_i, rank, pool),
            "k14": lambda: E.diversify_rows(pi, ps, core.V, n_i, rank, top, lam),
            "recommend_diverse": lambda: core.recommend_diverse(top, trade_off=lam, pool=pool),
        }
        for fn in calls.values():          # warm-up of each
            fn()
        torch.cuda.synchronize()
        ts = {name: [] for name in calls}
        for _ in range(args.repeats):
            for name, fn in calls.items():
                ts[name].append(_time(fn))
        _, _, ils_after = E.diversify_rows(pi, ps, core.V, n_i, rank, top, lam)
        ils_before = E.list_similarity_rows(pi[:, :top].contiguous(), core.V, n_i, rank)
        live = int(((pi >= 0) & ps.isfinite()).sum())
        k14_ms = float(np.median(ts["k14"]))
        r = {"top": top, "pool": pool, "repeats": args.repeats,
             **{name: _stats(t) for name, t in ts.items()},
             "k14_over_k5_pool": round(k14_ms / float(np.median(ts["k5_pool"])), 3),
             "k14_gathered_bytes": live * rank * 4,
             "k14_gathered_GB_per_s": round(live * rank * 4 / k14_ms / 1e6, 1),
             "mean_ils_plain_top": round(float(ils_before.nanmean()), 5),
             "mean_ils_diverse": round(float(ils_after.nanmean()), 5)}
        doc["results"].append(r)
        print(json.dumps(r), flush=True)
        flush()
        del pi, ps
    flush()


if __name__ == "__main__":
    main()
