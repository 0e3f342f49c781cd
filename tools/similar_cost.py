"""Cost of a neighbour search by its two routes.

For each table shape and each (queries, top): one engine.similar_rows call (K12: the raw
table swept once per 16 queries) and one engine.similar_rows_unit call (unit copy + K5: what
the kernels before K12 can do) are timed with device events, alternating in one loop after a
warm-up of both; median / min / max of the repeats.  K12's achieved bytes/s counts the table
once per pass.  Writes one JSON document (profiles/k12_similar_cost.json is a run of this).

    python tools/similar_cost.py --out profiles/k12_similar_cost.json
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
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(min(ts)), 4),
            "max_ms": round(float(max(ts)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", default="59047x64,1000000x128")
    ap.add_argument("--queries", default="1,16,64,256,1024,4096")
    ap.add_argument("--tops", default="10,100")
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("similar_cost.py needs a HIP GPU: nothing is measured without one")
    doc = {"tool": "tools/similar_cost.py", "device": "MI355X (gfx950), one GPU",
           "method": "device events around each engine call (similar_rows = K12, "
                     "similar_rows_unit = unit copy + K5), the two alternating in one loop; "
                     "median / min / max of the repeats after a warm-up of both",
           "results": []}

    def flush():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")

    for shape in args.shapes.split(","):
        n, rank = (int(x) for x in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(1)
        T = torch.zeros((n, E.ld_for(rank)), device="cuda")
        T[:, :rank] = torch.randn((n, rank), device="cuda", generator=g)
        table_bytes = n * E.ld_for(rank) * 4
        for top in (int(x) for x in args.tops.split(",")):
            for n_q in (int(x) for x in args.queries.split(",")):
                rows = torch.randperm(n, device="cuda", generator=g)[:n_q].sort().values
                self_rows = rows.to(torch.int32).contiguous()

                def k12():
                    Q = T.index_select(0, rows).contiguous()
                    return E.similar_rows(Q, n_q, T, n, rank, top, self_rows, None)

                def k5():
                    return E.similar_rows_unit(rows, T, n, rank, top, None)

                (i1, s1), (i2, s2) = k12(), k5()      # warm-up of both, and agreement
                torch.cuda.synchronize()
                agree = float((i1 == i2).float().mean())
                dsc = float((s1 - s2).abs().max())
                reps = args.repeats if n_q < 1024 else 3
                t12, t5 = [], []
                for _ in range(reps):
                    t12.append(_time(k12))
                    t5.append(_time(k5))
                passes = (n_q + 15) // 16
                r = {"rows": n, "rank": rank, "queries": n_q, "top": top, "repeats": reps,
                     "k12": _stats(t12), "unit_copy_k5": _stats(t5),
                     "k12_over_k5": round(float(np.median(t12) / np.median(t5)), 3),
                     "k12_passes": passes,
                     "k12_table_GB_per_s": round(passes * table_bytes / np.median(t12) / 1e6, 1),
                     "index_agreement": round(agree, 6), "max_abs_score_diff": dsc}
                doc["results"].append(r)
                print(json.dumps(r), flush=True)
                flush()
    flush()


if __name__ == "__main__":
    main()
