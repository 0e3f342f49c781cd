#!/usr/bin/env python3
"""Cost of taking ratings out of a core (K18, ALSCore.remove_ratings) beside what it replaces
(DESIGN.md section K18).

On the ML-25M-shaped synthetic ratings (datasets.synthetic_config("ml25m")), for 12, 1e4 and
1e6 stored pairs drawn at random, for one user (the one with the most ratings) and for the
most-rated item, after a warm-up of every call:
  * the steps of remove_ratings on a core that is left as it is: K18's mark pass and compact
    pass on each side (device events: the kernels alone), shrinking both id maps and scheduling
    both sides again (host clock: they hold host syncs);
  * the whole remove_ratings call on a shallow copy of the core (host clock), which adds the
    de-duplication and the sort of the listed pairs, the two delete CSRs and the read-back of
    the kept row lengths;
  * against it the existing way: ALSCore(the filtered triples) from device tensors;
  * each pass against its byte floor — mark: 4 B read per stored entry, 1 bit written, the row
    pointers and the delete list; compact: 8 B read per stored entry and 8 B written per kept
    one — over the bandwidth of a 1 GiB device-to-device copy in this run.
Figures are the median of the repeats with minimum and maximum beside it.  Clocks are taken as
found.  Writes one JSON document.

    python tools/remove_cost.py --out profiles/k18_remove_cost.json
"""
import argparse
import copy
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


def make_pairs(core, what, gen):
    """(user ids, item ids) int32 on the device."""
    ub, ib = core.user_block, core.item_block
    uids, iids = core.uidx.ids(), core.iidx.ids()
    if what in ("one_user", "top_item"):
        block, mine, theirs = (ub, uids, iids) if what == "one_user" else (ib, iids, uids)
        row = int(torch.argmax(block.row_ptr[1:] - block.row_ptr[:-1]))
        cols = block.col[int(block.row_ptr[row]):int(block.row_ptr[row + 1])].long()
        a, b = mine[row].expand(cols.numel()).contiguous(), theirs[cols]
        return (a, b) if what == "one_user" else (b, a)
    pos = torch.randint(0, core.nnz, (int(what),), device=core.device, generator=gen)
    rows = torch.searchsorted(ub.row_ptr, pos, right=True) - 1
    return uids[rows], iids[ub.col[pos].long()]


def steps(core, pairs, repeats):
    """remove_ratings taken apart on a core that is left as it is."""
    ws = core.ws
    ub, ib = core.user_block, core.item_block
    u, i, ur, ir = core._listed_pairs(*pairs, "remove_cost")
    n_u, n_i = core.n_users, core.n_items
    ku, ki = torch.sort(ur * n_i + ir).values, torch.sort(ir * n_u + ur).values
    del_u = E._delete_csr(ku // n_i, ku % n_i, n_u)
    del_i = E._delete_csr(ki // n_u, ki % n_u, n_i)
    names = ("mark_user", "mark_item", "shrink_index", "compact_user", "compact_item",
             "reschedule", "steps_sum")
    ts = {k: [] for k in names}
    for rep in range(repeats + 1):
        t_mu, mu = _events(lambda: E.remove_mark(ub.row_ptr, ub.col, *del_u, ws, count_hits=True))
        t_mi, mi = _events(lambda: E.remove_mark(ib.row_ptr, ib.col, *del_i, ws))
        nnz = int(mu[1][-1])

        def shrink():
            out = []
            for idx, m in ((core.uidx, mu), (core.iidx, mi)):
                kept = m[2][1:] - m[2][:-1]
                out.append(E.shrink_index(idx, (kept == 0).nonzero().flatten(), ws) + (kept,))
            return out

        t_idx, ((uidx, umap, kept_u), (iidx, imap, kept_i)) = _host(shrink)
        t_cu, cu = _events(lambda: E.remove_compact(ub.col, ub.val, mu[0], mu[1], imap, n_i, nnz))
        t_ci, ci = _events(lambda: E.remove_compact(ib.col, ib.val, mi[0], mi[1], umap, n_u, nnz))

        def reschedule():
            for idx, m, kept, cv, b in ((uidx, mu, kept_u, cu, ub), (iidx, mi, kept_i, ci, ib)):
                stays = torch.ones(b.n_rows + 1, dtype=torch.bool, device=core.device)
                stays[:-1] = kept > 0
                E.schedule_block(idx.n, nnz, m[2][stays].contiguous(), *cv, ws, b.chunk)

        t_s, _ = _host(reschedule)
        if rep:   # the first pass warms everything up
            vals = (t_mu, t_mi, t_idx, t_cu, t_ci, t_s)
            for k, v in zip(names, vals + (sum(vals),)):
                ts[k].append(v)
        del cu, ci
    shape = dict(listed_pairs=int(u.numel()), removed=core.nnz - nnz,
                 left_users=n_u - uidx.n, left_items=n_i - iidx.n)
    return ts, shape, nnz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--config", default="ml25m")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", default="12,10000,1000000,one_user,top_item")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("remove_cost.py needs a HIP GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    u, i, r = D.synthetic_config(args.config, device=dev)
    core = E.ALSCore(u, i, r, device=dev)
    gen = torch.Generator(device="cuda").manual_seed(1)
    src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    cp = [_events(lambda: dst.copy_(src), 4)[0] for _ in range(args.repeats)]
    bw = 2 * src.numel() / (float(np.median(cp)) * 1e-3)
    del src, dst
    doc = {"tool": "tools/remove_cost.py", "device": "MI355X (gfx950), one GPU",
           "config": args.config, "nnz": core.nnz, "n_users": core.n_users,
           "n_items": core.n_items, "remove_tile": E.csr_remove_tile(), "repeats": args.repeats,
           "method": "device events around the K18 passes, host clock around steps that end in "
                     "a sync (they hold host syncs) and around the whole calls; median / min / "
                     "max of the repeats after one warm-up pass; clocks as found",
           "copy_bandwidth_TB_per_s": round(bw / 1e12, 3), "batches": {}}
    key_all = (u.long() << 32) | (i.long() & 0xFFFFFFFF)
    for what in args.batches.split(","):
        pairs = make_pairs(core, what, gen)
        ts, shape, nnz_out = steps(core, pairs, args.repeats)
        keep = ~torch.isin(key_all, (pairs[0].long() << 32) | (pairs[1].long() & 0xFFFFFFFF))
        rest = [x[keep].contiguous() for x in (u, i, r)]
        call, rebuild = [], []
        for rep in range(args.repeats + 1):
            twin = copy.copy(core)     # the blocks are replaced, never written: a shallow copy
            t_c, info = _host(lambda: twin.remove_ratings(*pairs))
            t_r, fresh = _host(lambda: E.ALSCore(*rest, device=dev))
            if rep:
                call.append(t_c)
                rebuild.append(t_r)
            assert twin.nnz == fresh.nnz == nnz_out and twin.n_users == fresh.n_users
            del twin, fresh
        entry = {k: _stats(v) for k, v in ts.items()}
        entry.update(shape)
        entry["remove_ratings_call"] = _stats(call)
        entry["rebuild_core_from_filtered"] = _stats(rebuild)
        entry["rebuild_over_remove_ratings"] = round(float(np.median(rebuild))
                                                     / float(np.median(call)), 2)
        for side, n in (("user", core.n_users), ("item", core.n_items)):
            floors = {"mark": 4 * core.nnz + core.nnz / 8 + 32 * (n + 1) + 4 * shape["listed_pairs"],
                      "compact": 8 * core.nnz + core.nnz / 8 + 8 * nnz_out}
            for step, nbytes in floors.items():
                e = entry[f"{step}_{side}"]
                e["byte_floor_ms"] = round(nbytes / bw * 1e3, 4)
                e["over_byte_floor"] = round(e["median_ms"] / e["byte_floor_ms"], 2)
        doc["batches"][what] = entry
        print(json.dumps({what: entry}), flush=True)
        del rest, keep
    print(json.dumps(doc), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
