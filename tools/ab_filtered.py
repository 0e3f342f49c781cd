"""Dev measurement (NOT the bench) of the filtered top-k, ML-25M-shaped fit (configs[1]):
the unfiltered als_topk of another build of the library against this tree's (raw ctypes,
interleaved, outputs compared bit for bit), then exclude="train" / candidates against the
unfiltered call in the same process, and the one-time build of the exclusion list.
    python tools/ab_filtered.py OTHER_LIBALS_HIP.so OUT.json
(the record in profiles/r07/ab_filtered.json was taken with the parent commit's library)"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import _pkgload  # noqa: E402

_pkgload.load()
from als_mi355x import datasets as D, engine as E  # noqa: E402
from als_mi355x import _lib as L  # noqa: E402

REPS = 7
dev = torch.device("cuda", 0)
out = {"reps": REPS}


def raw(path):
    lib = ctypes.CDLL(path)
    res, args = L.SIGNATURES["als_topk"]
    lib.als_topk.restype, lib.als_topk.argtypes = res, args
    res, args = L.SIGNATURES["als_topk_workspace_bytes"]
    lib.als_topk_workspace_bytes.restype, lib.als_topk_workspace_bytes.argtypes = res, args
    return lib


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def ab(tag, Q, n_q, V, n_v, k, top, libs):
    idx = torch.empty((n_q, top), dtype=torch.int32, device=dev)
    sc = torch.empty((n_q, top), dtype=torch.float32, device=dev)
    ws = {n: torch.empty(int(l.als_topk_workspace_bytes(n_q, n_v, k, top)), dtype=torch.uint8,
                         device=dev) for n, l in libs.items()}
    ts = {n: [] for n in libs}

    def call(n):
        rc = libs[n].als_topk(Q.data_ptr(), n_q, V.data_ptr(), n_v, Q.shape[1], k, top,
                              idx.data_ptr(), sc.data_ptr(), ws[n].data_ptr(), ws[n].numel(), 0)
        assert rc == 0, rc
    res = {}
    for n in libs:  # warm-up, and the outputs compared bit for bit
        timed(lambda: call(n))
        res[n] = (idx.clone(), sc.clone())
    names = list(libs)
    if len(names) == 2:
        out[f"{tag}_same_output"] = bool(torch.equal(res[names[0]][0], res[names[1]][0]) and
                                         torch.equal(res[names[0]][1].view(torch.int32),
                                                     res[names[1]][1].view(torch.int32)))
    for _ in range(REPS):
        for n in names:  # interleaved
            ts[n].append(round(timed(lambda: call(n)), 4))
    for n in names:
        out[f"{tag}_{n}_ms"] = ts[n]
        out[f"{tag}_{n}_median_ms"] = statistics.median(ts[n])
    print(tag, {n: statistics.median(ts[n]) for n in names}, flush=True)


libs = {"parent": raw(sys.argv[1]),
        "new": raw(L.PRODUCT_LIB)}

# ---- configs[1]: ML-25M shape, rank 64, fitted factors
u, i, r = D.synthetic_config("ml25m", device=dev)
core = E.ALSCore(u, i, r, device=dev)
core.fit(64, 3, 0.1, seed=5)
torch.cuda.synchronize()
out["configs1"] = {"n_users": core.n_users, "n_items": core.n_items, "nnz": core.nnz}
ab("c1_top10", core.U, core.n_users, core.V, core.n_items, 64, 10, libs)
ab("c1_top100", core.U, core.n_users, core.V, core.n_items, 64, 100, libs)

# ---- filtered path on the same factors, same process
t0 = time.perf_counter()
core.train_exclusion(True)
torch.cuda.synchronize()
out["train_exclusion_build_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
core._train_ex.clear()
t0 = time.perf_counter()
rp, col = core.train_exclusion(True)
torch.cuda.synchronize()
out["train_exclusion_build_ms_second"] = round((time.perf_counter() - t0) * 1e3, 3)
beg, end = rp[:-1].contiguous(), rp[1:].contiguous()
for top in (10, 100):
    f, p = [], []
    E.topk_rows_filtered(core.U, core.n_users, core.V, core.n_items, 64, top, beg, end, col, None)
    for _ in range(REPS):
        p.append(round(timed(lambda: E.topk_rows(core.U, core.n_users, core.V, core.n_items, 64,
                                                 top)), 4))
        f.append(round(timed(lambda: E.topk_rows_filtered(core.U, core.n_users, core.V,
                                                          core.n_items, 64, top, beg, end, col,
                                                          None)), 4))
    out[f"c1_top{top}_unfiltered_ms"] = p
    out[f"c1_top{top}_exclude_train_ms"] = f
    out[f"c1_top{top}_unfiltered_median_ms"] = statistics.median(p)
    out[f"c1_top{top}_exclude_train_median_ms"] = statistics.median(f)
    print("filtered", top, statistics.median(p), statistics.median(f), flush=True)
# candidates: popular items (> 75 ratings, R:245) with the training exclusion; and the worst
# case, a set smaller than `top` (no list ever fills: every block refined, every pair tested)
from als_mi355x import filters as F  # noqa: E402
deg = core.item_block.row_ptr[1:] - core.item_block.row_ptr[:-1]
pop = torch.nonzero(deg > 75).reshape(-1)
out["c1_popular_items"] = int(pop.numel())
bits_pop = F.pack_allow_bits(pop, core.n_items)
bits_5 = F.pack_allow_bits(pop[:5], core.n_items)
t = [round(timed(lambda: E.topk_rows_filtered(core.U, core.n_users, core.V, core.n_items, 64, 10,
                                              beg, end, col, bits_pop)), 4) for _ in range(REPS)]
out["c1_top10_exclude_train_popular_ms"] = t
out["c1_top10_exclude_train_popular_median_ms"] = statistics.median(t)
nq_w = 16384
t = [round(timed(lambda: E.topk_rows_filtered(core.U, nq_w, core.V, core.n_items, 64, 10,
                                              beg[:nq_w], end[:nq_w], col, bits_5)), 4)
     for _ in range(3)]
out["c1_top10_worstcase_5_candidates_16384_users_ms"] = t
t = [round(timed(lambda: E.topk_rows(core.U, nq_w, core.V, core.n_items, 64, 10)), 4)
     for _ in range(3)]
out["c1_top10_unfiltered_16384_users_ms"] = t
print("candidates", out["c1_top10_exclude_train_popular_median_ms"],
      out["c1_top10_worstcase_5_candidates_16384_users_ms"], flush=True)
# end to end through the engine (list cached): recommend_all with exclude="train"
t = [round(timed(lambda: core.recommend_all(10, True, exclude="train")), 4) for _ in range(3)]
out["c1_recommend_all_top10_exclude_train_ms"] = t
# how much of the lists the filter changes
a, _ = E.topk_rows(core.U, core.n_users, core.V, core.n_items, 64, 10)
b, _ = E.topk_rows_filtered(core.U, core.n_users, core.V, core.n_items, 64, 10, beg, end, col, None)
out["c1_top10_slots_changed_by_filter"] = float((a != b).float().mean())
del core, u, i, r, a, b
torch.cuda.empty_cache()

# ---- configs[4] shape (rank 128, 1M items, 262,144-user sample), synthetic factors with a
# long-tailed norm spread; parent vs new only
g = torch.Generator(device=dev)
g.manual_seed(1)
n_q, n_v, k = 262_144, 1_000_000, 128
Q = torch.randn((n_q, k), generator=g, device=dev) * 0.3
V = torch.randn((n_v, k), generator=g, device=dev) * 0.3
V *= torch.exp(0.35 * torch.randn((n_v, 1), generator=g, device=dev))
out["configs4_shape"] = {"n_q": n_q, "n_v": n_v, "rank": k, "factors": "synthetic"}
ab("c4_top10", Q, n_q, V, n_v, k, 10, libs)
ab("c4_top100", Q, n_q, V, n_v, k, 100, libs)

with open(sys.argv[2], "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps({k_: v for k_, v in out.items() if "median" in k_ or "build" in k_ or "same" in k_
                  or "changed" in k_}))
