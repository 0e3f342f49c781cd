"""Dev probe (NOT the bench): does the order in which launch 1's tasks reach the machine
matter?  light_rows[:n_light_primal] is an input array and may be in any order, so the
probe permutes it on the device into the order a plain weighted merge would visit the
light rows (list A = the longest ceil(f * n) rows, list B = the rest, A spread evenly
through all of B, both ending together: csrc/task_order.h without its tail; the chunks
and the dual tail stay where they are) and times PHASE_LAUNCH1 alone with
HIP events, the orders interleaved call by call.  Results must not depend on the order:
X after the launch is compared bit for bit.
    python tools/ab_order.py c1|c2 [--reps 9] [--f 0.0625,0.125,0.25,0.5]
    python tools/ab_order.py c1 --only cur|F [--side item|user]   (one order, for a
        rocprofv3 --kernel-trace or --pmc pass of its own)
    python tools/ab_order.py c1 --segments 8     (the current order cut into consecutive
        launches: where in the launch the time, the gathers and the VALU work sit)
Library under test: ALS_HIP_DEV=1 ALS_HIP_LIB=... or the product one.  With a library whose
kernel already merges (task_order.h), "cur" is that merge and the permuted orders stack on it.
Prints one JSON line per side: per order the median, min and max of the launch in ms."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import _pkgload  # noqa: E402

_pkgload.load()
from als_mi355x import datasets as D, engine as E  # noqa: E402
from als_mi355x import _lib as _L  # noqa: E402


def merged_light_order(n_chunks: int, n_light: int, f: float) -> np.ndarray:
    """Positions of the light list in the order the weighted merge of task_order.h visits
    them (the chunks, which the probe cannot move, left out)."""
    n_a_light = min(n_light, int(np.ceil(f * n_light)))
    a, n = n_chunks + n_a_light, n_chunks + n_light
    t = np.arange(n, dtype=np.int64)
    ia = (t * a) // n
    take_a = ((t + 1) * a) // n > ia
    idx = np.where(take_a, ia - n_chunks, n_a_light + (t - ia))  # light position, < 0: a chunk
    idx = idx[idx >= 0]
    assert idx.size == n_light and np.array_equal(np.sort(idx), np.arange(n_light))
    return idx


def launch1_slice(core, block, Y, X, k, reg, lo, hi, chunks):
    """PHASE_LAUNCH1 over light_rows[lo:hi] (and the block's chunks or none): the launch
    cut into consecutive pieces of its own order (explicit; the workspace and the prep
    are those of the whole block)."""
    L = _L.lib()
    ptr = _L.ptr
    w = core.ws.get(L.als_solve_workspace_bytes(k, block.n_chunks, Y.shape[0],
                                                block.n_light + block.n_heavy), keep_scale=True)
    _L.check(L.als_solve_half(ptr(block.row_ptr), ptr(block.col), ptr(block.val),
                              ptr(block.light_rows[lo:hi]), hi - lo, hi - lo,
                              ptr(block.heavy_rows), ptr(block.heavy_slot_begin), block.n_heavy,
                              ptr(block.chunk_row), ptr(block.chunk_begin), ptr(block.chunk_end),
                              block.n_chunks if chunks else 0, 0, 0, ptr(Y), Y.shape[0], ptr(X),
                              X.shape[1], k, float(reg), 0, 1.0, None, ptr(core.status), ptr(w),
                              w.numel(), int(E.PHASE_LAUNCH1), _L.stream_ptr(X.device)),
             "als_solve_half")


def segments(core, name, block, Y, X, k, reg, n, nseg, reps):
    """The current order in pieces: the chunks alone, then nseg equal slices of the primal
    light list (longest first).  Per piece: tasks, ratings, median ms, and the algorithmic
    gather rate (ratings x 4 k bytes of split words) — under rocprofv3 --pmc each piece is
    one dispatch, so VALU busy and FETCH_SIZE can be read per piece."""
    lr = block.light_rows[:n].long()
    deg = (block.row_ptr[lr + 1] - block.row_ptr[lr]).cpu().numpy()
    cnnz = int((block.chunk_end[:block.n_chunks] - block.chunk_begin[:block.n_chunks]).sum()) \
        if block.n_chunks else 0
    cuts = [round(n * s / nseg) for s in range(nseg + 1)]
    pieces = [("chunks", 0, 0, True, block.n_chunks, cnnz)] if block.n_chunks else []
    pieces += [(f"light{s}", cuts[s], cuts[s + 1], False, cuts[s + 1] - cuts[s],
                int(deg[cuts[s]:cuts[s + 1]].sum())) for s in range(nseg)]
    pieces.append(("whole", 0, n, True, block.n_chunks + n, cnnz + int(deg.sum())))
    times = {p[0]: [] for p in pieces}
    for rep in range(reps + 1):
        for tag, lo, hi, ch, _, _ in pieces:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch1_slice(core, block, Y, X, k, reg, lo, hi, ch)
            b.record()
            torch.cuda.synchronize()
            if rep:
                times[tag].append(a.elapsed_time(b))
    core.check_status()
    rows = []
    for tag, lo, hi, ch, tasks, nnz in pieces:
        ms = statistics.median(times[tag])
        rows.append({"piece": tag, "tasks": tasks, "ratings": nnz,
                     "max_len": int(deg[lo]) if hi > lo and not ch else None,
                     "min_len": int(deg[hi - 1]) if hi > lo else None,
                     "ms": round(ms, 4), "gather_TBps": round(nnz * 4 * k / ms / 1e9, 2)})
    print(json.dumps({"side": name, "lib": _L.LIB_PATH, "segments": rows,
                      "sum_of_pieces_ms": round(sum(r["ms"] for r in rows[:-1]), 4)}), flush=True)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    wl = sys.argv[1]
    reps = int(arg("--reps", "9"))
    fs = [float(x) for x in arg("--f", "0.0625,0.125,0.25,0.5").split(",")]
    only = arg("--only", None)
    side_only = arg("--side", None)
    nseg = int(arg("--segments", "0"))
    dev = torch.device("cuda", 0)
    u, i, r = D.synthetic_config("ml25m", device=dev)
    k, imp, alpha = (64, False, 1.0) if wl == "c1" else (128, True, 40.0)
    core = E.ALSCore(u, i, r, device=dev)
    del u, i, r
    torch.cuda.empty_cache()
    core.init_factors(k, seed=5)
    reg = 0.1
    for _ in range(3):
        core.iterate(reg) if not imp else core.fit(k, 1, reg, implicit=True, alpha=alpha)
    torch.cuda.synchronize()
    for name, block, Y, X, n_src in (("item", core.item_block, core.U, core.V, core.n_users),
                                     ("user", core.user_block, core.V, core.U, core.n_items)):
        if side_only and side_only != name:
            continue
        n = block.n_light - (block.n_dual(k) if not imp else 0)
        orig = block.light_rows[:n].clone()
        orders = {"cur": orig}
        for f in fs:
            perm = torch.as_tensor(merged_light_order(block.n_chunks, n, f), device=dev)
            orders[f"{f:g}"] = orig[perm]
        if only:
            orders = {only: orders[only]}
        yty = E.compute_yty(Y, n_src, k, core.ws_yty) if imp else None
        E.solve_half(block, Y, X, k, reg, imp, alpha, yty, core.status, core.ws,
                     E.PHASE_PREP | E.PHASE_RSCALE)
        if nseg:
            assert not imp, "--segments: explicit only"
            segments(core, name, block, Y, X, k, reg, n, nseg, reps)
            continue
        times = {o: [] for o in orders}
        ref = None
        same = True
        for rep in range(reps + 1):  # the first round warms up
            for o, rows in orders.items():
                block.light_rows[:n].copy_(rows)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                E.solve_half(block, Y, X, k, reg, imp, alpha, yty, core.status, core.ws,
                             E.PHASE_LAUNCH1)
                b.record()
                torch.cuda.synchronize()
                if rep:
                    times[o].append(a.elapsed_time(b))
                elif ref is None:
                    ref = X.clone()
                else:
                    same = same and torch.equal(ref, X)
        block.light_rows[:n].copy_(orig)
        core.check_status()
        out = {"wl": wl, "lib": _L.LIB_PATH, "side": name, "n_chunks": block.n_chunks,
               "n_light_primal": n, "reps": reps, "bitwise_equal": same,
               "l1_ms": {o: {"median": round(statistics.median(t), 4), "min": round(min(t), 4),
                             "max": round(max(t), 4)} for o, t in times.items()}}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
