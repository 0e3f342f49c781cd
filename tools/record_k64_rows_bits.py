#!/usr/bin/env python3
"""Record the bits of the rank 33-64 explicit half-sweep (gram_solve_kernel<4, false>, the
launch-2 solve of its heavy rows) on a small case into tests/golden/k64_rows_bits.npz.

The kernel's sums are order-fixed by construction (one wavefront per task, MFMA steps in
rating order, chunk partials summed in slot order), so a change to how it holds its
accumulators, to its LDS or to its occupancy has to return the same bytes.  case() builds the
inputs from seeds alone; tests/test_gpu_k64_occupancy4.py imports this file, rebuilds them
and compares X of every (rank, reg, dual) run array for array.

case(): light rows of LIGHT_DEGREES ratings (the step and block edges of the Gram pipeline:
32-rating MFMA steps, 64-rating staging blocks), each twice with the same source ids and
ratings — once among the first rows and once after FILLERS filler rows, so the two copies
sit at different places of the task order with different co-resident neighbours — and one
heavy row of 2 * 4096 + 5 ratings (three chunk tasks at the production task length).

Re-record only when a change is MEANT to move bits, from a library built at the commit named:
    python tools/record_k64_rows_bits.py --commit $(git rev-parse HEAD)
"""
import argparse
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "k64_rows_bits.npz")

RANKS = (33, 48, 64)          # 33 and 48: padded dims, k % 16 != 0
GOLDEN_RANKS = (33, 64)
LIGHT_DEGREES = (1, 31, 32, 33, 63, 64, 65, 130)
CHUNK = 4096                  # engine.chunk_for(rank <= 64)
HEAVY_DEGREE = 2 * CHUNK + 5
N_SRC = HEAVY_DEGREE + 3
FILLERS = 200
FILLER_DEGREES = (130, 260)   # >= 2 * 64 + 2: full-rank Grams at every rank, also at reg = 0
# (reg, dual): reg = 0 switches the dual path off (engine.solve_half), so the short rows run
# the primal kernel; dual = False does the same at reg = 0.1
RUNS = ((0.0, True), (0.1, True), (0.1, False))


def run_id(rank, reg, dual):
    return f"k{rank}-reg{reg:g}-{'dual' if dual else 'primal'}"


def case(rank):
    """Host inputs of one rank, from seeds alone.  Rows: [light..., fillers..., heavy, the
    every-source row of helpers.degree_rows, light copies...]; copy_of[j] = (first, second)
    row of LIGHT_DEGREES[j]."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import degree_rows, unit_source_factors
    rng = np.random.default_rng(9000 + rank)
    fill = rng.integers(FILLER_DEGREES[0], FILLER_DEGREES[1] + 1, FILLERS).tolist()
    degrees = list(LIGHT_DEGREES) + fill + [HEAVY_DEGREE]
    dst, src, r = degree_rows(degrees, N_SRC, seed=9100 + rank)
    n0 = len(degrees) + 1
    cd, cs, cr = [dst], [src], [r]
    for j in range(len(LIGHT_DEGREES)):
        sel = dst == j
        cd.append(np.full(int(sel.sum()), n0 + j, np.int32))
        cs.append(src[sel])
        cr.append(r[sel])
    dst, src, r = np.concatenate(cd), np.concatenate(cs), np.concatenate(cr)
    return {"dst": dst, "src": src, "r": r, "n_rows": n0 + len(LIGHT_DEGREES),
            "heavy_row": len(degrees) - 1,
            "copy_of": [(j, n0 + j) for j in range(len(LIGHT_DEGREES))],
            "Y": unit_source_factors(N_SRC, rank, seed=9200 + rank)}


def digest(c):
    h = hashlib.sha256()
    for name in ("dst", "src", "r", "Y"):
        h.update(name.encode())
        h.update(np.ascontiguousarray(c[name]).tobytes())
    return h.hexdigest()


def solve(E, torch, c, rank, reg, dual, core=None):
    """One user half-sweep of the case through als_solve_half, the fp64 rescue held back until
    its list has been counted.  Returns (core, X [n_rows, ld] as numpy, rows the launches
    sent to the rescue)."""
    if core is None:
        core = E.ALSCore(c["dst"], c["src"], c["r"], device="cuda:0", chunk=CHUNK)
        core.init_factors(rank, seed=3)
        core.V[:, :rank] = torch.as_tensor(c["Y"]).to(core.V.device)
    core.U.fill_(7.0)
    core.status.zero_()
    args = (core.user_block, core.V, core.U, rank, reg, False, 1.0, None, core.status, core.ws)
    E.solve_half(*args, E.PHASE_ALL & ~E.PHASE_RESCUE, dual=dual)
    torch.cuda.synchronize()
    rescued = int(core.ws.buf[8:12].view(torch.int32).item())
    E.solve_half(*args, E.PHASE_RESCUE, dual=dual)
    torch.cuda.synchronize()
    return core, core.U.cpu().numpy(), rescued


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="commit the loaded library was built from")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import _pkgload
    _pkgload.load()
    from als_mi355x import engine as E
    if not torch.cuda.is_available():
        sys.exit("record_k64_rows_bits.py needs a HIP GPU")
    commit = a.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT,
                                                 text=True).strip()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    doc = {"meta/commit": np.array(commit),
           "meta/hipcc_version": np.array(subprocess.check_output([hipcc, "--version"], text=True)),
           "meta/device": np.array(torch.cuda.get_device_name(0))}
    for rank in GOLDEN_RANKS:
        c = case(rank)
        doc[f"k{rank}/inputs_sha256"] = np.array(digest(c))
        core = None
        for reg, dual in RUNS:
            core, X, rescued = solve(E, torch, c, rank, reg, dual, core)
            doc[f"{run_id(rank, reg, dual)}/X"] = X
            doc[f"{run_id(rank, reg, dual)}/status"] = core.status.cpu().numpy()
            print(f"{run_id(rank, reg, dual)}: status {int(core.status.item())}, "
                  f"{rescued} rows to the rescue")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **doc)
    print(f"{len(doc)} arrays, {os.path.getsize(a.out)} bytes -> {a.out} (commit {commit})")


if __name__ == "__main__":
    main()
