#!/usr/bin/env python3
"""Record the bits of the explicit rank 33-64 launch-1 solve on both sides of k == k_pad into
tests/golden/k64_full_bits.npz: rank 64 runs gram_solve_kernel<4, false>, compiled for the
full rank (no padded dims, the lean sweep), ranks 33-63 run gram_solve_kernel<-4, false>, which
masks its padded dims at run time (csrc/gram_solve.hip).  Both must return what the one kernel
before the split returned, bit for bit; tests/test_gpu_k64_full_rank.py imports this file,
rebuilds the inputs from the seeds and compares.

case(): solved rows whose lengths sit on the primal kernel's edges (EDGE_DEGREES: the 32-rating
MFMA step, the 64-rating staging block, one rating under the 4,096-rating task), each twice with
the same ratings at two places of the task order, FILLERS filler rows, and one heavy row of
4,097 ratings (two chunk tasks in the same launch; the every-source row of helpers.degree_rows
is a second one).  A row's source ids are distinct, so the 4,095-rating row sets the number of
source rows (N_SRC), not the ~300 a smaller longest row would need.  The dual path is off in
every run: every light row goes through the primal kernel.

Runs (run names -> what is recorded: X, the status word, the rows sent to the fp64 rescue):
  k{33,48,63,64}-reg0.1   the well-posed systems
  k64-ld68                rank 64 with ld = 68 on a 0xFF-filled X
  k64-reg0                rank 64, reg = 0: the 33- and 63-rating rows are singular -> rescue
  k64-tiny                rank 64, reg 0.1, the first 96-rating row's ratings x 2^-20: its
                          scaled ratings fall under the split window -> rescue

Re-record only when a change is MEANT to move bits, from a library built at the commit named:
    python tools/record_k64_full_bits.py --commit $(git rev-parse HEAD)
"""
import argparse
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "k64_full_bits.npz")

RANKS = (33, 48, 63, 64)
EDGE_DEGREES = (33, 63, 64, 65, 96, 97, 127, 128, 129, 4095)
CHUNK = 4096                  # engine.chunk_for(rank <= 64)
HEAVY_DEGREE = CHUNK + 1
N_SRC = CHUNK + 4
FILLERS = 178                 # 2 x 10 edge rows + fillers + 2 heavy rows = 200 solved rows
FILLER_DEGREES = (130, 260)
REG = 0.1
TINY_DEGREE = 96
TINY_SCALE = 2.0 ** -20
RUNS = tuple(f"k{k}-reg0.1" for k in RANKS) + ("k64-ld68", "k64-reg0", "k64-tiny")


def _rows_recorder():
    spec = importlib.util.spec_from_file_location(
        "record_k64_rows_bits", os.path.join(ROOT, "tools", "record_k64_rows_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ROWS = _rows_recorder()
digest = ROWS.digest


def case(rank, tiny=False):
    """Host inputs of one rank, from seeds alone.  Rows: [edge..., fillers..., heavy, the
    every-source row, edge copies...]; copy_of[j] = (first, second) row of EDGE_DEGREES[j].
    tiny: both copies of the TINY_DEGREE row have their ratings scaled by TINY_SCALE."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import degree_rows, unit_source_factors
    rng = np.random.default_rng(9300)
    fill = rng.integers(FILLER_DEGREES[0], FILLER_DEGREES[1] + 1, FILLERS).tolist()
    degrees = list(EDGE_DEGREES) + fill + [HEAVY_DEGREE]
    dst, src, r = degree_rows(degrees, N_SRC, seed=9400)
    if tiny:
        r = np.where(dst == EDGE_DEGREES.index(TINY_DEGREE), r * np.float32(TINY_SCALE), r)
    n0 = len(degrees) + 1
    cd, cs, cr = [dst], [src], [r]
    for j in range(len(EDGE_DEGREES)):
        sel = dst == j
        cd.append(np.full(int(sel.sum()), n0 + j, np.int32))
        cs.append(src[sel])
        cr.append(r[sel])
    dst, src, r = np.concatenate(cd), np.concatenate(cs), np.concatenate(cr)
    return {"dst": dst, "src": src, "r": r.astype(np.float32), "n_rows": n0 + len(EDGE_DEGREES),
            "heavy_row": len(degrees) - 1,
            "copy_of": [(j, n0 + j) for j in range(len(EDGE_DEGREES))],
            "Y": unit_source_factors(N_SRC, rank, seed=9500 + rank)}


def run_case(name):
    """(rank, case) of a run name."""
    rank = int(name[1:3])
    return rank, case(rank, tiny=name.endswith("tiny"))


def solve(E, torch, name, c):
    """One user half-sweep of run `name` with the dual path off, the fp64 rescue held back
    until its list has been counted: (X as numpy, status word, rows sent to the rescue)."""
    rank = int(name[1:3])
    reg = 0.0 if name.endswith("reg0") else REG
    core = E.ALSCore(c["dst"], c["src"], c["r"], device="cuda:0", chunk=CHUNK)
    core.init_factors(rank, seed=3)
    core.V[:, :rank] = torch.as_tensor(c["Y"]).to(core.V.device)
    Y, X = core.V, core.U
    if name.endswith("ld68"):
        Y = torch.zeros((core.V.shape[0], 68), dtype=torch.float32, device=core.V.device)
        Y[:, :rank] = core.V[:, :rank]
        X = torch.empty((core.U.shape[0], 68), dtype=torch.float32, device=core.U.device)
        X.view(torch.uint8).fill_(0xFF)
    else:
        X.fill_(7.0)
    core.status.zero_()
    args = (core.user_block, Y, X, rank, reg, False, 1.0, None, core.status, core.ws)
    E.solve_half(*args, E.PHASE_ALL & ~E.PHASE_RESCUE, dual=False)
    torch.cuda.synchronize()
    rescued = int(core.ws.buf[8:12].view(torch.int32).item())
    E.solve_half(*args, E.PHASE_RESCUE, dual=False)
    torch.cuda.synchronize()
    return X.cpu().numpy(), int(core.status.item()), rescued


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
        sys.exit("record_k64_full_bits.py needs a HIP GPU")
    commit = a.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT,
                                                 text=True).strip()
    doc = {"meta/commit": np.array(commit), "meta/device": np.array(torch.cuda.get_device_name(0))}
    for name in RUNS:
        rank, c = run_case(name)
        X, status, rescued = solve(E, torch, name, c)
        doc[f"{name}/inputs_sha256"] = np.array(digest(c))
        # the 4,095- and 4,097-rating rows aside, X is small; float32 bits, compressed
        doc[f"{name}/X"] = X
        doc[f"{name}/status"] = np.array([status], np.int32)
        doc[f"{name}/rescued"] = np.array([rescued], np.int32)
        print(f"{name}: status {status}, {rescued} rows to the rescue")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **doc)
    print(f"{len(doc)} arrays, {os.path.getsize(a.out)} bytes -> {a.out} (commit {commit})")


if __name__ == "__main__":
    main()
