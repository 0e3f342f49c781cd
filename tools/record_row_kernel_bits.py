#!/usr/bin/env python3
"""Record the bits of the three row-system kernels — K7 (als_fold_in), K11 (als_explain) and
K13 (als_nnls_rows) — into tests/golden/row_kernel_bits.npz.

Every output of the three entry points is order-fixed by construction, so a change to the
code they share (csrc/row_system.h) has to return the same bytes.  This tool runs a small
grid of cases through engine.fold_in_rows / explain_rows / nnls_rows and stores the outputs
only: tests/test_gpu_row_kernel_bits.py rebuilds the inputs from the seeds below (cases(),
inputs()) and compares array for array.  The file also holds a digest of each case's inputs,
the commit and the compiler the library was built with.

cases(), inputs() and run_case() are the test's code too (it imports this file): changing the
seeds, the inputs or which outputs are collected means recording again.

Re-record only when a change is MEANT to move bits, from a library built at the commit named:
    python tools/record_row_kernel_bits.py --commit $(git rev-parse HEAD)
                                           [--out tests/golden/row_kernel_bits.npz]
"""
import argparse
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "row_kernel_bits.npz")

N_SRC = 200
REG = 0.1
ALPHA = 40.0
TOP_N = 3
RANKS = (1, 16, 17, 33, 100, 128)  # all four NB; k_pad exact (16, 128) and ragged
NNLS_CHUNK = 32                    # the 33- and 65-rating rows go through the partial kernel
TARGETS = (1, 0, 16, 17, 1, 17, 16, 1, 17, 16)  # per row: none, one batch, two batches
PIVOT_RANK = 17


def cases():
    """(case id, k, implicit).  Every case but the failing pivot runs twice, with the sources
    stored tight (zeros in the padding) and wide (ld = k + 4 rounded up to a multiple of 4, NaN
    in the padding): no output may depend on the padding, so the file holds one set of arrays
    per case and both storages have to return it."""
    out = [(f"k{k}-{'implicit' if imp else 'explicit'}", k, imp)
           for k in RANKS for imp in (False, True)]
    return out + [("pivot", PIVOT_RANK, False)]


def storages(cid):
    return (False,) if cid == "pivot" else (False, True)


def _csr(rows):
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(c) for c, _ in rows], out=ptr[1:])
    col = np.concatenate([np.asarray(c, np.int64) for c, _ in rows]).astype(np.int32)
    val = np.concatenate([np.asarray(v, np.float64) for _, v in rows]).astype(np.float32)
    return ptr, col, val


def inputs(cid, k, implicit, wide):
    """The case's host inputs, from seeds alone: Y [N_SRC, ld], ptr, col, val, tgt_ptr, tgt, reg."""
    rng = np.random.default_rng(7000 + 13 * k + int(implicit))
    ld = (k + 4 + 3) // 4 * 4 if wide else (k + 3) // 4 * 4
    Y = np.full((N_SRC, ld), np.nan if wide else 0.0, np.float32)
    Y[:, :k] = (rng.standard_normal((N_SRC, k)) / np.sqrt(k)).astype(np.float32)
    if cid == "pivot":
        # reg = 0: the row of one repeated item has a rank-1 Gram, pivot 1 fails the test
        rows = [(rng.integers(0, N_SRC, 65), rng.integers(1, 6, 65)),
                (np.full(5, 17), rng.integers(1, 6, 5))]
        counts, reg = (2, 2), 0.0
    else:
        # the batch-of-32 edges, one repeated item, unknown items, r = 0 and r < 0
        rows = [(rng.integers(0, N_SRC, n), rng.integers(1, 6, n))
                for n in (0, 1, 31, 32, 33, 65, k + 1)]
        rows.append((np.full(40, 17), rng.integers(1, 6, 40)))
        mixed = rng.integers(0, N_SRC, 30)
        mixed[::3] = -1
        mixed[1::3] = N_SRC
        rows.append((mixed, rng.integers(1, 6, 30)))
        rows.append((rng.integers(0, N_SRC, 20), rng.integers(-2, 4, 20)))
        rows[-1][1][:3] = (0, -1, 2)
        counts, reg = TARGETS, REG
    ptr, col, val = _csr(rows)
    tgt_ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(counts, out=tgt_ptr[1:])
    tgt = rng.integers(0, N_SRC, int(tgt_ptr[-1])).astype(np.int32)
    for r, c in enumerate(counts):
        if c == 17:
            tgt[tgt_ptr[r] + 5] = -1  # an unknown target
    return {"Y": Y, "ptr": ptr, "col": col, "val": val, "tgt_ptr": tgt_ptr, "tgt": tgt,
            "reg": np.float64(reg)}


def digest(inp):
    h = hashlib.sha256()
    for name in sorted(inp):
        h.update(name.encode())
        h.update(np.ascontiguousarray(inp[name]).tobytes())
    return h.hexdigest()


def run_case(E, torch, cid, k, implicit, wide):
    """(digest of the case's inputs, every output array by name)."""
    inp = inputs(cid, k, implicit, wide)
    dev = torch.device("cuda")
    t = lambda a: torch.as_tensor(a).to(dev).contiguous()
    Y, ptr, col, val = t(inp["Y"]), t(inp["ptr"]), t(inp["col"]), t(inp["val"])
    reg = float(inp["reg"])
    ws = E.Workspace(dev)
    yty = None
    if implicit:  # YtY never reads the padding, but give it the tight table all the same
        Yt = torch.zeros((N_SRC, E.ld_for(k)), dtype=torch.float32, device=dev)
        Yt[:, :k] = Y[:, :k]
        yty = E.compute_yty(Yt, N_SRC, k, ws)
    args = (ptr, col, val, Y, N_SRC, k, reg, implicit, ALPHA, yty)
    out = {}

    status = torch.zeros(1, dtype=torch.int32, device=dev)
    X, n_used = E.fold_in_rows(*args, status, ws)
    out.update({"k7_X": X, "k7_n_used": n_used, "k7_status": status})

    status = torch.zeros(1, dtype=torch.int32, device=dev)
    score, pos, contrib, n_used = E.explain_rows(*args, t(inp["tgt_ptr"]), t(inp["tgt"]), TOP_N,
                                                 status, ws)
    out.update({"k11_score": score, "k11_pos": pos, "k11_contrib": contrib,
                "k11_n_used": n_used, "k11_status": status})

    if cid != "pivot":
        for tag, chunk in (("k13", E.DEFAULT_CHUNK), ("k13c32", NNLS_CHUNK)):
            X, n_used, iters = E.nnls_rows(*args, ws, chunk, iters=True)
            out.update({f"{tag}_X": X, f"{tag}_n_used": n_used, f"{tag}_iters": iters})
    torch.cuda.synchronize()
    return digest(inp), {n: v.cpu().numpy() for n, v in out.items()}


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
        sys.exit("record_row_kernel_bits.py needs a HIP GPU")
    commit = a.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT,
                                                 text=True).strip()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    doc = {"meta/commit": np.array(commit),
           "meta/hipcc_version": np.array(subprocess.check_output([hipcc, "--version"], text=True)),
           "meta/device": np.array(torch.cuda.get_device_name(0))}
    for cid, k, implicit in cases():
        first = None
        for wide in storages(cid):
            sha, out = run_case(E, torch, cid, k, implicit, wide)
            doc[f"{cid}/inputs_sha256_{'wide' if wide else 'tight'}"] = np.array(sha)
            if first is None:
                first = out
                doc.update({f"{cid}/{name}": arr for name, arr in out.items()})
            for name, arr in out.items():  # NaN padding changes nothing
                assert arr.tobytes() == first[name].tobytes(), (cid, name, "tight != wide")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **doc)
    print(f"{len(doc)} arrays, {os.path.getsize(a.out)} bytes -> {a.out} (commit {commit})")


if __name__ == "__main__":
    main()
