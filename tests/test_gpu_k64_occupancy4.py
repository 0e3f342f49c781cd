"""The rank 33-64 explicit half-sweep at four waves per SIMD (gram_solve_kernel<4, false>:
one rhs accumulator tile, LDS trimmed to the W1<4> solve, csrc/gram_solve.hip) on the
smallest case at which the changed pieces can go wrong (tools/record_k64_rows_bits.py
case()): ranks 33, 48, 64; light rows of 1, 31, 32, 33, 63, 64, 65 and 130 ratings, each twice
with the same ratings at two places of the task order, among 200 filler rows; one heavy row
of 2 * 4096 + 5 ratings (three chunk tasks whose rhs goes through store_slot_f32 and is
solved by launch 2).  Three runs per rank: reg = 0 (the dual path is off, every light row
runs the primal kernel), reg = 0.1 (rows <= 32 ratings take the dual path, 33 and above the
primal kernel) and reg = 0.1 with the dual path switched off (every length through the primal
kernel on a well-posed system).

Checks.  (1) Per row against oracle.c_oracle.half_sweep with the bar of
test_gpu_edges_k2_k3.py for this kernel: ||x - ref|| / ||ref|| <= 1e-4 and max error <= 8 x
the max error of the fp32 textbook solve of the same rows, no row in the fp64 rescue list.
At reg = 0 a row of n < rank ratings has a singular Gram (the oracle reports Spark's dppsv
failure, status != 0) and rows of n ~ rank ratings are too ill-conditioned for any fp32
solve (textbook error 2.3e-2 at rank 64, n = 64): the bar is applied to the rows the
reference itself holds to it — oracle status 0 and 8 x textbook error <= 1e-4, decided
from the oracle and the textbook solve alone — and the others may go to the rescue.
(2) The two copies of every light row are bitwise equal in every run, whatever the row's
conditioning: a wave reading or writing LDS beyond its trimmed allocation would meet
different neighbours at the two places.  (3) X of ranks 33 and 64 equals the bits recorded
from the parent of this change (tests/golden/k64_rows_bits.npz)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import als_mi355x.engine as E
from oracle import als_oracle as O
from oracle import c_oracle as C
from helpers import fp32_textbook_half_sweep, rel_row_errs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARDSTICK_FACTOR = 8.0  # test_gpu_edges_k2_k3.py


def _recorder():
    spec = importlib.util.spec_from_file_location(
        "record_k64_rows_bits", os.path.join(ROOT, "tools", "record_k64_rows_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
_CASES, _REFS, _CORES = {}, {}, {}


def _case(rank):
    if rank not in _CASES:
        c = REC.case(rank)
        c["csr"] = O.csr_build(c["dst"], c["src"], c["r"], c["n_rows"])
        _CASES[rank] = c
    return _CASES[rank]


def _refs(rank, reg):
    """(oracle X, oracle status, textbook error per row or inf where the textbook fp32
    Cholesky has no solution), once per (rank, reg)."""
    if (rank, reg) not in _REFS:
        c = _case(rank)
        indptr, indices, vals = c["csr"]
        X, st = C.half_sweep(indptr, indices, vals, c["Y"], reg)
        e_tb = np.full(len(st), np.inf)
        rows = np.nonzero((st == 0) & (np.diff(indptr) >= (rank if reg == 0 else 1)))[0]
        ip = np.zeros(len(rows) + 1, np.int64)
        np.cumsum(np.diff(indptr)[rows], out=ip[1:])
        sel = np.concatenate([np.arange(indptr[r], indptr[r + 1]) for r in rows])
        Xt = fp32_textbook_half_sweep(ip, indices[sel], vals[sel], c["Y"], reg)
        e_tb[rows] = rel_row_errs(Xt, X[rows])
        _REFS[(rank, reg)] = (X, st, e_tb)
    return _REFS[(rank, reg)]


def _solve(rank, reg, dual):
    """(X [n_rows, ld], status word, rows the launches sent to the fp64 rescue)."""
    c = _case(rank)
    fresh = rank not in _CORES
    core, X, rescued = REC.solve(E, torch, c, rank, reg, dual, _CORES.get(rank))
    _CORES[rank] = core
    if fresh:
        indptr, indices, vals = c["csr"]
        ub = core.user_block
        np.testing.assert_array_equal(ub.row_ptr.cpu().numpy(), indptr)
        np.testing.assert_array_equal(ub.col.cpu().numpy(), indices)
        assert (ub.n_heavy, ub.n_chunks) == (2, 6)  # the heavy row and the every-source row
        assert ub.n_dual(rank) == 2 * sum(d <= E.dual_limit(rank) for d in REC.LIGHT_DEGREES)
    return X, int(core.status.item()), rescued


def _bits_differ(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


@pytest.fixture(scope="module")
def golden():
    with np.load(REC.GOLDEN) as z:
        return {name: z[name] for name in z.files}


@pytest.mark.parametrize("reg,dual", REC.RUNS, ids=[REC.run_id(0, *r)[3:] for r in REC.RUNS])
@pytest.mark.parametrize("rank", REC.RANKS)
def test_rows_against_oracle_and_copies(rank, reg, dual):
    c = _case(rank)
    deg = np.diff(c["csr"][0])
    X_ref, st, e_tb = _refs(rank, reg)
    if reg > 0:
        assert not st.any() and 0 < YARDSTICK_FACTOR * e_tb.max() <= 1e-4
    posed = (st == 0) & (YARDSTICK_FACTOR * e_tb <= 1e-4)
    # at reg = 0 the reference holds every row of >= 130 ratings (fillers, heavy rows) to the bar
    assert posed[deg >= 130].all() and posed.sum() >= REC.FILLERS + 3
    X, _, rescued = _solve(rank, reg, dual)
    assert np.all(X[:, rank:] == 0.0), "padding columns [rank, ld) must be exactly 0"
    U = X[:, :rank]
    e = rel_row_errs(U[posed], X_ref[posed])
    worst = int(deg[posed][e.argmax()])
    per_degree = {int(d): float(f"{e[deg[posed] == d].max():.3g}")
                  for d in REC.LIGHT_DEGREES + (REC.HEAVY_DEGREE,) if (deg[posed] == d).any()}
    print(f"k64_occupancy4[{REC.run_id(rank, reg, dual)}]: max err {e.max():.3g} (deg {worst}), "
          f"textbook {e_tb[posed].max():.3g}, rescued {rescued}, rows under the bar "
          f"{int(posed.sum())} of {len(posed)}, per degree {per_degree}")
    for a, b in c["copy_of"]:
        assert _bits_differ(X[a], X[b]) == 0, (int(deg[a]), "the two copies of a row differ")
    if reg > 0:
        assert not np.any(X == 7.0), "a destination entry was never written"
        assert rescued == 0, f"{rescued} rows went to the fp64 rescue"
    else:
        assert rescued <= int((~posed).sum()), (rescued, int((~posed).sum()))
    assert e.max() <= 1e-4, (float(e.max()), worst)
    assert e.max() <= YARDSTICK_FACTOR * e_tb[posed].max(), (float(e.max()), worst)


@pytest.mark.parametrize("reg,dual", REC.RUNS, ids=[REC.run_id(0, *r)[3:] for r in REC.RUNS])
@pytest.mark.parametrize("rank", REC.GOLDEN_RANKS)
def test_bits_match_the_parent_recording(rank, reg, dual, golden):
    commit = str(golden["meta/commit"])
    assert REC.digest(_case(rank)) == str(golden[f"k{rank}/inputs_sha256"]), (
        f"rank {rank}: the inputs rebuilt from the seeds differ from those recorded at {commit}")
    X, status, _ = _solve(rank, reg, dual)
    # the status word names the first failing row to arrive (atomicCAS): which one is not fixed
    want_status = int(golden[f"{REC.run_id(rank, reg, dual)}/status"][0])
    assert (status != 0) == (want_status != 0)
    if status:
        assert _refs(rank, reg)[1][status - 1] != 0, "the reported row is singular for the oracle too"
    want = golden[f"{REC.run_id(rank, reg, dual)}/X"]
    assert X.dtype == want.dtype and X.shape == want.shape
    diff = _bits_differ(X, want)
    assert diff == 0, (f"{REC.run_id(rank, reg, dual)}: {diff} of {X.size} values differ from "
                       f"the bits recorded at commit {commit}")


def test_fixture_size():
    assert os.path.getsize(REC.GOLDEN) < 400 * 1024
