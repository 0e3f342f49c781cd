"""The explicit rank 33-64 launch-1 solve on both sides of k == k_pad: rank 64 runs
gram_solve_kernel<4, false>, compiled for the full rank (no test of a dim against k, the lean
diagonal-block sweep), ranks 33, 48 and 63 run gram_solve_kernel<-4, false> with the run-time
masks (csrc/gram_solve.hip).  One explicit problem (tools/record_k64_full_bits.py case()): rows
of 33, 63, 64, 65, 96, 97, 127, 128, 129 and 4,095 ratings, each twice at two places of the
task order, 178 fillers, one heavy row of 4,097 ratings (chunk tasks in the same launch); the
dual path off, so every light row goes through the primal kernel.

(a) / (b) per rank, reg 0.1: per-row ||x - ref|| / ||ref|| <= 1e-4 against the fp64 oracle
(oracle.c_oracle.half_sweep), no row rescued; the two copies of every edge row bitwise equal; X
bitwise equal to the recording taken from the parent of the kernel split
(tests/golden/k64_full_bits.npz).  (c) rank 64, ld = 68: columns 64-67 of every row are zero
on a 0xFF-filled X, the rest equal to the ld = 64 run.  (d) rank 64, reg = 0: the rows shorter
than the rank still reach the fp64 rescue — as many rescued rows as on the parent, X equal to
the recording.  (e) rank 64, one row's ratings scaled by 2^-20: the window guard still routes
it to the rescue (one rescued row more than without the scaling: both of its copies are
scaled, so two), X equal to the recording and inside the bar."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import als_mi355x.engine as E
from oracle import als_oracle as O
from oracle import c_oracle as C
from helpers import rel_row_errs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location(
        "record_k64_full_bits", os.path.join(ROOT, "tools", "record_k64_full_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
_RUNS = {}


def _run(name):
    """(case, X, status, rescued) of a run, once."""
    if name not in _RUNS:
        rank, c = REC.run_case(name)
        _RUNS[name] = (c,) + REC.solve(E, torch, name, c)
    return _RUNS[name]


def _oracle(c, reg):
    indptr, indices, vals = O.csr_build(c["dst"], c["src"], c["r"], c["n_rows"])
    X, st = C.half_sweep(indptr, indices, vals, c["Y"], reg)
    return X, st, np.diff(indptr)


def _bits_differ(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


@pytest.fixture(scope="module")
def golden():
    with np.load(REC.GOLDEN) as z:
        return {name: z[name] for name in z.files}


def _check_recording(name, golden):
    c, X, status, rescued = _run(name)
    commit = str(golden["meta/commit"])
    assert REC.digest(c) == str(golden[f"{name}/inputs_sha256"]), (
        f"{name}: the inputs rebuilt from the seeds differ from those recorded at {commit}")
    want = golden[f"{name}/X"]
    assert X.dtype == want.dtype and X.shape == want.shape
    diff = _bits_differ(X, want)
    print(f"k64_full[{name}]: rescued {rescued} (recorded {int(golden[f'{name}/rescued'][0])}), "
          f"{diff} of {X.size} values differ from the recording")
    assert rescued == int(golden[f"{name}/rescued"][0])
    assert (status != 0) == (int(golden[f"{name}/status"][0]) != 0)
    assert diff == 0, f"{name}: {diff} of {X.size} values differ from the bits recorded at {commit}"


@pytest.mark.parametrize("rank", REC.RANKS)
def test_rows_against_oracle_copies_and_recording(rank, golden):
    name = f"k{rank}-reg0.1"
    c, X, status, rescued = _run(name)
    X_ref, st, deg = _oracle(c, REC.REG)
    assert not st.any() and status == 0
    assert sorted(set(REC.EDGE_DEGREES) | {REC.HEAVY_DEGREE}) == sorted(
        set(deg.tolist()) & (set(REC.EDGE_DEGREES) | {REC.HEAVY_DEGREE}))
    assert np.all(X[:, rank:] == 0.0), "padding columns [rank, ld) must be exactly 0"
    assert not np.any(X == 7.0), "a destination entry was never written"
    e = rel_row_errs(X[:, :rank], X_ref)
    print(f"k64_full[{name}]: max err {e.max():.3g} (a {int(deg[e.argmax()])}-rating row), "
          f"rescued {rescued}")
    assert rescued == 0, f"{rescued} rows went to the fp64 rescue"
    assert e.max() <= 1e-4, (float(e.max()), int(deg[e.argmax()]))
    for a, b in c["copy_of"]:
        assert _bits_differ(X[a], X[b]) == 0, (int(deg[a]), "the two copies of a row differ")
    _check_recording(name, golden)


def test_rank64_ld68_pads_with_zeros(golden):
    c, X, status, rescued = _run("k64-ld68")
    assert X.shape[1] == 68 and status == 0 and rescued == 0
    assert _bits_differ(X[:, 64:], np.zeros_like(X[:, 64:])) == 0, "columns [64, 68) must be +0"
    assert _bits_differ(X[:, :64], _run("k64-reg0.1")[1][:, :64]) == 0
    _check_recording("k64-ld68", golden)


def test_rank64_reg0_short_rows_reach_the_rescue(golden):
    c, X, status, rescued = _run("k64-reg0")
    _, st, deg = _oracle(c, 0.0)
    short = int((deg < 64).sum())
    print(f"k64_full[k64-reg0]: {short} rows shorter than the rank, rescued {rescued}")
    assert short == 4 and rescued >= short  # both copies of the 33- and 63-rating rows
    for a, b in c["copy_of"]:
        assert _bits_differ(X[a], X[b]) == 0, (int(deg[a]), "the two copies of a row differ")
    _check_recording("k64-reg0", golden)


def test_rank64_tiny_ratings_row_takes_the_window_guard(golden):
    c, X, status, rescued = _run("k64-tiny")
    X_ref, st, deg = _oracle(c, REC.REG)
    tiny = list(c["copy_of"][REC.EDGE_DEGREES.index(REC.TINY_DEGREE)])
    assert np.abs(c["r"][np.isin(c["dst"], tiny)]).max() <= 5.0 * REC.TINY_SCALE
    base = _run("k64-reg0.1")[3]
    print(f"k64_full[k64-tiny]: rescued {rescued} (unscaled ratings: {base})")
    assert rescued == base + 2, "both copies of the scaled row go to the fp64 rescue"
    e = rel_row_errs(X[:, :64], X_ref)
    assert not st.any() and status == 0 and e.max() <= 1e-4, (float(e.max()), int(e.argmax()))
    assert _bits_differ(X[tiny[0]], X[tiny[1]]) == 0
    _check_recording("k64-tiny", golden)


def test_fixture_size():
    assert os.path.getsize(REC.GOLDEN) < 600 * 1024
