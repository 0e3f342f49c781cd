"""Nonnegative ALS (K13) without a GPU: the numpy restatement of Spark's NNLS solver
(tests/nnls_ref.py) against the exact constrained minimiser and hand cases, and the host side
of the surfaces that reach the kernel (setSolver, trainNonnegative, the refusals, the ABI).

The exact minimiser of x^T A x / 2 - b^T x over x >= 0 is scipy.optimize.nnls on the
Cholesky factor: with A = L L^T, |L^T x - L^-1 b|^2 = x^T A x - 2 b^T x + const.
"""
import inspect

import numpy as np
import pytest
import torch

import nnls_ref as R
from als_mi355x import _lib, engine as E, filters
from als_mi355x.ml.recommendation import ALS as MLALS
from als_mi355x.ml.recommendation import ALSModel
from als_mi355x.mllib.recommendation import ALS as MLlibALS
from als_mi355x.mllib.recommendation import MatrixFactorizationModel
from oracle import als_oracle as O
from test_abi import _header_signatures, declared_functions

REG = 0.1
NAMES = ("als_nnls_rows", "als_nnls_workspace_bytes")


def _system(k, deg, signed, seed=0, scale=1.0):
    """(A, b) of one explicit row: deg ratings of unit-norm (signed) or |unit-norm| sources."""
    rng = np.random.default_rng(1000 * k + 10 * deg + seed + (1 if signed else 0))
    Y = rng.standard_normal((500, k))
    Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    if not signed:
        Y = np.abs(Y)
    Y = (Y * scale).astype(np.float32)
    idx = rng.integers(0, 500, deg)
    r = (rng.integers(1, 11, deg) / 2.0).astype(np.float32)
    A, b, used = R.systems(np.array([0, deg]), idx, r, Y, REG)
    assert used[0] == deg
    return A[0], b[0]


def _rel(x, ref):
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-30))


# ------------------------------------------------------------------ the reference itself
def _issue_systems():
    """The systems of the CPU check the algorithm was accepted on, drawn exactly as that check
    drew them (one generator, seed 0, ranks and degrees in this order, fp64 unit-norm sources
    and their absolute values, half-star ratings, lambda 0.1): {(k, deg, signed): (A, b)}."""
    rng = np.random.default_rng(0)
    out = {}
    for k in (4, 16, 64, 128):
        for deg in (1, 3, k, 4 * k, 1000):
            Y = rng.standard_normal((500, k))
            Y /= np.linalg.norm(Y, axis=1, keepdims=True)
            for signed, T in ((True, Y), (False, np.abs(Y))):
                idx = rng.integers(0, 500, deg)
                r = rng.integers(1, 11, deg) / 2.0
                out[(k, deg, signed)] = (T[idx].T @ T[idx] + REG * deg * np.eye(k), T[idx].T @ r)
                rng.permutation(k)   # the check drew a summation order here
    return out


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "abs"])
@pytest.mark.parametrize("k", [4, 16, 64, 128])
def test_reference_reaches_the_exact_minimiser(k, signed):
    """<= 1e-6 per row against the exact constrained minimiser.  The solver's own stopping
    rule (squared direction below 1e-12 |x|^2) is of that order: an independent draw with
    fp32 sources measured 1.4e-6 at k = 128 with 3 ratings, so the cases are the accepted
    check's own draws."""
    so = pytest.importorskip("scipy.optimize")
    cases = _issue_systems()
    worst = 0.0
    for deg in (1, 3, k, 4 * k, 1000):
        A, b = cases[(k, deg, signed)]
        info = {}
        x = R.nnls_solve(A, b, info)
        L = np.linalg.cholesky(A)
        xe, _ = so.nnls(L.T, np.linalg.solve(L, b), maxiter=10000)
        err = _rel(x, xe)
        worst = max(worst, err)
        print(f"nnls_ref k={k} deg={deg} signed={signed}: iters {info['iters']}, "
              f"on the wall {(x == 0).sum()}, rel err {err:.2e}")
        assert (x >= 0).all()
        assert info["iters"] < max(400, 20 * k)   # stopped by its own test, not by iterMax
        assert err <= 1e-6
    print(f"nnls_ref k={k} signed={signed}: worst {worst:.2e}")


def test_b_not_positive_gives_exactly_zero():
    """b <= 0: the gradient -b at x = 0 is >= 0 everywhere and is projected away entirely, so
    the first test stops the solver at x = 0 — the minimiser, whatever A is."""
    for signed in (True, False):
        A, b = _system(16, 40, signed)
        for bb in (np.zeros(16), -np.abs(b), np.where(np.arange(16) % 2 == 0, -np.abs(b), 0.0)):
            info = {}
            x = R.nnls_solve(A, bb, info)
            assert info["iters"] == 0
            assert (x == 0).all() and not np.signbit(x).any()


def test_diagonal_system():
    d = np.array([0.5, 2.0, 4.0, 1.0, 8.0])
    b = np.array([1.0, -3.0, 2.0, 0.0, -0.5])
    x = R.nnls_solve(np.diag(d), b)
    np.testing.assert_allclose(x, np.maximum(b / d, 0.0), rtol=1e-6, atol=0)
    assert (x[[1, 3, 4]] == 0).all()


def test_positive_unconstrained_solution_is_the_cholesky_one():
    rng = np.random.default_rng(3)
    k = 12
    Y = np.abs(rng.standard_normal((60, k))).astype(np.float32)
    x_true = rng.uniform(0.5, 1.5, k)
    idx = np.arange(60)
    r = (Y.astype(np.float64) @ x_true).astype(np.float32)
    A, b, used = R.systems(np.array([0, 60]), idx, r, Y, 1e-3)
    chol = np.linalg.solve(A[0], b[0])
    assert (chol > 0).all()
    x = R.nnls_solve(A[0], b[0])
    assert _rel(x, chol) <= 1e-6
    # and through the oracle's own solver, which sees A without the regulariser
    A0, b0, ne = O.normal_equations(np.array([0, 60]), idx, r, Y)
    ref = O.solve(A0, b0, ne, 1e-3)[0]
    assert _rel(x.astype(np.float32), ref) <= 1e-6


def test_early_stop_of_a_large_system():
    """Spark's `step < 1e-7` test stops a row whose A is large at x = 0: reproduced, not
    repaired.  Sources scaled by 1e4: A ~ 1e8, so the first step is ~ 1e-8 or smaller."""
    A, b = _system(8, 16, True, scale=1e4)
    info = {}
    x = R.nnls_solve(A, b, info)
    assert 0 < info["first_step"] < 1e-8
    assert info["iters"] == 0
    assert (x == 0).all()


def test_kkt_yardstick_is_positive():
    """The KKT residual of the reference's own fp32-rounded rows is the yardstick of the GPU
    test's third bar: it is > 0 (rounding to fp32 alone leaves a residual), so that bar is
    never vacuous, and it is zero only at an exact minimiser."""
    for signed in (True, False):
        A, b = _system(16, 64, signed)
        x = R.nnls_solve(A, b)
        x32 = x.astype(np.float32).astype(np.float64)
        assert R.kkt(A, b, x32) > 0
        assert R.kkt(A, b, x32) < 1e-5
        assert R.kkt(A, b, x) < 1e-5
    assert R.kkt(np.eye(2), np.array([1.0, -1.0]), np.array([1.0, 0.0])) == 0.0


def test_reference_fit_is_nonnegative_and_follows_the_oracle_loop():
    rng = np.random.default_rng(5)
    u = rng.integers(0, 30, 300)
    i = rng.integers(0, 20, 300)
    r = rng.integers(1, 6, 300).astype(np.float32)
    hist = []
    U, V, umap, imap, uids, iids = R.fit(u, i, r, 4, 2, REG, seed=1, history=hist)
    assert (U >= 0).all() and (V >= 0).all() and len(hist) == 2
    assert U.dtype == V.dtype == np.float32
    # same start as the Cholesky oracle: the solver is the only difference
    U0 = O.initialize(len(uids), 4, 1)
    U2, V2 = R.fit(u, i, r, 4, 2, REG, U0=U0)[:2]
    np.testing.assert_array_equal(U, U2)
    np.testing.assert_array_equal(V, V2)


# ------------------------------------------------------------------ ABI and engine, host side
def test_abi_declares_and_binds_the_new_symbols():
    import ctypes
    raw = ctypes.CDLL(_lib.LIB_PATH)
    hdr = _header_signatures()
    for name in NAMES:
        assert name in declared_functions()
        assert hasattr(raw, name)
        assert hdr[name] == _lib.SIGNATURES[name][1]


def _nnls_args(**over):
    a = dict(row_ptr=16, col=16, val=16, n_rows=1, Y=16, n_src=1, ld=64, k=64, reg=0.1,
             implicit=0, alpha=1.0, yty=0, chunk=4096, X=16, ld_out=64, n_used=0, iters=0,
             ws=16, ws_bytes=1 << 24, stream=0)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("over,code", [
    (dict(k=0), -4), (dict(k=129, ld=132, ld_out=132), -4), (dict(ld=62), -1), (dict(ld=32), -1),
    (dict(ld_out=60), -1), (dict(n_rows=-1), -1), (dict(n_src=-1), -1), (dict(reg=-1.0), -1),
    (dict(alpha=-1.0), -1), (dict(implicit=1), -1), (dict(chunk=0), -1), (dict(row_ptr=0), -1),
    (dict(X=0), -1), (dict(Y=0), -1), (dict(Y=20), -1), (dict(ws=0), -1), (dict(ws=8), -1),
    (dict(ws_bytes=64), -2)])
def test_nnls_argument_errors_are_host_side(over, code):
    L = _lib.lib()
    assert L.als_nnls_rows(*_nnls_args(**over)) == code
    assert L.als_last_error()


def test_nnls_zero_rows_and_workspace_size():
    L = _lib.lib()
    assert L.als_nnls_rows(*_nnls_args(n_rows=0, row_ptr=0, col=0, val=0, X=0, ws=0)) == 0
    ws = L.als_nnls_workspace_bytes
    assert ws(0, 0, 64, 4096) == 0 and ws(10, 10, 0, 4096) == 0 and ws(10, 10, 129, 4096) == 0
    assert ws(10, 10, 64, 0) == 0
    assert 0 < ws(10, 100, 64, 4096) < ws(10 ** 5, 100, 64, 4096)
    # rows longer than chunk need a slot per task; none can exist when nnz <= chunk
    assert ws(10, 4096, 64, 4096) < ws(10, 10 ** 6, 64, 4096)
    assert ws(10, 10 ** 6, 64, 4096) < ws(10, 10 ** 6, 128, 4096)
    assert ws(10, 10 ** 6, 64, 4096) < ws(10, 10 ** 6, 64, 64)


def test_flag_defaults_to_off_everywhere():
    for fn in (E.ALSCore.fit, E.ALSCore.iterate, E.ALSCore.half_sweep_items,
               E.ALSCore.half_sweep_users, E.ALSCore.fold_in, E.ALSCore.recommend_new,
               MatrixFactorizationModel.foldInUsers,
               MatrixFactorizationModel.recommendProductsForNewUsers):
        assert inspect.signature(fn).parameters["nonnegative"].default is False, fn
    for fn in (ALSModel.foldInUsers, ALSModel.foldInItems, ALSModel.recommendForNewUsers):
        assert inspect.signature(fn).parameters["nonnegative"].default is None, fn
    for name in ("fold_in", "recommend_new"):
        assert inspect.signature(getattr(E.ALSCore, name)).parameters["nonnegative"].kind \
            is inspect.Parameter.KEYWORD_ONLY
    assert callable(E.nnls_rows)
    assert list(inspect.signature(MLlibALS.trainNonnegative).parameters) == [
        "ratings", "rank", "iterations", "lambda_", "seed", "implicitPrefs", "alpha"]
    sig = inspect.signature(MLlibALS.trainNonnegative)
    assert (sig.parameters["iterations"].default, sig.parameters["lambda_"].default,
            sig.parameters["alpha"].default) == (5, 0.01, 0.01)


def test_nonnegative_fit_refuses_a_checkpoint_directory(tmp_path):
    core = E.ALSCore.__new__(E.ALSCore)   # refused before anything is touched
    with pytest.raises(ValueError, match="checkpoint"):
        core.fit(4, 2, 0.1, nonnegative=True, checkpoint_dir=str(tmp_path))


# ------------------------------------------------------------------ surfaces
def test_set_solver_validates_and_copy_keeps_it():
    als = MLALS(rank=3)
    assert als.getSolver() == "cholesky"
    assert als.setSolver("nnls") is als and als.getSolver() == "nnls"
    for bad in ("NNLS", "qr", None, True):
        with pytest.raises(ValueError, match="solver"):
            als.setSolver(bad)
    assert als.getSolver() == "nnls"
    assert als.copy().getSolver() == "nnls"
    assert als.copy({MLALS.rank: 5}).getSolver() == "nnls"
    assert als.setSolver("cholesky").copy().getSolver() == "cholesky"
    # not a Spark Param: not among the params, so neither saved nor enumerated by the tuners
    assert "solver" not in MLALS._defaults and not hasattr(MLALS, "solver")


def test_model_records_the_solver_and_load_defaults_to_cholesky():
    core = E.ALSCore.__new__(E.ALSCore)
    m = ALSModel(core, dict(MLALS()._p), solver="nnls")
    assert m.solver == "nnls" and m._nonnegative(None) is True and m._nonnegative(False) is False
    m = ALSModel(core, dict(MLALS()._p))          # what load() builds
    assert m.solver == "cholesky" and m._nonnegative(None) is False
    assert m._nonnegative(True) is True


def test_spark_spellings_still_raise_and_name_the_new_ones():
    import pandas as pd
    df = pd.DataFrame({"user": [0, 1], "item": [0, 1], "rating": [1.0, 2.0]})
    with pytest.raises(NotImplementedError, match=r'setSolver\("nnls"\)'):
        MLALS(nonnegative=True).fit(df)
    with pytest.raises(NotImplementedError, match="trainNonnegative"):
        MLlibALS.train([(0, 0, 1.0)], 4, nonnegative=True)
    with pytest.raises(NotImplementedError, match="trainNonnegative"):
        MLlibALS.trainImplicit([(0, 0, 1.0)], 4, nonnegative=True)
    with pytest.raises(ValueError):
        MLlibALS.trainNonnegative([(0, 0, 1.0)], 0)
    with pytest.raises(NotImplementedError):
        MLlibALS.trainNonnegative([(0, 0, 1.0)], 129)


def test_sharded_engine_refuses_the_flag(monkeypatch):
    import torch.distributed as dist
    from als_mi355x import distributed as D
    assert D.reject_sharded_nonnegative is filters.reject_sharded_nonnegative
    assert "reject_sharded_nonnegative" in filters.__all__
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 4)
    made = {}
    monkeypatch.setattr(D.ShardedALS, "__init__", lambda self, *a, **k: made.update(s=1))
    eng = E.make_engine([1], [2], [3.0])
    assert isinstance(eng, D.ShardedALS) and made
    with pytest.raises(NotImplementedError, match="sharded"):
        eng.fit(4, 2, 0.1, nonnegative=True)
    with pytest.raises(NotImplementedError, match="sharded"):
        eng.fold_in([1], [2], [3.0], reg=0.1, nonnegative=True)
    with pytest.raises(NotImplementedError, match="sharded"):
        MLlibALS.trainNonnegative([(0, 0, 1.0)], 4)
    assert inspect.signature(D.ShardedALS.fit).parameters["nonnegative"].default is False
    assert isinstance(torch.zeros(1), torch.Tensor)
