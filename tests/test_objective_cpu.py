"""CPU tests of the training objective (K10): the reference's two forms against each other,
the C ABI's host-side behaviour, and the Python surface.  No GPU is needed and nothing is
launched: every native call below returns from its argument checks.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import objective_ref as R
from als_mi355x import _lib
from als_mi355x import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "als_hip.h")
SYMBOLS = ("als_objective_workspace_bytes", "als_objective_side", "als_gram_dot_f64")


def implicit_problem(n_u, n_i, nnz, k, seed):
    """Implicit ratings with r < 0, r = 0, a duplicate pair and user 0 without a positive
    rating; every user and item rated at least once."""
    rng = np.random.default_rng(seed)
    u = np.concatenate([np.arange(n_u), rng.integers(0, n_u, nnz - n_u)])
    i = np.concatenate([rng.integers(0, n_i, n_u - n_i) if n_u > n_i else np.empty(0, np.int64),
                        np.arange(n_i), rng.integers(0, n_i, nnz - max(n_u, n_i))])[:nnz]
    r = rng.integers(-3, 6, nnz).astype(np.float32)   # -3 .. 5: negatives and zeros included
    r[u == 0] = -np.abs(r[u == 0])                      # user 0: nothing positive
    d = int(np.flatnonzero(u != 0)[-1])
    u = np.append(u, u[d])
    i = np.append(i, i[d])                              # a duplicate pair, another rating
    r = np.append(r, np.float32(2.0))
    U = rng.normal(0, 0.4, (n_u, k)).astype(np.float32)
    V = rng.normal(0, 0.4, (n_i, k)).astype(np.float32)
    return u, i, r, U, V


@pytest.mark.parametrize("n_u,n_i,nnz,k", [(30, 20, 150, 6), (7, 5, 16, 3)])
@pytest.mark.parametrize("alpha", [0.01, 1.0, 40.0])
def test_dense_form_equals_sparse_plus_frobenius(n_u, n_i, nnz, k, alpha):
    u, i, r, U, V = implicit_problem(n_u, n_i, nnz, k, seed=n_u)
    assert (r < 0).any() and (r == 0).any() and not (r[u == 0] > 0).any()
    sparse = R.objective(u, i, r, U, V, 0.1, True, alpha)
    dense = R.objective_dense(u, i, r, U, V, 0.1, alpha)
    tol = 1e-12 * sparse["scale"]
    for key in ("objective", "data", "reg"):
        assert abs(sparse[key] - dense[key]) <= tol, (key, sparse[key], dense[key], tol)
    assert (sparse["n"], sparse["n_positive"]) == (dense["n"], dense["n_positive"]) \
        == (len(r), int((r > 0).sum()))
    assert sparse["objective"] == sparse["data"] + sparse["reg"]


def test_explicit_reference_by_hand():
    # two users, two items, rank 1: every number checkable by hand
    U = np.array([[1.0], [2.0]], np.float32)
    V = np.array([[0.5], [1.5]], np.float32)
    u, i, r = [0, 0, 1], [0, 1, 1], [1.0, 2.0, 2.0]
    got = R.objective(u, i, r, U, V, 0.5)
    data = (1 - 0.5) ** 2 + (2 - 1.5) ** 2 + (2 - 3.0) ** 2
    reg = 0.5 * (2 * 1.0 + 1 * 4.0 + 1 * 0.25 + 2 * 2.25)
    assert got == {"objective": data + reg, "data": data, "reg": reg, "scale": data + reg,
                   "n": 3, "n_positive": 3}


def oracle_protocol(rank, implicit, iterations=3):
    """The monotonicity protocol of tests/test_gpu_objective.py with the CPU oracle's
    half-sweeps: L after the start and after every half-sweep."""
    from oracle import als_oracle as O
    u, i, r = R.grouped_problem()
    U = R.grouped_start(200, rank)
    V = np.zeros((150, rank), np.float32)
    ip, up = R.csr(i, u, r, 150), R.csr(u, i, r, 200)
    L = [R.objective(u, i, r, U, V, 0.1, implicit, 1.0)["objective"]]
    for _ in range(iterations):
        V = O.half_sweep(*ip, U, 0.1, implicit, 1.0)
        L.append(R.objective(u, i, r, U, V, 0.1, implicit, 1.0)["objective"])
        U = O.half_sweep(*up, V, 0.1, implicit, 1.0)
        L.append(R.objective(u, i, r, U, V, 0.1, implicit, 1.0)["objective"])
    return L


@pytest.mark.parametrize("implicit", [False, True])
def test_oracle_half_sweeps_never_raise_the_objective(implicit):
    """The invariant the GPU test relies on, on the oracle first (rank 8 here; ranks 48 and
    128 behave alike): every half-sweep lowers L — the worst step of the six
    configurations still lowers it by 0.5 %, against a bound of L (1 + 1e-9) — and the first
    one takes it below half."""
    u, i, r = R.grouped_problem()
    assert len(r) == 4000 and r.min() >= 0.5 and r.max() <= 5.0
    assert np.bincount(u, minlength=200).min() >= 5 and np.bincount(i, minlength=150).min() >= 5
    L = oracle_protocol(8, implicit)
    ratios = [b / a for a, b in zip(L, L[1:])]
    print("oracle protocol rank 8 implicit", implicit, "L", L, "worst ratio - 1", max(ratios) - 1)
    assert max(ratios) <= 1 + 1e-9
    assert L[1] < 0.5 * L[0]


# ------------------------------------------------------------------ C ABI, host side
def test_symbols_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS + ("als_objective_span",):
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} not declared in als_hip.h"
        assert hasattr(raw, name), f"{name} not exported"
        assert name in _lib.SIGNATURES, f"{name} not bound"
    assert _lib.ABI_VERSION == 9 and _lib.lib().als_abi_version() == 9
    assert int(re.search(r"#define ALS_ABI_VERSION (\d+)", open(HEADER).read()).group(1)) == 9


def test_workspace_size_is_monotone():
    ws = _lib.lib().als_objective_workspace_bytes
    assert ws(10 ** 3, 10, 16) < ws(10 ** 8, 10, 16) < ws(10 ** 9, 10, 16)   # by ratings
    assert ws(10, 10 ** 5, 16) < ws(10, 10 ** 5, 64) < ws(10, 10 ** 5, 128)  # by rank
    assert ws(10, 100, 64) <= ws(10, 10 ** 4, 64) <= ws(10, 10 ** 6, 64)     # by rows
    sizes = [ws(0, n, 128) for n in range(1, 40000, 37)]
    assert sizes == sorted(sizes)          # never shrinks as the table grows
    assert ws(0, 0, 1) > 0
    span = _lib.lib().als_objective_span()
    assert span > 0 and span % 16 == 0


def _side_args(**over):
    a = dict(row_ptr=16, col=16, val=16, nnz=100, n_rows=10, n_cols=10, X=16, Y=16, ld=64, k=64,
             implicit=0, alpha=1.0, out=16, ws=16, ws_bytes=1 << 20, stream=0)
    a.update(over)
    return list(a.values())


def _gram_args(**over):
    a = dict(A=16, n_a=10, B=16, n_b=10, ld=64, k=64, out=16, ga=0, gb=0, ws=16,
             ws_bytes=1 << 24, stream=0)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("over,code", [
    (dict(k=0), -4), (dict(k=129, ld=132), -4), (dict(k=64, ld=60), -1), (dict(k=33, ld=34), -1),
    (dict(X=0), -1), (dict(row_ptr=0), -1), (dict(out=0), -1), (dict(nnz=-1), -1),
    (dict(alpha=-1.0), -1), (dict(X=20), -1), (dict(ws_bytes=16), -2), (dict(ws=0), -2)])
def test_objective_side_argument_errors(over, code):
    L = _lib.lib()
    assert L.als_objective_side(*_side_args(**over)) == code
    assert L.als_last_error()


@pytest.mark.parametrize("over,code", [
    (dict(k=0), -4), (dict(k=129, ld=132), -4), (dict(k=64, ld=60), -1), (dict(A=0), -1),
    (dict(B=0), -1), (dict(out=0), -1), (dict(n_a=-1), -1), (dict(ws_bytes=16), -2),
    (dict(ws=0), -2)])
def test_gram_dot_argument_errors(over, code):
    L = _lib.lib()
    assert L.als_gram_dot_f64(*_gram_args(**over)) == code
    assert L.als_last_error()


def test_zero_size_calls_are_noops():
    L = _lib.lib()
    assert L.als_objective_side(0, 0, 0, 0, 0, 0, 0, 0, 4, 4, 0, 1.0, 0, 0, 0, 0) == 0
    assert L.als_objective_side(0, 0, 0, 0, 5, 5, 0, 0, 4, 4, 1, 1.0, 0, 0, 0, 0) == 0
    assert L.als_gram_dot_f64(0, 0, 0, 0, 4, 4, 0, 0, 0, 0, 0, 0) == 0


# ------------------------------------------------------------------ Python surface
def test_set_objective_history_is_a_plain_setter_carried_by_copy():
    from als_mi355x.ml.recommendation import ALS, _Params
    als = ALS(rank=4)
    before = dict(als._p)
    assert als.setObjectiveHistory(2, tol=1e-3) is als
    assert als._p == before and set(als._p) == set(_Params._defaults)
    assert "objective" not in " ".join(_Params._defaults).lower()
    c = als.copy({ALS.rank: 7})
    assert (c._objective_every, c._objective_tol) == (2, 1e-3) and c.getRank() == 7
    assert set(c._p) == set(_Params._defaults)
    fresh = ALS()
    assert (fresh._objective_every, fresh._objective_tol) == (0, None)
    assert ALS().setObjectiveHistory()._objective_every == 1
    with pytest.raises(ValueError):
        ALS().setObjectiveHistory(-1)
    with pytest.raises(ValueError):
        ALS().setObjectiveHistory(1, tol=-0.5)


def test_sharded_engine_refuses_the_objective():
    from als_mi355x.distributed import ShardedALS
    eng = ShardedALS.__new__(ShardedALS)     # no process group: the refusals come first
    with pytest.raises(NotImplementedError, match="sharded engine"):
        eng.objective(0.1)
    with pytest.raises(NotImplementedError, match="sharded engine"):
        eng.fit(4, 1, 0.1, objective_every=1)
    with pytest.raises(NotImplementedError, match="sharded engine"):
        eng.fit(4, 1, 0.1, tol=0.0)


def test_fit_keywords_default_to_off():
    for cls in (E.ALSCore,):
        sig = inspect.signature(cls.fit)
        assert sig.parameters["objective_every"].default == 0
        assert sig.parameters["tol"].default is None
    from als_mi355x.distributed import ShardedALS
    sig = inspect.signature(ShardedALS.fit)
    assert sig.parameters["objective_every"].default == 0 and sig.parameters["tol"].default is None
    assert inspect.signature(E.ALSCore.objective).parameters["implicit"].default is False


def test_model_surface_exists():
    from als_mi355x.ml.recommendation import ALSModel
    from als_mi355x.mllib.recommendation import ALS as MLlibALS, MatrixFactorizationModel
    assert isinstance(ALSModel.objectiveHistory, property)
    assert isinstance(ALSModel.objectiveIterations, property)
    assert callable(ALSModel.trainingObjective)
    assert callable(MatrixFactorizationModel.trainingObjective)
    # the mllib trainers keep their signatures
    assert list(inspect.signature(MLlibALS.train).parameters) == [
        "ratings", "rank", "iterations", "lambda_", "blocks", "nonnegative", "seed"]
    assert list(inspect.signature(MLlibALS.trainImplicit).parameters) == [
        "ratings", "rank", "iterations", "lambda_", "blocks", "alpha", "nonnegative", "seed"]


def test_model_without_a_history_reports_an_empty_one():
    from als_mi355x.ml.recommendation import ALSModel

    class Core:          # what a from_factors core carries
        objective_history = []
        rank = 3
    m = ALSModel(Core(), {})
    assert m.objectiveHistory == [] and m.objectiveIterations == []
    Core.objective_history = [(2, 5.0), (4, 3.0)]
    m = ALSModel(Core(), {})
    Core.objective_history.append((5, 2.0))          # a later fit of the shared core
    assert m.objectiveHistory == [5.0, 3.0] and m.objectiveIterations == [2, 4]
