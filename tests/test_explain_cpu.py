"""CPU tests of explain (K11, als_explain; no GPU, no compute launched).

* tests/explain_ref.py against the existing oracle: the contributions of a row sum to
  y_t . x with x the oracle's solution of the same row.
* The header, the library and the ctypes table agree on the two entry points, under ABI 9.
* als_explain's argument checks run host-side and return the documented codes (small
  integers stand in for pointers; nothing is dereferenced before the checks).
* Host logic: pair grouping, the from_factors core without ratings, the sharded engine.
"""
import inspect
import re

import numpy as np
import pytest
import torch

import explain_ref as R
from als_mi355x import _lib
from als_mi355x import engine as E
from oracle import als_oracle as O
from test_abi import HEADER, _header_signatures, declared_functions

NAMES = ("als_explain", "als_explain_workspace_bytes")


# ------------------------------------------------------------------ reference vs oracle
@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("k", (1, 8, 33))
def test_reference_contributions_sum_to_the_oracle_score(k, implicit):
    """sum_j c_ref = y_t . x_ref per (row, target), relative to ||x|| ||y_t||:
    * to 1e-10 against the oracle's fp64 solution — oracle.normal_equations and the Cholesky
      steps of oracle.solve, which is half_sweep without its closing rounding;
    * to 2^-23 against half_sweep itself, whose rows are rounded to fp32 (2^-24 per
      component, Cauchy-Schwarz, and as much again in reserve): 1e-10 cannot hold there."""
    rng = np.random.default_rng(3 + k)
    n_items, reg, alpha = 60, 0.1, 40.0
    Y = (rng.standard_normal((n_items, k)) / np.sqrt(k)).astype(np.float32)
    lens = [1, 2, 5, k + 1, 40]
    rows = [(rng.integers(0, n_items, n), rng.integers(1, 6, n).astype(np.float32)) for n in lens]
    rows[2][1][1] = -3.0                  # implicit: counts in A, not in b
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    col = np.concatenate([c for c, _ in rows]).astype(np.int32)
    val = np.concatenate([v for _, v in rows])
    X32 = O.half_sweep(ptr, col, val, Y, reg, implicit, alpha).astype(np.float64)
    A, b, ne = O.normal_equations(ptr, col, val, Y, implicit, alpha)
    A = A + (O.yty(Y)[None] if implicit else 0.0)
    A[:, np.arange(k), np.arange(k)] += reg * ne[:, None]
    Lc = np.linalg.cholesky(A)
    X64 = np.linalg.solve(np.transpose(Lc, (0, 2, 1)), np.linalg.solve(Lc, b[..., None]))[..., 0]
    Yd = Y.astype(np.float64)
    targets = rng.integers(0, n_items, 7)
    worst64 = worst32 = 0.0
    for r, (c, v) in enumerate(rows):
        np.testing.assert_allclose(R.solve_row(c, v, Y, reg, implicit, alpha), X64[r],
                                   rtol=0, atol=1e-10 * np.linalg.norm(X64[r]))
        for t, (s, pos, con) in zip(targets, R.explain_row(c, v, Y, targets, reg, implicit,
                                                           alpha)):
            assert len(pos) == len(c) and (np.diff(con) <= 0).all()
            assert abs(con.sum() - s) <= 1e-12 * np.abs(con).sum()
            scale = np.linalg.norm(X64[r]) * np.linalg.norm(Yd[t])
            worst64 = max(worst64, abs(s - Yd[t] @ X64[r]) / scale)
            worst32 = max(worst32, abs(s - Yd[t] @ X32[r]) / scale)
    print(f"explain_ref k={k} implicit={implicit}: vs fp64 oracle {worst64:.2e}, "
          f"vs half_sweep (fp32 rows) {worst32:.2e}")
    assert worst64 <= 1e-10
    assert worst32 <= 2.0 ** -23


def test_reference_rules():
    """Unknown entries are skipped but keep their position; ties go by position; an unknown
    target and a row without a used entry give nothing."""
    Y = np.eye(3, dtype=np.float32)
    cols, vals = [0, -1, 0, 3, 1], [2.0, 5.0, 2.0, 5.0, 1.0]
    (s, pos, con), (s2, p2, c2), (s3, p3, _) = R.explain_row(cols, vals, Y, [0, 1, 7], 0.5,
                                                             False, 1.0)
    assert pos.tolist() == [0, 2, 4] and con[0] == con[1] > 0 and con[2] == 0
    np.testing.assert_allclose(s, 2 * 2.0 / (2 + 1.5))       # A = diag(2, 1, 0) + 0.5 * 3 I
    assert p2.tolist()[0] == 4 and s3 == 0.0 and len(p3) == 0
    assert R.explain_row([-1, 3], [1.0, 1.0], Y, [0], 0.5, False, 1.0)[0][0] == 0.0
    assert R.well_separated([3.0, 3.0, 1.0], [0, 1, 2])
    assert not R.well_separated([3.0, 3.0 - 1e-12, 1.0], [0, 1, 2])


# ------------------------------------------------------------------ ABI
def test_header_library_and_binding_agree():
    import ctypes
    raw = ctypes.CDLL(_lib.LIB_PATH)
    hdr = _header_signatures()
    for name in NAMES:
        assert name in declared_functions()
        assert hasattr(raw, name)
        assert hdr[name] == _lib.SIGNATURES[name][1]
    assert _lib.SIGNATURES["als_explain"][0] is ctypes.c_int
    assert _lib.SIGNATURES["als_explain_workspace_bytes"][0] is _lib.SZ
    assert len(_lib.SIGNATURES["als_explain"][1]) == 23
    assert _lib.ABI_VERSION == 9 == _lib.lib().als_abi_version()
    assert int(re.search(r"#define ALS_ABI_VERSION (\d+)", open(HEADER).read()).group(1)) == 9
    assert _lib.lib().als_explain_workspace_bytes(1000, 128) == 0


def _call(**over):
    a = dict(row_ptr=16, col=16, val=16, n_rows=1, Y=16, n_src=10, ld=64, k=64, reg=0.1,
             implicit=0, alpha=1.0, yty=0, tgt_ptr=16, tgt=16, top_n=10, score=16, pos=16,
             contrib=16, n_used=16, status=16, ws=0, ws_bytes=0, stream=0)
    a.update(over)
    return _lib.lib().als_explain(*a.values())


@pytest.mark.parametrize("over,code", [
    (dict(k=0), -4), (dict(k=129, ld=132), -4),
    (dict(top_n=0), -4), (dict(top_n=33), -4), (dict(top_n=-1), -4),
    (dict(ld=62), -1), (dict(ld=60), -1),
    (dict(row_ptr=0), -1), (dict(col=0), -1), (dict(val=0), -1), (dict(tgt_ptr=0), -1),
    (dict(tgt=0), -1), (dict(score=0), -1), (dict(pos=0), -1), (dict(contrib=0), -1),
    (dict(status=0), -1), (dict(Y=0), -1),
    (dict(implicit=1), -1),            # implicit without yty_packed
    (dict(reg=-1.0), -1), (dict(alpha=-1.0), -1), (dict(n_rows=-1), -1), (dict(n_src=-1), -1),
    (dict(Y=20), -1)])                 # base not 16-byte aligned
def test_argument_errors_before_any_device_call(over, code):
    L = _lib.lib()
    assert _call(**over) == code
    assert L.als_last_error()
    assert b"als_explain" in L.als_last_error()


def test_zero_rows_is_a_noop():
    none = dict(row_ptr=0, col=0, val=0, n_rows=0, Y=0, n_src=0, tgt_ptr=0, tgt=0, score=0,
                pos=0, contrib=0, n_used=0, status=0)
    assert _call(**none) == 0
    assert _call(**none, implicit=1, yty=16, k=1, ld=4, top_n=32) == 0


# ------------------------------------------------------------------ host logic
def test_group_pairs_groups_by_row_in_input_order():
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 7, 100)
    rows[rows == 4] = 5                                  # a row without pairs
    order, tgt_ptr = E.group_pairs(torch.as_tensor(rows), 7)
    order, tgt_ptr = order.numpy(), tgt_ptr.numpy()
    assert tgt_ptr.dtype == np.int64 and tgt_ptr[0] == 0 and tgt_ptr[-1] == 100
    assert sorted(order.tolist()) == list(range(100))
    for r in range(7):
        mine = order[tgt_ptr[r]:tgt_ptr[r + 1]]
        np.testing.assert_array_equal(mine, np.nonzero(rows == r)[0])   # ascending = input order
    assert tgt_ptr[5] == tgt_ptr[4]
    order, tgt_ptr = E.group_pairs(torch.zeros(0, dtype=torch.int64), 3)
    assert order.numel() == 0 and tgt_ptr.tolist() == [0, 0, 0, 0]


def _bare_core(with_factors=True):
    """An ALSCore shell on the CPU: explain's argument checks run before any library call."""
    core = E.ALSCore.__new__(E.ALSCore)
    core.device = torch.device("cpu")
    core.user_block = core.item_block = None
    core.rank = 2
    core.U = torch.zeros((3, 4)) if with_factors else None
    core.V = torch.zeros((3, 4)) if with_factors else None
    ids = torch.arange(3, dtype=torch.int32)
    core.uidx = core.iidx = E.IdIndex(ids.clone(), ids.clone(), 3)
    return core


def test_core_without_ratings_asks_for_them():
    core = _bare_core()
    with pytest.raises(ValueError, match="ratings="):
        core.explain([0, 1], [1, 2], reg=0.1)
    with pytest.raises(ValueError, match="top_n"):
        core.explain([0], [1], 0, reg=0.1)
    with pytest.raises(ValueError, match="top_n"):
        core.explain([0], [1], 33, reg=0.1)
    with pytest.raises(ValueError, match="same length"):
        core.explain([0, 1], [1], reg=0.1)
    with pytest.raises(ValueError, match=">= 0"):
        core.explain([0], [1], reg=-1.0)
    with pytest.raises(ValueError, match="factors"):
        _bare_core(False).explain([0], [1], reg=0.1)
    # no pair has a rating row: the empty result, still without a library call
    out = core.explain([0, 1], [1, 2], 4, reg=0.1, ratings=([7, 7], [0, 1], [3.0, 4.0]))
    assert [tuple(x.shape) for x in out] == [(0,), (0,), (0,), (0, 4), (0, 4), (0, 4), (0,)]


def test_sharded_engine_rejects_explain():
    from als_mi355x import distributed as D
    from als_mi355x import filters
    eng = D.ShardedALS.__new__(D.ShardedALS)  # no process group needed: it refuses at once
    with pytest.raises(NotImplementedError, match="sharded"):
        eng.explain([1], [2], reg=0.1)
    with pytest.raises(NotImplementedError, match="sharded"):
        filters.reject_sharded_explain()
    sharded = inspect.signature(D.ShardedALS.explain)
    single = inspect.signature(E.ALSCore.explain)
    assert list(sharded.parameters) == list(single.parameters)
    assert single.parameters["top_n"].default == sharded.parameters["top_n"].default == 10
    for kw in ("reg", "implicit", "alpha", "user_side", "ratings"):
        assert sharded.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
        assert sharded.parameters[kw].default == single.parameters[kw].default


def test_public_surfaces_carry_the_documented_signatures():
    from als_mi355x import personal
    from als_mi355x.ml.recommendation import ALSModel
    from als_mi355x.mllib.recommendation import MatrixFactorizationModel
    sig = inspect.signature(ALSModel.explainRecommendations)
    assert list(sig.parameters) == ["self", "dataset", "numContributions", "ratings"]
    assert sig.parameters["numContributions"].default == 10
    assert sig.parameters["ratings"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(MatrixFactorizationModel.explain)
    assert list(sig.parameters) == ["self", "user_product", "lambda_", "num", "implicit", "alpha",
                                    "ratings"]
    assert sig.parameters["num"].default == 10 and sig.parameters["alpha"].default == 0.01
    assert list(inspect.signature(personal.personal_explanations).parameters)[:4] == [
        "model", "rated", "movies", "movie_ids"]
    assert personal.personal_explanations(None, [], [], [1], 0.1) == []
