"""CPU tests of K19, co-rated neighbours (no GPU needed, no compute launched).

* co_rated_ref.py agrees with a hand-worked 4-user x 5-item example, with and without a
  duplicate entry.
* ALSCore.co_rated / co_rated_all and the binding refuse bad arguments before any kernel.
* The header, _lib.py and the exported symbols agree on the four entry points.
* als_co_rated_scratch_bytes is monotone in each argument and runs without a device.
* als_co_rated returns ALS_EINVAL on the host for bad arguments; zero queries are a no-op.
"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import co_rated_ref as R
from als_mi355x import _lib, filters
from als_mi355x import engine as E

NAMES = ("als_co_rated", "als_co_rated_scratch_bytes", "als_co_rated_task", "als_co_rated_window")

# (user, item): u0 rated 0 1 2, u1 rated 0 1, u2 rated 1 3, u3 rated 0 4
PAIRS = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 1), (2, 3), (3, 0), (3, 4)]


def _B(pairs):
    u, i = np.array(pairs).T
    return R.multiplicity(u, i, 4, 5)


def test_reference_on_the_hand_worked_example():
    B = _B(PAIRS)
    assert B.sum(0).tolist() == [3, 3, 1, 1, 1]
    idx, sc, com = R.co_rated(B, [0], 4, "jaccard")
    # c(0,1) = 2 (u0, u1), c(0,2) = 1 (u0), c(0,3) = 0, c(0,4) = 1 (u3)
    assert idx.tolist() == [[1, 2, 4, -1]] and com.tolist() == [[2, 1, 1, 0]]
    want = np.array([2 / 4, 1 / 3, 1 / 3], np.float64).astype(np.float32)
    assert sc[0, :3].tobytes() == want.tobytes() and sc[0, 3] == -np.inf
    _, sc, _ = R.co_rated(B, [0], 3, "cosine")
    want = (np.array([2, 1, 1]) / np.sqrt(np.array([9.0, 3.0, 3.0]))).astype(np.float32)
    assert sc[0].tobytes() == want.tobytes()
    idx, sc, com = R.co_rated(B, [0], 2, "count", min_common=2)
    assert idx.tolist() == [[1, -1]] and sc[0, 0] == 2.0 and com.tolist() == [[2, 0]]
    allow = np.array([1, 0, 1, 1, 1], bool)
    idx, _, _ = R.co_rated(B, [0, 3, -1, 5], 2, "count", allow=allow)
    assert idx.tolist() == [[2, 4], [-1, -1], [-1, -1], [-1, -1]]   # 3's only co-rated row is 1
    # the user side is the same with the blocks swapped: users 0 and 1 share items 0 and 1
    idx, _, com = R.co_rated(B.T, [0], 3, "count")
    assert idx.tolist() == [[1, 2, 3]] and com.tolist() == [[2, 1, 1]]


def test_reference_counts_duplicates_with_their_multiplicity():
    B = _B(PAIRS + [(3, 0)])             # u3 rated item 0 twice
    assert B[3, 0] == 2 and B.sum(0)[0] == 4
    idx, sc, com = R.co_rated(B, [0], 3, "jaccard")
    # c(0,4) = 2 x 1, c(0,1) = 2, c(0,2) = 1; n_0 = 4
    assert idx.tolist() == [[4, 1, 2]] and com.tolist() == [[2, 2, 1]]
    want = np.array([2 / 3, 2 / 5, 1 / 4], np.float64).astype(np.float32)
    assert sc[0].tobytes() == want.tobytes()
    idx, _, _ = R.co_rated(B, [0], 3, "count")
    assert idx.tolist() == [[1, 4, 2]]   # 1 and 4 tie on the count: rows ascending
    _, sc, com = R.co_rated(B, [4], 1, "jaccard")
    assert com.tolist() == [[2]] and sc[0, 0] == np.float32(2 / 3)


def test_reference_csr_keeps_input_order():
    u, i = np.array(PAIRS + [(3, 0)]).T
    rp, col = R.csr(i, u, 5)
    assert rp.tolist() == [0, 4, 7, 8, 9, 10] and col.tolist() == [0, 1, 3, 3, 0, 1, 2, 0, 2, 3]


def test_near_tie_positions_marks_only_one_ulp_neighbours():
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2))
    s = np.array([[2.0, up, one, one, 0.5, -np.inf]], np.float32)
    assert R.near_tie_positions(s).tolist() == [[False, True, True, False, False, False]]


# ---------------------------------------------------------------- ABI
def test_header_binding_and_library_agree():
    from test_abi import _header_signatures, declared_functions
    hdr = _header_signatures()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared_functions() and hasattr(raw, name)
        assert hdr[name] == _lib.SIGNATURES[name][1], name
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("als_co_rated")) == sorted(NAMES)
    assert _lib.SIGNATURES["als_co_rated"][0] is ctypes.c_int
    assert _lib.SIGNATURES["als_co_rated_scratch_bytes"][0] is _lib.SZ
    assert _lib.SIGNATURES["als_co_rated_task"][0] is _lib.I32
    assert _lib.ABI_VERSION == _lib.lib().als_abi_version()
    for name in NAMES:   # the guard-band registry of *_workspace_bytes is not touched
        assert not name.endswith("_workspace_bytes")


def test_every_co_rated_size_function_has_a_bounds_case():
    import test_gpu_co_rated_bounds as BB
    sizers = sorted(n for n in _lib.SIGNATURES
                    if n.startswith("als_co_rated_") and n.endswith("_bytes"))
    assert sizers == sorted(BB.SCRATCH_CASES) and sizers
    for name, tests in BB.SCRATCH_CASES.items():
        assert tests
        for t in tests:
            assert callable(getattr(BB, t, None)), f"{name}: {t} is not a test of the bounds file"


def test_constants_and_scratch_size_without_a_device():
    L = _lib.lib()
    assert L.als_co_rated_task() >= 64
    W = L.als_co_rated_window()
    assert W == L.als_list_exposure_window() and W & (W - 1) == 0
    assert E.co_rated_task() == L.als_co_rated_task() and E.co_rated_window() == W
    size = L.als_co_rated_scratch_bytes
    assert size(1000, 1, 10, 0) > 4 * 1000
    # monotone in each argument
    assert size(1000, 1, 10, 0) <= size(10 ** 5, 1, 10, 0) <= size(10 ** 7, 1, 10, 0)
    assert size(10 ** 5, 1, 10, 0) < size(10 ** 5, 8, 10, 0) <= size(10 ** 5, 32, 10, 0)
    assert size(10 ** 5, 32, 10, 0) == size(10 ** 5, 1000, 10, 0)      # one pass in flight
    tops = [size(10 ** 5, 8, t, 0) for t in (1, 2, 10, 100, 127, 128, 200, 255, 256)]
    assert tops == sorted(tops) and tops[0] < tops[-1]
    passes = [size(10 ** 5, 64, 10, p) for p in (1, 2, 3, 16, 32, 64)]
    assert passes == sorted(passes) and passes[0] < passes[-1]
    assert size(10 ** 5, 64, 10, 0) == size(10 ** 5, 64, 10, E.CO_RATED_PASS)
    assert size(10 ** 5, 64, 10, 64) >= 4 * 64 * 10 ** 5                # the strips
    for bad in ((-1, 1, 10, 0), (10, -1, 10, 0), (10, 1, 0, 0), (10, 1, 257, 0), (10, 1, 10, -1),
                (10, 1, 10, E.CO_RATED_MAX_PASS + 1), (2 ** 31 - 1, 1, 10, 0)):
        assert size(*bad) == 0, bad


def _call(**over):
    a = dict(row_ptr_q=8, col_q=4, n=5, row_ptr_o=8, col_o=4, n_o=4, q_rows=4, n_q=2, measure=1,
             min_common=1, allow=0, top=3, pas=0, task=0, idx=4, score=4, common=4, ws=256,
             ws_bytes=1 << 30, stream=0)
    a.update(over)
    return _lib.lib().als_co_rated(*a.values())


@pytest.mark.parametrize("over", [
    dict(top=0), dict(top=257), dict(measure=-1), dict(measure=3), dict(min_common=0),
    dict(min_common=-5), dict(n=-1), dict(n_o=-1), dict(n_q=-1), dict(n=2 ** 31 - 1),
    dict(pas=-1), dict(pas=65), dict(task=-1), dict(task=(1 << 20) + 1), dict(q_rows=0),
    dict(idx=0), dict(score=0), dict(common=0), dict(row_ptr_q=0), dict(row_ptr_o=0),
    dict(ws=264)])
def test_argument_errors_before_any_device_call(over):
    assert _call(**over) == -1
    assert b"als_co_rated" in _lib.lib().als_last_error()


def test_short_scratch_and_zero_queries():
    assert _call(ws_bytes=16) == -2 and _call(ws=0) == -2
    assert _call(n_q=0, q_rows=0, idx=0, score=0, common=0, ws=0, ws_bytes=0) == 0
    assert _call(n_q=0, top=0) == -1      # the ranges are checked even for a no-op


# ---------------------------------------------------------------- binding and engine
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name}) before the range checks")


@pytest.mark.parametrize("kw", [
    dict(top=0), dict(top=257), dict(measure="pearson"), dict(min_common=0),
    dict(pass_queries=0), dict(pass_queries=65), dict(task_entries=0)])
def test_binding_range_checks_raise_value_error(monkeypatch, kw):
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    a = dict(top=3, measure="jaccard", min_common=1, pass_queries=None, task_entries=None)
    a.update(kw)
    side = (torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32))
    with pytest.raises(ValueError):
        E.co_rated_rows(side, side, torch.zeros(1, dtype=torch.int32), a["top"], a["measure"],
                        a["min_common"], None, E.Workspace("cpu"), a["pass_queries"],
                        a["task_entries"])


def test_engine_argument_errors_need_no_kernel(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    core = E.ALSCore.__new__(E.ALSCore)
    core.device = torch.device("cpu")
    core.user_block = core.item_block = None     # what from_factors leaves
    for kw in (dict(top=0), dict(top=257), dict(top=3, measure="pearson"),
               dict(top=3, min_common=0)):
        with pytest.raises(ValueError, match="top|measure|min_common"):
            core.co_rated([1], **kw)
        with pytest.raises(ValueError, match="top|measure|min_common"):
            core.co_rated_all(**kw)
    for side in (False, True):
        with pytest.raises(ValueError, match="training ratings"):
            core.co_rated([1], 3, side)
        with pytest.raises(ValueError, match="training ratings"):
            core.co_rated_all(3, side)
    sig = inspect.signature(E.ALSCore.co_rated)
    assert list(sig.parameters) == ["self", "ids", "top", "user_side", "measure", "min_common",
                                    "candidates"]
    assert sig.parameters["measure"].default == "jaccard"
    assert sig.parameters["measure"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "len^2" in E.ALSCore.co_rated_all.__doc__ and "n^2" in E.ALSCore.co_rated_all.__doc__


def test_sharded_engine_refuses_with_the_single_gpu_signature():
    from als_mi355x import distributed as D
    eng = D.ShardedALS.__new__(D.ShardedALS)
    with pytest.raises(NotImplementedError, match="sharded"):
        eng.co_rated([1], 3)
    with pytest.raises(NotImplementedError, match="sharded"):
        eng.co_rated_all(3)
    with pytest.raises(NotImplementedError, match="sharded"):
        filters.reject_sharded_co_rated()
    for name in ("co_rated", "co_rated_all"):
        assert (list(inspect.signature(getattr(D.ShardedALS, name)).parameters)
                == list(inspect.signature(getattr(E.ALSCore, name)).parameters))


def test_list_agreement_of_two_id_tables():
    from als_mi355x.ml.recommendation import ALSModel
    a = torch.tensor([[1, 2, 3], [4, 5, 6]])
    ok = torch.ones_like(a, dtype=torch.bool)
    assert ALSModel._list_agreement(a, ok, a.flip(1), ok, 3) == 1.0
    b = torch.tensor([[3, 9, 1], [7, 8, 9]])
    assert ALSModel._list_agreement(a, ok, b, ok, 3) == pytest.approx((2 / 3 + 0) / 2)
    some = torch.tensor([[True, True, False], [True, True, True]])
    assert ALSModel._list_agreement(a, ok, b, some, 3) == pytest.approx((1 / 3 + 0) / 2)
    assert np.isnan(ALSModel._list_agreement(a[:0], ok[:0], b[:0], ok[:0], 3))
