"""CPU tests of the neighbour search boundary (K12, als_similar; no GPU, nothing launched).

* The fp64 reference (similar_ref.py) on a 6 x 3 case worked by hand: a duplicate row, a
  zero row, self-exclusion, the -1 / -inf padding.
* The header, the library and the ctypes table agree on the entry points, ABI still 9.
* Argument errors: ValueError from the binding before anything touches the device, and the
  documented codes from the C entry points (small integers stand in for pointers).
* Unknown ids are dropped before any kernel is reached.
* The sharded engine carries similar / similar_all and refuses them.
"""
import inspect
import re

import numpy as np
import pytest
import torch

import similar_ref as R
from als_mi355x import _lib, engine as E, filters
from test_abi import HEADER, _header_signatures, declared_functions

NAMES = ("als_similar", "als_similar_workspace_bytes", "als_similar_unit_rows")

# rows: 0 = e1, 1 = e1 again (a duplicate of 0), 2 = (1, 1, 0), 3 = zero, 4 = -e1, 5 = e2 x 2
T6 = np.array([[1, 0, 0], [1, 0, 0], [1, 1, 0], [0, 0, 0], [-1, 0, 0], [0, 2, 0]], np.float64)


def test_reference_cosine_by_hand():
    S = R.cosine(T6, T6)
    h = np.sqrt(0.5)
    want0 = [1, 1, h, np.nan, -1, 0]
    np.testing.assert_allclose(S[0], want0, atol=1e-15)
    np.testing.assert_allclose(S[5], [0, 0, h, np.nan, 0, 1], atol=1e-15)
    assert np.isnan(S[3]).all() and np.isnan(S[:, 3]).all()   # the zero row, both ways
    np.testing.assert_array_equal(R.has_direction(T6), [1, 1, 1, 0, 1, 1])


def test_reference_neighbours_by_hand():
    S = R.cosine(T6, T6)
    adm = R.admissible(T6, T6, self_rows=np.arange(6))
    assert not adm[np.arange(6), np.arange(6)].any() and not adm[:, 3].any() and not adm[3].any()
    idx, sc = R.neighbours(S, adm, 5)
    # query 0: its duplicate (row 1) at 1, then (1,1,0), then e2 at 0, then -e1; one slot open
    np.testing.assert_array_equal(idx[0], [1, 2, 5, 4, -1])
    np.testing.assert_allclose(sc[0], [1, np.sqrt(0.5), 0, -1, -np.inf])
    # query 5 (e2): (1,1,0) first, then the three orthogonal rows by ascending index
    np.testing.assert_array_equal(idx[5], [2, 0, 1, 4, -1])
    # the zero query lists nothing
    assert (idx[3] == -1).all() and np.isneginf(sc[3]).all()
    # without self-exclusion a query equal to a table row lists the LOWER index first
    idx2, sc2 = R.neighbours(S, R.admissible(T6, T6), 2)
    np.testing.assert_array_equal(idx2[1], [0, 1])
    np.testing.assert_allclose(sc2[1], [1, 1])
    # an allow mask, and top beyond the table: padding
    allow = np.array([0, 1, 0, 1, 0, 1], bool)
    idx3, sc3 = R.neighbours(S, R.admissible(T6, T6, np.arange(6), allow), 8)
    np.testing.assert_array_equal(idx3[0], [1, 5] + [-1] * 6)
    assert idx3.shape == sc3.shape == (6, 8)
    R.check(idx3, sc3.astype(np.float32), S, R.admissible(T6, T6, np.arange(6), allow), 8)


def test_reference_checker_rejects_wrong_lists():
    S = R.cosine(T6, T6)
    adm = R.admissible(T6, T6, self_rows=np.arange(6))
    idx, sc = R.neighbours(S, adm, 3)
    bad = idx.copy()
    bad[0, 0] = 0                       # the query's own row
    with pytest.raises(AssertionError):
        R.check(bad, sc, S, adm, 3)
    bad = idx.copy()
    bad[0, [1, 2]] = bad[0, [2, 1]]     # swapped where the scores do not tie
    with pytest.raises(AssertionError):
        R.check(bad, sc, S, adm, 3)
    # a swap inside the exact tie (rows 0 and 1 for query 5) is within the rule
    idx5, sc5 = R.neighbours(S, adm, 4)
    ok = idx5.copy()
    ok[5, [1, 2]] = ok[5, [2, 1]]
    R.check(ok, sc5, S, adm, 4)


def test_header_library_and_binding_agree():
    import ctypes
    raw = ctypes.CDLL(_lib.LIB_PATH)
    hdr = _header_signatures()
    for name in NAMES:
        assert name in declared_functions()
        assert hasattr(raw, name)
        assert hdr[name] == _lib.SIGNATURES[name][1]
    assert _lib.SIGNATURES["als_similar"][0] is ctypes.c_int
    assert _lib.SIGNATURES["als_similar_workspace_bytes"][0] is _lib.SZ
    assert _lib.ABI_VERSION == 9 == _lib.lib().als_abi_version()
    assert int(re.search(r"#define ALS_ABI_VERSION (\d+)", open(HEADER).read()).group(1)) == 9


def _call(**over):
    a = dict(T=16, n=100, ld=64, k=64, Q=16, n_q=1, ldq=64, self_rows=0, allow=0, top=10,
             slices=1, idx=16, score=16, ws=16, ws_bytes=1 << 30, stream=0)
    a.update(over)
    return _lib.lib().als_similar(*a.values())


@pytest.mark.parametrize("over,code", [
    (dict(k=0), -4), (dict(k=129, ld=132, ldq=132), -4), (dict(top=0), -4), (dict(top=257), -4),
    (dict(ld=62), -1), (dict(ldq=60), -1), (dict(n=-1), -1), (dict(n_q=-1), -1),
    (dict(slices=-1), -1), (dict(slices=4097), -1),
    (dict(T=0), -1), (dict(Q=0), -1), (dict(idx=0), -1), (dict(score=0), -1),
    (dict(T=20), -1), (dict(Q=24), -1), (dict(ws=24), -1),
    (dict(ws=0), -2), (dict(ws_bytes=8), -2)])
def test_c_argument_errors_before_any_device_call(over, code):
    L = _lib.lib()
    assert _call(**over) == code
    assert b"als_similar" in L.als_last_error()


def test_zero_queries_is_a_noop_and_workspace_sizes():
    assert _call(n_q=0, T=0, Q=0, idx=0, score=0, ws=0, ws_bytes=0) == 0
    ws = _lib.lib().als_similar_workspace_bytes
    assert ws(1000, 1, 10, 3) == 16 * 3 * 10 * 8          # 16 queries x slices x top keys
    assert ws(1000, 16, 10, 3) == ws(1000, 1, 10, 3)
    assert ws(10 ** 6, 16, 256, 128) >= 16 * 128 * 256 * 8  # plus the second merge stage
    assert ws(1000, 1, 0, 1) == ws(1000, 1, 257, 1) == ws(1000, 1, 10, -1) == 0
    assert 0 < ws(5, 1, 10, 0) <= ws(10 ** 6, 1, 10, 0)   # auto slices grow with the table
    unit = _lib.lib().als_similar_unit_rows
    assert unit(16, 10, 64, 129, 16, 0, 0, 0) == -4 and unit(16, 10, 62, 60, 16, 0, 0, 0) == -1
    assert unit(0, 10, 64, 64, 16, 0, 0, 0) == -1 and unit(16, 10, 64, 64, 20, 0, 0, 0) == -1
    assert unit(0, 0, 64, 64, 0, 0, 0, 0) == 0


@pytest.mark.parametrize("kw", [dict(top=0), dict(top=257), dict(rank=129), dict(slices=-1)])
def test_binding_argument_errors_raise_value_error(kw):
    a = dict(rank=8, top=5, slices=0)
    a.update(kw)
    T = torch.zeros((6, E.ld_for(8)))
    with pytest.raises(ValueError):
        E.similar_rows(T[:2], 2, T, 6, a["rank"], a["top"], None, None, a["slices"])
    if "top" in kw:
        with pytest.raises(ValueError):
            E.similar_rows_unit(None, T, 6, 8, kw["top"])


def _cpu_core(n_items=5, gap=3):
    """An ALSCore shell on CPU tensors: enough for the id handling, which runs before any
    kernel."""
    core = E.ALSCore.__new__(E.ALSCore)
    core.device = torch.device("cpu")
    core.rank = 4
    ids = torch.arange(n_items, dtype=torch.int32) * gap
    mp = torch.full((int(ids.max()) + 1,), -1, dtype=torch.int32)
    mp[ids.long()] = torch.arange(n_items, dtype=torch.int32)
    core.iidx = E.IdIndex(mp, ids, n_items, 0)
    core.uidx = E.IdIndex(mp.clone(), ids.clone(), n_items, 0)
    core.U = torch.zeros((n_items, 4))
    core.V = torch.zeros((n_items, 4))
    return core


def test_unknown_ids_are_dropped_before_any_kernel():
    core = _cpu_core()
    for user_side in (False, True):
        keys, ids, sc = core.similar([1, 2, 100, -7], 3, user_side)
        assert keys.numel() == 0 and tuple(ids.shape) == tuple(sc.shape) == (0, 3)
    keys, ids, sc = core.similar([1, 2], 10)               # t = min(top, n - 1)
    assert tuple(ids.shape) == (0, 4)
    for bad in (0, 257):
        with pytest.raises(ValueError):
            core.similar([3], bad)
        with pytest.raises(ValueError):
            core.similar_all(bad)
    one = _cpu_core(n_items=1)                             # a table of one row: t = 0
    keys, ids, sc = one.similar([0], 5)
    assert keys.tolist() == [0] and tuple(ids.shape) == (1, 0)
    keys, ids, sc = one.similar_all(5)
    assert keys.tolist() == [0] and tuple(sc.shape) == (1, 0)
    bare = E.ALSCore.__new__(E.ALSCore)
    bare.U = bare.V = None
    with pytest.raises(ValueError, match="factors"):
        bare.similar([1], 3)


def test_sharded_engine_rejects_similar(monkeypatch):
    import torch.distributed as dist
    from als_mi355x import distributed as D
    assert D.reject_sharded_similar is filters.reject_sharded_similar
    assert "reject_sharded_similar" in filters.__all__
    # what a rank of a world of size > 1 holds is the sharded engine (engine.make_engine)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 4)
    made = {}
    monkeypatch.setattr(D.ShardedALS, "__init__", lambda self, *a, **k: made.update(s=1))
    eng = E.make_engine([1], [2], [3.0])
    assert isinstance(eng, D.ShardedALS) and made
    with pytest.raises(NotImplementedError, match="sharded"):
        eng.similar([1], 10)
    with pytest.raises(NotImplementedError, match="sharded"):
        eng.similar_all(10, True, candidates=[2])
    for name in ("similar", "similar_all"):
        sharded = inspect.signature(getattr(D.ShardedALS, name))
        single = inspect.signature(getattr(E.ALSCore, name))
        assert list(sharded.parameters) == list(single.parameters)
        assert sharded.parameters["candidates"].kind is inspect.Parameter.KEYWORD_ONLY
        for p in sharded.parameters:
            assert sharded.parameters[p].default == single.parameters[p].default
