"""CPU tests of the fold-in boundary (K7, als_fold_in; no GPU, no compute launched).

* The header, the library and the ctypes table agree on the two entry points and ABI 9.
* als_fold_in's argument checks run host-side and return the documented codes (small
  integers stand in for pointers; nothing is dereferenced before the checks).
* filters.ragged_rows, the grouping of the new rows' ratings, on CPU tensors.
* The sharded engine carries fold_in / recommend_new and refuses them.
"""
import inspect
import re

import numpy as np
import pytest
import torch

from als_mi355x import _lib, filters
from test_abi import HEADER, _header_signatures, declared_functions

NAMES = ("als_fold_in", "als_fold_in_workspace_bytes")


def _call(**over):
    a = dict(row_ptr=16, col=16, val=16, n_rows=1, Y=16, n_src=10, ld=64, k=64, reg=0.1,
             implicit=0, alpha=1.0, yty=0, X=16, ld_out=64, n_used=16, status=16, ws=0,
             ws_bytes=0, stream=0)
    a.update(over)
    return _lib.lib().als_fold_in(*a.values())


def test_header_library_and_binding_agree():
    import ctypes
    raw = ctypes.CDLL(_lib.LIB_PATH)
    hdr = _header_signatures()
    for name in NAMES:
        assert name in declared_functions()
        assert hasattr(raw, name)
        assert hdr[name] == _lib.SIGNATURES[name][1]
    assert _lib.SIGNATURES["als_fold_in"][0] is ctypes.c_int
    assert _lib.SIGNATURES["als_fold_in_workspace_bytes"][0] is _lib.SZ
    assert _lib.ABI_VERSION == 9 == _lib.lib().als_abi_version()
    assert int(re.search(r"#define ALS_ABI_VERSION (\d+)", open(HEADER).read()).group(1)) == 9


@pytest.mark.parametrize("over,code", [
    (dict(k=0), -4), (dict(k=129, ld=132, ld_out=132), -4),
    (dict(ld=62), -1), (dict(ld_out=62), -1), (dict(ld=60), -1),
    (dict(row_ptr=0), -1), (dict(col=0), -1), (dict(val=0), -1), (dict(X=0), -1),
    (dict(status=0), -1), (dict(Y=0), -1),
    (dict(implicit=1), -1),            # implicit without yty_packed
    (dict(reg=-1.0), -1), (dict(alpha=-1.0), -1), (dict(n_rows=-1), -1), (dict(n_src=-1), -1),
    (dict(Y=20), -1), (dict(X=24), -1)])  # bases not 16-byte aligned
def test_argument_errors_before_any_device_call(over, code):
    L = _lib.lib()
    assert _call(**over) == code
    assert L.als_last_error()  # a message is set
    assert b"als_fold_in" in L.als_last_error()


def test_zero_rows_is_a_noop():
    assert _call(row_ptr=0, col=0, val=0, n_rows=0, Y=0, n_src=0, X=0, n_used=0, status=0) == 0
    assert _call(row_ptr=0, col=0, val=0, n_rows=0, Y=0, n_src=0, X=0, n_used=0, status=0,
                 implicit=1, yty=16, k=1, ld=4, ld_out=4) == 0


def test_workspace_size_is_monotone_and_may_be_zero():
    ws = _lib.lib().als_fold_in_workspace_bytes
    sizes = [[ws(n, k) for k in (1, 16, 64, 128)] for n in (0, 1, 1000, 10 ** 7)]
    for row in sizes:
        assert all(x >= 0 for x in row) and row == sorted(row)
    for c in zip(*sizes):
        assert list(c) == sorted(c)


def test_ragged_rows_groups_by_key_in_input_order():
    rng = np.random.default_rng(11)
    n = 400
    q = rng.choice([-5, 0, 3, 4, 70000, 2 ** 31 - 1], n).astype(np.int64)
    o = rng.integers(-1, 50, n)          # -1: an item the model does not know, kept
    v = rng.integers(1, 6, n).astype(np.float32)
    o[:4], q[:4] = 7, 3                  # duplicates are kept
    keys, row_ptr, col, val = filters.ragged_rows(torch.as_tensor(q).to(torch.int32),
                                                  torch.as_tensor(o), torch.as_tensor(v))
    assert row_ptr.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32
    assert keys.dtype == torch.int32
    keys, row_ptr, col, val = keys.numpy(), row_ptr.numpy(), col.numpy(), val.numpy()
    np.testing.assert_array_equal(keys, np.unique(q))       # ascending and distinct
    assert len(row_ptr) == len(keys) + 1 and row_ptr[0] == 0 and row_ptr[-1] == n
    for r, key in enumerate(keys):
        sel = q == key                                       # input order within the row
        np.testing.assert_array_equal(col[row_ptr[r]:row_ptr[r + 1]], o[sel])
        np.testing.assert_array_equal(val[row_ptr[r]:row_ptr[r + 1]], v[sel])
    assert (col == -1).sum() == (o == -1).sum() > 0
    r3 = list(keys).index(3)
    assert (col[row_ptr[r3]:row_ptr[r3 + 1]][:4] == 7).all()


def test_ragged_rows_empty_and_mismatched():
    e = torch.zeros(0, dtype=torch.int32)
    keys, row_ptr, col, val = filters.ragged_rows(e, e.long(), e.float())
    assert keys.numel() == 0 and row_ptr.tolist() == [0] and col.numel() == val.numel() == 0
    with pytest.raises(ValueError):
        filters.ragged_rows(torch.tensor([1, 2]), torch.tensor([1]), torch.tensor([1.0, 2.0]))


def test_sharded_engine_rejects_fold_in():
    from als_mi355x import distributed as D
    from als_mi355x.engine import ALSCore
    eng = D.ShardedALS.__new__(D.ShardedALS)  # no process group needed: both refuse at once
    with pytest.raises(NotImplementedError, match="sharded"):
        eng.fold_in([1], [2], [3.0], reg=0.1)
    with pytest.raises(NotImplementedError, match="sharded"):
        eng.recommend_new([1], [2], [3.0], 10, reg=0.1, candidates=[2])
    for name, kws in (("fold_in", ("reg", "implicit", "alpha", "user_side")),
                      ("recommend_new", ("reg", "implicit", "alpha", "user_side", "exclude_rated",
                                         "candidates"))):
        sharded = inspect.signature(getattr(D.ShardedALS, name))
        single = inspect.signature(getattr(ALSCore, name))
        assert list(sharded.parameters) == list(single.parameters)
        for kw in kws:
            assert sharded.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
            assert sharded.parameters[kw].default == single.parameters[kw].default
