"""CPU tests of the filtered top-k boundary (no GPU, no compute launched).

* als_topk_filtered's argument checks run host-side and return the documented codes
  (small integers stand in for pointers; nothing is dereferenced before the checks).
* The host helpers that build its inputs (filters.py) against numpy, on CPU tensors.
* The sharded engine refuses the two keywords without needing a process group.
"""
import numpy as np
import pytest
import torch

from als_mi355x import _lib, filters


def _call(Q=1, n_q=1, V=1, n_v=1, ld=64, k=64, top=10, eb=0, ee=0, ec=0, allow=0, idx=1, sc=1,
          ws=0, ws_bytes=0, stream=0):
    return _lib.lib().als_topk_filtered(Q, n_q, V, n_v, ld, k, top, eb, ee, ec, allow, idx, sc, ws,
                                        ws_bytes, stream)


@pytest.mark.parametrize("ex", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)])
def test_mismatched_exclusion_pointers(ex):
    assert _call(eb=ex[0], ee=ex[1], ec=ex[2]) == -1
    assert b"ex_begin" in _lib.lib().als_last_error()


@pytest.mark.parametrize("ex,allow", [((0, 0, 0), 0), ((1, 1, 1), 0), ((0, 0, 0), 1), ((1, 1, 1), 1)])
def test_same_codes_as_als_topk(ex, allow):
    f = dict(eb=ex[0], ee=ex[1], ec=ex[2], allow=allow)
    assert _call(k=129, ld=132, **f) == -4          # rank > 128
    assert _call(top=0, **f) == -4
    assert _call(top=257, **f) == -4
    assert _call(ld=60, **f) == -1                  # ld < k
    assert _call(**f) == -2                         # missing workspace
    assert _call(k=128, ld=128, top=256, **f) == -2
    assert _call(ws=8, ws_bytes=1 << 20, **f) == -1  # workspace not 16-byte aligned
    assert _call(Q=0, n_q=0, V=0, n_v=0, ld=4, k=4, top=1, idx=0, sc=0, **f) == 0  # n_q = 0
    assert _lib.lib().als_last_error()


def _bits_ref(rows, n_v):
    w = np.zeros(max((n_v + 31) // 32, 1), np.uint32)
    for j in rows:
        if 0 <= j < n_v:
            w[j >> 5] |= np.uint32(1) << np.uint32(j & 31)
    return w


@pytest.mark.parametrize("n_v,rows", [
    (70, [0, 31, 32, 63, 64, 69]),            # both sides of every word boundary, last row
    (64, [31, 31, 63, 63, 5]),                # duplicates; bit 31 (the int32 sign bit)
    (33, [-1, 40, 33, 32, -7, 2 ** 31 - 1]),  # unknown (-1) and out-of-range rows dropped
    (1, []), (0, []), (32, list(range(32))), (1000, list(range(0, 1000, 3)))])
def test_pack_allow_bits(n_v, rows):
    got = filters.pack_allow_bits(torch.tensor(rows, dtype=torch.int64), n_v)
    assert got.dtype == torch.int32
    np.testing.assert_array_equal(got.numpy().view(np.uint32), _bits_ref(rows, n_v))
    got32 = filters.pack_allow_bits(torch.tensor(rows, dtype=torch.int64).to(torch.int32)
                                    if all(abs(r) < 2 ** 31 for r in rows) else
                                    torch.tensor(rows, dtype=torch.int64), n_v)
    np.testing.assert_array_equal(got32.numpy(), got.numpy())


def test_exclusion_lists_against_numpy():
    rng = np.random.default_rng(3)
    n_q, n_v = 37, 50
    q = rng.integers(-1, n_q, 600)          # -1: unknown query id
    o = rng.integers(-1, n_v, 600)          # -1: unknown id of the other side
    q[:5], o[:5] = 7, 11                    # duplicates are kept
    q[q == 20] = 21                         # an empty row among non-empty ones
    beg, end, col = filters.exclusion_lists(torch.as_tensor(q), torch.as_tensor(o), n_q)
    assert beg.dtype == end.dtype == torch.int64 and col.dtype == torch.int32
    assert beg.shape == end.shape == (n_q,)
    beg, end, col = beg.numpy(), end.numpy(), col.numpy()
    for r in range(n_q):
        want = np.sort(o[(q == r) & (o >= 0)])
        np.testing.assert_array_equal(col[beg[r]:end[r]], want)
    assert end[20] == beg[20]
    assert (col[beg[7]:end[7]] == 11).sum() >= 5
    assert int((end - beg).sum()) == int(((q >= 0) & (o >= 0)).sum())


def test_exclusion_lists_empty_and_mismatched():
    beg, end, col = filters.exclusion_lists(torch.tensor([-1, -1]), torch.tensor([3, 4]), 4)
    assert beg.tolist() == end.tolist() == [0, 0, 0, 0]
    assert col.numel() >= 1          # never a null ex_col beside non-null ranges
    with pytest.raises(ValueError):
        filters.exclusion_lists(torch.tensor([1]), torch.tensor([1, 2]), 4)


def test_sharded_engine_rejects_the_filters():
    from als_mi355x import distributed as D
    assert D.reject_sharded_filters is filters.reject_sharded_filters
    assert filters.reject_sharded_filters(None, None) is None
    for kw in (dict(exclude="train", candidates=None), dict(exclude=None, candidates=[1, 2]),
               dict(exclude=([1], [2]), candidates=[3])):
        with pytest.raises(NotImplementedError, match="sharded"):
            filters.reject_sharded_filters(**kw)
    import inspect
    for name in ("recommend_all", "recommend_subset"):
        sig = inspect.signature(getattr(D.ShardedALS, name))
        for kw in ("exclude", "candidates"):
            assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
            assert sig.parameters[kw].default is None
