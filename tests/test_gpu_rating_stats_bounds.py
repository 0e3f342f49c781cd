"""Buffer contracts of the K16 entry points (als_row_moments, als_bias_update,
als_baseline_predict) on guard-band memory (guard_arena.py): the moments table, the total, the
bias table, the predictions, the flags and the scratch are carved to exactly the sizes
include/als_hip.h states, and the inputs are put 16 bytes past a 256-byte boundary.  Run on an
arena filled with 0x00 and on one filled with 0xFF: no guard byte may change, and the results
must be the same bits under both fills (nothing depends on memory the call does not own) and
equal the numpy reference.
"""
import ctypes

import numpy as np
import pytest
import torch

import baseline_ref as BR
import guard_arena as G
from als_mi355x import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, U8 = torch.float32, torch.float64, torch.uint8

# K16's size functions -> the tests below that run their entry point on an exact-size carve
# (test_rating_stats_cpu.py fails when the ABI gains an als_rating_stats_*_bytes without an
# entry here)
SCRATCH_CASES = {
    "als_rating_stats_scratch_bytes": ["test_rating_stats_all_guarded"],
}


def _call(name, *args):
    conv = [(0 if a is None else a.data_ptr()) if (a is None or isinstance(a, torch.Tensor))
            else a for a in args]
    _lib.check(getattr(_lib.lib(), name)(*conv, _lib.stream_ptr(DEV)), name)


def _lengths(kind):
    T = _lib.lib().als_rating_stats_task()
    R = _lib.lib().als_rating_stats_group_rows()
    if kind == "one":
        return [1]
    if kind == "empty":
        return [0] * (R + 1)
    if kind == "edges":
        return [0, 1, T - 1, T, T + 1, 3 * T + 5, 2, 0]
    return [3 * T + 1] + [0] * 300 + [7] * (2 * R - 1)


def _run(arena, side, n_cols, other, offset, damping, urow, irow, mu, n_u, n_i):
    L = _lib.lib()
    row_ptr, col, val = side
    n_rows, nnz = len(row_ptr) - 1, len(val)
    put = lambda x: arena.put(torch.as_tensor(x), offset16=True)
    rp = put(row_ptr)
    c = put(col) if nnz else None
    v = put(val) if nnz else None
    o = put(other)
    mom, total = arena.out((n_rows, 5), F64), arena.out((5,), F64)
    w = arena.carve(L.als_rating_stats_scratch_bytes(nnz, n_rows), offset16=True, name="scratch")
    off = ctypes.c_double(offset)
    _call("als_row_moments", rp, c, v, nnz, n_rows, n_cols, o, ctypes.addressof(off), mom, total,
          w, w.numel())
    bias = arena.out((n_rows,), F64)
    damp = ctypes.c_double(damping)
    _call("als_bias_update", mom, n_rows, ctypes.addressof(damp), bias)
    ur, ir = put(urow), put(irow)
    pred, known = arena.out((len(urow),), F32), arena.out((len(urow),), U8)
    m = ctypes.c_double(mu)
    bu = bias if n_u == n_rows else None   # the fresh table serves as the user biases
    _call("als_baseline_predict", ur, ir, len(urow), ctypes.addressof(m), bu, n_u, o, n_i, pred,
          known)
    torch.cuda.synchronize()
    return {k: t.clone() for k, t in dict(mom=mom, total=total, bias=bias, pred=pred,
                                          known=known).items()}


@pytest.mark.parametrize("kind", ["one", "empty", "edges", "heavy"])
def test_rating_stats_all_guarded(kind):
    rng = np.random.default_rng(len(kind))
    lengths = _lengths(kind)
    n_cols = 37
    side = BR.csr_from_lengths(lengths, n_cols, rng, "half")
    if len(side[1]) > 3:
        side[1][[0, 2]] = [-1, n_cols]      # outside the table: no gather, no access
    other = rng.integers(-8, 9, n_cols) * 0.25   # exact sums: every bit is comparable
    offset, damping, mu = 0.5, 2.0, 3.25
    n_rows = len(lengths)
    urow = rng.integers(-1, n_rows + 1, 301).astype(np.int32)
    irow = rng.integers(-1, n_cols + 1, 301).astype(np.int32)
    outs = []
    for fill in (0x00, 0xFF):
        arena = G.Arena(DEV, fill, capacity=48 << 20)
        outs.append(_run(arena, side, n_cols, other, offset, damping, urow, irow, mu, n_rows,
                         n_cols))
        bad = arena.check()
        assert not bad, (f"fill {fill:#04x}: bytes outside a buffer were written: "
                         f"{ {k: (v[:8], len(v)) for k, v in bad.items()} }")
    for key in outs[0]:
        a, b = outs[0][key].cpu().numpy(), outs[1][key].cpu().numpy()
        assert a.tobytes() == b.tobytes(), f"'{key}' depends on the arena's fill"
    got = {k: v.cpu().numpy() for k, v in outs[0].items()}
    mom, total, _, q = BR.row_moments(*side, n_cols, other, offset)
    for f in (0, 1, 3, 4):
        np.testing.assert_array_equal(got["mom"][:, f], mom[:, f])
        np.testing.assert_array_equal(got["total"][f], total[f])
    assert (np.abs(got["mom"][:, 2] - mom[:, 2]) <= 4 * mom[:, 0] * BR.U53 * q[:-1]).all()
    assert abs(got["total"][2] - total[2]) <= 4 * total[0] * BR.U53 * q[-1]
    np.testing.assert_array_equal(got["bias"], BR.bias_update(mom, damping))
    pred, known = BR.predict_sized(urow, irow, mu, got["bias"], n_rows, other, n_cols)
    np.testing.assert_array_equal(got["pred"], pred)
    np.testing.assert_array_equal(got["known"], known)
