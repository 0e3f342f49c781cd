"""Buffer contract of K17 (als_csr_merge) on guard-band memory (guard_arena.py): the three
outputs are carved to exactly the sizes include/als_hip.h states and the inputs are put 16
bytes past a 256-byte boundary.  Run on an arena filled with 0x00 and on one filled with 0xFF:
no guard byte may change, and the outputs must be the same bits under both fills (nothing
depends on memory the call does not own) and equal the numpy restatement (update_ref.merge),
which test_update_cpu.py holds to the oracle's csr_build on the concatenation.
"""
import numpy as np
import pytest
import torch

import guard_arena as G
import many_rows_ref as MR
import update_ref as UR
from als_mi355x import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"

# K17's size functions -> the tests that run the entry point on an exact-size carve.  The call
# takes no scratch, so there is none (test_update_cpu.py fails when the ABI gains an
# als_csr_merge_*_bytes without an entry here).
SCRATCH_CASES = {}


def _run(arena, inp):
    L = _lib.lib()
    put = lambda x: None if x is None or len(x) == 0 else arena.put(torch.as_tensor(x),
                                                                    offset16=True)
    t = {k: put(v) for k, v in inp.items() if k != "n_cols_old"}
    n_old, n_new = len(inp["row_ptr_old"]) - 1, len(inp["row_ptr_add"]) - 1
    nnz_old, nnz_add = len(inp["col_old"]), len(inp["col_add"])
    row_ptr = arena.out((n_new + 1,), torch.int64, name="row_ptr_out")
    col = arena.out((nnz_old + nnz_add,), torch.int32, name="col_out")
    val = arena.out((nnz_old + nnz_add,), torch.float32, name="val_out")
    p = lambda x: 0 if x is None else x.data_ptr()
    _lib.check(L.als_csr_merge(p(t["row_ptr_old"]), p(t["col_old"]), p(t["val_old"]), nnz_old,
                               n_old, inp["n_cols_old"], p(t["new_of_old_row"]),
                               p(t["new_of_old_col"]), p(t["row_ptr_add"]), p(t["col_add"]),
                               p(t["val_add"]), nnz_add, n_new, p(row_ptr), p(col), p(val),
                               _lib.stream_ptr(DEV)), "als_csr_merge")
    torch.cuda.synchronize()
    return [x.clone().cpu().numpy() for x in (row_ptr, col, val)]


# (b) new ids on both sides, on one side only (the other map NULL), (e) the tile edges and (f)
# a batch of one (both maps NULL)
@pytest.mark.parametrize("user_side", [True, False])
@pytest.mark.parametrize("name", ["b_new_both", "b_new_users", "e_tile_edges", "f_one"])
def test_csr_merge_all_guarded(name, user_side):
    T = _lib.lib().als_csr_merge_tile()
    inp, want = UR.side_inputs(*UR.case(name, T), user_side)
    null_row = name in ("e_tile_edges", "f_one") or (name == "b_new_users" and not user_side)
    null_col = name in ("e_tile_edges", "f_one") or (name == "b_new_users" and user_side)
    assert (inp["new_of_old_row"] is None) == null_row
    assert (inp["new_of_old_col"] is None) == null_col
    outs = []
    for fill in (0x00, 0xFF):
        arena = G.Arena(DEV, fill, capacity=48 << 20)
        outs.append(_run(arena, inp))
        bad = arena.check()
        assert not bad, (f"fill {fill:#04x}: bytes outside a buffer were written: "
                         f"{ {k: (v[:8], len(v)) for k, v in bad.items()} }")
    ref = UR.merge(inp["row_ptr_old"], inp["col_old"], inp["val_old"], inp["new_of_old_row"],
                   inp["new_of_old_col"], inp["row_ptr_add"], inp["col_add"], inp["val_add"])
    for a, b, r, w in zip(outs[0], outs[1], ref, want):
        assert a.tobytes() == b.tobytes(), "the output depends on the arena's fill"
        assert a.dtype == r.dtype and a.tobytes() == r.tobytes()
        assert a.tobytes() == w.tobytes()


def test_csr_merge_empty_rows_and_empty_sides_guarded():
    """Rows without a rating cannot come from K1, but the entry point takes them: empty rows
    before, between and after the others, an empty batch (a plain copy) and an empty old side."""
    T = _lib.lib().als_csr_merge_tile()
    rng = np.random.default_rng(3)

    def csr(lens, n_cols):
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        return (ptr, rng.integers(0, n_cols, ptr[-1]).astype(np.int32),
                rng.integers(1, 11, ptr[-1]).astype(np.float32))

    old = csr([0, 0, T + 1, 0, 3] + [0] * 300 + [T - 1, 0], 9)
    n_old = len(old[0]) - 1
    row_map = (np.arange(n_old) * 2 + 1).astype(np.int32)        # a new row around every old one
    n_new = 2 * n_old + 1
    col_map = (np.arange(9) + 2).astype(np.int32)
    lens_add = np.zeros(n_new, np.int64)
    lens_add[[0, 5, 6, 2 * n_old]] = [2, 1, T, 4]
    for add, rmap, cmap, n in ((csr(lens_add, 11), row_map, col_map, n_new),
                               (csr(np.zeros(n_old, np.int64), 9), None, None, n_old)):
        inp = dict(row_ptr_old=old[0], col_old=old[1], val_old=old[2], n_cols_old=9,
                   new_of_old_row=rmap, new_of_old_col=cmap, row_ptr_add=add[0], col_add=add[1],
                   val_add=add[2])
        ref = UR.merge(old[0], old[1], old[2], rmap, cmap, *add)
        for fill in (0x00, 0xFF):
            arena = G.Arena(DEV, fill, capacity=48 << 20)
            got = _run(arena, inp)
            assert arena.check() == {}
            for a, r in zip(got, ref):
                assert a.tobytes() == r.tobytes()
    add = csr([2, 0, 5], 4)
    empty = (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    inp = dict(row_ptr_old=empty[0], col_old=empty[1], val_old=empty[2], n_cols_old=0,
               new_of_old_row=None, new_of_old_col=None, row_ptr_add=add[0], col_add=add[1],
               val_add=add[2])
    arena = G.Arena(DEV, 0xFF, capacity=16 << 20)
    got = _run(arena, inp)
    assert arena.check() == {}
    for a, r in zip(got, add):
        assert a.tobytes() == r.tobytes()


@pytest.mark.parametrize("user_side", [True, False])
@pytest.mark.parametrize("kind", ["b_new_rows", "c_new_cols"])
def test_csr_merge_seams_guarded(kind, user_side):
    """many_rows_ref.seams: about 1100 rows, a tile that walks two batches of 256 rows with
    long rows on both sides of the seam; new rows in every gap (a row map of 1100 entries, the
    row pointer over several workgroups) or new columns."""
    T = _lib.lib().als_csr_merge_tile()
    old = MR.seams(T)
    inp, want = UR.side_inputs(old, MR.batch(old, kind), user_side)
    assert (inp["new_of_old_row"] is None) == ((kind == "c_new_cols") == user_side)
    outs = []
    for fill in (0x00, 0xFF):
        arena = G.Arena(DEV, fill, capacity=48 << 20)
        outs.append(_run(arena, inp))
        bad = arena.check()
        assert not bad, (f"fill {fill:#04x}: bytes outside a buffer were written: "
                         f"{ {k: (v[:8], len(v)) for k, v in bad.items()} }")
    ref = UR.merge(inp["row_ptr_old"], inp["col_old"], inp["val_old"], inp["new_of_old_row"],
                   inp["new_of_old_col"], inp["row_ptr_add"], inp["col_add"], inp["val_add"])
    for a, b, r, w in zip(outs[0], outs[1], ref, want):
        assert a.tobytes() == b.tobytes(), "the output depends on the arena's fill"
        assert a.dtype == r.dtype and a.tobytes() == r.tobytes()
        assert a.tobytes() == w.tobytes()
