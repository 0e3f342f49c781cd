"""Buffer contract of K18 (als_csr_remove_mark / als_csr_remove_compact) on guard-band memory
(guard_arena.py): the outputs and the scratch are carved to exactly the sizes include/als_hip.h
states and the inputs are put 16 bytes past a 256-byte boundary.  Run on an arena filled with
0x00 and on one filled with 0xFF: no guard byte may change, and the outputs must be the same
bits under both fills (nothing depends on memory the calls do not own) and equal the numpy
restatement (remove_ref.mark / compact), which test_remove_cpu.py holds to the oracle's
csr_build of the filtered ratings.
"""
import numpy as np
import pytest
import torch

import guard_arena as G
import many_rows_ref as MR
import remove_ref as RR
from als_mi355x import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"

# K18's size functions -> the tests that run the entry point on an exact-size carve
# (test_remove_cpu.py fails when the ABI gains an als_csr_remove_*_bytes without an entry here)
SCRATCH_CASES = {"als_csr_remove_scratch_bytes": ["test_csr_remove_all_guarded",
                                                  "test_csr_remove_plain_copy_guarded"]}


def _run(arena, inp, null_del=False):
    L = _lib.lib()
    T = L.als_csr_remove_tile()
    put = lambda x: None if x is None or len(x) == 0 else arena.put(torch.as_tensor(x),
                                                                    offset16=True)
    t = {k: put(v) for k, v in inp.items() if k != "n_cols_old"}
    n_old, nnz_old = len(inp["row_ptr_old"]) - 1, len(inp["col_old"])
    nnz_del = 0 if null_del else len(inp["col_del"])
    if null_del:
        t["row_ptr_del"] = t["col_del"] = None
    tiles = -(-nnz_old // T)
    keep_bits = arena.out((-(-nnz_old // 64),), torch.int64, name="keep_bits")
    tile_off = arena.out((tiles + 1,), torch.int64, name="tile_off")
    row_ptr_kept = arena.out((n_old + 1,), torch.int64, name="row_ptr_kept")
    hits = arena.out((nnz_del,), torch.int32, name="del_hits") if nnz_del else None
    need = L.als_csr_remove_scratch_bytes(nnz_old, n_old)
    scratch = arena.carve(need, name="scratch")
    p = lambda x: 0 if x is None else x.data_ptr()
    _lib.check(L.als_csr_remove_mark(p(t["row_ptr_old"]), p(t["col_old"]), nnz_old, n_old,
                                     p(t["row_ptr_del"]), p(t["col_del"]), nnz_del, p(keep_bits),
                                     p(tile_off), p(row_ptr_kept), p(hits), p(scratch), need,
                                     _lib.stream_ptr(DEV)), "als_csr_remove_mark")
    nnz_out = int(tile_off[-1])
    col = arena.out((nnz_out,), torch.int32, name="col_out")
    val = arena.out((nnz_out,), torch.float32, name="val_out")
    _lib.check(L.als_csr_remove_compact(p(t["col_old"]), p(t["val_old"]), nnz_old, p(keep_bits),
                                        p(tile_off), p(t["new_of_old_col"]), inp["n_cols_old"],
                                        p(col), p(val), nnz_out, _lib.stream_ptr(DEV)),
               "als_csr_remove_compact")
    torch.cuda.synchronize()
    outs = [keep_bits, tile_off, row_ptr_kept, col, val] + ([hits] if nnz_del else [])
    return [x.clone().cpu().numpy() for x in outs]


def _reference(inp, T, null_del=False):
    d = (None, None) if null_del else (inp["row_ptr_del"], inp["col_del"])
    keep_bits, tile_off, row_ptr_kept, hits = RR.mark(inp["row_ptr_old"], inp["col_old"], *d, T)
    col, val = RR.compact(inp["col_old"], inp["val_old"], keep_bits, inp["new_of_old_col"],
                          inp["n_cols_old"])
    return [keep_bits.view(np.int64), tile_off, row_ptr_kept, col, val] + (
        [hits] if len(hits) else [])


def _both_fills(inp, null_del=False):
    T = _lib.lib().als_csr_remove_tile()
    outs = []
    for fill in (0x00, 0xFF):
        arena = G.Arena(DEV, fill, capacity=48 << 20)
        outs.append(_run(arena, inp, null_del))
        bad = arena.check()
        assert not bad, (f"fill {fill:#04x}: bytes outside a buffer were written: "
                         f"{ {k: (v[:8], len(v)) for k, v in bad.items()} }")
    ref = _reference(inp, T, null_del)
    assert len(outs[0]) == len(ref)
    for a, b, r in zip(outs[0], outs[1], ref):
        assert a.tobytes() == b.tobytes(), "the output depends on the arena's fill"
        assert a.dtype == r.dtype and a.tobytes() == r.tobytes()
    return outs[0]


@pytest.mark.parametrize("user_side", [True, False])
@pytest.mark.parametrize("name", ["f_both_leave", "i_tile_edges", "a_one_pair"])
def test_csr_remove_all_guarded(name, user_side):
    T = _lib.lib().als_csr_remove_tile()
    old, spec = RR.case(name, T)
    inp, want = RR.side_inputs(old, RR.listed(old, spec), user_side)
    assert (inp["new_of_old_col"] is None) == (name == "a_one_pair")
    got = _both_fills(inp)
    assert RR.row_ptr_of(got[2], want["new_of_old_row"]).tobytes() == want["csr"][0].tobytes()
    assert got[3].tobytes() == want["csr"][1].tobytes()
    assert got[4].tobytes() == want["csr"][2].tobytes()


@pytest.mark.parametrize("user_side", [True, False])
def test_csr_remove_plain_copy_guarded(user_side):
    """(l) nothing listed, NULL delete list and NULL map: every bit set, row_ptr_kept ==
    row_ptr_old, the columns and values copied."""
    T = _lib.lib().als_csr_remove_tile()
    old, spec = RR.case("l_nothing_to_do", T)
    inp, _ = RR.side_inputs(old, RR.listed(old, spec), user_side)
    assert inp["new_of_old_col"] is None and len(inp["col_del"]) == 0
    got = _both_fills(inp, null_del=True)
    assert got[2].tobytes() == inp["row_ptr_old"].tobytes()
    assert got[3].tobytes() == inp["col_old"].tobytes()
    assert got[4].tobytes() == inp["val_old"].tobytes()
    nnz = len(inp["col_old"])
    bits = np.unpackbits(got[0].view(np.uint8), bitorder="little")
    assert bits[:nnz].all() and not bits[nnz:].any()


@pytest.mark.parametrize("user_side", [True, False])
@pytest.mark.parametrize("kind", ["every_5th", "seam_rows"])
def test_csr_remove_seams_guarded(kind, user_side):
    """many_rows_ref.seams: about 1100 rows, a tile that walks two batches of 256 rows with
    long rows on both sides of the seam; one entry of every 5th row leaves, or every entry of
    the rows on a seam."""
    T = _lib.lib().als_csr_remove_tile()
    old = MR.seams(T)
    inp, want = RR.side_inputs(old, MR.delete_pairs(old, kind, T), user_side)
    got = _both_fills(inp)
    assert RR.row_ptr_of(got[2], want["new_of_old_row"]).tobytes() == want["csr"][0].tobytes()
    assert got[3].tobytes() == want["csr"][1].tobytes()
    assert got[4].tobytes() == want["csr"][2].tobytes()
