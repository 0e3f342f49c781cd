"""Buffer contract of K20 (als_split_anchor / als_split_eligible / als_split_thresholds /
als_split_mark) on guard-band memory (guard_arena.py): the outputs and the scratch are carved
to exactly the sizes include/als_hip.h states and the inputs are put 16 bytes past a 256-byte
boundary.  Run on an arena filled with 0x00 and on one filled with 0xFF: no guard byte may
change, and the outputs must be the same bits under both fills (nothing depends on memory the
calls do not own, the uninitialised scratch included) and equal the numpy restatement
(split_ref.py, which test_split_cpu.py holds to the rule's properties).
"""
import numpy as np
import pytest
import torch

import guard_arena as G
import many_rows_ref as MR
from als_mi355x import _lib
from test_gpu_split import CAP, SEED, WINDOWS, _expected, _ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

# K20's size functions -> the tests that run the entry points on an exact-size carve
# (test_split_cpu.py fails when the ABI gains an als_split_*_bytes without an entry here)
SCRATCH_CASES = {"als_split_scratch_bytes": ["test_split_all_guarded"]}


def _run(arena, sp, row_cap):
    L = _lib.lib()
    T = L.als_csr_remove_tile()
    put = lambda x: arena.put(torch.as_tensor(np.ascontiguousarray(x)), offset16=True)
    st = _lib.stream_ptr(DEV)
    p = lambda x: 0 if x is None else x.data_ptr()
    sides = {}
    for user_rows in (True, False):
        row_ptr, col, _, n_rows, n_cols, row_ids, col_ids = sp.side(user_rows)
        t = [put(row_ptr), put(col), put(row_ids), put(col_ids)]
        sides[user_rows] = dict(t=t, args=[p(t[0]), p(t[1]), len(col), n_rows, n_cols, p(t[2]),
                                           p(t[3]), int(user_rows), SEED],
                                need=L.als_split_scratch_bytes(len(col), n_rows))
    sel, oth = sides[sp.user_side], sides[not sp.user_side]
    out = {}
    anchor = None
    if sp.anchor is not None:
        anchor = arena.out((oth["args"][3],), torch.int32, name="anchor")
        scratch = arena.carve(oth["need"], name="anchor_scratch")
        _lib.check(L.als_split_anchor(*oth["args"], p(anchor), p(scratch), oth["need"], st),
                   "als_split_anchor")
        out["anchor"] = anchor
    n_sel = sel["args"][3]
    out["eligible"] = arena.out((n_sel,), torch.int32, name="eligible")
    _lib.check(L.als_split_eligible(*sel["args"][:5], p(anchor), p(out["eligible"]), st),
               "als_split_eligible")
    win = [put(sp.lo), put(sp.hi)]
    for k, dt in (("lo_key", torch.int64), ("lo_col", torch.int32), ("hi_key", torch.int64),
                  ("hi_col", torch.int32)):
        out[k] = arena.out((n_sel,), dt, name=k)
    thr = [p(out[k]) for k in ("lo_key", "lo_col", "hi_key", "hi_col")]
    scratch = arena.carve(sel["need"], name="thr_scratch")
    _lib.check(L.als_split_thresholds(*sel["args"], p(anchor), p(win[0]), p(win[1]), row_cap,
                                      *thr, p(scratch), sel["need"], st), "als_split_thresholds")
    for user_rows in (True, False):
        s = sides[user_rows]
        nnz, n_rows = s["args"][2], s["args"][3]
        tiles = -(-nnz // T)
        kb = arena.out((-(-nnz // 64),), torch.int64, name=f"keep_bits{user_rows:d}")
        to = arena.out((tiles + 1,), torch.int64, name=f"tile_off{user_rows:d}")
        rk = arena.out((n_rows + 1,), torch.int64, name=f"row_ptr_kept{user_rows:d}")
        scratch = arena.carve(s["need"], name=f"mark_scratch{user_rows:d}")
        _lib.check(L.als_split_mark(*s["args"], int(user_rows == sp.user_side), *thr, p(anchor),
                                    p(kb), p(to), p(rk), p(scratch), s["need"], st),
                   "als_split_mark")
        out.update({f"keep_bits{user_rows:d}": kb, f"tile_off{user_rows:d}": to,
                    f"row_ptr_kept{user_rows:d}": rk})
    torch.cuda.synchronize()
    return {k: v.clone().cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("row_cap", [CAP, 0])
@pytest.mark.parametrize("user_side", [True, False])
@pytest.mark.parametrize("shape,window", [("edges", dict(mode="fold", value=(1, 3))),
                                          ("edges", dict(mode="count", value=3)),
                                          ("nnz+1", dict(mode="fraction", value=0.2))])
def test_split_all_guarded(shape, window, user_side, row_cap):
    sp = _ref(shape, user_side, True)
    sp.set_windows(window["mode"], window["value"])
    outs = []
    for fill in (0x00, 0xFF):
        arena = G.Arena(DEV, fill)   # some 25 carves, 2 MiB of guard each
        outs.append(_run(arena, sp, row_cap))
        bad = arena.check()
        assert not bad, (f"fill {fill:#04x}: bytes outside a buffer were written: "
                         f"{ {k: (v[:8], len(v)) for k, v in bad.items()} }")
    want = _expected(sp)
    assert sorted(outs[0]) == sorted(want)
    for k in want:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), f"{k} depends on the arena's fill"
        assert outs[0][k].dtype == want[k].dtype and outs[0][k].tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("window", ["fold1of3", "last"])
def test_split_many_listed_guarded(window):
    """many_rows_ref.many_listed at row_cap = 1: every one of the 2 * 2048 + 37 selecting rows
    is listed, so the list fills its part of the scratch and a workgroup of the long-row
    kernel takes two or three rows."""
    sp = MR.FastSplit(seed=SEED, keep_items=True, user_side=True, **MR.many_listed())
    w = WINDOWS[window]
    sp.set_windows(w.get("mode"), w.get("value"), w.get("min_keep", 1), w.get("win"))
    outs = []
    for fill in (0x00, 0xFF):
        arena = G.Arena(DEV, fill)
        outs.append(_run(arena, sp, 1))
        bad = arena.check()
        assert not bad, (f"fill {fill:#04x}: bytes outside a buffer were written: "
                         f"{ {k: (v[:8], len(v)) for k, v in bad.items()} }")
    want = _expected(sp)
    assert sorted(outs[0]) == sorted(want)
    for k in want:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), f"{k} depends on the arena's fill"
        assert outs[0][k].dtype == want[k].dtype and outs[0][k].tobytes() == want[k].tobytes(), k
