"""K20: per-user holdout and stratified folds (csrc/split.hip: als_split_anchor,
als_split_eligible, als_split_thresholds, als_split_mark), plus the torch-side window
arithmetic.  The contract is in include/als_hip.h."""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr
from .csr import keep_outputs
from .workspace import Workspace

SPLIT_MODES = ("count", "fraction", "fold")


def split_row_cap() -> int:
    """Longest row als_split_thresholds ranks in LDS (longer rows take the radix select)."""
    return int(_lib.lib().als_split_row_cap())


def split_seed(seed: int) -> int:
    """The 64 bits of `seed` as the int64 the ABI carries (the kernels read them as uint64)."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s - (1 << 64) if s >= (1 << 63) else s


def _side_args(row_ptr, col, n_cols, row_ids, col_ids, rows_are_users, seed):
    return (ptr(row_ptr), ptr(col), int(col.numel()), int(row_ptr.numel()) - 1, int(n_cols),
            ptr(row_ids), ptr(col_ids), int(bool(rows_are_users)), split_seed(seed))


def _scratch(ws: Workspace, nnz: int, n_rows: int):
    return ws.get(_lib.lib().als_split_scratch_bytes(int(nnz), int(n_rows)))


def split_anchor(row_ptr, col, n_cols: int, row_ids, col_ids, rows_are_users: bool, seed: int,
                 ws: Workspace):
    """als_split_anchor on one side: int32 [n_rows], the column of each row's smallest
    (key, column), -1 for an empty row."""
    dev = row_ptr.device
    n_rows = int(row_ptr.numel()) - 1
    anchor = torch.empty(n_rows, dtype=torch.int32, device=dev)
    w = _scratch(ws, col.numel(), n_rows)
    check(_lib.lib().als_split_anchor(*_side_args(row_ptr, col, n_cols, row_ids, col_ids,
                                                  rows_are_users, seed), ptr(anchor), ptr(w),
                                      w.numel(), stream_ptr(dev)), "als_split_anchor")
    return anchor


def split_eligible(row_ptr, col, n_cols: int, anchor):
    """als_split_eligible: int32 [n_rows], each row's entries that are no anchor (anchor: int32
    [n_cols] of the other side, None = every entry is eligible)."""
    dev = row_ptr.device
    n_rows = int(row_ptr.numel()) - 1
    out = torch.empty(n_rows, dtype=torch.int32, device=dev)
    check(_lib.lib().als_split_eligible(ptr(row_ptr), ptr(col), int(col.numel()), n_rows,
                                        int(n_cols), ptr(anchor), ptr(out), stream_ptr(dev)),
          "als_split_eligible")
    return out


def split_thresholds(row_ptr, col, n_cols: int, row_ids, col_ids, rows_are_users: bool,
                     seed: int, anchor, win_lo, win_hi, ws: Workspace, row_cap: int = 0):
    """als_split_thresholds on the selecting side: (lo_key int64 [n_rows] holding the uint64
    bits, lo_col int32, hi_key, hi_col)."""
    dev = row_ptr.device
    n_rows = int(row_ptr.numel()) - 1
    keys = [torch.empty(n_rows, dtype=torch.int64, device=dev) for _ in range(2)]
    cols = [torch.empty(n_rows, dtype=torch.int32, device=dev) for _ in range(2)]
    w = _scratch(ws, col.numel(), n_rows)
    check(_lib.lib().als_split_thresholds(
        *_side_args(row_ptr, col, n_cols, row_ids, col_ids, rows_are_users, seed), ptr(anchor),
        ptr(win_lo), ptr(win_hi), int(row_cap), ptr(keys[0]), ptr(cols[0]), ptr(keys[1]),
        ptr(cols[1]), ptr(w), w.numel(), stream_ptr(dev)), "als_split_thresholds")
    return keys[0], cols[0], keys[1], cols[1]


def split_mark(row_ptr, col, n_cols: int, row_ids, col_ids, rows_are_users: bool, seed: int,
               selecting: bool, thr, anchor, ws: Workspace):
    """als_split_mark on either side: (keep_bits, tile_off, row_ptr_kept) in remove_mark's
    format.  thr: split_thresholds' four arrays (of the selecting side)."""
    dev = row_ptr.device
    n_rows, nnz = int(row_ptr.numel()) - 1, int(col.numel())
    keep_bits, tile_off, row_ptr_kept = keep_outputs(nnz, n_rows, dev)
    w = _scratch(ws, nnz, n_rows)
    check(_lib.lib().als_split_mark(
        *_side_args(row_ptr, col, n_cols, row_ids, col_ids, rows_are_users, seed),
        int(bool(selecting)), ptr(thr[0]), ptr(thr[1]), ptr(thr[2]), ptr(thr[3]), ptr(anchor),
        ptr(keep_bits), ptr(tile_off), ptr(row_ptr_kept), ptr(w), w.numel(), stream_ptr(dev)),
        "als_split_mark")
    return keep_bits, tile_off, row_ptr_kept


def check_split_args(count=None, fraction=None, fold=None, min_keep=1):
    """Exactly one of count / fraction / fold=(f, F); returns (mode, value)."""
    given = [(m, v) for m, v in zip(SPLIT_MODES, (count, fraction, fold)) if v is not None]
    if len(given) != 1:
        raise ValueError("give exactly one of count=, fraction= and fold=(f, F)")
    mode, v = given[0]
    if int(min_keep) < 0:
        raise ValueError(f"min_keep must be >= 0, got {min_keep}")
    if mode == "count":
        if int(v) != v or int(v) < 0:
            raise ValueError(f"count must be a non-negative integer, got {v}")
        v = int(v)
    elif mode == "fraction":
        v = float(v)
        if not (0.0 <= v <= 1.0):
            raise ValueError(f"fraction must be in [0, 1], got {v}")
    else:
        f, F = (int(x) for x in v)
        if F < 1 or not (0 <= f < F):
            raise ValueError(f"fold must be (f, F) with 0 <= f < F, got {v}")
        v = (f, F)
    return mode, v


def split_windows(eligible: torch.Tensor, mode: str, value, min_keep: int = 1):
    """The rank window [lo, hi) of every row from its eligible count e (any integer tensor;
    the same arithmetic on a CPU tensor is what the tests compare with):
      count k     [0, min(k, max(e - min_keep, 0)))
      fraction p  [0, min(floor(p e + 0.5), max(e - min_keep, 0)))   (p e in fp64)
      fold f / F  [floor(f e / F), floor((f + 1) e / F))
    Returns (lo int32, hi int32)."""
    e = eligible.long()
    room = torch.clamp(e - int(min_keep), min=0)
    if mode == "count":
        lo, hi = torch.zeros_like(e), torch.clamp(room, max=int(value))
    elif mode == "fraction":
        want = torch.floor(float(value) * e.double() + 0.5).long()
        lo, hi = torch.zeros_like(e), torch.minimum(want, room)
    elif mode == "fold":
        f, F = value
        lo, hi = (f * e) // F, ((f + 1) * e) // F
    else:
        raise ValueError(f"mode must be one of {SPLIT_MODES}, got {mode!r}")
    return lo.to(torch.int32).contiguous(), hi.to(torch.int32).contiguous()
