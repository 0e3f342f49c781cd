"""K1, K17, K18: id maps and rating CSR (csrc/csr_build.hip: als_index_build,
als_csr_build; csrc/csr_merge.hip: als_csr_merge; csrc/csr_remove.hip:
als_csr_remove_mark, als_csr_remove_compact), plus the torch-side helpers that slice and
group CSR rows."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr
from .workspace import Workspace


@dataclass
class IdIndex:
    """Dense id map of one side (the device form of Spark's sorted InBlock.srcIds).

    Spark accepts any Int id (negative ones included).  The map is indexed by
    `id - offset`; `offset` is the smallest id when ids are negative or the id
    range starts far above 0, else 0 (ids used directly)."""
    map: torch.Tensor       # int32 [id_space], (id - offset) -> dense row or -1
    uniq: torch.Tensor      # int32 [n]   ascending ids - offset
    n: int
    offset: int = 0

    @property
    def id_space(self) -> int:
        return int(self.map.numel())

    def ids(self) -> torch.Tensor:
        """The original ids of the dense rows (ascending), int32."""
        return self.uniq if self.offset == 0 else (self.uniq.long() + self.offset).to(torch.int32)

    def rows_of(self, ids: torch.Tensor) -> torch.Tensor:
        """Dense row (int64) of each id, -1 when unknown."""
        k = ids.long() - self.offset
        ok = (k >= 0) & (k < self.id_space)
        out = torch.full_like(k, -1)
        out[ok] = self.map[k[ok]].long()
        return out

    def keys(self, ids: torch.Tensor) -> torch.Tensor:
        """Query ids -> map keys; ids outside the mapped range -> -1 (unknown)."""
        if self.offset == 0:
            return ids.to(torch.int32).contiguous()
        s = ids.long() - self.offset
        return torch.where((s >= 0) & (s < self.id_space), s, -1).to(torch.int32).contiguous()


MAX_ID_SPACE = 2 ** 31 - 1   # the map is indexed by int32


def id_offset(lo: int, hi: int) -> int:
    """Map offset for ids in [lo, hi]: 0 for the usual non-negative, compact ids."""
    off = 0 if (lo >= 0 and hi < (1 << 26)) else lo
    if hi - off + 1 > MAX_ID_SPACE:
        raise ValueError(f"id range [{lo}, {hi}] spans more than 2^31-1 values; this build "
                         "indexes ids through a dense int32 map")
    return off


def build_index(ids: torch.Tensor, id_space: int, ws: Workspace) -> IdIndex:
    L = _lib.lib()
    dev = ids.device
    mp = torch.empty(id_space, dtype=torch.int32, device=dev)
    uniq = torch.empty(id_space, dtype=torch.int32, device=dev)
    nu = torch.zeros(1, dtype=torch.int32, device=dev)
    need = L.als_index_workspace_bytes(ids.numel(), id_space)
    w = ws.get(need)
    check(L.als_index_build(ptr(ids), ids.numel(), id_space, ptr(mp), ptr(uniq), ptr(nu), ptr(w),
                            w.numel(), stream_ptr(dev)), "als_index_build")
    n = int(nu.item())
    return IdIndex(mp, uniq[:n].clone(), n)


def build_csr(row_ids: torch.Tensor, row_index: IdIndex, col_ids: torch.Tensor,
              col_index: IdIndex, vals: torch.Tensor, ws: Workspace):
    """K1 (als_csr_build) alone: (row_ptr int64 [n + 1], col int32, val f32) of one side,
    without a schedule."""
    L = _lib.lib()
    dev = row_ids.device
    nnz = int(row_ids.numel())
    n_rows = row_index.n
    row_ptr = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.float32, device=dev)
    w = ws.get(L.als_csr_workspace_bytes(nnz, n_rows))
    check(L.als_csr_build(ptr(row_ids), ptr(row_index.map), ptr(col_ids), ptr(col_index.map),
                          ptr(vals), nnz, n_rows, ptr(row_ptr), ptr(col), ptr(val), ptr(w),
                          w.numel(), stream_ptr(dev)), "als_csr_build")
    return row_ptr, col, val


def csr_merge_tile() -> int:
    """Output entries per workgroup of als_csr_merge (tests size their shapes from it)."""
    return int(_lib.lib().als_csr_merge_tile())


def merge_csr(row_ptr_old, col_old, val_old, n_cols_old: int, row_map, col_map, row_ptr_add,
              col_add, val_add):
    """K17 (als_csr_merge): the CSR K1 would build from concat(old ratings, batch), from the
    old side's CSR and the batch's CSR (built by K1 against the grown id maps), in one pass
    with no sort.  row_map / col_map: int32 [n_old] / [n_cols_old], the dense row each old
    row of this / the other side has after the growth, None where the side gained no id.
    Returns (row_ptr int64 [n_new + 1], col int32, val f32); the contract is in
    include/als_hip.h."""
    L = _lib.lib()
    dev = row_ptr_old.device
    n_old, n_new = int(row_ptr_old.numel()) - 1, int(row_ptr_add.numel()) - 1
    nnz_old, nnz_add = int(col_old.numel()), int(col_add.numel())
    row_ptr = torch.empty(n_new + 1, dtype=torch.int64, device=dev)
    col = torch.empty(nnz_old + nnz_add, dtype=torch.int32, device=dev)
    val = torch.empty(nnz_old + nnz_add, dtype=torch.float32, device=dev)
    check(L.als_csr_merge(ptr(row_ptr_old), ptr(col_old), ptr(val_old), nnz_old, n_old,
                          int(n_cols_old), ptr(row_map), ptr(col_map), ptr(row_ptr_add),
                          ptr(col_add), ptr(val_add), nnz_add, n_new, ptr(row_ptr), ptr(col),
                          ptr(val), stream_ptr(dev)), "als_csr_merge")
    return row_ptr, col, val


def grow_index(index: IdIndex, ids: torch.Tensor, ws: Workspace):
    """The id map of `index`'s ids plus `ids` (int32 original ids, device), as a fresh
    build_index over the union would make it: (grown IdIndex, new_of_old, new_rows).
    new_of_old: int32 [index.n], the dense row each old row has now (strictly increasing),
    None when no id is new; new_rows: int64, the dense rows of the new ids, ascending.  A new
    id below the old offset, or a negative one, re-bases the map (id_offset of the union)."""
    dev = ids.device
    old_lo, old_hi = int(index.uniq[0]) + index.offset, int(index.uniq[-1]) + index.offset
    lo, hi = min(old_lo, int(ids.min())), max(old_hi, int(ids.max()))
    off = id_offset(lo, hi)
    old_keys = (index.uniq.long() + (index.offset - off))
    keys = torch.cat([old_keys, ids.long() - off]).to(torch.int32).contiguous()
    grown = build_index(keys, hi - off + 1, ws)
    grown.offset = off
    if grown.n == index.n:
        return grown, None, torch.empty(0, dtype=torch.int64, device=dev)
    new_of_old = grown.map[old_keys].contiguous()
    is_new = torch.ones(grown.n, dtype=torch.bool, device=dev)
    is_new[new_of_old.long()] = False
    return grown, new_of_old, is_new.nonzero().flatten()


def csr_remove_tile() -> int:
    """Stored entries per workgroup of K18 (tests size their shapes from it)."""
    return int(_lib.lib().als_csr_remove_tile())


def keep_outputs(nnz: int, n_rows: int, dev):
    """The three results of a mark call (als_csr_remove_mark, als_split_mark), unfilled:
    (keep_bits int64 [ceil(nnz / 64)], tile_off int64 [tiles + 1], row_ptr_kept int64
    [n_rows + 1])."""
    tiles = -(-nnz // csr_remove_tile())
    return (torch.empty(-(-nnz // 64), dtype=torch.int64, device=dev),
            torch.empty(tiles + 1, dtype=torch.int64, device=dev),
            torch.empty(n_rows + 1, dtype=torch.int64, device=dev))


def remove_mark(row_ptr_old, col_old, row_ptr_del, col_del, ws: Workspace, count_hits=False):
    """K18, first call (als_csr_remove_mark): which stored entries of one side stay when the
    pairs of the delete CSR (row_ptr_del int64 [n + 1], col_del int32, every row's columns
    ascending; both None = delete nothing) leave.  Returns (keep_bits, tile_off, row_ptr_kept,
    del_hits): one bit per stored entry (int64 words holding the uint64 bits), the exclusive
    scan of the tiles' kept counts (tile_off[-1] = the entries that stay), the kept entries
    before every old row, and with count_hits the stored copies dropped per listed pair
    (else None).  The contract is in include/als_hip.h."""
    L = _lib.lib()
    dev = row_ptr_old.device
    n_old, nnz_old = int(row_ptr_old.numel()) - 1, int(col_old.numel())
    nnz_del = 0 if col_del is None else int(col_del.numel())
    keep_bits, tile_off, row_ptr_kept = keep_outputs(nnz_old, n_old, dev)
    hits = torch.empty(nnz_del, dtype=torch.int32, device=dev) if count_hits else None
    w = ws.get(L.als_csr_remove_scratch_bytes(nnz_old, n_old))
    check(L.als_csr_remove_mark(ptr(row_ptr_old), ptr(col_old), nnz_old, n_old, ptr(row_ptr_del),
                                ptr(col_del), nnz_del, ptr(keep_bits), ptr(tile_off),
                                ptr(row_ptr_kept), ptr(hits), ptr(w), w.numel(), stream_ptr(dev)),
          "als_csr_remove_mark")
    return keep_bits, tile_off, row_ptr_kept, hits


def remove_compact(col_old, val_old, keep_bits, tile_off, col_map, n_cols_old: int,
                   nnz_out: int):
    """K18, second call (als_csr_remove_compact): (col int32 [nnz_out], val f32 [nnz_out]), the
    kept entries in their stored order, columns passed through col_map (int32 [n_cols_old], the
    dense row each old row of the other side has now, None = unchanged)."""
    L = _lib.lib()
    dev = col_old.device
    col = torch.empty(int(nnz_out), dtype=torch.int32, device=dev)
    val = torch.empty(int(nnz_out), dtype=torch.float32, device=dev)
    check(L.als_csr_remove_compact(ptr(col_old), ptr(val_old), int(col_old.numel()),
                                   ptr(keep_bits), ptr(tile_off), ptr(col_map), int(n_cols_old),
                                   ptr(col), ptr(val), int(nnz_out), stream_ptr(dev)),
          "als_csr_remove_compact")
    return col, val


def shrink_index(index: IdIndex, leaving_rows: torch.Tensor, ws: Workspace):
    """The mirror of grow_index: the id map of `index` without the dense rows `leaving_rows`
    (int64, device), as a fresh build_index over the remaining ids would make it — offset and
    id_space are derived again, so they move when the smallest or the largest id leaves.
    Returns (IdIndex, new_of_old): new_of_old int32 [index.n], the dense row each old row has
    now, -1 for a row that left; (index, None) when none leaves.  At least one row must stay."""
    if leaving_rows.numel() == 0:
        return index, None
    dev = index.uniq.device
    stay = torch.ones(index.n, dtype=torch.bool, device=dev)
    stay[leaving_rows] = False
    ids = index.uniq[stay].long() + index.offset
    if ids.numel() == 0:
        raise ValueError("shrink_index: every row leaves")
    lo, hi = int(ids[0]), int(ids[-1])
    off = id_offset(lo, hi)
    shrunk = build_index((ids - off).to(torch.int32).contiguous(), hi - off + 1, ws)
    shrunk.offset = off
    new_of_old = torch.full((index.n,), -1, dtype=torch.int32, device=dev)
    new_of_old[stay] = torch.arange(shrunk.n, dtype=torch.int32, device=dev)
    return shrunk, new_of_old


def _delete_csr(rows: torch.Tensor, cols: torch.Tensor, n_rows: int):
    """(row_ptr int64 [n_rows + 1], col int32) of distinct (row, col) pairs that are sorted by
    row, then column: every row's columns ascending, as als_csr_remove_mark wants them."""
    row_ptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=rows.device)
    row_ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n_rows), 0)
    return row_ptr, cols.to(torch.int32).contiguous()


def gather_rows(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, rows: torch.Tensor):
    """The ragged rows `rows` (int64 dense rows) of a CSR as a CSR of their own, each row's
    entries in its stored order: (row_ptr int64 [m + 1], col int32, val f32), the input of
    fold_in_rows / nnls_rows."""
    beg = row_ptr[rows]
    ln = row_ptr[rows + 1] - beg
    out_ptr = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=row_ptr.device)
    out_ptr[1:] = torch.cumsum(ln, 0)
    src = torch.repeat_interleave(beg - out_ptr[:-1], ln) + torch.arange(
        int(out_ptr[-1]), device=row_ptr.device)
    return out_ptr, col[src].contiguous(), val[src].contiguous()


def group_pairs(rows: torch.Tensor, n_rows: int):
    """Pairs' row index (int64, in [0, n_rows)) -> (order, tgt_ptr int64 [n_rows + 1]):
    `order` lists the pairs grouped by row (stable: input order within a row), so pair
    order[s] fills target slot s of als_explain and each row is factored once."""
    rows = rows.reshape(-1).long()
    order = torch.sort(rows, stable=True).indices
    tgt_ptr = torch.zeros(int(n_rows) + 1, dtype=torch.int64, device=rows.device)
    if rows.numel():
        tgt_ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=int(n_rows)), 0)
    return order, tgt_ptr
