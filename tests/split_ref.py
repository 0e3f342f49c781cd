"""Numpy restatement of K20 (per-user holdout and stratified folds): the yardstick of
test_split_cpu.py, test_gpu_split.py and test_gpu_split_bounds.py.

Everything is brute force: the key per stored entry, the anchors by a sort per row of the other
side, the ranks by a sort per row of the selecting side, the windows, the thresholds as
include/als_hip.h defines them, the keep bits in K18's format (remove_ref.mark's layout), and
the kept / held-out triples.
"""
import numpy as np

M64 = (1 << 64) - 1
KEY_END = np.uint64(M64)
COL_END = np.int32(0x7FFFFFFF)


def key_py(seed, u, i):
    """The key with Python integers (the issue's four lines, mod 2^64)."""
    x = ((int(u) & 0xFFFFFFFF) << 32) | (int(i) & 0xFFFFFFFF)
    z = (x + ((int(seed) & M64) + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, u, i):
    """The same in numpy uint64, vectorised."""
    u = np.asarray(u, np.int64).astype(np.uint32).astype(np.uint64)
    i = np.asarray(i, np.int64).astype(np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        add = np.uint64(((int(seed) & M64) + 1) * 0x9E3779B97F4A7C15 & M64)
        z = ((u << np.uint64(32)) | i) + add
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def dense(ids, more=()):
    """(ascending distinct ids of `ids` and `more`, dense row of every element of `ids`); ids
    only in `more` make rows without entries."""
    ids = np.asarray(ids, np.int64)
    uniq = np.unique(np.concatenate([ids, np.asarray(more, np.int64)]))
    return uniq, np.searchsorted(uniq, ids).astype(np.int64)


def csr_side(rows, cols, n_rows):
    """K1's layout of one side: (row_ptr int64, col int32, order): rows ascending, input order
    within a row; order[q] = the input position of stored entry q."""
    order = np.argsort(rows, kind="stable")
    row_ptr = np.zeros(n_rows + 1, np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(rows, minlength=n_rows))
    return row_ptr, cols[order].astype(np.int32), order


def anchors(keys, sel_rows, oth_rows, n_oth):
    """int32 [n_oth]: per row of the other side the selecting-side row of its smallest
    (key, selecting row); -1 for a row without entries."""
    out = np.full(n_oth, -1, np.int32)
    for r in range(n_oth):
        at = np.nonzero(oth_rows == r)[0]
        if len(at):
            best = min((int(keys[j]), int(sel_rows[j])) for j in at)
            out[r] = best[1]
    return out


def windows(e, mode, value, min_keep=1):
    """(lo, hi) int32 per row from the eligible counts e, with Python integers per row."""
    lo, hi = [], []
    for n in np.asarray(e).tolist():
        room = max(n - min_keep, 0)
        if mode == "count":
            a, b = 0, min(int(value), room)
        elif mode == "fraction":
            a, b = 0, min(int(np.floor(np.float64(value) * np.float64(n) + 0.5)), room)
        else:
            f, F = value
            a, b = (f * n) // F, ((f + 1) * n) // F
        lo.append(a)
        hi.append(b)
    return np.array(lo, np.int32), np.array(hi, np.int32)


class Split:
    """The whole rule on triples (users, items, ratings), selecting side = users when
    user_side.  Attributes (all in INPUT order unless said otherwise):
      keys, eligible (bool), rank (int64, -1 where not eligible), held (bool),
      anchor int32 [rows of the other side] or None, e int64 [rows of the selecting side],
      lo / hi the windows used."""

    def __init__(self, users, items, seed, *, mode=None, value=None, min_keep=1,
                 keep_items=True, user_side=True, win=None, more_users=(), more_items=()):
        self.users = np.asarray(users, np.int64)
        self.items = np.asarray(items, np.int64)
        self.uids, self.urow = dense(self.users, more_users)
        self.iids, self.irow = dense(self.items, more_items)
        self.user_side = user_side
        self.keys = key(seed, self.users, self.items)
        sel, oth = (self.urow, self.irow) if user_side else (self.irow, self.urow)
        self.sel, self.oth = sel, oth
        self.n_sel = len(self.uids) if user_side else len(self.iids)
        self.n_oth = len(self.iids) if user_side else len(self.uids)
        self.anchor = anchors(self.keys, sel, oth, self.n_oth) if keep_items else None
        self.eligible = (np.ones(len(sel), bool) if self.anchor is None
                         else self.anchor[oth] != sel)
        self.e = np.bincount(sel[self.eligible], minlength=self.n_sel).astype(np.int64)
        self.rank = np.full(len(sel), -1, np.int64)
        for r in range(self.n_sel):
            at = np.nonzero((sel == r) & self.eligible)[0]
            comp = [(int(self.keys[j]), int(oth[j])) for j in at]
            first = {}
            for pos, c in enumerate(sorted(comp)):
                first.setdefault(c, pos)             # entries strictly below: copies share it
            for j, c in zip(at, comp):
                self.rank[j] = first[c]
        if mode is not None or win is not None:
            self.set_windows(mode, value, min_keep, win)

    def set_windows(self, mode=None, value=None, min_keep=1, win=None):
        """Windows by mode, or `win` = (lo, hi) arrays or a function of the eligible counts."""
        if win is None:
            win = windows(self.e, mode, value, min_keep)
        elif callable(win):
            win = win(self.e)
        sel = self.sel
        self.lo, self.hi = (np.asarray(w, np.int32) for w in win)
        self.held = self.eligible & (self.rank >= self.lo[sel]) & (self.rank < self.hi[sel])
        return self

    def thresholds(self):
        """(lo_key uint64, lo_col int32, hi_key, hi_col) per row of the selecting side: the
        smallest composite among the row's eligible entries of rank >= the window end, the
        end composite when there is none."""
        out = (np.full(self.n_sel, KEY_END), np.full(self.n_sel, COL_END),
               np.full(self.n_sel, KEY_END), np.full(self.n_sel, COL_END))
        for r in range(self.n_sel):
            at = np.nonzero((self.sel == r) & self.eligible)[0]
            for w, k in ((0, max(int(self.lo[r]), 0)), (2, max(int(self.hi[r]), 0))):
                comp = [(int(self.keys[j]), int(self.oth[j])) for j in at if self.rank[j] >= k]
                if comp:
                    out[w][r], out[w + 1][r] = np.uint64(min(comp)[0]), np.int32(min(comp)[1])
        return out

    def side(self, user_rows):
        """K1's CSR of one side: (row_ptr, col, order, n_rows, n_cols, row_ids, col_ids)."""
        rows, cols = (self.urow, self.irow) if user_rows else (self.irow, self.urow)
        ids = (self.uids, self.iids) if user_rows else (self.iids, self.uids)
        row_ptr, col, order = csr_side(rows, cols, len(ids[0]))
        return (row_ptr, col, order, len(ids[0]), len(ids[1]), ids[0].astype(np.int32),
                ids[1].astype(np.int32))

    def marks(self, user_rows, T):
        """(keep_bits uint64, tile_off int64, row_ptr_kept int64) of one side, K18's format."""
        row_ptr, _, order = self.side(user_rows)[:3]
        keep = ~self.held[order]
        nnz = len(keep)
        bits = np.zeros(-(-nnz // 64) * 64, np.uint8)
        bits[:nnz] = keep
        keep_bits = np.packbits(bits, bitorder="little").view(np.uint64)
        tiles = -(-nnz // T)
        tile_off = np.zeros(tiles + 1, np.int64)
        for t in range(tiles):
            tile_off[t + 1] = tile_off[t] + int(keep[t * T:(t + 1) * T].sum())
        before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
        return keep_bits, tile_off, before[row_ptr]

    def eligible_counts(self):
        return self.e.astype(np.int32)

    def kept(self, triples):
        """The kept triples in input order."""
        return tuple(np.asarray(x)[~self.held] for x in triples)

    def held_out(self, triples):
        """The held-out triples in the USER side's stored order (users ascending, input order
        within a user)."""
        order = np.argsort(self.urow, kind="stable")
        pick = order[self.held[order]]
        return tuple(np.asarray(x)[pick] for x in triples)
