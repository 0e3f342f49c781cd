"""Shapes for the paths of the CSR tile kernels (K17 als_csr_merge, K18 als_csr_remove_*, K20
als_split_*) that the ~40-row family of update_ref.base_ratings never reaches, and vectorised
numpy restatements (FastSplit, keep_format) that keep the GPU tests on them quick: the
brute-force split_ref.Split runs again per seed, side and window.

  ones         S1  3T + 17 rows of one entry: a tile meets T rows, T / 256 row batches
  seams        S2  rows of one entry with long rows (T + 5, 2, T - 1, 2T + 3 in turn) where the
                   row index counted from the tile's first row is 255, 256 or 257
  gaps         S3  raw CSR: 40 short rows, 600 empty, 40 short, 300 empty (or 300 empty first)
  two_long     S4  the item side has rows A (2048 + 700 entries from position 300), B (2048 + 9,
                   right after A: both meet anchor tile 1) and C (2 * 2048 + 1, starting on a
                   multiple of 2048)
  long65       S5  an item row of 65 * 2048 + 77 entries from position 5; two users occur in it
                   once, in anchor tiles 64 and 65
  many_listed  S6  2 * 2048 + 37 user rows of 2 to 5 entries (every row is listed at row_cap 1)
  carry        S7  raw CSR of 4096 T + T + 5 entries: 4098 tiles, two trips of the scan

Everything is integers and f32 ratings in half steps; the restatements use integer numpy only.
"""
import numpy as np

import split_ref as SR

TASK = 2048          # kSplitTask of csrc/split.hip (test_csr_many_rows_cpu.py reads it there)
BATCH = 256          # rows per trip of the row walk (kTileThreads of csrc/csr_tile_walk.h)
SCAN_TRIP = 4096     # tile counts per trip of remove_scan_kernel (kScanThreads * kScanItems)
LONG_GRID = 2048     # kSplitLongGrid
SEED = 20


def _half_steps(rng, n):
    return (rng.integers(1, 11, n) * 0.5).astype(np.float32)


def _ptr(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int64)


# ---------------------------------------------------------------- the row walk, described
def walk(row_ptr, T):
    """What the 256-rows-at-a-time walk of a tile kernel does on row_ptr, per tile: a list of
    dicts with row0 (the last row that starts at or before the tile's first entry) and trips, a
    list of (first row of the batch, done, stop): the entries [done, stop) are handled in that
    trip (stop == done: a batch of rows without an entry in the tile)."""
    row_ptr = np.asarray(row_ptr, np.int64)
    n, nnz = len(row_ptr) - 1, int(row_ptr[-1])
    out = []
    for p0 in range(0, nnz, T):
        p1 = min(p0 + T, nnz)
        row0 = int(np.searchsorted(row_ptr[:n + 1], p0, side="right")) - 1
        row0 = min(row0, n - 1)
        trips, done, r = [], p0, row0
        while done < p1:
            last = r + BATCH - 1
            batch_end = int(row_ptr[last + 1]) if last < n else nnz
            stop = min(batch_end, p1)
            trips.append((r, done, stop))
            done = max(done, stop)
            r += BATCH
        out.append(dict(row0=row0, trips=trips))
    return out


def seam_rows(row_ptr, T):
    """The rows at index 255 and 256 counted from a tile's first row (the last row of a batch
    and the first of the next), for every batch a tile walks, plus rows 0 and n - 1:
    ascending, distinct."""
    n = len(row_ptr) - 1
    rows = {0, n - 1}
    for w in walk(row_ptr, T):
        rows |= {w["row0"] + BATCH - 1, w["row0"] + BATCH}
        for r, _, _ in w["trips"][1:]:
            rows |= {r - 1, r}
    return np.array(sorted(x for x in rows if 0 <= x < n), np.int64)


# ---------------------------------------------------------------- S1, S2: triples
def _triples(lens, n_items, seed, user0=5, user_step=3, item0=4, item_step=2):
    """(users, items, ratings): user j (id user0 + user_step * j: new ids fit between) has
    lens[j] ratings of items drawn from a catalogue of n_items (every item occurs), shuffled."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    uid = user0 + user_step * np.arange(len(lens))
    iid = item0 + item_step * np.arange(n_items)
    u = np.repeat(uid, lens)
    i = iid[rng.integers(0, n_items, len(u))]
    i[rng.permutation(len(u))[:n_items]] = iid
    order = rng.permutation(len(u))
    return u[order].astype(np.int64), i[order].astype(np.int64), _half_steps(rng, len(u))


def ones_lens(T):
    return np.ones(3 * T + 17, np.int64)


def ones(T, seed=0):
    """S1."""
    return _triples(ones_lens(T), 41, seed)


def seams_lens(T, n_rows=1100):
    """Row lengths of S2: 1, except where the row's index counted from the first row of the
    tile it starts in is 255, 256 or 257; those rows take T + 5, 2, T - 1, 2T + 3 in turn."""
    turn = (T + 5, 2, T - 1, 2 * T + 3)
    lens, starts, k, pos = [], [], 0, 0
    for r in range(n_rows):
        p0 = pos // T * T
        starts.append(pos)
        # the last row that starts at or before p0 (this one when it starts the tile)
        row0 = int(np.searchsorted(np.asarray(starts), p0, side="right")) - 1
        if r - row0 in (255, 256, 257):
            lens.append(turn[k % 4])
            k += 1
        else:
            lens.append(1)
        pos += lens[-1]
    return np.asarray(lens, np.int64)


def seams(T, seed=1):
    """S2."""
    return _triples(seams_lens(T), 97, seed)


def batch(old, kind, seed=5):
    """A batch of ratings for K17 on old = S1 or S2 triples.
    a_no_new_id   200 ratings of known users and items, every 1/200 of the user rows hit
    b_new_rows    one rating by a new user in front, in every gap between two old ids, and by
                  300 consecutive new ids after the last one (known items)
    c_new_cols    200 ratings of known users, of new items in front, between and after
    d_empty       nothing"""
    rng = np.random.default_rng(seed)
    uid, iid = np.unique(old[0]), np.unique(old[1])
    if kind == "a_no_new_id":
        bu = uid[np.linspace(0, len(uid) - 1, 200).astype(np.int64)]
        bi = iid[rng.integers(0, len(iid), 200)]
    elif kind == "b_new_rows":
        bu = np.concatenate([[uid[0] - 1], uid[:-1] + 1, uid[-1] + 1 + np.arange(300)])
        bi = iid[rng.integers(0, len(iid), len(bu))]
    elif kind == "c_new_cols":
        bu = uid[np.linspace(0, len(uid) - 1, 200).astype(np.int64)]
        new = np.concatenate([[iid[0] - 2, iid[0] - 1], iid[:-1:3] + 1, iid[-1] + 1 + np.arange(9)])
        bi = new[rng.integers(0, len(new), 200)]
    elif kind == "d_empty":
        bu = bi = np.zeros(0, np.int64)
    else:
        raise KeyError(kind)
    order = rng.permutation(len(bu))
    return (np.asarray(bu, np.int64)[order], np.asarray(bi, np.int64)[order],
            _half_steps(rng, len(bu)))


BATCHES = ("a_no_new_id", "b_new_rows", "c_new_cols", "d_empty")


def user_csr(old):
    """(row_ptr, row of every input triple) of the user side of triples."""
    uid, row = np.unique(old[0], return_inverse=True)
    return _ptr(np.bincount(row, minlength=len(uid))), row


def delete_pairs(old, kind, T):
    """(users, items) listed for removal from old = S1 or S2 triples.
    every_5th   the first stored rating of every 5th user row
    seam_rows   every rating of the user rows on a batch seam (seam_rows)
    nothing     no pair"""
    row_ptr, row = user_csr(old)
    if kind == "every_5th":
        sel = np.argsort(row, kind="stable")[row_ptr[:-1]][::5]    # first input position per row
    elif kind == "seam_rows":
        sel = np.nonzero(np.isin(row, seam_rows(row_ptr, T)))[0]
    elif kind == "nothing":
        sel = np.zeros(0, np.int64)
    else:
        raise KeyError(kind)
    return old[0][sel], old[1][sel]


DELETES = ("every_5th", "seam_rows", "nothing")


# ---------------------------------------------------------------- S3: raw CSR with empty runs
def gaps_lens(front_empty=False):
    short = [1 + (j * 7) % 5 for j in range(40)]
    lens = short + [0] * 600 + short[::-1] + [0] * 300
    return np.asarray(([0] * 300 if front_empty else []) + lens, np.int64)


def gaps_csr(front_empty=False, n_cols=23, seed=2):
    """S3 as (row_ptr int64, col int32, val f32)."""
    rng = np.random.default_rng(seed)
    ptr = _ptr(gaps_lens(front_empty))
    return ptr, rng.integers(0, n_cols, ptr[-1]).astype(np.int32), _half_steps(rng, ptr[-1])


def gaps_merge_inputs(kind, front_empty=False, n_cols=23, seed=3):
    """als_csr_merge's inputs (update_ref.side_inputs' dict) on S3.  The batches are batch()'s
    kinds restated on rows: new rows in front, after every 7th old row (the runs of empty rows
    included: new_of_old_row is strictly increasing over them) and 300 after the last."""
    rng = np.random.default_rng(seed)
    ptr, col, val = gaps_csr(front_empty, n_cols)
    n_old = len(ptr) - 1
    has = np.nonzero(np.diff(ptr))[0]
    rmap = cmap = None
    n_new, n_cols_new = n_old, n_cols
    lens_add = np.zeros(n_old, np.int64)
    if kind == "a_no_new_id":
        lens_add[has[::2]] = 1 + np.arange(len(has[::2])) % 4
        lens_add[has[0] + 45] = 2          # a row of the empty run gets its first ratings
    elif kind == "b_new_rows":
        rmap = (1 + np.arange(n_old) + np.arange(n_old) // 7).astype(np.int32)
        n_new = int(rmap[-1]) + 1 + 300
        lens_add = np.ones(n_new, np.int64)
        lens_add[rmap] = 0
    elif kind == "c_new_cols":
        cmap = (2 + np.arange(n_cols) + np.arange(n_cols) // 3).astype(np.int32)
        n_cols_new = int(cmap[-1]) + 4
        lens_add[has[1::2]] = 1 + np.arange(len(has[1::2])) % 3
    elif kind != "d_empty":
        raise KeyError(kind)
    pa = _ptr(lens_add)
    return dict(row_ptr_old=ptr, col_old=col, val_old=val, n_cols_old=n_cols,
                new_of_old_row=rmap, new_of_old_col=cmap, row_ptr_add=pa,
                col_add=rng.integers(0, n_cols_new, pa[-1]).astype(np.int32),
                val_add=_half_steps(rng, pa[-1]))


def gaps_remove_inputs(kind, front_empty=False, n_cols=23):
    """The two K18 calls' inputs (remove_ref.side_inputs' dict) on S3; the delete lists are
    delete_pairs()'s kinds restated on rows.  Columns go through a map that drops column 0."""
    ptr, col, val = gaps_csr(front_empty, n_cols)
    n = len(ptr) - 1
    has = np.nonzero(np.diff(ptr))[0]
    dels = [np.zeros(0, np.int32)] * n
    if kind == "every_5th":
        for r in has[::5]:
            dels[r] = col[ptr[r]:ptr[r] + 1]
    elif kind == "seam_rows":      # the rows around the empty runs, whole
        for r in (has[0], has[39], has[40], has[-1]):
            dels[r] = np.unique(col[ptr[r]:ptr[r + 1]])
    elif kind != "nothing":
        raise KeyError(kind)
    cmap = (np.arange(n_cols) - 1).astype(np.int32)
    return dict(row_ptr_old=ptr, col_old=col, val_old=val, row_ptr_del=_ptr([len(d) for d in dels]),
                col_del=np.concatenate(dels).astype(np.int32), n_cols_old=n_cols,
                new_of_old_col=cmap)


def gaps_split(front_empty=False, seed=4):
    """S3 for K20: Split's keyword arguments; more_users supplies the rows without entries."""
    rng = np.random.default_rng(seed)
    lens = gaps_lens(front_empty)
    uid = 10 + np.arange(len(lens))
    u = np.repeat(uid, lens)
    i = rng.integers(0, 23, len(u)) - 5
    p = rng.permutation(len(u))
    return dict(users=u[p], items=i[p], more_users=uid[lens == 0])


# ---------------------------------------------------------------- S4 - S6: K20 shapes
def _short(rng, n_entries):
    """Row lengths 1 to 5 that sum to n_entries."""
    lens = []
    while sum(lens) < n_entries:
        lens.append(min(int(rng.integers(1, 6)), n_entries - sum(lens)))
    return lens


TWO_LONG = dict(a_start=300, a_len=TASK + 700, b_len=TASK + 9, c_len=2 * TASK + 1, n_users=4200)


def two_long(seed=6):
    """S4: (Split's keyword arguments, {"A" / "B" / "C": the item's dense row}).  Item rows in id
    order: short rows (300 entries), A, B, short rows up to the next multiple of 2048, C, a few
    short rows.  Users are distinct within an item's row."""
    rng = np.random.default_rng(seed)
    P = TWO_LONG
    lens = _short(rng, P["a_start"])
    rows = {"A": len(lens), "B": len(lens) + 1}
    lens += [P["a_len"], P["b_len"]]
    lens += _short(rng, -sum(lens) % TASK)
    rows["C"] = len(lens)
    lens += [P["c_len"]] + _short(rng, 40)
    iid = 3 * np.arange(len(lens)) - 30
    i = np.repeat(iid, lens)
    u = np.concatenate([rng.choice(P["n_users"], n, replace=False) for n in lens]) + 100
    p = rng.permutation(len(u))
    return dict(users=u[p], items=i[p]), rows


LONG65 = dict(start=5, length=65 * TASK + 77, catalogue=500)


def long65(seed=7):
    """S5: (Split's keyword arguments, the long item's dense row, {anchor tile: the user who
    occurs once in the long row, inside that tile}) for tiles 64 and 65 (the last)."""
    rng = np.random.default_rng(seed)
    P = LONG65
    lens = _short(rng, P["start"]) + [P["length"]] + _short(rng, 90)
    row = lens.index(P["length"])
    iid = 2 * np.arange(len(lens)) + 1
    cat = P["catalogue"]
    # in stored order first: the two planted users at fixed positions of the long row
    cols = [rng.integers(0, cat - 2, n) for n in lens]
    planted = {64: cat - 2, 65: cat - 1}
    cols[row][64 * TASK + 1000 - P["start"]] = planted[64]
    cols[row][65 * TASK + 40 - P["start"]] = planted[65]
    i, u = np.repeat(iid, lens), np.concatenate(cols) + 1000
    # a shuffle that keeps the order within every item: the stored order is the one above
    when = rng.random(len(u))
    for x in iid:
        when[i == x] = np.sort(when[i == x])
    p = np.argsort(when, kind="stable")
    return dict(users=u[p], items=i[p]), row, {t: v + 1000 for t, v in planted.items()}


MANY_LISTED = dict(n_rows=2 * LONG_GRID + 37, catalogue=300)


def many_listed(seed=8):
    """S6: Split's keyword arguments.  User j has 2 + j % 4 ratings; every 3rd user's are copies
    of one pair (a window edge inside the row falls between copies), every 7th other user rated
    one item twice."""
    rng = np.random.default_rng(seed)
    P = MANY_LISTED
    u, i = [], []
    for j in range(P["n_rows"]):
        n = 2 + j % 4
        if j % 3 == 0:
            it = [int(rng.integers(0, P["catalogue"]))] * n
        else:
            it = rng.choice(P["catalogue"], n, replace=False).tolist()
            if j % 7 == 0:
                it[-1] = it[0]
        u += [j + 50] * n
        i += it
    u, i = np.array(u), np.array(i) - 9
    p = rng.permutation(len(u))
    return dict(users=u[p], items=i[p])


def item_rows(kw, rows):
    """{row: (stored positions, users, items, user rows)} of some item rows of Split's keyword
    arguments kw, in the item side's stored order (items ascending, input order within one)."""
    users, items = np.asarray(kw["users"], np.int64), np.asarray(kw["items"], np.int64)
    _, urow = SR.dense(users, kw.get("more_users", ()))
    iids, irow = SR.dense(items, kw.get("more_items", ()))
    row_ptr, col, order = SR.csr_side(irow, urow, len(iids))
    out = {}
    for r in rows:
        at = np.arange(row_ptr[r], row_ptr[r + 1])
        out[r] = (at, users[order[at]], items[order[at]], col[at])
    return out


def item_row_min(entry, seed):
    """(stored position of the first copy, copies, user) of the smallest (key, user row) of
    one entry of item_rows()."""
    at, u, i, col = entry
    keys = SR.key(seed, u, i)
    best = np.lexsort((col, keys))[0]
    same = (keys == keys[best]) & (col == col[best])
    return int(at[best]), int(same.sum()), int(u[best])


def two_long_seed(kw, rows, start=SEED + 1, tries=2000):
    """The first seed >= start with the smallest composite of A and of B inside the anchor tile
    they share (tile 1) and that of C inside C's first tile (the one it starts exactly on)."""
    ent = item_rows(kw, rows.values())
    c_tile = int(ent[rows["C"]][0][0]) // TASK
    for seed in range(start, start + tries):
        tiles = {k: item_row_min(ent[r], seed)[0] // TASK for k, r in rows.items()}
        if tiles == {"A": 1, "B": 1, "C": c_tile}:
            return seed
    raise LookupError("many_rows_ref.two_long_seed: no seed found")


def long65_seed(kw, row, user, start=SEED + 1, tries=20000):
    """The first seed >= start for which the planted `user` holds the long row's smallest
    composite.  Only the row's distinct pairs are keyed."""
    at, u, i, col = item_rows(kw, [row])[row]
    _, first = np.unique(u, return_index=True)
    ent = (at[first], u[first], i[first], col[first])
    for seed in range(start, start + tries):
        if item_row_min(ent, seed)[2] == user:
            return seed
    raise LookupError("many_rows_ref.long65_seed: no seed found")


# ---------------------------------------------------------------- split_ref.Split, vectorised
class FastSplit(SR.Split):
    """split_ref.Split with the per-row Python loops replaced by np.lexsort on (row, key,
    column); test_csr_many_rows_cpu.py pins every attribute and method to the brute-force one."""

    def __init__(self, users, items, seed, *, mode=None, value=None, min_keep=1,
                 keep_items=True, user_side=True, win=None, more_users=(), more_items=()):
        self.users = np.asarray(users, np.int64)
        self.items = np.asarray(items, np.int64)
        self.uids, self.urow = SR.dense(self.users, more_users)
        self.iids, self.irow = SR.dense(self.items, more_items)
        self.user_side = user_side
        self.keys = SR.key(seed, self.users, self.items)
        sel, oth = (self.urow, self.irow) if user_side else (self.irow, self.urow)
        self.sel, self.oth = sel, oth
        self.n_sel = len(self.uids) if user_side else len(self.iids)
        self.n_oth = len(self.iids) if user_side else len(self.uids)
        self.anchor = None
        if keep_items:
            self.anchor = np.full(self.n_oth, -1, np.int32)
            o = np.lexsort((sel, self.keys, oth))
            first = np.ones(len(o), bool)
            first[1:] = oth[o][1:] != oth[o][:-1]
            self.anchor[oth[o][first]] = sel[o][first]
        self.eligible = (np.ones(len(sel), bool) if self.anchor is None
                         else self.anchor[oth] != sel)
        self.e = np.bincount(sel[self.eligible], minlength=self.n_sel).astype(np.int64)
        # eligible entries sorted by (selecting row, key, other row); a copy is not `new`
        at = np.nonzero(self.eligible)[0]
        o = at[np.lexsort((oth[at], self.keys[at], sel[at]))]
        s, k, c = sel[o], self.keys[o], oth[o]
        new = np.ones(len(o), bool)
        new[1:] = (s[1:] != s[:-1]) | (k[1:] != k[:-1]) | (c[1:] != c[:-1])
        start = np.concatenate([[0], np.cumsum(self.e)]).astype(np.int64)   # per selecting row
        first = np.maximum.accumulate(np.where(new, np.arange(len(o)), 0))
        self.rank = np.full(len(sel), -1, np.int64)
        self.rank[o] = first - start[s]
        # the next `new` entry at or after every sorted position (len(o) = none)
        nxt = np.where(new, np.arange(len(o)), len(o))
        self._next_new = np.minimum.accumulate(nxt[::-1])[::-1] if len(o) else nxt
        self._sorted, self._start = o, start
        if mode is not None or win is not None:
            self.set_windows(mode, value, min_keep, win)

    def thresholds(self):
        out = (np.full(self.n_sel, SR.KEY_END), np.full(self.n_sel, SR.COL_END),
               np.full(self.n_sel, SR.KEY_END), np.full(self.n_sel, SR.COL_END))
        o, start = self._sorted, self._start
        for w, win in ((0, self.lo), (2, self.hi)):
            k = np.maximum(np.asarray(win, np.int64), 0)
            inside = k < self.e
            j = np.where(inside, start[:-1] + np.minimum(k, np.maximum(self.e - 1, 0)), 0)
            j = self._next_new[np.minimum(j, max(len(o) - 1, 0))] if len(o) else j
            found = inside & (j < start[1:])
            src = o[j[found]]
            out[w][found] = self.keys[src]
            out[w + 1][found] = self.oth[src].astype(np.int32)
        return out

    def marks(self, user_rows, T):
        row_ptr, _, order = self.side(user_rows)[:3]
        keep = ~self.held[order]
        return keep_format(keep, row_ptr, T)


def keep_format(keep, row_ptr, T):
    """(keep_bits uint64, tile_off int64 [tiles + 1], row_ptr_kept) of a boolean keep vector in
    stored order: K18's format (remove_ref.mark's), without a loop."""
    keep = np.asarray(keep, bool)
    nnz = len(keep)
    bits = np.zeros(-(-nnz // 64) * 64, np.uint8)
    bits[:nnz] = keep
    keep_bits = np.packbits(bits, bitorder="little").view(np.uint64)
    tiles = -(-nnz // T)
    padded = np.zeros(tiles * T, np.int64)
    padded[:nnz] = keep
    tile_off = np.concatenate([[0], np.cumsum(padded.reshape(-1, T).sum(1))]).astype(np.int64)
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    return keep_bits, tile_off, before[np.asarray(row_ptr, np.int64)]


# ---------------------------------------------------------------- S7: the scan's carry
def carry(T, n_rows=70):
    """S7 as a dict: K18's inputs (row_ptr_old, col_old, val_old, row_ptr_del, col_del) and what
    the calls must give (keep_bits, tile_off, row_ptr_kept, del_hits, col, val).  nnz = 4096 T +
    T + 5: 4098 tiles; a row ends 3 entries before entry 4096 T and the next 2 after it;
    col_old[q] = q % 7 and every second row lists column 3."""
    nnz = SCAN_TRIP * T + T + 5
    edge = SCAN_TRIP * T
    cuts = [edge - 3, edge + 2, edge + T // 2]
    w = np.array([1 + (j * j * 5 + j * 37) % 101 for j in range(n_rows - len(cuts))], np.int64)
    cuts += (np.cumsum(w)[:-1] * (edge - 3) // w.sum()).tolist()
    row_ptr = np.array([0] + sorted(cuts) + [nnz], np.int64)
    assert len(row_ptr) == n_rows + 1 and (np.diff(row_ptr) > 0).all()
    q = np.arange(nnz, dtype=np.int64)
    col = (q % 7).astype(np.int32)
    val = ((q % 10 + 1) * 0.5).astype(np.float32)
    odd = np.arange(n_rows) % 2 == 1
    row = np.repeat(np.arange(n_rows), np.diff(row_ptr))
    keep = ~((col == 3) & odd[row])
    keep_bits, tile_off, row_ptr_kept = keep_format(keep, row_ptr, T)
    hits = np.bincount(row[~keep], minlength=n_rows)[odd].astype(np.int32)
    return dict(row_ptr_old=row_ptr, col_old=col, val_old=val, row_ptr_del=_ptr(odd),
                col_del=np.full(int(odd.sum()), 3, np.int32), keep_bits=keep_bits,
                tile_off=tile_off, row_ptr_kept=row_ptr_kept, del_hits=hits, col=col[keep],
                val=val[keep])
