"""numpy restatement of K17 (als_csr_merge) and the case list the update tests share.

merge(): row by row, the old segment with its columns renumbered, then the batch's segment.
grow(): the id map of the old ids plus the batch's, and the monotone old-to-new row map.
side_inputs(): everything als_csr_merge takes for one side, made from (old triples, batch
triples) with the oracle's index_build / csr_build, plus what it must return: the oracle's
csr_build of the concatenation.

The cases are built from a tile length T (als_csr_merge_tile() on the GPU, any number here):
about 40 rows per side, row lengths [0-free] 1, T-1, T, T+1, 2T+3, ..., batches of 1 to ~64.
"""
import numpy as np

from oracle import als_oracle as O

CASES = ("a_no_new_id", "b_new_users", "b_new_items", "b_new_both", "c_below_offset",
         "c_negative", "c_high_first_id", "d_duplicates", "e_tile_edges", "f_one", "g_every_row")


def id_offset(lo, hi):
    """engine.id_offset, restated."""
    return 0 if (lo >= 0 and hi < (1 << 26)) else lo


def merge(row_ptr_old, col_old, val_old, new_of_old_row, new_of_old_col, row_ptr_add, col_add,
          val_add):
    """als_csr_merge's contract, one row at a time.  Maps may be None (identity)."""
    n_old, n_new = len(row_ptr_old) - 1, len(row_ptr_add) - 1
    old_of_new = np.full(n_new, -1, np.int64)
    rows = np.arange(n_old) if new_of_old_row is None else np.asarray(new_of_old_row, np.int64)
    old_of_new[rows] = np.arange(n_old)
    cmap = None if new_of_old_col is None else np.asarray(new_of_old_col, np.int32)
    cols, vals, ptr = [], [], [0]
    for r in range(n_new):
        j = old_of_new[r]
        n = 0
        if j >= 0:
            c = np.asarray(col_old[row_ptr_old[j]:row_ptr_old[j + 1]], np.int32)
            cols.append(c if cmap is None else cmap[c])
            vals.append(val_old[row_ptr_old[j]:row_ptr_old[j + 1]])
            n += len(c)
        cols.append(col_add[row_ptr_add[r]:row_ptr_add[r + 1]])
        vals.append(val_add[row_ptr_add[r]:row_ptr_add[r + 1]])
        ptr.append(ptr[-1] + n + len(cols[-1]))
    cat = lambda xs, dt: (np.concatenate(xs) if xs else np.zeros(0)).astype(dt)
    return np.asarray(ptr, np.int64), cat(cols, np.int32), cat(vals, np.float32)


def index_of(ids):
    """(map, uniq, offset) as ALSCore builds them: the oracle's index over ids - offset."""
    ids = np.asarray(ids, np.int64)
    off = id_offset(int(ids.min()), int(ids.max()))
    mp, uniq = O.index_build(ids - off, int(ids.max()) - off + 1)
    return mp, uniq, off


def grow(old_ids, add_ids):
    """((map, uniq, offset) of the union, new_of_old int32 [n_old] or None when no id is
    new)."""
    old_ids, add_ids = np.asarray(old_ids, np.int64), np.asarray(add_ids, np.int64)
    mp, uniq, off = index_of(np.concatenate([old_ids, add_ids]))
    old_uniq = np.unique(old_ids)
    if len(uniq) == len(old_uniq):
        return (mp, uniq, off), None
    return (mp, uniq, off), mp[old_uniq - off].astype(np.int32)


def side_inputs(old, add, user_side=True):
    """old / add: (users, items, ratings).  Returns (inputs dict of als_csr_merge for the
    side, want = (row_ptr, col, val) of the oracle's csr_build on the concatenation)."""
    ro, co = (old[0], old[1]) if user_side else (old[1], old[0])
    ra, ca = (add[0], add[1]) if user_side else (add[1], add[0])
    ro, co, ra, ca = (np.asarray(x, np.int64) for x in (ro, co, ra, ca))
    rmp0, runiq0, roff0 = index_of(ro)
    cmp0, cuniq0, coff0 = index_of(co)
    old_csr = O.csr_build(rmp0[ro - roff0], cmp0[co - coff0], old[2], len(runiq0))
    (rmp, runiq, roff), rmap = grow(ro, ra)
    (cmp_, cuniq, coff), cmap = grow(co, ca)
    add_csr = O.csr_build(rmp[ra - roff], cmp_[ca - coff], add[2], len(runiq))
    rows = np.concatenate([ro, ra])
    cols = np.concatenate([co, ca])
    vals = np.concatenate([np.asarray(old[2], np.float32), np.asarray(add[2], np.float32)])
    want = O.csr_build(rmp[rows - roff], cmp_[cols - coff], vals, len(runiq))
    inputs = dict(row_ptr_old=old_csr[0], col_old=old_csr[1], val_old=old_csr[2],
                  n_cols_old=len(cuniq0), new_of_old_row=rmap, new_of_old_col=cmap,
                  row_ptr_add=add_csr[0], col_add=add_csr[1], val_add=add_csr[2])
    return inputs, want


def warm_cold_data(seed=3, share=0.02):
    """(old triples, batch triples) of the warm-start test: helpers.planted's seeded low-rank
    300 x 200 set (rank 8), `share` of it held back as the batch.  A held-back rating whose
    user or item would otherwise be unknown stays in the old set, so the batch brings no id."""
    from helpers import planted
    u, i, r = planted(300, 200, density=0.08, k_true=8, seed=seed)
    rng = np.random.default_rng(seed + 1)
    hold = np.zeros(len(u), bool)
    hold[rng.permutation(len(u))[:int(round(share * len(u)))]] = True
    for ids in (u, i):
        left = np.bincount(ids[~hold], minlength=int(ids.max()) + 1)
        hold &= left[ids] > 0
    return (u[~hold], i[~hold], r[~hold]), (u[hold], i[hold], r[hold])


def objective(u, i, r, U, V, reg):
    """The explicit training objective (als_hip.h, K10) in fp64 over dense-row triples:
    sum (r - <x_u, y_i>)^2 + reg (sum_u n_u |x_u|^2 + sum_i n_i |y_i|^2)."""
    U, V = np.asarray(U, np.float64), np.asarray(V, np.float64)
    s = (U[u] * V[i]).sum(1)
    nu, ni = np.bincount(u, minlength=len(U)), np.bincount(i, minlength=len(V))
    return float(((np.asarray(r, np.float64) - s) ** 2).sum()
                 + reg * ((nu * (U * U).sum(1)).sum() + (ni * (V * V).sum(1)).sum()))


def row_lengths(T):
    """User-row lengths of the base data: the tile edges first, then short rows up to ~40."""
    return [1, T - 1, T, T + 1, 2 * T + 3, 1, 2, T - 2, 3] + [2 + (j % 5) for j in range(31)]


def base_ratings(T, seed=0, n_items=41, user_step=3, item_step=2, user0=5, item0=4):
    """(users, items, ratings) of about 40 x 41 rows.  User ids user0, user0 + step, ... leave
    gaps for new ids between them; user j has row_lengths(T)[j] ratings (items repeat once a
    row is longer than the catalogue: duplicates are ordinary).  Every item is rated."""
    rng = np.random.default_rng(seed)
    lens = row_lengths(T)
    uid = user0 + user_step * np.arange(len(lens))
    iid = item0 + item_step * np.arange(n_items)
    u = np.repeat(uid, lens)
    i = iid[rng.integers(0, n_items, len(u))]
    i[:n_items] = iid                      # every item occurs (the first rows are long enough)
    order = rng.permutation(len(u))        # input order is not row order
    u, i = u[order], i[order]
    r = (rng.integers(1, 11, len(u)) * 0.5).astype(np.float32)
    return u.astype(np.int64), i.astype(np.int64), r


def case(name, T, seed=0):
    """(old triples, batch triples) of one named case."""
    rng = np.random.default_rng(100 + CASES.index(name))
    kw = {}
    if name == "c_below_offset":
        kw = dict(user0=(1 << 26) + 40, item0=(1 << 26) + 50)     # offset = the smallest id
    old = base_ratings(T, seed, **kw)
    u, i, _ = old
    uid, iid = np.unique(u), np.unique(i)
    lens = row_lengths(T)
    pick = lambda ids, n: ids[rng.integers(0, len(ids), n)]
    if name == "a_no_new_id":
        bu, bi = pick(uid, 40), pick(iid, 40)
    elif name == "b_new_users":      # before, between and after the existing ids
        bu = np.array([uid[0] - 2, uid[3] + 1, uid[3] + 2, uid[-1] + 7, uid[0] - 2, uid[10]])
        bi = pick(iid, len(bu))
    elif name == "b_new_items":
        bi = np.array([iid[0] - 1, iid[5] + 1, iid[-1] + 3, iid[-1] + 9, iid[7], iid[0] - 1])
        bu = pick(uid, len(bi))
    elif name == "b_new_both":
        bu = np.array([uid[0] - 1, uid[2] + 1, uid[-1] + 1, uid[4], uid[4], uid[0] - 1, uid[9] + 1])
        bi = np.array([iid[0] - 3, iid[1] + 1, iid[3], iid[-1] + 2, iid[0] - 3, iid[6], iid[-1] + 2])
    elif name == "c_below_offset":   # a new smallest id moves the offset down
        bu = np.array([uid[0] - 17, uid[5], uid[-1] + 1])
        bi = np.array([iid[3], iid[0] - 9, iid[0] - 9])
    elif name == "c_negative":       # a negative id: the offset leaves 0
        bu = np.array([-7, uid[2], uid[8], -7])
        bi = np.array([iid[1], -3, iid[4], -3])
    elif name == "c_high_first_id":  # a first id >= 2^26: the offset leaves 0 as well
        bu = np.array([(1 << 26) + 5, uid[1]])   # (users only: the map has 2^26 entries)
        bi = np.array([iid[2], iid[0]])
    elif name == "d_duplicates":     # a pair already rated, and one pair twice in the batch
        bu = np.array([u[0], u[7], uid[6], uid[6], u[0]])
        bi = np.array([i[0], i[7], iid[9], iid[9], i[0]])
    elif name == "e_tile_edges":     # the 2T + 3 row and the rows that meet a tile edge
        edge = [j for j, n in enumerate(lens) if n in (T - 1, T, T + 1, 2 * T + 3, T - 2)]
        bu = np.repeat(uid[edge + [0]], 3)
        bi = pick(iid, len(bu))
    elif name == "f_one":
        bu, bi = uid[4:5], iid[11:12]
    elif name == "g_every_row":
        bu = np.concatenate([uid, pick(uid, len(iid))])
        bi = np.concatenate([pick(iid, len(uid)), iid])
    else:
        raise KeyError(name)
    br = (rng.integers(1, 11, len(bu)) * 0.5).astype(np.float32)
    return old, (np.asarray(bu, np.int64), np.asarray(bi, np.int64), br)
