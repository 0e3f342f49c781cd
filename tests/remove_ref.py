"""numpy restatement of K18 (als_csr_remove_mark / als_csr_remove_compact) and the case list
the removal tests share.

mark(): one keep bit per stored entry (dropped iff its column is in its row's delete list), the
scan of the per-tile kept counts, the kept entries before every old row, the hits per listed
pair.  compact(): the kept entries in stored order, columns through the other side's map.
side_inputs(): everything the two calls take for one side, made from (old triples, listed
pairs) with the oracle's index_build / csr_build, plus what they must produce: the oracle's
index_build / csr_build of the filtered triples.

The base data is update_ref.base_ratings(T) — about 40 x 41 rows, user-row lengths 1, T - 1, T,
T + 1, 2T + 3, ..., shuffled input order, duplicates in the long rows — plus
  * users with 63, 64 and 65 ratings (the keep_bits word edge),
  * a smallest and a largest user id whose one rating is the only one of the smallest / largest
    item id (rows that leave on both sides, at both ends),
  * an item rated once, by the 2T + 3 user,
  * a user with WIDE distinct items nobody else rated (a delete list longer than 256 in a row).
"""
import numpy as np

import update_ref as UR
from oracle import als_oracle as O

CASES = ("a_one_pair", "b_stored_duplicates", "c_missing", "d_user_leaves", "e_item_leaves",
         "f_both_leave", "g_first_and_last_rows_leave", "h_offset_moves", "h_largest_leaves",
         "i_tile_edges", "j_whole_rows", "k_all_but_one_row", "l_nothing_to_do")
WIDE = 300


def base(T, seed=0, user0=5, item0=4):
    """(old triples, names): names maps the special ids described in the module docstring."""
    u, i, r = UR.base_ratings(T, seed, user0=user0, item0=item0)
    rng = np.random.default_rng(seed + 77)
    uid, iid = np.unique(u), np.unique(i)
    umax, imax = int(uid[-1]), int(iid[-1])
    n = dict(ulo=user0 - 3, ilo=item0 - 3, u63=umax + 3, u64=umax + 6, u65=umax + 9,
             uwide=umax + 12, uhi=umax + 15, ionce=imax + 2, iwide0=imax + 10,
             ihi=imax + 10 + WIDE + 90, ulong=int(uid[4]))
    eu, ei = [n["ulo"], n["uhi"], n["ulong"]], [n["ilo"], n["ihi"], n["ionce"]]
    for key, ln in (("u63", 63), ("u64", 64), ("u65", 65)):
        eu += [n[key]] * ln
        ei += iid[rng.integers(0, len(iid), ln)].tolist()
    eu += [n["uwide"]] * (WIDE + 40)
    ei += list(range(n["iwide0"], n["iwide0"] + WIDE)) + iid[:40].tolist()
    eu, ei = np.asarray(eu, np.int64), np.asarray(ei, np.int64)
    er = (rng.integers(1, 11, len(eu)) * 0.5).astype(np.float32)
    u, i, r = np.concatenate([u, eu]), np.concatenate([i, ei]), np.concatenate([r, er])
    order = rng.permutation(len(u))
    return (u[order], i[order], r[order]), n


def _pair_keys(u, i):
    return (np.asarray(u, np.int64) << 32) | (np.asarray(i, np.int64) & 0xFFFFFFFF)


def listed(old, spec):
    """The (users, items) pairs a case's spec stands for: its "pairs", plus every stored pair
    of its "users" and of its "items"."""
    u, i, _ = old
    pu, pi = (np.asarray(x, np.int64) for x in spec.get("pairs", ([], [])))
    sel = np.isin(u, spec.get("users", [])) | np.isin(i, spec.get("items", []))
    return np.concatenate([pu, u[sel]]), np.concatenate([pi, i[sel]])


def filtered(old, pairs):
    """The old triples without every copy of every listed pair, order kept."""
    keep = ~np.isin(_pair_keys(old[0], old[1]), _pair_keys(*pairs))
    return tuple(x[keep] for x in old)


def expected_info(old, pairs):
    """What remove_ratings reports, with touched rows in the NEW numbering."""
    new = filtered(old, pairs)
    listed_keys = np.unique(_pair_keys(*pairs))
    out = {"removed": len(old[0]) - len(new[0]),
           "missing": int((~np.isin(listed_keys, _pair_keys(old[0], old[1]))).sum())}
    for s, side in ((0, "users"), (1, "items")):
        out[f"left_{side}"] = np.setdiff1d(old[s], new[s])
        ids, had = np.unique(old[s], return_counts=True)
        now = np.array([(new[s] == x).sum() for x in ids])
        out[f"touched_{side}"] = np.searchsorted(np.unique(new[s]), ids[(now > 0) & (now < had)])
    return out


# ---------------------------------------------------------------- the two passes, restated
def mark(row_ptr_old, col_old, row_ptr_del, col_del, T):
    """als_csr_remove_mark: (keep_bits uint64, tile_off int64 [tiles + 1], row_ptr_kept int64
    [n + 1], del_hits int32 [nnz_del]).  row_ptr_del / col_del None = delete nothing."""
    row_ptr_old = np.asarray(row_ptr_old, np.int64)
    n, nnz = len(row_ptr_old) - 1, len(col_old)
    row = np.repeat(np.arange(n), np.diff(row_ptr_old))
    key = (row << 32) | np.asarray(col_old, np.int64)
    if row_ptr_del is None:
        dkey = np.zeros(0, np.int64)
    else:
        drow = np.repeat(np.arange(n), np.diff(np.asarray(row_ptr_del, np.int64)))
        dkey = (drow << 32) | np.asarray(col_del, np.int64)
        for r in range(n):
            seg = np.asarray(col_del[row_ptr_del[r]:row_ptr_del[r + 1]])
            assert (np.diff(seg) >= 0).all(), "a delete row must be ascending"
    keep = ~np.isin(key, dkey)
    stored, copies = np.unique(key, return_counts=True)
    at = np.minimum(np.searchsorted(stored, dkey), max(len(stored) - 1, 0))
    hits = (np.where(stored[at] == dkey, copies[at], 0) if len(stored) else
            np.zeros(len(dkey))).astype(np.int32)
    padded = np.zeros(-(-nnz // 64) * 64, np.uint8)
    padded[:nnz] = keep
    keep_bits = np.packbits(padded, bitorder="little").view(np.uint64)
    tiles = -(-nnz // T)
    tile_off = np.zeros(tiles + 1, np.int64)
    for t in range(tiles):
        tile_off[t + 1] = tile_off[t] + keep[t * T:(t + 1) * T].sum()
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    return keep_bits, tile_off, before[row_ptr_old], hits


def compact(col_old, val_old, keep_bits, new_of_old_col, n_cols_old):
    """als_csr_remove_compact: (col int32, val f32) of the kept entries, in stored order."""
    nnz = len(col_old)
    keep = np.unpackbits(np.asarray(keep_bits, np.uint64).view(np.uint8), bitorder="little")
    kept = np.nonzero(keep[:nnz])[0]
    col = np.asarray(col_old, np.int32)[kept]
    if new_of_old_col is not None:
        ok = (col >= 0) & (col < n_cols_old)
        col = np.where(ok, np.asarray(new_of_old_col, np.int32)[np.where(ok, col, 0)], -1)
    return col.astype(np.int32), np.asarray(val_old, np.float32)[kept]


def shrink(old_ids, new_ids):
    """((map, uniq, offset) of the remaining ids, new_of_old int32 [n_old] with -1 for a row
    that left, or None when none left)."""
    old_uniq = np.unique(np.asarray(old_ids, np.int64))
    mp, uniq, off = UR.index_of(new_ids)
    if len(uniq) == len(old_uniq):
        return (mp, uniq, off), None
    k = old_uniq - off
    ok = (k >= 0) & (k < len(mp))
    return (mp, uniq, off), np.where(ok, mp[np.where(ok, k, 0)], -1).astype(np.int32)


def side_inputs(old, pairs, user_side=True):
    """old: (users, items, ratings); pairs: (users, items) listed for removal.  Returns (inputs
    of the two K18 calls for the side, want): want["csr"] = the oracle's csr_build of the
    filtered triples against the oracle's index_build of the remaining ids, want["index"] =
    that index (map, uniq, offset), want["new_of_old_row"] the row map."""
    s, o = (0, 1) if user_side else (1, 0)
    ro, co = np.asarray(old[s], np.int64), np.asarray(old[o], np.int64)
    rmp0, runiq0, roff0 = UR.index_of(ro)
    cmp0, cuniq0, coff0 = UR.index_of(co)
    old_csr = O.csr_build(rmp0[ro - roff0], cmp0[co - coff0], old[2], len(runiq0))
    pr, pc = np.asarray(pairs[s], np.int64), np.asarray(pairs[o], np.int64)
    known = np.isin(pr, ro) & np.isin(pc, co)
    dr, dc = rmp0[pr[known] - roff0].astype(np.int64), cmp0[pc[known] - coff0].astype(np.int64)
    dkey = np.unique((dr << 32) | dc)                     # by row, then column: ascending rows
    row_ptr_del = np.concatenate([[0], np.cumsum(np.bincount(dkey >> 32, minlength=len(runiq0)))
                                  ]).astype(np.int64)
    col_del = (dkey & 0xFFFFFFFF).astype(np.int32)
    new = filtered(old, pairs)
    rn, cn = np.asarray(new[s], np.int64), np.asarray(new[o], np.int64)
    (rmp, runiq, roff), rmap = shrink(ro, rn)
    (cmp_, cuniq, coff), cmap = shrink(co, cn)
    want = dict(csr=O.csr_build(rmp[rn - roff], cmp_[cn - coff], new[2], len(runiq)),
                index=(rmp, runiq, roff), new_of_old_row=rmap)
    inputs = dict(row_ptr_old=old_csr[0], col_old=old_csr[1], val_old=old_csr[2],
                  row_ptr_del=row_ptr_del, col_del=col_del, n_cols_old=len(cuniq0),
                  new_of_old_col=cmap)
    return inputs, want


def row_ptr_of(row_ptr_kept, new_of_old_row):
    """The result's row pointer: row_ptr_kept of the rows that stay, plus nnz_out."""
    row_ptr_kept = np.asarray(row_ptr_kept, np.int64)
    if new_of_old_row is None:
        return row_ptr_kept
    stays = np.concatenate([np.asarray(new_of_old_row) >= 0, [True]])
    return row_ptr_kept[stays]


# ---------------------------------------------------------------- the cases
def case(name, T, seed=0):
    """(old triples, spec): spec has "pairs" (users, items) and / or "users" / "items" (whole
    rows, removed with remove_users / remove_items)."""
    kw = dict(user0=(1 << 26) + 40) if name.startswith("h_") else {}
    old, n = base(T, seed, **kw)
    u, i, _ = old
    uid, iid = np.unique(u), np.unique(i)
    (mp, _, off) = UR.index_of(u)
    (imp, _, ioff) = UR.index_of(i)
    ptr, col, _ = O.csr_build(mp[u - off], imp[i - ioff], old[2], len(uid))   # the user side
    at = lambda q: (uid[np.searchsorted(ptr, q, side="right") - 1], iid[col[q]])
    row_T1 = uid[np.nonzero(np.diff(ptr) == T + 1)[0][0]]
    pairs = lambda ps: dict(pairs=(np.asarray([p[0] for p in ps], np.int64),
                                   np.asarray([p[1] for p in ps], np.int64)))
    if name == "a_one_pair":
        return old, pairs([(row_T1, i[u == row_T1][0])])
    if name == "b_stored_duplicates":     # the item the 2T + 3 user rated most often, twice
        items, cnt = np.unique(i[u == n["ulong"]], return_counts=True)
        p = (n["ulong"], items[np.argmax(cnt)])
        return old, pairs([p, p])
    if name == "c_missing":               # unknown user, unknown item, known but unrated
        short = uid[np.nonzero(np.diff(ptr) == 2)[0][0]]
        unrated = np.setdiff1d(iid, i[u == short])[0]
        return old, pairs([(10 ** 6, iid[0]), (uid[3], 10 ** 6), (short, unrated)])
    if name == "d_user_leaves":           # a user with one rating, of a well-rated item
        one = [x for x in uid[np.diff(ptr) == 1] if x not in (n["ulo"], n["uhi"])][0]
        return old, pairs([(one, i[u == one][0])])
    if name == "e_item_leaves":
        return old, pairs([(n["ulong"], n["ionce"])])
    if name == "f_both_leave":
        return old, pairs([(n["uhi"], n["ihi"])])
    if name == "g_first_and_last_rows_leave":
        return old, pairs([(n["ulo"], n["ilo"]), (n["uhi"], n["ihi"])])
    if name == "h_offset_moves":          # the smallest user id carries the map's offset
        return old, pairs([(n["ulo"], n["ilo"])])
    if name == "h_largest_leaves":
        return old, pairs([(n["uhi"], n["ihi"])])
    if name == "i_tile_edges":
        # the last entry of tile 0 and the first of tile 1; every entry of tile 2; 260 of the
        # wide user's own items (one row's delete list longer than 256)
        ps = [at(T - 1), at(T)] + [at(q) for q in range(2 * T, 3 * T)]
        ps += [(n["uwide"], n["iwide0"] + j) for j in range(260)]
        return old, pairs(ps)
    if name == "j_whole_rows":            # the T-row user and two short ones; the top item
        row_T = uid[np.nonzero(np.diff(ptr) == T)[0][0]]
        short = uid[np.nonzero(np.diff(ptr) == 3)[0][:2]]
        items, cnt = np.unique(i, return_counts=True)
        return old, dict(users=[int(row_T)] + short.tolist(), items=[int(items[np.argmax(cnt)])])
    if name == "k_all_but_one_row":
        stay = uid[np.nonzero(np.diff(ptr) == 4)[0][0]]
        return old, dict(pairs=(u[u != stay], i[u != stay]))
    if name == "l_nothing_to_do":
        return old, pairs([])
    raise KeyError(name)
