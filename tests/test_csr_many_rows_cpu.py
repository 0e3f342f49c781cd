"""CPU tests of many_rows_ref.py (no GPU, nothing launched): every shape built for
test_gpu_csr_many_rows.py has the property that makes it reach its path of K17 / K18 / K20, the
constants the shapes are built from are the ones in the sources, and every vectorised
restatement equals the brute-force one (split_ref.Split, remove_ref.mark / compact) on the
existing small cases and, where the brute-force one is quick enough, on the new shapes too.
"""
import time

import numpy as np
import pytest

import grid_caps as GC
import many_rows_ref as MR
import remove_ref as RR
import split_ref as SR
import update_ref as UR
from als_mi355x import _lib
from helpers import report
from test_gpu_split import SHAPES, WINDOWS, _shape


def _T():
    L = _lib.lib()
    assert L.als_csr_merge_tile() == L.als_csr_remove_tile()
    return L.als_csr_remove_tile()


def _max_empty_run(lens):
    best = run = 0
    for n in np.asarray(lens).tolist():
        run = run + 1 if n == 0 else 0
        best = max(best, run)
    return best


# ---------------------------------------------------------------- constants
def test_constants_are_the_sources():
    split, compact = GC._source("split.hip"), GC._source("csr_compact.h")
    walk = GC._source("csr_tile_walk.h")   # the one geometry of the K17, K18 and K20 tiles
    assert GC.read_constant(split, "kSplitTask", "csrc/split.hip") == MR.TASK
    assert GC.read_constant(split, "kSplitLongGrid", "csrc/split.hip") == MR.LONG_GRID
    assert GC.read_constant(walk, "kTileThreads", "csrc/csr_tile_walk.h") == MR.BATCH
    for name in ("csr_merge.hip", "csr_remove.hip", "split.hip"):   # and no copy of it
        assert "__launch_bounds__(kTileThreads)" in GC._source(name), name
    assert (GC.read_constant(compact, "kScanThreads", "csrc/csr_compact.h")
            * GC.read_constant(compact, "kScanItems", "csrc/csr_compact.h")) == MR.SCAN_TRIP
    T = _T()
    assert T > MR.BATCH and T % MR.BATCH == 0 and T == MR.TASK   # a tile can meet T rows
    assert _lib.lib().als_split_row_cap() >= 64


# ---------------------------------------------------------------- S1 - S3, S7: the row walk
def test_ones_meets_a_tile_of_rows_in_eight_batches():
    T = _T()
    old = MR.ones(T)
    row_ptr, _ = MR.user_csr(old)
    assert len(row_ptr) - 1 == 3 * T + 17 and (np.diff(row_ptr) == 1).all()
    w = MR.walk(row_ptr, T)
    assert [len(x["trips"]) for x in w] == [T // MR.BATCH] * 3 + [1] and T // MR.BATCH == 8
    assert all(s - d == MR.BATCH for x in w[:3] for _, d, s in x["trips"])
    assert (np.diff(np.unique(old[0])) == 3).all()                # new ids fit in every gap
    assert not (np.diff(old[0]) >= 0).all()                       # shuffled
    assert (old[2] * 2 == np.round(old[2] * 2)).all() and old[2].dtype == np.float32
    # the batches: (a) reaches every row batch of every full tile, (b) makes whole batches of
    # batch-only rows and a row map of more than 6000 entries, (c) brings new columns
    a = MR.batch(old, "a_no_new_id")
    rows = np.searchsorted(np.unique(old[0]), a[0])
    assert set((rows // MR.BATCH).tolist()) >= set(range(3 * T // MR.BATCH))
    assert len(np.setdiff1d(a[0], old[0])) == 0 and len(np.setdiff1d(a[1], old[1])) == 0
    inp, _ = UR.side_inputs(old, MR.batch(old, "b_new_rows"), True)
    m = inp["new_of_old_row"]
    assert len(m) > 6000 and (np.diff(m) == 2).all() and m[0] == 1
    assert len(inp["row_ptr_add"]) - 1 == m[-1] + 1 + 300 > 40 * MR.BATCH   # several workgroups
    assert inp["new_of_old_col"] is None
    inp, _ = UR.side_inputs(old, MR.batch(old, "c_new_cols"), True)
    assert inp["new_of_old_row"] is None and inp["new_of_old_col"] is not None
    assert inp["new_of_old_col"][0] == 2 and (np.diff(inp["new_of_old_col"]) > 0).all()
    assert len(MR.batch(old, "d_empty")[0]) == 0


def test_seams_put_long_rows_on_both_sides_of_a_batch_seam():
    T = _T()
    lens = MR.seams_lens(T)
    old = MR.seams(T)
    row_ptr, _ = MR.user_csr(old)
    assert (np.diff(row_ptr) == lens).all() and 1000 <= len(lens) <= 1300
    assert set(lens.tolist()) == {1, 2, T - 1, T + 5, 2 * T + 3}
    w = MR.walk(row_ptr, T)
    last, first, whole = [], [], []
    for t, x in enumerate(w):
        for r in range(x["row0"], min(x["row0"] + 3 * MR.BATCH, len(lens))):
            if lens[r] >= T - 1 and row_ptr[r] < (t + 1) * T and row_ptr[r + 1] > t * T:
                (last if (r - x["row0"]) % MR.BATCH == MR.BATCH - 1 else
                 first if (r - x["row0"]) == MR.BATCH else whole).append((t, r))
    assert last and first, (last, first)
    # the long row that is first of a batch is reached in the tile's SECOND trip
    t, r = first[0]
    assert len(w[t]["trips"]) == 2 and w[t]["trips"][1][0] == r
    # a row holds a whole tile: that tile's search lands on it and it ends the only batch
    spans = [t for t, x in enumerate(w) if row_ptr[x["row0"]] <= t * T
             and row_ptr[x["row0"] + 1] >= (t + 1) * T]
    assert spans and all(len(w[t]["trips"]) == 1 for t in spans)
    seam = MR.seam_rows(row_ptr, T)
    assert {r for _, r in last + first} <= set(seam.tolist())
    for kind in MR.DELETES:
        pu, pi = MR.delete_pairs(old, kind, T)
        if kind == "every_5th":
            assert len(np.unique(pu)) == len(pu) == -(-len(lens) // 5)
        if kind == "seam_rows":     # every entry of the rows on a seam, long ones included
            assert set(np.unique(pu).tolist()) == set(np.unique(old[0])[seam].tolist())
            assert len(pu) == lens[seam].sum() > 2 * T
        if kind == "nothing":
            assert len(pu) == 0


@pytest.mark.parametrize("front_empty", [False, True])
def test_gaps_have_batches_of_empty_rows(front_empty):
    T = _T()
    lens = MR.gaps_lens(front_empty)
    assert _max_empty_run(lens) == 600 and (lens[-300:] == 0).all() and (lens > 0).sum() == 80
    assert (lens[:300] == 0).all() == front_empty
    ptr, col, val = MR.gaps_csr(front_empty)
    assert (np.diff(ptr) == lens).all() and ptr[-1] == len(col) == len(val)
    w = MR.walk(ptr, T)
    assert len(w) == 1 and w[0]["row0"] == (300 if front_empty else 0)
    assert [s - d for _, d, s in w[0]["trips"]] == [120, 0, 120]        # stop == done once
    # K17: the rows stay empty (neither old nor batch entries) in (a), (c) and (d)
    for kind in MR.BATCHES:
        inp = MR.gaps_merge_inputs(kind, front_empty)
        got = UR.merge(inp["row_ptr_old"], inp["col_old"], inp["val_old"], inp["new_of_old_row"],
                       inp["new_of_old_col"], inp["row_ptr_add"], inp["col_add"], inp["val_add"])
        assert got[0][-1] == len(inp["col_old"]) + len(inp["col_add"])
        if kind == "b_new_rows":
            m = inp["new_of_old_row"]
            assert (np.diff(m) >= 1).all() and m[0] == 1 and len(got[0]) - 1 == m[-1] + 301
            assert (np.diff(got[0])[m[-1] + 1:] == 1).all()              # 300 rows of the batch
        else:
            assert _max_empty_run(np.diff(got[0])) >= 2 * MR.BATCH
            assert any(s == d for x in MR.walk(got[0], T) for _, d, s in x["trips"])
        assert (inp["new_of_old_col"] is not None) == (kind == "c_new_cols")
    for kind in MR.DELETES:
        inp = MR.gaps_remove_inputs(kind, front_empty)
        d = np.diff(inp["row_ptr_del"])
        assert (d[lens == 0] == 0).all() and (d > 0).sum() == dict(every_5th=16, seam_rows=4,
                                                                   nothing=0)[kind]
    kw = MR.gaps_split(front_empty)
    sp = MR.FastSplit(seed=MR.SEED, keep_items=False, mode="count", value=1, **kw)
    assert (np.diff(sp.side(True)[0]) == lens).all()


def test_carry_takes_two_trips_of_the_scan():
    T = _T()
    t0 = time.perf_counter()
    c = MR.carry(T)
    report("csr_many_rows_host_s::carry_inputs_and_restatement", time.perf_counter() - t0)
    ptr, tiles = c["row_ptr_old"], len(c["tile_off"]) - 1
    assert tiles == MR.SCAN_TRIP + 2 and ptr[-1] == MR.SCAN_TRIP * T + T + 5
    assert len(ptr) - 1 == 70 and len(set(np.diff(ptr).tolist())) > 30          # uneven
    edge = MR.SCAN_TRIP * T
    assert edge - 3 in ptr and edge + 2 in ptr and edge not in ptr
    cnt = np.diff(c["tile_off"])
    assert len(set(cnt[:MR.SCAN_TRIP].tolist())) > 10 and cnt[-1] <= 5 < cnt[-2]
    assert c["tile_off"][MR.SCAN_TRIP] not in (0, c["tile_off"][-1])            # a true carry
    assert c["tile_off"][-1] == len(c["col"]) == c["row_ptr_kept"][-1] < ptr[-1]
    assert (np.diff(c["row_ptr_del"]) == np.arange(70) % 2).all() and (c["col_del"] == 3).all()
    assert c["del_hits"].sum() == ptr[-1] - len(c["col"]) and (c["del_hits"] > 0).all()


def test_the_carry_restatement_is_remove_ref_at_a_small_tile():
    """carry() at T = 16 is small enough for remove_ref.mark / compact (a Python loop per tile):
    the same code at the library's T is what the GPU test compares with."""
    T = 16
    c = MR.carry(T)
    kb, to, rk, hits = RR.mark(c["row_ptr_old"], c["col_old"], c["row_ptr_del"], c["col_del"], T)
    col, val = RR.compact(c["col_old"], c["val_old"], kb, None, 7)
    for name, want in (("keep_bits", kb), ("tile_off", to), ("row_ptr_kept", rk),
                       ("del_hits", hits), ("col", col), ("val", val)):
        assert c[name].dtype == want.dtype and c[name].tobytes() == want.tobytes(), name
    assert len(to) == MR.SCAN_TRIP + 3


@pytest.mark.parametrize("T", [16, 2048])
def test_keep_format_is_remove_ref_mark(T):
    old, spec = RR.case("i_tile_edges", T)
    inp, _ = RR.side_inputs(old, RR.listed(old, spec), True)
    kb, to, rk, _ = RR.mark(inp["row_ptr_old"], inp["col_old"], inp["row_ptr_del"],
                            inp["col_del"], T)
    keep = np.unpackbits(kb.view(np.uint8), bitorder="little")[:len(inp["col_old"])].astype(bool)
    for g, w in zip(MR.keep_format(keep, inp["row_ptr_old"], T), (kb, to, rk)):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()


# ---------------------------------------------------------------- S4 - S6: K20's shapes
def test_two_long_rows_share_an_anchor_tile_and_one_starts_on_a_tile_edge():
    kw, rows = MR.two_long()
    ent = MR.item_rows(kw, rows.values())
    span = {k: (int(ent[r][0][0]), int(ent[r][0][-1]) + 1) for k, r in rows.items()}
    P = MR.TWO_LONG
    assert span["A"] == (300, 300 + MR.TASK + 700) and span["B"][0] == span["A"][1]
    assert span["B"][1] - span["B"][0] == MR.TASK + 9
    assert span["C"][0] % MR.TASK == 0 and span["C"][1] - span["C"][0] == 2 * MR.TASK + 1
    assert all(b - a > MR.TASK for a, b in span.values())
    # tile 1 holds a part of A and a part of B: both of its slots are written and read
    assert span["A"][0] < MR.TASK < span["A"][1] < 2 * MR.TASK
    assert MR.TASK < span["B"][0] < 2 * MR.TASK < span["B"][1]
    for r in rows.values():
        assert len(np.unique(ent[r][3])) == len(ent[r][3])         # columns distinct in a row
    sp = MR.FastSplit(seed=MR.SEED, **kw)
    lens = np.diff(sp.side(False)[0])
    assert (lens > MR.TASK).sum() == 3 and np.median(lens) <= 5 and P["n_users"] >= lens.max()
    assert not (np.diff(kw["items"]) >= 0).all()
    # the planted seed: every long row's smallest composite lies in the tile in question, once
    seed = MR.two_long_seed(kw, rows)
    assert seed != MR.SEED
    at = {k: MR.item_row_min(ent[r], seed) for k, r in rows.items()}
    assert at["A"][0] // MR.TASK == 1 == at["B"][0] // MR.TASK
    assert at["C"][0] // MR.TASK == span["C"][0] // MR.TASK
    assert all(x[1] == 1 for x in at.values())
    planted = MR.FastSplit(seed=seed, **kw)
    for k, r in rows.items():
        assert planted.uids[planted.anchor[r]] == at[k][2]


def test_long65_has_its_minimum_past_the_64th_tile():
    kw, row, planted = MR.long65()
    at = MR.item_rows(kw, [row])[row]
    P = MR.LONG65
    assert at[0][0] == P["start"] and len(at[0]) == P["length"] == 65 * MR.TASK + 77
    first, last = int(at[0][0]) // MR.TASK, int(at[0][-1]) // MR.TASK
    assert (first, last) == (0, 65) and last - first + 1 > 64        # a second step of the lanes
    assert sorted(planted) == [64, last]
    assert len(np.unique(kw["users"])) <= P["catalogue"]
    sp = None
    for tile, user in planted.items():
        seed = MR.long65_seed(kw, row, user)
        pos, copies, who = MR.item_row_min(at, seed)
        assert (pos // MR.TASK, copies, who) == (tile, 1, user)
        sp = MR.FastSplit(seed=seed, **kw)
        assert sp.uids[sp.anchor[row]] == user
    assert len(sp.iids) <= 40 and len(sp.uids) <= P["catalogue"]


def test_many_listed_lists_more_rows_than_workgroups():
    kw = MR.many_listed()
    sp = MR.FastSplit(seed=MR.SEED, keep_items=False, **kw)
    lens = np.diff(sp.side(True)[0])
    assert len(lens) == 2 * MR.LONG_GRID + 37 and lens.min() == 2 and lens.max() == 5
    n_long = int((lens > 1).sum())                                   # row_cap = 1
    assert n_long > MR.LONG_GRID and -(-n_long // MR.LONG_GRID) == 3
    # consecutive rows of one workgroup (j, j + 2048, j + 4096 whatever the list's order: the
    # windows differ wherever the lengths do) and copies on a window edge
    for name in ("fold1of3", "last"):
        w = WINDOWS[name]
        sp.set_windows(w.get("mode"), w.get("value"), w.get("min_keep", 1), w.get("win"))
        assert len(set(zip(sp.lo.tolist(), sp.hi.tolist()))) >= 3
        thr = sp.thresholds()
        straddle = 0
        for r in np.nonzero(np.arange(len(lens)) % 3 == 0)[0][:50]:
            mine = sp.sel == r
            assert len(set(sp.keys[mine].tolist())) == 1             # copies of one pair
            # a rank inside the copies: the threshold is the end composite
            straddle += int(any(0 < k[r] < lens[r] and thr[w][r] == SR.KEY_END
                                for w, k in ((0, sp.lo), (2, sp.hi))))
        assert straddle >= 10, name


# ---------------------------------------------------------------- FastSplit is split_ref.Split
def _same_split(fast, brute, T):
    for name in ("keys", "eligible", "rank", "held", "e", "lo", "hi", "anchor"):
        a, b = getattr(fast, name), getattr(brute, name)
        assert (a is None) == (b is None), name
        if a is not None:
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    for a, b in zip(fast.thresholds(), brute.thresholds()):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    for user_rows in (True, False):
        for a, b in zip(fast.marks(user_rows, T), brute.marks(user_rows, T)):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("user_side", [True, False])
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_fast_split_equals_the_brute_force_one_on_the_existing_shapes(shape, keep, user_side):
    kw = _shape(shape)
    fast = MR.FastSplit(seed=MR.SEED, keep_items=keep, user_side=user_side, **kw)
    brute = SR.Split(seed=MR.SEED, keep_items=keep, user_side=user_side, **kw)
    for w in WINDOWS.values():
        for sp in (fast, brute):
            sp.set_windows(w.get("mode"), w.get("value"), w.get("min_keep", 1), w.get("win"))
        _same_split(fast, brute, _T())


@pytest.mark.parametrize("user_side", [True, False])
@pytest.mark.parametrize("shape", ["two_long", "long65", "many_listed", "gaps", "seams"])
def test_fast_split_equals_the_brute_force_one_on_the_new_shapes(shape, user_side):
    """split_ref.Split takes under a second on each of these on a desktop CPU (the figures go to
    the test report), so the new shapes are pinned directly as well."""
    kw = {"two_long": lambda: MR.two_long()[0], "long65": lambda: MR.long65()[0],
          "many_listed": MR.many_listed, "gaps": MR.gaps_split,
          "seams": lambda: dict(zip(("users", "items"), MR.seams(_T())[:2]))}[shape]()
    t0 = time.perf_counter()
    fast = MR.FastSplit(seed=MR.SEED, user_side=user_side, **kw)
    t1 = time.perf_counter()
    brute = SR.Split(seed=MR.SEED, user_side=user_side, **kw)
    t2 = time.perf_counter()
    report(f"csr_many_rows_host_s::split_ref[{shape}-{user_side}]", {"fast": t1 - t0,
                                                                    "brute": t2 - t1})
    for name in ("fold1of3", "last"):
        w = WINDOWS[name]
        for sp in (fast, brute):
            sp.set_windows(w.get("mode"), w.get("value"), w.get("min_keep", 1), w.get("win"))
        _same_split(fast, brute, _T())
