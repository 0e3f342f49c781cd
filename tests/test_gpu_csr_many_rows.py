"""GPU tests of the paths of K17 (als_csr_merge), K18 (als_csr_remove_mark / _compact) and K20
(als_split_*) that the ~40-row shapes of test_gpu_update.py, test_gpu_remove.py and
test_gpu_split.py never reach (shapes: many_rows_ref.py, held to their properties by
test_csr_many_rows_cpu.py):

  the row walk taking 2 to 8 batches of 256 rows in a tile, long rows on a batch seam, batches
  of rows without an entry (stop == done)                       ones / seams / gaps on K17, K18, K20
  merge_row_ptr_kernel over several workgroups and a lower bound over 6000 rows    K17 b_new_rows
  the scan's carry between two trips of 4096 tile counts                             K18 on carry
  two long rows in one anchor tile (slots 2t and 2t + 1), a long row starting on a tile edge
                                                                                     K20 two_long
  a long row over more than 64 anchor tiles                                          K20 long65
  more listed rows than workgroups of split_thr_long_kernel                K20 many_listed, cap 1

The bar everywhere is bit equality with a numpy restatement (integers and copied f32 bits).
"""
import time

import numpy as np
import pytest
import torch

import many_rows_ref as MR
import remove_ref as RR
import update_ref as UR
from als_mi355x import engine as E
from helpers import report
from test_gpu_split import CAP, WINDOWS, _expected, _kernels
from test_gpu_update import _assert_same_ratings, _cat

pytestmark = pytest.mark.gpu
DEV = "cuda"
_CACHE = {}


def _T():
    assert E.csr_merge_tile() == E.csr_remove_tile()
    return E.csr_remove_tile()


def _dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _old(shape):
    return _cached(shape, lambda: getattr(MR, shape)(_T()))


@pytest.fixture(autouse=True)
def _wall_time(request):
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    report(f"csr_many_rows_wall_s::{request.node.name}", time.perf_counter() - t0)


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got.view(np.int32 if got.itemsize == 4 else np.int64)
                         != want.view(np.int32 if want.itemsize == 4 else np.int64))[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} differ, first at {bad[:8]}")


# ---------------------------------------------------------------- K17
def _merge(inp):
    t = {k: _dev(v) for k, v in inp.items() if k != "n_cols_old"}
    got = E.merge_csr(t["row_ptr_old"], t["col_old"], t["val_old"], inp["n_cols_old"],
                      t["new_of_old_row"], t["new_of_old_col"], t["row_ptr_add"], t["col_add"],
                      t["val_add"])
    torch.cuda.synchronize()
    return got


def _merge_ref(inp):
    return UR.merge(inp["row_ptr_old"], inp["col_old"], inp["val_old"], inp["new_of_old_row"],
                    inp["new_of_old_col"], inp["row_ptr_add"], inp["col_add"], inp["val_add"])


@pytest.mark.parametrize("user_side", [True, False])
@pytest.mark.parametrize("kind", MR.BATCHES)
@pytest.mark.parametrize("shape", ["ones", "seams"])
def test_merge_on_many_rows(shape, kind, user_side):
    old = _old(shape)
    inp, want = UR.side_inputs(old, MR.batch(old, kind), user_side)
    if kind == "d_empty":
        assert inp["new_of_old_row"] is None and inp["new_of_old_col"] is None
    got = _merge(inp)
    for g, r, w, name in zip(got, _merge_ref(inp), want, ("row_ptr", "col", "val")):
        _same(g, r, (name, "update_ref.merge"))
        _same(g, w, (name, "csr_build of the concatenation"))


@pytest.mark.parametrize("front_empty", [False, True])
@pytest.mark.parametrize("kind", MR.BATCHES)
def test_merge_on_batches_of_empty_rows(kind, front_empty):
    inp = MR.gaps_merge_inputs(kind, front_empty)
    for g, r, name in zip(_merge(inp), _merge_ref(inp), ("row_ptr", "col", "val")):
        _same(g, r, name)


@pytest.mark.parametrize("shape", ["ones", "seams"])
def test_add_ratings_on_many_rows_gives_the_blocks_of_a_fresh_core(shape):
    old = _old(shape)
    add = _cat(MR.batch(old, "b_new_rows"), MR.batch(old, "c_new_cols"))
    core = E.ALSCore(*old)
    info = core.add_ratings(*add)
    assert info["added"] == len(add[0])
    _assert_same_ratings(core, E.ALSCore(*_cat(old, add)))


# ---------------------------------------------------------------- K18
def _remove(inp):
    """Both K18 calls: (keep_bits, tile_off, row_ptr_kept, del_hits, col, val) as numpy."""
    t = {k: _dev(v) for k, v in inp.items() if k != "n_cols_old"}
    ws = E.Workspace(torch.device(DEV))
    nothing = len(inp["col_del"]) == 0
    kb, to, rk, hits = E.remove_mark(t["row_ptr_old"], t["col_old"],
                                     None if nothing else t["row_ptr_del"],
                                     None if nothing else t["col_del"], ws, count_hits=True)
    col, val = E.remove_compact(t["col_old"], t["val_old"], kb, to, t.get("new_of_old_col"),
                                inp["n_cols_old"], int(to[-1]))
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (kb, to, rk, hits, col, val)]


def _remove_ref(inp, T):
    kb, to, rk, hits = RR.mark(inp["row_ptr_old"], inp["col_old"], inp["row_ptr_del"],
                               inp["col_del"], T)
    col, val = RR.compact(inp["col_old"], inp["val_old"], kb, inp.get("new_of_old_col"),
                          inp["n_cols_old"])
    return [kb.view(np.int64), to, rk, hits, col, val]


_K18_NAMES = ("keep_bits", "tile_off", "row_ptr_kept", "del_hits", "col", "val")


@pytest.mark.parametrize("user_side", [True, False])
@pytest.mark.parametrize("kind", MR.DELETES)
@pytest.mark.parametrize("shape", ["ones", "seams"])
def test_remove_on_many_rows(shape, kind, user_side):
    T = _T()
    old = _old(shape)
    inp, want = RR.side_inputs(old, MR.delete_pairs(old, kind, T), user_side)
    got = _remove(inp)
    for g, r, name in zip(got, _remove_ref(inp, T), _K18_NAMES):
        _same(g, r, name)
    _same(RR.row_ptr_of(got[2], want["new_of_old_row"]), want["csr"][0], "row_ptr of csr_build")
    _same(got[4], want["csr"][1], "col of csr_build")
    _same(got[5], want["csr"][2], "val of csr_build")
    if kind == "nothing":
        _same(got[2], inp["row_ptr_old"], "row_ptr_kept of a plain copy")


@pytest.mark.parametrize("front_empty", [False, True])
@pytest.mark.parametrize("kind", MR.DELETES)
def test_remove_on_batches_of_empty_rows(kind, front_empty):
    inp = MR.gaps_remove_inputs(kind, front_empty)
    for g, r, name in zip(_remove(inp), _remove_ref(inp, _T()), _K18_NAMES):
        _same(g, r, name)


def test_remove_ratings_on_seams_gives_the_blocks_of_a_fresh_core():
    T = _T()
    old = _old("seams")
    pairs = _cat(MR.delete_pairs(old, "every_5th", T), MR.delete_pairs(old, "seam_rows", T))
    core = E.ALSCore(*old)
    info = core.remove_ratings(*pairs)
    new = RR.filtered(old, pairs)
    assert info["removed"] == len(old[0]) - len(new[0]) > 2 * T and info["missing"] == 0
    _assert_same_ratings(core, E.ALSCore(*new))


def test_the_scan_carries_over_4096_tiles():
    T = _T()
    c = _cached("carry", lambda: MR.carry(T))
    inp = {k: c[k] for k in ("row_ptr_old", "col_old", "val_old", "row_ptr_del", "col_del")}
    inp["n_cols_old"] = 7
    first = _remove(inp)
    assert len(first[1]) == MR.SCAN_TRIP + 3
    for g, name in zip(first, _K18_NAMES):
        want = c[name].view(np.int64) if name == "keep_bits" else c[name]
        _same(g, want, name)
    for a, b, name in zip(first, _remove(inp), _K18_NAMES):
        assert a.tobytes() == b.tobytes(), (name, "two calls differ")


# ---------------------------------------------------------------- K20
def _split_case(shape):
    """(Split's keyword arguments, {name: seed})."""
    if shape == "seams":
        return dict(zip(("users", "items"), _old("seams")[:2])), {"seed": MR.SEED}
    if shape in ("gaps", "gaps_front"):
        return MR.gaps_split(shape == "gaps_front"), {"seed": MR.SEED}
    if shape == "many_listed":
        return MR.many_listed(), {"seed": MR.SEED}
    if shape == "two_long":
        kw, rows = MR.two_long()
        return kw, {"seed": MR.SEED, "minima_in_the_shared_tile": MR.two_long_seed(kw, rows)}
    if shape == "long65":
        kw, row, planted = MR.long65()
        return kw, {f"minimum_in_tile_{t}": MR.long65_seed(kw, row, u) for t, u in planted.items()}
    raise KeyError(shape)


SPLIT_SHAPES = {"seams": (False,), "gaps": (False,), "gaps_front": (False,),
                "many_listed": (False, True), "two_long": (True,), "long65": (True,)}
SPLIT_WINDOWS = ("fold1of3", "last", "fraction")


@pytest.mark.parametrize("user_side", [True, False])
@pytest.mark.parametrize("shape,keep", [(s, k) for s, ks in SPLIT_SHAPES.items() for k in ks])
def test_split_kernels_on_many_rows(shape, keep, user_side):
    kw, seeds = _cached(("split", shape), lambda: _split_case(shape))
    caps = (CAP, 0) + ((1,) if shape == "many_listed" else ())
    for seed in seeds.values():
        sp = MR.FastSplit(seed=seed, keep_items=keep, user_side=user_side, **kw)
        for name in SPLIT_WINDOWS:
            w = WINDOWS[name]
            sp.set_windows(w.get("mode"), w.get("value"), w.get("min_keep", 1), w.get("win"))
            want = _expected(sp)
            runs = [_kernels(sp, cap, seed) for cap in caps]
            assert sorted(runs[0]) == sorted(want)
            for k in want:
                _same(runs[0][k], want[k], (name, k, seed))
                for cap, other in zip(caps[1:], runs[1:]):
                    assert other[k].tobytes() == runs[0][k].tobytes(), (name, k, "row_cap", cap)
            assert runs[0]["tile_off1"][-1] == runs[0]["tile_off0"][-1] == int((~sp.held).sum())
