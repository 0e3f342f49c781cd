"""CPU tests of K18 (als_csr_remove_mark / als_csr_remove_compact) and the removal path (no GPU,
nothing launched).

* remove_ref.mark / compact — drop the entries whose column is in the row's delete list, keep
  the order — is the oracle's index_build / csr_build on the filtered triples, over the case
  list the GPU tests use (remove_ref.CASES), both sides, at two tile lengths.
* The header, the library and the ctypes table agree on the new entry points; the ABI is 9.
* The argument checks of both calls run host-side and return the documented codes (small
  integers stand in for pointers; nothing is dereferenced before the checks).
* The sharded engine and a core built from saved factors refuse the removal path.
"""
import ctypes
import inspect

import numpy as np
import pytest

import remove_ref as RR
from als_mi355x import _lib, filters
from test_abi import _header_signatures, declared_functions

NAMES = ("als_csr_remove_tile", "als_csr_remove_scratch_bytes", "als_csr_remove_mark",
         "als_csr_remove_compact")


def _same(a, b):
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("T", [16, 256])
@pytest.mark.parametrize("name", RR.CASES)
def test_mark_and_compact_are_csr_build_of_the_filtered_triples(name, T):
    old, spec = RR.case(name, T)
    pairs = RR.listed(old, spec)
    info = RR.expected_info(old, pairs)
    for user_side in (True, False):
        inp, want = RR.side_inputs(old, pairs, user_side)
        keep_bits, tile_off, row_ptr_kept, hits = RR.mark(
            inp["row_ptr_old"], inp["col_old"], inp["row_ptr_del"], inp["col_del"], T)
        col, val = RR.compact(inp["col_old"], inp["val_old"], keep_bits, inp["new_of_old_col"],
                              inp["n_cols_old"])
        _same(RR.row_ptr_of(row_ptr_kept, want["new_of_old_row"]), want["csr"][0])
        _same(col, want["csr"][1])
        _same(val, want["csr"][2])
        nnz = len(inp["col_old"])
        assert tile_off[-1] == row_ptr_kept[-1] == len(col) == nnz - info["removed"]
        assert len(keep_bits) == -(-nnz // 64) and len(tile_off) == -(-nnz // T) + 1
        assert int(hits.sum()) == info["removed"]
        # a row leaves exactly when it keeps nothing, and the map is the fresh index's
        kept = np.diff(row_ptr_kept)
        m = want["new_of_old_row"]
        assert ((kept == 0).any()) == (m is not None)
        if m is not None:
            assert ((m < 0) == (kept == 0)).all()
            assert (m[m >= 0] == np.arange(len(want["index"][1]))).all()
        side = "users" if user_side else "items"
        assert (kept == 0).sum() == len(info[f"left_{side}"])


def test_cases_cover_what_they_are_named_for():
    T = 16
    left = {}
    for name in RR.CASES:
        old, spec = RR.case(name, T)
        info = RR.expected_info(old, RR.listed(old, spec))
        left[name] = (len(info["left_users"]), len(info["left_items"]))
        assert info["removed"] < len(old[0]), name
        assert (info["missing"] > 0) == (name == "c_missing"), name
    assert left["a_one_pair"] == left["b_stored_duplicates"] == left["c_missing"] == (0, 0)
    assert left["d_user_leaves"] == (1, 0) and left["e_item_leaves"] == (0, 1)
    assert left["f_both_leave"] == (1, 1) and left["g_first_and_last_rows_leave"] == (2, 2)
    assert left["l_nothing_to_do"] == (0, 0)
    old, spec = RR.case("b_stored_duplicates", T)
    pu, pi = spec["pairs"]
    assert len(pu) == 2 and pu[0] == pu[1] and pi[0] == pi[1]                 # listed twice
    assert ((old[0] == pu[0]) & (old[1] == pi[0])).sum() >= 2                 # stored twice
    assert RR.expected_info(old, spec["pairs"])["missing"] == 0
    old, spec = RR.case("c_missing", T)
    info = RR.expected_info(old, spec["pairs"])
    assert info["missing"] == 3 and info["removed"] == 0
    # the first and the last row of both sides
    old, spec = RR.case("g_first_and_last_rows_leave", T)
    info = RR.expected_info(old, spec["pairs"])
    assert info["left_users"].tolist() == [old[0].min(), old[0].max()]
    assert info["left_items"].tolist() == [old[1].min(), old[1].max()]
    # the offset and the id space follow the ids that stay
    for name, lo_moves in (("h_offset_moves", True), ("h_largest_leaves", False)):
        old, spec = RR.case(name, T)
        _, want = RR.side_inputs(old, spec["pairs"], True)
        mp0, _, off0 = RR.UR.index_of(old[0])
        mp, _, off = want["index"]
        assert off0 == old[0].min() >= 1 << 26 and len(mp) < len(mp0)
        assert (off != off0) == lo_moves
    # tile edges on the user side: entries T - 1 and T, all of tile 2, a long delete row
    old, spec = RR.case("i_tile_edges", T)
    inp, _ = RR.side_inputs(old, spec["pairs"], True)
    keep = np.unpackbits(RR.mark(inp["row_ptr_old"], inp["col_old"], inp["row_ptr_del"],
                                 inp["col_del"], T)[0].view(np.uint8), bitorder="little")
    assert not keep[T - 1] and not keep[T] and not keep[2 * T:3 * T].any()
    assert np.diff(inp["row_ptr_del"]).max() > 256
    lens = np.diff(inp["row_ptr_old"])
    assert {1, T - 1, T, T + 1, 63, 64, 65} <= set(lens.tolist())
    old, spec = RR.case("j_whole_rows", T)
    assert len(spec["users"]) == 3 and len(spec["items"]) == 1
    old, spec = RR.case("k_all_but_one_row", T)
    assert len(np.unique(RR.filtered(old, spec["pairs"])[0])) == 1
    assert len(RR.case("l_nothing_to_do", T)[1]["pairs"][0]) == 0


def test_two_removals_in_sequence_equal_one():
    old, s1 = RR.case("f_both_leave", 16)
    _, s2 = RR.case("i_tile_edges", 16)
    p1, p2 = RR.listed(old, s1), RR.listed(old, s2)
    mid = RR.filtered(old, p1)
    twice = RR.filtered(mid, p2)
    once = RR.filtered(old, tuple(np.concatenate([a, b]) for a, b in zip(p1, p2)))
    for a, b in zip(twice, once):
        np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------- ABI
def test_header_library_and_binding_agree():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    hdr = _header_signatures()
    for name in NAMES:
        assert name in declared_functions()
        assert hasattr(raw, name)
        assert hdr[name] == _lib.SIGNATURES[name][1], name
    assert _lib.SIGNATURES["als_csr_remove_mark"][0] is ctypes.c_int
    assert _lib.SIGNATURES["als_csr_remove_compact"][0] is ctypes.c_int
    assert _lib.SIGNATURES["als_csr_remove_tile"][0] is _lib.I32
    assert _lib.SIGNATURES["als_csr_remove_scratch_bytes"][0] is _lib.SZ
    assert _lib.ABI_VERSION == _lib.lib().als_abi_version() == 9
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("als_csr_remove")) == sorted(NAMES)


def test_tile_and_scratch_size():
    L = _lib.lib()
    T = L.als_csr_remove_tile()
    assert T >= 256 and T % 64 == 0
    size = L.als_csr_remove_scratch_bytes
    assert size(0, 0) >= 4 and size(-1, 5) == 0
    assert size(T, 1) == size(1, 1) >= 4 and size(T + 1, 1) >= 8
    sizes = [size(n, 7) for n in (1, 10 * T, 1000 * T, (1 << 31) - 1)]
    assert sizes == sorted(sizes) and sizes[-1] >= 4 * (((1 << 31) - 1) // T)


def test_new_names_keep_clear_of_the_workspace_registry():
    for name in _lib.SIGNATURES:
        if name.startswith("als_csr_remove"):
            assert not name.endswith("_workspace_bytes")


def test_every_csr_remove_size_function_has_a_bounds_case():
    import test_gpu_remove_bounds as BB
    sizers = sorted(n for n in _lib.SIGNATURES
                    if n.startswith("als_csr_remove_") and n.endswith("_bytes"))
    assert sizers == sorted(BB.SCRATCH_CASES)
    for name, tests in BB.SCRATCH_CASES.items():
        assert tests
        for t in tests:
            assert callable(getattr(BB, t, None)), f"{name}: {t} is not a test of the bounds file"


def _mark(**over):
    a = dict(row_ptr_old=8, col_old=4, nnz_old=5, n_old=2, row_ptr_del=8, col_del=4, nnz_del=2,
             keep_bits=8, tile_off=8, row_ptr_kept=8, del_hits=0, scratch=8, scratch_bytes=256,
             stream=0)
    a.update(over)
    return _lib.lib().als_csr_remove_mark(*a.values())


@pytest.mark.parametrize("over,code", [
    (dict(nnz_old=-1), -1), (dict(nnz_del=-1), -1), (dict(n_old=-1), -1),
    (dict(row_ptr_old=0), -1), (dict(col_old=0), -1), (dict(keep_bits=0), -1),
    (dict(tile_off=0), -1), (dict(row_ptr_kept=0), -1),
    (dict(row_ptr_del=0), -1), (dict(col_del=0), -1), (dict(scratch=0), -1),
    (dict(scratch_bytes=3), -2),
    (dict(nnz_old=1 << 31), -4), (dict(n_old=0x7fffffff), -4)])
def test_mark_argument_errors_before_any_device_call(over, code):
    assert _mark(**over) == code, over
    assert b"als_csr_remove_mark" in _lib.lib().als_last_error()


def _compact(**over):
    a = dict(col_old=4, val_old=4, nnz_old=5, keep_bits=8, tile_off=8, col_map=4, n_cols_old=3,
             col_out=4, val_out=4, nnz_out=4, stream=0)
    a.update(over)
    return _lib.lib().als_csr_remove_compact(*a.values())


@pytest.mark.parametrize("over,code", [
    (dict(nnz_old=-1), -1), (dict(nnz_out=-1), -1), (dict(n_cols_old=-1), -1),
    (dict(nnz_out=6), -1),                                     # entries only leave
    (dict(col_old=0), -1), (dict(val_old=0), -1), (dict(keep_bits=0), -1),
    (dict(tile_off=0), -1), (dict(col_out=0), -1), (dict(val_out=0), -1),
    (dict(nnz_old=1 << 31), -4)])
def test_compact_argument_errors_before_any_device_call(over, code):
    assert _compact(**over) == code, over
    assert b"als_csr_remove_compact" in _lib.lib().als_last_error()


def test_nothing_kept_needs_no_output_and_launches_nothing():
    assert _compact(nnz_out=0, col_out=0, val_out=0) == 0


# ---------------------------------------------------------------- Python layer
def test_sharded_engine_refuses_the_removal_path():
    from als_mi355x.distributed import ShardedALS
    from als_mi355x.engine import ALSCore
    with pytest.raises(NotImplementedError, match="single-GPU engine"):
        filters.reject_sharded_remove()
    for name, args in (("remove_ratings", ([1], [2])), ("remove_users", ([1],)),
                       ("remove_items", ([1],)), ("set_ratings", ([1], [2], [3.0]))):
        with pytest.raises(NotImplementedError, match="single-GPU engine"):
            getattr(ShardedALS, name)(None, *args)
        sharded = inspect.signature(getattr(ShardedALS, name))
        single = inspect.signature(getattr(ALSCore, name))
        assert list(sharded.parameters) == list(single.parameters)
        for p in single.parameters.values():
            assert sharded.parameters[p.name].kind is p.kind
            assert sharded.parameters[p.name].default == p.default


def test_a_core_without_ratings_says_so():
    from als_mi355x.engine import ALSCore
    core = ALSCore.__new__(ALSCore)
    core.user_block = core.item_block = None
    for call in (lambda: core.remove_ratings([1], [2]), lambda: core.remove_users([1]),
                 lambda: core.remove_items([1]), lambda: core.set_ratings([1], [2], [3.0])):
        with pytest.raises(ValueError, match="from_factors"):
            call()


def test_models_check_their_mode_first():
    from als_mi355x.ml.recommendation import ALSModel
    from als_mi355x.mllib.recommendation import MatrixFactorizationModel
    ml, mllib = ALSModel(None, {}), MatrixFactorizationModel(None)
    for call in (lambda: ml.remove({}, mode="retrain"), lambda: ml.removeUsers([1], mode="x"),
                 lambda: ml.removeItems([1], mode="x"),
                 lambda: ml.update({}, mode="x", replace=True),
                 lambda: mllib.remove([(1, 2)], mode="x"), lambda: mllib.removeUsers([1], mode="x"),
                 lambda: mllib.removeProducts([1], mode="x"),
                 lambda: mllib.update([(1, 2, 3.0)], mode="x", replace=True)):
        with pytest.raises(ValueError, match="mode must be"):
            call()
    with pytest.raises(ValueError, match="iterations"):
        mllib.remove([(1, 2)], -1)


def test_personal_update_takes_replace():
    from als_mi355x import personal
    sig = inspect.signature(personal.personal_recommendations_update)
    assert sig.parameters["replace"].default is False
