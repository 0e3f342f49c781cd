"""CPU tests of K17 (als_csr_merge) and the update path (no GPU, nothing launched).

* update_ref.merge — per row, the old segment with renumbered columns, then the batch's — is
  the oracle's index_build / csr_build on the concatenation, over the case list the GPU tests
  use (update_ref.CASES), both sides, at two tile lengths.
* The header, the library and the ctypes table agree on the new entry points.
* als_csr_merge's argument checks run host-side and return the documented codes (small integers
  stand in for pointers; nothing is dereferenced before the checks).  The call takes no
  scratch, so there is no size function and no ALS_EWORKSPACE path; the test that every
  als_csr_merge_*_bytes has a bounds case holds that to the bounds file.
* The sharded engine and a core built from saved factors refuse add_ratings / refresh / refit.
"""
import ctypes
import inspect

import numpy as np
import pytest

import update_ref as UR
from als_mi355x import _lib, filters
from test_abi import _header_signatures, declared_functions

NAMES = ("als_csr_merge", "als_csr_merge_tile")


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("T", [16, 256])
@pytest.mark.parametrize("name", UR.CASES)
def test_merge_is_csr_build_of_the_concatenation(name, T):
    old, add = UR.case(name, T)
    for user_side in (True, False):
        inp, want = UR.side_inputs(old, add, user_side)
        got = UR.merge(inp["row_ptr_old"], inp["col_old"], inp["val_old"], inp["new_of_old_row"],
                       inp["new_of_old_col"], inp["row_ptr_add"], inp["col_add"], inp["val_add"])
        for g, w in zip(got, want):
            assert g.dtype == w.dtype
            np.testing.assert_array_equal(g.view(np.int32) if g.dtype == np.float32 else g,
                                          w.view(np.int32) if w.dtype == np.float32 else w)
        m = inp["new_of_old_row"]
        if m is not None:
            assert (np.diff(m) > 0).all() and m[-1] < len(want[0]) - 1


def test_cases_cover_what_they_are_named_for():
    T = 16
    for name in UR.CASES:
        old, add = UR.case(name, T)
        assert 1 <= len(add[0]) <= 96, name
        news = [len(np.setdiff1d(add[s], old[s])) for s in (0, 1)]
        offs = [(UR.index_of(old[s])[2], UR.index_of(np.concatenate([old[s], add[s]]))[2])
                for s in (0, 1)]
        if name[0] in "adefg":
            assert news == [0, 0], name
        if name == "b_new_users":
            assert news[0] >= 3 and news[1] == 0
        if name == "b_new_items":
            assert news[1] >= 3 and news[0] == 0
        if name == "b_new_both":
            assert min(news) >= 3
        if name.startswith("c_"):
            assert offs[0][0] != offs[0][1], name      # the user offset moves
        else:
            assert offs[0][0] == offs[0][1] == 0
    lens = UR.row_lengths(T)
    assert {1, T - 1, T, T + 1, 2 * T + 3} <= set(lens) and 35 <= len(lens) <= 45
    old, add = UR.case("d_duplicates", T)
    pairs = list(zip(add[0].tolist(), add[1].tolist()))
    assert len(set(pairs)) < len(pairs)                                   # twice in the batch
    assert (int(old[0][0]), int(old[1][0])) in pairs                      # already rated
    old, add = UR.case("g_every_row", T)
    assert set(np.unique(old[0])) <= set(add[0]) and set(np.unique(old[1])) <= set(add[1])
    assert len(UR.case("f_one", T)[1][0]) == 1


def test_two_merges_in_sequence_equal_one():
    """(h): merging batch 1 and then batch 2 is merging their concatenation."""
    old, a1 = UR.case("b_new_both", 16)
    _, a2 = UR.case("c_negative", 16)
    cat = lambda x, y: tuple(np.concatenate([p, q]) for p, q in zip(x, y))
    for user_side in (True, False):
        inp1, mid = UR.side_inputs(old, a1, user_side)
        inp2, want = UR.side_inputs(cat(old, a1), a2, user_side)
        for a, b in zip(mid, (inp2["row_ptr_old"], inp2["col_old"], inp2["val_old"])):
            np.testing.assert_array_equal(a, b)
        _, once = UR.side_inputs(old, cat(a1, a2), user_side)
        for a, b in zip(want, once):
            np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------- ABI
def test_header_library_and_binding_agree():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    hdr = _header_signatures()
    for name in NAMES:
        assert name in declared_functions()
        assert hasattr(raw, name)
        assert hdr[name] == _lib.SIGNATURES[name][1], name
    assert _lib.SIGNATURES["als_csr_merge"][0] is ctypes.c_int
    assert _lib.SIGNATURES["als_csr_merge_tile"][0] is _lib.I32
    assert _lib.ABI_VERSION == _lib.lib().als_abi_version()


def test_tile_is_a_whole_number_of_wavefronts():
    T = _lib.lib().als_csr_merge_tile()
    assert T >= 256 and T % 64 == 0


def test_new_names_keep_clear_of_the_workspace_registry():
    for name in _lib.SIGNATURES:
        if name.startswith("als_csr_merge"):
            assert not name.endswith("_workspace_bytes")


def test_every_csr_merge_size_function_has_a_bounds_case():
    import test_gpu_update_bounds as BB
    sizers = sorted(n for n in _lib.SIGNATURES
                    if n.startswith("als_csr_merge_") and n.endswith("_bytes"))
    assert sizers == sorted(BB.SCRATCH_CASES)
    for name, tests in BB.SCRATCH_CASES.items():
        assert tests
        for t in tests:
            assert callable(getattr(BB, t, None)), f"{name}: {t} is not a test of the bounds file"
    assert callable(BB.test_csr_merge_all_guarded)


def _merge(**over):
    a = dict(row_ptr_old=8, col_old=4, val_old=4, nnz_old=5, n_old=2, n_cols_old=3, row_map=4,
             col_map=4, row_ptr_add=8, col_add=4, val_add=4, nnz_add=2, n_new=3, row_ptr_out=8,
             col_out=4, val_out=4, stream=0)
    a.update(over)
    return _lib.lib().als_csr_merge(*a.values())


@pytest.mark.parametrize("over,code", [
    (dict(nnz_old=-1), -1), (dict(nnz_add=-1), -1), (dict(n_old=-1), -1), (dict(n_new=-1), -1),
    (dict(n_cols_old=-1), -1),
    (dict(n_new=1), -1),                                   # n_new < n_old
    (dict(row_map=0), -1),                                 # rows were added: the map is needed
    (dict(row_ptr_old=0), -1), (dict(row_ptr_add=0), -1), (dict(row_ptr_out=0), -1),
    (dict(col_old=0), -1), (dict(val_old=0), -1), (dict(col_add=0), -1), (dict(val_add=0), -1),
    (dict(col_out=0), -1), (dict(val_out=0), -1),
    (dict(nnz_old=(1 << 31) - 2), -4),                     # nnz_old + nnz_add reaches 2^31
    (dict(n_new=0x7fffffff), -4)])
def test_argument_errors_before_any_device_call(over, code):
    L = _lib.lib()
    assert _merge(**over) == code, over
    assert b"als_csr_merge" in L.als_last_error()


# ---------------------------------------------------------------- Python layer
def test_sharded_engine_refuses_the_update_path():
    from als_mi355x.distributed import ShardedALS
    from als_mi355x.engine import ALSCore
    with pytest.raises(NotImplementedError, match="single-GPU engine"):
        filters.reject_sharded_update()
    for name, args in (("add_ratings", ([1], [2], [3.0])), ("refresh", ()), ("refit", (2,))):
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
    for call in (lambda: core.add_ratings([1], [2], [3.0]), core.refresh, lambda: core.refit(2)):
        with pytest.raises(ValueError, match="from_factors"):
            call()


def test_model_update_checks_its_mode_first():
    from als_mi355x.ml.recommendation import ALSModel
    from als_mi355x.mllib.recommendation import MatrixFactorizationModel
    for model in (MatrixFactorizationModel(None), ALSModel(None, {})):
        with pytest.raises(ValueError, match="mode must be"):
            model.update([(1, 2, 3.0)], 2, mode="retrain")
    with pytest.raises(ValueError, match="iterations"):
        MatrixFactorizationModel(None).update([(1, 2, 3.0)], -1)


def test_personal_update_wants_one_user():
    from als_mi355x import personal
    assert "personal_recommendations_update" in personal.__all__
    with pytest.raises(ValueError, match="user_id"):
        personal.personal_recommendations_update(object(), 0, [(1, 2, 3.0)], [(2, "x")])
