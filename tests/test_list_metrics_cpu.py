"""CPU tests of K15 (no GPU): the numpy reference against brute force, the hand cases of the
measures, and the argument checks of the Python layer that fire before the library is
touched."""
import math

import numpy as np
import pytest
import torch

import list_metrics_ref as LR
from als_mi355x import engine as E
from als_mi355x import filters


def _duplicate_free_lists(rng, n_q, at, n_v):
    return np.stack([rng.permutation(n_v)[:at] for _ in range(n_q)]).astype(np.int32)


@pytest.mark.parametrize("n_q,at,n_v", [(1, 3, 5), (7, 4, 9), (40, 10, 37)])
def test_overlap_identity_against_pairwise_intersections(n_q, at, n_v):
    rng = np.random.default_rng(n_q)
    idx = _duplicate_free_lists(rng, n_q, at, n_v)
    counts, skipped = LR.exposure(idx, at, n_v)
    assert skipped == 0 and counts.sum() == n_q * at
    assert LR.concentration(counts)[5] == LR.overlap_pairs(idx)


def test_exposure_against_a_loop_with_every_skip_rule():
    rng = np.random.default_rng(3)
    n_v, at = 45, 6
    idx = rng.integers(-2, n_v + 3, size=(30, at + 2)).astype(np.int32)
    idx[4, 1] = np.iinfo(np.int32).min
    allowed = rng.random(n_v) < 0.7
    bits = LR.pack_bits(allowed)
    want = np.zeros(n_v, np.int64)
    skipped = 0
    for row in idx:
        for j in row[:at]:
            if 0 <= j < n_v and allowed[j]:
                want[j] += 1
            else:
                skipped += 1
    got, got_skipped = LR.exposure(idx, at, n_v, bits)
    assert (got == want).all() and got_skipped == skipped
    assert (LR.unpack_bits(bits, n_v) == allowed).all()
    assert (LR.pack_bits(allowed) == filters.pack_allow_bits(
        torch.as_tensor(np.nonzero(allowed)[0]), n_v).numpy()).all()


@pytest.mark.parametrize("n", [1, 2, 5, 64, 301])
def test_gini_sorted_form_equals_the_pairwise_form(n):
    rng = np.random.default_rng(n)
    c = rng.integers(0, 50, size=n)
    c[rng.integers(n)] += 1   # never all zero
    assert LR.gini_sorted(c) == pytest.approx(LR.gini_pairs(c), rel=1e-12, abs=1e-15)
    one = np.zeros(n, np.int64)
    one[n // 2] = 9
    assert LR.gini_sorted(one) == pytest.approx(1.0 - 1.0 / n, rel=1e-12, abs=1e-15)
    assert LR.gini_sorted(np.full(n, 4)) == 0.0


@pytest.mark.parametrize("n_v", [1, 6, 97])
def test_gini_with_leading_zeros_equals_the_compacted_form(n_v):
    rng = np.random.default_rng(n_v)
    counts = rng.integers(0, 30, size=n_v)
    in_cat = rng.random(n_v) < 0.6
    in_cat[rng.integers(n_v)] = True
    counts[np.nonzero(in_cat)[0][0]] += 1
    want = LR.gini_sorted(counts[in_cat])
    assert LR.gini_leading_zeros(counts, in_cat) == pytest.approx(want, rel=1e-12, abs=1e-15)
    assert LR.concentration(counts, LR.pack_bits(in_cat))[3] == want


def test_entropy_and_nan_rules():
    c = LR.concentration(np.array([4, 4, 4, 4]))
    assert c[:3] == [4.0, 4.0, 16.0] and c[3] == 0.0 and c[4] == pytest.approx(2.0, rel=1e-12)
    z = LR.concentration(np.zeros(5, np.int64))
    assert z[:3] == [5.0, 0.0, 0.0] and math.isnan(z[3]) and math.isnan(z[4]) and z[5:] == [0, 0]
    e = LR.concentration(np.zeros(0, np.int64))
    assert e[:3] == [0.0, 0.0, 0.0] and math.isnan(e[3]) and math.isnan(e[4])
    one = LR.concentration(np.array([0, 7, 0]))
    assert one[4] == 0.0 and one[5] == 21.0 and one[6] == 7.0


def test_hand_cases_same_disjoint_and_single_list():
    at, n_v = 4, 20
    same = np.tile(np.arange(at, dtype=np.int32), (6, 1))
    m = LR.metrics_dict(same, at, n_v)
    assert m["coverage"] == at / n_v and m["personalization"] == 0.0 and m["topItemShare"] == 1.0
    disjoint = np.arange(5 * at, dtype=np.int32).reshape(5, at)
    m = LR.metrics_dict(disjoint, at, n_v)
    assert m["coverage"] == 1.0 and m["personalization"] == 1.0 and m["gini"] == 0.0
    assert m["effectiveItems"] == pytest.approx(20.0, rel=1e-12)
    m = LR.metrics_dict(same[:1], at, n_v)
    assert math.isnan(m["personalization"]) and m["lists"] == 1 and m["entries"] == at
    # the engine's dictionary from the same sums
    counts, skipped = LR.exposure(same, at, n_v)
    d = E.list_metrics_dict(LR.concentration(counts), None, 6, at, skipped)
    want = LR.metrics_dict(same, at, n_v)
    assert set(d) == set(E.LIST_METRIC_FIELDS) == set(want)
    for k in want:
        assert d[k] == want[k] or (math.isnan(d[k]) and math.isnan(want[k])), k


def test_novelty_reference_by_hand():
    pop = np.array([8, 0, 2, 1], np.int64)
    idx = np.array([[0, 2, -1], [1, 1, 9], [-1, -1, -1], [3, 1, 0]], np.int32)
    tail = LR.pack_bits(np.array([False, True, False, True]))
    sums, rows = LR.novelty(idx, 3, 4, pop, 16, None, tail)
    assert rows[0].tolist() == [(1.0 + 3.0) / 2, 5.0, 0.0]
    assert math.isnan(rows[1, 0]) and rows[1, 1:].tolist() == [0.0, 1.0]
    assert np.isnan(rows[2]).all()
    assert rows[3].tolist() == [(4.0 + 1.0) / 2, 3.0, 2.0 / 3.0]
    assert sums == [2.0 + 2.5, 2.0, 8.0, 3.0, 0.0 + 1.0 + 2.0 / 3.0, 7.0, 5.0]
    _, no_tail = LR.novelty(idx, 3, 4, pop, 16)
    assert np.isnan(no_tail[:, 2]).all()


def test_long_tail_cut_and_ties():
    pop = torch.tensor([5, 9, 5, 5, 1, 0, 9, 3, 5, 2], dtype=torch.int32)
    # head = floor(0.4 * 10) = 4 rows: the two 9s, then the 5s by ascending row (0, 2)
    want = np.ones(10, bool)
    want[[1, 6, 0, 2]] = False
    assert (LR.long_tail(pop.numpy(), 10, 0.4) == want).all()
    got = E.long_tail_bits(pop, 10, 0.4)
    assert (LR.unpack_bits(got.numpy(), 10) == want).all()
    # a masked catalogue: 6 rows, head = floor(0.5 * 6) = 3 of them
    cat = torch.tensor([0, 2, 3, 4, 8, 9])
    in_cat = np.zeros(10, bool)
    in_cat[cat.numpy()] = True
    want = LR.long_tail(pop.numpy(), 10, 0.5, in_cat)
    assert sorted(np.nonzero(want)[0]) == [4, 8, 9]
    assert (LR.unpack_bits(E.long_tail_bits(pop, 10, 0.5, cat).numpy(), 10) == want).all()


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.1, 1.5, float("nan")])
def test_head_fraction_outside_the_open_interval(bad):
    pop = torch.ones(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="head_fraction"):
        E.long_tail_bits(pop, 4, bad)
    core = E.ALSCore.__new__(E.ALSCore)   # no device: the check comes first
    with pytest.raises(ValueError, match="head_fraction"):
        core.list_metrics(top=5, head_fraction=bad)
    with pytest.raises(ValueError, match="head_fraction"):
        E.list_metrics_rows(torch.zeros((2, 3), dtype=torch.int32), 3, 4, None, head_fraction=bad)


def test_list_metrics_wants_exactly_one_kind_of_lists():
    core = E.ALSCore.__new__(E.ALSCore)
    with pytest.raises(ValueError, match="either id_lists or top"):
        core.list_metrics()
    with pytest.raises(ValueError, match="either id_lists or top"):
        core.list_metrics(np.zeros((2, 3), np.int32), top=3)
    for top in (0, 257):
        with pytest.raises(ValueError, match="top must be"):
            core.list_metrics(top=top)
    with pytest.raises(ValueError, match="exclude"):
        core.list_metrics(np.zeros((2, 3), np.int32), exclude="train")


@pytest.mark.parametrize("shape", [(5,), (2, 3, 4), (3, 0), (3, 257)])
def test_list_shapes_of_the_core(shape):
    core = E.ALSCore.__new__(E.ALSCore)
    with pytest.raises(ValueError, match="id_lists must be"):
        core.list_metrics(np.zeros(shape, np.int32))


def test_list_shapes_of_the_wrappers():
    ok = torch.zeros((4, 6), dtype=torch.int32)
    pop = torch.ones(9, dtype=torch.int32)
    for fn in (lambda i, at: E.list_exposure_rows(i, at, 9),
               lambda i, at: E.list_novelty_rows(i, at, 9, pop, 4, None)):
        with pytest.raises(ValueError, match="int32"):
            fn(ok.long(), 6)
        with pytest.raises(ValueError, match="int32"):
            fn(ok[0], 6)
        with pytest.raises(ValueError, match="unit stride"):
            fn(ok.t(), 4)
        with pytest.raises(ValueError, match="width 6 < at = 7"):
            fn(ok, 7)
        for at in (0, 257):
            with pytest.raises(ValueError, match="at must be"):
                fn(ok, at)
    with pytest.raises(ValueError, match="counts must be"):
        E.list_exposure_rows(ok, 6, 9, counts=torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError, match="counts must be"):
        E.list_concentration(torch.zeros(9, dtype=torch.int64), 9, None, 4, 6, None)
    with pytest.raises(ValueError, match="pop must be"):
        E.list_novelty_rows(ok, 6, 9, pop[:8], 4, None)
    with pytest.raises(ValueError, match="n_pop"):
        E.list_novelty_rows(ok, 6, 9, pop, 0, None)


def test_sharded_engine_refuses_list_metrics():
    with pytest.raises(NotImplementedError, match="list_metrics"):
        filters.reject_sharded_list_metrics()
    from als_mi355x.distributed import ShardedALS
    with pytest.raises(NotImplementedError, match="single-GPU"):
        ShardedALS.list_metrics(None, top=10)


def test_binding_lists_the_k15_symbols():
    from als_mi355x import _lib
    for name in ("als_list_exposure", "als_list_exposure_window", "als_list_concentration",
                 "als_list_concentration_scratch_bytes", "als_list_novelty",
                 "als_list_novelty_scratch_bytes"):
        assert name in _lib.SIGNATURES
    L = _lib.lib()
    assert L.als_list_exposure_window() >= 0
    assert L.als_list_concentration_scratch_bytes(10) < \
        L.als_list_concentration_scratch_bytes(10 ** 6)
    assert L.als_list_novelty_scratch_bytes(10) <= L.als_list_novelty_scratch_bytes(10 ** 6)
    # host checks come before any device call (no GPU needed)
    assert L.als_list_exposure(1, 1, 4, 0, 5, 0, 0, 1, 0, 0) == -4
    assert L.als_list_exposure(1, 1, 4, 257, 5, 0, 0, 1, 0, 0) == -4
    assert L.als_list_exposure(1, 1, 3, 4, 5, 0, 0, 1, 0, 0) == -1
    assert L.als_list_novelty(1, 1, 4, 4, 5, 0, 1, 0, 0, 1, 0, 16, 1 << 20, 0) == -1  # n_pop
    assert L.als_list_concentration(1, 5, 0, 2, 4, 1, 16, 8, 0) == -2
    assert L.als_last_error()


def test_every_k15_size_function_has_a_bounds_case():
    """K15's workspaces are sized by als_list_*_scratch_bytes; each has a guard-band case in
    test_gpu_list_metrics_bounds.py (the registry of the *_workspace_bytes functions is
    test_gpu_buffer_bounds.WORKSPACE_CASES)."""
    import test_gpu_list_metrics_bounds as BL
    from als_mi355x import _lib
    sizers = sorted(n for n in _lib.SIGNATURES if n.startswith("als_list_") and n.endswith("_bytes"))
    assert sizers == sorted(BL.SCRATCH_CASES) and len(sizers) == 2
    for name, tests in BL.SCRATCH_CASES.items():
        assert tests
        for t in tests:
            assert callable(getattr(BL, t, None)), f"{name}: {t} is not a test of the bounds file"
