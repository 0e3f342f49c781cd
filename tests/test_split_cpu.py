"""CPU tests of K20 (per-user holdout and stratified folds): the numpy yardstick split_ref.py
against a big-integer restatement of the key and against the properties the rule promises, the
ABI (header prototypes == _lib.SIGNATURES for every als_split_*), the torch window arithmetic
of kernels/split.py against the reference's per-row Python integers, and the tuners' arguments.
No GPU is needed; every test here fails on the commit before K20.
"""
import ctypes

import numpy as np
import pytest
import torch

import split_ref as SR
from als_mi355x import _lib
from als_mi355x.kernels import split as KS
from test_abi import HEADER, _header_signatures, declared_functions

NAMES = ["als_split_row_cap", "als_split_scratch_bytes", "als_split_anchor",
         "als_split_eligible", "als_split_thresholds", "als_split_mark"]


# ---------------------------------------------------------------- the key
def test_numpy_key_equals_the_big_integer_restatement():
    rng = np.random.default_rng(0)
    edge = [0, 1, -1, 2 ** 31 - 1, -2 ** 31, 12345, -98765]
    seeds = [0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1, 42]
    us = edge + rng.integers(-2 ** 31, 2 ** 31, 30).tolist()
    is_ = edge[::-1] + rng.integers(-2 ** 31, 2 ** 31, 30).tolist()
    n = 0
    for seed in seeds:
        got = SR.key(seed, np.array(us)[:, None], np.array(is_)[None, :])
        for a, u in enumerate(us[:12]):
            for b, i in enumerate(is_[:12]):
                assert int(got[a, b]) == SR.key_py(seed, u, i)
                n += 1
        assert int(got[20, 30]) == SR.key_py(seed, us[20], is_[30])
    assert n >= 300
    assert SR.key_py(0, 0, 0) == 0xE220A8397B1DCDAF      # splitmix64's first output for seed 0
    assert SR.key_py(2 ** 64 - 1, 0, 0) == 0             # (seed + 1) wraps to 0: z = x = 0
    assert KS.split_seed(2 ** 64 - 1) == -1 and KS.split_seed(-1) == -1
    assert KS.split_seed(2 ** 63) == -2 ** 63 and KS.split_seed(5) == 5


# ---------------------------------------------------------------- the partition
def _ratings(seed=1, n=900, n_u=60, n_i=45):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, n_u, n) - 7
    i = np.minimum(rng.zipf(1.4, n) - 1, n_i - 1) - 3
    u, i = np.concatenate([u, u[:40], u[:10]]), np.concatenate([i, i[:40], i[:10]])   # copies
    r = rng.integers(1, 11, len(u)).astype(np.float32) / 2
    return u, i, r


MODES = [("count", 1), ("count", 3), ("fraction", 0.2), ("fraction", 0.9), ("fold", (0, 3)),
         ("fold", (2, 3))]


@pytest.mark.parametrize("user_side", [True, False])
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("mode,value", MODES)
def test_held_and_kept_partition_the_input(mode, value, keep, user_side):
    trip = _ratings()
    for min_keep in (0, 1, 2):
        sp = SR.Split(trip[0], trip[1], 9, mode=mode, value=value, min_keep=min_keep,
                      keep_items=keep, user_side=user_side)
        kept, held = sp.kept(trip), sp.held_out(trip)
        both = sorted(zip(*(np.concatenate([a, b]).tolist() for a, b in zip(kept, held))))
        assert both == sorted(zip(*(x.tolist() for x in trip)))
        pair = trip[0].astype(np.int64) * 10 ** 6 + trip[1]
        assert not set(pair[sp.held].tolist()) & set(pair[~sp.held].tolist())  # copies: one fate
        sel_ids, oth_ids = (trip[0], trip[1]) if user_side else (trip[1], trip[0])
        if keep:    # no row of the other side leaves
            assert set(oth_ids[~sp.held].tolist()) == set(oth_ids.tolist())
    if mode != "fold":
        # copies share a rank, so a window of k ranks can take more than k entries: the floor
        # is a promise about distinct pairs
        first = np.sort(np.unique(pair, return_index=True)[1])
        for min_keep in (0, 1, 2):
            sp = SR.Split(trip[0][first], trip[1][first], 9, mode=mode, value=value,
                          min_keep=min_keep, keep_items=keep, user_side=user_side)
            left = np.bincount(sp.sel[sp.eligible & ~sp.held], minlength=sp.n_sel)
            assert (left[sp.e > min_keep] >= min_keep).all()
            assert (left[sp.e <= min_keep] == sp.e[sp.e <= min_keep]).all()
            assert (np.bincount(sp.sel[sp.held], minlength=sp.n_sel) == sp.hi - sp.lo).all()


def test_fold_windows_partition_every_row():
    trip = _ratings(4)
    for F in (2, 3, 7):
        base = SR.Split(trip[0], trip[1], 3)
        seen = np.zeros(len(trip[0]), np.int64)
        sizes = []
        for f in range(F):
            base.set_windows("fold", (f, F))
            seen += base.held
            sizes.append(base.hi - base.lo)
        assert (seen == base.eligible).all()                 # every eligible entry exactly once
        sizes = np.array(sizes)
        assert (sizes.sum(axis=0) == base.e).all()
        assert (sizes.max(axis=0) - sizes.min(axis=0) <= 1).all()


def test_the_rule_ignores_the_stored_order_and_the_side():
    trip = _ratings(5)
    p = np.random.default_rng(0).permutation(len(trip[0]))
    a = SR.Split(trip[0], trip[1], 6, mode="count", value=2)
    b = SR.Split(trip[0][p], trip[1][p], 6, mode="count", value=2)
    assert (a.held[p] == b.held).all()
    T = 64
    nu = int(np.unpackbits(a.marks(True, T)[0].view(np.uint8)).sum())
    ni = int(np.unpackbits(a.marks(False, T)[0].view(np.uint8)).sum())
    assert nu == ni == int((~a.held).sum()) == a.marks(True, T)[1][-1]
    c = SR.Split(trip[0], trip[1], 7, mode="count", value=2)
    assert (a.held != c.held).any()                          # the seed matters


def test_thresholds_state_the_window():
    trip = _ratings(6)
    sp = SR.Split(trip[0], trip[1], 2, mode="fold", value=(1, 3))
    lo_k, lo_c, hi_k, hi_c = sp.thresholds()
    comp = list(zip(sp.keys.tolist(), sp.oth.tolist()))
    for j in np.nonzero(sp.eligible)[0]:
        r = sp.sel[j]
        inside = ((int(lo_k[r]), int(lo_c[r])) <= comp[j] < (int(hi_k[r]), int(hi_c[r])))
        assert inside == bool(sp.held[j])


# ---------------------------------------------------------------- windows
@pytest.mark.parametrize("min_keep", [0, 1, 3])
def test_window_arithmetic_equals_the_reference(min_keep):
    e = np.array([0, 1, 2, 3, 4, 5, 7, 10, 63, 64, 65, 1000, 32767, 2 ** 31 - 2], np.int64)
    cases = [("count", k) for k in (0, 1, 3, 100)]
    cases += [("fraction", p) for p in (0.0, 0.1, 0.2, 0.25, 0.5, 0.75, 1.0)]
    cases += [("fold", (f, F)) for F in (1, 2, 3, 7, 11) for f in (0, F // 2, F - 1)]
    for mode, value in cases:
        lo, hi = KS.split_windows(torch.as_tensor(e.astype(np.int32)), mode, value, min_keep)
        want = SR.windows(e, mode, value, min_keep)
        assert lo.dtype == hi.dtype == torch.int32
        assert lo.numpy().tolist() == want[0].tolist(), (mode, value)
        assert hi.numpy().tolist() == want[1].tolist(), (mode, value)
        assert (hi.numpy() <= e).all() and (lo.numpy() <= hi.numpy()).all()
        if mode != "fold":
            assert (hi.numpy()[e <= min_keep] == 0).all()


def test_split_argument_checks():
    assert KS.check_split_args(count=2) == ("count", 2)
    assert KS.check_split_args(fraction=0.5) == ("fraction", 0.5)
    assert KS.check_split_args(fold=(1, 3)) == ("fold", (1, 3))
    for bad in (dict(), dict(count=1, fraction=0.1), dict(count=1, fold=(0, 2)), dict(count=-1),
                dict(count=1.5), dict(fraction=1.5), dict(fraction=-0.1), dict(fold=(3, 3)),
                dict(fold=(0, 0)), dict(count=1, min_keep=-1)):
        with pytest.raises(ValueError):
            KS.check_split_args(**bad)


# ---------------------------------------------------------------- ABI
def test_header_library_and_binding_agree():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    hdr = _header_signatures()
    for name in NAMES:
        assert name in declared_functions()
        assert hasattr(raw, name)
        assert hdr[name] == _lib.SIGNATURES[name][1], name
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("als_split_")) == sorted(NAMES)
    assert _lib.SIGNATURES["als_split_row_cap"][0] is _lib.I32
    assert _lib.SIGNATURES["als_split_scratch_bytes"][0] is _lib.SZ
    import re
    macro = int(re.search(r"#define ALS_ABI_VERSION (\d+)", open(HEADER).read()).group(1))
    assert _lib.ABI_VERSION == macro == _lib.lib().als_abi_version()


def test_cap_and_scratch_size():
    L = _lib.lib()
    cap = L.als_split_row_cap()
    assert 64 <= cap <= 4096 and cap % 64 == 0
    size = L.als_split_scratch_bytes
    assert size(-1, 5) == 0 and size(5, -1) == 0 and size(0, 0) >= 4
    assert size(10 ** 6, 10) >= L.als_csr_remove_scratch_bytes(10 ** 6, 10)
    assert size(100, 10 ** 6) >= 4 * 10 ** 6                 # the long-row list
    sizes = [size(n, 100) for n in (1, 10 ** 4, 10 ** 7, (1 << 31) - 1)]
    assert sizes == sorted(sizes)


def test_argument_errors_come_before_any_launch():
    L = _lib.lib()
    side = lambda **o: list(dict(dict(row_ptr=8, col=8, nnz=5, n_rows=2, n_cols=3, row_ids=8,
                                      col_ids=8, rows_are_users=1, seed=0), **o).values())
    assert L.als_split_anchor(*side(nnz=-1), 8, 8, 1 << 20, 0) == -1
    assert L.als_split_anchor(*side(), 0, 8, 1 << 20, 0) == -1                  # null anchor
    assert L.als_split_anchor(*side(), 8, 8, 0, 0) == -2                        # short scratch
    assert L.als_split_anchor(*side(nnz=1 << 31), 8, 8, 1 << 40, 0) == -4
    assert L.als_split_eligible(8, 8, 5, 2, 3, 0, 0, 0) == -1                   # null output
    thr = [8, 8, 8, 8]
    assert L.als_split_thresholds(*side(), 0, 8, 8, L.als_split_row_cap() + 1, *thr, 8, 1 << 20,
                                  0) == -1
    assert L.als_split_thresholds(*side(), 0, 0, 8, 0, *thr, 8, 1 << 20, 0) == -1
    assert L.als_split_thresholds(*side(), 0, 8, 8, 0, *thr, 8, 0, 0) == -2
    assert L.als_split_mark(*side(), 1, *thr, 0, 0, 8, 8, 8, 1 << 20, 0) == -1  # null keep_bits
    assert L.als_split_mark(*side(), 1, *thr, 0, 8, 8, 8, 8, 0, 0) == -2
    assert L.als_last_error()


def test_every_split_size_function_has_a_bounds_case():
    import test_gpu_split_bounds as BB
    sizers = sorted(n for n in _lib.SIGNATURES
                    if n.startswith("als_split_") and n.endswith("_bytes"))
    assert sizers == sorted(BB.SCRATCH_CASES)
    for name, tests in BB.SCRATCH_CASES.items():
        assert tests
        for t in tests:
            assert callable(getattr(BB, t, None)), f"{name}: {t} is not a test of the bounds file"


# ---------------------------------------------------------------- tuners
class _NoEstimator:
    pass


def test_tuner_arguments():
    from als_mi355x.ml.tuning import CrossValidator, TrainValidationSplit
    maps = [{}]
    tv = TrainValidationSplit(_NoEstimator(), maps, None, stratify="user", holdOut=1)
    assert tv.getStratify() == "user" and tv.getHoldOut() == 1
    assert TrainValidationSplit(_NoEstimator(), maps, None).getStratify() is None
    cv = CrossValidator(_NoEstimator(), maps, None, stratify="user")
    assert cv.getStratify() == "user"
    for bad in (dict(stratify="item"), dict(holdOut=1), dict(stratify="user", holdOut=0),
                dict(stratify="user", holdOut=1.5)):
        with pytest.raises(ValueError):
            TrainValidationSplit(_NoEstimator(), maps, None, **bad)
    with pytest.raises(ValueError):
        CrossValidator(_NoEstimator(), maps, None, stratify="rows")
    with pytest.raises(ValueError, match="foldCol"):
        CrossValidator(_NoEstimator(), maps, None, stratify="user", foldCol="fold")


def test_unstratified_tuners_split_as_before():
    from als_mi355x import datasets as D
    from als_mi355x.ml.tuning import CrossValidator, TrainValidationSplit, fold_assignment
    tv = TrainValidationSplit(_NoEstimator(), [{}], None, trainRatio=0.8, seed=5, stratify=None)
    for a, b in zip(tv.split(1000), D.random_split(1000, (0.8, 1.0 - 0.8), 5)):
        assert a.tobytes() == b.tobytes()
    cv = CrossValidator(_NoEstimator(), [{}], None, numFolds=4, seed=6, stratify=None)
    data = {"user": np.arange(500), "item": np.arange(500), "rating": np.ones(500)}
    assert cv.folds(data).tobytes() == fold_assignment(500, 4, 6).tobytes()


def test_the_sharded_engine_refuses_with_the_same_signature():
    import inspect
    from als_mi355x.distributed import ShardedALS
    from als_mi355x.engine import ALSCore
    for name in ("holdout", "split"):
        assert (inspect.signature(getattr(ShardedALS, name))
                == inspect.signature(getattr(ALSCore, name)))
        with pytest.raises(NotImplementedError, match="single-GPU"):
            getattr(ShardedALS, name)(None, count=1)
