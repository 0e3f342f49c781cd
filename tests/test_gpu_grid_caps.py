"""The strided paths past the grid caps of K6, K9's reduction, K10's Gram and K15, on the GPU.

Every one of these kernels caps its grid; past the cap a block loops over further row groups
(`for (g = blockIdx.x; g < n_grp; g += gridDim.x)`), and no other test is large enough to make
the second trip.  The sizes come from the caps in the sources (tests/grid_caps.py): the cap
itself (no loop), + 1 (one wave makes a second trip), + 5 (a last group of one row whose other
waves skip the trip) and twice the cap + 1 (three trips).

Each test runs the entry point through the kernels/*.py wrapper (reached as engine.NAME) of
the kernel's own test file,
compares the per-row outputs on ALL rows (those at and past the cap are the point) and the sums
with a vectorised reference (held to the older row-by-row references on a prefix in
test_grid_caps_cpu.py), and calls twice for identical bytes.  The bars are those of the
kernels' own test files; where a larger shape needs an argument, the test's docstring gives it.
"""
import functools
import math

import numpy as np
import pytest
import torch

import grid_caps as G
import list_metrics_ref as LR
import test_gpu_list_metrics as TL
import test_gpu_rank_metrics as TR
from als_mi355x import _lib
from als_mi355x import engine as E
from helpers import report

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-12


def _d(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _rel_err(got, want):
    """Worst |got - want| / |want| over the finite entries with want != 0 (0 if none)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ok = np.isfinite(want) & (want != 0)
    return float((np.abs(got[ok] - want[ok]) / np.abs(want[ok])).max()) if ok.any() else 0.0


# ------------------------------------------------------------------ K6
PAD = 5


@functools.lru_cache(maxsize=None)
def _k6_case(at, n_max):
    """The pattern of test_gpu_rank_metrics extended to n_max rows (kinds cycle by r % 8, rows
    3 and 4 of every group alias one range), PAD columns holding a relevant id past `at`, and
    the per-row reference of every row."""
    lists, begin, end, col, _ = TR.pattern_inputs(at, n_max)
    wide = np.empty((n_max, at + PAD), np.int32)
    wide[:, :at] = lists
    wide[:, at:] = col[np.minimum(begin, len(col) - 1)][:, None]
    return wide, begin, end, col, G.rank_rows(lists, begin, end, col, at)


def _check_k6(at, n_q, n_max):
    wide, begin, end, col, ref = _k6_case(at, n_max)
    idx = _d(wide)[:n_q]
    b, e, c = _d(begin[:n_q]), _d(end[:n_q]), _d(col)
    sums, pr = TR.run(idx, at, b, e, c)
    want = ref[:n_q]
    assert pr.shape == (n_q, 4)
    np.testing.assert_array_equal(pr[:, :2], want[:, :2])            # precision, recall: bits
    err = _rel_err(pr[:, 2:], want[:, 2:])
    np.testing.assert_allclose(pr[:, 2:], want[:, 2:], rtol=RTOL, atol=0)
    want_sums = [math.fsum(want[:, j]) for j in range(4)]
    err_s = _rel_err(sums[:4], want_sums)
    print(f"K6 at={at} n_q={n_q}: worst AP/NDCG row error {err:.3e}, worst sum error "
          f"{err_s:.3e} (bar {RTOL:g})")
    report(f"grid_caps K6 at={at} n_q={n_q} per_row", err)
    report(f"grid_caps K6 at={at} n_q={n_q} sums", err_s)
    np.testing.assert_allclose(sums[:4], want_sums, rtol=RTOL, atol=0)
    assert sums[4] == float((end[:n_q] > begin[:n_q]).sum())         # rows with labels
    assert sums[5] == float((want[:, 0] > 0).sum())                  # rows with a hit
    sums2, pr2 = TR.run(idx, at, b, e, c)
    lean, none = TR.run(idx, at, b, e, c, per_row=False)
    assert none is None
    assert sums.tobytes() == sums2.tobytes() == lean.tobytes() and pr.tobytes() == pr2.tobytes()


@pytest.mark.parametrize("which", range(4))
def test_rank_metrics_past_the_cap(which):
    """K6 at kRmMaxBlocks x kRmRowsPerBlock rows, + 1, + 5 and 2 x + 1, at = 10.

    The sums are held to math.fsum of the reference rows at 1e-12 relative: a wave adds at most
    3 rows (three trips), a block its 4 waves, the final block at most 16 strided partials per
    thread and 8 tree levels, every term >= 0: fewer than 64 roundings on top of the rows' own
    1e-12, about 7e-15."""
    ns = G.sizes("rank_metrics")
    _check_k6(10, ns[which], ns[-1])


def test_rank_metrics_second_pass_inside_a_second_trip():
    """at = 65 (a second 64-position pass of a row) at cap + 5 rows (inside a second trip)."""
    n = G.sizes("rank_metrics")[2]
    _check_k6(65, n, n)


# ------------------------------------------------------------------ K9, the reduction alone
COUNTS = [E.FULL_RANK_SUMS.index(k) for k in
          ("rows", "pairs", "inadmissible", "auc_rows", "rr_rows", "pr_rows")]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("which", range(4))
def test_full_rank_metrics_past_the_cap(which, weighted):
    """als_full_rank_metrics on synthetic counts (grid_caps.full_rank_inputs; no sweep) at
    kFrMaxBlocks x kFrRowsPerBlock rows, + 1, + 5 and 2 x + 1.  Sums at rel = abs = 1e-12, the
    bar of test_gpu_full_rank.py (the chain past the row values is the one of K6, below 64
    roundings; a row AUC of synthetic counts can be negative, so that sum cancels a little);
    the six counts exactly; per_row at 1e-12 with the NaNs in the same places."""
    n_q = G.sizes("full_rank_metrics")[which]
    above, tied, n_adm, begin, end, w = G.full_rank_inputs(n_q, weighted=weighted)
    want, want_rows = G.full_rank_sums(above, tied, n_adm, begin, end, w)
    args = (_d(above), _d(tied), _d(n_adm), _d(begin), _d(end), E.Workspace(torch.device(DEV)),
            None if w is None else _d(w))
    sums, pr = E.full_rank_sums_rows(*args, per_row=True)
    sums, pr = sums.cpu().numpy(), pr.cpu().numpy()
    err_s, err_r = _rel_err(sums, want), _rel_err(pr, want_rows)
    print(f"K9 n_q={n_q} weighted={weighted}: worst sum error {err_s:.3e}, worst row error "
          f"{err_r:.3e} (bar {RTOL:g})")
    report(f"grid_caps K9 n_q={n_q} weighted={weighted} sums", err_s)
    report(f"grid_caps K9 n_q={n_q} weighted={weighted} per_row", err_r)
    assert sums.tolist() == pytest.approx(want, rel=1e-12, abs=1e-12)
    for j in COUNTS:
        assert sums[j] == want[j], E.FULL_RANK_SUMS[j]
    assert pr.shape == (n_q, 3)
    np.testing.assert_array_equal(np.isnan(pr), np.isnan(want_rows))
    np.testing.assert_allclose(pr, want_rows, rtol=RTOL, atol=0, equal_nan=True)
    assert not np.isnan(pr[n_q - 1, 2])              # the last row has entries of its own
    sums2, pr2 = E.full_rank_sums_rows(*args, per_row=True)
    lean, none = E.full_rank_sums_rows(*args)
    assert none is None
    assert sums.tobytes() == sums2.cpu().numpy().tobytes() == lean.cpu().numpy().tobytes()
    assert pr.tobytes() == pr2.cpu().numpy().tobytes()


# ------------------------------------------------------------------ K15 novelty
@pytest.mark.parametrize("which", range(4))
def test_novelty_past_the_cap(which):
    """als_list_novelty at kLnMaxBlocks x kLnRowsPerBlock lists, + 1, + 5 and 2 x + 1, at = 10;
    inputs and bars of test_gpu_list_metrics.test_novelty_against_the_reference."""
    n_q, at, n_v = G.sizes("novelty")[which], 10, 1200
    idx, pop, allow, tail = G.novelty_inputs(n_q, at, n_v)
    for bits, t in ((None, tail), (allow, tail), (None, None)):
        want_s, want_r = G.novelty(idx, at, n_v, pop, 4321, bits, t)
        got_s, got_r = TL._novelty(idx, at, n_v, pop, 4321, bits, t)   # three calls, same bytes
        err_r, err_s = _rel_err(got_r, want_r), _rel_err(got_s, want_s)
        print(f"K15 novelty n_q={n_q} mask={bits is not None} tail={t is not None}: worst row "
              f"error {err_r:.3e}, worst sum error {err_s:.3e} (bar {RTOL:g})")
        report(f"grid_caps K15 novelty n_q={n_q} per_row", err_r)
        report(f"grid_caps K15 novelty n_q={n_q} sums", err_s)
        assert got_r.shape == (n_q, 3)
        assert (np.isnan(got_r) == np.isnan(want_r)).all()
        np.testing.assert_allclose(got_r, want_r, rtol=RTOL, atol=0, equal_nan=True)
        np.testing.assert_allclose(got_s, want_s, rtol=RTOL, atol=0)
        assert got_s[[1, 3, 5, 6]].tolist() == [want_s[i] for i in (1, 3, 5, 6)]
        if t is None:
            assert np.isnan(got_r[:, 2]).all() and got_s[4] == 0.0
    assert np.isnan(got_r[0]).all() and math.isnan(got_r[2, 0]) and got_r[2, 1] == 0.0


# ------------------------------------------------------------------ K15 exposure
def _exposure_case(n_q, zipf):
    at, n_v = G.EXPOSURE_AT, 2 * TL._window() + 3
    idx = TL._lists(n_q, at, n_v, seed=n_q % 1000, zipf=zipf)
    hit = np.random.default_rng(n_q).random((n_q, at), dtype=np.float32)
    idx[:, :at][hit < 0.025] = -1
    idx[:, :at][(hit >= 0.025) & (hit < 0.05)] = n_v
    want, want_skipped = LR.exposure(idx, at, n_v)
    got, skipped = TL._exposure(idx, at, n_v)                          # two calls, same bytes
    assert got.dtype == np.int32 and (got == want).all()
    assert skipped == want_skipped and 0.04 * n_q * at < skipped < 0.06 * n_q * at
    assert int(got.sum()) + skipped == n_q * at
    return want


@pytest.mark.parametrize("which", range(3))
def test_exposure_past_the_cap(which):
    """als_list_exposure at at = 256 over 2 window + 3 rows with kLxMaxBlocks chunks, + 1 (a
    last chunk of one list, taken by workgroup 0 on its second trip) and 2 x + 1.  Integer adds:
    the counts equal np.bincount and `skipped` the 5 % of entries set to -1 or n_v exactly."""
    _exposure_case(G.exposure_sizes()[which], zipf=False)


def test_exposure_past_the_cap_zipf():
    want = _exposure_case(G.exposure_sizes()[1], zipf=True)
    assert want.max() > 50 * np.median(want[want > 0])


# ------------------------------------------------------------------ K15 concentration
@pytest.mark.parametrize("extra", [0, "one block + 1"])
def test_concentration_past_the_cap(extra):
    """als_list_concentration over kLcMaxBlocks x 2048 catalogue rows (every thread of
    lc_keys_kernel / lc_sorted_kernel makes 8 strided trips, the grid at its cap) and over 2049
    more (a ninth trip for the first 2049 threads).  Fields and bars of
    test_gpu_list_metrics._assert_concentration; list_metrics_ref.concentration is one sort."""
    per = G.constants()["lcItemsPerBlock"]
    n_v = G.cap_rows("concentration") + (per + 1 if extra else 0)
    rng = np.random.default_rng(n_v)
    p = 1.0 / np.arange(1, n_v + 1) ** 1.05
    counts = rng.permutation(rng.multinomial(40 * n_v + 7, p / p.sum()))
    in_cat = rng.random(n_v) < 0.5
    bits = LR.pack_bits(in_cat).copy()
    if n_v % 32:
        bits[-1] |= np.int32(-1) << np.int32(n_v % 32)               # bits past n_v: ignored
    for b in (None, bits):
        got, want = TL._concentration(counts, b), LR.concentration(counts, b)
        err = _rel_err(got[3:5], want[3:5])
        print(f"K15 concentration n_v={n_v} mask={b is not None}: worst Gini / entropy error "
              f"{err:.3e} (bar {RTOL:g})")
        report(f"grid_caps K15 concentration n_v={n_v} mask={b is not None}", err)
        TL._assert_concentration(got, want)
    assert got[0] == in_cat.sum() and 0 < got[1] < got[0]


# ------------------------------------------------------------------ K10 Gram
def _gram_table(F):
    n, k = F.shape
    T = torch.zeros((n, E.ld_for(k)), dtype=torch.float32, device=DEV)
    T[:, :k] = _d(F, torch.float32)
    return T


@pytest.mark.parametrize("rank", [1, 17, 128])
@pytest.mark.parametrize("which", range(3))
def test_gram_past_the_cap(which, rank):
    """als_gram_dot_f64 at kGramMaxBlocks x kGramMinRows rows (256 blocks of 64), + 1 and + 5:
    past the cap gram_rows_per_block leaves 64 (68 rows a block at 16,385 and 16,389) and the
    last block's run is no multiple of the 4 rows an instruction takes.

    Bar: |G - F^T F| <= 1e-13 sum_rows |f_a f_b| per entry, the bar of test_gpu_objective.py.
    It still holds by derivation: the products of two fp32 values are exact in fp64, so the
    error is that of the additions alone, each at most 2^-53 of the sum of absolute values.  At
    16,389 rows an entry is a block's chain of at most 68 additions (17 instructions of 4 rows)
    followed by the ascending fold of 242 blocks: 310 roundings x 2^-53 = 3.4e-14.  The dot is
    held as in test_gram_f64_matches_numpy.  A second call through the C ABI with a workspace
    of exactly als_objective_workspace_bytes(0, n, k) bytes must succeed with the same bits."""
    n = G.sizes("gram")[which]
    assert (G.gram_rows_per_block(n) + G.gram_blocks(n)) * 2.0 ** -53 < 1e-13 / 2
    rng = np.random.default_rng(1000 * n + rank)
    A = rng.normal(0, 1, (n, rank)).astype(np.float32)
    B = rng.normal(0, 1, (n // 2, rank)).astype(np.float32)
    Ad, Bd = _gram_table(A), _gram_table(B)
    Ad[:, rank:] = float("nan")           # garbage past k in one table: masked, not assumed 0
    if Ad.shape[1] > rank + 1:
        Ad[:, rank + 1:] = 1e30
    L = _lib.lib()
    need = int(L.als_objective_workspace_bytes(0, n, rank))
    ws = E.Workspace(torch.device(DEV))
    assert ws.get(4 * need).numel() >= 4 * need                      # a roomy workspace
    dot, ga, gb = E.gram_dot(Ad, n, Bd, len(B), rank, ws, grams=True)
    dot2, ga2, gb2 = E.gram_dot(Ad, n, Bd, len(B), rank, ws, grams=True)
    assert torch.equal(ga, ga2) and torch.equal(gb, gb2) and torch.equal(dot, dot2)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    absA, absB = np.abs(A64).T @ np.abs(A64), np.abs(B64).T @ np.abs(B64)
    for name, Gm, F64, absG in (("A", ga, A64, absA), ("B", gb, B64, absB)):
        err = np.abs(Gm.cpu().numpy() - F64.T @ F64) / absG
        print(f"K10 gram n={len(F64)} k={rank}: worst error / sum|f_a f_b| = {err.max():.3e} "
              "(bar 1e-13)")
        report(f"grid_caps K10 gram n={len(F64)} k={rank}", err.max())
        assert err.max() <= 1e-13, (n, rank, name, err.max())
    want = float(((A64.T @ A64) * (B64.T @ B64)).sum())
    tol = 1e-12 * float((absA * absB).sum())
    assert abs(float(dot.item()) - want) <= tol, (n, rank, float(dot.item()), want, tol)
    # the C ABI with the workspace the header promises is enough, and not a byte more
    exact = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.empty(1, dtype=torch.float64, device=DEV)
    ga3, gb3 = torch.empty_like(ga), torch.empty_like(gb)
    rc = L.als_gram_dot_f64(Ad.data_ptr(), n, Bd.data_ptr(), len(B), Ad.shape[1], rank,
                            out.data_ptr(), ga3.data_ptr(), gb3.data_ptr(), exact.data_ptr(),
                            need, E.stream_ptr(torch.device(DEV)))
    assert rc == 0, L.als_last_error()
    torch.cuda.synchronize()
    assert torch.equal(ga3, ga) and torch.equal(gb3, gb) and torch.equal(out, dot)
