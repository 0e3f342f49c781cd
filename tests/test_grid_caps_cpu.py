"""The arithmetic behind the grid-cap tests (tests/grid_caps.py), without a GPU.

1. The caps are found in the sources, and the test sizes derived from them do what
   test_gpu_grid_caps.py needs: the grid sits at its cap and the row groups exceed it.
2. K10: gram_partial_doubles(m, k) <= gram_partial_doubles_bound(n, k) for every m <= n, the
   claim als_objective_workspace_bytes rests on (objective.hip argues it in a comment only).
3. The vectorised references agree with the loops of ranking_ref / fullrank_ref /
   list_metrics_ref on a prefix of the very inputs the GPU tests use: bit for bit where the
   GPU tests ask for bits (K6's four columns, every count), 1e-14 relative elsewhere.
"""
import numpy as np
import pytest

import fullrank_ref as F
import grid_caps as G
import list_metrics_ref as LR
import ranking_ref as R
from als_mi355x import _lib

PREFIX = 1000


# ------------------------------------------------------------------ 1. caps and sizes
def test_every_cap_is_found_in_the_sources():
    c = G.constants()
    assert set(c) == set(G.CONSTANTS) | {"lcItemsPerBlock"}
    assert all(isinstance(v, int) and v >= 1 for v in c.values()), c
    assert c["kGramMinRows"] % 4 == 0


def test_a_pattern_that_no_longer_matches_raises_a_clear_error():
    with pytest.raises(LookupError, match="kRmMaxBlocks.*update tests/grid_caps.py"):
        G.read_constant("constexpr int kRmBlocks = 4096;", "kRmMaxBlocks")
    with pytest.raises(LookupError, match="kRmMaxBlocks"):
        G.read_constant("constexpr int kRmMaxBlocks = 16 * 256;", "kRmMaxBlocks")
    with pytest.raises(LookupError, match="lc_blocks"):
        G.read_lc_items_per_block("static inline int64_t lc_blocks(int64_t n_v) {\n"
                                  "  return n_v / 2048;\n}\n")
    assert G.read_lc_items_per_block("static inline int64_t lc_blocks(int64_t n_v) {\n"
                                     "  const int64_t g = (n_v + 1023) / 1024;\n}\n") == 1024


@pytest.mark.parametrize("kernel,blocks,per,cap", [
    ("rank_metrics", G.rm_blocks, "kRmRowsPerBlock", "kRmMaxBlocks"),
    ("full_rank_metrics", G.fr_blocks, "kFrRowsPerBlock", "kFrMaxBlocks"),
    ("novelty", G.ln_blocks, "kLnRowsPerBlock", "kLnMaxBlocks"),
    ("concentration", G.lc_blocks, "lcItemsPerBlock", "kLcMaxBlocks")])
def test_row_group_sizes_sit_at_and_past_the_cap(kernel, blocks, per, cap):
    c = G.constants()
    per, cap = c[per], c[cap]
    n0, n1, n5, n2 = G.sizes(kernel)
    assert n0 == G.cap_rows(kernel) == per * cap
    assert blocks(n0 - 1) == cap and blocks(n0 - per) == cap - 1   # the cap is first met at n0
    for n in (n0, n1, n5, n2):
        assert blocks(n) == cap
    assert G.groups(n0, per) == cap                  # no second trip
    assert G.groups(n1, per) == cap + 1              # block 0 alone makes a second trip
    assert n1 - cap * per == 1                       # ... for one row: its other waves skip
    if per == 4:
        assert G.groups(n5, per) == cap + 2 and n5 - (cap + 1) * per == 1
    assert G.groups(n2, per) == 2 * cap + 1          # block 0 makes three trips
    assert blocks(0) == 1 and blocks(1) == 1


def test_exposure_sizes_sit_at_and_past_the_cap():
    c = G.constants()
    at, nb = G.EXPOSURE_AT, c["kLxMaxBlocks"]
    rpc = G.lx_rows_per_chunk(at)
    assert rpc == c["kLxChunkEntries"] // at >= 1 and rpc * at < 2 ** 31
    n0, n1, n2 = G.exposure_sizes()
    assert [G.lx_chunks(n, at) for n in (n0, n1, n2)] == [nb, nb + 1, 2 * nb + 1]
    assert [G.lx_blocks(n, at) for n in (n0 - rpc, n0, n1, n2)] == [nb - 1, nb, nb, nb]
    assert G.lx_rows_per_chunk(257 * c["kLxChunkEntries"]) == 1


def test_gram_sizes_change_the_rows_per_block():
    c = G.constants()
    n0, n1, n5, _ = G.sizes("gram")
    assert G.gram_rows_per_block(n0) == c["kGramMinRows"] and G.gram_blocks(n0) == c["kGramMaxBlocks"]
    for n in (n1, n5):
        rpb, nb = G.gram_rows_per_block(n), G.gram_blocks(n)
        assert rpb > c["kGramMinRows"] and rpb % 4 == 0 and nb <= c["kGramMaxBlocks"]
        tail = n - (nb - 1) * rpb
        assert 0 < tail <= rpb and tail % 4 != 0     # the last block ends inside a step of 4
        print(f"gram n={n}: {nb} blocks of {rpb} rows, the last of {tail}")


# ------------------------------------------------------------------ 2. the Gram workspace
@pytest.mark.parametrize("k", [1, 16, 17, 128])
def test_gram_partials_never_exceed_the_bound_of_a_larger_table(k):
    ns = np.arange(1, 40001)
    need = np.array([G.gram_partial_doubles(int(n), k) for n in ns])
    bound = np.array([G.gram_partial_doubles_bound(int(n), k) for n in ns])
    assert (np.diff(bound) >= 0).all()               # the bound is monotone ...
    assert (np.diff(need) < 0).any()                 # ... the need is not: why there is a bound
    # need(m) <= bound(n) for every m <= n  <=>  the running maximum of need stays under bound
    assert (np.maximum.accumulate(need) <= bound).all()
    blocks = np.array([G.gram_blocks(int(n)) for n in ns])
    rpb = np.array([G.gram_rows_per_block(int(n)) for n in ns])
    assert (blocks * rpb >= ns).all() and ((blocks - 1) * rpb < ns).all()   # every row, no empty block


def test_gram_restatement_matches_the_library():
    L = _lib.lib()
    for k in (1, 16, 17, 128):
        for n in (0, 1, 63, 64, 65, 16384, 16385, 16389, 40000):
            assert L.als_objective_workspace_bytes(0, n, k) == G.objective_workspace_bytes_gram(n, k)


# ------------------------------------------------------------------ 3. the references
@pytest.mark.parametrize("at", [10, 65])
def test_rank_rows_equals_the_loop_bit_for_bit(at):
    from test_gpu_rank_metrics import pattern_inputs
    n = PREFIX + 37
    lists, begin, end, col, rows = pattern_inputs(at, n)
    got = G.rank_rows(lists, begin, end, col, at)
    want = R.per_row(rows[:PREFIX], at)
    assert got[:PREFIX].tobytes() == want.tobytes()
    assert got.shape == (n, 4) and (got[3] == 1.0).all() and (got[:2] == 0.0).all()
    # the wide form K6 is given (a relevant id past `at`) changes nothing
    wide = np.concatenate([lists, col[np.minimum(begin, len(col) - 1)][:, None]], axis=1)
    assert G.rank_rows(wide, begin, end, col, at).tobytes() == got.tobytes()


@pytest.mark.parametrize("weighted", [False, True])
def test_full_rank_sums_equal_the_loop(weighted):
    n_q = PREFIX + 29
    above, tied, n_adm, begin, end, w = G.full_rank_inputs(n_q, weighted=weighted)
    lens = end - begin
    assert set(lens.tolist()) == {0, 1, 3, 70}
    assert ((n_adm == 1) & (lens > 0)).any() and ((n_adm == lens) & (lens > 1)).any()
    assert (above < 0).any() and (above >= 0).any()
    row = np.repeat(np.arange(n_q), lens)
    got, per_row = G.full_rank_sums(above, tied, n_adm, begin, end, w)
    want = F.sums(above, tied, n_adm, row, w)
    for j, name in enumerate(F.SUMS):
        if name in ("auc_rows", "rr_rows", "rows", "pairs", "inadmissible", "pr_rows"):
            assert got[j] == want[j], name
        else:
            assert got[j] == pytest.approx(want[j], rel=1e-14, abs=0), name
    assert got[9] > 0 and got[4] < got[7] and got[10] < got[7]      # every branch is taken
    # per row, against the definitions on a few rows of each kind
    for r in list(range(8)) + [52, n_q - 1]:
        mine = (row == r) & (above >= 0)
        if not mine.any():
            assert np.isnan(per_row[r]).all()
            continue
        p = above[mine] + 0.5 * tied[mine]
        m, N = float(mine.sum()), float(n_adm[r])
        assert per_row[r, 2] == 1.0 / (1.0 + p.min())
        if N > 1:
            assert per_row[r, 0] == pytest.approx(p.sum() / (N - 1) / m, rel=1e-14)
        else:
            assert np.isnan(per_row[r, 0])
        if N > m:
            want_auc = 1.0 - (p.sum() - 0.5 * m * (m - 1)) / (m * (N - m))
            assert per_row[r, 1] == pytest.approx(want_auc, rel=1e-14)
        else:
            assert np.isnan(per_row[r, 1])
    # a prefix of the rows is a prefix of the ranges
    cut = int(end[PREFIX - 1])
    pre, _ = G.full_rank_sums(above[:cut], tied[:cut], n_adm[:PREFIX], begin[:PREFIX],
                              end[:PREFIX], None if w is None else w[:cut])
    want = F.sums(above[:cut], tied[:cut], n_adm[:PREFIX], row[:cut], None if w is None else w[:cut])
    assert pre == pytest.approx(want, rel=1e-14, abs=0)


def test_novelty_equals_the_loop():
    n_q, at = PREFIX + 27, 10
    idx, pop, allow, tail = G.novelty_inputs(n_q, at)
    for bits, t in ((None, tail), (allow, tail), (None, None)):
        got_s, got_r = G.novelty(idx, at, 1200, pop, 4321, bits, t)
        want_s, want_r = LR.novelty(idx[:PREFIX], at, 1200, pop, 4321, bits, t)
        assert (np.isnan(got_r[:PREFIX]) == np.isnan(want_r)).all()
        np.testing.assert_allclose(got_r[:PREFIX], want_r, rtol=1e-14, atol=0, equal_nan=True)
        # mean popularity and long-tail share are one division of two integers
        assert np.array_equal(got_r[:PREFIX, 1:], want_r[:, 1:], equal_nan=True)
        pre_s, _ = G.novelty(idx[:PREFIX], at, 1200, pop, 4321, bits, t)
        np.testing.assert_allclose(pre_s, want_s, rtol=1e-14, atol=0)
        assert [pre_s[i] for i in (1, 3, 5, 6)] == [want_s[i] for i in (1, 3, 5, 6)]
    assert np.isnan(got_r[0]).all() and np.isnan(got_r[2, 0]) and got_r[2, 1] == 0.0
