"""K9 on the GPU (als_rank_positions / als_full_rank_metrics) against the numpy fp64 oracle
tests/fullrank_ref.py.

1. Exact counts on integer factors (every product and sum exact, many genuine ties).
2. The band test on real-valued factors: tau = 2 * rank * 2^-24 * sum |q_d v_d| is the
   contract's bound, the kernel ships the fp32 fmaf chain whose own bound is half of it.
3. Agreement with K5's filtered top-16 lists.
4. Special rows (zero query, NaN rows of V, no query rows).
5. Bitwise reproducibility.
6. The public surfaces on a small implicit fit, a restored model, and TrainValidationSplit
   selecting an implicit fit by expected percentile rank.
"""
import math

import numpy as np
import pandas as pd
import pytest
import torch

import fullrank_ref as F
from als_mi355x import engine as E
from als_mi355x import filters

pytestmark = pytest.mark.gpu
DEV = "cuda"
PCT = ("expectedPercentileRank", "meanPercentileRank", "auc")


def _dev(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device=DEV, dtype=dtype)


def _padded(X, rank):
    out = np.zeros((len(X), E.ld_for(rank)), np.float32)
    out[:, :rank] = X
    return _dev(out, torch.float32)


def run_kernel(Q, V, rel, ex=None, allow=None, weights=None, per_row=False):
    """(above, tied, n_adm, sums, per_row) of K9 on host arrays, as numpy / lists."""
    rank, n_q, n_v = Q.shape[1], len(Q), len(V)
    rb, re_, rc = F.ranges(rel)
    args = [_dev(rb, torch.int64), _dev(re_, torch.int64), _dev(rc, torch.int32)]
    if ex is not None:
        eb, ee, ec = F.ranges(ex)
        args += [_dev(eb, torch.int64), _dev(ee, torch.int64), _dev(ec, torch.int32)]
    else:
        args += [None, None, None]
    args.append(None if allow is None else
                filters.pack_allow_bits(_dev(np.asarray(allow), torch.int64), n_v))
    above, tied, n_adm = E.rank_positions_rows(_padded(Q, rank), n_q, _padded(V, rank), n_v, rank,
                                               *args)
    n_ent = sum(len(x) for x in rel)
    w = None if weights is None else _dev(weights, torch.float32)
    sums, pr = E.full_rank_sums_rows(above, tied, n_adm, args[0], args[1],
                                     E.Workspace(torch.device(DEV)), w, per_row)
    return (above.cpu().numpy()[:n_ent], tied.cpu().numpy()[:n_ent], n_adm.cpu().numpy(),
            sums.cpu(), None if pr is None else pr.cpu().numpy())


def _filter_modes(rng, n_q, n_v, rel):
    ex = F.random_exclusions(rng, n_q, n_v, rel)
    allow = np.nonzero(rng.random(n_v) < 0.8)[0]
    return (("none", {}), ("exclude", dict(ex=ex)), ("allow", dict(allow=allow)),
            ("both", dict(ex=ex, allow=allow)))


def _check_exact(rng, rank, n_v, n_q, sizes, edit=None):
    """edit(rel, modes): changes the relevant sets and the filter modes' `ex` / `allow` in
    place before anything is computed from them."""
    Q, V = F.integer_factors(rng, n_q, rank), F.integer_factors(rng, n_v, rank)
    rel = F.random_relevant(rng, n_q, n_v, sizes)
    modes = _filter_modes(rng, n_q, n_v, rel)
    if edit is not None:
        edit(rel, dict(modes))
    seen_inadmissible = 0
    for name, kw in modes:
        ref = F.counts(Q, V, rel, **kw)
        above, tied, n_adm, sums, _ = run_kernel(Q, V, rel, **kw)
        np.testing.assert_array_equal(n_adm, ref["n_adm"], err_msg=f"n_adm, {name}")
        np.testing.assert_array_equal(above, ref["above"], err_msg=f"above, {name}")
        np.testing.assert_array_equal(tied, ref["tied"], err_msg=f"tied, {name}")
        want = F.sums(ref["above"], ref["tied"], ref["n_adm"], ref["row"])
        assert sums.tolist() == pytest.approx(want, rel=1e-12, abs=1e-12), name
        assert E.full_rank_dict(sums.tolist())["pairs"] == int((ref["above"] >= 0).sum())
        seen_inadmissible += int((ref["above"] < 0).sum())
    return seen_inadmissible


# every rank with some n_v / n_q, every n_v and every n_q with some rank
RANKS = (1, 7, 32, 33, 64, 65, 128)
NVS = (1, 15, 16, 17, 63, 64, 65, 257, 1031)
NQS = (1, 5, 17, 67)
SHAPES = sorted({(r, NVS[(3 * j + 2) % 9], NQS[j % 4]) for j, r in enumerate(RANKS)}
                | {(RANKS[(2 * j + 1) % 7], v, NQS[(j + 1) % 4]) for j, v in enumerate(NVS)}
                | {(RANKS[(j + 3) % 7], NVS[(2 * j + 4) % 9], q) for j, q in enumerate(NQS)})


def test_shape_list_covers_every_value():
    assert {s[0] for s in SHAPES} == set(RANKS)
    assert {s[1] for s in SHAPES} == set(NVS)
    assert {s[2] for s in SHAPES} == set(NQS)


@pytest.mark.parametrize("rank,n_v,n_q", SHAPES)
def test_exact_counts_on_integer_factors(rank, n_v, n_q):
    rng = np.random.default_rng(1000 * rank + 10 * n_v + n_q)
    sizes = rng.integers(0, min(n_v, 9) + 1, n_q)
    sizes[0] = min(1, n_v)
    if n_q > 1:
        sizes[1] = 0
    if n_q > 2:
        sizes[2] = n_v           # every row of V relevant: N == m without a filter
    inadmissible = _check_exact(rng, rank, n_v, n_q, sizes)
    if n_v >= 15 and n_q >= 5:
        assert inadmissible > 0  # relevant entries that are excluded / not allowed came back -1


def test_exact_counts_over_several_passes_of_a_workgroup():
    """67 rows of 100 relevant entries: a workgroup's rows hold more than the threshold table
    between them, so it sweeps V more than once and a row's entries straddle two sweeps."""
    table = E.rank_positions_table()
    rng = np.random.default_rng(77)
    assert 32 * 100 > table
    _check_exact(rng, 7, 1031, 67, np.full(67, 100))


def test_exact_counts_and_sums_over_more_than_256_partial_blocks():
    """1,029 query rows: 258 blocks of metric partials, the last holding one row, so the
    strided loop of the final sum (sum_partials_kernel) makes a second pass for threads 0
    and 1."""
    rng = np.random.default_rng(79)
    n_q, n_v = 1029, 65
    _check_exact(rng, 8, n_v, n_q, rng.integers(0, 10, n_q))


def test_exact_counts_for_a_row_larger_than_the_table():
    table = E.rank_positions_table()
    rng = np.random.default_rng(78)
    n_v = table + 150
    sizes = np.array([3, 0, table + 50, 1, 40])
    _check_exact(rng, 5, n_v, 5, sizes)


@pytest.mark.parametrize("n_v", [127, 128, 129, 256])
def test_exact_counts_at_the_sweep_tile_edges(n_v):
    """The sweep stages V in tiles of 128 rows: one row short of a tile, a full tile, one row
    into the second, two full tiles.  The allowed set is cut at the 32-bit words of the mask:
    rows 31 and 33 allowed and 32 not, 63 and 65 not and 64 allowed, and query row 0 holds all
    six as relevant entries."""
    edge = {31: True, 32: False, 33: True, 63: False, 64: True, 65: False}

    def edit(rel, modes):
        rel[0] = np.union1d(rel[0], list(edge)).astype(np.int64)
        allow = np.setdiff1d(np.union1d(modes["allow"]["allow"], [j for j in edge if edge[j]]),
                             [j for j in edge if not edge[j]])
        modes["allow"]["allow"] = modes["both"]["allow"] = allow

    rng = np.random.default_rng(n_v)
    n_q = 33
    assert _check_exact(rng, 9, n_v, n_q, rng.integers(0, 10, n_q), edit) >= 3


def _table_sizes(total, n_q=32):
    """n_q uneven row sizes that add up to `total`."""
    base = total // n_q
    sizes = np.full(n_q, base)
    d = np.arange(n_q // 2) % 9
    sizes[0::2] += d
    sizes[1::2] -= d
    sizes[-1] += total - int(sizes.sum())
    assert int(sizes.sum()) == total and sizes.min() > 0
    return sizes


@pytest.mark.parametrize("over", [0, 1])
def test_exact_counts_when_a_workgroup_fills_the_table_exactly(over):
    """The 32 rows of one workgroup hold exactly kRpTable relevant entries (one sweep, and the
    next pass finds nothing left), and one more (a second sweep for a single entry)."""
    table = E.rank_positions_table()
    sizes = _table_sizes(table + over)
    rng = np.random.default_rng(80 + over)
    _check_exact(rng, 7, int(sizes.max()) + 40, 32, sizes)


@pytest.mark.parametrize("tables", [1, 2])
def test_exact_counts_for_a_row_of_whole_tables(tables):
    """A single row of exactly kRpTable entries, and of exactly two tables' worth: its passes
    end on the table's last slot, and the rows after it wait for a pass of their own."""
    table = E.rank_positions_table()
    rng = np.random.default_rng(82 + tables)
    sizes = np.array([0, tables * table, 0, 0, 5 * (tables - 1)])
    _check_exact(rng, 5, tables * table + 10, 5, sizes)


def test_relevant_and_excluded_entries_outside_the_catalogue():
    """Relevant entries -1 and n_v come back as -1 and count as inadmissible; exclusion entries
    -1, n_v and n_v + 5 exclude nothing."""
    n_v, n_q = 129, 37

    def edit(rel, modes):
        for r in range(0, n_q, 3):
            rel[r] = np.concatenate([[-1], rel[r], [n_v]]).astype(np.int64)
        rel[1] = np.array([-1, n_v], np.int64)             # nothing but such entries
        ex = modes["exclude"]["ex"]
        for r in range(0, n_q, 2):
            ex[r] = np.concatenate([[-1, -1], ex[r], [n_v, n_v + 5]]).astype(np.int64)
        assert modes["both"]["ex"] is ex

    rng = np.random.default_rng(84)
    assert _check_exact(rng, 9, n_v, n_q, rng.integers(0, 10, n_q), edit) >= 4 * (2 * 13 + 1)


# ------------------------------------------------------------------ 2. band test
@pytest.fixture(scope="module", params=(10, 64, 128))
def real_case(request):
    rank = request.param
    rng = np.random.default_rng(20 + rank)
    n_q, n_v = 300, 1000
    Q = (rng.standard_normal((n_q, rank)) / math.sqrt(rank)).astype(np.float32)
    V = (rng.standard_normal((n_v, rank)) / math.sqrt(rank)).astype(np.float32)
    rel = F.random_relevant(rng, n_q, n_v, rng.integers(0, 21, n_q))
    ex = F.random_exclusions(rng, n_q, n_v, rel, mean=20)
    return Q, V, rel, ex, F.counts(Q, V, rel, ex=ex)


def test_band_on_real_valued_factors(real_case):
    Q, V, rel, ex, ref = real_case
    share = ref["banded"] / ref["compared"]
    print(f"rank {Q.shape[1]}: banded share {share:.3e} of {ref['compared']} comparisons")
    assert share < 1e-3          # the oracle alone: the bound leaves almost nothing undecided
    above, tied, n_adm, sums, _ = run_kernel(Q, V, rel, ex=ex)
    np.testing.assert_array_equal(n_adm, ref["n_adm"])
    ok = ref["above"] >= 0
    np.testing.assert_array_equal(above < 0, ~ok)
    np.testing.assert_array_equal(tied < 0, ~ok)
    assert (above[ok] >= ref["lo"][ok]).all()
    assert (above[ok] + tied[ok] <= ref["hi"][ok]).all()
    got = E.full_rank_dict(sums.tolist())
    want = F.metrics(ref["above"], ref["tied"], ref["n_adm"], ref["row"])
    tol = 2 * share + 1e-9
    for key in PCT:
        print(f"  {key}: kernel {got[key]:.12f} oracle {want[key]:.12f}")
        assert abs(got[key] - want[key]) <= tol, key
    assert (got["rows"], got["pairs"], got["inadmissible"]) == \
        (want["rows"], want["pairs"], want["inadmissible"])


def test_weights_and_per_row_values(real_case):
    Q, V, rel, ex, ref = real_case
    rng = np.random.default_rng(5)
    w = rng.integers(1, 6, len(ref["row"])).astype(np.float32)
    above, tied, n_adm, sums, per_row = run_kernel(Q, V, rel, ex=ex, weights=w, per_row=True)
    want = F.sums(above, tied, n_adm, ref["row"], w)       # the reduction alone, same counts
    assert sums.tolist() == pytest.approx(want, rel=1e-12, abs=1e-12)
    for r in (0, 1, 150, 299):
        mine = (ref["row"] == r) & (above >= 0)
        if not mine.any():
            assert np.isnan(per_row[r]).all()
            continue
        p = above[mine] + 0.5 * tied[mine]
        assert per_row[r, 0] == pytest.approx(p.mean() / (n_adm[r] - 1), rel=1e-12)
        assert per_row[r, 2] == pytest.approx(1 / (1 + p.min()), rel=1e-12)


# ------------------------------------------------------------------ 3. K5
def test_agreement_with_filtered_topk():
    rng = np.random.default_rng(9)
    n_q, n_v, rank = 37, 120, 33          # |q_0| * n_v < 2^10: the ramp breaks every tie
    Q, V = F.integer_factors(rng, n_q, rank), F.integer_factors(rng, n_v, rank)
    Q[Q[:, 0] == 0, 0] = 1.0
    V[:, 0] += np.arange(n_v, dtype=np.float32) * 2.0 ** -10
    s, _ = F.score_matrix(Q, V)
    assert all(len(np.unique(row)) == n_v for row in s)
    core = E.ALSCore.from_factors(np.arange(n_q), Q, np.arange(n_v), V)
    rel = F.random_relevant(rng, n_q, n_v, rng.integers(1, 30, n_q))
    ex = [np.setdiff1d(rng.integers(0, n_v, 25), rel[r]) for r in range(n_q)]
    ex_pairs = (np.concatenate([np.full(len(e), r) for r, e in enumerate(ex)]),
                np.concatenate(ex))
    users = np.concatenate([np.full(len(x), r) for r, x in enumerate(rel)])
    items = np.concatenate(rel)
    keys, ids, _ = core.recommend_subset(np.arange(n_q), 16, exclude=ex_pairs)
    out = core.full_rank_metrics(users, items, exclude=ex_pairs, positions=True)
    assert torch.equal(keys, out["keys"]) and out["inadmissible"] == 0
    ids = ids.cpu().numpy()
    row, col = out["row"].cpu().numpy(), out["col"].cpu().numpy()
    above, tied = out["above"].cpu().numpy(), out["tied"].cpu().numpy()
    assert (tied == 0).all()
    listed = 0
    for r, c, a in zip(row, col, above):
        where = np.nonzero(ids[r] == c)[0]
        if len(where):
            assert a == where[0]
            listed += 1
        else:
            assert a >= 16
    assert listed > n_q          # the lists do hold relevant items


# ------------------------------------------------------------------ 4. special rows
def test_special_rows():
    rng = np.random.default_rng(12)
    n_q, n_v, rank = 6, 70, 12
    Q = rng.standard_normal((n_q, rank)).astype(np.float32)
    V = rng.standard_normal((n_v, rank)).astype(np.float32)
    Q[2] = 0.0
    V[10] = np.nan
    V[65, 3] = np.nan
    rel = [np.array([4, 10, 30]), np.array([65]), np.array([1, 2, 3, 69]), np.array([], int),
           np.array([0]), np.array([9, 10, 11, 65, 66])]
    ref = F.counts(Q, V, rel)
    above, tied, n_adm, sums, per_row = run_kernel(Q, V, rel, per_row=True)
    assert (n_adm == n_v - 2).all() and (ref["n_adm"] == n_v - 2).all()
    np.testing.assert_array_equal(above, ref["above"])      # no near-ties in 6 x 70 normals
    np.testing.assert_array_equal(tied, ref["tied"])
    assert above[1] == -1 and above[3] == -1 and tied[1] == -1   # relevant rows that are NaN
    zero = ref["row"] == 2
    assert (above[zero] == 0).all() and (tied[zero] == n_v - 3).all()
    assert per_row[2, 0] == 0.5 and per_row[2, 1] == pytest.approx(0.5)
    assert np.isnan(per_row[3]).all() and np.isnan(per_row[1]).all()
    d = E.full_rank_dict(sums.tolist())
    assert (d["rows"], d["pairs"], d["inadmissible"]) == (4, 10, 4)


def test_no_query_rows_gives_zero_sums():
    dev = torch.device(DEV)
    sums = torch.full((11,), 7.0, dtype=torch.float64, device=dev)
    L = E._lib.lib()
    assert L.als_full_rank_metrics(0, 0, 0, 0, 0, 0, 0, sums.data_ptr(), 0, 0, 0,
                                   E.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    assert sums.tolist() == [0.0] * 11
    core = E.ALSCore.from_factors(np.array([1, 2]), np.ones((2, 3), np.float32),
                                  np.array([5, 6, 7]), np.ones((3, 3), np.float32))
    d = core.full_rank_metrics([9, 9], [5, 8], per_row=True, positions=True)   # unknown ids
    assert d["rows"] == 0 and d["dropped"] == 2 and math.isnan(d["expectedPercentileRank"])
    assert d["per_row"].shape == (0, 3) and d["above"].numel() == 0


# ------------------------------------------------------------------ 5. reproducibility
def test_two_calls_give_identical_bits(real_case):
    Q, V, rel, ex, _ = real_case
    a = run_kernel(Q, V, rel, ex=ex, per_row=True)
    b = run_kernel(Q, V, rel, ex=ex, per_row=True)
    assert torch.equal(a[3], b[3])
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a[4].view(np.int64), b[4].view(np.int64))


# ------------------------------------------------------------------ 6. surfaces
@pytest.fixture(scope="module")
def implicit_data():
    """300 users x 200 items of planted counts in four taste groups (a user takes an item of
    its own group with probability 0.3, any other with 0.02), one pair in five held out."""
    rng = np.random.default_rng(31)
    n_u, n_i = 300, 200
    same = rng.integers(0, 4, n_u)[:, None] == rng.integers(0, 4, n_i)[None, :]
    mask = rng.random((n_u, n_i)) < np.where(same, 0.3, 0.02)
    mask[np.arange(n_u), rng.integers(0, n_i, n_u)] = True
    mask[rng.integers(0, n_u, n_i), np.arange(n_i)] = True
    u, i = np.nonzero(mask)
    r = (1 + rng.poisson(1.5, len(u))).astype(np.float32)
    df = pd.DataFrame({"user": (3 * u + 1).astype(np.int32), "item": (2 * i).astype(np.int32),
                       "rating": r})
    held = rng.random(len(df)) < 0.2
    return df[~held].reset_index(drop=True), df[held].reset_index(drop=True)


IMPLICIT = dict(rank=8, maxIter=5, regParam=0.05, alpha=10.0, implicitPrefs=True, seed=3,
                coldStartStrategy="drop")


def _oracle_of(core, valid, train):
    """The oracle's metric dict and banded share on a core's fitted factors."""
    uids, U = core.user_factors()
    iids, V = core.item_factors()
    uids, iids = uids.cpu().numpy(), iids.cpu().numpy()
    U, V = U.cpu().numpy(), V.cpu().numpy()
    urow = {int(x): r for r, x in enumerate(uids)}
    irow = {int(x): r for r, x in enumerate(iids)}

    def lists(df, rows):
        out = {r: set() for r in rows}
        for a, b in zip(df["user"], df["item"]):
            if int(a) in urow and int(b) in irow and urow[int(a)] in out:
                out[urow[int(a)]].add(irow[int(b)])
        return [np.array(sorted(out[r]), np.int64) for r in rows]
    rows = sorted({urow[int(a)] for a, b in zip(valid["user"], valid["item"])
                   if int(a) in urow and int(b) in irow})
    rel, ex = lists(valid, rows), lists(train, rows)
    ref = F.counts(U[rows], V, rel, ex=ex)
    return (F.metrics(ref["above"], ref["tied"], ref["n_adm"], ref["row"]),
            ref["banded"] / ref["compared"])


def _close(got, want, tol):
    for key in PCT:
        assert abs(got[key] - want[key]) <= tol, (key, got[key], want[key])
    for key in ("rows", "pairs", "inadmissible"):
        assert got[key] == want[key]


def test_public_surfaces_on_an_implicit_fit(implicit_data, tmp_path):
    from als_mi355x.ml.recommendation import ALS, ALSModel
    from als_mi355x.mllib.recommendation import ALS as MLlibALS
    from als_mi355x.mllib.recommendation import MatrixFactorizationModel
    train, valid = implicit_data
    model = ALS(**IMPLICIT).fit(train)
    got = model.evaluateFullRanking(valid, exclude="train")
    want, share = _oracle_of(model.engine, valid, train)
    tol = 2 * share + 1e-9
    print(f"ml: {got}\noracle: {want}\nbanded share {share:.3e}")
    assert share < 1e-3
    _close(got, want, tol)
    # the held-out pairs are mostly in-group (0.3 x 1/4 against 0.02 x 3/4), and a fit that
    # found the groups puts an in-group item in the top quarter: well clear of random's 0.5
    assert got["expectedPercentileRank"] < 0.4 and got["auc"] > 0.6
    eng = model.engine.full_rank_metrics(valid["user"].to_numpy(), valid["item"].to_numpy(),
                                         exclude="train")
    assert eng == got
    # equal weights change nothing; the ratings as weights do
    ones = valid.assign(rating=np.float32(2.0))
    same = model.evaluateFullRanking(ones, weighted=True, exclude="train")
    assert same["expectedPercentileRank"] == pytest.approx(got["expectedPercentileRank"],
                                                           rel=1e-12)
    weighted = model.evaluateFullRanking(valid, weighted=True, exclude="train")
    assert weighted["meanPercentileRank"] == got["meanPercentileRank"]
    assert weighted["expectedPercentileRank"] != got["expectedPercentileRank"]
    # a threshold keeps the pairs at or above it
    few = model.evaluateFullRanking(valid, ratingThreshold=3.0, exclude="train")
    n_few = int((valid["rating"] >= 3.0).sum())
    assert n_few - got["dropped"] <= few["pairs"] <= n_few < got["pairs"]
    # a restored model has no training pairs of its own
    path = str(tmp_path / "model")
    model.save(path)
    back = ALSModel.load(path)
    assert back.evaluateFullRanking(valid, exclude=train) == got
    with pytest.raises(ValueError, match="from_factors"):
        back.evaluateFullRanking(valid, exclude="train")
    # mllib: its own fit, its own oracle
    triples = list(zip(train["user"].tolist(), train["item"].tolist(), train["rating"].tolist()))
    mf = MLlibALS.trainImplicit(triples, 8, iterations=5, lambda_=0.05, alpha=10.0, seed=3)
    held = list(zip(valid["user"].tolist(), valid["item"].tolist(), valid["rating"].tolist()))
    got2 = mf.fullRankingMetrics(held, exclude="train")
    want2, share2 = _oracle_of(mf.engine, valid, train)
    _close(got2, want2, 2 * share2 + 1e-9)
    mpath = str(tmp_path / "mllib")
    mf.save(None, mpath)
    back2 = MatrixFactorizationModel.load(None, mpath)
    pairs = list(zip(train["user"].tolist(), train["item"].tolist()))
    assert back2.fullRankingMetrics(held, exclude=pairs) == got2
    with pytest.raises(ValueError, match="from_factors"):
        back2.fullRankingMetrics(held, exclude="train")


def test_train_validation_split_selects_an_implicit_fit(implicit_data):
    from als_mi355x.ml.evaluation import FullRankingEvaluator
    from als_mi355x.ml.recommendation import ALS
    from als_mi355x.ml.tuning import ParamGridBuilder, TrainValidationSplit
    train, valid = implicit_data
    data = pd.concat([train, valid], ignore_index=True)
    regs = (0.05, 50.0)
    base = {k: v for k, v in IMPLICIT.items() if k != "regParam"}
    grid = ParamGridBuilder().addGrid(ALS.regParam, regs).build()
    tvs = TrainValidationSplit(ALS(**base), grid, FullRankingEvaluator(), trainRatio=0.8, seed=2)
    out = tvs.fit(data)
    tr, va = tvs.split(len(data))
    hand = [ALS(regParam=reg, **base).fit(data.iloc[tr])
            .evaluateFullRanking(data.iloc[va], exclude="train")["expectedPercentileRank"]
            for reg in regs]
    print(f"expected percentile rank by regParam {dict(zip(regs, hand))}")
    assert out.validationMetrics == pytest.approx(hand, rel=1e-12)
    assert abs(hand[0] - hand[1]) > 1e-3          # the two fits do differ
    best = regs[int(np.argmin(hand))]             # lower is better
    assert out.bestModel._p["regParam"] == best
