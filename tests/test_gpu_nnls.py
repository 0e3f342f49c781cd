"""Nonnegative ALS (K13, als_nnls_rows) on the GPU: the kernel against the fp64 restatement of
Spark's NNLS solver (tests/nnls_ref.py), its KKT residual, padding, determinism, chunked long
rows, the early stop, the fit, fold-in and the public surfaces.

Bars (per case of the grid):
  1. every output >= 0 exactly, padding exactly 0, nothing of the 7.0 prefill left, n_used exact;
  2. per-row relative error <= 1e-4 against nnls_ref (the project's bar);
  3. the KKT residual of each GPU row (fp64, on its fp32 values) <= 4 x the largest residual of
     the reference's own fp32-rounded rows of that case: the two runs may stop one iteration
     apart on the same contraction (tests/test_nnls_cpu.py asserts the yardstick is > 0);
  4. two calls are bit-identical.
Measured maxima (MI355X): DESIGN.md section K13.
"""
import functools

import numpy as np
import pytest
import torch

import nnls_ref as R
from als_mi355x import engine as E
from helpers import nnls_sources, ragged_csr, rel_row_errs, report
from oracle import als_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_SRC = 200
REG = 0.1
ALPHA = 40.0
RANKS = (1, 3, 16, 17, 33, 64, 65, 100, 128)
MODES = pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
SOURCES = pytest.mark.parametrize("signed", [True, False], ids=["signed", "abs"])


# ------------------------------------------------------------------ helpers
_sources = nnls_sources   # unit-norm rows of N_SRC sources, signed or their absolute values


def _rows(k, seed=0):
    """Lengths 0, 1, 2, k - 1, k, k + 1, 300, one row of one repeated item, one mixing valid
    entries with col = -1 and col = n_src."""
    rng = np.random.default_rng(60 + k + seed)
    rows = [(rng.integers(0, N_SRC, n), rng.integers(1, 6, n))
            for n in (0, 1, 2, k - 1, k, k + 1, 300)]
    rows.append((np.full(40, 17), rng.integers(1, 6, 40)))
    mixed = rng.integers(0, N_SRC, 30)
    mixed[::3] = -1
    mixed[1::3] = N_SRC
    rows.append((mixed, rng.integers(1, 6, 30)))
    return rows


_csr = ragged_csr


def _dev(M, ld=None, fill=0.0):
    k = M.shape[1]
    out = torch.full((M.shape[0], ld or E.ld_for(k)), fill, dtype=torch.float32, device=DEV)
    out[:, :k] = torch.as_tensor(M).to(DEV)
    return out


def _run(rows, Y, k, implicit, chunk=E.DEFAULT_CHUNK, ld=None, fill=0.0, reg=REG, alpha=ALPHA):
    """One als_nnls_rows call over `rows` against Y stored with leading dimension ld (padding
    columns = fill), the output prefilled with 7.0.  Returns (X [n, ld_out], n_used, iters)."""
    ptr, col, val = _csr(rows)
    t = lambda a, d: torch.as_tensor(a).to(DEV, d).contiguous()
    ws = E.Workspace(torch.device(DEV))
    yty = E.compute_yty(_dev(Y), N_SRC, k, ws) if implicit else None
    X = torch.full((len(rows), E.ld_for(k) + 4), 7.0, dtype=torch.float32, device=DEV)
    X, n_used, it = E.nnls_rows(t(ptr, torch.int64), t(col, torch.int32), t(val, torch.float32),
                                _dev(Y, ld, fill), N_SRC, k, reg, implicit, alpha, yty, ws,
                                chunk, X=X, iters=True)
    torch.cuda.synchronize()
    return X.cpu().numpy(), n_used.cpu().numpy(), it.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(k, signed, implicit):
    """(Y, rows, A, b, n_used, reference rows fp32, reference iterations): computed once."""
    Y, rows = _sources(k, signed), _rows(k)
    ptr, col, val = _csr(rows)
    A, b, used = R.systems(ptr, col, val, Y, REG, implicit, ALPHA)
    its, ref = [], np.zeros(b.shape, np.float32)
    for r in range(len(rows)):
        info = {}
        ref[r] = R.nnls_solve(A[r], b[r], info).astype(np.float32)
        its.append(info["iters"])
    for a in (A, b, used, ref):
        a.setflags(write=False)
    return Y, rows, A, b, used, ref, np.array(its)


# ------------------------------------------------------------------ the kernel, bars 1-4
@MODES
@SOURCES
@pytest.mark.parametrize("k", RANKS)
def test_kernel_against_the_reference(k, signed, implicit):
    Y, rows, A, b, used, ref, ref_it = _case(k, signed, implicit)
    X, n_used, it = _run(rows, Y, k, implicit)
    # bar 1
    assert (X[:, :k] >= 0).all()
    assert (X[:, k:] == 0).all() and not (X == 7.0).any()
    np.testing.assert_array_equal(n_used, used)
    empty = used == 0
    assert (X[empty] == 0).all() and (it[empty] == 0).all()
    assert (it <= max(400, 20 * k)).all()
    # bar 2
    errs = rel_row_errs(X[:, :k], ref)
    tag = f"k={k},signed={signed},implicit={implicit}"
    print(f"nnls parity {tag}: max rel row err {errs.max():.3e}; iterations GPU {it.tolist()} "
          f"reference {ref_it.tolist()}; on the wall {(ref == 0).sum(1).tolist()}")
    report(f"nnls_parity[{tag}]", float(errs.max()))
    # bar 3
    yard = max(R.kkt(A[r], b[r], ref[r]) for r in range(len(rows)))
    got = max(R.kkt(A[r], b[r], X[r, :k]) for r in range(len(rows)))
    print(f"nnls kkt {tag}: GPU {got:.3e} reference {yard:.3e} ratio {got / yard:.3f}")
    report(f"nnls_kkt_ratio[{tag}]", float(got / yard))
    assert errs.max() <= 1e-4
    assert yard > 0
    assert got <= 4 * yard
    # bar 4
    X2, n2, it2 = _run(rows, Y, k, implicit)
    assert X.tobytes() == X2.tobytes() and it.tobytes() == it2.tobytes()


@MODES
@pytest.mark.parametrize("k", RANKS)
def test_padding_columns_of_the_sources_are_ignored(k, implicit):
    """NaN in columns [k, ld) of Y_src changes nothing: the same bits as with zeros there."""
    Y, rows = _sources(k, True), _rows(k)
    ld = E.ld_for(k) if E.ld_for(k) > k else k + 4
    X0, n0, it0 = _run(rows, Y, k, implicit, ld=ld, fill=0.0)
    X1, n1, it1 = _run(rows, Y, k, implicit, ld=ld, fill=float("nan"))
    assert np.isfinite(X1).all()
    assert X0.tobytes() == X1.tobytes() and it0.tobytes() == it1.tobytes()
    np.testing.assert_array_equal(n0, n1)


# ------------------------------------------------------------------ long rows
@functools.lru_cache(maxsize=None)
def _long_case(k, implicit):
    Y = _sources(k, True, seed=1)
    rng = np.random.default_rng(80 + k)
    rows = [(rng.integers(0, N_SRC, n), rng.integers(1, 6, n))
            for n in (63, 64, 65, 129, 130, 1000)]
    unknown = rng.integers(0, N_SRC, 200)     # a chunked row with unknown columns in every task
    unknown[::5] = -1
    rows.append((unknown, rng.integers(1, 6, 200)))
    ptr, col, val = _csr(rows)
    ref = R.solve_rows(ptr, col, val, Y, REG, implicit, ALPHA)
    ref.setflags(write=False)
    return Y, rows, ref


@MODES
@pytest.mark.parametrize("k", [16, 64, 128])
def test_chunked_rows(k, implicit):
    Y, rows, ref = _long_case(k, implicit)
    Xc, nc, _ = _run(rows, Y, k, implicit, chunk=64)
    Xw, nw, _ = _run(rows, Y, k, implicit, chunk=4096)
    e_ref = rel_row_errs(Xc[:, :k], ref)
    e_one = rel_row_errs(Xc[:, :k], Xw[:, :k])
    print(f"nnls chunked k={k} implicit={implicit}: vs reference {e_ref.max():.3e}, "
          f"chunk 64 vs 4096 {e_one.max():.3e}")
    report(f"nnls_chunked[k={k},implicit={implicit}]", [float(e_ref.max()), float(e_one.max())])
    np.testing.assert_array_equal(nc, nw)
    assert nc.tolist() == [63, 64, 65, 129, 130, 1000, 160]
    assert (Xc[:, :k] >= 0).all() and (Xc[:, k:] == 0).all()
    assert e_ref.max() <= 1e-4
    assert e_one.max() <= 1e-6
    X2, _, _ = _run(rows, Y, k, implicit, chunk=64)
    assert Xc.tobytes() == X2.tobytes()


def test_more_rows_than_blocks():
    """Past 65,536 rows the workgroups stride over the row list."""
    k = 4
    Y = _sources(k, True)
    base = _rows(k)[:7]
    reps = 65536 // len(base) + 3
    rows = base * reps
    ptr, col, val = _csr(base)
    ref = R.solve_rows(ptr, col, val, Y, REG)
    X, n_used, _ = _run(rows, Y, k, False)
    assert len(rows) > 65536
    X = X[:, :k].reshape(reps, len(base), k)
    assert (X == X[0]).all()
    assert rel_row_errs(X[0], ref).max() <= 1e-4
    assert n_used.reshape(reps, len(base)).tolist() == [[len(c) for c, _ in base]] * reps


# ------------------------------------------------------------------ rows that end at zero
def test_early_stop_and_zero_rhs_rows_are_exactly_zero():
    k = 8
    rng = np.random.default_rng(9)
    Y = _sources(k, True) * np.float32(1e4)
    rows = [(rng.integers(0, N_SRC, 16), rng.integers(1, 6, 16))]
    ptr, col, val = _csr(rows)
    A, b, _ = R.systems(ptr, col, val, Y, REG)
    info = {}
    assert (R.nnls_solve(A[0], b[0], info) == 0).all() and 0 < info["first_step"] < 1e-8
    X, n_used, it = _run(rows, Y, k, False)
    assert (X == 0).all() and n_used.tolist() == [16] and it.tolist() == [0]
    # b = 0 with used entries: explicit zero ratings; implicit without a positive rating
    Y = _sources(k, True)
    cols = rng.integers(0, N_SRC, 12)
    X, n_used, it = _run([(cols, np.zeros(12))], Y, k, False)
    assert (X == 0).all() and n_used.tolist() == [12] and it.tolist() == [0]
    X, n_used, it = _run([(cols, -np.ones(12)), (cols, np.zeros(12))], Y, k, True)
    assert (X == 0).all() and n_used.tolist() == [12, 12] and it.tolist() == [0, 0]


# ------------------------------------------------------------------ the fit
@functools.lru_cache(maxsize=None)
def _ratings():
    rng = np.random.default_rng(11)
    n_u, n_i, nnz = 300, 200, 6000
    u = np.concatenate([np.arange(n_u), rng.integers(0, n_u, nnz - n_u - n_i), rng.integers(0, n_u, n_i)])
    i = np.concatenate([rng.integers(0, n_i, n_u), rng.integers(0, n_i, nnz - n_u - n_i), np.arange(n_i)])
    r = np.clip(np.round(3.5 + rng.normal(0, 1, nnz)), 1, 5).astype(np.float32)
    return u.astype(np.int32), i.astype(np.int32), r


@functools.lru_cache(maxsize=None)
def _ref_fit(k, implicit):
    u, i, r = _ratings()
    U0 = O.initialize(300, k, 5)
    hist = []
    R.fit(u, i, r, k, 5, REG, implicit, ALPHA if implicit else 1.0, U0=U0, history=hist)
    return U0, hist


@pytest.mark.parametrize("k,implicit", [(4, False), (8, False), (12, False), (8, True)])
def test_fit_against_the_reference_fit(k, implicit):
    u, i, r = _ratings()
    U0, hist = _ref_fit(k, implicit)
    alpha = ALPHA if implicit else 1.0
    core = E.ALSCore(u, i, r)
    core.init_factors(k, U0=U0)
    worst = 0.0
    for t in range(5):
        core.iterate(REG, implicit, alpha, nonnegative=True)
        U, V = core.U[:, :k].cpu().numpy(), core.V[:, :k].cpu().numpy()
        assert (U >= 0).all() and (V >= 0).all()
        err = max(rel_row_errs(U, hist[t][0]).max(), rel_row_errs(V, hist[t][1]).max())
        print(f"nnls fit k={k} implicit={implicit} iteration {t + 1}: max rel row err {err:.3e}")
        worst = max(worst, err)
        assert err <= 1e-4
    report(f"nnls_fit[k={k},implicit={implicit}]", worst)
    assert (core.U[:, k:] == 0).all() and (core.V[:, k:] == 0).all()
    # the same through fit(), with the objective observed
    core.fit(k, 5, REG, implicit, alpha, U0=U0, objective_every=1, nonnegative=True)
    np.testing.assert_array_equal(core.U[:, :k].cpu().numpy(), U)
    assert [it for it, _ in core.objective_history] == [1, 2, 3, 4, 5]
    vals = [v for _, v in core.objective_history]
    scale = core.objective(REG, implicit, alpha)["scale"]
    print(f"nnls fit k={k} implicit={implicit}: objective {vals}, scale {scale:.6e}")
    for a, b in zip(vals, vals[1:]):
        assert b - a <= 1e-9 * scale
    # the Cholesky path is untouched by the flag being off
    core.fit(k, 1, REG, implicit, alpha, U0=U0)
    assert (core.U[:, :k].cpu().numpy() < 0).any()


def test_fit_refuses_a_checkpoint_directory(tmp_path):
    u, i, r = _ratings()
    core = E.ALSCore(u, i, r)
    with pytest.raises(ValueError, match="checkpoint"):
        core.fit(4, 1, REG, nonnegative=True, checkpoint_dir=str(tmp_path))


# ------------------------------------------------------------------ fold-in and the surfaces
def test_fold_in_returns_the_fitted_users():
    u, i, r = _ratings()
    k = 8
    core = E.ALSCore(u, i, r)
    core.fit(k, 3, REG, seed=5, nonnegative=True)
    U = core.U[:, :k].cpu().numpy()
    keys, X, n_used = core.fold_in(u, i, r, reg=REG, nonnegative=True)
    assert keys.cpu().numpy().tolist() == list(range(300))
    errs = rel_row_errs(X.cpu().numpy(), U)
    print(f"nnls fold-in of the training users: max rel row err {errs.max():.3e}")
    assert errs.max() <= 1e-5
    assert (n_used.cpu().numpy() == np.bincount(u, minlength=300)).all()
    # a serving-only core gives the same rows, and the Cholesky fold-in differs
    serve = E.ALSCore.from_factors(core.uidx.ids(), core.U[:, :k], core.iidx.ids(), core.V[:, :k])
    _, X2, _ = serve.fold_in(u, i, r, reg=REG, nonnegative=True)
    assert torch.equal(X, X2)
    _, X3, _ = serve.fold_in(u, i, r, reg=REG)
    assert not torch.equal(X, X3)
    # recommend_new follows the folded rows
    sel = u < 5
    keys, ids, sc = serve.recommend_new(u[sel], i[sel], r[sel], 10, reg=REG, nonnegative=True)
    assert keys.cpu().numpy().tolist() == [0, 1, 2, 3, 4]
    best = (X[:5] @ serve.V[:, :k].T).cpu().numpy()
    rated = np.zeros_like(best, bool)
    rated[u[sel], i[sel]] = True
    best[rated] = -np.inf
    np.testing.assert_allclose(sc.cpu().numpy()[:, 0], best.max(1), rtol=1e-5)
    assert (sc.cpu().numpy() >= 0).all()


def test_ml_and_mllib_surfaces():
    import pandas as pd
    from als_mi355x.ml.recommendation import ALS as MLALS
    from als_mi355x.mllib.recommendation import ALS as MLlibALS
    u, i, r = _ratings()
    df = pd.DataFrame({"user": u, "item": i, "rating": r})
    est = MLALS(rank=6, maxIter=3, regParam=REG, seed=5).setSolver("nnls")
    model = est.fit(df)
    assert model.solver == "nnls"
    U = np.stack(model.userFactors["features"].to_numpy())
    V = np.stack(model.itemFactors["features"].to_numpy())
    assert (U >= 0).all() and (V >= 0).all() and U.shape == (300, 6)
    folded = model.foldInUsers(df)                     # None = the model's solver
    assert folded["id"].tolist() == list(range(300))
    assert rel_row_errs(np.stack(folded["features"].to_numpy()), U).max() <= 1e-5
    chol = np.stack(model.foldInUsers(df, nonnegative=False)["features"].to_numpy())
    assert (chol < 0).any()
    items = np.stack(model.foldInItems(df)["features"].to_numpy())
    assert (items >= 0).all() and items.shape == (200, 6)
    recs = model.recommendForNewUsers(df[df.user < 3], 5)
    assert recs["user"].tolist() == [0, 1, 2]
    assert all(s >= 0 for row in recs["recommendations"] for _, s in row)
    assert MLALS(rank=6, maxIter=1, regParam=REG, seed=5).fit(df).solver == "cholesky"
    with pytest.raises(NotImplementedError, match="setSolver"):
        MLALS(rank=6, nonnegative=True).fit(df)
    # mllib
    trip = list(zip(u.tolist(), i.tolist(), r.tolist()))
    m = MLlibALS.trainNonnegative(trip, 6, iterations=3, lambda_=REG, seed=5)
    Um = np.array([f for _, f in m.userFeatures()])
    np.testing.assert_array_equal(Um.astype(np.float32), U)   # the same engine call
    got = m.foldInUsers(trip, REG, nonnegative=True)
    assert [a for a, _ in got] == list(range(300))
    assert rel_row_errs(np.stack([x for _, x in got]), Um).max() <= 1e-5
    new = m.recommendProductsForNewUsers(trip[:40], 5, REG, nonnegative=True)
    assert all(x.rating >= 0 for _, lst in new for x in lst)
    mi = MLlibALS.trainNonnegative(trip, 4, iterations=2, lambda_=REG, seed=5, implicitPrefs=True,
                                   alpha=ALPHA)
    assert (np.array([f for _, f in mi.productFeatures()]) >= 0).all()
    with pytest.raises(NotImplementedError, match="trainNonnegative"):
        MLlibALS.train(trip, 6, nonnegative=True)
