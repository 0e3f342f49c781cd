"""GPU edge-shape parity tests for K1 (id map, CSR radix sort, scan, schedule), K2b
(als_yty) and K4 (als_predict / als_rmse_partial) against the CPU oracle.

The kernels change code path with the shape; every case here sits on such a change:

  * radix sort: ceil(bits / 8) passes (1-4, the ping-pong destination alternates with the
    count), 4096-key tiles, partial waves, all-equal / alternating / run keys (stability
    of the ballot ranking across waves, rounds and tiles);
  * scan: one, two and three levels (n <= 2048, <= 2048^2, above);
  * grid-stride loops past the grid caps (65,536 blocks; 1,024 for the schedule count);
  * schedule: degrees at chunk, chunk + 1, 2 chunk, 2 chunk + 1, empty rows, no / only
    heavy rows, chunks on the 1-pass / 2-pass boundary of its key sort;
  * K4: the second trip of the dot loop (rank > 64), its tail guards (k % 4 != 0), NaN in
    the padding columns [k, ld), ld > ld_for(k), pair counts around the 16-pair group and
    the 256-pair block, the strided final reduction (> 65,536 pairs), reproducibility;
  * K2b: 32-row / 64-row tasks (n <= / > 16384), 1-row tails, n < 32, n == 0, and a
    per-entry bar that sees a wrong small entry.

Bars: K1 bit-exact.  K4 predictions |got - ref| <= 2 k 2^-52 sum_d |a_d b_d| per pair
(the fp64 dot-product bound, products of fp32 values being exact in fp64, applied to both
sides); NaN positions and the RMSE count exact; SSE 1e-9 relative; the RMSE output
bit-identical from call to call.  K2b 1e-6 relative Frobenius, padding exactly zero, and
per entry |G_ij - ref_ij| <= 1e-6 sqrt(ref_ii ref_jj) (Cauchy-Schwarz over products good to
~2^-21 of their operands gives 4.8e-7; 1e-6 is the project's K2b figure).
"""
import numpy as np
import pytest
import torch

import als_mi355x.engine as E
from oracle import als_oracle as O
from helpers import report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _t(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV, dtype)


def _identity_index(n):
    """IdIndex of ids 0..n-1 all present (dense row = id), so n_rows is chosen freely."""
    ar = torch.arange(n, dtype=torch.int32, device=DEV)
    return E.IdIndex(ar, ar, n)


# ---------------------------------------------------------------- K1: CSR
N_COLS = 1000


def _csr_cols_vals(nnz, seed):
    assert nnz < (1 << 24)
    cols = np.random.default_rng(seed).integers(0, N_COLS, nnz).astype(np.int32)
    return cols, np.arange(nnz, dtype=np.float32)


def _radix_rows(n_rows, nnz):
    rng = np.random.default_rng(n_rows % 1000 + nnz)
    rows = rng.integers(0, n_rows, nnz).astype(np.int32)
    if nnz >= 2:  # the top row needs every key bit, the bottom one none
        rows[rng.integers(0, nnz)] = n_rows - 1
        rows[rng.integers(0, nnz)] = 0
    return rows


def _check_csr(rows, n_rows, seed):
    """als_csr_build of (rows, random cols, vals = position) vs O.csr_build, bit-exact.
    vals = arange(nnz) (exact in fp32 below 2^24) makes any mis-ordering visible."""
    nnz = len(rows)
    cols, vals = _csr_cols_vals(nnz, seed)
    blk = E.build_block(_t(rows, torch.int32), _identity_index(n_rows), _t(cols, torch.int32),
                        _identity_index(N_COLS), _t(vals, torch.float32), E.Workspace(DEV))
    ptr_, idx_, val_ = O.csr_build(rows, cols, vals, n_rows)
    np.testing.assert_array_equal(blk.row_ptr.cpu().numpy(), ptr_)
    np.testing.assert_array_equal(blk.col.cpu().numpy(), idx_)
    val = blk.val.cpu().numpy()
    np.testing.assert_array_equal(val, val_)
    return ptr_, val


@pytest.mark.parametrize("n_rows,nnz", [(1, 1), (1, 4097), (256, 4095), (256, 4096), (256, 4097),
                                        (257, 10000), (65536, 200000), (65537, 200000),
                                        ((1 << 24) + 1, 100000)])
def test_csr_radix_passes_and_tiles(n_rows, nnz):
    """bits = bit_length(n_rows - 1): 0 (one row), 8 (1 pass), 9 and 16 (2 passes), 17
    (3 passes), 25 (4 passes, most rows empty); nnz at the 4096-key tile boundaries and
    with a partial last wave."""
    _check_csr(_radix_rows(n_rows, nnz), n_rows, seed=nnz)


def _stability_rows(pattern, nnz, n_rows):
    if pattern == "one_row":  # every key equal: 4 waves x 16 rounds x 5 tiles rank one digit
        return np.full(nnz, 137, np.int32)
    if pattern == "alternating":
        return (np.arange(nnz) % 2).astype(np.int32)
    assert pattern == "runs"  # runs of 63, 64, 65 equal keys; each key comes back later
    lens = np.resize(np.array([63, 64, 65]), nnz // 63 + 1)
    keys = (np.arange(len(lens)) * 7) % 50
    return np.repeat(keys, lens)[:nnz].astype(np.int32)


@pytest.mark.parametrize("pattern", ["one_row", "alternating", "runs"])
def test_csr_sort_is_stable(pattern):
    n_rows, nnz = 300, 20000
    rows = _stability_rows(pattern, nnz, n_rows)
    ptr_, val = _check_csr(rows, n_rows, seed=3)
    # values are input positions: strictly ascending within every row
    asc = np.diff(val) > 0
    row_starts = ptr_[1:-1]
    asc[row_starts[(row_starts > 0) & (row_starts < nnz)] - 1] = True
    assert asc.all()


# ---------------------------------------------------------------- K1: id map / scan
@pytest.mark.parametrize("id_space,n", [(2048, 200000), (2049, 200000),
                                        (2048 * 2048 + 1, 200000), ((1 << 24) + 5000, 200000),
                                        ((1 << 24) + 5000, (1 << 24) + 4097)])
def test_index_build_scan_levels(id_space, n):
    """Scan of id_space flags: one level (2048), two (2049), three (2048^2 + 1 and above).
    id_space > 2^24 strides idx_finalize_kernel's grid, n > 2^24 ids idx_mark_kernel's.
    Ids -1 and id_space are ignored by the kernel."""
    rng = np.random.default_rng(id_space % 9973 + n % 101)
    ids = rng.integers(0, id_space, n).astype(np.int64)
    if id_space < 100000:  # leave holes: 200,000 draws would hit every id
        ids = ids[ids % 3 != 1]
    ids[0], ids[-1] = id_space - 1, 0
    ids[[7, len(ids) // 2, len(ids) - 9]] = -1
    ids[[11, len(ids) // 3]] = id_space
    ids = ids.astype(np.int32)
    idx = E.build_index(_t(ids, torch.int32), id_space, E.Workspace(DEV))
    valid = ids[(ids >= 0) & (ids < id_space)]
    assert len(valid) == len(ids) - 5
    mp, uniq = O.index_build(valid, id_space)
    assert idx.n == len(uniq)
    np.testing.assert_array_equal(idx.map.cpu().numpy(), mp)
    np.testing.assert_array_equal(idx.uniq.cpu().numpy(), uniq)


# ---------------------------------------------------------------- K1: schedule
def _edge_degrees(chunk):
    return sorted({x for x in (0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1,
                               3 * chunk - 1) if x >= 0})


def _mixed_row_ptr(n_rows, chunk, seed, nnz_cap=4e7):
    """row_ptr with every edge degree present in random row order.  Each degree gets an
    equal share of the rows, the long ones thinned so that nnz stays below ~5e7 (only
    row_ptr is read); rows left over are empty or hold one rating."""
    rng = np.random.default_rng(seed)
    degs = _edge_degrees(chunk)
    share = n_rows // len(degs)
    parts = [np.full(int(max(1, min(share, nnz_cap / len(degs) // max(d, 1)))), d) for d in degs]
    deg = np.concatenate(parts)
    deg = np.concatenate([deg, np.resize([0, 1], n_rows - len(deg))])
    deg = deg[rng.permutation(n_rows)].astype(np.int64)
    assert len(deg) == n_rows and set(deg.tolist()) == set(degs) and deg.sum() < 5e7
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)


def _check_schedule(rp, chunk):
    """als_schedule_count + als_schedule_build straight from a row_ptr vs O.schedule_build."""
    n_rows = len(rp) - 1
    dummy_c = torch.zeros(1, dtype=torch.int32, device=DEV)  # only row_ptr is read
    dummy_v = torch.zeros(1, dtype=torch.float32, device=DEV)
    blk = E.schedule_block(n_rows, int(rp[-1]), _t(rp, torch.int64), dummy_c, dummy_v,
                           E.Workspace(DEV), chunk)
    light, heavy, slot_begin, chunks = O.schedule_build(rp, chunk)
    assert (blk.n_light, blk.n_heavy, blk.n_chunks) == (len(light), len(heavy), len(chunks))
    np.testing.assert_array_equal(blk.light_rows[:len(light)].cpu().numpy(), light)
    np.testing.assert_array_equal(blk.heavy_rows[:len(heavy)].cpu().numpy(), heavy)
    np.testing.assert_array_equal(blk.heavy_slot_begin.cpu().numpy(), slot_begin)
    ch = np.array(chunks, dtype=np.int64).reshape(-1, 3)
    np.testing.assert_array_equal(blk.chunk_row[:len(ch)].cpu().numpy(), ch[:, 0])
    np.testing.assert_array_equal(blk.chunk_begin[:len(ch)].cpu().numpy(), ch[:, 1])
    np.testing.assert_array_equal(blk.chunk_end[:len(ch)].cpu().numpy(), ch[:, 2])
    return blk


@pytest.mark.parametrize("chunk", [1, 254, 255, 4096, 16384, 65535])
def test_schedule_edge_degrees(chunk):
    """Degrees 0, 1, chunk - 1, chunk, chunk + 1, 2 chunk, 2 chunk + 1, 3 chunk - 1 over 5,000
    rows.  The key sort uses bit_length(chunk + 1) bits: 1 pass up to chunk 254, 2 passes
    from 255 (and at the production chunks 4096 / 16384), 3 passes at 65535."""
    blk = _check_schedule(_mixed_row_ptr(5000, chunk, seed=chunk), chunk)
    assert blk.n_light > 0 and blk.n_heavy > 0


def test_schedule_all_light():
    rng = np.random.default_rng(1)
    deg = rng.integers(0, 4097, 5000)  # 0 .. chunk, many equal degrees (order by row id)
    deg[:3] = (4096, 0, 4096)
    blk = _check_schedule(np.concatenate([[0], np.cumsum(deg)]).astype(np.int64), 4096)
    assert blk.n_heavy == 0 and blk.n_chunks == 0


def test_schedule_all_heavy():
    rng = np.random.default_rng(2)
    deg = rng.integers(256, 3 * 255, 5000)  # chunk + 1 .. 3 chunk - 1
    deg[:3] = (256, 510, 511)
    blk = _check_schedule(np.concatenate([[0], np.cumsum(deg)]).astype(np.int64), 255)
    assert blk.n_light == 0


@pytest.mark.parametrize("deg", [0, 64, 65])
def test_schedule_single_row(deg):
    _check_schedule(np.array([0, deg], np.int64), 64)


def test_schedule_count_grid_stride():
    """300,000 rows: sched_count_kernel's 1,024 x 256 grid strides over them."""
    _check_schedule(_mixed_row_ptr(300000, 4096, seed=9), 4096)


# ---------------------------------------------------------------- K4
N_U, N_I = 200, 150


def _holey_map(n_rows, space, rng):
    """An id map of `space` ids, n_rows of them present (ascending), -1 elsewhere."""
    present = np.sort(rng.choice(space, n_rows, replace=False))
    mp = np.full(space, -1, np.int32)
    mp[present] = np.arange(n_rows, dtype=np.int32)
    return mp, present.astype(np.int32)


def _cancelling_signs(u):
    """Signs s with sum_d s_d u_d^2 near 0 (greedy: each term pulls the sum back)."""
    s = np.empty(len(u))
    run = 0.0
    for d in np.argsort(-np.abs(u)):
        s[d] = -1.0 if run > 0 else 1.0
        run += s[d] * float(u[d]) ** 2
    return s


class _Model:
    """Random 200 x k and 150 x k factor tables behind id maps with holes.  Item row j < 75
    is +-(user row j), signs arranged so that <U[j], V[j]> nearly cancels.  Columns
    [k, ld) of the device tables hold NaN: K4 must not read them into a result."""

    def __init__(self, k, ld, seed):
        rng = np.random.default_rng(seed)
        self.k, self.ld = k, ld
        self.U = rng.standard_normal((N_U, k)).astype(np.float32)
        self.V = rng.standard_normal((N_I, k)).astype(np.float32)
        self.n_cancel = N_I // 2
        for j in range(self.n_cancel):
            self.V[j] = (_cancelling_signs(self.U[j]) * self.U[j]).astype(np.float32)
        self.umap, self.uids = _holey_map(N_U, 260, rng)
        self.imap, self.iids = _holey_map(N_I, 190, rng)
        Ud = np.full((N_U, ld), np.nan, np.float32)
        Vd = np.full((N_I, ld), np.nan, np.float32)
        Ud[:, :k], Vd[:, :k] = self.U, self.V
        self.Ud, self.Vd = _t(Ud, torch.float32), _t(Vd, torch.float32)
        self.uidx = E.IdIndex(_t(self.umap, torch.int32), _t(self.uids, torch.int32), N_U)
        self.iidx = E.IdIndex(_t(self.imap, torch.int32), _t(self.iids, torch.int32), N_I)

    def pairs(self, n, seed):
        """n (user id, item id) pairs: even positions random ids (holes and out-of-range
        ids included), odd positions a cancelling pair."""
        rng = np.random.default_rng(seed)
        pu = rng.integers(-3, len(self.umap) + 3, n).astype(np.int32)
        pi = rng.integers(-3, len(self.imap) + 3, n).astype(np.int32)
        j = rng.integers(0, self.n_cancel, n)
        odd = np.arange(n) % 2 == 1
        pu[odd], pi[odd] = self.uids[j[odd]], self.iids[j[odd]]
        return pu, pi

    def predict(self, pu, pi):
        return E.predict_pairs(_t(pu, torch.int32), _t(pi, torch.int32), self.uidx, self.iidx,
                               self.Ud, self.Vd, self.k).cpu().numpy()

    def rmse(self, pu, pi, pr, ws):
        return E.rmse_pairs(_t(pu, torch.int32), _t(pi, torch.int32), _t(pr, torch.float32),
                            self.uidx, self.iidx, self.Ud, self.Vd, self.k, ws).cpu().numpy()

    def ref_predict(self, pu, pi):
        return O.predict(self.U, self.V, self.umap, self.imap, pu, pi)

    def dot_bound(self, pu, pi):
        """2 k 2^-52 sum_d |a_d b_d| per known pair (NaN elsewhere)."""
        def rows(mp, ids):
            ids = np.asarray(ids, np.int64)
            inside = (ids >= 0) & (ids < len(mp))
            return np.where(inside, mp[np.where(inside, ids, 0)], -1)
        ur, ir = rows(self.umap, pu), rows(self.imap, pi)
        known = (ur >= 0) & (ir >= 0)
        b = np.full(len(pu), np.nan)
        b[known] = 2.0 * self.k * 2.0 ** -52 * np.abs(
            self.U[ur[known]].astype(np.float64) * self.V[ir[known]].astype(np.float64)).sum(1)
        return b


@pytest.mark.parametrize("extra_ld", [0, 8])
@pytest.mark.parametrize("k", [1, 3, 4, 5, 63, 64, 65, 67, 68, 100, 127, 128])
def test_predict_rank_and_ld_grid(k, extra_ld):
    """Ranks around the float4 tail (k % 4) and the 64-column trip of the dot loop, with
    ld = ld_for(k) and ld_for(k) + 8, NaN in columns [k, ld).  Bar: the fp64 dot-product
    bound 2 k 2^-52 sum |a_d b_d| per pair (both sides sum exact fp64 products in their
    own order); half of the pairs nearly cancel, so the bar is absolute, not relative."""
    m = _Model(k, E.ld_for(k) + extra_ld, seed=k)
    pu, pi = m.pairs(3000, seed=k + 1)
    got, ref, bound = m.predict(pu, pi), m.ref_predict(pu, pi), m.dot_bound(pu, pi)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))  # a NaN read from the pad fails here
    ok = ~np.isnan(ref)
    assert ok.sum() > 1500
    if k >= 63:  # the cancelling pairs do cancel: |dot| far below sum |a_d b_d|
        odd = np.arange(len(pu)) % 2 == 1
        assert np.median(np.abs(ref[odd]) / (bound[odd] / (2.0 * k * 2.0 ** -52))) < 0.05
    err = np.abs(got[ok] - ref[ok])
    ratio = float(np.max(err / np.where(bound[ok] > 0, bound[ok], 1.0)))
    print(f"predict k={k} ld={m.ld}: max |got - ref| / bound = {ratio:.3g}")
    report(f"predict_bound_ratio[k={k},ld={m.ld}]", ratio)
    assert np.all(err <= bound[ok]), ratio


def _special_pairs(m):
    """Ten unknown pairs: each unknown kind of id (-1, INT32_MIN, INT32_MAX, id == map size,
    an id whose map entry is -1) on the user side beside a known item, then on the item
    side beside a known user."""
    bad_u = [-1, I32_MIN, I32_MAX, len(m.umap), int(np.nonzero(m.umap < 0)[0][3])]
    bad_i = [-1, I32_MIN, I32_MAX, len(m.imap), int(np.nonzero(m.imap < 0)[0][3])]
    su = bad_u + [int(m.uids[5])] * 5
    si = [int(m.iids[5])] * 5 + bad_i
    return np.array(su, np.int32), np.array(si, np.int32)


@pytest.fixture(scope="module")
def edge_model():
    k = 67  # second trip of the dot loop with a 3-column tail
    return _Model(k, E.ld_for(k), seed=77)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 70001])
def test_predict_rmse_pair_count_edges(edge_model, n):
    """Pair counts around the 16-pair group and the 256-pair block, and 70,001 pairs (274
    partial blocks: sum_partials_kernel's strided loop).  The last pairs — the ragged end
    of the last group — are the unknown kinds (-1, INT32_MIN, INT32_MAX, id == map size,
    map entry -1) as far as n has room beside one known pair."""
    m = edge_model
    pu, pi = m.pairs(n, seed=n)
    pu[0], pi[0] = m.uids[0], m.iids[N_I - 1]  # a known, non-cancelling pair
    su, si = _special_pairs(m)
    ns = min(len(su), n - 1)
    if ns:
        pu[n - ns:], pi[n - ns:] = su[:ns], si[:ns]
    pr = np.random.default_rng(n).uniform(0.5, 5, n).astype(np.float32)
    got, ref, bound = m.predict(pu, pi), m.ref_predict(pu, pi), m.dot_bound(pu, pi)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    assert np.isnan(ref[n - ns:]).all() and not np.isnan(ref[0])
    ok = ~np.isnan(ref)
    assert np.all(np.abs(got[ok] - ref[ok]) <= bound[ok])
    out = m.rmse(pu, pi, pr, E.Workspace(DEV))
    sse_ref, n_ref = O.rmse(m.U, m.V, m.umap, m.imap, pu, pi, pr)
    assert n_ref == ok.sum() and out[1] == n_ref
    rel = abs(out[0] - sse_ref) / sse_ref
    print(f"rmse n={n}: count {n_ref}, SSE rel err {rel:.3g}")
    assert rel <= 1e-9


@pytest.mark.parametrize("n", [1, 10, 17, 257])
def test_rmse_no_known_pair(edge_model, n):
    """Only unknown ids (every kind, cycled): NaN predictions, SSE 0 and count 0."""
    m = edge_model
    su, si = _special_pairs(m)
    pu, pi = np.resize(su, n), np.resize(si, n)
    got = m.predict(pu, pi)
    assert np.isnan(got).all() and np.isnan(m.ref_predict(pu, pi)).all()
    out = m.rmse(pu, pi, np.full(n, 3.0, np.float32), E.Workspace(DEV))
    assert out[0] == 0.0 and out[1] == 0.0


def test_rmse_bitwise_reproducible(edge_model):
    """als_rmse_partial's partials are summed in a fixed order: three calls over 70,001
    pairs, the workspace filled with garbage between them, give the same 16 bytes."""
    m = edge_model
    n = 70001
    pu, pi = m.pairs(n, seed=5)
    pr = np.random.default_rng(6).uniform(0.5, 5, n).astype(np.float32)
    ws = E.Workspace(DEV)
    outs = []
    for _ in range(3):
        outs.append(m.rmse(pu, pi, pr, ws).tobytes())
        ws.buf.fill_(0xFF)
    assert outs[0] == outs[1] == outs[2]
    sse, cnt = np.frombuffer(outs[0], np.float64)
    assert cnt > n // 2 and sse > 0


# ---------------------------------------------------------------- K2b
def _yty_full(Y, rank):
    """als_yty of the fp32 rows Y (padding columns zero) as a full k_pad x k_pad matrix."""
    n = Y.shape[0]
    Yd = torch.zeros((max(n, 1), E.ld_for(rank)), dtype=torch.float32, device=DEV)
    if n:
        Yd[:n, :rank] = torch.as_tensor(Y).to(DEV)
    G = E.compute_yty(Yd, n, rank, E.Workspace(DEV)).cpu().numpy()
    kp = E.k_pad(rank)
    full = np.zeros((kp, kp))
    ii, jj = np.tril_indices(kp)
    full[ii, jj] = G
    return full + np.tril(full, -1).T


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 16384, 16385])
@pytest.mark.parametrize("rank", [3, 16, 17, 32, 33, 64, 65, 128])
def test_yty_row_count_edges(rank, n):
    """One and two ranks per tile class (k_pad 16 / 32 / 64 / 128) incl. non-multiples of
    16; n below one 32-row task, at 1-row tails, at the 512-task edge (16384: 512 tasks of
    32 rows; 16385: 64-row tasks, the last of 1 row) and n == 0 (all zeros)."""
    Y = np.random.default_rng(1000 * rank + n).standard_normal((n, rank)).astype(np.float32)
    full = _yty_full(Y, rank)
    assert np.all(full[rank:, :] == 0)  # rows and (by symmetry) columns [k, k_pad)
    if n == 0:
        assert np.all(full == 0)
        return
    ref = O.yty(Y)
    assert np.linalg.norm(full[:rank, :rank] - ref) / np.linalg.norm(ref) <= 1e-6


@pytest.mark.parametrize("scaling", ["columns", 1e-4, 1e4])
@pytest.mark.parametrize("rank", [3, 17, 33, 64, 65, 128])
def test_yty_per_entry_accuracy(rank, scaling):
    """Every entry against its own operands: |G_ij - ref_ij| <= 1e-6 sqrt(ref_ii ref_jj),
    with columns scaled by 1, 2^-4, 2^-8 (a Frobenius norm would hide the small
    columns' entries) and with all of Y at 1e-4 and at 1e4."""
    rng = np.random.default_rng(rank)
    Y = rng.standard_normal((4000, rank))
    if scaling == "columns":
        Y = Y * (2.0 ** -(4 * rng.integers(0, 3, rank)))[None, :]
    else:
        Y = Y * scaling
    Y = Y.astype(np.float32)
    full = _yty_full(Y, rank)
    ref = O.yty(Y)
    d = np.sqrt(np.diag(ref))
    ratio = float((np.abs(full[:rank, :rank] - ref) / np.outer(d, d)).max())
    print(f"yty rank={rank} scaling={scaling}: max |G_ij - ref_ij| / sqrt(ref_ii ref_jj) = {ratio:.3g}")
    report(f"yty_per_entry[rank={rank},scaling={scaling}]", ratio)
    assert np.all(full[rank:, :] == 0)
    assert ratio <= 1e-6
