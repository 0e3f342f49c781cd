"""Buffer contracts of libals_hip.so on the GPU: no entry point writes or reads outside the
memory include/als_hip.h says it may, whatever that memory held before the call.

Every case runs its entry point on views carved from a guard-band arena (guard_arena.py):
workspaces of exactly *_workspace_bytes() bytes, at a 256-byte boundary and 16 bytes past
one (the alignment the header promises to accept), and, in the second tier, every output and
input table of exactly its stated size.  It runs twice, on an arena filled with 0x00 and on
one filled with 0xFF (NaN as f32 / f64, -1 as int32 / int64); workspaces and outputs still
hold the fill when the call starts.  Asserted:

  1. every guard byte of every carve, inputs included, still holds the fill;
  2. every output is bitwise identical between the two fills: an over-read that reaches a
     result, a dependence on stale scratch and an output word nobody writes all show here;
  3. the result equals, bitwise, the ordinary call on the same inputs (a roomy
     engine.Workspace, torch allocations, tables of the usual leading dimension) wherever the
     header promises reproducible bits.  als_solve_half, whose workspace layout follows
     ws_bytes, is held to the project's parity bar instead: 1e-4 relative per row against the
     fp64 oracle.

Tier A: every entry point with a workspace, through the engine wrappers and a
GuardedWorkspace (als_topk, als_topk_filtered, als_similar and als_nnls_rows through ctypes:
their wrappers allocate the workspace themselves).  Tier B: direct ctypes calls with every
pointer argument carved; factor tables 16 bytes past a boundary with ld = ld_for(k) + 4, so
the padding columns hold the fill.  Inputs are the generators of the kernels' own test
modules.  Nothing here passes a wrong size: the guards only observe.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import fullrank_ref as FR
import guard_arena as G
import test_gpu_diversify as TD
import test_gpu_edges_k1_k2b_k4 as TK1
import test_gpu_edges_k2_k3 as TK2
import test_gpu_explain as TX
import test_gpu_fold_in as TF
import test_gpu_kernels as TKN
import test_gpu_nnls as TN
import test_gpu_objective as TO
import test_gpu_rank_metrics as TM
import test_gpu_regression_metrics as TR
import test_gpu_similar as TS
import test_gpu_topk_filtered as TT
from als_mi355x import _lib
from als_mi355x import engine as E
from als_mi355x import filters
from helpers import unit_source_factors
from oracle import als_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
RANKS = (1, 17, 33, 64, 65, 128)     # k_pad 16, 32, 64, 128; 65: the first W1 rank
ALIGN = pytest.mark.parametrize("offset16", [False, True], ids=["a256", "a16"])
I32, I64, F32, F64 = torch.int32, torch.int64, torch.float32, torch.float64

# *_workspace_bytes() -> the tests below that run its entry point on an exact-size carve
# (test_guard_arena_cpu.py fails when the ABI gains a size function without an entry here)
WORKSPACE_CASES = {
    "als_index_workspace_bytes": ["test_index_build"],
    "als_csr_workspace_bytes": ["test_csr_and_schedule_build", "test_csr_build_all_guarded"],
    "als_schedule_workspace_bytes": ["test_csr_and_schedule_build"],
    "als_yty_workspace_bytes": ["test_yty"],
    "als_solve_workspace_bytes": ["test_solve_half", "test_solve_half_two_calls",
                                  "test_solve_half_two_segments", "test_solve_half_all_guarded"],
    "als_rmse_workspace_bytes": ["test_rmse_and_regression_moments"],
    "als_regression_moments_workspace_bytes": ["test_rmse_and_regression_moments"],
    "als_topk_workspace_bytes": ["test_topk", "test_topk_all_guarded"],
    "als_rank_metrics_workspace_bytes": ["test_rank_metrics"],
    "als_full_rank_workspace_bytes": ["test_rank_positions_and_full_rank_metrics"],
    "als_objective_workspace_bytes": ["test_objective_side_and_gram_dot"],
    "als_similar_workspace_bytes": ["test_similar"],
    "als_nnls_workspace_bytes": ["test_nnls_rows"],
    # these two return 0 (no workspace): the tests assert that and pass ws = NULL
    "als_fold_in_workspace_bytes": ["test_fold_in_all_guarded"],
    "als_explain_workspace_bytes": ["test_explain_all_guarded"],
}


# ------------------------------------------------------------------ the harness
class Mem:
    """Where a case's device memory comes from: a guard arena, or (arena None) torch's
    allocator and a roomy engine.Workspace, the ordinary call."""

    def __init__(self, arena=None, offset16=False):
        self.arena = arena
        self.offset16 = offset16
        self.ws = (G.GuardedWorkspace(arena, offset16) if arena is not None
                   else E.Workspace(torch.device(DEV)))

    @property
    def guarded(self):
        return self.arena is not None

    def inp(self, x, dtype, offset16=False):
        """An input array (host or device), exactly its own size."""
        x = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x)
        if self.guarded:
            return self.arena.put(x.to(dtype), offset16=offset16)
        return x.to(DEV, dtype).contiguous()

    def out(self, shape, dtype, offset16=False, prefill=None):
        """An output array still holding the arena's fill (torch.empty otherwise); prefill: a
        value that is neither fill pattern nor a possible result."""
        t = (self.arena.out(shape, dtype, offset16) if self.guarded
             else torch.empty(shape, dtype=dtype, device=DEV))
        if prefill is not None:
            t.fill_(prefill)
        return t

    def table(self, M, k, pad=None):
        """Factor rows M [n, >= k] as the library takes them.  Guarded: 16 bytes past a
        256-byte boundary, ld = ld_for(k) + 4, columns [k, ld) holding the arena's fill (pad
        None) or `pad` (the entry points that want zeros there).  Ordinary: ld_for(k), zeros."""
        M = torch.as_tensor(np.array(M) if isinstance(M, np.ndarray) else M)[:, :k].to(DEV, F32)
        if self.guarded:
            t = self.arena.out((M.shape[0], E.ld_for(k) + 4), F32, offset16=True)
            if pad is not None:
                t.fill_(pad)
        else:
            t = torch.zeros((M.shape[0], E.ld_for(k)), dtype=F32, device=DEV)
        t[:, :k] = M
        return t

    def scratch(self, nbytes):
        """A workspace of exactly nbytes for a ctypes call (None for 0): no 256-byte floor."""
        nbytes = int(nbytes)
        if nbytes == 0:
            return None
        if self.guarded:
            return self.arena.carve(nbytes, torch.uint8, None, self.offset16, name="workspace")
        return torch.empty(nbytes + 4096, dtype=torch.uint8, device=DEV)[:nbytes]


def _call(name, *args):
    """One ctypes call of the library: tensors as device pointers, None as NULL, the current
    stream appended (the marshalling of the kernels/*.py bindings)."""
    conv = [(0 if a is None else a.data_ptr()) if (a is None or isinstance(a, torch.Tensor))
            else a for a in args]
    _lib.check(getattr(_lib.lib(), name)(*conv, _lib.stream_ptr(DEV)), name)


def _snap(out):
    return {k: torch.as_tensor(v).detach().clone().contiguous() for k, v in out.items()
            if v is not None}


def _bits(t):
    return t.reshape(-1).view(torch.uint8)


def _assert_same_bits(a, b, what, pads=True):
    """pads=False leaves the '*_pad' outputs (columns [k, ld) of an output table) out: their
    width differs between the guarded and the ordinary call."""
    use = lambda d: sorted(k for k in d if pads or not k.endswith("_pad"))
    keys = use(a)
    assert keys == use(b), (what, sorted(a), sorted(b))
    for key in keys:
        x, y = a[key], b[key]
        assert x.shape == y.shape and x.dtype == y.dtype, (what, key, x.shape, y.shape)
        if not torch.equal(_bits(x), _bits(y)):
            n = x.element_size()
            diff = (_bits(x) != _bits(y)).view(-1, n).any(1) if x.numel() else _bits(x)
            where = diff.nonzero().flatten()[:8].tolist()
            raise AssertionError(f"{what}: output '{key}' differs at flat positions {where} "
                                 f"(of {x.numel()}): {x.reshape(-1)[where].tolist()} vs "
                                 f"{y.reshape(-1)[where].tolist()}")


def _bounds(run, offset16=False, plain=True, capacity=64 << 20):
    """run(mem) -> {name: output tensor} on a 0x00 arena, a 0xFF arena and (plain) ordinary
    memory; the three assertions of the module docstring.  Returns the guarded outputs."""
    outs = []
    for fill in (0x00, 0xFF):
        arena = G.Arena(DEV, fill, capacity)
        out = run(Mem(arena, offset16))
        torch.cuda.synchronize()
        assert arena.carves, "the case used no guarded memory"
        bad = arena.check()
        assert not bad, (f"fill {fill:#04x}: bytes outside a buffer were written, offsets "
                         f"relative to the payload: "
                         f"{ {k: (v[:8], len(v)) for k, v in bad.items()} }; sizes "
                         f"{ {c['name']: c['end'] - c['start'] for c in arena.carves} }")
        outs.append(_snap(out))
        for key, v in outs[-1].items():   # on the 0xFF arena an unwritten column reads as NaN
            if key.endswith("_pad"):
                assert v.numel() > 0 and bool((v == 0).all()), \
                    f"fill {fill:#04x}: '{key}': columns [k, ld) must be written as zero"
    _assert_same_bits(outs[0], outs[1], "arena filled with 0x00 vs 0xFF")
    if plain:
        ref = _snap(run(Mem(None)))
        torch.cuda.synchronize()
        _assert_same_bits(outs[0], ref, "guarded vs ordinary call", pads=False)
    return outs[0]


# ================================================================== Tier A
# ------------------------------------------------------------------ K1
@ALIGN
@pytest.mark.parametrize("n,id_space", [(1, 1), (300, 2048), (5000, 2049), (4096, 300),
                                        (4097, 4097)])
def test_index_build(n, id_space, offset16):
    """Scan of id_space flags at one tile (2048) and one tile + 1."""
    ids = np.random.default_rng(n + id_space).integers(0, id_space, n).astype(np.int32)

    def run(mem):
        idx = E.build_index(torch.as_tensor(ids).to(DEV), id_space, mem.ws)
        return dict(map=idx.map, uniq=idx.uniq, n=idx.n)
    got = _bounds(run, offset16)
    mp, uniq = O.index_build(ids, id_space)
    np.testing.assert_array_equal(got["map"].cpu().numpy(), mp)
    np.testing.assert_array_equal(got["uniq"].cpu().numpy(), uniq)


def _csr_inputs(n_rows, nnz):
    """test_csr_radix_passes_and_tiles' rows, columns and position values."""
    return (TK1._radix_rows(n_rows, nnz),) + TK1._csr_cols_vals(nnz, seed=nnz)


def _block_outputs(b):
    return dict(row_ptr=b.row_ptr, col=b.col, val=b.val, light=b.light_rows[:b.n_light],
                heavy=b.heavy_rows[:b.n_heavy], slot_begin=b.heavy_slot_begin,
                chunk_row=b.chunk_row[:b.n_chunks], chunk_begin=b.chunk_begin[:b.n_chunks],
                chunk_end=b.chunk_end[:b.n_chunks],
                counts=torch.tensor([b.n_light, b.n_heavy, b.n_chunks]))


CSR_SHAPES = [(1, 1), (256, 4096), (257, 4097), (2047, 3000), (2048, 3000), (4096, 5000),
              (4097, 5000)]   # radix tile 4096 keys, scan tile 2048 (of n_rows + 1 entries)


@ALIGN
@pytest.mark.parametrize("n_rows,nnz", CSR_SHAPES)
def test_csr_and_schedule_build(n_rows, nnz, offset16):
    """als_csr_build then als_schedule_build (chunk 4: light and heavy rows), each on its
    own exact workspace."""
    rows, cols, vals = _csr_inputs(n_rows, nnz)
    t = lambda a: torch.as_tensor(a).to(DEV)

    def run(mem):
        b = E.build_block(t(rows), TK1._identity_index(n_rows), t(cols),
                          TK1._identity_index(TK1.N_COLS), t(vals), mem.ws, chunk=4)
        assert not mem.guarded or len(mem.arena.carves) == 2
        return _block_outputs(b)
    got = _bounds(run, offset16)
    ptr_, idx_, val_ = O.csr_build(rows, cols, vals, n_rows)
    np.testing.assert_array_equal(got["row_ptr"].cpu().numpy(), ptr_)
    np.testing.assert_array_equal(got["col"].cpu().numpy(), idx_)
    np.testing.assert_array_equal(got["val"].cpu().numpy(), val_)


# ------------------------------------------------------------------ K2b
@ALIGN
@pytest.mark.parametrize("rank", RANKS)
def test_yty(rank, offset16):
    """n = 1, 33, 333 (32-row tasks) and, at two ranks, 16447 (64-row tasks)."""
    for n in (1, 33, 333) + ((16447,) if rank in (17, 128) else ()):
        Y = unit_source_factors(n, rank, seed=rank + n)

        def run(mem):
            return dict(yty=E.compute_yty(Mem(None).table(Y, rank), n, rank, mem.ws))
        _bounds(run, offset16)


# ------------------------------------------------------------------ K2/K3
SOLVE_CHUNK = 64
SOLVE_ALPHA = 4.0
SOLVE_REG = 0.1


@functools.lru_cache(maxsize=None)
def _solve_core():
    """test_split_window_row_norm_spread's ratings: 900 users (not a multiple of 64), 420
    items among which light rows, dual-path short rows, heavy items of 400-500 ratings
    (7-8 tasks at chunk 64) and, with the last 400 users' factors shrunk, rescued rows."""
    u, i, r = TKN._norm_spread_ratings()
    return E.ALSCore(u, i, r, device=DEV, chunk=SOLVE_CHUNK)


@functools.lru_cache(maxsize=None)
def _solve_case(rank, implicit):
    """(item block, source factors, yty, fp64 oracle rows) of one item half-sweep."""
    core = _solve_core()
    core.init_factors(rank, seed=3)
    U = core.U.clone()
    ib = core.item_block
    if implicit:
        ib = dataclasses.replace(ib, val=(ib.val - 2.5).contiguous())
    else:
        U[500:] /= 1e9          # the split-window rows: solved by the RESCUE launch
    assert U.shape[0] == 900 and ib.n_rows == 420
    assert ib.n_light > 0 and ib.n_heavy >= 2 and ib.n_chunks >= 5
    if not implicit and rank > 32:
        assert ib.n_dual(rank) > 0
    yty = E.compute_yty(U, 900, rank, E.Workspace(torch.device(DEV))) if implicit else None
    if not implicit:        # the case does reach the RESCUE launch
        ws, st = E.Workspace(torch.device(DEV)), torch.zeros(1, dtype=I32, device=DEV)
        a = (ib, U, torch.empty_like(core.V), rank, SOLVE_REG, False, SOLVE_ALPHA, None, st, ws)
        E.solve_half(*a, E.PHASE_ALL & ~E.PHASE_RESCUE)
        torch.cuda.synchronize()
        assert int(ws.buf[8:12].view(I32).item()) > 0
        E.solve_half(*a, E.PHASE_RESCUE)
    ref = O.half_sweep(ib.row_ptr.cpu().numpy(), ib.col.cpu().numpy(), ib.val.cpu().numpy(),
                       U[:, :rank].cpu().numpy(), SOLVE_REG, implicit, SOLVE_ALPHA)
    return ib, U, yty, ref


def _assert_solve_parity(got, ref, rank):
    assert int(got["status"].item()) == 0
    e = TKN._exact_rel_errs(got["X"].cpu().numpy(), ref)
    print(f"solve_half rank {rank}: max rel row err {e.max():.3e}")
    assert e.max() <= 1e-4, (float(e.max()), int(e.argmax()))


def _solve_outputs(X, rank, status):
    return dict(X=X[:, :rank], X_pad=X[:, rank:] if X.shape[1] > rank else None, status=status)


@ALIGN
@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("rank", RANKS)
def test_solve_half(rank, implicit, offset16):
    """PHASE_ALL on exactly als_solve_workspace_bytes(): slots, rescue list and split table
    at their closest, the table at (ws_bytes - table) & ~255 from a base that is only
    16-byte aligned, nothing in the scale words but the fill."""
    ib, U, yty, ref = _solve_case(rank, implicit)

    def run(mem):
        X = torch.full((ib.n_rows, U.shape[1]), 7.0, device=DEV)
        status = torch.zeros(1, dtype=I32, device=DEV)
        E.solve_half(ib, U, X, rank, SOLVE_REG, implicit, SOLVE_ALPHA, yty, status, mem.ws)
        return _solve_outputs(X, rank, status)
    _assert_solve_parity(_bounds(run, offset16, plain=False), ref, rank)


@ALIGN
@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("rank", (17, 64, 128))
def test_solve_half_two_calls(rank, implicit, offset16):
    """PREP | RSCALE | LAUNCH1, then DUAL | LAUNCH2 | RESCUE, on one carve; at rank 17 the
    explicit case has rows waiting in the rescue list between the calls."""
    ib, U, yty, ref = _solve_case(rank, implicit)
    first = E.PHASE_PREP | E.PHASE_RSCALE | E.PHASE_LAUNCH1
    waiting = []

    def run(mem):
        X = torch.full((ib.n_rows, U.shape[1]), 7.0, device=DEV)
        status = torch.zeros(1, dtype=I32, device=DEV)
        a = (ib, U, X, rank, SOLVE_REG, implicit, SOLVE_ALPHA, yty, status, mem.ws)
        E.solve_half(*a, first)
        mem.ws.hold = True
        torch.cuda.synchronize()
        waiting.append(int(mem.ws.buf[8:12].view(I32).item()))
        E.solve_half(*a, E.PHASE_ALL & ~first)
        assert not mem.guarded or len(mem.arena.carves) == 1
        return dict(_solve_outputs(X, rank, status), rescue_left=mem.ws.buf[8:12].view(I32))
    got = _bounds(run, offset16, plain=False)
    assert int(got["rescue_left"].item()) == 0
    # without a dual path (rank <= 32) the shrunk rows are flagged by LAUNCH1 already
    assert len(set(waiting)) == 1 and (implicit or rank > 32 or waiting[0] > 0), waiting
    _assert_solve_parity(got, ref, rank)


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("rank,offset16", [(17, False), (64, True), (128, False), (65, True)])
def test_solve_half_two_segments(rank, implicit, offset16):
    """test_two_segment_edges' rows (130 ratings, 0 .. 130 of them early, chunk 64) as a
    two-segment schedule whose slots start at slot_base = 3, early then late call on one
    carve sized for all slots."""
    n_src, cut, n, chunk, alpha = 512, 256, 130, 64, 2.0
    early, dst, src, r = TK2._two_segment_ratings(rank, implicit, n_src, cut, n)
    core = E.ALSCore(dst, src, r, device=DEV, chunk=chunk)
    core.init_factors(rank, seed=7)
    core.V[:, :rank] = torch.as_tensor(unit_source_factors(n_src, rank, seed=5000 + rank)).to(DEV)
    ub = core.user_block
    rp = ub.row_ptr.cpu().numpy()
    seg = torch.as_tensor(rp[:-1] + np.array(early + [cut])).to(DEV)
    sched = E.split_schedule(ub, seg, cut, chunk=chunk, slot_base=3)
    assert sched.slot_base == 3 and sched.n_slots == 3 + sched.early[3] + sched.late[3]
    yty = E.compute_yty(core.V, n_src, rank, core.ws_yty) if implicit else None
    V_early = core.V.clone()
    V_early[cut:] = float("nan")        # the source rows that have not arrived yet
    ref = O.half_sweep(rp, ub.col.cpu().numpy(), ub.val.cpu().numpy(),
                       core.V[:, :rank].cpu().numpy(), SOLVE_REG, implicit, alpha)

    def run(mem):
        X = torch.full_like(core.U, 7.0)
        status = torch.zeros(1, dtype=I32, device=DEV)
        E.solve_half_split(ub, sched, "early", V_early, X, rank, SOLVE_REG, implicit, alpha, yty,
                           status, mem.ws)
        mem.ws.hold = True
        E.solve_half_split(ub, sched, "late", core.V, X, rank, SOLVE_REG, implicit, alpha, yty,
                           status, mem.ws)
        assert not mem.guarded or len(mem.arena.carves) == 1
        return _solve_outputs(X, rank, status)
    _assert_solve_parity(_bounds(run, offset16, plain=False), ref, rank)


# ------------------------------------------------------------------ K4 / K8
@ALIGN
@pytest.mark.parametrize("rank", RANKS)
def test_rmse_and_regression_moments(rank, offset16):
    """als_rmse_partial, als_regression_moments and als_regression_moments_cols at 1, 16, 257
    pairs (one block + 1) and, at one rank, 65,537 (the strided final reduction)."""
    core = TR._core(rank)
    t = lambda a, d: torch.as_tensor(a).to(DEV, d).contiguous()
    for n in (1, 16, 257) + ((65537,) if rank == 17 else ()):
        u, i, r = TR._pairs(n, seed=n)
        u[n // 2] = 10 ** 6      # an unknown id: dropped by the join
        p = core.predict(u, i).nan_to_num(0.0)

        def run(mem):
            a = (t(u, I32), t(i, I32), t(r, F32), core.uidx, core.iidx, core.U, core.V, rank)
            return dict(rmse=E.rmse_pairs(*a, mem.ws), moments=E.regression_moments_pairs(*a, mem.ws),
                        cols=E.regression_moments_cols(t(r, F64), p, mem.ws))
        _bounds(run, offset16)


# ------------------------------------------------------------------ K5
TOPS = (10, 16, 17, 32, 33, 100, 128, 200)
TOPK_SHAPES = ((1, 5), (17, 257), (129, 2049), (257, 5))    # (n_q, n_v)


@functools.lru_cache(maxsize=None)
def _topk_case(rank, n_q, n_v):
    """test_gpu_topk_filtered's grid (factors with an exact tie, seven kinds of exclusion
    list, the 'half' allow mask) at the sizes asked for."""
    Q, V, _, lists, allows = TT._grid_case(rank, n_q, n_v)
    beg, end, col = FR.ranges([np.sort(np.asarray(x, np.int64)) for x in lists])
    return Q, V, beg, end, col, np.nonzero(allows["half"])[0]


def _topk(mem, rank, top, n_q, n_v, filtered, tables_guarded):
    Q, V, beg, end, col, allow = _topk_case(rank, n_q, n_v)
    tab = mem if tables_guarded else Mem(None)
    Qd, Vd = tab.table(Q, rank), tab.table(V, rank)
    idx = tab.out((n_q, top), I32, prefill=-77)
    sc = tab.out((n_q, top), F32)
    w = mem.scratch(_lib.lib().als_topk_workspace_bytes(n_q, n_v, rank, top))
    if filtered:
        bits = filters.pack_allow_bits(torch.as_tensor(allow).to(DEV), n_v)
        _call("als_topk_filtered", Qd, n_q, Vd, n_v, Qd.shape[1], rank, top,
              tab.inp(beg, I64), tab.inp(end, I64), tab.inp(col, I32), tab.inp(bits, I32),
              idx, sc, w, w.numel())
    else:
        _call("als_topk", Qd, n_q, Vd, n_v, Qd.shape[1], rank, top, idx, sc, w, w.numel())
    return dict(idx=idx, score=sc)


@pytest.mark.parametrize("top", TOPS)
@pytest.mark.parametrize("rank", RANKS)
def test_topk(rank, top):
    """als_topk and als_topk_filtered on exactly als_topk_workspace_bytes(): every topr class
    of the key logs (32, 64, 100, 128), no log (top <= 16 and top > 128, the LDS lists), one
    query row, 17, one 128-row block + 1 and one 256-row block + 1, n_v of 5 (< top), 257 and
    2049, every combination at both workspace alignments."""
    ri = RANKS.index(rank)
    for j, (n_q, _) in enumerate(TOPK_SHAPES):
        n_v = TOPK_SHAPES[(j + ri) % len(TOPK_SHAPES)][1]
        for filtered in (False, True):
            for offset16 in (False, True):
                got = _bounds(lambda mem: _topk(mem, rank, top, n_q, n_v, filtered, False),
                              offset16, capacity=16 << 20)
                listed = (got["idx"] >= 0).sum(1)
                assert int(listed.max()) <= min(top, n_v)
                if not filtered:
                    assert bool((listed == min(top, n_v)).all())


# ------------------------------------------------------------------ K6
@ALIGN
@pytest.mark.parametrize("at", (10, 256))
def test_rank_metrics(at, offset16):
    lists, begin, end, col, _, _ = TM.pattern(at)
    t = lambda a, d: torch.as_tensor(a).to(DEV, d).contiguous()
    for n_q in (1, 257, 1030):
        def run(mem):
            sums, rows = E.rank_metrics_rows(t(lists[:n_q], I32), at, t(begin[:n_q], I64),
                                             t(end[:n_q], I64), t(col, I32), mem.ws, per_row=True)
            return dict(sums=sums, rows=rows)
        _bounds(run, offset16)


# ------------------------------------------------------------------ K9 (Tier A and B)
@ALIGN
@pytest.mark.parametrize("rank,n_v,n_q", [(1, 17, 1), (17, 257, 33), (33, 65, 67), (64, 1031, 5),
                                          (65, 64, 17), (128, 257, 65)])
def test_rank_positions_and_full_rank_metrics(rank, n_v, n_q, offset16):
    """als_rank_positions through ctypes with Q, V, the ranges, the filter and all three
    output arrays carved; als_full_rank_metrics on its exact workspace over those counts."""
    rng = np.random.default_rng(rank + n_v)
    Q, V = FR.integer_factors(rng, n_q, rank), FR.integer_factors(rng, n_v, rank)
    rel = FR.random_relevant(rng, n_q, n_v, rng.integers(0, 9, n_q))
    ex = FR.random_exclusions(rng, n_q, n_v, rel)
    allow = np.nonzero(rng.random(n_v) < 0.8)[0]
    rb, re_, rc = FR.ranges(rel)
    eb, ee, ec = FR.ranges(ex)
    n_ent = sum(len(x) for x in rel)
    wts = rng.random(max(n_ent, 1)).astype(np.float32)
    assert _lib.lib().als_rank_positions_table() > 0

    def run(mem):
        bits = filters.pack_allow_bits(torch.as_tensor(allow).to(DEV), n_v)
        Qd, Vd = mem.table(Q, rank), mem.table(V, rank)
        rbd, red = mem.inp(rb, I64), mem.inp(re_, I64)
        above = mem.out((max(len(rc), 1),), I32, prefill=-77)   # rc has >= 1 entry
        tied = mem.out((max(len(rc), 1),), I32, prefill=-77)
        n_adm = mem.out((n_q,), I32, prefill=-77)
        _call("als_rank_positions", Qd, n_q, Vd, n_v, Qd.shape[1], rank, rbd, red,
              mem.inp(rc, I32), mem.inp(eb, I64), mem.inp(ee, I64), mem.inp(ec, I32),
              mem.inp(bits, I32), above, tied, n_adm, None, 0)
        sums, rows = E.full_rank_sums_rows(above, tied, n_adm, rbd, red, mem.ws,
                                           mem.inp(wts, F32), per_row=True)
        return dict(above=above[:n_ent], tied=tied[:n_ent], n_adm=n_adm, sums=sums, rows=rows)
    got = _bounds(run, offset16)
    ref = FR.counts(Q, V, rel, ex=ex, allow=allow)
    np.testing.assert_array_equal(got["above"].cpu().numpy(), ref["above"])
    np.testing.assert_array_equal(got["n_adm"].cpu().numpy(), ref["n_adm"])


# ------------------------------------------------------------------ K10
@ALIGN
@pytest.mark.parametrize("rank", RANKS)
def test_objective_side_and_gram_dot(rank, offset16):
    core = TO.small_core()
    TO._set_factors(core, rank, seed=rank)
    U, V = core.U.clone(), core.V.clone()

    def run(mem):
        out = {}
        for implicit, alpha in TO.MODES:
            out[f"side{implicit}{alpha}"] = E.objective_side(
                core.user_block, U, V, core.n_items, rank, implicit, alpha, mem.ws).clone()
        out["reg_only"] = E.objective_side(core.item_block, V, None, core.n_users, rank, True, 40.0,
                                           mem.ws)
        dot, ga, gb = E.gram_dot(U, core.n_users, V, core.n_items, rank, mem.ws, grams=True)
        return dict(out, dot=dot, gram_a=ga, gram_b=gb)
    _bounds(run, offset16)


# ------------------------------------------------------------------ K12
def _similar(mem, rank, n_q, top, slices):
    T, _ = TS._table(rank)
    n = len(T)
    rows = np.asarray(TS.QROWS[:n_q], np.int32)
    Td, Qd = mem.table(T, rank), mem.table(T[rows], rank)
    idx = mem.out((n_q, top), I32, prefill=-77)
    sc = mem.out((n_q, top), F32)
    w = mem.scratch(_lib.lib().als_similar_workspace_bytes(n, min(n_q, 16), top, slices))
    _call("als_similar", Td, n, Td.shape[1], rank, Qd, n_q, Qd.shape[1], mem.inp(rows, I32), None,
          top, slices, idx, sc, w, w.numel())
    return dict(idx=idx, score=sc)


@ALIGN
@pytest.mark.parametrize("rank", RANKS)
def test_similar(rank, offset16):
    """als_similar with T, Q, self_rows, both lists and the slice keys' workspace carved:
    slices 1 and 3, 1 and 17 queries (a second pass of 16), top 1 and 256."""
    for slices in (1, 3):
        for n_q in (1, 17):
            for top in (1, 256):
                _bounds(lambda mem: _similar(mem, rank, n_q, top, slices), offset16,
                        capacity=24 << 20)


def test_similar_unit_rows_all_guarded():
    for rank in (17, 128):
        T, allows = TS._table(rank)
        n = 1500 - 3             # 1497: not a multiple of 32, the last mask word is partial
        bits0 = filters.pack_allow_bits(torch.as_tensor(np.nonzero(allows["half"][:n])[0]).to(DEV), n)

        def run(mem):
            Td = mem.table(T[:n], rank)
            out = mem.out((n, Td.shape[1]), F32, offset16=True)
            bits = mem.inp(bits0, I32)
            valid = mem.out((n,), I32, prefill=-77)
            _call("als_similar_unit_rows", Td, n, Td.shape[1], rank, out, bits, valid)
            return dict(unit=out[:, :rank], unit_pad=out[:, rank:], bits=bits, valid=valid)
        got = _bounds(run)
        assert got["valid"].sum().item() == n - 3       # the zero, NaN and Inf rows


# ------------------------------------------------------------------ K13
def _nnls(mem, k, implicit, chunk):
    Y, rows = TN._sources(k, True), TN._rows(k)
    ptr, col, val = TN._csr(rows)
    n, L = len(rows), _lib.lib()
    assert sum(len(c) > chunk for c, _ in rows) >= 2      # rows cut into tasks
    yty = (E.compute_yty(TN._dev(Y), TN.N_SRC, k, E.Workspace(torch.device(DEV)))
           if implicit else None)
    Yd = mem.table(Y, k)
    X = mem.out((n, E.ld_for(k) + (4 if mem.guarded else 0)), F32, offset16=True)
    n_used, iters = mem.out((n,), I32, prefill=-77), mem.out((n,), I32, prefill=-77)
    w = mem.scratch(L.als_nnls_workspace_bytes(n, len(col), k, chunk))
    _call("als_nnls_rows", mem.inp(ptr, I64), mem.inp(col, I32), mem.inp(val, F32, True), n, Yd,
          TN.N_SRC, Yd.shape[1], k, TN.REG, int(implicit), TN.ALPHA,
          None if yty is None else mem.inp(yty, F64), chunk, X, X.shape[1], n_used, iters, w,
          w.numel())
    return dict(X=X[:, :k], X_pad=X[:, k:] if mem.guarded else None, n_used=n_used, iters=iters)


@ALIGN
@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("rank", RANKS)
def test_nnls_rows(rank, implicit, offset16):
    """als_nnls_rows with every argument carved, chunk 32: the 300-rating row and the row of
    40 entries of one item are cut into tasks whose partials live in workspace slots."""
    got = _bounds(lambda mem: _nnls(mem, rank, implicit, 32), offset16)
    assert bool((got["X"] >= 0).all())


# ================================================================== Tier B
@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("rank", (17, 64, 128))
def test_solve_half_all_guarded(rank, implicit):
    """als_solve_half through ctypes: X_dst, status, the CSR, the schedule and yty carved,
    Y_src and val 16 bytes past a boundary (the alignment the header names), ld = ld_for(k)
    + 4 with zero padding in Y_src (required) and the fill in X_dst's."""
    ib, U, yty, ref = _solve_case(rank, implicit)
    n_primal = ib.n_light - (0 if implicit else ib.n_dual(rank))

    def run(mem):
        Y = mem.table(U, rank, pad=0.0)
        X = mem.out((ib.n_rows, Y.shape[1]), F32, offset16=True)
        status = mem.inp(torch.zeros(1, dtype=I32), I32)
        w = mem.scratch(_lib.lib().als_solve_workspace_bytes(rank, ib.n_chunks, 900, ib.n_rows))
        _call("als_solve_half", mem.inp(ib.row_ptr, I64), mem.inp(ib.col, I32),
              mem.inp(ib.val, F32, offset16=True), mem.inp(ib.light_rows, I32), ib.n_light,
              n_primal, mem.inp(ib.heavy_rows, I32), mem.inp(ib.heavy_slot_begin, I32), ib.n_heavy,
              mem.inp(ib.chunk_row, I32), mem.inp(ib.chunk_begin, I64), mem.inp(ib.chunk_end, I64),
              ib.n_chunks, None, 0, Y, 900, X, X.shape[1], rank, SOLVE_REG, int(implicit),
              SOLVE_ALPHA, None if yty is None else mem.inp(yty, F64), status, w, w.numel(),
              E.PHASE_ALL)
        return _solve_outputs(X, rank, status)
    _assert_solve_parity(_bounds(run, offset16=True, plain=False), ref, rank)


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("rank", (1, 33, 128))
def test_fold_in_all_guarded(rank, implicit):
    V, rows = TF._factors(rank), TF._rows(rank)
    ptr, col, val = TF._csr(rows)
    n = len(rows)
    assert _lib.lib().als_fold_in_workspace_bytes(n, rank) == 0
    yty = (E.compute_yty(TF._dev(V), TF.N_ITEMS, rank, E.Workspace(torch.device(DEV)))
           if implicit else None)

    def run(mem):
        Y = mem.table(V, rank)
        X = mem.out((n, Y.shape[1]), F32, offset16=True)
        n_used = mem.out((n,), I32, prefill=-77)
        status = mem.inp(torch.zeros(1, dtype=I32), I32)
        _call("als_fold_in", mem.inp(ptr, I64), mem.inp(col, I32), mem.inp(val, F32), n, Y,
              TF.N_ITEMS, Y.shape[1], rank, TF.REG, int(implicit), TF.ALPHA,
              None if yty is None else mem.inp(yty, F64), X, X.shape[1], n_used, status, None, 0)
        return dict(X=X[:, :rank], X_pad=X[:, rank:] if mem.guarded else None, n_used=n_used,
                    status=status)
    got = _bounds(run)
    assert int(got["status"].item()) == 0
    assert got["n_used"].tolist() == [int(((np.asarray(c) >= 0) & (np.asarray(c) < TF.N_ITEMS)).sum())
                                      for c, _ in rows]


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("rank,top_n", [(1, 1), (33, 10), (128, 32)])
def test_explain_all_guarded(rank, top_n, implicit):
    V, rows = TX._factors(rank), TX._rows(rank)
    targets = TX._targets(rows, TX.N_TARGETS)
    ptr, col, val = TX._csr(rows)
    tptr, tg = TX._ragged(targets)
    n, T = len(rows), len(tg)
    assert _lib.lib().als_explain_workspace_bytes(n, rank) == 0
    yty = (E.compute_yty(TX._dev(V), TX.N_ITEMS, rank, E.Workspace(torch.device(DEV)))
           if implicit else None)

    def run(mem):
        Y = mem.table(V, rank)
        score = mem.out((T,), F32)
        pos = mem.out((T, top_n), I32, prefill=-77)
        contrib = mem.out((T, top_n), F32)
        n_used = mem.out((n,), I32, prefill=-77)
        status = mem.inp(torch.zeros(1, dtype=I32), I32)
        _call("als_explain", mem.inp(ptr, I64), mem.inp(col, I32), mem.inp(val, F32), n, Y,
              TX.N_ITEMS, Y.shape[1], rank, TX.REG, int(implicit), TX.ALPHA,
              None if yty is None else mem.inp(yty, F64), mem.inp(tptr, I64), mem.inp(tg, I32),
              top_n, score, pos, contrib, n_used, status, None, 0)
        return dict(score=score, pos=pos, contrib=contrib, n_used=n_used, status=status)
    got = _bounds(run)
    assert int(got["status"].item()) == 0 and int(got["pos"].min()) >= -1


@pytest.mark.parametrize("filtered", [False, True], ids=["topk", "filtered"])
@pytest.mark.parametrize("rank,top,n_q,n_v", [(17, 17, 129, 257), (64, 33, 257, 2049),
                                              (128, 200, 17, 257), (65, 10, 65, 5)])
def test_topk_all_guarded(rank, top, n_q, n_v, filtered):
    """Q, V, the exclusion ranges, the mask and both [n_q, top] lists carved: a tail lane
    writing row n_q or column `top` lands in a guard."""
    got = _bounds(lambda mem: _topk(mem, rank, top, n_q, n_v, filtered, True), offset16=True)
    assert int(got["idx"].min()) >= -1


@pytest.mark.parametrize("rank,m,top,n_q", [(17, 33, 17, 65), (128, 256, 65, 5), (1, 1, 1, 257)])
def test_diversify_and_list_similarity_all_guarded(rank, m, top, n_q):
    V = TD._table(rank)
    idx, sc = TD._pools(V, rank, n_q, m)
    idx, sc = idx.copy(), sc.copy()
    idx[0, m // 2:] = -1                      # open slots
    sc[0, m // 2:] = -np.inf

    def run(mem):
        Vd = mem.table(V, rank)
        idx_d = mem.inp(idx, I32)
        oi = mem.out((n_q, top), I32, prefill=-77)
        os_ = mem.out((n_q, top), F32)
        ils = mem.out((n_q,), F64)
        _call("als_diversify", Vd, len(V), Vd.shape[1], rank, idx_d, mem.inp(sc, F32), n_q, m, top,
              0.5, oi, os_, ils)
        ils2 = mem.out((n_q,), F64)
        _call("als_list_similarity", Vd, len(V), Vd.shape[1], rank, idx_d, n_q, m, ils2)
        return dict(idx=oi, score=os_, ils=ils, list_similarity=ils2)
    _bounds(run)


@pytest.mark.parametrize("rank", (17, 65, 128))
def test_predict_all_guarded(rank):
    core = TR._core(rank)
    for n in (1, 257):
        u, i, _ = TR._pairs(n, seed=n)
        u[n // 2] = 10 ** 6

        def run(mem):
            umap, imap = mem.inp(core.uidx.map, I32), mem.inp(core.iidx.map, I32)
            U, V = mem.table(core.U, rank), mem.table(core.V, rank)
            out = mem.out((n,), F64)
            _call("als_predict", mem.inp(core.uidx.keys(torch.as_tensor(u).to(DEV)), I32),
                  mem.inp(core.iidx.keys(torch.as_tensor(i).to(DEV)), I32), n, umap,
                  umap.numel(), imap, imap.numel(), U, V, U.shape[1], rank, out)
            return dict(pred=out)
        got = _bounds(run)
        assert bool(got["pred"][n // 2].isnan()) and int(got["pred"].isnan().sum()) == 1


@pytest.mark.parametrize("n_rows,nnz", [(257, 4097), (2048, 3000)])
def test_csr_build_all_guarded(n_rows, nnz):
    """row_ptr [n_rows + 1], col [nnz] and val [nnz] out, the id lists and maps in."""
    rows, cols, vals = _csr_inputs(n_rows, nnz)

    def run(mem):
        ar = lambda n: torch.arange(n, dtype=I32)
        row_ptr = mem.out((n_rows + 1,), I64)
        col, val = mem.out((nnz,), I32, prefill=-77), mem.out((nnz,), F32)
        w = mem.scratch(_lib.lib().als_csr_workspace_bytes(nnz, n_rows))
        _call("als_csr_build", mem.inp(rows, I32), mem.inp(ar(n_rows), I32), mem.inp(cols, I32),
              mem.inp(ar(TK1.N_COLS), I32), mem.inp(vals, F32), nnz, n_rows, row_ptr, col, val, w,
              w.numel())
        return dict(row_ptr=row_ptr, col=col, val=val)
    got = _bounds(run, offset16=True)
    ptr_, idx_, val_ = O.csr_build(rows, cols, vals, n_rows)
    np.testing.assert_array_equal(got["row_ptr"].cpu().numpy(), ptr_)
    np.testing.assert_array_equal(got["col"].cpu().numpy(), idx_)
    np.testing.assert_array_equal(got["val"].cpu().numpy(), val_)
