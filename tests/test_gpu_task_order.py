"""Launch-1 task order of the rank 33-64 explicit half-sweep (csrc/task_order.h): every
chunk and every light row is visited exactly once at the corner shapes of the merge, and
the order of the light list never changes a result.

Every row (light and heavy: a missed chunk leaves a stale partial slot) against the fp64
oracle from identical source factors, the K2/K3 bar of test_gpu_kernels.py: max over rows
of ||x - x_ref|| / ||x_ref|| <= 1e-4, after X was poisoned with NaN."""
import dataclasses

import numpy as np
import pytest
import torch

import als_mi355x.engine as E
from oracle import als_oracle as O
from helpers import rel_row_errs, report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RANK, REG, CHUNK, N_ITEMS = 64, 0.1, 64, 400


def _degree_data(degrees, seed):
    """Users with exactly the given degrees (distinct items each), planted half-star ratings."""
    rng = np.random.default_rng(seed)
    u = np.concatenate([np.full(d, uid) for uid, d in enumerate(degrees)]).astype(np.int32)
    i = np.concatenate([rng.choice(N_ITEMS, d, replace=False) for d in degrees]).astype(np.int32)
    uf = rng.normal(0, 0.35, (len(degrees), 8))
    vf = rng.normal(0, 0.35, (N_ITEMS, 8))
    r = np.clip(np.round((3.6 + (uf[u] * vf[i]).sum(1) + rng.normal(0, 0.8, len(u))) * 2) / 2,
                0.5, 5).astype(np.float32)
    return u, i, r


def _setup(degrees, seed):
    u, i, r = _degree_data(degrees, seed)
    core = E.ALSCore(u, i, r, device=DEV, chunk=CHUNK)
    core.init_factors(RANK, seed=3)
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    V0 = torch.randn((core.n_items, RANK), generator=g, device=DEV)
    V0 = V0 / torch.linalg.vector_norm(V0, dim=1, keepdim=True)
    core.V[:, :RANK] = V0
    ub = core.user_block
    U_ref = O.half_sweep(ub.row_ptr.cpu().numpy(), ub.col.cpu().numpy(), ub.val.cpu().numpy(),
                         V0.cpu().numpy(), REG)
    return core, ub, U_ref


def _one_chunk(ub):
    """The block with its single heavy row as one chunk task (K1 cuts a heavy row into at
    least two): n_chunks = 1."""
    assert ub.n_heavy == 1 and ub.n_chunks == 2
    return dataclasses.replace(
        ub, n_chunks=1, chunk_row=ub.chunk_row[:1].clone(), chunk_begin=ub.chunk_begin[:1].clone(),
        chunk_end=ub.chunk_end[1:2].clone(),
        heavy_slot_begin=torch.tensor([0, 1], dtype=torch.int32, device=DEV))


def _sweep(core, blk, dual=False):
    core.U.fill_(float("nan"))
    core.status.zero_()
    E.solve_half(blk, core.V, core.U, RANK, REG, False, 1.0, None, core.status, core.ws, dual=dual)
    torch.cuda.synchronize()
    core.check_status()
    return core.U.clone()


MIXED = [1 + (37 * j) % 64 for j in range(300)]  # ~300 light rows, 1..64 ratings
CASES = {
    # name: (degrees, n_chunks, n_light)
    "no_chunks_5_light": ([5, 9, 33, 40, 50], 0, 5),
    "one_chunk_2_light": ([100, 12, 40], 1, 2),
    "chunks_only": ([200], 4, 0),
    "chunks_1_light": ([200, 40], 4, 1),          # nA = n_light
    "more_chunks_than_light": ([200, 5, 40], 4, 2),
    "chunks_5_light": ([300, 3, 17, 33, 48, 64], 5, 5),
    "300_light_3_chunks": (MIXED + [2 * CHUNK + 2], 3, 300),  # a row just over two chunks
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_task_once(name):
    degrees, n_chunks, n_light = CASES[name]
    core, ub, U_ref = _setup(degrees, seed=len(degrees))
    blk = _one_chunk(ub) if name.startswith("one_chunk") else ub
    assert (blk.n_chunks, blk.n_light) == (n_chunks, n_light)
    U = _sweep(core, blk).cpu().numpy()
    assert np.isfinite(U[:, :RANK]).all(), np.argwhere(~np.isfinite(U[:, :RANK]).all(1)).ravel()
    assert np.all(U[:, RANK:] == 0.0)
    e = rel_row_errs(U[:, :RANK], U_ref)
    deg = np.diff(ub.row_ptr.cpu().numpy())
    report(f"task_order[{name}]", {"max_rel": float(e.max()),
                                   "max_rel_heavy": float(e[deg > CHUNK].max()) if n_chunks else None})
    assert e.max() <= 1e-4, (name, float(e.max()), int(e.argmax()))


@pytest.mark.parametrize("dual", [False, True])
def test_light_order_never_changes_a_result(dual):
    """The primal part of light_rows shuffled: bit-identical factors (with and without a
    dual tail behind it)."""
    degrees, _, _ = CASES["300_light_3_chunks"]
    core, ub, U_ref = _setup(degrees, seed=7)
    n_primal = ub.n_light - (ub.n_dual(RANK) if dual else 0)
    assert 0 < n_primal <= ub.n_light and (n_primal < ub.n_light) == dual
    U1 = _sweep(core, ub, dual)
    g = torch.Generator(device="cpu")
    g.manual_seed(5)
    lr = ub.light_rows.clone()
    lr[:n_primal] = lr[:n_primal][torch.randperm(n_primal, generator=g).to(DEV)]
    U2 = _sweep(core, dataclasses.replace(ub, light_rows=lr), dual)
    assert torch.equal(U1, U2)
    assert rel_row_errs(U1[:, :RANK].cpu().numpy(), U_ref).max() <= 1e-4
