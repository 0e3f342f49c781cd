"""Multi-process (world_size 2 and 8, gloo, CPU) test of the sharded ALS coordination
(als_mi355x.distributed.ShardedALS): id-space agreement, nnz-balanced row
ranges, the one-time all_to_all rating routing, padded factor layout, per
half-sweep all_gather and the implicit YtY all_reduce.

The HIP kernels cannot run on a CPU, so the arithmetic is injected: the test
passes `OracleKernels` (the CPU oracle behind ShardedALS's kernel interface).
The result must equal a single-process oracle fit from the same initial
factors — i.e. sharding changes nothing but where rows are solved."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import planted


class OracleKernels:
    """CPU oracle behind the kernel interface of ShardedALS (test only)."""

    def __init__(self):
        from oracle import als_oracle as O
        self.O = O

    def index_build(self, ids, id_space):
        mp_, uniq = self.O.index_build(ids.numpy(), id_space)
        return torch.as_tensor(mp_), torch.as_tensor(uniq), len(uniq)

    def build_block(self, rows, cols, vals, n_rows, n_cols):
        ptr, idx, val = self.O.csr_build(rows.numpy(), cols.numpy(), vals.numpy(), n_rows)
        return (ptr, idx, val)

    def yty(self, Y, n, rank):
        return torch.as_tensor(self.O.yty(Y[:n, :rank].numpy()))

    def solve_half(self, block, Y, X, rank, reg, implicit, alpha, yty, status, first=True):
        ptr, idx, val = block
        n = len(ptr) - 1
        if n == 0:
            return
        A, b, ne = self.O.normal_equations(ptr, idx, val, Y[:, :rank].numpy(), implicit, alpha)
        x = self.O.solve(A, b, ne, reg, None if yty is None else yty.numpy())
        X[:n, :rank] = torch.as_tensor(x)

    def split_schedule(self, block, seg, n_src_early, slot_base=0):
        return {"seg": np.asarray(seg.cpu()), "n_src_early": int(n_src_early), "part": None}

    def solve_split(self, block, sched, part, Y, X, rank, reg, implicit, alpha, yty, status,
                    first):
        """Two-segment half-sweep: the early part's normal equations from the early
        rating segments with every source row past n_src_early poisoned (NaN: the early
        part must never read the chunk still in flight), the late part's added in fp64."""
        ptr, idx, val = block
        n = len(ptr) - 1
        if n == 0:
            return
        row_of = np.repeat(np.arange(n), np.diff(ptr))
        early = np.arange(len(idx)) < sched["seg"][row_of]
        mask = early if part == "early" else ~early
        sub = np.zeros(n + 1, dtype=np.int64)
        sub[1:] = np.cumsum(np.bincount(row_of[mask], minlength=n))
        Ym = Y[:, :rank].numpy().copy()
        if part == "early":
            Ym[sched["n_src_early"]:] = np.nan
        A, b, ne = self.O.normal_equations(sub, idx[mask], val[mask], Ym, implicit, alpha)
        if part == "early":
            sched["part"] = (A, b, ne)
            return
        A0, b0, ne0 = sched["part"]
        sched["part"] = None
        x = self.O.solve(A0 + A, b0 + b, ne0 + ne, reg, None if yty is None else yty.numpy())
        X[:n, :rank] = torch.as_tensor(x)

    def predict(self, u_keys, i_keys, umap, imap, U, V, rank):
        u, i = u_keys.long(), i_keys.long()
        ok = (u >= 0) & (i >= 0)
        ur = torch.where(ok, umap[u.clamp(min=0)].long(), -1)
        ir = torch.where(ok, imap[i.clamp(min=0)].long(), -1)
        ok = ok & (ur >= 0) & (ir >= 0)
        out = torch.full((len(u),), float("nan"), dtype=torch.float64)
        out[ok] = (U[ur[ok], :rank].double() * V[ir[ok], :rank].double()).sum(1)
        return out

    def rmse_partial(self, u_keys, i_keys, r, umap, imap, U, V, rank):
        p = self.predict(u_keys, i_keys, umap, imap, U, V, rank)
        ok = ~torch.isnan(p)
        d = r.double()[ok] - p[ok]
        return torch.tensor([float((d * d).sum()), float(ok.sum())], dtype=torch.float64)

    def topk(self, Q, n_q, V, n_v, rank, top):
        i, s = self.O.topk(Q[:n_q, :rank].numpy(), V[:n_v, :rank].numpy(), top)
        return torch.as_tensor(i), torch.as_tensor(s, dtype=torch.float32)

    def ld(self, rank):
        return rank

    def block_values(self, block):
        return torch.as_tensor(block[2])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, implicit, chunks, out_dir, pipeline=None, exchange="ring"):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import _pkgload
    _pkgload.load()
    from als_mi355x.distributed import ShardedALS
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    u, i, r = planted(120, 90, density=0.08, seed=21, heavy_items=(3,), dup=10)
    if implicit:
        r = (r - 2.5).astype(np.float32)
    # arbitrary (non-aligned) input sharding: interleaved ratings
    sel = np.arange(len(u)) % world == rank
    K = ShardedALS(u[sel], i[sel], r[sel], device="cpu", kernels=OracleKernels(), chunks=chunks,
                   pipeline=pipeline, exchange=exchange)
    from oracle import als_oracle as O
    n_users = len(np.unique(u))
    U0 = O.initialize(n_users, 6, seed=2)
    K.fit(6, 3, 0.1, implicit=implicit, alpha=2.0, U0_global=U0)
    uid, Uf = K.user_factors()
    iid, Vf = K.item_factors()
    if rank == 0:
        np.savez(os.path.join(out_dir, f"dist_{int(implicit)}_{chunks}_{world}.npz"), uid=uid.numpy(),
                 U=Uf.numpy(), iid=iid.numpy(), V=Vf.numpy(), nnz=K.nnz,
                 u_starts=K.users.starts.numpy(), i_starts=K.items.starts.numpy(),
                 local=[K.user_rows, K.item_rows], pipeline=K.pipeline)
    dist.destroy_process_group()


def _serve_worker(rank, world, port, out_dir):
    """Seeded fit (no explicit U0) + rmse / predict / recommendForAll on world ranks."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import _pkgload
    _pkgload.load()
    from als_mi355x.distributed import ShardedALS
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    u, i, r = planted(90, 70, density=0.1, seed=31, heavy_items=(2,))
    u = (u - 40).astype(np.int32)  # negative user ids are legal (Spark Int ids)
    sel = np.arange(len(u)) % world == rank
    K = ShardedALS(u[sel], i[sel], r[sel], device="cpu", kernels=OracleKernels())
    K.fit(5, 2, 0.1, seed=11)
    rm, n = K.rmse(u[sel], i[sel], r[sel])  # every rank passes its own pairs
    q_u = np.array([u[0], u[1], 10 ** 6, -(10 ** 6)], np.int32)
    q_i = np.array([i[0], i[1], i[2], i[3]], np.int32)
    pred = K.predict(q_u, q_i).numpy()
    keys, ids, sc = K.recommend_all(7, True)
    skeys, sids, ssc = K.recommend_subset(np.array([i[5], i[5], 10 ** 7], np.int32), 4, False)
    uid, Uf = K.user_factors()
    iid, Vf = K.item_factors()
    np.savez(os.path.join(out_dir, f"serve_{world}_{rank}.npz"), rmse=rm, n=n, pred=pred,
             keys=keys.numpy(), ids=ids.numpy(), sc=sc.numpy(), skeys=skeys.numpy(),
             sids=sids.numpy(), ssc=ssc.numpy(), uid=uid.numpy(), U=Uf.numpy(),
             iid=iid.numpy(), V=Vf.numpy())
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [1, 2])
def test_sharded_serving_matches_oracle(tmp_path, world):
    """Seeded init over the global dense rows (independent of world size), the
    distributed RMSE (all_reduce of the fused partials), predict on replicated
    factors, and recommendForAll over each rank's own users, vs a single-process
    oracle fit from the same seeded start."""
    mp.spawn(_serve_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    from oracle import als_oracle as O
    u, i, r = planted(90, 70, density=0.1, seed=31, heavy_items=(2,))
    u = (u - 40).astype(np.int32)
    n_users = len(np.unique(u))
    g = torch.Generator(device="cpu")
    g.manual_seed(11)
    x = torch.randn((n_users, 5), generator=g, dtype=torch.float32)
    U0 = (x / torch.linalg.vector_norm(x, dim=1, keepdim=True)).numpy()
    U, V, umap, imap, uids, iids = O.train(u + 40, i, r, 5, 2, 0.1, U0=U0)
    uids = uids - 40
    sse, n_ref = O.rmse(U, V, umap, imap, u + 40, i, r)
    parts = [np.load(tmp_path / f"serve_{world}_{w}.npz") for w in range(world)]
    for d in parts:
        np.testing.assert_array_equal(d["uid"], uids)
        np.testing.assert_allclose(d["U"], U, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(d["V"], V, rtol=1e-5, atol=1e-6)
        assert int(d["n"]) == n_ref == len(u)
        assert abs(float(d["rmse"]) - np.sqrt(sse / n_ref)) <= 1e-9
        assert np.isnan(d["pred"][2:]).all() and not np.isnan(d["pred"][:2]).any()
    # recommendForAll: the union of the ranks' partitions is every user exactly once
    keys = np.concatenate([d["keys"] for d in parts])
    ids = np.concatenate([d["ids"] for d in parts])
    np.testing.assert_array_equal(np.sort(keys), uids)
    ref_i, ref_s = O.topk(U, V, 7)
    order = np.argsort(keys)
    np.testing.assert_array_equal(ids[order], iids[ref_i])
    d = parts[0]
    assert list(d["skeys"]) == [i[5]]
    row = int(np.searchsorted(iids, i[5]))
    ref_u, _ = O.topk(V[row:row + 1], U, 4)
    np.testing.assert_array_equal(d["sids"][0], uids[ref_u[0]])


@pytest.mark.parametrize("implicit,chunks,world,pipeline,exchange",
                         [(False, None, 2, None, "ring"), (True, None, 2, None, "ring"),
                          (False, 3, 2, True, "ring"), (True, 3, 2, True, "ring"),
                          (False, 3, 2, None, "ring"), (True, 3, 2, "auto", "ring"),
                          (False, 2, 8, True, "ring"), (True, 2, 8, True, "ring"),
                          (True, None, 8, None, "ring"),
                          (False, 3, 2, True, "peers"), (True, 2, 8, True, "peers"),
                          (False, None, 8, None, "peers")])
def test_sharded_als_matches_single_process(tmp_path, implicit, chunks, world, pipeline,
                                            exchange):
    """chunks=3: the [C, world, rows] layout with async per-chunk exchanges; with several
    ranks and >= 2 chunks, pipeline=True pipelines the item half-sweep: the item rows'
    early partials (users of chunks 0..C-2, every later source row poisoned with NaN in
    the oracle kernels) are formed while the last user chunk's exchange is in flight,
    the late ones after (all item chunks on one shared workspace, one Y prep per part);
    None (the default) runs the plain chunked exchange, "auto" asks the exchange model
    at the fit's rank (never for these tiny shapes).  exchange="peers": batched isend /
    irecv to every peer instead of the ring all-gather.  world 8: the target world size
    of BASELINE configs[3] (8 x MI355X), every rank a range of ~15 users and ~11 items,
    the full 3-iteration fit against the single-process oracle."""
    mp.spawn(_worker, args=(world, _free_port(), implicit, chunks, str(tmp_path), pipeline,
                            exchange), nprocs=world, join=True)
    d = np.load(tmp_path / f"dist_{int(implicit)}_{chunks}_{world}.npz")
    assert bool(d["pipeline"]) == (pipeline is True)
    from oracle import als_oracle as O
    u, i, r = planted(120, 90, density=0.08, seed=21, heavy_items=(3,), dup=10)
    if implicit:
        r = (r - 2.5).astype(np.float32)
    assert int(d["nnz"]) == len(u)
    U0 = O.initialize(len(np.unique(u)), 6, seed=2)
    U, V, umap, imap, uids, iids = O.train(u, i, r, 6, 3, 0.1, implicit=implicit, alpha=2.0,
                                           U0=U0)
    np.testing.assert_array_equal(d["uid"], uids)
    np.testing.assert_array_equal(d["iid"], iids)
    np.testing.assert_allclose(d["U"], U, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(d["V"], V, rtol=1e-5, atol=1e-6)
    # both ranks got a share of the rows; ranges cover all rows
    assert d["u_starts"][0] == 0 and d["u_starts"][-1] == len(uids)
    assert d["i_starts"][-1] == len(iids)
    assert all(x > 0 for x in np.diff(d["u_starts"]))


def _route_worker(rank, world, port, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import _pkgload
    _pkgload.load()
    from als_mi355x import distributed as Dm
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    # ids spread over a 20x wider space: the id-flag all_reduce of the setup covers
    # 2,400 user ids (9.6 KB of int32) and must split under the small cap
    u, i, r = planted(120, 90, density=0.08, seed=21, heavy_items=(3,), dup=10)
    u = u * 20
    sel = np.arange(len(u)) % world == rank
    ck = os.path.join(out_dir, "ckpt_route")
    ref = Dm.ShardedALS(u[sel], i[sel], r[sel], device="cpu", kernels=OracleKernels(), chunks=2)
    ref.fit(4, 2, 0.1, seed=3, checkpoint_dir=ck, checkpoint_interval=1)
    ref_rmse = ref.rmse(u[sel], i[sel], r[sel])
    # record the bytes of every collective call the package issues from here on
    sizes = []
    real = {n: getattr(dist, n) for n in ("all_reduce", "broadcast", "all_to_all_single",
                                          "all_gather_into_tensor")}

    def rec(name):
        def f(*a, **kw):
            ts = [x for x in a if isinstance(x, torch.Tensor)]
            sizes.append((name, max(x.numel() * x.element_size() for x in ts)))
            return real[name](*a, **kw)
        return f
    for n in real:
        setattr(dist, n, rec(n))
    Dm.MAX_COLLECTIVE_BYTES = 64  # forces many routing rounds, chunks and split reduces
    small = Dm.ShardedALS(u[sel], i[sel], r[sel], device="cpu", kernels=OracleKernels())
    ok = small.chunks >= 2
    for a, b in ((ref.user_blocks, small.user_blocks), (ref.item_blocks, small.item_blocks)):
        ok = ok and sum(x[0][-1] for x in a if x is not None) == \
            sum(x[0][-1] for x in b if x is not None)
    small.fit(4, 2, 0.1, U0_global=None, seed=3)  # every call within the 64-byte cap
    small_rmse = small.rmse(u[sel], i[sel], r[sel])
    # a resume broadcasts the checkpointed factor tables (split under the cap too)
    res = Dm.ShardedALS(u[sel], i[sel], r[sel], device="cpu", kernels=OracleKernels())
    res.fit(4, 2, 0.1, seed=3, checkpoint_dir=ck, checkpoint_interval=0, resume=True)
    for n, f in real.items():
        setattr(dist, n, f)
    _, Ua = ref.user_factors()
    _, Ub = small.user_factors()
    _, Ur = res.user_factors()
    flags = [b for n, b in sizes if n == "all_reduce" and b == 64]
    np.save(os.path.join(out_dir, f"route_{rank}.npy"),
            np.array([float(ok), float(np.abs(Ua.numpy() - Ub.numpy()).max()),
                      float(max(b for _, b in sizes)), float(len(sizes)),
                      float(len(flags)), abs(ref_rmse[0] - small_rmse[0]),
                      float(np.abs(Ua.numpy() - Ur.numpy()).max()),
                      float(sum(1 for n, _ in sizes if n == "broadcast"))]))
    dist.destroy_process_group()


def test_chunked_collectives_match(tmp_path):
    """With MAX_COLLECTIVE_BYTES lowered to 64: routing in several all_to_all rounds,
    factor all-gathers in more chunks, the setup's id-flag / degree all_reduces and a
    resume's factor broadcast split into pieces — every collective call the package
    issues (recorded at the torch.distributed functions) is within the cap, and the
    blocks, the fit, the RMSE and the resumed factors equal the uncapped run's."""
    mp.spawn(_route_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for w in range(2):
        ok, diff, biggest, n_calls, n_full_reduces, drmse, dres, n_bcast = \
            np.load(tmp_path / f"route_{w}.npy")
        assert ok == 1.0 and diff <= 1e-5
        assert biggest <= 64 and n_calls > 0
        assert n_full_reduces >= 2  # the flag / degree arrays went out in 64-byte pieces
        assert drmse <= 1e-9 and dres == 0.0 and n_bcast > 1


def _resume_worker(rank, world, port, out_dir, mode):
    """mode "full": 4 iterations; "ckpt": 2 iterations writing a checkpoint every 2;
    "resume": resume=True to 4 iterations; "at": resume at the checkpoint's own count."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import _pkgload
    _pkgload.load()
    from als_mi355x.distributed import ShardedALS
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    u, i, r = planted(100, 80, density=0.09, seed=41, heavy_items=(5,))
    sel = np.arange(len(u)) % world == rank
    K = ShardedALS(u[sel], i[sel], r[sel], device="cpu", kernels=OracleKernels())
    ck = os.path.join(out_dir, "ckpt")
    # resumes read the checkpoint on process 0 only (rank 1 is given an empty directory:
    # no shared filesystem) and broadcast the decision and the factors
    ck_r = ck if rank == 0 else os.path.join(out_dir, f"empty_{mode}_{rank}")
    if mode == "full":
        K.fit(5, 4, 0.1, seed=7)
    elif mode == "fresh99":
        K.fit(5, 4, 0.1, seed=99)
    elif mode == "ckpt":
        K.fit(5, 2, 0.1, seed=7, checkpoint_dir=ck, checkpoint_interval=2)
    elif mode == "resume":
        K.fit(5, 4, 0.1, seed=99, checkpoint_dir=ck_r, checkpoint_interval=0, resume=True)
    elif mode == "auto7":  # same seed: "auto" resumes
        K.fit(5, 4, 0.1, seed=7, checkpoint_dir=ck_r, checkpoint_interval=0, resume="auto")
    elif mode == "auto99":  # other seed: a different fit, "auto" starts fresh
        K.fit(5, 4, 0.1, seed=99, checkpoint_dir=ck_r, checkpoint_interval=0, resume="auto")
    elif mode == "broken":  # the generation directory named by als_state.json is gone
        import json
        import shutil
        if rank == 0:
            gen = json.load(open(os.path.join(ck, "als_state.json")))["generation"]
            shutil.rmtree(os.path.join(ck, gen))
        err = ""
        try:
            K.fit(5, 4, 0.1, seed=7, checkpoint_dir=ck_r, checkpoint_interval=0, resume="auto")
        except RuntimeError as e:
            err = str(e)
        np.save(os.path.join(out_dir, f"broken_{rank}.npy"),
                np.array([float("unreadable" in err)]))
        dist.destroy_process_group()
        return
    else:  # "at": nothing left to run, U and V come from the checkpoint
        K.fit(5, 2, 0.1, seed=99, checkpoint_dir=ck_r, checkpoint_interval=0, resume=True)
    _, Uf = K.user_factors()
    _, Vf = K.item_factors()
    if rank == 0:
        np.savez(os.path.join(out_dir, f"{mode}_w{world}.npz"), U=Uf.numpy(), V=Vf.numpy())
    dist.destroy_process_group()


def test_checkpoint_resume_across_world_sizes(tmp_path):
    """A fit checkpointed at iteration 2 on 1 rank and resumed to 4 on 2 ranks gives
    the uninterrupted 4-iteration factors: with resume=True the resume's own seed is
    ignored; with "auto" the seed must match (another seed is another fit and starts
    fresh).  Only process 0 sees the checkpoint; every rank resumes alike."""
    from als_mi355x import checkpoint as C
    for mode, world in (("full", 2), ("fresh99", 2), ("ckpt", 1), ("resume", 2), ("at", 2),
                        ("auto7", 2), ("auto99", 2)):
        mp.spawn(_resume_worker, args=(world, _free_port(), str(tmp_path), mode), nprocs=world,
                 join=True)
    full = np.load(tmp_path / "full_w2.npz")
    for mode in ("resume", "auto7"):
        res = np.load(tmp_path / f"{mode}_w2.npz")
        np.testing.assert_array_equal(res["U"], full["U"])
        np.testing.assert_array_equal(res["V"], full["V"])
    a99 = np.load(tmp_path / "auto99_w2.npz")
    np.testing.assert_array_equal(a99["U"], np.load(tmp_path / "fresh99_w2.npz")["U"])
    assert not np.array_equal(a99["U"], full["U"])
    st = C.load(str(tmp_path / "ckpt"))
    assert st.iteration == 2 and st.init == {"seed": 7}
    at = np.load(tmp_path / "at_w2.npz")
    np.testing.assert_array_equal(at["U"], st.U)
    np.testing.assert_array_equal(at["V"], st.V)
    # a checkpoint whose generation directory is missing: process 0 fails to read it
    # and the failure is broadcast, so every rank raises (none waits in a collective)
    mp.spawn(_resume_worker, args=(2, _free_port(), str(tmp_path), "broken"), nprocs=2, join=True)
    for w in range(2):
        assert np.load(tmp_path / f"broken_{w}.npy")[0] == 1.0


def _surface_worker(rank, world, port, out_dir):
    """ml.ALS.fit / transform / recommendForAllUsers and mllib ALS.train / predictAll on
    this rank's partition, through make_engine -> ShardedALS (kernels: the oracle)."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import _pkgload
    _pkgload.load()
    import pandas as pd
    from als_mi355x import distributed as Dm
    from als_mi355x import engine as Em
    from als_mi355x.ml.recommendation import ALS as MLALS
    from als_mi355x.mllib.recommendation import ALS as MLlibALS
    Dm.HipKernels = lambda device, chunk=None: OracleKernels()  # no GPU here
    # ... also on a host that has one: the oracle kernels are host code, so the engine's
    # default device (this worker process only) must be the CPU
    torch.cuda.is_available = lambda: False
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    u, i, r = planted(80, 60, density=0.12, seed=51, heavy_items=(1,))
    sel = np.arange(len(u)) % world == rank
    df = pd.DataFrame({"user": u[sel], "item": i[sel], "rating": r[sel]})
    model = MLALS(rank=4, maxIter=3, regParam=0.1, seed=13).fit(df)
    assert isinstance(model.engine, Dm.ShardedALS)
    test = pd.DataFrame({"user": [u[0], u[1], 999], "item": [i[0], i[1], i[2]]})
    pred = model.transform(test)["prediction"].to_numpy()
    recs = model.recommendForAllUsers(5)
    ml_users = recs["user"].to_numpy()
    ml_items = np.array([[x[0] for x in row] for row in recs["recommendations"]])
    mm = MLlibALS.train(np.stack([u[sel], i[sel], r[sel]], 1), 4, iterations=3, lambda_=0.1,
                        seed=13)
    assert isinstance(mm.engine, Dm.ShardedALS)
    pa = mm.predictAll([(int(u[2]), int(i[2])), (999, int(i[0]))])
    assert Em.make_engine is not None
    np.savez(os.path.join(out_dir, f"surface_{rank}.npz"), pred=pred, users=ml_users,
             items=ml_items, pa=np.array([[p[0], p[1], p[2]] for p in pa], dtype=np.float64))
    dist.destroy_process_group()


def test_ml_and_mllib_surface_on_sharded_engine(tmp_path):
    """With a process group of world size 2 initialised, ml/mllib fit builds the
    sharded engine; predictions, recommendForAllUsers (each rank its own users) and
    predictAll match a single-process oracle fit from the same seeded start."""
    world = 2
    mp.spawn(_surface_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    from oracle import als_oracle as O
    u, i, r = planted(80, 60, density=0.12, seed=51, heavy_items=(1,))
    n_users = len(np.unique(u))
    g = torch.Generator(device="cpu")
    g.manual_seed(13)
    x = torch.randn((n_users, 4), generator=g, dtype=torch.float32)
    U0 = (x / torch.linalg.vector_norm(x, dim=1, keepdim=True)).numpy()
    U, V, umap, imap, uids, iids = O.train(u, i, r, 4, 3, 0.1, U0=U0)
    ref_pred = [float(U[umap[u[0]]] @ V[imap[i[0]]]), float(U[umap[u[1]]] @ V[imap[i[1]]])]
    parts = [np.load(tmp_path / f"surface_{w}.npz") for w in range(world)]
    ref_i, _ = O.topk(U, V, 5)
    for d in parts:
        np.testing.assert_allclose(d["pred"][:2], ref_pred, rtol=1e-5, atol=1e-6)
        assert np.isnan(d["pred"][2])
        assert len(d["pa"]) == 1 and d["pa"][0][0] == u[2] and d["pa"][0][1] == i[2]
        np.testing.assert_allclose(d["pa"][0][2], U[umap[u[2]]] @ V[imap[i[2]]], rtol=1e-5)
    users = np.concatenate([d["users"] for d in parts])
    items = np.concatenate([d["items"] for d in parts])
    np.testing.assert_array_equal(np.sort(users), uids)
    order = np.argsort(users)
    np.testing.assert_array_equal(items[order], iids[ref_i])


def test_ranges_cap_padding_with_popularity_ordered_ids():
    """Row ids that correlate with popularity (unpermuted Zipf: id 0 the most popular)
    make pure nnz balance hand the last range most of the rows; the ranges are capped
    at PAD_CAP x the mean rows, so the replicated (padded) tables stay within 1.25x."""
    import math
    import _pkgload
    _pkgload.load()
    from als_mi355x import distributed as Dm
    n = 1_000_000
    p = 1.0 / np.arange(1, n + 1) ** 0.9
    deg = torch.as_tensor(np.maximum(1, np.round(1e9 * p / p.sum())).astype(np.int64))
    for parts in (2, 4, 8):
        st = Dm._ranges(deg, parts)
        rows = (st[1:] - st[:-1]).numpy()
        assert rows.sum() == n and st[0] == 0 and st[-1] == n
        assert rows.max() <= math.ceil(Dm.PAD_CAP * n / parts)
        assert parts * rows.max() / n <= Dm.PAD_CAP + 1e-6
        # uncapped nnz balance would have padded far more
        old = np.searchsorted(np.cumsum(deg.numpy()), [deg.sum().item() * w / parts
                                                       for w in range(1, parts)], side="right")
        old_rows = np.diff(np.concatenate([[0], old, [n]]))
        assert parts * old_rows.max() / n > 1.5


def _padding_worker(rank, world, port, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import _pkgload
    _pkgload.load()
    from als_mi355x.distributed import ShardedALS
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rng = np.random.default_rng(8)
    n_u, n_i = 400, 300
    # popularity follows the id: Zipf over item ids, user degrees decreasing with id
    pi = 1.0 / np.arange(1, n_i + 1) ** 0.9
    pi /= pi.sum()
    du = np.maximum(2, (60 / np.arange(1, n_u + 1) ** 0.5).astype(int))
    us, its = [], []
    for uid in range(n_u):
        its.append(rng.choice(n_i, min(du[uid], n_i), replace=False, p=pi))
        us.append(np.full(len(its[-1]), uid))
    u = np.concatenate(us).astype(np.int32)
    i = np.concatenate(its).astype(np.int32)
    # every item rated at least once
    miss = np.setdiff1d(np.arange(n_i), i)
    u = np.concatenate([u, rng.integers(0, n_u, len(miss))]).astype(np.int32)
    i = np.concatenate([i, miss]).astype(np.int32)
    r = np.clip(np.round(rng.normal(3.5, 1.0, len(u)) * 2) / 2, 0.5, 5).astype(np.float32)
    sel = np.arange(len(u)) % world == rank
    K = ShardedALS(u[sel], i[sel], r[sel], device="cpu", kernels=OracleKernels(), chunks=2)
    from oracle import als_oracle as O
    U0 = O.initialize(len(np.unique(u)), 5, seed=3)
    K.fit(5, 2, 0.1, U0_global=U0)
    _, Uf = K.user_factors()
    ex = K.exchange_stats()
    if rank == 0:
        U_ref, *_ = O.train(u, i, r, 5, 2, 0.1, U0=U0)
        np.save(os.path.join(out_dir, f"pad_{world}.npy"),
                np.array([ex["padding_users"], ex["padding_items"],
                          float(np.abs(Uf.numpy() - U_ref).max())]))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_padding_bounded_with_popularity_ordered_ids(tmp_path, world):
    mp.spawn(_padding_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    pu, pi, diff = np.load(tmp_path / f"pad_{world}.npy")
    assert pu <= 1.25 + 1e-9 and pi <= 1.25 + 1e-9, (pu, pi)
    assert diff <= 1e-4


def test_auto_chunks_keep_every_chunk_gather_within_the_cap():
    """_auto_chunks counts a chunk's all-gather exactly (W x the per-chunk row cap x
    512 B), for world sizes that are not powers of two too, and adds no chunk beyond
    what the cap needs.  Floors: 4 chunks from 1M rows per rank, 2 from 64k rows per
    rank at 4+ ranks (the weak-scaled configs[1] shape: chunk 0's all-gather hides
    behind chunk 1's solve), else 1."""
    import math
    from types import SimpleNamespace
    import _pkgload
    _pkgload.load()
    from als_mi355x import distributed as Dm
    for W in (1, 2, 3, 5, 6, 7, 8):
        for big in (1000, 162_541, 1_000_000, 10_000_000, 10_000_019, 123_456_789):
            c = Dm.ShardedALS._auto_chunks(SimpleNamespace(world=W), big, 7)
            rows = math.ceil(Dm.PAD_CAP * big / (W * c))
            assert W * rows * 512 <= Dm.MAX_COLLECTIVE_BYTES, (W, big, c)
            floor = 4 if (W > 1 and big // W >= (1 << 20)) else \
                (2 if (W >= 4 and big // W >= (1 << 16)) else 1)
            assert c >= floor
            if c > floor:  # one chunk fewer would break the cap
                assert W * math.ceil(Dm.PAD_CAP * big / (W * (c - 1))) * 512 > \
                    Dm.MAX_COLLECTIVE_BYTES


def _guard_worker(rank, world, port, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import _pkgload
    _pkgload.load()
    from als_mi355x import distributed as Dm
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    u, i, r = planted(120, 90, density=0.08, seed=21)
    sel = np.arange(len(u)) % world == rank
    K = Dm.ShardedALS(u[sel], i[sel], r[sel], device="cpu", kernels=OracleKernels(), chunks=1)
    Dm.MAX_COLLECTIVE_BYTES = 256  # one chunk's factor all-gather is larger than this
    msg = ""
    try:
        K.fit(8, 1, 0.1, seed=1)
    except RuntimeError as e:
        msg = str(e)
    np.save(os.path.join(out_dir, f"guard_{rank}.npy"), np.array([float("MAX_COLLECTIVE" in msg)]))
    dist.destroy_process_group()


def test_collective_size_guard_refuses_oversized_calls(tmp_path):
    """Every collective is checked against MAX_COLLECTIVE_BYTES before it is issued;
    an oversized all-gather (one chunk, forced) raises on every rank instead of
    reaching the transport."""
    mp.spawn(_guard_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for w in range(2):
        assert np.load(tmp_path / f"guard_{w}.npy")[0] == 1.0


def test_pipeline_choice_follows_the_exchange_model():
    """pipeline="auto" pipelines the item half-sweep only where the hidden all-gather
    outweighs the partial-slot traffic plus the extra Y prep, at the
    fit's rank and task length: the weak-scaled configs[1] shape on 8 ranks (2 chunks,
    8 x 162,541 users, 59,047 items: ~7.4k item rows of ~3.4k ratings per rank, rank
    64) — yes; configs[3] on 8 ranks (6 chunks, 10M users, 125k items of ~8k ratings
    per rank, rank-128 slots, 16384-rating tasks) — no; one rank or one chunk — never."""
    from als_mi355x.distributed import ShardedALS, PAD_CAP
    import math
    rpc1 = math.ceil(PAD_CAP * 8 * 162541 / (8 * 2))
    assert ShardedALS.pipeline_pays(8, 2, rpc1, 59047 // 8, 8 * 25_000_095 // 8, rank=64)
    c1 = ShardedALS.pipeline_cost(8, 2, rpc1, 59047 // 8, 8 * 25_000_095 // 8, rank=64)
    assert 0 < c1["added_s"] < 0.5 * c1["hidden_s"]
    # the prep over the arrived prefix of U is part of what the pipeline adds
    c1b = ShardedALS.pipeline_cost(8, 4, rpc1 // 2, 59047 // 8, 8 * 25_000_095 // 8, rank=64)
    assert c1b["added_s"] > c1["added_s"]
    rpc3 = math.ceil(PAD_CAP * 10_000_000 / (8 * 6))
    assert not ShardedALS.pipeline_pays(8, 6, rpc3, 1_000_000 // 8, 10 ** 9 // 8, rank=128,
                                        chunk=16384)
    # the model follows the rank: a rank-16 fit's slots are far smaller
    assert ShardedALS.pipeline_cost(8, 6, rpc3, 1_000_000 // 8, 10 ** 9 // 8, rank=16)[
        "added_s"] < ShardedALS.pipeline_cost(8, 6, rpc3, 1_000_000 // 8, 10 ** 9 // 8,
                                              rank=128)["added_s"]
    assert not ShardedALS.pipeline_pays(1, 4, rpc1, 59047, 25_000_095)
    assert not ShardedALS.pipeline_pays(8, 1, rpc1, 59047 // 8, 25_000_095)


def test_constructor_argument_checks():
    from als_mi355x.distributed import ShardedALS
    with pytest.raises(ValueError, match="exchange"):
        ShardedALS.__init__(object.__new__(ShardedALS), [0], [0], [1.0], exchange="tree")
    with pytest.raises(ValueError, match="pipeline"):
        ShardedALS.__init__(object.__new__(ShardedALS), [0], [0], [1.0], pipeline="yes")
