"""Device-resident ALS engine (one process per GPU).

This is the host side of the hot path that replaces Spark's
``ml.recommendation.ALS.train`` (upstream) as reached from
RecommenderSystem.py:148-149 / :163 / :218, and ``predictAll`` +
``computeError`` (RecommenderSystem.py:103-129, :150, :165, :222, :232).
Every arithmetic step runs in libals_hip.so (HIP, gfx950); torch supplies
device memory, streams and the RNG for the initial factors only.

Data layout in HBM (DESIGN.md "Data layout"):
  users/items id maps  int32[id_space]   (id -> dense row or -1)
  user side  CSR       row_ptr int64[n_u+1], col int32[nnz] (dense item), val f32[nnz]
  item side  CSR       row_ptr int64[n_i+1], col int32[nnz] (dense user), val f32[nnz]
  factors              U f32[n_u, ld], V f32[n_i, ld], ld = roundup(rank, 4), pad cols 0
  schedule per side    light rows (LPT order), heavy rows, chunk tasks
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import filters as _filters
from ._lib import check, ptr, stream_ptr  # noqa: F401 (re-exported, as the bindings below)
# every binding stays reachable as engine.NAME: bench.py, the tests and tools/ go through here
from .kernels.workspace import ld_for, Workspace, _to_device, k_pad, raise_status, _host_f64
from .kernels.csr import (
    IdIndex, MAX_ID_SPACE, id_offset, build_index, build_csr, csr_merge_tile, merge_csr,
    grow_index, csr_remove_tile, remove_mark, remove_compact, shrink_index, _delete_csr,
    gather_rows, group_pairs,
)
from .kernels.schedule import (
    DEFAULT_CHUNK, chunk_for, DUAL_MAX_RATINGS, DUAL_MAX_RATINGS_64, dual_limit, RatingBlock,
    build_block, schedule_block,
)
from .kernels.solve import (
    MAX_RANK, PHASE_LAUNCH1, PHASE_LAUNCH2, PHASE_PREP, PHASE_RSCALE, PHASE_DUAL, PHASE_RESCUE,
    PHASE_ALL, compute_yty, solve_half, SplitSchedule, _segment_tasks, split_schedule,
    solve_half_split,
)
from .kernels.rows import fold_in_rows, nnls_rows, EXPLAIN_MAX_TOP, explain_rows
from .kernels.predict import (
    predict_pairs, rmse_pairs, MOMENT_NAMES, regression_moments_pairs, regression_moments_cols,
    regression_dict,
)
from .kernels.topk import (
    ids_of, topk_rows, topk_rows_filtered, SIMILAR_MAX_TOP, SIMILAR_MAX_SLICES,
    SIMILAR_SWEEP_MIN_ROWS, similar_rows, unit_rows, similar_rows_unit, DIVERSIFY_MAX_POOL,
    DIVERSIFY_POOL_BYTES, _check_lists, diversify_rows, list_similarity_rows,
)
from .kernels.ranking import (
    LIST_MAX_AT, LIST_METRIC_FIELDS, _list_rows_args, list_exposure_window, list_exposure_rows,
    list_concentration, list_novelty_rows, long_tail_bits, list_metrics_dict, list_metrics_rows,
    MAX_RANK_AT, rank_metrics_rows, rank_metrics_dict, FULL_RANK_SUMS, rank_positions_table,
    rank_positions_rows, full_rank_sums_rows, full_rank_dict,
)
from .kernels.objective import OBJECTIVE_SIDE, objective_span, objective_side, gram_dot
from .kernels.stats import (
    RATING_MOMENTS, BASELINE_METHODS, rating_stats_task, rating_stats_group_rows, row_moments,
    bias_update, baseline_predict_rows, rating_stats_dict, Baseline,
)
from .kernels.split import (
    SPLIT_MODES, split_row_cap, split_anchor, split_eligible, split_thresholds, split_mark,
    check_split_args, split_windows,
)
from .kernels.co_rated import (
    CO_RATED_MEASURES, CO_RATED_MAX_TOP, CO_RATED_PASS, CO_RATED_MAX_PASS, co_rated_task,
    co_rated_window, co_rated_rows,
)


def make_engine(users, items, ratings, device=None):
    """The engine behind ALS.fit / ALS.train: one GPU (ALSCore), or — when this process
    is one rank of an initialised torch.distributed group of world size > 1 —
    the sharded engine (distributed.ShardedALS), fed with this rank's partition
    of the ratings (the role of a Spark DataFrame partition)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        from .distributed import ShardedALS
        return ShardedALS(users, items, ratings, device=device)
    return ALSCore(users, items, ratings, device=device)


class ALSCore:
    """Ratings, id maps, both CSR sides and both factor matrices resident on one GPU."""

    def __init__(self, users, items, ratings, device=None, chunk: Optional[int] = None):
        """chunk: ratings per heavy-row task; None = chunk_for(rank, implicit) of each
        half-sweep (the blocks are rescheduled when a fit asks for another length)."""
        _lib.require_gpu()
        self._auto_chunk = chunk is None
        chunk = DEFAULT_CHUNK if chunk is None else chunk
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda", torch.cuda.current_device())
        # both CSR sides hold the same ratings: one rating scale for every half-sweep
        self.ws = Workspace(self.device, shared_rating_scale=True)
        # computeYtY's task slots in a buffer of their own: written over the solve
        # workspace they would clobber its rating scale word, re-measured every half-sweep
        self.ws_yty = Workspace(self.device)
        u, i, r = self._triples(users, items, ratings)
        if u.numel() == 0:
            raise ValueError("ALS needs at least one rating")
        umin, umax = int(u.min()), int(u.max())
        imin, imax = int(i.min()), int(i.max())
        uoff, ioff = id_offset(umin, umax), id_offset(imin, imax)
        if uoff:
            u = (u.long() - uoff).to(torch.int32)
        if ioff:
            i = (i.long() - ioff).to(torch.int32)
        self.nnz = int(u.numel())
        self.uidx = build_index(u, umax - uoff + 1, self.ws)
        self.iidx = build_index(i, imax - ioff + 1, self.ws)
        self.uidx.offset, self.iidx.offset = uoff, ioff
        self.user_block = build_block(u, self.uidx, i, self.iidx, r, self.ws, chunk)
        self.item_block = build_block(i, self.iidx, u, self.uidx, r, self.ws, chunk)
        self._blank_state()

    def _blank_state(self) -> None:
        """What a core holds before its first fit, whichever way it was built."""
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._train_ex = {}  # user_side -> sorted training exclusion list (train_exclusion)
        self._fit_params = None  # reg / implicit / alpha / nonnegative of the last fit
        self._touched = None     # (user rows, item rows) that took ratings since the last fit
        self.objective_history = []   # (iteration, objective) pairs of the last fit (K10)
        self.iterations_run = 0       # where the last fit stopped
        self.U: Optional[torch.Tensor] = None
        self.V: Optional[torch.Tensor] = None
        self.rank = 0
        # buffers of their own, made on first use: the solve workspace keeps its rating scale
        self.ws_nnls = self.ws_obj = self.ws_rows = None

    @classmethod
    def from_factors(cls, user_ids, U, item_ids, V, device=None) -> "ALSCore":
        """A serving-only core (no ratings, cannot fit) from saved factors: ids ascending,
        U/V host or device arrays [n, rank].  predict / rmse / top-k run as after fit()."""
        _lib.require_gpu()
        self = cls.__new__(cls)
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda", torch.cuda.current_device())
        self.ws = Workspace(self.device)
        self.ws_yty = self.ws
        self.nnz = 0
        self._auto_chunk = False
        self.user_block = self.item_block = None
        self._blank_state()
        U = _to_device(U, torch.float32, self.device)
        V = _to_device(V, torch.float32, self.device)
        rank = int(U.shape[1])
        if V.shape[1] != rank or not (1 <= rank <= MAX_RANK):
            raise ValueError(f"factor ranks {U.shape[1]}/{V.shape[1]} invalid (max {MAX_RANK})")
        idx = []
        for ids, F in ((user_ids, U), (item_ids, V)):
            ids = _to_device(ids, torch.int32, self.device)
            if ids.numel() != F.shape[0] or ids.numel() == 0:
                raise ValueError("factor ids must be non-empty and match the rows")
            if ids.numel() > 1 and not bool((ids[1:] > ids[:-1]).all()):
                raise ValueError("factor ids must be strictly ascending")
            off = id_offset(int(ids.min()), int(ids.max()))
            key = (ids.long() - off)
            mp = torch.full((int(key.max()) + 1,), -1, dtype=torch.int32, device=self.device)
            mp[key] = torch.arange(ids.numel(), dtype=torch.int32, device=self.device)
            idx.append(IdIndex(mp, key.to(torch.int32), int(ids.numel()), off))
        self.uidx, self.iidx = idx
        self.rank = rank
        ld = ld_for(rank)
        self.U = torch.zeros((U.shape[0], ld), dtype=torch.float32, device=self.device)
        self.V = torch.zeros((V.shape[0], ld), dtype=torch.float32, device=self.device)
        self.U[:, :rank] = U
        self.V[:, :rank] = V
        return self

    @property
    def n_users(self) -> int:
        return self.uidx.n

    @property
    def n_items(self) -> int:
        return self.iidx.n

    # ---- checks and conversions the public methods share ----
    def _need_ratings(self, who: str) -> None:
        if self.user_block is None:
            raise ValueError(f"{who} needs the ratings the model was fitted on; this core "
                             "was built from saved factors (from_factors / load) and has none")

    def _need_factors(self, who: str) -> None:
        if self.U is None or self.V is None:
            raise ValueError(f"{who} needs factors: fit() the core or build it from_factors")

    def _pairs(self, users, items):
        """users, items as int32 device vectors of one length."""
        u = _to_device(users, torch.int32, self.device)
        i = _to_device(items, torch.int32, self.device)
        if u.numel() != i.numel():
            raise ValueError("users and items must have the same length")
        return u, i

    def _triples(self, users, items, ratings):
        """users, items (int32) and ratings (f32) as device vectors of one length."""
        u = _to_device(users, torch.int32, self.device)
        i = _to_device(items, torch.int32, self.device)
        r = _to_device(ratings, torch.float32, self.device)
        if not (u.numel() == i.numel() == r.numel()):
            raise ValueError("users, items and ratings must have the same length")
        return u, i, r

    def _known_rows(self, idx: IdIndex, ids):
        """(keys int32, dense rows int64) of the distinct ids `idx` knows, ascending."""
        keys = torch.unique(_to_device(ids, torch.int32, self.device))
        rows = idx.rows_of(keys)
        known = rows >= 0
        return keys[known], rows[known]

    def _allow_bits(self, idx: IdIndex, candidates):
        """The allow mask of the rows of `idx` named by `candidates` (ids; unknown ones
        dropped), None for no restriction."""
        if candidates is None:
            return None
        c = _to_device(candidates, torch.int32, self.device)
        return _filters.pack_allow_bits(idx.rows_of(c), idx.n)

    def _empty_lists(self, m: int, t: int):
        """The (ids int32, scores f32) pair of m lists with t slots, unfilled."""
        return (torch.empty((m, t), dtype=torch.int32, device=self.device),
                torch.empty((m, t), dtype=torch.float32, device=self.device))

    # Spark ALS.initialize: unit-norm Gaussian rows, fp32.
    def init_factors(self, rank: int, seed: int = 0, U0=None) -> None:
        if rank < 1 or rank > MAX_RANK:
            raise ValueError(f"rank must be in [1, {MAX_RANK}] on this build, got {rank}")
        self.rank = rank
        ld = ld_for(rank)
        self.U = torch.zeros((self.n_users, ld), dtype=torch.float32, device=self.device)
        self.V = torch.zeros((self.n_items, ld), dtype=torch.float32, device=self.device)
        if U0 is not None:
            U0 = _to_device(U0, torch.float32, self.device)
            if tuple(U0.shape) != (self.n_users, rank):
                raise ValueError(f"U0 must have shape {(self.n_users, rank)}")
            self.U[:, :rank] = U0
        else:
            g = torch.Generator(device=self.device)
            g.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
            x = torch.randn((self.n_users, rank), generator=g, device=self.device,
                            dtype=torch.float32)
            self.U[:, :rank] = x / torch.linalg.vector_norm(x, dim=1, keepdim=True)

    def schedule_for(self, implicit: bool) -> None:
        """The default heavy-row task length for this fit's rank and feedback type (no-op
        when the core was built with an explicit chunk)."""
        if self._auto_chunk:
            self.rechunk(chunk_for(self.rank, implicit))

    def rechunk(self, chunk: int) -> None:
        """Reschedule both sides for `chunk`-rating heavy-row tasks (same CSR)."""
        for name in ("user_block", "item_block"):
            b = getattr(self, name)
            if b.chunk != chunk:
                setattr(self, name, schedule_block(b.n_rows, b.nnz, b.row_ptr, b.col, b.val,
                                                   self.ws, chunk))

    def _half_sweep_nnls(self, block, Y, n_src, X, reg, implicit, alpha):
        """One computeFactors pass with Spark's NNLSSolver (K13); a buffer of its own, so the
        solve workspace keeps its rating scale."""
        if self.ws_nnls is None:
            self.ws_nnls = Workspace(self.device)
        yty = compute_yty(Y, n_src, self.rank, self.ws_yty) if implicit else None
        nnls_rows(block.row_ptr, block.col, block.val, Y, n_src, self.rank, reg, implicit, alpha,
                  yty, self.ws_nnls, DEFAULT_CHUNK, X=X)

    def half_sweep_items(self, reg, implicit=False, alpha=1.0, nonnegative=False):
        if nonnegative:
            return self._half_sweep_nnls(self.item_block, self.U, self.n_users, self.V, reg,
                                         implicit, alpha)
        self.schedule_for(implicit)
        yty = compute_yty(self.U, self.n_users, self.rank, self.ws_yty) if implicit else None
        solve_half(self.item_block, self.U, self.V, self.rank, reg, implicit, alpha, yty,
                   self.status, self.ws)

    def half_sweep_users(self, reg, implicit=False, alpha=1.0, nonnegative=False):
        if nonnegative:
            return self._half_sweep_nnls(self.user_block, self.V, self.n_items, self.U, reg,
                                         implicit, alpha)
        self.schedule_for(implicit)
        yty = compute_yty(self.V, self.n_items, self.rank, self.ws_yty) if implicit else None
        solve_half(self.user_block, self.V, self.U, self.rank, reg, implicit, alpha, yty,
                   self.status, self.ws)

    def iterate(self, reg, implicit=False, alpha=1.0, nonnegative=False):
        """One ALS iteration in Spark's order: items from users, then users from items.
        nonnegative: every row is solved under x >= 0 (K13, Spark's NNLSSolver)."""
        if nonnegative:
            self.half_sweep_items(reg, implicit, alpha, nonnegative=True)
            self.half_sweep_users(reg, implicit, alpha, nonnegative=True)
            return
        self.half_sweep_items(reg, implicit, alpha)
        self.half_sweep_users(reg, implicit, alpha)

    def check_status(self) -> None:
        raise_status(int(self.status.item()))

    def objective(self, reg, implicit=False, alpha=1.0) -> dict:
        """The training objective of the current factors: the function each half-sweep
        minimises row by row (K10; Spark's lambda * numExplicits weighting, als_hip.h):
          explicit  sum_obs (r - s)^2 + reg (sum_u n_u |x_u|^2 + sum_i n_i |y_i|^2)
          implicit  sum_all c (p - s)^2 + reg (sum_u n+_u |x_u|^2 + sum_i n+_i |y_i|^2)
        in fp64 over the stored fp32 factors.  Returns {"objective", "data" (implicit: the
        all-pairs term, <U^T U, V^T V>_F plus the correction over the ratings), "reg"
        (times reg already), "scale" (the sum of the absolute values of everything added:
        the size rounding errors are relative to), "n", "n_positive"}.  Deterministic: two
        calls on the same factors return the same bits.  One host sync."""
        self._need_ratings("objective")
        if self.U is None or self.V is None:
            raise ValueError("objective needs factors: fit() the core or init_factors() first")
        if reg < 0 or alpha < 0:
            raise ValueError(f"reg and alpha must be >= 0, got {reg}, {alpha}")
        if self.ws_obj is None:
            # observing a fit must not make the solve workspace re-measure its rating scale
            self.ws_obj = Workspace(self.device)
        n = len(OBJECTIVE_SIDE)
        out = torch.zeros(2 * n + 1, dtype=torch.float64, device=self.device)
        objective_side(self.user_block, self.U, self.V, self.n_items, self.rank, implicit, alpha,
                       self.ws_obj, out[:n])
        objective_side(self.item_block, self.V, None, self.n_users, self.rank, implicit, alpha,
                       self.ws_obj, out[n:2 * n])
        if implicit:
            gram_dot(self.U, self.n_users, self.V, self.n_items, self.rank, self.ws_obj,
                     out=out[2 * n:])
        v = out.tolist()
        side_u, side_i, frob = dict(zip(OBJECTIVE_SIDE, v[:n])), dict(zip(OBJECTIVE_SIDE, v[n:])), v[2 * n]
        data = side_u["data"] + frob
        regv = float(reg) * (side_u["reg"] + side_i["reg"])
        return {"objective": data + regv, "data": data, "reg": regv,
                "scale": side_u["scale"] + abs(frob) + regv, "n": int(side_u["n"]),
                "n_positive": int(side_u["n_positive"])}

    def fit(self, rank, max_iter, reg, implicit=False, alpha=1.0, seed=0, U0=None,
            checkpoint_dir=None, checkpoint_interval=10, resume=False, objective_every=0,
            tol=None, nonnegative=False):
        """max_iter ALS iterations from the seeded (or given U0) start.  checkpoint_dir:
        write U, V every checkpoint_interval iterations (checkpoint.py); resume
        (True / "auto"): continue from the checkpoint there at its iteration.
        objective_every = m > 0: evaluate objective() after iterations m, 2m, ... and after
        the last one, into self.objective_history as (iteration, value) pairs (a resumed fit
        starts its list at the first evaluated iteration after the checkpoint).  tol: stop
        after an evaluated iteration whose decrease L_prev - L_cur <= tol * L_prev (tol
        alone evaluates every iteration); a checkpoint due at that iteration is still
        written.  self.iterations_run is where the fit stopped.  With both off (the default)
        nothing is evaluated and no host sync is added.
        nonnegative: Spark's `nonnegative=true` — the same seeded signed start, then every
        half-sweep solves its rows under x >= 0 (K13), so all factors are >= 0 from the first
        one on; objective_every / tol evaluate the same objective.  Not with checkpoint_dir:
        a checkpoint does not record the solver, and resuming a Cholesky fit as NNLS (or
        the reverse) must not happen silently."""
        from . import checkpoint as C
        nonnegative = bool(nonnegative)
        if nonnegative and checkpoint_dir:
            raise ValueError("nonnegative=True cannot be combined with checkpoint_dir: a "
                             "checkpoint does not record the solver")
        every = int(objective_every)
        if every < 0:
            raise ValueError(f"objective_every must be >= 0, got {objective_every}")
        if tol is not None:
            tol = float(tol)
            if not tol >= 0:
                raise ValueError(f"tol must be >= 0, got {tol}")
            every = every or 1
        init = C.init_key(seed, U0) if checkpoint_dir else None
        start, Uc, Vc = C.resume_point(checkpoint_dir, resume, self, rank, reg, implicit, alpha,
                                       max_iter, init)
        self.init_factors(rank, seed, Uc if Uc is not None else U0)
        if Vc is not None:
            self.V[:, :rank] = _to_device(Vc, torch.float32, self.device)
        self.status.zero_()
        self._fit_params = {"reg": float(reg), "implicit": bool(implicit), "alpha": float(alpha),
                            "nonnegative": nonnegative}
        self._touched = None   # a fit re-solves every row
        self.objective_history = []
        self.iterations_run = start
        prev = None
        for it in range(start, max_iter):
            if nonnegative:
                self.iterate(reg, implicit, alpha, nonnegative=True)
            else:
                self.iterate(reg, implicit, alpha)
            stop = False
            if every and ((it + 1) % every == 0 or it + 1 == max_iter):
                cur = self.objective(reg, implicit, alpha)["objective"]
                self.objective_history.append((it + 1, cur))
                stop = tol is not None and prev is not None and prev - cur <= tol * prev
                prev = cur
            C.maybe_save(checkpoint_dir, checkpoint_interval, it + 1, self, rank, reg, implicit,
                         alpha, init=init)
            self.iterations_run = it + 1
            if stop:
                break
        self.check_status()
        return self

    # ---- K17: ratings that arrive after the fit ----
    def _solve_rows(self, csr, rows, Y, n_src, p, yty_of=None):
        """(X f32 [m, ld], n_used int32 [m]) of the dense rows `rows` of the CSR (row_ptr,
        col, val), each from its full rating list in stored order against the fixed factors
        Y: K7, or K13 when the fit was nonnegative.  yty_of: (table, rows) the implicit YtY
        is taken of, None = Y.  Raises, before anything is stored, for a row that is not
        positive definite."""
        row_ptr, col, val = gather_rows(*csr, rows)
        yty = compute_yty(*(yty_of or (Y, n_src)), self.rank, self.ws_yty) if p["implicit"] else None
        if p["nonnegative"]:
            if self.ws_nnls is None:
                self.ws_nnls = Workspace(self.device)
            X, n_used, _ = nnls_rows(row_ptr, col, val, Y, n_src, self.rank, p["reg"],
                                     p["implicit"], p["alpha"], yty, self.ws_nnls)
            return X, n_used
        if self.ws_rows is None:
            self.ws_rows = Workspace(self.device)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        X, n_used = fold_in_rows(row_ptr, col, val, Y, n_src, self.rank, p["reg"], p["implicit"],
                                 p["alpha"], yty, status, self.ws_rows)
        raise_status(int(status.item()), " of the rows being re-solved (ascending dense row)")
        return X, n_used

    def _update_params(self, reg=None, implicit=None, alpha=None, nonnegative=None) -> dict:
        p = dict(self._fit_params or {})
        for k, v in (("reg", reg), ("implicit", implicit), ("alpha", alpha),
                     ("nonnegative", nonnegative)):
            if v is not None:
                p[k] = v
        if "reg" not in p:
            raise ValueError("no fit to take reg / implicit / alpha / nonnegative from: fit() "
                             "the core first, or pass reg=")
        p = {"reg": float(p["reg"]), "implicit": bool(p.get("implicit", False)),
             "alpha": float(p.get("alpha", 1.0)), "nonnegative": bool(p.get("nonnegative", False))}
        if p["reg"] < 0 or p["alpha"] < 0:
            raise ValueError(f"reg and alpha must be >= 0, got {p['reg']}, {p['alpha']}")
        return p

    def add_ratings(self, users, items, ratings, *, seed=0) -> dict:
        """Add a batch of ratings to the core in place (the reference adds a new user's
        twelve ratings to the training set and fits again, RecommenderSystem.py:207-247).
        users / items / ratings: host or device arrays of one length; new ids on either side
        are welcome, and a pair that is already rated (or twice in the batch) is one more
        rating, as Spark keeps duplicates.  After the call every rating-derived thing — both
        id maps, both CSR sides and their schedules, nnz — is what ALSCore(concat(old,
        batch)) would hold, bit for bit:
          a. both id maps grow (als_index_build over the old ids plus the batch's; a new id
             below the offset, or a negative one, re-bases the map)
          b. K1 builds the batch's two small CSRs against the grown maps
          c. K17 (als_csr_merge) writes each side's merged CSR in one pass with no sort, and
             the side is scheduled again at its current chunk
          d. on a core with factors, the rows of U and V move to their new places bit for
             bit and every NEW row gets factors: new users from their ratings against the
             current V (K7, or K13 after a nonnegative fit; the parameters of the last fit;
             a rating of an item that is new as well is left out, as fold_in leaves out an
             unknown item), then new items against the grown U.  A new row without a used
             rating — a new user who rated only new items — gets a unit-norm Gaussian row
             from `seed`, as init_factors gives: a zero row would stay zero through every
             later sweep.  Rows that existed keep their factors until refresh() or refit()
          e. everything cached from the ratings (the train exclusion lists, the workspace's
             rating scale) is dropped.
        Needs one transient second copy of each side's col and val (8 B per rating and
        side, until the call returns).  An empty batch is a no-op; before any fit only the ratings are
        merged.  Nothing is changed when the call raises.
        Returns {"added", "new_users", "new_items" (ids, ascending), "touched_users",
        "touched_items" (int64 dense rows in the grown maps, ascending: the rows whose
        rating lists changed)}; the touched rows of every add since the last fit are kept
        for refresh()."""
        self._need_ratings("add_ratings")
        u, i, r = self._triples(users, items, ratings)
        empty = torch.empty(0, dtype=torch.int64, device=self.device)
        if u.numel() == 0:
            return {"added": 0, "new_users": empty.to(torch.int32), "new_items":
                    empty.to(torch.int32), "touched_users": empty, "touched_items": empty}
        return self._add_commit(self._add_compute(u, i, r, seed))

    def _add_compute(self, u, i, r, seed, user_csr=None, item_csr=None, nnz=None) -> dict:
        """add_ratings steps a-d on device arrays, storing nothing: the grown state of the
        core's id maps and of the two CSR sides (the core's own blocks, or the (row_ptr, col,
        val) triples given, which hold `nnz` ratings and may have empty rows: set_ratings
        passes the sides it has just compacted)."""
        ub, ib = self.user_block, self.item_block
        user_csr = user_csr or (ub.row_ptr, ub.col, ub.val)
        item_csr = item_csr or (ib.row_ptr, ib.col, ib.val)
        uidx, umap, new_u = grow_index(self.uidx, u, self.ws)
        iidx, imap, new_i = grow_index(self.iidx, i, self.ws)
        uk, ik = uidx.keys(u), iidx.keys(i)
        add_u = build_csr(uk, uidx, ik, iidx, r, self.ws)
        user_csr = merge_csr(*user_csr, ib.n_rows, umap, imap, *add_u)
        add_i = build_csr(ik, iidx, uk, uidx, r, self.ws)
        item_csr = merge_csr(*item_csr, ub.n_rows, imap, umap, *add_i)
        nnz = (self.nnz if nnz is None else int(nnz)) + int(u.numel())
        touched_u = (add_u[0][1:] > add_u[0][:-1]).nonzero().flatten()
        touched_i = (add_i[0][1:] > add_i[0][:-1]).nonzero().flatten()
        U = V = None
        if self.rank > 0 and self.U is not None:
            U, V = self._grown_factors(uidx.n, iidx.n, umap, imap, new_u, new_i, user_csr,
                                       item_csr, int(seed))
        return dict(added=int(u.numel()), uidx=uidx, iidx=iidx, umap=umap, imap=imap,
                    new_u=new_u, new_i=new_i, user_csr=user_csr, item_csr=item_csr, nnz=nnz,
                    touched_u=touched_u, touched_i=touched_i, U=U, V=V)

    def _add_commit(self, st: dict) -> dict:
        """Store what _add_compute made and return add_ratings' report: nothing before this
        touched the core, and from here on it cannot fail half-way."""
        uidx, iidx, umap, imap, nnz = st["uidx"], st["iidx"], st["umap"], st["imap"], st["nnz"]
        new_u, new_i, touched_u, touched_i = (st[k] for k in ("new_u", "new_i", "touched_u",
                                                              "touched_i"))
        U, V = st["U"], st["V"]
        ub, ib = self.user_block, self.item_block
        self.user_block = schedule_block(uidx.n, nnz, *st["user_csr"], self.ws, ub.chunk)
        self.item_block = schedule_block(iidx.n, nnz, *st["item_csr"], self.ws, ib.chunk)
        self.uidx, self.iidx, self.nnz = uidx, iidx, nnz
        if U is not None:
            self.U, self.V = U, V
        self._train_ex = {}
        self.ws.rating_scale_key = None   # the batch may hold the largest |rating|
        self._retouch((umap, imap), (touched_u, touched_i))
        return {"added": st["added"], "new_users": uidx.ids()[new_u], "new_items":
                iidx.ids()[new_i], "touched_users": touched_u, "touched_items": touched_i}

    def _retouch(self, maps, new_touched) -> None:
        """The rows refresh() owes a re-solve after the id maps moved: the (user, item) rows
        touched earlier, renumbered through `maps` (int32 old row -> new row, -1 = the row
        left and is dropped, None = this side's numbering is unchanged), united with
        `new_touched` (ascending int64 rows in the new numbering)."""
        if self._touched is None:
            self._touched = tuple(new_touched)
            return
        touched = []
        for mp, earlier, new in zip(maps, self._touched, new_touched):
            if mp is not None:
                earlier = mp[earlier].long()
                earlier = earlier[earlier >= 0]
            touched.append(torch.unique(torch.cat([earlier, new])))
        self._touched = tuple(touched)

    def _grown_factors(self, n_u, n_i, umap, imap, new_u, new_i, user_csr, item_csr, seed):
        """add_ratings step d: (U, V) for the grown id maps."""
        ld = ld_for(self.rank)

        def moved(F, n, mp):
            if mp is None:
                return F.clone()
            out = torch.zeros((n, ld), dtype=torch.float32, device=self.device)
            out[mp.long()] = F
            return out

        U, V = moved(self.U, n_u, umap), moved(self.V, n_i, imap)
        p = self._update_params() if self._fit_params else None
        g = torch.Generator(device=self.device)
        g.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)

        def fill(F, rows, csr, Y, n_src, unknown_cols, yty_of=None):
            if rows.numel() == 0:
                return
            X = torch.zeros((rows.numel(), ld), dtype=torch.float32, device=self.device)
            n_used = torch.zeros(rows.numel(), dtype=torch.int32, device=self.device)
            if p is not None:
                row_ptr, col, val = csr
                if unknown_cols.numel():   # a column that has no factors yet is not used
                    hide = torch.zeros(n_src, dtype=torch.bool, device=self.device)
                    hide[unknown_cols] = True
                    col = torch.where(hide[col.long()], -1, col).to(torch.int32)
                X, n_used = self._solve_rows((row_ptr, col, val), rows, Y, n_src, p, yty_of)
            blank = (n_used == 0).nonzero().flatten()
            if blank.numel():
                x = torch.randn((blank.numel(), self.rank), generator=g, device=self.device,
                                dtype=torch.float32)
                X[blank] = 0
                X[blank, :self.rank] = x / torch.linalg.vector_norm(x, dim=1, keepdim=True)
            F[rows] = X

        # YtY of the V the model had: the rows just added are zero and add nothing, and the
        # sum keeps the bits fold_in would have used before the growth
        fill(U, new_u, user_csr, V, n_i, new_i, (self.V, self.n_items))
        fill(V, new_i, item_csr, U, n_u, new_u[:0])
        return U, V

    def refresh(self, *, reg=None, implicit=None, alpha=None, nonnegative=None, sweeps=1):
        """Re-solve only the rows add_ratings touched since the last fit — the "serve it
        now" path between add_ratings and the next refit: touched users against V, then
        touched items against the new U, `sweeps` times, each row from its full merged rating
        list in block order (K7 als_fold_in, or K13 als_nnls_rows when nonnegative; YtY of
        the fixed side when implicit).  Every other row keeps its bits.  reg / implicit /
        alpha / nonnegative default to those of the last fit.  One workgroup per row in
        fp64, so it pays for a handful of rows only: on the ML-25M shape at rank 64 one new
        user's 12 ratings (1 + 12 rows) take 1.0 ms, 0.6 of a full iteration, but a batch of
        10^4 ratings (19 thousand rows) 12.6 ms, 7.5 iterations — there refit(1) is the
        cheaper call.  Returns self."""
        self._need_ratings("refresh")
        if self.U is None or self.V is None:
            raise ValueError("refresh needs factors: fit() the core first")
        p = self._update_params(reg, implicit, alpha, nonnegative)
        if int(sweeps) < 1:
            raise ValueError(f"sweeps must be >= 1, got {sweeps}")
        if self._touched is None:
            return self
        tu, ti = self._touched
        for _ in range(int(sweeps)):
            if tu.numel():
                b = self.user_block
                X, _ = self._solve_rows((b.row_ptr, b.col, b.val), tu, self.V, self.n_items, p)
                self.U[tu] = X
            if ti.numel():
                b = self.item_block
                X, _ = self._solve_rows((b.row_ptr, b.col, b.val), ti, self.U, self.n_users, p)
                self.V[ti] = X
        return self

    def refit(self, max_iter, **fit_kwargs):
        """The warm start: fit(rank, max_iter, ..., U0=the current U) with the parameters of
        the last fit (fit_kwargs override them and pass objective_every / tol through).
        Spark's order solves the items first from U alone and never reads V, so continuing
        from the current U is continuing the fit."""
        self._need_ratings("refit")
        if self.U is None or self.rank < 1:
            raise ValueError("refit needs factors: fit() the core first")
        if "U0" in fit_kwargs or "rank" in fit_kwargs:
            raise ValueError("refit starts from the current U at the current rank")
        kw = self._update_params(*(fit_kwargs.pop(k, None) for k in
                                   ("reg", "implicit", "alpha", "nonnegative")))
        kw.update(fit_kwargs)
        return self.fit(self.rank, int(max_iter), U0=self.U[:, :self.rank].clone(), **kw)

    # ---- K18: ratings that are taken back after the fit ----
    def _listed_pairs(self, users, items, who: str):
        """The distinct (user, item) pairs of a batch: (u int32, i int32, ur, ir int64 dense
        rows, -1 = unknown)."""
        self._need_ratings(who)
        u, i = self._pairs(users, items)
        if u.numel():
            key = torch.unique((u.long() << 32) | (i.long() & 0xFFFFFFFF))
            low = key & 0xFFFFFFFF
            u = (key >> 32).to(torch.int32)
            i = torch.where(low >= (1 << 31), low - (1 << 32), low).to(torch.int32)
        return u, i, self.uidx.rows_of(u), self.iidx.rows_of(i)

    def _mark_removed(self, ur, ir, who: str):
        """Both sides' K18 mark pass for the distinct stored-id pairs (ur, ir) (int64 dense
        rows).  Returns (user marks, item marks, stored copies dropped per pair in (ur, ir)
        order of the user side's sort, the ratings that stay)."""
        n_u, n_i = self.n_users, self.n_items
        ub, ib = self.user_block, self.item_block
        ku = torch.sort(ur * n_i + ir).values            # by user row, then item row
        ki = torch.sort(ir * n_u + ur).values            # by item row, then user row
        del_u = _delete_csr(ku // n_i, ku % n_i, n_u)
        del_i = _delete_csr(ki // n_u, ki % n_u, n_i)
        mu = remove_mark(ub.row_ptr, ub.col, *del_u, self.ws, count_hits=True)
        mi = remove_mark(ib.row_ptr, ib.col, *del_i, self.ws)
        nnz = int(mu[1][-1])
        if nnz != int(mi[1][-1]):
            raise RuntimeError(f"{who}: the two sides disagree on what stays")
        return mu, mi, mu[3], nnz

    def _kept_state(self, mu, mi, nnz, blocks_only: bool = False) -> dict:
        """remove_ratings steps c and d for the two sides' K18-format marks (keep_bits,
        tile_off, row_ptr_kept, ...) that keep `nnz` ratings, storing nothing: the shrunk id
        maps, the compacted CSR sides and the moved factor rows.  blocks_only: neither the
        factor rows nor the touched rows are made (split's new core has no use for them)."""
        ub, ib = self.user_block, self.item_block
        side = []
        for block, idx, marks in ((ub, self.uidx, mu), (ib, self.iidx, mi)):
            kept = marks[2][1:] - marks[2][:-1]
            had = block.row_ptr[1:] - block.row_ptr[:-1]
            left = (kept == 0).nonzero().flatten()
            shrunk, mp = shrink_index(idx, left, self.ws)
            touched = None
            if not blocks_only:
                changed = ((kept > 0) & (kept < had)).nonzero().flatten()
                touched = changed if mp is None else mp[changed].long()
            side.append(dict(idx=shrunk, map=mp, left=idx.ids()[left], kept=kept,
                             touched=touched))
        su, si = side
        csr = []
        for block, marks, me, other, n_cols in ((ub, mu, su, si, ib.n_rows),
                                                (ib, mi, si, su, ub.n_rows)):
            col, val = remove_compact(block.col, block.val, marks[0], marks[1], other["map"],
                                      n_cols, nnz)
            stays = torch.ones(block.n_rows + 1, dtype=torch.bool, device=self.device)
            stays[:-1] = me["kept"] > 0               # the last word is nnz
            csr.append((marks[2][stays].contiguous(), col, val))
        U = V = None
        if not blocks_only and self.rank > 0 and self.U is not None:
            U = self.U if su["map"] is None else self.U[su["kept"] > 0].contiguous()
            V = self.V if si["map"] is None else self.V[si["kept"] > 0].contiguous()
        return dict(su=su, si=si, csr=csr, U=U, V=V, nnz=nnz)

    def _kept_commit(self, st: dict) -> None:
        """Store what _kept_state made (remove_ratings steps d's scheduling and e): nothing
        before this touched the core, and from here on it cannot fail half-way."""
        su, si, csr, nnz = st["su"], st["si"], st["csr"], st["nnz"]
        ub, ib = self.user_block, self.item_block
        self.user_block = schedule_block(su["idx"].n, nnz, *csr[0], self.ws, ub.chunk)
        self.item_block = schedule_block(si["idx"].n, nnz, *csr[1], self.ws, ib.chunk)
        self.nnz = nnz
        self.uidx, self.iidx = su["idx"], si["idx"]
        if st["U"] is not None:
            self.U, self.V = st["U"], st["V"]
        self._train_ex = {}
        self.ws.rating_scale_key = None   # the largest |rating| may have left
        self._retouch((su["map"], si["map"]), (su["touched"], si["touched"]))

    def remove_ratings(self, users, items) -> dict:
        """Take ratings back from the core in place: every stored copy of every listed (user,
        item) pair goes (a pair listed twice is listed once).  After the call every
        rating-derived thing — both id maps, both CSR sides and their schedules, nnz — is what
        ALSCore(the training triples with those pairs filtered out, order kept) would hold,
        bit for bit:
          a. ids are mapped to dense rows; a pair with an unknown id is counted as missing
          b. K18's mark pass (als_csr_remove_mark) flags the stored entries of both sides
             that stay, against a small delete CSR per side with ascending columns, and
             gives the kept entries before every row; a listed pair that no stored entry
             matched is counted as missing as well
          c. a user or an item left without a rating leaves the model (an empty row would
             make Spark's lambda * n * I system singular): both id maps shrink
             (shrink_index: offset and id_space are derived again), the factor rows of the
             rows that stay move to their new places bit for bit
          d. K18's compact pass (als_csr_remove_compact) writes each side's kept entries in
             stored order, columns renumbered through the OTHER side's shrunk map; the row
             pointer is the kept count before every surviving row, and the side is scheduled
             again at its current chunk
          e. everything cached from the ratings (the train exclusion lists, the workspace's
             rating scale) is dropped.
        Rows that stay keep their factors until refresh() or refit(); the surviving rows whose
        rating lists changed join the rows refresh() re-solves, rows touched by earlier adds
        are renumbered, and those that left are dropped.  Needs one transient second copy of
        each side's col and val.  An empty batch is a no-op; a call that would remove every
        rating raises ValueError; nothing is changed when the call raises.
        Measured on the ML-25M shape (tools/remove_cost.py): 2.5 ms for
        12 pairs, 3.5 ms for 10^6, 2.9 ms for the busiest user and 3.7 ms for the most-rated
        item, against 7.9-8.4 ms for ALSCore(the filtered triples): 2.3 to 3.4 times cheaper.
        Returns {"removed" (stored ratings dropped), "missing" (distinct listed pairs that
        matched nothing), "left_users", "left_items" (ids, ascending), "touched_users",
        "touched_items" (int64 dense rows in the new numbering, ascending)}."""
        u, i, ur, ir = self._listed_pairs(users, items, "remove_ratings")
        empty = torch.empty(0, dtype=torch.int64, device=self.device)
        info = {"removed": 0, "missing": int(u.numel()), "left_users": empty.to(torch.int32),
                "left_items": empty.to(torch.int32), "touched_users": empty,
                "touched_items": empty}
        known = (ur >= 0) & (ir >= 0)
        if not bool(known.any()):
            return info
        mu, mi, hits, nnz = self._mark_removed(ur[known], ir[known], "remove_ratings")
        if nnz == self.nnz:
            return info
        if nnz == 0:
            raise ValueError("remove_ratings would remove every rating: a model needs one")
        st = self._kept_state(mu, mi, nnz)
        removed = self.nnz - nnz
        self._kept_commit(st)
        su, si = st["su"], st["si"]
        info.update(removed=removed,
                    missing=int(u.numel()) - int(known.sum()) + int((hits == 0).sum()),
                    left_users=su["left"], left_items=si["left"], touched_users=su["touched"],
                    touched_items=si["touched"])
        return info

    def _remove_rows(self, ids, user_side: bool, who: str) -> dict:
        self._need_ratings(who)
        ids = torch.unique(_to_device(ids, torch.int32, self.device))
        idx, block, other = ((self.uidx, self.user_block, self.iidx) if user_side else
                             (self.iidx, self.item_block, self.uidx))
        rows = idx.rows_of(ids)
        unknown = int((rows < 0).sum())
        rows = rows[rows >= 0]
        row_ptr, col, _ = gather_rows(block.row_ptr, block.col, block.val, rows)
        mine = torch.repeat_interleave(idx.ids()[rows], row_ptr[1:] - row_ptr[:-1])
        theirs = other.ids()[col.long()]
        info = self.remove_ratings(*((mine, theirs) if user_side else (theirs, mine)))
        info["missing"] += unknown
        return info

    def remove_users(self, ids) -> dict:
        """Forget users: remove_ratings of every rating of the listed user ids (their rows
        expanded into pairs on the device).  An unknown id is counted in "missing"; the
        users, and every item only they had rated, are in "left_users" / "left_items"."""
        return self._remove_rows(ids, True, "remove_users")

    def remove_items(self, ids) -> dict:
        """Withdraw items: remove_users for the other side."""
        return self._remove_rows(ids, False, "remove_items")

    def set_ratings(self, users, items, ratings, *, seed=0) -> dict:
        """Replace ratings: every stored copy of each listed pair goes, then the batch is
        added as add_ratings adds it; of a pair that is several times in the batch the LAST
        rating wins (the earlier ones are dropped, the order of the rest is kept).  The result
        is what ALSCore(the old triples without the listed pairs, then the de-duplicated
        batch) would hold, bit for bit.  A pair that is not stored, or whose ids are new, is
        simply added.  No row leaves on the way: every row that loses a rating gets one
        back, so a user whose only rating is replaced keeps the factor row and its bits (K18
        leaves such a row empty between the two steps, K17 takes empty rows).  The removed
        state and the added state are computed first and stored at the end: nothing is
        changed when the call raises.  Returns add_ratings' report for the de-duplicated
        batch plus "replaced", the stored ratings that went."""
        self._need_ratings("set_ratings")
        u, i, r = self._triples(users, items, ratings)
        if u.numel() == 0:
            return dict(self.add_ratings(u, i, r), replaced=0)
        key = (u.long() << 32) | (i.long() & 0xFFFFFFFF)
        uniq, inv = torch.unique(key, return_inverse=True)
        last = torch.full((uniq.numel(),), -1, dtype=torch.int64, device=self.device)
        last.scatter_reduce_(0, inv, torch.arange(key.numel(), device=self.device), "amax")
        pick = torch.sort(last).values                   # last occurrences, in batch order
        u, i, r = u[pick].contiguous(), i[pick].contiguous(), r[pick].contiguous()
        ur, ir = self.uidx.rows_of(u), self.iidx.rows_of(i)
        known = (ur >= 0) & (ir >= 0)
        ucsr = icsr = None
        nnz = self.nnz
        if bool(known.any()):
            mu, mi, _, nnz = self._mark_removed(ur[known], ir[known], "set_ratings")
            if nnz != self.nnz:   # rows stay where they are, empty or not: no map, no shrink
                ub, ib = self.user_block, self.item_block
                ucsr = (mu[2],) + remove_compact(ub.col, ub.val, mu[0], mu[1], None, ib.n_rows, nnz)
                icsr = (mi[2],) + remove_compact(ib.col, ib.val, mi[0], mi[1], None, ub.n_rows, nnz)
        replaced = self.nnz - nnz
        info = self._add_commit(self._add_compute(u, i, r, seed, ucsr, icsr, nnz))
        info["replaced"] = replaced
        return info

    # ---- K20: per-user holdout and stratified folds ----
    def _split_marks(self, count, fraction, fold, seed, min_keep, keep_items, user_side,
                     row_cap: int = 0):
        """K20's four calls: (user marks, item marks, the ratings that stay)."""
        mode, value = check_split_args(count, fraction, fold, min_keep)
        ub, ib = self.user_block, self.item_block
        uids, iids = self.uidx.ids().contiguous(), self.iidx.ids().contiguous()
        sel, oth = (ub, ib) if user_side else (ib, ub)
        sel_ids, oth_ids = (uids, iids) if user_side else (iids, uids)
        anchor = None
        if keep_items:
            anchor = split_anchor(oth.row_ptr, oth.col, sel.n_rows, oth_ids, sel_ids,
                                  not user_side, seed, self.ws)
        e = split_eligible(sel.row_ptr, sel.col, oth.n_rows, anchor)
        lo, hi = split_windows(e, mode, value, int(min_keep))
        thr = split_thresholds(sel.row_ptr, sel.col, oth.n_rows, sel_ids, oth_ids, user_side,
                               seed, anchor, lo, hi, self.ws, row_cap)
        mu = split_mark(ub.row_ptr, ub.col, ib.n_rows, uids, iids, True, seed, user_side, thr,
                        anchor, self.ws)
        mi = split_mark(ib.row_ptr, ib.col, ub.n_rows, iids, uids, False, seed, not user_side,
                        thr, anchor, self.ws)
        nnz = int(mu[1][-1])
        if nnz != int(mi[1][-1]):
            raise RuntimeError("holdout: the two sides disagree on what stays")
        return mu, mi, nnz

    def _held_triples(self, mu, nnz):
        """The held-out ratings from the user side's marks, in that side's stored order:
        als_csr_remove_compact on the complement bits (tile_off of the complement = the tile's
        start minus the kept offset, its row pointer = the old one minus the kept one)."""
        ub = self.user_block
        n_held = self.nnz - nnz
        keep_bits, tile_off, row_ptr_kept = mu[:3]
        T = csr_remove_tile()
        start = torch.clamp(torch.arange(tile_off.numel(), device=self.device) * T, max=self.nnz)
        col, val = remove_compact(ub.col, ub.val, ~keep_bits, start - tile_off, None,
                                  self.item_block.n_rows, n_held)
        gone = ub.row_ptr - row_ptr_kept
        users = torch.repeat_interleave(self.uidx.ids(), gone[1:] - gone[:-1])
        return users.contiguous(), self.iidx.ids()[col.long()].contiguous(), val

    def _no_triples(self):
        e = torch.empty(0, dtype=torch.int32, device=self.device)
        return e, e.clone(), torch.empty(0, dtype=torch.float32, device=self.device)

    def holdout(self, *, count=None, fraction=None, fold=None, seed=0, min_keep=1,
                keep_items=True, user_side=True):
        """Hold ratings of every user out of the core in place and return them: the split a
        ranking metric needs (leave-k-out; HR@k, NDCG@k, MRR and the percentile rank are
        reported under it).  Exactly one of
          count=k          k ratings of every user (count=1 is leave-one-out),
          fraction=p       round(p e) of a user's e eligible ratings,
          fold=(f, F)      fold f of F stratified folds: every user's eligible ratings are cut
                           into F parts whose sizes differ by at most one.
        Which ratings go is a function of (seed, user id, item id) alone (a splitmix64 key per
        pair, ranked within the user's eligible ratings; K20, include/als_hip.h): the same on
        every run, whatever order the ratings were given in.  min_keep: count and fraction
        leave a user at least this many eligible ratings.  keep_items: the rating of every
        item with the smallest key is never held out, so no item leaves and no held-out pair
        is cold.  user_side=False mirrors everything (per item; anchors protect users).
        Stored copies of a pair go or stay together.
        Afterwards the core is, bit for bit, what ALSCore(the kept triples in their original
        order) holds, as after remove_ratings, and by the same tail: a row left without a
        rating leaves, rows that stay keep their factors, the rows that lost ratings join
        those refresh() re-solves.  Returns (users int32, items int32, ratings f32), the
        held-out triples as device tensors with external ids, in the user side's stored
        order; add_ratings(*held) puts them back.  A call that holds nothing out returns
        empty tensors and changes nothing; one that would hold out everything raises
        ValueError; nothing is changed when the call raises."""
        self._need_ratings("holdout")
        mu, mi, nnz = self._split_marks(count, fraction, fold, seed, min_keep, keep_items,
                                        user_side)
        if nnz == self.nnz:
            return self._no_triples()
        if nnz == 0:
            raise ValueError("holdout would hold out every rating: a model needs one")
        held = self._held_triples(mu, nnz)
        self._kept_commit(self._kept_state(mu, mi, nnz))
        return held

    def split(self, *, count=None, fraction=None, fold=None, seed=0, min_keep=1,
              keep_items=True, user_side=True):
        """holdout() without touching this core: (train_core, (users, items, ratings)).  The
        training core is a new unfitted ALSCore made of the compacted sides on the device (no
        K1, no host copy) and equals ALSCore(the kept triples in their original order) bit for
        bit; it shares nothing mutable with this core."""
        self._need_ratings("split")
        mu, mi, nnz = self._split_marks(count, fraction, fold, seed, min_keep, keep_items,
                                        user_side)
        if nnz == 0:
            raise ValueError("split would hold out every rating: a model needs one")
        held = self._held_triples(mu, nnz) if nnz != self.nnz else self._no_triples()
        st = self._kept_state(mu, mi, nnz, blocks_only=True)
        return self._from_blocks(st["su"]["idx"], st["si"]["idx"], st["csr"], nnz), held

    def _from_blocks(self, uidx: IdIndex, iidx: IdIndex, csr, nnz: int) -> "ALSCore":
        """An unfitted core over the given id maps and CSR sides ((row_ptr, col, val) of the
        user and of the item side, device tensors the new core owns), scheduled as this core
        is."""
        core = ALSCore.__new__(ALSCore)
        core._auto_chunk = self._auto_chunk
        core.device = self.device
        core.ws = Workspace(self.device, shared_rating_scale=True)
        core.ws_yty = Workspace(self.device)
        core.nnz = int(nnz)
        core.uidx, core.iidx = uidx, iidx
        core.user_block = schedule_block(uidx.n, nnz, *csr[0], core.ws, self.user_block.chunk)
        core.item_block = schedule_block(iidx.n, nnz, *csr[1], core.ws, self.item_block.chunk)
        core._blank_state()
        return core

    def fingerprint(self) -> dict:
        """Order-independent identity of the training ratings (checkpoint matching)."""
        v = self.user_block.val
        return {"nnz": int(self.nnz), "n_users": int(self.n_users), "n_items": int(self.n_items),
                "rating_bits": int(v.view(torch.int32).long().sum()),
                "item_id_sum": int(self.iidx.ids().long().sum())}

    def user_factor_ids(self) -> torch.Tensor:
        return self.uidx.ids()

    # ---- K4 / K5 (the serving protocol shared with distributed.ShardedALS) ----
    def predict(self, users, items) -> torch.Tensor:
        """fp64 <u, v> per pair (MatrixFactorizationModel.predict's ddot); NaN where
        either id is unknown."""
        u = _to_device(users, torch.int32, self.device)
        i = _to_device(items, torch.int32, self.device)
        return predict_pairs(u, i, self.uidx, self.iidx, self.U, self.V, self.rank)

    def rmse(self, users, items, ratings):
        """(sqrt(sum (r - p)^2 / n), n) over the pairs whose ids are both known —
        computeError (RecommenderSystem.py:103-129) fused into one pass."""
        u = _to_device(users, torch.int32, self.device)
        i = _to_device(items, torch.int32, self.device)
        r = _to_device(ratings, torch.float32, self.device)
        sse, n = rmse_pairs(u, i, r, self.uidx, self.iidx, self.U, self.V, self.rank,
                            self.ws).tolist()
        return (math.sqrt(sse / n) if n > 0 else float("nan")), int(n)

    def _sides(self, user_side: bool):
        if user_side:
            return self.uidx, self.U, self.iidx, self.V
        return self.iidx, self.V, self.uidx, self.U

    def train_exclusion(self, user_side: bool = True):
        """The pairs this core was fitted on as an exclusion list for one side's queries:
        (row_ptr int64 [n + 1], col int32 [nnz]), row r's other-side dense rows ascending in
        col[row_ptr[r]:row_ptr[r + 1]] (duplicates kept).  Built once per side and cached.
        RatingBlock.col is in input order, so the list is made by K1 itself: the OPPOSITE
        block's CSR, expanded to COO, has the wanted index ascending already, and
        als_csr_build's sort by this side's row is stable (O(nnz) memory, no 64-bit
        sort of the ratings)."""
        got = self._train_ex.get(bool(user_side))
        if got is not None:
            return got
        if self.user_block is None:
            raise ValueError("exclude='train' needs the ratings the model was fitted on; this "
                             "core was built from saved factors (from_factors / load) and has "
                             "none: pass the pairs to exclude explicitly")
        mine, opp = (self.user_block, self.item_block) if user_side else (self.item_block,
                                                                          self.user_block)
        i32 = dict(dtype=torch.int32, device=self.device)
        deg = opp.row_ptr[1:] - opp.row_ptr[:-1]
        # COO of the opposite block: its row (= the other side's dense row) per entry,
        # ascending; its col = this side's dense row.  Both are dense rows already, so the
        # two id maps K1 looks them up in are the identity
        other = torch.repeat_interleave(torch.arange(opp.n_rows, **i32), deg)
        rows = torch.arange(mine.n_rows, **i32)
        cols = torch.arange(opp.n_rows, **i32)
        # K1 has no way to skip the values: the fp32 copy and the COO index go as soon as
        # the sort has run (peak: 3 x 4 B per rating beside the two rating blocks and
        # K1's workspace; kept: 4 B per rating per side)
        row_ptr, col = build_csr(opp.col, IdIndex(rows, rows, mine.n_rows), other,
                                 IdIndex(cols, cols, opp.n_rows), opp.val, self.ws)[:2]
        del other
        self._train_ex[bool(user_side)] = (row_ptr, col)
        return row_ptr, col

    def _filter_args(self, exclude, candidates, user_side: bool, rows=None):
        """(ex_begin, ex_end, ex_col, allow_bits) of a filtered top-k over the query rows
        `rows` (dense, int64; None = every row of the side).  exclude: None, "train", or
        (query ids, other ids) pairs (host or device; unknown ids dropped, as predict's
        inner join does); candidates: None or ids of the other side (unknown dropped)."""
        qi, _, oi, _ = self._sides(user_side)
        beg = end = col = None
        if isinstance(exclude, str):
            if exclude != "train":
                raise ValueError(f"exclude must be None, 'train' or (ids, ids) pairs, got {exclude!r}")
            rp, col = self.train_exclusion(user_side)
            beg, end = rp[:-1], rp[1:]
        elif exclude is not None:
            a, b = exclude
            a = _to_device(a, torch.int32, self.device)
            b = _to_device(b, torch.int32, self.device)
            beg, end, col = _filters.exclusion_lists(qi.rows_of(a), oi.rows_of(b), qi.n)
        if beg is not None:
            if rows is not None:
                beg, end = beg[rows], end[rows]
            beg, end = beg.contiguous(), end.contiguous()
        return beg, end, col, self._allow_bits(oi, candidates)

    def _topk(self, Q, n_q, user_side, top, exclude, candidates, rows=None):
        _, _, oi, Vo = self._sides(user_side)
        if exclude is None and candidates is None:
            return topk_rows(Q, n_q, Vo, oi.n, self.rank, top)
        return topk_rows_filtered(Q, n_q, Vo, oi.n, self.rank, top,
                                  *self._filter_args(exclude, candidates, user_side, rows))

    def recommend_all(self, top: int, user_side: bool = True, *, exclude=None, candidates=None):
        """recommendForAll: for every row of one side (dense order) its `top` best
        rows of the other side.  Returns (keys [n], ids [n, t], scores [n, t]) on the
        device, t = min(top, rows of the other side), scores descending.
        exclude: pairs a row must not list — "train" (the pairs the core was fitted on)
        or (query ids, other ids); candidates: ids of the other side the lists are
        restricted to.  Slots past a row's admissible rows have score -inf."""
        qi, Q, oi, Vo = self._sides(user_side)
        idx, sc = self._topk(Q, qi.n, user_side, top, exclude, candidates)
        t = min(int(top), oi.n)
        return qi.ids(), ids_of(oi.ids(), idx[:, :t]), sc[:, :t]

    def recommend_subset(self, ids, top: int, user_side: bool = True, *, exclude=None,
                         candidates=None):
        """recommendForUserSubset / ForItemSubset: distinct known ids of `ids`
        (ascending) -> (keys, ids [m, t], scores [m, t]).  exclude / candidates as
        recommend_all (the subset's rows point into the one exclusion list)."""
        qi, Q, oi, Vo = self._sides(user_side)
        keys, rows = self._known_rows(qi, ids)
        t = min(int(top), oi.n)
        if keys.numel() == 0:
            return (keys, *self._empty_lists(0, t))
        Qs = Q.index_select(0, rows.long()).contiguous()
        idx, sc = self._topk(Qs, keys.numel(), user_side, top, exclude, candidates, rows.long())
        return keys, ids_of(oi.ids(), idx[:, :t]), sc[:, :t]

    # ---- K12: which rows are like this one? ----
    def _similar_args(self, top, user_side: bool, candidates):
        """(index, table, t, kernel top, allow mask) of a neighbour search on one side."""
        self._need_factors("similar")
        top = int(top)
        if not 1 <= top <= SIMILAR_MAX_TOP:
            raise ValueError(f"top must be in [1, {SIMILAR_MAX_TOP}], got {top}")
        qi, T, _, _ = self._sides(user_side)
        return qi, T, min(top, qi.n - 1), self._allow_bits(qi, candidates)

    def similar(self, ids, top: int, user_side: bool = False, *, candidates=None):
        """Cosine nearest neighbours inside one side's factors: for the distinct known ids
        of `ids` (ascending; unknown ids dropped, as recommend_subset drops them) the `top`
        most similar OTHER rows of the same side — items by default, users with
        user_side=True.  Returns (keys [m], ids [m, t], scores [m, t]) on the device,
        t = min(top, n - 1), cosine descending, ties by ascending dense row.
        candidates: ids of the same side the neighbours (not the queries) are restricted
        to.  Never listed: the row itself (by index: a different row with the same factors
        is, at similarity 1), and a row whose factors are all zero or hold a NaN / Inf;
        such a row as a query gets an empty list.  Empty slots have score -inf.
        Fewer than SIMILAR_SWEEP_MIN_ROWS queries sweep the raw table (K12, als_similar);
        more take the unit copy + K5 route (similar_rows_unit).  Both keep this contract,
        scores within 1e-5 of each other; neighbours closer than that may swap places."""
        qi, T, t, bits = self._similar_args(top, user_side, candidates)
        keys, rows = self._known_rows(qi, ids)
        m = int(keys.numel())
        if m == 0 or t == 0:
            return (keys, *self._empty_lists(m, t))
        if m >= SIMILAR_SWEEP_MIN_ROWS:
            idx, sc = similar_rows_unit(rows, T, qi.n, self.rank, t, bits)
        else:
            Q = T.index_select(0, rows).contiguous()
            idx, sc = similar_rows(Q, m, T, qi.n, self.rank, t, rows.to(torch.int32).contiguous(),
                                   bits)
        return keys, ids_of(qi.ids(), idx), sc

    def similar_all(self, top: int, user_side: bool = False, *, candidates=None):
        """similar for every row of the side, in dense order: (keys [n], ids [n, t], scores
        [n, t]).  One unit-norm copy of the table, then one K5 sweep with the copy on both
        sides (never n / 16 passes of K12)."""
        qi, T, t, bits = self._similar_args(top, user_side, candidates)
        if t == 0:
            return (qi.ids(), *self._empty_lists(qi.n, 0))
        idx, sc = similar_rows_unit(None, T, qi.n, self.rank, t, bits)
        return qi.ids(), ids_of(qi.ids(), idx), sc

    # ---- K14: lists that cover more than one taste ----
    def recommend_diverse(self, top: int, user_side: bool = True, *, ids=None,
                          trade_off: float = 0.7, pool=None, exclude=None, candidates=None,
                          chunk_rows=None):
        """recommend_all / recommend_subset re-ranked for diversity: K5 (or filtered K5) lists
        `pool` candidates per row, then K14 (als_diversify) picks `top` of them greedily by
        maximal marginal relevance, trade_off * relevance - (1 - trade_off) * (largest cosine
        to what the list already holds); trade_off = 1 gives the plain lists.
        ids: None = every row of the side in dense order, else the distinct known ids
        ascending (as recommend_subset).  pool: None = min(256, max(4 top, 50)), at most
        DIVERSIFY_MAX_POOL, capped at the other side's row count.  exclude / candidates as
        recommend_all.  Returns (keys [n], ids [n, t], scores [n, t], ils f64 [n]) on the
        device, t = min(top, pool): the picks in pick order with their K5 scores (not
        descending), open slots score -inf, and each list's intra-list similarity (mean
        pairwise cosine, NaN under two picks).
        The query rows go through in chunks of chunk_rows (None: as many as keep the pool
        arrays within DIVERSIFY_POOL_BYTES); the result does not depend on the chunking."""
        self._need_factors("recommend_diverse")
        top, lam = int(top), float(trade_off)
        if top < 1:
            raise ValueError(f"top must be >= 1, got {top}")
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"trade_off must be in [0, 1], got {trade_off}")
        if pool is None:
            pool = min(DIVERSIFY_MAX_POOL, max(4 * top, 50))
        pool = int(pool)
        if not 1 <= pool <= DIVERSIFY_MAX_POOL:
            raise ValueError(f"pool must be in [1, {DIVERSIFY_MAX_POOL}], got {pool}")
        if chunk_rows is not None and int(chunk_rows) < 1:
            raise ValueError(f"chunk_rows must be >= 1, got {chunk_rows}")
        qi, Q, oi, Vo = self._sides(user_side)
        pool = min(pool, oi.n)
        t = min(top, pool)
        dev = self.device
        if ids is None:
            keys, rows, n = qi.ids(), None, qi.n
        else:
            keys = torch.unique(_to_device(ids, torch.int32, dev))
            rows = qi.rows_of(keys)
            keys, rows = keys[rows >= 0], rows[rows >= 0]
            n = int(keys.numel())
        out_i = torch.empty((n, t), dtype=torch.int32, device=dev)
        out_s = torch.empty((n, t), dtype=torch.float32, device=dev)
        ils = torch.empty(n, dtype=torch.float64, device=dev)
        if n == 0 or t == 0:
            return keys, out_i, out_s, ils
        filtered = exclude is not None or candidates is not None
        beg, end, col, bits = self._filter_args(exclude, candidates, user_side, rows)
        step = int(chunk_rows) if chunk_rows is not None else max(1, DIVERSIFY_POOL_BYTES
                                                                 // (8 * pool))
        for r0 in range(0, n, step):
            r1 = min(n, r0 + step)
            Qc = Q[r0:r1] if rows is None else Q.index_select(0, rows[r0:r1]).contiguous()
            if filtered:
                pi, ps = topk_rows_filtered(
                    Qc, r1 - r0, Vo, oi.n, self.rank, pool,
                    None if beg is None else beg[r0:r1].contiguous(),
                    None if end is None else end[r0:r1].contiguous(), col, bits)
            else:
                pi, ps = topk_rows(Qc, r1 - r0, Vo, oi.n, self.rank, pool)
            out_i[r0:r1], out_s[r0:r1], ils[r0:r1] = diversify_rows(pi, ps, Vo, oi.n, self.rank,
                                                                    t, lam)
            del pi, ps
        return keys, ids_of(oi.ids(), out_i), out_s, ils

    def list_similarity(self, id_lists, user_side: bool = True):
        """Intra-list similarity of any lists: id_lists [n, m] (m <= DIVERSIFY_MAX_POOL) hold
        ids of the OTHER side — items for user_side=True, as recommend_all's ids — and the
        result is f64 [n] on the device, each list's mean pairwise cosine between the factor
        rows of its known ids (an unknown id is an open slot; NaN under two known ids)."""
        self._need_factors("list_similarity")
        _, _, oi, Vo = self._sides(user_side)
        lists = _to_device(id_lists, torch.int32, self.device)
        if lists.dim() != 2:
            raise ValueError(f"id_lists must be [n, m], got shape {tuple(lists.shape)}")
        rows = oi.rows_of(lists).to(torch.int32)
        return list_similarity_rows(rows, Vo, oi.n, self.rank)

    # ---- K15: do all rows get the same few blockbusters? ----
    def popularity(self, user_side: bool = True):
        """How often each row of the OTHER side was rated (int32 [n], dense order): the
        row-pointer differences of its rating block, no pass over the ratings.  None on a
        core built from saved factors."""
        block = self.item_block if user_side else self.user_block
        if block is None:
            return None
        return (block.row_ptr[1:] - block.row_ptr[:-1]).to(torch.int32).contiguous()

    def list_metrics(self, id_lists=None, *, top=None, user_side: bool = True, exclude=None,
                     candidates=None, popularity=None, head_fraction: float = 0.2,
                     per_row: bool = False) -> dict:
        """The lists of ALL rows looked at together (K15): {"coverage", "gini", "entropy",
        "effectiveItems", "personalization", "topItemShare", "novelty", "averagePopularity",
        "longTailShare", "lists", "entries", "skipped"} as list_metrics_dict defines them.
        Exactly one of
          id_lists [n, m]  ids of the OTHER side (items for user_side=True), m <= 256, from
                           anywhere; an id the model does not know is an open slot, as in
                           list_similarity
          top              the lists are made here: recommend_all(top) with the same
                           exclude / candidates
        candidates also defines the catalogue the coverage group is measured over.
        Popularity is the other side's rating counts (popularity()), the listing side's row
        count standing for the number of raters; a core built from_factors has no ratings and
        takes popularity=(ids, counts) — without it the three popularity fields are NaN and
        the rest is returned all the same.  The long tail is every catalogue row outside the
        floor(head_fraction * catalogue rows) most-rated ones (ties by ascending dense row).
        per_row: also "per_row" (f64 [n, 3] on the device: novelty, mean popularity, long-tail
        share of each list, NaN where undefined) and, with top=, "keys" (the ids of the
        rows)."""
        if (id_lists is None) == (top is None):
            raise ValueError("list_metrics takes either id_lists or top=, not both and not "
                             "neither")
        head_fraction = float(head_fraction)
        if not 0.0 < head_fraction < 1.0:
            raise ValueError(f"head_fraction must be inside (0, 1), got {head_fraction}")
        if top is not None and not 1 <= int(top) <= LIST_MAX_AT:
            raise ValueError(f"top must be in [1, {LIST_MAX_AT}], got {top}")
        if id_lists is not None:
            shape = tuple(id_lists.shape) if hasattr(id_lists, "shape") else np.shape(id_lists)
            if len(shape) != 2 or not 1 <= int(shape[1]) <= LIST_MAX_AT:
                raise ValueError(f"id_lists must be [n, m] with 1 <= m <= {LIST_MAX_AT}, got "
                                 f"shape {shape}")
            if exclude is not None:
                raise ValueError("exclude= shapes the lists made with top=; lists given as "
                                 "id_lists are taken as they are")
        self._need_factors("list_metrics")
        qi, Q, oi, _ = self._sides(user_side)
        keys = None
        if id_lists is not None:
            rows = oi.rows_of(_to_device(id_lists, torch.int32, self.device)).to(torch.int32)
        else:
            at = min(int(top), oi.n)
            idx, _ = self._topk(Q, qi.n, user_side, at, exclude, candidates)
            rows, keys = idx[:, :at], qi.ids()
        out = self._list_metrics_of_rows(rows, user_side, candidates=candidates,
                                        popularity=popularity, head_fraction=head_fraction,
                                        per_row=per_row)
        if per_row and keys is not None:
            out["keys"] = keys
        return out

    def _list_metrics_of_rows(self, rows: torch.Tensor, user_side: bool = True, *,
                             candidates=None, popularity=None, head_fraction: float = 0.2,
                             per_row: bool = False) -> dict:
        """list_metrics for lists that hold DENSE rows of the other side already (int32
        [n, m] on the device, -1 = open slot): the catalogue from `candidates`, popularity
        from the rating blocks or from popularity=(ids, counts), then the three K15 calls."""
        qi, _, oi, _ = self._sides(user_side)
        dev = self.device
        bits = cat_rows = None
        if candidates is not None:
            c = _to_device(candidates, torch.int32, dev)
            cat_rows = torch.unique(oi.rows_of(c))
            cat_rows = cat_rows[cat_rows >= 0]
            bits = _filters.pack_allow_bits(cat_rows, oi.n)
        pop = self.popularity(user_side)
        if popularity is not None:
            ids, cnt = popularity
            r = oi.rows_of(_to_device(ids, torch.int32, dev))
            cnt = _to_device(cnt, torch.int32, dev).reshape(-1)
            if r.numel() != cnt.numel():
                raise ValueError("popularity: ids and counts must have the same length")
            pop = torch.zeros(oi.n, dtype=torch.int32, device=dev)
            pop[r[r >= 0]] = cnt[r >= 0]
        out, pr = list_metrics_rows(rows, int(rows.shape[1]), oi.n, self.ws, allow_bits=bits,
                                    cat_rows=cat_rows, pop=pop, n_pop=qi.n,
                                    head_fraction=head_fraction, per_row=per_row)
        if per_row:
            out["per_row"] = pr
        return out

    # ---- K7: rows the model has never seen ----
    def _fold_in(self, ids, other_ids, ratings, reg, implicit, alpha, user_side,
                 nonnegative=False):
        """(keys, X [m, ld], n_used, row_ptr, col) of fold_in, X with its padding columns."""
        self._need_factors("fold_in")
        if reg < 0 or alpha < 0:
            raise ValueError(f"reg and alpha must be >= 0, got {reg}, {alpha}")
        _, _, oi, Y = self._sides(user_side)
        q = _to_device(ids, torch.int32, self.device)
        o = _to_device(other_ids, torch.int32, self.device)
        r = _to_device(ratings, torch.float32, self.device)
        keys, row_ptr, col, val = _filters.ragged_rows(q, oi.rows_of(o), r)
        if keys.numel() == 0:
            return (keys, torch.empty((0, ld_for(self.rank)), dtype=torch.float32,
                                      device=self.device),
                    torch.empty(0, dtype=torch.int32, device=self.device), row_ptr, col)
        yty = compute_yty(Y, oi.n, self.rank, self.ws_yty) if implicit else None
        if nonnegative:
            X, n_used, _ = nnls_rows(row_ptr, col, val, Y, oi.n, self.rank, reg, implicit, alpha,
                                     yty, self.ws)
            return keys, X, n_used, row_ptr, col
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        X, n_used = fold_in_rows(row_ptr, col, val, Y, oi.n, self.rank, reg, implicit, alpha, yty,
                                 status, self.ws)
        raise_status(int(status.item()), " of the rows folded in (distinct ids ascending)")
        return keys, X, n_used, row_ptr, col

    def fold_in(self, ids, other_ids, ratings, *, reg, implicit=False, alpha=1.0,
                user_side: bool = True, nonnegative: bool = False):
        """Factor rows for rows the model was not fitted on, without a refit: one row of one
        half-sweep each (K7, als_fold_in), x = (sum y y^T + reg n I)^-1 sum r y over the
        row's ratings against the fixed other side (the implicit form with YtY when
        `implicit`).  ids: the grouping key of each rating — new users (new items when
        user_side is False); they may or may not collide with ids the model knows, and the
        model's own U / V are never touched.  other_ids: the rated items (users); one the
        model does not know is skipped.  reg / implicit / alpha as in fit().
        Returns (keys [m] = the distinct ids ascending, X f32 [m, rank], n_used int32 [m] =
        ratings used per row) on the device; a row whose every rating was skipped is zero
        with n_used 0.  Works on a from_factors core.  Raises RuntimeError when a row's
        normal equations are not positive definite (reg = 0 with fewer ratings than rank).
        nonnegative: the row is the minimiser under x >= 0 instead (K13, Spark's NNLS solver:
        what a half-sweep of fit(nonnegative=True) computes for it); no row fails."""
        keys, X, n_used, _, _ = self._fold_in(ids, other_ids, ratings, float(reg), bool(implicit),
                                              float(alpha), bool(user_side), bool(nonnegative))
        return keys, X[:, :self.rank], n_used

    def recommend_new(self, ids, other_ids, ratings, top: int, *, reg, implicit=False, alpha=1.0,
                      user_side: bool = True, exclude_rated: bool = True, candidates=None,
                      nonnegative: bool = False):
        """fold_in, then the `top` best rows of the other side for each folded row (K5 with
        the folded rows as the query matrix): (keys [m], ids [m, t], scores [m, t]) as
        recommend_subset returns them, t = min(top, rows of the other side).
        exclude_rated: a new row never lists what it rated itself (the reference's R:229
        for a user who is not in the model); candidates: ids of the other side the lists
        are restricted to (R:245).  Rows without a single used rating are dropped.
        nonnegative: as fold_in."""
        keys, X, n_used, row_ptr, col = self._fold_in(ids, other_ids, ratings, float(reg),
                                                      bool(implicit), float(alpha),
                                                      bool(user_side), bool(nonnegative))
        _, _, oi, Vo = self._sides(user_side)
        t = min(int(top), oi.n)
        keep = n_used > 0
        keys, Q = keys[keep], X[keep].contiguous()
        m = int(keys.numel())
        if m == 0:
            return (keys, *self._empty_lists(0, t))
        beg = end = ex = None
        if exclude_rated:
            n_all = int(row_ptr.numel()) - 1
            new_row = torch.repeat_interleave(torch.arange(n_all, device=self.device),
                                              row_ptr[1:] - row_ptr[:-1])
            beg, end, ex = _filters.exclusion_lists(new_row, col, n_all)
            beg, end = beg[keep].contiguous(), end[keep].contiguous()
        bits = self._allow_bits(oi, candidates)
        if beg is None and bits is None:
            idx, sc = topk_rows(Q, m, Vo, oi.n, self.rank, top)
        else:
            idx, sc = topk_rows_filtered(Q, m, Vo, oi.n, self.rank, top, beg, end, ex, bits)
        return keys, ids_of(oi.ids(), idx[:, :t]), sc[:, :t]

    # ---- K11: why was this recommended? ----
    def _explain_rows_of(self, q, user_side: bool, ratings):
        """(pair row int64 or -1, row_ptr, col, val): the rating rows behind the query ids
        q — slices of the training block (ratings None) or the caller's ratings grouped by
        filters.ragged_rows."""
        qi, _, oi, _ = self._sides(user_side)
        if ratings is not None:
            ids, other, vals = ratings
            keys, row_ptr, col, val = _filters.ragged_rows(
                _to_device(ids, torch.int32, self.device),
                oi.rows_of(_to_device(other, torch.int32, self.device)),
                _to_device(vals, torch.float32, self.device))
            if keys.numel() == 0:
                return torch.full_like(q, -1, dtype=torch.int64), row_ptr, col, val
            at = torch.searchsorted(keys, q).clamp_(max=keys.numel() - 1)
            return torch.where(keys[at] == q, at, -1), row_ptr, col, val
        block = self.user_block if user_side else self.item_block
        if block is None:
            raise ValueError("explain needs each row's ratings; this core was built from saved "
                             "factors (from_factors / load) and holds none: pass ratings=(ids, "
                             "other ids, values)")
        dense = qi.rows_of(q)
        uniq, inv = torch.unique(dense[dense >= 0], return_inverse=True)
        pair_row = torch.full_like(dense, -1)
        pair_row[dense >= 0] = inv
        return (pair_row, *gather_rows(block.row_ptr, block.col, block.val, uniq))

    def explain(self, users, items, top_n: int = 10, *, reg, implicit=False, alpha=1.0,
                user_side: bool = True, ratings=None):
        """Why each (user, item) pair scores what it does: the score as a sum with one term
        per rating the user gave, score = sum_j wb_j y_i^T A_u^-1 y_j over the user's
        normal equations (K11, als_explain; reg / implicit / alpha as in fit(), and as in
        fold_in they decide A_u).  Pairs are grouped by user, so a user is factored once
        however many items are explained.
        ratings=None: each user's ratings are the ones the core was fitted on.
        ratings=(ids, other_ids, values): the rows to explain from, grouped by id as fold_in
        groups them — users the model has never seen, or a core restored from_factors.
        user_side=False explains item rows against the user factors: the row is the item,
        its ratings are users, and the contributions name users.
        Returns device tensors over the pairs kept, in input order (a pair whose user has no
        rating row — unknown to the model, or absent from `ratings` — is dropped):
        (users [m], items [m], score f32 [m], ids int32 [m, top_n], ratings f32 [m, top_n],
        contrib f32 [m, top_n], n_contrib int32 [m]).  Row p lists its n_contrib[p] largest
        contributions, descending (ties: earlier rating first): the id of the other side
        that was rated, the rating, and its share of the score; slots past n_contrib hold
        id -1, rating 0 and contribution 0.  score sums ALL the row's contributions, not
        only the listed ones; it is NaN for a target the model does not know.  After a
        fit, score equals predict() to rounding on the side solved last (users)."""
        top_n = int(top_n)
        if not 1 <= top_n <= EXPLAIN_MAX_TOP:
            raise ValueError(f"top_n must be in [1, {EXPLAIN_MAX_TOP}], got {top_n}")
        self._need_factors("explain")
        reg, alpha = float(reg), float(alpha)
        if reg < 0 or alpha < 0:
            raise ValueError(f"reg and alpha must be >= 0, got {reg}, {alpha}")
        _, _, oi, Y = self._sides(user_side)
        u, i = (x.reshape(-1) for x in self._pairs(users, items))
        q, o = (u, i) if user_side else (i, u)
        pair_row, row_ptr, col, val = self._explain_rows_of(q, bool(user_side), ratings)
        keep = pair_row >= 0
        u, i, o, pair_row = u[keep], i[keep], o[keep], pair_row[keep]
        m = int(u.numel())
        f32 = dict(dtype=torch.float32, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        if m == 0:
            return (u, i, torch.empty(0, **f32), torch.empty((0, top_n), **i32),
                    torch.empty((0, top_n), **f32), torch.empty((0, top_n), **f32),
                    torch.empty(0, **i32))
        n_rows = int(row_ptr.numel()) - 1
        order, tgt_ptr = group_pairs(pair_row, n_rows)
        tgt = oi.rows_of(o)[order].to(torch.int32).contiguous()
        yty = compute_yty(Y, oi.n, self.rank, self.ws_yty) if implicit else None
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        score, pos, contrib, _ = explain_rows(row_ptr, col, val, Y, oi.n, self.rank, reg,
                                              bool(implicit), alpha, yty, tgt_ptr, tgt, top_n,
                                              status, self.ws)
        raise_status(int(status.item()), " of the rows explained (distinct ids ascending)")
        # entry offset inside the row -> the rated id and its rating
        filled = pos >= 0
        entry = (row_ptr[pair_row[order]].unsqueeze(1) + pos.clamp(min=0).long())
        entry = torch.where(filled, entry, 0)
        ids = torch.where(filled, ids_of(oi.ids(), col[entry].clamp(min=0)), -1).to(torch.int32)
        rat = torch.where(filled, val[entry], 0.0)
        score = torch.where(tgt >= 0, score, float("nan"))
        back = torch.empty_like(order)
        back[order] = torch.arange(m, device=self.device)  # slot of each input pair
        return (u, i, score[back], ids[back], rat[back], contrib[back],
                filled.sum(1).to(torch.int32)[back])

    def rank_metrics(self, users, items, at: int, *, ratings=None, threshold=None,
                     user_side: bool = True, exclude=None, candidates=None,
                     per_row: bool = False) -> dict:
        """Ranking quality of the top-`at` lists against held-out (user, item) pairs:
        Spark's RankingMetrics precisionAt / recallAt / meanAveragePrecisionAt / ndcgAt
        (binary relevance), lists and metrics both on the device (K5 then K6).
        Pairs with an unknown id are dropped (rmse's inner join); with `threshold` only
        pairs with rating >= threshold are relevant (`ratings` required).  The query
        rows are the users (items when user_side is False) with at least one relevant
        pair; their lists come from the recommend path with top = min(at, rows of the
        other side) and exclude / candidates passed through (exclude="train" scores
        unseen items only).  Returns {"precision", "recall", "map", "ndcg", "hitRate"
        (rows with at least one hit), "rows"}: means over `rows`, NaN when rows == 0.
        per_row: also "keys" (ids of the query rows, ascending) and "per_row"
        (f64 [rows, 4]: precision, recall, AP, NDCG), both on the device."""
        qi, Q, oi, _ = self._sides(user_side)
        at = int(at)
        if at < 1 or at > MAX_RANK_AT:
            raise ValueError(f"at must be in [1, {MAX_RANK_AT}], got {at}")
        u, i = self._pairs(users, items)
        q, o = (qi.rows_of(u), oi.rows_of(i)) if user_side else (qi.rows_of(i), oi.rows_of(u))
        keep = (q >= 0) & (o >= 0)
        if threshold is not None:
            if ratings is None:
                raise ValueError("threshold needs the held-out ratings")
            r = _to_device(ratings, torch.float32, self.device)
            if r.numel() != u.numel():
                raise ValueError("users, items and ratings must have the same length")
            keep &= r >= float(threshold)
        rows, inv = torch.unique(q[keep], return_inverse=True)  # ascending dense rows
        n = int(rows.numel())
        if n == 0:
            out = rank_metrics_dict([0.0] * 6, 0)
            if per_row:
                out["keys"] = qi.ids()[:0]
                out["per_row"] = torch.empty((0, 4), dtype=torch.float64, device=self.device)
            return out
        beg, end, col = _filters.relevance_lists(inv, o[keep], n)
        t = min(at, oi.n)
        Qs = Q.index_select(0, rows).contiguous()
        idx, _ = self._topk(Qs, n, user_side, t, exclude, candidates, rows)
        sums, pr = rank_metrics_rows(idx, t, beg, end, col, self.ws, per_row)
        sums = sums.tolist()
        out = rank_metrics_dict(sums, int(sums[4]))
        if per_row:
            out["keys"] = qi.ids()[rows]
            out["per_row"] = pr
        return out

    def full_rank_metrics(self, users, items, *, ratings=None, threshold=None,
                          weighted: bool = False, user_side: bool = True, exclude=None,
                          candidates=None, per_row: bool = False,
                          positions: bool = False) -> dict:
        """Where the held-out (user, item) pairs sit in each user's ordering of ALL
        admissible items (K9: one sweep of the whole score matrix, nothing cut at k): the
        measure an implicit-feedback fit is judged by.  Pairs with an unknown id are left
        out and counted in "dropped" (rmse's inner join); with `threshold` only pairs with
        rating >= threshold are relevant; duplicates count once.  exclude / candidates as
        rank_metrics: an item they rule out for a user is not part of that user's ordering
        (exclude="train" ranks each held-out item among the unseen items only), and a
        held-out pair they rule out itself is left out and counted in "inadmissible".
        weighted: each pair weighs its rating in expectedPercentileRank (Hu, Koren &
        Volinsky's sum r * rank / sum r; a duplicate pair keeps its first rating).
        Returns full_rank_dict's keys — expectedPercentileRank, meanPercentileRank, auc, mrr,
        rows, pairs, inadmissible — and "dropped".  Ties are counted at mid-rank.
        per_row: also "keys" (ids of the query rows, ascending) and "per_row" (f64 [rows, 3]:
        mean percentile rank, AUC, reciprocal rank; NaN where undefined), on the device.
        positions: also "row" / "col" (query-row index into "keys" order and dense row of
        the other side, per relevant pair), "above", "tied" (int32 per pair, -1 for an
        inadmissible one) and "n_adm" (int32 per query row), on the device."""
        self._need_factors("full_rank_metrics")
        qi, Q, oi, Vo = self._sides(user_side)
        u, i = self._pairs(users, items)
        r = None
        if threshold is not None or weighted:
            if ratings is None:
                raise ValueError("threshold / weighted need the held-out ratings")
            r = _to_device(ratings, torch.float32, self.device)
            if r.numel() != u.numel():
                raise ValueError("users, items and ratings must have the same length")
        q, o = (qi.rows_of(u), oi.rows_of(i)) if user_side else (qi.rows_of(i), oi.rows_of(u))
        keep = (q >= 0) & (o >= 0)
        dropped = int(u.numel()) - int(keep.sum().item())
        if threshold is not None:
            keep &= r >= float(threshold)
        rows, inv = torch.unique(q[keep], return_inverse=True)  # ascending dense rows
        n = int(rows.numel())
        i32 = dict(dtype=torch.int32, device=self.device)
        if n == 0:
            out = full_rank_dict([0.0] * len(FULL_RANK_SUMS))
            out["dropped"] = dropped
            if per_row:
                out["keys"] = qi.ids()[:0]
                out["per_row"] = torch.empty((0, 3), dtype=torch.float64, device=self.device)
            if positions:
                out.update(row=torch.empty(0, **i32), col=torch.empty(0, **i32),
                           above=torch.empty(0, **i32), tied=torch.empty(0, **i32),
                           n_adm=torch.empty(0, **i32))
                out.setdefault("keys", qi.ids()[:0])
            return out
        wts = None
        if weighted:
            beg, end, col, wts = _filters.relevance_lists_weighted(inv, o[keep], r[keep], n)
        else:
            beg, end, col = _filters.relevance_lists(inv, o[keep], n)
        Qs = Q.index_select(0, rows).contiguous()
        above, tied, n_adm = rank_positions_rows(
            Qs, n, Vo, oi.n, self.rank, beg, end, col,
            *self._filter_args(exclude, candidates, user_side, rows))
        sums, pr = full_rank_sums_rows(above, tied, n_adm, beg, end, self.ws, wts, per_row)
        out = full_rank_dict(sums.tolist())
        out["dropped"] = dropped
        if per_row or positions:
            out["keys"] = qi.ids()[rows]
        if per_row:
            out["per_row"] = pr
        if positions:
            out["row"] = torch.repeat_interleave(torch.arange(n, **i32), end - beg)
            out["col"] = col[:above.numel()]
            out.update(above=above, tied=tied, n_adm=n_adm)
        return out

    def regression_metrics(self, users, items, ratings, through_origin: bool = False) -> dict:
        """Spark's RegressionMetrics of the model's predictions against held-out ratings, in
        one fused pass (K8, als_regression_moments): no prediction column is materialised.
        Pairs with an unknown id are left out and counted (rmse's inner join).  Returns
        regression_dict's keys: mse, rmse, mae, r2, var, n, dropped, meanLabel, varLabel."""
        self._need_factors("regression_metrics")
        u, i, r = self._triples(users, items, ratings)
        m = regression_moments_pairs(u, i, r, self.uidx, self.iidx, self.U, self.V, self.rank,
                                     self.ws)
        return regression_dict(m.tolist(), through_origin)

    # ---- K16: rating statistics and bias baselines ----
    def _stats_block(self, user_side: bool, what: str) -> RatingBlock:
        block = self.user_block if user_side else self.item_block
        if block is None:
            raise ValueError(f"{what} needs the training ratings: a core built from_factors "
                             "holds none")
        return block

    def rating_stats(self, user_side: bool = False) -> dict:
        """Per-row statistics of the training ratings (K16; getCountsAndAverages plus spread
        and range), items by default: {"ids", "count", "mean", "std", "std_sample", "min",
        "max"} as rating_stats_dict defines them, device tensors in dense (ascending id)
        order."""
        block = self._stats_block(user_side, "rating_stats")
        mom, _ = row_moments(block, self.n_items if user_side else self.n_users, self.ws)
        out = {"ids": (self.uidx if user_side else self.iidx).ids()}
        out.update(rating_stats_dict(mom))
        return out

    def global_stats(self) -> dict:
        """{count, mean, std, min, max} of all training ratings (std: population), host
        numbers."""
        block = self._stats_block(False, "global_stats")
        _, total = row_moments(block, self.n_users, self.ws)
        n, s, m2, lo, hi = total.tolist()
        return {"count": int(n), "mean": s / n if n else float("nan"),
                "std": math.sqrt(m2 / n) if n else float("nan"), "min": lo, "max": hi}

    def top_rated(self, num: int, min_count: int = 0, user_side: bool = False,
                  damping: float = 0.0):
        """The `num` rows with more than `min_count` ratings (strictly) and the highest
        sum / (damping + count) — the plain mean at damping 0 — highest first, ties to the
        smaller id: (ids, means, counts), device tensors."""
        if int(num) < 0 or float(damping) < 0:
            raise ValueError("top_rated: num and damping must be >= 0")
        block = self._stats_block(user_side, "top_rated")
        mom, _ = row_moments(block, self.n_items if user_side else self.n_users, self.ws)
        n, s = mom[:, 0], mom[:, 1]
        keep = ((n > float(min_count)) & (n > 0)).nonzero().flatten()   # dense = ascending id
        score = s[keep] / (float(damping) + n[keep])
        order = torch.sort(score, descending=True, stable=True).indices[:int(num)]
        rows = keep[order]
        return ((self.uidx if user_side else self.iidx).ids()[rows], score[order],
                n[rows].to(torch.int64))

    def fit_baseline(self, method: str = "bias", reg_user: float = 10.0, reg_item: float = 25.0,
                     sweeps: int = 10) -> Baseline:
        """The mean / damped-bias predictor of the training ratings (K16):
          "global"  mu, the training mean (RecommenderSystem.py:172-177)
          "item"    mu + b_i, b_i = sum_i (r - mu) / (reg_item + n_i)
          "user"    mu + b_u, b_u = sum_u (r - mu) / (reg_user + n_u)
          "bias"    mu + b_u + b_i: `sweeps` times (b_i given b_u, then b_u given b_i) from zero
        Each update minimises SSE + reg_user sum b_u^2 + reg_item sum b_i^2 over its table
        exactly, so Baseline.history (that objective after every sweep; one entry for the
        other methods) never rises.  It comes from the sweep's own moments — a row updated to b
        keeps M2_row + n_row (mean_row - b)^2 of squared error — with no further pass over
        the ratings."""
        if method not in BASELINE_METHODS:
            raise ValueError(f"method must be one of {BASELINE_METHODS}, got {method!r}")
        if float(reg_user) < 0 or float(reg_item) < 0 or int(sweeps) < 1:
            raise ValueError("fit_baseline: reg_user, reg_item must be >= 0 and sweeps >= 1")
        ib = self._stats_block(False, "fit_baseline")
        ub = self._stats_block(True, "fit_baseline")
        f64 = dict(dtype=torch.float64, device=self.device)
        bu, bi = torch.zeros(self.n_users, **f64), torch.zeros(self.n_items, **f64)
        _, total = row_moments(ib, self.n_users, self.ws)
        n, s, m2 = total.tolist()[:3]
        mu = s / n

        def update(block, n_cols, other, damping, out):
            mom, _ = row_moments(block, n_cols, self.ws, other=other, offset=mu)
            bias_update(mom, damping, out=out)
            cnt, mean = mom[:, 0], torch.where(mom[:, 0] > 0, mom[:, 1] / mom[:, 0], 0.0)
            return (mom[:, 2] + cnt * (mean - out) ** 2).sum()

        history = []
        if method == "global":
            history.append(m2)
        elif method == "item":
            sse = update(ib, self.n_users, None, reg_item, bi)
            history.append(float(sse + reg_item * (bi * bi).sum()))
        elif method == "user":
            sse = update(ub, self.n_items, None, reg_user, bu)
            history.append(float(sse + reg_user * (bu * bu).sum()))
        else:
            for _ in range(int(sweeps)):
                update(ib, self.n_users, bu, reg_item, bi)
                sse = update(ub, self.n_items, bi, reg_user, bu)
                history.append(float(sse + reg_user * (bu * bu).sum()
                                     + reg_item * (bi * bi).sum()))
        return Baseline(method, mu, bu, bi, self.uidx, self.iidx, history, self.ws,
                        reg_user, reg_item)

    # ---- K19: which rows were rated together with this one? ----
    def _co_rated_args(self, top, user_side: bool, measure, min_common, candidates, what: str):
        """(index, queried block, other block, t, allow mask) of a co-rated search."""
        top = int(top)
        if not 1 <= top <= CO_RATED_MAX_TOP:
            raise ValueError(f"top must be in [1, {CO_RATED_MAX_TOP}], got {top}")
        if measure not in CO_RATED_MEASURES:
            raise ValueError(f"measure must be one of {CO_RATED_MEASURES}, got {measure!r}")
        if int(min_common) < 1:
            raise ValueError(f"min_common must be >= 1, got {min_common}")
        mine = self._stats_block(user_side, what)
        other = self._stats_block(not user_side, what)
        qi = self.uidx if user_side else self.iidx
        return qi, mine, other, top, self._allow_bits(qi, candidates)

    def co_rated(self, ids, top: int, user_side: bool = False, *, measure: str = "jaccard",
                 min_common: int = 1, candidates=None):
        """Co-rated neighbours from the training ratings themselves (K19, als_co_rated): for
        the distinct known ids of `ids` (ascending; unknown ids dropped, as similar drops
        them) the `top` OTHER rows of the same side that share the most raters with it —
        "who rated X also rated Y" for items (the default), "who rated what I rated" for
        users.  With n_a the ratings of row a and c the ratings the pair shares (rows of the
        other side that rated both; duplicate ratings count with their multiplicity),
        measure is "count" (c), "jaccard" (c / (n_a + n_b - c)) or "cosine" (c / sqrt(n_a
        n_b)); rating values are not used.  A row is listed when c >= min_common and it is
        among `candidates` (ids of the same side; None = all).  Returns (keys [m], ids [m, t],
        scores [m, t], common [m, t]) on the device, t = top, score descending, ties by
        ascending dense row; slots past a row's neighbours have score -inf and common 0.
        Exact: only integers are summed.  Needs the ratings (not a from_factors core)."""
        qi, mine, other, t, bits = self._co_rated_args(top, user_side, measure, min_common,
                                                       candidates, "co_rated")
        keys, rows = self._known_rows(qi, ids)
        idx, sc, common = co_rated_rows(mine, other, rows, t, measure, min_common, bits, self.ws)
        return keys, ids_of(qi.ids(), idx), sc, common

    def co_rated_all(self, top: int, user_side: bool = False, *, measure: str = "jaccard",
                     min_common: int = 1, candidates=None):
        """co_rated for every row of the side, in dense order: (keys [n], ids [n, t], scores
        [n, t], common [n, t]); the rows go through the kernel in passes of CO_RATED_PASS.
        Cost: counting walks, for every row of the other side, its ratings once per rating
        it holds — sum over those rows of len^2 integer adds; ranking reads the n counters
        of each of the n queries, n^2 overall.  That suits a catalogue of 10^4 - 10^5 rows
        (the item side), not a side of 10^7 users."""
        qi, mine, other, t, bits = self._co_rated_args(top, user_side, measure, min_common,
                                                       candidates, "co_rated_all")
        rows = torch.arange(qi.n, dtype=torch.int32, device=self.device)
        idx, sc, common = co_rated_rows(mine, other, rows, t, measure, min_common, bits, self.ws)
        return qi.ids(), ids_of(qi.ids(), idx), sc, common

    def recommend_users(self, top: int):
        """For every user (dense order): top items as (item ids, scores)."""
        _, ids, sc = self.recommend_all(top, True)
        return ids, sc

    def recommend_items(self, top: int):
        _, ids, sc = self.recommend_all(top, False)
        return ids, sc

    def user_factors(self, cache: bool = True):
        return self.uidx.ids(), self.U[:, :self.rank]

    def item_factors(self, cache: bool = True):
        return self.iidx.ids(), self.V[:, :self.rank]
