"""Buffer contract of K19 (als_co_rated) on guard-band memory (guard_arena.py): idx, score and
common are carved to exactly [n_q, top], the scratch to exactly als_co_rated_scratch_bytes()
and the inputs are put 16 bytes past a 256-byte boundary.  Run on an arena filled with 0x00
and on one filled with 0xFF: no guard byte may change, the outputs must be the same bits
under both fills and equal the numpy restatement, and — the scratch rule include/als_hip.h
states — the scratch needs no initialisation and its strips are zero after the call.
"""
import numpy as np
import pytest
import torch

import co_rated_ref as R
import guard_arena as G
from als_mi355x import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"

# K19's size function -> the tests that run the entry point on an exact-size carve
# (test_co_rated_cpu.py fails when the ABI gains an als_co_rated_*_bytes without an entry here)
SCRATCH_CASES = {"als_co_rated_scratch_bytes": ["test_co_rated_guarded",
                                                "test_co_rated_many_slices_guarded"]}


def _run(arena, sides, n, n_o, q, top, measure, min_common, allow, pas, task):
    L = _lib.lib()
    (rp_q, col_q), (rp_o, col_o) = sides
    t = [arena.put(torch.as_tensor(x), offset16=True) for x in (rp_q, col_q, rp_o, col_o)]
    qd = arena.put(torch.as_tensor(np.asarray(q, np.int32)), offset16=True)
    bits = None
    if allow is not None:
        words = np.packbits(np.pad(allow, (0, -len(allow) % 32)), bitorder="little").view(np.int32)
        bits = arena.put(torch.as_tensor(words), offset16=True)
    n_q = len(q)
    idx = arena.out((n_q, top), torch.int32, name="idx")
    score = arena.out((n_q, top), torch.float32, name="score")
    common = arena.out((n_q, top), torch.int32, name="common")
    need = L.als_co_rated_scratch_bytes(n, n_q, top, pas)
    assert need > 0
    ws = arena.carve(need, offset16=False, name="scratch")
    p = lambda x: 0 if x is None else x.data_ptr()
    _lib.check(L.als_co_rated(p(t[0]), p(t[1]), n, p(t[2]), p(t[3]), n_o, p(qd), n_q,
                              R.MEASURES.index(measure), min_common, p(bits), top, pas, task,
                              p(idx), p(score), p(common), p(ws), need, _lib.stream_ptr(DEV)),
               "als_co_rated")
    torch.cuda.synchronize()
    strips = 4 * min(n_q, pas or 32) * n
    assert int(ws[:strips].count_nonzero()) == 0, "the strips are not zero after the call"
    return [x.clone().cpu().numpy() for x in (idx, score, common)]


def _both_fills(users, items, n_u, n_i, q, top, measure, min_common=1, allow=None, pas=0, task=0,
                user_side=False):
    item_side, user_side_csr = R.csr(items, users, n_i), R.csr(users, items, n_u)
    B = R.multiplicity(users, items, n_u, n_i)
    if user_side:
        sides, B, n, n_o = (user_side_csr, item_side), B.T, n_u, n_i
    else:
        sides, n, n_o = (item_side, user_side_csr), n_i, n_u
    outs = []
    for fill in (0x00, 0xFF):
        arena = G.Arena(DEV, fill, capacity=64 << 20)
        outs.append(_run(arena, sides, n, n_o, q, top, measure, min_common, allow, pas, task))
        bad = arena.check()
        assert not bad, (f"fill {fill:#04x}: bytes outside a buffer were written: "
                         f"{ {k: (v[:8], len(v)) for k, v in bad.items()} }")
    ref = R.co_rated(B, q, top, measure, min_common, allow)
    for a, b, r in zip(outs[0], outs[1], ref):
        assert a.tobytes() == b.tobytes(), "the output depends on the arena's fill"
        assert a.dtype == r.dtype and a.tobytes() == r.tobytes()


def _ratings(seed, n_u, n_i, nnz):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n_u, nnz), np.minimum((rng.random(nnz) ** 2 * n_i).astype(np.int64),
                                                 n_i - 1)


@pytest.mark.parametrize("user_side", [False, True])
@pytest.mark.parametrize("measure,top,pas,task", [("count", 1, 0, 0), ("jaccard", 10, 3, 7),
                                                  ("jaccard", 256, 0, 1)])
def test_co_rated_guarded(measure, top, pas, task, user_side):
    n_u, n_i = 120, 97
    u, i = _ratings(17, n_u, n_i, 1500)
    n = n_u if user_side else n_i
    q = np.concatenate([np.arange(n), [-1, n, 5, 5]]).astype(np.int32)[:70 if pas else None]
    allow = np.ones(n, bool)
    allow[::9] = False
    _both_fills(u, i, n_u, n_i, q, top, measure, min_common=2 if top == 10 else 1,
                allow=allow if top != 1 else None, pas=pas, task=task, user_side=user_side)


def test_co_rated_many_slices_guarded():
    """A table of 65 slices (the two-stage merge), the last one shorter than the others."""
    n_i, n_u = 65 * 512 + 1, 12
    rng = np.random.default_rng(19)
    u = np.repeat(np.arange(n_u), 200)
    i = rng.integers(0, n_i, len(u))
    i[::200] = n_i - 1                               # every user rated the last row
    _both_fills(u, i, n_u, n_i, [n_i - 1, 0], 256, "jaccard")
