"""Buffer contracts of the K15 entry points (als_list_exposure, als_list_concentration,
als_list_novelty) on guard-band memory (guard_arena.py): counts, outputs, the per-row table
and the workspaces are carved to exactly the sizes include/als_hip.h states, the inputs are
put 16 bytes past a 256-byte boundary, and the lists have idx_ld == at, so nothing may be read
past a row.  Run on an arena filled with 0x00 and on one filled with 0xFF: no guard byte may
change, and the results must be the same bits under both fills (nothing depends on memory the
call does not own) and equal the numpy reference.
"""
import numpy as np
import pytest
import torch

import guard_arena as G
import list_metrics_ref as LR
from als_mi355x import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32, I64, F64 = torch.int32, torch.int64, torch.float64

# K15's size functions -> the tests below that run their entry point on an exact-size carve
# (test_list_metrics_cpu.py fails when the ABI gains an als_list_*_bytes without an entry here)
SCRATCH_CASES = {
    "als_list_concentration_scratch_bytes": ["test_list_metrics_all_guarded"],
    "als_list_novelty_scratch_bytes": ["test_list_metrics_all_guarded"],
}


def _call(name, *args):
    conv = [(0 if a is None else a.data_ptr()) if (a is None or isinstance(a, torch.Tensor))
            else a for a in args]
    _lib.check(getattr(_lib.lib(), name)(*conv, _lib.stream_ptr(DEV)), name)


def _case(n_q, at, n_v, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(-1, n_v + 1, size=(n_q, at)).astype(np.int32)   # -1 and n_v: skipped
    allowed = rng.random(n_v) < 0.7
    pop = rng.integers(0, 500, size=n_v).astype(np.int32)
    tail = LR.pack_bits(LR.long_tail(pop, n_v, 0.2, allowed))
    return idx, LR.pack_bits(allowed), pop, tail


def _run(arena, idx, bits, pop, tail, n_v):
    L = _lib.lib()
    n_q, at = idx.shape
    put = lambda x: arena.put(torch.as_tensor(x), offset16=True)
    idx_d, bits_d, pop_d, tail_d = put(idx), put(bits), put(pop), put(tail)
    counts = arena.out((n_v,), I32)
    skipped = arena.out((1,), I64)
    _call("als_list_exposure", idx_d, n_q, at, at, n_v, bits_d, 0, counts, skipped)
    conc = arena.out((7,), F64)
    w = arena.carve(L.als_list_concentration_scratch_bytes(n_v), offset16=True, name="ws_conc")
    _call("als_list_concentration", counts, n_v, bits_d, n_q, at, conc, w, w.numel())
    sums, rows = arena.out((7,), F64), arena.out((n_q, 3), F64)
    w2 = arena.carve(L.als_list_novelty_scratch_bytes(n_q), offset16=True, name="ws_nov")
    _call("als_list_novelty", idx_d, n_q, at, at, n_v, bits_d, pop_d, 1000, tail_d, sums, rows, w2,
          w2.numel())
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in dict(counts=counts, skipped=skipped, conc=conc, sums=sums,
                                          rows=rows).items()}


@pytest.mark.parametrize("n_q,at,n_v", [(1, 1, 1), (257, 10, 33), (70, 65, 20011), (5, 256, 1200)])
def test_list_metrics_all_guarded(n_q, at, n_v):
    idx, bits, pop, tail = _case(n_q, at, n_v, seed=n_q + at)
    outs = []
    for fill in (0x00, 0xFF):
        arena = G.Arena(DEV, fill, capacity=48 << 20)
        outs.append(_run(arena, idx, bits, pop, tail, n_v))
        bad = arena.check()
        assert not bad, (f"fill {fill:#04x}: bytes outside a buffer were written: "
                         f"{ {k: (v[:8], len(v)) for k, v in bad.items()} }")
    for key in outs[0]:
        a, b = outs[0][key].cpu().numpy(), outs[1][key].cpu().numpy()
        assert a.tobytes() == b.tobytes(), f"'{key}' depends on the arena's fill"
    got = {k: v.cpu().numpy() for k, v in outs[0].items()}
    counts, skipped = LR.exposure(idx, at, n_v, bits)
    assert (got["counts"] == counts).all() and int(got["skipped"][0]) == skipped
    want = LR.concentration(counts, bits)
    for f in (0, 1, 2, 5, 6):
        assert got["conc"][f] == want[f], f
    np.testing.assert_allclose(got["conc"][3:5], want[3:5], rtol=1e-12, atol=0, equal_nan=True)
    sums, rows = LR.novelty(idx, at, n_v, pop, 1000, bits, tail)
    np.testing.assert_allclose(got["rows"], rows, rtol=1e-12, atol=0, equal_nan=True)
    np.testing.assert_allclose(got["sums"], sums, rtol=1e-12, atol=0)
