"""The guard-band helper (guard_arena.py) on CPU tensors, and the coverage list of the GPU
buffer-contract tests: every *_workspace_bytes() of the ABI has a case there."""
import pytest
import torch

import guard_arena as G
from als_mi355x import _lib
from als_mi355x import engine as E


def _arena(fill=0xA5, n=3):
    return G.Arena("cpu", fill, capacity=n * (2 * G.GUARD + 4096))


def _poke(arena, view, offset, value):
    """Write one byte at `offset` relative to the view's first byte."""
    arena.buf[view.data_ptr() - arena.base + offset] = value


@pytest.mark.parametrize("fill", [0x00, 0xFF, 0xA5])
def test_clean_carves_report_nothing(fill):
    a = _arena(fill)
    x = a.carve(40, torch.int32, (2, 5))
    y = a.carve(24, torch.float64, None, offset16=True)
    z = a.put(torch.arange(7, dtype=torch.float32))
    assert x.shape == (2, 5) and x.dtype == torch.int32 and x.numel() * 4 == 40
    assert y.shape == (3,) and z.tolist() == list(range(7))
    assert bytes(x.view(torch.uint8).flatten().tolist()) == bytes([fill]) * 40   # payload = fill
    x.fill_(-7)          # writing the whole payload, first and last byte included, is clean
    y.fill_(1.5)
    assert a.check() == {}


def test_alignment_256_and_offset16():
    a = _arena(n=4)
    assert a.carve(1).data_ptr() % 256 == 0
    assert a.carve(16, torch.float32, (4,), offset16=True).data_ptr() % 256 == 16
    assert a.put(torch.zeros(5, dtype=torch.int64)).data_ptr() % 256 == 0
    assert a.out((3, 4), torch.float32, offset16=True).data_ptr() % 256 == 16
    for c in a.carves:   # at least GUARD bytes of fill on both sides of every payload
        assert c["start"] - c["front"] >= G.GUARD and c["back"] - c["end"] == G.GUARD
    assert [c["front"] for c in a.carves[1:]] == [c["back"] for c in a.carves[:-1]]


@pytest.mark.parametrize("offset16", [False, True])
def test_one_byte_outside_is_reported_at_its_offset(offset16):
    a = _arena(0x00, n=3)
    a.carve(64, name="before")
    v = a.carve(100, torch.uint8, None, offset16, name="mid")
    a.carve(64, name="after")
    c = a.carves[1]
    far_front = -(c["start"] - c["front"])
    far_back = 100 + G.GUARD - 1
    for off in (-1, 100, far_front, far_back):
        _poke(a, v, off, 1)
        assert a.check() == {"mid": [off]}, off
        _poke(a, v, off, 0)
        assert a.check() == {}
    for off in (-1, 100, far_front, far_back):
        _poke(a, v, off, 0xEE)
    assert a.check() == {"mid": [far_front, -1, 100, far_back]}
    # the neighbours' guards are their own: one byte past "mid"'s back guard is "after"'s
    _poke(a, v, far_back + 1, 3)
    got = a.check()
    assert set(got) == {"mid", "after"} and len(got["after"]) == 1 and got["after"][0] < 0


def test_fill_ff_sees_a_zero_written_outside():
    a = _arena(0xFF)
    v = a.carve(8, torch.int32, (2,))
    assert v.tolist() == [-1, -1]
    _poke(a, v, 8, 0)
    assert a.check() == {"carve0": [8]}


def test_bad_carves_are_refused():
    a = _arena(n=1)
    with pytest.raises(ValueError):
        a.carve(0)
    with pytest.raises(ValueError):
        a.carve(6, torch.float32)
    with pytest.raises(ValueError):
        G.Arena("cpu", 256, capacity=16)
    a.carve(4096)
    with pytest.raises(MemoryError):
        a.carve(4096)


def test_guarded_workspace_is_exact_fresh_and_unzeroed():
    a = _arena(0xFF, n=6)
    ws = G.GuardedWorkspace(a, offset16=True)
    assert isinstance(ws, E.Workspace)
    seen = set()
    for n in (0, 1, 255, 256, 257, 1000):
        w = ws.get(n)
        assert w.numel() == max(n, 256) and w.dtype == torch.uint8
        assert w.data_ptr() % 256 == 16 and w.data_ptr() not in seen   # never reused
        assert int(w.min()) == 0xFF                                     # not zeroed
        assert ws.buf is w
        seen.add(w.data_ptr())
    assert len(a.carves) == 6 and a.check() == {}
    assert G.GuardedWorkspace(a).offset16 is False


def test_guarded_workspace_hold_keeps_one_carve_for_a_call_sequence():
    a = _arena(n=3)
    ws = G.GuardedWorkspace(a)
    w0 = ws.get(512, keep_scale=True)
    ws.hold = True
    assert ws.get(512).data_ptr() == w0.data_ptr()
    w1 = ws.get(768)
    assert w1.data_ptr() != w0.data_ptr()      # another size: another carve
    ws.hold = False
    assert ws.get(768).data_ptr() != w1.data_ptr()
    assert len(a.carves) == 3


def test_every_workspace_size_function_has_a_bounds_case():
    """A new *_workspace_bytes() in the ABI must come with a guard-band case."""
    import test_gpu_buffer_bounds as B
    sizers = sorted(n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes"))
    assert len(sizers) >= 15
    missing = [n for n in sizers if not B.WORKSPACE_CASES.get(n)]
    assert not missing, f"no buffer-bounds case for {missing}"
    assert sorted(B.WORKSPACE_CASES) == sizers, "WORKSPACE_CASES names a function the ABI lacks"
    for name, tests in B.WORKSPACE_CASES.items():
        for t in tests:
            assert callable(getattr(B, t, None)), f"{name}: {t} is not a test of the bounds file"
