"""Guard-band memory for the buffer-contract tests (test_gpu_buffer_bounds.py).

Every compute call of libals_hip.so works in caller-owned memory: a workspace sized by the
matching *_workspace_bytes(), outputs of a stated shape, inputs of a stated length.  No GPU
address sanitizer is available to this project, so the tests hand the library views carved
out of one tensor they own, each exactly as long as the contract says and fenced by 1 MiB
of a known byte on both sides; after the call the fences are compared on the device.  An
overrun then lands in memory the test owns, and is seen.

    arena = Arena("cuda", 0xFF)
    ws = GuardedWorkspace(arena, offset16=True)   # an engine.Workspace of exact sizes
    out = arena.carve(4 * n, torch.int32, (n,))   # payload keeps the fill: "never written"
    Y = arena.put(Y_host_or_device, offset16=True)  # carved, then copied into
    ... call ...
    assert arena.check() == {}
"""
from typing import Dict, List, Optional

import torch

from als_mi355x import engine as E

GUARD = 1 << 20    # bytes of fill before and after every payload
ALIGN = 256        # payload start: a multiple of ALIGN, or 16 past one (offset16)


class Arena:
    """One uint8 tensor filled with the byte `fill`, handed out as fenced views."""

    def __init__(self, device, fill: int, capacity: int = 96 << 20):
        if not 0 <= int(fill) <= 255:
            raise ValueError(f"fill must be a byte, got {fill}")
        self.device = torch.device(device)
        self.fill = int(fill)
        self.buf = torch.full((int(capacity) + ALIGN,), self.fill, dtype=torch.uint8,
                              device=self.device)
        self.base = self.buf.data_ptr()
        self.cursor = 0          # first byte not yet part of a carve or its guards
        self.carves: List[dict] = []

    def carve(self, nbytes: int, dtype=torch.uint8, shape=None, offset16: bool = False,
              name: Optional[str] = None) -> torch.Tensor:
        """A view of exactly nbytes bytes (dtype, shape) between two guards of at least GUARD
        bytes.  Its address is a multiple of 256, or 16 past one with offset16.  The payload
        holds the fill."""
        nbytes = int(nbytes)
        item = torch.empty((), dtype=dtype).element_size()
        if nbytes <= 0 or nbytes % item:
            raise ValueError(f"carve of {nbytes} bytes as {dtype}: need a positive multiple of "
                             f"{item}")
        start = self.cursor + GUARD
        start += -(self.base + start) % ALIGN     # the slack joins the front guard
        if offset16:
            start += 16
        end = start + nbytes
        if end + GUARD > self.buf.numel():
            raise MemoryError(f"arena of {self.buf.numel()} bytes is full "
                              f"({len(self.carves)} carves; raise `capacity`)")
        view = self.buf[start:end].view(dtype)
        if shape is not None:
            view = view.view(shape)
        self.carves.append(dict(name=name or f"carve{len(self.carves)}", front=self.cursor,
                                start=start, end=end, back=end + GUARD))
        self.cursor = end + GUARD
        return view

    def out(self, shape, dtype, offset16: bool = False, name: Optional[str] = None
            ) -> torch.Tensor:
        """An output table of `shape`: exactly its bytes, still holding the fill."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = 1
        for s in shape:
            n *= s
        item = torch.empty((), dtype=dtype).element_size()
        return self.carve(n * item, dtype, shape, offset16, name)

    def put(self, src, dtype=None, offset16: bool = False, name: Optional[str] = None
            ) -> torch.Tensor:
        """An input table: carved to exactly src's bytes, then copied into, so the guards
        around it hold the fill and not whatever an allocator would have left there."""
        src = torch.as_tensor(src)
        if dtype is not None:
            src = src.to(dtype)
        view = self.out(tuple(src.shape), src.dtype, offset16, name)
        view.copy_(src.to(self.device))
        return view

    def check(self) -> Dict[str, List[int]]:
        """{carve name: byte offsets, relative to its payload, of the guard bytes that no
        longer hold the fill}; offsets are negative in the front guard and >= nbytes in the
        back guard.  {} = every guard is intact.  Compared on the device: only the indices
        of changed bytes come back."""
        if not self.carves:
            return {}
        bad = self.buf[:self.cursor] != self.fill
        for c in self.carves:
            bad[c["start"]:c["end"]] = False
        hits = bad.nonzero().flatten().tolist()
        out: Dict[str, List[int]] = {}
        j = 0
        for c in self.carves:   # carves are in address order, and so are the hits
            while j < len(hits) and hits[j] < c["back"]:
                out.setdefault(c["name"], []).append(hits[j] - c["start"])
                j += 1
        return out


class GuardedWorkspace(E.Workspace):
    """An engine.Workspace whose get(nbytes) is a fresh carve of exactly max(nbytes, 256)
    bytes (the floor of Workspace.get): never grown, never reused, never zeroed, so every
    engine wrapper passes the size function's own result as ws_bytes and the scratch starts
    as the arena's fill.  hold = True keeps handing back the last carve while the size asked
    for is the same: the multi-call sequences als_hip.h defines on one workspace."""

    def __init__(self, arena: Arena, offset16: bool = False):
        super().__init__(arena.device)
        self.arena = arena
        self.offset16 = offset16
        self.hold = False

    def get(self, nbytes: int, keep_scale: bool = False) -> torch.Tensor:
        nbytes = max(int(nbytes), 256)
        if not (self.hold and self.buf is not None and self.buf.numel() == nbytes):
            self.buf = self.arena.carve(nbytes, torch.uint8, None, self.offset16,
                                        name=f"workspace{len(self.arena.carves)}")
        self.rating_scale_key = None
        return self.buf
