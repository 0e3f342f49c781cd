"""Shared host plumbing of every binding module: the growable device scratch buffer the
library is handed on each call, host -> device conversion, the factor tables' padded row
length (ld_for, als_k_pad) and the solve status word (raise_status).  Binds no kernel of
its own."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from .. import _lib


def ld_for(rank: int) -> int:
    return (rank + 3) // 4 * 4


class Workspace:
    """One growable device scratch buffer; the library never allocates on a compute call.

    shared_rating_scale: every block solved with this workspace has the same ratings
    (ALSCore's user- and item-major CSR of one rating set), so the rating scale word
    that als_solve_half's phase 8 leaves at the start of the buffer stays valid until
    another call uses the buffer or it is reallocated; solve_half then skips phase 8."""

    def __init__(self, device, shared_rating_scale: bool = False):
        self.device = device
        self.buf: Optional[torch.Tensor] = None
        self.shared_rating_scale = shared_rating_scale
        self.rating_scale_key = None

    def get(self, nbytes: int, keep_scale: bool = False) -> torch.Tensor:
        nbytes = max(int(nbytes), 256)
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            # the scale / rescue-count words: a call without PREP on a fresh buffer
            # must not start from garbage
            self.buf[:256].zero_()
            self.rating_scale_key = None
        if not keep_scale:
            self.rating_scale_key = None
        return self.buf


def _to_device(x, dtype, device) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x)), device=device).to(dtype).contiguous()


def k_pad(rank: int) -> int:
    return int(_lib.lib().als_k_pad(rank))


def raise_status(s: int, where: str = "") -> None:
    """Raise for a non-zero solve status word: row + 1 of a failed Cholesky (Spark's
    dppsv info > 0), or -1 when the fp64 rescue list overflowed (als_solve_half's
    LAUNCH phases ran twice without the RESCUE phase between them)."""
    if s < 0:
        raise RuntimeError(f"als_solve_half rescue list overflow{where}: the LAUNCH phases ran "
                           "again before the RESCUE phase consumed the list (unsolved rows)")
    if s > 0:
        raise RuntimeError(
            f"Cholesky failed (non-positive pivot) for dense row {s - 1}{where}: the normal "
            "equations are not positive definite (Spark raises from LAPACK dppsv here)")


def _host_f64(x) -> ctypes.c_double:
    """A host double the library reads through its address before the call returns."""
    return ctypes.c_double(float(x))
