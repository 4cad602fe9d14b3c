"""Image history pool (Zhu et al. 2017, §4, after Shrivastava et al.): the
discriminators are updated on a buffer of earlier generated images, not
only on the newest ones. One HIP kernel per batch (_hip/pool.hip).

    pool_exchange(pool, fake, codes) -> out, per element b in batch order:

    codes[b] == -1       pass:  out[b] = fake[b]
    codes[b] == s <  P   swap:  out[b] = pool[s];  pool[s] = fake[b]
    codes[b] == P + s    fill:  pool[s] = fake[b]; out[b] = fake[b]

If two elements of one batch name the same slot, the second sees what the
first stored.

The decisions never depend on image content, so they are drawn on the host
(``ImagePool.draw``), possibly many steps ahead (``ImagePool.plan``), and
reach the kernel as a small int32 tensor. The kernel trusts ``codes``: a
bad value would be an out-of-range access on the GPU, so their range is
checked on the host where they are built — ``make_codes`` validates and
only then uploads. Nothing is read back from the device to check it.
"""

from __future__ import annotations

import copy
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import backend

PASS = -1


def check_codes(codes_host: torch.Tensor, P: int) -> None:
    """Host check: every code is in [-1, 2P)."""
    assert codes_host.device.type == "cpu"
    if codes_host.numel() and (int(codes_host.min()) < -1
                               or int(codes_host.max()) >= 2 * P):
        raise ValueError(
            f"pool: code out of range [-1, {2 * P}): "
            f"min {int(codes_host.min())}, max {int(codes_host.max())}")


def make_codes(values, P: int, device) -> torch.Tensor:
    """int32 codes ([B], or a [steps,B] table): built on the host,
    validated, uploaded."""
    codes = torch.as_tensor(values, dtype=torch.int64)
    check_codes(codes, P)
    return codes.to(torch.int32).to(device)


def _exchange_torch(pool, fake, codes, out):
    # the literal sequential loop: CPU implementation and kernel oracle
    P = pool.shape[0]
    codes_h = codes.cpu()
    check_codes(codes_h, P)
    for b, code in enumerate(codes_h.tolist()):
        if code < 0:
            out[b].copy_(fake[b])
        elif code < P:
            out[b].copy_(pool[code])
            pool[code].copy_(fake[b])
        else:
            pool[code - P].copy_(fake[b])
            out[b].copy_(fake[b])
    return out


def pool_exchange(pool: torch.Tensor, fake: torch.Tensor, codes: torch.Tensor,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pool [P,H,W,C] (updated in place), fake [B,H,W,C], codes i32 [B] ->
    [B,H,W,C], written into ``out`` if given. One dtype, all contiguous."""
    if (pool.dim() != 4 or fake.dim() != 4 or pool.shape[0] < 1
            or pool.shape[1:] != fake.shape[1:]):
        raise ValueError(f"pool: pool is {tuple(pool.shape)}, fake "
                         f"{tuple(fake.shape)}; expected [P,H,W,C] / [B,H,W,C]")
    if codes.dtype != torch.int32 or tuple(codes.shape) != (fake.shape[0],):
        raise ValueError(f"pool: codes is {tuple(codes.shape)} {codes.dtype}, "
                         f"expected ({fake.shape[0]},) torch.int32")
    if out is None:
        out = torch.empty_like(fake, memory_format=torch.contiguous_format)
    elif out.shape != fake.shape:
        raise ValueError(f"pool: out is {tuple(out.shape)}, expected "
                         f"{tuple(fake.shape)}")
    if fake.dtype != pool.dtype or out.dtype != pool.dtype:
        raise ValueError(f"pool: dtypes differ: pool {pool.dtype}, fake "
                         f"{fake.dtype}, out {out.dtype}")
    if not (pool.is_contiguous() and fake.is_contiguous()
            and out.is_contiguous() and codes.is_contiguous()):
        raise ValueError("pool: pool, fake, codes and out must be contiguous")
    if not backend.use_hip(pool, fake):
        return _exchange_torch(pool, fake, codes, out)
    return backend.ext().pool_exchange(pool, fake, codes, out)


class ImagePool:
    """A [P,H,W,C] history buffer and the host-side decision stream that
    drives it.

    ``draw`` is the published algorithm; ``plan`` draws many steps ahead
    and uploads them as one int32 table, so a step only needs a row of it
    (``next_codes``) — no host-to-device copy and no synchronisation per
    step. ``count`` is the fill count after every decision drawn so far,
    planned ones included; the rows planned but not yet consumed are part
    of the state."""

    def __init__(self, pool_size: int, image_shape: Sequence[int],
                 dtype: torch.dtype, device, seed):
        if pool_size < 1:
            raise ValueError(f"pool: pool_size must be >= 1, got {pool_size}")
        self.P = int(pool_size)
        self.buf = torch.zeros((self.P, *image_shape), dtype=dtype,
                               device=device)
        self.count = 0
        self.rng = np.random.default_rng(seed)
        # planned, not yet consumed: the host rows, the device table they
        # were uploaded as, and the table row of _pending[0]
        self._pending: List[List[int]] = []
        self._table: Optional[torch.Tensor] = None
        self._row = 0

    # ---- decisions (host) ----

    def draw(self, b: int) -> List[int]:
        """Codes of the next ``b`` elements. Per element, in order: fill
        slot ``count`` while the pool is not full; otherwise one
        ``rng.random()``, and if it is > 0.5 one ``rng.integers(P)`` names
        the slot to swap with; otherwise pass."""
        codes = []
        for _ in range(b):
            if self.count < self.P:
                codes.append(self.P + self.count)
                self.count += 1
            elif self.rng.random() > 0.5:
                codes.append(int(self.rng.integers(self.P)))
            else:
                codes.append(PASS)
        return codes

    def plan(self, batch_sizes: Sequence[int]) -> torch.Tensor:
        """Draw one row per step ahead of time -> int32 device table
        [steps, max(batch_sizes)], rows padded with -1; step i's kernel
        gets ``table[i, :batch_sizes[i]]`` from ``next_codes``."""
        if self._pending:
            raise RuntimeError(f"pool: {len(self._pending)} planned steps "
                               "have not been consumed")
        rows = [self.draw(b) for b in batch_sizes]
        self._set_plan(rows)
        return self._table

    def _set_plan(self, rows: List[List[int]]) -> None:
        self._pending, self._row = rows, 0
        if not rows:
            self._table = None
            return
        width = max(len(r) for r in rows)
        padded = [r + [PASS] * (width - len(r)) for r in rows]
        self._table = make_codes(padded, self.P, self.buf.device).reshape(
            len(rows), width)

    def next_codes(self, b: int) -> torch.Tensor:
        """Device codes [b] of the next step: the next planned row if a
        plan is pending, else a fresh draw uploaded now."""
        if not self._pending:
            return make_codes(self.draw(b), self.P, self.buf.device)
        if len(self._pending[0]) != b:
            raise RuntimeError(f"pool: next planned step has "
                               f"{len(self._pending[0])} elements, got {b}")
        self._pending.pop(0)
        row = self._table[self._row, :b]
        self._row += 1
        return row

    # ---- exchange (device) ----

    def exchange(self, fake: torch.Tensor, codes: torch.Tensor,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return pool_exchange(self.buf, fake, codes, out)

    # ---- state ----

    def decision_state(self) -> dict:
        """Everything but the buffer (host only)."""
        return {"count": self.count,
                "rng": copy.deepcopy(self.rng.bit_generator.state),
                "pending": [list(r) for r in self._pending]}

    def load_decision_state(self, state: dict) -> None:
        self.count = int(state["count"])
        self.rng.bit_generator.state = copy.deepcopy(state["rng"])
        self._set_plan([list(r) for r in state["pending"]])

    def state_dict(self) -> dict:
        return {"buf": self.buf.clone(), **self.decision_state()}

    def load_state_dict(self, state: dict) -> None:
        if tuple(state["buf"].shape) != tuple(self.buf.shape):
            raise ValueError(f"pool: saved buffer is "
                             f"{tuple(state['buf'].shape)}, this pool "
                             f"{tuple(self.buf.shape)}")
        self.buf.copy_(state["buf"])
        self.load_decision_state(state)
