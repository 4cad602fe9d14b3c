"""Gradient sink: where the HIP backward functions write parameter grads.

While one model group's backward pass runs (trainer._grads_for), the sink
maps each of that group's parameters to its view in the group's flat grad
buffer. The conv / norm backward functions then have the kernel that
finishes a gradient write it there, in the parameter's own layout, adding
to what is there when the parameter already received a gradient in this
pass (a model called twice in one step), and return None to autograd. That
removes the per-parameter crop/permute copy, autograd's add for twice-used
parameters and the copy into the flat buffer.

A conv parameter that requires grad but is not in the active sink belongs
to a model that is frozen for this pass (a discriminator in a generator's
pass): no weight or bias gradient is computed for it at all.

With no sink active (CPU path, ops called directly, CYG_NO_GRAD_SINK=1)
nothing changes: the backward functions return their gradients to autograd.

The state is host-side. Backward order is deterministic, so a captured
graph replays exactly the accumulate flags it was captured with.
"""

from __future__ import annotations

import os
from contextlib import contextmanager
from typing import Dict, Iterable, Optional, Tuple

import torch


class GradSink:
    """parameter -> [flat-grad view, touched]. Keyed on the parameter's
    storage address (its slice of the flat parameter buffer), which
    identifies it however autograd hands the saved tensor back."""

    def __init__(self, params: Iterable[torch.Tensor],
                 views: Iterable[torch.Tensor]):
        self._slots: Dict[int, list] = {}
        for p, v in zip(params, views):
            assert v.dtype == torch.float32 and v.is_contiguous()
            assert v.shape == p.shape
            self._slots[p.data_ptr()] = [v, False]

    def has(self, p: torch.Tensor) -> bool:
        return p.data_ptr() in self._slots

    def take(self, p: torch.Tensor) -> Tuple[torch.Tensor, bool]:
        """(destination view, accumulate) for p's next gradient; marks p
        as touched."""
        slot = self._slots[p.data_ptr()]
        view, touched = slot
        slot[1] = True
        return view, touched

    def touched(self, p: torch.Tensor) -> bool:
        slot = self._slots.get(p.data_ptr())
        return slot is not None and slot[1]


# the slot the backward functions read
_ACTIVE: Optional[GradSink] = None


def current() -> Optional[GradSink]:
    return _ACTIVE


def enabled() -> bool:
    """CYG_NO_GRAD_SINK=1 turns the sink off; read per backward pass."""
    return os.environ.get("CYG_NO_GRAD_SINK") != "1"


@contextmanager
def active(sink: Optional[GradSink]):
    global _ACTIVE
    prev, _ACTIVE = _ACTIVE, sink
    try:
        yield sink
    finally:
        _ACTIVE = prev


def frozen(sink: Optional[GradSink], p: torch.Tensor) -> bool:
    """p is a leaf parameter of a model the active pass does not train:
    its gradient would be discarded, so it is not computed.

    Precondition: while a sink is active, every leaf whose gradient the
    pass asks autograd for is in that sink, i.e. the ``inputs`` of
    torch.autograd.grad are exactly the group's flat-buffer parameters
    (trainer._grads_for). A leaf that requires grad, reaches an op here
    and is requested without being in the sink would get None silently;
    set_grads' returned-or-touched assertion covers the group's own
    parameters only."""
    return sink is not None and p.is_leaf and not sink.has(p)
