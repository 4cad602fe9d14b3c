"""Fused InstanceNorm (NHWC) — per-(sample,channel) mean/var over H*W.

Replicates tfa.layers.InstanceNormalization (groups=-1) semantics used by the
reference (/root/reference/cyclegan/model.py:58-72): eps=1e-3 (tfa default,
NOT PyTorch's 1e-5), affine gamma/beta with gamma~N(0,0.02), beta=0.

MI355X fusion: the normalize pass optionally fuses the following ReLU /
LeakyReLU and/or a residual add (resblock tail, model.py:73) so the
activation tensor makes one HBM round trip instead of three.

gamma/beta stay fp32 (256 floats — L2-resident); x may be bf16 or fp32;
statistics always accumulate in fp32.
"""

from __future__ import annotations

import os
from typing import Optional

import torch

from . import backend, grad_sink
from . import conv as _conv
from .conv import (ACT_NONE, ACT_RELU, ACT_LRELU, FP8_TWIN_ATTR,
                   IN_SLABS_ATTR, _ACT, Fp8Consumer)

EPS_DEFAULT = 1e-3  # tfa InstanceNormalization default


def _in_ref(x, gamma, beta, eps, act, slope, residual):
    # compute in fp32 for bf16 inputs; keep native precision otherwise
    # (fp64 gradcheck needs the graph to stay fp64)
    cdt = torch.float32 if x.dtype == torch.bfloat16 else x.dtype
    xf = x.to(cdt)
    mean = xf.mean(dim=(1, 2), keepdim=True)
    var = xf.var(dim=(1, 2), unbiased=False, keepdim=True)
    y = (xf - mean) * torch.rsqrt(var + eps)
    y = y * gamma.to(cdt) + beta.to(cdt)
    y = y.to(x.dtype)
    if residual is not None:
        y = y + residual
    if act == ACT_RELU:
        y = torch.relu(y)
    elif act == ACT_LRELU:
        y = torch.nn.functional.leaky_relu(y, slope)
    return y


def _mask_from_x(act: int) -> bool:
    """relu/lrelu backward can recompute the activation mask from x instead
    of reading the activated output in both backward kernels. Measured
    +0.4 % on the bench (333.6 -> 335.0 images/s), inside the run-to-run
    spread, so it is opt-in: CYG_IN_BWD_MASK_X=1."""
    return (act in (ACT_RELU, ACT_LRELU)
            and os.environ.get("CYG_IN_BWD_MASK_X") == "1")


class _InstNormFn(torch.autograd.Function):
    """amax_prev/amax_cur (the consumer conv's fp8_state slots, or None):
    the normalize kernel also writes the e4m3 twin of y and the call
    returns (y, yq), yq non-differentiable."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, act, slope, residual, psum, psq,
                amax_prev=None, amax_cur=None):
        ext = backend.ext()
        betaf = beta.float()
        yq = None
        if amax_prev is not None:
            y, mean, rstd, yq = ext.instnorm_fwd_q8(
                x, gamma.float(), betaf, eps, act, slope, residual, psum, psq,
                psum.shape[0] if psum is not None else 0, amax_prev, amax_cur)
        elif psum is not None:
            y, mean, rstd = ext.instnorm_fwd(x, gamma.float(), betaf, eps, act,
                                             slope, residual, psum, psq,
                                             psum.shape[0])
        else:
            y, mean, rstd = ext.instnorm_fwd(x, gamma.float(), betaf, eps, act,
                                             slope, residual)
        ctx.save_for_backward(x, gamma, mean, rstd, y, betaf)
        ctx.conf = (eps, act, slope, residual is not None)
        if yq is not None:
            # no zero-filled grad for the twin in backward
            ctx.set_materialize_grads(False)
            ctx.mark_non_differentiable(yq)
            return y, yq
        return y

    @staticmethod
    def backward(ctx, dy, *_):
        if dy is None:  # only with set_materialize_grads(False): y unused
            return (None,) * 11
        x, gamma, mean, rstd, y, betaf = ctx.saved_tensors
        eps, act, slope, has_res = ctx.conf
        ext = backend.ext()
        dy = dy.contiguous()
        # both parameters in the active sink: in_bwd_dx's atomics land in
        # their flat-grad views. Otherwise (no sink, or a model frozen for
        # this pass) the kernels run as ever into a buffer of their own.
        sink = grad_sink.current()
        dest = (None, None, False)
        if sink is not None and sink.has(gamma) and sink.has(betaf):
            dg_out, acc = sink.take(gamma)
            db_out, acc_b = sink.take(betaf)
            assert acc == acc_b
            dest = (dg_out, db_out, acc)
        if has_res and act != ACT_NONE:
            # rare combo: residual grad needs the transformed dy explicitly
            dy = ext.act_bwd(dy, y, act, slope)
            dres = dy
            dx, dgamma, dbeta = ext.instnorm_bwd(dy, x, gamma.float(), mean,
                                                 rstd, None, ACT_NONE, 0.0,
                                                 None, *dest)
        else:
            dres = dy if has_res else None
            yact = y if (act != ACT_NONE and not _mask_from_x(act)) else None
            dx, dgamma, dbeta = ext.instnorm_bwd(
                dy, x, gamma.float(), mean, rstd, yact, act, slope, betaf,
                *dest)
        if dest[0] is not None:
            dgamma = dbeta = None
        return (dx, dgamma, dbeta, None, None, None, dres,
                None, None, None, None)


def _slabs_for(x: torch.Tensor):
    """Slabs the producing conv attached to x, if they describe x."""
    st = getattr(x, IN_SLABS_ATTR, None)
    if st is None or x.dim() != 4:
        return None, None
    psum, psq = st
    want = (x.shape[0], x.shape[3])
    if (psum.dim() != 3 or tuple(psum.shape[1:]) != want
            or psq.shape != psum.shape or psum.device != x.device):
        return None, None
    return psum, psq


def _twin_slots(x: torch.Tensor, consumer: Optional[Fp8Consumer]):
    """(amax_prev, amax_cur) of the fp8 conv that will read this norm's
    output, when a twin is worth making: fp8 mode on, conv2d's own
    dispatch predicate says that conv takes the fp8 path for a tensor of
    x's shape and dtype (the norm keeps both), and the layer already owns
    a slot. On a layer's first eager call there is none: no twin, and the
    conv bootstraps its scale as before. CYG_NO_FP8_TWIN=1 turns it off."""
    if (consumer is None or not _conv.fp8_mode()
            or os.environ.get("CYG_NO_FP8_TWIN") == "1"
            or not _conv.takes_fp8_path(x, consumer.weight, consumer.stride)):
        return None
    from . import fp8_state
    return fp8_state.peek(consumer.weight)


def instance_norm(
    x: torch.Tensor,
    gamma: torch.Tensor,
    beta: torch.Tensor,
    eps: float = EPS_DEFAULT,
    act: Optional[str] = None,
    slope: float = 0.2,
    residual: Optional[torch.Tensor] = None,
    fp8_consumer: Optional[Fp8Consumer] = None,
) -> torch.Tensor:
    """``fp8_consumer`` names the conv that reads the result. In fp8 mode
    on the HIP path the result then carries that conv's e4m3 operand
    (FP8_TWIN_ATTR); everywhere else the hint is ignored."""
    a = _ACT[act]
    if backend.use_hip(x, gamma):
        psum, psq = _slabs_for(x)
        slots = _twin_slots(x, fp8_consumer)
        if slots is not None:
            y, yq = _InstNormFn.apply(x, gamma, beta, eps, a, slope, residual,
                                      psum, psq, slots[0], slots[1])
            setattr(y, FP8_TWIN_ATTR, (yq, slots[0]))
            return y
        return _InstNormFn.apply(x, gamma, beta, eps, a, slope, residual,
                                 psum, psq)
    return _in_ref(x, gamma, beta, eps, a, slope, residual)
