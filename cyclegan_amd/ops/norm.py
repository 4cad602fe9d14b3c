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

from . import backend
from .conv import ACT_NONE, ACT_RELU, ACT_LRELU, IN_SLABS_ATTR, _ACT

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
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, act, slope, residual, psum, psq):
        ext = backend.ext()
        betaf = beta.float()
        if psum is not None:
            y, mean, rstd = ext.instnorm_fwd(x, gamma.float(), betaf, eps, act,
                                             slope, residual, psum, psq,
                                             psum.shape[0])
        else:
            y, mean, rstd = ext.instnorm_fwd(x, gamma.float(), betaf, eps, act,
                                             slope, residual)
        ctx.save_for_backward(x, gamma, mean, rstd, y, betaf)
        ctx.conf = (eps, act, slope, residual is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd, y, betaf = ctx.saved_tensors
        eps, act, slope, has_res = ctx.conf
        ext = backend.ext()
        dy = dy.contiguous()
        if has_res and act != ACT_NONE:
            # rare combo: residual grad needs the transformed dy explicitly
            dy = ext.act_bwd(dy, y, act, slope)
            dres = dy
            dx, dgamma, dbeta = ext.instnorm_bwd(dy, x, gamma.float(), mean,
                                                 rstd, None, ACT_NONE, 0.0)
        else:
            dres = dy if has_res else None
            yact = y if (act != ACT_NONE and not _mask_from_x(act)) else None
            dx, dgamma, dbeta = ext.instnorm_bwd(
                dy, x, gamma.float(), mean, rstd, yact, act, slope, betaf)
        return (dx, dgamma.to(gamma.dtype), dbeta, None, None, None, dres,
                None, None)


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


def instance_norm(
    x: torch.Tensor,
    gamma: torch.Tensor,
    beta: torch.Tensor,
    eps: float = EPS_DEFAULT,
    act: Optional[str] = None,
    slope: float = 0.2,
    residual: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    a = _ACT[act]
    if backend.use_hip(x, gamma):
        psum, psq = _slabs_for(x)
        return _InstNormFn.apply(x, gamma, beta, eps, a, slope, residual,
                                 psum, psq)
    return _in_ref(x, gamma, beta, eps, a, slope, residual)
