"""Per-sample structural similarity (SSIM) with a backward pass.

``SSIM(y_true, y_pred) -> [B]`` fp32 for NHWC images on [-1, 1], reduced
like ``ops.MAE``. The semantics are those of ``tf.image.ssim(a, b,
max_val=2.0)``: an 11x11 Gaussian window (sigma 1.5, normalised to sum 1),
VALID placement, so an HxW image has an (H-10)x(W-10) grid of windows;
per channel and window

    S = (2 mx my + c1)(2 sxy + c2) / ((mx^2 + my^2 + c1)(sx^2 + sy^2 + c2))

with c1 = (0.01*2)^2, c2 = (0.03*2)^2; out[b] is the mean of S over all
windows and channels. Not in the reference: it feeds the optional
``--cycle_ssim`` loss term and the ``--test_ssim`` metric.

On the GPU both directions are HIP kernels (_hip/ssim.hip). The forward
saves the derivatives of S by the windows' raw moments; the backward
applies the adjoint of the blur to them (``ssim_grad_from_maps`` is the
same formula in torch). The torch implementation below is the CPU path and
the kernels' oracle.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from . import backend

WIN = 11
SIGMA = 1.5
MAX_VAL = 2.0
C1 = (0.01 * MAX_VAL) ** 2
C2 = (0.03 * MAX_VAL) ** 2


def gaussian_window(dtype=torch.float32, device=None) -> torch.Tensor:
    """The 11 taps of one axis, computed in fp64 and normalised to sum 1."""
    d = torch.arange(WIN, dtype=torch.float64) - (WIN - 1) / 2
    g = torch.exp(-d * d / (2.0 * SIGMA * SIGMA))
    return (g / g.sum()).to(dtype=dtype, device=device)


def _check(y_true: torch.Tensor, y_pred: torch.Tensor):
    if y_true.dim() != 4 or y_true.shape != y_pred.shape:
        raise ValueError(
            f"SSIM: inputs must be [B,H,W,C] of one shape, got "
            f"{tuple(y_true.shape)} and {tuple(y_pred.shape)}")
    if y_true.shape[1] < WIN or y_true.shape[2] < WIN:
        raise ValueError(
            f"SSIM: H and W must be at least {WIN} (one window), got "
            f"{y_true.shape[1]}x{y_true.shape[2]}")


def _planes(t: torch.Tensor) -> torch.Tensor:
    """[B,H,W,C] -> [B*C,1,H,W]: every channel is filtered on its own."""
    b, h, w, c = t.shape
    return t.permute(0, 3, 1, 2).reshape(b * c, 1, h, w)


def _blur(p: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """VALID separable Gaussian blur of [N,1,H,W] planes."""
    p = F.conv2d(p, g.view(1, 1, 1, WIN))
    return F.conv2d(p, g.view(1, 1, WIN, 1))


def _blur_adjoint(p: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """Adjoint of ``_blur``: full-mode correlation, zero outside the grid."""
    p = F.conv_transpose2d(p, g.view(1, 1, WIN, 1))
    return F.conv_transpose2d(p, g.view(1, 1, 1, WIN))


def _moments(x: torch.Tensor, y: torch.Tensor):
    g = gaussian_window(x.dtype, x.device)
    n = x.shape[0]
    m = _blur(torch.cat([x, y, x * x, y * y, x * y]), g)
    return g, m.split(n)


def _work_dtype(t: torch.Tensor) -> torch.dtype:
    return torch.float64 if t.dtype == torch.float64 else torch.float32


def _ssim_ref(y_true: torch.Tensor, y_pred: torch.Tensor) -> torch.Tensor:
    """Pure torch: depthwise conv2d moments, autograd for the backward.
    Computes in fp64 for fp64 inputs (the oracle of the tests), else fp32."""
    dt = _work_dtype(y_true)
    b = y_true.shape[0]
    x, y = _planes(y_true.to(dt)), _planes(y_pred.to(dt))
    _, (mx, my, qx, qy, p) = _moments(x, y)
    mxy = mx * my
    a1 = 2.0 * mxy + C1
    b1 = mx * mx + my * my + C1
    a2 = 2.0 * (p - mxy) + C2
    b2 = (qx - mx * mx) + (qy - my * my) + C2
    s = (a1 / b1) * (a2 / b2)
    return s.reshape(b, -1).mean(dim=1)


def ssim_grad_from_maps(y_true: torch.Tensor, y_pred: torch.Tensor,
                        dout: torch.Tensor) -> torch.Tensor:
    """The gradient by ``y_pred`` of ``(dout * SSIM(y_true, y_pred)).sum()``
    by the formula the backward kernel implements, in torch:

        dL/dy_j = dout[b]/N * [(G^T a)_j + 2 y_j (G^T b)_j + x_j (G^T c)_j]

    with a = dS/dE[y], b = dS/dE[y^2], c = dS/dE[xy] (the raw moments taken
    as independent variables), G^T the adjoint of the VALID blur and N the
    number of windows times channels. The gradient by ``y_true`` is the
    same call with the images swapped (SSIM is symmetric)."""
    dt = _work_dtype(y_true)
    bsz, h, w, ch = y_true.shape
    x, y = _planes(y_true.to(dt)), _planes(y_pred.to(dt))
    g, (mx, my, qx, qy, p) = _moments(x, y)
    mxy = mx * my
    a1 = 2.0 * mxy + C1
    b1 = mx * mx + my * my + C1
    a2 = 2.0 * (p - mxy) + C2
    b2 = (qx - mx * mx) + (qy - my * my) + C2
    r1 = a1 / b1
    s = r1 * (a2 / b2)
    am = 2.0 * (mx * (a2 - a1) - my * s * (b2 - b1)) / (b1 * b2)
    bm = -s / b2
    cm = 2.0 * r1 / b2
    grad = (_blur_adjoint(am, g) + 2.0 * y * _blur_adjoint(bm, g)
            + x * _blur_adjoint(cm, g))
    n = (h - WIN + 1) * (w - WIN + 1) * ch
    grad = grad.reshape(bsz, ch, h, w).permute(0, 2, 3, 1)
    return grad * (dout.to(dt) / n).view(bsz, 1, 1, 1)


class _SSIMFn(torch.autograd.Function):
    """out[b] = mean SSIM of sample b, fp32; HIP kernels both ways."""

    @staticmethod
    def forward(ctx, y_true, y_pred, save_maps):
        res = backend.ext().ssim_fwd(y_true, y_pred, save_maps)
        ctx.save_for_backward(y_true, y_pred, *res[1:])
        return res[0]

    @staticmethod
    def backward(ctx, dout):
        y_true, y_pred, *maps = ctx.saved_tensors
        ext = backend.ext()
        dout = dout.contiguous().float()
        gt = gp = None
        if ctx.needs_input_grad[1]:
            gp = ext.ssim_bwd(y_true, y_pred, maps[0], maps[1], maps[2], dout)
        if ctx.needs_input_grad[0]:
            # symmetric: the same kernel, images swapped, its own dS/dE[x]
            gt = ext.ssim_bwd(y_pred, y_true, maps[3], maps[1], maps[2], dout)
        return gt, gp, None


def _save_maps(y_true: torch.Tensor, y_pred: torch.Tensor) -> int:
    """Which coefficient maps the forward writes: 0 none, 1 those for
    y_pred's gradient, 2 also y_true's. Decided here, before apply: inside
    a Function's forward the grad mode is already off and needs_input_grad
    is requires_grad alone, which ignores an enclosing no_grad()."""
    if not torch.is_grad_enabled():
        return 0  # the test epoch
    if y_true.requires_grad:
        return 2
    return 1 if y_pred.requires_grad else 0


def SSIM(y_true: torch.Tensor, y_pred: torch.Tensor) -> torch.Tensor:
    """Per-sample mean SSIM of NHWC images on [-1, 1], shape [B] fp32
    (fp64 for fp64 inputs on the torch path)."""
    _check(y_true, y_pred)
    if backend.use_hip(y_true, y_pred):
        return _SSIMFn.apply(y_true, y_pred, _save_maps(y_true, y_pred))
    return _ssim_ref(y_true, y_pred)
