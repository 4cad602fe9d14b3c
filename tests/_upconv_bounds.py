"""fp64 references and derived bounds for the resize-convolution
(ops.upsample_conv2d), shared by tests/test_upconv_cpu.py and
tests/test_upconv_gpu.py. A plain helper module like _kernel_bounds.

The op is nearest-2x upsampling + zero-padded 3x3 conv. The HIP path runs
it as a 4x4 stride-2 'SAME' transpose conv (pt = pl = 1) whose kernel is
the fold V = M w M^T of the 3x3 master w on both axes. Everything here is
written from that definition and from F.conv2d on the explicitly
upsampled image, not through the project's fold code.

Folded-weight error. The arena computes V in fp32 from the fp32 masters
(at most 4 terms per element, any order within (4-1)*u32*A <= 4*u32*A of
the exact sum, A = M|w|M^T) and rounds once to bf16 (u16 of the rounded
value), so every element of the bf16 form is within

    dV = u16 * (|V64| + 4*u32*A) + 4*u32*A

of V64 = M w M^T taken in fp64 from the fp32 masters.
"""

import torch
import torch.nn.functional as F

from _kernel_bounds import (Case, U16, U32, apply_act, convt_fwd_lin,
                            dgrad_ref_bound, fwd_ref_bound, wgrad_ref_bound)

M = torch.tensor([[0, 0, 1], [0, 1, 1], [1, 1, 0], [1, 0, 0]],
                 dtype=torch.float64)

# (B, H, W, Cin, Cout) of the GPU cases, and what each reaches
GPU_SHAPES = {
    "nsq": (2, 5, 12, 128, 64),       # phase tiles with an M tail
    "cin96": (1, 6, 10, 96, 96),      # Cin % 64 != 0
    "ntile": (2, 4, 6, 64, 24),       # partial n-tile (the smallest)
    "bn128": (1, 8, 8, 64, 128),      # 128-wide tile
}


def up_case(name, shape) -> Case:
    B, H, W, Cin, Cout = shape
    return Case(name, "convt", B, H, W, Cin, Cout, 4, 4, 2, "same", False, "")


def master(shape, seed, scale=0.2):
    """An fp32 master weight (not bf16-representable on purpose)."""
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g) * 2 - 1) * scale).float()


def fold(w, m=M):
    """V[o,k,l,i] = sum_de m[k,d] m[l,e] w[o,d,e,i], in w's dtype."""
    m = m.to(w.dtype)
    return torch.einsum("kd,odei,le->okli", m, w, m)


def unfold(dv, m=M):
    """The adjoint: dw[o,d,e,i] = sum_kl m[k,d] m[l,e] dv[o,k,l,i]."""
    m = m.to(dv.dtype)
    return torch.einsum("kd,okli,le->odei", m, dv, m)


def delta_v(w32):
    w64 = w32.to(torch.float64)
    v64, a = fold(w64), fold(w64.abs())
    return v64, U16 * (v64.abs() + 4 * U32 * a) + 4 * U32 * a


def naive_fwd(x, w, bias=None):
    """The definition: repeat every pixel 2x2, zero-pad by 1, 3x3 conv."""
    xn = x.permute(0, 3, 1, 2)
    xn = xn.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    y = F.conv2d(F.pad(xn, (1, 1, 1, 1)), w.permute(0, 3, 1, 2), bias)
    return y.permute(0, 2, 3, 1)


def naive_grads(x, w, dy):
    """(dx, dw) of naive_fwd at dy, in the dtype of x and w."""
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    return torch.autograd.grad(naive_fwd(x, w), (x, w), dy.to(x.dtype))


def convt_up(x, v):
    """The folded formulation in the dtype of its arguments."""
    return convt_fwd_lin(x, v, None, 2, 1, 1, 2 * x.shape[1], 2 * x.shape[2])


def convt_up_adjoint(dy, v, x_shape):
    leaf = torch.zeros(x_shape, dtype=v.dtype, requires_grad=True)
    (g,) = torch.autograd.grad(convt_up(leaf, v), leaf, dy.to(v.dtype))
    return g


def fwd_bound(case, x, w32, vb, act=None):
    """Reference (fp64 naive, from the bf16 x and the fp32 master) and
    bound for the op's forward, vb the bf16 folded form it used.

    The kernel is within fwd_ref_bound's bound of the exact transpose conv
    with vb; that differs from the exact one with V64 by at most
    convt(|x|, |vb - V64|) <= convt(|x|, dV), which by the identity is the
    naive reference. The activations are 1-Lipschitz. (1 + u16) covers the
    final rounding of the part of the value that the weight error adds."""
    d = torch.float64
    ref = apply_act(naive_fwd(x.to(d), w32.to(d)), act)
    _, b0 = fwd_ref_bound(case, x, vb, None, act)
    _, dv = delta_v(w32)
    return ref, b0 + (1 + U16) * convt_up(x.to(d).abs(), dv)


def dgrad_bound(case, dy, w32, vb):
    d = torch.float64
    x0 = torch.zeros(case.x_shape, dtype=d)
    ref, _ = naive_grads(x0, w32.to(d), dy.to(d))
    _, b0 = dgrad_ref_bound(case, dy, vb)
    _, dv = delta_v(w32)
    return ref, b0 + (1 + U16) * convt_up_adjoint(dy.to(d).abs(), dv,
                                                  case.x_shape)


def dw_bound(case, x, dy):
    """dw reference (fp64 naive) and bound. The wgrad kernel gives the 4x4
    dV within bound_dV = wgrad_ref_bound's bound; the unfold adds at most
    four of them per element in fp32:

        bound = fold(bound_dV) + 4*u32 * fold(|dV_ref| + bound_dV),

    fold here the adjoint M^T . M applied to magnitudes."""
    d = torch.float64
    w0 = torch.zeros(case.Cout, 3, 3, case.Cin, dtype=d)
    _, ref = naive_grads(x.to(d), w0, dy.to(d))
    dv_ref, b_dv = wgrad_ref_bound(case, x, dy)
    return ref, unfold(b_dv) + 4 * U32 * unfold(dv_ref.abs() + b_dv), dv_ref, b_dv
