"""Shapes, inputs, oracle and bounds shared by the SSIM tests.

Bounds (they come from the formats and from the fp32 reference's own
error, never from what the kernels return):

forward, per case:   |kernel - fp64| <= max(8 * e32, 2^-20)
    e32 is the error of the fp32 torch reference on the CPU against the
    fp64 one on the same bf16-rounded inputs (max over the batch). The
    factor 8 covers another summation order over the 121 taps and fma
    contraction; the floor covers cases where the fp32 reference happens
    to land exactly. Measured e32 on the kinds and shapes below: 3.9e-6 on
    the nearly flat kind (E[x^2] - mx^2 cancels), below 1e-7 on the others
    (table in tests/test_ssim_gpu.py).

gradient, per element: |kernel - g| <= 2^-8 |g| + 8 * e32g + 2^-30
    g is the fp64 gradient, 2^-8 the relative error of the kernel's
    round-to-nearest bf16 store (8 significand bits), e32g the largest
    element error of the fp32 reference's gradient in that case.
"""

import torch
import torch.nn.functional as F

from cyclegan_amd.ops import ssim as S

# the kernels' tile of windows (forward) / pixels (backward)
TH = TW = 16

SHAPES = (
    (1, 11, 11, 3),            # one window
    (2, 12, 13, 3),
    (1, 11, 40, 1),            # one-row grid
    (1, 40, 11, 1),            # one-column grid
    (1, TH - 1 + 10, TW + 1 + 10, 3),   # grids of TH-1 / TH / TH+1 rows
    (1, TH + 10, TW - 1 + 10, 1),       # against TW+1 / TW-1 / TW columns
    (1, TH + 1 + 10, TW + 10, 3),
    (2, 37, 45, 3),            # crosses tile edges both ways
    (3, 64, 64, 3),
)
BIG_SHAPE = (1, 256, 256, 3)   # run once
KINDS = ("noise", "lowpass", "flat", "near", "same", "saturated")
DOUT = (0.5, -2.0, 1.0)

U16 = 2.0 ** -8


def _bf16(t):
    return t.to(torch.bfloat16).float()


def make_pair(shape, kind, seed=0):
    """x, y as fp32 tensors holding bf16-representable values."""
    g = torch.Generator().manual_seed(1000 + seed)
    n1 = torch.rand(shape, generator=g) * 2 - 1
    n2 = torch.rand(shape, generator=g) * 2 - 1
    if kind == "noise":
        x, y = n1, n2
    elif kind == "lowpass":
        def lp(n):
            p = n.permute(0, 3, 1, 2)
            p = F.avg_pool2d(p, 5, stride=1, padding=2,
                             count_include_pad=False)
            return (2.0 * p).clamp(-1, 1).permute(0, 2, 3, 1).contiguous()
        x, y = lp(n1), lp(0.5 * n1 + 0.5 * n2)
    elif kind == "flat":
        x, y = 0.5 + 0.01 * n1, 0.5 + 0.01 * n2
    elif kind == "near":
        x = n1
        y = _bf16(x) + 0.004 * n2
    elif kind == "same":
        x = y = n1
    elif kind == "saturated":
        x = torch.where(n1 >= 0, 1.0, -1.0)
        y = torch.where(n2 >= 0, 1.0, -1.0)
    else:
        raise KeyError(kind)
    return _bf16(x).contiguous(), _bf16(y).contiguous()


def dout_for(b):
    return torch.tensor(DOUT[:b], dtype=torch.float64)


def fwd_bound(e32: float) -> float:
    return max(8.0 * e32, 2.0 ** -20)


def grad_bound(g64: torch.Tensor, e32g: float) -> torch.Tensor:
    return U16 * g64.abs() + 8.0 * e32g + 2.0 ** -30


def _ref_with_grads(x, y, dout, dtype):
    x = x.detach().clone().to(dtype).requires_grad_(True)
    y = y.detach().clone().to(dtype).requires_grad_(True)
    out = S._ssim_ref(x, y)
    gx, gy = torch.autograd.grad((out * dout.to(dtype)).sum(), (x, y))
    return out.detach().double(), gx.double(), gy.double()


_oracles = {}


def oracle(shape, kind):
    """fp64 and fp32 references of a case, computed once and shared."""
    key = (tuple(shape), kind)
    if key not in _oracles:
        x, y = make_pair(shape, kind)
        dout = dout_for(shape[0])
        o64, gx64, gy64 = _ref_with_grads(x, y, dout, torch.float64)
        o32, gx32, gy32 = _ref_with_grads(x, y, dout, torch.float32)
        _oracles[key] = dict(
            x=x, y=y, dout=dout, out=o64, gx=gx64, gy=gy64, out32=o32,
            e32=(o32 - o64).abs().max().item(),
            e32gx=(gx32 - gx64).abs().max().item(),
            e32gy=(gy32 - gy64).abs().max().item())
    return _oracles[key]


# ---- an independent definition, and wrong variants of it ----

def window64(taps=11, normalise=True):
    d = torch.arange(taps, dtype=torch.float64) - (taps - 1) / 2
    g = torch.exp(-d * d / (2 * 1.5 * 1.5))
    return g / g.sum() if normalise else g


def ssim_bruteforce(x, y):
    """fp64, straight from the definition: explicit loops over samples,
    channels, windows and taps; no convolution call."""
    x, y = x.double(), y.double()
    b, h, w, c = x.shape
    g = window64().tolist()
    c1, c2 = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2
    out = []
    for n in range(b):
        total, count = 0.0, 0
        for ch in range(c):
            xs, ys = x[n, :, :, ch].tolist(), y[n, :, :, ch].tolist()
            for i in range(h - 10):
                for j in range(w - 10):
                    mx = my = qx = qy = p = 0.0
                    for u in range(11):
                        for v in range(11):
                            wt = g[u] * g[v]
                            xv, yv = xs[i + u][j + v], ys[i + u][j + v]
                            mx += wt * xv
                            my += wt * yv
                            qx += wt * xv * xv
                            qy += wt * yv * yv
                            p += wt * xv * yv
                    vx, vy, cov = qx - mx * mx, qy - my * my, p - mx * my
                    total += ((2 * mx * my + c1) * (2 * cov + c2)
                              / ((mx * mx + my * my + c1) * (vx + vy + c2)))
                    count += 1
        out.append(total / count)
    return torch.tensor(out, dtype=torch.float64)


def ssim_variant(x, y, variant):
    """fp64 SSIM with one deliberate mistake (or none: 'right')."""
    x, y = x.double(), y.double()
    b = x.shape[0]
    taps, norm, max_val, same = 11, True, 2.0, False
    if variant == "unnormalised":
        norm = False
    elif variant == "taps10":
        taps = 10
    elif variant == "maxval1":
        max_val = 1.0
    elif variant == "same":
        same = True
    elif variant != "right":
        raise KeyError(variant)
    g = window64(taps, norm)
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    px, py = S._planes(x), S._planes(y)
    pad = (taps // 2, (taps - 1) // 2) if same else (0, 0)

    def blur(t):
        t = F.pad(t, pad + pad)
        t = F.conv2d(t, g.view(1, 1, 1, taps))
        return F.conv2d(t, g.view(1, 1, taps, 1))

    mx, my = blur(px), blur(py)
    vx, vy = blur(px * px) - mx * mx, blur(py * py) - my * my
    cov = blur(px * py) - mx * my
    s = ((2 * mx * my + c1) * (2 * cov + c2)
         / ((mx * mx + my * my + c1) * (vx + vy + c2)))
    return s.reshape(b, -1).mean(dim=1)


WRONG_VARIANTS = ("unnormalised", "taps10", "maxval1", "same")
