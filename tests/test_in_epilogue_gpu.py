"""InstanceNorm statistics from the conv epilogue, IN backward without the
activated-output read, and the vectorised reflect pad.

Shapes are the smallest that still reach every path: 2 M-tiles per sample
(slice index + per-sample boundary), 64- and 128-wide n-tiles, two
n-tiles, a strided conv, the phased convT (eligible and not), an odd
sample count (XCD-chunked tile remap) and a 144-row sample that must fall
back to the separate reduce pass.

All tests @pytest.mark.gpu.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cyclegan_amd import ops
from cyclegan_amd.ops import backend
from cyclegan_amd.ops.conv import (IN_SLABS_ATTR, _ACT, _conv_ref, _convt_ref,
                                   same_pads)
from cyclegan_amd.ops.norm import _in_ref

DEV = "cuda:0"


def mk(shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand(shape, generator=g) * 2 - 1) * scale
    return t.to(DEV, torch.bfloat16)


def check_elem(got, ref, rtol, name=""):
    """Per-element |err| <= rtol * (|ref| + rms(ref)) — the bound form of
    tests/test_ops_gpu_fullshape.py."""
    got = got.float()
    ref = ref.float()
    assert got.shape == ref.shape, f"{name}: {got.shape} vs {ref.shape}"
    rms = ref.pow(2).mean().sqrt()
    bound = rtol * (ref.abs() + rms)
    err = (got - ref).abs()
    bad = (err > bound).sum().item()
    worst = (err / bound.clamp(min=1e-30)).max().item()
    print(f"{name}: worst err/bound {worst:.3f}")
    assert bad == 0, f"{name}: {bad}/{ref.numel()} elements out of bound, worst ratio {worst:.2f}"


# ---------------------------------------------------------------- slabs ----
# name, kind, B, H, W, Cin, Cout, K, stride, padding, pad_mode, eligible
STAT_CASES = [
    ("s1_c64",    "conv",  2, 16, 16,  64,  64, 3, 1, (1, 1, 1, 1), "reflect", True),
    ("s1_c128",   "conv",  2, 16, 16,  64, 128, 3, 1, (1, 1, 1, 1), "reflect", True),
    ("s1_c256",   "conv",  2, 16, 16,  64, 256, 3, 1, (1, 1, 1, 1), "reflect", True),
    ("s1_c128_b3", "conv", 3, 16, 16,  64, 128, 3, 1, (1, 1, 1, 1), "reflect", True),
    ("s1_c64_b3", "conv",  3, 16, 16,  64,  64, 3, 1, (1, 1, 1, 1), "reflect", True),
    ("s2_same",   "conv",  2, 32, 32,  64, 128, 3, 2, "same",       "zeros",   True),
    # phased convT: one parity class of a sample has (OH/2)*(OW/2) rows.
    # 8x8 -> 16x16 gives 64 (< one 128-row tile): not eligible.
    ("ct_8to16",  "convt", 2,  8,  8, 128,  64, 3, 2, None, None, False),
    ("ct_16to32", "convt", 2, 16, 16, 128,  64, 3, 2, None, None, True),
    ("ct_16to32_c128_b3", "convt", 3, 16, 16, 128, 128, 3, 2, None, None, True),
    # 12x12 output: 144 rows per sample, tiles straddle samples
    ("s1_12x12",  "conv",  2, 12, 12,  64,  64, 3, 1, (1, 1, 1, 1), "reflect", False),
]


def _run_stats(case):
    name, kind, b_, H, W, Cin, Cout, K, s, padding, pm, elig = case
    ext = backend.ext()
    x = mk((b_, H, W, Cin), seed=201)
    w = mk((Cout, K, K, Cin), seed=202, scale=0.2)
    if kind == "conv":
        pads = same_pads(H, W, K, K, s) if padding == "same" else tuple(padding)
        out = ext.conv2d_fwd_stats(x, w, None, s, *pads, pm == "reflect", 0, 0.2)
        plain = ext.conv2d_fwd(x, w, None, s, *pads, pm == "reflect", 0, 0.2)
    else:
        pt, _, pl, _ = same_pads(H * s, W * s, K, K, s)
        out = ext.convt2d_fwd_stats(x, w, None, s, pt, pl, H * s, W * s, 0, 0.2)
        plain = ext.convt2d_fwd(x, w, None, s, pt, pl, H * s, W * s, 0, 0.2)
    return out, plain


@pytest.mark.parametrize("case", STAT_CASES, ids=[c[0] for c in STAT_CASES])
def test_epilogue_slabs_match_tensor(case):
    """Slabs summed over slices == per-(b,c) sum / sum of squares of the
    returned bf16 tensor.

    Bound. The slabs add the same n = OH*OW values v (already rounded to
    bf16, converted back exactly) as the reference, only in another order.
    An fp32 sum of n terms in any order is within (n-1)*u*sum|v| of the
    exact sum (u = 2^-24, first order); each square v*v carries one more
    rounding (relative u). Kernel and torch reference each contribute one
    such error, so |slab - ref| <= 2*n*u*sum|v| for the sums and
    <= 2*n*u*sum(v^2) for the squares."""
    elig = case[-1]
    out, plain = _run_stats(case)
    y = out[0]
    # asking for slabs must not change the tensor itself
    assert torch.equal(y, plain)
    if not elig:
        assert len(out) == 1, "ineligible shape must not emit slabs"
        return
    assert len(out) == 3, "eligible shape must emit slabs"
    psum, psq = out[1], out[2]
    b_, OH, OW, C = y.shape
    assert psum.shape == psq.shape and tuple(psum.shape[1:]) == (b_, C)
    assert psum.shape[0] == OH * OW // 128
    n = OH * OW
    u = 2.0 ** -24
    yf = y.float()
    ref_s = yf.sum((1, 2))
    ref_q = (yf ** 2).sum((1, 2))
    abs_s = yf.abs().sum((1, 2))
    got_s = psum.sum(0)
    got_q = psq.sum(0)
    # the final add over slices is one more fp32 sum of NS terms of the same
    # values: covered by the (n-1) term count (NS partial sums regroup the
    # same n terms)
    err_s = ((got_s - ref_s).abs() / (2 * n * u * abs_s)).max().item()
    err_q = ((got_q - ref_q).abs() / (2 * n * u * ref_q)).max().item()
    print(f"{case[0]}: sum err/bound {err_s:.3f}, sumsq err/bound {err_q:.3f}")
    assert err_s <= 1.0 and err_q <= 1.0
    # run-to-run deterministic (no atomics)
    out2, _ = _run_stats(case)
    assert torch.equal(out2[1], psum) and torch.equal(out2[2], psq)


# ------------------------------------------------- conv -> IN -> loss ----
CHAIN_CASES = [c for c in STAT_CASES]
CHAIN_ACTS = [("relu", False), (None, True), ("lrelu", False)]


@pytest.mark.parametrize("actres", CHAIN_ACTS,
                         ids=["relu", "none_res", "lrelu"])
@pytest.mark.parametrize("case", CHAIN_CASES, ids=[c[0] for c in CHAIN_CASES])
def test_conv_in_chain_fwd_bwd(case, actres):
    """ops.conv2d / conv_transpose2d + ops.instance_norm (the hand-off
    plumbing) against _conv_ref/_convt_ref + _in_ref in fp32.

    The reference keeps the pipeline's one storage point: the conv output
    is a bf16 tensor, so it is rounded to bf16 before _in_ref (which then
    computes in fp32). Without that rounding the reference would normalise
    a different tensor than the one the op is defined on, and relu masks
    would legitimately differ wherever |pre-activation| is below the bf16
    rounding of the conv output."""
    name, kind, b_, H, W, Cin, Cout, K, s, padding, pm, elig = case
    act, use_res = actres
    x = mk((b_, H, W, Cin), seed=211)
    w32 = mk((Cout, K, K, Cin), seed=212, scale=0.2).float()
    g32 = (torch.randn(Cout, generator=torch.Generator().manual_seed(213)) * 0.5).to(DEV)
    b32 = (torch.randn(Cout, generator=torch.Generator().manual_seed(214)) * 0.1).to(DEV)

    xg = x.clone().requires_grad_(True)
    wg = w32.clone().requires_grad_(True)
    gg = g32.clone().requires_grad_(True)
    bg = b32.clone().requires_grad_(True)
    if kind == "conv":
        h = ops.conv2d(xg, wg, None, s, padding, pm)
    else:
        h = ops.conv_transpose2d(xg, wg, stride=s)
    assert (getattr(h, IN_SLABS_ATTR, None) is not None) == elig
    res = mk(h.shape, seed=215) if use_res else None
    y = ops.instance_norm(h, gg, bg, act=act, residual=res)
    dy = mk(y.shape, seed=216)
    y.backward(dy)

    xr = x.float().requires_grad_(True)
    wr = w32.clone().requires_grad_(True)
    gr = g32.clone().requires_grad_(True)
    br = b32.clone().requires_grad_(True)
    if kind == "conv":
        pads = same_pads(H, W, K, K, s) if padding == "same" else tuple(padding)
        hr = _conv_ref(xr, wr, None, s, pads, pm)
    else:
        pt, _, pl, _ = same_pads(H * s, W * s, K, K, s)
        hr = _convt_ref(xr, wr, None, s, pt, pl, H * s, W * s)
    hr = hr.to(torch.bfloat16)
    yr = _in_ref(hr, gr, br, 1e-3, _ACT[act], 0.2, res)
    yr.backward(dy)

    check_elem(y, yr, 0.04, f"{name}:{act}:y")
    check_elem(xg.grad, xr.grad, 0.06, f"{name}:{act}:dx")
    check_elem(wg.grad, wr.grad, 0.05, f"{name}:{act}:dw")
    check_elem(gg.grad, gr.grad, 0.05, f"{name}:{act}:dgamma")
    check_elem(bg.grad, br.grad, 0.05, f"{name}:{act}:dbeta")


def test_slabs_path_equals_reduce_path():
    """The normalise pass fed by epilogue slabs vs by in_reduce on the same
    tensor. The statistics differ only by fp32 summation order (bounded in
    test_epilogue_slabs_match_tensor, ~1e-5 relative), which can move an
    output across at most one bf16 rounding boundary: one bf16 ulp,
    2^-7 relative at worst."""
    ext = backend.ext()
    out, _ = _run_stats(STAT_CASES[2])
    h, psum, psq = out
    C = h.shape[3]
    g = (torch.randn(C, generator=torch.Generator().manual_seed(3)) * 0.5).to(DEV)
    b = (torch.randn(C, generator=torch.Generator().manual_seed(4)) * 0.1).to(DEV)
    y0, m0, r0 = ext.instnorm_fwd(h, g, b, 1e-3, 1, 0.2, None)
    y1, m1, r1 = ext.instnorm_fwd(h, g, b, 1e-3, 1, 0.2, None, psum, psq,
                                  psum.shape[0])
    check_elem(y1, y0, 2.0 ** -7, "slabs-vs-reduce:y")
    check_elem(m1, m0, 2.0 ** -7, "slabs-vs-reduce:mean")
    check_elem(r1, r0, 2.0 ** -7, "slabs-vs-reduce:rstd")


# ------------------------------------------------------ mask recompute ----
@pytest.mark.parametrize("beta_std", [0.0, 0.1], ids=["beta0", "beta0.1"])
@pytest.mark.parametrize("act", ["relu", "lrelu"])
@pytest.mark.parametrize("C", [64, 256])
def test_in_bwd_mask_recompute_equals_yact(C, act, beta_std):
    """instnorm_bwd with yact and without (mask from x) on the same inputs:
    dx equal element for element; dgamma/dbeta pass through atomics."""
    ext = backend.ext()
    a = _ACT[act]
    x = mk((2, 16, 16, C), seed=221)
    gen = torch.Generator().manual_seed(222)
    g = (torch.randn(C, generator=gen) * 0.02).to(DEV)
    b = (torch.randn(C, generator=gen) * beta_std).to(DEV)
    y, mean, rstd = ext.instnorm_fwd(x, g, b, 1e-3, a, 0.2, None)
    dy = mk(y.shape, seed=223)
    dx0, dg0, db0 = ext.instnorm_bwd(dy, x, g, mean, rstd, y, a, 0.2)
    dx1, dg1, db1 = ext.instnorm_bwd(dy, x, g, mean, rstd, None, a, 0.2, b)
    ndiff = (dx0 != dx1).sum().item()
    print(f"C={C} {act} beta_std={beta_std}: {ndiff} differing dx elements")
    assert torch.equal(dx0, dx1)
    check_elem(dg1, dg0, 0.05, "dgamma")
    check_elem(db1, db0, 0.05, "dbeta")


def test_in_bwd_without_yact_needs_beta():
    ext = backend.ext()
    x = mk((1, 16, 16, 64), seed=1)
    g = torch.ones(64, device=DEV)
    y, mean, rstd = ext.instnorm_fwd(x, g, torch.zeros_like(g), 1e-3, 1, 0.2, None)
    with pytest.raises(RuntimeError):
        ext.instnorm_bwd(y, x, g, mean, rstd, None, 1, 0.2)


# ----------------------------------------------------------------- pad ----
@pytest.mark.parametrize("pads", [(3, 3, 3, 5), (1, 1, 1, 1)])
@pytest.mark.parametrize("C", [8, 64, 3])
def test_reflect_pad_fwd_exact(C, pads):
    """A copy: bit-identical to F.pad(mode='reflect'). C=3 takes the scalar
    kernel, C % 8 == 0 the 16-byte one."""
    ext = backend.ext()
    pt, pb, pl, pr = pads
    x = mk((2, 16, 16, C), seed=231)
    y = ext.reflect_pad_fwd(x, pt, pb, pl, pr)
    ref = F.pad(x.permute(0, 3, 1, 2).float(), (pl, pr, pt, pb),
                mode="reflect").permute(0, 2, 3, 1).to(torch.bfloat16)
    assert y.shape == ref.shape
    assert torch.equal(y, ref.contiguous())
