"""Edge-shape sweep of the conv / convT / dgrad / wgrad kernels against
fp64 references with bounds derived from the arithmetic
(tests/_kernel_bounds.py; tests/test_kernel_bounds_cpu.py shows that the
bounds reject subtly wrong kernels). Every element is checked; nothing is
excluded.

The cases run at the extension level, so the kernels see exactly the bf16
tensors the bounds assume. Each row of the tables in _kernel_bounds is the
smallest shape that reaches the branch its `reaches` column names.

Also here: wgrad determinism (the split-M slabs are atomic-free and must
not depend on what the workspace held before), InstanceNorm on inputs
with a large mean, and InstanceNorm with residual + activation.

All tests @pytest.mark.gpu.
"""

import pytest
import torch

import _kernel_bounds as kb
from cyclegan_amd import ops
from cyclegan_amd.ops import backend

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDS = [c.id for c in kb.ALL_CASES]

_inputs = {}
_refs = {}


def inputs(case):
    """(x, w, bias, dy): bf16 CPU tensors, made once per case."""
    if case.id not in _inputs:
        _inputs[case.id] = kb.make_inputs(case)
    return _inputs[case.id]


def ref(case, what):
    """fp64 reference and bound, computed once and shared."""
    key = (case.id, what)
    if key not in _refs:
        x, w, _, dy = inputs(case)
        _refs[key] = {"fwd": lambda: kb.fwd_ref_bound(case, x, w),
                      "dgrad": lambda: kb.dgrad_ref_bound(case, dy, w),
                      "wgrad": lambda: kb.wgrad_ref_bound(case, x, dy)}[what]()
    return _refs[key]


def dev(t):
    return t.to(DEV).contiguous()


def run_fwd(case, x, w, bias=None, act=None):
    ext = backend.ext()
    a = kb.ACT_ID[act]
    if case.kind == "convt":
        pt, _, pl, _ = case.pads
        return ext.convt2d_fwd(x, w, bias, case.stride, pt, pl, *case.out_hw,
                               a, kb.SLOPE)
    return ext.conv2d_fwd(x, w, bias, case.stride, *case.pads, case.reflect,
                          a, kb.SLOPE)


def run_dgrad(case, dy, w):
    ext = backend.ext()
    wt = w.permute(3, 1, 2, 0).contiguous()      # [Cin,KH,KW,Cout]
    if case.kind == "convt":
        pt, _, pl, _ = case.pads
        return ext.convt2d_dgrad(dy, wt, case.H, case.W, case.stride, pt, pl)
    return ext.conv2d_dgrad(dy, wt, case.H, case.W, case.stride, *case.pads,
                            case.reflect)


def run_wgrad(case, x, dy):
    ext = backend.ext()
    pt, _, pl, _ = case.pads
    if case.kind == "convt":
        # conv wgrad with the roles swapped, then back to OHWI
        dwc = ext.conv2d_wgrad(dy, x, case.KH, case.KW, case.stride, pt, pl,
                               False)
        return dwc.permute(3, 1, 2, 0).contiguous()
    return ext.conv2d_wgrad(x, dy, case.KH, case.KW, case.stride, pt, pl,
                            case.reflect)


# ------------------------------------------------------------ sweep ----
@pytest.mark.parametrize("case", kb.ALL_CASES, ids=IDS)
def test_fwd(case):
    x, w, _, _ = inputs(case)
    y = run_fwd(case, dev(x), dev(w))
    assert tuple(y.shape) == case.y_shape
    kb.assert_within(y, *ref(case, "fwd"), f"{case.id}:y")


@pytest.mark.parametrize("case", kb.ALL_CASES, ids=IDS)
def test_dgrad(case):
    _, w, _, dy = inputs(case)
    dx = run_dgrad(case, dev(dy), dev(w))
    assert tuple(dx.shape) == case.x_shape
    kb.assert_within(dx, *ref(case, "dgrad"), f"{case.id}:dx")


@pytest.mark.parametrize("case", kb.ALL_CASES, ids=IDS)
def test_wgrad(case):
    x, _, _, dy = inputs(case)
    dw = run_wgrad(case, dev(x), dev(dy))
    assert dw.dtype == torch.float32 and tuple(dw.shape) == case.w_shape
    kb.assert_within(dw, *ref(case, "wgrad"), f"{case.id}:dw", "okki")


@pytest.mark.parametrize("cid,act", kb.FWD_ACT_CASES,
                         ids=[f"{c}-{a}" for c, a in kb.FWD_ACT_CASES])
def test_fwd_bias_act(cid, act):
    case = kb.CASE_BY_ID[cid]
    x, w, bias, _ = inputs(case)
    y = run_fwd(case, dev(x), dev(w), dev(bias), act)
    r, bound = kb.fwd_ref_bound(case, x, w, bias, act)
    kb.assert_within(y, r, bound, f"{cid}:bias:{act}:y")


# --------------------------------------------------- ops-level plumbing ----
@pytest.mark.parametrize("cid", ["cin96", "cout20", "s2_odd", "ct_nsq"])
def test_ops_plumbing(cid):
    """ops.conv2d / ops.conv_transpose2d forward + backward with fp32
    master weights that hold bf16 values: the autograd plumbing (shadow
    weights, channel-transposed weight, role-swapped convT wgrad) under the
    same bounds."""
    case = kb.CASE_BY_ID[cid]
    x, w, _, dy = inputs(case)
    xg = dev(x).requires_grad_(True)
    wg = dev(w).float().requires_grad_(True)
    if case.kind == "convt":
        y = ops.conv_transpose2d(xg, wg, stride=case.stride)
    else:
        y = ops.conv2d(xg, wg, None, case.stride, case.pads,
                       "reflect" if case.reflect else "zeros")
    y.backward(dev(dy))
    kb.assert_within(y, *ref(case, "fwd"), f"ops:{cid}:y")
    kb.assert_within(xg.grad, *ref(case, "dgrad"), f"ops:{cid}:dx")
    kb.assert_within(wg.grad, *ref(case, "wgrad"), f"ops:{cid}:dw", "okki")


def test_ops_packed_head_nonsquare(monkeypatch):
    """The 8-pixel-packed generator head (7x7 reflect-3, Cout = 3) on a
    9x24 image: y, dx, dw, db under the bounds of the plain 7x7 conv it
    stands for. The packed GEMM adds structural zeros to the same non-zero
    terms, which adds no rounding error, so K and M are those of the plain
    conv."""
    case = kb.Case("head_nsq", "conv", 1, 9, 24, 64, 3, 7, 7, 1,
                   (3, 3, 3, 3), True, "packed head, H != W")
    x = kb.uniform_bf16(case.x_shape, 31)
    w = kb.uniform_bf16(case.w_shape, 32, 0.2)
    bias = kb.uniform_bf16((3,), 33)
    dy = kb.uniform_bf16(case.y_shape, 34)

    ext = backend.ext()
    seen = []
    real = ext.conv2d_fwd

    def recorder(xa, wa, *rest):
        seen.append(tuple(wa.shape))
        return real(xa, wa, *rest)

    monkeypatch.setattr(ext, "conv2d_fwd", recorder)
    xg = dev(x).requires_grad_(True)
    wg = dev(w).float().requires_grad_(True)
    bg = dev(bias).float().requires_grad_(True)
    y = ops.conv2d(xg, wg, bg, 1, (3, 3, 3, 3), "reflect")
    y.backward(dev(dy))
    assert len(seen) == 1 and seen[0][1:3] == (7, 2), \
        f"packed path did not run: conv2d_fwd weights {seen}"

    kb.assert_within(y, *kb.fwd_ref_bound(case, x, w, bias), "head_nsq:y")
    kb.assert_within(xg.grad, *kb.dgrad_ref_bound(case, dy, w), "head_nsq:dx")
    kb.assert_within(wg.grad, *kb.wgrad_ref_bound(case, x, dy), "head_nsq:dw",
                     "okki")
    kb.assert_within(bg.grad, *kb.dbias_ref_bound(dy), "head_nsq:db", "c")


# ------------------------------------------------------- determinism ----
@pytest.mark.parametrize("cid", ["ow64_short", "s2_odd"])
def test_wgrad_bitwise_deterministic(cid):
    """The split-M slabs are written, not accumulated: the same call gives
    the same bits, also after the allocator's free memory was filled with
    NaN (a slab left unwritten would then show)."""
    case = kb.CASE_BY_ID[cid]
    x, _, _, dy = inputs(case)
    xd, dyd = dev(x), dev(dy)
    a = run_wgrad(case, xd, dyd)
    b = run_wgrad(case, xd, dyd)
    assert torch.equal(a, b)
    junk = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
    junk.view(torch.float32).fill_(float("nan"))
    del junk
    c = run_wgrad(case, xd, dyd)
    assert torch.isfinite(c).all()
    assert torch.equal(a, c)


# ------------------------------------------------------ InstanceNorm ----
@pytest.mark.parametrize("stats", [(4.0, 1.0), (8.0, 0.5)],
                         ids=["mean4_std1", "mean8_std0.5"])
@pytest.mark.parametrize("shape", [(2, 11, 13, 64), (2, 16, 16, 256)],
                         ids=["11x13x64", "16x16x256"])
def test_instnorm_nonzero_mean(shape, stats):
    """var = E[x^2] - mean^2 in fp32 on inputs whose mean dwarfs their
    spread; bounds in _kernel_bounds.in_ref_bounds."""
    mu, sd = stats
    g = torch.Generator().manual_seed(41)
    x = (torch.randn(shape, generator=g) * sd + mu).to(torch.bfloat16)
    gamma = torch.randn(shape[3], generator=g) * 0.5
    beta = torch.randn(shape[3], generator=g) * 0.1
    y, mean, rstd = backend.ext().instnorm_fwd(
        dev(x), dev(gamma), dev(beta), 1e-3, kb.ACT_NONE, kb.SLOPE, None)
    (ry, rm, rr), (by, bm, br), dmax = kb.in_ref_bounds(x, gamma, beta, 1e-3)
    print(f"delta max {dmax:.4f}")
    tag = f"in:{shape[1]}x{shape[2]}x{shape[3]}:m{mu:g}"
    kb.assert_within(mean, rm, bm, f"{tag}:mean", "bc")
    kb.assert_within(rstd, rr, br, f"{tag}:rstd", "bc")
    kb.assert_within(y, ry, by, f"{tag}:y")


def check_elem(got, ref, rtol, name=""):
    """Per-element |err| <= rtol * (|ref| + rms(ref)): the form of
    tests/test_in_epilogue_gpu.py."""
    got = got.detach().to("cpu", torch.float64)
    ref = ref.detach().to(torch.float64)
    assert got.shape == ref.shape, f"{name}: {got.shape} vs {ref.shape}"
    rms = ref.pow(2).mean().sqrt()
    bound = rtol * (ref.abs() + rms)
    err = (got - ref).abs()
    bad = (err > bound).sum().item()
    worst = (err / bound.clamp(min=1e-30)).max().item()
    print(f"{name}: worst err/bound {worst:.3f}")
    assert bad == 0, (f"{name}: {bad}/{ref.numel()} elements out of bound, "
                      f"worst ratio {worst:.2f}")


def test_instnorm_residual_act_backward():
    """ops.instance_norm(act='relu', residual=r): _InstNormFn.backward's
    branch that transforms dy through the activation first. fp64 reference
    whose pre-activation is rounded to bf16 (straight-through), so that
    its relu mask is taken where the op's stored output takes it; the
    mask makes a derived bound awkward, so this uses check_elem with the
    tolerances of tests/test_in_epilogue_gpu.py."""
    shape = (2, 12, 12, 64)
    d = torch.float64
    x = kb.uniform_bf16(shape, 51)
    r = kb.uniform_bf16(shape, 52)
    dy = kb.uniform_bf16(shape, 53)
    g = torch.Generator().manual_seed(54)
    gamma = torch.randn(64, generator=g) * 0.5
    beta = torch.randn(64, generator=g) * 0.1

    xg = dev(x).requires_grad_(True)
    rg = dev(r).requires_grad_(True)
    gg = dev(gamma).requires_grad_(True)
    bg = dev(beta).requires_grad_(True)
    y = ops.instance_norm(xg, gg, bg, act="relu", residual=rg)
    y.backward(dev(dy))

    xr = x.to(d).requires_grad_(True)
    rr = r.to(d).requires_grad_(True)
    gr = gamma.to(d).requires_grad_(True)
    br = beta.to(d).requires_grad_(True)
    mean = xr.mean((1, 2), keepdim=True)
    var = xr.var((1, 2), unbiased=False, keepdim=True)
    pre = (xr - mean) * (var + 1e-3).rsqrt() * gr + br + rr
    pre = pre + (pre.to(torch.bfloat16).to(d) - pre).detach()
    yr = torch.relu(pre)
    yr.backward(dy.to(d))

    check_elem(y, yr, 0.04, "in_res_relu:y")
    check_elem(xg.grad, xr.grad, 0.06, "in_res_relu:dx")
    check_elem(gg.grad, gr.grad, 0.05, "in_res_relu:dgamma")
    check_elem(bg.grad, br.grad, 0.05, "in_res_relu:dbeta")
    check_elem(rg.grad, rr.grad, 0.04, "in_res_relu:dres")
