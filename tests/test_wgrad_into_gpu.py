"""conv2d_wgrad_into / fold_packed_dw_into: the reduce that writes a weight
gradient straight into the parameter's block of a flat buffer.

Every case uses as `out` a view at an odd float offset inside a larger
buffer whose other elements are NaN, and the NaNs must be intact
afterwards. On the slab path the result must be bit-equal to what the
Python of the backward functions makes of conv2d_wgrad (crop, permute), and
with accumulate bit-equal to prior + that: the slab sum is formed by the
same four chains and the prior is added last.

All tests @pytest.mark.gpu.
"""

import pytest
import torch
import torch.nn.functional as F

import _kernel_bounds as kb
from cyclegan_amd.ops import backend
from cyclegan_amd.ops.conv import _fold_packed_dw

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OFFSET = 37          # odd: the view is only 4-byte aligned
TAIL = 29


def dev(t):
    return t.to(DEV).contiguous()


def nan_buffer(shape):
    """(buffer, view): a NaN-filled flat buffer and a view of `shape` at an
    odd float offset inside it."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((OFFSET + n + TAIL,), float("nan"), device=DEV)
    return buf, buf[OFFSET:OFFSET + n].view(shape)


def assert_rest_nan(buf, n):
    assert torch.isnan(buf[:OFFSET]).all() and \
        torch.isnan(buf[OFFSET + n:]).all(), "wrote outside the view"


def pad8(t):
    c = t.shape[-1]
    return t if c >= 8 else F.pad(t, (0, 8 - c))


# the slab (glds) path: the case-table rows the issue names, one row whose
# slice count is not a multiple of 4 (M = 420 -> 7 slices: one round of the
# four chains and a tail of 3), and the two channel crops
SLICES7 = kb.Case("slices7", "conv", 3, 10, 14, 64, 64, 3, 3, 1, kb.R1, True,
                  "7 split-M slices: reduce tail loop")
CIN_CROP = kb.Case("cin_crop", "conv", 1, 12, 12, 3, 16, 4, 4, 2, "same",
                   False, "true Cin 3 padded to 8")
COUT_CROP = kb.Case("cout_crop", "conv", 1, 6, 6, 64, 1, 4, 4, 1, "same",
                    False, "true Cout 1 padded to 8")
SLAB_CASES = [kb.CASE_BY_ID["cin24"], kb.CASE_BY_ID["grid8"],
              kb.CASE_BY_ID["s2_odd"], SLICES7, CIN_CROP, COUT_CROP,
              kb.CASE_BY_ID["ct_k4"], kb.CASE_BY_ID["ct_nsq"]]


def case_inputs(case, seed):
    x = kb.uniform_bf16(case.x_shape, seed)
    dy = kb.uniform_bf16(case.y_shape, seed + 3)
    return x, dy


def todays(case, x, dy):
    """What the backward functions made of conv2d_wgrad before there was a
    destination: (gemm operands, OHWI gradient)."""
    ext = backend.ext()
    pt, _, pl, _ = case.pads
    if case.kind == "convt":
        dwc = ext.conv2d_wgrad(dy, x, case.KH, case.KW, case.stride, pt, pl,
                               False)
        return (dy, x), dwc.permute(3, 1, 2, 0).contiguous()
    xp, dyp = pad8(x).contiguous(), pad8(dy).contiguous()
    dw = ext.conv2d_wgrad(xp, dyp, case.KH, case.KW, case.stride, pt, pl,
                          case.reflect)
    return (xp, dyp), dw[:case.Cout, :, :, :case.Cin].contiguous()


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accum"])
@pytest.mark.parametrize("case", SLAB_CASES, ids=[c.id for c in SLAB_CASES])
def test_wgrad_into(case, accumulate):
    ext = backend.ext()
    x, dy = case_inputs(case, 700 + 10 * SLAB_CASES.index(case))
    (a, b), want = todays(case, dev(x), dev(dy))
    assert tuple(want.shape) == case.w_shape
    buf, out = nan_buffer(case.w_shape)
    if accumulate:
        prior = torch.randn(case.w_shape, device=DEV,
                            generator=torch.Generator(DEV).manual_seed(5))
        out.copy_(prior)
        want = prior + want
    pt, _, pl, _ = case.pads
    ext.conv2d_wgrad_into(a, b, case.KH, case.KW, case.stride, pt, pl,
                          case.reflect and case.kind == "conv", out,
                          accumulate, case.kind == "convt")
    assert_rest_nan(buf, out.numel())
    assert torch.equal(out, want)


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accum"])
def test_wgrad_into_fallback(accumulate):
    """cout20 takes the atomics fallback (wgrad_kernel into zeros, then one
    ATen copy_/add_): atomics have no fixed order, so the wgrad bound
    2*M*u32*S_w replaces equality; the prior adds u32*|result|."""
    ext = backend.ext()
    case = kb.CASE_BY_ID["cout20"]
    x, _, _, dy = kb.make_inputs(case)
    ref, bound = kb.wgrad_ref_bound(case, x, dy)
    buf, out = nan_buffer(case.w_shape)
    if accumulate:
        prior = kb.uniform_bf16(case.w_shape, 77).float()
        out.copy_(prior)
        ref = ref + prior.double()
        bound = bound + kb.U32 * ref.abs()
    pt, _, pl, _ = case.pads
    ext.conv2d_wgrad_into(dev(x), dev(dy), case.KH, case.KW, case.stride, pt,
                          pl, case.reflect, out, accumulate, False)
    assert_rest_nan(buf, out.numel())
    kb.assert_within(out, ref, bound, f"cout20:into:{accumulate}", "okki")


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accum"])
def test_fold_packed_into(accumulate):
    """The packed head's fold kernel on the 1x9x24, 64 -> 3 head against
    _fold_packed_dw. Both add the same eight fp32 terms per element, in an
    order torch does not promise: bound 8*u32*sum_d|term| (plus u32*|result|
    for the prior's add)."""
    ext = backend.ext()
    B, H, W, Cin, O = 1, 9, 24, 64, 3
    x = kb.uniform_bf16((B, H, W, Cin), 31)
    dy = kb.uniform_bf16((B, H, W, O), 34)
    xp = ext.reflect_pad_fwd(dev(x), 3, 3, 3, 5)
    xf = xp.view(B, H + 6, (W + 8) // 8, 8 * Cin)
    dy_pk = pad8(dev(dy)).contiguous().view(B, H, W // 8, 64)
    dwp = ext.conv2d_wgrad(xf, dy_pk, 7, 2, 1, 0, 0, False)
    wshape = (O, 7, 7, Cin)
    ref = _fold_packed_dw(dwp.double(), wshape).cpu()
    bound = 8 * kb.U32 * _fold_packed_dw(dwp.double().abs(), wshape).cpu()
    buf, out = nan_buffer(wshape)
    if accumulate:
        prior = kb.uniform_bf16(wshape, 78).float()
        out.copy_(prior)
        ref = ref + prior.double()
        bound = bound + kb.U32 * ref.abs()
    ext.fold_packed_dw_into(dwp, out, accumulate)
    assert_rest_nan(buf, out.numel())
    kb.assert_within(out, ref, bound, f"fold_packed:{accumulate}", "okki")
