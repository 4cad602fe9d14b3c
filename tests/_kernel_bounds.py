"""fp64 references, derived error bounds and the edge-shape case tables
for the conv / convT / dgrad / wgrad kernels.

A plain helper module (no fixtures, no hooks) shared by
tests/test_kernel_bounds_cpu.py, which proves on the CPU that the bounds
accept a faithful emulation of the kernels' arithmetic and reject subtly
wrong variants, and tests/test_conv_edges_gpu.py, which holds the kernels
to the same bounds.

The references are written here from F.pad / F.conv2d /
F.conv_transpose2d directly, not through ops.conv's helpers, so that a
bug in those helpers cannot cancel; one CPU test checks that the two
agree.

Notation: u16 = 2^-8 is the unit roundoff of bf16 round-to-nearest-even,
u32 = 2^-24 that of fp32. Every bound is per element and excludes
nothing.
"""

from dataclasses import dataclass
from typing import Optional, Tuple, Union

import torch
import torch.nn.functional as F

from cyclegan_amd.ops.conv import same_pads

U16 = 2.0 ** -8
U32 = 2.0 ** -24

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
ACT_ID = {None: ACT_NONE, "relu": ACT_RELU, "lrelu": ACT_LRELU,
          "tanh": ACT_TANH}
SLOPE = 0.2


# ------------------------------------------------------------- cases ----
@dataclass(frozen=True)
class Case:
    """One shape. conv: x is [B,H,W,Cin]; convt: x is [B,H,W,Cin] and the
    output is [B,H*s,W*s,Cout]. Weights are OHWI [Cout,KH,KW,Cin]."""
    id: str
    kind: str                      # "conv" | "convt"
    B: int
    H: int
    W: int
    Cin: int
    Cout: int
    KH: int
    KW: int
    stride: int
    pad: Union[str, Tuple[int, int, int, int]]   # "same" | "none" | pads
    reflect: bool
    reaches: str

    @property
    def pads(self) -> Tuple[int, int, int, int]:
        """(pt, pb, pl, pr). For convt: the pads of the strided conv the
        transpose conv is the adjoint of (output frame -> input frame)."""
        if self.kind == "convt":
            return same_pads(self.H * self.stride, self.W * self.stride,
                             self.KH, self.KW, self.stride)
        if self.pad == "same":
            return same_pads(self.H, self.W, self.KH, self.KW, self.stride)
        if self.pad == "none":
            return (0, 0, 0, 0)
        return tuple(self.pad)

    @property
    def out_hw(self) -> Tuple[int, int]:
        if self.kind == "convt":
            return self.H * self.stride, self.W * self.stride
        pt, pb, pl, pr = self.pads
        return ((self.H + pt + pb - self.KH) // self.stride + 1,
                (self.W + pl + pr - self.KW) // self.stride + 1)

    @property
    def x_shape(self):
        return (self.B, self.H, self.W, self.Cin)

    @property
    def w_shape(self):
        return (self.Cout, self.KH, self.KW, self.Cin)

    @property
    def y_shape(self):
        return (self.B, *self.out_hw, self.Cout)


def _c(id, B, H, W, Cin, Cout, KH, KW, s, pad, reflect, reaches):
    return Case(id, "conv", B, H, W, Cin, Cout, KH, KW, s, pad, reflect,
                reaches)


def _t(id, B, H, W, Cin, Cout, K, s, reaches):
    return Case(id, "convt", B, H, W, Cin, Cout, K, K, s, "same", False,
                reaches)


R1 = (1, 1, 1, 1)

CONV_CASES = [
    _c("nsq_reflect", 2, 6, 20, 64, 64, 3, 3, 1, R1, True,
       "H != W; M = 240 tail"),
    _c("cin24", 2, 6, 20, 24, 24, 3, 3, 1, R1, True,
       "Cin < 64 with 64 % Cin != 0; partial 64-wide n-tile"),
    _c("cin40_s2", 1, 9, 14, 40, 16, 4, 4, 2, "same", False,
       "Cin < 64; asymmetric pads; 16-wide tile full"),
    _c("cin96", 1, 7, 9, 96, 96, 3, 3, 1, R1, True,
       "big_ci wrap with remainder; M = 63 < 128; second n-tile partial"),
    _c("cin72_s3", 3, 10, 13, 72, 24, 3, 3, 3, "same", False,
       "STRIDE = 0 template; B = 3"),
    _c("s3_dgrad", 2, 11, 8, 64, 64, 4, 4, 3, "same", False,
       "generic-stride convT gather (dgrad)"),
    _c("s2_odd", 2, 15, 17, 64, 128, 4, 4, 2, "same", False,
       "non-phased stride-2 gather in dgrad; BN = 128 tile"),
    _c("s2_odd_k3", 1, 13, 9, 128, 64, 3, 3, 2, "same", False,
       "non-phased stride-2 gather in dgrad, 3x3, M = 35"),
    _c("k1", 2, 8, 8, 64, 192, 1, 1, 1, "none", False,
       "nk = 1 (no advance); three 64-wide n-tiles; M = 128 exactly"),
    _c("k1_cin24", 1, 5, 7, 24, 8, 1, 1, 1, "none", False,
       "KTOT < BK; M = 35"),
    _c("k7x2_valid", 2, 10, 6, 64, 64, 7, 2, 1, "none", False,
       "KH != KW (the packed-head geometry) at small size"),
    _c("k1x3", 1, 6, 12, 64, 64, 1, 3, 1, (0, 0, 1, 1), False,
       "KH != KW, pad in W only"),
    _c("k7_padmax", 1, 4, 16, 8, 64, 7, 7, 1, (3, 3, 3, 3), True,
       "pad = H-1; KTOT = 392 (K-tail 8); fold has 3 live candidates "
       "per axis"),
    _c("ow64_short", 3, 4, 64, 64, 64, 3, 3, 1, R1, True,
       "wgrad ow_fast with a batch wrap every 4 steps"),
    _c("ow64_s2", 2, 6, 128, 64, 128, 3, 3, 2, "same", False,
       "ow_fast with stride 2 and pads (0,1,0,1)"),
    _c("cout20", 2, 6, 10, 64, 20, 3, 3, 1, R1, False,
       "Cout % 8 != 0: wgrad atomics fallback; scalar epilogue columns; "
       "dgrad through conv_gemm_kernel"),
    _c("cin12", 2, 6, 10, 12, 64, 3, 3, 1, R1, False,
       "conv_gemm_kernel unaligned; wgrad fallback"),
    _c("grid8", 4, 16, 16, 64, 128, 3, 3, 1, R1, True,
       "tile count % 8 == 0 (XCD remap on)"),
    _c("grid8_b3", 3, 16, 16, 64, 128, 3, 3, 1, R1, True,
       "tile count 6, remap off, same shape otherwise"),
    # rows added on reading the kernels: every row above has pt == pl
    # except k1x3 (where pt = 0), so a pt/pl or pb/pr mix-up in the gather
    # or in reflect_fold_kernel had one thin witness
    _c("pads_asym", 1, 7, 10, 64, 64, 3, 3, 1, (2, 0, 0, 2), False,
       "zero pads with pt != pl and pt != pb"),
    _c("reflect_asym", 1, 6, 9, 64, 64, 3, 3, 1, (2, 0, 0, 2), True,
       "reflect pads with pt != pl, pb = pl = 0: fold candidates differ "
       "per axis and per side"),
]

CONVT_CASES = [
    _t("ct_nsq", 2, 5, 12, 128, 64, 3, 2,
       "phased, H != W, phase tiles with M tail (Mp = 120)"),
    _t("ct_cin96", 1, 6, 10, 96, 96, 3, 2,
       "phased with KEFF differing per phase and Cin % 64 != 0"),
    _t("ct_k4", 2, 4, 6, 64, 24, 4, 2,
       "phased, even kernel (nvh = nvw = 2 for all phases), partial n-tile"),
    _t("ct_s3", 1, 4, 5, 64, 64, 3, 3,
       "non-phased generic-stride convT forward"),
    _t("ct_s1", 2, 6, 9, 64, 64, 3, 1, "convT stride 1 forward"),
    _t("ct_cin3", 2, 6, 6, 3, 16, 3, 2,
       "unaligned convT (conv_gemm_kernel<true,false,...>)"),
]

ALL_CASES = CONV_CASES + CONVT_CASES
CASE_BY_ID = {c.id: c for c in ALL_CASES}

# forward-only additions: (case id, act)
FWD_ACT_CASES = [(cid, act) for cid in ("cin24", "nsq_reflect")
                 for act in ("relu", "lrelu", "tanh")] + [("cout20", None)]


def uniform_bf16(shape, seed, scale=1.0):
    """Uniform in [-scale, scale], rounded to bf16 (CPU tensor)."""
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand(shape, generator=g) * 2 - 1) * scale
    return t.to(torch.bfloat16)


def case_seed(case: Case) -> int:
    return 1000 + 10 * ALL_CASES.index(case)


def make_inputs(case: Case):
    """(x, w, bias, dy) as bf16 CPU tensors; weights scaled by 0.2."""
    s = case_seed(case)
    x = uniform_bf16(case.x_shape, s)
    w = uniform_bf16(case.w_shape, s + 1, 0.2)
    bias = uniform_bf16((case.Cout,), s + 2)
    dy = uniform_bf16(case.y_shape, s + 3)
    return x, w, bias, dy


# -------------------------------------------------- plain operations ----
# Written for any float dtype: fp64 gives the references, fp32 the
# emulation of the kernels' accumulate.
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _pad(xn, pads, mode):
    pt, pb, pl, pr = pads
    if not (pt or pb or pl or pr):
        return xn
    return F.pad(xn, (pl, pr, pt, pb), mode=mode)


def conv_fwd_lin(x, w, bias, stride, pads, pad_mode="constant"):
    """NHWC conv, OHWI weight, explicit pads; pad_mode constant | reflect |
    replicate. Linear part only (no activation)."""
    xn = _pad(_nchw(x), pads, pad_mode)
    y = F.conv2d(xn, w.permute(0, 3, 1, 2), bias, stride=stride)
    return _nhwc(y)


def convt_fwd_lin(x, w, bias, stride, pt, pl, out_h, out_w):
    """out[b, s*o + k - pt, ..., co] += x[b, o, ..., ci] * w[co, k, ..., ci]:
    the full transpose conv, cropped to the 'SAME' output frame."""
    y = F.conv_transpose2d(_nchw(x), w.permute(3, 0, 1, 2), bias,
                           stride=stride)
    y = y[:, :, pt:pt + out_h, pl:pl + out_w]
    return _nhwc(y)


def apply_act(y, act, slope=SLOPE):
    if act == "relu":
        return torch.relu(y)
    if act == "lrelu":
        return F.leaky_relu(y, slope)
    if act == "tanh":
        return torch.tanh(y)
    assert act is None
    return y


def case_fwd_lin(case: Case, x, w, bias, pad_mode=None):
    """The case's forward (no activation) in the dtype of its arguments."""
    if case.kind == "convt":
        pt, _, pl, _ = case.pads
        oh, ow = case.out_hw
        return convt_fwd_lin(x, w, bias, case.stride, pt, pl, oh, ow)
    if pad_mode is None:
        pad_mode = "reflect" if case.reflect else "constant"
    return conv_fwd_lin(x, w, bias, case.stride, case.pads, pad_mode)


def _grad(fn, shape, dy, dtype):
    """Adjoint of the linear map fn at dy."""
    leaf = torch.zeros(shape, dtype=dtype, requires_grad=True)
    (g,) = torch.autograd.grad(fn(leaf), leaf, dy.to(dtype))
    return g


def case_dgrad(case: Case, dy, w, pad_mode=None):
    """d/dx of the case's forward, applied to dy."""
    return _grad(lambda x: case_fwd_lin(case, x, w, None, pad_mode),
                 case.x_shape, dy, w.dtype)


def case_wgrad(case: Case, x, dy, pad_mode=None):
    """d/dw of the case's forward, applied to dy; OHWI."""
    return _grad(lambda w: case_fwd_lin(case, x, w, None, pad_mode),
                 case.w_shape, dy, x.dtype)


def padded_shape(case: Case):
    pt, pb, pl, pr = case.pads
    return (case.B, case.H + pt + pb, case.W + pl + pr, case.Cin)


def dgrad_padded(case: Case, dy, w):
    """Gradient with respect to the explicitly padded input (the frame
    the reflect dgrad kernel writes before the fold)."""
    return _grad(lambda xp: conv_fwd_lin(xp, w, None, case.stride,
                                         (0, 0, 0, 0)),
                 padded_shape(case), dy, w.dtype)


def pad_adjoint(case: Case, tp, pad_mode="reflect"):
    """Adjoint of the pad: sums every padded-frame element onto the
    interior element it mirrors."""
    return _grad(lambda x: _nhwc(_pad(_nchw(x), case.pads, pad_mode)),
                 case.x_shape, tp, tp.dtype)


# ------------------------------------------------------------ bounds ----
def fwd_ref_bound(case: Case, x, w, bias=None, act=None):
    """Forward reference and bound; x, w, bias are the bf16 inputs.

    The kernel computes y = bf16(act(acc + bias)). Products of two bf16
    values are exact in fp32 (8 + 8 significand bits), so acc differs from
    the exact sum only by the K-term fp32 accumulation, K = KH*KW*Cin
    (the kernel adds every tap, padded or phase-excluded ones as exact
    zeros): |acc + bias - pre| <= e with

        e = 2 * K * u32 * S,

    S the same operation on |x|, |w|, |bias| (the sum of the terms'
    magnitudes). The classical bound is (K-1)*u32*S for round-to-nearest
    in any order; the factor 2 allows MFMA-internal additions that
    truncate instead of rounding, and covers the bias add. relu, lrelu
    and tanh are 1-Lipschitz, so the error after the activation is still
    <= e (tanhf itself adds a few ulp of a value <= 1: 4*u32). The final
    rounding to bf16 adds u16 * |value rounded| <= u16 * (|ref| + e):

        bound = u16 * (|ref| + e) + e.
    """
    d = torch.float64
    xf, wf = x.to(d), w.to(d)
    bf = bias.to(d) if bias is not None else None
    ref = apply_act(case_fwd_lin(case, xf, wf, bf), act)
    S = case_fwd_lin(case, xf.abs(), wf.abs(),
                     bf.abs() if bf is not None else None)
    K = case.KH * case.KW * case.Cin
    e = 2 * K * U32 * S
    if act == "tanh":
        e = e + 4 * U32
    return ref, U16 * (ref.abs() + e) + e


def dgrad_ref_bound(case: Case, dy, w):
    """dgrad reference and bound; dy, w are the bf16 inputs.

    Zero padding, and convT dgrad: dx = bf16(acc), acc an fp32 sum over
    the (tap, channel) terms of the adjoint; the kernels walk all
    K = KH*KW*Cout of them (taps that miss the stride grid or the image
    contribute exact zeros). With S the adjoint on |dy|, |w|:

        e = 2 * K * u32 * S,  bound = u16 * (|ref| + e) + e.

    Reflect padding: the kernel first writes the padded-frame gradient
    dxp = bf16(acc) (error <= u16*(|dxp_ref| + e) + e per padded element,
    as above), then reflect_fold_kernel sums the <= 9 mirror images of
    each interior element in fp32 and rounds to bf16 again. Folding the
    per-element errors through the pad's adjoint, with T = fold|dxp_ref|
    and E = fold(e):

        |sum - ref| <= u16*T + (1 + u16)*E + 8*u32*(T + ...)
        bound = u16 * (T + |ref|) + 2 * E.

    The second E absorbs u16*E, the fold's own fp32 additions (8*u32*T <
    E because e >= 2*K*u32*|dxp_ref| with K >= 72) and the second-order
    part of the final rounding u16*|sum|.
    """
    d = torch.float64
    dyf, wf = dy.to(d), w.to(d)
    K = case.KH * case.KW * case.Cout
    ref = case_dgrad(case, dyf, wf)
    if not (case.kind == "conv" and case.reflect):
        S = case_dgrad(case, dyf.abs(), wf.abs())
        e = 2 * K * U32 * S
        return ref, U16 * (ref.abs() + e) + e
    dxp_ref = dgrad_padded(case, dyf, wf)
    e = 2 * K * U32 * dgrad_padded(case, dyf.abs(), wf.abs())
    T = pad_adjoint(case, dxp_ref.abs())
    E = pad_adjoint(case, e)
    return ref, U16 * (T + ref.abs()) + 2 * E


def wgrad_M(case: Case) -> int:
    """Rows of the wgrad GEMM: positions of the strided conv's output
    frame (for convT that is the transpose conv's input)."""
    if case.kind == "convt":
        return case.B * case.H * case.W
    oh, ow = case.out_hw
    return case.B * oh * ow


def wgrad_ref_bound(case: Case, x, dy):
    """wgrad reference and bound; x, dy are the bf16 inputs.

    dw is fp32: the sum of M = B*OH*OW exact bf16 products per element,
    accumulated in fp32 in split-M slabs that a second kernel adds (or by
    fp32 atomics in the fallback kernel). Any summation order of M terms
    stays within (M-1)*u32*S_w; with the same factor 2 as the forward:

        bound = 2 * M * u32 * S_w,

    S_w the wgrad on |x|, |dy|. Where S_w == 0 (a tap that never meets
    data) the bound is 0 and the output must be exactly zero.
    """
    d = torch.float64
    xf, dyf = x.to(d), dy.to(d)
    ref = case_wgrad(case, xf, dyf)
    Sw = case_wgrad(case, xf.abs(), dyf.abs())
    return ref, 2 * wgrad_M(case) * U32 * Sw


def dbias_ref_bound(dy):
    """db = sum of dy over (b, h, w): an fp32 sum of M exact values,
    bound = 2 * M * u32 * sum|dy|."""
    dyf = dy.to(torch.float64)
    M = dy.shape[0] * dy.shape[1] * dy.shape[2]
    return dyf.sum((0, 1, 2)), 2 * M * U32 * dyf.abs().sum((0, 1, 2))


# ----------------------------------------------------------- checker ----
def worst_ratio(got, ref, bound):
    """(count outside, worst err/bound, flat index of the worst)."""
    got = got.detach().to("cpu", torch.float64)
    ref = ref.to(torch.float64)
    assert got.shape == ref.shape == bound.shape, \
        f"{tuple(got.shape)} vs {tuple(ref.shape)} vs {tuple(bound.shape)}"
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err,
                      torch.full_like(err, float("inf")))
    bad = err > bound
    # err/bound with 0/0 = 0 and x/0 = inf
    ratio = torch.where(err == 0, torch.zeros_like(err),
                        err / bound.clamp(min=1e-300))
    ratio = torch.where(bad & (bound == 0),
                        torch.full_like(ratio, float("inf")), ratio)
    flat = int(ratio.reshape(-1).argmax()) if ratio.numel() else 0
    return int(bad.sum()), float(ratio.reshape(-1)[flat]), flat, err


LAYOUTS = {"bhwc": ("b", "h", "w", "c"), "okki": ("co", "kh", "kw", "ci"),
           "bc": ("b", "c"), "c": ("c",)}

def assert_within(got, ref, bound, name, layout="bhwc"):
    """Every element of got within bound of ref. Prints the worst
    err/bound (the figures recorded in docs/KERNELS.md); on failure
    reports how many elements are outside, the worst err/bound and the
    worst element's index decoded into the layout's coordinates."""
    nbad, worst, flat, err = worst_ratio(got, ref, bound)
    print(f"{name}: worst err/bound {worst:.3f}")
    if nbad == 0:
        return worst
    idx = []
    for n in reversed(ref.shape):
        idx.append(flat % n)
        flat //= n
    idx = tuple(reversed(idx))
    names = LAYOUTS.get(layout, ())
    where = ", ".join(f"{n}={i}" for n, i in zip(names, idx)) or str(idx)
    g = got.detach().to("cpu", torch.float64)[idx].item()
    raise AssertionError(
        f"{name}: {nbad}/{ref.numel()} elements outside the bound, worst "
        f"err/bound {worst:.2f} at ({where}): got {g:.6g}, ref "
        f"{ref[idx].item():.6g}, bound {bound[idx].item():.3g}")


def violations(got, ref, bound) -> int:
    return worst_ratio(got, ref, bound)[0]


# --------------------------------------------------------- emulation ----
def rne(t):
    """fp32 -> bf16 round-to-nearest-even -> fp32."""
    return t.to(torch.bfloat16).to(torch.float32)


def trunc(t):
    """fp32 -> bf16 by dropping the low 16 bits -> fp32."""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def emu_fwd(case, x, w, bias=None, act=None, rnd=rne, pad_mode=None):
    """Kernel arithmetic: fp32 accumulate, one rounding to bf16."""
    f = torch.float32
    pre = case_fwd_lin(case, x.to(f), w.to(f),
                       bias.to(f) if bias is not None else None, pad_mode)
    return rnd(apply_act(pre, act))


def emu_dgrad(case, dy, w, rnd=rne, drop_mirror=False):
    """Kernel arithmetic of dgrad; with reflect padding the padded-frame
    gradient is rounded to bf16, folded in fp32 and rounded again.
    drop_mirror leaves one padded-frame border pixel out of the fold."""
    f = torch.float32
    if not (case.kind == "conv" and case.reflect):
        return rnd(case_dgrad(case, dy.to(f), w.to(f)))
    dxp = rnd(dgrad_padded(case, dy.to(f), w.to(f)))
    if drop_mirror:
        pt, pb, pl, pr = case.pads
        # one pixel of the pad border that is not a corner image
        if pt:
            dxp[0, 0, pl + 1, :] = 0
        elif pl:
            dxp[0, pt + 1, 0, :] = 0
        elif pb:
            dxp[0, -1, pl + 1, :] = 0
        else:
            dxp[0, pt + 1, -1, :] = 0
    return rnd(pad_adjoint(case, dxp))


def emu_wgrad(case, x, dy, pad_mode=None):
    f = torch.float32
    return case_wgrad(case, x.to(f), dy.to(f), pad_mode)


def conv_fwd_shifted(case, x, w, pt, pl):
    """Zero-padded conv as the kernel parameterises it: out[oh, ow] reads
    x[oh*s + kh - pt, ow*s + kw - pl] (zero outside the image) on the
    case's output frame, for any pt/pl."""
    assert case.kind == "conv" and not case.reflect
    oh, ow = case.out_hw
    s = case.stride
    pb = (oh - 1) * s + case.KH - case.H - pt
    pr = (ow - 1) * s + case.KW - case.W - pl
    # F.pad in constant mode crops for negative pads
    xn = F.pad(_nchw(x), (pl, pr, pt, pb))
    return _nhwc(F.conv2d(xn, w.permute(0, 3, 1, 2), None, stride=s))


# ------------------------------------------------------ InstanceNorm ----
def in_ref_bounds(x, gamma, beta, eps):
    """fp64 InstanceNorm of the bf16 x [B,H,W,C] and the bounds on the
    kernel's outputs.

    The kernels compute mean = sum(x)/HW and var = sum(x^2)/HW - mean^2 in
    fp32. Each fp32 sum of HW terms is within HW*u32*sum|term|, so

        |mean - mean_ref| <= d_m = HW * u32 * E|x|
        |var - var_ref|   <= ~ HW * u32 * (E[x^2] + mean^2) * 2 =: d * (var + eps)

    with d = 2*HW*u32*(E[x^2] + mean^2)/(var + eps) the relative error of
    var + eps (this is where a large mean hurts: the two subtracted terms
    are each ~ mean^2). rstd = (var+eps)^-1/2 then moves by 1/2 * d * rstd
    and the normalised value x^ = (x - mean) * rstd by 1/2*|x^|*d +
    d_m*rstd. Scaling by |gamma| and rounding the result to bf16:

        bound_y    = u16*|ref| + |gamma| * (1/2*|x^|*d + d_m*rstd)
        bound_mean = d_m,  bound_rstd = 1/2 * d * rstd.

    Returns (y, mean, rstd) references and the three bounds; mean/rstd
    are [B,C].
    """
    xf = x.to(torch.float64)
    HW = x.shape[1] * x.shape[2]
    g = gamma.to(torch.float64)
    b = beta.to(torch.float64)
    mean = xf.mean((1, 2))
    ex2 = (xf * xf).mean((1, 2))
    var = xf.var((1, 2), unbiased=False)
    rstd = (var + eps).rsqrt()
    xhat = (xf - mean[:, None, None]) * rstd[:, None, None]
    y = xhat * g + b
    d_m = HW * U32 * xf.abs().mean((1, 2))
    d = 2 * HW * U32 * (ex2 + mean * mean) / (var + eps)
    by = U16 * y.abs() + g.abs() * (
        0.5 * xhat.abs() * d[:, None, None]
        + (d_m * rstd)[:, None, None])
    return (y, mean, rstd), (by, d_m, 0.5 * d * rstd), float(d.max())
