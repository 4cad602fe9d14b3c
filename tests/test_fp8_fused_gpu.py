"""fp8 quantisation fused into InstanceNorm, InstanceNorm slabs from the fp8
conv epilogue, and the hand-off between the two (ops / models / trainer).

Kernel-level checks are exact: the twin bytes are defined as what
quant_fp8_d makes of the norm's stored bf16 output, and asking the fp8 conv
for slabs must not move its output. Shapes are the smallest that reach every
path: one and several slices per sample, a ragged row loop, the narrow-C /
C == NT / C > NT prologues, one and two n-tiles, an odd sample count (XCD
tile remap), a K tail, and the ineligible shapes.

All tests @pytest.mark.gpu.
"""

import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu

from cyclegan_amd import ops
from cyclegan_amd.models import Generator
from cyclegan_amd.models.layers import ResBlock
from cyclegan_amd.ops import backend, fp8_state
from cyclegan_amd.ops import conv as convmod
from cyclegan_amd.ops.conv import FP8_TWIN_ATTR, IN_SLABS_ATTR, _ACT

DEV = "cuda:0"


def mk(shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand(shape, generator=g) * 2 - 1) * scale
    return t.to(DEV, torch.bfloat16)


def check_elem(got, ref, rtol, name=""):
    """Per-element |err| <= rtol * (|ref| + rms(ref)) — the bound form of
    tests/test_in_epilogue_gpu.py."""
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


@pytest.fixture
def fp8_on():
    fp8_state.reset()
    convmod.set_fp8_mode(True)
    try:
        yield
    finally:
        convmod.set_fp8_mode(False)
        fp8_state.reset()


class QuantCounter:
    """Counts standalone quant_fp8_d launches."""

    def __init__(self, monkeypatch):
        ext = backend.ext()
        self.n = 0
        real = ext.quant_fp8_d

        def counted(*a):
            self.n += 1
            return real(*a)

        monkeypatch.setattr(ext, "quant_fp8_d", counted)


# ------------------------------------------------------------ twin kernel ---
def _affine(C):
    g = (torch.randn(C, generator=torch.Generator().manual_seed(3)) * 0.5).to(DEV)
    b = (torch.randn(C, generator=torch.Generator().manual_seed(4)) * 0.1).to(DEV)
    return g, b


def _check_twin(x, g, b, act, res, psum=None, psq=None):
    ext = backend.ext()
    a = _ACT[act]
    ns = psum.shape[0] if psum is not None else 0
    if psum is not None:
        y0, m0, r0 = ext.instnorm_fwd(x, g, b, 1e-3, a, 0.2, res, psum, psq, ns)
    else:
        y0, m0, r0 = ext.instnorm_fwd(x, g, b, 1e-3, a, 0.2, res)
    amax = y0.float().abs().max().reshape(1)
    assert amax.item() > 0
    # true amax; a quarter of it (saturated codes); 0 (scale clamps at 65504)
    for prev in (amax, amax / 4, torch.zeros_like(amax)):
        cur = torch.zeros(1, device=DEV)
        cur_ref = torch.zeros(1, device=DEV)
        y, m, r, yq = ext.instnorm_fwd_q8(x, g, b, 1e-3, a, 0.2, res, psum,
                                          psq, ns, prev, cur)
        ref_q = ext.quant_fp8_d(y0, prev, cur_ref)
        assert torch.equal(y, y0) and torch.equal(m, m0) and torch.equal(r, r0)
        assert yq.dtype == torch.uint8 and yq.shape == y.shape
        nbad = (yq != ref_q).sum().item()
        assert nbad == 0, f"prev={prev.item()}: {nbad} twin bytes differ"
        assert torch.equal(cur, cur_ref)
        assert torch.equal(cur, amax)


@pytest.mark.parametrize("variant", ["relu", "lrelu", "none_res"])
@pytest.mark.parametrize("C", [64, 256, 512])
@pytest.mark.parametrize("hw", [(16, 16), (12, 12), (5, 7)],
                         ids=["16x16", "12x12", "5x7"])
def test_twin_matches_standalone_quant(hw, C, variant):
    """in_reduce route: y/mean/rstd equal instnorm_fwd bit for bit, yq
    equals quant_fp8_d(y), amax_cur equals max|y|."""
    H, W = hw
    x = mk((2, H, W, C), seed=301)
    g, b = _affine(C)
    act = None if variant == "none_res" else variant
    res = mk(x.shape, seed=302) if variant == "none_res" else None
    _check_twin(x, g, b, act, res)


@pytest.mark.parametrize("variant", ["relu", "none_res"])
def test_twin_on_slab_route(variant):
    """Same, with the statistics taken from a bf16 conv's epilogue slabs."""
    ext = backend.ext()
    xin = mk((2, 16, 16, 64), seed=303)
    w = mk((256, 3, 3, 64), seed=304, scale=0.2)
    h, psum, psq = ext.conv2d_fwd_stats(xin, w, None, 1, 1, 1, 1, 1, True, 0, 0.2)
    g, b = _affine(256)
    act = None if variant == "none_res" else variant
    res = mk(h.shape, seed=305) if variant == "none_res" else None
    _check_twin(h, g, b, act, res, psum, psq)


def test_twin_leaves_larger_amax_cur_alone():
    ext = backend.ext()
    x = mk((2, 16, 16, 64), seed=306)
    g, b = _affine(64)
    y0, _, _ = ext.instnorm_fwd(x, g, b, 1e-3, 1, 0.2, None)
    amax = y0.float().abs().max().reshape(1)
    big = amax * 3 + 1
    cur = big.clone()
    ext.instnorm_fwd_q8(x, g, b, 1e-3, 1, 0.2, None, None, None, 0, amax, cur)
    assert torch.equal(cur, big)


# -------------------------------------------------------- fp8 conv slabs ---
# name, B, H, W, Cin, Cout, K, pads, reflect, eligible
FP8_STAT_CASES = [
    ("c64",      2, 16, 16, 128,  64, 3, (1, 1, 1, 1), True,  True),
    ("c128",     2, 16, 16, 128, 128, 3, (1, 1, 1, 1), True,  True),
    ("c64_b3",   3, 16, 16, 128,  64, 3, (1, 1, 1, 1), True,  True),
    ("k4_disc",  2, 16, 16, 128,  64, 4, (1, 2, 1, 2), False, True),
    ("ktail",    2, 16, 16,  64,  64, 3, (1, 1, 1, 1), True,  True),
    ("12x12",    2, 12, 12, 128,  64, 3, (1, 1, 1, 1), True,  False),
    ("cout16",   2, 16, 16, 128,  16, 3, (1, 1, 1, 1), True,  False),
]


def _run_fp8_stats(case):
    _, B, H, W, Cin, Cout, K, pads, reflect, _ = case
    ext = backend.ext()
    x = mk((B, H, W, Cin), seed=311)
    w = mk((Cout, K, K, Cin), seed=312, scale=0.2)
    sx = torch.tensor([448.0], device=DEV)
    sw = torch.tensor([448.0 / 0.2], device=DEV)
    xq = ext.quant_fp8(x, sx)
    wq = ext.quant_fp8(w, sw)
    dq = 1.0 / (sx * sw)
    args = (xq, wq, dq, None, None, 1, *pads, reflect, 0, 0.2)
    return ext.conv2d_fp8_fwd_stats(*args), ext.conv2d_fp8_fwd(*args)


@pytest.mark.parametrize("case", FP8_STAT_CASES,
                         ids=[c[0] for c in FP8_STAT_CASES])
def test_fp8_conv_slabs_match_tensor(case):
    """Bound as derived in test_in_epilogue_gpu.py::
    test_epilogue_slabs_match_tensor: the slabs add the same n = OH*OW
    stored bf16 values as the reference in another order, so
    |slab - ref| <= 2*n*u*sum|v| (sums) and 2*n*u*sum(v^2) (squares),
    u = 2^-24."""
    elig = case[-1]
    out, plain = _run_fp8_stats(case)
    y = out[0]
    assert torch.equal(y, plain)
    assert y.float().abs().max().item() > 0
    if not elig:
        assert len(out) == 1, "ineligible shape must not emit slabs"
        return
    assert len(out) == 3, "eligible shape must emit slabs"
    psum, psq = out[1], out[2]
    b_, OH, OW, C = y.shape
    assert tuple(psum.shape) == (OH * OW // 128, b_, C)
    assert psq.shape == psum.shape
    n = OH * OW
    u = 2.0 ** -24
    yf = y.float()
    ref_s = yf.sum((1, 2))
    ref_q = (yf ** 2).sum((1, 2))
    abs_s = yf.abs().sum((1, 2))
    err_s = ((psum.sum(0) - ref_s).abs() / (2 * n * u * abs_s)).max().item()
    err_q = ((psq.sum(0) - ref_q).abs() / (2 * n * u * ref_q)).max().item()
    print(f"{case[0]}: sum err/bound {err_s:.3f}, sumsq err/bound {err_q:.3f}")
    assert err_s <= 1.0 and err_q <= 1.0
    out2, _ = _run_fp8_stats(case)
    assert torch.equal(out2[1], psum) and torch.equal(out2[2], psq)


def test_fp8_slabs_path_equals_reduce_path():
    """test_slabs_path_equals_reduce_path with an fp8-conv producer: the
    statistics differ only by fp32 summation order, which moves an output
    across at most one bf16 rounding boundary (2^-7 relative)."""
    ext = backend.ext()
    out, _ = _run_fp8_stats(FP8_STAT_CASES[1])
    h, psum, psq = out
    g, b = _affine(h.shape[3])
    y0, m0, r0 = ext.instnorm_fwd(h, g, b, 1e-3, 1, 0.2, None)
    y1, m1, r1 = ext.instnorm_fwd(h, g, b, 1e-3, 1, 0.2, None, psum, psq,
                                  psum.shape[0])
    check_elem(y1, y0, 2.0 ** -7, "fp8 slabs-vs-reduce:y")
    check_elem(m1, m0, 2.0 ** -7, "fp8 slabs-vs-reduce:mean")
    check_elem(r1, r0, 2.0 ** -7, "fp8 slabs-vs-reduce:rstd")


# --------------------------------------------------------------- hand-off ---
def _block():
    torch.manual_seed(0)
    blk = ResBlock(256).to(DEV)
    with torch.no_grad():  # gammas of N(0, 0.02) would leave y ~ the residual
        blk.norm1.gamma.normal_(0.0, 0.5)
        blk.norm2.gamma.normal_(0.0, 0.5)
    return blk


def test_resblock_first_step_quantises_later_steps_hand_off(fp8_on, monkeypatch):
    blk = _block()
    x = mk((12, 16, 16, 256), seed=321)
    cnt = QuantCounter(monkeypatch)
    blk(x)
    assert cnt.n == 2, "first step: both convs bootstrap and quantise"
    fp8_state.roll()
    cnt.n = 0
    blk(x)
    assert cnt.n == 1, "later steps: only conv1 (test-made input) quantises"
    h1 = blk.conv1(x)
    assert getattr(h1, IN_SLABS_ATTR, None) is not None
    psum, psq = getattr(h1, IN_SLABS_ATTR)
    assert tuple(psum.shape) == (2, 12, 256)
    h = blk.norm1(h1, fp8_consumer=blk.conv2.fp8_hint())
    yq, prev = getattr(h, FP8_TWIN_ATTR)
    assert yq.shape == h.shape and yq.dtype == torch.uint8
    assert prev is fp8_state.peek(blk.conv2.weight)[0]


def test_no_twin_before_the_consumer_has_a_slot(fp8_on):
    blk = _block()
    x = mk((12, 16, 16, 256), seed=322)
    h = blk.norm1(blk.conv1(x), fp8_consumer=blk.conv2.fp8_hint())
    assert getattr(h, FP8_TWIN_ATTR, None) is None
    assert fp8_state.peek(blk.conv2.weight) is None


def test_twin_path_equals_standalone_path(fp8_on, monkeypatch):
    blk = _block()
    x = mk((12, 16, 16, 256), seed=323)
    blk(x)
    fp8_state.roll()
    w2 = blk.conv2.weight
    cnt = QuantCounter(monkeypatch)
    with torch.no_grad():
        y = blk.norm1(blk.conv1(x), fp8_consumer=blk.conv2.fp8_hint())
        assert getattr(y, FP8_TWIN_ATTR, None) is not None
        cnt.n = 0
        a = ops.conv2d(y, w2, None, 1, (1, 1, 1, 1), "reflect")
        assert cnt.n == 0
        b = ops.conv2d(y.detach().clone(), w2, None, 1, (1, 1, 1, 1), "reflect")
        assert cnt.n == 1
    assert torch.equal(a, b)

    # gradients: hinted run vs CYG_NO_FP8_TWIN=1 run, slabs off in both so
    # only the twin differs
    monkeypatch.setenv("CYG_NO_FP8_STATS", "1")

    def run():
        xg = x.clone().requires_grad_(True)
        for p in blk.parameters():
            p.grad = None
        out = blk(xg)
        out.float().sum().backward(retain_graph=True)
        grads = {"dx": xg.grad}
        grads.update((n, p.grad.clone()) for n, p in blk.named_parameters())
        return out, grads

    cnt.n = 0
    out_t, g_t = run()
    assert cnt.n == 1
    monkeypatch.setenv("CYG_NO_FP8_TWIN", "1")
    cnt.n = 0
    out_s, g_s = run()
    assert cnt.n == 2
    assert torch.equal(out_t, out_s)
    for n in g_t:
        d = (g_t[n].float() - g_s[n].float()).abs().max().item()
        print(f"{n}: max |diff| {d:.3e}")
    # Forward outputs and every tensor saved for backward are bit-equal, and
    # backward is the same code in both runs. dx and the conv weight grads
    # come out of fixed-order reductions: bit-equal.
    for n in ("dx", "conv1.weight", "conv2.weight"):
        assert torch.equal(g_t[n], g_s[n]), n
    # dgamma/dbeta: instnorm_bwd folds the B per-sample partials t_b (each a
    # fixed-order slab sum, identical in both runs) into one fp32 word per
    # channel with atomicAdd, in arrival order. Two runs of the SAME code
    # may differ there, so bit-equality cannot be asked of any pair of runs
    # (measured here: norm1.gamma 4.5e-13 on values ~1e-6, norm1.beta
    # 1.1e-13, the others 0). What two orders of one fp32 sum of B terms
    # can differ by is at most 2*(B-1)*u*sum_b|t_b|, u = 2^-24 (each order
    # is within (B-1)*u*sum|t_b| of the exact sum). |t_b| is read off a
    # backward pass of sample b's loss alone: the other samples then add
    # exact zeros.
    B = x.shape[0]
    norm_names = ["norm1.gamma", "norm1.beta", "norm2.gamma", "norm2.beta"]
    params = dict(blk.named_parameters())
    tabs = {n: torch.zeros_like(params[n]) for n in norm_names}
    for b_ in range(B):
        gs = torch.autograd.grad(out_s[b_].float().sum(),
                                 [params[n] for n in norm_names],
                                 retain_graph=True)
        for n, g in zip(norm_names, gs):
            tabs[n] += g.abs()
    u = 2.0 ** -24
    for n in norm_names:
        bound = 2 * (B - 1) * u * tabs[n]
        err = (g_t[n] - g_s[n]).abs()
        worst = (err / bound.clamp(min=1e-38)).max().item()
        print(f"{n}: worst err/bound {worst:.3f}")
        assert (err <= bound).all(), n


def test_twin_for_another_weight_is_ignored(fp8_on, monkeypatch):
    blk = _block()
    x = mk((12, 16, 16, 256), seed=324)
    blk(x)                      # conv1.weight and conv2.weight own slots
    fp8_state.roll()
    wa, wb = blk.conv2.weight, blk.conv1.weight
    cnt = QuantCounter(monkeypatch)
    with torch.no_grad():
        y = blk.norm1(blk.conv1(x), fp8_consumer=ops.Fp8Consumer(wa, 1))
        assert getattr(y, FP8_TWIN_ATTR)[1] is fp8_state.peek(wa)[0]
        cnt.n = 0
        got = ops.conv2d(y, wb, None, 1, (1, 1, 1, 1), "reflect")
        assert cnt.n == 1, "a twin made for another layer must not be used"
        ref = ops.conv2d(y.detach().clone(), wb, None, 1, (1, 1, 1, 1), "reflect")
    assert torch.equal(got, ref)


def test_generator_forward_without_standalone_quant(fp8_on, monkeypatch):
    torch.manual_seed(0)
    m = Generator(num_residual_blocks=2).to(DEV)
    x = mk((12, 64, 64, 3), seed=325)
    cnt = QuantCounter(monkeypatch)
    with torch.no_grad():
        m(x)
        assert cnt.n == 4
        fp8_state.roll()
        monkeypatch.setenv("CYG_NO_FP8_STATS", "1")
        cnt.n = 0
        on = m(x)
        assert cnt.n == 0
        monkeypatch.setenv("CYG_NO_FP8_TWIN", "1")
        off = m(x)
        assert cnt.n == 4
        assert torch.equal(on, off)
        monkeypatch.delenv("CYG_NO_FP8_STATS")
        monkeypatch.delenv("CYG_NO_FP8_TWIN")
        cnt.n = 0
        full = m(x)
        assert cnt.n == 0
    assert torch.isfinite(full.float()).all()


def test_fp8_trainer_two_steps(fp8_on, tmp_path):
    from cyclegan_amd.parallel import DistContext
    from cyclegan_amd.trainer import CycleGAN
    a = argparse.Namespace()
    a.output_dir = str(tmp_path)
    a.batch_size = 1
    a.global_batch_size = 1
    a.num_residual_blocks = 1
    a.compute_dtype = torch.bfloat16
    a.fp8 = True
    torch.manual_seed(0)
    ctx = DistContext(device=torch.device("cuda", 0))
    gan = CycleGAN(a, ctx)
    x = torch.rand(1, 64, 64, 3, device=ctx.device, dtype=torch.bfloat16)
    for _ in range(2):
        r = gan.train_step(x, x)
        torch.cuda.synchronize()
        for k, v in r.items():
            assert torch.isfinite(v), k
