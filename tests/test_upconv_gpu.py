"""Resize-convolution on the GPU: the shadow_fold arena refresh, the op's
forward / dgrad / wgrad against the fp64 naive formulation under the
derived bounds of tests/_upconv_bounds.py, the gradient unfold on its own,
the InstanceNorm slab hand-off and the trainer (eager, EMA swap, captured
step) with --upsample resize."""

import argparse

import pytest
import torch

import _kernel_bounds as kb
import _upconv_bounds as ub
from _kernel_bounds import U32, assert_within, uniform_bf16
from cyclegan_amd import ops
from cyclegan_amd.models import ConvNHWC, UpsampleConvNHWC
from cyclegan_amd.ops import backend, shadow
from cyclegan_amd.ops.conv import IN_SLABS_ATTR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = torch.float64


def dev(t):
    return t.to(DEV).contiguous()


# ---------------------------------------------------------- shadow_fold ----
def test_shadow_fold_arena():
    from cyclegan_amd.ops.arena import ShadowArena
    from cyclegan_amd.parallel import FlatParamGroup
    torch.manual_seed(0)
    mod = torch.nn.Sequential(UpsampleConvNHWC(16, 8),
                              ConvNHWC(16, 16, 3, bias=True)).to(DEV)
    up, conv = mod[0], mod[1]
    group = FlatParamGroup(mod)
    arena = ShadowArena(group, mod)
    assert arena.fold_idx.shape == (2 * 8 * 16 * 16, 4)

    def check(tag):
        w = up.weight.detach().cpu()
        f = arena.forms_of(up.weight)
        assert f["up"].shape == (8, 4, 4, 16) and f["up_t"].shape == (16, 4, 4, 8)
        assert_within(f["up"], *ub.delta_v(w), f"{tag}:up", "okki")
        assert torch.equal(f["up_t"], f["up"].permute(3, 1, 2, 0).contiguous())
        # the same bits as the torch build (same terms, same order)
        assert torch.equal(f["up"].cpu(), shadow._fold_up_weight_torch(w)
                           .to(torch.bfloat16))
        # the gather segment: today's values, bit for bit
        g = arena.forms_of(conv.weight)
        want = conv.weight.detach().to(torch.bfloat16)
        assert torch.equal(g["p"], want)
        assert torch.equal(g["tp"], want.permute(3, 1, 2, 0).contiguous())
        assert torch.equal(arena.forms_of(conv.bias)["bias_p"],
                           conv.bias.detach().to(torch.bfloat16))

    check("init")
    before = arena.forms_of(up.weight)["up"].clone()
    with torch.no_grad():
        group.flat_param.mul_(-1.7).add_(0.013)
    group.bump_versions()
    arena.refresh()
    assert not torch.equal(arena.forms_of(up.weight)["up"], before)
    check("after update")


# ------------------------------------------------- op vs the fp64 naive ----
CASES = [ub.up_case(n, s) for n, s in ub.GPU_SHAPES.items()]
_runs = {}


def run(case):
    """One forward + backward of the op per case, shared by the tests:
    (x, w, dy) on the CPU and (y, dx, dw, vb) as computed."""
    if case.id not in _runs:
        i = list(ub.GPU_SHAPES).index(case.id)
        x = uniform_bf16(case.x_shape, 100 + 10 * i)
        w = ub.master((case.Cout, 3, 3, case.Cin), 101 + 10 * i)
        dy = uniform_bf16(case.y_shape, 102 + 10 * i)
        xg = dev(x).requires_grad_(True)
        wg = dev(w).requires_grad_(True)
        y = ops.upsample_conv2d(xg, wg)
        vb = shadow.compute_weight_up(wg, xg).detach().cpu()
        y.backward(dev(dy))
        _runs[case.id] = (x, w, dy, y.detach().cpu(), xg.grad.cpu(),
                          wg.grad.cpu(), vb)
    return _runs[case.id]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_forward(case):
    x, w, _, y, _, _, vb = run(case)
    assert tuple(y.shape) == case.y_shape and y.dtype == torch.bfloat16
    assert vb.dtype == torch.bfloat16 and tuple(vb.shape) == case.w_shape
    assert_within(vb, *ub.delta_v(w), f"{case.id}:V", "okki")
    assert_within(y, *ub.fwd_bound(case, x, w, vb), f"{case.id}:y")


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_dgrad(case):
    _, w, dy, _, dx, _, vb = run(case)
    assert tuple(dx.shape) == case.x_shape
    assert_within(dx, *ub.dgrad_bound(case, dy, w, vb), f"{case.id}:dx")


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_wgrad(case):
    x, _, dy, _, _, dw, _ = run(case)
    assert dw.dtype == torch.float32
    assert tuple(dw.shape) == (case.Cout, 3, 3, case.Cin)
    ref, bound, _, _ = ub.dw_bound(case, x, dy)
    assert_within(dw, ref, bound, f"{case.id}:dw", "okki")


def test_forward_fused_relu():
    case = ub.up_case("ntile", ub.GPU_SHAPES["ntile"])
    x, w = run(case)[:2]
    y = ops.upsample_conv2d(dev(x), dev(w), act="relu")
    vb = shadow.compute_weight_up(dev(w), dev(x)).cpu()
    assert (y >= 0).all()
    assert_within(y, *ub.fwd_bound(case, x, w, vb, "relu"), "ntile:relu:y")


def test_weight_without_grad_gets_none():
    case = ub.up_case("ntile", ub.GPU_SHAPES["ntile"])
    x, w, dy = run(case)[:3]
    xg = dev(x).requires_grad_(True)
    wg = dev(w)
    ops.upsample_conv2d(xg, wg).backward(dev(dy))
    assert wg.grad is None
    assert_within(xg.grad, *ub.dgrad_bound(case, dy, w, run(case)[6]),
                  "ntile:dx, w without grad")


# --------------------------------------------- fold_upconv_dw_into alone ----
@pytest.mark.parametrize("transposed", [False, True])
def test_fold_upconv_dw_into(transposed):
    """dw = M^T dV M in fp32, at most four terms: within 4*u32*fold|dV| of
    the fp64 fold; accumulating adds one rounding of the sum,
    u32*(|base| + fold|dV|*(1 + 4*u32)). Stores stay inside ``out``."""
    ext = backend.ext()
    O, I, guard = 24, 64, 256
    g = torch.Generator().manual_seed(7)
    dv = torch.randn(O, 4, 4, I, generator=g)
    arg = dv.permute(3, 1, 2, 0).contiguous() if transposed else dv
    n = O * 9 * I
    base = torch.randn(n + 2 * guard, generator=g)
    buf = dev(base)
    out = buf[guard:guard + n].view(O, 3, 3, I)
    ref = ub.unfold(dv.to(D))
    F = ub.unfold(dv.to(D).abs())

    ext.fold_upconv_dw_into(dev(arg), out, False, transposed)
    assert_within(out, ref, 4 * U32 * F, f"fold:t{int(transposed)}", "okki")
    stored = out.cpu().clone()

    ext.fold_upconv_dw_into(dev(arg), out, True, transposed)
    ref2 = stored.to(D) + ref
    b2 = 4 * U32 * F + U32 * (stored.to(D).abs() + F * (1 + 4 * U32))
    assert_within(out, ref2, b2, f"fold+acc:t{int(transposed)}", "okki")

    got = buf.cpu()
    assert torch.equal(got[:guard], base[:guard])
    assert torch.equal(got[-guard:], base[-guard:])


# ------------------------------------------------------- InstanceNorm ----
def test_instance_norm_picks_up_the_slabs():
    case = ub.up_case("in", (1, 16, 16, 64, 64))
    x = uniform_bf16(case.x_shape, 61)
    w = ub.master((64, 3, 3, 64), 62)
    g = torch.Generator().manual_seed(63)
    gamma = torch.randn(64, generator=g) * 0.5
    beta = torch.randn(64, generator=g) * 0.1
    y = ops.upsample_conv2d(dev(x), dev(w))
    slabs = getattr(y, IN_SLABS_ATTR, None)
    assert slabs is not None, "the op's output carries no InstanceNorm slabs"
    assert tuple(slabs[0].shape[1:]) == (1, 64)
    with_slabs = ops.instance_norm(y, dev(gamma), dev(beta))
    plain = ops.instance_norm(y.clone(), dev(gamma), dev(beta))
    (ry, _, _), (by, _, _), _ = kb.in_ref_bounds(y.cpu(), gamma, beta, 1e-3)
    assert_within(plain, ry, by, "in:plain")
    assert_within(with_slabs, ry, by, "in:slabs")


# ------------------------------------------------------------- trainer ----
def make_args(tmp_path, batch=2, nrb=2, **kw):
    return argparse.Namespace(
        output_dir=str(tmp_path), batch_size=batch, global_batch_size=batch,
        num_residual_blocks=nrb, compute_dtype=torch.bfloat16,
        upsample="resize", **kw)


def _up_view_is_fold_of_masters(gan):
    for up in gan.G.ups[::2]:
        view = shadow.compute_weight_up(
            up.weight, torch.empty(1, device=DEV, dtype=torch.bfloat16))
        assert view is gan.arenas["G"].forms_of(up.weight)["up"]
        want = shadow._fold_up_weight_torch(up.weight.detach().cpu())
        assert torch.equal(view.cpu(), want.to(torch.bfloat16))


def test_gpu_losses_track_cpu_fp32(tmp_path):
    from cyclegan_amd.parallel import DistContext
    from cyclegan_amd.trainer import CycleGAN
    g = torch.Generator().manual_seed(5)
    x = torch.rand(1, 64, 64, 3, generator=g) * 2 - 1
    y = torch.rand(1, 64, 64, 3, generator=g) * 2 - 1

    torch.manual_seed(7)
    gan_g = CycleGAN(make_args(tmp_path, batch=1, ema_decay=0.999),
                     DistContext(device=torch.device("cuda", 0)))
    torch.manual_seed(7)
    args = make_args(tmp_path, batch=1, ema_decay=0.999)
    args.compute_dtype = torch.float32
    gan_c = CycleGAN(args, DistContext(device=torch.device("cpu")))

    def compare(tag):
        r_gpu, r_cpu = gan_g.test_step(x, y), gan_c.test_step(x, y)
        for k in r_cpu:
            a, b = r_gpu[k].item(), r_cpu[k].item()
            print(f"{tag} {k}: gpu {a:.5f} cpu {b:.5f}")
            assert abs(a - b) <= 0.05 * (abs(b) + 0.05), (tag, k, a, b)

    compare("live")
    # the folded forms follow the weight swap: give both trainers the same
    # distinct averages, then evaluate inside ema_weights()
    for gan in (gan_g, gan_c):
        for n in "GF":
            gan.optimizers[n].ema.mul_(0.5)
    live = shadow.compute_weight_up(
        gan_g.G.ups[0].weight, torch.empty(1, device=DEV,
                                           dtype=torch.bfloat16)).clone()
    with gan_g.ema_weights(), gan_c.ema_weights():
        _up_view_is_fold_of_masters(gan_g)
        assert not torch.equal(gan_g.arenas["G"].forms_of(
            gan_g.G.ups[0].weight)["up"], live)
        compare("ema")
    assert torch.equal(gan_g.arenas["G"].forms_of(
        gan_g.G.ups[0].weight)["up"], live)


def test_graphed_step_matches_eager(tmp_path):
    """tests/test_train_gpu.py's captured-vs-eager contract with resize
    generators: the fold rides in the captured refresh, the unfold in the
    captured backward."""
    from cyclegan_amd.parallel import DistContext
    from cyclegan_amd.trainer import CycleGAN, GraphedStep
    ctx = DistContext(device=torch.device("cuda", 0))
    data = []
    g = torch.Generator().manual_seed(11)
    for _ in range(4):
        data.append((torch.rand(2, 64, 64, 3, generator=g) * 2 - 1,
                     torch.rand(2, 64, 64, 3, generator=g) * 2 - 1))

    torch.manual_seed(3)
    gan_e = CycleGAN(make_args(tmp_path), ctx)
    for x, y in data:
        r_e = gan_e.train_step(x, y)
    torch.cuda.synchronize()

    torch.manual_seed(3)
    gan_g = CycleGAN(make_args(tmp_path), ctx)
    for x, y in data[:2]:
        gan_g.train_step(x, y)
    step = GraphedStep(gan_g, *data[2], warmup=0)
    for x, y in data[2:]:
        r_g = step(x, y)
    torch.cuda.synchronize()

    assert all(o.t == 4 for o in gan_g.optimizers.values())
    for k in r_e:
        a, b = r_e[k].item(), r_g[k].item()
        print(f"{k}: eager {a:.5f} graphed {b:.5f}")
        assert abs(a - b) <= 0.03 * (abs(b) + 0.03), (k, a, b)
    d = (gan_e.groups["G"].flat_param - gan_g.groups["G"].flat_param)
    print(f"max |dG| {d.abs().max().item():.3e}")
    assert d.abs().max().item() < 2.5e-3
    grad = gan_g.G.ups[0].weight.grad
    assert grad.data_ptr() >= gan_g.groups["G"].flat_grad.data_ptr()
    assert torch.isfinite(grad).all() and grad.abs().sum().item() > 0
    _up_view_is_fold_of_masters(gan_g)
