"""ops.SSIM HIP kernels against the fp64 torch oracle, and the trainer's
--cycle_ssim / --test_ssim paths on the GPU.

Inputs are rounded to bf16 first and the oracle gets those same values.
Bounds (tests/_ssim_cases.py, proved able to fail by tests/test_ssim_cpu.py):

    forward   |kernel - fp64| <= max(8 * e32, 2^-20)            per case
    gradient  |kernel - g|    <= 2^-8 |g| + 8 * e32g + 2^-30    per element

with e32 / e32g the error of the fp32 torch reference on the CPU in that
case. Measured on this suite's inputs, max over the shapes (CPU):

    kind        e32       e32g (by y_pred)
    noise       1.8e-8    1.4e-8
    lowpass     6.9e-8    1.3e-7
    flat        3.9e-6    2.6e-6
    near        6.5e-8    2.3e-7
    same        0         5.2e-8
    saturated   1.5e-8    3.3e-8

so outside the flat kind the forward bound is its floor, 2^-20 = 9.5e-7.
"""

import argparse
import types

import pytest
import torch

import _ssim_cases as sc
from cyclegan_amd import ops
from cyclegan_amd.ops import backend
from cyclegan_amd.ops import ssim as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _dev(t, grad=False):
    return t.detach().to(DEV, torch.bfloat16).requires_grad_(grad)


def _check_fwd(out, o, what):
    err = (out.detach().double().cpu() - o["out"]).abs().max().item()
    bound = sc.fwd_bound(o["e32"])
    print(f"{what}: fwd err {err:.3e} bound {bound:.3e} e32 {o['e32']:.3e}")
    assert out.dtype == torch.float32 and out.shape == o["out"].shape
    assert err <= bound, (what, err, bound)


def _check_grad(got, o, which, what):
    assert got.dtype == torch.bfloat16 and got.shape == o[which].shape
    err = (got.double().cpu() - o[which]).abs()
    bound = sc.grad_bound(o[which], o["e32" + which])
    worst = (err / bound).max().item()
    print(f"{what}: {which} worst err/bound {worst:.3f} "
          f"e32g {o['e32' + which]:.3e} max|g| {o[which].abs().max():.3e}")
    assert worst <= 1.0, (what, which, worst)


def _run_case(shape, kind):
    o = sc.oracle(shape, kind)
    what = f"{shape} {kind}"
    dout = o["dout"].to(DEV, torch.float32)
    # gradient by y_pred alone (three maps), as the trainer asks for it
    x, y = _dev(o["x"]), _dev(o["y"], True)
    out = ops.SSIM(x, y)
    _check_fwd(out, o, what)
    (gy,) = torch.autograd.grad((out * dout).sum(), (y,))
    _check_grad(gy, o, "gy", what)
    # by both inputs (four maps, two backward launches)
    x, y = _dev(o["x"], True), _dev(o["y"], True)
    out = ops.SSIM(x, y)
    _check_fwd(out, o, what + " both")
    gx, gy = torch.autograd.grad((out * dout).sum(), (x, y))
    _check_grad(gx, o, "gx", what + " both")
    _check_grad(gy, o, "gy", what + " both")
    if kind == "same":
        assert (out.detach().cpu() - 1).abs().max().item() <= 2.0 ** -20


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("shape", sc.SHAPES, ids=str)
def test_kernel_matches_fp64_oracle(shape, kind):
    _run_case(shape, kind)


def test_kernel_full_size_once():
    _run_case(sc.BIG_SHAPE, "noise")


def test_y_true_gradient_skipped_when_not_needed():
    o = sc.oracle((2, 12, 13, 3), "noise")
    x, y = _dev(o["x"]), _dev(o["y"])
    res = backend.ext().ssim_fwd(x, y, 1)
    assert len(res) == 4
    ctx = types.SimpleNamespace(saved_tensors=(x, y, *res[1:]),
                                needs_input_grad=(False, True))
    gt, gp, none = S._SSIMFn.backward(ctx, o["dout"].to(DEV, torch.float32))
    assert gt is None and none is None
    _check_grad(gp, o, "gy", "direct backward")


def test_arguments_and_dispatch():
    ext = backend.ext()
    o = sc.oracle((2, 12, 13, 3), "noise")
    x, y = _dev(o["x"]), _dev(o["y"])
    # non-contiguous, mismatched shapes, small images, dtypes, devices
    xt = _dev(o["x"].permute(0, 2, 1, 3).contiguous()).permute(0, 2, 1, 3)
    assert xt.shape == y.shape and not xt.is_contiguous()
    with pytest.raises(RuntimeError):
        ops.SSIM(xt, y)
    with pytest.raises((RuntimeError, ValueError)):
        ops.SSIM(x, y[:, :, :12])
    with pytest.raises(RuntimeError):
        ext.ssim_fwd(x, y[:1].contiguous(), 0)
    with pytest.raises(ValueError):
        ops.SSIM(x[:, :10].contiguous(), y[:, :10].contiguous())
    with pytest.raises(RuntimeError):
        ext.ssim_fwd(x[:, :10].contiguous(), y[:, :10].contiguous(), 0)
    with pytest.raises(RuntimeError):
        ext.ssim_fwd(x[:, :, :10].contiguous(), y[:, :, :10].contiguous(), 0)
    with pytest.raises(RuntimeError):
        ext.ssim_fwd(x.float(), y.float(), 0)
    with pytest.raises(RuntimeError):
        ext.ssim_fwd(x, y.float(), 0)
    with pytest.raises(RuntimeError):
        ext.ssim_fwd(x.cpu(), y.cpu(), 0)
    with pytest.raises(RuntimeError):
        ext.ssim_fwd(x[0], y[0], 0)
    with pytest.raises(RuntimeError):
        ext.ssim_fwd(x, y, 3)
    maps = ext.ssim_fwd(x, y, 1)[1:]
    dout = o["dout"].to(DEV, torch.float32)
    with pytest.raises(RuntimeError):  # maps of another shape
        ext.ssim_bwd(x, y, maps[0][:, :1].contiguous(), maps[1], maps[2], dout)
    with pytest.raises(RuntimeError):
        ext.ssim_bwd(x, y, maps[0], maps[1], maps[2], dout[:1])
    with pytest.raises(RuntimeError):
        ext.ssim_bwd(x, y, maps[0], maps[1], maps[2], dout.double())
    # a contiguous view one element into its storage: 2-byte aligned only
    n = x.numel()
    fx = torch.zeros(n + 1, device=DEV, dtype=torch.bfloat16)
    fy = torch.zeros(n + 1, device=DEV, dtype=torch.bfloat16)
    fx[1:].copy_(x.reshape(-1))
    fy[1:].copy_(y.reshape(-1))
    vx, vy = fx[1:].view(x.shape), fy[1:].view(y.shape).requires_grad_(True)
    assert vx.data_ptr() % 4 == 2 and vx.is_contiguous()
    out = ops.SSIM(vx, vy)
    _check_fwd(out, o, "offset view")
    (gy,) = torch.autograd.grad((out * dout).sum(), (vy,))
    _check_grad(gy, o, "gy", "offset view")


def test_no_grad_forward_writes_no_maps(monkeypatch):
    """Under no_grad ops.SSIM asks the binding for no maps and allocates
    none, also when y_pred requires grad (needs_input_grad alone would say
    otherwise); the value is the one computed with gradients on."""
    ext = backend.ext()
    asked = []

    class Spy:
        def __getattr__(self, name):
            return getattr(ext, name)

        def ssim_fwd(self, yt, yp, save_maps):
            asked.append(save_maps)
            return ext.ssim_fwd(yt, yp, save_maps)

    monkeypatch.setattr(backend, "ext", lambda: Spy())
    # one block per sample: a single atomicAdd onto zero, bit-reproducible
    o = sc.oracle((2, 12, 13, 3), "noise")
    x, y = _dev(o["x"]), _dev(o["y"], True)
    assert len(ext.ssim_fwd(x, y, 0)) == 1
    assert len(ext.ssim_fwd(x, y, 1)) == 4
    assert len(ext.ssim_fwd(x, y, 2)) == 5
    with torch.no_grad():
        quiet = ops.SSIM(x, y)
        both = ops.SSIM(_dev(o["x"], True), y)
    assert asked == [0, 0]
    loud = ops.SSIM(x, y)
    ops.SSIM(_dev(o["x"], True), y)
    ops.SSIM(x, _dev(o["y"]))
    assert asked == [0, 0, 1, 2, 0]
    assert quiet.grad_fn is None and loud.grad_fn is not None
    assert torch.equal(quiet, loud.detach()) and torch.equal(quiet, both)
    del quiet, both, loud, x, y
    # at full size: the PEAK over the no_grad call stays below one map
    # (726 KB; the output is 4 bytes), with gradients on three are kept
    o = sc.oracle(sc.BIG_SHAPE, "noise")
    x, y = _dev(o["x"]), _dev(o["y"], True)
    map_bytes = 246 * 246 * 3 * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    m0 = torch.cuda.memory_allocated()
    with torch.no_grad():
        quiet = ops.SSIM(x, y)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - m0
    m1 = torch.cuda.memory_allocated()
    loud = ops.SSIM(x, y)
    m2 = torch.cuda.memory_allocated()
    assert peak < map_bytes // 2, peak
    assert m2 - m1 >= 3 * map_bytes, m2 - m1
    _check_fwd(quiet, o, "no_grad")
    _check_fwd(loud, o, "grad")


def test_graph_capture_forward_backward():
    shape = (2, 37, 45, 3)
    cases = [sc.oracle(shape, "noise"), sc.oracle(shape, "lowpass")]
    dout = cases[0]["dout"].to(DEV, torch.float32)
    sx = torch.zeros(shape, device=DEV, dtype=torch.bfloat16)
    sy = torch.zeros(shape, device=DEV, dtype=torch.bfloat16,
                     requires_grad=True)

    def step():
        out = ops.SSIM(sx, sy)
        (g,) = torch.autograd.grad((out * dout).sum(), (sy,))
        return out.detach(), g

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out, g_grad = step()
    for o in cases + cases[:1]:
        with torch.no_grad():
            sx.copy_(_dev(o["x"]))
            sy.copy_(_dev(o["y"]))
        graph.replay()
        torch.cuda.synchronize()
        _check_fwd(g_out, o, "replay")
        _check_grad(g_grad, o, "gy", "replay")
        e_out, e_grad = step()
        # eager on the same inputs: both within the bounds of one oracle,
        # so they differ by at most twice the bound
        assert (e_out - g_out).abs().max().item() <= 2 * sc.fwd_bound(o["e32"])
        lim = 2 * sc.grad_bound(o["gy"], o["e32gy"])
        assert ((e_grad.double() - g_grad.double()).abs().cpu() <= lim).all()


# ---- trainer ----

def make_args(tmp_path, batch=2, nrb=2, **extra):
    a = argparse.Namespace()
    a.output_dir = str(tmp_path)
    a.batch_size = batch
    a.global_batch_size = batch
    a.num_residual_blocks = nrb
    a.compute_dtype = torch.bfloat16
    for k, v in extra.items():
        setattr(a, k, v)
    return a


def test_trainer_test_step_matches_cpu_fp32(tmp_path):
    from cyclegan_amd.parallel import DistContext
    from cyclegan_amd.trainer import CycleGAN
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 64, 64, 3, generator=g) * 2 - 1
    y = torch.rand(2, 64, 64, 3, generator=g) * 2 - 1

    torch.manual_seed(7)
    gan_g = CycleGAN(make_args(tmp_path, cycle_ssim=0.5),
                     DistContext(device=DEV))
    r_gpu = gan_g.test_step(x, y)

    torch.manual_seed(7)
    args = make_args(tmp_path, cycle_ssim=0.5)
    args.compute_dtype = torch.float32
    gan_c = CycleGAN(args, DistContext(device=torch.device("cpu")))
    r_cpu = gan_c.test_step(x, y)

    assert tuple(r_gpu) == tuple(r_cpu) and len(r_cpu) == 16
    assert "error/SSIM(X, F(G(X)))" in r_cpu
    assert "error/SSIM(Y, G(F(Y)))" in r_cpu
    for k in r_cpu:
        a, b = r_gpu[k].item(), r_cpu[k].item()
        print(k, a, b)
        assert abs(a - b) <= 0.05 * (abs(b) + 0.05), (k, a, b)


def test_trainer_graphed_step_matches_eager(tmp_path):
    """The protocol and tolerances of test_train_gpu.py::
    test_graphed_step_matches_eager, with the SSIM term on."""
    from cyclegan_amd.parallel import DistContext
    from cyclegan_amd.trainer import CycleGAN, GraphedStep
    ctx = DistContext(device=DEV)
    data = []
    g = torch.Generator().manual_seed(11)
    for _ in range(4):
        data.append((torch.rand(2, 64, 64, 3, generator=g) * 2 - 1,
                     torch.rand(2, 64, 64, 3, generator=g) * 2 - 1))

    torch.manual_seed(3)
    gan_e = CycleGAN(make_args(tmp_path, cycle_ssim=0.5), ctx)
    for x, y in data:
        r_e = gan_e.train_step(x, y)
    torch.cuda.synchronize()

    torch.manual_seed(3)
    gan_g = CycleGAN(make_args(tmp_path, cycle_ssim=0.5), ctx)
    for x, y in data[:2]:
        gan_g.train_step(x, y)
    step = GraphedStep(gan_g, *data[2], warmup=0)
    for x, y in data[2:]:
        r_g = step(x, y)
    torch.cuda.synchronize()

    assert all(o.t == 4 for o in gan_g.optimizers.values())
    assert len(r_g) == 10
    for k in r_e:
        a, b = r_e[k].item(), r_g[k].item()
        assert abs(a - b) <= 0.03 * (abs(b) + 0.03), (k, a, b)
    d = (gan_e.groups["G"].flat_param - gan_g.groups["G"].flat_param)
    assert d.abs().max().item() < 2.5e-3


def test_trainer_weight_zero_is_todays_step(tmp_path):
    """cycle_ssim = 0 against a trainer built without the attribute, on
    what the GPU computes reproducibly.

    The losses of two trainers after one step are NOT all comparable with
    torch.equal, with or without this feature: at 64x64x3
    persample_loss_kernel adds six block partials per sample with
    atomicAdd in arrival order, and two trainers built WITHOUT the
    attribute agreed bitwise in 4 of 12 pairs (one ulp apart otherwise,
    only in the MAE-fed keys loss_*/cycle, loss_*/identity and through
    them loss_*/total). So:

    - the keys MAE does not feed are torch.equal between the trainers;
    - cycle_loss itself is torch.equal between the trainers, and to the
      expression written out, on tensors with ONE block per sample
      (32x32x3 = 3072 elements: a single atomicAdd onto zero), at the
      step's shapes otherwise;
    - the MAE-fed keys are torch.equal on the CPU, where the whole step is
      deterministic (test_ssim_cpu.py::test_trainer_off_is_unchanged)."""
    from cyclegan_amd.parallel import DistContext
    from cyclegan_amd.trainer import CycleGAN
    ctx = DistContext(device=DEV)
    g = torch.Generator().manual_seed(13)
    x = torch.rand(2, 64, 64, 3, generator=g) * 2 - 1
    y = torch.rand(2, 64, 64, 3, generator=g) * 2 - 1
    real = _dev(torch.rand(2, 32, 32, 3, generator=g) * 2 - 1)
    cyc = _dev(torch.rand(2, 32, 32, 3, generator=g) * 2 - 1)
    torch.manual_seed(3)
    gan0 = CycleGAN(make_args(tmp_path), ctx)
    torch.manual_seed(3)
    gan1 = CycleGAN(make_args(tmp_path, cycle_ssim=0), ctx)
    assert gan1.cycle_ssim == 0.0 and not gan1.test_ssim
    with torch.no_grad():
        c0, c1 = gan0.cycle_loss(real, cyc), gan1.cycle_loss(real, cyc)
        want = 10.0 * (ops.MAE(real, cyc).sum() / 2)
    assert torch.equal(c0, c1) and torch.equal(c1, want)
    r0, r1 = gan0.train_step(x, y), gan1.train_step(x, y)
    torch.cuda.synchronize()
    assert tuple(r1) == CycleGAN._TRAIN_KEYS
    for k in ("loss_G/loss", "loss_F/loss", "loss_X/loss", "loss_Y/loss"):
        assert torch.equal(r0[k], r1[k]), (k, r0[k].item(), r1[k].item())
    # The MAE-fed keys, up to the order of the atomics: a per-sample value
    # is a sum of six non-negative fp32 partials, each order within 5u of
    # the exact sum (u = 2^-24), so two orders within 10u of each other;
    # the batch sum, the scaling and the (all positive) totals round at
    # most a few times more. 16u relative; a changed expression (an extra
    # factor, another term) is off by far more, and exactly so on the CPU.
    for k in r0:
        a, b = r0[k].item(), r1[k].item()
        assert abs(a - b) <= 16 * 2.0 ** -24 * abs(b), (k, a, b)
