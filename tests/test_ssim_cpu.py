"""ops.SSIM on the CPU: the torch reference against a brute-force
definition and closed forms, its gradient and the adjoint formula the
backward kernel implements, the error paths, the trainer's --cycle_ssim /
--test_ssim wiring, and a self-test of the GPU test's bound (wrong variants
fall outside it, the fp32 reference inside)."""

import argparse

import pytest
import torch

import _ssim_cases as sc
from cyclegan_amd import ops
from cyclegan_amd.ops import ssim as S
from cyclegan_amd.trainer import CycleGAN

C1, C2 = 0.0004, 0.0036


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1,
            torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1)


# ---- the reference itself ----

@pytest.mark.parametrize("shape", [(1, 11, 11, 1), (2, 12, 13, 3),
                                   (1, 15, 11, 3)])
def test_reference_matches_bruteforce_definition(shape):
    x, y = _rand(shape, 1)
    got = ops.SSIM(x, y)
    want = sc.ssim_bruteforce(x, y)
    assert got.dtype == torch.float64 and got.shape == (shape[0],)
    assert (got - want).abs().max().item() <= 1e-12


def test_constants_and_window():
    assert S.C1 == pytest.approx(C1, rel=1e-12)
    assert S.C2 == pytest.approx(C2, rel=1e-12)
    g = S.gaussian_window(torch.float64)
    assert g.shape == (11,) and abs(g.sum().item() - 1.0) < 1e-15
    assert torch.equal(g, g.flip(0))
    assert g[5] / g[4] == pytest.approx(float(torch.exp(torch.tensor(
        1.0 / 4.5, dtype=torch.float64))), rel=1e-12)


def test_closed_forms():
    x, y = _rand((2, 14, 17, 3), 2)
    one = torch.ones(2, dtype=torch.float64)
    assert (ops.SSIM(x, x) - one).abs().max().item() <= 1e-12
    sxy, syx = ops.SSIM(x, y), ops.SSIM(y, x)
    assert (sxy - syx).abs().max().item() <= 1e-14
    for v in (sxy, ops.SSIM(x, -x), ops.SSIM(x, 0.3 * y)):
        assert (v >= -1).all() and (v <= 1).all()
    # constant images: zero variances, S = (2pq + c1) / (p^2 + q^2 + c1)
    for p, q in ((0.5, -0.25), (1.0, 1.0), (-1.0, 1.0), (0.0, 0.7)):
        a = torch.full((1, 12, 11, 2), p, dtype=torch.float64)
        b = torch.full((1, 12, 11, 2), q, dtype=torch.float64)
        want = (2 * p * q + C1) / (p * p + q * q + C1)
        assert abs(ops.SSIM(a, b).item() - want) <= 1e-9


def test_fp32_path_returns_fp32():
    x, y = _rand((2, 12, 13, 3), 3)
    out = ops.SSIM(x.float(), y.float())
    assert out.dtype == torch.float32
    assert (out.double() - ops.SSIM(x, y)).abs().max().item() < 1e-5
    # bf16 inputs compute in fp32, like MAE
    outb = ops.SSIM(x.bfloat16(), y.bfloat16())
    assert outb.dtype == torch.float32


# ---- gradient ----

def test_gradcheck_reference_fp64():
    x, y = _rand((1, 12, 13, 2), 4)
    x.requires_grad_(True)
    y.requires_grad_(True)
    assert torch.autograd.gradcheck(ops.SSIM, (x, y), eps=1e-6, atol=1e-7)


@pytest.mark.parametrize("shape", [(1, 12, 13, 2), (3, 11, 24, 3)])
def test_adjoint_formula_matches_autograd(shape):
    """dL/dy = dout/N [G^T a + 2 y G^T b + x G^T c], and the swapped call
    for y_true: what the backward kernel computes."""
    x, y = _rand(shape, 5)
    dout = sc.dout_for(shape[0])
    xr, yr = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    gx, gy = torch.autograd.grad((ops.SSIM(xr, yr) * dout).sum(), (xr, yr))
    fy = S.ssim_grad_from_maps(x, y, dout)
    fx = S.ssim_grad_from_maps(y, x, dout)
    assert (fy - gy).abs().max().item() <= 1e-12
    assert (fx - gx).abs().max().item() <= 1e-12
    assert gy.abs().max().item() > 1e-4  # not a comparison of zeros


def test_save_maps_follows_grad_mode():
    """Which maps the GPU forward is asked for: none under no_grad even
    for inputs that require grad, as in the test epoch."""
    t, p = torch.zeros(1, 11, 11, 1), torch.zeros(1, 11, 11, 1)
    tg, pg = t.clone().requires_grad_(True), p.clone().requires_grad_(True)
    assert S._save_maps(t, p) == 0
    assert S._save_maps(t, pg) == 1
    assert S._save_maps(tg, p) == 2 and S._save_maps(tg, pg) == 2
    with torch.no_grad():
        assert S._save_maps(t, pg) == 0 and S._save_maps(tg, pg) == 0
    with torch.enable_grad():
        assert S._save_maps(t, pg) == 1


# ---- error paths ----

@pytest.mark.parametrize("shape", [(1, 10, 11, 3), (1, 11, 10, 3),
                                   (2, 10, 10, 1)])
def test_too_small_raises(shape):
    t = torch.zeros(shape)
    with pytest.raises(ValueError):
        ops.SSIM(t, t)


def test_shape_mismatch_raises():
    with pytest.raises(ValueError):
        ops.SSIM(torch.zeros(1, 12, 12, 3), torch.zeros(1, 12, 13, 3))


def test_parse_args_cycle_ssim():
    from main import parse_args
    for bad in ("1.5", "-0.1", "nan"):
        with pytest.raises(SystemExit):
            parse_args(["--cycle_ssim", bad])
    a = parse_args([])
    assert a.cycle_ssim == 0.0 and a.test_ssim is False
    assert parse_args(["--test_ssim"]).test_ssim is True
    a = parse_args(["--cycle_ssim", "0.25"])
    assert a.cycle_ssim == 0.25 and a.test_ssim is True  # implied
    assert parse_args(["--cycle_ssim", "1"]).cycle_ssim == 1.0


# ---- trainer ----

TODAY_TEST_KEYS = (
    "loss_G/loss", "loss_G/cycle", "loss_G/identity", "loss_G/total",
    "loss_F/loss", "loss_F/cycle", "loss_F/identity", "loss_F/total",
    "loss_X/loss", "loss_Y/loss", "error/MAE(X, F(G(X)))",
    "error/MAE(Y, G(F(Y)))", "error/MAE(X, F(X))", "error/MAE(Y, G(Y))")
SSIM_KEYS = ("error/SSIM(X, F(G(X)))", "error/SSIM(Y, G(F(Y)))")


def _gan(tmp_path, ctx, **extra):
    a = argparse.Namespace(output_dir=str(tmp_path), batch_size=2,
                           global_batch_size=2, num_residual_blocks=1,
                           compute_dtype=torch.float32, **extra)
    torch.manual_seed(0)
    return CycleGAN(a, ctx)


def _batch():
    g = torch.Generator().manual_seed(9)
    return (torch.rand(2, 32, 32, 3, generator=g) * 2 - 1,
            torch.rand(2, 32, 32, 3, generator=g) * 2 - 1)


@pytest.mark.parametrize("extra", [{}, {"cycle_ssim": 0.0},
                                   {"cycle_ssim": 0, "test_ssim": False}])
def test_trainer_off_is_unchanged(tmp_path, local_ctx, extra):
    x, y = _batch()
    base, gan = _gan(tmp_path, local_ctx), _gan(tmp_path, local_ctx, **extra)
    t0, t1 = base.test_step(x, y), gan.test_step(x, y)
    assert tuple(t1) == TODAY_TEST_KEYS == CycleGAN._TEST_KEYS
    assert tuple(gan.test_step(x[:0], y[:0])) == TODAY_TEST_KEYS
    for k in t0:
        assert torch.equal(t0[k], t1[k]), k
    r0, r1 = base.train_step(x, y), gan.train_step(x, y)
    assert tuple(r1) == CycleGAN._TRAIN_KEYS
    for k in r0:
        assert torch.equal(r0[k], r1[k]), k
    for n in base.groups:
        assert torch.equal(base.groups[n].flat_param,
                           gan.groups[n].flat_param), n


def test_trainer_cycle_loss_formula(tmp_path, local_ctx):
    w = 0.3
    x, y = _batch()
    gan = _gan(tmp_path, local_ctx, cycle_ssim=w)
    assert gan.test_ssim
    _, _, cycle_x, cycle_y = gan.cycle_step(x, y)
    want = {}
    for key, real, cyc in (("loss_G/cycle", y, cycle_y),
                           ("loss_F/cycle", x, cycle_x)):
        per = ((1 - w) * (real - cyc).abs().mean(dim=(1, 2, 3))
               + w * (1 - ops.SSIM(real, cyc)))
        want[key] = 10.0 * per.sum() / 2
    r = gan.train_step(x, y)  # losses are those of the pre-step weights
    assert len(r) == 10
    for key in want:
        assert abs(r[key].item() - want[key].item()) <= 1e-5 * abs(
            want[key].item()), key
    # and it is not the plain L1 value
    plain = _gan(tmp_path, local_ctx).train_step(x, y)
    assert abs(plain["loss_G/cycle"].item() - r["loss_G/cycle"].item()) > 1e-3


def test_trainer_ssim_term_reaches_F_gradient(tmp_path, local_ctx):
    x, y = _batch()
    grads = []
    for extra in ({}, {"cycle_ssim": 0.3}):
        gan = _gan(tmp_path, local_ctx, **extra)
        losses = gan._forward_losses(x, y)
        g = torch.autograd.grad(losses["loss_F/total"], gan.groups["F"].params,
                                retain_graph=True)
        grads.append(torch.cat([t.reshape(-1) for t in g]))
        # the detached cycle input still holds: nothing reaches G from
        # F's total, with or without the SSIM term
        gg = torch.autograd.grad(losses["loss_F/total"],
                                 gan.groups["G"].params, allow_unused=True)
        assert all(t is None for t in gg)
    assert torch.isfinite(grads[1]).all()
    assert (grads[0] - grads[1]).abs().max().item() > 1e-4


@pytest.mark.parametrize("extra", [{"test_ssim": True}, {"cycle_ssim": 0.3}])
def test_trainer_test_keys_with_ssim(tmp_path, local_ctx, extra):
    x, y = _batch()
    gan = _gan(tmp_path, local_ctx, **extra)
    r = gan.test_step(x, y)
    assert tuple(r) == TODAY_TEST_KEYS + SSIM_KEYS
    _, _, cycle_x, cycle_y = gan.cycle_step(x, y)
    assert torch.equal(r[SSIM_KEYS[0]], ops.SSIM(x, cycle_x).sum() / 2)
    assert torch.equal(r[SSIM_KEYS[1]], ops.SSIM(y, cycle_y).sum() / 2)
    z = gan.test_step(x[:0], y[:0])  # empty DP slice
    assert tuple(z) == TODAY_TEST_KEYS + SSIM_KEYS
    assert all(v.item() == 0 for v in z.values())
    # the class-level tuple is untouched: other instances keep today's keys
    assert CycleGAN._TEST_KEYS == TODAY_TEST_KEYS
    if "cycle_ssim" not in extra:  # the metric alone leaves the loss alone
        base = _gan(tmp_path, local_ctx).test_step(x, y)
        for k in base:
            assert torch.equal(base[k], r[k]), k


def test_trainer_rejects_bad_weight(tmp_path, local_ctx):
    with pytest.raises(ValueError):
        _gan(tmp_path, local_ctx, cycle_ssim=1.5)


# ---- the GPU test's bound can fail ----

SELF_SHAPES = sc.SHAPES


@pytest.mark.parametrize("shape", SELF_SHAPES, ids=str)
def test_bound_rejects_wrong_variants(shape):
    """On the GPU test's own inputs, each wrong variant misses the forward
    bound: on the noise, low-pass, flat and saturated kinds at every shape
    (y == x gives S = 1 under every variant, and cannot tell)."""
    for kind in ("noise", "lowpass", "flat", "saturated"):
        o = sc.oracle(shape, kind)
        bound = sc.fwd_bound(o["e32"])
        right = sc.ssim_variant(o["x"], o["y"], "right")
        assert (right - o["out"]).abs().max().item() <= 1e-12
        for v in sc.WRONG_VARIANTS:
            err = (sc.ssim_variant(o["x"], o["y"], v)
                   - o["out"]).abs().max().item()
            assert err > bound, (kind, v, err, bound)


@pytest.mark.parametrize("shape", SELF_SHAPES, ids=str)
def test_bound_accepts_fp32_reference(shape):
    """The fp32 reference sits inside the bounds. For the reference itself
    that holds by construction (e32 <= max(8 e32, 2^-20), likewise e32g);
    what can fail here is: e32 of fp32 size, an INDEPENDENT fp32 gradient
    (the written-out adjoint formula, other operations in another order
    than autograd's) inside the gradient bound, and S = 1, gradient 0 at
    y == x. There is no such independent check of the forward bound: a
    plain fp32 sum over the 2-D 11x11 window misses it on the nearly flat
    kind (14x at one window, E[x^2] - mx^2 cancelling), which is why the
    kernel takes its moments about a pivot pixel."""
    for kind in sc.KINDS:
        o = sc.oracle(shape, kind)
        assert o["e32"] <= sc.fwd_bound(o["e32"])
        assert o["e32"] <= 2e-5, (kind, o["e32"])  # an fp32-sized error
        for gk, ek in (("gx", "e32gx"), ("gy", "e32gy")):
            assert o[ek] <= sc.grad_bound(o[gk], o[ek]).min().item()
        d32 = o["dout"].float()
        for gk, a, b in (("gy", o["x"], o["y"]), ("gx", o["y"], o["x"])):
            g32 = S.ssim_grad_from_maps(a, b, d32)
            assert g32.dtype == torch.float32
            err = (g32.double() - o[gk]).abs()
            assert (err <= sc.grad_bound(o[gk], o["e32" + gk])).all(), (
                kind, gk)
        if kind == "same":
            assert (o["out"] - 1).abs().max().item() <= 1e-12
            assert o["gy"].abs().max().item() <= 1e-12
