"""Linear learning-rate decay and generator weight EMA on the CPU path (the
oracle of the fused kernel): the schedule function, the parser, FusedAdam's
lr_scale and ema, the trainer's ema_weights() context, checkpoints,
translate.py --ema and the resumed CLI run."""

import argparse
import glob
import math
import os
import subprocess
import sys

import pytest
import torch

from cyclegan_amd.ops.adam import FusedAdam
from cyclegan_amd.parallel import DistContext
from cyclegan_amd.trainer import CycleGAN, lr_factor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_env():
    """Child-process environment with every GPU hidden."""
    return dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="",
                ROCR_VISIBLE_DEVICES="")


# ---- schedule ----

def test_lr_factor_values():
    assert lr_factor(0, 200, 100) == 1.0
    assert lr_factor(99, 200, 100) == 1.0
    assert lr_factor(100, 200, 100) == pytest.approx(100 / 101, rel=1e-15)
    assert lr_factor(199, 200, 100) == pytest.approx(1 / 101, rel=1e-13)
    assert lr_factor(199, 200, 100) > 0.0
    # once per epoch, monotone, never below 0
    f = [lr_factor(e, 200, 100) for e in range(200)]
    assert all(a >= b for a, b in zip(f, f[1:]))
    assert all(lr_factor(e, 200, 0) == 1.0 for e in (0, 1, 100, 199, 500))
    assert lr_factor(200, 200, 100) == 0.0
    assert lr_factor(250, 200, 100) == 0.0
    # decay over the whole run: first epoch already below 1
    assert lr_factor(0, 4, 4) == pytest.approx(4 / 5)
    assert lr_factor(3, 4, 4) == pytest.approx(1 / 5)


@pytest.mark.parametrize("argv", [
    ["--epochs", "3", "--lr_decay_epochs", "4"],
    ["--lr_decay_epochs", "-1"],
    ["--ema_decay", "1.0"],
    ["--ema_decay", "-0.1"],
])
def test_parser_rejects(argv, capsys):
    sys.path.insert(0, ROOT)
    try:
        import main as cli
    finally:
        sys.path.remove(ROOT)
    with pytest.raises(SystemExit) as e:
        cli.parse_args(argv)
    assert e.value.code != 0
    capsys.readouterr()


def test_parser_accepts_and_defaults():
    sys.path.insert(0, ROOT)
    try:
        import main as cli
    finally:
        sys.path.remove(ROOT)
    a = cli.parse_args([])
    assert a.ema_decay == 0.0 and a.lr_decay_epochs == 0
    a = cli.parse_args(["--epochs", "4", "--lr_decay_epochs", "4",
                        "--ema_decay", "0.999"])
    assert a.ema_decay == 0.999 and a.lr_decay_epochs == 4


# ---- FusedAdam ----

N = 37


def _adam_inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(N, generator=g) * 0.05
    grads = [torch.randn(N, generator=g) * 0.02 for _ in range(3)]
    return p0, grads


def _steps(opt, grads, record=None):
    for gr in grads:
        opt.g.copy_(gr)
        opt.step()
        if record is not None:
            record.append(opt.p.clone())


def test_lr_scale_is_a_scaled_lr():
    p0, grads = _adam_inputs()
    a = FusedAdam(p0.clone(), torch.zeros(N))
    a.lr_scale = 0.25
    b = FusedAdam(p0.clone(), torch.zeros(N), lr=2e-4 * 0.25)
    assert b.lr_scale == 1.0
    _steps(a, grads)
    _steps(b, grads)
    assert torch.equal(a.p, b.p) and torch.equal(a.m, b.m)
    assert torch.equal(a.v, b.v)
    assert not torch.equal(a.p, p0)
    assert "lr_scale" not in a.state_dict()


def test_advance_lr_writes_the_scaled_value():
    opt = FusedAdam(torch.zeros(4), torch.zeros(4))
    opt.prepare_graph()
    opt.lr_scale = 0.25
    for t in range(1, 5):
        opt.advance_lr()
        want = (opt.lr * 0.25 * math.sqrt(1 - opt.b2 ** t)
                / (1 - opt.b1 ** t))
        assert opt.t == t
        assert abs(opt._lr_t_dev.item() - want) < 1e-9 * (1 + abs(want))
    opt.lr_scale = 0.0
    opt.advance_lr()
    assert opt._lr_t_dev.item() == 0.0


def test_ema_leaves_the_trajectory_alone_and_follows_it():
    d = 0.9
    p0, grads = _adam_inputs(1)
    plain = FusedAdam(p0.clone(), torch.zeros(N))
    assert plain.ema is None and plain.ema_decay == 0.0
    avg = FusedAdam(p0.clone(), torch.zeros(N), ema_decay=d)
    assert torch.equal(avg.ema, p0) and avg.ema.dtype == torch.float32
    assert avg.ema.data_ptr() != avg.p.data_ptr()
    snaps = []
    _steps(plain, grads)
    _steps(avg, grads, snaps)
    for name in ("p", "m", "v"):
        assert torch.equal(getattr(plain, name), getattr(avg, name)), name
    # fp64 recursion over the recorded p, from p_0. Per step: three fp32
    # roundings plus the casts of d and 1-d, under 6 * 2^-24 relative to
    # the magnitudes involved; k steps add up
    want = p0.double()
    for p in snaps:
        want = d * want + (1 - d) * p.double()
    k = len(snaps)
    big = torch.maximum(avg.ema.abs(), avg.p.abs()).double()
    err = (avg.ema.double() - want).abs()
    assert bool((err <= k * 6 * 2.0 ** -24 * big).all()), err.max()
    assert not torch.equal(avg.ema, avg.p)
    avg.reset_ema()
    assert torch.equal(avg.ema, avg.p)
    plain.reset_ema()  # no-op
    assert plain.ema is None


# ---- trainer ----

def make_args(tmp_path, ema_decay=None, lr_decay_epochs=None):
    a = argparse.Namespace()
    a.output_dir = str(tmp_path)
    a.batch_size = 1
    a.global_batch_size = 1
    a.num_residual_blocks = 1
    a.compute_dtype = torch.float32
    if ema_decay is not None:
        a.ema_decay = ema_decay
    if lr_decay_epochs is not None:
        a.lr_decay_epochs = lr_decay_epochs
    return a


@pytest.fixture
def ctx():
    return DistContext(device=torch.device("cpu"))


def _xy(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(1, 32, 32, 3, generator=g) * 2 - 1,
            torch.rand(1, 32, 32, 3, generator=g) * 2 - 1)


@pytest.fixture
def trained(tmp_path, ctx):
    """A CPU trainer with D=0.5 after two train steps."""
    torch.manual_seed(0)
    gan = CycleGAN(make_args(tmp_path, ema_decay=0.5), ctx)
    for s in (1, 2):
        gan.train_step(*_xy(s))
    return gan


def test_only_generators_average(trained):
    assert trained.optimizers["G"].ema is not None
    assert trained.optimizers["F"].ema is not None
    assert trained.optimizers["X"].ema is None
    assert trained.optimizers["Y"].ema is None


def test_set_lr_scale_reaches_all_four(trained):
    trained.set_lr_scale(0.5)
    assert [o.lr_scale for o in trained.optimizers.values()] == [0.5] * 4


def test_ema_weights_context(trained):
    gan = trained
    live = {n: gan.groups[n].flat_param.clone() for n in "GF"}
    avg = {n: gan.optimizers[n].ema.clone() for n in "GF"}
    ptrs = {n: (gan.groups[n].flat_param.data_ptr(),
                gan.optimizers[n].ema.data_ptr()) for n in "GF"}
    assert not torch.equal(live["G"], avg["G"])
    x, y = _xy(3)
    outside = gan.test_step(x, y)
    with gan.ema_weights():
        for n in "GF":
            assert torch.equal(gan.groups[n].flat_param, avg[n])
        # the module parameters are views of the flat buffer: they moved too
        w = next(iter(gan.G.parameters()))
        k = w.numel()
        assert torch.equal(w.detach().reshape(-1), avg["G"][:k])
        inside = gan.test_step(x, y)
    assert any(float(inside[k]) != float(outside[k]) for k in outside)

    def restored():
        for n in "GF":
            assert torch.equal(gan.groups[n].flat_param, live[n])
            assert torch.equal(gan.optimizers[n].ema, avg[n])
            assert ptrs[n] == (gan.groups[n].flat_param.data_ptr(),
                               gan.optimizers[n].ema.data_ptr())

    restored()
    again = gan.test_step(x, y)
    assert all(float(again[k]) == float(outside[k]) for k in outside)

    with pytest.raises(ZeroDivisionError):
        with gan.ema_weights():
            assert torch.equal(gan.groups["G"].flat_param, avg["G"])
            1 / 0
    restored()


def test_ema_weights_is_a_noop_when_off(tmp_path, ctx):
    torch.manual_seed(0)
    gan = CycleGAN(make_args(tmp_path), ctx)
    assert gan.ema_decay == 0.0
    gan.train_step(*_xy(1))
    live = gan.groups["G"].flat_param.clone()
    with gan.ema_weights():
        assert torch.equal(gan.groups["G"].flat_param, live)
    assert torch.equal(gan.groups["G"].flat_param, live)


# ---- checkpoint ----

TODAY_KEYS = {"G", "F", "X", "Y", "G_optimizer", "F_optimizer",
              "X_optimizer", "Y_optimizer"}


def test_checkpoint_roundtrip_restores_ema(trained, tmp_path, ctx):
    gan = trained
    gan.save_checkpoint()
    state = torch.load(gan.checkpoint_path, weights_only=True)
    assert set(state) == TODAY_KEYS | {"G_ema", "F_ema"}
    assert set(state["G_ema"]) == set(state["G"])
    assert set(state["G_optimizer"]) == {"m", "v", "t", "lr", "b1", "b2",
                                         "eps"}
    torch.manual_seed(5)  # another init: everything must come from the file
    gan2 = CycleGAN(make_args(tmp_path, ema_decay=0.5), ctx)
    assert gan2.load_checkpoint()
    for n in "GF":
        assert torch.equal(gan2.optimizers[n].ema, gan.optimizers[n].ema)
        assert torch.equal(gan2.groups[n].flat_param,
                           gan.groups[n].flat_param)
        assert not torch.equal(gan2.optimizers[n].ema,
                               gan2.groups[n].flat_param)
    # the saved average loads straight into a Generator
    from cyclegan_amd.models import Generator
    fresh = Generator(num_residual_blocks=1)
    fresh.load_state_dict(state["G_ema"])
    x = _xy(4)[0]
    with torch.no_grad(), gan.ema_weights():
        assert torch.equal(fresh(x), gan.G(x))


def test_checkpoint_without_ema_restarts_it_from_loaded_weights(tmp_path, ctx):
    torch.manual_seed(0)
    off = CycleGAN(make_args(tmp_path), ctx)
    off.train_step(*_xy(1))
    off.save_checkpoint()
    state = torch.load(off.checkpoint_path, weights_only=True)
    assert set(state) == TODAY_KEYS  # both features off: exactly today's

    torch.manual_seed(5)
    on = CycleGAN(make_args(tmp_path, ema_decay=0.9), ctx)
    init = on.groups["G"].flat_param.clone()
    assert on.load_checkpoint()
    for n in "GF":
        assert torch.equal(on.groups[n].flat_param, off.groups[n].flat_param)
        assert torch.equal(on.optimizers[n].ema, on.groups[n].flat_param)
    assert not torch.equal(on.optimizers["G"].ema, init)


def test_saved_ema_ignored_and_not_resaved_when_off(trained, tmp_path, ctx):
    trained.save_checkpoint()
    gan = CycleGAN(make_args(tmp_path, lr_decay_epochs=1), ctx)
    assert gan.load_checkpoint()
    assert gan.optimizers["G"].ema is None
    assert torch.equal(gan.groups["G"].flat_param,
                       trained.groups["G"].flat_param)
    gan.save_checkpoint()
    state = torch.load(gan.checkpoint_path, weights_only=True)
    assert set(state) == TODAY_KEYS


def test_translate_cli_ema(trained, tmp_path, ctx):
    trained.save_checkpoint()
    first = trained.checkpoint_path
    other = tmp_path / "off"
    off = CycleGAN(make_args(other), ctx)
    off.save_checkpoint()

    def run(ckpt, out):
        return subprocess.run(
            [sys.executable, "translate.py", "--checkpoint", str(ckpt),
             "--ema", "--synthetic", "2", "--image_size", "32",
             "--num_residual_blocks", "1", "--output_dir", str(out)],
            cwd=ROOT, env=_cpu_env(), capture_output=True, text=True,
            timeout=300)

    out = tmp_path / "translated"
    r = run(first, out)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["00000.png", "00001.png"]
    r = run(off.checkpoint_path, tmp_path / "translated2")
    assert r.returncode != 0
    assert "averaged" in r.stderr and "G_ema" in r.stderr


# ---- CLI ----

def test_main_cli_schedule_resumes_at_the_right_epoch(tmp_path):
    out = tmp_path / "run"

    def run(epochs):
        return subprocess.run(
            [sys.executable, "main.py", "--output_dir", str(out),
             "--epochs", str(epochs), "--batch_size", "2", "--verbose", "0",
             "--image_size", "32", "--num_residual_blocks", "1",
             "--num_train_samples", "4", "--num_test_samples", "2",
             "--dtype", "fp32", "--lr_decay_epochs", "1",
             "--ema_decay", "0.9"],
            cwd=ROOT, env=_cpu_env(), capture_output=True, text=True,
            timeout=600)

    r = run(2)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Epoch 001/002" in r.stdout and "Epoch 002/002" in r.stdout
    state = torch.load(out / "checkpoints" / "checkpoint.pt",
                       weights_only=True)
    assert state["G_optimizer"]["t"] == 4 and "G_ema" in state

    r = run(3)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Epoch 003/003" in r.stdout
    assert "Epoch 001/003" not in r.stdout
    assert "Epoch 002/003" not in r.stdout
    state = torch.load(out / "checkpoints" / "checkpoint.pt",
                       weights_only=True)
    assert state["G_optimizer"]["t"] == 6

    files = glob.glob(str(out / "events.out.tfevents.*"))
    assert files
    assert any(b"learning_rate" in open(f, "rb").read() for f in files)
    tests = glob.glob(str(out / "test" / "events.out.tfevents.*"))
    assert not any(b"learning_rate" in open(f, "rb").read() for f in tests)
