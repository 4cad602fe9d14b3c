"""Adam + weight EMA on the GPU: the fused kernel against the plain Adam
kernels (p, m, v bitwise) and against the fp64 EMA update, on aligned and
misaligned views and between guard elements; the captured step following
the learning-rate scale; capture leaving the average alone; evaluation
under ema_weights() seeing the averaged generators."""

import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR, B1, B2, EPS = 2e-4, 0.5, 0.9, 1e-7
SIZES = [1, 3, 4, 5, 255, 1024, 1027, 4 * 256 * 3 + 7]
# |ema_new - (d*ema_old + (1-d)*p_new)| <= 6 * 2^-24 * (|ema_old| +
# |p_new|) per step, elementwise: three roundings (two products and the
# sum) plus the fp32 casts of d and 1-d, each 2^-24 relative at most
EMA_BOUND = 6 * 2.0 ** -24


def _ext():
    from cyclegan_amd.ops import backend
    return backend.ext()


def _inputs(n, seed, offset=0, guard=0):
    """p, m, v, ema and three gradients; with offset/guard each tensor is
    the [offset : offset+n] slice of its own larger buffer."""
    g = torch.Generator().manual_seed(seed)

    def one(scale, positive=False):
        t = torch.randn(n, generator=g) * scale
        t = t.abs() if positive else t
        if not (offset or guard):
            return t.to(DEV)
        store = torch.full((offset + n + guard,), SENTINEL, device=DEV)
        store[offset:offset + n].copy_(t)
        return store

    p, m, v, ema = one(0.05), one(0.01), one(1e-4, True), one(0.05)
    grads = [one(0.02) for _ in range(3)]
    return p, m, v, ema, grads


SENTINEL = 1234.5


def _lr_t(t):
    import math
    return LR * math.sqrt(1 - B2 ** t) / (1 - B1 ** t)


def _run(n, dev_variant, decay, offset=0, guard=0, seed=0):
    """3 steps of the fused kernel on views, the plain kernel on clones;
    asserts p, m, v bitwise and the EMA bound. Returns the stores."""
    ext = _ext()
    stores = _inputs(n, seed + n, offset, guard)
    sl = slice(offset, offset + n)
    p, m, v, ema = (s[sl] for s in stores[:4])
    grads = [s[sl] for s in stores[4]]
    if offset % 4:
        assert p.data_ptr() % 16 != 0
    pr, mr, vr = p.clone(), m.clone(), v.clone()
    p0 = p.clone()
    lr_dev = torch.zeros(1, device=DEV)
    for t in range(1, 4):
        g = grads[t - 1]
        ema_old = ema.double()
        if dev_variant:
            lr_dev.fill_(_lr_t(t))
            ext.adam_ema_step_dev(p, g, m, v, ema, lr_dev, B1, B2, EPS, decay)
            ext.adam_step_dev(pr, g.clone(), mr, vr, lr_dev, B1, B2, EPS)
        else:
            ext.adam_ema_step(p, g, m, v, ema, LR, B1, B2, EPS, t, decay)
            ext.adam_step(pr, g.clone(), mr, vr, LR, B1, B2, EPS, t)
        assert torch.equal(p, pr), (n, t, "p")
        assert torch.equal(m, mr), (n, t, "m")
        assert torch.equal(v, vr), (n, t, "v")
        if decay == 0.0:
            assert torch.equal(ema, p), (n, t)
        want = decay * ema_old + (1.0 - decay) * p.double()
        bound = EMA_BOUND * (ema_old.abs() + p.double().abs())
        err = (ema.double() - want).abs()
        assert bool((err <= bound).all()), (n, t, (err - bound).max().item())
    assert not torch.equal(p, p0)  # something happened
    return stores


@pytest.mark.parametrize("dev_variant", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_plain_adam(n, dev_variant):
    _run(n, dev_variant, 0.9)
    _run(n, dev_variant, 0.999, seed=1)


@pytest.mark.parametrize("dev_variant", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_zero_decay_copies_p(n, dev_variant):
    _run(n, dev_variant, 0.0)


@pytest.mark.parametrize("dev_variant", [False, True])
@pytest.mark.parametrize("n", [5, 1027])
def test_misaligned_views(n, dev_variant):
    _run(n, dev_variant, 0.9, offset=1, guard=15)
    _run(n, dev_variant, 0.0, offset=1, guard=15)


@pytest.mark.parametrize("dev_variant", [False, True])
@pytest.mark.parametrize("offset", [4, 8, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 3, 5, 1027, 4 * 256 * 3 + 7])
def test_no_overrun(n, offset, dev_variant):
    """Middle slice between sentinel guards, 4-aligned and unaligned starts:
    a vector tail writing past n (or before the start) would hit them."""
    guard = 9
    stores = _run(n, dev_variant, 0.9, offset=offset, guard=guard)
    for s in list(stores[:4]) + list(stores[4]):
        assert bool((s[:offset] == SENTINEL).all())
        assert bool((s[offset + n:] == SENTINEL).all())
        assert s[offset + n:].numel() == guard


def test_kernel_rejects_bad_arguments():
    ext = _ext()
    p, m, v, ema, (g, _, _) = _inputs(8, 0)
    lr = torch.zeros(1, device=DEV)
    ext.adam_ema_step(p, g, m, v, ema, LR, B1, B2, EPS, 1, 0.9)
    bad = [(p, g, m, v, ema[:4]),                       # numel
           (p, g.double(), m, v, ema),                  # dtype
           (p, g, m, v, ema.cpu()),                     # device
           (p, g, m, torch.zeros(16, device=DEV)[::2], ema)]  # contiguous
    for args in bad:
        with pytest.raises(RuntimeError):
            ext.adam_ema_step(*args, LR, B1, B2, EPS, 1, 0.9)
        with pytest.raises(RuntimeError):
            ext.adam_ema_step_dev(*args, lr, B1, B2, EPS, 0.9)
    with pytest.raises(RuntimeError):
        ext.adam_ema_step_dev(p, g, m, v, ema, lr.cpu(), B1, B2, EPS, 0.9)
    torch.cuda.synchronize()


def test_fused_adam_dispatches_ema_kernels():
    """FusedAdam(ema_decay) on the GPU, eager and graph mode, against the
    CPU formula path (the oracle): p to the plain kernel's tolerance, ema
    following its own p."""
    from cyclegan_amd.ops.adam import FusedAdam
    g = torch.Generator().manual_seed(3)
    n = 1027
    p0 = torch.randn(n, generator=g) * 0.05
    grads = [torch.randn(n, generator=g) * 0.02 for _ in range(3)]
    cpu = FusedAdam(p0.clone(), torch.zeros(n), ema_decay=0.9)
    gpu = FusedAdam(p0.to(DEV), torch.zeros(n, device=DEV), ema_decay=0.9)
    gpu.lr_scale = cpu.lr_scale = 0.5
    for i, gr in enumerate(grads):
        cpu.g.copy_(gr)
        gpu.g.copy_(gr)
        if i == 2:
            gpu.prepare_graph()
            gpu.advance_lr()
        cpu.step()
        gpu.step()
    assert cpu.t == gpu.t == 3
    assert torch.allclose(gpu.p.cpu(), cpu.p, rtol=1e-5, atol=1e-7)
    assert torch.allclose(gpu.ema.cpu(), cpu.ema, rtol=1e-5, atol=1e-7)
    assert not torch.equal(gpu.ema, gpu.p)


# ---- trainer ----

def make_args(tmp_path, ema_decay, batch=2, nrb=1):
    a = argparse.Namespace()
    a.output_dir = str(tmp_path)
    a.batch_size = batch
    a.global_batch_size = batch
    a.num_residual_blocks = nrb
    a.compute_dtype = torch.bfloat16
    a.ema_decay = ema_decay
    return a


def _data(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(2, 64, 64, 3, generator=g) * 2 - 1,
             torch.rand(2, 64, 64, 3, generator=g) * 2 - 1)
            for _ in range(n)]


def _ctx():
    from cyclegan_amd.parallel import DistContext
    return DistContext(device=torch.device("cuda", 0))


STEP_CLASSES = ["GraphedStep", "SegmentedGraphedStep"]


def _step_class(name):
    from cyclegan_amd import trainer
    return getattr(trainer, name)


@pytest.mark.parametrize("step_class", STEP_CLASSES)
def test_captured_step_follows_schedule_and_averages(tmp_path, step_class):
    from cyclegan_amd.trainer import CycleGAN
    d = 0.9
    data = _data(3, 7)
    torch.manual_seed(1)
    gan = CycleGAN(make_args(tmp_path, d), _ctx())
    assert gan.optimizers["X"].ema is None and gan.optimizers["Y"].ema is None
    step = _step_class(step_class)(gan, *data[0], warmup=1,
                                   preserve_state=True)
    start = {n: gan.groups[n].flat_param.clone() for n in "GFXY"}
    snaps = {n: [start[n]] for n in "GF"}
    emas = {n: [gan.optimizers[n].ema.clone()] for n in "GF"}
    assert all(torch.equal(snaps[n][0], emas[n][0]) for n in "GF")

    def replay(x, y):
        step(x, y)
        torch.cuda.synchronize()
        for n in "GF":
            snaps[n].append(gan.groups[n].flat_param.clone())
            emas[n].append(gan.optimizers[n].ema.clone())

    replay(*data[1])
    for n in "GFXY":  # at lr_scale 1 the replay does move the weights
        assert not torch.equal(gan.groups[n].flat_param, start[n]), n
    before = {n: gan.groups[n].flat_param.clone() for n in "GFXY"}
    m_before = {n: gan.optimizers[n].m.clone() for n in "GFXY"}
    gan.set_lr_scale(0.0)
    replay(*data[2])
    for n in "GFXY":
        # lr_t == 0: p -= 0 * m / (...) leaves every bit
        assert torch.equal(gan.groups[n].flat_param, before[n]), n
        assert not torch.equal(gan.optimizers[n].m, m_before[n]), n
        assert gan.optimizers[n].t == 2
    # ema against the fp64 recursion over the run's own snapshots
    for n in "GF":
        for k in (1, 2):
            old, p = emas[n][k - 1].double(), snaps[n][k].double()
            want = d * old + (1 - d) * p
            bound = EMA_BOUND * (old.abs() + p.abs())
            err = (emas[n][k].double() - want).abs()
            assert bool((err <= bound).all()), (n, k, (err - bound).max())
        assert not torch.equal(emas[n][2], snaps[n][2])


@pytest.mark.parametrize("step_class", STEP_CLASSES)
def test_capture_does_not_leak_into_state(tmp_path, step_class):
    from cyclegan_amd.trainer import CycleGAN
    data = _data(2, 5)
    torch.manual_seed(0)
    gan = CycleGAN(make_args(tmp_path, 0.9), _ctx())
    gan.train_step(*data[0])  # ema != flat_param from here on
    torch.cuda.synchronize()

    def state():
        out = {}
        for n, o in gan.optimizers.items():
            out[n] = (gan.groups[n].flat_param.clone(), o.m.clone(),
                      o.v.clone(), o.t,
                      None if o.ema is None else o.ema.clone())
        return out

    s0 = state()
    assert not torch.equal(s0["G"][4], s0["G"][0])
    _step_class(step_class)(gan, *data[1], warmup=2, preserve_state=True)
    torch.cuda.synchronize()
    s1 = state()
    for n in "GFXY":
        for a, b in zip(s0[n], s1[n]):
            if torch.is_tensor(a):
                assert torch.equal(a, b), n
            else:
                assert a == b, n


def test_evaluation_sees_the_average(tmp_path):
    from cyclegan_amd.models import Generator
    from cyclegan_amd.trainer import CycleGAN
    data = _data(3, 9)
    torch.manual_seed(2)
    gan = CycleGAN(make_args(tmp_path, 0.5), _ctx())
    for x, y in data[:2]:
        gan.train_step(x, y)
    gan.save_checkpoint()
    x = gan._cast(data[2][0])
    state = torch.load(gan.checkpoint_path, map_location="cuda:0",
                       weights_only=True)
    fresh = Generator(num_residual_blocks=1).to("cuda:0")
    fresh.load_state_dict(state["G_ema"])
    with torch.no_grad():
        want = fresh(x)
        live = gan.G(x)
        with gan.ema_weights():
            got = gan.G(x)
        after = gan.G(x)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert not torch.equal(got, live)
    assert torch.equal(after, live)
