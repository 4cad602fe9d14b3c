"""Image history pool on the GPU: the exchange kernel against the CPU op
(bit-exact: it only copies), under graph capture, and inside the eager and
the captured train step."""

import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _code_sets(B, P):
    """Sequences of codes for one pool, applied one after the other: pass,
    fill, swap, the same slot swapped by every element, a slot swapped
    twice in a row, a slot filled and then swapped."""
    s = P - 1
    sets = [
        [-1] * B,
        [P + b % P for b in range(B)],            # fill (slots repeat if B > P)
        [b % P for b in range(B)],                # swap
        [s] * B,                                  # all-swap of one slot
        [(-1, 0, P + s)[b % 3] for b in range(B)],  # pass / swap / fill mix
    ]
    if B >= 2:
        sets.append([0, 0] + [-1] * (B - 2))      # duplicate swap slot
        sets.append([-1] * (B - 2) + [P + s, s])  # fill then swap of one slot
    if B >= 3:
        sets.append([P + 0, 0, 0] + [s] * (B - 3))
    return sets


def _images(shape, dtype, g):
    # distinct values everywhere, so a misplaced unit cannot go unnoticed
    return (torch.rand(shape, generator=g) * 2 - 1).to(dtype)


def _check_sequence(pool_gpu, pool_cpu, B, dtype, g, out_given):
    from cyclegan_amd.ops import pool_exchange
    P, shape = pool_cpu.shape[0], tuple(pool_cpu.shape[1:])
    for codes in _code_sets(B, P):
        fake = _images((B, *shape), dtype, g)
        c = torch.tensor(codes, dtype=torch.int32)
        want = pool_exchange(pool_cpu, fake, c)
        fake_gpu = fake.to(DEV)
        out = torch.full_like(fake_gpu, 3.0) if out_given else None
        got = pool_exchange(pool_gpu, fake_gpu, c.to(DEV), out=out)
        if out_given:
            assert got is out
        assert torch.equal(got.cpu(), want), codes
        assert torch.equal(pool_gpu.cpu(), pool_cpu), codes
        assert torch.equal(fake_gpu.cpu(), fake), codes  # fake unmodified


SHAPES = [((1, 2, 4, 1), 1),     # one 16-byte vector in bf16
          ((3, 5, 5, 3), 2),     # 150 bytes per image in bf16: scalar path
          ((4, 8, 8, 3), 3),
          ((2, 16, 16, 3), 50)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape,P", SHAPES)
def test_kernel_matches_cpu_op(shape, P, dtype):
    g = torch.Generator().manual_seed(P)
    B, image = shape[0], shape[1:]
    pool_cpu = _images((P, *image), dtype, g)
    pool_gpu = pool_cpu.to(DEV)
    _check_sequence(pool_gpu, pool_cpu, B, dtype, g, out_given=False)
    _check_sequence(pool_gpu, pool_cpu, B, dtype, g, out_given=True)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_kernel_on_unaligned_pool_view(dtype):
    """Image bytes are a multiple of 16 but the pool starts one element
    past a 16-byte boundary: the dispatch must not take the vector path."""
    g = torch.Generator().manual_seed(4)
    B, image, P = 2, (16, 16, 3), 3
    n = P * 16 * 16 * 3
    pool_cpu = _images((P, *image), dtype, g)
    store = torch.zeros(n + 16, dtype=dtype, device=DEV)
    pool_gpu = store[1:1 + n].view(P, *image)
    assert pool_gpu.is_contiguous() and pool_gpu.data_ptr() % 16 != 0
    pool_gpu.copy_(pool_cpu)
    _check_sequence(pool_gpu, pool_cpu, B, dtype, g, out_given=False)
    # nothing outside the view was written
    assert store[0].item() == 0 and not store[1 + n:].any().item()


def test_kernel_rejects_bad_arguments():
    from cyclegan_amd.ops import backend
    ext = backend.ext()
    pool = torch.zeros(2, 4, 4, 3, device=DEV)
    fake = torch.zeros(2, 4, 4, 3, device=DEV)
    codes = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    ext.pool_exchange(pool, fake, codes, torch.empty_like(fake))
    for args in ((pool, fake, codes.long(), torch.empty_like(fake)),
                 (pool, fake, codes.cpu(), torch.empty_like(fake)),
                 (pool, fake, codes[:1], torch.empty_like(fake)),
                 (pool, fake.bfloat16(), codes, torch.empty_like(fake)),
                 (pool, fake[:, :, :2], codes, torch.empty_like(fake)),
                 (pool[:, :, :2], fake[:, :, :2].contiguous(), codes,
                  torch.empty(2, 4, 2, 3, device=DEV)),
                 (pool, fake, codes, fake),          # out aliases fake
                 (pool, pool, codes, torch.empty_like(fake))):
        with pytest.raises(RuntimeError):
            ext.pool_exchange(*args)
    torch.cuda.synchronize()


def test_exchange_under_graph_capture():
    from cyclegan_amd.ops import pool_exchange
    g = torch.Generator().manual_seed(9)
    B, image, P = 3, (8, 8, 3), 2
    dtype = torch.bfloat16
    pool_cpu = _images((P, *image), dtype, g)
    pool_gpu = pool_cpu.to(DEV)
    fake_s = torch.zeros(B, *image, dtype=dtype, device=DEV)
    codes_s = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    out_s = torch.empty_like(fake_s)
    pool_exchange(pool_gpu, fake_s, codes_s, out=out_s)  # all pass: warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pool_exchange(pool_gpu, fake_s, codes_s, out=out_s)
    assert torch.equal(pool_gpu.cpu(), pool_cpu)  # capture ran nothing
    for codes in ([P + 0, 0, -1], [1, 1, 1], [-1, -1, -1], [0, P + 1, 1]):
        fake = _images((B, *image), dtype, g)
        c = torch.tensor(codes, dtype=torch.int32)
        want = pool_exchange(pool_cpu, fake, c)
        fake_s.copy_(fake)
        codes_s.copy_(c)
        graph.replay()
        assert torch.equal(out_s.cpu(), want), codes
        assert torch.equal(pool_gpu.cpu(), pool_cpu), codes


# ---- trainer ----

def make_args(tmp_path, batch=2, nrb=2, pool_size=0):
    a = argparse.Namespace()
    a.output_dir = str(tmp_path)
    a.batch_size = batch
    a.global_batch_size = batch
    a.num_residual_blocks = nrb
    a.compute_dtype = torch.bfloat16
    a.pool_size = pool_size
    return a


def _data(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(2, 64, 64, 3, generator=g) * 2 - 1,
             torch.rand(2, 64, 64, 3, generator=g) * 2 - 1)
            for _ in range(n)]


STEP_CLASSES = ["GraphedStep", "SegmentedGraphedStep"]


def _step_class(name):
    from cyclegan_amd import trainer
    return getattr(trainer, name)


@pytest.mark.parametrize("step_class", STEP_CLASSES)
def test_graphed_step_matches_eager_with_pool(tmp_path, step_class):
    """tests/test_train_gpu.py::test_graphed_step_matches_eager with the
    pool on: 6 logical steps at pool_size 3, batch 2 (fill, the fill/steady
    boundary inside step 2, swaps), eager vs 2 eager + 4 graph replays that
    take their decisions from a planned device table. Both graph steps."""
    from cyclegan_amd.parallel import DistContext
    from cyclegan_amd.trainer import CycleGAN
    ctx = DistContext(device=torch.device("cuda", 0))
    data = _data(6, 11)

    torch.manual_seed(3)
    gan_e = CycleGAN(make_args(tmp_path, pool_size=3), ctx)
    for x, y in data:
        r_e = gan_e.train_step(x, y)
    torch.cuda.synchronize()

    torch.manual_seed(3)
    gan_g = CycleGAN(make_args(tmp_path, pool_size=3), ctx)
    for x, y in data[:2]:
        gan_g.train_step(x, y)
    step = _step_class(step_class)(gan_g, *data[2], warmup=0)
    gan_g.plan_pools([2] * 4, (64, 64, 3))
    # as tests/test_train_gpu.py reads them: the static outputs of the
    # one-graph step, the cloned ones of the segmented step
    call = step if step_class == "GraphedStep" else step.call_cloned
    for x, y in data[2:]:
        r_g = call(x, y)
    torch.cuda.synchronize()

    assert all(o.t == 6 for o in gan_g.optimizers.values())
    for k in r_e:
        a, b = r_e[k].item(), r_g[k].item()
        assert abs(a - b) <= 0.03 * (abs(b) + 0.03), (k, a, b)
    d = (gan_e.groups["G"].flat_param - gan_g.groups["G"].flat_param)
    assert d.abs().max().item() < 2.5e-3
    # same fill counts, same decisions consumed, same ones to come
    for p_e, p_g in zip(gan_e.pools, gan_g.pools):
        assert p_e.count == p_g.count == 3
        assert p_e.decision_state() == p_g.decision_state()
        assert p_g.decision_state()["pending"] == []
        assert p_e.draw(8) == p_g.draw(8)


@pytest.mark.parametrize("step_class", STEP_CLASSES)
def test_capture_preserves_pool_state(tmp_path, step_class):
    from cyclegan_amd.parallel import DistContext
    from cyclegan_amd.trainer import CycleGAN
    ctx = DistContext(device=torch.device("cuda", 0))
    data = _data(2, 5)
    torch.manual_seed(0)
    gan = CycleGAN(make_args(tmp_path, pool_size=4), ctx)
    gan.train_step(*data[0])  # pools half full
    assert [p.count for p in gan.pools] == [2, 2]
    bufs = [p.buf.clone() for p in gan.pools]
    states = [p.decision_state() for p in gan.pools]
    params = gan.groups["X"].flat_param.clone()

    _step_class(step_class)(gan, *data[1], preserve_state=True)
    torch.cuda.synchronize()

    assert torch.equal(gan.groups["X"].flat_param, params)
    for p, buf, state in zip(gan.pools, bufs, states):
        assert torch.equal(p.buf, buf)
        assert p.decision_state() == state
        assert p.draw(4) == _replay(state, 4)  # the next draw is unchanged
    assert gan._static_codes is None  # eager steps draw for themselves


def _replay(state, n):
    """The next n codes of a saved decision stream, on a twin pool."""
    from cyclegan_amd.ops import ImagePool
    twin = ImagePool(4, (1, 1, 1), torch.float32, "cpu", 0)
    twin.load_decision_state(state)
    return twin.draw(n)


def test_pool_off_stays_off(tmp_path, monkeypatch):
    from cyclegan_amd.ops import pool as pool_mod
    from cyclegan_amd.parallel import DistContext
    from cyclegan_amd.trainer import CycleGAN
    calls = []
    real = pool_mod.pool_exchange
    monkeypatch.setattr(pool_mod, "pool_exchange",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    ctx = DistContext(device=torch.device("cuda", 0))
    x, y = _data(1, 2)[0]

    torch.manual_seed(0)
    gan = CycleGAN(make_args(tmp_path, pool_size=0), ctx)
    gan.train_step(x, y)
    gan._forward_losses(gan._cast(x), gan._cast(y))
    torch.cuda.synchronize()
    assert gan.pools is None and gan.pool_size == 0 and calls == []

    # the counter does count: one exchange per discriminator with it on
    gan = CycleGAN(make_args(tmp_path, pool_size=2), ctx)
    gan.train_step(x, y)
    torch.cuda.synchronize()
    assert len(calls) == 2 and gan.pools is not None
