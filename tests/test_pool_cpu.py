"""Image history pool on the CPU: the sequential exchange op, the host
decision stream (draw / plan / state), and how the trainer uses them.
Every comparison of the exchange itself is bit-exact: the op only copies."""

import argparse

import numpy as np
import pytest
import torch

from cyclegan_amd.ops import ImagePool, pool_exchange
from cyclegan_amd.ops.pool import check_codes, make_codes
from cyclegan_amd.parallel import DistContext
from cyclegan_amd.trainer import CycleGAN


# ---- the op against a plain list pool ----

class ListPool:
    """The published algorithm on a python list, fed by a numpy generator
    in ImagePool's draw order: fill while not full, else one random(), and
    if > 0.5 one integers(P) to pick the image that is swapped out."""

    def __init__(self, P, seed):
        self.P, self.images, self.rng = P, [], np.random.default_rng(seed)
        self.swaps = self.passes = self.collisions = 0

    def query(self, batch):
        out, slots = [], []
        for img in batch:
            if len(self.images) < self.P:
                slots.append(len(self.images))
                self.images.append(img.clone())
                out.append(img.clone())
            elif self.rng.random() > 0.5:
                s = int(self.rng.integers(self.P))
                slots.append(s)
                out.append(self.images[s])
                self.images[s] = img.clone()
                self.swaps += 1
            else:
                out.append(img.clone())
                self.passes += 1
        self.collisions += len(slots) != len(set(slots))
        return torch.stack(out)


def test_semantics_match_list_pool():
    P, B, steps, seed = 5, 3, 40, 7
    shape = (4, 4, 3)
    ref = ListPool(P, seed)
    pool = ImagePool(P, shape, torch.float32, "cpu", seed)
    g = torch.Generator().manual_seed(0)
    for step in range(steps):
        fake = torch.rand(B, *shape, generator=g)
        want = ref.query(fake)
        got = pool.exchange(fake, pool.next_codes(B))
        assert torch.equal(got, want), step
    assert torch.equal(pool.buf, torch.stack(ref.images))
    assert pool.count == P
    # the run covered what it is meant to cover
    assert ref.swaps >= 1 and ref.passes >= 1 and ref.collisions >= 1


# ---- hand-written codes ----

def _setup(P=3, B=3, shape=(2, 2, 3)):
    g = torch.Generator().manual_seed(1)
    pool = torch.rand(P, *shape, generator=g)
    fake = torch.rand(B, *shape, generator=g)
    return pool, fake


def _codes(values):
    return torch.tensor(values, dtype=torch.int32)


def test_duplicate_swap_slot_in_one_batch():
    pool, fake = _setup()
    p0 = pool.clone()
    out = pool_exchange(pool, fake, _codes([1, 1, 1]))
    assert torch.equal(out[0], p0[1])
    assert torch.equal(out[1], fake[0])  # sees what element 0 stored
    assert torch.equal(out[2], fake[1])
    assert torch.equal(pool[1], fake[2])
    assert torch.equal(pool[0], p0[0]) and torch.equal(pool[2], p0[2])


def test_fill_then_swap_of_one_slot():
    pool, fake = _setup()
    p0 = pool.clone()
    out = pool_exchange(pool, fake, _codes([3 + 2, 2, -1]))
    assert torch.equal(out[0], fake[0])
    assert torch.equal(out[1], fake[0])  # the image the fill just stored
    assert torch.equal(out[2], fake[2])
    assert torch.equal(pool[2], fake[1])
    assert torch.equal(pool[:2], p0[:2])  # untouched slots unchanged


def test_all_pass_leaves_pool_alone():
    pool, fake = _setup()
    p0, f0 = pool.clone(), fake.clone()
    out = pool_exchange(pool, fake, _codes([-1, -1, -1]))
    assert torch.equal(out, fake) and out.data_ptr() != fake.data_ptr()
    assert torch.equal(pool, p0) and torch.equal(fake, f0)


def test_out_given_equals_out_allocated():
    pool, fake = _setup()
    pool2 = pool.clone()
    codes = _codes([0, 3 + 1, 1])
    want = pool_exchange(pool, fake, codes)
    out = torch.full_like(fake, -7.0)
    got = pool_exchange(pool2, fake, codes, out=out)
    assert got is out
    assert torch.equal(got, want) and torch.equal(pool, pool2)


def test_op_rejects_mismatched_arguments():
    pool, fake = _setup()
    with pytest.raises(ValueError):
        pool_exchange(pool, fake, torch.tensor([0, 0, 0]))  # int64 codes
    with pytest.raises(ValueError):
        pool_exchange(pool, fake, _codes([0, 0]))  # wrong length
    with pytest.raises(ValueError):
        pool_exchange(pool, fake.double(), _codes([0, 0, 0]))
    with pytest.raises(ValueError):
        pool_exchange(pool, fake[:, :1], _codes([0, 0, 0]))


# ---- code validation ----

def test_code_validation():
    P = 4
    ok = torch.tensor([-1, 0, P - 1, P, 2 * P - 1])
    check_codes(ok, P)
    assert make_codes(ok.tolist(), P, "cpu").dtype == torch.int32
    for bad in (-2, 2 * P):
        with pytest.raises(ValueError):
            check_codes(torch.tensor([0, bad]), P)
        with pytest.raises(ValueError):
            make_codes([0, bad], P, "cpu")
    # the CPU op checks what it is handed, too
    pool, fake = _setup(P=P, B=1)
    with pytest.raises(ValueError):
        pool_exchange(pool, fake, _codes([2 * P]))


# ---- plan / state ----

def _pool(seed=3, P=4):
    return ImagePool(P, (2, 2, 3), torch.float32, "cpu", seed)


def test_plan_equals_draws():
    a, b = _pool(), _pool()
    table = a.plan([3, 3, 2])
    rows = [b.draw(3), b.draw(3), b.draw(2)]
    assert table.dtype == torch.int32 and tuple(table.shape) == (3, 3)
    assert table[0].tolist() == rows[0] and table[1].tolist() == rows[1]
    assert table[2].tolist() == rows[2] + [-1]  # padded tail
    assert a.count == b.count
    # the steps get the planned rows, cut to their batch
    for row in rows:
        assert a.next_codes(len(row)).tolist() == row
    # ... and then the same stream goes on
    assert a.next_codes(5).tolist() == b.draw(5)
    # a plan that was not used up is not silently dropped
    a.plan([2, 2])
    with pytest.raises(RuntimeError):
        a.plan([2])
    with pytest.raises(RuntimeError):
        a.next_codes(3)


def _run(pool, steps, g, B=3):
    outs = []
    for _ in range(steps):
        fake = torch.rand(B, *pool.buf.shape[1:], generator=g)
        outs.append(pool.exchange(fake, pool.next_codes(B)))
    return outs


def test_state_dict_round_trip_continues_stream():
    a = _pool()
    _run(a, 3, torch.Generator().manual_seed(0))
    a.plan([3, 3])  # planned but not consumed is part of the state
    state = a.state_dict()
    b = _pool(seed=99)  # another stream, overwritten by the load
    b.load_state_dict(state)
    assert b.count == a.count and torch.equal(a.buf, b.buf)
    ga, gb = (torch.Generator().manual_seed(5) for _ in range(2))
    for x, y in zip(_run(a, 6, ga), _run(b, 6, gb)):
        assert torch.equal(x, y)
    assert torch.equal(a.buf, b.buf)
    assert a.draw(8) == b.draw(8)
    # the saved state is a snapshot, not a view of the live pool
    assert not torch.equal(state["buf"], a.buf)


# ---- trainer ----

def make_args(tmp_path, batch=2, pool_size=0, seed=1234):
    a = argparse.Namespace()
    a.output_dir = str(tmp_path)
    a.batch_size = batch
    a.global_batch_size = batch
    a.num_residual_blocks = 1
    a.compute_dtype = torch.float32
    a.seed = seed
    if pool_size is not None:
        a.pool_size = pool_size
    return a


@pytest.fixture
def ctx():
    return DistContext(device=torch.device("cpu"))


def _batch(seed=0, b=2):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(b, 16, 16, 3, generator=g) * 2 - 1,
            torch.rand(b, 16, 16, 3, generator=g) * 2 - 1)


def _gan(tmp_path, ctx, **kw):
    torch.manual_seed(0)
    return CycleGAN(make_args(tmp_path, **kw), ctx)


def _full_pools(gan, seed):
    """Pools full of random images: the next step is in the swap phase."""
    g = torch.Generator().manual_seed(seed)
    for pool in gan._ensure_pools((16, 16, 3)):
        pool.buf.copy_(torch.rand(pool.buf.shape, generator=g) * 2 - 1)
        pool.count = pool.P
    return gan.pools


_TODAYS_KEYS = {"G", "F", "X", "Y", "G_optimizer", "F_optimizer",
                "X_optimizer", "Y_optimizer"}


def test_trainer_checkpoint_round_trip(tmp_path, ctx):
    gan = _gan(tmp_path, ctx, pool_size=3)
    for s in range(3):  # past the fill phase
        gan.train_step(*_batch(s))
    gan.save_checkpoint()
    saved = torch.load(gan.checkpoint_path, weights_only=True)
    assert set(saved) == _TODAYS_KEYS | {"pool_x", "pool_y"}

    gan2 = _gan(tmp_path, ctx, pool_size=3)
    assert gan2.load_checkpoint()
    for p, q in zip(gan.pools, gan2.pools):
        assert q.count == p.count == 3 and torch.equal(p.buf, q.buf)
    # the resumed run continues the same decisions and the same training
    for s in range(3, 6):
        gan.train_step(*_batch(s))
        gan2.train_step(*_batch(s))
    for n in ("G", "F", "X", "Y"):
        assert torch.equal(gan.groups[n].flat_param,
                           gan2.groups[n].flat_param), n
    for p, q in zip(gan.pools, gan2.pools):
        assert torch.equal(p.buf, q.buf) and p.draw(6) == q.draw(6)


def test_poolless_checkpoint_loads_with_empty_pools(tmp_path, ctx):
    off = _gan(tmp_path, ctx, pool_size=0)
    off.train_step(*_batch())
    off.save_checkpoint()
    on = _gan(tmp_path, ctx, pool_size=3)
    assert on.load_checkpoint()
    assert torch.equal(on.groups["X"].flat_param, off.groups["X"].flat_param)
    assert on.pools is None  # built, empty, at the first step
    on.train_step(*_batch(1))
    assert [p.count for p in on.pools] == [2, 2]


def test_pool_off_trainer_saves_todays_keys_and_ignores_pools(tmp_path, ctx):
    for kw in ({"pool_size": 0}, {"pool_size": None}):  # bench.py: no attr
        off = _gan(tmp_path, ctx, **kw)
        off.train_step(*_batch())
        assert off.pools is None
        off.save_checkpoint()
        assert set(torch.load(off.checkpoint_path,
                              weights_only=True)) == _TODAYS_KEYS
    on = _gan(tmp_path, ctx, pool_size=3)
    on.train_step(*_batch())
    on.save_checkpoint()
    off = _gan(tmp_path, ctx, pool_size=0)
    assert off.load_checkpoint() and off.pools is None


def test_pool_contents_reach_only_the_discriminators(tmp_path, ctx):
    """Same weights, same decisions, different pool images: G and F see
    the fresh fakes (bit-identical grads), X and Y the pooled ones."""
    x, y = _batch()
    gans = [_gan(tmp_path, ctx, pool_size=2) for _ in range(2)]
    before = [[p.buf.clone() for p in _full_pools(gan, seed)]
              for gan, seed in zip(gans, (10, 11))]
    for gan in gans:
        gan.train_step(x, y)
    # a swap took place in every pool (full pools change only by swaps)
    for gan, bufs in zip(gans, before):
        for pool, buf in zip(gan.pools, bufs):
            assert not torch.equal(pool.buf, buf)
    a, b = gans
    for n in ("G", "F"):
        assert torch.equal(a.groups[n].flat_grad, b.groups[n].flat_grad), n
    for n in ("X", "Y"):
        assert not torch.equal(a.groups[n].flat_grad, b.groups[n].flat_grad), n


def test_discriminator_grad_is_that_of_the_pooled_loss(tmp_path, ctx):
    x, y = _batch()
    gan = _gan(tmp_path, ctx, pool_size=2)
    pool_x = _full_pools(gan, 10)[0]
    # replay the step's exchange on a twin of the pool
    twin = ImagePool(2, (16, 16, 3), torch.float32, "cpu", 0)
    twin.load_state_dict(pool_x.state_dict())
    fake_x = gan.F(y).detach().contiguous()
    pooled = twin.exchange(fake_x, twin.next_codes(2))
    assert not torch.equal(pooled, fake_x)  # a swap: pooled != fresh
    loss = gan.discriminator_loss(gan.X(x), gan.X(pooled))
    gs = torch.autograd.grad(loss, gan.groups["X"].params)
    want = torch.cat([g.reshape(-1) for g in gs])

    gan.train_step(x, y)  # the optimizer step leaves grads in place
    got = gan.groups["X"].flat_grad
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-7)
    assert torch.equal(pool_x.buf, twin.buf)


def test_filling_pool_gives_pool_off_losses(tmp_path, ctx):
    """While the pool fills, pooled == fake: all ten losses are those of a
    pool-off trainer."""
    on = _gan(tmp_path, ctx, pool_size=50)
    off = _gan(tmp_path, ctx, pool_size=0)
    for s in range(2):
        x, y = _batch(s)
        r_on, r_off = on.train_step(x, y), off.train_step(x, y)
        assert set(r_on) == set(r_off) and len(r_on) == 10
        for k in r_off:
            assert torch.allclose(r_on[k], r_off[k], rtol=1e-5, atol=1e-7), k
    assert [p.count for p in on.pools] == [4, 4]


def test_short_and_empty_batches(tmp_path, ctx):
    gan = _gan(tmp_path, ctx, pool_size=3)
    gan.train_step(*_batch(0, b=1))  # short batch: b elements exchanged
    assert [p.count for p in gan.pools] == [1, 1]
    state = [p.decision_state() for p in gan.pools]
    bufs = [p.buf.clone() for p in gan.pools]
    empty = torch.empty(0, 16, 16, 3)
    gan.train_step(empty, empty)  # empty DP slice: no exchange, no draws
    gan.test_step(*_batch(1))
    gan.cycle_step(*_batch(1))
    assert [p.decision_state() for p in gan.pools] == state
    for p, buf in zip(gan.pools, bufs):
        assert torch.equal(p.buf, buf)


def test_pools_are_seeded_per_rank_and_domain(tmp_path, ctx):
    gan = _gan(tmp_path, ctx, pool_size=1, seed=5)
    other = _gan(tmp_path, ctx, pool_size=1, seed=6)
    streams = [p.draw(65)[1:] for g in (gan, other)
               for p in g._ensure_pools((16, 16, 3))]
    assert len({tuple(s) for s in streams}) == 4
    want = ImagePool(1, (1, 1, 1), torch.float32, "cpu",
                     seed=(5, ctx.rank, 1)).draw(65)[1:]
    assert streams[1] == want


# ---- CLI ----

def test_cli_pool_size():
    import main
    assert main.parse_args([]).pool_size == 0
    assert main.parse_args(["--pool_size", "50"]).pool_size == 50
    with pytest.raises(SystemExit):
        main.parse_args(["--pool_size", "-1"])
