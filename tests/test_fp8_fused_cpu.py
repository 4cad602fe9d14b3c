"""fp8 hand-off plumbing that needs no GPU: fp8_state.peek, the shared fp8
dispatch predicate, and the optional fp8_consumer hint being a no-op on the
CPU path (ops and models)."""

import pytest
import torch

from cyclegan_amd import ops
from cyclegan_amd.models import Discriminator, Generator
from cyclegan_amd.models.layers import ResBlock
from cyclegan_amd.ops import conv as convmod
from cyclegan_amd.ops import fp8_state


def test_peek_unknown_weight_allocates_nothing():
    fp8_state.reset()
    try:
        w = torch.zeros(4, 3, 3, 4)
        assert fp8_state.peek(w) is None
        assert fp8_state._used == 0
        # the consumer still sees its first call as fresh
        _, _, fresh = fp8_state.slots_for(w)
        assert fresh
        assert fp8_state._used == 1
    finally:
        fp8_state.reset()


def test_peek_returns_the_layers_views():
    fp8_state.reset()
    try:
        w1 = torch.zeros(4, 3, 3, 4)
        w2 = torch.zeros(4, 3, 3, 4)
        p1, c1, _ = fp8_state.slots_for(w1)
        got = fp8_state.peek(w1)
        assert got is not None and got[0] is p1 and got[1] is c1
        assert fp8_state.peek(w2) is None
        assert fp8_state._used == 1
        # peek did not consume anything: a second slots_for is not fresh
        # and hands out the same views
        p1b, c1b, fresh = fp8_state.slots_for(w1)
        assert not fresh and p1b is p1 and c1b is c1
    finally:
        fp8_state.reset()


def _x(b, c, dtype=torch.bfloat16):
    return torch.zeros(b, 16, 16, c, dtype=dtype)


def _w(cout, k, cin):
    return torch.zeros(cout, k, k, cin)


# name, x, w, stride, expected
PREDICATE_CASES = [
    ("k3_s1_c256_b11", _x(11, 256), _w(256, 3, 256), 1, False),
    ("k3_s1_c256_b12", _x(12, 256), _w(256, 3, 256), 1, True),
    ("k4_s1_c256_b1", _x(1, 256), _w(512, 4, 256), 1, True),
    ("k4_s1_c512_b1", _x(1, 512), _w(1, 4, 512), 1, True),
    ("k3_s2_c256_b12", _x(12, 256), _w(256, 3, 256), 2, False),
    ("k4_s2_c256_b12", _x(12, 256), _w(512, 4, 256), 2, False),
    ("k3_s1_c128_b12", _x(12, 128), _w(256, 3, 128), 1, False),
    ("k4_s1_c128_b12", _x(12, 128), _w(256, 4, 128), 1, False),
    ("k3_s1_c256_b12_fp32", _x(12, 256, torch.float32), _w(256, 3, 256), 1,
     False),
    ("k7_s1_c256_b12", _x(12, 256), _w(8, 7, 256), 1, False),
]


@pytest.mark.parametrize("case", PREDICATE_CASES,
                         ids=[c[0] for c in PREDICATE_CASES])
def test_shared_predicate_matches_documented_dispatch(case):
    _, x, w, stride, want = case
    assert convmod.takes_fp8_path(x, w, stride) is want


def test_predicate_excludes_packed_head():
    """With pads given, the packed-head geometry is rejected by name too."""
    x = _x(12, 256)
    w = _w(8, 7, 256)
    assert convmod._head_packable(x, w, 1, (3, 3, 3, 3), True)
    assert not convmod.takes_fp8_path(x, w, 1, (3, 3, 3, 3), True)


def test_instance_norm_ignores_hint_on_cpu():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 8, 8, 16, generator=g)
    gamma = torch.randn(16, generator=g)
    beta = torch.randn(16, generator=g)
    res = torch.randn(2, 8, 8, 16, generator=g)
    hint = ops.Fp8Consumer(torch.zeros(256, 3, 3, 256), 1)
    convmod.set_fp8_mode(True)
    try:
        for act, r in (("relu", None), (None, res), ("lrelu", None)):
            a = ops.instance_norm(x, gamma, beta, act=act, residual=r)
            b = ops.instance_norm(x, gamma, beta, act=act, residual=r,
                                  fp8_consumer=hint)
            assert torch.equal(a, b)
            assert getattr(b, convmod.FP8_TWIN_ATTR, None) is None
    finally:
        convmod.set_fp8_mode(False)
    assert fp8_state.peek(hint.weight) is None


def _plain_generator_forward(m, x):
    h = m.stem_norm(m.stem_conv(x))
    for d in m.downs:
        h = d(h)
    for b in m.blocks:
        t = b.norm1(b.conv1(h))
        h = b.norm2(b.conv2(t), residual=h)
    for u in m.ups:
        h = u(h)
    return m.head(h)


def test_generator_cpu_forward_unchanged_by_hints():
    torch.manual_seed(0)
    m = Generator(filters=8, num_residual_blocks=2)
    x = torch.randn(1, 16, 16, 3)
    assert torch.equal(m(x), _plain_generator_forward(m, x))
    # no resblocks: the last down norm has nobody to hint
    m0 = Generator(filters=8, num_residual_blocks=0)
    assert torch.equal(m0(x), _plain_generator_forward(m0, x))


def test_discriminator_cpu_forward_unchanged_by_hints():
    torch.manual_seed(0)
    m = Discriminator(filters=8)
    x = torch.randn(1, 32, 32, 3)
    h = m.stem(x)
    for layer in m.mids:
        h = layer(h)
    assert torch.equal(m(x), m.head(h))


def test_resblock_takes_optional_hint():
    torch.manual_seed(0)
    b = ResBlock(16)
    x = torch.randn(1, 8, 8, 16)
    hint = b.conv1.fp8_hint()
    assert hint.weight is b.conv1.weight and hint.stride == 1
    assert torch.equal(b(x), b(x, fp8_consumer=hint))
