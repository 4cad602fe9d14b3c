"""The Adam kernels' optional bf16 shadow: with it, p, m, v and ema are
bitwise what the same call gives without it, and the shadow is
bf16(p_new) at every element's own index, nothing written around it."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR, B1, B2, EPS, DECAY = 2e-4, 0.5, 0.9, 1e-7, 0.9
SENTINEL = 1024.0  # exact in bf16 too
GUARD = 8  # elements kept behind every slice, checked for stray writes

SIZES = [1, 3, 4, 7, 1027, 4096]   # 1027: 256 float4 words + a tail of 3
# element offset of every fp32 slice in its store (0: 16-byte aligned,
# 1: the all-scalar instantiation) and of the shadow slice in its own
# (0 / 4: 8-byte aligned, 1: scalar stores only)
OFFSETS = [(0, 0), (1, 1), (0, 4), (0, 1)]


def _ext():
    from cyclegan_amd.ops import backend
    return backend.ext()


def _store(values, offset):
    store = torch.full((offset + values.numel() + GUARD,), SENTINEL,
                       device=DEV, dtype=values.dtype)
    store[offset:offset + values.numel()].copy_(values)
    return store


def _state(n, seed, offset):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g) * 0.05
    m = torch.randn(n, generator=g) * 0.01
    v = (torch.randn(n, generator=g) * 1e-4).abs()
    ema = torch.randn(n, generator=g) * 0.05
    grad = torch.randn(n, generator=g) * 0.02
    return [_store(t, offset) for t in (p, grad, m, v, ema)]


def _call(kind, ext, p, g, m, v, ema, shadow):
    t = 3
    lr_t = torch.full((1,), LR * math.sqrt(1 - B2 ** t) / (1 - B1 ** t),
                      device=DEV)
    if kind == "adam_step":
        ext.adam_step(p, g, m, v, LR, B1, B2, EPS, t, shadow)
    elif kind == "adam_step_dev":
        ext.adam_step_dev(p, g, m, v, lr_t, B1, B2, EPS, shadow)
    elif kind == "adam_ema_step":
        ext.adam_ema_step(p, g, m, v, ema, LR, B1, B2, EPS, t, DECAY, shadow)
    else:
        ext.adam_ema_step_dev(p, g, m, v, ema, lr_t, B1, B2, EPS, DECAY,
                              shadow)


@pytest.mark.parametrize("offset,soffset", OFFSETS)
@pytest.mark.parametrize("kind", ["adam_step", "adam_step_dev",
                                  "adam_ema_step", "adam_ema_step_dev"])
def test_shadow_is_bf16_of_p_and_changes_nothing_else(kind, offset, soffset):
    ext = _ext()
    for n in SIZES:
        sl = slice(offset, offset + n)
        ref = _state(n, n, offset)
        got = [s.clone() for s in ref]
        sstore = torch.full((soffset + n + GUARD,), SENTINEL, device=DEV,
                            dtype=torch.bfloat16)
        shadow = sstore[soffset:soffset + n]
        if offset % 4:
            assert got[0][sl].data_ptr() % 16 != 0
        if soffset % 4:
            assert shadow.data_ptr() % 8 != 0

        _call(kind, ext, *(s[sl] for s in ref), None)
        _call(kind, ext, *(s[sl] for s in got), shadow)
        torch.cuda.synchronize()

        for name, a, b in zip("pgmve", got, ref):
            # whole stores: the slices and the sentinels around them
            assert torch.equal(a, b), (kind, n, name)
        assert not torch.equal(ref[0][sl], _state(n, n, offset)[0][sl])
        if "ema" not in kind:
            assert torch.equal(ref[4], _state(n, n, offset)[4])
        assert torch.equal(shadow, got[0][sl].to(torch.bfloat16)), (kind, n)
        assert (sstore[:soffset] == SENTINEL).all(), (kind, n)
        assert (sstore[soffset + n:] == SENTINEL).all(), (kind, n)


def test_shadow_arguments_are_checked():
    ext = _ext()
    p, g, m, v, ema = (s[:16] for s in _state(16, 0, 0))
    lr = torch.zeros(1, device=DEV)
    bad = [torch.zeros(16, device=DEV),                              # dtype
           torch.zeros(8, device=DEV, dtype=torch.bfloat16),         # short
           torch.zeros(16, dtype=torch.bfloat16),                    # device
           torch.zeros(32, device=DEV, dtype=torch.bfloat16)[::2]]   # strided
    for s in bad:
        with pytest.raises(RuntimeError):
            ext.adam_step(p, g, m, v, LR, B1, B2, EPS, 1, s)
        with pytest.raises(RuntimeError):
            ext.adam_step_dev(p, g, m, v, lr, B1, B2, EPS, s)
        with pytest.raises(RuntimeError):
            ext.adam_ema_step(p, g, m, v, ema, LR, B1, B2, EPS, 1, DECAY, s)
        with pytest.raises(RuntimeError):
            ext.adam_ema_step_dev(p, g, m, v, ema, lr, B1, B2, EPS, DECAY, s)
    torch.cuda.synchronize()


def test_fused_adam_reports_whether_it_wrote_the_shadow():
    from cyclegan_amd.ops.adam import FusedAdam
    n = 1027
    g = torch.Generator().manual_seed(5)
    p0 = (torch.randn(n, generator=g) * 0.05).to(DEV)
    grad = (torch.randn(n, generator=g) * 0.02).to(DEV)
    for decay in (0.0, 0.9):
        plain = FusedAdam(p0.clone(), grad.clone(), ema_decay=decay)
        opt = FusedAdam(p0.clone(), grad.clone(), ema_decay=decay)
        opt.shadow = torch.zeros(n + 5, device=DEV, dtype=torch.bfloat16)
        for graph in (False, True):
            if graph:
                for o in (plain, opt):
                    o.prepare_graph()
                    o.advance_lr()
            plain.step()
            opt.step()
            assert opt.wrote_shadow and not plain.wrote_shadow
            assert torch.equal(opt.p, plain.p)
            assert torch.equal(opt.shadow[:n], opt.p.to(torch.bfloat16))
            assert (opt.shadow[n:] == 0).all()
