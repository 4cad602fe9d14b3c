"""Shadow arena with the Adam-written mirror: the layout tables on the
CPU (kernels emulated in torch), and on the GPU every compute form after an
optimizer step against the full gather (CYG_NO_ADAM_SHADOW=1) from the same
masters."""
import argparse

import pytest
import torch

from cyclegan_amd.models import Discriminator, Generator
from cyclegan_amd.ops import arena as arena_mod
from cyclegan_amd.ops.arena import ShadowArena
from cyclegan_amd.parallel import FlatParamGroup


def _models():
    torch.manual_seed(0)
    return [Generator(num_residual_blocks=1),
            Generator(num_residual_blocks=1, upsample="resize"),
            Discriminator()]


# ---------------------------------------------------------------- CPU ----

def _emulate_gather(idx, flat):
    i = idx.long()
    return torch.where(i >= 0, flat[i.clamp(min=0)],
                       torch.zeros(())).to(torch.bfloat16)


def _emulate_fold(idx4, flat):
    i = idx4.long()
    s = torch.zeros(i.shape[0])
    for j in range(4):
        s = s + torch.where(i[:, j] >= 0, flat[i[:, j].clamp(min=0)],
                            torch.zeros(()))
    return s.to(torch.bfloat16)


def _emulate_refresh(a):
    """What refresh() launches, in torch, from the arena's own tables."""
    flat = a.group.flat_param.detach()
    if a.mirror is not None:
        a.mirror[:flat.numel()].copy_(flat.to(torch.bfloat16))
        for so, do, O, taps, I, _, _, _ in a.ttable.tolist():
            src = a.mirror[so:so + O * taps * I].view(O, taps, I)
            a.tbuf[do:do + O * taps * I].copy_(
                src.permute(2, 1, 0).reshape(-1))
    a.buf.copy_(_emulate_gather(a.idx, flat))
    a.fold_buf.copy_(_emulate_fold(a.fold_idx, flat))


def _build(module, mirror, monkeypatch):
    group = getattr(module, "_test_group", None) or FlatParamGroup(module)
    module._test_group = group
    monkeypatch.setattr(ShadowArena, "refresh",
                        lambda self, mirror_fresh=False: None)
    a = ShadowArena(group, module, mirror=mirror)
    _emulate_refresh(a)
    return a, group


def _inside(view, store):
    lo = store.data_ptr()
    return lo <= view.data_ptr() and \
        view.data_ptr() + view.numel() * 2 <= lo + store.numel() * 2


def test_layout_tables_are_consistent(monkeypatch):
    for module in _models():
        a, group = _build(module, True, monkeypatch)
        legacy, _ = _build(module, False, monkeypatch)
        off = {p: o for p, (o, _) in zip(group.params, group._offsets)}
        n = group.flat_param.numel()
        assert a.mirror.numel() == n + (-n) % 8 and a.mirror.numel() % 8 == 0
        assert legacy.mirror is None and legacy.ttable.shape[0] == 0
        assert a.idx.numel() == a.buf.numel() and a.idx.numel() % 8 == 0
        # the gather shrank by exactly the forms that left it (their sizes
        # are multiples of 64, so the padding to 8 is the same)
        moved = sum(v.numel() for p, f in a._by_param.items()
                    for name, v in f.items()
                    if a.source[p][name] in ("mirror", "transpose"))
        assert moved > 0 and moved % 64 == 0
        assert a.idx.numel() == legacy.idx.numel() - moved
        assert a.tbuf.numel() == moved // 2
        assert torch.equal(a.fold_idx, legacy.fold_idx)

        rows = {r[1]: r for r in a.ttable.tolist()}
        blocks = 0
        for r in a.ttable.tolist():
            assert r[5] == blocks
            assert r[6] == -(-r[4] // 64) and r[7] == -(-r[2] // 64)
            blocks += r[3] * r[6] * r[7]
        n_view = n_tr = 0
        for p, forms in a._by_param.items():
            assert set(forms) == set(legacy._by_param[p])
            for name, v in forms.items():
                kind = a.source[p][name]
                lv = legacy.forms_of(p)[name]
                assert legacy.source[p][name] in ("gather", "fold")
                assert v.shape == lv.shape and v.is_contiguous()
                # every form, wherever it comes from, is what the full
                # gather gives
                assert torch.equal(v, lv), (name, kind)
                if kind == "mirror":
                    n_view += 1
                    O, _, _, I = p.shape
                    assert name in ("p", "plain") and v.shape == p.shape
                    assert O >= 8 and I >= 8 and off[p] % 8 == 0
                    assert v.data_ptr() % 16 == 0
                    assert v.data_ptr() == a.mirror.data_ptr() + 2 * off[p]
                    assert _inside(v, a.mirror)
                elif kind == "transpose":
                    n_tr += 1
                    O, KH, KW, I = p.shape
                    assert name in ("tp", "t")
                    assert v.shape == (I, KH, KW, O)
                    assert _inside(v, a.tbuf) and v.data_ptr() % 16 == 0
                    d = (v.data_ptr() - a.tbuf.data_ptr()) // 2
                    assert rows[d][:5] == [off[p], d, O, KH * KW, I]
                    assert O % 8 == 0 and I % 8 == 0 and off[p] % 8 == 0
                elif kind == "gather":
                    assert _inside(v, a.buf)
                    # only what cannot be a view or a transpose is left
                    if name in ("p", "plain"):
                        assert not arena_mod.mirror_view_ok(off[p], p.shape)
                    if name in ("tp", "t"):
                        assert not arena_mod.transpose_ok(off[p], p.shape)
                else:
                    assert kind == "fold" and _inside(v, a.fold_buf)
        assert n_tr == a.ttable.shape[0] == len(rows)

        # which weights are views: every conv but the RGB stem and the
        # small-Cout head; resize layers live in the fold segment
        convs = [m for m in module.modules()
                 if type(m).__name__ in ("ConvNHWC", "ConvTransposeNHWC")]
        want = [m for m in convs if min(m.weight.shape[0],
                                        m.weight.shape[3]) >= 8]
        assert n_view == n_tr == len(want) == len(convs) - 2
        for m in convs:
            src = set(a.source[m.weight].values())
            if m in want:
                assert src >= {"mirror", "transpose"}
            else:
                assert src == {"gather"}
            if m.bias is not None:
                assert set(a.source[m.bias].values()) == {"gather"}


def test_odd_offset_keeps_the_gather(monkeypatch):
    """A weight whose flat offset is no multiple of 8 elements cannot be a
    16-byte aligned view or a transpose source."""
    from cyclegan_amd.models.layers import ConvNHWC
    torch.manual_seed(1)
    mod = torch.nn.Sequential(ConvNHWC(8, 8, 1, bias=True),
                              ConvNHWC(16, 16, 3))
    # parameter order: weight (64), bias (8), weight -> offsets 0, 64, 72;
    # a 3-element bias instead shifts the last one off the grid
    mod[0].bias = torch.nn.Parameter(torch.zeros(3))
    a, group = _build(mod, True, monkeypatch)
    offs = [o for o, _ in group._offsets]
    assert offs == [0, 64, 67]
    assert a.source[mod[0].weight] == {"p": "mirror", "tp": "transpose"}
    assert a.source[mod[1].weight] == {"p": "gather", "tp": "gather"}
    legacy, _ = _build(mod, False, monkeypatch)
    for form in ("p", "tp"):
        assert torch.equal(a.forms_of(mod[1].weight)[form],
                           legacy.forms_of(mod[1].weight)[form])


def test_switch_is_read_at_construction(monkeypatch):
    assert arena_mod.mirror_enabled()
    monkeypatch.setenv("CYG_NO_ADAM_SHADOW", "1")
    assert not arena_mod.mirror_enabled()
    # a CPU group never takes the mirror by default: its kernels are HIP
    monkeypatch.delenv("CYG_NO_ADAM_SHADOW")
    a, _ = _build(Discriminator(), None, monkeypatch)
    assert a.mirror is None


# ---------------------------------------------------------------- GPU ----

def _assert_forms_equal(a, legacy):
    assert set(a._by_param) == set(legacy._by_param)
    n = 0
    for p, forms in a._by_param.items():
        assert set(forms) == set(legacy.forms_of(p))
        for name, v in forms.items():
            assert torch.equal(v, legacy.forms_of(p)[name]), \
                (name, a.source[p][name], tuple(p.shape))
            n += 1
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("graph_mode", [False, True])
def test_forms_after_an_optimizer_step_match_the_full_gather(monkeypatch,
                                                             graph_mode):
    from cyclegan_amd.ops.adam import FusedAdam
    for module in _models():
        module = module.to("cuda")
        group = FlatParamGroup(module)
        a = ShadowArena(group, module)
        assert a.mirror is not None and a.ttable.shape[0] > 0
        opt = FusedAdam(group.flat_param, group.flat_grad)
        opt.shadow = a.mirror
        g = torch.Generator().manual_seed(7)
        group.flat_grad.copy_(torch.randn(group.flat_grad.numel(),
                                          generator=g) * 0.02)
        # poison what the step must rewrite: a stale mirror would show
        a.mirror.fill_(float("nan"))
        a.tbuf.fill_(float("nan"))
        a.buf.fill_(float("nan"))
        before = group.flat_param.clone()
        if graph_mode:
            opt.prepare_graph()
            opt.advance_lr()
        opt.step()
        assert opt.wrote_shadow
        a.refresh(mirror_fresh=True)
        torch.cuda.synchronize()
        assert not torch.equal(before, group.flat_param)
        n = group.flat_param.numel()
        assert torch.equal(a.mirror[:n],
                           group.flat_param.to(torch.bfloat16))

        monkeypatch.setenv("CYG_NO_ADAM_SHADOW", "1")
        legacy = ShadowArena(group, module)
        monkeypatch.delenv("CYG_NO_ADAM_SHADOW")
        assert legacy.mirror is None
        assert set(k for s in legacy.source.values() for k in s.values()) \
            <= {"gather", "fold"}
        assert _assert_forms_equal(a, legacy) > 10

        # outside the optimizer the refresh fills the mirror itself
        with torch.no_grad():
            group.flat_param.mul_(1.25)
        a.refresh()
        legacy.refresh()
        torch.cuda.synchronize()
        _assert_forms_equal(a, legacy)


@pytest.mark.gpu
@pytest.mark.parametrize("upsample", ["transpose", "resize"])
def test_trainer_step_leaves_forms_equal_to_the_full_gather(tmp_path,
                                                            monkeypatch,
                                                            upsample):
    from cyclegan_amd.parallel import DistContext
    from cyclegan_amd.trainer import CycleGAN
    args = argparse.Namespace(output_dir=str(tmp_path), batch_size=1,
                              global_batch_size=1, num_residual_blocks=1,
                              compute_dtype=torch.bfloat16, upsample=upsample)
    torch.manual_seed(11)
    gan = CycleGAN(args, DistContext(device=torch.device("cuda", 0)))
    for name, a in gan.arenas.items():
        assert a.mirror is not None
        assert gan.optimizers[name].shadow is a.mirror
    x = torch.rand(1, 64, 64, 3, device="cuda") * 2 - 1
    y = torch.rand(1, 64, 64, 3, device="cuda") * 2 - 1
    gan.train_step(x, y)
    torch.cuda.synchronize()
    monkeypatch.setenv("CYG_NO_ADAM_SHADOW", "1")
    for name, a in gan.arenas.items():
        assert gan.optimizers[name].wrote_shadow
        legacy = ShadowArena(gan.groups[name], getattr(gan, name))
        assert legacy.mirror is None
        _assert_forms_equal(a, legacy)
