"""shadow_transpose (shadow.hip): the index-free [Cout,KH,KW,Cin] ->
[Cin,KH,KW,Cout] transpose of the dgrad weight forms, bit for bit against
torch, and the mirror cast that feeds it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 1024.0  # exact in bf16
GUARD = 64


def _ext():
    from cyclegan_amd.ops import backend
    return backend.ext()


def _weights(shapes, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) * 0.05 for s in shapes]


def _run(ws, src_offs, dst_offs):
    """Transpose every w (OHWI, fp32 on the host) placed at src_offs in a
    bf16 source buffer into dst_offs of a destination buffer; both buffers
    are sentinel-filled. Returns (dst buffer, the expected buffer)."""
    from cyclegan_amd.ops.arena import transpose_row
    n_src = max(o + w.numel() for o, w in zip(src_offs, ws)) + GUARD
    n_dst = max(o + w.numel() for o, w in zip(dst_offs, ws)) + GUARD
    src = torch.full((n_src,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    dst = torch.full((n_dst,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    want = dst.clone()
    rows, blocks = [], 0
    for w, so, do in zip(ws, src_offs, dst_offs):
        wd = w.to(DEV)
        src[so:so + w.numel()].copy_(wd.to(torch.bfloat16).reshape(-1))
        want[do:do + w.numel()].copy_(
            wd.permute(3, 1, 2, 0).contiguous().to(torch.bfloat16).reshape(-1))
        row = transpose_row(so, do, tuple(w.shape), blocks)
        rows.append(row)
        blocks += row[3] * row[6] * row[7]
    table = torch.tensor(rows, dtype=torch.int32)
    _ext().shadow_transpose(src, table, table.to(DEV), dst)
    torch.cuda.synchronize()
    return dst, want


@pytest.mark.parametrize("shape", [(8, 1, 1, 8), (64, 3, 3, 64),
                                   (128, 4, 4, 64), (24, 3, 3, 40),
                                   (256, 3, 3, 256)])
def test_transpose_matches_torch(shape):
    (w,) = _weights([shape])
    dst, want = _run([w], [0], [0])
    assert torch.equal(dst, want)


def test_two_layers_second_at_an_odd_multiple_of_8():
    ws = _weights([(8, 1, 1, 8), (24, 3, 3, 40)], seed=1)
    # 64 elements, then a gap: the second layer starts at 8*9 on the source
    # side and 8*11 on the destination side
    dst, want = _run(ws, [0, 72], [0, 88])
    assert torch.equal(dst, want)
    assert (dst[64:88] == SENTINEL).all()


def test_binding_rejects_bad_tables():
    ext = _ext()
    from cyclegan_amd.ops.arena import transpose_row
    src = torch.zeros(64 * 9 * 64, dtype=torch.bfloat16, device=DEV)
    dst = torch.zeros_like(src)
    good = transpose_row(0, 0, (64, 3, 3, 64), 0)

    def call(row, s=src, d=dst):
        t = torch.tensor([row], dtype=torch.int32)
        ext.shadow_transpose(s, t, t.to(DEV), d)

    call(good)
    for i, val in [(0, 4), (1, 4), (0, 8), (1, 8),      # alignment, bounds
                   (2, 60), (4, 60), (2, 128),          # channels, bounds
                   (5, 1), (6, 2), (7, 2), (3, 10)]:    # block layout, bounds
        row = list(good)
        row[i] = val
        with pytest.raises(RuntimeError):
            call(row)
    with pytest.raises(RuntimeError):
        call(good, s=src[8:])          # source too short
    with pytest.raises(RuntimeError):
        call(good, d=dst.float())      # dtype
    t = torch.tensor([good], dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ext.shadow_transpose(src, t, t, dst)        # device table on host
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [1, 7, 8, 1027, 4096 + 13])
def test_mirror_cast(n):
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n, generator=g) * 0.05).to(DEV)
    out = torch.full((n + (-n) % 8 + 8,), SENTINEL, dtype=torch.bfloat16,
                     device=DEV)
    _ext().shadow_cast(x, out)
    torch.cuda.synchronize()
    assert torch.equal(out[:n], x.to(torch.bfloat16))
    assert (out[n:] == SENTINEL).all()


def test_ineligible_shape_stays_on_the_gather():
    """(3,7,7,64): Cout is no multiple of 8 (and padded), so both forms
    come from the gather, unchanged; an eligible layer beside it does
    not."""
    from cyclegan_amd.models.layers import ConvNHWC
    from cyclegan_amd.ops.arena import ShadowArena
    from cyclegan_amd.ops.shadow import _pad_dims
    from cyclegan_amd.parallel import FlatParamGroup
    torch.manual_seed(0)
    mod = torch.nn.Sequential(ConvNHWC(64, 3, 7), ConvNHWC(64, 64, 3)).to(DEV)
    group = FlatParamGroup(mod)
    arena = ShadowArena(group, mod)
    legacy = ShadowArena(group, mod, mirror=False)
    torch.cuda.synchronize()
    odd, reg = mod[0].weight, mod[1].weight
    assert tuple(odd.shape) == (3, 7, 7, 64)
    assert arena.source[odd] == {"p": "gather", "tp": "gather"}
    assert arena.source[reg] == {"p": "mirror", "tp": "transpose"}
    assert arena.ttable.shape[0] == 1
    want_p = _pad_dims(odd.detach()).to(torch.bfloat16)
    for a in (arena, legacy):
        assert torch.equal(a.forms_of(odd)["p"], want_p)
        assert torch.equal(a.forms_of(odd)["tp"],
                           want_p.permute(3, 1, 2, 0).contiguous())
    for form in ("p", "tp"):
        assert torch.equal(arena.forms_of(reg)[form],
                           legacy.forms_of(reg)[form])
