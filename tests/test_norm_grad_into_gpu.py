"""instnorm_bwd and channel_sum with gradient destinations: dgamma / dbeta /
bias gradients accumulated straight into slices of a flat buffer.

Destinations are views at odd float offsets inside a NaN-filled buffer; the
NaNs around them must survive. dx must not depend on where dgamma/dbeta go.

Bounds. dgamma[c] = sum over M = B*HW positions of d*xhat, dbeta[c] the sum
of d, d the activation-masked dy. Each addend is formed in fp32 from exact
bf16 inputs with at most three roundings, the M-term sum (slab partials,
then fp32 atomics over the batch, in no fixed order) adds (M-1)*u32:
|err| <= 2*M*u32*sum|addend|. With accumulate the prior joins as one more
addend of the atomics and the final value is rounded: one more
u32*|result| (taken on prior + reference). The bias gradient is the bound
of docs/KERNELS.md: 2*M*u32*sum|dy|.

All tests @pytest.mark.gpu.
"""

import pytest
import torch

import _kernel_bounds as kb
from cyclegan_amd.ops import backend

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ACTS = {"none": kb.ACT_NONE, "relu": kb.ACT_RELU}


def dev(t):
    return t.to(DEV).contiguous()


def nan_slices(*sizes):
    """A NaN-filled buffer and one view per size, each at an odd float
    offset, with NaN gaps between them."""
    offs, off = [], 5
    for n in sizes:
        offs.append(off)
        off += n + 7 + (n + 1) % 2      # keeps every offset odd
    buf = torch.full((off,), float("nan"), device=DEV)
    return buf, [buf[o:o + n] for o, n in zip(offs, sizes)]


def assert_gaps_nan(buf, views):
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
    base = buf.data_ptr()
    for v in views:
        o = (v.data_ptr() - base) // 4
        assert o % 2 == 1
        keep[o:o + v.numel()] = False
    assert torch.isnan(buf[keep]).all(), "wrote outside the destinations"


_fwd = {}


def norm_case(shape, act):
    """Inputs and forward results of one case, made once."""
    key = (shape, act)
    if key not in _fwd:
        g = torch.Generator().manual_seed(61)
        x = kb.uniform_bf16(shape, 62)
        dy = kb.uniform_bf16(shape, 63)
        gamma = torch.randn(shape[3], generator=g) * 0.5
        beta = torch.randn(shape[3], generator=g) * 0.1
        y, mean, rstd = backend.ext().instnorm_fwd(
            dev(x), dev(gamma), dev(beta), 1e-3, ACTS[act], kb.SLOPE, None)
        # fp64 reference from the tensors the backward kernels read
        d = dy.double()
        if act == "relu":
            d = d * (y.cpu().double() > 0)
        xh = ((x.double() - mean.cpu().double()[:, None, None])
              * rstd.cpu().double()[:, None, None])
        M = shape[0] * shape[1] * shape[2]
        ref = {"dgamma": (d * xh).sum((0, 1, 2)), "dbeta": d.sum((0, 1, 2)),
               "bgamma": 2 * M * kb.U32 * (d * xh).abs().sum((0, 1, 2)),
               "bbeta": 2 * M * kb.U32 * d.abs().sum((0, 1, 2))}
        _fwd[key] = (dev(x), dev(dy), dev(gamma), dev(beta), y, mean, rstd,
                     ref)
    return _fwd[key]


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accum"])
@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("shape", [(2, 16, 16, 64), (2, 8, 8, 256)],
                         ids=["16x16x64", "8x8x256"])
def test_instnorm_bwd_into(shape, act, accumulate):
    ext = backend.ext()
    x, dy, gamma, beta, y, mean, rstd, ref = norm_case(shape, act)
    C = shape[3]
    yact = y if act != "none" else None
    dx0, dg0, db0 = ext.instnorm_bwd(dy, x, gamma, mean, rstd, yact,
                                     ACTS[act], kb.SLOPE, beta)
    buf, (dg, db) = nan_slices(C, C)
    rg, rb = ref["dgamma"], ref["dbeta"]
    bg, bb = ref["bgamma"], ref["bbeta"]
    if accumulate:
        pg = kb.uniform_bf16((C,), 64).float()
        pb = kb.uniform_bf16((C,), 65).float()
        dg.copy_(pg)
        db.copy_(pb)
        rg, rb = rg + pg.double(), rb + pb.double()
        bg, bb = bg + kb.U32 * rg.abs(), bb + kb.U32 * rb.abs()
    dx1, dg1, db1 = ext.instnorm_bwd(dy, x, gamma, mean, rstd, yact,
                                     ACTS[act], kb.SLOPE, beta, dg, db,
                                     accumulate)
    assert dg1.data_ptr() == dg.data_ptr() and db1.data_ptr() == db.data_ptr()
    assert_gaps_nan(buf, [dg, db])
    assert torch.equal(dx1, dx0)
    tag = f"in_bwd:{shape[1]}x{shape[3]}:{act}:{accumulate}"
    kb.assert_within(dg, rg, bg, f"{tag}:dgamma", "c")
    kb.assert_within(db, rb, bb, f"{tag}:dbeta", "c")
    if not accumulate:  # and the call without destinations, same bound
        kb.assert_within(dg0, rg, bg, f"{tag}:dgamma0", "c")
        kb.assert_within(db0, rb, bb, f"{tag}:dbeta0", "c")


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accum"])
@pytest.mark.parametrize("shape,nout", [((2, 6, 10, 8), 8), ((2, 6, 10, 8), 3),
                                        ((2, 8, 8, 64), 64)],
                         ids=["6x10x8", "6x10x8_crop3", "8x8x64"])
def test_channel_sum_into(shape, nout, accumulate):
    """nout < C: the destination is a bias of the unpadded channel count."""
    ext = backend.ext()
    dy = kb.uniform_bf16(shape, 66)
    ref, bound = kb.dbias_ref_bound(dy)
    ref, bound = ref[:nout], bound[:nout]
    buf, (out,) = nan_slices(nout)
    if accumulate:
        prior = kb.uniform_bf16((nout,), 67).float()
        out.copy_(prior)
        ref = ref + prior.double()
        bound = bound + kb.U32 * ref.abs()
    got = ext.channel_sum(dev(dy), out, accumulate)
    assert got.data_ptr() == out.data_ptr()
    assert_gaps_nan(buf, [out])
    kb.assert_within(out, ref, bound, f"channel_sum:{shape}:{nout}", "c")
    # the form without a destination is unchanged
    kb.assert_within(ext.channel_sum(dev(dy)), *kb.dbias_ref_bound(dy),
                     f"channel_sum:{shape}:plain", "c")
