"""The bounds of tests/_kernel_bounds.py, proved on the CPU.

For every case of the edge-shape tables an emulation of the kernels'
arithmetic (the fp32 reference, rounded to bf16 where the kernel rounds)
must satisfy every bound, and each subtly wrong variant must violate it
in at least one element. This is what shows that tests/
test_conv_edges_gpu.py can fail.
"""

import pytest
import torch

import _kernel_bounds as kb
from cyclegan_amd.ops.conv import _conv_ref, _convt_ref

IDS = [c.id for c in kb.ALL_CASES]


class _Cache:
    """References are computed once per case and shared."""

    def __init__(self):
        self.d = {}

    def get(self, case):
        if case.id not in self.d:
            x, w, bias, dy = kb.make_inputs(case)
            self.d[case.id] = dict(
                x=x, w=w, bias=bias, dy=dy,
                fwd=kb.fwd_ref_bound(case, x, w),
                dgrad=kb.dgrad_ref_bound(case, dy, w),
                wgrad=kb.wgrad_ref_bound(case, x, dy))
        return self.d[case.id]


_cache = _Cache()


def _is_reflect(case):
    return case.kind == "conv" and case.reflect


def for_cases(pred=lambda c: True):
    """Parametrise over the cases a variant applies to."""
    sel = [c for c in kb.ALL_CASES if pred(c)]
    return pytest.mark.parametrize("case", sel, ids=[c.id for c in sel])


# ------------------------------------------------------- references ----
def test_case_tables_complete():
    """The tables keep every row the kernels' branches were read for."""
    assert len(kb.CONV_CASES) >= 19 and len(kb.CONVT_CASES) >= 6
    assert len(set(IDS)) == len(IDS)
    for c in kb.ALL_CASES:
        oh, ow = c.out_hw
        assert oh >= 1 and ow >= 1, c.id


def test_local_refs_agree_with_ops_refs():
    """The references written in _kernel_bounds against ops.conv's
    _conv_ref/_convt_ref, both in fp64: the same sums in (at most)
    another order, so they agree to a few fp64 ulps of the magnitude
    sum."""
    d = torch.float64
    for case in kb.ALL_CASES:
        x, w, bias, _ = kb.make_inputs(case)
        xf, wf, bf = x.to(d), w.to(d), bias.to(d)
        mine = kb.case_fwd_lin(case, xf, wf, bf)
        if case.kind == "conv":
            theirs = _conv_ref(xf, wf, bf, case.stride, case.pads,
                               "reflect" if case.reflect else "zeros")
        else:
            pt, _, pl, _ = case.pads
            theirs = _convt_ref(xf, wf, bf, case.stride, pt, pl,
                                *case.out_hw)
        assert mine.shape == theirs.shape == case.y_shape, case.id
        K = case.KH * case.KW * case.Cin + 1
        S = kb.case_fwd_lin(case, xf.abs(), wf.abs(), bf.abs())
        assert ((mine - theirs).abs() <= 2 * K * 2.0 ** -53 * S).all(), \
            case.id


def test_dgrad_padded_folds_to_dgrad():
    """fold(dgrad wrt the padded frame) == dgrad through the reflect pad
    (the identity the reflect bound rests on)."""
    d = torch.float64
    for case in kb.CONV_CASES:
        if not case.reflect:
            continue
        _, w, _, dy = kb.make_inputs(case)
        a = kb.pad_adjoint(case, kb.dgrad_padded(case, dy.to(d), w.to(d)))
        b = kb.case_dgrad(case, dy.to(d), w.to(d))
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-12), case.id


def test_rounding_helpers():
    t = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -9, -1.0 - 2.0 ** -8,
                      1.0 + 2.0 ** -8])
    # RNE: up / tie to even (down) / tie to even (down)
    assert kb.rne(t).tolist() == [1.0 + 2.0 ** -7, -1.0, 1.0]
    assert kb.trunc(t).tolist() == [1.0, -1.0, 1.0]


def test_assert_within_reports_worst_index():
    ref = torch.zeros(2, 3, 4, 5, dtype=torch.float64)
    bound = torch.full_like(ref, 1e-3)
    got = ref.clone().float()
    kb.assert_within(got, ref, bound, "ok")
    got[1, 2, 0, 3] = 0.5
    got[0, 1, 1, 1] = 0.01
    with pytest.raises(AssertionError) as ei:
        kb.assert_within(got, ref, bound, "t", "okki")
    msg = str(ei.value)
    assert "2/120 elements" in msg and "co=1, kh=2, kw=0, ci=3" in msg
    # a zero bound demands exact equality; NaN never passes
    bound[0, 0, 0, 0] = 0
    assert kb.violations(ref, ref, bound) == 0
    got = ref.clone()
    got[0, 0, 0, 0] = 1e-30
    assert kb.violations(got, ref, bound) == 1
    got[0, 0, 0, 0] = float("nan")
    assert kb.violations(got, ref, bound) == 1


# -------------------------------------------------------- emulation ----
@for_cases()
def test_emulation_within_bounds(case):
    c = _cache.get(case)
    kb.assert_within(kb.emu_fwd(case, c["x"], c["w"]), *c["fwd"],
                     f"{case.id}:y")
    kb.assert_within(kb.emu_dgrad(case, c["dy"], c["w"]), *c["dgrad"],
                     f"{case.id}:dx")
    kb.assert_within(kb.emu_wgrad(case, c["x"], c["dy"]), *c["wgrad"],
                     f"{case.id}:dw", "okki")


@pytest.mark.parametrize("cid,act", kb.FWD_ACT_CASES,
                         ids=[f"{c}-{a}" for c, a in kb.FWD_ACT_CASES])
def test_emulation_within_bounds_bias_act(cid, act):
    case = kb.CASE_BY_ID[cid]
    c = _cache.get(case)
    ref, bound = kb.fwd_ref_bound(case, c["x"], c["w"], c["bias"], act)
    kb.assert_within(kb.emu_fwd(case, c["x"], c["w"], c["bias"], act), ref,
                     bound, f"{cid}:{act}:y")
    # and the bound can fail there too: a missing bias, the activation
    # left out, truncation (not for tanh: its outputs saturate below 1,
    # where one bf16 ulp is about the size of e)
    got = kb.emu_fwd(case, c["x"], c["w"], None, act)
    assert kb.violations(got, ref, bound) > 0
    if act is not None:
        got = kb.emu_fwd(case, c["x"], c["w"], c["bias"], None)
        assert kb.violations(got, ref, bound) > 0
    if act != "tanh":
        got = kb.emu_fwd(case, c["x"], c["w"], c["bias"], act, rnd=kb.trunc)
        assert kb.violations(got, ref, bound) > 0


def test_emulation_in_and_dbias_bounds():
    """The InstanceNorm and bias-gradient bounds against an fp32
    emulation (sum / sum of squares in fp32, as the kernels do)."""
    g = torch.Generator().manual_seed(5)
    for shape, (mu, sd) in [((2, 11, 13, 64), (4.0, 1.0)),
                            ((2, 16, 16, 256), (8.0, 0.5))]:
        x = (torch.randn(shape, generator=g) * sd + mu).to(torch.bfloat16)
        gamma = torch.randn(shape[3], generator=g) * 0.5
        beta = torch.randn(shape[3], generator=g) * 0.1
        (y, m, r), (by, bm, br), dmax = kb.in_ref_bounds(x, gamma, beta,
                                                         1e-3)
        # d is about 0.016 for the second input (HW = 256, mean^2/var =
        # 256) and up to a quarter more where a sample's variance comes
        # out low: the bf16 rounding term still dominates the bound
        assert dmax <= 0.025
        xf = x.float()
        HW = shape[1] * shape[2]
        mean = xf.sum((1, 2)) / HW
        var = (xf * xf).sum((1, 2)) / HW - mean * mean
        rstd = (var + 1e-3).rsqrt()
        yy = kb.rne((xf - mean[:, None, None]) * rstd[:, None, None]
                    * gamma + beta)
        kb.assert_within(yy, y, by, "in:y")
        kb.assert_within(mean, m, bm, "in:mean", "bc")
        kb.assert_within(rstd, r, br, "in:rstd", "bc")
        # a biased mean (one element left out of the sum) is rejected
        mean2 = (xf.sum((1, 2)) - xf[:, 0, 0]) / HW
        assert kb.violations(mean2, m, bm) > 0
    dy = kb.uniform_bf16((1, 9, 24, 8), 7)
    ref, bound = kb.dbias_ref_bound(dy)
    kb.assert_within(dy.float().sum((0, 1, 2)), ref, bound, "db", "c")
    assert kb.violations(dy.float()[:, :-1].sum((0, 1, 2)), ref, bound) > 0


# --------------------------------------------------- wrong variants ----
def _tap(case):
    """A tap away from the corner where both exist."""
    return min(1, case.KH - 1), case.KW - 1


@for_cases()
def test_rejects_dropped_channel_chunk(case):
    """One 8-channel chunk of one tap missing from the K loop (all
    channels of the tap where Cin < 8)."""
    c = _cache.get(case)
    kh, kw = _tap(case)
    w2 = c["w"].clone()
    c0 = 8 if case.Cin >= 16 else 0
    w2[:, kh, kw, c0:c0 + 8] = 0
    assert kb.violations(kb.emu_fwd(case, c["x"], w2), *c["fwd"]) > 0
    # the same in dgrad: a chunk of output channels of one tap
    w3 = c["w"].clone()
    w3[0:8, kh, kw, :] = 0
    assert kb.violations(kb.emu_dgrad(case, c["dy"], w3), *c["dgrad"]) > 0
    # and in wgrad: the chunk's dw comes out zero
    dw = kb.emu_wgrad(case, c["x"], c["dy"])
    dw[:, kh, kw, c0:c0 + 8] = 0
    assert kb.violations(dw, *c["wgrad"]) > 0


@for_cases()
def test_rejects_truncation(case):
    c = _cache.get(case)
    got = kb.emu_fwd(case, c["x"], c["w"], rnd=kb.trunc)
    assert kb.violations(got, *c["fwd"]) > 0
    got = kb.emu_dgrad(case, c["dy"], c["w"], rnd=kb.trunc)
    if _is_reflect(case) and max(case.pads) >= min(case.H, case.W) - 1:
        # pad = H-1: every dx element is the sum of up to nine rounded
        # mirror images, so the bound rightly allows nine roundings of
        # terms much larger than the result, and truncation's extra half
        # ulp per term hides inside it. The forward check above stands.
        return
    assert kb.violations(got, *c["dgrad"]) > 0


@for_cases(_is_reflect)
def test_rejects_replicate_padding(case):
    c = _cache.get(case)
    got = kb.emu_fwd(case, c["x"], c["w"], pad_mode="replicate")
    assert kb.violations(got, *c["fwd"]) > 0
    got = kb.emu_wgrad(case, c["x"], c["dy"], pad_mode="replicate")
    assert kb.violations(got, *c["wgrad"]) > 0
    f = torch.float32
    got = kb.rne(kb.pad_adjoint(
        case, kb.rne(kb.dgrad_padded(case, c["dy"].to(f), c["w"].to(f))),
        "replicate"))
    assert kb.violations(got, *c["dgrad"]) > 0


@for_cases(lambda c: c.kind == "conv" and c.pads[0] != c.pads[2])
def test_rejects_swapped_pt_pl(case):
    c = _cache.get(case)
    pt, pb, pl, pr = case.pads
    f = torch.float32
    x, w = c["x"].to(f), c["w"].to(f)
    if case.reflect:
        # same totals, top/left exchanged
        sw = (pl, pt + pb - pl, pt, pl + pr - pt)
        assert min(sw) >= 0
        got = kb.rne(kb.conv_fwd_lin(x, w, None, case.stride, sw,
                                     "reflect"))
    else:
        # the helper reproduces the case when given its own pt, pl
        same = kb.rne(kb.conv_fwd_shifted(case, x, w, pt, pl))
        assert kb.violations(same, *c["fwd"]) == 0
        got = kb.rne(kb.conv_fwd_shifted(case, x, w, pl, pt))
    assert got.shape == case.y_shape
    assert kb.violations(got, *c["fwd"]) > 0


@for_cases(lambda c: c.KH == c.KW and c.KH > 1)
def test_rejects_transposed_kernel(case):
    """Weights with kh and kw exchanged (an H/W mix-up in the tap
    decode)."""
    c = _cache.get(case)
    wt = c["w"].transpose(1, 2).contiguous()
    assert kb.violations(kb.emu_fwd(case, c["x"], wt), *c["fwd"]) > 0
    assert kb.violations(kb.emu_dgrad(case, c["dy"], wt), *c["dgrad"]) > 0
    dw = kb.emu_wgrad(case, c["x"], c["dy"]).transpose(1, 2)
    assert kb.violations(dw, *c["wgrad"]) > 0


@for_cases()
def test_rejects_dropped_wgrad_row(case):
    """The last of the M rows left out of the wgrad sum."""
    c = _cache.get(case)
    if case.kind == "conv":
        dy2 = c["dy"].clone()
        dy2[-1, -1, -1, :] = 0
        got = kb.emu_wgrad(case, c["x"], dy2)
    else:
        x2 = c["x"].clone()
        x2[-1, -1, -1, :] = 0
        got = kb.emu_wgrad(case, x2, c["dy"])
    assert kb.violations(got, *c["wgrad"]) > 0


@for_cases(_is_reflect)
def test_rejects_missing_mirror_term(case):
    """One padded-frame pixel left out of the reflect fold."""
    c = _cache.get(case)
    got = kb.emu_dgrad(case, c["dy"], c["w"], drop_mirror=True)
    assert kb.violations(got, *c["dgrad"]) > 0


def test_variant_applicability():
    """Each variant has the cases the issue names for it: reflect cases,
    at least two cases with pt != pl, square kernels."""
    assert sum(_is_reflect(c) for c in kb.ALL_CASES) >= 8
    assert sum(c.kind == "conv" and c.pads[0] != c.pads[2]
               for c in kb.ALL_CASES) >= 2
