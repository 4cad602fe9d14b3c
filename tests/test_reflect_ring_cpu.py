"""Index logic of the reflect dgrad that writes the unpadded frame, in
pure torch on the CPU.

The functions below restate, line for line, the index arithmetic of
cyclegan_amd/ops/_hip/conv.hip: ring_index (where the gather puts a
padded-frame pixel outside the window), mirror_span (which rows / columns
of the image have a mirror source), span_nth / span_nth_out (how
reflect_ring_add_kernel enumerates its pixels) and the kernel's candidate
loop. The emulation builds dx the way the GPU does: window rows direct,
ring rows to the side image, ring add in place, in launch order. It must
equal the pad's adjoint applied to the same padded frame.

All sums here are fp64: a sum of at most nine bf16 values is exact there,
so the order of the additions cannot hide or fake an index error, and both
sides round once to bf16.
"""

import pytest
import torch

import _kernel_bounds as kb

REFLECT_CASES = ["nsq_reflect", "cin24", "cin96", "reflect_asym",
                 "k7_padmax", "ow64_short", "grid8"]
# pad combinations the table lacks: one side only on each axis, pad = n-1
# on one side only, the two intervals of an axis exactly touching
EXTRA_PADS = [(5, 7, (1, 0, 0, 1)), (5, 7, (0, 1, 1, 0)),
              (4, 6, (3, 0, 0, 5)), (4, 6, (0, 3, 5, 0)),
              (5, 8, (2, 2, 3, 4)), (6, 9, (2, 2, 1, 1)),
              (2, 2, (1, 1, 1, 1)), (3, 5, (0, 0, 2, 0))]


def ring_index(qh, qw, OH, OW, wt, wl, wH, wW):
    if qh < wt:
        return qh * OW + qw
    if qh >= wt + wH:
        return (qh - wH) * OW + qw
    return (OH - wH) * OW + (qh - wt) * (OW - wW) + (qw if qw < wl
                                                     else qw - wW)


def mirror_span(n, lo, hi):
    a0, b0 = 1, min(lo, n - 1)
    a1, b1 = max(n - 1 - hi, 0), n - 2
    n0, n1 = max(b0 - a0 + 1, 0), max(b1 - a1 + 1, 0)
    if n0 == 0:
        return (a1, n1, a1 + n1, 0)
    if n1 == 0:
        return (a0, n0, a0 + n0, 0)
    if a1 <= a0 + n0:
        a, b = min(a0, a1), max(b0, b1)
        return (a, b - a + 1, b + 1, 0)
    return (a0, n0, a1, n1)


def span_nth(s, k):
    return s[0] + k if k < s[1] else s[2] + (k - s[1])


def span_nth_out(s, k):
    if k >= s[0]:
        k += s[1]
    if k >= s[2]:
        k += s[3]
    return k


def mirror_idx(i, n):
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * n - 2 - i
    return i


def candidates(i, p_lo, n, np_):
    """Padded-frame indices that fold onto i along one axis, in
    reflect_fold_kernel's order and with its de-duplication."""
    c = [p_lo + i, p_lo - i, p_lo + 2 * (n - 1) - i]
    out = []
    for a, q in enumerate(c):
        if q < 0 or q >= np_:
            continue
        if a > 0 and q == c[0]:
            continue
        if a == 2 and q == c[1]:
            continue
        if mirror_idx(q - p_lo, n) != i:
            continue
        out.append((a, q))
    return out


def emulate_direct_fold(dxp, H, W, pads):
    """dxp: [B,HP,WP,C] fp64 holding bf16 values. Returns dx [B,H,W,C] as
    bf16 and the set of pixels the ring add visited."""
    pt, pb, pl, pr = pads
    B, HP, WP, C = dxp.shape
    rp = HP * WP - H * W
    dx = torch.full((B, H, W, C), float("nan"), dtype=torch.float64)
    ring = torch.full((B * rp, C), float("nan"), dtype=torch.float64)
    # the gather's row decode
    for b in range(B):
        for oh in range(HP):
            for ow in range(WP):
                i, j = oh - pt, ow - pl
                if 0 <= i < H and 0 <= j < W:
                    dx[b, i, j] = dxp[b, oh, ow]
                else:
                    k = b * rp + ring_index(oh, ow, HP, WP, pt, pl, H, W)
                    assert 0 <= k < B * rp
                    assert torch.isnan(ring[k]).all(), "ring slot reused"
                    ring[k] = dxp[b, oh, ow]
    assert not torch.isnan(ring).any(), "ring slot never written"
    # reflect_ring_add_kernel, one pixel per step, in place
    rs, cs = mirror_span(H, pt, pb), mirror_span(W, pl, pr)
    nr, nc = rs[1] + rs[3], cs[1] + cs[3]
    assert rs[0] + rs[1] <= rs[2] and cs[0] + cs[1] <= cs[2]
    ppb = nr * W + (H - nr) * nc
    seen = set()
    for b in range(B):
        for q in range(ppb):
            if q < nr * W:
                i, j = span_nth(rs, q // W), q % W
            else:
                q2 = q - nr * W
                i, j = span_nth_out(rs, q2 // nc), span_nth(cs, q2 % nc)
            assert 0 <= i < H and 0 <= j < W
            assert (b, i, j) not in seen, "pixel visited twice"
            seen.add((b, i, j))
            s = torch.zeros(C, dtype=torch.float64)
            for a, qh in candidates(i, pt, H, HP):
                for d, qw in candidates(j, pl, W, WP):
                    if a == 0 and d == 0:
                        s += dx[b, i, j]
                    else:
                        s += ring[b * rp + ring_index(qh, qw, HP, WP, pt,
                                                      pl, H, W)]
            dx[b, i, j] = s.to(torch.bfloat16).to(torch.float64)
    return dx.to(torch.bfloat16), seen


def check(dxp_bf16, H, W, pads, adjoint):
    dx, seen = emulate_direct_fold(dxp_bf16.to(torch.float64), H, W, pads)
    want = adjoint(dxp_bf16.to(torch.float64)).to(torch.bfloat16)
    assert torch.equal(dx, want)
    # the visited set is exactly the pixels with more than one source
    pt, pb, pl, pr = pads
    B, HP, WP, _ = dxp_bf16.shape
    for i in range(H):
        for j in range(W):
            n = len(candidates(i, pt, H, HP)) * len(candidates(j, pl, W, WP))
            assert n >= 1
            assert ((0, i, j) in seen) == (n > 1), (i, j, n)


@pytest.mark.parametrize("cid", REFLECT_CASES)
def test_direct_fold_index_logic(cid):
    case = kb.CASE_BY_ID[cid]
    _, w, _, dy = kb.make_inputs(case)
    f = torch.float32
    dxp = kb.rne(kb.dgrad_padded(case, dy.to(f), w.to(f))).to(torch.bfloat16)
    check(dxp, case.H, case.W, case.pads,
          lambda tp: kb.pad_adjoint(case, tp))


@pytest.mark.parametrize("H,W,pads", EXTRA_PADS)
def test_direct_fold_index_logic_extra_pads(H, W, pads):
    pt, pb, pl, pr = pads
    case = kb.Case("extra", "conv", 2, H, W, 8, 8, 3, 3, 1, pads, True, "")
    dxp = kb.uniform_bf16((2, H + pt + pb, W + pl + pr, 8), 77)
    check(dxp, H, W, pads, lambda tp: kb.pad_adjoint(case, tp))
