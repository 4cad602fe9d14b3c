"""Row order of the direct-fold reflect dgrad: window tiles first (the
forward conv's tiles), then the ring pixels in four classes whose tiles
walk only the taps that can reach dy (conv.hip, ReflectOrder).

Only the enumeration of GEMM rows changed, and a trimmed tap adds exact
zeros in the untrimmed walk, so dx must be torch.equal between the default,
CYG_DGRAD_FRAME_ORDER=1 (padded-frame order, every tap) and
CYG_NO_DIRECT_FOLD=1 (full-frame fold), and within the fp64 bound of
_kernel_bounds.dgrad_ref_bound. Shapes: every reflect row of the case
table plus the four below.

reflect_dgrad_rowmap returns the table that the kernel's prologue decodes
from (reflect_row, run on the host); the row-map tests state the order's
properties on it with nothing left out.

All tests @pytest.mark.gpu.
"""

import numpy as np
import pytest
import torch

import _kernel_bounds as kb
from cyclegan_amd.ops import backend
from test_reflect_ring_cpu import EXTRA_PADS, ring_index

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BM = 128

NEW_CASES = [
    kb.Case("ro_bnt128", "conv", 2, 8, 16, 128, 64, 3, 3, 1, (1, 1, 1, 1),
            True, "128-wide n-tile on dx; H*W = 128: window tiles aligned to "
            "samples, 2 window tiles; tile count not a multiple of 8"),
    kb.Case("ro_xcd", "conv", 4, 8, 16, 128, 128, 3, 3, 1, (1, 1, 1, 1),
            True, "4 window tiles x 2 n-tiles = 8: XCD remap on over the "
            "window part, ring tiles behind it"),
    kb.Case("ro_asym", "conv", 3, 5, 12, 64, 64, 3, 3, 1, (1, 2, 2, 1),
            True, "window tiles straddle samples; M tail in the last window "
            "tile; four classes of different sizes; two-wide tap windows"),
    kb.Case("ro_k5", "conv", 1, 3, 8, 64, 64, 5, 5, 1, (2, 2, 2, 2),
            True, "pad = H-1 with an odd kernel other than the head's"),
]
NEW_BY_ID = {c.id: c for c in NEW_CASES}
TABLE_CASES = [c for c in kb.CONV_CASES if c.reflect and c.stride == 1]
ALL = {c.id: c for c in TABLE_CASES + NEW_CASES}

_inputs = {}
_refs = {}


def inputs(case):
    if case.id not in _inputs:
        if case.id in kb.CASE_BY_ID:
            _, w, _, dy = kb.make_inputs(case)
        else:
            s = 7000 + 10 * NEW_CASES.index(case)
            w = kb.uniform_bf16(case.w_shape, s + 1, 0.2)
            dy = kb.uniform_bf16(case.y_shape, s + 3)
        _inputs[case.id] = (dy.to(DEV).contiguous(),
                            w.permute(3, 1, 2, 0).contiguous().to(DEV),
                            dy, w)
    return _inputs[case.id]


def ref(case):
    if case.id not in _refs:
        _, _, dy, w = inputs(case)
        _refs[case.id] = kb.dgrad_ref_bound(case, dy, w)
    return _refs[case.id]


def run_dgrad(case):
    dyd, wtd, _, _ = inputs(case)
    return backend.ext().conv2d_dgrad(dyd, wtd, case.H, case.W, case.stride,
                                      *case.pads, case.reflect)


def clear_switches(monkeypatch):
    monkeypatch.delenv("CYG_NO_DIRECT_FOLD", raising=False)
    monkeypatch.delenv("CYG_DGRAD_FRAME_ORDER", raising=False)


@pytest.mark.parametrize("cid", sorted(ALL))
def test_orders_bit_equal(cid, monkeypatch):
    case = ALL[cid]
    assert case.reflect and case.stride == 1
    clear_switches(monkeypatch)
    new = run_dgrad(case)
    monkeypatch.setenv("CYG_DGRAD_FRAME_ORDER", "1")
    frame = run_dgrad(case)
    monkeypatch.delenv("CYG_DGRAD_FRAME_ORDER")
    monkeypatch.setenv("CYG_NO_DIRECT_FOLD", "1")
    full = run_dgrad(case)
    assert tuple(new.shape) == case.x_shape and new.is_contiguous()
    # both orders are the direct fold (dx heads the padded-frame
    # allocation), the full-frame fold returns its own tensor
    assert new.untyped_storage().nbytes() > new.numel() * 2
    assert frame.untyped_storage().nbytes() > frame.numel() * 2
    assert full.untyped_storage().nbytes() == full.numel() * 2
    assert torch.equal(new, frame)
    assert torch.equal(new, full)
    kb.assert_within(new, *ref(case), f"{cid}:dx window/ring order")
    kb.assert_within(frame, *ref(case), f"{cid}:dx frame order")


@pytest.mark.parametrize("cid", ["ro_bnt128", "ro_asym"])
def test_no_element_read_before_written(cid, monkeypatch):
    """With the allocator's free memory full of NaN, a dx or ring element
    that the ring add read before the gather wrote it would show."""
    case = NEW_BY_ID[cid]
    clear_switches(monkeypatch)
    a = run_dgrad(case).clone()
    junk = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
    junk.view(torch.bfloat16).fill_(float("nan"))
    del junk
    b = run_dgrad(case)
    assert torch.isfinite(b).all()
    assert torch.equal(a, b)
    kb.assert_within(b, *ref(case), f"{cid}:dx after NaN fill")


# ------------------------------------------------------------ row map ----
MAP_SHAPES = [(c.id, c.B, c.H, c.W, c.pads, c.KH, c.KW)
              for c in TABLE_CASES + NEW_CASES]
MAP_SHAPES += [(f"extra{n}", 2, H, W, pads, 3, 3)
               for n, (H, W, pads) in enumerate(EXTRA_PADS)]


def rowmap(B, H, W, pads, KH, KW, **kw):
    t = backend.ext().reflect_dgrad_rowmap(B, H, W, *pads, KH, KW, **kw)
    assert t.dtype == torch.int32 and t.shape[1] == 10
    assert t.shape[0] % BM == 0
    t = t.numpy().astype(np.int64)
    cols = "ok b qh qw cls kh0 kh1 kw0 kw1 dst".split()
    return {k: t[:, n] for n, k in enumerate(cols)}


def geometric_class(qh, qw, H, W, pads):
    pt, pb, pl, pr = pads
    return np.where(qh < pt, 1, np.where(qh >= pt + H, 2, np.where(
        qw < pl, 3, np.where(qw >= pl + W, 4, 0))))


def expected_dst(b, qh, qw, B, H, W, pads):
    pt, pb, pl, pr = pads
    HP, WP = H + pt + pb, W + pl + pr
    out = []
    for bb, h, w in zip(b, qh, qw):
        if pt <= h < pt + H and pl <= w < pl + W:
            out.append((bb * H + h - pt) * W + w - pl)
        else:
            out.append(B * H * W + bb * (HP * WP - H * W) +
                       ring_index(h, w, HP, WP, pt, pl, H, W))
    return np.array(out)


@pytest.mark.parametrize("sid,B,H,W,pads,KH,KW", MAP_SHAPES,
                         ids=[s[0] for s in MAP_SHAPES])
def test_rowmap(sid, B, H, W, pads, KH, KW):
    pt, pb, pl, pr = pads
    HP, WP = H + pt + pb, W + pl + pr
    t = rowmap(B, H, W, pads, KH, KW)
    ok = t["ok"] == 1
    assert set(np.unique(t["ok"])) <= {0, 1}
    v = {k: a[ok] for k, a in t.items()}

    # valid rows <-> padded-frame pixels, one to one; every row's slot in
    # the [dx | ring] allocation is ring_index's, so the slots are a
    # permutation of the allocation: nothing outside it, nothing twice
    pix = (v["b"] * HP + v["qh"]) * WP + v["qw"]
    assert (v["b"] >= 0).all() and (v["b"] < B).all()
    assert (v["qh"] >= 0).all() and (v["qh"] < HP).all()
    assert (v["qw"] >= 0).all() and (v["qw"] < WP).all()
    assert np.array_equal(np.sort(pix), np.arange(B * HP * WP))
    assert np.array_equal(
        v["dst"], expected_dst(v["b"], v["qh"], v["qw"], B, H, W, pads))
    assert np.array_equal(np.sort(v["dst"]), np.arange(B * HP * WP))

    # window rows first, in (b, i, j) order; the rest of the last window
    # tile is invalid and no ring row
    Mw = B * H * W
    wrows = -(-Mw // BM) * BM
    m = np.arange(Mw)
    assert ok[:Mw].all() and not ok[Mw:wrows].any()
    assert (t["cls"][:wrows] == 0).all() and (t["cls"][wrows:] >= 1).all()
    assert np.array_equal(t["b"][:Mw], m // (H * W))
    assert np.array_equal(t["qh"][:Mw] - pt, m // W % H)
    assert np.array_equal(t["qw"][:Mw] - pl, m % W)

    # a tile holds one class and one tap window; a valid row's class is its
    # pixel's; classes come in order, each in (b, qh, qw) order, padded at
    # its end only
    for k in ("cls", "kh0", "kh1", "kw0", "kw1"):
        per_tile = t[k].reshape(-1, BM)
        assert (per_tile == per_tile[:, :1]).all(), k
    assert np.array_equal(
        v["cls"], geometric_class(v["qh"], v["qw"], H, W, pads))
    assert (np.diff(t["cls"]) >= 0).all()
    counts = {1: B * pt * WP, 2: B * pb * WP, 3: B * H * pl, 4: B * H * pr}
    for c, n in counts.items():
        sel = t["cls"] == c
        assert sel.sum() == -(-n // BM) * BM      # empty class: no tile
        assert ok[sel][:n].all() and not ok[sel][n:].any()
        key = pix[v["cls"] == c]
        assert (np.diff(key) > 0).all()

    # taps: window rows run all of them; for a ring row a tap whose source
    # (oh, ow) = (qh - kh, qw - kw) lies inside dy is inside the tile's
    # window (so every tap outside the window has its source out of range)
    full = ((t["kh0"] == 0) & (t["kh1"] == KH) & (t["kw0"] == 0) &
            (t["kw1"] == KW))
    assert full[t["cls"] == 0].all()
    SH, SW = HP - KH + 1, WP - KW + 1
    ring = v["cls"] >= 1
    for kh in range(KH):
        for kw in range(KW):
            oh, ow = v["qh"] - kh, v["qw"] - kw
            src_in = (oh >= 0) & (oh < SH) & (ow >= 0) & (ow < SW)
            tap_in = ((v["kh0"] <= kh) & (kh < v["kh1"]) &
                      (v["kw0"] <= kw) & (kw < v["kw1"]))
            assert not (ring & src_in & ~tap_in).any(), (kh, kw)
    # ... and the windows are the derived rectangles, not merely safe ones
    want = {1: (0, min(pt, KH), 0, KW), 2: (max(0, KH - pb), KH, 0, KW),
            3: (0, KH, 0, min(pl, KW)), 4: (0, KH, max(0, KW - pr), KW)}
    for c, win in want.items():
        sel = t["cls"] == c
        got = np.stack([t[k][sel] for k in ("kh0", "kh1", "kw0", "kw1")], 1)
        assert (got == np.array(win)).all(), c
        if sel.any():
            assert win[0] < win[1] and win[2] < win[3]


ORDER_SHAPES = MAP_SHAPES[:3] + MAP_SHAPES[-2:]


@pytest.mark.parametrize("sid,B,H,W,pads,KH,KW", ORDER_SHAPES,
                         ids=[s[0] for s in ORDER_SHAPES])
def test_rowmap_untrimmed_and_frame_order(sid, B, H, W, pads, KH, KW):
    """trim off (the gather's Cin % 64 != 0): same rows, every tap.
    frame on (CYG_DGRAD_FRAME_ORDER=1): the padded frame row by row."""
    pt, pb, pl, pr = pads
    HP, WP = H + pt + pb, W + pl + pr
    a = rowmap(B, H, W, pads, KH, KW)
    u = rowmap(B, H, W, pads, KH, KW, trim=False)
    for k in ("ok", "b", "qh", "qw", "cls", "dst"):
        assert np.array_equal(a[k], u[k]), k
    f = rowmap(B, H, W, pads, KH, KW, frame=True)
    M = B * HP * WP
    m = np.arange(M)
    assert len(f["ok"]) == -(-M // BM) * BM
    assert f["ok"][:M].all() and not f["ok"][M:].any()
    assert np.array_equal(f["b"][:M], m // (HP * WP))
    assert np.array_equal(f["qh"][:M], m // WP % HP)
    assert np.array_equal(f["qw"][:M], m % WP)
    assert np.array_equal(
        f["dst"][:M], expected_dst(f["b"][:M], f["qh"][:M], f["qw"][:M],
                                   B, H, W, pads))
    for t in (u, f):
        assert (t["kh0"] == 0).all() and (t["kh1"] == KH).all()
        assert (t["kw0"] == 0).all() and (t["kw1"] == KW).all()
    assert (f["cls"] == 0).all()
