"""bf16 shadow-weight cache.

Master parameters live in fp32 (optimizer numerics, exact DP all-reduce);
compute on MI355X runs in bf16 on the MFMA matrix cores. Instead of
recasting per call (the generator is invoked 3x per train step,
/root/reference/main.py:207-262), each master tensor gets a cached bf16
copy invalidated by the tensor's in-place version counter — the fused Adam
step bumps ``_version``, so shadows refresh exactly once per optimizer step.
"""

from __future__ import annotations

import torch
from torch.utils.weak import WeakTensorKeyDictionary

_cache: "WeakTensorKeyDictionary" = WeakTensorKeyDictionary()
_cache_t: "WeakTensorKeyDictionary" = WeakTensorKeyDictionary()
_cache_p: "WeakTensorKeyDictionary" = WeakTensorKeyDictionary()
_cache_tp: "WeakTensorKeyDictionary" = WeakTensorKeyDictionary()
_cache_f8: "WeakTensorKeyDictionary" = WeakTensorKeyDictionary()

# arena-backed forms (ops.arena): master param -> {form: bf16 view}.
# Views stay fresh because the trainer refreshes the arena after every
# parameter mutation (optimizer step / checkpoint load / broadcast).
_arena_forms: "WeakTensorKeyDictionary" = WeakTensorKeyDictionary()


def register_arena(arena):
    for p, forms in arena._by_param.items():
        _arena_forms[p] = forms


def _arena(p: torch.Tensor, form: str, like: torch.Tensor):
    if like.dtype != torch.bfloat16:
        return None
    forms = _arena_forms.get(p)
    return None if forms is None else forms.get(form)


def bf16_shadow(t: torch.Tensor) -> torch.Tensor:
    """Return a cached bf16 copy of ``t`` (refreshed when t changes in-place)."""
    if t.dtype == torch.bfloat16:
        return t
    ent = _cache.get(t)
    ver = t._version
    if ent is not None and ent[0] == ver:
        return ent[1]
    s = t.detach().to(torch.bfloat16)
    _cache[t] = (ver, s)
    return s


def compute_weight(w: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """Weight in the compute dtype of activation ``like`` (no autograd edge)."""
    v = _arena(w, "plain", like)
    if v is not None:
        return v
    if like.dtype == torch.bfloat16 and w.dtype != torch.bfloat16:
        return bf16_shadow(w)
    if w.dtype != like.dtype:
        return w.detach().to(like.dtype)
    return w.detach()


def compute_bias_p(b: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """Bias padded to >= 8 channels in the compute dtype."""
    v = _arena(b, "bias_p", like)
    if v is not None:
        return v
    bc = compute_weight(b, like)
    if bc.numel() < 8:
        bc = torch.nn.functional.pad(bc, (0, 8 - bc.numel()))
    return bc


def _pad_dims(w: torch.Tensor) -> torch.Tensor:
    """Zero-pad OHWI weight dims O and I up to 8 (glds kernel alignment).
    Padded input channels see zero activations and padded output channels
    are sliced away, so the math is unchanged."""
    cout, kh, kw, cin = w.shape
    po = max(0, 8 - cout)
    pi = max(0, 8 - cin)
    if po == 0 and pi == 0:
        return w
    return torch.nn.functional.pad(w, (0, pi, 0, 0, 0, 0, 0, po))


def compute_weight_p(w: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """Padded (dims >= 8) compute-dtype weight, cached per master version."""
    v = _arena(w, "p", like)
    if v is not None:
        return v
    ent = _cache_p.get(w)
    ver = w._version
    key = (ver, like.dtype, "p")
    if ent is not None and ent[0] == key:
        return ent[1]
    wp = _pad_dims(w.detach())
    if like.dtype == torch.bfloat16 and wp.dtype != torch.bfloat16:
        wp = wp.to(torch.bfloat16)
    elif wp.dtype != like.dtype:
        wp = wp.to(like.dtype)
    wp = wp.contiguous()
    _cache_p[w] = (key, wp)
    return wp


def compute_weight_tp(w: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """Padded channel-transposed weight ([I,kh,kw,O], dims >= 8)."""
    v = _arena(w, "tp", like)
    if v is not None:
        return v
    ent = _cache_tp.get(w)
    ver = w._version
    key = (ver, like.dtype, "tp")
    if ent is not None and ent[0] == key:
        return ent[1]
    wt = _pad_dims(w.detach()).permute(3, 1, 2, 0).contiguous()
    if like.dtype == torch.bfloat16 and wt.dtype != torch.bfloat16:
        wt = wt.to(torch.bfloat16)
    elif wt.dtype != like.dtype:
        wt = wt.to(like.dtype)
    _cache_tp[w] = (key, wt)
    return wt


def compute_weight_t(w: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """Channel-transposed weight (OHWI [O,kh,kw,I] -> [I,kh,kw,O]) in the
    compute dtype — the B^T operand of the adjoint (dgrad) kernels. Cached
    per master-version like the bf16 shadow (the backward of each of the
    generator's 3 calls per step reuses it)."""
    v = _arena(w, "t", like)
    if v is not None:
        return v
    ent = _cache_t.get(w)
    ver = w._version
    if ent is not None and ent[0] == ver and ent[1] == like.dtype:
        return ent[2]
    wt = w.detach().permute(3, 1, 2, 0).contiguous()
    if like.dtype == torch.bfloat16 and wt.dtype != torch.bfloat16:
        wt = wt.to(torch.bfloat16)
    elif wt.dtype != like.dtype:
        wt = wt.to(like.dtype)
    _cache_t[w] = (ver, like.dtype, wt)
    return wt


def _pack_head_weight_torch(w: torch.Tensor) -> torch.Tensor:
    """Packed head form [64, KH, 2, 8*I] (see arena._idx_packp) built in
    torch — fallback for masters without an arena (tests)."""
    O, KH, KW, I = w.shape
    out = w.new_zeros(8, 8, KH, 2, 8, I)
    for d in range(8):
        for blk in range(2):
            for pos in range(8):
                tx = blk * 8 + pos - d
                if 0 <= tx < KW:
                    out[d, :O, :, blk, pos, :] = w[:, :, tx, :]
    return out.reshape(64, KH, 2, 8 * I)


_cache_packp: "WeakTensorKeyDictionary" = WeakTensorKeyDictionary()
_cache_packb: "WeakTensorKeyDictionary" = WeakTensorKeyDictionary()


def compute_weight_packp(w: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    v = _arena(w, "packp", like)
    if v is not None:
        return v
    ent = _cache_packp.get(w)
    ver = w._version
    if ent is not None and ent[0] == ver:
        return ent[1]
    wp = _pack_head_weight_torch(w.detach()).to(like.dtype).contiguous()
    _cache_packp[w] = (ver, wp)
    return wp


def compute_bias_packb(b: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    v = _arena(b, "packb", like)
    if v is not None:
        return v
    ent = _cache_packb.get(b)
    ver = b._version
    if ent is not None and ent[0] == ver:
        return ent[1]
    n = b.numel()
    bp = torch.nn.functional.pad(b.detach(), (0, 8 - n)) if n < 8 else b.detach()
    bp = bp.repeat(8).to(like.dtype).contiguous()
    _cache_packb[b] = (ver, bp)
    return bp


def _fold_up_weight_torch(w: torch.Tensor) -> torch.Tensor:
    """Resize-convolution fold V = M w M^T of a 3x3 OHWI master, [O,4,4,I]
    in fp32 (docs/KERNELS.md) — the einsum 'kd,odei,le->okli' with M,
    written as its at most four terms per tap added in fp32 in the arena's
    order (d-major), so that it is the same number bit for bit."""
    from .arena import FOLD_M
    O, KH, KW, I = w.shape
    assert KH == 3 and KW == 3, "upsample_conv2d: 3x3 kernels only"
    wf = w.float()
    v = wf.new_zeros(O, 4, 4, I)
    for k in range(4):
        for l in range(4):
            for d in range(3):
                for e in range(3):
                    if FOLD_M[k][d] and FOLD_M[l][e]:
                        v[:, k, l, :] += wf[:, d, e, :]
    return v


_cache_up: "WeakTensorKeyDictionary" = WeakTensorKeyDictionary()


def _folded(w: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """(up, up_t) built in torch, cached per master version — fallback for
    masters without an arena (tests, ops called directly)."""
    ent = _cache_up.get(w)
    key = (w._version, like.dtype)
    if ent is not None and ent[0] == key:
        return ent[1]
    up = _fold_up_weight_torch(w.detach()).to(like.dtype).contiguous()
    forms = (up, up.permute(3, 1, 2, 0).contiguous())
    _cache_up[w] = (key, forms)
    return forms


def compute_weight_up(w: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """Folded 4x4 transpose-conv form [O,4,4,I] of a 3x3 master."""
    v = _arena(w, "up", like)
    return v if v is not None else _folded(w, like)[0]


def compute_weight_up_t(w: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """Its channel transpose [I,4,4,O], convt2d_dgrad's operand."""
    v = _arena(w, "up_t", like)
    return v if v is not None else _folded(w, like)[1]


def fp8_weight_shadow(w: torch.Tensor):
    """(wq uint8 e4m3 padded OHWI, sw fp32 scale tensor), cached per master
    version. scale = 448/amax (OCP e4m3 max normal)."""
    from . import backend
    ent = _cache_f8.get(w)
    ver = w._version
    if ent is not None and ent[0] == ver:
        return ent[1], ent[2]
    wp = _pad_dims(w.detach()).contiguous()
    amax = wp.abs().amax().float().clamp(min=1e-12)
    sw = (448.0 / amax).clamp(max=65504.0)
    wq = backend.ext().quant_fp8(wp.to(torch.bfloat16).contiguous(), sw)
    _cache_f8[w] = (ver, wq, sw)
    return wq, sw
