"""Shadow arena: all bf16 compute-weight forms of a model group in a few
flat buffers, refreshed once per optimizer step.

Masters live in a group's flat fp32 buffer (parallel.flat.FlatParamGroup).
Every conv needs derived bf16 forms — padded OHWI for forward, padded
channel-transposed [I,kh,kw,O] for dgrad, padded bias — which round 1
rebuilt per master via ~180 per-step ATen pad/cast/permute launches
(profiles/kernel_stats_final.csv: ~9% of GPU time in Fill/copy kernels).
Here each form is a view into one bf16 arena filled by shadow_gather
(shadow.hip) from a precomputed int32 index map; -1 entries produce the
alignment-pad zeros. The refresh is captured inside the hip-graph step.

Resize-convolution layers (UpsampleConvNHWC) need forms that are SUMS of
masters — the 4x4 transpose-conv kernel folded from the 3x3 one. Those
live in a second segment (fold_buf) with an [n,4] index table, filled by
shadow_fold right after the gather; a model without such layers has an
empty segment and launches only the gather.

Most of the bytes need no index map. On the GPU (CYG_NO_ADAM_SHADOW=1
restores the full gather) the arena keeps a MIRROR, the bf16 image of the
whole flat buffer, which the fused Adam kernels write while p_new is in a
register (FusedAdam.shadow):

- a conv weight's OHWI form is a VIEW into the mirror when no dimension is
  padded and its flat offset is a multiple of 8 elements (the glds weight
  loads need 16-byte alignment);
- its channel-transposed form comes from shadow_transpose, one launch per
  group over a small per-layer table, when Cout and Cin are multiples of 8
  as well;
- everything else (padded stems and heads, the packed head form, biases,
  odd offsets) stays on the gather, whose index map shrinks to that
  remainder. The fold segment is as it was.

refresh() casts the mirror itself unless the caller says Adam has just
written it, so masters changed any other way give valid forms too.

GPU-only: CPU paths keep the version-keyed caches in ops.shadow (fp32
compute needs no casting there).
"""

from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import torch

from . import backend

_PAD = 8  # glds kernels need channel dims >= 8

# shadow.hip: columns of a transpose-table row, tile edge of its blocks
_ST_COLS = 8
_ST_T = 64


def mirror_enabled() -> bool:
    """CYG_NO_ADAM_SHADOW=1 turns the mirror off (every form from the full
    gather again); read when an arena is built."""
    return os.environ.get("CYG_NO_ADAM_SHADOW") != "1"


def mirror_view_ok(base: int, shape) -> bool:
    """The OHWI form may be a view into the mirror: nothing padded, 16-byte
    aligned."""
    O, _, _, I = shape
    return O >= _PAD and I >= _PAD and base % 8 == 0


def transpose_ok(base: int, shape) -> bool:
    """shadow_transpose can build the channel-transposed form: whole
    16-byte words on both sides."""
    O, _, _, I = shape
    return O % 8 == 0 and I % 8 == 0 and base % 8 == 0


def transpose_row(src: int, dst: int, shape, first_block: int) -> List[int]:
    """One table row of shadow_transpose, and the blocks it takes."""
    O, KH, KW, I = shape
    tci, tco = -(-I // _ST_T), -(-O // _ST_T)
    return [src, dst, O, KH * KW, I, first_block, tci, tco]


def _conv_like(m: torch.nn.Module) -> bool:
    return type(m).__name__ == "ConvNHWC"


def _convt_like(m: torch.nn.Module) -> bool:
    return type(m).__name__ == "ConvTransposeNHWC"


def _upconv_like(m: torch.nn.Module) -> bool:
    return type(m).__name__ == "UpsampleConvNHWC"


# Resize-convolution fold (docs/KERNELS.md): V = M w M^T on both axes; row
# k of M lists the 3x3 taps that 4x4 tap k sums.
FOLD_M = ((0, 0, 1), (0, 1, 1), (1, 1, 0), (1, 0, 0))
_FOLD_TAPS = tuple(tuple(d for d in range(3) if row[d]) for row in FOLD_M)


def _idx_up(base: int, shape) -> torch.Tensor:
    """Folded transpose-conv form [O,4,4,I] of a 3x3 master, as an index
    table [O,4,4,I,4]: V[o,k,l,i] sums w[o,d,e,i] over the taps d of row k
    and e of row l of FOLD_M, d-major, -1 where there are fewer than 4."""
    O, KH, KW, I = shape
    assert KH == 3 and KW == 3
    o = torch.arange(O).view(-1, 1)
    i = torch.arange(I).view(1, -1)
    idx = torch.full((O, 4, 4, I, 4), -1, dtype=torch.int64)
    for k in range(4):
        for l in range(4):
            terms = [(d, e) for d in _FOLD_TAPS[k] for e in _FOLD_TAPS[l]]
            for j, (d, e) in enumerate(terms):
                idx[:, k, l, :, j] = base + ((o * 3 + d) * 3 + e) * I + i
    return idx.to(torch.int32)


def _idx_up_t(base: int, shape) -> torch.Tensor:
    """Channel-transposed folded form [I,4,4,O] (convt2d_dgrad's weight)."""
    return _idx_up(base, shape).permute(3, 1, 2, 0, 4).contiguous()


def _idx_p(base: int, shape) -> torch.Tensor:
    """Padded OHWI forward form: [O',KH,KW,I'], O'=max(O,8), I'=max(I,8)."""
    O, KH, KW, I = shape
    Op, Ip = max(O, _PAD), max(I, _PAD)
    o = torch.arange(Op).view(-1, 1, 1, 1)
    kh = torch.arange(KH).view(1, -1, 1, 1)
    kw = torch.arange(KW).view(1, 1, -1, 1)
    i = torch.arange(Ip).view(1, 1, 1, -1)
    idx = base + ((o * KH + kh) * KW + kw) * I + i
    idx = torch.where((o < O) & (i < I), idx, torch.tensor(-1))
    return idx.to(torch.int32)


def _idx_tp(base: int, shape) -> torch.Tensor:
    """Padded channel-transposed dgrad form: [I',KH,KW,O']."""
    return _idx_p(base, shape).permute(3, 1, 2, 0).contiguous()


def _idx_plain(base: int, shape) -> torch.Tensor:
    O, KH, KW, I = shape
    return (base + torch.arange(O * KH * KW * I)).view(O, KH, KW, I).to(torch.int32)


def _idx_t(base: int, shape) -> torch.Tensor:
    return _idx_plain(base, shape).permute(3, 1, 2, 0).contiguous()


def _idx_bias(base: int, n: int) -> torch.Tensor:
    np_ = max(n, _PAD)
    idx = base + torch.arange(np_)
    idx[n:] = -1
    return idx.to(torch.int32)


def head_packable(shape, stride, pad_mode, padding) -> bool:
    """Generator-head geometry: 7x7 stride-1 reflect(3) conv with tiny
    Cout and Cin divisible by 8 — runs as the 8-pixel-packed conv (see
    ops.conv._ConvHeadPackedFn)."""
    O, KH, KW, I = shape
    return (O <= 8 and KH == 7 and KW == 7 and stride == 1 and I % 8 == 0
            and I >= 8 and pad_mode == "reflect"
            and tuple(padding) == (3, 3, 3, 3))


def _idx_packp(base: int, shape) -> torch.Tensor:
    """Packed head weight [8*8, KH, 2, 8*I]: n = d*8 + co packs 8 adjacent
    output pixels into channels; k covers a 2-block (16-col) window; slot
    (d, co, ty, blk, pos, ci) maps to w[co][ty][blk*8+pos-d][ci] when the
    tap is in range, else zero (idx -1)."""
    O, KH, KW, I = shape
    assert KW == 7
    d = torch.arange(8).view(-1, 1, 1, 1, 1, 1)
    co = torch.arange(8).view(1, -1, 1, 1, 1, 1)
    ty = torch.arange(KH).view(1, 1, -1, 1, 1, 1)
    blk = torch.arange(2).view(1, 1, 1, -1, 1, 1)
    pos = torch.arange(8).view(1, 1, 1, 1, -1, 1)
    ci = torch.arange(I).view(1, 1, 1, 1, 1, -1)
    tx = blk * 8 + pos - d
    idx = base + ((co * KH + ty) * KW + tx) * I + ci
    ok = (tx >= 0) & (tx < KW) & (co < O)
    idx = torch.where(ok, idx, torch.tensor(-1))
    return idx.reshape(64, KH, 2, 8 * I).to(torch.int32)


def _idx_packb(base: int, n: int) -> torch.Tensor:
    """Packed head bias [64]: b[d*8+co] = bias[co] (co < n), else 0."""
    co = torch.arange(8).repeat(8)
    idx = base + co
    idx[co >= n] = -1
    return idx.to(torch.int32)


class ShadowArena:
    """Builds and refreshes the arena for one FlatParamGroup + its module.

    mirror: None takes the default (on for a device group unless
    CYG_NO_ADAM_SHADOW=1); False is the full gather."""

    def __init__(self, group, module: torch.nn.Module,
                 mirror: Optional[bool] = None):
        self.group = group
        dev = group.flat_param.device
        if mirror is None:
            mirror = group.flat_param.is_cuda and mirror_enabled()
        off = {p: o for p, (o, _) in zip(group.params, group._offsets)}

        pieces: List[torch.Tensor] = []           # int32 index chunks (cpu)
        plan: List[Tuple[torch.nn.Parameter, str, Tuple[int, ...], int]] = []
        total = 0
        # second segment: folded forms (sums of up to 4 masters), [n,4]
        fpieces: List[torch.Tensor] = []
        fplan: List[Tuple[torch.nn.Parameter, str, Tuple[int, ...], int]] = []
        ftotal = 0
        # mirror views (start = flat offset) and transposed forms (start in
        # tbuf, one table row each)
        vplan: List[Tuple[torch.nn.Parameter, str, Tuple[int, ...], int]] = []
        tplan: List[Tuple[torch.nn.Parameter, str, Tuple[int, ...], int]] = []
        trows: List[List[int]] = []
        ttotal = tblocks = 0
        for m in module.modules():
            if _upconv_like(m):
                w = m.weight
                for name, fn in (("up", _idx_up), ("up_t", _idx_up_t)):
                    idx = fn(off[w], tuple(w.shape))
                    fpieces.append(idx.reshape(-1, 4))
                    fplan.append((w, name, tuple(idx.shape[:-1]), ftotal))
                    ftotal += idx.numel() // 4
                continue
            if _conv_like(m):
                forms = (("p", _idx_p), ("tp", _idx_tp))
            elif _convt_like(m):
                forms = (("plain", _idx_plain), ("t", _idx_t))
            else:
                continue
            w = m.weight
            forms = list(forms)
            packed = (_conv_like(m) and head_packable(
                tuple(w.shape), m.stride, m.pad_mode, m.padding
                if not isinstance(m.padding, str) else (0,) * 4))
            if packed:
                forms.append(("packp", _idx_packp))
            shape = tuple(w.shape)
            O, KH, KW, I = shape
            for name, fn in forms:
                if mirror and name in ("p", "plain") \
                        and mirror_view_ok(off[w], shape):
                    vplan.append((w, name, shape, off[w]))
                    continue
                if mirror and name in ("tp", "t") \
                        and transpose_ok(off[w], shape):
                    row = transpose_row(off[w], ttotal, shape, tblocks)
                    trows.append(row)
                    tplan.append((w, name, (I, KH, KW, O), ttotal))
                    ttotal += w.numel()
                    tblocks += row[3] * row[6] * row[7]
                    continue
                idx = fn(off[w], shape)
                pieces.append(idx.reshape(-1))
                plan.append((w, name, tuple(idx.shape), total))
                total += idx.numel()
            if m.bias is not None:
                idx = _idx_bias(off[m.bias], m.bias.numel())
                pieces.append(idx.reshape(-1))
                plan.append((m.bias, "bias_p", tuple(idx.shape), total))
                total += idx.numel()
                if packed:
                    idx = _idx_packb(off[m.bias], m.bias.numel())
                    pieces.append(idx.reshape(-1))
                    plan.append((m.bias, "packb", tuple(idx.shape), total))
                    total += idx.numel()

        pad = (-total) % 8
        if pad:
            pieces.append(torch.full((pad,), -1, dtype=torch.int32))
        self.idx = torch.cat(pieces).to(dev) if pieces else \
            torch.empty(0, dtype=torch.int32, device=dev)
        self.buf = torch.empty(self.idx.numel(), dtype=torch.bfloat16, device=dev)

        fpad = (-ftotal) % 8
        if fpad:
            fpieces.append(torch.full((fpad, 4), -1, dtype=torch.int32))
        self.fold_idx = torch.cat(fpieces).to(dev) if fpieces else \
            torch.empty((0, 4), dtype=torch.int32, device=dev)
        self.fold_buf = torch.empty(self.fold_idx.shape[0],
                                    dtype=torch.bfloat16, device=dev)

        # mirror (flat length rounded up to whole 16-byte words), the
        # transposed forms and their table, on the host and on the device
        self.mirror = None
        if mirror:
            n = group.flat_param.numel()
            self.mirror = torch.zeros(n + (-n) % 8, dtype=torch.bfloat16,
                                      device=dev)
        self.tbuf = torch.empty(ttotal, dtype=torch.bfloat16, device=dev)
        self.ttable = torch.tensor(trows, dtype=torch.int32).reshape(
            -1, _ST_COLS)
        self.ttable_dev = self.ttable.to(dev)

        # per-(master, form) shaped views into the arena, and where each
        # one comes from: "mirror", "transpose", "gather" or "fold"
        self.views: Dict[Tuple[int, str], torch.Tensor] = {}
        self._by_param: Dict[torch.Tensor, Dict[str, torch.Tensor]] = {}
        self.source: Dict[torch.Tensor, Dict[str, str]] = {}
        for kind, store, entries in (("gather", self.buf, plan),
                                     ("fold", self.fold_buf, fplan),
                                     ("mirror", self.mirror, vplan),
                                     ("transpose", self.tbuf, tplan)):
            for p, name, shape, start in entries:
                v = store[start:start + int(torch.tensor(shape).prod())]
                self._by_param.setdefault(p, {})[name] = v.view(shape)
                self.source.setdefault(p, {})[name] = kind

        self.refresh()

    def refresh(self, mirror_fresh: bool = False):
        """Masters -> every bf16 form. With the mirror: a cast pass fills
        it unless ``mirror_fresh`` (the Adam step on this stream has just
        written it), one transpose launch builds the dgrad forms from it,
        and the gather does the irregular remainder. Without: one gather
        for everything. One fold kernel more when the model has
        resize-convolution layers."""
        ext = backend.ext()
        if self.mirror is not None:
            if not mirror_fresh:
                ext.shadow_cast(self.group.flat_param, self.mirror)
            if self.ttable.shape[0]:
                ext.shadow_transpose(self.mirror, self.ttable,
                                     self.ttable_dev, self.tbuf)
        if self.idx.numel():
            ext.shadow_gather(self.group.flat_param, self.idx, self.buf)
        if self.fold_idx.numel():
            ext.shadow_fold(self.group.flat_param, self.fold_idx,
                            self.fold_buf)

    def forms_of(self, p: torch.Tensor):
        return self._by_param.get(p)
