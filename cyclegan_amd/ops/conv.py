"""NHWC convolution ops (implicit-GEMM MFMA kernels on GPU).

Layouts (MI355X-first):
- activations: ``[B, H, W, C]`` contiguous (channels innermost → coalesced
  bf16x8 loads, C is the GEMM K/N dimension for the matrix cores).
- weights: OHWI ``[Cout, kh, kw, Cin]`` contiguous — the transposed
  implicit-GEMM B operand ``B^T[N = Cout][K = kh*kw*Cin]`` row-major, so
  weight staging is a coalesced row copy AND the per-lane MFMA B-fragment
  (8 contiguous k at one n) is a single ds_read_b128. No transpose
  anywhere on the forward path.
- conv_transpose weights: OHWI ``[Cout, kh, kw, Cin]`` with Cin = source
  channels (our own convention; checkpoints are native to this framework).

Padding follows the TF 'SAME'/'VALID' conventions of the reference
(pad_before = total//2 — /root/reference/main.py uses Keras Conv2D 'same');
pads are explicit ``(pt, pb, pl, pr)`` everywhere. ``pad_mode='reflect'``
implements ReflectionPadding2D folded into the conv
(/root/reference/cyclegan/model.py:14-33).

Activation epilogues (none/relu/lrelu/tanh) are fused into the conv kernel
— on 8 TB/s HBM the win is not re-reading the output tensor.

Autograd: the Function receives the fp32 master weight; bf16 compute copies
come from ops.shadow. Weight grads are produced in fp32 (split-K
accumulation) and flow straight into the fp32 master's grad bucket.
"""

from __future__ import annotations

import os
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

from . import backend, grad_sink
from .shadow import (compute_weight, compute_weight_t, compute_weight_p,
                     compute_weight_tp, compute_bias_p, compute_weight_packp,
                     compute_bias_packb, compute_weight_up,
                     compute_weight_up_t, fp8_weight_shadow)

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3

_ACT = {None: ACT_NONE, "none": ACT_NONE, "relu": ACT_RELU, "lrelu": ACT_LRELU, "tanh": ACT_TANH}


def same_pads(in_h: int, in_w: int, kh: int, kw: int, stride: int) -> Tuple[int, int, int, int]:
    """TF 'SAME' pads (pad_before = total//2, extra goes after)."""
    out_h = -(-in_h // stride)
    out_w = -(-in_w // stride)
    ph = max(0, (out_h - 1) * stride + kh - in_h)
    pw = max(0, (out_w - 1) * stride + kw - in_w)
    return ph // 2, ph - ph // 2, pw // 2, pw - pw // 2


def _apply_act(y: torch.Tensor, act: int, slope: float) -> torch.Tensor:
    if act == ACT_RELU:
        return torch.relu(y)
    if act == ACT_LRELU:
        return F.leaky_relu(y, slope)
    if act == ACT_TANH:
        return torch.tanh(y)
    return y


def act_bwd_from_output(dy: torch.Tensor, y: torch.Tensor, act: int, slope: float) -> torch.Tensor:
    """Backward of the fused activation, computed from the *output* y."""
    if act == ACT_RELU:
        return dy * (y > 0).to(dy.dtype)
    if act == ACT_LRELU:
        # slope > 0 keeps sign(pre-act) == sign(post-act)
        return torch.where(y > 0, dy, dy * slope)
    if act == ACT_TANH:
        return dy * (1 - y.float() * y.float()).to(dy.dtype)
    return dy


def _conv_ref(x, w, bias, stride, pads, pad_mode):
    """Differentiable torch reference (CPU path / GPU oracle); w is OHWI."""
    pt, pb, pl, pr = pads
    xn = x.permute(0, 3, 1, 2)
    if pt or pb or pl or pr:
        mode = "reflect" if pad_mode == "reflect" else "constant"
        xn = F.pad(xn, (pl, pr, pt, pb), mode=mode)
    wn = w.permute(0, 3, 1, 2)  # OHWI -> OIHW
    y = F.conv2d(xn.contiguous(), wn.contiguous(), bias, stride=stride)
    return y.permute(0, 2, 3, 1)


def _convt_ref(x, w, bias, stride, pt, pl, out_h, out_w):
    """Transpose conv = adjoint of the TF-'SAME' strided conv (gather form:
    out[i] += in[o]*w[k] where i = s*o + k - pt); w is OHWI."""
    xn = x.permute(0, 3, 1, 2)
    wn = w.permute(3, 0, 1, 2)  # OHWI -> (Cin, Cout, kh, kw)
    y = F.conv_transpose2d(xn.contiguous(), wn.contiguous(), bias, stride=stride)
    y = y[:, :, pt : pt + out_h, pl : pl + out_w]
    return y.permute(0, 2, 3, 1)


# Attribute under which a conv output carries the InstanceNorm partial
# slabs its epilogue produced: (psum, psq), each [NS, B, C] fp32,
# non-differentiable. ops.norm.instance_norm picks them up when the shapes
# match and then skips its own reduce pass. Only bias-free, activation-free
# bf16 HIP convs emit them (in these models: exactly the convs followed by
# IN), and only when the kernel library finds the shape eligible.
IN_SLABS_ATTR = "_cyg_in_slabs"


def _want_stats(bias, act) -> bool:
    return bias is None and act == ACT_NONE


def _attach_slabs(out):
    """Unpack a Function result that may carry slabs: (y, psum, psq) -> y
    with the slabs attached; a bare tensor passes through."""
    if isinstance(out, tuple):
        y, psum, psq = out
        setattr(y, IN_SLABS_ATTR, (psum, psq))
        return y
    return out


def _pad_channels(t: torch.Tensor, c_to: int = 8) -> torch.Tensor:
    """Zero-pad the channel (last) dim of an NHWC tensor up to c_to."""
    c = t.shape[-1]
    if c >= c_to:
        return t
    return F.pad(t, (0, c_to - c))


class _ConvFn(torch.autograd.Function):
    """HIP implicit-GEMM conv with fused pad + bias + activation.

    Channel dims < 8 (the RGB stem / 1-3 channel heads) are zero-padded to
    8 so every shape runs the fast glds kernels; padded input channels see
    zero activations (grads exactly zero) and padded output channels are
    sliced off."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pads, reflect, act, slope):
        ext = backend.ext()
        cout = w.shape[0]
        xp = _pad_channels(x).contiguous()
        wc = compute_weight_p(w, x)
        bc = compute_bias_p(bias, x) if bias is not None else None
        slabs = ()
        if _want_stats(bias, act) and cout >= 8:
            y, *slabs = ext.conv2d_fwd_stats(xp, wc, bc, stride, *pads,
                                             reflect, act, slope)
        else:
            y = ext.conv2d_fwd(xp, wc, bc, stride, *pads, reflect, act, slope)
        if cout < 8:
            y = y[..., :cout].contiguous()
        ctx.save_for_backward(xp, w, y, bias)
        ctx.conf = (stride, pads, reflect, act, slope, bias is not None,
                    x.shape[3])
        if slabs:
            # no zero-filled grads for the slab outputs in backward
            ctx.set_materialize_grads(False)
            ctx.mark_non_differentiable(*slabs)
            return (y, *slabs)
        return y

    @staticmethod
    def backward(ctx, dy, *_):
        if dy is None:  # only with set_materialize_grads(False): y unused
            return (None,) * 8
        xp, w, y, bias = ctx.saved_tensors
        stride, pads, reflect, act, slope, has_bias, cin = ctx.conf
        cout = w.shape[0]
        pt, pb, pl, pr = pads
        ext = backend.ext()
        sink = grad_sink.current()
        dy = dy.contiguous()
        if act != ACT_NONE:
            dy = ext.act_bwd(dy, y, act, slope)
        dyp = _pad_channels(dy).contiguous()
        db = None
        if has_bias and ctx.needs_input_grad[2]:
            db = _bias_grad(ext, sink, bias, dyp, dy.shape[-1])
        dx = dw = None
        if ctx.needs_input_grad[0]:
            wt = compute_weight_tp(w, xp)
            dx = ext.conv2d_dgrad(dyp, wt, xp.shape[1], xp.shape[2], stride,
                                  pt, pb, pl, pr, reflect)
            if cin < 8:
                dx = dx[..., :cin].contiguous()
        if ctx.needs_input_grad[1] and not grad_sink.frozen(sink, w):
            if sink is not None and sink.has(w):
                out, acc = sink.take(w)
                ext.conv2d_wgrad_into(xp, dyp, w.shape[1], w.shape[2], stride,
                                      pt, pl, reflect, out, acc, False)
            else:
                dw = ext.conv2d_wgrad(xp, dyp, w.shape[1], w.shape[2], stride,
                                      pt, pl, reflect)
                if cout < 8 or cin < 8:
                    dw = dw[:cout, :, :, :cin].contiguous()
        return dx, dw, db, None, None, None, None, None


def _bias_grad(ext, sink, bias, dyp, n):
    """Bias gradient (channel sum of the padded dy, first n channels): into
    the active sink's view, skipped for a frozen model's bias, returned to
    autograd when no sink is active."""
    if grad_sink.frozen(sink, bias):
        return None
    if sink is not None and sink.has(bias):
        out, acc = sink.take(bias)
        ext.channel_sum(dyp, out, acc)
        return None
    return ext.channel_sum(dyp)[:n]


def _head_packable(x, w, stride, pads, reflect) -> bool:
    """Generator-head geometry (7x7 s1 reflect-3, Cout <= 8, Cin % 8 == 0):
    runs as the 8-pixel-packed conv — 8 adjacent output pixels fold into
    the MFMA N dimension (Cout' = 64) so the matrix cores run dense
    instead of 8/16-wide, and the 49x input re-read of the skinny path
    collapses into a 7x2-block window over the channel-folded image."""
    import os
    if os.environ.get("CYG_NO_PACKHEAD") == "1":
        return False
    return (reflect and stride == 1 and pads == (3, 3, 3, 3)
            and w.shape[0] <= 8 and w.shape[1] == 7 and w.shape[2] == 7
            and w.shape[3] % 8 == 0 and w.shape[3] >= 8
            and x.shape[2] % 8 == 0 and x.shape[1] >= 7 and x.shape[2] >= 16)


def _fold_packed_dw(dwp: torch.Tensor, wshape) -> torch.Tensor:
    """[64, KH, 2, 8*I] packed wgrad -> OHWI [O, KH, KW, I]."""
    O, KH, KW, I = wshape
    d6 = dwp.view(8, 8, KH, 2, 8, I)                    # [d,co,ty,blk,pos,ci]
    d7 = d6.permute(0, 3, 4, 1, 2, 5).reshape(8, 16, 8, KH, I)  # [d,a,co,ty,ci]
    dev = dwp.device
    idx = (torch.arange(KW, device=dev).view(1, -1)
           + torch.arange(8, device=dev).view(-1, 1))   # a = tx + d
    idx = idx.view(8, KW, 1, 1, 1).expand(8, KW, 8, KH, I)
    dw = d7.gather(1, idx).sum(0)                       # [tx, co, ty, ci]
    return dw.permute(1, 2, 0, 3)[:O].contiguous()      # [co,ty,tx,ci]


class _ConvHeadPackedFn(torch.autograd.Function):
    """8-pixel-packed head conv (see _head_packable). Forward and wgrad
    run the packed dense-N GEMM; dgrad keeps the unpacked formulation
    (its packed form would do 2.4x the FLOPs on zero weights)."""

    @staticmethod
    def forward(ctx, x, w, bias, act, slope):
        ext = backend.ext()
        B, H, W, Cin = x.shape
        cout = w.shape[0]
        wpk = compute_weight_packp(w, x)
        bpk = compute_bias_packb(bias, x) if bias is not None else None
        xp = ext.reflect_pad_fwd(x.contiguous(), 3, 3, 3, 5)
        xf = xp.view(B, H + 6, (W + 8) // 8, 8 * Cin)
        yp = ext.conv2d_fwd(xf, wpk, bpk, 1, 0, 0, 0, 0, False, act, slope)
        y = yp.view(B, H, W, 8)
        if cout < 8:
            y = y[..., :cout].contiguous()
        ctx.save_for_backward(xp, w, y, bias)
        ctx.conf = (act, slope, bias is not None, cout, Cin, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        xp, w, y, bias = ctx.saved_tensors
        act, slope, has_bias, cout, Cin, H, W = ctx.conf
        ext = backend.ext()
        sink = grad_sink.current()
        dy = dy.contiguous()
        if act != ACT_NONE:
            dy = ext.act_bwd(dy, y, act, slope)
        dyp = _pad_channels(dy).contiguous()
        db = None
        if has_bias and ctx.needs_input_grad[2]:
            db = _bias_grad(ext, sink, bias, dyp, dy.shape[-1])
        dx = dw = None
        B = dyp.shape[0]
        if ctx.needs_input_grad[0]:
            wt = compute_weight_tp(w, xp)
            dx = ext.conv2d_dgrad(dyp, wt, H, W, 1, 3, 3, 3, 3, True)
        if ctx.needs_input_grad[1] and not grad_sink.frozen(sink, w):
            xf = xp.view(B, H + 6, (W + 8) // 8, 8 * Cin)
            dy_pk = dyp.view(B, H, W // 8, 64)
            dwp = ext.conv2d_wgrad(xf, dy_pk, 7, 2, 1, 0, 0, False)
            if sink is not None and sink.has(w):
                out, acc = sink.take(w)
                ext.fold_packed_dw_into(dwp, out, acc)
            else:
                dw = _fold_packed_dw(dwp, tuple(w.shape))
        return dx, dw, db, None, None


_FP8_MODE = False


def set_fp8_mode(on: bool):
    """Enable the CDNA4 fp8 (e4m3) forward-conv path (BASELINE config 5):
    per-tensor-scaled fp8 weights+activations on the fp8 MFMA, fp32
    accumulate, bf16 outputs; backward runs on the saved bf16 activations."""
    global _FP8_MODE
    _FP8_MODE = bool(on)


def fp8_mode() -> bool:
    return _FP8_MODE


# Attribute under which an InstanceNorm output carries the e4m3 twin the
# norm kernel wrote for the fp8 conv that consumes it: (yq, prev), yq uint8
# of the tensor's own NHWC shape, prev the amax_prev slot view (of
# ops.fp8_state) it was quantised with. Non-differentiable. The conv uses
# it instead of running quant_fp8_d, but only when prev is its own
# weight's slot (_twin_for).
FP8_TWIN_ATTR = "_cyg_fp8_twin"


class Fp8Consumer(NamedTuple):
    """Hint for ops.norm.instance_norm: the conv that reads its output."""
    weight: torch.Tensor   # the consumer's fp32 master weight (OHWI)
    stride: int = 1


def _knob_off(name: str) -> bool:
    """CYG_NO_FP8_TWIN / CYG_NO_FP8_STATS, read per call."""
    return os.environ.get(name) == "1"


def takes_fp8_path(x: torch.Tensor, w: torch.Tensor, stride: int,
                   pads=None, reflect: bool = False) -> bool:
    """Would conv2d(x, w, stride=...) run the fp8 kernel while fp8 mode is
    on? The ONE dispatch predicate: conv2d routes by it, and the producing
    norm decides by it whether to emit an fp8 twin for that conv.

    fp8 only where the 16x16x128 fp8 kernel + quant beats the bf16 glds
    kernel (tools/fp8_micro.py on MI355X): the wide-channel stride-1 3x3
    family at batch >= 12 (K3: 999 vs 715 TF/s) and the 4x4 s1 wide
    discriminator conv. Elsewhere the per-tensor quantization overhead
    cancels the MFMA-rate gain. The packed head comes first: skinny-Cout
    convs gain more from dense-N bf16 packing than from fp8's rate. It is
    7x7 only, so without pads (the norm's hint has none) the kernel-size
    test below already excludes it."""
    if x.dim() != 4 or w.dim() != 4 or x.dtype != torch.bfloat16:
        return False
    if pads is not None and _head_packable(x, w, stride, tuple(pads), reflect):
        return False
    return (w.shape[3] == x.shape[3]
            and w.shape[3] % 16 == 0 and w.shape[3] >= 256
            and stride == 1
            and ((w.shape[1] == 3 and x.shape[0] >= 12)
                 or w.shape[1] == 4))


def _twin_for(x: torch.Tensor, w: torch.Tensor):
    """The fp8 twin attached to x if it is this conv's operand: same shape
    and device as x, and quantised with THIS weight's amax_prev slot (the
    slot object itself, not just any slot). None -> quantise as usual."""
    if _knob_off("CYG_NO_FP8_TWIN"):
        return None
    tw = getattr(x, FP8_TWIN_ATTR, None)
    if tw is None:
        return None
    from . import fp8_state
    xq, tw_prev = tw
    ent = fp8_state.peek(w)
    if (ent is None or tw_prev is not ent[0] or xq.shape != x.shape
            or xq.device != x.device or xq.dtype != torch.uint8
            or x.shape[3] < 8 or not x.is_contiguous()
            or not xq.is_contiguous()):
        return None
    return xq


class _ConvFp8Fn(torch.autograd.Function):
    """fp8 e4m3 forward conv with delayed per-tensor activation scaling
    (ops.fp8_state): quantization uses last step's amax — no separate
    amax reduction in the hot path — and the dequant factor is computed
    inside the conv epilogue from the amax/sw scalars.

    ``twin`` (non-differentiable) is x already quantised with this layer's
    amax_prev by the kernel that produced x (see FP8_TWIN_ATTR); that
    kernel also maxed this step's amax into amax_cur, so quant_fp8_d is
    skipped. Bias-free, activation-free calls also return the
    InstanceNorm slabs of y when the shape is eligible, like _ConvFn."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pads, reflect, act, slope,
                twin=None):
        from . import fp8_state
        ext = backend.ext()
        cout = w.shape[0]
        xp = _pad_channels(x).contiguous()
        wq, sw = fp8_weight_shadow(w)
        prev, cur, fresh = fp8_state.slots_for(w)
        if fresh:  # bootstrap (eager, once per layer, pre-capture)
            prev.copy_(xp.detach().abs().amax().float().clamp(min=1e-12))
            twin = None  # cannot have been made with this (new) slot
        xq = twin if twin is not None else ext.quant_fp8_d(xp, prev, cur)
        bc = compute_bias_p(bias, x) if bias is not None else None
        slabs = ()
        if (_want_stats(bias, act) and cout >= 8
                and not _knob_off("CYG_NO_FP8_STATS")):
            y, *slabs = ext.conv2d_fp8_fwd_stats(xq, wq, prev, sw, bc, stride,
                                                 *pads, reflect, act, slope)
        else:
            y = ext.conv2d_fp8_fwd(xq, wq, prev, sw, bc, stride, *pads,
                                   reflect, act, slope)
        if cout < 8:
            y = y[..., :cout].contiguous()
        ctx.save_for_backward(xp, w, y, bias)
        ctx.conf = (stride, pads, reflect, act, slope, bias is not None,
                    x.shape[3])
        if slabs:
            # no zero-filled grads for the slab outputs in backward
            ctx.set_materialize_grads(False)
            ctx.mark_non_differentiable(*slabs)
            return (y, *slabs)
        return y

    @staticmethod
    def backward(ctx, dy, *_):
        # bf16 backward of _ConvFn on the saved bf16 activations; the twin
        # input has no gradient
        return _ConvFn.backward(ctx, dy) + (None,)


class _ConvTFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, pt, pl, out_h, out_w, act, slope):
        ext = backend.ext()
        wc = compute_weight(w, x)
        bc = compute_weight(bias, x) if bias is not None else None
        slabs = ()
        if _want_stats(bias, act):
            y, *slabs = ext.convt2d_fwd_stats(x, wc, bc, stride, pt, pl,
                                              out_h, out_w, act, slope)
        else:
            y = ext.convt2d_fwd(x, wc, bc, stride, pt, pl, out_h, out_w, act,
                                slope)
        ctx.save_for_backward(x, w, y)
        ctx.conf = (stride, pt, pl, act, slope, bias is not None)
        if slabs:
            # no zero-filled grads for the slab outputs in backward
            ctx.set_materialize_grads(False)
            ctx.mark_non_differentiable(*slabs)
            return (y, *slabs)
        return y

    @staticmethod
    def backward(ctx, dy, *_):
        if dy is None:  # only with set_materialize_grads(False): y unused
            return (None,) * 10
        x, w, y = ctx.saved_tensors
        stride, pt, pl, act, slope, has_bias = ctx.conf
        ext = backend.ext()
        sink = grad_sink.current()
        dy = dy.contiguous()
        if act != ACT_NONE:
            dy = ext.act_bwd(dy, y, act, slope)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            # adjoint of the gather is the forward strided conv of dy
            wt = compute_weight_t(w, x)
            dx = ext.convt2d_dgrad(dy, wt, x.shape[1], x.shape[2], stride, pt, pl)
        if ctx.needs_input_grad[1] and not grad_sink.frozen(sink, w):
            # convT wgrad == conv wgrad with roles swapped (x := dy, dy := x),
            # then a channel transpose back to OHWI (done by the reduce's
            # store when it writes into the sink)
            if sink is not None and sink.has(w):
                out, acc = sink.take(w)
                ext.conv2d_wgrad_into(dy, x, w.shape[1], w.shape[2], stride,
                                      pt, pl, False, out, acc, True)
            else:
                dwc = ext.conv2d_wgrad(dy, x, w.shape[1], w.shape[2], stride,
                                       pt, pl, False)
                dw = dwc.permute(3, 1, 2, 0).contiguous()
        if has_bias and ctx.needs_input_grad[2]:
            db = dy.float().sum(dim=(0, 1, 2))
        return dx, dw, db, None, None, None, None, None, None, None


class _UpConvFn(torch.autograd.Function):
    """Resize-convolution (nearest-2x upsample + zero-padded 3x3 conv) as
    the 4x4 stride-2 'SAME' transpose conv with the folded kernel
    V = M w M^T (ops.shadow.compute_weight_up): _ConvTFn with K = 4,
    pt = pl = 1, whose 4x4 weight gradient is folded back onto the 3x3
    master by fold_upconv_dw_into. The upsampled tensor never exists."""

    @staticmethod
    def forward(ctx, x, w, bias, act, slope):
        ext = backend.ext()
        x = x.contiguous()
        out_h, out_w = 2 * x.shape[1], 2 * x.shape[2]
        wc = compute_weight_up(w, x)
        bc = compute_weight(bias, x) if bias is not None else None
        slabs = ()
        if _want_stats(bias, act):
            y, *slabs = ext.convt2d_fwd_stats(x, wc, bc, 2, 1, 1, out_h,
                                              out_w, act, slope)
        else:
            y = ext.convt2d_fwd(x, wc, bc, 2, 1, 1, out_h, out_w, act, slope)
        ctx.save_for_backward(x, w, y)
        ctx.conf = (act, slope, bias is not None)
        if slabs:
            # no zero-filled grads for the slab outputs in backward
            ctx.set_materialize_grads(False)
            ctx.mark_non_differentiable(*slabs)
            return (y, *slabs)
        return y

    @staticmethod
    def backward(ctx, dy, *_):
        if dy is None:  # only with set_materialize_grads(False): y unused
            return (None,) * 5
        x, w, y = ctx.saved_tensors
        act, slope, has_bias = ctx.conf
        ext = backend.ext()
        sink = grad_sink.current()
        dy = dy.contiguous()
        if act != ACT_NONE:
            dy = ext.act_bwd(dy, y, act, slope)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            wt = compute_weight_up_t(w, x)
            dx = ext.convt2d_dgrad(dy, wt, x.shape[1], x.shape[2], 2, 1, 1)
        if ctx.needs_input_grad[1] and not grad_sink.frozen(sink, w):
            # dV by the role-swapped wgrad, [Cin,4,4,Cout]; the fold
            # transposes it back while it sums the taps
            dv = ext.conv2d_wgrad(dy, x, 4, 4, 2, 1, 1, False)
            if sink is not None and sink.has(w):
                out, acc = sink.take(w)
                ext.fold_upconv_dw_into(dv, out, acc, True)
            else:
                dw = torch.empty(w.shape, dtype=torch.float32,
                                 device=dv.device)
                ext.fold_upconv_dw_into(dv, dw, False, True)
        if has_bias and ctx.needs_input_grad[2]:
            db = dy.float().sum(dim=(0, 1, 2))
        return dx, dw, db, None, None


def conv2d(
    x: torch.Tensor,
    w: torch.Tensor,
    bias: Optional[torch.Tensor] = None,
    stride: int = 1,
    padding: str | Tuple[int, int, int, int] = "valid",
    pad_mode: str = "zeros",
    act: Optional[str] = None,
    slope: float = 0.2,
) -> torch.Tensor:
    """NHWC conv2d. ``padding`` is 'valid', 'same' (TF semantics) or explicit
    (pt, pb, pl, pr). ``pad_mode`` 'zeros'|'reflect'. ``act`` fused epilogue."""
    kh, kw = w.shape[1], w.shape[2]
    if padding == "valid":
        pads = (0, 0, 0, 0)
    elif padding == "same":
        pads = same_pads(x.shape[1], x.shape[2], kh, kw, stride)
    else:
        pads = tuple(padding)
    a = _ACT[act]
    if backend.use_hip(x, w):
        # packed head first: skinny-Cout convs gain more from dense-N
        # bf16 packing than from fp8's rate (and skip fp8's quant cost)
        if _head_packable(x, w, stride, pads, pad_mode == "reflect"):
            return _ConvHeadPackedFn.apply(x, w, bias, a, slope)
        if _FP8_MODE and takes_fp8_path(x, w, stride):
            return _attach_slabs(_ConvFp8Fn.apply(
                x, w, bias, stride, pads, pad_mode == "reflect", a, slope,
                _twin_for(x, w)))
        return _attach_slabs(_ConvFn.apply(x, w, bias, stride, pads,
                                           pad_mode == "reflect", a, slope))
    wc = w if w.dtype == x.dtype else w.to(x.dtype)
    bc = bias if (bias is None or bias.dtype == x.dtype) else bias.to(x.dtype)
    y = _conv_ref(x, wc, bc, stride, pads, pad_mode)
    return _apply_act(y, a, slope)


def conv_transpose2d(
    x: torch.Tensor,
    w: torch.Tensor,
    bias: Optional[torch.Tensor] = None,
    stride: int = 2,
    act: Optional[str] = None,
    slope: float = 0.2,
) -> torch.Tensor:
    """NHWC transpose conv with TF-'SAME' semantics: out = in*stride.

    Defined as the adjoint of conv2d(..., stride, 'same') mapping
    (in*stride) -> in, i.e. out[i] += in[o] * w[k] with i = s*o + k - pt.
    """
    kh, kw = w.shape[1], w.shape[2]
    out_h, out_w = x.shape[1] * stride, x.shape[2] * stride
    pt, _, pl, _ = same_pads(out_h, out_w, kh, kw, stride)
    a = _ACT[act]
    if backend.use_hip(x, w):
        return _attach_slabs(_ConvTFn.apply(x, w, bias, stride, pt, pl, out_h,
                                            out_w, a, slope))
    wc = w if w.dtype == x.dtype else w.to(x.dtype)
    bc = bias if (bias is None or bias.dtype == x.dtype) else bias.to(x.dtype)
    y = _convt_ref(x, wc, bc, stride, pt, pl, out_h, out_w)
    return _apply_act(y, a, slope)


def upsample_conv2d(
    x: torch.Tensor,
    w: torch.Tensor,
    bias: Optional[torch.Tensor] = None,
    act: Optional[str] = None,
    slope: float = 0.2,
) -> torch.Tensor:
    """Resize-convolution: nearest-neighbour 2x upsampling followed by a
    zero-padded ('SAME') 3x3 stride-1 conv, [B,H,W,Cin] -> [B,2H,2W,Cout];
    ``w`` is the OHWI 3x3 master.

    On the HIP path this runs as the equivalent 4x4 stride-2 transpose
    conv with the folded kernel (_UpConvFn). The torch path is the naive
    formulation, and the oracle of the other.
    """
    assert w.shape[1] == 3 and w.shape[2] == 3, \
        "upsample_conv2d: 3x3 kernels only"
    a = _ACT[act]
    if backend.use_hip(x, w) and x.dtype == torch.bfloat16:
        return _attach_slabs(_UpConvFn.apply(x, w, bias, a, slope))
    wc = w if w.dtype == x.dtype else w.to(x.dtype)
    bc = bias if (bias is None or bias.dtype == x.dtype) else bias.to(x.dtype)
    xu = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    y = _conv_ref(xu.permute(0, 2, 3, 1), wc, bc, 1, (1, 1, 1, 1), "zeros")
    return _apply_act(y, a, slope)
