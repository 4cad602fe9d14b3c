"""K15 input augmentation: flip-LR -> bilinear resize -> crop -> normalise
of uint8 images that live on the device (the reference's get_datasets map, its main.py:18-83), one HIP kernel per
batch (_hip/augment.hip).

    out[b] = apply_train_aug(src[idx[b]], *params[idx[b]], resize_hw, crop_hw)

``params[n] = (flip, oy, ox)`` is indexed by sample, not batch position.

The kernel trusts ``idx`` and ``params``: a bad value would be an
out-of-range read on the GPU. They are small host-built tensors, so their
range is checked on the host where they are created — ``make_idx`` /
``make_params`` validate and only then upload. Nothing is read back from
the device to check it.
"""

from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import backend


def check_idx(idx: torch.Tensor, n: int) -> None:
    """Host check: every sample index is in [0, n)."""
    assert idx.device.type == "cpu"
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
        raise ValueError(
            f"augment: sample index out of range [0, {n}): "
            f"min {int(idx.min())}, max {int(idx.max())}")


def check_params(params: torch.Tensor, resize_hw: Tuple[int, int],
                 crop_hw: Tuple[int, int]) -> None:
    """Host check: flip in {0,1}, 0 <= oy <= rh-ch, 0 <= ox <= rw-cw."""
    assert params.device.type == "cpu"
    (rh, rw), (ch, cw) = resize_hw, crop_hw
    if rh < ch or rw < cw:
        raise ValueError(f"augment: resize {resize_hw} smaller than crop {crop_hw}")
    if params.dim() != 2 or params.shape[1] != 3:
        raise ValueError(f"augment: params must be [N,3], got {tuple(params.shape)}")
    if not params.numel():
        return
    for col, name, hi in ((0, "flip", 1), (1, "oy", rh - ch), (2, "ox", rw - cw)):
        v = params[:, col]
        if int(v.min()) < 0 or int(v.max()) > hi:
            raise ValueError(
                f"augment: {name} out of range [0, {hi}]: "
                f"min {int(v.min())}, max {int(v.max())}")


def make_idx(values: Sequence[int], n: int, device) -> torch.Tensor:
    """int32 [B] sample indices: built on the host, validated, uploaded."""
    idx = torch.as_tensor(values, dtype=torch.int64).reshape(-1)
    check_idx(idx, n)
    return idx.to(torch.int32).to(device)


def make_params(values, resize_hw: Tuple[int, int], crop_hw: Tuple[int, int],
                device) -> torch.Tensor:
    """int32 [N,3] (flip, oy, ox) rows: built on the host, validated,
    uploaded."""
    params = torch.as_tensor(values, dtype=torch.int64).reshape(-1, 3)
    check_params(params, resize_hw, crop_hw)
    return params.to(torch.int32).to(device)


def _augment_torch(src, idx, params, resize_hw, crop_hw, dtype, out):
    # the host functions the Pipeline itself uses: bit-identical on CPU
    from ..data.pipeline import apply_train_aug
    idx_h, params_h, src_h = idx.cpu(), params.cpu(), src.cpu()
    check_idx(idx_h, src.shape[0])
    check_params(params_h, resize_hw, crop_hw)
    imgs = []
    for n in idx_h.tolist():
        flip, oy, ox = params_h[n].tolist()
        imgs.append(apply_train_aug(src_h[n], flip, oy, ox, resize_hw, crop_hw))
    if imgs:
        res = torch.stack(imgs).to(device=src.device, dtype=dtype)
    else:
        res = torch.empty(0, crop_hw[0], crop_hw[1], 3, dtype=dtype,
                          device=src.device)
    if out is None:
        return res
    out.copy_(res)
    return out


def augment_batch(src: torch.Tensor, idx: torch.Tensor, params: torch.Tensor,
                  resize_hw: Tuple[int, int], crop_hw: Tuple[int, int],
                  dtype: torch.dtype = torch.float32,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src u8 [N,Hs,Ws,3], idx i32 [B], params i32 [N,3] ->
    [B,ch,cw,3] of ``dtype`` (bf16 | fp32), written into ``out`` if given."""
    shape = (idx.shape[0], crop_hw[0], crop_hw[1], 3)
    if out is not None and (tuple(out.shape) != shape or out.dtype != dtype):
        raise ValueError(f"augment: out is {tuple(out.shape)} {out.dtype}, "
                         f"expected {shape} {dtype}")
    if not backend.use_hip(src):
        return _augment_torch(src, idx, params, resize_hw, crop_hw, dtype, out)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=src.device)
    return backend.ext().augment_batch(src, idx, params, resize_hw[0],
                                       resize_hw[1], out)
