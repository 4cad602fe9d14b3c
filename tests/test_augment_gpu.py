"""The fused augmentation kernel (ops/_hip/augment.hip) against the host
pipeline's own functions.

Oracle: data.pipeline.apply_train_aug on CPU fp32 over random uint8 images
— random pixels make a wrong tap, a wrong offset or a missed flip an O(1)
error. Every element is compared.

Bounds (derived, not measured), S = max(Hs, Ws, rh, rw):
  fp32: |err| <= S * 2^-20 + 2^-22 — four fp32 roundings of a coordinate of
        magnitude <= S give d(lambda) <= S * 2^-22, and each axis
        contributes <= 2 * d(lambda) after the /127.5;
  bf16: the fp32 bound + 2^-9 (round-to-nearest at |v| <= 1).
"""

import argparse
import functools
import importlib.util
import itertools
import pathlib
import struct

import pytest
import torch

from cyclegan_amd.data import DevicePipeline, Pipeline
from cyclegan_amd.data.pipeline import apply_train_aug
from cyclegan_amd.ops.augment import augment_batch, make_idx, make_params

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def fp32_bound(src_hw, resize_hw):
    return max(*src_hw, *resize_hw) * 2.0 ** -20 + 2.0 ** -22


def bound(dtype, src_hw, resize_hw):
    b = fp32_bound(src_hw, resize_hw)
    return b + 2.0 ** -9 if dtype == torch.bfloat16 else b


# name -> (source [N,Hs,Ws,3], resize, crop, idx)
SHAPES = {
    # non-square, upscale, odd widths for the vector tail; idx repeats and
    # is not monotonic
    "upscale_odd": ((5, 13, 19, 3), (17, 23), (11, 21), [4, 0, 4, 2]),
    # downscale without antialias
    "downscale": ((3, 40, 33, 3), (18, 18), (16, 16), [0, 1, 2]),
    # identity: exact in fp32
    "identity": ((2, 5, 7, 3), (5, 7), (5, 7), [0, 1]),
    # the workload's own shape, B=4
    "workload": ((4, 256, 256, 3), (286, 286), (256, 256), [0, 1, 2, 3]),
}


@functools.lru_cache(maxsize=None)
def source(name):
    g = torch.Generator().manual_seed(sorted(SHAPES).index(name))
    return torch.randint(0, 256, SHAPES[name][0], generator=g,
                         dtype=torch.uint8)


@functools.lru_cache(maxsize=None)
def oracle(name, n, flip, oy, ox):
    """CPU fp32 reference of one sample; computed once, shared, never
    modified."""
    _, resize, crop, _ = SHAPES[name]
    return apply_train_aug(source(name)[n], flip, oy, ox, resize, crop)


def corners(resize, crop):
    return list(itertools.product((0, resize[0] - crop[0]),
                                  (0, resize[1] - crop[1])))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_vs_host_pipeline(name, dtype):
    shape, resize, crop, idx = SHAPES[name]
    src = source(name).to(DEV)
    idx_d = make_idx(idx, shape[0], DEV)
    tol = bound(dtype, shape[1:3], resize)
    # a set: corners coincide when resize == crop
    for flip, (oy, ox) in itertools.product(
            (0, 1), sorted(set(corners(resize, crop)))):
        params = make_params([[flip, oy, ox]] * shape[0], resize, crop, DEV)
        got = augment_batch(src, idx_d, params, resize, crop, dtype)
        assert got.shape == (len(idx), crop[0], crop[1], 3)
        assert got.dtype == dtype
        want = torch.stack([oracle(name, n, flip, oy, ox) for n in idx])
        err = (got.float().cpu() - want).abs().max().item()
        print(f"{name} {dtype} flip={flip} oy={oy} ox={ox}: "
              f"max err {err:.3e} (bound {tol:.3e})")
        assert err <= tol, (name, dtype, flip, oy, ox, err, tol)
        if name == "identity" and dtype == torch.float32:
            assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
def test_params_are_indexed_by_sample(dtype):
    """Each sample carries its own (flip, oy, ox); idx repeats and permutes,
    so params[b] in place of params[idx[b]] would be an O(1) error."""
    name = "upscale_odd"
    shape, resize, crop, idx = SHAPES[name]
    per_sample = [[0, 0, 0], [1, 6, 2], [0, 6, 0], [1, 0, 2], [1, 3, 1]]
    params = make_params(per_sample, resize, crop, DEV)
    got = augment_batch(source(name).to(DEV), make_idx(idx, shape[0], DEV),
                        params, resize, crop, dtype)
    want = torch.stack([oracle(name, n, *per_sample[n]) for n in idx])
    err = (got.float().cpu() - want).abs().max().item()
    assert err <= bound(dtype, shape[1:3], resize), err


@pytest.mark.parametrize("offset", [16, 3], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
def test_out_is_written_in_place(dtype, offset):
    """out= is a slice of a larger poisoned buffer: same storage, and not
    one element outside the slice is touched. Offset 3 takes the base off
    16-byte alignment (scalar-store path); 693 elements per image leave a
    partial vector group at the end either way."""
    name = "upscale_odd"
    shape, resize, crop, idx = SHAPES[name]
    numel = len(idx) * crop[0] * crop[1] * 3
    poison = 7.0
    buf = torch.full((offset + numel + 64,), poison, dtype=dtype, device=DEV)
    out = buf[offset:offset + numel].view(len(idx), crop[0], crop[1], 3)
    params = make_params([[1, 6, 2]] * shape[0], resize, crop, DEV)
    ret = augment_batch(source(name).to(DEV), make_idx(idx, shape[0], DEV),
                        params, resize, crop, dtype, out=out)
    assert ret.data_ptr() == out.data_ptr()
    assert ret.data_ptr() == buf.data_ptr() + offset * buf.element_size()
    host = buf.float().cpu()
    assert (host[:offset] == poison).all()
    assert (host[offset + numel:] == poison).all()
    want = torch.stack([oracle(name, n, 1, 6, 2) for n in idx])
    err = (host[offset:offset + numel].view_as(want) - want).abs().max().item()
    assert err <= bound(dtype, shape[1:3], resize), err


def test_empty_batch():
    name = "identity"
    shape, resize, crop, _ = SHAPES[name]
    params = make_params([[0, 0, 0]] * shape[0], resize, crop, DEV)
    got = augment_batch(source(name).to(DEV), make_idx([], shape[0], DEV),
                        params, resize, crop, torch.bfloat16)
    assert got.shape == (0, crop[0], crop[1], 3)
    assert got.dtype == torch.bfloat16 and got.is_cuda


def test_binding_refuses_bad_arguments():
    name = "identity"
    shape, resize, crop, idx = SHAPES[name]
    src = source(name).to(DEV)
    idx_d = make_idx(idx, shape[0], DEV)
    params = make_params([[0, 0, 0]] * shape[0], resize, crop, DEV)
    with pytest.raises(RuntimeError, match="smaller than crop"):
        # resize below crop: bypass the Python-side parameter check
        augment_batch(src, idx_d, params, (4, 7), crop, torch.float32)
    with pytest.raises(RuntimeError, match="idx must be"):
        augment_batch(src, idx_d.long(), params, resize, crop, torch.float32)
    with pytest.raises(RuntimeError, match="src must be"):
        augment_batch(src.float(), idx_d, params, resize, crop, torch.float32)
    with pytest.raises(RuntimeError, match="params must be"):
        augment_batch(src, idx_d, params[:1], resize, crop, torch.float32)


def make_args(gb=2, b=2, n_train=10, n_test=4):
    a = argparse.Namespace()
    a.global_batch_size = gb
    a.batch_size = b
    a.num_train_samples = n_train
    a.num_test_samples = n_test
    a.data_dir = None
    a.seed = 1234
    return a


def test_device_pipeline_matches_host_pipeline(local_ctx):
    args = make_args()
    p = Pipeline(args, local_ctx, image_size=64)
    d = DevicePipeline(args, local_ctx, image_size=64, device=DEV)
    assert d.dtype == torch.bfloat16
    tol = bound(torch.bfloat16, (64, 64), d.resize_hw)
    got, want = list(d.train_epoch(0)), list(p.train_epoch(0))
    assert len(got) == len(want) == 5
    for (gx, gy), (wx, wy) in zip(got, want):
        assert gx.is_cuda and gx.dtype == torch.bfloat16
        assert gx.shape == wx.shape and gy.shape == wy.shape
        assert (gx.float().cpu() - wx).abs().max().item() <= tol
        assert (gy.float().cpu() - wy).abs().max().item() <= tol
    tol_t = bound(torch.bfloat16, (64, 64), d.crop_hw)
    for (gx, gy), (wx, wy) in zip(d.test_epoch(), p.test_epoch()):
        assert (gx.float().cpu() - wx).abs().max().item() <= tol_t
        assert (gy.float().cpu() - wy).abs().max().item() <= tol_t


def _load_main():
    path = pathlib.Path(__file__).resolve().parent.parent / "main.py"
    spec = importlib.util.spec_from_file_location("cyclegan_main", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _train_scalars(path, tags):
    """tag -> [values] from an events file (utils/tb_writer.py framing: u64
    length, u32 crc, payload, u32 crc; a scalar value is the tag string
    field followed by float field 2)."""
    out = {t: [] for t in tags}
    data = open(path, "rb").read()
    pos = 0
    while pos + 12 <= len(data):
        (n,) = struct.unpack_from("<Q", data, pos)
        rec = data[pos + 12:pos + 12 + n]
        pos += 12 + n + 4
        for t in tags:
            key = b"\x0a" + bytes([len(t)]) + t.encode() + b"\x15"
            at = rec.find(key)
            if at >= 0:
                out[t].append(struct.unpack_from("<f", rec, at + len(key))[0])
    return out


def test_main_end_to_end_device_pipeline(tmp_path, local_ctx):
    """main.py on the device pipeline with per-epoch augmentation: epoch 0
    captures the graph, epoch 1 writes every batch straight into the
    graph's static inputs."""
    import glob
    import math
    import os
    main = _load_main()
    argv = ["--output_dir", str(tmp_path), "--data_device", "gpu",
            "--image_size", "64", "--num_residual_blocks", "2",
            "--num_train_samples", "8", "--num_test_samples", "4",
            "--batch_size", "2", "--epochs", "2", "--augment", "epoch",
            "--verbose", "0"]
    gan = main.main(main.parse_args(argv))
    torch.cuda.synchronize()
    assert gan.graphed is not None

    host = Pipeline(make_args(n_train=8), local_ctx, image_size=64)
    assert all(o.t == 2 * host.train_steps for o in gan.optimizers.values())

    files = glob.glob(os.path.join(str(tmp_path), "events.out.tfevents.*"))
    assert len(files) == 1
    scalars = _train_scalars(files[0], gan._TRAIN_KEYS)
    assert len(scalars) == 10
    for tag, vals in scalars.items():
        assert len(vals) == 2, (tag, vals)
        assert all(math.isfinite(v) for v in vals), (tag, vals)

    # the last full batch the pipeline produced sits in the graph's inputs
    ref = DevicePipeline(make_args(n_train=8), local_ctx, image_size=64,
                         augment="epoch")
    wx, wy = list(ref.train_epoch(1))[-1]
    tol = bound(torch.bfloat16, (64, 64), ref.resize_hw)
    assert gan.graphed.sx.dtype == torch.bfloat16
    assert (gan.graphed.sx.float().cpu() - wx).abs().max().item() <= tol
    assert (gan.graphed.sy.float().cpu() - wy).abs().max().item() <= tol
