"""Resize-convolution measurements (results: profiles/README.md).

    python tools/upconv_micro.py layer [--iters N] [--warmup W]
        forward and forward+backward of the generator's two upsampling
        layers (256->128 channels at 64x64, 128->64 at 128x128, B=4,
        bf16) in three forms: ``folded`` ops.upsample_conv2d (one 4x4
        stride-2 transpose conv with the folded kernel), ``transpose``
        ops.conv_transpose2d 3x3 (today's layer), and ``unfused``
        F.interpolate + ops.conv2d 3x3 (materialises the 4x larger
        activation). Device events around N calls issued from the host.

    python tools/upconv_micro.py step --upsample {transpose,resize}
                                      [--steps K] [--warmup W]
        ms/step of the captured train step in bench.py's configuration
        (batch 4, 256x256, bf16, 9 residual blocks, synthetic inputs).
        Compare the two settings by alternating runs of this command.

Each mode prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

# (Cin, Cout, H = W) of Generator.ups at 256x256 inputs
LAYER_SHAPES = ((256, 128, 64), (128, 64, 128))
BATCH = 4


def _forms():
    from cyclegan_amd import ops

    def unfused(x, w):
        xu = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2,
                           mode="nearest").permute(0, 2, 3, 1).contiguous()
        return ops.conv2d(xu, w, None, 1, (1, 1, 1, 1))

    return {"folded": ops.upsample_conv2d,
            "transpose": lambda x, w: ops.conv_transpose2d(x, w, stride=2),
            "unfused": unfused}


def _time(fn, iters, warmup):
    ev0, ev1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(iters):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) * 1e3 / iters


def layer(args):
    dev = torch.device("cuda", 0)
    res = {"batch": BATCH, "dtype": "bf16", "iters": args.iters, "layers": []}
    g = torch.Generator().manual_seed(0)
    for cin, cout, hw in LAYER_SHAPES:
        x = (torch.rand(BATCH, hw, hw, cin, generator=g) * 2 - 1).to(
            dev, torch.bfloat16).requires_grad_(True)
        w = (torch.randn(cout, 3, 3, cin, generator=g) * 0.02).to(
            dev).requires_grad_(True)
        dy = (torch.rand(BATCH, 2 * hw, 2 * hw, cout, generator=g) * 2
              - 1).to(dev, torch.bfloat16)
        row = {"cin": cin, "cout": cout, "hw": hw}
        for name, op in _forms().items():
            def fwd():
                with torch.no_grad():
                    op(x, w)

            def fwd_bwd():
                torch.autograd.grad(op(x, w), (x, w), dy)

            f_us = _time(fwd, args.iters, args.warmup)
            fb_us = _time(fwd_bwd, args.iters, args.warmup)
            row[name] = {"fwd_us": round(f_us, 1),
                         "fwd_bwd_us": round(fb_us, 1)}
        res["layers"].append(row)
    print(json.dumps(res))


def step(args):
    from cyclegan_amd.parallel import DistContext
    from cyclegan_amd.trainer import CycleGAN, GraphedStep
    dev = torch.device("cuda", 0)
    a = argparse.Namespace(
        output_dir="/tmp/cyclegan_upconv_micro", batch_size=BATCH,
        global_batch_size=BATCH, num_residual_blocks=9,
        compute_dtype=torch.bfloat16, upsample=args.upsample, seed=1234)
    ctx = DistContext()
    torch.manual_seed(1234)
    gan = CycleGAN(a, ctx)
    g = torch.Generator(device="cpu").manual_seed(4321)
    data = []
    for _ in range(4):
        x = torch.rand(BATCH, 256, 256, 3, generator=g) * 2 - 1
        y = torch.rand(BATCH, 256, 256, 3, generator=g) * 2 - 1
        data.append((x.to(dev, torch.bfloat16), y.to(dev, torch.bfloat16)))
    for i in range(args.warmup):
        gan.train_step(*data[i % 4])
    graphed = GraphedStep(gan, *data[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        out = graphed(*data[i % 4])
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    print(json.dumps({"upsample": args.upsample, "steps": args.steps,
                      "warmup": args.warmup,
                      "loss_G_total": round(float(out["loss_G/total"]), 4),
                      "ms_per_step": round(elapsed / args.steps * 1e3, 3)}))


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    la = sub.add_parser("layer")
    la.add_argument("--iters", type=int, default=1000)
    la.add_argument("--warmup", type=int, default=50)
    s = sub.add_parser("step")
    s.add_argument("--upsample", default="resize",
                   choices=["transpose", "resize"])
    s.add_argument("--steps", type=int, default=100)
    s.add_argument("--warmup", type=int, default=10)
    return ap


if __name__ == "__main__":
    args = build_parser().parse_args()
    {"layer": layer, "step": step}[args.mode](args)
