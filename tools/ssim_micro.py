"""SSIM kernel measurements (results: profiles/README.md).

    python tools/ssim_micro.py kernel [--iters N] [--warmup W] [--replays R]

Times, at the workload shape ([4,256,256,3] bf16), forward alone (under
no_grad: no coefficient maps) and forward + backward (gradient by y_pred,
as the trainer asks for it) of

    ssim        ops.SSIM, the HIP kernels
    mae         ops.MAE on the same tensors (the loss it joins)
    ssim_torch  ops.SSIM composed from torch ops (CYGAN_FORCE_TORCH=1:
                depthwise conv2d moments, autograd backward)

Two figures per case, both from device events around many calls after a
warm-up: issued one by one from the host (what an eager step pays) and,
for the HIP paths, replayed from a hip graph of 20 calls (what the captured
step pays: no host launch gap). Next to the times: the bytes each path has
to move and the bandwidth that amounts to.

    python tools/ssim_micro.py step --cycle_ssim W [--steps K] [--warmup W]

ms/step of the captured train step in bench.py's configuration (batch 4,
256x256, bf16, 9 residual blocks, synthetic inputs) with the SSIM term at
weight W; W = 0 is bench.py's own loop. Compare weights by alternating runs
of this command.

Each mode prints one JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

SHAPE = (4, 256, 256, 3)
GRAPH_CALLS = 20


def must_move(shape=SHAPE):
    """Bytes each case has to read and write, by name."""
    b, h, w, c = shape
    image = b * h * w * c * 2                      # one bf16 image batch
    maps = 3 * b * (h - 10) * (w - 10) * c * 4     # a, b, c in fp32
    return {
        # forward reads x and y; with a gradient it also writes the maps;
        # the backward reads x, y and the maps and writes one gradient
        "ssim_fwd": 2 * image,
        "ssim_fwd_bwd": (2 * image + maps) + (2 * image + maps + image),
        # MAE's backward reads both images and writes both gradients
        "mae_fwd": 2 * image,
        "mae_fwd_bwd": 2 * image + 4 * image,
    }


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--iters", type=int, default=500)
    k.add_argument("--warmup", type=int, default=50)
    k.add_argument("--replays", type=int, default=50)
    s = sub.add_parser("step")
    s.add_argument("--cycle_ssim", type=float, default=0.5)
    s.add_argument("--steps", type=int, default=100)
    s.add_argument("--warmup", type=int, default=10)
    return ap


def _time_calls(fn, iters, warmup):
    ev0, ev1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(iters):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) * 1e3 / iters  # us per call


def _time_graph(fn, replays):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(GRAPH_CALLS):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    ev0, ev1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    ev0.record()
    for _ in range(replays):
        graph.replay()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) * 1e3 / (GRAPH_CALLS * replays)


def kernel(args):
    from cyclegan_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(SHAPE, generator=g) * 2 - 1).to(dev, torch.bfloat16)
    y = (torch.rand(SHAPE, generator=g) * 2 - 1).to(dev, torch.bfloat16)
    yg = y.clone().requires_grad_(True)
    dout = torch.tensor([0.5, -2.0, 1.0, 0.25], device=dev)

    def fwd(op):
        def run():
            with torch.no_grad():
                return op(x, y)
        return run

    def fwd_bwd(op):
        def run():
            return torch.autograd.grad((op(x, yg) * dout).sum(), (yg,))
        return run

    need = must_move()
    res = {"shape": list(SHAPE), "dtype": "bf16", "iters": args.iters}
    for name, op, force_torch in (("ssim", ops.SSIM, False),
                                  ("mae", ops.MAE, False),
                                  ("ssim_torch", ops.SSIM, True)):
        if force_torch:
            os.environ["CYGAN_FORCE_TORCH"] = "1"
        try:
            for case, make in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                fn = make(op)
                row = {"eager_us": round(
                    _time_calls(fn, args.iters, args.warmup), 2)}
                if not force_torch:
                    row["graph_us"] = round(_time_graph(fn, args.replays), 2)
                    moved = need[f"{name}_{case}"]
                    row["bytes"] = moved
                    row["graph_GBps"] = round(
                        moved / row["graph_us"] * 1e-3, 1)
                res[f"{name}_{case}"] = row
        finally:
            os.environ.pop("CYGAN_FORCE_TORCH", None)
    for case in ("fwd", "fwd_bwd"):
        res[f"torch_over_hip_{case}"] = round(
            res[f"ssim_torch_{case}"]["eager_us"]
            / res[f"ssim_{case}"]["eager_us"], 2)
    print(json.dumps(res))


def step(args):
    import tempfile
    import time
    from cyclegan_amd.parallel import DistContext
    from cyclegan_amd.trainer import CycleGAN, GraphedStep
    dev = torch.device("cuda", 0)
    a = argparse.Namespace(
        output_dir=tempfile.mkdtemp(prefix="ssim_micro_"), batch_size=4,
        global_batch_size=4, num_residual_blocks=9,
        compute_dtype=torch.bfloat16, cycle_ssim=args.cycle_ssim)
    torch.manual_seed(1234)
    gan = CycleGAN(a, DistContext())
    g = torch.Generator(device="cpu").manual_seed(4321)
    data = []
    for _ in range(4):
        x = torch.rand(4, 256, 256, 3, generator=g) * 2 - 1
        y = torch.rand(4, 256, 256, 3, generator=g) * 2 - 1
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
    print(json.dumps({"cycle_ssim": args.cycle_ssim, "steps": args.steps,
                      "warmup": args.warmup,
                      "loss_G/cycle": round(out["loss_G/cycle"].item(), 4),
                      "ms_per_step": round(elapsed / args.steps * 1e3, 3)}))


if __name__ == "__main__":
    args = build_parser().parse_args()
    {"kernel": kernel, "step": step}[args.mode](args)
