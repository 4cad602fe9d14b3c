"""Fused Adam + weight EMA measurements (results: profiles/README.md).

    python tools/adam_micro.py kernel
        The optimizer update of one generator (n = 11,383,427 fp32
        parameters) three ways: adam_step_dev alone (28 B/param),
        adam_ema_step_dev (the fused kernel, 36 B/param) and adam_step_dev
        followed by a separate torch EMA pass (ema.mul_(d).add_(p, 1-d):
        two kernels, 48 B/param in all; a one-kernel pass would make it
        40). Two figures per case, both from
        device events around many launches: issued one by one from the
        host (what an eager step pays) and replayed from a hip graph of 200
        launches (what the captured step pays: no host launch gap). The
        cases are timed in turn, --rounds times over, and the median round
        is reported.

    python tools/adam_micro.py step --ema_decay D [--steps K] [--warmup W]
        ms/step of the captured train step in bench.py's configuration
        (batch 4, 256x256, bf16, 9 residual blocks, synthetic inputs) with
        the generator average at decay D; D=0 is bench.py's own loop.
        Compare settings by alternating runs of this command.

Each mode prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from cyclegan_amd.ops import backend  # noqa: E402

DEV = torch.device("cuda", 0)
N_GENERATOR = 11_383_427
B1, B2, EPS, DECAY = 0.5, 0.9, 1e-7, 0.999


def kernel(args):
    ext = backend.ext()
    n = args.n
    g = torch.Generator().manual_seed(0)
    p = (torch.randn(n, generator=g) * 0.05).to(DEV)
    grad = (torch.randn(n, generator=g) * 0.02).to(DEV)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    ema = p.clone()
    lr_t = torch.full((1,), 2e-4, device=DEV)

    def plain():
        ext.adam_step_dev(p, grad, m, v, lr_t, B1, B2, EPS)

    def fused():
        ext.adam_ema_step_dev(p, grad, m, v, ema, lr_t, B1, B2, EPS, DECAY)

    def separate():
        ext.adam_step_dev(p, grad, m, v, lr_t, B1, B2, EPS)
        ema.mul_(DECAY).add_(p, alpha=1 - DECAY)

    # bytes the op needs per parameter: p, m, v read and written, g read;
    # the average read and written; the separate pass reads p again and,
    # as two torch kernels, reads and writes the average twice
    cases = {"adam": (plain, 28), "adam_ema_fused": (fused, 36),
             "adam_then_ema_pass": (separate, 48)}
    ev0, ev1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    graphs = {}
    for name, (fn, _) in cases.items():
        for _ in range(10):  # warm-up
            fn()
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(200):
                fn()
        graphs[name].replay()
    torch.cuda.synchronize()

    eager = {k: [] for k in cases}
    graph = {k: [] for k in cases}
    for _ in range(args.rounds):
        for name, (fn, _) in cases.items():
            ev0.record()
            for _ in range(args.launches):
                fn()
            ev1.record()
            torch.cuda.synchronize()
            eager[name].append(ev0.elapsed_time(ev1) * 1e3 / args.launches)
            ev0.record()
            for _ in range(args.replays):
                graphs[name].replay()
            ev1.record()
            torch.cuda.synchronize()
            graph[name].append(ev0.elapsed_time(ev1) * 1e3
                               / (200 * args.replays))
    res = {"n": n, "ema_decay": DECAY, "rounds": args.rounds}
    for name, (_, bpp) in cases.items():
        e, gr = statistics.median(eager[name]), statistics.median(graph[name])
        res[name] = {"eager_us": round(e, 2), "graph_us": round(gr, 2),
                     "graph_us_min_max": [round(min(graph[name]), 2),
                                          round(max(graph[name]), 2)],
                     "bytes": bpp * n,
                     "graph_GBps": round(bpp * n / gr * 1e-3, 1)}
    a, f, s = (res[k]["graph_us"] for k in cases)
    res["fused_over_adam"] = round(f / a, 3)
    res["fused_over_separate"] = round(f / s, 3)
    print(json.dumps(res))


def step(args):
    from cyclegan_amd.parallel import DistContext
    from cyclegan_amd.trainer import CycleGAN, GraphedStep
    a = argparse.Namespace(
        output_dir="/tmp/cyclegan_adam_micro", batch_size=4,
        global_batch_size=4, num_residual_blocks=9,
        compute_dtype=torch.bfloat16, ema_decay=args.ema_decay, seed=1234)
    ctx = DistContext()
    torch.manual_seed(1234)
    gan = CycleGAN(a, ctx)
    g = torch.Generator(device="cpu").manual_seed(4321)
    data = []
    for _ in range(4):
        x = torch.rand(4, 256, 256, 3, generator=g) * 2 - 1
        y = torch.rand(4, 256, 256, 3, generator=g) * 2 - 1
        data.append((x.to(DEV, torch.bfloat16), y.to(DEV, torch.bfloat16)))
    for i in range(args.warmup):
        gan.train_step(*data[i % 4])
    graphed = GraphedStep(gan, *data[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        graphed(*data[i % 4])
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    print(json.dumps({"ema_decay": args.ema_decay, "steps": args.steps,
                      "warmup": args.warmup,
                      "ms_per_step": round(elapsed / args.steps * 1e3, 3)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--n", type=int, default=N_GENERATOR)
    k.add_argument("--launches", type=int, default=500)
    k.add_argument("--replays", type=int, default=5)
    k.add_argument("--rounds", type=int, default=5)
    s = sub.add_parser("step")
    s.add_argument("--ema_decay", type=float, default=0.999)
    s.add_argument("--steps", type=int, default=100)
    s.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    {"kernel": kernel, "step": step}[args.mode](args)
