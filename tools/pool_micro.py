"""Image history pool measurements (results: profiles/README.md).

    python tools/pool_micro.py kernel
        pool_exchange alone at the workload shape ([4,256,256,3] bf16,
        P=50) for all-pass, all-swap and all-fill codes. Two figures per
        case, both from device events around many launches: issued one by
        one from the host (what an eager step pays) and replayed from a
        hip graph of 200 launches (what the captured step pays: no host
        launch gap). The slots rotate through the whole pool, so swap and
        fill touch all 50 images, not one cached slot.

    python tools/pool_micro.py step --pool_size N [--steps K] [--warmup W]
        ms/step of the captured train step in bench.py's configuration
        (batch 4, 256x256, bf16, 9 residual blocks, synthetic inputs) with
        the pool at size N; N=0 is bench.py's own loop. The decisions of
        all timed steps are planned beforehand, as main.py does per epoch.
        Compare sizes by alternating runs of this command.

Each mode prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from cyclegan_amd.ops.pool import make_codes, pool_exchange  # noqa: E402

DEV = torch.device("cuda", 0)


def kernel(args):
    B, P, image = 4, 50, (256, 256, 3)
    g = torch.Generator().manual_seed(0)
    pool = (torch.rand(P, *image, generator=g) * 2 - 1).to(DEV, torch.bfloat16)
    fake = (torch.rand(B, *image, generator=g) * 2 - 1).to(DEV, torch.bfloat16)
    out = torch.empty_like(fake)
    n_rows = 25  # 25 rows x 4 slots walk the 50-slot pool twice
    slots = [[(r * B + b) % P for b in range(B)] for r in range(n_rows)]
    tables = {
        "pass": make_codes([[-1] * B] * n_rows, P, DEV),
        "swap": make_codes(slots, P, DEV),
        "fill": make_codes([[P + s for s in row] for row in slots], P, DEV),
    }
    image_bytes = fake[0].numel() * 2
    # bytes the op needs per element: pass/fill read fake and write two or
    # one copies of it; swap also reads the slot
    need = {"pass": 2, "fill": 3, "swap": 4}
    res = {"shape": [B, *image], "P": P, "dtype": "bf16"}
    ev0, ev1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    for name, table in tables.items():
        def launches(n):
            for i in range(n):
                pool_exchange(pool, fake, table[i % n_rows], out=out)
        launches(50)  # warm-up
        torch.cuda.synchronize()
        ev0.record()
        launches(args.launches)
        ev1.record()
        torch.cuda.synchronize()
        eager_us = ev0.elapsed_time(ev1) * 1e3 / args.launches

        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            launches(200)
        graph.replay()
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(args.replays):
            graph.replay()
        ev1.record()
        torch.cuda.synchronize()
        graph_us = ev0.elapsed_time(ev1) * 1e3 / (200 * args.replays)
        moved = need[name] * B * image_bytes
        res[name] = {"eager_us": round(eager_us, 2),
                     "graph_us": round(graph_us, 2),
                     "bytes": moved,
                     "graph_GBps": round(moved / graph_us * 1e-3, 1)}
    print(json.dumps(res))


def step(args):
    from cyclegan_amd.parallel import DistContext
    from cyclegan_amd.trainer import CycleGAN, GraphedStep
    a = argparse.Namespace(
        output_dir="/tmp/cyclegan_pool_micro", batch_size=4,
        global_batch_size=4, num_residual_blocks=9,
        compute_dtype=torch.bfloat16, pool_size=args.pool_size, seed=1234)
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
    if args.pool_size:
        gan.plan_pools([4] * args.steps, (256, 256, 3))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        graphed(*data[i % 4])
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    print(json.dumps({"pool_size": args.pool_size, "steps": args.steps,
                      "warmup": args.warmup,
                      "pool_count": [p.count for p in gan.pools or ()],
                      "ms_per_step": round(elapsed / args.steps * 1e3, 3)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--launches", type=int, default=2000)
    k.add_argument("--replays", type=int, default=20)
    s = sub.add_parser("step")
    s.add_argument("--pool_size", type=int, default=50)
    s.add_argument("--steps", type=int, default=100)
    s.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    {"kernel": kernel, "step": step}[args.mode](args)
