"""CycleGAN training CLI — same contract as the reference
(/root/reference/main.py:405-413: --output_dir --epochs --batch_size
--verbose --clear_output_dir; --batch_size is PER-REPLICA, global batch =
world_size * batch_size).

Single GPU / CPU:    python main.py --output_dir runs
Multi-GPU (DP/RCCL): python -m torch.distributed.run --nnodes=1
                     --nproc-per-node 8 --master-addr 127.0.0.1 main.py ...

Extra flags cover the BASELINE.json configs only (synthetic data source,
image size, resblock count, dtype) and the input path: --data_device gpu
keeps the dataset on the device as uint8 and builds every batch with one
augmentation kernel (data/device.py); --augment epoch re-draws the
augmentation each epoch (device path only). --pool_size N updates the
discriminators on a history of N generated images (the CycleGAN paper's
image pool, N = 50 there; ops/pool.py). --lr_decay_epochs N decays the
learning rate linearly towards zero over the last N epochs (the paper:
N = epochs/2), stepping once per epoch; a resumed run picks the schedule
up at the epoch the optimizer's step count implies. --ema_decay D keeps an
exponential moving average of the generator weights inside the fused Adam
kernel; the test epoch, the cycle plots and ``translate.py --ema`` then use
the averaged generators. --upsample resize builds both generators with
resize-convolution upsampling blocks (nearest-2x + conv3x3, run as one
folded 4x4 transpose conv) instead of the reference's transpose convs; the
checkpoint records it: resuming with the other setting is refused, and
``translate.py`` builds the matching generator from the checkpoint alone.
--cycle_ssim W (0..1) mixes a structural-similarity term into the cycle
loss, per sample (1-W)·MAE + W·(1-SSIM) with the SSIM of
``tf.image.ssim(max_val=2)`` (ops/ssim.py); --test_ssim adds the SSIM of
the two cycles to the test epoch's metrics (implied by --cycle_ssim > 0).
Neither changes the checkpoint.
"""

from __future__ import annotations

import argparse
import os
from shutil import rmtree
from time import time

import numpy as np
import torch
from tqdm import tqdm

from cyclegan_amd.parallel import DistContext
from cyclegan_amd.trainer import CycleGAN, lr_factor
from cyclegan_amd.data import Pipeline, DevicePipeline, DevicePrefetcher
from cyclegan_amd import utils


def train(args, pipe, gan, summary, epoch: int):
    results = {}
    # steady-state step as ONE hip graph at N=1 (same path bench.py
    # measures); short final batches and multi-rank training run eager
    use_graph = (gan.device.type == "cuda" and gan.ctx.world_size == 1
                 and not os.environ.get("CYG_NO_GRAPH"))
    if args.data_device == "gpu":
        # batches are born on the device in the compute dtype; once the
        # graph exists they are written straight into its static inputs
        static = ((gan.graphed.sx, gan.graphed.sy)
                  if gan.graphed is not None else None)
        it = pipe.train_epoch(epoch, out=static)
    else:
        it = DevicePrefetcher(pipe.train_epoch(epoch), gan.device,
                              gan.compute_dtype)
    if use_graph and gan.pool_size:
        # the captured step cannot draw: plan the epoch's pool decisions
        # now, one device table, and let every step take its row
        gb, n = pipe.global_batch, pipe.num_train
        sizes = [min(gb, n - s * gb) for s in range(pipe.train_steps)]
        gan.plan_pools(sizes, (pipe.image_size, pipe.image_size, 3))
    for x, y in tqdm(it, desc="Train", total=pipe.train_steps,
                     disable=args.verbose == 0 or not gan.ctx.is_main):
        if use_graph and x.shape[0] == args.batch_size:
            if gan.graphed is None:
                from cyclegan_amd.trainer import GraphedStep
                gan.graphed = GraphedStep(gan, x, y, preserve_state=True)
            if x is gan.graphed.sx:  # already written in place: no copy
                result = gan.graphed.call_cloned(None, None)
            else:
                result = gan.graphed.call_cloned(x, y)
        else:
            result = gan.train_step(x, y)
        utils.append_dict(results, result)
    reduced = gan.reduce_results(results)
    if summary is not None:
        for key, value in reduced.items():
            summary.scalar(key, value, step=epoch, training=True)


def test(args, pipe, gan, summary, epoch: int):
    results = {}
    it = pipe.test_epoch()
    if args.data_device != "gpu":
        it = DevicePrefetcher(it, gan.device, gan.compute_dtype)
    with gan.ema_weights():  # the averaged generators, when kept
        for x, y in tqdm(it, desc="Test", total=pipe.test_steps,
                         disable=args.verbose == 0 or not gan.ctx.is_main):
            result = gan.test_step(x, y)
            utils.append_dict(results, result)
    reduced = gan.reduce_results(results)
    if summary is not None:
        for key, value in reduced.items():
            summary.scalar(key, value, step=epoch, training=False)
    return reduced


def main(args):
    ctx = DistContext()
    if ctx.is_main:
        if args.clear_output_dir and os.path.exists(args.output_dir):
            rmtree(args.output_dir)
        os.makedirs(args.output_dir, exist_ok=True)
    ctx.barrier()

    # reference seeds np/tf with 1234 (main.py:366-367); --seed overrides
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)

    args.global_batch_size = ctx.world_size * args.batch_size
    if args.dtype:
        args.compute_dtype = {"fp32": torch.float32, "bf16": torch.bfloat16,
                              "fp8": torch.bfloat16}[args.dtype]
        args.fp8 = args.dtype == "fp8"
    else:
        args.compute_dtype = None
    print(f"Number of devices: {ctx.world_size}")

    summary = utils.Summary(args.output_dir) if ctx.is_main else None

    if args.data_device == "gpu":
        pipe = DevicePipeline(args, ctx, image_size=args.image_size,
                              augment=args.augment)
    else:
        pipe = Pipeline(args, ctx, image_size=args.image_size)
    args.train_steps, args.test_steps = pipe.train_steps, pipe.test_steps

    gan = CycleGAN(args, ctx)
    gan.load_checkpoint()

    # a schedule that restarted on resume would be wrong: with the decay
    # on, go on at the epoch the restored optimizer step count implies
    first_epoch = 0
    if args.lr_decay_epochs > 0:
        first_epoch = gan.optimizers["G"].t // pipe.train_steps

    for epoch in range(first_epoch, args.epochs):
        if ctx.is_main:
            print(f"Epoch {epoch + 1:03d}/{args.epochs:03d}")
        if args.lr_decay_epochs > 0:
            scale = lr_factor(epoch, args.epochs, args.lr_decay_epochs)
            gan.set_lr_scale(scale)
            if summary is not None:
                summary.scalar("learning_rate",
                               gan.optimizers["G"].lr * scale, step=epoch,
                               training=True)

        start = time()
        train(args, pipe, gan, summary, epoch)
        results = test(args, pipe, gan, summary, epoch)
        end = time()
        if summary is not None:
            summary.scalar("elapse", end - start, step=epoch)
            if args.verbose == 2:
                # extension: RCCL all-reduce GPU-time per epoch (hip events
                # around each flat-grad all-reduce, parallel/dp.py)
                summary.scalar("comm/all_reduce_ms", gan.sync.pop_comm_ms(),
                               step=epoch)

        if ctx.is_main and results:
            # (the reference console print swaps two labels, main.py:394-397
            #  — corrected here; TB values are identical)
            print(f'MAE(X, F(G(X))): {results["error/MAE(X, F(G(X)))"]:.04f}\t\t'
                  f'MAE(Y, G(F(Y))): {results["error/MAE(Y, G(F(Y)))"]:.04f}\n'
                  f'MAE(X, F(X)): {results["error/MAE(X, F(X))"]:.04f}\t\t'
                  f'MAE(Y, G(Y)): {results["error/MAE(Y, G(Y))"]:.04f}\n'
                  + (f'SSIM(X, F(G(X))): '
                     f'{results["error/SSIM(X, F(G(X)))"]:.04f}\t\t'
                     f'SSIM(Y, G(F(Y))): '
                     f'{results["error/SSIM(Y, G(F(Y)))"]:.04f}\n'
                     if gan.test_ssim else '')
                  + f'Elapse: {end - start:.02f}s\n')

        if epoch % 10 == 0 or epoch == args.epochs - 1:
            gan.save_checkpoint()
            if ctx.is_main:
                with gan.ema_weights():
                    utils.plot_cycle(pipe.plot_pairs(), gan, summary, epoch)
            ctx.barrier()

    if summary is not None:
        summary.close()
    return gan


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    parser.add_argument("--output_dir", default="runs")
    parser.add_argument("--epochs", default=200, type=int)
    parser.add_argument("--batch_size", default=1, type=int,
                        help="per-replica batch size")
    parser.add_argument("--verbose", default=1, type=int, choices=[0, 1, 2])
    parser.add_argument("--clear_output_dir", action="store_true")
    # MI355X/BASELINE extras
    parser.add_argument("--data_dir", default=None,
                        help="trainA/trainB/testA/testB image folders; "
                             "default: synthetic horse2zebra-shaped data")
    parser.add_argument("--image_size", default=256, type=int)
    parser.add_argument("--num_residual_blocks", default=9, type=int)
    parser.add_argument("--dtype", default=None, choices=[None, "fp32", "bf16", "fp8"])
    parser.add_argument("--num_train_samples", default=None, type=int)
    parser.add_argument("--num_test_samples", default=None, type=int)
    parser.add_argument("--seed", default=1234, type=int)
    parser.add_argument("--data_device", default="host", choices=["host", "gpu"],
                        help="host: batches built on the host and copied; "
                             "gpu: uint8 dataset resident on the device, "
                             "batches built by the augmentation kernel")
    parser.add_argument("--pool_size", default=0, type=int,
                        help="image history pool: update the discriminators "
                             "on a buffer of the last N generated images "
                             "(the CycleGAN paper uses 50); 0: off")
    parser.add_argument("--lr_decay_epochs", default=0, type=int,
                        help="decay the learning rate linearly towards zero "
                             "over the last N epochs (the CycleGAN paper: "
                             "half the run); 0: constant")
    parser.add_argument("--ema_decay", default=0.0, type=float,
                        help="keep an exponential moving average of the "
                             "generator weights with this decay (e.g. 0.999) "
                             "and evaluate with it; 0: off")
    parser.add_argument("--upsample", default="transpose",
                        choices=["transpose", "resize"],
                        help="generator upsampling blocks. transpose: the "
                             "reference's stride-2 3x3 transpose conv; "
                             "resize: nearest-2x upsampling + 3x3 conv "
                             "(no checkerboard artifacts; not in the "
                             "reference). Recorded in the checkpoint")
    parser.add_argument("--cycle_ssim", default=0.0, type=float,
                        help="weight W in [0, 1] of a structural-similarity "
                             "term in the cycle loss: per sample "
                             "(1-W)*MAE + W*(1-SSIM); 0: the reference's "
                             "pure L1 (not in the reference)")
    parser.add_argument("--test_ssim", action="store_true",
                        help="also report the SSIM of both cycles in the "
                             "test epoch (implied by --cycle_ssim > 0)")
    parser.add_argument("--augment", default="frozen", choices=["frozen", "epoch"],
                        help="frozen: one augmentation per sample for the run "
                             "(the reference's .map().cache()); epoch: re-drawn "
                             "every epoch (needs --data_device gpu)")
    return parser


def parse_args(argv=None) -> argparse.Namespace:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.augment == "epoch" and args.data_device != "gpu":
        parser.error("--augment epoch requires --data_device gpu")
    if args.pool_size < 0:
        parser.error("--pool_size must be >= 0")
    if not 0 <= args.lr_decay_epochs <= args.epochs:
        parser.error("--lr_decay_epochs must be in [0, --epochs]")
    if not 0.0 <= args.ema_decay < 1.0:
        parser.error("--ema_decay must be in [0, 1)")
    if not 0.0 <= args.cycle_ssim <= 1.0:
        parser.error("--cycle_ssim must be in [0, 1]")
    if args.cycle_ssim > 0.0:
        args.test_ssim = True
    return args


if __name__ == "__main__":
    main(parse_args())
