"""CycleGAN trainer.

Replicates the reference trainer semantics (/root/reference/main.py:106-329)
on the MI355X execution model:

- 4 models (G: X->Y, F: Y->X, discriminators X, Y), 4 TF-style Adam
  optimizers (2e-4, beta1=0.5, beta2=0.9, eps=1e-7) over flat fp32 buffers;
- losses pre-scaled by 1/global_batch_size so SUM all-reduce over DP
  replicas is the exact global mean (main.py:172-174);
- per-step: one shared forward mega-graph; 4 gradient passes restricted to
  each model's variables (``torch.autograd.grad(loss, group.params)`` ==
  TF ``optimizer.minimize(var_list=...)``; grads land in the flat buffer
  via one batched multi-tensor copy), each followed immediately by an
  async RCCL all-reduce of that group's flat gradient, overlapping the next
  backward (reference runs the 4 groups serially, main.py:249-260);
- G's adversarial gradient flows through the frozen discriminator (the
  ``inputs=`` restriction limits accumulation, not the gradient path);
  each fake is discriminated ONCE and the node is shared by the
  adversarial and discriminator losses — gradient-identical to the
  reference's recomputed X(fake_x)/Y(fake_y) calls (main.py:239-245)
  under its var_list restriction, asserted by
  tests/test_trainer.py::test_train_step_grads_match_reference_structure;
- compute dtype bf16 on GPU (fp32 masters), fp32 on CPU;
- optional image history pool (``pool_size`` > 0, ops/pool.py; not in the
  reference): the discriminator losses see fakes exchanged with a buffer
  of earlier ones, the generator losses keep the fresh fakes;
- optional SSIM term in the cycle loss (``cycle_ssim`` = W in (0, 1],
  ops/ssim.py; not in the reference): per sample (1-W)·MAE + W·(1-SSIM),
  and two SSIM metrics in the test epoch (``test_ssim``, implied by W > 0).
"""

from __future__ import annotations

import contextlib
import os
from typing import Dict, Optional

import torch

from .models import Generator, Discriminator
from .ops import MAE, MSE, MSE_const, SSIM, ImagePool, backend, grad_sink
from .ops.adam import FusedAdam
from .parallel import DistContext, GradSync, FlatParamGroup


def lr_factor(epoch: int, epochs: int, decay_epochs: int) -> float:
    """Learning-rate factor of 0-based ``epoch`` in a run of ``epochs``:
    1 for the first ``epochs - decay_epochs`` epochs, then linear towards
    zero over the last ``decay_epochs`` — the schedule of the CycleGAN
    authors' public implementation with n_epochs = epochs - decay_epochs.
    It steps once per epoch, is 1/(decay_epochs+1) in the last epoch and
    never reaches 0 inside the run; decay_epochs == 0 gives 1 always."""
    if decay_epochs <= 0:
        return 1.0
    f = 1.0 - max(0, epoch - (epochs - decay_epochs) + 1) / (decay_epochs + 1)
    return min(1.0, max(0.0, f))


class CycleGAN:
    LAMBDA_CYCLE = 10.0
    LAMBDA_IDENTITY = 0.5 * 10.0
    # the four models, in optimizer and collective order
    _NAMES = ("G", "F", "X", "Y")

    def __init__(self, args, ctx: DistContext):
        self.ctx = ctx
        self.device = ctx.device
        self.global_batch_size = args.global_batch_size
        self.compute_dtype = getattr(args, "compute_dtype", None) or (
            torch.bfloat16 if self.device.type == "cuda" else torch.float32)
        self._fp8 = bool(getattr(args, "fp8", False))
        if self._fp8:
            from .ops import set_fp8_mode
            set_fp8_mode(True)
            self.compute_dtype = torch.bfloat16

        self.checkpoint_dir = os.path.join(args.output_dir, "checkpoints")
        if ctx.is_main:
            os.makedirs(self.checkpoint_dir, exist_ok=True)
        self.checkpoint_path = os.path.join(self.checkpoint_dir, "checkpoint.pt")

        nrb = getattr(args, "num_residual_blocks", 9)
        # generator upsampling blocks: "transpose" (the reference) or
        # "resize" (nearest-2x + conv3x3); recorded in the checkpoint
        self.upsample = getattr(args, "upsample", None) or "transpose"
        self.G = Generator(num_residual_blocks=nrb,
                           upsample=self.upsample).to(self.device)
        self.F = Generator(num_residual_blocks=nrb,
                           upsample=self.upsample).to(self.device)
        self.X = Discriminator().to(self.device)
        self.Y = Discriminator().to(self.device)

        # mirror rank-0 init to every replica (reference S7 broadcast)
        for m in (self.G, self.F, self.X, self.Y):
            ctx.broadcast_module(m)

        self.groups = {name: FlatParamGroup(getattr(self, name))
                       for name in self._NAMES}
        # averaged generator weights (ema_decay > 0): kept by G's and F's
        # optimizers only, the discriminators never run at inference
        self.ema_decay = float(getattr(args, "ema_decay", 0.0) or 0.0)
        self.lr_decay_epochs = int(getattr(args, "lr_decay_epochs", 0) or 0)
        self.optimizers = {
            name: FusedAdam(g.flat_param, g.flat_grad,
                            ema_decay=self.ema_decay if name in "GF" else 0.0)
            for name, g in self.groups.items()}
        self.sync = GradSync(ctx, timing=getattr(args, "verbose", 1) == 2)

        # shadow arenas: every bf16 compute form of a group, refreshed
        # after each optimizer step (ops/arena.py). Adam writes the arena's
        # mirror itself; the refresh builds the rest from it
        self.arenas = {}
        if (self.device.type == "cuda"
                and self.compute_dtype == torch.bfloat16
                and backend.load_ext() is not None):
            from .ops.arena import ShadowArena
            from .ops import shadow as _shadow
            for name in self._NAMES:
                a = ShadowArena(self.groups[name], getattr(self, name))
                _shadow.register_arena(a)
                self.arenas[name] = a
                self.optimizers[name].shadow = a.mirror

        # image history pools (fake x, fake y): built at the first step,
        # when the image shape is known; every rank keeps its own
        self.pool_size = int(getattr(args, "pool_size", 0) or 0)
        self._pool_seed = (int(getattr(args, "seed", 1234)), int(ctx.rank))
        self.pools = None
        # int32 [b] device codes of the step being built (one per pool)
        self._step_codes = None
        # while a graph step warms up and captures: its static all-pass
        # codes, so train_step draws nothing
        self._static_codes = None

        # SSIM: weight of the (1 - SSIM) term in the cycle loss, and the two
        # SSIM metrics of the test epoch (always on with the loss term).
        # Neither touches the weights: checkpoints are interchangeable
        self.cycle_ssim = float(getattr(args, "cycle_ssim", 0.0) or 0.0)
        if not 0.0 <= self.cycle_ssim <= 1.0:
            raise ValueError("cycle_ssim must be in [0, 1]")
        self.test_ssim = (bool(getattr(args, "test_ssim", False))
                          or self.cycle_ssim > 0.0)
        self._test_keys = self._TEST_KEYS + (
            self._SSIM_KEYS if self.test_ssim else ())

        # lazily-captured hip-graph step (main.py at N=1)
        self.graphed = None

    def _refresh_shadows(self, after_adam: bool = False):
        """after_adam: called right behind the optimizer steps on the same
        stream, so a mirror that Adam wrote is current; anywhere else the
        arena casts it from the masters itself."""
        for name, a in self.arenas.items():
            a.refresh(mirror_fresh=after_adam
                      and self.optimizers[name].wrote_shadow)

    def _snapshot_state(self):
        """Everything a train step may touch, for _restore_state: flat
        params and Adam m/v/t of every group, the weight averages (warm-up
        steps must not leak into them), the pools."""
        opts = self.optimizers
        return ({n: (g.flat_param.clone(), opts[n].m.clone(),
                     opts[n].v.clone(), opts[n].t)
                 for n, g in self.groups.items()},
                {n: o.ema.clone() for n, o in opts.items()
                 if o.ema is not None},
                [p.state_dict() for p in self.pools or ()])

    @torch.no_grad()
    def _restore_state(self, saved):
        state, emas, pools = saved
        for n, (p, m, v, t) in state.items():
            self.groups[n].flat_param.copy_(p)
            self.optimizers[n].m.copy_(m)
            self.optimizers[n].v.copy_(v)
            self.optimizers[n].t = t
        for n, e in emas.items():
            self.optimizers[n].ema.copy_(e)
        for p, s in zip(self.pools or (), pools):
            p.load_state_dict(s)
        self._refresh_shadows()

    # ---- learning-rate schedule, averaged generator weights ----

    def set_lr_scale(self, s: float):
        """Schedule factor on every optimizer's lr. A captured step picks
        it up through the device lr_t scalar (FusedAdam.advance_lr)."""
        for opt in self.optimizers.values():
            opt.lr_scale = float(s)

    @torch.no_grad()
    def _exchange_ema(self):
        for name in ("G", "F"):
            p, ema = self.groups[name].flat_param, self.optimizers[name].ema
            tmp = p.clone()
            p.copy_(ema)
            ema.copy_(tmp)
            self.groups[name].bump_versions()
        self._refresh_shadows()

    @contextlib.contextmanager
    def ema_weights(self):
        """Evaluate with the averaged generators: inside, G and F compute
        with the EMA weights; on exit (also on an exception) the live
        weights are back, both buffers bitwise as before. The CONTENTS of
        flat_param and ema are exchanged, never the pointers: the captured
        graph, the parameter views and the shadow arenas hold the
        addresses. A no-op with the average off."""
        if not self.ema_decay:
            yield
            return
        assert not (self.device.type == "cuda"
                    and torch.cuda.is_current_stream_capturing()), \
            "ema_weights() inside a graph capture"
        self._exchange_ema()
        try:
            yield
        finally:
            self._exchange_ema()

    def _ema_state_dict(self, name: str):
        """The averaged weights of G or F in module state_dict format:
        parameters viewed out of the flat average through the group's
        offsets, buffers taken from the live module."""
        module, group = getattr(self, name), self.groups[name]
        ema = self.optimizers[name].ema
        views = {id(p): ema[off:off + k].view(p.shape)
                 for p, (off, k) in zip(group.params, group._offsets)}
        sd = module.state_dict()
        for key, p in module.named_parameters():
            if id(p) in views:
                sd[key] = views[id(p)]
        return sd

    @torch.no_grad()
    def _load_ema_state_dict(self, name: str, sd):
        module, group = getattr(self, name), self.groups[name]
        ema = self.optimizers[name].ema
        offs = {id(p): ok for p, ok in zip(group.params, group._offsets)}
        for key, p in module.named_parameters():
            if id(p) in offs:
                off, k = offs[id(p)]
                ema[off:off + k].copy_(sd[key].reshape(-1))

    # ---- image history pool ----

    def _ensure_pools(self, image_shape):
        if self.pools is None:
            self.pools = tuple(
                ImagePool(self.pool_size, tuple(image_shape),
                          self.compute_dtype, self.device,
                          seed=self._pool_seed + (which,))
                for which in (0, 1))
        return self.pools

    def plan_pools(self, batch_sizes, image_shape):
        """Draw the pool decisions of the next ``len(batch_sizes)`` steps
        now and keep them on the device: the steps then take one table row
        each (ImagePool.next_codes) instead of an upload."""
        for pool in self._ensure_pools(image_shape):
            pool.plan(batch_sizes)

    def static_pool_codes(self, x):
        """All-pass codes for a graph step's warm-up and capture (None with
        the pool off): they leave pool contents, fill counts and decision
        streams alone. Set before each replay by refresh_pool_codes."""
        if not self.pool_size:
            return None
        self._ensure_pools(x.shape[1:])  # allocated outside the capture
        return tuple(torch.full((x.shape[0],), -1, dtype=torch.int32,
                                device=self.device) for _ in self.pools)

    def refresh_pool_codes(self, static_codes):
        """Next step's decisions into a captured step's static codes: a
        device-to-device row copy when the steps were planned."""
        for pool, codes in zip(self.pools, static_codes):
            codes.copy_(pool.next_codes(codes.shape[0]), non_blocking=True)

    def _pooled_discriminator_losses(self, x, y, fake_x, fake_y):
        """Discriminator losses on pooled fakes: one 2b-batched call per
        discriminator. The pooled images carry no graph, so these losses
        share nothing with the generator losses."""
        b = x.shape[0]
        out = []
        for D, real, fake, pool, codes in (
                (self.X, x, fake_x, self.pools[0], self._step_codes[0]),
                (self.Y, y, fake_y, self.pools[1], self._step_codes[1])):
            # (the HIP convs return contiguous NHWC: no copy there)
            pooled = pool.exchange(fake.detach().contiguous(), codes)
            d_real, d_fake = D(torch.cat([real, pooled])).split(b)
            out.append(self.discriminator_loss(d_real, d_fake))
        return out

    # ---- loss functions (reference main.py:172-195) ----

    def reduce_mean(self, per_sample: torch.Tensor) -> torch.Tensor:
        return per_sample.sum() / self.global_batch_size

    def generator_loss(self, discriminate_fake):
        return self.reduce_mean(MSE_const(discriminate_fake, 1.0))

    def cycle_loss(self, real, cycled):
        if self.cycle_ssim:
            w = self.cycle_ssim
            return self.LAMBDA_CYCLE * self.reduce_mean(
                (1.0 - w) * MAE(real, cycled)
                + w * (1.0 - SSIM(real, cycled)))
        return self.LAMBDA_CYCLE * self.reduce_mean(MAE(real, cycled))

    def identity_loss(self, real, same):
        return self.LAMBDA_IDENTITY * self.reduce_mean(MAE(real, same))

    def discriminator_loss(self, discriminate_real, discriminate_fake):
        real = MSE_const(discriminate_real, 1.0)
        fake = MSE_const(discriminate_fake, 0.0)
        return self.reduce_mean(0.5 * (real + fake))

    # ---- steps ----

    def _cast(self, t: torch.Tensor) -> torch.Tensor:
        return t.to(self.device, self.compute_dtype, non_blocking=True)

    _TRAIN_KEYS = ("loss_G/loss", "loss_G/cycle", "loss_G/identity",
                   "loss_G/total", "loss_F/loss", "loss_F/cycle",
                   "loss_F/identity", "loss_F/total", "loss_X/loss",
                   "loss_Y/loss")
    _TEST_KEYS = _TRAIN_KEYS + ("error/MAE(X, F(G(X)))",
                                "error/MAE(Y, G(F(Y)))",
                                "error/MAE(X, F(X))", "error/MAE(Y, G(Y))")
    # added to an instance's test keys by test_ssim
    _SSIM_KEYS = ("error/SSIM(X, F(G(X)))", "error/SSIM(Y, G(F(Y)))")

    def _zero_losses(self, keys) -> Dict[str, torch.Tensor]:
        z = torch.zeros((), device=self.device)
        return {k: z for k in keys}

    def _empty_train_step(self) -> Dict[str, torch.Tensor]:
        """Short final global batch under DP: this rank's slice is empty
        (the reference's MirroredStrategy replicas idle the same way,
        main.py:80-81). Contribute zero gradients but still join the
        all-reduces and take the identical optimizer step — after the
        SUM all-reduce every rank applies the same update, so replicas
        stay in sync."""
        for g in self.groups.values():
            g.flat_grad.zero_()
            self.sync.launch(g.flat_grad)
        self.sync.wait_all()
        # no fp8 amax roll: the empty slice recorded no amax, and
        # prev <- cur would zero prev
        self._optimize(roll_amax=False)
        return self._zero_losses(self._TRAIN_KEYS)

    def _forward_losses(self, x, y) -> Dict[str, torch.Tensor]:
        """The step's forward mega-graph: all 10 loss scalars, grads not
        yet taken (shared by the eager, fully-graphed, and segmented-graph
        step drivers)."""
        b = x.shape[0]
        # batched generator calls: every op is per-sample (convs, per-sample
        # InstanceNorm stats, per-sample losses), so G(cat(x,y)) is
        # numerically identical to G(x), G(y) — fewer, larger kernels.
        #
        # The cycle inputs are detached: under the reference's var_list
        # restriction (main.py:249-260) no optimizer ever follows the
        # fake_y -> G path out of F's cycle branch (F_cycle is only in
        # F_total, whose grads stop at F's own weights), so cutting it is
        # gradient-identical and lets F run as ONE 3b-batched call without
        # autograd descending a numerically-zero path into G.
        # torch.split, not slicing: split's backward is ONE cat of the
        # branch grads; slice backward is a zero-fill + copy + add per
        # branch (and leaves non-contiguous dy for the conv backwards)
        fake_y, same_y = self.G(torch.cat([x, y])).split(b)
        f_out = self.F(torch.cat([y, x, fake_y.detach()]))
        fake_x, same_x, cycle_x = f_out.split(b)
        cycle_y = self.G(fake_x.detach())

        # ONE discriminator pass per fake, shared by the adversarial and
        # discriminator losses (the reference recomputes X(fake_x) at
        # main.py:239-245 with identical values; TF graph-mode CSE merges
        # them the same way). X's own update never reaches fake_x: the
        # path stops at X's first conv weights.
        discriminate_fake_x = self.X(fake_x)
        discriminate_fake_y = self.Y(fake_y)

        G_loss = self.generator_loss(discriminate_fake_y)
        F_loss = self.generator_loss(discriminate_fake_x)
        G_cycle_loss = self.cycle_loss(y, cycle_y)
        F_cycle_loss = self.cycle_loss(x, cycle_x)
        G_identity_loss = self.identity_loss(y, same_y)
        F_identity_loss = self.identity_loss(x, same_x)
        losses = self._loss_dict(G_loss, G_cycle_loss, G_identity_loss,
                                 F_loss, F_cycle_loss, F_identity_loss)
        if self.pool_size:
            # history pool: the discriminators train on exchanged fakes,
            # so their pass over the fake is no longer the generators' one
            losses["loss_X/loss"], losses["loss_Y/loss"] = \
                self._pooled_discriminator_losses(x, y, fake_x, fake_y)
        else:
            losses["loss_X/loss"] = self.discriminator_loss(
                self.X(x), discriminate_fake_x)
            losses["loss_Y/loss"] = self.discriminator_loss(
                self.Y(y), discriminate_fake_y)
        return losses

    @staticmethod
    def _loss_dict(G_loss, G_cycle, G_identity, F_loss, F_cycle,
                   F_identity) -> Dict[str, torch.Tensor]:
        """The loss dict of a step from the six generator terms, in
        _TRAIN_KEYS order. The caller adds loss_X/loss and loss_Y/loss
        afterwards: the totals are summed here, before the discriminators
        see the real images, which is where the step has always launched
        those additions."""
        return {
            "loss_G/loss": G_loss, "loss_G/cycle": G_cycle,
            "loss_G/identity": G_identity,
            "loss_G/total": G_loss + G_cycle + G_identity,
            "loss_F/loss": F_loss, "loss_F/cycle": F_cycle,
            "loss_F/identity": F_identity,
            "loss_F/total": F_loss + F_cycle + F_identity,
        }

    _GROUP_LOSS = tuple(zip(_NAMES, ("loss_G/total", "loss_F/total",
                                     "loss_X/loss", "loss_Y/loss")))

    def _grads_for(self, losses: Dict[str, torch.Tensor], name: str,
                   retain: bool):
        """One group's backward pass into its flat grad buffer.

        torch.autograd.grad (not .backward): no AccumulateGrad per-param
        add into the .grad views (~300 tiny launches/step) and no flat
        zero-fill. On the HIP path the backward kernels write each
        gradient into its flat-grad view themselves (ops.grad_sink);
        whatever autograd still returns as a tensor (CPU path,
        CYG_NO_GRAD_SINK=1) lands there via ONE batched multi-tensor copy.
        retain_graph through X's pass: the shared discriminate_fake_*
        subgraphs are traversed by both the generator and discriminator
        passes (see _retain)."""
        key = dict(self._GROUP_LOSS)[name]
        group = self.groups[name]
        # on the HIP path the kernels that finish a gradient write it into
        # the flat buffer themselves (ops.grad_sink) and autograd gets None
        sink = group.grad_sink()
        with grad_sink.active(sink):
            grads = torch.autograd.grad(losses[key], group.params,
                                        retain_graph=retain,
                                        allow_unused=sink is not None)
        group.set_grads(grads, sink)

    def _retain(self, i: int) -> bool:
        """retain_graph for the i-th pass of _GROUP_LOSS. Pool off: the
        discriminate_fake_* subgraphs are shared, keep them until Y's pass.
        Pool on: the four losses have disjoint graphs (cycle inputs and
        pooled fakes are detached), each pass may free its own."""
        return i < 3 and not self.pool_size

    def _optimize(self, roll_amax: bool = True):
        """The optimizer stage of every step driver (eager, empty slice,
        both graph steps): nothing else steps the optimizers."""
        for opt in self.optimizers.values():
            opt.step()
        for g in self.groups.values():
            g.bump_versions()  # invalidate bf16 shadow caches (see flat.py)
        self._refresh_shadows(after_adam=True)
        if self._fp8 and roll_amax:
            from .ops import fp8_state
            fp8_state.roll()  # delayed-scaling amax: prev <- cur

    def train_step(self, x, y) -> Dict[str, torch.Tensor]:
        x, y = self._cast(x), self._cast(y)
        if x.shape[0] == 0:
            return self._empty_train_step()
        if self.pool_size:
            # the eager step draws for itself; a graph step that is
            # warming up or capturing has set its static codes instead
            self._step_codes = self._static_codes or tuple(
                pool.next_codes(x.shape[0])
                for pool in self._ensure_pools(x.shape[1:]))
        losses = self._forward_losses(x, y)
        for i, (name, _) in enumerate(self._GROUP_LOSS):
            self._grads_for(losses, name, retain=self._retain(i))
            self.sync.launch(self.groups[name].flat_grad)
        self.sync.wait_all()
        self._optimize()
        return {k: losses[k].detach() for k in self._TRAIN_KEYS}

    @torch.no_grad()
    def cycle_step(self, x, y, training: bool = False):
        x, y = self._cast(x), self._cast(y)
        fake_y = self.G(x)
        cycle_x = self.F(fake_y)
        fake_x = self.F(y)
        cycle_y = self.G(fake_x)
        return fake_x, fake_y, cycle_x, cycle_y

    @torch.no_grad()
    def test_step(self, x, y) -> Dict[str, torch.Tensor]:
        x, y = self._cast(x), self._cast(y)
        if x.shape[0] == 0:  # empty DP slice of a short final batch
            return self._zero_losses(self._test_keys)
        fake_x, fake_y, cycle_x, cycle_y = self.cycle_step(x, y)

        discriminate_fake_x = self.X(fake_x)
        discriminate_fake_y = self.Y(fake_y)
        G_loss = self.generator_loss(discriminate_fake_y)
        F_loss = self.generator_loss(discriminate_fake_x)
        F_cycle_loss = self.cycle_loss(x, cycle_x)
        G_cycle_loss = self.cycle_loss(y, cycle_y)
        same_x = self.F(x)
        same_y = self.G(y)
        G_identity_loss = self.identity_loss(y, same_y)
        F_identity_loss = self.identity_loss(x, same_x)
        losses = self._loss_dict(G_loss, G_cycle_loss, G_identity_loss,
                                 F_loss, F_cycle_loss, F_identity_loss)
        X_loss = self.discriminator_loss(self.X(x), discriminate_fake_x)
        Y_loss = self.discriminator_loss(self.Y(y), discriminate_fake_y)

        results = {
            **losses, "loss_X/loss": X_loss, "loss_Y/loss": Y_loss,
            "error/MAE(X, F(G(X)))": self.reduce_mean(MAE(x, cycle_x)),
            "error/MAE(Y, G(F(Y)))": self.reduce_mean(MAE(y, cycle_y)),
            "error/MAE(X, F(X))": self.reduce_mean(MAE(x, same_x)),
            "error/MAE(Y, G(Y))": self.reduce_mean(MAE(y, same_y)),
        }
        if self.test_ssim:
            results["error/SSIM(X, F(G(X)))"] = self.reduce_mean(
                SSIM(x, cycle_x))
            results["error/SSIM(Y, G(F(Y)))"] = self.reduce_mean(
                SSIM(y, cycle_y))
        return results

    # ---- checkpoint (reference main.py:148-170: one overwriting prefix,
    # all 4 models + 4 optimizer states, auto-resume if present) ----

    def save_checkpoint(self):
        if self.ctx.is_main:
            state = {n: getattr(self, n).state_dict() for n in self._NAMES}
            # the generator variants share keys and shapes: say which. The
            # default writes nothing (a missing entry means transpose), so
            # its checkpoints keep exactly the keys they always had
            if self.upsample != "transpose":
                state["arch"] = {"upsample": self.upsample}
            for n in self._NAMES:
                state[f"{n}_optimizer"] = self.optimizers[n].state_dict()
            if self.ema_decay:
                state["G_ema"] = self._ema_state_dict("G")
                state["F_ema"] = self._ema_state_dict("F")
            if self.pools is not None:  # this rank's; ranks are not synced
                state["pool_x"] = self.pools[0].state_dict()
                state["pool_y"] = self.pools[1].state_dict()
            tmp = self.checkpoint_path + ".tmp"
            torch.save(state, tmp)
            os.replace(tmp, self.checkpoint_path)
            print(f"\nsaved checkpoint to {self.checkpoint_path}\n")
        self.ctx.barrier()

    def load_checkpoint(self) -> bool:
        if not os.path.exists(self.checkpoint_path):
            return False
        state = torch.load(self.checkpoint_path, map_location=self.device,
                           weights_only=True)
        # a checkpoint from before the flag has no entry: transpose
        saved = state.get("arch", {}).get("upsample", "transpose")
        if saved != self.upsample:
            raise RuntimeError(
                f"{self.checkpoint_path} was trained with --upsample {saved}, "
                f"this run has --upsample {self.upsample}: the weights have "
                "the same shapes but are not interchangeable; pass "
                f"--upsample {saved} or use another --output_dir")
        for name in self._NAMES:
            getattr(self, name).load_state_dict(state[name])
        for name in self._NAMES:
            self.optimizers[name].load_state_dict(state[f"{name}_optimizer"])
        if self.ema_decay:
            # a checkpoint without averages restarts them from the weights
            # just loaded (the construction-time copy holds the random
            # init); with the average off, saved ones are ignored
            for name in ("G", "F"):
                if f"{name}_ema" in state:
                    self._load_ema_state_dict(name, state[f"{name}_ema"])
                else:
                    self.optimizers[name].reset_ema()
        if self.pool_size and "pool_x" in state:
            # a checkpoint without pools starts them empty; with the pool
            # off, saved pools are ignored
            pools = self._ensure_pools(state["pool_x"]["buf"].shape[1:])
            pools[0].load_state_dict(state["pool_x"])
            pools[1].load_state_dict(state["pool_y"])
        self._refresh_shadows()
        print(f"\nloaded checkpoint from {self.checkpoint_path}\n")
        return True

    # ---- epoch-level metric reduction (S5, deferred to epoch end) ----

    def reduce_results(self, accumulated: Dict[str, list]) -> Dict[str, float]:
        """Mean over steps, SUM all-reduce over replicas, to host floats."""
        if not accumulated:
            return {}
        keys = list(accumulated.keys())
        means = torch.stack([torch.stack([v.float() for v in accumulated[k]]).mean()
                             for k in keys])
        self.ctx.all_reduce_(means)
        vals = means.tolist()
        return dict(zip(keys, vals))


class _GraphStep:
    """What the two graph steps share: static inputs and pool codes,
    warm-up, the state roll-back after the capture, and everything a
    replay does around its graph launches. A subclass captures in
    ``_capture`` (which sets ``out`` and ``_packed``) and launches in
    ``_replay``."""

    def __init__(self, gan: CycleGAN, x: torch.Tensor, y: torch.Tensor,
                 warmup: int = 2, preserve_state: bool = False):
        assert gan.ctx.device.type == "cuda"
        self.gan = gan
        self.sx = gan._cast(x).clone()
        self.sy = gan._cast(y).clone()
        # history pool: static codes, all-pass through warm-up and capture
        self.codes = gan._static_codes = gan.static_pool_codes(self.sx)
        # preserve_state: roll model/optimizer state back after the warmup
        # steps so capturing mid-training perturbs nothing (main.py uses
        # this to capture on the first batch of an epoch)
        saved = gan._snapshot_state() if preserve_state else None
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                gan.train_step(self.sx, self.sy)
        torch.cuda.current_stream().wait_stream(s)
        for opt in gan.optimizers.values():
            opt.prepare_graph()
        # capture records the kernel sequence without executing it: the
        # optimizer step count is NOT advanced here, so replay #1 runs the
        # exact t the eager path would
        self._capture()
        gan._static_codes = None  # eager steps draw for themselves again
        if saved is not None:
            gan._restore_state(saved)

    def __call__(self, x=None, y=None) -> Dict[str, torch.Tensor]:
        gan = self.gan
        if x is not None:
            self.sx.copy_(gan._cast(x))
            self.sy.copy_(gan._cast(y))
        for opt in gan.optimizers.values():
            opt.advance_lr()
        if self.codes is not None:
            gan.refresh_pool_codes(self.codes)
        self._replay()
        for g in gan.groups.values():
            g.bump_versions()
        return self.out

    def call_cloned(self, x, y) -> Dict[str, torch.Tensor]:
        """Replay and return loss scalars detached from the static graph
        outputs (ONE clone kernel), safe to accumulate across steps."""
        self(x, y)
        p = self._packed.clone()
        return {k: p[i] for i, k in enumerate(self.gan._TRAIN_KEYS)}


class GraphedStep(_GraphStep):
    """The steady-state train step captured as ONE hip graph.

    The whole step — bf16 shadow recasts, batched G/F/D forwards, the four
    backward passes, flat-grad copies and the four fused Adam updates —
    replays as a single graph launch, eliminating the per-kernel host
    launch gaps of ~300 small launches (the reference leans on TF's
    tracing compiler for the same effect, reference main.py:198-205;
    the MI355X-native equivalent is hipGraph capture).

    Requirements: static shapes, CUDA device, world_size == 1 (RCCL graph
    capture is intentionally not enabled yet). The optimizer's bias
    correction is read from a device scalar refreshed before every replay,
    so the captured step tracks t exactly like the eager path.
    """

    def __init__(self, gan: CycleGAN, x: torch.Tensor, y: torch.Tensor,
                 warmup: int = 2, preserve_state: bool = False):
        # world_size > 1 capture (RCCL collectives inside the graph) is
        # proven at 1 rank (profiles/rccl_shakeout.md) but intentionally
        # opt-in for multi-rank until measured there: CYG_GRAPH_DIST=1.
        assert gan.ctx.device.type == "cuda" and (
            gan.ctx.world_size == 1
            or os.environ.get("CYG_GRAPH_DIST") == "1")
        super().__init__(gan, x, y, warmup, preserve_state)

    def _capture(self):
        gan = self.gan
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = gan.train_step(self.sx, self.sy)
            self._packed = torch.stack([self.out[k] for k in gan._TRAIN_KEYS])

    def _replay(self):
        self.graph.replay()


class SegmentedGraphedStep(_GraphStep):
    """Multi-rank graph step: the step is captured as FIVE RCCL-free hip
    graphs (forward + G-grads, F-grads, X-grads, Y-grads, optimizers)
    sharing one capture pool, and the four flat-gradient all-reduces are
    issued EAGERLY between the replays. Multi-rank runs get the captured
    kernel-launch profile (eager measured ~3.5% slower at N=1) without
    capturing any collective — RCCL-in-graph capture stays opt-in
    (CYG_GRAPH_DIST=1, GraphedStep). Collective order matches the eager
    path exactly (G, F, X, Y), so graphed and eager/empty-slice ranks
    interoperate."""

    def _capture(self):
        gan = self.gan
        gan._step_codes = self.codes  # train_step's part, skipped below
        self.grad_graphs, pool = {}, None
        for i, name in enumerate(gan._NAMES):
            g = self.grad_graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool):
                if i == 0:  # the forward rides in G's graph
                    losses = gan._forward_losses(self.sx, self.sy)
                gan._grads_for(losses, name, retain=gan._retain(i))
            pool = pool or g.pool()
        self.opt_graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.opt_graph, pool=pool):
            gan._optimize()
            self._packed = torch.stack([losses[k] for k in gan._TRAIN_KEYS])
        self.out = {k: losses[k].detach() for k in gan._TRAIN_KEYS}

    def _replay(self):
        gan = self.gan
        for name, g in self.grad_graphs.items():
            g.replay()
            gan.sync.launch(gan.groups[name].flat_grad)
        gan.sync.wait_all()
        self.opt_graph.replay()

