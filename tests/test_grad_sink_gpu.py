"""The gradient sink end to end: a 64x64, 1-resblock CycleGAN's forward and
its four backward passes, with the sink and with CYG_NO_GRAD_SINK=1, from
the same weights.

Conv-weight gradients lie on an atomics-free path (split-M slabs summed in
a fixed order, the prior added last), so as long as the no-sink path itself
repeats bit for bit the sink must reproduce it bit for bit; otherwise both
are held to the wgrad bound. The one exception is the packed generator
head: its fold adds eight fp32 terms per element, the kernel in ascending d
and _fold_packed_dw in whatever order torch.sum takes (measured: not the
same bits), so from identical packed results the two differ by at most
2*E with E = sum over calls of 8*u32*sum_d|term| + u32*|result|, the bound
of the fold's unit test. gamma / beta / bias gradients are sums of fp32
atomics with no fixed order: each run is within

    E = sum over the parameter's calls of 2*M*u32*sum|addend| + u32*|result|

of the exact sum of the same addends (M = rows the call reduces; the second
term is the add of the prior), so two runs differ by at most 2*E. The
addends' magnitudes are recorded from the arguments of the no-sink run, in
the pass of the group that owns the parameter only (the calls a generator's
pass makes for the frozen discriminator add nothing to the gradient and
nothing to E).

Also counted, by wrapping the extension's entry points: no weight gradient
runs for a parameter outside the active group.

All tests @pytest.mark.gpu.
"""

import argparse

import pytest
import torch

import _kernel_bounds as kb
from cyclegan_amd.models.layers import ConvNHWC, ConvTransposeNHWC
from cyclegan_amd.ops import backend, conv as conv_ops

pytestmark = pytest.mark.gpu

# forward calls of each model in one step (trainer._forward_losses): G on
# cat(x, y) and on fake_x; F once on the 3b batch; X and Y on real and fake
CALLS = {"G": 2, "F": 1, "X": 2, "Y": 2}
# the frozen discriminator a generator's pass walks through
FROZEN = {"G": "Y", "F": "X"}


def n_convs(m):
    return sum(isinstance(s, (ConvNHWC, ConvTransposeNHWC))
               for s in m.modules())


class Recorder:
    """Wraps the extension's gradient entry points: counts weight-gradient
    launches per pass and sums the addend magnitudes of the atomics."""

    def __init__(self, monkeypatch, gan):
        self.ext = ext = backend.ext()
        self.gan = gan
        self.pass_name = None
        self.wgrad = []       # (pass, "plain" | "into", out or None)
        self.mag = {}         # param data_ptr -> fp64 [n] bound, summed
        self.owned = {n: {p.data_ptr() for p in g.params}
                      for n, g in gan.groups.items()}
        for name in ("conv2d_wgrad", "conv2d_wgrad_into", "instnorm_bwd"):
            monkeypatch.setattr(ext, name, self._wrap(name, getattr(ext, name)))
        real_bias = conv_ops._bias_grad

        def bias_grad(ext_, sink, bias, dyp, n):
            M = dyp.numel() // dyp.shape[-1]
            s = dyp.double().abs().sum((0, 1, 2))[:n]
            self._add(bias, 2 * M * kb.U32 * s)
            return real_bias(ext_, sink, bias, dyp, n)

        monkeypatch.setattr(conv_ops, "_bias_grad", bias_grad)
        real_fold = conv_ops._fold_packed_dw
        self.head_mag = {}    # pass -> fp64 OHWI bound of the folds, summed

        def fold(dwp, wshape):
            b = 8 * kb.U32 * real_fold(dwp.double().abs(), wshape)
            self.head_mag[self.pass_name] = \
                self.head_mag.get(self.pass_name, 0) + b
            return real_fold(dwp, wshape)

        monkeypatch.setattr(conv_ops, "_fold_packed_dw", fold)

    def _add(self, p, bound):
        """Only the calls that form the compared gradient count: those of
        the pass whose group owns p. A generator's pass also calls the
        norm backward (and, without the sink, the bias sum) of the frozen
        discriminator it walks through; that result is dropped."""
        k = p.data_ptr()
        if k not in self.owned[self.pass_name]:
            return
        self.mag[k] = self.mag.get(k, 0) + bound

    def _wrap(self, name, real):
        def f(*a, **kw):
            if name == "conv2d_wgrad":
                self.wgrad.append((self.pass_name, "plain", None))
            elif name == "conv2d_wgrad_into":
                self.wgrad.append((self.pass_name, "into", a[8]))
            else:
                self._norm_mag(*a[:9])
            return real(*a, **kw)
        return f

    def _norm_mag(self, dy, x, gamma, mean, rstd, yact, act, slope,
                  beta=None):
        d = dy.double()
        if act != kb.ACT_NONE:
            assert yact is not None and act in (kb.ACT_RELU, kb.ACT_LRELU)
            neg = 0.0 if act == kb.ACT_RELU else slope
            d = torch.where(yact > 0, d, d * neg)
        xh = ((x.double() - mean.double()[:, None, None])
              * rstd.double()[:, None, None])
        M = x.shape[0] * x.shape[1] * x.shape[2]
        self._add(gamma, 2 * M * kb.U32 * (d * xh).abs().sum((0, 1, 2)))
        if beta is not None:
            self._add(beta, 2 * M * kb.U32 * d.abs().sum((0, 1, 2)))


def run_passes(gan, x, y, rec=None):
    """Forward + the four backward passes; the flat grads, cloned. The
    buffers start as NaN: every element must be written."""
    for g in gan.groups.values():
        g.flat_grad.fill_(float("nan"))
    losses = gan._forward_losses(x, y)
    for i, (name, _) in enumerate(gan._GROUP_LOSS):
        if rec is not None:
            rec.pass_name = name
        gan._grads_for(losses, name, retain=i < 3)
    torch.cuda.synchronize()
    return {n: g.flat_grad.clone() for n, g in gan.groups.items()}


def param_slices(group):
    return [(p, slice(off, off + k)) for p, (off, k)
            in zip(group.params, group._offsets)]


def test_sink_matches_no_sink(tmp_path, monkeypatch):
    from cyclegan_amd.parallel import DistContext
    from cyclegan_amd.trainer import CycleGAN
    a = argparse.Namespace()
    a.output_dir = str(tmp_path)
    a.batch_size = a.global_batch_size = 1
    a.num_residual_blocks = 1
    a.compute_dtype = torch.bfloat16
    torch.manual_seed(0)
    ctx = DistContext(device=torch.device("cuda", 0))
    gan = CycleGAN(a, ctx)
    x = torch.rand(1, 64, 64, 3, device=ctx.device, dtype=torch.bfloat16) * 2 - 1
    y = torch.rand(1, 64, 64, 3, device=ctx.device, dtype=torch.bfloat16) * 2 - 1
    models = {"G": gan.G, "F": gan.F, "X": gan.X, "Y": gan.Y}

    rec = Recorder(monkeypatch, gan)
    monkeypatch.setenv("CYG_NO_GRAD_SINK", "1")
    ref = run_passes(gan, x, y, rec)
    ref_calls, rec.wgrad = rec.wgrad, []
    mag, head_mag = dict(rec.mag), dict(rec.head_mag)
    assert sorted(head_mag) == ["F", "G"]
    ref2 = run_passes(gan, x, y)
    monkeypatch.delenv("CYG_NO_GRAD_SINK")
    rec.wgrad = []
    got = run_passes(gan, x, y, rec)
    sink_calls = rec.wgrad

    # ---- launches: every conv's wgrad once per forward call of its model;
    # without the sink also the frozen discriminator's in each generator's
    # pass (one forward call of it lies on that path)
    own = sum(n_convs(models[n]) * CALLS[n] for n in models)
    wasted = sum(n_convs(models[d]) for d in FROZEN.values())
    assert (n_convs(gan.G), n_convs(gan.X)) == (8, 5)
    assert own == 44 and wasted == 10
    assert len(ref_calls) == own + wasted == 54
    assert len(sink_calls) == own
    for name in models:
        mine = [c for c in sink_calls if c[0] == name]
        assert len(mine) == n_convs(models[name]) * CALLS[name], name
        fg = gan.groups[name].flat_grad
        lo, hi = fg.data_ptr(), fg.data_ptr() + fg.numel() * 4
        for _, kind, out in mine:
            if kind == "into":
                assert lo <= out.data_ptr() < hi, \
                    f"{name}: wgrad written outside the active group"
        # plain conv2d_wgrad under the sink: only the packed heads, whose
        # fold kernel writes the destination
        heads = CALLS[name] if name in FROZEN else 0
        assert sum(c[1] == "plain" for c in mine) == heads, name

    # ---- values
    exact = all(torch.equal(ref[n][s], ref2[n][s]) for n in models
                for p, s in param_slices(gan.groups[n]) if p.dim() == 4)
    print(f"no-sink conv-weight grads repeat bit for bit: {exact}")
    assert exact, "precondition: the no-sink wgrad path is not deterministic"
    for n in models:
        assert torch.isfinite(got[n]).all() and torch.isfinite(ref[n]).all()
        worst = 0.0
        for p, s in param_slices(gan.groups[n]):
            if p.dim() == 4 and not (n in head_mag
                                     and p is models[n].head.weight):
                assert torch.equal(got[n][s], ref[n][s]), \
                    f"{n}: conv weight grad {tuple(p.shape)} differs"
                continue
            if p.dim() == 4:  # packed head: see the module docstring
                r = ref[n][s].double()
                E = head_mag[n].reshape(-1) + kb.U32 * r.abs()
                err = (got[n][s].double() - r).abs()
                assert (err <= 2 * E).all(), f"{n}: packed head weight grad"
                print(f"{n}: packed head err/bound "
                      f"{float((err / (2 * E).clamp(min=1e-300)).max()):.3f}")
                continue
            r = ref[n][s].double()
            E = mag[p.data_ptr()] + kb.U32 * r.abs()
            err = (got[n][s].double() - r).abs()
            assert (err <= 2 * E).all(), \
                f"{n}: 1-d grad [{p.numel()}] off by {(err / (2 * E)).max()}"
            worst = max(worst, float((err / (2 * E).clamp(min=1e-300)).max()))
        print(f"{n}: worst 1-d err/bound {worst:.3f}")
