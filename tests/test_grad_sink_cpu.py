"""Without the HIP path the gradient sink is inert: _grads_for fills the
flat grad buffers with exactly what torch.autograd.grad returns."""

import argparse

import torch

from cyclegan_amd.ops import grad_sink
from cyclegan_amd.parallel import DistContext
from cyclegan_amd.trainer import CycleGAN


def make_gan(tmp_path):
    a = argparse.Namespace()
    a.output_dir = str(tmp_path)
    a.batch_size = a.global_batch_size = 1
    a.num_residual_blocks = 1
    a.compute_dtype = torch.float32
    torch.manual_seed(0)
    return CycleGAN(a, DistContext(device=torch.device("cpu")))


def test_sink_inert_on_cpu(tmp_path):
    gan = make_gan(tmp_path)
    x = torch.rand(1, 16, 16, 3) * 2 - 1
    y = torch.rand(1, 16, 16, 3) * 2 - 1
    losses = gan._forward_losses(x, y)
    for name, key in gan._GROUP_LOSS:
        group = gan.groups[name]
        assert group.grad_sink() is None
        want = torch.autograd.grad(losses[key], group.params,
                                   retain_graph=True)
        flat = torch.cat([g.reshape(-1) for g in want])
        group.flat_grad.fill_(float("nan"))
        gan._grads_for(losses, name, retain=True)
        assert grad_sink.current() is None
        assert torch.equal(group.flat_grad, flat), name
        assert group.check_views()


def test_sink_bookkeeping():
    """GradSink on plain tensors: first take writes, later takes
    accumulate; tensors outside it are frozen only while it is active."""
    p = [torch.zeros(4, requires_grad=True), torch.zeros(2, 3, requires_grad=True)]
    other = torch.zeros(5, requires_grad=True)
    views = [torch.zeros(4), torch.zeros(2, 3)]
    sink = grad_sink.GradSink(p, views)
    assert not grad_sink.frozen(None, other)
    assert grad_sink.frozen(sink, other) and not grad_sink.frozen(sink, p[0])
    assert not grad_sink.frozen(sink, other * 2)      # not a leaf
    v, acc = sink.take(p[1])
    assert v is views[1] and acc is False and sink.touched(p[1])
    assert sink.take(p[1])[1] is True
    assert not sink.touched(p[0]) and not sink.touched(other)
    with grad_sink.active(sink):
        assert grad_sink.current() is sink
    assert grad_sink.current() is None
