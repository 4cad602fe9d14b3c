"""Reflect dgrad that writes the unpadded frame (the gather sends window
rows to dx and ring rows to a side image, reflect_ring_add_kernel folds
the ring in place) against the full-frame fold it replaces
(CYG_NO_DIRECT_FOLD=1, read per call) and against fp64.

The two paths round the same fp32 sums in the same order, so dx must be
equal, not merely close. Shapes are the reflect rows of
tests/_kernel_bounds.py: every pad combination of the table, H != W, an M
tail, pad = H-1 (three live candidates per axis, the two mirrored
intervals of an axis merge), pads on one side only, a 128-wide tile with
the XCD remap on. tests/test_reflect_ring_cpu.py proves the ring layout
and the set of mirrored pixels on the CPU.

All tests @pytest.mark.gpu.
"""

import pytest
import torch

import _kernel_bounds as kb
from cyclegan_amd.ops import backend

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FOLD_CASES = ["nsq_reflect", "cin24", "cin96", "reflect_asym", "k7_padmax",
              "ow64_short", "grid8"]

_inputs = {}
_refs = {}


def inputs(case):
    if case.id not in _inputs:
        _, w, _, dy = kb.make_inputs(case)
        _inputs[case.id] = (dy.to(DEV).contiguous(),
                            w.permute(3, 1, 2, 0).contiguous().to(DEV),
                            dy, w)
    return _inputs[case.id]


def ref(case):
    if case.id not in _refs:
        _, _, dy, w = inputs(case)
        _refs[case.id] = kb.dgrad_ref_bound(case, dy, w)
    return _refs[case.id]


def run_dgrad(case):
    dyd, wtd, _, _ = inputs(case)
    return backend.ext().conv2d_dgrad(dyd, wtd, case.H, case.W, case.stride,
                                      *case.pads, case.reflect)


@pytest.mark.parametrize("cid", FOLD_CASES)
def test_direct_fold_equals_full_frame_fold(cid, monkeypatch):
    case = kb.CASE_BY_ID[cid]
    assert case.reflect and case.stride == 1
    monkeypatch.delenv("CYG_NO_DIRECT_FOLD", raising=False)
    direct = run_dgrad(case)
    monkeypatch.setenv("CYG_NO_DIRECT_FOLD", "1")
    full = run_dgrad(case)
    assert tuple(direct.shape) == case.x_shape and direct.is_contiguous()
    # the switch took effect: the full-frame path returns its own tensor,
    # the direct path the head of the padded-frame allocation
    assert full.untyped_storage().nbytes() == full.numel() * 2
    assert direct.untyped_storage().nbytes() > direct.numel() * 2
    assert torch.equal(direct, full)
    kb.assert_within(direct, *ref(case), f"{cid}:dx direct")
    kb.assert_within(full, *ref(case), f"{cid}:dx full-frame")


@pytest.mark.parametrize("cid", ["nsq_reflect", "k7_padmax"])
def test_no_element_read_before_written(cid, monkeypatch):
    """With the allocator's free memory full of NaN, a dx or ring element
    that the ring add read before the gather wrote it would show."""
    case = kb.CASE_BY_ID[cid]
    monkeypatch.delenv("CYG_NO_DIRECT_FOLD", raising=False)
    a = run_dgrad(case).clone()
    junk = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
    junk.view(torch.bfloat16).fill_(float("nan"))
    del junk
    b = run_dgrad(case)
    assert torch.isfinite(b).all()
    assert torch.equal(a, b)
    kb.assert_within(b, *ref(case), f"{cid}:dx after NaN fill")


def test_zero_pad_dgrad_unchanged_by_switch(monkeypatch):
    """The window decode is off unless the call is a reflect dgrad."""
    case = kb.CASE_BY_ID["pads_asym"]
    monkeypatch.delenv("CYG_NO_DIRECT_FOLD", raising=False)
    a = run_dgrad(case)
    monkeypatch.setenv("CYG_NO_DIRECT_FOLD", "1")
    b = run_dgrad(case)
    assert torch.equal(a, b)
    _, _, dy, w = inputs(case)
    kb.assert_within(a, *kb.dgrad_ref_bound(case, dy, w), "pads_asym:dx")
