"""CPU test for tools/ssim_micro.py: it imports without a GPU, parses its
options and states the bytes each case has to move."""

import importlib.util
import os

import pytest


def _load():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "ssim_micro", os.path.join(root, "tools", "ssim_micro.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_ssim_micro_imports_and_parses():
    mod = _load()
    ap = mod.build_parser()
    a = ap.parse_args(["kernel"])
    assert (a.mode, a.iters, a.warmup, a.replays) == ("kernel", 500, 50, 50)
    a = ap.parse_args(["kernel", "--iters", "7", "--warmup", "2"])
    assert (a.iters, a.warmup) == (7, 2)
    a = ap.parse_args(["step", "--cycle_ssim", "0", "--steps", "7"])
    assert (a.mode, a.cycle_ssim, a.steps, a.warmup) == ("step", 0.0, 7, 10)
    assert ap.parse_args(["step"]).cycle_ssim == 0.5
    for bad in ([], ["layer"], ["kernel", "--bogus"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    assert mod.SHAPE == (4, 256, 256, 3)
    need = mod.must_move()
    image = 4 * 256 * 256 * 3 * 2
    maps = 3 * 4 * 246 * 246 * 3 * 4
    assert need == {"ssim_fwd": 2 * image,
                    "ssim_fwd_bwd": 5 * image + 2 * maps,
                    "mae_fwd": 2 * image, "mae_fwd_bwd": 6 * image}
