"""CPU test for tools/upconv_micro.py: it imports without a GPU and parses
its two modes."""

import importlib.util
import os

import pytest


def _load():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "upconv_micro", os.path.join(root, "tools", "upconv_micro.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_upconv_micro_imports_and_parses():
    mod = _load()
    ap = mod.build_parser()
    a = ap.parse_args(["layer"])
    assert a.mode == "layer" and a.iters == 1000 and a.warmup == 50
    a = ap.parse_args(["step", "--upsample", "transpose", "--steps", "7"])
    assert (a.mode, a.upsample, a.steps, a.warmup) == ("step", "transpose",
                                                       7, 10)
    assert ap.parse_args(["step"]).upsample == "resize"
    for bad in ([], ["step", "--upsample", "bilinear"], ["kernel"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    # the generator's two upsampling layers at 256x256 inputs
    assert mod.LAYER_SHAPES == ((256, 128, 64), (128, 64, 128))
    assert set(mod._forms()) == {"folded", "transpose", "unfused"}
