"""fp8 microbenchmarks at train batch sizes (GPU box).

    python tools/fp8_micro.py                 # fp8-vs-bf16 per-shape A/B
    python tools/fp8_micro.py norm_quant      # instnorm_fwd + quant_fp8_d
                                              #   vs instnorm_fwd_q8
    python tools/fp8_micro.py conv_stats      # conv2d_fp8_fwd + reduce-route
                                              #   norm vs conv2d_fp8_fwd_stats
                                              #   + slab-route norm
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cyclegan_amd.ops import backend

e = backend.ext()
DEV = "cuda:0"
torch.manual_seed(0)


def timeit(fn, iters=30, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    t = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    t.record()
    torch.cuda.synchronize()
    return s.elapsed_time(t) / iters * 1000


def mk(*shape):
    return (torch.rand(*shape, device=DEV, dtype=torch.bfloat16) - 0.5)


sx = torch.tensor([1.0], device=DEV)
ap = torch.tensor([0.5], device=DEV)
ac = torch.zeros(1, device=DEV)


def dispatch_ab():
    for B in (4, 8, 12):
        x = mk(B, 64, 64, 256)
        w = mk(256, 3, 3, 256) * 0.1
        fl = 2 * (B * 64 * 64) * 256 * 2304
        us_bf = timeit(lambda: e.conv2d_fwd(x, w, None, 1, 1, 1, 1, 1, True, 0, 0.2))
        xq = e.quant_fp8(x, sx)
        wq = e.quant_fp8(w, sx)
        us_f8 = timeit(lambda: e.conv2d_fp8_fwd(xq, wq, sx, None, None, 1, 1, 1, 1, 1, True, 0, 0.2))
        us_q = timeit(lambda: e.quant_fp8_d(x, ap, ac))
        print(f"K3 B={B:2d}: bf16 {us_bf:7.1f}us ({fl/us_bf/1e6:.0f} TF/s)  "
              f"fp8 {us_f8:7.1f}us ({fl/us_f8/1e6:.0f} TF/s)  quant {us_q:6.1f}us  "
              f"fp8+q vs bf16: {us_f8+us_q-us_bf:+7.1f}us")

    # down conv 3x3 s2 at train batch
    for B in (8, 12):
        x = mk(B, 128, 128, 128)
        w = mk(256, 3, 3, 128) * 0.1
        fl = 2 * (B * 64 * 64) * 256 * (9 * 128)
        us_bf = timeit(lambda: e.conv2d_fwd(x, w, None, 2, 0, 1, 0, 1, False, 0, 0.2))
        xq = e.quant_fp8(x, sx)
        wq = e.quant_fp8(w, sx)
        us_f8 = timeit(lambda: e.conv2d_fp8_fwd(xq, wq, sx, None, None, 2, 0, 1, 0, 1, False, 0, 0.2))
        us_q = timeit(lambda: e.quant_fp8_d(x, ap, ac))
        print(f"down B={B:2d}: bf16 {us_bf:7.1f}us  fp8 {us_f8:7.1f}us  quant {us_q:6.1f}us  "
              f"fp8+q vs bf16: {us_f8+us_q-us_bf:+7.1f}us")

    # disc 4x4 s2 256->512-ish wide at 32^2 (s1) and 64^2 (s2)
    for name, B, H, Cin, Cout, K, s, pads in (
            ("D_wide", 4, 32, 256, 512, 4, 1, (1, 2, 1, 2)),
            ("D_down2", 4, 64, 128, 256, 4, 2, (1, 2, 1, 2))):
        x = mk(B, H, H, Cin)
        w = mk(Cout, K, K, Cin) * 0.1
        OH = (H + pads[0] + pads[1] - K) // s + 1
        fl = 2 * (B * OH * OH) * Cout * (K * K * Cin)
        us_bf = timeit(lambda: e.conv2d_fwd(x, w, None, s, *pads, False, 0, 0.2))
        xq = e.quant_fp8(x, sx)
        wq = e.quant_fp8(w, sx)
        us_f8 = timeit(lambda: e.conv2d_fp8_fwd(xq, wq, sx, None, None, s, *pads, False, 0, 0.2))
        us_q = timeit(lambda: e.quant_fp8_d(x, ap, ac))
        print(f"{name} B={B}: bf16 {us_bf:7.1f}us  fp8 {us_f8:7.1f}us  quant {us_q:6.1f}us  "
              f"fp8+q vs bf16: {us_f8+us_q-us_bf:+7.1f}us")


# the two fused shapes: K3 resblock conv at conv batch 12 (its input is a
# 64x64x256 norm output) and the 4x4 s1 256->512 discriminator conv at the
# bench's batch-4 discriminator call (32x32x256 in, 32x32x512 out)
FUSED_SHAPES = (
    # name, B, H, Cin, Cout, K, pads, reflect, norm act
    ("K3 B=12", 12, 64, 256, 256, 3, (1, 1, 1, 1), True, 1),
    ("D 4x4s1 B=4", 4, 32, 256, 512, 4, (1, 2, 1, 2), False, 2),
)


def norm_quant():
    """The producer side: a norm then a standalone quant of its output,
    against the norm that writes the fp8 twin itself."""
    for name, B, H, Cin, _, _, _, _, act in FUSED_SHAPES:
        x = mk(B, H, H, Cin)
        g = torch.rand(Cin, device=DEV) + 0.5
        b = torch.zeros(Cin, device=DEV)
        us_n = timeit(lambda: e.instnorm_fwd(x, g, b, 1e-3, act, 0.2, None))
        y = e.instnorm_fwd(x, g, b, 1e-3, act, 0.2, None)[0]
        us_q = timeit(lambda: e.quant_fp8_d(y, ap, ac))
        us_f = timeit(lambda: e.instnorm_fwd_q8(x, g, b, 1e-3, act, 0.2, None,
                                                None, None, 0, ap, ac))
        print(f"{name}: instnorm_fwd {us_n:6.1f}us + quant_fp8_d {us_q:6.1f}us"
              f" = {us_n+us_q:6.1f}us   instnorm_fwd_q8 {us_f:6.1f}us"
              f"   saved {us_n+us_q-us_f:+6.1f}us")


def conv_stats():
    """The consumer side: fp8 conv then a norm that reduces its own
    statistics, against the fp8 conv with the slab epilogue and the norm
    on the slab route."""
    for name, B, H, Cin, Cout, K, pads, reflect, act in FUSED_SHAPES:
        x = mk(B, H, H, Cin)
        w = mk(Cout, K, K, Cin) * 0.1
        xq = e.quant_fp8(x, sx)
        wq = e.quant_fp8(w, sx)
        g = torch.rand(Cout, device=DEV) + 0.5
        b = torch.zeros(Cout, device=DEV)
        args = (xq, wq, sx, None, None, 1, *pads, reflect, 0, 0.2)
        us_c = timeit(lambda: e.conv2d_fp8_fwd(*args))
        h = e.conv2d_fp8_fwd(*args)
        us_n = timeit(lambda: e.instnorm_fwd(h, g, b, 1e-3, act, 0.2, None))
        out = e.conv2d_fp8_fwd_stats(*args)
        if len(out) != 3:
            print(f"{name}: not eligible for epilogue slabs")
            continue
        us_cs = timeit(lambda: e.conv2d_fp8_fwd_stats(*args))
        _, ps, pq = out
        us_ns = timeit(lambda: e.instnorm_fwd(h, g, b, 1e-3, act, 0.2, None,
                                              ps, pq, ps.shape[0]))
        print(f"{name}: conv {us_c:6.1f}us + norm(reduce) {us_n:6.1f}us"
              f" = {us_c+us_n:6.1f}us   conv_stats {us_cs:6.1f}us +"
              f" norm(slabs) {us_ns:6.1f}us = {us_cs+us_ns:6.1f}us"
              f"   saved {us_c+us_n-us_cs-us_ns:+6.1f}us")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "dispatch"
    {"dispatch": dispatch_ab, "norm_quant": norm_quant,
     "conv_stats": conv_stats}[mode]()
