"""augment_batch-only microbench at the workload shape (B=4, bf16, 256x256
sources resized to 286 and cropped to 256), for focused rocprofv3
--kernel-trace --stats runs: 20 warm-up + 500 launches over rotating
indices of a 256-image device-resident dataset."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cyclegan_amd.ops.augment import augment_batch, make_idx, make_params
dev = torch.device("cuda", 0)
g = torch.Generator().manual_seed(0)
N, B, resize, crop = 256, 4, (286, 286), (256, 256)
src = torch.randint(0, 256, (N, 256, 256, 3), generator=g,
                    dtype=torch.uint8).to(dev)
p = torch.stack([torch.randint(0, 2, (N,), generator=g),
                 torch.randint(0, 31, (N,), generator=g),
                 torch.randint(0, 31, (N,), generator=g)], 1)
params = make_params(p, resize, crop, dev)
order = make_idx(torch.randperm(N, generator=g), N, dev)
out = torch.empty(B, 256, 256, 3, dtype=torch.bfloat16, device=dev)
for i in range(520):
    lo = (i * B) % N
    augment_batch(src, order[lo:lo + B], params, resize, crop,
                  torch.bfloat16, out=out)
torch.cuda.synchronize()
# bytes the algorithm needs per launch: every output element written once,
# every source byte under the crop window read once
need = out.numel() * 2 + B * 3 * int(256 * 256 * (256 / 286) ** 2)
print("ok", tuple(out.shape), "bytes/launch", need)
