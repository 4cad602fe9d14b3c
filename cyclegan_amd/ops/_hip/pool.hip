// Image history pool exchange — gfx950.
//
// The CycleGAN history buffer (Zhu et al. 2017, §4): the discriminators
// see a mix of fresh fakes and fakes of earlier steps kept in a pool of P
// images. One launch applies a batch of host-drawn decisions:
//
//   codes[b] == -1        pass:  out[b] = fake[b]
//   codes[b] == s <  P    swap:  out[b] = pool[s];  pool[s] = fake[b]
//   codes[b] == P + s     fill:  pool[s] = fake[b]; out[b] = fake[b]
//
// in batch order: if two elements name one slot, the second sees what the
// first stored.
//
// Mapping: an image is a run of N units; a thread owns ONE unit position v
// and walks b = 0..B-1 itself. Every address the launch touches
// (fake[b][v], out[b][v], pool[s][v]) belongs to the thread that owns v,
// so the batch order is plain program order of that thread: no atomics,
// no barriers, no second launch, and no hazard between blocks.
//
// The op only copies bytes. A unit is 16 bytes (one dwordx4 load/store per
// lane, 1 KiB contiguous per wave) when the per-image byte count is a
// multiple of 16 and pool, fake and out are 16-byte aligned; otherwise a
// unit is one element (1/2/4/8 bytes). At 256x256x3 bf16 that is 24 576
// threads moving at most 4 x 393 KB per element.
//
// The kernel trusts codes: a bad value would be an out-of-range access.
// Their range is validated on the host where they are built (ops/pool.py).

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

namespace cyg {

constexpr int POOL_NT = 256;

// pool and out are written and may be read back by the same thread: no
// __restrict__ on them
template <typename U>
__global__ __launch_bounds__(POOL_NT) void pool_exchange_kernel(
    U* pool, const U* __restrict__ fake, const int* __restrict__ codes,
    U* out, int B, int P, long N) {
  const long v = (long)blockIdx.x * POOL_NT + threadIdx.x;
  if (v >= N) return;
  for (int b = 0; b < B; ++b) {
    const int code = codes[b];  // wave-uniform
    U val = fake[(long)b * N + v];
    if (code >= 0) {
      const bool swap = code < P;
      U* slot = pool + (long)(swap ? code : code - P) * N + v;
      U fresh = val;
      if (swap) val = *slot;
      *slot = fresh;
    }
    out[(long)b * N + v] = val;
  }
}

template <typename U>
static void pool_launch(at::Tensor& pool, const at::Tensor& fake,
                        const at::Tensor& codes, at::Tensor& out,
                        long image_bytes) {
  const long N = image_bytes / (long)sizeof(U);
  const long blocks = (N + POOL_NT - 1) / POOL_NT;
  TORCH_CHECK(blocks <= 0x7fffffffL, "pool_exchange: image too large");
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL((pool_exchange_kernel<U>), dim3((unsigned)blocks),
                     dim3(POOL_NT), 0, stream, (U*)pool.mutable_data_ptr(),
                     (const U*)fake.const_data_ptr(),
                     (const int*)codes.const_data_ptr(),
                     (U*)out.mutable_data_ptr(), (int)fake.size(0),
                     (int)pool.size(0), N);
}

at::Tensor pool_exchange(at::Tensor pool, at::Tensor fake, at::Tensor codes,
                         at::Tensor out) {
  TORCH_CHECK(pool.is_cuda() && pool.is_contiguous() && pool.dim() == 4,
              "pool_exchange: pool must be a contiguous cuda [P,H,W,C]");
  TORCH_CHECK(fake.is_cuda() && fake.is_contiguous() && fake.dim() == 4,
              "pool_exchange: fake must be a contiguous cuda [B,H,W,C]");
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.dim() == 4,
              "pool_exchange: out must be a contiguous cuda [B,H,W,C]");
  TORCH_CHECK(codes.is_cuda() && codes.scalar_type() == at::kInt &&
              codes.is_contiguous() && codes.dim() == 1 &&
              codes.size(0) == fake.size(0),
              "pool_exchange: codes must be a contiguous cuda int32 [B]");
  TORCH_CHECK(fake.scalar_type() == pool.scalar_type() &&
              out.scalar_type() == pool.scalar_type(),
              "pool_exchange: pool, fake and out must share one dtype");
  TORCH_CHECK(out.sizes() == fake.sizes(),
              "pool_exchange: out must have the shape of fake");
  for (int d = 1; d < 4; ++d)
    TORCH_CHECK(pool.size(d) == fake.size(d),
                "pool_exchange: pool and fake image shapes differ");
  TORCH_CHECK(pool.get_device() == fake.get_device() &&
              pool.get_device() == out.get_device() &&
              pool.get_device() == codes.get_device(),
              "pool_exchange: tensors on different devices");
  TORCH_CHECK(pool.size(0) >= 1 && pool.size(0) <= 0x3fffffffL &&
              fake.size(0) <= 0x7fffffffL,
              "pool_exchange: pool size or batch out of range");
  const long esz = (long)pool.element_size();
  const long image_bytes = (long)(pool.numel() / pool.size(0)) * esz;
  const long nbytes = (long)fake.numel() * esz;
  if (nbytes == 0) return out;  // B == 0 or an empty image
  // the walk is only ordered per address: the three buffers must not overlap
  auto lo = [](const at::Tensor& t) { return (uintptr_t)t.const_data_ptr(); };
  auto apart = [&](const at::Tensor& a, long na, const at::Tensor& b, long nb) {
    return lo(a) + na <= lo(b) || lo(b) + nb <= lo(a);
  };
  const long pbytes = (long)pool.numel() * esz;
  TORCH_CHECK(apart(pool, pbytes, fake, nbytes) &&
              apart(pool, pbytes, out, nbytes) &&
              apart(fake, nbytes, out, nbytes),
              "pool_exchange: pool, fake and out must not overlap");
  const bool vec = image_bytes % 16 == 0 && lo(pool) % 16 == 0 &&
                   lo(fake) % 16 == 0 && lo(out) % 16 == 0;
  if (vec) {
    pool_launch<uint4>(pool, fake, codes, out, image_bytes);
  } else {
    switch (esz) {
      case 1: pool_launch<unsigned char>(pool, fake, codes, out, image_bytes); break;
      case 2: pool_launch<unsigned short>(pool, fake, codes, out, image_bytes); break;
      case 4: pool_launch<unsigned int>(pool, fake, codes, out, image_bytes); break;
      case 8: pool_launch<unsigned long>(pool, fake, codes, out, image_bytes); break;
      default:
        TORCH_CHECK(false, "pool_exchange: unsupported element size ", esz);
    }
  }
  return out;
}

}  // namespace cyg
