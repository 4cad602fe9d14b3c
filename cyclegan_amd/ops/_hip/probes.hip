// Instruction-semantics probes (test and tool aids, never on a hot path):
// one-wave kernels that dump what a gfx950 instruction actually does, so
// the fragment layouts the conv kernels rely on are measured, not assumed.
//   glds_probe   raw_ptr_buffer_load_lds lane->LDS placement and OOB zeros
//   tr_probe     ds_read_b64_tr_b16 lane->element mapping
//   mx_probe     mfma_scale_f32_32x32x64_f8f6f4 raw operand dump
//   mx_probe16   mfma_scale_f32_16x16x128_f8f6f4 raw operand dump
//   mfma_probe   mfma_f32_16x16x32_bf16 fragment layout

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

namespace cyg {

// ---- glds probe (test aid): verify raw_ptr_buffer_load_lds semantics ----
// lane l loads 16B from x at voff[l]; expect LDS dest = base + l*16 and
// OOB voffsets to produce zeros.
__global__ void glds_probe_kernel(const float* x, const unsigned* voff,
                                  int nbytes, float* out) {
  __shared__ float lds[128];
  int l = threadIdx.x;  // 64 threads
  lds[l] = -1.f; lds[64 + l] = -1.f;
  __syncthreads();
  auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, nbytes, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(
      rsrc, (__attribute__((address_space(3))) void*)&lds[0], 16, voff[l], 0,
      0, 0);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  out[l] = lds[l];
  out[64 + l] = lds[64 + l];
}

at::Tensor glds_probe(at::Tensor x, at::Tensor voff) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat);
  TORCH_CHECK(voff.scalar_type() == at::kInt && voff.numel() == 64);
  auto out = at::empty({128}, x.options());
  hipLaunchKernelGGL(glds_probe_kernel, dim3(1), dim3(64), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const float*)x.const_data_ptr(),
                     (const unsigned*)voff.const_data_ptr(),
                     (int)(x.numel() * 4), (float*)out.mutable_data_ptr());
  return out;
}

// ---- ds_read_b64_tr_b16 probe: identity-filled LDS, per-lane address by
// mode; out[l*4+j] = LDS element index that lane l's element j received.
typedef bf16r v4bf __attribute__((ext_vector_type(4)));
typedef short v4sh __attribute__((ext_vector_type(4)));
__global__ void tr_probe_kernel(short* out, int mode) {
  __shared__ short lds[1024];
  int l = threadIdx.x;
  for (int i = l; i < 1024; i += 64) lds[i] = (short)i;
  __syncthreads();
  int addr;
  switch (mode) {
    case 0: addr = (l & 15) + (l >> 4) * 64; break;
    case 1: addr = 0; break;
    case 2: addr = l * 4; break;
    default: addr = (l & 15) * 2 + (l >> 4) * 64; break;
  }
  auto p = (__attribute__((address_space(3))) v4bf*)(
      (__attribute__((address_space(3))) short*)lds + addr);
  v4bf r = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(p);
  #pragma unroll
  for (int j = 0; j < 4; ++j) out[l * 4 + j] = ((v4sh&)r)[j];
}

at::Tensor tr_probe(int64_t mode) {
  auto out = at::empty({256}, at::TensorOptions().dtype(at::kShort).device(at::kCUDA));
  hipLaunchKernelGGL(tr_probe_kernel, dim3(1), dim3(64), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (short*)out.mutable_data_ptr(), (int)mode);
  return out;
}

// ---- MX-scaled fp8 MFMA probe: raw per-lane operand dump for
// mapping the 32x32x64 f8f6f4 fragment layout empirically, exactly how
// mfma_probe established the bf16 16x16x32 layout. Operands are the raw
// 32 bytes each lane supplies (a/b as [64][8] int32); scale operands use
// cbsz/blgp = 0 (e4m3 A and B) and a single scale byte broadcast.
typedef int v8i_ __attribute__((ext_vector_type(8)));
typedef float v16f_ __attribute__((ext_vector_type(16)));
__global__ void mx_probe_kernel(const int* a, const int* b, float* d,
                                int sa, int sb) {
  int lane = threadIdx.x & 63;
  v8i_ av = *(const v8i_*)(a + lane * 8);
  v8i_ bv = *(const v8i_*)(b + lane * 8);
  v16f_ acc = {};
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
      av, bv, acc, 0, 0, 0, sa, 0, sb);
  #pragma unroll
  for (int r = 0; r < 16; ++r) d[lane * 16 + r] = acc[r];
}

// 16x16x128 scaled-fp8 probe: same raw per-lane operand dump for the
// D[16,16] = A[16,128] @ B[128,16] fragment (v4f acc).
__global__ void mx_probe16_kernel(const int* a, const int* b, float* d,
                                  int sa, int sb) {
  int lane = threadIdx.x & 63;
  v8i_ av = *(const v8i_*)(a + lane * 8);
  v8i_ bv = *(const v8i_*)(b + lane * 8);
  v4f acc = {};
  acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
      av, bv, acc, 0, 0, 0, sa, 0, sb);
  #pragma unroll
  for (int r = 0; r < 4; ++r) d[lane * 4 + r] = acc[r];
}

at::Tensor mx_probe16(at::Tensor a, at::Tensor b, int64_t sa, int64_t sb) {
  TORCH_CHECK(a.is_cuda() && a.scalar_type() == at::kInt &&
              a.sizes() == at::IntArrayRef({64, 8}) &&
              b.sizes() == at::IntArrayRef({64, 8}));
  auto d = at::empty({64, 4}, a.options().dtype(at::kFloat));
  hipLaunchKernelGGL(mx_probe16_kernel, dim3(1), dim3(64), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const int*)a.contiguous().const_data_ptr(),
                     (const int*)b.contiguous().const_data_ptr(),
                     (float*)d.mutable_data_ptr(), (int)sa, (int)sb);
  return d;
}

at::Tensor mx_probe(at::Tensor a, at::Tensor b, int64_t sa, int64_t sb) {
  TORCH_CHECK(a.is_cuda() && a.scalar_type() == at::kInt &&
              a.sizes() == at::IntArrayRef({64, 8}) &&
              b.sizes() == at::IntArrayRef({64, 8}));
  auto d = at::empty({64, 16}, a.options().dtype(at::kFloat));
  hipLaunchKernelGGL(mx_probe_kernel, dim3(1), dim3(64), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const int*)a.contiguous().const_data_ptr(),
                     (const int*)b.contiguous().const_data_ptr(),
                     (float*)d.mutable_data_ptr(), (int)sa, (int)sb);
  return d;
}

// ---- MFMA layout probe (test aid): C[16,16] = A[16,32] @ Bt[16,32]^T ----
__global__ void mfma_probe_kernel(const short* a, const short* bt, float* c) {
  int lane = threadIdx.x & 63;
  int fr = lane & 15, fg = lane >> 4;
  v8bf av = *(const v8bf*)(a + fr * 32 + fg * 8);
  v8bf bv = *(const v8bf*)(bt + fr * 32 + fg * 8);
  v4f d = {};
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, d, 0, 0, 0);
  #pragma unroll
  for (int r = 0; r < 4; ++r) c[(fg * 4 + r) * 16 + fr] = d[r];
}

at::Tensor mfma_probe(at::Tensor a, at::Tensor bt) {
  TORCH_CHECK(a.sizes() == at::IntArrayRef({16, 32}) &&
              bt.sizes() == at::IntArrayRef({16, 32}));
  auto c = at::empty({16, 16}, a.options().dtype(at::kFloat));
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const short*)a.contiguous().const_data_ptr(),
                     (const short*)bt.contiguous().const_data_ptr(),
                     (float*)c.mutable_data_ptr());
  return c;
}

}  // namespace cyg
