// Shadow-arena gather — gfx950.
//
// One launch refreshes EVERY bf16 compute-shadow form of a model group
// (padded OHWI forward weights, channel-transposed dgrad weights, padded
// biases) from the group's flat fp32 master buffer. Replaces the ~180
// per-step ATen pad/cast/permute launches of the per-tensor shadow cache
// (the reference hides the equivalent work inside TF variable reads,
// /root/reference/main.py:207-262; MI355X-native form is one indexed
// gather at HBM speed).
//
// out[i] = idx[i] >= 0 ? bf16(src[idx[i]]) : 0
// n is padded to a multiple of 8 by the Python side (idx pad = -1).

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

namespace cyg {

constexpr int SG_NT = 256;

typedef int v8i __attribute__((ext_vector_type(8)));

__global__ __launch_bounds__(SG_NT) void shadow_gather_kernel(
    const float* __restrict__ src, const int* __restrict__ idx,
    short* __restrict__ out, long n8) {
  long t = (long)blockIdx.x * SG_NT + threadIdx.x;
  long stride = (long)gridDim.x * SG_NT;
  for (; t < n8; t += stride) {
    v8i ix = *(const v8i*)(idx + t * 8);
    v8s o;
    #pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = ix[j] >= 0 ? f2b(src[ix[j]]) : (short)0;
    *(v8s*)(out + t * 8) = o;
  }
}

void shadow_gather(at::Tensor src, at::Tensor idx, at::Tensor out) {
  TORCH_CHECK(src.is_cuda() && src.scalar_type() == at::kFloat &&
              src.is_contiguous());
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kInt &&
              idx.is_contiguous());
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kBFloat16 &&
              out.is_contiguous());
  TORCH_CHECK(idx.numel() == out.numel() && idx.numel() % 8 == 0);
  long n8 = idx.numel() / 8;
  int blocks = (int)min((long)4096, (n8 + SG_NT - 1) / SG_NT);
  hipLaunchKernelGGL(shadow_gather_kernel, dim3(blocks), dim3(SG_NT), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const float*)src.const_data_ptr(),
                     (const int*)idx.const_data_ptr(),
                     (short*)out.mutable_data_ptr(), n8);
}

// ---- folded forms (resize-convolution, ops.conv._UpConvFn) ----
//
// nearest-2x upsample + zero-padded 3x3 conv == 4x4 stride-2 'SAME'
// transpose conv whose kernel is V = M w M^T per axis pair, M =
// [[0,0,1],[0,1,1],[1,1,0],[1,0,0]]: every folded element is the sum of at
// most four masters. The Python side (ops.arena) lays the sums out as an
// [n,4] index table, -1 for an absent term.
//
// out[i] = bf16( Σ_{j<4, idx4[i][j] >= 0} src[idx4[i][j]] ), fp32 sum in the
// order j = 0..3; n is a multiple of 8 (pad rows are all -1 -> exact zero).
typedef int v4i __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(SG_NT) void shadow_fold_kernel(
    const float* __restrict__ src, const int* __restrict__ idx4,
    short* __restrict__ out, long n8) {
  long t = (long)blockIdx.x * SG_NT + threadIdx.x;
  long stride = (long)gridDim.x * SG_NT;
  for (; t < n8; t += stride) {
    v8s o;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      v4i ix = *(const v4i*)(idx4 + (t * 8 + j) * 4);
      float s = 0.f;
      #pragma unroll
      for (int q = 0; q < 4; ++q)
        if (ix[q] >= 0) s += src[ix[q]];
      o[j] = f2b(s);
    }
    *(v8s*)(out + t * 8) = o;
  }
}

void shadow_fold(at::Tensor src, at::Tensor idx4, at::Tensor out) {
  TORCH_CHECK(src.is_cuda() && src.scalar_type() == at::kFloat &&
              src.is_contiguous());
  TORCH_CHECK(idx4.is_cuda() && idx4.scalar_type() == at::kInt &&
              idx4.is_contiguous() && idx4.dim() == 2 && idx4.size(1) == 4);
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kBFloat16 &&
              out.is_contiguous());
  TORCH_CHECK(idx4.size(0) == out.numel() && out.numel() % 8 == 0);
  long n8 = out.numel() / 8;
  if (n8 == 0) return;
  int blocks = (int)min((long)4096, (n8 + SG_NT - 1) / SG_NT);
  hipLaunchKernelGGL(shadow_fold_kernel, dim3(blocks), dim3(SG_NT), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const float*)src.const_data_ptr(),
                     (const int*)idx4.const_data_ptr(),
                     (short*)out.mutable_data_ptr(), n8);
}

// Gradient unfold, the adjoint of the fold above:
// dw[co,d,e,ci] = Σ_{k in {2-d,3-d}} Σ_{l in {2-e,3-e}} dV[co,k,l,ci]
// (the k with M[k][d] = 1), four fp32 terms in (k,l) ascending order. One
// thread per element of out, every element written. tr: dv is laid out
// [Cin,4,4,Cout], as the role-swapped wgrad of a transpose conv returns it.
__global__ void fold_upconv_dw_kernel(const float* __restrict__ dv,
                                      float* __restrict__ out, int O, int I,
                                      int tr, int accum) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)O * 9 * I;
  if (idx >= total) return;
  int ci = (int)(idx % I);
  long t = idx / I;
  int e = (int)(t % 3);
  t /= 3;
  int d = (int)(t % 3);
  int co = (int)(t / 3);
  float s = 0.f;
  #pragma unroll
  for (int a = 0; a < 2; ++a) {
    #pragma unroll
    for (int b = 0; b < 2; ++b) {
      int tap = (2 - d + a) * 4 + (2 - e + b);
      s += tr ? dv[((long)ci * 16 + tap) * O + co]
              : dv[((long)co * 16 + tap) * I + ci];
    }
  }
  out[idx] = accum ? out[idx] + s : s;
}

void fold_upconv_dw_into(at::Tensor dv, at::Tensor out, bool accumulate,
                         bool transposed) {
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kFloat &&
                  out.is_contiguous(),
              "fold_upconv_dw_into: out must be a contiguous fp32 device "
              "tensor");
  TORCH_CHECK(dv.is_cuda() && dv.scalar_type() == at::kFloat &&
              dv.is_contiguous() && dv.dim() == 4 && out.dim() == 4);
  const int64_t O = out.size(0), I = out.size(3);
  TORCH_CHECK(out.size(1) == 3 && out.size(2) == 3 && dv.size(1) == 4 &&
                  dv.size(2) == 4 && dv.size(0) == (transposed ? I : O) &&
                  dv.size(3) == (transposed ? O : I),
              "fold_upconv_dw_into: shape mismatch");
  long total = out.numel();
  if (total == 0) return;
  hipLaunchKernelGGL(fold_upconv_dw_kernel, dim3((total + 255) / 256),
                     dim3(256), 0, at::cuda::getCurrentCUDAStream(),
                     (const float*)dv.const_data_ptr(),
                     (float*)out.mutable_data_ptr(), (int)O, (int)I,
                     transposed ? 1 : 0, accumulate ? 1 : 0);
}

}  // namespace cyg
