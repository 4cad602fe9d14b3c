// Shadow-arena refresh kernels — gfx950.
//
// The gather: one launch builds bf16 compute-shadow forms of a model group
// (padded OHWI forward weights, channel-transposed dgrad weights, padded
// biases) from the group's flat fp32 master buffer. Replaces the ~180
// per-step ATen pad/cast/permute launches of the per-tensor shadow cache
// (the reference hides the equivalent work inside TF variable reads,
// /root/reference/main.py:207-262; MI355X-native form is one indexed
// gather at HBM speed). With the Adam-written mirror (below) it keeps only
// the forms that are neither a view of the mirror nor a plain transpose.
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

// ---- mirror: the bf16 image of the whole flat buffer ----
//
// The fused Adam kernels write it while p_new is in a register (SHADOW in
// norm_elem.hip); this cast fills it when the masters change any other way
// (construction, checkpoint load, a state roll-back, the EMA exchange).
// out[i] = bf16(src[i]), i < n: 8 per thread, then a scalar tail of n % 8.
__global__ __launch_bounds__(SG_NT) void shadow_cast_kernel(
    const float* __restrict__ src, short* __restrict__ out, long n) {
  const long tid = (long)blockIdx.x * SG_NT + threadIdx.x;
  const long stride = (long)gridDim.x * SG_NT;
  const long n8 = n >> 3;
  for (long t = tid; t < n8; t += stride) {
    v4f a = *(const v4f*)(src + t * 8);
    v4f b = *(const v4f*)(src + t * 8 + 4);
    v8s o = {f2b(a[0]), f2b(a[1]), f2b(a[2]), f2b(a[3]),
             f2b(b[0]), f2b(b[1]), f2b(b[2]), f2b(b[3])};
    *(v8s*)(out + t * 8) = o;
  }
  for (long i = (n8 << 3) + tid; i < n; i += stride) out[i] = f2b(src[i]);
}

void shadow_cast(at::Tensor src, at::Tensor out) {
  TORCH_CHECK(src.is_cuda() && src.scalar_type() == at::kFloat &&
              src.is_contiguous());
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kBFloat16 &&
              out.is_contiguous() && out.device() == src.device());
  TORCH_CHECK(out.numel() >= src.numel(), "shadow_cast: out too short");
  TORCH_CHECK(((reinterpret_cast<uintptr_t>(src.const_data_ptr()) |
                reinterpret_cast<uintptr_t>(out.const_data_ptr())) & 15) == 0,
              "shadow_cast: 16-byte aligned buffers only");
  long n = src.numel();
  if (n == 0) return;
  long work = std::max<long>(n >> 3, n & 7);
  int blocks = (int)min((long)4096, (work + SG_NT - 1) / SG_NT);
  hipLaunchKernelGGL(shadow_cast_kernel, dim3(blocks), dim3(SG_NT), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const float*)src.const_data_ptr(),
                     (short*)out.mutable_data_ptr(), n);
}

// ---- index-free transposes of the dgrad forms ----
//
// dgrad reads a conv weight channel-transposed: [Cout,taps,Cin] (OHWI, taps
// = KH*KW) -> [Cin,taps,Cout]. One launch does every eligible layer of a
// group from a table, one row of ST_COLS int32 per layer:
//   {src offset (in the mirror), dst offset, Cout, taps, Cin,
//    first block, tiles along Cin, tiles along Cout}
// Offsets and channel counts are multiples of 8 (checked by the host), so
// every global access is a whole 16-byte word. A block moves one
// ST_T x ST_T (co x ci) tile of one tap: rows of 8 lanes load 128
// contiguous bytes of a [co] row, scatter them transposed into LDS, and
// rows of 8 lanes store 128 contiguous bytes of a [ci] row.
constexpr int ST_COLS = 8;
constexpr int ST_T = 64;
constexpr int ST_LD = ST_T + 8;  // LDS row pitch: keeps 16-byte alignment

__global__ __launch_bounds__(SG_NT) void shadow_transpose_kernel(
    const short* __restrict__ src, const int* __restrict__ table, int rows,
    short* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) short tile[ST_T * ST_LD];
  const int blk = blockIdx.x;
  // the row this block belongs to: the last one whose first block <= blk
  int r = 0;
  while (r + 1 < rows && table[(r + 1) * ST_COLS + 5] <= blk) ++r;
  const int* row = table + r * ST_COLS;
  const long src_off = row[0], dst_off = row[1];
  const int Cout = row[2], taps = row[3], Cin = row[4];
  const int tci = row[6], tco = row[7];
  int local = blk - row[5];
  const int ci0 = (local % tci) * ST_T;
  local /= tci;
  const int co0 = (local % tco) * ST_T;
  const int tap = local / tco;
  if (tap >= taps) return;  // whole block: nothing reaches the barrier

  // ST_T rows of ST_T/8 16-byte words = 512 words, two per thread
  #pragma unroll
  for (int k = 0; k < (ST_T * ST_T / 8) / SG_NT; ++k) {
    const int w = threadIdx.x + k * SG_NT;
    const int co = co0 + w / (ST_T / 8);
    const int cw = (w % (ST_T / 8)) * 8;  // first ci of this word, in tile
    if (co < Cout && ci0 + cw < Cin) {
      v8s x = *(const v8s*)(src + src_off +
                            ((long)co * taps + tap) * Cin + ci0 + cw);
      #pragma unroll
      for (int j = 0; j < 8; ++j) tile[(cw + j) * ST_LD + (co - co0)] = x[j];
    }
  }
  __syncthreads();
  #pragma unroll
  for (int k = 0; k < (ST_T * ST_T / 8) / SG_NT; ++k) {
    const int w = threadIdx.x + k * SG_NT;
    const int ci = ci0 + w / (ST_T / 8);
    const int cw = (w % (ST_T / 8)) * 8;  // first co of this word, in tile
    if (ci < Cin && co0 + cw < Cout) {
      v8s x = *(const v8s*)(tile + (ci - ci0) * ST_LD + cw);
      *(v8s*)(dst + dst_off + ((long)ci * taps + tap) * Cout + co0 + cw) = x;
    }
  }
}

// table: the rows on the host (int32 [L, ST_COLS]); table_dev: the same on
// the device. Every call re-checks the host copy against both buffers, so
// a stale or hand-made table cannot send the kernel out of bounds.
void shadow_transpose(at::Tensor src, at::Tensor table, at::Tensor table_dev,
                      at::Tensor dst) {
  TORCH_CHECK(src.is_cuda() && src.scalar_type() == at::kBFloat16 &&
              src.is_contiguous());
  TORCH_CHECK(dst.is_cuda() && dst.scalar_type() == at::kBFloat16 &&
              dst.is_contiguous() && dst.device() == src.device());
  TORCH_CHECK(!table.is_cuda() && table.scalar_type() == at::kInt &&
              table.is_contiguous() && table.dim() == 2 &&
              table.size(1) == ST_COLS);
  TORCH_CHECK(table_dev.is_cuda() && table_dev.device() == src.device() &&
              table_dev.scalar_type() == at::kInt &&
              table_dev.is_contiguous() &&
              table_dev.sizes() == table.sizes());
  TORCH_CHECK(((reinterpret_cast<uintptr_t>(src.const_data_ptr()) |
                reinterpret_cast<uintptr_t>(dst.const_data_ptr())) & 15) == 0,
              "shadow_transpose: 16-byte aligned buffers only");
  const int rows = (int)table.size(0);
  if (rows == 0) return;
  const int* t = (const int*)table.const_data_ptr();
  long blocks = 0;
  for (int r = 0; r < rows; ++r) {
    const int* row = t + r * ST_COLS;
    const long so = row[0], d_o = row[1], Cout = row[2], taps = row[3],
               Cin = row[4];
    TORCH_CHECK(Cout > 0 && taps > 0 && Cin > 0 && Cout % 8 == 0 &&
                    Cin % 8 == 0 && so >= 0 && d_o >= 0 && so % 8 == 0 &&
                    d_o % 8 == 0,
                "shadow_transpose: row ", r, " is not eligible");
    const long n = Cout * taps * Cin;
    TORCH_CHECK(so + n <= src.numel() && d_o + n <= dst.numel(),
                "shadow_transpose: row ", r, " out of bounds");
    const long tci = (Cin + ST_T - 1) / ST_T, tco = (Cout + ST_T - 1) / ST_T;
    TORCH_CHECK(row[5] == blocks && row[6] == tci && row[7] == tco,
                "shadow_transpose: row ", r, " has a wrong block layout");
    blocks += taps * tci * tco;
  }
  TORCH_CHECK(blocks < (1L << 31));
  hipLaunchKernelGGL(shadow_transpose_kernel, dim3((unsigned)blocks),
                     dim3(SG_NT), 0, at::cuda::getCurrentCUDAStream(),
                     (const short*)src.const_data_ptr(),
                     (const int*)table_dev.const_data_ptr(), rows,
                     (short*)dst.mutable_data_ptr());
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
