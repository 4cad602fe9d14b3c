// InstanceNorm (NHWC, fused act/residual), activation backward, reflection
// pad, per-sample losses, fused TF-Adam — gfx950.
//
// InstanceNorm strategy (channels innermost): threads cover whole C-rows
// with bf16x8 vector loads. Per-(b,c) statistics are fp32 slab partials
// psum/psq[(slice*B + b)*C + c] with no atomics (run-to-run
// deterministic): either in_reduce_kernel writes one slab per spatial
// slice, or the producing conv's epilogue writes one per 128-row M-tile
// (conv.hip) and in_reduce is skipped. Every block of the normalize pass
// sums the slabs in its prologue, then fuses affine + activation +
// residual add. Backward is two passes (slab partials, then dx); the
// relu/lrelu mask comes from the activated output or, when the caller
// passes beta instead, from x through the forward's own expression
// (in_affine).
// eps = 1e-3 semantics live in Python.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

namespace cyg {

constexpr int NT = 256;

static inline int cdiv64(long a, long b) { return (int)((a + b - 1) / b); }

// ---- pass 1: slab partials over spatial slices (no atomics) ----
// grid (B * S); writes psum/psq[(sl*B + b)*C + c]; C % 8 == 0, C/8 <= NT.
__global__ __launch_bounds__(NT) void in_reduce_kernel(
    const short* __restrict__ x, float* __restrict__ psum,
    float* __restrict__ psq, int B, long HW, int C, int S) {
  int b = blockIdx.x / S;
  int sl = blockIdx.x % S;
  long rows = (HW + S - 1) / S;
  long r0 = sl * rows, r1 = min(r0 + rows, HW);
  const int gpr = C / 8;              // 8-channel groups per row
  const int tid = threadIdx.x;
  const short* xb = x + (long)b * HW * C;

  int g = tid % gpr;
  int rstep = NT / gpr;
  int rof = tid / gpr;
  float s[8] = {}, q[8] = {};
  #pragma unroll 4
  for (long r = r0 + rof; r < r1; r += rstep) {
    v8s v = *(const v8s*)(xb + r * C + g * 8);
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = b2f(v[j]);
      s[j] += f; q[j] += f * f;
    }
  }
  // one-barrier reduce: every thread parks its 16 partials in LDS, then
  // C*2 output elements are summed in parallel.
  __shared__ float red[NT * 17];  // +1 pad: conflict-free strided reads
  #pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[tid * 17 + j] = s[j];
    red[tid * 17 + 8 + j] = q[j];
  }
  __syncthreads();
  long out = ((long)sl * B + b) * C;
  for (int o = tid; o < C * 2; o += NT) {
    int c = o % C;
    int issq = o / C;
    int g2 = c / 8, j = c % 8;
    float t = 0;
    for (int k = 0; k < rstep; ++k)
      t += red[(g2 + k * gpr) * 17 + issq * 8 + j];
    (issq ? psq : psum)[out + c] = t;
  }
}

// normalize + affine, pre-activation. ONE definition shared by the forward
// (in_norm) and by the backward's mask recompute, so both
// evaluate the same fp32 operations (sub, mul, fma) on the same saved
// mean/rstd: sign(in_affine) in backward == sign of what forward activated.
DEV float in_affine(float xv, float m, float rs, float g, float b) {
  return __fmaf_rn((xv - m) * rs, g, b);
}

// ---- pass 2 (fused): per-block slab-sum stats + normalize + affine +
// act (+ residual); slice-0 blocks also persist mean/rstd for backward.
// S slices the grid; NS is the number of slabs to sum (== S after
// in_reduce, HW/128 when the conv epilogue produced them) ----
//
// Q8 (compile-time, so the plain instantiation's row loop is untouched):
// the kernel also hands the consuming fp8 conv its operand. Every 16 B of
// bf16 it stores goes out a second time as 8 B of e4m3 in yq, quantised
// from the bf16-ROUNDED value with delayed_sx(amax_prev[0]) — the bytes
// quant_fp8_d would produce from y — and max|y| block-reduces into ONE
// atomicMax per block on amax_cur (grid B*S <= ~512 blocks; see the
// same-address-atomic note on quant_fp8_d_kernel).
constexpr int MAXC = 2048;
template <bool Q8>
__global__ __launch_bounds__(NT) void in_norm_kernel(
    const short* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ psum,
    const float* __restrict__ psq, float* __restrict__ mean,
    float* __restrict__ rstd, const short* __restrict__ res,
    short* __restrict__ y, int B, long HW, int C, int S, int NS, int act,
    float slope, float eps, unsigned char* __restrict__ yq,
    const float* __restrict__ amax_prev, float* __restrict__ amax_cur) {
  int b = blockIdx.x / S;
  int sl = blockIdx.x % S;
  long rows = (HW + S - 1) / S;
  long r0 = sl * rows, r1 = min(r0 + rows, HW);
  const int gpr = C / 8;
  const int tid = threadIdx.x;
  const long base = (long)b * HW * C;
  const float inv_hw = 1.f / (float)HW;

  __shared__ float sm[MAXC], sr[MAXC];
  __shared__ float part[2 * NT];
  if (C >= NT) {
    for (int c = tid; c < C; c += NT) {
      float sv = 0, qv = 0;
      int k = 0;
      for (; k + 4 <= NS; k += 4) {  // 4 independent chains hide L2 latency
        float s0 = psum[((long)(k + 0) * B + b) * C + c];
        float s1 = psum[((long)(k + 1) * B + b) * C + c];
        float s2 = psum[((long)(k + 2) * B + b) * C + c];
        float s3 = psum[((long)(k + 3) * B + b) * C + c];
        float q0 = psq[((long)(k + 0) * B + b) * C + c];
        float q1 = psq[((long)(k + 1) * B + b) * C + c];
        float q2 = psq[((long)(k + 2) * B + b) * C + c];
        float q3 = psq[((long)(k + 3) * B + b) * C + c];
        sv += (s0 + s1) + (s2 + s3);
        qv += (q0 + q1) + (q2 + q3);
      }
      for (; k < NS; ++k) {
        sv += psum[((long)k * B + b) * C + c];
        qv += psq[((long)k * B + b) * C + c];
      }
      float m = sv * inv_hw;
      float var = qv * inv_hw - m * m;
      if (var < 0.f) var = 0.f;
      float rs = rsqrtf(var + eps);
      sm[c] = m;
      sr[c] = rs;
      if (sl == 0) {
        mean[(long)b * C + c] = m;
        rstd[(long)b * C + c] = rs;
      }
    }
  } else {
    // narrow C (stem/upsample norms, C=64): split the slab sum over
    // (c, slab-chunk) so all NT lanes work instead of C of them; the
    // per-chunk partials meet in LDS (C and NT are powers of two)
    const int PS = NT / C;
    const int kc = tid / C;
    const int c = tid - kc * C;
    float sv = 0, qv = 0;
    int k = kc;
    for (; k + 3 * PS < NS; k += 4 * PS) {
      float s0 = psum[((long)(k + 0 * PS) * B + b) * C + c];
      float s1 = psum[((long)(k + 1 * PS) * B + b) * C + c];
      float s2 = psum[((long)(k + 2 * PS) * B + b) * C + c];
      float s3 = psum[((long)(k + 3 * PS) * B + b) * C + c];
      float q0 = psq[((long)(k + 0 * PS) * B + b) * C + c];
      float q1 = psq[((long)(k + 1 * PS) * B + b) * C + c];
      float q2 = psq[((long)(k + 2 * PS) * B + b) * C + c];
      float q3 = psq[((long)(k + 3 * PS) * B + b) * C + c];
      sv += (s0 + s1) + (s2 + s3);
      qv += (q0 + q1) + (q2 + q3);
    }
    for (; k < NS; k += PS) {
      sv += psum[((long)k * B + b) * C + c];
      qv += psq[((long)k * B + b) * C + c];
    }
    part[tid] = sv;
    part[NT + tid] = qv;
    __syncthreads();
    if (tid < C) {
      float svt = 0, qvt = 0;
      for (int j = 0; j < PS; ++j) {
        svt += part[j * C + tid];
        qvt += part[NT + j * C + tid];
      }
      float m = svt * inv_hw;
      float var = qvt * inv_hw - m * m;
      if (var < 0.f) var = 0.f;
      float rs = rsqrtf(var + eps);
      sm[tid] = m;
      sr[tid] = rs;
      if (sl == 0) {
        mean[(long)b * C + tid] = m;
        rstd[(long)b * C + tid] = rs;
      }
    }
  }
  __syncthreads();

  float qs = 0.f, mx = 0.f;
  if constexpr (Q8) qs = delayed_sx(amax_prev[0]);
  {
    int g = tid % gpr;
    int rstep = NT / gpr;
    int rof = tid / gpr;
    #pragma unroll 4
    for (long r = r0 + rof; r < r1; r += rstep) {
      long off = base + r * C + g * 8;
      v8s v = *(const v8s*)(x + off);
      v8s rv = {};
      if (res) rv = *(const v8s*)(res + off);
      v8s out;
      alignas(8) unsigned char oq[8];
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        int c = g * 8 + j;
        float val = in_affine(b2f(v[j]), sm[c], sr[c], gamma[c], beta[c]);
        if (res) val += b2f(rv[j]);
        out[j] = f2b(apply_act(val, act, slope));
        if constexpr (Q8) {
          float fv = b2f(out[j]);
          mx = fmaxf(mx, fabsf(fv));
          oq[j] = f2e4m3(fv, qs);
        }
      }
      *(v8s*)(y + off) = out;
      if constexpr (Q8) *(uint2*)(yq + off) = *(uint2*)oq;
    }
  }
  if constexpr (Q8) {
    // block max: xor-shuffles inside each wave, then the NT/64 waves meet
    // in LDS; max is exact in any order
    __shared__ float wmax[NT / 64];
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((tid & 63) == 0) wmax[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
      #pragma unroll
      for (int k = 1; k < NT / 64; ++k) mx = fmaxf(mx, wmax[k]);
      // nonneg float bits order == value order
      atomicMax((unsigned*)amax_cur, __float_as_uint(mx));
    }
  }
}

// ---- backward pass 1: slab partials of s1 = Σ dy, s2 = Σ dy*xhat ----
// yy is the activated output when the caller passed yact, else (relu/lrelu
// only) the recomputed pre-activation in_affine(x): both have the sign the
// mask needs. tanh needs the output value and always takes yact.
// The mask source is a template parameter of the backward kernels so the
// row loops carry no loop-invariant branches (a runtime select there kept
// the compiler from batching the unrolled loads).
constexpr int MASK_NONE = 0, MASK_YACT = 1, MASK_X = 2;
DEV float actbw(float d, float yy, int act, float slope) {
  if (act == ACT_RELU) return yy > 0.f ? d : 0.f;
  if (act == ACT_LRELU) return yy > 0.f ? d : d * slope;
  if (act == ACT_TANH) return d * (1.f - yy * yy);
  return d;
}

template <int MM>
__global__ __launch_bounds__(NT) void in_bwd_reduce_kernel(
    const short* __restrict__ dy, const short* __restrict__ x,
    const short* __restrict__ yact, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ mean,
    const float* __restrict__ rstd,
    float* __restrict__ p1, float* __restrict__ p2, int B, long HW, int C,
    int S, int act, float slope, float* __restrict__ zbeta,
    float* __restrict__ zgamma) {
  int b = blockIdx.x / S;
  int sl = blockIdx.x % S;
  // zero the dgamma/dbeta accumulators the NEXT kernel (in_bwd_dx) fills
  // with atomics — saves the host-side at::zeros fill launch. Null when
  // the caller accumulates onto what the destinations already hold.
  if (blockIdx.x == 0 && zbeta != nullptr)
    for (int i = threadIdx.x; i < C; i += NT) {
      zbeta[i] = 0.f;
      zgamma[i] = 0.f;
    }
  long rows = (HW + S - 1) / S;
  long r0 = sl * rows, r1 = min(r0 + rows, HW);
  const int gpr = C / 8;
  const int tid = threadIdx.x;
  const long base = (long)b * HW * C;

  int g = tid % gpr;
  int rstep = NT / gpr;
  int rof = tid / gpr;
  float a1[8] = {}, a2[8] = {};
  float mv[8], rv[8], gv[8] = {}, bv[8] = {};
  #pragma unroll
  for (int j = 0; j < 8; ++j) {
    mv[j] = mean[(long)b * C + g * 8 + j];
    rv[j] = rstd[(long)b * C + g * 8 + j];
    if (MM == MASK_X) {
      gv[j] = gamma[g * 8 + j];
      bv[j] = beta[g * 8 + j];
    }
  }
  #pragma unroll 4
  for (long r = r0 + rof; r < r1; r += rstep) {
    long off = base + r * C + g * 8;
    v8s dv = *(const v8s*)(dy + off);
    v8s xv = *(const v8s*)(x + off);
    v8s yv = {};
    if (MM == MASK_YACT) yv = *(const v8s*)(yact + off);
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      float d = b2f(dv[j]);
      float xf = b2f(xv[j]);
      if (MM == MASK_YACT) d = actbw(d, b2f(yv[j]), act, slope);
      if (MM == MASK_X)
        d = actbw(d, in_affine(xf, mv[j], rv[j], gv[j], bv[j]), act, slope);
      float xh = (xf - mv[j]) * rv[j];
      a1[j] += d; a2[j] += d * xh;
    }
  }
  __shared__ float red[NT * 17];
  #pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[tid * 17 + j] = a1[j];
    red[tid * 17 + 8 + j] = a2[j];
  }
  __syncthreads();
  long out = ((long)sl * B + b) * C;
  for (int o = tid; o < C * 2; o += NT) {
    int c = o % C;
    int is2 = o / C;
    int g2 = c / 8, j = c % 8;
    float t = 0;
    for (int k = 0; k < rstep; ++k)
      t += red[(g2 + k * gpr) * 17 + is2 * 8 + j];
    (is2 ? p2 : p1)[out + c] = t;
  }
}



// ---- backward pass 2: dx; also dgamma/dbeta reduce over b ----
template <int MM>
__global__ __launch_bounds__(NT) void in_bwd_dx_kernel(
    const short* __restrict__ dy, const short* __restrict__ x,
    const short* __restrict__ yact, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ p1,
    const float* __restrict__ p2, short* __restrict__ dx,
    float* __restrict__ dbeta, float* __restrict__ dgamma, int B, long HW,
    int C, int S, int act, float slope) {
  int b = blockIdx.x / S;
  int sl = blockIdx.x % S;
  long rows = (HW + S - 1) / S;
  long r0 = sl * rows, r1 = min(r0 + rows, HW);
  const int gpr = C / 8;
  const int tid = threadIdx.x;
  const long base = (long)b * HW * C;
  const float inv_hw = 1.f / (float)HW;

  __shared__ float sm1[MAXC], sm2[MAXC], smean[MAXC], srstd[MAXC];
  __shared__ float part[2 * NT];
  if (C >= NT) {
    for (int c = tid; c < C; c += NT) {
      float t1 = 0, t2 = 0;
      int k = 0;
      for (; k + 4 <= S; k += 4) {
        float a0 = p1[((long)(k + 0) * B + b) * C + c];
        float a1 = p1[((long)(k + 1) * B + b) * C + c];
        float a2 = p1[((long)(k + 2) * B + b) * C + c];
        float a3 = p1[((long)(k + 3) * B + b) * C + c];
        float b0 = p2[((long)(k + 0) * B + b) * C + c];
        float b1 = p2[((long)(k + 1) * B + b) * C + c];
        float b2 = p2[((long)(k + 2) * B + b) * C + c];
        float b3 = p2[((long)(k + 3) * B + b) * C + c];
        t1 += (a0 + a1) + (a2 + a3);
        t2 += (b0 + b1) + (b2 + b3);
      }
      for (; k < S; ++k) {
        t1 += p1[((long)k * B + b) * C + c];
        t2 += p2[((long)k * B + b) * C + c];
      }
      sm1[c] = t1 * inv_hw;
      sm2[c] = t2 * inv_hw;
      smean[c] = mean[(long)b * C + c];
      srstd[c] = rstd[(long)b * C + c];
      if (sl == 0) {  // fold the dgamma/dbeta reduction in (B adders per c)
        atomicAdd(&dbeta[c], t1);
        atomicAdd(&dgamma[c], t2);
      }
    }
  } else {
    // narrow C: split the slab sum over (c, slab-chunk) — see in_norm
    const int PS = NT / C;
    const int kc = tid / C;
    const int c = tid - kc * C;
    float t1 = 0, t2 = 0;
    int k = kc;
    for (; k + 3 * PS < S; k += 4 * PS) {
      float a0 = p1[((long)(k + 0 * PS) * B + b) * C + c];
      float a1 = p1[((long)(k + 1 * PS) * B + b) * C + c];
      float a2 = p1[((long)(k + 2 * PS) * B + b) * C + c];
      float a3 = p1[((long)(k + 3 * PS) * B + b) * C + c];
      float b0 = p2[((long)(k + 0 * PS) * B + b) * C + c];
      float b1 = p2[((long)(k + 1 * PS) * B + b) * C + c];
      float b2 = p2[((long)(k + 2 * PS) * B + b) * C + c];
      float b3 = p2[((long)(k + 3 * PS) * B + b) * C + c];
      t1 += (a0 + a1) + (a2 + a3);
      t2 += (b0 + b1) + (b2 + b3);
    }
    for (; k < S; k += PS) {
      t1 += p1[((long)k * B + b) * C + c];
      t2 += p2[((long)k * B + b) * C + c];
    }
    part[tid] = t1;
    part[NT + tid] = t2;
    __syncthreads();
    if (tid < C) {
      float s1 = 0, s2 = 0;
      for (int j = 0; j < PS; ++j) {
        s1 += part[j * C + tid];
        s2 += part[NT + j * C + tid];
      }
      sm1[tid] = s1 * inv_hw;
      sm2[tid] = s2 * inv_hw;
      smean[tid] = mean[(long)b * C + tid];
      srstd[tid] = rstd[(long)b * C + tid];
      if (sl == 0) {
        atomicAdd(&dbeta[tid], s1);
        atomicAdd(&dgamma[tid], s2);
      }
    }
  }
  __syncthreads();

  {
    int g = tid % gpr;
    int rstep = NT / gpr;
    int rof = tid / gpr;
    #pragma unroll 4
    for (long r = r0 + rof; r < r1; r += rstep) {
      long off = base + r * C + g * 8;
      v8s dv = *(const v8s*)(dy + off);
      v8s xv = *(const v8s*)(x + off);
      v8s yv = {};
      if (MM == MASK_YACT) yv = *(const v8s*)(yact + off);
      v8s out;
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        int c = g * 8 + j;
        float rs = srstd[c];
        float xf = b2f(xv[j]);
        float xh = (xf - smean[c]) * rs;
        float d = b2f(dv[j]);
        if (MM == MASK_YACT) d = actbw(d, b2f(yv[j]), act, slope);
        if (MM == MASK_X)
          d = actbw(d, in_affine(xf, smean[c], rs, gamma[c], beta[c]), act,
                    slope);
        out[j] = f2b(gamma[c] * rs * (d - sm1[c] - xh * sm2[c]));
      }
      *(v8s*)(dx + off) = out;
    }
  }
}

// ---- channel sum: out[c] = sum over (b,h,w) of x[...,c] (bias grads) ----
__global__ __launch_bounds__(NT) void channel_sum_kernel(
    const short* __restrict__ x, float* __restrict__ out, long rows, int C,
    int S, int nout) {
  int sl = blockIdx.x;
  long per = (rows + S - 1) / S;
  long r0 = sl * per, r1 = min(r0 + per, rows);
  const int gpr = C / 8;
  const int tid = threadIdx.x;
  int g = tid % gpr;
  int rstep = NT / gpr;
  int rof = tid / gpr;
  float a[8] = {};
  for (long r = r0 + rof; r < r1; r += rstep) {
    v8s v = *(const v8s*)(x + r * C + g * 8);
    #pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += b2f(v[j]);
  }
  __shared__ float red[NT * 17];
  #pragma unroll
  for (int j = 0; j < 8; ++j) red[tid * 17 + j] = a[j];
  __syncthreads();
  for (int c = tid; c < nout; c += NT) {  // nout <= C: the unpadded count
    int g2 = c / 8, j = c % 8;
    float t = 0;
    for (int k = 0; k < rstep; ++k) t += red[(g2 + k * gpr) * 17 + j];
    atomicAdd(&out[c], t);
  }
}

// ---- activation backward (from output) ----
__global__ void act_bwd_kernel(const short* __restrict__ dy,
                               const short* __restrict__ y,
                               short* __restrict__ out, long n, int act,
                               float slope) {
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i >= n) return;
  if (i + 8 <= n) {
    v8s dv = *(const v8s*)(dy + i);
    v8s yv = *(const v8s*)(y + i);
    v8s o;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      float d = b2f(dv[j]), yy = b2f(yv[j]);
      float r;
      if (act == ACT_RELU) r = yy > 0.f ? d : 0.f;
      else if (act == ACT_LRELU) r = yy > 0.f ? d : d * slope;
      else r = d * (1.f - yy * yy);  // tanh
      o[j] = f2b(r);
    }
    *(v8s*)(out + i) = o;
  } else {
    for (long k = i; k < n; ++k) {
      float d = b2f(dy[k]), yy = b2f(y[k]);
      float r;
      if (act == ACT_RELU) r = yy > 0.f ? d : 0.f;
      else if (act == ACT_LRELU) r = yy > 0.f ? d : d * slope;
      else r = d * (1.f - yy * yy);
      out[k] = f2b(r);
    }
  }
}

// ---- reflection pad ----
__global__ void reflect_pad_fwd_kernel(const short* __restrict__ x,
                                       short* __restrict__ y, int B, int H,
                                       int W, int C, int pt, int pb, int pl,
                                       int pr) {
  int HP = H + pt + pb, WP = W + pl + pr;
  long total = (long)B * HP * WP * C;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int c = (int)(i % C);
  long t = i / C;
  int qw = (int)(t % WP);
  t /= WP;
  int qh = (int)(t % HP);
  int b = (int)(t / HP);
  int ih = mirror_idx(qh - pt, H);
  int iw = mirror_idx(qw - pl, W);
  y[i] = x[(((long)b * H + ih) * W + iw) * C + c];
}

// C % 8 == 0: one thread copies 8 channels (16 B) of one padded pixel, so
// the pixel decode runs once per 16 B instead of once per element; IDX is
// unsigned when the padded tensor has < 2^31 vectors (32-bit div/mod).
template <typename IDX>
__global__ __launch_bounds__(256) void reflect_pad_fwd_vec_kernel(
    const short* __restrict__ x, short* __restrict__ y, int B, int H, int W,
    int C, int pt, int pb, int pl, int pr) {
  const int HP = H + pt + pb, WP = W + pl + pr;
  const IDX gpr = (IDX)(C / 8);
  const IDX total = (IDX)B * HP * WP * gpr;
  IDX i = (IDX)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  IDX t = i / gpr;
  int g = (int)(i - t * gpr);
  IDX t2 = t / (IDX)WP;
  int qw = (int)(t - t2 * WP);
  IDX b = t2 / (IDX)HP;
  int qh = (int)(t2 - b * HP);
  int ih = mirror_idx(qh - pt, H);
  int iw = mirror_idx(qw - pl, W);
  long src = (((long)b * H + ih) * W + iw) * C + g * 8;
  *(v8s*)(y + (long)i * 8) = *(const v8s*)(x + src);
}

__global__ void reflect_pad_bwd_kernel(const short* __restrict__ dyp,
                                       short* __restrict__ dx, int B, int H,
                                       int W, int C, int pt, int pb, int pl,
                                       int pr) {
  long total = (long)B * H * W * C;
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int c = (int)(idx % C);
  long t = idx / C;
  int j = (int)(t % W);
  t /= W;
  int i = (int)(t % H);
  int b = (int)(t / H);
  int HP = H + pt + pb, WP = W + pl + pr;
  float s = 0.f;
  int hc[3] = {pt + i, pt - i, pt + 2 * (H - 1) - i};
  int wc_[3] = {pl + j, pl - j, pl + 2 * (W - 1) - j};
  #pragma unroll
  for (int a = 0; a < 3; ++a) {
    int qh = hc[a];
    if (qh < 0 || qh >= HP) continue;
    if (a > 0 && qh == hc[0]) continue;
    if (a == 2 && qh == hc[1]) continue;
    #pragma unroll
    for (int d = 0; d < 3; ++d) {
      int qw = wc_[d];
      if (qw < 0 || qw >= WP) continue;
      if (d > 0 && qw == wc_[0]) continue;
      if (d == 2 && qw == wc_[1]) continue;
      s += b2f(dyp[(((long)b * HP + qh) * WP + qw) * C + c]);
    }
  }
  dx[idx] = f2b(s);
}

// ---- per-sample losses ----
// out[b] = mean over D of |a-b| or (a-b)^2; fp32 accumulation.
__global__ __launch_bounds__(NT) void persample_loss_kernel(
    const short* __restrict__ yt, const short* __restrict__ yp,
    float* __restrict__ out, long D, int squared, float cconst,
    int use_const) {
  int b = blockIdx.y;
  long base = (long)b * D;
  long per = (D + gridDim.x - 1) / gridDim.x;
  long i0 = blockIdx.x * per, i1 = min(i0 + per, D);
  float acc = 0.f;
  for (long i = i0 + threadIdx.x * 8; i < i1; i += (long)NT * 8) {
    if (i + 8 <= i1) {
      v8s pv = *(const v8s*)(yp + base + i);
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        float t = use_const ? cconst : b2f(yt[base + i + j]);
        float d = b2f(pv[j]) - t;
        acc += squared ? d * d : fabsf(d);
      }
    } else {
      for (long k = i; k < i1; ++k) {
        float t = use_const ? cconst : b2f(yt[base + k]);
        float d = b2f(yp[k + base]) - t;
        acc += squared ? d * d : fabsf(d);
      }
    }
  }
  // wave then block reduce
  #pragma unroll
  for (int off = 32; off; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ float red[NT / 64];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0;
    #pragma unroll
    for (int k = 0; k < NT / 64; ++k) s += red[k];
    atomicAdd(&out[b], s / (float)D);
  }
}

__global__ void persample_loss_bwd_kernel(
    const short* __restrict__ yt, const short* __restrict__ yp,
    const float* __restrict__ dout, short* __restrict__ gt,
    short* __restrict__ gp, long D, int squared, float cconst,
    int use_const) {
  long n = (long)gridDim.y * D;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int b = blockIdx.y;
  long base = (long)b * D;
  if (i >= D) return;
  float t = use_const ? cconst : b2f(yt[base + i]);
  float p = b2f(yp[base + i]);
  float d = p - t;
  float g = dout[b] / (float)D;
  float gpv = squared ? 2.f * d * g : (d > 0.f ? g : (d < 0.f ? -g : 0.f));
  if (gp) gp[base + i] = f2b(gpv);
  if (gt) gt[base + i] = f2b(-gpv);
  (void)n;
}

// ---- fused TF-formula Adam over flat fp32 buffers ----
// One element's update, shared by every Adam kernel below. Contraction is
// off: each product, sum, quotient and root rounds once on its own, so
// the scalar and the 16-byte kernels give the same bits whatever the
// compiler would otherwise fuse in one loop shape and not in the other
// (it fused none of this in the scalar loops and all of it in the
// vectorised one).
__device__ __forceinline__ void adam_elem(float& p, float g, float& m,
                                          float& v, float lr_t, float b1,
                                          float b2, float eps) {
#pragma clang fp contract(off)
  float gi = g;
  float mi = b1 * m + (1.f - b1) * gi;
  float vi = b2 * v + (1.f - b2) * gi * gi;
  m = mi;
  v = vi;
  p -= lr_t * mi / (sqrtf(vi) + eps);
}

// SHADOW (all Adam kernels): also store bf16(p_new) at the element's own
// index of `shadow`, the mirror region of the shadow arena (ops.arena) —
// the updated p is in a register, so the unpadded OHWI compute forms cost
// 2 B/param here instead of a gather pass. p, m, v (and ema) are what the
// !SHADOW instantiation writes, bit for bit (tests/test_adam_shadow_gpu.py).
template <bool SHADOW>
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v,
                            long n, float lr_t, float b1, float b2,
                            float eps, short* __restrict__ shadow) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    adam_elem(p[i], g[i], m[i], v[i], lr_t, b1, b2, eps);
    if (SHADOW) shadow[i] = f2b(p[i]);
  }
}

// graph-capture variant: lr_t read from device memory so a captured step
// picks up the per-step bias correction the host writes before each replay
template <bool SHADOW>
__global__ void adam_kernel_dev(float* __restrict__ p,
                                const float* __restrict__ g,
                                float* __restrict__ m, float* __restrict__ v,
                                long n, const float* __restrict__ lr_t_ptr,
                                float b1, float b2, float eps,
                                short* __restrict__ shadow) {
  const float lr_t = *lr_t_ptr;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    adam_elem(p[i], g[i], m[i], v[i], lr_t, b1, b2, eps);
    if (SHADOW) shadow[i] = f2b(p[i]);
  }
}

// ---- Adam + exponential moving average of the weights, one pass ----
// ema = d*ema + (1-d)*p_new rides the Adam walk: the updated p is still in
// a register, so the average costs its own read and write (8 B/param) and
// nothing else. The m/v/p arithmetic is adam_elem, the plain kernels'
// own: p, m, v come out bitwise what they give
// (tests/test_adam_ema_gpu.py), so switching the average on cannot move
// the training trajectory.
__device__ __forceinline__ void adam_ema_elem(float& p, float g, float& m,
                                              float& v, float& e, float lr_t,
                                              float b1, float b2, float eps,
                                              float d, float omd) {
#pragma clang fp contract(off)
  adam_elem(p, g, m, v, lr_t, b1, b2, eps);
  e = d * e + omd * p;
}

// VEC: 16-byte loads/stores over the first n/4*4 elements (all five
// pointers 16-byte aligned, checked by the host) and a scalar tail of
// n%4; !VEC: scalar throughout, for views at an odd storage offset.
// LR_DEV: lr_t read from device memory (capture-safe, as adam_kernel_dev).
// SHADOW: as above; the VEC path stores its four bf16 as one 8-byte word
// (shadow 8-byte aligned, checked by the host).
template <bool VEC, bool LR_DEV, bool SHADOW>
__global__ void adam_ema_kernel(float* __restrict__ p,
                                const float* __restrict__ g,
                                float* __restrict__ m, float* __restrict__ v,
                                float* __restrict__ ema, long n, float lr_imm,
                                const float* __restrict__ lr_t_ptr, float b1,
                                float b2, float eps, float d, float omd,
                                short* __restrict__ shadow) {
  const float lr_t = LR_DEV ? *lr_t_ptr : lr_imm;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  long done = 0;
  if (VEC) {
    const long n4 = n >> 2;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    float4* e4 = reinterpret_cast<float4*>(ema);
    for (long i = tid; i < n4; i += stride) {
      float4 pi = p4[i], gi = g4[i], mi = m4[i], vi = v4[i], ei = e4[i];
      adam_ema_elem(pi.x, gi.x, mi.x, vi.x, ei.x, lr_t, b1, b2, eps, d, omd);
      adam_ema_elem(pi.y, gi.y, mi.y, vi.y, ei.y, lr_t, b1, b2, eps, d, omd);
      adam_ema_elem(pi.z, gi.z, mi.z, vi.z, ei.z, lr_t, b1, b2, eps, d, omd);
      adam_ema_elem(pi.w, gi.w, mi.w, vi.w, ei.w, lr_t, b1, b2, eps, d, omd);
      m4[i] = mi;
      v4[i] = vi;
      p4[i] = pi;
      e4[i] = ei;
      if (SHADOW) {
        v4s s = {f2b(pi.x), f2b(pi.y), f2b(pi.z), f2b(pi.w)};
        reinterpret_cast<v4s*>(shadow)[i] = s;
      }
    }
    done = n4 << 2;
  }
  for (long i = done + tid; i < n; i += stride) {
    adam_ema_elem(p[i], g[i], m[i], v[i], ema[i], lr_t, b1, b2, eps, d, omd);
    if (SHADOW) shadow[i] = f2b(p[i]);
  }
}

// ================= host wrappers =================

static int slices_for(long HW, int B) {
  // >= ~512 blocks for occupancy, but cap slices: slab traffic in the
  // stats phases scales with S per block.
  int s = (int)std::min<long>(std::max<long>(1, 512 / std::max(B, 1)),
                              std::max<long>(1, HW / 64));
  return std::max(1, s);
}

// amax_prev/amax_cur given (instnorm_fwd_q8): the normalize pass also
// writes the consumer's e4m3 operand and returns {y, mean, rstd, yq}.
static std::vector<at::Tensor> instnorm_fwd_impl(
    at::Tensor x, at::Tensor gamma, at::Tensor beta, double eps, int64_t act,
    double slope, c10::optional<at::Tensor> residual,
    c10::optional<at::Tensor> psum_in, c10::optional<at::Tensor> psq_in,
    int64_t nslabs, const at::Tensor* amax_prev, at::Tensor* amax_cur) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.is_contiguous());
  int B = x.size(0), C = x.size(3);
  long HW = (long)x.size(1) * x.size(2);
  TORCH_CHECK(C % 8 == 0 && (C / 8) <= 256 && 256 % std::min(C / 8, 256) == 0,
              "instnorm: unsupported channel count ", C);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto fopt = x.options().dtype(at::kFloat);
  int S = slices_for(HW, B);
  auto mean = at::empty({B, C}, fopt);
  auto rstd = at::empty({B, C}, fopt);
  auto y = at::empty_like(x);
  const short* resf = residual.has_value()
                          ? (const short*)residual->const_data_ptr() : nullptr;
  const bool q8 = amax_prev != nullptr;
  at::Tensor yq;
  if (q8) {
    TORCH_CHECK(amax_cur != nullptr && amax_prev->is_cuda() &&
                amax_cur->is_cuda() &&
                amax_prev->scalar_type() == at::kFloat &&
                amax_cur->scalar_type() == at::kFloat &&
                amax_prev->numel() >= 1 && amax_cur->numel() >= 1,
                "instnorm_fwd_q8: bad amax slots");
    yq = at::empty_like(x, x.options().dtype(at::kByte));
  }
  // the slabs the normalize prologue sums: the producing conv's epilogue
  // wrote them ([nslabs,B,C] fp32, one per 128-row M-tile), or in_reduce
  // writes one per spatial slice here. The grid keeps slices_for() either
  // way; only the prologue's slab count changes.
  at::Tensor psum, psq;
  int ns = S;
  if (psum_in.has_value()) {
    TORCH_CHECK(psq_in.has_value() && nslabs >= 1 &&
                psum_in->scalar_type() == at::kFloat &&
                psq_in->scalar_type() == at::kFloat &&
                psum_in->is_contiguous() && psq_in->is_contiguous() &&
                psum_in->numel() == nslabs * B * C &&
                psq_in->numel() == nslabs * B * C,
                "instnorm_fwd: bad precomputed slabs");
    psum = *psum_in;
    psq = *psq_in;
    ns = (int)nslabs;
  } else {
    psum = at::empty({S, B, C}, fopt);
    psq = at::empty({S, B, C}, fopt);
    hipLaunchKernelGGL(in_reduce_kernel, dim3(B * S), dim3(NT), 0, stream,
                       (const short*)x.const_data_ptr(),
                       (float*)psum.mutable_data_ptr(),
                       (float*)psq.mutable_data_ptr(), B, HW, C, S);
  }
  const float* ps = (const float*)psum.const_data_ptr();
  const float* pq = (const float*)psq.const_data_ptr();
  if (q8)
    hipLaunchKernelGGL(in_norm_kernel<true>, dim3(B * S), dim3(NT), 0,
                       stream, (const short*)x.const_data_ptr(),
                       (const float*)gamma.const_data_ptr(),
                       (const float*)beta.const_data_ptr(), ps, pq,
                       (float*)mean.mutable_data_ptr(),
                       (float*)rstd.mutable_data_ptr(), resf,
                       (short*)y.mutable_data_ptr(), B, HW, C, S, ns,
                       (int)act, (float)slope, (float)eps,
                       (unsigned char*)yq.mutable_data_ptr(),
                       (const float*)amax_prev->const_data_ptr(),
                       (float*)amax_cur->mutable_data_ptr());
  else
    hipLaunchKernelGGL(in_norm_kernel<false>, dim3(B * S), dim3(NT), 0,
                       stream, (const short*)x.const_data_ptr(),
                       (const float*)gamma.const_data_ptr(),
                       (const float*)beta.const_data_ptr(), ps, pq,
                       (float*)mean.mutable_data_ptr(),
                       (float*)rstd.mutable_data_ptr(), resf,
                       (short*)y.mutable_data_ptr(), B, HW, C, S, ns,
                       (int)act, (float)slope, (float)eps,
                       (unsigned char*)nullptr, (const float*)nullptr,
                       (float*)nullptr);
  std::vector<at::Tensor> out{y, mean, rstd};
  if (q8) out.push_back(yq);
  return out;
}

std::vector<at::Tensor> instnorm_fwd(at::Tensor x, at::Tensor gamma,
                                     at::Tensor beta, double eps, int64_t act,
                                     double slope,
                                     c10::optional<at::Tensor> residual,
                                     c10::optional<at::Tensor> psum_in,
                                     c10::optional<at::Tensor> psq_in,
                                     int64_t nslabs) {
  return instnorm_fwd_impl(x, gamma, beta, eps, act, slope, residual, psum_in,
                           psq_in, nslabs, nullptr, nullptr);
}

// instnorm_fwd that also emits the e4m3 twin of y for the fp8 conv that
// consumes it: yq == quant_fp8_d(y, amax_prev, .) byte for byte, and
// amax_cur = max(amax_cur, max|y|). Returns {y, mean, rstd, yq}.
std::vector<at::Tensor> instnorm_fwd_q8(at::Tensor x, at::Tensor gamma,
                                        at::Tensor beta, double eps,
                                        int64_t act, double slope,
                                        c10::optional<at::Tensor> residual,
                                        c10::optional<at::Tensor> psum_in,
                                        c10::optional<at::Tensor> psq_in,
                                        int64_t nslabs, at::Tensor amax_prev,
                                        at::Tensor amax_cur) {
  return instnorm_fwd_impl(x, gamma, beta, eps, act, slope, residual, psum_in,
                           psq_in, nslabs, &amax_prev, &amax_cur);
}

// launch a backward kernel template with the mask mode chosen at run time
#define LAUNCH_MM(kern, mm, grid, stream, ...)                              \
  do {                                                                      \
    if ((mm) == MASK_X)                                                     \
      hipLaunchKernelGGL(kern<MASK_X>, grid, dim3(NT), 0, stream,           \
                         __VA_ARGS__);                                      \
    else if ((mm) == MASK_YACT)                                             \
      hipLaunchKernelGGL(kern<MASK_YACT>, grid, dim3(NT), 0, stream,        \
                         __VA_ARGS__);                                      \
    else                                                                    \
      hipLaunchKernelGGL(kern<MASK_NONE>, grid, dim3(NT), 0, stream,        \
                         __VA_ARGS__);                                      \
  } while (0)

std::vector<at::Tensor> instnorm_bwd(at::Tensor dy, at::Tensor x,
                                     at::Tensor gamma, at::Tensor mean,
                                     at::Tensor rstd,
                                     c10::optional<at::Tensor> yact,
                                     int64_t act, double slope,
                                     c10::optional<at::Tensor> beta,
                                     c10::optional<at::Tensor> dgamma_out,
                                     c10::optional<at::Tensor> dbeta_out,
                                     bool accumulate) {
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16 &&
              dy.is_contiguous() && x.is_contiguous());
  // destinations: two separate fp32 [C] blocks (slices of a flat grad
  // buffer) the atomics of in_bwd_dx land in; with accumulate they are not
  // zeroed first
  TORCH_CHECK(dgamma_out.has_value() == dbeta_out.has_value(),
              "instnorm_bwd: pass both destinations or neither");
  TORCH_CHECK(!accumulate || dgamma_out.has_value(),
              "instnorm_bwd: accumulate needs destinations");
  if (dgamma_out.has_value())
    for (const at::Tensor* t : {&*dgamma_out, &*dbeta_out})
      TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat &&
                      t->is_contiguous() && t->numel() == x.size(3),
                  "instnorm_bwd: destinations must be contiguous fp32 [C]");
  // without yact the relu/lrelu mask is recomputed from x, which needs
  // beta; tanh needs the output value itself
  TORCH_CHECK(act == ACT_NONE || yact.has_value() ||
              ((act == ACT_RELU || act == ACT_LRELU) && beta.has_value()),
              "instnorm_bwd: act ", act, " needs yact (or beta for relu/lrelu)");
  TORCH_CHECK(!beta.has_value() ||
              (beta->scalar_type() == at::kFloat && beta->numel() == x.size(3)),
              "instnorm_bwd: beta must be fp32 [C]");
  const float* betap =
      beta.has_value() ? (const float*)beta->const_data_ptr() : nullptr;
  const int mm = act == ACT_NONE ? MASK_NONE
                                 : (yact.has_value() ? MASK_YACT : MASK_X);
  int B = x.size(0), C = x.size(3);
  long HW = (long)x.size(1) * x.size(2);
  TORCH_CHECK(C % 8 == 0 && (C / 8) <= 256 && 256 % std::min(C / 8, 256) == 0,
              "instnorm_bwd: unsupported channel count ", C);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto fopt = x.options().dtype(at::kFloat);
  int S = slices_for(HW, B);
  auto dx = at::empty_like(x);
  at::Tensor dbeta, dgamma;
  if (dgamma_out.has_value()) {
    dbeta = *dbeta_out;
    dgamma = *dgamma_out;
  } else {
    auto dgb = at::empty({2, C}, fopt);
    dbeta = dgb[0];
    dgamma = dgb[1];
  }
  float* zb = accumulate ? nullptr : (float*)dbeta.mutable_data_ptr();
  float* zg = accumulate ? nullptr : (float*)dgamma.mutable_data_ptr();
  const short* yp = yact.has_value()
                        ? (const short*)yact->const_data_ptr() : nullptr;

  auto p1 = at::empty({S, B, C}, fopt);
  auto p2 = at::empty({S, B, C}, fopt);
  LAUNCH_MM(in_bwd_reduce_kernel, mm, dim3(B * S), stream,
                     (const short*)dy.const_data_ptr(),
                     (const short*)x.const_data_ptr(), yp,
                     (const float*)gamma.const_data_ptr(), betap,
                     (const float*)mean.const_data_ptr(),
                     (const float*)rstd.const_data_ptr(),
                     (float*)p1.mutable_data_ptr(),
                     (float*)p2.mutable_data_ptr(), B, HW, C, S, (int)act,
                     (float)slope, zb, zg);
  LAUNCH_MM(in_bwd_dx_kernel, mm, dim3(B * S), stream,
                     (const short*)dy.const_data_ptr(),
                     (const short*)x.const_data_ptr(), yp,
                     (const float*)gamma.const_data_ptr(), betap,
                     (const float*)mean.const_data_ptr(),
                     (const float*)rstd.const_data_ptr(),
                     (const float*)p1.const_data_ptr(),
                     (const float*)p2.const_data_ptr(),
                     (short*)dx.mutable_data_ptr(),
                     (float*)dbeta.mutable_data_ptr(),
                     (float*)dgamma.mutable_data_ptr(), B, HW, C, S,
                     (int)act, (float)slope);
  return {dx, dgamma, dbeta};
}

// out (optional): a contiguous fp32 destination of the first out.numel()
// <= C channels (a bias's slice of a flat grad buffer; x may be channel-
// padded); with accumulate the sums are added to what it holds. The zero
// fill stays a memset: the kernel has no grid-wide ordering to hide it
// behind, and an accumulating call skips it.
at::Tensor channel_sum(at::Tensor x, c10::optional<at::Tensor> dest,
                       bool accumulate) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.is_contiguous());
  int C = x.size(-1);
  long rows = x.numel() / C;
  TORCH_CHECK(C % 8 == 0 && (C / 8) <= NT && NT % (C / 8) == 0,
              "channel_sum: unsupported C ", C);
  TORCH_CHECK(!accumulate || dest.has_value(),
              "channel_sum: accumulate needs a destination");
  at::Tensor out;
  if (dest.has_value()) {
    out = *dest;
    TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kFloat &&
                    out.is_contiguous() && out.numel() >= 1 &&
                    out.numel() <= C,
                "channel_sum: out must be contiguous fp32 of <= C elements");
  } else {
    out = at::empty({C}, x.options().dtype(at::kFloat));
  }
  const int nout = (int)out.numel();
  if (!accumulate)
    CHECK_HIP(hipMemsetAsync(out.mutable_data_ptr(), 0, nout * sizeof(float),
                             at::cuda::getCurrentCUDAStream()));
  int S = (int)std::min<long>(512, std::max<long>(1, rows / 64));
  hipLaunchKernelGGL(channel_sum_kernel, dim3(S), dim3(NT), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const short*)x.const_data_ptr(),
                     (float*)out.mutable_data_ptr(), rows, C, S, nout);
  return out;
}

at::Tensor act_bwd(at::Tensor dy, at::Tensor y, int64_t act, double slope) {
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16);
  auto out = at::empty_like(dy);
  long n = dy.numel();
  long blocks = (n / 8 + 255) / 256 + 1;
  hipLaunchKernelGGL(act_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const short*)dy.const_data_ptr(),
                     (const short*)y.const_data_ptr(),
                     (short*)out.mutable_data_ptr(), n, (int)act,
                     (float)slope);
  return out;
}

at::Tensor reflect_pad_fwd(at::Tensor x, int64_t pt, int64_t pb, int64_t pl,
                           int64_t pr) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.is_contiguous());
  int B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  auto y = at::empty({B, H + pt + pb, W + pl + pr, C}, x.options());
  long total = y.numel();
  TORCH_CHECK(pt >= 0 && pb >= 0 && pl >= 0 && pr >= 0 && pt < H && pb < H &&
              pl < W && pr < W, "reflect_pad: pads must be in [0, size)");
  // CYG_NO_PAD_VEC=1 restores the one-element-per-thread kernel everywhere
  static const bool no_vec = []() {
    const char* e = getenv("CYG_NO_PAD_VEC");
    return e && e[0] == '1';
  }();
  const bool al16 = ((uintptr_t)x.const_data_ptr() % 16) == 0 &&
                    ((uintptr_t)y.const_data_ptr() % 16) == 0;
  if (!no_vec && C % 8 == 0 && al16 && total > 0) {
    long nvec = total / 8;
    TORCH_CHECK((nvec + 255) / 256 < (1L << 31), "reflect_pad: too large");
    dim3 grid((unsigned)((nvec + 255) / 256));
    if (nvec < (1L << 31) - 256) {
      hipLaunchKernelGGL(reflect_pad_fwd_vec_kernel<unsigned>, grid,
                         dim3(256), 0, at::cuda::getCurrentCUDAStream(),
                         (const short*)x.const_data_ptr(),
                         (short*)y.mutable_data_ptr(), B, H, W, C, (int)pt,
                         (int)pb, (int)pl, (int)pr);
    } else {
      hipLaunchKernelGGL(reflect_pad_fwd_vec_kernel<unsigned long>, grid,
                         dim3(256), 0, at::cuda::getCurrentCUDAStream(),
                         (const short*)x.const_data_ptr(),
                         (short*)y.mutable_data_ptr(), B, H, W, C, (int)pt,
                         (int)pb, (int)pl, (int)pr);
    }
    return y;
  }
  hipLaunchKernelGGL(reflect_pad_fwd_kernel, dim3(cdiv64(total, 256)),
                     dim3(256), 0, at::cuda::getCurrentCUDAStream(),
                     (const short*)x.const_data_ptr(),
                     (short*)y.mutable_data_ptr(), B, H, W, C, (int)pt,
                     (int)pb, (int)pl, (int)pr);
  return y;
}

at::Tensor reflect_pad_bwd(at::Tensor dyp, int64_t pt, int64_t pb, int64_t pl,
                           int64_t pr) {
  TORCH_CHECK(dyp.is_cuda() && dyp.scalar_type() == at::kBFloat16 && dyp.is_contiguous());
  int B = dyp.size(0);
  int H = dyp.size(1) - pt - pb, W = dyp.size(2) - pl - pr, C = dyp.size(3);
  auto dx = at::empty({B, H, W, C}, dyp.options());
  long total = dx.numel();
  hipLaunchKernelGGL(reflect_pad_bwd_kernel, dim3(cdiv64(total, 256)),
                     dim3(256), 0, at::cuda::getCurrentCUDAStream(),
                     (const short*)dyp.const_data_ptr(),
                     (short*)dx.mutable_data_ptr(), B, H, W, C, (int)pt,
                     (int)pb, (int)pl, (int)pr);
  return dx;
}

static at::Tensor persample_fwd_impl(c10::optional<at::Tensor> yt,
                                     at::Tensor yp, bool squared,
                                     double cconst) {
  TORCH_CHECK(yp.is_cuda() && yp.scalar_type() == at::kBFloat16 && yp.is_contiguous());
  int B = yp.size(0);
  long D = yp.numel() / B;
  auto out = at::empty({B}, yp.options().dtype(at::kFloat));
  CHECK_HIP(hipMemsetAsync(out.mutable_data_ptr(), 0, B * sizeof(float),
                           at::cuda::getCurrentCUDAStream()));
  int gx = (int)std::min<long>(32, std::max<long>(1, D / (256 * 8)));
  dim3 grid(gx, B);
  hipLaunchKernelGGL(persample_loss_kernel, grid, dim3(NT), 0,
                     at::cuda::getCurrentCUDAStream(),
                     yt.has_value() ? (const short*)yt->const_data_ptr() : nullptr,
                     (const short*)yp.const_data_ptr(),
                     (float*)out.mutable_data_ptr(), D, squared ? 1 : 0,
                     (float)cconst, yt.has_value() ? 0 : 1);
  return out;
}

at::Tensor persample_loss_fwd(at::Tensor yt, at::Tensor yp, bool squared) {
  return persample_fwd_impl(yt.contiguous(), yp, squared, 0.0);
}

at::Tensor persample_loss_const_fwd(at::Tensor yp, double cconst, bool squared) {
  return persample_fwd_impl(c10::nullopt, yp, squared, cconst);
}

std::vector<at::Tensor> persample_loss_bwd(at::Tensor yt, at::Tensor yp,
                                           at::Tensor dout, bool squared,
                                           bool need_gt, bool need_gp) {
  int B = yp.size(0);
  long D = yp.numel() / B;
  auto gt = need_gt ? at::empty_like(yt) : at::Tensor();
  auto gp = need_gp ? at::empty_like(yp) : at::Tensor();
  dim3 grid(cdiv64(D, 256), B);
  hipLaunchKernelGGL(persample_loss_bwd_kernel, grid, dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const short*)yt.const_data_ptr(),
                     (const short*)yp.const_data_ptr(),
                     (const float*)dout.const_data_ptr(),
                     need_gt ? (short*)gt.mutable_data_ptr() : nullptr,
                     need_gp ? (short*)gp.mutable_data_ptr() : nullptr, D,
                     squared ? 1 : 0, 0.f, 0);
  return {gt, gp};
}

at::Tensor persample_loss_const_bwd(at::Tensor yp, double cconst,
                                    at::Tensor dout, bool squared) {
  int B = yp.size(0);
  long D = yp.numel() / B;
  auto gp = at::empty_like(yp);
  dim3 grid(cdiv64(D, 256), B);
  hipLaunchKernelGGL(persample_loss_bwd_kernel, grid, dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(), nullptr,
                     (const short*)yp.const_data_ptr(),
                     (const float*)dout.const_data_ptr(), nullptr,
                     (short*)gp.mutable_data_ptr(), D, squared ? 1 : 0,
                     (float)cconst, 1);
  return gp;
}

// The optional mirror (SHADOW kernels): bf16, contiguous, on p's device, at
// least p.numel() long. Returns its pointer, or nullptr when absent.
static short* adam_shadow_ptr(const c10::optional<at::Tensor>& shadow,
                              const at::Tensor& p) {
  if (!shadow.has_value()) return nullptr;
  const at::Tensor& s = *shadow;
  TORCH_CHECK(s.is_cuda() && s.device() == p.device() &&
                  s.scalar_type() == at::kBFloat16 && s.is_contiguous() &&
                  s.numel() >= p.numel(),
              "adam: shadow must be a contiguous bf16 tensor on the "
              "parameters' device, at least as long as they are");
  return (short*)s.mutable_data_ptr();
}

void adam_step(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
               double lr, double b1, double b2, double eps, int64_t t,
               c10::optional<at::Tensor> shadow) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat);
  long n = p.numel();
  short* sp = adam_shadow_ptr(shadow, p);
  // TF formula: lr_t = lr*sqrt(1-b2^t)/(1-b1^t); eps beside sqrt(v)
  double lr_t = lr * std::sqrt(1.0 - std::pow(b2, (double)t)) /
                (1.0 - std::pow(b1, (double)t));
  int blocks = (int)std::min<long>(2048, (n + 255) / 256);
#define CYG_ADAM(SH)                                                        \
  hipLaunchKernelGGL(adam_kernel<SH>, dim3(blocks), dim3(256), 0,           \
                     at::cuda::getCurrentCUDAStream(),                      \
                     (float*)p.mutable_data_ptr(),                          \
                     (const float*)g.const_data_ptr(),                      \
                     (float*)m.mutable_data_ptr(),                          \
                     (float*)v.mutable_data_ptr(), n, (float)lr_t,          \
                     (float)b1, (float)b2, (float)eps, sp)
  if (sp) CYG_ADAM(true); else CYG_ADAM(false);
#undef CYG_ADAM
}

void adam_step_dev(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
                   at::Tensor lr_t, double b1, double b2, double eps,
                   c10::optional<at::Tensor> shadow) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat);
  TORCH_CHECK(lr_t.is_cuda() && lr_t.scalar_type() == at::kFloat);
  long n = p.numel();
  short* sp = adam_shadow_ptr(shadow, p);
  int blocks = (int)std::min<long>(2048, (n + 255) / 256);
#define CYG_ADAM_DEV(SH)                                                    \
  hipLaunchKernelGGL(adam_kernel_dev<SH>, dim3(blocks), dim3(256), 0,       \
                     at::cuda::getCurrentCUDAStream(),                      \
                     (float*)p.mutable_data_ptr(),                          \
                     (const float*)g.const_data_ptr(),                      \
                     (float*)m.mutable_data_ptr(),                          \
                     (float*)v.mutable_data_ptr(), n,                       \
                     (const float*)lr_t.const_data_ptr(), (float)b1,        \
                     (float)b2, (float)eps, sp)
  if (sp) CYG_ADAM_DEV(true); else CYG_ADAM_DEV(false);
#undef CYG_ADAM_DEV
}

// shared by adam_ema_step / adam_ema_step_dev: checks, path choice, launch
static void adam_ema_launch(at::Tensor& p, at::Tensor& g, at::Tensor& m,
                            at::Tensor& v, at::Tensor& ema, float lr_imm,
                            const float* lr_t_ptr, double b1, double b2,
                            double eps, double ema_decay,
                            const c10::optional<at::Tensor>& shadow) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat);
  short* sp = adam_shadow_ptr(shadow, p);
  for (const at::Tensor* t : {&p, &g, &m, &v, &ema}) {
    TORCH_CHECK(t->scalar_type() == at::kFloat, "adam_ema: fp32 only");
    TORCH_CHECK(t->numel() == p.numel(), "adam_ema: numel mismatch");
    TORCH_CHECK(t->is_contiguous(), "adam_ema: contiguous only");
    TORCH_CHECK(t->device() == p.device(), "adam_ema: device mismatch");
  }
  TORCH_CHECK(ema_decay >= 0.0 && ema_decay <= 1.0);
  long n = p.numel();
  if (n == 0) return;
  float* pp = (float*)p.mutable_data_ptr();
  const float* gp = (const float*)g.const_data_ptr();
  float* mp = (float*)m.mutable_data_ptr();
  float* vp = (float*)v.mutable_data_ptr();
  float* ep = (float*)ema.mutable_data_ptr();
  // a sliced view may start at an odd storage offset: 16-byte accesses
  // only when every pointer allows them
  bool vec = ((reinterpret_cast<uintptr_t>(pp) |
               reinterpret_cast<uintptr_t>(gp) |
               reinterpret_cast<uintptr_t>(mp) |
               reinterpret_cast<uintptr_t>(vp) |
               reinterpret_cast<uintptr_t>(ep)) & 15) == 0 &&
             (reinterpret_cast<uintptr_t>(sp) & 7) == 0;
  // constants of the run: 1-d in double, then cast (a captured graph
  // bakes both in)
  float d = (float)ema_decay, omd = (float)(1.0 - ema_decay);
  long work = vec ? std::max<long>(n >> 2, n & 3) : n;
  int blocks = (int)std::min<long>(2048, (work + 255) / 256);
  auto stream = at::cuda::getCurrentCUDAStream();
#define CYG_ADAM_EMA(VEC, LRD)                                              \
  do {                                                                      \
    if (sp)                                                                 \
      hipLaunchKernelGGL((adam_ema_kernel<VEC, LRD, true>), dim3(blocks),   \
                         dim3(256), 0, stream, pp, gp, mp, vp, ep, n,       \
                         lr_imm, lr_t_ptr, (float)b1, (float)b2,            \
                         (float)eps, d, omd, sp);                           \
    else                                                                    \
      hipLaunchKernelGGL((adam_ema_kernel<VEC, LRD, false>), dim3(blocks),  \
                         dim3(256), 0, stream, pp, gp, mp, vp, ep, n,       \
                         lr_imm, lr_t_ptr, (float)b1, (float)b2,            \
                         (float)eps, d, omd, sp);                           \
  } while (0)
  if (lr_t_ptr) {
    if (vec) CYG_ADAM_EMA(true, true); else CYG_ADAM_EMA(false, true);
  } else {
    if (vec) CYG_ADAM_EMA(true, false); else CYG_ADAM_EMA(false, false);
  }
#undef CYG_ADAM_EMA
}

void adam_ema_step(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
                   at::Tensor ema, double lr, double b1, double b2,
                   double eps, int64_t t, double ema_decay,
                   c10::optional<at::Tensor> shadow) {
  // same host arithmetic as adam_step: the immediate must be bit-equal
  double lr_t = lr * std::sqrt(1.0 - std::pow(b2, (double)t)) /
                (1.0 - std::pow(b1, (double)t));
  adam_ema_launch(p, g, m, v, ema, (float)lr_t, nullptr, b1, b2, eps,
                  ema_decay, shadow);
}

void adam_ema_step_dev(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
                       at::Tensor ema, at::Tensor lr_t, double b1, double b2,
                       double eps, double ema_decay,
                       c10::optional<at::Tensor> shadow) {
  TORCH_CHECK(lr_t.is_cuda() && lr_t.scalar_type() == at::kFloat &&
              lr_t.numel() == 1 && lr_t.device() == p.device());
  adam_ema_launch(p, g, m, v, ema, 0.f, (const float*)lr_t.const_data_ptr(),
                  b1, b2, eps, ema_decay, shadow);
}

}  // namespace cyg
