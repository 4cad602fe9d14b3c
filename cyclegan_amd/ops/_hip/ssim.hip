// Per-sample mean SSIM and its gradient — gfx950.
//
// Semantics of tf.image.ssim(x, y, max_val=2): an 11x11 Gaussian window
// (sigma 1.5, sum 1, separable), VALID placement — the window grid of an
// HxW image is OH x OW = (H-10) x (W-10) — per-channel statistics, and
//
//   mx = E[x]  my = E[y]  qx = E[x^2]  qy = E[y^2]  p = E[xy]
//   A1 = 2 mx my + c1            B1 = mx^2 + my^2 + c1
//   A2 = 2 (p - mx my) + c2      B2 = (qx - mx^2) + (qy - my^2) + c2
//   S  = (A1/B1) (A2/B2),        out[b] = mean of S over windows, channels
//
// Inputs are NHWC bf16; every sum is fp32. C is a runtime value and a pixel
// is C*2 bytes (6 at C = 3): the kernels load and store single bf16
// elements and assume no alignment beyond 2 bytes.
//
// Forward: a block owns a TH x TW tile of windows of one sample and loops
// over the channels. Per channel it stages the (TH+10) x (TW+10) patch of
// x and y in LDS as fp32, runs the horizontal 11-tap pass over the five
// maps x, y, x^2, y^2, xy into LDS, and each thread runs the vertical pass
// of ONE window and forms S. The block's sum goes through wave shuffles
// and LDS to one atomicAdd of (sum / N) into out[b], as in
// persample_loss_kernel. When a gradient is wanted the thread also stores
// the derivatives of S by the raw moments of the image(s) to
// differentiate, taken as independent variables:
//
//   ay = dS/dE[y]   = 2 [mx (A2-A1) - my S (B2-B1)] / (B1 B2)
//   ax = dS/dE[x]   = 2 [my (A2-A1) - mx S (B2-B1)] / (B1 B2)
//   b  = dS/dE[y^2] = dS/dE[x^2] = -S / B2
//   c  = dS/dE[xy]  = 2 (A1/B1) / B2
//
// Backward (gradient by y; by x: swap the images and pass ax):
//
//   dL/dy_j = dout[b]/N * [ (G^T ay)_j + 2 y_j (G^T b)_j + x_j (G^T c)_j ]
//
// G^T is the adjoint of the VALID blur: a full-mode correlation of a map
// over the window grid, zero outside it. A block owns a TH x TW tile of
// PIXELS, stages the (TH+10) x (TW+10) patch of each of the three maps
// (window rows h-10..h, columns w-10..w), runs the two 11-tap passes with
// the taps reversed, combines and stores bf16.
//
// LDS, static, per block: forward 2 patches + 5 row-filtered maps, backward
// 3 + 3; sizes at the constants below. Patch rows are padded to a stride
// of 48 floats (16 mod 32) so the two rows a 32-lane group reads in the
// horizontal pass fall on disjoint banks.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

namespace cyg {

constexpr int SSIM_K = 11;             // window taps
constexpr int SSIM_TH = 16;            // tile rows
constexpr int SSIM_TW = 16;            // tile columns
constexpr int SSIM_NT = SSIM_TH * SSIM_TW;
constexpr int SSIM_PH = SSIM_TH + SSIM_K - 1;  // patch rows (26)
constexpr int SSIM_PW = SSIM_TW + SSIM_K - 1;  // patch columns (26)
constexpr int SSIM_PS = 48;            // patch row stride in floats
static_assert(SSIM_NT % 64 == 0, "whole waves");
static_assert(SSIM_PS >= SSIM_PW, "patch row fits its stride");
// forward: 2*26*48*4 + 5*26*16*4 + 16 = 18 320 B; backward 3*(26*48+26*16)*4
// = 19 968 B
static_assert((2 * SSIM_PH * SSIM_PS + 5 * SSIM_PH * SSIM_TW) * 4 + 64 <=
              64 * 1024, "forward LDS");
static_assert(3 * (SSIM_PH * SSIM_PS + SSIM_PH * SSIM_TW) * 4 <= 64 * 1024,
              "backward LDS");

struct SsimWin { float g[SSIM_K]; };

// grid (tiles_w, tiles_h, B). N = OH*OW*C. ay/ax/bm/cm may be null.
__global__ __launch_bounds__(SSIM_NT) void ssim_fwd_kernel(
    const short* __restrict__ X, const short* __restrict__ Y,
    float* __restrict__ out, float* __restrict__ ay, float* __restrict__ ax,
    float* __restrict__ bm, float* __restrict__ cm, int H, int W, int C,
    SsimWin win, float c1, float c2, float inv_n) {
  __shared__ float sx[SSIM_PH][SSIM_PS];
  __shared__ float sy[SSIM_PH][SSIM_PS];
  __shared__ float hm[5][SSIM_PH][SSIM_TW];
  __shared__ float red[SSIM_NT / 64];

  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int OH = H - (SSIM_K - 1), OW = W - (SSIM_K - 1);
  const int h0 = blockIdx.y * SSIM_TH, w0 = blockIdx.x * SSIM_TW;
  const int ty = tid / SSIM_TW, tx = tid % SSIM_TW;
  const int oh = h0 + ty, ow = w0 + tx;
  const bool live = oh < OH && ow < OW;
  const long img = (long)b * H * W * C;
  float acc = 0.f;

  for (int c = 0; c < C; ++c) {
    // pivots: the tile's first pixel (h0 < OH, w0 < OW: inside the image).
    // Variances and the covariance do not move with a shift, and the
    // differences are exact in fp32 for bf16 inputs of like magnitude, so
    // taking the moments of x - px, y - py keeps E[x^2] - mx^2 from
    // cancelling on nearly flat images
    const long at0 = img + ((long)h0 * W + w0) * C + c;
    const float px = b2f(X[at0]), py = b2f(Y[at0]);
    // stage: zero past the image edge (only dead windows read it)
    for (int i = tid; i < SSIM_PH * SSIM_PW; i += SSIM_NT) {
      const int r = i / SSIM_PW, q = i % SSIM_PW;
      const int gh = h0 + r, gw = w0 + q;
      float xv = 0.f, yv = 0.f;
      if (gh < H && gw < W) {
        const long at = img + ((long)gh * W + gw) * C + c;
        xv = b2f(X[at]) - px;
        yv = b2f(Y[at]) - py;
      }
      sx[r][q] = xv;
      sy[r][q] = yv;
    }
    __syncthreads();
    // horizontal pass
    for (int i = tid; i < SSIM_PH * SSIM_TW; i += SSIM_NT) {
      const int r = i / SSIM_TW, j = i % SSIM_TW;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
      #pragma unroll
      for (int k = 0; k < SSIM_K; ++k) {
        const float g = win.g[k];
        const float xv = sx[r][j + k], yv = sy[r][j + k];
        s0 += g * xv;
        s1 += g * yv;
        s2 += g * (xv * xv);
        s3 += g * (yv * yv);
        s4 += g * (xv * yv);
      }
      hm[0][r][j] = s0;
      hm[1][r][j] = s1;
      hm[2][r][j] = s2;
      hm[3][r][j] = s3;
      hm[4][r][j] = s4;
    }
    __syncthreads();
    // vertical pass of this thread's window, then S
    float mx = 0.f, my = 0.f, qx = 0.f, qy = 0.f, p = 0.f;
    #pragma unroll
    for (int k = 0; k < SSIM_K; ++k) {
      const float g = win.g[k];
      mx += g * hm[0][ty + k][tx];
      my += g * hm[1][ty + k][tx];
      qx += g * hm[2][ty + k][tx];
      qy += g * hm[3][ty + k][tx];
      p += g * hm[4][ty + k][tx];
    }
    if (live) {
      // Contraction off: every product rounds on its own, so that at
      // y == x (mx == my, qx == qy == p bitwise) A1 == B1 and A2 == B2
      // bitwise, S is exactly 1, ay and ax exactly 0 and c exactly -2 b.
      // An fma would round mx*mx + my*my differently from 2 (mx*my).
      #pragma clang fp contract(off)
      // central moments from the shifted ones, then the means shift back
      const float A2 = 2.f * (p - mx * my) + c2;
      const float B2 = (qx - mx * mx) + (qy - my * my) + c2;
      mx += px;
      my += py;
      const float A1 = 2.f * (mx * my) + c1;
      const float B1 = mx * mx + my * my + c1;
      const float r1 = A1 / B1, ib2 = 1.f / B2;
      const float S = r1 * (A2 / B2);
      acc += S;
      if (bm) {
        const long at = (((long)b * OH + oh) * OW + ow) * C + c;
        const float dA = A2 - A1, dB = S * (B2 - B1);
        const float sc = 2.f * ib2 / B1;
        if (ay) ay[at] = (mx * dA - my * dB) * sc;
        if (ax) ax[at] = (my * dA - mx * dB) * sc;
        bm[at] = -S * ib2;
        cm[at] = 2.f * r1 * ib2;
      }
    }
    __syncthreads();  // sx/sy/hm are rewritten by the next channel
  }

  #pragma unroll
  for (int off = 32; off; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    #pragma unroll
    for (int k = 0; k < SSIM_NT / 64; ++k) s += red[k];
    atomicAdd(&out[b], s * inv_n);
  }
}

// grid (tiles_w, tiles_h, B) over PIXELS. Gradient by Y of
// mean-SSIM(X, Y) given am = dS/dE[y], bm, cm on the OH x OW window grid.
__global__ __launch_bounds__(SSIM_NT) void ssim_bwd_kernel(
    const short* __restrict__ X, const short* __restrict__ Y,
    const float* __restrict__ am, const float* __restrict__ bm,
    const float* __restrict__ cm, const float* __restrict__ dout,
    short* __restrict__ dY, int H, int W, int C, SsimWin win, float inv_n) {
  __shared__ float sp[3][SSIM_PH][SSIM_PS];
  __shared__ float hm[3][SSIM_PH][SSIM_TW];

  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int OH = H - (SSIM_K - 1), OW = W - (SSIM_K - 1);
  const int h0 = blockIdx.y * SSIM_TH, w0 = blockIdx.x * SSIM_TW;
  const int ty = tid / SSIM_TW, tx = tid % SSIM_TW;
  const int h = h0 + ty, w = w0 + tx;
  const bool live = h < H && w < W;
  const long img = (long)b * H * W * C;
  const long grid0 = (long)b * OH * OW * C;
  const float scale = dout[b] * inv_n;

  for (int c = 0; c < C; ++c) {
    // patch[r][q] = map[h0 - 10 + r][w0 - 10 + q], zero off the window grid
    for (int i = tid; i < SSIM_PH * SSIM_PW; i += SSIM_NT) {
      const int r = i / SSIM_PW, q = i % SSIM_PW;
      const int gh = h0 - (SSIM_K - 1) + r, gw = w0 - (SSIM_K - 1) + q;
      float v0 = 0.f, v1 = 0.f, v2 = 0.f;
      if (gh >= 0 && gh < OH && gw >= 0 && gw < OW) {
        const long at = grid0 + ((long)gh * OW + gw) * C + c;
        v0 = am[at];
        v1 = bm[at];
        v2 = cm[at];
      }
      sp[0][r][q] = v0;
      sp[1][r][q] = v1;
      sp[2][r][q] = v2;
    }
    __syncthreads();
    // pixel column w0+j takes tap k from window column w0+j-k
    for (int i = tid; i < SSIM_PH * SSIM_TW; i += SSIM_NT) {
      const int r = i / SSIM_TW, j = i % SSIM_TW;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
      #pragma unroll
      for (int k = 0; k < SSIM_K; ++k) {
        const float g = win.g[k];
        const int q = j + (SSIM_K - 1) - k;
        s0 += g * sp[0][r][q];
        s1 += g * sp[1][r][q];
        s2 += g * sp[2][r][q];
      }
      hm[0][r][j] = s0;
      hm[1][r][j] = s1;
      hm[2][r][j] = s2;
    }
    __syncthreads();
    float ta = 0.f, tb = 0.f, tc = 0.f;
    #pragma unroll
    for (int k = 0; k < SSIM_K; ++k) {
      const float g = win.g[k];
      const int r = ty + (SSIM_K - 1) - k;
      ta += g * hm[0][r][tx];
      tb += g * hm[1][r][tx];
      tc += g * hm[2][r][tx];
    }
    if (live) {
      const long at = img + ((long)h * W + w) * C + c;
      const float xv = b2f(X[at]), yv = b2f(Y[at]);
      float v;
      {
        // each product rounds on its own: at y == x the map c is exactly
        // -2 b, and the last two terms must cancel exactly, not up to the
        // rounding of one of them as they would inside an fma
        #pragma clang fp contract(off)
        const float t1 = (2.f * yv) * tb;
        const float t2 = xv * tc;
        v = (ta + (t1 + t2)) * scale;
      }
      dY[at] = f2b(v);
    }
    __syncthreads();
  }
}

static void ssim_check_launch(const char* who) {
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, who, ": launch failed: ",
              hipGetErrorString(err));
}

static SsimWin ssim_window() {
  double g[SSIM_K], s = 0.0;
  for (int k = 0; k < SSIM_K; ++k) {
    const double d = k - (SSIM_K - 1) / 2;
    g[k] = std::exp(-d * d / (2.0 * 1.5 * 1.5));
    s += g[k];
  }
  SsimWin w;
  for (int k = 0; k < SSIM_K; ++k) w.g[k] = (float)(g[k] / s);
  return w;
}

// the checks both entry points share
static void ssim_check_images(const at::Tensor& x, const at::Tensor& y,
                              const char* who) {
  TORCH_CHECK(x.is_cuda() && y.is_cuda(), who, ": inputs must be cuda tensors");
  TORCH_CHECK(x.dim() == 4 && y.dim() == 4, who, ": inputs must be [B,H,W,C]");
  TORCH_CHECK(x.scalar_type() == y.scalar_type(), who,
              ": inputs must share one dtype");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, who,
              ": only bfloat16 inputs are supported");
  TORCH_CHECK(x.sizes() == y.sizes(), who, ": input shapes differ");
  TORCH_CHECK(x.is_contiguous() && y.is_contiguous(), who,
              ": inputs must be contiguous");
  TORCH_CHECK(x.get_device() == y.get_device(), who,
              ": inputs on different devices");
  TORCH_CHECK(x.size(1) >= SSIM_K && x.size(2) >= SSIM_K, who,
              ": H and W must be at least ", SSIM_K);
  // int H, W, C in the kernels; grid y/z limits, and grid.x * 256 threads
  // below 2^32 (at most 2^24 - 1 tiles a row); element offsets are long
  TORCH_CHECK(x.size(0) <= 65535, who, ": batch larger than 65535");
  TORCH_CHECK(x.size(1) <= 65535L * SSIM_TH &&
              x.size(2) <= ((1L << 24) - 1) * SSIM_TW &&
              x.size(3) <= 0x7fffffffL, who, ": image too large");
  TORCH_CHECK(x.numel() <= (1L << 46), who, ": too many elements");
}

// -> {out[B]} or, with save_maps 1: {out, ay, b, c}; 2: {out, ay, b, c, ax}.
// ay/ax: derivative maps for the gradient by y_pred / y_true.
std::vector<at::Tensor> ssim_fwd(at::Tensor x, at::Tensor y,
                                 int64_t save_maps) {
  ssim_check_images(x, y, "ssim_fwd");
  TORCH_CHECK(save_maps >= 0 && save_maps <= 2, "ssim_fwd: save_maps in 0..2");
  const long B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const long OH = H - (SSIM_K - 1), OW = W - (SSIM_K - 1);
  auto fopt = x.options().dtype(at::kFloat);
  auto out = at::zeros({B}, fopt);  // on the current stream
  std::vector<at::Tensor> res{out};
  float *ay = nullptr, *ax = nullptr, *bm = nullptr, *cm = nullptr;
  if (save_maps)  // also for an empty batch: the result keeps its length
    for (int i = 0; i < (save_maps == 2 ? 4 : 3); ++i)
      res.push_back(at::empty({B, OH, OW, C}, fopt));
  if (B == 0 || C == 0) return res;
  if (save_maps) {
    ay = (float*)res[1].mutable_data_ptr();
    bm = (float*)res[2].mutable_data_ptr();
    cm = (float*)res[3].mutable_data_ptr();
    if (save_maps == 2) ax = (float*)res[4].mutable_data_ptr();
  }
  dim3 grid((unsigned)((OW + SSIM_TW - 1) / SSIM_TW),
            (unsigned)((OH + SSIM_TH - 1) / SSIM_TH), (unsigned)B);
  const double n = (double)OH * (double)OW * (double)C;
  hipLaunchKernelGGL(ssim_fwd_kernel, grid, dim3(SSIM_NT), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const short*)x.const_data_ptr(),
                     (const short*)y.const_data_ptr(),
                     (float*)out.mutable_data_ptr(), ay, ax, bm, cm, (int)H,
                     (int)W, (int)C, ssim_window(), 0.0004f, 0.0036f,
                     (float)(1.0 / n));
  ssim_check_launch("ssim_fwd");
  return res;
}

// gradient of sum_b dout[b] * SSIM(x, y)[b] by y, from the maps of ssim_fwd
// (am = ay). By x: ssim_bwd(y, x, ax, b, c, dout).
at::Tensor ssim_bwd(at::Tensor x, at::Tensor y, at::Tensor am, at::Tensor bm,
                    at::Tensor cm, at::Tensor dout) {
  ssim_check_images(x, y, "ssim_bwd");
  const long B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const long OH = H - (SSIM_K - 1), OW = W - (SSIM_K - 1);
  for (const at::Tensor* m : {&am, &bm, &cm}) {
    TORCH_CHECK(m->is_cuda() && m->scalar_type() == at::kFloat &&
                m->is_contiguous() && m->dim() == 4 &&
                m->get_device() == x.get_device(),
                "ssim_bwd: maps must be contiguous cuda fp32 [B,H-10,W-10,C]");
    TORCH_CHECK(m->size(0) == B && m->size(1) == OH && m->size(2) == OW &&
                m->size(3) == C, "ssim_bwd: map shape does not fit the inputs");
  }
  TORCH_CHECK(dout.is_cuda() && dout.scalar_type() == at::kFloat &&
              dout.is_contiguous() && dout.dim() == 1 && dout.size(0) == B &&
              dout.get_device() == x.get_device(),
              "ssim_bwd: dout must be a contiguous cuda fp32 [B]");
  auto dy = at::empty_like(y);
  if (B == 0 || C == 0) return dy;
  dim3 grid((unsigned)((W + SSIM_TW - 1) / SSIM_TW),
            (unsigned)((H + SSIM_TH - 1) / SSIM_TH), (unsigned)B);
  const double n = (double)OH * (double)OW * (double)C;
  hipLaunchKernelGGL(ssim_bwd_kernel, grid, dim3(SSIM_NT), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const short*)x.const_data_ptr(),
                     (const short*)y.const_data_ptr(),
                     (const float*)am.const_data_ptr(),
                     (const float*)bm.const_data_ptr(),
                     (const float*)cm.const_data_ptr(),
                     (const float*)dout.const_data_ptr(),
                     (short*)dy.mutable_data_ptr(), (int)H, (int)W, (int)C,
                     ssim_window(), (float)(1.0 / n));
  ssim_check_launch("ssim_bwd");
  return dy;
}

}  // namespace cyg
