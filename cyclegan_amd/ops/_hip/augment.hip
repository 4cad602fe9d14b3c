// Fused input augmentation — gfx950.
//
// One launch turns raw uint8 images resident on the device into a
// normalised training batch:
//
//   out[b] = crop_{oy,ox,ch,cw}( resize_{rh,rw}( flip?( src[idx[b]] ) ) ) / 127.5 - 1
//
// (reference get_datasets map: flip-LR -> bilinear resize -> random crop ->
// normalise, reference main.py:18-83). params[n] = (flip, oy, ox) is
// indexed by SAMPLE n = idx[b]. Only the crop window is computed; the
// resized image never exists.
//
// Resize is data/pipeline.resize_bilinear (half-pixel centres, no
// antialias), all in fp32:
//   s  = max(0, (d + 0.5) * (in / out) - 0.5)
//   i0 = floor(s), i1 = min(i0 + 1, in - 1), lambda = s - i0
// The flip is applied to the source ("flip, then resize"): a tap at column
// x reads source column Ws-1-x with the same weight.
//
// Mapping: the output is one flat run of B*ch*cw*3 elements; a thread owns
// V consecutive elements (16 bytes) and writes them with one vector store,
// so a wave writes 1 KiB contiguous. The last, partial group and outputs
// whose base is not 16-byte aligned (V = 1) take scalar stores. The four
// u8 taps of neighbouring elements share cache lines; the kernel moves
// ~1.6 MB per B=4 batch and is nowhere near any roof.
//
// Range of idx / oy / ox is validated on the host where those tensors are
// built (ops/augment.py); tap coordinates are clamped into the image by
// the resize rule itself.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

namespace cyg {

constexpr int AUG_NT = 256;

struct AugGeom {
  int Hs, Ws;   // source image
  int rh, rw;   // resize target
  int ch, cw;   // crop window
};

template <typename T> struct AugOut;
template <> struct AugOut<float> {
  static constexpr int V = 4;
  typedef v4f vec;
  static DEV float cvt(float v) { return v; }
};
template <> struct AugOut<short> {  // raw bf16
  static constexpr int V = 8;
  typedef v8s vec;
  static DEV short cvt(float v) { return f2b(v); }  // RNE
};

// source coordinate of destination index d -> taps i0,i1 and weight lambda
DEV void aug_tap(int d, float scale, int in, int& i0, int& i1, float& lam) {
  float s = fmaxf(0.f, ((float)d + 0.5f) * scale - 0.5f);
  i0 = min((int)s, in - 1);
  i1 = min(i0 + 1, in - 1);
  lam = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}

// flat output element g -> normalised value
DEV float aug_value(const unsigned char* __restrict__ src,
                    const int* __restrict__ idx,
                    const int* __restrict__ params, const AugGeom& G,
                    float sy, float sx, long g) {
  const int row = G.cw * 3;
  int xc = (int)(g % row);
  long t = g / row;
  int y = (int)(t % G.ch);
  int b = (int)(t / G.ch);
  int x = xc / 3, c = xc - x * 3;

  int n = idx[b];
  const int* p = params + (long)n * 3;
  int flip = p[0], oy = p[1], ox = p[2];

  int y0, y1, x0, x1;
  float ly, lx;
  aug_tap(y + oy, sy, G.Hs, y0, y1, ly);
  aug_tap(x + ox, sx, G.Ws, x0, x1, lx);
  if (flip) {
    x0 = G.Ws - 1 - x0;
    x1 = G.Ws - 1 - x1;
  }
  const unsigned char* img = src + (long)n * G.Hs * G.Ws * 3 + c;
  const unsigned char* r0 = img + (long)y0 * G.Ws * 3;
  const unsigned char* r1 = img + (long)y1 * G.Ws * 3;
  float v00 = (float)r0[x0 * 3], v01 = (float)r0[x1 * 3];
  float v10 = (float)r1[x0 * 3], v11 = (float)r1[x1 * 3];
  float wx0 = 1.f - lx, wy0 = 1.f - ly;
  float v = wy0 * (wx0 * v00 + lx * v01) + ly * (wx0 * v10 + lx * v11);
  return v / 127.5f - 1.0f;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(AUG_NT) void augment_batch_kernel(
    const unsigned char* __restrict__ src, const int* __restrict__ idx,
    const int* __restrict__ params, T* __restrict__ out, AugGeom G,
    long total) {
  constexpr int V = VEC ? AugOut<T>::V : 1;
  const float sy = (float)G.Hs / (float)G.rh;
  const float sx = (float)G.Ws / (float)G.rw;
  long g0 = ((long)blockIdx.x * AUG_NT + threadIdx.x) * V;
  if (g0 >= total) return;
  if constexpr (VEC) {
    if (g0 + V <= total) {
      typename AugOut<T>::vec o;
      #pragma unroll
      for (int j = 0; j < V; ++j)
        o[j] = AugOut<T>::cvt(aug_value(src, idx, params, G, sy, sx, g0 + j));
      *(typename AugOut<T>::vec*)(out + g0) = o;
      return;
    }
  }
  // scalar tail (and the whole output when its base is not 16-byte aligned)
  const long g1 = g0 + V < total ? g0 + V : total;
  for (long g = g0; g < g1; ++g)
    out[g] = AugOut<T>::cvt(aug_value(src, idx, params, G, sy, sx, g));
}

template <typename T>
static void augment_launch(const at::Tensor& src, const at::Tensor& idx,
                           const at::Tensor& params, at::Tensor& out,
                           const AugGeom& G, long total) {
  T* op = (T*)out.mutable_data_ptr();
  bool vec = ((uintptr_t)op % 16) == 0;
  long per = vec ? AugOut<T>::V : 1;
  long threads = (total + per - 1) / per;
  long blocks = (threads + AUG_NT - 1) / AUG_NT;
  TORCH_CHECK(blocks <= 0x7fffffffL, "augment_batch: output too large");
  auto stream = at::cuda::getCurrentCUDAStream();
  auto* sp = (const unsigned char*)src.const_data_ptr();
  auto* ip = (const int*)idx.const_data_ptr();
  auto* pp = (const int*)params.const_data_ptr();
  if (vec)
    hipLaunchKernelGGL((augment_batch_kernel<T, true>), dim3((unsigned)blocks),
                       dim3(AUG_NT), 0, stream, sp, ip, pp, op, G, total);
  else
    hipLaunchKernelGGL((augment_batch_kernel<T, false>), dim3((unsigned)blocks),
                       dim3(AUG_NT), 0, stream, sp, ip, pp, op, G, total);
}

at::Tensor augment_batch(at::Tensor src, at::Tensor idx, at::Tensor params,
                         int64_t rh, int64_t rw, at::Tensor out) {
  TORCH_CHECK(src.is_cuda() && src.scalar_type() == at::kByte &&
              src.is_contiguous() && src.dim() == 4 && src.size(3) == 3,
              "augment_batch: src must be a contiguous cuda uint8 [N,Hs,Ws,3]");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kInt &&
              idx.is_contiguous() && idx.dim() == 1,
              "augment_batch: idx must be a contiguous cuda int32 [B]");
  TORCH_CHECK(params.is_cuda() && params.scalar_type() == at::kInt &&
              params.is_contiguous() && params.dim() == 2 &&
              params.size(0) == src.size(0) && params.size(1) == 3,
              "augment_batch: params must be a contiguous cuda int32 [N,3]");
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.dim() == 4 &&
              out.size(0) == idx.size(0) && out.size(3) == 3 &&
              (out.scalar_type() == at::kBFloat16 ||
               out.scalar_type() == at::kFloat),
              "augment_batch: out must be a contiguous cuda bf16|fp32 [B,ch,cw,3]");
  TORCH_CHECK(src.get_device() == idx.get_device() &&
              src.get_device() == params.get_device() &&
              src.get_device() == out.get_device(),
              "augment_batch: tensors on different devices");
  int64_t Hs = src.size(1), Ws = src.size(2);
  int64_t ch = out.size(1), cw = out.size(2);
  TORCH_CHECK(src.size(0) >= 1 && Hs >= 1 && Ws >= 1 && ch >= 1 && cw >= 1,
              "augment_batch: empty image or crop");
  TORCH_CHECK(rh >= ch && rw >= cw, "augment_batch: resize (", rh, ",", rw,
              ") smaller than crop (", ch, ",", cw, ")");
  // per-image and per-row quantities stay int; bases are 64-bit in-kernel
  TORCH_CHECK(Hs * Ws * 3 <= 0x7fffffffL && rh <= (1 << 24) &&
              rw <= (1 << 24) && ch * cw * 3 <= 0x7fffffffL,
              "augment_batch: image too large");
  long total = (long)out.numel();
  if (total == 0) return out;  // B == 0: nothing to launch
  AugGeom G{(int)Hs, (int)Ws, (int)rh, (int)rw, (int)ch, (int)cw};
  if (out.scalar_type() == at::kFloat)
    augment_launch<float>(src, idx, params, out, G, total);
  else
    augment_launch<short>(src, idx, params, out, G, total);
  return out;
}

}  // namespace cyg
