// Common device helpers for the cyclegan_amd gfx950 kernels.
// CDNA4: wave64, MFMA bf16 16x16x32, LDS 160KiB/CU. Compiled only for
// --offload-arch=gfx950 (no multi-arch dispatch).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp8.h>

#define DEV __device__ __forceinline__

typedef __bf16 bf16r;
typedef bf16r v8bf __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef short v8s __attribute__((ext_vector_type(8)));
typedef short v4s __attribute__((ext_vector_type(4)));

// raw bf16 <-> f32 (RNE via hardware conversion)
DEV float b2f(short raw) {
  union { float f; unsigned u; } v;
  v.u = ((unsigned)(unsigned short)raw) << 16;
  return v.f;
}

DEV short f2b(float f) {
  __hip_bfloat16 h = __float2bfloat16(f);  // RNE
  return *reinterpret_cast<short*>(&h);
}

// ---- fp8 (OCP e4m3) delayed-scaling quantisation ----
// ONE definition of the scale and of the conversion, shared by the
// standalone quant kernels and the conv epilogue (conv.hip) and by the
// InstanceNorm kernel that emits its consumer's fp8 operand
// (norm_elem.hip): identical inputs give identical bytes everywhere.
// sx comes from the PREVIOUS step's amax (persistent per-layer slot).
DEV float delayed_sx(float amax_prev) {
  return fminf(448.f / fmaxf(amax_prev, 1e-12f), 65504.f);
}

// e4m3 byte of f * s (fp32 product, saturating RNE conversion)
DEV unsigned char f2e4m3(float f, float s) {
  __hip_fp8_e4m3 q(f * s);
  return q.__x;
}

// activation codes shared with python (ops/conv.py)
#define ACT_NONE 0
#define ACT_RELU 1
#define ACT_LRELU 2
#define ACT_TANH 3

DEV float apply_act(float v, int act, float slope) {
  switch (act) {
    case ACT_RELU: return v > 0.f ? v : 0.f;
    case ACT_LRELU: return v > 0.f ? v : v * slope;
    case ACT_TANH: return tanhf(v);
    default: return v;
  }
}

// reflect index into [0, n) for single reflection (pad < n)
DEV int mirror_idx(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return i;
}

#define CHECK_HIP(x) do { hipError_t e = (x); \
  if (e != hipSuccess) { \
    printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); \
  } } while (0)
