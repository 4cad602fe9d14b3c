// Implicit-GEMM NHWC convolutions on gfx950 MFMA (bf16 in, fp32 accumulate).
//
// Three kernels cover every conv op in the framework:
//   conv_fwd_kernel   y[b,oh,ow,n] = act(Σ_{dk,ci} x[b,oh*s+dk-pt,ci]·w[n,dk,ci] + bias)
//                     (also conv_transpose dgrad, via the channel-transposed weight)
//   convt_fwd_kernel  y[b,i,j,n]   = act(Σ_{dk,ci; i=s*o+dk-pt} in[b,o,ci]·w[n,dk,ci] + bias)
//                     (also conv2d dgrad: same gather, channel-transposed weight, no tap flip)
//   wgrad_kernel      dw[n,dk,ci] += Σ_{b,o} x_patch[m,(dk,ci)]·dy[m,n]   (fp32, split-M atomics)
//
// GEMM view: M = B*OH*OW output pixels, N = Cout, K = KH*KW*Cin, with the
// im2col A-tile gathered on the fly (reflection padding = a load-index
// mirror, never materialized). Weights are OHWI so the B^T operand rows
// (fixed n, k contiguous) are vector loads AND single ds_read_b128 MFMA
// fragments.
//
// Tiling (conv_glds_kernel, the production path): BM=128 rows, BK=64,
// n-tile width 128/64/16 by Cout (8 waves for 128/64, Cout<=16 heads get
// 16-wide NF=1 tiles), glds (buffer_load_lds) double-buffered staging
// with the XOR bank swizzle riding the gather address, incremental
// im2col addressing, XCD-chunked blockIdx->tile mapping;
// mfma_f32_16x16x32_bf16 fragments: A row = lane&15, k = (lane>>4)*8..+8;
// D col = lane&15, row = (lane>>4)*4 + reg (verified by tests/test_ops_gpu.py
// via the mfma_probe binding and oracle comparisons). A halo-tiled direct
// head-conv kernel exists behind CYG_HALO=1 (see NOTES.md). The plain
// conv_gemm_kernel remains as the unaligned-channel fallback.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

namespace cyg {

constexpr int BM = 128, BN = 64, BK = 64;
constexpr int NTHREADS = 256;
constexpr int LDK = BK + 8;  // +16B pad: conflict-free b128 column-of-rows reads

struct ConvParams {
  const short* __restrict__ x;   // [B,H,W,Cin] bf16 raw
  const short* __restrict__ w;   // [Cout,KH,KW,Cin] bf16 raw
  const short* __restrict__ bias;  // [Cout] bf16 or null
  short* __restrict__ y;         // [B,OH,OW,Cout]
  int B, H, W, Cin, OH, OW, Cout, KH, KW;
  int stride, pt, pl;
  int reflect;                   // conv_fwd only
  int act;  float slope;
  const float* dq;               // fp8: amax_prev (with dqb) or 1/(sx*sw)
  const float* dqb;              // fp8 delayed-scaling: sw scalar
  long M, KTOT;
  int mtiles, ntiles;
  // optional InstanceNorm partial slabs written by conv_glds_kernel's
  // epilogue (null = off): per-(M-tile, channel) sums of the bf16-rounded
  // outputs and their squares, laid out [(slice*B + b)*Cout + n] with
  // slice = the tile's index within its sample. tps = M-tiles per sample
  // (per sample and phase class for the phased convT); the host enables
  // this only when every tile lies inside one sample.
  float* psum;
  float* psq;
  int tps;
};

// XCD-aware block remap: hardware dispatches blockIdx round-robin over the
// 8 XCDs, so consecutive tiles (which gather overlapping input rows) land
// in different XCDs' L2s and each L2 re-pulls the same lines from HBM.
// Chunking gives every XCD a CONTIGUOUS tile range: XCD k executes blocks
// k, k+8, k+16, ... which remap to tiles k*nb/8 + 0, 1, 2, ...
DEV int xcd_chunk(int bid, int nb) {
  return (nb % 8 == 0) ? (bid % 8) * (nb / 8) + bid / 8 : bid;
}

// ---------------- shared GEMM core ----------------
// As rows = m (output pixel), Bs rows = n (cout); both k-contiguous.

template <bool IS_CONVT, bool ALIGNED, int STRIDE>
__global__ __launch_bounds__(NTHREADS) void conv_gemm_kernel(ConvParams p) {
  const int stride = STRIDE ? STRIDE : p.stride;
  __shared__ short As[BM][LDK];
  __shared__ short Bs[BN][LDK];
  __shared__ long rowxb[BM];    // batch base offset into x
  __shared__ long rowyb[BM];    // output base offset (elements)
  __shared__ int rowih[BM], rowiw[BM];  // gather base coords (see below)
  __shared__ char rowok[BM];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int bid = xcd_chunk(blockIdx.x, gridDim.x);
  const int mt = bid % p.mtiles, nt = bid / p.mtiles;
  const long m0 = (long)mt * BM;
  const int n0 = nt * BN;

  // ---- per-row precompute (constant across the K loop) ----
  for (int r = tid; r < BM; r += NTHREADS) {
    long m = m0 + r;
    bool ok = m < p.M;
    long mm = ok ? m : 0;
    int ow = (int)(mm % p.OW);
    int oh = (int)((mm / p.OW) % p.OH);
    int b = (int)(mm / ((long)p.OW * p.OH));
    rowok[r] = ok;
    rowxb[r] = (long)b * p.H * p.W * p.Cin;
    rowyb[r] = ((long)(b * p.OH + oh) * p.OW + ow) * p.Cout;
    if (IS_CONVT) {
      rowih[r] = oh + p.pt;   // output coord + pad (gather: o = (i+pt-dk)/s)
      rowiw[r] = ow + p.pl;
    } else {
      rowih[r] = oh * stride - p.pt;
      rowiw[r] = ow * stride - p.pl;
    }
  }
  __syncthreads();

  v4f acc[4][2] = {};

  const int wr = wid >> 1, wc = wid & 1;
  const int wm0 = wr * 64, wn0 = wc * 32;
  const int fr = lane & 15;          // fragment row-in-16
  const int fg = lane >> 4;          // k-group 0..3

  for (long k0 = 0; k0 < p.KTOT; k0 += BK) {
    // ---- stage A (im2col gather) ----
    if (ALIGNED) {
      #pragma unroll 2
      for (int c = tid; c < BM * (BK / 8); c += NTHREADS) {
        int row = c >> 3;
        int kc = (c & 7) * 8;
        long k = k0 + kc;
        v8s val = {};
        if (k < p.KTOT && rowok[row]) {
          int tap = (int)(k / p.Cin);
          int ci = (int)(k - (long)tap * p.Cin);
          int dkh = tap / p.KW, dkw = tap - (tap / p.KW) * p.KW;
          bool valid = true;
          int ih, iw;
          if (IS_CONVT) {
            int nh = rowih[row] - dkh, nw = rowiw[row] - dkw;
            valid = nh >= 0 && nw >= 0 && (nh % stride) == 0 &&
                    (nw % stride) == 0;
            ih = nh / stride; iw = nw / stride;
            valid = valid && ih < p.H && iw < p.W;
          } else {
            ih = rowih[row] + dkh; iw = rowiw[row] + dkw;
            if (p.reflect) {
              ih = mirror_idx(ih, p.H); iw = mirror_idx(iw, p.W);
            } else {
              valid = ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
            }
          }
          if (valid)
            val = *(const v8s*)(p.x + rowxb[row] + ((long)ih * p.W + iw) * p.Cin + ci);
        }
        *(v8s*)&As[row][kc] = val;
      }
    } else {  // generic scalar path (Cin % 8 != 0, e.g. the RGB stem)
      for (int c = tid; c < BM * BK; c += NTHREADS) {
        int row = c >> 6;          // BK = 64
        int kc = c & 63;
        long k = k0 + kc;
        short val = 0;
        if (k < p.KTOT && rowok[row]) {
          int tap = (int)(k / p.Cin);
          int ci = (int)(k - (long)tap * p.Cin);
          int dkh = tap / p.KW, dkw = tap - (tap / p.KW) * p.KW;
          bool valid = true;
          int ih, iw;
          if (IS_CONVT) {
            int nh = rowih[row] - dkh, nw = rowiw[row] - dkw;
            valid = nh >= 0 && nw >= 0 && (nh % stride) == 0 &&
                    (nw % stride) == 0;
            ih = nh / stride; iw = nw / stride;
            valid = valid && ih < p.H && iw < p.W;
          } else {
            ih = rowih[row] + dkh; iw = rowiw[row] + dkw;
            if (p.reflect) {
              ih = mirror_idx(ih, p.H); iw = mirror_idx(iw, p.W);
            } else {
              valid = ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
            }
          }
          if (valid)
            val = p.x[rowxb[row] + ((long)ih * p.W + iw) * p.Cin + ci];
        }
        As[row][kc] = val;
      }
    }

    // ---- stage B^T (weight rows, k contiguous) ----
    if (ALIGNED) {
      #pragma unroll 2
      for (int c = tid; c < BN * (BK / 8); c += NTHREADS) {
        int n = c >> 3;
        int kc = (c & 7) * 8;
        long k = k0 + kc;
        v8s val = {};
        if (n0 + n < p.Cout && k < p.KTOT)
          val = *(const v8s*)(p.w + (long)(n0 + n) * p.KTOT + k);
        *(v8s*)&Bs[n][kc] = val;
      }
    } else {
      for (int c = tid; c < BN * BK; c += NTHREADS) {
        int n = c >> 6;
        int kc = c & 63;
        long k = k0 + kc;
        Bs[n][kc] = (n0 + n < p.Cout && k < p.KTOT)
                        ? p.w[(long)(n0 + n) * p.KTOT + k] : (short)0;
      }
    }
    __syncthreads();

    // ---- MFMA: 2 k-substeps of 32 ----
    #pragma unroll
    for (int kk = 0; kk < BK; kk += 32) {
      v8bf a0 = *(const v8bf*)&As[wm0 + 0 * 16 + fr][kk + fg * 8];
      v8bf a1 = *(const v8bf*)&As[wm0 + 1 * 16 + fr][kk + fg * 8];
      v8bf a2 = *(const v8bf*)&As[wm0 + 2 * 16 + fr][kk + fg * 8];
      v8bf a3 = *(const v8bf*)&As[wm0 + 3 * 16 + fr][kk + fg * 8];
      v8bf b0 = *(const v8bf*)&Bs[wn0 + 0 * 16 + fr][kk + fg * 8];
      v8bf b1 = *(const v8bf*)&Bs[wn0 + 1 * 16 + fr][kk + fg * 8];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[1][1], 0, 0, 0);
      acc[2][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b0, acc[2][0], 0, 0, 0);
      acc[2][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b1, acc[2][1], 0, 0, 0);
      acc[3][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a3, b0, acc[3][0], 0, 0, 0);
      acc[3][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a3, b1, acc[3][1], 0, 0, 0);
    }
    __syncthreads();
  }

  // ---- epilogue: bias + activation + bf16 store ----
  #pragma unroll
  for (int nf = 0; nf < 2; ++nf) {
    int n = n0 + wn0 + nf * 16 + fr;
    if (n >= p.Cout) continue;
    float bv = p.bias ? b2f(p.bias[n]) : 0.f;
    #pragma unroll
    for (int mf = 0; mf < 4; ++mf) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        int rl = wm0 + mf * 16 + fg * 4 + r;
        if (!rowok[rl]) continue;
        float v = apply_act(acc[mf][nf][r] + bv, p.act, p.slope);
        p.y[rowyb[rl] + n] = f2b(v);
      }
    }
  }
}

// ---------------- glds pipelined conv GEMM ----------------
// Same math as conv_gemm_kernel, but staged by LDS-DMA
// (buffer_load_dwordx4 ... lds) with double-buffered LDS and an XOR
// swizzle. The swizzle and the out-of-bounds zero-fill both ride on the
// per-lane GATHER address: the LDS image is lane-linear (glds requirement),
// the source lane->element permutation implements byte ^= ((row&7)<<4),
// and invalid taps (padding, stride phase, M-tail) get an OOB voffset that
// the buffer descriptor turns into zeros. One __shared__ object only
// (hipcc de-pipelines glds next to a second one).

template <int NBUF, int BNT = BN>
struct ConvSmemT {
  // small arrays first: keeps their ds offsets within the 16-bit
  // immediate range even when the tile images exceed 64 KiB
  long rowyb[BM];
  int rowih[BM], rowiw[BM];
  unsigned rowxb[BM];  // byte offset of batch base (tensors < 4 GiB)
  char rowok[BM];
  char _pad[16 - (BM % 16 ? BM % 16 : 16)];
  short A[NBUF][BM * BK];
  short Bt[NBUF][BNT * BK];
};
using ConvSmem = ConvSmemT<2>;

template <bool IS_CONVT, int STRIDE, int NBUF = 2, int NW = 4, int BNT = BN,
          bool PHASED = false>
__global__ __launch_bounds__(NW * 64) void conv_glds_kernel(ConvParams p) {
  constexpr int NT = NW * 64;        // threads
  constexpr int API = 16 / NW;       // A glds instructions per wave
  constexpr int TBI = BNT / 8;       // B glds instructions total
  constexpr int BPI = TBI >= NW ? TBI / NW : 1;  // per wave (maybe idle)
  constexpr int NF = BNT >= 32 ? 2 : 1;  // n-fragments per wave
  constexpr int NWC = BNT / (NF * 16);   // wave-grid columns
  constexpr int NWR = NW / NWC;      // wave-grid rows
  constexpr int MF = (BM / NWR) / 16;  // m-fragments per wave
  const int stride = STRIDE ? STRIDE : p.stride;
  // dynamic LDS (the BNT=128 image exceeds the 64 KiB static limit);
  // ONE region, 16-B aligned (G17), opted-in at launch time.
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  auto& sm = *reinterpret_cast<ConvSmemT<NBUF, BNT>*>(smem_raw);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  // stride-2 convT-gather decode prefers the hardware round-robin (its
  // taps scatter anyway and chunking hotspots DRAM channels): measured
  // -25% on the s2 dgrad shape, +6% on the K3 forward.
  const int bid = (IS_CONVT && STRIDE == 2)
                      ? blockIdx.x : xcd_chunk(blockIdx.x, gridDim.x);
  const int mt = bid % p.mtiles, nt = bid / p.mtiles;
  const int n0 = nt * BNT;

  // PHASED (convT stride-2 only): the M space is regrouped into 4 output
  // phase classes; each tile enumerates ONLY its phase's taps (KEFF =
  // nvh*nvw*Cin), removing the 3/4 structural-zero gather waste.
  static_assert(!PHASED || (IS_CONVT && STRIDE == 2), "PHASED");
  const int tpp = PHASED ? (p.mtiles >> 2) : 0;
  const int phase = PHASED ? mt / tpp : 0;
  const int phh = phase >> 1, phw = phase & 1;
  const int OH2 = p.OH >> 1, OW2 = p.OW >> 1;
  const long m0 = PHASED ? (long)(mt - phase * tpp) * BM : (long)mt * BM;
  const int nvh = PHASED ? ((p.KH - phh + 1) >> 1) : 0;
  const int nvw = PHASED ? ((p.KW - phw + 1) >> 1) : 0;
  const long KEFF = PHASED ? (long)nvh * nvw * p.Cin : p.KTOT;

  for (int r = tid; r < BM; r += NT) {
    if (PHASED) {
      long mp = m0 + r;
      long Mp = (long)p.B * OH2 * OW2;
      bool ok = mp < Mp;
      long mm = ok ? mp : 0;
      int owp = (int)(mm % OW2);
      int ohp = (int)((mm / OW2) % OH2);
      int b = (int)(mm / ((long)OW2 * OH2));
      int i = 2 * ohp + ((phh + p.pt) & 1);
      int j = 2 * owp + ((phw + p.pl) & 1);
      sm.rowok[r] = ok && i < p.OH && j < p.OW;
      sm.rowxb[r] = (unsigned)((long)b * p.H * p.W * p.Cin * 2);
      sm.rowyb[r] = ((long)(b * p.OH + i) * p.OW + j) * p.Cout;
      sm.rowih[r] = (i + p.pt - phh) >> 1;  // oh = this - vh
      sm.rowiw[r] = (j + p.pl - phw) >> 1;
    } else {
      long m = m0 + r;
      bool ok = m < p.M;
      long mm = ok ? m : 0;
      int ow = (int)(mm % p.OW);
      int oh = (int)((mm / p.OW) % p.OH);
      int b = (int)(mm / ((long)p.OW * p.OH));
      sm.rowok[r] = ok;
      sm.rowxb[r] = (unsigned)((long)b * p.H * p.W * p.Cin * 2);
      sm.rowyb[r] = ((long)(b * p.OH + oh) * p.OW + ow) * p.Cout;
      if (IS_CONVT) {
        sm.rowih[r] = oh + p.pt;
        sm.rowiw[r] = ow + p.pl;
      } else {
        sm.rowih[r] = oh * stride - p.pt;
        sm.rowiw[r] = ow * stride - p.pl;
      }
    }
  }
  __syncthreads();

  // per-lane persistent gather state
  const int lr = lane >> 3;                    // row-in-8 of each instr
  const int klog = ((lane & 7) ^ lr) << 3;     // swizzled k-chunk (elems)
  int aih[API], aiw[API];
  unsigned axb[API];
  bool aok[API];
  #pragma unroll
  for (int j = 0; j < API; ++j) {
    int r = (w * API + j) * 8 + lr;
    aih[j] = sm.rowih[r];
    aiw[j] = sm.rowiw[r];
    axb[j] = sm.rowxb[r];
    aok[j] = sm.rowok[r];
  }
  int bn[BPI];
  #pragma unroll
  for (int j = 0; j < BPI; ++j) bn[j] = (w * BPI + j) * 8 + lr + n0;
  const bool bw_on = w * BPI < TBI;  // waves beyond TBI stage no B
  static_assert(BNT == 16 || BNT == 64 || BNT == 128, "BNT");

  auto rx = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.x, 0, (unsigned)((long)p.B * p.H * p.W * p.Cin * 2), 0x00020000);
  auto rw = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.w, 0, (unsigned)(p.Cout * p.KTOT * 2), 0x00020000);

  const int nk = (int)((KEFF + BK - 1) / BK);
  const bool big_ci = p.Cin >= BK;  // wave-uniform

  // incremental gather state: recompute voffsets only at tap boundaries
  // (every Cin/64 K-steps); otherwise one predicated add per instruction.
  long kcur;
  bool kv;
  int ci, dkh, dkw;  // PHASED: dkh/dkw hold (vh, vw)
  unsigned avo[API];
  bool avalid[API];
  unsigned bvo[BPI];
  bool bnv[BPI];

  auto recompute_a = [&]() {
    #pragma unroll
    for (int j = 0; j < API; ++j) {
      avalid[j] = false;
      avo[j] = 0xFF000000u;
      if (!aok[j]) continue;
      bool valid = true;
      int ih, iw;
      if (PHASED) {
        ih = aih[j] - dkh; iw = aiw[j] - dkw;  // oh = base - vh
        valid = ih >= 0 && iw >= 0 && ih < p.H && iw < p.W;
      } else if (IS_CONVT) {
        int nh = aih[j] - dkh, nw = aiw[j] - dkw;
        valid = nh >= 0 && nw >= 0 && (nh % stride) == 0 && (nw % stride) == 0;
        ih = nh / stride; iw = nw / stride;
        valid = valid && ih < p.H && iw < p.W;
      } else {
        ih = aih[j] + dkh; iw = aiw[j] + dkw;
        if (p.reflect) {
          ih = mirror_idx(ih, p.H); iw = mirror_idx(iw, p.W);
        } else {
          valid = ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
        }
      }
      if (valid) {
        avalid[j] = true;
        avo[j] = axb[j] + (unsigned)((((long)ih * p.W + iw) * p.Cin + ci) * 2);
      }
    }
  };

  auto recompute_b = [&]() {
    long kw_idx = kcur;
    if (PHASED)
      kw_idx = ((long)(2 * dkh + phh) * p.KW + (2 * dkw + phw)) * p.Cin + ci;
    #pragma unroll
    for (int j = 0; j < BPI; ++j)
      bvo[j] = (unsigned)(((long)bn[j] * p.KTOT + kw_idx) * 2);
  };

  auto decode_tap = [&]() {
    int tap = (int)(kcur / p.Cin);
    ci = (int)(kcur - (long)tap * p.Cin);
    if (PHASED) {
      dkh = tap / nvw;          // vh
      dkw = tap - dkh * nvw;    // vw
    } else {
      dkh = tap / p.KW;
      dkw = tap - dkh * p.KW;
    }
  };

  auto init_state = [&]() {
    kcur = klog;
    kv = kcur < KEFF;
    decode_tap();
    recompute_a();
    #pragma unroll
    for (int j = 0; j < BPI; ++j) bnv[j] = bn[j] < p.Cout;
    recompute_b();
  };

  auto advance = [&]() {
    kcur += BK;
    kv = kcur < KEFF;
    if (big_ci) {
      ci += BK;
      if (ci >= p.Cin) {
        ci -= p.Cin;
        if (PHASED) {
          if (++dkw == nvw) { dkw = 0; ++dkh; }
        } else {
          if (++dkw == p.KW) { dkw = 0; ++dkh; }
        }
        recompute_a();
        recompute_b();
      } else {
        #pragma unroll
        for (int j = 0; j < API; ++j) avo[j] += BK * 2;
        #pragma unroll
        for (int j = 0; j < BPI; ++j) bvo[j] += BK * 2;
      }
    } else {
      // Cin < 64: a K-step crosses several taps — full recompute
      decode_tap();
      recompute_a();
      recompute_b();
    }
  };

  auto stage = [&](int buf) {
    #pragma unroll
    for (int j = 0; j < API; ++j) {
      unsigned vo = (kv && avalid[j]) ? avo[j] : 0xFF000000u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rx, (__attribute__((address_space(3))) void*)&sm.A[buf][(w * API + j) * 512],
          16, vo, 0, 0, 0);
    }
    if (bw_on) {
      #pragma unroll
      for (int j = 0; j < BPI; ++j) {
        unsigned vo = (kv && bnv[j]) ? bvo[j] : 0xFF000000u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rw, (__attribute__((address_space(3))) void*)&sm.Bt[buf][(w * BPI + j) * 512],
            16, vo, 0, 0, 0);
      }
    }
  };

  v4f acc[MF][NF] = {};
  const int wr = w / NWC, wc = w % NWC;
  const int wm0 = wr * (MF * 16), wn0 = wc * (NF * 16);
  const int fr = lane & 15;
  const int fg = lane >> 4;
  const int swz = (fr & 7) << 4;  // read-side XOR (bytes)

  init_state();
  stage(0);
  __syncthreads();
#ifdef CYG_DEBUG_EPI
  if (bid == 0 && tid == 0)
    printf("dbg NW=%d BNT=%d API=%d TBI=%d BPI=%d NF=%d NWC=%d MF=%d nk=%d "
           "kv=%d klog=%d bvo0=%u bnv0=%d avo0=%u avalid0=%d "
           "A0123=%d %d %d %d Bt0123=%d %d %d %d\n",
           NW, BNT, API, TBI, BPI, NF, NWC, MF, nk, (int)kv, klog, bvo[0],
           (int)bnv[0], avo[0], (int)avalid[0],
           (int)sm.A[0][0], (int)sm.A[0][1], (int)sm.A[0][2], (int)sm.A[0][3],
           (int)sm.Bt[0][0], (int)sm.Bt[0][1], (int)sm.Bt[0][2],
           (int)sm.Bt[0][3]);
#endif

  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) {
      advance();
      stage((kt + 1) & 1);
    }
    const char* Ab = (const char*)sm.A[kt & 1];
    const char* Bb = (const char*)sm.Bt[kt & 1];
    #pragma unroll
    for (int kk = 0; kk < BK; kk += 32) {
      const int kbyte = (kk + fg * 8) * 2;
      v8bf a[MF], b[NF];
      #pragma unroll
      for (int mf = 0; mf < MF; ++mf)
        a[mf] = *(const v8bf*)(Ab + ((wm0 + mf * 16 + fr) << 7) + (kbyte ^ swz));
      #pragma unroll
      for (int nf = 0; nf < NF; ++nf)
        b[nf] = *(const v8bf*)(Bb + ((wn0 + nf * 16 + fr) << 7) + (kbyte ^ swz));
      #pragma unroll
      for (int mf = 0; mf < MF; ++mf)
        #pragma unroll
        for (int nf = 0; nf < NF; ++nf)
          acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[mf], b[nf], acc[mf][nf], 0, 0, 0);
    }
    __syncthreads();  // drains the in-flight glds (vmcnt(0) in the release)
  }

  // per-lane column sums of the stored (bf16-rounded) values and their
  // squares over this lane's MF*4 rows; lanes past Cout keep zeros
  float cs[NF] = {}, cq[NF] = {};
  #pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
    int n = n0 + wn0 + nf * 16 + fr;
    if (n >= p.Cout) continue;
    float bv = p.bias ? b2f(p.bias[n]) : 0.f;
    #pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        int rl = wm0 + mf * 16 + fg * 4 + r;
        if (!sm.rowok[rl]) continue;
#ifdef CYG_DEBUG_EPI
        if (sm.rowyb[rl] < 0 || sm.rowyb[rl] + n >= p.M * p.Cout) {
          printf("EPI OOB bid=%d tid=%d rl=%d rowyb=%ld n=%d\n",
                 bid, tid, rl, (long)sm.rowyb[rl], n);
          continue;
        }
#endif
        float v = apply_act(acc[mf][nf][r] + bv, p.act, p.slope);
        short hv = f2b(v);
        p.y[sm.rowyb[rl] + n] = hv;
        float fv = b2f(hv);
        cs[nf] += fv;
        cq[nf] += fv * fv;
      }
    }
  }

  // InstanceNorm partial slabs (block-uniform branch). Fixed-order
  // reduction, no atomics: the four lane>>4 row groups of a wave fold with
  // two xor shuffles, the NWR waves that share a column meet in LDS, and
  // one thread per column adds them in wave-row order. The final K-loop
  // barrier has retired every read of the staging buffers, so A[0]
  // (16 KiB >= NWR*BNT*2 floats) is free to hold the partials.
  if (p.psum != nullptr) {
    float* red = reinterpret_cast<float*>(sm.A[0]);  // [NWR][BNT][2]
    static_assert(NWR * BNT * 2 * sizeof(float) <= sizeof(sm.A[0]), "red");
    #pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      float s = cs[nf], q = cq[nf];
      s += __shfl_xor(s, 16, 64);
      q += __shfl_xor(q, 16, 64);
      s += __shfl_xor(s, 32, 64);
      q += __shfl_xor(q, 32, 64);
      if (fg == 0) {
        int col = wn0 + nf * 16 + fr;
        red[(wr * BNT + col) * 2] = s;
        red[(wr * BNT + col) * 2 + 1] = q;
      }
    }
    __syncthreads();
    if (tid < BNT && n0 + tid < p.Cout) {
      float s = 0.f, q = 0.f;
      #pragma unroll
      for (int k = 0; k < NWR; ++k) {
        s += red[(k * BNT + tid) * 2];
        q += red[(k * BNT + tid) * 2 + 1];
      }
      const int mtl = PHASED ? mt - phase * tpp : mt;
      const int b = mtl / p.tps;
      const int slice = phase * p.tps + (mtl - b * p.tps);
      const long o = ((long)slice * p.B + b) * p.Cout + n0 + tid;
      p.psum[o] = s;
      p.psq[o] = q;
    }
  }
}

// ---------------- halo-tiled direct conv (tiny-Cout heads) ----------------
// The generator head 7x7 (64->3, padded to 8) is gather-bound in the
// implicit-GEMM path: every input byte crosses the load path KH*KW times
// (1.6 GB through L2 for 34 MB of unique input). This kernel stages the
// whole input halo of an output-row tile in LDS ONCE and slides the
// filter window inside LDS, so HBM traffic drops to the unique bytes.
//
// One block = HB_BM consecutive output pixels of one output row.
// LDS: x halo [KH][HB_BM+KW-1][Cin] bf16, XOR ch-group swizzle riding the
//      glds SOURCE address (same trick as the GEMM tiles, guide rule 21);
//      w [nk][4 kgrp][8 n][8 bf16] staged by plain loads (n >= 8 MFMA
//      fragments read zero — Cout is exactly 8 after channel padding).
// Gate (host): stride 1, !convT, Cout == 8, Cin % 32 == 0, LDS fits.
constexpr int HB_BM = 64;

template <int NW = 4>
__global__ __launch_bounds__(NW * 64) void conv_halo_kernel(ConvParams p) {
  constexpr int NT = NW * 64;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int tiles_w = (p.OW + HB_BM - 1) / HB_BM;
  const int bid = xcd_chunk(blockIdx.x, gridDim.x);
  const int owt = bid % tiles_w;
  const int t2 = bid / tiles_w;
  const int oh = t2 % p.OH;
  const int b = t2 / p.OH;
  const int ow0 = owt * HB_BM;
  const int CW = HB_BM + p.KW - 1;
  constexpr int CG = 8;                 // Cin = 64 specialist (head convs)
  constexpr int SL = CG + 1;            // 9 slots/pixel: the pad slot makes
                                        // the pixel stride 36 words, which
                                        // spreads the 16 fragment lanes
                                        // over all 64 LDS banks (no XOR,
                                        // conflict-free ds_read_b128)
  constexpr int halves = 2;             // 32-elem K-steps per tap
  const int nk = p.KH * p.KW * halves;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  short* xs = (short*)smem_raw;                       // halo image
  const int xgr = p.KH * CW * SL;                     // halo granules
  const int xgr_pad = ((xgr + NT - 1) / NT) * NT;

  auto rx = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.x, 0, (unsigned)((long)p.B * p.H * p.W * p.Cin * 2),
      0x00020000);

  // ---- stage halo: glds, swizzle on the source ch-group ----
  // (row, col, chs) advance incrementally across rounds: NT granules =
  // NT/CG columns per step, so the loop runs without integer divisions
  // (runtime-divisor idiv is ~40 VALU cycles and this is a latency-
  // critical serial section at 1-2 blocks/CU).
  const long xbase = (long)b * p.H * p.W * p.Cin;
  {
    int g = w * 64 + lane;
    int chs = g % SL;                     // constexpr divisor: cheap
    int pix = g / SL;
    int col = pix % CW;                   // once; then incremental
    int row = pix / CW;
    constexpr int dpix = NT / SL;         // pixels advanced per round
    constexpr int dchs = NT - dpix * SL;  // slot advance per round
    for (int g0 = 0; g0 < xgr_pad; g0 += NT) {
      unsigned vo = 0xFF000000u;          // OOB (and pad slot) -> zeros
      if (row < p.KH && chs < CG) {
        int ih = oh - p.pt + row;
        int iw = ow0 - p.pl + col;
        bool okp = true;
        if (p.reflect) {
          ih = mirror_idx(ih, p.H);
          iw = mirror_idx(iw, p.W);
        } else {
          okp = ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
        }
        if (okp)
          vo = (unsigned)((xbase + ((long)ih * p.W + iw) * p.Cin + chs * 8) * 2);
      }
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rx, (__attribute__((address_space(3))) void*)(xs + (long)(g0 + w * 64) * 8),
          16, vo, 0, 0, 0);
      chs += dchs;
      col += dpix;
      if (chs >= SL) { chs -= SL; ++col; }
      while (col >= CW) { col -= CW; ++row; }
    }
  }

  __syncthreads();  // drains the halo glds (vmcnt(0))

  // ---- K loop: slide the window inside LDS ----
  // NW=8: waves pair up on each m-fragment and split the K range in half
  // (k-split), halving the per-wave latency chain; partials meet in LDS.
  constexpr int KSPLIT = NW >= 8 ? 2 : 1;
  const int mf = KSPLIT > 1 ? (w & 3) : w;
  const int kh2 = KSPLIT > 1 ? (w >> 2) : 0;
  const int fr = lane & 15;
  const int fg = lane >> 4;
  const int p0 = mf * 16;                 // wave's pixel base
  const v8bf bz = {};
  v4f acc = {};
  const int k0 = kh2 * (nk / KSPLIT);
  const int k1 = (kh2 == KSPLIT - 1) ? nk : (kh2 + 1) * (nk / KSPLIT);
  int tap = k0 / halves, h = k0 - tap * halves;
  int ty = tap / p.KW, tx = tap - ty * p.KW;
  #pragma unroll 8
  for (int kt = k0; kt < k1; ++kt) {
    int col = p0 + fr + tx;
    int chs = h * 4 + fg;
    v8bf a = *(const v8bf*)(xs + (((ty * CW + col) * SL + chs) << 3));
    // B straight from L2: the padded weight is 50 KB and shared by every
    // block; k = kt*32 + fg*8, contiguous per lane, pipelined by the
    // unroll. Keeping it OUT of LDS halves the block footprint -> 2
    // blocks/CU, which is what lets the next block's halo fill overlap
    // this block's MFMA tail.
    v8bf bf = bz;
    if (fr < 8)
      bf = *(const v8bf*)(p.w + (long)fr * p.KTOT + kt * 32 + fg * 8);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bf, acc, 0, 0, 0);
    if (++h == halves) {                  // advance (tap, half) counters
      h = 0;
      ++tap;
      if (++tx == p.KW) { tx = 0; ++ty; }
    }
  }

  if (KSPLIT > 1) {
    // meet the k-split partials in the (no longer needed) halo LDS
    __syncthreads();
    float* red = (float*)xs;
    if (kh2 == 1)
      *(v4f*)&red[(mf * 64 + lane) * 4] = acc;
    __syncthreads();
    if (kh2 != 0) return;
    acc += *(const v4f*)&red[(mf * 64 + lane) * 4];
  }

  // ---- epilogue: lane holds col n = fr, rows p0 + fg*4 + r ----
  if (fr < p.Cout) {
    float bv = p.bias ? b2f(p.bias[fr]) : 0.f;
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      int ow = ow0 + p0 + fg * 4 + r;
      if (ow >= p.OW) continue;
      float v = apply_act(acc[r] + bv, p.act, p.slope);
      p.y[(((long)b * p.OH + oh) * p.OW + ow) * p.Cout + fr] = f2b(v);
    }
  }
}

// ---------------- fp8 (e4m3) forward conv ----------------
// CDNA4 fp8 MFMA path (BASELINE config 5): activations and weights are
// quantized to OCP e4m3 with per-tensor scales; fp32 accumulate; the
// epilogue multiplies by 1/(sx*sw) before bias/activation. Byte-level tile
// geometry is IDENTICAL to the bf16 glds kernel (128-B rows, 16-B lane
// granules, same XOR swizzle) — a K-step covers 128 fp8 elements and runs
// 4 mfma_f32_16x16x32_fp8_fp8 substeps. Forward only: backward reuses the
// bf16 kernels from the saved bf16 activations (master-grad numerics).

constexpr int BKF = 128;  // fp8 K-step (elements == bytes)
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));

struct Fp8Smem {
  unsigned char A[2][BM * BKF];
  unsigned char Bt[2][BN * BKF];
  long rowyb[BM];
  int rowih[BM], rowiw[BM];
  unsigned rowxb[BM];  // byte offsets (1 B / element)
  char rowok[BM];
};

__global__ void quant_fp8_kernel(const short* __restrict__ x,
                                 const float* __restrict__ scale,
                                 unsigned char* __restrict__ y, long n) {
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  float s = scale[0];
  if (i + 8 <= n) {
    v8s v = *(const v8s*)(x + i);
    unsigned char out[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      out[j] = f2e4m3(b2f(v[j]), s);
    }
    *(uint2*)(y + i) = *(uint2*)out;
  } else if (i < n) {
    for (long k = i; k < n; ++k) {
      y[k] = f2e4m3(b2f(x[k]), scale[0]);
    }
  }
}

// ---- delayed-scaling quant ----
// sx comes from the PREVIOUS step's amax (persistent per-layer slot,
// transformer-engine style) so no separate full-tensor reduction runs
// before quantization; this call's max|x| block-reduces and atomically
// maxes into the CURRENT slot (nonneg float bits order == value order),
// rolled once per step by amax_roll. delayed_sx and the e4m3 conversion
// live in common.h.

__global__ __launch_bounds__(256) void quant_fp8_d_kernel(
    const short* __restrict__ x, const float* __restrict__ amax_prev,
    float* __restrict__ amax_cur, unsigned char* __restrict__ y, long n) {
  // grid-stride with a bounded grid: ONE same-address atomicMax per
  // block. (A block per 2048 elems meant ~6000 serialized atomics on one
  // MALL line — measured ~45 us per call; same-address atomics are
  // ~7 ns each.)
  const float s = delayed_sx(amax_prev[0]);
  float mx = 0.f;
  long t = (long)blockIdx.x * 256 + threadIdx.x;
  long nthreads = (long)gridDim.x * 256;
  for (long i = t * 8; i + 8 <= n; i += nthreads * 8) {
    v8s v = *(const v8s*)(x + i);
    unsigned char out[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = b2f(v[j]);
      mx = fmaxf(mx, fabsf(f));
      out[j] = f2e4m3(f, s);
    }
    *(uint2*)(y + i) = *(uint2*)out;
  }
  // tail (n not divisible by 8): first thread of block 0
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (long k = n & ~7L; k < n; ++k) {
      float f = b2f(x[k]);
      mx = fmaxf(mx, fabsf(f));
      y[k] = f2e4m3(f, s);
    }
  }
  __shared__ float red[256];
  red[threadIdx.x] = mx;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off)
      red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + off]);
    __syncthreads();
  }
  if (threadIdx.x == 0)
    atomicMax((unsigned*)amax_cur, __float_as_uint(red[0]));
}

__global__ void amax_roll_kernel(float* __restrict__ arena, int n, int cap) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    arena[i] = arena[cap + i];
    arena[cap + i] = 0.f;
  }
}

// STATS: also emit the InstanceNorm partial slabs (p.psum/p.psq/p.tps as
// in conv_glds_kernel). A template parameter, so the plain instantiation
// carries neither the extra accumulators nor the branch.
template <int STRIDE, bool STATS>
__global__ __launch_bounds__(NTHREADS) void conv_fp8_kernel(ConvParams p) {
  const int stride = STRIDE ? STRIDE : p.stride;
  __shared__ Fp8Smem sm;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int bid = xcd_chunk(blockIdx.x, gridDim.x);
  const int mt = bid % p.mtiles, nt = bid / p.mtiles;
  const long m0 = (long)mt * BM;
  const int n0 = nt * BN;
  const bool reflect = p.reflect != 0;

  for (int r = tid; r < BM; r += NTHREADS) {
    long m = m0 + r;
    bool ok = m < p.M;
    long mm = ok ? m : 0;
    int ow = (int)(mm % p.OW);
    int oh = (int)((mm / p.OW) % p.OH);
    int b = (int)(mm / ((long)p.OW * p.OH));
    sm.rowok[r] = ok;
    sm.rowxb[r] = (unsigned)((long)b * p.H * p.W * p.Cin);
    sm.rowyb[r] = ((long)(b * p.OH + oh) * p.OW + ow) * p.Cout;
    sm.rowih[r] = oh * stride - p.pt;
    sm.rowiw[r] = ow * stride - p.pl;
  }
  __syncthreads();

  const int lr = lane >> 3;
  const int klog = ((lane & 7) ^ lr) << 4;  // 16-elem granule
  int aih[4], aiw[4];
  unsigned axb[4];
  bool aok[4];
  #pragma unroll
  for (int j = 0; j < 4; ++j) {
    int r = w * 32 + j * 8 + lr;
    aih[j] = sm.rowih[r];
    aiw[j] = sm.rowiw[r];
    axb[j] = sm.rowxb[r];
    aok[j] = sm.rowok[r];
  }
  const int bn[2] = {(w * 2 + 0) * 8 + lr + n0, (w * 2 + 1) * 8 + lr + n0};

  auto rx = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.x, 0, (unsigned)((long)p.B * p.H * p.W * p.Cin), 0x00020000);
  auto rw = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.w, 0, (unsigned)(p.Cout * p.KTOT), 0x00020000);

  const int nk = (int)((p.KTOT + BKF - 1) / BKF);
  const bool big_ci = p.Cin >= BKF;

  long kcur;
  bool kv;
  int ci, dkh, dkw;
  unsigned avo[4], bvo[2];
  bool avalid[4], bnv[2];

  auto recompute_a = [&]() {
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      avalid[j] = false;
      avo[j] = 0xFF000000u;
      if (!aok[j]) continue;
      bool valid = true;
      int ih = aih[j] + dkh, iw = aiw[j] + dkw;
      if (reflect) {
        ih = mirror_idx(ih, p.H); iw = mirror_idx(iw, p.W);
      } else {
        valid = ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
      }
      if (valid) {
        avalid[j] = true;
        avo[j] = axb[j] + (unsigned)(((long)ih * p.W + iw) * p.Cin + ci);
      }
    }
  };

  auto init_state = [&]() {
    kcur = klog;
    kv = kcur < p.KTOT;
    int tap = (int)(kcur / p.Cin);
    ci = (int)(kcur - (long)tap * p.Cin);
    dkh = tap / p.KW;
    dkw = tap - dkh * p.KW;
    recompute_a();
    #pragma unroll
    for (int j = 0; j < 2; ++j) {
      bnv[j] = bn[j] < p.Cout;
      bvo[j] = (unsigned)((long)bn[j] * p.KTOT + kcur);
    }
  };

  auto advance = [&]() {
    kcur += BKF;
    kv = kcur < p.KTOT;
    #pragma unroll
    for (int j = 0; j < 2; ++j) bvo[j] += BKF;
    if (big_ci) {
      ci += BKF;
      if (ci >= p.Cin) {
        ci -= p.Cin;
        if (++dkw == p.KW) { dkw = 0; ++dkh; }
        recompute_a();
      } else {
        #pragma unroll
        for (int j = 0; j < 4; ++j) avo[j] += BKF;
      }
    } else {
      int tap = (int)(kcur / p.Cin);
      ci = (int)(kcur - (long)tap * p.Cin);
      dkh = tap / p.KW;
      dkw = tap - dkh * p.KW;
      recompute_a();
    }
  };

  auto stage = [&](int buf) {
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned vo = (kv && avalid[j]) ? avo[j] : 0xFF000000u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rx, (__attribute__((address_space(3))) void*)&sm.A[buf][(w * 4 + j) * 1024],
          16, vo, 0, 0, 0);
    }
    #pragma unroll
    for (int j = 0; j < 2; ++j) {
      unsigned vo = (kv && bnv[j]) ? bvo[j] : 0xFF000000u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rw, (__attribute__((address_space(3))) void*)&sm.Bt[buf][(w * 2 + j) * 1024],
          16, vo, 0, 0, 0);
    }
  };

  v4f acc[4][2] = {};
  const int wr = w >> 1, wc = w & 1;
  const int wm0 = wr * 64, wn0 = wc * 32;
  const int fr = lane & 15;
  const int fg = lane >> 4;
  const int swz = (fr & 7) << 4;

  init_state();
  stage(0);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) {
      advance();
      stage((kt + 1) & 1);
    }
    const char* Ab = (const char*)sm.A[kt & 1];
    const char* Bb = (const char*)sm.Bt[kt & 1];
    // ONE mfma_scale_f32_16x16x128_f8f6f4 consumes the whole 128-B K-row
    // (4x fewer matrix instructions than the 16x16x32 form). Fragment
    // (mapped empirically, tools/mx_map.py map16): lane l supplies
    // A[row = l%16][k = (l//16)*32 + b] for b = 0..31 — i.e. rows fr,
    // byte window fg*32..fg*32+31, read as two XOR-swizzled b128s.
    // Per-tensor scales are folded in the fp32 epilogue; sa = sb = 127
    // (E8M0 2^0) keeps the MFMA unscaled.
    {
      const int c0 = (fg * 32) ^ swz;
      const int c1 = (fg * 32 + 16) ^ swz;
      v8i fa[4], fb[2];
      #pragma unroll
      for (int mf = 0; mf < 4; ++mf) {
        const char* r = Ab + ((wm0 + mf * 16 + fr) << 7);
        v4i lo = *(const v4i*)(r + c0);
        v4i hi = *(const v4i*)(r + c1);
        fa[mf] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
      #pragma unroll
      for (int nf = 0; nf < 2; ++nf) {
        const char* r = Bb + ((wn0 + nf * 16 + fr) << 7);
        v4i lo = *(const v4i*)(r + c0);
        v4i hi = *(const v4i*)(r + c1);
        fb[nf] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
      #pragma unroll
      for (int mf = 0; mf < 4; ++mf)
        #pragma unroll
        for (int nf = 0; nf < 2; ++nf)
          acc[mf][nf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              fa[mf], fb[nf], acc[mf][nf], 0, 0, 0, 127, 0, 127);
    }
    __syncthreads();
  }

  const float dqs = p.dq
      ? (p.dqb ? 1.f / (delayed_sx(p.dq[0]) * p.dqb[0]) : p.dq[0])
      : 1.f;
  // STATS: per-lane column sums of the stored (bf16-rounded) values and
  // their squares over this lane's 16 rows; lanes past Cout keep zeros
  float cs[2] = {}, cq[2] = {};
  #pragma unroll
  for (int nf = 0; nf < 2; ++nf) {
    int n = n0 + wn0 + nf * 16 + fr;
    if (n >= p.Cout) continue;
    float bv = p.bias ? b2f(p.bias[n]) : 0.f;
    #pragma unroll
    for (int mf = 0; mf < 4; ++mf) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        int rl = wm0 + mf * 16 + fg * 4 + r;
        if (!sm.rowok[rl]) continue;
        float v = apply_act(acc[mf][nf][r] * dqs + bv, p.act, p.slope);
        short hv = f2b(v);
        p.y[sm.rowyb[rl] + n] = hv;
        if (STATS) {
          float fv = b2f(hv);
          cs[nf] += fv;
          cq[nf] += fv * fv;
        }
      }
    }
  }

  // InstanceNorm partial slabs, the epilogue of conv_glds_kernel on this
  // kernel's fixed 2x2-wave 128x64 tile: the four lane>>4 row groups fold
  // with two xor shuffles, the two wave rows meet in LDS, one thread per
  // column adds them in wave-row order. No atomics, fixed order. The
  // final K-loop barrier has retired every read of the staging buffers,
  // so A[0] (16 KiB >= 2*BN*2 floats) is free to hold the partials.
  if (STATS) {
    float* red = reinterpret_cast<float*>(sm.A[0]);  // [2][BN][2]
    static_assert(2 * BN * 2 * sizeof(float) <= sizeof(sm.A[0]), "red");
    #pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      float s = cs[nf], q = cq[nf];
      s += __shfl_xor(s, 16, 64);
      q += __shfl_xor(q, 16, 64);
      s += __shfl_xor(s, 32, 64);
      q += __shfl_xor(q, 32, 64);
      if (fg == 0) {
        int col = wn0 + nf * 16 + fr;
        red[(wr * BN + col) * 2] = s;
        red[(wr * BN + col) * 2 + 1] = q;
      }
    }
    __syncthreads();
    if (tid < BN && n0 + tid < p.Cout) {
      float s = red[tid * 2] + red[(BN + tid) * 2];
      float q = red[tid * 2 + 1] + red[(BN + tid) * 2 + 1];
      const int b = mt / p.tps;
      const int slice = mt - b * p.tps;
      const long o = ((long)slice * p.B + b) * p.Cout + n0 + tid;
      p.psum[o] = s;
      p.psq[o] = q;
    }
  }
}

// ---------------- weight gradient ----------------
// dw[n][k] = Σ_m A[m][k] · dy[m][n];  A-tile and dy-tile staged TRANSPOSED
// (m contiguous per row) so the MFMA reduce dim is m. fp32 atomics over
// split-M slices.

struct WgradParams {
  const short* __restrict__ x;    // [B,H,W,Cin]
  const short* __restrict__ dy;   // [B,OH,OW,Cout]
  float* __restrict__ dw;         // [Cout,KH,KW,Cin] fp32 (pre-zeroed)
  float* __restrict__ ws;         // [slices*ktiles*ntiles][WG_BN][WG_BK] slabs
  int B, H, W, Cin, OH, OW, Cout, KH, KW;
  int stride, pt, pl, reflect;
  long M, KTOT;
  int ktiles, ntiles, slices;
  long mchunks_per_slice;   // in units of 64 rows
};

constexpr int WG_BK = 128;  // k-tile (weight elements; 2x2 waves x 64k each)
constexpr int WG_BN = 64;   // n-tile (cout)
constexpr int WG_BM = 64;   // m per iteration (the mfma reduce dim)
constexpr int WG_LDM = WG_BM + 8;

__global__ __launch_bounds__(NTHREADS) void wgrad_kernel(WgradParams p) {
  __shared__ short At[WG_BK][WG_LDM];   // [k][m]
  __shared__ short Dt[WG_BN][WG_LDM];   // [n][m]
  // per-m gather state, double-buffered, decoded once per m-step
  __shared__ int mih[2][WG_BM], miw[2][WG_BM];
  __shared__ long mxb[2][WG_BM];
  __shared__ char mok[2][WG_BM];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wbid = xcd_chunk(blockIdx.x, gridDim.x);
  const int kt = wbid % p.ktiles;
  const int nt = (wbid / p.ktiles) % p.ntiles;
  const int sl = wbid / (p.ktiles * p.ntiles);
  const long k0 = (long)kt * WG_BK;
  const int n0 = nt * WG_BN;
  const long mstart = sl * p.mchunks_per_slice * WG_BM;
  long mend = mstart + p.mchunks_per_slice * WG_BM;
  if (mend > p.M) mend = p.M;

  v4f acc[4][2] = {};
  const int wr = wid >> 1, wc = wid & 1;
  const int wk0 = wr * 64, wn0 = wc * 32;  // wave tile: 64 k x 32 n
  const int fr = lane & 15, fg = lane >> 4;

  // Staging is transposed: global loads VECTORIZE along the natural inner
  // dims (ci for x, cout for dy) and scatter into the [k][m] / [n][m]
  // images as b64/b32 writes. The vectorized path register-pipelines the
  // next m-step's loads under the current step's MFMAs (T14 split).
  const bool a_vec = (p.Cin % 8) == 0;
  const bool d_vec = (p.Cout % 8) == 0;

  if (a_vec && d_vec && mstart < mend) {
    // fixed per-thread chunk identities (exactly 256 chunks each)
    const int a_mloc = (tid & 15) * 4, a_kc = (tid >> 4) * 8;
    const int d_mloc = (tid & 31) * 2, d_nc = (tid >> 5) * 8;
    const long ak = k0 + a_kc;
    const bool akv = ak < p.KTOT;
    int tap = akv ? (int)(ak / p.Cin) : 0;
    const int ci = (int)(ak - (long)tap * p.Cin);
    const int dkh = tap / p.KW, dkw = tap - (tap / p.KW) * p.KW;
    const bool dnv = n0 + d_nc < p.Cout;

    auto decode = [&](int buf, long ms) {
      for (int r = tid; r < WG_BM; r += NTHREADS) {
        bool ok = ms + r < p.M;
        int mm = ok ? (int)(ms + r) : 0;
        int ow = mm % p.OW;
        int t = mm / p.OW;
        int oh = t % p.OH;
        int b = t / p.OH;
        mok[buf][r] = ok;
        mih[buf][r] = oh * p.stride - p.pt;
        miw[buf][r] = ow * p.stride - p.pl;
        mxb[buf][r] = (long)b * p.H * p.W * p.Cin;
      }
    };

    const v8s VZERO = {};
    v8s areg[4], dreg[2];
    auto load_regs = [&](int buf, long ms) {
      #pragma unroll
      for (int u = 0; u < 4; ++u) {
        areg[u] = VZERO;
        if (akv && mok[buf][a_mloc + u]) {
          int ih = mih[buf][a_mloc + u] + dkh;
          int iw = miw[buf][a_mloc + u] + dkw;
          bool valid = true;
          if (p.reflect) {
            ih = mirror_idx(ih, p.H); iw = mirror_idx(iw, p.W);
          } else {
            valid = ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
          }
          if (valid)
            areg[u] = *(const v8s*)(p.x + mxb[buf][a_mloc + u] +
                                    ((long)ih * p.W + iw) * p.Cin + ci);
        }
      }
      #pragma unroll
      for (int u = 0; u < 2; ++u) {
        dreg[u] = VZERO;
        long m = ms + d_mloc + u;
        if (dnv && m < p.M)
          dreg[u] = *(const v8s*)(p.dy + m * p.Cout + n0 + d_nc);
      }
    };

    decode(0, mstart);
    __syncthreads();
    load_regs(0, mstart);

    int cur = 0;
    for (long ms = mstart; ms < mend; ms += WG_BM, cur ^= 1) {
      // write the registers staged last iteration into the LDS tiles
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        short pa[4] = {areg[0][j], areg[1][j], areg[2][j], areg[3][j]};
        *(uint2*)&At[a_kc + j][a_mloc] = *(uint2*)pa;
        short pd[2] = {dreg[0][j], dreg[1][j]};
        *(unsigned*)&Dt[d_nc + j][d_mloc] = *(unsigned*)pd;
      }
      bool more = ms + WG_BM < mend;
      if (more) decode(cur ^ 1, ms + WG_BM);
      __syncthreads();
      if (more) load_regs(cur ^ 1, ms + WG_BM);  // overlaps the MFMAs below
      #pragma unroll
      for (int kk = 0; kk < WG_BM; kk += 32) {
        v8bf a0 = *(const v8bf*)&At[wk0 + 0 * 16 + fr][kk + fg * 8];
        v8bf a1 = *(const v8bf*)&At[wk0 + 1 * 16 + fr][kk + fg * 8];
        v8bf a2 = *(const v8bf*)&At[wk0 + 2 * 16 + fr][kk + fg * 8];
        v8bf a3 = *(const v8bf*)&At[wk0 + 3 * 16 + fr][kk + fg * 8];
        v8bf b0 = *(const v8bf*)&Dt[wn0 + 0 * 16 + fr][kk + fg * 8];
        v8bf b1 = *(const v8bf*)&Dt[wn0 + 1 * 16 + fr][kk + fg * 8];
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[1][1], 0, 0, 0);
        acc[2][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b0, acc[2][0], 0, 0, 0);
        acc[2][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b1, acc[2][1], 0, 0, 0);
        acc[3][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a3, b0, acc[3][0], 0, 0, 0);
        acc[3][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a3, b1, acc[3][1], 0, 0, 0);
      }
      __syncthreads();
    }

    #pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      int n = n0 + wn0 + nf * 16 + fr;
      if (n >= p.Cout) continue;
      #pragma unroll
      for (int kf = 0; kf < 4; ++kf) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          long k = k0 + wk0 + kf * 16 + fg * 4 + r;
          if (k < p.KTOT)
            atomicAdd(&p.dw[(long)n * p.KTOT + k], acc[kf][nf][r]);
        }
      }
    }
    return;
  }

  for (long ms = mstart; ms < mend; ms += WG_BM) {
    __syncthreads();  // previous iteration's MFMA reads done
    // decode the 64 m-coordinates once (32-bit divisions)
    for (int r = tid; r < WG_BM; r += NTHREADS) {
      int m = (int)(ms + r);
      bool ok = ms + r < p.M;
      int mm = ok ? m : 0;
      int ow = mm % p.OW;
      int t = mm / p.OW;
      int oh = t % p.OH;
      int b = t / p.OH;
      mok[0][r] = ok;
      mih[0][r] = oh * p.stride - p.pt;
      miw[0][r] = ow * p.stride - p.pl;
      mxb[0][r] = (long)b * p.H * p.W * p.Cin;
    }
    __syncthreads();
    {
      for (int c = tid; c < WG_BK * 8; c += NTHREADS) {
        int krow = c >> 3;
        int mc = (c & 7) * 8;
        long k = k0 + krow;
        short vals[8];
        int tap = 0, ci = 0, dkh = 0, dkw = 0;
        bool krows_ok = k < p.KTOT;
        if (krows_ok) {
          tap = (int)(k / p.Cin);
          ci = (int)(k - (long)tap * p.Cin);
          dkh = tap / p.KW; dkw = tap - dkh * p.KW;
        }
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
          long m = ms + mc + j;
          short v = 0;
          if (krows_ok && m < p.M) {
            int ow = (int)(m % p.OW);
            int oh = (int)((m / p.OW) % p.OH);
            int b = (int)(m / ((long)p.OW * p.OH));
            int ih = oh * p.stride - p.pt + dkh;
            int iw = ow * p.stride - p.pl + dkw;
            bool valid = true;
            if (p.reflect) {
              ih = mirror_idx(ih, p.H); iw = mirror_idx(iw, p.W);
            } else {
              valid = ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
            }
            if (valid)
              v = p.x[(((long)b * p.H + ih) * p.W + iw) * p.Cin + ci];
          }
          vals[j] = v;
        }
        *(v8s*)&At[krow][mc] = *(v8s*)vals;
      }
    }
    // ---- stage Dt[n][m]: chunk = (2 m, 8 n); register transpose ----
    if (d_vec) {
      for (int c = tid; c < (WG_BM / 2) * (WG_BN / 8); c += NTHREADS) {
        int m_loc = (c % (WG_BM / 2)) * 2;
        int nc = (c / (WG_BM / 2)) * 8;
        v8s v0 = {}, v1 = {};
        if (n0 + nc < p.Cout) {
          long m = ms + m_loc;
          if (m < p.M) v0 = *(const v8s*)(p.dy + m * p.Cout + n0 + nc);
          if (m + 1 < p.M) v1 = *(const v8s*)(p.dy + (m + 1) * p.Cout + n0 + nc);
        }
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
          short pack[2] = {v0[j], v1[j]};
          *(unsigned*)&Dt[nc + j][m_loc] = *(unsigned*)pack;
        }
      }
    } else {
      for (int c = tid; c < WG_BN * 8; c += NTHREADS) {
        int n = c >> 3;
        int mc = (c & 7) * 8;
        short vals[8];
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
          long m = ms + mc + j;
          vals[j] = (n0 + n < p.Cout && m < p.M)
                        ? p.dy[m * p.Cout + n0 + n] : (short)0;
        }
        *(v8s*)&Dt[n][mc] = *(v8s*)vals;
      }
    }
    __syncthreads();

    #pragma unroll
    for (int kk = 0; kk < WG_BM; kk += 32) {
      v8bf a0 = *(const v8bf*)&At[wk0 + 0 * 16 + fr][kk + fg * 8];
      v8bf a1 = *(const v8bf*)&At[wk0 + 1 * 16 + fr][kk + fg * 8];
      v8bf a2 = *(const v8bf*)&At[wk0 + 2 * 16 + fr][kk + fg * 8];
      v8bf a3 = *(const v8bf*)&At[wk0 + 3 * 16 + fr][kk + fg * 8];
      v8bf b0 = *(const v8bf*)&Dt[wn0 + 0 * 16 + fr][kk + fg * 8];
      v8bf b1 = *(const v8bf*)&Dt[wn0 + 1 * 16 + fr][kk + fg * 8];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[1][1], 0, 0, 0);
      acc[2][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b0, acc[2][0], 0, 0, 0);
      acc[2][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b1, acc[2][1], 0, 0, 0);
      acc[3][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a3, b0, acc[3][0], 0, 0, 0);
      acc[3][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a3, b1, acc[3][1], 0, 0, 0);
    }
    __syncthreads();
  }

  // ---- atomic accumulate: D row = k (= (lane>>4)*4+r), col = n ----
  #pragma unroll
  for (int nf = 0; nf < 2; ++nf) {
    int n = n0 + wn0 + nf * 16 + fr;
    if (n >= p.Cout) continue;
    #pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        long k = k0 + wk0 + kf * 16 + fg * 4 + r;
        if (k < p.KTOT)
          atomicAdd(&p.dw[(long)n * p.KTOT + k], acc[kf][nf][r]);
      }
    }
  }
}

// ---------------- glds + tr_b16 weight gradient ----------------
// Natural [m][k] / [m][n] LDS images staged by LDS-DMA (the same coalesced
// gather as the fwd kernel), consumed TRANSPOSED by ds_read_b64_tr_b16:
// per 16-lane group the 16 8-byte loads form a [4][16] bf16 matrix and
// lane l receives column l&15 (verified by the tr_probe binding), so the
// MFMA reduce dim is m with zero shuffle cost. Double-buffered, XOR
// swizzle rides on the gather lane->element assignment:
//   A image: [64 m][256 B], stored cb = logical_cb ^ ((m&7)<<5)
//   D image: [64 m][128 B], stored cb = logical_cb ^ ((m&3)<<5)

typedef bf16r v4bfx __attribute__((ext_vector_type(4)));

// XOR swizzles for the wgrad images. Row bit 3 feeds cb bit 4 so the two
// 16-lane tr groups of a 32-lane bank half land on different 16-B slots.
#define AXOR(row) ((((row) & 7) << 5) | ((((row) >> 3) & 1) << 4))
#define DXOR(row) ((((row) & 3) << 5) | ((((row) >> 3) & 1) << 4))

DEV v4bfx tr16_read(const char* plds) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) v4bfx*)plds);
}

template <int WBN, int KT = 1>
struct WgSmemT {
  short A[2][KT * WG_BM * WG_BK];   // [ktile][m][k] swizzled
  short D[2][WG_BM * WBN];          // [m][n] swizzled
};

// KT = k-tiles per block (2 for the wide resblock shapes): D staging and
// all per-iteration overhead (advance, loop control, barriers) amortize
// over KT x the MFMA work; A gather state is per (ktile, instr) slot.
template <int NW = 4, int WBN = 64, int KT = 1>
__global__ __launch_bounds__(NW * 64) void wgrad_glds_kernel(WgradParams p) {
  constexpr int API = 16 / NW;        // A glds instructions per wave
  constexpr int AT = KT * API;        // gather slots per wave
  constexpr int DCH = WBN / 8;        // 16-B chunks per D row
  constexpr int DRPI = 64 / DCH;      // D rows per glds instruction
  constexpr int TDI = (WG_BM * DCH) / 64;   // D glds instructions total
  constexpr int DPI = TDI >= NW ? TDI / NW : 1;  // per wave (maybe idle)
  // n-fragments per wave: the 4-wave/128-n config packs 4x4 fragments
  // per wave (32 MFMAs per tr-read set) halving LDS re-read redundancy
  constexpr int NFW = (NW == 4 && WBN == 128) ? 4 : (WBN >= 32 ? 2 : 1);
  constexpr int NWCW = WBN / (NFW * 16);    // wave-grid columns
  constexpr int KF = (WG_BK / (NW / NWCW)) / 16;  // k-fragments per wave
  extern __shared__ __attribute__((aligned(16))) char wg_smem_raw[];
  auto& sm = *reinterpret_cast<WgSmemT<WBN, KT>*>(wg_smem_raw);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int wbid = xcd_chunk(blockIdx.x, gridDim.x);
  const int pairs = p.ktiles / KT;    // host guarantees p.ktiles % KT == 0
  const int ktp = wbid % pairs;
  const int kt = ktp * KT;            // first k-tile of this block
  const int nt = (wbid / pairs) % p.ntiles;
  const int sl = wbid / (pairs * p.ntiles);
  const long k0 = (long)kt * WG_BK;
  const int n0 = nt * WBN;
  const long mstart = sl * p.mchunks_per_slice * WG_BM;
  long mend = mstart + p.mchunks_per_slice * WG_BM;
  if (mend > p.M) mend = p.M;
  if (mstart >= mend) {
    // idle slice (host over-split): MUST still zero its output slab —
    // wgrad_reduce sums every chunk, and at::empty memory is dirty
    // (this was a real bug: reused allocator pages leaked garbage into
    // dw at shapes where slices * mchunks_per_slice overshot M)
    for (int t = 0; t < KT; ++t) {
      long chunk = (((long)sl * p.ktiles + kt + t) * p.ntiles + nt) *
                   ((long)WBN * WG_BK);
      for (int i = tid; i < WBN * WG_BK; i += NW * 64) p.ws[chunk + i] = 0.f;
    }
    return;
  }

  auto rx = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.x, 0, (unsigned)((long)p.B * p.H * p.W * p.Cin * 2), 0x00020000);
  auto rd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.dy, 0, (unsigned)(p.M * p.Cout * 2), 0x00020000);

  // ---- per-lane gather identities ----
  // A: 16 instrs: instr i covers rows i*4..i*4+3; per-wave share = API
  int a_row[AT], a_ci[AT], a_dkh[AT], a_dkw[AT];
  bool a_kv[AT];
  #pragma unroll
  for (int t = 0; t < KT; ++t) {
    #pragma unroll
    for (int j = 0; j < API; ++j) {
      int sidx = t * API + j;
      int row = (w * API + j) * 4 + (lane >> 4);
      int cb = ((lane & 15) * 16) ^ AXOR(row);
      long k = k0 + (long)t * WG_BK + cb / 2;
      a_row[sidx] = row;
      a_kv[sidx] = k < p.KTOT;
      int tap = a_kv[sidx] ? (int)(k / p.Cin) : 0;
      a_ci[sidx] = (int)(k - (long)tap * p.Cin);
      a_dkh[sidx] = tap / p.KW;
      a_dkw[sidx] = tap - a_dkh[sidx] * p.KW;
    }
  }
  // D: instr i covers DRPI rows; per-wave share = DPI
  const bool dw_on = w * DPI < TDI;  // waves beyond TDI stage no D
  int d_row[DPI], d_n[DPI];
  #pragma unroll
  for (int j = 0; j < DPI; ++j) {
    int row = (w * DPI + j) * DRPI + lane / DCH;
    int cb = ((lane % DCH) * 16) ^
             (WBN == 128 ? AXOR(row) : WBN == 64 ? DXOR(row) : 0);
    d_row[j] = row;
    d_n[j] = n0 + cb / 2;
  }

  // incremental m-decode AND incremental voffsets: interior steps cost two
  // small multiplies per instruction; full address recomputation happens
  // only at image borders / batch wraps (O(1/OH) of steps).
  const unsigned C2 = (unsigned)p.Cin * 2;
  const unsigned WC2 = (unsigned)p.W * C2;
  int a_ow[AT], a_oh[AT], a_b[AT], a_ih[AT], a_iw[AT];
  unsigned avo[AT];
  bool ainb[AT], avalid[AT], a_iw_ok[AT];
  unsigned dvo[DPI];

  auto full_a = [&](int j) {
    int ih = a_ih[j], iw = a_iw[j];
    bool valid = a_kv[j];   // k-tail folds in permanently
    if (p.reflect) {
      ih = mirror_idx(ih, p.H); iw = mirror_idx(iw, p.W);
    } else {
      valid = valid && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
    }
    avalid[j] = valid;
    avo[j] = valid ? (unsigned)(((((long)a_b[j] * p.H + ih) * p.W + iw) *
                                 p.Cin + a_ci[j]) * 2)
                   : 0xFF000000u;
  };

  #pragma unroll
  for (int j = 0; j < AT; ++j) {
    long m = mstart + a_row[j];
    a_ow[j] = (int)(m % p.OW);
    int t = (int)(m / p.OW);
    a_oh[j] = t % p.OH;
    a_b[j] = t / p.OH;
    a_ih[j] = a_oh[j] * p.stride - p.pt + a_dkh[j];
    a_iw[j] = a_ow[j] * p.stride - p.pl + a_dkw[j];
    a_iw_ok[j] = (unsigned)a_iw[j] < (unsigned)p.W;
    ainb[j] = (unsigned)a_ih[j] < (unsigned)p.H && a_iw_ok[j];
    full_a(j);
  }
  #pragma unroll
  for (int j = 0; j < DPI; ++j)
    // n-overflow folds permanently: 0xFF000000 plus all increments stays
    // far above num_records (tensor < 100 MB), so the load returns 0
    dvo[j] = d_n[j] < p.Cout
                 ? (unsigned)(((mstart + d_row[j]) * p.Cout + d_n[j]) * 2)
                 : 0xFF000000u;

  const bool ow_fast = (p.OW == WG_BM);  // K3/down shapes: ow invariant
  const unsigned sWC2 = (unsigned)(p.stride * (int)WC2);
  auto advance = [&]() {
    if (ow_fast) {
      // ow (and iw) never change: interior step = oh+1, ih+stride, ONE
      // voffset add. Batch wraps / ih border transitions take the rare
      // exec-masked path (1/OH of steps) — this was the 20-mult-per-iter
      // hot spot the compiler was predicating on every iteration.
      #pragma unroll
      for (int j = 0; j < AT; ++j) {
        bool rare = (++a_oh[j] >= p.OH);
        if (!rare) {
          int ih = a_ih[j] + p.stride;
          a_ih[j] = ih;
          bool inb = (unsigned)ih < (unsigned)p.H;
          if (inb && ainb[j] && avalid[j]) {
            avo[j] += sWC2;
          } else {
            rare = true;
          }
          ainb[j] = inb && a_iw_ok[j];
        }
        if (rare) {
          while (a_oh[j] >= p.OH) { a_oh[j] -= p.OH; ++a_b[j]; }
          a_ih[j] = a_oh[j] * p.stride - p.pt + a_dkh[j];
          full_a(j);
          ainb[j] = ((unsigned)a_ih[j] < (unsigned)p.H) && a_iw_ok[j];
        }
      }
    } else {
      #pragma unroll
      for (int j = 0; j < AT; ++j) {
        int ow0 = a_ow[j], oh0 = a_oh[j], b0 = a_b[j];
        a_ow[j] += WG_BM;
        while (a_ow[j] >= p.OW) { a_ow[j] -= p.OW; ++a_oh[j]; }
        while (a_oh[j] >= p.OH) { a_oh[j] -= p.OH; ++a_b[j]; }
        int dih = (a_oh[j] - oh0) * p.stride;
        int diw = (a_ow[j] - ow0) * p.stride;
        a_ih[j] += dih;
        a_iw[j] += diw;
        bool inb = (unsigned)a_ih[j] < (unsigned)p.H &&
                   (unsigned)a_iw[j] < (unsigned)p.W;
        if (a_b[j] == b0 && inb && ainb[j] && avalid[j]) {
          avo[j] += (unsigned)(dih * (int)WC2 + diw * (int)C2);
        } else {
          full_a(j);
        }
        ainb[j] = inb;
      }
    }
    #pragma unroll
    for (int j = 0; j < DPI; ++j) dvo[j] += (unsigned)(WG_BM * p.Cout * 2);
  };

  // m-tail guard is UNIFORM (a_row < WG_BM): only the last chunk of a
  // slice that crosses p.M needs per-row selects; the steady state stages
  // straight from the folded avo/dvo registers.
  auto stage = [&](int buf, long ms, bool tail) {
    #pragma unroll
    for (int t = 0; t < KT; ++t) {
      #pragma unroll
      for (int j = 0; j < API; ++j) {
        int sidx = t * API + j;
        unsigned vo = (!tail || ms + a_row[sidx] < p.M) ? avo[sidx]
                                                        : 0xFF000000u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rx, (__attribute__((address_space(3))) void*)
                &sm.A[buf][t * (WG_BM * WG_BK) + (w * API + j) * 512],
            16, vo, 0, 0, 0);
      }
    }
    if (dw_on) {
      #pragma unroll
      for (int j = 0; j < DPI; ++j) {
        unsigned vo = (!tail || ms + d_row[j] < p.M) ? dvo[j] : 0xFF000000u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rd, (__attribute__((address_space(3))) void*)&sm.D[buf][(w * DPI + j) * 512],
            16, vo, 0, 0, 0);
      }
    }
  };

  v4f acc[KT][KF][NFW] = {};
  const int wr = w / NWCW, wc = w % NWCW;
  const int wk0 = wr * (KF * 16), wn0 = wc * (NFW * 16);
  const int fr = lane & 15, fg = lane >> 4;
  const int jg = lane & 15;
  // tr-read per-lane address components (bytes)
  const int tr_row_a = jg >> 2;            // row-in-4 within the tr tile
  const int tr_cb_a = (jg & 3) * 8;        // 4-elem column sub-offset

  // tr-read addresses are kk-invariant up to +kk*rowpitch: kk in {0,32}
  // only touches address bits >= 5 of the row, so AXOR/DXOR (bits derived
  // from row&7 and (row>>3)&1, with fg*8 keeping row&7 = tr_row_a and
  // kk>>3 even) never change across the m-loop. Hoist the full per-lane
  // byte offsets once; the inner loop is pure adds (was the 7.6 VALU/MFMA
  // hot spot, profiles/pmc_bench286.md row 1).
  int a_base[KF][2], d_base[NFW][2];
  #pragma unroll
  for (int kf = 0; kf < KF; ++kf) {
    #pragma unroll
    for (int h = 0; h < 2; ++h) {
      int row = fg * 8 + tr_row_a + 4 * h;
      int cbl = (wk0 + kf * 16) * 2 + tr_cb_a;
      a_base[kf][h] = row * 256 + (cbl ^ AXOR(row));
    }
  }
  #pragma unroll
  for (int nf = 0; nf < NFW; ++nf) {
    #pragma unroll
    for (int h = 0; h < 2; ++h) {
      int row = fg * 8 + tr_row_a + 4 * h;
      int cbl = (wn0 + nf * 16) * 2 + tr_cb_a;
      d_base[nf][h] = row * (WBN * 2) +
          (cbl ^ (WBN == 128 ? AXOR(row) : WBN == 64 ? DXOR(row) : 0));
    }
  }

  stage(0, mstart, mstart + WG_BM > p.M);
  __syncthreads();

  int cur = 0;
  for (long ms = mstart; ms < mend; ms += WG_BM, cur ^= 1) {
    if (ms + WG_BM < mend) {
      advance();
      stage(cur ^ 1, ms + WG_BM, ms + 2 * WG_BM > p.M);
    }
    const char* Ab = (const char*)sm.A[cur];
    const char* Db = (const char*)sm.D[cur];
    #pragma unroll
    for (int kk = 0; kk < WG_BM; kk += 32) {
      v8bf bfr[NFW];
      #pragma unroll
      for (int nf = 0; nf < NFW; ++nf) {
        v4bfx lo = tr16_read(Db + kk * (WBN * 2) + d_base[nf][0]);
        v4bfx hi = tr16_read(Db + kk * (WBN * 2) + d_base[nf][1]);
        bfr[nf] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
      // A fragments: MFMA row = weight-k col0+fr, reduce elems = m
      #pragma unroll
      for (int t = 0; t < KT; ++t) {
        const char* At = Ab + t * (WG_BM * WG_BK * 2);
        v8bf a[KF];
        #pragma unroll
        for (int kf = 0; kf < KF; ++kf) {
          v4bfx lo = tr16_read(At + kk * 256 + a_base[kf][0]);
          v4bfx hi = tr16_read(At + kk * 256 + a_base[kf][1]);
          a[kf] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        }
        #pragma unroll
        for (int kf = 0; kf < KF; ++kf)
          #pragma unroll
          for (int nf = 0; nf < NFW; ++nf)
            acc[t][kf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a[kf], bfr[nf], acc[t][kf][nf], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // slab store (no atomics): chunk layout [WBN][WG_BK], float4 rows
  #pragma unroll
  for (int t = 0; t < KT; ++t) {
    long chunk = (((long)sl * p.ktiles + kt + t) * p.ntiles + nt) *
                 ((long)WBN * WG_BK);
    #pragma unroll
    for (int nf = 0; nf < NFW; ++nf) {
      int nl = wn0 + nf * 16 + fr;
      if (nl >= WBN) continue;
      #pragma unroll
      for (int kf = 0; kf < KF; ++kf) {
        int kl = wk0 + kf * 16 + fg * 4;
        *(float4*)&p.ws[chunk + (long)nl * WG_BK + kl] =
            *(const float4*)&acc[t][kf][nf];
      }
    }
  }
}

// sum the split-M slabs into dw (coalesced; also applies the K/N guards)
__global__ void wgrad_reduce_kernel(const float* __restrict__ ws,
                                    float* __restrict__ dw, long KTOT,
                                    int Cout, int ktiles, int ntiles,
                                    int slices, int wbn) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)ktiles * WG_BK * ntiles * wbn;
  if (idx >= total) return;
  // idx -> (nt, nl, kt, kl) with kl fastest for coalescing
  int kl = (int)(idx % WG_BK);
  long t = idx / WG_BK;
  int kt = (int)(t % ktiles);
  t /= ktiles;
  int nl = (int)(t % wbn);
  int nt = (int)(t / wbn);
  long k = (long)kt * WG_BK + kl;
  int n = nt * wbn + nl;
  if (k >= KTOT || n >= Cout) return;
  long stride = (long)ktiles * ntiles * wbn * WG_BK;
  long off = (((long)kt * ntiles + nt) * wbn + nl) * WG_BK + kl;
  // 4 independent accumulation chains: with ~14 slices per element the
  // single-chain loop was latency-bound at 4x the memory floor
  float s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  int sl = 0;
  for (; sl + 4 <= slices; sl += 4) {
    s0 += ws[off + (sl + 0) * stride];
    s1 += ws[off + (sl + 1) * stride];
    s2 += ws[off + (sl + 2) * stride];
    s3 += ws[off + (sl + 3) * stride];
  }
  for (; sl < slices; ++sl) s0 += ws[off + sl * stride];
  dw[(long)n * KTOT + k] = (s0 + s1) + (s2 + s3);
}

// ---------------- reflect fold (dgrad border scatter) ----------------
// dx[b,i,j,c] = Σ over padded positions q with mirror(q - pad) == (i,j)
// vectorized: one thread folds 8 channels of one (b,i,j); the candidate
// logic is per-pixel, shared by all 8 lanes' channels.
__global__ void reflect_fold_kernel(const short* __restrict__ dxp,
                                    short* __restrict__ dx,
                                    int B, int H, int W, int C,
                                    int pt, int pb, int pl, int pr) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int gpr = C / 8;
  long total = (long)B * H * W * gpr;
  if (idx >= total) return;
  int g = (int)(idx % gpr);
  long t = idx / gpr;
  int j = (int)(t % W);
  t /= W;
  int i = (int)(t % H);
  int b = (int)(t / H);
  int HP = H + pt + pb, WP = W + pl + pr;
  float s[8] = {};
  int hc[3] = {pt + i, pt - i, pt + 2 * (H - 1) - i};
  int wc_[3] = {pl + j, pl - j, pl + 2 * (W - 1) - j};
  #pragma unroll
  for (int a = 0; a < 3; ++a) {
    int qh = hc[a];
    if (qh < 0 || qh >= HP) continue;
    if (a > 0 && qh == hc[0]) continue;           // dedupe (i==0 cases)
    if (a == 2 && qh == hc[1]) continue;
    if (mirror_idx(qh - pt, H) != i) continue;
    #pragma unroll
    for (int d = 0; d < 3; ++d) {
      int qw = wc_[d];
      if (qw < 0 || qw >= WP) continue;
      if (d > 0 && qw == wc_[0]) continue;
      if (d == 2 && qw == wc_[1]) continue;
      if (mirror_idx(qw - pl, W) != j) continue;
      v8s v = *(const v8s*)(dxp + (((long)b * HP + qh) * WP + qw) * C + g * 8);
      #pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += b2f(v[e]);
    }
  }
  v8s out;
  #pragma unroll
  for (int e = 0; e < 8; ++e) out[e] = f2b(s[e]);
  *(v8s*)(dx + (((long)b * H + i) * W + j) * C + g * 8) = out;
}

// ================= host wrappers =================

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

template <bool IS_CONVT, bool ALIGNED>
static void launch_conv_s(const ConvParams& p, dim3 grid, hipStream_t stream) {
  switch (p.stride) {
    case 1:
      hipLaunchKernelGGL((conv_gemm_kernel<IS_CONVT, ALIGNED, 1>), grid,
                         dim3(NTHREADS), 0, stream, p);
      break;
    case 2:
      hipLaunchKernelGGL((conv_gemm_kernel<IS_CONVT, ALIGNED, 2>), grid,
                         dim3(NTHREADS), 0, stream, p);
      break;
    default:
      hipLaunchKernelGGL((conv_gemm_kernel<IS_CONVT, ALIGNED, 0>), grid,
                         dim3(NTHREADS), 0, stream, p);
  }
}

static int conv_nw() {
  static int v = []() {
    const char* e = getenv("CYG_CONV_NW");
    return e ? atoi(e) : 8;
  }();
  return v;
}

static int conv_bn() {
  static int v = []() {
    const char* e = getenv("CYG_CONV_BN");
    return e ? atoi(e) : 128;
  }();
  return v;
}

template <bool IS_CONVT, int STRIDE, int NBUF, int NW, int BNT,
          bool PHASED = false>
static void launch_one_glds(const ConvParams& p, dim3 grid,
                            hipStream_t stream) {
  constexpr size_t SMB = sizeof(ConvSmemT<NBUF, BNT>);
  static bool init = []() {
    hipFuncSetAttribute(
        (const void*)(conv_glds_kernel<IS_CONVT, STRIDE, NBUF, NW, BNT,
                                       PHASED>),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMB);
    return true;
  }();
  (void)init;
  hipLaunchKernelGGL(
      (conv_glds_kernel<IS_CONVT, STRIDE, NBUF, NW, BNT, PHASED>), grid,
      dim3(NW * 64), SMB, stream, p);
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "conv_glds launch failed (NW=", NW,
              " BNT=", BNT, " PHASED=", PHASED, "): ",
              hipGetErrorString(err));
}

template <bool IS_CONVT>
static void launch_glds_s(const ConvParams& p, dim3 grid, hipStream_t stream) {
  if constexpr (!IS_CONVT) {
    // Halo-tiled head kernel: correct but still 137us vs the BN16
    // implicit-GEMM's 122us on the 7x7 head (see NOTES.md for the
    // measured iteration trail); off by default pending round-2 work.
    static const bool use_halo = []() {
      const char* e = getenv("CYG_HALO");
      return e && atoi(e) != 0;
    }();
    if (use_halo && p.Cout == 8 && p.stride == 1 && p.Cin == 64) {
      // halo-tiled direct kernel for the tiny-Cout heads (see kernel doc)
      const int CW = HB_BM + p.KW - 1;
      const int xgr = p.KH * CW * 9;       // 9 slots/pixel (bank spread)
      const int xgr_pad = ((xgr + 511) / 512) * 512;
      const size_t smb = (size_t)xgr_pad * 16;
      if (smb <= 150 * 1024) {
        static bool init = []() {
          hipFuncSetAttribute((const void*)(conv_halo_kernel<8>),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              150 * 1024);
          return true;
        }();
        (void)init;
        const int tiles_w = (p.OW + HB_BM - 1) / HB_BM;
        dim3 gh((long)p.B * p.OH * tiles_w);
        hipLaunchKernelGGL((conv_halo_kernel<8>), gh, dim3(512), smb,
                           stream, p);
        hipError_t err = hipGetLastError();
        TORCH_CHECK(err == hipSuccess, "conv_halo launch failed: ",
                    hipGetErrorString(err));
        return;
      }
    }
  }
  if (p.Cout <= 16) {
    // tiny-N (the 1-8 channel heads, padded to 8): 16-wide n-tiles
    ConvParams q = p;
    q.ntiles = (p.Cout + 15) / 16;
    dim3 g2((long)q.mtiles * q.ntiles);
    switch (p.stride) {
      case 1: launch_one_glds<IS_CONVT, 1, 2, 8, 16>(q, g2, stream); return;
      case 2: launch_one_glds<IS_CONVT, 2, 2, 8, 16>(q, g2, stream); return;
      default: launch_one_glds<IS_CONVT, 0, 2, 8, 16>(q, g2, stream); return;
    }
  }
  if (conv_nw() == 8 && conv_bn() == 128 && (p.Cout % 128) == 0) {
    // wider n-tile: 1.5x arithmetic intensity for Cout >= 128 layers
    ConvParams q = p;
    q.ntiles = (p.Cout + 127) / 128;
    dim3 g2((long)q.mtiles * q.ntiles);
    switch (p.stride) {
      case 1: launch_one_glds<IS_CONVT, 1, 2, 8, 128>(q, g2, stream); return;
      case 2: launch_one_glds<IS_CONVT, 2, 2, 8, 128>(q, g2, stream); return;
      default: launch_one_glds<IS_CONVT, 0, 2, 8, 128>(q, g2, stream); return;
    }
  }
  if (conv_nw() == 8) {
    switch (p.stride) {
      case 1: launch_one_glds<IS_CONVT, 1, 2, 8, 64>(p, grid, stream); return;
      case 2: launch_one_glds<IS_CONVT, 2, 2, 8, 64>(p, grid, stream); return;
      default: launch_one_glds<IS_CONVT, 0, 2, 8, 64>(p, grid, stream); return;
    }
  }
  switch (p.stride) {
    case 1: launch_one_glds<IS_CONVT, 1, 2, 4, 64>(p, grid, stream); break;
    case 2: launch_one_glds<IS_CONVT, 2, 2, 4, 64>(p, grid, stream); break;
    default: launch_one_glds<IS_CONVT, 0, 2, 4, 64>(p, grid, stream);
  }
}

// glds path needs 8-aligned channels and 32-bit byte offsets into x and w
static bool glds_eligible(const ConvParams& p) {
  return (p.Cin % 8) == 0 &&
         (long)p.B * p.H * p.W * p.Cin * 2 < (1L << 31) &&
         (long)p.Cout * p.KTOT * 2 < (1L << 31);
}

static bool phased_eligible(const ConvParams& p, bool is_convt) {
  return glds_eligible(p) && is_convt && p.stride == 2 && (p.OH % 2) == 0 &&
         (p.OW % 2) == 0;
}

// InstanceNorm slabs from the conv epilogue: number of slabs per sample
// this call can emit (0 = not eligible; the norm then runs in_reduce).
// Eligible = conv_glds_kernel runs it with 64/128-wide n-tiles and every
// 128-row M-tile lies inside one sample: OH*OW % 128 == 0 for the plain
// row order; for the phased convT the rows of one parity class of one
// sample are contiguous, so (OH/2)*(OW/2) % 128 == 0 (4 classes per
// sample). The slab count is capped because every in_norm block re-sums
// all slabs of its sample in its prologue: HW/128 slabs is a win up to
// 128^2 (<= today's slice count) and a loss at 256^2 (512 slabs vs 128).
// CYG_NO_CONV_STATS=1 turns the path off; CYG_CONV_STATS_MAXSLABS moves
// the cap for A/B runs.
static int stats_cap() {
  static const int cap = []() {
    const char* off = getenv("CYG_NO_CONV_STATS");
    if (off && off[0] == '1') return 0;
    const char* e = getenv("CYG_CONV_STATS_MAXSLABS");
    return e ? atoi(e) : 128;
  }();
  return cap;
}

static int stats_slabs(const ConvParams& p, bool is_convt, int* tps) {
  const int cap = stats_cap();
  if (cap <= 0 || !glds_eligible(p) || p.Cout <= 16 || (p.Cout % 8) != 0)
    return 0;
  long per, ns;
  if (phased_eligible(p, is_convt)) {
    per = (long)(p.OH / 2) * (p.OW / 2);
    ns = 4 * (per / BM);
  } else {
    per = (long)p.OH * p.OW;
    ns = per / BM;
  }
  if (per % BM != 0 || ns > cap) return 0;
  *tps = (int)(per / BM);
  return (int)ns;
}

static void launch_conv(const ConvParams& p, bool is_convt, hipStream_t stream) {
  dim3 grid(p.mtiles * p.ntiles);
  bool aligned = (p.Cin % 8) == 0;
  bool glds_ok = glds_eligible(p);
  if (phased_eligible(p, is_convt)) {
    // phase-decomposed: 4 phase classes, only matching-parity taps
    ConvParams q = p;
    long Mp = (long)q.B * (q.OH / 2) * (q.OW / 2);
    q.mtiles = 4 * cdiv(Mp, BM);
    if (conv_nw() == 8 && conv_bn() == 128 && (q.Cout % 128) == 0) {
      q.ntiles = (q.Cout + 127) / 128;
      dim3 g2((long)q.mtiles * q.ntiles);
      launch_one_glds<true, 2, 2, 8, 128, true>(q, g2, stream);
    } else if (conv_nw() == 8) {
      dim3 g2((long)q.mtiles * q.ntiles);
      launch_one_glds<true, 2, 2, 8, 64, true>(q, g2, stream);
    } else {
      dim3 g2((long)q.mtiles * q.ntiles);
      launch_one_glds<true, 2, 2, 4, 64, true>(q, g2, stream);
    }
    return;
  }
  if (glds_ok) {
    if (is_convt) launch_glds_s<true>(p, grid, stream);
    else launch_glds_s<false>(p, grid, stream);
    return;
  }
  if (is_convt) {
    if (aligned) launch_conv_s<true, true>(p, grid, stream);
    else launch_conv_s<true, false>(p, grid, stream);
  } else {
    if (aligned) launch_conv_s<false, true>(p, grid, stream);
    else launch_conv_s<false, false>(p, grid, stream);
  }
}

static ConvParams fill_common(const at::Tensor& x, const at::Tensor& w,
                              const c10::optional<at::Tensor>& bias,
                              at::Tensor& y, int stride, int act, double slope) {
  ConvParams p{};
  p.x = (const short*)x.const_data_ptr();
  p.w = (const short*)w.const_data_ptr();
  p.bias = bias.has_value() ? (const short*)bias->const_data_ptr() : nullptr;
  p.y = (short*)y.mutable_data_ptr();
  p.B = x.size(0); p.H = x.size(1); p.W = x.size(2); p.Cin = x.size(3);
  p.OH = y.size(1); p.OW = y.size(2); p.Cout = y.size(3);
  p.KH = w.size(1); p.KW = w.size(2);
  p.stride = stride;
  p.act = act; p.slope = (float)slope;
  p.M = (long)p.B * p.OH * p.OW;
  p.KTOT = (long)p.KH * p.KW * p.Cin;
  p.mtiles = cdiv(p.M, BM);
  p.ntiles = cdiv(p.Cout, BN);
  return p;
}

static void check_conv_inputs(const at::Tensor& x, const at::Tensor& w) {
  TORCH_CHECK(x.is_cuda() && w.is_cuda(), "conv: tensors must be on GPU");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16,
              "conv: GPU path is bf16 (got ", x.scalar_type(), ")");
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous(), "conv: need contiguous");
  TORCH_CHECK(w.size(3) == x.size(3), "conv: Cin mismatch");
}

// want_stats: also return the InstanceNorm partial slabs {y, psum, psq}
// ([NS,B,Cout] fp32) when the call is eligible (stats_slabs); {y} otherwise.
static std::vector<at::Tensor> run_fwd(ConvParams& p, at::Tensor& y,
                                       bool is_convt, bool want_stats) {
  std::vector<at::Tensor> out{y};
  int tps = 0;
  int ns = want_stats ? stats_slabs(p, is_convt, &tps) : 0;
  if (ns > 0) {
    auto ps = at::empty({2, ns, (long)p.B, (long)p.Cout},
                        y.options().dtype(at::kFloat));
    p.psum = (float*)ps.mutable_data_ptr();
    p.psq = p.psum + (long)ns * p.B * p.Cout;
    p.tps = tps;
    out.push_back(ps[0]);
    out.push_back(ps[1]);
  }
  launch_conv(p, is_convt, at::cuda::getCurrentCUDAStream());
  return out;
}

static std::vector<at::Tensor> conv2d_fwd_impl(
    at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias,
    int64_t stride, int64_t pt, int64_t pb, int64_t pl, int64_t pr,
    bool reflect, int64_t act, double slope, bool want_stats) {
  check_conv_inputs(x, w);
  int H = x.size(1), W = x.size(2);
  int KH = w.size(1), KW = w.size(2);
  int OH = (H + pt + pb - KH) / stride + 1;
  int OW = (W + pl + pr - KW) / stride + 1;
  auto y = at::empty({x.size(0), OH, OW, w.size(0)}, x.options());
  auto p = fill_common(x, w, bias, y, stride, act, slope);
  p.pt = pt; p.pl = pl; p.reflect = reflect ? 1 : 0;
  return run_fwd(p, y, false, want_stats);
}

static std::vector<at::Tensor> convt2d_fwd_impl(
    at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias,
    int64_t stride, int64_t pt, int64_t pl, int64_t out_h, int64_t out_w,
    int64_t act, double slope, bool want_stats) {
  check_conv_inputs(x, w);
  auto y = at::empty({x.size(0), out_h, out_w, w.size(0)}, x.options());
  auto p = fill_common(x, w, bias, y, stride, act, slope);
  p.pt = pt; p.pl = pl; p.reflect = 0;
  return run_fwd(p, y, true, want_stats);
}

at::Tensor conv2d_fwd(at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias,
                      int64_t stride, int64_t pt, int64_t pb, int64_t pl,
                      int64_t pr, bool reflect, int64_t act, double slope) {
  return conv2d_fwd_impl(x, w, bias, stride, pt, pb, pl, pr, reflect, act,
                         slope, false)[0];
}

std::vector<at::Tensor> conv2d_fwd_stats(
    at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias,
    int64_t stride, int64_t pt, int64_t pb, int64_t pl, int64_t pr,
    bool reflect, int64_t act, double slope) {
  return conv2d_fwd_impl(x, w, bias, stride, pt, pb, pl, pr, reflect, act,
                         slope, true);
}

at::Tensor convt2d_fwd(at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias,
                       int64_t stride, int64_t pt, int64_t pl,
                       int64_t out_h, int64_t out_w, int64_t act, double slope) {
  return convt2d_fwd_impl(x, w, bias, stride, pt, pl, out_h, out_w, act,
                          slope, false)[0];
}

std::vector<at::Tensor> convt2d_fwd_stats(
    at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias,
    int64_t stride, int64_t pt, int64_t pl, int64_t out_h, int64_t out_w,
    int64_t act, double slope) {
  return convt2d_fwd_impl(x, w, bias, stride, pt, pl, out_h, out_w, act,
                          slope, true);
}

// conv dgrad: dx = gather-adjoint of conv_fwd == convt kernel on dy with the
// channel-transposed weight (wt: [Cin,KH,KW,Cout]), same taps, no flip.
at::Tensor conv2d_dgrad(at::Tensor dy, at::Tensor wt, int64_t H, int64_t W,
                        int64_t stride, int64_t pt, int64_t pb, int64_t pl,
                        int64_t pr, bool reflect) {
  check_conv_inputs(dy, wt);
  auto stream = at::cuda::getCurrentCUDAStream();
  if (!reflect) {
    auto dx = at::empty({dy.size(0), H, W, wt.size(0)}, dy.options());
    auto p = fill_common(dy, wt, c10::nullopt, dx, stride, ACT_NONE, 0.0);
    p.pt = pt; p.pl = pl;
    launch_conv(p, true, stream);
    return dx;
  }
  // reflect: dgrad into the padded frame, then fold mirrors back
  long HP = H + pt + pb, WP = W + pl + pr;
  auto dxp = at::empty({dy.size(0), HP, WP, wt.size(0)}, dy.options());
  auto p = fill_common(dy, wt, c10::nullopt, dxp, stride, ACT_NONE, 0.0);
  p.pt = 0; p.pl = 0;
  launch_conv(p, true, stream);
  auto dx = at::empty({dy.size(0), H, W, wt.size(0)}, dy.options());
  TORCH_CHECK(wt.size(0) % 8 == 0, "reflect dgrad: Cin % 8 != 0");
  long total = dx.numel() / 8;
  int threads = 256;
  hipLaunchKernelGGL(reflect_fold_kernel, dim3(cdiv(total, threads)),
                     dim3(threads), 0, stream,
                     (const short*)dxp.const_data_ptr(),
                     (short*)dx.mutable_data_ptr(),
                     (int)dy.size(0), (int)H, (int)W, (int)wt.size(0),
                     (int)pt, (int)pb, (int)pl, (int)pr);
  return dx;
}

// convt dgrad: adjoint of the convt gather == strided conv_fwd of dy.
at::Tensor convt2d_dgrad(at::Tensor dy, at::Tensor wt, int64_t IH, int64_t IW,
                         int64_t stride, int64_t pt, int64_t pl) {
  check_conv_inputs(dy, wt);
  int KH = wt.size(1), KW = wt.size(2);
  auto dx = at::empty({dy.size(0), IH, IW, wt.size(0)}, dy.options());
  auto p = fill_common(dy, wt, c10::nullopt, dx, stride, ACT_NONE, 0.0);
  p.pt = pt; p.pl = pl; p.reflect = 0;
  launch_conv(p, false, at::cuda::getCurrentCUDAStream());
  return dx;
}

at::Tensor conv2d_wgrad(at::Tensor x, at::Tensor dy, int64_t KH, int64_t KW,
                        int64_t stride, int64_t pt, int64_t pl, bool reflect) {
  TORCH_CHECK(x.is_cuda() && dy.is_cuda() && x.is_contiguous() && dy.is_contiguous());
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && dy.scalar_type() == at::kBFloat16);
  TORCH_CHECK(dy.size(0) == x.size(0));
  WgradParams p{};
  p.x = (const short*)x.const_data_ptr();
  p.dy = (const short*)dy.const_data_ptr();
  p.B = x.size(0); p.H = x.size(1); p.W = x.size(2); p.Cin = x.size(3);
  p.OH = dy.size(1); p.OW = dy.size(2); p.Cout = dy.size(3);
  p.KH = KH; p.KW = KW; p.stride = stride; p.pt = pt; p.pl = pl;
  p.reflect = reflect ? 1 : 0;
  p.M = (long)p.B * p.OH * p.OW;
  p.KTOT = (long)KH * KW * p.Cin;
  p.ktiles = cdiv(p.KTOT, WG_BK);
  p.ntiles = cdiv(p.Cout, WG_BN);
  // split M so total blocks ≈ 2-4x CU count (CYG_WG_BLOCKS to sweep)
  long mchunks = (p.M + WG_BM - 1) / WG_BM;
  static int tgt_blocks = []() {
    const char* e = getenv("CYG_WG_BLOCKS");
    return e ? atoi(e) : 512;
  }();
  int target = std::max<long>(1, tgt_blocks / ((long)p.ktiles * p.ntiles));
  int slices = (int)std::min<long>(mchunks, target);
  p.mchunks_per_slice = (mchunks + slices - 1) / slices;
  // re-derive so no slice is empty (ceil division can overshoot)
  p.slices = (int)((mchunks + p.mchunks_per_slice - 1) / p.mchunks_per_slice);
  dim3 grid((long)p.ktiles * p.ntiles * p.slices);
  bool glds_ok = (p.Cin % 8) == 0 && (p.Cout % 8) == 0 &&
                 (long)p.B * p.H * p.W * p.Cin * 2 < (1L << 31) &&
                 p.M * p.Cout * 2 < (1L << 31);
  auto stream = at::cuda::getCurrentCUDAStream();
  if (glds_ok) {
    auto dw = at::empty({p.Cout, (long)KH, (long)KW, p.Cin},
                        x.options().dtype(at::kFloat));
    p.dw = (float*)dw.mutable_data_ptr();
    int wbn = (conv_nw() == 8 && conv_bn() == 128 && (p.Cout % 128) == 0)
                  ? 128 : WG_BN;
    if (p.Cout <= 16) wbn = 16;  // tiny-N heads: 16-wide n-tiles
    if (wbn != WG_BN) {
      p.ntiles = (p.Cout + wbn - 1) / wbn;
      // re-balance the split-M slices for the changed tile count
      long mchunks = (p.M + WG_BM - 1) / WG_BM;
      static int tgt2 = []() {
        const char* e = getenv("CYG_WG_BLOCKS");
        return e ? atoi(e) : 512;
      }();
      int target = std::max<long>(1, tgt2 / ((long)p.ktiles * p.ntiles));
      p.slices = (int)std::min<long>(mchunks, target);
      p.mchunks_per_slice = (mchunks + p.slices - 1) / p.slices;
      p.slices = (int)((mchunks + p.mchunks_per_slice - 1) /
                       p.mchunks_per_slice);
      grid = dim3((long)p.ktiles * p.ntiles * p.slices);
    }
    static int wg_nw = []() {
      const char* e = getenv("CYG_WG_NW");
      return e ? atoi(e) : 8;
    }();
    static int wg_kt = []() {
      // measured NEGATIVE (K3 wgrad 65.8 vs 45.2 us; bench 300 vs 326):
      // the 96 KB LDS footprint drops occupancy to 1 block/CU and the
      // lost latency hiding dwarfs the amortized staging. CYG_WG_KT=2
      // to re-enable.
      const char* e = getenv("CYG_WG_KT");
      return e ? atoi(e) : 1;
    }();
    // 2 k-tiles per block (wide shapes with an even k-tile count):
    // re-balance the split-M slices for the halved block count
    bool kt2 = wbn == 128 && wg_nw == 8 && wg_kt == 2 &&
               (p.ktiles % 2) == 0;
    if (kt2) {
      long mchunks2 = (p.M + WG_BM - 1) / WG_BM;
      int pairs = p.ktiles / 2;
      int target2 =
          std::max<long>(1, tgt_blocks / ((long)pairs * p.ntiles));
      p.slices = (int)std::min<long>(mchunks2, target2);
      p.mchunks_per_slice = (mchunks2 + p.slices - 1) / p.slices;
      p.slices = (int)((mchunks2 + p.mchunks_per_slice - 1) /
                       p.mchunks_per_slice);
      grid = dim3((long)pairs * p.ntiles * p.slices);
    }
    auto ws = at::empty({(long)p.slices * p.ktiles * p.ntiles *
                         wbn * WG_BK},
                        x.options().dtype(at::kFloat));
    p.ws = (float*)ws.mutable_data_ptr();
    if (wbn == 128) {
      constexpr size_t SMB = sizeof(WgSmemT<128>);
      constexpr size_t SMB2 = sizeof(WgSmemT<128, 2>);
      static bool init = []() {
        hipFuncSetAttribute((const void*)(wgrad_glds_kernel<8, 128>),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)SMB);
        hipFuncSetAttribute((const void*)(wgrad_glds_kernel<4, 128>),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)SMB);
        hipFuncSetAttribute((const void*)(wgrad_glds_kernel<8, 128, 2>),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)SMB2);
        return true;
      }();
      (void)init;
      if (kt2)
        hipLaunchKernelGGL((wgrad_glds_kernel<8, 128, 2>), grid, dim3(512),
                           SMB2, stream, p);
      else if (wg_nw == 4)
        hipLaunchKernelGGL((wgrad_glds_kernel<4, 128>), grid, dim3(256), SMB,
                           stream, p);
      else
        hipLaunchKernelGGL((wgrad_glds_kernel<8, 128>), grid, dim3(512), SMB,
                           stream, p);
    } else if (wbn == 16) {
      hipLaunchKernelGGL((wgrad_glds_kernel<8, 16>), grid, dim3(512),
                         sizeof(WgSmemT<16>), stream, p);
    } else if (conv_nw() == 8) {
      hipLaunchKernelGGL((wgrad_glds_kernel<8, 64>), grid, dim3(512),
                         sizeof(WgSmemT<64>), stream, p);
    } else {
      hipLaunchKernelGGL((wgrad_glds_kernel<4, 64>), grid, dim3(NTHREADS),
                         sizeof(WgSmemT<64>), stream, p);
    }
    long total = (long)p.ktiles * WG_BK * p.ntiles * wbn;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv(total, 256)),
                       dim3(256), 0, stream,
                       (const float*)ws.const_data_ptr(), p.dw, p.KTOT,
                       p.Cout, p.ktiles, p.ntiles, p.slices, wbn);
    return dw;
  }
  auto dw = at::zeros({p.Cout, (long)KH, (long)KW, p.Cin},
                      x.options().dtype(at::kFloat));
  p.dw = (float*)dw.mutable_data_ptr();
  hipLaunchKernelGGL(wgrad_kernel, grid, dim3(NTHREADS), 0, stream, p);
  return dw;
}

// ---- fp8 host wrappers ----
at::Tensor quant_fp8(at::Tensor x, at::Tensor scale) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.is_contiguous());
  TORCH_CHECK(scale.scalar_type() == at::kFloat);
  auto y = at::empty_like(x, x.options().dtype(at::kByte));
  long n = x.numel();
  long blocks = (n / 8 + 255) / 256 + 1;
  hipLaunchKernelGGL(quant_fp8_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const short*)x.const_data_ptr(),
                     (const float*)scale.const_data_ptr(),
                     (unsigned char*)y.mutable_data_ptr(), n);
  return y;
}

at::Tensor quant_fp8_d(at::Tensor x, at::Tensor amax_prev,
                       at::Tensor amax_cur) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 &&
              x.is_contiguous());
  TORCH_CHECK(amax_prev.scalar_type() == at::kFloat &&
              amax_cur.scalar_type() == at::kFloat);
  auto y = at::empty_like(x, x.options().dtype(at::kByte));
  long n = x.numel();
  long blocks = std::min<long>((n / 8 + 255) / 256 + 1, 768);
  hipLaunchKernelGGL(quant_fp8_d_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const short*)x.const_data_ptr(),
                     (const float*)amax_prev.const_data_ptr(),
                     (float*)amax_cur.mutable_data_ptr(),
                     (unsigned char*)y.mutable_data_ptr(), n);
  return y;
}

void amax_roll(at::Tensor arena, int64_t n) {
  // arena [2, cap] fp32: prev <- cur; cur <- 0 for the first n slots
  TORCH_CHECK(arena.is_cuda() && arena.scalar_type() == at::kFloat &&
              arena.dim() == 2 && arena.size(0) == 2 && arena.is_contiguous());
  int cap = (int)arena.size(1);
  TORCH_CHECK(n <= cap);
  hipLaunchKernelGGL(amax_roll_kernel, dim3(cdiv(n, 256)), dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (float*)arena.mutable_data_ptr(), (int)n, cap);
}

// conv_fp8_kernel always runs 128x64 tiles in plain row order, so the
// stats_slabs rule reduces to: every M-tile inside one sample, the slab
// count under the same cap, and the same Cout limits.
static int stats_slabs_fp8(const ConvParams& p) {
  const int cap = stats_cap();
  if (cap <= 0 || p.Cout <= 16 || (p.Cout % 8) != 0) return 0;
  long per = (long)p.OH * p.OW;
  if (per % BM != 0 || per / BM > cap) return 0;
  return (int)(per / BM);
}

// want_stats: {y, psum, psq} when stats_slabs_fp8 finds the call eligible,
// {y} otherwise; y is the same either way.
static std::vector<at::Tensor> conv2d_fp8_fwd_impl(
    at::Tensor xq, at::Tensor wq, at::Tensor dq, c10::optional<at::Tensor> sw,
    c10::optional<at::Tensor> bias, int64_t stride, int64_t pt, int64_t pb,
    int64_t pl, int64_t pr, bool reflect, int64_t act, double slope,
    bool want_stats) {
  TORCH_CHECK(xq.is_cuda() && xq.scalar_type() == at::kByte && xq.is_contiguous());
  TORCH_CHECK(wq.scalar_type() == at::kByte && wq.is_contiguous());
  TORCH_CHECK(xq.size(3) == wq.size(3) && xq.size(3) % 16 == 0,
              "fp8 conv: Cin % 16 != 0");
  int H = xq.size(1), W = xq.size(2);
  int KH = wq.size(1), KW = wq.size(2);
  int OH = (H + pt + pb - KH) / stride + 1;
  int OW = (W + pl + pr - KW) / stride + 1;
  auto y = at::empty({xq.size(0), OH, OW, wq.size(0)},
                     xq.options().dtype(at::kBFloat16));
  ConvParams p{};
  p.x = (const short*)xq.const_data_ptr();
  p.w = (const short*)wq.const_data_ptr();
  p.bias = bias.has_value() ? (const short*)bias->const_data_ptr() : nullptr;
  p.dq = (const float*)dq.const_data_ptr();
  p.dqb = sw.has_value() ? (const float*)sw->const_data_ptr() : nullptr;
  p.y = (short*)y.mutable_data_ptr();
  p.B = xq.size(0); p.H = H; p.W = W; p.Cin = xq.size(3);
  p.OH = OH; p.OW = OW; p.Cout = wq.size(0);
  p.KH = KH; p.KW = KW;
  p.stride = stride; p.pt = pt; p.pl = pl;
  p.reflect = reflect ? 1 : 0;
  p.act = act; p.slope = (float)slope;
  p.M = (long)p.B * OH * OW;
  p.KTOT = (long)KH * KW * p.Cin;
  p.mtiles = cdiv(p.M, BM);
  p.ntiles = cdiv(p.Cout, BN);
  TORCH_CHECK((long)p.B * H * W * p.Cin < (1L << 31) &&
              (long)p.Cout * p.KTOT < (1L << 31));
  std::vector<at::Tensor> out{y};
  const int ns = want_stats ? stats_slabs_fp8(p) : 0;
  if (ns > 0) {
    auto ps = at::empty({2, ns, (long)p.B, (long)p.Cout},
                        y.options().dtype(at::kFloat));
    p.psum = (float*)ps.mutable_data_ptr();
    p.psq = p.psum + (long)ns * p.B * p.Cout;
    p.tps = ns;
    out.push_back(ps[0]);
    out.push_back(ps[1]);
  }
  auto stream = at::cuda::getCurrentCUDAStream();
  dim3 grid(p.mtiles * p.ntiles);
#define LAUNCH_FP8(S)                                                        \
  do {                                                                       \
    if (ns > 0)                                                              \
      hipLaunchKernelGGL((conv_fp8_kernel<S, true>), grid, dim3(NTHREADS),   \
                         0, stream, p);                                      \
    else                                                                     \
      hipLaunchKernelGGL((conv_fp8_kernel<S, false>), grid, dim3(NTHREADS),  \
                         0, stream, p);                                      \
  } while (0)
  switch (p.stride) {
    case 1: LAUNCH_FP8(1); break;
    case 2: LAUNCH_FP8(2); break;
    default: LAUNCH_FP8(0);
  }
#undef LAUNCH_FP8
  return out;
}

at::Tensor conv2d_fp8_fwd(at::Tensor xq, at::Tensor wq, at::Tensor dq,
                          c10::optional<at::Tensor> sw,
                          c10::optional<at::Tensor> bias, int64_t stride,
                          int64_t pt, int64_t pb, int64_t pl, int64_t pr,
                          bool reflect, int64_t act, double slope) {
  return conv2d_fp8_fwd_impl(xq, wq, dq, sw, bias, stride, pt, pb, pl, pr,
                             reflect, act, slope, false)[0];
}

std::vector<at::Tensor> conv2d_fp8_fwd_stats(
    at::Tensor xq, at::Tensor wq, at::Tensor dq, c10::optional<at::Tensor> sw,
    c10::optional<at::Tensor> bias, int64_t stride, int64_t pt, int64_t pb,
    int64_t pl, int64_t pr, bool reflect, int64_t act, double slope) {
  return conv2d_fp8_fwd_impl(xq, wq, dq, sw, bias, stride, pt, pb, pl, pr,
                             reflect, act, slope, true);
}

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

// ---- MFMA layout probe (test aid): C[16,16] = A[16,32] @ Bt[16,32]^T ----
// MX-scaled fp8 MFMA probe (round-2 prep): raw per-lane operand dump for
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
