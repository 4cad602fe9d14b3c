// Implicit-GEMM NHWC convolutions on gfx950 MFMA (bf16 in, fp32 accumulate).
//
// Two gathers and one weight gradient cover every conv op in the framework
// (SURVEY §2.3 K1-K6):
//   conv   (IS_CONVT=false)  y[b,oh,ow,n] = act(Σ_{dk,ci} x[b,oh*s+dk-pt,ci]·w[n,dk,ci] + bias)
//          (also conv_transpose dgrad, via the channel-transposed weight)
//   convT  (IS_CONVT=true)   y[b,i,j,n]   = act(Σ_{dk,ci; i=s*o+dk-pt} in[b,o,ci]·w[n,dk,ci] + bias)
//          (also conv2d dgrad: same gather, channel-transposed weight, no tap flip)
//   wgrad  dw[n,dk,ci] = Σ_{b,o} x_patch[m,(dk,ci)]·dy[m,n]   (fp32, split-M)
//
// Kernels in this file:
//   conv_glds_kernel     production conv/convT: LDS-DMA staging, n-tile
//                        16/64/128 (conv_ntile), PHASED form for the
//                        stride-2 convT, RING form for the reflect dgrad
//                        (window tiles first, tap-trimmed ring tiles
//                        last); optional InstanceNorm slab epilogue
//   conv_gemm_kernel     fallback for Cin % 8 != 0 or tensors past 2 GiB
//   conv_fp8_kernel      e4m3 forward conv (quant_fp8_kernel,
//                        quant_fp8_d_kernel, amax_roll_kernel feed it)
//   wgrad_glds_kernel    production wgrad: split-M slabs summed by
//                        wgrad_reduce_kernel, no atomics
//   wgrad_kernel         fallback for Cin % 8 != 0 or Cout % 8 != 0
//                        (fp32 atomics over the split-M slices)
//   reflect_ring_add_kernel  reflect dgrad: adds the pad ring onto the
//                        mirrored rows/columns of dx (the gather writes the
//                        unpadded frame itself)
//   reflect_fold_kernel  full-frame fold of a padded-frame dgrad (fallback
//                        path and CYG_NO_DIRECT_FOLD=1)
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
// via the mfma_probe binding of probes.hip and oracle comparisons).

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "common.h"

namespace cyg {

constexpr int BM = 128, BN = 64, BK = 64;
constexpr int NTHREADS = 256;
constexpr int LDK = BK + 8;  // +16B pad: conflict-free b128 column-of-rows reads

// ---------------- reflect dgrad: layout and row order ----------------
#define HDEV __host__ __device__ __forceinline__

// Compact layout of the padded-frame pixels outside the window, per
// sample: the rows above the window, then the rows below it (both OW
// wide), then for each window row its left and right pieces side by side.
// Shared by the dgrad row decode and reflect_ring_add_kernel.
HDEV int ring_index(int qh, int qw, int OH, int OW, int wt, int wl, int wH,
                    int wW) {
  if (qh < wt) return qh * OW + qw;
  if (qh >= wt + wH) return (qh - wH) * OW + qw;
  return (OH - wH) * OW + (qh - wt) * (OW - wW) + (qw < wl ? qw : qw - wW);
}

// Which GEMM row of the direct-fold reflect dgrad is which pixel of the
// padded frame [B, pt+H+pb, pl+W+pr]. Only the enumeration lives here;
// where a pixel is stored is ring_index's business and does not depend on
// the order.
//   window tiles (tile < wtiles): the B*H*W window pixels in (b,i,j)
//     order, i.e. the forward conv's tiles; they run every tap.
//   ring tiles, behind them: the pixels outside the window in four
//     classes (top rows, bottom rows, left and right pieces of the window
//     rows), each in (b,qh,qw) order and padded to whole tiles, so a tile
//     holds one class and its rows share a tap window (reflect_taps).
// frame = 1 (CYG_DGRAD_FRAME_ORDER=1) enumerates the padded frame row by
// row instead: every tile is a "window" tile and there are no ring tiles.
struct ReflectOrder {
  int B, H, W;         // the window: the unpadded image
  int pt, pb, pl, pr;  // ring widths
  int KH, KW;
  int frame;           // rows enumerate the padded frame
  int trim;            // ring tiles walk only their class's taps
  int wtiles;          // tiles before the first ring tile
  int cstart[5];       // first tile of top, bottom, left, right; [4] = all
  int crows[4];        // rows of each class, all samples together
};

// Taps of a ring class that can have a source inside dy, as the rectangle
// [kh0,kh1) x [kw0,kw1): the source row is oh = qh - kh in [0, HP-KH+1).
// A top row has qh < pt, so kh <= qh < pt; a bottom row qh >= HP-pb, so
// kh > qh - (HP-KH+1) >= KH-pb-1; columns alike. cls 0 (window) and
// untrimmed calls get every tap.
struct TapWindow { int kh0, kh1, kw0, kw1; };
HDEV TapWindow reflect_taps(const ReflectOrder& o, int cls) {
  TapWindow t = {0, o.KH, 0, o.KW};
  if (!o.trim) return t;
  if (cls == 1) t.kh1 = o.pt < o.KH ? o.pt : o.KH;
  if (cls == 2) t.kh0 = o.KH > o.pb ? o.KH - o.pb : 0;
  if (cls == 3) t.kw1 = o.pl < o.KW ? o.pl : o.KW;
  if (cls == 4) t.kw0 = o.KW > o.pr ? o.KW - o.pr : 0;
  return t;
}

// 0 = window (or any tile of the frame order), 1..4 = top, bottom, left,
// right. cstart is non-decreasing; an empty class has no tile.
HDEV int reflect_tile_class(const ReflectOrder& o, int tile) {
  if (tile < o.wtiles) return 0;
  return 1 + (tile >= o.cstart[1]) + (tile >= o.cstart[2]) +
         (tile >= o.cstart[3]);
}

// Row r of a tile: the padded-frame pixel (b, qh, qw), whether it is a row
// at all (ok), its class, its tile's tap window, and dst, its pixel slot in
// the [dx | ring] allocation (element offset = dst * channels).
struct ReflectRow {
  int ok, b, qh, qw, cls;
  TapWindow taps;
  long dst;
};
HDEV ReflectRow reflect_row(const ReflectOrder& o, int tile, int r) {
  const int HP = o.pt + o.H + o.pb, WP = o.pl + o.W + o.pr;
  ReflectRow d;
  d.cls = reflect_tile_class(o, tile);
  d.taps = reflect_taps(o, d.cls);
  if (d.cls == 0) {
    const long m = (long)tile * BM + r;
    const int fh = o.frame ? HP : o.H, fw = o.frame ? WP : o.W;
    d.ok = m < (long)o.B * fh * fw;
    const long mm = d.ok ? m : 0;
    d.qw = (int)(mm % fw) + (o.frame ? 0 : o.pl);
    d.qh = (int)((mm / fw) % fh) + (o.frame ? 0 : o.pt);
    d.b = (int)(mm / ((long)fw * fh));
  } else {
    const int c = d.cls;
    const int start = c == 1 ? o.cstart[0] : c == 2 ? o.cstart[1]
                    : c == 3 ? o.cstart[2] : o.cstart[3];
    const int rows = c == 1 ? o.crows[0] : c == 2 ? o.crows[1]
                   : c == 3 ? o.crows[2] : o.crows[3];
    const int wide = c <= 2 ? WP : c == 3 ? o.pl : o.pr;  // row length
    const int x = (tile - start) * BM + r;
    d.ok = x < rows;
    const int xx = d.ok ? x : 0;
    const int per = rows / o.B;  // rows of one sample
    d.b = xx / per;
    const int rem = xx - d.b * per;
    d.qh = rem / wide + (c == 1 ? 0 : c == 2 ? o.pt + o.H : o.pt);
    d.qw = rem % wide + (c == 4 ? o.pl + o.W : 0);
  }
  const int i = d.qh - o.pt, j = d.qw - o.pl;
  if ((unsigned)i < (unsigned)o.H && (unsigned)j < (unsigned)o.W) {
    d.dst = ((long)d.b * o.H + i) * o.W + j;
  } else {
    const long rp = (long)HP * WP - (long)o.H * o.W;
    d.dst = (long)o.B * o.H * o.W + d.b * rp +
            ring_index(d.qh, d.qw, HP, WP, o.pt, o.pl, o.H, o.W);
  }
  return d;
}

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
  // reflect dgrad straight into the unpadded frame (the RING instantiation
  // of conv_glds_kernel only): window pixels of the padded frame [B,OH,OW]
  // go to y as a [B,H,W,Cout] image, every other pixel to the compact ring
  // image behind it (ring_index below). ro says which GEMM row is which
  // pixel; mtiles counts its window and ring tiles together.
  ReflectOrder ro;
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

template <int BNT>
struct ConvSmemT {
  // small arrays first: keeps their ds offsets within the 16-bit
  // immediate range even when the tile images exceed 64 KiB
  long rowyb[BM];
  int rowih[BM], rowiw[BM];
  unsigned rowxb[BM];  // byte offset of batch base (tensors < 4 GiB)
  char rowok[BM];
  char _pad[16 - (BM % 16 ? BM % 16 : 16)];
  short A[2][BM * BK];   // double-buffered
  short Bt[2][BNT * BK];
};

constexpr int NW = 8;  // waves per block of the glds kernels (conv, wgrad)

template <bool IS_CONVT, int STRIDE, int BNT, bool PHASED = false,
          bool RING = false>
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
  auto& sm = *reinterpret_cast<ConvSmemT<BNT>*>(smem_raw);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  // stride-2 convT-gather decode prefers the hardware round-robin (its
  // taps scatter anyway and chunking hotspots DRAM channels): measured
  // -25% on the s2 dgrad shape, +6% on the K3 forward.
  int mt, nt;
  if (RING) {
    // RING (reflect dgrad into the unpadded frame, p.ro): the window tiles
    // take the low block ids, chunked over the XCDs among themselves like
    // a forward conv's; the short ring tiles take the highest ids, so they
    // are dispatched last and fill the tail of the launch.
    static_assert(!RING || (IS_CONVT && STRIDE == 1 && !PHASED), "RING");
    const int nbw = p.ro.wtiles * p.ntiles;
    const int rb = (int)blockIdx.x - nbw;
    if (rb < 0) {
      const int bid = xcd_chunk(blockIdx.x, nbw);
      mt = bid % p.ro.wtiles; nt = bid / p.ro.wtiles;
    } else {
      const int rt = p.mtiles - p.ro.wtiles;
      mt = p.ro.wtiles + rb % rt; nt = rb / rt;
    }
  } else {
    const int bid = (IS_CONVT && STRIDE == 2)
                        ? blockIdx.x : xcd_chunk(blockIdx.x, gridDim.x);
    mt = bid % p.mtiles; nt = bid / p.mtiles;
  }
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
  // RING: a ring tile enumerates only its class's tap rectangle
  // (block-uniform, reflect_taps): tap counters (dkh, dkw) below run over
  // [0,kh1-kh0) x [0,nkw), the real tap is (kh0 + dkh, kw0 + dkw). Every
  // tap left out has no source inside dy for any row of the tile.
  const TapWindow tw =
      RING ? reflect_taps(p.ro, reflect_tile_class(p.ro, mt)) : TapWindow{};
  const int nkw = RING ? tw.kw1 - tw.kw0 : 0;
  const long KEFF = PHASED ? (long)nvh * nvw * p.Cin
                  : RING ? (long)(tw.kh1 - tw.kh0) * nkw * p.Cin : p.KTOT;
  const int tapw = PHASED ? nvw : RING ? nkw : p.KW;  // taps per counter row

  for (int r = tid; r < BM; r += NT) {
    if (RING) {
      const ReflectRow d = reflect_row(p.ro, mt, r);
      sm.rowok[r] = d.ok;
      sm.rowxb[r] = (unsigned)((long)d.b * p.H * p.W * p.Cin * 2);
      sm.rowyb[r] = d.dst * p.Cout;
      sm.rowih[r] = d.qh + p.pt - tw.kh0;  // oh = this - dkh
      sm.rowiw[r] = d.qw + p.pl - tw.kw0;
    } else if (PHASED) {
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

  unsigned xbytes = (unsigned)((long)p.B * p.H * p.W * p.Cin * 2);
  unsigned wbytes = (unsigned)(p.Cout * p.KTOT * 2);
  if (RING) {
    // hipcc shares these products with the per-row ones of reflect_row and
    // leaves them in VGPRs; a descriptor in VGPRs costs a readfirstlane
    // loop around every glds
    xbytes = __builtin_amdgcn_readfirstlane(xbytes);
    wbytes = __builtin_amdgcn_readfirstlane(wbytes);
  }
  auto rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, xbytes, 0x00020000);
  auto rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, wbytes, 0x00020000);

  const int nk = (int)((KEFF + BK - 1) / BK);
  const bool big_ci = p.Cin >= BK;  // wave-uniform

  // incremental gather state: recompute voffsets only at tap boundaries
  // (every Cin/64 K-steps); otherwise one predicated add per instruction.
  long kcur;
  bool kv;
  int ci, dkh, dkw;  // PHASED: (vh, vw); RING: counters inside tw
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
    if (RING)
      kw_idx = ((long)(tw.kh0 + dkh) * p.KW + (tw.kw0 + dkw)) * p.Cin + ci;
    #pragma unroll
    for (int j = 0; j < BPI; ++j)
      bvo[j] = (unsigned)(((long)bn[j] * p.KTOT + kw_idx) * 2);
  };

  auto decode_tap = [&]() {
    int tap = (int)(kcur / p.Cin);
    ci = (int)(kcur - (long)tap * p.Cin);
    dkh = tap / tapw;          // PHASED: vh
    dkw = tap - dkh * tapw;    // PHASED: vw
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
        if (++dkw == tapw) { dkw = 0; ++dkh; }
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

template <int WBN>
struct WgSmemT {
  short A[2][WG_BM * WG_BK];        // [m][k] swizzled
  short D[2][WG_BM * WBN];          // [m][n] swizzled
};

template <int WBN>
__global__ __launch_bounds__(NW * 64) void wgrad_glds_kernel(WgradParams p) {
  constexpr int API = 16 / NW;        // A glds instructions per wave
  constexpr int DCH = WBN / 8;        // 16-B chunks per D row
  constexpr int DRPI = 64 / DCH;      // D rows per glds instruction
  constexpr int TDI = (WG_BM * DCH) / 64;   // D glds instructions total
  constexpr int DPI = TDI >= NW ? TDI / NW : 1;  // per wave (maybe idle)
  constexpr int NFW = WBN >= 32 ? 2 : 1;    // n-fragments per wave
  constexpr int NWCW = WBN / (NFW * 16);    // wave-grid columns
  constexpr int KF = (WG_BK / (NW / NWCW)) / 16;  // k-fragments per wave
  extern __shared__ __attribute__((aligned(16))) char wg_smem_raw[];
  auto& sm = *reinterpret_cast<WgSmemT<WBN>*>(wg_smem_raw);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int wbid = xcd_chunk(blockIdx.x, gridDim.x);
  const int kt = wbid % p.ktiles;
  const int nt = (wbid / p.ktiles) % p.ntiles;
  const int sl = wbid / (p.ktiles * p.ntiles);
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
    long chunk = (((long)sl * p.ktiles + kt) * p.ntiles + nt) *
                 ((long)WBN * WG_BK);
    for (int i = tid; i < WBN * WG_BK; i += NW * 64) p.ws[chunk + i] = 0.f;
    return;
  }

  auto rx = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.x, 0, (unsigned)((long)p.B * p.H * p.W * p.Cin * 2), 0x00020000);
  auto rd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.dy, 0, (unsigned)(p.M * p.Cout * 2), 0x00020000);

  // ---- per-lane gather identities ----
  // A: 16 instrs: instr i covers rows i*4..i*4+3; per-wave share = API
  int a_row[API], a_ci[API], a_dkh[API], a_dkw[API];
  bool a_kv[API];
  #pragma unroll
  for (int j = 0; j < API; ++j) {
    int row = (w * API + j) * 4 + (lane >> 4);
    int cb = ((lane & 15) * 16) ^ AXOR(row);
    long k = k0 + cb / 2;
    a_row[j] = row;
    a_kv[j] = k < p.KTOT;
    int tap = a_kv[j] ? (int)(k / p.Cin) : 0;
    a_ci[j] = (int)(k - (long)tap * p.Cin);
    a_dkh[j] = tap / p.KW;
    a_dkw[j] = tap - a_dkh[j] * p.KW;
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
  int a_ow[API], a_oh[API], a_b[API], a_ih[API], a_iw[API];
  unsigned avo[API];
  bool ainb[API], avalid[API], a_iw_ok[API];
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
  for (int j = 0; j < API; ++j) {
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
      for (int j = 0; j < API; ++j) {
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
      for (int j = 0; j < API; ++j) {
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
    for (int j = 0; j < API; ++j) {
      unsigned vo = (!tail || ms + a_row[j] < p.M) ? avo[j] : 0xFF000000u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rx, (__attribute__((address_space(3))) void*)&sm.A[buf][(w * API + j) * 512],
          16, vo, 0, 0, 0);
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

  v4f acc[KF][NFW] = {};
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
      v8bf a[KF];
      #pragma unroll
      for (int kf = 0; kf < KF; ++kf) {
        v4bfx lo = tr16_read(Ab + kk * 256 + a_base[kf][0]);
        v4bfx hi = tr16_read(Ab + kk * 256 + a_base[kf][1]);
        a[kf] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
      #pragma unroll
      for (int kf = 0; kf < KF; ++kf)
        #pragma unroll
        for (int nf = 0; nf < NFW; ++nf)
          acc[kf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[kf], bfr[nf], acc[kf][nf], 0, 0, 0);
    }
    __syncthreads();
  }

  // slab store (no atomics): chunk layout [WBN][WG_BK], float4 rows
  const long chunk = (((long)sl * p.ktiles + kt) * p.ntiles + nt) *
                     ((long)WBN * WG_BK);
  #pragma unroll
  for (int nf = 0; nf < NFW; ++nf) {
    int nl = wn0 + nf * 16 + fr;
    if (nl >= WBN) continue;
    #pragma unroll
    for (int kf = 0; kf < KF; ++kf) {
      int kl = wk0 + kf * 16 + fg * 4;
      *(float4*)&p.ws[chunk + (long)nl * WG_BK + kl] =
          *(const float4*)&acc[kf][nf];
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

// wgrad_reduce_kernel that finishes the gradient where the optimizer reads
// it: out is the parameter's own OHWI block (typically a 4-byte-aligned
// view into the flat grad buffer, hence scalar stores). The slab sum is the
// same four chains as above; what differs is the store:
//   crop     the GEMM ran on channel counts padded to 8 (cin_g, Cout);
//            elements outside (co_true, ci_true) are skipped
//   tr       transpose-conv gradient: the GEMM result is [Cin_w,KH,KW,Cout_w]
//            and (n, tap, ci) goes to out[ci][tap][n]
//   accum    out += sum (one more fp32 add, performed last) for a parameter
//            that already received a gradient in this backward pass
__global__ void wgrad_reduce_into_kernel(const float* __restrict__ ws,
                                         float* __restrict__ out, long KTOT,
                                         int Cout, int ktiles, int ntiles,
                                         int slices, int wbn, int cin_g,
                                         int taps, int co_true, int ci_true,
                                         int tr, int accum) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)ktiles * WG_BK * ntiles * wbn;
  if (idx >= total) return;
  int kl = (int)(idx % WG_BK);
  long t = idx / WG_BK;
  int kt = (int)(t % ktiles);
  t /= ktiles;
  int nl = (int)(t % wbn);
  int nt = (int)(t / wbn);
  long k = (long)kt * WG_BK + kl;
  int n = nt * wbn + nl;
  if (k >= KTOT || n >= Cout) return;
  int tap = (int)(k / cin_g);
  int ci = (int)(k - (long)tap * cin_g);
  if (n >= co_true || ci >= ci_true) return;
  long stride = (long)ktiles * ntiles * wbn * WG_BK;
  long off = (((long)kt * ntiles + nt) * wbn + nl) * WG_BK + kl;
  float s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  int sl = 0;
  for (; sl + 4 <= slices; sl += 4) {
    s0 += ws[off + (sl + 0) * stride];
    s1 += ws[off + (sl + 1) * stride];
    s2 += ws[off + (sl + 2) * stride];
    s3 += ws[off + (sl + 3) * stride];
  }
  for (; sl < slices; ++sl) s0 += ws[off + sl * stride];
  float s = (s0 + s1) + (s2 + s3);
  long o = tr ? ((long)ci * taps + tap) * co_true + n
              : ((long)n * taps + tap) * ci_true + ci;
  out[o] = accum ? out[o] + s : s;
}

// packed-head fold: the packed wgrad's [64, KH, 2, 8*I] result (n = d*8+co,
// the 8 pixel shifts d folded into N) -> OHWI [O, KH, KW, I] with O <= 8,
// KW <= 9. One thread per output element, its eight d terms summed in
// ascending d: dw[co][ty][tx][ci] = Σ_d dwp[d*8+co][ty][blk][pos*I+ci],
// blk*8+pos = tx+d.
__global__ void fold_packed_dw_kernel(const float* __restrict__ dwp,
                                      float* __restrict__ out, int O, int KH,
                                      int KW, int I, int accum) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)O * KH * KW * I;
  if (idx >= total) return;
  int ci = (int)(idx % I);
  long t = idx / I;
  int tx = (int)(t % KW);
  t /= KW;
  int ty = (int)(t % KH);
  int co = (int)(t / KH);
  float s = 0.f;
  #pragma unroll
  for (int d = 0; d < 8; ++d) {
    int a = tx + d;  // < 16
    s += dwp[((((long)(d * 8 + co) * KH + ty) * 2 + (a >> 3)) * 8 + (a & 7)) *
                 I + ci];
  }
  out[idx] = accum ? out[idx] + s : s;
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

// Up to two disjoint index intervals [a0, a0+n0) and [a1, a1+n1) with
// a0 + n0 <= a1: the rows (or columns) of the image that have a mirror
// source in the padded frame.
struct Span2 { int a0, n0, a1, n1; };
DEV int span_nth(Span2 s, int k) {      // k-th index inside
  return k < s.n0 ? s.a0 + k : s.a1 + (k - s.n0);
}
DEV int span_nth_out(Span2 s, int k) {  // k-th index outside
  if (k >= s.a0) k += s.n0;
  if (k >= s.a1) k += s.n1;
  return k;
}

// ---------------- reflect ring add (direct-fold dgrad) ----------------
// The dgrad has written window pixels of the padded frame straight into
// dx and the others into the ring image (ReflectRow::dst). Only dx
// pixels in a mirrored row or column (rs / cs) receive anything more; one
// thread per 8 channels of such a pixel re-sums it in
// reflect_fold_kernel's candidate order (rows outer, cols inner; direct,
// low mirror, high mirror; same de-duplication), the direct term from dx
// itself and every mirror term from the ring, rounds once and writes in
// place. No thread reads another thread's dx pixel.
__global__ void reflect_ring_add_kernel(short* __restrict__ dx,
                                        const short* __restrict__ ring,
                                        int B, int H, int W, int C,
                                        int pt, int pb, int pl, int pr,
                                        Span2 rs, Span2 cs) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int gpr = C / 8;
  const int nr = rs.n0 + rs.n1, nc = cs.n0 + cs.n1;
  const int ppb = nr * W + (H - nr) * nc;  // pixels per sample
  long total = (long)B * ppb * gpr;
  if (idx >= total) return;
  int g = (int)(idx % gpr);
  long t = idx / gpr;
  int q = (int)(t % ppb);
  int b = (int)(t / ppb);
  int i, j;
  if (q < nr * W) {
    i = span_nth(rs, q / W);
    j = q % W;
  } else {
    q -= nr * W;
    i = span_nth_out(rs, q / nc);
    j = span_nth(cs, q % nc);
  }
  int HP = H + pt + pb, WP = W + pl + pr;
  long rp = (long)HP * WP - (long)H * W;
  short* own = dx + (((long)b * H + i) * W + j) * C + g * 8;
  float s[8] = {};
  int hc[3] = {pt + i, pt - i, pt + 2 * (H - 1) - i};
  int wc_[3] = {pl + j, pl - j, pl + 2 * (W - 1) - j};
  #pragma unroll
  for (int a = 0; a < 3; ++a) {
    int qh = hc[a];
    if (qh < 0 || qh >= HP) continue;
    if (a > 0 && qh == hc[0]) continue;
    if (a == 2 && qh == hc[1]) continue;
    if (mirror_idx(qh - pt, H) != i) continue;
    #pragma unroll
    for (int d = 0; d < 3; ++d) {
      int qw = wc_[d];
      if (qw < 0 || qw >= WP) continue;
      if (d > 0 && qw == wc_[0]) continue;
      if (d == 2 && qw == wc_[1]) continue;
      if (mirror_idx(qw - pl, W) != j) continue;
      // a surviving mirror candidate lies outside the window
      const short* src = (a == 0 && d == 0)
          ? own
          : ring + (b * rp + ring_index(qh, qw, HP, WP, pt, pl, H, W)) * C +
                g * 8;
      v8s v = *(const v8s*)src;
      #pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += b2f(v[e]);
    }
  }
  v8s out;
  #pragma unroll
  for (int e = 0; e < 8; ++e) out[e] = f2b(s[e]);
  *(v8s*)own = out;
}

// ================= host wrappers =================

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// A/B switches that are read on every call (a test flips them inside one
// process): pass the getenv() result.
static inline bool env_flag(const char* v) { return v && v[0] == '1'; }

// Indices of an axis of length n that have a mirror source under reflect
// pads (lo, hi): 1..lo from the low side, n-1-hi..n-2 from the high side
// (reflect_fold_kernel's surviving candidates), merged where they touch.
static Span2 mirror_span(int n, int lo, int hi) {
  const int a0 = 1, b0 = std::min(lo, n - 1);
  const int a1 = std::max(n - 1 - hi, 0), b1 = n - 2;
  const int n0 = std::max(b0 - a0 + 1, 0), n1 = std::max(b1 - a1 + 1, 0);
  if (n0 == 0) return {a1, n1, a1 + n1, 0};
  if (n1 == 0) return {a0, n0, a0 + n0, 0};
  if (a1 <= a0 + n0) {
    const int a = std::min(a0, a1), b = std::max(b0, b1);
    return {a, b - a + 1, b + 1, 0};
  }
  return {a0, n0, a1, n1};
}

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

// n-tile width of the glds kernels: the one rule shared by the plain glds
// launch, the phased convT launch and conv2d_wgrad.
static int conv_ntile(int Cout) {
  if (Cout <= 16) return 16;  // tiny-N (the 1-8 channel heads, padded to 8)
  // wider n-tile: 1.5x arithmetic intensity for Cout >= 128 layers
  return (Cout % 128) == 0 ? 128 : 64;
}

template <bool IS_CONVT, int STRIDE, int BNT, bool PHASED = false,
          bool RING = false>
static void launch_one_glds(const ConvParams& p, hipStream_t stream) {
  constexpr size_t SMB = sizeof(ConvSmemT<BNT>);
  static bool init = []() {
    hipFuncSetAttribute(
        (const void*)(conv_glds_kernel<IS_CONVT, STRIDE, BNT, PHASED, RING>),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMB);
    return true;
  }();
  (void)init;
  hipLaunchKernelGGL((conv_glds_kernel<IS_CONVT, STRIDE, BNT, PHASED, RING>),
                     dim3((long)p.mtiles * p.ntiles), dim3(NW * 64), SMB,
                     stream, p);
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "conv_glds launch failed (BNT=", BNT,
              " PHASED=", PHASED, " RING=", RING, "): ",
              hipGetErrorString(err));
}

// Row order of the direct-fold reflect dgrad (ReflectOrder). frame: the
// plain padded-frame enumeration; trim: ring tiles walk only their tap
// window (the caller allows it when the gather's Cin % BK == 0, so that
// every kept K-step is a K-step of the untrimmed walk).
static ReflectOrder reflect_order(int B, int H, int W, int pt, int pb, int pl,
                                  int pr, int KH, int KW, bool frame,
                                  bool trim) {
  ReflectOrder o{};
  o.B = B; o.H = H; o.W = W;
  o.pt = pt; o.pb = pb; o.pl = pl; o.pr = pr;
  o.KH = KH; o.KW = KW;
  o.frame = frame; o.trim = trim && !frame;
  const long HP = H + pt + pb, WP = W + pl + pr;
  o.wtiles = cdiv(frame ? B * HP * WP : (long)B * H * W, BM);
  const long rows[4] = {B * pt * WP, B * pb * WP, (long)B * H * pl,
                        (long)B * H * pr};
  o.cstart[0] = o.wtiles;
  for (int c = 0; c < 4; ++c) {
    o.crows[c] = frame ? 0 : (int)rows[c];
    o.cstart[c + 1] = o.cstart[c] + cdiv(o.crows[c], BM);
  }
  return o;
}

// The reflect dgrad gather: 64- or 128-wide n-tiles only (Cout <= 16 takes
// the 64-wide tile, as in the phased launch).
static void launch_ring(ConvParams p, hipStream_t stream) {
  p.mtiles = p.ro.cstart[4];
  if (conv_ntile(p.Cout) == 128) {
    p.ntiles = cdiv(p.Cout, 128);
    launch_one_glds<true, 1, 128, false, true>(p, stream);
  } else {
    p.ntiles = cdiv(p.Cout, 64);
    launch_one_glds<true, 1, 64, false, true>(p, stream);
  }
}

template <bool IS_CONVT, int BNT>
static void launch_glds_s(const ConvParams& p, hipStream_t stream) {
  switch (p.stride) {
    case 1: launch_one_glds<IS_CONVT, 1, BNT>(p, stream); break;
    case 2: launch_one_glds<IS_CONVT, 2, BNT>(p, stream); break;
    default: launch_one_glds<IS_CONVT, 0, BNT>(p, stream);
  }
}

template <bool IS_CONVT>
static void launch_glds(ConvParams p, hipStream_t stream) {
  const int bnt = conv_ntile(p.Cout);
  p.ntiles = cdiv(p.Cout, bnt);
  switch (bnt) {
    case 16: launch_glds_s<IS_CONVT, 16>(p, stream); break;
    case 128: launch_glds_s<IS_CONVT, 128>(p, stream); break;
    default: launch_glds_s<IS_CONVT, 64>(p, stream);
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
// Eligible = the kernel runs it with 64/128-wide n-tiles and every
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

// fp8: conv_fp8_kernel always runs 128x64 tiles in plain row order and its
// wrapper checks its own offset limits, so neither the phased regrouping
// nor the glds-eligibility term applies; everything else is shared.
static int stats_slabs(const ConvParams& p, bool is_convt, bool fp8,
                       int* tps) {
  const int cap = stats_cap();
  if (cap <= 0 || p.Cout <= 16 || (p.Cout % 8) != 0) return 0;
  if (!fp8 && !glds_eligible(p)) return 0;
  const bool phased = !fp8 && phased_eligible(p, is_convt);
  const long per = phased ? (long)(p.OH / 2) * (p.OW / 2)
                          : (long)p.OH * p.OW;
  const long ns = (phased ? 4 : 1) * (per / BM);
  if (per % BM != 0 || ns > cap) return 0;
  *tps = (int)(per / BM);
  return (int)ns;
}

static void launch_conv(const ConvParams& p, bool is_convt, hipStream_t stream) {
  if (phased_eligible(p, is_convt)) {
    // phase-decomposed: 4 phase classes, only matching-parity taps. The
    // phased kernel has no 16-wide form; tiny Cout takes the 64-wide tile.
    ConvParams q = p;
    long Mp = (long)q.B * (q.OH / 2) * (q.OW / 2);
    q.mtiles = 4 * cdiv(Mp, BM);
    if (conv_ntile(q.Cout) == 128) {
      q.ntiles = cdiv(q.Cout, 128);
      launch_one_glds<true, 2, 128, true>(q, stream);
    } else {
      launch_one_glds<true, 2, 64, true>(q, stream);
    }
    return;
  }
  if (glds_eligible(p)) {
    if (is_convt) launch_glds<true>(p, stream);
    else launch_glds<false>(p, stream);
    return;
  }
  dim3 grid(p.mtiles * p.ntiles);
  bool aligned = (p.Cin % 8) == 0;
  if (is_convt) {
    if (aligned) launch_conv_s<true, true>(p, grid, stream);
    else launch_conv_s<true, false>(p, grid, stream);
  } else {
    if (aligned) launch_conv_s<false, true>(p, grid, stream);
    else launch_conv_s<false, false>(p, grid, stream);
  }
}

// x/w may be bf16 or (fp8 conv) e4m3 byte tensors: only their sizes and
// base pointers are read. The caller sets pt/pl/reflect (and dq/dqb).
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

// want_stats: when the call is eligible (stats_slabs), allocate the
// InstanceNorm partial slabs ([NS,B,Cout] fp32 each), point p at them and
// append {psum, psq} to out = {y}. Returns the slab count (0 = none).
static int add_stats(ConvParams& p, bool is_convt, bool fp8, bool want_stats,
                     std::vector<at::Tensor>& out) {
  int tps = 0;
  const int ns = want_stats ? stats_slabs(p, is_convt, fp8, &tps) : 0;
  if (ns > 0) {
    auto ps = at::empty({2, ns, (long)p.B, (long)p.Cout},
                        out[0].options().dtype(at::kFloat));
    p.psum = (float*)ps.mutable_data_ptr();
    p.psq = p.psum + (long)ns * p.B * p.Cout;
    p.tps = tps;
    out.push_back(ps[0]);
    out.push_back(ps[1]);
  }
  return ns;
}

static std::vector<at::Tensor> run_fwd(ConvParams& p, at::Tensor& y,
                                       bool is_convt, bool want_stats) {
  std::vector<at::Tensor> out{y};
  add_stats(p, is_convt, false, want_stats, out);
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
  TORCH_CHECK(wt.size(0) % 8 == 0, "reflect dgrad: Cin % 8 != 0");
  long HP = H + pt + pb, WP = W + pl + pr;
  // Direct fold: the gather writes window pixels of the padded frame
  // straight into dx and only the ring around it into a side image, then
  // reflect_ring_add_kernel adds the ring onto the mirrored rows and
  // columns in place. glds path and stride 1 only (no model pairs reflect
  // padding with a stride; that and the conv_gemm_kernel fallback keep the
  // full-frame fold below). CYG_NO_DIRECT_FOLD=1, read per call, selects
  // the full-frame fold.
  const long B = dy.size(0), C = wt.size(0);
  const long nimg = B * H * W * C;
  auto dxp = at::empty({B, HP, WP, C}, dy.options());
  auto p = fill_common(dy, wt, c10::nullopt, dxp, stride, ACT_NONE, 0.0);
  p.pt = 0; p.pl = 0;
  int threads = 256;
  if (stride == 1 && HP * WP > H * W && glds_eligible(p) &&
      !env_flag(getenv("CYG_NO_DIRECT_FOLD"))) {
    // image + ring are exactly the padded frame's size: dx is the leading
    // [B,H,W,C] of the same allocation, the ring image the rest
    auto dx = dxp.view({-1}).narrow(0, 0, nimg).view({B, H, W, C});
    const int KH = wt.size(1), KW = wt.size(2);
    TORCH_CHECK(dy.size(1) == HP - KH + 1 && dy.size(2) == WP - KW + 1,
                "reflect dgrad: dy is not the stride-1 output frame");
    // Window tiles first, tap-trimmed ring tiles last (ReflectOrder).
    // CYG_DGRAD_FRAME_ORDER=1, read per call, enumerates the padded frame
    // instead and runs every tap everywhere (A/B runs, bisection).
    p.ro = reflect_order(B, H, W, pt, pb, pl, pr, KH, KW,
                         env_flag(getenv("CYG_DGRAD_FRAME_ORDER")),
                         p.Cin % BK == 0);
    launch_ring(p, stream);
    const Span2 rs = mirror_span(H, pt, pb), cs = mirror_span(W, pl, pr);
    const long nr = rs.n0 + rs.n1, nc = cs.n0 + cs.n1;
    const long total = B * (nr * W + (H - nr) * nc) * (C / 8);
    if (total > 0)
      hipLaunchKernelGGL(reflect_ring_add_kernel, dim3(cdiv(total, threads)),
                         dim3(threads), 0, stream, p.y, p.y + nimg, (int)B,
                         (int)H, (int)W, (int)C, (int)pt, (int)pb, (int)pl,
                         (int)pr, rs, cs);
    return dx;
  }
  // full-frame fold: dgrad into the padded frame, then fold mirrors back
  launch_conv(p, true, stream);
  auto dx = at::empty({B, H, W, C}, dy.options());
  long total = dx.numel() / 8;
  hipLaunchKernelGGL(reflect_fold_kernel, dim3(cdiv(total, threads)),
                     dim3(threads), 0, stream,
                     (const short*)dxp.const_data_ptr(),
                     (short*)dx.mutable_data_ptr(),
                     (int)dy.size(0), (int)H, (int)W, (int)wt.size(0),
                     (int)pt, (int)pb, (int)pl, (int)pr);
  return dx;
}

// The direct-fold reflect dgrad's row order as a CPU int32 table, one line
// [ok, b, qh, qw, cls, kh0, kh1, kw0, kw1, dst] per (tile, r), tiles in
// order: reflect_row, the function the kernel's prologue calls, run on the
// host. Launches nothing and needs no GPU.
at::Tensor reflect_dgrad_rowmap(int64_t B, int64_t H, int64_t W, int64_t pt,
                                int64_t pb, int64_t pl, int64_t pr,
                                int64_t KH, int64_t KW, bool trim,
                                bool frame) {
  TORCH_CHECK(B > 0 && H > 0 && W > 0 && KH > 0 && KW > 0 && pt >= 0 &&
              pb >= 0 && pl >= 0 && pr >= 0, "reflect_dgrad_rowmap: sizes");
  TORCH_CHECK(B * (H + pt + pb) * (W + pl + pr) < (1L << 24),
              "reflect_dgrad_rowmap: a table for small shapes");
  const ReflectOrder o =
      reflect_order(B, H, W, pt, pb, pl, pr, KH, KW, frame, trim);
  const int tiles = o.cstart[4];
  auto out = at::empty({(long)tiles * BM, 10}, at::kInt);
  int* t = out.data_ptr<int>();
  for (int tile = 0; tile < tiles; ++tile)
    for (int r = 0; r < BM; ++r, t += 10) {
      const ReflectRow d = reflect_row(o, tile, r);
      t[0] = d.ok; t[1] = d.b; t[2] = d.qh; t[3] = d.qw; t[4] = d.cls;
      t[5] = d.taps.kh0; t[6] = d.taps.kh1;
      t[7] = d.taps.kw0; t[8] = d.taps.kw1;
      t[9] = (int)d.dst;
    }
  return out;
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

// split M so total blocks ≈ 2-4x CU count (CYG_WG_BLOCKS to sweep)
struct WgSplit { int slices; long mchunks_per_slice; };  // chunks of 64 rows
static WgSplit wgrad_split(long M, int ktiles, int ntiles) {
  static const int tgt_blocks = []() {
    const char* e = getenv("CYG_WG_BLOCKS");
    return e ? atoi(e) : 512;
  }();
  const long mchunks = (M + WG_BM - 1) / WG_BM;
  const int target = std::max<long>(1, tgt_blocks / ((long)ktiles * ntiles));
  const int slices = (int)std::min<long>(mchunks, target);
  const long per = (mchunks + slices - 1) / slices;
  // re-derive so no slice is empty (ceil division can overshoot)
  return {(int)((mchunks + per - 1) / per), per};
}

template <int WBN>
static void launch_wgrad_glds(const WgradParams& p, dim3 grid,
                              hipStream_t stream) {
  constexpr size_t SMB = sizeof(WgSmemT<WBN>);
  if constexpr (WBN == 128) {  // the 64 KiB image needs the opt-in
    static bool init = []() {
      hipFuncSetAttribute((const void*)(wgrad_glds_kernel<128>),
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)SMB);
      return true;
    }();
    (void)init;
  }
  hipLaunchKernelGGL((wgrad_glds_kernel<WBN>), grid, dim3(NW * 64), SMB,
                     stream, p);
}

// into == nullptr: returns the GEMM-shaped [Cout,KH,KW,Cin] gradient.
// Otherwise the reduce writes (or adds to) *into, cropped / transposed as
// wgrad_reduce_into_kernel describes, and *into is returned.
static at::Tensor wgrad_impl(at::Tensor x, at::Tensor dy, int64_t KH,
                             int64_t KW, int64_t stride, int64_t pt,
                             int64_t pl, bool reflect, const at::Tensor* into,
                             bool accumulate, bool transpose_oi) {
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
  const bool glds_ok = (p.Cin % 8) == 0 && (p.Cout % 8) == 0 &&
                       (long)p.B * p.H * p.W * p.Cin * 2 < (1L << 31) &&
                       p.M * p.Cout * 2 < (1L << 31);
  // the unaligned-channel fallback (wgrad_kernel) has WG_BN-wide tiles only
  const int wbn = glds_ok ? conv_ntile(p.Cout) : WG_BN;
  p.ktiles = cdiv(p.KTOT, WG_BK);
  p.ntiles = cdiv(p.Cout, wbn);
  const WgSplit split = wgrad_split(p.M, p.ktiles, p.ntiles);
  p.slices = split.slices;
  p.mchunks_per_slice = split.mchunks_per_slice;
  dim3 grid((long)p.ktiles * p.ntiles * p.slices);
  auto stream = at::cuda::getCurrentCUDAStream();
  if (!glds_ok) {
    auto dw = at::zeros({p.Cout, (long)KH, (long)KW, p.Cin},
                        x.options().dtype(at::kFloat));
    p.dw = (float*)dw.mutable_data_ptr();
    hipLaunchKernelGGL(wgrad_kernel, grid, dim3(NTHREADS), 0, stream, p);
    if (!into) return dw;
    // no model shape comes here: finish with one ATen copy_/add_
    auto v = transpose_oi ? dw.permute({3, 1, 2, 0}) : dw;
    v = v.narrow(0, 0, into->size(0)).narrow(3, 0, into->size(3));
    if (accumulate) into->add_(v); else into->copy_(v);
    return *into;
  }
  at::Tensor dw;
  if (!into) {
    dw = at::empty({p.Cout, (long)KH, (long)KW, p.Cin},
                   x.options().dtype(at::kFloat));
    p.dw = (float*)dw.mutable_data_ptr();
  }
  auto ws = at::empty({(long)p.slices * p.ktiles * p.ntiles * wbn * WG_BK},
                      x.options().dtype(at::kFloat));
  p.ws = (float*)ws.mutable_data_ptr();
  switch (wbn) {
    case 16: launch_wgrad_glds<16>(p, grid, stream); break;
    case 128: launch_wgrad_glds<128>(p, grid, stream); break;
    default: launch_wgrad_glds<64>(p, grid, stream);
  }
  long total = (long)p.ktiles * WG_BK * p.ntiles * wbn;
  if (!into) {
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv(total, 256)),
                       dim3(256), 0, stream,
                       (const float*)ws.const_data_ptr(), p.dw, p.KTOT,
                       p.Cout, p.ktiles, p.ntiles, p.slices, wbn);
    return dw;
  }
  const int co_true = (int)into->size(transpose_oi ? 3 : 0);
  const int ci_true = (int)into->size(transpose_oi ? 0 : 3);
  hipLaunchKernelGGL(wgrad_reduce_into_kernel, dim3(cdiv(total, 256)),
                     dim3(256), 0, stream,
                     (const float*)ws.const_data_ptr(),
                     (float*)into->mutable_data_ptr(), p.KTOT, p.Cout,
                     p.ktiles, p.ntiles, p.slices, wbn, p.Cin, (int)(KH * KW),
                     co_true, ci_true, transpose_oi ? 1 : 0,
                     accumulate ? 1 : 0);
  return *into;
}

at::Tensor conv2d_wgrad(at::Tensor x, at::Tensor dy, int64_t KH, int64_t KW,
                        int64_t stride, int64_t pt, int64_t pl, bool reflect) {
  return wgrad_impl(x, dy, KH, KW, stride, pt, pl, reflect, nullptr, false,
                    false);
}

static void check_grad_dest(const at::Tensor& out, const char* who) {
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kFloat &&
                  out.is_contiguous(),
              who, ": out must be a contiguous fp32 device tensor");
}

// conv2d_wgrad whose reduce writes the parameter's true OHWI block `out`
// (see wgrad_reduce_into_kernel). The GEMM channel counts may be the
// padded ones; out.size(0)/out.size(3) are the true ones.
void conv2d_wgrad_into(at::Tensor x, at::Tensor dy, int64_t KH, int64_t KW,
                       int64_t stride, int64_t pt, int64_t pl, bool reflect,
                       at::Tensor out, bool accumulate, bool transpose_oi) {
  check_grad_dest(out, "conv2d_wgrad_into");
  TORCH_CHECK(out.dim() == 4 && out.size(1) == KH && out.size(2) == KW,
              "conv2d_wgrad_into: out must be [O,KH,KW,I]");
  const int64_t co = out.size(transpose_oi ? 3 : 0);
  const int64_t ci = out.size(transpose_oi ? 0 : 3);
  TORCH_CHECK(co >= 1 && co <= dy.size(3) && ci >= 1 && ci <= x.size(3),
              "conv2d_wgrad_into: out channels exceed the GEMM's");
  wgrad_impl(x, dy, KH, KW, stride, pt, pl, reflect, &out, accumulate,
             transpose_oi);
}

// packed-head fold (fold_packed_dw_kernel): dwp is conv2d_wgrad's result
// for the 8-pixel-packed head, out the head weight's OHWI gradient block.
void fold_packed_dw_into(at::Tensor dwp, at::Tensor out, bool accumulate) {
  check_grad_dest(out, "fold_packed_dw_into");
  TORCH_CHECK(dwp.is_cuda() && dwp.scalar_type() == at::kFloat &&
              dwp.is_contiguous() && dwp.dim() == 4 && out.dim() == 4);
  const int64_t O = out.size(0), KH = out.size(1), KW = out.size(2),
                I = out.size(3);
  TORCH_CHECK(O >= 1 && O <= 8 && KW >= 1 && KW <= 9 && dwp.size(0) == 64 &&
                  dwp.size(1) == KH && dwp.size(2) == 2 &&
                  dwp.size(3) == 8 * I,
              "fold_packed_dw_into: shape mismatch");
  long total = out.numel();
  hipLaunchKernelGGL(fold_packed_dw_kernel, dim3(cdiv(total, 256)), dim3(256),
                     0, at::cuda::getCurrentCUDAStream(),
                     (const float*)dwp.const_data_ptr(),
                     (float*)out.mutable_data_ptr(), (int)O, (int)KH, (int)KW,
                     (int)I, accumulate ? 1 : 0);
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

// want_stats: {y, psum, psq} when stats_slabs finds the call eligible,
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
  auto p = fill_common(xq, wq, bias, y, stride, act, slope);
  p.pt = pt; p.pl = pl; p.reflect = reflect ? 1 : 0;
  p.dq = (const float*)dq.const_data_ptr();
  p.dqb = sw.has_value() ? (const float*)sw->const_data_ptr() : nullptr;
  TORCH_CHECK((long)p.B * H * W * p.Cin < (1L << 31) &&
              (long)p.Cout * p.KTOT < (1L << 31));
  std::vector<at::Tensor> out{y};
  const int ns = add_stats(p, false, true, want_stats, out);
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

}  // namespace cyg
