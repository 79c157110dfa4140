// The attention side of RFCBAMConv (models/rfa.py:78-127) and its SE block, everything but the main contraction, gfx950: activations
// T = float / __bf16, tables fp32, moments double.  All are bandwidth-trivial next to the convolutions; they exist so that the big tensors are
// read a minimal number of times and the 9x-expanded RFCBAM tensor is never written.
//
//   ly_colsum                  spatial sum per (image, channel, slice)                        (SE gap, models/rfa.py:90)
//   ly_se_fwd                  ly_colsum + sigmoid(Wb relu(Wa mean))                          (models/rfa.py:78-92)
//   ly_se_bwd                  the same under autograd; dgap for ly_rf_bwd_dx                 (models/rfa.py:88-92)
//   ly_rfcbam_stats (+ _describe)  max_c / mean_c of relu(bn(generate(x))) on the expanded grid, k = 1 with the SE partials   (models/rfa.py:115-126)
//   ly_rfa_map                 sigmoid(conv3x3([max, mean]))                                  (models/rfa.py:107,127)
//   ly_rfcbam_mid              the SE step and ly_rfa_map as one launch (they share ly_se_mlp_body / ly_se_lds_floats with ly_se_fwd)
//   ly_rfcbam_tap_moments (+ _describe)  train mode, k = 3: the 9 + 45 tap moments per channel behind generate's BatchNorm statistics
//   ly_rfcbam_gen_prepare      train mode: moments -> generate's BatchNorm coefficients, running stats and folded weights   (models/rfa.py:101-106)
#include <float.h>

#include "ly_tile.hpp"
#include "ly_params.h"
// ---------------------------------------------------------------------------------------------------
// SE: partial spatial sums then the two tiny linears
// ---------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_colsum_kernel(const T* __restrict__ x, int ldx, int P, int C, int slices,
                                                                float* __restrict__ part) {
  __shared__ f32x4 red[LY_THREADS];
  const int n = blockIdx.x / slices, sl = blockIdx.x - n * slices;
  const int nc4 = C >> 2, tid = threadIdx.x;
  const int per = (P + slices - 1) / slices;
  const int j_lo = sl * per, j_hi = (j_lo + per) < P ? (j_lo + per) : P;
  const int groups = LY_THREADS / nc4;              // C <= 1024
  const int c4 = tid % nc4, j0 = tid / nc4;
  f32x4 s = ly_zero4();
  if (j0 < groups) {
#pragma unroll 4
    for (int j = j_lo + j0; j < j_hi; j += groups) s += ly_ld4<T>(x + ((long)n * P + j) * ldx + 4 * c4);
  }
  red[tid] = s;
  __syncthreads();
  if (j0 == 0) {
    for (int g = 1; g < groups; ++g) s += red[g * nc4 + c4];
    ly_stg4(part + ((long)n * slices + sl) * C + 4 * c4, s);
  }
}

// LDS floats of the SE step: g[C] + hid[R] + red[LY_THREADS][4], plus — when they fit 48 KiB — both weight matrices (2 R C): staged while the
// pooling partials are on their way, so that the step is ONE global round trip instead of three dependent ones (partials, fc1 rows, fc2 rows:
// 12.6 us per launch of ly_rfcbam_mid was this chain, not the get_weight map that runs beside it)
__host__ __device__ __forceinline__ size_t ly_se_lds_floats(int C, int R) {
  const size_t base = (size_t)((C + R + 3) & ~3) + 4 * LY_THREADS;
  const size_t w = 2 * (size_t)R * C;
  return (C & 3) == 0 && w * 4 <= 48 * 1024 ? base + w : base;
}

__device__ __forceinline__ void ly_se_mlp_body(float* sm, const int n, const float* __restrict__ part, int slices, int C, float inv_hw,
                                               const float* __restrict__ wa, const float* __restrict__ wb, int R, float* __restrict__ ca) {
  float* g = sm;                     // g[C] + hid[R] + red[LY_THREADS][4] (+ wa[R][C] + wb[C][R])
  float* hid = sm + C;
  f32x4* red = reinterpret_cast<f32x4*>(sm + ((C + R + 3) & ~3));
  const size_t base = (size_t)((C + R + 3) & ~3) + 4 * LY_THREADS;
  const bool staged = ly_se_lds_floats(C, R) > base;
  float* was = sm + base;
  float* wbs = was + (size_t)R * C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // slice partials -> channel means.  All 256 threads load: thread = (slice group, 4 channels), so the up to 128 slices
  // are a handful of independent float4 loads per thread instead of a 128-long chain per channel; groups meet in LDS.
  const int nq = C >> 2;                 // channel quads: C % 4 == 0 and C <= 1024, so nq <= 256
  const int ng = LY_THREADS / nq;        // slice groups
  const int q = tid % nq, sg = tid / nq;
  f32x4 s4 = ly_zero4();
  if (sg < ng) {
    int sl = sg;
    for (; sl + 3 * ng < slices; sl += 4 * ng) {         // four loads in flight per trip
      const f32x4 a0 = ly_ldg4(part + ((long)n * slices + sl) * C + 4 * q), a1 = ly_ldg4(part + ((long)n * slices + sl + ng) * C + 4 * q);
      const f32x4 a2 = ly_ldg4(part + ((long)n * slices + sl + 2 * ng) * C + 4 * q), a3 = ly_ldg4(part + ((long)n * slices + sl + 3 * ng) * C + 4 * q);
      s4 += a0; s4 += a1; s4 += a2; s4 += a3;
    }
    for (; sl < slices; sl += ng) s4 += ly_ldg4(part + ((long)n * slices + sl) * C + 4 * q);
  }
  if (staged) {
    const int nw4 = (R * C) >> 2;                        // float4 items per matrix (C % 4 == 0)
    for (int i = tid; i < nw4; i += 4 * LY_THREADS) {
      f32x4 va[4], vb[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int j = i + k * LY_THREADS < nw4 ? i + k * LY_THREADS : i;
        va[k] = ly_ldg4(wa + 4 * j);
        vb[k] = ly_ldg4(wb + 4 * j);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (i + k * LY_THREADS < nw4) {
          *reinterpret_cast<f32x4*>(was + 4 * (i + k * LY_THREADS)) = va[k];
          *reinterpret_cast<f32x4*>(wbs + 4 * (i + k * LY_THREADS)) = vb[k];
        }
    }
  }
  red[tid] = s4;
  __syncthreads();
  if (sg == 0) {
    for (int k = 1; k < ng; ++k) s4 += red[tid + k * nq];
    g[4 * q] = s4[0] * inv_hw; g[4 * q + 1] = s4[1] * inv_hw; g[4 * q + 2] = s4[2] * inv_hw; g[4 * q + 3] = s4[3] * inv_hw;
  }
  __syncthreads();
  const float* wap = staged ? was : wa;
  const float* wbp = staged ? wbs : wb;
  for (int r = wave; r < R; r += 4) {
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += wap[r * C + c] * g[c];
    s = ly_group_sum(s, 64);
    if (lane == 0) hid[r] = fmaxf(s, 0.f);
  }
  __syncthreads();
  for (int c = tid; c < C; c += LY_THREADS) {
    float s = 0.f;
    for (int r = 0; r < R; ++r) s += wbp[c * R + r] * hid[r];
    ca[(long)n * C + c] = ly_sigmoid(s);
  }
}

__global__ __launch_bounds__(LY_THREADS) void ly_se_mlp_kernel(const float* __restrict__ part, int slices, int C, float inv_hw,
                                                                const float* __restrict__ wa, const float* __restrict__ wb, int R,
                                                                float* __restrict__ ca) {
  extern __shared__ float sm[];
  ly_se_mlp_body(sm, blockIdx.x, part, slices, C, inv_hw, wa, wb, R, ca);
}

// SE pooling partials alone: part[n][slice][C] = sum of x over the slice's pixels (for ly_rfcbam_mid)
extern "C" int ly_colsum(const void* x, int ldx, int n_img, int HW, int C, float* part, int slices, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "colsum");
  LY_CHECK(x && part && (C & 3) == 0 && (ldx & 3) == 0 && C <= 1024 && slices > 0, "colsum: bad arguments");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LY_WITH_T(dtype, hipLaunchKernelGGL(ly_colsum_kernel<T>, dim3(n_img * slices), dim3(LY_THREADS), 0, st, reinterpret_cast<const T*>(x), ldx, HW, C, slices, part));
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_se_fwd(const void* x, int ldx, int n_img, int HW, int C, const float* wa, const float* wb, int R, float* part,
                         int slices, float* ca, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "se");
  LY_CHECK(x && wa && wb && part && ca, "se: null pointer");
  LY_CHECK((C & 3) == 0 && (ldx & 3) == 0 && C <= 1024 && slices > 0 && R > 0 && R <= 256, "se: bad arguments");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LY_WITH_T(dtype, hipLaunchKernelGGL(ly_colsum_kernel<T>, dim3(n_img * slices), dim3(LY_THREADS), 0, st, reinterpret_cast<const T*>(x), ldx, HW, C, slices, part));
  LY_LAUNCH_CHECK();
  hipLaunchKernelGGL(ly_se_mlp_kernel, dim3(n_img), dim3(LY_THREADS), sizeof(float) * ly_se_lds_floats(C, R), st, part, slices, C, 1.f / (float)HW,
                     wa, wb, R, ca);
  LY_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------
// RFCBAM statistics, k = 1:  g = relu(x*a + b);  mm[pix] = (max_c g, mean_c g).  One wave per pixel.
// ---------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_rfcbam_stats1_kernel(const T* __restrict__ x, int ldx, long M, int C,
                                                                       const float* __restrict__ a, const float* __restrict__ b,
                                                                       float* __restrict__ mm) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * 4;
  const int nc4 = C >> 2;
  const float inv = 1.f / (float)C;
  for (long p = wave; p < M; p += nwaves) {
    float mx = -FLT_MAX, sm = 0.f;
    for (int c4 = lane; c4 < nc4; c4 += 64) {
      const f32x4 v = ly_ld4<T>(x + p * ldx + 4 * c4), s = ly_ldg4(a + 4 * c4), t = ly_ldg4(b + 4 * c4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float g = fmaxf(v[r] * s[r] + t[r], 0.f);
        mx = fmaxf(mx, g);
        sm += g;
      }
    }
    mx = ly_group_max(mx, 64);                              // (in-row steps as DPP moves: ly_common.hpp)
    sm = ly_group_sum(sm, 64);
    if (lane == 0) {
      mm[2 * p] = mx;
      mm[2 * p + 1] = sm * inv;
    }
  }
}

// k = 1 statistics AND the SE pooling in one pass over x: block = (image, slice of its pixels), wave = one pixel at a time, lane =
// channel quads lane, lane + 64, ...  The per-pixel [max, mean] needs a wave reduction (as above); the per-channel sums of the SE
// global average pool stay in the lanes' registers over the block's pixels and leave as one partial row per block (no atomics,
// no zero fill): part[n][slice][C], summed by the SE step (ly_rfcbam_mid / ly_se_mlp).
#define LY_PRE1_NS 3                 // channel-quad slots per lane: C <= 768
template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_rfcbam_pre1_kernel(const T* __restrict__ x, int ldx, int HW, int C, int slices,
                                                                    const float* __restrict__ a, const float* __restrict__ b,
                                                                    float* __restrict__ mm, float* __restrict__ part) {
  __shared__ f32x4 red[3][LY_PRE1_NS * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x / slices, sl = blockIdx.x - n * slices;
  const int per = (HW + slices - 1) / slices;
  const int j_lo = sl * per, j_hi = (j_lo + per) < HW ? (j_lo + per) : HW;
  const int nc4 = C >> 2;
  const float inv = 1.f / (float)C;
  f32x4 sa[LY_PRE1_NS], sb[LY_PRE1_NS], gs[LY_PRE1_NS];
#pragma unroll
  for (int q = 0; q < LY_PRE1_NS; ++q) {
    const int c4 = lane + 64 * q;
    const bool ok = c4 < nc4;
    sa[q] = ok ? ly_ldg4(a + 4 * c4) : ly_zero4();
    sb[q] = ok ? ly_ldg4(b + 4 * c4) : ly_zero4();
    gs[q] = ly_zero4();
  }
  for (int j = j_lo + wave; j < j_hi; j += 4) {
    const long p = (long)n * HW + j;
    float mx = 0.f, sm = 0.f;                  // relu(.) >= 0: zero is the identity of the channel max (absent lanes contribute 0)
#pragma unroll
    for (int q = 0; q < LY_PRE1_NS; ++q) {
      const int c4 = lane + 64 * q;
      if (c4 < nc4) {
        const f32x4 v = ly_ld4<T>(x + p * ldx + 4 * c4);
        gs[q] += v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float g = fmaxf(v[r] * sa[q][r] + sb[q][r], 0.f);
          mx = fmaxf(mx, g);
          sm += g;
        }
      }
    }
    mx = ly_group_max(mx, 64);                              // (in-row steps as DPP moves: ly_common.hpp)
    sm = ly_group_sum(sm, 64);
    if (lane == 0) {
      mm[2 * p] = mx;
      mm[2 * p + 1] = sm * inv;
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int q = 0; q < LY_PRE1_NS; ++q) red[wave - 1][q * 64 + lane] = gs[q];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int q = 0; q < LY_PRE1_NS; ++q) {
      const int c4 = lane + 64 * q;
      if (c4 < nc4) ly_stg4(part + ((long)n * slices + sl) * C + 4 * c4, gs[q] + red[0][q * 64 + lane] + red[1][q * 64 + lane] + red[2][q * 64 + lane]);
    }
  }
}

// The same pass with SEVERAL pixels per wave (round 6).  Above, a wave takes one pixel per trip: one 8-byte load per lane in flight and two
// 64-lane reductions per pixel (two of their six steps go through the LDS pipe) — a chain of dependent latencies per pixel, 16-24 us per launch
// where the bytes need 5-10.  Here LPP = 4 .. 16 lanes share a pixel (64 / LPP pixels per wave and trip), a lane holds VPL 16-byte vectors of
// its pixel — all loads of a trip issued together — and the per-pixel [max, mean] is a reduction over LPP <= 16 lanes: DPP moves only.  The SE
// pooling sums stay per lane over the block's pixels and meet once, in LDS.
template <typename T, int VPL>                  // 16-byte vectors per lane: C / VW <= 16 * VPL (vector ln + 16 v of the pixel; absent ones are masked)
__global__ __launch_bounds__(LY_THREADS) void ly_rfcbam_pre1v_kernel(const T* __restrict__ x, int ldx, int HW, int C, int slices,
                                                                     const float* __restrict__ a, const float* __restrict__ b,
                                                                     float* __restrict__ mm, float* __restrict__ part) {
  constexpr int LPP = 16, VW = LyT<T>::VW, NQ = VW / 4, PPW = 64 / LPP, NPG = 4 * PPW;        // pixels per wave and trip, pixel groups per block
  const int nv = C / VW;
  using RV = typename LyT<T>::RV;
  extern __shared__ f32x4 pre1v_sm[];                  // [NPG][C / 4]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ln = lane % LPP, pg = wave * PPW + lane / LPP;
  const int n = blockIdx.x / slices, sl = blockIdx.x - n * slices;
  const int per = (HW + slices - 1) / slices;
  const int j_lo = sl * per, j_hi = (j_lo + per) < HW ? (j_lo + per) : HW;
  const float inv = 1.f / (float)C;
  f32x4 sa[VPL][NQ], sb[VPL][NQ], gs[VPL][NQ];
#pragma unroll
  for (int v = 0; v < VPL; ++v)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const bool ok = ln + LPP * v < nv;
      const int c = ok ? VW * (ln + LPP * v) + 4 * q : 0;
      sa[v][q] = ok ? ly_ldg4(a + c) : ly_zero4(); sb[v][q] = ok ? ly_ldg4(b + c) : ly_zero4(); gs[v][q] = ly_zero4();      // absent vectors: relu(0 * x + 0) = 0
    }
  for (int j0 = j_lo; j0 < j_hi; j0 += NPG) {
    const int j = j0 + pg;
    const bool live = j < j_hi;
    const long p = (long)n * HW + (live ? j : j_hi - 1);
    RV xv[VPL];
#pragma unroll
    for (int v = 0; v < VPL; ++v) xv[v] = ly_ldrv<T>(x + p * ldx + (ln + LPP * v < nv ? VW * (ln + LPP * v) : 0));      // (clamped: straight-line loads)
    float mx = 0.f, sm = 0.f;                  // relu(.) >= 0: zero is the identity of the channel max
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      f32x4 xq[NQ];
      ly_rv_unpack(xv[v], xq);
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (live) gs[v][q] += xq[q];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float g = fmaxf(xq[q][r] * sa[v][q][r] + sb[v][q][r], 0.f);
          mx = fmaxf(mx, g);
          sm += g;
        }
      }
    }
    mx = ly_group_max(mx, LPP);
    sm = ly_group_sum(sm, LPP);
    if (ln == 0 && live) *reinterpret_cast<f32x2*>(mm + 2 * p) = (f32x2){mx, sm * inv};
  }
  const int nc4 = C >> 2;
#pragma unroll
  for (int v = 0; v < VPL; ++v)
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (ln + LPP * v < nv) pre1v_sm[pg * nc4 + (VW * (ln + LPP * v) >> 2) + q] = gs[v][q];
  __syncthreads();
  for (int c4 = threadIdx.x; c4 < nc4; c4 += LY_THREADS) {
    f32x4 t = pre1v_sm[c4];
    for (int g = 1; g < NPG; ++g) t += pre1v_sm[g * nc4 + c4];
    ly_stg4(part + ((long)n * slices + sl) * C + 4 * c4, t);
  }
}

template <typename T>
static int pre1v_launch(const T* x, int ldx, int n_img, int HW, int C, int slices, const float* a1, const float* b1, float* mm, float* part, const LyOut& out) {
  constexpr int VW = LyT<T>::VW;
  if (C % VW || ldx % VW) return 1;                             // 1: not this kernel's shape
  const int nv = C / VW, vpl = (nv + 15) / 16;
  const size_t lds = (size_t)16 * C * sizeof(float);            // 16 pixel groups per block
#define LY_PV(V_)                                                                                                                                                  \
  case V_:                                                                                                                                                         \
    return LY_EMIT(out, (ly_launch<ly_rfcbam_pre1v_kernel<T, V_>>(dim3((unsigned)(n_img * slices)), dim3(LY_THREADS), lds, out.st, x, ldx, HW, C, slices, a1, b1, mm, part)), \
                   "ly_rfcbam_pre1v_kernel<%s, " #V_ ">", ly_tname<T>())
  switch (vpl) { LY_PV(1); LY_PV(2); LY_PV(3); LY_PV(4); default: break; }
#undef LY_PV
  return 1;
}

// ---------------------------------------------------------------------------------------------------
// RFCBAM statistics, k = 3 (stride s, pad 1).  lane = output pixel of a TH x TW tile, the 4 waves
// split the channels (channel c0 + wave + 4j of each 32-channel chunk); depthwise weights are wave-
// uniform scalar loads from wq[C32/32][4 waves][9 t][8 j][10] = 9 folded weights W'[t][u] + folded
// bias b'[t] per (t, channel), zero padded to a multiple of 32 channels (pack.rfcbam_stats_weights).
// ---------------------------------------------------------------------------------------------------
#define LY_SCC 32
#define LY_ST3_NV 10              // float4 staging items per thread per chunk: IH*IW*8 <= 10*256
#define LY_ST3_WF (9 * 4 * 20)    // floats of folded weights per wave per chunk: [9 t][4 channel pairs][9 x (w_a, w_b) + (b_a, b_b)]
template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_rfcbam_stats3_kernel(const T* __restrict__ x, int ldx, int H, int W, int C,
                                                                       int Ho, int Wo, int s, int TH, int TW, int nct, int nrt,
                                                                       const float* __restrict__ wg, float* __restrict__ mm, float* __restrict__ part) {
  extern __shared__ float lds[];
  const int IH = s * (TH - 1) + 3, IW = s * (TW - 1) + 3;
  float* wsm = lds;                                  // [4 waves][LY_ST3_WF]: this chunk's folded weights (16-B aligned)
  float* xs = lds + 4 * LY_ST3_WF;                   // [IH*IW][LY_SCC + 1]
  float* red = xs + IH * IW * (LY_SCC + 1);          // [4][18][64]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int b = blockIdx.x;
  const int ct = b % nct; b /= nct;
  const int rt = b % nrt;
  const int n = b / nrt;
  const int oy0 = rt * TH, ox0 = ct * TW;
  const int ly = lane / TW, lx = lane - ly * TW;
  const int oy = oy0 + ly, ox = ox0 + lx;
  const bool active = ly < TH && oy < Ho && ox < Wo;
  const int iy0 = s * oy0 - 1, ix0 = s * ox0 - 1;

  // staging plan of this thread (independent of the channel chunk): global element offset (or -1) and LDS slot
  const int items = IH * IW * (LY_SCC / 4);
  long soff[LY_ST3_NV];
  int doff[LY_ST3_NV];
#pragma unroll
  for (int e = 0; e < LY_ST3_NV; ++e) {
    const int idx = tid + e * LY_THREADS;
    long so = -1;
    int dd = -1;
    if (idx < items) {
      const int ip = idx >> 3, c4 = idx & 7;
      const int r = ip / IW, q = ip - r * IW;
      const int iy = iy0 + r, ix = ix0 + q;
      dd = ip * (LY_SCC + 1) + 4 * c4;
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) so = (((long)n * H + iy) * W + ix) * ldx + 4 * c4;
    }
    soff[e] = so; doff[e] = dd;
  }
  // x addresses of the 9 taps of this lane's pixel (LDS float index, channel 0)
  int xa[9];
#pragma unroll
  for (int u = 0; u < 9; ++u) xa[u] = ((s * ly + u / 3) * IW + (s * lx + u % 3)) * (LY_SCC + 1);

  float mx[9], sm[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) { mx[t] = 0.f; sm[t] = 0.f; }      // G = relu(.) >= 0, so 0 is the identity of the channel max

  // the input tile (pv) and the folded weights (wv) of chunk c+1 are requested before chunk c is regenerated: no load is waited
  // for right after it is issued
  typename LyT<T>::R4 pv[LY_ST3_NV];
  auto prefetch = [&](int c0) {
#pragma unroll
    for (int e = 0; e < LY_ST3_NV; ++e) {
      const bool ok = soff[e] >= 0 && c0 + 4 * ((tid + e * LY_THREADS) & 7) < C;
      pv[e] = ly_ldr4<T>(ok ? x + soff[e] + c0 : x);
    }
  };
  constexpr int WV = (4 * LY_ST3_WF / 4 + LY_THREADS - 1) / LY_THREADS;
  f32x4 wv[WV];
  auto wprefetch = [&](int chunk) {
    const float* wsrc = wg + (long)chunk * (4 * LY_ST3_WF);
#pragma unroll
    for (int e = 0; e < WV; ++e) {
      const int i = tid + e * LY_THREADS;
      wv[e] = ly_ldg4(wsrc + 4 * (i < 4 * LY_ST3_WF / 4 ? i : 0));
    }
  };
  wprefetch(0);
  prefetch(0);

  for (int c0 = 0; c0 < C; c0 += LY_SCC) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < WV; ++e) {
      const int i = tid + e * LY_THREADS;
      if (i < 4 * LY_ST3_WF / 4) reinterpret_cast<f32x4*>(wsm)[i] = wv[e];
    }
    const bool more = c0 + LY_SCC < C;
    wprefetch(more ? c0 / LY_SCC + 1 : 0);
#pragma unroll
    for (int e = 0; e < LY_ST3_NV; ++e) {
      if (doff[e] >= 0) {
        const bool ok = soff[e] >= 0 && c0 + 4 * ((tid + e * LY_THREADS) & 7) < C;
        const f32x4 pf = ly_r4_f32(pv[e]);
        float* d = xs + doff[e];
        d[0] = ok ? pf[0] : 0.f; d[1] = ok ? pf[1] : 0.f; d[2] = ok ? pf[2] : 0.f; d[3] = ok ? pf[3] : 0.f;
      }
    }
    prefetch(more ? c0 + LY_SCC : 0);      // unconditional: a load under a run-time branch makes every later wait conservative
    __syncthreads();
    if (part) {
      // SE global-average-pool partial of this tile (models/rfa.py:90) from the staged chunk: the block OWNS input rows
      // [s*oy0, s*(oy0+TH)) x cols [s*ox0, s*(ox0+TW)) (every input pixel belongs to exactly one tile), thread = (channel, 1 of 8
      // pixel stripes); the stripes meet in LDS (red is free until the end) and leave as one row of part[n][tile][C]
      const int ch = tid & 31, stripe = tid >> 5;
      const int rows_own = min(s * TH, H - s * oy0), cols_own = min(s * TW, W - s * ox0);
      float acc = 0.f;
      for (int q = stripe; q < rows_own * cols_own; q += 8) {
        const int r = q / cols_own, cq = q - r * cols_own;
        acc += xs[((r + 1) * IW + cq + 1) * (LY_SCC + 1) + ch];
      }
      red[stripe * 32 + ch] = acc;
      __syncthreads();
      if (tid < 32 && c0 + tid < C) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) t += red[g * 32 + tid];
        part[((long)n * (nrt * nct) + rt * nct + ct) * C + c0 + tid] = t;
      }
      __syncthreads();
    }
    {
      // inputs of this wave's 8 channels (c0 + wave + 4j) as 4 packed pairs (j = 2p, 2p+1), then the folded
      // weights [t][p][9 x (w_a, w_b), (b_a, b_b)] read as wave-uniform LDS broadcasts: v_pk_fma_f32 does two
      // channels per instruction; two pairs at a time so that two independent accumulation chains interleave.
      f32x2 xv[4][9];
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int u = 0; u < 9; ++u) {
          const float a = xs[xa[u] + wave + 8 * p], c = xs[xa[u] + wave + 8 * p + 4];
          xv[p][u] = active ? (f32x2){a, c} : (f32x2){0.f, 0.f};
        }
      const f32x4* wq = reinterpret_cast<const f32x4*>(wsm + wave * LY_ST3_WF);
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {
          f32x4 q0[5], q1[5];
#pragma unroll
          for (int i = 0; i < 5; ++i) {
            q0[i] = wq[(t * 4 + 2 * ph) * 5 + i];
            q1[i] = wq[(t * 4 + 2 * ph + 1) * 5 + i];
          }
          f32x2 a0 = {q0[4][2], q0[4][3]}, a1 = {q1[4][2], q1[4][3]};
#pragma unroll
          for (int u = 0; u < 9; ++u) {
            a0 += xv[2 * ph][u] * (f32x2){q0[u >> 1][2 * (u & 1)], q0[u >> 1][2 * (u & 1) + 1]};
            a1 += xv[2 * ph + 1][u] * (f32x2){q1[u >> 1][2 * (u & 1)], q1[u >> 1][2 * (u & 1) + 1]};
          }
          const float g0 = fmaxf(a0[0], 0.f), g1 = fmaxf(a0[1], 0.f), g2 = fmaxf(a1[0], 0.f), g3 = fmaxf(a1[1], 0.f);
          mx[t] = fmaxf(fmaxf(mx[t], fmaxf(g0, g1)), fmaxf(g2, g3));
          sm[t] += (g0 + g1) + (g2 + g3);
        }
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    red[(wave * 18 + t) * 64 + lane] = mx[t];
    red[(wave * 18 + 9 + t) * 64 + lane] = sm[t];
  }
  __syncthreads();
  if (wave == 0 && active) {
    const float inv = 1.f / (float)C;
    const int HK = 3 * Ho, WK = 3 * Wo;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      float m = red[t * 64 + lane], a = red[(9 + t) * 64 + lane];
      for (int w2 = 1; w2 < 4; ++w2) {
        m = fmaxf(m, red[(w2 * 18 + t) * 64 + lane]);
        a += red[(w2 * 18 + 9 + t) * 64 + lane];
      }
      const long o = (((long)n * HK + 3 * oy + t / 3) * WK + 3 * ox + t % 3) * 2;
      mm[o] = m;
      mm[o + 1] = a * inv;
    }
  }
}

static int rfcbam_stats_entry(const void* x, int ldx, int n_img, int H, int W, int C, int k, int s, const float* wg, const float* a1, const float* b1, int TH,
                              int TW, float* mm, float* part, int slices, int dtype, const LyOut& out) {
  LY_CHECK_DTYPE(dtype, "rfcbam_stats");
  LY_CHECK(x && mm && (C & 3) == 0 && (ldx & 3) == 0, "rfcbam_stats: bad arguments");
  if (k == 1) {
    LY_CHECK(s == 1 && a1 && b1, "rfcbam_stats: k=1 needs stride 1 and folded scale/shift");
    long M = (long)n_img * H * W;
    if (part) {           // statistics + SE pooling partials in one pass
      LY_CHECK(slices > 0 && C <= 256 * LY_PRE1_NS, "rfcbam_stats: fused SE pooling needs slices > 0 and C <= %d", 256 * LY_PRE1_NS);
      int rc = 1;
      LY_WITH_T(dtype, rc = pre1v_launch<T>(reinterpret_cast<const T*>(x), ldx, n_img, H * W, C, slices, a1, b1, mm, part, out));      // several pixels per wave
      if (rc != 1) return rc;
      LY_WITH_T(dtype, return LY_EMIT(out, (ly_launch<ly_rfcbam_pre1_kernel<T>>(dim3((unsigned)(n_img * slices)), dim3(LY_THREADS), 0, out.st, reinterpret_cast<const T*>(x),
                                                                                ldx, H * W, C, slices, a1, b1, mm, part)),
                                      "ly_rfcbam_pre1_kernel<%s>", ly_tname<T>()));
    }
    long blocks = (M + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;
    LY_WITH_T(dtype, return LY_EMIT(out, (ly_launch<ly_rfcbam_stats1_kernel<T>>(dim3((unsigned)blocks), dim3(LY_THREADS), 0, out.st, reinterpret_cast<const T*>(x), ldx, M, C,
                                                                                a1, b1, mm)),
                                    "ly_rfcbam_stats1_kernel<%s>", ly_tname<T>()));
  }
  LY_CHECK(k == 3 && s >= 1 && wg, "rfcbam_stats: only k in {1,3} is built");
  LY_CHECK(TW >= 1 && TH >= 1 && TH * TW <= 64, "rfcbam_stats: tile %dx%d does not fit a wave", TH, TW);
  const int Ho = (H + 2 - 3) / s + 1, Wo = (W + 2 - 3) / s + 1;
  const int nct = (Wo + TW - 1) / TW, nrt = (Ho + TH - 1) / TH;
  LY_CHECK(!part || slices == nct * nrt, "rfcbam_stats: k=3 fused SE pooling writes one partial row per tile: slices must be %d", nct * nrt);
  // the pooling reads the inputs a tile OWNS, s*TH x s*TW of them, out of the staged tile of s*(TH-1)+3 x s*(TW-1)+3: held for s <= 2 only
  LY_CHECK(!part || s <= 2, "rfcbam_stats: k=3 fused SE pooling is built for stride 1 and 2 (stride %d: take the partials with ly_colsum)", s);
  const int IH = s * (TH - 1) + 3, IW = s * (TW - 1) + 3;
  size_t lds = sizeof(float) * ((size_t)4 * LY_ST3_WF + (size_t)IH * IW * (LY_SCC + 1) + 4 * 18 * 64);
  LY_CHECK(IH * IW * (LY_SCC / 4) <= LY_ST3_NV * LY_THREADS, "rfcbam_stats: input tile %dx%d exceeds the staging capacity", IH, IW);
  LY_CHECK(lds <= LY_LDS_MAX, "rfcbam_stats: tile needs %zu B LDS", lds);
  LY_WITH_T(dtype, return LY_EMIT(out, (ly_launch_lds<ly_rfcbam_stats3_kernel<T>>(dim3(n_img * nrt * nct), dim3(LY_THREADS), lds, out.st, reinterpret_cast<const T*>(x), ldx,
                                                                                  H, W, C, Ho, Wo, s, TH, TW, nct, nrt, wg, mm, part)),
                                  "ly_rfcbam_stats3_kernel<%s>", ly_tname<T>()));
}

extern "C" int ly_rfcbam_stats(const void* x, int ldx, int n_img, int H, int W, int C, int k, int s, const float* wg,
                               const float* a1, const float* b1, int TH, int TW, float* mm, float* part, int slices, int dtype, void* stream) {
  return rfcbam_stats_entry(x, ldx, n_img, H, W, C, k, s, wg, a1, b1, TH, TW, mm, part, slices, dtype, LY_ON_STREAM(stream));
}

// the arguments of ly_rfcbam_stats with (name, cap) for the stream
extern "C" int ly_rfcbam_stats_describe(const void* x, int ldx, int n_img, int H, int W, int C, int k, int s, const float* wg, const float* a1, const float* b1, int TH,
                                        int TW, float* mm, float* part, int slices, int dtype, char* name, int cap) {
  LY_CHECK(name && cap > 0, "rfcbam_stats_describe: bad arguments");
  return rfcbam_stats_entry(x, ldx, n_img, H, W, C, k, s, wg, a1, b1, TH, TW, mm, part, slices, dtype, LyOut{nullptr, name, cap});
}

// rfa[n, y, x] = sigmoid( sum_{ch, dy, dx} w[ch][dy][dx] * mm[n, y+dy-1, x+dx-1, ch] )
// A thread owns FOUR horizontally adjacent outputs: 3 rows x 6 columns of [max, mean] pairs = 18 eight-byte loads (clamped addresses, all
// issued before the first use) for 72 multiply-adds — one output per thread was 18 guarded loads for 18 (12.6 us per launch at 120 x 120 x 64,
// all of it L2 round trips).  Items: i -> (n, y, x0 = 4 * (i % ceil(WK / 4))).
__device__ __forceinline__ void ly_rfa_map_body(const long i, const float* __restrict__ mm, int HK, int WK, long total4,
                                                const float* __restrict__ w, float* __restrict__ rfa) {
  if (i >= total4) return;
  const int wq = (WK + 3) >> 2;
  const int x0 = 4 * (int)(i % wq);
  const int yk = (int)((i / wq) % HK);
  const long n = i / ((long)wq * HK);
  f32x2 v[3][6];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int yy = yk + dy - 1;
    const int yc = yy < 0 ? 0 : (yy >= HK ? HK - 1 : yy);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const int xx = x0 + c - 1;
      const int xc = xx < 0 ? 0 : (xx >= WK ? WK - 1 : xx);
      v[dy][c] = *reinterpret_cast<const f32x2*>(mm + ((n * HK + yc) * WK + xc) * 2);
    }
  }
  float wv[18];
#pragma unroll
  for (int k = 0; k < 18; ++k) wv[k] = w[k];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int yy = yk + dy - 1;
    const bool yok = yy >= 0 && yy < HK;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const int xx = x0 + c - 1;
      const bool ok = yok && xx >= 0 && xx < WK;
      const f32x2 p = ok ? v[dy][c] : (f32x2){0.f, 0.f};
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int dx = c - o;                            // output x0 + o reads column x0 + o + dx - 1 = x0 + c - 1
        if (dx >= 0 && dx < 3) s[o] += wv[dy * 3 + dx] * p[0] + wv[9 + dy * 3 + dx] * p[1];
      }
    }
  }
  float* out = rfa + (n * HK + yk) * WK + x0;
  if (x0 + 3 < WK && (WK & 3) == 0) {
    *reinterpret_cast<f32x4*>(out) = (f32x4){ly_sigmoid(s[0]), ly_sigmoid(s[1]), ly_sigmoid(s[2]), ly_sigmoid(s[3])};
  } else {
#pragma unroll
    for (int o = 0; o < 4; ++o)
      if (x0 + o < WK) out[o] = ly_sigmoid(s[o]);
  }
}

__global__ __launch_bounds__(LY_THREADS) void ly_rfa_map_kernel(const float* __restrict__ mm, int HK, int WK, long total4,
                                                                 const float* __restrict__ w, float* __restrict__ rfa) {
  ly_rfa_map_body((long)blockIdx.x * LY_THREADS + threadIdx.x, mm, HK, WK, total4, w, rfa);
}

// The two small dependent steps between the statistics pass and the main contraction of RFCBAMConv as ONE launch: blocks
// [0, n_img) finish SE (slice partials -> mean -> fc -> sigmoid, models/rfa.py:88-92), the remaining blocks evaluate
// get_weight (3x3 conv on the [max, mean] map + sigmoid, models/rfa.py:107,127).  They are independent of each other.
__global__ __launch_bounds__(LY_THREADS) void ly_rfcbam_mid_kernel(const float* __restrict__ part, int slices, int C, float inv_hw,
                                                                   const float* __restrict__ wa, const float* __restrict__ wb, int R,
                                                                   float* __restrict__ ca, int n_img, const float* __restrict__ mm, int HK, int WK,
                                                                   long total4, const float* __restrict__ w18, float* __restrict__ rfa) {
  extern __shared__ float sm[];
  if ((int)blockIdx.x < n_img) ly_se_mlp_body(sm, blockIdx.x, part, slices, C, inv_hw, wa, wb, R, ca);
  else ly_rfa_map_body((long)(blockIdx.x - n_img) * LY_THREADS + threadIdx.x, mm, HK, WK, total4, w18, rfa);
}

extern "C" int ly_rfcbam_mid(const float* part, int slices, int C, int HW, const float* wa, const float* wb, int R, float* ca, int n_img,
                             const float* mm, int HK, int WK, const float* w18, float* rfa, void* stream) {
  LY_CHECK(part && wa && wb && ca && mm && w18 && rfa, "rfcbam_mid: null pointer");
  LY_CHECK((C & 3) == 0 && C <= 1024 && slices > 0 && R > 0 && R <= 256 && n_img > 0, "rfcbam_mid: bad arguments");
  const long total4 = (long)n_img * HK * ((WK + 3) / 4);
  const unsigned blocks = (unsigned)(n_img + (total4 + LY_THREADS - 1) / LY_THREADS);
  hipLaunchKernelGGL(ly_rfcbam_mid_kernel, dim3(blocks), dim3(LY_THREADS), sizeof(float) * ly_se_lds_floats(C, R),
                     reinterpret_cast<hipStream_t>(stream), part, slices, C, 1.f / (float)HW, wa, wb, R, ca, n_img, mm, HK, WK, total4, w18, rfa);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_rfa_map(const float* mm, int n_img, int HK, int WK, const float* w, float* rfa, void* stream) {
  LY_CHECK(mm && w && rfa, "rfa_map: null pointer");
  const long total4 = (long)n_img * HK * ((WK + 3) / 4);
  hipLaunchKernelGGL(ly_rfa_map_kernel, dim3((unsigned)((total4 + LY_THREADS - 1) / LY_THREADS)), dim3(LY_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), mm, HK, WK, total4, w, rfa);
  LY_LAUNCH_CHECK();
  return 0;
}

// RFCBAMConv k=3 `generate` BatchNorm statistics (train mode).  The pre-BN value of channel c, tap-output t at
// an output pixel is a_t = sum_u w[c,t,u] * x_u with x_u the 9 (zero padded, stride s) input taps of that pixel,
// so  sum a_t = w_t . m   and   sum a_t^2 = w_t^T M w_t  with  m[u] = sum_pixels x_u,  M[u][v] = sum_pixels x_u x_v.
// This kernel accumulates the 9 + 45 moments per channel: thread = channel (coalesced NHWC reads), blocks split
// the output pixels, 54 vectorised atomics per thread at the end.  mom layout: [54][C].
template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_rfcbam_tap_moments_kernel(const T* __restrict__ x, int ldx, int n_img, int H, int W,
                                                                            int C, int Ho, int Wo, int s, double* __restrict__ mom) {
  const int cb = C < LY_THREADS ? C : LY_THREADS;          // channels handled per pass by this block
  const int subs = LY_THREADS / cb;
  const int tid = threadIdx.x;
  const int cl = tid % cb, sub = tid / cb;
  const long npix = (long)n_img * Ho * Wo;
  for (int c0 = 0; c0 < C; c0 += cb) {
    const int c = c0 + cl;
    float m1[9], m2[45];
#pragma unroll
    for (int i = 0; i < 9; ++i) m1[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 45; ++i) m2[i] = 0.f;
    if (sub < subs && c < C) {
      // two output pixels per trip, their 18 taps loaded unconditionally from clamped coordinates before the first use (`ok ? load : 0` is a
      // branch around a load: every wait after it turns conservative and the taps arrive one round trip at a time); masks in the arithmetic
      const long stride = (long)gridDim.x * subs;
      for (long p0 = (long)blockIdx.x * subs + sub; p0 < npix; p0 += 2 * stride) {
        float xv[2][9];
        bool okk[2][9];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const long p = p0 + j * stride;
          const bool live = p < npix;
          const long pc = live ? p : npix - 1;
          const int ox = (int)(pc % Wo);
          const long q = pc / Wo;
          const int oy = (int)(q % Ho);
          const long n = q / Ho;
#pragma unroll
          for (int u = 0; u < 9; ++u) {
            const int iy = s * oy + u / 3 - 1, ix = s * ox + u % 3 - 1;
            okk[j][u] = live && iy >= 0 && iy < H && ix >= 0 && ix < W;
            const int cy = iy < 0 ? 0 : (iy >= H ? H - 1 : iy), cx = ix < 0 ? 0 : (ix >= W ? W - 1 : ix);
            xv[j][u] = ly_ld1<T>(x + ((n * H + cy) * W + cx) * ldx + c);
          }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
          for (int u = 0; u < 9; ++u) xv[j][u] = okk[j][u] ? xv[j][u] : 0.f;
          int k = 0;
#pragma unroll
          for (int u = 0; u < 9; ++u) {
            m1[u] += xv[j][u];
#pragma unroll
            for (int v = u; v < 9; ++v) m2[k++] += xv[j][u] * xv[j][v];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 9; ++i) atomicAdd(mom + (long)i * C + c, (double)m1[i]);
#pragma unroll
      for (int i = 0; i < 45; ++i) atomicAdd(mom + (long)(9 + i) * C + c, (double)m2[i]);
    }
  }
}

// Stride-2 form through an LDS tile (the two k = 3 RFCBAMConv layers of the detector): a block walks 8 x 8 tiles of output pixels; the 17 x 17 input
// pixels x 64 channels of a tile are staged ONCE with 16-byte loads, lane = channel then reads its nine taps from LDS.  The 54 moments stay in
// registers over all tiles of the block and are reduced over its four waves before ONE atomic per moment, channel and block — the per-pixel
// kernel above issues eighteen 2-byte loads per trip and 54 atomics per thread (91 us per launch at bs=64; fewer blocks starve it of loads in
// flight, more blocks drown it in atomics).
#define LY_TM_T 8
template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_rfcbam_tap_moments_s2t_kernel(const T* __restrict__ x, int ldx, int n_img, int H, int W, int C, int Ho, int Wo,
                                                                                int tiles_y, int tiles_x, double* __restrict__ mom) {
  constexpr int TM = LY_TM_T, TW = 2 * TM + 1, NPX = TW * TW;
  constexpr int VE = 16 / (int)sizeof(T), VPR = 64 / VE;
  extern __shared__ f32x4 ly_tm_smem[];
  T* const tile = reinterpret_cast<T*>(ly_tm_smem);              // [NPX][64]
  float* const red = reinterpret_cast<float*>(ly_tm_smem);       // reused after the walk: [4][27][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.y * 64;
  const int c = c0 + lane;
  const bool cok = c < C;
  // two output pixels per trip as the halves of float2 accumulators: the 54 multiply-adds per pixel become 54 packed ones per PAIR
  // (v_pk_fma_f32) — the kernel is bound by exactly these
  typedef float ly_f2 __attribute__((ext_vector_type(2)));
  ly_f2 a1[9], a2[45];
#pragma unroll
  for (int i = 0; i < 9; ++i) a1[i] = (ly_f2){0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 45; ++i) a2[i] = (ly_f2){0.f, 0.f};
  const long ntiles = (long)n_img * tiles_y * tiles_x;
  for (long tix = ly_xcd_remap((int)blockIdx.x, (int)gridDim.x); tix < ntiles; tix += gridDim.x) {
    const int tx = (int)(tix % tiles_x);
    const long q = tix / tiles_x;
    const int ty = (int)(q % tiles_y);
    const long n = q / tiles_y;
    const int oy0 = ty * TM, ox0 = tx * TM;
    __syncthreads();                                             // the previous tile has been consumed
    for (int i = tid; i < NPX * VPR; i += LY_THREADS) {
      const int px = i / VPR, v = i - px * VPR;
      const int iy = 2 * oy0 - 1 + px / TW, ix = 2 * ox0 - 1 + px % TW;
      const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W && c0 + v * VE < C;
      const int cy = iy < 0 ? 0 : (iy >= H ? H - 1 : iy), cx = ix < 0 ? 0 : (ix >= W ? W - 1 : ix);
      ly_u32x4 raw = *reinterpret_cast<const ly_u32x4*>(x + ((n * H + cy) * W + cx) * (long)ldx + (c0 + v * VE < C ? c0 + v * VE : 0));
      if (!ok) raw = (ly_u32x4){0u, 0u, 0u, 0u};
      *reinterpret_cast<ly_u32x4*>(tile + (long)px * 64 + v * VE) = raw;
    }
    __syncthreads();
    for (int p = wave; p < TM * TM; p += 8) {                   // pixels p and p + 4 (TM*TM is a multiple of 8)
      const int pa = p, pb = p + 4;
      const int ya = pa / TM, xa = pa - ya * TM, yb = pb / TM, xb = pb - yb * TM;
      const bool la = oy0 + ya < Ho && ox0 + xa < Wo, lb = oy0 + yb < Ho && ox0 + xb < Wo;
      ly_f2 xv[9];
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        const float va = (float)tile[((2 * ya + u / 3) * TW + 2 * xa + u % 3) * 64 + lane];
        const float vb = (float)tile[((2 * yb + u / 3) * TW + 2 * xb + u % 3) * 64 + lane];
        xv[u] = (ly_f2){la ? va : 0.f, lb ? vb : 0.f};
      }
      int k = 0;
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        a1[u] += xv[u];
#pragma unroll
        for (int v = u; v < 9; ++v) a2[k++] += xv[u] * xv[v];
      }
    }
  }
  float m1[9], m2[45];
#pragma unroll
  for (int i = 0; i < 9; ++i) m1[i] = a1[i][0] + a1[i][1];
#pragma unroll
  for (int i = 0; i < 45; ++i) m2[i] = a2[i][0] + a2[i][1];
  // block reduction over the four waves, two rounds of 27 moments through the tile's LDS, then one atomic per (moment, channel)
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 27; ++i) {
      const int e = half * 27 + i;
      red[(wave * 27 + i) * 64 + lane] = e < 9 ? m1[e < 9 ? e : 0] : m2[e >= 9 ? e - 9 : 0];
    }
    __syncthreads();
    for (int j = tid; j < 27 * 64; j += LY_THREADS) {
      const int i = j >> 6, l = j & 63;
      if (c0 + l < C) atomicAdd(mom + (long)(half * 27 + i) * C + c0 + l, (double)((red[j] + red[27 * 64 + j]) + (red[2 * 27 * 64 + j] + red[3 * 27 * 64 + j])));
    }
  }
  (void)cok;
}

static int tap_moments_entry(const void* x, int ldx, int n_img, int H, int W, int C, int s, double* mom, int dtype, const LyOut& out) {
  LY_CHECK_DTYPE(dtype, "rfcbam_tap_moments");
  LY_CHECK(x && mom && s >= 1 && C > 0, "rfcbam_tap_moments: bad arguments");
  const int Ho = (H + 2 - 3) / s + 1, Wo = (W + 2 - 3) / s + 1;
  long npix = (long)n_img * Ho * Wo;
  const int esz = dtype == LY_BF16 ? 2 : 4;
  if (s == 2 && C % (16 / esz) == 0 && ldx % (16 / esz) == 0 && ((uintptr_t)x & 15) == 0) {
    const int tiles_y = (Ho + LY_TM_T - 1) / LY_TM_T, tiles_x = (Wo + LY_TM_T - 1) / LY_TM_T;
    const int groups = (C + 63) / 64;
    long nb = (long)n_img * tiles_y * tiles_x;
    const long cap = 768 / groups > 0 ? 768 / groups : 1;               // ~768 blocks: 3456 atomics each
    if (nb > cap) nb = cap;
    constexpr int NPX = (2 * LY_TM_T + 1) * (2 * LY_TM_T + 1);
    size_t lds = (size_t)NPX * 64 * esz;
    if (lds < 4 * 27 * 64 * sizeof(float)) lds = 4 * 27 * 64 * sizeof(float);
    LY_WITH_T(dtype, return LY_EMIT(out, (ly_launch_lds<ly_rfcbam_tap_moments_s2t_kernel<T>>(dim3((unsigned)nb, (unsigned)groups), dim3(LY_THREADS), lds, out.st,
                                                                                             reinterpret_cast<const T*>(x), ldx, n_img, H, W, C, Ho, Wo, tiles_y, tiles_x, mom)),
                                    "ly_rfcbam_tap_moments_s2t_kernel<%s>", ly_tname<T>()));
  }
  long blocks = npix / 32 + 1;
  if (blocks > 1024) blocks = 1024;
  LY_WITH_T(dtype, return LY_EMIT(out, (ly_launch<ly_rfcbam_tap_moments_kernel<T>>(dim3((unsigned)blocks), dim3(LY_THREADS), 0, out.st, reinterpret_cast<const T*>(x), ldx,
                                                                                   n_img, H, W, C, Ho, Wo, s, mom)),
                                  "ly_rfcbam_tap_moments_kernel<%s>", ly_tname<T>()));
}

extern "C" int ly_rfcbam_tap_moments(const void* x, int ldx, int n_img, int H, int W, int C, int s, double* mom, int dtype, void* stream) {
  return tap_moments_entry(x, ldx, n_img, H, W, C, s, mom, dtype, LY_ON_STREAM(stream));
}

// the arguments of ly_rfcbam_tap_moments with (name, cap) for the stream
extern "C" int ly_rfcbam_tap_moments_describe(const void* x, int ldx, int n_img, int H, int W, int C, int s, double* mom, int dtype, char* name, int cap) {
  LY_CHECK(name && cap > 0, "rfcbam_tap_moments_describe: bad arguments");
  return tap_moments_entry(x, ldx, n_img, H, W, C, s, mom, dtype, LyOut{nullptr, name, cap});
}

// ---------------------------------------------------------------------------------------------------
// RFCBAMConv `generate` BatchNorm in training, everything between the moment kernel and the contraction in ONE launch
// (models/rfa.py:101-106 generate = depthwise conv -> BatchNorm -> ReLU, training=True):
//   from the tap moments of x (k = 3: ly_rfcbam_tap_moments, 9 first + 45 second moments per channel; k = 1: ly_chan_moments, sum x and
//   sum x^2) and the depthwise weights, per generate channel g = c*KK + t:
//     sum a = w_t . m,  sum a^2 = w_t^T M w_t   ->  batch mean / var  ->  scale = gamma*invstd, shift = beta - mean*scale,
//     running_mean / running_var (momentum, unbiased) and num_batches_tracked updated as nn.BatchNorm2d does;
//   outputs: scale, shift, mean, invstd in [c*KK + t] order, the same four in [t*C + c] order (what the backward kernels index),
//   and — k = 3 — the folded weights (w*scale | shift) in the two LDS orders of the statistics / contraction kernels
//   (pack.rfcbam_gen_weights: [C_pad/chunk][4 waves][9 t][chunk/8 pairs][10][2]); k = 1: a1 = w*scale.
// Replaces ~40 tiny torch launches per module and step (einsum / index_put / cat / permute / BatchNorm arithmetic).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ long ly_gw_index(int ch, int t, int e, int chunk, bool contiguous) {
  const int per = chunk >> 2;
  const int q = ch / chunk, r = ch - q * chunk;
  const int w = contiguous ? r / per : r & 3;
  const int j = contiguous ? r - w * per : r >> 2;
  const int p = j >> 1, ab = j & 1;
  return (((((long)q * 4 + w) * 9 + t) * (per >> 1) + p) * 10 + e) * 2 + ab;
}

__global__ __launch_bounds__(LY_THREADS) void ly_rfcbam_gen_prepare_kernel(
    const double* __restrict__ mom, int C, int KK, const float* __restrict__ gen_w, const float* __restrict__ gamma,
    const float* __restrict__ beta, float eps, float momentum, double count, float* __restrict__ running_mean,
    float* __restrict__ running_var, long* __restrict__ nbt, float* __restrict__ out8 /* [8][C*KK] */, float* __restrict__ a1,
    float* __restrict__ wq_stats, int cp_stats, float* __restrict__ wq_main, int cp_main, float* __restrict__ wq_c, const int mom_stripes) {
  const int G = C * KK;
  const int cpm = cp_stats > cp_main ? cp_stats : cp_main;
  const int total = (KK == 9 ? (cpm > C ? cpm : C) : C) * KK;
  for (int g = blockIdx.x * LY_THREADS + threadIdx.x; g < total; g += gridDim.x * LY_THREADS) {
    const int c = g / KK, t = g - c * KK;
    if (c >= C) {                                          // padded channels of the packed images: zero weights
      for (int e = 0; e < 10; ++e) {
        if (c < cp_stats) wq_stats[ly_gw_index(c, t, e, 32, false)] = 0.f;
        if (c < cp_main) wq_main[ly_gw_index(c, t, e, 16, true)] = 0.f;
      }
      continue;
    }
    double s1 = 0.0, s2 = 0.0;
    float w[9];
    if (KK == 9) {
#pragma unroll
      for (int u = 0; u < 9; ++u) w[u] = gen_w[(long)g * 9 + u];
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        s1 += (double)w[u] * mom[u * C + c];
#pragma unroll
        for (int v = u; v < 9; ++v) {
          const int tri = u * 9 - (u * (u - 1)) / 2 + (v - u);                 // torch.triu_indices(9, 9) order
          const double m = mom[(9 + tri) * C + c];
          s2 += (u == v ? 1.0 : 2.0) * (double)w[u] * (double)w[v] * m;
        }
      }
    } else {
      w[0] = gen_w[g];
      // k = 1: the moments as ly_chan_moments left them — mom_stripes copies of [2C] doubles, folded here in index order (was a launch of its own)
      double m1 = 0.0, m2 = 0.0;
      for (int st = 0; st < mom_stripes; ++st) {
        m1 += mom[(size_t)st * 2 * C + c];
        m2 += mom[(size_t)st * 2 * C + C + c];
      }
      s1 = (double)w[0] * m1;
      s2 = (double)w[0] * (double)w[0] * m2;
    }
    const double mean = s1 / count;
    double var = s2 / count - mean * mean;
    var = var > 0.0 ? var : 0.0;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const float sc = gamma[g] * invstd;
    const float sh = beta[g] - (float)mean * sc;
    if (running_mean) {
      running_mean[g] = (1.f - momentum) * running_mean[g] + momentum * (float)mean;
      running_var[g] = (1.f - momentum) * running_var[g] + momentum * (float)(var * (count / (count > 1.0 ? count - 1.0 : 1.0)));
    }
    const int gt = t * C + c;
    out8[g] = sc;            out8[G + g] = sh;             out8[2 * G + g] = (float)mean;  out8[3 * G + g] = invstd;
    out8[4 * G + gt] = sc;   out8[5 * G + gt] = sh;        out8[6 * G + gt] = (float)mean; out8[7 * G + gt] = invstd;
    if (KK == 9) {
#pragma unroll
      for (int e = 0; e < 10; ++e) {
        const float v = e < 9 ? w[e] * sc : sh;
        wq_stats[ly_gw_index(c, t, e, 32, false)] = v;
        wq_main[ly_gw_index(c, t, e, 16, true)] = v;
        if (wq_c) {                                                            // lane = channel order, RAW form (ly_rf3c.hpp rc_load_w)
          const int i = e < 9 ? t * 9 + e : 81 + t;
          wq_c[(((long)(c >> 5) * 25 + (i >> 2)) * 32 + (c & 31)) * 4 + (i & 3)] = e < 9 ? w[e] : sh;
          if (e == 9) wq_c[(((long)(c >> 5) * 25 + ((90 + t) >> 2)) * 32 + (c & 31)) * 4 + ((90 + t) & 3)] = sc;
        }
      }
    } else {
      a1[g] = w[0] * sc;
    }
  }
  if (nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;
}

extern "C" int ly_rfcbam_gen_prepare(const double* mom, int C, int k, const float* gen_w, const float* gamma, const float* beta, float eps,
                                     float momentum, double count, float* running_mean, float* running_var, long* nbt, float* out8,
                                     float* a1, float* wq_stats, float* wq_main, float* wq_c, int mom_stripes, void* stream) {
  LY_CHECK(mom && gen_w && gamma && beta && out8 && C > 0 && (k == 1 || k == 3) && count > 0, "rfcbam_gen_prepare: bad arguments");
  LY_CHECK(mom_stripes >= 1 && (k == 1 || mom_stripes == 1), "rfcbam_gen_prepare: striped moments are read for k = 1 only (mom_stripes=%d)", mom_stripes);
  LY_CHECK(k == 1 ? a1 != nullptr : (wq_stats && wq_main), "rfcbam_gen_prepare: missing output for k=%d", k);
  LY_CHECK(!running_mean == !running_var, "rfcbam_gen_prepare: running_mean and running_var go together");
  const int KK = k * k;
  const int cp_s = (C + 31) / 32 * 32, cp_m = (C + 15) / 16 * 16;
  const int total = (k == 3 ? cp_s : C) * KK;
  hipLaunchKernelGGL(ly_rfcbam_gen_prepare_kernel, dim3((unsigned)((total + LY_THREADS - 1) / LY_THREADS)), dim3(LY_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), mom, C, KK, gen_w, gamma, beta, eps, momentum, count, running_mean, running_var, nbt,
                     out8, a1, wq_stats, k == 3 ? cp_s : 0, wq_main, k == 3 ? cp_m : 0, k == 3 ? wq_c : nullptr, mom_stripes);
  LY_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------
// SE backward in training (models/rfa.py:88-92 under autograd), one block per image:
//   gap = mean x (from the forward's slice partials);  h = relu(Wa gap);  ca = sigmoid(Wb h)  (ca given)
//   dz = d_ca*ca*(1-ca);  dWb[c,r] += dz[c]*h[r];  dh = (Wb^T dz) * (h > 0);  dWa[r,c] += dh[r]*gap[c];  dgap[n,c] = Wa^T dh  (written)
// dgap / HW is what every pixel of x receives from the pooling: ly_rf_bwd_dx adds it while it writes dx.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LY_THREADS) void ly_se_bwd_kernel(const float* __restrict__ part, int slices, int C, float inv_hw,
                                                                const float* __restrict__ wa, const float* __restrict__ wb, int R,
                                                                const float* __restrict__ ca, const void* __restrict__ d_ca_v, const int d_ca_f64,
                                                                float* __restrict__ ws, float* __restrict__ dgap) {
  extern __shared__ float sm[];
  float* g = sm;                     // g[C] | dz[C] | hid[R] | dh[R] | red
  float* dz = sm + C;
  float* hid = sm + 2 * C;
  float* dh = hid + R;
  f32x4* red = reinterpret_cast<f32x4*>(sm + ((2 * C + 2 * R + 3) & ~3));
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nq = C >> 2, ng = LY_THREADS / nq;
  const int q = tid % nq, sg = tid / nq;
  f32x4 s4 = ly_zero4();
  if (sg < ng)
    for (int sl = sg; sl < slices; sl += ng) s4 += ly_ldg4(part + ((long)n * slices + sl) * C + 4 * q);
  red[tid] = s4;
  __syncthreads();
  if (sg == 0) {
    for (int k = 1; k < ng; ++k) s4 += red[tid + k * nq];
#pragma unroll
    for (int e = 0; e < 4; ++e) g[4 * q + e] = s4[e] * inv_hw;
  }
  for (int c = tid; c < C; c += LY_THREADS) {
    const float a = ca[(long)n * C + c];
    // d_ca as the double accumulators ly_rf1_bwd / ly_rf3c_bwd left it in (d_ca_f64), no conversion pass in between
    const float dca = d_ca_f64 ? (float)reinterpret_cast<const double*>(d_ca_v)[(long)n * C + c] : reinterpret_cast<const float*>(d_ca_v)[(long)n * C + c];
    dz[c] = dca * a * (1.f - a);
  }
  __syncthreads();
  for (int r = wave; r < R; r += 4) {
    float s = 0.f, d = 0.f;
    for (int c = lane; c < C; c += 64) {
      s += wa[r * C + c] * g[c];
      d += wb[c * R + r] * dz[c];
    }
    s = ly_group_sum(s, 64);
    d = ly_group_sum(d, 64);
    if (lane == 0) {
      hid[r] = fmaxf(s, 0.f);
      dh[r] = s > 0.f ? d : 0.f;
    }
  }
  __syncthreads();
  // the per-image factors of the two weight gradients go to the workspace ws[n][g | dz | hid | dh]; ly_se_bwd_wsum_kernel sums the outer
  // products over the images, one thread per weight (2*C*R float atomics per image here made the launch 38 us at bs=64)
  float* const wsn = ws + (long)n * (2 * C + 2 * R);
  for (int c = tid; c < C; c += LY_THREADS) {
    float dg = 0.f;
    for (int r = 0; r < R; ++r) dg += dh[r] * wa[r * C + c];
    dgap[(long)n * C + c] = dg;
    wsn[c] = g[c];
    wsn[C + c] = dz[c];
  }
  for (int r = tid; r < R; r += LY_THREADS) {
    wsn[2 * C + r] = hid[r];
    wsn[2 * C + R + r] = dh[r];
  }
}

// dWb[c][r] += sum_n dz[n][c]*hid[n][r],  dWa[r][c] += sum_n dh[n][r]*g[n][c]   (thread = (r, c), c fastest: deterministic, no atomics)
__global__ __launch_bounds__(LY_THREADS) void ly_se_bwd_wsum_kernel(const float* __restrict__ ws, int n_img, int C, int R, float* __restrict__ dwa,
                                                                     float* __restrict__ dwb) {
  const int i = blockIdx.x * LY_THREADS + threadIdx.x;
  if (i >= C * R) return;
  const int r = i / C, c = i - r * C;
  const int st = 2 * C + 2 * R;
  // eight images per trip, all 32 loads issued before the first use (one image per trip was 64 dependent L2 round trips: 19 us for 80 KB);
  // the sums keep the image order
  float sa = 0.f, sb = 0.f;
  int n = 0;
  for (; n + 8 <= n_img; n += 8) {
    float a0[8], a1[8], b0[8], b1[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float* w = ws + (long)(n + k) * st;
      b0[k] = w[C + c]; b1[k] = w[2 * C + r]; a0[k] = w[2 * C + R + r]; a1[k] = w[c];
    }
    __builtin_amdgcn_sched_barrier(0);               // (left alone the scheduler sinks the loads back between the FMAs: four per round trip again)
#pragma unroll
    for (int k = 0; k < 8; ++k) { sb += b0[k] * b1[k]; sa += a0[k] * a1[k]; }
  }
  for (; n < n_img; ++n) {
    const float* w = ws + (long)n * st;
    sb += w[C + c] * w[2 * C + r];
    sa += w[2 * C + R + r] * w[c];
  }
  dwb[c * R + r] += sb;
  dwa[r * C + c] += sa;
}

extern "C" int ly_se_bwd(const float* part, int slices, int n_img, int HW, int C, const float* wa, const float* wb, int R, const float* ca,
                         const void* d_ca, int d_ca_f64, float* dwa, float* dwb, float* dgap, float* ws, void* stream) {
  LY_CHECK(part && wa && wb && ca && d_ca && dwa && dwb && dgap && ws, "se_bwd: null pointer");
  LY_CHECK((C & 3) == 0 && C <= 1024 && slices > 0 && R > 0 && R <= 256 && n_img > 0 && HW > 0, "se_bwd: bad arguments");
  hipLaunchKernelGGL(ly_se_bwd_kernel, dim3(n_img), dim3(LY_THREADS), sizeof(float) * (((2 * C + 2 * R + 3) & ~3) + 4 * LY_THREADS),
                     reinterpret_cast<hipStream_t>(stream), part, slices, C, 1.f / (float)HW, wa, wb, R, ca, d_ca, d_ca_f64, ws, dgap);
  LY_LAUNCH_CHECK();
  hipLaunchKernelGGL(ly_se_bwd_wsum_kernel, dim3((unsigned)((C * R + LY_THREADS - 1) / LY_THREADS)), dim3(LY_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), ws, n_img, C, R, dwa, dwb);
  LY_LAUNCH_CHECK();
  return 0;
}
