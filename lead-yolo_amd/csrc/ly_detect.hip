// Detect level in ONE launch (eval): the head's 1x1 convolution to na*no channels + the decode of models/yolo.py:95-120   (gfx950 only)
//   p[n, a, h, w, o] = (W x[n, h, w, :] + b)[a*no + o]                              (the raw map the reference returns beside z)
//   z[n, zoff + (a*H + h)*W + w, o] = xy: (2 sig - 0.5 + grid) * stride, wh: (2 sig)^2 * anchor * stride, rest: sig
// The generic route was two launches per level — a GEMM to an [M, 20]-column buffer in the storage type (N = 18 is no multiple of 4: its
// slow epilogue) and ly_detect_tail re-reading it — ~17 us per level in the serving forward for a few MB.  Here a wave owns 16 pixels: its B
// operand is read straight from the feature map (lane (pixel, g) loads the 8 channels 32 s + 8 g .. of its pixel per k-step: 64 contiguous bytes
// per pixel over the four g), the two weight tiles (32 rows, natural k order: pack.frag_pack_nat) sit in LDS, and sigmoid / grid / anchor
// arithmetic runs on the fp32 accumulators — the raw map is no longer rounded to bf16 on its way to p.
//
//   ly_detect_level, ly_detect_level_aug the one-launch level above, plain and with the test-time augmentation's _descale_pred
//   ly_detect_level_ok                   whether (K, na, no, dtype) is built
// Beside it, the pieces of the generic route and of the training step:
//   ly_detect_tail, ly_detect_tail_aug   raw map + decode from the head GEMM's output y[n, h, w, na*no]          (models/yolo.py:95-120)
//   ly_detect_head_bwd                   adjoint of the raw-map permute: dp -> the head's du rows and dbias        (models/yolo.py:88)
#include "ly_common.hpp"
#include "ly_tile.hpp"

#define LY_DET_LD 36            // floats per pixel row of a wave's output tile in LDS (32 channels + pad, rows 16-byte aligned)

// AUG (test-time augmentation, ly_detect_level_aug): _descale_pred of models/yolo.py applied to the decoded rows before the store — xywh / dscale
// (a true division, as torch's `/=`), then x = img_w - x for the left-right flipped pass; p may be NULL.  A compile-time flag: the plain
// instantiations below are the kernels they were.
template <typename T, int S, bool NAT, bool AUG>
__global__ __launch_bounds__(LY_THREADS) void ly_detect_level_kernel(const T* __restrict__ x, const int ldx, const long M, const int H, const int W,
                                                                      const uint4* __restrict__ wp, const float* __restrict__ bias, const int na,
                                                                      const int no, const float* __restrict__ anchors, const float stride,
                                                                      float* __restrict__ p, float* __restrict__ z, const long zrows, const long zoff,
                                                                      const int ntiles, const int tpw, const float dscale, const int dflip,
                                                                      const float img_w) {
  constexpr int PL = LyT<T>::PL;
  extern __shared__ uint4 ly_det_w[];                       // [2 tiles][S][PL][64 lanes]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 2 * S * PL * 64; i += LY_THREADS) ly_det_w[i] = wp[i];
  __syncthreads();
  const int px = lane & 15, g = lane >> 4;
  const int co = na * no, HW = H * W;
  const float invHW = 1.f / (float)HW, invW = 1.f / (float)W;
  float cb[2][4];                                            // bias of the lane's channels c = 16 t + 4 g + r
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = 16 * t + 4 * g + r;
      cb[t][r] = c < co ? bias[c] : 0.f;
    }
  float* const ot = reinterpret_cast<float*>(ly_det_w + 2 * S * PL * 64) + wave * (16 * LY_DET_LD);
  const int tile0 = (blockIdx.x * (LY_THREADS / 64) + wave) * tpw;
  for (int i = 0; i < tpw; ++i) {
    const int tile = tile0 + i;
    if (tile >= ntiles) break;
    const long m = (long)tile * 16 + px;
    const bool live = m < M;
    // NAT: the lane's 8 channels of a k-step are consecutive (32 s + 8 g ..: one 16-byte load in bf16); else the k order of pack.frag_pack3
    // (32 s + 4 g + 0..3 and 32 s + 16 + 4 g + 0..3: the training step's packed weights are used as they are)
    const T* row = x + (live ? m : M - 1) * ldx + (NAT ? 8 : 4) * g;
    constexpr int SECOND = NAT ? 4 : 16;
    bf16x8 xh[S], xl[S];
    if constexpr (PL == 1) {
      ly_u32x2 ra[S], rb[S];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        ra[s] = *reinterpret_cast<const ly_u32x2*>(row + 32 * s);
        rb[s] = *reinterpret_cast<const ly_u32x2*>(row + 32 * s + SECOND);
      }
#pragma unroll
      for (int s = 0; s < S; ++s) {
        xh[s] = ly_cat8(__builtin_bit_cast(bf16x4, ra[s]), __builtin_bit_cast(bf16x4, rb[s]));
        xl[s] = xh[s];
      }
    } else {
      f32x4 ra[S], rb[S];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        ra[s] = *reinterpret_cast<const f32x4*>(row + 32 * s);
        rb[s] = *reinterpret_cast<const f32x4*>(row + 32 * s + SECOND);
      }
#pragma unroll
      for (int s = 0; s < S; ++s) {
        bf16x4 h0, l0, h1, l1;
        ly_split4(ra[s], h0, l0);
        ly_split4(rb[s], h1, l1);
        xh[s] = ly_cat8(h0, h1);
        xl[s] = ly_cat8(l0, l1);
      }
    }
    f32x4 acc[2] = {ly_zero4(), ly_zero4()};
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const bf16x8 wh = __builtin_bit_cast(bf16x8, ly_det_w[((t * S + s) * PL + 0) * 64 + lane]);
        if constexpr (PL == 2) {
          const bf16x8 wl = __builtin_bit_cast(bf16x8, ly_det_w[((t * S + s) * PL + 1) * 64 + lane]);
          acc[t] = ly_mfma3(wh, wl, xh[s], xl[s], acc[t]);
        } else {
          acc[t] = ly_mfma_bf16(wh, xh[s], acc[t]);
        }
      }
    // accumulators (+ bias) -> the wave's [16 px][36] fp32 LDS tile -> lanes walk the tile's outputs in MEMORY order (anchor, pixel, o): p and z
    // of 16 consecutive pixels are na runs of 16 no contiguous floats each, so every store instruction writes consecutive addresses
    // (written from the accumulator layout — lane = (pixel, 4 channels) — the same bytes took 16 scattered 4-byte stores per lane: 19.6 us at
    // 80 x 80 x 128, bs=16).
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[t][r] + cb[t][r];
      *reinterpret_cast<f32x4*>(ot + px * LY_DET_LD + 16 * t + 4 * g) = v;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);                      // lgkmcnt(0): the tile is written (one wave: no block barrier)
    const long m0 = (long)tile * 16;
    const int run = 16 * no, total = na * run;
    for (int e = lane; e < total; e += 64) {
      const int a = e / run, q = e - a * run;
      const int pl = q / no, o = q - pl * no;
      const long mm = m0 + pl;
      if (mm >= M) continue;
      const int n = ly_fdiv((int)mm, HW, invHW);
      const int hw = (int)mm - n * HW;
      const float v = ot[pl * LY_DET_LD + a * no + o];
      if constexpr (AUG) {
        if (p) p[(((long)n * na + a) * HW + hw) * no + o] = v;
      } else {
        p[(((long)n * na + a) * HW + hw) * no + o] = v;
      }
      if (z) {
        const int h = ly_fdiv(hw, W, invW);
        const int w = hw - h * W;
        const float sg = ly_sigmoid(v);
        float r = sg;
        if (o == 0) r = (sg * 2.f + ((float)w - 0.5f)) * stride;
        else if (o == 1) r = (sg * 2.f + ((float)h - 0.5f)) * stride;
        else if (o == 2 || o == 3) { const float d = sg * 2.f; r = d * d * (anchors[a * 2 + (o - 2)] * stride); }
        if constexpr (AUG) {
          if (o < 4) r = r / dscale;
          if (o == 0 && dflip) r = img_w - r;
        }
        z[((long)n * zrows + zoff + (long)a * HW + hw) * no + o] = r;
      }
    }
    __builtin_amdgcn_wave_barrier();                         // (the next tile overwrites the LDS tile)
  }
}

template <typename T, int S, bool AUG>
static void detect_level_launch(const int nat, const void* x, int ldx, long M, int H, int W, const void* wp, const float* bias, int na, int no, const float* anchors,
                                float stride, float* p, float* z, long zrows, long zoff, float dscale, int dflip, float img_w, hipStream_t st) {
  const int ntiles = (int)((M + 15) / 16);
  // tiles per wave: one until every SIMD holds ~4 waves, then more (the 2 x K weight rows a block stages are amortised over 4 tpw tiles).
  // Measured at bs=16 (one round of blocks): every further tile per wave adds ~5 us — a tile is one serial chain of memory round trips.
  int tpw = ntiles / (256 * 4 * 4);
  tpw = tpw < 1 ? 1 : tpw > 8 ? 8 : tpw;
  const int per_block = (LY_THREADS / 64) * tpw;
  const size_t lds = (size_t)2 * S * LyT<T>::PL * 64 * sizeof(uint4) + (LY_THREADS / 64) * 16 * LY_DET_LD * sizeof(float);
  const dim3 grid((unsigned)((ntiles + per_block - 1) / per_block));
  if (nat)
    hipLaunchKernelGGL((ly_detect_level_kernel<T, S, true, AUG>), grid, dim3(LY_THREADS), lds, st, reinterpret_cast<const T*>(x), ldx, M, H, W,
                       reinterpret_cast<const uint4*>(wp), bias, na, no, anchors, stride, p, z, zrows, zoff, ntiles, tpw, dscale, dflip, img_w);
  else
    hipLaunchKernelGGL((ly_detect_level_kernel<T, S, false, AUG>), grid, dim3(LY_THREADS), lds, st, reinterpret_cast<const T*>(x), ldx, M, H, W,
                       reinterpret_cast<const uint4*>(wp), bias, na, no, anchors, stride, p, z, zrows, zoff, ntiles, tpw, dscale, dflip, img_w);
}

template <bool AUG>
static int detect_level_entry(const char* who, const void* x, int ldx, int n_img, int H, int W, int K, const void* wp, int nat, const float* bias,
                              int na, int no, const float* anchors, float stride, float* p, float* z, long zrows, long zoff, float dscale, int dflip,
                              float img_w, int dtype, void* stream) {
  LY_CHECK((dtype) == LY_F32 || (dtype) == LY_BF16, "%s: unknown dtype %d", who, dtype);
  if constexpr (AUG)
    LY_CHECK(x && wp && bias && anchors && z && n_img > 0 && H > 0 && W > 0 && dscale > 0.f, "%s: null pointer / bad sizes", who);
  else
    LY_CHECK(x && wp && bias && anchors && p && n_img > 0 && H > 0 && W > 0, "%s: null pointer / bad sizes", who);
  LY_CHECK(na * no <= 32 && na > 0 && no > 0, "%s: na*no = %d exceeds the 32 output rows of the kernel", who, na * no);
  const int vw = dtype == LY_BF16 ? 8 : 4;
  LY_CHECK((K & 31) == 0 && ldx >= K && (ldx % vw) == 0 && ((uintptr_t)x & 15) == 0, "%s: K = %d must be a multiple of 32, rows 16-byte aligned", who, K);
  const long M = (long)n_img * H * W;
  LY_CHECK(M < (1L << 24), "%s: too many pixels", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int S = K / 32;
#define LY_DET(S_) LY_WITH_T(dtype, (detect_level_launch<T, S_, AUG>(nat, x, ldx, M, H, W, wp, bias, na, no, anchors, stride, p, z, zrows, zoff, dscale, dflip, img_w, st)))
  if (S == 2) LY_DET(2);
  else if (S == 4) LY_DET(4);
  else if (S == 8) LY_DET(8);
  else if (S == 16 && dtype == LY_BF16) detect_level_launch<__bf16, 16, AUG>(nat, x, ldx, M, H, W, wp, bias, na, no, anchors, stride, p, z, zrows, zoff, dscale, dflip, img_w, st);
  else { ly_set_error("%s: K = %d is not built (64, 128, 256; 512 in bf16)", who, K); return -1; }
#undef LY_DET
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_detect_level(const void* x, int ldx, int n_img, int H, int W, int K, const void* wp, int nat, const float* bias, int na, int no,
                               const float* anchors, float stride, float* p, float* z, long zrows, long zoff, int dtype, void* stream) {
  return detect_level_entry<false>("detect_level", x, ldx, n_img, H, W, K, wp, nat, bias, na, no, anchors, stride, p, z, zrows, zoff, 1.f, 0, 0.f, dtype,
                                   stream);
}

extern "C" int ly_detect_level_aug(const void* x, int ldx, int n_img, int H, int W, int K, const void* wp, int nat, const float* bias, int na, int no,
                                   const float* anchors, float stride, float* p, float* z, long zrows, long zoff, float dscale, int dflip, float img_w,
                                   int dtype, void* stream) {
  return detect_level_entry<true>("detect_level_aug", x, ldx, n_img, H, W, K, wp, nat, bias, na, no, anchors, stride, p, z, zrows, zoff, dscale, dflip,
                                  img_w, dtype, stream);
}

extern "C" int ly_detect_level_ok(int K, int na, int no, int dtype) {
  const int S = K / 32;
  return (K % 32 == 0) && na * no <= 32 && (S == 2 || S == 4 || S == 8 || (S == 16 && dtype == LY_BF16));
}

// ---------------------------------------------------------------------------------------------------
// Detect tail (reference models/yolo.py:95-120): from the head GEMM output y[n, h, w, na*no] (row stride
// ldy) write the raw map p[n, a, h, w, o] and, in eval mode, the decoded rows z[n, zoff + (a*H + h)*W + w, o]:
//   xy = (2*sig - 0.5 + grid) * stride,  wh = (2*sig)^2 * anchor*stride,  rest = sig.
// ---------------------------------------------------------------------------------------------------
// AUG: the _descale_pred step of test-time augmentation on the decoded rows (see ly_detect_level_kernel above); p may be NULL there.
template <typename T, bool AUG>
__device__ __forceinline__ void ly_detect_tail_body(const T* __restrict__ y, int ldy, long total, int H, int W, int na, int no,
                                                    const float* __restrict__ anchors /* [na,2] grid units */, float stride,
                                                    float* __restrict__ p, float* __restrict__ z, long zrows, long zoff, float dscale, int dflip,
                                                    float img_w) {
  const long i = (long)blockIdx.x * LY_THREADS + threadIdx.x;      // over n*na*H*W*no, output order
  if (i >= total) return;
  const int o = (int)(i % no);
  long t = i / no;
  const int w = (int)(t % W); t /= W;
  const int h = (int)(t % H); t /= H;
  const int a = (int)(t % na);
  const long n = t / na;
  const float v = ly_ld1<T>(y + ((n * H + h) * W + w) * ldy + a * no + o);
  if constexpr (AUG) {
    if (p) p[i] = v;
  } else {
    p[i] = v;
  }
  if (z) {
    const float s = ly_sigmoid(v);
    float r = s;
    if (o == 0) r = (s * 2.f + ((float)w - 0.5f)) * stride;
    else if (o == 1) r = (s * 2.f + ((float)h - 0.5f)) * stride;
    else if (o == 2 || o == 3) { const float q = s * 2.f; r = q * q * (anchors[a * 2 + (o - 2)] * stride); }
    if constexpr (AUG) {
      if (o < 4) r = r / dscale;
      if (o == 0 && dflip) r = img_w - r;
    }
    z[(n * zrows + zoff + ((long)a * H + h) * W + w) * no + o] = r;
  }
}

template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_detect_tail_kernel(const T* __restrict__ y, int ldy, long total, int H, int W, int na, int no,
                                                                    const float* __restrict__ anchors /* [na,2] grid units */, float stride,
                                                                    float* __restrict__ p, float* __restrict__ z, long zrows, long zoff) {
  ly_detect_tail_body<T, false>(y, ldy, total, H, W, na, no, anchors, stride, p, z, zrows, zoff, 1.f, 0, 0.f);
}

template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_detect_tail_aug_kernel(const T* __restrict__ y, int ldy, long total, int H, int W, int na, int no,
                                                                        const float* __restrict__ anchors, float stride, float* __restrict__ p,
                                                                        float* __restrict__ z, long zrows, long zoff, float dscale, int dflip, float img_w) {
  ly_detect_tail_body<T, true>(y, ldy, total, H, W, na, no, anchors, stride, p, z, zrows, zoff, dscale, dflip, img_w);
}

extern "C" int ly_detect_tail(const void* y, int ldy, int n_img, int H, int W, int na, int no, const float* anchors, float stride,
                              float* p, float* z, long zrows, long zoff, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "detect_tail");
  LY_CHECK(y && p && anchors, "detect_tail: null pointer");
  const long total = (long)n_img * na * H * W * no;
  LY_WITH_T(dtype, hipLaunchKernelGGL(ly_detect_tail_kernel<T>, dim3((unsigned)((total + LY_THREADS - 1) / LY_THREADS)), dim3(LY_THREADS), 0,
                                      reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const T*>(y), ldy, total, H, W, na, no, anchors, stride, p, z, zrows, zoff));
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_detect_tail_aug(const void* y, int ldy, int n_img, int H, int W, int na, int no, const float* anchors, float stride,
                                  float* p, float* z, long zrows, long zoff, float dscale, int dflip, float img_w, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "detect_tail_aug");
  LY_CHECK(y && z && anchors && dscale > 0.f, "detect_tail_aug: null pointer / bad descale");
  const long total = (long)n_img * na * H * W * no;
  LY_WITH_T(dtype, hipLaunchKernelGGL(ly_detect_tail_aug_kernel<T>, dim3((unsigned)((total + LY_THREADS - 1) / LY_THREADS)), dim3(LY_THREADS), 0,
                                      reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const T*>(y), ldy, total, H, W, na, no, anchors, stride, p, z,
                                      zrows, zoff, dscale, dflip, img_w));
  LY_LAUNCH_CHECK();
  return 0;
}

// Adjoint of the raw-map permute above for the training step (models/yolo.py:88 `x[i].view(bs, na, no, ny, nx).permute(0, 1, 3, 4, 2)`):
// dp fp32 [n, na, H, W, no] -> du rows [n*H*W][ldu] of T (columns a*no + o, columns >= na*no zero: the operand of the head's dgrad /
// wgrad contractions), and dbias[a*no + o] += sum over pixels.  One launch instead of autograd's cast + two layout copies + zero-padded
// copy + a reduction.  A block walks (image, row) pairs: the na runs of W*no contiguous floats are staged in LDS, written back as
// whole rows, and the column sums are kept in registers until one atomic per column and block.
#define LY_DH_MAXW 160
#define LY_DH_MAXLD 32
#define LY_DH_TILE 12288                                   // floats of the LDS tile (48 KB): RB image rows of W pixels x (ldu + 1); >= MAXW * (MAXLD + 1)
// RB image rows per trip (as many as fit the tile, at most 8): one trip's loads are all in flight together — with one row per trip a block
// of the 80 x 80 level paid a dependent global -> LDS -> global round trip and two barriers per 5.6 KB — and the rows leave as 8-byte
// vectors (were 2-byte element stores).
template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_detect_head_bwd_kernel(const float* __restrict__ dp, int n_img, int H, int W, int na, int no,
                                                                        T* __restrict__ du, int ldu, float* __restrict__ dbias, const int f64, const int RB) {
  __shared__ float tile[LY_DH_TILE];
  __shared__ float red[LY_THREADS];
  const int tid = threadIdx.x, co = na * no, LT = ldu + 1;
  const int col = tid & 31, part = tid >> 5;              // column sums: 8 row classes x 32 columns
  float bsum = 0.f;
  for (int i = tid; i < RB * W * LT; i += LY_THREADS) tile[i] = 0.f;      // pad columns stay zero
  const long rows_total = (long)n_img * H;
  const int q4 = ldu >> 2;                                // 4-element groups of an output row (ldu % 4 == 0: checked by the launcher)
  for (long r0 = (long)blockIdx.x * RB; r0 < rows_total; r0 += (long)gridDim.x * RB) {
    const int nr = rows_total - r0 < RB ? (int)(rows_total - r0) : RB;
    __syncthreads();
    // one CELL (image row, anchor, pixel: `no` contiguous floats) per thread and step: its index arithmetic is done once, not per value (the
    // per-value form spent ~30 instructions of divisions on each 4-byte load: 43 us for the 80 x 80 level's 49 MB); no even: 8-byte loads
    const int cells = nr * na * W;
    for (int e = tid; e < cells; e += LY_THREADS) {
      const int rr = e / (na * W), e1 = e - rr * (na * W);
      const int a = e1 / W, w = e1 - a * W;
      const long r = r0 + rr;
      const long n = r / H;
      const int h = (int)(r - n * H);
      const float* const src = dp + ((((n * na + a) * H + h) * (long)W) + w) * no;
      float* const dst = tile + (rr * W + w) * LT + a * no;
      if ((no & 1) == 0) {
        for (int o = 0; o < no; o += 2) {
          const float2 v = *reinterpret_cast<const float2*>(src + o);
          dst[o] = v.x;
          dst[o + 1] = v.y;
        }
      } else {
        for (int o = 0; o < no; ++o) dst[o] = src[o];
      }
    }
    __syncthreads();
    T* const out = du + r0 * (long)W * ldu;               // the nr rows are contiguous in du
    for (int e = tid; e < nr * W * q4; e += LY_THREADS) {
      const int px = e / q4, g = e - px * q4;
      const float* t = tile + px * LT + 4 * g;
      ly_st4<T>(out + (long)px * ldu + 4 * g, (f32x4){t[0], t[1], t[2], t[3]});
    }
    if (col < co)
      for (int px = part; px < nr * W; px += LY_THREADS / 32) bsum += tile[px * LT + col];
  }
  red[tid] = bsum;
  __syncthreads();
  if (tid < 32 && tid < co) {
    float s = 0.f;
    for (int g = 0; g < LY_THREADS / 32; ++g) s += red[g * 32 + tid];
    ly_gacc(dbias, tid, s, f64);
  }
}

extern "C" int ly_detect_head_bwd(const float* dp, int n_img, int H, int W, int na, int no, void* du, int ldu, float* dbias, int dbias_f64, int dtype,
                                  void* stream) {
  LY_CHECK_DTYPE(dtype, "detect_head_bwd");
  LY_CHECK(dp && du && dbias && n_img > 0 && H > 0 && W > 0 && na > 0 && no > 0 && ((uintptr_t)dp & 7) == 0, "detect_head_bwd: bad arguments");
  LY_CHECK(W <= LY_DH_MAXW && ldu <= LY_DH_MAXLD && na * no <= ldu && (ldu & 3) == 0 && ((uintptr_t)du & 15) == 0,
           "detect_head_bwd: W=%d (max %d) / ldu=%d (max %d, >= na*no=%d, a multiple of 4) out of range", W, LY_DH_MAXW, ldu, LY_DH_MAXLD, na * no);
  int RB = LY_DH_TILE / (W * (ldu + 1));
  if (RB > 8) RB = 8;
  long blocks = ((long)n_img * H + RB - 1) / RB;
  if (blocks > 1024) blocks = 1024;
  LY_WITH_T(dtype, hipLaunchKernelGGL(ly_detect_head_bwd_kernel<T>, dim3((unsigned)blocks), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), dp,
                                      n_img, H, W, na, no, reinterpret_cast<T*>(du), ldu, dbias, dbias_f64, RB));
  LY_LAUNCH_CHECK();
  return 0;
}
