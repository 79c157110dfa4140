// Train-mode BatchNorm + activation of a conv -> BN -> act unit (models/common.py:1890-1910 under `scaler.scale(loss).backward()`, train.py:324),
// gfx950: activations / activation gradients T = float or __bf16, statistics and per-channel vectors fp32 or double.
//
//   ly_chan_moments                                   per-channel sum / sum of squares of an [rows, C] matrix (striped double accumulators)
//   ly_bn_finalize (+ _pair)                          striped sums -> batch mean / invstd, scale / shift, running-stat update
//   ly_bnact_fwd                                      y = act(a u + b): the elementwise pass after the contraction stored u
//   ly_bnact_bwd_reduce (+ _pair)                     sum dv, sum dv*u with dv = dy * act'(a u + b)
//   ly_bn_bwd_coeffs (+ _pair)                        those sums -> dgamma, dbeta and the affine map du = alpha dv + kappa + lambda u
//   ly_bnact_bwd_apply (+ _pair)                      du
// The _pair forms serve both halves of a cv1 || cv2 unit in one launch.
#include "ly_tile.hpp"
#include "ly_params.h"
// -------------------------------------------------------------------------------------------------
// BN(train)+activation backward.  Forward:  v = a[c]*u + b[c],  y = act(v).
//   reduce:  s1[c] = sum_r dv,  s2[c] = sum_r dv*u          with dv = dy * act'(v)
//   apply :  du = alpha[c]*dv + kappa[c] + lambda[c]*u      (coefficients built on the host from s1, s2:
//            the usual  gamma*invstd*(dv - mean(dv) - xhat*mean(dv*xhat))  written as an affine map of (dv, u))
// -------------------------------------------------------------------------------------------------
template <int ACT>
__device__ __forceinline__ f32x4 ly_dact4(const f32x4 v, const f32x4 dy) {
  f32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (ACT == LY_ACT_RELU) {
      r[i] = v[i] > 0.f ? dy[i] : 0.f;
    } else if (ACT == LY_ACT_SILU) {
      const float s = ly_sigmoid(v[i]);
      r[i] = dy[i] * s * (1.f + v[i] * (1.f - s));
    } else {
      r[i] = dy[i];
    }
  }
  return r;
}

// Row ranges per XCD for the streaming BatchNorm / activation passes: XCD x (= blockIdx.x % 8, round-robin dispatch) walks the x-th eighth of the
// items with its own blocks, so that a row is written / read by the XCD whose L2 the neighbouring tile kernels (ly_xcd_remap: contiguous
// tile ranges per XCD) use for the same rows.  (LY_XCD_STREAM=0 at build time: the plain grid-stride order.)
#ifndef LY_XCD_STREAM
#define LY_XCD_STREAM 1
#endif
#if LY_XCD_STREAM
#define LY_XCD_RANGE(total)                                                                                             \
  const bool xr_on = gridDim.x >= 8;                          /* fewer blocks than XCDs: an eighth would have no block */ \
  const long xr_x = blockIdx.x & 7, xr_slot = blockIdx.x >> 3, xr_n = ((long)gridDim.x + 7 - xr_x) >> 3;                  \
  const long xr_per = (((total) + 7) / 8 + LY_THREADS - 1) / LY_THREADS * LY_THREADS;                                      \
  const long xr_lo = xr_x * xr_per, xr_hi = xr_lo + xr_per < (total) ? xr_lo + xr_per : (total);                           \
  const long xr_begin = xr_on ? xr_lo + xr_slot * LY_THREADS + threadIdx.x : (long)blockIdx.x * LY_THREADS + threadIdx.x; \
  const long xr_end = xr_on ? xr_hi : (total), xr_step = (xr_on ? xr_n : (long)gridDim.x) * LY_THREADS
#else
#define LY_XCD_RANGE(total)                                                                                             \
  const long xr_begin = (long)blockIdx.x * LY_THREADS + threadIdx.x, xr_end = (total), xr_step = (long)gridDim.x * LY_THREADS
#endif

// The same split over ROWS for the kernels whose threads keep a fixed channel vector and walk rows (`groups` rows per block and trip): XCD x's
// blocks (slot s of n) take rows lo + s * groups + j, stepping by n * groups inside [lo, hi) = the x-th eighth of the rows.
#define LY_EW_UR 4
#define LY_XCD_ROWS(rows_, groups_)                                                                                     \
  const bool xw_on = gridDim.x >= 8;                                                                                      \
  const long xw_x = blockIdx.x & 7, xw_slot = blockIdx.x >> 3, xw_n = ((long)gridDim.x + 7 - xw_x) >> 3;                  \
  const long xw_per = ((rows_) + 7) / 8;                                                                                  \
  const long xw_lo = xw_on ? xw_x * xw_per : 0, xw_end = xw_on ? (xw_lo + xw_per < (rows_) ? xw_lo + xw_per : (rows_)) : (rows_); \
  const long xw_begin = xw_lo + (xw_on ? xw_slot : (long)blockIdx.x) * (groups_);                                         \
  const long xw_step = (xw_on ? xw_n : (long)gridDim.x) * (groups_)

template <typename T, int ACT>
__global__ __launch_bounds__(LY_THREADS) void ly_bnact_bwd_reduce_kernel(const T* __restrict__ dy, int lddy, const T* __restrict__ u,
                                                                          int ldu, long rows, int C, const float* __restrict__ a,
                                                                          const float* __restrict__ b, double* __restrict__ sums,
                                                                          const T* __restrict__ dy2, int lddy2, int csplit, double* __restrict__ sums2) {
  // (pair form, csplit < C: channels >= csplit take their gradient from dy2 — column c - csplit — and their sums go to sums2: the two
  // BatchNorms over one stacked pre-activation tensor, C3_CA's cv1 | cv2, in ONE pass; csplit == C: one unit)
  // thread = (channel quad, row lane).  Four rows per trip with all eight loads issued before the first use, in straight-line code
  // (a load under a run-time branch makes every later s_waitcnt conservative: the first unrolled version, which still chose the vector
  // width at run time, was SLOWER than one row per trip).  Rows past the end re-read the last row and are masked.
  __shared__ f32x4 red1[LY_THREADS], red2[LY_THREADS];
  using R4 = typename LyT<T>::R4;
  const int ncv = C >> 2, tid = threadIdx.x;
  const int groups = LY_THREADS / ncv;
  const int cv = tid % ncv, j0 = tid / ncv;
  f32x4 s1 = ly_zero4(), s2 = ly_zero4();
  const bool second = 4 * cv >= csplit;
  if (j0 < groups) {
    const f32x4 av = ly_ldg4(a + 4 * cv), bv = ly_ldg4(b + 4 * cv);
    constexpr int UR = 4;
    // round 6: rows walked in per-XCD ranges, as the forward / apply passes do (LY_XCD_ROWS: XCD x's blocks take the x-th eighth of the rows) —
    // dy was just written by a tile kernel whose tiles of these rows ran on the same XCD (ly_xcd_remap): with the plain grid-stride order every
    // row was fetched past the reading block's L2
    LY_XCD_ROWS(rows, groups);
    const long stride = xw_step;
    const T* const dyb = second ? dy2 + (4 * cv - csplit) : dy + 4 * cv;      // (a selected base pointer: no load under a branch)
    const long ldd = second ? lddy2 : lddy;
    for (long r0 = xw_begin + j0; r0 < xw_end; r0 += UR * stride) {
      R4 qu[UR], qg[UR];
#pragma unroll
      for (int k = 0; k < UR; ++k) {
        const long r = r0 + k * stride < xw_end ? r0 + k * stride : xw_end - 1;
        qu[k] = ly_ldr4<T>(u + r * ldu + 4 * cv);
        qg[k] = ly_ldr4<T>(dyb + r * ldd);
      }
#pragma unroll
      for (int k = 0; k < UR; ++k) {
        const f32x4 uu = ly_r4_f32(qu[k]);
        f32x4 dv = ly_dact4<ACT>(av * uu + bv, ly_r4_f32(qg[k]));
        if (!(r0 + k * stride < xw_end)) dv = ly_zero4();
        s1 += dv;
        s2 += dv * uu;
      }
    }
  }
  red1[tid] = s1;
  red2[tid] = s2;
  __syncthreads();
  if (j0 == 0) {
    const int ch = second ? C - csplit : csplit, lc = 4 * cv - (second ? csplit : 0);        // channels of this unit, the thread's first one in it
    double* sm = (second ? sums2 : sums) + (size_t)(blockIdx.x & (LY_STATS_STRIPES - 1)) * 2 * ch;      // double accumulators: see ly_stats_flush (ly_common.hpp)
    for (int g = 1; g < groups; ++g) { s1 += red1[g * ncv + cv]; s2 += red2[g * ncv + cv]; }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      atomicAdd(sm + lc + r, (double)s1[r]);
      atomicAdd(sm + ch + lc + r, (double)s2[r]);
    }
  }
}

template <typename T, int ACT>
__global__ __launch_bounds__(LY_THREADS) void ly_bnact_bwd_apply_kernel(const T* __restrict__ dy, int lddy, const T* u, int ldu,
                                                                         long rows, int C, const float* __restrict__ a,
                                                                         const float* __restrict__ b, const float* __restrict__ alpha,
                                                                         const float* __restrict__ kappa, const float* __restrict__ lambda,
                                                                         T* du, int lddu, const T* __restrict__ dy2, int lddy2, int csplit) {
  // 16-byte accesses in both dtypes (4 fp32 / 8 bf16 channels per thread) when C allows, else 4 channels
  // (pair form, csplit < C: channels >= csplit read their gradient from dy2, column c - csplit; csplit a multiple of the vector width)
  // Round 6: thread = (channel vector, row lane), as in the reduce pass — the five coefficient vectors of the thread's channels are loaded ONCE,
  // rows advance by a pointer stride, LY_EW_UR rows are in flight per trip.  (The first form walked a flat item index: a 64-bit division per
  // item and ten coefficient loads per trip were half of the loop's instructions — ~400 issue cycles of index arithmetic per 8 elements.)
  constexpr int VW = LyT<T>::VW, NQ = VW / 4;
  using RV = typename LyT<T>::RV;
  if ((C % VW) == 0 && (ldu % VW) == 0 && (lddy % VW) == 0 && (lddu % VW) == 0 && (lddy2 % VW) == 0 && (csplit % VW) == 0 && C / VW <= LY_THREADS) {
    const int ncv = C / VW, groups = LY_THREADS / ncv;
    const int cv = threadIdx.x % ncv, j0 = threadIdx.x / ncv;
    if (j0 >= groups) return;
    const int c = VW * cv;
    f32x4 ca[NQ], cb[NQ], cal[NQ], cka[NQ], cla[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      ca[q] = ly_ldg4(a + c + 4 * q); cb[q] = ly_ldg4(b + c + 4 * q);
      cal[q] = ly_ldg4(alpha + c + 4 * q); cka[q] = ly_ldg4(kappa + c + 4 * q); cla[q] = ly_ldg4(lambda + c + 4 * q);
    }
    LY_XCD_ROWS(rows, groups);
    const T* const gb = c >= csplit ? dy2 + (c - csplit) : dy + c;        // (a selected base pointer: no load under a branch)
    const long ldg = c >= csplit ? lddy2 : lddy;
    for (long r0 = xw_begin + j0; r0 < xw_end; r0 += LY_EW_UR * xw_step) {
      RV qu[LY_EW_UR], qg[LY_EW_UR];
#pragma unroll
      for (int k = 0; k < LY_EW_UR; ++k) {
        const long r = r0 + k * xw_step < xw_end ? r0 + k * xw_step : xw_end - 1;       // rows past the end re-read the last row (straight-line loads)
        qu[k] = ly_ldrv<T>(u + r * ldu + c);
        qg[k] = ly_ldrv<T>(gb + r * ldg);
      }
#pragma unroll
      for (int k = 0; k < LY_EW_UR; ++k) {
        f32x4 uu[NQ], g[NQ];
        ly_rv_unpack(qu[k], uu);
        ly_rv_unpack(qg[k], g);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const f32x4 dv = ly_dact4<ACT>(ca[q] * uu[q] + cb[q], g[q]);
          uu[q] = cal[q] * dv + cka[q] + cla[q] * uu[q];
        }
        const long r = r0 + k * xw_step;
        if (r < xw_end) *reinterpret_cast<RV*>(du + r * lddu + c) = ly_rv_pack(uu, (RV*)nullptr);
      }
    }
    return;
  }
  const int nc4 = C >> 2;
  const long total = rows * nc4;
  LY_XCD_RANGE(total);
  for (long i = xr_begin; i < xr_end; i += xr_step) {
    const long r = i / nc4;
    const int c = 4 * (int)(i - r * nc4);
    const f32x4 uu = ly_ld4<T>(u + r * ldu + c);
    const f32x4 g = ly_ld4<T>(c >= csplit ? dy2 + r * lddy2 + (c - csplit) : dy + r * lddy + c);
    const f32x4 dv = ly_dact4<ACT>(ly_ldg4(a + c) * uu + ly_ldg4(b + c), g);
    ly_st4<T>(du + r * lddu + c, ly_ldg4(alpha + c) * dv + ly_ldg4(kappa + c) + ly_ldg4(lambda + c) * uu);
  }
}

// y = act(a[c]*u + b[c]) over an [rows, C] matrix: the second half of a train-mode conv -> BN -> act unit whose
// contraction pass stored the pre-BN value u and accumulated its statistics in the same launch
template <typename T, int ACT>
__global__ __launch_bounds__(LY_THREADS) void ly_bnact_fwd_kernel(const T* __restrict__ u, int ldu, long rows, int C, const float* __restrict__ a,
                                                                   const float* __restrict__ b, T* __restrict__ y, int ldy) {
  constexpr int VW = LyT<T>::VW, NQ = VW / 4;
  using RV = typename LyT<T>::RV;
  if ((C % VW) == 0 && (ldu % VW) == 0 && (ldy % VW) == 0 && C / VW <= LY_THREADS) {
    // thread = (channel vector, row lane): scale / shift of the thread's channels in registers, LY_EW_UR rows in flight (see ly_bnact_bwd_apply_kernel)
    const int ncv = C / VW, groups = LY_THREADS / ncv;
    const int cv = threadIdx.x % ncv, j0 = threadIdx.x / ncv;
    if (j0 >= groups) return;
    const int c = VW * cv;
    f32x4 ca[NQ], cb[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) { ca[q] = ly_ldg4(a + c + 4 * q); cb[q] = ly_ldg4(b + c + 4 * q); }
    LY_XCD_ROWS(rows, groups);
    for (long r0 = xw_begin + j0; r0 < xw_end; r0 += LY_EW_UR * xw_step) {
      RV qu[LY_EW_UR];
#pragma unroll
      for (int k = 0; k < LY_EW_UR; ++k) {
        const long r = r0 + k * xw_step < xw_end ? r0 + k * xw_step : xw_end - 1;
        qu[k] = ly_ldrv<T>(u + r * ldu + c);
      }
#pragma unroll
      for (int k = 0; k < LY_EW_UR; ++k) {
        f32x4 uu[NQ];
        ly_rv_unpack(qu[k], uu);
#pragma unroll
        for (int q = 0; q < NQ; ++q) uu[q] = ly_act4(ca[q] * uu[q] + cb[q], ACT);
        const long r = r0 + k * xw_step;
        if (r < xw_end) *reinterpret_cast<RV*>(y + r * ldy + c) = ly_rv_pack(uu, (RV*)nullptr);
      }
    }
    return;
  }
  const int nc4 = C >> 2;
  const long total = rows * nc4;
  LY_XCD_RANGE(total);
  for (long i = xr_begin; i < xr_end; i += xr_step) {
    const long r = i / nc4;
    const int c = 4 * (int)(i - r * nc4);
    const f32x4 v = ly_ldg4(a + c) * ly_ld4<T>(u + r * ldu + c) + ly_ldg4(b + c);
    ly_st4<T>(y + r * ldy + c, ly_act4(v, ACT));
  }
}

// grid of the row-walking elementwise kernels (thread = channel vector x row lane, LY_EW_UR rows per trip): a whole number of trips per block
// (at most 8 x 256 blocks resident per XCD eighth), a multiple of 8 so that every XCD range has its blocks
static long ly_ew_row_blocks(long rows, int C, int vw) {
  const int ncv = C / vw;
  if (ncv <= 0 || ncv > LY_THREADS) return ly_ew_blocks(rows * (C >> 2));
  const long groups = LY_THREADS / ncv;
  const long trips = ((rows + 7) / 8 + groups * LY_EW_UR - 1) / (groups * LY_EW_UR);        // per XCD eighth
  const long per = (trips + 255) / 256;                                                       // trips per block
  const long bx = (trips + per - 1) / per;                                                    // blocks per eighth
  return 8 * (bx < 1 ? 1 : bx);
}

extern "C" int ly_bnact_fwd(const void* u_, int ldu, long rows, int C, const float* a, const float* b, int act, void* y_, int ldy, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "bnact_fwd");
  LY_CHECK(u_ && a && b && y_ && rows > 0, "bnact_fwd: null pointer");
  LY_CHECK((C & 3) == 0 && C > 0 && (ldu & 3) == 0 && (ldy & 3) == 0, "bnact_fwd: C=%d / ld must be multiples of 4", C);
  const int vw_ = dtype == LY_BF16 ? 8 : 4;
  const bool vec_ = (C % vw_) == 0 && (ldu % vw_) == 0 && (ldy % vw_) == 0 && C / vw_ <= LY_THREADS;
  const long blocks = vec_ ? ly_ew_row_blocks(rows, C, vw_) : ly_ew_blocks(rows * (C >> 2));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LY_WITH_T(dtype, {
    const T* u = reinterpret_cast<const T*>(u_);
    T* y = reinterpret_cast<T*>(y_);
    if (act == LY_ACT_SILU) hipLaunchKernelGGL((ly_bnact_fwd_kernel<T, LY_ACT_SILU>), dim3((unsigned)blocks), dim3(LY_THREADS), 0, st, u, ldu, rows, C, a, b, y, ldy);
    else if (act == LY_ACT_RELU) hipLaunchKernelGGL((ly_bnact_fwd_kernel<T, LY_ACT_RELU>), dim3((unsigned)blocks), dim3(LY_THREADS), 0, st, u, ldu, rows, C, a, b, y, ldy);
    else hipLaunchKernelGGL((ly_bnact_fwd_kernel<T, LY_ACT_NONE>), dim3((unsigned)blocks), dim3(LY_THREADS), 0, st, u, ldu, rows, C, a, b, y, ldy);
  });
  LY_LAUNCH_CHECK();
  return 0;
}

static int bnact_bwd_reduce_launch(const void* dy_, int lddy, const void* dy2_, int lddy2, int csplit, const void* u_, int ldu, long rows, int C, const float* a,
                                   const float* b, int act, double* sums, double* sums2, int dtype, void* stream) {
  // channels per thread: 4 in both dtypes.  (8 bf16 channels = 16-byte accesses measured SLOWER here, 24.6 -> 29.0 us per launch:
  // half as many threads share a row, and this pass lives on loads in flight; the elementwise apply / forward passes gain, 21 -> 18.6
  // and 14.6 -> 12.6 us, and use 16-byte accesses.)
  const int vw = 4;
  const int groups = LY_THREADS / (C / vw);
#ifndef LY_RED_ROWS
#define LY_RED_ROWS 32            // rows per row lane and block.  Measured round 6 (bnact family per step): 16 -> 1.83, 32 -> 1.78, 64 -> 1.96, 128 -> 2.31 ms
#endif
  long blocks = (rows + groups * (long)LY_RED_ROWS - 1) / (groups * (long)LY_RED_ROWS);
  blocks = blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks;
  if (blocks >= 8) blocks = (blocks + 7) / 8 * 8;           // every XCD eighth of the rows has its blocks (LY_XCD_ROWS)
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define LY_RED(A) hipLaunchKernelGGL((ly_bnact_bwd_reduce_kernel<T, A>), dim3((unsigned)blocks), dim3(LY_THREADS), 0, st, dy, lddy, u, ldu, rows, C, a, b, sums, dy2, lddy2, csplit, sums2)
  LY_WITH_T(dtype, {
    const T* dy = reinterpret_cast<const T*>(dy_);
    const T* dy2 = reinterpret_cast<const T*>(dy2_);
    const T* u = reinterpret_cast<const T*>(u_);
    if (act == LY_ACT_SILU) LY_RED(LY_ACT_SILU);
    else if (act == LY_ACT_RELU) LY_RED(LY_ACT_RELU);
    else LY_RED(LY_ACT_NONE);
  });
#undef LY_RED
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_bnact_bwd_reduce(const void* dy_, int lddy, const void* u_, int ldu, long rows, int C, const float* a, const float* b,
                                   int act, double* sums, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "bnact_bwd_reduce");
  LY_CHECK(dy_ && u_ && a && b && sums && rows > 0, "bnact_bwd_reduce: null pointer");
  LY_CHECK((C & 3) == 0 && C > 0 && C <= 1024 && (lddy & 3) == 0 && (ldu & 3) == 0, "bnact_bwd_reduce: C=%d / ld must be multiples of 4", C);
  return bnact_bwd_reduce_launch(dy_, lddy, dy_, lddy, C, u_, ldu, rows, C, a, b, act, sums, sums, dtype, stream);
}

// Two conv -> BN(train) -> act units over ONE stacked pre-activation tensor u [rows, C] (channels [0, csplit) and [csplit, C): C3_CA's cv1 | cv2,
// models/common.py:1630-1636) in one pass: unit 1's gradient dy1 [rows, csplit], unit 2's dy2 [rows, C - csplit]; sums1 / sums2 as `sums` of
// ly_bnact_bwd_reduce for csplit / C - csplit channels.
extern "C" int ly_bnact_bwd_reduce_pair(const void* dy1, int lddy1, const void* dy2, int lddy2, int csplit, const void* u_, int ldu, long rows, int C,
                                        const float* a, const float* b, int act, double* sums1, double* sums2, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "bnact_bwd_reduce_pair");
  LY_CHECK(dy1 && dy2 && u_ && a && b && sums1 && sums2 && rows > 0, "bnact_bwd_reduce_pair: null pointer");
  LY_CHECK((C & 3) == 0 && C > 0 && C <= 1024 && csplit > 0 && csplit < C && (csplit & 3) == 0 && (lddy1 & 3) == 0 && (lddy2 & 3) == 0 && (ldu & 3) == 0,
           "bnact_bwd_reduce_pair: C=%d csplit=%d / ld must be multiples of 4", C, csplit);
  return bnact_bwd_reduce_launch(dy1, lddy1, dy2, lddy2, csplit, u_, ldu, rows, C, a, b, act, sums1, sums2, dtype, stream);
}

static int bnact_bwd_apply_launch(const void* dy_, int lddy, const void* dy2_, int lddy2, int csplit, const void* u_, int ldu, long rows, int C, const float* a,
                                  const float* b, int act, const float* alpha, const float* kappa, const float* lambda, void* du_, int lddu, int dtype, void* stream) {
  const int vw_ = dtype == LY_BF16 ? 8 : 4;
  const bool vec_ = (C % vw_) == 0 && (ldu % vw_) == 0 && (lddy % vw_) == 0 && (lddu % vw_) == 0 && (lddy2 % vw_) == 0 && (csplit % vw_) == 0 && C / vw_ <= LY_THREADS;
  const long blocks = vec_ ? ly_ew_row_blocks(rows, C, vw_) : ly_ew_blocks(rows * (C >> 2));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define LY_APP(A) hipLaunchKernelGGL((ly_bnact_bwd_apply_kernel<T, A>), dim3((unsigned)blocks), dim3(LY_THREADS), 0, st, dy, lddy, u, ldu, rows, C, a, b, alpha, kappa, lambda, du, lddu, dy2, lddy2, csplit)
  LY_WITH_T(dtype, {
    const T* dy = reinterpret_cast<const T*>(dy_);
    const T* dy2 = reinterpret_cast<const T*>(dy2_);
    const T* u = reinterpret_cast<const T*>(u_);
    T* du = reinterpret_cast<T*>(du_);
    if (act == LY_ACT_SILU) LY_APP(LY_ACT_SILU);
    else if (act == LY_ACT_RELU) LY_APP(LY_ACT_RELU);
    else LY_APP(LY_ACT_NONE);
  });
#undef LY_APP
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_bnact_bwd_apply(const void* dy_, int lddy, const void* u_, int ldu, long rows, int C, const float* a, const float* b,
                                  int act, const float* alpha, const float* kappa, const float* lambda, void* du_, int lddu, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "bnact_bwd_apply");
  LY_CHECK(dy_ && u_ && a && b && alpha && kappa && lambda && du_ && rows > 0, "bnact_bwd_apply: null pointer");
  LY_CHECK((C & 3) == 0 && C > 0 && (lddy & 3) == 0 && (ldu & 3) == 0 && (lddu & 3) == 0, "bnact_bwd_apply: C=%d / ld must be multiples of 4", C);
  return bnact_bwd_apply_launch(dy_, lddy, dy_, lddy, C, u_, ldu, rows, C, a, b, act, alpha, kappa, lambda, du_, lddu, dtype, stream);
}

// the pair form (see ly_bnact_bwd_reduce_pair): du [rows, C] from dy1 | dy2, coefficient vectors of C entries (both units' side by side)
extern "C" int ly_bnact_bwd_apply_pair(const void* dy1, int lddy1, const void* dy2, int lddy2, int csplit, const void* u_, int ldu, long rows, int C,
                                       const float* a, const float* b, int act, const float* alpha, const float* kappa, const float* lambda, void* du_,
                                       int lddu, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "bnact_bwd_apply_pair");
  LY_CHECK(dy1 && dy2 && u_ && a && b && alpha && kappa && lambda && du_ && rows > 0, "bnact_bwd_apply_pair: null pointer");
  LY_CHECK((C & 3) == 0 && C > 0 && csplit > 0 && csplit < C && (csplit & 3) == 0 && (lddy1 & 3) == 0 && (lddy2 & 3) == 0 && (ldu & 3) == 0 && (lddu & 3) == 0,
           "bnact_bwd_apply_pair: C=%d csplit=%d / ld must be multiples of 4", C, csplit);
  return bnact_bwd_apply_launch(dy1, lddy1, dy2, lddy2, csplit, u_, ldu, rows, C, a, b, act, alpha, kappa, lambda, du_, lddu, dtype, stream);
}

// -------------------------------------------------------------------------------------------------
// Per-channel vector work of BatchNorm, one launch each (replaces ~10 tiny elementwise launches):
//   ly_bn_finalize   striped (sum, sum^2) accumulators -> batch mean / invstd, y = x*scale + shift, running-stat update
//   ly_bn_bwd_coeffs striped (sum dv, sum dv*u)        -> dgamma, dbeta and the affine map du = alpha*dv + kappa + lambda*u
// Sums over stripes and the mean / variance arithmetic are done in double (E[x^2] - E[x]^2 cancels badly in fp32).
// -------------------------------------------------------------------------------------------------
// One thread per channel: its stripes are 2 x `stripes` independent loads (all in flight together, coalesced over the channels of a wave) folded
// in stripe order, and every per-channel parameter is requested before the fold — one memory round trip per launch.  (The first form — a
// 32-lane group per channel and two double shuffle trees, parameters loaded after them — was a chain of ~25 dependent LDS-pipe and memory
// latencies: 4.4 us per launch, 79 launches per step.)
#define LY_BNV_THREADS 64
template <typename TS>
__device__ __forceinline__ void ly_fold_stripes(const TS* __restrict__ p, const int stripes, const size_t stride, const int second, double& s1, double& s2) {
  s1 = 0.0;
  s2 = 0.0;
  int q = 0;
  if (stripes == LY_STATS_STRIPES) {
    // the usual case: all 2 x 32 loads of the channel in flight together, folded in stripe order (in batches of eight the fold was four
    // dependent memory round trips: the atomics' results come from the memory side)
    TS a[LY_STATS_STRIPES], b[LY_STATS_STRIPES];
#pragma unroll
    for (int k = 0; k < LY_STATS_STRIPES; ++k) {
      a[k] = p[(size_t)k * stride];
      b[k] = p[(size_t)k * stride + second];
    }
#pragma unroll
    for (int k = 0; k < LY_STATS_STRIPES; ++k) {
      s1 += (double)a[k];
      s2 += (double)b[k];
    }
    return;
  }
  for (; q + 8 <= stripes; q += 8) {
    TS a[8], b[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      a[k] = p[(size_t)(q + k) * stride];
      b[k] = p[(size_t)(q + k) * stride + second];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      s1 += (double)a[k];
      s2 += (double)b[k];
    }
  }
  for (; q < stripes; ++q) {
    s1 += (double)p[(size_t)q * stride];
    s2 += (double)p[(size_t)q * stride + second];
  }
}

template <typename TS>
__global__ __launch_bounds__(LY_BNV_THREADS) void ly_bn_finalize_kernel(const TS* __restrict__ stats, int stripes, int nch, int c_off, int N,
                                                                    double count, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                    const float* __restrict__ bias, float eps, float momentum, float* running_mean,
                                                                    float* running_var, long* nbt, float* __restrict__ scale, float* __restrict__ shift,
                                                                    float* __restrict__ mean, float* __restrict__ invstd) {
  const int c = blockIdx.x * LY_BNV_THREADS + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x == 0 && nbt) *nbt += 1;
  if (c >= N) return;
  const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f, bi = bias ? bias[c] : 0.f;
  const float rm = running_mean ? running_mean[c] : 0.f, rv = running_var ? running_var[c] : 0.f;
  double s1, s2;
  ly_fold_stripes(stats + c_off + c, stripes, (size_t)2 * nch, nch, s1, s2);
  const double m = s1 / count;
  double var = s2 / count - m * m;
  var = var > 0.0 ? var : 0.0;
  const float is = (float)(1.0 / sqrt(var + (double)eps));
  const float sc = g * is;
  float sh = b - (float)m * sc;
  if (bias) sh += bi * sc;
  scale[c] = sc;
  shift[c] = sh;
  if (mean) mean[c] = (float)m;
  if (invstd) invstd[c] = is;
  if (running_mean) running_mean[c] = (1.f - momentum) * rm + momentum * (float)m;
  if (running_var) running_var[c] = (1.f - momentum) * rv + momentum * (float)(var * (count / (count > 1.0 ? count - 1.0 : 1.0)));
}

extern "C" int ly_bn_finalize(const void* stats, int stats_f64, int stripes, int nch, int c_off, int N, double count, const float* gamma, const float* beta,
                              const float* bias, float eps, float momentum, float* running_mean, float* running_var, long* nbt, float* scale,
                              float* shift, float* mean, float* invstd, void* stream) {
  LY_CHECK(stats && scale && shift && stripes > 0 && N > 0 && c_off >= 0 && c_off + N <= nch && count > 0, "bn_finalize: bad arguments");
  if (stats_f64)
    hipLaunchKernelGGL(ly_bn_finalize_kernel<double>, dim3((N + LY_BNV_THREADS - 1) / LY_BNV_THREADS), dim3(LY_BNV_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const double*>(stats), stripes, nch, c_off, N, count, gamma, beta, bias, eps, momentum, running_mean, running_var, nbt,
                       scale, shift, mean, invstd);
  else
    hipLaunchKernelGGL(ly_bn_finalize_kernel<float>, dim3((N + LY_BNV_THREADS - 1) / LY_BNV_THREADS), dim3(LY_BNV_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const float*>(stats), stripes, nch, c_off, N, count, gamma, beta, bias, eps, momentum, running_mean, running_var, nbt,
                       scale, shift, mean, invstd);
  LY_LAUNCH_CHECK();
  return 0;
}

// Two BatchNorms over one stacked output (ConvBnActPair: C3_CA's cv1 | cv2, channels [0, c_half) and [c_half, 2 c_half) of one
// statistics array) in ONE launch: every one of these coefficient kernels is a dependent ~4 us launch on the step's critical path.
struct LyBnSide {
  const float* gamma; const float* beta; float* running_mean; float* running_var; long* nbt; float eps, momentum;
};
template <typename TS>
__global__ __launch_bounds__(LY_BNV_THREADS) void ly_bn_finalize_pair_kernel(const TS* __restrict__ stats, int stripes, int c_half, double count, const LyBnSide u0,
                                                                         const LyBnSide u1, float* __restrict__ scale, float* __restrict__ shift,
                                                                         float* __restrict__ mean, float* __restrict__ invstd) {
  const int c = blockIdx.x * LY_BNV_THREADS + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 2) {
    long* nbt = threadIdx.x ? u1.nbt : u0.nbt;
    if (nbt) *nbt += 1;
  }
  const int nch = 2 * c_half;
  if (c >= nch) return;
  const bool hi = c >= c_half;
  const LyBnSide& U = hi ? u1 : u0;
  const int cl = hi ? c - c_half : c;
  const float g = U.gamma ? U.gamma[cl] : 1.f, b = U.beta ? U.beta[cl] : 0.f;
  const float rm = U.running_mean ? U.running_mean[cl] : 0.f, rv = U.running_var ? U.running_var[cl] : 0.f;
  double s1, s2;
  ly_fold_stripes(stats + c, stripes, (size_t)2 * nch, nch, s1, s2);
  const double m = s1 / count;
  double var = s2 / count - m * m;
  var = var > 0.0 ? var : 0.0;
  const float is = (float)(1.0 / sqrt(var + (double)U.eps));
  const float sc = g * is;
  scale[c] = sc;
  shift[c] = b - (float)m * sc;
  mean[c] = (float)m;
  invstd[c] = is;
  if (U.running_mean) U.running_mean[cl] = (1.f - U.momentum) * rm + U.momentum * (float)m;
  if (U.running_var) U.running_var[cl] = (1.f - U.momentum) * rv + U.momentum * (float)(var * (count / (count > 1.0 ? count - 1.0 : 1.0)));
}

extern "C" int ly_bn_finalize_pair(const void* stats, int stats_f64, int stripes, int c_half, double count, const float* gamma0, const float* beta0, float eps0,
                                   float momentum0, float* running_mean0, float* running_var0, long* nbt0, const float* gamma1, const float* beta1,
                                   float eps1, float momentum1, float* running_mean1, float* running_var1, long* nbt1, float* scale, float* shift,
                                   float* mean, float* invstd, void* stream) {
  LY_CHECK(stats && scale && shift && mean && invstd && stripes > 0 && c_half > 0 && count > 0, "bn_finalize_pair: bad arguments");
  const LyBnSide u0 = {gamma0, beta0, running_mean0, running_var0, nbt0, eps0, momentum0}, u1 = {gamma1, beta1, running_mean1, running_var1, nbt1, eps1, momentum1};
  const dim3 grid((2 * c_half + LY_BNV_THREADS - 1) / LY_BNV_THREADS);
  if (stats_f64)
    hipLaunchKernelGGL(ly_bn_finalize_pair_kernel<double>, grid, dim3(LY_BNV_THREADS), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const double*>(stats),
                       stripes, c_half, count, u0, u1, scale, shift, mean, invstd);
  else
    hipLaunchKernelGGL(ly_bn_finalize_pair_kernel<float>, grid, dim3(LY_BNV_THREADS), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const float*>(stats),
                       stripes, c_half, count, u0, u1, scale, shift, mean, invstd);
  LY_LAUNCH_CHECK();
  return 0;
}

// the backward coefficients of the same two units: sums0 / sums1 are the two striped arrays of ly_bnact_bwd_reduce_pair ([stripes][2 c_half]
// each), a / mean / invstd and alpha / kappa / lambda the stacked [2 c_half] vectors, dgamma / dbeta per unit (ACCUMULATED, as below)
template <typename TS>
__global__ __launch_bounds__(LY_BNV_THREADS) void ly_bn_bwd_coeffs_pair_kernel(const TS* __restrict__ sums0, const TS* __restrict__ sums1, int stripes, int c_half,
                                                                           double count, const float* __restrict__ a, const float* __restrict__ mean,
                                                                           const float* __restrict__ invstd, float* __restrict__ dgamma0,
                                                                           float* __restrict__ dbeta0, float* __restrict__ dgamma1, float* __restrict__ dbeta1,
                                                                           float* __restrict__ alpha, float* __restrict__ kappa, float* __restrict__ lambda) {
  const int c = blockIdx.x * LY_BNV_THREADS + threadIdx.x;
  if (c >= 2 * c_half) return;
  const bool hi = c >= c_half;
  const int cl = hi ? c - c_half : c;
  float* const dgamma = hi ? dgamma1 : dgamma0;
  float* const dbeta = hi ? dbeta1 : dbeta0;
  const double mu = mean[c], is = invstd[c], av = a[c];
  const float dg0 = dgamma[cl], db0 = dbeta[cl];
  double s1, s2;
  ly_fold_stripes((hi ? sums1 : sums0) + cl, stripes, (size_t)2 * c_half, c_half, s1, s2);
  const double dg = (s2 - mu * s1) * is;
  dgamma[cl] = dg0 + (float)dg;
  dbeta[cl] = db0 + (float)s1;
  alpha[c] = (float)av;
  const double lam = -av * dg * is / count;
  lambda[c] = (float)lam;
  kappa[c] = (float)(-av * s1 / count - lam * mu);
}

extern "C" int ly_bn_bwd_coeffs_pair(const void* sums0, const void* sums1, int sums_f64, int stripes, int c_half, double count, const float* a, const float* mean,
                                     const float* invstd, float* dgamma0, float* dbeta0, float* dgamma1, float* dbeta1, float* alpha, float* kappa,
                                     float* lambda, void* stream) {
  LY_CHECK(sums0 && sums1 && a && mean && invstd && dgamma0 && dbeta0 && dgamma1 && dbeta1 && alpha && kappa && lambda && c_half > 0 && count > 0 && stripes > 0,
           "bn_bwd_coeffs_pair: bad arguments");
  const dim3 grid((2 * c_half + LY_BNV_THREADS - 1) / LY_BNV_THREADS);
  if (sums_f64)
    hipLaunchKernelGGL(ly_bn_bwd_coeffs_pair_kernel<double>, grid, dim3(LY_BNV_THREADS), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const double*>(sums0),
                       reinterpret_cast<const double*>(sums1), stripes, c_half, count, a, mean, invstd, dgamma0, dbeta0, dgamma1, dbeta1, alpha, kappa, lambda);
  else
    hipLaunchKernelGGL(ly_bn_bwd_coeffs_pair_kernel<float>, grid, dim3(LY_BNV_THREADS), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const float*>(sums0),
                       reinterpret_cast<const float*>(sums1), stripes, c_half, count, a, mean, invstd, dgamma0, dbeta0, dgamma1, dbeta1, alpha, kappa, lambda);
  LY_LAUNCH_CHECK();
  return 0;
}

template <typename TS>
__global__ __launch_bounds__(LY_BNV_THREADS) void ly_bn_bwd_coeffs_kernel(const TS* __restrict__ sums, int stripes, int N, double count,
                                                                      const float* __restrict__ a, const float* __restrict__ mean,
                                                                      const float* __restrict__ invstd, int train, float* __restrict__ dgamma,
                                                                      float* __restrict__ dbeta, float* __restrict__ alpha, float* __restrict__ kappa,
                                                                      float* __restrict__ lambda, const int tr_a, const int tr_b) {
  const int c = blockIdx.x * LY_BNV_THREADS + threadIdx.x;
  if (c >= N) return;
  // tr_a > 0: the sums are in [tr_a][tr_b] order (RFCBAMConv's generate BatchNorm: [tap][channel]) and dgamma / dbeta are the parameter's own
  // [tr_b][tr_a] storage — the transpose rides on the accumulation instead of two copies + two adds per layer
  const int cd = tr_a > 0 ? (c % tr_b) * tr_a + c / tr_b : c;
  const double mu = mean[c], is = invstd[c], av = a[c];
  const float dg0 = dgamma[cd], db0 = dbeta[cd];
  double s1, s2;
  ly_fold_stripes(sums + c, stripes, (size_t)2 * N, N, s1, s2);
  const double dg = (s2 - mu * s1) * is;
  dgamma[cd] = dg0 + (float)dg;    // ACCUMULATED: the targets may be the parameters' persistent .grad storage (zeroed by the optimiser step)
  dbeta[cd] = db0 + (float)s1;
  alpha[c] = (float)av;
  if (train) {
    const double lam = -av * dg * is / count;
    lambda[c] = (float)lam;
    kappa[c] = (float)(-av * s1 / count - lam * mu);
  } else {
    lambda[c] = 0.f;
    kappa[c] = 0.f;
  }
}

extern "C" int ly_bn_bwd_coeffs(const void* sums, int sums_f64, int stripes, int N, double count, const float* a, const float* mean, const float* invstd,
                                int train, float* dgamma, float* dbeta, float* alpha, float* kappa, float* lambda, int tr_a, int tr_b, void* stream) {
  LY_CHECK(sums && a && mean && invstd && dgamma && dbeta && alpha && kappa && lambda && N > 0 && count > 0, "bn_bwd_coeffs: bad arguments");
  LY_CHECK(tr_a == 0 || (tr_a > 0 && tr_b > 0 && tr_a * tr_b == N), "bn_bwd_coeffs: transposed targets need tr_a * tr_b == N");
  if (sums_f64)
    hipLaunchKernelGGL(ly_bn_bwd_coeffs_kernel<double>, dim3((N + LY_BNV_THREADS - 1) / LY_BNV_THREADS), dim3(LY_BNV_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const double*>(sums), stripes, N, count, a, mean, invstd, train, dgamma, dbeta, alpha, kappa, lambda, tr_a, tr_b);
  else
    hipLaunchKernelGGL(ly_bn_bwd_coeffs_kernel<float>, dim3((N + LY_BNV_THREADS - 1) / LY_BNV_THREADS), dim3(LY_BNV_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const float*>(sums), stripes, N, count, a, mean, invstd, train, dgamma, dbeta, alpha, kappa, lambda, tr_a, tr_b);
  LY_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------
// Train-mode BatchNorm support kernels (statistics passes; normalisation itself is folded into the
// consumers' scale/shift exactly like the eval path)
// ---------------------------------------------------------------------------------------------------
// per-channel sum / sum of squares over all rows of an [rows, C] matrix: mom[c] += sum x, mom[C + c] += sum x^2
template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_chan_moments_kernel(const T* __restrict__ x, int ldx, long rows, int C,
                                                                      double* __restrict__ mom) {
  __shared__ f32x4 red1[LY_THREADS], red2[LY_THREADS];
  const int nc4 = C >> 2, tid = threadIdx.x;
  const int groups = LY_THREADS / nc4;
  const int c4 = tid % nc4, j0 = tid / nc4;
  f32x4 s1 = ly_zero4(), s2 = ly_zero4();
  if (j0 < groups) {
    // four rows per trip, all four loads issued before the first use (one row per trip paid a round trip per row: 21 us for the 8 MB of
    // RFCBAMConv layer 9's input, on 67 blocks); rows past the end re-read the last row and are masked
    const long step = (long)gridDim.x * groups;
    for (long r = (long)blockIdx.x * groups + j0; r < rows; r += 4 * step) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long rr = r + u * step;
        v[u] = ly_ld4<T>(x + (rr < rows ? rr : rows - 1) * ldx + 4 * c4);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const f32x4 w = r + u * step < rows ? v[u] : ly_zero4();
        s1 += w;
        s2 += w * w;
      }
    }
  }
  red1[tid] = s1; red2[tid] = s2;
  __syncthreads();
  if (j0 == 0) {
    for (int g = 1; g < groups; ++g) { s1 += red1[g * nc4 + c4]; s2 += red2[g * nc4 + c4]; }
    double* m = mom + (size_t)(blockIdx.x & (LY_STATS_STRIPES - 1)) * 2 * C;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      atomicAdd(m + 4 * c4 + r, (double)s1[r]);
      atomicAdd(m + C + 4 * c4 + r, (double)s2[r]);
    }
  }
}

extern "C" int ly_chan_moments(const void* x, int ldx, long rows, int C, double* mom, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "chan_moments");
  LY_CHECK(x && mom && (C & 3) == 0 && (ldx & 3) == 0 && C <= 1024 && rows > 0, "chan_moments: bad arguments");
  const int groups = LY_THREADS / (C >> 2);
  long blocks = (rows + groups * 16L - 1) / (groups * 16L);    // ~16 rows per row group: four trips of four rows in flight
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  LY_WITH_T(dtype, hipLaunchKernelGGL(ly_chan_moments_kernel<T>, dim3((unsigned)blocks), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                                      reinterpret_cast<const T*>(x), ldx, rows, C, mom));
  LY_LAUNCH_CHECK();
  return 0;
}
