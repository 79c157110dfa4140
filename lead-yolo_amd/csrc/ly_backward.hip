// Backward building blocks of the training step, gfx950; activations / activation gradients T = float or
// __bf16, BatchNorm sums and attention-table gradients fp32.
//
//   ly_bnact_bwd_reduce / ly_bnact_bwd_apply   BatchNorm(train) + activation backward on an [rows, C] matrix
//   ly_up2_bwd, ly_unpatch2                    adjoints of the nearest-2x read and of the k=s=2 patch gather
//
// The weight gradients (ly_wgrad: contraction over PIXELS with the forward's gather) are in ly_wgrad.hip.
// Data gradients (dgrad) of the 1x1 / 3x3 convolutions reuse the forward contraction kernels
// (ly_gemm_fwd / ly_conv3x3_fwd) with transposed, frag-packed weights: the adjoint of a stride-1
// convolution is a stride-1 convolution.
//
// Replaces what autograd derives for Conv2d -> BatchNorm2d -> SiLU/ReLU in the reference's
// `scaler.scale(loss).backward()` (train.py:324) over models/common.py:1890-1910 (Conv),
// :1478-1482 (MLPBlock), :1537-1561 (patch layers).
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

static long ly_ew_blocks(long items) {
  long b = (items + LY_THREADS * 4L - 1) / (LY_THREADS * 4L);
  return b < 1 ? 1 : b > 4096 ? 4096 : b;
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
// Adjoint of the nearest-2x upsampled read (nn.Upsample(2,'nearest'), models/LEAD-YOLO.yaml neck):
//   dsrc[n, h, w, :] = sum of the four dst pixels (2h+{0,1}, 2w+{0,1})
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_up2_bwd_kernel(const T* __restrict__ d, int ldd, int n_img, int Hs, int Ws, int C,
                                                                T* __restrict__ o, int ldo) {
  const int nc4 = C >> 2;
  const long total = (long)n_img * Hs * Ws * nc4;
  for (long i = (long)blockIdx.x * LY_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * LY_THREADS) {
    const long pix = i / nc4;
    const int c = 4 * (int)(i - pix * nc4);
    const long row = pix / Ws;
    const int w = (int)(pix - row * Ws);
    const long n = row / Hs;
    const int h = (int)(row - n * Hs);
    const T* s = d + (((n * 2 * Hs + 2 * h) * 2L * Ws) + 2 * w) * ldd + c;
    const f32x4 v = ly_ld4<T>(s) + ly_ld4<T>(s + ldd) + ly_ld4<T>(s + 2L * Ws * ldd) + ly_ld4<T>(s + 2L * Ws * ldd + ldd);
    ly_st4<T>(o + pix * ldo + c, v);
  }
}

extern "C" int ly_up2_bwd(const void* d, int ldd, int n_img, int Hs, int Ws, int C, void* out, int ldo, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "up2_bwd");
  LY_CHECK(d && out && n_img > 0 && Hs > 0 && Ws > 0 && (C & 3) == 0 && (ldd & 3) == 0 && (ldo & 3) == 0, "up2_bwd: bad arguments");
  LY_WITH_T(dtype, hipLaunchKernelGGL(ly_up2_bwd_kernel<T>, dim3((unsigned)ly_ew_blocks((long)n_img * Hs * Ws * (C >> 2))), dim3(LY_THREADS), 0,
                                      reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const T*>(d), ldd, n_img, Hs, Ws, C, reinterpret_cast<T*>(out), ldo));
  LY_LAUNCH_CHECK();
  return 0;
}

// -------------------------------------------------------------------------------------------------
// Adjoint of the k = s = 2 patch gather (PatchMerging_FasterNet, models/common.py:1555-1561): the dgrad GEMM
// produces g[m = (n, ho, wo)][(ky, kx, c)]; scatter it to dx[n, 2ho+ky, 2wo+kx, c] (every input pixel belongs
// to exactly one patch).
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_unpatch_kernel(const T* __restrict__ g, int n_img, int Ho, int Wo, int C, int ks,
                                                                T* __restrict__ dx) {
  const int nc4 = C >> 2;
  const int kc = ks * ks * nc4;
  const long total = (long)n_img * Ho * Wo * kc;
  for (long i = (long)blockIdx.x * LY_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * LY_THREADS) {
    const long m = i / kc;
    int r = (int)(i - m * kc);
    const int tap = r / nc4;
    const int c = 4 * (r - tap * nc4);
    const int ky = tap / ks, kx = tap - ky * ks;
    const long row = m / Wo;
    const int wo = (int)(m - row * Wo);
    const long n = row / Ho;
    const int ho = (int)(row - n * Ho);
    const long dst = ((n * Ho * ks + (long)ho * ks + ky) * ((long)Wo * ks) + (long)wo * ks + kx) * C + c;
    ly_st4<T>(dx + dst, ly_ld4<T>(g + m * ((long)ks * ks * C) + (long)tap * C + c));
  }
}

// -------------------------------------------------------------------------------------------------
// dst[c] (+)= sum_r src[r][c]: the partial-row buffers of the backward (per-block generate weight gradients, per-group conv weight
// gradients, per-chunk d_rfa slabs, moment slices) folded deterministically — fixed order, no atomics.  Block = 64 columns x 16 row lanes;
// a row lane walks rows lane, lane + 16, ... with four loads in flight.  (Was `tensor.sum(0)`: ATen's multi-block reduction keeps scratch
// state of its own, and a captured instance returned wrong sums once the same reduction had also run eagerly in the process.)
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void ly_sum_rows_kernel(const float* __restrict__ src, const long R, const long C, const long ld,
                                                          float* __restrict__ dst, const int accumulate, const int rls) {
  __shared__ float red[16][64];                            // rls row lanes (4 for R <= 192, else 16: see ly_wgrad_fold)
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const long c = (long)blockIdx.x * 64 + cl;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (c < C) {
    const float* p = src + c;
    long r = rl;
    for (; r + 7 * rls < R; r += 8 * rls) {             // eight loads fenced ahead of the adds
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = p[(r + rls * k) * ld];
      __builtin_amdgcn_sched_barrier(0);
      a0 += v[0]; a1 += v[1]; a2 += v[2]; a3 += v[3];
      a0 += v[4]; a1 += v[5]; a2 += v[6]; a3 += v[7];
    }
    for (; r + 3 * rls < R; r += 4 * rls) {
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = p[(r + rls * k) * ld];
      __builtin_amdgcn_sched_barrier(0);
      a0 += v[0]; a1 += v[1]; a2 += v[2]; a3 += v[3];
    }
    for (; r < R; r += rls) a0 += p[r * ld];
  }
  red[rl][cl] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (rl == 0 && c < C) {
    float s = 0.f;
    for (int i = 0; i < rls; ++i) s += red[i][cl];
    dst[c] = accumulate ? dst[c] + s : s;
  }
}

extern "C" int ly_sum_rows(const float* src, long R, long C, long ld, float* dst, int accumulate, void* stream) {
  LY_CHECK(src && dst && R > 0 && C > 0 && ld >= C, "sum_rows: bad arguments");
  LY_CHECK((C + 63) / 64 < (1L << 31), "sum_rows: too many columns");
  const int rls = R <= 192 ? 4 : 16;
  hipLaunchKernelGGL(ly_sum_rows_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64 * rls), 0, reinterpret_cast<hipStream_t>(stream), src, R, C, ld, dst,
                     accumulate, rls);
  LY_LAUNCH_CHECK();
  return 0;
}

// column sums of a small [R][C] matrix of doubles (the stripes of a double statistics accumulator), rows added in index order
__global__ __launch_bounds__(LY_THREADS) void ly_sum_rows_f64_kernel(const double* __restrict__ src, const int R, const int C, double* __restrict__ dst) {
  const int c = blockIdx.x * LY_THREADS + threadIdx.x;
  if (c >= C) return;
  double a = 0.0;
  for (int r = 0; r < R; ++r) a += src[(long)r * C + c];
  dst[c] = a;
}
// dst[i] += (float)src[i] for up to LY_F64_ADD_MAX small vectors in one launch (the double scratches of ly_gacc, ly_common.hpp)
__global__ __launch_bounds__(LY_THREADS) void ly_f64_add_kernel(const LyF64AddTable T) {
  const int e = blockIdx.y;
  const int i = blockIdx.x * LY_THREADS + threadIdx.x;
  if (e < T.count && i < T.n[e]) T.dst[e][i] += (float)T.src[e][i];
}
extern "C" int ly_f64_add(const LyF64AddTable* t, void* stream) {
  LY_CHECK(t && t->count > 0 && t->count <= LY_F64_ADD_MAX, "f64_add: bad table");
  int nmax = 0;
  for (int e = 0; e < t->count; ++e) {
    LY_CHECK(t->src[e] && t->dst[e] && t->n[e] > 0, "f64_add: entry %d is empty", e);
    nmax = t->n[e] > nmax ? t->n[e] : nmax;
  }
  hipLaunchKernelGGL(ly_f64_add_kernel, dim3((unsigned)((nmax + LY_THREADS - 1) / LY_THREADS), (unsigned)t->count), dim3(LY_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), *t);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_sum_rows_f64(const double* src, int R, int C, double* dst, void* stream) {
  LY_CHECK(src && dst && R > 0 && C > 0, "sum_rows_f64: bad arguments");
  hipLaunchKernelGGL(ly_sum_rows_f64_kernel, dim3((unsigned)((C + LY_THREADS - 1) / LY_THREADS)), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), src,
                     R, C, dst);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_unpatch(const void* g, int n_img, int Ho, int Wo, int C, int ks, void* dx, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "unpatch");
  LY_CHECK(g && dx && n_img > 0 && Ho > 0 && Wo > 0 && ks > 0 && (C & 3) == 0, "unpatch: bad arguments");
  LY_WITH_T(dtype, hipLaunchKernelGGL(ly_unpatch_kernel<T>, dim3((unsigned)ly_ew_blocks((long)n_img * Ho * Wo * ks * ks * (C >> 2))), dim3(LY_THREADS), 0,
                                      reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const T*>(g), n_img, Ho, Wo, C, ks, reinterpret_cast<T*>(dx)));
  LY_LAUNCH_CHECK();
  return 0;
}

// -------------------------------------------------------------------------------------------------
// Space-to-depth of the uint8 NCHW image for PatchEmbed's weight gradient (models/common.py:1537-1550, k = s = 4): rows[m][(c, ky, kx)]
// = the integer pixel values as T (exact in bf16), so that ly_wgrad contracts plain rows; the caller applies 1/255 to the small dw.
// Block = 64 patches of one patch row: coalesced 4-byte loads (the 4 kx of a patch) staged through LDS, 16-byte row stores
// (was: a permuted torch copy + a cast, 250 us at bs=64 640x640; one pass at the copy rate now).
// -------------------------------------------------------------------------------------------------
#define LY_P4_WO 64
template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_patch4_rows_u8_kernel(const unsigned char* __restrict__ img, int C, int H, int W, T* __restrict__ rows) {
  extern __shared__ f32x4 ly_p4_smem[];
  T* const tile = reinterpret_cast<T*>(ly_p4_smem);
  const int Wo = W >> 2, Ho = H >> 2;
  const int K = 16 * C, KP = K + 8;                       // padded LDS row
  const int wo0 = blockIdx.x * LY_P4_WO;
  const int n = blockIdx.y / Ho, ho = blockIdx.y - n * Ho;
  const int nw = Wo - wo0 < LY_P4_WO ? Wo - wo0 : LY_P4_WO;
  for (int i = threadIdx.x; i < 4 * C * LY_P4_WO; i += LY_THREADS) {
    const int wl = i & (LY_P4_WO - 1), r = i / LY_P4_WO;  // r = c * 4 + ky
    const int c = r >> 2, ky = r & 3;
    const int wc = wl < nw ? wl : nw - 1;
    const unsigned v = *reinterpret_cast<const unsigned*>(img + (((long)n * C + c) * H + 4 * ho + ky) * W + 4 * (wo0 + wc));
    T* d = tile + wl * KP + 4 * r;
    d[0] = (T)(float)(v & 255u); d[1] = (T)(float)((v >> 8) & 255u); d[2] = (T)(float)((v >> 16) & 255u); d[3] = (T)(float)(v >> 24);
  }
  __syncthreads();
  constexpr int VE = 16 / sizeof(T);                       // elements per 16-byte store
  const int vpr = K / VE;
  T* const out = rows + ((long)blockIdx.y * Wo + wo0) * K;
  for (int j = threadIdx.x; j < nw * vpr; j += LY_THREADS) {
    const int wl = j / vpr, q = j - wl * vpr;
    *reinterpret_cast<f32x4*>(out + (long)wl * K + q * VE) = *reinterpret_cast<const f32x4*>(tile + wl * KP + q * VE);
  }
}

extern "C" int ly_patch4_rows_u8(const unsigned char* img, int n_img, int C, int H, int W, void* rows, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "patch4_rows_u8");
  LY_CHECK(img && rows && n_img > 0 && C > 0 && C <= 16 && H > 0 && W > 0 && (H & 3) == 0 && (W & 3) == 0, "patch4_rows_u8: bad arguments");
  LY_CHECK(((uintptr_t)img & 3) == 0 && ((uintptr_t)rows & 15) == 0, "patch4_rows_u8: unaligned pointer");
  LY_CHECK((long)n_img * (H >> 2) < 65536, "patch4_rows_u8: too many patch rows");
  const dim3 grid((unsigned)(((W >> 2) + LY_P4_WO - 1) / LY_P4_WO), (unsigned)(n_img * (H >> 2)));
  LY_WITH_T(dtype, hipLaunchKernelGGL(ly_patch4_rows_u8_kernel<T>, grid, dim3(LY_THREADS), (size_t)LY_P4_WO * (16 * C + 8) * sizeof(T),
                                      reinterpret_cast<hipStream_t>(stream), img, C, H, W, reinterpret_cast<T*>(rows)));
  LY_LAUNCH_CHECK();
  return 0;
}

// -------------------------------------------------------------------------------------------------
// CoordAtt (models/common.py:1595-1609) backward pieces.
//   gate:  out = x * a_h[n,h,:] * a_w[n,w,:]
//          dx = dout*a_h*a_w,  da_h[n,h,c] = sum_w dout*x*a_w,  da_w[n,w,c] = sum_h dout*x*a_h
//   pools: pool[n, 0:H, c] = mean_w x,  pool[n, H:H+W, c] = mean_h x
//          dx[n,h,w,c] = gp[n,h,c]/W + gp[n,H+w,c]/H
// One block per (image, row h): da_h is reduced in the block, da_w (zeroed by the caller) by float atomics.
// -------------------------------------------------------------------------------------------------
// One block per (image, band of RB rows): da_h is reduced per row in the block; the da_w contributions of the band's rows are
// summed in registers (a thread owns a fixed set of (w, channel quad) pairs) and added with ONE float atomic per element and
// band instead of one per element and row.
#define LY_CAG_RB 8
#define LY_CAG_MAXW 8        // (w, c4) pairs per thread: ceil(W / groups) <= 8
template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_coordatt_gate_bwd_kernel(const T* __restrict__ dout, int ldd, const T* __restrict__ x,
                                                                           int ldx, int H, int W, int C, const float* __restrict__ a_h,
                                                                           const float* __restrict__ a_w, T* __restrict__ dx, int lddx,
                                                                           float* __restrict__ da_h, float* __restrict__ da_w, int bands, int slabs, long n_img) {
  __shared__ f32x4 red[LY_THREADS];
  const int nc4 = C >> 2, tid = threadIdx.x;
  const int groups = LY_THREADS / nc4;
  const int c4 = tid % nc4, g0 = tid / nc4;
  const int slab = blockIdx.x % slabs;                       // column slab of groups * LY_CAG_MAXW columns
  const int bb = blockIdx.x / slabs;
  const long n = bb / bands;
  const int band = bb - (int)n * bands;
  const int w0 = slab * groups * LY_CAG_MAXW;
  const int h_lo = band * LY_CAG_RB, h_hi = h_lo + LY_CAG_RB < H ? h_lo + LY_CAG_RB : H;
  f32x4 accw[LY_CAG_MAXW], aw[LY_CAG_MAXW];
  bool okw[LY_CAG_MAXW];
  int wcl[LY_CAG_MAXW];
  // the thread's columns are the same for every row of the band: their a_w factors are loaded once; per row all 16 row loads are issued from
  // clamped addresses before the first use (they sat under a per-column branch: one exposed round trip per column)
  const bool gok = g0 < groups;
#pragma unroll
  for (int i = 0; i < LY_CAG_MAXW; ++i) {
    accw[i] = ly_zero4();
    const int w = w0 + g0 + i * groups;
    okw[i] = gok && w < W;
    wcl[i] = okw[i] ? w : (w0 < W ? w0 : 0);
    aw[i] = ly_ldg4(a_w + (n * W + wcl[i]) * C + 4 * (gok ? c4 : 0));
  }
  using R4 = typename LyT<T>::R4;
  for (int h = h_lo; h < h_hi; ++h) {
    const long nh = n * H + h;
    f32x4 sh = ly_zero4();
    {
      const int c4c = gok ? c4 : 0;
      const f32x4 ah = ly_ldg4(a_h + nh * C + 4 * c4c);
      R4 dr[LY_CAG_MAXW], xr[LY_CAG_MAXW];
#pragma unroll
      for (int i = 0; i < LY_CAG_MAXW; ++i) {
        const long row = nh * W + wcl[i];
        dr[i] = ly_ldr4<T>(dout + row * ldd + 4 * c4c);
        xr[i] = ly_ldr4<T>(x + row * ldx + 4 * c4c);
      }
#pragma unroll
      for (int i = 0; i < LY_CAG_MAXW; ++i) {
        if (okw[i]) {
          const long row = nh * W + wcl[i];
          const f32x4 d = ly_r4_f32(dr[i]), xv = ly_r4_f32(xr[i]);
          ly_st4<T>(dx + row * lddx + 4 * c4, d * ah * aw[i]);
          const f32x4 t = d * xv;
          sh += t * aw[i];
          accw[i] += t * ah;
        }
      }
    }
    __syncthreads();
    red[tid] = sh;
    __syncthreads();
    if (g0 == 0) {
      for (int g = 1; g < groups; ++g) sh += red[g * nc4 + c4];
      // one PARTIAL per row, slab and channel, stored (not added): da_h_part[slab][n][h][c].  (Float atomics into one [n][h][c] array
      // summed in arrival order and seeded run-to-run differences of dx; the caller folds the slabs in index order: ly_sum_rows)
      ly_stg4(da_h + ((long)slab * n_img * H + nh) * C + 4 * c4, sh);
    }
  }
  if (g0 < groups) {
#pragma unroll
    for (int i = 0; i < LY_CAG_MAXW; ++i) {
      const int w = w0 + g0 + i * groups;
      if (w < W) {
        ly_stg4(da_w + ((long)band * n_img * W + n * W + w) * C + 4 * c4, accw[i]);      // da_w_part[band][n][w][c]
      }
    }
  }
}

extern "C" int ly_coordatt_gate_bwd(const void* dout, int ldd, const void* x, int ldx, int n_img, int H, int W, int C, const float* a_h,
                                    const float* a_w, void* dx, int lddx, float* da_h, float* da_w, int bands_in, int slabs_in, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "coordatt_gate_bwd");
  LY_CHECK(dout && x && a_h && a_w && dx && da_h && da_w, "coordatt_gate_bwd: null pointer");
  LY_CHECK((C & 3) == 0 && C <= 1024 && (ldd & 3) == 0 && (ldx & 3) == 0 && (lddx & 3) == 0, "coordatt_gate_bwd: C / ld must be multiples of 4");
  const int groups = LY_THREADS / (C >> 2);
  const int slabs = (W + groups * LY_CAG_MAXW - 1) / (groups * LY_CAG_MAXW);
  const int bands = (H + LY_CAG_RB - 1) / LY_CAG_RB;
  LY_CHECK(bands_in == bands && slabs_in == slabs, "coordatt_gate_bwd: the partial buffers are da_h [%d slabs][n][H][C] and da_w [%d bands][n][W][C] (got %d, %d)",
           slabs, bands, slabs_in, bands_in);
  LY_WITH_T(dtype, hipLaunchKernelGGL(ly_coordatt_gate_bwd_kernel<T>, dim3((unsigned)(n_img * bands * slabs)), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                                      reinterpret_cast<const T*>(dout), ldd, reinterpret_cast<const T*>(x), ldx, H, W, C, a_h, a_w, reinterpret_cast<T*>(dx), lddx, da_h, da_w,
                                      bands, slabs, (long)n_img));
  LY_LAUNCH_CHECK();
  return 0;
}

template <typename T, bool ACC>
__global__ __launch_bounds__(LY_THREADS) void ly_pool_hw_bwd_kernel(const float* __restrict__ gp, int n_img, int H, int W, int C,
                                                                    T* __restrict__ dx, int lddx) {
  // thread = (16-byte channel vector, column lane): a block walks (image, row) pairs, the row's own pool gradient is loaded once per pair and
  // columns advance by a stride — no per-item index arithmetic (the flat form below pays three 64-bit divisions per 8 bytes)
  constexpr int VW = LyT<T>::VW, NQ = VW / 4;
  using RV = typename LyT<T>::RV;
  if ((C % VW) == 0 && (lddx % VW) == 0 && C / VW <= LY_THREADS) {
    const int ncv = C / VW, groups = LY_THREADS / ncv;
    const int cv = threadIdx.x % ncv, wl = threadIdx.x / ncv;
    if (wl >= groups) return;
    const int c = VW * cv;
    const float iw = 1.f / (float)W, ih = 1.f / (float)H;
    const long rows = (long)n_img * H;
    for (long nh = blockIdx.x; nh < rows; nh += gridDim.x) {
      const long n = nh / H;
      const int h = (int)(nh - n * H);
      const float* const ga = gp + (n * (H + W) + h) * C + c;
      const float* const gb = gp + (n * (H + W) + H) * C + c;
      f32x4 a[NQ];
#pragma unroll
      for (int q = 0; q < NQ; ++q) a[q] = ly_ldg4(ga + 4 * q) * iw;
      T* const drow = dx + nh * (long)W * lddx + c;
      for (int w = wl; w < W; w += groups) {
        f32x4 v[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) v[q] = a[q] + ly_ldg4(gb + (long)w * C + 4 * q) * ih;
        if (ACC) {
          f32x4 o[NQ];
          ly_rv_unpack(ly_ldrv<T>(drow + (long)w * lddx), o);
#pragma unroll
          for (int q = 0; q < NQ; ++q) v[q] += o[q];
        }
        *reinterpret_cast<RV*>(drow + (long)w * lddx) = ly_rv_pack(v, (RV*)nullptr);
      }
    }
    return;
  }
  const int nc4 = C >> 2;
  const long total = (long)n_img * H * W * nc4;
  const float iw = 1.f / (float)W, ih = 1.f / (float)H;
  for (long i = (long)blockIdx.x * LY_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * LY_THREADS) {
    const long pix = i / nc4;
    const int c = 4 * (int)(i - pix * nc4);
    const long row = pix / W;
    const int w = (int)(pix - row * W);
    const long n = row / H;
    const int h = (int)(row - n * H);
    const f32x4 a = ly_ldg4(gp + (n * (H + W) + h) * C + c), b = ly_ldg4(gp + (n * (H + W) + H + w) * C + c);
    f32x4 v = a * iw + b * ih;
    if (ACC) v += ly_ld4<T>(dx + pix * lddx + c);
    ly_st4<T>(dx + pix * lddx + c, v);
  }
}

extern "C" int ly_pool_hw_bwd(const float* gp, int n_img, int H, int W, int C, void* dx, int lddx, int accumulate, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "pool_hw_bwd");
  LY_CHECK(gp && dx && n_img > 0 && H > 0 && W > 0 && (C & 3) == 0 && (lddx & 3) == 0, "pool_hw_bwd: bad arguments");
  long nb = ly_ew_blocks((long)n_img * H * W * (C >> 2));
  if (nb > (long)n_img * H) nb = (long)n_img * H;              // (the row-walking form: a block per (image, row) pair at most)
  const dim3 grid((unsigned)nb);
  if (accumulate) {
    LY_WITH_T(dtype, hipLaunchKernelGGL((ly_pool_hw_bwd_kernel<T, true>), grid, dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), gp, n_img, H, W, C,
                                        reinterpret_cast<T*>(dx), lddx));
  } else {
    LY_WITH_T(dtype, hipLaunchKernelGGL((ly_pool_hw_bwd_kernel<T, false>), grid, dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), gp, n_img, H, W, C,
                                        reinterpret_cast<T*>(dx), lddx));
  }
  LY_LAUNCH_CHECK();
  return 0;
}

// -------------------------------------------------------------------------------------------------
// k x k / stride 1 / pad k//2 max-pool backward (SPPF, models/common.py:348-366): for every output position the
// argmax of its window (first maximum in row-major scan order, as ATen's max_pool2d) is recomputed from x and
// dy is added there: dx[argmax] += dy.  dx is accumulated into (float atomics), so chained pools can add into
// the gradient slots of the concat buffer in place.
// -------------------------------------------------------------------------------------------------
template <typename T, int K>
__global__ __launch_bounds__(LY_THREADS) void ly_maxpool_bwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ dy, int lddy,
                                                                    int n_img, int H, int W, int C, int k_rt, float* __restrict__ dx, int lddx) {
  // K > 0: window size known at compile time — the K*K loads of a position are all issued before the first compare, from clamped
  // coordinates (a `continue` around a load is a branch around a load: every later s_waitcnt turns conservative and the window is
  // walked one round trip at a time); out-of-range taps are masked in the compare.  K == 0: run-time window (any odd k).
  const int nc4 = C >> 2;
  const int k = K > 0 ? K : k_rt, r = k >> 1;
  const long total = (long)n_img * H * W * nc4;
  for (long i = (long)blockIdx.x * LY_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * LY_THREADS) {
    const long pix = i / nc4;
    const int c = 4 * (int)(i - pix * nc4);
    const long row = pix / W;
    const int w = (int)(pix - row * W);
    const long n = row / H;
    const int h = (int)(row - n * H);
    f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    long arg[4] = {-1, -1, -1, -1};
    if constexpr (K > 0) {
      typename LyT<T>::R4 raw[K * K];
#pragma unroll
      for (int dyy = 0; dyy < K; ++dyy)
#pragma unroll
        for (int dxx = 0; dxx < K; ++dxx) {
          int yy = h - r + dyy, xx = w - r + dxx;
          yy = yy < 0 ? 0 : (yy >= H ? H - 1 : yy);
          xx = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);
          raw[dyy * K + dxx] = ly_ldr4<T>(x + ((n * H + yy) * W + xx) * ldx + c);
        }
#pragma unroll
      for (int dyy = 0; dyy < K; ++dyy)
#pragma unroll
        for (int dxx = 0; dxx < K; ++dxx) {
          const int yy = h - r + dyy, xx = w - r + dxx;
          const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
          const long q = (n * H + yy) * W + xx;
          const f32x4 v = ly_r4_f32(raw[dyy * K + dxx]);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (ok && (v[e] > best[e] || arg[e] < 0)) { best[e] = v[e]; arg[e] = q; }
        }
    } else {
      for (int yy = h - r; yy <= h + r; ++yy) {
        if (yy < 0 || yy >= H) continue;
        for (int xx = w - r; xx <= w + r; ++xx) {
          if (xx < 0 || xx >= W) continue;
          const long q = (n * H + yy) * W + xx;
          const f32x4 v = ly_ld4<T>(x + q * ldx + c);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (v[e] > best[e] || arg[e] < 0) { best[e] = v[e]; arg[e] = q; }
        }
      }
    }
    const f32x4 g = ly_ldg4(dy + pix * lddy + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) atomicAdd(dx + arg[e] * lddx + c + e, g[e]);
  }
}

extern "C" int ly_maxpool_bwd(const void* x, int ldx, const float* dy, int lddy, int n_img, int H, int W, int C, int k, float* dx, int lddx,
                              int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "maxpool_bwd");
  LY_CHECK(x && dy && dx && n_img > 0 && H > 0 && W > 0 && (k & 1) == 1, "maxpool_bwd: bad arguments");
  LY_CHECK((C & 3) == 0 && (ldx & 3) == 0 && (lddy & 3) == 0, "maxpool_bwd: C / ld must be multiples of 4");
  const dim3 grid((unsigned)ly_ew_blocks((long)n_img * H * W * (C >> 2)));
  if (k == 5) {                                            // SPPF(k=5): the one size LEAD-YOLO uses
    LY_WITH_T(dtype, hipLaunchKernelGGL((ly_maxpool_bwd_kernel<T, 5>), grid, dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                                        reinterpret_cast<const T*>(x), ldx, dy, lddy, n_img, H, W, C, k, dx, lddx));
  } else {
    LY_WITH_T(dtype, hipLaunchKernelGGL((ly_maxpool_bwd_kernel<T, 0>), grid, dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                                        reinterpret_cast<const T*>(x), ldx, dy, lddy, n_img, H, W, C, k, dx, lddx));
  }
  LY_LAUNCH_CHECK();
  return 0;
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

// -------------------------------------------------------------------------------------------------
// bf16x3 fragment packing on the device (pack.frag_pack3 as ONE launch; weights change every optimiser step):
//   out[((t*S + s)*2 + plane)*64 + lane][j] = plane(W[16t + (lane&15)][32s + 16(j>>2) + 4(lane>>4) + (j&3)])
// W[r][k] is read as w[r*ld_r + k*ld_k], so a transposed view is packed without materialising it.
// -------------------------------------------------------------------------------------------------
template <int PL>
__global__ __launch_bounds__(LY_THREADS) void ly_frag_pack3_kernel(const float* __restrict__ w, int R, int K, long ld_r, long ld_k, int T, int S,
                                                                   uint4* __restrict__ out) {
  const long total = (long)T * S * 64;
  for (long i = (long)blockIdx.x * LY_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * LY_THREADS) {
    const int lane = (int)(i & 63);
    const long ts = i >> 6;
    const int s = (int)(ts % S), t = (int)(ts / S);
    const int row = 16 * t + (lane & 15), q = lane >> 4;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 32 * s + 16 * (j >> 2) + 4 * q + (j & 3);
      v[j] = (row < R && k < K) ? w[row * ld_r + k * ld_k] : 0.f;
    }
    bf16x8 hi, lo;
    ly_split8(v, hi, lo);
    out[(ts * PL) * 64 + lane] = __builtin_bit_cast(uint4, hi);
    if constexpr (PL == 2) out[(ts * PL + 1) * 64 + lane] = __builtin_bit_cast(uint4, lo);
  }
}

extern "C" int ly_frag_pack3(const float* w, int R, int K, long ld_r, long ld_k, int rows_to, int planes, void* out, void* stream) {
  LY_CHECK(w && out && R > 0 && K > 0 && (planes == 1 || planes == 2), "frag_pack3: bad arguments");
  const int rr = R > rows_to ? R : rows_to;
  const int T = (rr + 15) / 16, S = (K + 31) / 32;
  if (planes == 2)
    hipLaunchKernelGGL(ly_frag_pack3_kernel<2>, dim3((unsigned)ly_ew_blocks((long)T * S * 64)), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), w,
                       R, K, ld_r, ld_k, T, S, reinterpret_cast<uint4*>(out));
  else
    hipLaunchKernelGGL(ly_frag_pack3_kernel<1>, dim3((unsigned)ly_ew_blocks((long)T * S * 64)), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), w,
                       R, K, ld_r, ld_k, T, S, reinterpret_cast<uint4*>(out));
  LY_LAUNCH_CHECK();
  return 0;
}


// -------------------------------------------------------------------------------------------------
// Batched packing: every packed weight matrix the model needs (forward, transposed for dgrad, tap-flipped, ...) refreshed by ONE
// launch over a device-resident table of descriptors (113-144 ly_frag_pack3 launches per training step before).  A descriptor
// reads the fp32 parameter IN PLACE through an index map, so none of the permuted / padded / concatenated temporaries the
// per-matrix path built on the host exist any more:
//   packed row r = ra*nrb + rb, column k = (a*nb + b)*nc + c;   valid iff r < r_valid, b < vb, c < vc
//   element = src[ra*sra + rb*srb + a*sa + b*sb + c*sc]                (strides may be negative: tap flips)
// and writes row tiles [t0, t0 + T) of a [Ttot][S][planes][64][8] bf16 fragment image (zeros where invalid).
// -------------------------------------------------------------------------------------------------
template <int PL>
__device__ __forceinline__ void ly_pack_one(const LyPackDesc& d, long i) {
  const int lane = (int)(i & 63);
  const long ts = i >> 6;
  const int s = (int)(ts % d.S), t = (int)(ts / d.S);
  const int row = 16 * t + (lane & 15), q = lane >> 4;
  const bool rok = row < d.r_valid;
  const int ra = row / d.nrb, rb = row - ra * d.nrb;
  const long roff = (long)ra * d.sra + (long)rb * d.srb;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 32 * s + 16 * (j >> 2) + 4 * q + (j & 3);
    const int c = k % d.nc, ab = k / d.nc;
    const int b = ab % d.nb, a = ab / d.nb;
    const bool ok = rok && k < d.K && b < d.vb && c < d.vc;
    v[j] = ok ? d.src[roff + (long)a * d.sa + (long)b * d.sb + (long)c * d.sc] : 0.f;
  }
  bf16x8 hi, lo;
  ly_split8(v, hi, lo);
  uint4* out = reinterpret_cast<uint4*>(d.dst);
  const long fs = ((long)(d.t0 + t) * d.S + s) * PL;
  out[fs * 64 + lane] = __builtin_bit_cast(uint4, hi);
  if constexpr (PL == 2) out[(fs + 1) * 64 + lane] = __builtin_bit_cast(uint4, lo);
}

__global__ __launch_bounds__(LY_THREADS) void ly_pack_table_kernel(const LyPackDesc* __restrict__ tab, const int* __restrict__ blk_desc) {
  const LyPackDesc d = tab[blk_desc[blockIdx.x]];
  const long i = ((long)blockIdx.x - d.blk0) * LY_THREADS + threadIdx.x;
  if (i >= (long)d.T * d.S * 64) return;
  if (d.planes == 2) ly_pack_one<2>(d, i);
  else ly_pack_one<1>(d, i);
}

extern "C" int ly_pack_table(const LyPackDesc* table, const int* blk_desc, int n_blocks, void* stream) {
  LY_CHECK(table && blk_desc && n_blocks > 0, "pack_table: bad arguments");
  hipLaunchKernelGGL(ly_pack_table_kernel, dim3((unsigned)n_blocks), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), table, blk_desc);
  LY_LAUNCH_CHECK();
  return 0;
}

// -------------------------------------------------------------------------------------------------
// MLPBlock backward, last step: dx = dy + g, except the first c4 channels (the partial 3x3 conv's) which take dy + t
// (t [rows, ldt]: the data gradient of the partial conv).  One pass instead of two adds and a strided copy.
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_mlp_dx_kernel(const T* __restrict__ dy, const T* __restrict__ g, const T* __restrict__ t, int ldt,
                                                                long rows, int C, int c4, T* __restrict__ dx) {
  const int nq = C >> 2;
  const long total = rows * nq;
  for (long i = (long)blockIdx.x * LY_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * LY_THREADS) {
    const long r = i / nq;
    const int c = 4 * (int)(i - r * nq);
    const f32x4 a = ly_ld4<T>(dy + r * C + c);
    f32x4 b = ly_ld4<T>(g + r * C + c);
    if (c < c4) {                                           // (c4 need not be a multiple of 4: per-channel select in the boundary quad)
      const f32x4 tv = ly_ld4<T>(t + r * ldt + c);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < c4) b[e] = tv[e];
    }
    ly_st4<T>(dx + r * C + c, a + b);
  }
}

extern "C" int ly_mlp_dx(const void* dy, const void* g, const void* t, int ldt, long rows, int C, int c4, void* dx, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "mlp_dx");
  LY_CHECK(dy && g && t && dx && rows > 0 && (C & 3) == 0 && (ldt & 3) == 0 && c4 > 0 && c4 <= C && ((c4 + 3) & ~3) <= ldt, "mlp_dx: bad arguments");
  LY_WITH_T(dtype, hipLaunchKernelGGL(ly_mlp_dx_kernel<T>, dim3((unsigned)ly_ew_blocks(rows * (C >> 2))), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                                      reinterpret_cast<const T*>(dy), reinterpret_cast<const T*>(g), reinterpret_cast<const T*>(t), ldt, rows, C, c4,
                                      reinterpret_cast<T*>(dx)));
  LY_LAUNCH_CHECK();
  return 0;
}

// -------------------------------------------------------------------------------------------------
// SPPF backward without atomics (models/common.py:348-366, three chained k x k / s1 max-pools): the routing of every window — the tap
// index of its first maximum in row-major scan order, ATen's rule — is computed ONCE for all levels (ly_maxpool_arg over the first 3c
// channels of the [y | m(y) | m(m(y)) | m(m(m(y)))] buffer), then each level is a GATHER:
//   dtot[p] = d_own[p] + sum over the k*k windows q that contain p of [arg(q) == tap of p in q] * d_up[q]
// Deterministic, every output written once (the scatter version added with float atomics: 98 us per level).
// -------------------------------------------------------------------------------------------------
template <typename T, int K>
__global__ __launch_bounds__(LY_THREADS) void ly_maxpool_arg_kernel(const T* __restrict__ x, int ldx, int n_img, int H, int W, int C,
                                                                    unsigned char* __restrict__ arg, int lda) {
  constexpr int r = K >> 1;
  const int nc4 = C >> 2;
  const long total = (long)n_img * H * W * nc4;
  for (long i = (long)blockIdx.x * LY_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * LY_THREADS) {
    const long pix = i / nc4;
    const int c = 4 * (int)(i - pix * nc4);
    const long row = pix / W;
    const int w = (int)(pix - row * W);
    const long n = row / H;
    const int h = (int)(row - n * H);
    typename LyT<T>::R4 raw[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) {
      int yy = h - r + t / K, xx = w - r + t % K;
      yy = yy < 0 ? 0 : (yy >= H ? H - 1 : yy);
      xx = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);
      raw[t] = ly_ldr4<T>(x + ((n * H + yy) * W + xx) * ldx + c);
    }
    f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int a[4] = {-1, -1, -1, -1};
#pragma unroll
    for (int t = 0; t < K * K; ++t) {
      const int yy = h - r + t / K, xx = w - r + t % K;
      const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
      const f32x4 v = ly_r4_f32(raw[t]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (ok && (v[e] > best[e] || a[e] < 0)) { best[e] = v[e]; a[e] = t; }
    }
    *reinterpret_cast<unsigned*>(arg + pix * lda + c) = (unsigned)a[0] | ((unsigned)a[1] << 8) | ((unsigned)a[2] << 16) | ((unsigned)a[3] << 24);
  }
}

template <typename TD, typename TO, int K>
__global__ __launch_bounds__(LY_THREADS) void ly_maxpool_gather_kernel(const unsigned char* __restrict__ arg, int lda, const float* __restrict__ d_up, int ldu,
                                                                       const TD* __restrict__ d_own, int ldd, int n_img, int H, int W, int C,
                                                                       TO* __restrict__ out, int ldo) {
  constexpr int r = K >> 1;
  const int nc4 = C >> 2;
  const long total = (long)n_img * H * W * nc4;
  for (long i = (long)blockIdx.x * LY_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * LY_THREADS) {
    const long pix = i / nc4;
    const int c = 4 * (int)(i - pix * nc4);
    const long row = pix / W;
    const int w = (int)(pix - row * W);
    const long n = row / H;
    const int h = (int)(row - n * H);
    unsigned av[K * K];
    f32x4 dv[K * K];
    // window q = (h - (ty - r), w - (tx - r)) sees this pixel as its tap t = ty*K + tx; all loads first, from clamped coordinates
#pragma unroll
    for (int t = 0; t < K * K; ++t) {
      int qy = h - (t / K - r), qx = w - (t % K - r);
      qy = qy < 0 ? 0 : (qy >= H ? H - 1 : qy);
      qx = qx < 0 ? 0 : (qx >= W ? W - 1 : qx);
      const long q = (n * H + qy) * W + qx;
      av[t] = *reinterpret_cast<const unsigned*>(arg + q * lda + c);
      dv[t] = ly_ldg4(d_up + q * ldu + c);
    }
    f32x4 s = ly_ld4<TD>(d_own + pix * ldd + c);
#pragma unroll
    for (int t = 0; t < K * K; ++t) {
      const int qy = h - (t / K - r), qx = w - (t % K - r);
      const bool ok = qy >= 0 && qy < H && qx >= 0 && qx < W;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (ok && ((av[t] >> (8 * e)) & 255u) == (unsigned)t) s[e] += dv[t][e];
    }
    ly_st4<TO>(out + pix * ldo + c, s);
  }
}

// SPPF backward in ONE launch for small maps (models/common.py:348-366 at 20 x 20 / 40 x 40): a block owns one image x 8 channels and keeps the
// whole map in LDS — per level j = 2, 1, 0 it stages y_j, computes the window argmax of every pixel (the rule of ly_maxpool_arg), and gathers
// t_j = d_j + sum over the windows routed to the pixel of t_{j+1} (the order of ly_maxpool_gather: bit-identical sums); t_3 = d_3.  The three
// per-level launches read every routing byte and gradient 25 times through L2 (180 us for a 4 MB map at bs=64); here they come from LDS.
#define LY_SPPF_CG 8
template <typename T, int K>
__global__ __launch_bounds__(LY_THREADS) void ly_sppf_bwd_kernel(const T* __restrict__ buf, int ldb, const T* __restrict__ d, int ldd, int H, int W, int c,
                                                                 T* __restrict__ out, int ldo) {
  constexpr int r = K >> 1, CG = LY_SPPF_CG, NQ = CG / 4;
  extern __shared__ f32x4 ly_sppf_smem[];
  const int HW = H * W;
  f32x4* const GA = ly_sppf_smem;                                  // [HW][NQ] running gradient t_{j+1}
  f32x4* const GB = GA + HW * NQ;                                  // [HW][NQ] t_j being built
  f32x4* const Y = GB + HW * NQ;                                   // [HW][NQ] y_j as fp32 (exact for bf16 / fp32 inputs)
  unsigned* const A = reinterpret_cast<unsigned*>(Y + HW * NQ);    // [HW][NQ] four routing bytes
  const int groups = c / CG;
  const int bid = ly_xcd_remap((int)blockIdx.x, (int)gridDim.x);            // the channel groups of an image read the same cache lines: one XCD's L2
  const long n = bid / groups;
  const int c0 = (int)(bid - n * groups) * CG;
  const int tid = threadIdx.x;
  const T* const bn = buf + n * HW * (long)ldb;
  const T* const dn = d + n * HW * (long)ldd;
  for (int i = tid; i < HW * NQ; i += LY_THREADS) {
    const int pix = i / NQ, q = i - pix * NQ;
    GA[i] = ly_ld4<T>(dn + (long)pix * ldd + 3 * c + c0 + 4 * q);
  }
  f32x4* gin = GA;
  f32x4* gout = GB;
  for (int j = 2; j >= 0; --j) {
    // y_j and d_j of the level are requested together (d_j waits in gout, which the gather below overwrites item by item): one memory
    // round trip per level instead of two
    for (int i = tid; i < HW * NQ; i += LY_THREADS) {
      const int pix = i / NQ, q = i - pix * NQ;
      const f32x4 yv = ly_ld4<T>(bn + (long)pix * ldb + j * c + c0 + 4 * q);
      const f32x4 dv = ly_ld4<T>(dn + (long)pix * ldd + j * c + c0 + 4 * q);
      Y[i] = yv;
      gout[i] = dv;
    }
    __syncthreads();
    for (int i = tid; i < HW * NQ; i += LY_THREADS) {
      const int pix = i / NQ, q = i - pix * NQ;
      const int h = pix / W, w = pix - h * W;
      f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      int a[4] = {-1, -1, -1, -1};
#pragma unroll
      for (int t = 0; t < K * K; ++t) {
        const int yy = h - r + t / K, xx = w - r + t % K;
        const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const f32x4 v = Y[(ok ? yy * W + xx : pix) * NQ + q];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (ok && (v[e] > best[e] || a[e] < 0)) { best[e] = v[e]; a[e] = t; }
      }
      A[i] = (unsigned)a[0] | ((unsigned)a[1] << 8) | ((unsigned)a[2] << 16) | ((unsigned)a[3] << 24);
    }
    __syncthreads();
    for (int i = tid; i < HW * NQ; i += LY_THREADS) {
      const int pix = i / NQ, q = i - pix * NQ;
      const int h = pix / W, w = pix - h * W;
      f32x4 sacc = gout[i];
#pragma unroll
      for (int t = 0; t < K * K; ++t) {
        // window qp = (h - (ty - r), w - (tx - r)) sees this pixel as its tap t
        const int qy = h - (t / K - r), qx = w - (t % K - r);
        const bool ok = qy >= 0 && qy < H && qx >= 0 && qx < W;
        const int qp = ok ? qy * W + qx : pix;
        const unsigned av = A[qp * NQ + q];
        const f32x4 dv = gin[qp * NQ + q];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (ok && ((av >> (8 * e)) & 255u) == (unsigned)t) sacc[e] += dv[e];
      }
      if (j == 0) ly_st4<T>(out + (n * HW + pix) * (long)ldo + c0 + 4 * q, sacc);
      else gout[i] = sacc;
    }
    __syncthreads();
    f32x4* const tmp = gin; gin = gout; gout = tmp;
  }
}

// returns 1 (nothing launched) when the map does not fit the fused kernel: the caller then uses ly_maxpool_arg / ly_maxpool_gather
extern "C" int ly_sppf_bwd(const void* buf, int ldb, const void* d, int ldd, int n_img, int H, int W, int c, int k, void* out, int ldo, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "sppf_bwd");
  LY_CHECK(buf && d && out && n_img > 0 && H > 0 && W > 0 && c > 0, "sppf_bwd: bad arguments");
  const size_t lds = (size_t)H * W * (LY_SPPF_CG / 4) * (3 * sizeof(f32x4) + sizeof(unsigned));
  if (k != 5 || c % LY_SPPF_CG || (ldb & 3) || (ldd & 3) || (ldo & 3) || lds > 150 * 1024 || (long)n_img * (c / LY_SPPF_CG) > 2000000000L) return 1;
  const dim3 grid((unsigned)(n_img * (c / LY_SPPF_CG)));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LY_WITH_T(dtype, return ly_launch_lds<ly_sppf_bwd_kernel<T, 5>>(grid, dim3(LY_THREADS), lds, st, reinterpret_cast<const T*>(buf), ldb, reinterpret_cast<const T*>(d),
                                                                  ldd, H, W, c, reinterpret_cast<T*>(out), ldo));
}

extern "C" int ly_maxpool_arg(const void* x, int ldx, int n_img, int H, int W, int C, int k, unsigned char* arg, int lda, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "maxpool_arg");
  LY_CHECK(x && arg && n_img > 0 && H > 0 && W > 0 && k == 5, "maxpool_arg: bad arguments (built for k = 5, SPPF)");
  LY_CHECK((C & 3) == 0 && (ldx & 3) == 0 && (lda & 3) == 0, "maxpool_arg: C / ld must be multiples of 4");
  LY_WITH_T(dtype, hipLaunchKernelGGL((ly_maxpool_arg_kernel<T, 5>), dim3((unsigned)ly_ew_blocks((long)n_img * H * W * (C >> 2))), dim3(LY_THREADS), 0,
                                      reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const T*>(x), ldx, n_img, H, W, C, arg, lda));
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_maxpool_gather(const unsigned char* arg, int lda, const float* d_up, int ldu, const void* d_own, int ldd, int own_dtype, int n_img, int H,
                                 int W, int C, int k, void* out, int ldo, int out_dtype, void* stream) {
  LY_CHECK_DTYPE(own_dtype, "maxpool_gather");
  LY_CHECK_DTYPE(out_dtype, "maxpool_gather");
  LY_CHECK(arg && d_up && d_own && out && n_img > 0 && H > 0 && W > 0 && k == 5, "maxpool_gather: bad arguments (built for k = 5, SPPF)");
  LY_CHECK((C & 3) == 0 && (lda & 3) == 0 && (ldu & 3) == 0 && (ldd & 3) == 0 && (ldo & 3) == 0, "maxpool_gather: C / ld must be multiples of 4");
  const dim3 grid((unsigned)ly_ew_blocks((long)n_img * H * W * (C >> 2)));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define LY_MPG(TD, TO) hipLaunchKernelGGL((ly_maxpool_gather_kernel<TD, TO, 5>), grid, dim3(LY_THREADS), 0, st, arg, lda, d_up, ldu, reinterpret_cast<const TD*>(d_own), ldd, \
                                          n_img, H, W, C, reinterpret_cast<TO*>(out), ldo)
  if (own_dtype == LY_BF16 && out_dtype == LY_BF16) LY_MPG(__bf16, __bf16);
  else if (own_dtype == LY_BF16) LY_MPG(__bf16, float);
  else if (out_dtype == LY_BF16) LY_MPG(float, __bf16);
  else LY_MPG(float, float);
#undef LY_MPG
  LY_LAUNCH_CHECK();
  return 0;
}
