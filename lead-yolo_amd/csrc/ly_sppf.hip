// SPPF's chained max-pools (models/common.py:348-366: three k x k / stride 1 / pad k//2 pools and the concat), forward and backward, gfx950:
// activations T = float / __bf16, gradients in flight fp32.
//
//   ly_sppf_pool        [x | m(x) | m(m(x)) | m(m(m(x)))] from one LDS copy of the map
//   ly_sppf_bwd         small maps: the three levels' backward in ONE launch, map and routing in LDS (returns 1 when the map does not fit)
//   ly_maxpool_arg      the routing of every window (tap of its first maximum), once for all levels
//   ly_maxpool_gather   one level's backward as a gather over that routing: deterministic, every output written once
//   ly_maxpool_bwd      one level's backward as a scatter with float atomics (any k)
#include <float.h>

#include "ly_tile.hpp"
#include "ly_params.h"
// ---------------------------------------------------------------------------------------------------
// SPPF pooling: out[n, p, 0:C] = x, [C:2C] = m5(x), [2C:3C] = m5(m5(x)), [3C:4C] = m5(m5(m5(x)))
// (k x k, stride 1, pad k//2, -inf padding; reference models/common.py:348-366).  Chained k-max pools
// equal single (2k-1)- and (3k-2)-wide max windows, computed separably from one LDS copy of the map.
// One block per (image, 16-channel group); the map (H*W <= 4096) lives in LDS.
// ---------------------------------------------------------------------------------------------------
#define LY_SP_CG 4     // channels per block: n_img * C/4 blocks keep the whole chip busy on the small P5 map
template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_sppf_pool_kernel(const T* __restrict__ x, int ldx, int H, int W, int C, int k,
                                                                  T* __restrict__ out, int ldo) {
  extern __shared__ f32x4 sp4[];               // a[HW], b[HW] as float4 (4 channels per position)
  const int HW = H * W;
  f32x4* a = sp4;
  f32x4* b = sp4 + HW;
  const int groups = C / LY_SP_CG;
  const int bid = ly_xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int n = bid / groups, g = bid - n * groups;
  const int c0 = g * LY_SP_CG;
  const int tid = threadIdx.x, r = k / 2;
  const f32x4 ninf = (f32x4){-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int p = tid; p < HW; p += LY_THREADS) {
    const f32x4 v = ly_ld4<T>(x + ((long)n * HW + p) * ldx + c0);
    a[p] = v;
    ly_st4<T>(out + ((long)n * HW + p) * ldo + c0, v);
  }
  __syncthreads();
  for (int level = 1; level <= 3; ++level) {
    // b = row-max of a, then a = col-max of b  (one k x k max pool of the previous level)
    for (int p = tid; p < HW; p += LY_THREADS) {
      const int h = p / W, w = p - h * W;
      f32x4 m = ninf;
      for (int d = -r; d <= r; ++d) {
        const int ww = w + d;
        if (ww >= 0 && ww < W) {
          const f32x4 v = a[h * W + ww];
#pragma unroll
          for (int q = 0; q < 4; ++q) m[q] = fmaxf(m[q], v[q]);
        }
      }
      b[p] = m;
    }
    __syncthreads();
    for (int p = tid; p < HW; p += LY_THREADS) {
      const int h = p / W, w = p - h * W;
      f32x4 m = ninf;
      for (int d = -r; d <= r; ++d) {
        const int hh = h + d;
        if (hh >= 0 && hh < H) {
          const f32x4 v = b[hh * W + w];
#pragma unroll
          for (int q = 0; q < 4; ++q) m[q] = fmaxf(m[q], v[q]);
        }
      }
      a[p] = m;
      ly_st4<T>(out + ((long)n * HW + p) * ldo + level * C + c0, m);
    }
    __syncthreads();
  }
}

extern "C" int ly_sppf_pool(const void* x, int ldx, int n_img, int H, int W, int C, int k, void* out, int ldo, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "sppf_pool");
  LY_CHECK(x && out && k >= 1 && (k & 1) && (C & 3) == 0 && (ldx & 3) == 0 && (ldo & 3) == 0, "sppf_pool: bad arguments");
  size_t lds = sizeof(float) * 2 * (size_t)H * W * 4;
  LY_CHECK(lds <= LY_LDS_MAX, "sppf_pool: %dx%d map does not fit LDS (%zu B)", H, W, lds);
  LY_WITH_T(dtype, return ly_launch_lds<ly_sppf_pool_kernel<T>>(dim3(n_img * (C / LY_SP_CG)), dim3(LY_THREADS), lds, reinterpret_cast<hipStream_t>(stream),
                                                                reinterpret_cast<const T*>(x), ldx, H, W, C, k, reinterpret_cast<T*>(out), ldo));
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
