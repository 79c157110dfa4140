// Backward building blocks of the training step that belong to no single module, gfx950; activations / activation
// gradients T = float or __bf16.
//
//   ly_up2_bwd                            adjoint of the nearest-2x upsampled read (models/LEAD-YOLO.yaml neck)
//   ly_unpatch                            adjoint of the k = s = 2 patch gather (models/common.py:1555-1561)
//   ly_patch4_rows_u8                     space-to-depth of the uint8 image for PatchEmbed's weight gradient (models/common.py:1537-1550)
//   ly_sum_rows, ly_sum_rows_f64, ly_f64_add   fixed-order folds of partial-row buffers, fp64 accumulator adds
//   ly_mlp_dx                             last step of the MLPBlock backward (models/common.py:1478-1482)
//
// The BatchNorm + activation passes are in ly_bnact.hip, the weight gradients (ly_wgrad: contraction over PIXELS with the forward's
// gather) in ly_wgrad.hip, the per-module backward kernels with their forwards (ly_coordatt.hip, ly_sppf.hip, ly_detect.hip,
// ly_rfcbam_att.hip).  Data gradients (dgrad) of the 1x1 / 3x3 convolutions reuse the forward contraction kernels
// (ly_gemm_fwd / ly_conv3x3_fwd) with transposed, frag-packed weights: the adjoint of a stride-1
// convolution is a stride-1 convolution.
#include "ly_tile.hpp"
#include "ly_params.h"
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
