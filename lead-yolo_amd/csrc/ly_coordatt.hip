// CoordAtt (models/common.py:1595-1609, 1623), forward and training backward, gfx950: activations T = float / __bf16, the pooled vectors, the
// attention tables a_h / a_w and every parameter gradient fp32.  All kernels are bandwidth-trivial next to the convolutions; they exist so
// that the map is read a minimal number of times.
//
//   ly_pool_hw               pool_h / pool_w: row and column means of the map                 (models/common.py:1598-1599)
//   ly_coordatt_conv1_stats  train mode: sum / sum of squares of conv1's output for bn1
//   ly_coordatt_mlp          conv1 + bn1 + h_swish, conv_h / conv_w + sigmoid                 (models/common.py:1600-1607)
//   ly_coordatt_gate         out = x * a_w * a_h (+ res)                                      (models/common.py:1608, 1623)
//   ly_coordatt_gate_bwd     dx = dout * a_h * a_w and the partial sums of da_h, da_w
//   ly_coordatt_mlp_bwd      the vector MLP under autograd, two launches (bn1 needs its sums over all positions first)
//   ly_pool_hw_bwd           the pools' gradient, written or added into dx
#include "ly_tile.hpp"
#include "ly_params.h"
// ---------------------------------------------------------------------------------------------------
// generic strided reduction:  out[o, c] = scale * sum_{j < L} x[base(o) + j*stride + c]
// one block per output row o; threads = (c4, j-lane)
// ---------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_pool_hw_kernel(const T* __restrict__ x, int ldx, int H, int W, int C,
                                                                 float* __restrict__ pool) {
  // block b -> (n, pos); pos < H: mean over w of row pos; else mean over h of column pos-H
  __shared__ f32x4 red[LY_THREADS];
  const int L = H + W;
  const int bid = ly_xcd_remap((int)blockIdx.x, (int)gridDim.x);     // an image's H row blocks and W column blocks read the same cache lines: one XCD's L2
  const int n = bid / L, pos = bid - n * L;
  const int nc4 = C >> 2;
  const int tid = threadIdx.x;
  const int groups = LY_THREADS / nc4;
  const bool row = pos < H;
  const int len = row ? W : H;
  const long base = row ? ((long)n * H + pos) * W : ((long)n * H) * W + (pos - H);
  const long step = row ? 1 : W;
  const int c4 = tid % nc4, j0 = tid / nc4;       // C <= 1024 so nc4 <= 256
  f32x4 s = ly_zero4();
  if (j0 < groups) {
#pragma unroll 4
    for (int j = j0; j < len; j += groups) s += ly_ld4<T>(x + (base + j * step) * ldx + 4 * c4);
  }
  red[tid] = s;
  __syncthreads();
  if (j0 == 0) {
    for (int g = 1; g < groups; ++g) s += red[g * nc4 + c4];
    const float inv = 1.f / (float)len;
    ly_stg4(pool + ((long)n * L + pos) * C + 4 * c4, s * inv);
  }
}

extern "C" int ly_pool_hw(const void* x, int ldx, int n_img, int H, int W, int C, float* pool, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "pool_hw");
  LY_CHECK(x && pool && (C & 3) == 0 && (ldx & 3) == 0 && C <= 1024, "pool_hw: bad arguments (C=%d ldx=%d)", C, ldx);
  LY_WITH_T(dtype, hipLaunchKernelGGL(ly_pool_hw_kernel<T>, dim3(n_img * (H + W)), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                                      reinterpret_cast<const T*>(x), ldx, H, W, C, pool));
  LY_LAUNCH_CHECK();
  return 0;
}

// y = hswish(W1' pool + b1')  (BN folded),  a = sigmoid(Wx y + bx);  one block per (n, pos)
__global__ __launch_bounds__(LY_THREADS) void ly_coordatt_mlp_kernel(const float* __restrict__ pool, int H, int W, int C, int mip,
                                                                      const float* __restrict__ w1, const float* __restrict__ b1,
                                                                      const float* __restrict__ sc, const float* __restrict__ sh,
                                                                      const float* __restrict__ wh, const float* __restrict__ bh,
                                                                      const float* __restrict__ ww, const float* __restrict__ bw,
                                                                      float* __restrict__ a_h, float* __restrict__ a_w) {
  __shared__ float ys[64];
  const int L = H + W;
  const int n = blockIdx.x / L, pos = blockIdx.x - n * L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* p = pool + ((long)n * L + pos) * C;
  for (int m = wave; m < mip; m += 4) {
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += w1[m * C + c] * p[c];
    s = ly_group_sum(s, 64);
    if (lane == 0) ys[m] = ly_hswish(sc ? (s + b1[m]) * sc[m] + sh[m] : s + b1[m]);
  }
  __syncthreads();
  const bool isrow = pos < H;
  const float* wx = isrow ? wh : ww;
  const float* bx = isrow ? bh : bw;
  float* out = isrow ? a_h + ((long)n * H + pos) * C : a_w + ((long)n * W + (pos - H)) * C;
  for (int c = tid; c < C; c += LY_THREADS) {
    float s = bx[c];
    for (int m = 0; m < mip; ++m) s += wx[c * mip + m] * ys[m];
    out[c] = ly_sigmoid(s);
  }
}

extern "C" int ly_coordatt_mlp(const float* pool, int n_img, int H, int W, int C, int mip, const float* w1, const float* b1,
                               const float* sc, const float* sh, const float* wh, const float* bh, const float* ww, const float* bw, float* a_h, float* a_w,
                               void* stream) {
  LY_CHECK(pool && w1 && b1 && wh && bh && ww && bw && a_h && a_w && (!sc == !sh), "coordatt_mlp: null pointer");
  LY_CHECK(mip > 0 && mip <= 64, "coordatt_mlp: mip=%d out of range", mip);
  hipLaunchKernelGGL(ly_coordatt_mlp_kernel, dim3(n_img * (H + W)), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     pool, H, W, C, mip, w1, b1, sc, sh, wh, bh, ww, bw, a_h, a_w);
  LY_LAUNCH_CHECK();
  return 0;
}

// CoordAtt bn1 statistics: y1[n, pos, m] = w1[m, :] . pool[n, pos, :] + b1[m];  stats[m] += y1, stats[mip + m] += y1^2
// One WAVE per position: lanes stride the channels and carry all `mip` outputs (MIPMAX accumulators), one shuffle tree per position,
// lanes m < mip keep the running sums; the four waves of a block meet in LDS and the block adds ONCE per output.  (The first version
// gave each wave two outputs and walked the block's positions serially per output: 113 us per launch.)
template <int MIPMAX>
__global__ __launch_bounds__(LY_THREADS) void ly_coordatt_conv1_stats_kernel(const float* __restrict__ pool, long positions, int C, int mip,
                                                                              const float* __restrict__ w1, const float* __restrict__ b1,
                                                                              double* __restrict__ stats) {
  __shared__ float red[4][2 * MIPMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float a1 = 0.f, a2 = 0.f;
  // the lane that accumulates output m: lane m on the general path; on the fast path the reduce-scatter leaves output m in lane m * (64 / MIPMAX)
  constexpr bool FASTP = MIPMAX <= 16;
  constexpr int LSTEP = FASTP ? 64 / MIPMAX : 1;
  const bool fast = FASTP && C <= 256;
  const int mine = fast ? lane / LSTEP : lane;
  const bool owner = (fast ? (lane % LSTEP) == 0 : true) && mine < mip;
  const float bm = owner ? b1[mine] : 0.f;
  const long nw = (long)gridDim.x * 4;
  if constexpr (FASTP) if (fast) {
    // the lane's weights stay in registers over all positions, and two positions per trip have all their loads issued before the first use
    // (the one-position loop re-read w1 and paid a dependent round trip per position: 23 us for 2.6 MB)
    constexpr int KC = 4;
    float wreg[KC][MIPMAX];
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
      for (int m = 0; m < MIPMAX; ++m) wreg[k][m] = (m < mip && lane + 64 * k < C) ? w1[m * C + lane + 64 * k] : 0.f;
    constexpr int UP = 2;
    for (long pos0 = (long)blockIdx.x * 4 + wave; pos0 < positions; pos0 += UP * nw) {
      float pv[UP][KC];
#pragma unroll
      for (int u = 0; u < UP; ++u) {
        const long pos = pos0 + u * nw < positions ? pos0 + u * nw : positions - 1;
#pragma unroll
        for (int k = 0; k < KC; ++k) pv[u][k] = lane + 64 * k < C ? pool[pos * C + lane + 64 * k] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < UP; ++u) {
        const bool live = pos0 + u * nw < positions;
        float y[MIPMAX];
#pragma unroll
        for (int m = 0; m < MIPMAX; ++m) {
          y[m] = 0.f;
#pragma unroll
          for (int k = 0; k < KC; ++k) y[m] += wreg[k][m] * pv[u][k];
        }
        ly_reduce_scatter<MIPMAX>(y, lane);                 // MIPMAX - 1 + log2(64 / MIPMAX) cross-lane moves instead of 6 MIPMAX
        if (owner && live) {
          const float v = y[0] + bm;
          a1 += v;
          a2 += v * v;
        }
      }
    }
  }
  if (!fast) {
  for (long pos = (long)blockIdx.x * 4 + wave; pos < positions; pos += nw) {
    const float* p = pool + pos * C;
    float y[MIPMAX];
#pragma unroll
    for (int m = 0; m < MIPMAX; ++m) y[m] = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float pv = p[c];
#pragma unroll
      for (int m = 0; m < MIPMAX; ++m)
        if (m < mip) y[m] += w1[m * C + c] * pv;
    }
#pragma unroll
    for (int m = 0; m < MIPMAX; ++m) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) y[m] += __shfl_xor(y[m], o);
      if (lane == m) {
        const float v = y[m] + bm;
        a1 += v;
        a2 += v * v;
      }
    }
  }
  }
  if (owner) { red[wave][mine] = a1; red[wave][MIPMAX + mine] = a2; }
  __syncthreads();
  if (wave == 0 && lane < mip) {
    atomicAdd(stats + lane, (double)((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane])));
    atomicAdd(stats + mip + lane, (double)((red[0][MIPMAX + lane] + red[1][MIPMAX + lane]) + (red[2][MIPMAX + lane] + red[3][MIPMAX + lane])));
  }
}

extern "C" int ly_coordatt_conv1_stats(const float* pool, long positions, int C, int mip, const float* w1, const float* b1,
                                       double* stats, void* stream) {
  LY_CHECK(pool && w1 && b1 && stats && positions > 0 && mip > 0, "coordatt_conv1_stats: bad arguments");
  LY_CHECK(mip <= 64, "coordatt_conv1_stats: mip=%d out of range", mip);
  long blocks = (positions + 3) / 4;
  if (blocks > 256) blocks = 256;                          // one atomic per (block, output): keep the adds per address few
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (mip <= 8) hipLaunchKernelGGL(ly_coordatt_conv1_stats_kernel<8>, dim3((unsigned)blocks), dim3(LY_THREADS), 0, st, pool, positions, C, mip, w1, b1, stats);
  else if (mip <= 16) hipLaunchKernelGGL(ly_coordatt_conv1_stats_kernel<16>, dim3((unsigned)blocks), dim3(LY_THREADS), 0, st, pool, positions, C, mip, w1, b1, stats);
  else hipLaunchKernelGGL(ly_coordatt_conv1_stats_kernel<64>, dim3((unsigned)blocks), dim3(LY_THREADS), 0, st, pool, positions, C, mip, w1, b1, stats);
  LY_LAUNCH_CHECK();
  return 0;
}

// standalone CoordAtt gating: out = x * a_w[n,w,:] * a_h[n,h,:] (+ res)   (models/common.py:1608, 1623)
// One block per (image, band of 8 rows, slab of columns); a thread owns a 16-byte channel vector of up to 8 columns: their a_w factors are
// loaded once, a row's a_h factor once per row, and each row's x (+ res) vectors are all requested before the first use — per 16 bytes of the
// map one load and one store.  (The first version — thread = (pixel, 4 channels), three 64-bit divisions and two fp32 table loads per 8 bytes
// of x — ran at 2.4 TB/s.)
#define LY_GT_RB 8
#define LY_GT_MAXW 8
template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_gate_kernel(const T* __restrict__ x, int ldx, int H, int W, int C,
                                                              const float* __restrict__ a_h, const float* __restrict__ a_w,
                                                              const T* __restrict__ res, int ldres, T* __restrict__ out, int ldo, int bands, int slabs, int cpt) {
  constexpr int VW = LyT<T>::VW, NQ = VW / 4;
  using RV = typename LyT<T>::RV;
  const int ncv = C / VW, tid = threadIdx.x;
  const int groups = LY_THREADS / ncv;
  const int cv = tid % ncv, g0 = tid / ncv;
  if (g0 >= groups) return;
  const int slab = blockIdx.x % slabs;
  const int bb = blockIdx.x / slabs;
  const long n = bb / bands;
  const int band = bb - (int)n * bands;
  const int w0 = slab * groups * cpt;
  const int h_lo = band * LY_GT_RB, h_hi = h_lo + LY_GT_RB < H ? h_lo + LY_GT_RB : H;
  const int c = VW * cv;
  f32x4 aw[LY_GT_MAXW][NQ];
  bool okw[LY_GT_MAXW];
  int wcl[LY_GT_MAXW];
#pragma unroll
  for (int i = 0; i < LY_GT_MAXW; ++i) {
    const int w = w0 + g0 + i * groups;
    okw[i] = i < cpt && w < W;
    wcl[i] = okw[i] ? w : (w0 < W ? w0 : 0);
#pragma unroll
    for (int q = 0; q < NQ; ++q) aw[i][q] = ly_ldg4(a_w + (n * W + wcl[i]) * C + c + 4 * q);
  }
  for (int h = h_lo; h < h_hi; ++h) {
    const long nh = n * H + h;
    f32x4 ah[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) ah[q] = ly_ldg4(a_h + nh * C + c + 4 * q);
    RV xr[LY_GT_MAXW], rr[LY_GT_MAXW];
#pragma unroll
    for (int i = 0; i < LY_GT_MAXW; ++i) {
      if (i >= cpt) break;                                                     // (uniform: columns per thread of this launch)
      const long row = nh * W + wcl[i];
      xr[i] = ly_ldrv<T>(x + row * ldx + c);
      if (res) rr[i] = ly_ldrv<T>(res + row * ldres + c);
    }
#pragma unroll
    for (int i = 0; i < LY_GT_MAXW; ++i) {
      if (i >= cpt) break;
      f32x4 v[NQ], r[NQ];
      ly_rv_unpack(xr[i], v);
      if (res) ly_rv_unpack(rr[i], r);
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        v[q] = v[q] * aw[i][q] * ah[q];
        if (res) v[q] += r[q];
      }
      if (okw[i]) *reinterpret_cast<RV*>(out + (nh * W + wcl[i]) * ldo + c) = ly_rv_pack(v, (RV*)nullptr);
    }
  }
}

extern "C" int ly_coordatt_gate(const void* x, int ldx, int n_img, int H, int W, int C, const float* a_h, const float* a_w,
                                const void* res, int ldres, void* out, int ldo, int dtype, void* stream) {
  LY_CHECK_DTYPE(dtype, "gate");
  const int vw = dtype == LY_BF16 ? 8 : 4;
  LY_CHECK(x && a_h && a_w && out && (C % vw) == 0 && (ldx % vw) == 0 && (ldo % vw) == 0 && (ldres % vw) == 0 && C / vw <= LY_THREADS,
           "gate: C = %d and the row strides must be multiples of %d (16-byte channel vectors)", C, vw);
  const int groups = LY_THREADS / (C / vw);
  int cpt = (W + groups - 1) / groups;
  if (cpt > LY_GT_MAXW) cpt = LY_GT_MAXW;
  const int slabs = (W + groups * cpt - 1) / (groups * cpt);
  const int bands = (H + LY_GT_RB - 1) / LY_GT_RB;
  LY_WITH_T(dtype, hipLaunchKernelGGL(ly_gate_kernel<T>, dim3((unsigned)((long)n_img * bands * slabs)), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                                      reinterpret_cast<const T*>(x), ldx, H, W, C, a_h, a_w, reinterpret_cast<const T*>(res), ldres, reinterpret_cast<T*>(out), ldo,
                                      bands, slabs, cpt));
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

// ---------------------------------------------------------------------------------------------------
// CoordAtt vector MLP, training backward (models/common.py:1600-1607 under autograd):
//   y0 = W1 pool + b1;  xh = (y0 - mean) * invstd;  y1 = gamma*xh + beta;  y2 = h_swish(y1);  a = sigmoid(Wx y2 + bx)
// with Wx = conv_h for the H row positions of an image and conv_w for its W column positions.  Two launches, because
// BatchNorm's backward needs sum(dy1) and sum(dy1*xh) over ALL positions before any dy0 exists:
//   bwd1 (one WAVE per position, lanes stride the channels, both length-C reductions are shuffle trees, nothing synchronises):
//         dz = da*a*(1-a) -> dpool buffer;  dy1 = (Wx^T dz) * h_swish'(y1);  (dy1, xh, y2) -> ws;  sums += (dy1, dy1*xh)  (striped)
//   bwd2 (lane = channel, block = 64 channels x a chunk of positions, waves = row phases):
//         dy0 = gamma*invstd*(dy1 - S1/R - xh*S2/R);  dpool = W1^T dy0 (over dz, in place);  dW1 += dy0 (x) pool;
//         dWx += dz (x) y2, dbx += dz;  dgamma += S2, dbeta += S1.   (db1 = sum dy0 is identically zero: BatchNorm removes the mean.)
// Every parameter gradient is summed in registers, then over the block's waves through LDS, and ADDED to its target once per block
// (a few dozen adds per address: same-address float atomics serialise, ~0.05 us each).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ly_hswish_grad(float x) { return x <= -3.f ? 0.f : (x >= 3.f ? 1.f : (2.f * x + 3.f) * (1.f / 6.f)); }
#define LY_CA_STRIPES 32

template <int MIP, int NS>
__global__ __launch_bounds__(LY_THREADS) void ly_coordatt_mlp_bwd1_kernel(
    const float* __restrict__ pool, int n_img, int H, int W, int C, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ wh, const float* __restrict__ ww, const float* __restrict__ a_h, const float* __restrict__ a_w,
    const float* __restrict__ da_h, const float* __restrict__ da_w, float* __restrict__ ws, double* __restrict__ sums, float* __restrict__ dzb) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = H + W;
  const long R = (long)n_img * L;
  float s1 = 0.f, s2 = 0.f;                                // the lane that owns output m: sum dy1[m], sum dy1[m]*xh[m]
  static_assert(MIP == 8 || MIP == 16, "ly_coordatt_mlp_bwd1: MIP = 8 or 16");
  constexpr int LSTEP = 64 / MIP;
  const int mine = lane / LSTEP;
  const bool owner = (lane % LSTEP) == 0;
  const float b1m = b1[mine], meanm = mean[mine], invm = invstd[mine], gm = gamma[mine], bem = beta[mine];
  const long nw = (long)gridDim.x * 4;
  for (long r = (long)blockIdx.x * 4 + wave; r < R; r += nw) {
    const long n = r / L;
    const int pos = (int)(r - n * L);
    const bool isrow = pos < H;
    const long q = isrow ? n * H + pos : n * W + (pos - H);
    const float* wx = isrow ? wh : ww;
    const float* am = (isrow ? a_h : a_w) + q * C;
    const float* dam = (isrow ? da_h : da_w) + q * C;
    float y[MIP], d[MIP];
#pragma unroll
    for (int m = 0; m < MIP; ++m) { y[m] = 0.f; d[m] = 0.f; }
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) {
      const int c = lane + 64 * sl;
      if (c < C) {
        const float pv = pool[r * C + c];
        const float av = am[c];
        const float dz = dam[c] * av * (1.f - av);
        dzb[r * C + c] = dz;
#pragma unroll
        for (int m = 0; m < MIP; ++m) {
          y[m] += w1[m * C + c] * pv;
          d[m] += dz * wx[c * MIP + m];
        }
      }
    }
    // both length-C reductions as reduce-scatters (ly_common.hpp): 2 (MIP - 1 + log2(64 / MIP)) cross-lane moves per position instead of 12 MIP;
    // output m ends up in lane m * (64 / MIP), which keeps its running sums
    ly_reduce_scatter<MIP>(y, lane);
    ly_reduce_scatter<MIP>(d, lane);
    if (owner) {
      const float xh = (y[0] + b1m - meanm) * invm;
      const float y1 = gm * xh + bem;
      const float g = d[0] * ly_hswish_grad(y1);
      s1 += g;
      s2 += g * xh;
      ws[r * 3 * MIP + mine] = g;
      ws[r * 3 * MIP + MIP + mine] = xh;
      ws[r * 3 * MIP + 2 * MIP + mine] = ly_hswish(y1);
    }
  }
  if (owner) {
    double* st = sums + ((blockIdx.x * 4 + wave) & (LY_CA_STRIPES - 1)) * 2 * MIP;      // double accumulators: see ly_stats_flush (ly_common.hpp)
    atomicAdd(st + mine, (double)s1);
    atomicAdd(st + MIP + mine, (double)s2);
  }
}

template <int MIP>
__global__ __launch_bounds__(LY_THREADS) void ly_coordatt_mlp_bwd2_kernel(
    const float* __restrict__ pool, int n_img, int H, int W, int C, long rows_per_block, const float* __restrict__ w1,
    const float* __restrict__ gamma, const float* __restrict__ invstd, const float* __restrict__ ws, const double* __restrict__ sums,
    float* __restrict__ dpool /* in: dz */, float* __restrict__ dw1, float* __restrict__ dgamma, float* __restrict__ dbeta,
    float* __restrict__ dwh, float* __restrict__ dbh, float* __restrict__ dww, float* __restrict__ dbw, const int f64) {
  constexpr int NA = 3 * MIP + 2;                          // accumulators per channel: dW1[m], dWh[m], dWw[m], dbh, dbw
  __shared__ float red[4 * 64 * (3 * MIP + 2)];
  __shared__ float ssum[2 * MIP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = H + W;
  const long R = (long)n_img * L;
  const int c = blockIdx.x * 64 + lane;
  const bool cok = c < C;
  if (tid < 2 * MIP) {
    double v = 0.0;
    for (int st = 0; st < LY_CA_STRIPES; ++st) v += sums[st * 2 * MIP + tid];
    ssum[tid] = (float)v;
  }
  __syncthreads();
  const float invR = 1.f / (float)R;
  float k0[MIP], m1[MIP], m2[MIP], w1r[MIP];
  float acc[NA];
#pragma unroll
  for (int m = 0; m < MIP; ++m) {
    k0[m] = gamma[m] * invstd[m];
    m1[m] = ssum[m] * invR;
    m2[m] = ssum[MIP + m] * invR;
    w1r[m] = cok ? w1[m * C + c] : 0.f;
  }
#pragma unroll
  for (int e = 0; e < NA; ++e) acc[e] = 0.f;
  const long r_lo = (long)blockIdx.y * rows_per_block;
  const long r_hi = r_lo + rows_per_block < R ? r_lo + rows_per_block : R;
  // four rows per trip, every load of the trip issued before the first use (the one-row loop paid a dependent round trip per row: 47 us
  // for 2.6 MB of pooled vectors); rows past the block's range re-read its last row and are masked
  constexpr int UR = 4;
  for (long r0 = r_lo + wave; r0 < r_hi; r0 += 4 * UR) {
    float pv[UR], dz[UR], wv[UR][3 * MIP];
    bool live[UR];
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      const long rr = r0 + 4 * u;
      live[u] = rr < r_hi;
      const long r = live[u] ? rr : r_hi - 1;
      const float* wr = ws + r * 3 * MIP;                  // wave-uniform row: (dy1, xh, y2)
#pragma unroll
      for (int m = 0; m < 3 * MIP; ++m) wv[u][m] = wr[m];
      pv[u] = cok ? pool[r * C + c] : 0.f;
      dz[u] = cok ? dpool[r * C + c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      const long r = r0 + 4 * u;
      const int pos = (int)(r % L);
      const bool isrow = pos < H;
      const float dzu = live[u] ? dz[u] : 0.f, pvu = live[u] ? pv[u] : 0.f;
      float g = 0.f;
#pragma unroll
      for (int m = 0; m < MIP; ++m) {
        const float dy0 = live[u] ? k0[m] * (wv[u][m] - m1[m] - wv[u][MIP + m] * m2[m]) : 0.f;
        const float t = dzu * wv[u][2 * MIP + m];
        g += dy0 * w1r[m];
        acc[m] += dy0 * pvu;
        acc[MIP + m] += isrow ? t : 0.f;
        acc[2 * MIP + m] += isrow ? 0.f : t;
      }
      acc[3 * MIP] += isrow ? dzu : 0.f;
      acc[3 * MIP + 1] += isrow ? 0.f : dzu;
      if (cok && live[u]) dpool[r * C + c] = g;
    }
  }
#pragma unroll
  for (int e = 0; e < NA; ++e) red[(wave * 64 + lane) * NA + e] = acc[e];
  __syncthreads();
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid < MIP) {
    ly_gacc(dgamma, tid, ssum[MIP + tid], f64);
    ly_gacc(dbeta, tid, ssum[tid], f64);
  }
  for (int e = tid; e < 64 * NA; e += LY_THREADS) {
    const int cl = e / NA, k = e - cl * NA;
    const int cc = blockIdx.x * 64 + cl;
    if (cc >= C) continue;
    const float v = red[e] + red[64 * NA + e] + red[2 * 64 * NA + e] + red[3 * 64 * NA + e];
    if (k < MIP) ly_gacc(dw1, k * C + cc, v, f64);
    else if (k < 2 * MIP) ly_gacc(dwh, cc * MIP + (k - MIP), v, f64);
    else if (k < 3 * MIP) ly_gacc(dww, cc * MIP + (k - 2 * MIP), v, f64);
    else if (k == 3 * MIP) ly_gacc(dbh, cc, v, f64);
    else ly_gacc(dbw, cc, v, f64);
  }
}

template <int MIP, int NS>
static void launch_coordatt_bwd(hipStream_t st, const float* pool, int n_img, int H, int W, int C, const float* w1, const float* b1, const float* mean,
                                const float* invstd, const float* gamma, const float* beta, const float* wh, const float* ww, const float* a_h,
                                const float* a_w, const float* da_h, const float* da_w, float* ws, double* sums, float* dpool, float* dw1,
                                float* dgamma, float* dbeta, float* dwh, float* dbh, float* dww, float* dbw, int f64) {
  const long R = (long)n_img * (H + W);
  long b1n = (R + 3) / 4;
  if (b1n > 1024) b1n = 1024;
  hipLaunchKernelGGL((ly_coordatt_mlp_bwd1_kernel<MIP, NS>), dim3((unsigned)b1n), dim3(LY_THREADS), 0, st, pool, n_img, H, W, C, w1, b1, mean, invstd, gamma,
                     beta, wh, ww, a_h, a_w, da_h, da_w, ws, sums, dpool);
  const int groups = (C + 63) / 64;
  long chunks = (96 + groups - 1) / groups;                // ~96 blocks; each target address then receives `chunks` same-address adds
  if (chunks > (R + 31) / 32) chunks = (R + 31) / 32;
  if (chunks < 1) chunks = 1;
  const long rpb = (R + chunks - 1) / chunks;
  chunks = (R + rpb - 1) / rpb;
  hipLaunchKernelGGL((ly_coordatt_mlp_bwd2_kernel<MIP>), dim3((unsigned)groups, (unsigned)chunks), dim3(LY_THREADS), 0, st, pool, n_img, H, W, C, rpb, w1,
                     gamma, invstd, ws, sums, dpool, dw1, dgamma, dbeta, dwh, dbh, dww, dbw, f64);
}

extern "C" int ly_coordatt_mlp_bwd(const float* pool, int n_img, int H, int W, int C, int mip, const float* w1, const float* b1,
                                   const float* mean, const float* invstd, const float* gamma, const float* beta, const float* wh,
                                   const float* ww, const float* a_h, const float* a_w, const float* da_h, const float* da_w, float* ws,
                                   double* sums, float* dpool, float* dw1, float* dgamma, float* dbeta, float* dwh, float* dbh,
                                   float* dww, float* dbw, int grads_f64, void* stream) {
  LY_CHECK(pool && w1 && b1 && mean && invstd && gamma && beta && wh && ww && a_h && a_w && da_h && da_w && ws && sums && dpool && dw1 &&
               dgamma && dbeta && dwh && dbh && dww && dbw, "coordatt_mlp_bwd: null pointer");
  LY_CHECK((mip == 8 || mip == 16) && C > 0 && C <= 512 && n_img > 0 && H > 0 && W > 0, "coordatt_mlp_bwd: built for mip 8 / 16 and C <= 512 (mip=%d C=%d)", mip, C);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define LY_CA_BWD(MIP, NS) launch_coordatt_bwd<MIP, NS>(st, pool, n_img, H, W, C, w1, b1, mean, invstd, gamma, beta, wh, ww, a_h, a_w, da_h, da_w, ws, sums, \
                                                        dpool, dw1, dgamma, dbeta, dwh, dbh, dww, dbw, grads_f64)
  const int ns = (C + 63) / 64;
  if (mip == 8) {
    if (ns <= 1) LY_CA_BWD(8, 1); else if (ns <= 2) LY_CA_BWD(8, 2); else if (ns <= 4) LY_CA_BWD(8, 4); else LY_CA_BWD(8, 8);
  } else {
    if (ns <= 4) LY_CA_BWD(16, 4); else LY_CA_BWD(16, 8);
  }
#undef LY_CA_BWD
  LY_LAUNCH_CHECK();
  return 0;
}
