// The weight-gradient family of the training step, gfx950: activations / activation gradients T = float or __bf16, dw fp32.
//
//   ly_wgrad_kernel                 the generic per-lane gather kernel: any width, NCHW images
//   ly_wgrad_tiled_kernel (+ group) LDS-staged tiles in quad or octet staging, partial tiles to a slab or float atomics
//   ly_wgrad_combine_kernel (+ group)  the fixed-order fold of a slab launch
//   WgPlan, wg_plan, wg_plan_group  the ONE statement of which kernel runs, on what grid, with what chunks and flush — the kernels above,
//                                   ly_wgrad1.hip (plain-row 1x1, bf16) and ly_wgrad3.hip (3x3 / stride 1 / pad 1, bf16) are launched from it
//   ly_wgrad, ly_wgrad_group, ly_wgrad_describe   the entry points: plan, then launch the plan or print its kernel's name
//
// Replaces what autograd derives for the weights of Conv2d in the reference's `scaler.scale(loss).backward()` (train.py:324) over
// models/common.py:1890-1910 (Conv), :1478-1482 (MLPBlock), :1537-1561 (patch layers).
#include "ly_tile.hpp"
#include "ly_params.h"
#include "ly_wgrad.hpp"
#include <stdio.h>
#include <stdlib.h>

// -------------------------------------------------------------------------------------------------
// Weight gradient:  dw[n][tap*Cin + c] += sum_{p in pixels} du[p][n] * X[src(p, tap)][c]
//
// The contraction index is the PIXEL, which is the slow index of both operands in memory (NHWC rows), so
// the MFMA fragments are gathered straight from global memory with per-lane dword loads: lane (i, q) of a
// 16x16x32 step reads channel (tile*16 + i) of the 8 pixels p0 + 8q + j.  At fixed j the 16 lanes of a
// quarter-wave read 64 contiguous bytes of one pixel row, so every load instruction moves four full 64-byte
// segments.  The same per-lane addressing makes the forward's gathers (3x3 taps with zero padding, k=s patch
// gathers of an NHWC map or an NCHW image, the nearest-2x upsampled read) a pure address computation.
// bf16x3 products, fp32 accumulation.  Block = 64 x 64 output tile (wave = 32 x 32), grid.y splits the pixels;
// partial sums are added to dw with float atomics (dw is zeroed by the caller).
// -------------------------------------------------------------------------------------------------
template <typename T, bool ROWS>
__global__ __launch_bounds__(LY_THREADS) void ly_wgrad_kernel(const LyWgradParams P, const int tiles_k, const long chunk_px) {
  constexpr int PL = LyT<T>::PL;
  const T* const du = reinterpret_cast<const T*>(P.du);
  const T* const xin = reinterpret_cast<const T*>(P.x);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lq = lane >> 4;
  const int tk = blockIdx.x % tiles_k, tn = blockIdx.x / tiles_k;
  const int n_base = tn * 64 + (wave & 1) * 32, k_base = tk * 64 + (wave >> 1) * 32;
  const long p_begin = (long)blockIdx.y * chunk_px;
  const long p_end = p_begin + chunk_px < P.M ? p_begin + chunk_px : P.M;
  const int Ktot = P.ks * P.ks * P.Cin;

  int arow[2], bcol[2], ky[2], kx[2], cc[2];
  bool aok[2], bok[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int r = n_base + 16 * t + li;
    aok[t] = r < P.N;
    arow[t] = aok[t] ? r : 0;
    const int c = k_base + 16 * t + li;
    bok[t] = c < Ktot;
    bcol[t] = bok[t] ? c : 0;
    const int tap = bcol[t] / P.Cin;
    cc[t] = bcol[t] - tap * P.Cin;
    ky[t] = tap / P.ks;
    kx[t] = tap - ky[t] * P.ks;
  }
  const int Hv = P.up2 ? 2 * P.Hin : P.Hin, Wv = P.up2 ? 2 * P.Win : P.Win;
  const float invW = 1.f / (float)P.W, invH = 1.f / (float)P.H;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = ly_zero4();

  for (long p0 = p_begin; p0 < p_end; p0 += 32) {
    float av[2][8], bv[2][8];
    const long pf = p0 + 8 * lq;
    int n_i = 0, ho = 0, wo = 0;
    if (!ROWS) {
      const int g = (int)(pf < P.M ? pf : P.M - 1);
      const int row = ly_fdiv(g, P.W, invW);
      wo = g - row * P.W;
      n_i = ly_fdiv(row, P.H, invH);
      ho = row - n_i * P.H;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long p = pf + j;
      const bool pok = p < p_end;
      const long pc = pok ? p : p_end - 1;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float v = ly_ld1<T>(du + pc * P.lddu + arow[t]);
        av[t][j] = (pok && aok[t]) ? v : 0.f;
      }
      if (ROWS) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const float v = ly_ld1<T>(xin + pc * P.ldx + bcol[t]);
          bv[t][j] = (pok && bok[t]) ? v : 0.f;
        }
      } else {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          int hi = ho * P.stride + ky[t] - P.pad, wi = wo * P.stride + kx[t] - P.pad;
          const bool ok = pok && bok[t] && hi >= 0 && hi < Hv && wi >= 0 && wi < Wv;
          if (P.up2) { hi >>= 1; wi >>= 1; }
          long off = P.nchw ? (((long)n_i * P.Cin + cc[t]) * P.Hin + hi) * P.Win + wi
                            : (((long)n_i * P.Hin + hi) * P.Win + wi) * P.ldx + cc[t];
          const float v = ly_ld1<T>(xin + (ok ? off : 0));
          bv[t][j] = ok ? v : 0.f;
        }
        if (++wo == P.W) { wo = 0; if (++ho == P.H) { ho = 0; ++n_i; } }
      }
    }
    bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      ly_split8(av[t], ah[t], al[t]);
      ly_split8(bv[t], bh[t], bl[t]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = ly_mfmapp<PL>(ah[i], al[i], bh[j], bl[j], acc[i][j]);
  }

  // D: lane (i = column, q) holds rows 4q + r
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = k_base + 16 * j + li;
      if (col >= Ktot) continue;
      const int tap = col / P.Cin, cch = col - tap * P.Cin;
      if (cch >= P.c_valid) continue;
      const long cidx = (long)tap * P.dw_ts + (long)cch * P.dw_cs;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = n_base + 16 * i + 4 * lq + r;
        if (row < P.n_valid) atomicAdd(P.dw + (long)row * P.lddw + cidx, acc[i][j][r]);
      }
    }
}


// -------------------------------------------------------------------------------------------------
// Tiled weight gradient (the fast path: N, Cin, lddu, ldx multiples of 4, NHWC input).
// Block = BN x BK output tile, 4 waves as 2 x 2, wave tile (BN/2) x (BK/2) = 64 accumulator registers.
// Per step of P pixels (32, or 64 for skinny outputs) the block stages the [P px][BN] slab of du and the gathered [P px][BK]
// slab of x ONCE:
// a thread owns one channel quad x one group of 8 consecutive pixels, i.e. 8 coalesced float4 row loads (a wave reads
// 512 contiguous bytes per pixel row), transposes them in registers and writes, per channel, the 8 pixels as ONE
// 16-byte bf16 vector into the hi / lo planes  plane[channel][P px].  An MFMA fragment (lane (i, q):
// channel i, pixels 8q..8q+7) is then a single conflict-free ds_read_b128, for both operands.  Global loads of step
// s+1 are in flight while step s is contracted (register prefetch, two LDS buffers, one barrier per step).
// Re-reads drop from (N/64 + K/64) to (N/BN + K/BK) passes over the two tensors.
// -------------------------------------------------------------------------------------------------
// SLAB: 0 = atomic flush only, 1 = slab when the pointer is given (run-time), 2 = slab always (the grouped launch's instantiation: a second flush
// path compiled into it de-pipelined its pixel loop)
template <typename T, int BN, int BK, int P, bool ROWS, bool PRO, int SLAB = 1, bool OCT = false>
__device__ __forceinline__ void ly_wgrad_tiled_body(const LyWgradParams& Q, const int tile_idx, const int chunk_idx, const int tiles_k, const long chunk_px,
                                                    float* __restrict__ const slab, const int tiles) {
  using R4 = typename LyT<T>::R4;
  constexpr int PL = LyT<T>::PL;
  const T* const du = reinterpret_cast<const T*>(Q.du);
  const T* const xin = reinterpret_cast<const T*>(Q.x);
  constexpr int PG = P / 8;                             // 8-pixel groups per step
  constexpr int TASKS = (BN / 4 + BK / 4) * PG;         // (channel quad, pixel group) pairs per step
  constexpr int TPT = (TASKS + LY_THREADS - 1) / LY_THREADS;
  constexpr int NI = BN / 32, NJ = BK / 32;             // MFMA tiles per wave along n / k
  // LDS image of a step: [plane hi | lo][pixel group g of 8][row slot][8 px bf16 = 16 bytes].  A fragment read (ds_read_b128: lane (i, q) takes
  // row i, pixel group 4 ks + q) walks 16 consecutive row slots per pixel group, and a commit (4 channel rows x 16 bytes per thread, threads on
  // consecutive channel quads) must not put rows 4 cq + e of neighbouring threads 64 bytes apart — so row r sits at slot (r & 3) (NR/4 + 4) +
  // (r >> 2): for a fixed e consecutive threads write consecutive slots, and rows 0 .. 15 of a fragment land on 16 different slots modulo 16
  // ((r & 3) * 4 + (r >> 2): a 4 x 4 transpose).  Both conflict-free; the round-5 image ([row][P px] with 16 bytes of row padding) read with one
  // 2-way slot per lane group and wrote 4-way: SQ_LDS_BANK_CONFLICT = 24 % of the grouped kernel's cycles (profiles/r05_train_bf16_pmc_wait.txt).
  constexpr int NR = BN + BK;
  constexpr int PLANE = (NR + 16) * 16;                 // bytes per pixel group
  constexpr int BUF = PL * PG * PLANE;
  // OC (round 6; bf16 storage, plain rows, every width / stride a multiple of 8): a staging task is a channel OCTET x 8 pixels = eight 16-byte
  // row loads (a wave reads four 256-byte row pieces per instruction) instead of a quad x 8 pixels = eight 8-byte loads: half the vector-memory
  // instructions per step, and 16-byte accesses (the 8-byte form streams at 0.54-0.70 of their rate: MI355X guide, HBM section; the kernels sat
  // at 2.6-3.5 TB/s).  The 8 x 8 transpose is 32 v_perm_b32 per task (the quads' 4 x 8: 16) — the same count per byte.  Row r then sits at slot
  // (r & 7) (NR/8 + 2) + (r >> 3): for a fixed channel-in-octet consecutive threads write consecutive slots, and rows 0 .. 15 of a fragment land
  // on the 16 slots (r & 7) * 2 + (r >> 3) modulo 16 (NR/8 + 2 = 2 mod 16 for NR = 64, 96, 128, 160, 192, 256).
  constexpr bool OC = OCT && LyT<T>::BF;                // (gathered inputs too: an octet lies inside one tap when Cin is a multiple of 8)
  static_assert(!OC || ((NR / 8 + 2) % 16 == 2 || (NR / 8 + 2) % 16 == 10 || (NR / 8 + 2) % 16 == 6 || (NR / 8 + 2) % 16 == 14), "octet row map: fragment rows must hit 16 slots");
  auto rowoff = [](int r) -> int { return OC ? ((r & 7) * (NR / 8 + 2) + (r >> 3)) * 16 : ((r & 3) * (NR / 4 + 4) + (r >> 2)) * 16; };
  constexpr int ISTEP = OC ? 32 : 64;                   // bytes between the row slots of rows r and r + 16
  constexpr int TASKS8 = (BN / 8 + BK / 8) * PG, TPT8 = (TASKS8 + LY_THREADS - 1) / LY_THREADS;
  extern __shared__ f32x4 ly_smem4[];
  char* const lds = reinterpret_cast<char*>(ly_smem4);
  constexpr bool SB = PL * P >= 128;       // 128 bf16 / 64 fp32 pixels per step: ONE LDS buffer (see the loop below)
  float* const sab = reinterpret_cast<float*>(lds + (SB ? 1 : 2) * BUF);      // [scale BK | shift BK] of the optional x prologue
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lq = lane >> 4;
  const int tk = tile_idx % tiles_k, tn = tile_idx / tiles_k;
  const int n0 = tn * BN, k0 = tk * BK;
  const long p_begin = (long)chunk_idx * chunk_px;
  const long p_end = p_begin + chunk_px < Q.M ? p_begin + chunk_px : Q.M;
  const int Ktot = Q.ks * Q.ks * Q.Cin;
  // x prologue max(x*scale + shift, 0) (LyWgradParams.x_scale): the block's BK columns of both vectors staged once; applied while the x slab
  // is transposed into LDS (masked pixels meet zero rows of du, so relu(shift) there is harmless; masked columns get scale = shift = 0)
  // PRO: the instantiation that can; a group may mix problems with and without vectors (pro is uniform over the block).  Straight-line on
  // purpose — a load under a branch makes every later s_waitcnt conservative (the first version, `if (pro) { loads }`, doubled the kernel's
  // time): all threads load (a problem without vectors reads the head of x as a harmless stand-in), the select happens on values.
  const bool pro = ROWS && PRO && Q.x_scale != nullptr;
  if constexpr (ROWS && PRO) {
    const float* const sp = pro ? Q.x_scale : reinterpret_cast<const float*>(Q.x);      // (4*Cin bytes of x exist: M >= 2 rows)
    const float* const hp = pro ? Q.x_shift : reinterpret_cast<const float*>(Q.x);
    const int i = tid & (BK - 1);
    const int k = k0 + i < Ktot ? k0 + i : 0;
    const float sv = sp[k], hv = hp[k];
    sab[i] = k0 + i < Ktot ? sv : 0.f;
    sab[BK + i] = k0 + i < Ktot ? hv : 0.f;
    __syncthreads();
  }

  // ---- per-task constants ---------------------------------------------------------------------
  bool t_isA[TPT], t_ok[TPT];
  int t_row[TPT], t_g[TPT], t_c[TPT], t_ky[TPT], t_kx[TPT];
#pragma unroll
  for (int u = 0; u < TPT; ++u) {
    const int t = tid + u * LY_THREADS;
    const bool live = t < TASKS;
    t_isA[u] = t < (BN / 4) * PG;
    const int tt = t_isA[u] ? t : t - (BN / 4) * PG;
    const int quads = t_isA[u] ? BN / 4 : BK / 4;
    const int cq = tt % quads;
    t_g[u] = (tt / quads) % PG;
    t_row[u] = (t_isA[u] ? 0 : BN) + 4 * cq;            // first of the 4 LDS rows this task writes
    if (t_isA[u]) {
      t_c[u] = n0 + 4 * cq;
      t_ok[u] = live && t_c[u] < Q.N;
      t_ky[u] = t_kx[u] = 0;
    } else {
      const int col = k0 + 4 * cq;
      t_ok[u] = live && col < Ktot;
      const int cc = t_ok[u] ? col : 0;
      const int tap = cc / Q.Cin;
      t_c[u] = cc - tap * Q.Cin;
      t_ky[u] = tap / Q.ks;
      t_kx[u] = tap - t_ky[u] * Q.ks;
    }
    if (!live) t_row[u] = -1;
  }
  const int Hv = Q.up2 ? 2 * Q.Hin : Q.Hin, Wv = Q.up2 ? 2 * Q.Win : Q.Win;
  const float invW = 1.f / (float)Q.W, invH = 1.f / (float)Q.H;

  // DEFER (the grouped slab instantiation): the loads of a step are pure — masked pixels are zeroed when the registers are committed to LDS,
  // not right behind each load.  With the select behind the load hipcc's scheduler, in THIS instantiation, sank every load next to its
  // select: one `s_waitcnt vmcnt(0)` per load, the pixel loop ran at one memory round trip per 8 bytes (53 -> 108 us per launch).
  constexpr bool DEFER = SLAB == 2 && ROWS;      // (the same change in the single-problem instantiations: 32.6 -> 37.7 us — only where the scheduler had gone wrong)
  long pre_p0 = 0;
  R4 pre[TPT][8];
  auto prefetch = [&](long p0) {
    pre_p0 = p0;
#pragma unroll
    for (int u = 0; u < TPT; ++u) {
      const long pf = p0 + 8 * t_g[u];
      int n_i = 0, ho = 0, wo = 0;
      if (!ROWS && !t_isA[u]) {
        const int g = (int)(pf < Q.M ? pf : Q.M - 1);
        const int row = ly_fdiv(g, Q.W, invW);
        wo = g - row * Q.W;
        n_i = ly_fdiv(row, Q.H, invH);
        ho = row - n_i * Q.H;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const long p = pf + j;
        bool ok = t_ok[u] && p < p_end;
        const T* src;
        if (t_isA[u]) {
          src = du + (ok ? p : p_begin) * Q.lddu + t_c[u];
        } else if (ROWS) {
          src = xin + (ok ? p : p_begin) * Q.ldx + t_c[u];
        } else {
          int hi = ho * Q.stride + t_ky[u] - Q.pad, wi = wo * Q.stride + t_kx[u] - Q.pad;
          ok = ok && hi >= 0 && hi < Hv && wi >= 0 && wi < Wv;
          if (Q.up2) { hi >>= 1; wi >>= 1; }
          src = xin + (ok ? (((long)n_i * Q.Hin + hi) * Q.Win + wi) * Q.ldx : 0) + t_c[u];
          if (++wo == Q.W) { wo = 0; if (++ho == Q.H) { ho = 0; ++n_i; } }
        }
        R4 v = ly_ldr4<T>(src);
        if constexpr (!DEFER) {
          if (!ok) ly_zero_raw(v);
        }
        pre[u][j] = v;
      }
    }
  };
  auto commit = [&](int buf) {
    char* base = lds + buf * BUF;
#pragma unroll
    for (int u = 0; u < TPT; ++u) {
      if (t_row[u] < 0) continue;
      if constexpr (DEFER) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (!(t_ok[u] && pre_p0 + 8 * t_g[u] + j < p_end)) ly_zero_raw(pre[u][j]);
      }
      const bool pb = pro && !t_isA[u];
      f32x4 sa = ly_zero4(), sh = ly_zero4();
      if constexpr (ROWS && PRO) {
        const int lc = t_isA[u] ? 0 : t_row[u] - BN;
        sa = *reinterpret_cast<const f32x4*>(sab + lc);
        sh = *reinterpret_cast<const f32x4*>(sab + BK + lc);
      }
      if constexpr (PL == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v[8] = {pre[u][0][e], pre[u][1][e], pre[u][2][e], pre[u][3][e], pre[u][4][e], pre[u][5][e], pre[u][6][e], pre[u][7][e]};
          if constexpr (ROWS && PRO) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = pb ? fmaxf(v[j] * sa[e] + sh[e], 0.f) : v[j];
          }
          bf16x8 hi, lo;
          ly_split8(v, hi, lo);
          char* d = base + t_g[u] * PLANE + t_row[u] * 4 + e * ((NR / 4 + 4) * 16);      // rowoff(t_row + e), t_row a multiple of 4
          *reinterpret_cast<bf16x8*>(d) = hi;
          *reinterpret_cast<bf16x8*>(d + PG * PLANE) = lo;
        }
      } else {
        // bf16 storage: a pure 8 x 4 transpose of 16-bit values (channel e of the 8 pixels becomes one 16-byte row piece)
        bf16x4 q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = __builtin_bit_cast(bf16x4, pre[u][j]);
        if constexpr (ROWS && PRO) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            f32x4 v = ly_cvt4(q[j]) * sa + sh;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            const bf16x4 r = ly_cvtb4(v);
            q[j] = pb ? r : q[j];
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bf16x8 row = {q[0][e], q[1][e], q[2][e], q[3][e], q[4][e], q[5][e], q[6][e], q[7][e]};
          *reinterpret_cast<bf16x8*>(base + t_g[u] * PLANE + t_row[u] * 4 + e * ((NR / 4 + 4) * 16)) = row;      // rowoff(t_row + e), t_row a multiple of 4
        }
      }
    }
  };

  // ---- the octet form of the same two steps -------------------------------------------------------
  bool o_isA[OC ? TPT8 : 1], o_ok[OC ? TPT8 : 1];
  int o_row[OC ? TPT8 : 1], o_g[OC ? TPT8 : 1], o_c[OC ? TPT8 : 1], o_ky[OC ? TPT8 : 1], o_kx[OC ? TPT8 : 1];
  ly_u32x4 pre8[OC ? TPT8 : 1][OC ? 8 : 1];
  if constexpr (OC) {
#pragma unroll
    for (int u = 0; u < TPT8; ++u) {
      const int t = tid + u * LY_THREADS;
      const bool live = t < TASKS8;
      o_isA[u] = t < (BN / 8) * PG;
      const int tt = o_isA[u] ? t : t - (BN / 8) * PG;
      const int octs = o_isA[u] ? BN / 8 : BK / 8;
      const int co = tt % octs;
      o_g[u] = (tt / octs) % PG;
      o_row[u] = live ? (o_isA[u] ? 0 : BN) + 8 * co : -1;
      o_c[u] = (o_isA[u] ? n0 : k0) + 8 * co;
      o_ok[u] = live && o_c[u] < (o_isA[u] ? Q.N : Ktot);
      o_ky[u] = o_kx[u] = 0;
      if (!ROWS && !o_isA[u]) {                              // gathered input: column -> (tap, channel inside the tap)
        const int cc = o_ok[u] ? o_c[u] : 0;
        const int tap = cc / Q.Cin;
        o_c[u] = cc - tap * Q.Cin;
        o_ky[u] = tap / Q.ks;
        o_kx[u] = tap - o_ky[u] * Q.ks;
      }
    }
  }
  auto prefetch8 = [&](long p0) {
    pre_p0 = p0;
#pragma unroll
    for (int u = 0; u < (OC ? TPT8 : 0); ++u) {
      const long pf = p0 + 8 * o_g[u];
      int n_i = 0, ho = 0, wo = 0;
      if (!ROWS && !o_isA[u]) {
        const int g = (int)(pf < Q.M ? pf : Q.M - 1);
        const int row = ly_fdiv(g, Q.W, invW);
        wo = g - row * Q.W;
        n_i = ly_fdiv(row, Q.H, invH);
        ho = row - n_i * Q.H;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const long p = pf + j;
        bool ok = o_ok[u] && p < p_end;
        const T* src;
        if (o_isA[u]) {
          src = du + (ok ? p : p_begin) * Q.lddu + (ok ? o_c[u] : 0);
        } else if (ROWS) {
          src = xin + (ok ? p : p_begin) * Q.ldx + (ok ? o_c[u] : 0);
        } else {
          int hi = ho * Q.stride + o_ky[u] - Q.pad, wi = wo * Q.stride + o_kx[u] - Q.pad;
          ok = ok && hi >= 0 && hi < Hv && wi >= 0 && wi < Wv;
          if (Q.up2) { hi >>= 1; wi >>= 1; }
          src = xin + (ok ? (((long)n_i * Q.Hin + hi) * Q.Win + wi) * Q.ldx + o_c[u] : 0);
          if (++wo == Q.W) { wo = 0; if (++ho == Q.H) { ho = 0; ++n_i; } }
        }
        ly_u32x4 v = *reinterpret_cast<const ly_u32x4*>(src);
        if constexpr (!DEFER) {
          if (!ok) v = (ly_u32x4){0u, 0u, 0u, 0u};
        }
        pre8[u][j] = v;
      }
    }
  };
  auto commit8 = [&](int buf) {
    char* base = lds + buf * BUF;
#pragma unroll
    for (int u = 0; u < (OC ? TPT8 : 0); ++u) {
      if (o_row[u] < 0) continue;
      if constexpr (DEFER) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (!(o_ok[u] && pre_p0 + 8 * o_g[u] + j < p_end)) pre8[u][j] = (ly_u32x4){0u, 0u, 0u, 0u};
      }
      if constexpr (PRO) {
        if (pro && !o_isA[u]) {
          const int lc = o_row[u] - BN;
          const f32x4 sa0 = *reinterpret_cast<const f32x4*>(sab + lc), sa1 = *reinterpret_cast<const f32x4*>(sab + lc + 4);
          const f32x4 sh0 = *reinterpret_cast<const f32x4*>(sab + BK + lc), sh1 = *reinterpret_cast<const f32x4*>(sab + BK + lc + 4);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            f32x4 q[2];
            ly_rv_unpack(pre8[u][j], q);
            q[0] = q[0] * sa0 + sh0;
            q[1] = q[1] * sa1 + sh1;
#pragma unroll
            for (int e = 0; e < 4; ++e) { q[0][e] = fmaxf(q[0][e], 0.f); q[1][e] = fmaxf(q[1][e], 0.f); }
            pre8[u][j] = ly_rv_pack(q, (ly_u32x4*)nullptr);
          }
        }
      }
      // 8 pixels x 8 channels of 16 bits -> channel e: its 8 pixels as one 16-byte row piece (dword k = pixels 2k, 2k + 1)
      char* const d0 = base + o_g[u] * PLANE + (o_row[u] >> 3) * 16;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        ly_u32x4 row;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          row[k] = __builtin_amdgcn_perm(pre8[u][2 * k + 1][e >> 1], pre8[u][2 * k][e >> 1], (e & 1) ? 0x07060302u : 0x05040100u);
        *reinterpret_cast<ly_u32x4*>(d0 + e * ((NR / 8 + 2) * 16)) = row;            // rowoff(o_row + e), o_row a multiple of 8
      }
    }
  };
  auto prefetch_any = [&](long p0) { if constexpr (OC) prefetch8(p0); else prefetch(p0); };
  auto commit_any = [&](int buf) { if constexpr (OC) commit8(buf); else commit(buf); };

  f32x4 acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = ly_zero4();
  const int wn = (wave & 1) * (BN / 2), wk = BN + (wave >> 1) * (BK / 2);
  // the lane's fragment addresses: everything else is an immediate (wn, wk multiples of 16: rows r + 16 m sit m * ISTEP bytes further)
  const int rd_a = lq * PLANE + rowoff(li) + (wn / 16) * ISTEP, rd_b = lq * PLANE + rowoff(li) + (wk / 16) * ISTEP;

  // SB: ONE LDS buffer (two would leave one block per CU); the loads of the next step are in flight during the contraction, the buffer is
  prefetch_any(p_begin);                   // rewritten between two barriers
  commit_any(0);
  __syncthreads();
  int buf = 0;
  for (long p0 = p_begin; p0 < p_end; p0 += P) {
    const bool more = p0 + P < p_end;
    if (more) prefetch_any(p0 + P);
    const char* base = lds + buf * BUF;
#pragma unroll
    for (int ks = 0; ks < P / 32; ++ks) {
      bf16x8 ah[NI], al[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const char* r = base + rd_a + ks * (4 * PLANE) + i * ISTEP;     // row wn + 16 i + li: wn and 16 i are multiples of 16 (4 / 2 slots of 16 bytes per 16 rows)
        ah[i] = *reinterpret_cast<const bf16x8*>(r);
        al[i] = PL == 2 ? *reinterpret_cast<const bf16x8*>(r + (PL - 1) * PG * PLANE) : ah[i];
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const char* r = base + rd_b + ks * (4 * PLANE) + j * ISTEP;
        const bf16x8 bh = *reinterpret_cast<const bf16x8*>(r);
        const bf16x8 bl = PL == 2 ? *reinterpret_cast<const bf16x8*>(r + (PL - 1) * PG * PLANE) : bh;
#pragma unroll
        for (int i = 0; i < NI; ++i) acc[i][j] = ly_mfmapp<PL>(ah[i], al[i], bh, bl, acc[i][j]);
      }
    }
    if constexpr (SB) {
      __syncthreads();
      if (more) commit_any(0);
      __syncthreads();
    } else {
      if (more) commit_any(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }

  if (SLAB == 2 || (SLAB == 1 && slab)) {
    // the chunk's tile [BN][BK] into its own slab with plain stores (16 lanes = 64 contiguous bytes); ly_wgrad_combine folds the chunks in a
    // fixed order: no float atomics (the atomic flush of 512 x 64 KB was a quarter of a launch), bit-reproducible dw
    float* const sl = slab + ((long)chunk_idx * tiles + tile_idx) * (BN * BK);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int lc = (wave >> 1) * (BK / 2) + 16 * j + li;
        const int col = k0 + lc;
        if (col >= Ktot) continue;
        const int tap = col / Q.Cin, cch = col - tap * Q.Cin;
        if (cch >= Q.c_valid) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int lr = wn + 16 * i + 4 * lq + r;
          if (n0 + lr < Q.n_valid) sl[lr * BK + lc] = acc[i][j][r];
        }
      }
    return;
  }
  if constexpr (SLAB != 2) {
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = k0 + (wave >> 1) * (BK / 2) + 16 * j + li;
      if (col >= Ktot) continue;
      const int tap = col / Q.Cin, cch = col - tap * Q.Cin;
      if (cch >= Q.c_valid) continue;
      const long cidx = (long)tap * Q.dw_ts + (long)cch * Q.dw_cs;     // (tap, channel) -> position inside a dw row: the weight's own layout
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = n0 + wn + 16 * i + 4 * lq + r;
        if (row < Q.n_valid) atomicAdd(Q.dw + (long)row * Q.lddw + cidx, acc[i][j][r]);
      }
    }
  }
}

// dw[n][tap][c] += sum over chunks of slab[chunk][tile][row][col] in a fixed order, one writer per element (the second launch of a tiled
// weight gradient whose chunks left their tiles in LyWgradParams.ws).  Block = 64 slab columns x rls row lanes; this is the decode of a slab
// column into (row, tap, channel), the sum is ly_wgrad_fold (ly_wgrad.hpp).
__device__ __forceinline__ void ly_wgrad_combine_body(const LyWgradParams& P, const float* __restrict__ slab, const int chunks, const int tiles_k,
                                                      const int tiles, const int BN, const int BK, const long blk, const int rls) {
  const long E = (long)tiles * BN * BK;
  const long e = blk * 64 + (threadIdx.x & 63);
  const int tile = (int)(e / (BN * BK));
  const int rem = (int)(e - (long)tile * (BN * BK));
  const int lr = rem / BK, lc = rem - lr * BK;
  const int tk = tile % tiles_k, tn = tile / tiles_k;
  const int row = tn * BN + lr, col = tk * BK + lc;
  const int tap = col / P.Cin, cch = col - tap * P.Cin;
  const bool live = e < E && row < P.n_valid && col < P.ks * P.ks * P.Cin && cch < P.c_valid;
  ly_wgrad_fold(slab + e, E, chunks, rls, live, P.dw + (long)row * P.lddw + (long)tap * P.dw_ts + (long)cch * P.dw_cs);
}
__global__ __launch_bounds__(1024) void ly_wgrad_combine_kernel(const LyWgradParams P, const float* __restrict__ slab, const int chunks, const int tiles_k,
                                                               const int tiles, const int BN, const int BK, const int rls) {
  ly_wgrad_combine_body(P, slab, chunks, tiles_k, tiles, BN, BK, (long)blockIdx.x, rls);
}
static void wgrad_combine_launch(const LyWgradParams& P, const float* slab, long chunks, int tiles_k, long tiles, int BN, int BK, hipStream_t st) {
  const long E = tiles * BN * BK;
  const int rls = chunks <= 192 ? 4 : 16;                 // row lanes: see ly_wgrad_fold
  hipLaunchKernelGGL(ly_wgrad_combine_kernel, dim3((unsigned)((E + 63) / 64)), dim3(64 * rls), 0, st, P, slab, (int)chunks, tiles_k, (int)tiles, BN, BK, rls);
}

template <typename T, int BN, int BK, int P, bool ROWS, bool PRO = false, bool OCT = false>
__global__ __launch_bounds__(LY_THREADS) __attribute__((amdgpu_waves_per_eu(BN + BK > 160 ? 2 : 3))) void ly_wgrad_tiled_kernel(const LyWgradParams P_, const int tiles_k, const long chunk_px, float* const slab) {
  // (no XCD-aware re-ordering here: tile / chunk computed from the remapped id with a run-time division made hipcc treat them as per-lane values —
  // the 128 x 128 rows form took 3x as long, 45 -> 146 us per launch; forced back to scalars (readfirstlane) it fetched a third less from HBM
  // but still ran 45 -> 50 us, the other forms +-1 us.  The grouped kernel, ly_wgrad3 and the other tile kernels keep the remap.)
  ly_wgrad_tiled_body<T, BN, BK, P, ROWS, PRO, 1, OCT>(P_, (int)blockIdx.x, (int)blockIdx.y, tiles_k, chunk_px, slab, (int)gridDim.x);
}

// Several independent weight gradients of ONE tile class in one launch (ly_wgrad_group): the problems share the ~512 blocks, so each block
// walks a longer pixel chunk — the fixed cost of a block (first-load latency, the atomic flush of its 64 KB tile) is paid half / a third as
// often per pixel, and the launch fills the chip where a lone small problem leaves a ragged second wave.  (LyWgradGroupArgs: ly_wgrad.hpp)
template <typename T, int BN, int BK, int P, bool ROWS, bool PRO = false, bool GSLAB = false, bool OCT = false>
__global__ __launch_bounds__(LY_THREADS) __attribute__((amdgpu_waves_per_eu(BN + BK > 160 ? 2 : 3))) void ly_wgrad_tiled_group_kernel(const LyWgradGroupArgs G) {
  const int bid = ly_xcd_remap((int)blockIdx.x, (int)gridDim.x);            // (see ly_wgrad_tiled_kernel)
  int g = 0;
#pragma unroll
  for (int i = 1; i < LY_WGRAD_GROUP_MAX; ++i)
    if (i < G.n && bid >= G.blk0[i]) g = i;
  g = __builtin_amdgcn_readfirstlane(g);
  const int local = bid - G.blk0[g];
  const int tiles = G.tiles[g];
  // (no slab path here: with it compiled in, every wait of this instantiation's pixel loop became `s_waitcnt vmcnt(0)` — 53 -> 107 us per launch;
  // a grouped launch keeps the atomic flush, whose cost the longer pixel runs per block already halve)
  // GSLAB: every block leaves its tile in the problem's slab (plain stores) and ly_wgrad_combine_group_kernel folds the chunks in index order —
  // no float atomics: the grouped weight gradients are the same bits in every run
  ly_wgrad_tiled_body<T, BN, BK, P, ROWS, PRO, GSLAB ? 2 : 0, OCT>(G.p[g], local % tiles, local / tiles, G.tiles_k[g], G.chunk_px[g], GSLAB ? G.slab[g] : nullptr, tiles);
}
// the combine launches of a group's problems as ONE launch
__global__ __launch_bounds__(1024) void ly_wgrad_combine_group_kernel(const LyWgradGroupArgs G, const int BN, const int BK, const int rls) {
  int g = 0;
#pragma unroll
  for (int i = 1; i < LY_WGRAD_GROUP_MAX; ++i)
    if (i < G.n && (int)blockIdx.x >= G.cblk0[i]) g = i;
  g = __builtin_amdgcn_readfirstlane(g);
  ly_wgrad_combine_body(G.p[g], G.slab[g], G.chunks[g], G.tiles_k[g], G.tiles[g], BN, BK, (long)((int)blockIdx.x - G.cblk0[g]), rls);
}

// blocks a weight-gradient launch aims for (development builds, `make DEVEL=1`, read LY_WG_BLOCKS / LY_WG_GROUP_BLOCKS)
static long wg_target_blocks(bool group) {
#ifdef LY_DEVEL
  static long t[2] = {0, 0};
  if (!t[group]) {
    const char* e = getenv(group ? "LY_WG_GROUP_BLOCKS" : "LY_WG_BLOCKS");
    t[group] = e && atol(e) > 0 ? atol(e) : 512;
  }
  return t[group];
#else
  (void)group;
  return 512;
#endif
}

// the octet staging of ly_wgrad_tiled_body applies: bf16 storage, both operands' widths, strides and addresses in whole 16-byte vectors
template <typename T>
static bool wgrad_octets(const LyWgradParams& Q) {
  if constexpr (!LyT<T>::BF) return false;
#ifdef LY_DEVEL
  static int off = -1;
  if (off < 0) { const char* e = getenv("LY_WG_NO_OCT"); off = e && atoi(e) ? 1 : 0; }
  if (off) return false;
#endif
  return (Q.N & 7) == 0 && (Q.Cin & 7) == 0 && (Q.lddu & 7) == 0 && (Q.ldx & 7) == 0 && ((uintptr_t)Q.du & 15) == 0 && ((uintptr_t)Q.x & 15) == 0;
}

static int g_ly_wgrad1 = 1;
extern "C" int ly_tune_wgrad1(int on) {                            // development switch: 0 sends plain-row 1x1 bf16 problems back to ly_wgrad_tiled_body
  const int was = g_ly_wgrad1;
  g_ly_wgrad1 = on;
  return was;
}
static int g_ly_wgrad3 = 1;
extern "C" int ly_tune_wgrad3(int on) {                            // development switch: 0 sends 3x3 problems back to the generic tiled kernel
  const int was = g_ly_wgrad3;
  g_ly_wgrad3 = on;
  return was;
}

// -------------------------------------------------------------------------------------------------
// The launch plan: which kernel a problem (or a group) runs on, with what tile, grid, pixel chunks, flush and LDS.  Written down here and
// nowhere else; the launch functions below take a plan and recompute nothing, and ly_wgrad_describe prints the kernel of the same plan.
// -------------------------------------------------------------------------------------------------
enum WgKind { WG_GENERIC, WG_TILED, WG_W1, WG_W3 };      // ly_wgrad_kernel | ly_wgrad_tiled_kernel | ly_wgrad1.hip | ly_wgrad3.hip
struct WgPlan {
  WgKind kind;
  int BN, BK, PX;                // output tile, pixels per step
  bool rows, pro, oct;           // plain rows (no gather) | x prologue | octet staging.  A group: any member's prologue, every member's octets
  int tiles_n, tiles_k;
  long tiles, chunks, chunk_px;  // grid = tiles x chunks.  A group: tiles and chunks (= blocks) of all members, the per-member ones in LyWgradGroupArgs
  bool slab;                     // partial tiles into LyWgradParams.ws + a fold launch; else the float-atomic flush
  size_t lds;                    // dynamic LDS of the tiled kernels (ly_wgrad1.hip sizes its own image, ly_wgrad3.hip plans itself)
};

// the vector-friendly problems, the ones the tiled kernels take: NHWC, widths and strides in whole quads, addresses aligned to four elements
template <typename T>
static bool wg_vec_ok(const LyWgradParams& P) {
  return !P.nchw && (P.N & 3) == 0 && (P.Cin & 3) == 0 && (P.lddu & 3) == 0 && (P.ldx & 3) == 0 && ((uintptr_t)P.du & (4 * sizeof(T) - 1)) == 0 &&
         ((uintptr_t)P.x & (4 * sizeof(T) - 1)) == 0;
}

// M pixels in chunks for a launch that aims at `target` blocks over `tiles` output tiles: no chunk below min_px pixels, chunks of whole steps
static void wg_chunks(const long M, const long tiles, const long target, const int min_px, const int step, long& chunks, long& chunk_px) {
  chunks = (target + tiles - 1) / tiles;
  const long max_chunks = (M + min_px - 1) / min_px;
  if (chunks > max_chunks) chunks = max_chunks;
  if (chunks < 1) chunks = 1;
  chunk_px = (M + chunks - 1) / chunks;
  chunk_px = (chunk_px + step - 1) / step * step;
  chunks = (M + chunk_px - 1) / chunk_px;
}

// LDS of ly_wgrad_tiled_body: [hi | lo planes][P / 8 pixel groups][BN + BK + 16 row slots][16 bytes], one buffer from 128 bf16 / 64 fp32 pixels
// per step on, else two; + [scale BK | shift BK] of the x prologue
template <typename T>
static size_t wg_lds(const int BN, const int BK, const int P) {
  return (LyT<T>::PL * P >= 128 ? 1 : 2) * (size_t)LyT<T>::PL * (P / 8) * (BN + BK + 16) * 16 + 2 * BK * sizeof(float);
}

// the caller's scratch holds the BN x BK tile of every block
static bool wg_slab_fits(const LyWgradParams& P, const long blocks, const int BN, const int BK) {
  return P.ws != nullptr && blocks * (long)(BN * BK) <= P.ws_floats;
}

// the plan of ly_wgrad(P), or its refusal
template <typename T>
static int wg_plan(const LyWgradParams& P, WgPlan& W) {
  LY_CHECK(P.du && P.x && P.dw, "wgrad: null pointer");
  LY_CHECK(P.M > 0 && P.H > 0 && P.W > 0 && P.N > 0 && P.Cin > 0 && P.ks > 0 && P.stride > 0, "wgrad: bad sizes");
  LY_CHECK(P.M < (1L << 24), "wgrad: M=%ld pixels exceeds the 2^24 limit of the fast index path", P.M);
  LY_CHECK(P.M % ((long)P.H * P.W) == 0, "wgrad: M is not a whole number of images");
  const int Ktot = P.ks * P.ks * P.Cin;
  LY_CHECK(P.n_valid > 0 && P.n_valid <= P.N && P.c_valid > 0 && P.c_valid <= P.Cin && P.dw_ts > 0 && P.dw_cs > 0, "wgrad: bad dw layout");
  LY_CHECK((long)P.lddw >= (long)(P.ks * P.ks - 1) * P.dw_ts + (long)(P.c_valid - 1) * P.dw_cs + 1, "wgrad: lddw=%d does not cover a dw row", P.lddw);
  const bool rows = P.ks == 1 && P.stride == 1 && P.pad == 0 && !P.nchw && !P.up2;
  if (rows) LY_CHECK(P.Hin == P.H && P.Win == P.W, "wgrad: 1x1 gather needs Hin == H, Win == W");
  LY_CHECK((P.x_scale == nullptr) == (P.x_shift == nullptr), "wgrad: x_scale and x_shift come together");
  const bool tiled_ok = wg_vec_ok<T>(P);
  if (P.x_scale) LY_CHECK(rows && tiled_ok, "wgrad: the x prologue is built for plain-row 1x1 problems with vector-friendly widths");
  W = WgPlan{};
  W.rows = rows;
  W.pro = rows && P.x_scale;                             // the x_scale prologue exists for rows only
  if (g_ly_wgrad3 && ly_wgrad3_ok(P)) {                  // 3x3 / stride 1, bf16: halo-tile kernel (ly_wgrad3.hip)
    W.kind = WG_W3;
    return 0;
  }
  if (tiled_ok) {
    // One step of a block is one memory round trip, so what matters for the skinny shapes is how many blocks a CU holds and how many
    // bytes each has in flight: the 64 x 256 tile's 92 KB of LDS meant ONE block (N=8 K=72 M=1.6M: 690 -> 280 us, N=64 K=576: 538 -> 342 us
    // with the tiles below; all wgrad launches of a bs=64 step 7.8 -> 6.5 ms in round 1).
    // pixels per step: 128 (bf16) / 64 (fp32) = the same 272-byte LDS rows in both, held in ONE buffer (the rows of the next step are in
    // flight in registers during the contraction and the buffer is rewritten between two barriers).  Against the double-buffered
    // 64 / 32-pixel step this doubles the bytes in flight per block at the same blocks per CU: all wgrad launches of a bs=64 bf16 step
    // 3.56 -> 3.28 ms.
    W.PX = LyT<T>::BF ? 128 : 64;
    W.BN = W.BK = 128;
    if (P.N <= 64 && Ktot <= 64) W.BN = W.BK = 64;
    else if (P.N <= 32) W.BN = 32;
    else if (P.N <= 64) W.BN = 64;
  } else {
    W.BN = W.BK = 64;
    W.PX = 32;
  }
  W.tiles_n = (P.N + W.BN - 1) / W.BN;
  W.tiles_k = (Ktot + W.BK - 1) / W.BK;
  W.tiles = (long)W.tiles_n * W.tiles_k;
  // tiled: ~512 blocks: every chunk adds its whole tile to dw with float atomics (a quarter of all wgrad time at 1024 blocks; 256 blocks
  // leave CUs idle: 3.80 / 3.56 / 4.36 ms per bs=64 bf16 step for 1024 / 512 / 256)
  if (tiled_ok) wg_chunks(P.M, W.tiles, wg_target_blocks(false), 512, W.PX, W.chunks, W.chunk_px);
  else wg_chunks(P.M, W.tiles, 2048, 256, 32, W.chunks, W.chunk_px);
  LY_CHECK(W.chunks < 65536, "wgrad: too many pixel chunks");
  if (!tiled_ok) {
    W.kind = WG_GENERIC;
    return 0;
  }
  W.lds = wg_lds<T>(W.BN, W.BK, W.PX);
  W.slab = W.chunks > 1 && wg_slab_fits(P, W.chunks * W.tiles, W.BN, W.BK);
  W.oct = wgrad_octets<T>(P);                            // OCT (bf16 storage, every width a multiple of 8) = 16-byte staging loads, the octet form of ly_wgrad_tiled_body
  // plain rows in whole 16-byte vectors, no prologue: [pixel][channel] LDS tiles and transposed fragment reads (ly_wgrad1.hip), same grid,
  // chunks and slab; several chunks without a slab keep the atomic flush of the tiled kernel
  W.kind = g_ly_wgrad1 && rows && !W.pro && W.oct && (W.slab || W.chunks == 1) ? WG_W1 : WG_TILED;
  return 0;
}

// true when P takes the plain-rows 128 x 128 tile of the fast path (the class ly_wgrad_group batches)
template <typename T>
static bool wgrad_is_rows128(const LyWgradParams& P) {
  if (!(P.du && P.x && P.dw) || !(P.M > 0 && P.H > 0 && P.W > 0 && P.N > 64 && P.Cin > 0) || P.M >= (1L << 24) || P.M % ((long)P.H * P.W) != 0) return false;
  if (!(P.ks == 1 && P.stride == 1 && P.pad == 0 && !P.nchw && !P.up2 && P.Hin == P.H && P.Win == P.W)) return false;
  if (!(P.n_valid > 0 && P.n_valid <= P.N && P.c_valid > 0 && P.c_valid <= P.Cin && P.dw_ts > 0 && P.dw_cs > 0)) return false;
  if ((long)P.lddw < (long)(P.c_valid - 1) * P.dw_cs + 1) return false;
  return wg_vec_ok<T>(P);
}

// the plan of ly_wgrad_group(arr, n) for 2 .. LY_WGRAD_GROUP_MAX problems that all are wgrad_is_rows128: the members' tiles, chunks, first
// blocks and slabs in G (the kernels' argument), what they share in S
template <typename T>
static void wg_plan_group(const LyWgradParams* arr, const int n, WgPlan& S, LyWgradGroupArgs& G) {
  S = WgPlan{};
  S.BN = S.BK = 128;
  S.PX = LyT<T>::BF ? 128 : 64;
  S.rows = true;
  S.oct = true;
  for (int g = 0; g < n; ++g) {
    G.p[g] = arr[g];
    G.tiles_k[g] = (arr[g].Cin + S.BK - 1) / S.BK;
    G.tiles[g] = ((arr[g].N + S.BN - 1) / S.BN) * G.tiles_k[g];
    S.tiles += G.tiles[g];
    S.pro = S.pro || arr[g].x_scale != nullptr;
    S.oct = S.oct && wgrad_octets<T>(arr[g]);
  }
  G.n = n;
  G.blk0[0] = G.cblk0[0] = 0;
  for (int g = 0; g < n; ++g) {
    long chunks;
    wg_chunks(arr[g].M, S.tiles, wg_target_blocks(true), 512, S.PX, chunks, G.chunk_px[g]);      // the group shares the ~512 blocks (wg_plan's policy)
    G.chunks[g] = (int)chunks;
    G.blk0[g + 1] = G.blk0[g] + (int)(chunks * G.tiles[g]);
    G.cblk0[g + 1] = G.cblk0[g] + (int)(((long)G.tiles[g] * S.BN * S.BK + 63) / 64);
  }
  S.chunks = G.blk0[n];
  // slab form when the caller's scratch (LyWgradParams.ws of the first problem) holds every block's tile
  S.slab = wg_slab_fits(arr[0], S.chunks, S.BN, S.BK);
  for (int g = 0; g < n; ++g) G.slab[g] = S.slab ? arr[0].ws + (long)G.blk0[g] * (S.BN * S.BK) : nullptr;
  for (int g = n; g < LY_WGRAD_GROUP_MAX; ++g) {
    G.tiles_k[g] = G.tiles[g] = 1; G.chunk_px[g] = S.PX; G.blk0[g + 1] = G.blk0[n]; G.p[g] = arr[0]; G.chunks[g] = 0; G.slab[g] = nullptr;
    G.cblk0[g + 1] = G.cblk0[n];
  }
  S.lds = wg_lds<T>(S.BN, S.BK, S.PX);
  S.oct = S.oct && S.slab;                               // the octet staging goes with the slab form (and bf16 storage) only
  S.kind = g_ly_wgrad1 && S.oct && !S.pro ? WG_W1 : WG_TILED;      // every member eligible: the grouped form of ly_wgrad1.hip
}

// -------------------------------------------------------------------------------------------------
// A plan onto the stream, or its kernel's name (LyOut): plan fields -> template instantiation
// -------------------------------------------------------------------------------------------------
template <typename T, int BN, int BK, int P>
static int wg_launch_tiled(const LyWgradParams& Q, const WgPlan& W, const dim3 grid, float* const slab, const LyOut& out) {
  // <ROWS, PRO, OCT>
#define WG_TILED(ROWS_, PRO_, OCT_)                                                                                                                            \
  LY_EMIT(out, (ly_launch_lds<ly_wgrad_tiled_kernel<T, BN, BK, P, ROWS_, PRO_, OCT_>>(grid, dim3(LY_THREADS), W.lds, out.st, Q, W.tiles_k, W.chunk_px, slab)), \
             "ly_wgrad_tiled_kernel<%s, %d, %d, %d, " #ROWS_ ", " #PRO_ ", " #OCT_ ">", ly_tname<T>(), BN, BK, P)
  if constexpr (LyT<T>::BF) {
    if (W.oct) return !W.rows ? WG_TILED(false, false, true) : W.pro ? WG_TILED(true, true, true) : WG_TILED(true, false, true);
  }
  return !W.rows ? WG_TILED(false, false, false) : W.pro ? WG_TILED(true, true, false) : WG_TILED(true, false, false);
#undef WG_TILED
}

template <typename T>
static int wg_launch(const LyWgradParams& Q, const WgPlan& W, const LyOut& out) {
  constexpr int PX = LyT<T>::BF ? 128 : 64;
  if (W.kind == WG_W3) return LY_EMIT(out, ly_wgrad3_launch(Q, out.st), "ly_wgrad3_kernel");
  const dim3 grid((unsigned)W.tiles, (unsigned)W.chunks);
  if (W.kind == WG_GENERIC) {
#define WG_GENERIC_(ROWS_) \
  LY_EMIT(out, (ly_launch<ly_wgrad_kernel<T, ROWS_>>(grid, dim3(LY_THREADS), 0, out.st, Q, W.tiles_k, W.chunk_px)), "ly_wgrad_kernel<%s, " #ROWS_ ">", ly_tname<T>())
    return W.rows ? WG_GENERIC_(true) : WG_GENERIC_(false);
#undef WG_GENERIC_
  }
  float* const slab = W.slab ? Q.ws : nullptr;
  if (W.kind == WG_W1) LY_TRY(ly_wgrad1_launch(Q, W.BN, W.BK, grid, W.tiles_k, W.chunk_px, slab, out));
  else if (W.BN == 64 && W.BK == 64) LY_TRY((wg_launch_tiled<T, 64, 64, PX>(Q, W, grid, slab, out)));
  else if (W.BN == 32) LY_TRY((wg_launch_tiled<T, 32, 128, PX>(Q, W, grid, slab, out)));
  else if (W.BN == 64) LY_TRY((wg_launch_tiled<T, 64, 128, PX>(Q, W, grid, slab, out)));
  else LY_TRY((wg_launch_tiled<T, 128, 128, PX>(Q, W, grid, slab, out)));
  if (out.name) return 0;
  if (slab) wgrad_combine_launch(Q, slab, W.chunks, W.tiles_k, W.tiles, W.BN, W.BK, out.st);
  LY_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int wg_launch_group(const WgPlan& S, const LyWgradGroupArgs& G, const LyOut& out) {
  constexpr int PX = LyT<T>::BF ? 128 : 64, BN = 128, BK = 128;
  // <PRO, GSLAB, OCT> of the rows form
#define WG_GROUP(PRO_, GSLAB_, OCT_)                                                                                                                      \
  LY_EMIT(out, (ly_launch_lds<ly_wgrad_tiled_group_kernel<T, BN, BK, PX, true, PRO_, GSLAB_, OCT_>>(dim3((unsigned)S.chunks), dim3(LY_THREADS), S.lds, out.st, G)), \
             "ly_wgrad_tiled_group_kernel<%s, %d, %d, %d, true, " #PRO_ ", " #GSLAB_ ", " #OCT_ ">", ly_tname<T>(), BN, BK, PX)
  const auto launch = [&]() -> int {
    if (S.kind == WG_W1) return ly_wgrad1_group_launch(G, out);
    if (!S.slab) return S.pro ? WG_GROUP(true, false, false) : WG_GROUP(false, false, false);
    if constexpr (LyT<T>::BF) {
      if (S.oct) return S.pro ? WG_GROUP(true, true, true) : WG_GROUP(false, true, true);
    }
    return S.pro ? WG_GROUP(true, true, false) : WG_GROUP(false, true, false);
  };
#undef WG_GROUP
  LY_TRY(launch());
  if (S.slab && !out.name) {
    int cmax = 0;
    for (int g = 0; g < G.n; ++g) cmax = G.chunks[g] > cmax ? G.chunks[g] : cmax;
    const int rls = cmax <= 64 ? 4 : 16;
    hipLaunchKernelGGL(ly_wgrad_combine_group_kernel, dim3((unsigned)G.cblk0[G.n]), dim3(64 * rls), 0, out.st, G, BN, BK, rls);
    LY_LAUNCH_CHECK();
  }
  return 0;
}

// -------------------------------------------------------------------------------------------------
// Entry points
// -------------------------------------------------------------------------------------------------
template <typename T>
static int wgrad_dispatch(const LyWgradParams& P, const LyOut& out) {
  WgPlan W;
  LY_TRY(wg_plan<T>(P, W));
  return wg_launch<T>(P, W, out);
}

static int wgrad_one(const LyWgradParams* p, const LyOut& out) {
  LY_CHECK(p, "wgrad: null params");
  LY_CHECK_DTYPE(p->dtype, "wgrad");
  return p->dtype == LY_BF16 ? wgrad_dispatch<__bf16>(*p, out) : wgrad_dispatch<float>(*p, out);
}

template <typename T>
static int wgrad_group_dispatch(const LyWgradParams* arr, const int n, const LyOut& out) {
  WgPlan S;
  LyWgradGroupArgs G;
  wg_plan_group<T>(arr, n, S, G);
  return wg_launch_group<T>(S, G, out);
}

// ly_wgrad_group and its description: 0, or — describing a group that is not one launch — 1
static int wgrad_many(const LyWgradParams* arr, const int n, const LyOut& out) {
  LY_CHECK(arr && n > 0, "wgrad_group: bad arguments");
  bool same = n >= 2 && n <= LY_WGRAD_GROUP_MAX;
  for (int g = 0; g < n && same; ++g) {
    LY_CHECK_DTYPE(arr[g].dtype, "wgrad_group");
    same = arr[g].dtype == arr[0].dtype && (arr[g].dtype == LY_BF16 ? wgrad_is_rows128<__bf16>(arr[g]) : wgrad_is_rows128<float>(arr[g]));
  }
  if (!same) {                                                        // anything else: one launch per problem, as ly_wgrad would
    for (int g = 0; g < n; ++g) {
      const int rc = wgrad_one(arr + g, out);
      if (rc) return rc;
    }
    return out.name && n >= 2 ? 1 : 0;
  }
  return arr[0].dtype == LY_BF16 ? wgrad_group_dispatch<__bf16>(arr, n, out) : wgrad_group_dispatch<float>(arr, n, out);
}

extern "C" int ly_wgrad(const LyWgradParams* p, void* stream) { return wgrad_one(p, LyOut{reinterpret_cast<hipStream_t>(stream), nullptr, 0}); }

extern "C" int ly_wgrad_group(const LyWgradParams* arr, int n, void* stream) {
  return wgrad_many(arr, n, LyOut{reinterpret_cast<hipStream_t>(stream), nullptr, 0});
}

extern "C" int ly_wgrad_describe(const LyWgradParams* arr, int n, char* name, int cap) {
  LY_CHECK(arr && n > 0 && name && cap > 0, "wgrad_describe: bad arguments");
  return wgrad_many(arr, n, LyOut{nullptr, name, cap});
}
