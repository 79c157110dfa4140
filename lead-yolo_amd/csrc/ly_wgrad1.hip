// Weight gradient of a plain-row 1x1 convolution, bf16 storage, gfx950:
//      dW[n][c] += sum over pixels p of  du[p][n] * x[p][c]
// for the problems the octet staging of ly_wgrad_tiled_body (ly_wgrad.hip) took: N, Cin, lddu, ldx multiples of 8, 16-byte aligned bases,
// no gather, no x prologue.  That kernel transposes both operands in registers on their way into [channel][pixel] LDS planes (32 v_perm_b32
// per 8 x 8 piece, a zero select per load, 64 staging registers: the vector pipe was busy half the time in a kernel that should stream).  Here,
// as in ly_wgrad3.hip,
//   * both operands stay in their global layout, [pixel][channel], in LDS: staging is a plain 16-byte copy, and the MFMA fragments (the
//     contraction index is the PIXEL) come out through transposed reads (ds_read_b64_tr_b16), two per 16x16x32 operand, in the k-set of
//     ly_tile.hpp;
//   * a step is 64 pixels; two LDS buffers, one barrier per step, and the raw rows of the next TWO steps in flight in registers (two register
//     sets of (BN + BK) / 32 16-byte vectors: without the transpose the registers are there);
//   * rows past the chunk's end and channel pieces past N / Cin are loaded from a valid address and written to LDS as zeros: the loop body is
//     straight-line, no load under a branch, EXEC all ones at every transposed read.
// Block tile, wave split (2 x 2), accumulator layout, chunking and the slab format [chunk][tile][BN * BK] are those of ly_wgrad_tiled_body: the
// fold kernels of ly_wgrad.hip are reused as they are, and the fold order is unchanged.
// LDS image of a step: du tile [64 px][2 BN + 32 B] | x tile [64 px][2 BK + 32 B].  The row strides are 32 x odd bytes: the 8 pixel rows x 32
// bytes a half-wave's transposed read touches hit all 64 banks once, and a staging store is 16 bytes x consecutive lanes of one row.
#include "ly_tile.hpp"
#include "ly_params.h"
#include "ly_wgrad.hpp"

#define W1_PX 64

template <int BN, int BK>
struct W1 {
  static constexpr int RSA = 2 * BN + 32, RSB = 2 * BK + 32;             // row strides in bytes
  static constexpr int A_BYTES = W1_PX * RSA, BUF = A_BYTES + W1_PX * RSB;
  static constexpr int LDS = 2 * BUF;
  static constexpr int LA = BN / 32, LB = BK / 32;                       // 16-byte loads per thread and step
  static constexpr int WAVES = BN + BK > 160 ? 2 : 3;                    // waves per SIMD the registers are budgeted for
};

// LDS row of pixel r of a step.  A lane's transposed reads deliver rows 4*lq .. 4*lq + 3 and those + 16 of a 32-row k-step; with pixel
// 8*q + 4*h + t of the k-step in row 16*h + 4*q + t those are the pixels 8*lq .. 8*lq + 7: every MFMA sums the same 32 products in the same
// operand positions as the register-transposing kernel did (one ds_read_b128 of 8 consecutive pixels per lane), the k-steps follow in pixel
// order in both, and dw comes out bit for bit as before.  The permutation costs nothing: it is part of the staging store's address.
__host__ __device__ constexpr int w1_row(const int r) { return (r & ~28) | ((r & 4) << 2) | ((r & 24) >> 1); }

typedef short w1_s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bf16x4 w1_tr(const char* p) {
  typedef __attribute__((address_space(3))) w1_s16x4 lds_s16x4;
  return __builtin_bit_cast(bf16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p));
}

// SLAB: the block's tile goes to its slab with plain stores; otherwise it is added to dw with float atomics (dispatched for one chunk only:
// one writer per element)
template <int BN, int BK, bool SLAB>
__device__ __forceinline__ void ly_wgrad1_body(const LyWgradParams& Q, const int tile_idx, const int chunk_idx, const int tiles_k, const long chunk_px,
                                               float* __restrict__ const slab, const int tiles) {
  using C = W1<BN, BK>;
  constexpr int NI = BN / 32, NJ = BK / 32;                              // MFMA tiles per wave along n / c
  constexpr int PRA = BN / 8, PRB = BK / 8;                              // 16-byte pieces per row
  constexpr int RPA = LY_THREADS / PRA, RPB = LY_THREADS / PRB;          // rows one pass of the block covers
  extern __shared__ f32x4 ly_smem4[];
  char* const lds = reinterpret_cast<char*>(ly_smem4);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lq = lane >> 4;
  const int tk = tile_idx % tiles_k, tn = tile_idx / tiles_k;
  const int n0 = tn * BN, k0 = tk * BK;
  const long p_begin = (long)chunk_idx * chunk_px;
  const long p_end = p_begin + chunk_px < Q.M ? p_begin + chunk_px : Q.M;
  if (p_begin >= p_end) return;                                          // (the whole block)
  const __bf16* const du = reinterpret_cast<const __bf16*>(Q.du);
  const __bf16* const xin = reinterpret_cast<const __bf16*>(Q.x);

  // ---- staging plan (the same for every step): piece tid % PR of rows tid / PR + e * RP ----
  const int pcA = tid % PRA, rA = tid / PRA;
  const int pcB = tid % PRB, rB = tid / PRB;
  const bool okA = n0 + 8 * pcA < Q.N, okB = k0 + 8 * pcB < Q.Cin;
  const int colA = okA ? n0 + 8 * pcA : 0, colB = okB ? k0 + 8 * pcB : 0;
  const int stA = w1_row(rA) * C::RSA + 16 * pcA, stB = C::A_BYTES + w1_row(rB) * C::RSB + 16 * pcB;      // (w1_row(rA + e * RPA) = w1_row(rA) + w1_row(e * RPA))
  struct Regs {
    ly_u32x4 a[C::LA], b[C::LB];
    int rows;                                                            // pixels of the step inside the chunk (<= 0: a step past the end)
  };
  auto prefetch = [&](Regs& R, const long p0) {
    const int rows = (int)(p_end - p0 < W1_PX ? p_end - p0 : W1_PX);
    R.rows = rows;
    const long pc = rows > 0 ? p0 : p_begin;                             // masked rows re-request a valid one
    const int rl = rows > 0 ? rows - 1 : 0;
    const __bf16* const da = du + pc * Q.lddu;
    const __bf16* const xa = xin + pc * Q.ldx;
#pragma unroll
    for (int e = 0; e < C::LA; ++e) {
      const int r = rA + e * RPA;
      R.a[e] = *reinterpret_cast<const ly_u32x4*>(da + (unsigned)((r < rl ? r : rl) * Q.lddu + colA));
    }
#pragma unroll
    for (int e = 0; e < C::LB; ++e) {
      const int r = rB + e * RPB;
      R.b[e] = *reinterpret_cast<const ly_u32x4*>(xa + (unsigned)((r < rl ? r : rl) * Q.ldx + colB));
    }
  };
  auto commit = [&](const Regs& R, char* const buf) {
    const ly_u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < C::LA; ++e) *reinterpret_cast<ly_u32x4*>(buf + stA + w1_row(e * RPA) * C::RSA) = (okA && rA + e * RPA < R.rows) ? R.a[e] : z;
#pragma unroll
    for (int e = 0; e < C::LB; ++e) *reinterpret_cast<ly_u32x4*>(buf + stB + w1_row(e * RPB) * C::RSB) = (okB && rB + e * RPB < R.rows) ? R.b[e] : z;
  };

  // ---- fragment addressing (step-invariant) ----
  // transposed read: lane (li, lq) fetches the 8-byte chunk li & 3 of pixel row 4*lq + (li >> 2) (and of row + 16) of a 32-row k-step and
  // receives channel li of the 4 x 16 block its 16-lane group fetched: k = 4*lq .. 4*lq + 3 (and + 16), the k-set of ly_tile.hpp, over LDS
  // rows (w1_row: which pixels those are)
  const int wn = (wave & 1) * (BN / 2), wk = (wave >> 1) * (BK / 2);
  const int r0 = 4 * lq + (li >> 2);
  const int chunk8 = (li & 3) * 8;
  const int fa = r0 * C::RSA + 2 * wn + chunk8;                          // + ks*32*RSA (+ 16*RSA) + i*32
  const int fb = C::A_BYTES + r0 * C::RSB + 2 * wk + chunk8;

  f32x4 acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = ly_zero4();

  auto contract = [&](const char* const buf) {
#pragma unroll
    for (int ks = 0; ks < W1_PX / 32; ++ks) {
      bf16x8 af[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const char* p = buf + fa + ks * 32 * C::RSA + i * 32;
        af[i] = ly_cat8(w1_tr(p), w1_tr(p + 16 * C::RSA));
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const char* p = buf + fb + ks * 32 * C::RSB + j * 32;
        const bf16x8 bf = ly_cat8(w1_tr(p), w1_tr(p + 16 * C::RSB));
#pragma unroll
        for (int i = 0; i < NI; ++i) acc[i][j] = ly_mfma_bf16(af[i], bf, acc[i][j]);
      }
    }
  };

  // Two steps per trip (the register sets and the buffers alternate by name).  A buffer is rewritten one barrier after its fragments were
  // read: the barrier of the other buffer's step lies in between.  A chunk with an odd number of steps contracts one step of zeros.
  Regs R0, R1;
  prefetch(R0, p_begin);
  __builtin_amdgcn_sched_barrier(0);       // R0's loads first: issued after R1's, the first commit of the loop waits for both sets (vmcnt(0)) on every trip
  prefetch(R1, p_begin + W1_PX);
  for (long p0 = p_begin; p0 < p_end; p0 += 2 * W1_PX) {
    // (the fences keep a set's loads behind the other set's commit: mixed, the narrow tiles' commits waited for loads just issued)
    __builtin_amdgcn_sched_barrier(0);
    commit(R0, lds);
    __builtin_amdgcn_sched_barrier(0);
    prefetch(R0, p0 + 2 * W1_PX);
    __syncthreads();
    contract(lds);
    __builtin_amdgcn_sched_barrier(0);
    commit(R1, lds + C::BUF);
    __builtin_amdgcn_sched_barrier(0);
    prefetch(R1, p0 + 3 * W1_PX);
    __syncthreads();
    contract(lds + C::BUF);
  }

  // ---- flush: D lane (li, lq) register r = dW[row 4*lq + r of the 16-row tile][column li] ----
  if constexpr (SLAB) {
    // the chunk's tile [BN][BK] into its own slab with plain stores (16 lanes = 64 contiguous bytes); ly_wgrad_combine folds the chunks
    float* const sl = slab + ((long)chunk_idx * tiles + tile_idx) * (BN * BK);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int lc = wk + 16 * j + li;
        if (k0 + lc >= Q.c_valid) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int lr = wn + 16 * i + 4 * lq + r;
          if (n0 + lr < Q.n_valid) sl[lr * BK + lc] = acc[i][j][r];
        }
      }
  } else {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int cch = k0 + wk + 16 * j + li;
        if (cch >= Q.c_valid) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = n0 + wn + 16 * i + 4 * lq + r;
          if (row < Q.n_valid) atomicAdd(Q.dw + (long)row * Q.lddw + (long)cch * Q.dw_cs, acc[i][j][r]);
        }
      }
  }
}

template <int BN, int BK, bool SLAB>
__global__ __launch_bounds__(LY_THREADS) __attribute__((amdgpu_waves_per_eu(W1<BN, BK>::WAVES))) void ly_wgrad1_kernel(const LyWgradParams P, const int tiles_k,
                                                                                                                        const long chunk_px, float* const slab) {
  ly_wgrad1_body<BN, BK, SLAB>(P, (int)blockIdx.x, (int)blockIdx.y, tiles_k, chunk_px, slab, (int)gridDim.x);
}

// the grouped launch of ly_wgrad_tiled_group_kernel (ly_wgrad.hip: same arguments, same block-to-problem map), slab form
__global__ __launch_bounds__(LY_THREADS) __attribute__((amdgpu_waves_per_eu(W1<128, 128>::WAVES))) void ly_wgrad1_group_kernel(const LyWgradGroupArgs G) {
  const int bid = ly_xcd_remap((int)blockIdx.x, (int)gridDim.x);
  int g = 0;
#pragma unroll
  for (int i = 1; i < LY_WGRAD_GROUP_MAX; ++i)
    if (i < G.n && bid >= G.blk0[i]) g = i;
  g = __builtin_amdgcn_readfirstlane(g);
  const int local = bid - G.blk0[g];
  const int tiles = G.tiles[g];
  const int chunk = __builtin_amdgcn_readfirstlane(local / tiles);
  const int tile = __builtin_amdgcn_readfirstlane(local - chunk * tiles);
  ly_wgrad1_body<128, 128, true>(G.p[g], tile, chunk, G.tiles_k[g], G.chunk_px[g], G.slab[g], tiles);
}

template <int BN, int BK>
static int wgrad1_launch_tile(const LyWgradParams& Q, const dim3 grid, const int tiles_k, const long chunk_px, float* const slab, const LyOut& out) {
#define W1_LAUNCH(SLAB_)                                                                                                                          \
  LY_EMIT(out, (ly_launch_lds<ly_wgrad1_kernel<BN, BK, SLAB_>>(grid, dim3(LY_THREADS), (size_t)W1<BN, BK>::LDS, out.st, Q, tiles_k, chunk_px, slab)), \
             "ly_wgrad1_kernel<%d, %d, " #SLAB_ ">", BN, BK)
  return slab ? W1_LAUNCH(true) : W1_LAUNCH(false);
#undef W1_LAUNCH
}

int ly_wgrad1_launch(const LyWgradParams& Q, const int BN, const int BK, const dim3 grid, const int tiles_k, const long chunk_px, float* const slab,
                     const LyOut& out) {
  LY_CHECK(chunk_px % W1_PX == 0, "wgrad1: chunk of %ld pixels is not a whole number of steps", chunk_px);
  LY_CHECK(slab || grid.y == 1, "wgrad1: several chunks need the slab");
  if (BN == 128 && BK == 128) return wgrad1_launch_tile<128, 128>(Q, grid, tiles_k, chunk_px, slab, out);
  if (BN == 64 && BK == 128) return wgrad1_launch_tile<64, 128>(Q, grid, tiles_k, chunk_px, slab, out);
  if (BN == 32 && BK == 128) return wgrad1_launch_tile<32, 128>(Q, grid, tiles_k, chunk_px, slab, out);
  if (BN == 64 && BK == 64) return wgrad1_launch_tile<64, 64>(Q, grid, tiles_k, chunk_px, slab, out);
  LY_CHECK(false, "wgrad1: no %d x %d tile", BN, BK);
  return 0;
}

int ly_wgrad1_group_launch(const LyWgradGroupArgs& G, const LyOut& out) {
  for (int g = 0; g < G.n; ++g) LY_CHECK(G.chunk_px[g] % W1_PX == 0 && G.slab[g], "wgrad1: group member %d has no slab or a ragged chunk", g);
  return LY_EMIT(out, (ly_launch_lds<ly_wgrad1_group_kernel>(dim3((unsigned)G.blk0[G.n]), dim3(LY_THREADS), (size_t)W1<128, 128>::LDS, out.st, G)),
                    "ly_wgrad1_group_kernel");
}
