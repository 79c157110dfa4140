// What the weight-gradient translation units share: ly_wgrad.hip (the generic and tiled kernels, the launch plan and the dispatch),
// ly_wgrad3.hip (3x3 / stride 1 / pad 1, bf16) and ly_wgrad1.hip (plain-row 1x1, bf16, 16-byte friendly widths).
#pragma once
#include "ly_common.hpp"
#include "ly_params.h"

bool ly_wgrad3_ok(const LyWgradParams& P);                         // ly_wgrad3.hip
int ly_wgrad3_launch(const LyWgradParams& P, hipStream_t st);

// Several independent weight gradients of ONE tile class in one launch (ly_wgrad_group): what the grouped kernels and their fold take
#define LY_WGRAD_GROUP_MAX 4
struct LyWgradGroupArgs {
  LyWgradParams p[LY_WGRAD_GROUP_MAX];
  long chunk_px[LY_WGRAD_GROUP_MAX];
  float* slab[LY_WGRAD_GROUP_MAX];       // per problem: [chunks][tiles][BN * BK] partial tiles (the slab form), else unused
  int tiles_k[LY_WGRAD_GROUP_MAX], tiles[LY_WGRAD_GROUP_MAX], blk0[LY_WGRAD_GROUP_MAX + 1];
  int chunks[LY_WGRAD_GROUP_MAX], cblk0[LY_WGRAD_GROUP_MAX + 1];      // combine launch: chunks per problem, first combine block per problem
  int n;
};

// ly_wgrad1.hip: the launches of wg_launch / wg_launch_group (ly_wgrad.hip) for a problem the plan found eligible — same grid, chunking and
// slab; slab == nullptr (one chunk only) adds to dw directly
int ly_wgrad1_launch(const LyWgradParams& P, int BN, int BK, dim3 grid, int tiles_k, long chunk_px, float* slab, const LyOut& out);
int ly_wgrad1_group_launch(const LyWgradGroupArgs& G, const LyOut& out);

// The fold of a slab launch's partial tiles: *d += sum over chunks of p[chunk * E], in a fixed order whatever the block count of the producing
// launch, one writer per element.  Block = 64 slab columns (threadIdx & 63) x rls row lanes (threadIdx >> 6) that walk the chunks: 16 for
// the single-problem launches (hundreds of chunks per element), 4 when there are a few dozen (1024 threads with two loads apiece were all
// overhead: 13 us).  p = the lane's column of chunk 0, E = floats per chunk; `live` lanes own an element, d is used by those of row lane 0
// (whose thread index is their column).  The kernels that call it keep only their own decode of the column into (row, tap, channel).
__device__ __forceinline__ void ly_wgrad_fold(const float* __restrict__ p, const long E, const int chunks, const int rls, const bool live, float* const d) {
  __shared__ float red[16 * 64];                      // [row lane][column]: a lane's slot is its thread index
  const int rl = threadIdx.x >> 6;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (live) {
    // four loads in flight per lane (the launch is a handful of dependent memory round trips: 8.6 -> ~6 us with two more in flight)
    int c = rl;
    for (; c + 7 * rls < chunks; c += 8 * rls) {        // eight loads fenced ahead of the adds (the scheduler sinks them back otherwise)
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = p[(long)(c + rls * k) * E];
      __builtin_amdgcn_sched_barrier(0);
      a0 += v[0]; a1 += v[1]; a2 += v[2]; a3 += v[3];
      a0 += v[4]; a1 += v[5]; a2 += v[6]; a3 += v[7];
    }
    for (; c + 3 * rls < chunks; c += 4 * rls) {
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = p[(long)(c + rls * k) * E];
      __builtin_amdgcn_sched_barrier(0);
      a0 += v[0]; a1 += v[1]; a2 += v[2]; a3 += v[3];
    }
    if (c < chunks) a0 += p[(long)c * E];
    if (c + rls < chunks) a1 += p[(long)(c + rls) * E];
    if (c + 2 * rls < chunks) a2 += p[(long)(c + 2 * rls) * E];
  }
  red[threadIdx.x] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (rl == 0 && live) {
    float s = 0.f;
    for (int i = 0; i < rls; ++i) s += red[64 * i + threadIdx.x];
    *d += s;
  }
}
