// Whole-scene detection on the device: a SAR scene of 10 000 .. 30 000 pixels a side runs at native resolution as overlapping tiles, and the
// tiles' detections are merged in scene coordinates.  What a user of the reference does on the host around detect.py — cut windows out of
// the scene, pad them with 114, transpose((2, 0, 1))[::-1], shift every tile's boxes by its origin, de-duplicate in numpy — as three
// launches per scene around the forward and the per-tile NMS   (gfx950 only)
//
//   ly_scene_tiles_u8   windows of the scene -> the model's uint8 RGB planes.  A pure copy: a lane owns 16 consecutive pixels of one tile row
//                       (48 source bytes for BGR, 16 for grey) and stores one 16-byte vector per plane.  The window's first byte,
//                       scene + (y0 + v) * pitch + (x0 + u) * C, is aligned to nothing in general, so the source is read in one of three
//                       forms chosen per lane from its address: three (one) 16-byte loads when the address is 16-byte aligned and the lane's
//                       pixels are all inside the scene (the tile plan's origins are multiples of tile - overlap: the usual case); else the
//                       aligned dwords that cover the bytes, shifted into place with v_alignbyte_b32; at the scene's right edge only the
//                       dwords that hold at least one byte of the row.  A dword that holds a byte of the row lies in the 4-byte word of that
//                       byte, so no load leaves the allocation's words.  Offsets are 64-bit throughout (a scene is up to 2.7 GB).
//   ly_scene_collect    what nms_padded returned for the tiles -> one candidate list in scene pixels: boxes shifted by the tile's origin
//                       and clipped to the scene, score = conf, padding rows score = -1.  One thread per row.
//   (sort)              torch.sort(score, descending=True, stable=True) on the device, as lead-yolo_amd/nms.py
//   ly_scene_nms        greedy suppression across tiles over the sorted candidates.  ly_nms_greedy's structure (one block, the alive set an
//                       LDS bitset, the block's threads — 1024 here, four candidates each per step — share the later candidates of each kept box) with two differences that a scene
//                       needs: classes are COMPARED (ly_nms_greedy shifts boxes by cls * 7680, which real coordinates of a scene exceed), and
//                       a pair from one tile is exempt (nms_padded has settled it).  The only atomics are and / min on LDS words, whose
//                       result does not depend on their order: the same keep in every run.
// Built with -ffp-contract=off (Makefile): the shift, the clip and the overlap metric are the operations written, in the order written.
#include "ly_common.hpp"
#include "ly_params.h"

#define LY_SCENE_MAXN 30016               // >= max_merge, multiple of 32 (the alive set: 938 LDS words, as ly_nms_greedy)
#define LY_SCENE_WORDS (LY_SCENE_MAXN / 32)

namespace {

constexpr int kPx = 16;                   // tile pixels per lane: one 16-byte store per plane
constexpr unsigned kFill4 = 0x72727272u;  // four pixels of 114
constexpr int kNmsThreads = 1024;         // ly_scene_nms: one block of 16 waves
constexpr int kNmsUnroll = 4;             // candidates per thread and step

union LyPx16 {
  uint4 q;
  unsigned w[4];
};

// byte b of the little-endian byte string d[0], d[1], ...
#define LY_SC_BYTE(d, b) (((d)[(b) >> 2] >> (8 * ((b) & 3))) & 0xffu)

// the 4 * NW bytes that start `sh` bytes into the aligned dwords w[0 .. NW]: v_alignbyte_b32 per dword
template <int NW>
__device__ __forceinline__ void ly_sc_align(const unsigned (&w)[NW + 1], const unsigned sh, unsigned (&d)[NW]) {
#pragma unroll
  for (int i = 0; i < NW; ++i) d[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sh);
}

template <int C>
__global__ __launch_bounds__(LY_THREADS) void ly_scene_tiles_kernel(const unsigned char* __restrict__ scene, const int H, const int W, const long pitch,
                                                                    const int* __restrict__ origins, const int T,
                                                                    unsigned char* __restrict__ dst) {
  constexpr int NW = kPx * C / 4;         // dwords of a lane's source bytes: 12 (BGR) or 4 (grey)
  const int per_row = T / kPx;
  const int i = blockIdx.x * LY_THREADS + threadIdx.x;     // lane of tile blockIdx.y: T * T / 16 <= 2^22
  const int v = i / per_row;
  if (v >= T) return;
  const int u0 = (i - v * per_row) * kPx;
  const int k = blockIdx.y;
  const int y0 = origins[2 * k], x0 = origins[2 * k + 1];
  const int y = y0 + v, x = x0 + u0;
  // pixels of this lane inside the scene.  The origins are device data the entry cannot inspect: one that breaks the contract (outside the
  // scene) gives an all-114 tile, never a read outside the scene
  int npx = y0 >= 0 && x0 >= 0 && y < H ? W - x : 0;
  npx = npx < 0 ? 0 : (npx > kPx ? kPx : npx);
  unsigned d[NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) d[j] = 0u;
  if (npx > 0) {
    const unsigned char* p = scene + ((long)y * pitch + (long)x * C);
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (npx == kPx && (a & 15) == 0) {
#pragma unroll
      for (int j = 0; j < NW / 4; ++j) {
        const uint4 q = reinterpret_cast<const uint4*>(p)[j];
        d[4 * j] = q.x; d[4 * j + 1] = q.y; d[4 * j + 2] = q.z; d[4 * j + 3] = q.w;
      }
    } else {
      const unsigned sh = (unsigned)(a & 3);
      const unsigned* q = reinterpret_cast<const unsigned*>(p - sh);
      unsigned w[NW + 1];
      if (npx == kPx) {
#pragma unroll
        for (int j = 0; j < NW; ++j) w[j] = q[j];
        w[NW] = sh ? q[NW] : 0u;                           // the last dword holds bytes of the row only when the start is unaligned
      } else {
        const int end = (int)sh + npx * C;                 // one past the row's last byte, counted from q
#pragma unroll
        for (int j = 0; j <= NW; ++j) w[j] = 4 * j < end ? q[j] : 0u;
      }
      ly_sc_align<NW>(w, sh, d);
    }
  }
  // de-interleave: plane c of the output takes channel 2 - c (BGR -> RGB); pixels past the scene are 114
  LyPx16 out[3];
#pragma unroll
  for (int g = 0; g < 4; ++g) {                            // pixels 4g .. 4g + 3
    const int in = npx - 4 * g;
    const unsigned mask = in >= 4 ? 0xffffffffu : (in <= 0 ? 0u : ((1u << (8 * in)) - 1u));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      unsigned val = 0u;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int b = C == 3 ? (4 * g + e) * 3 + (2 - c) : 4 * g + e;
        val |= LY_SC_BYTE(d, b) << (8 * e);
      }
      out[c].w[g] = (val & mask) | (kFill4 & ~mask);
    }
  }
  const long plane = (long)T * T;
  unsigned char* o = dst + ((long)k * 3 * plane + (long)v * T + u0);
  *reinterpret_cast<uint4*>(o) = out[0].q;
  *reinterpret_cast<uint4*>(o + plane) = out[1].q;
  *reinterpret_cast<uint4*>(o + 2 * plane) = out[2].q;
}

__global__ __launch_bounds__(LY_THREADS) void ly_scene_collect_kernel(const float* __restrict__ dets, const int* __restrict__ counts,
                                                                      const int* __restrict__ origins, const long rows, const int max_det,
                                                                      const float fH, const float fW, float* __restrict__ boxes,
                                                                      float* __restrict__ score) {
  const long i = (long)blockIdx.x * LY_THREADS + threadIdx.x;
  if (i >= rows) return;
  const int t = (int)(i / max_det);
  const int r = (int)(i - (long)t * max_det);
  float* o = boxes + i * 6;
  if (r >= counts[t]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = 0.f;
    score[i] = -1.f;
    return;
  }
  const float* p = dets + i * 6;
  const float y0 = (float)origins[2 * t], x0 = (float)origins[2 * t + 1];
  o[0] = fminf(fmaxf(p[0] + x0, 0.f), fW);
  o[1] = fminf(fmaxf(p[1] + y0, 0.f), fH);
  o[2] = fminf(fmaxf(p[2] + x0, 0.f), fW);
  o[3] = fminf(fmaxf(p[3] + y0, 0.f), fH);
  o[4] = p[4];
  o[5] = p[5];
  score[i] = p[4];
}

// the overlap metric of the header: boxes a (area_a) and b (area_b)
template <int METRIC>
__device__ __forceinline__ float ly_scene_metric(const float ax1, const float ay1, const float ax2, const float ay2, const float area_a,
                                                 const float bx1, const float by1, const float bx2, const float by2, const float area_b) {
  const float iw = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.f), ih = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.f);
  const float inter = iw * ih;
  const float den = METRIC == 0 ? (area_a + area_b) - inter : fminf(area_a, area_b);
  return den == 0.f ? 0.f : inter / den;
}

template <int METRIC>
__global__ __launch_bounds__(kNmsThreads) void ly_scene_nms_kernel(const float* __restrict__ boxes, const long* __restrict__ order,
                                                                  const float* __restrict__ sorted_score, const int N, const int max_det_tile,
                                                                  const float thres, const int agnostic, const int max_det, const int max_merge,
                                                                  int* __restrict__ keep, int* __restrict__ count) {
  __shared__ unsigned alive[LY_SCENE_WORDS];
  __shared__ int s_n, s_next;
  const int tid = threadIdx.x;
  if (tid == 0) s_n = 0;
  __syncthreads();
  // candidates = the sorted prefix with score >= 0 (padding rows carry -1)
  int cnt = 0;
  for (int j = tid; j < N; j += kNmsThreads) cnt += sorted_score[j] >= 0.f ? 1 : 0;
  atomicAdd(&s_n, cnt);
  __syncthreads();
  int n = s_n;
  n = n < max_merge ? n : max_merge;
  n = n < LY_SCENE_MAXN ? n : LY_SCENE_MAXN;
  for (int wi = tid; wi < LY_SCENE_WORDS; wi += kNmsThreads) {
    const int lo = wi * 32;
    alive[wi] = lo + 32 <= n ? 0xffffffffu : (lo < n ? ((1u << (n - lo)) - 1u) : 0u);
  }
  __syncthreads();
  int kept = 0, cur = 0;
  while (kept < max_det && cur < n) {
    if (tid == 0) s_next = n;
    __syncthreads();
    // first alive candidate >= cur
    for (int wi = (cur >> 5) + tid; wi * 32 < n; wi += kNmsThreads) {
      unsigned m = alive[wi];
      if (wi == (cur >> 5)) m &= ~((1u << (cur & 31)) - 1u);
      if (m) { atomicMin(&s_next, wi * 32 + __ffs(m) - 1); break; }
    }
    __syncthreads();
    const int i = s_next;
    if (i >= n) break;
    const long oi = order[i];
    if (tid == 0) keep[kept] = (int)oi;
    const float* di = boxes + oi * 6;
    const float ax1 = di[0], ay1 = di[1], ax2 = di[2], ay2 = di[3], cls_i = di[5];
    const float area_i = (ax2 - ax1) * (ay2 - ay1);
    const int tile_i = (int)oi / max_det_tile;               // N < 2^31
    // the later candidates, kNmsUnroll per thread and step: the addresses of a step do not depend on one another (a candidate that is
    // out of range or dead reads the kept box instead), so its loads are in flight together
    for (int j0 = i + 1 + tid; j0 < n; j0 += kNmsUnroll * kNmsThreads) {
      bool on[kNmsUnroll];
      long oj[kNmsUnroll];
      float2 b01[kNmsUnroll], b23[kNmsUnroll], b45[kNmsUnroll];
#pragma unroll
      for (int u = 0; u < kNmsUnroll; ++u) {
        const int j = j0 + u * kNmsThreads;
        on[u] = j < n && ((alive[j >> 5] >> (j & 31)) & 1u);
        oj[u] = on[u] ? order[j] : oi;
      }
#pragma unroll
      for (int u = 0; u < kNmsUnroll; ++u) {
        const float2* dj = reinterpret_cast<const float2*>(boxes + oj[u] * 6);   // a row is 24 bytes: 8-byte aligned
        b01[u] = dj[0]; b23[u] = dj[1]; b45[u] = dj[2];
      }
#pragma unroll
      for (int u = 0; u < kNmsUnroll; ++u) {
        const int j = j0 + u * kNmsThreads;
        if (!on[u]) continue;
        if ((int)oj[u] / max_det_tile == tile_i) continue;   // one tile: nms_padded has settled the pair
        if (!agnostic && b45[u].y != cls_i) continue;
        const float bx1 = b01[u].x, by1 = b01[u].y, bx2 = b23[u].x, by2 = b23[u].y;
        const float area_j = (bx2 - bx1) * (by2 - by1);
        if (ly_scene_metric<METRIC>(ax1, ay1, ax2, ay2, area_i, bx1, by1, bx2, by2, area_j) > thres) atomicAnd(&alive[j >> 5], ~(1u << (j & 31)));
      }
    }
    ++kept;
    cur = i + 1;
    __syncthreads();
  }
  for (int r = kept + tid; r < max_det; r += kNmsThreads) keep[r] = 0;
  if (tid == 0) count[0] = kept;
}

}  // namespace

extern "C" int ly_scene_tiles_u8(const unsigned char* scene, int H, int W, int C, long pitch, const int* origins, int n, int T, unsigned char* dst,
                                 void* stream) {
  LY_CHECK(scene && origins && dst, "scene_tiles_u8: null pointer");
  LY_CHECK(C == 3 || C == 1, "scene_tiles_u8: C = %d (3: HWC BGR, 1: one grey plane)", C);
  LY_CHECK(H >= 1 && W >= 1 && pitch >= (long)W * C, "scene_tiles_u8: scene %d x %d x %d with a row pitch of %ld bytes", H, W, C, pitch);
  LY_CHECK(n >= 1 && n <= 65535, "scene_tiles_u8: n = %d outside [1, 65535]", n);
  LY_CHECK(T >= kPx && T % kPx == 0 && T <= 8192, "scene_tiles_u8: T = %d must be a multiple of 16 in [16, 8192]", T);
  LY_CHECK((reinterpret_cast<uintptr_t>(dst) & 15) == 0, "scene_tiles_u8: dst must be 16-byte aligned");
  const dim3 grid((unsigned)((T * (T / kPx) + LY_THREADS - 1) / LY_THREADS), (unsigned)n);
  if (C == 3)
    hipLaunchKernelGGL(ly_scene_tiles_kernel<3>, grid, dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), scene, H, W, pitch, origins, T, dst);
  else
    hipLaunchKernelGGL(ly_scene_tiles_kernel<1>, grid, dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), scene, H, W, pitch, origins, T, dst);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_scene_collect(const float* dets, const int* counts, const int* origins, int n_tiles, int max_det, int H, int W, float* boxes,
                                float* score, void* stream) {
  LY_CHECK(dets && counts && origins && boxes && score, "scene_collect: null pointer");
  LY_CHECK(n_tiles > 0 && max_det > 0 && (long)n_tiles * max_det < (1L << 31) && H >= 1 && W >= 1, "scene_collect: bad sizes (n_tiles=%d max_det=%d H=%d W=%d)",
           n_tiles, max_det, H, W);
  const long rows = (long)n_tiles * max_det;
  hipLaunchKernelGGL(ly_scene_collect_kernel, dim3((unsigned)((rows + LY_THREADS - 1) / LY_THREADS)), dim3(LY_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), dets, counts, origins, rows, max_det, (float)H, (float)W, boxes, score);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_scene_nms(const float* boxes, const long* order, const float* sorted_score, int N, int max_det_tile, int metric, float thres,
                            int agnostic, int max_det, int max_merge, int* keep, int* count, void* stream) {
  LY_CHECK(boxes && order && sorted_score && keep && count && N > 0 && max_det_tile > 0 && max_det > 0 && max_merge > 0, "scene_nms: bad arguments");
  LY_CHECK((reinterpret_cast<uintptr_t>(boxes) & 7) == 0, "scene_nms: boxes must be 8-byte aligned");
  LY_CHECK(metric == 0 || metric == 1, "scene_nms: metric %d (0: IoU, 1: intersection over the smaller box)", metric);
  LY_CHECK(max_merge <= 30000, "scene_nms: max_merge=%d exceeds the 30000 candidates the alive set holds", max_merge);
  if (metric == 0)
    hipLaunchKernelGGL(ly_scene_nms_kernel<0>, dim3(1), dim3(kNmsThreads), 0, reinterpret_cast<hipStream_t>(stream), boxes, order, sorted_score, N, max_det_tile,
                       thres, agnostic, max_det, max_merge, keep, count);
  else
    hipLaunchKernelGGL(ly_scene_nms_kernel<1>, dim3(1), dim3(kNmsThreads), 0, reinterpret_cast<hipStream_t>(stream), boxes, order, sorted_score, N, max_det_tile,
                       thres, agnostic, max_det, max_merge, keep, count);
  LY_LAUNCH_CHECK();
  return 0;
}
