// Autoanchor on the device: what utils/autoanchor.py computes before the first epoch (check_anchors, kmean_anchors), over the label
// sizes the ImageBank already holds.  Three groups of kernels:
//
//   ly_anchor_wh            wh[j] = labels[j, 3:5] * (shape[img(j)] * scale[img(j)])  (autoanchor.py:34-36 / 128-129): float64 products as numpy
//                           forms them, rounded once to float32
//   ly_anchor_metric        `metric` (autoanchor.py:38-44 and 104-112) for G candidate anchor sets in one launch: r = wh / k, x = min over
//                           the two sides of min(r, 1 / r), best = max over anchors of x; per (label slice, candidate) the partials of
//                           sum best * (best > 1/thr), count best > 1/thr, count x > 1/thr.  bpr, aat and anchor_fitness are these three
//                           numbers over n.
//   ly_anchor_evolve_eval   the body of kmean_anchors' `for _ in pbar` loop (autoanchor.py:156-165) for B speculative generations at once:
//   ly_anchor_evolve_pick   candidate c is kg = max(k * v[g + c], 2.0) from the CURRENT k; the one-block pick folds the fitness partials
//                           and accepts the lowest c with fg > f (k = kg_c, f = fg_c, g += c + 1; none: g += B).  A candidate behind an
//                           accepted one is evaluated again from the new k in the next round: the reference's serial chain, exactly.
//   ly_kmeans_assign        one Lloyd iteration of R independent runs (scipy.cluster.vq.kmeans -> _kmeans -> vq / update_cluster_means):
//   ly_kmeans_update        nearest centroid by dx*dx + dy*dy in float32 (lowest index on equality), per-block double partials of
//                           (sum x, sum y, count) per centroid and of sqrtf(d2) per run; the one-block update folds them, sets
//                           centroid = float32(sum / count) and the run's distortion, and closes a run whose distortion moved by at most
//                           `thresh` or that lost a centroid's last point (discarded, as the reference's `assert n == len(k)` does).
//
// No atomics anywhere: every block leaves its partial in a slab row, and the slabs are folded in index order (ly_sum_rows_f64 for the
// metric, the pick / update kernels for the other two), so the results do not depend on the scheduling — and not on the slice count
// either where the sums are exact (float32 terms in (0.25, 1]: up to 2^26 of them add exactly in double).
// The file is compiled with -ffp-contract=off: every float32 quotient, product and sum is the operation the reference performs, in its order;
// `/` is hipcc's correctly rounded division (its default), 1 / r included.
#include "ly_common.hpp"
#include "../../include/lead_yolo_hip.h"

#define LY_AN_WAVES (LY_THREADS / LY_WAVE)

// sum of v over the block, in a fixed order: a shuffle tree inside each wave, then the waves' partials in index order.  s_w: LY_AN_WAVES
// doubles of LDS owned by this call (no barrier after the read: give every call its own row).  Valid on thread 0.
__device__ __forceinline__ double ly_an_block_sum(double v, double* s_w) {
#pragma unroll
  for (int m = LY_WAVE / 2; m >= 1; m >>= 1) v += __shfl_down(v, m);
  if ((threadIdx.x & (LY_WAVE - 1)) == 0) s_w[threadIdx.x / LY_WAVE] = v;
  __syncthreads();
  double a = s_w[0];
#pragma unroll
  for (int w = 1; w < LY_AN_WAVES; ++w) a += s_w[w];
  return a;
}

// the label range of slice s: [lo, hi), contiguous chunks of ceil(n / slices) labels
__device__ __forceinline__ void ly_an_slice(long n, int slices, int s, long& lo, long& hi) {
  const long chunk = (n + slices - 1) / slices;
  lo = (long)s * chunk;
  hi = lo + chunk < n ? lo + chunk : n;
  if (lo > n) lo = n;
}

__device__ __forceinline__ float ly_an_min(float a, float b) { return b < a ? b : a; }

// metric of one label against the na anchors in LDS: best = max_a min(min(w / kw, 1 / (w / kw)), min(h / kh, 1 / (h / kh))); above: how many x > ithr
__device__ __forceinline__ float ly_an_best(const float2 p, const float* s_k, int na, float ithr, int& above) {
  float best = 0.f;
  bool first = true;
  for (int a = 0; a < na; ++a) {
    const float r0 = p.x / s_k[2 * a], r1 = p.y / s_k[2 * a + 1];
    const float x = ly_an_min(ly_an_min(r0, 1.f / r0), ly_an_min(r1, 1.f / r1));
    above += x > ithr ? 1 : 0;
    best = first || x > best ? x : best;
    first = false;
  }
  return best;
}

__global__ __launch_bounds__(LY_THREADS) void ly_anchor_wh_kernel(const double* __restrict__ labels, const int* __restrict__ img, long n,
                                                                  const double* __restrict__ shapes, int n_img, const double* __restrict__ scale,
                                                                  float* __restrict__ wh) {
  const long j = (long)blockIdx.x * LY_THREADS + threadIdx.x;
  if (j >= n) return;
  const int i = img[j];
  float2 o = make_float2(__builtin_nanf(""), __builtin_nanf(""));          // an image index outside [0, n_img): NaN, nothing is read
  if (i >= 0 && i < n_img) {
    double sw = shapes[2 * i], sh = shapes[2 * i + 1];
    if (scale) { sw *= scale[i]; sh *= scale[i]; }                          // `shapes * scale` first, as the reference's zip does
    o.x = (float)(labels[j * 5 + 3] * sw);
    o.y = (float)(labels[j * 5 + 4] * sh);
  }
  reinterpret_cast<float2*>(wh)[j] = o;
}

// grid (slices, G); part[s][3 g + 0..2] = (sum best * (best > ithr), count best > ithr, count x > ithr) of slice s, the counts as exact doubles
__global__ __launch_bounds__(LY_THREADS) void ly_anchor_metric_kernel(const float* __restrict__ wh, long n, const float* __restrict__ k, int na,
                                                                      float ithr, double* __restrict__ part) {
  __shared__ float s_k[2 * LY_ANCHOR_NA_MAX];
  __shared__ double s_w[3][LY_AN_WAVES];
  const int g = blockIdx.y, s = blockIdx.x, G = gridDim.y, tid = threadIdx.x;
  if (tid < 2 * na) s_k[tid] = k[(long)g * 2 * na + tid];
  __syncthreads();
  long lo, hi;
  ly_an_slice(n, gridDim.x, s, lo, hi);
  double sum = 0.0;
  int nb = 0, nx = 0;
  for (long j = lo + tid; j < hi; j += LY_THREADS) {
    const float best = ly_an_best(reinterpret_cast<const float2*>(wh)[j], s_k, na, ithr, nx);
    if (best > ithr) { sum += (double)best; ++nb; }
  }
  const double a0 = ly_an_block_sum(sum, s_w[0]), a1 = ly_an_block_sum((double)nb, s_w[1]), a2 = ly_an_block_sum((double)nx, s_w[2]);
  if (tid == 0) {
    double* o = part + ((long)s * G + g) * 3;
    o[0] = a0; o[1] = a1; o[2] = a2;
  }
}

// grid (slices, B); candidate c = blockIdx.y is generation cursor[0] + c: kg = float32(max(k * v[g + c], 2.0)); part[s][c] = its fitness sum over slice s
__global__ __launch_bounds__(LY_THREADS) void ly_anchor_evolve_eval_kernel(const float* __restrict__ wh, long n, const double* __restrict__ v, int gen,
                                                                           int na, const double* __restrict__ k, const int* __restrict__ cursor,
                                                                           float ithr, double* __restrict__ part) {
  __shared__ float s_k[2 * LY_ANCHOR_NA_MAX];
  __shared__ double s_w[LY_AN_WAVES];
  const int c = blockIdx.y, s = blockIdx.x, B = gridDim.y, tid = threadIdx.x;
  const long g = (long)cursor[0] + c;
  if (g < 0 || g >= gen) {                                                  // past the table (block-uniform): the pick never reads this candidate
    if (tid == 0) part[(long)s * B + c] = 0.0;
    return;
  }
  if (tid < 2 * na) {
    const double kg = k[tid] * v[g * 2 * na + tid];
    s_k[tid] = (float)(kg < 2.0 ? 2.0 : kg);
  }
  __syncthreads();
  long lo, hi;
  ly_an_slice(n, gridDim.x, s, lo, hi);
  double sum = 0.0;
  int nx = 0;
  for (long j = lo + tid; j < hi; j += LY_THREADS) {
    const float best = ly_an_best(reinterpret_cast<const float2*>(wh)[j], s_k, na, ithr, nx);
    if (best > ithr) sum += (double)best;
  }
  const double a = ly_an_block_sum(sum, s_w);
  if (tid == 0) part[(long)s * B + c] = a;
}

// one block: fg_c = sum over slices (index order); the lowest c with fg_c > f is accepted.  cursor[0]: generation, cursor[1]: acceptances.
__global__ __launch_bounds__(LY_THREADS) void ly_anchor_evolve_pick_kernel(const double* __restrict__ part, int slices, int B, const double* __restrict__ v,
                                                                           int gen, int na, double* k, double* f, int* cursor) {
  __shared__ double s_f[LY_THREADS];
  __shared__ int s_pick;
  const int tid = threadIdx.x;
  const long g = cursor[0];
  if (tid < B) {
    double a = 0.0;
    for (int s = 0; s < slices; ++s) a += part[(long)s * B + tid];
    s_f[tid] = a;
  }
  __syncthreads();
  if (tid == 0) {
    const double f0 = f[0];
    int pick = -1;
    for (int c = 0; c < B && g + c < gen; ++c)
      if (s_f[c] > f0) { pick = c; break; }
    s_pick = pick;
  }
  __syncthreads();
  const int pick = s_pick;
  if (pick >= 0 && tid < 2 * na) {
    const double kg = k[tid] * v[(g + pick) * 2 * na + tid];
    k[tid] = kg < 2.0 ? 2.0 : kg;
  }
  if (tid == 0) {
    if (pick >= 0) { f[0] = s_f[pick]; cursor[1] += 1; }
    const long g1 = g + (pick >= 0 ? pick + 1 : B);
    cursor[0] = (int)(g1 < gen ? g1 : gen);
  }
}

// grid (slices, R); part[s][r][3 c + 0..2] = (sum x, sum y, count) of the points of slice s nearest to centroid c of run r, part[s][r][3 na] =
// the sum of their distances sqrtf(d2).  A closed run (flags != 0) is skipped.  assign (NULL or [R][n]): the chosen centroids.
__global__ __launch_bounds__(LY_THREADS) void ly_kmeans_assign_kernel(const float* __restrict__ pts, long n, const float* __restrict__ cent, int na,
                                                                      const int* __restrict__ flags, double* __restrict__ part,
                                                                      int* __restrict__ assign) {
  __shared__ float s_c[2 * LY_ANCHOR_NA_MAX];
  __shared__ double s_w[3 * LY_ANCHOR_NA_MAX + 1][LY_AN_WAVES];
  const int r = blockIdx.y, s = blockIdx.x, R = gridDim.y, tid = threadIdx.x;
  if (flags[r]) return;                                                     // block-uniform
  if (tid < 2 * na) s_c[tid] = cent[(long)r * 2 * na + tid];
  __syncthreads();
  long lo, hi;
  ly_an_slice(n, gridDim.x, s, lo, hi);
  double sx[LY_ANCHOR_NA_MAX], sy[LY_ANCHOR_NA_MAX], dist = 0.0;
  int cnt[LY_ANCHOR_NA_MAX];
#pragma unroll
  for (int c = 0; c < LY_ANCHOR_NA_MAX; ++c) { sx[c] = 0.0; sy[c] = 0.0; cnt[c] = 0; }
  for (long j = lo + tid; j < hi; j += LY_THREADS) {
    const float2 p = reinterpret_cast<const float2*>(pts)[j];
    int bc = 0;
    float bd = 0.f;
    for (int c = 0; c < na; ++c) {
      const float dx = p.x - s_c[2 * c], dy = p.y - s_c[2 * c + 1];
      const float d2 = dx * dx + dy * dy;
      if (c == 0 || d2 < bd) { bd = d2; bc = c; }                           // strict: the lowest index keeps an equal distance
    }
#pragma unroll
    for (int c = 0; c < LY_ANCHOR_NA_MAX; ++c) {                            // predicated: the accumulators stay in registers
      const bool m = c == bc;
      sx[c] += m ? (double)p.x : 0.0;
      sy[c] += m ? (double)p.y : 0.0;
      cnt[c] += m ? 1 : 0;
    }
    dist += (double)sqrtf(bd);
    if (assign) assign[(long)r * n + j] = bc;
  }
  double* o = part + ((long)s * R + r) * (3 * na + 1);
#pragma unroll
  for (int c = 0; c < LY_ANCHOR_NA_MAX; ++c) {
    if (c < na) {                                                           // block-uniform
      const double a0 = ly_an_block_sum(sx[c], s_w[3 * c]), a1 = ly_an_block_sum(sy[c], s_w[3 * c + 1]);
      const double a2 = ly_an_block_sum((double)cnt[c], s_w[3 * c + 2]);
      if (tid == 0) { o[3 * c] = a0; o[3 * c + 1] = a1; o[3 * c + 2] = a2; }
    }
  }
  const double ad = ly_an_block_sum(dist, s_w[3 * LY_ANCHOR_NA_MAX]);
  if (tid == 0) o[3 * na] = ad;
}

// one block.  Items (r, c), c < na: fold the slices in index order, centroid = float32(sum / count); item (r, na): distortion = sum / n.
// flags[r]: bit 0 closed (|previous distortion - distortion| <= thresh), bit 1 discarded (a centroid without points; the run keeps its centroids).
// active[0] = the runs still open after this iteration.
__global__ __launch_bounds__(LY_THREADS) void ly_kmeans_update_kernel(const double* __restrict__ part, int slices, int R, int na, long n, double thresh,
                                                                      float* cent, double* dist, int* __restrict__ count, int* flags, int* iters,
                                                                      int* __restrict__ active) {
  __shared__ int s_empty[LY_THREADS];                                       // per run: a centroid lost its points (R <= LY_THREADS)
  const int tid = threadIdx.x, w = 3 * na + 1;
  for (int r = tid; r < R; r += LY_THREADS) s_empty[r] = 0;
  __syncthreads();
  // pass 1: counts (an empty centroid closes the whole run before any of its centroids moves)
  for (int it = tid; it < R * na; it += LY_THREADS) {
    const int r = it / na, c = it - r * na;
    if (flags[r]) continue;
    double a = 0.0;
    for (int s = 0; s < slices; ++s) a += part[((long)s * R + r) * w + 3 * c + 2];
    count[it] = (int)a;
    if (a == 0.0) s_empty[r] = 1;                                           // every writer stores the same value
  }
  __syncthreads();
  for (int it = tid; it < R * (na + 1); it += LY_THREADS) {
    const int r = it / (na + 1), c = it - r * (na + 1);
    if (flags[r]) continue;
    if (c < na) {
      if (s_empty[r]) continue;
      double ax = 0.0, ay = 0.0, ac = 0.0;
      for (int s = 0; s < slices; ++s) {
        const double* p = part + ((long)s * R + r) * w + 3 * c;
        ax += p[0]; ay += p[1]; ac += p[2];
      }
      cent[((long)r * na + c) * 2] = (float)(ax / ac);
      cent[((long)r * na + c) * 2 + 1] = (float)(ay / ac);
    }
  }
  __syncthreads();                                                          // every reader of flags[] above is done
  for (int r = tid; r < R; r += LY_THREADS) {
    if (flags[r]) continue;
    double a = 0.0;
    for (int s = 0; s < slices; ++s) a += part[((long)s * R + r) * w + 3 * na];
    const double d = a / (double)n, prev = dist[r];
    dist[r] = d;
    iters[r] += 1;
    const double diff = prev > d ? prev - d : d - prev;                     // prev starts at +inf: the first difference is +inf
    flags[r] = (s_empty[r] ? 3 : 0) | (diff <= thresh ? 1 : 0);
  }
  __syncthreads();
  if (tid == 0) {
    int open = 0;
    for (int r = 0; r < R; ++r) open += flags[r] ? 0 : 1;
    active[0] = open;
  }
}

static int ly_an_slices_ok(int slices, const char* what) {
  LY_CHECK(slices >= 1 && slices <= LY_ANCHOR_SLICES_MAX, "%s: slices=%d outside [1, %d]", what, slices, LY_ANCHOR_SLICES_MAX);
  return 0;
}

extern "C" int ly_anchor_wh(const double* labels, const int* img, long n, const double* shapes, int n_img, const double* scale, float* wh,
                            void* stream) {
  LY_CHECK(n >= 0 && n_img > 0 && shapes, "anchor_wh: bad sizes (n=%ld n_img=%d)", n, n_img);
  if (n == 0) return 0;
  LY_CHECK(labels && img && wh, "anchor_wh: null pointer");
  LY_CHECK((n + LY_THREADS - 1) / LY_THREADS < (1L << 31), "anchor_wh: too many labels (n=%ld)", n);
  hipLaunchKernelGGL(ly_anchor_wh_kernel, dim3((unsigned)((n + LY_THREADS - 1) / LY_THREADS)), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     labels, img, n, shapes, n_img, scale, wh);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_anchor_metric(const float* wh, long n, const float* k, int G, int na, double thr, int slices, double* part, void* stream) {
  LY_CHECK(wh && k && part && n > 0, "anchor_metric: bad arguments (n=%ld)", n);
  LY_CHECK(G >= 1 && G <= 65535 && na >= 1 && na <= LY_ANCHOR_NA_MAX, "anchor_metric: G=%d outside [1, 65535] or na=%d outside [1, %d]", G, na,
           LY_ANCHOR_NA_MAX);
  LY_CHECK(thr > 0.0, "anchor_metric: thr=%f must be positive", thr);
  LY_TRY(ly_an_slices_ok(slices, "anchor_metric"));
  hipLaunchKernelGGL(ly_anchor_metric_kernel, dim3((unsigned)slices, (unsigned)G), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), wh, n, k, na,
                     (float)(1.0 / thr), part);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_anchor_evolve_eval(const float* wh, long n, const double* v, int gen, int na, const double* k, const int* cursor, int B, double thr,
                                     int slices, double* part, void* stream) {
  LY_CHECK(wh && v && k && cursor && part && n > 0 && gen > 0, "anchor_evolve_eval: bad arguments (n=%ld gen=%d)", n, gen);
  LY_CHECK(B >= 1 && B <= LY_THREADS && na >= 1 && na <= LY_ANCHOR_NA_MAX, "anchor_evolve_eval: B=%d outside [1, %d] or na=%d outside [1, %d]", B,
           LY_THREADS, na, LY_ANCHOR_NA_MAX);
  LY_CHECK(thr > 0.0, "anchor_evolve_eval: thr=%f must be positive", thr);
  LY_TRY(ly_an_slices_ok(slices, "anchor_evolve_eval"));
  hipLaunchKernelGGL(ly_anchor_evolve_eval_kernel, dim3((unsigned)slices, (unsigned)B), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), wh, n, v,
                     gen, na, k, cursor, (float)(1.0 / thr), part);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_anchor_evolve_pick(const double* part, int slices, int B, const double* v, int gen, int na, double* k, double* f, int* cursor,
                                     void* stream) {
  LY_CHECK(part && v && k && f && cursor && gen > 0, "anchor_evolve_pick: bad arguments (gen=%d)", gen);
  LY_CHECK(B >= 1 && B <= LY_THREADS && na >= 1 && na <= LY_ANCHOR_NA_MAX, "anchor_evolve_pick: B=%d outside [1, %d] or na=%d outside [1, %d]", B,
           LY_THREADS, na, LY_ANCHOR_NA_MAX);
  LY_TRY(ly_an_slices_ok(slices, "anchor_evolve_pick"));
  hipLaunchKernelGGL(ly_anchor_evolve_pick_kernel, dim3(1), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), part, slices, B, v, gen, na, k, f,
                     cursor);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_kmeans_assign(const float* pts, long n, const float* cent, int R, int na, const int* flags, int slices, double* part, int* assign,
                                void* stream) {
  LY_CHECK(pts && cent && flags && part && n > 0, "kmeans_assign: bad arguments (n=%ld)", n);
  LY_CHECK(R >= 1 && R <= LY_THREADS && na >= 1 && na <= LY_ANCHOR_NA_MAX, "kmeans_assign: R=%d outside [1, %d] or na=%d outside [1, %d]", R, LY_THREADS,
           na, LY_ANCHOR_NA_MAX);
  LY_TRY(ly_an_slices_ok(slices, "kmeans_assign"));
  hipLaunchKernelGGL(ly_kmeans_assign_kernel, dim3((unsigned)slices, (unsigned)R), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), pts, n, cent,
                     na, flags, part, assign);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_kmeans_update(const double* part, int slices, int R, int na, long n, double thresh, float* cent, double* dist, int* count, int* flags,
                                int* iters, int* active, void* stream) {
  LY_CHECK(part && cent && dist && count && flags && iters && active && n > 0, "kmeans_update: bad arguments (n=%ld)", n);
  LY_CHECK(R >= 1 && R <= LY_THREADS && na >= 1 && na <= LY_ANCHOR_NA_MAX, "kmeans_update: R=%d outside [1, %d] or na=%d outside [1, %d]", R, LY_THREADS,
           na, LY_ANCHOR_NA_MAX);
  LY_TRY(ly_an_slices_ok(slices, "kmeans_update"));
  hipLaunchKernelGGL(ly_kmeans_update_kernel, dim3(1), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), part, slices, R, na, n, thresh, cent, dist,
                     count, flags, iters, active);
  LY_LAUNCH_CHECK();
  return 0;
}
