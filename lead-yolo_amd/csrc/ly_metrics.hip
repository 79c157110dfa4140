// Validation scoring on the device: val.py's per-image preparation (val.py:150-166) and `process_batch` (val.py:79-101) for a whole batch in one
// launch, fed by what `nms_padded` returns (dets [bs, max_det, 6], counts [bs]) and by the target tensor ComputeLoss takes ([nt, 6]: image,
// class, normalised xywh), without a host round trip per image.
//
//   ly_val_match    one block per image b, results into slot cursor + b of a pre-allocated accumulator:
//     labels        the rows of `targets` with image == b, IN ROW ORDER (ordered compaction, LY_THREADS rows at a time), into LDS:
//                   xywh * (W, H, W, H) (val.py:217), then xywh2xyxy (val.py:160; x - w / 2 ...), then — with a `shapes` row —
//                   scale_boxes with ratio_pad and clip_boxes (val.py:161; utils/general.py:800-829)
//     detections    one thread per detection: single_cls forces the class to 0 (val.py:152); the box copy used for matching takes the same
//                   scale_boxes / clip_boxes (val.py:157-158); box_iou (utils/metrics.py:406-424) against every LDS label of its class
//     matching      the reference sorts the (label, detection) pairs of a level by IoU, keeps the first pair of every detection
//                   (np.unique over detections), then the first pair of every label (np.unique over labels; the re-sort between the
//                   two is commented out in the reference, so the second pass sees the pairs in detection order).  In closed form:
//                   l*(d) = the label of d's class with the largest IoU, iou*(d) that IoU; at level i detection d is correct iff
//                   iou*(d) >= level[i] and d is the lowest-indexed detection among those with the same l* that pass level i.
//                   A detection whose best label is taken is NOT moved to its second-best label.  On EQUAL IoU the lowest label row
//                   wins here; the reference's order under ties comes from an unstable argsort and is unspecified.  Labels without
//                   overlap (IoU == 0) never match: match_label = -1, match_iou = 0.
//                   LDS atomicMin of d into first[label][level], a barrier, then bit i of `correct` survives iff first == d: integer
//                   atomics only, the result does not depend on arrival order.
//   ly_val_advance  one thread: cursor += bs, behind ly_val_match on the same stream — a captured (match, advance) pair replays batch
//                   after batch.
// The file is compiled with -ffp-contract=off: every product, sum and quotient above is the float32 operation the reference performs, in its
// order, so IoUs are bit-equal to the reference's and the `>= level` decisions are the same.
#include <limits.h>

#include "ly_boxes.hpp"                 // ly_val_native: scale_boxes with ratio_pad + clip_boxes
#include "ly_common.hpp"
#include "ly_params.h"

#define LY_VAL_LEVELS 10                 // val.py:171 `iouv = torch.linspace(0.5, 0.95, 10)`; one uint16 bit per level
#define LY_VAL_OVF_LABELS 1              // bits of the per-slot overflow flag
#define LY_VAL_OVF_CLASS 2

static_assert(LY_VAL_MAX_LABELS >= 512 && LY_VAL_MAX_LABELS * (LY_VAL_LEVELS + 6) * 4 + 64 <= 65536, "labels + first[][] must fit static LDS");

__global__ __launch_bounds__(LY_THREADS) void ly_val_match_kernel(const float* __restrict__ dets, const int* __restrict__ counts, int max_det,
                                                                  const float* __restrict__ targets, long nt, float W, float H,
                                                                  const float* __restrict__ shapes, const float* __restrict__ levels,
                                                                  int single_cls, int nc, const int* __restrict__ cursor, int capacity,
                                                                  int row_width, unsigned short* correct, float* __restrict__ conf,
                                                                  float* __restrict__ cls_out, int* match_label, float* __restrict__ match_iou,
                                                                  int* __restrict__ n_det, int* nt_class, int* __restrict__ overflow) {
  __shared__ float s_box[LY_VAL_MAX_LABELS][4];
  __shared__ float s_cls[LY_VAL_MAX_LABELS];
  __shared__ int s_row[LY_VAL_MAX_LABELS];
  __shared__ int s_first[LY_VAL_MAX_LABELS * LY_VAL_LEVELS];
  __shared__ int s_wcnt[LY_THREADS / LY_WAVE];
  __shared__ int s_ovf;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (LY_WAVE - 1), wave = tid / LY_WAVE;
  const long slot = (long)cursor[0] + b;
  if (slot < 0 || slot >= capacity) return;                 // past the accumulator: nothing is written (the host compares cursor and capacity)
  const bool native = shapes != nullptr;
  float h0 = 0.f, w0 = 0.f, gain = 1.f, padw = 0.f, padh = 0.f;
  if (native) { const float* s = shapes + (long)b * 5; h0 = s[0]; w0 = s[1]; gain = s[2]; padw = s[3]; padh = s[4]; }
  int* hist = nt_class + slot * nc;
  for (int c = tid; c < nc; c += LY_THREADS) hist[c] = 0;
  if (tid == 0) s_ovf = 0;
  __syncthreads();

  // ---- labels of image b, in row order
  int nl = 0;                                                // labels seen so far (block-uniform)
  for (long base = 0; base < nt; base += LY_THREADS) {
    const long r = base + tid;
    const bool mine = r < nt && targets[r * 6] == (float)b;
    const unsigned long long bal = __ballot(mine);
    if (lane == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();
    int pos = nl + __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
    for (int k = 0; k < LY_THREADS / LY_WAVE; ++k) {
      if (k < wave) pos += s_wcnt[k];
      total += s_wcnt[k];
    }
    if (mine) {
      const float* t = targets + r * 6;
      const float c = t[1];
      const int ci = (int)c;
      if (c >= 0.f && c < (float)nc && (float)ci == c) atomicAdd(hist + ci, 1);
      else atomicOr(&s_ovf, LY_VAL_OVF_CLASS);
      if (pos < LY_VAL_MAX_LABELS) {
        const float x = t[2] * W, y = t[3] * H, w = t[4] * W, h = t[5] * H;          // val.py:217
        float x1 = x - w / 2, y1 = y - h / 2, x2 = x + w / 2, y2 = y + h / 2;        // xywh2xyxy (utils/general.py:760-767)
        if (native) {
          x1 = ly_val_native(x1, padw, gain, w0); x2 = ly_val_native(x2, padw, gain, w0);
          y1 = ly_val_native(y1, padh, gain, h0); y2 = ly_val_native(y2, padh, gain, h0);
        }
        s_box[pos][0] = x1; s_box[pos][1] = y1; s_box[pos][2] = x2; s_box[pos][3] = y2;
        s_cls[pos] = c;
        s_row[pos] = (int)r;
      }
    }
    nl += total;
    __syncthreads();                                         // s_wcnt is rewritten by the next chunk
  }
  const bool too_many = nl > LY_VAL_MAX_LABELS;
  if (too_many) nl = 0;                                      // the image is flagged and its matching skipped
  for (int i = tid; i < nl * LY_VAL_LEVELS; i += LY_THREADS) s_first[i] = INT_MAX;
  float lv[LY_VAL_LEVELS];
#pragma unroll
  for (int i = 0; i < LY_VAL_LEVELS; ++i) lv[i] = levels[i];
  __syncthreads();

  // ---- detections: best label of the class, its IoU, the levels it passes
  int n = counts[b];
  n = n < 0 ? 0 : (n > max_det ? max_det : n);
  const long row = slot * row_width;
  for (int d = tid; d < row_width; d += LY_THREADS) {
    unsigned mask = 0u;
    int best_l = -1;
    float best = 0.f, cf = 0.f, cl = 0.f;
    if (d < n) {
      const float* p = dets + ((long)b * max_det + d) * 6;
      float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
      cf = p[4];
      cl = single_cls ? 0.f : p[5];
      if (native) {
        x1 = ly_val_native(x1, padw, gain, w0); x2 = ly_val_native(x2, padw, gain, w0);
        y1 = ly_val_native(y1, padh, gain, h0); y2 = ly_val_native(y2, padh, gain, h0);
      }
      const float area_d = (x2 - x1) * (y2 - y1);
      for (int l = 0; l < nl; ++l) {
        if (s_cls[l] != cl) continue;
        const float a1x = s_box[l][0], a1y = s_box[l][1], a2x = s_box[l][2], a2y = s_box[l][3];
        float iw = fminf(a2x, x2) - fmaxf(a1x, x1), ih = fminf(a2y, y2) - fmaxf(a1y, y1);
        iw = iw < 0.f ? 0.f : iw;
        ih = ih < 0.f ? 0.f : ih;
        const float inter = iw * ih;
        const float iou = inter / ((((a2x - a1x) * (a2y - a1y) + area_d) - inter) + 1e-7f);
        if (iou > best) { best = iou; best_l = l; }           // strict: the lowest label row keeps an equal IoU
      }
      if (best_l >= 0) {
#pragma unroll
        for (int i = 0; i < LY_VAL_LEVELS; ++i)
          if (best >= lv[i]) {
            mask |= 1u << i;
            atomicMin(&s_first[best_l * LY_VAL_LEVELS + i], d);
          }
      }
    }
    correct[row + d] = (unsigned short)mask;                  // provisional: the levels d passes
    match_label[row + d] = best_l;                            // provisional: the LDS index (d >= n: rewritten below)
    conf[row + d] = cf;
    cls_out[row + d] = cl;
    match_iou[row + d] = best;
  }
  __syncthreads();
  // ---- a label credits its lowest-indexed (most confident) candidate of each level; every thread revisits the rows it wrote itself
  for (int d = tid; d < row_width; d += LY_THREADS) {
    const int l = match_label[row + d];
    if (d >= n) { match_label[row + d] = 0; continue; }
    if (l < 0) continue;
    unsigned mask = correct[row + d];
#pragma unroll
    for (int i = 0; i < LY_VAL_LEVELS; ++i)
      if ((mask >> i & 1u) && s_first[l * LY_VAL_LEVELS + i] != d) mask &= ~(1u << i);
    correct[row + d] = (unsigned short)mask;
    match_label[row + d] = s_row[l];
  }
  if (tid == 0) {
    n_det[slot] = n;
    overflow[slot] = s_ovf | (too_many ? LY_VAL_OVF_LABELS : 0);
  }
}

__global__ void ly_val_advance_kernel(int* cursor, int bs) { cursor[0] += bs; }

extern "C" int ly_val_match(const float* dets, const int* counts, int bs, int max_det, const float* targets, long nt, int W, int H,
                            const float* shapes, const float* levels, int single_cls, int nc, const int* cursor, int capacity, int row_width,
                            void* correct, float* conf, float* cls, int* match_label, float* match_iou, int* n_det, int* nt_class, int* overflow,
                            void* stream) {
  LY_CHECK(dets && counts && levels && cursor && correct && conf && cls && match_label && match_iou && n_det && nt_class && overflow,
           "val_match: null pointer");
  LY_CHECK(bs > 0 && max_det > 0 && W > 0 && H > 0 && capacity > 0, "val_match: bad sizes (bs=%d max_det=%d W=%d H=%d capacity=%d)", bs, max_det, W, H,
           capacity);
  LY_CHECK(nt >= 0 && nt <= INT_MAX && (targets || nt == 0), "val_match: bad targets (nt=%ld)", nt);
  LY_CHECK(max_det <= row_width, "val_match: max_det=%d exceeds the accumulator's row width %d", max_det, row_width);
  LY_CHECK(nc >= 1 && nc <= 4096, "val_match: nc=%d outside [1, 4096]", nc);
  hipLaunchKernelGGL(ly_val_match_kernel, dim3((unsigned)bs), dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), dets, counts, max_det, targets, nt,
                     (float)W, (float)H, shapes, levels, single_cls, nc, cursor, capacity, row_width, reinterpret_cast<unsigned short*>(correct), conf, cls,
                     match_label, match_iou, n_det, nt_class, overflow);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_val_advance(int* cursor, int bs, void* stream) {
  LY_CHECK(cursor && bs > 0, "val_advance: bad arguments (bs=%d)", bs);
  hipLaunchKernelGGL(ly_val_advance_kernel, dim3(1), dim3(1), 0, reinterpret_cast<hipStream_t>(stream), cursor, bs);
  LY_LAUNCH_CHECK();
  return 0;
}
