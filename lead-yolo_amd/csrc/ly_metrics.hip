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
//   ly_val_confusion  ConfusionMatrix.process_batch (utils/metrics.py; val.py calls it per image with labels, at conf 0.25 / IoU 0.45) for the same
//                   inputs, one block per image, ADDED to a [(nc + 1)^2] int32 matrix (row: predicted class, column: true class, nc:
//                   background).  Labels and detections are prepared as above.  The reference keeps the pairs with IoU > iou_thres, sorts
//                   them by IoU, keeps the first pair of every detection, sorts again, keeps the first pair of every label.  In closed form,
//                   over the detections with conf > conf_thres: l*(d) = the label OF ANY CLASS with the largest IoU > iou_thres (lowest
//                   row on equal IoU); d*(l) = the detection with the largest IoU among those with l* = l (lowest index on equal IoU).  A
//                   label with a d* counts in M[cls(d*), cls(l)], one without in M[nc, cls(l)]; a kept detection that is not the d* of
//                   its l* counts in M[cls(d), nc] — but only when the image has at least one match (the reference's `if n:`); an image
//                   without labels adds nothing (val.py calls process_batch only for images with labels).
//                   d* comes from a 64-bit LDS atomicMax of (IoU bits << 32) | ~d per label: integer atomics only, independent of
//                   arrival order.  The counts are pre-summed in LDS when the matrix is small (for nc = 1 every add hits one of four cells).
// The file is compiled with -ffp-contract=off: every product, sum and quotient above is the float32 operation the reference performs, in its
// order, so IoUs are bit-equal to the reference's and the `>= level` decisions are the same.
#include <limits.h>

#include "ly_val_labels.hpp"            // label staging, box_iou, the overflow bits; ly_boxes.hpp: ly_val_native

#define LY_VAL_LEVELS 10                 // val.py:171 `iouv = torch.linspace(0.5, 0.95, 10)`; one uint16 bit per level

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
  const int b = blockIdx.x, tid = threadIdx.x;
  const long slot = (long)cursor[0] + b;
  if (slot < 0 || slot >= capacity) return;                 // past the accumulator: nothing is written (the host compares cursor and capacity)
  const LyValGeom g = ly_val_geom(shapes, b);
  int* hist = nt_class + slot * nc;
  for (int c = tid; c < nc; c += LY_THREADS) hist[c] = 0;
  if (tid == 0) s_ovf = 0;
  __syncthreads();

  // ---- labels of image b, in row order (ly_val_labels.hpp)
  int nl = ly_val_stage_labels(targets, nt, b, W, H, g, nc, hist, &s_ovf, s_box, s_cls, s_row, s_wcnt);
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
      if (g.native) {
        x1 = ly_val_native(x1, g.padw, g.gain, g.w0); x2 = ly_val_native(x2, g.padw, g.gain, g.w0);
        y1 = ly_val_native(y1, g.padh, g.gain, g.h0); y2 = ly_val_native(y2, g.padh, g.gain, g.h0);
      }
      const float area_d = (x2 - x1) * (y2 - y1);
      for (int l = 0; l < nl; ++l) {
        if (s_cls[l] != cl) continue;
        const float iou = ly_val_iou(s_box[l], x1, y1, x2, y2, area_d);
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

#define LY_VAL_CM_LDS 1024                // matrices of up to this many cells are pre-summed in LDS (nc <= 31)
#define LY_VAL_CM_MAX_DET 16384           // l*(d) of every detection is kept in dynamic LDS, 2 bytes each

__global__ __launch_bounds__(LY_THREADS) void ly_val_confusion_kernel(const float* __restrict__ dets, const int* __restrict__ counts, int max_det,
                                                                      const float* __restrict__ targets, long nt, float W, float H,
                                                                      const float* __restrict__ shapes, float conf_thres, float iou_thres,
                                                                      int single_cls, int nc, int* matrix, int* flags) {
  __shared__ float s_box[LY_VAL_MAX_LABELS][4];
  __shared__ float s_cls[LY_VAL_MAX_LABELS];
  __shared__ unsigned long long s_best[LY_VAL_MAX_LABELS];  // (IoU bits << 32) | ~d of the label's best detection; 0: none
  __shared__ int s_m[LY_VAL_CM_LDS];
  __shared__ int s_wcnt[LY_THREADS / LY_WAVE];
  __shared__ int s_ovf, s_any;
  extern __shared__ short s_lstar[];                         // [max_det]: l*(d); -1: d is not counted (dropped), -2: kept without a label
  const int b = blockIdx.x, tid = threadIdx.x;
  const LyValGeom g = ly_val_geom(shapes, b);
  const int side = nc + 1, cells = side * side;
  const bool presum = cells <= LY_VAL_CM_LDS;
  if (tid == 0) { s_ovf = 0; s_any = 0; }
  if (presum)
    for (int i = tid; i < cells; i += LY_THREADS) s_m[i] = 0;
  __syncthreads();
  int nl = ly_val_stage_labels(targets, nt, b, W, H, g, nc, nullptr, &s_ovf, s_box, s_cls, nullptr, s_wcnt);
  const bool too_many = nl > LY_VAL_MAX_LABELS;
  if (too_many) nl = 0;                                      // the image is flagged and skipped
  for (int l = tid; l < nl; l += LY_THREADS) s_best[l] = 0ull;
  __syncthreads();
  if (nl > 0) {                                              // block-uniform; an image without labels adds nothing
    int n = counts[b];
    n = n < 0 ? 0 : (n > max_det ? max_det : n);
    // ---- kept detections: the best label of any class above iou_thres; the label keeps its best detection
    for (int d = tid; d < n; d += LY_THREADS) {
      const float* p = dets + ((long)b * max_det + d) * 6;
      int ls = -1;
      if (p[4] > conf_thres) {
        if (!single_cls && !ly_val_class_ok(p[5], nc)) {
          atomicOr(&s_ovf, LY_VAL_OVF_CLASS);                // a detection class outside [0, nc): flagged, not counted
        } else {
          float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
          if (g.native) {
            x1 = ly_val_native(x1, g.padw, g.gain, g.w0); x2 = ly_val_native(x2, g.padw, g.gain, g.w0);
            y1 = ly_val_native(y1, g.padh, g.gain, g.h0); y2 = ly_val_native(y2, g.padh, g.gain, g.h0);
          }
          const float area_d = (x2 - x1) * (y2 - y1);
          float best = iou_thres;
          ls = -2;
          for (int l = 0; l < nl; ++l) {
            if (!ly_val_class_ok(s_cls[l], nc)) continue;    // flagged by the staging, not counted
            const float iou = ly_val_iou(s_box[l], x1, y1, x2, y2, area_d);
            if (iou > best) { best = iou; ls = l; }          // strict: above the threshold, and the lowest label row keeps an equal IoU
          }
          if (ls >= 0) {
            atomicMax(&s_best[ls], ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)~d);       // best > 0: its bits order as integers
            s_any = 1;                                       // every writer stores the same value
          }
        }
      }
      s_lstar[d] = (short)ls;
    }
    __syncthreads();
    // ---- labels: matched -> M[cls(d*), cls(l)], else the background row
    for (int l = tid; l < nl; l += LY_THREADS) {
      if (!ly_val_class_ok(s_cls[l], nc)) continue;
      const int gc = (int)s_cls[l];
      int pc = nc;
      if (s_best[l]) {
        const int d = (int)~(unsigned)s_best[l];
        pc = single_cls ? 0 : (int)dets[((long)b * max_det + d) * 6 + 5];
      }
      atomicAdd(presum ? &s_m[pc * side + gc] : &matrix[pc * side + gc], 1);
    }
    // ---- kept detections that did not get their label -> the background column, only in an image with a match (the reference's `if n:`)
    if (s_any) {
      for (int d = tid; d < n; d += LY_THREADS) {
        const int ls = s_lstar[d];
        if (ls == -1 || (ls >= 0 && (int)~(unsigned)s_best[ls] == d)) continue;
        const int pc = single_cls ? 0 : (int)dets[((long)b * max_det + d) * 6 + 5];
        atomicAdd(presum ? &s_m[pc * side + nc] : &matrix[pc * side + nc], 1);
      }
    }
    if (presum) {
      __syncthreads();
      for (int i = tid; i < cells; i += LY_THREADS)
        if (s_m[i]) atomicAdd(&matrix[i], s_m[i]);
    }
  }
  if (tid == 0) {
    const int f = s_ovf | (too_many ? LY_VAL_OVF_LABELS : 0);
    if (f) atomicOr(flags, f);
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

extern "C" int ly_val_confusion(const float* dets, const int* counts, int bs, int max_det, const float* targets, long nt, int W, int H,
                                const float* shapes, float conf_thres, float iou_thres, int single_cls, int nc, int* matrix, int* flags,
                                void* stream) {
  LY_CHECK(dets && counts && matrix && flags, "val_confusion: null pointer");
  LY_CHECK(bs > 0 && max_det > 0 && max_det <= LY_VAL_CM_MAX_DET && W > 0 && H > 0, "val_confusion: bad sizes (bs=%d max_det=%d [1, %d] W=%d H=%d)", bs,
           max_det, LY_VAL_CM_MAX_DET, W, H);
  LY_CHECK(nt >= 0 && nt <= INT_MAX && (targets || nt == 0), "val_confusion: bad targets (nt=%ld)", nt);
  LY_CHECK(nc >= 1 && nc <= 4096, "val_confusion: nc=%d outside [1, 4096]", nc);
  LY_CHECK(iou_thres >= 0.f, "val_confusion: iou_thres=%f is negative", (double)iou_thres);
  hipLaunchKernelGGL(ly_val_confusion_kernel, dim3((unsigned)bs), dim3(LY_THREADS), (size_t)max_det * sizeof(short),
                     reinterpret_cast<hipStream_t>(stream), dets, counts, max_det, targets, nt, (float)W, (float)H, shapes, conf_thres, iou_thres,
                     single_cls, nc, matrix, flags);
  LY_LAUNCH_CHECK();
  return 0;
}
