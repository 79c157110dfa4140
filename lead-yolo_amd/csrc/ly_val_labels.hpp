// Label staging shared by the two validation kernels of ly_metrics.hip (ly_val_match, ly_val_confusion): the rows of `targets` with
// image == b, IN ROW ORDER (ordered compaction, LY_THREADS rows at a time), into LDS as val.py prepares them: xywh * (W, H, W, H)
// (val.py:217), xywh2xyxy (val.py:160), and — with a `shapes` row — scale_boxes with ratio_pad + clip_boxes (val.py:161).  The file that
// includes this is compiled with -ffp-contract=off.
#pragma once
#include "ly_boxes.hpp"
#include "ly_common.hpp"
#include "ly_params.h"

#define LY_VAL_OVF_LABELS 1              // bits of the overflow flag
#define LY_VAL_OVF_CLASS 2

struct LyValGeom {                       // one row of `shapes` (h0, w0, gain, padw, padh); native == false: boxes stay on the canvas
  bool native;
  float h0, w0, gain, padw, padh;
};

__device__ __forceinline__ LyValGeom ly_val_geom(const float* __restrict__ shapes, int b) {
  LyValGeom g = {shapes != nullptr, 0.f, 0.f, 1.f, 0.f, 0.f};
  if (g.native) { const float* s = shapes + (long)b * 5; g.h0 = s[0]; g.w0 = s[1]; g.gain = s[2]; g.padw = s[3]; g.padh = s[4]; }
  return g;
}

__device__ __forceinline__ bool ly_val_class_ok(float c, int nc) { return c >= 0.f && c < (float)nc && (float)(int)c == c; }

// Called by every thread of the block, after a barrier behind the initialisation of *s_ovf (and of hist).  -> the number of labels of image
// b (block-uniform); the first LY_VAL_MAX_LABELS of them are in s_box / s_cls (/ s_row: their targets rows, when given).  A label class outside
// [0, nc) sets LY_VAL_OVF_CLASS in *s_ovf and is left out of hist (when given); the label is staged all the same.  Ends behind a barrier when
// nt > 0.
__device__ __forceinline__ int ly_val_stage_labels(const float* __restrict__ targets, long nt, int b, float W, float H, const LyValGeom g, int nc,
                                                   int* hist, int* s_ovf, float (*s_box)[4], float* s_cls, int* s_row, int* s_wcnt) {
  const int tid = threadIdx.x, lane = tid & (LY_WAVE - 1), wave = tid / LY_WAVE;
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
      if (ly_val_class_ok(c, nc)) {
        if (hist) atomicAdd(hist + (int)c, 1);
      } else {
        atomicOr(s_ovf, LY_VAL_OVF_CLASS);
      }
      if (pos < LY_VAL_MAX_LABELS) {
        const float x = t[2] * W, y = t[3] * H, w = t[4] * W, h = t[5] * H;          // val.py:217
        float x1 = x - w / 2, y1 = y - h / 2, x2 = x + w / 2, y2 = y + h / 2;        // xywh2xyxy (utils/general.py:760-767)
        if (g.native) {
          x1 = ly_val_native(x1, g.padw, g.gain, g.w0); x2 = ly_val_native(x2, g.padw, g.gain, g.w0);
          y1 = ly_val_native(y1, g.padh, g.gain, g.h0); y2 = ly_val_native(y2, g.padh, g.gain, g.h0);
        }
        s_box[pos][0] = x1; s_box[pos][1] = y1; s_box[pos][2] = x2; s_box[pos][3] = y2;
        s_cls[pos] = c;
        if (s_row) s_row[pos] = (int)r;
      }
    }
    nl += total;
    __syncthreads();                                         // s_wcnt is rewritten by the next chunk
  }
  return nl;
}

// box_iou (utils/metrics.py:406-424) of the LDS label a with the box (x1, y1, x2, y2) of area area_d: the reference's float32 operations in its
// order
__device__ __forceinline__ float ly_val_iou(const float* a, float x1, float y1, float x2, float y2, float area_d) {
  const float a1x = a[0], a1y = a[1], a2x = a[2], a2y = a[3];
  float iw = fminf(a2x, x2) - fmaxf(a1x, x1), ih = fminf(a2y, y2) - fmaxf(a1y, y1);
  iw = iw < 0.f ? 0.f : iw;
  ih = ih < 0.f ? 0.f : ih;
  const float inter = iw * ih;
  return inter / ((((a2x - a1x) * (a2y - a1y) + area_d) - inter) + 1e-7f);
}
