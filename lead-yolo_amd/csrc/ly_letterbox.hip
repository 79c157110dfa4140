// Detect input path on the device: what the reference does per image on the CPU between the decoder and the model, and between NMS and the
// caller, for a whole batch in one launch each   (gfx950 only)
//
// ly_letterbox_u8: utils/augmentations.py letterbox (cv2.resize INTER_LINEAR + cv2.copyMakeBorder(114)) and the HWC BGR -> CHW RGB
// transpose of utils/dataloaders.py LoadImages.__next__ (layout LY_LB_CHW_RGB), or the cv2.resize of load_image into the image bank (layout
// LY_LB_HWC_BGR).  One entry of the device table per blockIdx.y; the grid covers maxH x maxW and the lanes past an entry's own H x W exit.
// A lane owns 16 consecutive pixels of one canvas row: the two source rows and the vertical weights are the lane's, the horizontal taps are
// per pixel, and the 16-byte groups that straddle the picture's edge mix border and picture pixel by pixel.  The arithmetic is OpenCV's
// 8-bit INTER_LINEAR in integers (the contract in include/lead_yolo_hip.h); equal sizes take the same path with the weights (2048, 0),
// which is the identity.  Every source index is clamped to the source, addresses are 64-bit.  Bandwidth-bound: the source rows of an
// output row are shared by neighbouring lanes through the caches, nothing is staged.
//
// ly_scale_boxes: utils/general.py scale_boxes + clip_boxes (+ .round()) on the padded rows nms_padded returns, one thread per row.
// Built with -ffp-contract=off (Makefile): the tap positions and the box arithmetic are the operations written, in the order written.
#include "ly_boxes.hpp"
#include "ly_common.hpp"
#include "ly_params.h"

// the layout lead-yolo_amd/capi.py mirrors (ctypes, natural alignment)
static_assert(sizeof(LyLetterboxImage) == 48, "LyLetterboxImage layout changed: lead-yolo_amd/predict.py fills it field by field");

namespace {

constexpr int kPx = 16;         // canvas pixels per lane (CHW: one 16-byte store per plane)
constexpr int kFill = 114;      // letterbox's border colour
constexpr int kCoef = 2048;     // INTER_RESIZE_COEF_SCALE

struct LyLbTap {
  int i0, i1;                   // the two source indices
  int c0, c1;                   // their weights, c0 + c1 = 2048 up to rounding
};

// destination index d of n_dst onto a source of n_src: OpenCV's resize tables (imgproc/src/resize.cpp, INTER_LINEAR, 8-bit)
__device__ __forceinline__ LyLbTap ly_lb_tap(const int d, const int n_dst, const int n_src) {
  const double scale = 1.0 / ((double)n_dst / n_src);
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) {
    s = 0;
    f = 0.f;
  }
  if (s >= n_src - 1) {
    s = n_src - 1;
    f = 0.f;
  }
  LyLbTap t;
  t.i0 = s;
  t.i1 = s + 1 < n_src ? s + 1 : n_src - 1;
  t.c1 = (int)__builtin_rintf(f * 2048.f);
  t.c0 = (int)__builtin_rintf((1.f - f) * 2048.f);
  return t;
}

template <int LAYOUT>
__global__ __launch_bounds__(LY_THREADS) void ly_letterbox_kernel(const LyLetterboxImage* __restrict__ imgs, const int maxH, const int per_row) {
  const LyLetterboxImage& im = imgs[blockIdx.y];          // block-uniform, read-only: its fields come through the scalar cache
  const int i = blockIdx.x * LY_THREADS + threadIdx.x;
  const int v = i / per_row;
  const int u0 = (i - v * per_row) * kPx;
  const int H = im.H, W = im.W;
  if (v >= maxH || v >= H || u0 >= W) return;
  // an entry that breaks the CHW contract (W % 16, alignment) is left unwritten rather than written out of bounds
  if (LAYOUT == LY_LB_CHW_RGB && (u0 + kPx > W || ((uintptr_t)im.dst & 15) != 0)) return;
  const int h0 = im.h0, w0 = im.w0, nh = im.nh, nw = im.nw, left = im.left;
  const int dy = v - im.top;
  const bool copy = nh == h0 && nw == w0;
  const bool row_in = h0 >= 1 && w0 >= 1 && nw >= 1 && dy >= 0 && dy < nh;
  LyLbTap ty = {0, 0, kCoef, 0};
  if (row_in) ty = copy ? LyLbTap{dy, dy, kCoef, 0} : ly_lb_tap(dy, nh, h0);
  const unsigned char* row0 = im.src + (size_t)ty.i0 * w0 * 3;
  const unsigned char* row1 = im.src + (size_t)ty.i1 * w0 * 3;
  union Px { uint4 q; unsigned char c[16]; };
  Px pr, pg, pb;
#pragma unroll
  for (int j = 0; j < kPx; ++j) {
    const int dx = u0 + j - left;
    int bgr[3] = {kFill, kFill, kFill};
    if (row_in && dx >= 0 && dx < nw) {
      const LyLbTap tx = copy ? LyLbTap{dx, dx, kCoef, 0} : ly_lb_tap(dx, nw, w0);
      const unsigned char* p00 = row0 + (size_t)tx.i0 * 3;
      const unsigned char* p01 = row0 + (size_t)tx.i1 * 3;
      const unsigned char* p10 = row1 + (size_t)tx.i0 * 3;
      const unsigned char* p11 = row1 + (size_t)tx.i1 * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int r0 = (int)p00[c] * tx.c0 + (int)p01[c] * tx.c1;
        const int r1 = (int)p10[c] * tx.c0 + (int)p11[c] * tx.c1;
        bgr[c] = (((ty.c0 * (r0 >> 4)) >> 16) + ((ty.c1 * (r1 >> 4)) >> 16) + 2) >> 2;
      }
    }
    if (LAYOUT == LY_LB_CHW_RGB) {
      pb.c[j] = (unsigned char)bgr[0];
      pg.c[j] = (unsigned char)bgr[1];
      pr.c[j] = (unsigned char)bgr[2];
    } else if (u0 + j < W) {
      unsigned char* o = im.dst + ((size_t)v * W + (u0 + j)) * 3;
      o[0] = (unsigned char)bgr[0];
      o[1] = (unsigned char)bgr[1];
      o[2] = (unsigned char)bgr[2];
    }
  }
  if (LAYOUT == LY_LB_CHW_RGB) {
    const size_t plane = (size_t)H * W;
    unsigned char* o = im.dst + (size_t)v * W + u0;
    *reinterpret_cast<uint4*>(o) = pr.q;
    *reinterpret_cast<uint4*>(o + plane) = pg.q;
    *reinterpret_cast<uint4*>(o + 2 * plane) = pb.q;
  }
}

__global__ __launch_bounds__(LY_THREADS) void ly_scale_boxes_kernel(const float* dets, const int* __restrict__ counts, const long rows,
                                                                    const int max_det, const float* __restrict__ shapes, const int round_boxes,
                                                                    float* out) {
  const long i = (long)blockIdx.x * LY_THREADS + threadIdx.x;
  if (i >= rows) return;
  const int b = (int)(i / max_det);
  const int d = (int)(i - (long)b * max_det);
  float* o = out + i * 6;
  if (d >= counts[b]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = 0.f;
    return;
  }
  const float* p = dets + i * 6;                           // read whole before the first store: out may alias dets
  const float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3], cf = p[4], cl = p[5];
  const float* s = shapes + (long)b * 5;
  const float h0 = s[0], w0 = s[1], gain = s[2], padw = s[3], padh = s[4];
  float q[4] = {ly_val_native(x1, padw, gain, w0), ly_val_native(y1, padh, gain, h0), ly_val_native(x2, padw, gain, w0),
                ly_val_native(y2, padh, gain, h0)};
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = round_boxes ? __builtin_rintf(q[k]) : q[k];
  o[4] = cf;
  o[5] = cl;
}

}  // namespace

extern "C" int ly_letterbox_u8(const LyLetterboxImage* imgs, int n_img, int maxH, int maxW, int layout, void* stream) {
  LY_CHECK(imgs && n_img > 0 && n_img <= 65535, "letterbox_u8: null table / n_img = %d outside [1, 65535]", n_img);
  LY_CHECK(layout == LY_LB_CHW_RGB || layout == LY_LB_HWC_BGR, "letterbox_u8: unknown layout %d", layout);
  LY_CHECK(maxH >= 1 && maxW >= 1 && maxH <= 32768 && maxW <= 32768, "letterbox_u8: canvas %d x %d outside [1, 32768]", maxH, maxW);
  LY_CHECK(layout != LY_LB_CHW_RGB || maxW % kPx == 0, "letterbox_u8: the CHW layout needs W a multiple of 16 (maxW = %d)", maxW);
  const int per_row = (maxW + kPx - 1) / kPx;
  const long lanes = (long)maxH * per_row;
  const dim3 grid((unsigned)((lanes + LY_THREADS - 1) / LY_THREADS), (unsigned)n_img);
  if (layout == LY_LB_CHW_RGB)
    hipLaunchKernelGGL(ly_letterbox_kernel<LY_LB_CHW_RGB>, grid, dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), imgs, maxH, per_row);
  else
    hipLaunchKernelGGL(ly_letterbox_kernel<LY_LB_HWC_BGR>, grid, dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), imgs, maxH, per_row);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_scale_boxes(const float* dets, const int* counts, int bs, int max_det, const float* shapes, int round_boxes, float* out,
                              void* stream) {
  LY_CHECK(dets && counts && shapes && out, "scale_boxes: null pointer");
  LY_CHECK(bs > 0 && max_det > 0 && (long)bs * max_det < (1L << 31), "scale_boxes: bad sizes (bs=%d max_det=%d)", bs, max_det);
  const long rows = (long)bs * max_det;
  hipLaunchKernelGGL(ly_scale_boxes_kernel, dim3((unsigned)((rows + LY_THREADS - 1) / LY_THREADS)), dim3(LY_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), dets, counts, rows, max_det, shapes, round_boxes, out);
  LY_LAUNCH_CHECK();
  return 0;
}
