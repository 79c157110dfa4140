// On-device training augmentation: the batch that utils/dataloaders.py LoadImagesAndLabels.__getitem__ builds on the CPU (load_mosaic or
// letterbox, random_perspective, augment_hsv, flipud / fliplr, HWC BGR -> CHW RGB) and its collate_fn labels, for a whole batch in two
// launches   (gfx950 only)
//
// ly_mosaic_img: out[b, c, v, u] (uint8 NCHW, s x s, RGB plane order).  Per output pixel: mirror (u, v) for the flips, map it through the
// inverse affine onto the mosaic canvas, take the four bilinear taps there (cv2.warpAffine INTER_LINEAR, BORDER_CONSTANT 114) and round
// once.  A canvas pixel is read from the source tile whose placement rectangle holds it, 114 elsewhere: the 2s x 2s canvas of load_mosaic is
// never stored.  Then the optional HSV step (OpenCV's 8-bit BGR2HSV, the per-image LUTs, OpenCV's float HSV2BGR).  Purely gather-bound: a
// lane owns 16 consecutive output pixels of one row, computes all three channels (HSV needs the whole pixel) and does three 16-byte stores.
// Taps outside every rectangle cost no load.
//
// ly_mosaic_labels: the label rows of the same batch, float64 arithmetic, one block: a candidate slot per (image, tile, label) in that order,
// a ballot scan compacts the survivors image-major, the tail is padding.
//
// ly_mosaic_mix_img / ly_mosaic_mix_labels: the same with mixup (utils/augmentations.py mixup, after a second load_mosaic): an image that
// has a partner entry is the float64 blend, truncated, of the two warped and rounded images, before the HSV step; its label rows are the
// primary's followed by the partner's.  Both kernels share the per-pixel / per-label functions with the plain ones.
// Built with -ffp-contract=off (Makefile): every floating-point operation is the one written, in the order written.
#include "ly_common.hpp"
#include "ly_tile.hpp"

// the layout lead-yolo_amd/capi.py mirrors (ctypes, natural alignment)
static_assert(sizeof(LyMosaicTile) == 72 && sizeof(LyMosaicImage) == 392, "LyMosaicTile / LyMosaicImage layout changed: update capi.py");
static_assert(sizeof(LyMixup) == 16, "LyMixup layout changed");

namespace {

// OpenCV's RGB2HSV_b tables (imgproc/src/color_hsv.simd.hpp, hsv_shift = 12): sdiv[i] = cvRound((255 << 12) / (1. * i)),
// hdiv[i] = cvRound((180 << 12) / (6. * i)); cvRound rounds half to even.  Computed exactly in integers at compile time.
constexpr int kHsvShift = 12;
constexpr int ly_round_div(long n, long d) {
  const long q = n / d, r = n % d;
  return (int)(2 * r > d ? q + 1 : (2 * r == d ? q + (q & 1) : q));
}
struct LyHsvTables {
  int sdiv[256];
  int hdiv[256];
};
constexpr LyHsvTables ly_hsv_make() {
  LyHsvTables t{};
  for (int i = 1; i < 256; ++i) {
    t.sdiv[i] = ly_round_div(255L << kHsvShift, i);
    t.hdiv[i] = ly_round_div(180L << kHsvShift, 6L * i);
  }
  return t;
}
__constant__ const LyHsvTables ly_hsv_tab = ly_hsv_make();

// canvas pixel (cx, cy), channel-interleaved BGR, of image `im`: the tile whose rectangle holds it, else the fill value.  (`im` is
// block-uniform and read-only: its fields come through the scalar cache)
__device__ __forceinline__ void ly_canvas_px(const unsigned char* __restrict__ bank, const LyMosaicImage& im, const int cx, const int cy, float& b,
                                             float& g, float& r) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const LyMosaicTile& tl = im.tile[t];
    if (cx >= tl.x1a && cx < tl.x2a && cy >= tl.y1a && cy < tl.y2a) {
      const unsigned char* p = bank + tl.off + ((long)(cy - tl.y1a + tl.y1b) * tl.w + (cx - tl.x1a + tl.x1b)) * 3;
      b = (float)p[0];
      g = (float)p[1];
      r = (float)p[2];
      return;
    }
  }
  b = g = r = 114.f;
}

__device__ __forceinline__ int ly_u8_round(float acc) {
  const int v = (int)(acc + 0.5f);
  return v > 255 ? 255 : v;
}

// OpenCV RGB2HSV_b (hrange 180) -> LUT -> HSV2RGB_b (float path: h * 6/180, s / 255, v / 255, sector table, x 255, cvRound)
__device__ __forceinline__ void ly_hsv_apply(const unsigned char* __restrict__ lut, int& b, int& g, int& r) {
  int v = b > g ? b : g;
  v = v > r ? v : r;
  int vmin = b < g ? b : g;
  vmin = vmin < r ? vmin : r;
  const int diff = v - vmin;
  const int vr = v == r ? -1 : 0, vg = v == g ? -1 : 0;
  const int s = (diff * ly_hsv_tab.sdiv[v] + (1 << (kHsvShift - 1))) >> kHsvShift;
  int h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))));
  h = (h * ly_hsv_tab.hdiv[diff] + (1 << (kHsvShift - 1))) >> kHsvShift;
  h += h < 0 ? 180 : 0;
  const int h2 = lut[h], s2 = lut[256 + s], v2 = lut[512 + v];
  const float fv = (float)v2 * (1.f / 255.f);
  float fb, fg, fr;
  const float fs = (float)s2 * (1.f / 255.f);
  if (fs == 0.f) {
    fb = fg = fr = fv;
  } else {
    float fh = (float)h2 * (6.f / 180.f);
    fh = fmodf(fh, 6.f);
    int sector = (int)floorf(fh);
    fh -= (float)sector;
    if ((unsigned)sector >= 6u) {
      sector = 0;
      fh = 0.f;
    }
    const float t0 = fv, t1 = fv * (1.f - fs), t2 = fv * (1.f - fs * fh), t3 = fv * (1.f - fs * (1.f - fh));
    // sector_data = {{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}}: the (b, g, r) entries of tab = {t0, t1, t2, t3}, one nibble
    // per sector
    const int sb = (0x200311 >> (4 * sector)) & 15;                // 1,1,3,0,0,2
    const int sg = (0x112003 >> (4 * sector)) & 15;                // 3,0,0,2,1,1
    const int sr = (0x031120 >> (4 * sector)) & 15;                // 0,2,1,1,3,0
    auto tab = [&](const int k) { return k == 0 ? t0 : k == 1 ? t1 : k == 2 ? t2 : t3; };
    fb = tab(sb);
    fg = tab(sg);
    fr = tab(sr);
  }
  // saturate_cast<uchar>(float): round half to even, clamp
  b = (int)fminf(fmaxf(__builtin_rintf(fb * 255.f), 0.f), 255.f);
  g = (int)fminf(fmaxf(__builtin_rintf(fg * 255.f), 0.f), 255.f);
  r = (int)fminf(fmaxf(__builtin_rintf(fr * 255.f), 0.f), 255.f);
}

constexpr int kPx = 16;         // output pixels per lane (one 16-byte store per plane)

// one output pixel of entry `im` before the HSV step: the canvas point of the mirrored column uf (bx = minv[1] * v, by = minv[4] * v, the
// row's share), four taps, one rounding, three channels
__device__ __forceinline__ void ly_warp_px(const unsigned char* __restrict__ bank, const LyMosaicImage& im, const float a0, const float bx,
                                           const float a2, const float a3, const float by, const float a5, const float uf, int& cb, int& cg,
                                           int& cr) {
  // canvas point; the same fp32 operations, in the same order, as the restatement in tests/test_gpu_mosaic.py
  float X = (a0 * uf + bx) + a2;
  float Y = (a3 * uf + by) + a5;
  X = fminf(fmaxf(X, -8.f), 1.0e6f);
  Y = fminf(fmaxf(Y, -8.f), 1.0e6f);
  const float x0 = floorf(X), y0 = floorf(Y);
  float fx = X - x0, fy = Y - y0;
  // keep the two fractions where they are written: computed once this function is inlined, the compiler otherwise moves the subtractions
  // behind the tap loads and carries X, x0, Y, y0 across them instead (2 registers per lane more: 74, and 6 waves per SIMD instead of 7)
  asm("" : "+v"(fx), "+v"(fy));
  const int ix = (int)x0, iy = (int)y0;
  float b00, g00, r00, b01, g01, r01, b10, g10, r10, b11, g11, r11;
  ly_canvas_px(bank, im, ix, iy, b00, g00, r00);
  ly_canvas_px(bank, im, ix + 1, iy, b01, g01, r01);
  ly_canvas_px(bank, im, ix, iy + 1, b10, g10, r10);
  ly_canvas_px(bank, im, ix + 1, iy + 1, b11, g11, r11);
  const float wx0 = 1.f - fx, wy0 = 1.f - fy;
  cb = ly_u8_round(wy0 * (wx0 * b00 + fx * b01) + fy * (wx0 * b10 + fx * b11));
  cg = ly_u8_round(wy0 * (wx0 * g00 + fx * g01) + fy * (wx0 * g10 + fx * g11));
  cr = ly_u8_round(wy0 * (wx0 * r00 + fx * r01) + fy * (wx0 * r10 + fx * r11));
}

// the 16 output pixels at (u0 .. u0 + 15, v) of image b from entry `im` alone: warp, the optional HSV step, three 16-byte stores
__device__ __forceinline__ void ly_plain_px16(const unsigned char* __restrict__ bank, const LyMosaicImage& im, const int s, const int v, const int u0,
                                              unsigned char* __restrict__ o) {
  const float a0 = im.minv[0], a1 = im.minv[1], a2 = im.minv[2], a3 = im.minv[3], a4 = im.minv[4], a5 = im.minv[5];
  const int fud = im.flipud, flr = im.fliplr;
  const unsigned char* lut = im.lut;
  const float vf = (float)(fud ? s - 1 - v : v);
  const float bx = a1 * vf, by = a4 * vf;
  union Px { uint4 q; unsigned char c[16]; };
  Px pr, pg, pb;
#pragma unroll
  for (int j = 0; j < kPx; ++j) {
    const int u = u0 + j;
    const float uf = (float)(flr ? s - 1 - u : u);
    int cb, cg, cr;
    ly_warp_px(bank, im, a0, bx, a2, a3, by, a5, uf, cb, cg, cr);
    if (lut) ly_hsv_apply(lut, cb, cg, cr);
    pr.c[j] = (unsigned char)cr;
    pg.c[j] = (unsigned char)cg;
    pb.c[j] = (unsigned char)cb;
  }
  const size_t plane = (size_t)s * s;
  *reinterpret_cast<uint4*>(o) = pr.q;
  *reinterpret_cast<uint4*>(o + plane) = pg.q;
  *reinterpret_cast<uint4*>(o + 2 * plane) = pb.q;
}

__global__ __launch_bounds__(LY_THREADS) void ly_mosaic_img_kernel(const unsigned char* __restrict__ bank, const LyMosaicImage* __restrict__ imgs,
                                                                   const int s, unsigned char* __restrict__ out) {
  const int b = blockIdx.y;
  const int per_row = s / kPx;
  const int i = blockIdx.x * LY_THREADS + threadIdx.x;
  if (i >= per_row * s) return;
  const int v = i / per_row;
  const int u0 = (i - v * per_row) * kPx;
  ly_plain_px16(bank, imgs[b], s, v, u0, out + (size_t)b * 3 * s * s + (size_t)v * s + u0);
}

// utils/augmentations.py mixup: im = (im * r + im2 * (1 - r)).astype(np.uint8) of two uint8 images, r a float64 — float64 products, one
// float64 sum, truncation; no clamp (a convex combination of two bytes that rounds to 255.00000000000003 truncates to 255)
__device__ __forceinline__ int ly_mixup_blend(const int c1, const int c2, const double r, const double q) {
  return (int)((double)c1 * r + (double)c2 * q);
}

// four consecutive output pixels (columns u .. u + 3 before mirroring) of the blend of entries im and im2 -> one 32-bit word per plane.  The
// two warps of a pixel run one after the other: the first one's taps are dead when the second one's are loaded.  Two pixels in flight, not
// four: unrolled fully the kernel needs 88 registers (5 waves per SIMD, which the images without a partner pay too: 4 % slower than
// ly_mosaic_img_kernel on them, and 789 us instead of 699 us for 64 blended images at 640); with two it needs 72 (7 waves, as the plain kernel)
__device__ __forceinline__ void ly_mix_px4(const unsigned char* __restrict__ bank, const LyMosaicImage& im, const LyMosaicImage& im2,
                                           const float vf, const double r, const double q, const unsigned char* __restrict__ lut, const int flr,
                                           const int s, const int u, unsigned& wr, unsigned& wg, unsigned& wb) {
  const float bx = im.minv[1] * vf, by = im.minv[4] * vf, bx2 = im2.minv[1] * vf, by2 = im2.minv[4] * vf;
  wr = wg = wb = 0u;
#pragma unroll 2
  for (int k = 0; k < 4; ++k) {
    const float uf = (float)(flr ? s - 1 - (u + k) : u + k);
    int cb, cg, cr, cb2, cg2, cr2;
    ly_warp_px(bank, im, im.minv[0], bx, im.minv[2], im.minv[3], by, im.minv[5], uf, cb, cg, cr);
    ly_warp_px(bank, im2, im2.minv[0], bx2, im2.minv[2], im2.minv[3], by2, im2.minv[5], uf, cb2, cg2, cr2);
    cb = ly_mixup_blend(cb, cb2, r, q);
    cg = ly_mixup_blend(cg, cg2, r, q);
    cr = ly_mixup_blend(cr, cr2, r, q);
    if (lut) ly_hsv_apply(lut, cb, cg, cr);
    wr |= (unsigned)cr << (8 * k);
    wg |= (unsigned)cg << (8 * k);
    wb |= (unsigned)cb << (8 * k);
  }
}

// ly_mosaic_img_kernel with mixup: image b is entry b, blended with entry mix[b].partner where that is one.  The partner is warped through
// its own tiles and minv at the same mirrored (u, v); lut and the flips are the primary's.  mix[b] is block-uniform: an image without a
// partner pays a scalar load and runs the plain kernel's loop.  With a partner the 16 pixels are four groups of four written out one by one,
// each packed into a word (as one loop over a byte array the compiler declines to unroll it fully and moves the array to LDS).
__global__ __launch_bounds__(LY_THREADS) void ly_mosaic_mix_img_kernel(const unsigned char* __restrict__ bank, const LyMosaicImage* __restrict__ imgs,
                                                                       const LyMixup* __restrict__ mix, const int n_entry, const int s,
                                                                       unsigned char* __restrict__ out) {
  const int b = blockIdx.y;
  const int per_row = s / kPx;
  const int i = blockIdx.x * LY_THREADS + threadIdx.x;
  if (i >= per_row * s) return;
  const int v = i / per_row;
  const int u0 = (i - v * per_row) * kPx;
  const LyMosaicImage& im = imgs[b];
  const int fud = im.flipud, flr = im.fliplr;
  const unsigned char* lut = im.lut;
  const float vf = (float)(fud ? s - 1 - v : v);
  const int partner = mix[b].partner;
  const size_t plane = (size_t)s * s;
  unsigned char* o = out + (size_t)b * 3 * plane + (size_t)v * s + u0;
  if ((unsigned)partner >= (unsigned)n_entry) {                  // -1 (or an index outside the table): no second image
    ly_plain_px16(bank, im, s, v, u0, o);
  } else {
    const LyMosaicImage& im2 = imgs[partner];
    const double r = mix[b].r, q = 1.0 - r;
    uint4 qr, qg, qb;
    ly_mix_px4(bank, im, im2, vf, r, q, lut, flr, s, u0, qr.x, qg.x, qb.x);
    ly_mix_px4(bank, im, im2, vf, r, q, lut, flr, s, u0 + 4, qr.y, qg.y, qb.y);
    ly_mix_px4(bank, im, im2, vf, r, q, lut, flr, s, u0 + 8, qr.z, qg.z, qb.z);
    ly_mix_px4(bank, im, im2, vf, r, q, lut, flr, s, u0 + 12, qr.w, qg.w, qb.w);
    *reinterpret_cast<uint4*>(o) = qr;
    *reinterpret_cast<uint4*>(o + plane) = qg;
    *reinterpret_cast<uint4*>(o + 2 * plane) = qb;
  }
}

constexpr int kLabThreads = 1024;

// one candidate label: false when it is filtered (or the slot is empty), else its output row (cls, x, y, w, h).  The flips are arguments: a
// mixup partner's rows take its primary's
__device__ bool ly_mosaic_label(const double* __restrict__ labels, const LyMosaicImage& im, const int t, const int j, const int s, const int flipud,
                                const int fliplr, float row[5]) {
  const LyMosaicTile& tl = im.tile[t];
  if (tl.src < 0 || j >= tl.nlab) return false;
  const double* l = labels + (size_t)(tl.lab + j) * 5;
  const double w = tl.w, h = tl.h;
  // xywhn2xyxy(lab, w, h, padw, padh) (utils/general.py)
  double x1 = w * (l[1] - l[3] / 2) + tl.padw;
  double y1 = h * (l[2] - l[4] / 2) + tl.padh;
  double x2 = w * (l[1] + l[3] / 2) + tl.padw;
  double y2 = h * (l[2] + l[4] / 2) + tl.padh;
  if (im.mosaic) {                                            // load_mosaic: np.clip(labels4[:, 1:], 0, 2 * s)
    const double c = 2.0 * s;
    x1 = fmin(fmax(x1, 0.0), c);
    y1 = fmin(fmax(y1, 0.0), c);
    x2 = fmin(fmax(x2, 0.0), c);
    y2 = fmin(fmax(y2, 0.0), c);
  }
  // random_perspective: corners x1y1, x2y2, x1y2, x2y1 through M, min / max, clip to the output
  const double* m = im.m;
  const double cxs[4] = {x1, x2, x1, x2}, cys[4] = {y1, y2, y2, y1};
  double nx0 = 0, ny0 = 0, nx1 = 0, ny1 = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double X = (m[0] * cxs[k] + m[1] * cys[k]) + m[2];
    const double Y = (m[3] * cxs[k] + m[4] * cys[k]) + m[5];
    nx0 = k ? fmin(nx0, X) : X;
    nx1 = k ? fmax(nx1, X) : X;
    ny0 = k ? fmin(ny0, Y) : Y;
    ny1 = k ? fmax(ny1, Y) : Y;
  }
  const double S = s;
  nx0 = fmin(fmax(nx0, 0.0), S);
  nx1 = fmin(fmax(nx1, 0.0), S);
  ny0 = fmin(fmax(ny0, 0.0), S);
  ny1 = fmin(fmax(ny1, 0.0), S);
  // box_candidates(box1 = targets * scale, box2 = new, wh_thr = 2, ar_thr = 100, area_thr = 0.10, eps = 1e-16)
  const double w1 = x2 * im.scale - x1 * im.scale, h1 = y2 * im.scale - y1 * im.scale;
  const double w2 = nx1 - nx0, h2 = ny1 - ny0;
  const double eps = 1e-16;
  const double ar = fmax(w2 / (h2 + eps), h2 / (w2 + eps));
  if (!(w2 > 2.0 && h2 > 2.0 && w2 * h2 / (w1 * h1 + eps) > 0.10 && ar < 100.0)) return false;
  // xyxy2xywhn(w = s, h = s, clip = True, eps = 1e-3)
  const double lim = S - 1e-3;
  nx0 = fmin(fmax(nx0, 0.0), lim);
  nx1 = fmin(fmax(nx1, 0.0), lim);
  ny0 = fmin(fmax(ny0, 0.0), lim);
  ny1 = fmin(fmax(ny1, 0.0), lim);
  double xc = ((nx0 + nx1) / 2) / S, yc = ((ny0 + ny1) / 2) / S;
  if (flipud) yc = 1 - yc;
  if (fliplr) xc = 1 - xc;
  row[0] = (float)l[0];
  row[1] = (float)xc;
  row[2] = (float)yc;
  row[3] = (float)((nx1 - nx0) / S);
  row[4] = (float)((ny1 - ny0) / S);
  return true;
}

// kMix false: 4 * max_labels slots per image (its four tiles).  kMix: 8 * max_labels: half 0 is entry b, half 1 entry mix[b].partner (empty
// when there is none), so that within an image the primary's rows come before the partner's (mixup's np.concatenate)
template <bool kMix>
__global__ __launch_bounds__(kLabThreads) void ly_mosaic_labels_kernel(const double* __restrict__ labels, const LyMosaicImage* __restrict__ imgs,
                                                                       const LyMixup* __restrict__ mix, const int n_img, const int n_entry,
                                                                       const int s, const int max_labels, float* __restrict__ tg, const long cap) {
  __shared__ int wave_cnt[kLabThreads / LY_WAVE];
  const int lane = threadIdx.x & (LY_WAVE - 1), wave = threadIdx.x / LY_WAVE;
  const long per_entry = 4L * max_labels, per_img = kMix ? 2 * per_entry : per_entry;
  const long slots = (long)n_img * per_img;
  long base = 0;
  for (long c0 = 0; c0 < slots; c0 += kLabThreads) {
    const long slot = c0 + threadIdx.x;
    float row[5];
    int b = 0;
    bool keep = false;
    if (slot < slots) {
      b = (int)(slot / per_img);
      int rest = (int)(slot - (long)b * per_img);
      int e = b;
      if (kMix && rest >= per_entry) {
        rest -= (int)per_entry;
        e = mix[b].partner;
      }
      if (!kMix || (unsigned)e < (unsigned)n_entry)
        keep = ly_mosaic_label(labels, imgs[e], rest / max_labels, rest % max_labels, s, imgs[b].flipud, imgs[b].fliplr, row);
    }
    const unsigned long long mask = __ballot(keep);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wave] = __popcll(mask);
    __syncthreads();
    long at = base + before;
    int total = 0;
    for (int w = 0; w < kLabThreads / LY_WAVE; ++w) {
      at += w < wave ? wave_cnt[w] : 0;
      total += wave_cnt[w];
    }
    if (keep && at < cap) {
      float* o = tg + at * 6;
      o[0] = (float)b;
#pragma unroll
      for (int k = 0; k < 5; ++k) o[k + 1] = row[k];
    }
    base += total;
    __syncthreads();
  }
  for (long r = base + threadIdx.x; r < cap; r += kLabThreads) {
    float* o = tg + r * 6;
    o[0] = -1.f;
#pragma unroll
    for (int k = 1; k < 6; ++k) o[k] = 0.f;
  }
}

}  // namespace

extern "C" int ly_mosaic_img(const unsigned char* bank, const LyMosaicImage* imgs, int n_img, int s, unsigned char* out, void* stream) {
  LY_CHECK(bank && imgs && out && n_img > 0, "mosaic_img: null pointer / no images");
  LY_CHECK(s >= 16 && s % 16 == 0 && (long)s * s * 3 * n_img < (1L << 40), "mosaic_img: s = %d must be a positive multiple of 16", s);
  LY_CHECK(((uintptr_t)out & 15) == 0, "mosaic_img: output not 16-byte aligned");
  const long lanes = (long)s * (s / kPx);
  const dim3 grid((unsigned)((lanes + LY_THREADS - 1) / LY_THREADS), (unsigned)n_img);
  hipLaunchKernelGGL(ly_mosaic_img_kernel, grid, dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), bank, imgs, s, out);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_mosaic_labels(const double* labels, const LyMosaicImage* imgs, int n_img, int s, int max_labels, float* targets, long cap,
                                void* stream) {
  LY_CHECK(imgs && targets && n_img > 0 && s > 0 && max_labels >= 0, "mosaic_labels: null pointer / bad sizes");
  LY_CHECK(labels || max_labels == 0, "mosaic_labels: labels NULL with max_labels = %d", max_labels);
  LY_CHECK(cap >= (long)n_img * 4 * max_labels, "mosaic_labels: capacity %ld < n_img * 4 * max_labels = %ld", cap, (long)n_img * 4 * max_labels);
  hipLaunchKernelGGL(ly_mosaic_labels_kernel<false>, dim3(1), dim3(kLabThreads), 0, reinterpret_cast<hipStream_t>(stream), labels, imgs,
                     (const LyMixup*)nullptr, n_img, n_img, s, max_labels, targets, cap);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_mosaic_mix_img(const unsigned char* bank, const LyMosaicImage* imgs, const LyMixup* mix, int n_img, int n_entry, int s,
                                 unsigned char* out, void* stream) {
  LY_CHECK(bank && imgs && mix && out && n_img > 0, "mosaic_mix_img: null pointer / no images");
  LY_CHECK(n_entry >= n_img, "mosaic_mix_img: n_entry = %d < n_img = %d", n_entry, n_img);
  LY_CHECK(s >= 16 && s % 16 == 0 && (long)s * s * 3 * n_img < (1L << 40), "mosaic_mix_img: s = %d must be a positive multiple of 16", s);
  LY_CHECK(((uintptr_t)out & 15) == 0, "mosaic_mix_img: output not 16-byte aligned");
  const long lanes = (long)s * (s / kPx);
  const dim3 grid((unsigned)((lanes + LY_THREADS - 1) / LY_THREADS), (unsigned)n_img);
  hipLaunchKernelGGL(ly_mosaic_mix_img_kernel, grid, dim3(LY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), bank, imgs, mix, n_entry, s, out);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_mosaic_mix_labels(const double* labels, const LyMosaicImage* imgs, const LyMixup* mix, int n_img, int n_entry, int s,
                                    int max_labels, float* targets, long cap, void* stream) {
  LY_CHECK(imgs && mix && targets && n_img > 0 && s > 0 && max_labels >= 0, "mosaic_mix_labels: null pointer / bad sizes");
  LY_CHECK(n_entry >= n_img, "mosaic_mix_labels: n_entry = %d < n_img = %d", n_entry, n_img);
  LY_CHECK(labels || max_labels == 0, "mosaic_mix_labels: labels NULL with max_labels = %d", max_labels);
  LY_CHECK(cap >= (long)n_img * 8 * max_labels, "mosaic_mix_labels: capacity %ld < n_img * 8 * max_labels = %ld", cap,
           (long)n_img * 8 * max_labels);
  hipLaunchKernelGGL(ly_mosaic_labels_kernel<true>, dim3(1), dim3(kLabThreads), 0, reinterpret_cast<hipStream_t>(stream), labels, imgs, mix, n_img,
                     n_entry, s, max_labels, targets, cap);
  LY_LAUNCH_CHECK();
  return 0;
}
