// Test-time augmentation: the image resampling of utils/torch_utils.py scale_img (same_shape=False), for every scaled pass of a batch in ONE
// launch   (gfx950 only)
//   out_k[n, c, y, x] = bilinear(flip_k ? x.flip(3) : x, Hs_k x Ws_k)[n, c, y, x]   for y < Hs_k, x < Ws_k,   pad   elsewhere (y < Ho_k, x < Wo_k)
// with F.interpolate(mode='bilinear', align_corners=False) index arithmetic (aten/src/ATen/native/UpSample.h, area_pixel_compute_source_index):
//   scale = (float)in / out,  src = max(scale * (dst + 0.5) - 0.5, 0),  i0 = (int)src,  i1 = i0 + (i0 < in - 1),  l1 = src - i0,  l0 = 1 - l1.
// blockIdx.y picks the output spec, so the graph of an augmented forward has one node in front of its fork into passes.  Purely
// bandwidth-bound: a lane owns 16 contiguous output bytes (4 fp32 / 8 16-bit columns of one row) and computes its row and column weights
// inline; the source taps are element loads that neighbouring lanes share through the caches (about one source read per output).  The pad
// region is written by the same stores.  fp32 arithmetic, one rounding to the storage type, vector stores only.
#include "ly_common.hpp"
#include "ly_tile.hpp"

struct LyScaleImgArgs {
  LyScaleImgSpec s[LY_SCALE_IMG_MAX];
  float sh[LY_SCALE_IMG_MAX], sw[LY_SCALE_IMG_MAX];        // (float)H / Hs, (float)W / Ws
};

template <typename T> __device__ __forceinline__ float ly_img_ld(const T* p) { return (float)*p; }

// The half-pixel source taps of one output index along one axis (the arithmetic in the head comment): both resampling kernels of this
// file take their indices and weights from here.
struct LyTaps {
  int i0, i1;
  float w0, w1;
};
__device__ __forceinline__ LyTaps ly_bilinear_taps(const float scale, const int dst, const int in) {
  float f = scale * ((float)dst + 0.5f) - 0.5f;
  f = f < 0.f ? 0.f : f;
  LyTaps t;
  t.i0 = (int)f;
  t.i1 = t.i0 + (t.i0 < in - 1);
  t.w1 = f - (float)t.i0;
  t.w0 = 1.f - t.w1;
  return t;
}

template <typename T>
__global__ __launch_bounds__(LY_THREADS) void ly_scale_img_kernel(const T* __restrict__ x, const int C, const int H, const int W, const int n_img,
                                                                  const float pad, const LyScaleImgArgs a) {
  constexpr int V = 16 / sizeof(T);
  struct alignas(16) Pack { T v[V]; };
  const int k = blockIdx.y;
  const LyScaleImgSpec sp = a.s[k];
  const float sh = a.sh[k], sw = a.sw[k];
  const int wv = sp.Wo / V;
  const unsigned rows = (unsigned)n_img * C * sp.Ho;
  const unsigned total = rows * wv;
  T* const out = reinterpret_cast<T*>(sp.out);
  const T tpad = (T)pad;
  for (unsigned i = blockIdx.x * LY_THREADS + threadIdx.x; i < total; i += gridDim.x * LY_THREADS) {
    const unsigned r = i / wv;                              // output row (n, c, y)
    const int x0 = (int)(i - r * wv) * V;
    const unsigned nc = r / sp.Ho;
    const int oy = (int)(r - nc * sp.Ho);
    Pack pk;
    if (oy >= sp.Hs || x0 >= sp.Ws) {
#pragma unroll
      for (int j = 0; j < V; ++j) pk.v[j] = tpad;
    } else {
      const LyTaps ty = ly_bilinear_taps(sh, oy, H);
      const float wy0 = ty.w0, wy1 = ty.w1;
      const T* const r0 = x + ((size_t)nc * H + ty.i0) * W;
      const T* const r1 = x + ((size_t)nc * H + ty.i1) * W;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int ox = x0 + j;
        if (ox >= sp.Ws) {
          pk.v[j] = tpad;
          continue;
        }
        const LyTaps tx = ly_bilinear_taps(sw, ox, W);
        const float wx0 = tx.w0, wx1 = tx.w1;
        int c0 = tx.i0, c1 = tx.i1;
        if (sp.flip) {                                      // column c of x.flip(3) is column W - 1 - c of x
          c0 = W - 1 - c0;
          c1 = W - 1 - c1;
        }
        const float v = wy0 * (wx0 * ly_img_ld(r0 + c0) + wx1 * ly_img_ld(r0 + c1)) + wy1 * (wx0 * ly_img_ld(r1 + c0) + wx1 * ly_img_ld(r1 + c1));
        pk.v[j] = (T)v;
      }
    }
    *reinterpret_cast<uint4*>(out + (size_t)r * sp.Wo + x0) = __builtin_bit_cast(uint4, pk);
  }
}

extern "C" int ly_scale_img(const void* x, int n_img, int C, int H, int W, const LyScaleImgSpec* specs, int nspec, float pad, int dtype, void* stream) {
  LY_CHECK(dtype == LY_F32 || dtype == LY_BF16 || dtype == LY_F16, "scale_img: unknown dtype %d", dtype);
  LY_CHECK(x && specs && n_img > 0 && C > 0 && H > 0 && W > 0 && nspec >= 1 && nspec <= LY_SCALE_IMG_MAX, "scale_img: null pointer / bad sizes");
  const int V = dtype == LY_F32 ? 4 : 8;
  LyScaleImgArgs a;
  long most = 0;
  for (int k = 0; k < LY_SCALE_IMG_MAX; ++k) a.s[k] = specs[k < nspec ? k : 0];
  for (int k = 0; k < nspec; ++k) {
    const LyScaleImgSpec& s = specs[k];
    LY_CHECK(s.out && ((uintptr_t)s.out & 15) == 0, "scale_img: output %d is NULL or not 16-byte aligned", k);
    LY_CHECK(s.Hs >= 1 && s.Ws >= 1 && s.Hs <= s.Ho && s.Ws <= s.Wo && s.Wo % V == 0, "scale_img: spec %d: %d x %d in %d x %d (Wo a multiple of %d)",
             k, s.Hs, s.Ws, s.Ho, s.Wo, V);
    const long vecs = (long)n_img * C * s.Ho * (s.Wo / V);
    LY_CHECK((long)n_img * C * s.Ho * s.Wo < (1L << 31), "scale_img: output %d too large", k);
    most = vecs > most ? vecs : most;
    a.sh[k] = (float)H / (float)s.Hs;
    a.sw[k] = (float)W / (float)s.Ws;
  }
  for (int k = nspec; k < LY_SCALE_IMG_MAX; ++k) a.sh[k] = a.sw[k] = 1.f;
  // grid-stride: at most 8 blocks of 256 lanes per CU and spec (each lane then walks a few 16-byte vectors)
  long bx = (most + LY_THREADS - 1) / LY_THREADS;
  bx = bx > 2048 ? 2048 : bx;
  const dim3 grid((unsigned)bx, (unsigned)nspec);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == LY_F32)
    hipLaunchKernelGGL(ly_scale_img_kernel<float>, grid, dim3(LY_THREADS), 0, st, reinterpret_cast<const float*>(x), C, H, W, n_img, pad, a);
  else if (dtype == LY_BF16)
    hipLaunchKernelGGL(ly_scale_img_kernel<__bf16>, grid, dim3(LY_THREADS), 0, st, reinterpret_cast<const __bf16*>(x), C, H, W, n_img, pad, a);
  else
    hipLaunchKernelGGL(ly_scale_img_kernel<_Float16>, grid, dim3(LY_THREADS), 0, st, reinterpret_cast<const _Float16*>(x), C, H, W, n_img, pad, a);
  LY_LAUNCH_CHECK();
  return 0;
}

// ---- multi-scale training: the uint8 batch resized for the step (train.py --multi-scale; train.multi_scale_shape) ------------------------
//   out = F.interpolate(x.float() / 255, size=(Ho, Wo), mode='bilinear', align_corners=False)     x uint8 [n, C, H, W], out fp32
// in one launch: the fp32 copy of the source never exists.  A lane owns 16 output bytes — 4 consecutive fp32 columns — of a row.  The work
// is laid out so that a row costs a lane little besides its memory instructions: within one plane (n, c) a WAVE owns one chunk of 64 such
// column vectors and every `phases`-th output row, so
//   * the column taps (4 x (i0, i1, w0, w1)) are computed once per lane, before the row loop, which takes 4 rows at a time so that a
//     lane has the loads of 4 rows in flight;
//   * the row taps are wave-uniform: computed once per row, the two source rows and the output row are scalar base addresses and every
//     load / store is base + a lane offset that does not change from row to row (no multiplications or divisions in the loop);
//   * per row a lane loads its taps from the two source rows (neighbouring lanes share them through the caches), blends the pixel values
//     in fp32, scales the blend by 1/255 (one multiply per output) and writes one 16-byte vector store.
// The taps are what bounds the kernel (16 byte loads per 16-byte store ran at 1.8 TB/s over output + source bytes, whatever the arithmetic
// around them), so WINDOWS = true fetches them as 8-byte windows instead: the taps of an output column pair (i0 of the first ... i1 of the
// second) span at most ceil(scale) + 2 <= 8 source bytes for scale <= 5, so one unaligned 8-byte load per column pair and source row
// holds them, and a tap is a byte of that window at a shift fixed before the row loop.  A window is moved left where it would cross the
// end of the row (W >= 8), so no load leaves the row.  WINDOWS = false (W < 8 or scale > 5): one byte load per tap.
struct LyResizeCols {
  unsigned c0[4], c1[4];                                    // source columns of the 4 outputs; WINDOWS: bit shifts inside the pair's window
  unsigned win[2];                                          // WINDOWS: first byte of each column pair's window
  float w0[4], w1[4];
};

// R output rows oy, oy + step, ... of one lane's 4 columns: the loads of all R rows are issued before the first blend
template <bool WINDOWS, int R>
__device__ __forceinline__ void ly_resize_rows(const unsigned char* __restrict__ xp, float* __restrict__ op, const LyResizeCols& cc, const int H,
                                               const int W, const int Wo, const float sh, const int oy, const int step) {
  unsigned long long q0[R][2], q1[R][2];
  const unsigned char *r0[R], *r1[R];
  float wy0[R], wy1[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const LyTaps ty = ly_bilinear_taps(sh, oy + k * step, H);
    wy0[k] = ty.w0, wy1[k] = ty.w1;
    r0[k] = xp + (size_t)__builtin_amdgcn_readfirstlane(ty.i0) * W;         // wave-uniform: scalar row bases
    r1[k] = xp + (size_t)__builtin_amdgcn_readfirstlane(ty.i1) * W;
    if constexpr (WINDOWS) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        __builtin_memcpy(&q0[k][p], r0[k] + cc.win[p], 8);
        __builtin_memcpy(&q1[k][p], r1[k] + cc.win[p], 8);
      }
    }
  }
  if constexpr (R > 1) __builtin_amdgcn_sched_barrier(0);   // (hipcc otherwise sinks each row's loads behind the previous row's blend)
#pragma unroll
  for (int k = 0; k < R; ++k) {
    float4 v;
    float* const pv = &v.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float t00, t01, t10, t11;
      if constexpr (WINDOWS) {
        t00 = (float)((unsigned)(q0[k][j / 2] >> cc.c0[j]) & 255u), t01 = (float)((unsigned)(q0[k][j / 2] >> cc.c1[j]) & 255u);
        t10 = (float)((unsigned)(q1[k][j / 2] >> cc.c0[j]) & 255u), t11 = (float)((unsigned)(q1[k][j / 2] >> cc.c1[j]) & 255u);
      } else {
        t00 = (float)r0[k][cc.c0[j]], t01 = (float)r0[k][cc.c1[j]], t10 = (float)r1[k][cc.c0[j]], t11 = (float)r1[k][cc.c1[j]];
      }
      const float top = cc.w0[j] * t00 + cc.w1[j] * t01;
      const float bot = cc.w0[j] * t10 + cc.w1[j] * t11;
      pv[j] = (wy0[k] * top + wy1[k] * bot) * (1.f / 255.f);
    }
    *reinterpret_cast<float4*>(op + (size_t)(oy + k * step) * Wo) = v;
  }
}

template <bool WINDOWS>
__global__ __launch_bounds__(LY_THREADS) void ly_resize_u8_kernel(const unsigned char* __restrict__ x, const int H, const int W, float* __restrict__ out,
                                                                  const int Ho, const int Wo, const int chunks, const int bpp, const float sh,
                                                                  const float sw) {
  // grid: planes x bpp blocks; the 4 * bpp waves of a plane = chunks x phases (launcher: bpp a multiple of chunks)
  const int plane = blockIdx.x / bpp;
  const int gw = __builtin_amdgcn_readfirstlane((int)((blockIdx.x - plane * bpp) * (LY_THREADS / 64) + (threadIdx.x >> 6)));
  const int phase = gw / chunks, phases = bpp * (LY_THREADS / 64) / chunks;
  const unsigned x0 = (unsigned)((gw - phase * chunks) * 64 + (threadIdx.x & 63)) * 4;
  if (x0 >= (unsigned)Wo) return;
  LyResizeCols cc;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const LyTaps tx = ly_bilinear_taps(sw, (int)x0 + j, W);
    cc.c0[j] = (unsigned)tx.i0, cc.c1[j] = (unsigned)tx.i1, cc.w0[j] = tx.w0, cc.w1[j] = tx.w1;
  }
  cc.win[0] = cc.win[1] = 0;
  if constexpr (WINDOWS) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      cc.win[p] = cc.c0[2 * p] < (unsigned)W - 8 ? cc.c0[2 * p] : (unsigned)W - 8;
#pragma unroll
      for (int j = 2 * p; j < 2 * p + 2; ++j) cc.c0[j] = (cc.c0[j] - cc.win[p]) * 8, cc.c1[j] = (cc.c1[j] - cc.win[p]) * 8;
    }
  }
  const unsigned char* const xp = x + (size_t)plane * H * W;
  float* const op = out + (size_t)plane * Ho * Wo + x0;
  int oy = phase;
  if constexpr (WINDOWS)                                    // (the byte-tap form keeps one row in flight: its loads sit between its blends)
    for (; oy + 3 * phases < Ho; oy += 4 * phases) ly_resize_rows<WINDOWS, 4>(xp, op, cc, H, W, Wo, sh, oy, phases);
  for (; oy < Ho; oy += phases) ly_resize_rows<WINDOWS, 1>(xp, op, cc, H, W, Wo, sh, oy, phases);
}

extern "C" int ly_resize_u8(const unsigned char* x, int n_img, int C, int H, int W, float* out, int Ho, int Wo, void* stream) {
  LY_CHECK(x && out, "resize_u8: null pointer");
  LY_CHECK(n_img > 0 && C > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "resize_u8: bad sizes %d x %d x %d x %d -> %d x %d", n_img, C, H, W, Ho, Wo);
  LY_CHECK(Wo % 4 == 0, "resize_u8: Wo = %d must be a multiple of 4 (a lane writes 4 fp32 columns)", Wo);
  LY_CHECK(((uintptr_t)out & 15) == 0, "resize_u8: out is not 16-byte aligned");
  LY_CHECK((long)n_img * C * H * W < (1L << 31) && (long)n_img * C * Ho * Wo < (1L << 31), "resize_u8: %d x %d images of %d x %d -> %d x %d: too large",
           n_img, C, H, W, Ho, Wo);
  const long planes = (long)n_img * C;
  const int chunks = (Wo / 4 + 63) / 64;                    // 64-lane column chunks of a row
  // blocks per plane = chunks * k: 4 * k row phases.  k: about 8 blocks per CU over the launch, and no more phases than rows
  long k = (2048 + planes * chunks - 1) / (planes * chunks);
  const long kmax = (Ho + 3) / 4;
  k = k > kmax ? kmax : k;
  const int bpp = (int)(chunks * k);
  const dim3 grid((unsigned)(planes * bpp));
  const float sh = (float)H / (float)Ho, sw = (float)W / (float)Wo;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (W >= 8 && sw <= 5.f)
    hipLaunchKernelGGL(ly_resize_u8_kernel<true>, grid, dim3(LY_THREADS), 0, st, x, H, W, out, Ho, Wo, chunks, bpp, sh, sw);
  else
    hipLaunchKernelGGL(ly_resize_u8_kernel<false>, grid, dim3(LY_THREADS), 0, st, x, H, W, out, Ho, Wo, chunks, bpp, sh, sw);
  LY_LAUNCH_CHECK();
  return 0;
}
