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
      float fy = sh * ((float)oy + 0.5f) - 0.5f;
      fy = fy < 0.f ? 0.f : fy;
      const int y0 = (int)fy;
      const int y1 = y0 + (y0 < H - 1);
      const float wy1 = fy - (float)y0, wy0 = 1.f - wy1;
      const T* const r0 = x + ((size_t)nc * H + y0) * W;
      const T* const r1 = x + ((size_t)nc * H + y1) * W;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int ox = x0 + j;
        if (ox >= sp.Ws) {
          pk.v[j] = tpad;
          continue;
        }
        float fx = sw * ((float)ox + 0.5f) - 0.5f;
        fx = fx < 0.f ? 0.f : fx;
        int c0 = (int)fx;
        int c1 = c0 + (c0 < W - 1);
        const float wx1 = fx - (float)c0, wx0 = 1.f - wx1;
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
