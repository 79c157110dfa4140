// Fused multi-tensor Adam / AdamW step of the training loop, fp32 master weights, gfx950 — the `--optimizer Adam|AdamW` form of
// ly_optim.hip (reference utils/torch_utils.py:318-346 smart_optimizer, train.py:330-341, torch.optim.Adam's foreach update).
//
// Per optimisation step, three launches over the same device table form as ly_optim_step (4096-element blocks):
//   ly_adam_norm    sum of squares of every gradient -> ws[0] (double; zeroed by the previous call's finish)
//   ly_adam_update  coef = min(1, max_norm / (sqrt(ws[0]) * scale + 1e-6));  g' = g * coef * scale (Adam: + wd*p);  AdamW: p *= 1 - lr*wd;
//                   m = lerp(m, g', 1 - b1);  v = b2*v + (1 - b2)*g'*g';  p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps);
//                   g = 0;  ema = d*ema + (1-d)*p;  entries without a gradient (BatchNorm running statistics) take the EMA update only
//   ly_adam_finish  ws[0] = 0, EMA updates += 1, T += 1
// t = T + 1 - step0 per entry (a parameter whose state was created or loaded at another step count than its neighbours'), the two
// bias corrections in double once per block, as torch computes them on the host.  Every step-dependent value lives in the device
// array `hyper`, so the launches can be captured into the hipGraph of the whole step.
#include "ly_common.hpp"
#include "ly_params.h"

#define LY_ADAM_CHUNK 4096                // elements per block (= LY_OPT_CHUNK of ly_optim.hip: the host builds both tables alike)

// hyper: [0..2] lr of groups 0..2, [3] beta1, [4] beta2, [5] eps, [6] max_norm (<= 0: no clipping), [7] ema decay (< 0: no EMA),
//        [8] ema tau, [9] ema updates so far, [10] gradient scale, [11] T = Adam steps taken so far

__device__ __forceinline__ bool ly_al16(const void* q) { return ((unsigned long)q & 15) == 0; }

__global__ __launch_bounds__(LY_THREADS) void ly_adam_norm_kernel(const LyAdamTensor* __restrict__ tab, const int* __restrict__ blk_tensor,
                                                                  const long* __restrict__ blk_off, double* __restrict__ ws) {
  __shared__ float red[4];
  const LyAdamTensor t = tab[blk_tensor[blockIdx.x]];
  float s = 0.f;
  if (t.g) {
    // the sum of squares does not depend on the element order: a tap-major gradient is read in its storage order
    const long off = blk_off[blockIdx.x];
    const long end = off + LY_ADAM_CHUNK < t.n ? off + LY_ADAM_CHUNK : t.n;
    long i0 = off;
    if (ly_al16(t.g)) {                   // off is a multiple of 4096: the block's first element keeps the tensor's alignment
      const long nv = (end - off) >> 2;
      const f32x4* g4 = reinterpret_cast<const f32x4*>(t.g + off);
      for (long j = threadIdx.x; j < nv; j += LY_THREADS) {
        const f32x4 v = g4[j];
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
      }
      i0 = off + 4 * nv;
    }
    for (long i = i0 + threadIdx.x; i < end; i += LY_THREADS) { const float v = t.g[i]; s += v * v; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0 && t.g) atomicAdd(ws, (double)(red[0] + red[1] + red[2] + red[3]));
}

struct LyAdamCoef {
  float gmul;      // clip coefficient * gradient scale
  float wd_g;      // Adam: weight decay added to the gradient (0 for AdamW)
  float pmul;      // AdamW: 1 - lr * wd (1 for Adam)
  float w1;        // 1 - beta1 (lerp weight)
  float b2, w2;    // beta2, 1 - beta2
  float bc2s;      // sqrt(1 - beta2^t)
  float eps;
  float nstep;     // -lr / (1 - beta1^t)
};

// one element; the operation order of torch's foreach Adam (_multi_tensor_adam, capturable = False)
__device__ __forceinline__ float ly_adam_elem(float p, float g, float& m, float& v, const LyAdamCoef& k) {
  g = g * k.gmul;
  g += k.wd_g * p;
  p *= k.pmul;
  m = k.w1 < 0.5f ? m + k.w1 * (g - m) : g - (g - m) * (1.f - k.w1);      // torch's lerp
  v = k.b2 * v + k.w2 * g * g;
  return p + k.nstep * (m / (sqrtf(v) / k.bc2s + k.eps));
}

__global__ __launch_bounds__(LY_THREADS) void ly_adam_update_kernel(const LyAdamTensor* __restrict__ tab, const int* __restrict__ blk_tensor,
                                                                    const long* __restrict__ blk_off, const double* __restrict__ ws,
                                                                    const float* __restrict__ hyper, int decoupled, float* __restrict__ norm_out) {
  __shared__ float bc[2];
  const LyAdamTensor t = tab[blk_tensor[blockIdx.x]];
  const long off = blk_off[blockIdx.x];
  const long end = off + LY_ADAM_CHUNK < t.n ? off + LY_ADAM_CHUNK : t.n;
  const float b1 = hyper[3], b2 = hyper[4], max_norm = hyper[6], ema_decay = hyper[7], tau = hyper[8], updates = hyper[9] + 1.f;
  const float gscale = hyper[10];
  const float total = (float)sqrt(ws[0]) * gscale;          // norm of the scaled gradients
  float coef = 1.f;
  if (max_norm > 0.f) { coef = max_norm / (total + 1e-6f); coef = coef > 1.f ? 1.f : coef; }
  if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) *norm_out = total;
  const float d = ema_decay >= 0.f ? ema_decay * (1.f - __expf(-updates / tau)) : 0.f;
  const float lr = t.group >= 0 ? hyper[t.group] : 0.f;
  if (threadIdx.x == 0 && t.g) {
    const double step = (double)((long)hyper[11] + 1 - t.step0);
    const double bc1 = 1.0 - pow((double)b1, step), bc2 = 1.0 - pow((double)b2, step);
    bc[0] = (float)(-(double)lr / bc1);
    bc[1] = (float)sqrt(bc2);
  }
  __syncthreads();
  LyAdamCoef k;
  k.gmul = coef * gscale;
  k.wd_g = decoupled ? 0.f : t.wd;
  k.pmul = decoupled ? (float)(1.0 - (double)lr * (double)t.wd) : 1.f;
  k.w1 = (float)(1.0 - (double)b1);
  k.b2 = b2;
  k.w2 = (float)(1.0 - (double)b2);
  k.eps = hyper[5];
  k.nstep = bc[0];
  k.bc2s = bc[1];
  const bool ema = t.ema && ema_decay >= 0.f;
  long i0 = off;
  // 16-byte form: contiguous gradient (not tap-major) and every pointer 16-byte aligned (a stacked pair's second half need not be)
  if (t.taps <= 1 && ly_al16(t.p) && (!t.g || (ly_al16(t.g) && ly_al16(t.m) && ly_al16(t.v))) && (!t.ema || ly_al16(t.ema))) {
    const long nv = (end - off) >> 2;
    for (long j = threadIdx.x; j < nv; j += LY_THREADS) {
      const long i = off + 4 * j;
      f32x4 p = *reinterpret_cast<const f32x4*>(t.p + i);
      if (t.g) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(t.g + i);
        f32x4 m = *reinterpret_cast<const f32x4*>(t.m + i), v = *reinterpret_cast<const f32x4*>(t.v + i);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float mc = m[c], vc = v[c];
          p[c] = ly_adam_elem(p[c], g[c], mc, vc, k);
          m[c] = mc;
          v[c] = vc;
        }
        *reinterpret_cast<f32x4*>(t.p + i) = p;
        *reinterpret_cast<f32x4*>(t.m + i) = m;
        *reinterpret_cast<f32x4*>(t.v + i) = v;
        *reinterpret_cast<f32x4*>(t.g + i) = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      if (ema) {
        f32x4 e = *reinterpret_cast<const f32x4*>(t.ema + i);
        e = d * e + (1.f - d) * p;
        *reinterpret_cast<f32x4*>(t.ema + i) = e;
      }
    }
    i0 = off + 4 * nv;
  }
  const long tc = (long)t.taps * t.cin;
  for (long i = i0 + threadIdx.x; i < end; i += LY_THREADS) {
    float p = t.p[i];
    if (t.g) {
      // tap-major gradient storage ([cout][kh*kw][cin]) of a [cout][cin][kh*kw] weight: the index map of ly_optim_update_kernel;
      // the moments stay in the parameter's layout
      long gi = i;
      if (t.taps > 1) {
        const long co = i / tc, r = i - co * tc;
        const int c = (int)(r / t.taps), tp = (int)(r - (long)c * t.taps);
        gi = (co * t.taps + tp) * t.cin + c;
      }
      float m = t.m[i], v = t.v[i];
      p = ly_adam_elem(p, t.g[gi], m, v, k);
      t.m[i] = m;
      t.v[i] = v;
      t.p[i] = p;
      t.g[gi] = 0.f;
    }
    if (ema) t.ema[i] = d * t.ema[i] + (1.f - d) * p;
  }
}

// last launch of the step: EMA update count, Adam step counter and the norm accumulator for the next step (plain stores of one lane)
__global__ void ly_adam_finish_kernel(double* __restrict__ ws, float* __restrict__ hyper) {
  if (threadIdx.x == 0) { ws[0] = 0.0; hyper[9] += 1.f; hyper[11] += 1.f; }
}

extern "C" int ly_adam_step(const LyAdamTensor* table, const int* blk_tensor, const long* blk_off, int n_blocks, double* ws, float* hyper,
                            int decoupled, float* norm_out, void* stream) {
  LY_CHECK(table && blk_tensor && blk_off && ws && hyper && n_blocks > 0, "adam_step: bad arguments");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ly_adam_norm_kernel, dim3((unsigned)n_blocks), dim3(LY_THREADS), 0, st, table, blk_tensor, blk_off, ws);
  hipLaunchKernelGGL(ly_adam_update_kernel, dim3((unsigned)n_blocks), dim3(LY_THREADS), 0, st, table, blk_tensor, blk_off, ws, hyper,
                     decoupled, norm_out);
  hipLaunchKernelGGL(ly_adam_finish_kernel, dim3(1), dim3(64), 0, st, ws, hyper);
  LY_LAUNCH_CHECK();
  return 0;
}
