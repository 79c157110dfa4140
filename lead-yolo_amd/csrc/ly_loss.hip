// Detection loss of one pyramid level, forward AND gradient in three launches (reference utils/loss.py:121-268
// `ComputeLoss.__call__` / `build_targets`, utils/metrics.py:293-354 `bbox_iou(EIoU=True)`); any nc (class BCE with label smoothing and
// cls_pw when nc > 1, utils/loss.py:168-173), obj_pw; and the options of the reference's recipe: focal loss on both BCEs (fl_gamma > 0,
// utils/loss.py:36-61 FocalLoss, alpha 0.25), gr < 1, sort_obj_iou and autobalance — uniform branches on kernel arguments, the default
// path (gamma 0, gr 1, no sort, no device balance) keeps its instruction sequence and its bits.
//
// The reference runs ~150 tiny ops forward and ~250 backward per step here (anchor matching with boolean indexing — a
// host sync per level —, EIoU, two BCEs): 3.4 ms + 4.2 ms of pure launch latency at bs=64, a fifth of the training step.
//
//   ly_loss_match   one thread per CANDIDATE (offset k in 0..4, anchor a, target t), order index = k*na*nt + a*nt + t — exactly
//                   the order the reference's `t.repeat((5,1,1))[sel]` produces.  Valid candidates (anchor ratio test, offset
//                   rule) compute their cell, the target box, the predicted box and EIoU WITH its gradient (forward-mode dual
//                   numbers over the 4 box parameters), add (1 - eiou) and 1 to the level's accumulators, and enter the
//                   per-cell "last writer" election (atomicMax of the order index: the reference's `tobj[b,a,gj,gi] = iou`
//                   assigns sequentially on the CPU, so the highest order index wins; on CUDA the reference itself is unordered).
//   ly_loss_apply   per valid candidate: box gradient * box*bs/count into dpred (atomic: several candidates can share a cell),
//                   and the elected candidate writes tobj = max(iou, 0).
//   ly_loss_obj     per cell: BCE-with-logits against tobj, its gradient into dpred[..., 4], level sum by block reduction.
// ly_loss_finish combines the level accumulators into (loss, lbox, lobj, lcls) exactly as the reference does (mean per level,
// balance [4, 1, 0.4], * hyp gains, * batch size).
//
// Focal loss: FocalLoss(BCEWithLogitsLoss(pos_weight), gamma, alpha) per element, with s = sigmoid(x) and a SOFT target z (tobj in [0, 1],
// cp / cn):  u = 1 - p_t = z (1 - s) + (1 - z) s,  af = z alpha + (1 - z)(1 - alpha),  loss = bce * af * u^gamma,
//   d loss / dx = af * [ bce' * u^gamma - bce * gamma * u^(gamma - 1) * (2z - 1) * s (1 - s) ]      (the modulating factor's own derivative included,
// as the reference's autograd includes it).  1 - s is taken as sigmoid(-x), not as a float subtraction, so u keeps its relative precision for
// large |x| and reaches 0 only where exp(-|x|) underflows.  Where u == 0 the second term is taken as 0 — a deliberate difference: torch
// evaluates 0^(gamma - 1) * 0 = inf * 0 = NaN there for gamma < 1.
// gr < 1: the elected candidate writes tobj = (1 - gr) + gr * max(iou, 0).
// sort_obj_iou: the reference sorts the level's candidates by ascending iou before `tobj[b,a,gj,gi] = iou`, i.e. a cell keeps the MAXIMUM
// of its candidates' values (equal values tie invisibly): an integer atomicMax on the bit pattern of the non-negative float into the zeroed
// tobj — monotone because the values are >= 0 — replaces the last-writer election; no sort, no winner index.
// autobalance: the balance vector lives on the device as double[nl] (the reference's is a list of Python floats; its per-level .item() would
// be a host sync).  ly_loss_obj reads its level's entry for the gradient scale — the value BEFORE this call's update, as in the reference —
// and ly_loss_finish, after forming lobj with the old values, does balance[i] = balance[i] * 0.9999 + 0.0001 / obji and divides the vector
// by balance[ssi] (ssi = the stride-16 level).  obji == 0 divides by zero as in the reference: the Inf propagates.
//
// The three loss sums of a level are ORDER-INDEPENDENT: every term (a candidate's 1 - eiou and class BCE, a block's objectness partial — itself
// a fixed-order sum) is converted to 2^-30 fixed point on its own and added with a 64-bit INTEGER atomic, so two runs on the same inputs give the
// same bits whatever order the blocks arrive in (float atomics gave the last bit of lbox / lobj to the scheduler).  The count and the rejected
// rows are float sums of 1.0, exact below 2^24.  A term that is not finite, or is 2^20 or more, goes to a float slot as it is (a NaN or an Inf
// still reaches the loss); fixed point holds 2^33 / (term size) terms, far beyond any batch.
#include "ly_common.hpp"

#define LY_LOSS_ACC 16             // floats per level accumulator, 8-byte aligned: [0,1] [2,3] [4,5] int64 fixed-point sums of 1 - eiou, objectness
                                   // BCE, class BCE; [6] matches; [7] rejected target rows; [8] [9] [10] the same three sums' terms that fixed
                                   // point does not take (non-finite or >= 2^20), as floats; the rest unused
enum { LY_LOSS_BOX = 0, LY_LOSS_OBJ = 1, LY_LOSS_CLS = 2, LY_LOSS_COUNT = 6, LY_LOSS_BAD = 7, LY_LOSS_WILD = 8 };
#define LY_LOSS_FIX 1073741824.0   // 2^30

__device__ __forceinline__ void ly_loss_add(float* acc, int which, float v) {
  if (fabsf(v) < 1048576.f)        // false for a NaN
    atomicAdd(reinterpret_cast<unsigned long long*>(acc) + which, (unsigned long long)(long long)((double)v * LY_LOSS_FIX));
  else
    atomicAdd(acc + LY_LOSS_WILD + which, v);
}
__device__ __forceinline__ float ly_loss_sum(const float* acc, int which) {
  return (float)((double)reinterpret_cast<const long long*>(acc)[which] * (1.0 / LY_LOSS_FIX)) + acc[LY_LOSS_WILD + which];
}

struct D4 {                        // value + derivatives w.r.t. (px, py, pw, ph)
  float v, d[4];
};
__device__ __forceinline__ D4 d4c(float v) { return D4{v, {0.f, 0.f, 0.f, 0.f}}; }
__device__ __forceinline__ D4 d4v(float v, int i) { D4 r = d4c(v); r.d[i] = 1.f; return r; }
__device__ __forceinline__ D4 operator+(D4 a, D4 b) { D4 r; r.v = a.v + b.v; for (int i = 0; i < 4; ++i) r.d[i] = a.d[i] + b.d[i]; return r; }
__device__ __forceinline__ D4 operator-(D4 a, D4 b) { D4 r; r.v = a.v - b.v; for (int i = 0; i < 4; ++i) r.d[i] = a.d[i] - b.d[i]; return r; }
__device__ __forceinline__ D4 operator*(D4 a, D4 b) { D4 r; r.v = a.v * b.v; for (int i = 0; i < 4; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i]; return r; }
__device__ __forceinline__ D4 operator/(D4 a, D4 b) {
  D4 r; const float ib = 1.f / b.v; r.v = a.v * ib;
  for (int i = 0; i < 4; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) * ib;
  return r;
}
__device__ __forceinline__ D4 operator*(D4 a, float s) { D4 r; r.v = a.v * s; for (int i = 0; i < 4; ++i) r.d[i] = a.d[i] * s; return r; }
__device__ __forceinline__ D4 operator+(D4 a, float s) { a.v += s; return a; }
__device__ __forceinline__ D4 d4min(D4 a, float b) { return a.v <= b ? a : d4c(b); }       // torch.minimum: gradient to the smaller (ties: first)
__device__ __forceinline__ D4 d4max(D4 a, float b) { return a.v >= b ? a : d4c(b); }
__device__ __forceinline__ D4 d4clamp0(D4 a) { return a.v > 0.f ? a : d4c(0.f); }         // clamp(0): zero gradient at and below 0

// EIoU of the predicted box (px, py, pw, ph: dual) against the target box, as bbox_eiou in loss.py (reference metrics.py:293-354)
__device__ __forceinline__ D4 ly_eiou(D4 px, D4 py, D4 pw, D4 ph, float tx, float ty, float tw, float th) {
  const float eps = 1e-7f;
  const D4 ax1 = px - pw * 0.5f, ax2 = px + pw * 0.5f, ay1 = py - ph * 0.5f, ay2 = py + ph * 0.5f;
  const float bx1 = tx - tw * 0.5f, bx2 = tx + tw * 0.5f, by1 = ty - th * 0.5f, by2 = ty + th * 0.5f;
  const D4 iw = d4clamp0(d4min(ax2, bx2) - d4max(ax1, bx1)), ih = d4clamp0(d4min(ay2, by2) - d4max(ay1, by1));
  const D4 inter = iw * ih;
  const D4 uni = pw * ph + (tw * th) - inter + eps;
  const D4 iou = inter / (uni + eps);
  const D4 cw = d4max(ax2, bx2) - d4min(ax1, bx1), ch = d4max(ay2, by2) - d4min(ay1, by1);
  const D4 c2 = cw * cw + ch * ch + eps;
  const D4 sx = d4c(bx1 + bx2) - ax1 - ax2, sy = d4c(by1 + by2) - ay1 - ay2;
  const D4 rho2 = (sx * sx + sy * sy) * 0.25f;
  const D4 dw = d4c(bx2 - bx1) - (ax2 - ax1), dh = d4c(by2 - by1) - (ay2 - ay1);
  return iou - (rho2 / c2 + (dw * dw) / (cw * cw + eps) + (dh * dh) / (ch * ch + eps));
}

struct LyLossLevel {
  const float* p;        // [bs][na][ny][nx][no]
  float* dp;             // same shape, zeroed by the caller
  const float* anchors;  // [na][2], grid units
  const float* targets;  // [nt][6]: image, class, x, y, w, h (normalised)
  int bs, na, ny, nx, no;
  long nt;
  float anchor_t;
  // workspaces (per level)
  float* tobj;           // [cells], zeroed
  int* winner;           // [cells], filled with -1
  long* cand_cell;       // [5*na*nt], -1 = invalid
  float* cand;           // [5*na*nt][5]: iou, d(1-eiou)/d(raw0..3)
  float* acc;            // [LY_LOSS_ACC], zeroed, 8-byte aligned: see LY_LOSS_ACC
  float* tbox;           // optional [5*na*nt][4]: (gx - gi, gy - gj, gw, gh) of every valid candidate (build_targets' tbox)
  float cp, cn, cls_pw, obj_pw;      // class targets (label smoothing: 1 - eps/2, eps/2), positive weights of the two BCEs
  float gamma, alpha;    // focal loss on both BCEs when gamma > 0 (alpha: weight of the positive side)
  float gr;              // tobj = (1 - gr) + gr * max(iou, 0) when gr < 1
  int sort;              // sort_obj_iou: a cell keeps the maximum of its candidates instead of the last writer's value
};

// BCE-with-logits with a positive weight (torch.nn.BCEWithLogitsLoss(pos_weight = pw)): value and d/dx
__device__ __forceinline__ float ly_bce(float x, float z, float pw) {
  const float sp = log1pf(__expf(-fabsf(x))) + fmaxf(-x, 0.f);         // softplus(-x) = -log sigmoid(x)
  return (1.f - z) * x + (1.f + (pw - 1.f) * z) * sp;
}
__device__ __forceinline__ float ly_bce_grad(float x, float z, float pw) {
  const float sg = ly_sigmoid(x);
  return (1.f - z) * sg - pw * z * (1.f - sg);
}

// FocalLoss(BCEWithLogitsLoss(pos_weight = pw), gamma, alpha) of one element: value, and d/dx into *grad (see the head of the file)
__device__ __forceinline__ float ly_focal(float x, float z, float pw, float gamma, float alpha, float* grad) {
  const float e = __expf(-fabsf(x)), r = 1.f / (1.f + e);
  const float big = r, small = e * r;                                    // sigmoid(|x|), sigmoid(-|x|): neither is a difference from 1
  const float s = x >= 0.f ? big : small, sn = x >= 0.f ? small : big;   // s = sigmoid(x), sn = 1 - s
  const float sp = log1pf(e) + fmaxf(-x, 0.f);
  const float bce = (1.f - z) * x + (1.f + (pw - 1.f) * z) * sp;
  const float dbce = (1.f - z) * s - pw * z * sn;
  const float u = z * sn + (1.f - z) * s;
  const float af = z * alpha + (1.f - z) * (1.f - alpha);
  const float m = powf(u, gamma);
  const float dm = u > 0.f ? gamma * (m / u) * (1.f - 2.f * z) * (s * sn) : 0.f;     // u == 0: the term is taken as 0 (torch: inf * 0)
  *grad = af * (dbce * m + bce * dm);
  return bce * af * m;
}

__global__ __launch_bounds__(LY_THREADS) void ly_loss_match_kernel(const LyLossLevel L) {
  const long ncand = 5L * L.na * L.nt;
  const long idx = (long)blockIdx.x * LY_THREADS + threadIdx.x;
  if (idx >= ncand) return;
  const int k = (int)(idx / ((long)L.na * L.nt));
  const long rem = idx - (long)k * L.na * L.nt;
  const int a = (int)(rem / L.nt);
  const long t = rem - (long)a * L.nt;
  const float* tg = L.targets + t * 6;
  const float gx = __fmul_rn(tg[2], (float)L.nx), gy = __fmul_rn(tg[3], (float)L.ny), gw = __fmul_rn(tg[4], (float)L.nx), gh = __fmul_rn(tg[5], (float)L.ny);
  const float aw = L.anchors[2 * a], ah = L.anchors[2 * a + 1];
  const float rw = gw / aw, rh = gh / ah;
  // A target row whose image index is outside [0, bs) (a last partial batch, per-rank slices that kept global indices) or that
  // holds a NaN would index p / dp / winner out of bounds; the torch formulation raises IndexError there.  Such rows are
  // rejected and counted: ly_loss_finish turns a non-zero count into a NaN loss (loud, and without a host sync).
  const int b = (int)tg[0];
  const bool padding = tg[0] == -1.f;                     // a row with image index exactly -1 is PADDING (fixed-shape target
                                                          // buffers of a captured step): ignored silently
  // nc > 1: the class column selects the positive class.  The reference's `t[range(n), tcls[i]] = cp` raises for an index >= nc; a negative
  // index -k wraps there to class nc - k (torch indexing) — a deliberate difference: a negative class is a corrupt label here, not a way
  // to count classes from the end.  A class whose truncation (.long()) is outside [0, nc), or a NaN, would train every class of the row as
  // a negative (NaN: class 0 as the positive): such a row is rejected and counted like a bad image index.  nc = 1 never reads the column.
  const float cf = tg[1];
  const bool cls_ok = L.no - 5 <= 1 || (cf > -1.f && cf < (float)(L.no - 5));
  const bool sane = tg[0] >= 0.f && b < L.bs && gx == gx && gy == gy && gw == gw && gh == gh && cls_ok;
  if (!sane && !padding && k == 0 && a == 0) atomicAdd(L.acc + LY_LOSS_BAD, 1.f);
  bool ok = sane && fmaxf(fmaxf(rw, 1.f / rw), fmaxf(rh, 1.f / rh)) < L.anchor_t;
  const float g = 0.5f;
  float ox = 0.f, oy = 0.f;
  if (k == 1) { ok = ok && (fmodf(gx, 1.f) < g && gx > 1.f); ox = g; }
  else if (k == 2) { ok = ok && (fmodf(gy, 1.f) < g && gy > 1.f); oy = g; }
  else if (k == 3) { const float ix = L.nx - gx; ok = ok && (fmodf(ix, 1.f) < g && ix > 1.f); ox = -g; }
  else if (k == 4) { const float iy = L.ny - gy; ok = ok && (fmodf(iy, 1.f) < g && iy > 1.f); oy = -g; }
  long cell = -1;
  if (ok) {
    const int gi_raw = (int)(gx - ox), gj_raw = (int)(gy - oy);           // .long(): truncation
    const int gi = gi_raw < 0 ? 0 : gi_raw > L.nx - 1 ? L.nx - 1 : gi_raw;
    const int gj = gj_raw < 0 ? 0 : gj_raw > L.ny - 1 ? L.ny - 1 : gj_raw;
    cell = (((long)b * L.na + a) * L.ny + gj) * L.nx + gi;
    const float tx = __fsub_rn(gx, (float)gi_raw), ty = __fsub_rn(gy, (float)gj_raw);   // tbox uses the UNclamped cell; no FMA contraction with gx = x*nx (bit-exact vs torch)
    if (L.tbox) { float* tb = L.tbox + idx * 4; tb[0] = tx; tb[1] = ty; tb[2] = gw; tb[3] = gh; }
    const float* pr = L.p + cell * L.no;
    const float s0 = ly_sigmoid(pr[0]), s1 = ly_sigmoid(pr[1]), s2 = ly_sigmoid(pr[2]), s3 = ly_sigmoid(pr[3]);
    const float pxv = s0 * 2.f - 0.5f, pyv = s1 * 2.f - 0.5f, pwv = (s2 * 2.f) * (s2 * 2.f) * aw, phv = (s3 * 2.f) * (s3 * 2.f) * ah;
    const D4 e = ly_eiou(d4v(pxv, 0), d4v(pyv, 1), d4v(pwv, 2), d4v(phv, 3), tx, ty, gw, gh);
    float* c = L.cand + idx * 5;
    c[0] = e.v;                                                            // (the reference's `iou` here is the EIoU value)
    // d(1 - eiou)/d raw = -d eiou/d box * d box/d raw
    c[1] = -e.d[0] * 2.f * s0 * (1.f - s0);
    c[2] = -e.d[1] * 2.f * s1 * (1.f - s1);
    c[3] = -e.d[2] * 8.f * s2 * s2 * (1.f - s2) * aw;
    c[4] = -e.d[3] * 8.f * s3 * s3 * (1.f - s3) * ah;
    ly_loss_add(L.acc, LY_LOSS_BOX, 1.f - e.v);
    atomicAdd(L.acc + LY_LOSS_COUNT, 1.f);
    atomicMax(L.winner + cell, (int)idx);
    const int nc = L.no - 5;
    if (nc > 1) {                                                          // class BCE of this matched row (utils/loss.py:168-173)
      const int cls = (int)tg[1];
      float sc = 0.f;
      if (L.gamma > 0.f) {
        float unused;
        for (int q = 0; q < nc; ++q) sc += ly_focal(pr[5 + q], q == cls ? L.cp : L.cn, L.cls_pw, L.gamma, L.alpha, &unused);
      } else {
        for (int q = 0; q < nc; ++q) sc += ly_bce(pr[5 + q], q == cls ? L.cp : L.cn, L.cls_pw);
      }
      ly_loss_add(L.acc, LY_LOSS_CLS, sc);
    }
  }
  L.cand_cell[idx] = cell;
}

__global__ __launch_bounds__(LY_THREADS) void ly_loss_apply_kernel(const LyLossLevel L, float box_gain, float cls_gain) {
  const long ncand = 5L * L.na * L.nt;
  const long idx = (long)blockIdx.x * LY_THREADS + threadIdx.x;
  if (idx >= ncand) return;
  const long cell = L.cand_cell[idx];
  if (cell < 0) return;
  const float* c = L.cand + idx * 5;
  const float scale = box_gain * (float)L.bs / L.acc[LY_LOSS_COUNT];                   // d/d(1-eiou) of  box * mean(1-eiou) * bs
  float* d = L.dp + cell * L.no;
#pragma unroll
  for (int r = 0; r < 4; ++r) atomicAdd(d + r, scale * c[1 + r]);
  if (L.sort) {                                                            // sort_obj_iou: the cell's maximum (values >= 0: monotone as integers)
    float v = fmaxf(c[0], 0.f);
    if (L.gr < 1.f) v = (1.f - L.gr) + L.gr * v;
    atomicMax(reinterpret_cast<int*>(L.tobj + cell), __float_as_int(v));
  } else if (L.winner[cell] == (int)idx) {
    if (L.gr < 1.f) L.tobj[cell] = (1.f - L.gr) + L.gr * fmaxf(c[0], 0.f);
    else L.tobj[cell] = fmaxf(c[0], 0.f);
  }
  const int nc = L.no - 5;
  if (nc > 1) {                                                            // d/dx of  cls * mean over (rows, classes) of BCE * bs
    const long t = idx % L.nt;
    const int cls = (int)L.targets[t * 6 + 1];
    const float cs = cls_gain * (float)L.bs / (L.acc[LY_LOSS_COUNT] * (float)nc);
    const float* pr = L.p + cell * L.no;
    if (L.gamma > 0.f) {
      for (int q = 0; q < nc; ++q) {
        float gq;
        ly_focal(pr[5 + q], q == cls ? L.cp : L.cn, L.cls_pw, L.gamma, L.alpha, &gq);
        atomicAdd(d + 5 + q, cs * gq);
      }
    } else {
      for (int q = 0; q < nc; ++q) atomicAdd(d + 5 + q, cs * ly_bce_grad(pr[5 + q], q == cls ? L.cp : L.cn, L.cls_pw));
    }
  }
}

// balance_dev == NULL: obj_scale by value (host balance); else the level's entry of the device balance vector (autobalance), read before
// ly_loss_finish updates it
__global__ __launch_bounds__(LY_THREADS) void ly_loss_obj_kernel(const LyLossLevel L, float obj_scale, float obj_gain, const double* __restrict__ balance_dev,
                                                                 int level) {
  __shared__ float red[4];
  const long cells = (long)L.bs * L.na * L.ny * L.nx;
  if (balance_dev) obj_scale = obj_gain * (float)balance_dev[level] * (float)L.bs / (float)cells;
  float s = 0.f;
  if (L.gamma > 0.f) {
    for (long i = (long)blockIdx.x * LY_THREADS + threadIdx.x; i < cells; i += (long)gridDim.x * LY_THREADS) {
      float g;
      s += ly_focal(L.p[i * L.no + 4], L.tobj[i], L.obj_pw, L.gamma, L.alpha, &g);
      L.dp[i * L.no + 4] = g * obj_scale;
    }
  } else {
    for (long i = (long)blockIdx.x * LY_THREADS + threadIdx.x; i < cells; i += (long)gridDim.x * LY_THREADS) {
      const float x = L.p[i * L.no + 4], z = L.tobj[i];
      s += ly_bce(x, z, L.obj_pw);
      L.dp[i * L.no + 4] = ly_bce_grad(x, z, L.obj_pw) * obj_scale;          // obj_scale = obj * balance * bs / cells
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) ly_loss_add(L.acc, LY_LOSS_OBJ, red[0] + red[1] + red[2] + red[3]);
}

extern "C" int ly_loss_level_opts(const float* p, float* dp, const float* anchors, const float* targets, int bs, int na, int ny, int nx, int no, long nt,
                                  float anchor_t, float box_gain, float obj_gain, float balance, float* tobj, int* winner, long* cand_cell, float* cand,
                                  float* acc, float* tbox, int match_only, float cls_gain, float cp, float cn, float cls_pw, float obj_pw,
                                  float fl_gamma, float fl_alpha, float gr, int sort_obj_iou, const double* balance_dev, int level, void* stream) {
  LY_CHECK(fl_gamma >= 0.f && fl_alpha >= 0.f && fl_alpha <= 1.f && gr >= 0.f && gr <= 1.f, "loss_level: fl_gamma >= 0, fl_alpha and gr in [0, 1]");
  LY_CHECK(!balance_dev || (level >= 0 && ((uintptr_t)balance_dev & 7) == 0), "loss_level: device balance needs its level index and 8-byte alignment");
  LY_CHECK(((uintptr_t)acc & 7) == 0, "loss_level: acc must be 8-byte aligned (64-bit integer atomics)");
  LY_CHECK(p && (dp || match_only) && anchors && tobj && winner && acc && (nt == 0 || (targets && cand_cell && cand)), "loss_level: null pointer");
  LY_CHECK(bs > 0 && na > 0 && ny > 0 && nx > 0 && no >= 5 && nt >= 0, "loss_level: bad sizes");
  const long cells = (long)bs * na * ny * nx;
  LY_CHECK(5L * na * nt < (1L << 31) && cells < (1L << 40), "loss_level: too many candidates");
  LyLossLevel L{p, dp, anchors, targets, bs, na, ny, nx, no, nt, anchor_t, tobj, winner, cand_cell, cand, acc, tbox, cp, cn, cls_pw, obj_pw, fl_gamma, fl_alpha, gr, sort_obj_iou != 0};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long ncand = 5L * na * nt;
  if (ncand > 0) {
    const unsigned blocks = (unsigned)((ncand + LY_THREADS - 1) / LY_THREADS);
    hipLaunchKernelGGL(ly_loss_match_kernel, dim3(blocks), dim3(LY_THREADS), 0, st, L);
    if (!match_only) hipLaunchKernelGGL(ly_loss_apply_kernel, dim3(blocks), dim3(LY_THREADS), 0, st, L, box_gain, cls_gain);
  }
  if (match_only) {            // target assignment only (ComputeLoss.build_targets): cand_cell / tbox are the result
    LY_LAUNCH_CHECK();
    return 0;
  }
  long ob = (cells + LY_THREADS * 8L - 1) / (LY_THREADS * 8L);
  ob = ob < 1 ? 1 : ob > 2048 ? 2048 : ob;
  hipLaunchKernelGGL(ly_loss_obj_kernel, dim3((unsigned)ob), dim3(LY_THREADS), 0, st, L, obj_gain * balance * (float)bs / (float)cells, obj_gain,
                     balance_dev, level);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_loss_level(const float* p, float* dp, const float* anchors, const float* targets, int bs, int na, int ny, int nx, int no, long nt,
                             float anchor_t, float box_gain, float obj_gain, float balance, float* tobj, int* winner, long* cand_cell, float* cand,
                             float* acc, float* tbox, int match_only, float cls_gain, float cp, float cn, float cls_pw, float obj_pw, void* stream) {
  return ly_loss_level_opts(p, dp, anchors, targets, bs, na, ny, nx, no, nt, anchor_t, box_gain, obj_gain, balance, tobj, winner, cand_cell, cand, acc,
                            tbox, match_only, cls_gain, cp, cn, cls_pw, obj_pw, 0.f, 0.25f, 1.f, 0, nullptr, 0, stream);
}

// out[0] = total loss, out[1..3] = (lbox, lobj, lcls) as the reference returns them; acc = [nl][LY_LOSS_ACC] level accumulators.
// balance_dev != NULL (autobalance): lobj with the device vector's present values, then its update and normalisation in place
__global__ void ly_loss_finish_kernel(const float* __restrict__ acc, int nl, const float* __restrict__ cells, const float* __restrict__ balance,
                                      float box_gain, float obj_gain, float cls_gain, int nc, float bs, float* __restrict__ out,
                                      double* __restrict__ balance_dev, int ssi) {
  if (threadIdx.x != 0) return;
  float lbox = 0.f, lobj = 0.f, lcls = 0.f, bad = 0.f;
  for (int i = 0; i < nl; ++i) {
    const float* a = acc + LY_LOSS_ACC * i;
    const float count = a[LY_LOSS_COUNT];
    bad += a[LY_LOSS_BAD];
    if (count > 0.f) {
      lbox += ly_loss_sum(a, LY_LOSS_BOX) / count;
      if (nc > 1) lcls += ly_loss_sum(a, LY_LOSS_CLS) / (count * (float)nc);
    }
    if (balance_dev) {
      lobj += ly_loss_sum(a, LY_LOSS_OBJ) / cells[i] * (float)balance_dev[i];
      const double obji = ((double)reinterpret_cast<const long long*>(a)[LY_LOSS_OBJ] * (1.0 / LY_LOSS_FIX) + (double)a[LY_LOSS_WILD + LY_LOSS_OBJ]) / (double)cells[i];
      balance_dev[i] = balance_dev[i] * 0.9999 + 0.0001 / obji;              // utils/loss.py:178
    } else {
      lobj += ly_loss_sum(a, LY_LOSS_OBJ) / cells[i] * balance[i];
    }
  }
  if (balance_dev) {                                                         // utils/loss.py:180-181
    const double d = balance_dev[ssi];
    for (int i = 0; i < nl; ++i) balance_dev[i] /= d;
  }
  lbox *= box_gain;
  lobj *= obj_gain;
  lcls *= cls_gain;
  out[0] = bad > 0.f ? __builtin_nanf("") : (lbox + lobj + lcls) * bs;      // rejected target rows (image index outside the batch / NaN): fail loudly
  out[1] = lbox;
  out[2] = lobj;
  out[3] = lcls;
}

extern "C" int ly_loss_finish_opts(const float* acc, int nl, const float* cells, const float* balance, float box_gain, float obj_gain, float cls_gain,
                                   int nc, int bs, float* out, double* balance_dev, int ssi, void* stream) {
  LY_CHECK(acc && cells && (balance || balance_dev) && out && nl > 0, "loss_finish: bad arguments");
  LY_CHECK(!balance_dev || (ssi >= 0 && ssi < nl && ((uintptr_t)balance_dev & 7) == 0), "loss_finish: device balance needs ssi in [0, nl) and 8-byte alignment");
  hipLaunchKernelGGL(ly_loss_finish_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), acc, nl, cells, balance, box_gain, obj_gain,
                     cls_gain, nc, (float)bs, out, balance_dev, ssi);
  LY_LAUNCH_CHECK();
  return 0;
}

extern "C" int ly_loss_finish(const float* acc, int nl, const float* cells, const float* balance, float box_gain, float obj_gain, float cls_gain,
                              int nc, int bs, float* out, void* stream) {
  LY_CHECK(balance, "loss_finish: bad arguments");
  return ly_loss_finish_opts(acc, nl, cells, balance, box_gain, obj_gain, cls_gain, nc, bs, out, nullptr, 0, stream);
}
