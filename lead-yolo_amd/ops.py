"""Thin host wrappers over the C-ABI (capi.py): torch supplies device memory and the current stream,
every arithmetic step is a HIP kernel in libleadyolo_hip.so.  Activations are logical NCHW tensors
with channels_last (NHWC) storage; a channel slice of such a tensor (a slot of a concat buffer) is
addressed as rows of stride `ld` without copying.

Storage dtype: every wrapper takes it from its activation argument — float32 (bf16x3 products) or bfloat16 (plain bf16
products, BASELINE configs[2]-[4]); outputs have the input's dtype, statistics / attention tables / weight gradients
are float32.  `edge_in` is the dtype policy at a module's edge (autocast, .half())."""
import ctypes
import os

import torch

from . import capi
from .capi import (ACT_NONE, ACT_RELU, ACT_SILU, GATHER_PATCH, GATHER_PATCH_NCHW, GATHER_PATCH_NCHW_BF16, GATHER_PATCH_NCHW_F16, GATHER_PATCH_NCHW_U8, GATHER_ROWS, GATHER_UP2,  # noqa: F401
                   PRO_AFFINE_RELU_CA, PRO_GATE, PRO_NONE)


# ---- optional per-launch timing (bench.py / tools): PROFILE = [] turns it on -----------------------
PROFILE = None


class _Timed:
    """Brackets one C-ABI call with events on the launch stream and records (kernel name as rocprofv3
    prints it, algorithmic MFMA flops, algorithmic bytes, algorithmic VALU flops).  `flops` = 2*MAC of the contractions that run on
    the matrix cores; `valu_flops` = 2*MAC of work that is vector arithmetic by construction (the RFCBAM `generate` regeneration:
    81 MAC per (output pixel, channel) and pass; the two are priced against different peaks)."""

    def __init__(self, name, flops, nbytes, valu_flops=0.0):
        self.rec = None
        if PROFILE is not None:
            self.rec = [name, float(flops), float(nbytes), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), float(valu_flops)]

    def __enter__(self):
        if self.rec is not None:
            self.rec[3].record()

    def __exit__(self, *a):
        if self.rec is not None:
            self.rec[4].record()
            PROFILE.append(self.rec)


def _label(describe, *args):
    """the `_Timed` name of a C-ABI call whose kernel the library picks: what the entry's describe twin (include/lead_yolo_hip.h) says it
    would launch for these arguments, as rocprofv3 prints it.  Asked only while a profile is recorded; a refused call is reported by the
    launch itself, and where there is no name (a refusal, ly_mlpblock_pconv's "not built" code) the record carries the entry's."""
    if PROFILE is None:
        return None
    name = ctypes.create_string_buffer(160)
    rc = getattr(capi.lib(), describe)(*args, name, len(name))
    return name.value.decode() if rc >= 0 and name.value else describe[:-len("_describe")]


_CONV_TILE_CACHE = {}


def pick_conv_tile(h, w, max_px=128, max_frame=192):
    """TH x TW patch (<= 128 pixels, frame (TH+2)(TW+2) <= 192) covering an h x w map with the fewest
    MFMA pixel tiles, ties broken by the smaller halo frame."""
    key = (h, w)
    if key not in _CONV_TILE_CACHE:
        best = None
        for tw in range(1, min(w, max_px) + 1):
            for th in range(1, min(h, max_px // tw) + 1):
                if (th + 2) * (tw + 2) > max_frame:
                    continue
                blocks = -(-h // th) * -(-w // tw)
                work = blocks * (-(-(th * tw) // 16))               # MFMA pixel tiles issued
                halo = blocks * (th + 2) * (tw + 2)                 # frame positions staged
                score = (work * 16 + 0.35 * halo, blocks)
                if best is None or score < best[0]:
                    best = (score, th, tw)
        _CONV_TILE_CACHE[key] = (best[1], best[2])
    return _CONV_TILE_CACHE[key]


MLP_WIDTHS = (16, 24, 40, 80, 160, 320)     # C values ly_mlpblock_fwd is instantiated for (include/lead_yolo_hip.h)


def require_cuda(x, who, mod=None):
    if mod is not None and not mod.training and torch.is_grad_enabled() and x.requires_grad:
        raise NotImplementedError(f"{who}: backward is built for train mode (batch-statistics BatchNorm); an eval-mode module would return "
                                  "tensors detached from autograd — call .train(), or run inference under torch.no_grad()")
    if not x.is_cuda:
        raise RuntimeError(f"{who}: the HIP path needs a CUDA/ROCm tensor (got {x.device}); there is no CPU fallback")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError(f"{who}: activations must be float32 or bfloat16 here (got {x.dtype}); float16 is converted at the "
                                  "module edge (ops.edge_in)")


def edge_in(x, who, mod=None):
    """Dtype policy at a module's edge (SURVEY §8b call contract: fp32, or fp16 under `autocast` / `.half()`, train.py:229,316).
      * under torch.autocast('cuda', dtype) a float32 input is cast to the autocast dtype, as autocast does for convolutions;
      * bfloat16 runs the bf16 kernels; float32 (outside autocast) the fp32-storage kernels;
      * float16 (the reference's AMP dtype) has no kernels of its own: it is computed as bfloat16 (same 16-bit storage, wider
        exponent, fp32 accumulation) and the module's output is cast back to float16, so neighbours still see fp16.
    Returns (tensor to compute on, dtype to cast the output back to or None)."""
    if not isinstance(x, torch.Tensor):
        return x, None
    if not x.is_cuda:
        raise RuntimeError(f"{who}: the HIP path needs a CUDA/ROCm tensor (got {x.device}); there is no CPU fallback")
    want = x.dtype
    if torch.is_autocast_enabled("cuda") and x.dtype == torch.float32:
        want = torch.get_autocast_dtype("cuda")
    if want not in (torch.float32, torch.bfloat16, torch.float16):
        raise NotImplementedError(f"{who}: unsupported activation dtype {x.dtype}")
    compute = torch.bfloat16 if want == torch.float16 else want
    back = torch.float16 if (want == torch.float16 and x.dtype != torch.bfloat16) else None
    if x.dtype != compute:
        x = x.to(compute)
    require_cuda(x, who, mod)
    return x, back


def edge_out(y, back):
    if back is None:
        return y
    if isinstance(y, torch.Tensor):
        return y.to(back)
    if isinstance(y, (list, tuple)):
        return type(y)(edge_out(t, back) for t in y)
    return y


def planes_of(t):
    """operand planes of the weight packs a kernel call on tensor / dtype `t` needs: 2 (bf16x3, fp32 storage) or 1 (bf16 storage)"""
    d = t if isinstance(t, torch.dtype) else t.dtype
    return 1 if d == torch.bfloat16 else 2


def vw_of(t):
    """elements of one 16-byte vector: channel counts / leading dimensions of contraction sources must be multiples of it"""
    d = t if isinstance(t, torch.dtype) else t.dtype
    return 8 if d == torch.bfloat16 else 4


def nhwc(x):
    return x.contiguous(memory_format=torch.channels_last)


def empty_nhwc(n, c, h, w, like, dtype=None):
    return torch.empty((n, c, h, w), dtype=dtype or like.dtype, device=like.device, memory_format=torch.channels_last)


def rows(x):
    """(tensor, ld): x as an [n*h*w, c] row matrix with row stride ld floats, zero-copy when x is a
    channels_last tensor or a channel slice of one; otherwise a channels_last copy is made."""
    n, c, h, w = x.shape
    if x.is_contiguous(memory_format=torch.channels_last) and x.stride(1) == 1:
        return x, c
    sn, sc, sh, sw = x.stride()
    if sc == 1 and sw >= c and sw % vw_of(x) == 0 and (h == 1 or sh == w * sw) and (n == 1 or sn == h * w * sw) and w > 1 \
            and x.data_ptr() % 16 == 0:
        return x, sw
    return rows_dense(x), c


def rows_dense(x):
    """NHWC-dense view of a logical [n, c, h, w] tensor (copy only if needed)."""
    x = nhwc(x)
    if x.stride(1) != 1:        # degenerate shapes where torch reports ambiguous strides
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return x


_p = capi.ptr


def gemm(*, M, H, W, K, N, a0, lda0, k0, wp, out, ldo, a1=None, lda1=0, gather=GATHER_ROWS, Hin=0, Win=0, Cin=0, ks=0, pk=0,
         pro=PRO_NONE, g_h=None, g_w=None, res=None, ldres=0, p_scale=None, p_shift=None, p_ca=None, e_scale=None,
         e_shift=None, rowscale=None, act=ACT_NONE, stats=None, dtype=None, scat_ks=0, scat_c=0, eadd=None, ldeadd=0):
    # element type of the call: the output's (statistics passes: the source's); the NCHW image gather always READS fp32 — or uint8
    # (pixel / 255 on load: the training loop's `imgs.float() / 255` folded into the gather)
    # or a 16-bit image as it is (the `im.half()` batch of a reduced-precision forward; LY_BF16 calls)
    if gather == GATHER_PATCH_NCHW:
        gather = {torch.uint8: GATHER_PATCH_NCHW_U8, torch.bfloat16: GATHER_PATCH_NCHW_BF16, torch.float16: GATHER_PATCH_NCHW_F16}.get(a0.dtype, gather)
    image = gather in (GATHER_PATCH_NCHW, GATHER_PATCH_NCHW_U8, GATHER_PATCH_NCHW_BF16, GATHER_PATCH_NCHW_F16)
    dt = (out if out is not None else a0).dtype if not image or out is not None else torch.float32
    if dtype is not None:
        dt = dtype
    code = capi.dtype_code(dt)
    P = capi.LyGemmParams(M, H, W, K, N, _p(a0), lda0, k0, _p(a1), lda1, gather, Hin, Win, Cin, ks, pk, pro, _p(g_h), _p(g_w),
                          _p(res), ldres, _p(p_scale), _p(p_shift), _p(p_ca), _p(wp), _p(e_scale), _p(e_shift), _p(rowscale),
                          act, _p(out), ldo, _p(stats), code, scat_ks, scat_c, _p(eadd), ldeadd)
    if eadd is not None and eadd.dtype != out.dtype:
        raise ValueError("gemm: eadd must have the output's dtype")
    es_i = 1 if gather == GATHER_PATCH_NCHW_U8 else 2 if gather in (GATHER_PATCH_NCHW_BF16, GATHER_PATCH_NCHW_F16) else 4 if (code == 0 or image) else 2
    es_o = 4 if code == 0 else 2
    with _Timed(_label("ly_gemm_describe", ctypes.byref(P)), 2.0 * M * K * N, es_i * M * K + (es_o * M * N if out is not None else 0) + 4.0 * N * K):
        capi.check(capi.lib().ly_gemm_fwd(ctypes.byref(P), capi.stream_ptr()), "ly_gemm_fwd")


def mlpblock_pconv(x, z, n, h, w, c, wp):
    """z = [conv3x3(x[:, :c/4]; wp) | x[:, c/4:]] in one pass (persistent MLPBlock kernel, partial conv only); x, z dense NHWC [n, c, h, w].
    Returns False when the kernel is not built for this shape (the caller then copies and calls conv3x3)."""
    with _Timed(_label("ly_mlpblock_pconv_describe", n, h, w, c, capi.dtype_code(x)), 18.0 * n * h * w * (c // 4) ** 2, 2.0 * x.element_size() * n * h * w * c):
        rc = capi.lib().ly_mlpblock_pconv(_p(x), _p(z), n, h, w, c, _p(wp), capi.dtype_code(x), capi.stream_ptr())
    if rc < 0:
        capi.check(rc, "ly_mlpblock_pconv")
    return rc == 0


def conv3x3(*, M, H, W, Cin, N, x, ldx, wp, out, ldo, e_scale=None, e_shift=None, act=ACT_NONE, stats=None):
    th, tw = pick_conv_tile(H, W)
    code = capi.dtype_code(x)
    P = capi.LyConv3Params(M, H, W, Cin, N, th, tw, _p(x), ldx, _p(wp), _p(e_scale), _p(e_shift), act, _p(out), ldo, _p(stats), code)
    with _Timed(_label("ly_conv3x3_describe", ctypes.byref(P)), 2.0 * M * 9 * Cin * N, x.element_size() * M * (Cin + N) + 4.0 * 9 * Cin * N):
        capi.check(capi.lib().ly_conv3x3_fwd(ctypes.byref(P), capi.stream_ptr()), "ly_conv3x3_fwd")


class Lazy:
    """A not-yet-materialised activation a consumer GEMM can absorb: channel concat of up to two row
    sources, the first optionally at half resolution (nearest 2x upsample) or gated by CoordAtt."""

    def __init__(self, shape, a0, lda0, k0, a1=None, lda1=0, up=False, gate=None, keep=()):
        self.shape = shape          # logical (n, c, h, w)
        self.a0, self.lda0, self.k0 = a0, lda0, k0
        self.a1, self.lda1 = a1, lda1
        self.up = up
        self.gate = gate            # (a_h, a_w) or None
        self.keep = keep            # tensors kept alive

    @staticmethod
    def of(x, x1=None, up=False):
        """x itself when it is a Lazy, else the rows of the tensor x [| x1 beside it], x at half resolution when `up`"""
        if isinstance(x, Lazy):
            return x
        t, ld = rows(x)
        n, c, h, w = t.shape
        if up:
            h, w = 2 * h, 2 * w
        if x1 is None:
            return Lazy((n, c, h, w), t, ld, c, up=up, keep=(t,))
        t1, ld1 = rows(x1)
        return Lazy((n, c + t1.shape[1], h, w), t, ld, c, a1=t1, lda1=ld1, up=up, keep=(t, t1))

    def materialize(self):
        n, c, h, w = self.shape
        if self.gate is not None:
            assert self.a1 is None and not self.up
            return coordatt_gate(self.a0, self.lda0, n, h, w, c, self.gate[0], self.gate[1])
        parts = []
        a0 = self.keep[0]
        if self.up:
            a0 = torch.nn.functional.interpolate(a0, scale_factor=2, mode="nearest")
        parts.append(a0)
        if self.a1 is not None:
            parts.append(self.keep[1])
        return parts[0] if len(parts) == 1 else torch.cat(parts, 1)


def sources(x):
    """(x0, x1, up) of a tensor or Lazy: the tensors autograd sees as the inputs of a training node (Lazy.of(x0, x1, up) is the
    node's source again).  The nodes carry no gate prologue: a gated Lazy is materialised first."""
    if not isinstance(x, Lazy):
        return x, None, False
    if x.gate is not None:
        return x.materialize(), None, False
    return x.keep[0], (x.keep[1] if x.a1 is not None else None), x.up


def unit_out(kind, src, n_out, k=1, dtype=None):
    """fresh NHWC output of conv_unit(kind, src, ..., n_out) (k: the patch size of kind "patch")"""
    n, _, h, w = src.shape
    return empty_nhwc(n, n_out, h // k, w // k, src.a0 if isinstance(src, Lazy) else src, dtype)


def conv_unit(kind, src, wp, n_out, e_scale, e_shift, act, *, stats=None, out=None, ldo=None, k=1, nchw=False, dtype=None):
    """THE forward launch of a conv -> [BN] -> act unit, eval and training: out rows (stride ldo, default n_out) = act(e_scale * conv(src; wp)
    + e_shift), and / or its per-channel statistics.  kind "pw": 1x1 over a Lazy (one or two row sources, 2x-upsample gather, CoordAtt gate
    prologue); "c3": 3x3 stride 1 pad 1 over a tensor; "patch": k x k stride k over an NHWC tensor, or (nchw) over an NCHW image.  dtype: the
    storage type of the patch output when it is not the source's (an fp32 / uint8 image -> a bf16 map)."""
    ep = dict(N=n_out, wp=wp, out=out, ldo=n_out if ldo is None else ldo, e_scale=e_scale, e_shift=e_shift, act=act, stats=stats)
    if kind == "pw":
        n, c, h, w = src.shape
        pro = dict(pro=PRO_GATE, g_h=src.gate[0], g_w=src.gate[1]) if src.gate is not None else {}
        gemm(M=n * h * w, H=h, W=w, K=c, a0=src.a0, lda0=src.lda0, k0=src.k0, a1=src.a1, lda1=src.lda1,
             gather=GATHER_UP2 if src.up else GATHER_ROWS, **pro, **ep)
    elif kind == "c3":
        x, ld = rows(src)
        n, c, h, w = x.shape
        conv3x3(M=n * h * w, H=h, W=w, Cin=c, x=x, ldx=ld, **ep)
    else:
        n, c, h, w = src.shape
        if nchw:
            if k != 4 or w % 4 != 0:
                raise NotImplementedError("HIP patch embedding of an NCHW image needs patch_size 4 and W % 4 == 0")
            g = dict(K=16 * c, a0=src.contiguous(), lda0=0, k0=16 * c, gather=GATHER_PATCH_NCHW, ks=4, pk=0)
        else:                                           # the patch gather walks dense rows (lda0 = c): a channel slice is copied
            g = dict(K=k * k * c, a0=rows_dense(src), lda0=c, k0=k * k * c, gather=GATHER_PATCH, ks=k, pk=k * c)
        gemm(M=n * (h // k) * (w // k), H=h // k, W=w // k, Hin=h, Win=w, Cin=c, dtype=dtype or g["a0"].dtype, **g, **ep)


def _tname(t):
    return "float" if t.dtype == torch.float32 else "__bf16"


def _bname(flag):
    return "true" if flag else "false"


def pool_hw(x, ldx, n, h, w, c):
    pool = torch.empty((n, h + w, c), dtype=torch.float32, device=x.device)
    with _Timed(f"ly_pool_hw_kernel<{_tname(x)}>", 1.0 * n * h * w * c, x.element_size() * n * h * w * c):
        capi.check(capi.lib().ly_pool_hw(_p(x), ldx, n, h, w, c, _p(pool), capi.dtype_code(x), capi.stream_ptr()), "ly_pool_hw")
    return pool


def coordatt_mlp(pool, n, h, w, c, mip, w1, b1, wh, bh, ww, bw, sc=None, sh=None):
    """sc/sh: bn1 as a per-channel affine applied after the raw conv1 (train mode); None = already folded into w1/b1"""
    a_h = torch.empty((n, h, c), dtype=torch.float32, device=pool.device)
    a_w = torch.empty((n, w, c), dtype=torch.float32, device=pool.device)
    capi.check(capi.lib().ly_coordatt_mlp(_p(pool), n, h, w, c, mip, _p(w1), _p(b1), _p(sc), _p(sh), _p(wh), _p(bh), _p(ww), _p(bw), _p(a_h),
                                          _p(a_w), capi.stream_ptr()), "ly_coordatt_mlp")
    return a_h, a_w


def coordatt_mlp_bwd(pool, n, h, w, c, mip, w1, b1, mean, invstd, gamma, beta, wh, ww, a_h, a_w, da_h, da_w, targets):
    """targets: (dw1, dgamma, dbeta, dwh, dbh, dww, dbw) buffers that are ADDED to — all fp32, or all float64 scratches (small_grad_scratch);
    returns dpool [n, h+w, c]"""
    r = n * (h + w)
    sums = zeros_f64(32 * 2 * mip, pool.device)                        # striped (sum dy1, sum dy1*xh), double accumulators
    ws = torch.empty(r * 3 * mip, dtype=torch.float32, device=pool.device)
    dpool = torch.empty((n, h + w, c), dtype=torch.float32, device=pool.device)
    # (two launches: the record carries the second, whose instantiation `mip` alone fixes; ly_coordatt_mlp_bwd1_kernel<mip, NS> runs ahead of it)
    with _Timed(f"ly_coordatt_mlp_bwd2_kernel<{mip}>", 8.0 * r * c * mip, 4.0 * 4 * r * c):
        capi.check(capi.lib().ly_coordatt_mlp_bwd(_p(pool), n, h, w, c, mip, _p(w1), _p(b1), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(wh), _p(ww),
                                                  _p(a_h), _p(a_w), _p(da_h), _p(da_w), _p(ws), _p(sums), _p(dpool),
                                                  *[_p(t) for t in targets], int(targets[0].dtype == torch.float64), capi.stream_ptr()),
                   "ly_coordatt_mlp_bwd")
    return dpool


def coordatt_gate(x, ldx, n, h, w, c, a_h, a_w, res=None, ldres=0):
    out = empty_nhwc(n, c, h, w, x)
    with _Timed(f"ly_gate_kernel<{_tname(x)}>", 2.0 * n * h * w * c, 2.0 * x.element_size() * n * h * w * c):
        capi.check(capi.lib().ly_coordatt_gate(_p(x), ldx, n, h, w, c, _p(a_h), _p(a_w), _p(res), ldres, _p(out), c, capi.dtype_code(x),
                                               capi.stream_ptr()), "ly_coordatt_gate")
    return out


def se_attention(x, ldx, n, hw, c, wa, wb, r, want_part=False):
    slices = se_slices(hw)                       # short per-block row loops: the pass is latency-bound, not bandwidth-bound
    part = torch.empty((n, slices, c), dtype=torch.float32, device=x.device)
    ca = torch.empty((n, c), dtype=torch.float32, device=x.device)
    with _Timed(f"ly_colsum_kernel<{_tname(x)}> + ly_se_mlp_kernel", 1.0 * n * hw * c, x.element_size() * n * hw * c):
        capi.check(capi.lib().ly_se_fwd(_p(x), ldx, n, hw, c, _p(wa), _p(wb), r, _p(part), slices, _p(ca), capi.dtype_code(x), capi.stream_ptr()),
                   "ly_se_fwd")
    return (ca, part) if want_part else ca


def se_bwd(part, n, hw, c, wa, wb, r, ca, d_ca, dwa, dwb):
    """SE backward: dwa [r, c] / dwb [c, r] are ADDED to; returns dgap [n, c] = d/d(mean x).  d_ca: float32, or the float64 accumulators
    the RFCBAM backward kernels sum it in (read as they are)"""
    if d_ca.dtype not in (torch.float32, torch.float64) or d_ca.numel() != n * c or not d_ca.is_contiguous():
        raise ValueError("se_bwd: d_ca must be a contiguous float32 / float64 [n, c]")
    dgap = torch.empty((n, c), dtype=torch.float32, device=part.device)
    ws = torch.empty(n * (2 * c + 2 * r), dtype=torch.float32, device=part.device)
    capi.check(capi.lib().ly_se_bwd(_p(part), part.shape[1], n, hw, c, _p(wa), _p(wb), r, _p(ca), _p(d_ca), int(d_ca.dtype == torch.float64), _p(dwa), _p(dwb), _p(dgap), _p(ws),
                                    capi.stream_ptr()), "ly_se_bwd")
    return dgap


def se_slices(hw):
    """pixel slices of the SE pooling partials: a function of the MAP only, so results do not change with the batch split"""
    return max(1, min(hw // 64, 128))


def colsum(x, ldx, n, hw, c):
    """SE pooling partials part[n][slice][c] (one pass over x)"""
    slices = se_slices(hw)
    part = torch.empty((n, slices, c), dtype=torch.float32, device=x.device)
    with _Timed(f"ly_colsum_kernel<{_tname(x)}>", 1.0 * n * hw * c, x.element_size() * n * hw * c):
        capi.check(capi.lib().ly_colsum(_p(x), ldx, n, hw, c, _p(part), slices, capi.dtype_code(x), capi.stream_ptr()), "ly_colsum")
    return part


def pick_tile(ho, wo):
    """TH x TW (<= 64 output pixels, one per lane) minimising idle lanes over the Ho x Wo map."""
    best = None
    for nct in range(1, 9):
        tw = -(-wo // nct)
        if tw > 64:
            continue
        th = max(1, 64 // tw)
        th = min(th, ho)
        nrt = -(-ho // th)
        eff = (ho * wo) / (nct * nrt * 64.0)
        if best is None or eff > best[0] + 1e-9:
            best = (eff, th, tw)
    if best is None:
        return 1, 64
    return best[1], best[2]


def rf_out_hw(h, w, k, s):
    """output map of RFCBAMConv's `generate` (kernel k, padding k // 2, stride s) over an h x w input"""
    return (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1


def rf3c_ok(c, s):
    """the lane = channel RFCBAMConv k=3 kernels (csrc/ly_rf3c.hip) cover C % 32 == 0 at stride 1 / 2"""
    return c % 32 == 0 and s in (1, 2)


def rf3m_mt(o):
    """32-channel output tiles per block of ly_rf3m_fwd, and of pack.rf3m_stream's weight stream: 4 (128 channels) or 2 (64)"""
    return 4 if o % 128 == 0 else 2


RF3M_MIN_UNITS = 1500      # wave tiles x output-channel blocks below which the lane = channel kernels are faster (measured, MI355X, module time in us,
                           # rf3c / rf3m: layer 17 bs 16: 79 / 89, bs 32: 135 / 101, bs 64: 227 / 185; layer 20 bs 32: 110 / 144, bs 64: 165 / 155 — a block of
                           # ly_rf3m walks ALL input channels of its 256 pixels serially, ~45 us however small the launch)


CONCURRENT_PARTS = 1       # graph.GraphedForward runs the batch as this many sub-batches side by side: size-based dispatch decisions look at the
                           # whole batch, so that a sub-batched replay takes the kernels (and returns the bits) of the eager forward of the full batch


def rf3m_ok(x, c, o, s, n=None, ho=None, wo=None):
    """`generate` on the matrix cores (csrc/ly_rf3m.hip): bf16 storage, C % 32 == 0, O % 64 == 0, stride 1 / 2 — and, when the problem size
    is given, enough wave tiles to fill the chip (RF3M_MIN_UNITS)"""
    if not ((x if isinstance(x, torch.dtype) else x.dtype) == torch.bfloat16 and c % 32 == 0 and o % 64 == 0 and s in (1, 2)):
        return False
    return n is None or rf3m_units(n, ho, wo, o, s) >= RF3M_MIN_UNITS


def rf3m_units(n, ho, wo, o, s):
    """wave tiles x output-channel blocks of ly_rf3m_fwd over the whole batch (all CONCURRENT_PARTS sub-batches)"""
    th, tw = pick_tile_m(ho, wo, s)
    return n * CONCURRENT_PARTS * -(-ho // th) * -(-wo // tw) * (o // (32 * rf3m_mt(o)))


def pick_tile_m(ho, wo, s):
    """TH x TW wave tile of csrc/ly_rf3m.hip: at most 32 output pixels reading at most 160 input positions; fewest tiles, then smallest halo"""
    best = None
    for tw in range(1, 33):
        for th in range(1, 32 // tw + 1):
            pos = (s * (th - 1) + 3) * (s * (tw - 1) + 3)
            if pos > 160 or th > ho or tw > max(wo, 1) * 2:
                continue
            key = (-(-ho // th) * -(-wo // tw), pos)
            if best is None or key < best[0]:
                best = (key, th, tw)
    return best[1], best[2]


def _rf3_stats_out(x, n, h, w, c, s, th, tw, gap):
    """what a fused k = 3 statistics pass (rf3c_stats, rf3m_stats) writes: (ho, wo, tiles, mm [n, 3ho, 3wo, 2], part [n, tiles, c] or None)"""
    ho, wo = rf_out_hw(h, w, 3, s)
    tiles = -(-ho // th) * -(-wo // tw)
    mm = torch.empty((n, 3 * ho, 3 * wo, 2), dtype=torch.float32, device=x.device)
    part = torch.empty((n, tiles, c), dtype=torch.float32, device=x.device) if gap else None
    return ho, wo, tiles, mm, part


def rf3m_stats(x, ldx, n, h, w, c, s, wst, th, tw, gap=True):
    """ONE pass over x (csrc/ly_rf3m.hip): (mm [n, 3ho, 3wo, 2], part [n, tiles, c])"""
    ho, wo, tiles, mm, part = _rf3_stats_out(x, n, h, w, c, s, th, tw, gap)
    # generate on the MFMAs: 3 + 3 products of 32 x 32 x 16 per 4-channel group and 32 pixels (3/4 of them multiply structural zeros)
    with _Timed("ly_rf3m_stats_kernel", 2.0 * n * ho * wo * (c // 4) * 6 * 32 * 16, x.element_size() * n * h * w * c + 4.0 * 18 * n * ho * wo):
        capi.check(capi.lib().ly_rf3m_stats(_p(x), ldx, n, h, w, c, s, _p(wst), th, tw, _p(mm), _p(part), tiles, capi.stream_ptr()), "ly_rf3m_stats")
    return mm, part


def rf3m_fwd(*, n, h, w, c, ho, wo, N, s, th, tw, x, ldx, ca, rfa, wp, e_scale, e_shift, out, ldo):
    P = capi.LyRfcbam3Params(n, h, w, c, ho, wo, N, s, th, tw, _p(x), ldx, None, _p(ca), _p(rfa), _p(wp), _p(e_scale),
                             _p(e_shift), _p(out), ldo, None, 0, capi.dtype_code(x))
    mo = n * ho * wo
    with _Timed(_label("ly_rf3m_fwd_describe", ctypes.byref(P)), 2.0 * mo * 9 * c * N + 2.0 * mo * (N // (32 * rf3m_mt(N))) * (c // 4) * 6 * 32 * 16,
                x.element_size() * (n * h * w * c + mo * N) + 2.0 * 9 * c * N):
        capi.check(capi.lib().ly_rf3m_fwd(ctypes.byref(P), capi.stream_ptr()), "ly_rf3m_fwd")


def pick_tile_c(ho, wo, s):
    """TH x TW tile of the lane = channel kernels: TW even, TH*TW <= 64, at most 320 input positions; fewest tiles, then smallest halo"""
    best = None
    for tw in range(2, 65, 2):
        th = min(64 // tw, ho)
        if th < 1:
            continue
        pos = (s * (th - 1) + 3) * (s * (tw - 1) + 3)
        if pos > 320:
            continue
        tiles = -(-ho // th) * -(-wo // tw)
        key = (tiles, pos)
        if best is None or key < best[0]:
            best = (key, th, tw)
    return best[1], best[2]


def pick_tile_bwd_dx(ho, wo, o):
    """tile of the recompute backward's dx pass (csrc/ly_rf3c_bwd.hip pass C): its pixel pairs are walked in four colours (row parity x pair-column
    parity) of ceil(count / 8) iterations each — fewest iteration slots over the map among the tiles whose LDS footprint fits, then smallest halo"""
    best = None
    for tw in range(2, 65, 2):
        th = min(64 // tw, ho)
        ih, iw = 2 * (th - 1) + 3, 2 * (tw - 1) + 3
        pos = ih * iw
        nct = -(-wo // tw)
        if th < 1 or pos > 320 or capi.lib().ly_rf3c_bwd_lds(2, th, tw, wo, o) > 160 * 1024:
            continue
        its = sum(-(-(((th + 1 - ry) // 2) * ((tw // 2 + 1 - rx) // 2)) // 8) for ry in (0, 1) for rx in (0, 1))
        key = (-(-ho // th) * nct * its, pos)
        if best is None or key < best[0]:
            best = (key, th, tw)
    return best[1], best[2]


def rf3c_stats(x, ldx, n, h, w, c, s, wq, th, tw, gap=True, raw=False):
    """ONE pass over x: (mm [n, 3ho, 3wo, 2], part [n, tiles, c]) — the [max, mean] map of relu(bn(generate(x))) and SE's pooling partials"""
    ho, wo, tiles, mm, part = _rf3_stats_out(x, n, h, w, c, s, th, tw, gap)
    with _Timed(f"ly_rf3c_stats_kernel<{_tname(x)}, {s}, {'true' if raw else 'false'}>", 0.0, x.element_size() * n * h * w * c + 4.0 * 18 * n * ho * wo, valu_flops=2.0 * n * ho * wo * c * 81):
        capi.check(capi.lib().ly_rf3c_stats(_p(x), ldx, n, h, w, c, s, _p(wq), int(raw), th, tw, _p(mm), _p(part), tiles, capi.dtype_code(x),
                                            capi.stream_ptr()), "ly_rf3c_stats")
    return mm, part


def rf3c_fwd(*, n, h, w, c, ho, wo, N, s, th, tw, x, ldx, wq, ca, rfa, wp, e_scale, e_shift, out, ldo, stats=None, linear=False, raw=False):
    P = capi.LyRfcbam3Params(n, h, w, c, ho, wo, N, s, th, tw, _p(x), ldx, None, _p(ca), _p(rfa), _p(wp), _p(e_scale),
                             _p(e_shift), _p(out), ldo, _p(stats), int(linear), capi.dtype_code(x))
    mo = n * ho * wo
    with _Timed(_label("ly_rf3c_fwd_describe", ctypes.byref(P), _p(wq), int(raw)), 2.0 * mo * 9 * c * N,
                x.element_size() * (n * h * w * c + mo * N) + 4.0 * 9 * c * N, valu_flops=2.0 * mo * 81 * c):
        capi.check(capi.lib().ly_rf3c_fwd(ctypes.byref(P), _p(wq), int(raw), capi.stream_ptr()), "ly_rf3c_fwd")


PRE1_PIXELS = 64           # pixels per block of the k = 1 statistics + pooling pass (ly_rfcbam_pre1v: 16 pixels per trip; measured 16 / 32 / 64 / 128:
                           # 19.5 / 16.9 / 16.7 / 16.2 us at 256 x 40 x 40 x 64, 10.5 / 10.4 / 10.4 / 11.1 at 160 x 20 x 20 x 64)


def rfcbam_stats(x, ldx, n, h, w, c, k, s, wg=None, a1=None, b1=None, th=1, tw=64, gap=False):
    """[max, mean] map of relu(bn(generate(x))); gap=True: the same pass also leaves the SE pooling partials -> (mm, part)"""
    ho, wo = rf_out_hw(h, w, k, s)
    mm = torch.empty((n, k * ho, k * wo, 2), dtype=torch.float32, device=x.device)
    part, slices = None, 0
    if gap:
        if k == 3:
            raise NotImplementedError("the fused statistics + pooling pass is built for k = 1 (for k = 3 the extra per-chunk LDS pass cost more "
                                      "than the separate ly_colsum launch it saved: measured 44 -> 69 us)")
        slices = max(1, min(h * w // PRE1_PIXELS, 128))    # a function of the map only: results do not change with the batch split
        part = torch.empty((n, slices, c), dtype=torch.float32, device=x.device)
    args = (_p(x), ldx, n, h, w, c, k, s, _p(wg), _p(a1), _p(b1), th, tw, _p(mm), _p(part), slices, capi.dtype_code(x))
    with _Timed(_label("ly_rfcbam_stats_describe", *args), 0.0,
                x.element_size() * n * h * w * c + 4.0 * 2 * k * k * n * ho * wo, valu_flops=2.0 * n * ho * wo * c * (81 if k == 3 else 1)):
        capi.check(capi.lib().ly_rfcbam_stats(*args, capi.stream_ptr()), "ly_rfcbam_stats")
    return (mm, part) if gap else mm


def rfcbam_mid(part, hw, wa, wb, r, mm, w18):
    """SE's linears (from the pooling partials) + get_weight's 3x3 conv on the [max, mean] map, one launch -> (ca, rfa)"""
    n, slices, c = part.shape
    _, hk, wk, _ = mm.shape
    ca = torch.empty((n, c), dtype=torch.float32, device=part.device)
    rfa = torch.empty((n, hk, wk), dtype=torch.float32, device=mm.device)
    with _Timed("ly_rfcbam_mid_kernel", 36.0 * n * hk * wk, 12.0 * n * hk * wk + 4.0 * n * slices * c):
        capi.check(capi.lib().ly_rfcbam_mid(_p(part), slices, c, hw, _p(wa), _p(wb), r, _p(ca), n, _p(mm), hk, wk, _p(w18), _p(rfa), capi.stream_ptr()),
                   "ly_rfcbam_mid")
    return ca, rfa


def rfa_map(mm, w18):
    n, hk, wk, _ = mm.shape
    rfa = torch.empty((n, hk, wk), dtype=torch.float32, device=mm.device)
    with _Timed("ly_rfa_map_kernel", 36.0 * n * hk * wk, 12.0 * n * hk * wk):
        capi.check(capi.lib().ly_rfa_map(_p(mm), n, hk, wk, _p(w18), _p(rfa), capi.stream_ptr()), "ly_rfa_map")
    return rfa


def rfcbam3(*, n, h, w, c, ho, wo, N, s, th, tw, x, ldx, wg, ca, rfa, wp, e_scale, e_shift, out, ldo, stats=None, linear=False):
    P = capi.LyRfcbam3Params(n, h, w, c, ho, wo, N, s, th, tw, _p(x), ldx, _p(wg), _p(ca), _p(rfa), _p(wp), _p(e_scale),
                             _p(e_shift), _p(out), ldo, _p(stats), int(linear), capi.dtype_code(x))
    mo = n * ho * wo
    with _Timed(_label("ly_rfcbam3_describe", ctypes.byref(P)), 2.0 * mo * 9 * c * N,
                x.element_size() * (n * h * w * c + mo * N) + 4.0 * 9 * c * N, valu_flops=2.0 * mo * 81 * c):
        capi.check(capi.lib().ly_rfcbam3_fwd(ctypes.byref(P), capi.stream_ptr()), "ly_rfcbam3_fwd")


def sppf_pool_fits(h, w):
    return 2 * h * w * 4 * 4 <= 160 * 1024


def sppf_pool(x, ldx, n, h, w, c, k, out, ldo):
    with _Timed(f"ly_sppf_pool_kernel<{_tname(x)}>", 0.0, 5.0 * x.element_size() * n * h * w * c):
        capi.check(capi.lib().ly_sppf_pool(_p(x), ldx, n, h, w, c, k, _p(out), ldo, capi.dtype_code(x), capi.stream_ptr()), "ly_sppf_pool")


def detect_tail(y, ldy, n, h, w, na, no, anchors, stride, p, z, zrows, zoff):
    capi.check(capi.lib().ly_detect_tail(_p(y), ldy, n, h, w, na, no, _p(anchors), float(stride), _p(p), _p(z), zrows, zoff,
                                         capi.dtype_code(y), capi.stream_ptr()), "ly_detect_tail")


def detect_level_ok(k, na, no, dtype):
    return dtype in (torch.float32, torch.bfloat16) and bool(capi.lib().ly_detect_level_ok(k, na, no, capi.dtype_code(dtype)))


FUSED_DETECT_LEVEL = True      # development switch: False sends Detect levels, eval and training, through the GEMM + ly_detect_tail pair
                               # (training forward: measured 25-50 us per step slower)


def detect_level_rows(x, cin, na, no):
    """the feature map x as (rows, ld) when the one-launch level kernel (detect_level / detect_level_aug) takes it, else None"""
    if not FUSED_DETECT_LEVEL or not detect_level_ok(cin, na, no, x.dtype):
        return None
    t, ld = rows(x)
    return (t, ld) if ld % vw_of(t) == 0 and t.data_ptr() % 16 == 0 else None


def detect_level(x, ldx, n, h, w, k, wp, bias, na, no, anchors, stride, p, z, zrows, zoff, nat=True):
    """head 1x1 convolution + decode of one Detect level in ONE launch (ly_detect_level): x rows [n*h*w, k] -> p [n, na, h, w, no], z rows
    (z None: raw maps only).  nat: wp from pack.frag_pack_nat, else the frag_pack3 layout (>= 32 rows)"""
    es = x.element_size()
    with _Timed(f"ly_detect_level_kernel<{_tname(x)}, {k // 32}, {_bname(nat)}, false>", 2.0 * n * h * w * k * 32, es * n * h * w * k + 8.0 * n * h * w * na * no):
        capi.check(capi.lib().ly_detect_level(_p(x), ldx, n, h, w, k, _p(wp), int(nat), _p(bias), na, no, _p(anchors), float(stride), _p(p), _p(z), zrows, zoff,
                                              capi.dtype_code(x), capi.stream_ptr()), "ly_detect_level")


def detect_tail_aug(y, ldy, n, h, w, na, no, anchors, stride, z, zrows, zoff, dscale, dflip, img_w):
    """ly_detect_tail with the _descale_pred step of test-time augmentation on the decoded rows (no raw maps)"""
    capi.check(capi.lib().ly_detect_tail_aug(_p(y), ldy, n, h, w, na, no, _p(anchors), float(stride), None, _p(z), zrows, zoff, float(dscale),
                                             int(dflip), float(img_w), capi.dtype_code(y), capi.stream_ptr()), "ly_detect_tail_aug")


def detect_level_aug(x, ldx, n, h, w, k, wp, bias, na, no, anchors, stride, z, zrows, zoff, dscale, dflip, img_w, nat=True):
    """ly_detect_level with the _descale_pred step of test-time augmentation on the decoded rows: z[..., :4] / dscale, then x = img_w - x when
    dflip; no raw maps"""
    es = x.element_size()
    with _Timed(f"ly_detect_level_kernel<{_tname(x)}, {k // 32}, {_bname(nat)}, true>", 2.0 * n * h * w * k * 32, es * n * h * w * k + 4.0 * n * h * w * na * no):
        capi.check(capi.lib().ly_detect_level_aug(_p(x), ldx, n, h, w, k, _p(wp), int(nat), _p(bias), na, no, _p(anchors), float(stride), None, _p(z),
                                                  zrows, zoff, float(dscale), int(dflip), float(img_w), capi.dtype_code(x), capi.stream_ptr()),
                   "ly_detect_level_aug")


SCALE_IMG_PAD = 0.447       # utils/torch_utils.py scale_img: F.pad(value=0.447)
_IMG_DTYPES = {torch.float32: capi.LY_F32, torch.bfloat16: capi.LY_BF16, torch.float16: capi.LY_F16}


def scale_img(x, specs, pad=SCALE_IMG_PAD):
    """The resampled passes of test-time augmentation in ONE launch (ly_scale_img): x NCHW [n, c, h, w] (float32 / bfloat16 / float16);
    specs = [(hs, ws, ho, wo, flip)]: (x.flip(3) if flip else x) bilinearly resized to hs x ws (F.interpolate, align_corners=False) in the
    top-left corner of an ho x wo canvas of `pad`.  Returns the list of outputs, contiguous NCHW, x's dtype."""
    if not x.is_cuda:
        raise RuntimeError(f"scale_img: the HIP path needs a CUDA/ROCm tensor (got {x.device}); there is no CPU fallback")
    if x.dtype not in _IMG_DTYPES or x.dim() != 4:
        raise TypeError(f"scale_img: a float32 / bfloat16 / float16 NCHW image batch expected (got {x.dtype}, {tuple(x.shape)})")
    if not 1 <= len(specs) <= capi.SCALE_IMG_MAX:
        raise ValueError(f"scale_img: 1..{capi.SCALE_IMG_MAX} outputs per launch (got {len(specs)})")
    x = x.contiguous()
    n, c, h, w = x.shape
    outs = [torch.empty((n, c, ho, wo), dtype=x.dtype, device=x.device) for (_, _, ho, wo, _) in specs]
    arr = (capi.LyScaleImgSpec * len(specs))(*[capi.LyScaleImgSpec(o.data_ptr(), hs, ws, ho, wo, int(bool(fl)))
                                               for o, (hs, ws, ho, wo, fl) in zip(outs, specs)])
    tn = {torch.float32: "float", torch.bfloat16: "__bf16", torch.float16: "_Float16"}[x.dtype]
    # algorithmic bytes: the source once per output, every output element once
    with _Timed(f"ly_scale_img_kernel<{tn}>", 0.0, x.element_size() * sum(n * c * (h * w + ho * wo) for (_, _, ho, wo, _) in specs)):
        capi.check(capi.lib().ly_scale_img(_p(x), n, c, h, w, arr, len(specs), float(pad), _IMG_DTYPES[x.dtype], capi.stream_ptr()), "ly_scale_img")
    return outs


def resize_u8(x, size, out=None):
    """The resized batch of a multi-scale training step in ONE launch (ly_resize_u8): x uint8 NCHW [n, c, h, w] ->
    F.interpolate(x.float() / 255, size=size, mode='bilinear', align_corners=False), float32 contiguous NCHW; `size` = (ho, wo), wo a
    multiple of 4.  `out` (float32 [n, c, ho, wo], contiguous): written in place of a new tensor — the input buffer of a captured graph."""
    if not x.is_cuda:
        raise RuntimeError(f"resize_u8: the HIP path needs a CUDA/ROCm tensor (got {x.device}); there is no CPU fallback")
    if x.dtype != torch.uint8 or x.dim() != 4:
        raise TypeError(f"resize_u8: a uint8 NCHW image batch expected (got {x.dtype}, {tuple(x.shape)})")
    x = x.contiguous()
    n, c, h, w = x.shape
    ho, wo = (int(s) for s in size)
    if out is None:
        if ho <= 0 or wo <= 0 or n * c * ho * wo >= 1 << 31:
            raise ValueError(f"resize_u8: cannot resize {tuple(x.shape)} to {ho} x {wo}")
        out = torch.empty((n, c, ho, wo), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n, c, ho, wo) or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"resize_u8: out must be a contiguous float32 {(n, c, ho, wo)} tensor on {x.device} (got {out.dtype}, {tuple(out.shape)})")
    # algorithmic bytes: the source once, every output element once
    with _Timed("ly_resize_u8_kernel", 0.0, 1.0 * n * c * h * w + 4.0 * n * c * ho * wo):
        capi.check(capi.lib().ly_resize_u8(_p(x), n, c, h, w, _p(out), ho, wo, capi.stream_ptr()), "ly_resize_u8")
    return out


def detect_head_bwd(dp, n, h, w, na, no, du, ldu, dbias):
    """dp fp32 [n, na, h, w, no] -> du rows [n*h*w, ldu] (columns >= na*no zero), dbias[na*no] += column sums (dbias fp32, or a float64
    scratch of small_grad_scratch)"""
    capi.check(capi.lib().ly_detect_head_bwd(_p(dp), n, h, w, na, no, _p(du), ldu, _p(dbias), int(dbias.dtype == torch.float64), capi.dtype_code(du),
                                             capi.stream_ptr()), "ly_detect_head_bwd")


# ---- small parameter-gradient reductions, reproducibly -------------------------------------------------------------------------------
# A few kernels add a handful of values from many blocks into a parameter gradient (Detect bias, get_weight's taps, the k = 1 generate weight,
# CoordAtt's MLP).  With float atomics those gradients moved by ~1e-6 from run to run — the only part of a training step that was not the same
# bits every time.  Inside a backward pass they accumulate into zeroed DOUBLE scratches instead (the arrival order then only moves the 53rd
# bit), and ONE ly_f64_add launch, queued on the autograd engine for the end of the pass, rounds every sum into its fp32 `.grad` storage.
class _SmallGrads:
    pending = []            # (scratch, flat fp32 target, parameter)
    task = -1               # autograd graph-task id the pending entries (and the queued end-of-pass callback) belong to
    announced = set()       # id(parameter) of the entries that already left in this pass (early flush under a gradient listener)
    nodes = {}              # id(scratch) -> id of the autograd node that took it


DETERMINISTIC_SMALL_GRADS = True


def _graph_task():
    task = getattr(torch._C, "_current_graph_task_id", None)
    return task() if task is not None else -1


def small_grads_ok():
    """inside a backward pass of the autograd engine (where the end-of-pass callback can be queued)?"""
    return DETERMINISTIC_SMALL_GRADS and _graph_task() != -1


def small_grads_reset():
    """drop whatever an aborted backward pass left behind (the engine discards a graph task's final callbacks when a backward raises:
    the entries would otherwise wait for a flush that never comes)"""
    _SmallGrads.pending, _SmallGrads.task, _SmallGrads.announced, _SmallGrads.nodes = [], -1, set(), {}
    _WgradQueue.items, _WgradQueue.notify, _WgradQueue.task = [], [], -1


def small_grad_scratch(target, param):
    """zeroed float64 stand-in for the fp32 gradient storage `target` (contiguous) of `param`; added into it — and `grad_done(param)` called —
    when the running backward pass ends.  The pending list is keyed on the engine's graph-task id: entries of ANOTHER pass are leftovers of a
    backward that raised after taking a scratch (its callback was dropped with it) — they are discarded and the callback queued anew.  A
    parameter deferred twice in one pass (a module applied twice, shared weights) reuses ONE scratch: ly_f64_add's table then holds one
    entry per destination (two entries with the same target would race)."""
    task = _graph_task()
    if task != _SmallGrads.task:
        _SmallGrads.pending, _SmallGrads.task, _SmallGrads.announced, _SmallGrads.nodes = [], task, set(), {}
        torch.autograd.Variable._execution_engine.queue_callback(flush_small_grads)
    tgt = target.view(-1)
    for scr, t, prm in _SmallGrads.pending:
        if t.data_ptr() == tgt.data_ptr() and t.numel() == tgt.numel():
            return scr
    node = _autograd_node()
    if GRAD_LISTENERS and SMALL_GRADS_EARLY_FLUSH and node is not None:
        # under a gradient listener (ddp.GradReducer) a waiting sum holds back its whole bucket's exchange until the backward pass ends
        # (tools/dp_overlap_probe.py: 5.4 of 12.5 MB left at 99-100 % of the backward).  Entries taken by EARLIER autograd nodes are complete
        # — their kernels are in the stream — and leave as soon as a handful has collected; entries of the running node stay (it may not
        # have launched the kernel that fills them yet).
        if param is not None and id(param) in _SmallGrads.announced:
            raise RuntimeError("small_grad_scratch: a parameter whose deferred gradient was already announced to the gradient listeners "
                               "receives another contribution in the same backward pass (shared weights under a GradReducer): set "
                               "ops.SMALL_GRADS_EARLY_FLUSH = False")
        old = [e for e in _SmallGrads.pending if _SmallGrads.nodes.get(id(e[0])) != node]
        if len(old) >= SMALL_GRADS_FLUSH_MIN:
            _SmallGrads.pending = [e for e in _SmallGrads.pending if _SmallGrads.nodes.get(id(e[0])) == node]
            _flush_small_items(old)
    scr = zeros_f64(target.numel(), target.device)
    if param is not None and not any(prm is param for _, _, prm in _SmallGrads.pending):
        for fn in GRAD_DEFER_LISTENERS:
            fn(param)
    _SmallGrads.pending.append((scr, tgt, param))
    _SmallGrads.nodes[id(scr)] = node
    return scr


SMALL_GRADS_EARLY_FLUSH = True
SMALL_GRADS_FLUSH_MIN = 6


def _autograd_node():
    fn = getattr(torch._C, "_current_autograd_node", None)
    n = fn() if fn is not None else None
    return id(n) if n is not None else None


def f64_round(scratches, shapes):
    """fp32 tensors holding the rounded sums of float64 scratches (the route without a gradient sink: the values go back to autograd) — ONE
    ly_f64_add launch into one zeroed buffer"""
    assert 0 < len(scratches) <= capi.F64_ADD_MAX
    sizes = [s_.numel() for s_ in scratches]
    flat = torch.zeros(sum(sizes), dtype=torch.float32, device=scratches[0].device)
    t = capi.LyF64AddTable()
    outs, off = [], 0
    for j, (scr, n, shp) in enumerate(zip(scratches, sizes, shapes)):
        t.src[j], t.dst[j], t.n[j] = scr.data_ptr(), flat.data_ptr() + 4 * off, n
        outs.append(flat[off:off + n].view(shp))
        off += n
    t.count = len(scratches)
    capi.check(capi.lib().ly_f64_add(ctypes.byref(t), capi.stream_ptr()), "ly_f64_add")
    return outs


def flush_small_grads():
    items, _SmallGrads.pending, _SmallGrads.task = _SmallGrads.pending, [], -1
    _flush_small_items(items)
    _SmallGrads.announced, _SmallGrads.nodes = set(), {}


def _flush_small_items(items):
    for i in range(0, len(items), capi.F64_ADD_MAX):
        chunk = items[i:i + capi.F64_ADD_MAX]
        t = capi.LyF64AddTable()
        for j, (scr, tgt, _) in enumerate(chunk):
            t.src[j], t.dst[j], t.n[j] = scr.data_ptr(), tgt.data_ptr(), tgt.numel()
        t.count = len(chunk)
        capi.check(capi.lib().ly_f64_add(ctypes.byref(t), capi.stream_ptr()), "ly_f64_add")
    done = set()
    for _, _, prm in items:
        if prm is not None and id(prm) not in done:
            done.add(id(prm))
            _SmallGrads.announced.add(id(prm))
            grad_done(prm)


class SmallGrad:
    """Where ONE parameter's small gradient of `numel` values goes.  `buf` is what the kernel ADDS into, `f64` says whether it holds doubles;
    `finish()` is called once the kernel that fills it is in the stream.  The sink's storage is taken when it is contiguous and holds `numel`
    values: as a deferred float64 scratch inside a backward pass, directly outside the engine.  Without it the values go back to autograd,
    through a fresh float64 buffer (DETERMINISTIC_SMALL_GRADS) or a plain fp32 one.
    `numel` is the parameter's own element count at every site (Detect's bias: na * no, get_weight: 18, the k = 1 generate weight: c), and a
    sink target has its parameter's shape: the size test only ever refused a Detect bias of another length, and still does; the value handed
    to autograd has the parameter's shape, as autograd demands."""

    def __init__(self, param, numel):
        t = grad_target(param)
        self.param = param
        self.target = t = t if t is not None and t.is_contiguous() and t.numel() == numel else None
        self.deferred = t is not None and small_grads_ok()        # rounded into the sink when the backward pass ends
        self.f64 = self.deferred or (t is None and DETERMINISTIC_SMALL_GRADS)
        self.buf = small_grad_scratch(t, param) if self.deferred else t.view(-1) if t is not None else \
            zeros_f64(numel, param.device) if self.f64 else torch.zeros(numel, dtype=torch.float32, device=param.device)      # (handed to autograd: not from the pool)

    def finish(self):
        """-> what the autograd function returns for the parameter (None: the gradient went to the sink)"""
        if self.target is None:
            return f64_round([self.buf], [self.param.shape])[0] if self.f64 else self.buf.view(self.param.shape)
        if not self.deferred:
            grad_done(self.param)               # (a deferred gradient is announced by flush_small_grads)
        return None


class _SmallGradGroup:
    """SmallGrad.group(params, zero): the small gradients of ONE kernel with a single float64 flag (CoordAtt's MLP backward) take one route:
      1. deferred float64 scratches (small_grad_scratch): inside a backward pass, every gradient bound for a contiguous sink target;
      2. fresh float64 buffers rounded by ONE f64_round launch in values(): no sink target anywhere, DETERMINISTIC_SMALL_GRADS;
      3. fp32 as they are: each one's sink target, or fresh zeros.
    params[i], i in `zero`, has a zero gradient (zero_bias_grad) and no buffer.  A parameter that does not require grad gets a buffer (the
    kernel writes all of `bufs`), but nothing is returned or announced for it."""

    def __init__(self, params, zero=()):
        self.params, self.zero, self.ret, self.bufs = params, zero, [], []
        for i, p in enumerate(params):
            if i in zero:
                self.ret.append(zero_bias_grad(p, p) if p.requires_grad else None)
                continue
            t = grad_target(p)
            self.bufs.append(t if t is not None else torch.zeros(p.shape, dtype=torch.float32, device=p.device))
            self.ret.append(self.bufs[-1] if t is None and p.requires_grad else None)
        live = [p for i, p in enumerate(params) if i not in zero]
        self.deferred = small_grads_ok() and all(r is None for r in self.ret) and all(b.is_contiguous() for b in self.bufs)
        self.fresh64 = not self.deferred and DETERMINISTIC_SMALL_GRADS and all(grad_target(p) is None for p in live)
        if self.deferred:
            self.bufs = [small_grad_scratch(b, p if p.requires_grad else None) for b, p in zip(self.bufs, live)]
        elif self.fresh64:
            self.shapes = [b.shape for b in self.bufs]
            self.bufs = [zeros_f64(b.numel(), b.device) for b in self.bufs]

    def values(self):              # once the kernel that fills `bufs` is in the stream -> the return values in the order of `params`
        if self.fresh64:
            rounded = iter(f64_round(self.bufs, self.shapes))
            for i, r in enumerate(self.ret):
                if i not in self.zero:
                    v = next(rounded)
                    self.ret[i] = v if r is not None else None
        return self.ret

    def finish(self):              # after the node's last launch, where it always announced: the listeners are told of what went to the sink
        for i, (p, r) in enumerate(zip(self.params, self.ret)):
            if r is None and p.requires_grad and (i in self.zero or not self.deferred):      # (deferred: announced by flush_small_grads)
                grad_done(p)


SmallGrad.group = _SmallGradGroup


def zero_bias_grad(like, param=None):
    """gradient of a convolution bias in front of a train-mode BatchNorm: BN removes the batch mean, d/dbias = 0.  Zeros of `like` for
    autograd to accumulate — or, with `param`, None when a sink holds the bias's gradient storage (adding zero launches nothing)."""
    return None if grad_target(param) is not None else torch.zeros_like(like)


OWN, CONTIGUOUS, TAP_ROWS = "own", "contiguous", "tap_rows"          # the sink-target layouts a kernel can add into (ParamGrad)


def tap_major(g):
    """gradient tensor of a [co, ci, kh, kw] weight whose storage is [co][kh][kw][ci] (see optim.FusedSGD)"""
    return g.dim() == 4 and not g.is_contiguous() and g.stride(1) == 1 and g.stride(3) == g.shape[1]


def _sink_view(param, accept):
    """the sink's tensor for `param` as a kernel that writes the layout `accept` adds into it, or None: no target, or not in that layout.
    OWN: whatever the target's strides are (the kernel takes them: ly_wgrad's dw_ts / dw_cs).  CONTIGUOUS: the parameter's own order.
    TAP_ROWS: [co, taps * ci] rows in [co][tap][ci] order — the storage behind a tap-major k x k target, a contiguous one-tap target."""
    t = grad_target(param)
    if t is None or accept == OWN:
        return t
    if accept == TAP_ROWS and t.dim() == 4 and t.shape[2] * t.shape[3] > 1:
        rows = t.permute(0, 2, 3, 1)            # (not contiguous: a reshape would hand out a copy, and the gradient written into it be lost)
        return rows.view(t.shape[0], -1) if tap_major(t) and rows.is_contiguous() else None
    return t if t.is_contiguous() and t.numel() == param.numel() else None


class ParamGrad:
    """Where the full-size fp32 gradient of ONE parameter goes — or of several that one kernel writes together (gamma / beta through
    ly_bn_bwd_coeffs, the SE linears through ly_se_bwd): the sink takes all or none.  `direct`: into the sink's storage, in the layout
    `accept`.  `bufs` (`buf`: the first) is what the kernels ADD into: the sink's tensors, else zeros made on first use — by torch.zeros,
    not from the step pool (they go to autograd), of the parameter's shape, or what the callable `fresh` returns (the caller's own
    storage).  `targets`: the sink's tensors or Nones, for a wrapper that makes its own fresh ones.  finish() is called once the launches
    that fill `bufs` are in the stream (or queued in _WgradQueue): direct -> the listeners are told, None; else what the autograd function
    returns: `bufs` — or the `values` the consumer made instead — each through `view`.  One parameter: one value; several: a tuple."""

    def __init__(self, *params, accept=OWN, fresh=None, view=None):
        self.params, self._fresh, self._view = params, fresh, view
        views = [_sink_view(p, accept) for p in params]
        self.direct = all(v is not None for v in views)
        self.targets = views if self.direct else [None] * len(params)
        self._bufs = views if self.direct else None

    @property
    def bufs(self):
        if self._bufs is None:
            f = self._fresh() if self._fresh is not None else [torch.zeros(p.shape, dtype=torch.float32, device=p.device) for p in self.params]
            self._bufs = [f] if torch.is_tensor(f) else list(f)
        return self._bufs

    buf = property(lambda self: self.bufs[0])

    def finish(self, *values):
        if self.direct:
            for p in self.params:
                grad_done(p)
        out = [None if self.direct else v if self._view is None else self._view(v) for v in (values or self.bufs)]
        return out[0] if len(out) == 1 else tuple(out)


def mlpblock(x, y, n, h, w, c, wp, w1, w2, sc, sh, stats=None):
    m = n * h * w
    with _Timed(_label("ly_mlpblock_fwd_describe", n, h, w, c, capi.dtype_code(x), int(stats is not None)), 2.0 * m * (9 * (c // 4) ** 2 + 4 * c * c),
                x.element_size() * (1 if stats is not None else 2) * m * c + 4.0 * (9 * (c // 4) ** 2 + 4 * c * c)):
        capi.check(capi.lib().ly_mlpblock_fwd(_p(x), _p(y), n, h, w, c, _p(wp), _p(w1), _p(w2), _p(sc), _p(sh), _p(stats), capi.dtype_code(x),
                                              capi.stream_ptr()), "ly_mlpblock_fwd")


def mlpblock_bwd_ok(x, c):
    """the fused MLPBlock backward (csrc/ly_mlpblock_bwd.hpp) is built for bf16 storage and C in 16 / 24 / 40 / 80"""
    return MLP_BWD_FUSED and x.dtype == torch.bfloat16 and bool(capi.lib().ly_mlpblock_bwd_ok(c, capi.dtype_code(x)))


MLP_BWD_FUSED = True       # tools / tests: False keeps the unfused backward (eleven launches over 2C-wide tensors)


def _mlpblock_bwd_slab(c, device):
    """the slab the fused backward's blocks park their weight-gradient tiles in: written by the pass and read back by its fold launch.  Taken
    from the caching allocator PER CALL (round 6; it was one persistent buffer per (device, C) shared by every MLPBlock of that width, safe
    only while all of them ran on one stream in order — ADVICE r5): the allocator orders reuse by stream, and inside a hipGraph capture the
    block comes from the graph's private pool, whose address the replay keeps."""
    return torch.empty(int(capi.lib().ly_mlpblock_bwd_slab_floats(c)), dtype=torch.float32, device=device)


def mlpblock_bwd(x, dy, n, h, w, c, wp, w1, w2t, w1t, a, b, *, stats=None, g=None, alpha=None, kappa=None, lam=None, dw1=None, dw2=None):
    """one pass of the fused MLPBlock backward: stats given = pass 1 (BatchNorm sums), else pass 2 (g, dw1 +=, dw2 +=)"""
    m = n * h * w
    p1 = stats is not None
    slab = None if p1 else _mlpblock_bwd_slab(c, x.device)
    hid = 2 * c
    flops = 2.0 * m * (9 * (c // 4) ** 2 + (2 if p1 else 5) * c * hid)
    with _Timed(_label("ly_mlpblock_bwd_describe", n, h, w, c, capi.dtype_code(x), 1 if p1 else 2), flops, x.element_size() * (2 if p1 else 3) * m * c + 4.0 * (9 * (c // 4) ** 2 + 2 * c * hid)):
        capi.check(capi.lib().ly_mlpblock_bwd(_p(x), _p(dy), _p(g), n, h, w, c, _p(wp), _p(w1), _p(w2t), _p(w1t), _p(a), _p(b), _p(alpha), _p(kappa), _p(lam),
                                              _p(stats), _p(slab), slab.numel() if slab is not None else 0, _p(dw1), _p(dw2), 1 if p1 else 2,
                                              capi.dtype_code(x), capi.stream_ptr()), "ly_mlpblock_bwd")


def mlpblock_bwd_dx_ok(x, c, w):
    """ly_mlpblock_bwd_dx is built for this (storage, C) and its tile fits LDS at map width w"""
    return MLP_BWD_FUSED and x.dtype == torch.bfloat16 and bool(capi.lib().ly_mlpblock_bwd_dx_ok(c, w, capi.dtype_code(x)))


def mlpblock_bwd_dx(g, dy, x, n, h, w, c, wpt, dwp=None, lddw=0, dw_ts=0, dw_cs=0):
    """dx = dy + [pconv^T(g[:, :c/4]) | g[:, c/4:]] (+ dwp += the partial conv's weight gradient where the kernel builds it in): returns
    (dx, whether dwp was done)"""
    dx = torch.empty_like(dy)
    m = n * h * w
    slab = _mlpblock_bwd_slab(c, x.device) if (dwp is not None and capi.lib().ly_mlpblock_bwd_slab_floats(c) > 0) else None
    with _Timed(_label("ly_mlpblock_bwd_dx_describe", n, h, w, c, capi.dtype_code(x), int(slab is not None)), 2.0 * m * 18 * (c // 4) ** 2, x.element_size() * m * (3 * c + c // 4) + 4.0 * 9 * (c // 4) ** 2):
        rc = capi.lib().ly_mlpblock_bwd_dx(_p(g), _p(dy), _p(x), _p(dx), n, h, w, c, _p(wpt), _p(slab), slab.numel() if slab is not None else 0,
                                           _p(dwp if slab is not None else None), lddw, dw_ts, dw_cs, capi.dtype_code(x), capi.stream_ptr())
    if rc < 0:
        capi.check(rc, "ly_mlpblock_bwd_dx")
    return dx, rc == 0


def chan_moments(x, ldx, rows, c, f64=False, striped=False):
    """per-channel (sum x, sum x^2) over the rows of an [rows, c] matrix -> [2c]; accumulated in double stripes, folded in index order
    (float32 result unless f64: ly_rfcbam_gen_prepare takes the doubles; striped: the [STRIPES][2c] accumulators as they are — that kernel
    folds them itself)"""
    mom = new_stats(c, x.device)
    with _Timed(f"ly_chan_moments_kernel<{_tname(x)}>", 3.0 * rows * c, x.element_size() * rows * c):
        capi.check(capi.lib().ly_chan_moments(_p(x), ldx, rows, c, _p(mom), capi.dtype_code(x), capi.stream_ptr()), "ly_chan_moments")
    if striped:
        return mom
    out = torch.empty(2 * c, dtype=torch.float64, device=x.device)
    capi.check(capi.lib().ly_sum_rows_f64(_p(mom), mom.shape[0], 2 * c, _p(out), capi.stream_ptr()), "ly_sum_rows_f64")
    return out if f64 else out.float()


STRIPES = capi.STATS_STRIPES


class _StatsPool:
    """One zero fill per training step instead of one per BatchNorm pass (74 launches at lead-yolo-s): between
    `stats_pool_begin` and `stats_pool_end` (train.train_step) `new_stats` hands out slices of one buffer that was zeroed at
    `begin`.  Safe because a statistics accumulator is transient — written by one pass, read by the `ly_bn_finalize` /
    `ly_bn_bwd_coeffs` launch right after it on the same stream, never saved — and the next `begin` (same stream) is ordered
    after every reader.  Outside a begin/end pair, or when the buffer is too small (first step, a larger model), `new_stats`
    falls back to its own `torch.zeros`; the demand seen in a step sizes the buffer of the next."""
    buf = None
    off = 0
    used = 0
    need = 0
    active = False


_POOL = _StatsPool()


def stats_pool_begin(device):
    small_grads_reset()                      # (a step starts outside any backward pass: whatever is pending belongs to an aborted one)
    p = _POOL
    if p.buf is None or p.buf.device != device or p.buf.numel() < p.need:
        p.buf = torch.zeros(max(p.need, 1), dtype=torch.float32, device=device) if p.need else None
    elif p.buf is not None:
        p.buf.zero_()
    p.off = p.used = 0
    p.active = True


def stats_pool_end():
    p = _POOL
    p.active = False
    p.need = max(p.need, p.used)


_ONES = {}


def ones_f32(numel, device):
    """a shared READ-ONLY vector of ones (an identity epilogue scale): allocated once per (size, device), no fill launch per step"""
    t = _ONES.get((numel, device))
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            return torch.ones(numel, dtype=torch.float32, device=device)
        t = _ONES[(numel, device)] = torch.ones(numel, dtype=torch.float32, device=device)
    return t


def zeros_f64(numel, device):
    """zeroed float64 scratch out of the step's zero pool (an 8-byte view of 2 * numel pool floats; pool slices are 256-byte aligned)"""
    return zeros_f32(2 * numel, device).view(torch.float64)


def new_stats(nch, device):
    """zeroed striped DOUBLE accumulator for a forward statistics pass over `nch` channels: [STRIPES][2*nch] float64 (ly_stats_flush of
    csrc/ly_common.hpp adds the waves' fp32 partial sums as doubles: the batch statistics, and with them every ReLU / arg-max decision of
    a training step, are reproducible from run to run; ly_bn_finalize reads it with stats_f64 = 1)"""
    return zeros_f64(STRIPES * 2 * nch, device).view(STRIPES, 2 * nch)


def zeros_f32(numel, device):
    """zeroed fp32 scratch (transient accumulators of one launch sequence: never saved, never a parameter gradient) from the step's
    pool, so that a training step issues one fill for all of them"""
    p = _POOL
    if p.active:
        span = (numel + 63) // 64 * 64
        p.used += span
        if p.buf is not None and p.buf.device == device and p.off + span <= p.buf.numel():
            v = p.buf[p.off:p.off + numel]
            p.off += span
            return v
    return torch.zeros(numel, dtype=torch.float32, device=device)


def bn_finalize(bn, stats, nch, count, n=None, c_off=0, pad_to=0, want_stats=False, into=None):
    """Train-mode BatchNorm2d from the striped sums of a statistics pass, ONE launch (ly_bn_finalize): returns
    (scale, shift) of y = x*scale + shift [+ (mean, invstd)], updates running_mean/var/num_batches_tracked in place.
    into = (scale, shift, mean, invstd): contiguous fp32 [n] destinations (slices of a wider vector: two BatchNorms over one stacked output)."""
    n = nch if n is None else n
    dev = stats.device
    size = max(n, pad_to)
    if into is not None:
        scale, shift, mean, invstd = into
        want_stats = True
    else:
        if size > n:                 # zero-padded tails (MLPBlock's hidden tiles): out of the step's zero pool, no fill launches
            scale, shift = zeros_f32(size, dev), zeros_f32(size, dev)
        else:
            scale, shift = torch.empty(size, dtype=torch.float32, device=dev), torch.empty(size, dtype=torch.float32, device=dev)
        mean = torch.empty(n, dtype=torch.float32, device=dev) if want_stats else None
        invstd = torch.empty(n, dtype=torch.float32, device=dev) if want_stats else None
    track = bn.track_running_stats and bn.running_mean is not None
    if bn.weight is not None and bn.weight.dtype != torch.float32:
        raise NotImplementedError("train-mode BatchNorm needs float32 parameters and buffers: train under torch.autocast (fp32 master "
                                  "weights, as the reference does), not with a .half()/.bfloat16() model")
    if track and bn.momentum is None:
        raise NotImplementedError("BatchNorm with momentum=None (cumulative average) is not built")
    if track:
        from . import pack
        pack.touch()                     # running statistics are written by the kernel: eval-mode folded caches must refresh
    if stats.dtype not in (torch.float32, torch.float64):
        raise TypeError("bn_finalize: statistics must be float32 or float64")
    capi.check(capi.lib().ly_bn_finalize(_p(stats), int(stats.dtype == torch.float64), stats.shape[0], nch, c_off, n, float(count), _p(bn.weight), _p(bn.bias), None, float(bn.eps),
                                         float(bn.momentum or 0.0), _p(bn.running_mean if track else None), _p(bn.running_var if track else None),
                                         _p(bn.num_batches_tracked if track else None), _p(scale), _p(shift), _p(mean), _p(invstd),
                                         capi.stream_ptr()), "ly_bn_finalize")
    return (scale, shift, mean, invstd) if want_stats else (scale, shift)


def _bn_train_args(bn):
    """(gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked) of a train-mode BatchNorm for the finalize kernels"""
    track = bn.track_running_stats and bn.running_mean is not None
    if bn.weight is not None and bn.weight.dtype != torch.float32:
        raise NotImplementedError("train-mode BatchNorm needs float32 parameters and buffers: train under torch.autocast (fp32 master "
                                  "weights, as the reference does), not with a .half()/.bfloat16() model")
    if track and bn.momentum is None:
        raise NotImplementedError("BatchNorm with momentum=None (cumulative average) is not built")
    if track:
        from . import pack
        pack.touch()                     # running statistics are written by the kernel: eval-mode folded caches must refresh
    return (_p(bn.weight), _p(bn.bias), float(bn.eps), float(bn.momentum or 0.0), _p(bn.running_mean if track else None),
            _p(bn.running_var if track else None), _p(bn.num_batches_tracked if track else None))


def bn_finalize_pair(bn1, bn2, stats, c_half, count, v):
    """bn_finalize of two BatchNorms over one stacked [2 c_half]-channel statistics array in ONE launch; v: fp32 [4, 2 c_half] that
    receives scale, shift, mean, invstd"""
    if stats.dtype not in (torch.float32, torch.float64) or v.dtype != torch.float32 or not v.is_contiguous() or tuple(v.shape) != (4, 2 * c_half):
        raise TypeError("bn_finalize_pair: float32 / float64 statistics and a contiguous float32 [4, 2 c_half] result expected")
    capi.check(capi.lib().ly_bn_finalize_pair(_p(stats), int(stats.dtype == torch.float64), stats.shape[0], c_half, float(count), *_bn_train_args(bn1),
                                              *_bn_train_args(bn2), _p(v[0]), _p(v[1]), _p(v[2]), _p(v[3]), capi.stream_ptr()), "ly_bn_finalize_pair")


def bn_bwd_coeffs_pair(sums0, sums1, c_half, count, v, targets, coef):
    """bn_bwd_coeffs (train) of the same two units in ONE launch.  v: [4, 2 c_half] of bn_finalize_pair; targets = ((dgamma0, dbeta0),
    (dgamma1, dbeta1)): fp32 [c_half] tensors the kernel ADDS into; coef: fp32 [3, 2 c_half] that receives alpha, kappa, lambda"""
    if sums0.dtype != sums1.dtype or sums0.shape != sums1.shape or sums0.dim() != 2:
        raise TypeError("bn_bwd_coeffs_pair: two striped sum arrays of one shape expected")
    (g0, b0), (g1, b1) = targets
    capi.check(capi.lib().ly_bn_bwd_coeffs_pair(_p(sums0), _p(sums1), int(sums0.dtype == torch.float64), sums0.shape[0], c_half, float(count), _p(v[0]), _p(v[2]),
                                                _p(v[3]), _p(g0), _p(b0), _p(g1), _p(b1), _p(coef[0]), _p(coef[1]), _p(coef[2]), capi.stream_ptr()),
               "ly_bn_bwd_coeffs_pair")


def bn_bwd_coeffs(sums, n, count, a, mean, invstd, train, dgamma=None, dbeta=None, transpose=None, into=None):
    """(dgamma, dbeta, alpha, kappa, lambda) from (striped) sums [.., 2n] of ly_bnact_bwd_reduce, ONE launch.  dgamma / dbeta given:
    the kernel ADDS into them (a parameter's persistent gradient storage, see GradSink) and None is returned in their place.
    transpose = (A, B): the sums' channels are in [A][B] order, dgamma / dbeta in [B][A] (generate BatchNorm of RFCBAMConv k = 3)."""
    dev = sums.device
    stripes = sums.shape[0] if sums.dim() == 2 else 1
    # into = (alpha, kappa, lambda): contiguous fp32 [n] destinations (slices of wider vectors: two units side by side)
    out = torch.empty(5 if into is None else 2, n, dtype=torch.float32, device=dev)
    direct = dgamma is not None and dbeta is not None
    if not direct:
        out[:2].zero_()
    capi.check(capi.lib().ly_bn_bwd_coeffs(_p(sums), int(sums.dtype == torch.float64), stripes, n, float(count), _p(a), _p(mean), _p(invstd), int(train), _p(dgamma if direct else out[0]),
                                           _p(dbeta if direct else out[1]), *[_p(t) for t in (into if into is not None else (out[2], out[3], out[4]))],
                                           *((transpose if direct else None) or (0, 0)), capi.stream_ptr()), "ly_bn_bwd_coeffs")
    al, ka, la = into if into is not None else (out[2], out[3], out[4])
    return (None if direct else out[0]), (None if direct else out[1]), al, ka, la


class GradSink:
    """Where the backward kernels put parameter gradients.  Default (no sink installed): fresh tensors handed to autograd, which
    accumulates them into `.grad` — one extra launch per parameter and step, plus the zero fill of every fresh tensor.  With a sink
    (optim.FusedSGD installs one: its persistent, step-zeroed gradient storage) ly_wgrad / ly_bn_bwd_coeffs ADD straight into
    `param.grad` and the autograd function returns None for that parameter; `grad_done(param)` then stands in for the post-accumulate
    hook (ddp.GradReducer launches a bucket's all-reduce from it).
    The invariant whoever fills `targets` keeps (optim's fused optimisers, over their own storage or ddp.GradReducer's bucket views): a
    target has its parameter's SHAPE, is fp32 and is contiguous — or, for a k x k convolution weight, tap-major (`tap_major`).  Which of
    the two layouts a kernel can add into is a fact about the kernel: its caller names it (OWN / CONTIGUOUS / TAP_ROWS) to ParamGrad,
    the one place that decides between the sink and a fresh tensor."""

    def __init__(self):
        self.targets = {}          # id(param) -> gradient tensor (see the invariant above)
        self.writes = 0            # bumped whenever a backward kernel is handed a target (or a captured backward is replayed): the
                                   # optimiser's zero_grad() compares it with the value at its last step() to know whether the storage is dirty

    def is_target(self, t):
        """t is (a view from the start of) one of the sink's persistent gradient tensors"""
        if getattr(self, "_ptr_src", None) is not self.targets or len(self.targets) != self._nptr:      # (the optimiser assigns a whole new dict)
            self._ptrs, self._nptr, self._ptr_src = {v.data_ptr() for v in self.targets.values()}, len(self.targets), self.targets
        return t.data_ptr() in self._ptrs

    def target(self, p):
        if p is None or not torch.is_tensor(p) or not p.requires_grad:
            return None                         # (a parameter frozen since the optimiser built its table: autograd drops what is returned for it)
        t = self.targets.get(id(p))
        if t is not None and p.grad is not t:
            return None                         # someone re-assigned .grad: fall back to autograd for this one
        if t is not None:
            self.writes += 1
        return t



SINK = None
GRAD_DEFER_LISTENERS = []          # callables(param): told that a directly-written gradient will be announced at the end of the backward pass
GRAD_LISTENERS = []                # callables(param): told when a directly-written gradient is complete (ddp.GradReducer)


def grad_target(p):
    return SINK.target(p) if SINK is not None else None


def grad_done(p):
    """the directly-written gradient of parameter p is complete AND its launches are in the stream.  A weight gradient that still waits in the
    deferral queue (_WgradQueue) is announced when its group has been launched instead; the listeners are told now that it comes later."""
    if GRAD_LISTENERS and _WgradQueue.items and SINK is not None:
        t = SINK.targets.get(id(p))
        # a waiting problem covers the address RANGE [dw, dw + N * lddw): the stacked cv1 / cv2 problem of a ConvBnActPair (N = 2 c_) also writes
        # its partner's storage, which starts 4 * numel bytes behind dw — a pointer-equality match announced that partner early
        if t is not None and any(lo <= t.data_ptr() < hi for lo, hi in map(_wgrad_span, _WgradQueue.items)):
            if all(prm is not p for prm, _ in _WgradQueue.notify):
                _WgradQueue.notify.append((p, t.data_ptr()))
                for fn in GRAD_DEFER_LISTENERS:
                    fn(p)
            return
    for fn in GRAD_LISTENERS:
        fn(p)


def coordatt_conv1_stats(pool, positions, c, mip, w1, b1):
    st = zeros_f64(2 * mip, pool.device)
    capi.check(capi.lib().ly_coordatt_conv1_stats(_p(pool), positions, c, mip, _p(w1), _p(b1), _p(st), capi.stream_ptr()),
               "ly_coordatt_conv1_stats")
    return st


def rfcbam_gen_prepare(x, ldx, n, h, w, c, k, s, gen_w, bn):
    """Train-mode `generate` BatchNorm of RFCBAMConv in two launches: the moment kernel over x, then ly_rfcbam_gen_prepare (batch
    statistics, running-stat update, scale / shift in both index orders and the folded weights in the kernels' LDS orders).
    Returns dict(gs, gb, gmean, ginv [c*kk + t order], ag, bg, gmean_tc, ginv_tc [t*c + c order], a1 (k=1), wq_stats, wq_main (k=3))."""
    kk = k * k
    dev = x.device
    if k == 3:
        mom = zeros_f64(54 * c, dev)
        args = (_p(x), ldx, n, h, w, c, s, _p(mom), capi.dtype_code(x))
        with _Timed(_label("ly_rfcbam_tap_moments_describe", *args), 108.0 * n * h * w * c / (s * s), x.element_size() * n * h * w * c):
            capi.check(capi.lib().ly_rfcbam_tap_moments(*args, capi.stream_ptr()), "ly_rfcbam_tap_moments")
        ho, wo = rf_out_hw(h, w, 3, s)
        count = n * ho * wo
    else:
        mom = chan_moments(x, ldx, n * h * w, c, striped=True)
        count = n * h * w
    g = c * kk
    out8 = torch.empty(8, g, dtype=torch.float32, device=dev)
    a1 = torch.empty(c, dtype=torch.float32, device=dev) if k == 1 else None
    cps, cpm = (c + 31) // 32 * 32, (c + 15) // 16 * 16
    wqs = torch.empty(cps * 90, dtype=torch.float32, device=dev) if k == 3 else None
    wqm = torch.empty(cpm * 90, dtype=torch.float32, device=dev) if k == 3 else None
    wqc = torch.empty(c * 100, dtype=torch.float32, device=dev) if (k == 3 and c % 32 == 0) else None
    if bn.weight.dtype != torch.float32:
        raise NotImplementedError("train-mode BatchNorm needs float32 parameters and buffers")
    track = bn.track_running_stats and bn.running_mean is not None
    capi.check(capi.lib().ly_rfcbam_gen_prepare(_p(mom), c, k, _p(gen_w.detach()), _p(bn.weight.detach()), _p(bn.bias.detach()), float(bn.eps),
                                                float(bn.momentum or 0.0), float(count), _p(bn.running_mean if track else None),
                                                _p(bn.running_var if track else None), _p(bn.num_batches_tracked if track else None), _p(out8),
                                                _p(a1), _p(wqs), _p(wqm), _p(wqc), mom.shape[0] if k == 1 else 1, capi.stream_ptr()), "ly_rfcbam_gen_prepare")
    from . import pack
    pack.touch()                                   # running statistics written behind torch's version counters
    return dict(gs=out8[0], gb=out8[1], gmean=out8[2], ginv=out8[3], ag=out8[4], bg=out8[5], gmean_tc=out8[6], ginv_tc=out8[7], a1=a1,
                wq_stats=wqs, wq_main=wqm, wq_c=wqc)


# ---- backward building blocks (training step) --------------------------------------------------------
def bnact_fwd(u, ldu, rows, c, a, b, act, y, ldy):
    with _Timed(f"ly_bnact_fwd_kernel<{_tname(u)}, {act}>", 4.0 * rows * c, 2.0 * u.element_size() * rows * c):
        capi.check(capi.lib().ly_bnact_fwd(_p(u), ldu, rows, c, _p(a), _p(b), act, _p(y), ldy, capi.dtype_code(u), capi.stream_ptr()), "ly_bnact_fwd")


def bnact_bwd_reduce(dy, lddy, u, ldu, rows, c, a, b, act):
    sums = new_stats(c, u.device)                 # double accumulators: the coefficients of du, and with them the whole activation-gradient chain, are reproducible
    with _Timed(f"ly_bnact_bwd_reduce_kernel<{_tname(u)}, {act}>", 6.0 * rows * c, 2.0 * u.element_size() * rows * c):
        capi.check(capi.lib().ly_bnact_bwd_reduce(_p(dy), lddy, _p(u), ldu, rows, c, _p(a), _p(b), act, _p(sums), capi.dtype_code(u),
                                                  capi.stream_ptr()), "ly_bnact_bwd_reduce")
    return sums


def bnact_bwd_apply(dy, lddy, u, ldu, rows, c, a, b, act, alpha, kappa, lam, du, lddu):
    with _Timed(f"ly_bnact_bwd_apply_kernel<{_tname(u)}, {act}>", 8.0 * rows * c, 3.0 * u.element_size() * rows * c):
        capi.check(capi.lib().ly_bnact_bwd_apply(_p(dy), lddy, _p(u), ldu, rows, c, _p(a), _p(b), act, _p(alpha), _p(kappa), _p(lam),
                                                 _p(du), lddu, capi.dtype_code(u), capi.stream_ptr()), "ly_bnact_bwd_apply")


def bnact_bwd_reduce_pair(dy1, lddy1, dy2, lddy2, csplit, u, ldu, rows, c, a, b, act):
    """both units of a stacked pair in one pass -> (sums1, sums2)"""
    s1, s2 = new_stats(csplit, u.device), new_stats(c - csplit, u.device)
    with _Timed(f"ly_bnact_bwd_reduce_kernel<{_tname(u)}, {act}>", 6.0 * rows * c, 2.0 * u.element_size() * rows * c):
        capi.check(capi.lib().ly_bnact_bwd_reduce_pair(_p(dy1), lddy1, _p(dy2), lddy2, csplit, _p(u), ldu, rows, c, _p(a), _p(b), act, _p(s1), _p(s2),
                                                       capi.dtype_code(u), capi.stream_ptr()), "ly_bnact_bwd_reduce_pair")
    return s1, s2


def bnact_bwd_apply_pair(dy1, lddy1, dy2, lddy2, csplit, u, ldu, rows, c, a, b, act, alpha, kappa, lam, du, lddu):
    with _Timed(f"ly_bnact_bwd_apply_kernel<{_tname(u)}, {act}>", 8.0 * rows * c, 3.0 * u.element_size() * rows * c):
        capi.check(capi.lib().ly_bnact_bwd_apply_pair(_p(dy1), lddy1, _p(dy2), lddy2, csplit, _p(u), ldu, rows, c, _p(a), _p(b), act, _p(alpha), _p(kappa),
                                                      _p(lam), _p(du), lddu, capi.dtype_code(u), capi.stream_ptr()), "ly_bnact_bwd_apply_pair")


def wgrad(*, M, H, W, N, du, lddu, x, ldx, Hin, Win, Cin, dw, lddw, ks=1, stride=1, pad=0, nchw=False, up2=False, du_off=0, x_off=0,
          dw_off=0, dw_ts=None, dw_cs=1, n_valid=None, c_valid=None, x_scale=None, x_shift=None, _now=False):
    """dw[n][tap*dw_ts + c*dw_cs] += sum_pixels du[p][n] * x[src(p, tap)][c] for n < n_valid, c < c_valid; *_off are element offsets
    into the tensors.  Defaults: packed rows (dw_ts = Cin, dw_cs = 1), everything valid.  x_scale / x_shift (fp32 [Cin], plain-row 1x1
    problems): x is read as max(x*x_scale + x_shift, 0)."""
    q = dict(M=M, H=H, W=W, N=N, du=du, lddu=lddu, x=x, ldx=ldx, Hin=Hin, Win=Win, Cin=Cin, dw=dw, lddw=lddw, ks=ks, stride=stride,
             pad=pad, nchw=nchw, up2=up2, du_off=du_off, x_off=x_off, dw_off=dw_off, dw_ts=dw_ts, dw_cs=dw_cs, n_valid=n_valid,
             c_valid=c_valid, x_scale=x_scale, x_shift=x_shift)
    if not _now and _wgrad_deferrable(q):
        return _wgrad_enqueue(q)
    P = _wgrad_params(**q)
    with _Timed(_label("ly_wgrad_describe", ctypes.byref(P), 1), 2.0 * M * N * ks * ks * Cin, x.element_size() * M * (N + Cin) + 4.0 * N * ks * ks * Cin):
        capi.check(capi.lib().ly_wgrad(ctypes.byref(P), capi.stream_ptr()), "ly_wgrad")


def _wgrad_params(*, M, H, W, N, du, lddu, x, ldx, Hin, Win, Cin, dw, lddw, ks=1, stride=1, pad=0, nchw=False, up2=False, du_off=0, x_off=0,
                  dw_off=0, dw_ts=None, dw_cs=1, n_valid=None, c_valid=None, x_scale=None, x_shift=None):
    def at(t, off):
        return ctypes.c_void_p(t.data_ptr() + t.element_size() * off)
    if du.dtype != x.dtype:
        raise capi.HipLibraryError(f"wgrad: du ({du.dtype}) and x ({x.dtype}) must share one storage dtype")
    if (x_scale is None) != (x_shift is None):
        raise ValueError("wgrad: x_scale and x_shift come together")
    if x_scale is not None and (x_scale.dtype != torch.float32 or x_shift.dtype != torch.float32 or x_scale.numel() < Cin or x_shift.numel() < Cin):
        raise ValueError("wgrad: x_scale / x_shift must be float32 vectors of at least Cin elements")
    ws = wgrad_workspace(x.device)
    return capi.LyWgradParams(M, H, W, N, at(du, du_off), lddu, at(x, x_off), ldx, Hin, Win, Cin, ks, stride, pad, int(nchw), int(up2),
                              at(dw, dw_off), lddw, capi.dtype_code(x), Cin if dw_ts is None else dw_ts, dw_cs, N if n_valid is None else n_valid,
                              Cin if c_valid is None else c_valid, _p(x_scale), _p(x_shift), _p(ws), ws.numel() if ws is not None else 0)


WGRAD_WS_FLOATS = 24 << 20          # 96 MB of fp32 scratch per device: the partial tiles of one weight-gradient launch (largest: 38 MB)
_WGRAD_WS = {}


def wgrad_workspace(device):
    """Per-device scratch the weight-gradient kernels park their per-chunk partial tiles in (LyWgradParams.ws).  Allocated ONCE (a captured
    hipGraph keeps its address; every launch overwrites what it reads back in the same launch sequence, stream-ordered), never zeroed.
    ONE buffer per device: weight-gradient launches of a device are expected on one stream at a time (the training step's); two training
    loops on different streams of the same device in one process must set WGRAD_WS_FLOATS = 0 (atomic accumulation) for one of them."""
    if WGRAD_WS_FLOATS <= 0:
        return None
    ws = _WGRAD_WS.get(device)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            return None                               # (a first use inside a capture: this launch keeps the atomic path)
        ws = _WGRAD_WS[device] = torch.empty(WGRAD_WS_FLOATS, dtype=torch.float32, device=device)
    return ws


def _wgrad_groupable(q, dtype):
    return (q.get("ks", 1) == 1 and q.get("stride", 1) == 1 and q.get("pad", 0) == 0 and not q.get("nchw") and not q.get("up2")
            and q["N"] > 64 and q["N"] % 4 == 0 and q["Cin"] % 4 == 0 and q["lddu"] % 4 == 0 and q["ldx"] % 4 == 0
            and q["Hin"] == q["H"] and q["Win"] == q["W"] and q["x"].dtype == dtype)


class _WgradQueue:
    """Weight gradients are leaves of the backward pass: a plain-row problem of the 128 x 128 tile class whose destination is the gradient
    sink's persistent storage need not launch where the backward reaches it.  Such problems wait here (operands kept alive) and leave four
    at a time as ONE grouped launch + ONE fold (ly_wgrad_group) — the small-map problems (25600 pixels: ~30 us each alone, a few blocks per CU
    walking long pixel runs) share the chip — and the rest leaves when the pass ends (engine callback).  Program order fixes the grouping:
    the step stays bit-reproducible and a captured step replays the same launches.  `grad_done(param)` of a gradient that still waits here
    is passed on to the listeners (ddp.GradReducer) when its group has been launched (`notify`).  Narrow problems (Cin <= 64, or a column slice of a wider gradient) stay
    out: the group runs every problem on the 128 x 128 tile, and with the two K = 40 / 80 concat-slice problems of the neck in the groups
    the step went from 10.01 to 10.21 ms."""
    items = []
    notify = []         # (param, gradient data_ptr): grad_done arrived while the gradient's problem was waiting
    task = -1


WGRAD_DEFER = True                  # a module constant (tests monkeypatch it): not reachable from the environment
WGRAD_GROUP_MAX = 4
WGRAD_DEFER_MAX_MACS = 4 << 30      # M * N * K: a larger problem fills the chip alone, and the grouped kernel costs ~15 % more per unit of work than the
                                    # single-problem one (lead-yolo-l bs=16 1280x1280 with all its plain-row problems in groups: 33.96 -> 34.96 ms per step;
                                    # lead-yolo-s: every deferred problem is below 3.4 G)


def _wgrad_deferrable(q):
    return (WGRAD_DEFER and SINK is not None and q["x"].dtype == torch.bfloat16 and _wgrad_groupable(q, torch.bfloat16)
            and q["Cin"] > 64 and q["M"] * q["N"] * q["Cin"] <= WGRAD_DEFER_MAX_MACS and q.get("dw_off", 0) == 0 and SINK.is_target(q["dw"]) and _graph_task() >= 0)


def _wgrad_span(q):
    """byte range of the gradient storage a queued problem adds into"""
    lo = q["dw"].data_ptr() + 4 * q.get("dw_off", 0)
    return lo, lo + 4 * q["N"] * q["lddw"]


def _wgrad_enqueue(q):
    """A queued problem keeps REFERENCES to du / x / x_scale / x_shift and reads them when its group launches (after up to three more problems
    have collected, or when the backward pass ends): the caller must not write those tensors in place after ops.wgrad returns.  Their torch
    version counters are recorded here and checked at the launch; two problems adding into overlapping gradient storage never wait together
    (the group flushes them through one fold: the second would be lost / the order undefined)."""
    task = _graph_task()
    if _WgradQueue.task != task:
        _WgradQueue.items, _WgradQueue.notify, _WgradQueue.task = [], [], task    # (leftovers of a backward pass that raised are dropped with it)
        torch.autograd.Variable._execution_engine.queue_callback(wgrad_flush)
    lo, hi = _wgrad_span(q)
    if any(l2 < hi and lo < h2 for l2, h2 in map(_wgrad_span, _WgradQueue.items)):
        wgrad_flush(final=False)               # shared weights: the earlier problem leaves before this one is queued
    q["_versions"] = tuple(t._version for t in (q["du"], q["x"], q.get("x_scale"), q.get("x_shift")) if t is not None)
    _WgradQueue.items.append(q)
    # under a gradient listener (ddp.GradReducer) a waiting gradient holds back its whole bucket's exchange: leave in pairs there
    # (tools/dp_overlap_probe.py: with fours a 1.3 MB bucket was released at 77 % of the backward instead of 33 %)
    if len(_WgradQueue.items) >= (2 if GRAD_LISTENERS else WGRAD_GROUP_MAX):
        wgrad_flush(final=False)


def wgrad_flush(final=True):
    """launch what waits in the deferral queue (end of the backward pass, or four problems collected)"""
    items, _WgradQueue.items = _WgradQueue.items, []
    if final:
        _WgradQueue.task = -1
    for q in items:
        now = tuple(t._version for t in (q["du"], q["x"], q.get("x_scale"), q.get("x_shift")) if t is not None)
        if now != q.pop("_versions", now):
            raise RuntimeError("ops.wgrad: an operand of a deferred weight gradient was written in place before its launch (du / x / x_scale / "
                               "x_shift must stay untouched until the group leaves: see _wgrad_enqueue)")
    if len(items) == 1:
        wgrad(_now=True, **items[0])
    elif items:
        wgrad_group(items, _now=True)
    if _WgradQueue.notify:
        spans = [_wgrad_span(q) for q in _WgradQueue.items]
        waits = lambda ptr: any(lo <= ptr < hi for lo, hi in spans)
        ready = [prm for prm, ptr in _WgradQueue.notify if not waits(ptr)]
        _WgradQueue.notify = [(prm, ptr) for prm, ptr in _WgradQueue.notify if waits(ptr)]
        for prm in ready:
            for fn in GRAD_LISTENERS:
                fn(prm)


def wgrad_group(problems, _now=False):
    """Several independent weight gradients (each a dict of `wgrad` arguments) in ONE launch when all are plain-row 1x1 problems of the
    128 x 128 tile class (ly_wgrad_group: N > 64, vector-friendly widths, no gather, at most 4); otherwise one `wgrad` each."""
    if not _now and all(_wgrad_deferrable(q) for q in problems):
        for q in problems:
            _wgrad_enqueue(q)
        return
    if not (2 <= len(problems) <= 4) or not all(_wgrad_groupable(q, problems[0]["x"].dtype) for q in problems):
        for q in problems:
            wgrad(_now=_now, **q)
        return
    arr = (capi.LyWgradParams * len(problems))(*[_wgrad_params(**q) for q in problems])
    x0 = problems[0]["x"]
    with _Timed(_label("ly_wgrad_describe", arr, len(problems)), sum(2.0 * q["M"] * q["N"] * q["Cin"] for q in problems),
                sum(x0.element_size() * q["M"] * (q["N"] + q["Cin"]) + 4.0 * q["N"] * q["Cin"] for q in problems)):
        capi.check(capi.lib().ly_wgrad_group(arr, len(problems), capi.stream_ptr()), "ly_wgrad_group")


def tune_wgrad1(on):
    """0 sends the plain-row 1x1 bf16 weight gradients back to the register-transposing tiled kernel (A/B timing, the equivalence tests);
    returns the previous setting"""
    return capi.lib().ly_tune_wgrad1(int(bool(on)))


def sum_rows(t, out=None, accumulate=False):
    """sum over dim 0 of a contiguous fp32 tensor [R, ...] -> [...] (ly_sum_rows: fixed order, no atomics, no ATen reduction scratch)"""
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError("sum_rows: contiguous float32 tensor expected")
    r = t.shape[0]
    c = t.numel() // r
    if out is None:
        out = torch.empty(t.shape[1:], dtype=torch.float32, device=t.device)
    capi.check(capi.lib().ly_sum_rows(_p(t), r, c, c, _p(out), int(accumulate), capi.stream_ptr()), "ly_sum_rows")
    return out


def up2_bwd(d, ldd, n, hs, ws, c):
    out = empty_nhwc(n, c, hs, ws, d)
    capi.check(capi.lib().ly_up2_bwd(_p(d), ldd, n, hs, ws, c, _p(out), c, capi.dtype_code(d), capi.stream_ptr()), "ly_up2_bwd")
    return out


def unpatch(g, n, ho, wo, c, ks, h, w):
    """g [n*ho*wo, ks*ks*c] -> dx [n, c, h, w] (NHWC storage); rows/cols beyond ks*ho / ks*wo stay zero."""
    exact = (h == ho * ks and w == wo * ks)
    if not exact:
        raise NotImplementedError("patch-gather backward needs H, W divisible by the patch size")
    dx = empty_nhwc(n, c, h, w, g)
    capi.check(capi.lib().ly_unpatch(_p(g), n, ho, wo, c, ks, _p(dx), capi.dtype_code(g), capi.stream_ptr()), "ly_unpatch")
    return dx


def patch4_rows_u8(img, dtype):
    """uint8 NCHW image [n, c, h, w] -> rows [n*h/4*w/4, 16*c] of `dtype` holding the integer pixel values (PatchEmbed weight gradient)"""
    n, c, h, w = img.shape
    if img.dtype != torch.uint8 or not img.is_contiguous() or h % 4 or w % 4:
        raise ValueError("patch4_rows_u8: contiguous uint8 NCHW image with H, W multiples of 4 expected")
    rows = torch.empty((n * (h // 4) * (w // 4), 16 * c), dtype=dtype, device=img.device)
    capi.check(capi.lib().ly_patch4_rows_u8(_p(img), n, c, h, w, _p(rows), capi.dtype_code(rows), capi.stream_ptr()), "ly_patch4_rows_u8")
    return rows


def patch4_wgrad_u8_ok(img, du, n_out):
    """ly_patch4_wgrad_u8 applies: contiguous uint8 RGB batch with H, W multiples of 4, bf16 gradient rows of a vector-friendly width, and the
    weight-gradient workspace of the device holds the per-block partials"""
    n, c, h, w = img.shape
    ws = wgrad_workspace(img.device)
    return (img.dtype == torch.uint8 and img.is_contiguous() and c == 3 and h % 4 == 0 and w % 4 == 0 and du.dtype == torch.bfloat16
            and n_out % 8 == 0 and 8 <= n_out <= 64 and du.data_ptr() % 16 == 0 and ws is not None and ws.numel() >= 1536 * n_out * 48
            and n * (h // 4) * (w // 4) < (1 << 24))


def patch4_wgrad_u8(img, du, lddu, n_out, dw, scale):
    """dw [n_out][48] (fp32) += scale * sum over output pixels of du (x) the 4 x 4 patches of the uint8 image (csrc/ly_patch4.hip): the
    PatchEmbed weight gradient without the space-to-depth rows"""
    n, c, h, w = img.shape
    m = n * (h // 4) * (w // 4)
    ws = wgrad_workspace(img.device)
    args = (_p(img), n, c, h, w, _p(du), lddu, n_out, float(scale), _p(ws), ws.numel(), _p(dw), capi.dtype_code(du))
    with _Timed(_label("ly_patch4_wgrad_u8_describe", *args), 2.0 * m * n_out * 48, 1.0 * n * c * h * w + 2.0 * m * n_out + 4.0 * n_out * 48):
        capi.check(capi.lib().ly_patch4_wgrad_u8(*args, capi.stream_ptr()), "ly_patch4_wgrad_u8")


def coordatt_gate_bwd(dout, x, ldx, n, h, w, c, a_h, a_w, ldd=None):
    """dout: rows of the incoming gradient with row stride ldd (default c: dense) — a channel slice of a wider gradient is read in place"""
    ldd = c if ldd is None else ldd
    dx = empty_nhwc(n, c, h, w, x)
    # partial sums per column slab (da_h) / row band (da_w), plain stores, folded in index order: no atomics (csrc/ly_coordatt.hip)
    groups = 256 // (c // 4)
    slabs, bands = -(-w // (groups * 8)), -(-h // 8)
    ph = torch.empty((slabs, n * h * c), dtype=torch.float32, device=dout.device)
    pw = torch.empty((bands, n * w * c), dtype=torch.float32, device=dout.device)
    with _Timed(f"ly_coordatt_gate_bwd_kernel<{_tname(x)}>", 6.0 * n * h * w * c, 3.0 * x.element_size() * n * h * w * c):
        capi.check(capi.lib().ly_coordatt_gate_bwd(_p(dout), ldd, _p(x), ldx, n, h, w, c, _p(a_h), _p(a_w), _p(dx), c, _p(ph), _p(pw), bands, slabs,
                                                   capi.dtype_code(x), capi.stream_ptr()), "ly_coordatt_gate_bwd")
    da_h = (sum_rows(ph) if slabs > 1 else ph[0]).view(n, h, c)
    da_w = (sum_rows(pw) if bands > 1 else pw[0]).view(n, w, c)
    return dx, da_h, da_w


def pool_hw_bwd(gp, n, h, w, c, dtype=torch.float32, into=None):
    """into: a dense NHWC gradient the pool gradient is ADDED to in place (one pass instead of write + add)"""
    dx = into if into is not None else empty_nhwc(n, c, h, w, gp, dtype=dtype)
    capi.check(capi.lib().ly_pool_hw_bwd(_p(gp), n, h, w, c, _p(dx), c, 1 if into is not None else 0, capi.dtype_code(dx), capi.stream_ptr()),
               "ly_pool_hw_bwd")
    return dx


def maxpool_bwd(x, x_off, ldx, dy, dy_off, lddy, n, h, w, c, k, dx, dx_off, lddx):
    """x: the pooled map (storage dtype); dy / dx: ALWAYS float32 (the gradient is accumulated with float atomics)"""
    at = lambda t, off: ctypes.c_void_p(t.data_ptr() + t.element_size() * off)
    assert dy.dtype == torch.float32 and dx.dtype == torch.float32
    capi.check(capi.lib().ly_maxpool_bwd(at(x, x_off), ldx, at(dy, dy_off), lddy, n, h, w, c, k, at(dx, dx_off), lddx, capi.dtype_code(x),
                                         capi.stream_ptr()), "ly_maxpool_bwd")


def sppf_bwd(buf, ldb, d, ldd, n, h, w, c, k):
    """the three chained pools' backward in ONE launch (csrc/ly_sppf.hip), map and routing in LDS: buf = the forward's [y | m(y) | m(m(y)) |
    m(m(m(y)))] rows, d its gradient in the same dtype.  Returns dy, or None where the map does not fit (the entry's code 1)"""
    out = empty_nhwc(n, c, h, w, buf)
    rc = capi.lib().ly_sppf_bwd(_p(buf), ldb, _p(d), ldd, n, h, w, c, k, _p(out), c, capi.dtype_code(buf), capi.stream_ptr())
    if rc == 0:
        return out
    if rc != 1:
        capi.check(rc, "ly_sppf_bwd")
    return None


def maxpool_arg(x, ldx, n, h, w, c, k, arg, lda):
    """arg (uint8 rows of lda): per window and channel the tap of its first maximum in row-major scan order, ATen's rule"""
    capi.check(capi.lib().ly_maxpool_arg(_p(x), ldx, n, h, w, c, k, _p(arg), lda, capi.dtype_code(x), capi.stream_ptr()), "ly_maxpool_arg")


def maxpool_gather(arg, arg_off, lda, d_up, ldu, d_own, own_off, ldd, n, h, w, c, k, out, ldo):
    """out = d_own + the d_up (float32) of every window that routes to the position (arg: ly_maxpool_arg's); arg / d_own from a column offset"""
    at = lambda t, off: ctypes.c_void_p(t.data_ptr() + t.element_size() * off)
    capi.check(capi.lib().ly_maxpool_gather(at(arg, arg_off), lda, _p(d_up), ldu, at(d_own, own_off), ldd, capi.dtype_code(d_own), n, h, w, c, k,
                                            _p(out), ldo, capi.dtype_code(out), capi.stream_ptr()), "ly_maxpool_gather")


def mlp_dx(dy, g, t, ldt, rows, c, c4, dx):
    """MLPBlock backward, last step: dx = dy + g, the first c4 channels dy + t (t rows of ldt)"""
    capi.check(capi.lib().ly_mlp_dx(_p(dy), _p(g), _p(t), ldt, rows, c, c4, _p(dx), capi.dtype_code(dy), capi.stream_ptr()), "ly_mlp_dx")


# ---- autoanchor (csrc/ly_anchors.hip; lead-yolo_amd/anchors.py holds the host loops) ------------------------------------------------
ANCHOR_NA_MAX, ANCHOR_SLICES_MAX = capi.ANCHOR_NA_MAX, capi.ANCHOR_SLICES_MAX


def anchor_slices(n, slices=None):
    """label slices of a launch: one per 1024 labels, at most 64, unless the caller names a count"""
    s = min(64, max(1, -(-int(n) // 1024))) if slices is None else int(slices)
    if not 1 <= s <= ANCHOR_SLICES_MAX:
        raise ValueError(f"slices={s} outside [1, {ANCHOR_SLICES_MAX}]")
    return s


def anchor_wh(labels, img, shapes, scale=None):
    """wh [n, 2] float32 = labels[:, 3:5] * (shapes[img] * scale[img]), float64 products rounded once (labels [n, 5] float64, img [n] int32,
    shapes [n_img, 2] float64 (w, h), scale None or [n_img] float64; all on the labels' device)"""
    n = labels.shape[0]
    wh = torch.empty((n, 2), dtype=torch.float32, device=labels.device)
    capi.check(capi.lib().ly_anchor_wh(_p(labels), _p(img), n, _p(shapes), shapes.shape[0], _p(scale), _p(wh), capi.stream_ptr()), "ly_anchor_wh")
    return wh


def anchor_metric(wh, k, thr, slices=None):
    """-> [G, 3] float64: (sum best * (best > 1/thr), count best > 1/thr, count x > 1/thr) of every candidate set k [G, na, 2] over wh [n, 2]"""
    n, (g, na, _) = wh.shape[0], k.shape
    s = anchor_slices(n, slices)
    part = torch.empty((s, 3 * g), dtype=torch.float64, device=wh.device)
    with _Timed("ly_anchor_metric_kernel", 0.0, 8.0 * n * g):
        capi.check(capi.lib().ly_anchor_metric(_p(wh), n, _p(k), g, na, float(thr), s, _p(part), capi.stream_ptr()), "ly_anchor_metric")
    out = torch.empty(3 * g, dtype=torch.float64, device=wh.device)
    capi.check(capi.lib().ly_sum_rows_f64(_p(part), s, 3 * g, _p(out), capi.stream_ptr()), "ly_sum_rows_f64")
    return out.view(g, 3)


def anchor_evolve_round(wh, v, k, f, cursor, batch, thr, part):
    """one (eval, pick) pair: `batch` speculative generations from cursor[0]; part [slices, batch] float64 scratch"""
    n, (gen, na, _), s = wh.shape[0], v.shape, part.shape[0]
    st = capi.stream_ptr()
    with _Timed("ly_anchor_evolve_eval_kernel", 0.0, 8.0 * n * batch):
        capi.check(capi.lib().ly_anchor_evolve_eval(_p(wh), n, _p(v), gen, na, _p(k), _p(cursor), batch, float(thr), s, _p(part), st),
                   "ly_anchor_evolve_eval")
    capi.check(capi.lib().ly_anchor_evolve_pick(_p(part), s, batch, _p(v), gen, na, _p(k), _p(f), _p(cursor), st), "ly_anchor_evolve_pick")


def kmeans_assign(pts, cent, flags, part, assign=None):
    """the assign + accumulate half of a Lloyd iteration: part [slices, R, 3 na + 1] float64"""
    n, (r, na, _), s = pts.shape[0], cent.shape, part.shape[0]
    with _Timed("ly_kmeans_assign_kernel", 0.0, 8.0 * n * r):
        capi.check(capi.lib().ly_kmeans_assign(_p(pts), n, _p(cent), r, na, _p(flags), s, _p(part), _p(assign), capi.stream_ptr()), "ly_kmeans_assign")


def kmeans_update(part, n, thresh, cent, dist, count, flags, iters, active):
    """the fold + update half: centroids, distortions, counts, flags, iteration counts and the open-run count, all in place"""
    s, (r, na, _) = part.shape[0], cent.shape
    capi.check(capi.lib().ly_kmeans_update(_p(part), s, r, na, n, float(thresh), _p(cent), _p(dist), _p(count), _p(flags), _p(iters), _p(active),
                                           capi.stream_ptr()), "ly_kmeans_update")
