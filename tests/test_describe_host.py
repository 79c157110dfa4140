"""The launch dispatch of every kernel family, read back on the host through the ly_<entry>_describe twins (include/lead_yolo_hip.h): the name
of the contraction kernel a call would launch, formatted by the launch function itself.  No GPU: the addresses below are made-up integers with
the alignment a case needs (no describe entry dereferences one), the library is the built .so as in test_wgrad_plan_host.py.

The expected names are not taken from the code under test: the branch cases' come from the dispatch rules as the comments of csrc/, DESIGN.md
and the header state them (each rule is quoted where it is used), the committed step's from rocprofv3's own table of that step
(profiles/r07_train_bf16_step_kernels.txt), the tile choices from the pure-Python function this library had before the LDS figure came from C."""
import collections
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

from lead_yolo_amd import capi, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, C_, D, E, F = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000      # 16-byte aligned "device" addresses
F32, BF16 = capi.LY_F32, capi.LY_BF16
T = {F32: "float", BF16: "__bf16"}


def describe(fn, *args, cap=160):
    """(return code, name) of the describe entry `fn` on the arguments (structs go by reference)"""
    name = ctypes.create_string_buffer(cap)
    rc = getattr(capi.lib(), fn)(*[ctypes.byref(a) if isinstance(a, ctypes.Structure) else a for a in args], name, cap)
    return rc, name.value.decode()


def err():
    return capi.lib().ly_last_error().decode()


# ---- the problems ---------------------------------------------------------------------------------------------------------------------
def gemm(N, K, dtype=BF16, M=25600, H=160, W=160, gather=capi.GATHER_ROWS, pro=capi.PRO_NONE, out=True, stats=False, ldo=None, **kw):
    f = dict(M=M, H=H, W=W, K=K, N=N, a0=A, lda0=K, k0=K, gather=gather, pro=pro, wp=B, out=C_ if out else None, ldo=ldo or N,
             stats=D if stats else None, dtype=dtype)
    if pro == capi.PRO_GATE:
        f.update(g_h=E, g_w=E + 4096)
    if pro == capi.PRO_AFFINE_RELU_CA:
        f.update(p_scale=E, p_shift=E + 4096, p_ca=E + 8192, rowscale=F)
    f.update(kw)
    return capi.LyGemmParams(**f)


def image(N, gather, dtype, stats=False, Cin=3):
    """a 4 x 4 patch embedding of an NCHW image: 64 x 64 pixels -> 16 x 16 patches, two images"""
    return gemm(N, 16 * Cin, dtype, M=512, H=16, W=16, gather=gather, stats=stats, lda0=0, Hin=64, Win=64, Cin=Cin, ks=4, pk=0)


def conv3(N, n, hw, th, tw, dtype=BF16, Cin=64):
    return capi.LyConv3Params(M=n * hw * hw, H=hw, W=hw, Cin=Cin, N=N, TH=th, TW=tw, x=A, ldx=Cin, wp=B, e_scale=C_, e_shift=C_ + 4096, act=2, out=D,
                              ldo=N, stats=None, dtype=dtype)


def rf3(N, n=2, hw=16, c=64, s=1, th=8, tw=8, dtype=BF16, wg=True, stats=False, out=True):
    ho = (hw + 2 - 3) // s + 1
    return capi.LyRfcbam3Params(n_img=n, H=hw, W=hw, C=c, Ho=ho, Wo=ho, N=N, s=s, TH=th, TW=tw, x=A, ldx=c, wg=B if wg else None, ca=C_, rfa=C_ + 4096,
                                wp=D, e_scale=E, e_shift=E + 4096, out=F if out else None, ldo=N, stats=F + 65536 if stats else None, linear=0, dtype=dtype)


# ---- every branch: (entry, arguments, the kernel the stated rules give) -------------------------------------------------------------------
def _gemm_cases():
    g = "ly_gemm_kernel_d2"
    rows = []
    # Tile policy (ly_gemm_dispatch): N > 64: 64 px x 128 ch <4, 2, 4>; N > 32: 64 x 64 <4, 1, 4>; else 128 px x 32 ch <2, 2, 1> — but a
    # CoordAtt-gate prologue never takes the 128 x 32 tile: <4, 1, 4>.  Variant (launch_gemm_v): K in one / two chunks of 16 vectors (128 bf16, 64
    # fp32 elements) = weights resident NCH 1 / 2 where the instantiation fits 256 registers (one chunk: WC == 4 or no prologue; two: WC == 4 and
    # no gate; with the BatchNorm sums also: never with a gate, two chunks only without prologue); epilogue FAST 1 = branch-free (N, ldo multiples
    # of 4 and an output), 2 = + statistics, 3 = scatter store, 4 = scatter + eadd; long K keeps FAST without prologue, and with the gate when
    # there are no statistics; anything else is <.., 0, 0>.
    for dt, ck in ((BF16, 128), (F32, 64)):
        t = T[dt]
        rows += [(gemm(128, ck, dt), f"{g}<{t}, {t}, 4, 2, 4, 0, 0, 1, 1>"),
                 (gemm(128, 2 * ck, dt), f"{g}<{t}, {t}, 4, 2, 4, 0, 0, 2, 1>"),
                 (gemm(128, 3 * ck, dt), f"{g}<{t}, {t}, 4, 2, 4, 0, 0, 0, 1>"),
                 (gemm(128, ck, dt, stats=True), f"{g}<{t}, {t}, 4, 2, 4, 0, 0, 1, 2>"),
                 (gemm(128, 2 * ck, dt, stats=True), f"{g}<{t}, {t}, 4, 2, 4, 0, 0, 2, 2>"),
                 (gemm(128, 3 * ck, dt, stats=True), f"{g}<{t}, {t}, 4, 2, 4, 0, 0, 0, 2>"),
                 (gemm(128, ck, dt, out=False, stats=True), f"{g}<{t}, {t}, 4, 2, 4, 0, 0, 0, 0>"),         # statistics only: no output, not FAST
                 (gemm(48, ck, dt, stats=True), f"{g}<{t}, {t}, 4, 1, 4, 0, 0, 1, 2>"),
                 (gemm(24, ck, dt), f"{g}<{t}, {t}, 2, 2, 1, 0, 0, 1, 1>"),
                 (gemm(24, 2 * ck, dt), f"{g}<{t}, {t}, 2, 2, 1, 0, 0, 0, 1>"),                             # WC == 1: two chunks are not resident
                 (gemm(30, ck, dt), f"{g}<{t}, {t}, 2, 2, 1, 0, 0, 0, 0>"),                                 # N % 4 != 0
                 (gemm(128, ck, dt, ldo=130), f"{g}<{t}, {t}, 4, 2, 4, 0, 0, 0, 0>"),                       # ldo % 4 != 0
                 # the gate prologue: N = 32 on the 64 x 64 tile (the case the Python copy labelled <2, 2, 1>)
                 (gemm(32, ck, dt, pro=capi.PRO_GATE), f"{g}<{t}, {t}, 4, 1, 4, 0, 1, 1, 1>"),
                 (gemm(32, 2 * ck, dt, pro=capi.PRO_GATE), f"{g}<{t}, {t}, 4, 1, 4, 0, 1, 0, 1>"),
                 (gemm(24, ck, dt, pro=capi.PRO_GATE, stats=True), f"{g}<{t}, {t}, 4, 1, 4, 0, 1, 0, 0>"),
                 (gemm(128, ck, dt, pro=capi.PRO_GATE), f"{g}<{t}, {t}, 4, 2, 4, 0, 1, 1, 1>"),
                 # the affine (RFCBAM k = 1) prologue
                 (gemm(128, ck, dt, pro=capi.PRO_AFFINE_RELU_CA, stats=True), f"{g}<{t}, {t}, 4, 2, 4, 0, 2, 1, 2>"),
                 (gemm(128, 2 * ck, dt, pro=capi.PRO_AFFINE_RELU_CA), f"{g}<{t}, {t}, 4, 2, 4, 0, 2, 2, 1>"),
                 (gemm(128, 2 * ck, dt, pro=capi.PRO_AFFINE_RELU_CA, stats=True), f"{g}<{t}, {t}, 4, 2, 4, 0, 2, 0, 0>"),
                 (gemm(24, ck, dt, pro=capi.PRO_AFFINE_RELU_CA), f"{g}<{t}, {t}, 2, 2, 1, 0, 2, 0, 0>"),     # WC == 1 with a prologue: nothing resident
                 # gathers: 2x upsample, k x k patches of an NHWC map
                 (gemm(128, ck, dt, gather=capi.GATHER_UP2), f"{g}<{t}, {t}, 4, 2, 4, 1, 0, 1, 1>"),
                 (gemm(128, ck, dt, M=6400, H=80, W=80, gather=capi.GATHER_PATCH, lda0=ck // 4, ks=2, pk=ck // 2, Hin=160, Win=160, Cin=ck // 4),
                  f"{g}<{t}, {t}, 4, 2, 4, 2, 0, 1, 1>"),
                 # scatter store, and eadd: plain rows + eadd re-enters as the scatter epilogue with a 1 x 1 patch
                 (gemm(128, ck, dt, scat_ks=2, scat_c=32), f"{g}<{t}, {t}, 4, 2, 4, 0, 0, 1, 3>"),
                 (gemm(128, 3 * ck, dt, scat_ks=2, scat_c=32), f"{g}<{t}, {t}, 4, 2, 4, 0, 0, 0, 3>"),
                 (gemm(128, ck, dt, eadd=F, ldeadd=128), f"{g}<{t}, {t}, 4, 2, 4, 0, 0, 1, 4>"),
                 (gemm(128, 2 * ck, dt, eadd=F, ldeadd=128), f"{g}<{t}, {t}, 4, 2, 4, 0, 0, 2, 4>"),
                 (gemm(128, 3 * ck, dt, scat_ks=2, scat_c=32, eadd=F, ldeadd=32), f"{g}<{t}, {t}, 4, 2, 4, 0, 0, 0, 4>"),
                 # an NCHW image the patch4 kernel does not take (N > 80): TI is the image's element type, the gather code the fp32 image's
                 (image(96, capi.GATHER_PATCH_NCHW, dt), f"{g}<float, {t}, 4, 2, 4, 3, 0, 1, 1>"),
                 (image(96, capi.GATHER_PATCH_NCHW_U8, dt), f"{g}<unsigned char, {t}, 4, 2, 4, 3, 0, 1, 1>"),
                 # ly_patch4_try: RGB, K = 48, 20 <= N <= 80: <TI, TO, max(2, ceil(N / 16)), statistics>
                 (image(24, capi.GATHER_PATCH_NCHW_U8, dt, stats=True), f"ly_patch4_kernel<unsigned char, {t}, 2, true>"),
                 (image(48, capi.GATHER_PATCH_NCHW, dt), f"ly_patch4_kernel<float, {t}, 3, false>"),
                 (image(64, capi.GATHER_PATCH_NCHW_U8, dt), f"ly_patch4_kernel<unsigned char, {t}, 4, false>"),
                 (image(80, capi.GATHER_PATCH_NCHW, dt, stats=True), f"ly_patch4_kernel<float, {t}, 5, true>")]
    # 16-bit images: LY_BF16 calls only
    rows += [(image(96, capi.GATHER_PATCH_NCHW_BF16, BF16), f"{g}<ly_bf16img, __bf16, 4, 2, 4, 3, 0, 1, 1>"),
             (image(96, capi.GATHER_PATCH_NCHW_F16, BF16), f"{g}<ly_f16img, __bf16, 4, 2, 4, 3, 0, 1, 1>"),
             (image(24, capi.GATHER_PATCH_NCHW_BF16, BF16), "ly_patch4_kernel<ly_bf16img, __bf16, 2, false>"),
             (image(24, capi.GATHER_PATCH_NCHW_F16, BF16, stats=True), "ly_patch4_kernel<ly_f16img, __bf16, 2, true>")]
    return [("ly_gemm_describe", (p,), name) for p, name in rows]


def _conv3_cases():
    # conv3_dispatch: 128 channels per block <2, 4> for N > 64, else <2, 2>; bf16 instantiations carry the patch's active pixel tiles
    # ntv = ceil(TH * TW / 16) at compile time — <2, 4, 5>, <2, 4, 8>, and <2, 2, 4> for ntv == 8 — every other case 0; a bf16 grid under two
    # blocks per CU (images x patches x ceil(N / 128) < 512) with N > 64 takes the latency form <__bf16, 2, 2>
    k = "ly_conv3x3_kernel"
    rows = [(conv3(128, 64, 40, 10, 8), f"{k}<__bf16, 2, 4, 5>"), (conv3(128, 64, 80, 16, 8), f"{k}<__bf16, 2, 4, 8>"),
            (conv3(128, 64, 40, 4, 8), f"{k}<__bf16, 2, 4, 0>"), (conv3(64, 64, 80, 16, 8), f"{k}<__bf16, 2, 2, 4>"),
            (conv3(64, 64, 40, 10, 8), f"{k}<__bf16, 2, 2, 0>"), (conv3(64, 2, 20, 20, 4), f"{k}<__bf16, 2, 2, 0>"),
            (conv3(128, 2, 20, 20, 4), "ly_conv3x3_lat_kernel<__bf16, 2, 2>"), (conv3(256, 2, 20, 20, 4), "ly_conv3x3_lat_kernel<__bf16, 2, 2>"),
            (conv3(128, 64, 40, 10, 8, F32), f"{k}<float, 2, 4, 0>"), (conv3(128, 2, 20, 20, 4, F32), f"{k}<float, 2, 4, 0>"),
            (conv3(64, 64, 80, 16, 8, F32), f"{k}<float, 2, 2, 0>")]
    return [("ly_conv3x3_describe", (p,), name) for p, name in rows]


def _mlp_cases():
    ring, one, occ4, per, res, pc1 = ("ly_mlpblock_fwd_ring_kernel", "ly_mlpblock_fwd_kernel", "ly_mlpblock_fwd_occ4_kernel", "ly_mlpblock_persist_kernel",
                                      "ly_mlpblock_res_kernel", "ly_mlpblock_pconv1_kernel")
    rows = []
    # Tiling policy (ly_mlpblock.hpp): <T, C, NT, HT, T2D, STATS>, HT = 2, 4, 2, 2, 4, 4 for C = 16 .. 320.
    # C < 80: the persistent patch walk <T, C, 2, HT, MODE, 1> (MODE 0 forward, 1 statistics, 2 partial conv) where W % 16 == 0, W >= 32 and there
    # are >= 1024 patches of 8 x 16 — not for fp32 at C = 40; else 2-D patches (T2D, NT 2) where W % 16 == 0 and W >= 64, with four waves per SIMD
    # (occ4) for C <= 24; else flattened runs with NT = 4 from 256 K pixels, 2 from 64 K, else 1.
    for dt in (BF16, F32):
        t = T[dt]
        for st in (0, 1):
            s = "true" if st else "false"
            rows += [(("ly_mlpblock_fwd_describe", (64, 160, 160, 24, dt, st)), f"{per}<{t}, 24, 2, 4, {st}, 1>"),
                     (("ly_mlpblock_fwd_describe", (64, 160, 160, 16, dt, st)), f"{per}<{t}, 16, 2, 2, {st}, 1>"),
                     (("ly_mlpblock_fwd_describe", (1, 64, 64, 24, dt, st)), f"{occ4}<{t}, 24, 2, 4, true, {s}>"),
                     (("ly_mlpblock_fwd_describe", (1, 64, 64, 40, dt, st)), f"{one}<{t}, 40, 2, 2, true, {s}>"),
                     (("ly_mlpblock_fwd_describe", (1, 13, 17, 16, dt, st)), f"{one}<{t}, 16, 1, 2, false, {s}>"),
                     (("ly_mlpblock_fwd_describe", (16, 65, 65, 16, dt, st)), f"{one}<{t}, 16, 2, 2, false, {s}>"),
                     (("ly_mlpblock_fwd_describe", (64, 65, 65, 40, dt, st)), f"{one}<{t}, 40, 4, 2, false, {s}>"),
                     # C >= 80: the ring kernel on flattened runs; two pixel tiles per wave from 200 x 128 pixels (C = 320: always one)
                     (("ly_mlpblock_fwd_describe", (64, 20, 20, 160, dt, st)), f"{ring}<{t}, 160, 2, 4, false, {s}>"),
                     (("ly_mlpblock_fwd_describe", (2, 20, 20, 160, dt, st)), f"{ring}<{t}, 160, 1, 4, false, {s}>"),
                     (("ly_mlpblock_fwd_describe", (64, 20, 20, 320, dt, st)), f"{ring}<{t}, 320, 1, 4, false, {s}>"),
                     (("ly_mlpblock_fwd_describe", (2, 20, 20, 80, dt, st)), f"{ring}<{t}, 80, 1, 2, false, {s}>")]
        rows += [(("ly_mlpblock_fwd_describe", (64, 80, 80, 40, dt, 0)), f"{per}<__bf16, 40, 2, 2, 0, 1>" if dt == BF16 else f"{one}<float, 40, 2, 2, true, false>"),
                 # the partial conv alone: the persistent walk in MODE 2 under the same shape rule (fp32: C < 40), else the one-shot kernel on 64-pixel runs
                 (("ly_mlpblock_pconv_describe", (64, 160, 160, 24, dt)), f"{per}<{t}, 24, 2, 4, 2, 1>"),
                 (("ly_mlpblock_pconv_describe", (64, 80, 80, 40, dt)), f"{per}<__bf16, 40, 2, 2, 2, 1>" if dt == BF16 else f"{pc1}<float, 40, 1, 2, false>"),
                 (("ly_mlpblock_pconv_describe", (1, 13, 17, 16, dt)), f"{pc1}<{t}, 16, 1, 2, false>"),
                 (("ly_mlpblock_pconv_describe", (64, 20, 20, 160, dt)), f"{pc1}<{t}, 160, 1, 4, false>"),
                 (("ly_mlpblock_pconv_describe", (2, 40, 40, 80, dt)), f"{pc1}<{t}, 80, 1, 2, false>"),
                 (("ly_mlpblock_pconv_describe", (2, 20, 20, 320, dt)), f"{pc1}<{t}, 320, 1, 4, false>")]
    # C = 80: bf16 with >= 128 runs of 256 pixels takes the resident-weights kernel <__bf16, 80, 2, 2, STATS, 4> — unless the map is too wide
    # for its halo plan (256 + 2 W + 2 positions x 5 vectors <= 2048: W <= 75), then the ring kernel, four tiles per wave from 384 x 256 pixels
    rows += [(("ly_mlpblock_fwd_describe", (64, 40, 40, 80, BF16, 1)), f"{res}<__bf16, 80, 2, 2, true, 4>"),
             (("ly_mlpblock_fwd_describe", (64, 40, 40, 80, BF16, 0)), f"{res}<__bf16, 80, 2, 2, false, 4>"),
             (("ly_mlpblock_fwd_describe", (8, 80, 80, 80, BF16, 0)), f"{ring}<__bf16, 80, 2, 2, false, false>"),
             (("ly_mlpblock_fwd_describe", (16, 80, 80, 80, BF16, 1)), f"{ring}<__bf16, 80, 4, 2, false, true>"),
             (("ly_mlpblock_fwd_describe", (16, 40, 40, 80, BF16, 0)), f"{ring}<__bf16, 80, 2, 2, false, false>"),      # 25600 pixels: under 128 x 256
             (("ly_mlpblock_fwd_describe", (64, 40, 40, 80, F32, 0)), f"{ring}<float, 80, 2, 2, false, false>")]
    # the fused backward, bf16 only: <C, 2, T2D, PASS, 1>; 2-D patches "unless more than a quarter of the 16-wide patch columns would lie outside
    # the map" and never under 12 columns: W = 40 (8 of 48 outside) and W = 12 (4 of 16) take patches, W = 20 (12 of 32) and W = 11 do not
    for c in (16, 24, 40, 80):
        for ps in (1, 2):
            rows += [(("ly_mlpblock_bwd_describe", (64, 40, 40, c, BF16, ps)), f"ly_mlpblock_bwd_kernel<{c}, 2, true, {ps}, 1>"),
                     (("ly_mlpblock_bwd_describe", (64, 20, 20, c, BF16, ps)), f"ly_mlpblock_bwd_kernel<{c}, 2, false, {ps}, 1>")]
    rows += [(("ly_mlpblock_bwd_describe", (64, 11, 11, 80, BF16, 2)), "ly_mlpblock_bwd_kernel<80, 2, false, 2, 1>"),
             (("ly_mlpblock_bwd_describe", (64, 12, 12, 80, BF16, 2)), "ly_mlpblock_bwd_kernel<80, 2, true, 2, 1>")]
    # its tail <C, T2D, WG>: the same patch rule; the weight gradient is built in (WG) on patches, when a slab and dwp are given, for C / 4 <= 32
    for c in (16, 24, 40, 80):
        rows += [(("ly_mlpblock_bwd_dx_describe", (64, 40, 40, c, BF16, 1)), f"ly_mlpblock_bwd_dx_kernel<{c}, true, true>"),
                 (("ly_mlpblock_bwd_dx_describe", (64, 40, 40, c, BF16, 0)), f"ly_mlpblock_bwd_dx_kernel<{c}, true, false>"),
                 (("ly_mlpblock_bwd_dx_describe", (64, 20, 20, c, BF16, 1)), f"ly_mlpblock_bwd_dx_kernel<{c}, false, false>")]
    rows += [(("ly_mlpblock_bwd_dx_describe", (64, 20, 20, 160, BF16, 1)), "ly_mlpblock_bwd_dx_kernel<160, false, false>"),
             (("ly_mlpblock_bwd_dx_describe", (64, 12, 12, 160, BF16, 1)), "ly_mlpblock_bwd_dx_kernel<160, true, false>")]
    return [(fn, args, name) for (fn, args), name in rows]


def _rf_cases():
    rows = []
    for dt in (BF16, F32):
        t = T[dt]
        # rc_dispatch_fwd <T, MT, NW, S, RAW>: N <= 64: 4 waves x 16 channels <1, 4>; N <= 128: <2, 4>; wider, bf16 only: 8 waves <2, 8>
        wide = "2, 8" if dt == BF16 else "2, 4"
        for raw in (0, 1):
            r = "true" if raw else "false"
            rows += [("ly_rf3c_fwd_describe", (rf3(64, s=1, dtype=dt, wg=False), B, raw), f"ly_rf3c_fwd_kernel<{t}, 1, 4, 1, {r}>"),
                     ("ly_rf3c_fwd_describe", (rf3(128, s=2, dtype=dt, wg=False), B, raw), f"ly_rf3c_fwd_kernel<{t}, 2, 4, 2, {r}>"),
                     ("ly_rf3c_fwd_describe", (rf3(256, s=2, dtype=dt, wg=False), B, raw), f"ly_rf3c_fwd_kernel<{t}, {wide}, 2, {r}>"),
                     ("ly_rf3c_fwd_describe", (rf3(256, s=1, dtype=dt, wg=False, stats=True, out=False), B, raw), f"ly_rf3c_fwd_kernel<{t}, {wide}, 1, {r}>")]
        # rf3_dispatch <T, MT>: MT = 1 / 2 / 4 for N <= 64 / <= 128 / wider; launch_rf3: the MT = 4 tile reads its weights through the scalar
        # cache (_sw) once the grid (images x tiles x ceil(N / 256)) has more than 256 blocks
        rows += [("ly_rfcbam3_describe", (rf3(64, dtype=dt),), f"ly_rfcbam3_kernel<{t}, 1>"),
                 ("ly_rfcbam3_describe", (rf3(128, dtype=dt),), f"ly_rfcbam3_kernel<{t}, 2>"),
                 ("ly_rfcbam3_describe", (rf3(256, n=64, dtype=dt),), f"ly_rfcbam3_kernel<{t}, 4>"),                 # 64 x 4 x 1 = 256 blocks: not more
                 ("ly_rfcbam3_describe", (rf3(256, n=65, dtype=dt),), f"ly_rfcbam3_sw_kernel<{t}, 4>"),
                 ("ly_rfcbam3_describe", (rf3(512, n=33, dtype=dt),), f"ly_rfcbam3_sw_kernel<{t}, 4>"),              # 33 x 4 x 2 = 264
                 # ly_rfcbam_tap_moments: the LDS-tiled kernel at stride 2 with whole 16-byte channel vectors, else the per-pixel one
                 ("ly_rfcbam_tap_moments_describe", (A, 64, 2, 16, 16, 64, 2, B, dt), f"ly_rfcbam_tap_moments_s2t_kernel<{t}>"),
                 ("ly_rfcbam_tap_moments_describe", (A, 64, 2, 16, 16, 64, 1, B, dt), f"ly_rfcbam_tap_moments_kernel<{t}>"),
                 ("ly_rfcbam_tap_moments_describe", (A, 66, 2, 16, 16, 66, 2, B, dt), f"ly_rfcbam_tap_moments_kernel<{t}>"),
                 ("ly_rfcbam_tap_moments_describe", (A + 4, 64, 2, 16, 16, 64, 2, B, dt), f"ly_rfcbam_tap_moments_kernel<{t}>"),
                 # ly_rf_bwd_dx: k = 3 at stride 2 on an even map with C % 8 == 0 through 4 x 4 LDS tiles <T, 4, addnc given>; else the gather
                 # <T, k, ADD>: ADD 0 without addnc, 2 when a block's pixel chunk (at least 8 per sub-group) lies inside one image, else 1
                 ("ly_rf_bwd_dx_describe", (2, 16, 16, 64, 3, 2, A, B, C_, 64, D, 0.5, dt), f"ly_rf_bwd_dx_s2t_kernel<{t}, 4, 1>"),
                 ("ly_rf_bwd_dx_describe", (2, 16, 16, 64, 3, 2, A, B, C_, 64, None, 0.0, dt), f"ly_rf_bwd_dx_s2t_kernel<{t}, 4, 0>"),
                 ("ly_rf_bwd_dx_describe", (2, 15, 15, 64, 3, 2, A, B, C_, 64, None, 0.0, dt), f"ly_rf_bwd_dx_kernel<{t}, 3, 0>"),
                 ("ly_rf_bwd_dx_describe", (2, 20, 20, 64, 3, 1, A, B, C_, 64, D, 0.5, dt), f"ly_rf_bwd_dx_kernel<{t}, 3, 2>"),
                 ("ly_rf_bwd_dx_describe", (2, 4, 4, 64, 3, 1, A, B, C_, 64, D, 0.5, dt), f"ly_rf_bwd_dx_kernel<{t}, 3, 1>"),      # 32-pixel chunks, 16-pixel images
                 ("ly_rf_bwd_dx_describe", (2, 20, 20, 64, 1, 1, A, B, C_, 64, None, 0.0, dt), f"ly_rf_bwd_dx_kernel<{t}, 1, 0>"),
                 ("ly_rf_bwd_dx_describe", (2, 20, 20, 64, 1, 1, A, B, C_, 64, D, 0.5, dt), f"ly_rf_bwd_dx_kernel<{t}, 1, 2>"),
                 ("ly_rf_bwd_dx_describe", (2, 4, 4, 64, 1, 1, A, B, C_, 64, D, 0.5, dt), f"ly_rf_bwd_dx_kernel<{t}, 1, 1>")]
        # ly_rfcbam_stats: k = 3: stats3; k = 1 without pooling partials: stats1; with them the several-pixels-per-wave kernel <T, V>, V = 16-byte
        # vectors per lane = ceil(C / VW / 16) up to 4, for whole vectors (C and ldx multiples of VW = 4 fp32 / 8 bf16), else one pixel per wave
        vw = 8 if dt == BF16 else 4
        rows += [("ly_rfcbam_stats_describe", (A, 64, 2, 16, 16, 64, 3, 1, B, None, None, 8, 8, C_, None, 0, dt), f"ly_rfcbam_stats3_kernel<{t}>"),
                 ("ly_rfcbam_stats_describe", (A, 64, 2, 16, 16, 64, 1, 1, None, B, B + 4096, 1, 64, C_, None, 0, dt), f"ly_rfcbam_stats1_kernel<{t}>"),
                 ("ly_rfcbam_stats_describe", (A, 16 * vw, 2, 16, 16, 16 * vw, 1, 1, None, B, B + 4096, 1, 64, C_, D, 4, dt), f"ly_rfcbam_pre1v_kernel<{t}, 1>"),
                 ("ly_rfcbam_stats_describe", (A, 20 * vw, 2, 16, 16, 20 * vw, 1, 1, None, B, B + 4096, 1, 64, C_, D, 4, dt), f"ly_rfcbam_pre1v_kernel<{t}, 2>"),
                 ("ly_rfcbam_stats_describe", (A, 48 * vw, 2, 16, 16, 48 * vw, 1, 1, None, B, B + 4096, 1, 64, C_, D, 4, dt), f"ly_rfcbam_pre1v_kernel<{t}, 3>"),
                 ("ly_rfcbam_stats_describe", (A, 64 * vw, 2, 16, 16, 64 * vw, 1, 1, None, B, B + 4096, 1, 64, C_, D, 4, dt), f"ly_rfcbam_pre1v_kernel<{t}, 4>"),
                 ("ly_rfcbam_stats_describe", (A, 20, 2, 16, 16, 20, 1, 1, None, B, B + 4096, 1, 64, C_, D, 4, dt),
                  f"ly_rfcbam_pre1_kernel<{t}>" if dt == BF16 else f"ly_rfcbam_pre1v_kernel<{t}, 1>"),                      # 20 channels: whole quads, no whole octets
                 ("ly_rfcbam_stats_describe", (A, 65 * vw, 2, 16, 16, 65 * vw, 1, 1, None, B, B + 4096, 1, 64, C_, D, 4, dt),
                  f"ly_rfcbam_pre1_kernel<{t}>")]                                                                             # more than 64 vectors per pixel
    # ly_rf3m_fwd, bf16 only: blocks of 128 output channels <4, false>, or 64 when N % 128 != 0 <2, false> (the second argument is the
    # profiling form of development builds)
    rows += [("ly_rf3m_fwd_describe", (rf3(256, th=4, tw=8, wg=False),), "ly_rf3m_fwd_kernel<4, false>"),
             ("ly_rf3m_fwd_describe", (rf3(192, th=4, tw=8, s=2, wg=False),), "ly_rf3m_fwd_kernel<2, false>")]
    # the PatchEmbed weight gradient from the uint8 image: <ceil(N / 16)>
    for n_out, mtn in ((8, 1), (24, 2), (40, 3), (64, 4)):
        rows.append(("ly_patch4_wgrad_u8_describe", (A, 2, 3, 64, 64, B, n_out, n_out, 1 / 255, C_, 1536 * 64 * 48, D, BF16), f"ly_patch4_wgrad_u8_kernel<{mtn}>"))
    return rows


CASES = _gemm_cases() + _conv3_cases() + _mlp_cases() + _rf_cases()


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{i}-{c[2].split('<')[0]}" for i, c in enumerate(CASES)])
def test_every_branch_of_every_dispatch(i):
    fn, args, want = CASES[i]
    rc, name = describe(fn, *args)
    assert (rc, name) == (0, want), (fn, rc, name, err() if rc < 0 else "")


# ---- spelling -----------------------------------------------------------------------------------------------------------------------------
def _library_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from demangle import norm
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = [line.split()[-1] for line in out.splitlines() if line.strip()]
    return {norm(s) for s in syms if s.startswith("_Z") and "ly_" in s}


def _step_calls():
    """[(entry, ctypes arguments)] of profiles/r08_train_bf16_step_calls.jsonl (tools/step_calls.py)"""
    calls = []
    for line in open(os.path.join(ROOT, "profiles", "r08_train_bf16_step_calls.jsonl")):
        c = json.loads(line)
        args = []
        for a in c["args"]:
            if isinstance(a, dict):
                a = getattr(capi, a["struct"])(**a["fields"])
            elif isinstance(a, list):
                a = (getattr(capi, a[0]["struct"]) * len(a))(*[getattr(capi, s["struct"])(**s["fields"]) for s in a])
            args.append(a)
        calls.append((c["fn"], args))
    return calls


def test_every_described_name_is_a_kernel_of_the_built_library():
    """every name any describe in this file returns — the branch cases' (equal to the expected names, as the branch test holds) and the committed
    step's — is, letter for letter, a kernel the library exports a handle for"""
    built = _library_kernels()
    assert "ly_wgrad3_kernel" in built and len(built) > 500
    names = {want for _, _, want in CASES} | {describe(fn, *args)[1] for fn, args in _step_calls()}
    assert not sorted(names - built)


# ---- the committed step ---------------------------------------------------------------------------------------------------------------------
def test_the_committed_step_gets_the_names_rocprofv3_printed():
    """the 120 described calls of the bs=64 bf16 step, profiles/r08_train_bf16_step_calls.jsonl, described one by one: the multiset of names is the
    launch count of every contraction row of these families in that step's rocprofv3 table"""
    got = collections.Counter()
    for fn, args in _step_calls():
        rc, name = describe(fn, *args)
        assert rc == 0, (fn, rc, name, err())
        got[name] += 1

    families = r"ly_(gemm_kernel_d2|patch4_kernel|patch4_wgrad_u8_kernel|conv3x3|mlpblock_(fwd|persist|res|pconv1|bwd_kernel|bwd_dx_kernel)|rf3c_fwd|rfcbam_stats|rfcbam_pre1|rfcbam_tap_moments|rf_bwd_dx|wgrad)"
    table = collections.Counter()
    for line in open(os.path.join(ROOT, "profiles", "r07_train_bf16_step_kernels.txt")):
        m = re.match(r"(ly_\S*(?: \S+)*?)\s{2,}(\d+)\s+[\d.]+ us\s+[\d.]+ us\s*$", line)
        if m and re.match(families, m[1]) and "_combine" not in m[1]:
            name = m[1]
            # rocprofv3's own demangler garbles a `__bf16` template argument behind another type into "bool _Accum, ..." (tools/demangle.py); of the
            # families here that is the patch embedding's row, whose spelling profiles/r06_train_bf16_pmc_traffic.json (demangled by
            # tools/demangle.py) gives in full
            if name == "ly_patch4_kernel<unsigned char, bool _Accum, int, EL, bool, E>":
                name = "ly_patch4_kernel<unsigned char, __bf16, 2, true>"
                assert name in open(os.path.join(ROOT, "profiles", "r06_train_bf16_pmc_traffic.json")).read()
            table[name] += int(m[2])
    g = "ly_gemm_kernel_d2<__bf16, __bf16, "
    by_hand = {g + "4, 2, 4, 0, 0, 2, 1>": 12, g + "4, 2, 4, 0, 0, 1, 4>": 4, g + "4, 2, 4, 0, 0, 2, 2>": 5, g + "4, 2, 4, 0, 0, 1, 1>": 6,
               g + "4, 2, 4, 0, 0, 1, 2>": 3, g + "4, 2, 4, 0, 0, 0, 2>": 3, g + "4, 2, 4, 0, 0, 0, 1>": 4, g + "4, 2, 4, 1, 0, 2, 2>": 1,
               g + "4, 2, 4, 0, 2, 0, 0>": 2, g + "4, 1, 4, 0, 0, 1, 1>": 2, g + "4, 2, 4, 1, 0, 0, 2>": 1, g + "4, 2, 4, 0, 0, 1, 3>": 1,
               g + "4, 1, 4, 2, 0, 1, 2>": 1, g + "4, 2, 4, 0, 0, 2, 4>": 2, g + "4, 1, 4, 0, 0, 1, 2>": 1, g + "4, 2, 4, 2, 0, 2, 2>": 1,
               g + "4, 2, 4, 2, 0, 0, 2>": 1, "ly_patch4_kernel<unsigned char, __bf16, 2, true>": 1, "ly_patch4_wgrad_u8_kernel<2>": 1,
               "ly_conv3x3_kernel<__bf16, 2, 4, 5>": 6, "ly_conv3x3_kernel<__bf16, 2, 2, 4>": 2,
               "ly_mlpblock_bwd_kernel<80, 2, true, 2, 1>": 3, "ly_mlpblock_bwd_kernel<80, 2, true, 1, 1>": 3, "ly_mlpblock_bwd_kernel<24, 2, true, 2, 1>": 1,
               "ly_mlpblock_bwd_kernel<24, 2, true, 1, 1>": 1, "ly_mlpblock_bwd_kernel<40, 2, true, 2, 1>": 1, "ly_mlpblock_bwd_kernel<40, 2, true, 1, 1>": 1,
               "ly_mlpblock_bwd_dx_kernel<80, true, true>": 3, "ly_mlpblock_bwd_dx_kernel<24, true, true>": 1, "ly_mlpblock_bwd_dx_kernel<40, true, true>": 1,
               "ly_mlpblock_bwd_dx_kernel<160, false, false>": 1, "ly_mlpblock_res_kernel<__bf16, 80, 2, 2, true, 4>": 3,
               "ly_mlpblock_res_kernel<__bf16, 80, 2, 2, false, 4>": 3, "ly_mlpblock_persist_kernel<__bf16, 24, 2, 4, 0, 1>": 1,
               "ly_mlpblock_persist_kernel<__bf16, 24, 2, 4, 1, 1>": 1, "ly_mlpblock_persist_kernel<__bf16, 40, 2, 2, 1, 1>": 1,
               "ly_mlpblock_persist_kernel<__bf16, 40, 2, 2, 0, 1>": 1, "ly_mlpblock_fwd_ring_kernel<__bf16, 160, 2, 4, false, false>": 1,
               "ly_mlpblock_fwd_ring_kernel<__bf16, 160, 2, 4, false, true>": 1, "ly_mlpblock_pconv1_kernel<__bf16, 160, 1, 4, false>": 1,
               "ly_rf3c_fwd_kernel<__bf16, 2, 4, 2, true>": 1, "ly_rf3c_fwd_kernel<__bf16, 2, 8, 2, true>": 1,
               "ly_rfcbam_tap_moments_s2t_kernel<__bf16>": 2, "ly_rfcbam_stats1_kernel<__bf16>": 2, "ly_rf_bwd_dx_s2t_kernel<__bf16, 4, 1>": 1,
               "ly_wgrad1_group_kernel": 10, "ly_wgrad3_kernel": 5, "ly_wgrad1_kernel<32, 128, true>": 3, "ly_wgrad1_kernel<128, 128, true>": 2,
               "ly_wgrad_tiled_kernel<__bf16, 128, 128, 128, false, false, true>": 2,
               "ly_wgrad_tiled_kernel<__bf16, 64, 128, 128, false, false, true>": 1, "ly_wgrad1_kernel<64, 64, true>": 1}
    assert dict(table) == by_hand and sum(table.values()) == 120
    assert got == table


# ---- the contract -------------------------------------------------------------------------------------------------------------------------
def test_refusals_carry_the_entrys_message():
    for (fn, args), msg in [(("ly_gemm_describe", (gemm(128, 100),)), "gemm: K=100 must be a multiple of 8"),
                            (("ly_gemm_describe", (gemm(128, 128, a0=A + 8),)), "gemm: sources must be 16-byte aligned"),
                            (("ly_gemm_describe", (gemm(128, 128, dtype=7),)), "gemm: unknown dtype 7"),
                            (("ly_gemm_describe", (gemm(128, 128, gather=capi.GATHER_UP2, pro=capi.PRO_GATE),)), "gemm: upsampled source with a prologue is not built"),
                            (("ly_gemm_describe", (image(96, capi.GATHER_PATCH_NCHW_BF16, F32),)), "gemm: a 16-bit image source is built for LY_BF16 calls only"),
                            (("ly_conv3x3_describe", (conv3(128, 2, 20, 20, 8),)), "conv3x3: patch 20x8 exceeds 128 pixels"),
                            (("ly_mlpblock_fwd_describe", (2, 20, 20, 48, BF16, 0)), "mlpblock: unsupported channel count C=48"),
                            (("ly_mlpblock_bwd_describe", (2, 20, 20, 80, F32, 1)), "mlpblock_bwd: bf16 storage only"),
                            (("ly_mlpblock_bwd_describe", (2, 20, 20, 80, BF16, 3)), "mlpblock_bwd: pass must be 1"),
                            (("ly_mlpblock_bwd_dx_describe", (2, 20, 20, 320, BF16, 0)), "mlpblock_bwd_dx: unsupported channel count C=320"),
                            (("ly_rf3c_fwd_describe", (rf3(128, c=48, wg=False), B, 0)), "rf3c_fwd: C=48 must be a multiple of 32"),
                            (("ly_rfcbam3_describe", (rf3(128, wg=False),)), "rfcbam3: null pointer"),
                            (("ly_rf3m_fwd_describe", (rf3(256, th=4, tw=8, dtype=F32, wg=False),)), "rf3m_fwd: bf16 storage only"),
                            (("ly_patch4_wgrad_u8_describe", (A, 2, 3, 64, 64, B, 20, 20, 1 / 255, C_, 1 << 20, D, BF16)), "patch4_wgrad_u8: N=20 must be a multiple of 8"),
                            (("ly_rfcbam_tap_moments_describe", (None, 64, 2, 16, 16, 64, 2, B, BF16)), "rfcbam_tap_moments: bad arguments"),
                            (("ly_rf_bwd_dx_describe", (2, 16, 16, 64, 2, 2, A, B, C_, 64, None, 0.0, BF16)), "rfcbam backward: kernel_size must be 1 or 3")]:
        rc, _ = describe(fn, *args)
        assert rc < 0 and msg in err(), (fn, rc, err())
    assert describe("ly_mlpblock_pconv_describe", 2, 20, 20, 48, BF16) == (1, "")             # ly_mlpblock_pconv's "not built for this width"
    P = gemm(128, 128)
    for fn, args in [("ly_gemm_describe", (ctypes.byref(P),)), ("ly_mlpblock_fwd_describe", (2, 20, 20, 80, BF16, 0))]:
        for name, cap in ((None, 16), (ctypes.create_string_buffer(16), 0)):
            assert getattr(capi.lib(), fn)(*args, name, cap) < 0 and "_describe: bad arguments" in err()
    assert capi.lib().ly_gemm_describe(None, ctypes.create_string_buffer(16), 16) < 0 and "gemm: null params" in err()


def test_describing_writes_nothing_but_the_name():
    full = "ly_gemm_kernel_d2<__bf16, __bf16, 4, 2, 4, 0, 0, 1, 1>"
    P = gemm(128, 128)
    before = bytes(P)
    for cap in (160, len(full) + 1, len(full), 10, 1):
        buf = ctypes.create_string_buffer(b"\xaa" * (8 + cap + 8), 8 + cap + 8)
        assert capi.lib().ly_gemm_describe(ctypes.byref(P), ctypes.byref(buf, 8), cap) == 0
        raw = bytes(buf)
        assert raw[:8] == b"\xaa" * 8 and raw[8 + cap:] == b"\xaa" * 8, f"cap={cap}: bytes outside name[cap] were written"
        want = full[:cap - 1].encode()
        assert raw[8:8 + len(want) + 1] == want + b"\0", f"cap={cap}: not the name cut to cap - 1 characters and terminated"
    assert bytes(P) == before


# ---- pick_tile_bwd_dx: the LDS figure now comes from ly_rf3c_bwd_lds ---------------------------------------------------------------------
def test_pick_tile_bwd_dx_chooses_what_the_python_formula_chose():
    """literals from the pure-Python ops.pick_tile_bwd_dx of the commit before this one (pass C's LDS formula written out in Python)"""
    was = {(7, 64): (7, 8), (7, 128): (7, 8), (7, 256): (7, 8), (10, 64): (10, 2), (10, 128): (10, 2), (10, 256): (10, 2), (13, 64): (13, 2),
           (13, 128): (13, 2), (13, 256): (13, 2), (20, 64): (8, 8), (20, 128): (8, 8), (20, 256): (20, 2), (40, 64): (8, 8), (40, 128): (8, 8),
           (40, 256): (4, 14), (80, 64): (8, 8), (80, 128): (4, 14), (80, 256): (1, 34)}
    assert {(hw, o): ops.pick_tile_bwd_dx(hw, hw, o) for hw in (7, 10, 13, 20, 40, 80) for o in (64, 128, 256)} == was
    # the figure itself, pass C at an 8 x 8 tile of a 40-wide map, O = 128, from the layout comment of csrc/ly_rf3c_bwd.hip: x tile 17 x 17 x 32 fp32,
    # the [288][128 B] operand tile, 64 du rows of 2 O + 16 bytes, the [32][9][8] fp32 table, 256 B; pass C adds the dx tile, a row and a column
    # carry (17 and 2 * 8 * 5 + 2 positions) and the 27 coefficient rows, 32 fp32 each
    assert capi.lib().ly_rf3c_bwd_lds(2, 8, 8, 40, 128) == 289 * 128 + 288 * 128 + 64 * 272 + 32 * 9 * 8 * 4 + 256 + (289 + 17 + 82 + 27) * 128
    assert capi.lib().ly_rf3c_bwd_lds(0, 8, 8, 40, 128) == 289 * 128 + 288 * 128 + 64 * 272 + 32 * 9 * 2 * 4 + 256
    assert capi.lib().ly_rf3c_bwd_lds(3, 8, 8, 40, 128) < 0 and "rf3c_bwd_lds: bad arguments" in err()
