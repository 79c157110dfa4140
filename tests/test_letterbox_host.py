"""The host side of the detect input path (lead-yolo_amd/predict.py letterbox_plan, the C ABI of csrc/ly_letterbox.hip) and the premise of the
device tests: the pixel contract of ly_letterbox_u8, restated here in numpy integers, against float64 half-pixel bilinear interpolation.
No GPU.  tests/test_gpu_letterbox.py holds the kernel to `resize_u8` / `ref_letterbox` of this file bit for bit."""
import ctypes
import re

import numpy as np
import pytest

from lead_yolo_amd import capi
from lead_yolo_amd import predict as P

SIZES = [(37, 53), (120, 75), (97, 131), (64, 64), (200, 300), (33, 65), (128, 128), (5, 7), (1, 9), (1080, 1920), (480, 640)]
NINE = SIZES[:9]
# two more for the device batch: onto 64 the nine give even `left` and `nw` only; (96, 50) is resized to 64 x 33 at left = 15, (64, 37) is a copy at
# left = 13 — the 16-byte groups of the kernel then straddle the picture's edges at odd offsets
BATCH = NINE + [(96, 50), (64, 37)]


# ---- the reference's letterbox arithmetic (utils/augmentations.py letterbox, scaleFill=False), its statements in its order ---------------
def ref_plan(shape, new_shape, auto, scaleup, stride=32):
    new_shape = (new_shape, new_shape)
    r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
    if not scaleup:
        r = min(r, 1.0)
    new_unpad = int(round(shape[1] * r)), int(round(shape[0] * r))
    dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]
    if auto:
        dw, dh = np.mod(dw, stride), np.mod(dh, stride)
    dw /= 2
    dh /= 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return dict(r=r, nw=new_unpad[0], nh=new_unpad[1], dw=float(dw), dh=float(dh), top=top, left=left, H=new_unpad[1] + top + bottom,
                W=new_unpad[0] + left + right)


def ref_detect_shape(canvas, shape0):
    """scale_boxes(img1_shape = canvas, boxes, img0_shape = shape0, ratio_pad=None): its gain and pad (utils/general.py)"""
    gain = min(canvas[0] / shape0[0], canvas[1] / shape0[1])
    pad = (canvas[1] - shape0[1] * gain) / 2, (canvas[0] - shape0[0] * gain) / 2
    return shape0[0], shape0[1], gain, pad[0], pad[1]


# ---- the pixel contract of ly_letterbox_u8 (include/lead_yolo_hip.h), in numpy integers ---------------------------------------------------
def taps(n_dst, n_src):
    """per destination index: the two source indices and their 11-bit weights"""
    d = np.arange(n_dst, dtype=np.float64)
    scale = 1.0 / (np.float64(n_dst) / n_src)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    assert f.dtype == np.float32
    lo, hi = s < 0, s >= n_src - 1
    s[lo], f[lo] = 0, 0
    s[hi], f[hi] = n_src - 1, 0
    c1 = np.rint(f * np.float32(2048)).astype(np.int64)                   # np.rint: half to even
    c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, n_src - 1), c0, c1


def resize_u8(src, nh, nw):
    """[h0, w0, 3] uint8 -> [nh, nw, 3] uint8"""
    h0, w0 = src.shape[:2]
    if (nh, nw) == (h0, w0):
        return src.copy()
    x0, x1, a0, a1 = taps(nw, w0)
    y0, y1, b0, b1 = taps(nh, h0)
    S = src.astype(np.int64)
    a0, a1, b0, b1 = a0[None, :, None], a1[None, :, None], b0[:, None, None], b1[:, None, None]
    r0 = S[y0][:, x0] * a0 + S[y0][:, x1] * a1
    r1 = S[y1][:, x0] * a0 + S[y1][:, x1] * a1
    out = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def ref_letterbox(src, nh, nw, top, left, H, W):
    """the canvas LoadImages.__next__ hands to the model: [3, H, W] uint8, RGB planes"""
    canvas = np.full((H, W, 3), 114, np.uint8)
    canvas[top:top + nh, left:left + nw] = resize_u8(src, nh, nw)
    return np.ascontiguousarray(canvas.transpose(2, 0, 1)[::-1])


def bilinear64(src, nh, nw):
    """half-pixel-centre bilinear interpolation in float64 with the coordinates clamped to the image: written independently of `taps`"""
    h0, w0 = src.shape[:2]
    y = np.clip((np.arange(nh) + 0.5) * (h0 / nh) - 0.5, 0, h0 - 1)
    x = np.clip((np.arange(nw) + 0.5) * (w0 / nw) - 0.5, 0, w0 - 1)
    yi, xi = np.minimum(np.floor(y).astype(int), max(h0 - 2, 0)), np.minimum(np.floor(x).astype(int), max(w0 - 2, 0))
    fy, fx = (y - yi)[:, None, None], (x - xi)[None, :, None]
    yj, xj = np.minimum(yi + 1, h0 - 1), np.minimum(xi + 1, w0 - 1)
    S = src.astype(np.float64)
    return (1 - fy) * ((1 - fx) * S[yi][:, xi] + fx * S[yi][:, xj]) + fy * ((1 - fx) * S[yj][:, xi] + fx * S[yj][:, xj])


def rand_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- letterbox_plan ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("new_shape", [64, 96, 640])
@pytest.mark.parametrize("auto", [False, True])
@pytest.mark.parametrize("scaleup", [False, True])
def test_letterbox_plan_is_the_reference_arithmetic(new_shape, auto, scaleup):
    for hw in SIZES:
        p = P.letterbox_plan([hw], new_shape, auto=auto, scaleup=scaleup, stride=32)
        w = ref_plan(hw, new_shape, auto, scaleup)
        assert p.n == 1 and (int(p.h0[0]), int(p.w0[0])) == hw
        got = {k: int(getattr(p, k)[0]) for k in ("nh", "nw", "top", "left", "H", "W")}
        assert got == {k: w[k] for k in got}, (hw, got, w)
        assert (p.r[0], p.dw[0], p.dh[0]) == (w["r"], w["dw"], w["dh"])
        assert 1 <= got["nh"] <= got["H"] - got["top"] and 1 <= got["nw"] <= got["W"] - got["left"]
        if auto:
            assert got["H"] % 32 == 0 and got["W"] % 32 == 0 and got["H"] <= new_shape and got["W"] <= new_shape
        else:
            assert got["H"] == got["W"] == new_shape
        assert p.canvas == (got["H"], got["W"])
        assert p.shapes.dtype == p.val_shapes.dtype == np.float32 and p.shapes.shape == p.val_shapes.shape == (1, 5)
        assert np.array_equal(p.shapes[0], np.array(ref_detect_shape((w["H"], w["W"]), hw), np.float32)), hw
        assert np.array_equal(p.val_shapes[0], np.array((hw[0], hw[1], w["nh"] / hw[0], w["dw"], w["dh"]), np.float32)), hw
        assert p.shapes_dev is None and p.val_shapes_dev is None


def test_letterbox_plan_of_a_batch():
    p = P.letterbox_plan(SIZES, 64)
    assert p.n == len(SIZES) and p.canvas == (64, 64)
    for i, hw in enumerate(SIZES):
        one = P.letterbox_plan([hw], 64)
        for k in P.LetterboxPlan._INT + P.LetterboxPlan._FLT:
            assert getattr(p, k)[i] == getattr(one, k)[0]
        assert np.array_equal(p.shapes[i], one.shapes[0]) and np.array_equal(p.val_shapes[i], one.val_shapes[0])
    both = P.LetterboxPlan.concat([P.letterbox_plan(SIZES[:4], 64), P.letterbox_plan(SIZES[4:], 64)])
    assert np.array_equal(both.shapes, p.shapes) and np.array_equal(both.top, p.top) and both.n == p.n
    # the cases the device test relies on: odd left, odd nw (resized and copied), top > 0, a copy, an upscale, a 1-row source
    pb = P.letterbox_plan(BATCH, 64)
    resized = [(h, w) != (nh, nw) for (h, w), nh, nw in zip(BATCH, pb.nh, pb.nw)]
    odd = (pb.left % 2 == 1) & (pb.nw % 2 == 1)
    assert (odd & resized).any() and (odd & ~np.array(resized)).any() and (pb.top > 0).any()
    assert not all(resized) and (pb.r > 1).any() and any(h == 1 for h, _ in BATCH)


def test_auto_with_two_canvases_raises():
    with pytest.raises(ValueError, match=r"33 x 65.*32 x 64.*37 x 53.*64 x 64"):          # names the two shapes
        P.letterbox_plan([(37, 53), (120, 75), (33, 65)], 64, auto=True)
    assert P.letterbox_plan([(37, 53), (74, 106), (120, 75)], 64, auto=True).canvas == (64, 64)
    assert P.letterbox_plan([(33, 65)], 64, auto=True).canvas == (32, 64)
    with pytest.raises(ValueError):
        P.letterbox_plan([(1, 200)], 64)                                  # would be resized to 0 rows
    with pytest.raises(ValueError):
        P.letterbox_plan([], 64)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_letterbox_entries():
    assert ctypes.sizeof(capi.LyLetterboxImage) == 48
    assert [n for n, _ in capi.LyLetterboxImage._fields_] == ["src", "dst", "h0", "w0", "H", "W", "nh", "nw", "top", "left"]
    P_, I = ctypes.c_void_p, ctypes.c_int
    assert capi.SIGNATURES["ly_letterbox_u8"] == [P_, I, I, I, I, P_] and capi.RESTYPES["ly_letterbox_u8"] is I
    assert capi.SIGNATURES["ly_scale_boxes"] == [P_, P_, I, I, P_, I, P_, P_] and capi.RESTYPES["ly_scale_boxes"] is I
    hdr = re.sub(r"/\*.*?\*/", " ", open(capi.HEADER_PATH).read(), flags=re.S)
    enum = dict(re.findall(r"(LY_LB_\w+)\s*=\s*(\d+)", hdr))
    assert enum == {"LY_LB_CHW_RGB": str(P.LB_CHW_RGB), "LY_LB_HWC_BGR": str(P.LB_HWC_BGR)}


# ---- premise of the device test's bound ----------------------------------------------------------------------------------------------------
def test_restated_contract_is_bilinear_within_one_grey_level():
    """the integer contract against float64 bilinear on the size pairs of the device test's batch (worst case measured: 0.78): the device test may
    then hold the kernel's pixels to `< 1.0` of float64 bilinear without hiding anything"""
    plan = P.letterbox_plan(BATCH, 64)
    worst = 0.0
    for i, (h0, w0) in enumerate(BATCH):
        src = rand_image(h0, w0, 100 + i)
        nh, nw = int(plan.nh[i]), int(plan.nw[i])
        got = resize_u8(src, nh, nw)
        assert got.shape == (nh, nw, 3) and got.dtype == np.uint8
        worst = max(worst, float(np.abs(got.astype(np.float64) - bilinear64(src, nh, nw)).max()))
    print(f"restated contract vs float64 bilinear: max |diff| = {worst:.4f}")
    assert worst < 1.0


def test_restated_contract_identity_and_exact_halving():
    src = rand_image(64, 64, 5)
    assert np.array_equal(resize_u8(src, 64, 64), src)
    x0, x1, a0, a1 = taps(64, 64)                                         # the general path is the identity too at equal sizes
    assert np.array_equal(x0, np.arange(64)) and (a0 == 2048).all() and (a1 == 0).all()
    big = rand_image(128, 128, 6)
    s = big.astype(np.int64)
    mean = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
    assert np.array_equal(resize_u8(big, 64, 64), mean.astype(np.uint8))
    row = rand_image(1, 9, 7)                                             # a 1-row source: both vertical taps are row 0
    up = resize_u8(row, 7, 64)
    assert (up == up[:1]).all()
