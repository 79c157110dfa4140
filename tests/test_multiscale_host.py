"""Multi-scale training, host side: the reference's size draw and resized shape (train.py:308-313) restated, the float64 judge of the
resize kernel against CPU F.interpolate and against planted defects (tests/multiscale_ref.py), and the generated binding."""
import ctypes
import math
import random

import pytest
import torch
import torch.nn.functional as F

import lead_yolo_amd as L
from tests import multiscale_ref as R


class CountingRandom(random.Random):
    """a random.Random that counts its randrange calls"""
    calls = 0

    def randrange(self, *a, **k):
        self.calls += 1
        return super().randrange(*a, **k)


@pytest.mark.parametrize("imgsz", [640, 256])
def test_multi_scale_size_draws_the_reference_sequence(imgsz):
    gs = 32
    ours, ref = CountingRandom(5), random.Random(5)
    for i in range(200):
        want = ref.randrange(int(imgsz * 0.5), int(imgsz * 1.5) + gs) // gs * gs           # train.py:309
        assert L.multi_scale_size(imgsz, gs, ours) == want
        assert ours.calls == i + 1
    assert ours.getstate() == ref.getstate()


def test_multi_scale_size_uses_the_module_generator_by_default():
    random.seed(11)
    want = [random.randrange(320, 960 + 32) // 32 * 32 for _ in range(5)]
    random.seed(11)
    assert [L.multi_scale_size(640) for _ in range(5)] == want


def test_multi_scale_size_covers_320_to_960():
    rng = random.Random(0)
    seen = {L.multi_scale_size(640, 32, rng) for _ in range(2000)}
    assert seen == set(range(320, 961, 32)) and len(seen) == 21


def test_multi_scale_shape():
    for base in (640, 256):
        for sz in range(base // 2, base * 3 // 2 + 1, 32):
            assert L.multi_scale_shape((base, base), sz) == (sz, sz)
    assert L.multi_scale_shape((192, 256), 160) == (128, 160)
    assert L.multi_scale_shape((192, 256), 256) == (192, 256)                               # sf == 1: the batch's own shape
    assert L.multi_scale_shape((200, 256), 256) == (200, 256)                               # ... even when it is off the grid
    for (h, w), sz in [((192, 256), 384), ((480, 640), 352), ((640, 480), 928)]:           # the reference's lines, literally
        sf = sz / max(h, w)
        assert L.multi_scale_shape((h, w), sz) == tuple(math.ceil(x * sf / 32) * 32 for x in (h, w))


# ---- the judge ------------------------------------------------------------------------------------------------------------------------
def test_bound_values():
    assert abs(R.bound(640, 640) - 2.45e-4) < 1e-6 and abs(R.bound(128, 128) - 3.1e-5) < 1e-6


@pytest.mark.parametrize("src,dst", R.CASES)
def test_interpolate_lies_within_the_bound_of_the_judge(src, dst):
    x = R.noise((2, 3, *src), 100 + src[0] + dst[0])
    got = F.interpolate(x.float() / 255, size=dst, mode="bilinear", align_corners=False)
    err = R.max_err(got, R.resize_f64(x, dst))
    assert err <= R.bound(*src), (src, dst, err, R.bound(*src))


@pytest.mark.parametrize("src,dst", [((128, 128), (96, 96)), ((128, 128), (192, 192)), ((96, 160), (64, 96)), ((96, 160), (128, 224)), ((640, 640), (960, 960))])
def test_planted_defects_exceed_the_bound(src, dst):
    x = R.noise((1, 3, *src), 7 + dst[0])
    want, b = R.resize_f64(x, dst), R.bound(*src)
    xf = x.float() / 255
    defects = {
        "half-pixel shift": torch.from_numpy(R.resize_f64(x, dst, shift=0.5)).float(),
        "align_corners=True": F.interpolate(xf, size=dst, mode="bilinear", align_corners=True),
        "missing / 255": F.interpolate(x.float(), size=dst, mode="bilinear", align_corners=False),
        "nearest": F.interpolate(xf, size=dst, mode="nearest"),
    }
    if src[0] != src[1]:
        defects["swapped axes"] = torch.from_numpy(R.resize_f64(x, dst, swap=True)).float()
    for name, got in defects.items():
        assert R.max_err(got, want) > 100 * b, (name, src, dst)
    assert R.max_err(torch.from_numpy(want).float(), want) <= b                             # (and the judge rounded to fp32 passes)


# ---- the binding ----------------------------------------------------------------------------------------------------------------------
def test_generated_binding_holds_resize_u8():
    P, I = ctypes.c_void_p, ctypes.c_int
    assert L.capi.SIGNATURES["ly_resize_u8"] == [P, I, I, I, I, P, I, I, P]                  # the header's nine parameters
    assert L.capi.RESTYPES["ly_resize_u8"] is I
    assert hasattr(ctypes.CDLL(L.capi.LIB_PATH), "ly_resize_u8")
    assert L.capi.lib().ly_abi_version() == 5


def test_resize_u8_refuses_host_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.ops.resize_u8(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), (16, 16))
