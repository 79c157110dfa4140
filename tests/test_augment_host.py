"""Augmented inference (augment=True), host side: the pass plan against a restatement of the reference's arithmetic, the dead-layer plan,
and the C ABI of the new kernels."""
import ctypes
import math

import pytest

import lead_yolo_amd as L


# ---- the reference, restated (models/yolo.py _forward_augment / _clip_augmented, utils/torch_utils.py scale_img) ----------------------
def ref_scale_img_size(h, w, ratio, gs):
    if ratio == 1.0:
        return (h, w), (h, w)
    s = (int(h * ratio), int(w * ratio))
    h, w = (math.ceil(v * ratio / gs) * gs for v in (h, w))
    return s, (h, w)


def ref_rows(h, w, strides, na):
    """rows of one _forward_once on an h x w image, per level"""
    return [na * (h // s) * (w // s) for s in strides]


def ref_clip(rows0, rows_last, nl):
    """_clip_augmented: rows dropped from the end of the first pass and from the start of the last"""
    g = sum(4 ** x for x in range(nl))
    e = 1
    i0 = (rows0 // g) * sum(4 ** x for x in range(e))
    i1 = (rows_last // g) * sum(4 ** (nl - 1 - x) for x in range(e))
    return i0, i1


@pytest.fixture(scope="module")
def model_s():
    return L.Model(L.load_cfg(scale="s"))


def test_augment_plan_matches_reference_arithmetic(model_s):
    m = model_s
    det = m.model[-1]
    strides = [int(v) for v in det.stride]
    gs = max(strides)
    sizes = range(64, 1281, 32)
    for h in sizes:
        for w in sizes:
            plan = m.augment_plan(h, w)
            ps = plan["passes"]
            assert len(ps) == 3
            full = []
            for p, si, fi in zip(ps, (1, 0.83, 0.67), (None, 3, None)):
                resized, padded = ref_scale_img_size(h, w, si, gs)
                assert p["resized"] == resized and p["size"] == padded and p["flip"] == (fi == 3) and p["scale"] == si, (h, w, si)
                full.append(ref_rows(*padded, strides, det.na))
            i0, i1 = ref_clip(sum(full[0]), sum(full[-1]), det.nl)
            kept = [sum(full[0]) - i0, sum(full[1]), sum(full[2]) - i1]
            assert [p["rows"] for p in ps] == kept, (h, w)
            assert plan["rows"] == sum(kept)
            assert [p["offset"] for p in ps] == [0, kept[0], kept[0] + kept[1]]
            # the clipped rows are whole levels: the scale-1 pass loses its last, the smallest its first
            assert ps[0]["levels"] == (0, 1) and ps[1]["levels"] == (0, 1, 2) and ps[2]["levels"] == (1, 2)
            for p, rows in zip(ps, full):
                o = p["offset"]
                for i in p["levels"]:
                    assert p["offsets"][i] == o
                    o += rows[i]
                assert o == p["offset"] + p["rows"]
    p640 = m.augment_plan(640, 640)
    assert p640["rows"] == 45147 and [p["rows"] for p in p640["passes"]] == [24000, 18207, 2940]
    assert [p["size"] for p in p640["passes"]] == [(640, 640), (544, 544), (448, 448)]
    assert [p["size"] for p in m.augment_plan(640, 480)["passes"]] == [(640, 480), (544, 416), (448, 352)]


@pytest.mark.parametrize("hw", [(640, 630), (100, 640), (0, 64)])
def test_augment_plan_rejects_sizes_off_the_stride(model_s, hw):
    with pytest.raises(ValueError):
        model_s.augment_plan(*hw)


@pytest.mark.parametrize("scale", ["s", "l"])
def test_dead_layer_plan(scale):
    m = L.Model(L.load_cfg(scale=scale))
    plan = m.augment_plan(640, 640)["passes"]
    assert sorted(m._dead_layers(plan[0]["levels"])) == [20, 21, 22]      # the scale-1 pass drops P5: its branch of the neck
    assert sorted(m._dead_layers(plan[1]["levels"])) == []
    assert sorted(m._dead_layers(plan[2]["levels"])) == []                 # drops P3 only: layer 16 still feeds 17


def test_augment_entry_points_exported():
    lib = ctypes.CDLL(L.capi.LIB_PATH)
    for name in ("ly_scale_img", "ly_detect_level_aug", "ly_detect_tail_aug"):
        assert hasattr(lib, name), name
        assert name in L.capi.SIGNATURES
    assert L.capi.lib().ly_abi_version() >= 4


def test_augment_input_errors_on_host(model_s):
    import torch
    m = model_s.train()
    with pytest.raises(RuntimeError, match="eval"):
        m(torch.zeros(1, 3, 64, 64), augment=True)
    m.eval()
    with pytest.raises(TypeError, match="floating-point"):
        m(torch.zeros(1, 3, 64, 64, dtype=torch.uint8), augment=True)
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 3, 64, 64), profile=True)
