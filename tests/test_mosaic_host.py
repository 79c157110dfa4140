"""Host side of the on-device training augmentation (lead-yolo_amd/mosaic.py): the parameter table MosaicAugment builds, against the
reference formulas restated here in float64 numpy (utils/dataloaders.py load_mosaic, utils/augmentations.py letterbox / random_perspective /
augment_hsv, torch's DistributedSampler).  No GPU."""
import math

import numpy as np
import pytest
import torch

import lead_yolo_amd as L
from lead_yolo_amd import mosaic as MZ


def _bank(sizes, labels=None, s=64, seed=0):
    rng = np.random.default_rng(seed)
    ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    if labels is None:
        labels = [np.array([[0, 0.5, 0.5, 0.2, 0.3]] * (i % 3), dtype=np.float32).reshape(-1, 5) for i in range(len(sizes))]
    return L.ImageBank(ims, labels, s, device="cpu"), ims


# ---- the reference, restated ------------------------------------------------------------------------------------------------------------
def ref_mosaic_canvas(s, xc, yc, ims):
    """load_mosaic's img4 (utils/dataloaders.py)"""
    img4 = np.full((s * 2, s * 2, 3), 114, dtype=np.uint8)
    for i, img in enumerate(ims):
        h, w = img.shape[:2]
        if i == 0:
            x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
            x1b, y1b, x2b, y2b = w - (x2a - x1a), h - (y2a - y1a), w, h
        elif i == 1:
            x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, s * 2), yc
            x1b, y1b, x2b, y2b = 0, h - (y2a - y1a), min(w, x2a - x1a), h
        elif i == 2:
            x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(s * 2, yc + h)
            x1b, y1b, x2b, y2b = w - (x2a - x1a), 0, w, min(y2a - y1a, h)
        else:
            x1a, y1a, x2a, y2a = xc, yc, min(xc + w, s * 2), min(s * 2, yc + h)
            x1b, y1b, x2b, y2b = 0, 0, min(w, x2a - x1a), min(y2a - y1a, h)
        img4[y1a:y2a, x1a:x2a] = img[y1b:y2b, x1b:x2b]
    return img4


def ref_letterbox(im, s):
    """letterbox(im, s, auto=False) without the resize (r = 1): -> (image, (dw, dh))"""
    h, w = im.shape[:2]
    dw, dh = (s - w) / 2, (s - h) / 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    out = np.pad(im, ((top, bottom), (left, right), (0, 0)), constant_values=114)
    return out, (dw, dh)


def table_canvas(e, bank, size):
    """the canvas a LyMosaicImage entry describes, read the way ly_mosaic_img reads it (tile rectangles, 114 elsewhere)"""
    cv = np.full((size, size, 3), 114, dtype=np.uint8)
    flat = bank.data.numpy()
    for t in range(4):
        tl = e.tile[t]
        if tl.src < 0:
            continue
        src = flat[tl.off:tl.off + tl.h * tl.w * 3].reshape(tl.h, tl.w, 3)
        hh, ww = tl.y2a - tl.y1a, tl.x2a - tl.x1a
        if hh > 0 and ww > 0:
            cv[tl.y1a:tl.y2a, tl.x1a:tl.x2a] = src[tl.y1b:tl.y1b + hh, tl.x1b:tl.x1b + ww]
    return cv


def ref_matrix(im_w, im_h, border, a, sc, shx, shy, tx, ty):
    """random_perspective's M with the draws given (perspective = 0)"""
    height, width = im_h + border * 2, im_w + border * 2
    C = np.eye(3)
    C[0, 2], C[1, 2] = -im_w / 2, -im_h / 2
    R = np.eye(3)
    ang = math.radians(a)
    R[:2] = [[math.cos(ang) * sc, math.sin(ang) * sc, 0], [-math.sin(ang) * sc, math.cos(ang) * sc, 0]]
    S = np.eye(3)
    S[0, 1], S[1, 0] = math.tan(shx * math.pi / 180), math.tan(shy * math.pi / 180)
    T = np.eye(3)
    T[0, 2], T[1, 2] = tx * width, ty * height
    return T @ S @ R @ C


# ---- tests ------------------------------------------------------------------------------------------------------------------------------
def test_mosaic_placement_matches_load_mosaic():
    """the four tile rectangles of many (h, w, xc, yc) — tiles clipped at every canvas edge, portrait / landscape sources, sources smaller
    than s — paint exactly load_mosaic's canvas"""
    s = 64
    rng = np.random.default_rng(1)
    sizes = [(64, 64), (64, 20), (17, 64), (10, 12), (64, 48), (33, 64), (5, 5), (64, 1)]
    bank, ims = _bank(sizes, s=s)
    aug = L.MosaicAugment(bank, batch_size=1)
    cases = [(s // 2, s // 2), (s // 2, 3 * s // 2 - 1), (3 * s // 2 - 1, s // 2), (3 * s // 2 - 1, 3 * s // 2 - 1), (s, s), (1, 127), (127, 1)]
    cases += [tuple(int(v) for v in rng.integers(s // 2, 3 * s // 2, 2)) for _ in range(40)]
    for k, (xc, yc) in enumerate(cases):
        src = [int(v) for v in rng.integers(0, len(sizes), 4)]
        p = aug.plan([MZ.Draw(True, src, xc, yc)])
        e = p.table[0]
        want = ref_mosaic_canvas(s, xc, yc, [ims[i] for i in src])
        np.testing.assert_array_equal(table_canvas(e, bank, 2 * s), want, err_msg=str((xc, yc, src)))
        for t in range(4):
            tl = e.tile[t]
            assert (tl.padw, tl.padh) == (tl.x1a - tl.x1b, tl.y1a - tl.y1b)
            assert tl.src == src[t] and tl.nlab == len(bank.host_labels[src[t]])
            assert 0 <= tl.x1a <= tl.x2a <= 2 * s and 0 <= tl.y1a <= tl.y2a <= 2 * s
            assert 0 <= tl.x1b and tl.x1b + tl.x2a - tl.x1a <= tl.w and 0 <= tl.y1b and tl.y1b + tl.y2a - tl.y1a <= tl.h


def test_letterbox_pads():
    """letterbox(auto=False): the image at (round(dw - 0.1), round(dh - 0.1)) on an s x s canvas of 114, labels shifted by the FLOAT half-pads"""
    s = 64
    sizes = [(64, 64), (64, 33), (64, 34), (21, 64), (64, 1)]
    bank, ims = _bank(sizes, s=s)
    aug = L.MosaicAugment(bank, batch_size=1)
    for i, im in enumerate(ims):
        e = aug.plan([MZ.Draw(False, [i])]).table[0]
        want, (dw, dh) = ref_letterbox(im, s)
        assert want.shape == (s, s, 3)
        np.testing.assert_array_equal(table_canvas(e, bank, s), want)
        assert (e.tile[0].padw, e.tile[0].padh) == (dw, dh) and e.mosaic == 0
        assert all(e.tile[t].src == -1 for t in (1, 2, 3))
    big, _ = _bank([(64, 40), (40, 50)], s=64)
    aug = L.MosaicAugment(big, batch_size=1)
    with pytest.raises(ValueError, match="load_image"):
        aug.plan([MZ.Draw(False, [1])])                  # long side 50 != 64: letterbox would resize


@pytest.mark.parametrize("mosaic", [True, False])
def test_matrix_and_inverse(mosaic):
    """M = T @ S @ R @ C of random_perspective with its border (-s/2 for mosaic), m = M[:2] in float64, minv = the float64 inverse in fp32"""
    s = 64
    bank, _ = _bank([(64, 64)] * 4, s=s)
    aug = L.MosaicAugment(bank, batch_size=1)
    rng = np.random.default_rng(4)
    for _ in range(20):
        a, sc, shx, shy, tx, ty = rng.uniform(-30, 30), rng.uniform(0.5, 1.5), rng.uniform(-10, 10), rng.uniform(-10, 10), *rng.uniform(0.3, 0.7, 2)
        d = MZ.Draw(mosaic, [0, 1, 2, 3] if mosaic else [0], s, s, a, sc, (shx, shy), (tx, ty))
        p = aug.plan([d])
        e = p.table[0]
        want = ref_matrix(2 * s, 2 * s, -s // 2, a, sc, shx, shy, tx, ty) if mosaic else ref_matrix(s, s, 0, a, sc, shx, shy, tx, ty)
        np.testing.assert_allclose(np.array(e.m[:]).reshape(2, 3), want[:2], rtol=1e-14, atol=1e-12)
        inv = np.linalg.inv(want)[:2]
        np.testing.assert_allclose(np.array(e.minv[:], dtype=np.float64).reshape(2, 3), inv, rtol=1e-6, atol=1e-4)
        np.testing.assert_array_equal(np.array(e.minv[:], dtype=np.float32), MZ.invert_affine(want).reshape(-1).astype(np.float32))
        assert e.scale == sc


def test_hsv_luts_match_augment_hsv():
    for r in ([1.0, 1.0, 1.0], [0.985, 1.7, 0.6], [1.015, 0.3, 1.4], [0.99, 0.0, 2.0]):
        r = np.array(r)
        x = np.arange(0, 256, dtype=r.dtype)
        want = [((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8), np.clip(x * r[2], 0, 255).astype(np.uint8)]
        np.testing.assert_array_equal(MZ.hsv_luts(r), np.stack(want))


def test_sampler_ranges_and_seed():
    s = 64
    bank, _ = _bank([(64, 64), (40, 64), (64, 20)] * 3, s=s)
    hyp = dict(degrees=10.0, shear=5.0, translate=0.1, scale=0.5, flipud=0.5, fliplr=0.5, mosaic=0.5)
    a, b = L.MosaicAugment(bank, hyp, batch_size=8, seed=7), L.MosaicAugment(bank, hyp, batch_size=8, seed=7)
    ds = [a.draw(i % len(bank)) for i in range(400)]
    db = [b.draw(i % len(bank)) for i in range(400)]
    for x, y in zip(ds, db):
        assert {k: str(getattr(x, k)) for k in x.__slots__} == {k: str(getattr(y, k)) for k in y.__slots__}
    mos = [d for d in ds if d.mosaic]
    assert 120 < len(mos) < 280
    for i, d in enumerate(ds):
        assert -10 <= d.degrees <= 10 and 0.5 <= d.scale <= 1.5 and all(-5 <= v <= 5 for v in d.shear)
        assert all(0.4 <= v <= 0.6 for v in d.translate)
        assert np.all(np.abs(d.gains - 1) <= [0.015, 0.7, 0.4])
        if d.mosaic:
            assert len(d.sources) == 4 and (i % len(bank)) in d.sources and all(0 <= j < len(bank) for j in d.sources)
            assert s // 2 <= d.xc < 3 * s // 2 and s // 2 <= d.yc < 3 * s // 2
        else:
            assert d.sources == [i % len(bank)]
    assert 120 < sum(d.fliplr for d in ds) < 280 and 120 < sum(d.flipud for d in ds) < 280
    c = L.MosaicAugment(bank, hyp, batch_size=8, seed=8)
    assert [c.draw(0).degrees for _ in range(5)] != [ds[0].degrees] + [a.draw(0).degrees for _ in range(4)]
    off = L.MosaicAugment(bank, dict(hsv_h=0, hsv_s=0, hsv_v=0), batch_size=2)
    p = off.sample([0, 1])
    assert all(d.gains is None for d in p.draws) and not p.luts.any()


@pytest.mark.parametrize("n,world", [(40, 4), (37, 3), (10, 1)])
def test_batches_shard_like_distributed_sampler(n, world):
    bank, _ = _bank([(32, 32)] * n, s=32)
    aug = L.MosaicAugment(bank, batch_size=3, seed=11)
    for epoch in (0, 1):
        shards = []
        for r in range(world):
            smp = torch.utils.data.DistributedSampler(range(n), num_replicas=world, rank=r, shuffle=True, seed=11)
            smp.set_epoch(epoch)
            want = list(smp)
            got = list(aug.batches(epoch, rank=r, world_size=world))
            assert all(len(b) == 3 for b in got) and len(got) == len(want) // 3
            assert sum(got, []) == want[:len(got) * 3]
            shards.append(want)
        allidx = sum(shards, [])
        assert set(allidx) == set(range(n))                           # covering
        if n % world == 0:
            assert len(allidx) == len(set(allidx))                    # disjoint
    assert list(aug.batches(0)) != list(aug.batches(1))


def test_capacity_bound():
    labels = [np.zeros((k, 5), np.float32) for k in (0, 3, 7, 1)]
    bank, _ = _bank([(32, 32)] * 4, labels=labels, s=32)
    assert bank.max_labels == 7
    aug = L.MosaicAugment(bank, batch_size=5)
    assert aug.capacity == 5 * 4 * 7
    empty, _ = _bank([(32, 32)] * 2, labels=[np.zeros((0, 5))] * 2, s=32)
    assert L.MosaicAugment(empty, batch_size=2).capacity == 2 * 4          # at least one row per tile: the target tensor is never empty


@pytest.mark.parametrize("key,val", [("mixup", 0.1), ("copy_paste", 0.1), ("perspective", 0.001)])
def test_not_implemented(key, val):
    bank, _ = _bank([(32, 32)], s=32)
    with pytest.raises(NotImplementedError, match=key):
        L.MosaicAugment(bank, {key: val})


def test_bank_layout_and_rgb():
    rng = np.random.default_rng(2)
    ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((32, 20), (7, 32), (32, 32))]
    bank = L.ImageBank(ims, [np.zeros((0, 5))] * 3, 32, bgr=False, device="cpu")
    flat = bank.data.numpy()
    for i, im in enumerate(ims):
        h, w = bank.hw[i]
        np.testing.assert_array_equal(flat[bank.off[i]:bank.off[i] + h * w * 3].reshape(h, w, 3), im[..., ::-1])

    class DS:                                             # the duck-typed reference dataset
        img_size = 32
        labels = [np.array([[0, 0.5, 0.5, 0.1, 0.1]], np.float32)] * 3

        def __len__(self):
            return 3

        def load_image(self, i):
            return ims[i], (0, 0), ims[i].shape[:2]

    b2 = L.ImageBank.from_dataset(DS(), device="cpu")
    assert b2.max_labels == 1 and b2.labels.dtype == torch.float64 and tuple(b2.labels.shape) == (3, 5)
    np.testing.assert_array_equal(b2.data.numpy()[:32 * 20 * 3], ims[0].reshape(-1))
