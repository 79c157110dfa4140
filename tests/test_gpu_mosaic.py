"""On-device training augmentation (csrc/ly_mosaic.hip, lead-yolo_amd/mosaic.py) against the reference restated here: load_mosaic / letterbox
canvases, random_perspective's warp (cv2.warpAffine INTER_LINEAR, borderValue 114, restated as fp32 bilinear sampling with the kernel's order of
operations: OpenCV itself samples at 1/32 pixel in fixed point, so this pins the kernel, not cv2 — within 1 level of it), OpenCV's 8-bit HSV
round trip, the flips, the float64 label arithmetic, the captured training step fed by it."""
import copy
import os

import numpy as np
import pytest
import torch

import lead_yolo_amd as L
from lead_yolo_amd import mosaic as MZ
from tests.test_gpu_modules import _dev
from tests.test_mosaic_host import ref_letterbox, ref_mosaic_canvas

pytestmark = pytest.mark.gpu


# ---- the reference, restated ----------------------------------------------------------------------------------------------------------
def ref_warp(canvas, minv, s):
    """warpAffine(canvas, M, (s, s), borderValue=114) sampled at X = minv[0]*u + minv[1]*v + minv[2] (fp32, the kernel's operation order)"""
    a = np.asarray(minv, dtype=np.float32)
    v, u = np.meshgrid(np.arange(s, dtype=np.float32), np.arange(s, dtype=np.float32), indexing="ij")
    X = (a[0] * u + a[1] * v) + a[2]
    Y = (a[3] * u + a[4] * v) + a[5]
    X, Y = np.clip(X, np.float32(-8), np.float32(1e6)), np.clip(Y, np.float32(-8), np.float32(1e6))
    x0, y0 = np.floor(X), np.floor(Y)
    fx, fy = X - x0, Y - y0
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
    H, W = canvas.shape[:2]

    def tap(xx, yy):
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        out = np.full(xx.shape + (3,), 114, dtype=np.float32)
        out[ok] = canvas[yy[ok], xx[ok]].astype(np.float32)
        return out
    p00, p01, p10, p11 = tap(ix, iy), tap(ix + 1, iy), tap(ix, iy + 1), tap(ix + 1, iy + 1)
    wx0, wy0, fx, fy = (1 - fx)[..., None], (1 - fy)[..., None], fx[..., None], fy[..., None]
    acc = wy0 * (wx0 * p00 + fx * p01) + fy * (wx0 * p10 + fx * p11)
    return np.minimum((acc + np.float32(0.5)).astype(np.int64), 255).astype(np.uint8)


def _cv_round_div(n, d):
    q, r = n // d, n % d
    return np.where(2 * r > d, q + 1, np.where(2 * r == d, q + (q & 1), q))


_I = np.arange(256)
SDIV = np.where(_I > 0, _cv_round_div(255 << 12, np.maximum(_I, 1)), 0)
HDIV = np.where(_I > 0, _cv_round_div(180 << 12, 6 * np.maximum(_I, 1)), 0)


def ref_bgr2hsv(im):
    """OpenCV RGB2HSV_b, BGR order, hrange 180"""
    b, g, r = (im[..., k].astype(np.int64) for k in range(3))
    v = np.maximum(np.maximum(b, g), r)
    vmin = np.minimum(np.minimum(b, g), r)
    diff = v - vmin
    vr = np.where(v == r, -1, 0)
    vg = np.where(v == g, -1, 0)
    s = (diff * SDIV[v] + (1 << 11)) >> 12
    h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))))
    h = (h * HDIV[diff] + (1 << 11)) >> 12
    h += np.where(h < 0, 180, 0)
    return h, s, v


def ref_hsv2bgr(h, s, v):
    """OpenCV HSV2RGB_b (float path), BGR order"""
    fh = h.astype(np.float32) * np.float32(6.0 / 180.0)
    fs = s.astype(np.float32) * np.float32(1.0 / 255.0)
    fv = v.astype(np.float32) * np.float32(1.0 / 255.0)
    fh = np.fmod(fh, np.float32(6))
    sector = np.floor(fh).astype(np.int64)
    fh = fh - sector.astype(np.float32)
    bad = (sector < 0) | (sector >= 6)
    sector, fh = np.where(bad, 0, sector), np.where(bad, np.float32(0), fh)
    one = np.float32(1)
    tab = np.stack([fv, fv * (one - fs), fv * (one - fs * fh), fv * (one - fs * (one - fh))], -1)
    sd = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    out = np.take_along_axis(tab, sd[sector], -1)
    out = np.where((fs == 0)[..., None], fv[..., None], out)
    return np.clip(np.rint(out * np.float32(255)), 0, 255).astype(np.uint8)


def ref_hsv(im, lut):
    h, s, v = ref_bgr2hsv(im)
    return ref_hsv2bgr(lut[0][h].astype(np.int64), lut[1][s].astype(np.int64), lut[2][v].astype(np.int64))


def ref_image(plan, b, ims, s):
    """the output image b (CHW RGB) of the restated pipeline"""
    d, e = plan.draws[b], plan.table[b]
    if d.mosaic:
        canvas = ref_mosaic_canvas(s, d.xc, d.yc, [ims[i] for i in d.sources])
    else:
        canvas, _ = ref_letterbox(ims[d.sources[0]], s)
    im = ref_warp(canvas, e.minv[:], s)
    if d.gains is not None:
        im = ref_hsv(im, plan.luts[b])
    if d.flipud:
        im = im[::-1]
    if d.fliplr:
        im = im[:, ::-1]
    return np.ascontiguousarray(im.transpose(2, 0, 1)[::-1])


def ref_labels(plan, bank, s):
    """__getitem__'s label rows + collate_fn's image index, float64, the kernel's formula order"""
    rows = []
    for b, (d, e) in enumerate(zip(plan.draws, plan.table)):
        m = np.array(e.m[:])
        for t in range(4):
            tl = e.tile[t]
            if tl.src < 0:
                continue
            for lb in bank.host_labels[tl.src]:
                w, h = float(tl.w), float(tl.h)
                x1 = w * (lb[1] - lb[3] / 2) + tl.padw
                y1 = h * (lb[2] - lb[4] / 2) + tl.padh
                x2 = w * (lb[1] + lb[3] / 2) + tl.padw
                y2 = h * (lb[2] + lb[4] / 2) + tl.padh
                if d.mosaic:
                    x1, y1, x2, y2 = (min(max(c, 0.0), 2.0 * s) for c in (x1, y1, x2, y2))
                xs = [(m[0] * cx + m[1] * cy) + m[2] for cx, cy in ((x1, y1), (x2, y2), (x1, y2), (x2, y1))]
                ys = [(m[3] * cx + m[4] * cy) + m[5] for cx, cy in ((x1, y1), (x2, y2), (x1, y2), (x2, y1))]
                nx0, nx1 = min(max(min(xs), 0.0), s), min(max(max(xs), 0.0), s)
                ny0, ny1 = min(max(min(ys), 0.0), s), min(max(max(ys), 0.0), s)
                w1, h1 = x2 * d.scale - x1 * d.scale, y2 * d.scale - y1 * d.scale
                w2, h2 = nx1 - nx0, ny1 - ny0
                ar = max(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16))
                if not (w2 > 2 and h2 > 2 and w2 * h2 / (w1 * h1 + 1e-16) > 0.1 and ar < 100):
                    continue
                lim = s - 1e-3
                nx0, nx1, ny0, ny1 = (min(max(c, 0.0), lim) for c in (nx0, nx1, ny0, ny1))
                xc, yc = ((nx0 + nx1) / 2) / s, ((ny0 + ny1) / 2) / s
                if d.flipud:
                    yc = 1 - yc
                if d.fliplr:
                    xc = 1 - xc
                rows.append([b, lb[0], xc, yc, (nx1 - nx0) / s, (ny1 - ny0) / s])
    return np.array(rows, dtype=np.float64).reshape(-1, 6)


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
def _rand_bank(s, n, seed, labels=True, long_side=True):
    rng = np.random.default_rng(seed)
    ims, labs = [], []
    for i in range(n):
        if long_side:
            h, w = (s, int(rng.integers(s // 4, s + 1))) if i % 2 else (int(rng.integers(s // 4, s + 1)), s)
        else:
            h, w = (int(v) for v in rng.integers(4, s + 1, 2))
        base = rng.integers(0, 256, (h // 4 + 2, w // 4 + 2, 3)).astype(np.float64)          # smooth-ish: upsampled noise + fine noise
        im = np.kron(base, np.ones((4, 4, 1)))[:h, :w] + rng.normal(0, 12, (h, w, 3))
        ims.append(np.clip(im, 0, 255).astype(np.uint8))
        k = int(rng.integers(0, 6)) if labels else 0
        xy = rng.uniform(0.05, 0.95, (k, 2))
        wh = rng.uniform(0.02, 0.5, (k, 2))
        labs.append(np.concatenate([rng.integers(0, 3, (k, 1)), xy, wh], 1).astype(np.float32))
    return ims, labs


def _check_labels(plan, bank, targets, s, cap):
    want = ref_labels(plan, bank, s)
    got = targets.cpu().numpy().astype(np.float64)
    k = want.shape[0]
    assert got.shape == (cap, 6)
    np.testing.assert_array_equal(got[:k, :2], want[:, :2])            # the same kept set, in the same order (image, class)
    np.testing.assert_allclose(got[:k, 2:], want[:, 2:], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(got[k:], np.tile([-1, 0, 0, 0, 0, 0], (cap - k, 1)))
    return k


def _check_images(plan, ims, out, s, max_frac=1e-3):
    got = out.cpu().numpy()
    worst, frac = 0, 0.0
    for b in range(plan.n):
        want = ref_image(plan, b, ims, s)
        d = np.abs(got[b].astype(np.int64) - want.astype(np.int64))
        worst, frac = max(worst, int(d.max())), max(frac, float((d > 0).mean()))
    assert worst <= 1 and frac <= max_frac, (worst, frac)
    return worst, frac


# ---- tests ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mosaic", [True, False])
def test_geometry_bit_exact(mosaic):
    """integer translations, scale 1, angle 0, no shear / HSV / flips: the output IS the restated canvas crop — tile placement, 114 fill,
    BGR -> RGB plane order, NCHW layout — for mosaic and letterbox, with random source sizes"""
    s = 320
    ims, labs = _rand_bank(s, 12, 5, long_side=not mosaic)
    bank = L.ImageBank(ims, labs, s, device=_dev())
    aug = L.MosaicAugment(bank, dict(hsv_h=0, hsv_s=0, hsv_v=0), batch_size=8)
    rng = np.random.default_rng(9)
    draws = []
    for b in range(8):
        tr = tuple(0.5 + int(j) / 64 for j in rng.integers(-6, 7, 2))                    # T = translate * 320: integers
        if mosaic:
            xc, yc = (int(v) for v in rng.integers(s // 2, 3 * s // 2, 2))
            draws.append(MZ.Draw(True, [int(v) for v in rng.integers(0, len(ims), 4)], xc, yc, translate=tr))
        else:
            draws.append(MZ.Draw(False, [b], translate=tr))
    plan = aug.plan(draws)
    imgs, tg = aug(plan=plan)
    got = imgs.cpu().numpy()
    for b in range(8):
        d = draws[b]
        canvas = ref_mosaic_canvas(s, d.xc, d.yc, [ims[i] for i in d.sources]) if mosaic else ref_letterbox(ims[b], s)[0]
        ox, oy = (int(round(t * s)) - (s if mosaic else s // 2) for t in d.translate)      # output = canvas shifted by T + C
        pad = np.pad(canvas, ((s, s), (s, s), (0, 0)), constant_values=114)
        crop = pad[s - oy:2 * s - oy, s - ox:2 * s - ox]
        np.testing.assert_array_equal(got[b], crop.transpose(2, 0, 1)[::-1], err_msg=f"image {b}")
    _check_labels(plan, bank, tg, s, aug.capacity)


@pytest.mark.parametrize("mosaic", [True, False])
def test_general_affine(mosaic):
    """degrees, scale, shear, translate: within 1 level of the restatement, at most 1e-3 of the pixels differ; the labels' kept set and
    order are identical, coordinates within 1e-6"""
    s = 320
    ims, labs = _rand_bank(s, 10, 6, long_side=not mosaic)
    bank = L.ImageBank(ims, labs, s, device=_dev())
    hyp = dict(degrees=20.0, scale=0.5, shear=8.0, translate=0.2, hsv_h=0, hsv_s=0, hsv_v=0, mosaic=1.0 if mosaic else 0.0)
    aug = L.MosaicAugment(bank, hyp, batch_size=8, seed=3)
    plan = aug.sample(list(range(8)))
    imgs, tg = aug(plan=plan)
    _check_images(plan, ims, imgs, s)
    assert _check_labels(plan, bank, tg, s, aug.capacity) > 0


def test_hsv():
    """the BGR -> HSV + LUT stage is exact against OpenCV's integer arithmetic restated (all 2^24 colours through the kernel); after
    HSV -> BGR the image is within 1 level of the restatement"""
    s = 4096
    cube = np.arange(1 << 24, dtype=np.int64)
    im = np.stack([cube & 255, (cube >> 8) & 255, cube >> 16], -1).astype(np.uint8).reshape(s, s, 3)
    h, sat, v = ref_bgr2hsv(im)
    assert h.min() >= 0 and h.max() < 180 and sat.max() <= 255
    # every colour, identity geometry, letterbox of one s x s image: the kernel output is the HSV round trip of each pixel
    bank = L.ImageBank([im], [np.zeros((0, 5))], s, device=_dev())
    aug = L.MosaicAugment(bank, dict(mosaic=0.0), batch_size=1)
    ident = [(1.0, 1.0, 1.0), (0.985, 1.7, 0.6), (1.015, 0.3, 1.4)]
    for gains in ident:
        plan = aug.plan([MZ.Draw(False, [0], translate=(0.5, 0.5), gains=gains)])
        out, _ = aug(plan=plan)
        got = out[0].cpu().numpy()[::-1].transpose(1, 2, 0)                # back to HWC BGR
        lut = plan.luts[0]
        want = ref_hsv2bgr(lut[0][h].astype(np.int64), lut[1][sat].astype(np.int64), lut[2][v].astype(np.int64))
        dd = np.abs(got.astype(np.int64) - want.astype(np.int64))
        assert dd.max() <= 1, (gains, int(dd.max()))
        assert (dd > 0).mean() <= 1e-3, (gains, float((dd > 0).mean()))


def test_flips_mirror():
    """the flipped output is the mirror of the unflipped output with otherwise equal parameters; flipped labels are 1 - x / 1 - y"""
    s = 320
    ims, labs = _rand_bank(s, 8, 7)
    bank = L.ImageBank(ims, labs, s, device=_dev())
    aug = L.MosaicAugment(bank, dict(degrees=10.0, shear=3.0), batch_size=4, seed=5)
    base = [aug.draw(i) for i in range(4)]
    outs = {}
    for ud, lr in ((0, 0), (1, 0), (0, 1), (1, 1)):
        ds = [copy.copy(d) for d in base]
        for d in ds:
            d.flipud, d.fliplr = bool(ud), bool(lr)
        im, tg = aug(plan=aug.plan(ds))
        outs[ud, lr] = (im.cpu(), tg.cpu())
    im0, t0 = outs[0, 0]
    assert torch.equal(outs[1, 0][0], im0.flip(2)) and torch.equal(outs[0, 1][0], im0.flip(3)) and torch.equal(outs[1, 1][0], im0.flip(2, 3))
    k = int((t0[:, 0] >= 0).sum())
    assert k > 0
    for (ud, lr), (_, t) in outs.items():
        want = t0.clone()
        if ud:
            want[:k, 3] = 1 - want[:k, 3]
        if lr:
            want[:k, 2] = 1 - want[:k, 2]
        torch.testing.assert_close(t, want, rtol=0, atol=1e-6)


def test_label_edge_cases():
    """an image without labels, a tile whose boxes are all filtered, boxes crossing a tile seam and the 2s clip, letterbox float pads,
    padding rows"""
    s = 64
    rng = np.random.default_rng(8)
    ims = [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in ((64, 64), (64, 41), (37, 64), (64, 64))]
    labs = [np.zeros((0, 5), np.float32),                                                  # no labels
            np.array([[1, 0.5, 0.5, 0.01, 0.01], [2, 0.2, 0.5, 0.9, 0.005]], np.float32),   # both too small / too thin: filtered
            np.array([[0, 0.02, 0.5, 0.3, 0.4], [1, 0.98, 0.02, 0.3, 0.3]], np.float32),   # cross the image edges -> seam / clip
            np.array([[2, 0.5, 0.5, 1.0, 1.0], [0, 0.3, 0.6, 0.2, 0.1]], np.float32)]
    bank = L.ImageBank(ims, labs, s, device=_dev())
    aug = L.MosaicAugment(bank, dict(hsv_h=0, hsv_s=0, hsv_v=0), batch_size=4)
    draws = [MZ.Draw(True, [0, 0, 0, 0], 40, 50),
             MZ.Draw(True, [1, 1, 1, 1], 64, 64, scale=1.0),
             MZ.Draw(True, [2, 3, 2, 3], 33, 90, degrees=7.0, scale=0.8, translate=(0.45, 0.58)),
             MZ.Draw(False, [2], translate=(0.53, 0.47), scale=1.2)]
    plan = aug.plan(draws)
    imgs, tg = aug(plan=plan)
    k = _check_labels(plan, bank, tg, s, aug.capacity)
    got = tg.cpu().numpy()
    assert 0 < k < aug.capacity and not (got[:k, 0] <= 1).any()                           # images 0 and 1 keep nothing
    assert set(got[:k, 0]) == {2.0, 3.0} and plan.table[3].tile[0].padh == 13.5          # letterbox: float half-pad (64 - 37) / 2
    _check_images(plan, ims, imgs, s, max_frac=2e-3)


def _ssdd_bank(s):
    """SSDD crops (tests/golden) cut to varied aspect ratios (long side kept), three channels, labels renormalised to the crop"""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    ims, labs = [], []
    rng = np.random.default_rng(12)
    for f in ("ssdd16.npz", "ssdd_train48_0.npz", "ssdd_train48_1.npz"):
        z = np.load(os.path.join(root, f))
        for i, g in enumerate(z["imgs"]):
            t = z["targets"][z["targets"][:, 0] == i][:, 1:].astype(np.float64)
            short = int(rng.integers(s // 3, s + 1))
            x0 = int(rng.integers(0, s - short + 1))
            gi = g.astype(np.int64)
            im = np.stack([gi, np.clip(gi * 9 // 10 + 10, 0, 255), np.clip(255 - gi // 2, 0, 255)], -1).astype(np.uint8)
            if i % 2:
                im, t = im[:, x0:x0 + short], t.copy()
                t[:, 1] = (t[:, 1] * s - x0) / short
                t[:, 3] = t[:, 3] * s / short
                keep = (t[:, 1] > 0) & (t[:, 1] < 1)
            else:
                im, t = im[x0:x0 + short], t.copy()
                t[:, 2] = (t[:, 2] * s - x0) / short
                t[:, 4] = t[:, 4] * s / short
                keep = (t[:, 2] > 0) & (t[:, 2] < 1)
            ims.append(np.ascontiguousarray(im))
            labs.append(t[keep].astype(np.float32))
    return ims, labs


def test_realistic_ssdd_bank():
    """SSDD images through the whole hyp.scratch-low pipeline (mosaic, scale 0.5, translate 0.1, HSV, fliplr 0.5) at s = 320, bs = 16"""
    s = 320
    ims, labs = _ssdd_bank(s)
    bank = L.ImageBank(ims, labs, s, device=_dev())
    aug = L.MosaicAugment(bank, batch_size=16, seed=1)
    for idx in list(aug.batches(0))[:2]:
        plan = aug.sample(idx)
        imgs, tg = aug(plan=plan)
        _check_images(plan, ims, imgs, s)
        assert _check_labels(plan, bank, tg, s, aug.capacity) > 0


def test_no_host_sync_and_reproducible():
    s = 320
    ims, labs = _rand_bank(s, 10, 13)
    bank = L.ImageBank(ims, labs, s, device=_dev())
    a, b = L.MosaicAugment(bank, batch_size=8, seed=21), L.MosaicAugment(bank, batch_size=8, seed=21)
    idx = list(range(8))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ia, ta = a(idx)
        ia2, ta2 = a(idx)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    ib, tb = b(idx)
    assert torch.equal(ia, ib) and torch.equal(ta, tb)
    assert not torch.equal(ia, ia2)                                   # the generator moved on


def test_graphed_step_fed_through_out():
    """a GraphedTrainStep fed through out=(step.imgs, step.targets): three replays, each loss equal (to 1e-6, an ulp) to an eager train_step
    from the same state fed clones of the tensors the augmenter returned"""
    from lead_yolo_amd import pack
    from tests.test_gpu_adam import _model
    s = 128
    ims, labs = _rand_bank(s, 20, 17)
    labs = [np.concatenate([np.zeros((len(lb), 1), np.float32), lb[:, 1:]], 1) for lb in labs]      # nc = 1
    bank = L.ImageBank(ims, labs, s, device=_dev())
    aug = L.MosaicAugment(bank, batch_size=4, seed=2)
    m = _model()
    opt = L.smart_optimizer(m, "SGD", 1e-3, 0.937, 5e-4, fused=True)
    cl = L.ComputeLoss(m)
    batches = list(aug.batches(0))
    imgs, tg = aug(batches[0])
    step = L.GraphedTrainStep(m, cl, opt, imgs, tg, warmup=2)
    assert tuple(step.targets.shape) == (aug.capacity, 6)

    def state():
        return [v for v in m.state_dict().values() if v.is_floating_point()] + opt.device_state()

    for r in range(3):
        got_imgs, got_tg = aug(batches[1 + r], out=(step.imgs, step.targets))
        assert got_imgs is step.imgs and got_tg is step.targets
        feed = (got_imgs.clone(), got_tg.clone())
        torch.cuda.synchronize()
        saved = [t.clone() for t in state()]
        le, _ = L.train_step(m, cl, opt, *feed)
        le = le.clone()
        torch.cuda.synchronize()
        with torch.no_grad():
            for dst, src in zip(state(), saved):
                dst.copy_(src)
        pack.touch_weights()
        lg, _ = step()
        torch.cuda.synchronize()
        # (the loss's own reductions are float atomics: between two runs of the same step it moves by an ulp at most — test_gpu_adam's bound)
        assert abs(float(le) - float(lg)) <= 1e-6 * abs(float(le)), (r, float(le), float(lg))
        assert float((feed[1][:, 0] >= 0).sum()) > 0
