"""Mixup in the on-device training augmentation (csrc/ly_mosaic.hip ly_mosaic_mix_img / ly_mosaic_mix_labels, lead-yolo_amd/mosaic.py with
allow_mixup=True).  The blend is held to the reference's bytes: the expected image is `mixup_blend` (the reference's numpy expression: float64,
truncated) of the two renders the plain kernel gives for the two mosaics, and the kernel's output must equal it exactly.  The restatements of
the pipeline come from tests/test_gpu_mosaic.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lead_yolo_amd as L
from lead_yolo_amd import capi
from lead_yolo_amd import mosaic as MZ
from tests import test_gpu_mosaic as TM
from tests.test_gpu_modules import _dev

pytestmark = pytest.mark.gpu

S = 64
R114 = 0.4105263202137452            # 114 * r + 114 * (1 - r) = 113.99999999999999 in float64: the shared border comes out as 113
NO_HSV = dict(hsv_h=0, hsv_s=0, hsv_v=0)
PAD = [-1, 0, 0, 0, 0, 0]


def _bare(d, gains=None):
    """the draw without its partner"""
    return MZ.Draw(d.mosaic, d.sources, d.xc, d.yc, d.degrees, d.scale, d.shear, d.translate, gains, d.flipud, d.fliplr)


def _no_gains(d):
    return MZ.Draw(d.mosaic, d.sources, d.xc, d.yc, d.degrees, d.scale, d.shear, d.translate, None, d.flipud, d.fliplr, d.partner, d.ratio)


def _as_primary(d):
    """the partner of d as an image of its own, with d's flips (HSV and the flips act on the blended image)"""
    p = d.partner
    return MZ.Draw(True, p.sources, p.xc, p.yc, p.degrees, p.scale, p.shear, p.translate, None, d.flipud, d.fliplr)


class Case:
    """a bank of 10 images (long side 64, 0 to 5 labels each; image 0 has none) and a batch of 6 explicit draws, partners yes, no, yes, yes,
    no, no; the renders of the primaries and of the partners through the PLAIN augmenter (the kernel as it was before mixup), once"""

    def __init__(self):
        s = S
        self.ims, self.labs = TM._rand_bank(s, 10, 31)
        self.labs[0] = np.zeros((0, 5), np.float32)
        assert max(len(lb) for lb in self.labs) >= 3
        self.bank = L.ImageBank(self.ims, self.labs, s, device=_dev())
        rng = np.random.default_rng(32)

        def mosaic(sources=None, scale=None, translate=None, **kw):
            xc, yc = (int(v) for v in rng.integers(s // 2, 3 * s // 2, 2))
            return MZ.Draw(True, sources or [int(v) for v in rng.integers(0, 10, 4)], xc, yc, float(rng.uniform(-15, 15)),
                           scale or float(rng.uniform(0.5, 0.9)), tuple(float(v) for v in rng.uniform(-6, 6, 2)),
                           translate or tuple(float(v) for v in rng.uniform(0.35, 0.65, 2)), **kw)

        gains = [rng.uniform(-1, 1, 3) * [0.015, 0.7, 0.4] + 1 for _ in range(6)]
        flips = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 1), (1, 0)]
        # image 0: scale 0.5 for both mosaics and both pushed left, so the columns at the right are warpAffine's 114 border in both
        # image 2: a primary of four copies of the image without labels, a partner with labels
        spec = [dict(scale=0.5, translate=(0.38, 0.5), partner=mosaic(scale=0.5, translate=(0.36, 0.52)), ratio=R114),
                dict(),
                dict(sources=[0, 0, 0, 0], partner=mosaic(sources=[1, 2, 3, 4], scale=0.9, translate=(0.5, 0.5)), ratio=float(rng.beta(32.0, 32.0))),
                dict(partner=mosaic(), ratio=float(rng.beta(32.0, 32.0))),
                dict(), dict()]
        self.draws = [mosaic(gains=gains[b], flipud=bool(flips[b][0]), fliplr=bool(flips[b][1]), **kw) for b, kw in enumerate(spec)]
        self.mixed = [b for b, d in enumerate(self.draws) if d.partner is not None]
        assert self.mixed == [0, 2, 3]
        self.plain = L.MosaicAugment(self.bank, NO_HSV, batch_size=6)
        self.mix = L.MosaicAugment(self.bank, dict(mixup=1.0), batch_size=6, allow_mixup=True)
        assert self.mix.capacity == 2 * self.plain.capacity == 6 * 8 * self.bank.max_labels
        self.plan1 = self.plain.plan([_bare(d) for d in self.draws])                          # primaries, no HSV, their own flips
        self.plan2 = self.plain.plan([_as_primary(self.draws[b]) for b in self.mixed])        # partners, their primaries' flips
        self.render1 = self.plain(plan=self.plan1)[0].cpu().numpy()
        self.render2 = self.plain(plan=self.plan2)[0].cpu().numpy()
        self.blend = self.render1.copy()                                                      # the exact expectation without HSV
        for k, b in enumerate(self.mixed):
            self.blend[b] = MZ.mixup_blend(self.render1[b], self.render2[k], self.draws[b].ratio)
        for a in (self.render1, self.render2, self.blend):
            a.setflags(write=False)

    def want_labels(self):
        """per image the primary plan's rows, then the partner plan's (image index b)"""
        r1, r2 = TM.ref_labels(self.plan1, self.bank, S), TM.ref_labels(self.plan2, self.bank, S)
        rows = []
        for b in range(6):
            rows.append(r1[r1[:, 0] == b])
            if b in self.mixed:
                part = r2[r2[:, 0] == self.mixed.index(b)].copy()
                part[:, 0] = b
                rows.append(part)
        return np.concatenate(rows), r1, r2


@functools.lru_cache(None)
def _case():
    return Case()


def _diff(got, want):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    return int(d.max()), float((d > 0).mean())


def test_blend_bit_exact():
    c = _case()
    # premise: image 0 has pixels where both renders are the 114 border, and the reference's float64 blend truncates them to 113
    both = (c.render1[0] == 114).all(0) & (c.render2[0] == 114).all(0)
    assert both.sum() >= S and (c.blend[0][:, both] == 113).all()
    assert 114 * R114 + 114 * (1 - R114) < 114
    imgs, _ = c.mix(plan=c.mix.plan([_no_gains(d) for d in c.draws]))
    got = imgs.cpu().numpy()
    for b in range(6):
        np.testing.assert_array_equal(got[b], c.blend[b], err_msg=f"image {b}")
    # and against the restated pipeline (fp32 warp of the restated canvases, blended on the host): the plain kernel's bound
    worst, frac = 0, 0.0
    for b in range(6):
        want = TM.ref_image(c.plan1, b, c.ims, S)
        if b in c.mixed:
            want = MZ.mixup_blend(want, TM.ref_image(c.plan2, c.mixed.index(b), c.ims, S), c.draws[b].ratio)
        w, f = _diff(got[b], want)
        worst, frac = max(worst, w), max(frac, f)
    print(f"mixup vs restated pipeline: worst {worst}, differing share {frac:.2e}")
    assert worst <= 1 and frac <= 1e-3, (worst, frac)


def test_blend_then_hsv():
    """gains on every image: the HSV step acts on the blended image"""
    c = _case()
    plan = c.mix.plan(c.draws)
    assert all(d.gains is not None for d in c.draws)
    got = c.mix(plan=plan)[0].cpu().numpy()
    worst, frac = 0, 0.0
    for b in range(6):
        bgr = np.ascontiguousarray(c.blend[b][::-1].transpose(1, 2, 0))                       # CHW RGB -> HWC BGR; HSV is per pixel
        want = TM.ref_hsv(bgr, plan.luts[b]).transpose(2, 0, 1)[::-1]
        w, f = _diff(got[b], want)
        worst, frac = max(worst, w), max(frac, f)
    print(f"mixup + HSV: worst {worst}, differing share {frac:.2e}")
    assert worst <= 1 and frac <= 1e-3, (worst, frac)


def test_labels_primary_then_partner():
    c = _case()
    want, r1, r2 = c.want_labels()
    # premise: image 2's primary keeps nothing, its partner keeps some
    assert (r1[:, 0] == 2).sum() == 0 and (r2[:, 0] == c.mixed.index(2)).sum() > 0 and len(r2) > 0 and len(r1) > 0
    _, tg = c.mix(plan=c.mix.plan(c.draws))
    got = tg.cpu().numpy().astype(np.float64)
    k, cap = len(want), c.mix.capacity
    assert got.shape == (cap, 6) and 0 < k < cap
    np.testing.assert_array_equal(got[:k, :2], want[:, :2])                 # the same kept set, in the same order (image, class)
    np.testing.assert_allclose(got[:k, 2:], want[:, 2:], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(got[k:], np.tile(PAD, (cap - k, 1)))


def test_no_partner_is_the_plain_kernels():
    """the mix entry points on a batch without partners: the plain entry points' bytes (HSV included), padding up to the doubled capacity"""
    c = _case()
    draws = [_bare(d, d.gains) for d in c.draws]
    plain = L.MosaicAugment(c.bank, batch_size=6)
    plan = c.mix.plan(draws)
    assert plan.k == 0 and all(m.partner == -1 for m in plan.mix)
    i0, t0 = plain(plan=plain.plan(draws))
    i1, t1 = c.mix(plan=plan)
    assert torch.equal(i0, i1) and torch.equal(t0, t1[:plain.capacity])
    assert int((t0[:, 0] >= 0).sum()) > 0
    np.testing.assert_array_equal(t1[plain.capacity:].cpu().numpy(), np.tile(PAD, (c.mix.capacity - plain.capacity, 1)).astype(np.float32))


def test_capacity_is_checked_before_the_launch():
    c = _case()
    plan = c.mix.plan(c.draws)
    tab = c.mix.upload(plan)
    n, ml = plan.n, c.bank.max_labels
    cap = n * 8 * ml - 1
    tg = torch.full((n * 8 * ml, 6), 7.0, device=_dev())
    mp = tab.data_ptr() + (n + plan.k) * ctypes.sizeof(capi.LyMosaicImage)
    torch.cuda.synchronize()
    with pytest.raises(capi.HipLibraryError, match=rf"capacity {cap} < n_img \* 8 \* max_labels = {cap + 1}"):
        capi.check(capi.lib().ly_mosaic_mix_labels(capi.ptr(c.bank.labels), tab.data_ptr(), mp, n, n + plan.k, S, ml, capi.ptr(tg), cap,
                                                   capi.stream_ptr()), "ly_mosaic_mix_labels")
    with pytest.raises(capi.HipLibraryError, match="n_entry"):
        capi.check(capi.lib().ly_mosaic_mix_labels(capi.ptr(c.bank.labels), tab.data_ptr(), mp, n, n - 1, S, ml, capi.ptr(tg), cap + 1,
                                                   capi.stream_ptr()), "ly_mosaic_mix_labels")
    torch.cuda.synchronize()
    assert bool((tg == 7.0).all())                                          # nothing ran


def test_no_host_sync_and_reproducible():
    c = _case()
    hyp = dict(mixup=1.0, degrees=10.0, shear=4.0, scale=0.9)
    a, b = (L.MosaicAugment(c.bank, hyp, batch_size=6, seed=21, allow_mixup=True) for _ in range(2))
    idx = list(range(6))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ia, ta = a(idx)
        ia2, _ = a(idx)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    ib, tb = b(idx)
    assert torch.equal(ia, ib) and torch.equal(ta, tb)
    assert not torch.equal(ia, ia2)                                         # the generator moved on


def test_graphed_step_with_doubled_targets():
    """a GraphedTrainStep constructed with targets of the doubled capacity, fed one mixup batch through out=: its loss equals (to 1e-6, the
    bound of test_gpu_mosaic's fed step) an eager train_step from the same state"""
    from lead_yolo_amd import pack
    from tests.test_gpu_adam import _model
    s = 128
    ims, labs = TM._rand_bank(s, 20, 17)
    labs = [np.concatenate([np.zeros((len(lb), 1), np.float32), lb[:, 1:]], 1) for lb in labs]      # nc = 1
    bank = L.ImageBank(ims, labs, s, device=_dev())
    aug = L.MosaicAugment(bank, dict(mixup=1.0), batch_size=4, seed=2, allow_mixup=True)
    assert aug.capacity == 4 * 8 * bank.max_labels
    m = _model()
    opt = L.smart_optimizer(m, "SGD", 1e-3, 0.937, 5e-4, fused=True)
    cl = L.ComputeLoss(m)
    batches = list(aug.batches(0))
    imgs, tg = aug(batches[0])
    step = L.GraphedTrainStep(m, cl, opt, imgs, tg, warmup=2)
    assert tuple(step.targets.shape) == (aug.capacity, 6)

    def state():
        return [v for v in m.state_dict().values() if v.is_floating_point()] + opt.device_state()

    plan = aug.sample(batches[1])
    assert plan.k == 4
    got_imgs, got_tg = aug(plan=plan, out=(step.imgs, step.targets))
    assert got_imgs is step.imgs and got_tg is step.targets
    feed = (got_imgs.clone(), got_tg.clone())
    torch.cuda.synchronize()
    primary_rows = len(TM.ref_labels(aug.plan([_bare(d) for d in plan.draws]), bank, s))
    assert int((feed[1][:, 0] >= 0).sum()) > primary_rows > 0                # rows of the partners are in the targets
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
    assert abs(float(le) - float(lg)) <= 1e-6 * abs(float(le)), (float(le), float(lg))
