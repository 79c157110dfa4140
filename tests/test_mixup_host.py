"""Host side of mixup in the on-device training augmentation (lead-yolo_amd/mosaic.py, allow_mixup=True): the opt-in, the random stream of
configurations without mixup, the distributions of the second mosaic's draws and of the ratio, the Plan's partner table and LyMixup table, the
blend formula, the ABI additions.  No GPU."""
import ctypes

import numpy as np
import pytest

import lead_yolo_amd as L
from lead_yolo_amd import capi
from lead_yolo_amd import mosaic as MZ

R114 = 0.4105263202137452            # 114 * r + 114 * (1 - r) = 113.99999999999999 in float64


def _bank(n=9, s=64, seed=0):
    rng = np.random.default_rng(seed)
    sizes = [(s, int(rng.integers(s // 4, s + 1))) if i % 2 else (int(rng.integers(s // 4, s + 1)), s) for i in range(n)]
    ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    labels = [np.array([[0, 0.5, 0.5, 0.2, 0.3]] * (i % 4), dtype=np.float32).reshape(-1, 5) for i in range(n)]
    return L.ImageBank(ims, labels, s, device="cpu")


def _fields(d):
    return {k: str(getattr(d, k)) for k in d.__slots__}


def test_opt_in_and_capacity():
    bank = _bank()
    assert bank.max_labels == 3
    aug = L.MosaicAugment(bank, {"mixup": 0.1}, batch_size=5, allow_mixup=True)
    assert aug.capacity == 5 * 8 * 3
    with pytest.raises(NotImplementedError, match="allow_mixup"):
        L.MosaicAugment(bank, {"mixup": 0.1}, batch_size=5)
    assert L.MosaicAugment(bank, {"mixup": 0.0}, batch_size=5, allow_mixup=True).capacity == 5 * 4 * 3     # nothing to mix: as without it


@pytest.mark.parametrize("key,val", [("copy_paste", 0.1), ("perspective", 0.001)])
def test_still_refused_with_the_keyword(key, val):
    with pytest.raises(NotImplementedError, match=key):
        L.MosaicAugment(_bank(), {key: val, "mixup": 0.1}, allow_mixup=True)


def test_stream_unmoved_without_mixup():
    """mixup == 0: the keyword changes no draw and no table byte"""
    bank = _bank()
    hyp = dict(degrees=10.0, shear=5.0, flipud=0.5, mosaic=0.7)
    a, b = L.MosaicAugment(bank, hyp, batch_size=50, seed=7), L.MosaicAugment(bank, hyp, batch_size=50, seed=7, allow_mixup=True)
    da, db = [a.draw(i % len(bank)) for i in range(50)], [b.draw(i % len(bank)) for i in range(50)]
    for x, y in zip(da, db):
        assert _fields(x) == _fields(y) and x.partner is None and x.ratio is None
    pa, pb = a.plan(da), b.plan(db)
    assert bytes(pa.table) == bytes(pb.table) and np.array_equal(pa.luts, pb.luts)
    assert pb.partner_table is None and pb.k == 0 and all(m.partner == -1 for m in pb.mix)


def test_partner_distributions():
    s = 64
    bank = _bank(s=s)
    hyp = dict(mixup=1.0, mosaic=1.0, degrees=10.0, shear=5.0, scale=0.9, translate=0.1)
    aug = L.MosaicAugment(bank, hyp, batch_size=8, seed=3, allow_mixup=True)
    ds = [aug.draw(i % len(bank)) for i in range(2000)]
    for d in ds:
        p = d.partner
        assert d.mosaic and p is not None and p.mosaic and p.partner is None
        assert len(p.sources) == 4 and all(0 <= j < len(bank) for j in p.sources)
        assert s // 2 <= p.xc < 3 * s // 2 and s // 2 <= p.yc < 3 * s // 2
        assert p.gains is None and not p.flipud and not p.fliplr
        assert -10 <= p.degrees <= 10 and 0.1 <= p.scale <= 1.9 and all(-5 <= v <= 5 for v in p.shear) and all(0.4 <= v <= 0.6 for v in p.translate)
        assert 0.0 < d.ratio < 1.0
    r = np.array([d.ratio for d in ds])
    # beta(32, 32): mean 0.5, std sqrt(1 / (4 * 65)) = 0.0620; the mean of 2000 has a standard error of 0.0014
    assert abs(r.mean() - 0.5) <= 0.01 and 0.055 <= r.std() <= 0.069, (r.mean(), r.std())
    # the partner is an independent mosaic: its sources are not tied to the index, its geometry not to the primary's
    assert np.mean([(i % len(bank)) in d.partner.sources for i, d in enumerate(ds)]) < 0.6
    assert all((d.partner.xc, d.partner.degrees, d.partner.scale) != (d.xc, d.degrees, d.scale) for d in ds)
    same = L.MosaicAugment(bank, hyp, batch_size=8, seed=3, allow_mixup=True)
    assert all(_fields(same.draw(i % len(bank)).partner) == _fields(ds[i].partner) for i in range(20))

    none = L.MosaicAugment(bank, dict(mixup=1.0, mosaic=0.0), batch_size=8, seed=3, allow_mixup=True)
    assert all(none.draw(i % len(bank)).partner is None for i in range(500))          # mixup applies to a mosaic only
    tenth = L.MosaicAugment(bank, dict(mixup=0.1), batch_size=8, seed=4, allow_mixup=True)
    share = np.mean([tenth.draw(i % len(bank)).partner is not None for i in range(4000)])
    assert abs(share - 0.1) <= 0.02, share                                            # binomial: sigma = 0.0047


def test_plan_tables():
    bank = _bank()
    hyp = dict(mixup=0.5, degrees=10.0, shear=5.0)
    aug = L.MosaicAugment(bank, hyp, batch_size=16, seed=5, allow_mixup=True)
    draws = [aug.draw(i % len(bank)) for i in range(16)]
    mixed = [b for b, d in enumerate(draws) if d.partner is not None]
    assert 0 < len(mixed) < 16
    plan = aug.plan(draws)
    n = plan.n
    assert n == 16 and len(plan.table) == 16 and len(plan.draws) == 16 and len(plan.mix) == 16 and plan.k == len(plan.partner_table) == len(mixed)
    bare = []
    for d in draws:
        bare.append(MZ.Draw(d.mosaic, d.sources, d.xc, d.yc, d.degrees, d.scale, d.shear, d.translate, d.gains, d.flipud, d.fliplr))
    plain = aug.plan(bare)
    assert bytes(plan.table) == bytes(plain.table) and np.array_equal(plan.luts, plain.luts)
    alone = aug.plan([draws[b].partner for b in mixed])                               # the partners as images of their own
    assert bytes(plan.partner_table) == bytes(alone.table)
    for b, d in enumerate(draws):
        if d.partner is None:
            assert plan.mix[b].partner == -1
        else:
            assert plan.mix[b].partner == n + mixed.index(b) and plan.mix[b].r == d.ratio
    # an augmenter without mixup refuses a draw with a partner: its capacity has no room for the rows
    with pytest.raises(ValueError, match="mixup"):
        L.MosaicAugment(bank, batch_size=16).plan(draws)
    with pytest.raises(ValueError, match="partner"):
        MZ.Draw(False, [0], partner=draws[mixed[0]].partner, ratio=0.5)


def test_blend_is_the_reference_expression():
    rng = np.random.default_rng(6)
    a, b = (rng.integers(0, 256, (37, 41, 3), dtype=np.uint8) for _ in range(2))
    for r in (R114, 0.5, 0.37, float(rng.beta(32.0, 32.0))):
        want = (a * r + b * (1 - r)).astype(np.uint8)
        got = MZ.mixup_blend(a, b, r)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    px = np.array([114], dtype=np.uint8)
    assert int(MZ.mixup_blend(px, px, R114)[0]) == 113 and int(MZ.mixup_blend(px, px, 0.5)[0]) == 114
    full = np.array([255], dtype=np.uint8)
    assert all(int(MZ.mixup_blend(full, full, float(r))[0]) in (254, 255) for r in rng.beta(32.0, 32.0, 200))      # never wraps


def test_abi_additions():
    assert ctypes.sizeof(capi.LyMixup) == 16
    assert [n for n, _ in capi.LyMixup._fields_] == ["partner", "unused", "r"] and capi.LyMixup.r.offset == 8
    P, I = ctypes.c_void_p, ctypes.c_int
    assert capi.SIGNATURES["ly_mosaic_mix_img"] == [P, P, P, I, I, I, P, P]
    assert capi.SIGNATURES["ly_mosaic_mix_labels"] == [P, P, P, I, I, I, I, P, ctypes.c_long, P]
    assert capi.SIGNATURES["ly_mosaic_img"] == [P, P, I, I, P, P] and capi.SIGNATURES["ly_mosaic_labels"] == [P, P, I, I, I, P, ctypes.c_long, P]
