"""Multi-scale training on the device: the resize kernel (csrc/ly_augment.hip ly_resize_u8) against the float64 judge of
tests/multiscale_ref.py, `img_size=` on the eager step, and MultiScaleTrainStep — per-size captured steps on one memory pool — bit for
bit against the eager loop.  The model tests train lead-yolo-n at bs = 2 from base size 256 (draw range 128 ... 384)."""
import copy
import ctypes
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lead_yolo_amd as L
from lead_yolo_amd import capi, ops, pack
from oracle import functional as OF
from oracle import synth
from tests import multiscale_ref as R
from tests.test_gpu_adam import _cfg, _model
from tests.test_gpu_modules import _dev

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
# + odd source height and a source width off 16; the kernel's other tap path: a source narrower than a tap window, a scale beyond 5
KERNEL_CASES = [(2, 3, *src, *dst) for src, dst in R.CASES] + [(3, 1, 37, 52, 32, 64), (2, 3, 9, 6, 24, 16), (1, 3, 40, 100, 8, 16)]


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,c,h,w,ho,wo", KERNEL_CASES)
def test_resize_u8_against_float64(n, c, h, w, ho, wo):
    x = R.noise((n, c, h, w), 300 + h + ho)
    want, b = R.resize_f64(x, (ho, wo)), R.bound(h, w)
    xd = x.to(_dev())
    got = ops.resize_u8(xd, (ho, wo))
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, c, ho, wo) and got.is_contiguous()
    err = R.max_err(got, want)
    aten = F.interpolate(xd.float() / 255, size=(ho, wo), mode="bilinear", align_corners=False)
    d_aten, e_aten = float((got - aten).abs().max()), R.max_err(aten, want)
    print(f"resize_u8 {h}x{w} -> {ho}x{wo}: |hip - f64| {err:.3e}  |aten(device) - f64| {e_aten:.3e}  |hip - aten(device)| {d_aten:.3e}  bound {b:.3e}")
    assert err <= b, (err, b)
    assert d_aten <= 2 * b, (d_aten, b)                     # both sides lie within the bound of the exact result
    # out=: into a preallocated buffer (guard elements on both sides stay untouched)
    buf = torch.full((n * c * ho * wo + 8,), -7.0, device=_dev())
    out = buf[4:-4].view(n, c, ho, wo)
    assert ops.resize_u8(xd, (ho, wo), out=out) is out
    assert torch.equal(out, got) and bool((buf[:4] == -7).all()) and bool((buf[-4:] == -7).all())


def test_resize_u8_inside_a_captured_graph():
    n, c, h, w, ho, wo = 2, 3, 96, 160, 128, 224
    src = R.noise((n, c, h, w), 41).to(_dev())
    out = torch.empty((n, c, ho, wo), device=_dev())
    ops.resize_u8(src, (ho, wo), out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.resize_u8(src, (ho, wo), out=out)
    for seed in (42, 43):
        x = R.noise((n, c, h, w), seed)
        src.copy_(x.to(_dev()))
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert R.max_err(out, R.resize_f64(x, (ho, wo))) <= R.bound(h, w)


def test_resize_u8_rejections():
    x = torch.zeros((1, 3, 8, 8), dtype=torch.uint8, device=_dev())
    with pytest.raises(capi.HipLibraryError, match="multiple of 4"):
        ops.resize_u8(x, (8, 6))
    buf = torch.empty(3 * 8 * 8 + 4, device=_dev())
    with pytest.raises(capi.HipLibraryError, match="16-byte aligned"):
        ops.resize_u8(x, (8, 8), out=buf[1:1 + 3 * 64].view(1, 3, 8, 8))
    with pytest.raises(TypeError, match="uint8"):
        ops.resize_u8(x.float(), (8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resize_u8(x.cpu(), (8, 8))
    with pytest.raises(ValueError, match="out must be"):
        ops.resize_u8(x, (8, 8), out=torch.empty((1, 3, 8, 12), device=_dev()))
    # sizes at or beyond 2^31 elements: the launcher refuses before it launches (the small buffers are never touched)
    out = torch.empty(64, device=_dev())
    lib, P = capi.lib(), ctypes.c_void_p
    for args in [(1, 3, 8, 8, 32768, 32768),               # output 3 * 2^30
                 (2, 1, 8, 8, 32768, 32768),               # output exactly 2^31
                 (1, 2, 32768, 32768, 8, 8)]:              # source exactly 2^31
        n, c, h, w, ho, wo = args
        with pytest.raises(capi.HipLibraryError, match="too large"):
            capi.check(lib.ly_resize_u8(P(x.data_ptr()), n, c, h, w, P(out.data_ptr()), ho, wo, capi.stream_ptr()), "ly_resize_u8")
    with pytest.raises(capi.HipLibraryError, match="null pointer"):
        capi.check(lib.ly_resize_u8(P(0), 1, 3, 8, 8, P(out.data_ptr()), 8, 8, capi.stream_ptr()), "ly_resize_u8")
    torch.cuda.synchronize()


# ---- 2. the training step ----------------------------------------------------------------------------------------------------------------
def _targets(bs, seed, per_image, cap=None):
    """synthetic targets, padded to `cap` rows with rows whose image index is -1"""
    t = synth.synth_targets(bs, seed, per_image=per_image)
    if cap is not None:
        pad = torch.zeros((cap - t.shape[0], 6))
        pad[:, 0] = -1
        t = torch.cat([t, pad])
    return t.to(_dev())


class _Run:
    """model + fused SGD + EMA + loss, and the snapshot / restore of everything a step changes (test_configs2_full_size_graphed_step's)"""

    def __init__(self, seed=5151):
        self.m = _model(seed)
        self.opt = L.smart_optimizer(self.m, "SGD", 0.01, 0.937, 5e-4)
        self.ema = L.ModelEMA(self.m)
        self.cl = L.ComputeLoss(self.m)

    def tensors(self):
        m, ema, opt = self.m, self.ema, self.opt
        return ({k: v for k, v in m.state_dict().items() if v.is_floating_point()},
                {k: v for k, v in ema.ema.state_dict().items() if v.is_floating_point()},
                {n: opt.state[p]["momentum_buffer"] for n, p in m.named_parameters() if p in opt.state})

    def snap(self):
        torch.cuda.synchronize()
        return [{k: v.detach().clone() for k, v in d.items()} for d in self.tensors()], self.opt._table["hyper"].clone(), self.ema.updates

    def restore(self, s):
        with torch.no_grad():
            for live, saved in zip(self.tensors(), s[0]):
                for k, v in live.items():
                    v.copy_(saved[k])
            self.opt._table["hyper"].copy_(s[1])
        self.ema.updates = s[2]
        pack.touch_weights()

    def eager(self, imgs, tg, amp=None, **kw):
        return L.train_step(self.m, self.cl, self.opt, imgs, tg, ema=self.ema, amp=amp, **kw)[0]


def _same_bits(a, b, what):
    for wi, name in enumerate(("weights", "EMA", "momentum")):
        bad = [k for k in a[0][wi] if not torch.equal(a[0][wi][k], b[0][wi][k])]
        assert not bad, (what, name, len(bad), bad[:6])
        assert all(bool(torch.isfinite(v).all()) for v in a[0][wi].values()), (what, name)
    assert torch.equal(a[1], b[1]), (what, "hyper", a[1], b[1])
    assert a[2] == b[2], (what, "ema.updates")


def _moved(a, b):
    return sum(int(not torch.equal(a[0][0][k], b[0][0][k])) for k in a[0][0])


@pytest.fixture(scope="module")
def eager_run():
    r = _Run()
    imgs = synth.synth_images(2, 256, 77).to(_dev())
    tg = _targets(2, 78, 5)
    r.eager(imgs, tg)                                       # the optimiser's table and momentum buffers exist from here on
    return r, imgs, tg, r.snap()


def test_eager_img_size_equals_resizing_first(eager_run):
    r, imgs, tg, s0 = eager_run
    r.restore(s0)
    r.eager(imgs, tg, img_size=(128, 128))
    a = r.snap()
    r.restore(s0)
    r.eager(ops.resize_u8(imgs, (128, 128)), tg)
    b = r.snap()
    _same_bits(a, b, "img_size=(128, 128) vs train_step on resize_u8's result")
    assert _moved(a, s0) > 100
    r.restore(s0)
    r.eager(imgs, tg, img_size=128)                         # one int: a square
    _same_bits(a, r.snap(), "img_size=128")


def test_eager_img_size_of_the_batch_is_todays_uint8_step(eager_run):
    r, imgs, tg, s0 = eager_run
    r.restore(s0)
    r.eager(imgs, tg, img_size=(256, 256))
    a = r.snap()
    r.restore(s0)
    r.eager(imgs, tg)
    _same_bits(a, r.snap(), "img_size = the batch's size vs the uint8 step")
    with pytest.raises(ValueError, match="uint8"):
        r.eager(imgs.float() / 255, tg, img_size=(128, 128))
    r.restore(s0)


@pytest.mark.parametrize("size", [128, 384])
def test_eager_img_size_first_loss_against_the_oracle(eager_run, size):
    r, imgs, tg, s0 = eager_run
    r.restore(s0)
    so = {k: v.detach().cpu().clone() for k, v in r.m.state_dict().items()}
    loss = float(r.eager(imgs, tg, img_size=(size, size)))
    r.restore(s0)
    x = F.interpolate(imgs.cpu().float() / 255, size=(size, size), mode="bilinear", align_corners=False)
    with torch.no_grad():
        want, _ = OF.compute_loss(OF.model_forward(copy.deepcopy(so), _cfg("n"), x, r.m.stride, training=True), tg.cpu(), r.m.model[-1].anchors.cpu(), nc=1)
    assert abs(loss - float(want)) <= 1e-3 * abs(float(want)), (size, loss, float(want))


def _batches(k, bs=2, base=(256, 256), cap=14):
    """k changing batches with padded targets"""
    return [(R.noise((bs, 3, *base), 900 + i).to(_dev()), _targets(bs, 950 + i, 3 + i % 5, cap)) for i in range(k)]


def _against_eager(r, step, batches, sizes, amp, base):
    """the object over `sizes`, then the eager img_size= loop from the same state: same bits everywhere, every loss to 1e-5"""
    s0 = r.snap()
    got = []
    for (imgs, tg), sz in zip(batches, sizes):
        got.append(float(step(imgs, tg, size=sz)[0]))
        assert step.last_size == sz
    a = r.snap()
    r.restore(s0)
    want = [float(r.eager(imgs, tg, amp=amp, img_size=L.multi_scale_shape(base, sz))) for (imgs, tg), sz in zip(batches, sizes)]
    b = r.snap()
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.isfinite(g) and abs(g - w) <= 1e-5 * abs(w), (i, sizes[i], g, w)
    _same_bits(a, b, f"MultiScaleTrainStep vs the eager loop over {sizes}")
    assert _moved(a, s0) > 100
    assert a[2] == s0[2] + len(sizes)


@pytest.mark.parametrize("amp", [None, BF])
def test_multiscale_step_equals_the_eager_loop(amp):
    """first-use captures in the middle of training that leave no trace, replays in another order than the capture order on the shared pool,
    the identity size on the uint8 path, a return to an earlier size"""
    r = _Run()
    sizes = [256, 128, 384, 128, 320, 256]
    batches = _batches(len(sizes) + 1)
    step = L.MultiScaleTrainStep(r.m, r.cl, r.opt, *batches[-1], ema=r.ema, amp=amp, warmup=1, img_size=256, seed=0)
    assert step.graphed_sizes == [(256, 256)]
    _against_eager(r, step, batches, sizes, amp, (256, 256))
    assert step.graphed_sizes == [(256, 256), (128, 128), (384, 384), (320, 320)]
    assert all(s.graph.pool() == step._pool for s in step._steps.values())


def test_multiscale_step_non_square():
    r = _Run()
    base = (192, 256)
    batches = _batches(4, base=base)
    step = L.MultiScaleTrainStep(r.m, r.cl, r.opt, *batches[-1], ema=r.ema, warmup=1, img_size=256)
    _against_eager(r, step, batches, [160, 256, 160], None, base)
    assert step.graphed_sizes == [(192, 256), (128, 160)]


def test_multiscale_step_max_graphs():
    r = _Run()
    sizes = [128, 384, 128, 384, 256]
    batches = _batches(len(sizes) + 1)
    step = L.MultiScaleTrainStep(r.m, r.cl, r.opt, *batches[-1], ema=r.ema, warmup=1, img_size=256, max_graphs=2)
    _against_eager(r, step, batches, sizes, None, (256, 256))
    assert step.graphed_sizes == [(256, 256), (128, 128)]  # 384, the third distinct size, ran eager


def test_multiscale_capture_ahead_leaves_no_trace():
    r = _Run()
    (imgs, tg), = _batches(1)
    step = L.MultiScaleTrainStep(r.m, r.cl, r.opt, imgs, tg, ema=r.ema, warmup=2, img_size=256, max_graphs=2)
    s0 = r.snap()
    assert step.capture(384) and step.graphed_sizes == [(256, 256), (384, 384)]
    _same_bits(r.snap(), s0, "capture(384)")
    assert not step.capture(128) and step.capture(384) and len(step.graphed_sizes) == 2      # max_graphs reached / already there
    _same_bits(r.snap(), s0, "capture at the limit")
    with pytest.raises(ValueError, match="multiple of the grid size"):
        step.capture(130)


def test_multiscale_step_draws_as_the_reference():
    r = _Run()
    (imgs, tg), = _batches(1)
    step = L.MultiScaleTrainStep(r.m, r.cl, r.opt, imgs, tg, ema=r.ema, warmup=1, img_size=256, seed=3, max_graphs=1)
    ref = random.Random(3)
    for _ in range(8):
        step(imgs, tg)
        assert step.last_size == L.multi_scale_size(256, 32, ref)
    step(imgs, tg, size=128)                                # consumes nothing from the generator
    assert step.last_size == 128 and step.rng.getstate() == ref.getstate()
    step(imgs, tg)
    assert step.last_size == L.multi_scale_size(256, 32, ref)
    assert bool(torch.isfinite(step(imgs, tg)[0]))


def test_multiscale_step_errors():
    r = _Run()
    (imgs, tg), = _batches(1)
    args = (r.m, r.cl, r.opt, imgs, tg)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        L.MultiScaleTrainStep(*args, reducer=object())
    with pytest.raises(NotImplementedError, match="accumulate"):
        L.MultiScaleTrainStep(*args, accumulate=2)
    with pytest.raises(ValueError, match="uint8"):
        L.MultiScaleTrainStep(r.m, r.cl, r.opt, imgs.float() / 255, tg)
    step = L.MultiScaleTrainStep(*args, warmup=1, img_size=256, max_graphs=1)
    with pytest.raises(ValueError, match="shape"):
        step(imgs[:, :, :128], tg)
    with pytest.raises(ValueError, match="dtype"):
        step(imgs.float(), tg)
    with pytest.raises(ValueError, match="targets"):
        step(imgs, tg[:-1])
    with pytest.raises(ValueError, match="multiple of the grid size"):
        step(imgs, tg, size=100)
    # GraphedTrainStep's own input buffer stays the uint8 batch at its own size, whatever img_size is
    g = L.GraphedTrainStep(r.m, r.cl, r.opt, imgs, tg, warmup=1, img_size=(128, 128))
    assert g.imgs.dtype == torch.uint8 and tuple(g.imgs.shape) == tuple(imgs.shape)
    with pytest.raises(ValueError, match="shape"):
        g(ops.resize_u8(imgs, (128, 128)), tg)
    assert bool(torch.isfinite(g(imgs, tg)[0]))


def test_multiscale_step_fed_by_the_augmenter():
    from tests.test_gpu_mosaic import _rand_bank
    s = 256
    ims, labs = _rand_bank(s, 12, 17)
    labs = [np.concatenate([np.zeros((len(lb), 1), np.float32), lb[:, 1:]], 1) for lb in labs]      # nc = 1
    aug = L.MosaicAugment(L.ImageBank(ims, labs, s, device=_dev()), batch_size=2, seed=2)
    r = _Run()
    batches = list(aug.batches(0))
    step = L.MultiScaleTrainStep(r.m, r.cl, r.opt, *aug(batches[0]), ema=r.ema, warmup=1, img_size=s)
    s0 = r.snap()
    for b, sz in zip(batches[1:3], (128, 384)):
        got_imgs, got_tg = aug(b, out=(step.imgs, step.targets))
        assert got_imgs is step.imgs and got_tg is step.targets
        assert np.isfinite(float(step(size=sz)[0]))
    assert step.graphed_sizes == [(256, 256), (128, 128), (384, 384)]
    assert _moved(r.snap(), s0) > 100
