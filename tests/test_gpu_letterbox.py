"""csrc/ly_letterbox.hip (ly_letterbox_u8, ly_scale_boxes) and lead-yolo_amd/predict.py on the device: pixels bit for bit against the integer
contract restated in tests/test_letterbox_host.py (`resize_u8`, `ref_letterbox`) and within one grey level of float64 bilinear, the image
bank built from native images, boxes back to native pixels against torch on the CPU, and Detector end to end against the same pipeline
assembled by hand from the existing pieces."""
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_augment import _model as _synth_model
from tests.test_gpu_modules import _dev
from tests.test_letterbox_host import BATCH, NINE, bilinear64, rand_image, ref_letterbox, resize_u8
from tests.test_metrics_host import LEVELS, best_labels, closed_form, pixel_labels

pytestmark = pytest.mark.gpu
S = 64


def _images(sizes, seed):
    return [rand_image(h, w, seed + i) for i, (h, w) in enumerate(sizes)]


def _want(images, plan):
    return np.stack([ref_letterbox(im, int(plan.nh[i]), int(plan.nw[i]), int(plan.top[i]), int(plan.left[i]), int(plan.H[i]), int(plan.W[i]))
                     for i, im in enumerate(images)])


# ---------------------------------------------------------------------------------------------- 1. pixels
@pytest.mark.parametrize("scaleup", [True, False])
def test_pixels_bit_for_bit(scaleup):
    """one batch onto 64: the nine sizes plus two that put the picture's edges at odd offsets (scaleup=False turns the small ones into copies
    at odd offsets as well).  Equal to the restated contract; inside the picture within < 1.0 of float64 bilinear, an independent reference"""
    import lead_yolo_amd as L
    sizes = BATCH if scaleup else NINE
    images = _images(sizes, 300)
    batch, plan = L.letterbox(images, S, scaleup=scaleup, device=_dev())
    assert batch.dtype == torch.uint8 and tuple(batch.shape) == (len(sizes), 3, S, S) and plan.canvas == (S, S)
    got = batch.cpu().numpy()
    want = _want(images, plan)
    for i in range(len(sizes)):
        assert np.array_equal(got[i], want[i]), (sizes[i], int(np.abs(got[i].astype(int) - want[i]).max()))
    worst = 0.0
    for i, im in enumerate(images):
        nh, nw, top, left = (int(getattr(plan, k)[i]) for k in ("nh", "nw", "top", "left"))
        inside = got[i][::-1, top:top + nh, left:left + nw].transpose(1, 2, 0).astype(np.float64)      # back to HWC BGR
        worst = max(worst, float(np.abs(inside - bilinear64(im, nh, nw)).max()))
        border = np.ones((S, S), bool)
        border[top:top + nh, left:left + nw] = False
        assert (got[i][:, border] == 114).all()
    print(f"kernel vs float64 bilinear inside the picture: max |diff| = {worst:.4f}")
    assert worst < 1.0
    resized = np.array([(h, w) != (int(nh), int(nw)) for (h, w), nh, nw in zip(sizes, plan.nh, plan.nw)])
    odd = (plan.left % 2 == 1) & (plan.nw % 2 == 1)
    assert odd.any() and (plan.top > 0).any() and (~resized).any() and any(h == 1 for h, _ in sizes)
    if scaleup:
        assert (odd & resized).any() and (odd & ~resized).any() and (plan.r > 1).any()


def test_real_sizes():
    import lead_yolo_amd as L
    images = _images([(1080, 1920), (480, 640)], 310)
    batch, plan = L.letterbox(images, 640, device=_dev())
    assert (plan.nh.tolist(), plan.nw.tolist(), plan.top.tolist()) == ([360, 480], [640, 640], [140, 80])
    assert np.array_equal(batch.cpu().numpy(), _want(images, plan))


# ---------------------------------------------------------------------------------------------- 2. the HWC layout: ImageBank.from_native
def test_bank_from_native():
    import lead_yolo_amd as L
    sizes = [(37, 53), (120, 75), (64, 64), (200, 300), (5, 7)]
    images = _images(sizes, 320)
    rng = np.random.default_rng(4)
    labels = [np.concatenate([np.zeros((k, 1)), rng.uniform(0.3, 0.7, (k, 2)), rng.uniform(0.1, 0.4, (k, 2))], 1).astype(np.float32)
              for k in (2, 1, 3, 0, 2)]
    bank = L.ImageBank.from_native(images, labels, S, device=_dev())
    restated = []
    for im in images:
        h0, w0 = im.shape[:2]
        r = S / max(h0, w0)
        restated.append(resize_u8(im, int(h0 * r), int(w0 * r)))                      # load_image: (int(w0 * r), int(h0 * r)), INTER_LINEAR
    assert bank.hw.tolist() == [list(a.shape[:2]) for a in restated] and max(bank.hw.max(1)) == S and len(bank) == 5
    assert any(a.shape[1] % 16 for a in restated) and any(a.shape[0] > h for a, (h, _) in zip(restated, sizes))    # odd widths, an upscale
    data = bank.data.cpu().numpy()
    assert data.size == sum(a.size for a in restated)
    for a, off in zip(restated, bank.off):
        assert np.array_equal(data[off:off + a.size], a.reshape(-1))
    ref = L.ImageBank(restated, labels, S, device=_dev())
    assert torch.equal(bank.data, ref.data) and torch.equal(bank.labels, ref.labels) and bank.max_labels == ref.max_labels
    idx = [0, 1, 2, 3]
    ia, ta = L.MosaicAugment(bank, batch_size=4, seed=3)(idx)
    ib, tb = L.MosaicAugment(ref, batch_size=4, seed=3)(idx)
    assert torch.equal(ia, ib) and torch.equal(ta, tb) and int((ta[:, 0] >= 0).sum()) > 0
    with pytest.raises(ValueError, match="uint8 HWC"):
        L.ImageBank.from_native([images[0].astype(np.float32)], labels[:1], S, device=_dev())


# ---------------------------------------------------------------------------------------------- 3. sources, out=, synchronisation
def test_device_sources_and_out():
    import lead_yolo_amd as L
    dev = _dev()
    images = _images(BATCH[:6], 330)
    want, plan0 = L.letterbox(images, S, device=dev)
    on_dev = [torch.from_numpy(im).to(dev) for im in images]
    got, plan = L.letterbox(on_dev, S)                                    # addressed where they are
    assert torch.equal(got, want) and np.array_equal(plan.shapes, plan0.shapes)
    flipped = np.ascontiguousarray(images[4][:, ::-1])[:, ::-1]            # images[4] again, with a negative stride
    mixed = [on_dev[0], images[1], torch.from_numpy(images[2]), on_dev[3], flipped, on_dev[5]]
    assert torch.equal(L.letterbox(mixed, S)[0], want)
    buf = torch.zeros((8, 3, S, S), dtype=torch.uint8, device=dev)
    out, _ = L.letterbox(images, S, out=buf[1:7])
    assert out.data_ptr() == buf[1].data_ptr() and torch.equal(buf[1:7], want) and not buf[0].any() and not buf[7].any()
    assert torch.equal(plan.shapes_dev.cpu(), torch.from_numpy(plan.shapes)) and torch.equal(plan.val_shapes_dev.cpu(), torch.from_numpy(plan.val_shapes))
    with pytest.raises(ValueError, match="out must be"):
        L.letterbox(images, S, out=buf[:5])
    with pytest.raises(ValueError, match="uint8 HWC"):
        L.letterbox([images[0][:, :, 0]], S, device=dev)
    with pytest.raises(ValueError, match="contiguous"):
        L.letterbox([on_dev[0][:, ::2]], S)
    with pytest.raises(L.capi.HipLibraryError, match="multiple of 16"):
        L.capi.check(L.capi.lib().ly_letterbox_u8(L.capi.ptr(buf), 1, 64, 72, 0, L.capi.stream_ptr()), "ly_letterbox_u8")


def test_no_host_sync():
    import lead_yolo_amd as L
    dev = _dev()
    images = _images(BATCH[:4], 340)
    on_dev = [torch.from_numpy(im).to(dev) for im in images]
    want = L.letterbox(images, S, device=dev)[0]
    buf = torch.empty((4, 3, S, S), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a, _ = L.letterbox(images, S, device=dev)
        b, _ = L.letterbox(on_dev, S, out=buf)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(a, want) and torch.equal(b, want)


# ---------------------------------------------------------------------------------------------- 4. ly_scale_boxes
def _ref_scale_boxes(boxes, shape):
    """utils/general.py scale_boxes with gain and pad given + clip_boxes: the reference's statements, in order, on a float32 CPU tensor"""
    h0, w0, gain, padw, padh = (float(v) for v in shape)
    boxes[..., [0, 2]] -= padw
    boxes[..., [1, 3]] -= padh
    boxes[..., :4] /= gain
    boxes[..., 0].clamp_(0, w0)
    boxes[..., 1].clamp_(0, h0)
    boxes[..., 2].clamp_(0, w0)
    boxes[..., 3].clamp_(0, h0)
    return boxes


def test_scale_boxes_equals_torch_cpu():
    import lead_yolo_amd as L
    rng = np.random.default_rng(8)
    bs, md = 4, 16
    counts = np.array([0, 1, 9, 16], np.int32)
    shapes = np.array([[1080, 1920, 1 / 30, 0.0, 14.0], [33, 65, 64 / 65, 0.0, 15.753846], [240, 320, 0.5, 8.0, 40.0], [100, 150, 0.4, 2.0, 12.0]], np.float32)
    dets = rng.uniform(-6, 70, (bs, md, 6)).astype(np.float32)            # past every border of a 64 x 64 canvas
    dets[..., 4:] = rng.uniform(0, 1, (bs, md, 2))
    # image 2 (gain 0.5, pads 8 / 40): (x - 8) / 0.5 lands exactly on k + 0.5 -> half to even; and on both clamps
    dets[2, 0, :4] = (8 + 1.25, 40 + 1.75, 8 + 2.25, 40 + 2.75)         # 2.5, 3.5, 4.5, 5.5 -> 2, 4, 4, 6
    dets[2, 1, :4] = (8 + 0.25, 40 + 0.75, 7.0, 39.0)                    # 0.5, 1.5 -> 0, 2; the others clamp to 0
    dets[2, 2, :4] = (8 + 160.25, 40 + 120.25, 8 + 159.75, 40 + 119.75)  # past w0 = 320 / h0 = 240 -> the clamp; 319.5, 239.5 -> 320, 240
    dets[1, 0, :4] = (0.0, 15.753846, 64.0, 48.25)
    dev = _dev()
    d, c, s = torch.from_numpy(dets).to(dev), torch.from_numpy(counts).to(dev), torch.from_numpy(shapes).to(dev)
    for rnd in (False, True):
        want = torch.zeros((bs, md, 6))
        for b in range(bs):
            rows = torch.from_numpy(dets[b, :counts[b]].copy())
            _ref_scale_boxes(rows[:, :4], shapes[b])
            if rnd:
                rows[:, :4] = rows[:, :4].round()
            want[b, :counts[b]] = rows
        got = L.scale_boxes(d, c, s, round_boxes=rnd)
        assert got.data_ptr() != d.data_ptr() and torch.equal(d.cpu(), torch.from_numpy(dets))          # the input is untouched
        assert np.array_equal(got.cpu().numpy(), want.numpy()), rnd
        alias = d.clone()
        assert L.scale_boxes(alias, c, s, round_boxes=rnd, out=alias) is alias
        assert np.array_equal(alias.cpu().numpy(), want.numpy()), rnd
        assert not got[0].any() and not got[1, 1:].any() and not got[2, 9:].any()                       # rows past the count are zero
        if rnd:
            assert want[2, 0, :4].tolist() == [2, 4, 4, 6] and want[2, 1, :4].tolist() == [0, 2, 0, 0] and want[2, 2, :4].tolist() == [320, 240, 320, 240]
        lo, hi = (want[..., :4] == 0).sum(), sum(int((want[b, :counts[b], :4] == torch.tensor([w, h, w, h])).sum()) for b, (h, w) in enumerate(shapes[:, :2]))
        assert lo > 3 and hi > 3                                          # boxes straddle both clamps


# ---------------------------------------------------------------------------------------------- 5. ly_val_match after the move of ly_val_native
def test_val_match_native_unchanged():
    """one fixed image scored in native space: correct, match_iou (bits) and match_label against the float32 formulas computed here"""
    import lead_yolo_amd as L
    from tests.test_gpu_metrics import _crafted
    rows, det = _crafted(3)
    shape = np.array([100, 150, 0.4, 2.0, 12.0], np.float32)

    def native(boxes):
        h0, w0, gain, padw, padh = shape
        out = np.asarray(boxes, np.float32).copy()
        out[:, [0, 2]] = np.clip((out[:, [0, 2]] - padw) / gain, np.float32(0), w0)
        out[:, [1, 3]] = np.clip((out[:, [1, 3]] - padh) / gain, np.float32(0), h0)
        return out

    lab = pixel_labels(rows, S, S)
    lab[:, 1:] = native(lab[:, 1:])
    dn = det.copy()
    dn[:, :4] = native(det[:, :4])
    l, best, tied = best_labels(dn, lab)
    assert not tied.any()
    want = closed_form(dn, lab, LEVELS)[0]
    dev = _dev()
    dets = torch.zeros((1, 8, 6), device=dev)
    dets[0, :5] = torch.from_numpy(det).to(dev)
    acc = L.match_padded(dets, torch.tensor([5], dtype=torch.int32, device=dev), torch.from_numpy(rows).to(dev), S,
                         shapes=torch.from_numpy(shape[None]).to(dev), nc=3)
    h = acc.host()
    assert np.array_equal(L.unpack_correct(h.correct[0, :5]), want) and want.any() and not want.all()
    assert np.array_equal(h.match_iou[0, :5].view(np.uint32), best.view(np.uint32))
    assert np.array_equal(h.match_label[0, :5], l)


# ---------------------------------------------------------------------------------------------- 6. Detector end to end
E2E_SIZES = [(37, 53), (120, 75), (97, 131), (64, 64), (200, 300), (33, 65)]
BS, CONF, IOU, MAX_DET = 4, 0.001, 0.45, 300


@functools.lru_cache(maxsize=None)
def _net():
    """lead-yolo-n, random weights of a fixed seed; the heads' biases lifted by 2 (as tools/val_bench.py does) so that a random network
    passes boxes through conf_thres = 0.001"""
    m, st = _synth_model("n", 8100)
    for i in range(len(m.model[-1].m)):
        st[f"model.23.m.{i}.bias"] = st[f"model.23.m.{i}.bias"] + 2.0
    m.load_state_dict(st)
    return m.to(_dev()).eval()


@functools.lru_cache(maxsize=None)
def _e2e_images():
    return tuple(_images(E2E_SIZES, 350))


def _hand_batches(m, augment):
    """the letterboxed chunks the reference's loader would hand over, in the form Detector gives the model: [BS, 3, S, S], free slots 114"""
    import lead_yolo_amd as L
    images = _e2e_images()
    u8 = m.u8_input and not augment
    for lo in range(0, len(images), BS):
        chunk = images[lo:lo + BS]
        plan = L.letterbox_plan([im.shape[:2] for im in chunk], S, stride=int(m.stride.max()))
        batch = np.full((BS, 3, S, S), 114, np.uint8)
        batch[:len(chunk)] = _want(chunk, plan)
        x = torch.from_numpy(batch).to(_dev())
        yield chunk, plan, (x if u8 else x.float() / 255)


def _hand(m, forward, augment=False):
    """restated letterbox -> forward -> L.non_max_suppression -> torch scale_boxes(...).round() on the CPU, image by image"""
    import lead_yolo_amd as L
    out = []
    for chunk, plan, x in _hand_batches(m, augment):
        dets = L.non_max_suppression(forward(x), CONF, IOU, max_det=MAX_DET)
        for i, im in enumerate(chunk):
            d = dets[i].cpu().clone()
            h0, w0 = im.shape[:2]
            gain = min(S / h0, S / w0)                                    # scale_boxes, ratio_pad=None
            _ref_scale_boxes(d[:, :4], (h0, w0, gain, (S - w0 * gain) / 2, (S - h0 * gain) / 2))
            d[:, :4] = d[:, :4].round()
            out.append(d)
    return out


def _same(got, want):
    assert len(got) == len(want) == len(E2E_SIZES)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g.cpu().numpy(), w.numpy()), (i, g.shape, w.shape)
    with_boxes = sum(len(w) > 0 for w in want)
    assert with_boxes >= 4, f"only {with_boxes} of the images have a detection: the seed of _net() is wrong"
    for w, (h0, w0) in zip(want, E2E_SIZES):                              # native pixels: inside the image, whole numbers
        assert (w[:, [0, 2]] <= w0).all() and (w[:, [1, 3]] <= h0).all() and (w[:, :4] >= 0).all() and torch.equal(w[:, :4], w[:, :4].round())


def test_detector_eager_equals_the_pipeline_by_hand():
    import lead_yolo_amd as L
    m = _net()
    with torch.no_grad():
        want = _hand(m, lambda x: m(x)[0])
    det = L.Detector(m, img_size=S, batch_size=BS, conf_thres=CONF, iou_thres=IOU, max_det=MAX_DET, graphed=False)
    assert not det.stale() and det.stride == 32
    _same(det(list(_e2e_images())), want)
    on_dev = [torch.from_numpy(im).to(_dev()) for im in _e2e_images()]
    _same(det(on_dev), want)
    dets, counts, plan = det.padded(on_dev)
    assert tuple(dets.shape) == (6, MAX_DET, 6) and counts.tolist() == [len(w) for w in want] and plan.n == 6
    for i, c in enumerate(counts.tolist()):
        assert not dets[i, c:].any()
    with pytest.raises(RuntimeError, match="eval"):
        L.Detector(torch.nn.Linear(1, 1), img_size=S)                     # a module in training mode
    with pytest.raises(ValueError, match="stride"):
        L.Detector(m, img_size=72, graphed=False)


def test_detector_graphed_equals_the_graph_by_hand():
    import lead_yolo_amd as L
    m = _net()
    example = next(_hand_batches(m, False))[2]
    g = L.GraphedForward(m, example)
    want = _hand(m, lambda x: g(x)[0])
    det = L.Detector(m, img_size=S, batch_size=BS, conf_thres=CONF, iou_thres=IOU, max_det=MAX_DET)
    assert det.graphed and not det.stale()
    _same(det(list(_e2e_images())), want)
    _same(det(list(_e2e_images())), want)                                  # a second pass over the same graph


@pytest.mark.parametrize("graphed", [False, True])
def test_detector_augmented(graphed):
    import lead_yolo_amd as L
    m = _net()
    if graphed:
        g = L.GraphedForward(m, next(_hand_batches(m, True))[2], augment=True)
        forward = lambda x: g(x)[0]                                       # noqa: E731
    else:
        forward = lambda x: m(x, augment=True)[0]                         # noqa: E731
    with torch.no_grad():
        want = _hand(m, forward, augment=True)
    det = L.Detector(m, img_size=S, batch_size=BS, conf_thres=CONF, iou_thres=IOU, max_det=MAX_DET, augment=True, graphed=graphed)
    _same(det(list(_e2e_images())), want)


def test_detector_padded_feeds_the_validator():
    import lead_yolo_amd as L
    m = _net()
    rng = np.random.default_rng(11)
    n = len(E2E_SIZES)
    tg = np.concatenate([np.repeat(np.arange(n), 3)[:, None], np.zeros((3 * n, 1)), rng.uniform(0.3, 0.7, (3 * n, 2)), rng.uniform(0.2, 0.5, (3 * n, 2))],
                        1).astype(np.float32)
    targets = torch.from_numpy(tg).to(_dev())
    det = L.Detector(m, img_size=S, batch_size=BS, conf_thres=CONF, iou_thres=IOU, max_det=MAX_DET, graphed=False)
    dets, counts, plan = det.padded(list(_e2e_images()), native=False)
    v = L.Validator(1, max_det=MAX_DET, capacity_images=n, size=S)
    v.update((dets, counts), targets, shapes=plan.val_shapes)
    # by hand: the same letterboxed batches through model and nms_padded, val.py's shapes from the reference's letterbox numbers
    hd, hc, hs = [], [], []
    with torch.no_grad():
        for chunk, p, x in _hand_batches(m, False):
            d, c, _ = L.nms_padded(m(x)[0], CONF, IOU, max_det=MAX_DET)
            hd.append(d[:len(chunk)])
            hc.append(c[:len(chunk)])
            hs += [(im.shape[0], im.shape[1], int(p.nh[i]) / im.shape[0], (S - int(p.nw[i])) / 2, (S - int(p.nh[i])) / 2) for i, im in enumerate(chunk)]
    assert torch.equal(dets, torch.cat(hd)) and torch.equal(counts, torch.cat(hc))
    v2 = L.Validator(1, max_det=MAX_DET, capacity_images=n, size=S)
    v2.update((torch.cat(hd), torch.cat(hc)), targets, shapes=torch.tensor(hs, dtype=torch.float32))
    a, b = v.stats(), v2.stats()
    assert a[0].shape[0] == int(counts.sum()) > 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # and scoring Detector's native boxes without shapes is not the same thing: the tables matter
    assert not np.array_equal(plan.shapes, plan.val_shapes)


def test_detector_staleness():
    import lead_yolo_amd as L
    from lead_yolo_amd import pack
    m, _ = _synth_model("n", 8100)
    st = _net().state_dict()
    m.load_state_dict({k: v.cpu() for k, v in st.items()})
    m = m.to(_dev()).eval()
    images = list(_e2e_images())
    det = L.Detector(m, img_size=S, batch_size=BS, conf_thres=CONF, iou_thres=IOU, max_det=MAX_DET)
    before = [d.clone() for d in det(images)]
    assert not det.stale()
    with torch.no_grad():
        for i in range(len(m.model[-1].m)):
            m.model[-1].m[i].bias.data[4::m.model[-1].no] -= 1.0             # every anchor's objectness: other confidences, other boxes kept
    pack.touch_weights()
    assert det.stale()
    det.refresh()
    assert not det.stale()
    after = det(images)
    assert any(a.shape != b.shape or not torch.equal(a, b) for a, b in zip(before, after))
    g = L.GraphedForward(m, next(_hand_batches(m, False))[2])              # graph against graph, both captured with the new weights
    want = _hand(m, lambda x: g(x)[0])
    for a, w in zip(after, want):
        assert a.shape == w.shape and np.array_equal(a.cpu().numpy(), w.numpy())
