"""csrc/ly_metrics.hip (ly_val_match, ly_val_advance) and lead-yolo_amd/metrics.py on the device against the oracle's process_batch /
mean_results: per-image matching on the smallest shapes that can still go wrong, native-space scoring, the capacity guards, accumulation
over batches, replay from a captured graph, and the SSDD fixture end to end."""
import os

import numpy as np
import pytest
import torch

from oracle import metrics as OMET
from oracle import synth
from tests.test_gpu_modules import _cfg, _dev
from tests.test_metrics_host import LEVELS, best_labels, closed_form, crowded_case, pixel_labels

pytestmark = pytest.mark.gpu
S, MAX_DET = 64, 300
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssdd16.npz")


def _crafted(nc):
    """labels A, B (class 0, overlapping) and C (class 1 when nc > 1); d0, d1 on A (only d0 may be correct), d2 with best label A (0.71,
    taken by d0) that also overlaps the free label B (0.64: it must stay incorrect), d3 on C with the wrong class, d4 on C"""
    c1 = 1.0 if nc > 1 else 0.0
    boxes = np.array([[10, 10, 30, 30], [18, 10, 38, 30], [40, 40, 60, 60]], np.float32)
    rows = np.array([[0, c, (b[0] + b[2]) / 2 / S, (b[1] + b[3]) / 2 / S, (b[2] - b[0]) / S, (b[3] - b[1]) / S] for c, b in zip((0, 0, c1), boxes)],
                    np.float32)
    dets = np.array([[10, 10, 30, 30.5, 0.9, 0], [10, 11, 30, 30, 0.8, 0], [13, 10, 34, 30, 0.7, 0], [40, 40, 60, 60.5, 0.6, 0],
                     [40, 40.5, 60, 60, 0.5, c1]], np.float32)
    return rows, dets


def _batch(nc, seed, bs=8):
    """per image (label rows, detections); image 0: no detections, 1: no labels, 2: neither, 3: max_det detections, 4: 300 labels,
    5: the crafted cases, the rest crowded"""
    rng = np.random.default_rng(seed)
    plan = {0: (9, 0), 1: (0, 30), 2: (0, 0), 3: (40, MAX_DET), 4: (300, 120)}
    out = []
    for b in range(bs):
        if b == 5:
            out.append(_crafted(nc))
        else:
            n_lab, n_det = plan.get(b, (int(rng.integers(3, 41)), int(rng.integers(50, 290))))
            out.append(crowded_case(rng, nc, n_lab, n_det, size=float(S)))
    return out


def _to_device(images, seed, pad_rows=0):
    """dets [bs, MAX_DET, 6], counts, targets with the rows of all images interleaved in a seeded random order (row order inside an image
    kept or not does not matter to the caller: it reads the rows back through the returned permutation), plus `pad_rows` padding rows"""
    bs = len(images)
    dets = np.zeros((bs, MAX_DET, 6), np.float32)
    counts = np.zeros(bs, np.int32)
    rows = []
    for b, (lab, det) in enumerate(images):
        dets[b, :len(det)] = det
        counts[b] = len(det)
        lab = lab.copy()
        lab[:, 0] = b
        rows.append(lab)
    rows = np.concatenate(rows + [np.concatenate([np.full((pad_rows, 1), -1.0), np.zeros((pad_rows, 5))], 1).astype(np.float32)])
    rows = rows[np.random.default_rng(seed).permutation(len(rows))]
    dev = _dev()
    return torch.from_numpy(dets).to(dev), torch.from_numpy(counts).to(dev), torch.from_numpy(rows).to(dev), rows


def _check_rows(h, slot0, rows, dets_per_image, W, H, single_cls=False, native=None, skip=()):
    """every image's slot against process_batch / box_iou on labels gathered in row order; -> stats (correct, conf, cls, target classes)"""
    import lead_yolo_amd as L
    stats = []
    for b, det in enumerate(dets_per_image):
        if b in skip:
            continue
        s = slot0 + b
        idx = np.nonzero(rows[:, 0] == b)[0]
        lab = pixel_labels(rows[idx], W, H)
        det = det.copy()
        if single_cls:
            det[:, 5] = 0
        dn = det.copy()
        if native is not None:
            lab[:, 1:], dn[:, :4] = native(b, lab[:, 1:]), native(b, det[:, :4])
        n = len(det)
        l, best, tied = best_labels(dn, lab)
        assert not tied.any(), "premise: no detection has two same-class labels of equal best IoU"
        want = OMET.process_batch(dn, lab, LEVELS) if len(lab) else np.zeros((n, 10), bool)
        assert np.array_equal(want, closed_form(dn, lab)[0])
        assert h.n_det[s] == n and h.overflow[s] == 0
        assert np.array_equal(L.unpack_correct(h.correct[s, :n]), want), b
        assert np.array_equal(h.match_label[s, :n], np.where(l >= 0, idx[np.maximum(l, 0)] if len(idx) else -1, -1)), b
        assert np.array_equal(h.match_iou[s, :n].view(np.uint32), best.view(np.uint32)), b          # bit-equal to the float32 numpy box_iou
        assert np.array_equal(h.conf[s, :n], det[:, 4]) and np.array_equal(h.cls[s, :n], det[:, 5])
        for a in (h.correct, h.conf, h.cls, h.match_label, h.match_iou):
            assert not a[s, n:].any()                                                             # zero past the count
        stats.append((want, det[:, 4], det[:, 5], rows[idx, 1]))
    return stats


# ---------------------------------------------------------------------------------------------- 4. match_padded per image
@pytest.mark.parametrize("nc, single_cls", [(1, False), (3, False), (80, False), (3, True)])
def test_match_padded_equals_process_batch(nc, single_cls):
    import lead_yolo_amd as L
    images = _batch(nc, 40 + nc)
    if single_cls:                                                  # val.py:152: every prediction is class 0, and so is every label
        images = [(np.concatenate([lab[:, :1], np.zeros_like(lab[:, 1:2]), lab[:, 2:]], 1), det) for lab, det in images]
    dets, counts, targets, rows = _to_device(images, 7)
    idx4 = np.nonzero(rows[:, 0] == 4)[0]
    assert len(idx4) == 300 and idx4.max() - idx4.min() >= len(idx4)                # rows of different images interleaved
    acc = L.match_padded(dets, counts, targets, S, single_cls=single_cls, nc=1 if single_cls else nc)
    h = acc.host()
    assert h.cursor == 0
    _check_rows(h, 0, rows, [d for _, d in images], S, S, single_cls=single_cls)
    for b in range(8):
        assert np.array_equal(h.nt_class[b], np.bincount(rows[rows[:, 0] == b, 1].astype(int), minlength=acc.nc))
    if nc == 3 and not single_cls:
        got = L.unpack_correct(h.correct[5, :5])
        assert got[0].all() and not got[1].any() and not got[2].any() and not got[3].any() and got[4].all()
        row_a, row_c = (int(np.nonzero((rows[:, 0] == 5) & (rows[:, 2] == np.float32(x / S)))[0][0]) for x in (20, 50))      # labels A and C by centre
        assert h.match_label[5, :5].tolist() == [row_a, row_a, row_a, -1, row_c] and h.match_iou[5, 2] > 0.7 and h.match_iou[5, 3] == 0


# ---------------------------------------------------------------------------------------------- 5. native-space scoring
def test_match_padded_native_space():
    import lead_yolo_amd as L
    nc = 3
    images = _batch(nc, 77)
    rng = np.random.default_rng(3)
    # letterbox geometry (h0, w0, gain, padw, padh) of images that were scaled by `gain` and centred on the S x S canvas
    shapes = np.zeros((8, 5), np.float32)
    for b in range(8):
        gain = np.float32(rng.uniform(0.3, 0.9))
        w0, h0 = (round(S / gain), int(rng.integers(20, round(S / gain)))) if b % 2 else (int(rng.integers(20, round(S / gain))), round(S / gain))
        shapes[b] = (h0, w0, gain, (S - w0 * gain) / 2, (S - h0 * gain) / 2)
    dets, counts, targets, rows = _to_device(images, 9)

    def native(b, boxes):
        """scale_boxes with ratio_pad + clip_boxes (utils/general.py:800-829) in float32"""
        h0, w0, gain, padw, padh = shapes[b]
        out = np.asarray(boxes, np.float32).copy()
        out[:, [0, 2]] = np.clip((out[:, [0, 2]] - padw) / gain, np.float32(0), w0)
        out[:, [1, 3]] = np.clip((out[:, [1, 3]] - padh) / gain, np.float32(0), h0)
        return out

    clipped = sum(int((native(b, pixel_labels(lab, S, S)[:, 1:]) == 0).any() + (native(b, det[:, :4]) == 0).any()) for b, (lab, det) in enumerate(images)
                  if len(lab) and len(det))
    assert clipped >= 3                                             # boxes cut at the native border are part of the case
    acc = L.match_padded(dets, counts, targets, S, shapes=torch.from_numpy(shapes).to(_dev()), nc=nc)
    h = acc.host()
    stats = _check_rows(h, 0, rows, [d for _, d in images], S, S, native=native)
    assert sum(int(s[0].sum()) for s in stats) > 100


# ---------------------------------------------------------------------------------------------- 6. capacity guards
def test_label_overflow_and_capacity_are_reported_not_faults():
    import lead_yolo_amd as L
    images = _batch(1, 12, bs=4)
    rng = np.random.default_rng(1)
    images[1] = crowded_case(rng, 1, L.metrics.MAX_LABELS + 1, 60, size=float(S))
    dets, counts, targets, rows = _to_device(images, 5)
    v = L.Validator(1, capacity_images=6, size=S)
    v.update((dets, counts), targets)                               # returns: the guard is on the device, the report in compute()
    h = v.acc.host()
    assert h.cursor == 4 and h.overflow[:4].tolist() == [0, 1, 0, 0] and h.nt_class[1, 0] == L.metrics.MAX_LABELS + 1
    assert h.n_det[1] == 60 and not h.correct[1].any() and (h.match_label[1, :60] == -1).all() and np.array_equal(h.conf[1, :60], images[1][1][:, 4])
    _check_rows(h, 0, rows, [d for _, d in images], S, S, skip=(1,))           # the other images' rows are still right
    with pytest.raises(RuntimeError, match="overflow"):
        v.compute()
    with pytest.raises(RuntimeError, match="capacity_images"):
        v.update((dets, counts), targets)                           # 4 + 4 > 6: raised on the host, nothing launched
    assert v.acc.host().cursor == 4
    bad = targets.clone()
    bad[bad[:, 0] == 0, 1] = 3.0                                     # a label class outside [0, nc)
    v.reset().update((dets[:1], counts[:1]), bad)
    with pytest.raises(RuntimeError, match="class outside"):
        v.compute()
    with pytest.raises(L.capi.HipLibraryError, match="row width"):
        L.match_padded(dets, counts, targets, S, out=L.MatchAccumulator(4, MAX_DET - 1, 1, _dev()))
    with pytest.raises(ValueError):
        L.MatchAccumulator(4, MAX_DET, 0, _dev())


# ---------------------------------------------------------------------------------------------- 7. accumulation and replay
def test_three_updates_equal_one_oracle_pass():
    import lead_yolo_amd as L
    nc = 3
    images = _batch(nc, 21, bs=8) + _batch(nc, 22, bs=8) + _batch(nc, 23, bs=5)
    v = L.Validator(nc, capacity_images=21, size=S)
    want = []
    for k, (lo, hi) in enumerate(((0, 8), (8, 16), (16, 21))):
        dets, counts, targets, rows = _to_device(images[lo:hi], 30 + k)
        v.update((dets, counts), targets)
        want += _check_rows(v.acc.host(), lo, rows, [d for _, d in images[lo:hi]], S, S)
    correct, conf, cls, nt = v.stats()
    cat = [np.concatenate(x) for x in zip(*want)]
    assert np.array_equal(correct, cat[0]) and np.array_equal(conf, cat[1]) and np.array_equal(cls, cat[2])
    assert np.array_equal(nt, np.bincount(cat[3].astype(int), minlength=nc))
    res, ref = v.compute(), OMET.mean_results(want)
    np.testing.assert_allclose(res[:4], ref, rtol=0, atol=1e-12)
    assert res.map50 > 0.1 and len(res.p) == len(res.classes) == nc and np.array_equal(res.nt, nt)


def test_captured_update_replays_batch_after_batch():
    import lead_yolo_amd as L
    nc = 3
    batches = [_batch(nc, 50 + k) for k in range(3)]
    pad = max(sum(len(lab) for lab, _ in b) for b in batches)
    dev_batches = []
    for k, b in enumerate(batches):
        n = sum(len(lab) for lab, _ in b)
        dev_batches.append(_to_device(b, 60 + k, pad_rows=pad - n)[:3])           # fixed-shape targets: padding rows carry image -1
    eager, graphed = L.Validator(nc, capacity_images=24, size=S), L.Validator(nc, capacity_images=24, size=S)
    for dets, counts, targets in dev_batches:
        eager.update((dets, counts), targets)
    sd, sc, st = (t.clone() for t in dev_batches[0])
    graphed.update((sd, sc), st)                                    # warm-up off the capture
    graphed.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                       # one stream, no parallel branches: match, then advance
        graphed.update((sd, sc), st)
    graphed.reset()
    for dets, counts, targets in dev_batches:
        sd.copy_(dets), sc.copy_(counts), st.copy_(targets)
        g.replay()
    torch.cuda.synchronize()
    assert int(graphed.acc.cursor[0]) == 24
    assert torch.equal(graphed.acc.buf, eager.acc.buf)              # the accumulator bytes
    np.testing.assert_array_equal(graphed.compute()[:4], eager.compute()[:4])


# ---------------------------------------------------------------------------------------------- 8. the SSDD fixture end to end
def test_validator_end_to_end_on_ssdd16():
    import lead_yolo_amd as L
    d = np.load(FIX)
    imgs = torch.from_numpy(d["imgs"]).unsqueeze(1).expand(-1, 3, -1, -1).contiguous()
    tg = torch.from_numpy(d["targets"])
    torch.manual_seed(0)
    m = L.Model(_cfg("n"))
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 6262)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    st["model.23.m.0.bias"] = st["model.23.m.0.bias"] + 2.0        # as test_val_pipeline_boxes_match_oracle: lift a few boxes over the threshold
    m.load_state_dict(st)
    with torch.no_grad():
        z, _ = m.to(_dev()).eval()((imgs.float() / 255).to(_dev()))
    dets, counts, _ = L.nms_padded(z, 0.001, 0.6)                   # val.py:230-234; the SAME boxes go down both routes
    v = L.Validator(1, capacity_images=16, size=320)
    v.update((dets, counts), tg.to(_dev()))
    correct, conf, cls, nt = v.stats()
    res = v.compute()
    dn, cn, rows = dets.cpu().numpy(), counts.cpu().numpy(), tg.numpy()
    assert cn.sum() >= 200
    stats = []
    for i in range(16):
        lab = pixel_labels(rows[rows[:, 0] == i], 320, 320)         # scale, then xywh2xyxy, in float32
        pred = dn[i, :cn[i]]
        if len(pred) == 0 and len(lab) == 0:
            continue
        c = OMET.process_batch(pred, lab, LEVELS) if len(lab) and len(pred) else np.zeros((len(pred), 10), bool)
        stats.append((c, pred[:, 4], pred[:, 5], lab[:, 0]))
    assert np.array_equal(correct, np.concatenate([s[0] for s in stats])) and np.array_equal(conf, np.concatenate([s[1] for s in stats]))
    assert int(nt[0]) == len(rows)
    np.testing.assert_allclose(res[:4], OMET.mean_results(stats), rtol=0, atol=1e-12)
    print(f"ssdd16, random weights: {int(cn.sum())} detections, {int(correct[:, 0].sum())} correct at 0.5, (P, R, mAP50, mAP) = {res[:4]}")
