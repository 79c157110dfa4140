"""csrc/ly_metrics.hip `ly_val_confusion` and metrics.ConfusionMatrix / Validator(confusion=True) on the device against
ConfusionMatrix.process_batch restated in numpy (tests/test_valset_host.py ref_confusion): whole batches by array_equal, a crafted image for
every rule, native-space scoring, accumulation, replay from a captured graph, and the label guard.  The reference's order under equal IoUs is
unspecified, so every case asserts on the host that it has none (no_ties)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_metrics import MAX_DET, S, _batch, _to_device
from tests.test_gpu_modules import _dev
from tests.test_metrics_host import crowded_case, pixel_labels
from tests.test_valset_host import closed_confusion, no_ties, ref_confusion

pytestmark = pytest.mark.gpu


def _expected(rows, dets_per_image, nc, single_cls=False, native=None, skip=()):
    """the sum of the restated per-image calls, as val.py makes them: only for images that have labels, detections=None without detections"""
    M = np.zeros((nc + 1, nc + 1), np.int64)
    for b, det in enumerate(dets_per_image):
        idx = np.nonzero(rows[:, 0] == b)[0]
        if len(idx) == 0 or b in skip:
            continue
        lab = pixel_labels(rows[idx], S, S)
        det = det.copy()
        if single_cls:
            det[:, 5] = 0
        if native is not None:
            lab[:, 1:], det[:, :4] = native(b, lab[:, 1:]), native(b, det[:, :4])
        assert no_ties(det, lab), f"premise: image {b} has no equal IoUs among the pairs above the threshold"
        one, closed = np.zeros_like(M), np.zeros_like(M)
        ref_confusion(one, det if len(det) else None, lab, nc)
        closed_confusion(closed, det if len(det) else None, lab, nc)
        assert np.array_equal(one, closed), b
        M += one
    return M


# ---------------------------------------------------------------------------------------------- 5. whole batches
@pytest.mark.parametrize("nc, single_cls", [(1, False), (3, False), (80, False), (3, True)])
def test_confusion_equals_process_batch(nc, single_cls):
    import lead_yolo_amd as L
    images = _batch(nc, 40 + nc)          # 0: no detections, 1: no labels but 30 detections, 2: neither, 3: max_det detections, 4: 300 labels, ...
    if single_cls:
        images = [(np.concatenate([lab[:, :1], np.zeros_like(lab[:, 1:2]), lab[:, 2:]], 1), det) for lab, det in images]
    dets, counts, targets, rows = _to_device(images, 7, pad_rows=9)
    idx4 = np.nonzero(rows[:, 0] == 4)[0]
    assert len(idx4) == 300 and idx4.max() - idx4.min() >= len(idx4) and (rows[:, 0] == -1).sum() == 9        # interleaved rows, padding rows
    assert counts[3] == MAX_DET and counts[0] == 0 and counts[1] == 30 and not (rows[:, 0] == 1).any()
    k = 1 if single_cls else nc
    cm = L.ConfusionMatrix(k)
    cm.update((dets, counts), targets, S, single_cls=single_cls)
    got = cm.matrix()
    want = _expected(rows, [d for _, d in images], k, single_cls=single_cls)
    assert got.dtype == np.int64 and got.shape == (k + 1, k + 1)
    assert np.array_equal(got, want), (got, want)
    assert want[:k, :k].sum() + want[k, :k].sum() == (rows[:, 0] >= 0).sum()            # every label once: matched or missed
    assert np.trace(want[:k, :k]) > 50 and want[:k, k].sum() > 100 and want[k, :k].sum() > 100 and want[k, k] == 0
    only1 = L.ConfusionMatrix(k)                                                          # image 1 alone: 30 detections, no labels -> nothing
    only1.update((dets[1:2].contiguous(), counts[1:2].contiguous()), targets[:0], S, single_cls=single_cls)
    assert not only1.matrix().any()
    tp, fp = cm.tp_fp()
    assert np.array_equal(tp, want.diagonal()[:-1]) and np.array_equal(fp, (want.sum(1) - want.diagonal())[:-1])


# ---------------------------------------------------------------------------------------------- 6. every rule on a crafted image
def _rows_of(image, cls_boxes):
    return np.array([[image, c, (b[0] + b[2]) / 2 / S, (b[1] + b[3]) / 2 / S, (b[2] - b[0]) / S, (b[3] - b[1]) / S] for c, b in cls_boxes], np.float32)


def test_confusion_rules_on_crafted_images():
    import lead_yolo_amd as L
    nc = 3
    # image 0 — labels A, B (class 0, overlapping), C (class 0), D (class 2)
    lab0 = _rows_of(0, [(0, (10, 10, 30, 30)), (0, (18, 10, 38, 30)), (0, (40, 40, 60, 60)), (2, (4, 40, 14, 60))])
    det0 = np.array([[10, 10, 30, 30.5, 0.9, 0],        # d0 on A (IoU 0.976): A's detection
                     [13, 10, 34, 30, 0.8, 0],           # d1: best label A (0.708, taken by d0); it also overlaps the free label B (0.64 > 0.45)
                     [40, 40, 60, 60.5, 0.7, 1],         # d2: a class-1 detection on the class-0 label C
                     [4, 40, 14, 60, 0.25, 2]], np.float32)      # d3: exactly on D, conf == 0.25 exactly
    # image 1 — one label, two kept detections that overlap nothing
    lab1 = _rows_of(1, [(1, (10, 10, 20, 20))])
    det1 = np.array([[40, 40, 50, 50, 0.9, 0], [30, 30, 40, 40, 0.8, 2]], np.float32)
    dets, counts, targets, rows = _to_device([(lab0, det0), (lab1, det1)], 3, pad_rows=2)
    cm = L.ConfusionMatrix(nc)
    cm.update((dets[1:].contiguous(), counts[1:].contiguous()), torch.from_numpy(lab1 * np.array([0, 1, 1, 1, 1, 1], np.float32)).to(_dev()), S)
    m1 = cm.matrix()
    want1 = np.zeros((4, 4), np.int64)
    want1[nc, 1] = 1
    assert np.array_equal(m1, want1), "kept detections without any overlap are not false positives: only M[nc, gt] (the reference's `if n:`)"
    cm.reset().update((dets[:1].contiguous(), counts[:1].contiguous()), targets, S)
    m0 = cm.matrix()
    assert m0[0, 0] == 1, "d0 is A's detection"
    assert m0[0, nc] == 1 and m0[nc, 0] == 1, "d1's best label A is taken: it is a false positive, NOT moved to the free label B, which is missed"
    assert m0[1, 0] == 1, "a class-1 detection on a class-0 label lands in M[1, 0]"
    assert m0[nc, 2] == 1 and m0[2].sum() == 0, "conf == 0.25 exactly is dropped: D is missed and class 2 predicts nothing"
    assert m0.sum() == 5
    assert np.array_equal(m0 + m1, _expected(rows, [det0, det1], nc))
    cm.reset().update((dets, counts), targets, S)
    assert np.array_equal(cm.matrix(), m0 + m1)


# ---------------------------------------------------------------------------------------------- 7. native space
def test_confusion_native_space():
    import lead_yolo_amd as L
    nc = 3
    images = _batch(nc, 77)
    rng = np.random.default_rng(3)
    shapes = np.zeros((8, 5), np.float32)                              # (h0, w0, gain, padw, padh): scaled by `gain`, centred on the S x S canvas
    for b in range(8):
        gain = np.float32(rng.uniform(0.3, 0.9))
        w0, h0 = (round(S / gain), int(rng.integers(20, round(S / gain)))) if b % 2 else (int(rng.integers(20, round(S / gain))), round(S / gain))
        shapes[b] = (h0, w0, gain, (S - w0 * gain) / 2, (S - h0 * gain) / 2)
    assert (shapes[:, 2] != 1).all() and (shapes[:, 3:] > 0).any(0).all()
    dets, counts, targets, rows = _to_device(images, 9)

    def native(b, boxes):
        """scale_boxes with ratio_pad + clip_boxes (utils/general.py) in float32"""
        h0, w0, gain, padw, padh = shapes[b]
        out = np.asarray(boxes, np.float32).copy()
        out[:, [0, 2]] = np.clip((out[:, [0, 2]] - padw) / gain, np.float32(0), w0)
        out[:, [1, 3]] = np.clip((out[:, [1, 3]] - padh) / gain, np.float32(0), h0)
        return out

    clipped = sum(int((native(b, pixel_labels(lab, S, S)[:, 1:]) == 0).any() + (native(b, det[:, :4]) == 0).any()) for b, (lab, det) in enumerate(images)
                  if len(lab) and len(det))
    assert clipped >= 3                                                 # boxes cut at the native border are part of the case
    cm = L.ConfusionMatrix(nc)
    cm.update((dets, counts), targets, S, shapes=torch.from_numpy(shapes).to(_dev()))
    want = _expected(rows, [d for _, d in images], nc, native=native)
    assert np.array_equal(cm.matrix(), want)
    assert np.trace(want[:nc, :nc]) > 30 and want[:nc, nc].sum() > 100


# ---------------------------------------------------------------------------------------------- 8. accumulation and replay
def test_three_updates_equal_one_pass_and_reset():
    import lead_yolo_amd as L
    nc = 3
    images = _batch(nc, 21, bs=8) + _batch(nc, 22, bs=8) + _batch(nc, 23, bs=5)
    cm = L.ConfusionMatrix(nc)
    want = np.zeros((nc + 1, nc + 1), np.int64)
    for k, (lo, hi) in enumerate(((0, 8), (8, 16), (16, 21))):
        dets, counts, targets, rows = _to_device(images[lo:hi], 30 + k)
        cm.update((dets, counts), targets, S)
        want += _expected(rows, [d for _, d in images[lo:hi]], nc)
    assert np.array_equal(cm.matrix(), want) and want.sum() > 1000
    assert not cm.reset().matrix().any() and not cm.buf.any()


def test_captured_validator_with_confusion_replays():
    import lead_yolo_amd as L
    nc = 3
    batches = [_batch(nc, 50 + k) for k in range(3)]
    pad = max(sum(len(lab) for lab, _ in b) for b in batches)
    dev_batches, want = [], np.zeros((nc + 1, nc + 1), np.int64)
    for k, b in enumerate(batches):
        n = sum(len(lab) for lab, _ in b)
        d, c, t, rows = _to_device(b, 60 + k, pad_rows=pad - n)         # fixed-shape targets: padding rows carry image -1
        dev_batches.append((d, c, t))
        want += _expected(rows, [x for _, x in b], nc)
    eager = L.Validator(nc, capacity_images=24, size=S, confusion=True)
    graphed = L.Validator(nc, capacity_images=24, size=S, confusion=True)
    plain = L.Validator(nc, capacity_images=24, size=S)
    assert plain.confusion is None
    for dets, counts, targets in dev_batches:
        eager.update((dets, counts), targets)
        plain.update((dets, counts), targets)
    sd, sc, st = (t.clone() for t in dev_batches[0])
    graphed.update((sd, sc), st)                                        # warm-up off the capture
    graphed.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                           # one stream: match, advance, confusion
        graphed.update((sd, sc), st)
    graphed.reset()
    assert not graphed.confusion.buf.any()                              # reset() zeroes the matrix too
    for dets, counts, targets in dev_batches:
        sd.copy_(dets), sc.copy_(counts), st.copy_(targets)
        g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(eager.confusion.matrix(), want)
    assert np.array_equal(graphed.confusion.matrix(), want)
    assert torch.equal(graphed.acc.buf, eager.acc.buf) and torch.equal(plain.acc.buf, eager.acc.buf)       # the scoring is what it was


# ---------------------------------------------------------------------------------------------- 9. the guards
def test_too_many_labels_are_flagged_and_the_image_skipped():
    import lead_yolo_amd as L
    images = _batch(1, 12, bs=4)
    images[1] = crowded_case(np.random.default_rng(1), 1, L.metrics.MAX_LABELS + 1, 60, size=float(S))
    assert len(images[1][0]) == 513
    dets, counts, targets, rows = _to_device(images, 5)
    cm = L.ConfusionMatrix(1)
    cm.update((dets, counts), targets, S)                               # returns: the guard is on the device, the report in matrix()
    h = cm.buf.cpu().numpy()
    assert h[-1] == L.metrics.OVF_LABELS
    assert np.array_equal(h[:-1].reshape(2, 2), _expected(rows, [d for _, d in images], 1, skip=(1,)))         # the other images are counted
    with pytest.raises(RuntimeError, match="overflow of the 512 labels"):
        cm.matrix()
    bad = targets.clone()
    bad[bad[:, 0] == 0, 1] = 3.0                                        # a label class outside [0, nc)
    cm.reset().update((dets[:1].contiguous(), counts[:1].contiguous()), bad, S)
    with pytest.raises(RuntimeError, match="class outside"):
        cm.matrix()
    assert not cm.buf[:-1].any()                                        # image 0 has no other labels: nothing is counted
    with pytest.raises(ValueError):
        L.ConfusionMatrix(0)
