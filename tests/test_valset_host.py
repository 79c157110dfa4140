"""Host side of the device validation run (lead-yolo_amd/valrun.py, metrics.ConfusionMatrix), no GPU: val_plan and val_labels against the
validation dataloader's formulas restated here (utils/dataloaders.py LoadImagesAndLabels.__init__ / load_image / __getitem__ / collate_fn,
utils/augmentations.py letterbox, utils/general.py xywhn2xyxy / xyxy2xywhn / clip_boxes), ConfusionMatrix.process_batch (utils/metrics.py)
restated in numpy against the closed form csrc/ly_metrics.hip `ly_val_confusion` computes, and the C ABI of the new entry.
tests/test_gpu_confusion.py and tests/test_gpu_valrun.py import the restatements from here."""
import ctypes
import re

import numpy as np
import pytest

from lead_yolo_amd import capi
from lead_yolo_amd import valrun as V
from oracle import metrics as OMET
from tests.test_metrics_host import crowded_case, pixel_labels

TEN = [(40, 120), (50, 110), (60, 100), (70, 90), (90, 100), (100, 90), (90, 60), (110, 60), (120, 50), (128, 40)]


# ---- the reference's dataloader arithmetic, its statements in its order -------------------------------------------------------------------
def ref_rect(shapes_hw, img_size, batch_size, stride, pad):
    """LoadImagesAndLabels.__init__, `if self.rect:` -> (irect, batch_shapes [nb, 2] = (H, W)); the sort is made stable (the reference's order
    among equal aspect ratios is unspecified)"""
    s = np.array([(w, h) for h, w in shapes_hw])                       # self.shapes: wh
    n = len(s)
    bi = np.floor(np.arange(n) / batch_size).astype(int)
    nb = bi[-1] + 1
    ar = s[:, 1] / s[:, 0]
    irect = ar.argsort(kind="stable")
    ar = ar[irect]
    shapes = [[1, 1]] * nb
    for i in range(nb):
        ari = ar[bi == i]
        mini, maxi = ari.min(), ari.max()
        if maxi < 1:
            shapes[i] = [maxi, 1]
        elif mini > 1:
            shapes[i] = [1, 1 / mini]
    return irect, np.ceil(np.array(shapes) * img_size / stride + pad).astype(int) * stride


def ref_letterbox_hw(shape, new_shape, scaleup=False):
    """utils/augmentations.py letterbox(im, new_shape=(H, W), auto=False, scaleFill=False, scaleup) on an image of `shape` = (h, w)"""
    r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
    if not scaleup:
        r = min(r, 1.0)
    ratio = r, r
    new_unpad = int(round(shape[1] * r)), int(round(shape[0] * r))
    dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]
    dw /= 2
    dh /= 2
    top, left = int(round(dh - 0.1)), int(round(dw - 0.1))
    return dict(ratio=ratio, nw=new_unpad[0], nh=new_unpad[1], pad=(dw, dh), top=top, left=left)


def ref_item(h0, w0, img_size, shape):
    """__getitem__ of a non-augmenting loader: load_image, then letterbox(img, shape, auto=False, scaleup=False) -> the letterbox numbers,
    (h, w) of load_image and val.py's `shapes` entry flattened to (h0, w0, h / h0, dw, dh)"""
    r = img_size / max(h0, w0)
    h, w = int(h0 * r), int(w0 * r)                                     # cv2.resize(im, (int(w0 * r), int(h0 * r)))
    lb = ref_letterbox_hw((h, w), shape)
    return lb, (h, w), (h0, w0, h / h0, lb["pad"][0], lb["pad"][1])


def xywhn2xyxy(x, w=640, h=640, padw=0, padh=0):
    y = np.copy(x)
    y[..., 0] = w * (x[..., 0] - x[..., 2] / 2) + padw
    y[..., 1] = h * (x[..., 1] - x[..., 3] / 2) + padh
    y[..., 2] = w * (x[..., 0] + x[..., 2] / 2) + padw
    y[..., 3] = h * (x[..., 1] + x[..., 3] / 2) + padh
    return y


def xyxy2xywhn(x, w=640, h=640, clip=False, eps=0.0):
    if clip:
        x[..., [0, 2]] = x[..., [0, 2]].clip(0, w - eps)               # clip_boxes(x, (h - eps, w - eps))
        x[..., [1, 3]] = x[..., [1, 3]].clip(0, h - eps)
    y = np.copy(x)
    y[..., 0] = ((x[..., 0] + x[..., 2]) / 2) / w
    y[..., 1] = ((x[..., 1] + x[..., 3]) / 2) / h
    y[..., 2] = (x[..., 2] - x[..., 0]) / w
    y[..., 3] = (x[..., 3] - x[..., 1]) / h
    return y


def ref_label_rows(lab, lb, hw, canvas, image):
    """__getitem__'s label lines and collate_fn's image column for one image: lab float32 [m, 5] -> ([m, 6] float32, was the clip active?)"""
    labels = np.array(lab, dtype=np.float32).reshape(-1, 5).copy()
    clipped = False
    if labels.size:
        labels[:, 1:] = xywhn2xyxy(labels[:, 1:], lb["ratio"][0] * hw[1], lb["ratio"][1] * hw[0], padw=lb["pad"][0], padh=lb["pad"][1])
    if len(labels):
        before = labels[:, 1:5].copy()
        labels[:, 1:5] = xyxy2xywhn(labels[:, 1:5], w=canvas[1], h=canvas[0], clip=True, eps=1e-3)
        clipped = bool((before[:, [0, 2]] > canvas[1] - 1e-3).any() or (before[:, [1, 3]] > canvas[0] - 1e-3).any() or (before < 0).any())
    assert labels.dtype == np.float32
    return np.concatenate([np.full((len(labels), 1), image, np.float32), labels], 1), clipped


# ---- ConfusionMatrix.process_batch (utils/metrics.py), restated, and the closed form the kernel computes -----------------------------------
def ref_confusion(M, det, lab, nc, conf=0.25, thr=0.45):
    """adds one image to M [nc + 1, nc + 1].  det [n, 6] (xyxy, conf, cls) or None, lab [m, 5] (cls, xyxy), m >= 1 (val.py calls it only for
    images that have labels)"""
    gt = lab[:, 0].astype(int)
    if det is None:
        for g in gt:
            M[nc, g] += 1
        return
    det = det[det[:, 4] > conf]
    dc = det[:, 5].astype(int)
    iou = OMET.box_iou(lab[:, 1:], det[:, :4])
    x = np.nonzero(iou > thr)
    if x[0].shape[0]:
        m = np.concatenate((np.stack(x, 1), iou[x[0], x[1]][:, None]), 1)
        if x[0].shape[0] > 1:
            m = m[m[:, 2].argsort()[::-1]]
            m = m[np.unique(m[:, 1], return_index=True)[1]]
            m = m[m[:, 2].argsort()[::-1]]
            m = m[np.unique(m[:, 0], return_index=True)[1]]
    else:
        m = np.zeros((0, 3))
    n = m.shape[0] > 0
    m0, m1, _ = m.transpose().astype(int)
    for i, g in enumerate(gt):
        j = m0 == i
        if n and sum(j) == 1:
            M[dc[m1[j]], g] += 1
        else:
            M[nc, g] += 1
    if n:
        for i, d in enumerate(dc):
            if not any(m1 == i):
                M[d, nc] += 1


def no_ties(det, lab, conf=0.25, thr=0.45):
    """the premise under which the reference's unstable sorts have one answer: among the pairs with IoU > thr no kept detection has two labels
    of equal IoU and no label two kept detections of equal IoU"""
    det = det[det[:, 4] > conf]
    if len(det) == 0 or len(lab) == 0:
        return True
    iou = OMET.box_iou(lab[:, 1:], det[:, :4])
    for a in (iou, iou.T):
        for row in a:
            v = row[row > thr]
            if len(np.unique(v)) != len(v):
                return False
    return True


def closed_confusion(M, det, lab, nc, conf=0.25, thr=0.45):
    """the closed form: l*(d) = the label of any class with the largest IoU > thr (lowest row on equal IoU), d*(l) = the detection with the
    largest IoU among those with l* = l (lowest index on equal IoU)"""
    gt = lab[:, 0].astype(int)
    det = np.zeros((0, 6), np.float32) if det is None else det[det[:, 4] > conf]
    dc = det[:, 5].astype(int)
    iou = OMET.box_iou(lab[:, 1:], det[:, :4]) if len(det) else np.zeros((len(lab), 0), np.float32)
    lstar = np.full(len(det), -1)
    for d in range(len(det)):
        col = np.where(iou[:, d] > thr, iou[:, d], np.float32(-1))
        if col.max() > 0:
            lstar[d] = int(col.argmax())
    dstar = np.full(len(lab), -1)
    for l in range(len(lab)):
        ds = np.nonzero(lstar == l)[0]
        if len(ds):
            dstar[l] = int(ds[iou[l, ds].argmax()])
    for l, g in enumerate(gt):
        M[dc[dstar[l]] if dstar[l] >= 0 else nc, g] += 1
    if (dstar >= 0).any():
        for d in range(len(det)):
            if lstar[d] < 0 or dstar[lstar[d]] != d:
                M[dc[d], nc] += 1


# ---------------------------------------------------------------------------------------------- 1. val_plan
def _check_plan(sizes, img_size, batch_size, rect, stride=32, pad=0.5):
    p = V.val_plan(sizes, img_size, batch_size, stride, pad, rect)
    n = len(sizes)
    if rect:
        order, bshapes = ref_rect(sizes, img_size, batch_size, stride, pad)
    else:
        order, bshapes = np.arange(n), np.full(((n - 1) // batch_size + 1, 2), img_size)
    assert np.array_equal(p.order, order) and np.array_equal(p.batch_shapes, bshapes)
    assert p.n == n and p.nb == len(bshapes) and [(lo, hi) for lo, hi, _ in p.batches()] == [(i, min(i + batch_size, n)) for i in
                                                                                           range(0, n, batch_size)]
    want = {k: [] for k in ("h0", "w0", "nh", "nw", "top", "left", "H", "W", "h", "w")}
    vshapes = []
    for pos, i in enumerate(order):
        h0, w0 = sizes[i]
        H, W = bshapes[pos // batch_size]
        lb, (h, w), row = ref_item(h0, w0, img_size, (H, W))
        for k, v in zip(want, (h0, w0, lb["nh"], lb["nw"], lb["top"], lb["left"], H, W, h, w)):
            want[k].append(v)
        vshapes.append(row)
        assert (p.lb.r[pos], p.lb.dw[pos], p.lb.dh[pos]) == (lb["ratio"][0], lb["pad"][0], lb["pad"][1])
        assert lb["top"] + lb["nh"] <= H and lb["left"] + lb["nw"] <= W                       # the picture fits its canvas
    for k in want:
        assert np.array_equal(getattr(p, k) if k in ("h", "w") else getattr(p.lb, k), np.array(want[k])), k
    assert p.lb.val_shapes.dtype == np.float32 and np.array_equal(p.lb.val_shapes, np.array(vshapes, np.float32).reshape(-1, 5))
    return p


def test_val_plan_is_the_dataloader_arithmetic():
    rng = np.random.default_rng(11)
    canvases = set()
    for case in range(50):
        n = int(rng.integers(1, 41))
        sizes = [(int(h), int(w)) for h, w in rng.integers(20, 401, (n, 2))]
        if case % 5 == 0:                                               # equal aspect ratios: the stable order decides
            sizes += sizes[:3]
        img_size, batch_size = (64, 128, 640)[case % 3], (1, 4, 32)[(case // 3) % 3]
        for rect in (True, False):
            p = _check_plan(sizes, img_size, batch_size, rect)
            canvases |= {tuple(s) for s in p.batch_shapes.tolist()} if rect else set()
            if not rect:
                assert (p.batch_shapes == img_size).all() and np.array_equal(p.order, np.arange(len(sizes)))
    assert len(canvases) > 10 and any(h < w for h, w in canvases) and any(h > w for h, w in canvases)


def test_val_plan_ten_size_example():
    p = _check_plan(TEN, 128, 4, True)
    assert p.batch_shapes.tolist() == [[128, 160], [160, 160], [160, 96]]
    assert p.order.tolist() == list(range(10))                          # TEN is sorted by h / w already
    assert (p.h[0], p.w[0], p.lb.nh[0], p.lb.top[0], p.lb.left[0]) == (42, 128, 42, 43, 16)           # int(40 * 128 / 120) = 42: truncated
    assert [hi - lo for lo, hi, _ in p.batches()] == [4, 4, 2]
    with pytest.raises(ValueError):
        V.val_plan([], 128, 4)
    with pytest.raises(ValueError):
        V.val_plan([(1, 400)], 128, 4)                                  # load_image would give 0 rows


def test_load_image_size_is_stated_once():
    from lead_yolo_amd import predict
    assert predict.load_image_size(1080, 1920, 640) == (360, 640) and predict.load_image_size(40, 120, 128) == (42, 128)
    assert V.load_image_size is predict.load_image_size


# ---------------------------------------------------------------------------------------------- 2. label rows
def _labels_for(rng, n):
    """per image: a box covering the whole image and one in the far corner (both touch the border, where the clip acts when the picture fills
    its canvas, as on the square canvases of rect=False), two boxes reaching far past the left and right borders (past the canvas's edge even
    behind rect's padding), random boxes; image 2 has no labels"""
    out = []
    for i in range(n):
        m = int(rng.integers(0, 6))
        xy, wh = rng.uniform(0.1, 0.9, (m, 2)), rng.uniform(0.02, 0.2, (m, 2))
        rows = np.concatenate([rng.integers(0, 3, (m, 1)).astype(np.float64), xy, wh], 1)
        fixed = np.array([[0, 0.5, 0.5, 1.0, 1.0], [1, 0.9, 0.9, 0.2, 0.2], [2, -0.2, 0.5, 0.3, 0.3], [0, 1.25, 0.5, 0.4, 0.2]])
        out.append(np.zeros((0, 5), np.float32) if i == 2 else np.concatenate([fixed, rows]).astype(np.float32))
    return out


@pytest.mark.parametrize("rect", [True, False])
def test_val_labels_are_the_dataloader_rows(rect):
    rng = np.random.default_rng(5)
    sizes = TEN + [(128, 128), (64, 64), (256, 100)]
    labels = _labels_for(rng, len(sizes))
    plan = V.val_plan(sizes, 128, 4, rect=rect)
    got = V.val_labels(labels, plan)
    assert len(got) == plan.nb
    any_clip = 0
    for b, (lo, hi, canvas) in enumerate(plan.batches()):
        rows = []
        for pos in range(lo, hi):
            i = plan.order[pos]
            lb, hw, _ = ref_item(*sizes[i], 128, canvas)
            r, c = ref_label_rows(labels[i], lb, hw, canvas, pos - lo)
            rows.append(r)
            any_clip += c
        want = np.concatenate(rows)
        assert got[b].dtype == np.float32 and got[b].shape == want.shape
        assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), (b, got[b], want)           # float32, bit for bit
        assert (got[b][:, 2:] >= 0).all() and (got[b][:, 2:] <= 1).all()
    assert any_clip >= 3                                                # the clip was active
    pos2 = int(np.nonzero(plan.order == 2)[0][0])
    assert not (got[pos2 // 4][:, 0] == pos2 % 4).any()                 # the image without labels has no rows
    with pytest.raises(ValueError):
        V.val_labels(labels[:-1], plan)


# ---------------------------------------------------------------------------------------------- 3. the closed form of the confusion matrix
@pytest.mark.parametrize("nc", [1, 3, 80])
def test_closed_form_confusion_equals_process_batch(nc):
    rng = np.random.default_rng(300 + nc)                            # (seed 280: one label with 272 detections, two of equal IoU)
    shapes = [(1, 0), (1, 1), (5, 0), (1, 7), (5, 40), (12, 120), (40, 300), (25, 200)] + [(int(rng.integers(1, 41)), int(rng.integers(0, 301)))
                                                                                          for _ in range(42)]
    total_ref, total = np.zeros((nc + 1, nc + 1), np.int64), np.zeros((nc + 1, nc + 1), np.int64)
    for n_lab, n_det in shapes:
        rows, dets = crowded_case(rng, nc, n_lab, n_det)
        lab = pixel_labels(rows, 64, 64)
        assert no_ties(dets, lab), "the generator must give no equal IoUs inside a row or a column of the pairs above the threshold"
        want, got = np.zeros_like(total), np.zeros_like(total)
        ref_confusion(want, dets if n_det else None, lab, nc)
        closed_confusion(got, dets if n_det else None, lab, nc)
        assert np.array_equal(got, want), (nc, n_lab, n_det)
        assert want[:, :nc].sum() == n_lab                             # every label is counted once
        total_ref += want
        total += got
    assert np.array_equal(total, total_ref)
    assert np.trace(total[:nc, :nc]) > 300 and total[:nc, nc].sum() > 1000 and total[nc, :nc].sum() > 50          # TP, FP, FN: not vacuous
    if nc > 1:
        assert total[:nc, :nc].sum() - np.trace(total[:nc, :nc]) > 20                                            # off-diagonal confusions


def test_confusion_if_n_quirk_in_the_restatement():
    """kept detections without any pair above the threshold are NOT counted as false positives (the reference's `if n:`)"""
    lab = np.array([[0, 10, 10, 20, 20]], np.float32)
    det = np.array([[40, 40, 50, 50, 0.9, 1], [30, 30, 40, 40, 0.8, 0]], np.float32)
    for fn in (ref_confusion, closed_confusion):
        M = np.zeros((3, 3), np.int64)
        fn(M, det, lab, 2)
        assert M.tolist() == [[0, 0, 0], [0, 0, 0], [1, 0, 0]], fn.__name__


# ---------------------------------------------------------------------------------------------- 4. the C ABI
def test_header_declares_the_confusion_entry():
    text = open(capi.HEADER_PATH).read()
    assert re.search(r"^int ly_val_confusion\(", text, re.M)
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    sig = capi.SIGNATURES["ly_val_confusion"]
    assert len(sig) == 16 and capi.RESTYPES["ly_val_confusion"] is I
    assert sig == [P, P, I, I, P, ctypes.c_long, I, I, P, F, F, I, I, P, P, P]
    assert capi.SIGNATURES["ly_val_match"][:9] == sig[:9]               # the same inputs as ly_val_match


def test_new_names_are_exported():
    import lead_yolo_amd as L
    for name in ("ConfusionMatrix", "ValSet", "ValPlan", "ValRun", "val_plan", "val_labels", "validate", "load_image_size"):
        assert hasattr(L, name), name
