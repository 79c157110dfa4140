"""Eval tail: non_max_suppression.  CPU: the oracle restatement (oracle/nms.py) against hand-computed cases and the defining properties of
greedy NMS.  GPU: the HIP path (lead-yolo_amd/nms.py -> csrc/ly_nms.hip) against the oracle, kept indices bit-exact."""
import numpy as np
import pytest
import torch

from oracle import nms as ON


def _iou(a, b):
    iw = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
    inter = iw * ih
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def _random_pred(bs, n, nc, seed, cluster=True):
    g = np.random.default_rng(seed)
    p = np.zeros((bs, n, 5 + nc), np.float32)
    centres = g.uniform(50, 590, (bs, 12, 2))
    which = g.integers(0, 12, (bs, n))
    xy = np.take_along_axis(centres, which[..., None].repeat(2, -1), 1) + g.normal(0, 6 if cluster else 200, (bs, n, 2))
    p[..., 0:2] = xy
    p[..., 2:4] = g.uniform(20, 120, (bs, n, 2))
    p[..., 4] = g.uniform(0, 1, (bs, n)) ** 2
    p[..., 5:] = g.uniform(0, 1, (bs, n, nc))
    return p


def test_oracle_hand_case():
    # three boxes of one class: the second overlaps the first (IoU 0.68 > 0.45) and is dropped, the third is apart
    pred = np.array([[[50, 50, 20, 20, 0.9, 1.0], [52, 52, 20, 20, 0.8, 1.0], [100, 100, 20, 20, 0.7, 1.0], [10, 10, 5, 5, 0.1, 1.0]]], np.float32)
    out, kept = ON.non_max_suppression(pred, 0.25, 0.45)
    assert kept[0].tolist() == [0, 2]
    np.testing.assert_allclose(out[0], [[40, 40, 60, 60, 0.9, 0], [90, 90, 110, 110, 0.7, 0]], rtol=0, atol=1e-6)
    # different classes do not suppress each other (class offset), unless agnostic
    pred2 = np.array([[[50, 50, 20, 20, 0.9, 1.0, 0.0], [52, 52, 20, 20, 0.8, 0.0, 1.0]]], np.float32)
    assert ON.non_max_suppression(pred2, 0.25, 0.45)[1][0].tolist() == [0, 1]
    assert ON.non_max_suppression(pred2, 0.25, 0.45, agnostic=True)[1][0].tolist() == [0]
    assert ON.non_max_suppression(pred2, 0.25, 0.45, classes=[1])[1][0].tolist() == [1]
    assert ON.non_max_suppression(pred2, 0.25, 0.45, max_det=1)[1][0].tolist() == [0]


@pytest.mark.parametrize("nc,agnostic", [(1, False), (3, False), (3, True)])
def test_oracle_greedy_properties(nc, agnostic):
    pred = _random_pred(2, 600, nc, 7)
    conf, thr = 0.2, 0.45
    out, kept = ON.non_max_suppression(pred, conf, thr, agnostic=agnostic, max_det=10000)
    for b in range(2):
        d = out[b]
        assert d.shape[0] > 5
        assert np.all(np.diff(d[:, 4]) <= 0)                                   # sorted by confidence
        off = 0.0 if agnostic else ON.MAX_WH
        bx = d[:, :4] + d[:, 5:6] * off
        for i in range(len(d)):                                               # kept boxes do not suppress each other
            for j in range(i):
                assert _iou(bx[j], bx[i]) <= thr + 1e-6
        # every candidate that was dropped overlaps a kept box of higher (or equal) confidence
        x = pred[b]
        cand = np.nonzero(x[:, 4] > conf)[0]
        sc = (x[cand, 5:] * x[cand, 4:5])
        cls = sc.argmax(1)
        sc = sc.max(1)
        ok = sc > conf
        cand, sc, cls = cand[ok], sc[ok], cls[ok]
        boxes = ON.xywh2xyxy(x[cand, :4]) + cls[:, None].astype(np.float32) * off
        kept_set = set(kept[b].tolist())
        for i, ci in enumerate(cand):
            if ci in kept_set:
                continue
            assert any(_iou(bk, boxes[i]) > thr - 1e-6 and sk >= sc[i] for bk, sk in zip(bx, d[:, 4]))


@pytest.mark.gpu
@pytest.mark.parametrize("nc,agnostic,classes,conf,max_det", [(1, False, None, 0.25, 300), (1, False, None, 0.001, 300), (3, False, None, 0.2, 300),
                                                                (3, True, None, 0.2, 50), (4, False, [0, 2], 0.1, 300)])
def test_hip_nms_matches_oracle(nc, agnostic, classes, conf, max_det):
    import lead_yolo_amd as L
    dev = torch.device("cuda:0")
    pred = _random_pred(3, 2500, nc, 11 + nc)
    want, want_idx = ON.non_max_suppression(pred, conf, 0.45, classes=classes, agnostic=agnostic, max_det=max_det)
    got = L.non_max_suppression(torch.from_numpy(pred).to(dev), conf, 0.45, classes=classes, agnostic=agnostic, max_det=max_det)
    dets, count, keep = L.nms_padded(torch.from_numpy(pred).to(dev), conf, 0.45, classes=classes, agnostic=agnostic, max_det=max_det)
    for b in range(3):
        assert int(count[b]) == len(want_idx[b])
        assert keep[b, :len(want_idx[b])].cpu().tolist() == want_idx[b].tolist()           # the same boxes, in the same order: bit-exact
        np.testing.assert_array_equal(got[b].cpu().numpy(), want[b])
        assert float(dets[b, len(want_idx[b]):].abs().sum()) == 0.0


def test_oracle_multi_label_hand_case():
    """multi_label (utils/general.py:921, 951-955): a box whose two class scores both pass becomes two detections (one per class, class-offset
    boxes do not suppress each other); with best-class-only it is one"""
    pred = np.array([[[50, 50, 20, 20, 1.0, 0.9, 0.8, 0.05],            # classes 0 and 1 pass
                      [52, 50, 20, 20, 1.0, 0.1, 0.7, 0.05],            # class 1 only: overlaps the first box, lower score -> suppressed within class 1
                      [150, 150, 10, 10, 0.9, 0.05, 0.05, 0.6]]], np.float32)
    out, idx = ON.non_max_suppression(pred, 0.25, 0.45, multi_label=True)
    assert idx[0].tolist() == [0 * 3 + 0, 0 * 3 + 1, 2 * 3 + 2]
    np.testing.assert_allclose(out[0][:, 4], [0.9, 0.8, 0.54], rtol=1e-6)
    assert out[0][:, 5].tolist() == [0.0, 1.0, 2.0]
    out1, idx1 = ON.non_max_suppression(pred, 0.25, 0.45, multi_label=False)
    assert idx1[0].tolist() == [0, 1, 2] and out1[0][:, 5].tolist() == [0.0, 1.0, 2.0]      # best class only: box 1 (class 1) survives, no class-1 twin of box 0


@pytest.mark.gpu
@pytest.mark.parametrize("nc,agnostic,classes,conf,max_det", [(3, False, None, 0.2, 300), (5, True, None, 0.15, 100), (4, False, [1, 3], 0.1, 300),
                                                                (2, False, None, 0.001, 300)])
def test_hip_multi_label_nms_matches_oracle(nc, agnostic, classes, conf, max_det):
    """val.py's NMS setting for nc > 1 (multi_label=True): kept (box, class) pairs bit-exact vs the oracle, in the same order"""
    import lead_yolo_amd as L
    dev = torch.device("cuda:0")
    pred = _random_pred(3, 2000, nc, 31 + nc)
    want, want_idx = ON.non_max_suppression(pred, conf, 0.45, classes=classes, agnostic=agnostic, max_det=max_det, multi_label=True)
    got = L.non_max_suppression(torch.from_numpy(pred).to(dev), conf, 0.45, classes=classes, agnostic=agnostic, max_det=max_det, multi_label=True)
    _, count, keep = L.nms_padded(torch.from_numpy(pred).to(dev), conf, 0.45, classes=classes, agnostic=agnostic, max_det=max_det, multi_label=True)
    total = 0
    for b in range(3):
        assert int(count[b]) == len(want_idx[b])
        assert keep[b, :len(want_idx[b])].cpu().tolist() == want_idx[b].tolist()
        np.testing.assert_array_equal(got[b].cpu().numpy(), want[b])
        total += len(want_idx[b])
    assert total > 20


@pytest.mark.gpu
def test_hip_nms_edge_cases():
    import lead_yolo_amd as L
    dev = torch.device("cuda:0")
    empty = torch.zeros((2, 100, 6), device=dev)
    out = L.non_max_suppression(empty)
    assert [tuple(o.shape) for o in out] == [(0, 6), (0, 6)]
    one = torch.tensor([[[50.0, 50, 20, 20, 0.9, 1.0]]], device=dev)
    out = L.non_max_suppression(one)
    np.testing.assert_allclose(out[0].cpu().numpy(), [[40, 40, 60, 60, 0.9, 0]], atol=1e-6)
    assert [tuple(o.shape) for o in L.non_max_suppression(torch.zeros((1, 10, 8), device=dev), multi_label=True)] == [(0, 6)]
    with pytest.raises(NotImplementedError):
        L.non_max_suppression(torch.zeros((1, 10, 8), device=dev), labels=[torch.zeros(1, 5)])
    with pytest.raises(RuntimeError):
        L.non_max_suppression(torch.zeros((1, 10, 6)))
    # model in validation mode hands (inference_out, loss_out)
    out = L.non_max_suppression((one, None))
    assert out[0].shape == (1, 6)


# ---- edges of ly_nms_greedy: truncation at max_nms, the bitset's tail word, max_det, exact score ties, class filters at nc >= 64 -----------
# Every case below is compared bit for bit.  A pair whose IoU lies within rounding of iou_thres could legitimately flip between numpy and
# the device (different contraction of the same fp32 expression), so a case only counts when the oracle's keep set is the same with the IoU
# evaluated in float32 and in float64: `oracle_keep_stable` asserts that, on the CPU for every synthetic case and again inside each GPU test.
def _nms64(boxes, scores, iou_thres):
    """oracle.nms.nms with the IoU arithmetic in float64 (same fp32 boxes, same fp32 threshold)"""
    boxes = boxes.astype(np.float64)
    thr = np.float64(np.float32(iou_thres))
    n = boxes.shape[0]
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    alive = np.ones(n, dtype=bool)
    keep = []
    for i in range(n):
        if not alive[i]:
            continue
        keep.append(i)
        j = np.arange(i + 1, n)[alive[i + 1:]]
        if j.size == 0:
            continue
        iw = np.maximum(np.minimum(boxes[i, 2], boxes[j, 2]) - np.maximum(boxes[i, 0], boxes[j, 0]), 0.0)
        ih = np.maximum(np.minimum(boxes[i, 3], boxes[j, 3]) - np.maximum(boxes[i, 1], boxes[j, 1]), 0.0)
        inter = iw * ih
        alive[j[inter / (area[i] + area[j] - inter) > thr]] = False
    return np.asarray(keep, dtype=np.int64)


def oracle_keep_stable(pred, conf, iou=0.45, **kw):
    """the oracle's result, after asserting that its keep set does not depend on the precision of the IoU arithmetic"""
    want, idx = ON.non_max_suppression(pred, conf, iou, **kw)
    saved = ON.nms
    ON.nms = _nms64
    try:
        _, idx64 = ON.non_max_suppression(pred, conf, iou, **kw)
    finally:
        ON.nms = saved
    for a, b in zip(idx, idx64):
        assert np.array_equal(a, b), "an IoU of this case is within rounding of the threshold: pick another seed"
    return want, idx


MAX_NMS_EDGE = ON.MAX_NMS


def _keep_with_max_nms(pred, conf, max_nms, **kw):
    """the oracle's kept indices with its cut moved to max_nms"""
    saved = ON.MAX_NMS
    ON.MAX_NMS = max_nms
    try:
        return ON.non_max_suppression(pred, conf, 0.45, **kw)[1]
    finally:
        ON.MAX_NMS = saved


def _count_case(n, seed):
    """one image, 30100 single-class boxes in 12 tight clusters, every score above the threshold; objectness 0 on all but n random rows"""
    N = 30100
    p = _random_pred(1, N, 1, seed)
    g = np.random.default_rng(seed + 1)
    p[..., 4] = g.uniform(0.1, 1.0, (1, N))
    p[..., 5] = g.uniform(0.1, 1.0, (1, N))
    perm = g.permutation(N)
    p[0, perm[n:], 4] = 0.0
    if n >= MAX_NMS_EDGE:
        # the candidate with the lowest score stands alone, far from the clusters: nothing suppresses it, so it is kept exactly when the cut
        # at max_nms leaves it in — rank 29999 (n = 30000) is inside, rank 30000 (n = 30001) is the first one outside
        live = perm[:n]
        last = live[np.argmin((p[0, live, 4] * p[0, live, 5]))]
        p[0, last, 0:2] = 5000.0
    return p


def _grid_case(seed):
    """1600 disjoint boxes: nobody suppresses anybody, max_det cuts"""
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
    p = np.zeros((1, 1600, 6), np.float32)
    p[0, :, 0], p[0, :, 1] = xx.reshape(-1) * 16 + 8, yy.reshape(-1) * 16 + 8
    p[0, :, 2:4] = g.uniform(4, 12, (1600, 2))
    p[0, :, 4] = g.uniform(0.3, 1.0, 1600)
    p[0, :, 5] = 1.0
    return p


def _first_takes_all_case(seed):
    """row 700 has the top score; every other box is that box moved by a pixel or two: all suppressed by it"""
    g = np.random.default_rng(seed)
    p = np.zeros((1, 1500, 6), np.float32)
    p[0, :, 0:2] = 300 + g.uniform(-2, 2, (1500, 2))
    p[0, :, 2:4] = 100 + g.uniform(-2, 2, (1500, 2))
    p[0, :, 4] = g.uniform(0.3, 0.9, 1500)
    p[0, :, 5] = 1.0
    p[0, 700, 4] = 0.95
    return p


def _tie_case(seed):
    """600 rows = 200 boxes, each three times with the SAME score: once more on the spot (rows i and 200 + i overlap fully) and once 3000 px
    away (row 400 + i, apart from both)"""
    base = _random_pred(1, 200, 1, seed, cluster=False)
    base[..., 0:2] = np.clip(base[..., 0:2], 50, 2500)
    base[..., 4] = np.maximum(base[..., 4], 0.3)
    base[..., 5] = 1.0
    far = base.copy()
    far[..., 0] += 3000
    return np.concatenate((base, base.copy(), far), 1)


_COUNT_CASES = [(1, 300), (31, 300), (32, 1), (33, 300), (255, 1000), (256, 300), (257, 300), (30000, 1000), (30001, 1000)]      # (max_det 1000: the walk must reach the last rank)


def _edge_case(name):
    """-> (pred, conf_thres, kwargs)"""
    if name.startswith("count"):
        n, max_det = (int(v) for v in name.split("-")[1:])
        return _count_case(n, 500 + n), 0.001, dict(max_det=max_det)
    if name.startswith("grid"):
        return _grid_case(61), 0.25, dict(max_det=int(name.split("-")[1]))
    if name == "first-takes-all":
        return _first_takes_all_case(62), 0.25, dict(max_det=300)
    if name == "ties":
        return _tie_case(63), 0.25, dict(max_det=1000)
    if name == "nc64-class63":
        return _random_pred(2, 1500, 64, 64), 0.05, dict(classes=[63], max_det=300)
    raise KeyError(name)


EDGE_CASES = [f"count-{n}-{d}" for n, d in _COUNT_CASES] + ["grid-1", "grid-300", "grid-1000", "first-takes-all", "ties", "nc64-class63"]


def _check_edge_premise(name, pred, conf, kw, idx):
    """what makes the case mean something, from the oracle's side"""
    if name.startswith("count"):
        n = int(name.split("-")[1])
        x = pred[0]
        assert int(((x[:, 4] > conf) & (x[:, 4] * x[:, 5] > conf)).sum()) == n          # the candidate count the kernel sees
        assert len(idx[0]) >= 1
        if n >= MAX_NMS_EDGE:
            # the position of the cut decides the result: one candidate fewer or more than max_nms = 30000 changes the kept set
            lone = int(np.nonzero(x[:, 0] == 5000.0)[0][0])
            assert (lone in idx[0].tolist()) == (n == MAX_NMS_EDGE)
            other = _keep_with_max_nms(pred, conf, MAX_NMS_EDGE - 1 if n == MAX_NMS_EDGE else MAX_NMS_EDGE + 1, **kw)
            assert (lone in other[0].tolist()) == (n != MAX_NMS_EDGE)
            assert not np.array_equal(other[0], idx[0])
    elif name.startswith("grid"):
        assert len(idx[0]) == kw["max_det"]                                            # max_det is what stops it
    elif name == "first-takes-all":
        assert idx[0].tolist() == [700]
    elif name == "ties":
        k = set(idx[0].tolist())
        assert len(k) > 100
        for i in range(200):                                                           # of two identical rows the lower index; the far twin too
            assert (200 + i) not in k
            assert (i in k) == ((400 + i) in k)
        assert sum(1 for i in range(200) if i in k) > 50
    elif name == "nc64-class63":
        assert sum(len(v) for v in idx) > 5


@pytest.mark.parametrize("name", EDGE_CASES)
def test_edge_case_premises_hold_in_the_oracle(name):
    """CPU: every synthetic edge case keeps the same boxes with float32 and float64 IoU arithmetic, and does what its name says"""
    pred, conf, kw = _edge_case(name)
    _, idx = oracle_keep_stable(pred, conf, **kw)
    _check_edge_premise(name, pred, conf, kw, idx)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE_CASES)
def test_hip_nms_edges_match_oracle(name):
    """ly_nms_greedy at candidate counts around the bitset's word (32) and block (256) sizes and around max_nms = 30000 (the lowest-scored candidate stands alone: at
    30000 it is the last one inside the cut and kept, at 30001 it is cut before the walk — _check_edge_premise asserts that the oracle's
    result changes when its cut moves by one), with max_det 1 / 300 / 1000, everything suppressed by the first box, nothing
    suppressed at all, exact score ties (stable: ascending candidate index), and a class filter on the last representable class"""
    import lead_yolo_amd as L
    dev = torch.device("cuda:0")
    pred, conf, kw = _edge_case(name)
    want, want_idx = oracle_keep_stable(pred, conf, **kw)
    _check_edge_premise(name, pred, conf, kw, want_idx)
    pt = torch.from_numpy(pred).to(dev)
    got = L.non_max_suppression(pt, conf, 0.45, **kw)
    dets, count, keep = L.nms_padded(pt, conf, 0.45, **kw)
    for b in range(pred.shape[0]):
        assert int(count[b]) == len(want_idx[b])
        assert keep[b, :len(want_idx[b])].cpu().tolist() == want_idx[b].tolist()
        np.testing.assert_array_equal(got[b].cpu().numpy(), want[b])
        assert float(dets[b, len(want_idx[b]):].abs().sum()) == 0.0


@pytest.mark.gpu
def test_hip_nms_class_filter_above_63_is_refused():
    import lead_yolo_amd as L
    pred = torch.from_numpy(_random_pred(1, 100, 80, 65)).to(torch.device("cuda:0"))
    with pytest.raises(NotImplementedError):
        L.non_max_suppression(pred, 0.05, 0.45, classes=[70])
