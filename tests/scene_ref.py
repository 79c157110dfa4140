"""numpy restatements of csrc/ly_scene.hip (the contracts in include/lead_yolo_hip.h) and the seeded inputs the merge tests share: the host
tests (tests/test_scene_host.py) check the restatements by hand-written cases and hold every input to the premise under which a float32 kernel
and a float64 loop must take the same decisions; the GPU tests (tests/test_gpu_scene.py) hold the kernels to the restatements on these inputs."""
import functools

import numpy as np

FILL = 114


def tiles_ref(scene, origins, T):
    """ly_scene_tiles_u8: scene uint8 [H, W, 3] (BGR) or [H, W] -> [n, 3, T, T] RGB planes, 114 past the scene's edges"""
    scene = np.asarray(scene)
    H, W = scene.shape[:2]
    src = scene[:, :, ::-1] if scene.ndim == 3 else np.stack([scene] * 3, -1)
    out = np.full((len(origins), 3, T, T), FILL, np.uint8)
    for k, (y0, x0) in enumerate(np.asarray(origins).tolist()):
        win = src[y0:y0 + T, x0:x0 + T]
        out[k, :, :win.shape[0], :win.shape[1]] = win.transpose(2, 0, 1)
    return out


def collect_ref(dets, counts, origins, H, W):
    """ly_scene_collect in float32, the same operations: -> (boxes [n * max_det, 6], score [n * max_det])"""
    dets = np.asarray(dets, np.float32)
    n, md = dets.shape[:2]
    boxes, score = np.zeros((n * md, 6), np.float32), np.full(n * md, -1, np.float32)
    fH, fW = np.float32(H), np.float32(W)
    for t in range(n):
        y0, x0 = np.float32(origins[t][0]), np.float32(origins[t][1])
        for r in range(int(counts[t])):
            p, o = dets[t, r], boxes[t * md + r]
            o[0] = min(max(np.float32(p[0] + x0), np.float32(0)), fW)
            o[1] = min(max(np.float32(p[1] + y0), np.float32(0)), fH)
            o[2] = min(max(np.float32(p[2] + x0), np.float32(0)), fW)
            o[3] = min(max(np.float32(p[3] + y0), np.float32(0)), fH)
            o[4], o[5] = p[4], p[5]
            score[t * md + r] = p[4]
    return boxes, score


def metric_matrix(boxes, metric, dtype):
    """m(i, j) of the header for every pair, one operation per step in `dtype` (float32: the kernel's arithmetic; float64: the judge's)"""
    b = np.asarray(boxes)[:, :4].astype(dtype)
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    zero = dtype(0)
    iw = np.maximum(np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]), zero)
    ih = np.maximum(np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]), zero)
    inter = iw * ih
    area = (x2 - x1) * (y2 - y1)
    den = (area[:, None] + area[None]) - inter if metric == "iou" else np.minimum(area[:, None], area[None])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den == zero, zero, inter / den).astype(dtype)


def evaluated_pairs(boxes, score, max_det_tile, agnostic):
    """[N, N] bool: the pairs the rule may evaluate — both live, different tiles, same class (any class when agnostic), i != j"""
    boxes, score = np.asarray(boxes), np.asarray(score)
    live = score >= 0
    tile = np.arange(len(boxes)) // max_det_tile
    pair = live[:, None] & live[None] & (tile[:, None] != tile[None])
    if not agnostic:
        pair &= boxes[:, 5][:, None] == boxes[:, 5][None]
    return pair


def margin(boxes, metric, thres, score=None, max_det_tile=1, agnostic=True):
    """the smallest |m - thres| over all pairs the rule would evaluate (float64); inf when there is none.  Defaults: every row live, a tile of
    its own, classes ignored — all pairs"""
    boxes = np.asarray(boxes)
    score = np.zeros(len(boxes)) if score is None else score
    pair = evaluated_pairs(boxes, score, max_det_tile, agnostic)
    if not pair.any():
        return np.inf
    return float(np.abs(metric_matrix(boxes, metric, np.float64) - thres)[pair].min())


def merge_ref(boxes, score, max_det_tile, metric="ios", thres=0.5, agnostic=False, max_det=3000, max_merge=30000, defect=None, stats=None):
    """ly_scene_nms (around its stable descending sort) as a plain sequential loop in float64 -> the kept row indices, in kept order.
    defect: one of the planted mutations the judge must catch — "cls_offset" (classes separated by shifting boxes by cls * 7680 instead of
    comparing them), "no_exempt" (pairs of one tile are judged too), "unstable" (equal scores in the opposite row order), "ge" (>= thres).
    stats: a dict that receives `suppressed`, the number of candidates dropped."""
    boxes, score = np.asarray(boxes, np.float64), np.asarray(score, np.float64)
    idx = np.arange(len(score))
    order = np.lexsort((-idx if defect == "unstable" else idx, -score))           # descending score, ties by ascending (descending) row
    order = [int(j) for j in order if score[j] >= 0][:max_merge]
    b = boxes[:, :4].copy()
    if defect == "cls_offset" and not agnostic:
        b += boxes[:, 5:6] * 7680.0

    def m(i, j):
        iw = max(min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0]), 0.0)
        ih = max(min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1]), 0.0)
        inter = iw * ih
        ai, aj = (b[i, 2] - b[i, 0]) * (b[i, 3] - b[i, 1]), (b[j, 2] - b[j, 0]) * (b[j, 3] - b[j, 1])
        den = (ai + aj) - inter if metric == "iou" else min(ai, aj)
        return 0.0 if den == 0 else inter / den

    kept, dropped = [], 0
    for j in order:
        if len(kept) >= max_det:
            break
        for i in kept:
            if i // max_det_tile == j // max_det_tile and defect != "no_exempt":
                continue
            if not (agnostic or defect == "cls_offset" or boxes[i, 5] == boxes[j, 5]):
                continue
            v = m(i, j)
            if v >= thres if defect == "ge" else v > thres:
                dropped += 1
                break
        else:
            kept.append(j)
    if stats is not None:
        stats["suppressed"] = dropped
    return kept


# ---- the seeded inputs of the merge tests ----------------------------------------------------------------------------------------------------
def clustered(seed, n_tiles, mdt, n_clusters, lo, nc=2, extent=1500.0, ties=False, shift=0.0):
    """n_tiles x mdt rows as ly_scene_collect leaves them: tile t has counts[t] in [lo, mdt] live rows — jittered, scaled or border-cut copies
    of n_clusters ship-sized boxes, so that a cluster has members in several tiles and several members in one tile — then padding rows (zeros,
    score -1).  ties: confidences on a grid of 0.05, so that many are equal."""
    rng = np.random.default_rng(seed)
    boxes, score = np.zeros((n_tiles * mdt, 6), np.float32), np.full(n_tiles * mdt, -1, np.float32)
    cxy, wh = rng.uniform(60, extent - 60, (n_clusters, 2)), rng.uniform(10, 100, (n_clusters, 2))
    cls = rng.integers(0, nc, n_clusters)
    counts = rng.integers(lo, mdt + 1, n_tiles)
    for t in range(n_tiles):
        conf = np.sort(rng.uniform(0.05, 1.0, counts[t]))[::-1]
        for r in range(counts[t]):
            c = rng.integers(n_clusters)
            w, h = wh[c] * rng.uniform(0.7, 1.2, 2)
            x, y = cxy[c] + wh[c] * rng.uniform(-0.25, 0.25, 2)
            box = np.array([x - w / 2, y - h / 2, x + w / 2, y + h / 2])
            if rng.random() < 0.3:                                                # cut by a tile border: a part of the box
                k = rng.integers(4)
                box[k] = box[k] + (box[(k + 2) % 4] - box[k]) * rng.uniform(0.3, 0.7)
            boxes[t * mdt + r, :4] = box + shift
            boxes[t * mdt + r, 4] = np.round(conf[r] * 20) / 20 if ties else conf[r]
            boxes[t * mdt + r, 5] = cls[c] if rng.random() < 0.75 else rng.integers(nc)      # overlapping boxes of different classes too
            score[t * mdt + r] = boxes[t * mdt + r, 4]
    return boxes, score


def _rows(rows, mdt, n_tiles):
    """hand-written rows {(tile, r): (x1, y1, x2, y2, conf, cls)} -> (boxes, score)"""
    boxes, score = np.zeros((n_tiles * mdt, 6), np.float32), np.full(n_tiles * mdt, -1, np.float32)
    for (t, r), row in rows.items():
        boxes[t * mdt + r] = row
        score[t * mdt + r] = row[4]
    return boxes, score


def _far():
    """scene coordinates beyond 7680: a class-1 box and a class-0 box exactly 7680 apart in x and y, in different tiles — what the cls * 7680
    offset of ly_nms_greedy lays on top of one another; and an honest duplicate pair out there"""
    return _rows({(0, 0): (9000, 1000, 9060, 1040, 0.9, 1), (1, 0): (9000 + 7680, 1000 + 7680, 9060 + 7680, 1040 + 7680, 0.8, 0),
                  (2, 0): (15000, 12000, 15080, 12030, 0.7, 0), (3, 0): (15004, 12002, 15078, 12028, 0.6, 0),
                  (3, 1): (18000.5, 300.25, 18050, 340, 0.5, 1)}, 2, 4)


def _exact():
    """small whole-number boxes whose metric is a dyadic fraction: IoS exactly 0.5 (kept under `>`, dropped under `>=`), 0.75 and 0.25"""
    return _rows({(0, 0): (0, 0, 10, 10, 0.9, 0), (1, 0): (5, 0, 15, 10, 0.8, 0),            # inter 50 / min 100 = 0.5
                  (0, 1): (100, 0, 108, 8, 0.7, 0), (1, 1): (102, 0, 110, 8, 0.6, 0),        # 48 / 64 = 0.75
                  (2, 0): (200, 0, 216, 16, 0.5, 0), (1, 2): (212, 0, 228, 16, 0.4, 0)}, 3, 3)  # 64 / 256 = 0.25


V = dict                          # a variant: the keyword arguments of merge_ref / scene_merge


@functools.lru_cache(maxsize=None)
def merge_cases():
    """name -> (boxes, score, max_det_tile, [variants], exact).  The seeds were chosen so that the premise of tests/test_scene_host.py holds.  exact: the case's metrics are computed without rounding in float32 (checked by
    the host test instead of the margin — it holds pairs AT the threshold, which is what tells `>` from `>=`)"""
    both = [V(metric="ios", thres=0.5), V(metric="iou", thres=0.45)]
    ag = [V(metric="ios", thres=0.5, agnostic=True), V(metric="iou", thres=0.45, agnostic=True)]
    cases = {}
    b, s = clustered(100, 1, 1, 1, 1)
    cases["n1"] = (b, s, 1, both, False)
    b, s = clustered(100, 2, 4, 2, 4)
    cases["n8"] = (b, s, 4, both + ag, False)
    b, s = clustered(100, 3, 37, 6, 20)                                        # N = 111
    cases["n111"] = (b, s, 37, both + ag + [V(metric="ios", thres=0.5, max_det=7), V(metric="iou", thres=0.45, agnostic=True, max_det=7)], False)
    b, s = clustered(101, 5, 61, 12, 30, nc=3)                                 # N = 305
    cases["n305"] = (b, s, 61, both + ag, False)
    b, s = clustered(101, 9, 140, 150, 126, extent=3000.0)                     # ~1200 live of N = 1260
    cases["n1260"] = (b, s, 140, both + ag[:1], False)
    b, s = clustered(100, 4, 20, 10, 20)                                       # 80 live, the merge sees 50
    cases["merge50"] = (b, s, 20, [V(metric="ios", thres=0.5, max_merge=50), V(metric="iou", thres=0.45, max_merge=50), V(metric="ios", thres=0.5)], False)
    b, s = clustered(103, 6, 33, 8, 20, ties=True)                             # N = 198, many equal scores
    cases["ties"] = (b, s, 33, both + ag, False)
    b, s = clustered(100, 4, 25, 10, 15, shift=12000.0)                        # real coordinates beyond 7680
    cases["shifted"] = (b, s, 25, both, False)
    cases["allpad"] = (np.zeros((3 * 7, 6), np.float32), np.full(3 * 7, -1, np.float32), 7, both, False)
    b, s = _far()
    cases["far"] = (b, s, 2, both + ag, False)
    b, s = _exact()
    cases["exact"] = (b, s, 3, [V(metric="ios", thres=0.5), V(metric="ios", thres=0.25), V(metric="ios", thres=0.75)], True)
    return cases
