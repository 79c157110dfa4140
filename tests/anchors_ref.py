"""numpy restatements of utils/autoanchor.py as csrc/ly_anchors.hip computes it (float32 operations one by one, EXACT float64 sums), the
seeded data of tests/test_anchors_host.py and tests/test_gpu_anchors.py, and the planted defects.  Everything here is computed once
(lru_cache) and shared; callers must not modify what they get.

`defect=` plants one mistake in a restatement (the host tests show that each changes the result on the test data, so a device kernel
with that mistake cannot pass): "no_recip" (1 / r omitted), "ge" (`>` taken as `>=` at the threshold), "no_reeval" (a candidate behind an
accepted one is not evaluated again from the new k), "no_clip" (clip(min=2) omitted), "stale_assign" (a centroid updated from the previous
iteration's assignment)."""
import functools
import math

import numpy as np

F32 = np.float32
KMEANS_THRESH, KMEANS_MAX_ITER = 1e-5, 100


# ---- label sizes ---------------------------------------------------------------------------------------------------------------------
def label_wh(labels, shapes, img_size, scale=None):
    """autoanchor.py:34-36 / 128-129, literally: float64 products, one rounding to float32"""
    shapes = np.asarray(shapes).reshape(-1, 2)
    s = img_size * shapes / shapes.max(1, keepdims=True)
    if scale is not None:
        s = s * np.asarray(scale, dtype=np.float64).reshape(-1, 1)
    rows = [np.asarray(lb, dtype=np.float64).reshape(-1, 5)[:, 3:5] * si for si, lb in zip(s, labels)]
    return np.concatenate(rows).astype(F32) if rows else np.zeros((0, 2), F32)


# ---- metric --------------------------------------------------------------------------------------------------------------------------
def metric_x(wh, k, defect=None):
    """x [n, na], best [n]: float32 throughout (numpy's float32 `/` is correctly rounded)"""
    wh, k = np.asarray(wh, dtype=F32), np.asarray(k, dtype=F32)
    with np.errstate(divide="ignore"):
        r = wh[:, None] / k[None]
        x = (r if defect == "no_recip" else np.minimum(r, F32(1) / r)).min(2)
    return x, x.max(1)


def metric_terms(wh, k, thr, defect=None):
    """(the float32 fitness terms best * (best > 1/thr) that are non-zero, count best > 1/thr, count x > 1/thr)"""
    ithr = F32(1.0 / thr)                                  # torch compares a float32 tensor with the scalar rounded to float32
    x, best = metric_x(wh, k, defect)
    above = (lambda a: a >= ithr) if defect == "ge" else (lambda a: a > ithr)
    return best[above(best)], int(above(best).sum()), int(above(x).sum())


def metric_sums(wh, k, thr, defect=None):
    """(sum, count best, count x): the sum is exact (math.fsum), as the device's is"""
    t, nb, nx = metric_terms(wh, k, thr, defect)
    return math.fsum(t.astype(np.float64)), nb, nx


def fitness_sum(wh, k, thr, defect=None):
    return metric_sums(wh, np.asarray(k).astype(F32), thr, defect)[0]


# ---- evolution -----------------------------------------------------------------------------------------------------------------------
def evolve(wh, k, v, thr, defect=None, batch=32):
    """the serial chain of autoanchor.py:156-165 over the mutation table v [gen, na, 2]: -> k (float64), fitness sum, accepted generations.
    "no_reeval" needs `batch`: inside a batch every candidate is formed from the k the batch started with, and ALL that beat the running f
    are accepted in turn."""
    k = np.asarray(k, dtype=np.float64).reshape(-1, 2).copy()
    f, accepted = fitness_sum(wh, k, thr, defect), []
    clip = (lambda a: a) if defect == "no_clip" else (lambda a: a.clip(min=2.0))
    k0 = k
    for g in range(len(v)):
        if defect == "no_reeval":
            if g % batch == 0:
                k0 = k.copy()
            kg = clip(k0 * v[g])
        else:
            kg = clip(k * v[g])
        fg = fitness_sum(wh, kg, thr, defect)
        if fg > f:
            f, k = fg, kg.copy()
            accepted.append(g)
    return k, f, accepted


# ---- k-means -------------------------------------------------------------------------------------------------------------------------
def lloyd_assign(pts, cent):
    """pts [n, 2], cent [R, na, 2] float32 -> assign [R, n], d2 [R, n, na] (float32: dx*dx + dy*dy as written)"""
    d = pts[None, :, None, :] - cent[:, None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    return d2.argmin(2), d2                                # argmin: the first of equal minima


def lloyd_step(pts, cent, assign_prev=None):
    """one iteration: -> assign, count [R, na], new cent (float32(float64 sum / count); an empty centroid keeps the run's centroids),
    dist [R] (float64 sum of the float32 distances / n), empty [R], d2.  assign_prev: the "stale_assign" defect."""
    pts, cent = np.asarray(pts, dtype=F32), np.asarray(cent, dtype=F32)
    assign, d2 = lloyd_assign(pts, cent)
    use = assign if assign_prev is None else assign_prev
    R, na = cent.shape[:2]
    count = np.stack([np.bincount(use[r], minlength=na) for r in range(R)])
    new = cent.copy()
    p64 = pts.astype(np.float64)
    for r in range(R):
        if (count[r] == 0).any():
            continue
        for c in range(na):
            new[r, c] = (p64[use[r] == c].sum(0) / count[r, c]).astype(F32)
    dmin = np.sqrt(np.take_along_axis(d2, assign[..., None], 2)[..., 0])                       # float32 sqrt, correctly rounded
    dist = dmin.astype(np.float64).sum(1) / len(pts)
    return assign, count, new, dist, (count == 0).any(1), d2


def lloyd(pts, init, thresh=KMEANS_THRESH, max_iter=KMEANS_MAX_ITER, defect=None, trace=None):
    """scipy's _kmeans for R runs at once, as anchors.lloyd: a run closes at |previous distortion - distortion| <= thresh or when a centroid
    loses its points (discarded); -> dict(run, iters, run_iters, dist, discarded, cent).  trace: a list that receives, per iteration,
    (open runs, d2 of the open runs, |delta distortion| of the open runs)."""
    cent = np.asarray(init, dtype=F32).copy()
    R = cent.shape[0]
    closed, discarded = np.zeros(R, bool), np.zeros(R, bool)
    dist, run_iters, it = np.full(R, np.inf), np.zeros(R, np.int64), 0
    prev_assign = None
    while it < max_iter and not closed.all():
        o = np.flatnonzero(~closed)
        stale = prev_assign[o] if defect == "stale_assign" and prev_assign is not None else None
        assign, _, new, d, empty, d2 = lloyd_step(pts, cent[o], stale)
        if prev_assign is None:
            prev_assign = np.zeros((R, len(pts)), np.int64)
        prev_assign[o] = assign
        with np.errstate(invalid="ignore"):
            delta = np.abs(dist[o] - d)
        cent[o], dist[o] = new, d
        run_iters[o] += 1
        discarded[o] = empty
        closed[o] = empty | (delta <= thresh)
        it += 1
        if trace is not None:
            trace.append((o, d2, delta))
    ok = np.flatnonzero(~discarded)
    run = int(ok[np.argmin(dist[ok])]) if len(ok) else -1
    return dict(run=run, iters=it, run_iters=run_iters, dist=dist, discarded=discarded, cent=cent)


def kmeans_init(n_points, n, runs=30, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(n_points, n, replace=False) for _ in range(runs)]).astype(np.int64)


def whiten(wh):
    """(wh / s, s): s = float32 of the float64 standard deviation"""
    s = np.asarray(wh, dtype=np.float64).std(0).astype(F32)
    return (np.asarray(wh, dtype=F32) / s).astype(F32), s


def margins(d2):
    """relative gap between every point's nearest and second-nearest squared distance, [..., n]"""
    s = np.sort(d2.astype(np.float64), axis=-1)
    return (s[..., 1] - s[..., 0]) / np.maximum(s[..., 1], 1e-300)


# ---- seeded data ---------------------------------------------------------------------------------------------------------------------
def _sizes(rng, n, lo, hi, aspect):
    """n (w, h) pairs in pixels, log-uniform long side in [lo, hi], aspect (h / w) log-uniform in `aspect`"""
    w = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    a = np.exp(rng.uniform(np.log(aspect[0]), np.log(aspect[1]), n))
    return np.stack([w, w * a], 1)


@functools.lru_cache(None)
def wh_set(seed, n=4096, kind="sar"):
    """float32 [n, 2] label sizes in pixels: "sar" small and narrow (ships in SAR scenes), "coco" spread as the COCO anchors are"""
    rng = np.random.default_rng(seed)
    wh = _sizes(rng, n, 3.0, 60.0, (0.2, 0.6)) if kind == "sar" else _sizes(rng, n, 12.0, 380.0, (0.6, 1.7))
    wh = wh.astype(F32)
    wh.setflags(write=False)
    return wh


@functools.lru_cache(None)
def dataset(seed, n_img=48, kind="sar", img_size=640, empty_every=7):
    """(labels: list of [ni, 5] float64, shapes [n_img, 2] int (w, h)): every `empty_every`-th image has no labels"""
    rng = np.random.default_rng(seed)
    shapes = np.stack([rng.integers(300, 900, n_img), rng.integers(300, 900, n_img)], 1)
    norm = img_size * shapes / shapes.max(1, keepdims=True)
    labels = []
    for i in range(n_img):
        ni = 0 if (empty_every and i % empty_every == 3) else int(rng.integers(1, 40))
        px = _sizes(rng, ni, 4.0, 50.0, (0.2, 0.6)) if kind == "sar" else _sizes(rng, ni, 14.0, 330.0, (0.6, 1.7))
        whn = np.minimum(px / norm[i], 0.999)
        xy = rng.uniform(0.1, 0.9, (ni, 2))
        labels.append(np.concatenate([np.zeros((ni, 1)), xy, whn], 1))
    return labels, shapes


COCO_ANCHORS = np.array([[10, 13], [16, 30], [33, 23], [30, 61], [62, 45], [59, 119], [116, 90], [156, 198], [373, 326]], dtype=F32)


@functools.lru_cache(None)
def step_points(seed, n, R, na=9):
    """(pts [n, 2] float32, cent [R, na, 2] float32) for ONE Lloyd iteration: every point's nearest and second-nearest squared distances
    differ by more than 1e-5 relative in every run (seeded rejection: a point that fails is drawn again; none is left out)"""
    rng = np.random.default_rng(seed)
    cent = np.exp(rng.uniform(np.log(0.3), np.log(6.0), (R, na, 2))).astype(F32)
    pts = np.exp(rng.uniform(np.log(0.2), np.log(8.0), (n, 2))).astype(F32)
    for _ in range(100):
        bad = np.flatnonzero((margins(lloyd_assign(pts, cent)[1]) <= 1e-5).any(0))
        if len(bad) == 0:
            break
        pts[bad] = np.exp(rng.uniform(np.log(0.2), np.log(8.0), (len(bad), 2))).astype(F32)
    else:
        raise AssertionError("step_points: rejection did not converge")
    pts.setflags(write=False)
    cent.setflags(write=False)
    return pts, cent


def loop_premises(wh, n, runs, seed):
    """runs the restated whole loop over wh and measures premise (b): -> (result, points that fail the margin, closest |delta - 1e-5|,
    gap of the two best distortions)"""
    pts, _ = whiten(wh)
    trace = []
    res = lloyd(pts, pts[kmeans_init(len(pts), n, runs, seed)], trace=trace)
    bad = np.zeros(len(pts), bool)
    near = np.inf
    for _, d2, delta in trace:
        bad |= (margins(d2) <= 1e-5).any(0)
        fin = delta[np.isfinite(delta)]
        if len(fin):
            near = min(near, float(np.abs(fin - KMEANS_THRESH).min()))
    d = np.sort(res["dist"][~res["discarded"]])
    gap = float(d[1] - d[0]) if len(d) > 1 else np.inf
    return res, np.flatnonzero(bad), near, gap


@functools.lru_cache(None)
def loop_wh(seed, n_points=512, n=9, runs=30):
    """float32 [n_points, 2] sizes for the whole k-means loop (seed `seed` for the initial centroids too) that satisfy premise (b) in
    every iteration of the restated loop: seeded rejection, a point that fails in any iteration is drawn again and the loop re-run"""
    rng = np.random.default_rng(seed)
    wh = _sizes(rng, n_points, 3.0, 60.0, (0.2, 0.6)).astype(F32)
    for _ in range(200):
        _, bad, near, gap = loop_premises(wh, n, runs, seed)
        if len(bad) == 0 and near > 1e-9 and gap > 1e-9:
            wh.setflags(write=False)
            return wh
        redo = bad if len(bad) else np.array([int(rng.integers(n_points))])
        wh[redo] = _sizes(rng, len(redo), 3.0, 60.0, (0.2, 0.6)).astype(F32)
    raise AssertionError("loop_wh: rejection did not converge")
