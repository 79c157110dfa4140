"""Autoanchor on the device: the reference's `check_anchors` / `kmean_anchors` (utils/autoanchor.py), the step train.py runs before the
first epoch unless --noautoanchor is given, over labels that are already in device memory (ImageBank.labels) — csrc/ly_anchors.hip.

  label_wh        labels[:, 3:5] * shape * scale per label (float64 products, rounded once to float32)          ly_anchor_wh
  anchor_metric   bpr, aat and anchor_fitness of G candidate anchor sets in one launch                         ly_anchor_metric
  kmeans          scipy.cluster.vq.kmeans(wh / s, n, iter=30): the 30 Lloyd runs batched, a pair of launches    ly_kmeans_assign / _update
                  per iteration, 4 bytes read back per iteration (the count of runs still open)
  evolve          kmean_anchors' mutation loop: the whole [gen, na, 2] table of mutation factors is drawn up    ly_anchor_evolve_eval / _pick
                  front, `batch` speculative generations per pair of launches, 4 bytes read back per pair
  kmean_anchors, check_anchors   the reference's two functions on top of these

Stated differences from the reference
  * The reference compares float32 `torch.mean`s, whose summation order depends on the host's thread count; here fitnesses are EXACT sums
    (float32 terms in (0.25, 1] add exactly in double) and `fg > f`, `new_bpr > bpr` compare those.  The two can differ only where two
    fitnesses agree to about 1e-7 relative.  bpr / aat are count / n in double.
  * k-means starts from `n` distinct points per run drawn from a seeded numpy Generator: scipy's own draws cannot be reproduced and are not
    the contract.  The runs iterate until |previous distortion - distortion| <= 1e-5 (scipy's thresh) or 100 iterations; a run in which a
    centroid loses all its points is discarded (scipy would return fewer centroids and the reference's `assert n == len(k)` would fail).
    If every run is discarded, or there are fewer points than anchors, the reference's random fallback is taken.
  * The whitening sigmas `wh.std(0)` are computed in float64 and rounded to float32; the `>= 2 px` filter is applied to the float32 sizes.
  * Everything random comes from generators seeded with `seed` (numpy RandomState + random.Random in the reference's call order for the
    augment scale, the fallback and the mutations), never from the global ones.
  * For an ImageBank the image shapes are `bank.hw[:, ::-1]`, `load_image`'s truncated sizes: a short side can differ by under a pixel
    from the data set's native aspect ratio (`dataset.shapes`), so sizes differ from the reference's by under 1 part in the short side.

`check_anchors` writes `m.anchors[:]` in place, which bumps the buffer's version: GraphedForward.stale() / Detector.stale() report it and
a ComputeLoss built earlier re-reads the buffer.  A GraphedTrainStep that has already captured the model is NOT updated: call check_anchors
before capture, where train.py has it.  There is no CPU fallback: the label sizes must be on a GPU."""
import logging
import random

import numpy as np
import torch

from . import ops
from .model import check_anchor_order

LOGGER = logging.getLogger(__name__)
KMEANS_THRESH, KMEANS_MAX_ITER = 1e-5, 100          # scipy's `thresh` default; the iteration cap of the batched loop
MUTATION_PROB, MUTATION_SIGMA = 0.9, 0.1            # kmean_anchors' mp, s


class AnchorCheck:
    """result of check_anchors: bpr / aat of the model's anchors, new_bpr of the evolved ones (None: not evolved), the anchors in pixels
    ([na, 2] float32, sorted by area: the evolved ones if they replaced the model's), replaced"""

    def __init__(self, bpr, aat, new_bpr, anchors, replaced):
        self.bpr, self.aat, self.new_bpr, self.anchors, self.replaced = bpr, aat, new_bpr, anchors, replaced

    def __repr__(self):
        return f"AnchorCheck(bpr={self.bpr:.4f}, aat={self.aat:.2f}, new_bpr={self.new_bpr}, replaced={self.replaced})"


class Evolved:
    """result of evolve: k [na, 2] float64, f (mean fitness, exact sum / n), fsum, accepted mutations, rounds ((eval, pick) launch pairs)"""

    def __init__(self, k, fsum, n, accepted, rounds):
        self.k, self.fsum, self.f, self.accepted, self.rounds = k, fsum, fsum / n, accepted, rounds


class KMeans:
    """result of kmeans / lloyd: k [n, 2] float32 in pixels (None: every run discarded or too few points), run, iters (launch pairs),
    run_iters / dist / flags per run (flags bit 1: discarded), cent [R, n, 2] whitened centroids, s the whitening sigmas"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _device(device):
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise RuntimeError(f"autoanchor runs on the GPU (csrc/ly_anchors.hip); got device {dev} — there is no CPU fallback")
    return dev


def _flat_labels(labels, device):
    """-> (flat [N, 5] float64 device tensor, img [N] int32 device tensor, n_img).  labels: a list of per-image [ni, 5] arrays, or
    (flat device tensor, per-image counts)"""
    if isinstance(labels, tuple) and len(labels) == 2 and isinstance(labels[0], torch.Tensor) and isinstance(labels[1], np.ndarray):
        flat, nlab = labels[0], np.asarray(labels[1], dtype=np.int64)
        dev = flat.device if device is None else _device(device)
        flat = flat.to(dev, torch.float64).reshape(-1, 5).contiguous()
    else:
        dev = _device(device)
        arrs = [np.asarray(lb.cpu().numpy() if isinstance(lb, torch.Tensor) else lb, dtype=np.float64).reshape(-1, 5) for lb in labels]
        nlab = np.array([a.shape[0] for a in arrs], dtype=np.int64)
        flat = torch.from_numpy(np.concatenate(arrs, 0) if len(arrs) else np.zeros((0, 5))).to(dev)
    if flat.device.type != "cuda":
        _device(flat.device)
    if int(nlab.sum()) != flat.shape[0]:
        raise ValueError(f"label counts sum to {int(nlab.sum())}, the flat array has {flat.shape[0]} rows")
    img = torch.from_numpy(np.repeat(np.arange(len(nlab), dtype=np.int32), nlab)).to(flat.device)
    return flat, img, len(nlab)


def _source(data, device=None):
    """(labels, shapes) of an ImageBank, a duck-typed reference dataset (.labels, .shapes) or a (labels, shapes) pair; shapes (w, h)"""
    from .mosaic import ImageBank
    if isinstance(data, ImageBank):
        return (data.labels, data.nlab), data.hw[:, ::-1]
    if isinstance(data, (tuple, list)) and len(data) == 2:
        return data[0], data[1]
    if hasattr(data, "labels") and hasattr(data, "shapes"):
        return data.labels, data.shapes
    raise TypeError(f"autoanchor: expected an ImageBank, a dataset with .labels and .shapes, or a (labels, shapes) pair, got {type(data).__name__}")


def label_wh(labels, shapes, img_size, scale=None, device=None):
    """autoanchor.py:34-36 / 128-129: `shapes = img_size * shapes / shapes.max(1, keepdims=True)`, then every label's
    `l[3:5] * (shape * scale)` -> float32 [N, 2] on the device.  labels: list of per-image [ni, 5] arrays (or (flat device tensor, counts));
    shapes [n_img, 2] = (w, h); scale None or [n_img] (check_anchors' uniform(0.9, 1.1) augment scale, drawn by the caller)."""
    flat, img, n_img = _flat_labels(labels, device)
    shapes = np.asarray(shapes).reshape(-1, 2)
    if shapes.shape[0] != n_img:
        raise ValueError(f"label_wh: {n_img} label arrays and {shapes.shape[0]} shapes")
    norm = np.ascontiguousarray(img_size * shapes / shapes.max(1, keepdims=True), dtype=np.float64)
    sc = None
    if scale is not None:
        sc = np.ascontiguousarray(np.asarray(scale, dtype=np.float64).reshape(-1))
        if sc.shape[0] != n_img:
            raise ValueError(f"label_wh: {n_img} images and {sc.shape[0]} scales")
        sc = torch.from_numpy(sc).to(flat.device)
    return ops.anchor_wh(flat, img, torch.from_numpy(norm).to(flat.device), sc)


def _sets(anchors, device):
    k = torch.as_tensor(np.asarray(anchors.detach().cpu() if isinstance(anchors, torch.Tensor) else anchors, dtype=np.float32))
    if k.dim() == 2:
        k = k[None]
    if k.dim() != 3 or k.shape[2] != 2 or not 1 <= k.shape[1] <= ops.ANCHOR_NA_MAX:
        raise ValueError(f"anchors must be [na, 2] or [G, na, 2] with na <= {ops.ANCHOR_NA_MAX}, got {tuple(k.shape)}")
    return k.contiguous().to(device)


def metric_sums(wh, anchors, thr=4.0, slices=None):
    """[G, 3] float64 numpy: (sum best * (best > 1/thr), count best > 1/thr, count x > 1/thr) per candidate set — the raw, exact quantities"""
    if wh.shape[0] == 0:
        raise ValueError("anchor_metric: no labels")
    return ops.anchor_metric(wh, _sets(anchors, wh.device), thr, slices).cpu().numpy()


def anchor_metric(wh, anchors, thr=4.0, slices=None):
    """(bpr, aat, fitness) of one anchor set [na, 2], or arrays of them for sets [G, na, 2]: check_anchors' `metric` and kmean_anchors'
    `anchor_fitness`, as exact sums over n"""
    s, n = metric_sums(wh, anchors, thr, slices), wh.shape[0]
    bpr, aat, fit = s[:, 1] / n, s[:, 2] / n, s[:, 0] / n
    single = (anchors.dim() if isinstance(anchors, torch.Tensor) else np.ndim(anchors)) == 2
    return (float(bpr[0]), float(aat[0]), float(fit[0])) if single else (bpr, aat, fit)


def mutation_table(gen, shape, seed=0, rs=None, py=None):
    """[gen, na, 2] float64: the factors `v` of kmean_anchors' loop (autoanchor.py:158-161) for every generation, in the reference's call
    order — npr.random, random.random, npr.randn per attempt, redrawn while all ones, clipped to [0.3, 3.0].  rs / py: a numpy RandomState
    and a random.Random to continue from (default: fresh ones seeded with `seed`)."""
    rs = np.random.RandomState(seed) if rs is None else rs
    py = random.Random(seed) if py is None else py
    out = np.empty((gen,) + tuple(shape), dtype=np.float64)
    for g in range(gen):
        v = np.ones(shape)
        while (v == 1).all():
            v = ((rs.random_sample(shape) < MUTATION_PROB) * py.random() * rs.randn(*shape) * MUTATION_SIGMA + 1).clip(0.3, 3.0)
        out[g] = v
    return out


def evolve(wh, k, thr=4.0, gen=1000, seed=0, batch=32, table=None, slices=None):
    """kmean_anchors' mutation loop from anchors k [na, 2] over wh (float32 [n, 2] on the device): generation g tries
    kg = max(k * v[g], 2.0) and keeps it when its fitness is larger — the reference's serial chain, `batch` speculative generations per
    round.  -> Evolved"""
    k = np.ascontiguousarray(np.asarray(k, dtype=np.float64).reshape(-1, 2))
    na, n, dev = k.shape[0], wh.shape[0], wh.device
    if not 1 <= batch <= 256:
        raise ValueError(f"evolve: batch={batch} outside [1, 256]")
    f = ops.anchor_metric(wh, _sets(k, dev), thr, slices)[0, :1].clone()               # anchor_fitness(k): the float32 image of k
    if gen <= 0:
        return Evolved(k.copy(), float(f.item()), n, 0, 0)
    v = mutation_table(gen, (na, 2), seed) if table is None else np.ascontiguousarray(table, dtype=np.float64)
    if v.shape != (gen, na, 2):
        raise ValueError(f"evolve: the mutation table is {v.shape}, need {(gen, na, 2)}")
    v_dev, k_dev = torch.from_numpy(v).to(dev), torch.from_numpy(k).to(dev)
    cursor = torch.zeros(2, dtype=torch.int32, device=dev)
    part = torch.empty((ops.anchor_slices(n, slices), batch), dtype=torch.float64, device=dev)
    rounds = 0
    while True:
        ops.anchor_evolve_round(wh, v_dev, k_dev, f, cursor, batch, thr, part)
        rounds += 1
        if int(cursor[0].item()) >= gen:                                                # the 4 bytes the host reads per round
            break
    return Evolved(k_dev.cpu().numpy(), float(f.item()), n, int(cursor[1].item()), rounds)


def kmeans_step(pts, cent, slices=None, thresh=KMEANS_THRESH, prev=None, want_assign=True):
    """ONE Lloyd iteration of the R runs cent [R, na, 2] over the whitened points pts [n, 2] (both float32, on the device): -> dict of
    assign [R, n], count [R, na], cent (new), dist [R], flags [R] (device tensors).  The inspection form of what `lloyd` loops over."""
    n, (r, na, _), dev = pts.shape[0], cent.shape, pts.device
    cent = cent.contiguous().clone()
    part = torch.empty((ops.anchor_slices(n, slices), r, 3 * na + 1), dtype=torch.float64, device=dev)
    flags, iters, active = (torch.zeros(m, dtype=torch.int32, device=dev) for m in (r, r, 1))
    dist = torch.full((r,), float("inf"), dtype=torch.float64, device=dev) if prev is None else prev.to(dev, torch.float64).clone()
    count = torch.zeros((r, na), dtype=torch.int32, device=dev)
    assign = torch.empty((r, n), dtype=torch.int32, device=dev) if want_assign else None
    ops.kmeans_assign(pts, cent, flags, part, assign)
    ops.kmeans_update(part, n, thresh, cent, dist, count, flags, iters, active)
    return dict(assign=assign, count=count, cent=cent, dist=dist, flags=flags)


def lloyd(pts, init, thresh=KMEANS_THRESH, max_iter=KMEANS_MAX_ITER, slices=None):
    """scipy's `_kmeans` for R runs at once from the centroids init [R, na, 2]: iterate until every run is closed or max_iter iterations;
    the best run has the lowest distortion among those not discarded (the lowest run on equality).  -> KMeans (k, s left None)"""
    n, (r, na, _), dev = pts.shape[0], init.shape, pts.device
    cent = init.to(dev, torch.float32).contiguous().clone()
    part = torch.empty((ops.anchor_slices(n, slices), r, 3 * na + 1), dtype=torch.float64, device=dev)
    flags, iters, active = (torch.zeros(m, dtype=torch.int32, device=dev) for m in (r, r, 1))
    dist = torch.full((r,), float("inf"), dtype=torch.float64, device=dev)
    count = torch.zeros((r, na), dtype=torch.int32, device=dev)
    it = 0
    while it < max_iter:
        ops.kmeans_assign(pts, cent, flags, part)
        ops.kmeans_update(part, n, thresh, cent, dist, count, flags, iters, active)
        it += 1
        if int(active.item()) == 0:                                                     # the 4 bytes the host reads per iteration
            break
    fl, d = flags.cpu().numpy(), dist.cpu().numpy()
    ok = np.flatnonzero((fl & 2) == 0)
    run = int(ok[np.argmin(d[ok])]) if len(ok) else -1                                  # argmin: the first of equal minima
    return KMeans(k=None, s=None, run=run, iters=it, run_iters=iters.cpu().numpy(), dist=d, flags=fl, cent=cent.cpu().numpy())


def kmeans_init(n_points, n, runs=30, seed=0):
    """[runs, n] indices: n distinct points per run from numpy's Generator seeded with `seed`"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(n_points, n, replace=False) for _ in range(runs)]).astype(np.int64)


def kmeans(wh, n, runs=30, seed=0, slices=None):
    """`kmeans(wh / s, n, iter=30)[0] * s` of autoanchor.py:139-140 over wh (float32 [m, 2] on the device, already filtered).  -> KMeans;
    .k is None when m < n or every run was discarded (the caller takes the reference's random fallback)"""
    m = wh.shape[0]
    if m < n or n < 1:
        return KMeans(k=None, s=None, run=-1, iters=0, run_iters=np.zeros(runs, np.int32), dist=None, flags=None, cent=None)
    if n > ops.ANCHOR_NA_MAX:
        raise ValueError(f"kmeans: n={n} anchors, at most {ops.ANCHOR_NA_MAX}")
    s = wh.double().std(0, unbiased=False).float()                                      # sigmas for whitening
    pts = (wh / s).contiguous()
    idx = torch.from_numpy(kmeans_init(m, n, runs, seed)).to(wh.device)
    res = lloyd(pts, pts[idx], slices=slices)
    res.s = s.cpu().numpy()
    if res.run >= 0:
        res.k = res.cent[res.run] * res.s                                               # float32 * float32, as `kmeans(...)[0] * s`
    return res


def _by_area(k):
    return k[np.argsort(k.prod(1))]                                                     # print_results: sort small to large


def kmean_anchors(data, n=9, img_size=640, thr=4.0, gen=1000, seed=0, batch=32, info=None):
    """autoanchor.py:69-169 `kmean_anchors(dataset, n, img_size, thr, gen)`: k-means on the label sizes, then `gen` generations of mutation.
    -> float32 [n, 2] in pixels, sorted by area.  data: an ImageBank, a dataset with .labels / .shapes, or a (labels, shapes) pair.
    info: a dict that receives the counts of the run (k-means iterations, evolve rounds, acceptances, fallback)."""
    labels, shapes = _source(data)
    rs, py = np.random.RandomState(seed), random.Random(seed)
    wh0 = label_wh(labels, shapes, img_size)
    small = int((wh0 < 3.0).any(1).sum())
    if small:
        LOGGER.info("autoanchor: %d of %d labels are < 3 pixels in size", small, wh0.shape[0])
    wh = wh0[(wh0 >= 2.0).any(1)].contiguous()                                         # filter > 2 pixels
    if wh.shape[0] == 0:
        raise ValueError("kmean_anchors: no label is 2 pixels or larger")
    km = kmeans(wh, n, seed=seed)
    if km.k is None:
        LOGGER.warning("autoanchor: switching strategies from kmeans to random init")
        k = np.sort(rs.rand(n * 2)).reshape(n, 2) * img_size
    else:
        k = km.k.astype(np.float64)
    k = _by_area(k)
    ev = evolve(wh, k, thr, gen, batch=batch, table=mutation_table(gen, (n, 2), rs=rs, py=py) if gen > 0 else None)
    k = _by_area(ev.k).astype(np.float32)
    LOGGER.info("autoanchor: %d labels, k-means %d iterations (run %d), evolution %d generations in %d rounds, %d accepted, fitness %.4f",
                wh.shape[0], km.iters, km.run, gen, ev.rounds, ev.accepted, ev.f)
    if info is not None:
        info.update(labels=int(wh.shape[0]), kmeans_iters=km.iters, kmeans_run=km.run, fallback=km.k is None, rounds=ev.rounds,
                    accepted=ev.accepted, fitness=ev.f, launches=2 * km.iters + 2 * ev.rounds + 3)
    return k


def check_anchors(data, model, thr=4.0, imgsz=640, seed=0, info=None):
    """autoanchor.py:30-66 `check_anchors(dataset, model, thr, imgsz)`: best possible recall of the model's anchors over the labels
    (augment scale uniform(0.9, 1.1) per image from RandomState(seed)); at bpr <= 0.98 kmean_anchors evolves new ones, and if their bpr is
    larger they are written into `m.anchors` in place (pixel space, check_anchor_order, then / stride).  -> AnchorCheck.
    Call it before the model is captured by a GraphedTrainStep (train.py calls it before the first epoch).  info: see kmean_anchors."""
    det = model.module.model[-1] if hasattr(model, "module") else model.model[-1]
    labels, shapes = _source(data)
    shapes = np.asarray(shapes).reshape(-1, 2)
    scale = np.random.RandomState(seed).uniform(0.9, 1.1, size=(shapes.shape[0], 1))   # augment scale
    wh = label_wh(labels, shapes, imgsz, scale=scale)
    stride = det.stride.to(det.anchors.device).view(-1, 1, 1)
    anchors = (det.anchors.clone() * stride).float().cpu().view(-1, 2).numpy()          # current anchors
    sums = metric_sums(wh, anchors, thr)[0]
    n = wh.shape[0]
    bpr, aat = sums[1] / n, sums[2] / n
    if bpr > 0.98:                                                                      # threshold to recompute
        LOGGER.info("autoanchor: %.2f anchors/target, %.3f best possible recall: the current anchors are a good fit", aat, bpr)
        return AnchorCheck(bpr, aat, None, anchors, False)
    LOGGER.info("autoanchor: %.2f anchors/target, %.3f best possible recall: a poor fit, attempting to improve", aat, bpr)
    new = kmean_anchors((labels, shapes), n=det.anchors.numel() // 2, img_size=imgsz, thr=thr, gen=1000, seed=seed, info=info)
    new_sums = metric_sums(wh, new, thr)[0]
    new_bpr = new_sums[1] / n
    if not new_sums[1] > sums[1]:                                                       # counts over the same n: new_bpr > bpr, exactly
        LOGGER.info("autoanchor: the original anchors are better than the new ones (%.3f), keeping them", new_bpr)
        return AnchorCheck(bpr, aat, new_bpr, anchors, False)
    with torch.no_grad():
        det.anchors[:] = torch.tensor(new, device=det.anchors.device).type_as(det.anchors).view_as(det.anchors)
        check_anchor_order(det)                                                         # must be in pixel-space (not grid-space)
        det.anchors /= stride
    LOGGER.info("autoanchor: anchors replaced, best possible recall %.3f (update the model yaml to keep them)", new_bpr)
    return AnchorCheck(bpr, aat, new_bpr, new, True)
