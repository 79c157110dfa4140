"""Autoanchor, device route against a host restatement of the reference: wall time of `check_anchors` over a synthetic label set of
SAR-ship size (about 40 k square chips, about 60 k small and narrow boxes), lead-yolo-n's Detect head with the yaml's COCO anchors.

  device   lead_yolo_amd.check_anchors: ly_anchor_wh, ly_anchor_metric, batched k-means (ly_kmeans_assign / _update), evolution
           (ly_anchor_evolve_eval / _pick), from labels resident on the device (the ImageBank form) and from host label arrays (upload included)
  host     utils/autoanchor.py restated as the reference runs it: numpy label sizes, float32 torch metric on the CPU, scipy.cluster.vq.kmeans
           (iter=30), 1000 generations of mutation, one fitness per generation

ms from a host clock around the call (the device route ends in its own read-backs), medians of `--rounds` alternating rounds after one warm-up
of each leg; the anchors are put back before every call.  The two routes do not start k-means from the same points (scipy's draws are its
own), so their anchors differ; both report the best possible recall they reach.  Prints one JSON line.

  python tools/anchors_bench.py [--images 40000] [--rounds 3]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lead_yolo_amd as L  # noqa: E402


def _labels(n_img, seed):
    """per image 1 .. 4 boxes (mean about 1.5), long side 6 .. 60 px of a 256 px chip shown at 640, aspect 0.2 .. 0.6"""
    rng = np.random.default_rng(seed)
    counts = rng.choice([1, 2, 3, 4], n_img, p=[0.68, 0.2, 0.08, 0.04])
    n = int(counts.sum())
    w = np.exp(rng.uniform(np.log(6.0), np.log(60.0), n)) / 640.0
    h = w * np.exp(rng.uniform(np.log(0.2), np.log(0.6), n))
    flat = np.concatenate([np.zeros((n, 1)), rng.uniform(0.1, 0.9, (n, 2)), w[:, None], h[:, None]], 1)
    return np.split(flat, np.cumsum(counts)[:-1]), np.full((n_img, 2), 256, dtype=np.int64), flat, counts


# ---- the reference, restated for the host (utils/autoanchor.py:30-66, 69-169) --------------------------------------------------------------
def _host_check_anchors(labels, shapes, anchors_px, thr=4.0, imgsz=640, gen=1000, seed=0):
    from scipy.cluster.vq import kmeans
    npr, rnd = np.random.RandomState(seed), random.Random(seed)
    sh = imgsz * shapes / shapes.max(1, keepdims=True)
    scale = npr.uniform(0.9, 1.1, size=(sh.shape[0], 1))
    wh_c = torch.tensor(np.concatenate([lb[:, 3:5] * s for s, lb in zip(sh * scale, labels)])).float()

    def metric(k):
        r = wh_c[:, None] / k[None]
        x = torch.min(r, 1 / r).min(2)[0]
        best = x.max(1)[0]
        return (best > 1 / thr).float().mean(), (x > 1 / thr).float().sum(1).mean()

    bpr, aat = metric(torch.tensor(anchors_px))
    if bpr > 0.98:
        return float(bpr), None
    n = len(anchors_px)
    wh0 = np.concatenate([lb[:, 3:5] * s for s, lb in zip(sh, labels)])
    wh = wh0[(wh0 >= 2.0).any(1)].astype(np.float32)
    s = wh.std(0)
    k = kmeans(wh / s, n, iter=30)[0] * s
    assert n == len(k)
    wh = torch.tensor(wh, dtype=torch.float32)
    ithr = 1 / thr

    def fitness(k):
        r = wh[:, None] / torch.tensor(k, dtype=torch.float32)[None]
        best = torch.min(r, 1 / r).min(2)[0].max(1)[0]
        return (best * (best > ithr).float()).mean()

    k = k[np.argsort(k.prod(1))]
    f, shp = fitness(k), k.shape
    for _ in range(gen):
        v = np.ones(shp)
        while (v == 1).all():
            v = ((npr.random(shp) < 0.9) * rnd.random() * npr.randn(*shp) * 0.1 + 1).clip(0.3, 3.0)
        kg = (k.copy() * v).clip(min=2.0)
        fg = fitness(kg)
        if fg > f:
            f, k = fg, kg.copy()
    k = k[np.argsort(k.prod(1))].astype(np.float32)
    return float(bpr), float(metric(torch.tensor(k))[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=40000)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("anchors_bench: no GPU (a timing needs the device; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    labels, shapes, flat, counts = _labels(a.images, 0)
    torch.manual_seed(0)
    model = L.Model(L.load_cfg(scale="n")).to(dev)
    det = model.model[-1]
    saved = det.anchors.clone()
    anchors_px = (saved * det.stride.to(dev).view(-1, 1, 1)).view(-1, 2).cpu().numpy()
    resident = ((torch.from_numpy(flat).to(dev), counts), shapes)
    info, res = {}, {}

    def restore():
        with torch.no_grad():
            det.anchors.copy_(saved)

    def leg_resident():
        restore()
        res["resident"] = L.check_anchors(resident, model, info=info)

    def leg_upload():
        restore()
        res["upload"] = L.check_anchors((labels, shapes), model)

    def leg_host():
        res["host"] = _host_check_anchors(labels, shapes, anchors_px)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    legs = dict(resident=leg_resident, upload=leg_upload, host=leg_host)
    for fn in legs.values():
        fn()
    t = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            t[k].append(timed(fn))
    med = lambda v: float(np.median(v))          # noqa: E731
    r = res["resident"]
    out = dict(metric="check_anchors", images=a.images, labels=int(counts.sum()), n_anchors=9, thr=4.0, imgsz=640, gen=1000, rounds=a.rounds,
               host_threads=torch.get_num_threads(),
               baseline="utils/autoanchor.py restated on the host: numpy sizes, float32 torch metric on the CPU, scipy kmeans(iter=30), 1000 serial generations",
               device_resident_ms=round(med(t["resident"]), 2), device_upload_ms=round(med(t["upload"]), 2), host_ms=round(med(t["host"]), 1),
               host_over_device=round(med(t["host"]) / med(t["resident"]), 1),
               device_all=[round(v, 2) for v in t["resident"]], upload_all=[round(v, 2) for v in t["upload"]], host_all=[round(v, 1) for v in t["host"]],
               bpr_before=round(float(r.bpr), 4), aat_before=round(float(r.aat), 3), replaced=bool(r.replaced),
               device_new_bpr=round(float(r.new_bpr), 4), host_bpr_before=round(res["host"][0], 4), host_new_bpr=round(res["host"][1], 4),
               same_anchors_both_device_legs=bool(np.array_equal(r.anchors, res["upload"].anchors)),
               kmeans_iterations=info["kmeans_iters"], kmeans_run=info["kmeans_run"], evolve_rounds=info["rounds"], accepted=info["accepted"],
               kmean_anchors_launches=info["launches"], check_anchors_launches=info["launches"] + 6,
               anchors=[[round(float(v), 2) for v in row] for row in r.anchors])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
