"""Whole-scene detection (lead-yolo_amd/scene.py SceneDetector, csrc/ly_scene.hip) on one synthetic scene resident on the device — by default
8192 x 8192 x 3, tile 640, overlap 128, 32 tiles per batch: 256 tiles in 8 chunks — lead-yolo-s, bf16 autocast, graphed forward, one GPU.

  tiles_us             ly_scene_tiles_u8 alone for one full chunk (origins already on the device): median of --reps HIP-event timings after
                       warm-up; `tiles_moved_mb` = the chunk's output bytes + the source bytes of its windows, and that as a share of 8 TB/s.
                       tiles_unaligned_us: the same windows shifted by one pixel, so that no source row is 16-byte aligned
  collect_us / sort_us / nms_us   ly_scene_collect, the torch.sort and ly_scene_nms alone at the candidates the run produced (`candidates`
                       live rows of `rows`; `kept` leave the merge), HIP events.  sparse_*: sort and ly_scene_nms again with at most --sparse
                       live rows per tile (a detector that finds a few ships per tile; the random network fills every tile's 300 rows)
  forward_nms_ms       the graphed forward + nms_padded of all chunks on a batch that is already in place: what ly_scene_nms is held against
  scene_ms             SceneDetector.padded per scene end to end, host clock to a synchronise
  baseline_ms          the same graphed forward + nms_padded fed and merged the way a user of the package writes it without scene.py: per tile
                       slice + F.pad(114) + flip + permute, stacked into the graph's input; the boxes shifted, clipped and sorted with torch
                       ops and the greedy rule restated as a pair mask over the live candidates iterated to its fixed point on the device
Rounds of the two legs alternate in one process; medians.  The weights are random with the heads' biases lifted (as tools/val_bench.py), so
the candidate counts are the random network's, not a trained detector's.  Writes one JSON line to --out (default profiles/scene_bench.json)
and prints it.

    python tools/scene_bench.py [--side 8192] [--tile 640] [--overlap 128] [--bs 32] [--rounds 5] [--steps 3] [--reps 30] [--sparse 8] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lead_yolo_amd as L  # noqa: E402
from lead_yolo_amd import capi  # noqa: E402
from lead_yolo_amd import scene as S  # noqa: E402

HBM_BYTES_PER_US = 8e6            # 8 TB/s


def _model(dev):
    from oracle import synth
    torch.manual_seed(0)
    m = L.Model(L.load_cfg(scale="s"))
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 4242)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    for i in range(len(m.model[-1].m)):
        st[f"model.23.m.{i}.bias"] = st[f"model.23.m.{i}.bias"] + 2.0
    m.load_state_dict(st)
    return m.to(dev).eval()


def _scene(side, dev):
    """blocks of 8 x 8 pixels of one colour plus noise, built on the device (content does not change the timing of the copies)"""
    g = torch.Generator(device=dev).manual_seed(5)
    base = torch.randint(0, 200, (side // 8 + 1, side // 8 + 1, 3), dtype=torch.uint8, device=dev, generator=g)
    big = base.repeat_interleave(8, 0).repeat_interleave(8, 1)[:side, :side]
    return (big + torch.randint(0, 56, (side, side, 3), dtype=torch.uint8, device=dev, generator=g)).contiguous()


def _events(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


def _wall(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def _torch_merge(dets, counts, origins, H, W, mdt, metric, thres, agnostic, max_det, max_merge):
    """the merge with torch ops: shift, clip, stable sort, then the greedy rule as its fixed point — S[i, j] = (i before j, other tile, same
    class, m > thres); keep[j] = no kept i with S[i, j], iterated from all-kept until nothing changes (entry j is final after j rounds; the
    rounds needed are the longest suppression chain)"""
    n = dets.shape[0]
    off = origins.flip(1).float().repeat(1, 2)[:, None]                     # (x0, y0, x0, y0)
    lim = torch.tensor([W, H, W, H], dtype=torch.float32, device=dets.device)
    boxes = dets.clone()
    boxes[..., :4] = torch.minimum((dets[..., :4] + off).clamp_min(0), lim)
    live = torch.arange(mdt, device=dets.device)[None] < counts[:, None]
    boxes = (boxes * live[..., None]).reshape(n * mdt, 6)
    score = torch.where(live, dets[..., 4], torch.full_like(dets[..., 4], -1)).reshape(-1)
    svals, order = torch.sort(score, descending=True, stable=True)
    k = min(int((svals >= 0).sum()), max_merge)                             # the user's code knows no better than to ask
    order = order[:k]
    b, tile = boxes[order], order // mdt
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    sup = torch.empty((k, k), dtype=torch.bool, device=dets.device)
    for lo in range(0, k, 4096):
        a = b[lo:lo + 4096]
        iw = (torch.minimum(a[:, None, 2], b[None, :, 2]) - torch.maximum(a[:, None, 0], b[None, :, 0])).clamp_min(0)
        ih = (torch.minimum(a[:, None, 3], b[None, :, 3]) - torch.maximum(a[:, None, 1], b[None, :, 1])).clamp_min(0)
        inter = iw * ih
        aa = area[lo:lo + 4096, None]
        den = (aa + area[None]) - inter if metric == "iou" else torch.minimum(aa, area[None])
        m = torch.where(den == 0, torch.zeros_like(den), inter / den)
        ok = (m > thres) & (tile[lo:lo + 4096, None] != tile[None])
        if not agnostic:
            ok &= a[:, None, 5] == b[None, :, 5]
        sup[lo:lo + 4096] = ok
    sup.triu_(1)
    keep = torch.ones(k, dtype=torch.bool, device=dets.device)
    rounds = 0
    while True:
        new = ~(sup & keep[:, None]).any(0)
        rounds += 1
        if torch.equal(new, keep):
            break
        keep = new
    return b[keep][:max_det], order[keep][:max_det], rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=8192)
    ap.add_argument("--tile", type=int, default=640)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sparse", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_bench: no GPU (a timing needs the device; there is no CPU fallback)")
    if a.reps < 20:
        raise SystemExit("scene_bench: --reps must be at least 20")
    dev = torch.device("cuda:0")
    side, T, bs = a.side, a.tile, a.bs
    kw = dict(conf_thres=0.25, iou_thres=0.45, max_det_tile=300, metric="ios", merge_thres=0.5, max_det=3000)
    nms = dict(conf_thres=kw["conf_thres"], iou_thres=kw["iou_thres"], max_det=kw["max_det_tile"])
    m = _model(dev)
    med = lambda v: float(np.median(v))          # noqa: E731
    scene = _scene(side, dev)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        sd = L.SceneDetector(m, tile=T, overlap=a.overlap, batch_size=bs, **kw)
        g = sd._g                                    # both legs replay the same captured forward
        origins, (ny, nx) = L.scene_plan(side, side, T, a.overlap)
        n = len(origins)
        chunks = -(-n // bs)
        # ---- ly_scene_tiles_u8 alone: the first full chunk, and the same windows one pixel to the right
        k = min(bs, n)
        org = S._to_device(origins[:k], dev)
        shifted = origins[:k].copy()
        shifted[:, 1] = np.minimum(shifted[:, 1] + 1, side - T)
        org1 = S._to_device(shifted, dev)
        tiles_us = _events(lambda: S._launch_tiles(scene, side, side, 3, side * 3, org, k, T, sd._u8), a.reps)
        tiles1_us = _events(lambda: S._launch_tiles(scene, side, side, 3, side * 3, org1, k, T, sd._u8), a.reps)
        moved = 2 * k * 3 * T * T
        # ---- the merge's launches alone, at the candidates the run produced
        dets, counts, origins_dev = sd.tiles_padded(scene)
        boxes, score = L.scene_collect(dets, counts, origins_dev, side, side)
        svals, order = torch.sort(score, descending=True, stable=True)
        keep = torch.empty((kw["max_det"],), dtype=torch.int32, device=dev)
        count = torch.empty((1,), dtype=torch.int32, device=dev)
        lib, p = capi.lib(), capi.ptr

        def run_nms():
            capi.check(lib.ly_scene_nms(p(boxes), p(order), p(svals), boxes.shape[0], kw["max_det_tile"], S.METRICS[kw["metric"]], kw["merge_thres"], 0,
                                        kw["max_det"], S.MAX_NMS, p(keep), p(count), capi.stream_ptr()), "ly_scene_nms")

        collect_us = _events(lambda: L.scene_collect(dets, counts, origins_dev, side, side), a.reps)
        sort_us = _events(lambda: torch.sort(score, descending=True, stable=True), a.reps)
        nms_us = _events(run_nms, a.reps)
        candidates, kept = int(counts.sum()), int(count)
        # the same launches with at most --sparse live rows per tile: what a detector that finds a few ships per tile hands the merge
        counts_s = counts.clamp(max=a.sparse)
        boxes, score = L.scene_collect(dets, counts_s, origins_dev, side, side)
        svals, order = torch.sort(score, descending=True, stable=True)
        sparse_sort_us = _events(lambda: torch.sort(score, descending=True, stable=True), a.reps)
        sparse_nms_us = _events(run_nms, a.reps)
        sparse_candidates, sparse_kept = int(counts_s.sum()), int(count)

        # ---- the two legs
        def forward_nms():
            for _ in range(chunks):
                L.nms_padded(g()[0], **nms)

        def leg_new():
            return sd.padded(scene)

        def leg_base():
            ds, cs = [], []
            for lo in range(0, n, bs):
                xs = []
                for y0, x0 in origins[lo:lo + bs].tolist():
                    w = scene[y0:y0 + T, x0:x0 + T]
                    if w.shape[0] < T or w.shape[1] < T:
                        w = F.pad(w.permute(2, 0, 1), (0, T - w.shape[1], 0, T - w.shape[0]), value=114).permute(1, 2, 0)
                    xs.append(w.flip(2).permute(2, 0, 1))
                kk = len(xs)
                g.x[:kk].copy_(torch.stack(xs))
                if kk < bs:
                    g.x[kk:].fill_(114)
                d, c, _ = L.nms_padded(g()[0], **nms)
                ds.append(d[:kk])
                cs.append(c[:kk])
            return _torch_merge(torch.cat(ds), torch.cat(cs), origins_dev, side, side, kw["max_det_tile"], kw["metric"], kw["merge_thres"], False,
                                kw["max_det"], S.MAX_NMS)

        if not sd.u8:
            raise SystemExit("scene_bench: the baseline writes uint8 tiles into the graph's input; the model does not take uint8")
        new_d, new_n = leg_new()
        base_b, base_rows, base_rounds = leg_base()
        same = bool(int(new_n) == len(base_b) and torch.equal(new_d[:int(new_n)], base_b))
        t_new, t_base = [], []
        for _ in range(a.rounds):
            t_new.append(_wall(leg_new, a.steps))
            t_base.append(_wall(leg_base, a.steps))
        fwd_nms_ms = med([_wall(forward_nms, a.steps) for _ in range(a.rounds)])
    out = dict(metric="scene_pipeline", model="lead-yolo-s", dtype="bf16", scene=[side, side, 3], tile=T, overlap=a.overlap, bs=bs, tiles=n,
               plan=[ny, nx], chunks=chunks, rounds=a.rounds, steps_per_round=a.steps, reps=a.reps,
               **{("merge_metric" if key == "metric" else key): v for key, v in kw.items()},
               baseline="per tile slice + F.pad(114) + flip + permute, stacked; graphed forward, nms_padded; torch shift / clip / sort and the "
                        "greedy rule as a pair mask iterated to its fixed point",
               tiles_us=round(tiles_us, 2), tiles_unaligned_us=round(tiles1_us, 2), tiles_per_launch=k, tiles_moved_mb=round(moved / 1e6, 2),
               tiles_hbm_share=round(moved / tiles_us / HBM_BYTES_PER_US, 4), tiles_unaligned_hbm_share=round(moved / tiles1_us / HBM_BYTES_PER_US, 4),
               rows=int(boxes.shape[0]), candidates=candidates, kept=kept, nms_form="one block (ly_nms_greedy's structure)",
               collect_us=round(collect_us, 2), sort_us=round(sort_us, 2), nms_us=round(nms_us, 1), forward_nms_ms=round(fwd_nms_ms, 3),
               sparse_rows_per_tile=a.sparse, sparse_candidates=sparse_candidates, sparse_kept=sparse_kept, sparse_sort_us=round(sparse_sort_us, 2),
               sparse_nms_us=round(sparse_nms_us, 1), nms_over_forward_nms=round(nms_us / 1e3 / fwd_nms_ms, 3), scene_ms=round(med(t_new), 3), baseline_ms=round(med(t_base), 3),
               baseline_over_scene=round(med(t_base) / med(t_new), 2), baseline_equal=same, baseline_fixed_point_rounds=base_rounds,
               scene_all=[round(t, 3) for t in t_new], baseline_all=[round(t, 3) for t in t_base])
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
