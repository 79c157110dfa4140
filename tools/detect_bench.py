"""The detect pipeline at bs = 32 onto 640 x 640 (lead-yolo-s, bf16 autocast, graphed forward), for sources of 1080 x 1920 and of 480 x 640 that
are resident on the device (a decoder's output), on one GPU.  Per workload:

  letterbox_us         ly_letterbox_u8 alone (table already uploaded): median of --reps HIP-event timings after warm-up; `moved_mb` = output bytes
                       + the source bytes its taps reference (distinct rows x distinct columns x 3 per image: the convention of the mosaic row),
                       and that as a share of 8 TB/s
  h2d_ms / h2d_copy_us the same sources starting on the HOST: packing into the pinned block + the one copy, host clock to a synchronise (ms), and
                       the copy of that block alone by HIP events (us)
  detector_ms          Detector.padded per batch end to end (letterbox -> graphed forward -> nms_padded -> ly_scale_boxes), host clock to a synchronise
  baseline_ms          the same graphed forward + nms_padded fed the way a user of the package writes it without predict.py: per image
                       F.interpolate(bilinear, antialias=False) on float + F.pad(114) + channel flip, stacked and cast into the graph's input,
                       then scale_boxes / clip_boxes with torch ops per image
  pre_*_us             the preprocessing alone of either leg (letterbox() with its table upload / the per-image loop), HIP events
Rounds of the two legs alternate in one process; medians.  The weights are random with the heads' biases lifted (as tools/val_bench.py).
Writes one JSON line to --out (default profiles/detect_bench.json) and prints it.

    python tools/detect_bench.py [--bs 32] [--size 640] [--rounds 5] [--steps 10] [--reps 30] [--out profiles/detect_bench.json]"""
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
from lead_yolo_amd import predict as P  # noqa: E402

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


def _sources(n, h, w, seed):
    """n different images of h x w: blocks of 8 x 8 pixels of one colour plus noise (content does not change the timing; this keeps it cheap)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        base = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
        out.append(np.ascontiguousarray(np.kron(base, np.ones((8, 8, 1), np.uint8))[:h, :w]))
    return out


def _touched(n_dst, n_src):
    """distinct source indices the taps of a resize n_src -> n_dst reference (the contract of ly_letterbox_u8)"""
    if n_dst == n_src:
        return n_src
    f = ((np.arange(n_dst) + 0.5) * (1.0 / (n_dst / n_src)) - 0.5).astype(np.float32)
    s = np.clip(np.floor(f).astype(np.int64), 0, n_src - 1)
    return len(np.unique(np.concatenate([s, np.minimum(s + 1, n_src - 1)])))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detect_bench: no GPU (a timing needs the device; there is no CPU fallback)")
    if a.reps < 20:
        raise SystemExit("detect_bench: --reps must be at least 20")
    dev = torch.device("cuda:0")
    bs, S = a.bs, a.size
    nms = dict(conf_thres=0.25, iou_thres=0.45, max_det=300)
    m = _model(dev)
    med = lambda v: float(np.median(v))          # noqa: E731
    out = dict(metric="detect_pipeline", model="lead-yolo-s", dtype="bf16", bs=bs, size=S, rounds=a.rounds, steps_per_round=a.steps, reps=a.reps, **nms,
               baseline="per-image F.interpolate(bilinear) + F.pad(114) + flip + stack, graphed forward, nms_padded, torch scale_boxes per image")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        det = L.Detector(m, img_size=S, batch_size=bs, **nms)
        g = det._g                                   # both legs replay the same captured forward
        for h0, w0 in ((1080, 1920), (480, 640)):
            host = _sources(bs, h0, w0, h0)
            imgs = [torch.from_numpy(im).to(dev) for im in host]
            # ---- ly_letterbox_u8 alone
            src, keep = P._sources(imgs, dev, "detect_bench")
            plan = L.letterbox_plan([(h0, w0)] * bs, S, stride=det.stride)
            batch = torch.empty((bs, 3, S, S), dtype=torch.uint8, device=dev)
            table = (capi.LyLetterboxImage * bs)()
            for i, (p, _, _) in enumerate(src):
                table[i] = capi.LyLetterboxImage(p, batch.data_ptr() + i * 3 * S * S, h0, w0, S, S, int(plan.nh[i]), int(plan.nw[i]), int(plan.top[i]),
                                                 int(plan.left[i]))
            table_dev, _ = P._upload(table, np.zeros(0, np.float32), dev)
            lb_us = _events(lambda: P._launch(table_dev, bs, S, S, P.LB_CHW_RGB), a.reps)
            moved = batch.numel() + sum(3 * _touched(int(plan.nh[i]), h0) * _touched(int(plan.nw[i]), w0) for i in range(bs))
            # ---- the sources starting on the host
            h2d_ms = med([_wall(lambda: P._sources(host, dev, "detect_bench"), 3) for _ in range(a.rounds)])
            pinned = torch.empty(bs * h0 * w0 * 3, dtype=torch.uint8, pin_memory=True)
            staged = torch.empty_like(pinned, device=dev)
            h2d_copy_us = _events(lambda: staged.copy_(pinned, non_blocking=True), a.reps)
            del pinned, staged

            # ---- the two legs
            def pre_new():
                return L.letterbox(imgs, S, stride=det.stride, out=g.x)

            def pre_base():
                xs = []
                for i, im in enumerate(imgs):
                    nh, nw, top, left = (int(getattr(plan, k)[i]) for k in ("nh", "nw", "top", "left"))
                    x = im.permute(2, 0, 1)[None].float()
                    if (nh, nw) != (h0, w0):
                        x = F.interpolate(x, size=(nh, nw), mode="bilinear", align_corners=False, antialias=False)
                    x = F.pad(x, (left, S - nw - left, top, S - nh - top), value=114.0)
                    xs.append(x.flip(1))
                g.x.copy_(torch.cat(xs).round_().clamp_(0, 255))

            def leg_new():
                return det.padded(imgs)

            def leg_base():
                pre_base()
                dets, counts, _ = L.nms_padded(g()[0], **nms)
                for i in range(bs):                                        # scale_boxes + clip_boxes + round, per image, as detect.py does
                    gain = min(S / h0, S / w0)
                    b = dets[i, :, :4]
                    b[:, [0, 2]] -= (S - w0 * gain) / 2
                    b[:, [1, 3]] -= (S - h0 * gain) / 2
                    b /= gain
                    b[:, [0, 2]] = b[:, [0, 2]].clamp(0, w0)
                    b[:, [1, 3]] = b[:, [1, 3]].clamp(0, h0)
                    dets[i, :, :4] = b.round()
                return dets, counts

            for fn in (leg_new, leg_base):
                fn()
            pre_base()
            base_batch = g.x.clone()
            pre_new()
            differ = (g.x.int() - base_batch.int()).abs()
            counts = leg_new()[1]
            t_new, t_base = [], []
            for _ in range(a.rounds):
                t_new.append(_wall(leg_new, a.steps))
                t_base.append(_wall(leg_base, a.steps))
            pre_new_us, pre_base_us = _events(pre_new, a.reps), _events(pre_base, a.reps)
            fwd_nms_ms = med([_wall(lambda: L.nms_padded(g()[0], **nms), a.steps) for _ in range(a.rounds)])
            out[f"src_{h0}x{w0}"] = dict(
                letterbox_us=round(lb_us, 2), moved_mb=round(moved / 1e6, 2), hbm_share=round(moved / lb_us / HBM_BYTES_PER_US, 4),
                h2d_ms=round(h2d_ms, 3), h2d_copy_us=round(h2d_copy_us, 1), source_mb=round(bs * h0 * w0 * 3 / 1e6, 2),
                detector_ms=round(med(t_new), 3), baseline_ms=round(med(t_base), 3), baseline_over_detector=round(med(t_base) / med(t_new), 2),
                pre_detector_us=round(pre_new_us, 1), pre_baseline_us=round(pre_base_us, 1), forward_nms_ms=round(fwd_nms_ms, 3),
                detections_per_image=round(float(counts.float().mean()), 1), batch_max_abs_diff_vs_baseline=int(differ.max()),
                detector_all=[round(t, 3) for t in t_new], baseline_all=[round(t, 3) for t in t_base])
            del imgs, keep, table_dev
            torch.cuda.empty_cache()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
