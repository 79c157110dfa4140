"""One validation pass through `validate`, rectangular batches against square ones: lead-yolo-s, bf16 (autocast), 256 synthetic images, batch 32,
img_size 640, for 1080 x 1920 (16:9) and 480 x 640 (4:3) sources, on one GPU.

Both legs are `validate(model, ValSet(...), compute_loss=ComputeLoss(model))` with val.py's settings (conf_thres 0.001, iou_thres 0.6, the
confusion matrix on, graphed forward) and differ in the ValSet only:
  rect     ValSet(rect=True): the reference's validation loader — 16:9 sources on 384 x 672 canvases, 4:3 on 512 x 672
  square   ValSet(rect=False): every image on a 640 x 640 canvas, what tests/test_val_pipeline.py and tools/val_bench.py validate on
ms per pass from a host clock around a call that ends in its own device synchronisation, medians of alternating rounds in one process after
a warm-up pass of each leg (which captures the graphs); `speed` is validate's own (pre, inference, nms) ms per image from HIP events, the
median over the rounds.  ly_val_confusion alone is timed with HIP events on one batch of the rect leg.  The random weights get the +2.0
head-bias lift of the tests so that NMS keeps max_det = 300 boxes per image, as it does at conf_thres 0.001 on a trained model.  Prints one
JSON line and writes it to --out.

  python tools/valrun_bench.py [--images 256] [--bs 32] [--size 640] [--rounds 5] [--out profiles/valrun_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lead_yolo_amd as L  # noqa: E402


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


def _dataset(n, h0, w0, seed, per_image=5):
    """n images of one size (eight distinct random pictures, repeated) and per_image random labels each"""
    rng = np.random.default_rng(seed)
    distinct = [rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8) for _ in range(8)]
    labels = [np.concatenate([np.zeros((per_image, 1)), rng.uniform(0.1, 0.9, (per_image, 2)), rng.uniform(0.02, 0.2, (per_image, 2))], 1)
              .astype(np.float32) for _ in range(n)]
    return [distinct[i % 8] for i in range(n)], labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "valrun_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("valrun_bench: no GPU (a timing needs the device; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    m = _model(dev)
    loss_fn = L.ComputeLoss(m)
    med = lambda v: float(np.median(v))          # noqa: E731
    out = dict(metric="validation_pass", model="lead-yolo-s", dtype="bf16", images=a.images, bs=a.bs, img_size=a.size, conf_thres=0.001,
               iou_thres=0.6, max_det=300, rounds=a.rounds, baseline="ValSet(rect=False): square img_size canvases")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for name, (h0, w0) in (("1080x1920", (1080, 1920)), ("480x640", (480, 640))):
            images, labels = _dataset(a.images, h0, w0, 7)
            t0 = time.perf_counter()
            legs = dict(rect=L.ValSet(images, labels, a.size, a.bs, rect=True, device=dev), square=L.ValSet(images, labels, a.size, a.bs, rect=False, device=dev))
            torch.cuda.synchronize()
            build_ms = (time.perf_counter() - t0) * 1e3
            del images
            times, speeds, last = {k: [] for k in legs}, {k: [] for k in legs}, {}
            for k, vs in legs.items():                         # warm-up: captures the graphs, fills the allocator pools
                L.validate(m, vs, compute_loss=loss_fn)
            for _ in range(a.rounds):
                for k, vs in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[k] = L.validate(m, vs, compute_loss=loss_fn)
                    times[k].append((time.perf_counter() - t0) * 1e3)
                    speeds[k].append(last[k].speed)
            res = dict(valset_build_both_ms=round(build_ms, 1))
            for k, vs in legs.items():
                H, W = vs.canvas[0]
                sp = np.median(np.array(speeds[k]), 0)
                res[k] = dict(canvas=[H, W], canvases=len(set(vs.canvas)), resident_mb=round(vs.nbytes() / 2 ** 20, 1), pass_ms=round(med(times[k]), 2),
                              ms_per_image=round(med(times[k]) / a.images, 4), pre_ms_per_image=round(float(sp[0]), 4),
                              inference_ms_per_image=round(float(sp[1]), 4), nms_ms_per_image=round(float(sp[2]), 4),
                              map50=round(last[k].metrics.map50, 4), loss=[round(float(v), 5) for v in last[k].loss],
                              detections_per_image=round(len(last[k].stats[0]) / a.images, 1), pass_all=[round(t, 2) for t in times[k]])
            r, s = res["rect"], res["square"]
            res["pixel_ratio"] = round(r["canvas"][0] * r["canvas"][1] / (s["canvas"][0] * s["canvas"][1]), 3)
            res["rect_over_square"] = round(r["pass_ms"] / s["pass_ms"], 3)
            # ly_val_confusion alone on one batch of the rect leg
            vs = legs["rect"]
            with torch.no_grad():
                z = m(vs.x[0] if m.u8_input else vs.x[0].to(next(m.parameters()).dtype) / 255)[0]
                dets, counts, _ = L.nms_padded(z, 0.001, 0.6)
            cm = L.ConfusionMatrix(1)
            W_H = (vs.canvas[0][1], vs.canvas[0][0])
            cm.update((dets, counts), vs.targets[0], W_H, shapes=vs.val_shapes[0])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                cm.update((dets, counts), vs.targets[0], W_H, shapes=vs.val_shapes[0])
            e1.record()
            torch.cuda.synchronize()
            res["val_confusion_us"] = round(e0.elapsed_time(e1) * 1e3 / 50, 2)
            res["kept_above_0.25_per_image"] = round(float((dets[..., 4] > 0.25).sum()) / a.bs, 1)
            out[name] = res
            del legs, vs, last
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
