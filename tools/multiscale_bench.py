"""Multi-scale training at lead-yolo-s, bs = 64, base size 640, bf16 (FusedSGD + EMA as bench.py).  Within each item the alternatives are
timed in alternating rounds in one process and medians are reported.  One JSON line (profiles/multiscale_bench.json):

  kernel      ly_resize_u8 at 640 -> 320, 608, 672, 960: us per launch and GB/s over output + source bytes, against
              F.interpolate(imgs.float() / 255, ...) on the device for the same shapes
  reserved    torch.cuda.memory_reserved() after capturing 640 only and after the largest size alone (a fresh child process each: a plain
              GraphedTrainStep), and after all 21 sizes of MultiScaleTrainStep on its one pool, captured in three orders: ascending and
              largest first (child processes, MultiScaleTrainStep.capture), outwards from 640 at first use (this process, before
              anything else runs)
  capture     seconds per size: state saved and put back, warm-up steps, capture, first replay
  sizes       per size 320 ... 960: the replayed resized step, and a plain GraphedTrainStep on a native uint8 batch of that size (which
              prices the float-image route through PatchEmbed)
  draws       mean step time over 200 seeded draws (every size captured beforehand) against the fixed 640 step

    python tools/multiscale_bench.py [--bs 64] [--size 640] [--scale s] [--rounds 3] [--steps 10] [--draws 200] [--no-native]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lead_yolo_amd as L  # noqa: E402

GS = 32


def batch(bs, s, seed):
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randint(0, 256, (bs, 3, s, s), dtype=torch.uint8, generator=g).cuda()
    n = bs * 7
    tg = torch.cat([torch.arange(bs).repeat_interleave(7).float()[:, None], torch.zeros(n, 1), torch.rand(n, 2, generator=g) * 0.8 + 0.1,
                    torch.rand(n, 2, generator=g) * 0.2 + 0.02], 1).cuda()
    return imgs, tg


def trainer(scale):
    torch.manual_seed(0)
    model = L.Model(L.load_cfg(scale=scale)).cuda().train()
    return model, L.ComputeLoss(model), L.smart_optimizer(model, "SGD", 0.01, 0.937, 5e-4), L.ModelEMA(model)


def timed(fn, n):
    """ms per call over n calls (device events)"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def reserved_alone(a, size):
    """child process: a plain GraphedTrainStep whose step runs at `size` (resized from the base batch), nothing else -> reserved bytes"""
    model, cl, opt, ema = trainer(a.scale)
    imgs, tg = batch(a.bs, a.size, 1)
    L.GraphedTrainStep(model, cl, opt, imgs, tg, ema=ema, amp=torch.bfloat16, warmup=3, img_size=(size, size))()
    torch.cuda.synchronize()
    print(json.dumps(dict(reserved=torch.cuda.memory_reserved(), allocated=torch.cuda.memory_allocated())))


def reserved_all(a, order):
    """child process: every size captured on MultiScaleTrainStep's one pool in the given order, no step taken -> reserved bytes"""
    model, cl, opt, ema = trainer(a.scale)
    imgs, tg = batch(a.bs, a.size, 1)
    step = L.MultiScaleTrainStep(model, cl, opt, imgs, tg, ema=ema, amp=torch.bfloat16, warmup=3, img_size=a.size, gs=GS, seed=0)
    sizes = list(range(int(a.size * 0.5) // GS * GS, int(a.size * 1.5) // GS * GS + 1, GS))
    for s in (sizes if order == "ascending" else sizes[::-1]):
        step.capture(s)
    torch.cuda.synchronize()
    print(json.dumps(dict(reserved=torch.cuda.memory_reserved(), allocated=torch.cuda.memory_allocated(), graphed=len(step.graphed_sizes))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--scale", default="s")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--draws", type=int, default=200)
    ap.add_argument("--no-native", action="store_true", help="skip the native-size GraphedTrainStep of every size")
    ap.add_argument("--reserved-alone", type=int, default=None, metavar="SIZE", help=argparse.SUPPRESS)
    ap.add_argument("--reserved-all", default=None, choices=("ascending", "descending"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reserved_alone is not None:
        return reserved_alone(a, a.reserved_alone)
    if a.reserved_all is not None:
        return reserved_all(a, a.reserved_all)
    bs, base = a.bs, a.size
    sizes = list(range(int(base * 0.5) // GS * GS, int(base * 1.5) // GS * GS + 1, GS))
    med = lambda xs: float(np.median(xs))          # noqa: E731
    gib = lambda b: round(b / 2 ** 30, 3)          # noqa: E731
    res = dict(model=f"lead-yolo-{a.scale}", bs=bs, size=base, dtype="bf16", sizes=sizes, rounds=a.rounds, steps_per_round=a.steps)

    # ---- reserved memory: fresh child processes, before this one opens the device
    def child(*args):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), *args, "--bs", str(bs), "--size", str(base), "--scale", a.scale],
                             check=True, capture_output=True, text=True).stdout
        return json.loads(out.strip().splitlines()[-1])
    res.update(reserved_gib_base_only=gib(child("--reserved-alone", str(base))["reserved"]),
               reserved_gib_largest_alone=gib(child("--reserved-alone", str(sizes[-1]))["reserved"]),
               reserved_gib_all_sizes_ascending=gib(child("--reserved-all", "ascending")["reserved"]),
               reserved_gib_all_sizes_largest_first=gib(child("--reserved-all", "descending")["reserved"]))

    # ---- every size captured on the one pool: capture time per size, reserved memory after all of them
    imgs, tg = batch(bs, base, 1)
    model, cl, opt, ema = trainer(a.scale)
    t0 = time.perf_counter()
    step = L.MultiScaleTrainStep(model, cl, opt, imgs, tg, ema=ema, amp=torch.bfloat16, warmup=3, img_size=base, gs=GS, seed=0)
    torch.cuda.synchronize()
    capture_s = {base: time.perf_counter() - t0}
    for s in sorted(sizes, key=lambda v: (abs(v - base), v)):      # outwards from the base size: the largest comes last
        if s != base:
            t0 = time.perf_counter()
            step(size=s)
            torch.cuda.synchronize()
            capture_s[s] = time.perf_counter() - t0            # (state saved and put back, warm-up steps, capture, first replay)
    res.update(reserved_gib_all_sizes_outwards=gib(torch.cuda.memory_reserved()), allocated_gib_all_sizes=gib(torch.cuda.memory_allocated()),
               graphed_sizes=len(step.graphed_sizes), capture_s={str(k): round(v, 2) for k, v in sorted(capture_s.items())})

    # ---- the kernel against F.interpolate on the device
    kern = {}
    for s in (base // 2, base - GS, base + GS, sizes[-1]):
        out = torch.empty((bs, 3, s, s), device="cuda")
        runs = dict(hip=lambda: L.ops.resize_u8(imgs, (s, s), out=out),
                    aten=lambda: F.interpolate(imgs.float() / 255, size=(s, s), mode="bilinear", align_corners=False))
        us = {k: [] for k in runs}
        for fn in runs.values():
            timed(fn, 5)
        for _ in range(a.rounds):
            for k, fn in runs.items():
                us[k].append(timed(fn, 50) * 1e3)
        nbytes = imgs.numel() + 4 * out.numel()
        kern[str(s)] = dict(resize_u8_us=round(med(us["hip"]), 2), resize_u8_gbs=round(nbytes / med(us["hip"]) / 1e3, 1),
                            interpolate_us=round(med(us["aten"]), 2), mb=round(nbytes / 1e6, 1),
                            resize_u8_all=[round(x, 2) for x in us["hip"]], interpolate_all=[round(x, 2) for x in us["aten"]])
        del out
    res.update(kernel=kern)

    # ---- per size: the replayed resized step against the native-size step
    per = {}
    for s in sizes:
        runs = dict(resized=lambda: step(size=s))
        native = None
        if not a.no_native:
            model_n, cl_n, opt_n, ema_n = trainer(a.scale)
            native = L.GraphedTrainStep(model_n, cl_n, opt_n, *batch(bs, s, 2), ema=ema_n, amp=torch.bfloat16, warmup=3)
            runs["native"] = native
        ms = {k: [] for k in runs}
        for fn in runs.values():
            timed(fn, 3)
        for _ in range(a.rounds):
            for k, fn in runs.items():
                ms[k].append(timed(fn, a.steps))
        per[str(s)] = dict(**{f"{k}_ms": round(med(v), 4) for k, v in ms.items()},
                           **{f"{k}_all": [round(x, 4) for x in v] for k, v in ms.items()})
        if native is not None:
            per[str(s)]["resized_over_native"] = round(med(ms["resized"]) / med(ms["native"]), 4)
            del native, runs, model_n, cl_n, opt_n, ema_n
            torch.cuda.empty_cache()
    res.update(per_size=per)

    # ---- 200 seeded draws against the fixed base size, alternating
    import random
    rng = random.Random(0)
    draws = [L.multi_scale_size(base, GS, rng) for _ in range(a.draws)]
    it = iter(draws * (a.rounds + 1))
    fixed, drawn = [], []
    timed(lambda: step(size=base), 3)
    for _ in range(a.rounds):
        fixed.append(timed(lambda: step(size=base), a.steps))
        drawn.append(timed(lambda: step(size=next(it)), a.draws))
    res.update(step_fixed_ms=round(med(fixed), 4), step_drawn_mean_ms=round(med(drawn), 4), drawn_over_fixed=round(med(drawn) / med(fixed), 4),
               draws=a.draws, drawn_pixels_over_base=round(float(np.mean([d * d for d in draws])) / (base * base), 4),
               step_fixed_all=[round(x, 4) for x in fixed], step_drawn_all=[round(x, 4) for x in drawn])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
