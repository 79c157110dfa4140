"""On-device training augmentation at bs = 64, s = 640 (hyp.scratch-low, a synthetic bank of load_image-shaped images): ly_mosaic_img and
ly_mosaic_labels alone (us per launch, GB/s over the output bytes + the source bytes the warp references), the host cost of sample(), and the
captured lead-yolo-s bf16 training step in two forms, in alternating rounds in one process: replayed on a fixed batch, and fed by MosaicAugment
through out=(step.imgs, step.targets) before every replay.  One JSON line; --profile-fed runs only fed steps (the program a
`rocprofv3 --kernel-trace --stats` run wraps).

--mixup P: the mixup entry points instead (MosaicAugment(..., allow_mixup=True) with hyp['mixup'] = P; every other key scratch-low).  One plan
drawn at P; in alternating rounds in one process, medians: ly_mosaic_img on the plan's primaries, ly_mosaic_mix_img on the same primaries
without partners, ly_mosaic_mix_img with the partners; ly_mosaic_mix_labels; then the captured step (targets of the doubled capacity) fed by
that augmenter against the fixed batch (--kernels-only leaves the step out).  One JSON line.

    python tools/mosaic_bench.py [--bs 64] [--size 640] [--bank 256] [--rounds 5] [--steps 20] [--profile-fed] [--mixup P [--kernels-only]]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lead_yolo_amd as L  # noqa: E402


def make_bank(n, s, seed=0):
    rng = np.random.default_rng(seed)
    ims, labs = [], []
    for i in range(n):
        short = int(rng.integers(s * 9 // 16, s + 1))
        h, w = (s, short) if i % 2 else (short, s)
        base = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
        ims.append(np.ascontiguousarray(np.kron(base, np.ones((8, 8, 1), np.uint8))[:h, :w]))
        k = int(rng.integers(0, 12))
        labs.append(np.concatenate([np.zeros((k, 1)), rng.uniform(0.1, 0.9, (k, 2)), rng.uniform(0.02, 0.2, (k, 2))], 1).astype(np.float32))
    return L.ImageBank(ims, labs, s, device="cuda")


def referenced_bytes(aug, plan):
    """source bytes the warp reads: distinct canvas pixels inside a tile rectangle that some output pixel's taps touch, x 3"""
    s, total = aug.img_size, 0
    v, u = np.meshgrid(np.arange(s, dtype=np.float32), np.arange(s, dtype=np.float32), indexing="ij")
    for e in list(plan.table) + list(plan.partner_table or []):            # with mixup the second mosaics are read too
        a = np.array(e.minv[:], dtype=np.float32)
        X = np.floor((a[0] * u + a[1] * v) + a[2]).astype(np.int64)
        Y = np.floor((a[3] * u + a[4] * v) + a[5]).astype(np.int64)
        pts = np.concatenate([np.stack([X + dx, Y + dy], -1).reshape(-1, 2) for dx in (0, 1) for dy in (0, 1)])
        inside = np.zeros(len(pts), bool)
        for t in range(4):
            tl = e.tile[t]
            if tl.src >= 0:
                inside |= (pts[:, 0] >= tl.x1a) & (pts[:, 0] < tl.x2a) & (pts[:, 1] >= tl.y1a) & (pts[:, 1] < tl.y2a)
        p = pts[inside]
        total += 3 * len(np.unique(p[:, 1] * (8 * s) + p[:, 0]))
    return total


def time_kernel(fn, reps=50):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--bank", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--profile-fed", action="store_true")
    ap.add_argument("--mixup", type=float, default=None, metavar="P")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    bs, s = a.bs, a.size
    bank = make_bank(a.bank, s)
    med = lambda xs: float(np.median(xs))          # noqa: E731
    if a.mixup is None:
        aug = L.MosaicAugment(bank, batch_size=bs, seed=0)
        res = dict(bs=bs, size=s, bank_images=len(bank), capacity=aug.capacity, hyp="scratch-low")
    else:
        aug = L.MosaicAugment(bank, dict(mixup=a.mixup), batch_size=bs, seed=0, allow_mixup=True)
        res = dict(bs=bs, size=s, bank_images=len(bank), capacity=aug.capacity, hyp="scratch-low + mixup", mixup=a.mixup)
    batches = [b for e in range(4) for b in aug.batches(e)]
    if a.mixup is not None:
        plain = L.MosaicAugment(bank, batch_size=bs, seed=0)
        plan = aug.sample(batches[0])
        bare = [L.mosaic.Draw(d.mosaic, d.sources, d.xc, d.yc, d.degrees, d.scale, d.shear, d.translate, d.gains, d.flipud, d.fliplr)
                for d in plan.draws]
        tab_plain, tab_none, tab_mix = plain.upload(plain.plan(bare)), aug.upload(aug.plan(bare)), aug.upload(plan)
        imgs = torch.empty((bs, 3, s, s), dtype=torch.uint8, device="cuda")
        tg = torch.empty((aug.capacity, 6), dtype=torch.float32, device="cuda")
        runs = dict(mosaic_img_us=lambda: plain.launch(tab_plain, bs, imgs, tg, which=1),
                    mix_img_no_partner_us=lambda: aug.launch(tab_none, bs, imgs, tg, which=1),
                    mix_img_us=lambda: aug.launch(tab_mix, bs, imgs, tg, which=1, k=plan.k),
                    mix_labels_us=lambda: aug.launch(tab_mix, bs, imgs, tg, which=2, k=plan.k))
        for fn in runs.values():
            time_kernel(fn, reps=5)
        us = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                us[k].append(time_kernel(fn))
        out_b, src_b, src_plain = imgs.numel(), referenced_bytes(aug, plan), referenced_bytes(plain, plain.plan(bare))
        res.update({k: round(med(v), 2) for k, v in us.items()})
        res.update({k[:-3] + "_all": [round(x, 2) for x in v] for k, v in us.items()})
        res.update(partners=plan.k, out_mb=round(out_b / 1e6, 2), src_mb=round(src_b / 1e6, 2), src_primaries_mb=round(src_plain / 1e6, 2),
                   mosaic_img_spread_us=round(max(us["mosaic_img_us"]) - min(us["mosaic_img_us"]), 2),
                   no_partner_over_plain=round(med(us["mix_img_no_partner_us"]) / med(us["mosaic_img_us"]), 4),
                   mix_over_plain=round(med(us["mix_img_us"]) / med(us["mosaic_img_us"]), 4),
                   mix_img_gbs=round((out_b + src_b) / med(us["mix_img_us"]) / 1e3, 1), kernel_rounds=a.rounds)
        t0 = time.perf_counter()
        for b in batches[:20]:
            aug.sample(b)
        res.update(sample_host_ms=round((time.perf_counter() - t0) * 1e3 / 20, 3))
        if a.kernels_only:
            print(json.dumps(res))
            return
    elif not a.profile_fed:
        plan = aug.sample(batches[0])
        tab = aug.upload(plan)
        imgs = torch.empty((bs, 3, s, s), dtype=torch.uint8, device="cuda")
        tg = torch.empty((aug.capacity, 6), dtype=torch.float32, device="cuda")
        us_img = time_kernel(lambda: aug.launch(tab, bs, imgs, tg, which=1))
        us_lab = time_kernel(lambda: aug.launch(tab, bs, imgs, tg, which=2))
        out_b, src_b = imgs.numel(), referenced_bytes(aug, plan)
        t0 = time.perf_counter()
        for b in batches[:20]:
            aug.sample(b)
        host_ms = (time.perf_counter() - t0) * 1e3 / 20
        res.update(mosaic_img_us=round(us_img, 2), mosaic_labels_us=round(us_lab, 2), out_mb=round(out_b / 1e6, 2), src_mb=round(src_b / 1e6, 2),
                   mosaic_img_gbs=round((out_b + src_b) / us_img / 1e3, 1), sample_host_ms=round(host_ms, 3))
    # the captured training step (lead-yolo-s, bf16, FusedSGD + EMA as bench.py)
    model = L.Model(L.load_cfg(scale="s")).cuda().train()
    opt = L.smart_optimizer(model, "SGD", 0.01, 0.937, 5e-4)
    ema = L.ModelEMA(model)
    cl = L.ComputeLoss(model)
    imgs, tg = aug(batches[0])
    step = L.GraphedTrainStep(model, cl, opt, imgs, tg, ema=ema, amp=torch.bfloat16, warmup=3)
    fixed_imgs, fixed_tg = imgs.clone(), tg.clone()
    it = iter(batches * 100)

    def run(fed, n):
        if not fed:
            step.imgs.copy_(fixed_imgs)
            step.targets.copy_(fixed_tg)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(n):
            if fed:
                aug(next(it), out=(step.imgs, step.targets))
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n, (time.perf_counter() - t0) * 1e3 / n

    if a.profile_fed:
        run(True, a.steps)
        print(json.dumps(dict(profile_fed_steps=a.steps)))
        return
    run(False, 3)
    run(True, 3)
    fixed, fed = [], []
    for _ in range(a.rounds):
        fixed.append(run(False, a.steps)[0])
        fed.append(run(True, a.steps)[0])
    res.update(step_fixed_ms=round(med(fixed), 4), step_fed_ms=round(med(fed), 4), fed_over_fixed=round(med(fed) / med(fixed), 4),
               rounds=a.rounds, steps_per_round=a.steps, step_fixed_all=[round(x, 4) for x in fixed], step_fed_all=[round(x, 4) for x in fed])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
