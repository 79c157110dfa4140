"""Times the full training step (forward, loss, backward, clip, optimiser) of lead-yolo-s on synthetic COCO-shaped data.

    --optimizer SGD | Adam | AdamW, or a comma list (e.g. SGD,AdamW): one model per optimiser, timed in alternating rounds
    --fl-gamma G / --autobalance: the loss options (focal loss on both BCEs, device-resident autobalance); a name may carry them per leg as
      NAME+focal (fl_gamma 1.5 and autobalance), e.g. --optimizer SGD,SGD+focal times both settings in alternating rounds of one process
    --graphed: the captured step (train.GraphedTrainStep with ModelEMA), as bench.py times it; --dtype bf16: autocast bf16"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import lead_yolo_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--bs", type=int, default=32)
ap.add_argument("--size", type=int, default=640)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--scale", default="s")
ap.add_argument("--fwd-only", action="store_true")
ap.add_argument("--optimizer", default="SGD")
ap.add_argument("--graphed", action="store_true")
ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
ap.add_argument("--rounds", type=int, default=1, help="alternating timed rounds of --steps steps per optimiser")
ap.add_argument("--fl-gamma", type=float, default=0.0, help="focal loss gamma (0: plain BCE)")
ap.add_argument("--autobalance", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda:0")
amp = torch.bfloat16 if a.dtype == "bf16" else None
g = torch.Generator().manual_seed(0)
imgs = torch.randint(0, 256, (a.bs, 3, a.size, a.size), dtype=torch.uint8, generator=g).to(dev)
nb = 7 * a.bs
tg = torch.cat((torch.sort(torch.randint(0, a.bs, (nb, 1), generator=g).float(), 0)[0], torch.zeros(nb, 1),
                torch.rand(nb, 2, generator=g) * 0.8 + 0.1, torch.rand(nb, 2, generator=g) * 0.2 + 0.02), 1).to(dev)


def make(name):
    name, _, leg = name.partition("+")
    gamma, auto = (1.5, True) if leg == "focal" else (a.fl_gamma, a.autobalance)
    torch.manual_seed(0)
    m = L.Model(L.load_cfg(scale=a.scale)).to(dev).train()
    opt = L.smart_optimizer(m, name, 0.01 if name == "SGD" else 1e-3, 0.937, 5e-4 * a.bs / 64)
    cl = L.ComputeLoss(m, autobalance=auto, hyp=dict(fl_gamma=gamma), allow_focal=True)
    if a.fwd_only:
        def step():
            with torch.no_grad():
                return m(imgs.float() / 255)
    elif a.graphed:
        step = L.GraphedTrainStep(m, cl, opt, imgs, tg, ema=L.ModelEMA(m), amp=amp, warmup=max(a.warmup, 2))
    else:
        def step():
            return L.train_step(m, cl, opt, imgs, tg, amp=amp)
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    return step


names = a.optimizer.split(",")
steps = {n: make(n) for n in names}
times = {n: [] for n in names}
for _ in range(a.rounds):
    for n in names:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            steps[n]()
        torch.cuda.synchronize()
        times[n].append((time.perf_counter() - t0) / a.steps)
what = "train-fwd" if a.fwd_only else ("graphed train-step" if a.graphed else "train-step")
for n in names:
    ts = sorted(times[n])
    dt = ts[len(ts) // 2]
    print(f"{n}: bs={a.bs} size={a.size} {a.dtype} {what}: {dt*1e3:.3f} ms/step (median of {len(ts)} rounds, min {ts[0]*1e3:.3f}, "
          f"max {ts[-1]*1e3:.3f})  {a.bs/dt:.1f} img/s  peak mem {torch.cuda.max_memory_allocated()/2**30:.2f} GiB")
