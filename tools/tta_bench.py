"""Augmented inference (augment=True) timing: lead-yolo-s, 640 x 640, batch 32, fp32 and bf16 (autocast), on one GPU.

For each dtype: the plain forward and the augmented forward, eager and graphed (graph.GraphedForward), and the ly_scale_img launch alone,
timed with HIP events as the median of --rounds rounds of --iters calls; the resample's share of HBM is its algorithmic bytes (the source
once per output + both outputs) over its time against 6.3 TB/s.  Prints one JSON line.

  python tools/tta_bench.py [--bs 32] [--size 640] [--iters 20] [--rounds 5]
  python tools/tta_bench.py --profile-replay       one captured augmented replay after one eager warm-up (run under rocprofv3 --kernel-trace)
  python tools/tta_bench.py --summarize DIR        per-kernel table of that replay from the trace under DIR: every dispatch from the last
                                                   ly_scale_img launch on (the replay's first node)"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12            # achievable copy rate, bytes / s (MI355X guide)


def _model(dev):
    import torch
    import lead_yolo_amd as L
    from oracle import synth
    torch.manual_seed(0)
    m = L.Model(L.load_cfg(scale="s"))
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 4242)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    m.load_state_dict(st)
    return m.to(dev).eval()


def _time(fn, iters, rounds):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return sorted(ms)[len(ms) // 2]


def bench(bs, size, iters, rounds):
    import torch
    import lead_yolo_amd as L
    from lead_yolo_amd import ops
    dev = torch.device("cuda:0")
    m = _model(dev)
    x = torch.rand((bs, 3, size, size), generator=torch.Generator().manual_seed(1)).to(dev)
    plan = m.augment_plan(size, size)
    specs = [(*p["resized"], *p["size"], p["flip"]) for p in plan["passes"] if p["scale"] != 1.0]
    nbytes = x.element_size() * sum(x.numel() + bs * 3 * ho * wo for (_, _, ho, wo, _) in specs)
    out = dict(metric="tta_forward", model="lead-yolo-s", bs=bs, size=size, rows_plain=sum(plan["passes"][0]["level_rows"]), rows_aug=plan["rows"])
    for name, dt in (("fp32", None), ("bf16", torch.bfloat16)):
        ctx = (lambda: torch.autocast("cuda", dtype=dt)) if dt is not None else (lambda: torch.autocast("cuda", enabled=False))
        r = {}
        with torch.no_grad(), ctx():
            r["plain_eager_ms"] = _time(lambda: m(x), iters, rounds)
            r["aug_eager_ms"] = _time(lambda: m(x, augment=True), iters, rounds)
            g = L.GraphedForward(m, x)
            r["plain_graph_ms"] = _time(lambda: g(), iters, rounds)
            del g
            ga = L.GraphedForward(m, x, augment=True)
            r["aug_graph_ms"] = _time(lambda: ga(), iters, rounds)
            del ga
            r["scale_img_us"] = 1e3 * _time(lambda: ops.scale_img(x, specs), iters, rounds)
        r["aug_over_plain_graph"] = r["aug_graph_ms"] / r["plain_graph_ms"]
        r["aug_over_plain_eager"] = r["aug_eager_ms"] / r["plain_eager_ms"]
        r["scale_img_MB"] = nbytes / 1e6
        r["scale_img_hbm_share"] = nbytes / (r["scale_img_us"] * 1e-6) / HBM
        out[name] = {k: round(v, 4) for k, v in r.items()}
        torch.cuda.empty_cache()
    return out


def profile_replay(bs, size):
    import torch
    import lead_yolo_amd as L
    dev = torch.device("cuda:0")
    m = _model(dev)
    x = torch.rand((bs, 3, size, size), generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        g = L.GraphedForward(m, x, augment=True, warmup=1)
        torch.cuda.synchronize()
        g()
        torch.cuda.synchronize()
    print(json.dumps(dict(profile_replay=True, bs=bs, size=size)))


def _dispatches(d):
    """(name, start, end) of every kernel dispatch rocprofv3 wrote under d: its rocpd database (*.db), else *kernel_trace.csv"""
    out = []
    for f in glob.glob(os.path.join(d, "**", "*.db"), recursive=True):
        import sqlite3
        with sqlite3.connect(f) as c:
            out += list(c.execute("select name, start, end from kernels"))
    if not out:
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(f) as fh:
                out += [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(fh)]
    return sorted(out, key=lambda r: r[1])


def summarize(d):
    rows = _dispatches(d)
    first = max(i for i, r in enumerate(rows) if r[0].startswith("void ly_scale_img_kernel") or r[0].startswith("ly_scale_img_kernel"))
    rows = rows[first:]                                     # the replay opens with its one resampling launch; set-up and warm-up precede it
    agg = {}
    for name, t0, t1 in rows:
        a = agg.setdefault(name, [0, 0.0])
        a[0] += 1
        a[1] += (t1 - t0) / 1e3
    total = sum(v[1] for v in agg.values())
    span = (max(r[2] for r in rows) - rows[0][1]) / 1e3
    print(f"# one graphed augmented replay, lead-yolo-s 640 x 640 bs 32 fp32 (rocprofv3 --kernel-trace --stats; tools/tta_bench.py --summarize): "
          f"{len(rows)} kernels, {total:.1f} us of kernel time, {span:.1f} us from the first start to the last end (three passes overlap)")
    print(f"{'calls':>5} {'total_us':>10} {'avg_us':>9} {'share':>6}  kernel")
    for k, (n, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print(f"{n:5d} {t:10.1f} {t / n:9.1f} {t / total:6.1%}  {k[:160]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile-replay", action="store_true")
    ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.profile_replay:
        profile_replay(a.bs, a.size)
    else:
        print(json.dumps(bench(a.bs, a.size, a.iters, a.rounds)))


if __name__ == "__main__":
    main()
