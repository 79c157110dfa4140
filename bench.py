"""bench.py — LEAD-YOLO hot path on MI355X.  Contract: see the task statement / DESIGN.md §6.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--scale s] [--size 640] [--dtype bf16|f32] [--mode train|forward]
                    [--dump-outputs DIR] [--full]

A plain run sets up, runs W warm-up steps, times exactly K steps, and prints the line (`ms_per_step` = one timed step).  `--full` adds
everything else the line can carry: 3 timed regions (median), the sustained run, the eager step, the per-kernel roofline probe, the step's
kernel families, the pconv_rfcbam probes, the secondary forward figures and the CPU baseline.  `--dump-outputs DIR` writes what the timed
path computed in its last timed step as DIR/<name>.npy (float32; a fixed seeded sample where the total would exceed 64 MB): train mode the
loss, the loss items and the model's and the EMA's floating-point state after the step, forward mode the detections and the three levels'
raw maps.  Inputs and weights are seeded, so two builds run with the same arguments can be compared output for output.

Default line = BASELINE.json's metric: images/sec (640x640) fwd+bwd — one "step" is one full optimisation step of
lead-yolo-s at bs=64/GPU (BASELINE.json configs[2]): uint8 batch already resident in HBM -> train-mode forward ->
ComputeLoss -> HIP backward -> [N > 1: each ~2 MB gradient bucket's RCCL all-reduce is released by an event node inside the replayed
backward graph and runs on a communication stream while the rest of backward executes] -> clip 10 -> SGD-nesterov (3 groups) -> EMA.  `--gpus N` with N > 1 and no WORLD_SIZE in the environment makes THIS process a launcher:
it starts N ranks through `torch.distributed.run` (before anything touches the GPU) and exits with their code; under
an external torchrun it is a rank and WORLD_SIZE must equal --gpus.  Rank 0 prints ONE JSON line.

`roofline` = the largest kernel of the kernel FAMILY that owns most of the step (roofline.step.families: every launch of one steady-state
step, by family, with algorithmic and PMC bytes), timed live with HIP events on the launch stream (ops.PROFILE hooks); `roofline.step` = the
whole step against the HBM roof (SURVEY §8(d) block-fused bytes / step time);
`roofline.pconv_rfcbam_fwd` = the north-star sub-metric: every launch of the six MLPBlocks and four RFCBAMConvs
(eval forward, bs=64) against SURVEY §8(d)'s algorithmic bytes; `cpu_baseline` = the oracle (oracle/functional.py, the
parity-pinned CPU restatement of the reference) taking the same optimisation step on the host cores over a bounded
sample; `forward` = the eval-forward throughput of configs[1] (bs=32, hipGraph replay) as a secondary figure.
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured float4 copy)
VALU_F32_PEAK_TFLOPS = 157.3     # MI355X_MICROARCH.md: peak FP32 (vector) = PACKED FMA (v_pk_fma_f32); a SIMD issues one wave64 vector instruction per ~4
                                 # cycles however many waves it holds (profiles/r06_valu_probe.txt), so scalar v_fma_f32 code tops out at half of this
# kernels that issue matrix instructions: the `flops` their wrappers report (ops._Timed) are MFMA work, `valu_flops` vector work
MFMA_KERNELS = ("ly_gemm_kernel", "ly_conv3x3", "ly_mlp", "ly_wgrad", "ly_rf3c", "ly_rf3m", "ly_rfcbam3")
BF16_MFMA_PEAK_TFLOPS = 2500.0  # dense bf16; fp32-grade products take 3 bf16 MFMAs (csrc/ly_tile.hpp)
ARITH = {"f32": "fp32 storage and accumulation, bf16x3 split products on the bf16 matrix cores (~2^-16 per product)",
         "bf16": "bf16 activations / saved tensors / activation gradients, single-plane bf16 MFMA products, fp32 accumulate, "
                 "fp32 BatchNorm statistics, fp32 master weights and weight gradients"}
# fused PConv+RFCBAMConv forward, elements per image (in + out) and parameters
PCONV_RFCBAM_ELEMS_PER_IMG = 2_636_800 + 2_316_800
PCONV_RFCBAM_PARAMS = 1_094_432


def build_model(scale, device, seed=0, train=False):
    import lead_yolo_amd as L
    torch.manual_seed(seed)
    m = L.Model(L.load_cfg(scale=scale))
    g = torch.Generator().manual_seed(seed + 1)
    for mod in m.modules():                      # non-trivial BN statistics
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
    m = m.to(device)
    return m.train() if train else m.eval()


def synth_u8(b, size, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (b, 3, size, size), generator=g, dtype=torch.uint8)


def synth_batch(b, size, seed, device):
    return (synth_u8(b, size, seed).float() / 255).to(device)


def synth_targets(b, seed):
    """COCO-shaped labels: ~7 boxes per image, (img, cls=0, xy ~ U(.1,.9), wh ~ U(.02,.22))"""
    nb = 7 * b
    g = torch.Generator().manual_seed(seed)
    return torch.cat((torch.sort(torch.randint(0, b, (nb, 1), generator=g).float(), 0)[0], torch.zeros(nb, 1),
                      torch.rand(nb, 2, generator=g) * 0.8 + 0.1, torch.rand(nb, 2, generator=g) * 0.2 + 0.02), 1)


def probe_step(step_fn, iters=2):
    """Times every C-ABI launch of `step_fn` with HIP events on the launch stream (ops.PROFILE hooks), groups them by
    the kernel name rocprofv3 prints, and returns the per-kernel table.  Algorithmic bytes: input once + output once +
    parameters once at the storage dtype; algorithmic flops: 2*MAC."""
    from lead_yolo_amd import ops
    step_fn()
    torch.cuda.synchronize()
    ops.PROFILE = []
    try:
        for _ in range(iters):
            step_fn()
        torch.cuda.synchronize()
    finally:
        recs, ops.PROFILE = ops.PROFILE, None
    table = {}
    for name, flops, nbytes, e0, e1, vflops in recs:
        t = table.setdefault(name, dict(kernel=name, calls=0, ms=0.0, flops=0.0, bytes=0.0, valu_flops=0.0))
        if not name.startswith(MFMA_KERNELS):         # no matrix instruction in the kernel: whatever arithmetic it reports is vector work
            flops, vflops = 0.0, vflops + flops
        t["calls"] += 1
        t["ms"] += e0.elapsed_time(e1)
        t["flops"] += flops
        t["valu_flops"] += vflops
        t["bytes"] += nbytes
    rows = []
    for t in table.values():
        c = t["calls"]
        rows.append(dict(kernel=t["kernel"], calls_per_step=c / iters, ms_per_launch=t["ms"] / c, ms_per_step=t["ms"] / iters,
                         flops=t["flops"] / c, valu_flops=t["valu_flops"] / c, bytes=t["bytes"] / c))
    rows.sort(key=lambda r: -r["ms_per_step"])
    return rows


def committed_pmc(kernel, suffix):
    """per-launch figures of `kernel` from the newest committed rocprofv3 PMC summary profiles/*_<suffix>.json
    (tools/pmc_traffic.py: FETCH_SIZE doubled per MI355X_MICROARCH.md + WRITE_SIZE; tools/pmc_mfma.py), or None."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", f"*_{suffix}.json")), reverse=True):
        try:
            d = json.load(open(path))
        except (OSError, ValueError):
            continue
        if kernel in d:
            return dict(d[kernel], source=os.path.basename(path))
    return None


def committed_row0(dtype):
    """first kernel row of the newest committed per-kernel table of one steady-state training step (profiles/*_train_<dtype>_step_kernels.txt,
    tools/step_kernels.py: device time per KERNEL, most time first), or None"""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", f"*_train_{dtype}_step_kernels.txt")), reverse=True):
        try:
            lines = [ln for ln in open(path).read().splitlines()[1:] if ln.strip()]
        except OSError:
            continue
        if lines:
            return lines[0][:130].strip(), os.path.basename(path)
    return None


def usable_cores():
    """host cores this process may actually use: affinity mask capped by the cgroup CPU quota"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _cpu_train_leg(scale, size, b, threads, budget_s, min_steps=3, max_steps=40):
    """median optimisation-step time of the oracle (train-mode forward, loss, autograd backward, clip 10, SGD-nesterov with the three groups)"""
    from oracle import functional as OF
    import lead_yolo_amd as L
    torch.set_num_threads(threads)
    m = build_model(scale, "cpu", train=True)
    st = {k: v.clone() for k, v in m.state_dict().items()}
    cfg = L.load_cfg(scale=scale)
    imgs = synth_u8(b, size, 0).float() / 255
    tg = synth_targets(b, 1)
    params = {k: v for k, v in st.items() if v.is_floating_point() and "running" not in k and not k.endswith("anchors")}
    groups = {g: [k for k in ks if k in params] for g, ks in OF.param_groups(list(st)).items()}
    bufs, times = {}, []
    t_all = time.perf_counter()
    while True:
        t0 = time.perf_counter()
        for p in params.values():
            p.requires_grad_(True)
            p.grad = None
        pred = OF.model_forward(st, cfg, imgs, m.stride, training=True)
        loss, _ = OF.compute_loss(pred, tg, st["model.23.anchors"], nc=1)
        loss.backward()
        grads = {k: p.grad for k, p in params.items()}
        total = torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())).float()
        coef = torch.clamp(10.0 / (total + 1e-6), max=1.0)
        grads = {k: g * coef for k, g in grads.items()}
        with torch.no_grad():
            for gname, dec in (("decay", 5e-4), ("bn", 0.0), ("bias", 0.0)):
                OF.sgd_nesterov_step({k: params[k] for k in groups[gname]}, grads, bufs, 0.01, 0.937, dec)
        times.append(time.perf_counter() - t0)
        if (time.perf_counter() - t_all > budget_s and len(times) >= min_steps + 1) or len(times) >= max_steps + 1:
            break
    return times[1:]                                 # first step = warm-up (allocator, oneDNN primitive caches)


def _cpu_forward_leg(scale, size, b, threads, budget_s, min_iters=3, max_iters=100):
    from oracle import functional as OF
    import lead_yolo_amd as L
    torch.set_num_threads(threads)
    m = build_model(scale, "cpu")
    st = {k: v.clone() for k, v in m.state_dict().items()}
    cfg = L.load_cfg(scale=scale)
    x = synth_batch(b, size, 0, "cpu")
    times = []
    with torch.no_grad():
        OF.model_forward(dict(st), cfg, x, m.stride, training=False)      # warm-up
        t_all = time.perf_counter()
        while True:
            t0 = time.perf_counter()
            OF.model_forward(st, cfg, x, m.stride, training=False)
            times.append(time.perf_counter() - t0)
            if (time.perf_counter() - t_all > budget_s and len(times) >= min_iters) or len(times) >= max_iters:
                break
    return times


def _leg(times, b, what, threads):
    med = statistics.median(times)
    return dict(value=round(b / med, 2), unit="images/sec", batch=b, threads=threads, iterations=len(times),
                ms_min_median_max=[round(min(times) * 1e3, 1), round(med * 1e3, 1), round(max(times) * 1e3, 1)], what=what)


def cpu_forward_legs(scale, size, cores):
    """the oracle's eval forward at bs=1 and bs=32 on all usable cores, and the 1-thread figure (bs=1)"""
    return {"eval_forward_bs1": _leg(_cpu_forward_leg(scale, size, 1, cores, 2.0, min_iters=5), 1, "eval forward", cores),
            "eval_forward_bs32": _leg(_cpu_forward_leg(scale, size, 32, cores, 4.0), 32, "eval forward", cores),
            "eval_forward_bs1_1thread": _leg(_cpu_forward_leg(scale, size, 1, 1, 2.0), 1, "eval forward", 1)}


def cpu_baseline_train(scale, size, budget_s=10.0, b=16):
    """The oracle taking the same optimisation step (train-mode forward, loss, autograd backward, clip 10, SGD-nesterov
    with the three groups) on the host cores: median step time over a bounded sample, at the largest batch that keeps >= 3 timed
    steps inside the budget; beside it the 1-thread figure and the eval-forward legs of section 3 (i)."""
    cores = usable_cores()
    timed = _cpu_train_leg(scale, size, b, cores, budget_s)
    med = statistics.median(timed)
    out = dict(value=round(b / med, 2), unit="images/sec", cores=cores, kind="port", cpu=cpu_model_name(),
               sample=f"median of {len(timed)} optimisation steps (fwd + loss + bwd + clip + SGD-nesterov) of lead-yolo-{scale} bs={b} "
                      f"{size}x{size} fp32 by oracle/functional.py (torch {torch.__version__} CPU, {cores} threads), after 1 warm-up step; "
                      f"min/median/max {min(timed) * 1e3:.0f}/{med * 1e3:.0f}/{max(timed) * 1e3:.0f} ms per step")
    legs = {"train_step_1thread": _leg(_cpu_train_leg(scale, size, 2, 1, 4.0, min_steps=2), 2, "optimisation step", 1)}
    legs.update(cpu_forward_legs(scale, size, cores))
    out["legs"] = legs
    torch.set_num_threads(cores)
    return out


def cpu_baseline_forward(scale, size, budget_s=8.0, b=32):
    cores = usable_cores()
    times = _cpu_forward_leg(scale, size, b, cores, budget_s)
    med = statistics.median(times)
    out = dict(value=round(b / med, 2), unit="images/sec", cores=cores, kind="port", cpu=cpu_model_name(),
               sample=f"median of {len(times)} eval forwards of lead-yolo-{scale} bs={b} {size}x{size} fp32 by oracle/functional.py "
                      f"(torch {torch.__version__} CPU, {cores} threads)")
    out["legs"] = {"eval_forward_bs1": _leg(_cpu_forward_leg(scale, size, 1, cores, 2.0, min_iters=5), 1, "eval forward", cores),
                   "eval_forward_bs1_1thread": _leg(_cpu_forward_leg(scale, size, 1, 1, 2.0), 1, "eval forward", 1)}
    torch.set_num_threads(cores)
    return out


def pconv_rfcbam_probe(model, x, dtype, iters=10):
    """north-star sub-metric: eval forward of every MLPBlock (6) and RFCBAMConv (4) of lead-yolo-s at the batch in `x`,
    each module timed as a WHOLE (HIP events around the module call: SE pooling + MLP, statistics pass, rfa map, the
    contraction — every launch counts), summed, against SURVEY §8(d)'s algorithmic bytes (input once + output once +
    parameters once at the storage dtype)."""
    import lead_yolo_amd as L
    was_training = model.training
    model.eval()
    targets, inputs = [], {}
    for layer in model.model:
        if isinstance(layer, (L.BasicStage, L.RFCBAMConv)):
            targets.append(layer)
        elif isinstance(layer, torch.nn.Sequential) and all(isinstance(s, L.BasicStage) for s in layer):
            targets.extend(layer)
    hooks = [t.register_forward_pre_hook(lambda mod, a: inputs.__setitem__(id(mod), a[0])) for t in targets]
    try:
        with torch.no_grad():
            model(x)
    finally:
        for h in hooks:
            h.remove()
    # Each module is captured into its own hipGraph and replayed (serving mode, as the forward bench itself runs): at bs=64 the small
    # modules are a few launches of 5-30 us each, and eager launches through ctypes would time the host, not the kernels.
    total_ms, per, pairs = 0.0, [], []
    with torch.no_grad():
        for t in targets:
            xi = inputs[id(t)]
            if isinstance(xi, L.Lazy):
                xi = xi.materialize()
            xi = xi.clone()
            pairs.append((t, xi))
            side = torch.cuda.Stream(device=xi.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    yo = t(xi)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            # the module's own algorithmic bytes (input + output once at the storage dtype + fp32 parameters once) and the time
            # the north-star target of 0.22 of HBM would allow it (per-module budgets in the line)
            mod_bytes = (xi.numel() + yo.numel()) * xi.element_size() + 4 * sum(p.numel() for p in t.parameters())
            mode = "hipGraph replay"
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    t(xi)
                run = g.replay
            except Exception as e:                          # noqa: BLE001
                print(f"[bench] module capture unavailable ({type(e).__name__}: {e}); timing eager launches", file=sys.stderr)
                run, mode = (lambda t=t, xi=xi: t(xi)), "eager"
            for _ in range(2):
                run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / iters
            total_ms += ms
            per.append((type(t).__name__, tuple(xi.shape[1:]), round(ms * 1e3, 1), round(mod_bytes / ms / 1e6 / HBM_PEAK_GBS, 3),
                        round(mod_bytes / (0.22 * HBM_PEAK_GBS * 1e9) * 1e6, 1)))
        # the same ten modules replayed from ONE hipGraph (their launches back to back on the stream): separates the kernels' time from the
        # ~5 us fixed cost every single-module replay above carries (MI355X guide: graph-replay floor)
        one_ms = None
        try:
            g1 = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(g1, capture_error_mode="thread_local"):
                for t, xi in pairs:
                    t(xi)
            for _ in range(2):
                g1.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                g1.replay()
            e1.record()
            torch.cuda.synchronize()
            one_ms = e0.elapsed_time(e1) / iters
        except Exception as e:                              # noqa: BLE001
            print(f"[bench] one-graph capture of the ten modules unavailable ({type(e).__name__}: {e})", file=sys.stderr)
    if was_training:
        model.train()
    esize = 2 if dtype == "bf16" else 4
    b = x.shape[0]
    nbytes = PCONV_RFCBAM_ELEMS_PER_IMG * esize * b + PCONV_RFCBAM_PARAMS * 4
    gbs = nbytes / total_ms / 1e6
    one = {} if one_ms is None else dict(one_graph_ms=round(one_ms, 4), one_graph_hbm_frac=round(nbytes / one_ms / 1e6 / HBM_PEAK_GBS, 4))
    return dict(batch=b, modules=len(targets), ms=round(total_ms, 4), algorithmic_bytes=nbytes, achieved_gbs=round(gbs, 1),
                hbm_frac=round(gbs / HBM_PEAK_GBS, 4), **one, us_per_module=per,
                note="eval forward; every launch of the 6 MLPBlocks + 4 RFCBAMConvs (SE, stats, rfa map, contraction) inside the timed "
                     "region, each module replayed from its own hipGraph (serving mode); one_graph_ms = the ten modules replayed from ONE "
                     "hipGraph (no per-module replay floor); bytes = SURVEY 8(d): in + out once at the storage dtype + fp32 parameters once; "
                     "us_per_module rows = [module, input shape, us per replay, the module's own fraction of HBM, budget_us = what 0.22 of HBM "
                     "(the round's target for the set) allows that module]")


# whole-model block-fused lower bound, lead-yolo-s @640: 85.4 MB per image in fp32 = 21.35 M activation elements in + out
# once per fused block; a training step moves ~3x that (forward, saved activations read back + activation gradients, parameter gradients)
BLOCK_FUSED_ELEMS_PER_IMG = {"s": 21_350_000}

FAMILIES = (("rfcbam", ("ly_rf", "ly_se_", "ly_chan_moments", "ly_colsum")),
            ("wgrad", ("ly_wgrad", "ly_patch4_rows", "ly_patch4_wgrad")),
            ("gemm", ("ly_gemm_kernel",)),
            ("bnact", ("ly_bnact", "ly_bn_")),
            ("mlpblock", ("ly_mlp",)),
            ("conv3x3", ("ly_conv3x3",)),
            ("coordatt", ("ly_coordatt", "ly_pool_hw", "ly_gate")),
            ("loss_optim_pack", ("ly_loss", "ly_optim", "ly_pack", "ly_frag")),
            ("sppf_detect_misc", ("ly_",)))


def family_of(name):
    """kernel name -> the family the step table groups it under (first matching prefix; ATen / memcpy launches are 'aten')"""
    for fam, prefixes in FAMILIES:
        if any(name.startswith(p) for p in prefixes):
            return fam
    return "aten"


def step_families(step_fn, rows):
    """Device time of EVERY launch of one steady-state eager step (torch profiler, device activity — the HIP-event table of probe_step only
    sees the wrappers that carry byte counts), grouped into kernel families; per family: launches, ms, the algorithmic bytes of its
    instrumented launches (rows) and, where profiles/ holds a PMC pass for the kernel, the HBM bytes the counters saw."""
    from torch.profiler import ProfilerActivity, profile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from demangle import demangle, short
    step_fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step_fn()
        torch.cuda.synchronize()
    evs = [ev for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and not ev.name.startswith("Optimizer.")]
    names = demangle([ev.name for ev in evs])
    fam = {}
    for ev, nm in zip(evs, names):
        nm = short(nm) if "ly_" in nm else nm
        f = fam.setdefault(family_of(nm), dict(launches=0, ms=0.0, algorithmic_bytes=0.0, pmc_bytes=0.0, pmc_launches=0))
        f["launches"] += 1
        f["ms"] += ev.device_time / 1e3
        tr = committed_pmc(nm, "pmc_traffic")
        if tr:
            f["pmc_bytes"] += tr["hbm_bytes"]
            f["pmc_launches"] += 1
    for r in rows:
        f = fam.get(family_of(r["kernel"]))
        if f is not None:
            f["algorithmic_bytes"] += r["bytes"] * r["calls_per_step"]
    busy = sum(f["ms"] for f in fam.values())
    out = {}
    for k, f in sorted(fam.items(), key=lambda kv: -kv[1]["ms"]):
        out[k] = dict(launches=f["launches"], ms=round(f["ms"], 4), share=round(f["ms"] / busy, 4),
                      algorithmic_bytes=round(f["algorithmic_bytes"]) or None,
                      pmc_bytes=round(f["pmc_bytes"]) if f["pmc_launches"] else None, pmc_launches=f["pmc_launches"])
    return out, busy, len(evs)


def step_roofline(args, ms_per_step, step_fn, rows):
    """the whole optimisation step against the HBM roof: SURVEY §8(d)'s block-fused bytes (every block reads its input and writes its
    output once; x3 for a training step) / measured step time / 8 TB/s, plus the per-family table that says where the step goes."""
    elems = BLOCK_FUSED_ELEMS_PER_IMG.get(args.scale)
    esize = 2 if args.dtype == "bf16" else 4
    out = dict(ms_per_step=round(ms_per_step, 4))
    if elems is not None and args.size == 640:
        nbytes = elems * esize * args.batch * (3 if args.mode == "train" else 1)
        gbs = nbytes / ms_per_step / 1e6
        out.update(block_fused_bytes=nbytes, achieved_gbs=round(gbs, 1), frac=round(gbs / HBM_PEAK_GBS, 4),
                   bytes_note="SURVEY 8(d): 21.35 M activation elements per image in + out once per fused block at the storage dtype"
                              + (", x3 for a training step (forward, saved tensors + activation gradients, parameter gradients)" if args.mode == "train" else ""))
    try:
        fams, busy, n = step_families(step_fn, rows)
        out.update(kernel_busy_ms=round(busy, 4), launches=n, families=fams,
                   families_note="one steady-state eager step under the torch profiler (device activity): every launch, ATen included; algorithmic_bytes "
                                 "= in + out + parameters once per instrumented launch (ops._Timed); pmc_bytes = 2*FETCH_SIZE + WRITE_SIZE per launch from "
                                 "the committed rocprofv3 --pmc pass (profiles/), summed over the pmc_launches launches it names")
    except Exception as e:                                  # noqa: BLE001
        out["families"] = None
        out["families_note"] = f"profiler pass unavailable: {type(e).__name__}: {e}"
    return out


def _fractions(r, dtype):
    gbs = r["bytes"] / r["ms_per_launch"] / 1e6
    tfs = r["flops"] / r["ms_per_launch"] / 1e9
    vtfs = r.get("valu_flops", 0.0) / r["ms_per_launch"] / 1e9
    mfma_peak = BF16_MFMA_PEAK_TFLOPS if dtype == "bf16" else BF16_MFMA_PEAK_TFLOPS / 3.0
    return gbs, tfs, vtfs, mfma_peak, gbs / HBM_PEAK_GBS, tfs / mfma_peak, vtfs / VALU_F32_PEAK_TFLOPS


def _limited_by(hbm_frac, mfma_frac, valu_frac):
    """the unit with the largest fraction of its peak, or "latency" when none is a quarter busy (derived, not a constant)"""
    best = max((hbm_frac, "hbm"), (mfma_frac, "mfma"), (valu_frac, "valu"))
    return "latency" if best[0] < 0.25 else best[1]


def roofline_of(rows, dtype, families=None, prefer=None):
    """`roofline` of the line, SURVEY 8(d): the DOMINANT kernel = the instrumented kernel with the most time per step (rows are sorted by it: a
    deterministic pick — the "largest kernel of the largest family" of rounds 2-4 flipped between two kernels from run to run), priced against
    the roof 8(d) names for it: HBM for every bf16-storage kernel; for fp32 storage the larger of the HBM and matrix fractions (deep fp32 blocks
    are matrix-bound once fused).  `mfma_frac` / `valu_frac` are side fields; `limited_by` = "latency" when no unit is a quarter busy (such a
    kernel is bound by none of the roofs: occupancy / dependent round trips).  `largest_single_launch` is the same accounting for the longest
    single launch of the step."""
    dom = rows[0]
    picked = "the instrumented kernel with the most time per step (launches x mean launch time)"
    if prefer is not None:
        # train mode: the pick is row 0 of the COMMITTED per-kernel step table (device time per kernel); this run's rows time C-ABI calls — a
        # weight-gradient call is its kernel plus the fold of its slabs — and two kernels within a few per cent of each other (round 6: the
        # BatchNorm / activation reduce pass, 18 x 22 us, and the grouped weight gradient, 8 x 46 us + 8 x 10 us of folds) would swap places
        # between the two accountings
        hit = [r for r in rows if r["kernel"] == prefer[0]]
        if hit:
            dom = hit[0]
            picked = f"row 0 of the committed per-kernel step table {prefer[1]} (most device time per step); the figures are this run's live timing of it"
    dom_family = family_of(dom["kernel"])
    gbs, tfs, vtfs, mfma_peak, hbm_frac, mfma_frac, valu_frac = _fractions(dom, dtype)
    if dtype != "bf16" and mfma_frac > hbm_frac:
        roof = dict(bound="mfma", achieved=round(tfs, 2), peak=round(mfma_peak, 1), unit="TFLOP/s", frac=round(mfma_frac, 4),
                    peak_note="dense bf16 2500 TFLOP/s / 3: fp32-grade products = 3 bf16 MFMAs")
    else:
        roof = dict(bound="hbm", achieved=round(gbs, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(hbm_frac, 4))
    roof["limited_by"] = _limited_by(hbm_frac, mfma_frac, valu_frac)
    tr = committed_pmc(dom["kernel"], "pmc_traffic")
    roof["traffic"] = tr["hbm_bytes"] if tr else None
    roof["traffic_source"] = tr["source"] if tr else None
    roof["traffic_is"] = ("HBM bytes per launch of this kernel from the COMMITTED rocprofv3 --pmc pass named in traffic_source (same command, earlier run): "
                          "counters cannot be collected inside the driver's timed run") if tr else None
    roof["mfma_busy"] = committed_pmc(dom["kernel"], "pmc_mfma")
    roof["kernel"] = dom["kernel"]
    roof["kernel_is"] = picked
    if dom["kernel"].startswith(("ly_wgrad", "ly_mlpblock_bwd")):
        # these C-ABI calls launch the named kernel AND the fixed-order fold of its slabs: the HIP-event pair brackets both (rocprofv3 lists
        # the fold as its own row: ly_wgrad_combine* / ly_mlpblock_bwd*_combine_kernel)
        roof["timed_region"] = "one C-ABI call = the named kernel + the fold launch of its partial tiles (ms_per_launch covers both)"
    roof["kernel_family"] = dom_family
    roof["launches_per_step"] = round(dom["calls_per_step"], 2)
    roof["ms_per_launch"] = round(dom["ms_per_launch"], 5)
    roof["ms_per_step"] = round(dom["ms_per_step"], 4)
    roof["algorithmic_bytes_per_launch"] = round(dom["bytes"])
    roof["algorithmic_mfma_flops_per_launch"] = round(dom["flops"])
    roof["algorithmic_valu_flops_per_launch"] = round(dom.get("valu_flops", 0.0))
    roof["hbm_frac"] = round(hbm_frac, 4)
    roof["mfma_frac"] = round(mfma_frac, 4)
    roof["valu_frac"] = round(valu_frac, 4)
    big = max(rows, key=lambda r: r["ms_per_launch"])
    g2, t2, v2, _, h2, m2, vf2 = _fractions(big, dtype)
    tr2 = committed_pmc(big["kernel"], "pmc_traffic")
    roof["largest_single_launch"] = dict(kernel=big["kernel"], kernel_family=family_of(big["kernel"]), ms_per_launch=round(big["ms_per_launch"], 5),
                                         launches_per_step=round(big["calls_per_step"], 2), algorithmic_bytes_per_launch=round(big["bytes"]),
                                         achieved_gbs=round(g2, 1), hbm_frac=round(h2, 4), mfma_frac=round(m2, 4), valu_frac=round(vf2, 4),
                                         traffic=tr2["hbm_bytes"] if tr2 else None, traffic_source=tr2["source"] if tr2 else None,
                                         limited_by=_limited_by(h2, m2, vf2))
    return roof


def print_layers(rows):
    for r in rows:
        print(f"  {r['kernel']:<58} {r['calls_per_step']:5.1f}/step {r['ms_per_launch'] * 1e3:8.1f} us  {r['ms_per_step'] * 1e3:8.1f} us/step  "
              f"{r['bytes'] / r['ms_per_launch'] / 1e6:8.1f} GB/s  {r['flops'] / r['ms_per_launch'] / 1e9:8.2f} MFMA TFLOP/s  "
              f"{r.get('valu_flops', 0.0) / r['ms_per_launch'] / 1e9:7.2f} VALU TFLOP/s", file=sys.stderr)


DUMP_MAX_BYTES = 64_000_000          # everything --dump-outputs writes, .npy headers included
NPY_HEADER_BYTES = 1024              # per file: np.save writes 128 bytes of header for these shapes


def dump_outputs(out_dir, arrays, max_bytes=DUMP_MAX_BYTES):
    """arrays: name -> tensor.  Writes out_dir/<name>.npy in float32, at most `max_bytes` on disk in all.  Where the data would not fit,
    every array gets a share of the budget proportional to its size and keeps that many elements of its flattened form at sorted positions
    drawn from a generator seeded by the array's size (the same positions for the same shapes from run to run and build to build)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    total = sum(t.numel() for t in arrays.values()) * 4
    budget = max_bytes - NPY_HEADER_BYTES * len(arrays)
    for name, t in arrays.items():
        t = t.detach().float().cpu()
        if total > budget:
            keep = max(1, int(t.numel() * budget // total))
            if keep < t.numel():
                idx = torch.randperm(t.numel(), generator=torch.Generator().manual_seed(t.numel()))[:keep].sort()[0]
                t = t.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), t.numpy())


def train_outputs(model, ema, loss, items):
    """what one optimisation step hands its caller: the loss and loss items it returns and the state it leaves behind (every floating-point
    entry of the model's and the EMA's state dicts, concatenated in state-dict order)"""
    def flat(sd):
        return torch.cat([v.detach().float().reshape(-1) for v in sd.values() if v.is_floating_point()])
    return {"loss": loss.reshape(-1), "loss_items": items.reshape(-1), "model_state": flat(model.state_dict()), "ema_state": flat(ema.ema.state_dict())}


class Ctx:
    pass


def timed_repeats(ctx, step, steps, warmup, repeats):
    """W warm-up steps, then `repeats` timed regions of EXACTLY `steps` steps, each bracketed by barrier + synchronize on
    both sides, MAX over ranks per region; returns the per-region seconds."""
    for _ in range(warmup):
        step()
    out = []
    for _ in range(repeats):
        ctx.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        ctx.barrier()
        dt = time.perf_counter() - t0
        if ctx.dist is not None:
            t = torch.tensor([dt], device=ctx.device, dtype=torch.float64)
            ctx.dist.all_reduce(t, op=ctx.dist.ReduceOp.MAX)
            dt = float(t.item())
        out.append(dt)
    return out


def sustained_run(ctx, step, sec_per_step, seconds=3.0):
    """The same step for ~3 s without a pause (every rank the same count): a second, longer measurement beside the contract's K timed steps —
    and a window in which an outside observer (rocm-smi sampled by the driver) sees the GPU busy: the K-step regions are 0.2 s bursts between
    host-side phases (CPU baseline, graph capture)."""
    n = int(min(max(seconds / max(sec_per_step, 1e-6), 50), 2000))
    ctx.barrier()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    ctx.barrier()
    dt = time.perf_counter() - t0
    if ctx.dist is not None:
        t = torch.tensor([dt], device=ctx.device, dtype=torch.float64)
        ctx.dist.all_reduce(t, op=ctx.dist.ReduceOp.MAX)
        dt = float(t.item())
    return dict(steps=n, seconds=round(dt, 3), ms_per_step=round(dt / n * 1e3, 4))


def run_train(args, ctx):
    import lead_yolo_amd as L
    model = build_model(args.scale, ctx.device, train=True)
    amp = torch.bfloat16 if args.dtype == "bf16" else None       # the autocast region of train.py:316, bf16 instead of fp16
    if ctx.dist is not None:                         # rank 0's parameters and buffers everywhere (train.py:233-235 DDP init)
        for t in list(model.parameters()) + list(model.buffers()):
            ctx.dist.broadcast(t.data, src=0)
    # lr 1e-3, constant: the reference's lr0 = 1e-2 is reached through a warm-up ramp (train.py:295-310); applied from step 0 to ONE synthetic batch
    # it drives the loss from 12 to 3.6 in 100 steps and then back up to a plateau near 10.8 (gpurun_dbg runs, round 5) — the arithmetic per
    # step is the same either way, but `final_loss` of a few hundred steps should say "this trains"
    opt = L.smart_optimizer(model, "SGD", 1e-3, 0.937, 5e-4 * args.batch * ctx.world / 64)
    loss_fn = L.ComputeLoss(model)
    ema = L.ModelEMA(model)                          # SURVEY config 3: "(+EMA)" — train.py:139,331: the EMA update is part of every optimisation step
    reducer = L.GradReducer(list(model.parameters())).attach() if ctx.world > 1 else None
    imgs = synth_u8(args.batch, args.size, ctx.rank).to(ctx.device)
    tg = synth_targets(args.batch, 1 + ctx.rank).to(ctx.device)
    state = {}

    def eager_step():
        state["loss"], state["items"] = L.train_step(model, loss_fn, opt, imgs, tg, ema=ema, reducer=reducer, world_size=ctx.world, amp=amp)

    step, launch = eager_step, "eager launches"
    if not args.no_graph:
        # N = 1: the whole optimisation step replayed from one hipGraph (train.GraphedTrainStep): identical kernels, no host work per
        # step.  N > 1: graph A (forward + backward, bucket-completion event nodes) -> per-bucket RCCL all-reduce released from those events
        # while A is still running -> graph B (fused optimiser); the all-reduce launches are the only eager work.
        try:
            g = L.GraphedTrainStep(model, loss_fn, opt, imgs, tg, ema=ema, amp=amp, warmup=max(args.warmup, 2), reducer=reducer, world_size=ctx.world,
                                   dp_exchange=args.dp_exchange)

            def step():
                state["loss"], state["items"] = g()
            if ctx.world == 1:
                launch = "hipGraph replay of the whole optimisation step"
            elif getattr(g, "_serial", False):
                launch = ("hipGraph A (forward + backward) -> ONE synchronous all-reduce of all gradients "
                          f"({sum(b['flat'].numel() * b['flat'].element_size() for b in reducer.buckets) / 2**20:.1f} MiB, {len(reducer.buckets)} buckets in one "
                          "master buffer) issued from the step's stream -> hipGraph B = fused optimiser dividing by the world size (serial exchange"
                          + (f": timed at construction on {g.dp_probe['ranks']} ranks, {g.dp_probe['serial_ms']} ms per step against "
                             f"{g.dp_probe['overlapped_ms']} ms for the overlapped form)" if g.dp_probe else ", forced)"))
            else:
                launch = ("hipGraph A (forward + backward) with an event-record node where each gradient bucket completes; the bucket's RCCL all-reduce is "
                          "released from that event on a communication stream while A is still executing the rest of backward (overlapped); hipGraph B = fused "
                          f"optimiser dividing by the world size; {len(g._marked)} of {len(reducer.buckets)} buckets released mid-graph"
                          + (f"; timed at construction on {g.dp_probe['ranks']} ranks: {g.dp_probe['overlapped_ms']} ms per step against "
                             f"{g.dp_probe['serial_ms']} ms for the serial form" if g.dp_probe else "; forced"))
        except Exception as e:                                  # noqa: BLE001
            print(f"[bench] hipGraph capture of the train step unavailable ({type(e).__name__}: {e}); timing eager launches", file=sys.stderr)
            step = eager_step

    regions = timed_repeats(ctx, step, args.steps, args.warmup, args.repeats)
    if args.dump_outputs and ctx.rank == 0:
        dump_outputs(args.dump_outputs, train_outputs(model, ema, state["loss"], state["items"]))
    sustained = sustained_run(ctx, step, statistics.median(regions) / args.steps) if args.full and not args.no_sustained else None
    # The drop-in route (`python -m lead_yolo_amd.run train.py`) runs EAGER launches — one ctypes call per kernel from the
    # reference's unchanged Python loop: the same optimisation step without the hipGraph, so that the line says what that route costs
    # (not `value`: the contract's figure is the replayed step above).  Every rank runs it (at N > 1 the eager step exchanges gradients).
    eager_ms = None
    if args.full and step is not eager_step:
        eager_ms = round(statistics.median(timed_repeats(ctx, eager_step, 5, 2, 2)) / 5 * 1e3, 4)
    res = dict(regions=regions, eager_ms_per_step=eager_ms, sustained=sustained, final_loss=float(state["loss"]), peak_mem_gib=round(torch.cuda.max_memory_allocated() / 2**30, 2), model=model, step=eager_step, launch=launch,
               workload=f"lead-yolo-{args.scale} bs={args.batch}/gpu 3x{args.size}x{args.size} {args.dtype} full train step: uint8 batch -> "
                        "train-mode forward (batch-statistics BN), ComputeLoss, HIP backward, clip 10, SGD-nesterov 3 groups, ModelEMA update "
                        "(BASELINE.json configs[2]" + ("" if args.dtype == "bf16" else " shape in fp32") + "); random-init weights",
               parallelism=(f"dp{ctx.world}: one process per GPU, ~2 MB reverse-order gradient buckets (gradients are views into them) "
                            + ("all-reduced over RCCL (torch.distributed 'nccl')" if ctx.backend == "nccl" else
                               f"exchanged over '{ctx.backend}' — FUNCTIONAL DRY RUN of the N > 1 path, not a measurement")) if ctx.world > 1
               else "dp1 (single GPU, no collective)",
               metric="images/sec (640x640) fwd+bwd")
    if reducer is not None:
        res["rccl_ranks"] = ctx.dist.get_world_size()
        res["grad_buckets"] = len(reducer.buckets)
        res["grad_bytes"] = sum(b["flat"].numel() * b["flat"].element_size() for b in reducer.buckets)
        if args.full and step is not eager_step:
            # where in the replayed backward every bucket's all-reduce is released (this rank), and what the step costs beside the
            # forward + backward graph alone: the driver computes scaling from the per-N values, this says WHY a step is longer than N = 1's
            try:
                pr = [g.profile_step() for _ in range(3)][-1]
                if getattr(g, "_serial", False):
                    res["dp_overlap"] = dict(mode="serial", graph_a_ms=round(pr["graph_a_ms"], 4), step_ms=round(pr["step_ms"], 4),
                                             exchange_and_optimizer_tail_ms=round(pr["step_ms"] - pr["graph_a_ms"], 4), bucket_release_pct_of_graph_a=[],
                                             note="rank 0, one profiled step after the timed region: serial exchange — one all-reduce of all gradients on "
                                                  "the step's stream between graph A (forward + backward) and graph B (optimiser); the tail is its whole cost")
                else:
                    res["dp_overlap"] = dict(mode="overlapped", graph_a_ms=round(pr["graph_a_ms"], 4), step_ms=round(pr["step_ms"], 4),
                                         exchange_and_optimizer_tail_ms=round(pr["step_ms"] - pr["graph_a_ms"], 4),
                                         bucket_release_pct_of_graph_a=[dict(bucket=bi, bytes=nb, released_at_pct=pct) for bi, nb, pct in pr["buckets"]],
                                         note="rank 0, one profiled step after the timed region: a bucket's all-reduce is queued on the communication "
                                              "stream behind an event node inside graph A (forward + backward); < 100 % = released while backward was running")
                # both exchange forms as timed at construction over this process group (max over ranks), and which one the step runs
                res["dp_overlap"]["probe"] = g.dp_probe if g.dp_probe else dict(chosen=res["dp_overlap"]["mode"], forced=True)
                res["dp_overlap"]["rccl_ranks"] = ctx.dist.get_world_size()
            except Exception as e:                              # noqa: BLE001
                res["dp_overlap"] = dict(error=f"{type(e).__name__}: {e}")
    return res


def run_forward(args, ctx, batch=None, steps=None, warmup=None, repeats=None):
    import lead_yolo_amd as L
    batch = batch or args.batch
    model = build_model(args.scale, ctx.device)
    x = synth_batch(batch, args.size, ctx.rank, ctx.device)
    if args.dtype == "bf16":
        x = x.to(torch.bfloat16)                       # bf16 input => every module takes its bf16 path (modules.py dtype policy)
    step, launch = (lambda: model(x)), "eager"
    if not args.no_graph:
        try:
            g = L.GraphedForward(model, x)
            with torch.no_grad():
                ref = model(x)
            got = g()
            torch.cuda.synchronize()
            if not all(torch.equal(a, b) for a, b in zip([got[0], *got[1]], [ref[0], *ref[1]])):
                raise RuntimeError("graph replay differs from the eager forward")
            step, launch = g, "hipGraph replay"
        except Exception as e:                                  # noqa: BLE001
            print(f"[bench] hipGraph capture unavailable ({type(e).__name__}: {e}); timing eager launches", file=sys.stderr)
    last = {}

    def timed():
        last["out"] = step()
    with torch.no_grad():
        regions = timed_repeats(ctx, timed, steps or args.steps, args.warmup if warmup is None else warmup, repeats or args.repeats)
    if args.dump_outputs and ctx.rank == 0:
        z, feats = last["out"]
        dump_outputs(args.dump_outputs, {"pred": z, **{f"feat{i}": f for i, f in enumerate(feats)}})
    return dict(regions=regions, model=model, x=x, launch=launch, batch=batch,
                step=lambda: model(x),
                workload=f"lead-yolo-{args.scale} bs={batch}/gpu 3x{args.size}x{args.size} {args.dtype} eval forward (BASELINE.json configs[1]" + ("" if args.dtype == "f32" else " shape in bf16") + "); "
                         "random-init weights, perturbed BN stats",
                parallelism=f"dp{ctx.world} (independent replicas, no data-path collective)", metric="images/sec (640x640) forward")


def launch_ranks(n):
    """this process becomes a launcher: N fresh rank processes through torch.distributed.run.  Nothing here has touched the GPU
    (importing torch does not), so no GPU-initialised process is ever replaced or forked."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=None, help="timed regions of --steps steps each; the line reports their median (default 1, 3 with --full)")
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (default 64 for train, 32 for forward)")
    ap.add_argument("--scale", default="s")
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--dtype", default=None, choices=("f32", "bf16"),
                    help="activation storage / product precision; default: bf16 for the train step (BASELINE.json configs[2]), f32 for --mode forward (configs[1])")
    ap.add_argument("--mode", default="train", choices=("train", "forward"),
                    help="train (default): the BASELINE metric, full optimisation step; forward: eval forward of configs[1]")
    ap.add_argument("--train", action="store_true", help="alias of --mode train")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-sustained", action="store_true", help="skip the ~3 s back-to-back replay after the timed repeats")
    ap.add_argument("--no-secondary", action="store_true", help="skip the secondary eval-forward figure and the pconv_rfcbam probe")
    ap.add_argument("--layers", action="store_true", help="print the per-kernel table to stderr")
    ap.add_argument("--no-roofline", action="store_true", help="skip the per-kernel probe (for whole-step rocprof runs)")
    ap.add_argument("--no-graph", action="store_true", help="time eager launches instead of replaying the captured hipGraph of the step")
    ap.add_argument("--dp-exchange", default="probe", choices=("probe", "serial", "overlapped"),
                    help="N > 1: gradient exchange form of the captured step (probe = time both at construction over the real group, keep the faster)")
    ap.add_argument("--full", action="store_true",
                    help="also every secondary measurement and check: median of 3 timed regions, sustained run, eager step, per-kernel roofline probe, "
                         "step families, pconv_rfcbam probes, secondary forward figures, CPU baseline (the --no-* options switch single ones off)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last timed step as DIR/<name>.npy (float32, at most 64 MB in all)")
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 3 if args.full else 1
    if args.layers and not args.full:
        ap.error("--layers prints the per-kernel table of the roofline probe, which only runs with --full")
    if args.train:
        args.mode = "train"
    if args.batch is None:
        args.batch = 64 if args.mode == "train" else 32
    if args.dtype is None:                       # the precision BASELINE.json quotes each configuration in
        args.dtype = "bf16" if args.mode == "train" else "f32"

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus))
    ctx = Ctx()
    ctx.rank = int(os.environ.get("RANK", 0))
    ctx.local_rank = int(os.environ.get("LOCAL_RANK", 0))
    ctx.world = int(os.environ.get("WORLD_SIZE", 1))
    if ctx.world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={ctx.world}: launch with --nproc-per-node {args.gpus} (or drop the external launcher "
                 f"and let `python bench.py --gpus {args.gpus}` start the ranks itself)")
    ctx.dist = None
    ctx.backend = "nccl"
    if ctx.world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # Functional dry runs of the N > 1 path on a one-GPU box (tests / development, never a measurement): LY_BENCH_ONE_GPU=1 puts every
        # rank on GPU 0 and LY_BENCH_BACKEND=gloo exchanges through the host (RCCL refuses two ranks on one device).
        if os.environ.get("LY_BENCH_ONE_GPU") == "1":
            ctx.local_rank = 0
        ctx.backend = os.environ.get("LY_BENCH_BACKEND", "nccl")
        torch.cuda.set_device(ctx.local_rank)
        if ctx.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", ctx.local_rank))
        else:
            dist.init_process_group(ctx.backend)
        ctx.dist = dist
    ctx.device = torch.device("cuda", ctx.local_rank)
    torch.cuda.set_device(ctx.device)

    def barrier():
        if ctx.dist is not None:
            if ctx.backend == "nccl":
                ctx.dist.barrier(device_ids=[ctx.local_rank])
            else:
                ctx.dist.barrier()
        torch.cuda.synchronize()
    ctx.barrier = barrier

    res = run_train(args, ctx) if args.mode == "train" else run_forward(args, ctx)
    regions = res["regions"]
    dt = statistics.median(regions)
    ms_per_step = dt / args.steps * 1e3
    value = ctx.world * args.batch * args.steps / dt

    # The per-kernel probe replays the EAGER step, which at N > 1 exchanges gradient buckets: every rank must run it (a rank-0-only probe
    # would pair its all-reduces with the other ranks' final barrier).  The table itself is only used on rank 0.
    rows = step_roof = None
    if args.full and not args.no_roofline:
        if args.mode == "train":
            rows = probe_step(res["step"], iters=2)
            step_roof = step_roofline(args, ms_per_step, res["step"], rows)
        else:
            with torch.no_grad():
                rows = probe_step(res["step"], iters=10)
                step_roof = step_roofline(args, ms_per_step, res["step"], rows)
    if ctx.rank == 0:
        out = {
            "metric": res["metric"], "value": round(value, 2), "unit": "images/sec", "n_gpus": ctx.world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": res["workload"], "global_batch": ctx.world * args.batch, "parallelism": res["parallelism"],
                       "arithmetic": ARITH[args.dtype], "world_size": ctx.world},
            "timed_repeats": len(regions), "repeat_ms_per_step": [round(r / args.steps * 1e3, 4) for r in regions],
            "value_is": "median of the timed repeats (each: exactly `steps` steps between barrier+synchronize, max over ranks)",
        }
        if res.get("sustained"):
            out["sustained"] = dict(res["sustained"], value=round(ctx.world * args.batch / res["sustained"]["ms_per_step"] * 1e3, 2), unit="images/sec",
                                    note="the same step replayed back to back for ~3 s after the timed repeats (not `value`: the contract's K steps are)")
        if res.get("eager_ms_per_step") is not None:
            out["eager_ms_per_step"] = res["eager_ms_per_step"]
            out["eager_is"] = ("the same optimisation step as eager launches (no hipGraph; fused HIP optimiser, HIP loss): median of 2 x 5 steps — what the drop-in "
                               "route that keeps the reference's train.py unchanged pays per step in launch overhead; `value` is the replayed step")
        for k in ("final_loss", "peak_mem_gib", "rccl_ranks", "grad_buckets", "grad_bytes", "dp_overlap", "launch"):
            if k in res:
                out[k if k != "launch" else "launch_mode"] = res[k]
        if not args.full or args.no_roofline:
            out["roofline"] = None
            out["cpu_baseline"] = None
        else:
            if args.layers:
                print_layers(rows)
            roof = roofline_of(rows, args.dtype, step_roof.get("families"), committed_row0(args.dtype) if (args.mode == "train" and args.batch == 64 and args.size == 640 and args.scale == "s") else None)
            roof["step"] = step_roof
            if ctx.world == 1 and not args.no_secondary:
                del res["step"]
                if args.mode == "train":
                    xb = synth_batch(args.batch, args.size, 0, ctx.device).to(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
                    model = res.pop("model")
                    roof["pconv_rfcbam_fwd"] = pconv_rfcbam_probe(model, xb, args.dtype)
                    del model, xb
                    torch.cuda.empty_cache()
                    if args.dtype != "f32":                # the 0.70 target is quoted for both storage types: the fp32 sub-metric beside it
                        m32 = build_model(args.scale, ctx.device)
                        roof["pconv_rfcbam_fwd_f32"] = pconv_rfcbam_probe(m32, synth_batch(args.batch, args.size, 0, ctx.device), "f32")
                        del m32
                        torch.cuda.empty_cache()
                    # secondary figure: the eval forward of configs[1] in ITS dtype (fp32), and the same shape in this line's dtype
                    out["forward"] = {}
                    for fdtype in dict.fromkeys(("f32", args.dtype)):
                        fargs = argparse.Namespace(**{**vars(args), "dtype": fdtype, "dump_outputs": None})
                        fw = run_forward(fargs, ctx, batch=32, steps=20, warmup=3, repeats=3)
                        fdt = statistics.median(fw["regions"])
                        out["forward"][fdtype] = {"metric": fw["metric"], "value": round(32 * 20 / fdt, 2), "unit": "images/sec", "ms_per_step": round(fdt / 20 * 1e3, 4),
                                                  "workload": fw["workload"], "launch_mode": fw["launch"]}
                        del fw
                        torch.cuda.empty_cache()
                else:
                    xb = synth_batch(64, args.size, 0, ctx.device).to(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
                    roof["pconv_rfcbam_fwd"] = pconv_rfcbam_probe(res["model"], xb, args.dtype)
            out["roofline"] = roof
            out["cpu_baseline"] = None
            if ctx.world == 1 and not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline_train(args.scale, args.size) if args.mode == "train" else cpu_baseline_forward(args.scale, args.size)
        print(json.dumps(out))
    if ctx.dist is not None:
        ctx.barrier()
        ctx.dist.destroy_process_group()


if __name__ == "__main__":
    main()
