"""Every name an ops.PROFILE record carries is a kernel the device ran: the records of a small training step (bf16 and fp32) and an eval
forward of lead-yolo-s, against torch.profiler's device activity of the same runs (as bench.step_families reads it).  Names are exact."""
import collections
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_profile_records_name_kernels_the_profiler_saw():
    import lead_yolo_amd as L
    from lead_yolo_amd import ops
    from lead_yolo_amd.train import forward_backward
    from torch.profiler import ProfilerActivity, profile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from demangle import demangle, short
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    imgs = torch.randint(0, 256, (2, 3, 64, 64), dtype=torch.uint8, device=dev)
    tg = torch.tensor([[0, 0, 0.5, 0.5, 0.3, 0.3], [1, 0, 0.4, 0.6, 0.2, 0.5]], device=dev)
    model = L.Model(L.load_cfg(scale="s")).to(dev).train()
    loss_fn = L.ComputeLoss(model)

    def runs():
        model.train()
        forward_backward(model, loss_fn, imgs, tg, amp=torch.bfloat16)
        forward_backward(model, loss_fn, imgs, tg)
        model.eval()
        with torch.no_grad():
            model(imgs.float() / 255)

    runs()                                                  # packs, workspaces and LDS caps are set up outside the recorded runs
    torch.cuda.synchronize()
    ops.PROFILE = []
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            runs()
            torch.cuda.synchronize()
    finally:
        recs, ops.PROFILE = ops.PROFILE, None
    seen = collections.Counter(short(nm) for nm in demangle([ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA])
                               if "ly_" in nm)
    labelled = collections.Counter(part for rec in recs for part in rec[0].split(" + "))
    assert len(labelled) > 40 and any(k.startswith("ly_gemm_kernel_d2<float") for k in labelled) and any(k.startswith("ly_gemm_kernel_d2<__bf16") for k in labelled)
    wrong = {k: (n, seen.get(k, 0)) for k, n in labelled.items() if n > seen.get(k, 0)}
    # The profiler hands out names its tracer has already demangled, and that demangler garbles some instantiations with a `__bf16` argument
    # ("ly_bnact_fwd_kernel<__bf16, 1>" arrives as "ly_bnact_fwd_kernel<bool _Accum, int, E>", tools/demangle.py): such a name cannot be compared letter
    # by letter.  What is held for it: the profiler saw garbled launches of that very kernel — same name up to the `__bf16` — at least as many
    # as all such records together.
    garbled = collections.Counter()
    for k, n in seen.items():
        if "bool _Accum" in k:
            garbled[k[:k.index("bool _Accum")]] += n
    unmatched = collections.Counter()
    for k in list(wrong):
        head = k[:k.index("__bf16")] if "__bf16" in k else None
        if head in garbled and seen.get(k, 0) == 0:
            unmatched[head] += wrong.pop(k)[0]
    wrong.update({head + "…": (n, garbled[head]) for head, n in unmatched.items() if n > garbled[head]})
    assert not wrong, f"record name: (records, launches the profiler saw) {wrong}"
