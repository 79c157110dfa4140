"""Every described C-ABI call of ONE eager training step of lead-yolo-s (bs=64, 640x640), one JSON line per call: the describe entry's name
and its arguments — struct fields by name, scalars as they are, every pointer reduced to 0 (null) or 0x1000 + its low four bits (nullness
and alignment are all a describe entry reads of a pointer).  tests/test_describe_host.py replays the committed output on the host.
    python tools/step_calls.py [bf16|f32] [bs] > profiles/<tag>_step_calls.jsonl"""
import ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench as B
import lead_yolo_amd as L
from lead_yolo_amd import capi, ops

dev = torch.device("cuda:0")
amp = torch.bfloat16 if (len(sys.argv) < 2 or sys.argv[1] == "bf16") else None
bs = int(sys.argv[2]) if len(sys.argv) > 2 else 64
model = B.build_model("s", dev, train=True)
opt = L.smart_optimizer(model, "SGD", 0.01, 0.937, 5e-4, fused=True)
cl = L.ComputeLoss(model)
imgs = B.synth_u8(bs, 640, 0).to(dev)
tg = B.synth_targets(bs, 1).to(dev)
for _ in range(3):
    L.train_step(model, cl, opt, imgs, tg, amp=amp)
torch.cuda.synchronize()


def ptr(v):
    v = v.value if isinstance(v, ctypes.c_void_p) else v
    return 0 if not v else 0x1000 + (int(v) & 15)


def struct(s):
    return {"struct": type(s).__name__,
            "fields": {f: ptr(getattr(s, f)) if t is ctypes.c_void_p else getattr(s, f) for f, t in s._fields_}}


def arg(a, ctype):
    obj = getattr(a, "_obj", a)                            # byref(struct) -> the struct
    if isinstance(obj, ctypes.Structure):
        return struct(obj)
    if isinstance(obj, ctypes.Array):
        return [struct(s) for s in obj]
    return ptr(a) if ctype is ctypes.c_void_p else a


CALLS = []
_label = ops._label


def label(describe, *args):
    CALLS.append({"fn": describe, "args": [arg(a, t) for a, t in zip(args, capi.SIGNATURES[describe])]})
    return _label(describe, *args)


ops._label = label
ops.PROFILE = []
L.train_step(model, cl, opt, imgs, tg, amp=amp)
torch.cuda.synchronize()
ops.PROFILE, ops._label = None, _label
for c in CALLS:
    print(json.dumps(c))
print(f"{len(CALLS)} described calls", file=sys.stderr)
