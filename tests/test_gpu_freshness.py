"""Do the HIP modules compute with the weights they hold NOW?

Every module computes from prepared copies of its parameters — packed bf16 fragment images (pack.PLAN), folded BatchNorm tables and
other tables in the per-module `_Prepared` slots, float32 shadows of `.half()` / `.bfloat16()` parameters (pack.master), the tables a
captured graph addresses — kept fresh by torch's per-tensor `_version`, the global pack.EPOCH / pack.W_EPOCH and an address-identity check.
A stale copy gives a finite, plausible, slightly-off result, and a test that loads its weights before the first forward never asks the
caches to notice anything.  Here the weights change AFTER the caches are warm.

The judge is a COLD TWIN: `copy.deepcopy` of the module after the change (`_Prepared.__deepcopy__` gives empty caches, the new
parameter addresses give new PLAN entries), run on the same input.  Same kernels on the same values give the same bits: `torch.equal`,
no tolerance.  The warm module always runs BEFORE the twin exists (PLAN.refresh re-packs every registered image of every model in one
launch: a twin that ran first could repair the module under test).  Every case also asserts its premises: the twin is run twice and
returns the same bits, and the output after the change differs from the output before it.  Once per module the warm output is also held
to the CPU oracle, so that the check is not twin against twin only.

tests/test_freshness_host.py pins the `_version` facts and pack.master's shadow key on the CPU."""
import copy
import gc

import pytest
import torch

from oracle import functional as OF
from oracle import synth
from tests.test_gpu_backward import _close as _close_max
from tests.test_gpu_bf16 import _close as _close_l2
from tests.test_gpu_modules import ATOL, RTOL, _bn_eps, _cfg, _cmp, _ctor, _dev, _load, _oracle
from tests.test_gpu_multiclass import _counted

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
ANCHORS = ((10, 13, 16, 30, 33, 23), (30, 61, 62, 45, 59, 119), (116, 90, 156, 198, 373, 326))
STRIDES = (8.0, 16.0, 32.0)
LEVEL_PX = (5, 3, 2)                                   # Detect levels: s x (s + 1) pixels
SEED_A, SEED_B = 4101, 4202


class Subject:
    """one module kind at the smallest shape its kernels accept.  dts: the storage types its sweep runs in (the first is the one the routes
    use); route: the ops entry point that must be called (the case exercises the path it is named after); no_train: why there is no
    train-mode case."""

    def __init__(self, name, kind, ctor, shape, dts=(F32, BF), route=None, min_units=None, no_train=None):
        self.name, self.kind, self.ctor, self.shape, self.dts = name, kind, ctor, shape, dts
        self.route, self.min_units, self.no_train = route, min_units, no_train

    def setup(self, monkeypatch):
        if self.min_units is not None:                  # RFCBAMConv k = 3 on the matrix cores: lift the size threshold of the dispatch
            from lead_yolo_amd import ops
            monkeypatch.setattr(ops, "RF3M_MIN_UNITS", self.min_units)


def _detect(name, nc, dt, route):
    ch = (64, 128, 256) if dt == F32 else (128, 256, 512)          # as test_detect_level_one_launch_matches_gemm_plus_tail
    return Subject(name, "Detect", (nc, ch), None, (dt,), route)


SUBJECTS = [
    Subject("basicstage_fused", "BasicStage", (24, 1), (1, 24, 9, 7), route="mlpblock"),
    # composed path: bf16 storage needs dim % 32 == 0 (16-byte channel slices), 48 runs in fp32 storage only
    Subject("basicstage_composed", "BasicStage", (48, 1), (2, 48, 5, 7), (F32,)),
    Subject("patchembed", "PatchEmbed_FasterNet", (3, 16, 4, 4), (1, 3, 32, 36)),
    Subject("patchmerge", "PatchMerging_FasterNet", (24, 40, 2, 2), (1, 24, 10, 6)),
    Subject("conv_k1", "Conv", (64, 32, 1, 1), (1, 64, 9, 7)),
    Subject("conv_k3", "Conv", (64, 32, 3, 1), (1, 64, 9, 7)),
    Subject("conv_k3s2", "Conv", (64, 32, 3, 2), (1, 64, 9, 7), no_train="stride 2 is built for inference"),
    Subject("rfcbam_k1", "RFCBAMConv", (160, 256, 1, 1), (1, 160, 8, 8), route="rfcbam_stats"),
    Subject("rfcbam_k3s1", "RFCBAMConv", (32, 48, 3, 1), (2, 32, 9, 70), route="rf3c_fwd"),
    Subject("rfcbam_k3s2", "RFCBAMConv", (64, 64, 3, 2), (1, 64, 21, 13), route="rf3c_fwd"),
    # not in the issue's table: fp32 storage with more than 128 output channels keeps the first-generation lane = pixel kernels, which
    # read tables of their own (wq_stats, wq_main, the 10-slot conv image) that no other case reads
    Subject("rfcbam_k3_pixel", "RFCBAMConv", (64, 256, 3, 2), (1, 64, 9, 7), (F32,), route="rfcbam3"),
    Subject("rfcbam_rf3m", "RFCBAMConv", (128, 128, 3, 2), (2, 128, 16, 16), (BF,), route="rf3m_fwd", min_units=0),
    Subject("coordatt", "CoordAtt", (128, 128, 32), (2, 128, 11, 23)),
    Subject("ca_bottleneck", "CA_Bottleneck", (64, 64, True, 1, 1.0), (2, 64, 17, 9)),
    Subject("c3_ca", "C3_CA", (64, 64, 3, True), (2, 64, 13, 11)),
    Subject("sppf", "SPPF", (160, 160, 5), (1, 160, 6, 6), route="sppf_pool"),
    _detect("detect_nc1", 1, F32, "detect_level"),
    _detect("detect_nc1_bf16", 1, BF, "detect_level"),
    # the issue's table names nc = 3 for the GEMM + tail route, but na * no = 3 * 8 = 24 <= 32 is still the one-launch kernel (with the
    # second weight tile partly used); nc = 6 (na * no = 33) is the first width on the GEMM + ly_detect_tail route.  Both are kept.
    _detect("detect_nc3", 3, F32, "detect_level"),
    _detect("detect_nc3_bf16", 3, BF, "detect_level"),
    _detect("detect_nc6", 6, F32, "detect_tail"),
    _detect("detect_nc6_bf16", 6, BF, "detect_tail"),
]
MODEL = Subject("model_n", "Model", "n", (2, 3, 64, 96))
BY_NAME = {s.name: s for s in SUBJECTS + [MODEL]}
_ids = lambda subs: [s.name for s in subs]


# ---- building blocks ---------------------------------------------------------------------------------------------------------------------
def _new(sub):
    import lead_yolo_amd as L
    torch.manual_seed(0)
    if sub.kind == "Detect":
        det = L.Detect(nc=sub.ctor[0], anchors=ANCHORS, ch=sub.ctor[1])
        det.stride = torch.tensor(STRIDES)
        det.anchors /= det.stride.view(-1, 1, 1)
        return det
    if sub.kind == "Model":
        return L.Model(_cfg(sub.ctor))
    if sub.kind == "Conv":
        return L.Conv(*sub.ctor)
    return _ctor(sub.kind)(*sub.ctor)


def _state(m, seed, anchors_times=1.0):
    st = synth.synth_state(synth.shapes_of(m.state_dict()), seed)
    for k in st:
        if k.endswith("anchors"):
            st[k] = dict(m.named_buffers())[k].detach().cpu().float().clone() * anchors_times
    return st


def _make(sub, seed=SEED_A):
    """the module on the device, eval mode, state `seed` loaded BEFORE its first forward"""
    m = _new(sub)
    _bn_eps(_load(m, _state(m, seed)))
    return m.to(_dev()).eval()


def _input(sub, dt, seed=7):
    dev = _dev()
    if sub.kind == "Detect":
        return [synth.synth_input((2, c, s, s + 1), seed + i).to(dev).to(dt).contiguous(memory_format=torch.channels_last)
                for i, (c, s) in enumerate(zip(sub.ctor[1], LEVEL_PX))]
    if sub.kind == "Model":
        n, _, h, w = sub.shape
        return (synth.synth_images(n, max(h, w), seed)[:, :, :h, :w].float() / 255).to(dev).to(dt)
    return synth.synth_input(sub.shape, seed).to(dev).to(dt)


def _flat(y):
    if isinstance(y, torch.Tensor):
        return (y,)
    return tuple(t for part in y for t in _flat(part))


def _fwd(m, x):
    with torch.no_grad():
        return _flat(m(list(x) if isinstance(x, list) else x))


def _diff(a, b):
    """None when the two output tuples hold the same bits, else a description of the first difference"""
    if len(a) != len(b):
        return f"{len(a)} vs {len(b)} outputs"
    for i, (s, t) in enumerate(zip(a, b)):
        if s.dtype != t.dtype or s.shape != t.shape:
            return f"output {i}: {s.dtype} {tuple(s.shape)} vs {t.dtype} {tuple(t.shape)}"
        if not torch.equal(s, t):
            d = (s.double() - t.double()).abs()
            return f"output {i}: {int((d > 0).sum())} / {d.numel()} elements differ, max {float(d.max()):.3e} (scale {float(t.double().abs().max()):.3e})"
    return None


def _live(m):
    """name -> the live floating tensor of every state_dict entry (parameters, running statistics, Detect.anchors)"""
    live = {**dict(m.named_parameters()), **dict(m.named_buffers())}
    return {k: live[k] for k, v in m.state_dict().items() if v.is_floating_point()}


def _findings(after, before, twin, x, what, expect_change=True):
    """the warm module's output `after` against the cold `twin` -> list of findings; the twin runs twice (premise: same bits)"""
    t1, t2 = _fwd(twin, x), _fwd(twin, x)
    assert all(bool(torch.isfinite(t).all()) for t in t1), f"{what}: the cold twin's output is not finite"
    bad = []
    d = _diff(t1, t2)
    if d:
        bad.append(f"{what}: PREMISE, two runs of the cold twin differ: {d}")
    if expect_change and before is not None and _diff(after, before) is None:
        bad.append(f"{what}: PREMISE, the change did not reach the output")
    d = _diff(after, t1)
    if d:
        bad.append(f"{what}: STALE, the warm module differs from its cold twin: {d}")
    return bad


def _judge(m, x, before, what, expect_change=True):
    """the warm module `m` after its change against a cold twin -> (output of m, list of findings).  `m` runs FIRST."""
    after = _fwd(m, x)
    return after, _findings(after, before, copy.deepcopy(m), x, what, expect_change)


def _vs_oracle(sub, m, x, got, what):
    """the warm output against the CPU oracle on the state the module holds now (fp32 storage: _cmp's band, bf16 storage: the bf16 module
    bound of tests/test_gpu_bf16.py; the whole model in bf16: its bound there, 5x / 8x)"""
    st = {k: (v.detach().float().cpu().clone() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in m.state_dict().items()}
    with torch.no_grad():
        if sub.kind == "Detect":
            want = _flat(OF.detect(st, "", [t.float().cpu() for t in x], torch.tensor(STRIDES), sub.ctor[0]))
        elif sub.kind == "Model":
            want = _flat(OF.model_forward(st, _cfg(sub.ctor), x.float().cpu(), torch.tensor(STRIDES), training=False))
        else:
            want = (_oracle(sub.kind, list(sub.ctor), st, x.float().cpu()),)
    assert len(want) == len(got)
    bf16 = (x[0] if isinstance(x, list) else x).dtype == BF
    for i, (g, w) in enumerate(zip(got, want)):
        if not bf16:
            _cmp(g, w, f"{what} output {i} vs oracle")
        elif sub.kind == "Model":
            _close_l2(g, w, f"{what} output {i} vs oracle", rel=5 * 8 * 2.0 ** -8, mx=8 * 2.0 ** -4)
        else:
            _close_l2(g, w, f"{what} output {i} vs oracle")
    return want


def _report(problems):
    assert not problems, "\n".join(problems)


# ---- the subjects take the paths they are named after ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", [s for s in SUBJECTS if s.route], ids=_ids([s for s in SUBJECTS if s.route]))
def test_subject_takes_its_route(sub, monkeypatch):
    sub.setup(monkeypatch)
    m = _make(sub)
    names = ("mlpblock", "rfcbam_stats", "rf3c_fwd", "rfcbam3", "rf3m_fwd", "sppf_pool", "detect_level", "detect_tail")
    with _counted(*names) as n:
        _fwd(m, _input(sub, sub.dts[0]))
    assert n[sub.route] > 0, (sub.name, n)
    exclusive = {"rf3c_fwd": ("rfcbam3", "rf3m_fwd"), "rfcbam3": ("rf3c_fwd", "rf3m_fwd"),
                 "rf3m_fwd": ("rf3c_fwd", "rfcbam3"), "detect_level": ("detect_tail",), "detect_tail": ("detect_level",)}
    assert all(n[k] == 0 for k in exclusive.get(sub.route, ())), (sub.name, n)


# ---- a. per-tensor sweep, eval mode -------------------------------------------------------------------------------------------------------
def _eval_sweep(sub, dts, monkeypatch):
    """every floating state_dict entry, one at a time: warm forward(s), in-place change under no_grad, forward(s), cold twin; then the
    tensor is put back, which must give the bits of the forward before the change.  With two storage types both `_Prepared` variants
    are warm before the change and both are checked after it."""
    sub.setup(monkeypatch)
    m = _make(sub)
    xs = {dt: _input(sub, dt) for dt in dts}
    live = _live(m)
    problems, after, prev = [], None, None
    for key, t in live.items():
        if prev is not None:                                         # put the previous tensor back: every change is probed at the state loaded at
            with torch.no_grad():                                    # the start (changes that pile up saturate C3_CA's gates within three bottlenecks)
                prev[1].copy_(prev[2])
            for dt in dts:                                           # the same values as two forwards ago: the same bits, or something is stale
                d = _diff(_fwd(m, xs[dt]), before[dt])
                if d:
                    problems.append(f"{sub.name} {str(dt)[6:]} {prev[0]}: STALE after the tensor was put back: {d}")
        before = {dt: _fwd(m, xs[dt]) for dt in dts}
        prev = (key, t, t.detach().clone())
        with torch.no_grad():
            t.mul_(1.25)
            if not key.endswith("anchors"):
                t.add_(0.05)
        after = {dt: _fwd(m, xs[dt]) for dt in dts}                  # the warm module first, in every variant
        twin = copy.deepcopy(m)
        for dt in dts:
            problems += _findings(after[dt], before[dt], twin, xs[dt], f"{sub.name} {str(dt)[6:]} {key}")
    print(f"FRESHNESS eval sweep {sub.name} [{', '.join(str(dt)[6:] for dt in dts)}]: {len(live)} state tensors")
    _report(problems)
    for dt in dts:                                                   # once per module, after the last change: not twin against twin only
        _vs_oracle(sub, m, xs[dt], after[dt], f"{sub.name} {str(dt)[6:]} after the sweep")


EVAL_CASES = [(s, dt) for s in SUBJECTS for dt in s.dts]


@pytest.mark.parametrize("sub,dt", EVAL_CASES, ids=[f"{s.name}-{str(dt)[6:]}" for s, dt in EVAL_CASES])
def test_eval_sweep_every_state_tensor(sub, dt, monkeypatch):
    _eval_sweep(sub, (dt,), monkeypatch)


BOTH = [s for s in SUBJECTS if s.dts == (F32, BF) and s.name in ("basicstage_fused", "patchmerge", "conv_k3", "rfcbam_k3s2", "c3_ca")]


@pytest.mark.parametrize("sub", BOTH, ids=_ids(BOTH))
def test_eval_sweep_both_storage_variants_warm(sub, monkeypatch):
    """the `_Prepared` slots are per `variant` (2 weight planes for fp32 storage, 1 for bf16): both are warm before each change, and each
    must refresh on its own"""
    _eval_sweep(sub, (F32, BF), monkeypatch)


# ---- b. per-parameter sweep, train mode ---------------------------------------------------------------------------------------------------
def _fwd_bwd(m, x, dys=None):
    """train-mode forward and one backward of a fixed cotangent -> (outputs, input gradients, cotangents); an image input (3 channels)
    takes no gradient.  bf16 storage as tests/test_gpu_bf16.py trains: bf16 input (an image stays fp32) under autocast, fp32 parameters."""
    xs = x if isinstance(x, list) else [x]
    bf16 = any(t.dtype == BF for t in xs) or getattr(m, "_freshness_autocast", False)
    leaves = [t.detach().clone(memory_format=torch.preserve_format).requires_grad_(t.shape[1] != 3) for t in xs]
    for p in m.parameters():
        p.grad = None
    with torch.autocast("cuda", dtype=BF, enabled=bf16):
        outs = _flat(m(list(leaves) if isinstance(x, list) else leaves[0]))
    if dys is None:
        dys = [synth.synth_input(tuple(o.shape), 50 + i).to(o.device).to(o.dtype) for i, o in enumerate(outs)]
    if any(t.requires_grad for t in leaves):
        torch.autograd.backward(list(outs), list(dys))
    return tuple(o.detach() for o in outs), tuple(t.grad for t in leaves if t.requires_grad), dys


def _mean_free(m, key):
    """a convolution bias in front of a train-mode BatchNorm (RFCBAMConv.conv[0], CoordAtt.conv1): the batch statistics remove a
    per-channel constant, its value cannot reach the training output — the one change exempt from the `reached the output` premise"""
    import lead_yolo_amd as L
    owner, _, leaf = key.rpartition(".")
    if leaf != "bias":
        return False
    holder, _, name = owner.rpartition(".")
    parent = m.get_submodule(holder) if holder else m
    if isinstance(parent, L.CoordAtt):
        return name == "conv1"
    if name == "0" and holder.rpartition(".")[2] == "conv":                  # <RFCBAMConv>.conv.0.bias
        top = holder.rpartition(".")[0]
        return isinstance(m.get_submodule(top) if top else m, L.RFCBAMConv)
    return False


TRAIN_CASES = [(s, dt, still) for s in SUBJECTS if s.no_train is None for dt in s.dts for still in (False, True)]


@pytest.mark.parametrize("sub,dt,epoch_still", TRAIN_CASES,
                         ids=[f"{s.name}-{str(dt)[6:]}" + ("-epoch_still" if still else "") for s, dt, still in TRAIN_CASES])
def test_train_sweep_every_parameter(sub, dt, epoch_still, monkeypatch):
    """train mode, fp32 and bf16 storage: the output and the input gradient dx of one backward after each parameter's change, against the
    cold twin; then the parameter is put back, which must give the bits of the step before.  dx reads the transposed / flipped weight
    images, which PLAN keeps apart from the forward's.  Running statistics do not enter a training forward and stay as they are.

    A training forward through a tracked BatchNorm calls pack.touch(), and pack.versions() ends every `_Prepared` key with that epoch: as
    the package runs, every slot of a module with a BatchNorm is rebuilt on every training forward whatever its key lists, and what this
    sweep then holds to account is PLAN's per-source version compare.  epoch_still: the same sweep with pack.touch() silenced, so that
    the keys themselves (`_packed_train`'s deliberately partial one among them) have to notice the parameter.  Withholding the signal is
    sound here because it only says that running statistics moved, which no training forward reads; the eval check at the end, which
    does read them, runs in the other variant only.

    Should dx of some module not be the same bits in two runs of the twin, it is held to a band instead and a FRESHNESS line says so:
    fp32 storage the band of test_module_backward_shapes_vs_oracle (1e-3 of the gradient's largest magnitude), bf16 storage 2^-7 of it
    (one bf16 rounding of an element is 2^-9 relative; a summation-order difference moves an element by at most a few of them)."""
    from lead_yolo_amd import pack
    sub.setup(monkeypatch)
    m = _make(sub)
    x = _input(sub, dt)
    if dt == BF and sub.kind != "Detect" and sub.shape[1] == 3:
        x = x.float()                                              # the image stays fp32, the patch gather writes bf16 under autocast
        m._freshness_autocast = True
    ev0 = _fwd(m, x)                                               # eval caches warm: the running statistics will move under them
    m.train()
    if epoch_still:
        monkeypatch.setattr(pack, "touch", lambda: None)
    params = dict(m.named_parameters())
    problems, loose = [], set()
    dys, prev = None, None
    for key, p in params.items():
        if prev is not None:                                       # put the previous parameter back: the bits of the step before its change
            with torch.no_grad():
                prev[1].copy_(prev[2])
            yr, dxr, _ = _fwd_bwd(m, x, dys)
            d = _diff(yr, y0) or (_diff(dxr, dx0) if prev[0] not in loose else None)
            if d:
                problems.append(f"{sub.name} train {prev[0]}: STALE after the parameter was put back: {d}")
        y0, dx0, dys = _fwd_bwd(m, x, dys)
        prev = (key, p, p.detach().clone())
        with torch.no_grad():
            p.mul_(1.25).add_(0.05)
        y1, dx1, _ = _fwd_bwd(m, x, dys)                           # the warm module first
        twin = copy.deepcopy(m)
        (ya, dxa, _), (yb, dxb, _) = _fwd_bwd(twin, x, dys), _fwd_bwd(twin, x, dys)
        what = f"{sub.name} train {key}"
        assert all(bool(torch.isfinite(v).all()) for v in ya + dxa), f"{what}: the cold twin's output or dx is not finite"
        d = _diff(ya, yb)
        if d:
            problems.append(f"{what}: PREMISE, two forwards of the cold twin differ: {d}")
        if not _mean_free(m, key) and _diff(y1 + dx1, y0 + dx0) is None:
            problems.append(f"{what}: PREMISE, the change reached neither the output nor dx")
        d = _diff(y1, ya)
        if d:
            problems.append(f"{what}: STALE forward, the warm module differs from its cold twin: {d}")
        if _diff(dxa, dxb) is None:
            d = _diff(dx1, dxa)
            if d:
                problems.append(f"{what}: STALE backward, dx of the warm module differs from its cold twin's: {d}")
        else:
            loose.add(key)
            for i, (g, w) in enumerate(zip(dx1, dxa)):
                _close_max(g, w, f"{what} dx {i} (twin dx not bit-stable: band)", rtol=1e-3 if dt == F32 else 2.0 ** -7)
    print(f"FRESHNESS train sweep {sub.name} {str(dt)[6:]}{' epoch still' if epoch_still else ''}: {len(params)} parameters"
          + (f"; dx of the twin not bit-stable for {sorted(loose)}" if loose else ""))
    _report(problems)
    if not epoch_still:
        m.eval()
        _, bad = _judge(m, x, ev0, f"{sub.name} eval after the training forwards")
        _report(bad)


# ---- c. routes: all tensors from state A to state B ------------------------------------------------------------------------------------
ROUTES = ["load_state_dict", "no_grad_copy", "detach_copy", "data_copy_touch", "bf16_copy", "bf16_data_copy_touch", "bf16_float_round_trip",
          "sgd_step"]


def _route(route, m, B):
    """move every floating tensor of m to state B (on m's device) by one route; sgd_step moves the parameters only"""
    from lead_yolo_amd import pack
    live = _live(m)
    if route == "load_state_dict":
        m.load_state_dict(B)
    elif route in ("no_grad_copy", "bf16_copy"):
        with torch.no_grad():
            for k, t in live.items():
                t.copy_(B[k])
    elif route == "detach_copy":
        for k, t in live.items():
            t.detach().copy_(B[k])
    elif route in ("data_copy_touch", "bf16_data_copy_touch"):
        for k, t in live.items():
            t.data.copy_(B[k])
        pack.touch_weights()                                         # the documented contract for writes that move no version counter
    elif route == "sgd_step":
        opt = torch.optim.SGD(m.parameters(), lr=1.0)
        for k, p in m.named_parameters():
            p.grad = p.detach() - B[k]
        opt.step()
    else:
        raise ValueError(route)


def _route_case(sub, route, monkeypatch, graph=False):
    """-> nothing; graph: also GraphedForward's staleness report and a graph built anew (whole model)"""
    import lead_yolo_amd as L
    sub.setup(monkeypatch)
    m = _make(sub, SEED_A)
    B = {k: v.to(_dev()) for k, v in _state(m, SEED_B, anchors_times=1.25).items()}
    dt0 = sub.dts[0]
    dtb = BF if BF in sub.dts else F32                               # `.bfloat16()` parameters: bf16 storage where the module has it, else fp32 kernels on the shadows
    what = f"{sub.name} {route}"
    g = None
    if route == "bf16_float_round_trip":
        x = _input(sub, dt0)
        before = _fwd(m, x)
        if graph:
            g = L.GraphedForward(m, x)
        m.bfloat16()
        _fwd(m, _input(sub, dtb))                                    # the shadows and the bf16 variant are warm too
        m.float()
    else:
        if route.startswith("bf16"):
            m.bfloat16()
        x = _input(sub, dtb if route.startswith("bf16") else dt0)
        before = _fwd(m, x)
        if graph:
            g = L.GraphedForward(m, x)
            assert not g.stale()
            z0 = tuple(t.clone() for t in _flat(g()))
            _flat(g(x))
            torch.cuda.synchronize()
            assert not g.stale(), "replays must not look like weight changes"
            assert _diff(z0, before) is None
        _route(route, m, B)
    if g is not None:
        assert g.stale(), f"{what}: GraphedForward did not notice the weight change"
    # rounding the weights to bf16 and back: in bf16 storage the single-plane images hold the same bf16 values as before
    after, bad = _judge(m, x, before, what, expect_change=not (route == "bf16_float_round_trip" and dt0 == BF))
    _report(bad)
    if graph:
        g2 = L.GraphedForward(m, x)
        got = _flat(g2(x))
        torch.cuda.synchronize()
        assert _diff(got, after) is None, f"{what}: a GraphedForward built after the change differs from the eager forward: {_diff(got, after)}"
        assert not g2.stale()
    return m, x, after


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("sub", SUBJECTS, ids=_ids(SUBJECTS))
def test_route_every_module_kind(sub, route, monkeypatch):
    _route_case(sub, route, monkeypatch)


@pytest.mark.parametrize("route", ROUTES)
def test_route_whole_model_and_graphed_forward(route, monkeypatch):
    """lead-yolo-n, 64 x 96, batch 2: the eager forward after each route against the cold twin; a GraphedForward captured BEFORE the
    change reports stale() (its replays still read the tables of the capture), one built after it returns the eager forward's bits.
    One fp32 route and one bf16-parameter route are also held to the oracle on state B."""
    m, x, after = _route_case(MODEL, route, monkeypatch, graph=True)
    if route in ("load_state_dict", "bf16_data_copy_touch"):
        _vs_oracle(MODEL, m, x, after, f"model_n {route}")


def test_detect_bf16_parameters_vs_oracle():
    """`.bfloat16()` converts Detect.anchors with the parameters; the decode kernels read float32 anchors (they used to be handed the
    bf16 buffer as it was).  z and the raw maps of a `.bfloat16()` head against the oracle on the bf16-rounded state."""
    sub = BY_NAME["detect_nc1_bf16"]
    m = _make(sub).bfloat16()
    assert m.anchors.dtype == BF
    x = _input(sub, BF)
    _vs_oracle(sub, m, x, _fwd(m, x), "detect_nc1 .bfloat16()")


# ---- d. raw-pointer writers, whole model ---------------------------------------------------------------------------------------------
def _model_and_graph():
    import lead_yolo_amd as L
    m = _make(MODEL)
    x = _input(MODEL, F32)
    before = _fwd(m, x)
    g = L.GraphedForward(m, x)
    assert not g.stale()
    return m, x, before, g


def _fresh_graph_matches(m, x, after, what):
    import lead_yolo_amd as L
    g2 = L.GraphedForward(m, x)
    got = _flat(g2(x))
    torch.cuda.synchronize()
    assert _diff(got, after) is None, f"{what}: a GraphedForward built after the change differs from the eager forward: {_diff(got, after)}"


@pytest.mark.parametrize("name", ["SGD", "AdamW"])
def test_fused_optimizer_step_with_ema(name, monkeypatch):
    """optim.FusedSGD / FusedAdamW with attach_ema write parameters AND the EMA copy through raw pointers: the eval forward of the trained
    model and of ema.ema follow, and a GraphedForward of either is reported stale"""
    import lead_yolo_amd as L
    from lead_yolo_amd import ops
    monkeypatch.setattr(ops, "SINK", ops.SINK)                     # the first fused step installs its gradient sink: put back afterwards
    m, x, before, g = _model_and_graph()
    ema = L.ModelEMA(m)
    before_e = _fwd(ema.ema, x)
    ge = L.GraphedForward(ema.ema, x)
    opt = L.smart_optimizer(m, name, 0.01, 0.937, 5e-4, fused=True)
    assert isinstance(opt, L.FusedSGD if name == "SGD" else L.FusedAdamW)
    opt.attach_ema(ema, m)
    gen = torch.Generator().manual_seed(3)
    for p in m.parameters():
        p.grad = (torch.randn(p.shape, generator=gen) * 0.1).to(_dev())
    opt.step()
    assert g.stale() and ge.stale()
    after, bad = _judge(m, x, before, f"model_n after Fused{name}.step")
    after_e, bad_e = _judge(ema.ema, x, before_e, f"ema of model_n after Fused{name}.step")
    _report(bad + bad_e)
    _fresh_graph_matches(m, x, after, f"Fused{name}.step")
    _fresh_graph_matches(ema.ema, x, after_e, f"Fused{name}.step, ema")


def test_eval_after_train_mode_forward():
    """a train-mode forward writes the running statistics through ly_bn_finalize (no version counter moves): the eval forward follows"""
    m, x, before, g = _model_and_graph()
    m.train()
    with torch.no_grad():
        m(x)
    m.eval()
    assert g.stale()
    after, bad = _judge(m, x, before, "model_n eval after a train-mode forward")
    _report(bad)
    _fresh_graph_matches(m, x, after, "train-mode forward")


def test_eval_after_graphed_train_step_replay(monkeypatch):
    """one replay of the captured optimisation step (parameters, running statistics and the EMA written by the graph's kernels)"""
    import lead_yolo_amd as L
    from lead_yolo_amd import ops
    monkeypatch.setattr(ops, "SINK", ops.SINK)
    m = _make(MODEL).train()
    opt = L.smart_optimizer(m, "SGD", 0.01, 0.937, 5e-4)
    ema = L.ModelEMA(m)
    cl = L.ComputeLoss(m)
    imgs = [synth.synth_images(2, 64, 21 + i).to(_dev()) for i in range(2)]
    tgs = [synth.synth_targets(2, 31 + i, per_image=3).to(_dev()) for i in range(2)]
    step = L.GraphedTrainStep(m, cl, opt, imgs[0], tgs[0], ema=ema, warmup=2)
    x = _input(MODEL, F32)
    m.eval()
    before, before_e = _fwd(m, x), _fwd(ema.ema, x)                 # eval caches warm after the capture
    g = L.GraphedForward(m, x)
    m.train()
    step(imgs[1], tgs[1])
    m.eval()
    assert g.stale()
    after, bad = _judge(m, x, before, "model_n eval after a GraphedTrainStep replay")
    _, bad_e = _judge(ema.ema, x, before_e, "ema of model_n after a GraphedTrainStep replay")
    _report(bad + bad_e)
    _fresh_graph_matches(m, x, after, "GraphedTrainStep replay")


# ---- e. address reuse ---------------------------------------------------------------------------------------------------------------------
def test_address_reuse_by_a_second_model():
    """a model dies and the allocator hands its parameters' addresses to the next one of the same architecture: PLAN's entries are keyed
    by address and layout, so only the identity check in `_Plan.get` stands between the new model and the dead one's images.  The twin
    cannot judge this (it gets other addresses): the oracle does, and states A and B are far enough apart that an image of A cannot pass."""
    x = _input(MODEL, F32)
    ptrs, wants = [], []
    for seed in (SEED_A, SEED_B):
        m = _make(MODEL, seed)
        ptrs.append(next(iter(m.parameters())).data_ptr())
        got = _fwd(m, x)
        wants.append(_vs_oracle(MODEL, m, x, got, f"model_n state {seed}"))
        del m, got
        gc.collect()
    a, b = (torch.cat([t.reshape(-1) for t in w]) for w in wants)
    far = ((a - b).abs() > 10 * (ATOL + RTOL * b.abs())).float().mean()
    assert float(far) > 0.5, f"states A and B are too close for this case to tell them apart ({float(far):.2f} of the elements differ by 10 bands)"
    print(f"FRESHNESS address reuse: first weight at {ptrs[0]:#x} then {ptrs[1]:#x}: "
          + ("reused" if ptrs[0] == ptrs[1] else "NOT reused, the case did not exercise the identity check"))


def test_address_reuse_forced():
    """the same, with the reuse made certain: model B takes over the very storage of model A's tensors after A died (what the allocator
    does when it hands the addresses back), filled with state B before B's first forward.  B is on the device before A's last forward,
    so no conversion, no version counter and no epoch moves between A's images and B's first request: only the identity check in
    `_Plan.get` can tell that the images registered at these addresses belong to a dead model."""
    x = _input(MODEL, F32)
    mb = _make(MODEL, SEED_B)
    sb = {k: v.detach().clone() for k, v in _live(mb).items()}
    ma = _make(MODEL, SEED_A)
    _vs_oracle(MODEL, ma, x, _fwd(ma, x), "model_n state A")
    keep = {k: t.data for k, t in _live(ma).items()}                # aliases: the storage outlives the model, the parameters do not
    del ma
    gc.collect()
    for k, t in _live(mb).items():
        keep[k].copy_(sb[k])
        t.data = keep[k]
        assert t.data_ptr() == keep[k].data_ptr()
    _vs_oracle(MODEL, mb, x, _fwd(mb, x), "model_n state B in the storage of A")


# ---- f. GraphedForward -----------------------------------------------------------------------------------------------------------------
def test_graphed_forward_not_stale_after_capture_and_replays():
    m, x, before, g = _model_and_graph()
    for seed in (8, 9, 7):
        xi = _input(MODEL, F32, seed)
        got = tuple(t.clone() for t in _flat(g(xi)))
        torch.cuda.synchronize()
        assert not g.stale()
        assert _diff(got, _fwd(m, xi)) is None
    assert _diff(got, before) is None
