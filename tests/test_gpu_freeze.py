"""Training with frozen parameters on the device (the reference's `--freeze N`: requires_grad = False, model left in .train(), so frozen
BatchNorms keep using and updating batch statistics): every module and the whole step under every mask that splits what the kernels treat
together — input without parameters, parameters without input, BatchNorm affine against weights, every second parameter (cv1 / cv2 pairs,
gamma / beta, the SE and get_weight weights) — with and without the optimiser's gradient sink, and the mask changing between steps.

References (tests/test_freeze_host.py asserts their premises on the CPU): autograd through the oracle — the gradient of a trainable parameter
does not depend on which others are frozen, so the oracle's full gradient restricted to the trainable set serves every mask — and the same
HIP module run with nothing frozen: its forward and running statistics must be the same BITS (the forward does not read requires_grad), so
no ReLU / arg-max decision differs and the trainable gradients may differ by summation order only.
Bounds are the suite's: test_gpu_backward._close (1e-3 of the tensor's largest magnitude) in fp32, the bounds at the top of
tests/test_gpu_bf16.py in bf16, the whole-model and per-step loss bounds of test_whole_model_gradients_vs_oracle and
test_training_trajectory_vs_oracle."""
import copy
import functools

import pytest
import torch

from oracle import synth
from tests import test_freeze_host as H
from tests.test_gpu_backward import RTOL, _close, _floor, _one_rank_group, _oracle_grads
from tests.test_gpu_bf16 import BF, MAX_REL, REL_L2
from tests.test_gpu_modules import _bn_eps, _ctor, _dev, _load
from tests.test_oracle_golden import _run

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_sink_left_behind(monkeypatch):
    """every test starts without a gradient sink (a fused optimiser's first step installs one process-wide) and puts back what it found"""
    from lead_yolo_amd import ops
    monkeypatch.setattr(ops, "SINK", None)


# ---- module level ---------------------------------------------------------------------------------------------------------------------
MASKS = ("params-only", "affine-frozen", "weights-frozen", "alternate", "alternate-odd", "input-only")

FP32_CASES = [
    ("BasicStage", (24, 1), (2, 24, 40, 36)),
    ("BasicStage", (160, 1), (2, 160, 20, 20)),                 # the mlpblock_bwd_dx tail
    ("BasicStage", (48, 2), (2, 48, 17, 13)),                   # the composed path
    ("PatchEmbed_FasterNet", (3, 24, 4, 4), (2, 3, 64, 96)),    # reads the image: parameter masks only
    ("PatchMerging_FasterNet", (40, 80, 2, 2), (2, 40, 24, 20)),
    ("CoordAtt", (128, 128, 32), (2, 128, 11, 23)),
    ("CA_Bottleneck", (64, 64, True, 1, 1.0), (2, 64, 17, 9)),
    ("C3_CA", (64, 64, 3, True), (2, 64, 13, 11)),
    ("C3_CA", (168, 128, 1, False), (1, 168, 40, 40)),
    ("SPPF", (160, 160, 5), (2, 160, 20, 20)),
    ("RFCBAMConv", (160, 256, 1, 1), (2, 160, 20, 20)),
    ("RFCBAMConv", (64, 64, 3, 2), (1, 64, 21, 13)),
]
BF16_CASES = [
    ("BasicStage", (24, 1), (2, 24, 40, 48)),                   # the fused MLPBlock backward (shapes of test_mlpblock_fused_backward_bf16)
    ("BasicStage", (80, 1), (2, 80, 20, 24)),
    ("RFCBAMConv", (64, 64, 3, 2), (2, 64, 24, 24)),            # the recompute route
    ("RFCBAMConv", (256, 256, 3, 2), (1, 256, 16, 16)),         # streamed
]
_ids = lambda cases: ["-".join([c[0]] + [str(v) for v in c[1]]) for c in cases]           # noqa: E731


@functools.lru_cache(maxsize=None)
def _case(kind, ctor, shape, bf16):
    """-> (state, x, cotangent r, oracle y, oracle dx, oracle parameter gradients): computed once per case, shared, left unchanged"""
    torch.manual_seed(0)
    m = _ctor(kind)(*ctor)
    shapes = synth.shapes_of(m.state_dict())
    if not bf16:                                                  # the recipe of test_module_backward_shapes_vs_oracle
        st = synth.synth_state(shapes, 9100 + sum(shape) + len(kind))
        x = synth.synth_input(shape, 37 + shape[1])
        with torch.no_grad():
            y0 = _run(kind, list(ctor), copy.deepcopy(st), x.clone(), True)[0]
        r = synth.synth_input(tuple(y0.shape), 41 + shape[1])
        r = r * (y0.abs() > 1e-4)                                 # no cotangent within 1e-4 of a ReLU kink
    elif kind == "BasicStage":                                    # the recipe of test_mlpblock_fused_backward_bf16
        c, (n, _, h, w) = ctor[0], shape
        st = synth.synth_state(shapes, 6100 + c + w)
        x = synth.synth_input(shape, 177 + c + h).to(BF).float()
        r = synth.synth_input(shape, 178 + c + h).to(BF).float()
    else:                                                         # the recipe of test_rfcbam_backward_bf16_smooth_case: no routing decision
        c, o, k, s = ctor
        st = synth.synth_state(shapes, 7300 + c + o + k)
        st["generate.1.weight"] = torch.full_like(st["generate.1.weight"], 0.1)
        gb = torch.ones_like(st["generate.1.bias"])
        gb[:k * k] = 2.0
        st["generate.1.bias"] = gb
        st["conv.1.weight"] = torch.full_like(st["conv.1.weight"], 0.1)
        st["conv.1.bias"] = torch.ones_like(st["conv.1.bias"])
        st["se.fc.0.weight"] = st["se.fc.0.weight"].abs()
        x = synth.synth_input(shape, 41 + c) + 1.0
        ho, wo = (shape[2] + 2 * (k // 2) - k) // s + 1, (shape[3] + 2 * (k // 2) - k) // s + 1
        r = synth.synth_input((shape[0], o, ho, wo), 43 + o)
    yo, dxo, gpo = _oracle_grads(kind, list(ctor), st, x, r)
    if bf16 and kind == "RFCBAMConv":
        assert float(yo.min()) > 0.2                              # the premise of the smooth bound: no output at a ReLU kink
    return st, x, r, yo, dxo, gpo


def _frozen_names(mask, named):
    """the parameter names `mask` freezes, in registration order"""
    names = [k for k, _ in named]
    if mask == "input-only":
        return names
    if mask in ("params-only", "none"):
        return []
    if mask == "affine-frozen":
        return [k for k, p in named if p.dim() == 1]
    if mask == "weights-frozen":
        return [k for k, p in named if p.dim() >= 2]
    return names[(0 if mask == "alternate" else 1)::2]


def _hip_run(kind, ctor, st, x, r, mask, sink, bf16):
    """one train-mode forward + backward of a fresh module under `mask` (sink: through a FusedSGD's gradient storage, then a real step)
    -> dict(y, dx, grads, stats, frozen, x_grad)"""
    from lead_yolo_amd import ops, optim
    m = _bn_eps(_load(_ctor(kind)(*ctor), copy.deepcopy(st))).to(_dev()).train()
    named = list(m.named_parameters())
    frozen = set(_frozen_names(mask, named))
    for k, p in named:
        p.requires_grad_(k not in frozen)
    x_grad = mask != "params-only" and kind != "PatchEmbed_FasterNet"
    opt = None
    if sink:
        opt = optim.FusedSGD(m.parameters(), lr=0.01, weight_decay=5e-4)
        for g in opt.param_groups:                                # the first step builds the storage and installs the sink: at lr = 0 it moves nothing
            g["lr"] = 0.0
        opt.step()
        for g in opt.param_groups:
            g["lr"] = 0.01
        opt.zero_grad()
        assert ops.SINK is not None
        for k, p in named:
            assert torch.equal(p.detach().cpu(), st[k]), k
            assert (p.grad is None and ops.grad_target(p) is None) if k in frozen else (ops.grad_target(p) is p.grad and p.grad is not None), k
    xt = x.to(_dev())
    xt = (xt.to(BF) if bf16 and kind != "PatchEmbed_FasterNet" else xt).requires_grad_(x_grad)
    with torch.autocast("cuda", dtype=BF, enabled=bf16):
        y = m(xt)
    if bf16:
        y.backward(r.to(_dev()).to(BF))
    else:
        (y * r.to(_dev())).sum().backward()
    torch.cuda.synchronize()
    out = dict(y=y.detach().cpu(), dx=xt.grad.detach().float().cpu() if x_grad else None, frozen=frozen, x_grad=x_grad,
               grads={k: (None if p.grad is None else p.grad.detach().float().cpu().clone()) for k, p in named},
               stats={k: v.detach().cpu().clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k})
    assert xt.grad is None or x_grad
    if sink:
        opt.step()
        torch.cuda.synchronize()
        for k, p in named:
            same = torch.equal(p.detach().cpu(), st[k])
            if k in frozen:
                assert same, f"{kind}{ctor} {mask}: frozen {k} changed in the optimiser step"
                assert p.grad is None, k
            elif float(out["grads"][k].abs().max()) > 0:
                assert not same, f"{kind}{ctor} {mask}: trainable {k} has a gradient and did not move"
                assert float(p.grad.abs().max()) == 0.0, k       # zero_grad is part of the step
    return out


@functools.lru_cache(maxsize=None)
def _unfrozen(kind, ctor, shape, bf16):
    """the same module, weights and input with nothing frozen (no sink): run once per case"""
    st, x, r, _, _, _ = _case(kind, ctor, shape, bf16)
    return _hip_run(kind, ctor, st, x, r, "none", False, bf16)


def _l2_within(got, want, rel, floor=0.0):
    """||got - want|| <= rel * ||want|| + floor (floor: absolute slack for gradients that are zero in exact arithmetic, as _floor gives the
    fp32 comparisons) -> (holds, the error relative to ||want||)"""
    err, nw = float((got.double() - want.double()).norm()), float(want.double().norm())
    return err <= rel * nw + floor, err / max(nw, 1e-30)


def _check_grad(what, got, oracle, unfrozen, bf16, floor_o, floor_u, mx=None):
    assert got is not None, f"{what}: no gradient"
    if not bf16:
        _close(got, oracle, what + " vs oracle", floor=floor_o)
        _close(got, unfrozen, what + " vs unfrozen run", rtol=RTOL, floor=floor_u)
        return
    nfl = 1e-5 * max(floor_o, floor_u)                           # floor_o / floor_u here: the largest gradient NORM of the module (0 for dx)
    if float(oracle.norm()) > nfl:                                # (a zero gradient has no direction)
        cos = float((got.double() * oracle.double()).sum() / (got.double().norm() * oracle.double().norm()))
        assert cos >= 0.995, (what, cos)
    (ok_o, l2o), (ok_u, l2u) = _l2_within(got, oracle, 2 * REL_L2, nfl), _l2_within(got, unfrozen, 2 * REL_L2, nfl)
    assert ok_o, f"{what} vs oracle: relative L2 {l2o:.3e}"
    assert ok_u, f"{what} vs unfrozen run: relative L2 {l2u:.3e}"
    if mx is not None:
        me = float((got - oracle).abs().max()) / max(float(oracle.abs().max()), 1e-12)
        assert me <= mx or float(oracle.norm()) <= nfl, f"{what} vs oracle: max error / max |want| {me:.3e}"


def _module_masks(kind, ctor, shape, sink, bf16):
    st, x, r, yo, dxo, gpo = _case(kind, ctor, shape, bf16)
    base = _unfrozen(kind, ctor, shape, bf16)
    assert all(g is not None for g in base["grads"].values())
    if bf16:
        floor_o = max(float(v.norm()) for v in gpo.values())
        floor_u = max(float(v.norm()) for v in base["grads"].values())
    else:
        floor_o, floor_u = _floor(gpo), _floor(base["grads"])
    masks = [mk for mk in MASKS if not (kind == "PatchEmbed_FasterNet" and mk == "input-only")]
    for mask in masks:
        what = f"{kind}{ctor} {mask}{' sink' if sink else ''}"
        got = _hip_run(kind, ctor, st, x, r, mask, sink, bf16)
        frozen, names = got["frozen"], list(got["grads"])
        # premises: something is frozen (a parameter, or the input), something trains, and something trainable has a gradient
        assert frozen or not got["x_grad"], what
        assert len(frozen) < len(names) or got["x_grad"], what
        assert frozen <= set(names) and (mask not in ("alternate", "alternate-odd") or abs(len(names) - 2 * len(frozen)) <= 1)
        # the forward does not read requires_grad: same bits, same running statistics
        assert torch.equal(got["y"], base["y"]), f"{what}: the forward output differs from the unfrozen run"
        assert got["stats"].keys() == base["stats"].keys() and len(got["stats"]) > 0
        for k, v in got["stats"].items():
            assert torch.equal(v, base["stats"][k]), f"{what}: {k} differs from the unfrozen run"
            assert "num_batches" in k or not torch.equal(v, st[k]), f"{what}: {k} did not move (train-mode BatchNorm)"
        nonzero = 0
        for k in names:
            if k in frozen:
                assert got["grads"][k] is None, f"{what}: frozen {k} has a gradient"
                continue
            _check_grad(f"{what} d{k}", got["grads"][k], gpo[k], base["grads"][k], bf16, floor_o, floor_u, mx=4 * MAX_REL if kind == "BasicStage" else None)
            nonzero += float(got["grads"][k].abs().max()) > 0
        if got["x_grad"]:
            _check_grad(f"{what} dx", got["dx"], dxo, base["dx"], bf16, 0.0, 0.0, mx=4 * MAX_REL if kind == "BasicStage" else None)
            nonzero += float(got["dx"].abs().max()) > 0
        assert nonzero > 0, f"{what}: no trainable gradient is nonzero"


@pytest.mark.parametrize("sink", [False, True], ids=["autograd", "sink"])
@pytest.mark.parametrize("kind,ctor,shape", FP32_CASES, ids=_ids(FP32_CASES))
def test_module_frozen_masks_fp32(kind, ctor, shape, sink):
    """every mask of MASKS on every training module: outputs and running statistics bit-equal to the unfrozen run, every trainable gradient
    against the oracle and the unfrozen run, no gradient on a frozen parameter; sink: through a FusedSGD's storage, then a real step —
    frozen parameters bit-identical afterwards (no decay), every trainable tensor with a gradient moved"""
    _module_masks(kind, ctor, shape, sink, False)


@pytest.mark.parametrize("sink", [False, True], ids=["autograd", "sink"])
@pytest.mark.parametrize("kind,ctor,shape", BF16_CASES, ids=_ids(BF16_CASES))
def test_module_frozen_masks_bf16(kind, ctor, shape, sink):
    """the same under bf16 autocast on the routes fp32 does not take: the fused MLPBlock backward, RFCBAMConv's recompute route and its
    streamed route at the smooth-case weights (cosine >= 0.995 and 2 * REL_L2 against the oracle, 2 * REL_L2 against the unfrozen run)"""
    _module_masks(kind, ctor, shape, sink, True)


# ---- whole model ------------------------------------------------------------------------------------------------------------------------
def _wm_model(nfreeze=0):
    """lead-yolo-n with the state of tests/test_freeze_host.setup on the device, layers 0 .. nfreeze-1 frozen"""
    import lead_yolo_amd as L
    cfg, _, st, _, _ = H.setup()
    torch.manual_seed(0)
    m = L.Model(cfg)
    m.load_state_dict(st)
    m = m.to(_dev()).train()
    frozen = L.freeze_layers(m, nfreeze)
    assert sorted(frozen) == sorted(k for k, _ in m.named_parameters() if k.startswith(H.prefixes(nfreeze)))
    return m


def _wm_batch():
    _, _, _, imgs, tg = H.setup()
    return imgs.to(_dev()), tg.to(_dev())


def _frozen_set(nfreeze):
    _, _, st, _, _ = H.setup()
    return [k for k, v in st.items() if H.is_param(k, v) and k.startswith(H.prefixes(nfreeze))]


@functools.lru_cache(maxsize=None)
def _wm_grads(nfreeze, bf16):
    """loss(model(x)).backward() of the HIP model -> (prediction levels, loss, gradients by name (None where there is none))"""
    import lead_yolo_amd as L
    m = _wm_model(nfreeze)
    imgs, tg = _wm_batch()
    with torch.autocast("cuda", dtype=BF, enabled=bf16):
        pred = m(imgs.float() / 255)
        loss, _ = L.ComputeLoss(m)(pred, tg)
    loss.backward()
    torch.cuda.synchronize()
    return ([p.detach().cpu() for p in pred], float(loss.detach()),
            {k: (None if p.grad is None else p.grad.detach().float().cpu().clone()) for k, p in m.named_parameters()})


def _cat(d, names):
    return torch.cat([d[k].double().reshape(-1) for k in names])


@pytest.mark.parametrize("nfreeze", [4, 9])
def test_whole_model_frozen_gradients_fp32(nfreeze):
    """freeze 4 and freeze 9 (Concat 15 / 11 then read one source without gradient): no gradient on a frozen parameter, the trainable ones
    against the oracle (bounds of test_whole_model_gradients_vs_oracle) and the unfrozen HIP run, prediction levels bit-equal to it"""
    want = H.oracle_run(H.SCHEDULES["none"]).grads[0]
    pred0, loss0, g0 = _wm_grads(0, False)
    pred, loss, g = _wm_grads(nfreeze, False)
    frozen = set(_frozen_set(nfreeze))
    train = [k for k in g if k not in frozen]
    assert len(frozen) == 186 - len(train) and len(train) == {4: 170, 9: 138}[nfreeze]
    assert all(g[k] is None for k in frozen), [k for k in frozen if g[k] is not None][:6]
    assert all(g[k] is not None for k in train) and any(float(g[k].abs().max()) > 0 for k in train)
    assert len(pred) == 3 and all(torch.equal(a, b) for a, b in zip(pred, pred0)) and abs(loss - loss0) <= 1e-6 * abs(loss0)
    got, ref = _cat(g, train), _cat(want, train)
    cos, rel = float(torch.dot(got, ref) / (got.norm() * ref.norm())), float((got - ref).norm() / ref.norm())
    assert cos > 0.9995 and rel < 3e-2, (cos, rel)
    floor_o, floor_u = _floor({k: want[k] for k in train}), _floor({k: g0[k] for k in train})
    for k in train:
        if k.startswith("model.23."):
            _close(g[k], want[k], f"freeze {nfreeze} d{k}")
        _close(g[k], g0[k], f"freeze {nfreeze} d{k} vs unfrozen run", rtol=RTOL, floor=floor_u)
    assert floor_o > 0


def test_whole_model_frozen_gradients_bf16():
    """freeze 9 under bf16 autocast against the unfrozen HIP run: prediction levels bit-equal, trainable gradients within 2 * REL_L2"""
    pred0, loss0, g0 = _wm_grads(0, True)
    pred, loss, g = _wm_grads(9, True)
    frozen = set(_frozen_set(9))
    train = [k for k in g if k not in frozen]
    assert len(train) == 138 and all(g[k] is None for k in frozen) and all(g[k] is not None for k in train)
    assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(pred, pred0)) and abs(loss - loss0) <= 1e-5 * abs(loss0)
    assert any(float(g[k].abs().max()) > 0 for k in train)
    nfl = 1e-5 * max(float(g0[k].norm()) for k in train)
    for k in train:
        ok, l2 = _l2_within(g[k], g0[k], 2 * REL_L2, nfl)
        assert ok, f"freeze 9 bf16 d{k} vs unfrozen run: relative L2 {l2:.3e}"
    assert _l2_within(_cat(g, train), _cat(g0, train), 2 * REL_L2)[0]


def _params(m):
    return {k: p.detach().clone() for k, p in m.named_parameters()}


def _assert_mask_held(m, before, frozen, what):
    """frozen parameters are the same bits as `before`, every trainable one moved (the recipe decays or updates each of them)"""
    moved = {k: not torch.equal(p.detach(), before[k]) for k, p in m.named_parameters()}
    bad = [k for k in frozen if moved[k]]
    assert not bad, (what, "frozen parameters moved", len(bad), bad[:6])
    still = [k for k in moved if k not in frozen and not moved[k] and ".bias" not in k]       # (a bias in front of a BatchNorm: no gradient, no decay)
    assert not still, (what, "trainable parameters stayed put", len(still), still[:6])
    assert sum(moved.values()) >= 0.9 * (len(moved) - len(frozen)), what


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch"])
def test_frozen_backbone_trajectory_sgd(fused):
    """four train_steps with layers 0-8 frozen, the recipe of test_training_trajectory_vs_oracle: losses follow the oracle's FROZEN
    trajectory (which leaves the unfrozen one by more than the bounds), frozen parameters keep their bits (no decay, no momentum), the
    frozen layers' running statistics follow the oracle's, and the clip norm of the fused step covers the trainable gradients only.
    With ModelEMA: the average of a frozen parameter stays at the parameter — to the rounding of d * e + (1 - d) * p, which is what
    ModelEMA.update itself computes for an entry that does not change (<= 2 ulp per step)."""
    import lead_yolo_amd as L
    _, _, st, _, _ = H.setup()
    ref = H.oracle_run(H.SCHEDULES["freeze9"])
    frozen = _frozen_set(9)
    imgs, tg = _wm_batch()
    twin = _wm_model(9)                                           # the first step's gradients as autograd leaves them: the norm the fused step must report
    L.forward_backward(twin, L.ComputeLoss(twin), imgs, tg)
    twin_norm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in twin.parameters() if p.grad is not None)))
    m = _wm_model(9)
    opt = L.smart_optimizer(m, "SGD", H.LR, H.MOM, H.WD, fused=fused)
    assert isinstance(opt, L.FusedSGD) == fused
    ema = L.ModelEMA(m)
    cl = L.ComputeLoss(m)
    got, norms = [], []
    for i in range(4):
        if fused:
            loss, _ = L.train_step(m, cl, opt, imgs, tg, ema=ema)
            norms.append(float(opt.grad_norm))
        else:
            loss, _ = L.forward_backward(m, cl, imgs, tg)
            assert all(p.grad is None for k, p in m.named_parameters() if k in set(frozen))
            norms.append(float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters() if p.grad is not None))))
            L.optimizer_step(m, opt, ema=ema)
        got.append(float(loss))
    for i, (a, b) in enumerate(zip(got, ref.losses)):
        assert abs(a - b) <= H.BOUNDS[i] * abs(b), (got, ref.losses)
    sd = m.state_dict()
    for k in frozen:
        assert torch.equal(sd[k].cpu(), st[k]), f"frozen {k} moved"
    assert any(not torch.equal(sd[k].cpu(), st[k]) for k in st if H.is_param(k, st[k]) and k not in set(frozen))
    running = [k for k in st if k.startswith(H.prefixes(9)) and "running" in k]
    assert len(running) >= 16
    for k in running:
        _close(sd[k], ref.states[-1][k], f"frozen layer's {k} after four steps")
        assert not torch.equal(sd[k].cpu(), st[k]), k
    # the clip norm is the trainable gradients' (the oracle's full norm is more than 1e-2 away: test_freeze_host): against the norm of the
    # gradients a twin model's backward leaves, to the 1e-4 of test_fused_optimizer_matches_torch_sgd, and against the oracle's to the
    # whole-model gradient bound
    assert abs(norms[0] - twin_norm) <= 1e-4 * twin_norm, (norms, twin_norm)
    assert abs(norms[0] - ref.totals[0]) <= 3e-2 * ref.totals[0], (norms, ref.totals)
    esd = ema.ema.state_dict()
    assert ema.updates == 4
    for k in frozen:
        assert bool(((esd[k] - sd[k]).abs() <= 1e-6 * sd[k].abs()).all()), f"EMA of frozen {k} left the parameter"
    assert any(not torch.equal(esd[k], sd[k]) for k in st if H.is_param(k, st[k]) and k not in set(frozen))


def test_frozen_backbone_trajectory_adamw():
    """FusedAdamW against torch.optim.AdamW on a twin HIP model, layers 0-8 frozen in both: the bounds of
    test_adamw_training_trajectory_tracks_torch; frozen parameters keep their bits under both"""
    import lead_yolo_amd as L
    _, _, st, _, _ = H.setup()
    imgs, tg = _wm_batch()
    frozen = _frozen_set(9)
    traj = []
    for fused in (False, True):
        m = _wm_model(9)
        opt = L.smart_optimizer(m, "AdamW", 1e-3, 0.937, 5e-4, fused=fused)
        assert isinstance(opt, L.FusedAdamW) == fused
        cl = L.ComputeLoss(m)
        traj.append([float(L.train_step(m, cl, opt, imgs, tg)[0]) for _ in range(8)])
        sd = m.state_dict()
        assert all(torch.equal(sd[k].cpu(), st[k]) for k in frozen), fused
        assert any(not torch.equal(sd[k].cpu(), st[k]) for k in st if H.is_param(k, st[k]) and k not in set(frozen))
    want, got = traj
    for i, (a, b) in enumerate(zip(got, want)):
        tol = (1e-4, 1e-3, 5e-3)[i] if i < 3 else 3e-2
        assert abs(a - b) <= tol * abs(b), (got, want)
    assert got[-1] < got[0] and want[-1] < want[0], (got, want)


@pytest.mark.parametrize("amp", [None, BF], ids=["fp32", "bf16"])
def test_graphed_step_with_frozen_backbone(amp):
    """GraphedTrainStep on the freeze-9 model: ONE replay from a restored state against the eager step with the assertions of
    test_graphed_train_step_matches_eager (loss to 1e-6 / 1e-5, every weight, EMA entry and momentum buffer the same bits, the state
    moved), then frozen parameters bit-unchanged after three replays"""
    import lead_yolo_amd as L
    from lead_yolo_amd import pack
    _, _, st, _, _ = H.setup()
    frozen = set(_frozen_set(9))
    m = _wm_model(9)
    imgs, tg = _wm_batch()
    opt = L.smart_optimizer(m, "SGD", H.LR, H.MOM, H.WD)
    ema = L.ModelEMA(m)
    cl = L.ComputeLoss(m)
    step = L.GraphedTrainStep(m, cl, opt, imgs, tg, ema=ema, amp=amp, warmup=2)

    def tensors():
        return (("weight", {k: v for k, v in m.state_dict().items() if v.is_floating_point()}),
                ("ema", {k: v for k, v in ema.ema.state_dict().items() if v.is_floating_point()}),
                ("momentum", {n: opt.state[p]["momentum_buffer"] for n, p in m.named_parameters() if p in opt.state}))

    def snap():
        torch.cuda.synchronize()
        return [{k: v.detach().clone() for k, v in d.items()} for _, d in tensors()], opt._table["hyper"].clone(), ema.updates

    def restore(state):
        with torch.no_grad():
            for (_, live), saved in zip(tensors(), state[0]):
                for k, v in live.items():
                    v.copy_(saved[k])
            opt._table["hyper"].copy_(state[1])
        ema.updates = state[2]
        pack.touch_weights()

    s0 = snap()
    assert set(s0[0][2]) == {k for k, _ in m.named_parameters()} - frozen          # no momentum for a frozen parameter
    outs = []
    for how in ("eager", "eager", "graph"):
        restore(s0)
        loss, _ = step() if how == "graph" else L.train_step(m, cl, opt, imgs, tg, ema=ema, amp=amp)
        after = snap()
        assert after[2] == s0[2] + 1
        outs.append((float(loss), after[0]))
    (le, e), (le2, e2), (lg, g) = outs
    tight = 1e-6 if amp is None else 1e-5
    assert abs(le - lg) <= tight * abs(le) and abs(le - le2) <= tight * abs(le), (le, le2, lg)
    for wi, what in enumerate(("weight", "ema", "momentum")):
        a, a2, b = e[wi], e2[wi], g[wi]
        assert a.keys() == b.keys() == a2.keys() and len(a) > 100
        bad_e = [k for k in a if not torch.equal(a[k], a2[k])]
        bad_g = [k for k in a if not torch.equal(a[k], b[k])]
        assert not bad_e, (what, "two eager steps differ", len(bad_e), bad_e[:6])
        assert not bad_g, (what, "graph replay differs from the eager step", len(bad_g), bad_g[:6])
        free = [k for k in a if k not in frozen]
        moved = sum(not torch.equal(a[k], s0[0][wi][k]) for k in free)
        assert moved > 0.9 * len(free), (what, "the step did not move the state", moved, len(free))
        if what == "weight":
            assert all(torch.equal(b[k], s0[0][wi][k]) for k in frozen)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    sd = m.state_dict()
    assert all(torch.equal(sd[k].cpu(), st[k]) for k in frozen)
    assert all(p.grad is None for k, p in m.named_parameters() if k in frozen)


def test_reducer_with_frozen_backbone():
    """GradReducer over all parameters of the freeze-9 model, exchanging on a one-rank RCCL group: the buckets hold exactly the trainable
    elements, and two steps leave the weights two steps without it leave (bounds of test_train_step_with_gradient_reducer)"""
    import lead_yolo_amd as L
    _, _, st, _, _ = H.setup()
    frozen = set(_frozen_set(9))
    imgs, tg = _wm_batch()
    dist = _one_rank_group()
    try:
        res = []
        for use_reducer in (False, True):
            m = _wm_model(9)
            opt = L.smart_optimizer(m, "SGD", H.LR, H.MOM, H.WD)
            red = None
            if use_reducer:
                red = L.GradReducer(list(m.parameters())).attach()
                red.exchange_single = True
                want = sum(p.numel() for p in m.parameters() if p.requires_grad)
                assert 0 < want < sum(p.numel() for p in m.parameters())
                assert sum(b["flat"].numel() for b in red.buckets) == want and red.total_bytes() == 4 * want
                assert all(p.grad is None for k, p in m.named_parameters() if k in frozen)
            cl = L.ComputeLoss(m)
            for _ in range(2):
                loss, _ = L.train_step(m, cl, opt, imgs, tg, reducer=red)
            if red is not None:
                red.detach()
            res.append((float(loss), {k: v.detach().clone() for k, v in m.state_dict().items() if v.is_floating_point()}))
            assert all(torch.equal(res[-1][1][k].cpu(), st[k]) for k in frozen)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    assert abs(res[0][0] - res[1][0]) <= 2e-3 * abs(res[0][0])
    for k, v in res[0][1].items():
        d = float((res[1][1][k] - v).abs().max())
        assert d <= 2e-3 * float(v.abs().max()) + 1e-4, (k, d)
    assert any(not torch.equal(res[1][1][k].cpu(), st[k]) for k in st if H.is_param(k, st[k]) and k not in frozen)


# ---- the mask changes between steps -----------------------------------------------------------------------------------------------------
def _run_schedule(name):
    """fused SGD through a schedule of masks -> (model, losses, parameters after every step, a check of the gradients each step left)"""
    import lead_yolo_amd as L
    m = _wm_model(0)
    imgs, tg = _wm_batch()
    opt = L.smart_optimizer(m, "SGD", H.LR, H.MOM, H.WD)
    assert isinstance(opt, L.FusedSGD)
    cl = L.ComputeLoss(m)
    losses, states, left = [], [], []
    for nf in H.SCHEDULES[name]:
        L.freeze_layers(m, nf)
        loss, _ = L.train_step(m, cl, opt, imgs, tg)
        losses.append(float(loss))
        torch.cuda.synchronize()
        states.append(_params(m))
        left.append({k: (p.requires_grad, None if p.grad is None else float(p.grad.abs().max())) for k, p in m.named_parameters()})

    def grads_as_the_step_leaves_them():
        # zero_grad is part of the fused step; a frozen parameter has no gradient (what the reference's zero_grad() leaves)
        for i, d in enumerate(left):
            bad = [k for k, (req, g) in d.items() if (g != 0.0 if req else g is not None)]
            assert not bad, (name, f"step {i + 1}: gradients not zeroed / not None where frozen", len(bad), bad[:6])
    return m, losses, states, grads_as_the_step_leaves_them


def test_freezing_after_the_first_step():
    """(a) one unfrozen step, then layers 0-8 frozen for two: the frozen parameters keep the bits of step 1 (no gradient lands in the
    optimiser's storage, no decay, no momentum), the rest trains on, and the losses follow the oracle running the same schedule"""
    ref = H.oracle_run(H.SCHEDULES["a"])
    _, _, st, _, _ = H.setup()
    m, losses, states, check_grads = _run_schedule("a")
    frozen = _frozen_set(9)
    assert any(not torch.equal(states[0][k].cpu(), st[k]) for k in frozen)             # the backbone did train in step 1
    for i in (1, 2):
        bad = [k for k in frozen if not torch.equal(states[i][k], states[0][k])]
        assert not bad, (f"frozen parameters moved in step {i + 1}", len(bad), bad[:6])
        assert any(not torch.equal(states[i][k], states[i - 1][k]) for k in states[i] if k not in set(frozen))
    for i, (a, b) in enumerate(zip(losses, ref.losses)):
        assert abs(a - b) <= H.BOUNDS[i] * abs(b), (losses, ref.losses)
    check_grads()


def test_unfreezing_after_the_first_step():
    """(b) layers 0-8 frozen for two steps, then everything trains for two: the backbone stands still, then moves in step 3 AND in step 4
    (under a mask that never changed it moves by exactly 0 — the one thing the losses of this schedule cannot show, see test_freeze_host),
    its gradients are zeroed by each step like everybody's, and the losses follow the oracle running the same schedule, where a
    parameter that starts training starts without a momentum buffer"""
    ref = H.oracle_run(H.SCHEDULES["b"])
    _, _, st, _, _ = H.setup()
    m, losses, states, check_grads = _run_schedule("b")
    frozen = _frozen_set(9)
    assert all(torch.equal(states[1][k].cpu(), st[k]) for k in frozen)
    for i in (2, 3):
        still = [k for k in frozen if torch.equal(states[i][k], states[i - 1][k]) and ".bias" not in k]
        assert not still, (f"unfrozen parameters did not move in step {i + 1}", len(still), still[:6])
    check_grads()
    assert all(p.requires_grad and p.grad is not None for p in m.parameters())
    for i, (a, b) in enumerate(zip(losses, ref.losses)):
        assert abs(a - b) <= H.BOUNDS[i] * abs(b), (losses, ref.losses)


def _follows_or_refuses(m, nfreeze, call, what):
    """`call` runs one step of an object built under ANOTHER mask than the one set now (layers 0 .. nfreeze-1 frozen).  Either it raises a
    RuntimeError that says to rebuild, and nothing moved; or it follows the new mask.  A frozen parameter that moves or — without an
    error — a trainable one that stays put fails."""
    before = _params(m)
    frozen = set(_frozen_set(nfreeze))
    try:
        call()
    except RuntimeError as e:
        assert "rebuild" in str(e), (what, str(e))
        torch.cuda.synchronize()
        assert all(torch.equal(p.detach(), before[k]) for k, p in m.named_parameters()), (what, "refused, yet parameters moved")
        return "refused"
    torch.cuda.synchronize()
    _assert_mask_held(m, before, frozen, what)
    return "followed"


@pytest.mark.parametrize("built,then", [(9, 0), (0, 9)], ids=["unfreeze", "freeze"])
def test_captured_step_under_a_changed_mask(built, then):
    """(c) a GraphedTrainStep captured under one mask and called under another: refuses (RuntimeError, rebuild) or follows; under the mask
    it was built for it works before and after"""
    import lead_yolo_amd as L
    m = _wm_model(built)
    imgs, tg = _wm_batch()
    opt = L.smart_optimizer(m, "SGD", H.LR, H.MOM, H.WD)
    cl = L.ComputeLoss(m)
    step = L.GraphedTrainStep(m, cl, opt, imgs, tg, warmup=2)
    assert _follows_or_refuses(m, built, step, "captured step, its own mask") == "followed"
    L.freeze_layers(m, then)
    how = _follows_or_refuses(m, then, step, f"captured step built at freeze {built}, called at freeze {then}")
    if how == "refused":
        L.freeze_layers(m, built)
        assert _follows_or_refuses(m, built, step, "captured step, its own mask again") == "followed"
        # what the error asks for: a new captured step under the new mask
        L.freeze_layers(m, then)
        step = L.GraphedTrainStep(m, cl, opt, imgs, tg, warmup=2)
        assert _follows_or_refuses(m, then, step, "rebuilt captured step") == "followed"


@pytest.mark.parametrize("built,then", [(9, 0), (0, 9)], ids=["unfreeze", "freeze"])
def test_reducer_under_a_changed_mask(built, then):
    """(c) a GradReducer built under one mask and used under another: refuses (RuntimeError, rebuild) or follows; rebuilt, the step follows"""
    import lead_yolo_amd as L
    m = _wm_model(built)
    imgs, tg = _wm_batch()
    opt = L.smart_optimizer(m, "SGD", H.LR, H.MOM, H.WD)
    cl = L.ComputeLoss(m)
    red = L.GradReducer(list(m.parameters())).attach()
    one = lambda: L.train_step(m, cl, opt, imgs, tg, reducer=red)           # noqa: E731
    try:
        assert _follows_or_refuses(m, built, one, "reducer, its own mask") == "followed"
        L.freeze_layers(m, then)
        how = _follows_or_refuses(m, then, one, f"reducer built at freeze {built}, used at freeze {then}")
        if how == "refused":
            red.detach()
            red = L.GradReducer(list(m.parameters())).attach()
            assert sum(b["flat"].numel() for b in red.buckets) == sum(p.numel() for p in m.parameters() if p.requires_grad)
            assert _follows_or_refuses(m, then, one, "rebuilt reducer") == "followed"
            assert _follows_or_refuses(m, then, one, "rebuilt reducer, second step") == "followed"
    finally:
        red.detach()


def test_fused_adamw_counts_steps_per_parameter_across_a_freeze():
    """FusedAdamW against torch.optim.AdamW on the same synthetic gradients while one parameter is frozen for two steps and unfrozen again:
    torch counts a parameter's steps (its bias correction) per parameter, only where it had a gradient; the fused optimiser keeps one device
    counter and an offset per parameter, which a freeze has to shift.  The bound of test_fused_adam_matches_torch."""
    from lead_yolo_amd import optim
    g = torch.Generator().manual_seed(3)
    init = [torch.randn(s, generator=g) for s in ((5000,), (16, 8, 3, 3), (33,))]
    sets = []
    for cls in (optim.FusedAdamW, torch.optim.AdamW):
        ps = [torch.nn.Parameter(t.clone().to(_dev())) for t in init]
        sets.append((ps, cls(ps, lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, **({"max_norm": 0.0} if cls is optim.FusedAdamW else {}))))
    for step in range(6):
        grads = [torch.randn(t.shape, generator=g) for t in init]
        for ps, opt in sets:
            ps[1].requires_grad_(step not in (2, 3))
            for p, gr in zip(ps, grads):
                if not p.requires_grad:
                    p.grad = None
                elif p.grad is None:
                    p.grad = gr.to(_dev()).clone()
                else:
                    p.grad.copy_(gr)
            opt.step()
    torch.cuda.synchronize()
    (pf, of), (pt, ot) = sets
    for i, (a, b) in enumerate(zip(pf, pt)):
        assert float((a.detach() - b.detach()).abs().max()) <= 1e-5 * float(b.detach().abs().max()) + 1e-7, i
    steps = [float(of.state_dict()["state"][i]["step"]) for i in range(3)]
    assert steps == [6.0, 4.0, 6.0] == [float(ot.state[p]["step"]) for p in pt], steps
