"""GPU parity tests of the training-step backward: gradients of the HIP modules vs the
reference's own vectors (dx_train, per-parameter gradient norms in the fixtures) and vs autograd through the
oracle on identical inputs.  Tolerance: 1e-3 relative to the largest magnitude of each gradient tensor."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import synth
from tests import golden_util as G
from tests.test_gpu_modules import _bn_eps, _ctor, _dev, _load
from tests.test_oracle_golden import _run

pytestmark = pytest.mark.gpu

RTOL = 1e-3


def _close(got, want, what, rtol=RTOL, floor=0.0):
    got = got.detach().float().cpu().numpy()
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    assert err <= rtol * scale + floor + 1e-6, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _floor(grads):
    """absolute slack for gradients that are zero in exact arithmetic (a bias in front of a train-mode BatchNorm):
    rounding noise there scales with the other gradients of the module, not with the (zero) value itself"""
    return 1e-5 * max(float(v.abs().max()) for v in grads.values())


def _oracle_grads(kind, ctor, st, x, r):
    st = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running_" not in k else v.clone()) for k, v in st.items()}
    xt = x.clone().requires_grad_(True)
    y = _run(kind, list(ctor), st, xt, True)[0]
    (y * r).sum().backward()
    return y.detach(), xt.grad, {k: v.grad for k, v in st.items() if v.is_floating_point() and v.requires_grad}


def _hip_grads(m, x, r):
    xt = x.to(_dev()).requires_grad_(True)
    y = m(xt)
    (y * r.to(_dev())).sum().backward()
    return y.detach(), xt.grad, {k: p.grad for k, p in m.named_parameters()}


BACKWARD_MODULES = [n for n in (G.names("basicstage") + G.names("patchmerge") + G.names("coordatt") + G.names("cabottleneck") + G.names("c3ca")
                                + G.names("sppf") + G.names("rfcbam"))]


@pytest.mark.parametrize("name", BACKWARD_MODULES)
def test_module_backward_golden(name):
    """dx and every parameter gradient of a train-mode step, vs the reference (fixture) and the oracle (elementwise)"""
    meta, arr = G.load(name)
    st = G.state_for(meta)
    x = synth.synth_input(meta["in_shape"], meta["seed"] + 1)
    m = _bn_eps(_load(_ctor(meta["kind"])(*meta["ctor"]), st)).to(_dev()).train()
    r = synth.synth_input(arr["y_train"].shape, meta["seed"] + 2)
    y, dx, gp = _hip_grads(m, x, r)
    _close(y, arr["y_train"], name + " y_train")
    _close(dx, arr["dx_train"], name + " dx")
    nfloor = 1e-4 * max(meta["grad_norms"].values())      # slack for gradients that are exactly zero in exact arithmetic
    for k, want in meta["grad_norms"].items():
        assert gp[k] is not None, f"{name}: no gradient for {k}"
        got = float(gp[k].double().norm())
        assert abs(got - want) <= 2e-3 * want + nfloor + 1e-5, f"{name} |d{k}| = {got:.6e}, reference {want:.6e}"
    _, dxo, gpo = _oracle_grads(meta["kind"], meta["ctor"], st, x, r)
    for k, want in gpo.items():
        _close(gp[k], want, f"{name} d{k}", floor=_floor(gpo))
    sd = m.state_dict()
    for k in arr:
        if k.startswith("post_"):
            _close(sd[k[5:]], arr[k], name + " " + k)


def test_patchembed_backward_golden():
    """PatchEmbed reads the NCHW image: parameter gradients only (the image needs no gradient)"""
    name = "patchembed_3_24"
    meta, arr = G.load(name)
    st = G.state_for(meta)
    x = synth.synth_input(meta["in_shape"], meta["seed"] + 1)
    m = _bn_eps(_load(_ctor(meta["kind"])(*meta["ctor"]), st)).to(_dev()).train()
    r = synth.synth_input(arr["y_train"].shape, meta["seed"] + 2)
    y = m(x.to(_dev()))
    (y * r.to(_dev())).sum().backward()
    _close(y, arr["y_train"], name + " y_train")
    _, _, gpo = _oracle_grads(meta["kind"], meta["ctor"], st, x, r)
    for k, p in m.named_parameters():
        _close(p.grad, gpo[k], f"{name} d{k}", floor=_floor(gpo))


BWD_CASES = [
    ("BasicStage", (24, 1), (2, 24, 40, 36)),
    ("BasicStage", (40, 1), (3, 40, 17, 13)),
    ("BasicStage", (160, 1), (2, 160, 20, 20)),
    ("PatchMerging_FasterNet", (40, 80, 2, 2), (2, 40, 24, 20)),
    ("C3_CA", (168, 128, 1, False), (1, 168, 40, 40)),
    ("C3_CA", (64, 64, 3, True), (2, 64, 13, 11)),
    ("SPPF", (160, 160, 5), (2, 160, 20, 20)),
    ("RFCBAMConv", (160, 256, 1, 1), (2, 160, 20, 20)),
    ("RFCBAMConv", (128, 128, 3, 2), (2, 128, 40, 40)),
    ("RFCBAMConv", (64, 64, 3, 2), (1, 64, 21, 13)),
    # lead-yolo-l widths: channel counts above one 256-channel block group, C = 320 MLP tiles, 1024-wide C3_CA
    ("BasicStage", (320, 1), (2, 320, 10, 12)),
    ("RFCBAMConv", (512, 512, 3, 2), (2, 512, 12, 12)),
    ("RFCBAMConv", (320, 512, 1, 1), (2, 320, 10, 10)),
    ("C3_CA", (1024, 1024, 3, False), (1, 1024, 6, 6)),
    ("PatchMerging_FasterNet", (160, 320, 2, 2), (1, 160, 10, 14)),
    ("SPPF", (320, 320, 5), (2, 320, 9, 7)),
    # widths outside the six the fused MLPBlock kernel is built for (models/common.py:1494-1521 takes any dim): the composed path —
    # partial 3x3 on a channel slice, two 1x1 contraction units, their own autograd nodes
    ("BasicStage", (48, 2), (2, 48, 17, 13)),
    ("BasicStage", (64, 1), (1, 64, 24, 20)),
]


def _sink_on(m, monkeypatch):
    """an optim.FusedSGD over m's parameters, as train.py builds it.  Its first step() creates the persistent gradient storage and installs
    ops.SINK (put back when the test ends); the gradients are zero there, so the weights stay as they are.  From then on the backward kernels
    add straight into `p.grad`."""
    from lead_yolo_amd import ops, optim
    monkeypatch.setattr(ops, "SINK", ops.SINK)
    opt = optim.FusedSGD(m.parameters())
    opt.step()
    assert all(ops.grad_target(p) is p.grad for p in m.parameters())
    opt.zero_grad()


def _with_sink_cases(cases, pick):
    """every case without the gradient sink under the id it always had, and the cases `pick` selects once more with it"""
    ids = ["-".join(v if isinstance(v, str) else f"{name}{i}" for name, v in zip(("kind", "ctor", "shape")[-len(case):], case))
           for i, case in enumerate(cases)]
    return [pytest.param(*case, False, id=i) for case, i in zip(cases, ids)] + \
        [pytest.param(*case, True, id=i + "-sink") for case, i in zip(cases, ids) if pick(case)]


# the smallest case of every other node family, repeated with the sink: fused MLPBlock backward, unfused, composed ConvBnAct nodes,
# ConvBnActPair + CoordAttFn, PatchMerging, SPPF
SINK_CASES = {("BasicStage", (24, 1)), ("BasicStage", (160, 1)), ("BasicStage", (48, 2)), ("C3_CA", (64, 64, 3, True)),
              ("PatchMerging_FasterNet", (40, 80, 2, 2)), ("SPPF", (320, 320, 5))}


@pytest.mark.parametrize("kind,ctor,shape,sink", _with_sink_cases(BWD_CASES, lambda case: case[0] == "RFCBAMConv" or case[:2] in SINK_CASES))
def test_module_backward_shapes_vs_oracle(kind, ctor, shape, sink, monkeypatch):
    """real layer shapes and ragged sizes: every gradient elementwise against autograd through the oracle.  sink: the RFCBAMConv routes
    (k = 1 recompute, streamed with ly_rf3s_bwd, ragged, streamed thread = channel passes, generic k = 1) and the smallest case of every
    other node family once more with the parameter gradients written straight into an optimiser's storage"""
    torch.manual_seed(0)
    m = _ctor(kind)(*ctor)
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 9100 + sum(shape) + len(kind))
    _bn_eps(_load(m, st))
    x = synth.synth_input(shape, 37 + shape[1])
    with torch.no_grad():
        y0 = _run(kind, list(ctor), copy.deepcopy(st), x.clone(), True)[0]
    r = synth.synth_input(tuple(y0.shape), 41 + shape[1])
    # no cotangent on outputs within 1e-4 of a ReLU kink: whether such an element is "on" is decided by rounding
    # (5e-6 forward differences), and one flipped element changes every gradient by O(1) * r there
    r = r * (y0.abs() > 1e-4)
    yo, dxo, gpo = _oracle_grads(kind, ctor, st, x, r)
    m = m.to(_dev()).train()
    if sink:
        _sink_on(m, monkeypatch)
    y, dx, gp = _hip_grads(m, x, r)
    _close(y, yo, f"{kind}{ctor} y")
    _close(dx, dxo, f"{kind}{ctor} dx")
    for k, want in gpo.items():
        _close(gp[k], want, f"{kind}{ctor} d{k}", floor=_floor(gpo))


def _cfg(scale):
    import lead_yolo_amd as L
    return L.load_cfg(scale=scale)


def test_three_sgd_steps_golden():
    """Row T end to end: 3 optimiser steps of lead-yolo-n (forward, loss, HIP backward, clip, SGD-nesterov with the
    reference's three parameter groups) against the loss trajectory and weights the reference itself produced."""
    import lead_yolo_amd as L
    meta, arr = G.load("trainsteps_n")
    pm, pa = G.load("parse_n")
    st = G.state_for(meta, {"model.23.anchors": G.t(pa["anchors"])})
    m = L.Model(_cfg("n"))
    m.load_state_dict(st)
    m = m.to(_dev()).train()
    opt = L.smart_optimizer(m, "SGD", meta["lr0"], meta["momentum"], meta["weight_decay"])
    assert [len(g["params"]) for g in opt.param_groups] == [meta["groups"]["n_bias"], meta["groups"]["n_decay"], meta["groups"]["n_bn"]]
    cl = L.ComputeLoss(m)
    B = meta["B"]
    for step in range(3):
        imgs = synth.synth_images(B, 64, 910 + step).to(_dev())
        tg = synth.synth_targets(B, 920 + step, per_image=3).to(_dev())
        loss, items = L.train_step(m, cl, opt, imgs, tg)
        want = meta["losses"][step]
        assert abs(float(loss) - want) <= 1e-3 * abs(want), (step, float(loss), want)
        _close(items, arr[f"items{step}"], f"loss items step {step}")
    sd = m.state_dict()
    for k in meta["probe"]:
        # 64x64 input, batch 4: the P5 BatchNorms see 16 samples and amplify rounding differences of the forward; the
        # loss trajectory above is the tight check, the weights after three steps get a band of 3e-3
        got, want = sd[k].detach().float().cpu().numpy(), arr["final_" + k]
        np.testing.assert_allclose(got, want, rtol=3e-3, atol=3e-3, err_msg=k)


def test_whole_model_gradients_vs_oracle():
    """lead-yolo-s at 128x128, loss(model(x)).backward() against autograd through the oracle.
    The two forwards differ by ~1e-4 (bf16x3 products through 24 layers of batch-statistics BatchNorm), which flips
    the derivative of the ReLU / max units that sit within that distance of their kink; a fraction f of flipped units
    perturbs a gradient sum by ~sqrt(f), i.e. ~1e-2 — so the end-to-end comparison is a direction/length check, the
    tight check is test_whole_model_layerwise_backward below."""
    import lead_yolo_amd as L
    from oracle import functional as OF
    torch.manual_seed(0)
    m = L.Model(_cfg("s"))
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 4343)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    m.load_state_dict(st)
    x = synth.synth_images(4, 128, 17).float() / 255
    tg = synth.synth_targets(4, 18, per_image=4)
    so = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k and not k.endswith("anchors") else v.clone())
          for k, v in st.items()}
    pred = OF.model_forward(so, _cfg("s"), x, m.stride, training=True)
    lo, _ = OF.compute_loss(pred, tg, m.model[-1].anchors, nc=1)
    lo.backward()
    m = m.to(_dev()).train()
    loss, _ = L.ComputeLoss(m)(m(x.to(_dev())), tg.to(_dev()))
    loss.backward()
    assert abs(float(loss.detach()) - float(lo.detach())) <= 1e-3 * abs(float(lo.detach()))
    got = torch.cat([p.grad.detach().cpu().double().reshape(-1) for _, p in m.named_parameters()])
    want = torch.cat([so[k].grad.double().reshape(-1) for k, _ in m.named_parameters()])
    cos = float(torch.dot(got, want) / (got.norm() * want.norm()))
    rel = float((got - want).norm() / want.norm())
    assert cos > 0.9995 and rel < 3e-2, (cos, rel)
    for k, p in m.named_parameters():                       # the head sees no kink between itself and the loss: tight
        if k.startswith("model.23."):
            _close(p.grad, so[k].grad, "d" + k)


def test_whole_model_layerwise_backward():
    """Inside a full lead-yolo-s training step: every layer's (input, output cotangent) is captured from the HIP model
    and that layer is replayed alone through the oracle with the SAME tensors, so forward differences do not
    accumulate across layers.  Within a layer a handful of ReLU units (out of ~1e5-1e6) still sit closer to their kink
    than the 5e-6 forward difference and take the other branch; one such unit moves single gradient entries by O(1/N_px),
    so this test bounds the relative L2 error of every gradient tensor (~sqrt(fraction of flipped units); bound 3e-2) — it checks the composition (shared inputs, two-source / upsampled reads, strided slices); the per-module
    tests above hold the 1e-3 elementwise bar."""
    import lead_yolo_amd as L
    from lead_yolo_amd.modules import Lazy
    from oracle import functional as OF
    cfg = _cfg("s")
    torch.manual_seed(0)
    m = L.Model(cfg)
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 4343)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    m.load_state_dict(st)
    x = synth.synth_images(4, 256, 17).float() / 255
    tg = synth.synth_targets(4, 18, per_image=4)
    m = m.to(_dev()).train()
    rec = {}

    def hook(key):
        def fn(mod, inp, out):
            xin = inp[0]
            if isinstance(xin, (list, tuple)) or not isinstance(out, torch.Tensor):
                return
            r = dict(x=(xin.materialize() if isinstance(xin, Lazy) else xin).detach().clone(), y=out.detach().clone())
            out.register_hook(lambda g: r.__setitem__("dy", g.detach().clone()))
            rec[key] = r
        return fn

    for i, mod in enumerate(m.model):
        if isinstance(mod, torch.nn.Sequential) and not isinstance(mod, L.BasicStage):
            for j, sub in enumerate(mod):
                sub.register_forward_hook(hook(f"{i}.{j}"))
        else:
            mod.register_forward_hook(hook(str(i)))
    loss, _ = L.ComputeLoss(m)(m(x.to(_dev())), tg.to(_dev()))
    loss.backward()
    gp = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    layers, _ = OF.parse_graph(cfg, 3)
    kinds = {str(Lr["i"]): (Lr["kind"], Lr["args"]) for Lr in layers}
    checked = 0
    for key, r in rec.items():
        kind, args = kinds[key.split(".")[0]]
        run = {"PatchEmbed_FasterNet": lambda s_, p_, x_: OF.patch_conv(s_, p_, x_, args[2], "proj", True),
               "PatchMerging_FasterNet": lambda s_, p_, x_: OF.patch_conv(s_, p_, x_, args[2], "reduction", True),
               "BasicStage": lambda s_, p_, x_: OF.basic_stage(s_, p_, x_, True),
               "SPPF": lambda s_, p_, x_: OF.sppf(s_, p_, x_, args[2], True),
               "RFCBAMConv": lambda s_, p_, x_: OF.rfcbam(s_, p_, x_, args[2], args[3], True),
               "C3_CA": lambda s_, p_, x_: OF.c3_ca(s_, p_, x_, args[3], True)}.get(kind)
        if run is None or "dy" not in r:
            continue
        pfx = f"model.{key}."
        so = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.clone()) for k, v in st.items()
              if k.startswith(pfx)}
        xt = r["x"].cpu().contiguous().clone()
        y = run(so, pfx, xt)
        dy = r["dy"].cpu() * (y.detach().abs() > 1e-4 if kind == "RFCBAMConv" else 1.0)      # see BWD_CASES: ReLU kink
        y.backward(dy)
        _close(r["y"], y.detach(), f"layer {key} {kind} y")
        grads = {k: v.grad for k, v in so.items() if v.requires_grad}
        gs = max(float(v.abs().max()) for v in grads.values())
        for k, want in grads.items():
            if float(want.abs().max()) < 1e-4 * gs:
                continue                                   # zero in exact arithmetic (bias in front of a batch-stat BN)
            l2 = float((gp[k] - want).norm() / want.norm())
            assert l2 < 3e-2, f"layer {key} {kind} d{k[len(pfx):]}: relative L2 error {l2:.2e}"
        checked += 1
    assert checked == 19


def test_train_step_with_gradient_reducer():
    """the bucketed reducer (gradients are views into flat buckets, hooks fire per parameter) under the HIP backward:
    one step with the reducer attached must leave the same weights as one step without it (world size 1)"""
    import lead_yolo_amd as L
    res = []
    for use_reducer in (False, True):
        torch.manual_seed(0)
        m = L.Model(_cfg("n"))
        st = synth.synth_state(synth.shapes_of(m.state_dict()), 5151)
        st["model.23.anchors"] = m.model[-1].anchors.clone()
        m.load_state_dict(st)
        m = m.to(_dev()).train()
        opt = L.smart_optimizer(m, "SGD", 0.01, 0.937, 5e-4)
        red = L.GradReducer(list(m.parameters())).attach() if use_reducer else None
        imgs = synth.synth_images(4, 128, 21).to(_dev())
        tg = synth.synth_targets(4, 22, per_image=3).to(_dev())
        for _ in range(2):
            loss, _ = L.train_step(m, L.ComputeLoss(m), opt, imgs, tg, reducer=red)
        res.append((float(loss), {k: v.detach().clone() for k, v in m.state_dict().items() if v.is_floating_point()}))
    assert abs(res[0][0] - res[1][0]) <= 2e-3 * abs(res[0][0])
    for k, v in res[0][1].items():
        d = float((res[1][1][k] - v).abs().max())
        assert d <= 2e-3 * float(v.abs().max()) + 1e-4, (k, d)


def test_eval_mode_refuses_autograd():
    """backward is built for train mode; an eval-mode module must not silently return detached tensors"""
    import lead_yolo_amd as L
    m = L.BasicStage(24, 1).to(_dev()).eval()
    x = torch.randn(1, 24, 8, 8, device=_dev(), requires_grad=True)
    with pytest.raises(NotImplementedError):
        m(x)
    with torch.no_grad():
        m(x)


@pytest.mark.parametrize("scale,hw", [("s", 160), ("l", 128)])
def test_training_trajectory_vs_oracle(scale, hw):
    """other scales end to end: four optimisation steps (forward, loss, HIP backward, clip, SGD-nesterov, three groups) on a fixed
    batch follow the loss trajectory of the same steps taken by the oracle (autograd + its SGD restatement) on the CPU"""
    import lead_yolo_amd as L
    from oracle import functional as OF
    cfg = _cfg(scale)
    torch.manual_seed(0)
    m = L.Model(cfg)
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 8181)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    m.load_state_dict(st)
    imgs = synth.synth_images(4, hw, 31)
    tg = synth.synth_targets(4, 32, per_image=3)
    lr, mom, wd = 0.01, 0.937, 5e-4
    # oracle
    so = {k: v.clone() for k, v in st.items()}
    params = {k: v for k, v in so.items() if v.is_floating_point() and "running" not in k and not k.endswith("anchors")}
    groups = OF.param_groups(list(so))
    groups = {g: [k for k in ks if k in params] for g, ks in groups.items()}
    bufs, want = {}, []
    for _ in range(4):
        for p in params.values():
            p.requires_grad_(True)
            p.grad = None
        pred = OF.model_forward(so, cfg, imgs.float() / 255, m.stride, training=True)
        loss, _ = OF.compute_loss(pred, tg, so["model.23.anchors"], nc=1)
        loss.backward()
        want.append(float(loss.detach()))
        grads = {k: p.grad for k, p in params.items()}
        total = torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())).float()
        coef = torch.clamp(10.0 / (total + 1e-6), max=1.0)
        grads = {k: g * coef for k, g in grads.items()}
        with torch.no_grad():
            for gname, dec in (("decay", wd), ("bn", 0.0), ("bias", 0.0)):
                OF.sgd_nesterov_step({k: params[k] for k in groups[gname]}, grads, bufs, lr, mom, dec)
    # HIP
    m = m.to(_dev()).train()
    opt = L.smart_optimizer(m, "SGD", lr, mom, wd)
    cl = L.ComputeLoss(m)
    got = []
    for _ in range(4):
        loss, _ = L.train_step(m, cl, opt, imgs.to(_dev()), tg.to(_dev()))
        got.append(float(loss))
    # the two runs are the same algorithm in different arithmetic: they separate slowly (ReLU / max kinks)
    for (a, b), tol in zip(zip(got, want), (1e-4, 1e-3, 5e-3, 3e-2)):
        assert abs(a - b) <= tol * abs(b), (got, want)
    assert got[-1] < 0.7 * got[0]


def test_fused_optimizer_matches_torch_sgd():
    """optim.FusedSGD (clip + SGD-nesterov, 3 groups + zero_grad + EMA in two launches) vs torch.optim.SGD + clip_grad_norm_ +
    ModelEMA.update on the same gradients, four steps: parameters, momentum buffers, EMA state and the reported norm"""
    import lead_yolo_amd as L
    torch.manual_seed(0)
    ms = [L.Model(_cfg("n")).to(_dev()).train() for _ in range(2)]
    ms[1].load_state_dict(ms[0].state_dict())
    opts = [L.smart_optimizer(ms[0], "SGD", 0.02, 0.937, 5e-4, fused=True, max_norm=0.5), L.smart_optimizer(ms[1], "SGD", 0.02, 0.937, 5e-4, fused=False)]
    assert isinstance(opts[0], L.FusedSGD) and not isinstance(opts[1], L.FusedSGD)
    emas = [L.ModelEMA(m) for m in ms]
    opts[0].attach_ema(emas[0], ms[0])
    g = torch.Generator().manual_seed(1)
    for step in range(4):
        grads = [torch.randn(p.shape, generator=g) * (0.3 if step % 2 else 3.0) for p in ms[0].parameters()]       # clipped and unclipped steps
        for m in ms:
            for p, gr in zip(m.parameters(), grads):
                if p.grad is None:
                    p.grad = gr.to(_dev()).clone()
                else:
                    p.grad.copy_(gr)
            for b in m.buffers():
                if b.dtype.is_floating_point:
                    b.add_(0.01 * (step + 1))                            # running statistics move too (EMA covers buffers)
        for gr in opts[0].param_groups + opts[1].param_groups:
            gr["lr"] = 0.02 / (step + 1)                                 # a schedule: the fused step must follow param_groups
        opts[0].step()
        want_norm = torch.nn.utils.clip_grad_norm_(ms[1].parameters(), max_norm=0.5)
        opts[1].step()
        emas[1].update(ms[1])
        assert abs(float(opts[0].grad_norm) - float(want_norm)) <= 1e-4 * float(want_norm)
        assert all(float(p.grad.abs().max()) == 0.0 for p in ms[0].parameters())          # zero_grad is part of the step
    assert emas[0].updates == emas[1].updates == 4
    for (k, a), b in zip(ms[0].state_dict().items(), ms[1].state_dict().values()):
        if a.dtype.is_floating_point:
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-7, k
    for (k, a), b in zip(emas[0].ema.state_dict().items(), emas[1].ema.state_dict().values()):
        if a.dtype.is_floating_point:
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-7, ("ema", k)
    for pa, pb in zip(ms[0].parameters(), ms[1].parameters()):
        a, b = opts[0].state[pa]["momentum_buffer"], opts[1].state[pb]["momentum_buffer"]
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-7


@pytest.mark.parametrize("amp", [None, torch.bfloat16])
def test_graphed_train_step_matches_eager(amp):
    """the whole optimisation step captured into a hipGraph (forward, device loss, HIP backward, fused clip/SGD/EMA) against the eager
    step: ONE step from an IDENTICAL restored state (weights, BatchNorm statistics, momentum buffers, EMA, step counter), replayed vs
    eager — loss to 1e-3 (fp32) / 2^-7 (bf16) (or 3x what a second eager step differs by), the update of weights / EMA / momentum as
    whole vectors (direction and size) and per tensor for most tensors (see the comments at the assertions for why not all).  This test
    found a captured ATen reduction returning wrong sums (ly_sum_rows replaced it).  Then a short trajectory on changing batches,
    loosely (training noise compounds: two EAGER runs of these 4 steps differ by up to 17 % of a momentum buffer's scale)."""
    import lead_yolo_amd as L
    from lead_yolo_amd import pack
    torch.manual_seed(0)
    m = L.Model(_cfg("n"))
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 5151)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    m.load_state_dict(st)
    m = m.to(_dev()).train()
    opt = L.smart_optimizer(m, "SGD", 0.01, 0.937, 5e-4)
    ema = L.ModelEMA(m)
    cl = L.ComputeLoss(m)
    batches = [(synth.synth_images(4, 128, 21 + i).to(_dev()), synth.synth_targets(4, 22 + i, per_image=3).to(_dev())) for i in range(3)]
    nt = max(t.shape[0] for _, t in batches) + 2
    batches = [(im, torch.cat((t, torch.full((nt - t.shape[0], 6), -1.0, device=_dev())))) for im, t in batches]      # fixed shape: -1 rows are padding
    step = L.GraphedTrainStep(m, cl, opt, *batches[0], ema=ema, amp=amp, warmup=2)       # 2 eager steps on batch 0, then the capture

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
    outs = []
    for how in ("eager", "eager", "graph"):
        restore(s0)
        if how == "graph":
            loss, _ = step(*batches[1])
        else:
            loss, _ = L.train_step(m, cl, opt, *batches[1], ema=ema, amp=amp)
        after = snap()
        assert after[2] == s0[2] + 1
        outs.append((float(loss), after[0]))
    (le, e), (le2, e2), (lg, g) = outs
    # Round 4: the batch statistics (forward) and the BatchNorm-backward sums are double accumulators, so the forward of a step — every
    # ReLU / channel-max / clamp decision — is the same bits in every run and in the replay: the loss agrees to the float sums of the loss
    # kernel, and in fp32 the whole update agrees to the summation order of the weight-gradient atomics (was: 1e-3 loss band, cosine 0.98,
    # 80 % of the tensors within 5 %).  bf16 keeps wider bands: rounding the activation gradients to bf16 amplifies the last-bit noise of the
    # fp32 atomics layer by layer (tools/step_repro.py: 1e-4 at the neck, 1e-2 at the stem).
    tight = 1e-6 if amp is None else 1e-5
    assert abs(le - lg) <= tight * abs(le) and abs(le - le2) <= tight * abs(le), (le, le2, lg)
    # Round 4 (second half): nothing in the step depends on the arrival order of atomics any more (slab + fixed-order combine for every tiled
    # weight gradient, float64 scratches for the small reductions, double accumulators everywhere else) — the cosine / ratio / 95 % bands this
    # test carried are gone: two eager steps from one state, and the graph replay of that step, leave the SAME BITS in every weight, EMA
    # entry and momentum buffer.
    for wi, what in enumerate(("weight", "ema", "momentum")):
        a, a2, b = e[wi], e2[wi], g[wi]
        assert a.keys() == b.keys() == a2.keys() and len(a) > 100
        bad_e = [k for k in a if not torch.equal(a[k], a2[k])]
        bad_g = [k for k in a if not torch.equal(a[k], b[k])]
        assert not bad_e, (what, "two eager steps differ", len(bad_e), bad_e[:6])
        assert not bad_g, (what, "graph replay differs from the eager step", len(bad_g), bad_g[:6])
        moved = sum(not torch.equal(a[k], s0[0][wi][k]) for k in a)
        assert moved > 0.9 * len(a), (what, "the step did not move the state", moved, len(a))
    # ---- a short trajectory on changing batches: graph replays vs eager steps from the same state, loosely ----
    traj = []
    for how in ("eager", "graph"):
        restore(s0)
        losses = []
        for i in [1, 2, 0, 1]:
            loss, _ = step(*batches[i]) if how == "graph" else L.train_step(m, cl, opt, *batches[i], ema=ema, amp=amp)
            losses.append(float(loss))
        traj.append((losses, snap()))
    (l0, t0), (l1, t1) = traj
    assert t0[2] == t1[2] == s0[2] + 4
    tol = 1e-2 if amp is None else 5e-2
    for i, (a, b) in enumerate(zip(l0, l1)):
        assert abs(a - b) <= tol * (1 + i) * abs(a), (l0, l1)
    for a, b in zip(t0[0][:2], t1[0][:2]):
        for k in a:
            assert float((a[k] - b[k]).abs().max()) <= 10 * tol * float(a[k].abs().max()) + 1e-4, k


def _one_rank_group():
    """an RCCL process group of ONE rank on this GPU: every all-reduce is really issued (launch path, streams, events), the wire is trivial"""
    import torch.distributed as dist
    if not dist.is_initialized():
        port = 29900 + os.getpid() % 2000
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=_dev())
    return dist


@pytest.mark.parametrize("rccl,accumulate,form", [(False, 1, "overlapped"), (True, 1, "overlapped"), (True, 1, "serial"), (False, 1, "serial"),
                                                  (True, 2, "overlapped"), (True, 1, "probe"), (False, 1, "probe")])
def test_graphed_step_with_reducer_matches_eager(rccl, accumulate, form):
    """(form = "serial": ONE blocking all-reduce of the reducer's master buffer issued from the step's stream between the two graphs;
    "overlapped": the form below; "probe" (the default): both are timed at construction over the real group — 2 x (2 + DP_PROBE_REPLAYS)
    real optimisation steps whose effect on parameters, BatchNorm buffers, momentum, EMA and the optimiser's device scalars is put back —
    and the faster one kept: the trajectory afterwards must equal the eager one exactly as for a forced form)
    the data-parallel form of the captured step — graph A = forward + backward into the reducer's bucket views with an event-record
    node where each bucket completes, per-bucket all-reduce released from those events on a communication stream while A is still
    running, graph B = fused optimiser (dividing by the world size) — against eager train_step with the same reducer.  World size 1:
    without a process group (the exchange is skipped) and with a one-rank RCCL group (every bucket's all-reduce really launched);
    accumulate = 2: two micro-batches per optimiser step (reference train.py:157,300,330) vs eager no_sync accumulation."""
    import lead_yolo_amd as L
    dist = _one_rank_group() if rccl else None
    try:
        runs = []
        for graphed in (False, True):
            torch.manual_seed(0)
            m = L.Model(_cfg("n"))
            st = synth.synth_state(synth.shapes_of(m.state_dict()), 5151)
            st["model.23.anchors"] = m.model[-1].anchors.clone()
            m.load_state_dict(st)
            m = m.to(_dev()).train()
            red = L.GradReducer(list(m.parameters())).attach()
            red.exchange_single = rccl
            opt = L.smart_optimizer(m, "SGD", 0.01, 0.937, 5e-4)
            ema = L.ModelEMA(m)
            cl = L.ComputeLoss(m)
            data = [(synth.synth_images(4, 128, 21 + i).to(_dev()), synth.synth_targets(4, 22, per_image=3).to(_dev())) for i in range(2)]
            losses = []
            if graphed:
                step = L.GraphedTrainStep(m, cl, opt, *data[0], ema=ema, warmup=2, reducer=red, world_size=1, accumulate=accumulate, dp_exchange=form)
                assert len(step._marked) + len(step._unmarked) == len(red.buckets) and len(step._marked) >= 1, (step._marked, step._unmarked)
                assert red.master_covers_all()
                if form == "probe" and rccl:
                    pr = step.dp_probe                    # both forms were really timed on the group, and the step runs the faster one
                    assert pr and pr["ranks"] == 1 and pr["serial_ms"] > 0 and pr["overlapped_ms"] > 0
                    assert pr["chosen"] == ("serial" if pr["serial_ms"] < pr["overlapped_ms"] else "overlapped") and step._serial == (pr["chosen"] == "serial")
                    assert ema.updates == 2               # the probe's steps were put back
                elif form == "probe":
                    assert step.dp_probe is None and not step._serial        # no group: nothing to exchange, nothing to time
                else:
                    assert step._serial == (form == "serial" and accumulate == 1)
                for _ in range(3):
                    for j in range(accumulate):
                        loss, _ = step(*data[j % 2])
                        assert step.stepped == (j == accumulate - 1)
                    losses.append(float(loss))
            else:
                for i in range(5):
                    if accumulate == 1 or i < 2:              # (the graphed object's warm-up steps are plain steps on data[0])
                        loss, _ = L.train_step(m, cl, opt, *data[0], ema=ema, reducer=red)
                    else:
                        red.reset()
                        with red.no_sync():
                            for j in range(accumulate - 1):
                                L.forward_backward(m, cl, *data[j % 2])
                        loss, _ = L.forward_backward(m, cl, *data[(accumulate - 1) % 2])
                        red.wait()
                        L.optimizer_step(m, opt, ema=ema, reducer=red)
                    if i >= 2:
                        losses.append(float(loss))
            red.detach()
            runs.append((losses, {k: v.detach().clone() for k, v in m.state_dict().items() if v.is_floating_point()}, ema.updates))
        (l0, w0, u0), (l1, w1, u1) = runs
        assert u0 == u1 == 5
        for a, b in zip(l0, l1):
            assert abs(a - b) <= 1e-2 * abs(a), runs
        for k in w0:
            assert float((w0[k] - w1[k]).abs().max()) <= 1e-1 * float(w0[k].abs().max()) + 1e-4, k
    finally:
        if dist is not None and dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("amp", [None, torch.bfloat16])
def test_training_forward_and_gradients_are_reproducible_bit_for_bit(amp):
    """batch statistics used to be summed by float atomics in arrival order; their 1e-7 noise flipped ReLU / arg-max
    decisions downstream and two runs of the SAME step differed by 1e-3 .. 5e-2 in whole gradients (and made every end-to-end training test
    loose).  The forward statistics are double accumulators now (csrc/ly_common.hpp ly_stats_flush): from one state, two runs of forward +
    loss + backward must give (a) BIT-IDENTICAL predictions, loss and BatchNorm running statistics — every routing decision is the same —
    and (b) BIT-IDENTICAL parameter gradients (plain autograd route, no gradient sink)."""
    import lead_yolo_amd as L
    torch.manual_seed(0)
    m = L.Model(_cfg("n"))
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 7373)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    m.load_state_dict(st)
    m = m.to(_dev()).train()
    cl = L.ComputeLoss(m)
    imgs = synth.synth_images(4, 160, 71).to(_dev())
    tg = synth.synth_targets(4, 72, per_image=4).to(_dev())
    bufs0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    runs = []
    for _ in range(3):
        m.load_state_dict(bufs0)
        for p in m.parameters():
            p.grad = None
        x = imgs.float() / 255
        with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
            pred = m(x)
            loss, items = cl(pred, tg)
        loss.backward()
        torch.cuda.synchronize()
        runs.append(([p_.detach().clone() for p_ in pred], loss.detach().clone(), {k: v.detach().clone() for k, v in m.state_dict().items() if "running" in k},
                     {n: p.grad.detach().clone() for n, p in m.named_parameters()}))
    p0, l0, r0, g0 = runs[0]
    for p1, l1, r1, g1 in runs[1:]:
        for i, (a, b) in enumerate(zip(p0, p1)):
            assert torch.equal(a, b), f"prediction level {i} differs between two runs of the same step ({float((a.float() - b.float()).abs().max()):.3e})"
        assert abs(float(l0) - float(l1)) <= 1e-6 * abs(float(l0)), (float(l0), float(l1))       # (the loss sums are float atomics)
        for k in r0:
            assert torch.equal(r0[k], r1[k]), f"{k} differs between two runs"
        # round 4, second half: the gradients are the same bits as well, on this route too (gradients returned to autograd, no sink): the
        # tiled weight gradients leave through slabs + fixed-order combines and the small reductions through float64 scratches rounded by
        # ly_f64_add (was: <= 1e-5 of the whole vector, <= 5e-4 per tensor — the summation order of float atomics)
        bad = [n for n in g0 if not torch.equal(g0[n], g1[n])]
        assert not bad, f"{len(bad)} parameter gradients differ between two runs of the same step: {bad[:8]}"


@pytest.mark.parametrize("scale,bs,size", [("n", 4, 160), ("s", 8, 256)])
@pytest.mark.parametrize("amp", [None, torch.bfloat16])
def test_training_step_is_bit_reproducible_through_the_gradient_sink(amp, scale, bs, size):
    """with optim.FusedSGD's gradient sink (what train_step uses) NOTHING in a training step depends on the arrival order of
    atomics any more — batch statistics and activation-gradient sums are double accumulators, every tiled weight gradient (single and grouped
    launches) leaves through slabs + a fixed-order combine, and the small reductions (Detect bias, get_weight, k = 1 generate, CoordAtt's MLP)
    accumulate in float64 scratches that ly_f64_add rounds into the sink at the end of the backward pass.  From one state: (a) three runs of
    forward + loss + backward give BIT-IDENTICAL gradients for every parameter, (b) two optimisation steps leave BIT-IDENTICAL weights, EMA
    and momentum buffers."""
    import lead_yolo_amd as L
    torch.manual_seed(0)
    m = L.Model(_cfg(scale))
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 7373)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    m.load_state_dict(st)
    m = m.to(_dev()).train()
    cl = L.ComputeLoss(m)
    opt = L.smart_optimizer(m, "SGD", 0.01, 0.937, 5e-4, fused=True)
    imgs = synth.synth_images(bs, size, 71).to(_dev())
    tg = synth.synth_targets(bs, 72, per_image=4).to(_dev())
    L.train_step(m, cl, opt, imgs, tg, amp=amp)                       # creates the sink's persistent gradient storage
    bufs0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    mom0 = [{k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in opt.state[p_].items()} for g_ in opt.param_groups for p_ in g_["params"]]
    runs = []
    for _ in range(3):
        m.load_state_dict(bufs0)
        for p in m.parameters():
            p.grad.zero_()
        with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
            loss, _ = cl(m(imgs.float() / 255), tg)
        loss.backward()
        torch.cuda.synchronize()
        runs.append({n: p.grad.detach().clone() for n, p in m.named_parameters()})
    assert sum(float(g.abs().sum()) > 0 for g in runs[0].values()) > 0.9 * len(runs[0])
    for other in runs[1:]:
        bad = [n for n in runs[0] if not torch.equal(runs[0][n], other[n])]
        assert not bad, f"{len(bad)} parameter gradients differ between two runs of the same step: {bad[:8]}"
    for p in m.parameters():
        p.grad.zero_()
    ends = []
    for _ in range(2):
        m.load_state_dict(bufs0)
        k = 0
        for g_ in opt.param_groups:
            for p_ in g_["params"]:
                for kk, v in mom0[k].items():
                    if torch.is_tensor(v):
                        opt.state[p_][kk].copy_(v)
                k += 1
        L.train_step(m, cl, opt, imgs, tg, amp=amp)
        torch.cuda.synchronize()
        ends.append({k_: v.detach().clone() for k_, v in m.state_dict().items()})
    bad = [k_ for k_ in ends[0] if not torch.equal(ends[0][k_], ends[1][k_])]
    assert not bad, f"two optimisation steps from one state leave different tensors: {bad[:8]}"


def test_reference_training_objects_stock_ddp_gradscaler_fp16_autocast():
    """the route `python -m lead_yolo_amd.run train.py` takes, without the reference travelling: the HIP `Model` wrapped in stock
    torch.nn.parallel.DistributedDataParallel(static_graph=True) (utils/torch_utils.py:55-63) on a one-rank RCCL group, torch.optim.SGD with
    the reference's three groups (smart_optimizer, fused=False), torch.autocast(float16) + GradScaler (train.py:258, 316-341), clip_grad_norm_,
    EMA — five optimisation steps.  The modules take the non-sink gradient path here (autograd's AccumulateGrad feeds DDP's reducer hooks).
    Checked: every parameter receives a finite gradient in every step (DDP(static_graph) asserts on unused parameters), the scaler never
    skips a step, the loss falls, and after the first step the gradients equal the ones the plain (no DDP, no scaler, bf16-free fp32) HIP
    step computes from the same state up to fp16-storage noise (cosine of the whole gradient vector)."""
    import lead_yolo_amd as L
    from torch.nn.parallel import DistributedDataParallel as DDP
    dist = _one_rank_group()
    try:
        torch.manual_seed(0)
        m = L.Model(_cfg("n"))
        st = synth.synth_state(synth.shapes_of(m.state_dict()), 6262)
        st["model.23.anchors"] = m.model[-1].anchors.clone()
        m.load_state_dict(st)
        m = m.to(_dev()).train()
        imgs = (synth.synth_images(4, 128, 61).float() / 255).to(_dev())
        tg = synth.synth_targets(4, 62, per_image=3).to(_dev())
        # reference gradient: the plain fp32 HIP step from the same state
        cl = L.ComputeLoss(m)
        loss0, _ = cl(m(imgs), tg)
        loss0.backward()
        ref = torch.cat([p.grad.detach().flatten() for p in m.parameters()]).double().clone()
        for p in m.parameters():
            p.grad = None
        ddp = DDP(m, device_ids=[_dev().index or 0], static_graph=True)
        opt = L.smart_optimizer(m, "SGD", 0.01, 0.937, 5e-4, fused=False)
        assert type(opt) is torch.optim.SGD and len(opt.param_groups) == 3
        scaler = torch.amp.GradScaler("cuda", enabled=True)
        ema = L.ModelEMA(m)
        losses = []
        for it in range(5):
            with torch.autocast("cuda", dtype=torch.float16):
                pred = ddp(imgs)
                loss, _ = cl(pred, tg)
            scaler.scale(loss).backward()
            scaler.unscale_(opt)
            grads = [p.grad for p in m.parameters()]
            assert all(g is not None and torch.isfinite(g).all() for g in grads), f"step {it}: a parameter has no / a non-finite gradient"
            if it == 0:
                got = torch.cat([g.detach().flatten() for g in grads]).double()
                cos = float(got @ ref / (got.norm() * ref.norm()))
                assert cos > 0.95 and 0.9 < float(got.norm() / ref.norm()) < 1.1, (cos, float(got.norm() / ref.norm()))
            torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=10.0)
            scale_before = scaler.get_scale()
            scaler.step(opt)
            scaler.update()
            assert scaler.get_scale() >= scale_before, "GradScaler skipped a step (inf / nan gradients)"
            opt.zero_grad()
            ema.update(m)
            losses.append(float(loss))
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_graphed_step_rejects_wrong_batch_and_survives_later_allocations():
    """(a) a float batch must not be copied into the captured uint8 buffer (it would truncate to zeros); (b) the graph keeps
    the buffers it addresses alive: an eager step at a LARGER shape afterwards re-allocates the zero pool / loss constants, and replaying
    the old graph must still give the loss it gave before"""
    import lead_yolo_amd as L
    torch.manual_seed(0)
    m = L.Model(_cfg("n")).to(_dev()).train()
    opt = L.smart_optimizer(m, "SGD", 0.0, 0.937, 0.0)             # lr 0: every replay sees the same weights
    cl = L.ComputeLoss(m)
    imgs, tg = synth.synth_images(2, 64, 3).to(_dev()), synth.synth_targets(2, 4, per_image=3).to(_dev())
    assert imgs.dtype == torch.uint8
    step = L.GraphedTrainStep(m, cl, opt, imgs, tg, warmup=2)
    with pytest.raises(ValueError, match="dtype and shape"):
        step(imgs.float() / 255, tg)
    with pytest.raises(ValueError, match="dtype and shape"):
        step(imgs[:1], tg)
    before = float(step(imgs, tg)[0])
    big = synth.synth_images(4, 128, 5).to(_dev())
    L.train_step(m, cl, opt, big, synth.synth_targets(4, 6, per_image=3).to(_dev()))     # grows the pool, new loss constants
    torch.cuda.synchronize()
    after = float(step(imgs, tg)[0])
    assert abs(after - before) <= 2e-3 * abs(before), (before, after)      # lr = 0 but BN batch statistics differ by atomic noise only
    # (c) the packed-weight descriptor table: another model registers its images (the process-wide table is rebuilt and the old one freed),
    # dies (an eager step then drops its entries: rebuilt again), and other tensors take the freed memory.  The captured refresh launch
    # must not have been addressing that table (it did: an intermittent GPU memory fault in full-suite runs)
    import gc
    m2 = L.Model(_cfg("s")).to(_dev()).eval()
    with torch.no_grad():
        m2(big.float() / 255)
    del m2
    gc.collect()
    L.train_step(m, cl, opt, imgs, tg)
    junk = [torch.full((1 << 14,), -1, dtype=torch.int32, device=_dev()) for _ in range(256)]
    torch.cuda.synchronize()
    again = float(step(imgs, tg)[0])
    torch.cuda.synchronize()
    assert abs(again - before) <= 2e-3 * abs(before), (before, again)
    del junk


def _ddp_rank(rank, world, port, q, backend="nccl", one_gpu=False):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    import torch.distributed as dist
    import lead_yolo_amd as L
    try:
        dev = torch.device("cuda", 0 if one_gpu else rank)               # one_gpu: both ranks share GPU 0 (gloo stages through the host; RCCL refuses)
        torch.cuda.set_device(dev)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        torch.manual_seed(0)
        m = L.Model(L.load_cfg(scale="n")).to(dev).train()
        for t in list(m.parameters()) + list(m.buffers()):
            dist.broadcast(t.data, src=0)
        opt = L.smart_optimizer(m, "SGD", 0.01, 0.937, 5e-4)
        cl = L.ComputeLoss(m)
        imgs = synth.synth_images(4, 128, 40 + rank).to(dev)              # a different shard per rank
        tg = synth.synth_targets(4, 50 + rank, per_image=3).to(dev)
        red = L.GradReducer(list(m.parameters())).attach()
        L.train_step(m, cl, opt, imgs, tg, reducer=red, world_size=world)  # (installs the in-place gradient sink over the bucket views)
        # (1) what the exchange must produce: the MEAN over ranks of the single-GPU gradients of loss * world (train.py:321-322)
        params = [p for p in m.parameters() if p.requires_grad]
        red.reset()
        with red.no_sync():                                                # accumulate only: this rank's own gradient
            L.forward_backward(m, cl, imgs, tg, world_size=world)
        local = torch.cat([p.grad.detach().reshape(-1) for p in params]).clone()
        want = local.clone()
        dist.all_reduce(want)
        want /= world
        red.reset()
        L.forward_backward(m, cl, imgs, tg, world_size=world)              # hooks / sink callbacks launch the bucket exchanges
        red.wait()
        got = torch.cat([p.grad.detach().reshape(-1) for p in params]) * opt.grad_scale
        err = float((got - want).norm() / want.norm())
        # `want` comes from ANOTHER backward run of the same batch: since round 4 two runs of a step differ only by the summation order of the
        # weight-gradient atomics (~1e-7; the 2e-2 band this used to need failed once at 5e-2 with the float statistics accumulators).  What
        # this must catch is structural: a sum instead of a mean (err = 1), a bucket that was not exchanged or went out before its last
        # gradient (>= 0.1), a stale gradient
        assert err < 1e-4, f"exchanged gradient is not the mean of the ranks' gradients: rel err {err}"
        assert float((local - want).norm() / want.norm()) > 1e-2          # the shards really differ
        red.reset()
        for _ in range(2):
            L.train_step(m, cl, opt, imgs, tg, reducer=red, world_size=world)
        # (2) the captured form: graph A with bucket events, RCCL released from them, graph B
        step = L.GraphedTrainStep(m, cl, opt, imgs, tg, warmup=1, reducer=red, world_size=world)
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        # replicas must hold identical weights after averaged-gradient steps (BatchNorm running statistics are per-rank by design)
        flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
        other = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(other, flat)
        same = all(torch.equal(other[0], o) for o in other[1:])
        q.put((rank, "ok" if same else "replicas diverged"))
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e)))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _free_port():
    import socket
    with socket.socket() as s:                                           # a port nobody holds right now (the fixed base + pid scheme met an
        s.bind(("127.0.0.1", 0))                                         # "address already in use" on a busy box once)
        return s.getsockname()[1]


def _run_two_ranks(backend, one_gpu, port0, timeout):
    res = _run_two_ranks_once(backend, one_gpu, _free_port(), timeout)
    if any("in use" in str(r[1]) for r in res):                          # lost the race for the port: once more on another one
        res = _run_two_ranks_once(backend, one_gpu, _free_port(), timeout)
    return res


def _run_two_ranks_once(backend, one_gpu, port, timeout):
    import queue
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_ddp_rank, args=(r, 2, port, q, backend, one_gpu)) for r in range(2)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in procs:
            res.append(q.get(timeout=timeout))
    except queue.Empty:
        res.append((-1, f"no answer within {timeout} s"))
    for p in procs:
        p.join(timeout=30)
        if p.is_alive():
            p.kill()                                                     # (this exact child: never a pattern kill)
    return sorted(res)


def test_two_rank_rccl_train_step():
    """data-parallel train step over RCCL on two GPUs (skipped on a one-GPU box): rank-0 broadcast, per-rank shards, bucketed
    all-reduce from the gradient hooks / in-place gradient sink — the exchanged gradient equals the MEAN of the ranks' single-GPU gradients —
    fused optimiser, then the captured step with the exchange released from in-graph bucket events; replicas stay bit-identical"""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    assert _run_two_ranks("nccl", False, 29600, 600) == [(0, "ok"), (1, "ok")]


def test_two_rank_step_on_one_gpu_over_gloo():
    """the same two-rank protocol with BOTH ranks on GPU 0 and the gloo backend (which stages device tensors through the host; RCCL refuses
    two ranks on one device): a world-size-2 HIP training step — in-place gradient sink into bucket views, per-bucket exchange, 1/world in
    the fused optimiser, the captured graph A / exchange / graph B form — runs under test on a one-GPU box.  The wire is not what is tested."""
    assert _run_two_ranks("gloo", True, 31600, 300) == [(0, "ok"), (1, "ok")]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 3, 64, 96), (1, 3, 8, 260), (3, 1, 32, 32)])
def test_patch4_rows_u8_equals_permuted_copy(shape, dtype):
    """space-to-depth of the uint8 image for PatchEmbed's weight gradient (models/common.py:1537-1550): bit-exact vs the torch permute"""
    import lead_yolo_amd as L
    n, c, h, w = shape
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).to(_dev())
    got = L.ops.patch4_rows_u8(img, dtype)
    want = img.reshape(n, c, h // 4, 4, w // 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(-1, 16 * c).to(dtype)
    assert got.shape == want.shape and torch.equal(got, want)


def test_bn_bwd_coeffs_transposed_targets_accumulate():
    """ly_bn_bwd_coeffs with tr_a, tr_b (RFCBAMConv's generate BatchNorm: sums in [tap][channel] order, parameters in [channel][tap]):
    dgamma / dbeta are ADDED into the transposed targets, alpha / kappa / lambda stay in the sums' order"""
    from lead_yolo_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(2)
    kk, c, count = 9, 40, 777.0
    n = kk * c
    sums = torch.randn(ops.STRIPES, 2 * n, generator=g, dtype=torch.float64).to(dev)
    a, mean = torch.rand(n, generator=g).to(dev) + 0.5, torch.randn(n, generator=g).to(dev)
    invstd = torch.rand(n, generator=g).to(dev) + 0.5
    dg0, db0, al0, ka0, la0 = ops.bn_bwd_coeffs(sums, n, count, a, mean, invstd, True)
    tg, tb = torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
    tg1, tb1 = tg.clone(), tb.clone()
    r = ops.bn_bwd_coeffs(sums, n, count, a, mean, invstd, True, dgamma=tg1, dbeta=tb1, transpose=(kk, c))
    assert r[0] is None and r[1] is None
    tr = lambda v: v.view(kk, c).t().contiguous().view(-1)
    torch.testing.assert_close(tg1, tg + tr(dg0), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(tb1, tb + tr(db0), rtol=1e-6, atol=1e-6)
    assert torch.equal(r[2], al0) and torch.equal(r[3], ka0) and torch.equal(r[4], la0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("geom", [(2, 64, 20, 20), (1, 40, 7, 13), (3, 128, 5, 160)])
def test_detect_head_node_equals_autograd_chain(geom, dtype):
    """grad.DetectHeadFn (one Detect level in training, models/yolo.py:84-88) vs the generic conv node followed by autograd's
    view / permute / copy chain: same raw map (the node's forward is ly_detect_level where it is built: the fp32 accumulators go to the
    map as they are, the chain rounds the head output to the storage type first), same dx / dW / dbias (both use the same contraction
    kernels; the fused adjoint only changes who lays out du and who sums the bias gradient)."""
    import lead_yolo_amd as L
    from lead_yolo_amd import grad, pack
    bs, cin, ny, nx = geom
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    det = L.Detect(nc=1, anchors=((10, 13, 16, 30, 33, 23),), ch=(cin,)).to(dev).train()
    with torch.no_grad():
        det.m[0].weight.copy_(torch.randn(det.m[0].weight.shape, generator=g) * 0.1)
        det.m[0].bias.copy_(torch.randn(det.m[0].bias.shape, generator=g))
    x0 = torch.randn(bs, cin, ny, nx, generator=g).to(dev).to(dtype).contiguous(memory_format=torch.channels_last)
    r = torch.randn(bs, det.na, ny, nx, det.no, generator=g).to(dev)
    conv = det.m[0]
    wp, _ = det._packed(0, L.ops.planes_of(x0))
    res = []
    for fused in (True, False):
        conv.weight.grad = conv.bias.grad = None
        x = x0.clone().requires_grad_(True)
        if fused:
            p = grad.DetectHeadFn.apply(det, 0, wp, x, conv.weight, conv.bias)
        else:
            y = grad.conv_bn_act(grad.ConvSpec("pw", conv.out_channels), wp, x, None, conv.weight, conv.bias, None)
            p = torch.empty((bs, det.na, ny, nx, det.no), dtype=torch.float32, device=dev)
            p.copy_(y.view(bs, det.na, det.no, ny, nx).permute(0, 1, 3, 4, 2))
        (p * r).sum().backward()
        res.append((p.detach().clone(), x.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone()))
    (p1, dx1, dw1, db1), (p2, dx2, dw2, db2) = res
    torch.testing.assert_close(p1, p2, rtol=1e-5 if dtype == torch.float32 else 8e-3, atol=1e-5 if dtype == torch.float32 else 8e-3)
    tol = 1e-5 if dtype == torch.float32 else 1e-2        # bf16: the chain rounds dp to bf16 before summing the bias gradient, the node after
    _close(dx1, dx2.float(), "dx", rtol=tol)
    _close(dw1, dw2, "dw", rtol=tol)
    _close(db1, db2, "dbias", rtol=tol)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_wgrad_group_equals_separate_launches(dtype):
    """ly_wgrad_group (several plain-row 1x1 weight gradients sharing one launch) against one ly_wgrad launch per problem and against
    the plain matrix product; a non-groupable mix (N <= 64) must fall back to separate launches with the same result"""
    import lead_yolo_amd as L
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    n, h, w = 3, 20, 24
    m = n * h * w

    def problem(N, C, ldx_extra=0):
        du = torch.randn(m, N, generator=g).to(dev).to(dtype)
        x = torch.randn(m, C + ldx_extra, generator=g).to(dev).to(dtype)
        return du, x, dict(M=m, H=h, W=w, N=N, du=du, lddu=N, x=x, ldx=C + ldx_extra, Hin=h, Win=w, Cin=C, lddw=C)
    for shapes in ([(160, 80, 0), (80, 160, 0)], [(256, 128, 8), (128, 256, 0), (72, 200, 0)], [(160, 80, 0), (40, 80, 0)]):
        probs = [problem(*sh) for sh in shapes]
        outs = []
        for grouped in (True, False):
            dws = [torch.zeros(q["N"], q["Cin"], dtype=torch.float32, device=dev) for _, _, q in probs]
            qs = [dict(q, dw=dw) for (_, _, q), dw in zip(probs, dws)]
            if grouped:
                L.ops.wgrad_group(qs)
            else:
                for q in qs:
                    L.ops.wgrad(**q)
            outs.append(dws)
        for (du, x, q), a, b in zip(probs, *outs):
            want = du.float().t() @ x.float()[:, :q["Cin"]]
            tol = 1e-3 if dtype == torch.float32 else 1e-5        # bf16 inputs: products exact in fp32, only the summation order differs
            _close(a, want, "grouped vs matmul", rtol=max(tol, 2e-4))
            _close(a, b, "grouped vs separate", rtol=2e-4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(24, 48), (40, 80), (80, 160), (160, 320)])
def test_wgrad_x_prologue(shape, dtype):
    """LyWgradParams.x_scale / x_shift: dw = du^T . max(x*scale + shift, 0) without materialising the activated tensor (the MLPBlock's
    hidden tensor in the training backward), every tile class of the plain-row path, alone and inside a grouped launch"""
    import lead_yolo_amd as L
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    N, C = shape
    n, h, w = 2, 20, 28
    m = n * h * w
    du = torch.randn(m, N, generator=g).to(dev).to(dtype)
    x = torch.randn(m, C, generator=g).to(dev).to(dtype)
    a = (torch.rand(C + 12, generator=g) + 0.5).to(dev)
    b = torch.randn(C + 12, generator=g).to(dev)
    act = torch.relu(x.float() * a[:C] + b[:C])
    if dtype == torch.bfloat16:
        act = act.to(dtype).float()                       # the kernel rounds the activated value to the storage type before the product
    want = du.float().t() @ act
    q = dict(M=m, H=h, W=w, N=N, du=du, lddu=N, x=x, ldx=C, Hin=h, Win=w, Cin=C, lddw=C, x_scale=a, x_shift=b)
    dw = torch.zeros(N, C, dtype=torch.float32, device=dev)
    L.ops.wgrad(**dict(q, dw=dw))
    _close(dw, want, "prologue", rtol=1e-3 if dtype == torch.float32 else 1e-4)
    dw2 = torch.zeros(N, C, dtype=torch.float32, device=dev)
    other = torch.zeros(C, N, dtype=torch.float32, device=dev)
    L.ops.wgrad_group([dict(q, dw=dw2), dict(M=m, H=h, W=w, N=C, du=x, lddu=C, x=du, ldx=N, Hin=h, Win=w, Cin=N, dw=other, lddw=N)])
    _close(dw2, want, "prologue in a group", rtol=1e-3 if dtype == torch.float32 else 1e-4)
    _close(other, x.float().t() @ du.float(), "its plain neighbour", rtol=1e-3 if dtype == torch.float32 else 1e-4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("geom", [(3, 16, 20, 20), (2, 40, 7, 13), (1, 8, 24, 24)])
def test_sppf_backward_fused_equals_per_level_kernels(geom, dtype):
    """ly_sppf_bwd (the three max-pool levels of SPPF's backward from LDS, one launch) against the per-level ly_maxpool_arg /
    ly_maxpool_gather launches it replaces: bit-identical (same routing rule, same summation order), ties included"""
    import ctypes
    import lead_yolo_amd as L
    n, c, h, w = geom
    dev = _dev()
    g = torch.Generator().manual_seed(17)
    y = (torch.randint(-3, 4, (n, c, h, w), generator=g).float() * 0.5).to(dev).to(dtype).contiguous(memory_format=torch.channels_last)   # many ties
    yr = y.detach().clone().requires_grad_(True)
    from lead_yolo_amd import grad as Gm
    buf = Gm.SppfPool.apply(yr, 5)
    r = torch.randn(buf.shape, generator=g).to(dev).to(dtype).contiguous(memory_format=torch.channels_last)
    buf.backward(r)
    fused = yr.grad.clone()
    # the per-level path, called directly
    C = L.capi
    st = C.stream_ptr()
    at = lambda t, off: ctypes.c_void_p(t.data_ptr() + t.element_size() * off)
    b = buf.detach()
    c4 = 4 * c
    arg = torch.empty((n * h * w, 3 * c), dtype=torch.uint8, device=dev)
    C.check(C.lib().ly_maxpool_arg(C.ptr(b), c4, n, h, w, 3 * c, 5, C.ptr(arg), 3 * c, C.dtype_code(b), st), "ly_maxpool_arg")
    up = r[:, 3 * c:].float().contiguous(memory_format=torch.channels_last)
    tmp = [torch.empty((n * h * w, c), dtype=torch.float32, device=dev) for _ in range(2)]
    out = L.ops.empty_nhwc(n, c, h, w, b)
    for j in (2, 1, 0):
        dst = out if j == 0 else tmp[j & 1]
        C.check(C.lib().ly_maxpool_gather(at(arg, j * c), 3 * c, C.ptr(up) if j == 2 else C.ptr(tmp[(j + 1) & 1]), c, at(r, j * c), c4, C.dtype_code(r),
                                          n, h, w, c, 5, C.ptr(dst), c, C.dtype_code(dst), st), "ly_maxpool_gather")
    assert torch.equal(fused, out)


@pytest.mark.parametrize("offset", [10.0, 100.0])
def test_batchnorm_statistics_with_large_mean(offset):
    """|mean| >> std in front of a train-mode BatchNorm: the statistics are fp32 sums of u and u^2 (striped float atomics,
    stripes summed in double, var = E[u^2] - E[u]^2), so the variance loses ~(mean/std)^2 * 2^-24 relative accuracy.  An input offset of
    10 / 100 standard deviations through PatchMerging's k2s2 conv + BatchNorm (models/common.py:1555-1561) must stay inside the 1e-3
    budget in the output and the input gradient (measured 4e-5 / 3e-4); the envelope ends near offset 1000 (1.6e-2), DESIGN §4a."""
    import lead_yolo_amd as L
    from tests.test_oracle_golden import _run
    kind, ctor, shape = "PatchMerging_FasterNet", (24, 40, 2, 2), (4, 24, 40, 36)
    torch.manual_seed(0)
    m = L.PatchMerging_FasterNet(*ctor)
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 4242)
    _bn_eps(_load(m, st))
    x = synth.synth_input(shape, 7) + offset
    stt = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.clone()) for k, v in st.items()}
    xt = x.clone().requires_grad_(True)
    yo, _ = _run(kind, list(ctor), stt, xt, True)
    g = synth.synth_input(tuple(yo.shape), 9)
    yo.backward(g)
    m = m.to(_dev()).train()
    xg = x.to(_dev()).requires_grad_(True)
    y = m(xg)
    y.backward(g.to(_dev()))
    ey = float((y.detach().cpu() - yo.detach()).abs().max()) / float(yo.detach().abs().max())
    ex = float((xg.grad.cpu() - xt.grad).abs().max()) / float(xt.grad.abs().max())
    assert ey <= 1e-3 and ex <= 1e-3, (offset, ey, ex)
    # running statistics follow the reference's update too
    rm, rv = m.norm.running_mean.cpu(), m.norm.running_var.cpu()
    assert torch.allclose(rm, stt["norm.running_mean"], rtol=1e-4, atol=1e-4) and torch.allclose(rv, stt["norm.running_var"], rtol=2e-3, atol=1e-4), offset


@pytest.mark.parametrize("n,h,w,nout", [(3, 64, 64, 24), (2, 52, 76, 24), (1, 640, 640, 24), (5, 36, 44, 40), (2, 48, 48, 16), (2, 40, 56, 64)])
def test_patch4_wgrad_from_the_uint8_image(n, h, w, nout):
    """PatchEmbed's weight gradient straight from the uint8 batch (ly_patch4_wgrad_u8: no space-to-depth rows) against the contraction it
    replaces, written out in fp64: dw[o][c, ky, kx] = sum_m du[m][o] * img[n, c, 4 ho + ky, 4 wo + kx] / 255; ragged last units, one to
    four output-channel tiles; added onto what dw held; two launches return the same bits (fixed-order fold of the block partials)"""
    from lead_yolo_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(100 * n + nout)
    img = torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8).to(dev)
    ho, wo = h // 4, w // 4
    m = n * ho * wo
    du = (torch.randn(m, nout, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    assert ops.patch4_wgrad_u8_ok(img, du, nout)
    base = torch.randn(nout, 48, generator=g).to(dev)
    rows = img.reshape(n, 3, ho, 4, wo, 4).permute(0, 2, 4, 1, 3, 5).reshape(m, 48).double()
    want = base.double() + du.double().t() @ rows / 255.0
    outs = []
    for _ in range(2):
        dw = base.clone()
        ops.patch4_wgrad_u8(img, du, nout, nout, dw, 1.0 / 255.0)
        torch.cuda.synchronize()
        outs.append(dw)
    scale = want.abs().max().item()
    assert (outs[0].double() - want).abs().max().item() <= 2e-5 * scale + 1e-5, ((outs[0].double() - want).abs().max().item(), scale)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("n,h,w,cin,cout,cvalid,ldx", [(2, 16, 16, 64, 64, 64, 64), (3, 20, 20, 128, 96, 128, 128), (1, 13, 27, 32, 200, 32, 32),
                                                      (2, 40, 24, 8, 8, 6, 24), (2, 9, 11, 40, 40, 40, 160), (1, 80, 80, 64, 64, 64, 64)])
def test_wgrad3_halo_kernel(n, h, w, cin, cout, cvalid, ldx):
    """ly_wgrad3 (3x3 / stride 1 / pad 1 weight gradient from an LDS halo tile with transposed fragment reads, csrc/ly_wgrad3.hip) vs the
    weight gradient autograd gives nn.Conv2d (models/common.py:1890-1910; partial conv: models/common.py:1412-1437) in fp64, and vs the
    generic tiled kernel it replaces: ragged maps, output channels off the 64-row tile, a channel SLICE of a wider tensor with padded
    channels (the partial conv: 6 valid of 8 read), tap-major gradient storage"""
    import lead_yolo_amd as L
    from lead_yolo_amd import capi, ops
    dev = _dev()
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + cin)
    xfull = torch.randn(n, h, w, ldx, generator=g).to(dev).to(torch.bfloat16)            # NHWC rows of width ldx; the conv reads channels [0, cin)
    du = torch.randn(n, h, w, cout, generator=g).to(dev).to(torch.bfloat16)
    xs = xfull[..., :cvalid].float().permute(0, 3, 1, 2).double()
    want = torch.nn.grad.conv2d_weight(xs, (cout, cvalid, 3, 3), du.float().permute(0, 3, 1, 2).double(), stride=1, padding=1)      # [o, c, ky, kx]
    got = {}
    for on in (1, 0):
        was = capi.lib().ly_tune_wgrad3(on)
        try:
            dw = torch.zeros(cout, 3, 3, cin, dtype=torch.float32, device=dev)             # tap-major storage [o][ky][kx][c]
            ops.wgrad(M=n * h * w, H=h, W=w, N=cout, du=du, lddu=cout, x=xfull, ldx=ldx, Hin=h, Win=w, Cin=cin, dw=dw, lddw=9 * cin, ks=3, stride=1, pad=1,
                      c_valid=cvalid)
            ops.wgrad(M=n * h * w, H=h, W=w, N=cout, du=du, lddu=cout, x=xfull, ldx=ldx, Hin=h, Win=w, Cin=cin, dw=dw, lddw=9 * cin, ks=3, stride=1, pad=1,
                      c_valid=cvalid)                                                     # accumulates: twice the gradient
            torch.cuda.synchronize()
            got[on] = dw.permute(0, 3, 1, 2)[:, :cvalid].double() / 2
            assert float(dw[..., cvalid:].abs().max()) == 0.0 if cvalid < cin else True   # padded channels untouched
        finally:
            capi.lib().ly_tune_wgrad3(was)
    scale = float(want.abs().max())
    for on in (1, 0):
        assert float((got[on] - want).abs().max()) <= 2e-3 * scale, (on, float((got[on] - want).abs().max()), scale)      # bf16 products, fp32 sums
    assert float((got[1] - got[0]).abs().max()) <= 5e-4 * scale


def test_large_lds_kernels_on_two_devices_of_one_process():
    """Kernels whose dynamic LDS exceeds the 64 KB a launch gets by default, launched on device 0 and then on device 1 from ONE process
    (skipped on a one-GPU box): the cap is a per-device function attribute (ly_launch_lds, csrc/ly_common.hpp), so the second device needs
    it set as well; a refused launch is the library's error return.  By the launchers' own formulas:
      * ops.wgrad, plain-row 1x1, N = 128, Cin = 128, M = 2 * 16 * 16: the 128 x 128 tile of launch_wgrad_tiled (csrc/ly_wgrad.hip),
        one LDS buffer of PL * (PX / 8) rows of (128 + 128 + 16) * 16 B + 2 * 128 floats = 70,656 B for bf16 (PL 1, PX 128) and the same
        70,656 B for fp32 (PL 2, PX 64);
      * Conv k = 3, fp32, 128 -> 128 channels on 2 x 16 x 16 (ops.conv3x3, launch_conv3 in csrc/ly_conv3x3.hip): patch 16 x 8
        (pick_conv_tile), row pitch 640 B, plane stride 18 * 640 = 11,520 B, PL * 4 planes = 92,160 B.
    Each result against the fp64 contraction on the host with the tolerance of the op's single-device test: 2e-3 of the reference's
    maximum for the bf16 weight gradient (test_wgrad3_halo_kernel), 1e-3 for fp32 (test_wgrad_x_prologue), 2^-14 * sum |w x| for the fp32
    3x3 convolution (test_bf16x3_adversarial_bounds, tests/test_gpu_modules.py)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    import torch.nn.functional as F
    import lead_yolo_amd as L
    from lead_yolo_amd import ops
    g = torch.Generator().manual_seed(11)
    n, h, w, N, C = 2, 16, 16, 128, 128
    m = n * h * w
    wg = {}
    for dtype in (torch.bfloat16, torch.float32):
        du, x = torch.randn(m, N, generator=g).to(dtype), torch.randn(m, C, generator=g).to(dtype)
        wg[dtype] = (du, x, du.double().t() @ x.double())
    conv = L.Conv(C, N, 3, 1)
    with torch.no_grad():
        conv.conv.weight.copy_(0.05 * torch.randn(N, C, 3, 3, generator=g))
        conv.bn.weight.fill_(1.0); conv.bn.bias.zero_(); conv.bn.running_mean.zero_(); conv.bn.running_var.fill_(1.0)
        conv.bn.eps = 0.0
        conv.act = torch.nn.Identity()
        xc = torch.randn(n, C, h, w, generator=g)
        want_c = F.conv2d(xc.double(), conv.conv.weight.double(), padding=1)
        mag_c = F.conv2d(xc.abs().double(), conv.conv.weight.abs().double(), padding=1)         # sum_k |w_k x_k|
    for d in (0, 1):
        dev = torch.device("cuda", d)
        with torch.cuda.device(d):
            for dtype, (du, x, want) in wg.items():
                dw = torch.zeros(N, C, dtype=torch.float32, device=dev)
                ops.wgrad(M=m, H=h, W=w, N=N, du=du.to(dev), lddu=N, x=x.to(dev), ldx=C, Hin=h, Win=w, Cin=C, dw=dw, lddw=C)
                torch.cuda.synchronize()
                err, scale = float((dw.cpu().double() - want).abs().max()), float(want.abs().max())
                assert err <= (2e-3 if dtype == torch.bfloat16 else 1e-3) * scale, (d, dtype, err, scale)
            with torch.no_grad():
                got = copy.deepcopy(conv).to(dev).eval()(xc.to(dev)).double().cpu()
            assert bool(((got - want_c).abs() <= 2.0 ** -14 * mag_c + 1e-7).all()), (d, float(((got - want_c).abs() / mag_c).max()))


def _pack_plain(w, dtype):
    """packed fragment image of a [N, K] fp32 matrix (pack.packed over a parameter-like tensor)"""
    from lead_yolo_amd import ops, pack
    p = torch.nn.Parameter(w.clone())
    return p, pack.packed(pack.src_matrix(p, w.shape[0], w.shape[1]), w.shape[1], ops.planes_of(torch.empty(1, dtype=dtype, device=w.device)))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n,h,w,k,c,ks", [(2, 6, 10, 64, 24, 2), (3, 5, 7, 128, 40, 2), (1, 4, 4, 256, 8, 4), (2, 9, 5, 136, 128, 1), (2, 8, 8, 320, 256, 1)])
def test_gemm_scatter_store_and_added_gradient(n, h, w, k, c, ks, dtype):
    """LyGemmParams.scat_ks (the adjoint of the k = s patch gather as the store) and LyGemmParams.eadd (another consumer's gradient added
    before the store, read with a row stride of its own) vs the two-step form in fp64"""
    from lead_yolo_amd import ops
    g = torch.Generator().manual_seed(5 + n + k)
    a = torch.randn(n * h * w, k, generator=g).to(dtype)
    wm = torch.randn(ks * ks * c, k, generator=g) * 0.1
    prm, wp = _pack_plain(wm.to(_dev()), dtype)
    ad = a.to(_dev())
    lde = c + 8
    prev = torch.randn(n * ks * h * ks * w, lde, generator=g).to(dtype)
    ref = a.double() @ wm.to(dtype if dtype == torch.bfloat16 else torch.float32).double().t() if dtype == torch.bfloat16 else a.double() @ wm.double().t()
    ref = ref.view(n, h, w, ks, ks, c).permute(0, 1, 3, 2, 4, 5).reshape(n * ks * h * ks * w, c)
    for eadd in (None, prev.to(_dev())):
        out = torch.full((n * ks * h * ks * w, c), float("nan"), dtype=dtype, device=_dev())
        kw = dict(scat_ks=ks, scat_c=c) if ks > 1 else {}
        if eadd is not None:
            kw.update(eadd=eadd, ldeadd=lde)
        elif ks == 1:
            continue
        ops.gemm(M=n * h * w, H=h, W=w, K=k, N=ks * ks * c, a0=ad, lda0=k, k0=k, wp=wp, out=out, ldo=c, **kw)
        want = ref if eadd is None else ref + prev[:, :c].double()
        tol = 2e-2 if dtype == torch.bfloat16 else 2e-3
        err = float((out.double().cpu() - want).abs().max())
        assert torch.isfinite(out).all() and err <= tol * float(want.abs().max()), (ks, eadd is not None, err)


@pytest.mark.parametrize("amp", [None, torch.bfloat16])
def test_fork_sum_matches_autograd_sum(amp, monkeypatch):
    """grad.fork (the six two-consumer layer outputs of lead-yolo: the second gradient is added in a GEMM's store, LyGemmParams.eadd) vs
    autograd's own sum of the two gradients, from one state: the same predictions bit for bit, parameter gradients equal within the storage
    rounding of the one summed tensor, and all six sums are stores (LyGemmParams.eadd launches)"""
    import lead_yolo_amd as L
    from lead_yolo_amd import grad
    torch.manual_seed(0)
    m = L.Model(_cfg("s"))
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 7373)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    m.load_state_dict(st)
    m = m.to(_dev()).train()
    assert sorted(m._two_consumer_layers()) == [3, 5, 9, 13, 16, 19]
    cl = L.ComputeLoss(m)
    imgs = synth.synth_images(4, 160, 71).to(_dev())
    tg = synth.synth_targets(4, 72, per_image=4).to(_dev())
    bufs0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    res = {}
    for on in (True, False):
        monkeypatch.setattr(grad, "FORK_SUM", on)
        m.load_state_dict(bufs0)
        for p in m.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
            pred = m(imgs.float() / 255)
            loss, _ = cl(pred, tg)
        added = []
        real_gemm = grad.ops.gemm
        monkeypatch.setattr(grad.ops, "gemm", lambda **kw: (added.append(kw["N"]) if kw.get("eadd") is not None else None, real_gemm(**kw))[1])
        loss.backward()
        monkeypatch.setattr(grad.ops, "gemm", real_gemm)
        torch.cuda.synchronize()
        res[on] = ([p_.detach().clone() for p_ in pred], {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}, len(added))
    for a, b in zip(res[True][0], res[False][0]):
        assert torch.equal(a, b)
    assert res[True][2] == 6 and res[False][2] == 0, (res[True][2], res[False][2])       # one store-side sum per two-consumer tensor
    if amp is None:                 # fp32 storage: the same sums, only the association of one addition differs
        for k in res[True][1]:
            a, b = res[True][1][k], res[False][1][k]
            assert float((a - b).abs().max()) <= 2e-4 * float(b.abs().max()) + 1e-7, k
    else:                           # bf16 storage: the summed tensor is rounded once (fp32 sum in the store) instead of twice — rounding-level
        # differences, which cancellation-heavy gradients (a bias in front of the first BatchNorm) amplify: direction and length of the
        # whole gradient, and every tensor's length
        va = torch.cat([res[True][1][k].flatten() for k in res[True][1]])
        vb = torch.cat([res[False][1][k].flatten() for k in res[True][1]])
        cos = float(torch.dot(va, vb) / (va.norm() * vb.norm()))
        assert cos >= 0.999 and abs(float(va.norm() / vb.norm()) - 1) <= 1e-2, (cos, float(va.norm()), float(vb.norm()))
        for k in res[True][1]:
            a, b = res[True][1][k], res[False][1][k]
            assert float((a - b).norm()) <= 0.25 * float(b.norm()) + 1e-3 * float(vb.abs().max()), k


@pytest.mark.parametrize("c_half", [64, 40, 256])
def test_pair_coefficient_kernels_equal_two_single_launches(c_half):
    """ly_bn_finalize_pair / ly_bn_bwd_coeffs_pair (both BatchNorms of a cv1 | cv2 unit in one launch each) leave the same bits as the two
    single-unit launches they replace: scale / shift / mean / invstd, the running statistics and num_batches_tracked, dgamma / dbeta added into
    their targets, alpha / kappa / lambda"""
    from lead_yolo_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(11 + c_half)
    co, count = 2 * c_half, 4321.0
    mk = lambda: [torch.nn.BatchNorm2d(c_half, momentum=0.03, eps=1e-3).to(dev).train() for _ in range(2)]
    bns_a, bns_b = mk(), mk()
    for pa, pb in zip(bns_a, bns_b):
        w, b = torch.rand(c_half, generator=g) + 0.5, torch.randn(c_half, generator=g)
        rm, rv = torch.randn(c_half, generator=g), torch.rand(c_half, generator=g) + 0.5
        for bn in (pa, pb):
            bn.weight.data.copy_(w); bn.bias.data.copy_(b); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    s1 = torch.randn(ops.STRIPES, co, generator=g, dtype=torch.float64) * 3
    s2 = torch.rand(ops.STRIPES, co, generator=g, dtype=torch.float64) * 50 + 200
    stats = torch.cat([s1, s2], 1).contiguous().to(dev)                       # [stripes][2 co]: sums | sums of squares
    v_pair = torch.empty(4, co, dtype=torch.float32, device=dev)
    ops.bn_finalize_pair(bns_a[0], bns_a[1], stats, c_half, count, v_pair)
    v_one = torch.empty(4, co, dtype=torch.float32, device=dev)
    for i, bn in enumerate(bns_b):
        sl = slice(i * c_half, (i + 1) * c_half)
        ops.bn_finalize(bn, stats, co, count, n=c_half, c_off=i * c_half, into=(v_one[0, sl], v_one[1, sl], v_one[2, sl], v_one[3, sl]))
    assert torch.equal(v_pair, v_one)
    for pa, pb in zip(bns_a, bns_b):
        assert torch.equal(pa.running_mean, pb.running_mean) and torch.equal(pa.running_var, pb.running_var)
        assert int(pa.num_batches_tracked) == int(pb.num_batches_tracked) == 1
    sums = [torch.randn(ops.STRIPES, 2 * c_half, generator=g, dtype=torch.float64).to(dev) for _ in range(2)]
    t0 = [torch.randn(c_half, generator=g).to(dev) for _ in range(4)]
    tp, to = [t.clone() for t in t0], [t.clone() for t in t0]
    coef_p = torch.empty(3, co, dtype=torch.float32, device=dev)
    ops.bn_bwd_coeffs_pair(sums[0], sums[1], c_half, count, v_pair, ((tp[0], tp[1]), (tp[2], tp[3])), coef_p)
    coef_o = torch.empty(3, co, dtype=torch.float32, device=dev)
    for i in range(2):
        sl = slice(i * c_half, (i + 1) * c_half)
        ops.bn_bwd_coeffs(sums[i], c_half, count, v_one[0, sl], v_one[2, sl], v_one[3, sl], True, dgamma=to[2 * i], dbeta=to[2 * i + 1],
                          into=(coef_o[0, sl], coef_o[1, sl], coef_o[2, sl]))
    assert torch.equal(coef_p, coef_o)
    for a, b in zip(tp, to):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows,c", [(25600, 160), (1000, 256), (37, 8), (4099, 64)])
def test_chan_moments_striped_and_folded(rows, c, dtype):
    """ly_chan_moments (four rows in flight, ~16 rows per row group) against float64 sums of the stored values; the striped accumulators folded
    by torch equal the kernel's own fold"""
    from lead_yolo_amd import ops
    g = torch.Generator().manual_seed(rows + c)
    x = (torch.randn(rows, c, generator=g) * 2 + 0.3).to(dtype).to(_dev())
    folded = ops.chan_moments(x, c, rows, c, f64=True)
    striped = ops.chan_moments(x, c, rows, c, striped=True)
    xd = x.double()
    want = torch.cat([xd.sum(0), (xd * xd).sum(0)])
    torch.testing.assert_close(folded, want, rtol=1e-6, atol=1e-6 * rows)
    torch.testing.assert_close(striped.sum(0), want, rtol=1e-6, atol=1e-6 * rows)


def test_se_bwd_reads_double_accumulators():
    """ly_se_bwd with d_ca handed over as float64 (what ly_rf1_bwd / ly_rf3s_bwd accumulate) equals the float32 call on the rounded values"""
    from lead_yolo_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    n, c, r, hw, slices = 6, 160, 10, 400, 5
    part = torch.randn(n, slices, c, generator=g).to(dev)
    wa, wb = (torch.randn(r, c, generator=g) * 0.1).to(dev), (torch.randn(c, r, generator=g) * 0.1).to(dev)
    ca = torch.rand(n, c, generator=g).to(dev) * 0.8 + 0.1
    d64 = torch.randn(n, c, generator=g, dtype=torch.float64).to(dev)
    d32 = d64.float()
    outs = []
    for d in (d64, d32):
        dwa, dwb = torch.zeros_like(wa), torch.zeros_like(wb)
        dgap = ops.se_bwd(part, n, hw, c, wa, wb, r, ca, d, dwa, dwb)
        outs.append((dgap, dwa, dwb))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
