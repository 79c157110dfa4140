"""bf16 storage path (BASELINE.json configs[2]-[4]: bf16 activations / saved tensors / activation gradients, plain bf16 MFMA
products, fp32 accumulation, fp32 BatchNorm statistics and master weights) vs the fp32 oracle.

Tolerance (stated, not tuned per case): every tensor that crosses HBM is rounded to bf16 (relative 2^-9 per element), every
product uses bf16-rounded operands.  For a module with R rounding stages between input and output the relative L2 error is
bounded by ~R * 2^-8; R <= 8 for the deepest fused module (C3_CA with n = 3), so modules must satisfy
    ||got - want|| <= 8 * 2^-8 * ||want||   (= 3.1e-2)       and      max|got - want| <= 2^-4 * max|want|
(the second catches single wild elements).  Gradients of smooth modules: twice that bound on the relative L2 error, cosine >= 0.995.
Modules that ROUTE gradients through a discrete choice — SPPF's max-pools (rounding to bf16 creates exact ties inside the 5x5
windows, the winner then follows the scan-order rule instead of the fp32 order) and RFCBAMConv (max over channels, ReLU kinks of
G at 2^-9 relative perturbations) — are not Lipschitz in the perturbation: a flipped choice moves a whole gradient entry.  They
get a direction bound (cosine >= 0.98) and a 15 % relative-L2 bound, and the routing itself is pinned exactly by
test_sppf_pool_bf16_ties_follow_aten (same bf16-valued input, fp32 reference: identical winners).
The fp32 path keeps its 1e-3 elementwise bound (tests/test_gpu_modules.py)."""
import copy

import numpy as np
import pytest
import torch

from oracle import functional as OF
from oracle import synth
from tests import golden_util as G
from tests.test_gpu_backward import _sink_on, _with_sink_cases
from tests.test_gpu_modules import CASES, GOLDEN_MODULES, _bn_eps, _cfg, _ctor, _dev, _load, _oracle

pytestmark = pytest.mark.gpu

REL_L2 = 8 * 2.0 ** -8
MAX_REL = 2.0 ** -4
BF = torch.bfloat16


def _close(got, want, what, rel=REL_L2, mx=MAX_REL):
    got = got.detach().float().cpu()
    want = want.detach().float().cpu() if isinstance(want, torch.Tensor) else torch.from_numpy(np.asarray(want)).float()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    nw = float(want.norm())
    l2 = float((got - want).norm()) / max(nw, 1e-12)
    me = float((got - want).abs().max()) / max(float(want.abs().max()), 1e-12)
    assert l2 <= rel and me <= mx, f"{what}: relative L2 {l2:.3e} (bound {rel:.2e}), max error / max |want| {me:.3e} (bound {mx:.2e})"
    return l2


@pytest.mark.parametrize("name", G.names("basicstage") + GOLDEN_MODULES)
def test_module_eval_golden_bf16(name):
    """every hot-path module, bf16 storage, vs the vectors the reference itself produced (fp32)"""
    meta, arr = G.load(name)
    st = G.state_for(meta)
    x = synth.synth_input(meta["in_shape"], meta["seed"] + 1)
    m = _bn_eps(_load(_ctor(meta["kind"])(*meta["ctor"]), st)).to(_dev()).eval()
    with torch.no_grad():
        y = m(x.to(_dev()).to(BF))
    assert y.dtype == BF
    _close(y, arr["y_eval"], name)


@pytest.mark.parametrize("kind,ctor,shape", CASES)
def test_module_shapes_vs_oracle_bf16(kind, ctor, shape):
    """real layer shapes, ragged tiles, odd sizes, n>1 bottlenecks, shortcut — bf16 storage"""
    if kind == "RFCBAMConv" and ctor[0] % 8:
        pytest.skip("bf16 needs channels % 8 == 0")
    torch.manual_seed(0)
    m = _ctor(kind)(*ctor)
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 9000 + sum(shape) + len(kind))
    _bn_eps(_load(m, st))
    x = synth.synth_input(shape, 31 + shape[1])
    want = _oracle(kind, list(ctor), st, x)
    with torch.no_grad():
        got = m.to(_dev()).eval()(x.to(_dev()).to(BF))
    assert got.dtype == BF
    _close(got, want, f"{kind}{ctor} {shape}")


TRAIN_MODULES = G.names("basicstage") + G.names("patch") + G.names("coordatt") + G.names("cabottleneck") + G.names("c3ca") + G.names("sppf") \
    + G.names("rfcbam")


@pytest.mark.parametrize("name", TRAIN_MODULES)
def test_module_train_forward_and_backward_bf16(name):
    """train-mode forward (batch-statistics BN from fp32 accumulators), running-stat updates and the input gradient, bf16 storage,
    vs the reference's fp32 vectors"""
    meta, arr = G.load(name)
    st = G.state_for(meta)
    x = synth.synth_input(meta["in_shape"], meta["seed"] + 1)
    m = _bn_eps(_load(_ctor(meta["kind"])(*meta["ctor"]), st)).to(_dev()).train()
    image = x.shape[1] == 3
    xd = x.to(_dev()) if image else x.to(_dev()).to(BF).requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        y = m(xd)
    assert y.dtype == BF
    _close(y, arr["y_train"], name + " y_train")
    sd = m.state_dict()
    for k in arr:
        if k.startswith("post_"):
            _close(sd[k[5:]], arr[k], name + " " + k)
    if image or "dx_train" not in arr:
        return
    # the fixture's cotangent: the generator recipe of oracle/gen_golden.py (r = synth_input(y.shape, seed + 2))
    dy = synth.synth_input(tuple(arr["y_train"].shape), meta["seed"] + 2)
    y.backward(dy.to(_dev()).to(BF))
    got, want = xd.grad.float().cpu(), torch.from_numpy(arr["dx_train"])
    cos = float((got * want).sum() / (got.norm() * want.norm()))
    routing = meta["kind"] in ("SPPF", "RFCBAMConv")
    assert cos >= (0.98 if routing else 0.995), (name, cos)
    _close(got, want, name + " dx", rel=0.15 if routing else 2 * REL_L2, mx=2.0 if routing else 4 * MAX_REL)     # routing: single entries may move by their whole value


@pytest.mark.parametrize("ctor,shape,sink", _with_sink_cases(
    [((64, 64, 3, 2), (2, 64, 24, 24)), ((128, 128, 3, 2), (2, 128, 16, 16)), ((256, 256, 3, 2), (1, 256, 16, 16)),
     ((32, 48, 3, 1), (2, 32, 9, 14)), ((64, 128, 1, 1), (2, 64, 12, 12))], lambda case: True))
def test_rfcbam_backward_bf16_smooth_case(ctor, shape, sink, monkeypatch):
    """RFCBAMConv backward in bf16 WITHOUT routing decisions, at the smooth-module bound (the 15 % band of the routing modules
    must not be the only check of ly_rf*_bwd / ly_rf3c_bwd / ly_rf1_bwd).  Both BatchNorms get gamma = 0.1, beta = 1: every pre-ReLU value
    is 1 + 0.1 * xhat > 0 (no kinks), channel 0's generate-BatchNorm gets beta = 2: the channel maximum is channel 0 everywhere, by a
    margin no bf16 rounding closes (no flipped arg-max), and SE's hidden ReLU sees positive weights on a positive pooled input.  What is left is smooth, so the input gradient and the weight gradients must meet
    2 * 8 * 2^-8 relative L2 and cosine >= 0.995 against the fp32 oracle — a wrong-by-10 % tap weight in any backward kernel fails this.  sink: the same, with the parameter gradients written
    straight into an optimiser's storage (rows 0-1: recompute route, row 2: streamed with ly_rf3s_bwd, row 3: stride 1, row 4: k = 1)."""
    from tests.test_gpu_backward import _oracle_grads
    c, o, k, s = ctor
    torch.manual_seed(0)
    m = _ctor("RFCBAMConv")(*ctor)
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 7300 + c + o + k)
    kk = k * k
    st["generate.1.weight"] = torch.full_like(st["generate.1.weight"], 0.1)
    gb = torch.ones_like(st["generate.1.bias"])
    gb[:kk] = 2.0                                                    # generate channels are (c, tap) = c * k^2 + tap: channel 0 dominates every tap
    st["generate.1.bias"] = gb
    st["conv.1.weight"] = torch.full_like(st["conv.1.weight"], 0.1)
    st["conv.1.bias"] = torch.ones_like(st["conv.1.bias"])
    st["se.fc.0.weight"] = st["se.fc.0.weight"].abs()              # SE's hidden ReLU: positive weights on a positive pooled input (x + 1 below)
    _bn_eps(_load(m, st))
    x = synth.synth_input(shape, 41 + c) + 1.0
    ho, wo = (shape[2] + 2 * (k // 2) - k) // s + 1, (shape[3] + 2 * (k // 2) - k) // s + 1
    r = synth.synth_input((shape[0], o, ho, wo), 43 + o)
    y0, dx0, g0 = _oracle_grads("RFCBAMConv", list(ctor), st, x, r)
    m = m.to(_dev()).train()
    if sink:                                                     # the parameter gradients go straight into an optimiser's storage
        _sink_on(m, monkeypatch)
    xt = x.to(_dev()).to(BF).requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        y = m(xt)
    assert y.dtype == BF and float(y0.min()) > 0.2               # the oracle's outputs confirm: no output sits at a ReLU kink
    y.backward(r.to(_dev()).to(BF))
    _close(y, y0, f"{ctor} y")
    checks = [("dx", xt.grad, dx0)] + [(kname, dict(m.named_parameters())[kname].grad, g0[kname])
                                       for kname in ("conv.0.weight", "generate.0.weight", "generate.1.weight", "generate.1.bias", "conv.1.weight",
                                                     "se.fc.0.weight", "se.fc.2.weight", "get_weight.0.weight")]
    for what, got, want in checks:
        got, want = got.detach().float().cpu().flatten(), want.float().flatten()
        cos = float(got @ want / (got.norm() * want.norm()))
        l2 = float((got - want).norm() / want.norm())
        assert cos >= 0.995 and l2 <= 2 * REL_L2, (ctor, what, cos, l2)


@pytest.mark.parametrize("ctor,shape", [((64, 64, 3, 2), (2, 64, 16, 16)), ((128, 128, 3, 2), (2, 128, 24, 20)), ((256, 256, 3, 2), (1, 256, 14, 18)),
                                        ((32, 64, 3, 1), (2, 32, 9, 14)), ((128, 128, 3, 2), (3, 128, 80, 80)), ((256, 256, 3, 2), (2, 256, 40, 40)),
                                        ((512, 512, 3, 2), (1, 512, 12, 12))])
def test_rf3m_generate_on_matrix_cores_vs_oracle(ctor, shape, monkeypatch):
    """RFCBAMConv k = 3, bf16 inference on csrc/ly_rf3m.hip (the depthwise `generate` as block-diagonal MFMA products whose accumulators feed the
    main contraction in registers; models/rfa.py:113-129): the module output against the fp32 oracle at the bf16 module bound, and the kernel's
    intermediates — the [max_c, mean_c] map and the SE pooling sums — against the lane = channel kernels (fp32 generate weights: the MFMA
    form rounds them to bf16, 2^-9 relative).  The size threshold of the dispatch is lifted so that the small shapes take these kernels too;
    ragged tiles, tiles at image borders, stride 1, C up to 512 and both output-channel block sizes are covered."""
    from lead_yolo_amd import modules as M, ops
    c, o, k, s = ctor
    monkeypatch.setattr(ops, "RF3M_MIN_UNITS", 0)
    torch.manual_seed(0)
    m = _ctor("RFCBAMConv")(*ctor)
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 1234 + c + shape[2])
    _bn_eps(_load(m, st))
    x = synth.synth_input(shape, 99 + c).to(BF).float()
    with torch.no_grad():
        want = OF.rfcbam(copy.deepcopy(st), "", x, k, s, False)
    m = m.to(_dev()).eval().bfloat16()
    xd = x.to(_dev()).to(BF).contiguous(memory_format=torch.channels_last)
    calls = []
    real = ops.rf3m_fwd
    monkeypatch.setattr(ops, "rf3m_fwd", lambda **kw: (calls.append(1), real(**kw))[1])
    with torch.no_grad():
        y = m(xd)
    assert calls, "the module did not take the ly_rf3m path"
    _close(y, want, f"rf3m {ctor} {shape}")
    xr, ld = ops.rows(xd)
    n, _, h, w = xr.shape
    ho, wo = (h + 2 - 3) // s + 1, (w + 2 - 3) // s + 1
    P = m._packed(ops.planes_of(xr))
    mm_c, part_c = ops.rf3c_stats(xr, ld, n, h, w, c, s, P["wq_c"], *ops.pick_tile_c(ho, wo, s))
    mm_m, part_m = ops.rf3m_stats(xr, ld, n, h, w, c, s, P["wm_stats"], *ops.pick_tile_m(ho, wo, s))
    _close(mm_m, mm_c, f"rf3m {ctor} [max, mean] map", rel=4 * 2.0 ** -9, mx=8 * 2.0 ** -8)
    _close(part_m.sum(1), part_c.sum(1), f"rf3m {ctor} pooling sums", rel=1e-5, mx=1e-5)


def test_rf3c_backward_bit_stable_beside_mfma_stream():
    """the recompute backward of RFCBAMConv k = 3 (csrc/ly_rf3c_bwd.hip: hand-written v_pk_fma_f32 with op_sel weight broadcasts,
    no atomics) must return the SAME BITS when other waves issue MFMAs on its CUs.  The same backward runs alone, then repeatedly while a
    second stream keeps the matrix cores busy with zero-LDS bf16 GEMMs (torch.matmul) — what a second process on the GPU, an eval stream or an
    overlapped all-reduce look like to these kernels.  tools/pkfma_probe.hip holds the instruction-level experiment (seven forms of the packed
    FMA beside an MFMA aggressor: bit-exact vs the host's fmaf in all of them)."""
    torch.manual_seed(0)
    ctor, shape = (64, 64, 3, 2), (4, 64, 48, 48)
    c, o, k, s = ctor
    m = _ctor("RFCBAMConv")(*ctor)
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 9100)
    _bn_eps(_load(m, st))
    m = m.to(_dev()).train()
    x = synth.synth_input(shape, 77).to(_dev()).to(BF)
    r = synth.synth_input((shape[0], o, shape[2] // s, shape[3] // s), 78).to(_dev()).to(BF)
    names = ("conv.0.weight", "generate.0.weight", "generate.1.weight", "generate.1.bias", "se.fc.0.weight", "se.fc.2.weight", "get_weight.0.weight")

    def run():
        for p in m.parameters():
            p.grad = None
        xt = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=BF):
            y = m(xt)
        y.backward(r)
        torch.cuda.synchronize()
        return [xt.grad.clone()] + [dict(m.named_parameters())[n].grad.clone() for n in names]

    base = run()
    again = run()
    stable_alone = [torch.equal(a, b) for a, b in zip(base, again)]
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=_dev(), dtype=BF)
    bad = []
    for it in range(12):
        with torch.cuda.stream(side):
            for _ in range(40):
                a = torch.matmul(a, a) * 1e-3
        got = run()
        for nm, g0, g1, ok in zip(("dx",) + names, base, got, stable_alone):
            if ok and not torch.equal(g0, g1):
                bad.append((it, nm, float((g0.float() - g1.float()).abs().max())))
        side.synchronize()
    if not any(stable_alone):
        pytest.skip("no gradient of this module is bit-stable between two runs ALONE (batch-statistics atomics upstream): nothing to compare")
    assert not bad, f"RFCBAMConv backward changed bits beside an MFMA stream: {bad[:6]}"


def test_sppf_pool_bf16_ties_follow_aten():
    """the three chained 5x5 max-pools and their backward on a bf16 map FULL of exact ties (values drawn from 16 levels): forward
    values and the gradient routing (first maximum in row-major scan order, ATen's rule) must equal the fp32 CPU reference on
    the same values — only the bf16 rounding of the summed gradients separates them"""
    import torch.nn.functional as F
    from lead_yolo_amd import grad
    g = torch.Generator().manual_seed(5)
    y = (torch.randint(0, 16, (2, 32, 20, 20), generator=g).float() / 4 - 2)
    dy = synth.synth_input((2, 128, 20, 20), 6).to(BF).float()
    yc = y.clone().requires_grad_(True)
    p1 = F.max_pool2d(yc, 5, 1, 2); p2 = F.max_pool2d(p1, 5, 1, 2); p3 = F.max_pool2d(p2, 5, 1, 2)
    ref = torch.cat((yc, p1, p2, p3), 1)
    (ref * dy).sum().backward()
    yd = y.to(_dev()).to(BF).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out = grad.SppfPool.apply(yd, 5)
    assert out.dtype == BF and torch.equal(out.float().cpu(), ref.detach())
    out.backward(dy.to(_dev()).to(BF))
    got, want = yd.grad.float().cpu(), yc.grad
    assert float((got - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max())


@pytest.mark.parametrize("scale,hw,bs", [("n", (64, 64), 2), ("s", (640, 640), 2), ("l", (320, 320), 1), ("n", (640, 640), 1), ("l", (1280, 1280), 1)])
def test_whole_model_eval_bf16(scale, hw, bs):
    """whole detector, bf16 storage end to end (image fp32 -> PatchEmbed writes bf16), decoded rows vs the fp32 oracle.  24 layers
    deep: the bound is the per-module one times sqrt(depth)."""
    import lead_yolo_amd as L
    torch.manual_seed(0)
    m = L.Model(_cfg(scale))
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 6100 + hw[0])
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    m.load_state_dict(st)
    x = synth.synth_images(bs, max(hw), 11)[:, :, :hw[0], :hw[1]].float() / 255
    with torch.no_grad():
        zo, outs_o = OF.model_forward(copy.deepcopy(st), _cfg(scale), x, m.stride, training=False)
        with torch.autocast("cuda", dtype=BF):
            z, outs = m.to(_dev()).eval()(x.to(_dev()))
    assert z.dtype == torch.float32          # decoded rows and raw maps leave Detect as fp32
    for i, (a, b) in enumerate(zip(outs, outs_o)):
        _close(a, b, f"model_{scale} {hw} p{i}", rel=5 * REL_L2, mx=8 * MAX_REL)
    _close(z, zo, f"model_{scale} {hw} z", rel=5 * REL_L2, mx=8 * MAX_REL)


# l: configs[4]'s model at a size the oracle finishes in seconds; its 3x deeper C3_CA stacks amplify the bf16 perturbation faster (the fourth
# loss is already 6 % off while the first three are within 0.02 / 0.5 / 1.9 %), so three steps are compared
@pytest.mark.parametrize("scale,hw,steps", [("n", 128, 4), ("s", 160, 4), ("l", 128, 3)])
def test_training_trajectory_bf16(scale, hw, steps):
    """configs[2] arithmetic end to end at a size the CPU oracle finishes in seconds: `steps` optimisation steps under autocast(bf16)
    (bf16 forward / backward, fp32 loss, fp32 master weights, clip, SGD-nesterov) follow the fp32 oracle's loss trajectory.  bf16
    perturbs every activation by 2^-9: losses must agree to 3 %, and the run must learn (loss falls as the oracle's does)."""
    import lead_yolo_amd as L
    cfg = _cfg(scale)
    torch.manual_seed(0)
    m = L.Model(cfg)
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 8181)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    m.load_state_dict(st)
    imgs = synth.synth_images(4, hw, 31)
    tg = synth.synth_targets(4, 32, per_image=3)
    lr, mom, wd = 0.01, 0.937, 5e-4
    so = {k: v.clone() for k, v in st.items()}
    params = {k: v for k, v in so.items() if v.is_floating_point() and "running" not in k and not k.endswith("anchors")}
    groups = OF.param_groups(list(so))
    groups = {g: [k for k in ks if k in params] for g, ks in groups.items()}
    bufs, want = {}, []
    for _ in range(steps):
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
    m = m.to(_dev()).train()
    opt = L.smart_optimizer(m, "SGD", lr, mom, wd)
    cl = L.ComputeLoss(m)
    got = []
    for _ in range(steps):
        loss, _ = L.train_step(m, cl, opt, imgs.to(_dev()), tg.to(_dev()), amp=BF)
        got.append(float(loss))
    assert all(p.dtype == torch.float32 for p in m.parameters())          # fp32 master weights
    for a, b in zip(got, want):
        assert abs(a - b) <= 3e-2 * abs(b), (got, want)
    assert got[-1] < (0.75 if steps >= 4 else 0.85) * got[0]


def test_whole_model_gradients_bf16():
    """full-model parameter gradients of one bf16 step vs the fp32 oracle: direction (cosine over all parameters) and size"""
    import lead_yolo_amd as L
    cfg = _cfg("n")
    torch.manual_seed(0)
    m = L.Model(cfg)
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 5151)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    m.load_state_dict(st)
    imgs = synth.synth_images(4, 128, 21).float() / 255
    tg = synth.synth_targets(4, 22, per_image=3)
    so = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k and not k.endswith("anchors") else v.clone())
          for k, v in st.items()}
    pred = OF.model_forward(so, cfg, imgs, m.stride, training=True)
    loss_o, _ = OF.compute_loss(pred, tg, so["model.23.anchors"], nc=1)
    loss_o.backward()
    m = m.to(_dev()).train()
    with torch.autocast("cuda", dtype=BF):
        loss, _ = L.ComputeLoss(m)(m(imgs.to(_dev())), tg.to(_dev()))
    loss.backward()
    assert abs(float(loss) - float(loss_o)) <= 2e-2 * abs(float(loss_o))
    dot = nn = no = 0.0
    for k, p in m.named_parameters():
        g, w = p.grad.float().cpu().double(), so[k].grad.double()
        dot += float((g * w).sum()); nn += float((g * g).sum()); no += float((w * w).sum())
    cos = dot / (nn ** 0.5 * no ** 0.5)
    # direction over all 0.8 M parameters: rounding flips a fraction of the ReLU / max / argmax decisions of 24 layers (see the
    # module docstring), which perturbs the full gradient by ~sqrt(fraction); the fp32 path's bound on the same quantity is 0.9995
    assert cos >= 0.975 and 0.9 <= (nn / no) ** 0.5 <= 1.1, (cos, (nn / no) ** 0.5)


@pytest.mark.parametrize("c,n,h,w", [(24, 12, 160, 160), (40, 24, 80, 80), (16, 8, 128, 128), (64, 2, 24, 20), (96, 1, 9, 31)])
def test_mlpblock_persistent_kernel_bf16(c, n, h, w):
    """the persistent patch-walk form of the fused MLPBlock (weights in LDS, double-buffered patches), bf16 storage; the last two widths
    are not among the fused kernel's and take the composed path (dim % 32 == 0 in bf16 storage)"""
    import lead_yolo_amd as L
    torch.manual_seed(c)
    m = L.BasicStage(c, 1)
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 5000 + c)
    _bn_eps(_load(m, st))
    x = synth.synth_input((n, c, h, w), 77 + c)
    with torch.no_grad():
        want = OF.basic_stage(copy.deepcopy(st), "", x, False)
        got = m.to(_dev()).eval()(x.to(_dev()).to(BF))
    _close(got, want, f"basicstage c={c} {n}x{h}x{w} bf16")


@pytest.mark.parametrize("n,h,w", [(24, 40, 40), (21, 40, 40), (9, 61, 67), (40, 31, 29)])
def test_mlpblock_resident_weights_kernel_bf16(n, h, w):
    """C = 80 at >= 128 runs of 256 pixels: the resident-weights form (csrc/ly_mlpblock_res.hpp: one LDS copy of the fragments, 8 waves,
    contiguous pixel ranges whose last run is ragged, runs that straddle images and rows), eval AND the train-mode statistics + forward,
    against the oracle; and bit for bit against the one-shot kernels, which a map wider than the halo plan (W = 80) still takes"""
    import lead_yolo_amd as L
    c = 80
    assert n * h * w >= 128 * 256 and w <= 75
    torch.manual_seed(n)
    m = L.BasicStage(c, 1)
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 5100 + n)
    _bn_eps(_load(m, st))
    x = synth.synth_input((n, c, h, w), 177 + n)
    with torch.no_grad():
        want = OF.basic_stage(copy.deepcopy(st), "", x, False)
        want_t = OF.basic_stage(copy.deepcopy(st), "", x, True)
        md = m.to(_dev())
        got = md.eval()(x.to(_dev()).to(BF))
        got_t = md.train()(x.to(_dev()).to(BF))
    _close(got, want, f"basicstage c=80 {n}x{h}x{w} bf16 eval (resident weights)")
    _close(got_t, want_t, f"basicstage c=80 {n}x{h}x{w} bf16 train-mode forward (resident weights)")


def test_mlpblock_resident_weights_bits_equal_one_shot():
    """the same pixels through both kernels: an [n, 80, 40, 40] map (resident-weights form) and the same values laid out as rows of an
    [n, 80, 20, 80] map's left half cannot be compared (different neighbours), so the comparison is on a 1 x 1-neighbourhood-free input:
    with the partial conv's weight zeroed except its centre tap the block is pointwise, and the two tilings must agree bit for bit"""
    import lead_yolo_amd as L
    c = 80
    m = L.BasicStage(c, 1)
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 5200)
    for k, v in st.items():
        if v.dim() == 4 and v.shape[-1] == 3:                # the partial 3x3: centre tap only
            z = torch.zeros_like(v)
            z[:, :, 1, 1] = v[:, :, 1, 1]
            st[k] = z
    _bn_eps(_load(m, st))
    md = m.to(_dev()).eval()
    x = synth.synth_input((32, c, 40, 40), 31).to(_dev()).to(BF)
    with torch.no_grad():
        a = md(x)                                            # W = 40: resident-weights kernel
        xb = x.permute(0, 2, 3, 1).reshape(16, 40, 80, c).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
        b = md(xb)                                           # W = 80: one-shot kernels
    b = b.permute(0, 2, 3, 1).reshape(32, 40, 40, c).permute(0, 3, 1, 2)
    assert torch.equal(a.float(), b.float())


def test_configs2_full_size_graphed_step():
    """BASELINE configs[2] at FULL size — lead-yolo-s, bs=64, 640x640, bf16, the captured optimisation step the bench times — through
    size-independent properties (the CPU oracle cannot run this batch in seconds):
      (a) the replayed graph's loss equals the eager step's loss from the same restored state (float sums of the loss kernel);
      (b) every gradient-carrying state tensor (weights, momentum buffers, EMA) is finite after the step, the weights moved, and the replay
          and two eager steps leave the same bits;
      (c) train-mode BatchNorm couples the images of a batch, eval mode does not: eight sampled images of the batch replayed ALONE
          through the fp32 oracle in eval mode agree with the HIP model's rows of the full batch within the whole-model bf16 bound."""
    import lead_yolo_amd as L
    from lead_yolo_amd import pack
    torch.manual_seed(0)
    cfg = _cfg("s")
    m = L.Model(cfg)
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 7272)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    m.load_state_dict(st)
    m = m.to(_dev()).train()
    bs = 64
    imgs = synth.synth_images(bs, 640, 77).to(_dev())
    tg = synth.synth_targets(bs, 78, per_image=7).to(_dev())
    opt = L.smart_optimizer(m, "SGD", 0.01, 0.937, 5e-4)
    ema = L.ModelEMA(m)
    cl = L.ComputeLoss(m)
    step = L.GraphedTrainStep(m, cl, opt, imgs, tg, ema=ema, amp=BF, warmup=2)

    def tensors():
        return ({k: v for k, v in m.state_dict().items() if v.is_floating_point()},
                {k: v for k, v in ema.ema.state_dict().items() if v.is_floating_point()},
                {n: opt.state[p]["momentum_buffer"] for n, p in m.named_parameters() if p in opt.state})

    def snap():
        torch.cuda.synchronize()
        return [{k: v.detach().clone() for k, v in d.items()} for d in tensors()], opt._table["hyper"].clone(), ema.updates

    def restore(s):
        with torch.no_grad():
            for live, saved in zip(tensors(), s[0]):
                for k, v in live.items():
                    v.copy_(saved[k])
            opt._table["hyper"].copy_(s[1])
        ema.updates = s[2]
        pack.touch_weights()
    s0 = snap()
    outs = []
    for how in ("eager", "eager", "graph"):
        restore(s0)
        loss = step(imgs, tg)[0] if how == "graph" else L.train_step(m, cl, opt, imgs, tg, ema=ema, amp=BF)[0]
        outs.append((float(loss), snap()))
    (le, e), (le2, e2), (lg, g) = outs
    # (a) the forward of a step is reproducible bit for bit (double statistics accumulators, round 4): the loss of the replay and of two
    # eager steps agree to the float sums of the loss kernel
    assert np.isfinite(le) and np.isfinite(lg) and abs(le - lg) <= 1e-5 * abs(le) and abs(le - le2) <= 1e-5 * abs(le), (le, le2, lg)
    # (b) finite everywhere, and — round 4, second half: no result of the step depends on the arrival order of atomics any more — the replay
    # and two eager steps from the same state leave the SAME BITS in every weight, EMA entry and momentum buffer at the full size
    # (was: cosine >= 0.99999 / norm ratio within 1e-3; before that cosine >= 0.9, ratio 0.8 .. 1.25)
    moved = 0
    for wi in range(3):
        for k in e[0][wi]:
            assert torch.isfinite(g[0][wi][k]).all(), k
            moved += int(not torch.equal(g[0][wi][k], s0[0][wi][k]))
        bad_e = [k for k in e[0][wi] if not torch.equal(e[0][wi][k], e2[0][wi][k])]
        bad_g = [k for k in e[0][wi] if not torch.equal(e[0][wi][k], g[0][wi][k])]
        assert not bad_e, (wi, "two eager steps differ", len(bad_e), bad_e[:6])
        assert not bad_g, (wi, "graph replay differs from the eager step", len(bad_g), bad_g[:6])
    assert moved > 500
    # (c) eval rows of single images vs the oracle on the same (restored) weights
    restore(s0)
    so = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    m.eval()
    with torch.no_grad():
        with torch.autocast("cuda", dtype=BF):
            z, _ = m(imgs.float() / 255)
        for i in (0, 5, 13, 22, 31, 41, 50, 63):
            zo, _ = OF.model_forward(copy.deepcopy(so), cfg, imgs[i:i + 1].cpu().float() / 255, m.stride, training=False)
            _close(z[i:i + 1], zo, f"configs[2] image {i} of the bs=64 batch", rel=5 * REL_L2, mx=8 * MAX_REL)


@pytest.mark.parametrize("bs", [2, 16])
def test_configs4_shape_lead_yolo_l_1280(bs):
    """BASELINE configs[4]'s shape on one GPU: lead-yolo-l, 1280x1280, bf16, at bs=2 and at the REAL per-GPU batch of 16 (7.9 GiB peak):
    one captured optimisation step equals the eager step from the same state, everything stays finite, and the large-map kernels
    (160 x 160 ... 320 x 320 feature maps, 1024-wide C3_CA, 26 M pixel rows at bs=16) run inside their index limits."""
    import lead_yolo_amd as L
    from lead_yolo_amd import pack
    torch.manual_seed(0)
    m = L.Model(_cfg("l")).to(_dev()).train()
    imgs = synth.synth_images(bs, 1280, 91).to(_dev())
    tg = synth.synth_targets(bs, 92, per_image=7).to(_dev())
    opt = L.smart_optimizer(m, "SGD", 0.01, 0.937, 5e-4)
    cl = L.ComputeLoss(m)
    step = L.GraphedTrainStep(m, cl, opt, imgs, tg, amp=BF, warmup=2)
    w0 = {k: v.detach().clone() for k, v in m.state_dict().items() if v.is_floating_point()}
    b0 = {n: opt.state[p]["momentum_buffer"].detach().clone() for n, p in m.named_parameters() if p in opt.state}
    h0 = opt._table["hyper"].clone()

    def restore():
        with torch.no_grad():
            for k, v in m.state_dict().items():
                if k in w0:
                    v.copy_(w0[k])
            for n, p in m.named_parameters():
                if n in b0:
                    opt.state[p]["momentum_buffer"].copy_(b0[n])
            opt._table["hyper"].copy_(h0)
        pack.touch_weights()
    outs = []
    for how in ("eager", "eager", "graph"):
        restore()
        loss = step(imgs, tg)[0] if how == "graph" else L.train_step(m, cl, opt, imgs, tg, amp=BF)[0]
        torch.cuda.synchronize()
        outs.append((float(loss), {k: v.detach().clone() for k, v in m.state_dict().items() if k in w0}))
    (le, we), (le2, we2), (lg, wg) = outs
    assert np.isfinite(le) and np.isfinite(lg) and abs(le - lg) <= 1e-5 * abs(le) and abs(le - le2) <= 1e-5 * abs(le), (le, le2, lg)
    dg, de, de2 = [], [], []
    for k in we:
        assert torch.isfinite(wg[k]).all(), k
        dg.append((wg[k] - w0[k]).flatten()); de.append((we[k] - w0[k]).flatten()); de2.append((we2[k] - w0[k]).flatten())
    dg, de, de2 = torch.cat(dg).double(), torch.cat(de).double(), torch.cat(de2).double()
    cos = float(dg @ de / (dg.norm() * de.norm()))
    cos_noise = float(de2 @ de / (de2.norm() * de.norm()))
    # (round 4: reproducible forward + double accumulators wherever a sum feeds an activation gradient: the replay's update equals the eager one)
    assert cos >= 0.99999 and cos_noise >= 0.99999 and abs(float(dg.norm() / de.norm()) - 1) <= 1e-3, (cos, cos_noise)


@pytest.mark.parametrize("c,n,h,w", [(24, 2, 40, 48), (24, 3, 13, 32), (40, 3, 24, 32), (24, 2, 20, 20), (40, 1, 7, 9), (16, 2, 16, 64), (40, 2, 33, 80),
                                     (80, 2, 20, 24), (80, 3, 40, 40), (80, 1, 5, 7), (160, 2, 20, 20), (160, 1, 16, 32)])
def test_mlpblock_fused_backward_bf16(c, n, h, w, monkeypatch):
    """The fused MLPBlock backward (csrc/ly_mlpblock_bwd.hpp: two passes over (x, dy), the 2C-wide hidden tensors and both 1x1 weight
    gradients on chip; reference: autograd of models/common.py:1432-1437, 1478-1482) — T2D patches (W % 16 == 0, ragged H included) and
    flattened runs (any W, tiles spanning images) — against (a) autograd through the fp32 oracle on the same bf16-rounded input, at the bf16
    bound for smooth modules, and (b) the unfused HIP backward (eleven launches, hidden tensors rounded to bf16 in HBM): the two must agree
    more tightly with each other than either does with fp32.  Running statistics and the forward are untouched by the switch."""
    import lead_yolo_amd as L
    from lead_yolo_amd import ops
    from tests.test_gpu_backward import _oracle_grads
    torch.manual_seed(c)
    st = synth.synth_state(synth.shapes_of(L.BasicStage(c, 1).state_dict()), 6100 + c + w)
    x = synth.synth_input((n, c, h, w), 177 + c + h).to(BF).float()
    r = synth.synth_input((n, c, h, w), 178 + c + h).to(BF).float()
    _, dxo, gpo = _oracle_grads("BasicStage", [c, 1], st, x, r)

    def run(fused):
        monkeypatch.setattr(ops, "MLP_BWD_FUSED", fused)
        m = _bn_eps(_load(L.BasicStage(c, 1), copy.deepcopy(st))).to(_dev()).train()
        xt = x.to(_dev()).to(BF).requires_grad_(True)
        with torch.autocast("cuda", dtype=BF):
            y = m(xt)
        y.backward(r.to(_dev()).to(BF))
        return xt.grad.float().cpu(), {k: p.grad.float().cpu() for k, p in m.named_parameters()}

    dxf, gf = run(True)
    dxu, gu = run(False)
    what = f"mlpblock fused bwd c={c} {n}x{h}x{w}"
    _close(dxf, dxo, what + " dx vs oracle", rel=2 * REL_L2, mx=4 * MAX_REL)
    _close(dxf, dxu, what + " dx vs unfused", rel=REL_L2, mx=2 * MAX_REL)
    for k, want in gpo.items():
        assert gf[k] is not None, (what, k)
        cos = float((gf[k] * want).sum() / (gf[k].norm() * want.norm() + 1e-30))
        assert cos >= 0.995, (what, k, cos)
        _close(gf[k], want, f"{what} d{k} vs oracle", rel=2 * REL_L2, mx=4 * MAX_REL)
        _close(gf[k], gu[k], f"{what} d{k} vs unfused", rel=REL_L2, mx=2 * MAX_REL)
