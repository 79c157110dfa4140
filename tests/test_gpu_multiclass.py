"""Detection heads with more than one class (nc > 1), end to end on the device: Detect levels in eval and in training, whole models,
test-time augmentation, gradients, optimiser steps and val.py's NMS setting, each against a reference that does not share the kernels.
The references: a float64 restatement of Detect written out here (models/yolo.py:84-120; the CPU test below pins the oracle's own Detect to
it at nc > 1), float64 autograd for the training node, and the oracle (oracle/functional.py, oracle/nms.py) for whole models."""
import contextlib
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import functional as OF
from oracle import nms as ON
from oracle import synth
from tests.test_gpu_backward import _close as _close_max
from tests.test_gpu_bf16 import MAX_REL, REL_L2, _close as _close_l2
from tests.test_gpu_modules import ATOL, RTOL, _cmp, _dev
from tests.test_nms import oracle_keep_stable

ANCHORS = ((10, 13, 16, 30, 33, 23), (30, 61, 62, 45, 59, 119), (116, 90, 156, 198, 373, 326))
STRIDES = (8.0, 16.0, 32.0)
BF = torch.bfloat16


# ---- the float64 restatement of Detect ---------------------------------------------------------------------------------------------------
def detect64(xs, ws, bs_, anchors_px, strides, nc):
    """models/yolo.py:84-120 in float64, formula by formula: 1x1 convolution, view(bs, na, no, ny, nx).permute(0, 1, 3, 4, 2), sigmoid,
    xy = (2 s + grid - 0.5) * stride, wh = (2 s)^2 * anchor (pixels), the rest s.  -> z [bs, rows, no], list of raw maps, and per level
    |W| |x| + |b| in the raw maps' layout (the magnitude the rounding of a dot product scales with)"""
    na, no = len(anchors_px[0]) // 2, nc + 5
    z, ps, mags = [], [], []
    for x, w, b, anc, s in zip(xs, ws, bs_, anchors_px, strides):
        x, w, b = x.double(), w.double().reshape(w.shape[0], -1), b.double()
        n, _, ny, nx = x.shape
        y = torch.einsum("oc,nchw->nohw", w, x) + b.view(1, -1, 1, 1)
        mag = torch.einsum("oc,nchw->nohw", w.abs(), x.abs()) + b.abs().view(1, -1, 1, 1)
        p = y.view(n, na, no, ny, nx).permute(0, 1, 3, 4, 2).contiguous()
        mags.append(mag.view(n, na, no, ny, nx).permute(0, 1, 3, 4, 2).contiguous())
        sg = 1.0 / (1.0 + torch.exp(-p))
        gx = torch.arange(nx, dtype=torch.float64).view(1, 1, 1, nx)
        gy = torch.arange(ny, dtype=torch.float64).view(1, 1, ny, 1)
        a = torch.tensor(anc, dtype=torch.float64).view(1, na, 1, 1, 2)
        d = sg.clone()
        d[..., 0] = (sg[..., 0] * 2 + (gx - 0.5)) * s
        d[..., 1] = (sg[..., 1] * 2 + (gy - 0.5)) * s
        d[..., 2:4] = (sg[..., 2:4] * 2) ** 2 * a
        z.append(d.view(n, na * ny * nx, no))
        ps.append(p)
    return torch.cat(z, 1), ps, mags


def _level_inputs(nc, ch, grids, bs, seed, dt=torch.float32):
    g = torch.Generator().manual_seed(seed)
    co = 3 * (nc + 5)
    xs = [torch.randn(bs, c, ny, nx, generator=g).to(dt).float() for c, (ny, nx) in zip(ch, grids)]
    ws = [(torch.randn(co, c, 1, 1, generator=g) * (2.0 / c ** 0.5)).to(dt).float() for c in ch]
    bs_ = [torch.randn(co, generator=g) for _ in ch]
    return xs, ws, bs_


U32 = 2.0 ** -24          # unit roundoff of fp32


@pytest.mark.parametrize("nc", [2, 5, 80])
def test_oracle_detect_multiclass_matches_float64(nc):
    """CPU: oracle.functional.detect (what the GPU tests of whole models lean on) at nc > 1 against the float64 restatement above.
    Bound: a K-term fp32 dot product is within K u (|W| |x| + |b|) of the exact one (u = 2^-24, K <= 512); the decode is Lipschitz in the raw
    value (sigmoid' <= 1/4: xy stride / 2, wh <= 32/27 anchor, rest 1/4) and adds a few roundings of its own result."""
    ch, grids = (64, 128, 512), ((20, 21), (10, 11), (5, 6))
    xs, ws, bs_ = _level_inputs(nc, ch, grids, 2, 40 + nc)
    anchors = torch.tensor(ANCHORS).float().view(3, 3, 2) / torch.tensor(STRIDES).view(3, 1, 1)
    st = {"d.anchors": anchors}
    for i in range(3):
        st[f"d.m.{i}.weight"], st[f"d.m.{i}.bias"] = ws[i], bs_[i]
    with torch.no_grad():
        z, ps = OF.detect(st, "d.", xs, torch.tensor(STRIDES), nc)
    z64, p64, mags = detect64(xs, ws, bs_, ANCHORS, STRIDES, nc)
    assert z.shape == z64.shape == (2, 3 * (420 + 110 + 30), nc + 5)
    row = 0
    for i, (p, q, m) in enumerate(zip(ps, p64, mags)):
        tol_p = ch[i] * U32 * m
        assert bool(((p.double() - q).abs() <= tol_p).all()), (i, float((p.double() - q).abs().max()))
        n_rows = q[0].numel() // (nc + 5)
        zl = z64[:, row:row + n_rows].view(q.shape)
        anc = torch.tensor(ANCHORS[i], dtype=torch.float64).view(1, 3, 1, 1, 2)
        tol_z = 0.25 * tol_p + 16 * U32 * zl.abs()
        tol_z[..., 0:2] = STRIDES[i] / 2 * tol_p[..., 0:2] + 16 * U32 * (zl[..., 0:2].abs() + STRIDES[i] * max(grids[i]))     # (grid + 2 s) cancels
        tol_z[..., 2:4] = 32.0 / 27.0 * anc * tol_p[..., 2:4] + 16 * U32 * zl[..., 2:4].abs()
        err = (z[:, row:row + n_rows].double().view(q.shape) - zl).abs()
        assert bool((err <= tol_z).all()), (i, float((err - tol_z).max()))
        row += n_rows


# ---- item 2: Detect levels, eval ---------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _counted(*names):
    """counts the calls of lead_yolo_amd.ops functions without changing them: the tests assert which route ran"""
    from lead_yolo_amd import ops
    n = dict.fromkeys(names, 0)
    saved = {k: getattr(ops, k) for k in names}

    def wrap(k):
        def counted(*a, **kw):
            n[k] += 1
            return saved[k](*a, **kw)
        return counted
    for k in names:
        setattr(ops, k, wrap(k))
    try:
        yield n
    finally:
        for k in names:
            setattr(ops, k, saved[k])


def _cmp_z(z, z64, grids, nc, what):
    """1e-3 abs + rel; for xy / wh (pixels) the absolute part is scaled by stride * max(anchor) of the level, objectness and classes keep 1e-3"""
    got = z.detach().cpu().double()
    row = 0
    for i, (ny, nx) in enumerate(grids):
        n_rows = 3 * ny * nx
        g, w = got[:, row:row + n_rows], z64[:, row:row + n_rows]
        scale = torch.ones(nc + 5, dtype=torch.float64)
        scale[:4] = float(max(ANCHORS[i]))
        bad = (g - w).abs() > ATOL * scale + RTOL * w.abs()
        assert not bool(bad.any()), f"{what} z level {i}: {int(bad.sum())} elements off, max err {float((g - w).abs().max()):.3e}"
        row += n_rows


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("nc", [2, 3, 4, 5, 6, 80])
def test_detect_levels_multiclass_vs_float64(nc, dt):
    """L.Detect in eval at na*no = 21, 24, 27, 30 (ly_detect_level: bias guard, second weight tile partly used, LDS walk of 16 no floats per
    anchor) and 33, 255 (head GEMM to ldo = 36 / 256 columns + ly_detect_tail) on non-square grids whose last 16-pixel tile is partial and
    whose tiles straddle images, z and every raw map against float64 on the same (bf16 storage: bf16-rounded) inputs and weights.
    bf16 storage at nc >= 6 used to send the raw map through the head GEMM's bf16 buffer (max error 2.9e-2 / 3.1e-2 here); the head now
    contracts the widened feature map in fp32 storage there."""
    import lead_yolo_amd as L
    dev = _dev()
    ch = (64, 128, 256) if dt == torch.float32 else (128, 256, 512)
    grids = ((20, 21), (10, 11), (5, 6))
    xs, ws, bs_ = _level_inputs(nc, ch, grids, 3, 50 + nc, dt)
    det = L.Detect(nc=nc, anchors=ANCHORS, ch=ch)
    with torch.no_grad():
        for i in range(3):
            det.m[i].weight.copy_(ws[i])
            det.m[i].bias.copy_(bs_[i])
    det = det.to(dev).eval()
    det.stride = torch.tensor(STRIDES, device=dev)
    det.anchors /= det.stride.view(-1, 1, 1)
    with torch.no_grad(), _counted("detect_level", "detect_tail") as n:
        z, ps = det([x.to(dev).to(dt).contiguous(memory_format=torch.channels_last) for x in xs])
    assert n == ({"detect_level": 3, "detect_tail": 0} if nc <= 5 else {"detect_level": 0, "detect_tail": 3}), n
    z64, p64, _ = detect64(xs, ws, bs_, ANCHORS, STRIDES, nc)
    assert z.dtype == torch.float32 and tuple(z.shape) == tuple(z64.shape)
    for i, (a, b) in enumerate(zip(ps, p64)):
        assert a.dtype == torch.float32
        _cmp(a, b.float(), f"Detect nc={nc} p{i}")
    _cmp_z(z, z64, grids, nc, f"Detect nc={nc}")


# ---- items 3, 10: whole models -------------------------------------------------------------------------------------------------------------
def _cfg(scale, nc):
    import lead_yolo_amd as L
    cfg = L.load_cfg(scale=scale)
    cfg["nc"] = nc
    return cfg


def _model(scale, nc, seed):
    import lead_yolo_amd as L
    torch.manual_seed(0)
    cfg = _cfg(scale, nc)
    m = L.Model(cfg, nc=nc)
    assert m.model[-1].nc == nc and m.model[-1].m[0].out_channels == 3 * (nc + 5)
    st = synth.synth_state(synth.shapes_of(m.state_dict()), seed)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    m.load_state_dict(st)
    return m, st, cfg


@functools.lru_cache(maxsize=None)
def _eval_pair(scale, nc, hw, bs, amp=False):
    """(device z, device raw maps, oracle z, oracle raw maps, route counts) of one eval forward"""
    m, st, cfg = _model(scale, nc, 9000 + nc + hw[0])
    x = synth.synth_images(bs, max(hw), 11)[:, :, :hw[0], :hw[1]].float() / 255
    with torch.no_grad():
        zo, po = OF.model_forward(copy.deepcopy(st), cfg, x, m.stride, training=False)
        m = m.to(_dev()).eval()
        with _counted("detect_level", "detect_tail") as n, torch.autocast("cuda", dtype=BF, enabled=amp):
            z, p = m(x.to(_dev()))
    return z.cpu(), [t.cpu() for t in p], zo, po, dict(n)


def _routes(scale, nc, bf16=False):
    """launches per route a whole-model forward must show: nc <= 5 takes the one-launch level kernel wherever it is built — every level of
    lead-yolo-n (64 / 128 / 256 channels); lead-yolo-s' P5 has 512 channels, which is built for bf16 storage only —, nc >= 6 the tail"""
    if nc > 5:
        return {"detect_level": 0, "detect_tail": 3}
    fused = 3 if scale == "n" or bf16 else 2
    return {"detect_level": fused, "detect_tail": 3 - fused}


@pytest.mark.gpu
@pytest.mark.parametrize("scale,nc,hw,bs", [("n", 3, (96, 160), 2), ("n", 80, (96, 160), 2), ("s", 3, (96, 160), 2), ("s", 80, (96, 160), 2),
                                            ("s", 3, (640, 640), 1)])
def test_whole_model_multiclass_vs_oracle(scale, nc, hw, bs):
    z, p, zo, po, n = _eval_pair(scale, nc, hw, bs)
    assert n == _routes(scale, nc), n
    assert tuple(z.shape) == (bs, 3 * sum((hw[0] // s) * (hw[1] // s) for s in (8, 16, 32)), nc + 5)
    _cmp(z, zo, f"model_{scale} nc={nc} {hw} z")
    for i, (a, b) in enumerate(zip(p, po)):
        _cmp(a, b, f"model_{scale} nc={nc} {hw} p{i}")


@pytest.mark.gpu
@pytest.mark.parametrize("nc", [3, 80])
def test_whole_model_multiclass_bf16(nc):
    """bf16 storage end to end at nc > 1 (nc = 80: the head GEMM in fp32 storage on the widened map, then ly_detect_tail), the relative-L2 rule of test_gpu_bf16.py"""
    z, p, zo, po, n = _eval_pair("s", nc, (96, 160), 2, True)
    assert n == _routes("s", nc, True), n
    assert z.dtype == torch.float32
    for i, (a, b) in enumerate(zip(p, po)):
        _close_l2(a, b, f"bf16 nc={nc} p{i}", rel=5 * REL_L2, mx=8 * MAX_REL)
    _close_l2(z, zo, f"bf16 nc={nc} z", rel=5 * REL_L2, mx=8 * MAX_REL)


@pytest.mark.gpu
def test_graphed_forward_multiclass_matches_eager():
    import lead_yolo_amd as L
    m, _, _ = _model("s", 3, 9777)
    m = m.to(_dev()).eval()
    x1 = (synth.synth_images(2, 256, 5)[:, :, :160, :].float() / 255).to(_dev())
    x2 = (synth.synth_images(2, 256, 6)[:, :, :160, :].float() / 255).to(_dev())
    g = L.GraphedForward(m, x1)
    for x in (x1, x2, x1):
        with torch.no_grad():
            ze, pe = m(x)
        zg, pg = g(x)
        torch.cuda.synchronize()
        assert ze.shape[-1] == 8 and torch.equal(zg, ze)
        assert all(torch.equal(a, b) for a, b in zip(pg, pe))


@pytest.mark.gpu
def test_val_setting_nms_on_model_output():
    """val.py's NMS call for nc > 1 (conf_thres 0.001, multi_label) on the decoded rows of a real nc = 3 forward at 640 x 640: 75600 (box,
    class) pairs of which more than max_nms = 30000 pass, so the sorted list is cut before the greedy walk.  max_det = 300 is reached long
    before rank 30000: this case shows that the cut ran on real output, not where it falls — tests/test_nms.py's count-30000 / count-30001
    cases pin its position."""
    import lead_yolo_amd as L
    z, _, _, _, _ = _eval_pair("s", 3, (640, 640), 1)
    pred = z.numpy()
    passing = int(((pred[0, :, 4:5] > 0.001) & (pred[0, :, 5:] * pred[0, :, 4:5] > 0.001)).sum())
    assert passing > ON.MAX_NMS, passing
    kw = dict(multi_label=True, max_det=300)
    want, want_idx = oracle_keep_stable(pred, 0.001, 0.45, **kw)
    assert len(want_idx[0]) > 20
    zt = z.to(_dev())
    got = L.non_max_suppression(zt, 0.001, 0.45, **kw)
    _, count, keep = L.nms_padded(zt, 0.001, 0.45, **kw)
    assert int(count[0]) == len(want_idx[0])
    assert keep[0, :len(want_idx[0])].cpu().tolist() == want_idx[0].tolist()
    np.testing.assert_array_equal(got[0].cpu().numpy(), want[0])


# ---- item 4: test-time augmentation ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nc", [3, 6])
def test_augmented_forward_multiclass_vs_oracle(nc):
    """model(x, augment=True) at nc = 3 (ly_detect_level_aug) and nc = 6 (head GEMM + ly_detect_tail_aug) against the reference's
    _forward_augment restated over the oracle (tests/test_gpu_augment.py)"""
    from tests.test_gpu_augment import ref_forward_augment
    m, st, cfg = _model("n", nc, 7300 + nc)
    x = synth.synth_images(2, 320, 11)[:, :, :256, :].float() / 255
    with torch.no_grad():
        zo = ref_forward_augment(st, cfg, x, m.stride)
    m = m.to(_dev()).eval()
    with torch.no_grad(), _counted("detect_level_aug", "detect_tail_aug") as n:
        z, p = m(x.to(_dev()), augment=True)
    assert p is None and z.dtype == torch.float32 and z.shape[-1] == nc + 5
    assert (n["detect_level_aug"] > 0 and n["detect_tail_aug"] == 0) if nc <= 5 else (n["detect_tail_aug"] > 0 and n["detect_level_aug"] == 0), n
    _cmp(z, zo, f"augmented nc={nc}")


# ---- item 5: the training node of one Detect level ---------------------------------------------------------------------------------------------
_HEAD_GEOMS = [(2, 64, 20, 20), (1, 128, 7, 13), (3, 128, 5, 160), (3, 128, 9, 24)]          # (3, 128, 9, 24): 27 image rows, 8 per trip
# bf16 storage: du (the gradient of the head's output rows) and dx are bf16 tensors.  Largest error of float64 autograd with du and dx
# rounded to bf16 against float64 autograd without, relative to each tensor's max, over every case below, measured on the CPU
# (test_head_bf16_gap_is_what_the_bound_assumes re-measures it): dx 4.41e-3, dW 2.17e-3, dbias 2.68e-3 (dbias is not given this slack: both branches sum it before
# any rounding; the figure is kept as the re-measured record).  The bound is 4 x the gap + the fp32 bound.
_BF16_GAP = dict(dx=4.5e-3, dw=2.2e-3, db=2.7e-3)


def _head_case(nc, geom, dt):
    bs, cin, ny, nx = geom
    g = torch.Generator().manual_seed(11 + nc)
    no = nc + 5
    w = (torch.randn(3 * no, cin, 1, 1, generator=g) * 0.1).to(dt).float()
    b = torch.randn(3 * no, generator=g)
    x = torch.randn(bs, cin, ny, nx, generator=g).to(dt).float()
    r = torch.randn(bs, 3, ny, nx, no, generator=g)
    return x, w, b, r


def _head64(x, w, b, r, round_du=False):
    x, w, b, r = (t.double().clone().requires_grad_(True) for t in (x, w, b, r))
    bs, _, ny, nx = x.shape
    no = r.shape[-1]
    y = F.conv2d(x, w, b)
    if round_du:
        y.register_hook(lambda gy: gy.to(BF).double())
    p = y.view(bs, 3, no, ny, nx).permute(0, 1, 3, 4, 2)
    (p * r.detach()).sum().backward()
    dx = x.grad.to(BF).double() if round_du else x.grad
    return p.detach(), dx, w.grad, b.grad


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("nc", [2, 3, 4, 5, 6, 80])
def test_head_bf16_gap_is_what_the_bound_assumes(nc):
    """CPU: the reference-only gap _BF16_GAP is derived from, re-measured"""
    for geom in _HEAD_GEOMS if nc <= 5 else _HEAD_GEOMS[:2]:
        x, w, b, r = _head_case(nc, geom, BF)
        _, dx, dw, db = _head64(x, w, b, r)
        _, dx2, dw2, db2 = _head64(x, w, b, r, round_du=True)
        gaps = dict(dx=_rel(dx2, dx), dw=_rel(dw2, dw), db=_rel(db2, db))
        print(nc, geom, gaps)
        assert all(gaps[k] <= _BF16_GAP[k] for k in gaps), (nc, geom, gaps)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("nc", [2, 3, 4, 5, 6, 80])
def test_detect_head_node_multiclass_vs_float64(nc, dt):
    """grad.detect_head at no odd and even, cq = ceil(co / vw) vw with and without pad columns (nc = 4: 28 in fp32, 32 in bf16; nc = 3: 24,
    none), and the generic branch (nc = 6, 80), against float64 autograd of conv1x1 + view + permute on the same inputs: p, dx, dW, dbias.
    fp32: 1e-5 of each tensor's max.  bf16: p and dbias likewise (fp32 accumulators reach the raw map on both branches; the bias gradient
    is summed before any rounding), dx and dW get 4 x the reference's own gap under bf16 rounding of du / dx (_BF16_GAP) on top of that."""
    import lead_yolo_amd as L
    from lead_yolo_amd import grad
    dev = _dev()
    for geom in _HEAD_GEOMS if nc <= 5 else _HEAD_GEOMS[:2]:
        bs, cin, ny, nx = geom
        x0, w0, b0, r0 = _head_case(nc, geom, dt)
        det = L.Detect(nc=nc, anchors=(ANCHORS[0],), ch=(cin,)).to(dev).train()
        conv = det.m[0]
        with torch.no_grad():
            conv.weight.copy_(w0)
            conv.bias.copy_(b0)
        x = x0.to(dev).to(dt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        wp, _ = det._packed(0, L.ops.planes_of(x))
        with _counted("detect_head_bwd") as n:
            p = grad.detect_head(det, 0, wp, x, conv.weight, conv.bias)
            (p * r0.to(dev)).sum().backward()
        assert n["detect_head_bwd"] == (1 if nc <= 5 else 0), (nc, n)
        p64, dx64, dw64, db64 = _head64(x0, w0, b0, r0)
        what = f"nc={nc} {geom} {dt}"
        bf = dt == BF
        assert p.dtype == torch.float32
        _close_max(p, p64.float(), what + " p", rtol=1e-5)
        _close_max(x.grad, dx64.float(), what + " dx", rtol=1e-5 + (4 * _BF16_GAP["dx"] if bf else 0.0))
        _close_max(conv.weight.grad, dw64.float(), what + " dW", rtol=1e-5 + (4 * _BF16_GAP["dw"] if bf else 0.0))
        _close_max(conv.bias.grad, db64.float(), what + " dbias", rtol=1e-5)


# ---- items 6, 7: whole-model gradients and optimiser steps at nc = 3 ------------------------------------------------------------------------------
def _targets(b, seed, per_image, nc):
    tg = synth.synth_targets(b, seed, per_image=per_image)
    tg[:, 1] = torch.randint(0, nc, (tg.shape[0],), generator=torch.Generator().manual_seed(seed + 1)).float()
    assert len(set(tg[:, 1].tolist())) == nc
    return tg


@pytest.mark.gpu
def test_whole_model_gradients_multiclass_vs_oracle():
    """test_whole_model_gradients_vs_oracle (lead-yolo-s, 128 x 128) with three classes: same direction / length bounds, the head's own
    gradients (no kink between it and the loss) tight"""
    import lead_yolo_amd as L
    nc = 3
    m, st, cfg = _model("s", nc, 4343)
    x = synth.synth_images(4, 128, 17).float() / 255
    tg = _targets(4, 18, 4, nc)
    so = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k and not k.endswith("anchors") else v.clone())
          for k, v in st.items()}
    lo, io = OF.compute_loss(OF.model_forward(so, cfg, x, m.stride, training=True), tg, m.model[-1].anchors, nc=nc)
    lo.backward()
    assert float(io[2]) > 0
    m = m.to(_dev()).train()
    loss, items = L.ComputeLoss(m)(m(x.to(_dev())), tg.to(_dev()))
    loss.backward()
    assert float(items[2]) > 0
    assert abs(float(loss.detach()) - float(lo.detach())) <= 1e-3 * abs(float(lo.detach()))
    got = torch.cat([p.grad.detach().cpu().double().reshape(-1) for _, p in m.named_parameters()])
    want = torch.cat([so[k].grad.double().reshape(-1) for k, _ in m.named_parameters()])
    cos = float(torch.dot(got, want) / (got.norm() * want.norm()))
    rel = float((got - want).norm() / want.norm())
    assert cos > 0.9995 and rel < 3e-2, (cos, rel)
    for k, p in m.named_parameters():
        if k.startswith("model.23."):
            _close_max(p.grad, so[k].grad, "d" + k)


@pytest.mark.gpu
def test_training_trajectory_multiclass_vs_oracle():
    """three SGD steps at nc = 3 follow the oracle's (test_training_trajectory_vs_oracle's recipe and bounds)"""
    import lead_yolo_amd as L
    nc = 3
    m, st, cfg = _model("s", nc, 8181)
    imgs = synth.synth_images(4, 160, 31)
    tg = _targets(4, 32, 3, nc)
    lr, mom, wd = 0.01, 0.937, 5e-4
    so = {k: v.clone() for k, v in st.items()}
    params = {k: v for k, v in so.items() if v.is_floating_point() and "running" not in k and not k.endswith("anchors")}
    groups = OF.param_groups(list(so))
    groups = {g: [k for k in ks if k in params] for g, ks in groups.items()}
    bufs, want = {}, []
    for _ in range(3):
        for p in params.values():
            p.requires_grad_(True)
            p.grad = None
        loss, items = OF.compute_loss(OF.model_forward(so, cfg, imgs.float() / 255, m.stride, training=True), tg, so["model.23.anchors"], nc=nc)
        loss.backward()
        assert float(items[2]) > 0
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
    for _ in range(3):
        loss, _ = L.train_step(m, cl, opt, imgs.to(_dev()), tg.to(_dev()))
        got.append(float(loss))
    for (a, b), tol in zip(zip(got, want), (1e-4, 1e-3, 5e-3)):
        assert abs(a - b) <= tol * abs(b), (got, want)
    assert got[-1] < got[0]
