"""The options of the device loss (focal loss, gr, sort_obj_iou, autobalance) on the host: the restatement tests/lossopts_ref.py against the
oracle and the reference's vectors at neutral options, the closed-form focal gradient csrc/ly_loss.hip implements against autograd of the
literal FocalLoss, the premises of the GPU cases (tests/test_gpu_lossopts.py), the planted defects against the judges the GPU tests use, and
ComputeLoss's construction rules.  No GPU."""
import numpy as np
import pytest
import torch

from tests import golden_util as G
from tests import lossopts_ref as R

_HYP_KEYS = ("box", "cls", "cls_pw", "obj", "obj_pw", "anchor_t", "fl_gamma", "label_smoothing")
GAMMAS = (0.5, 1.5, 2.0)


class _Det:
    def __init__(self, anchors, nc=1, stride=None):
        self.na, self.nc, self.nl, self.anchors = anchors.shape[1], nc, anchors.shape[0], anchors
        if stride is not None:
            self.stride = torch.tensor(stride)


# ---- neutral options ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nc,keys", [("loss_n", 1, ("rand", "edge", "empty")), ("loss_nc3", 3, (None,))])
def test_neutral_restatement_is_the_oracle_and_the_reference(name, nc, keys):
    from oracle import functional as OF
    meta, arr = G.load(name)
    hyp = {k: meta["hyp"][k] for k in _HYP_KEYS if k in meta["hyp"]}
    anchors = G.t(arr["anchors"])
    for key in keys:
        pre = f"{key}_" if key else ""
        tg = G.t(arr[pre + "targets"])
        p32 = [G.t(arr[f"pred{i}"]).clone().requires_grad_(True) for i in range(3)]
        po = [G.t(arr[f"pred{i}"]).clone().requires_grad_(True) for i in range(3)]
        l32, i32, bal = R.compute_loss(p32, tg, anchors, nc, hyp=hyp)
        lo, io = OF.compute_loss(po, tg, anchors, nc=nc, hyp=hyp)
        l32.backward()
        lo.backward()
        assert torch.equal(l32, lo) and torch.equal(i32, io) and bal == R.default_balance(3)       # float32: the same operations
        for a, b in zip(p32, po):
            assert torch.equal(a.grad, b.grad)
        p64 = [G.t(arr[f"pred{i}"]).double().requires_grad_(True) for i in range(3)]
        l64, i64, _ = R.compute_loss(p64, tg, anchors, nc, hyp=hyp)
        l64.backward()
        np.testing.assert_allclose(l64.detach().numpy(), arr[pre + "loss"], rtol=1e-5)
        np.testing.assert_allclose(i64.numpy(), arr[pre + "items"], rtol=1e-5, atol=1e-7)
        for i in range(3):
            np.testing.assert_allclose(p64[i].grad.numpy(), arr[f"{pre}dpred{i}"], rtol=1e-4, atol=1e-7)


# ---- the focal formula ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("pw", [1.0, 0.8, 1.3])
def test_closed_form_focal_gradient_is_autograd_of_focal_loss(gamma, pw):
    xs = torch.linspace(-R.XMAX, R.XMAX, 41, dtype=torch.float64)
    zs = torch.tensor([0.0, 0.05, 0.3, 0.5, 0.77, 0.95, 1.0], dtype=torch.float64)          # hard and soft targets (tobj, cp / cn)
    x = xs[:, None].expand(-1, zs.numel()).clone().requires_grad_(True)
    z = zs[None].expand(xs.numel(), -1)
    fl = R.FocalLoss(torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([pw], dtype=torch.float64), reduction="sum"), gamma, R.ALPHA)
    total = fl(x, z)
    total.backward()
    val, grad = R.focal_closed_form(x.detach(), z, gamma, R.ALPHA, pw)
    np.testing.assert_allclose(float(val.sum()), float(total.detach()), rtol=1e-13)
    np.testing.assert_allclose(grad.numpy(), x.grad.numpy(), rtol=1e-9, atol=1e-15)
    # the derivative of the modulating factor is a real part of it: without it the gradient is another one
    fl0 = R.FocalLoss(torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([pw], dtype=torch.float64), reduction="sum"), gamma, R.ALPHA, "const_mod")
    x0 = x.detach().clone().requires_grad_(True)
    fl0(x0, z).backward()
    assert float((x0.grad - x.grad).abs().max()) > 1e-2 * float(x.grad.abs().max())


def test_saturation_premise():
    """|x| <= XMAX keeps u = 1 - p_t away from 0 in float32 (the cases judged against float64 never take the u == 0 branch), while the
    separate saturated case of the GPU tests (x = +-40, +-120) does reach it in torch's float32"""
    x = torch.tensor([-R.XMAX, R.XMAX], dtype=torch.float32)
    s = torch.sigmoid(x)
    assert float((1 - s).min()) > 1e-5 and float(s.min()) > 1e-5
    assert float(1 - torch.sigmoid(torch.tensor(40.0))) == 0.0 and float(torch.sigmoid(torch.tensor(-120.0))) == 0.0
    for grids in R.GRIDS:
        for nc in (1, 3):
            for v in range(R.AUTO_CALLS):
                assert all(float(p.abs().max()) <= R.XMAX for p in R.inputs(grids, nc, v)[0])
    # and there torch's own gradient is not finite for gamma < 1, where the closed form takes the term as 0
    xs = torch.tensor([120.0], dtype=torch.float32, requires_grad=True)
    R.FocalLoss(torch.nn.BCEWithLogitsLoss(), 0.5, R.ALPHA)(xs, torch.ones(1)).backward()
    assert not bool(torch.isfinite(xs.grad).all())
    _, g = R.focal_closed_form(torch.tensor([120.0]), torch.ones(1), 0.5, R.ALPHA, 1.0)
    assert float(g) == 0.0


# ---- the premises of the GPU cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grids", list(R.GRIDS))
@pytest.mark.parametrize("nc", [1, 3])
def test_case_premises(grids, nc):
    """every level has matched rows, cells are contended (several candidates per cell, level 0's crowded cell most of all), exact ties
    exist, some iou are negative (the clamp matters) and padding rows are there; sorting then assigning is the per-cell maximum, and
    differs from the last writer's value"""
    from oracle import functional as OF
    preds, tg = R.inputs(grids, nc)
    anchors, strides, ssi = R.geometry(grids)
    assert strides[ssi] == 16.0 and int((tg[:, 0] == -1).sum()) == 3 and 38 <= tg.shape[0]
    real = tg[tg[:, 0] != -1]
    assert len(torch.unique(real, dim=0)) == real.shape[0] - 4                                # four exact duplicates
    _, tbox, indices, anch = OF.build_targets([tuple(p.shape) for p in preds], real, anchors)
    differs = 0
    for i, pi in enumerate(preds):
        b, a, gj, gi = indices[i]
        assert b.numel() > 0 and b.numel() < 3000
        ny, nx = pi.shape[2:4]
        cell = ((b * 3 + a) * ny + gj) * nx + gi
        counts = torch.unique(cell, return_counts=True)[1]
        if i == 0:
            assert int(counts.max()) >= 6
        sel = pi.double()[b, a, gj, gi]
        box = torch.cat((sel[:, 0:2].sigmoid() * 2 - 0.5, (sel[:, 2:4].sigmoid() * 2) ** 2 * anch[i].double()), 1)
        iou = OF.eiou(box, tbox[i].double()).squeeze(-1)
        assert float(iou.min()) < 0
        for gr in (1.0, 0.5):
            want = torch.zeros(pi.shape[:4], dtype=torch.float64).view(-1)
            v = iou.clamp(0)
            want.scatter_reduce_(0, cell, (1.0 - gr) + gr * v if gr < 1 else v, "amax", include_self=True)
            got = R.tobj_of(pi.shape[:4], indices[i], iou, gr, True)
            assert torch.equal(got.view(-1), want)
            differs += int((R.tobj_of(pi.shape[:4], indices[i], iou, gr, False).view(-1) != want).sum())
    assert differs > 0


# ---- planted defects ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect,grids,nc,gamma,opt", [
    ("const_mod", "pyr", 1, 1.5, "plain"), ("const_mod", "pyr", 3, 0.5, "all"), ("const_mod", "rect", 3, 2.0, "plain"),
    ("alpha_side", "pyr", 1, 1.5, "plain"), ("alpha_side", "rect", 3, 2.0, "all"),
    ("gr_before_clamp", "pyr", 1, 1.5, "gr.5"), ("gr_before_clamp", "rect", 3, 0.5, "all"),
    ("last_writer", "pyr", 1, 1.5, "sort"), ("last_writer", "pyr", 3, 2.0, "all"), ("last_writer", "rect", 1, 0.5, "sort"),
])
def test_planted_defects_are_caught(defect, grids, nc, gamma, opt):
    want, bound = R.reference(grids, nc, gamma, opt)
    assert R.judge(want, want, bound) == []
    bad, _ = R.reference(grids, nc, gamma, opt, defect=defect)
    caught = {k for k, _, _ in R.judge({k: v for k, v in bad.items() if k != "balance"}, want, bound)}
    assert "loss" in caught or "const_mod" == defect, caught                                  # (const_mod leaves the value alone)
    assert any(k.startswith("dpred") for k in caught), caught


@pytest.mark.parametrize("defect", ["balance_early", "norm_level0"])
@pytest.mark.parametrize("grids,nc", [("pyr", 1), ("pyr", 3)])
def test_planted_autobalance_defects_are_caught(defect, grids, nc):
    ref = R.reference_autobalance(grids, nc, 1.5, "all")
    bad = R.reference_autobalance(grids, nc, 1.5, "all", defect=defect)
    _, _, ssi = R.geometry(grids)
    moved = 0.0
    for c, ((want, bound), (got, _)) in enumerate(zip(ref, bad)):
        assert float(want["balance"][ssi]) == 1.0
        moved = max(moved, float((want["balance"] - torch.tensor(R.default_balance(3))).abs().max()))
        caught = {k for k, _, _ in R.judge(got, want, bound)}
        if defect == "balance_early":
            assert "lobj" in caught and any(k.startswith("dpred") for k in caught), (c, caught)   # from the very first call
        elif c == 0:
            assert "balance" in caught, caught                                                  # the vector after call 1, then lobj from call 2 on
        else:
            assert {"balance", "lobj"} <= caught, (c, caught)
    assert moved > 1e-5


# ---- construction ---------------------------------------------------------------------------------------------------------------------------
def test_construction_rules():
    from lead_yolo_amd.loss import ComputeLoss
    anchors, strides, ssi = R.geometry("pyr")
    with pytest.raises(NotImplementedError, match="allow_focal"):
        ComputeLoss(_Det(anchors), hyp=dict(fl_gamma=1.5))
    cl = ComputeLoss(_Det(anchors), hyp=dict(fl_gamma=1.5), allow_focal=True)
    assert cl.gamma == 1.5 and cl.gr == 1.0 and cl.sort_obj_iou is False and cl.balance == [4.0, 1.0, 0.4]
    assert ComputeLoss(_Det(anchors), allow_focal=True).gamma == 0.0
    with pytest.raises(ValueError, match="stride-16"):
        ComputeLoss(_Det(anchors), autobalance=True)
    with pytest.raises(ValueError, match="stride-16"):
        ComputeLoss(_Det(anchors, stride=[8.0, 32.0, 64.0]), autobalance=True)
    cl = ComputeLoss(_Det(anchors, stride=strides), autobalance=True)
    assert cl.autobalance and cl.ssi == ssi == 1 and cl.balance == [4.0, 1.0, 0.4]
    cl.gr = 1.5
    with pytest.raises(RuntimeError, match="no CPU fallback"):                                  # the device check comes first, as before
        cl([torch.zeros(1, 3, 2, 2, 6)] * 3, torch.zeros(0, 6))
