"""torch restatement of the reference's `ComputeLoss.__call__` (utils/loss.py:121-191) WITH its four options — focal loss (`FocalLoss`,
utils/loss.py:36-61, literally), `gr`, `sort_obj_iou` (argsort) and autobalance (Python-float balance, stride-16 normalisation) — in any
dtype, gradients from autograd; the seeded cases of tests/test_lossopts_host.py and tests/test_gpu_lossopts.py; the judges both use; and the
planted defects.  Independent of lead_yolo_amd.  Everything cached here is computed once and shared; callers must not modify it.

Target assignment is oracle.functional.build_targets in float32 (the decisions — anchor ratio, offsets, truncation — are float32 decisions,
bit-exact with the device's, tests/test_loss.py); its float32 results are then carried into the working dtype.

`defect=` plants one mistake: "const_mod" (the modulating factor treated as a constant in the gradient), "alpha_side" (alpha on the negative
side), "gr_before_clamp" ((1 - gr) + gr * iou clamped afterwards), "balance_early" (balance updated before lobj uses it), "norm_level0"
(normalised by level 0 instead of ssi), "last_writer" (sort_obj_iou ignored).

Bounds (`bounds_of`): for every compared quantity, MARGIN x the largest deviation of this restatement run in float32 from its float64 run
on the same case, with a floor of FLOOR_ULPS float32 ulps of the quantity's largest magnitude."""
import functools

import torch
import torch.nn as nn

from oracle import functional as OF

MARGIN, FLOOR_ULPS = 4.0, 4.0
EPS32 = 2.0 ** -23
ALPHA = 0.25
DEFECTS = ("const_mod", "alpha_side", "gr_before_clamp", "balance_early", "norm_level0", "last_writer")


class FocalLoss(nn.Module):
    """utils/loss.py:36-61"""

    def __init__(self, loss_fcn, gamma=1.5, alpha=0.25, defect=None):
        super().__init__()
        self.loss_fcn = loss_fcn
        self.gamma = gamma
        self.alpha = alpha
        self.reduction = loss_fcn.reduction
        self.loss_fcn.reduction = "none"
        self.defect = defect

    def forward(self, pred, true):
        loss = self.loss_fcn(pred, true)
        pred_prob = torch.sigmoid(pred)
        p_t = true * pred_prob + (1 - true) * (1 - pred_prob)
        alpha_factor = true * self.alpha + (1 - true) * (1 - self.alpha)
        if self.defect == "alpha_side":
            alpha_factor = true * (1 - self.alpha) + (1 - true) * self.alpha
        modulating_factor = (1.0 - p_t) ** self.gamma
        if self.defect == "const_mod":
            modulating_factor = modulating_factor.detach()
        loss *= alpha_factor * modulating_factor
        if self.reduction == "mean":
            return loss.mean()
        elif self.reduction == "sum":
            return loss.sum()
        return loss


def focal_closed_form(x, z, gamma, alpha, pw):
    """(loss, d loss / dx) per element, the formulas csrc/ly_loss.hip implements"""
    s = torch.sigmoid(x)
    sp = torch.nn.functional.softplus(-x)
    bce = (1 - z) * x + (1 + (pw - 1) * z) * sp
    dbce = (1 - z) * s - pw * z * (1 - s)
    u = z * (1 - s) + (1 - z) * s
    af = z * alpha + (1 - z) * (1 - alpha)
    m = u ** gamma
    second = torch.where(u > 0, bce * gamma * u ** (gamma - 1) * (2 * z - 1) * s * (1 - s), torch.zeros_like(u))
    return bce * af * m, af * (dbce * m - second)


def default_balance(nl):
    return {3: [4.0, 1.0, 0.4]}.get(nl, [4.0, 1.0, 0.25, 0.06, 0.02])[:nl]


def tobj_of(shape, idx, iou, gr=1.0, sort_obj_iou=False, defect=None):
    """utils/loss.py:158-165: the objectness target of one level from the matched rows' (detached) iou"""
    b, a, gj, gi = idx
    tobj = torch.zeros(shape, dtype=iou.dtype)
    if defect == "gr_before_clamp":
        iou = ((1.0 - gr) + gr * iou).clamp(0) if gr < 1 else iou.clamp(0)
    else:
        iou = iou.clamp(0)
    if sort_obj_iou and defect != "last_writer":
        j = iou.argsort()
        b, a, gj, gi, iou = b[j], a[j], gj[j], gi[j], iou[j]
    if gr < 1 and defect != "gr_before_clamp":
        iou = (1.0 - gr) + gr * iou
    tobj[b, a, gj, gi] = iou          # sequential on the CPU below 3000 rows: the last assignment to a cell stays
    return tobj


def compute_loss(preds, targets, anchors, nc, hyp=None, gr=1.0, sort_obj_iou=False, autobalance=False, balance=None, ssi=0, defect=None):
    """-> loss * bs [1], items [3] (lbox, lobj, lcls), the balance list after the call.  preds: leaves of the working dtype."""
    hyp = dict(OF.DEFAULT_HYP, **(hyp or {}))
    dt = preds[0].dtype
    nl = len(preds)
    balance = list(balance) if balance is not None else default_balance(nl)
    targets = targets[targets[:, 0] != -1].float()                         # padding rows
    tcls, tbox, indices, anch = OF.build_targets([tuple(p.shape) for p in preds], targets, anchors.float(), hyp["anchor_t"])
    BCEcls = nn.BCEWithLogitsLoss(pos_weight=torch.tensor([hyp["cls_pw"]], dtype=dt))
    BCEobj = nn.BCEWithLogitsLoss(pos_weight=torch.tensor([hyp["obj_pw"]], dtype=dt))
    g = hyp["fl_gamma"]
    if g > 0:
        BCEcls, BCEobj = FocalLoss(BCEcls, g, ALPHA, defect), FocalLoss(BCEobj, g, ALPHA, defect)
    cp, cn = 1.0 - 0.5 * hyp["label_smoothing"], 0.5 * hyp["label_smoothing"]
    lcls, lbox, lobj = torch.zeros(1, dtype=dt), torch.zeros(1, dtype=dt), torch.zeros(1, dtype=dt)
    for i, pi in enumerate(preds):
        b, a, gj, gi = indices[i]
        n = b.shape[0]
        tobj = torch.zeros(pi.shape[:4], dtype=dt)
        if n:
            sel = pi[b, a, gj, gi]
            pxy = sel[:, 0:2].sigmoid() * 2 - 0.5
            pwh = (sel[:, 2:4].sigmoid() * 2) ** 2 * anch[i].to(dt)
            iou = OF.eiou(torch.cat((pxy, pwh), 1), tbox[i].to(dt)).squeeze(-1)
            lbox = lbox + (1.0 - iou).mean()
            tobj = tobj_of(pi.shape[:4], indices[i], iou.detach(), gr, sort_obj_iou, defect)
            if nc > 1:
                pcls = sel[:, 5:]
                t = torch.full_like(pcls, cn)
                t[range(n), tcls[i]] = cp
                lcls = lcls + BCEcls(pcls, t)
        obji = BCEobj(pi[..., 4], tobj)
        if autobalance and defect == "balance_early":
            balance[i] = balance[i] * 0.9999 + 0.0001 / obji.detach().item()
        lobj = lobj + obji * balance[i]
        if autobalance and defect != "balance_early":
            balance[i] = balance[i] * 0.9999 + 0.0001 / obji.detach().item()
    if autobalance:
        d = balance[0 if defect == "norm_level0" else ssi]
        balance = [x / d for x in balance]
    lbox = lbox * hyp["box"]
    lobj = lobj * hyp["obj"]
    lcls = lcls * hyp["cls"]
    bs = preds[0].shape[0]
    return (lbox + lobj + lcls) * bs, torch.cat((lbox, lobj, lcls)).detach(), balance


# ---- the seeded cases ---------------------------------------------------------------------------------------------------------------------
_A = torch.tensor([[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]], dtype=torch.float32).view(3, 3, 2)
_STRIDES = (8.0, 16.0, 32.0)
# grids -> (levels' (ny, nx), which of the three anchor sets, batch, random target rows)
GRIDS = {"pyr": (((8, 8), (4, 4), (2, 2)), (0, 1, 2), 2, 28),          # a 64 x 64 image
         "rect": (((3, 5),), (1,), 2, 28),                              # one level at stride 16, ny != nx
         "big": (((40, 40), (20, 20), (10, 10)), (0, 1, 2), 4, 120)}    # more than one block per kernel
XMAX = 10.0                                                             # |logit| <= XMAX in everything judged against float64


def geometry(grids):
    """anchors [nl, 3, 2] in grid units, strides, ssi"""
    levels, sets, _, _ = GRIDS[grids]
    anchors = torch.stack([_A[s] / _STRIDES[s] for s in sets])
    strides = [_STRIDES[s] for s in sets]
    return anchors, strides, strides.index(16.0)


@functools.lru_cache(None)
def inputs(grids, nc, variant=0, empty=False):
    """preds (float32, |x| <= XMAX), targets [n, 6] with crowded cells, exact duplicates and padding rows; variant: another draw of the logits
    on the same targets (the autobalance sequence)"""
    levels, _, bs, nrand = GRIDS[grids]
    g = torch.Generator().manual_seed(1000 + 17 * len(grids) + nc)
    ny, nx = levels[0]
    tg = torch.cat((torch.randint(0, bs, (nrand, 1), generator=g).float(), torch.randint(0, nc, (nrand, 1), generator=g).float(),
                    torch.rand(nrand, 2, generator=g), torch.rand(nrand, 2, generator=g) * 0.92 + 0.03), 1)
    # six rows inside one cell of level 0 (image 0), sizes around that level's anchors; four of them once more: exact ties
    cx, cy = nx // 2, ny // 2
    crowd = torch.cat((torch.zeros(6, 1), torch.randint(0, nc, (6, 1), generator=g).float(),
                       (cx + 0.55 + 0.4 * torch.rand(6, 1, generator=g)) / nx, (cy + 0.55 + 0.4 * torch.rand(6, 1, generator=g)) / ny,
                       (1.0 + 2.0 * torch.rand(6, 1, generator=g)) / nx, (1.0 + 2.0 * torch.rand(6, 1, generator=g)) / ny), 1)
    pad = torch.tensor([[-1.0, 0.0, 0.5, 0.5, 0.2, 0.2], [-1.0, 99.0, 0.1, 0.9, 0.5, 0.5], [-1.0, -3.0, 0.0, 0.0, 0.0, 0.0]])
    tg = torch.cat((tg[:10], pad[:1], crowd, tg[10:20], crowd[1:5], pad[1:], tg[20:]))
    if empty:
        tg = pad.clone()
    gp = torch.Generator().manual_seed(2000 + 31 * variant + nc + len(grids))
    preds = tuple((torch.randn(bs, 3, y, x, 5 + nc, generator=gp) * 3).clamp(-XMAX, XMAX) for y, x in levels)
    return preds, tg


OPTION_SETS = {"plain": {}, "pw": dict(obj_pw=0.8, cls_pw=1.3), "smooth": dict(label_smoothing=0.1), "gr.5": dict(gr=0.5), "gr0": dict(gr=0.0),
               "sort": dict(sort=True), "all": dict(obj_pw=0.8, cls_pw=1.3, label_smoothing=0.1, gr=0.5, sort=True)}


def options(gamma, name):
    """-> hyp, gr, sort_obj_iou"""
    o = dict(OPTION_SETS[name])
    gr, sort = o.pop("gr", 1.0), o.pop("sort", False)
    return dict(o, fl_gamma=gamma), gr, sort


def _run(preds, tg, anchors, nc, dtype, **kw):
    ps = [p.to(dtype).clone().requires_grad_(True) for p in preds]
    loss, items, balance = compute_loss(ps, tg, anchors, nc, **kw)
    loss.backward()
    out = {"loss": loss.detach().double().reshape(1), "lbox": items[0:1].double(), "lobj": items[1:2].double(), "lcls": items[2:3].double(),
           "balance": torch.tensor(balance, dtype=torch.float64)}
    for i, p in enumerate(ps):
        out[f"dpred{i}"] = p.grad.double()
    return out


def bounds_of(want, f32):
    """quantity -> largest allowed |got - want|"""
    return {k: max(MARGIN * float((f32[k] - want[k]).abs().max()), FLOOR_ULPS * EPS32 * float(want[k].abs().max())) for k in want}


def judge(got, want, bound):
    """[(quantity, worst deviation, bound)] of the quantities that miss their bound (a NaN or an Inf in `got` misses); `got` may hold a subset"""
    bad = []
    for k, g in got.items():
        g = torch.as_tensor(g).double().cpu().reshape(want[k].shape)
        err = float((g - want[k]).abs().max()) if bool(torch.isfinite(g).all()) else float("inf")
        if not err <= bound[k]:
            bad.append((k, err, bound[k]))
    return bad


def ratios(got, want, bound):
    """quantity -> deviation / bound (what the GPU tests print)"""
    return {k: float((torch.as_tensor(g).double().cpu().reshape(want[k].shape) - want[k]).abs().max()) / bound[k] if bound[k] > 0 else 0.0
            for k, g in got.items()}


@functools.lru_cache(None)
def reference(grids, nc, gamma, optname, empty=False, defect=None):
    """-> want (float64 run), bound; with a defect: the defective float64 run instead of `want`, no bound"""
    preds, tg = inputs(grids, nc, 0, empty)
    anchors, _, _ = geometry(grids)
    hyp, gr, sort = options(gamma, optname)
    kw = dict(hyp=hyp, gr=gr, sort_obj_iou=sort)
    if defect is not None:
        return _run(preds, tg, anchors, nc, torch.float64, defect=defect, **kw), None
    want = _run(preds, tg, anchors, nc, torch.float64, **kw)
    return want, bounds_of(want, _run(preds, tg, anchors, nc, torch.float32, **kw))


AUTO_CALLS = 5


@functools.lru_cache(None)
def reference_autobalance(grids, nc, gamma, optname, defect=None):
    """AUTO_CALLS consecutive calls on changing predictions, the balance carried from call to call -> [(want, bound)] per call"""
    anchors, _, ssi = geometry(grids)
    hyp, gr, sort = options(gamma, optname)
    out = []
    bal = {torch.float64: None, torch.float32: None}
    for c in range(AUTO_CALLS):
        preds, tg = inputs(grids, nc, c)
        runs = {}
        for dt in ((torch.float64,) if defect is not None else (torch.float64, torch.float32)):
            runs[dt] = _run(preds, tg, anchors, nc, dt, hyp=hyp, gr=gr, sort_obj_iou=sort, autobalance=True, balance=bal[dt], ssi=ssi, defect=defect)
            bal[dt] = runs[dt]["balance"].tolist()
        out.append((runs[torch.float64], None if defect is not None else bounds_of(runs[torch.float64], runs[torch.float32])))
    return out
