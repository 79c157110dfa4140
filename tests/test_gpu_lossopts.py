"""The options of the device loss (csrc/ly_loss.hip: focal loss on both BCEs, gr, sort_obj_iou, autobalance) against the float64
restatement of the reference (tests/lossopts_ref.py): loss, the three items and d/dpred of every level, class logits included; the balance
vector over consecutive calls; the neutral options through the new entry points bit for bit; reproducibility; a captured training step.

Shapes: bs 2, na 3, levels 8x8 / 4x4 / 2x2 ("pyr"), one 3x5 level ("rect"), and 40 / 20 / 10 with bs 4 ("big": several blocks per kernel);
41 target rows with a crowded cell, exact duplicates and padding rows; |logit| <= 10.

Bounds: per quantity, 4 x the deviation of the float32 CPU run of the restatement from its float64 run on the same case, floor 4 float32 ulps
of the quantity's largest magnitude (lossopts_ref.bounds_of).  Every test prints deviation / bound per quantity.
Measured on an MI355X (largest deviation / bound over the family, and the quantity that had it):
  pyr, gamma 0.5: nc 1 0.48 (dpred1), nc 3 0.44 (dpred0)      pyr, gamma 1.5: nc 1 0.36 (dpred2), nc 3 0.26 (lcls)
  pyr, gamma 2.0: nc 1 0.43 (dpred2), nc 3 0.31 (dpred1)      pyr, gr / sort without focal loss: nc 1 0.25 (dpred2), nc 3 0.36 (dpred1)
  rect: gamma 0.5 0.23 (loss), 1.5 0.19 (loss), 2.0 0.30 (lcls) big: 0.36 (dpred2), 0.30 (lcls)      no targets: 0.21 (dpred0)
  autobalance, five calls: pyr nc 1 0.36, nc 3 0.35, rect 0.29 (a level's gradient each time); the balance vector itself < 0.001
i.e. the kernels deviate from float64 by at most about twice what torch's own float32 does; no case needed more than half the bound.
Plain ComputeLoss run twice on these inputs differs in the box / class gradient of cells with three or more candidates (float atomics; up
to 2e-8 of the level's largest gradient) and nowhere else: what test_neutral_options_keep_the_bits allows for.
"""
import pytest
import torch

from oracle import synth
from tests import lossopts_ref as R
from tests.test_gpu_modules import _dev

pytestmark = pytest.mark.gpu

GAMMAS = (0.5, 1.5, 2.0)
CASES = [("pyr", nc, g, o) for nc in (1, 3) for g in GAMMAS for o in R.OPTION_SETS] + \
        [("rect", nc, g, o) for nc in (1, 3) for g in GAMMAS for o in ("plain", "all")] + \
        [("pyr", nc, 0.0, o) for nc in (1, 3) for o in ("gr.5", "gr0", "sort", "all")] + \
        [("big", 3, 1.5, "all"), ("big", 1, 0.5, "plain")]


class _Det:
    def __init__(self, anchors, nc, stride):
        self.na, self.nc, self.nl, self.anchors, self.stride = anchors.shape[1], nc, anchors.shape[0], anchors, torch.tensor(stride)


def _loss_object(grids, nc, gamma, optname, autobalance=False):
    from lead_yolo_amd.loss import ComputeLoss
    anchors, strides, _ = R.geometry(grids)
    hyp, gr, sort = R.options(gamma, optname)
    cl = ComputeLoss(_Det(anchors.to(_dev()), nc, strides), autobalance=autobalance, hyp=hyp, allow_focal=True)
    cl.gr, cl.sort_obj_iou = gr, sort
    return cl


def _call(cl, preds, tg):
    pd = [p.to(_dev()).clone().requires_grad_(True) for p in preds]
    loss, items = cl(pd, tg.to(_dev()))
    loss.backward()
    got = {"loss": loss.detach(), "lbox": items[0:1], "lobj": items[1:2], "lcls": items[2:3]}
    got.update({f"dpred{i}": p.grad for i, p in enumerate(pd)})
    return got


def _held(got, want, bound, what):
    r = R.ratios(got, want, bound)
    worst = max(r, key=r.get)
    print(f"{what}: deviation / bound: worst {r[worst]:.3f} ({worst}); " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    bad = R.judge(got, want, bound)
    assert not bad, (what, bad)


@pytest.mark.parametrize("grids,nc,gamma,optname", CASES)
def test_options_vs_float64(grids, nc, gamma, optname):
    preds, tg = R.inputs(grids, nc)
    want, bound = R.reference(grids, nc, gamma, optname)
    if nc > 1:
        assert float(want["lcls"]) > 0
    _held(_call(_loss_object(grids, nc, gamma, optname), preds, tg), want, bound, (grids, nc, gamma, optname))


@pytest.mark.parametrize("nc", [1, 3])
def test_no_targets(nc):
    """only padding rows, and no rows at all: the objectness term alone, focal, every cell a negative"""
    preds, tg = R.inputs("pyr", nc, 0, True)
    want, bound = R.reference("pyr", nc, 1.5, "all", empty=True)
    assert float(want["lbox"]) == 0 and float(want["lobj"]) > 0
    cl = _loss_object("pyr", nc, 1.5, "all")
    _held(_call(cl, preds, tg), want, bound, ("padding only", nc))
    _held(_call(cl, preds, tg[:0]), want, bound, ("no rows", nc))


@pytest.mark.parametrize("gamma", [0.5, 1.5])
def test_saturated_logits_stay_finite(gamma):
    """objectness and class logits of +-40 and +-120 (float32: 1 - sigmoid(40) == 0, and exp(-120) == 0, so u == 0 is really reached):
    everything finite — torch's own gradient is NaN here for gamma < 1 (tests/test_lossopts_host.py) — and where u == 0 and the modulating
    factor is 0 the gradient is exactly 0: the term with u^(gamma - 1) is taken as 0 (csrc/ly_loss.hip, head of the file)"""
    from oracle import functional as OF
    nc = 3
    preds, tg = R.inputs("pyr", nc)
    g = torch.Generator().manual_seed(5)
    vals = torch.tensor([-120.0, -40.0, 40.0, 120.0])
    preds = [torch.cat((p[..., :4], vals[torch.randint(0, 4, p[..., 4:].shape, generator=g)]), -1) for p in preds]
    got = _call(_loss_object("pyr", nc, gamma, "all"), preds, tg)
    anchors, _, _ = R.geometry("pyr")
    _, _, indices, _ = OF.build_targets([tuple(p.shape) for p in preds], tg[tg[:, 0] != -1], anchors)
    zeros = 0
    for i, p in enumerate(preds):
        assert all(bool(torch.isfinite(v).all()) for v in got.values())
        unmatched = torch.ones(p.shape[:4], dtype=torch.bool)
        unmatched[indices[i][0], indices[i][1], indices[i][2], indices[i][3]] = False
        sel = unmatched & (p[..., 4] == -120.0)                                  # z = 0, s = 0: u = 0
        zeros += int(sel.sum())
        assert bool((got[f"dpred{i}"].cpu()[..., 4][sel] == 0).all())
        far = unmatched & (p[..., 4] == 120.0)                                   # z = 0, s = 1: the full negative gradient, (1 - alpha) / cells scale
        assert bool((got[f"dpred{i}"].cpu()[..., 4][far] > 0).all())
    assert zeros > 10 and float(got["loss"]) > 0


@pytest.mark.parametrize("grids,nc", [("pyr", 1), ("pyr", 3), ("rect", 1)])
def test_autobalance_sequence(grids, nc):
    """AUTO_CALLS consecutive calls on changing predictions with focal loss and all options: after each call the balance vector, the loss, lobj
    (formed with the balance BEFORE the call's update) and every gradient against the restatement; balance[ssi] == 1 after every call"""
    ref = R.reference_autobalance(grids, nc, 1.5, "all")
    _, _, ssi = R.geometry(grids)
    cl = _loss_object(grids, nc, 1.5, "all", autobalance=True)
    start = list(cl.balance)
    assert start == R.default_balance(len(start))
    for c, (want, bound) in enumerate(ref):
        preds, tg = R.inputs(grids, nc, c)
        got = _call(cl, preds, tg)
        got["balance"] = torch.tensor(cl.balance, dtype=torch.float64)
        assert float(got["balance"][ssi]) == 1.0
        _held(got, want, bound, ("autobalance", grids, nc, "call", c))
    assert cl.balance != start
    cl.balance = start                                                           # assignment writes the device vector in place
    assert cl.balance == start


@pytest.mark.parametrize("grids,nc", [("pyr", 3), ("big", 1)])
def test_neutral_options_keep_the_bits(grids, nc):
    """allow_focal=True with gamma 0, gr 1, no sort, no autobalance: the bits of plain ComputeLoss — in the loss, the items, the objectness
    gradient of every cell and the box / class gradient of every cell with at most two candidates.  A cell shared by three or more takes its
    box and class gradient from as many float atomics, whose order the scheduler picks: two runs of PLAIN ComputeLoss differ there in
    the last bits (the crowded cells of these inputs have up to ten candidates), so those entries are held to 32 ulps of the level's
    largest gradient instead."""
    from lead_yolo_amd.loss import ComputeLoss
    from oracle import functional as OF
    preds, tg = R.inputs(grids, nc)
    anchors, strides, _ = R.geometry(grids)
    hyp = dict(obj_pw=0.8, cls_pw=1.3, label_smoothing=0.1)
    a = _call(ComputeLoss(_Det(anchors.to(_dev()), nc, strides), hyp=hyp), preds, tg)
    b = _call(ComputeLoss(_Det(anchors.to(_dev()), nc, strides), hyp=dict(hyp, fl_gamma=0.0), allow_focal=True), preds, tg)
    _, _, indices, _ = OF.build_targets([tuple(p.shape) for p in preds], tg[tg[:, 0] != -1], anchors)
    for k in ("loss", "lbox", "lobj", "lcls"):
        assert torch.equal(a[k], b[k]), k
    for i, p in enumerate(preds):
        x, y = a[f"dpred{i}"].cpu(), b[f"dpred{i}"].cpu()
        assert torch.equal(x[..., 4], y[..., 4]), i
        count = torch.zeros(p.shape[:4])
        count.index_put_(indices[i], torch.ones(indices[i][0].numel()), accumulate=True)
        assert bool((count <= 2).any()) and torch.equal(x[count <= 2], y[count <= 2]), i
        assert float((x - y).abs().max()) <= 32 * R.EPS32 * float(x.abs().max()), i
    c = _call(_loss_object(grids, nc, 1.5, "plain"), preds, tg)                  # and focal loss is another loss
    assert not torch.equal(a["loss"], c["loss"])


def test_old_entry_points_forward_with_neutral_values():
    """ly_loss_level / ly_loss_finish (the entry points external binders use) called directly: the loss, the items and the
    objectness gradient ComputeLoss gives at default options, bit for bit"""
    from lead_yolo_amd import capi
    from lead_yolo_amd.loss import ACC, ComputeLoss
    nc = 3
    preds, tg = R.inputs("pyr", nc)
    anchors, strides, _ = R.geometry("pyr")
    hyp = dict(obj_pw=0.8, cls_pw=1.3, label_smoothing=0.1)
    want = _call(ComputeLoss(_Det(anchors.to(_dev()), nc, strides), hyp=hyp), preds, tg)
    dev, lib, st = _dev(), capi.lib(), capi.stream_ptr()
    pd, tgd, an = [p.to(dev).contiguous() for p in preds], tg.to(dev).contiguous(), [a.to(dev).contiguous() for a in anchors]
    nt, bs = tg.shape[0], pd[0].shape[0]
    cells = [p.numel() // p.shape[-1] for p in pd]
    acc = torch.zeros(3, ACC, device=dev)
    dps = []
    for i, p in enumerate(pd):
        dp, tobj, winner = torch.zeros_like(p), torch.zeros(cells[i], device=dev), torch.full((cells[i],), -1, dtype=torch.int32, device=dev)
        cand_cell, cand = torch.empty(15 * nt, dtype=torch.int64, device=dev), torch.empty(15 * nt, 5, device=dev)
        capi.check(lib.ly_loss_level(capi.ptr(p), capi.ptr(dp), capi.ptr(an[i]), capi.ptr(tgd), bs, 3, p.shape[2], p.shape[3], p.shape[4], nt, 4.0, 0.05,
                                     1.0, [4.0, 1.0, 0.4][i], capi.ptr(tobj), capi.ptr(winner), capi.ptr(cand_cell), capi.ptr(cand), capi.ptr(acc[i]),
                                     capi.ptr(None), 0, 0.5, 0.95, 0.05, 1.3, 0.8, st), "ly_loss_level")
        dps.append(dp)
    out = torch.empty(4, device=dev)
    cells_t, bal_t = torch.tensor([float(c) for c in cells], device=dev), torch.tensor([4.0, 1.0, 0.4], device=dev)
    capi.check(lib.ly_loss_finish(capi.ptr(acc), 3, capi.ptr(cells_t), capi.ptr(bal_t), 0.05, 1.0, 0.5, nc, bs, capi.ptr(out), st), "ly_loss_finish")
    torch.cuda.synchronize()
    assert torch.equal(out[:1], want["loss"]) and torch.equal(out[1:2], want["lbox"]) and torch.equal(out[2:3], want["lobj"]) and \
        torch.equal(out[3:4], want["lcls"])
    for i, dp in enumerate(dps):
        assert torch.equal(dp[..., 4], want[f"dpred{i}"][..., 4]), i


def test_all_options_reproduce_their_bits():
    """two runs of three autobalanced calls with every option on: the same bits in the loss, the items, the balance vector and the
    objectness gradient — what the fixed-point sums promise (box and class gradients of a shared cell are float atomics, as before)"""
    runs = []
    for _ in range(2):
        cl = _loss_object("big", 3, 1.5, "all", autobalance=True)
        out = []
        for c in range(3):
            got = _call(cl, *R.inputs("big", 3, c))
            out.append([got["loss"], got["lbox"], got["lobj"], got["lcls"], torch.tensor(cl.balance, dtype=torch.float64)] +
                       [got[f"dpred{i}"][..., 4] for i in range(3)])
        runs.append(out)
    for x, y in zip(*runs):
        assert all(torch.equal(u, v) for u, v in zip(x, y))


def test_captured_step_with_options():
    """lead-yolo-n, 2 x 3 x 64 x 64: focal loss + autobalance + sort_obj_iou inside a GraphedTrainStep.  From one state (weights, BatchNorm
    statistics, optimiser state, balance vector), two eager steps and two replays leave the same bits in all of it; the balance vector is
    device state that every replay moves"""
    import lead_yolo_amd as L
    from lead_yolo_amd import pack
    from tests.test_gpu_adam import _model
    m = _model()
    opt = L.smart_optimizer(m, "SGD", 0.01, 0.937, 5e-4)
    cl = L.ComputeLoss(m, autobalance=True, hyp=dict(fl_gamma=1.5), allow_focal=True)
    cl.sort_obj_iou = True
    first = list(cl.balance)
    imgs, tg = synth.synth_images(2, 64, 3).to(_dev()), synth.synth_targets(2, 4, per_image=3).to(_dev())
    step = L.GraphedTrainStep(m, cl, opt, imgs, tg, warmup=2)

    def state():
        return [v for v in m.state_dict().values() if v.is_floating_point()] + opt.device_state()

    torch.cuda.synchronize()
    saved, bal0 = [t.clone() for t in state()], list(cl.balance)
    assert bal0 != first and bal0[cl.ssi] == 1.0                               # the warm-up steps moved it

    def run(how):
        with torch.no_grad():
            for dst, src in zip(state(), saved):
                dst.copy_(src)
        cl.balance = bal0
        pack.touch_weights()
        for _ in range(2):
            loss, _ = step() if how == "graph" else L.train_step(m, cl, opt, imgs, tg)
        torch.cuda.synchronize()
        return [t.clone() for t in state()], list(cl.balance), float(loss)

    we, be, le = run("eager")
    wg, bg, lg = run("graph")
    assert be == bg and be != bal0 and be[cl.ssi] == 1.0, (bal0, be, bg)
    assert le == lg, (le, lg)
    bad = [i for i, (x, y) in enumerate(zip(we, wg)) if not torch.equal(x, y)]
    assert not bad, (len(bad), len(we))
    assert sum(not torch.equal(x, y) for x, y in zip(we, saved)) > 0.5 * len(saved)
