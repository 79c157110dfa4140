"""Device loss / target assignment (lead_yolo_amd.loss -> csrc/ly_loss.hip) vs the vectors the reference produced:
int64 indices bit-exact, loss and input gradients to fp32 rounding; and vs the oracle (oracle/functional.py, CPU) on random
many-targets-per-cell cases.  The product has no CPU loss: the CPU side of these tests is the oracle."""
import numpy as np
import pytest
import torch

from tests import golden_util as G


class _Det:
    def __init__(self, anchors):
        self.na, self.nc, self.nl, self.anchors = anchors.shape[1], 1, anchors.shape[0], anchors


def test_loss_refuses_cpu():
    from lead_yolo_amd.loss import ComputeLoss
    _, arr = G.load("loss_n")
    cl = ComputeLoss(_Det(G.t(arr["anchors"])))
    preds = [G.t(arr[f"pred{i}"]) for i in range(3)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cl(preds, G.t(arr["rand_targets"]))
    with pytest.raises(NotImplementedError):
        ComputeLoss(_Det(G.t(arr["anchors"])), hyp=dict(fl_gamma=1.5))


_HYP_KEYS = ("box", "cls", "cls_pw", "obj", "obj_pw", "anchor_t", "fl_gamma", "label_smoothing")


def test_oracle_multiclass_loss_matches_reference():
    """oracle/functional.compute_loss with nc = 3, label smoothing 0.1, cls_pw 1.3, obj_pw 0.8 vs the reference's own vectors
    (tests/golden/loss_nc3.npz, oracle/gen_golden.py gen_loss_multiclass; utils/loss.py:168-173)"""
    from oracle import functional as OF
    meta, arr = G.load("loss_nc3")
    preds = [G.t(arr[f"pred{i}"]).requires_grad_(True) for i in range(3)]
    loss, items = OF.compute_loss(preds, G.t(arr["targets"]), G.t(arr["anchors"]), nc=3, hyp={k: meta["hyp"][k] for k in _HYP_KEYS})
    loss.backward()
    np.testing.assert_allclose(loss.detach().numpy(), arr["loss"], rtol=1e-5)
    np.testing.assert_allclose(items.numpy(), arr["items"], rtol=1e-5, atol=1e-7)
    assert arr["items"][2] > 0                       # the class term is really there
    for i in range(3):
        np.testing.assert_allclose(preds[i].grad.numpy(), arr[f"dpred{i}"], rtol=1e-4, atol=1e-7)


@pytest.mark.gpu
def test_multiclass_loss_gpu():
    """the device loss with nc = 3 (class BCE, label smoothing, cls_pw, obj_pw — utils/loss.py:137-141, 168-173) vs the reference's
    vectors: loss, items, d/dpred of every level incl. the class logits, and build_targets' tcls bit-exact"""
    from lead_yolo_amd.loss import ComputeLoss
    device = torch.device("cuda:0")
    meta, arr = G.load("loss_nc3")
    det = _Det(G.t(arr["anchors"]).to(device))
    det.nc = 3
    cl = ComputeLoss(det, hyp={k: meta["hyp"][k] for k in _HYP_KEYS})
    preds = [G.t(arr[f"pred{i}"]).to(device).requires_grad_(True) for i in range(3)]
    tg = G.t(arr["targets"]).to(device)
    tcls, _, _, _ = cl.build_targets(preds, tg)
    for i in range(3):
        got = tcls[i].cpu().numpy()
        assert got.dtype == np.int64 and np.array_equal(got, arr[f"tcls{i}"])
    loss, items = cl(preds, tg)
    np.testing.assert_allclose(loss.detach().cpu().numpy(), arr["loss"], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(items.cpu().numpy(), arr["items"], rtol=2e-5, atol=1e-6)
    loss.backward()
    for i in range(3):
        np.testing.assert_allclose(preds[i].grad.cpu().numpy(), arr[f"dpred{i}"], rtol=2e-4, atol=2e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rand", "edge", "empty"])
def test_loss_gpu(case):
    from lead_yolo_amd.loss import ComputeLoss
    device = torch.device("cuda:0")
    meta, arr = G.load("loss_n")
    anchors = G.t(arr["anchors"]).to(device)
    cl = ComputeLoss(_Det(anchors), hyp={k: v for k, v in meta["hyp"].items() if k in _HYP_KEYS})
    preds = [G.t(arr[f"pred{i}"]).to(device).requires_grad_(True) for i in range(3)]
    tg = G.t(arr[f"{case}_targets"]).to(device)
    tcls, tbox, indices, anch = cl.build_targets(preds, tg)          # the matching kernel's own buffers, read back
    for i in range(3):
        got = np.stack([v.cpu().numpy() for v in indices[i]])
        assert got.dtype == np.int64 and np.array_equal(got, arr[f"{case}_idx{i}"])
        np.testing.assert_array_equal(tbox[i].detach().cpu().numpy(), arr[f"{case}_tbox{i}"])
        np.testing.assert_array_equal(anch[i].cpu().numpy(), arr[f"{case}_anch{i}"])
    loss, items = cl(preds, tg)
    np.testing.assert_allclose(loss.detach().cpu().numpy(), arr[f"{case}_loss"], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(items.cpu().numpy(), arr[f"{case}_items"], rtol=2e-5, atol=1e-6)
    loss.backward()
    for i in range(3):
        got, want = preds[i].grad.cpu().numpy(), arr[f"{case}_dpred{i}"]
        # `tobj[b, a, gj, gi] = iou` has duplicate cells (several targets per cell).  The reference's vectors come from the CPU,
        # where the last assignment wins; the device loss elects the same winner (highest candidate index), so the GPU result
        # matches cell for cell — unlike torch's unordered scatter on a GPU.
        np.testing.assert_allclose(got, want, rtol=2e-4, atol=2e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("bs,nt,seed", [(8, 200, 0), (4, 1, 1), (16, 900, 2)])
def test_device_loss_vs_oracle(bs, nt, seed):
    """the device loss against the oracle on the CPU (sequential scatter = the reference's semantics) on random predictions
    with many targets per cell: total, items, the gradient of every prediction, and build_targets' indices bit-exact"""
    from lead_yolo_amd.loss import ComputeLoss
    from oracle import functional as OF
    _, arr = G.load("loss_n")
    anchors = G.t(arr["anchors"])
    g = torch.Generator().manual_seed(seed)
    preds = [torch.randn(bs, 3, s, s, 6, generator=g) for s in (40, 20, 10)]
    tg = torch.cat((torch.randint(0, bs, (nt, 1), generator=g).float(), torch.zeros(nt, 1), torch.rand(nt, 2, generator=g),
                    torch.rand(nt, 2, generator=g) * 0.4 + 0.01), 1)
    nthreads = torch.get_num_threads()
    ps = [p.clone().requires_grad_(True) for p in preds]
    torch.set_num_threads(1)          # torch's CPU index_put splits > 3000 indices over threads; one thread keeps `tobj[...] = iou` sequential
    try:
        l0, i0 = OF.compute_loss(ps, tg, anchors, nc=1)
        l0.backward()
    finally:
        torch.set_num_threads(nthreads)
    g0 = [p.grad for p in ps]
    dev = torch.device("cuda:0")
    cl = ComputeLoss(_Det(anchors.to(dev)))
    pd = [p.clone().to(dev).requires_grad_(True) for p in preds]
    l1, i1 = cl(pd, tg.to(dev))
    l1.backward()
    np.testing.assert_allclose(l1.detach().cpu().numpy(), l0.detach().numpy(), rtol=1e-4)
    np.testing.assert_allclose(i1.cpu().numpy(), i0.detach().numpy(), rtol=1e-4, atol=1e-6)
    for a, b in zip(pd, g0):
        np.testing.assert_allclose(a.grad.cpu().numpy(), b.numpy(), rtol=5e-4, atol=2e-6)
    _, tb1, idx1, an1 = cl.build_targets(pd, tg.to(dev))
    _, tb0, idx0, an0 = OF.build_targets([tuple(p.shape) for p in preds], tg, anchors)
    for i in range(3):
        for u, v in zip(idx1[i], idx0[i]):
            assert torch.equal(u.cpu(), v)
        assert torch.equal(tb1[i].cpu(), tb0[i]) and torch.equal(an1[i].cpu(), an0[i])


@pytest.mark.gpu
def test_out_of_range_image_index_is_loud_and_safe():
    """a target row whose image index is outside the batch (last partial batch, per-rank slices with global indices) must not
    index out of bounds: the row is rejected, the loss comes back NaN, build_targets raises IndexError (as torch indexing would)"""
    from lead_yolo_amd.loss import ComputeLoss
    _, arr = G.load("loss_n")
    dev = torch.device("cuda:0")
    cl = ComputeLoss(_Det(G.t(arr["anchors"]).to(dev)))
    preds = [G.t(arr[f"pred{i}"]).to(dev).requires_grad_(True) for i in range(3)]
    bs = preds[0].shape[0]
    tg = G.t(arr["rand_targets"]).to(dev).clone()
    guard = torch.full((1 << 20,), 7.0, device=dev)              # memory right after the allocations above keeps its contents
    for bad in (float(bs), float(bs + 1000), -2.0, float("nan")):
        t2 = tg.clone()
        t2[0, 0] = bad
        loss, _ = cl(preds, t2)
        assert torch.isnan(loss).all()
        with pytest.raises(IndexError):
            cl.build_targets(preds, t2)
    assert bool((guard == 7.0).all())
    loss, _ = cl(preds, tg)
    assert torch.isfinite(loss).all()
    # rows with image index exactly -1 are padding (fixed-shape target buffers of a captured training step): ignored
    pad = torch.cat((tg, torch.full((5, 6), -1.0, device=dev)))
    loss_p, items_p = cl(preds, pad)
    assert torch.equal(loss_p, loss)


# ---- nc > 1, ny != nx, crowded cells, targets on the matching rule's edges -------------------------------------------------------------
_HYP_SETS = {"default": None, "smooth": dict(label_smoothing=0.1, cls_pw=1.3, obj_pw=0.8)}
_GRIDS = {(40, 40): ((40, 40), (20, 20), (10, 10)), (24, 40): ((24, 40), (12, 20), (6, 10)), (40, 24): ((40, 24), (20, 12), (10, 6)),
          (5, 7): ((5, 7), (3, 4), (2, 2))}


def _edge_targets(bs, nc, grids, g):
    """rows that sit on the decisions of build_targets (utils/loss.py:222-250) at level 0's grid: exactly on cell boundaries (x * nx = k), within
    one ulp of the half-cell rule (x * nx = k + 0.5), below / at / above one cell from either border (the `> 1` rule), and at 0 and 1
    (the gi / gj clamp)"""
    ny, nx = grids[0]
    vals = []
    for n_, k in ((nx, 1), (nx, nx // 2), (nx, nx - 1), (ny, 1), (ny, ny // 2), (ny, ny - 1)):
        for v in (k / n_, (k + 0.5) / n_):
            f = np.float32(v)
            vals += [float(np.nextafter(f, np.float32(0))), float(f), float(np.nextafter(f, np.float32(2)))]
    vals += [0.0, 1e-4, 1.0 - 1e-4, float(np.nextafter(np.float32(1), np.float32(0))), 1.0]
    v = torch.tensor(vals, dtype=torch.float32)
    n = v.numel()
    other = torch.rand(n, generator=g)
    xy = torch.cat((torch.stack((v, other), 1), torch.stack((other, v), 1), torch.stack((v, v.flip(0)), 1)))
    m = xy.shape[0]
    # box sizes inside every level's anchor band at these grids would depend on the grid: draw them as the random rows do
    return torch.cat((torch.randint(0, bs, (m, 1), generator=g).float(), torch.randint(0, nc, (m, 1), generator=g).float(), xy,
                      torch.rand(m, 2, generator=g) * 0.4 + 0.01), 1)


def _loss_case(nc, grid, layout, seed, bs=16, nt=900):
    g = torch.Generator().manual_seed(seed)
    grids = _GRIDS[grid]
    preds = [torch.randn(bs, 3, ny, nx, 5 + nc, generator=g) for ny, nx in grids]
    img = torch.randint(0, bs, (nt, 1), generator=g).float()
    cls = torch.randint(0, nc, (nt, 1), generator=g).float()
    if layout == "crowded":
        # all targets of an image inside one 3 x 3 cell neighbourhood of level 0 (its own per image), sizes that match the anchors of every level
        ny, nx = grids[0]
        cx = torch.randint(1, nx - 1, (bs,), generator=g).float()
        cy = torch.randint(1, ny - 1, (bs,), generator=g).float()
        b = img[:, 0].long()
        xy = torch.stack(((cx[b] - 1 + 3 * torch.rand(nt, generator=g)) / nx, (cy[b] - 1 + 3 * torch.rand(nt, generator=g)) / ny), 1)
    else:
        xy = torch.rand(nt, 2, generator=g)
    # (5, 7) is a 40 x 56 pixel image: boxes up to the whole image, or nothing would reach the anchors of the coarser levels
    wh = torch.rand(nt, 2, generator=g) * 0.95 + 0.04 if grid == (5, 7) else torch.rand(nt, 2, generator=g) * 0.4 + 0.01
    tg = torch.cat((img, cls, xy, wh), 1)
    if layout == "spread":
        tg = torch.cat((tg, _edge_targets(bs, nc, grids, g)))
    return preds, tg


_MC_CASES = [(nc, grid, hyp, "spread") for nc in (1, 3, 80) for grid in _GRIDS for hyp in _HYP_SETS] + \
            [(3, (40, 40), "smooth", "crowded"), (80, (24, 40), "smooth", "crowded"), (1, (40, 24), "default", "crowded")]


@pytest.mark.gpu
@pytest.mark.parametrize("nc,grid,hyp,layout", _MC_CASES)
def test_device_loss_multiclass_rect_vs_oracle(nc, grid, hyp, layout):
    """test_device_loss_vs_oracle for nc in {1, 3, 80}, rectangular grids (ny != nx: the nx - gx / ny - gy offsets, the clamps, the cell
    unravelling), both hyp sets, 900 random targets over 16 images plus rows on the edges of the matching rule, and a layout where all
    targets of an image share a 3 x 3 neighbourhood (the election and the class-gradient atomics of ly_loss_apply are both contended).
    Total, items, every gradient; build_targets bit-exact: indices, tbox, anch, tcls."""
    from lead_yolo_amd.loss import ComputeLoss
    from oracle import functional as OF
    _, arr = G.load("loss_n")
    anchors = G.t(arr["anchors"])
    preds, tg = _loss_case(nc, grid, layout, 100 + nc + grid[0] + 7 * grid[1])
    hp = _HYP_SETS[hyp]
    nthreads = torch.get_num_threads()
    ps = [p.clone().requires_grad_(True) for p in preds]
    torch.set_num_threads(1)          # keeps `tobj[...] = iou` sequential (see test_device_loss_vs_oracle)
    try:
        l0, i0 = OF.compute_loss(ps, tg, anchors, nc=nc, hyp=hp)
        l0.backward()
    finally:
        torch.set_num_threads(nthreads)
    tc0, tb0, idx0, an0 = OF.build_targets([tuple(p.shape) for p in preds], tg, anchors)
    # the premises: matched rows at every level, a class term when there are classes, shared cells — many of them in the crowded layout
    mult = []
    for i, (b, a, gj, gi) in enumerate(idx0):
        assert b.numel() > 0
        ny, nx = _GRIDS[grid][i]
        assert int(gj.max()) < ny and int(gi.max()) < nx
        cell = ((b * 3 + a) * ny + gj) * nx + gi
        mult.append(torch.unique(cell, return_counts=True)[1])
    assert int(mult[0].max()) > 1
    if layout == "crowded":
        assert float(mult[0].float().mean()) > 3.0 and int(mult[0].max()) >= 8
    if layout == "spread" and grid != (5, 7):
        assert int(idx0[0][3].max()) == _GRIDS[grid][0][1] - 1 and int(idx0[0][3].min()) == 0     # both borders reached
    assert (float(i0[2]) > 0) == (nc > 1)
    dev = torch.device("cuda:0")
    det = _Det(anchors.to(dev))
    det.nc = nc
    cl = ComputeLoss(det, hyp=hp)
    pd = [p.clone().to(dev).requires_grad_(True) for p in preds]
    l1, i1 = cl(pd, tg.to(dev))
    l1.backward()
    tc1, tb1, idx1, an1 = cl.build_targets(pd, tg.to(dev))
    for i in range(3):
        for u, v in zip(idx1[i], idx0[i]):
            assert u.dtype == torch.int64 and torch.equal(u.cpu(), v)
        assert torch.equal(tb1[i].cpu(), tb0[i]) and torch.equal(an1[i].cpu(), an0[i]) and torch.equal(tc1[i].cpu(), tc0[i])
    print(f"loss {float(l1):.7g} vs {float(l0):.7g}; items {i1.cpu().tolist()} vs {i0.tolist()}")
    np.testing.assert_allclose(l1.detach().cpu().numpy(), l0.detach().numpy(), rtol=1e-4)
    np.testing.assert_allclose(i1.cpu().numpy(), i0.detach().numpy(), rtol=1e-4, atol=1e-6)
    for a, b in zip(pd, ps):
        got, want = a.grad.cpu().numpy(), b.grad.numpy()
        print("max gradient error over (5e-4 |want| + 2e-6):", float((np.abs(got - want) - 5e-4 * np.abs(want)).max()) - 2e-6)
        np.testing.assert_allclose(got, want, rtol=5e-4, atol=2e-6)


@pytest.mark.gpu
def test_out_of_range_class_is_loud_and_safe():
    """nc > 1: a target row whose class is >= nc, negative or NaN is rejected like a row with a bad image index (the reference's
    `t[range(n), tcls[i]] = cp` raises for a class >= nc and wraps a negative one, which is refused here on purpose; the kernel used to train all
    classes of the row as negatives, silently): NaN loss,
    IndexError from build_targets, nothing written out of bounds.  Padding rows stay silent whatever their class column holds, and nc = 1
    never reads the column."""
    from lead_yolo_amd.loss import ComputeLoss
    meta, arr = G.load("loss_nc3")
    dev = torch.device("cuda:0")
    det = _Det(G.t(arr["anchors"]).to(dev))
    det.nc = 3
    cl = ComputeLoss(det, hyp={k: meta["hyp"][k] for k in _HYP_KEYS})
    preds = [G.t(arr[f"pred{i}"]).to(dev).requires_grad_(True) for i in range(3)]
    tg = G.t(arr["targets"]).to(dev).clone()
    guard = torch.full((1 << 20,), 7.0, device=dev)
    loss, items = cl(preds, tg)
    assert torch.isfinite(loss).all() and float(items[2]) > 0
    for bad in (3.0, 1000.0, -1.0, -7.5, float("nan"), float("inf")):
        t2 = tg.clone()
        t2[1, 1] = bad
        l2, _ = cl(preds, t2)
        assert torch.isnan(l2).all(), bad
        with pytest.raises(IndexError):
            cl.build_targets(preds, t2)
    assert bool((guard == 7.0).all())
    # .long() truncates: 2.9 is class 2, -0.5 is class 0 — the reference's own reading of the column, still accepted
    t2 = tg.clone()
    t2[1, 1] = 2.9
    t3 = tg.clone()
    t3[1, 1] = 2.0
    assert torch.equal(cl(preds, t2)[0], cl(preds, t3)[0])
    for junk in (99.0, -3.0, float("nan")):
        pad = torch.cat((tg, torch.tensor([[-1.0, junk, 0.5, 0.5, 0.1, 0.1]] * 5, device=dev)))
        loss_p, _ = cl(preds, pad)
        assert torch.equal(loss_p, loss), junk
        cl.build_targets(preds, pad)
    # nc = 1: the class column is never read (utils/loss.py:168 `if self.nc > 1`)
    _, arr1 = G.load("loss_n")
    cl1 = ComputeLoss(_Det(G.t(arr1["anchors"]).to(dev)))
    p1 = [G.t(arr1[f"pred{i}"]).to(dev) for i in range(3)]
    t1 = G.t(arr1["rand_targets"]).to(dev).clone()
    want = cl1(p1, t1)[0]
    t1[:, 1] = 5.0
    assert torch.equal(cl1(p1, t1)[0], want)
