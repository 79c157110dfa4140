"""csrc/ly_anchors.hip and lead-yolo_amd/anchors.py on the device against the float64 / numpy restatements of tests/anchors_ref.py: bit-equal
label sizes, counts, exact fitness sums, the evolution chain for every batch size, one k-means iteration and the whole loop, check_anchors
on a model and what reads the anchors afterwards.  tests/test_anchors_host.py asserts the premises these comparisons rest on."""
import functools

import numpy as np
import pytest
import torch

import lead_yolo_amd as L
from lead_yolo_amd import anchors as A
from tests import anchors_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.array(a)).to(_dev())                                 # a copy: the shared reference data is read-only


# ---- label_wh ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True])
def test_label_wh_bit_equal(scaled):
    labels, shapes = R.dataset(2)                                                   # 815 labels (not a multiple of 256), images without labels
    assert sum(len(lb) for lb in labels) % 256 != 0 and any(len(lb) == 0 for lb in labels)
    sc = np.random.RandomState(3).uniform(0.9, 1.1, size=(len(shapes), 1)) if scaled else None
    got = A.label_wh(labels, shapes, 640, scale=sc, device=_dev()).cpu().numpy()
    want = R.label_wh(labels, shapes, 640, sc)
    assert got.dtype == F32 and got.shape == want.shape and np.array_equal(got, want)
    flat = _t(np.concatenate(labels))                                               # the ImageBank form: flat device array + counts
    got2 = A.label_wh((flat, np.array([len(lb) for lb in labels])), shapes, 640, scale=sc).cpu().numpy()
    assert np.array_equal(got2, want)


# ---- anchor_metric -------------------------------------------------------------------------------------------------------------------
def _candidates(G, na, seed):
    base = np.concatenate([R.COCO_ANCHORS, [[5, 2], [9, 3], [20, 6]]]).astype(F32)[np.linspace(0, 11, na).astype(int)]
    v = A.mutation_table(G, (na, 2), seed)
    v[0] = 1.0                                                                      # set 0: the base anchors themselves
    return (base[None].astype(np.float64) * v).clip(min=2.0).astype(F32), base


def _at_threshold(k, ithr):
    """a width w with float32(w / k) == ithr exactly (searched among the neighbours of k * ithr)"""
    w = F32(k * ithr)
    for _ in range(8):
        r = F32(w / k)
        if r == ithr:
            return w
        w = np.nextafter(w, F32(np.inf) if r < ithr else F32(0), dtype=F32)
    return None


def _metric_wh(n, thr, base):
    wh = R.wh_set(7, 4099).copy()[:n]
    ithr = F32(1.0 / thr)
    planted = 0
    for j, kk in enumerate(base[:min(n, 3)]):                                       # labels exactly at the threshold of an anchor
        w = _at_threshold(kk[0], ithr)
        if w is not None:
            wh[j] = (w, kk[1])
            planted += 1
    if n > 3:
        wh[3] = (1.5, 30.0)                                                         # a width below 2 px
    return wh, planted


@pytest.mark.parametrize("thr", [4.0, 2.9])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096, 4099])
def test_anchor_metric_bit_equal(n, thr):
    for G in (1, 3, 64):
        for na in (3, 9, 12):
            k, base = _candidates(G, na, 100 + na)
            wh, planted = _metric_wh(n, thr, base)
            assert planted >= 1
            x, _ = R.metric_x(wh, base)
            assert (x == F32(1.0 / thr)).any()                                      # the threshold case is really in the data
            want = np.array([R.metric_sums(wh, k[g], thr) for g in range(G)], dtype=np.float64)
            whd = _t(wh)
            for slices in (None, 1, 3):                                             # the result does not depend on the slice count
                got = A.metric_sums(whd, k, thr, slices=slices)
                assert got.shape == (G, 3) and np.array_equal(got, want), (G, na, slices)
    bpr, aat, fit = A.anchor_metric(whd, k[0], thr)
    assert (bpr, aat, fit) == (want[0, 1] / n, want[0, 2] / n, want[0, 0] / n)


# ---- evolve --------------------------------------------------------------------------------------------------------------------------
GEN = 1000


@functools.lru_cache(None)
def _chain():
    wh, k0 = R.wh_set(1), R.COCO_ANCHORS.astype(np.float64)
    v = A.mutation_table(GEN, (9, 2), 1)
    k, f, acc = R.evolve(wh, k0, v, 4.0)
    return wh, k0, v, k, f, acc


@pytest.mark.parametrize("batch", [1, 7, 32, 64])
def test_evolve_is_the_serial_chain(batch):
    wh, k0, v, k, f, acc = _chain()
    assert len(wh) == 4096 and len(acc) >= 20 and GEN % 7 != 0 and GEN % 32 != 0
    ev = A.evolve(_t(wh), k0, thr=4.0, gen=GEN, seed=1, batch=batch)
    assert ev.accepted == len(acc)
    assert ev.k.dtype == np.float64 and np.array_equal(ev.k.view(np.int64), k.view(np.int64))
    assert ev.fsum == f and ev.f == f / 4096
    assert ev.rounds >= max(len(acc), -(-GEN // batch)) and ev.rounds <= len(acc) + -(-GEN // batch)
    if batch == 1:
        assert ev.rounds == GEN


def test_evolve_gen_zero_and_table():
    wh, k0, v, k, f, acc = _chain()
    whd = _t(wh)
    ev = A.evolve(whd, k0, gen=0)
    assert np.array_equal(ev.k, k0) and ev.accepted == 0 and ev.rounds == 0 and ev.fsum == R.fitness_sum(wh, k0, 4.0)
    short = A.evolve(whd, k0, gen=37, table=v[:37], batch=32)                       # a given table, gen not a multiple of batch
    ks, fs, accs = R.evolve(wh, k0, v[:37], 4.0)
    assert np.array_equal(short.k, ks) and short.fsum == fs and short.accepted == len(accs)


# ---- k-means -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,runs", [(64, 1), (64, 30), (4099, 1), (4099, 30)])
def test_kmeans_one_iteration(n, runs):
    pts, cent = R.step_points(10 + runs, n, runs)                                   # the sets whose premises the host test asserts
    assign, count, new, dist, empty, _ = R.lloyd_step(pts, cent)
    for slices in (None, 2):
        got = A.kmeans_step(_t(pts), _t(cent), slices=slices)
        torch.cuda.synchronize()
        assert np.array_equal(got["assign"].cpu().numpy(), assign)
        assert np.array_equal(got["count"].cpu().numpy(), count)
        assert np.array_equal(got["cent"].cpu().numpy(), new)                       # float32(float64 sum / count); an emptied run keeps its centroids
        fl = got["flags"].cpu().numpy()
        assert np.array_equal((fl & 2) != 0, empty) and np.array_equal(fl[empty], np.full(empty.sum(), 3))
        d = got["dist"].cpu().numpy()
        assert (np.abs(d - dist) <= n * 2.0 ** -52 * dist).all()
    if (n, runs) == (64, 30):
        assert empty.any()


def test_kmeans_whole_loop():
    wh = R.loop_wh(3)
    want, bad, near, gap = R.loop_premises(wh, 9, 30, 3)
    pts, s = R.whiten(wh)
    got = A.kmeans(_t(wh), 9, runs=30, seed=3)
    assert np.array_equal(got.s, s)
    assert got.run == want["run"] and got.iters == want["iters"] and np.array_equal(got.run_iters, want["run_iters"])
    assert np.array_equal((got.flags & 2) != 0, want["discarded"])
    assert np.array_equal(got.cent[got.run], want["cent"][want["run"]])
    assert np.array_equal(got.cent, want["cent"])
    assert np.array_equal(got.k, want["cent"][want["run"]] * s)


def test_kmeans_fallbacks():
    wh = R.loop_wh(3)
    assert A.kmeans(_t(wh[:5]), 9).k is None                                        # fewer points than anchors
    two = np.repeat(np.array([[4.0, 2.0], [30.0, 11.0]], dtype=F32), 32, 0)         # 64 points, two distinct: every run loses a centroid
    res = A.kmeans(_t(two), 9)
    assert res.k is None and res.run == -1 and ((res.flags & 2) != 0).all() and res.iters == 1
    labels = [np.concatenate([np.zeros((64, 1)), np.full((64, 2), 0.5), two / 640.0], 1)]
    info = {}
    k = A.kmean_anchors((labels, np.array([[640, 640]])), n=9, img_size=640, gen=0, seed=4, info=info)
    rand = np.sort(np.random.RandomState(4).rand(18)).reshape(9, 2) * 640
    assert info["fallback"] and np.array_equal(k, rand[np.argsort(rand.prod(1))].astype(F32))


# ---- check_anchors -------------------------------------------------------------------------------------------------------------------
def _model():
    torch.manual_seed(0)
    return L.Model(L.load_cfg(scale="n")).to(_dev())


def _pixel_anchors(m):
    det = m.model[-1]
    return (det.anchors.float() * det.stride.to(det.anchors.device).view(-1, 1, 1)).view(-1, 2).cpu().numpy()


def _ref_bpr(labels, shapes, anchors, seed=0, thr=4.0):
    sc = np.random.RandomState(seed).uniform(0.9, 1.1, size=(len(shapes), 1))
    wh = R.label_wh(labels, shapes, 640, sc)
    return R.metric_sums(wh, anchors, thr)[1] / len(wh)


@functools.lru_cache(None)
def _replaced():
    """(model after check_anchors on SAR-like labels, the result, the anchors before, a GraphedForward captured before, its input)"""
    labels, shapes = R.dataset(2, kind="sar")
    m = _model().eval()
    before = _pixel_anchors(m)
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(3)).to(_dev())
    g = L.GraphedForward(m, x)
    assert not g.stale()
    res = L.check_anchors((labels, shapes), m, thr=4.0, imgsz=640, seed=0)
    return m, res, before, g, x


def test_check_anchors_replaces_poor_anchors():
    labels, shapes = R.dataset(2, kind="sar")
    m, res, before, g, _ = _replaced()
    want_bpr = _ref_bpr(labels, shapes, before)
    assert want_bpr < 0.98 and res.bpr == want_bpr                                  # the default anchors fail the reference's test on these labels
    assert res.replaced and res.new_bpr > res.bpr
    assert res.new_bpr == _ref_bpr(labels, shapes, res.anchors)
    k = L.kmean_anchors((labels, shapes), n=9, img_size=640, thr=4.0, gen=1000, seed=0)
    assert k.dtype == F32 and k.shape == (9, 2) and (np.diff(k.prod(1)) >= 0).all()
    assert np.array_equal(res.anchors, k) and np.array_equal(_pixel_anchors(m), k)  # level order: small to large, as the strides
    assert not np.array_equal(before, k)
    assert g.stale()                                                                # a forward captured before reports it


def test_check_anchors_keeps_good_anchors():
    labels, shapes = R.dataset(2, kind="coco")
    m = _model()
    det = m.model[-1]
    before, version = det.anchors.clone(), det.anchors._version
    res = L.check_anchors((labels, shapes), m)
    assert res.bpr > 0.98 and res.bpr == _ref_bpr(labels, shapes, _pixel_anchors(m)) and not res.replaced and res.new_bpr is None
    assert torch.equal(det.anchors, before) and det.anchors._version == version


def test_eval_forward_decodes_with_the_new_anchors():
    m, res, before, _, x = _replaced()
    det = m.model[-1]
    with torch.no_grad():
        z, p = m(x)
    def decode(pixel_anchors):                                                      # the float64 decode of the raw maps
        rows = []
        for i, pi in enumerate(p):
            a = pixel_anchors[i].view(1, det.na, 1, 1, 2)
            rows.append(((pi[..., 2:4].double().sigmoid() * 2) ** 2 * a).reshape(pi.shape[0], -1, 2))
        return torch.cat(rows, 1)

    want = decode(det.anchors.double() * det.stride.to(_dev()).double().view(-1, 1, 1))            # from the NEW buffer
    # (2 sigmoid)^2 doubles sigmoid's relative error: v_exp_f32 and v_rcp_f32 (1 ulp each) and the argument scaling of the fast exponential
    # (|x| * 1.44 * 2^-24, |x| <= 10) stay below 2.5e-6 together
    assert float(torch.cat([pi[..., 2:4].reshape(-1) for pi in p]).abs().max()) <= 10
    got = z[..., 2:4].double()
    assert got.shape == want.shape and ((got - want).abs() <= 1e-5 * want).all()
    old = decode(torch.from_numpy(before).double().to(_dev()).view(det.nl, det.na, 2))
    assert not ((got - old).abs() <= 1e-5 * old).all()                              # the anchors of before the replacement miss it


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_loss_built_before_follows_the_new_anchors(dtype):
    labels, shapes = R.dataset(2, kind="sar")
    m = _model().train()
    if dtype is torch.bfloat16:
        m = m.bfloat16()
    det = m.model[-1]
    gen = torch.Generator().manual_seed(11)
    bs, hw = 2, 256
    preds = [torch.randn(bs, det.na, hw // s, hw // s, det.no, generator=gen).to(_dev(), dtype) for s in (8, 16, 32)]
    # two targets per image, more than two cells apart on every level: no two candidates share a cell.  (The gradients of a shared cell are
    # added with float atomics in an order the scheduler chooses, so two runs of ONE loss object differ there in the last bit.)
    tg = torch.tensor([[0, 0, 0.27, 0.27, 0.08, 0.032], [0, 0, 0.77, 0.77, 0.15, 0.06],
                       [1, 0, 0.27, 0.77, 0.15, 0.06], [1, 0, 0.77, 0.27, 0.08, 0.032]]).to(_dev())

    def run(cl):
        ps = [p.clone().requires_grad_(True) for p in preds]
        loss, items = cl(ps, tg)
        loss.backward()
        return loss.detach().clone(), items.clone(), [p.grad.clone() for p in ps]

    early = L.ComputeLoss(m)
    l0, _, _ = run(early)                                                           # the loss object has run once: its constants are cached
    res = L.check_anchors((labels, shapes), m)
    assert res.replaced
    l1, i1, g1 = run(early)
    l2, i2, g2 = run(L.ComputeLoss(m))
    assert torch.equal(l1, l2) and torch.equal(i1, i2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    assert not torch.equal(l0, l2)                                                  # the anchors decide the matching: the loss did change


def test_check_anchors_input_forms():
    labels, _ = R.dataset(2, kind="sar")
    rng = np.random.default_rng(8)
    ims = []
    for _ in labels:                                                                # tiny pictures: only the aspect ratios matter
        long_side, short = 32, int(rng.integers(12, 33))
        h, w = (long_side, short) if rng.integers(2) else (short, long_side)
        ims.append(np.zeros((h, w, 3), np.uint8))
    bank = L.ImageBank(ims, labels, 32, device=_dev())
    shapes = bank.hw[:, ::-1].copy()

    class Dataset:
        pass

    ds = Dataset()
    ds.labels, ds.shapes = labels, shapes
    out = []
    for data in (bank, ds, (labels, shapes)):
        m = _model()
        res = L.check_anchors(data, m, thr=4.0, imgsz=640, seed=2)
        out.append((res.bpr, res.aat, res.new_bpr, res.replaced, res.anchors, _pixel_anchors(m)))
    assert out[0][3]
    for o in out[1:]:
        assert o[:4] == out[0][:4] and np.array_equal(o[4], out[0][4]) and np.array_equal(o[5], out[0][5])
