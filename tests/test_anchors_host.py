"""The restatements of tests/anchors_ref.py against a literal transcription of utils/autoanchor.py (float32 torch means), the mutation
table against the reference's draws, the premises the device cases of tests/test_gpu_anchors.py rest on, and the planted defects.
Host only: no GPU."""
import math
import random
import re

import numpy as np
import pytest
import torch

import lead_yolo_amd as L
from lead_yolo_amd import anchors as A, capi
from tests import anchors_ref as R

THR = 4.0


# ---- literal transcription (autoanchor.py:38-44, 104-116, 156-165) ------------------------------------------------------------------
def t_metric(k, wh, thr):
    r = wh[:, None] / k[None]
    x = torch.min(r, 1 / r).min(2)[0]
    best = x.max(1)[0]
    aat = (x > 1 / thr).float().sum(1).mean()
    bpr = (best > 1 / thr).float().mean()
    return bpr, aat


def t_fitness(k, wh, thr):
    r = wh[:, None] / torch.tensor(k, dtype=torch.float32)[None]
    best = torch.min(r, 1 / r).min(2)[0].max(1)[0]
    return (best * (best > 1 / thr).float()).mean()


def t_evolve(k, wh, thr, gen, npr, rnd):
    """the `for _ in pbar` loop, drawing from the generators it is given; -> k, f, accepted generations, the v it drew"""
    f, sh, mp, s = t_fitness(k, wh, thr), k.shape, 0.9, 0.1
    accepted, drawn = [], []
    for g in range(gen):
        v = np.ones(sh)
        while (v == 1).all():
            v = ((npr.random(sh) < mp) * rnd.random() * npr.randn(*sh) * s + 1).clip(0.3, 3.0)
        drawn.append(v)
        kg = (k.copy() * v).clip(min=2.0)
        fg = t_fitness(kg, wh, thr)
        if fg > f:
            f, k = fg, kg.copy()
            accepted.append(g)
    return k, float(f), accepted, np.stack(drawn)


@pytest.mark.parametrize("seed,gen,thr", [(1, 1000, 4.0), (2, 300, 2.9)])
def test_restatement_matches_transcription(seed, gen, thr):
    wh = R.wh_set(seed)
    n = len(wh)
    wt = torch.from_numpy(wh.copy())
    bpr, aat = t_metric(torch.from_numpy(R.COCO_ANCHORS.copy()), wt, thr)
    s, nb, nx = R.metric_sums(wh, R.COCO_ANCHORS, thr)
    assert abs(float(bpr) - nb / n) <= 1e-6 * (nb / n) and abs(float(aat) - nx / n) <= 1e-6 * (nx / n)
    assert float(bpr) < 0.98                                                        # the SAR-like sizes do fail the reference's test
    k0 = R.COCO_ANCHORS.astype(np.float64)
    kt, ft, acc_t, v = t_evolve(k0.copy(), wt, thr, gen, np.random.RandomState(seed), random.Random(seed))
    assert np.array_equal(v, A.mutation_table(gen, (9, 2), seed))
    kr, fr, acc_r = R.evolve(wh, k0, v, thr)
    assert acc_r == acc_t and len(acc_r) >= 20                                       # the same chain; no near-tie for these seeds
    assert np.array_equal(kr, kt)
    assert abs(ft - fr / n) <= 1e-6 * (fr / n)                                      # float32 mean against the exact sum: n * 2^-24 * small


def test_mutation_table():
    v = A.mutation_table(200, (9, 2), seed=5)
    assert v.shape == (200, 9, 2) and v.dtype == np.float64
    assert not (v == 1).all((1, 2)).any() and v.min() >= 0.3 and v.max() <= 3.0
    assert np.array_equal(v, A.mutation_table(200, (9, 2), seed=5)) and not np.array_equal(v, A.mutation_table(200, (9, 2), seed=6))
    # what the reference's loop draws from the GLOBAL generators seeded alike (their state is put back afterwards)
    st_np, st_py = np.random.get_state(), random.getstate()
    try:
        np.random.seed(5)
        random.seed(5)
        _, _, _, drawn = t_evolve(np.full((9, 2), 30.0), torch.full((8, 2), 20.0), THR, 200, np.random, random)
    finally:
        np.random.set_state(st_np)
        random.setstate(st_py)
    assert np.array_equal(v, drawn)
    # a table of three anchors that hits the `while (v == 1).all()` redraw somewhere still never holds an all-ones generation
    assert not (A.mutation_table(3000, (1, 2), seed=0) == 1).all((1, 2)).any()


def test_premise_a_fitness_sums_are_exact():
    for seed, thr in ((1, 4.0), (2, 2.9)):
        t = R.metric_terms(R.wh_set(seed), R.COCO_ANCHORS, thr)[0].astype(np.float64)
        assert len(t) > 1000 and t.min() > 0.25 and t.max() <= 1.0
        assert math.fsum(t) == float(np.sum(t)) == float(np.sum(t[::-1])) == float(np.cumsum(t)[-1])


@pytest.mark.parametrize("n,runs", [(64, 1), (64, 30), (4099, 1), (4099, 30)])
def test_premise_b_one_iteration(n, runs):
    pts, cent = R.step_points(10 + runs, n, runs)
    assign, count, new, dist, empty, d2 = R.lloyd_step(pts, cent)
    assert (R.margins(d2) > 1e-5).all()                                             # every point, every run
    p64 = pts.astype(np.float64)
    for r in range(runs):
        for c in range(cent.shape[1]):
            sel = p64[assign[r] == c]
            for a in (0, 1):
                assert math.fsum(sel[:, a]) == float(sel[:, a].sum()) == float(sel[::-1, a].sum())
    if n == 64 and runs == 30:
        assert empty.any() and not empty.all()                                      # the discarded-run case is in the data
    if n == 4099:
        assert not empty.any()


def test_premise_b_whole_loop():
    wh = R.loop_wh(3)
    res, bad, near, gap = R.loop_premises(wh, 9, 30, 3)
    assert len(bad) == 0 and near > 1e-9 and gap > 1e-9
    assert res["run"] >= 0 and 5 < res["iters"] < R.KMEANS_MAX_ITER and len(set(res["run_iters"])) > 3      # runs close at different iterations


def test_planted_defects_are_caught():
    wh, k0 = R.wh_set(1), R.COCO_ANCHORS
    good = R.metric_sums(wh, k0, THR)
    assert R.metric_sums(wh, k0, THR, "no_recip") != good                           # 1 / r omitted
    # labels exactly at the threshold: w / k = 1 / thr on one side, inside on the other
    at = np.stack([k0[:, 0] / np.float32(THR), k0[:, 1]], 1).astype(np.float32)
    assert R.metric_sums(at, k0, THR)[1:] != R.metric_sums(at, k0, THR, "ge")[1:]   # `>` taken as `>=`
    v = A.mutation_table(300, (9, 2), 1)
    k, f, acc = R.evolve(wh, k0, v, THR)
    for defect in ("no_reeval", "no_clip"):
        kd, fd, accd = R.evolve(wh, k0, v, THR, defect=defect)
        assert accd != acc and not np.array_equal(kd, k), defect
    # clip(min=2) matters on its own data too: a 3 px anchor mutated below 2
    small = np.array([[2.1, 2.2], [3.0, 9.0], [8.0, 30.0]])
    vs = A.mutation_table(50, (3, 2), 2)
    assert ((small * vs) < 2.0).any()
    pts, s = R.whiten(R.loop_wh(3))
    init = pts[R.kmeans_init(len(pts), 9, 30, 3)]
    a, b = R.lloyd(pts, init), R.lloyd(pts, init, defect="stale_assign")
    assert not np.array_equal(a["cent"], b["cent"])                                 # a centroid updated from the previous assignment


def test_label_wh_restatement():
    labels, shapes = R.dataset(2)
    assert any(len(lb) == 0 for lb in labels)
    sc = np.random.RandomState(0).uniform(0.9, 1.1, size=(len(shapes), 1))
    norm = 640 * shapes / shapes.max(1, keepdims=True)
    want = np.concatenate([lb[:, 3:5] * s for s, lb in zip(norm * sc, labels)])    # check_anchors' own line
    assert np.array_equal(R.label_wh(labels, shapes, 640, sc), want.astype(np.float32))
    assert R.label_wh(labels, shapes, 640).dtype == np.float32


def test_abi_and_exports():
    text = open(capi.HEADER_PATH).read()
    for fn in ("ly_anchor_wh", "ly_anchor_metric", "ly_anchor_evolve_eval", "ly_anchor_evolve_pick", "ly_kmeans_assign", "ly_kmeans_update"):
        assert re.search(rf"^int {fn}\(", text, re.M) and fn in capi.SIGNATURES and hasattr(capi.lib(), fn)
    assert text.count("autoanchor.py:") >= 4                                        # every entry cites the lines it replaces
    assert capi.lib().ly_abi_version() == 5
    for name in ("check_anchors", "kmean_anchors", "anchor_metric", "label_wh", "kmeans", "evolve"):
        assert getattr(L, name) is getattr(A, name)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.label_wh([np.zeros((1, 5))], np.array([[640, 480]]), 640, device="cpu")
