"""lead-yolo_amd/scene.py scene_plan and the restatements of tests/scene_ref.py, without a GPU: the plan's guarantees exhaustively, merge_ref
on hand-written cases, the premise of every GPU merge case (float32 and float64 take the same decisions) and the planted defects the judge
must catch."""
import numpy as np
import pytest

from lead_yolo_amd.scene import scene_plan
from tests.scene_ref import _rows, collect_ref, evaluated_pairs, margin, merge_cases, merge_ref, metric_matrix, tiles_ref

PLANS = [(32, 0), (32, 8), (32, 16), (64, 16)]


# ---------------------------------------------------------------------------------------------- 1. the tile plan
@pytest.mark.parametrize("tile, overlap", PLANS)
def test_plan_properties(tile, overlap):
    for L in range(1, 201):
        origins, (ny, nx) = scene_plan(L, 1, tile, overlap)
        assert origins.dtype == np.int32 and origins.shape == (ny, 2) and nx == 1 and (origins[:, 1] == 0).all()
        o = origins[:, 0].tolist()
        other, (my, mx) = scene_plan(1, L, tile, overlap)                     # the same arithmetic on the other axis
        assert other[:, 1].tolist() == o and (my, mx) == (1, ny)
        if L <= tile:
            assert o == [0]
            continue
        assert o[0] == 0 and o[-1] + tile == L and o == sorted(set(o))        # starts at 0, ends on the edge, strictly increasing
        covered = np.zeros(L, bool)
        for a in o:
            covered[a:a + tile] = True
        assert covered.all()
        assert all(a + tile - b >= overlap for a, b in zip(o, o[1:]))         # consecutive tiles share >= overlap pixels
        assert len(o) == -(-(L - tile) // (tile - overlap)) + 1
        for s in range(0, L - overlap + 1):                                   # every interval of length `overlap` lies inside some tile
            assert any(a <= s and s + overlap <= a + tile for a in o), (L, s)


def test_plan_order_and_refusals():
    origins, (ny, nx) = scene_plan(300, 420, 128, 32)
    assert (ny, nx) == (3, 5) and len(origins) == 15
    assert origins[:6].tolist() == [[0, 0], [0, 96], [0, 192], [0, 288], [0, 292], [96, 0]] and origins[-1].tolist() == [172, 292]
    assert len(scene_plan(8192, 8192)[0]) == 16 * 16
    for bad in (dict(tile=0), dict(tile=-32), dict(tile=32, overlap=-1), dict(tile=32, overlap=17), dict(tile=33, overlap=17)):
        with pytest.raises(ValueError, match="scene_plan"):
            scene_plan(100, 100, **bad)
    assert len(scene_plan(100, 100, 33, 16)[0]) == 25
    with pytest.raises(ValueError, match="scene_plan"):
        scene_plan(0, 100)


# ---------------------------------------------------------------------------------------------- 2. the restatements on hand-written cases
def test_tiles_ref_and_collect_ref_by_hand():
    scene = np.arange(3 * 4 * 3, dtype=np.uint8).reshape(3, 4, 3)
    t = tiles_ref(scene, [(1, 2), (0, 0)], 4)
    assert t.shape == (2, 3, 4, 4) and t[0, 0, 0, 0] == scene[1, 2, 2] and t[0, 2, 1, 1] == scene[2, 3, 0]
    assert (t[0, :, 2:] == 114).all() and (t[0, :, :, 2:] == 114).all() and (t[1, :, :3, :] == scene[:, :, ::-1].transpose(2, 0, 1)).all()
    g = tiles_ref(scene[:, :, 0], [(2, 3)], 4)
    assert (g[0, :, 0, 0] == scene[2, 3, 0]).all() and (g[0].reshape(3, -1)[:, 1:] == 114).all()
    dets = np.zeros((2, 2, 6), np.float32)
    dets[0, 0] = (-3, 5, 20, 30, 0.5, 1)
    dets[1, 0] = (10, 10, 40, 50, 0.25, 0)
    dets[1, 1] = (9, 9, 9, 9, 0.9, 2)                                          # past the count: dropped
    boxes, score = collect_ref(dets, [1, 1], [(0, 0), (70, 80)], 100, 110)
    assert boxes.dtype == np.float32 and boxes.tolist() == [[0, 5, 20, 30, 0.5, 1], [0] * 6, [90, 80, 110, 100, 0.25, 0], [0] * 6]
    assert score.tolist() == [0.5, -1, 0.25, -1]


FULL, PART = (100, 100, 160, 130, 0.9, 0), (100, 100, 112, 130, 0.8, 0)          # a ship, and the fifth of it a tile border left


def test_merge_ref_by_hand():
    b, s = _rows({(0, 0): FULL, (1, 0): PART}, 2, 2)
    assert merge_ref(b, s, 2, "ios", 0.5) == [0] and merge_ref(b, s, 2, "iou", 0.45) == [0, 2]      # IoS 1.0, IoU 0.2
    assert margin(b, "iou", 0.45, s, 2, False) == pytest.approx(0.25) and margin(b, "ios", 0.5, s, 2, False) == pytest.approx(0.5)
    b, s = _rows({(0, 0): FULL, (0, 1): PART}, 2, 2)                           # the same pair inside one tile: nms_padded's business
    assert merge_ref(b, s, 2, "ios", 0.5) == [0, 1] and merge_ref(b, s, 2, "iou", 0.45) == [0, 1]
    assert margin(b, "ios", 0.5, s, 2, False) == np.inf
    # equal scores: the lower row first, and it is the one that stays
    b, s = _rows({(0, 1): FULL[:4] + (0.7, 0), (1, 0): FULL[:4] + (0.7, 0), (1, 1): (0, 0, 5, 5, 0.7, 0)}, 2, 2)
    assert merge_ref(b, s, 2, "iou", 0.45) == [1, 3]
    assert merge_ref(b, s, 2, "iou", 0.45, defect="unstable") == [3, 2]
    # classes: compared unless agnostic
    b, s = _rows({(0, 0): FULL, (1, 0): PART[:5] + (1,)}, 1, 2)
    assert merge_ref(b, s, 1, "ios", 0.5) == [0, 1] and merge_ref(b, s, 1, "ios", 0.5, agnostic=True) == [0]
    # a suppressed box suppresses nothing: C overlaps B (dropped by A) but not A
    b, s = _rows({(0, 0): (0, 0, 10, 10, 0.9, 0), (1, 0): (4, 0, 14, 10, 0.8, 0), (2, 0): (9, 0, 19, 10, 0.7, 0)}, 1, 3)
    assert merge_ref(b, s, 1, "ios", 0.5) == [0, 2]
    # the cuts: five boxes far apart, by descending score rows 4, 3, 2, 1, 0
    b, s = _rows({(t, 0): (50 * t, 0, 50 * t + 10, 10, 0.1 * (t + 1), 0) for t in range(5)}, 1, 5)
    st = {}
    assert merge_ref(b, s, 1, "ios", 0.5, stats=st) == [4, 3, 2, 1, 0] and st["suppressed"] == 0
    assert merge_ref(b, s, 1, "ios", 0.5, max_det=2) == [4, 3] and merge_ref(b, s, 1, "ios", 0.5, max_merge=3) == [4, 3, 2]
    b[3, :4] = b[4, :4]                                                       # row 3 duplicates row 4: max_merge counts candidates, max_det kept boxes
    assert merge_ref(b, s, 1, "ios", 0.5, max_merge=3) == [4, 2] and merge_ref(b, s, 1, "ios", 0.5, max_det=2) == [4, 2]
    # a box without area: the denominator of IoS is 0 -> m = 0
    b, s = _rows({(0, 0): (0, 0, 10, 10, 0.9, 0), (1, 0): (5, 5, 5, 9, 0.8, 0)}, 1, 2)
    assert merge_ref(b, s, 1, "ios", 0.5) == [0, 1] and metric_matrix(b, "ios", np.float32)[0, 1] == 0


# ---------------------------------------------------------------------------------------------- 3. the premise of the GPU merge cases
@pytest.mark.parametrize("name", sorted(merge_cases()))
def test_merge_case_premise(name):
    """float32 (the kernel's arithmetic, the header's operation order) and float64 (merge_ref) decide every pair alike: each evaluated pair is
    at least 1e-4 from the threshold — or, for the `exact` case, whose pairs sit AT the threshold, float32 computes the metric without rounding"""
    boxes, score, mdt, variants, exact = merge_cases()[name]
    assert boxes.dtype == np.float32 and score.dtype == np.float32 and len(boxes) == len(score) and len(boxes) % mdt == 0
    assert np.array_equal(score[score >= 0], boxes[score >= 0, 4]) and not boxes[score < 0].any()
    for v in variants:
        agnostic = v.get("agnostic", False)
        pair = evaluated_pairs(boxes, score, mdt, agnostic)
        m32, m64 = metric_matrix(boxes, v["metric"], np.float32), metric_matrix(boxes, v["metric"], np.float64)
        t32, t64 = np.float32(v["thres"]), v["thres"]
        assert np.array_equal((m32 > t32)[pair], (m64 > t64)[pair]), v
        if exact:
            assert np.array_equal(m32.astype(np.float64)[pair], m64[pair]) and float(t32) == t64 and (m64[pair] == t64).any(), v
        else:
            assert margin(boxes, v["metric"], v["thres"], score, mdt, agnostic) >= 1e-4, v


def test_merge_cases_cover_the_ground():
    cases = merge_cases()
    live = {k: int((c[1] >= 0).sum()) for k, c in cases.items()}
    assert live["n1"] == 1 and live["n8"] == 8 and live["allpad"] == 0 and live["merge50"] == 80 and 1100 <= live["n1260"] <= 1260
    assert all(len(cases[k][0]) % d for k in ("n111", "n305") for d in (32, 64, 256))
    b, s, mdt, _, _ = cases["n111"]
    assert len(merge_ref(b, s, mdt, "ios", 0.5)) > 7                          # max_det = 7 cuts survivors
    assert merge_ref(b, s, mdt, "ios", 0.5, max_det=7) == merge_ref(b, s, mdt, "ios", 0.5)[:7]
    b, s, mdt, _, _ = cases["merge50"]
    assert merge_ref(b, s, mdt, "ios", 0.5, max_merge=50) != merge_ref(b, s, mdt, "ios", 0.5)
    b, s, mdt, _, _ = cases["far"]
    assert b[:, :4].max() > 2 * 7680 and {0, 2} <= set(merge_ref(b, s, mdt, "ios", 0.5)) and 6 not in merge_ref(b, s, mdt, "ios", 0.5)
    b, s, mdt, _, _ = cases["ties"]
    assert len(np.unique(s[s >= 0])) < live["ties"] / 4
    for k in ("n8", "n111", "n305", "n1260", "ties"):                         # agnostic matters, both metrics matter, boxes get dropped
        b, s, mdt, _, _ = cases[k]
        st = {}
        a = merge_ref(b, s, mdt, "ios", 0.5, stats=st)
        assert st["suppressed"] > 0, k
        if k != "n8":
            assert a != merge_ref(b, s, mdt, "ios", 0.5, agnostic=True) and a != merge_ref(b, s, mdt, "iou", 0.45), k


@pytest.mark.parametrize("defect, where", [("cls_offset", "far"), ("no_exempt", "n111"), ("unstable", "ties"), ("ge", "exact")])
def test_planted_defects_are_caught(defect, where):
    """the judge of the GPU cases — equality of the kept rows with merge_ref on these inputs — tells each mutation from the rule, on the case
    that was written for it"""
    b, s, mdt, variants, _ = merge_cases()[where]
    caught = [i for i, v in enumerate(variants) if merge_ref(b, s, mdt, defect=defect, **v) != merge_ref(b, s, mdt, **v)]
    print(defect, "caught by", where, caught)
    assert caught
