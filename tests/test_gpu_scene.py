"""csrc/ly_scene.hip (ly_scene_tiles_u8, ly_scene_collect, ly_scene_nms) and lead-yolo_amd/scene.py on the device: the three entries bit for
bit against the numpy restatements of tests/scene_ref.py — the merge on the seeded inputs whose premise tests/test_scene_host.py holds — and
SceneDetector end to end against the same pipeline assembled by hand from the restatements and the existing pieces."""
import functools

import numpy as np
import pytest
import torch

from tests.scene_ref import collect_ref, margin, merge_cases, merge_ref, tiles_ref
from tests.test_gpu_augment import _model as _synth_model
from tests.test_gpu_modules import _dev
from tests.test_letterbox_host import rand_image

pytestmark = pytest.mark.gpu
T = 32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _grey(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- 1. ly_scene_tiles_u8
def _origins(H, W):
    """the origin, the interior at odd x0 (no source alignment holds), the last pixel, the last row / column alone, and one origin twice"""
    o = [(0, 0), (H // 2, (W // 2) | 1 if W > 1 else 0), (H - 1, W - 1), (H - 1, 0), (0, W - 1)]
    return [(min(y, H - 1), min(x, W - 1)) for y, x in o]


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("H, W", [(1, 1), (31, 47), (32, 32), (70, 101), (48, 64)])
def test_tiles_bit_for_bit(H, W, C):
    """fill on the right, at the bottom and on both; rows whose first byte is 16-byte aligned (48 x 64: all of them), 4-byte aligned and
    unaligned; n = 1 and n = 5 with a repeated origin; a pitched view: a column slice of a wider tensor, whose first byte is odd"""
    import lead_yolo_amd as L
    scene = rand_image(H, W, 7 * H + W) if C == 3 else _grey(H, W, 7 * H + W)
    o = _origins(H, W)
    five = o[:4] + [o[1]]
    want = tiles_ref(scene, five, T)
    if H > T // 2 and W > T // 2:
        assert (want[1] == 114).any() and (want[1] != 114).any()
    got = L.scene_tiles(_t(scene), five, T)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (5, 3, T, T)
    assert np.array_equal(got.cpu().numpy(), want)
    for k in (0, 1):                                                          # n = 1, into a slice of a larger buffer
        buf = torch.zeros((3, 3, T, T), dtype=torch.uint8, device=_dev())
        out = L.scene_tiles(_t(scene), o[k:k + 1], T, out=buf[1:2])
        assert out.data_ptr() == buf[1].data_ptr() and np.array_equal(buf[1].cpu().numpy(), want[k]) and not buf[0].any() and not buf[2].any()
    assert np.array_equal(L.scene_tiles(scene, five, T, device=_dev()).cpu().numpy(), want)                # a host scene: one pinned block
    wide = np.random.default_rng(3).integers(0, 256, (H, W + 11) + scene.shape[2:], dtype=np.uint8)
    wide[:, 3:3 + W] = scene
    view = _t(wide)[:, 3:3 + W]
    assert not view.is_contiguous() or H == 1
    assert view.data_ptr() % 4 != 0
    assert np.array_equal(L.scene_tiles(view, five, T).cpu().numpy(), want)
    rows = _t(np.concatenate([wide, wide]))[H:, 3:3 + W]                    # a row and column view
    assert np.array_equal(L.scene_tiles(rows, five, T).cpu().numpy(), want)


def test_tiles_beyond_2_31_bytes():
    """a 46 500 x 16 000 x 3 scene (2.2 GB, never initialised) with four seeded 32 x 32 windows: the origin, the far corner, and the rows just
    below and just above byte 2^31 (row 44 739 holds it)"""
    import lead_yolo_amd as L
    H, W = 46500, 16000
    assert 44739 * W * 3 < 2 ** 31 < 44740 * W * 3
    origins = [(0, 0), (H - T, W - T), (44739 - T, 5001), (44740, 5001)]
    scene = torch.empty((H, W, 3), dtype=torch.uint8, device=_dev())
    pat = [rand_image(T, T, 900 + k) for k in range(4)]
    for (y, x), p in zip(origins, pat):
        scene[y:y + T, x:x + T] = _t(p)
    got = L.scene_tiles(scene, origins, T).cpu().numpy()
    for k, p in enumerate(pat):
        assert np.array_equal(got[k], p[:, :, ::-1].transpose(2, 0, 1)), origins[k]
    grey = scene.view(H, W * 3)                                               # the same bytes as one grey plane of 48 000 columns
    g = L.scene_tiles(grey, [(H - T, 3 * (W - T)), (44740, 3 * 5001)], T).cpu().numpy()
    assert np.array_equal(g[0, 1], pat[1].reshape(T, T * 3)[:, :T]) and np.array_equal(g[1, 2], pat[3].reshape(T, T * 3)[:, :T])
    del scene, grey
    torch.cuda.empty_cache()


def test_tiles_refusals():
    import lead_yolo_amd as L
    capi = L.capi
    lib, st = capi.lib(), capi.stream_ptr()
    scene, dst = _t(rand_image(40, 50, 1)), torch.zeros((1, 3, 48, 48), dtype=torch.uint8, device=_dev())
    org = torch.zeros((1, 2), dtype=torch.int32, device=_dev())

    def call(C=3, pitch=150, T=32, d=None):
        d = dst.data_ptr() if d is None else d
        return lib.ly_scene_tiles_u8(capi.ptr(scene), 40, 50, C, pitch, capi.ptr(org), 1, T, d, st)

    assert call() == 0
    for kw, msg in ((dict(T=24), "multiple of 16"), (dict(T=0), "multiple of 16"), (dict(C=2), "C = 2"), (dict(pitch=149), "pitch"),
                    (dict(d=dst.data_ptr() + 8), "16-byte aligned")):
        with pytest.raises(capi.HipLibraryError, match=msg):
            capi.check(call(**kw), "ly_scene_tiles_u8")
    for bad in ([(40, 0)], [(0, 50)], [(0, 0), (-1, 3)]):
        with pytest.raises(ValueError, match="outside the 40 x 50 scene"):
            L.scene_tiles(scene, bad, T)
    with pytest.raises(ValueError, match="multiple of 16"):
        L.scene_tiles(scene, [(0, 0)], 40)
    with pytest.raises(ValueError, match="out must be"):
        L.scene_tiles(scene, [(0, 0)], T, out=dst)
    with pytest.raises(ValueError, match="unit pixel stride"):
        L.scene_tiles(scene[:, ::2], [(0, 0)], T)
    with pytest.raises(ValueError, match="unit pixel stride"):
        L.scene_tiles(scene[:, :, 0], [(0, 0)], T)                            # a grey view with a pixel stride of 3
    with pytest.raises(ValueError, match=r"uint8 \[H, W, 3\]"):
        L.scene_tiles(scene[:, :, :2], [(0, 0)], T)
    with pytest.raises(NotImplementedError, match="16-bit"):
        L.scene_tiles(np.zeros((40, 50), np.uint16), [(0, 0)], T, device=_dev())


# ---------------------------------------------------------------------------------------------- 2. ly_scene_collect
@pytest.mark.parametrize("n_tiles, max_det", [(1, 1), (1, 5), (7, 1), (7, 5)])
def test_collect_bit_for_bit(n_tiles, max_det):
    import lead_yolo_amd as L
    rng = np.random.default_rng(20 + n_tiles + max_det)
    H, W = 300, 420
    dets = rng.uniform(-8, 136, (n_tiles, max_det, 6)).astype(np.float32)      # past every border of a 128-pixel tile
    dets[..., 4:] = rng.uniform(0, 1, (n_tiles, max_det, 2))
    dets[..., 5] = np.round(dets[..., 5] * 3)
    counts = np.array([max_det, 0, max_det // 2, 1, 0, max_det, max_det - 1][:n_tiles], np.int32)
    if n_tiles == 7:
        dets[0, 0, :4], dets[5, 0, :4] = (-3, -2, 50, 60), (5, 5, 100, 100)   # across the scene's left / top and right / bottom edges
    origins = np.array(([(0, 0), (172, 292), (96, 292), (172, 96), (0, 0), (250, 400), (299, 419)])[:n_tiles], np.int32)
    for cnt in ([counts] if n_tiles > 1 else [counts, np.zeros(1, np.int32)]):
        want_b, want_s = collect_ref(dets, cnt, origins, H, W)
        got_b, got_s = L.scene_collect(_t(dets), _t(cnt), _t(origins), H, W)
        assert np.array_equal(got_b.cpu().numpy().view(np.uint32), want_b.view(np.uint32))
        assert np.array_equal(got_s.cpu().numpy().view(np.uint32), want_s.view(np.uint32))
        if n_tiles == 7 and max_det == 5:                                     # boxes cross the left / top, right and bottom edges
            live = want_s >= 0
            assert (want_b[live, 0] == 0).any() and (want_b[live, 2] == W).any() and (want_b[live, 3] == H).any() and (~live).any()
    with pytest.raises(ValueError, match="scene_collect"):
        L.scene_collect(_t(dets), _t(counts), _t(origins[:, :1]), H, W)


# ---------------------------------------------------------------------------------------------- 3. ly_scene_nms
@functools.lru_cache(maxsize=None)
def _want_keep(name, i):
    b, s, mdt, variants, _ = merge_cases()[name]
    return merge_ref(b, s, mdt, **variants[i])


@pytest.mark.parametrize("name", sorted(merge_cases()))
def test_merge_equals_merge_ref(name):
    """keep and count equal to the float64 loop on the inputs whose premise tests/test_scene_host.py holds; twice: the same bits"""
    import lead_yolo_amd as L
    b, s, mdt, variants, _ = merge_cases()[name]
    boxes, score = _t(b), _t(s)
    for i, v in enumerate(variants):
        want = _want_keep(name, i)
        kw = dict(metric=v["metric"], thres=v["thres"], agnostic=v.get("agnostic", False), max_det=v.get("max_det", 1500),
                  max_merge=v.get("max_merge", 30000))
        keep, count = L.scene_merge(boxes, score, mdt, **kw)
        keep2, count2 = L.scene_merge(boxes, score, mdt, **kw)
        k, c = keep.cpu().numpy(), int(count.item())
        assert keep.dtype == torch.int32 and tuple(keep.shape) == (kw["max_det"],) and tuple(count.shape) == (1,)
        assert c == len(want) and k[:c].tolist() == want and not k[c:].any(), (name, v, c, len(want))
        assert torch.equal(keep, keep2) and torch.equal(count, count2)
    if name == "far":
        assert {0, 2} <= set(_want_keep(name, 0))                             # the two classes 7680 apart both survive
    if name == "allpad":
        assert _want_keep(name, 0) == []


def test_merge_refusals():
    import lead_yolo_amd as L
    b, s, mdt, _, _ = merge_cases()["n8"]
    with pytest.raises(ValueError, match="'iou' or 'ios'"):
        L.scene_merge(_t(b), _t(s), mdt, metric="union")
    with pytest.raises(L.capi.HipLibraryError, match="max_merge=30001"):
        L.scene_merge(_t(b), _t(s), mdt, max_merge=30001)
    with pytest.raises(ValueError, match="score must be"):
        L.scene_merge(_t(b), _t(s[:-1]), mdt)


# ---------------------------------------------------------------------------------------------- 4. SceneDetector end to end
SH, SW, TILE, OVERLAP, BS, CONF, IOU, MDT = 300, 420, 128, 32, 4, 0.001, 0.45, 60
KW = dict(tile=TILE, overlap=OVERLAP, batch_size=BS, conf_thres=CONF, iou_thres=IOU, max_det_tile=MDT)


@functools.lru_cache(maxsize=None)
def _net():
    """tests/test_gpu_letterbox.py's _net(), restated: lead-yolo-n, random weights of a fixed seed, the heads' biases lifted by 2 so that a
    random network passes boxes through conf_thres = 0.001"""
    m, st = _synth_model("n", 8100)
    for i in range(len(m.model[-1].m)):
        st[f"model.23.m.{i}.bias"] = st[f"model.23.m.{i}.bias"] + 2.0
    m.load_state_dict(st)
    return m.to(_dev()).eval()


@functools.lru_cache(maxsize=None)
def _scene():
    return rand_image(SH, SW, 777)


def _hand_tiles(m, forward, scene, tile=TILE, overlap=OVERLAP, bs=BS, mdt=MDT):
    """the tiles cut by tiles_ref, through `forward` in the batch slots SceneDetector uses (free slots 114), then nms_padded -> (dets, counts,
    origins) on the host"""
    import lead_yolo_amd as L
    origins, _ = L.scene_plan(scene.shape[0], scene.shape[1], tile, overlap)
    tiles = tiles_ref(scene, origins, tile)
    dets, counts = [], []
    for lo in range(0, len(origins), bs):
        k = min(bs, len(origins) - lo)
        batch = np.full((bs, 3, tile, tile), 114, np.uint8)
        batch[:k] = tiles[lo:lo + k]
        x = torch.from_numpy(batch).to(_dev())
        d, c, _ = L.nms_padded(forward(x if getattr(m, "u8_input", False) else x.float() / 255), CONF, IOU, max_det=mdt)
        dets.append(d[:k].cpu().numpy())
        counts.append(c[:k].cpu().numpy())
    return np.concatenate(dets), np.concatenate(counts), origins


def _hand_scene(dets, counts, origins, H, W, mdt=MDT, metric="ios", thres=0.5, stats=None):
    boxes, score = collect_ref(dets, counts, origins, H, W)
    return boxes[merge_ref(boxes, score, mdt, metric, thres, stats=stats)], boxes, score


def _check_scene(sd, scene, hand):
    dets, counts, origins = hand
    td, tc, to = sd.tiles_padded(scene)
    assert np.array_equal(to.cpu().numpy(), origins) and to.dtype == torch.int32 and len(origins) == 15
    assert np.array_equal(tc.cpu().numpy(), counts) and np.array_equal(td.cpu().numpy().view(np.uint32), dets.view(np.uint32))
    st = {}
    want, boxes, score = _hand_scene(dets, counts, origins, SH, SW, stats=st)
    mg = margin(boxes, "ios", 0.5, score, MDT, False)
    print(f"tiles with detections {int((counts > 0).sum())} of {len(counts)}, candidates {int(counts.sum())}, kept {len(want)}, "
          f"suppressed across tiles {st['suppressed']}, margin {mg:.3g}")
    assert (counts > 0).sum() >= 8 and st["suppressed"] >= 1 and len(want) >= 1, "the seed of _net() / _scene() is wrong: nothing to merge"
    got = sd(scene)
    assert got.shape == want.shape and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert (want[:, [0, 2]] <= SW).all() and (want[:, [1, 3]] <= SH).all() and (want[:, :4] >= 0).all() and (want[:, 2] > TILE).any()
    return want


def test_scene_detector_eager_equals_the_pipeline_by_hand():
    import lead_yolo_amd as L
    m, scene = _net(), _scene()
    with torch.no_grad():
        hand = _hand_tiles(m, lambda x: m(x)[0], scene)
    sd = L.SceneDetector(m, graphed=False, **KW)
    assert not sd.stale() and sd.stride == 32 and not sd.graphed
    want = _check_scene(sd, scene, hand)
    # the other metric, by hand as well; a list of scenes returns a list
    iou = L.SceneDetector(m, graphed=False, metric="iou", merge_thres=0.45, **KW)
    want_iou = _hand_scene(*hand, SH, SW, metric="iou", thres=0.45)[0]
    got = iou([scene, scene])
    assert isinstance(got, list) and len(got) == 2 and all(np.array_equal(g.cpu().numpy(), want_iou) for g in got)
    dets, count = sd.padded(scene)
    assert tuple(dets.shape) == (3000, 6) and count.dtype == torch.int32 and int(count) == len(want) and not dets[len(want):].any()


def test_scene_detector_graphed_equals_the_graph_by_hand():
    import lead_yolo_amd as L
    m, scene = _net(), _scene()
    example = torch.full((BS, 3, TILE, TILE), 114, dtype=torch.uint8, device=_dev())
    g = L.GraphedForward(m, example if getattr(m, "u8_input", False) else example.float() / 255)
    hand = _hand_tiles(m, lambda x: g(x)[0], scene)
    sd = L.SceneDetector(m, **KW)
    assert sd.graphed and not sd.stale()
    _check_scene(sd, scene, hand)
    _check_scene(sd, scene, hand)                                             # a second pass over the same graph


def test_one_tile_scene_equals_detector():
    """a scene of exactly one tile returns what the per-tile NMS returned: Detector's boxes for that image, bit for bit"""
    import lead_yolo_amd as L
    m = _net()
    scene = rand_image(TILE, TILE, 778)
    det = L.Detector(m, img_size=TILE, batch_size=BS, conf_thres=CONF, iou_thres=IOU, max_det=MDT, round_boxes=False, graphed=False)
    want = det([scene])[0]
    got = L.SceneDetector(m, graphed=False, **KW)(scene)
    assert len(want) > 1 and got.shape == want.shape and torch.equal(got, want)


def test_scene_smaller_than_a_tile():
    import lead_yolo_amd as L
    m = _net()
    scene = rand_image(90, 100, 779)
    sd = L.SceneDetector(m, graphed=False, **KW)
    td, tc, to = sd.tiles_padded(scene)
    assert to.tolist() == [[0, 0]] and tuple(td.shape) == (1, MDT, 6) and int(tc[0]) > 1
    with torch.no_grad():
        hand = _hand_tiles(m, lambda x: m(x)[0], scene)
    want = _hand_scene(*hand, 90, 100)[0]
    got = sd(scene).cpu().numpy()
    assert np.array_equal(got, want) and len(want) == int(tc[0])
    assert got[:, 2].max() <= 100 and got[:, 3].max() <= 90
    raw = td[0, :int(tc[0])].cpu().numpy()
    assert (raw[:, 2] > 100).any() or (raw[:, 3] > 90).any(), "no box reaches past the scene: the clip is not exercised"


def test_sources_grey_and_no_host_sync():
    import lead_yolo_amd as L
    m, dev = _net(), _dev()
    scene = _scene()
    sd = L.SceneDetector(m, **KW)
    want, want_n = sd.padded(scene)
    want, want_n = want.clone(), want_n.clone()
    on_dev = _t(scene)
    wide = _t(np.concatenate([scene, scene], 1))[:, SW - 7:2 * SW - 7]       # a pitched view of the same pixels, rolled by 7 columns
    rolled = _t(np.roll(scene, 7, 1))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a, an = sd.padded(scene)
        a, an = a.clone(), an.clone()
        b, bn = sd.padded(on_dev)
        b, bn = b.clone(), bn.clone()
        c, cn = sd.padded(wide)
        c, cn = c.clone(), cn.clone()
        r, rn = sd.padded(rolled)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert int(want_n) > 0 and torch.equal(a, want) and torch.equal(an, want_n) and torch.equal(b, want) and torch.equal(bn, want_n)
    assert torch.equal(c, r) and torch.equal(cn, rn)
    # one grey plane equals the same plane stacked to three equal channels
    grey = _grey(SH, SW, 780)
    g3 = sd(np.stack([grey] * 3, -1)).clone()
    g1 = sd(_t(grey))
    assert len(g3) > 0 and torch.equal(g1, g3) and torch.equal(sd(grey), g3)


def test_scene_detector_refusals_and_staleness():
    import lead_yolo_amd as L
    from lead_yolo_amd import pack
    m0 = _net()
    with pytest.raises(RuntimeError, match="eval"):
        L.SceneDetector(torch.nn.Linear(1, 1))                                # a module in training mode
    with pytest.raises(ValueError, match="stride"):
        L.SceneDetector(m0, tile=72, graphed=False)
    with pytest.raises(ValueError, match="overlap"):
        L.SceneDetector(m0, tile=128, overlap=65, graphed=False)
    with pytest.raises(ValueError, match="'iou'"):
        L.SceneDetector(m0, metric="union", graphed=False)
    with pytest.raises(NotImplementedError, match="augment"):
        L.SceneDetector(m0, augment=True, graphed=False)
    sd0 = L.SceneDetector(m0, graphed=False, **KW)
    with pytest.raises(NotImplementedError, match="16-bit"):
        sd0(np.zeros((SH, SW), np.uint16))
    with pytest.raises(ValueError, match="unit pixel stride"):
        sd0(_t(_scene())[:, ::2])
    # staleness, as test_detector_staleness: a model of its own, since the weights move
    m, _ = _synth_model("n", 8100)
    m.load_state_dict({k: v.cpu() for k, v in m0.state_dict().items()})
    m = m.to(_dev()).eval()
    scene = _scene()
    sd = L.SceneDetector(m, **KW)
    before = sd(scene).clone()
    assert not sd.stale()
    with torch.no_grad():
        for i in range(len(m.model[-1].m)):
            m.model[-1].m[i].bias.data[4::m.model[-1].no] -= 1.0             # every anchor's objectness: other confidences, other boxes kept
    pack.touch_weights()
    assert sd.stale()
    sd.refresh()
    assert not sd.stale()
    after = sd(scene)
    assert after.shape != before.shape or not torch.equal(after, before)
    example = torch.full((BS, 3, TILE, TILE), 114, dtype=torch.uint8, device=_dev())
    g = L.GraphedForward(m, example if getattr(m, "u8_input", False) else example.float() / 255)  # graph against graph, both captured with the new weights
    want = _hand_scene(*_hand_tiles(m, lambda x: g(x)[0], scene), SH, SW)[0]
    assert np.array_equal(after.cpu().numpy(), want)
