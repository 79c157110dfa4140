"""RFCBAMConv forward routes, the host side (no GPU): rfcbam.select's table of four, the weight images RFCBAMConv._packed / _packed_train
build for the routes a module could take, and ops.rf_out_hw."""
import itertools

import pytest
import torch

import lead_yolo_amd as L
from lead_yolo_amd import modules as M, ops, pack, rfcbam

F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(autouse=True)
def _shipped_switches(monkeypatch):
    for mod, name, value in ((M, "RF3M", True), (M, "RF3C", True), (ops, "RF3M_MIN_UNITS", 1500), (ops, "CONCURRENT_PARTS", 1)):
        monkeypatch.setattr(mod, name, value)


@pytest.mark.parametrize("n,c,o,hw,route,tile,units", [(30, 128, 128, 40, "rf3m", (8, 4), 1500), (29, 128, 128, 40, "rf3c", (8, 8), 1450),
                                                       (32, 256, 256, 20, "rf3c", (3, 20), 896), (64, 256, 256, 20, "rf3m", (10, 3), 1792)])
def test_matrix_core_route_from_1500_units(n, c, o, hw, route, tile, units):
    r = rfcbam.select(False, BF16, 3, 2, c, o, n, hw, hw)
    assert (r.name, (r.th, r.tw), r.could) == (route, tile, (route,))
    assert ops.rf3m_units(n, hw, hw, o, 2) == units
    assert (r.th, r.tw) == {"rf3m": ops.pick_tile_m, "rf3c": ops.pick_tile_c}[route](hw, hw, 2)


def test_switches_are_read_at_call_time(monkeypatch):
    assert rfcbam.select(False, BF16, 3, 2, 128, 128, 30, 40, 40).name == "rf3m"
    monkeypatch.setattr(M, "RF3M", False)
    assert rfcbam.select(False, BF16, 3, 2, 128, 128, 30, 40, 40).name == "rf3c"
    monkeypatch.setattr(M, "RF3M", True)
    assert rfcbam.select(False, BF16, 3, 2, 128, 128, 15, 40, 40).name == "rf3c"
    monkeypatch.setattr(ops, "CONCURRENT_PARTS", 2)             # a sub-batched replay of 30 images
    assert rfcbam.select(False, BF16, 3, 2, 128, 128, 15, 40, 40).name == "rf3m"
    monkeypatch.setattr(ops, "CONCURRENT_PARTS", 1)
    monkeypatch.setattr(ops, "RF3M_MIN_UNITS", 0)
    assert rfcbam.select(False, BF16, 3, 2, 32, 64, 2, 5, 5).name == "rf3m"


def test_fp32_wide_exception_is_eval_only():
    assert rfcbam.select(False, F32, 3, 2, 256, 256).name == "rf3"
    assert rfcbam.select(False, F32, 3, 2, 256, 256, 2, 20, 20).name == "rf3"
    assert rfcbam.select(False, F32, 3, 2, 128, 128).name == "rf3c"
    assert rfcbam.select(False, F32, 3, 1, 32, 192, 1, 6, 6).name == "rf3"
    for dt in (F32, BF16):
        assert rfcbam.select(True, dt, 3, 2, 256, 256).name == "rf3c"
        assert rfcbam.select(True, dt, 3, 2, 256, 256, 2, 20, 20).name == "rf3c"


def test_training_never_takes_the_matrix_core_route():
    r = rfcbam.select(True, BF16, 3, 2, 128, 128, 64, 40, 40)
    assert (r.name, (r.th, r.tw)) == ("rf3c", ops.pick_tile_c(40, 40, 2))
    assert rfcbam.select(False, BF16, 3, 2, 128, 128, 64, 40, 40).name == "rf3m"


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_lane_pixel_and_k1_rules(training, dtype, monkeypatch):
    for s, o in itertools.product((1, 2, 3), (48, 64, 128, 256)):
        for c in (16, 48):                                     # no multiple of 32
            assert rfcbam.select(training, dtype, 3, s, c, o).name == "rf3"
            assert rfcbam.select(training, dtype, 3, s, c, o, 4, 9, 11) == rfcbam.Route("rf3", *ops.pick_tile(9, 11), ("rf3",))
        assert rfcbam.select(training, dtype, 3, 3, 32, o).name == "rf3"        # stride 3
        assert rfcbam.select(training, dtype, 1, 1, 32, o, 4, 9, 11) == rfcbam.Route("k1", None, None, ("k1",))
    monkeypatch.setattr(M, "RF3C", False)
    for s, c, o in itertools.product((1, 2, 3), (32, 64, 256), (48, 64, 256)):
        for size in ((), (64, 40, 40)):
            r = rfcbam.select(training, dtype, 3, s, c, o, *size)
            assert r.name in ("rf3", "rf3m") and (r.name == "rf3m") == (not training and dtype == BF16 and o % 64 == 0 and s < 3)


def test_unsized_answer_covers_every_sized_answer(monkeypatch):
    sizes = [(1, 1, 1), (2, 5, 7), (29, 40, 40), (30, 40, 40), (64, 20, 20), (256, 80, 80)]
    for rf3m, rf3c in itertools.product((True, False), repeat=2):
        monkeypatch.setattr(M, "RF3M", rf3m)
        monkeypatch.setattr(M, "RF3C", rf3c)
        for training, dtype, (k, s), c, o in itertools.product((False, True), (F32, BF16), ((1, 1), (3, 1), (3, 2), (3, 3)), (16, 32, 48, 128),
                                                               (48, 64, 128, 192, 256)):
            could = rfcbam.select(training, dtype, k, s, c, o).could
            for n, ho, wo in sizes:
                r = rfcbam.select(training, dtype, k, s, c, o, n, ho, wo)
                assert r.name in could and r.could == (r.name,), (training, dtype, k, s, c, o, n, ho, wo, r, could)


@pytest.mark.parametrize("scale", ["n", "s", "l"])
def test_packed_keys_of_the_model(scale, monkeypatch):
    """the images every RFCBAMConv of cfg/LEAD-YOLO.yaml packs, against the rules written out before there was a selector: lane = channel
    images wherever C % 32 == 0 at stride 1 / 2 (eval: whatever the dtype and width; training: in place of the lane = pixel image), the
    matrix-core streams for bf16 (one operand plane) where also O % 64 == 0"""
    monkeypatch.setattr(pack, "packed", lambda *a, **kw: None)              # (the operand images themselves are built on the device)
    monkeypatch.setattr(pack, "rf3m_stream", lambda *a, **kw: None)
    mods = [m for m in L.Model(L.load_cfg(scale=scale)).modules() if isinstance(m, L.RFCBAMConv)]
    assert mods
    for m, planes in itertools.product(mods, (1, 2)):
        k, s, c, o = m.kernel_size, m.stride, m.c, m.o
        lane_c = c % 32 == 0 and s in (1, 2)
        if k == 1:
            want, want_train = {"a1", "b1", "w18", "wp", "es", "eb"}, {"w18", "wp"}
        else:
            want = {"wq_stats", "wq_main", "w18", "wp", "es", "eb"} | ({"wq_c", "wp_c"} if lane_c else set())
            want |= {"wm_stats", "wm"} if planes == 1 and lane_c and o % 64 == 0 else set()
            want_train = {"w18", "wp_c"} if lane_c else {"w18", "wp"}
        assert set(m._packed(planes)) == want, (k, s, c, o, planes)
        assert set(m._packed_train(planes)) == want_train, (k, s, c, o, planes)


def test_rf_out_hw_is_conv2d_output_shape():
    for k, s, h, w in itertools.product((1, 3), (1, 2, 3), range(1, 10), range(1, 10)):
        y = torch.nn.functional.conv2d(torch.zeros(1, 1, h, w), torch.zeros(1, 1, k, k), stride=s, padding=k // 2)
        assert ops.rf_out_hw(h, w, k, s) == tuple(y.shape[2:]), (k, s, h, w)
