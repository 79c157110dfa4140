"""Host side of the RFCBAMConv backward tests (tests/rfcbam_ref.py): the stage references composed in the order of the two routes against
float64 autograd through the reference module, the judges against planted defects (the evidence that tests/test_gpu_rfcbam_bwd.py would
fail on a subtly wrong kernel — no broken kernel is ever built or run), the measured constants, the premises of every device case (no
element in the ReLU band, no undecided maximum, no undecided SE unit, the planted all-negative positions really there) and the launch
arithmetic that each case id claims.  Every mutant is computed in float64 and rounded as a kernel's result would be stored.  No GPU."""
import pytest
import torch

from tests import rfcbam_ref as R

DT = {R.F32: "f32", R.BF16: "bf16"}
BOTH = [pytest.param(R.F32, id="f32"), pytest.param(R.BF16, id="bf16")]


def _rejects(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


# ---------------------------------------------------------------- the references against autograd -------------------------------------------
@pytest.mark.parametrize("n,h,w,c,o,k,s,route", [(2, 5, 4, 6, 5, 1, 1, "k1"), (2, 5, 4, 6, 5, 1, 1, "streamed"), (2, 6, 5, 4, 5, 3, 1, "streamed"),
                                                 (2, 7, 5, 4, 6, 3, 2, "streamed")], ids=["k1", "k1-streamed", "k3s1", "k3s2-odd"])
def test_stage_references_equal_float64_autograd(n, h, w, c, o, k, s, route):
    """the stage references, composed as grad._rfcbam_backward_streamed / _k1 compose the kernels, reproduce float64 autograd through
    oracle.functional.rfcbam(training=True): the input gradient and every parameter gradient to 1e-10; conv.0.bias: zero up to rounding"""
    g = torch.Generator().manual_seed(5)
    p = R.chain_params(g, c, o, k, 3)
    x = torch.randn(n, h, w, c, generator=g, dtype=torch.float64)
    r = torch.randn(n, *R.out_hw(h, w, k, s), o, generator=g, dtype=torch.float64)
    au, pa = R.chain_autograd(x, p, r, k, s), R.chain_parts(x, p, r, k, s, route)
    for key in R.GRADS + ("y",):
        if key != "conv_b":
            assert float((pa[key] - au[key]).abs().max()) <= 1e-10 * float(au[key].abs().max()), key
    assert max(float(au["conv_b"].abs().max()), float(pa["conv_b"].abs().max())) <= 1e-12 * float(au["out_beta"].abs().max())


# ---------------------------------------------------------------- measured constants ---------------------------------------------------------
def test_measured_k_holds():
    """every K of tests/rfcbam_ref.py is at least four times what the reference itself shows in float32 over every case of the tables, at most 64"""
    for key, v in R.measure_k().items():
        assert 4 * v <= R.K[key] <= 64, (key, v)


# ---------------------------------------------------------------- builders: premises ---------------------------------------------------------
def _check_stage(x, what, dt):
    """no element in a band; gmax == 0 at the planted positions and only there; the rounded reference passes the attention and ReLU judges"""
    u = R.d(x["ug"])
    R.assert_premises(u, x["aeff"], R.d(x["bg"]), what)
    a = R._stage_args(x, R.ATTN_KEYS)
    want = R.attn(*a)
    n, ho, wo, k = x["n"], x["ho"], x["wo"], x["k"]
    zero = R.from_map(want["gmax"], n, ho, wo, k) == 0
    planted = torch.zeros_like(zero)
    for m, t in R.allneg_positions(n * ho * wo, k * k):
        planted[m, t] = True
    assert torch.equal(zero, planted), what
    assert float(R.from_map(want["d_rfa"], n, ho, wo, k)[planted].abs().max()) == 0.0
    rl = R.relu(*R._stage_args(x, R.RELU_KEYS))
    assert float(rl["dv"][planted].abs().max()) == 0.0 and float(rl["dv"][..., -1].abs().max()) == 0.0
    assert torch.equal(R.d(x["gmax"]), want["gmax"].float().double()), what          # the fp32 G of the leader is the reference's, rounded
    ch = (8.0, 8.0, 8.0)
    R.judge_attn(dict(cd=want["cd"].to(dt), d_rfa=want["d_rfa"].float(), gmax=want["gmax"].float(), d_ca=want["d_ca"].float()), x, ch, what)
    R.judge_relu(dict(dv=rl["dv"].to(dt), s1=rl["s1"].float(), s2=rl["s2"].float()), x, 8.0, what)
    return want


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("cid", list(R.TC_CASES))
def test_thread_channel_cases_hold_their_premises(cid, dtype):
    x = R.tc_inputs(cid, dtype)
    want = _check_stage(x, cid, dtype)
    c, kk = x["ug"].shape[-1], x["k"] ** 2
    if c >= 128:
        # the -0.0 case: a whole wave of channels gives fma(a, +0, -0.0) = -0.0 at tap KK / 2, and the reference's gmax there is positive
        zt = kk // 2
        assert bool((x["ag"][zt, 64:128] < 0).all()) and bool(torch.signbit(x["bg"][zt, 64:128]).all()) and float(x["ug"][:, zt, 64:128].abs().max()) == 0.0
        v = torch.addcmul(x["bg"][zt, 64:128], x["ag"][zt, 64:128], x["ug"][:, zt, 64:128].float())
        assert bool(torch.signbit(v).all()) and float(v.abs().max()) == 0.0
        assert float(R.from_map(want["gmax"], x["n"], x["ho"], x["wo"], x["k"])[:, zt].min()) > 0.0
    a = (R.d(x["x"]), R.d(x["wg"]), x["k"], x["s"])
    R.judge_generate(R.generate(*a).to(dtype), x, cid)
    gn = R.gen(R.taps(a[0], x["k"], x["s"]), *[R.d(x[q]) for q in ("ug", "dv", "alpha", "kappa", "lam")])
    R.judge_gen(dict(dug=gn["dug"].to(dtype), dwg=gn["dwg"].float()), x, 8.0, cid)
    R.judge_dx(R.dx(R.d(x["dug"]), a[1], x["n"], x["h"], x["w"], x["k"], x["s"], R.d(x["addnc"]), x["add_scale"]).to(dtype), x, cid)


@pytest.mark.parametrize("dtype", BOTH)
def test_rf3s_and_rf1_cases_hold_their_premises(dtype):
    for cid, (cf, cb, ho, wo, n) in R.RF3S_CASES.items():
        _check_stage(R.stage_inputs("rf3s", n, ho, wo, R.c_of((cf, cb), dtype), 3, dtype), cid, dtype)
    for cid, (cf, cb, hw, n) in R.RF1_CASES.items():
        x = R.rf1_inputs(n, hw, R.c_of((cf, cb), dtype), dtype)
        R.assert_premises(R.d(x["x"]), x["aeff"], R.d(x["bg"]), cid)
        a = [R.d(x[q]) for q in R.RF1_KEYS] + [n, hw]
        want = R.rf1_a(*a)
        planted = torch.zeros(n * hw, dtype=torch.bool)
        planted[[m for m, _ in R.allneg_positions(n * hw, 1)]] = True
        assert torch.equal(want["gmax"] == 0, planted), cid
        R.judge_rf1_a(dict(cd=want["cd"].to(dtype), d_rfa=want["d_rfa"].float(), gmax=want["gmax"].float(), d_ca=want["d_ca"].float()), x, cid)
        rb = R.rf1_b(*a[:7], R.d(x["d_mm"]), n, hw)
        R.judge_rf1_b(dict(s1=rb["s1"].float(), s2=rb["s2"].float()), x, cid)
        rc = R.rf1_c(*a[:7], *[R.d(x[q]) for q in ("d_mm", "alpha", "kappa", "lam", "dgap")], x["scale"], n, hw)
        R.judge_rf1_c(dict(dx=rc["dx"].to(dtype), dgw=rc["dgw"].float() + 0.5), x, cid, False, prefill=0.5)


def test_rfa_and_se_cases_hold_their_premises():
    for cid in R.RFA_CASES:
        x = R.rfa_inputs(cid)
        want = R.getw_bwd(*[R.d(x[q]) for q in ("d_rfa", "rfa", "mm", "w18")])
        R.judge_getw(dict(d_mm=want["d_mm"].float(), dw18=want["dw18"].float() + 0.5), x, False, cid, prefill=0.5)
        assert x["rfa"].numel() == 1 or (float(x["rfa"].max()) == 1.0 and float(x["rfa"].min()) < 1e-8)          # saturated sigmoids
    for cid, (n, c, r, slices) in R.SE_CASES.items():
        x = R.se_inputs(cid)
        assert not bool(R.se_margin_short(R.d(x["part"]), R.d(x["wa"]), x["hw"]).any()), cid
        want = R.se_bwd(*[R.d(x[q]) for q in R.SE_KEYS], x["hw"])
        assert bool((want["pre"][:, x["off"]] < 0).all()) and (r < 4 or bool(x["off"].any())) and bool((want["pre"] > 0).any()), cid
        R.judge_se(dict(dgap=want["dgap"].float(), dWa=want["dWa"].float() + 0.5, dWb=want["dWb"].float() + 0.5), x, cid, prefill=0.5)


def test_builders_move_planted_band_elements_out():
    """an element planted on the ReLU kink and a position with two equal maxima are moved, and nothing is left in a band"""
    a, b = torch.tensor([[1.0, 1.0, 1.0]]).double(), torch.tensor([[-1.0, 0.5, 0.25]]).double()
    u = torch.tensor([[[1.0, 2.0, 2.25]], [[3.0, 0.5, 0.1]]])
    assert int(R.in_band(u.double(), a.expand_as(u), b.expand_as(u)).sum()) == 1 and int(R.max_margin_short(u.double(), a, b).sum()) == 1
    u, k1 = R.nudge(u, a.expand_as(u), b.expand_as(u), R.F32)
    u, k2 = R.raise_leader(u, a, b, R.F32)
    assert k1 == 1 and k2 == 1
    R.assert_premises(u.double(), a, b, "moved")


# ---------------------------------------------------------------- seeded defects -------------------------------------------------------------
def test_relu_judge_rejects_sums_from_rounded_dv_missing_guard_and_dropped_mean():
    """relu: sums from the bf16-rounded dv; d_max routed without the G > 0 guard; d_mean / C dropped"""
    cid = "subs4-odd-parity-straddle-c64"
    x = R.tc_inputs(cid, R.BF16)
    a = R._stage_args(x, R.RELU_KEYS)
    ch = R.attn_chains("tc", x["n"], x["ho"], x["wo"], 64, 3, R.BF16, x["h"], x["w"], x["s"])[2]
    st = lambda o: dict(dv=o["dv"].to(R.BF16), s1=o["s1"].float(), s2=o["s2"].float())
    R.judge_relu(st(R.relu(*a)), x, ch, cid)
    bad = st(R.relu(*a, sums_dtype=R.BF16))
    _rejects(R.judge_relu, bad, x, ch, "sums from the rounded dv", keys=("s1",))
    _rejects(R.judge_relu, bad, x, ch, "sums from the rounded dv", keys=("s2",))
    for dt in (R.F32, R.BF16):
        x = R.tc_inputs(cid, dt)
        a = R._stage_args(x, R.RELU_KEYS)
        st = lambda o: dict(dv=o["dv"].to(dt), s1=o["s1"].float(), s2=o["s2"].float())
        for key in ("dv", "s1", "s2"):
            _rejects(R.judge_relu, st(R.relu(*a, no_guard=True)), x, ch, "no G > 0 guard", keys=(key,))
        _rejects(R.judge_relu, st(R.relu(*a, no_mean=True)), x, ch, "d_mean / C dropped", keys=("s1",))
        if dt == R.F32:
            _rejects(R.judge_relu, st(R.relu(*a, no_mean=True)), x, ch, "d_mean / C dropped", keys=("dv",))


@pytest.mark.parametrize("dtype", BOTH)
def test_attn_judge_rejects_swapped_tap_position(dtype):
    """attn: rf_pos with tx and ty exchanged, on a case with Ho != Wo"""
    cid = "subs4-odd-parity-straddle-c64"
    x = R.tc_inputs(cid, dtype)
    a = R._stage_args(x, R.ATTN_KEYS)
    ch = R.attn_chains("tc", x["n"], x["ho"], x["wo"], 64, 3, dtype, x["h"], x["w"], x["s"])
    st = lambda o: dict(cd=o["cd"].to(dtype), d_rfa=o["d_rfa"].float(), gmax=o["gmax"].float(), d_ca=o["d_ca"].float())
    R.judge_attn(st(R.attn(*a)), x, ch, cid)
    for key in ("cd", "d_rfa", "gmax", "d_ca"):
        _rejects(R.judge_attn, st(R.attn(*a, swap_pos=True)), x, ch, "tx / ty swapped", keys=(key,))


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("cid", list(R.TC_CASES))
def test_generate_judge_rejects_clamped_border(cid, dtype):
    """generate: the border clamped instead of zero padded (k = 3 cases; k = 1 has no border)"""
    x = R.tc_inputs(cid, dtype)
    a = (R.d(x["x"]), R.d(x["wg"]), x["k"], x["s"])
    R.judge_generate(R.generate(*a).to(dtype), x, cid)
    if x["k"] == 3:
        _rejects(R.judge_generate, R.generate(*a, clamp=True).to(dtype), x, cid + " clamped")


@pytest.mark.parametrize("dtype", BOTH)
def test_dx_judge_rejects_neighbouring_addend_and_dropped_halo(dtype):
    """dx: on the case whose chunk straddles two images, the second image's pixels of that chunk take the first image's addend; on the tiled
    cases the tile's halo row / column is dropped"""
    cid = "subs4-odd-parity-straddle-c64"
    x = R.tc_inputs(cid, dtype)
    g = R.dx_geom(*R.TC_CASES[cid], dtype)
    a = (R.d(x["dug"]), R.d(x["wg"]), x["n"], x["h"], x["w"], x["k"], x["s"], R.d(x["addnc"]), x["add_scale"])
    R.judge_dx(R.dx(*a).to(dtype), x, cid)
    bad = R.dx(*a, next_image_chunk=g["chunk"])
    assert 0 < int((bad != R.dx(*a)).any(-1).sum()) < g["chunk"]
    _rejects(R.judge_dx, bad.to(dtype), x, cid + " neighbouring addend")
    cid = "cb128-clamped-s2t-partial-c72"
    x = R.tc_inputs(cid, dtype)
    g = R.dx_geom(*R.TC_CASES[cid], dtype)
    a = (R.d(x["dug"]), R.d(x["wg"]), x["n"], x["h"], x["w"], x["k"], x["s"], R.d(x["addnc"]), x["add_scale"])
    R.judge_dx(R.dx(*a).to(dtype), x, cid)
    _rejects(R.judge_dx, R.dx(*a, drop_halo=g["tm"]).to(dtype), x, cid + " halo dropped")


def test_getw_judge_rejects_unflipped_conv():
    for cid in ("halo-four-tiles-17x65", "wide-3x200"):
        x = R.rfa_inputs(cid)
        bad = R.getw_bwd(*[R.d(x[q]) for q in ("d_rfa", "rfa", "mm", "w18")], no_flip=True)
        _rejects(R.judge_getw, dict(d_mm=bad["d_mm"].float(), dw18=bad["dw18"].float()), x, False, cid + " not flipped", keys=("d_mm",))
    want = R.getw_bwd(*[R.d(x[q]) for q in ("d_rfa", "rfa", "mm", "w18")])
    _rejects(R.judge_getw, dict(dw18=want["dw18"].float()), x, False, "stored, not added", prefill=0.5, keys=("dw18",))


@pytest.mark.parametrize("dtype", BOTH)
def test_rf1_c_judge_rejects_unscaled_dgap(dtype):
    cid = "c24-24-hw37-n1"
    cf, cb, hw, n = R.RF1_CASES[cid]
    x = R.rf1_inputs(n, hw, R.c_of((cf, cb), dtype), dtype)
    a = [R.d(x[q]) for q in R.RF1_KEYS + ("d_mm", "alpha", "kappa", "lam", "dgap")] + [x["scale"], n, hw]
    bad = R.rf1_c(*a, no_scale=True)
    _rejects(R.judge_rf1_c, dict(dx=bad["dx"].to(dtype), dgw=bad["dgw"].float()), x, cid + " dgap not scaled", False, keys=("dx",))
    want = R.rf1_c(*a)
    _rejects(R.judge_rf1_c, dict(dx=want["dx"].to(dtype), dgw=want["dgw"].float()), x, cid + " stored, not added", False, prefill=0.5, keys=("dgw",))
    b = [R.d(x[q]) for q in R.RF1_KEYS + ("d_mm",)] + [n, hw]
    for sw in (dict(no_guard=True), dict(no_mean=True)):
        o = R.rf1_b(*b, **sw)
        _rejects(R.judge_rf1_b, dict(s1=o["s1"].float(), s2=o["s2"].float()), x, f"{cid} {sw}")


def test_se_judge_rejects_unmasked_dh():
    for cid in ("n3-c160-r10-nq40", "n9-c256-r16-trip-plus-one"):
        x = R.se_inputs(cid)
        bad = R.se_bwd(*[R.d(x[q]) for q in R.SE_KEYS], x["hw"], no_mask=True)
        for key in ("dgap", "dWa"):
            _rejects(R.judge_se, {key: bad[key].float()}, x, cid + " dh without the mask", keys=(key,))


# ---------------------------------------------------------------- geometry: each id takes the branch it names --------------------------------
@pytest.mark.parametrize("cid", list(R.TC_CASES))
def test_thread_channel_geometry(cid):
    n, h, w, c, k, s = R.TC_CASES[cid]
    g, claim = R.rf_geom(n, h, w, c, k, s), R.TC_CLAIMS[cid]
    for key in ("chunk", "gx", "subs", "cb", "gy", "clamped", "threads"):
        assert g[key] == claim[key], (cid, key, g[key])
    for dt in (R.F32, R.BF16):
        gd = R.dx_geom(n, h, w, c, k, s, dt)
        for key in ("form", "gather", "tiles_x", "cgroups"):
            if key in claim:
                assert gd[key] == claim[key], (cid, key, gd.get(key))
        assert R.dx_geom(n, h, w, c, k, s, dt, addend=False)["form"] in (0, "s2t")
    gd = R.dx_geom(n, h, w, c, k, s, R.F32)
    if cid == "subs4-odd-parity-straddle-c64":
        assert (h % 2, w % 2) == (1, 1) and gd["chunk"] <= h * w
        assert any((b * gd["chunk"]) // (h * w) != (min((b + 1) * gd["chunk"], n * h * w) - 1) // (h * w) for b in range(gd["gx"])), "no chunk straddles"
    if cid == "chunk-over-image-add1-c8":
        assert gd["chunk"] > h * w and R.out_hw(h, w, k, s) == (2, 2)
    if cid == "cb128-clamped-s2t-partial-c72":
        assert c % 64 != 0 and (w // 2) % gd["tm"] != 0
    if cid == "gy2-clamped-s2t-c320":
        assert c // 4 > 64 >= c // 8                                   # fp32: past ly_rf3s_bwd's 64 lanes per pixel, the route falls back
    for rows in (4, 512):
        gg = R.gen_geom(n, h, w, c, k, s, rows)
        assert gg["gx"] * gg["subs"] <= rows


def test_rf3s_rf1_rfa_se_geometry():
    for cid, (cf, cb, ho, wo, n) in R.RF3S_CASES.items():
        for i, dt in enumerate((R.F32, R.BF16)):
            g = R.rf3s_geom(n, ho * wo, R.c_of((cf, cb), dt), dt)
            assert (g["lpp2"], g["pp"], g["threads"]) == R.RF3S_CLAIMS[cf][i], (cid, dt, g)
            assert g["threads"] <= 576 and g["grid"][0] * g["chunk"] >= ho * wo
    assert R.rf3s_geom(1, 15, 24, R.F32)["lpp"] == 6 and R.rf3s_geom(1, 15, 24, R.BF16)["lpp"] == 3        # rounded up to 8 / 4: idle lanes
    assert any(R.rf3s_geom(n, ho * wo, cf, R.F32)["grid"][0] > 1 for cf, cb, ho, wo, n in R.RF3S_CASES.values())
    for cid, (cf, cb, hw, n) in R.RF1_CASES.items():
        for dt in (R.F32, R.BF16):
            c = R.c_of((cf, cb), dt)
            g = R.rf1_geom(n, hw, c, dt)
            assert g["lpp2"] >= g["lpp"] and g["pb"] * g["lpp2"] == 256 and g["grid"][0] * g["chunk"] >= hw and g["chunk"] % g["pb"] == 0
    g = R.rf1_geom(1, 1031, 4, R.F32)
    assert g["pb"] == 256 and g["grid"][0] == 2 and 0 < (1031 - g["chunk"]) % (2 * g["pb"]) - g["pb"] < g["pb"]   # a trip whose second pixel is live on 7 slots only
    assert R.rf1_geom(3, 1031, 64, R.F32)["grid"] == (17, 3)
    claims = {"one-position": (1, 1), "inside-one-tile-15x63": (2, 2), "exact-tile-16x64": (1, 1), "halo-four-tiles-17x65": (8, 8), "wide-3x200": (4, 4),
              "block-cap-513-tiles": (513, 512)}
    for cid, v in R.RFA_CASES.items():
        g = R.rfa_geom(*v)
        assert (g["tiles"], g["blocks"]) == claims[cid], (cid, g)
    claims = {"n1-c8-r1": (2, 128, 0, 1), "n3-c160-r10-nq40": (40, 6, 0, 3), "n8-c64-r4-one-trip": (16, 16, 1, 0), "n9-c256-r16-trip-plus-one": (64, 4, 1, 1),
              "n17-c1024-r64-two-trips-plus-one": (256, 1, 2, 1)}
    for cid, v in R.SE_CASES.items():
        g = R.se_chains(*v)
        assert (g["nq"], g["ng"], g["trips"], g["tail"]) == claims[cid], (cid, g)
    assert 256 % 40 != 0
