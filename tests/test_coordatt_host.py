"""Host side of the CoordAtt chain tests (tests/coordatt_ref.py): the float64 references against autograd, the judges against planted defects
(the evidence that tests/test_gpu_coordatt.py would fail on a subtly wrong kernel — no broken kernel is ever built or run), the measured
constants, and the premises of every device case (no element in the h_swish kink band, all three h_swish regimes populated, saturated
sigmoids).  Every mutant is computed in float64 and rounded to fp32, as a kernel's result would be stored.  No GPU."""
import pytest
import torch

from tests import coordatt_ref as R

DT = {R.F32: "f32", R.BF16: "bf16"}


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp(min=1e-300))


def _rejects(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


# ---------------------------------------------------------------- the references against autograd -------------------------------------------
@pytest.mark.parametrize("n,h,w,c,mip", [(2, 5, 7, 24, 8), (3, 4, 4, 40, 16), (1, 1, 9, 8, 8)])
def test_mlp_bwd_equals_float64_autograd(n, h, w, c, mip):
    """mlp_bwd's formulas (the comment above ly_coordatt_mlp_bwd1_kernel) are float64 autograd of mlp() through bn1's batch statistics; the
    gradient of conv1.bias is zero up to rounding"""
    x = R.mlp_bwd_inputs(f"host-{n}-{h}-{w}-{c}-{mip}", n, h, w, c, mip)
    w64 = {k: v.double() for k, v in x.items() if torch.is_tensor(v)}
    au = R.mlp_bwd_autograd(w64["pool"], w64["w1"], w64["b1"], w64["gamma"], w64["beta"], w64["wh"], w64["bh"], w64["ww"], w64["bw"], h,
                            w64["da_h"], w64["da_w"], R.EPS)
    got = R.mlp_bwd(w64["pool"], w64["w1"], w64["b1"], au["mean"], au["invstd"], w64["gamma"], w64["beta"], w64["wh"], w64["ww"], au["a_h"], au["a_w"],
                    w64["da_h"], w64["da_w"])
    for k in ("dpool",) + R.BWD_SUMS:
        assert _rel(got[k], au[k]) <= 1e-11, k
    assert float(au["db1"].abs().max()) <= 1e-12 * float(au["dbeta"].abs().max())


@pytest.mark.parametrize("case", R.CHAIN_CASES, ids=lambda v: "c%d-r%d-%dx%dx%d" % v)
def test_chain_autograd_equals_its_parts(case):
    """the reference module under float64 autograd equals pool -> conv1_stats -> mlp -> gate and gate_bwd -> mlp_bwd -> pool_bwd composed;
    running statistics as nn.BatchNorm2d updates them (momentum 0.03, unbiased variance)"""
    c, red, n, h, w = case
    ci = R.chain_inputs(c, red, n, h, w, R.F32)
    au = R.chain_autograd(R.d(ci["x"]), ci["params"], R.d(ci["r"]), rm=ci["rm"], rv=ci["rv"])
    pa = R.chain_parts(R.d(ci["x"]), ci["params"], R.d(ci["r"]), rm=ci["rm"], rv=ci["rv"])
    for k in R.CHAIN_KEYS + ("rm", "rv"):
        assert _rel(pa[k], au[k]) <= 1e-11, k
    assert float(au["db1"].abs().max()) <= 1e-12 * float(au["dbeta"].abs().max()) and float(pa["db1"].abs().max()) == 0.0


# ---------------------------------------------------------------- measured constants ---------------------------------------------------------
def test_measured_k_and_chain_tolerance_hold():
    """every K of tests/coordatt_ref.py is at least four times what the reference itself shows when evaluated in float32 over every case of
    the tables, and no more than 64; CHAIN_TOL likewise and at most 1e-4"""
    k = R.measure_k()
    for key, v in k.items():
        assert 4 * v <= R.K[key] <= 64, (key, v)
    t = R.measure_chain_tol()
    assert max(t.values()) * 4 <= R.CHAIN_TOL <= 1e-4, t


# ---------------------------------------------------------------- the judges: rounded reference accepted, mutants rejected -------------------
def test_pool_judge_accepts_rounded_on_every_case():
    for cid in R.POOL_CASES:
        for dt in (R.F32, R.BF16):
            x = R.d(R.pool_inputs(cid, dt))
            R.judge_pool(R.pool(x).float(), x, cid)
            assert float(x[..., -1].abs().max()) == 0.0 and float(x.abs().max()) <= 30.0


def test_pool_judge_rejects_exchanged_divisors_on_a_nearly_square_map():
    """(20, 21): 1 / W where 1 / H belongs is 5 % off — inside 1e-3 + 1e-3 |want| for none of the means, and far outside the sums' bound"""
    g = torch.Generator().manual_seed(3)
    x = R.make_x(g, 2, 20, 21, 24, R.F32).double()
    R.judge_pool(R.pool(x).float(), x, "rounded")
    _rejects(R.judge_pool, R.pool(x, swap_div=True).float(), x, "divisors exchanged")


@pytest.mark.parametrize("cid", list(R.STATS_CASES))
def test_stats_judge_accepts_rounded_rejects_dropped_last_position(cid):
    x = R.stats_inputs(cid)
    a = [x[k].double() for k in ("pool", "w1", "b1")]
    s1, s2 = R.conv1_stats(*a)
    R.judge_stats(s1.float(), s2.float(), x, cid)
    if R.STATS_CASES[cid][0] > 1:
        b1, b2 = R.conv1_stats(*a, drop_last=True)
        _rejects(R.judge_stats, b1.float(), s2.float(), x, cid)
        _rejects(R.judge_stats, s1.float(), b2.float(), x, cid)


@pytest.mark.parametrize("train", [True, False], ids=["train", "folded"])
@pytest.mark.parametrize("cid", list(R.MLP_CASES))
def test_mlp_judge_accepts_rounded_and_inputs_hold_their_premises(cid, train):
    """the rounded reference passes; y1 populates all three h_swish regimes; sigmoid arguments reach +-20; position 0 of the pool is zero"""
    n, h, w, c, mip = R.MLP_CASES[cid]
    x = R.mlp_inputs(cid, n, h, w, c, mip, train)
    a = [None if x[k] is None else x[k].double() for k in R.MLP_KEYS]
    a_h, a_w = R.mlp(x["pool"].double(), h, *a)
    R.judge_mlp(a_h.float(), a_w.float(), x, h, cid)
    lo, mid, hi = R.regimes(R._y1(x["pool"].double(), *a[:4]))
    assert lo > 0 and mid > 0 and hi > 0, (cid, lo, mid, hi)
    both = torch.cat((a_h, a_w), 1)
    assert float(both.min()) < 1e-7 and float(both.max()) > 1 - 1e-7, cid              # sigmoid(-+ 16) and beyond
    assert float(x["pool"][0, 0].abs().max()) == 0.0


def test_mlp_judge_rejects_exchanged_heads_on_a_square_map():
    """conv_h / conv_w exchanged at H = W (every shape still fits)"""
    n, h, w, c, mip = 2, 6, 6, 168, 8
    x = R.mlp_inputs("host-square", n, h, w, c, mip, True)
    a = [x[k].double() for k in R.MLP_KEYS]
    bad = R.mlp(x["pool"].double(), h, *a, swap_hw=True)
    _rejects(R.judge_mlp, bad[0].float(), bad[1].float(), x, h, "heads exchanged")


@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=DT.values())
def test_gate_judge_accepts_rounded_rejects_gate_without_a_w(dtype):
    for cid, v in R.GATE_CASES.items():
        x = R.gate_inputs(cid, dtype, v[5] is not None)
        a = [None if x[k] is None else R.d(x[k]) for k in ("x", "a_h", "a_w", "res")]
        R.judge_gate(R.gate(*a).to(dtype), x, cid)
        _rejects(R.judge_gate, R.gate(*a, no_aw=True).to(dtype), x, cid + " without a_w")


@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=DT.values())
def test_gate_bwd_judge_accepts_rounded_rejects_missing_row_band(dtype):
    """da_w summed over the first 16 of 17 rows (the last band of 8 rows holds one row) is rejected"""
    for cid, (n, h, w, c, _) in R.GATE_BWD_CASES.items():
        x = R.gate_bwd_inputs(cid, dtype)
        a = [R.d(x[k]) for k in ("dout", "x", "a_h", "a_w")]
        dx, da_h, da_w = R.gate_bwd(*a)
        R.judge_gate_bwd(dx.to(dtype), da_h.float(), da_w.float(), x, cid)
        if h > 8:
            bad = R.gate_bwd(*a, da_w_rows=8 * ((h - 1) // 8))[2]
            _rejects(R.judge_gate_bwd, dx.to(dtype), da_h.float(), bad.float(), x, cid + " last band missing")


@pytest.mark.parametrize("cid", list(R.MLP_BWD_CASES))
def test_mlp_bwd_judge_accepts_rounded_and_inputs_hold_their_premises(cid):
    """the rounded reference passes (fp32 and float64 targets, with a prefill); NO element of y1 is in the kink band; the three h_swish regimes
    are populated"""
    n, h, w, c, mip = R.MLP_BWD_CASES[cid]
    x = R.mlp_bwd_inputs(cid, n, h, w, c, mip)
    want, mag = R.mlp_bwd(*R.bwd_args(x)), R.mlp_bwd_mag(*R.bwd_args(x))
    R.assert_no_kink(want["y1"], mag["y1"], cid)
    lo, mid, hi = R.regimes(want["y1"])
    assert lo > 0 and mid > 0 and hi > 0, (cid, lo, mid, hi)
    R.judge_mlp_bwd({k: want[k].float() for k in ("dpool",) + R.BWD_SUMS}, x, False, cid)
    pre = {k: torch.full_like(want[k], 0.5) for k in R.BWD_SUMS}
    R.judge_mlp_bwd({k: (want[k] + (0.5 if k != "dpool" else 0.0)) for k in ("dpool",) + R.BWD_SUMS}, x, True, cid, prefill=pre)


def test_mlp_bwd_judge_rejects_the_listed_mutants():
    """on the R = 4100 case: h_swish' taken as 1 on (2.9, 3), BatchNorm's backward without xh S2 / R, dbh accumulating the column positions,
    and results STORED over a prefilled target instead of added"""
    cid = "m8-ns2-c84-r4100"
    n, h, w, c, mip = R.MLP_BWD_CASES[cid]
    x = R.mlp_bwd_inputs(cid, n, h, w, c, mip)
    want = R.mlp_bwd(*R.bwd_args(x))
    assert int(((want["y1"] > 2.9) & (want["y1"] < 3)).sum()) > 0
    f32 = lambda o: {k: o[k].float() for k in ("dpool",) + R.BWD_SUMS}
    hs = f32(R.mlp_bwd(*R.bwd_args(x), hs_one=True))
    _rejects(R.judge_mlp_bwd, hs, x, False, "h_swish' = 1", keys=("dpool",))
    for k in ("dW1", "dgamma", "dbeta"):
        _rejects(R.judge_mlp_bwd, hs, x, False, "h_swish' = 1", keys=(k,))
    ns = f32(R.mlp_bwd(*R.bwd_args(x), no_s2=True))
    _rejects(R.judge_mlp_bwd, ns, x, False, "no S2 term", keys=("dpool",))
    _rejects(R.judge_mlp_bwd, ns, x, False, "no S2 term", keys=("dW1",))
    _rejects(R.judge_mlp_bwd, f32(R.mlp_bwd(*R.bwd_args(x), dbh_all=True)), x, False, "dbh over all positions", keys=("dbh",))
    pre = {k: torch.full_like(want[k], 0.5) for k in R.BWD_SUMS}
    for k in R.BWD_SUMS:
        _rejects(R.judge_mlp_bwd, f32(want), x, False, "stored, not added", prefill=pre, keys=(k,))


@pytest.mark.parametrize("cid", ["m8-ns1-c24-r33", "m16-ns4-c168-r2", "m16-ns8-c320-r100"])
def test_mlp_bwd_judge_rejects_missing_s2_term_on_small_cases(cid):
    n, h, w, c, mip = R.MLP_BWD_CASES[cid]
    x = R.mlp_bwd_inputs(cid, n, h, w, c, mip)
    bad = R.mlp_bwd(*R.bwd_args(x), no_s2=True)
    _rejects(R.judge_mlp_bwd, {"dpool": bad["dpool"].float()}, x, False, cid, keys=("dpool",))


def test_pool_bwd_judge_accepts_rounded_rejects_exchanged_divisors():
    for cid, (n, h, w, c, dts) in R.POOL_BWD_CASES.items():
        for dt in dts:
            x = R.pool_bwd_inputs(cid, dt)
            for acc in (False, True):
                want = R.pool_bwd(x["gp"].double(), h, w, R.d(x["dx0"]) if acc else None)
                R.judge_pool_bwd(want.to(dt), x, h, w, acc, cid)
    x = dict(gp=torch.randn(2, 41, 24, generator=torch.Generator().manual_seed(1)), dx0=torch.zeros(2, 20, 21, 24))
    bad = x["gp"][:, :20].double().unsqueeze(2) / 20 + x["gp"][:, 20:].double().unsqueeze(1) / 21
    _rejects(R.judge_pool_bwd, bad.float(), x, 20, 21, False, "divisors exchanged")


# ---------------------------------------------------------------- the whole chain ------------------------------------------------------------
@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=DT.values())
@pytest.mark.parametrize("case", R.CHAIN_CASES, ids=lambda v: "c%d-r%d-%dx%dx%d" % v)
def test_chain_inputs_hold_their_premises_and_judge_sees_one_channel(case, dtype):
    """no position in the kink band by the reference's own statistics, three regimes, a zero channel; the rounded reference passes the chain
    judge, an error of 1e-4 confined to ONE channel of dx (inside 1e-3 of the tensor's maximum) does not"""
    c, red, n, h, w = case
    ci = R.chain_inputs(c, red, n, h, w, dtype)
    ref = R.chain_parts(R.d(ci["x"]), ci["params"], R.d(ci["r"]))
    R.assert_no_kink(ref["y1"], ref["m_y1"], str(case))
    lo, mid, hi = R.regimes(ref["y1"])
    assert lo > 0 and mid > 0 and hi > 0, (case, lo, mid, hi)
    assert float(ci["x"][..., -1].abs().max()) == 0.0
    bf = dtype == R.BF16
    got = {k: (ref[k].to(dtype) if k in ("out", "dx") else ref[k].float()) for k in R.CHAIN_KEYS}
    R.judge_chain(got, ref, str(case), bf16=bf)
    if bf:                                          # (bf16's storage allowance 2^-8 is itself above 1e-3: the one-channel mutant is an fp32 matter)
        return
    amp = ref["dx"].abs().reshape(-1, c).amax(0)
    quiet = int(torch.where(amp > 0, amp, torch.full_like(amp, float("inf"))).argmin())
    bad = ref["dx"].clone()
    bad[..., quiet] *= 1 + 1e-4
    assert float((bad - ref["dx"]).abs().max()) <= 1e-3 * float(ref["dx"].abs().max())
    _rejects(R.judge_chain, dict(dx=bad.to(dtype)), ref, "dx one channel", bf16=bf)
    _rejects(R.judge_chain, dict(dgamma=ref["dgamma"].float() + 1e-3 * ref["dgamma"].abs().max().float()), ref, "dgamma off")


def test_nudge_moves_a_planted_band_element_out():
    """a position planted exactly on y1 = 3 is moved, and the band is empty afterwards"""
    w1, b1 = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).double(), torch.zeros(1).double()
    y1_of = lambda p: (R.conv1(p, w1, b1), R.conv1_mag(p, w1, b1))
    pl = torch.tensor([[[3.0, 1.0, 1.0, 1.0], [0.5, 1.0, 1.0, 1.0]]])
    assert int(R.in_band(*y1_of(pl.double())).sum()) == 1
    out, moved = R.nudge_pool(pl, y1_of, "planted")
    assert moved == 1 and torch.equal(out[0, 1], pl[0, 1])
    R.assert_no_kink(*y1_of(out.double()), "nudged")
