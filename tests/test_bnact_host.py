"""Host side of the BatchNorm + activation chain tests (tests/bnact_ref.py): the float64 reference against autograd and nn.BatchNorm2d, the
judges against planted defects (the evidence that tests/test_gpu_bnact.py would fail on a subtly wrong kernel — no broken kernel is ever
built or run), the measured constants, and the ReLU-band premise of every device case.  No GPU."""
import pytest
import torch

from tests import bnact_ref as R

ACT_IDS = {R.ACT_NONE: "none", R.ACT_RELU: "relu", R.ACT_SILU: "silu"}


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp(min=1e-300))


def _w(x):
    """the tensors of an input dict widened to float64"""
    return {k: (R.d(v) if torch.is_tensor(v) else v) for k, v in x.items()}


# ---------------------------------------------------------------- the reference against itself ----------------------------------------------
@pytest.mark.parametrize("act", R.ACTS, ids=ACT_IDS.values())
@pytest.mark.parametrize("rows,c", [(37, 8), (300, 24)])
def test_reference_chain_equals_autograd(rows, c, act):
    """fwd(finalize(.)) and apply(coeffs(reduce(.))) are F.batch_norm(training=True) + activation and its autograd, in float64 to 1e-12"""
    g = torch.Generator().manual_seed(rows + c + act)
    u = torch.randn(rows, c, generator=g, dtype=torch.float64) * 1.3 + 0.4
    r = torch.randn(rows, c, generator=g, dtype=torch.float64)
    gamma, beta = torch.rand(c, generator=g, dtype=torch.float64) + 0.5, torch.randn(c, generator=g, dtype=torch.float64)
    eps = 1e-3
    y, du, dg, db = R.chain_autograd(u, gamma, beta, eps, act, r)
    f = R.finalize(u.sum(0), (u * u).sum(0), float(rows), gamma, beta, eps, 0.03)
    assert _rel(R.fwd(u, f["scale"], f["shift"], act), y) <= 1e-12
    s1, s2 = R.reduce(r, u, f["scale"], f["shift"], act)
    co = R.coeffs(s1, s2, float(rows), f["scale"], f["mean"], f["invstd"], 1)
    assert _rel(co["dgamma"], dg) <= 1e-12 and _rel(co["dbeta"], db) <= 1e-12
    assert _rel(R.apply(r, u, f["scale"], f["shift"], act, co["alpha"], co["kappa"], co["lam"]), du) <= 1e-12


@pytest.mark.parametrize("count_hw", [(1, 1), (37, 1), (5, 7)])
def test_reference_running_statistics_equal_batchnorm2d(count_hw):
    """finalize's running mean / variance / num_batches_tracked are nn.BatchNorm2d's float64 update with momentum 0.03 (count = 1 included:
    torch refuses a single value per channel in training, so that case is checked against the formula's own limit var = 0)"""
    h, w = count_hw
    n, c = 3 if h * w > 1 else 1, 6
    count = n * h * w
    g = torch.Generator().manual_seed(count)
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) + 0.3
    rm, rv = torch.randn(c, generator=g, dtype=torch.float64), torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    rows = x.permute(0, 2, 3, 1).reshape(count, c)
    f = R.finalize(rows.sum(0), (rows * rows).sum(0), float(count), torch.ones(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64), 1e-3, 0.03, rm, rv, 4)
    assert f["nbt"] == 5
    if count == 1:
        assert _rel(f["rm"], 0.97 * rm + 0.03 * rows[0]) <= 1e-12 and _rel(f["rv"], 0.97 * rv) <= 1e-9
        return
    bn = torch.nn.BatchNorm2d(c, eps=1e-3, momentum=0.03).double().train()
    bn.running_mean.copy_(rm)
    bn.running_var.copy_(rv)
    bn.num_batches_tracked.fill_(4)
    y = bn(x)
    assert _rel(f["rm"], bn.running_mean) <= 1e-12 and _rel(f["rv"], bn.running_var) <= 1e-10 and int(bn.num_batches_tracked) == f["nbt"]
    assert _rel(R.fwd(rows, f["scale"], f["shift"], R.ACT_NONE), y.detach().permute(0, 2, 3, 1).reshape(count, c)) <= 1e-11


@pytest.mark.parametrize("act", [R.ACT_RELU, R.ACT_SILU], ids=["relu", "silu"])
def test_reference_eval_coefficients_equal_autograd(act):
    """train = 0: kappa = lambda = 0 and dgamma / dbeta / du are autograd's through an eval-mode BatchNorm"""
    rows, c, eps = 50, 12, 1e-3
    g = torch.Generator().manual_seed(5 + act)
    u, r = torch.randn(rows, c, generator=g, dtype=torch.float64), torch.randn(rows, c, generator=g, dtype=torch.float64)
    gamma, beta = torch.rand(c, generator=g, dtype=torch.float64) + 0.5, torch.randn(c, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(c, generator=g, dtype=torch.float64) * 0.3, torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    y, du, dg, db = R.chain_autograd(u, gamma, beta, eps, act, r, training=False, rm=rm, rv=rv)
    invstd = 1 / torch.sqrt(rv + eps)
    a, b = gamma * invstd, beta - rm * gamma * invstd
    s1, s2 = R.reduce(r, u, a, b, act)
    co = R.coeffs(s1, s2, float(rows), a, rm, invstd, 0)
    assert float(co["kappa"].abs().max()) == 0.0 and float(co["lam"].abs().max()) == 0.0
    assert _rel(co["dgamma"], dg) <= 1e-12 and _rel(co["dbeta"], db) <= 1e-12
    assert _rel(R.apply(r, u, a, b, act, co["alpha"], co["kappa"], co["lam"]), du) <= 1e-12
    assert _rel(R.fwd(u, a, b, act), y) <= 1e-12


# ---------------------------------------------------------------- measured constants ---------------------------------------------------------
def test_measured_k_and_chain_tolerance_hold():
    """the constants of tests/bnact_ref.py are four times what the reference itself shows when evaluated in float32 (and so every judge accepts
    torch's float32 evaluation of the reference over every case), K_ELEM stays under 64 and CHAIN_TOL under 1e-4"""
    k = R.measure_k()
    assert max(k.values()) * 4 <= R.K_ELEM <= 64, k
    t = R.measure_chain_tol()
    assert max(t.values()) * 4 <= R.CHAIN_TOL <= 1e-4, t


# ---------------------------------------------------------------- judge sensitivity ----------------------------------------------------------
def _rejects(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("act", R.ACTS, ids=ACT_IDS.values())
def test_elementwise_judge_accepts_rounded_and_float32_rejects_stale_row(act, dtype):
    """(4099, 64): the float64 result rounded to the storage type and torch's float32 evaluation pass; one row of 4099 left at its old value
    (du written over u: the row still holds u) does not"""
    rows, c = 4099, 64
    x = R.elem_inputs("sens", rows, c, dtype, act)
    w = _w(x)
    bf = dtype == R.BF16
    args = (w["dy"], w["u"], w["a"], w["b"], act, w["alpha"], w["kappa"], w["lam"])
    want, mag = R.apply(*args), R.apply_mag(*args)
    R.judge_elem(want.to(dtype), want, mag, "apply rounded", bf16=bf)
    f32 = R.apply(x["dy"].float(), x["u"].float(), x["a"], x["b"], act, x["alpha"], x["kappa"], x["lam"])
    R.judge_elem(f32.to(dtype), want, mag, "apply float32", bf16=bf)
    bad = want.to(dtype).clone()
    bad[2047] = x["u"][2047]
    _rejects(R.judge_elem, bad, want, mag, "apply stale row", bf16=bf)
    wy, my = R.fwd(w["u"], w["a"], w["b"], act), R.fwd_mag(w["u"], w["a"], w["b"], act)
    R.judge_elem(wy.to(dtype), wy, my, "fwd rounded", bf16=bf)
    R.judge_elem(R.fwd(x["u"].float(), x["a"], x["b"], act).to(dtype), wy, my, "fwd float32", bf16=bf)
    bad = wy.to(dtype).clone()
    bad[rows - 1] = x["u"][rows - 1]
    _rejects(R.judge_elem, bad, wy, my, "fwd stale row", bf16=bf)


@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=["f32", "bf16"])
def test_judges_reject_silu_derivative_without_inner_term(dtype):
    """dv = dy s instead of dy s (1 + v (1 - s)): rejected elementwise (apply) and in the sums (reduce)"""
    rows, c = 37, 8
    x = R.elem_inputs("sens-silu", rows, c, dtype, R.ACT_SILU)
    w = _w(x)
    args = (w["dy"], w["u"], w["a"], w["b"], R.ACT_SILU, w["alpha"], w["kappa"], w["lam"])
    want, mag = R.apply(*args), R.apply_mag(*args)
    dv_bad = w["dy"] * torch.sigmoid(w["a"] * w["u"] + w["b"])
    _rejects(R.judge_elem, (w["alpha"] * dv_bad + w["kappa"] + w["lam"] * w["u"]).to(dtype), want, mag, "apply", bf16=dtype == R.BF16)
    s1, s2 = R.reduce(*args[:5])
    (t1, t2), (m1, m2) = R.reduce_mag(*args[:5])
    ch = R.reduce_chain(rows, c)
    R.judge_sum(s1, s1, ch, t1, m1, "s1")
    _rejects(R.judge_sum, dv_bad.sum(0), s1, ch, t1, m1, "s1")
    _rejects(R.judge_sum, (dv_bad * w["u"]).sum(0), s2, ch, t2, m2, "s2")


@pytest.mark.parametrize("act", R.ACTS, ids=ACT_IDS.values())
def test_sum_judge_accepts_float32_rejects_dropped_row(act):
    """(4099, 64): the float64 sums rounded to float32 and torch's float32 sums pass; the LAST ROW OF ONE EIGHTH of the rows (an XCD range's
    end) missing from the sum does not"""
    rows, c = 4099, 64
    x = R.elem_inputs("sens-sum", rows, c, R.F32, act)
    w = _w(x)
    args = (w["dy"], w["u"], w["a"], w["b"], act)
    s1, s2 = R.reduce(*args)
    (t1, t2), (m1, m2) = R.reduce_mag(*args)
    ch = R.reduce_chain(rows, c)
    R.judge_sum(s1.float(), s1, ch, t1, m1, "s1 rounded")
    R.judge_sum(s2.float(), s2, ch, t2, m2, "s2 rounded")
    f1, f2 = R.reduce(x["dy"], x["u"], x["a"], x["b"], act)
    R.judge_sum(f1, s1, ch, t1, m1, "s1 float32")
    R.judge_sum(f2, s2, ch, t2, m2, "s2 float32")
    last = 3 * ((rows + 7) // 8) - 1                    # the last row of the third eighth
    dv = R.dact(w["a"] * w["u"] + w["b"], w["dy"], act)
    _rejects(R.judge_sum, (s1 - dv[last]).float(), s1, ch, t1, m1, "s1 without a row")
    _rejects(R.judge_sum, (s2 - dv[last] * w["u"][last]).float(), s2, ch, t2, m2, "s2 without a row")
    # the plain row sums of ly_sum_rows / ly_chan_moments: the same judge with exact terms
    xs = w["u"]
    R.judge_sum(x["u"].sum(0), xs.sum(0), R.sum_rows_chain(rows), xs.abs().sum(0), torch.zeros(c, dtype=torch.float64), "plain sum float32")
    _rejects(R.judge_sum, (xs.sum(0) - xs[last]).float(), xs.sum(0), R.sum_rows_chain(rows), xs.abs().sum(0), torch.zeros(c, dtype=torch.float64), "plain sum")


@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=["f32", "bf16"])
def test_judges_reject_pair_second_unit_from_first_gradient(dtype):
    """the second unit of a pair computed from dy1 (the two gradients differ in scale, x1 and x100): rejected in apply and in reduce"""
    cid = "pair-half-c80"
    rows, c, cs = R.PAIR_CASES[cid][:3]
    x = R.elem_inputs(cid, rows, c, dtype, R.ACT_SILU, cs)
    w = _w(x)
    sl = slice(cs, c)
    co = [w[k][sl] for k in ("a", "b")] + [R.ACT_SILU] + [w[k][sl] for k in ("alpha", "kappa", "lam")]
    want, mag = R.apply(w["dy"][:, sl], w["u"][:, sl], *co), R.apply_mag(w["dy"][:, sl], w["u"][:, sl], *co)
    R.judge_elem(want.to(dtype), want, mag, "unit 2", bf16=dtype == R.BF16)
    swapped = R.apply(w["dy"][:, :c - cs], w["u"][:, sl], *co)
    _rejects(R.judge_elem, swapped.to(dtype), want, mag, "unit 2 from dy1", bf16=dtype == R.BF16)
    s1, _ = R.reduce(w["dy"][:, sl], w["u"][:, sl], *co[:3])
    (t1, _), (m1, _) = R.reduce_mag(w["dy"][:, sl], w["u"][:, sl], *co[:3])
    b1, _ = R.reduce(w["dy"][:, :c - cs], w["u"][:, sl], *co[:3])
    _rejects(R.judge_sum, b1, s1, R.reduce_chain(rows, c), t1, m1, "unit 2 sums from dy1")


def _coeff_inputs(n, stripes, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    sums = (torch.randn(stripes, 2 * n, generator=g, dtype=torch.float64) * 3).to(dtype)
    a = (torch.rand(n, generator=g, dtype=torch.float64) + 0.5).float()
    mean = torch.randn(n, generator=g, dtype=torch.float64).float()
    invstd = (torch.rand(n, generator=g, dtype=torch.float64) + 0.5).float()
    return sums, a, mean, invstd


def test_coefficient_judge_rejects_kappa_off_and_missing_stripe():
    """kappa off by 1e-3 relative in ONE channel of 160, and one stripe of 32 missing from the fold: rejected; the float64 results rounded to
    float32 pass"""
    n, count = 160, 4321.0
    sums, a, mean, invstd = _coeff_inputs(n, R.STRIPES, 3)
    want = R.coeffs(*R.fold(sums), count, R.d(a), R.d(mean), R.d(invstd), 1)
    got = {k: want[k].float() for k in ("dgamma", "dbeta", "alpha", "kappa", "lam")}
    R.judge_coeffs(got, want, "rounded")
    bad = dict(got)
    bad["kappa"] = got["kappa"].clone()
    bad["kappa"][97] *= 1.001
    _rejects(R.judge_coeffs, bad, want, "kappa off")
    short = torch.cat([sums[:17], sums[18:]])
    miss = R.coeffs(*R.fold(short), count, R.d(a), R.d(mean), R.d(invstd), 1)
    for key in ("dgamma", "dbeta", "kappa", "lam"):
        _rejects(R.judge_coeffs, {key: miss[key].float()}, want, "stripe missing")


def test_finalize_judge_rejects_biased_variance_and_missing_stripe():
    """count = 37: the running variance from the BIASED batch variance is rejected (36/37 of the right value), as is a fold that misses one
    stripe of 32; float64 rounded to float32 passes"""
    n, count = 65, 37.0
    g = torch.Generator().manual_seed(8)
    x = torch.randn(R.STRIPES, 37, n, generator=g, dtype=torch.float64) * 0.2 + 0.1        # each stripe's share of the 37 values... as sums
    stats = torch.cat([x.sum(1) / R.STRIPES, (x * x).sum(1) / R.STRIPES], 1)
    gamma, beta = torch.rand(n, generator=g, dtype=torch.float64) + 0.5, torch.randn(n, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(n, generator=g, dtype=torch.float64), torch.rand(n, generator=g, dtype=torch.float64) + 0.5
    want = R.finalize(*R.fold(stats), count, gamma, beta, 1e-3, 0.03, rm, rv, 0)
    keys = ("scale", "shift", "mean", "invstd", "rm", "rv")
    R.judge_finalize({**{k: want[k].float() for k in keys}, "nbt": 1}, want, "rounded")
    _rejects(R.judge_finalize, {"nbt": 2}, want, "counted twice")
    biased = R.finalize(*R.fold(stats), count, gamma, beta, 1e-3, 0.03, rm, rv, 0, biased=True)
    _rejects(R.judge_finalize, {"rv": biased["rv"].float()}, want, "biased")
    miss = R.finalize(*R.fold(torch.cat([stats[:5], stats[6:]])), count, gamma, beta, 1e-3, 0.03, rm, rv, 0)
    for key in keys:
        _rejects(R.judge_finalize, {key: miss[key].float()}, want, "stripe missing")


def test_chain_judge_rejects_error_confined_to_one_channel():
    """the per-channel judge sees what `1e-3 x max|tensor|` does not: one channel of 64 off by 1e-4 of its own size"""
    rows, c = 4099, 64
    ci = R.chain_inputs(rows, c, R.F32, R.ACT_SILU)
    ref = R.chain_reference(ci, rows, R.ACT_SILU)
    R.judge_channels(ref["du"].float(), ref["du"], "du rounded")
    bad = ref["du"].clone()
    amp = ref["du"].abs().amax(0)
    quiet = int(torch.where(amp > 0, amp, torch.full_like(amp, float("inf"))).argmin())       # (the gamma = 0 channel's du is exactly 0)
    bad[:, quiet] *= 1 + 1e-4
    assert float((bad - ref["du"]).abs().max()) <= 1e-3 * float(ref["du"].abs().max())
    _rejects(R.judge_channels, bad.float(), ref["du"], "du one channel")


# ---------------------------------------------------------------- the band premise of every device case --------------------------------------
def test_no_device_case_has_an_element_in_the_relu_band():
    """for every (seed, shape) tests/test_gpu_bnact.py uses, the builder leaves NO element in the kink band (the cap is zero); the
    deliberate exact-zero column is there and decided"""
    for cid, (rows, c, _, _, _, dts, _) in R.ELEM_CASES.items():
        for dt in dts:
            x = R.elem_inputs(cid, rows, c, dt, R.ACT_RELU)
            R.assert_no_kink(x["u"], x["a"], x["b"], cid)
            assert float(x["u"][:, c - 1].abs().max()) == 0.0 and float(x["b"][c - 1]) == 0.0
    for cid, (rows, c, cs, _, _, dts) in R.PAIR_CASES.items():
        for dt in dts:
            x = R.elem_inputs(cid, rows, c, dt, R.ACT_RELU, cs)
            R.assert_no_kink(x["u"], x["a"], x["b"], cid)
    for rows, c in R.CHAIN_CASES:
        for dt in (R.F32, R.BF16):
            ci = R.chain_inputs(rows, c, dt, R.ACT_RELU)
            a, b = R.chain_ab(ci, rows)
            R.assert_no_kink(ci["u"], a, b, f"chain {rows}x{c}", R.CHAIN_KINK)
            v = a * R.d(ci["u"]) + b
            assert bool((v[:, 2] < 0).all())                         # the dead channel is dead on every row


def test_nudge_moves_planted_band_elements_out():
    """the builder's nudge, on elements planted exactly on the kink (fp32 and bf16 storage)"""
    for dt in (R.F32, R.BF16):
        a, b = torch.tensor([1.25, 0.75]), torch.tensor([0.5, -1.5])
        u = torch.stack([-b / a, -b / a]).to(dt)                   # v = 0 up to storage rounding
        u2, moved = R.nudge(u, a, b, dt)
        assert moved > 0
        R.assert_no_kink(u2, a, b, "nudged")


def test_edge_values_reach_the_silu_limits():
    """the builder's v = +-90 elements: the float64 reference is finite there, equal to the limits y = v / 0 and dv = dy / 0 within the judge"""
    x = _w(R.elem_inputs("lanes-c8-r37", 37, 8, R.F32, R.ACT_SILU))
    v = x["a"] * x["u"] + x["b"]
    assert abs(float(v[0, 0]) - 90) < 1e-3 and abs(float(v[36, 1]) + 90) < 1e-3 and float(v.abs().max()) < 91 and float(v.abs()[5].max()) > 15
    y = R.fwd(x["u"], x["a"], x["b"], R.ACT_SILU)
    assert bool(torch.isfinite(y).all()) and abs(float(y[0, 0] - v[0, 0])) < 1e-30 and abs(float(y[36, 1])) < 1e-36
    dv = R.dact(v, x["dy"], R.ACT_SILU)
    assert abs(float(dv[0, 0] - x["dy"][0, 0])) < 1e-30 and abs(float(dv[36, 1])) < 1e-35
