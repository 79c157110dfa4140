"""The train-mode BatchNorm + activation kernel chain, kernel by kernel against float64 (tests/bnact_ref.py: references, judges with
conditioned bounds, input builders, case tables; tests/test_bnact_host.py shows on the CPU that those judges reject subtly wrong results).
Everything goes through lead_yolo_amd.ops; no judge compares a kernel with itself except the bit-for-bit aliasing / repeatability checks.

Measured on the MI355X, worst over all cases (each test prints its own figures before the next one asserts):
    elementwise, what is left of the error after the storage allowance, in units of 2^-24 M:  fwd 3.54, apply 4.44   (K_ELEM = 22;
        torch's float32 evaluation on the CPU: 3.48, 5.35)
    whole chain, fp32, per channel:  y 9.1e-7, du 3.5e-7 of max|ref|   (CHAIN_TOL = 2.1e-6; float32 autograd on the CPU: 4.6e-7, 5.2e-7);
        dgamma / dbeta inside the sums' floor; bf16 tensors inside the storage allowance
No defect was found in the kernels: nothing in csrc/ changed with these tests.

branch of the kernels                                  ->  case id (ELEM_CASES / PAIR_CASES of tests/bnact_ref.py, or test)
  thread = (channel vector, row lane)
    C = 8: ncv = 2 (fp32) / 1 (bf16), 128 / 256 groups     lanes-c8-r{1,7,8,9,37}
    C = 24: ncv = 6, 42 groups, 4 idle threads (fp32,      lanes-c24-r*          (bf16 forward / apply: ncv = 3, 85 groups, 1 idle)
      and the reduce pass in both dtypes)
    C = 160: a common model width                           lanes-c160-r*
    C = 1024: one group, the reduce pass's limit            lanes-c1024-r*
  per-XCD row split (LY_XCD_ROWS)
    forward / apply: grid always >= 8, most eighths empty   lanes-*-r1 ... r9
    reduce: 7 blocks (off) / 8 blocks (on, uneven eighths)  xcd-off-c160-r1344 / xcd-on-c160-r1351, xcd-off-c1024-r224 / xcd-on-c1024-r233
  four rows in flight, clamped re-reads of the last row     rows 1, 7, 9, 37, 1351, 233 (no multiple of 4 x groups)
  16-byte vectors vs the flat-index fallback
    C % VW                                                  fallback-bf16-c12-r37, fallback-bf16-c20-r37
    ld % VW                                                 fallback-bf16-c16-ld20
    C / VW > 256                                            fallback-f32-c1028 (forward, apply; the reduce pass refuses it: test_refusals)
    LY_XCD_RANGE on (>= 8 blocks) / off (1 block)           fallback-bf16-c12-r2500-xcdrange / fallback-bf16-c12-r37
    csplit % VW                                             pair-20-of-40-fallback (bf16)
  ld > C, each operand on its own, sentinel columns         ld-u-c160, ld-dy-c160, ld-out-c160, ld-all-c24
  du over u / over dy                                       every case whose leading dimensions allow it (test_bnact_fwd_apply_reduce)
  pair form: dy2 / sums2 by channel                         pair-half-c{16,80,512}, pair-8-of-40, pair-32-of-40, pair-ld-differ-c80
  ly_fold_stripes: 32 stripes / batches of 8 / tail         test_bn_finalize, test_bn_bwd_coeffs [s32 / s9 (8 + 1) / s1]
  ly_sum_rows: 8 / 4 / 1-row loops, 4 vs 16 row lanes       test_sum_rows [R = 1 ... 1000: 192 -> 4 lanes, 193 -> 16]
"""
import pytest
import torch

from tests import bnact_ref as R

pytestmark = pytest.mark.gpu

ACT_IDS = {R.ACT_NONE: "none", R.ACT_RELU: "relu", R.ACT_SILU: "silu"}
DT_IDS = {R.F32: "f32", R.BF16: "bf16"}
SENTINEL = 777.0


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a CUDA/ROCm device"
    return torch.device("cuda:0")


def _vw(dt):
    return 8 if dt == R.BF16 else 4


def _place(t, ld, dev):
    """t [rows, C] inside a full [rows, ld] allocation filled with a sentinel, as a channel-slice view.  The slice starts one 16-byte vector
    in (what ops.rows admits: data_ptr % 16 == 0 with ld % vw == 0) when it fits, else at column 0.  -> (full, view, offset)"""
    rows, c = t.shape
    vw = _vw(t.dtype)
    off = vw if (ld % vw == 0 and c + vw <= ld) else 0
    full = torch.full((rows, ld), SENTINEL, dtype=t.dtype, device=dev)
    full[:, off:off + c] = t.to(dev)
    return full, full[:, off:off + c], off


def _outside_untouched(full, off, c):
    rest = torch.cat([full[:, :off], full[:, off + c:]], 1)
    return bool((rest == SENTINEL).all())


def _cases(table, dt_index):
    return [pytest.param(cid, dt, id=f"{cid}-{DT_IDS[dt]}") for cid, v in table.items() for dt in v[dt_index]]


def test_activation_codes():
    from lead_yolo_amd import ops
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_SILU) == (R.ACT_NONE, R.ACT_RELU, R.ACT_SILU) and ops.STRIPES == R.STRIPES


# ---------------------------------------------------------------- forward / apply / reduce ---------------------------------------------------
@pytest.mark.parametrize("cid,dtype", _cases(R.ELEM_CASES, 5))
def test_bnact_fwd_apply_reduce(cid, dtype):
    """ly_bnact_fwd, ly_bnact_bwd_apply and ly_bnact_bwd_reduce against float64 of the stored operands, none / ReLU / SiLU: |v| up to 30, v = +-90,
    an exact-zero column; every operand a slice view of its own full allocation (columns outside [0, C) of the destination keep their bits);
    du over u and over dy leave the bits of the out-of-place call"""
    from lead_yolo_amd import ops
    rows, c, ldu, lddy, ldo, _, with_reduce = R.ELEM_CASES[cid]
    dev = _dev()
    bf = dtype == R.BF16
    for act in R.ACTS:
        x = R.elem_inputs(cid, rows, c, dtype, act)
        if act == R.ACT_RELU:
            R.assert_no_kink(x["u"], x["a"], x["b"], cid)
        w = {k: R.d(v) for k, v in x.items() if torch.is_tensor(v)}
        co = {k: x[k].to(dev) for k in ("a", "b", "alpha", "kappa", "lam")}
        _, u, _ = _place(x["u"], ldu, dev)
        _, dy, _ = _place(x["dy"], lddy, dev)
        what = f"{cid} {DT_IDS[dtype]} {ACT_IDS[act]}"
        # forward
        yfull, y, yoff = _place(torch.zeros(rows, c, dtype=dtype), ldo, dev)
        y.fill_(SENTINEL)
        ops.bnact_fwd(u, ldu, rows, c, co["a"], co["b"], act, y, ldo)
        torch.cuda.synchronize()
        rf = R.judge_elem(y, R.fwd(w["u"], w["a"], w["b"], act), R.fwd_mag(w["u"], w["a"], w["b"], act), what + " fwd", bf16=bf)
        assert _outside_untouched(yfull, yoff, c), what + " fwd wrote outside [0, C)"
        # apply, out of place
        args = (w["dy"], w["u"], w["a"], w["b"], act, w["alpha"], w["kappa"], w["lam"])
        dfull, du, doff = _place(torch.zeros(rows, c, dtype=dtype), ldo, dev)
        du.fill_(SENTINEL)
        ops.bnact_bwd_apply(dy, lddy, u, ldu, rows, c, co["a"], co["b"], act, co["alpha"], co["kappa"], co["lam"], du, ldo)
        torch.cuda.synchronize()
        ra = R.judge_elem(du, R.apply(*args), R.apply_mag(*args), what + " apply", bf16=bf)
        assert _outside_untouched(dfull, doff, c), what + " apply wrote outside [0, C)"
        if act == R.ACT_RELU:                       # the exact-zero column: dv = 0, du = kappa
            assert torch.equal(du[:, c - 1].cpu(), x["kappa"][c - 1].to(dtype).expand(rows)), what + " exact zeros"
        # apply over u, over dy: the same bits
        for name, src, ld in (("u", x["u"], ldu), ("dy", x["dy"], lddy)):
            full, alias, off = _place(src, ld, dev)
            if name == "u":
                ops.bnact_bwd_apply(dy, lddy, alias, ld, rows, c, co["a"], co["b"], act, co["alpha"], co["kappa"], co["lam"], alias, ld)
            else:
                ops.bnact_bwd_apply(alias, ld, u, ldu, rows, c, co["a"], co["b"], act, co["alpha"], co["kappa"], co["lam"], alias, ld)
            torch.cuda.synchronize()
            assert torch.equal(alias, du), f"{what} apply over {name}"
            assert _outside_untouched(full, off, c), f"{what} apply over {name} wrote outside [0, C)"
        # reduce
        if with_reduce:
            sums = ops.bnact_bwd_reduce(dy, lddy, u, ldu, rows, c, co["a"], co["b"], act)
            torch.cuda.synchronize()
            assert tuple(sums.shape) == (R.STRIPES, 2 * c) and sums.dtype == torch.float64
            s1, s2 = R.fold(sums)
            w1, w2 = R.reduce(*args[:5])
            (t1, t2), (m1, m2) = R.reduce_mag(*args[:5])
            ch = R.reduce_chain(rows, c)
            R.judge_sum(s1, w1, ch, t1, m1, what + " reduce s1")
            R.judge_sum(s2, w2, ch, t2, m2, what + " reduce s2")
            if act == R.ACT_RELU:
                assert float(s1[c - 1]) == 0.0 and float(s2[c - 1]) == 0.0, what + " exact zeros"
        print(f"{what}: worst err / (2^-24 M)  fwd {rf:.2f}  apply {ra:.2f}")


@pytest.mark.parametrize("cid,dtype", _cases(R.PAIR_CASES, 5))
def test_bnact_pair_forms(cid, dtype):
    """ly_bnact_bwd_reduce_pair / ly_bnact_bwd_apply_pair against float64 PER UNIT (unit 2's gradient is 100 x unit 1's: a swapped source
    is far outside every bound), equal and unequal splits, the csplit % 8 fallback in bf16, lddy1 != lddy2"""
    from lead_yolo_amd import ops
    rows, c, cs, ld1, ld2, _ = R.PAIR_CASES[cid]
    dev = _dev()
    bf = dtype == R.BF16
    for act in R.ACTS:
        x = R.elem_inputs(cid, rows, c, dtype, act, cs)
        if act == R.ACT_RELU:
            R.assert_no_kink(x["u"], x["a"], x["b"], cid)
        w = {k: R.d(v) for k, v in x.items() if torch.is_tensor(v)}
        co = {k: x[k].to(dev) for k in ("a", "b", "alpha", "kappa", "lam")}
        u = x["u"].to(dev)
        _, dy1, _ = _place(x["dy"][:, :cs], ld1, dev)
        _, dy2, _ = _place(x["dy"][:, cs:], ld2, dev)
        what = f"{cid} {DT_IDS[dtype]} {ACT_IDS[act]}"
        sa, sb = ops.bnact_bwd_reduce_pair(dy1, ld1, dy2, ld2, cs, u, c, rows, c, co["a"], co["b"], act)
        du = torch.full((rows, c), SENTINEL, dtype=dtype, device=dev)
        ops.bnact_bwd_apply_pair(dy1, ld1, dy2, ld2, cs, u, c, rows, c, co["a"], co["b"], act, co["alpha"], co["kappa"], co["lam"], du, c)
        torch.cuda.synchronize()
        ch = R.reduce_chain(rows, c)
        for unit, sl, sums in ((1, slice(0, cs), sa), (2, slice(cs, c), sb)):
            n = sl.stop - sl.start
            assert tuple(sums.shape) == (R.STRIPES, 2 * n)
            args = (w["dy"][:, sl], w["u"][:, sl], w["a"][sl], w["b"][sl], act, w["alpha"][sl], w["kappa"][sl], w["lam"][sl])
            R.judge_elem(du[:, sl], R.apply(*args), R.apply_mag(*args), f"{what} apply unit {unit}", bf16=bf)
            s1, s2 = R.fold(sums)
            w1, w2 = R.reduce(*args[:5])
            (t1, t2), (m1, m2) = R.reduce_mag(*args[:5])
            R.judge_sum(s1, w1, ch, t1, m1, f"{what} reduce s1 unit {unit}")
            R.judge_sum(s2, w2, ch, t2, m2, f"{what} reduce s2 unit {unit}")


# ---------------------------------------------------------------- finalize -------------------------------------------------------------------
def _bn(n, g, dev, momentum=0.03, eps=1e-3, track=True):
    bn = torch.nn.BatchNorm2d(n, eps=eps, momentum=momentum, track_running_stats=track).train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(n, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(n, generator=g))
        if track:
            bn.running_mean.copy_(torch.randn(n, generator=g))
            bn.running_var.copy_(torch.rand(n, generator=g) + 0.5)
            bn.num_batches_tracked.fill_(3)
    return bn.to(dev)


def _stats(stripes, nch, count, dtype, g):
    """striped (sum, sum of squares) [stripes][2 nch] of `count` values per channel, stored as dtype: channel 0 is constant, channel 1 has
    s2 / count < mean^2 by rounding (the clamp), the rest have mean ~ N, variance in [0.2, 2.2]"""
    mu = torch.randn(nch, generator=g, dtype=torch.float64)
    var = torch.rand(nch, generator=g, dtype=torch.float64) * 2 + 0.2 if count > 1 else torch.zeros(nch, dtype=torch.float64)
    var[0] = 0.0
    s1, s2 = count * mu, count * (var + mu * mu)
    if nch > 1:
        mu1 = 1.1 if float(mu[1].abs()) < 0.1 else float(mu[1])
        s1[1], s2[1] = count * mu1, count * mu1 * mu1 * (1 - (2.0 ** -40 if dtype == torch.float64 else 2.0 ** -18))
    wgt = torch.rand(stripes, 1, generator=g, dtype=torch.float64) + 0.1
    wgt = wgt / wgt.sum()
    if nch > 1 and stripes > 1:                      # the clamp channel lives in one stripe: its deficit survives the storage rounding
        st = torch.cat([wgt * s1, wgt * s2], 1)
        st[:, 1], st[:, nch + 1] = 0.0, 0.0
        st[stripes - 1, 1], st[stripes - 1, nch + 1] = s1[1], s2[1]
    else:
        st = torch.cat([wgt * s1, wgt * s2], 1)
    return st.to(dtype).contiguous()


def _want_finalize(bn, stats_cpu, count, sl=slice(None), nch=None):
    s1, s2 = R.fold(stats_cpu)
    track = bn.running_mean is not None
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))           # eps / momentum reach the kernel as floats
    return R.finalize(s1[sl], s2[sl], float(count), R.d(bn.weight), R.d(bn.bias), f32(bn.eps), f32(bn.momentum), R.d(bn.running_mean) if track else None,
                      R.d(bn.running_var) if track else None, int(bn.num_batches_tracked) if track else 0)


@pytest.mark.parametrize("sdt", [torch.float64, torch.float32], ids=["s64", "s32"])
@pytest.mark.parametrize("stripes", [1, 9, 32], ids=["s1", "s9", "s32"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_bn_finalize(n, stripes, sdt):
    """ly_bn_finalize against float64: scale, shift, mean, invstd, running mean / variance (unbiased), num_batches_tracked + 1 per launch;
    momentum 0.03 and 1.0, a BatchNorm without running statistics; a constant channel and a channel whose variance is clamped; count = 1"""
    from lead_yolo_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(1000 * n + 10 * stripes + (sdt == torch.float32))
    for count, momentum, track in ((37.0, 0.03, True), (4321.0, 1.0, True), (37.0, 0.03, False), (1.0, 0.03, True)):
        bn = _bn(n, g, dev, momentum=momentum, track=track)
        st = _stats(stripes, n, count, sdt, g)
        want = _want_finalize(bn, st, count)
        if n > 1 and count > 1:
            s1, s2 = R.fold(st)
            eps32 = float(torch.tensor(bn.eps, dtype=torch.float32))
            assert float(s2[1] / count - (s1[1] / count) ** 2) < 0 and float(want["invstd"][1]) == 1.0 / eps32 ** 0.5      # the clamp is reached
        scale, shift, mean, invstd = ops.bn_finalize(bn, st.to(dev), n, count, want_stats=True)
        torch.cuda.synchronize()
        got = dict(scale=scale, shift=shift, mean=mean, invstd=invstd)
        if track:
            got.update(rm=bn.running_mean, rv=bn.running_var, nbt=bn.num_batches_tracked)
        R.judge_finalize(got, want, f"finalize n={n} stripes={stripes} count={count} momentum={momentum} track={track}")
        if track:                                    # a second launch counts once more
            ops.bn_finalize(bn, st.to(dev), n, count)
            torch.cuda.synchronize()
            assert int(bn.num_batches_tracked) == 5


@pytest.mark.parametrize("sdt", [torch.float64, torch.float32], ids=["s64", "s32"])
def test_bn_finalize_windows_padding_and_slices(sdt):
    """c_off / n windows of a wider statistics array, pad_to > n (the tail stays zero), into= slices of a wider vector"""
    from lead_yolo_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(77)
    count = 300.0
    # MLPBlock's form: the first n of nch channels, zero-padded to pad_to
    nch, n, pad = 96, 80, 96
    bn, st = _bn(n, g, dev), _stats(32, nch, count, sdt, g)
    want = _want_finalize(bn, st, count, slice(0, n))
    scale, shift, mean, invstd = ops.bn_finalize(bn, st.to(dev), nch, count, n=n, pad_to=pad, want_stats=True)
    torch.cuda.synchronize()
    assert scale.numel() == pad and shift.numel() == pad and float(scale[n:].abs().max()) == 0.0 and float(shift[n:].abs().max()) == 0.0
    R.judge_finalize(dict(scale=scale[:n], shift=shift[:n], mean=mean, invstd=invstd, rm=bn.running_mean, rv=bn.running_var, nbt=bn.num_batches_tracked),
                     want, "finalize pad_to")
    # two BatchNorms over one stacked array: windows [0, 65) and [65, 130), written into slices of one [4, 130] tensor
    nch, half = 130, 65
    st = _stats(9, nch, count, sdt, g)
    v = torch.full((4, nch), SENTINEL, dtype=torch.float32, device=dev)
    bns = [_bn(half, g, dev), _bn(half, g, dev, momentum=0.1, eps=1e-5)]
    wants = [_want_finalize(bn, st, count, slice(i * half, (i + 1) * half)) for i, bn in enumerate(bns)]
    ops.bn_finalize(bns[1], st.to(dev), nch, count, n=half, c_off=half, into=tuple(v[k, half:] for k in range(4)))
    torch.cuda.synchronize()
    assert bool((v[:, :half] == SENTINEL).all())
    ops.bn_finalize(bns[0], st.to(dev), nch, count, n=half, c_off=0, into=tuple(v[k, :half] for k in range(4)))
    torch.cuda.synchronize()
    for i, bn in enumerate(bns):
        sl = slice(i * half, (i + 1) * half)
        R.judge_finalize(dict(scale=v[0, sl], shift=v[1, sl], mean=v[2, sl], invstd=v[3, sl], rm=bn.running_mean, rv=bn.running_var, nbt=bn.num_batches_tracked),
                         wants[i], f"finalize window {i}")


@pytest.mark.parametrize("stripes,sdt", [(32, torch.float64), (9, torch.float32), (1, torch.float64)], ids=["s32-f64", "s9-f32", "s1-f64"])
@pytest.mark.parametrize("c_half", [1, 32, 33, 65, 130])
def test_bn_finalize_pair(c_half, stripes, sdt):
    """ly_bn_finalize_pair against float64 per unit (the units differ in eps and momentum; the second one also runs without running
    statistics): every output, and num_batches_tracked of BOTH units goes up by exactly one"""
    from lead_yolo_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(31 * c_half + stripes)
    count = 523.0
    for track2 in (True, False):
        bns = [_bn(c_half, g, dev), _bn(c_half, g, dev, momentum=0.1, eps=1e-5, track=track2)]
        st = _stats(stripes, 2 * c_half, count, sdt, g)
        wants = [_want_finalize(bn, st, count, slice(i * c_half, (i + 1) * c_half)) for i, bn in enumerate(bns)]
        v = torch.empty(4, 2 * c_half, dtype=torch.float32, device=dev)
        ops.bn_finalize_pair(bns[0], bns[1], st.to(dev), c_half, count, v)
        torch.cuda.synchronize()
        for i, bn in enumerate(bns):
            sl = slice(i * c_half, (i + 1) * c_half)
            got = dict(scale=v[0, sl], shift=v[1, sl], mean=v[2, sl], invstd=v[3, sl])
            if bn.running_mean is not None:
                got.update(rm=bn.running_mean, rv=bn.running_var, nbt=bn.num_batches_tracked)
            R.judge_finalize(got, wants[i], f"finalize_pair c_half={c_half} unit {i} track2={track2}")


# ---------------------------------------------------------------- backward coefficients ------------------------------------------------------
def _coeff_case(n, stripes, sdt, g, scale=1.0):
    sums = (torch.randn(stripes, 2 * n, generator=g, dtype=torch.float64) * 3 * scale).to(sdt)
    a = (torch.rand(n, generator=g, dtype=torch.float64) + 0.5).float()
    mean = torch.randn(n, generator=g, dtype=torch.float64).float()
    invstd = (torch.rand(n, generator=g, dtype=torch.float64) + 0.5).float()
    a[0] = 0.0                                                    # a gamma = 0 channel
    if n >= 3:
        sums[:, n - 1], sums[:, 2 * n - 1] = 0.0, 0.0               # all-zero sums
    return sums, a, mean, invstd


@pytest.mark.parametrize("train", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("stripes,sdt", [(32, torch.float64), (9, torch.float32), (1, torch.float64)], ids=["s32-f64", "s9-f32", "s1-f64"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_bn_bwd_coeffs(n, stripes, sdt, train):
    """ly_bn_bwd_coeffs against float64: dgamma / dbeta returned, and ADDED into non-zero targets; alpha, kappa, lambda (kappa = lambda = 0
    with train = 0); a gamma = 0 channel, all-zero sums"""
    from lead_yolo_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(7 * n + stripes + train)
    count = 777.0
    sums, a, mean, invstd = _coeff_case(n, stripes, sdt, g)
    s1, s2 = R.fold(sums)
    dev_args = (sums.to(dev), n, count, a.to(dev), mean.to(dev), invstd.to(dev), bool(train))
    dg, db, al, ka, la = ops.bn_bwd_coeffs(*dev_args)
    torch.cuda.synchronize()
    want = R.coeffs(s1, s2, count, R.d(a), R.d(mean), R.d(invstd), train)
    R.judge_coeffs(dict(dgamma=dg, dbeta=db, alpha=al, kappa=ka, lam=la), want, f"coeffs n={n}")
    if not train:
        assert float(ka.abs().max()) == 0.0 and float(la.abs().max()) == 0.0
    assert float(al[0]) == 0.0 and float(ka[0].abs()) == 0.0 and float(la[0].abs()) == 0.0          # gamma = 0
    tg0, tb0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    tg, tb = tg0.to(dev), tb0.to(dev)
    r = ops.bn_bwd_coeffs(*dev_args, dgamma=tg, dbeta=tb)
    torch.cuda.synchronize()
    assert r[0] is None and r[1] is None
    want = R.coeffs(s1, s2, count, R.d(a), R.d(mean), R.d(invstd), train, R.d(tg0), R.d(tb0))
    R.judge_coeffs(dict(dgamma=tg, dbeta=tb, alpha=r[2], kappa=r[3], lam=r[4]), want, f"coeffs n={n} into targets")
    if n >= 3:
        assert float(tg[n - 1]) == float(tg0[n - 1]) and float(tb[n - 1]) == float(tb0[n - 1])        # zero sums add nothing


def test_bn_bwd_coeffs_transposed_targets_against_formula():
    """tr_a, tr_b = 9, 40 (RFCBAMConv's generate BatchNorm): sums in [tap][channel] order, dgamma / dbeta ADDED into [channel][tap] targets —
    against the float64 formula, not against another launch"""
    from lead_yolo_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(2)
    kk, c, count = 9, 40, 777.0
    n = kk * c
    sums, a, mean, invstd = _coeff_case(n, R.STRIPES, torch.float64, g)
    tg0, tb0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    tg, tb = tg0.to(dev), tb0.to(dev)
    r = ops.bn_bwd_coeffs(sums.to(dev), n, count, a.to(dev), mean.to(dev), invstd.to(dev), True, dgamma=tg, dbeta=tb, transpose=(kk, c))
    torch.cuda.synchronize()
    tr = lambda t: t.view(kk, c).t().reshape(-1)                 # [tap][channel] -> [channel][tap]
    itr = lambda t: t.view(c, kk).t().reshape(-1)
    want = R.coeffs(*R.fold(sums), count, R.d(a), R.d(mean), R.d(invstd), 1, itr(R.d(tg0)), itr(R.d(tb0)))
    R.judge_coeffs(dict(alpha=r[2], kappa=r[3], lam=r[4]), want, "coeffs transposed")
    R.judge_vec(tg, tr(want["dgamma"]), tr(want["mag"]["dgamma"]), "coeffs transposed dgamma")
    R.judge_vec(tb, tr(want["dbeta"]), tr(want["mag"]["dbeta"]), "coeffs transposed dbeta")


@pytest.mark.parametrize("stripes,sdt", [(32, torch.float64), (9, torch.float32)], ids=["s32-f64", "s9-f32"])
@pytest.mark.parametrize("c_half", [1, 33, 64, 65])
def test_bn_bwd_coeffs_pair(c_half, stripes, sdt):
    """ly_bn_bwd_coeffs_pair against float64 per unit; unit 2's sums are 100 x unit 1's, the targets are non-zero"""
    from lead_yolo_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(13 * c_half + stripes)
    count = 1351.0
    units = [_coeff_case(c_half, stripes, sdt, g, scale=s) for s in (1.0, 100.0)]
    v = torch.zeros(4, 2 * c_half, dtype=torch.float32)
    for i, (_, a, mean, invstd) in enumerate(units):
        sl = slice(i * c_half, (i + 1) * c_half)
        v[0, sl], v[2, sl], v[3, sl] = a, mean, invstd
    t0 = [torch.randn(c_half, generator=g) for _ in range(4)]
    t = [x.to(dev) for x in t0]
    coef = torch.empty(3, 2 * c_half, dtype=torch.float32, device=dev)
    ops.bn_bwd_coeffs_pair(units[0][0].to(dev), units[1][0].to(dev), c_half, count, v.to(dev), ((t[0], t[1]), (t[2], t[3])), coef)
    torch.cuda.synchronize()
    for i, (sums, a, mean, invstd) in enumerate(units):
        sl = slice(i * c_half, (i + 1) * c_half)
        want = R.coeffs(*R.fold(sums), count, R.d(a), R.d(mean), R.d(invstd), 1, R.d(t0[2 * i]), R.d(t0[2 * i + 1]))
        R.judge_coeffs(dict(dgamma=t[2 * i], dbeta=t[2 * i + 1], alpha=coef[0, sl], kappa=coef[1, sl], lam=coef[2, sl]), want, f"coeffs_pair unit {i}")


# ---------------------------------------------------------------- sums -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=DT_IDS.values())
@pytest.mark.parametrize("rows,c", [(37, 8), (1351, 160), (233, 1024)])
def test_chan_moments_per_channel(rows, c, dtype):
    """ly_chan_moments per channel against float64 with the chain length of its code (tests/bnact_ref.py: moments_chain)"""
    from lead_yolo_amd import ops
    g = torch.Generator().manual_seed(rows + c)
    x = (torch.randn(rows, c, generator=g) * 2 + 0.3).to(dtype)
    st = ops.chan_moments(x.to(_dev()), c, rows, c, striped=True)
    torch.cuda.synchronize()
    s1, s2 = R.fold(st)
    xd, zero, ch = R.d(x), torch.zeros(c, dtype=torch.float64), R.moments_chain(rows, c)
    R.judge_sum(s1, xd.sum(0), ch, xd.abs().sum(0), zero, "moments sum")
    R.judge_sum(s2, (xd * xd).sum(0), ch, (xd * xd).sum(0), zero, "moments sum of squares")


@pytest.mark.parametrize("r", R.SUM_ROWS_R)
def test_sum_rows(r):
    """ops.sum_rows against float64 per column: 4 vs 16 row lanes (R <= 192), the 8 / 4 / 1-row loops with and without tails, column counts
    around the 64-column block; accumulate on and off over a non-zero destination; the same bits from two calls"""
    from lead_yolo_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(r)
    for c in R.SUM_ROWS_C:
        t = torch.randn(r, c, generator=g)
        d0 = torch.randn(c, generator=g)
        td = t.to(dev)
        want, mag, zero, ch = R.d(t).sum(0), R.d(t).abs().sum(0), torch.zeros(c, dtype=torch.float64), R.sum_rows_chain(r)
        out = ops.sum_rows(td)
        again = ops.sum_rows(td, out=d0.to(dev))                    # accumulate off: the destination's old value is gone
        acc = ops.sum_rows(td, out=d0.to(dev), accumulate=True)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (c,)
        R.judge_sum(out, want, ch, mag, zero, f"sum_rows R={r} C={c}")
        assert torch.equal(out, again), f"sum_rows R={r} C={c}: two calls differ"
        R.judge_sum(acc, want + R.d(d0), ch, mag + R.d(d0).abs(), zero, f"sum_rows R={r} C={c} accumulate")


# ---------------------------------------------------------------- the whole chain ------------------------------------------------------------
def _judge_chain(got, ref, ci, rows, c, bf, what):
    ratios = dict(y=R.judge_channels(got["y"], ref["y"], what + " y", bf16=bf), du=R.judge_channels(got["du"], ref["du"], what + " du", bf16=bf),
                  dgamma=R.judge_channels(got["dgamma"], ref["dgamma"], what + " dgamma", floor=ref["floor_g"]),
                  dbeta=R.judge_channels(got["dbeta"], ref["dbeta"], what + " dbeta", floor=ref["floor_b"]))
    # running statistics: the coefficient bound on top of the statistics pass's own (fp32 partial sums of moments_chain terms)
    k = (R.moments_chain(rows, c) + R.K_VEC) * R.U24
    R.judge_channels(got["rm"], ref["rm"], what + " running_mean", floor=k * ref["mag"]["rm"])
    ud = R.d(ci["u"])
    R.judge_channels(got["rv"], ref["rv"], what + " running_var", floor=k * (ref["mag"]["rv"] + 2 * ci["momentum"] * (ud * ud).mean(0)))
    return ratios


@pytest.mark.parametrize("act", [R.ACT_SILU, R.ACT_RELU], ids=["silu", "relu"])
@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=DT_IDS.values())
@pytest.mark.parametrize("rows,c", R.CHAIN_CASES)
def test_chain_against_float64_autograd(rows, c, dtype, act):
    """chan_moments(striped) -> bn_finalize -> bnact_fwd -> bnact_bwd_reduce -> bn_bwd_coeffs(train) -> bnact_bwd_apply, and the pair route
    (bn_finalize_pair / bnact_bwd_reduce_pair / bn_bwd_coeffs_pair / bnact_bwd_apply_pair over the two halves), against F.batch_norm +
    activation under float64 autograd, judged PER CHANNEL; a constant channel, a gamma = 0 channel, a channel dead under ReLU (du exactly 0)"""
    from lead_yolo_amd import ops
    dev = _dev()
    bf = dtype == R.BF16
    ci = R.chain_inputs(rows, c, dtype, act)
    if act == R.ACT_RELU:
        R.assert_no_kink(ci["u"], *R.chain_ab(ci, rows), f"chain {rows}x{c}", R.CHAIN_KINK)
    ref = R.chain_reference(ci, rows, act)
    u, r = ci["u"].to(dev), ci["r"].to(dev)

    def bn_of(sl):
        bn = torch.nn.BatchNorm2d(sl.stop - sl.start, eps=ci["eps"], momentum=ci["momentum"]).train()
        with torch.no_grad():
            bn.weight.copy_(ci["gamma"][sl]); bn.bias.copy_(ci["beta"][sl]); bn.running_mean.copy_(ci["rm"][sl]); bn.running_var.copy_(ci["rv"][sl])
        return bn.to(dev)

    what = f"chain {rows}x{c} {DT_IDS[dtype]} {ACT_IDS[act]}"
    # one unit
    bn = bn_of(slice(0, c))
    stats = ops.chan_moments(u, c, rows, c, striped=True)
    a, b, mean, invstd = ops.bn_finalize(bn, stats, c, rows, want_stats=True)
    y = torch.empty_like(u)
    ops.bnact_fwd(u, c, rows, c, a, b, act, y, c)
    sums = ops.bnact_bwd_reduce(r, c, u, c, rows, c, a, b, act)
    dg, db, al, ka, la = ops.bn_bwd_coeffs(sums, c, rows, a, mean, invstd, True)
    du = torch.empty_like(u)
    ops.bnact_bwd_apply(r, c, u, c, rows, c, a, b, act, al, ka, la, du, c)
    torch.cuda.synchronize()
    got = dict(y=y, du=du, dgamma=dg, dbeta=db, rm=bn.running_mean, rv=bn.running_var)
    ratios = _judge_chain(got, ref, ci, rows, c, bf, what)
    assert int(bn.num_batches_tracked) == 1
    if act == R.ACT_RELU:
        assert float(du[:, 2].abs().max()) == 0.0 and float(y[:, 2].abs().max()) == 0.0, what + ": dead channel"
    assert float(du[:, 1].abs().max()) == 0.0, what + ": gamma = 0 channel"
    # the pair route over the two halves
    h = c // 2
    bns = [bn_of(slice(0, h)), bn_of(slice(h, c))]
    v = torch.empty(4, c, dtype=torch.float32, device=dev)
    ops.bn_finalize_pair(bns[0], bns[1], ops.chan_moments(u, c, rows, c, striped=True), h, rows, v)
    y2 = torch.empty_like(u)
    ops.bnact_fwd(u, c, rows, c, v[0], v[1], act, y2, c)
    r1, r2 = r[:, :h].contiguous(), r[:, h:].contiguous()
    sa, sb = ops.bnact_bwd_reduce_pair(r1, h, r2, h, h, u, c, rows, c, v[0], v[1], act)
    tg = torch.zeros(4, h, dtype=torch.float32, device=dev)
    coef = torch.empty(3, c, dtype=torch.float32, device=dev)
    ops.bn_bwd_coeffs_pair(sa, sb, h, rows, v, ((tg[0], tg[1]), (tg[2], tg[3])), coef)
    du2 = torch.empty_like(u)
    ops.bnact_bwd_apply_pair(r1, h, r2, h, h, u, c, rows, c, v[0], v[1], act, coef[0], coef[1], coef[2], du2, c)
    torch.cuda.synchronize()
    got = dict(y=y2, du=du2, dgamma=torch.cat([tg[0], tg[2]]), dbeta=torch.cat([tg[1], tg[3]]),
               rm=torch.cat([bns[0].running_mean, bns[1].running_mean]), rv=torch.cat([bns[0].running_var, bns[1].running_var]))
    _judge_chain(got, ref, ci, rows, c, bf, what + " pair")
    assert int(bns[0].num_batches_tracked) == 1 and int(bns[1].num_batches_tracked) == 1
    print(f"{what}: worst per-channel err / max|ref|  " + "  ".join(f"{k} {val:.2e}" for k, val in ratios.items()))


# ---------------------------------------------------------------- grad.affine_backward -------------------------------------------------------
def _affine_case(n, c, h, w, dtype, act, train, dev):
    rows = n * h * w
    ci = R.chain_inputs(rows, c, dtype, act)
    ud, rd = R.d(ci["u"]), R.d(ci["r"])
    g64, b64 = R.d(ci["gamma"]), R.d(ci["beta"])
    if train:
        f = R.finalize(ud.sum(0), (ud * ud).sum(0), float(rows), g64, b64, ci["eps"], ci["momentum"])
        mean, invstd = f["mean"], f["invstd"]
        ref = R.chain_autograd(ud, g64, b64, ci["eps"], act, rd)
    else:
        mean, rv = R.d(ci["rm"]) * 0.3, R.d(ci["rv"])
        invstd = 1 / torch.sqrt(rv + ci["eps"])
        ref = R.chain_autograd(ud, g64, b64, ci["eps"], act, rd, training=False, rm=mean, rv=rv)
    a, b = g64 * invstd, b64 - mean * g64 * invstd
    if act == R.ACT_RELU:
        R.assert_no_kink(ci["u"], a, b, "affine_backward", R.CHAIN_KINK)
    nhwc = lambda t: t.view(n, h, w, -1).permute(0, 3, 1, 2)          # NHWC-dense [n, c, h, w]
    floors = R.grad_floors(rd, ud, a, b, act, mean, invstd)          # the sums' own bound under dgamma / dbeta
    dev_co = [t.float().to(dev) for t in (a, b, mean, invstd)]
    return ci, ref, nhwc, dev_co, floors


@pytest.mark.parametrize("variant", ["inplace", "fresh", "out-is-dy", "dy-slice", "eval", "sink"])
@pytest.mark.parametrize("act", [R.ACT_SILU, R.ACT_RELU], ids=["silu", "relu"])
@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=DT_IDS.values())
@pytest.mark.parametrize("shape", [(2, 40, 7, 13), (1, 160, 20, 20)], ids=["2x40x7x13", "1x160x20x20"])
def test_affine_backward(shape, dtype, act, variant, monkeypatch):
    """grad.affine_backward (reduce -> coefficients -> apply) on an NHWC-dense [n, c, h, w] pair against float64 autograd: du over u, into a
    fresh tensor, over dy; dy a channel slice of a wider gradient; an eval-mode BatchNorm; a gradient sink holding gamma / beta"""
    from lead_yolo_amd import grad
    n, c, h, w = shape
    dev = _dev()
    train = variant != "eval"
    ci, ref, nhwc, (a, b, mean, invstd), (floor_g, floor_b) = _affine_case(n, c, h, w, dtype, act, train, dev)
    u = nhwc(ci["u"].to(dev))
    if variant == "dy-slice":
        vw = _vw(dtype)
        wide = torch.full((n * h * w, c + 2 * vw), SENTINEL, dtype=dtype, device=dev)
        wide[:, vw:vw + c] = ci["r"].to(dev)
        dy, lddy = nhwc(wide)[:, vw:vw + c], c + 2 * vw
    else:
        dy, lddy = nhwc(ci["r"].to(dev)), None
    kw = dict(inplace=variant == "inplace", lddy=lddy)
    if variant == "out-is-dy":
        kw.update(inplace=False, out=dy)
    bn = None
    if variant == "sink":
        from tests.test_gpu_backward import _sink_on
        bn = torch.nn.BatchNorm2d(c).to(dev)
        _sink_on(bn, monkeypatch)
        kw.update(gamma=bn.weight, beta=bn.bias)
    u0 = u.clone()
    du, dg, db = grad.affine_backward(dy, u, a, b, act, mean, invstd, train, **kw)
    torch.cuda.synchronize()
    if variant == "inplace":
        assert du.data_ptr() == u.data_ptr()
    else:
        assert torch.equal(u, u0), "u was saved for backward and must keep its bits"
    if variant == "out-is-dy":
        assert du.data_ptr() == dy.data_ptr()
    if variant == "sink":
        assert dg is None and db is None
        dg, db = bn.weight.grad, bn.bias.grad
    bf = dtype == R.BF16
    what = f"affine_backward {shape} {DT_IDS[dtype]} {ACT_IDS[act]} {variant}"
    got_du = du.permute(0, 2, 3, 1).reshape(n * h * w, c)
    R.judge_channels(got_du, ref[1], what + " du", bf16=bf)
    R.judge_channels(dg, ref[2], what + " dgamma", floor=floor_g)
    R.judge_channels(db, ref[3], what + " dbeta", floor=floor_b)


# ---------------------------------------------------------------- refusals -------------------------------------------------------------------
def test_refusals():
    """argument checks that return before any launch: C no multiple of 4, a leading dimension no multiple of 4, the reduce pass beyond 1024
    channels"""
    from lead_yolo_amd import capi, ops
    dev = _dev()
    u = torch.zeros(4, 1040, device=dev)
    co = torch.ones(1040, device=dev)
    y = torch.zeros(4, 1040, device=dev)
    with pytest.raises(capi.HipLibraryError):
        ops.bnact_fwd(u, 8, 4, 6, co, co, R.ACT_SILU, y, 8)
    with pytest.raises(capi.HipLibraryError):
        ops.bnact_fwd(u, 10, 4, 8, co, co, R.ACT_SILU, y, 8)
    with pytest.raises(capi.HipLibraryError):
        ops.bnact_bwd_apply(u, 8, u, 10, 4, 8, co, co, R.ACT_SILU, co, co, co, y, 8)
    with pytest.raises(capi.HipLibraryError):
        ops.bnact_bwd_reduce(u, 1028, u, 1028, 4, 1028, co, co, R.ACT_SILU)
    with pytest.raises(capi.HipLibraryError):
        ops.bnact_bwd_reduce(u, 8, u, 8, 4, 6, co, co, R.ACT_SILU)
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0
