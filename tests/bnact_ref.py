"""Float64 reference, judges, input builders and case tables for the train-mode BatchNorm + activation kernel chain

    ly_chan_moments -> ly_bn_finalize(_pair) -> ly_bnact_fwd
    ly_bnact_bwd_reduce(_pair) -> ly_bn_bwd_coeffs(_pair) -> ly_bnact_bwd_apply(_pair)          (+ ly_sum_rows)

(csrc/ly_bnact.hip; ly_sum_rows in csrc/ly_backward.hip).  A plain helper module: tests/test_bnact_host.py (CPU) and tests/test_gpu_bnact.py (device)
import the SAME references, judges, builders and case tables from here.

References take the stored values — the fp32 / bf16 tensors a kernel is given — widened exactly to float64, and restate the operation in
plain torch float64 on the CPU.  Judges raise AssertionError; nothing here compares a kernel with itself.

Bounds (u24 = 2^-24, one fp32 rounding of a value of magnitude 1)

  elementwise (fwd, apply)   |got - want| <= K_ELEM * u24 * M + 2^-126 * U [+ 2^-8 |want| when the result is stored as bf16]
      (2^-8 is bf16's unit roundoff: 8 significant bits.  Half of it, 2^-9, is NOT met by the float64 result rounded to bf16 — 28 % of the
      elements of a (4099, 64) result exceed it, tests/test_bnact_host.py — so it cannot be the storage term.)
      M is the sum of the magnitudes of the terms with the cancelling inner factor taken by absolute value:
        M_apply = |alpha dy| D + |kappa| + |lambda u|,  D = s (1 + |v| (1 - s)) (1 + |v|) for SiLU, [v > 0] for ReLU, 1 for none
        M_fwd   = (|a u| + |b|) D',                     D' = s (1 + |v| (1 - s)) for SiLU (|dy/dv| with the inner factor by magnitude), else 1
      U is the fp32 underflow term: fp32 holds no sigmoid below 2^-126 (at v = -90 the true s is 8e-40 and the kernel's, correctly, 0), so
      2^-126 (1 + |v|) times the factor that multiplies s (|alpha dy| (1 + |v|), resp. 1) is allowed on top.  It is ~1e-34 here: it decides
      nothing but the v = -90 elements.
      K_ELEM: torch's own float32 evaluation of the two references on the CPU, against float64, over every elementwise and pair case of
      ELEM_CASES / PAIR_CASES x three activations (measure_k below; tests/test_bnact_host.py re-measures and holds it under K_ELEM / 4):
        worst ratio  apply 5.35, fwd 3.48  (units of u24 * M)   ->   K_ELEM = 4 * 5.35 = 21.4, taken as 22
      (factor 4: v_exp_f32 / v_rcp_f32 at <= 1 ulp each, __expf's error growing with |v|, fused vs separate multiply-add.)

  sums (reduce, chan_moments, sum_rows)   per channel  |got - want| <= u24 * (L * sum_r |term_r| + K_ELEM * sum_r M_r)
      L is the longest fp32 addition chain, from the code:
        reduce        rows per row lane and block + the `groups` fold of the block (LDS) — reduce_chain(rows, C): blocks =
                      ceil(rows / (groups * 32)) capped at 2048, rounded up to a multiple of 8 from 8 on; an XCD eighth of ceil(rows / 8)
                      rows is walked by blocks / 8 blocks, `groups` rows per trip.  The stripes are added as doubles (no fp32 rounding).
        chan_moments  ceil(rows / (groups * blocks)) rows per lane with blocks = ceil(rows / (groups * 16)) capped at 2048, + groups
        sum_rows      ceil(ceil(R / rls) / 4) per accumulator (four accumulators per row lane) + 2 (the accumulator tree) + rls (lane fold)
                      + 1 (accumulate), rls = 4 for R <= 192 else 16
      The second summand is the terms' own roundings (their fp32 underflow at v = -90 included, as above): a term dv (or dv u) carries the elementwise error K_ELEM u24 M_r with
      M_r = |dy| D (|u|); moments and sum_rows terms are exact or one rounding (x^2), which 1 more unit of L covers.
      Reference-only figure: a plain fp32 sum of dv (torch, CPU) against float64 is within 1.0 units of u24 * sum|dv| at (4099, 64).

  per-channel vectors (finalize, coeffs)   4 * u24 * (sum of the magnitudes of the terms of that output), e.g. |beta| + |mean scale| for
      shift, |a s1 / count| + |lambda mu| for kappa: every output is a few fp32 roundings of double intermediates.

  ReLU kink   elements with |v64| <= 2^-22 (|a u| + |b|) are undecidable (the kernel's fp32 a u + b is within ~1 ulp of the terms); the
      builders nudge such elements out (u +- 2^-10 (|u| + |b / a|), at least one step of the storage type) and every test asserts that NO
      element of its input is in the band: the cap on excluded elements is zero, nothing is masked.  Exact zeros (u = 0, b = 0) are a
      separate deliberate case: dv = 0.

  whole chain against float64 autograd   per channel  max_r |err[:, c]| <= CHAIN_TOL * max_r |ref[:, c]| [+ 2^-8 max_r|ref| for bf16 tensors]
      CHAIN_TOL: chain_autograd run in float32 on the CPU against float64 over CHAIN_CASES x (SiLU, ReLU) (measure_chain_tol):
        worst per-channel ratio 5.2e-7 (du), 4.6e-7 (y); dgamma, dbeta inside their floor (3.9e-7, 3.0e-7 of max(|ref|, floor))
        ->   CHAIN_TOL = 4 * 5.2e-7 = 2.1e-6  (<= 1e-4)
      dgamma / dbeta (one number per channel, a sum that may cancel to ~0 and then cannot be relative to itself) are bounded by
      max(CHAIN_TOL |ref|, (reduce_chain + K_ELEM) u24 sum_r |term_r|): the sums' own bound as the floor, with dgamma's terms those of
      (s2 - mean s1) invstd, the form the coefficient kernel computes.
"""
import math

import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_SILU = 0, 1, 2          # the C ABI's codes (tests/test_gpu_bnact.py holds them to lead_yolo_amd.ops)
ACTS = (ACT_NONE, ACT_RELU, ACT_SILU)
U24 = 2.0 ** -24
BF16_EPS = 2.0 ** -8                             # unit roundoff of bf16 (8 significant bits, round to nearest)
TINY = 2.0 ** -126
K_ELEM = 22.0
K_VEC = 4.0
KINK = 2.0 ** -22
CHAIN_KINK = 2.0 ** -19                          # a, b of the chain are the kernel's own: each within 4 u24 of its terms, v within ~9 u24 of (|a u| + |b|)
CHAIN_TOL = 2.1e-6
STRIPES = 32
THREADS = 256
RED_ROWS = 32


def d(t):
    """a stored tensor widened exactly to float64 on the CPU"""
    return t.detach().to("cpu").to(torch.float64)


# ---------------------------------------------------------------- references -------------------------------------------------------------
def act_fn(v, act):
    if act == ACT_RELU:
        return torch.clamp(v, min=0.0)
    if act == ACT_SILU:
        return v * torch.sigmoid(v)
    return v


def dact(v, dy, act):
    if act == ACT_RELU:
        return dy * (v > 0).to(dy.dtype)
    if act == ACT_SILU:
        s = torch.sigmoid(v)
        return dy * s * (1 + v * (1 - s))
    return dy


def _dmag(v, act, outer):
    """conditioned magnitude of act'(v): the cancelling factor 1 + v (1 - s) by absolute value; outer: times (1 + |v|) (errors of v and of s)"""
    if act == ACT_RELU:
        return (v > 0).to(v.dtype)
    if act == ACT_SILU:
        s = torch.sigmoid(v)
        m = s * (1 + v.abs() * (1 - s))
        return m * (1 + v.abs()) if outer else m
    return torch.ones_like(v)


def fwd(u, a, b, act):
    return act_fn(a * u + b, act)


def fwd_mag(u, a, b, act):
    """(M_fwd, underflow term)"""
    v = a * u + b
    t = (a * u).abs() + b.abs()
    return t * _dmag(v, act, False), (TINY * (1 + v.abs()) if act == ACT_SILU else torch.zeros_like(v))


def reduce(dy, u, a, b, act):
    dv = dact(a * u + b, dy, act)
    return dv.sum(0), (dv * u).sum(0)


def reduce_mag(dy, u, a, b, act):
    """per channel: (sum |dv|, sum |dv u|) with the inner factor by magnitude, and the same with the terms' conditioned magnitudes M_r"""
    v = a * u + b
    t = dy.abs() * _dmag(v, act, False)
    m = dy.abs() * _dmag(v, act, True)
    if act == ACT_SILU:                                 # the terms' fp32 underflow (see apply_mag), ~1e-34: in units of u24 it joins M
        m = m + TINY * dy.abs() * (1 + v.abs()) ** 2 / U24
    return (t.sum(0), (t * u.abs()).sum(0)), (m.sum(0), (m * u.abs()).sum(0))


def apply(dy, u, a, b, act, alpha, kappa, lam):
    return alpha * dact(a * u + b, dy, act) + kappa + lam * u


def apply_mag(dy, u, a, b, act, alpha, kappa, lam):
    v = a * u + b
    m = (alpha * dy).abs() * _dmag(v, act, True) + kappa.abs() + (lam * u).abs()
    uf = TINY * (alpha * dy).abs() * (1 + v.abs()) ** 2 if act == ACT_SILU else torch.zeros_like(v)
    return m, uf


def fold(stats):
    """[stripes][2n] -> (s1, s2), stripes added in index order in float64"""
    st = d(stats)
    if st.dim() == 1:
        st = st.view(1, -1)
    acc = torch.zeros(st.shape[1], dtype=torch.float64)
    for k in range(st.shape[0]):
        acc = acc + st[k]
    n = st.shape[1] // 2
    return acc[:n], acc[n:]


def finalize(s1, s2, count, gamma, beta, eps, momentum, rm=None, rv=None, nbt=0, biased=False):
    """ly_bn_finalize: dict(scale, shift, mean, invstd, rm, rv, nbt) and `mag`, the per-output sums of term magnitudes.  The unbiased variance is
    var count / max(count - 1, 1), the variance is clamped at 0 (the kernel's header comment).  biased=True is the DEFECT the host tests plant."""
    m = s1 / count
    var = torch.clamp(s2 / count - m * m, min=0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - m * scale
    out = dict(scale=scale, shift=shift, mean=m, invstd=invstd, nbt=nbt + 1)
    mag = dict(scale=scale.abs(), shift=beta.abs() + (m * scale).abs(), mean=m.abs(), invstd=invstd.abs())
    if rm is not None:
        unb = var if biased else var * (count / max(count - 1.0, 1.0))
        out["rm"] = (1 - momentum) * rm + momentum * m
        out["rv"] = (1 - momentum) * rv + momentum * unb
        mag["rm"] = ((1 - momentum) * rm).abs() + (momentum * m).abs()
        mag["rv"] = ((1 - momentum) * rv).abs() + abs(momentum) * unb
    out["mag"] = mag
    # E[x^2] - E[x]^2 is formed in double: its own rounding, 2^-53 of the two terms, is all that is left of a constant channel's variance
    out["abs"] = dict(rv=8 * 2.0 ** -53 * abs(momentum) * (s2 / count + m * m) * (count / max(count - 1.0, 1.0))) if rm is not None else {}
    return out


def coeffs(s1, s2, count, a, mean, invstd, train, dg0=None, db0=None):
    """ly_bn_bwd_coeffs: dict(dgamma, dbeta, alpha, kappa, lam) (+ `mag`); dgamma / dbeta are ADDED to dg0 / db0"""
    dg = (s2 - mean * s1) * invstd
    z = torch.zeros_like(s1)
    dg0 = z if dg0 is None else dg0
    db0 = z if db0 is None else db0
    lam = -a * dg * invstd / count
    kappa = -a * s1 / count - lam * mean
    mag = dict(dgamma=dg0.abs() + (s2.abs() + (mean * s1).abs()) * invstd.abs(), dbeta=db0.abs() + s1.abs(), alpha=a.abs(), lam=lam.abs(),
               kappa=(a * s1 / count).abs() + (lam * mean).abs())
    if not train:
        lam, kappa = z.clone(), z.clone()
    return dict(dgamma=dg0 + dg, dbeta=db0 + s1, alpha=a.clone(), kappa=kappa, lam=lam, mag=mag)


def chain_autograd(u, gamma, beta, eps, act, r, dtype=torch.float64, training=True, rm=None, rv=None):
    """F.batch_norm + activation under autograd, loss = sum(y r): (y, du, dgamma, dbeta).  u, r: [rows, C]"""
    u = u.to(dtype).clone().requires_grad_(True)
    g = gamma.to(dtype).clone().requires_grad_(True)
    be = beta.to(dtype).clone().requires_grad_(True)
    rm = None if rm is None else rm.to(dtype).clone()
    rv = None if rv is None else rv.to(dtype).clone()
    y = act_fn(F.batch_norm(u, rm, rv, g, be, training, 0.0, eps), act)
    (y * r.to(dtype)).sum().backward()
    return y.detach(), u.grad, g.grad, be.grad


# ---------------------------------------------------------------- judges ------------------------------------------------------------------
def _fail(what, err, bound, extra=""):
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    i = int(torch.argmax(ratio))
    idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ratio.shape)) if ratio.dim() else ()
    raise AssertionError(f"{what}: |got - want| = {float(err.flatten()[i]):.4e} > bound {float(bound.flatten()[i]):.4e} at {idx} "
                         f"(x{float(ratio.flatten()[i]):.2f}; {int((err > bound).sum())} of {err.numel()} over) {extra}")


def _ratio(err, m, uf):
    """worst err / (u24 M), the underflow allowance taken off first"""
    return float(((err - uf).clamp(min=0.0) / (U24 * m).clamp(min=1e-300))[m > 0].max()) if bool((m > 0).any()) else 0.0


def judge_elem(got, want, mag, what, bf16=False, k=K_ELEM):
    """elementwise result against float64; mag = (M, underflow) of fwd_mag / apply_mag.  Returns, for the record, the worst ratio of what is left
    of the error after the underflow and storage allowances to u24 M."""
    got = d(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    m, uf = mag
    err = (got - want).abs()
    bound = k * U24 * m + uf + (BF16_EPS * want.abs() if bf16 else 0.0)
    if bool((err > bound).any()):
        _fail(what, err, bound)
    return _ratio(err - (BF16_EPS * want.abs() if bf16 else 0.0), m, uf)


def judge_sum(got, want, chain, term_abs, term_mag, what, k=K_ELEM):
    """per-channel sum against float64: u24 (chain * sum|term| + k * sum M)"""
    got = d(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    err = (got - want).abs()
    bound = U24 * (chain * term_abs + k * term_mag)
    if bool((err > bound).any()):
        _fail(what, err, bound, f"chain = {chain}")


def judge_vec(got, want, mag, what, k=K_VEC, extra=0.0):
    """per-channel vector of a coefficient kernel: k u24 (sum of the magnitudes of the output's terms) [+ extra: an absolute allowance]"""
    got = d(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    err = (got - want).abs()
    bound = k * U24 * mag + extra
    if bool((err > bound).any()):
        _fail(what, err, bound)


def judge_finalize(got, want, what):
    """got: dict of the kernel's outputs (any subset of scale, shift, mean, invstd, rm, rv) and nbt"""
    for key, val in got.items():
        if key == "nbt":
            assert int(val) == int(want["nbt"]), f"{what}: num_batches_tracked {int(val)} != {int(want['nbt'])}"
        else:
            judge_vec(val, want[key], want["mag"][key], f"{what} {key}", extra=want["abs"].get(key, 0.0))


def judge_coeffs(got, want, what):
    for key, val in got.items():
        judge_vec(val, want[key], want["mag"][key], f"{what} {key}")


def judge_channels(got, want, what, tol=CHAIN_TOL, bf16=False, floor=None):
    """whole-chain judge, per channel (last dim): max_r |err| <= max(tol max_r |ref|, floor) [+ 2^-8 max_r |ref|]; floor: an absolute bound per
    channel (the sums' own bound for dgamma / dbeta).  Returns the worst ratio (err - floor) / max_r |ref| for the record."""
    got = d(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    err, ref = (got - want).abs(), want.abs()
    if got.dim() == 2:
        err, ref = err.amax(0), ref.amax(0)
    bound = tol * ref
    if floor is not None:
        bound = torch.maximum(bound, floor)
    bound = bound + (BF16_EPS * ref if bf16 else 0.0)
    if bool((err > bound).any()):
        _fail(what, err, bound)
    over = (err - (0.0 if floor is None else floor) - (BF16_EPS * ref if bf16 else 0.0)).clamp(min=0.0)
    return float((over / ref.clamp(min=1e-300))[ref > 0].max())


def in_band(u, a, b, width=KINK):
    v = a * u + b
    t = (a * u).abs() + b.abs()
    return (v.abs() <= width * t) & (t > 0)


def assert_no_kink(u, a, b, what, width=KINK):
    """the ReLU premise: NO element of the input is undecidable (exact zeros u = 0, b = 0 are decided: dv = 0)"""
    n = int(in_band(d(u), d(a), d(b), width).sum())
    assert n == 0, f"{what}: {n} elements inside the ReLU kink band"


# ---------------------------------------------------------------- chain lengths -----------------------------------------------------------
def reduce_chain(rows, c):
    groups = THREADS // (c // 4)
    blocks = min(max(-(-rows // (groups * RED_ROWS)), 1), 2048)
    if blocks >= 8:
        blocks = (blocks + 7) // 8 * 8
        span, nb = -(-rows // 8), blocks // 8
    else:
        span, nb = rows, blocks
    return -(-span // (groups * nb)) + groups


def moments_chain(rows, c):
    groups = THREADS // (c // 4)
    blocks = min(max(-(-rows // (groups * 16)), 1), 2048)
    return -(-rows // (groups * blocks)) + groups + 1


def sum_rows_chain(r):
    rls = 4 if r <= 192 else 16
    return -(-(-(-r // rls)) // 4) + 2 + rls + 1


# ---------------------------------------------------------------- input builders ----------------------------------------------------------
def nudge(u, a, b, dtype, width=KINK):
    """moves the elements of u (stored as dtype) that lie in the ReLU kink band out of it; returns (u, moved)"""
    moved = 0
    for _ in range(6):
        ud, ad, bd = d(u), d(a), d(b)
        band = in_band(ud, ad, bd, width)
        n = int(band.sum())
        if n == 0:
            break
        moved += n
        step = 2.0 ** -10 * (ud.abs() + (bd / torch.where(ad == 0, torch.ones_like(ad), ad)).abs())
        ulp = ud.abs() * (2.0 ** -6 if dtype == torch.bfloat16 else 2.0 ** -21) + 1e-30
        cand = ud + torch.sign(ad * ud + bd + 1e-300) * torch.maximum(step, ulp)
        u = torch.where(band, cand, ud).to(dtype)
    return u, moved


# elementwise cases: id -> (rows, C, ldu, lddy, ldo, dtypes, with_reduce).  Offsets of the channel-slice views: one 16-byte vector (what
# ops.rows admits: data_ptr % 16 == 0, ld % vw == 0) whenever ld > C and the row stride is itself a multiple of the vector.
F32, BF16 = torch.float32, torch.bfloat16
ELEM_CASES = {}
for _c in (8, 24, 160, 1024):
    for _r in (1, 7, 8, 9, 37):
        ELEM_CASES[f"lanes-c{_c}-r{_r}"] = (_r, _c, _c, _c, _c, (F32, BF16), True)
ELEM_CASES.update({
    "xcd-off-c160-r1344": (1344, 160, 160, 160, 160, (F32, BF16), True),
    "xcd-on-c160-r1351": (1351, 160, 160, 160, 160, (F32, BF16), True),
    "xcd-off-c1024-r224": (224, 1024, 1024, 1024, 1024, (F32, BF16), True),
    "xcd-on-c1024-r233": (233, 1024, 1024, 1024, 1024, (F32, BF16), True),
    "fallback-bf16-c12-r37": (37, 12, 12, 12, 12, (BF16,), True),
    "fallback-bf16-c20-r37": (37, 20, 20, 20, 20, (BF16,), True),
    "fallback-bf16-c16-ld20": (37, 16, 20, 20, 20, (BF16,), True),
    "fallback-f32-c1028": (9, 1028, 1028, 1028, 1028, (F32,), False),
    "fallback-bf16-c12-r2500-xcdrange": (2500, 12, 12, 12, 12, (BF16,), True),
    "ld-u-c160": (37, 160, 176, 160, 160, (F32, BF16), True),
    "ld-dy-c160": (37, 160, 160, 176, 160, (F32, BF16), True),
    "ld-out-c160": (37, 160, 160, 160, 176, (F32, BF16), True),
    "ld-all-c24": (9, 24, 40, 48, 32, (F32, BF16), True),
})
# pair cases: id -> (rows, C, csplit, lddy1, lddy2, dtypes)
PAIR_CASES = {
    "pair-half-c16": (300, 16, 8, 8, 8, (F32, BF16)),
    "pair-half-c80": (300, 80, 40, 40, 40, (F32, BF16)),
    "pair-half-c512": (300, 512, 256, 256, 256, (F32, BF16)),
    "pair-8-of-40": (300, 40, 8, 8, 32, (F32, BF16)),
    "pair-32-of-40": (300, 40, 32, 32, 8, (F32, BF16)),
    "pair-20-of-40-fallback": (300, 40, 20, 20, 20, (BF16, F32)),
    "pair-ld-differ-c80": (37, 80, 40, 56, 48, (F32, BF16)),
}
CHAIN_CASES = [(37, 8), (1351, 160), (233, 1024), (4099, 64)]
SUM_ROWS_R = (1, 3, 4, 7, 8, 31, 32, 33, 192, 193, 1000)
SUM_ROWS_C = (1, 63, 64, 65, 4000)


def _seed(*key):
    s = 17
    for k in key:
        s = (s * 1000003 + (hash(k) if not isinstance(k, str) else sum(ord(ch) * (i + 1) for i, ch in enumerate(k)))) % (2 ** 31 - 1)
    return s


def elem_inputs(case_id, rows, c, dtype, act, scale2=None):
    """the operands of one elementwise / reduce / pair case, as stored: u, dy [rows, C] in `dtype`; a, b, alpha, kappa, lam fp32 [C].
    Plain draws (u ~ N, a ~ U(0.5, 1.5), b ~ N) plus: |v| up to ~30 on some rows, v = +-90 on a few elements (SiLU's limits), an exact-zero
    column (u = 0, b = 0: ReLU must give dv = 0).  ReLU cases are nudged out of the kink band."""
    g = torch.Generator().manual_seed(_seed(case_id, str(dtype), act))
    u = torch.randn(rows, c, generator=g, dtype=torch.float64)
    dy = torch.randn(rows, c, generator=g, dtype=torch.float64)
    a = (torch.rand(c, generator=g, dtype=torch.float64) + 0.5).float()
    b = torch.randn(c, generator=g, dtype=torch.float64).float()
    alpha = a.clone()
    kappa = (torch.randn(c, generator=g, dtype=torch.float64) * 0.1).float()
    lam = (torch.randn(c, generator=g, dtype=torch.float64) * 0.1).float()
    b[c - 1] = 0.0
    ad, bd = a.double(), b.double()
    # targets for v: every 5th row spans [-30, 30]; rows 0 / last carry +-90 in columns 0, 1
    big = torch.arange(0, rows, 5)
    if len(big):
        t = (torch.rand(len(big), c, generator=g, dtype=torch.float64) * 2 - 1) * 30
        u[big] = (t - bd) / ad
    u[0, 0] = (90.0 - bd[0]) / ad[0]
    u[rows - 1, 1] = (-90.0 - bd[1]) / ad[1]
    u[:, c - 1] = 0.0                                   # the exact-zero column
    if scale2 is not None:                              # pair: the second unit's gradient at another scale
        dy[:, scale2:] *= 100.0
    u, dy = u.to(dtype), dy.to(dtype)
    moved = 0
    if act == ACT_RELU:
        u, moved = nudge(u, a, b, dtype)
    return dict(u=u, dy=dy, a=a, b=b, alpha=alpha, kappa=kappa, lam=lam, moved=moved)


def chain_inputs(rows, c, dtype, act):
    """u, r [rows, C] stored as dtype with |mean| <= std per channel, gamma / beta / running statistics fp32; channel 0 constant (0.5: sums
    exact), channel 1 gamma = 0, channel 2 dead under ReLU (gamma 0.01, beta -5).  ReLU: nudged until no element is in the chain's band
    (the band is taken with the reference's own a, b; the statistics move with the nudge, hence the loop)."""
    g = torch.Generator().manual_seed(_seed("chain", rows, c, str(dtype), act))
    std = torch.rand(c, generator=g, dtype=torch.float64) * 1.5 + 0.5
    mu = (torch.rand(c, generator=g, dtype=torch.float64) * 2 - 1) * std * 0.9
    u = torch.randn(rows, c, generator=g, dtype=torch.float64) * std + mu
    r = torch.randn(rows, c, generator=g, dtype=torch.float64)
    gamma = (torch.rand(c, generator=g, dtype=torch.float64) + 0.5).float()
    beta = (torch.randn(c, generator=g, dtype=torch.float64) * 0.5).float()
    rm = torch.randn(c, generator=g, dtype=torch.float64).float()
    rv = (torch.rand(c, generator=g, dtype=torch.float64) + 0.5).float()
    u[:, 0] = 0.5
    gamma[0], beta[0] = 1.0, 1.0                        # (y = beta + scale (u - mean) with scale = gamma eps^-1/2 = 31.6: judged against |beta| = 1)
    gamma[1] = 0.0
    gamma[2], beta[2] = 0.01, -5.0
    u, r = u.to(dtype), r.to(dtype)
    eps = float(torch.tensor(1e-3, dtype=torch.float32))          # (eps and momentum reach the kernels as floats)
    moved = 0
    if act == ACT_RELU:
        for _ in range(6):
            ud = d(u)
            f = finalize(ud.sum(0), (ud * ud).sum(0), float(rows), gamma.double(), beta.double(), eps, 0.03)
            n = int(in_band(ud, f["scale"], f["shift"], CHAIN_KINK).sum())
            if n == 0:
                break
            u, k = nudge(u, f["scale"].float(), f["shift"].float(), dtype, CHAIN_KINK)
            moved += k
    return dict(u=u, r=r, gamma=gamma, beta=beta, rm=rm, rv=rv, eps=eps, momentum=float(torch.tensor(0.03, dtype=torch.float32)), moved=moved)


def chain_ab(ci, rows):
    """the reference's scale / shift of a chain case (for the band premise)"""
    ud = d(ci["u"])
    f = finalize(ud.sum(0), (ud * ud).sum(0), float(rows), d(ci["gamma"]), d(ci["beta"]), ci["eps"], ci["momentum"])
    return f["scale"], f["shift"]


def grad_floors(dy, u, a, b, act, mean, invstd):
    """the sums' own bound, L u24 sum|term| with L = reduce_chain + K_ELEM, as absolute floors under dgamma = (s2 - mean s1) invstd and
    dbeta = s1: the terms of dgamma are s2 and mean s1 (a constant channel's dgamma is their exact cancellation)"""
    rows, c = u.shape
    unit = (reduce_chain(rows, c) + K_ELEM) * U24
    dv = dy.abs() * _dmag(a * u + b, act, False)
    return ((dv * u.abs()).sum(0) + mean.abs() * dv.sum(0)) * invstd.abs() * unit, dv.sum(0) * unit


def chain_reference(ci, rows, act):
    """float64 autograd of a chain case: dict(y, du, dgamma, dbeta, rm, rv, floor_g, floor_b)"""
    ud, rd = d(ci["u"]), d(ci["r"])
    y, du, dg, db = chain_autograd(ud, d(ci["gamma"]), d(ci["beta"]), ci["eps"], act, rd)
    f = finalize(ud.sum(0), (ud * ud).sum(0), float(rows), d(ci["gamma"]), d(ci["beta"]), ci["eps"], ci["momentum"], d(ci["rm"]), d(ci["rv"]))
    # what the gradients of gamma / beta are sums OF: a channel whose sum cancels is judged against the size of its terms
    floor_g, floor_b = grad_floors(rd, ud, f["scale"], f["shift"], act, f["mean"], f["invstd"])
    return dict(y=y, du=du, dgamma=dg, dbeta=db, rm=f["rm"], rv=f["rv"], mag=f["mag"], floor_b=floor_b, floor_g=floor_g)


# ---------------------------------------------------------------- measurements (reference only) -------------------------------------------
def measure_k(cases=None):
    """worst ratio, in units of u24 M, of torch's float32 evaluation of fwd / apply against float64 over the elementwise and pair cases"""
    worst = dict(fwd=0.0, apply=0.0)
    items = [(k, v[0], v[1], v[5], None) for k, v in ELEM_CASES.items()] + [(k, v[0], v[1], v[5], v[2]) for k, v in PAIR_CASES.items()]
    for cid, rows, c, dts, cs in items:
        if cases is not None and cid not in cases:
            continue
        for dt in dts:
            for act in ACTS:
                x = elem_inputs(cid, rows, c, dt, act, cs)
                f32 = {k: (v.float() if torch.is_tensor(v) else v) for k, v in x.items()}
                f64 = {k: (d(v) if torch.is_tensor(v) else v) for k, v in x.items()}
                m, uf = fwd_mag(f64["u"], f64["a"], f64["b"], act)
                e = (d(fwd(f32["u"], f32["a"], f32["b"], act)) - fwd(f64["u"], f64["a"], f64["b"], act)).abs()
                worst["fwd"] = max(worst["fwd"], _ratio(e, m, uf))
                args = ("dy", "u", "a", "b")
                rest = ("alpha", "kappa", "lam")
                m, uf = apply_mag(*[f64[k] for k in args], act, *[f64[k] for k in rest])
                e = (d(apply(*[f32[k] for k in args], act, *[f32[k] for k in rest])) - apply(*[f64[k] for k in args], act, *[f64[k] for k in rest])).abs()
                worst["apply"] = max(worst["apply"], _ratio(e, m, uf))
    return worst


def measure_chain_tol():
    """worst per-channel ratio of chain_autograd in float32 against float64 over CHAIN_CASES x (SiLU, ReLU) x dtypes"""
    worst = dict(y=0.0, du=0.0, dgamma=0.0, dbeta=0.0)
    # torch's float32 batch-norm reductions split their rows by thread count, and the figures move with it (y: 4.6e-7 on 8 threads, 1.0e-6 on
    # 16): the figures next to CHAIN_TOL are those of 8 threads, so the measurement is taken on 8 wherever it runs
    threads = torch.get_num_threads()
    torch.set_num_threads(8)
    try:
        for rows, c in CHAIN_CASES:
            for dt in (F32, BF16):
                for act in (ACT_SILU, ACT_RELU):
                    ci = chain_inputs(rows, c, dt, act)
                    ref = chain_reference(ci, rows, act)
                    y, du, dg, db = chain_autograd(ci["u"].float(), ci["gamma"], ci["beta"], ci["eps"], act, ci["r"].float(), dtype=torch.float32)
                    worst["y"] = max(worst["y"], judge_channels(y, ref["y"], "y", tol=1.0))
                    worst["du"] = max(worst["du"], judge_channels(du, ref["du"], "du", tol=1.0))
                    worst["dgamma"] = max(worst["dgamma"], judge_channels(dg, ref["dgamma"], "dgamma", tol=1.0, floor=ref["floor_g"]))
                    worst["dbeta"] = max(worst["dbeta"], judge_channels(db, ref["dbeta"], "dbeta", tol=1.0, floor=ref["floor_b"]))
    finally:
        torch.set_num_threads(threads)
    return worst
