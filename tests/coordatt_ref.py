"""Float64 references, judges, input builders and case tables for the CoordAtt kernel chain

    forward   ly_pool_hw -> ly_coordatt_conv1_stats -> (ly_bn_finalize) -> ly_coordatt_mlp -> ly_coordatt_gate
    backward  ly_coordatt_gate_bwd (+ ly_sum_rows) -> ly_coordatt_mlp_bwd (bwd1 + bwd2) -> ly_pool_hw_bwd (accumulating)

(csrc/ly_coordatt.hip; ly_bn_finalize in csrc/ly_bnact.hip; wired together by grad.CoordAttFn).  A plain helper module: tests/test_coordatt_host.py (CPU)
and tests/test_gpu_coordatt.py (device) import the SAME references, judges, builders and case tables from here.  The judges' forms and
`_fail` are those of tests/bnact_ref.py and are imported from there.

References take the stored values — the fp32 / bf16 tensors a kernel is given — widened exactly to float64 and restate
models/common.py:1595-1609 and its derivative in plain torch float64 on the CPU, one function per entry point.  Maps are [n, H, W, C]
(NHWC rows), pooled vectors [n, H + W, C] with the H row positions first.  Nothing here calls a kernel or lead_yolo_amd.ops.

Bounds (u24 = 2^-24)

  elementwise (mlp, gate, gate_bwd's dx, mlp_bwd's dpool, pool_bwd)   |got - want| <= K u24 M [+ 2^-8 |want| for a bf16 result]
      M is the sum of the magnitudes of the terms of the result, every intermediate carried with the magnitudes of ITS terms (`*_mag`):
        gate      |x a_h a_w| + |res|                       pool_bwd  |gp_h| / W + |gp_w| / H + |dx0|
        mlp       a (1 - a) M_z + a,   M_z = |Wx| (1.5 M_y1 + |y2|) + |bx| + (mip + 1) / K (|Wx| |y2| + |bx|)   (z's own chain: see mlp_mag),
                  M_y1 = (|W1| |pool| + |b1|) |sc| + |sh|     (|h_swish'| <= 1.5)
        mlp_bwd   see mlp_bwd_mag: dz, d2 = Wx^T dz, y0, xh, y1, g = d2 h_swish'(y1), S1, S2, dy0, dpool in that order
  sums (pool, conv1_stats, da_h / da_w, the seven parameter gradients)   |got - want| <= u24 (L sum|term| + K sum M_term)
      L is the longest fp32 addition chain, from the code:
        pool_hw       ceil(len / groups) per lane + the `groups` fold (at most min(groups, len)) + 2 (1 / len and the product) — pool_chain
        conv1_stats   positions per wave (grid = ceil(positions / 4) blocks capped at 256, four waves each) + 4 (bias, square, the four-wave
                      fold) — stats_chain.  The per-block sums are added as doubles: no fp32 rounding
        gate_bwd      da_h: 8 columns per thread + the `groups` fold + sum_rows over the slabs; da_w: 8 rows per band + sum_rows over the bands
        mlp_bwd S1/S2 positions per wave of bwd1 (grid = ceil(R / 4) capped at 1024) + 1; the stripes are doubles.  dgamma / dbeta: + 2
        mlp_bwd rest  bwd2: ceil(rows_per_block / 4) per wave (the UR = 4 trips add into one accumulator each) + 3 (four-wave LDS fold)
                      + chunks + 1 (one float atomic per block into the pre-filled target); float64 targets: the atomics add no rounding
  K, per kernel: the SAME references evaluated in torch float32 on the CPU against float64 over every case of the tables (measure_k), the
      worst ratio err / (u24 M) times 4 (v_exp_f32 / v_rcp_f32 at <= 1 ulp each, __expf's error growing with |z|, fused vs separate
      multiply-add), rounded up.  tests/test_coordatt_host.py re-measures and holds 4 x worst <= K:
        worst ratio   y0 4.98   mlp 1.34   gate 2.50   gate_dx 1.93   bwd 2.58 (over g, dy0, y2, dpool)   pool_bwd 2.10
        (y0: the worst of up to 4100 x 16 dot products over C terms; the rigorous bound of such a sum is C + 1)
        K             y0 20     mlp 6      gate 10     gate_dx 8      bwd 11                              pool_bwd 9
  whole chain against float64 autograd (chain_autograd)   per channel  max_r |err| <= max(CHAIN_TOL max_r |ref|, floor) [+ 2^-8 max_r |ref| bf16]
      CHAIN_TOL: chain_autograd in float32 on the CPU against float64 over CHAIN_CASES x (fp32, bf16 operands), on ONE thread (measure_chain_tol:
      torch's float32 reductions split their work by thread count and the figures move with it — with 8 threads the worst is out 9.2e-6; the
      single-thread figures are the largest and the same on every machine):
        worst per-channel ratio  out 3.1e-6  dx 2.2e-6  dW1 5.5e-6  dWh 2.3e-6  dWw 2.2e-5; dgamma, dbeta, dbh, dbw inside their floors
        ->  CHAIN_TOL = 4 * 2.21e-5 = 8.9e-5   (<= 1e-4)
      (out's figure comes from the channels saturated at sigmoid(-20): a = 2e-9 carries the absolute error of its argument as a relative one.)
      dgamma, dbeta, dbh, dbw (sums that may cancel to ~0) take the sums' own bound (L + K) u24 sum |term| as their floor (chain_parts); the
      weight gradients dW1 [mip, C], dWh / dWw [C, mip] are judged per column of the matrix without a floor.  dbh / dbw's floor also holds the
      forward's error of the stored gate factor (a = 1 - 2e-9 is stored as 1: its rounding is all of 1 - a).  A bf16 dx is rounded twice — by
      ly_coordatt_gate_bwd's store and by the accumulating ly_pool_hw_bwd — so 2^-8 max_r |dout a_h a_w| is allowed on top (judge_chain).

  h_swish kinks   h_swish' jumps at y1 = +-3.  Elements with ||y1| - 3| <= KINK M_y1 (KINK = 2^-19: y1 is a dot product over C, a mean, an
      inverse deviation and an affine — each within a few u24 of its terms) are undecidable for the backward; the builders nudge such
      positions out (nudge_pool / chain_inputs) and every test asserts that NO element is in the band: the cap is zero, nothing is masked.
"""
import math

import torch
import torch.nn.functional as F

from tests.bnact_ref import BF16, BF16_EPS, F32, U24, _fail, _seed, d, judge_channels, judge_elem, judge_sum, sum_rows_chain  # noqa: F401

K = dict(y0=20.0, mlp=6.0, gate=10.0, gate_dx=8.0, bwd=11.0, pool_bwd=9.0)
KINK = 2.0 ** -19
CHAIN_TOL = 8.9e-5
THREADS = 256
EPS = float(torch.tensor(1e-3, dtype=torch.float32))
MOMENTUM = float(torch.tensor(0.03, dtype=torch.float32))


# ---------------------------------------------------------------- references -------------------------------------------------------------
def hswish(y):
    return y * torch.clamp(y + 3, 0, 6) / 6


def dhswish(y):
    return torch.where(y <= -3, torch.zeros_like(y), torch.where(y >= 3, torch.ones_like(y), (2 * y + 3) / 6))


def pool(x, swap_div=False):
    """x [n, H, W, C] -> [n, H + W, C]: rows 0..H-1 the mean over w, rows H.. the mean over h.  swap_div: the DEFECT 1/H <-> 1/W"""
    n, h, w, c = x.shape
    dh, dw = (h, w) if swap_div else (w, h)
    return torch.cat((x.sum(2) / dh, x.sum(1) / dw), 1)


def pool_mag(x):
    return pool(x.abs())


def conv1(pl, w1, b1):
    return pl @ w1.t() + b1


def conv1_mag(pl, w1, b1):
    return pl.abs() @ w1.abs().t() + b1.abs()


def conv1_stats(pl, w1, b1, drop_last=False):
    """(sum y0, sum y0^2) over all positions.  drop_last: the DEFECT of a pass that misses the last position"""
    y0 = conv1(pl, w1, b1).reshape(-1, w1.shape[0])
    if drop_last:
        y0 = y0[:-1]
    return y0.sum(0), (y0 * y0).sum(0)


def conv1_stats_mag(pl, w1, b1):
    """((sum |y0|, sum y0^2), (sum M_y0, sum 2 |y0| M_y0 + y0^2))"""
    m = w1.shape[0]
    y0, my = conv1(pl, w1, b1).reshape(-1, m), conv1_mag(pl, w1, b1).reshape(-1, m)
    return (y0.abs().sum(0), (y0 * y0).sum(0)), (my.sum(0), (2 * y0.abs() * my + y0 * y0).sum(0))


def _y1(pl, w1, b1, sc, sh):
    y0 = conv1(pl, w1, b1)
    return y0 if sc is None else y0 * sc + sh


def _y1_mag(pl, w1, b1, sc, sh):
    m = conv1_mag(pl, w1, b1)
    return m if sc is None else m * sc.abs() + sh.abs()


def mlp(pl, h, w1, b1, sc, sh, wh, bh, ww, bw, swap_hw=False):
    """(a_h [n, H, C], a_w [n, W, C]); sc is None: the folded form.  swap_hw: the DEFECT conv_h <-> conv_w"""
    y2 = hswish(_y1(pl, w1, b1, sc, sh))
    if swap_hw:
        wh, bh, ww, bw = ww, bw, wh, bh
    return torch.sigmoid(y2[:, :h] @ wh.t() + bh), torch.sigmoid(y2[:, h:] @ ww.t() + bw)


def mlp_mag(pl, h, w1, b1, sc, sh, wh, bh, ww, bw):
    """(M_ah, M_aw).  z = bx + sum_m Wx[c, m] y2[m] is accumulated by ONE thread, sequentially over the mip (up to 64) terms on top of its bias
    (ly_coordatt_mlp_kernel: `s = bx[c]; for m: s += ...`): z is a sum in the sense of the sums' bound, u24 (L_z sum |term| + K sum M_term) with
    L_z = mip + 1 from the code, and enters M as L_z / K of its terms.  (At a channel saturated by its bias, |z| = 20 from the first add on, every
    one of the mip adds rounds at the size of 20: torch's float32 matmul on the CPU, which K is measured on, does not add in that order.)  y1 is
    a 64-lane shuffle tree over at most 16 terms per lane and stays with K."""
    mip = w1.shape[0]
    y1, m1 = _y1(pl, w1, b1, sc, sh), _y1_mag(pl, w1, b1, sc, sh)
    y2 = hswish(y1).abs()
    lz = (mip + 1) / K["mlp"]
    a_h, a_w = mlp(pl, h, w1, b1, sc, sh, wh, bh, ww, bw)
    mz_h = (1.5 * m1[:, :h] + y2[:, :h]) @ wh.abs().t() + bh.abs() + lz * (y2[:, :h] @ wh.abs().t() + bh.abs())
    mz_w = (1.5 * m1[:, h:] + y2[:, h:]) @ ww.abs().t() + bw.abs() + lz * (y2[:, h:] @ ww.abs().t() + bw.abs())
    return a_h * (1 - a_h) * mz_h + a_h, a_w * (1 - a_w) * mz_w + a_w


def gate(x, a_h, a_w, res=None, no_aw=False):
    """out = x a_h[n, h] a_w[n, w] (+ res).  no_aw: the DEFECT of a gate without a_w"""
    out = x * a_h.unsqueeze(2) * (1.0 if no_aw else a_w.unsqueeze(1))
    return out if res is None else out + res


def gate_mag(x, a_h, a_w, res=None):
    return gate(x.abs(), a_h, a_w, None if res is None else res.abs())


def gate_bwd(dout, x, a_h, a_w, da_w_rows=None):
    """(dx, da_h, da_w).  da_w_rows: the DEFECT of da_w summed over the first `da_w_rows` rows only (a missing row band)"""
    t = dout * x
    th = t if da_w_rows is None else t[:, :da_w_rows]
    ah = a_h if da_w_rows is None else a_h[:, :da_w_rows]
    return dout * a_h.unsqueeze(2) * a_w.unsqueeze(1), (t * a_w.unsqueeze(1)).sum(2), (th * ah.unsqueeze(2)).sum(1)


def gate_bwd_mag(dout, x, a_h, a_w):
    """(M_dx, sum |term| of da_h, sum |term| of da_w): the terms are three-factor products, their own roundings are K times themselves"""
    return gate_bwd(dout.abs(), x.abs(), a_h, a_w)


def mlp_bwd(pl, w1, b1, mean, invstd, gamma, beta, wh, ww, a_h, a_w, da_h, da_w, no_s2=False, hs_one=False, dbh_all=False):
    """the derivative of mlp() in its train form through BatchNorm's batch statistics, by the formulas of the comment above
    ly_coordatt_mlp_bwd1_kernel; a_h / a_w are the STORED forward results (the kernel reads them), mean / invstd the stored statistics.
    -> dict(dpool, dW1, dgamma, dbeta, dWh, dbh, dWw, dbw) and the intermediates.  The keyword switches plant DEFECTS for the host tests:
    no_s2 (BatchNorm backward without xh S2 / R), hs_one (h_swish' = 1 on (2.9, 3)), dbh_all (dbh also sums the column positions)"""
    n, l, c = pl.shape
    h = a_h.shape[1]
    r = n * l
    row = (torch.arange(l) < h).to(pl.dtype).view(1, l, 1)
    a, da = torch.cat((a_h, a_w), 1), torch.cat((da_h, da_w), 1)
    dz = da * a * (1 - a)
    dzh, dzw = dz * row, dz * (1 - row)
    d2 = dzh @ wh + dzw @ ww
    y0 = conv1(pl, w1, b1)
    xh = (y0 - mean) * invstd
    y1 = gamma * xh + beta
    y2 = hswish(y1)
    hp = dhswish(y1)
    if hs_one:
        hp = torch.where((y1 > 2.9) & (y1 < 3), torch.ones_like(hp), hp)
    g = d2 * hp
    s1, s2 = g.sum((0, 1)), (g * xh).sum((0, 1))
    dy0 = gamma * invstd * (g - s1 / r - (0.0 if no_s2 else xh * s2 / r))
    return dict(dpool=dy0 @ w1, dW1=torch.einsum("nlm,nlc->mc", dy0, pl), dgamma=s2, dbeta=s1, dWh=torch.einsum("nlc,nlm->cm", dzh, y2),
                dbh=(dz if dbh_all else dzh).sum((0, 1)), dWw=torch.einsum("nlc,nlm->cm", dzw, y2), dbw=dzw.sum((0, 1)),
                dz=dz, y1=y1, y2=y2, g=g, dy0=dy0, xh=xh)


def mlp_bwd_mag(pl, w1, b1, mean, invstd, gamma, beta, wh, ww, a_h, a_w, da_h, da_w):
    """magnitudes for mlp_bwd: `dpool` (and the intermediates g, dy0, y2, y1) elementwise; for every sum a pair (sum |term|, sum M_term)"""
    n, l, c = pl.shape
    h = a_h.shape[1]
    r = n * l
    o = mlp_bwd(pl, w1, b1, mean, invstd, gamma, beta, wh, ww, a_h, a_w, da_h, da_w)
    row = (torch.arange(l) < h).to(pl.dtype).view(1, l, 1)
    a, da = torch.cat((a_h, a_w), 1), torch.cat((da_h, da_w), 1)
    dz, xh, y1, g, dy0 = o["dz"], o["xh"], o["y1"], o["g"], o["dy0"]
    m_dz = dz.abs()
    d2 = (dz * row) @ wh + (dz * (1 - row)) @ ww
    m_d2 = (m_dz * row + dz.abs() * row) @ wh.abs() + (m_dz * (1 - row) + dz.abs() * (1 - row)) @ ww.abs()
    m_y0 = conv1_mag(pl, w1, b1)
    m_xh = (m_y0 + mean.abs()) * invstd.abs() + 2 * xh.abs()
    m_y1 = gamma.abs() * m_xh + beta.abs()
    inside = (y1.abs() < 3).to(pl.dtype)
    m_g = m_d2 * dhswish(y1).abs() + d2.abs() * m_y1 / 3 * inside + g.abs()
    l1 = bwd1_chain(r)
    s1, s2 = o["dbeta"], o["dgamma"]
    t1, t2 = (g.abs().sum((0, 1)), m_g.sum((0, 1))), ((g * xh).abs().sum((0, 1)), (m_g * xh.abs() + g.abs() * m_xh).sum((0, 1)))
    e1, e2 = (l1 * t1[0] + t1[1]) / r, (l1 * t2[0] + t2[1]) / r
    m_dy0 = (gamma * invstd).abs() * (m_g + e1 + m_xh * s2.abs() / r + xh.abs() * e2 + g.abs() + s1.abs() / r + (xh * s2).abs() / r)
    m_y2 = 1.5 * m_y1 + o["y2"].abs()
    ein = lambda a_, b_: torch.einsum("nlc,nlm->cm", a_, b_)
    return dict(dpool=m_dy0 @ w1.abs() + dy0.abs() @ w1.abs(), g=m_g, dy0=m_dy0, y2=m_y2, y1=m_y1, dbeta=t1, dgamma=t2,
                dW1=(ein(pl.abs(), dy0.abs()).t(), ein(pl.abs(), m_dy0).t()),
                dWh=(ein(dz.abs() * row, o["y2"].abs()), ein(m_dz * row, o["y2"].abs()) + ein(dz.abs() * row, m_y2)),
                dWw=(ein(dz.abs() * (1 - row), o["y2"].abs()), ein(m_dz * (1 - row), o["y2"].abs()) + ein(dz.abs() * (1 - row), m_y2)),
                dbh=((dz.abs() * row).sum((0, 1)), (m_dz * row).sum((0, 1))), dbw=((dz.abs() * (1 - row)).sum((0, 1)), (m_dz * (1 - row)).sum((0, 1))))


def mlp_bwd_autograd(pl, w1, b1, gamma, beta, wh, bh, ww, bw, h, da_h, da_w, eps):
    """the same gradients through float64 autograd of mlp() with bn1 on batch statistics: built independently of mlp_bwd's formulas"""
    leaves = [t.clone().requires_grad_(True) for t in (pl, w1, b1, gamma, beta, wh, bh, ww, bw)]
    p, W1, B1, ga, be, Wh, Bh, Ww, Bw = leaves
    y0 = conv1(p, W1, B1)
    mean = y0.mean((0, 1))
    var = ((y0 - mean) ** 2).mean((0, 1))
    y2 = hswish(ga * (y0 - mean) / torch.sqrt(var + eps) + be)
    a_h, a_w = torch.sigmoid(y2[:, :h] @ Wh.t() + Bh), torch.sigmoid(y2[:, h:] @ Ww.t() + Bw)
    ((a_h * da_h).sum() + (a_w * da_w).sum()).backward()
    keys = ("dpool", "dW1", "db1", "dgamma", "dbeta", "dWh", "dbh", "dWw", "dbw")
    out = {k: t.grad for k, t in zip(keys, leaves)}
    out.update(a_h=a_h.detach(), a_w=a_w.detach(), mean=mean.detach(), invstd=(1 / torch.sqrt(var + eps)).detach())
    return out


def pool_bwd(gp, h, w, dx0=None):
    """dx[n, h, w, c] = gp[n, h, c] / W + gp[n, H + w, c] / H (+ dx0)"""
    dx = gp[:, :h].unsqueeze(2) / w + gp[:, h:].unsqueeze(1) / h
    return dx if dx0 is None else dx + dx0


def pool_bwd_mag(gp, h, w, dx0=None):
    return pool_bwd(gp.abs(), h, w, None if dx0 is None else dx0.abs())


PARAMS = ("w1", "b1", "gamma", "beta", "wh", "bh", "ww", "bw")
GRADS = ("dW1", "db1", "dgamma", "dbeta", "dWh", "dbh", "dWw", "dbw")


def chain_autograd(x, params, r, dtype=torch.float64, rm=None, rv=None, eps=EPS, momentum=MOMENTUM):
    """the reference module (models/common.py:1595-1609) in train mode under autograd, in torch ops on NCHW tensors: loss = sum(out r).
    x, r [n, H, W, C]; params: dict of PARAMS (2-D weights).  -> dict(out, dx [n, H, W, C], the eight GRADS, rm, rv)"""
    xx = x.to(dtype).permute(0, 3, 1, 2).clone().requires_grad_(True)
    p = {k: params[k].to(dtype).clone().requires_grad_(True) for k in PARAMS}
    rm = None if rm is None else rm.to(dtype).clone()
    rv = None if rv is None else rv.to(dtype).clone()
    n, c, h, w = xx.shape
    y = torch.cat((xx.mean(3, keepdim=True), xx.mean(2, keepdim=True).permute(0, 1, 3, 2)), 2)
    y = F.conv2d(y, p["w1"][:, :, None, None], p["b1"])
    y = F.batch_norm(y, rm, rv, p["gamma"], p["beta"], True, momentum, eps)
    y = y * F.relu6(y + 3) / 6
    a_h = torch.sigmoid(F.conv2d(y[:, :, :h], p["wh"][:, :, None, None], p["bh"]))
    a_w = torch.sigmoid(F.conv2d(y[:, :, h:].permute(0, 1, 3, 2), p["ww"][:, :, None, None], p["bw"]))
    out = xx * a_w * a_h
    (out * r.to(dtype).permute(0, 3, 1, 2)).sum().backward()
    res = dict(out=out.detach().permute(0, 2, 3, 1), dx=xx.grad.permute(0, 2, 3, 1), rm=rm, rv=rv)
    res.update({g: p[k].grad for g, k in zip(GRADS, PARAMS)})
    return res


def chain_parts(x, params, r, rm=None, rv=None, eps=EPS, momentum=MOMENTUM):
    """the chain composed of this module's own parts, float64: the same dict as chain_autograd plus the intermediates and `floors`"""
    x, r = x.double(), r.double()
    p = {k: params[k].double() for k in PARAMS}
    n, h, w, c = x.shape
    cnt = n * (h + w)
    pl = pool(x)
    s1, s2 = conv1_stats(pl, p["w1"], p["b1"])
    mean = s1 / cnt
    var = torch.clamp(s2 / cnt - mean * mean, min=0.0)
    invstd = 1 / torch.sqrt(var + eps)
    sc, sh = p["gamma"] * invstd, p["beta"] - mean * p["gamma"] * invstd
    a_h, a_w = mlp(pl, h, p["w1"], p["b1"], sc, sh, p["wh"], p["bh"], p["ww"], p["bw"])
    out = gate(x, a_h, a_w)
    dxg, da_h, da_w = gate_bwd(r, x, a_h, a_w)
    args = (pl, p["w1"], p["b1"], mean, invstd, p["gamma"], p["beta"], p["wh"], p["ww"], a_h, a_w, da_h, da_w)
    b = mlp_bwd(*args)
    res = dict(out=out, dx=pool_bwd(b["dpool"], h, w, dxg), dx_gate=dxg, db1=torch.zeros_like(p["b1"]), y1=b["y1"], pool=pl, mean=mean, invstd=invstd)
    res.update({k: b[k] for k in GRADS if k != "db1"})
    if rm is not None:
        res["rm"] = (1 - momentum) * rm.double() + momentum * mean
        res["rv"] = (1 - momentum) * rv.double() + momentum * var * (cnt / max(cnt - 1.0, 1.0))
    # floors: the sums' own bound over the terms of the LAST sum, (L + K) u24 sum |term|, for the four gradients that may cancel to ~0
    mg = mlp_bwd_mag(*args)
    l2, l1 = bwd2_chain(cnt, c, True), bwd1_chain(cnt) + 2
    res["floors"] = {k: U24 * ((l1 if k in ("dgamma", "dbeta") else l2) + K["bwd"]) * mg[k][0] for k in ("dgamma", "dbeta", "dbh", "dbw")}
    # dbh / dbw are sums of dz = da a (1 - a) with a the STORED fp32 gate factor: at a saturated channel (a = 1 - 2e-9, stored as 1) the rounding
    # of a is all of 1 - a, so the forward's own error K_mlp u24 M_a times |da| joins the floor
    m_ah, m_aw = mlp_mag(pl, h, p["w1"], p["b1"], sc, sh, p["wh"], p["bh"], p["ww"], p["bw"])
    res["floors"]["dbh"] = res["floors"]["dbh"] + U24 * K["mlp"] * (da_h.abs() * m_ah).sum((0, 1))
    res["floors"]["dbw"] = res["floors"]["dbw"] + U24 * K["mlp"] * (da_w.abs() * m_aw).sum((0, 1))
    res["m_y1"] = mg["y1"]
    return res


# ---------------------------------------------------------------- chain lengths (from the code) -------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def pool_chain(length, c):
    groups = THREADS // (c // 4)
    return _cdiv(length, groups) + min(groups, length) + 2


def stats_chain(positions):
    blocks = min(_cdiv(positions, 4), 256)
    return _cdiv(positions, blocks * 4) + 4


def gate_bwd_chains(h, w, c):
    """(L of da_h, L of da_w)"""
    groups = THREADS // (c // 4)
    slabs, bands = _cdiv(w, groups * 8), _cdiv(h, 8)
    return 8 + groups + (sum_rows_chain(slabs) if slabs > 1 else 0), 8 + (sum_rows_chain(bands) if bands > 1 else 0)


def bwd1_chain(r):
    blocks = min(_cdiv(r, 4), 1024)
    return _cdiv(r, blocks * 4) + 1


def bwd2_geometry(r, c):
    """(chunks, rows per block) of launch_coordatt_bwd"""
    groups = _cdiv(c, 64)
    chunks = max(min(_cdiv(96, groups), _cdiv(r, 32)), 1)
    rpb = _cdiv(r, chunks)
    return _cdiv(r, rpb), rpb


def bwd2_chain(r, c, f64):
    chunks, rpb = bwd2_geometry(r, c)
    return _cdiv(rpb, 4) + 3 + (0 if f64 else chunks + 1)


# ---------------------------------------------------------------- judges ------------------------------------------------------------------
def judge(got, want, mag, what, k, bf16=False):
    """elementwise: K u24 M [+ 2^-8 |want|]; returns the worst err / (u24 M) for the record"""
    return judge_elem(got, want, (mag, torch.zeros_like(mag)), what, bf16=bf16, k=k)


def sum_ratio(got, want, chain, term_abs, term_mag, k):
    """for the record: the worst |err| / bound of a sum"""
    bound = U24 * (chain * term_abs + k * term_mag)
    err = (d(got).reshape(want.shape) - want).abs()
    return float((err / bound.clamp(min=1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0


def _zeros(t):
    return torch.zeros_like(t)


def elem_ratio(got, want, mag, bf16=False):
    """for the record: the worst (|err| - storage allowance) / (u24 M)"""
    err = (d(got).reshape(want.shape) - want).abs() - (BF16_EPS * want.abs() if bf16 else 0.0)
    return float((err.clamp(min=0.0) / (U24 * mag).clamp(min=1e-300))[mag > 0].max()) if bool((mag > 0).any()) else 0.0


def _say(what, **ratios):
    """every judge below prints its figures BEFORE it asserts"""
    print(f"{what}: " + "  ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    return ratios


def judge_pool(got, x, what):
    """ly_pool_hw against pool(x): a sum judge per output with the chain of ITS reduction; the terms are exact.  -> err / bound"""
    n, h, w, c = x.shape
    want, mag = pool(x), pool_mag(x)
    ch = torch.cat((torch.full((h,), float(pool_chain(w, c))), torch.full((w,), float(pool_chain(h, c))))).double().view(1, h + w, 1)
    out = _say(what, pool_err_over_bound=sum_ratio(got, want, ch, mag, _zeros(mag), 0.0))
    judge_sum(got, want, ch, mag, _zeros(mag), what)
    return out


def judge_stats(s1, s2, x, what):
    """ly_coordatt_conv1_stats (the float64 accumulator [2 mip]) against conv1_stats"""
    a = [x[k].double() for k in ("pool", "w1", "b1")]
    (w1_, w2_), ((t1, t2), (m1, m2)) = conv1_stats(*a), conv1_stats_mag(*a)
    ch = stats_chain(a[0].shape[0] * a[0].shape[1])
    out = _say(what, stats_err_over_bound=max(sum_ratio(s1, w1_, ch, t1, m1, K["y0"]), sum_ratio(s2, w2_, ch, t2, m2, K["y0"])))
    judge_sum(s1, w1_, ch, t1, m1, what + " sum", k=K["y0"])
    judge_sum(s2, w2_, ch, t2, m2, what + " sum of squares", k=K["y0"])
    return out


MLP_KEYS = ("w1", "b1", "sc", "sh", "wh", "bh", "ww", "bw")


def judge_mlp(a_h, a_w, x, h, what):
    a = [None if x[k] is None else x[k].double() for k in MLP_KEYS]
    want, mag = mlp(x["pool"].double(), h, *a), mlp_mag(x["pool"].double(), h, *a)
    out = _say(what, mlp=max(elem_ratio(a_h, want[0], mag[0]), elem_ratio(a_w, want[1], mag[1])))
    judge(a_h, want[0], mag[0], what + " a_h", K["mlp"])
    judge(a_w, want[1], mag[1], what + " a_w", K["mlp"])
    return out


def judge_gate(got, x, what):
    a = [None if x[k] is None else d(x[k]) for k in ("x", "a_h", "a_w", "res")]
    bf = x["x"].dtype == BF16
    out = _say(what, gate=elem_ratio(got, gate(*a), gate_mag(*a), bf))
    judge(got, gate(*a), gate_mag(*a), what, K["gate"], bf16=bf)
    return out


def judge_gate_bwd(dx, da_h, da_w, x, what):
    a = [d(x[k]) for k in ("dout", "x", "a_h", "a_w")]
    n, h, w, c = a[1].shape
    bf = x["x"].dtype == BF16
    (wdx, wh_, ww_), (mdx, th, tw) = gate_bwd(*a), gate_bwd_mag(*a)
    lh, lw = gate_bwd_chains(h, w, c)
    out = _say(what, gate_dx=elem_ratio(dx, wdx, mdx, bf),
               da_err_over_bound=max(sum_ratio(da_h, wh_, lh, th, th, K["gate_dx"]), sum_ratio(da_w, ww_, lw, tw, tw, K["gate_dx"])))
    judge(dx, wdx, mdx, what + " dx", K["gate_dx"], bf16=bf)
    judge_sum(da_h, wh_, lh, th, th, what + " da_h", k=K["gate_dx"])
    judge_sum(da_w, ww_, lw, tw, tw, what + " da_w", k=K["gate_dx"])
    return out


BWD_SUMS = ("dW1", "dgamma", "dbeta", "dWh", "dbh", "dWw", "dbw")


def judge_mlp_bwd(got, x, f64, what, prefill=None, keys=None):
    """got: dict(dpool and the seven BWD_SUMS targets); prefill: what the targets held before (the results are ADDED)"""
    n, l, c = x["pool"].shape
    r = n * l
    want, mag = mlp_bwd(*bwd_args(x)), mlp_bwd_mag(*bwd_args(x))
    sums = {}
    for k in (keys or ("dpool",) + BWD_SUMS):
        if k == "dpool":
            continue
        p0 = _zeros(want[k]) if prefill is None else prefill[k].double().reshape(want[k].shape)
        ch = bwd1_chain(r) + 2 if k in ("dgamma", "dbeta") else bwd2_chain(r, c, f64)
        sums[k] = (d(got[k]).reshape(want[k].shape), want[k] + p0, ch, mag[k][0] + p0.abs(), mag[k][1])
    out = _say(what, bwd=elem_ratio(got["dpool"], want["dpool"], mag["dpool"]) if "dpool" in (keys or ("dpool",)) else 0.0,
               sums_err_over_bound=max([sum_ratio(*v, K["bwd"]) for v in sums.values()] + [0.0]))
    if "dpool" in (keys or ("dpool",)):
        judge(got["dpool"], want["dpool"], mag["dpool"], what + " dpool", K["bwd"])
    for k, v in sums.items():
        judge_sum(*v, f"{what} {k}", k=K["bwd"])
    return out


def judge_pool_bwd(dx, x, h, w, acc, what):
    dx0 = d(x["dx0"]) if acc else None
    bf = x["dx0"].dtype == BF16
    want, mag = pool_bwd(x["gp"].double(), h, w, dx0), pool_bwd_mag(x["gp"].double(), h, w, dx0)
    out = _say(what, pool_bwd=elem_ratio(dx, want, mag, bf))
    judge(dx, want, mag, what, K["pool_bwd"], bf16=bf)
    return out


def in_band(y1, m_y1, width=KINK):
    return (y1.abs() - 3).abs() <= width * m_y1


def assert_no_kink(y1, m_y1, what, width=KINK):
    n = int(in_band(y1, m_y1, width).sum())
    assert n == 0, f"{what}: {n} elements inside the h_swish kink band"


def regimes(y1):
    """(elements with y1 <= -3, inside, y1 >= 3)"""
    return int((y1 <= -3).sum()), int((y1.abs() < 3).sum()), int((y1 >= 3).sum())


# ---------------------------------------------------------------- input builders ----------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(_seed("coordatt", *key))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64)


def make_x(g, n, h, w, c, dtype):
    """mixed sign, per-channel scale in (0.5, 10), |x| <= 30, channel c - 1 exactly zero"""
    x = (_randn(g, n, h, w, c) * (_rand(g, c) * 9.5 + 0.5)).clamp(-30, 30)
    x[..., c - 1] = 0.0
    return x.to(dtype)


def make_dout(g, n, h, w, c, dtype):
    """cancelling signs: neighbouring pixels nearly opposite"""
    base = _randn(g, n, 1, 1, c)
    sign = (1 - 2 * ((torch.arange(h).view(h, 1) + torch.arange(w).view(1, w)) % 2)).to(torch.float64).view(1, h, w, 1)
    return (base * sign + 0.05 * _randn(g, n, h, w, c)).to(dtype)


def make_gates(g, n, h, w, c):
    """a_h, a_w in (0, 1) with saturated channels (sigmoid of +-20)"""
    z = _randn(g, n, h + w, c) * 2
    z[..., 3 % c] = 20.0
    z[..., 5 % c] = -20.0
    a = torch.sigmoid(z).float()
    return a[:, :h].contiguous(), a[:, h:].contiguous()


def make_heads(g, c, mip):
    """conv_h / conv_w: arguments of the sigmoid ~ N(0, 2) and +20 / -20 in channels 3 / 5 of every seven (saturation)"""
    out = []
    for _ in range(2):
        wx, bx = _randn(g, c, mip) * 0.5, _randn(g, c)
        for rem, val in ((3, 20.0), (5, -20.0)):
            sat = torch.arange(c) % 7 == rem
            bx[sat] = val
            wx[sat] *= 0.05
        out += [wx.float(), bx.float()]
    return out


GAMMAS = (4.5, 1.0, 2.5, 3.6)


def make_bn(g, y0, mip):
    """(mean, invstd, gamma, beta) fp32 that spread y1 = gamma (y0 - mean) invstd + beta over (-6, 6) and beyond: all three h_swish regimes"""
    flat = y0.reshape(-1, mip)
    mean = flat.mean(0)
    var = ((flat - mean) ** 2).mean(0)
    invstd = 1 / torch.sqrt(var + EPS)
    gamma = torch.tensor([GAMMAS[m % 4] for m in range(mip)], dtype=torch.float64)
    beta = _rand(g, mip) - 0.5
    return mean.float(), invstd.float(), gamma.float(), beta.float()


def nudge_pool(pl, y1_of, what):
    """scales the positions of pool [n, L, C] that hold an element in the kink band by 1 + 2^-10 until none is left; -> (pool, moved)"""
    moved = 0
    for _ in range(8):
        y1, m1 = y1_of(pl.double())
        band = in_band(y1, m1).any(-1)
        k = int(band.sum())
        if k == 0:
            return pl, moved
        moved += k
        pl = torch.where(band.unsqueeze(-1), pl.double() * (1 + 2.0 ** -10), pl.double()).float()
    raise AssertionError(f"{what}: the kink band could not be emptied")


def mlp_inputs(cid, n, h, w, c, mip, train):
    """pool [n, H + W, C] fp32 (position 0 all zero), conv1 / bn1 / heads; train: sc, sh else None (folded)"""
    g = _gen("mlp", cid)
    pl = (_randn(g, n, h + w, c) * (_rand(g, c) * 3 + 0.2)).float()
    pl[0, 0] = 0.0
    w1, b1 = (_randn(g, mip, c) / math.sqrt(c)).float(), (_randn(g, mip) * 0.1).float()
    mean, invstd, gamma, beta = make_bn(g, conv1(pl.double(), w1.double(), b1.double()), mip)
    sc, sh = (gamma.double() * invstd.double()).float(), (beta.double() - mean.double() * gamma.double() * invstd.double()).float()
    if not train:                                    # folded: the affine goes into the weights
        w1, b1, sc, sh = (w1.double() * sc.double().view(-1, 1)).float(), (b1.double() * sc.double() + sh.double()).float(), None, None
    wh, bh, ww, bw = make_heads(g, c, mip)
    return dict(pool=pl, w1=w1, b1=b1, sc=sc, sh=sh, wh=wh, bh=bh, ww=ww, bw=bw)


def mlp_bwd_inputs(cid, n, h, w, c, mip):
    """the operands of ly_coordatt_mlp_bwd as stored (all fp32); a_h / a_w are the float64 forward rounded to fp32; pool nudged out of the band"""
    g = _gen("mlpbwd", cid)
    pl = (_randn(g, n, h + w, c) * (_rand(g, c) * 3 + 0.2)).float()
    w1, b1 = (_randn(g, mip, c) / math.sqrt(c)).float(), (_randn(g, mip) * 0.1).float()
    mean, invstd, gamma, beta = make_bn(g, conv1(pl.double(), w1.double(), b1.double()), mip)
    wh, bh, ww, bw = make_heads(g, c, mip)
    w64 = [t.double() for t in (w1, b1, mean, invstd, gamma, beta)]

    def y1_of(p):
        xh = (conv1(p, w64[0], w64[1]) - w64[2]) * w64[3]
        return w64[4] * xh + w64[5], w64[4].abs() * ((conv1_mag(p, w64[0], w64[1]) + w64[2].abs()) * w64[3] + 2 * xh.abs()) + w64[5].abs()
    pl, moved = nudge_pool(pl, y1_of, cid)
    sc, sh = w64[4] * w64[3], w64[5] - w64[2] * w64[4] * w64[3]
    a_h, a_w = mlp(pl.double(), h, w64[0], w64[1], sc, sh, wh.double(), bh.double(), ww.double(), bw.double())
    sign = (1 - 2 * (torch.arange(h + w) % 2)).to(torch.float64).view(1, h + w, 1)
    da = (_randn(g, n, 1, c) * sign * 3 + 0.3 * _randn(g, n, h + w, c)).float()
    return dict(pool=pl, w1=w1, b1=b1, mean=mean, invstd=invstd, gamma=gamma, beta=beta, wh=wh, bh=bh, ww=ww, bw=bw, a_h=a_h.float().contiguous(),
                a_w=a_w.float().contiguous(), da_h=da[:, :h].contiguous(), da_w=da[:, h:].contiguous(), moved=moved)


BWD_KEYS = ("pool", "w1", "b1", "mean", "invstd", "gamma", "beta", "wh", "ww", "a_h", "a_w", "da_h", "da_w")


def bwd_args(x):
    return [x[k].double() for k in BWD_KEYS]


def chain_inputs(c, reduction, n, h, w, dtype):
    """x, r [n, H, W, C] stored as dtype, the module's parameters (fp32) with bn1.weight / bias spreading y1 over the three regimes, running
    statistics; rows / columns of x holding a position in the kink band (by the reference's own statistics) are scaled until none is left"""
    mip = max(8, c // reduction)
    g = _gen("chain", c, reduction, n, h, w, str(dtype))
    x, r = make_x(g, n, h, w, c, dtype), make_dout(g, n, h, w, c, dtype)
    w1, b1 = (_randn(g, mip, c) / math.sqrt(c)).float(), (_randn(g, mip) * 0.1).float()
    gamma = torch.tensor([GAMMAS[m % 4] for m in range(mip)], dtype=torch.float32)
    beta = (_rand(g, mip) - 0.5).float()
    wh, bh, ww, bw = make_heads(g, c, mip)
    params = dict(w1=w1, b1=b1, gamma=gamma, beta=beta, wh=wh, bh=bh, ww=ww, bw=bw)
    rm, rv = _randn(g, mip).float(), (_rand(g, mip) + 0.5).float()
    moved = 0
    step = 1 + (2.0 ** -5 if dtype == BF16 else 2.0 ** -10)
    for _ in range(8):
        ref = chain_parts(d(x), params, d(r))
        band = in_band(ref["y1"], ref["m_y1"]).any(-1)          # [n, H + W]
        k = int(band.sum())
        if k == 0:
            break
        moved += k
        xd = d(x)
        xd = torch.where(band[:, :h].view(n, h, 1, 1), xd * step, xd)
        xd = torch.where(band[:, h:].view(n, 1, w, 1), xd * step, xd)
        x = xd.to(dtype)
    return dict(x=x, r=r, params=params, rm=rm, rv=rv, mip=mip, moved=moved)


# ---------------------------------------------------------------- case tables -------------------------------------------------------------
# branch of the kernels -> case id: the table in the docstring of tests/test_gpu_coordatt.py
HW6 = ((1, 1), (1, 37), (37, 1), (7, 13), (20, 20), (5, 160))
# ly_pool_hw: id -> (n, H, W, C, ldx)
POOL_CASES = {f"c{c}-{h}x{w}": (3 if (h, w) == (7, 13) else 1, h, w, c, c) for c in (8, 24, 168, 512, 1024) for h, w in HW6}
POOL_CASES.update({"ld-c24-7x13": (2, 7, 13, 24, 40), "ld-c168-5x9": (3, 5, 9, 168, 184)})
# ly_coordatt_conv1_stats: id -> (positions, C, mip)
STATS_POS = (1, 3, 4, 5, 1025, 2047, 2049, 4100)
STATS_CASES = {f"fast-c84-m8-p{p}": (p, 84, 8) for p in STATS_POS}
STATS_CASES.update({f"general-c320-m16-p{p}": (p, 320, 16) for p in STATS_POS})
for _c, _m, _tag in ((8, 8, "fast"), (256, 8, "fast"), (8, 16, "fast"), (84, 16, "fast"), (256, 16, "fast"), (84, 12, "fast-mip12"),
                     (320, 8, "general"), (512, 8, "general"), (512, 16, "general"), (84, 20, "wide64"), (320, 20, "wide64")):
    for _p in (5, 1025):
        STATS_CASES[f"{_tag}-c{_c}-m{_m}-p{_p}"] = (_p, _c, _m)
# ly_coordatt_mlp: id -> (n, H, W, C, mip); both forms each
MLP_CASES = {"c8-m8": (2, 5, 7, 8, 8), "c168-m12": (2, 5, 7, 168, 12), "c512-m16": (2, 7, 5, 512, 16), "c1024-m20": (1, 3, 4, 1024, 20),
             "c168-m64": (2, 5, 7, 168, 64), "c1024-m8": (1, 1, 6, 1024, 8)}
# ly_coordatt_gate: id -> (n, H, W, channel vectors C / vw, extra ldx, extra ldres (None: no res))
GATE_CASES = {"v1-5x7": (2, 5, 7, 1, 0, None), "v21-9x9-res": (2, 9, 9, 21, 0, 0), "v21-8x7-ld": (1, 8, 7, 21, 2, 3), "v128-1x9-res": (2, 1, 9, 128, 0, 1),
              "v128-9x7": (1, 9, 7, 128, 1, None)}
GATE_CASES.update({f"v256-{h}x{w}{'-res' if w in (7, 65) else ''}": (1, h, w, 256, 0, (0 if w in (7, 65) else None))
                   for h, w in ((1, 1), (8, 7), (9, 9), (3, 65))})
# ly_coordatt_gate_bwd: id -> (n, H, W, C, extra ldd in 16-byte vectors)
GATE_BWD_CASES = {"c8-1x7": (2, 1, 7, 8, 0), "c84-8x9": (2, 8, 9, 84, 0), "c168-9x13-ld": (1, 9, 13, 168, 2), "c512-17x17-slabs": (1, 17, 17, 512, 0),
                  "c512-8x16-oneslab": (2, 8, 16, 512, 0), "c1024-9x9-slabs": (1, 9, 9, 1024, 0), "c1024-1x65-slabs-ld": (1, 1, 65, 1024, 1),
                  "c8-17x1100-slabs": (1, 17, 1100, 8, 0)}
# ly_coordatt_mlp_bwd: id -> (n, H, W, C, mip);  R = n (H + W)
RSHAPES = {2: (1, 1, 1), 31: (1, 13, 18), 33: (3, 4, 7), 100: (4, 12, 13), 4100: (2, 1025, 1025)}
MLP_BWD_CASES = {}
for _m, _ns, _c in ((8, 1, 24), (8, 2, 84), (8, 4, 168), (8, 8, 320), (16, 4, 168), (16, 8, 320)):
    for _r in ((2, 31, 33, 100, 4100) if (_m, _ns) in ((8, 2), (16, 4)) else (33, 100)):
        MLP_BWD_CASES[f"m{_m}-ns{_ns}-c{_c}-r{_r}"] = RSHAPES[_r] + (_c, _m)
MLP_BWD_CASES["m16-ns8-c512-r100"] = RSHAPES[100] + (512, 16)
# ly_pool_hw_bwd: id -> (n, H, W, C, dtypes)
POOL_BWD_CASES = {"c8-1x1": (2, 1, 1, 8, (F32, BF16)), "c24-7x13": (2, 7, 13, 24, (F32, BF16)), "c168-5x9": (3, 5, 9, 168, (F32, BF16)),
                  "c1024-3x5": (1, 3, 5, 1024, (F32, BF16)), "c8-5x160": (1, 5, 160, 8, (F32, BF16)), "c168-1x300-gridcap": (1, 1, 300, 168, (F32, BF16)),
                  "flat-bf16-c12-7x13": (2, 7, 13, 12, (BF16,)), "flat-bf16-c20-5x9": (1, 5, 9, 20, (BF16,))}
# the whole chain: (c, reduction, n, H, W)
CHAIN_CASES = [(8, 32, 2, 5, 7), (168, 32, 1, 13, 11), (256, 16, 2, 9, 20), (512, 32, 2, 6, 6)]


def pool_inputs(cid, dtype):
    n, h, w, c, _ = POOL_CASES[cid]
    return make_x(_gen("pool", cid, str(dtype)), n, h, w, c, dtype)


def stats_inputs(cid):
    p, c, mip = STATS_CASES[cid]
    g = _gen("stats", cid)
    pl = (_randn(g, 1, p, c) * (_rand(g, c) * 3 + 0.2) + 0.3).float()
    return dict(pool=pl, w1=(_randn(g, mip, c) / math.sqrt(c)).float(), b1=(_randn(g, mip) * 0.5).float())


def gate_inputs(cid, dtype, with_res):
    n, h, w, ncv = GATE_CASES[cid][:4]
    c = ncv * (8 if dtype == BF16 else 4)
    g = _gen("gate", cid, str(dtype))
    a_h, a_w = make_gates(g, n, h, w, c)
    return dict(x=make_x(g, n, h, w, c, dtype), a_h=a_h, a_w=a_w, res=(_randn(g, n, h, w, c) * 5).to(dtype) if with_res else None)


def gate_bwd_inputs(cid, dtype):
    n, h, w, c, _ = GATE_BWD_CASES[cid]
    g = _gen("gatebwd", cid, str(dtype))
    a_h, a_w = make_gates(g, n, h, w, c)
    return dict(x=make_x(g, n, h, w, c, dtype), dout=make_dout(g, n, h, w, c, dtype), a_h=a_h, a_w=a_w)


def pool_bwd_inputs(cid, dtype):
    n, h, w, c, _ = POOL_BWD_CASES[cid]
    g = _gen("poolbwd", cid, str(dtype))
    return dict(gp=(_randn(g, n, h + w, c) * 3).float(), dx0=make_dout(g, n, h, w, c, dtype))


# ---------------------------------------------------------------- measurements (reference only) -------------------------------------------
class _one_thread:
    """torch's float32 reductions split their work by thread count: the measurements run on one thread and give the same figures everywhere"""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)


def _r(got, want, mag):
    m = mag > 0
    return float(((d(got) - want).abs() / (U24 * mag).clamp(min=1e-300))[m].max()) if bool(m.any()) else 0.0


def measure_k():
    """worst ratio, in units of u24 M, of torch's float32 evaluation of the references against float64 over every case of the tables"""
    with _one_thread():
        return _measure_k()


def _measure_k():
    worst = {k: 0.0 for k in K}
    up = lambda key, v: worst.__setitem__(key, max(worst[key], v))
    f32 = lambda t: None if t is None else t.float()
    f64 = lambda t: None if t is None else t.double()
    for cid in STATS_CASES:
        x = stats_inputs(cid)
        a = [x[k] for k in ("pool", "w1", "b1")]
        up("y0", _r(conv1(*a), conv1(*map(f64, a)), conv1_mag(*map(f64, a))))
    for cid, (n, h, w, c, mip) in MLP_CASES.items():
        for train in (True, False):
            x = mlp_inputs(cid, n, h, w, c, mip, train)
            a = [x[k] for k in ("w1", "b1", "sc", "sh", "wh", "bh", "ww", "bw")]
            got, want = mlp(x["pool"], h, *a), mlp(x["pool"].double(), h, *map(f64, a))
            mag = mlp_mag(x["pool"].double(), h, *map(f64, a))
            for i in (0, 1):
                up("mlp", _r(got[i], want[i], mag[i]))
    for cid, v in GATE_CASES.items():
        for dt in (F32, BF16):
            x = gate_inputs(cid, dt, v[5] is not None)
            a = [x[k] for k in ("x", "a_h", "a_w", "res")]
            up("gate", _r(gate(*map(f32, a)), gate(*map(f64, a)), gate_mag(*map(f64, a))))
    for cid in GATE_BWD_CASES:
        for dt in (F32, BF16):
            x = gate_bwd_inputs(cid, dt)
            a = [x[k] for k in ("dout", "x", "a_h", "a_w")]
            up("gate_dx", _r(gate_bwd(*map(f32, a))[0], gate_bwd(*map(f64, a))[0], gate_bwd_mag(*map(f64, a))[0]))
    for cid, (n, h, w, c, mip) in MLP_BWD_CASES.items():
        x = mlp_bwd_inputs(cid, n, h, w, c, mip)
        got, want, mag = mlp_bwd(*[x[k] for k in BWD_KEYS]), mlp_bwd(*bwd_args(x)), mlp_bwd_mag(*bwd_args(x))
        for k in ("dpool", "g", "dy0", "y2"):
            up("bwd", _r(got[k], want[k], mag[k]))
    for cid, (n, h, w, c, dts) in POOL_BWD_CASES.items():
        for dt in dts:
            x = pool_bwd_inputs(cid, dt)
            up("pool_bwd", _r(pool_bwd(x["gp"], h, w, x["dx0"].float()), pool_bwd(x["gp"].double(), h, w, d(x["dx0"])), pool_bwd_mag(x["gp"].double(), h, w, d(x["dx0"]))))
    return worst


CHAIN_KEYS = ("out", "dx", "dW1", "dgamma", "dbeta", "dWh", "dbh", "dWw", "dbw")


def judge_chain(got, ref, what, tol=CHAIN_TOL, bf16=False):
    """got: dict over CHAIN_KEYS (and db1, rm, rv, nbt when present) against chain_parts' dict; -> worst per-channel ratios for the record"""
    ratios = {}
    for k in CHAIN_KEYS:
        if k not in got:
            continue
        g, w_ = d(got[k]), ref[k]
        if k in ("out", "dx"):
            c = w_.shape[-1]
            # dx is ROUNDED TO bf16 TWICE: ly_coordatt_gate_bwd stores dout a_h a_w, ly_pool_hw_bwd reads it back, adds the pool gradient and
            # stores again — the first store's 2^-8 |dout a_h a_w| joins the storage allowance 2^-8 |dx|
            twice = BF16_EPS * ref["dx_gate"].abs().reshape(-1, c).amax(0) if (bf16 and k == "dx") else None
            ratios[k] = judge_channels(g.reshape(-1, c), w_.reshape(-1, c), f"{what} {k}", tol=tol, bf16=bf16, floor=twice)
        else:
            ratios[k] = judge_channels(g.reshape(w_.shape), w_, f"{what} {k}", tol=tol, floor=ref["floors"].get(k))      # 2-D: per column
    return ratios


def measure_chain_tol():
    """worst per-channel ratio of chain_autograd in float32 against the float64 reference over CHAIN_CASES x operand dtypes"""
    worst = {k: 0.0 for k in CHAIN_KEYS}
    with _one_thread():
        for c, red, n, h, w in CHAIN_CASES:
            for dt in (F32, BF16):
                ci = chain_inputs(c, red, n, h, w, dt)
                ref = chain_parts(d(ci["x"]), ci["params"], d(ci["r"]))
                got = chain_autograd(ci["x"].float(), ci["params"], ci["r"].float(), dtype=torch.float32)
                for k, v in judge_chain(got, ref, f"chain c{c}", tol=1.0).items():
                    worst[k] = max(worst[k], v)
    return worst
