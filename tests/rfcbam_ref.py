"""Float64 references, judges, input builders and case tables for the RFCBAMConv backward kernels of the streamed and the k = 1 routes

    streamed (grad._rfcbam_backward_streamed)   ly_rf_generate -> ly_rf_bwd_attn | ly_rf3s_bwd 0 -> ly_rfa_bwd -> ly_rf_bwd_relu | ly_rf3s_bwd 1
                                                -> (ly_bn_bwd_coeffs) -> ly_rf_bwd_gen -> ly_se_bwd -> ly_rf_bwd_dx
    k = 1    (grad._rfcbam_backward_k1)         ly_rf1_bwd 0 -> ly_rfa_bwd -> ly_rf1_bwd 1 -> (ly_bn_bwd_coeffs) -> ly_se_bwd -> ly_rf1_bwd 2

(csrc/ly_rfcbam_bwd.hip, csrc/ly_rf1_bwd.hip, csrc/ly_rfcbam_att.hip).  A plain helper module: tests/test_rfcbam_host.py (CPU) and
tests/test_gpu_rfcbam_bwd.py (device) import the SAME references, judges, builders and case tables from here.  The judges' forms, `_fail`,
`nudge`, `in_band` and KINK are those of tests/bnact_ref.py and are imported from there.  Nothing here calls a kernel or lead_yolo_amd.ops.

References take the stored values — the fp32 / bf16 tensors a kernel is given — widened exactly, in the kernels' own layouts (the comments at
the top of the two .hip files): x [n, H, W, C]; expanded tensors [m][t][c] with m = (n, ho, wo) the output pixel and t = ty k + tx the tap;
maps [n][k Ho][k Wo] (mm / d_mm with a trailing 2 = (max, mean)), position of (m, t) = (ho k + ty, wo k + tx); ag / bg / alpha / kappa /
lambda / the sums [t][c]; the generate weight [c KK][KK] = w[c][t][u]; ca / d_ca / dgap [n][c].  One function per entry point and pass, each
with a `*_mag` companion that carries the sum of the magnitudes of its terms, and with keyword switches that plant ONE named defect each
(tests/test_rfcbam_host.py shows that the judges reject them; no broken kernel is ever built).

Decisions.  Three decisions of these kernels cannot be judged with a bound when their argument is within rounding of the threshold; the
builders remove every such element, the cap is ZERO and no judge masks anything (assert_premises, asserted by every host and device test):
  1. ReLU of fma(a, u, b): bnact_ref.nudge on u with bnact_ref.KINK = 2^-22 (stored a, u, b and one fused multiply-add; for k = 1 u = gw x is
     one more rounding, 2^-24 |a u|, still inside the band's 4 u24);
  2. the channel that holds the maximum of a map position: the largest G leads the runner-up by >= 2 KINK (|a u| + |b|) of the leader
     (raise_leader lifts the leader's u where it does not);
  3. SE's h > 0: |Wa gap| >= 2^-12 sum |wa gap| for every hidden unit (se_inputs).
Planted on purpose: map positions where every channel is negative (gmax = 0, d_rfa = 0, dv = 0 for every channel although G == gmax holds
for all of them), all-negative channels, SE hidden units that are clearly off, and for C >= 128 a whole wave of 64 channels with a < 0,
b = -0.0, u = +0 at tap KK / 2: fma gives -0.0 there, and ly_rf_bwd_attn takes gmax with an integer atomicMax on the float's bits, under
which -0.0 (0x80000000) would beat every positive maximum.  An exact tie of two POSITIVE maxima is not a case: autograd gives d_max to one
index, the kernels to every tied channel; the margin of decision 2 keeps ties out of the inputs.

Bounds (u24 = 2^-24), the forms of bnact_ref
  elementwise   |got - want| <= u24 (K M + L T) [+ 2^-8 |want| for a result stored as bf16]     (judge_elem with M + L / K T as its M)
  sums          |got - want| <= u24 (L sum |term| + K sum M_term)                                 (judge_sum)
  M: the sum of the magnitudes of the terms with every intermediate carried with ITS terms: M_G = (|a u| + |b|) [G > 0];
  M_dv = |dcd rfa ca| + |d_mean| / C + [max] |d_max|; M_dug = |alpha dv| + |kappa| + |lambda u|; sums of products use the products themselves.
  L: the longest fp32 addition chain, from the code (the geometry functions below restate the launch arithmetic):
    ug            KK + 1 (one accumulator over the KK taps)
    d_rfa         ly_rf_bwd_attn: 6 (wave shuffle tree) + ceil(C / 64) float atomics + 1; ly_rf3s_bwd / ly_rf1_bwd: VW per lane + log2(lpp2)
    d_ca          ly_rf_bwd_attn: KK ceil(chunk / subs) per thread + one float atomic per block (gx) + 1;
                  ly_rf3s_bwd: ceil(chunk / pp) per lane + the 9 pp slots of the LDS fold; ly_rf1_bwd: ceil(chunk / PB) + PB; doubles after that
    s1 / s2       ly_rf_bwd_relu: ceil(chunk / subs) (rf_geom with 512 blocks) + gx float atomics + 1 (the product);
                  ly_rf3s_bwd: ceil(chunk / pp) + pp + 1; ly_rf1_bwd: ceil(chunk / PB) + PB + 1; the stripes are doubles
    d_mm          9 + 1;   dw18: 4 positions x ceil(tiles / blocks) per thread + 6 + 3 (wave tree, four waves) + blocks float atomics + 1
                  (a float64 target: no rounding from the atomics), blocks = min(tiles, 512)
    dwg           ceil(chunk / subs) + 1 per row of partial sums (rf_geom with part_rows / subs blocks); the rows are folded in float64
    dx            KK x the (m, u) pairs of an input pixel (ceil(k / s)^2) + 2
    dgw (k = 1)   ceil(chunk / PB) + PB + (the blocks' float atomics: grid x n, fp32 target only) + 1
    ly_se_bwd     gap: ceil(slices / ng) + ng + 1;  h, dh: ceil(C / 64) + 6 + 1;  dgap: R;  dWa / dWb: n_img + 1 (in image order, the eight-image
                  trips keep it) — each intermediate's chain enters the M of what is built on it (se_bwd_mag)
  K, per reference: the SAME references evaluated in torch float32 on the CPU against float64 over every case of the tables (measure_k), the
      worst err / (u24 M) times 4 (v_rcp / v_exp at one ulp each, fused against separate multiply-add), rounded up; tests/test_rfcbam_host.py
      re-measures and holds 4 x worst <= K.  The device's own figures never enter a bound.
        worst ratio   gen 3.21   G 3.57   dv 2.78   dug 2.57   dx 3.01   dmm 4.17   se 0.93   rf1 4.29
        K             gen 13     G 15     dv 12     dug 11     dx 13     dmm 17     se 4      rf1 18
"""
import math

import torch
import torch.nn.functional as F

from tests.bnact_ref import (ACT_RELU, BF16, BF16_EPS, F32, KINK, U24, _fail, _seed, apply, coeffs, d, fold, in_band, judge_channels,  # noqa: F401
                             judge_elem, judge_sum, nudge, reduce, sum_rows_chain)

K = dict(gen=13.0, G=15.0, dv=12.0, dug=11.0, dx=13.0, dmm=17.0, se=4.0, rf1=18.0)
THREADS = 256
SE_MARGIN = 2.0 ** -12
EPS = 1e-3                                       # the BatchNorms of chain_parts: oracle.functional.BN_EPS


def _cdiv(a, b):
    return -(-a // b)


def vw_of(dtype):
    return 8 if dtype == BF16 else 4


# ---------------------------------------------------------------- layouts -----------------------------------------------------------------
def out_hw(h, w, k, s):
    p = k // 2
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def taps(x, k, s, clamp=False):
    """x [n, H, W, C] -> the KK input taps of every output pixel [m, u, C], zero padded.  clamp: the DEFECT of a clamped border"""
    n, h, w, c = x.shape
    p = k // 2
    ho, wo = out_hw(h, w, k, s)
    xp = F.pad(x.permute(0, 3, 1, 2), (p, p, p, p), mode="replicate" if (clamp and p) else "constant")
    cols = [xp[:, :, uy:uy + s * (ho - 1) + 1:s, ux:ux + s * (wo - 1) + 1:s] for uy in range(k) for ux in range(k)]
    return torch.stack(cols, 0).permute(1, 3, 4, 0, 2).reshape(n * ho * wo, k * k, c)


def to_map(e, n, ho, wo, k, swap=False):
    """per-(m, t) values [m, KK] -> the map [n, k Ho, k Wo] (rf_pos).  swap: the DEFECT tx <-> ty"""
    v = e.reshape(n, ho, wo, k, k)
    if swap:
        v = v.transpose(3, 4)
    return v.permute(0, 1, 3, 2, 4).reshape(n, k * ho, k * wo)


def from_map(mp, n, ho, wo, k, swap=False):
    v = mp.reshape(n, ho, k, wo, k).permute(0, 1, 3, 2, 4)
    if swap:
        v = v.transpose(3, 4)
    return v.reshape(n * ho * wo, k * k)


def _exp(ca, rfa, n, ho, wo, k, swap=False):
    """ca [n, C] and the map rfa as factors of an expanded tensor: [m, 1, C], [m, KK, 1]"""
    return ca.repeat_interleave(ho * wo, 0).unsqueeze(1), from_map(rfa, n, ho, wo, k, swap).unsqueeze(-1)


def gact(u, a, b):
    """(G, M_G) of G = relu(a u + b)"""
    v = a * u + b
    on = (v > 0).to(u.dtype)
    return torch.clamp(v, min=0.0), ((a * u).abs() + b.abs()) * on


# ---------------------------------------------------------------- references -------------------------------------------------------------
def generate(x, wg, k, s, clamp=False):
    """ly_rf_generate: ug[m][t][c] = sum_u wg[c KK + t][u] x_u(m)[c]"""
    c, kk = x.shape[-1], k * k
    return torch.einsum("ctu,muc->mtc", wg.reshape(c, kk, kk), taps(x, k, s, clamp))


def generate_mag(x, wg, k, s):
    return generate(x.abs(), wg.abs(), k, s)


def attn(ug, dcd, ag, bg, ca, rfa, n, ho, wo, k, swap_pos=False):
    """ly_rf_bwd_attn / ly_rf3s_bwd pass 0: dict(cd, d_rfa, gmax, d_ca).  swap_pos: the DEFECT rf_pos with tx and ty exchanged"""
    g, _ = gact(ug, ag, bg)
    cae, re = _exp(ca, rfa, n, ho, wo, k, swap_pos)
    c = ug.shape[-1]
    return dict(cd=g * cae * re, d_rfa=to_map((dcd * g * cae).sum(-1), n, ho, wo, k, swap_pos), gmax=to_map(g.amax(-1), n, ho, wo, k, swap_pos),
                d_ca=(dcd * re * g).reshape(n, -1, c).sum(1))


def attn_mag(ug, dcd, ag, bg, ca, rfa, n, ho, wo, k):
    """cd, gmax: M; d_rfa, d_ca: (sum |term|, sum M_term)"""
    g, mg = gact(ug, ag, bg)
    cae, re = _exp(ca, rfa, n, ho, wo, k)
    c = ug.shape[-1]
    lead = torch.gather(mg, 2, g.argmax(-1, keepdim=True)).squeeze(-1)
    mp = lambda e: to_map(e, n, ho, wo, k)
    img = lambda e: e.reshape(n, -1, c).sum(1)
    return dict(cd=mg * cae * re.abs(), gmax=mp(lead), d_rfa=(mp((dcd.abs() * g * cae).sum(-1)), mp((dcd.abs() * mg * cae).sum(-1))),
                d_ca=(img(dcd.abs() * re.abs() * g), img(dcd.abs() * re.abs() * mg)))


def _shift(t, dy, dx):
    """s[q] = t[q + (dy, dx)], zero outside the map; t [n, Hk, Wk]"""
    h, w = t.shape[1:]
    p = F.pad(t, (1, 1, 1, 1))
    return p[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


def getw_fwd(mm, w18):
    """rfa = sigmoid(pre), pre[p] = sum w[ch][dy][dx] mm[p + (dy - 1, dx - 1)][ch]"""
    w = w18.reshape(2, 3, 3)
    return torch.sigmoid(sum(w[ch, dy, dx] * _shift(mm[..., ch], dy - 1, dx - 1) for ch in range(2) for dy in range(3) for dx in range(3)))


def getw_bwd(d_rfa, rfa, mm, w18, no_flip=False):
    """ly_rfa_bwd: dict(d_mm [n, Hk, Wk, 2], dw18 [18]) through the sigmoid and the zero-padded 3x3 conv 2 -> 1.
    no_flip: the DEFECT of d_mm gathered with the forward's offsets (the conv not flipped)"""
    dpre = d_rfa * rfa * (1 - rfa)
    w = w18.reshape(2, 3, 3)
    sg = 1 if no_flip else -1
    d_mm = torch.stack([sum(w[ch, dy, dx] * _shift(dpre, sg * (dy - 1), sg * (dx - 1)) for dy in range(3) for dx in range(3)) for ch in range(2)], -1)
    dw = torch.stack([(dpre * _shift(mm[..., ch], dy - 1, dx - 1)).sum() for ch in range(2) for dy in range(3) for dx in range(3)])
    return dict(d_mm=d_mm, dw18=dw)


def getw_bwd_mag(d_rfa, rfa, mm, w18):
    """d_mm: sum |w d_pre|; dw18: sum |d_pre mm| (d_pre = d_rfa rfa (1 - rfa): three roundings of itself, inside K)"""
    dpre = (d_rfa * rfa * (1 - rfa)).abs()
    w = w18.reshape(2, 3, 3).abs()
    d_mm = torch.stack([sum(w[ch, dy, dx] * _shift(dpre, -(dy - 1), -(dx - 1)) for dy in range(3) for dx in range(3)) for ch in range(2)], -1)
    dw = torch.stack([(dpre * _shift(mm[..., ch].abs(), dy - 1, dx - 1)).sum() for ch in range(2) for dy in range(3) for dx in range(3)])
    return dict(d_mm=d_mm, dw18=dw)


def relu(ug, dcd, ag, bg, ca, rfa, d_mm, n, ho, wo, k, sums_dtype=None, no_guard=False, no_mean=False):
    """ly_rf_bwd_relu / ly_rf3s_bwd pass 1: dict(dv, s1, s2 [KK, C]); dv = [G > 0] (dcd rfa ca + d_mean / C + [G == gmax] d_max), the sums from
    the UNROUNDED dv.  DEFECTS: sums_dtype (the sums taken from dv rounded to that type), no_guard (d_max also routed where G = 0: every channel
    of an all-negative position equals gmax = 0), no_mean (d_mean / C dropped)"""
    g, _ = gact(ug, ag, bg)
    cae, re = _exp(ca, rfa, n, ho, wo, k)
    c = ug.shape[-1]
    ismax = (g == g.amax(-1, keepdim=True)).to(ug.dtype)
    dmax, dmean = from_map(d_mm[..., 0], n, ho, wo, k).unsqueeze(-1), from_map(d_mm[..., 1], n, ho, wo, k).unsqueeze(-1)
    dg = dcd * re * cae + (0.0 if no_mean else dmean / c) + ismax * dmax
    dv = torch.where(g > 0, dg, ismax * dmax if no_guard else torch.zeros_like(dg))
    sv = dv if sums_dtype is None else dv.to(sums_dtype).to(dv.dtype)
    return dict(dv=dv, s1=sv.sum(0), s2=(sv * ug).sum(0))


def relu_mag(ug, dcd, ag, bg, ca, rfa, d_mm, n, ho, wo, k):
    """dv: M; s1, s2: (sum |term|, sum M_term)"""
    g, _ = gact(ug, ag, bg)
    cae, re = _exp(ca, rfa, n, ho, wo, k)
    c = ug.shape[-1]
    ismax = (g == g.amax(-1, keepdim=True)).to(ug.dtype)
    dmax, dmean = from_map(d_mm[..., 0], n, ho, wo, k).unsqueeze(-1), from_map(d_mm[..., 1], n, ho, wo, k).unsqueeze(-1)
    m = ((dcd * re * cae).abs() + dmean.abs() / c + ismax * dmax.abs()) * (g > 0).to(ug.dtype)
    dv = relu(ug, dcd, ag, bg, ca, rfa, d_mm, n, ho, wo, k)["dv"].abs()
    return dict(dv=m, s1=(dv.sum(0), m.sum(0)), s2=((dv * ug.abs()).sum(0), (m * ug.abs()).sum(0)))


def gen(xt, ug, dv, alpha, kappa, lam):
    """ly_rf_bwd_gen: dict(dug, dwg [C, KK (t), KK (u)]); xt = taps(x) [m, u, C]"""
    dug = alpha * dv + kappa + lam * ug
    return dict(dug=dug, dwg=torch.einsum("mtc,muc->ctu", dug, xt))


def gen_mag(xt, ug, dv, alpha, kappa, lam):
    """dug: M; dwg: (sum |term|, sum M_term)"""
    m = (alpha * dv).abs() + kappa.abs() + (lam * ug).abs()
    dug = (alpha * dv + kappa + lam * ug).abs()
    return dict(dug=m, dwg=(torch.einsum("mtc,muc->ctu", dug, xt.abs()), torch.einsum("mtc,muc->ctu", m, xt.abs())))


def dx(dug, wg, n, h, w, k, s, addnc=None, add_scale=1.0, next_image_chunk=None, drop_halo=None):
    """ly_rf_bwd_dx: dx[n, hi, wi, c] = sum over the (m, u) that read this input pixel of sum_t dug[m][t][c] wg[c][t][u] + addnc[n][c] add_scale.
    DEFECTS: next_image_chunk = the block's pixel chunk: a pixel of the chunk's SECOND image takes the addend of the neighbouring (first) image;
    drop_halo = TM: the halo row and column of the LDS tile (the output pixels below / right of the tile, which the tile's last odd input row /
    column also take from) dropped"""
    c, kk = dug.shape[-1], k * k
    p = k // 2
    ho, wo = out_hw(h, w, k, s)
    g = torch.einsum("mtc,ctu->muc", dug, wg.reshape(c, kk, kk)).reshape(n, ho, wo, kk, c)
    if drop_halo:
        g = g.clone()
        g[:, (torch.arange(ho) % drop_halo == 0) & (torch.arange(ho) > 0), :, 0:k] = 0.0        # uy = 0: input row 2 ho - 1, the last row of the tile above
        g[:, :, (torch.arange(wo) % drop_halo == 0) & (torch.arange(wo) > 0), 0::k] = 0.0       # ux = 0: the column halo likewise
    out = torch.zeros(n, h + 2 * p + s, w + 2 * p + s, c, dtype=dug.dtype)
    for uy in range(k):
        for ux in range(k):
            out[:, uy:uy + s * (ho - 1) + 1:s, ux:ux + s * (wo - 1) + 1:s] += g[:, :, :, uy * k + ux]
    out = out[:, p:p + h, p:p + w].clone()
    if addnc is not None:
        img = torch.arange(n).view(n, 1).expand(n, h * w).clone()
        if next_image_chunk:
            pix = torch.arange(n * h * w).view(n, h * w)
            first = (pix // next_image_chunk * next_image_chunk) // (h * w)
            img = first
        out = out + (addnc * add_scale)[img.reshape(-1)].view(n, h, w, c)
    return out


def dx_mag(dug, wg, n, h, w, k, s, addnc=None, add_scale=1.0):
    return dx(dug.abs(), wg.abs(), n, h, w, k, s, None if addnc is None else addnc.abs(), abs(add_scale))


def se_bwd(part, ca, d_ca, wa, wb, hw, no_mask=False):
    """ly_se_bwd: dict(dgap [n, C], dWa [R, C], dWb [C, R]) and the intermediates.  no_mask: the DEFECT dh without [h > 0]"""
    gap = part.sum(1) / hw
    pre = gap @ wa.t()
    h = torch.clamp(pre, min=0.0)
    dz = d_ca * ca * (1 - ca)
    dh = dz @ wb
    if not no_mask:
        dh = dh * (pre > 0).to(dh.dtype)
    return dict(dgap=dh @ wa, dWa=dh.t() @ gap, dWb=dz.t() @ h, gap=gap, pre=pre, h=h, dz=dz, dh=dh)


def se_bwd_mag(part, ca, d_ca, wa, wb, hw, chains=None):
    """dgap, dWa, dWb: (sum |term|, sum M_term).  chains = se_chains(...): each intermediate's own addition chain enters its M as L / K of its
    terms; None: the plain magnitudes (measure_k: torch's float32 matmuls carry their own, shorter chains)"""
    ch = chains or dict(gap=0, dot=0)
    lg, ld = ch["gap"] / K["se"], ch["dot"] / K["se"]
    o = se_bwd(part, ca, d_ca, wa, wb, hw)
    on = (o["pre"] > 0).to(part.dtype)
    m_gap = (1 + lg) * part.abs().sum(1) / hw
    m_h = ((1 + ld) * (o["gap"].abs() @ wa.abs().t()) + m_gap @ wa.abs().t()) * on
    m_dz = o["dz"].abs()
    m_dh = ((1 + ld) * (o["dz"].abs() @ wb.abs()) + m_dz @ wb.abs()) * on
    return dict(dgap=(o["dh"].abs() @ wa.abs(), m_dh @ wa.abs()),
                dWa=(o["dh"].abs().t() @ o["gap"].abs(), m_dh.t() @ o["gap"].abs() + o["dh"].abs().t() @ m_gap),
                dWb=(o["dz"].abs().t() @ o["h"], m_dz.t() @ o["h"] + o["dz"].abs().t() @ m_h))


def _k1(x, dcd, gw, ag, bg, rfa, n, hw):
    """the k = 1 passes in the general references' layouts: u = gw x, one tap, maps [n, HW, 1]"""
    return (gw * x).unsqueeze(1), dcd.unsqueeze(1), ag.view(1, -1), bg.view(1, -1), rfa.reshape(n, hw, 1)


def rf1_a(x, dcd, gw, ag, bg, ca, rfa, n, hw):
    """ly_rf1_bwd pass 0 (G recomputed from x [n HW, C]): dict(cd [n HW, C], d_rfa, gmax [n HW], d_ca [n, C])"""
    u, dc, a, b, r = _k1(x, dcd, gw, ag, bg, rfa, n, hw)
    o = attn(u, dc, a, b, ca, r, n, hw, 1, 1)
    return dict(cd=o["cd"][:, 0], d_rfa=o["d_rfa"].reshape(-1), gmax=o["gmax"].reshape(-1), d_ca=o["d_ca"])


def rf1_a_mag(x, dcd, gw, ag, bg, ca, rfa, n, hw):
    u, dc, a, b, r = _k1(x, dcd, gw, ag, bg, rfa, n, hw)
    o = attn_mag(u, dc, a, b, ca, r, n, hw, 1, 1)
    return dict(cd=o["cd"][:, 0], gmax=o["gmax"].reshape(-1), d_rfa=tuple(t.reshape(-1) for t in o["d_rfa"]), d_ca=o["d_ca"])


def rf1_b(x, dcd, gw, ag, bg, ca, rfa, d_mm, n, hw, **defects):
    """ly_rf1_bwd pass 1: dict(dv [n HW, C], s1, s2 [C])"""
    u, dc, a, b, r = _k1(x, dcd, gw, ag, bg, rfa, n, hw)
    o = relu(u, dc, a, b, ca, r, d_mm.reshape(n, hw, 1, 2), n, hw, 1, 1, **defects)
    return dict(dv=o["dv"][:, 0], s1=o["s1"][0], s2=o["s2"][0])


def rf1_b_mag(x, dcd, gw, ag, bg, ca, rfa, d_mm, n, hw):
    u, dc, a, b, r = _k1(x, dcd, gw, ag, bg, rfa, n, hw)
    o = relu_mag(u, dc, a, b, ca, r, d_mm.reshape(n, hw, 1, 2), n, hw, 1, 1)
    return dict(dv=o["dv"][:, 0], s1=tuple(t[0] for t in o["s1"]), s2=tuple(t[0] for t in o["s2"]))


def rf1_c(x, dcd, gw, ag, bg, ca, rfa, d_mm, alpha, kappa, lam, dgap, scale, n, hw, no_scale=False):
    """ly_rf1_bwd pass 2: dict(dx [n HW, C], dgw [C]); dgap None: no addend.  no_scale: the DEFECT dgap added without dgap_scale"""
    dv = rf1_b(x, dcd, gw, ag, bg, ca, rfa, d_mm, n, hw)["dv"]
    du = alpha * dv + kappa + lam * (gw * x)
    out = du * gw
    if dgap is not None:
        out = out + (dgap * (1.0 if no_scale else scale)).repeat_interleave(hw, 0)
    return dict(dx=out, dgw=(du * x).sum(0), du=du)


def rf1_c_mag(x, dcd, gw, ag, bg, ca, rfa, d_mm, alpha, kappa, lam, dgap, scale, n, hw):
    """dx: M; dgw: (sum |term|, sum M_term)"""
    m_dv = rf1_b_mag(x, dcd, gw, ag, bg, ca, rfa, d_mm, n, hw)["dv"]
    du = rf1_c(x, dcd, gw, ag, bg, ca, rfa, d_mm, alpha, kappa, lam, dgap, scale, n, hw)["du"]
    m_du = alpha.abs() * m_dv + kappa.abs() + (lam * gw * x).abs()
    m = m_du * gw.abs()
    if dgap is not None:
        m = m + (dgap * scale).abs().repeat_interleave(hw, 0)
    return dict(dx=m, dgw=((du * x).abs().sum(0), (m_du * x.abs()).sum(0)))


# ---------------------------------------------------------------- the whole module: stages composed, and autograd -------------------------
def chain_params(g, c, o, k, r):
    """the module's parameters (float64) in the reference's own shapes"""
    kk = k * k
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ru = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    return dict(wa=rn(r, c) / math.sqrt(c), wb=rn(c, r), gen_w=rn(c * kk, 1, k, k) * 0.5, gen_gamma=ru(c * kk) + 0.5, gen_beta=rn(c * kk) * 0.3,
                getw=rn(1, 2, 3, 3) * 0.5, conv_w=rn(o, c, k, k) / math.sqrt(c * kk), conv_b=rn(o) * 0.1, out_gamma=ru(o) + 0.5, out_beta=rn(o) * 0.3)


GRADS = ("dx", "wa", "wb", "gen_w", "gen_gamma", "gen_beta", "getw", "conv_w", "conv_b", "out_gamma", "out_beta")


def chain_autograd(x, p, r, k, s):
    """oracle.functional.rfcbam(training=True) under float64 autograd, loss = sum(y r).  x [n, H, W, C], r [n, Ho, Wo, O] -> dict over GRADS + y"""
    from oracle import functional as OF
    leaves = {key: v.clone().requires_grad_(True) for key, v in p.items()}
    xx = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    c, o = x.shape[-1], p["conv_w"].shape[0]
    names = {"m.se.fc.0.weight": "wa", "m.se.fc.2.weight": "wb", "m.generate.0.weight": "gen_w", "m.generate.1.weight": "gen_gamma",
             "m.generate.1.bias": "gen_beta", "m.get_weight.0.weight": "getw", "m.conv.0.weight": "conv_w", "m.conv.0.bias": "conv_b",
             "m.conv.1.weight": "out_gamma", "m.conv.1.bias": "out_beta"}
    st = {name: leaves[key] for name, key in names.items()}
    for pre, ch in (("m.generate.1.", c * k * k), ("m.conv.1.", o)):
        st[pre + "running_mean"], st[pre + "running_var"] = torch.zeros(ch, dtype=torch.float64), torch.ones(ch, dtype=torch.float64)
    y = OF.rfcbam(st, "m.", xx, k, s, training=True)
    (y * r.permute(0, 3, 1, 2)).sum().backward()
    out = {key: leaves[key].grad for key in p}
    out.update(dx=xx.grad.permute(0, 2, 3, 1), y=y.detach().permute(0, 2, 3, 1))
    return out


def _bn(t, gamma, beta):
    """batch statistics over dim 0 -> (a, b, mean, invstd)"""
    mean = t.mean(0)
    invstd = 1 / torch.sqrt(((t - mean) ** 2).mean(0) + EPS)
    return gamma * invstd, beta - mean * gamma * invstd, mean, invstd


def chain_parts(x, p, r, k, s, route):
    """the module composed of this file's stage references in the order of grad._rfcbam_backward_streamed (route "streamed") or
    grad._rfcbam_backward_k1 (route "k1"); the GEMM-shaped steps are float64 matmuls, the BatchNorms bnact_ref's reduce / coeffs / apply"""
    n, h, w, c = x.shape
    kk, o = k * k, p["conv_w"].shape[0]
    ho, wo = out_hw(h, w, k, s)
    mo = n * ho * wo
    wg = p["gen_w"].reshape(c * kk, kk)
    tc = lambda v: v.view(c, kk).t()                                 # a per-(c, t) parameter in the kernels' [t][c] order
    # forward
    xt = taps(x, k, s)
    ug = generate(x, wg, k, s)
    ag, bg, gmean, ginv = _bn(ug, tc(p["gen_gamma"]), tc(p["gen_beta"]))
    g, _ = gact(ug, ag, bg)
    mm = torch.stack((to_map(g.amax(-1), n, ho, wo, k), to_map(g.mean(-1), n, ho, wo, k)), -1)
    w18 = p["getw"].reshape(18)
    rfa = getw_fwd(mm, w18)
    part = x.reshape(n, 1, h * w, c).sum(2)                           # one slice of pooling partials
    ca = torch.sigmoid(torch.clamp(part.sum(1) / (h * w) @ p["wa"].t(), min=0.0) @ p["wb"].t())
    cae, re = _exp(ca, rfa, n, ho, wo, k)
    wc = p["conv_w"].permute(0, 2, 3, 1).reshape(o, kk * c)           # rows (t, c)
    u = (g * cae * re).reshape(mo, kk * c) @ wc.t() + p["conv_b"]
    ao, bo, omean, oinv = _bn(u, p["out_gamma"], p["out_beta"])
    y = torch.clamp(ao * u + bo, min=0.0)
    # backward: output BatchNorm + ReLU, then the stages
    dy = r.reshape(mo, o)
    s1, s2 = reduce(dy, u, ao, bo, ACT_RELU)
    co = coeffs(s1, s2, float(mo), ao, omean, oinv, True)
    du = apply(dy, u, ao, bo, ACT_RELU, co["alpha"], co["kappa"], co["lam"])
    dcd = (du @ wc).reshape(mo, kk, c)
    out = dict(y=y.reshape(n, ho, wo, o), out_gamma=co["dgamma"], out_beta=co["dbeta"], conv_b=du.sum(0))
    if route == "streamed":
        a = attn(ug, dcd, ag, bg, ca, rfa, n, ho, wo, k)
        gwb = getw_bwd(a["d_rfa"], rfa, mm, w18)
        rl = relu(ug, dcd, ag, bg, ca, rfa, gwb["d_mm"], n, ho, wo, k)
        cg = coeffs(rl["s1"].reshape(-1), rl["s2"].reshape(-1), float(mo), ag.reshape(-1), gmean.reshape(-1), ginv.reshape(-1), True)
        al, ka, la = (cg[q].view(kk, c) for q in ("alpha", "kappa", "lam"))
        gn = gen(xt, ug, rl["dv"], al, ka, la)
        se = se_bwd(part, ca, a["d_ca"], p["wa"], p["wb"], h * w)
        out.update(dx=dx(gn["dug"], wg, n, h, w, k, s, se["dgap"], 1.0 / (h * w)), gen_w=gn["dwg"].reshape(p["gen_w"].shape), cd=a["cd"])
        out.update(gen_gamma=cg["dgamma"].view(kk, c).t().reshape(-1), gen_beta=cg["dbeta"].view(kk, c).t().reshape(-1))
    else:
        assert k == 1 and s == 1
        xf, dc, gw = x.reshape(mo, c), dcd[:, 0], p["gen_w"].reshape(c)
        a1, b1, rf = ag[0], bg[0], rfa.reshape(-1)
        a = rf1_a(xf, dc, gw, a1, b1, ca, rf, n, h * w)
        gwb = getw_bwd(a["d_rfa"].view(n, h, w), rfa, mm, w18)
        rb = rf1_b(xf, dc, gw, a1, b1, ca, rf, gwb["d_mm"].reshape(-1, 2), n, h * w)
        cg = coeffs(rb["s1"], rb["s2"], float(mo), a1, gmean[0], ginv[0], True)
        se = se_bwd(part, ca, a["d_ca"], p["wa"], p["wb"], h * w)
        rc = rf1_c(xf, dc, gw, a1, b1, ca, rf, gwb["d_mm"].reshape(-1, 2), cg["alpha"], cg["kappa"], cg["lam"], se["dgap"], 1.0 / (h * w), n, h * w)
        out.update(dx=rc["dx"].view(n, h, w, c), gen_w=rc["dgw"].reshape(p["gen_w"].shape), gen_gamma=cg["dgamma"], gen_beta=cg["dbeta"], cd=a["cd"].unsqueeze(1))
    out.update(wa=se["dWa"], wb=se["dWb"], getw=gwb["dw18"].reshape(p["getw"].shape),
               conv_w=(du.t() @ out["cd"].reshape(mo, kk * c)).view(o, k, k, c).permute(0, 3, 1, 2))
    return out


# ---------------------------------------------------------------- geometry (from the code) -----------------------------------------------
def rf_geom(n, h, w, c, k, s, pixels=None, max_blocks=2048):
    """rf_geom of csrc/ly_rfcbam_bwd.hip: dict(cb, subs, gy, chunk, gx, threads = the live threads of a block); pixels: output pixels unless given"""
    ho, wo = out_hw(h, w, k, s)
    pixels = n * ho * wo if pixels is None else pixels
    cb = (min(c, 256) + 63) // 64 * 64
    subs = THREADS // cb
    gy = _cdiv(c, cb)
    chunk = max(_cdiv(pixels, max_blocks // gy), 8 * subs)
    chunk = _cdiv(chunk, subs) * subs
    return dict(cb=cb, subs=subs, gy=gy, chunk=chunk, gx=_cdiv(pixels, chunk), threads=subs * cb, ho=ho, wo=wo, clamped=gy * cb - c)


def gen_geom(n, h, w, c, k, s, part_rows):
    """ly_rf_bwd_gen: rf_geom with part_rows / subs blocks; every (block, sub-group) owns one row"""
    cb = (min(c, 256) + 63) // 64 * 64
    subs, groups = THREADS // cb, _cdiv(c, 256)
    g = rf_geom(n, h, w, c, k, s, max_blocks=(part_rows // subs) * groups)
    assert g["gx"] * g["subs"] <= part_rows
    return g


def dx_geom(n, h, w, c, k, s, dtype, addend=True):
    """ly_rf_bwd_dx: rf_geom over the INPUT pixels + `form`: "s2t" (the LDS-tiled kernel: k = 3, stride 2, even H and W, C a multiple of 8; with
    tiles_y, tiles_x, cgroups) or the addend form 0 / 1 / 2 of the generic kernel (2: the chunk touches at most two images) and `gather`"""
    g = rf_geom(n, h, w, c, k, s, pixels=n * h * w)
    if k == 3 and s == 2 and h % 2 == 0 and w % 2 == 0 and c % 8 == 0:
        tm = 4
        g.update(form="s2t", tiles_y=_cdiv(h // 2, tm), tiles_x=_cdiv(w // 2, tm), cgroups=_cdiv(c, 64), tm=tm)
    else:
        g.update(form=(0 if not addend else (2 if g["chunk"] <= h * w else 1)), gather="parity" if (k == 3 and s == 2) else "generic")
    return g


def dx_chain(k, s):
    return k * k * _cdiv(k, s) ** 2 + 2


def _pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def rf3s_geom(n, hw, c, dtype):
    """launch arithmetic of ly_rf3s_bwd"""
    lpp = c // vw_of(dtype)
    lpp2 = _pow2(lpp)
    pp = min(max(576 // (9 * lpp2), 1), 4)
    per_img = max(min(_cdiv(1024, n), _cdiv(hw, 2 * pp)), 1)
    chunk = _cdiv(_cdiv(hw, per_img), pp) * pp
    return dict(lpp=lpp, lpp2=lpp2, pp=pp, threads=9 * lpp2 * pp, chunk=chunk, grid=(_cdiv(hw, chunk), n))


def rf1_geom(n, hw, c, dtype):
    """rf1_launch of csrc/ly_rf1_bwd.hip"""
    lpp = c // vw_of(dtype)
    lpp2 = _pow2(lpp)
    pb = THREADS // lpp2
    per_img = max(min(_cdiv(1536, n), _cdiv(hw, 4 * pb)), 1)
    chunk = _cdiv(_cdiv(hw, per_img), pb) * pb
    return dict(lpp=lpp, lpp2=lpp2, pb=pb, chunk=chunk, grid=(_cdiv(hw, chunk), n))


def rfa_geom(n, hk, wk):
    """ly_rfa_bwd: 16 x 64 tiles, at most 512 blocks"""
    ty, tx = _cdiv(hk, 16), _cdiv(wk, 64)
    tiles = n * ty * tx
    return dict(tiles_y=ty, tiles_x=tx, tiles=tiles, blocks=min(tiles, 512))


def rfa_chain(n, hk, wk, f64):
    g = rfa_geom(n, hk, wk)
    return 4 * _cdiv(g["tiles"], g["blocks"]) + 9 + (0 if f64 else g["blocks"]) + 1


def se_chains(n, c, r, slices):
    """ly_se_bwd: nq = C / 4 lanes per slice group, ng = 256 / nq groups"""
    nq = c // 4
    ng = THREADS // nq
    return dict(nq=nq, ng=ng, gap=_cdiv(slices, ng) + ng + 1, dot=_cdiv(c, 64) + 6 + 1, dgap=r, dw=n + 1, trips=n // 8, tail=n % 8)


def attn_chains(kind, n, ho, wo, c, k, dtype, h=None, w=None, s=None):
    """(L of d_rfa, L of d_ca, L of s1 / s2) of the kernel `kind` = "tc" (ly_rf_bwd_attn / ly_rf_bwd_relu), "rf3s", "rf1" """
    if kind == "tc":
        ga, gr = rf_geom(n, h, w, c, k, s), rf_geom(n, h, w, c, k, s, max_blocks=512)
        return 6 + _cdiv(c, 64) + 1, k * k * _cdiv(ga["chunk"], ga["subs"]) + ga["gx"] + 1, _cdiv(gr["chunk"], gr["subs"]) + gr["gx"] + 1
    if kind == "rf3s":
        g = rf3s_geom(n, ho * wo, c, dtype)
        return vw_of(dtype) + int(math.log2(g["lpp2"])), _cdiv(g["chunk"], g["pp"]) + 9 * g["pp"], _cdiv(g["chunk"], g["pp"]) + g["pp"] + 1
    g = rf1_geom(n, ho * wo, c, dtype)
    return vw_of(dtype) + int(math.log2(g["lpp2"])), _cdiv(g["chunk"], g["pb"]) + g["pb"], _cdiv(g["chunk"], g["pb"]) + g["pb"] + 1


# ---------------------------------------------------------------- judges ------------------------------------------------------------------
def _say(what, **ratios):
    """every judge below prints its figures BEFORE it asserts"""
    print(f"{what}: " + "  ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    return ratios


def elem_ratio(got, want, mag, bf16=False):
    """for the record: the worst (|err| - storage allowance) / (u24 M)"""
    err = (d(got).reshape(want.shape) - want).abs() - (BF16_EPS * want.abs() if bf16 else 0.0)
    return float((err.clamp(min=0.0) / (U24 * mag).clamp(min=1e-300))[mag > 0].max()) if bool((mag > 0).any()) else 0.0


def sum_ratio(got, want, chain, term_abs, term_mag, k):
    """for the record: the worst |err| / bound of a sum"""
    bound = U24 * (chain * term_abs + k * term_mag)
    err = (d(got).reshape(want.shape) - want).abs()
    return float((err / bound.clamp(min=1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0


def _elem(got, want, mag, key, what, bf16=False, chain=0.0, terms=None):
    """elementwise: u24 (K M + L T) [+ 2^-8 |want|]; exact zeros of M must be exact zeros"""
    got = d(got).reshape(want.shape)
    m = mag + (chain / K[key]) * (mag if terms is None else terms)
    return judge_elem(got, want, (m, torch.zeros_like(m)), what, bf16=bf16, k=K[key])


def _sum(got, want, chain, tm, key, what):
    judge_sum(d(got).reshape(want.shape), want, chain, tm[0], tm[1], what, k=K[key])


def judge_generate(ug, x, what):
    """x: dict(x, wg, k, s) as stored"""
    a = (d(x["x"]), d(x["wg"]), x["k"], x["s"])
    bf = x["x"].dtype == BF16
    want, mag = generate(*a), generate_mag(*a)
    out = _say(what, gen=elem_ratio(ug, want, mag, bf))
    _elem(ug, want, mag, "gen", what + " ug", bf16=bf, chain=x["k"] ** 2 + 1)
    return out


ATTN_KEYS = ("ug", "dcd", "ag", "bg", "ca", "rfa")


def _stage_args(x, keys):
    return [d(x[q]) for q in keys] + [x["n"], x["ho"], x["wo"], x["k"]]


def judge_attn(got, x, chains, what, keys=("cd", "d_rfa", "gmax", "d_ca")):
    """got: dict(cd [m, KK, C], d_rfa, gmax maps, d_ca [n, C]); chains = attn_chains(...)"""
    a = _stage_args(x, ATTN_KEYS)
    bf = x["ug"].dtype == BF16
    want, mag = attn(*a), attn_mag(*a)
    out = _say(what, G=max(elem_ratio(got["cd"], want["cd"], mag["cd"], bf) if "cd" in keys else 0.0,
                          elem_ratio(got["gmax"], want["gmax"], mag["gmax"]) if "gmax" in keys else 0.0),
               sums_err_over_bound=max([sum_ratio(got[q], want[q], chains[i], *mag[q], K["G"]) for i, q in ((0, "d_rfa"), (1, "d_ca")) if q in keys] + [0.0]))
    if "cd" in keys:
        _elem(got["cd"], want["cd"], mag["cd"], "G", what + " cd", bf16=bf)
    if "gmax" in keys:
        _elem(got["gmax"], want["gmax"], mag["gmax"], "G", what + " gmax")
    if "d_rfa" in keys:
        _sum(got["d_rfa"], want["d_rfa"], chains[0], mag["d_rfa"], "G", what + " d_rfa")
    if "d_ca" in keys:
        _sum(got["d_ca"], want["d_ca"], chains[1], mag["d_ca"], "G", what + " d_ca")
    return out


RELU_KEYS = ("ug", "dcd", "ag", "bg", "ca", "rfa", "d_mm")


def judge_relu(got, x, chain, what, keys=("dv", "s1", "s2")):
    """got: dict(dv [m, KK, C] as stored, s1, s2 [KK, C])"""
    a = _stage_args(x, RELU_KEYS)
    bf = x["ug"].dtype == BF16
    want, mag = relu(*a), relu_mag(*a)
    out = _say(what, dv=elem_ratio(got["dv"], want["dv"], mag["dv"], bf) if "dv" in keys else 0.0,
               sums_err_over_bound=max([sum_ratio(got[q], want[q], chain, *mag[q], K["dv"]) for q in ("s1", "s2") if q in keys] + [0.0]))
    if "dv" in keys:
        _elem(got["dv"], want["dv"], mag["dv"], "dv", what + " dv", bf16=bf)
    for q in ("s1", "s2"):
        if q in keys:
            _sum(got[q], want[q], chain, mag[q], "dv", f"{what} {q}")
    return out


def judge_getw(got, x, f64, what, prefill=0.0, keys=("d_mm", "dw18")):
    """got: dict(d_mm [n, Hk, Wk, 2], dw18 [18] = prefill + the gradient)"""
    a = [d(x[q]) for q in ("d_rfa", "rfa", "mm", "w18")]
    n, hk, wk = a[0].shape
    want, mag = getw_bwd(*a), getw_bwd_mag(*a)
    ch = rfa_chain(n, hk, wk, f64)
    out = _say(what, dmm=elem_ratio(got["d_mm"], want["d_mm"], mag["d_mm"]) if "d_mm" in keys else 0.0,
               dw18_err_over_bound=sum_ratio(got["dw18"], want["dw18"] + prefill, ch, mag["dw18"] + abs(prefill), mag["dw18"], K["dmm"]) if "dw18" in keys else 0.0)
    if "d_mm" in keys:
        _elem(got["d_mm"], want["d_mm"], mag["d_mm"], "dmm", what + " d_mm", chain=10)
    if "dw18" in keys:
        _sum(got["dw18"], want["dw18"] + prefill, ch, (mag["dw18"] + abs(prefill), mag["dw18"]), "dmm", what + " dw18")
    return out


def judge_gen(got, x, chain, what, keys=("dug", "dwg")):
    """got: dict(dug [m, KK, C] as stored, dwg [C, KK, KK] = the rows of partial sums folded in float64)"""
    xt = taps(d(x["x"]), x["k"], x["s"])
    a = [xt] + [d(x[q]) for q in ("ug", "dv", "alpha", "kappa", "lam")]
    bf = x["ug"].dtype == BF16
    want, mag = gen(*a), gen_mag(*a)
    out = _say(what, dug=elem_ratio(got["dug"], want["dug"], mag["dug"], bf) if "dug" in keys else 0.0,
               dwg_err_over_bound=sum_ratio(got["dwg"], want["dwg"], chain, *mag["dwg"], K["dug"]) if "dwg" in keys else 0.0)
    if "dug" in keys:
        _elem(got["dug"], want["dug"], mag["dug"], "dug", what + " dug", bf16=bf)
    if "dwg" in keys:
        _sum(got["dwg"], want["dwg"], chain, mag["dwg"], "dug", what + " dwg")
    return out


def judge_dx(got, x, what, addend=True):
    """got [n, H, W, C] as stored; x: dict(dug, wg, addnc, add_scale, n, h, w, k, s)"""
    a = (d(x["dug"]), d(x["wg"]), x["n"], x["h"], x["w"], x["k"], x["s"], d(x["addnc"]) if addend else None, x["add_scale"])
    bf = x["dug"].dtype == BF16
    want, mag = dx(*a), dx_mag(*a)
    out = _say(what, dx=elem_ratio(got, want, mag, bf))
    _elem(got, want, mag, "dx", what, bf16=bf, chain=dx_chain(x["k"], x["s"]))
    return out


SE_KEYS = ("part", "ca", "d_ca", "wa", "wb")


def judge_se(got, x, what, prefill=0.0, keys=("dgap", "dWa", "dWb")):
    """got: dict(dgap [n, C], dWa [R, C], dWb [C, R] = prefill + the gradients)"""
    a = [d(x[q]) for q in SE_KEYS] + [x["hw"]]
    n, slices, c = x["part"].shape
    ch = se_chains(n, c, x["wa"].shape[0], slices)
    want, mag = se_bwd(*a), se_bwd_mag(*a, chains=ch)
    L = dict(dgap=ch["dgap"], dWa=ch["dw"], dWb=ch["dw"])
    pf = dict(dgap=0.0, dWa=prefill, dWb=prefill)
    out = _say(what, **{q + "_err_over_bound": sum_ratio(got[q], want[q] + pf[q], L[q], mag[q][0] + abs(pf[q]), mag[q][1], K["se"]) for q in keys})
    for q in keys:
        _sum(got[q], want[q] + pf[q], L[q], (mag[q][0] + abs(pf[q]), mag[q][1]), "se", f"{what} {q}")
    return out


RF1_KEYS = ("x", "dcd", "gw", "ag", "bg", "ca", "rfa")


def judge_rf1_a(got, x, what, keys=("cd", "d_rfa", "gmax", "d_ca")):
    a = [d(x[q]) for q in RF1_KEYS] + [x["n"], x["hw"]]
    bf = x["x"].dtype == BF16
    want, mag = rf1_a(*a), rf1_a_mag(*a)
    ch = attn_chains("rf1", x["n"], x["hw"], 1, x["x"].shape[-1], 1, x["x"].dtype)
    out = _say(what, rf1=max(elem_ratio(got["cd"], want["cd"], mag["cd"], bf) if "cd" in keys else 0.0,
                            elem_ratio(got["gmax"], want["gmax"], mag["gmax"]) if "gmax" in keys else 0.0),
               sums_err_over_bound=max([sum_ratio(got[q], want[q], ch[i], *mag[q], K["rf1"]) for i, q in ((0, "d_rfa"), (1, "d_ca")) if q in keys] + [0.0]))
    if "cd" in keys:
        _elem(got["cd"], want["cd"], mag["cd"], "rf1", what + " cd", bf16=bf)
    if "gmax" in keys:
        _elem(got["gmax"], want["gmax"], mag["gmax"], "rf1", what + " gmax")
    if "d_rfa" in keys:
        _sum(got["d_rfa"], want["d_rfa"], ch[0], mag["d_rfa"], "rf1", what + " d_rfa")
    if "d_ca" in keys:
        _sum(got["d_ca"], want["d_ca"], ch[1], mag["d_ca"], "rf1", what + " d_ca")
    return out


def judge_rf1_b(got, x, what):
    """got: dict(s1, s2 [C]) (the striped sums folded)"""
    a = [d(x[q]) for q in RF1_KEYS + ("d_mm",)] + [x["n"], x["hw"]]
    want, mag = rf1_b(*a), rf1_b_mag(*a)
    ch = attn_chains("rf1", x["n"], x["hw"], 1, x["x"].shape[-1], 1, x["x"].dtype)[2]
    out = _say(what, sums_err_over_bound=max(sum_ratio(got[q], want[q], ch, *mag[q], K["rf1"]) for q in ("s1", "s2")))
    for q in ("s1", "s2"):
        _sum(got[q], want[q], ch, mag[q], "rf1", f"{what} {q}")
    return out


def judge_rf1_c(got, x, what, f64, prefill=0.0, dgap=True, keys=("dx", "dgw")):
    """got: dict(dx [n HW, C] as stored, dgw [C] = prefill + the gradient)"""
    a = [d(x[q]) for q in RF1_KEYS + ("d_mm", "alpha", "kappa", "lam")] + [d(x["dgap"]) if dgap else None, x["scale"], x["n"], x["hw"]]
    bf = x["x"].dtype == BF16
    want, mag = rf1_c(*a), rf1_c_mag(*a)
    g = rf1_geom(x["n"], x["hw"], x["x"].shape[-1], x["x"].dtype)
    ch = _cdiv(g["chunk"], g["pb"]) + g["pb"] + (0 if f64 else g["grid"][0] * g["grid"][1]) + 1
    out = _say(what, rf1=elem_ratio(got["dx"], want["dx"], mag["dx"], bf) if "dx" in keys else 0.0,
               dgw_err_over_bound=sum_ratio(got["dgw"], want["dgw"] + prefill, ch, mag["dgw"][0] + abs(prefill), mag["dgw"][1], K["rf1"]) if "dgw" in keys else 0.0)
    if "dx" in keys:
        _elem(got["dx"], want["dx"], mag["dx"], "rf1", what + " dx", bf16=bf)
    if "dgw" in keys:
        _sum(got["dgw"], want["dgw"] + prefill, ch, (mag["dgw"][0] + abs(prefill), mag["dgw"][1]), "rf1", what + " dgw")
    return out


# ---------------------------------------------------------------- premises ----------------------------------------------------------------
def max_margin_short(u, a, b):
    """[m, KK] positions whose positive maximum leads the runner-up by less than 2 KINK (|a u| + |b|) of the leader (C = 1: none)"""
    g, mg = gact(u, a, b)
    if u.shape[-1] < 2:
        return torch.zeros(u.shape[:-1], dtype=torch.bool)
    top = torch.topk(g, 2, dim=-1)
    lead_m = torch.gather(mg, -1, top.indices[..., :1]).squeeze(-1)
    return (top.values[..., 0] > 0) & (top.values[..., 0] - top.values[..., 1] < 2 * KINK * lead_m)


def assert_premises(u, a, b, what):
    """NO element in the ReLU band, NO map position with an undecided maximum; u, a, b float64 (a [KK, C] or [C] broadcast over u)"""
    nb = int(in_band(u, a.expand_as(u), b.expand_as(u)).sum())
    nm = int(max_margin_short(u, a, b).sum())
    assert nb == 0 and nm == 0, f"{what}: {nb} elements inside the ReLU kink band, {nm} positions with an undecided maximum"


def raise_leader(u, a, b, dtype):
    """lifts the leader's u (towards a larger G) at the positions max_margin_short flags; -> (u as stored, positions moved)"""
    moved = 0
    for _ in range(8):
        ud = d(u)
        short = max_margin_short(ud, a, b)
        k = int(short.sum())
        if k == 0:
            return u, moved
        moved += k
        g, _ = gact(ud, a, b)
        lead = F.one_hot(g.argmax(-1), ud.shape[-1]).bool() & short.unsqueeze(-1)
        step = (2.0 ** -5 if dtype == BF16 else 2.0 ** -12) * (ud.abs() + (b / a).abs().expand_as(ud))
        u = torch.where(lead, ud + torch.sign(a).expand_as(ud) * step, ud).to(dtype)
    raise AssertionError("the maximum's margin could not be made")


def se_margin_short(part, wa, hw):
    gap = part.sum(1) / hw
    return (gap @ wa.t()).abs() < SE_MARGIN * (gap.abs() @ wa.abs().t())


# ---------------------------------------------------------------- input builders ----------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(_seed("rfcbam", *key))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64)


def allneg_positions(mo, kk):
    """the planted all-negative map positions (m, t): the first and the last pixel at tap 0, the second pixel at the last tap"""
    return sorted({(0, 0), (mo - 1, 0), (min(1, mo - 1), kk - 1)})


def stage_inputs(key, n, ho, wo, c, k, dtype, gw=False):
    """the operands of the attention / ReLU / generate-gradient stages as stored: ug, dcd [m, KK, C] in `dtype`; ag, bg, alpha, kappa, lam
    [KK, C], ca [n, C], the maps rfa, d_mm fp32; gmax = the fp32 G of the leader (what pass 0 stores), dv = relu()'s dv as stored.
    gw: the k = 1 form — `ug` is x and G = relu(ag (gw x) + bg); the premises are taken with ag gw.  Planted: all-negative positions
    (allneg_positions), channel C - 1 negative everywhere, for C >= 128 channels 64..127 with a < 0, b = -0.0, u = +0 at tap KK / 2"""
    g = _gen(key, n, ho, wo, c, k, str(dtype), gw)
    kk, mo = k * k, n * ho * wo
    u = _randn(g, mo, kk, c) * (_rand(g, c) * 2 + 0.3)
    ag = (_rand(g, kk, c) + 0.5) * torch.where(_rand(g, kk, c) < 0.25, -1.0, 1.0)
    bg = _randn(g, kk, c) * 0.5
    ag[:, c - 1], bg[:, c - 1] = 0.01, -50.0                         # an all-negative channel
    gwv = ((_rand(g, c) + 0.5) * torch.where(_rand(g, c) < 0.3, -1.0, 1.0)).float() if gw else None
    ag, bg = ag.float(), bg.float()
    aeff = ag.double() * (gwv.double() if gw else 1.0)
    dead = (aeff * u + bg.double()).amax(-1) <= 0                    # narrow cases: a position that is all-negative by chance gets channel 0 lit
    lit = ((1 + _rand(g, mo, kk)) * bg[:, 0].double().abs().clamp(min=1.0) - bg[:, 0].double()) / aeff[:, 0]
    u[..., 0] = torch.where(dead, lit, u[..., 0])
    for m, t in allneg_positions(mo, kk):
        vt = -(1 + _rand(g, c)) * bg[t].double().abs().clamp(min=1.0)
        u[m, t] = (vt - bg[t].double()) / aeff[t]
    zt = kk // 2
    if c >= 128 and not gw:
        ag[zt, 64:128] = -ag[zt, 64:128].abs()
        bg[zt, 64:128] = -0.0
        u[:, zt, 64:128] = 0.0
        aeff = ag.double()
    u = u.to(dtype)
    moved = 0
    for _ in range(6):
        u, k1 = nudge(u, aeff.expand(mo, kk, c), bg.expand(mo, kk, c), dtype)
        u, k2 = raise_leader(u, aeff, bg.double(), dtype)
        moved += k1 + k2
        if k1 + k2 == 0:
            break
    dcd = (_randn(g, mo, kk, c) * (_rand(g, c) + 0.2)).to(dtype)
    ca = torch.sigmoid(_randn(g, n, c) * 2).float()
    rfa = torch.sigmoid(_randn(g, n, k * ho, k * wo) * 2).float()
    d_mm = (_randn(g, n, k * ho, k * wo, 2) * 3).float()
    ueff = d(u) * (gwv.double() if gw else 1.0)
    if gw:
        ueff = ueff.float().double()                                # the kernel's u = fl(gw x)
    gmax = to_map(torch.clamp(ag.double() * ueff + bg.double(), min=0.0).amax(-1), n, ho, wo, k).float()
    alpha = ag.clone()
    kappa, lam = (_randn(g, kk, c) * 0.1).float(), (_randn(g, kk, c) * 0.1).float()
    x = dict(ug=u, dcd=dcd, ag=ag, bg=bg, ca=ca, rfa=rfa, d_mm=d_mm, gmax=gmax, alpha=alpha, kappa=kappa, lam=lam, n=n, ho=ho, wo=wo, k=k,
             moved=moved, aeff=aeff, gw=gwv)
    if not gw:
        x["dv"] = relu(*_stage_args(x, RELU_KEYS))["dv"].to(dtype)
    return x


def tc_inputs(cid, dtype):
    """a thread = channel case: stage_inputs + x [n, H, W, C] and the generate weight for ly_rf_generate / ly_rf_bwd_gen, dug (gen()'s result as
    stored), addnc [n, C] and add_scale for ly_rf_bwd_dx"""
    n, h, w, c, k, s = TC_CASES[cid]
    ho, wo = out_hw(h, w, k, s)
    x = stage_inputs(cid, n, ho, wo, c, k, dtype)
    g = _gen("tc", cid, str(dtype))
    x["x"] = (_randn(g, n, h, w, c) * (_rand(g, c) * 2 + 0.3)).to(dtype)
    x["wg"] = (_randn(g, c * k * k, k * k) * 0.4).float()
    x["addnc"] = (_randn(g, n, c) * 50).float()
    x.update(h=h, w=w, s=s, add_scale=float(torch.tensor(1.0 / (h * w), dtype=torch.float32)))
    xt = taps(d(x["x"]), k, s)
    x["dug"] = gen(xt, *[d(x[q]) for q in ("ug", "dv", "alpha", "kappa", "lam")])["dug"].to(dtype)
    return x


def rf1_inputs(n, hw, c, dtype):
    """a k = 1 case of ly_rf1_bwd: x, dcd [n HW, C], gw, ag, bg, alpha, kappa, lam [C], ca, dgap [n, C], rfa, gmax [n HW], d_mm [n HW, 2]"""
    s = stage_inputs("rf1", n, hw, 1, c, 1, dtype, gw=True)
    g = _gen("rf1x", n, hw, c, str(dtype))
    return dict(x=s["ug"][:, 0].contiguous(), dcd=s["dcd"][:, 0].contiguous(), gw=s["gw"], ag=s["ag"][0].contiguous(), bg=s["bg"][0].contiguous(), ca=s["ca"],
                rfa=s["rfa"].reshape(-1), d_mm=s["d_mm"].reshape(-1, 2), gmax=s["gmax"].reshape(-1), alpha=s["alpha"][0].contiguous(), kappa=s["kappa"][0].contiguous(),
                lam=s["lam"][0].contiguous(), dgap=(_randn(g, n, c) * 50).float(), scale=float(torch.tensor(1.0 / hw, dtype=torch.float32)), n=n, hw=hw,
                aeff=s["aeff"][0], moved=s["moved"])


def rfa_inputs(cid):
    n, hk, wk = RFA_CASES[cid]
    g = _gen("rfa", cid)
    z = _randn(g, n, hk, wk) * 2
    z[:, 0, 0], z[:, hk - 1, wk - 1] = 20.0, -20.0                   # saturated sigmoids at two corners
    mm = torch.stack((_rand(g, n, hk, wk) * 3, _rand(g, n, hk, wk)), -1)
    return dict(d_rfa=(_randn(g, n, hk, wk) * 2).float(), rfa=torch.sigmoid(z).float(), mm=mm.float(), w18=(_randn(g, 18) * 0.5).float())


def se_inputs(cid):
    """part [n, slices, C] (positive: sums of a ReLU's output), wa [R, C] with every fourth unit clearly off (all weights negative) and unit 0 clearly on, wb [C, R],
    ca in (0, 1) with saturated channels, d_ca fp32; hidden units inside the margin are moved out"""
    n, c, r, slices = SE_CASES[cid]
    g = _gen("se", cid)
    hw = 64 * slices + 3
    part = ((_rand(g, n, slices, c) + 0.1) * hw / slices).float()
    wa = _randn(g, r, c) / math.sqrt(c)
    off = torch.arange(r) % 4 == 3
    wa[off] = -wa[off].abs()
    wa[0] = wa[0].abs()                                              # unit 0 clearly on (R = 1: the only unit)
    wa = wa.float()
    for _ in range(8):
        short = se_margin_short(part.double(), wa.double(), hw).any(0)
        if not bool(short.any()):
            break
        wa[short, 0] += 0.05
    z = _randn(g, n, c) * 2
    z[:, 3 % c], z[:, 5 % c] = 20.0, -20.0
    return dict(part=part, ca=torch.sigmoid(z).float(), d_ca=(_randn(g, n, c) * 5).float(), wa=wa, wb=_randn(g, c, r).float(), hw=hw, off=off)


# ---------------------------------------------------------------- case tables -------------------------------------------------------------
# branch of the kernels -> case id: the table in the docstring of tests/test_gpu_rfcbam_bwd.py
# thread = channel kernels: id -> (n, H, W, C, k, s)
TC_CASES = {"subs4-odd-parity-straddle-c64": (2, 9, 7, 64, 3, 2), "cb128-clamped-s2t-partial-c72": (1, 8, 12, 72, 3, 2),
            "subs1-idlewave-s1-c192": (2, 5, 6, 192, 3, 1), "gy2-clamped-s2t-c320": (3, 6, 6, 320, 3, 2), "k1-c6": (2, 7, 5, 6, 1, 1),
            "chunk-over-image-add1-c8": (5, 3, 3, 8, 3, 2)}
# what each id claims: chunk and grid x over the output pixels, subs, cb, gy, clamped lanes of the last channel group, live threads, dx form
TC_CLAIMS = {"subs4-odd-parity-straddle-c64": dict(chunk=32, gx=2, subs=4, cb=64, gy=1, clamped=0, threads=256, form=2, gather="parity"),
             "cb128-clamped-s2t-partial-c72": dict(chunk=16, gx=2, subs=2, cb=128, gy=1, clamped=56, threads=256, form="s2t", tiles_x=2, cgroups=2),
             "subs1-idlewave-s1-c192": dict(chunk=8, gx=8, subs=1, cb=192, gy=1, clamped=0, threads=192, form=2, gather="generic"),
             "gy2-clamped-s2t-c320": dict(chunk=8, gx=4, subs=1, cb=256, gy=2, clamped=192, threads=256, form="s2t", tiles_x=1, cgroups=5),
             "k1-c6": dict(chunk=32, gx=3, subs=4, cb=64, gy=1, clamped=58, threads=256, form=2, gather="generic"),
             "chunk-over-image-add1-c8": dict(chunk=32, gx=1, subs=4, cb=64, gy=1, clamped=56, threads=256, form=1, gather="parity")}
# ly_rf3s_bwd: id -> (C fp32, C bf16, Ho, Wo, n)
RF3S_C = ((4, 8), (24, 24), (64, 64), (160, 160), (256, 512))
RF3S_SHAPES = {4: ((1, 1, 1), (3, 5, 3), (9, 11, 1)), 24: ((3, 5, 1), (9, 11, 3)), 64: ((1, 1, 3), (9, 11, 1)), 160: ((3, 5, 3), (9, 11, 1)),
               256: ((3, 5, 1), (9, 11, 3))}
RF3S_CASES = {f"c{cf}-{cb}-{ho}x{wo}-n{n}": (cf, cb, ho, wo, n) for cf, cb in RF3S_C for ho, wo, n in RF3S_SHAPES[cf]}
# (lpp2, pp, threads) per (fp32, bf16) of each C pair
RF3S_CLAIMS = {4: ((1, 4, 36), (1, 4, 36)), 24: ((8, 4, 288), (4, 4, 144)), 64: ((16, 4, 576), (8, 4, 288)), 160: ((64, 1, 576), (32, 2, 576)),
               256: ((64, 1, 576), (64, 1, 576))}
# ly_rf1_bwd: id -> (C fp32, C bf16, HW, n)
RF1_SHAPES = {4: ((1, 1), (37, 3), (1031, 1)), 24: ((37, 1), (400, 3)), 64: ((400, 1), (1031, 3)), 160: ((37, 3), (400, 1)), 256: ((1, 3), (37, 1), (1031, 1))}
RF1_CASES = {f"c{cf}-{cb}-hw{hw}-n{n}": (cf, cb, hw, n) for cf, cb in RF3S_C for hw, n in RF1_SHAPES[cf]}
# ly_rfa_bwd: id -> (n, Hk, Wk)
RFA_CASES = {"one-position": (1, 1, 1), "inside-one-tile-15x63": (2, 15, 63), "exact-tile-16x64": (1, 16, 64), "halo-four-tiles-17x65": (2, 17, 65),
             "wide-3x200": (1, 3, 200), "block-cap-513-tiles": (19, 48, 576)}
# ly_se_bwd: id -> (n, C, R, slices)
SE_CASES = {"n1-c8-r1": (1, 8, 1, 1), "n3-c160-r10-nq40": (3, 160, 10, 6), "n8-c64-r4-one-trip": (8, 64, 4, 2), "n9-c256-r16-trip-plus-one": (9, 256, 16, 7),
            "n17-c1024-r64-two-trips-plus-one": (17, 1024, 64, 128)}


def c_of(pair, dtype):
    return pair[1] if dtype == BF16 else pair[0]


# ---------------------------------------------------------------- measurements (reference only) -------------------------------------------
def _r(got, want, mag):
    m = mag > 0
    return float(((d(got) - want).abs() / (U24 * mag).clamp(min=1e-300))[m].max()) if bool(m.any()) else 0.0


def measure_k():
    """worst ratio, in units of u24 M, of torch's float32 evaluation of the references against float64 over every case of the tables (one
    thread: torch's float32 reductions split their work by thread count)"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _measure_k()
    finally:
        torch.set_num_threads(threads)


def _measure_k():
    worst = {key: 0.0 for key in K}
    up = lambda key, v: worst.__setitem__(key, max(worst[key], v))
    f32 = lambda a: [t.float() if torch.is_tensor(t) else t for t in a]
    stage_cases = [(cid, out_hw(v[1], v[2], v[4], v[5]), v[0], v[3], v[4]) for cid, v in TC_CASES.items()]
    stage_cases += [(cid, (v[2], v[3]), v[4], None, 3) for cid, v in RF3S_CASES.items()]
    for dt in (F32, BF16):
        for cid, (ho, wo), n, c, k in stage_cases:
            x = tc_inputs(cid, dt) if cid in TC_CASES else stage_inputs("rf3s", n, ho, wo, c_of(RF3S_CASES[cid], dt), 3, dt)
            a = _stage_args(x, ATTN_KEYS)
            got, want, mag = attn(*f32(a)), attn(*a), attn_mag(*a)
            up("G", max(_r(got["cd"], want["cd"], mag["cd"]), _r(got["gmax"], want["gmax"], mag["gmax"])))
            a = _stage_args(x, RELU_KEYS)
            up("dv", _r(relu(*f32(a))["dv"], relu(*a)["dv"], relu_mag(*a)["dv"]))
            if cid in TC_CASES:
                a = (d(x["x"]), d(x["wg"]), x["k"], x["s"])
                up("gen", _r(generate(*f32(a)), generate(*a), generate_mag(*a)))
                a = [taps(d(x["x"]), x["k"], x["s"])] + [d(x[q]) for q in ("ug", "dv", "alpha", "kappa", "lam")]
                up("dug", _r(gen(*f32(a))["dug"], gen(*a)["dug"], gen_mag(*a)["dug"]))
                a = (d(x["dug"]), d(x["wg"]), x["n"], x["h"], x["w"], x["k"], x["s"], d(x["addnc"]), x["add_scale"])
                up("dx", _r(dx(*f32(a)), dx(*a), dx_mag(*a)))
        for cid, (cf, cb, hw, n) in RF1_CASES.items():
            x = rf1_inputs(n, hw, c_of((cf, cb), dt), dt)
            a = [d(x[q]) for q in RF1_KEYS] + [n, hw]
            got, want, mag = rf1_a(*f32(a)), rf1_a(*a), rf1_a_mag(*a)
            up("rf1", max(_r(got["cd"], want["cd"], mag["cd"]), _r(got["gmax"], want["gmax"], mag["gmax"])))
            a = [d(x[q]) for q in RF1_KEYS + ("d_mm", "alpha", "kappa", "lam", "dgap")] + [x["scale"], n, hw]
            up("rf1", _r(rf1_c(*f32(a))["dx"], rf1_c(*a)["dx"], rf1_c_mag(*a)["dx"]))
    for cid in RFA_CASES:
        x = rfa_inputs(cid)
        a = [d(x[q]) for q in ("d_rfa", "rfa", "mm", "w18")]
        up("dmm", _r(getw_bwd(*f32(a))["d_mm"], getw_bwd(*a)["d_mm"], getw_bwd_mag(*a)["d_mm"]))
    for cid in SE_CASES:
        x = se_inputs(cid)
        a = [d(x[q]) for q in SE_KEYS] + [x["hw"]]
        got, want, mag = se_bwd(*f32(a)), se_bwd(*a), se_bwd_mag(*a)
        up("se", max(_r(got[q], want[q], mag[q][1]) for q in ("dgap", "dWa", "dWb")))
    return worst
