"""Float64 references, judges, input builders and case tables for the RFCBAMConv FORWARD kernels

    k = 3, lane = channel       ly_rf3c_stats -> ly_rfcbam_mid -> ly_rf3c_fwd                        (csrc/ly_rf3c.hip, ly_rf3c.hpp)
    k = 3, matrix cores (bf16)  ly_rf3m_stats -> ly_rfcbam_mid -> ly_rf3m_fwd                        (csrc/ly_rf3m.hip)
    k = 3, lane = pixel         ly_colsum, ly_rfcbam_stats (k = 3) -> ly_rfcbam_mid -> ly_rfcbam3_fwd   (csrc/ly_rfcbam_att.hip, ly_rfcbam3.hip)
    k = 1                       ly_rfcbam_stats (k = 1) -> ly_rfcbam_mid -> ly_gemm_fwd with PRO_AFFINE_RELU_CA and rowscale
    the small steps             ly_colsum, ly_se_fwd, ly_rfcbam_mid, ly_rfa_map

A plain helper module: tests/test_rfcbam_fwd_host.py (CPU) and tests/test_gpu_rfcbam_fwd.py (device) import the SAME references, judges,
builders and case tables from here.  Nothing here calls a kernel or lead_yolo_amd.ops.  The judges' forms, `_fail` and `_seed` are those of
tests/bnact_ref.py; `taps`, `to_map`, `from_map`, `getw_fwd` and the SE / map shape tables are those of tests/rfcbam_ref.py.

Layouts (the kernels' own): x [n, H, W, C]; G, B [m][t][c] with m = (n, ho, wo) the output pixel and t = ty k + tx the tap; maps
[n][k Ho][k Wo] (mm with a trailing 2 = (max, mean)), position of (m, t) = (ho k + ty, wo k + tx); the generate parameters w [C][KK (t)][KK (u)],
a, b [C][KK] (BatchNorm scale / shift) and the folded wf = fl32(w a); the conv weight wc [O][C][KK]; part [n][slice][C]; ca [n][C].

References (float64, from the stored values widened exactly)
    v = b + sum_u wf x_u (folded)   |   v = a (sum_u w x_u) + b (raw)          G = relu(v)         x zero padded (pad 1, stride s)
    mm = (max_c G, mean_c G)    part = sums of x per slice    ca = sigmoid(Wb relu(Wa mean_hw x))    rfa = sigmoid(conv3x3_pad1(mm; w18))
    u = e_scale (sum_{t, c} wc G ca rfa) + e_shift      out = relu(u), or u when `linear` / a statistics pass      s1 = sum u, s2 = sum u^2
Keyword switches plant ONE named defect each (tests/test_rfcbam_fwd_host.py shows that the judges reject them; no broken kernel is built).

Two input families per case (the same beacon placements in both):
  lattice   every operand on a dyadic grid (x, wc multiples of 1/4, w of 1/2, b and e_shift of 1/8, a in {1/2, 1} with either sign, ca, rfa,
            e_scale powers of two; |v| < 16 in units of 1/16: G ca rfa has at most 8 significant bits, every product and partial sum is exact
            in fp32, the lo plane of the fp32 split is zero).  The float64 reference IS the kernel's result: judged with torch.equal on the
            fp32 value (rounded once to bf16 for bf16 storage).  Two exceptions, both by arithmetic and not by choice: the mean at C = 96
            (sum * fl(1/96): the exact sum is judged at one unit in the last place, 2^-23 |want|), and s2, the sum of SQUARES of a value of up
            to 22 significant bits, which no fp32 product holds exactly (s2 is judged with the bound in both families; s1 is exact).
  rounded   seeded random values, judged with conditioned bounds (below).
Beacons: (image, oy, ox, tap) placements — the two padded corners, the last pixel of the first tile, the last pixel of the map (the last
column of a ragged tile), the first pixel of the second image — each with its own channel, the first in channel chunk 0 and the others
counted down from C - 1 (the last chunk): the centre input of the pixel is large in that channel (on the rounded family its only input), the generate weight of (channel, tap,
centre) — the channel's only generate weight — and the conv weights wc[:, channel, tap] are large, the latter with a large lo plane.  A beacon product is > 1/2 of its sum and
> 100 bounds (asserted by the host test).  Tap DEAD = 5 is negative in every channel (b = -40; -12 on the lattice) except where a beacon
lights it: its maximum is 0, the identity the kernels start from.

Bounds (u24 = 2^-24), the forms of tests/bnact_ref.py
  elementwise   |got - want| <= u24 (K M + L T) [+ operand allowance] [+ 2^-8 |want| for a value stored as bf16]
  sums          |got - want| <= u24 L sum |term| + sum E_term          (E_term: the elementwise bound of the term; doubles add no chain)
  M: the sum of the magnitudes of the terms, every intermediate carried with ITS terms and NOT masked by the ReLU (relu, max and sigmoid are
     continuous: no band, no mask, nothing left out): M_v = |b| + sum |wf x| resp. |a| sum |w x| + |b|; M_max = max_c M_v; M_mean = mean_c M_v;
     M_B = M_v ca rfa; M_u = |e_scale| sum |wc| M_B + |e_shift|; sigmoid outputs: sigma'(z) e^E E with E the bound of z, + K u24 sigma + 2^-126 (fp32 holds no smaller sigmoid).
  L: the longest fp32 addition chain, from the code (the geometry functions below):
     v          KK + 1 (one accumulator over the taps; raw: + the affine step) — inside K, it is what measure_k's float32 evaluation does too
     mean       C + 8   (ly_rf3c_stats: one accumulator per (pixel, tap) over every channel of every chunk, the ninth tap 4 per group and
                chunk + 8 groups; ly_rfcbam_stats3: 8 per wave and chunk, pairwise, + 4 waves; ly_rf3m_stats: 4 per unit + the half-wave
                exchange; k = 1: ceil(C / 4 / lanes) x 4 per lane + log2(lanes)) — C + 8 covers each
     part       k = 3, rf3c: 3 (own, stride 2) + 4 (pixel pairs of a lane) + 1 + 1 + 3 = 12; stats3: ceil(s TH s TW / 8) + 8; rf3m: 12 (MFMA
                k-steps) + 5 (tree); k = 1 / colsum: ceil(per / groups) + groups (part_chain)
     u          KK C + 2 (the MFMA accumulator over every k-step + the epilogue's multiply-add; k = 1: C + 3 with the row scale)
     s1 / s2    4 (pixel slots of a lane) + 4 (16-lane tree) = 8, then double atomics
     ca         gap: ceil(slices / ng) + ng + 1; hidden: ceil(C / 64) + 6; out: R          rfa   18 (two products per step, nine steps) + 1
  operand allowance of the MFMA contractions, on top: fp32 storage 2^-14 sum |wc B| |e_scale| (the three-term bf16 split,
     tests/test_gpu_bf16.py::test_bf16x3_adversarial_bounds), bf16 storage 2^-9 sum |wc B| |e_scale| (half an ulp of the bf16 rounding of a B at
     the top of its binade; at the bottom it is 2^-8 |B|, so the allowance holds for a sum of many operands and NOT for one that dominates its
     sum: a beacon's B is therefore built as a bf16 value, 192 = 1.5 * 2 * 64 with ca = rfa = 1, in a channel that is dark elsewhere, and carries
     no operand rounding at all, and the rounded family keeps the other operands comparable — channel scales of x in [0.75, 1.25], ca and rfa
     in [0.5, 1], |wc| within a factor 2 — so that no handful of products carries a sum of K = 32 .. 864.  The exact arithmetic (B rounded to
     bf16, an exact sum, one bf16 rounding) then stays under 0.83 of the bound on every case, evaluated on the CPU);
     wc enters as stored: one bf16 plane, widened, for bf16 storage.  ly_rf3m: the folded generate weights are the bf16-rounded ones of
     pack.rf3m_stream (torch's own conversion), the shift its hi + lo + lolo split; x is stored bf16: only the accumulation chain enters.
  K, per reference: the SAME references in torch float32 on the CPU against float64 over every rounded case of the tables, the k = 1 statistics rows included (measure_k),
     worst err / (u24 M) times 4 (v_rcp / v_exp at one ulp each, fused against separate multiply-add), rounded up;
     tests/test_rfcbam_fwd_host.py re-measures and holds 4 x worst <= K.  No device figure enters a bound.
        worst ratio   v 4.15   mean 2.31   ca 1.74   rfa 4.64   u 12.9 (torch's float32 einsum over up to 864 products: its own chain is in it)
        K             v 17     mean 10     ca 7      rfa 19     u 52
"""
import math

import torch

from tests.bnact_ref import BF16, BF16_EPS, F32, U24, _fail, _seed, d, fold  # noqa: F401
from tests.rfcbam_ref import RFA_CASES, SE_CASES, _cdiv, _shift, from_map, getw_fwd, out_hw, taps, to_map, vw_of  # noqa: F401

K = dict(v=17.0, mean=10.0, ca=7.0, rfa=19.0, u=52.0)
DEAD = 5
ULP_MEAN = 2.0 ** -23 + 2.0 ** -46                # fl(sum * fl(1 / C)) for an exact sum: (1 + 2^-24)^2 - 1, two roundings to nearest
THREADS = 256
FAMILIES = ("lattice", "rounded")
TINY = 2.0 ** -126                                # fp32 holds no sigmoid below it (the kernels' v_exp / v_rcp flush there)
WBIG = 1.0 + 2.0 ** -8 - 2.0 ** -12               # rounds to 1.0 in bf16: a lo plane of 2^-8 of the value


# ---------------------------------------------------------------- references -------------------------------------------------------------
def gen_v(x, p, k, s, raw, clamp=False, swap_tap=False, folded_in_raw=False):
    """v [m, KK, C]: the BatchNorm output of `generate` before the ReLU.  p: dict(w [C, KK, KK], a, b [C, KK], wf).  DEFECTS: clamp (the border
    clamped instead of zero padded), swap_tap (taps (0, 1) and (1, 0) exchanged: ty <-> tx), folded_in_raw (the raw form fed the folded weights)"""
    xt = taps(x, k, s, clamp)
    if raw:
        v = p["a"].t() * torch.einsum("ctu,muc->mtc", p["wf"] if folded_in_raw else p["w"], xt) + p["b"].t()
    else:
        v = torch.einsum("ctu,muc->mtc", p["wf"], xt) + p["b"].t()
    if swap_tap and k == 3:
        v = v.clone()
        v[:, [1, 3]] = v[:, [3, 1]]
    return v


def gen_v_mag(x, p, k, s, raw):
    xt = taps(x.abs(), k, s)
    if raw:
        return p["a"].abs().t() * torch.einsum("ctu,muc->mtc", p["w"].abs(), xt) + p["b"].abs().t()
    return torch.einsum("ctu,muc->mtc", p["wf"].abs(), xt) + p["b"].abs().t()


def mm_of(v, n, ho, wo, k, drop_chunk=False, pre_relu_max=False):
    """[n, k Ho, k Wo, 2] = (max_c, mean_c) of relu(v).  DEFECTS: drop_chunk (the last 32 channels missing from the mean), pre_relu_max"""
    g = torch.clamp(v, min=0.0)
    c = v.shape[-1]
    mx = (v if pre_relu_max else g).amax(-1)
    mean = (g[..., :c - 32] if drop_chunk else g).sum(-1) / c
    return torch.stack((to_map(mx, n, ho, wo, k), to_map(mean, n, ho, wo, k)), -1)


def mm_mag(v, vm, n, ho, wo, k):
    """(M of the max, M of the mean, T of the mean = the mean itself)"""
    g = torch.clamp(v, min=0.0)
    mp = lambda e: to_map(e, n, ho, wo, k)
    return mp(vm.amax(-1)), mp(vm.mean(-1)), mp(g.mean(-1))


def tile_slices(h, w, s, ho, wo, th, tw):
    """k = 3: the input rectangle every output tile OWNS, in tile order: rows [s rt TH, s (rt + 1) TH) x cols [s ct TW, s (ct + 1) TW), cut at the map"""
    return [(s * rt * th, min(s * (rt + 1) * th, h), s * ct * tw, min(s * (ct + 1) * tw, w)) for rt in range(_cdiv(ho, th)) for ct in range(_cdiv(wo, tw))]


def part_tiles(x, s, ho, wo, th, tw):
    """part [n, tiles, C] of the k = 3 statistics passes"""
    n, h, w, c = x.shape
    return torch.stack([x[:, r0:r1, c0:c1].reshape(n, -1, c).sum(1) for r0, r1, c0, c1 in tile_slices(h, w, s, ho, wo, th, tw)], 1)


def part_slices(x, slices):
    """part [n, slices, C] of ly_colsum / the k = 1 pass: slice sl holds the pixels [sl per, (sl + 1) per) with per = ceil(HW / slices)"""
    n, c = x.shape[0], x.shape[-1]
    xf = x.reshape(n, -1, c)
    per = _cdiv(xf.shape[1], slices)
    return torch.stack([xf[:, sl * per:(sl + 1) * per].sum(1) for sl in range(slices)], 1)


def se_ca(part, wa, wb, hw):
    """ca [n, C] = sigmoid(Wb relu(Wa mean)) from the pooling partials; -> dict(ca, z, gap, hid)"""
    gap = part.sum(1) / hw
    hid = torch.clamp(gap @ wa.t(), min=0.0)
    z = hid @ wb.t()
    return dict(ca=torch.sigmoid(z), z=z, gap=gap, hid=hid)


def se_chains(c, r, slices):
    nq = c // 4
    ng = THREADS // nq
    return dict(gap=_cdiv(slices, ng) + ng + 1, hid=_cdiv(c, 64) + 6, out=r)


def _sig_bound(z, e, key):
    """|sigmoid(z + e') - sigmoid(z)| for |e'| <= e, + the sigmoid's own roundings"""
    sg = torch.sigmoid(z)
    return sg * (1 - sg) * torch.exp(e) * e + K[key] * U24 * sg + TINY


def se_ca_bound(part, wa, wb, hw, chains=None):
    """the elementwise bound of ca; chains None: the plain magnitudes in units of u24 (measure_k)"""
    ch = chains or dict(gap=0, hid=0, out=0)
    o = se_ca(part, wa, wb, hw)
    t_gap = part.abs().sum(1) / hw
    e_gap = (K["ca"] + ch["gap"]) * t_gap                                   # in units of u24
    e_hid = (K["ca"] + ch["hid"]) * (o["gap"].abs() @ wa.abs().t()) + e_gap @ wa.abs().t()
    e_z = (K["ca"] + ch["out"]) * (o["hid"] @ wb.abs().t()) + e_hid @ wb.abs().t()
    return e_z, _sig_bound(o["z"], U24 * e_z, "ca")


def rfa_pre(mm, w18):
    """the 3x3 conv 2 -> 1, zero padded, before the sigmoid, and the sum of the magnitudes of its terms"""
    w = w18.reshape(2, 3, 3)
    pre = sum(w[ch, dy, dx] * _shift(mm[..., ch], dy - 1, dx - 1) for ch in range(2) for dy in range(3) for dx in range(3))
    mag = sum(w[ch, dy, dx].abs() * _shift(mm[..., ch].abs(), dy - 1, dx - 1) for ch in range(2) for dy in range(3) for dx in range(3))
    return pre, mag


RFA_CHAIN = 19


def contract(g, ca, rfa, wc, es, esh, n, ho, wo, k, linear=False, ca_next=False, rfa_swapped=False, sq_after_relu=False, rowscale=False):
    """the main contraction from G [m, KK, C]: dict(u [m, O], out, s1, s2 [O], B).  wc [O, C, KK].  rowscale: the k = 1 form (rfa multiplies the
    accumulator in the epilogue, B = G ca).  DEFECTS: ca_next (ca of the neighbouring image), rfa_swapped (rfa read at (wo, ho)), sq_after_relu
    (s2 from the activated value)"""
    c = g.shape[-1]
    cae = (ca.roll(-1, 0) if ca_next else ca).repeat_interleave(ho * wo, 0).unsqueeze(1)
    re = from_map(rfa, n, ho, wo, k)
    if rfa_swapped:
        hk, wk = rfa.shape[1:]
        m = torch.arange(n * ho * wo)
        oy, ox = (m // wo) % ho, m % wo
        t = torch.arange(k * k)
        yy = (ox.view(-1, 1) * k + (t // k).view(1, -1)) % hk
        xx = (oy.view(-1, 1) * k + (t % k).view(1, -1)) % wk
        re = rfa[(m // (ho * wo)).view(-1, 1), yy, xx]
    re = re.unsqueeze(-1)
    b = g * cae * (1.0 if rowscale else re)
    acc = torch.einsum("mtc,oct->mo", b, wc)
    u = es * (acc * re[:, 0] if rowscale else acc) + esh
    act = torch.clamp(u, min=0.0)
    return dict(u=u, out=u if linear else act, s1=u.sum(0), s2=((act if sq_after_relu else u) ** 2).sum(0), B=b)


def contract_bound(g, gm, ca, rfa, wc, es, esh, n, ho, wo, k, storage, chain, rowscale=False, allowance=True):
    """E_u [m, O]: the elementwise bound of u without the storage term: u24 (K M + L T) + the operand allowance.  chain None, allowance False:
    M alone in units of u24 (measure_k)"""
    cae = ca.repeat_interleave(ho * wo, 0).unsqueeze(1)
    re = from_map(rfa, n, ho, wo, k).unsqueeze(-1)
    f = cae * (1.0 if rowscale else re)
    rs = re[:, 0] if rowscale else 1.0
    t_acc = torch.einsum("mtc,oct->mo", g * f, wc.abs()) * rs * es.abs()
    m_u = torch.einsum("mtc,oct->mo", gm * f, wc.abs()) * rs * es.abs() + esh.abs()
    if chain is None:
        return m_u
    e = U24 * (K["u"] * m_u + chain * t_acc)
    if allowance:
        e = e + (2.0 ** -9 if storage == BF16 else 2.0 ** -14) * t_acc
    return e


def u_chain(c, k, rowscale=False):
    return k * k * c + (3 if rowscale else 2)


STATS_CHAIN = 8


# ---------------------------------------------------------------- stored weights of the three routes -------------------------------------
def stored_params(p, route):
    """the generate parameters as the route's kernels hold them, float64: "rf3m": wf rounded to bf16 by torch, b as the hi + lo + lolo split of
    pack.rf3m_stream; every other route: the fp32 values"""
    q = {key: d(v) for key, v in p.items() if torch.is_tensor(v)}
    if route == "rf3m":
        q["wf"] = p["wf"].bfloat16().double()
        b = p["b"].float()
        bh = b.bfloat16().float()
        bl = (b - bh).bfloat16().float()
        q["b"] = bh.double() + bl.double() + (b - bh - bl).bfloat16().double()
    return q


def stored_wc(wc, storage):
    return (wc.bfloat16() if storage == BF16 else wc).double()


def unpack_wq_c(img, c):
    """pack.rfcbam_gen_weights_c's image -> [C, 100]: element i of channel ch at ((ch // 32 * 25 + i // 4) * 32 + ch % 32) * 4 + i % 4"""
    return img.view(c // 32, 25, 32, 4).permute(0, 2, 1, 3).reshape(c, 100)


def unpack_rf3m_gen(stream, c):
    """pack.rf3m_stream's statistics stream -> (wf [C, 9, 9], shift slots [C, 9, 3]) as float64: fragment (chunk, unit j, st) of the 8-tap tile holds
    row r = 8 (channel 4j + r // 8 slot) + tap at lane (r, h), element e <-> patch slot 4 st + 2 h + e // 4, channel slot e % 4; the tap-8 tile
    (fragments 3 .. 5 of a unit) holds channel r of the chunk in row r < 16"""
    st = stream.double().view(c // 16, 4, 6, 2, 32, 2, 4)                    # [chunk][j][frag][h][r][e // 4][e % 4]
    wx = torch.zeros(c, 9, 12, dtype=torch.float64)
    for ch in range(c):
        q, j, cs = ch // 16, (ch % 16) // 4, ch % 4
        for t in range(8):
            r = 8 * cs + t
            for u in range(12):
                wx[ch, t, u] = st[q, j, u // 4, (u % 4) // 2, r, u % 2, cs]
        for u in range(12):
            wx[ch, 8, u] = st[q, j, 3 + u // 4, (u % 4) // 2, ch % 16, u % 2, cs]
    return wx[..., :9], wx[..., 9:]


# ---------------------------------------------------------------- geometry (from the code) -----------------------------------------------
def pick_tile_c(ho, wo, s):
    """ops.pick_tile_c restated (the host test holds the two together)"""
    best = None
    for tw in range(2, 65, 2):
        th = min(64 // tw, ho)
        pos = (s * (th - 1) + 3) * (s * (tw - 1) + 3)
        if th < 1 or pos > 320:
            continue
        key = (_cdiv(ho, th) * _cdiv(wo, tw), pos)
        if best is None or key < best[0]:
            best = (key, th, tw)
    return best[1], best[2]


def pick_tile_m(ho, wo, s):
    """ops.pick_tile_m restated"""
    best = None
    for tw in range(1, 33):
        for th in range(1, 32 // tw + 1):
            pos = (s * (th - 1) + 3) * (s * (tw - 1) + 3)
            if pos > 160 or th > ho or tw > max(wo, 1) * 2:
                continue
            key = (_cdiv(ho, th) * _cdiv(wo, tw), pos)
            if best is None or key < best[0]:
                best = (key, th, tw)
    return best[1], best[2]


def pick_tile(ho, wo):
    """ops.pick_tile restated"""
    best = None
    for nct in range(1, 9):
        tw = _cdiv(wo, nct)
        if tw > 64:
            continue
        th = min(max(1, 64 // tw), ho)
        eff = (ho * wo) / (nct * _cdiv(ho, th) * 64.0)
        if best is None or eff > best[0] + 1e-9:
            best = (eff, th, tw)
    return (1, 64) if best is None else (best[1], best[2])


def rf3c_claim(storage, n_out, s, raw):
    """rc_dispatch_fwd: N <= 64: MT 1, 4 waves; N <= 128 (fp32: any wider N, in groups of 128): MT 2, 4 waves; bf16 wider: MT 2, 8 waves"""
    mt, nw = (2, 8) if (storage == BF16 and n_out > 128) else ((2, 4) if n_out > 64 else (1, 4))
    return f"ly_rf3c_fwd_kernel<{'__bf16' if storage == BF16 else 'float'}, {mt}, {nw}, {s}, {'true' if raw else 'false'}>"


def rf3m_claim(n_out):
    return f"ly_rf3m_fwd_kernel<{4 if n_out % 128 == 0 else 2}, false>"


def rf3_claim(storage, n_out, blocks):
    """rf3_dispatch: MT 1 / 2 / 4 for N <= 64 / <= 128 / wider; MT 4 with more than 256 blocks: the scalar-weight kernel"""
    mt = 4 if n_out > 128 else (2 if n_out > 64 else 1)
    return f"ly_rfcbam3{'_sw' if mt == 4 and blocks > 256 else ''}_kernel<{'__bf16' if storage == BF16 else 'float'}, {mt}>"


def stats1_claim(storage, c, part):
    """rfcbam_stats_entry, k = 1: with part pre1v<T, ceil(C / VW / 16)> when C is a multiple of the vector width and that is <= 4, else pre1;
    without part stats1"""
    t = "__bf16" if storage == BF16 else "float"
    if not part:
        return f"ly_rfcbam_stats1_kernel<{t}>"
    vw = vw_of(storage)
    vpl = _cdiv(c // vw, 16)
    return f"ly_rfcbam_pre1v_kernel<{t}, {vpl}>" if c % vw == 0 and vpl <= 4 else f"ly_rfcbam_pre1_kernel<{t}>"


def gemm_claim(storage, kdim, n_out):
    """ly_gemm_dispatch with the affine prologue (tests/test_describe_host.py quotes the rules): N > 64: <4, 2, 4>, N > 32: <4, 1, 4>; K in one /
    two chunks of 16 vectors resident (NCH 1 / 2), longer K: 0; FAST 1 with NCH > 0, else 0"""
    t = "__bf16" if storage == BF16 else "float"
    tile = "4, 2, 4" if n_out > 64 else "4, 1, 4"
    nch = _cdiv(kdim, 16 * vw_of(storage))
    nch = nch if nch <= 2 else 0
    return f"ly_gemm_kernel_d2<{t}, {t}, {tile}, 0, 2, {nch}, {1 if nch else 0}>"


def part_chain(hw, c, slices):
    """ly_colsum: groups = 256 / (C / 4) pixel lanes, ceil(per / groups) + groups; pre1v: ceil(per / 16) + 16; pre1: ceil(per / 4) + 4 — the largest"""
    per = _cdiv(hw, slices)
    groups = max(THREADS // (c // 4), 1)
    return max(_cdiv(per, groups) + groups, _cdiv(per, 16) + 16, _cdiv(per, 4) + 4)


def tile_part_chain(s, th, tw):
    return max(12, _cdiv(s * th * s * tw, 8) + 8, 17)


# ---------------------------------------------------------------- beacons and builders ----------------------------------------------------
def beacons(n, ho, wo, th, tw, c, k):
    """[(image, oy, ox, tap, channel)]: the same placements for both families"""
    kk = k * k
    spots = [(0, 0, 0, 0), (0, ho - 1, wo - 1, kk - 1), (0, min(th, ho) - 1, min(tw, wo) - 1, kk // 2), (0, 0, wo - 1, min(2, kk - 1))]
    if n > 1:
        spots.append((1, 0, 0, min(3, kk - 1)))
    out, seen = [], set()
    for img, oy, ox, t in spots:
        if (img, oy, ox) in seen:
            continue
        seen.add((img, oy, ox))
        ch = 1 if not out else c - len(out)
        out.append((img, oy, ox, t, ch))
    return out


def _gen(*key):
    return torch.Generator().manual_seed(_seed("rfcbam_fwd", *key))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64)


def _ri(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _pow2(g, choices, *shape):
    return torch.tensor(choices, dtype=torch.float64)[torch.randint(0, len(choices), shape, generator=g)]


def inputs(cid, n, h, w, c, k, s, n_out, th, tw, storage, family):
    """every operand of one case as stored: x [n, H, W, C] in `storage`; p = dict(w, a, b, wf) fp32; ca [n, C], rfa [n, k Ho, k Wo], wc [O, C, KK],
    es, esh [O] fp32; `beacons`.  The maps ca / rfa are the builder's own (each entry point is tested on its own operands)"""
    g = _gen(cid, str(storage), family)
    kk = k * k
    ho, wo = out_hw(h, w, k, s)
    lat = family == "lattice"
    bl = beacons(n, ho, wo, th, tw, c, k)
    if lat:
        x = _ri(g, -4, 4, n, h, w, c) / 4
        wg = _ri(g, -2, 2, c, kk, kk) / 2
        a = _pow2(g, (0.5, 1.0, -0.5, 1.0), c, kk)
        b = _ri(g, -8, 8, c, kk) / 8
        ca, rfa = _pow2(g, (0.5, 1.0), n, c), _pow2(g, (0.5, 1.0), n, k * ho, k * wo)
        wc = _ri(g, -4, 4, n_out, c, kk) / 4
        es, esh = _pow2(g, (0.5, 1.0, 2.0), n_out), _ri(g, -8, 8, n_out) / 8
        xbig, wbig, wcb, bdead = 2.0, 1.0, 1.0, -12.0
    else:
        x = _randn(g, n, h, w, c) * (_rand(g, c) * 0.5 + 0.75)
        wg = _randn(g, c, kk, kk) * 0.4
        a = (_rand(g, c, kk) + 0.5) * torch.where(_rand(g, c, kk) < 0.25, -1.0, 1.0)
        b = _randn(g, c, kk) * 0.5
        ca, rfa = 0.5 + 0.5 * _rand(g, n, c), 0.5 + 0.5 * _rand(g, n, k * ho, k * wo)      # comparable operands: see "operand allowance"
        wc = (0.5 + 0.5 * _rand(g, n_out, c, kk)) * torch.where(_rand(g, n_out, c, kk) < 0.5, -1.0, 1.0) / math.sqrt(c * kk)
        es, esh = (_rand(g, n_out) + 0.5) * torch.where(_rand(g, n_out) < 0.2, -1.0, 1.0), _randn(g, n_out) * 0.3
        xbig, wbig, wcb, bdead = 64.0, 2.0, WBIG, -40.0
    if kk > 1:
        b[:, DEAD] = bdead
    sign = torch.where(torch.arange(n_out) % 2 == 0, 1.0, -1.0).double()
    if not lat:
        for _, _, _, _, ch in bl:
            x[..., ch] = 0.0                                         # rounded: the channel is dark but for its beacon: its large wc multiplies nothing else
    for img, oy, ox, t, ch in bl:
        # the beacon's operand B = relu(a w x) ca rfa = 1.5 * 2 * 64 = 192 (lattice: 2) is itself a bf16 value: the centre weight of its tap is the
        # channel's only weight and its shift is zero, ca = rfa = 1 there (see "operand allowance" in the docstring)
        if t == DEAD and kk > 1:
            raise AssertionError("a beacon on the dead tap")
        x[img, s * oy, s * ox, ch] = xbig
        wg[ch] = 0.0
        wg[ch, t, kk // 2] = wbig
        dead = b[ch, DEAD].clone() if kk > 1 else None
        b[ch] = 0.0
        if kk > 1:
            b[ch, DEAD] = dead
        a[ch, t] = 1.0 if lat else 1.5
        ca[img, ch] = 1.0
        rfa[img, k * oy + t // k, k * ox + t % k] = 1.0
        wc[:, ch, t] = wcb * sign
    x = x.to(storage)
    wg, a, b = wg.float(), a.float(), b.float()
    p = dict(w=wg, a=a, b=b, wf=(wg * a.unsqueeze(-1)).contiguous())
    return dict(x=x, p=p, ca=ca.float(), rfa=rfa.float(), wc=wc.float(), es=es.float(), esh=esh.float(), beacons=bl, n=n, h=h, w=w, c=c, k=k, s=s,
                ho=ho, wo=wo, th=th, tw=tw, n_out=n_out, storage=storage, family=family)


def want_for(x, route, raw, **defects):
    """(v, M_v) of a case on a route, float64, from the stored values"""
    q = stored_params(x["p"], route)
    gdef = {key: val for key, val in defects.items() if key in ("clamp", "swap_tap", "folded_in_raw")}
    return gen_v(d(x["x"]), q, x["k"], x["s"], raw, **gdef), gen_v_mag(d(x["x"]), q, x["k"], x["s"], raw)


def se_inputs_fwd(cid):
    """part [n, slices, C] of either sign (sums of x), wa [R, C], wb [C, R] of tests/rfcbam_ref.SE_CASES' shapes; two saturated channels"""
    n, c, r, slices = SE_CASES[cid]
    g = _gen("se", cid)
    hw = 64 * slices + 3
    part = (_randn(g, n, slices, c) * hw / slices).float()
    wb = _randn(g, c, r)
    wb[3 % c], wb[5 % c] = 40.0, -40.0
    return dict(part=part, wa=(_randn(g, r, c) / math.sqrt(c)).float(), wb=wb.float(), hw=hw, n=n, c=c, r=r, slices=slices)


def se_x_inputs(cid, storage, family):
    """x [n, HW, C] for ly_colsum / ly_se_fwd at the widths and slice counts of SE_CASES, HW = 2 slices + 1 (no multiple of the slice count)"""
    n, c, r, slices = SE_CASES[cid]
    hw = 2 * slices + 1
    g = _gen("sex", cid, str(storage), family)
    x = (_ri(g, -4, 4, n, hw, c) / 4 if family == "lattice" else _randn(g, n, hw, c) * (_rand(g, c) * 2 + 0.3)).to(storage)
    return dict(x=x, n=n, c=c, r=r, slices=slices, hw=hw, family=family, k=1)


def k1_inputs(cid, storage, family):
    """the operands of a k = 1 statistics case: inputs() on a 1 x HW map"""
    row = K1_CASES[cid]
    return inputs(f"k1:{cid}", row[0], 1, row[1], k1_c(row, storage), 1, 1, 16, 1, 64, storage, family)


MAP_CASES = dict(RFA_CASES)
MAP_CASES.update({"tail-wk-7": (2, 5, 7), "wk-3-under-a-vector": (1, 4, 3), "hk-1": (2, 1, 9)})


def map_inputs(cid):
    n, hk, wk = MAP_CASES[cid]
    g = _gen("map", cid)
    mm = torch.stack((_rand(g, n, hk, wk) * 3, _rand(g, n, hk, wk)), -1)
    mm[:, 0, 0], mm[:, hk - 1, wk - 1] = 40.0, 40.0
    w18 = _randn(g, 18) * 0.5
    w18[4], w18[13] = 1.0, -2.0                                       # the two corners saturate, one each way on the wider maps
    return dict(mm=mm.float(), w18=w18.float(), n=n, hk=hk, wk=wk)


# ---------------------------------------------------------------- case tables -------------------------------------------------------------
# k = 3 shapes: id -> (n, H, W, C, s, TH, TW); TH None: ops.pick_tile_c / pick_tile_m / pick_tile of the output map
RC_SHAPES = {
    "c32-s1-1x1-map-tile1x2": (1, 1, 1, 32, 1, 1, 2),
    "c32-s1-pick-one-tile": (2, 6, 10, 32, 1, None, None),
    "c32-s1-ragged-4x6": (1, 11, 13, 32, 1, 4, 6),
    "c64-s2-odd-7x9-pick": (2, 7, 9, 64, 2, None, None),
    "c64-s2-4x16-maxpos": (2, 9, 40, 64, 2, 4, 16),
    "c96-s2-3img-8x8-maxpos": (3, 18, 20, 96, 2, 8, 8),
    "c96-s1-odd-5x7-tile2x4": (1, 5, 7, 96, 1, 2, 4),
}
# ly_rf3c_fwd: id -> (shape id, N, raw, mode); modes: relu, linear, stats-out, stats-only
RC_FWD = {
    "n64-mt1-folded-relu": ("c32-s1-ragged-4x6", 64, False, "relu"),
    "n64-mt1-raw-stats-out-1x1": ("c32-s1-1x1-map-tile1x2", 64, True, "stats-out"),
    "n72-ragged-channel-tile-raw-relu": ("c32-s1-pick-one-tile", 72, True, "relu"),
    "n128-mt2-folded-relu-s2-odd": ("c64-s2-odd-7x9-pick", 128, False, "relu"),
    "n128-mt2-raw-stats-only": ("c64-s2-4x16-maxpos", 128, True, "stats-only"),
    "n128-mt2-raw-linear": ("c96-s1-odd-5x7-tile2x4", 128, True, "linear"),
    "n256-wide-folded-relu-3img": ("c96-s2-3img-8x8-maxpos", 256, False, "relu"),
    "n256-wide-raw-stats-out": ("c64-s2-odd-7x9-pick", 256, True, "stats-out"),
    "n80-partial-block-folded-linear": ("c64-s2-4x16-maxpos", 80, False, "linear"),
}
RC_LD = {"ldx": "n64-mt1-folded-relu", "ldo": "n128-mt2-folded-relu-s2-odd"}
# ly_rf3m: id -> (n, H, W, C, s, TH, TW, N); 8 wave tiles per block
RM_CASES = {
    "c32-s1-n64-mt2-25-tiles-partial-last-block": (1, 5, 20, 32, 1, 1, 4, 64),
    "c64-s2-n128-mt4-4x8-maxpos-3img-straddle": (3, 16, 24, 64, 2, 4, 8, 128),
    "c32-s2-n128-mt4-odd-pick-6-tiles-one-partial-block": (1, 21, 23, 32, 2, None, None, 128),
    "c64-s1-n64-mt2-pick-1x1-map": (2, 1, 1, 64, 1, None, None, 64),
}
# lane = pixel: ly_rfcbam_stats k = 3: id -> (n, H, W, C, s, TH, TW)
ST3_CASES = {
    "c16-s1-pick": (2, 6, 9, 16, 1, None, None),
    "c48-s2-odd-2x2": (2, 7, 5, 48, 2, 2, 2),
    "c48-s3-2x2": (1, 8, 11, 48, 3, 2, 2),
    "c16-s2-pick-3img": (3, 12, 10, 16, 2, None, None),
}
# ly_rfcbam3_fwd: id -> (n, H, W, C, s, TH, TW, N, mode)
RF3_CASES = {
    "c16-n64-mt1-s1-pick-relu": (2, 6, 9, 16, 1, None, None, 64, "relu"),
    "c48-n128-mt2-s2-odd-2x2-stats-out": (2, 7, 5, 48, 2, 2, 2, 128, "stats-out"),
    "c48-n72-s1-2x2-linear": (1, 5, 4, 48, 1, 2, 2, 72, "linear"),
    "c16-n256-mt4-lds-64-blocks": (1, 16, 16, 16, 1, 2, 2, 256, "relu"),
    "c16-n256-mt4-sw-320-blocks": (5, 16, 16, 16, 1, 2, 2, 256, "relu"),
    "c16-n256-mt4-s2-stats-only": (2, 9, 12, 16, 2, None, None, 256, "stats-only"),
}
RF3_LD = {"ldx": "c16-n64-mt1-s1-pick-relu", "ldo": "c48-n72-s1-2x2-linear"}
# k = 1 statistics: id -> (n, HW, C fp32, C bf16, slices; None: ops.rfcbam_stats' own, 0: no part)
K1_CASES = {
    "pre1v-1-hw100": (2, 100, 64, 128, None),
    "pre1v-2-hw37-one-slice": (3, 37, 128, 256, None),
    "pre1v-3-hw200-slices7-ragged": (1, 200, 192, 384, 7),
    "pre1v-4-hw130": (2, 130, 256, 512, None),
    "pre1-plain-c260-c12": (2, 70, 260, 12, 3),
    "pre1-plain-c520-c768-limit": (1, 45, 520, 768, None),
    "stats1-small": (2, 37, 64, 64, 0),
    "stats1-block-cap-c4": (1, 16500, 4, 4, 0),
}
# the k = 1 contraction: id -> (n, H, W, K, N)
GEMM_CASES = {"k32-n64": (2, 5, 7, 32, 64), "k160-n64": (2, 3, 5, 160, 64), "k32-n256": (2, 4, 4, 32, 256), "k160-n256": (2, 5, 7, 160, 256)}


def case(table, cid):
    """one row of a k = 3 / contraction table as dict(n, h, w, c, k, s, n_out, th, tw, raw, mode, ho, wo); tiles left open are picked as the
    route's ops.pick_tile* would"""
    raw, mode, n_out, k = False, "relu", 16, 3
    if table == "rc_fwd":
        sid, n_out, raw, mode = RC_FWD[cid]
        n, h, w, c, s, th, tw = RC_SHAPES[sid]
    elif table == "rc_stats":
        n, h, w, c, s, th, tw = RC_SHAPES[cid]
    elif table == "rm":
        n, h, w, c, s, th, tw, n_out = RM_CASES[cid]
    elif table == "st3":
        n, h, w, c, s, th, tw = ST3_CASES[cid]
    elif table == "rf3":
        n, h, w, c, s, th, tw, n_out, mode = RF3_CASES[cid]
    else:
        n, h, w, c, n_out = GEMM_CASES[cid]
        k, s, th, tw = 1, 1, 1, 64
    ho, wo = out_hw(h, w, k, s)
    if th is None:
        th, tw = pick_tile_c(ho, wo, s) if table.startswith("rc") else (pick_tile_m(ho, wo, s) if table == "rm" else pick_tile(ho, wo))
    return dict(n=n, h=h, w=w, c=c, k=k, s=s, n_out=n_out, th=th, tw=tw, raw=raw, mode=mode, ho=ho, wo=wo)


def case_inputs(table, cid, storage, family):
    q = case(table, cid)
    return inputs(f"{table}:{cid}", q["n"], q["h"], q["w"], q["c"], q["k"], q["s"], q["n_out"], q["th"], q["tw"], storage, family), q


TABLES = dict(rc_fwd=RC_FWD, rc_stats=RC_SHAPES, rm=RM_CASES, st3=ST3_CASES, rf3=RF3_CASES, gemm=GEMM_CASES)


def k1_c(v, storage):
    return v[3] if storage == BF16 else v[2]


def k1_slices(hw, want):
    return max(1, min(hw // 64, 128)) if want is None else want


# ---------------------------------------------------------------- judges ------------------------------------------------------------------
def _say(what, **figs):
    print(f"{what}: " + "  ".join(f"{k} {v:.3g}" for k, v in figs.items()))


def _ratio(err, bound):
    ok = bound > 0
    return float((err[ok] / bound[ok]).max()) if bool(ok.any()) else 0.0


def _bounded(got, want, bound, what):
    got = d(got).reshape(want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    err = (got - want).abs()
    r = _ratio(err, bound)
    _say(what, err_over_bound=r)
    if bool((err > bound).any()):
        _fail(what, err, bound)
    return r


def _exact(got, want, what, storage=F32):
    """lattice: the float64 reference rounded once to the storage type IS the result"""
    w = want.to(storage)
    g = got.detach().cpu().reshape(w.shape)
    bad = int((g != w).sum()) + int((torch.isnan(g.float())).sum())
    _say(what, unequal=bad)
    assert g.dtype == w.dtype and bad == 0, f"{what}: {bad} of {w.numel()} elements differ from the exact result; first at " \
                                            f"{tuple(int(i) for i in torch.nonzero(g != w)[0]) if bad else ()}"
    return 0.0


def judge_mm(got, x, v, vm, what):
    """got [n, k Ho, k Wo, 2] fp32"""
    n, ho, wo, k, c = x["n"], x["ho"], x["wo"], x["k"], x["c"]
    want = mm_of(v, n, ho, wo, k)
    if x["family"] == "lattice":
        _exact(got[..., 0], want[..., 0], what + " max")
        if c & (c - 1) == 0:
            return _exact(got[..., 1], want[..., 1], what + " mean")
        return _bounded(got[..., 1], want[..., 1], ULP_MEAN * want[..., 1].abs(), what + " mean (sum * fl(1 / C): one unit in the last place)")
    m_max, m_mean, t_mean = mm_mag(v, vm, n, ho, wo, k)
    r0 = _bounded(got[..., 0], want[..., 0], U24 * K["v"] * m_max, what + " max")
    r1 = _bounded(got[..., 1], want[..., 1], U24 * (K["mean"] * m_mean + (c + 8) * t_mean), what + " mean")
    return max(r0, r1)


def judge_part(got, x, want, want_abs, chain, what):
    """got [n, slices, C] fp32 against the float64 partials in the SAME slicing (want_abs: of |x|): slice by slice, and folded over the slices
    against the image sum"""
    if x["family"] == "lattice":
        _exact(got, want, what + " part")
        return _exact(d(got).sum(1).float(), want.sum(1), what + " part folded")
    r = _bounded(got, want, U24 * chain * want_abs, what + " part")
    return max(r, _bounded(d(got).sum(1), want.sum(1), U24 * chain * want_abs.sum(1), what + " part folded"))


def judge_ca(got, x, what):
    a = (d(x["part"]), d(x["wa"]), d(x["wb"]), x["hw"])
    want = se_ca(*a)["ca"]
    return _bounded(got, want, se_ca_bound(*a, chains=se_chains(x["c"], x["r"], x["slices"]))[1], what + " ca")


def judge_rfa(got, x, what):
    pre, mag = rfa_pre(d(x["mm"]), d(x["w18"]))
    e = U24 * (K["rfa"] + RFA_CHAIN) * mag
    return _bounded(got, torch.sigmoid(pre), _sig_bound(pre, e, "rfa"), what + " rfa")


def judge_out(got, x, v, vm, mode, what, rowscale=False, wc=None):
    """got: dict(out [m, O] as stored or None, stats [stripes, 2 O] doubles or None); mode relu / linear / stats-out / stats-only"""
    n, ho, wo, k, c, st = x["n"], x["ho"], x["wo"], x["k"], x["c"], x["storage"]
    g, lin = torch.clamp(v, min=0.0), mode != "relu"
    a = (d(x["ca"]), d(x["rfa"]), stored_wc(x["wc"], st) if wc is None else wc, d(x["es"]), d(x["esh"]), n, ho, wo, k)
    want = contract(g, *a, linear=lin, rowscale=rowscale)
    e_u = contract_bound(g, vm, *a, st, u_chain(c, k, rowscale), rowscale=rowscale)
    lat = x["family"] == "lattice"
    worst = 0.0
    if got.get("out") is not None:
        if lat:
            _exact(got["out"], want["out"], what + " out", st)
        else:
            worst = _bounded(got["out"], want["out"], e_u + (BF16_EPS * want["out"].abs() if st == BF16 else 0.0), what + " out")
    if got.get("stats") is not None:
        s1, s2 = fold(got["stats"])
        if lat:
            _exact(s1, want["s1"], what + " s1", torch.float64)
        else:
            worst = max(worst, _bounded(s1, want["s1"], U24 * STATS_CHAIN * want["u"].abs().sum(0) + e_u.sum(0), what + " s1"))
        u = want["u"].abs()
        e_sq = U24 * (STATS_CHAIN + 1) * (u * u).sum(0) + ((2 * u + e_u) * e_u).sum(0)
        worst = max(worst, _bounded(s2, want["s2"], e_sq if not lat else U24 * (STATS_CHAIN + 1) * (u * u).sum(0), what + " s2"))
    return worst


def beacon_report(x, v, wc):
    """per beacon: (its product's share of sum |wc B| at output channel 0, the product over the elementwise bound)"""
    n, ho, wo, k, st = x["n"], x["ho"], x["wo"], x["k"], x["storage"]
    g = torch.clamp(v, min=0.0)
    a = (d(x["ca"]), d(x["rfa"]), wc, d(x["es"]), d(x["esh"]), n, ho, wo, k)
    b = contract(g, *a)["B"]
    tot = torch.einsum("mtc,ct->m", b, wc[0].abs())
    e_u = contract_bound(g, gen_v_mag(d(x["x"]), stored_params(x["p"], "rf3c"), k, x["s"], False), *a, st, u_chain(x["c"], k))
    out = []
    for img, oy, ox, t, ch in x["beacons"]:
        m = (img * ho + oy) * wo + ox
        prod = float(b[m, t, ch] * wc[0, ch, t].abs() * d(x["es"])[0].abs())
        out.append((float(b[m, t, ch] * wc[0, ch, t].abs() / tot[m]), prod / float(e_u[m, 0] + (BF16_EPS * prod if st == BF16 else 0.0))))
    return out


# ---------------------------------------------------------------- measurements (reference only) -------------------------------------------
def _r(got, want, mag, floor=0.0):
    ok = mag > 0
    return float((((d(got) - want).abs() - floor).clamp(min=0.0) / (U24 * mag).clamp(min=1e-300))[ok].max()) if bool(ok.any()) else 0.0


def measure_k():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _measure_k()
    finally:
        torch.set_num_threads(threads)


def _measure_k():
    worst = {key: 0.0 for key in K}
    up = lambda key, val: worst.__setitem__(key, max(worst[key], val))
    for table, rows in TABLES.items():
        for cid in rows:
            for st in (F32, BF16):
                if table == "rm" and st == F32:
                    continue
                x, q = case_inputs(table, cid, st, "rounded")
                n, k, s, ho, wo, rs = q["n"], q["k"], q["s"], q["ho"], q["wo"], q["k"] == 1
                pq = stored_params(x["p"], "rf3m" if table == "rm" else "rf3c")
                p32 = {key: val.float() for key, val in pq.items()}
                xd = d(x["x"])
                for raw in ((False, True) if table in ("rc_stats", "rc_fwd") else (False,)):
                    v, vm = gen_v(xd, pq, k, s, raw), gen_v_mag(xd, pq, k, s, raw)
                    v32 = gen_v(xd.float(), p32, k, s, raw)
                    up("v", _r(v32, v, vm))
                    up("mean", _r(mm_of(v32, n, ho, wo, k)[..., 1], mm_of(v, n, ho, wo, k)[..., 1], mm_mag(v, vm, n, ho, wo, k)[1]))
                    if table in ("rc_stats", "st3"):
                        continue
                    a = (d(x["ca"]), d(x["rfa"]), stored_wc(x["wc"], st), d(x["es"]), d(x["esh"]), n, ho, wo, k)
                    a32 = tuple(t.float() if torch.is_tensor(t) else t for t in a)
                    u32 = contract(torch.clamp(v32, min=0.0), *a32, rowscale=rs)["u"]
                    g = torch.clamp(v, min=0.0)
                    up("u", _r(u32, contract(g, *a, rowscale=rs)["u"], contract_bound(g, vm, *a, st, None, rowscale=rs, allowance=False)))
    for cid in K1_CASES:
        for st in (F32, BF16):
            x = k1_inputs(cid, st, "rounded")
            pq = stored_params(x["p"], "rf3c")
            xd = d(x["x"])
            v, vm = gen_v(xd, pq, 1, 1, False), gen_v_mag(xd, pq, 1, 1, False)
            v32 = gen_v(xd.float(), {key: val.float() for key, val in pq.items()}, 1, 1, False)
            up("v", _r(v32, v, vm))
            up("mean", _r(mm_of(v32, x["n"], 1, x["wo"], 1)[..., 1], mm_of(v, x["n"], 1, x["wo"], 1)[..., 1], mm_mag(v, vm, x["n"], 1, x["wo"], 1)[1]))
    for cid in SE_CASES:
        x = se_inputs_fwd(cid)
        a = (d(x["part"]), d(x["wa"]), d(x["wb"]), x["hw"])
        o, o32 = se_ca(*a), se_ca(*[t.float() if torch.is_tensor(t) else t for t in a])
        e_z, _ = se_ca_bound(*a)
        up("ca", _r(o32["z"], o["z"], e_z / K["ca"]))
        sg = o["ca"]
        up("ca", _r(o32["ca"], sg, sg * (1 - sg) * (d(o32["z"]) - o["z"]).abs() / U24 + sg, TINY))
    for cid in MAP_CASES:
        x = map_inputs(cid)
        pre, mag = rfa_pre(d(x["mm"]), d(x["w18"]))
        pre32, _ = rfa_pre(x["mm"], x["w18"])
        up("rfa", _r(pre32, pre, mag))
        sg = torch.sigmoid(pre)
        up("rfa", _r(torch.sigmoid(pre32), sg, sg * (1 - sg) * (d(pre32) - pre).abs() / U24 + sg, TINY))
    return worst
