"""The RFCBAMConv backward kernels of the streamed and the k = 1 routes, entry point by entry point and pass by pass against float64
(tests/rfcbam_ref.py: references, judges with conditioned bounds, input builders, case tables; tests/test_rfcbam_host.py shows on the CPU
that those judges reject subtly wrong results and that every case id takes the branch it names).  ly_se_bwd goes through ops.se_bwd, everything
else through lead_yolo_amd.capi exactly as grad.py calls it.  No judge compares a kernel with itself except the bit-for-bit repeatability
(plain stores only — nothing behind a float atomic) and untouched-operand checks.  Every judge prints its worst figures before it asserts; every
test asserts the premises first: NO element in the ReLU band, NO map position with an undecided maximum, NO undecided SE unit.

Measured on the MI355X, worst over all cases, next to torch's float32 evaluation of the same references on the CPU:
    elementwise, what is left of the error after the storage allowance, in units of 2^-24 M   (K of tests/rfcbam_ref.py; CPU float32)
        ug 3.06 (13; 3.21)   cd / gmax: attn 2.50, rf3s 2.63 (15; 3.57)   dv: relu 2.59, rf3s 2.26 (12; 2.78)   dug 2.11 (11; 2.57)
        dx 6.08 (13 + its chain of up to 83; 3.01 — torch's float32 einsum does not add the 81 products one by one)   d_mm 4.40 (17; 4.17)
        ly_rf1_bwd cd / gmax / dx 3.24 (18; 4.29)
    sums, worst |err| / bound
        ly_rf_bwd_attn d_rfa / d_ca 0.11   ly_rf_bwd_relu s1 / s2 0.14   ly_rf3s_bwd 0.13   ly_rf1_bwd d_rfa / d_ca / s1 / s2 0.13, dgw 0.13
        dwg (rows folded in float64) 0.18   dw18 0.024   ly_se_bwd dgap 0.044, dWa 0.025, dWb 0.12   (K_se 4; CPU float32 0.93)
No defect was found in the kernels: nothing in csrc/ changed with these tests.  The -0.0 case does not bite: fmaxf(fma(a, +0, -0.0), 0) comes
out as +0 on the device (no sign bit set in any gmax), so the integer atomicMax of ly_rf_bwd_attn never sees 0x80000000.

branch of the kernels                                              ->  case id (tables of tests/rfcbam_ref.py) or test
  thread = channel kernels (fp32, bf16): ly_rf_generate, ly_rf_bwd_attn, ly_rf_bwd_relu, ly_rf_bwd_gen, ly_rf_bwd_dx
    four pixel sub-groups (cb = 64); odd H and W: dx's parity gather;  TC_CASES subs4-odd-parity-straddle-c64
      a block whose chunk straddles two images (addend form 2)
    cb = 128 with 56 clamped lanes; dx tiled (s2t), partial second    cb128-clamped-s2t-partial-c72
      channel group, Wo = 6 no multiple of the tile (a live halo column)
    one sub-group with an idle wave (cb = 192); generic stride-1      subs1-idlewave-s1-c192
      gather; a wave of -0.0 under ly_rf_bwd_attn's integer atomicMax
    two channel groups, the second clamped; dx tiled, five 64-channel gy2-clamped-s2t-c320
      groups; in fp32 the width past ly_rf3s_bwd (the route's fallback)
    k = 1, six live lanes, the bf16 pair exchange with one tap        k1-c6
    a chunk longer than an image (addend form 1); every tap of the    chunk-over-image-add1-c8
      corner pixels padded
    x with ldx > C (generate, gen)                                    test_generate / test_gen [cb128-*], [k1-c6]
    dx without addend; dx with lddx > C into a sentinel allocation    test_dx[*-noadd], [*-ld]
    gen with part_rows 4 and 512; 3 refused                           test_gen[*-rows4], [*-rows512]; test_refusals
  ly_rf3s_bwd passes 0 / 1 (fp32, bf16)
    one lane per pixel, 36 threads; lpp 6 -> 8 (bf16 3 -> 4) with     RF3S_CASES c4-8-*, c24-24-*, c64-64-*, c160-160-*, c256-512-*
      idle lanes, pp = 4; lpp2 64 / 32 with pp 1 / 2; the full LDS fold
    Ho x Wo = 1x1, 3x5, 9x11; n = 1, 3; more than one block per image  *-9x11-*
  ly_rf1_bwd passes 0 / 1 / 2 (fp32, bf16)
    the same widths; HW = 1, 37, 400, 1031 (a partial last trip); n    RF1_CASES c*-hw*-n*
    dgw a prefilled fp32 target / a zeroed float64 scratch            test_rf1[*-f32], [*-f64]
    ldx > C and lddx > C; dgap = NULL                                 test_rf1_ld_and_no_dgap
  ly_rfa_bwd
    one position; inside one tile; an exact tile; a halo across four   RFA_CASES
      tiles; 3 x 200; 513 tiles behind the 512-block cap
    dw18 a prefilled fp32 target / a zeroed float64 scratch           test_rfa_bwd[*-f32], [*-f64]
  ly_se_bwd (ops.se_bwd)
    nq = 2 ... 256; nq = 40 does not divide 256; eight images exactly, SE_CASES
      one over, two trips plus one
    d_ca fp32 / float64; dwa, dwb prefilled (added, not stored)       test_se_bwd[*-f32], [*-f64]
  refusals before any launch                                          test_refusals
"""
import ctypes

import pytest
import torch

from tests import rfcbam_ref as R

pytestmark = pytest.mark.gpu

DT_IDS = {R.F32: "f32", R.BF16: "bf16"}
BOTH = [pytest.param(R.F32, id="f32"), pytest.param(R.BF16, id="bf16")]
F64 = [pytest.param(False, id="f32"), pytest.param(True, id="f64")]
SENTINEL = 768.0                                 # (on the bf16 grid)
LD_CASES = ("cb128-clamped-s2t-partial-c72", "k1-c6")


@pytest.fixture(autouse=True)
def _no_sink_left_behind(monkeypatch):
    """every test starts without a gradient sink (a fused optimiser's first step installs one process-wide) and puts back what it found"""
    from lead_yolo_amd import ops
    monkeypatch.setattr(ops, "SINK", None)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a CUDA/ROCm device"
    return torch.device("cuda:0")


def _place(t, extra, dev, fill=True):
    """t [..., C] as rows inside a [rows, C + extra vectors] allocation filled with a sentinel, the slice one 16-byte vector in (extra > 0).
    -> (full, view [rows, C], ld)"""
    c = t.shape[-1]
    rows = t.reshape(-1, c)
    vw = R.vw_of(t.dtype)
    ld, off = c + extra * vw, vw if extra else 0
    full = torch.full((rows.shape[0], ld), SENTINEL, dtype=t.dtype, device=dev)
    if fill:
        full[:, off:off + c] = rows.to(dev)
    return full, full[:, off:off + c], ld


def _outside(full, c, extra, vw):
    """the sentinel columns of a _place allocation"""
    return torch.cat((full[:, :vw if extra else 0], full[:, (vw if extra else 0) + c:]), 1)


def _to(x, keys, dev):
    return {q: x[q].to(dev).contiguous() for q in keys}


def _kept(dv, keep):
    return all(torch.equal(dv[q], keep[q]) for q in keep)


def _capi():
    from lead_yolo_amd import capi
    return capi, capi.lib(), capi.ptr, capi.stream_ptr()


# ---------------------------------------------------------------- thread = channel kernels -------------------------------------------------
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("cid", list(R.TC_CASES))
def test_generate(cid, dtype):
    """ly_rf_generate: ug = sum_u wg x_u, zero padded; x a channel slice of a wider sentinel allocation on two cases; two calls, same bits"""
    capi, lib, p, st = _capi()
    n, h, w, c, k, s = R.TC_CASES[cid]
    dev = _dev()
    x = R.tc_inputs(cid, dtype)
    full, xv, ldx = _place(x["x"], 1 if cid in LD_CASES else 0, dev)
    keep = full.clone()
    wg = x["wg"].to(dev)
    mo = n * x["ho"] * x["wo"]
    ug = [torch.full((mo, k * k, c), SENTINEL, dtype=dtype, device=dev) for _ in range(2)]
    for t in ug:
        capi.check(lib.ly_rf_generate(p(xv), ldx, n, h, w, c, k, s, p(wg), p(t), capi.dtype_code(dtype), st), "ly_rf_generate")
    torch.cuda.synchronize()
    R.judge_generate(ug[0], x, f"generate {cid} {DT_IDS[dtype]}")
    assert torch.equal(ug[0], ug[1]), "two calls differ"
    assert torch.equal(full, keep) and torch.equal(wg.cpu(), x["wg"])


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("cid", list(R.TC_CASES))
def test_attn(cid, dtype):
    """ly_rf_bwd_attn: cd elementwise, d_rfa / gmax on the maps, d_ca per image; gmax = 0 and d_rfa = 0 at the all-negative positions, a
    positive gmax where a whole wave holds -0.0; the operands keep their bits"""
    capi, lib, p, st = _capi()
    n, h, w, c, k, s = R.TC_CASES[cid]
    dev = _dev()
    x = R.tc_inputs(cid, dtype)
    R.assert_premises(R.d(x["ug"]), x["aeff"], R.d(x["bg"]), cid)
    dv = _to(x, R.ATTN_KEYS, dev)
    keep = {q: v.clone() for q, v in dv.items()}
    cd = torch.full_like(dv["ug"], SENTINEL)
    d_rfa, gmax, d_ca = torch.zeros_like(dv["rfa"]), torch.zeros_like(dv["rfa"]), torch.zeros_like(dv["ca"])
    capi.check(lib.ly_rf_bwd_attn(n, h, w, c, k, s, p(dv["ug"]), p(dv["dcd"]), p(dv["ag"]), p(dv["bg"]), p(dv["ca"]), p(dv["rfa"]), p(cd), p(d_rfa), p(gmax),
                                  p(d_ca), capi.dtype_code(dtype), st), "ly_rf_bwd_attn")
    torch.cuda.synchronize()
    what = f"attn {cid} {DT_IDS[dtype]}"
    print(f"{what}: gmax sign bits set {int(torch.signbit(gmax).sum())}, min {float(gmax.min()):.3g}")
    R.judge_attn(dict(cd=cd, d_rfa=d_rfa, gmax=gmax, d_ca=d_ca), x, R.attn_chains("tc", n, x["ho"], x["wo"], c, k, dtype, h, w, s), what)
    gm = R.from_map(R.d(gmax), n, x["ho"], x["wo"], k)
    for m, t in R.allneg_positions(n * x["ho"] * x["wo"], k * k):
        assert float(gm[m, t]) == 0.0 and float(R.from_map(R.d(d_rfa), n, x["ho"], x["wo"], k)[m, t]) == 0.0
    assert _kept(dv, keep), "an operand changed"


@pytest.mark.parametrize("f64", F64)
@pytest.mark.parametrize("cid", list(R.RFA_CASES))
def test_rfa_bwd(cid, f64):
    """ly_rfa_bwd: d_mm elementwise (plain stores: two calls, same bits), dw18 ADDED into a prefilled fp32 target / a zeroed float64 scratch"""
    capi, lib, p, st = _capi()
    n, hk, wk = R.RFA_CASES[cid]
    dev = _dev()
    x = R.rfa_inputs(cid)
    dv = _to(x, ("d_rfa", "rfa", "mm", "w18"), dev)
    keep = {q: v.clone() for q, v in dv.items()}
    pre = 0.0 if f64 else 0.5
    d_mm = [torch.full((n, hk, wk, 2), SENTINEL, device=dev) for _ in range(2)]
    dw = [torch.full((18,), pre, dtype=torch.float64 if f64 else torch.float32, device=dev) for _ in range(2)]
    for a, b in zip(d_mm, dw):
        capi.check(lib.ly_rfa_bwd(p(dv["d_rfa"]), p(dv["rfa"]), p(dv["mm"]), p(dv["w18"]), n, hk, wk, p(a), p(b), int(f64), st), "ly_rfa_bwd")
    torch.cuda.synchronize()
    R.judge_getw(dict(d_mm=d_mm[0], dw18=dw[0]), x, f64, f"rfa_bwd {cid} {'f64' if f64 else 'f32'}", prefill=pre)
    assert torch.equal(d_mm[0], d_mm[1]), "two calls differ"
    assert _kept(dv, keep), "an operand changed"


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("cid", list(R.TC_CASES))
def test_relu(cid, dtype):
    """ly_rf_bwd_relu: dv written over dcd, the BatchNorm sums from the unrounded dv added into zeroed fp32 sums; dv = 0 for every channel of
    an all-negative position and for the all-negative channel"""
    capi, lib, p, st = _capi()
    n, h, w, c, k, s = R.TC_CASES[cid]
    dev = _dev()
    x = R.tc_inputs(cid, dtype)
    R.assert_premises(R.d(x["ug"]), x["aeff"], R.d(x["bg"]), cid)
    dv = _to(x, R.RELU_KEYS + ("gmax",), dev)
    keep = {q: v.clone() for q, v in dv.items() if q != "dcd"}
    kk = k * k
    sums = torch.zeros(2 * kk * c, device=dev)
    capi.check(lib.ly_rf_bwd_relu(n, h, w, c, k, s, p(dv["ug"]), p(dv["dcd"]), p(dv["ag"]), p(dv["bg"]), p(dv["ca"]), p(dv["rfa"]), p(dv["gmax"]), p(dv["d_mm"]),
                                  p(sums), capi.dtype_code(dtype), st), "ly_rf_bwd_relu")
    torch.cuda.synchronize()
    got = dict(dv=dv["dcd"], s1=sums[:kk * c].view(kk, c), s2=sums[kk * c:].view(kk, c))
    R.judge_relu(got, x, R.attn_chains("tc", n, x["ho"], x["wo"], c, k, dtype, h, w, s)[2], f"relu {cid} {DT_IDS[dtype]}")
    for m, t in R.allneg_positions(n * x["ho"] * x["wo"], kk):
        assert float(dv["dcd"][m, t].float().abs().max()) == 0.0
    assert float(dv["dcd"][..., c - 1].float().abs().max()) == 0.0 and _kept(dv, keep)


@pytest.mark.parametrize("rows", [4, 512], ids=["rows4", "rows512"])
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("cid", list(R.TC_CASES))
def test_gen(cid, dtype, rows):
    """ly_rf_bwd_gen: dug written over dv, the generate weight gradient as rows of partial sums (folded here in float64; rows nobody owns stay
    zero); part_rows 4 and 512; x a channel slice on two cases; two calls, same bits"""
    capi, lib, p, st = _capi()
    n, h, w, c, k, s = R.TC_CASES[cid]
    dev = _dev()
    x = R.tc_inputs(cid, dtype)
    full, xv, ldx = _place(x["x"], 1 if cid in LD_CASES else 0, dev)
    dv = _to(x, ("ug", "alpha", "kappa", "lam"), dev)
    keep = dict({q: v.clone() for q, v in dv.items()}, x=full.clone())
    kk = k * k
    g = R.gen_geom(n, h, w, c, k, s, rows)
    outs = []
    for _ in range(2):
        dvv, dwg = x["dv"].to(dev).contiguous(), torch.zeros(rows, c * kk, kk, device=dev)
        capi.check(lib.ly_rf_bwd_gen(p(xv), ldx, n, h, w, c, k, s, p(dv["ug"]), p(dvv), p(dv["alpha"]), p(dv["kappa"]), p(dv["lam"]), p(dwg), rows,
                                     capi.dtype_code(dtype), st), "ly_rf_bwd_gen")
        outs.append((dvv, dwg))
    torch.cuda.synchronize()
    (dug, dwg), (dug2, dwg2) = outs
    R.judge_gen(dict(dug=dug, dwg=dwg.double().sum(0).view(c, kk, kk)), x, R._cdiv(g["chunk"], g["subs"]) + 1, f"gen {cid} {DT_IDS[dtype]} rows{rows}")
    assert float(dwg[g["gx"] * g["subs"]:].abs().max() if g["gx"] * g["subs"] < rows else 0.0) == 0.0
    assert torch.equal(dug, dug2) and torch.equal(dwg, dwg2), "two calls differ"
    assert _kept(dict(dv, x=full), keep), "an operand changed"


@pytest.mark.parametrize("variant", ["add", "noadd", "ld"])
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("cid", list(R.TC_CASES))
def test_dx(cid, dtype, variant):
    """ly_rf_bwd_dx (the generic gather, the stride-2 parity gather, the LDS-tiled kernel; addend forms 0 / 1 / 2): with the addend, with
    addnc = NULL, and with lddx > C into a sentinel-filled allocation whose other columns keep their bits; two calls, same bits"""
    capi, lib, p, st = _capi()
    n, h, w, c, k, s = R.TC_CASES[cid]
    dev = _dev()
    x = R.tc_inputs(cid, dtype)
    dv = _to(x, ("dug", "wg", "addnc"), dev)
    keep = {q: v.clone() for q, v in dv.items()}
    add = variant != "noadd"
    extra = 1 if variant == "ld" else 0
    outs = []
    for _ in range(2):
        full, view, lddx = _place(torch.empty(n * h * w, c, dtype=dtype), extra, dev, fill=False)
        capi.check(lib.ly_rf_bwd_dx(n, h, w, c, k, s, p(dv["dug"]), p(dv["wg"]), p(view), lddx, p(dv["addnc"]) if add else p(None), x["add_scale"],
                                    capi.dtype_code(dtype), st), "ly_rf_bwd_dx")
        outs.append((full, view))
    torch.cuda.synchronize()
    R.judge_dx(outs[0][1].reshape(n, h, w, c), x, f"dx {cid} {DT_IDS[dtype]} {variant}", addend=add)
    assert torch.equal(outs[0][0], outs[1][0]), "two calls differ"
    assert bool((_outside(outs[0][0], c, extra, R.vw_of(dtype)) == SENTINEL).all()), "a column outside [0, C) changed"
    assert _kept(dv, keep), "an operand changed"


# ---------------------------------------------------------------- ly_rf3s_bwd --------------------------------------------------------------
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("cid", list(R.RF3S_CASES))
def test_rf3s(cid, dtype):
    """ly_rf3s_bwd pass 0 (cd, d_rfa, gmax plain stores: two calls, same bits; d_ca in double accumulators) and pass 1 (dv over dcd, the striped
    double sums folded with bnact_ref.fold), each on the builder's own operands"""
    capi, lib, p, st = _capi()
    cf, cb, ho, wo, n = R.RF3S_CASES[cid]
    c = R.c_of((cf, cb), dtype)
    dev = _dev()
    x = R.stage_inputs("rf3s", n, ho, wo, c, 3, dtype)
    R.assert_premises(R.d(x["ug"]), x["aeff"], R.d(x["bg"]), cid)
    dv = _to(x, R.RELU_KEYS + ("gmax",), dev)
    keep = {q: v.clone() for q, v in dv.items()}
    code = capi.dtype_code(dtype)
    ch = R.attn_chains("rf3s", n, ho, wo, c, 3, dtype)
    what = f"rf3s {cid} {DT_IDS[dtype]}"
    outs = []
    for _ in range(2):
        cd, d_rfa, gmax = torch.full_like(dv["ug"], SENTINEL), torch.full_like(dv["rfa"], SENTINEL), torch.full_like(dv["rfa"], SENTINEL)
        d_ca = torch.zeros(n, c, dtype=torch.float64, device=dev)
        P = capi.LyRf1BwdParams(n, ho * wo, c, p(dv["ug"]), c, p(dv["dcd"]), None, p(dv["ag"]), p(dv["bg"]), p(dv["ca"]), p(dv["rfa"]), p(cd), p(d_rfa), p(gmax),
                                p(d_ca), p(gmax), None, None, None, None, None, None, 0.0, None, c, None, code)
        capi.check(lib.ly_rf3s_bwd(ctypes.byref(P), ho, wo, 0, st), "ly_rf3s_bwd 0")
        outs.append(dict(cd=cd, d_rfa=d_rfa, gmax=gmax, d_ca=d_ca))
    torch.cuda.synchronize()
    R.judge_attn(outs[0], x, ch, what + " pass 0")
    assert all(torch.equal(outs[0][q], outs[1][q]) for q in ("cd", "d_rfa", "gmax")), "two calls differ"
    assert _kept(dv, keep), "an operand changed"
    sums = torch.zeros(capi.STATS_STRIPES, 2 * 9 * c, dtype=torch.float64, device=dev)
    P = capi.LyRf1BwdParams(n, ho * wo, c, p(dv["ug"]), c, p(dv["dcd"]), None, p(dv["ag"]), p(dv["bg"]), p(dv["ca"]), p(dv["rfa"]), None, None, None,
                            None, p(dv["gmax"]), p(dv["d_mm"]), p(sums), None, None, None, None, 0.0, None, c, None, code)
    capi.check(lib.ly_rf3s_bwd(ctypes.byref(P), ho, wo, 1, st), "ly_rf3s_bwd 1")
    torch.cuda.synchronize()
    s1, s2 = R.fold(sums)
    R.judge_relu(dict(dv=dv["dcd"], s1=s1.view(9, c), s2=s2.view(9, c)), x, ch[2], what + " pass 1")
    for m, t in R.allneg_positions(n * ho * wo, 9):
        assert float(dv["dcd"][m, t].float().abs().max()) == 0.0
    del keep["dcd"]
    assert _kept(dv, keep), "an operand changed"


# ---------------------------------------------------------------- ly_rf1_bwd ---------------------------------------------------------------
RF1_IN = R.RF1_KEYS + ("d_mm", "gmax", "alpha", "kappa", "lam", "dgap")


def _rf1(x, dtype, f64, dev, extra=0, dgap=True):
    """the three passes of ly_rf1_bwd on one case, each on the builder's own operands -> (results of pass 0, 1, 2; the placed x / dx blocks)"""
    capi, lib, p, st = _capi()
    n, hw, c = x["n"], x["hw"], x["x"].shape[-1]
    dv = _to(x, RF1_IN, dev)
    xfull, xv, ldx = _place(x["x"], extra, dev)
    dxfull, dxv, lddx = _place(torch.empty(n * hw, c, dtype=dtype), extra, dev, fill=False)
    cd, d_rfa, gmax = torch.full((n * hw, c), SENTINEL, dtype=dtype, device=dev), torch.full((n * hw,), SENTINEL, device=dev), torch.full((n * hw,), SENTINEL, device=dev)
    d_ca = torch.zeros(n, c, dtype=torch.float64, device=dev)
    sums = torch.zeros(capi.STATS_STRIPES, 2 * c, dtype=torch.float64, device=dev)
    dgw = torch.full((c,), 0.0 if f64 else 0.5, dtype=torch.float64 if f64 else torch.float32, device=dev)
    P = capi.LyRf1BwdParams(n, hw, c, p(xv), ldx, p(dv["dcd"]), p(dv["gw"]), p(dv["ag"]), p(dv["bg"]), p(dv["ca"]), p(dv["rfa"]), p(cd), p(d_rfa), p(gmax), p(d_ca),
                            p(dv["gmax"]), p(dv["d_mm"]), p(sums), p(dv["alpha"]), p(dv["kappa"]), p(dv["lam"]), p(dv["dgap"]) if dgap else None, x["scale"],
                            p(dxv), lddx, p(dgw), capi.dtype_code(dtype), int(f64))
    for ps in (0, 1, 2):
        capi.check(lib.ly_rf1_bwd(ctypes.byref(P), ps, st), f"ly_rf1_bwd {ps}")
    torch.cuda.synchronize()
    s1, s2 = R.fold(sums)
    return dict(cd=cd, d_rfa=d_rfa, gmax=gmax, d_ca=d_ca), dict(s1=s1, s2=s2), dict(dx=dxv, dgw=dgw), (xfull, dxfull), dv


@pytest.mark.parametrize("f64", F64)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("cid", list(R.RF1_CASES))
def test_rf1(cid, dtype, f64):
    """ly_rf1_bwd passes 0 / 1 / 2 (G recomputed from x in each): cd, d_rfa, gmax, dx plain stores (two runs, same bits), d_ca and the striped
    sums in doubles, dgw ADDED into a prefilled fp32 target / a zeroed float64 scratch"""
    cf, cb, hw, n = R.RF1_CASES[cid]
    dev = _dev()
    x = R.rf1_inputs(n, hw, R.c_of((cf, cb), dtype), dtype)
    R.assert_premises(R.d(x["x"]), x["aeff"], R.d(x["bg"]), cid)
    keep = _to(x, RF1_IN, dev)
    a, b, c_, (xfull, _), dv = _rf1(x, dtype, f64, dev)
    a2, _, c2, _, _ = _rf1(x, dtype, f64, dev)
    what = f"rf1 {cid} {DT_IDS[dtype]} {'f64' if f64 else 'f32'}"
    R.judge_rf1_a(a, x, what + " pass 0")
    R.judge_rf1_b(b, x, what + " pass 1")
    R.judge_rf1_c(c_, x, what + " pass 2", f64, prefill=0.0 if f64 else 0.5)
    assert all(torch.equal(a[q], a2[q]) for q in ("cd", "d_rfa", "gmax")) and torch.equal(c_["dx"], c2["dx"]), "two runs differ"
    for m, _ in R.allneg_positions(n * hw, 1):
        assert float(a["gmax"][m]) == 0.0 and float(a["d_rfa"][m]) == 0.0
    assert _kept(dv, keep) and torch.equal(xfull.cpu(), x["x"]), "an operand changed"


@pytest.mark.parametrize("dtype", BOTH)
def test_rf1_ld_and_no_dgap(dtype):
    """x and dx as channel slices of wider sentinel allocations (ldx > C, lddx > C) whose other columns keep their bits; dgap = NULL"""
    cid = "c24-24-hw400-n3"
    cf, cb, hw, n = R.RF1_CASES[cid]
    c = R.c_of((cf, cb), dtype)
    dev = _dev()
    x = R.rf1_inputs(n, hw, c, dtype)
    a, b, c_, (xfull, dxfull), _ = _rf1(x, dtype, False, dev, extra=1)
    what = f"rf1 {cid} {DT_IDS[dtype]} ld"
    R.judge_rf1_a(a, x, what + " pass 0")
    R.judge_rf1_b(b, x, what + " pass 1")
    R.judge_rf1_c(c_, x, what + " pass 2", False, prefill=0.5)
    vw = R.vw_of(dtype)
    assert bool((_outside(dxfull, c, 1, vw) == SENTINEL).all()) and bool((_outside(xfull, c, 1, vw) == SENTINEL).all())
    assert torch.equal(xfull[:, vw:vw + c].cpu(), x["x"])
    _, _, c_, _, _ = _rf1(x, dtype, True, dev, dgap=False)
    R.judge_rf1_c(c_, x, what + " no dgap", True, dgap=False)


# ---------------------------------------------------------------- ly_se_bwd ----------------------------------------------------------------
@pytest.mark.parametrize("f64", F64)
@pytest.mark.parametrize("cid", list(R.SE_CASES))
def test_se_bwd(cid, f64):
    """ops.se_bwd: dgap written (two calls, same bits), dWa / dWb ADDED into targets prefilled with 0.5; d_ca fp32 or the float64 accumulators of
    the attention passes; clearly-off hidden units, saturated ca"""
    from lead_yolo_amd import ops
    n, c, r, slices = R.SE_CASES[cid]
    dev = _dev()
    x = R.se_inputs(cid)
    assert not bool(R.se_margin_short(R.d(x["part"]), R.d(x["wa"]), x["hw"]).any())
    dv = _to(x, R.SE_KEYS, dev)
    if f64:
        dv["d_ca"] = dv["d_ca"].double()
    keep = {q: v.clone() for q, v in dv.items()}
    outs = []
    for _ in range(2):
        dwa, dwb = torch.full((r, c), 0.5, device=dev), torch.full((c, r), 0.5, device=dev)
        dgap = ops.se_bwd(dv["part"], n, x["hw"], c, dv["wa"], dv["wb"], r, dv["ca"], dv["d_ca"], dwa, dwb)
        outs.append(dict(dgap=dgap, dWa=dwa, dWb=dwb))
    torch.cuda.synchronize()
    assert tuple(outs[0]["dgap"].shape) == (n, c)
    R.judge_se(outs[0], x, f"se_bwd {cid} {'f64' if f64 else 'f32'}", prefill=0.5)
    assert all(torch.equal(outs[0][q], outs[1][q]) for q in outs[0]), "two calls differ"
    assert _kept(dv, keep), "an operand changed"


# ---------------------------------------------------------------- refusals -----------------------------------------------------------------
def test_refusals():
    """argument checks that return before any launch; every output keeps its sentinel"""
    from lead_yolo_amd import ops
    capi, lib, p, st = _capi()
    dev = _dev()
    n, h, w = 1, 4, 4
    z = lambda *s: torch.zeros(*s, device=dev)
    sent = lambda *s, dtype=torch.float32: torch.full(s, SENTINEL, dtype=dtype, device=dev)

    def refused(rc, what):
        with pytest.raises(capi.HipLibraryError):
            capi.check(rc, what)

    for c, k in ((7, 3), (8, 2)):                                   # odd C; k = 2
        kk, mo = 9, n * h * w
        e, mp = z(mo, kk, 8), z(n, 3 * h, 3 * w)
        outs = [sent(mo, kk, 8), sent(n, 3 * h, 3 * w), sent(n, 3 * h, 3 * w), sent(n, 8), sent(2 * kk * 8), sent(4, 8 * kk, kk), sent(n * h * w, 8)]
        cd, d_rfa, gmax, d_ca, sums, dwg, dxo = outs
        refused(lib.ly_rf_generate(p(z(n, h, w, 8)), 8, n, h, w, c, k, 1, p(z(8 * kk, kk)), p(cd), 0, st), "ly_rf_generate")
        refused(lib.ly_rf_bwd_attn(n, h, w, c, k, 1, p(e), p(e), p(z(kk, 8)), p(z(kk, 8)), p(z(n, 8)), p(mp), p(cd), p(d_rfa), p(gmax), p(d_ca), 0, st), "ly_rf_bwd_attn")
        refused(lib.ly_rf_bwd_relu(n, h, w, c, k, 1, p(e), p(cd), p(z(kk, 8)), p(z(kk, 8)), p(z(n, 8)), p(mp), p(mp), p(z(n, 3 * h, 3 * w, 2)), p(sums), 0, st),
                "ly_rf_bwd_relu")
        refused(lib.ly_rf_bwd_gen(p(z(n, h, w, 8)), 8, n, h, w, c, k, 1, p(e), p(cd), p(z(kk, 8)), p(z(kk, 8)), p(z(kk, 8)), p(dwg), 4, 0, st), "ly_rf_bwd_gen")
        refused(lib.ly_rf_bwd_dx(n, h, w, c, k, 1, p(e), p(z(8 * kk, kk)), p(dxo), 8, p(None), 1.0, 0, st), "ly_rf_bwd_dx")
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in outs)
    # part_rows = 3
    c, kk, mo = 8, 9, n * h * w
    dvv, dwg = sent(mo, kk, c), sent(4, c * kk, kk)
    refused(lib.ly_rf_bwd_gen(p(z(n, h, w, c)), c, n, h, w, c, 3, 1, p(z(mo, kk, c)), p(dvv), p(z(kk, c)), p(z(kk, c)), p(z(kk, c)), p(dwg), 3, 0, st), "ly_rf_bwd_gen")
    # ly_rf1_bwd: C no multiple of the vector width, C above 64 vectors, a misaligned ldx; ly_rf3s_bwd: HW != Ho Wo, pass 2
    hw = 16
    for c, ldx, dt in ((6, 6, R.F32), (260, 260, R.F32), (12, 12, R.BF16), (8, 9, R.F32)):
        cd, d_rfa, gmax, dxo, dgw = sent(hw, c, dtype=dt), sent(hw), sent(hw), sent(hw, c, dtype=dt), sent(c)
        d_ca, sums = sent(1, c, dtype=torch.float64), sent(32, 2 * c, dtype=torch.float64)
        xx = torch.zeros(hw, ldx, dtype=dt, device=dev)
        v = z(c)
        P = capi.LyRf1BwdParams(1, hw, c, p(xx), ldx, p(torch.zeros(hw, c, dtype=dt, device=dev)), p(v), p(v), p(v), p(v), p(z(hw)), p(cd), p(d_rfa), p(gmax), p(d_ca),
                                p(z(hw)), p(z(hw, 2)), p(sums), p(v), p(v), p(v), None, 1.0, p(dxo), c, p(dgw), capi.dtype_code(dt), 0)
        for ps in (0, 1, 2):
            refused(lib.ly_rf1_bwd(ctypes.byref(P), ps, st), "ly_rf1_bwd")
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in (cd, d_rfa, gmax, dxo, dgw, d_ca, sums))
    c, ho, wo = 8, 3, 5
    e = z(ho * wo, 9, c)
    cd, d_rfa, gmax = sent(ho * wo, 9, c), sent(1, 3 * ho, 3 * wo), sent(1, 3 * ho, 3 * wo)
    d_ca, sums = sent(1, c, dtype=torch.float64), sent(32, 2 * 9 * c, dtype=torch.float64)
    for hw_, ps in ((ho * wo + 1, 0), (ho * wo + 1, 1), (ho * wo, 2)):
        P = capi.LyRf1BwdParams(1, hw_, c, p(e), c, p(cd), None, p(z(9, c)), p(z(9, c)), p(z(1, c)), p(z(1, 3 * ho, 3 * wo)), p(cd), p(d_rfa), p(gmax), p(d_ca),
                                p(z(1, 3 * ho, 3 * wo)), p(z(1, 3 * ho, 3 * wo, 2)), p(sums), None, None, None, None, 0.0, None, c, None, 0)
        refused(lib.ly_rf3s_bwd(ctypes.byref(P), ho, wo, ps, st), "ly_rf3s_bwd")
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (cd, d_rfa, gmax, d_ca, sums, dvv, dwg))
    # ly_se_bwd with C = 1028
    c, r = 1028, 4
    dwa, dwb = sent(r, c), sent(c, r)
    with pytest.raises(capi.HipLibraryError):
        ops.se_bwd(z(1, 1, c), 1, 64, c, z(r, c), z(c, r), r, z(1, c), z(1, c), dwa, dwb)
    torch.cuda.synchronize()
    assert bool((dwa == SENTINEL).all()) and bool((dwb == SENTINEL).all())
