"""The RFCBAMConv forward kernels, entry point by entry point against float64 (tests/rfcbam_fwd_ref.py: references, judges with conditioned
bounds, the lattice and the rounded input family with their beacons, case tables; tests/test_rfcbam_fwd_host.py shows on the CPU that those
judges reject subtly wrong results, that the lattice is exact and that every case id takes the kernel it names).  ly_rf3c_fwd, ly_rf3m_fwd,
ly_rfcbam3_fwd and the k = 1 contraction go through the thin ops wrappers exactly as modules.py / grad.py call them, everything else through
lead_yolo_amd.capi with sentinel-filled outputs.  Every operand is built by the test; the weights are packed by pack.rfcbam_gen_weights(_c),
pack.rf3m_stream and pack.frag_pack3 (tests/test_pack_host.py, tests/test_gpu_pack.py).  No judge compares one kernel with another, except the
two stated identities: ly_rfcbam_mid against ly_se_fwd's ca and ly_rfa_map's rfa, and a second call against the first (plain stores: the same
bits; the double accumulators of a statistics pass: the same bits on the lattice, where every addend is exact, and the same fp32 value of the
folded sums on the rounded family — the arrival order of the double atomics may move the 53rd bit of a stripe, csrc/ly_common.hpp).  No
float atomic stands behind any output here.  Every judge prints its worst ratio before it asserts; every input is asserted unchanged.

Measured on the MI355X: every lattice comparison (324 of them) has 0 unequal elements; worst |err| / bound over the rounded cases, fp32 / bf16
storage (CPU float32 evaluation of the same references, in units of 2^-24 M: v 4.15, mean 2.31, ca 1.74, rfa 4.64, u 12.9 -> K 17, 10, 7, 19, 52):
    ly_rf3c_stats     max 0.17 / 0.17   mean 0.048 / 0.051   part 0.12 / 0.006        ly_rf3m_stats   max 0.074   mean 0.036   part 0.013
    ly_rfcbam_stats   k = 3: max 0.13 / 0.11   mean 0.048 / 0.041   part 0.10 / 0     k = 1: max 0.058 / 0.058   mean 0.045 / 0.063   part 0.11 / 0.019
    ly_rf3c_fwd       out 0.017 / 0.66   s1 0.006 / 0.006   s2 0.17 / 0.18           ly_rf3m_fwd     out 0.63
    ly_rfcbam3_fwd    out 0.046 / 0.79   s1 0.003 / 0.007   s2 0.13 / 0.12           k = 1 contraction   out 0.10 / 0.83
    ly_colsum         part 0.11 / 0.052   ly_se_fwd ca 0.20 / 0.65   ly_rfcbam_mid ca 0.28, rfa 0.065   ly_rfa_map 0.081
    (the bf16 contractions sit at 0.6 .. 0.8 of the bound because the operand allowance of bf16 storage, 2^-9 sum |wc B| (contract_bound in tests/rfcbam_fwd_ref.py), is half an ulp of an operand at
    the TOP of its binade: the exact arithmetic — B rounded to bf16, an exact sum, one bf16 rounding of the result — reaches the same figures on the
    CPU; the rounded family therefore keeps its operands comparable in size, see "operand allowance" in tests/rfcbam_fwd_ref.py)
One defect was found and fixed in csrc/: ly_rfcbam_stats (k = 3) with the fused pooling partials at a stride above 2 summed inputs its staged
tile does not hold (the rows and columns s (TH - 1) + 3 .. s TH of a tile: LDS of the neighbouring buffers, no fault, wrong partials).  No
caller reaches it (ops.rfcbam_stats takes the partials with ly_colsum for k = 3); the entry now refuses it before any launch
(test_refusals), and the statistics map at stride 3 stays covered by test_stats3[c48-s3-2x2-*].

branch of the kernels                                                    ->  case id (tables of tests/rfcbam_fwd_ref.py) or test
  ly_rf3c_stats (fp32, bf16; folded, raw; lattice, rounded)                  test_rf3c_stats[RC_SHAPES x ...]
    one chunk, a 1x1 output, the small tile 1x2                              c32-s1-1x1-map-tile1x2
    ops.pick_tile_c's tile, one tile per image, two images                   c32-s1-pick-one-tile
    a map that is no multiple of the tile in either direction                c32-s1-ragged-4x6
    the prefetched second chunk; odd H and W at stride 2                     c64-s2-odd-7x9-pick
    the 4x16 / 8x8 tiles RC_MAXPOS is sized for; three images, several       c64-s2-4x16-maxpos, c96-s2-3img-8x8-maxpos
      tiles each; C = 96: the mean with a non-dyadic 1 / C
    odd map at stride 1, tile 2x4, three chunks                              c96-s1-odd-5x7-tile2x4
    part == NULL; x with ldx > C inside a sentinel allocation                test_rf3c_stats[*-nopart], [*-ldx]
  ly_rf3c_fwd (ops.rf3c_fwd)                                                 test_rf3c_fwd[RC_FWD x ...]
    N = 64: MT 1; N = 128: MT 2, four waves; N = 256: eight waves (bf16),    n64-*, n128-*, n256-*
      two channel groups (fp32)
    N = 72: the last 16-channel tile half empty, scalar stores; N = 80: a    n72-ragged-channel-tile-raw-relu, n80-partial-block-folded-linear
      block whose second wave pair has no tile
    stats with out (the pre-BN value stored), stats with out == NULL,        *-stats-out*, *-stats-only, *-linear
      linear
    ldx > C and ldo > N inside sentinel allocations                          test_rf3c_fwd[n64-mt1-folded-relu-ldx], [n128-mt2-folded-relu-s2-odd-ldo]
  ly_rf3m_stats / ly_rf3m_fwd (bf16)                                         test_rf3m_stats, test_rf3m_fwd[RM_CASES x ...]
    25 tiles: the last block partial; MT 2                                   c32-s1-n64-mt2-25-tiles-partial-last-block
    the 4x8 tile at stride 2 (153 positions); 12 tiles of three images:      c64-s2-n128-mt4-4x8-maxpos-3img-straddle
      one block holds tiles of two images; MT 4
    ops.pick_tile_m's tile, odd map, 6 tiles: a single partial block         c32-s2-n128-mt4-odd-pick-6-tiles-one-partial-block
    a 1x1 map, two images                                                    c64-s1-n64-mt2-pick-1x1-map
    ldx > C, ldo > N                                                         [c64-s2-*-ldx], [c32-s1-*-ldo]
  ly_rfcbam_stats k = 3 (lane = pixel)                                       test_stats3[ST3_CASES x ...]
    C = 16 padded to 32; C = 48; stride 1, 2, 3; ops.pick_tile and 2x2       c16-s1-pick, c48-s2-odd-2x2, c48-s3-2x2, c16-s2-pick-3img
    the partials, one row per tile in tile order (stride 1, 2)               every case but c48-s3-2x2
  ly_rfcbam3_fwd (ops.rfcbam3)                                               test_rfcbam3_fwd[RF3_CASES x ...]
    MT 1, 2, 4; N = 72; stats with out, stats only, linear                   c16-n64-*, c48-n128-*, c48-n72-*, c16-n256-*
    MT 4 with 64 blocks: weights from LDS; 320 blocks: the scalar-cache      c16-n256-mt4-lds-64-blocks, c16-n256-mt4-sw-320-blocks
      kernel
  ly_rfcbam_stats k = 1                                                      test_stats1[K1_CASES x ...]
    pre1v<T, 1 .. 4>; the plain pre1 kernel (bf16 C = 12: no multiple of     pre1v-*, pre1-plain-c260-c12, pre1-plain-c520-c768-limit
      the vector; C above 16 x 4 vectors, up to the limit of 768)
    HW no multiple of the slice count; HW < 64: one slice; ops' own count    pre1v-3-hw200-slices7-ragged, pre1v-2-hw37-one-slice, (slices None)
    without part: a small case, and 16500 pixels behind the 4096-block cap   stats1-small, stats1-block-cap-c4
  ly_colsum, ly_se_fwd, ly_rfcbam_mid, ly_rfa_map                            test_colsum_and_se_fwd[SE_CASES], test_rfa_map[MAP_CASES], test_mid
    x with ldx > C inside a sentinel allocation (ly_colsum, ly_se_fwd)       test_colsum_and_se_fwd[n3-c160-r10-nq40-ldx-*]
    WK no multiple of 4 (the scalar store tail), WK < 4, HK = 1              tail-wk-7, wk-3-under-a-vector, hk-1
  the k = 1 contraction (ops.gemm, PRO_AFFINE_RELU_CA, rowscale)             test_gemm_k1[GEMM_CASES x ...]; lda0 > K, ldo > N: [*-ldx], [*-ldo]
  refusals before any launch                                                 test_refusals
"""
import pytest
import torch

from tests import rfcbam_fwd_ref as R

pytestmark = pytest.mark.gpu

DT_IDS = {R.F32: "f32", R.BF16: "bf16"}
BOTH = [pytest.param(R.F32, id="f32"), pytest.param(R.BF16, id="bf16")]
FAM = [pytest.param(f, id=f) for f in R.FAMILIES]
FORM = [pytest.param(False, id="folded"), pytest.param(True, id="raw")]
SENTINEL = 768.0                                 # (on the bf16 grid)
PAD = 8                                          # elements on either side of a placed block: 16 bytes in bf16, 32 in fp32; ld stays a multiple of 8


@pytest.fixture(autouse=True)
def _no_sink_left_behind(monkeypatch):
    from lead_yolo_amd import ops
    monkeypatch.setattr(ops, "SINK", None)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a CUDA/ROCm device"
    return torch.device("cuda:0")


def _capi():
    from lead_yolo_amd import capi
    return capi, capi.lib(), capi.ptr, capi.stream_ptr()


def _place(t, wide, dev, fill=True):
    """t [..., C] as rows inside a [rows, C + 2 PAD] allocation filled with a sentinel (wide), the block PAD elements in -> (full, view, ld)"""
    c = t.shape[-1]
    rows = t.reshape(-1, c)
    ld, off = (c + 2 * PAD, PAD) if wide else (c, 0)
    full = torch.full((rows.shape[0], ld), SENTINEL, dtype=t.dtype, device=dev)
    if fill:
        full[:, off:off + c] = rows.to(dev)
    return full, full[:, off:off + c], ld


def _outside_ok(full, c, wide):
    return (not wide) or bool((torch.cat((full[:, :PAD], full[:, PAD + c:]), 1) == SENTINEL).all())


def _sent(*shape, dtype=torch.float32, dev=None):
    return torch.full(shape, SENTINEL, dtype=dtype, device=dev)


def _gen_args(x, dev):
    """generate.0.weight [C KK, 1, k, k], the BatchNorm scale and shift [C KK] on the device: the arguments of the pack functions"""
    p, c, k = x["p"], x["c"], x["k"]
    return p["w"].reshape(c * k * k, 1, k, k).to(dev), p["a"].reshape(-1).to(dev), p["b"].reshape(-1).to(dev)


def _same_stats(a, b, family):
    if family == "lattice":
        return torch.equal(a, b)
    return all(torch.equal(s.float(), t.float()) for s, t in zip(R.fold(a), R.fold(b)))


def _with_ld(table, ld_cases):
    return [pytest.param(cid, "dense", id=cid) for cid in table] + [pytest.param(cid, ld, id=f"{cid}-{ld}") for ld, cid in ld_cases.items()]


# ---------------------------------------------------------------- ly_rf3c_stats -----------------------------------------------------------
RC_STATS_VARIANTS = _with_ld(R.RC_SHAPES, {"ldx": "c64-s2-odd-7x9-pick", "nopart": "c32-s1-ragged-4x6"})


@pytest.mark.parametrize("family", FAM)
@pytest.mark.parametrize("raw", FORM)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("cid,variant", RC_STATS_VARIANTS)
def test_rf3c_stats(cid, variant, dtype, raw, family):
    """ly_rf3c_stats: the [max, mean] map elementwise, the pooling partials tile by tile and folded; part == NULL on one case; two calls, same bits"""
    from lead_yolo_amd import pack
    capi, lib, p, st = _capi()
    dev = _dev()
    x, q = R.case_inputs("rc_stats", cid, dtype, family)
    n, h, w, c, s, th, tw, ho, wo = (q[key] for key in ("n", "h", "w", "c", "s", "th", "tw", "ho", "wo"))
    wq = pack.rfcbam_gen_weights_c(*_gen_args(x, dev), raw=raw)
    keep_w = wq.clone()
    full, xv, ldx = _place(x["x"], variant == "ldx", dev)
    keep = full.clone()
    tiles = R._cdiv(ho, th) * R._cdiv(wo, tw)
    outs = []
    for _ in range(2):
        mm, part = _sent(n, 3 * ho, 3 * wo, 2, dev=dev), _sent(n, tiles, c, dev=dev)
        capi.check(lib.ly_rf3c_stats(p(xv), ldx, n, h, w, c, s, p(wq), int(raw), th, tw, p(mm), p(None if variant == "nopart" else part), tiles,
                                     capi.dtype_code(dtype), st), "ly_rf3c_stats")
        outs.append((mm, part))
    torch.cuda.synchronize()
    what = f"rf3c_stats {cid} {variant} {DT_IDS[dtype]} {'raw' if raw else 'folded'} {family}"
    v, vm = R.want_for(x, "rf3c", raw)
    R.judge_mm(outs[0][0], x, v, vm, what)
    if variant == "nopart":
        assert bool((outs[0][1] == SENTINEL).all())
    else:
        xd = R.d(x["x"])
        R.judge_part(outs[0][1], x, R.part_tiles(xd, s, ho, wo, th, tw), R.part_tiles(xd.abs(), s, ho, wo, th, tw), R.tile_part_chain(s, th, tw), what)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two calls differ"
    assert torch.equal(full, keep) and torch.equal(wq, keep_w), "an input changed"


# ---------------------------------------------------------------- the three k = 3 contractions -------------------------------------------
def _run_fwd(route, x, q, variant, dev, raw=False):
    """one forward contraction on a route ("rf3c", "rf3m", "rf3") through its ops wrapper, twice -> (got of the first call, checks passed)"""
    from lead_yolo_amd import ops, pack
    capi = _capi()[0]
    n, h, w, c, s, th, tw, ho, wo, n_out, mode = (q[key] for key in ("n", "h", "w", "c", "s", "th", "tw", "ho", "wo", "n_out", "mode"))
    dtype, family = x["storage"], x["family"]
    planes = 1 if dtype == R.BF16 else 2
    gw, gs, gb = _gen_args(x, dev)
    wc = x["wc"].to(dev)
    extra = {}
    if route == "rf3c":
        extra["wq"] = pack.rfcbam_gen_weights_c(gw, gs, gb, raw=raw)
        # conv.0.weight as [N][C / 32 chunks][9 taps][32 channels]: k = chunk 288 + t 32 + channel
        wp = pack.frag_pack3(wc.view(n_out, c // 32, 32, 9).permute(0, 1, 3, 2).reshape(n_out, 9 * c).contiguous(), planes=planes)
    elif route == "rf3m":
        wp = pack.rf3m_stream(gw, gs, gb, wc.view(n_out, c, 3, 3), 4 if n_out % 128 == 0 else 2)
    else:
        extra["wg"] = pack.rfcbam_gen_weights(gw, gs, gb, 16, True)
        # conv.0.weight as [N][C / 16 chunks][10 tap slots (9 real)][16 channels]: k = chunk 160 + t 16 + channel
        m = torch.zeros(n_out, c // 16, 10, 16, device=dev)
        m[:, :, :9] = wc.view(n_out, c // 16, 16, 9).permute(0, 1, 3, 2)
        wp = pack.frag_pack3(m.reshape(n_out, (c // 16) * 160), planes=planes)
    ins = dict(ca=x["ca"].to(dev), rfa=x["rfa"].to(dev), es=x["es"].to(dev), esh=x["esh"].to(dev), wp=wp, **extra)
    full, xv, ldx = _place(x["x"], variant == "ldx", dev)
    ins["x"] = full
    keep = {key: val.clone() for key, val in ins.items()}
    fn = dict(rf3c=ops.rf3c_fwd, rf3m=ops.rf3m_fwd, rf3=ops.rfcbam3)[route]
    runs = []
    for _ in range(2):
        ofull, ov, ldo = _place(torch.empty(n * ho * wo, n_out, dtype=dtype), variant == "ldo", dev, fill=False)
        stats = torch.zeros(capi.STATS_STRIPES, 2 * n_out, dtype=torch.float64, device=dev) if mode.startswith("stats") else None
        kw = dict(n=n, h=h, w=w, c=c, ho=ho, wo=wo, N=n_out, s=s, th=th, tw=tw, x=xv, ldx=ldx, ca=ins["ca"], rfa=ins["rfa"], wp=wp, e_scale=ins["es"],
                  e_shift=ins["esh"], out=None if mode == "stats-only" else ov, ldo=ldo)
        if route == "rf3c":
            kw.update(wq=extra["wq"], raw=raw)
        if route == "rf3":
            kw.update(wg=extra["wg"])
        if route != "rf3m":
            kw.update(stats=stats, linear=mode == "linear")
        fn(**kw)
        runs.append((ofull, ov, stats))
    torch.cuda.synchronize()
    (of0, ov0, st0), (of1, _, st1) = runs
    assert torch.equal(of0, of1) and (st0 is None or _same_stats(st0, st1, family)), "two calls differ"
    if mode == "stats-only":
        assert bool((of0 == SENTINEL).all()), "out == NULL and something was stored"
    assert _outside_ok(of0, n_out, variant == "ldo"), "a column outside [0, N) changed"
    assert all(torch.equal(ins[key], keep[key]) for key in ins), "an input changed"
    return dict(out=None if mode == "stats-only" else ov0, stats=st0)


@pytest.mark.parametrize("family", FAM)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("cid,variant", _with_ld(R.RC_FWD, R.RC_LD))
def test_rf3c_fwd(cid, variant, dtype, family):
    """ly_rf3c_fwd through ops.rf3c_fwd: out elementwise (the pre-BN value in a statistics pass), the striped double sums folded in float64"""
    dev = _dev()
    x, q = R.case_inputs("rc_fwd", cid, dtype, family)
    got = _run_fwd("rf3c", x, q, variant, dev, raw=q["raw"])
    v, vm = R.want_for(x, "rf3c", q["raw"])
    R.judge_out(got, x, v, vm, q["mode"], f"rf3c_fwd {cid} {variant} {DT_IDS[dtype]} {family}")


RM_LD = {"ldx": "c64-s2-n128-mt4-4x8-maxpos-3img-straddle", "ldo": "c32-s1-n64-mt2-25-tiles-partial-last-block"}


@pytest.mark.parametrize("family", FAM)
@pytest.mark.parametrize("cid,variant", _with_ld(R.RM_CASES, RM_LD))
def test_rf3m_fwd(cid, variant, family):
    """ly_rf3m_fwd through ops.rf3m_fwd (bf16): the generate weights of the reference are the stream's bf16 values"""
    dev = _dev()
    x, q = R.case_inputs("rm", cid, R.BF16, family)
    got = _run_fwd("rf3m", x, q, variant, dev)
    v, vm = R.want_for(x, "rf3m", False)
    R.judge_out(got, x, v, vm, "relu", f"rf3m_fwd {cid} {variant} {family}")


@pytest.mark.parametrize("family", FAM)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("cid,variant", _with_ld(R.RF3_CASES, R.RF3_LD))
def test_rfcbam3_fwd(cid, variant, dtype, family):
    """ly_rfcbam3_fwd through ops.rfcbam3: the lane = pixel contraction, MT 1 / 2 / 4, weights from LDS and through the scalar cache"""
    dev = _dev()
    x, q = R.case_inputs("rf3", cid, dtype, family)
    got = _run_fwd("rf3", x, q, variant, dev)
    v, vm = R.want_for(x, "rf3c", False)
    R.judge_out(got, x, v, vm, q["mode"], f"rfcbam3_fwd {cid} {variant} {DT_IDS[dtype]} {family}")


# ---------------------------------------------------------------- ly_rf3m_stats ---------------------------------------------------------------
@pytest.mark.parametrize("family", FAM)
@pytest.mark.parametrize("cid,variant", _with_ld(R.RM_CASES, {"ldx": RM_LD["ldx"], "nopart": "c32-s2-n128-mt4-odd-pick-6-tiles-one-partial-block"}))
def test_rf3m_stats(cid, variant, family):
    """ly_rf3m_stats (bf16): map and partials as for ly_rf3c_stats, the generate on bf16 operands with fp32 accumulation"""
    from lead_yolo_amd import pack
    capi, lib, p, st = _capi()
    dev = _dev()
    x, q = R.case_inputs("rm", cid, R.BF16, family)
    n, h, w, c, s, th, tw, ho, wo = (q[key] for key in ("n", "h", "w", "c", "s", "th", "tw", "ho", "wo"))
    wst = pack.rf3m_stream(*_gen_args(x, dev), pool_stride=s)
    keep_w = wst.clone()
    full, xv, ldx = _place(x["x"], variant == "ldx", dev)
    keep = full.clone()
    tiles = R._cdiv(ho, th) * R._cdiv(wo, tw)
    outs = []
    for _ in range(2):
        mm, part = _sent(n, 3 * ho, 3 * wo, 2, dev=dev), _sent(n, tiles, c, dev=dev)
        capi.check(lib.ly_rf3m_stats(p(xv), ldx, n, h, w, c, s, p(wst), th, tw, p(mm), p(None if variant == "nopart" else part), tiles, st), "ly_rf3m_stats")
        outs.append((mm, part))
    torch.cuda.synchronize()
    what = f"rf3m_stats {cid} {variant} {family}"
    v, vm = R.want_for(x, "rf3m", False)
    R.judge_mm(outs[0][0], x, v, vm, what)
    if variant == "nopart":
        assert bool((outs[0][1] == SENTINEL).all())
    else:
        xd = R.d(x["x"])
        R.judge_part(outs[0][1], x, R.part_tiles(xd, s, ho, wo, th, tw), R.part_tiles(xd.abs(), s, ho, wo, th, tw), R.tile_part_chain(s, th, tw), what)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two calls differ"
    assert torch.equal(full, keep) and torch.equal(wst, keep_w), "an input changed"


# ---------------------------------------------------------------- ly_rfcbam_stats, k = 3 and k = 1 ---------------------------------------------
@pytest.mark.parametrize("family", FAM)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("cid,variant", _with_ld(R.ST3_CASES, {"ldx": "c48-s2-odd-2x2"}))
def test_stats3(cid, variant, dtype, family):
    """ly_rfcbam_stats, k = 3 (lane = pixel; weights padded to 32 channels): the map at stride 1, 2, 3; the partials one row per tile at stride 1, 2"""
    from lead_yolo_amd import pack
    capi, lib, p, st = _capi()
    dev = _dev()
    x, q = R.case_inputs("st3", cid, dtype, family)
    n, h, w, c, s, th, tw, ho, wo = (q[key] for key in ("n", "h", "w", "c", "s", "th", "tw", "ho", "wo"))
    wg = pack.rfcbam_gen_weights(*_gen_args(x, dev), 32, False)
    keep_w = wg.clone()
    full, xv, ldx = _place(x["x"], variant == "ldx", dev)
    keep = full.clone()
    tiles = R._cdiv(ho, th) * R._cdiv(wo, tw)
    with_part = s <= 2
    outs = []
    for _ in range(2):
        mm, part = _sent(n, 3 * ho, 3 * wo, 2, dev=dev), _sent(n, tiles, c, dev=dev)
        capi.check(lib.ly_rfcbam_stats(p(xv), ldx, n, h, w, c, 3, s, p(wg), p(None), p(None), th, tw, p(mm), p(part if with_part else None), tiles if with_part else 0,
                                       capi.dtype_code(dtype), st), "ly_rfcbam_stats")
        outs.append((mm, part))
    torch.cuda.synchronize()
    what = f"stats3 {cid} {variant} {DT_IDS[dtype]} {family}"
    v, vm = R.want_for(x, "rf3c", False)
    R.judge_mm(outs[0][0], x, v, vm, what)
    if with_part:
        xd = R.d(x["x"])
        R.judge_part(outs[0][1], x, R.part_tiles(xd, s, ho, wo, th, tw), R.part_tiles(xd.abs(), s, ho, wo, th, tw), R.tile_part_chain(s, th, tw), what)
    else:
        assert bool((outs[0][1] == SENTINEL).all())
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two calls differ"
    assert torch.equal(full, keep) and torch.equal(wg, keep_w), "an input changed"


@pytest.mark.parametrize("family", FAM)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("cid,variant", _with_ld(R.K1_CASES, {"ldx": "pre1v-2-hw37-one-slice"}))
def test_stats1(cid, variant, dtype, family):
    """ly_rfcbam_stats, k = 1: pre1v<T, 1 .. 4> and pre1 with the pooling partials in the slicing ceil(HW / slices), stats1 without them"""
    capi, lib, p, st = _capi()
    dev = _dev()
    row = R.K1_CASES[cid]
    n, hw, c = row[0], row[1], R.k1_c(row, dtype)
    slices = 0 if row[4] == 0 else R.k1_slices(hw, row[4])
    x = R.k1_inputs(cid, dtype, family)
    a1, b1 = x["p"]["wf"].reshape(c).to(dev), x["p"]["b"].reshape(c).to(dev)
    full, xv, ldx = _place(x["x"], variant == "ldx", dev)
    keep = (full.clone(), a1.clone(), b1.clone())
    outs = []
    for _ in range(2):
        mm, part = _sent(n, hw, 1, 2, dev=dev), _sent(n, max(slices, 1), c, dev=dev)
        capi.check(lib.ly_rfcbam_stats(p(xv), ldx, n, 1, hw, c, 1, 1, p(None), p(a1), p(b1), 1, 64, p(mm), p(part if slices else None), slices, capi.dtype_code(dtype), st),
                   "ly_rfcbam_stats")
        outs.append((mm, part))
    torch.cuda.synchronize()
    what = f"stats1 {cid} {variant} {DT_IDS[dtype]} {family}"
    v, vm = R.want_for(x, "rf3c", False)
    R.judge_mm(outs[0][0], x, v, vm, what)
    if slices:
        xd = R.d(x["x"])
        R.judge_part(outs[0][1], x, R.part_slices(xd, slices), R.part_slices(xd.abs(), slices), R.part_chain(hw, c, slices), what)
    else:
        assert bool((outs[0][1] == SENTINEL).all())
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two calls differ"
    assert torch.equal(full, keep[0]) and torch.equal(a1, keep[1]) and torch.equal(b1, keep[2]), "an input changed"


# ---------------------------------------------------------------- the small steps ----------------------------------------------------------
@pytest.mark.parametrize("family", FAM)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("cid,variant", _with_ld(R.SE_CASES, {"ldx": "n3-c160-r10-nq40"}))
def test_colsum_and_se_fwd(cid, variant, dtype, family):
    """ly_colsum: the partials slice by slice and folded; ly_se_fwd: the same partials (bit for bit: its first half IS ly_colsum) and ca against
    float64 from x, the partials' own chain carried into the bound of the mean; x with ldx > C inside a sentinel allocation on one case"""
    capi, lib, p, st = _capi()
    dev = _dev()
    x = R.se_x_inputs(cid, dtype, family)
    n, c, r, slices, hw = x["n"], x["c"], x["r"], x["slices"], x["hw"]
    w = R.se_inputs_fwd(cid)
    wa, wb = w["wa"].to(dev), w["wb"].to(dev)
    full, xv, ldx = _place(x["x"], variant == "ldx", dev)
    keep = (full.clone(), wa.clone(), wb.clone())
    code = capi.dtype_code(dtype)
    outs = []
    for _ in range(2):
        part, part2, ca = _sent(n, slices, c, dev=dev), _sent(n, slices, c, dev=dev), _sent(n, c, dev=dev)
        capi.check(lib.ly_colsum(p(xv), ldx, n, hw, c, p(part), slices, code, st), "ly_colsum")
        capi.check(lib.ly_se_fwd(p(xv), ldx, n, hw, c, p(wa), p(wb), r, p(part2), slices, p(ca), code, st), "ly_se_fwd")
        outs.append((part, part2, ca))
    torch.cuda.synchronize()
    what = f"colsum / se_fwd {cid} {variant} {DT_IDS[dtype]} {family}"
    xd = R.d(x["x"])
    want = R.part_slices(xd, slices)
    chain = R.part_chain(hw, c, slices)
    R.judge_part(outs[0][0], x, want, R.part_slices(xd.abs(), slices), chain, what)
    assert torch.equal(outs[0][0], outs[0][1]), "ly_se_fwd's partials are not ly_colsum's"
    ch = R.se_chains(c, r, slices)
    ch["gap"] += chain
    a = (want, R.d(w["wa"]), R.d(w["wb"]), hw)
    R._bounded(outs[0][2], R.se_ca(*a)["ca"], R.se_ca_bound(*a, chains=ch)[1], what + " ca")
    assert all(torch.equal(s, t) for s, t in zip(outs[0], outs[1])), "two calls differ"
    assert torch.equal(full, keep[0]) and torch.equal(wa, keep[1]) and torch.equal(wb, keep[2]), "an input (or a sentinel column beside x) changed"
    assert _outside_ok(full, c, variant == "ldx")


@pytest.mark.parametrize("cid", list(R.MAP_CASES))
def test_rfa_map(cid):
    """ly_rfa_map: sigmoid of the zero-padded 3x3 conv on the [max, mean] map; the vector store, its scalar tail, WK < 4, HK = 1, saturated corners"""
    capi, lib, p, st = _capi()
    dev = _dev()
    x = R.map_inputs(cid)
    mm, w18 = x["mm"].to(dev), x["w18"].to(dev)
    keep = (mm.clone(), w18.clone())
    outs = []
    for _ in range(2):
        rfa = _sent(x["n"], x["hk"], x["wk"], dev=dev)
        capi.check(lib.ly_rfa_map(p(mm), x["n"], x["hk"], x["wk"], p(w18), p(rfa), st), "ly_rfa_map")
        outs.append(rfa)
    torch.cuda.synchronize()
    R.judge_rfa(outs[0], x, f"rfa_map {cid}")
    assert torch.equal(outs[0], outs[1]), "two calls differ"
    assert torch.equal(mm, keep[0]) and torch.equal(w18, keep[1]), "an input changed"


MID_MAPS = {"n1-c8-r1": "wk-3-under-a-vector", "n3-c160-r10-nq40": "tail-wk-7", "n8-c64-r4-one-trip": "hk-1", "n9-c256-r16-trip-plus-one": "halo-four-tiles-17x65",
            "n17-c1024-r64-two-trips-plus-one": "inside-one-tile-15x63"}


@pytest.mark.parametrize("cid", list(R.SE_CASES))
def test_mid(cid):
    """ly_rfcbam_mid on the builders' own partials and map (the map's shape from MAP_CASES, its image count the SE case's): ca and rfa against
    float64; rfa bit for bit ly_rfa_map's; ca bit for bit ly_se_fwd's — taken on an x of one pixel per slice in fp32 storage, whose ly_colsum
    partials ARE the builder's partials (asserted), with the pixel count both entries then divide by"""
    capi, lib, p, st = _capi()
    dev = _dev()
    x = R.se_inputs_fwd(cid)
    n, c, r, slices = x["n"], x["c"], x["r"], x["slices"]
    mcid = MID_MAPS[cid]
    m = R.map_inputs(mcid)
    g = R._gen("midmap", cid)
    hk, wk = m["hk"], m["wk"]
    m = dict(mm=torch.stack((R._rand(g, n, hk, wk) * 3, R._rand(g, n, hk, wk)), -1).float(), w18=m["w18"], n=n, hk=hk, wk=wk)
    dv = {key: val.to(dev) for key, val in dict(part=x["part"], wa=x["wa"], wb=x["wb"], mm=m["mm"], w18=m["w18"]).items()}
    keep = {key: val.clone() for key, val in dv.items()}

    def mid(hw):
        ca, rfa = _sent(n, c, dev=dev), _sent(n, hk, wk, dev=dev)
        capi.check(lib.ly_rfcbam_mid(p(dv["part"]), slices, c, hw, p(dv["wa"]), p(dv["wb"]), r, p(ca), n, p(dv["mm"]), hk, wk, p(dv["w18"]), p(rfa), st), "ly_rfcbam_mid")
        return ca, rfa

    outs = [mid(x["hw"]), mid(x["hw"])]
    ca_px, _ = mid(slices)
    rfa2, ca2, part2 = _sent(n, hk, wk, dev=dev), _sent(n, c, dev=dev), _sent(n, slices, c, dev=dev)
    capi.check(lib.ly_rfa_map(p(dv["mm"]), n, hk, wk, p(dv["w18"]), p(rfa2), st), "ly_rfa_map")
    capi.check(lib.ly_se_fwd(p(dv["part"]), c, n, slices, c, p(dv["wa"]), p(dv["wb"]), r, p(part2), slices, p(ca2), capi.dtype_code(R.F32), st), "ly_se_fwd")
    torch.cuda.synchronize()
    what = f"mid {cid} / {mcid}"
    R.judge_ca(outs[0][0], x, what)
    R.judge_rfa(outs[0][1], m, what)
    assert torch.equal(outs[0][1], rfa2), "ly_rfcbam_mid's rfa is not ly_rfa_map's"
    assert torch.equal(part2, dv["part"]), "one pixel per slice: the partials are x"
    assert torch.equal(ca_px, ca2), "ly_rfcbam_mid's ca is not ly_se_fwd's"
    assert all(torch.equal(s, t) for s, t in zip(outs[0], outs[1])), "two calls differ"
    assert all(torch.equal(dv[key], keep[key]) for key in dv), "an input changed"


# ---------------------------------------------------------------- the k = 1 contraction ---------------------------------------------------
@pytest.mark.parametrize("family", FAM)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("cid,variant", _with_ld(R.GEMM_CASES, {"ldx": "k160-n64", "ldo": "k32-n256"}))
def test_gemm_k1(cid, variant, dtype, family):
    """ops.gemm with pro = PRO_AFFINE_RELU_CA, p_ca and rowscale = rfa as RFCBAMConv.forward calls it: relu(a1 x + b1) ca[image] as the operand,
    rfa on the accumulator; two images, so ca changes inside a row block"""
    from lead_yolo_amd import ops, pack
    dev = _dev()
    x, q = R.case_inputs("gemm", cid, dtype, family)
    n, h, w, c, n_out = q["n"], q["h"], q["w"], q["c"], q["n_out"]
    m = n * h * w
    planes = 1 if dtype == R.BF16 else 2
    ins = dict(a1=x["p"]["wf"].reshape(c).to(dev), b1=x["p"]["b"].reshape(c).to(dev), ca=x["ca"].to(dev), rfa=x["rfa"].reshape(m).to(dev), es=x["es"].to(dev),
               esh=x["esh"].to(dev), wp=pack.frag_pack3(x["wc"].reshape(n_out, c).to(dev), planes=planes))
    full, xv, ldx = _place(x["x"], variant == "ldx", dev)
    ins["x"] = full
    keep = {key: val.clone() for key, val in ins.items()}
    runs = []
    for _ in range(2):
        ofull, ov, ldo = _place(torch.empty(m, n_out, dtype=dtype), variant == "ldo", dev, fill=False)
        ops.gemm(M=m, H=h, W=w, K=c, N=n_out, a0=xv, lda0=ldx, k0=c, wp=ins["wp"], out=ov, ldo=ldo, pro=ops.PRO_AFFINE_RELU_CA, p_scale=ins["a1"], p_shift=ins["b1"],
                 p_ca=ins["ca"], rowscale=ins["rfa"], e_scale=ins["es"], e_shift=ins["esh"], act=ops.ACT_RELU)
        runs.append((ofull, ov))
    torch.cuda.synchronize()
    v, vm = R.want_for(x, "rf3c", False)
    R.judge_out(dict(out=runs[0][1]), x, v, vm, "relu", f"gemm k1 {cid} {variant} {DT_IDS[dtype]} {family}", rowscale=True)
    assert torch.equal(runs[0][0], runs[1][0]), "two calls differ"
    assert _outside_ok(runs[0][0], n_out, variant == "ldo"), "a column outside [0, N) changed"
    assert all(torch.equal(ins[key], keep[key]) for key in ins), "an input changed"


# ---------------------------------------------------------------- refusals -----------------------------------------------------------------
def test_refusals():
    """argument checks that stand before any launch (read in csrc/: rc_check_tile, rm_check and the entries' own LY_CHECKs precede every
    dispatch): the call returns -1 and every output keeps its sentinel"""
    import ctypes
    capi, lib, p, st = _capi()
    dev = _dev()
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)
    n, h, w, ho, wo = 1, 8, 8, 8, 8
    mm, part, out = _sent(n, 3 * 64, 3 * 64, 2, dev=dev), _sent(n, 64, 64, dev=dev), _sent(64 * 64, 256, dev=dev)
    outb, stats = _sent(64 * 64, 256, dtype=R.BF16, dev=dev), _sent(32, 512, dtype=torch.float64, dev=dev)
    wbuf, x32, x16 = z(1 << 16), z(n, 64, 64, 64), z(n, 64, 64, 64, dtype=R.BF16)
    ca, rfa, es = z(n, 64), z(n, 3 * 64, 3 * 64), z(256)

    def refused(rc, what):
        assert rc == -1, what
        with pytest.raises(capi.HipLibraryError):
            capi.check(rc, what)

    def params(c=32, s=1, th=8, tw=8, n_out=64, dtype=R.F32, ho_=None, stats_=None, linear=0, h_=h, w_=w):
        ho_ = ((h_ + 2 - 3) // s + 1) if ho_ is None else ho_
        return capi.LyRfcbam3Params(n, h_, w_, c, ho_, (w_ + 2 - 3) // s + 1, n_out, s, th, tw, p(x16 if dtype == R.BF16 else x32), c, p(wbuf), p(ca), p(rfa), p(wbuf), p(es), p(es),
                                    p(outb if dtype == R.BF16 else out), n_out, p(stats_), linear, capi.dtype_code(dtype))

    # C no multiple of 32 (lane = channel, matrix cores) / of 16 (lane = pixel)
    refused(lib.ly_rf3c_stats(p(x32), 48, n, h, w, 48, 1, p(wbuf), 0, 8, 8, p(mm), p(part), 1, 0, st), "rf3c_stats C = 48")
    refused(lib.ly_rf3c_fwd(ctypes.byref(params(c=48)), p(wbuf), 0, st), "rf3c_fwd C = 48")
    refused(lib.ly_rf3m_stats(p(x16), 48, n, h, w, 48, 1, p(wbuf), 4, 8, p(mm), p(part), 2, st), "rf3m_stats C = 48")
    refused(lib.ly_rf3m_fwd(ctypes.byref(params(c=48, th=4, dtype=R.BF16)), st), "rf3m_fwd C = 48")
    refused(lib.ly_rfcbam3_fwd(ctypes.byref(params(c=24)), st), "rfcbam3 C = 24")
    # an odd TW; a tile over the position limit: 2 x 32 at stride 2 reads 5 x 65 = 325 > 320, 2 x 16 reads 5 x 33 = 165 > 160
    refused(lib.ly_rf3c_stats(p(x32), 32, n, h, w, 32, 1, p(wbuf), 0, 8, 7, p(mm), p(part), 2, 0, st), "rf3c_stats TW = 7")
    refused(lib.ly_rf3c_fwd(ctypes.byref(params(tw=7)), p(wbuf), 0, st), "rf3c_fwd TW = 7")
    refused(lib.ly_rf3c_stats(p(x32), 32, n, 64, 64, 32, 2, p(wbuf), 0, 2, 32, p(mm), p(part), 16, 0, st), "rf3c_stats 325 positions")
    refused(lib.ly_rf3c_fwd(ctypes.byref(params(s=2, th=2, tw=32, h_=64, w_=64)), p(wbuf), 0, st), "rf3c_fwd 325 positions")
    refused(lib.ly_rf3m_stats(p(x16), 32, n, 64, 64, 32, 2, p(wbuf), 2, 16, p(mm), p(part), 32, st), "rf3m_stats 165 positions")
    refused(lib.ly_rf3m_fwd(ctypes.byref(params(s=2, th=2, tw=16, h_=64, w_=64, dtype=R.BF16)), st), "rf3m_fwd 165 positions")
    refused(lib.ly_rf3m_stats(p(x16), 32, n, h, w, 32, 1, p(wbuf), 5, 8, p(mm), p(part), 2, st), "rf3m_stats 40 pixels")
    # slices different from the tile count (one 8 x 8 tile / two 4 x 8 tiles here)
    refused(lib.ly_rf3c_stats(p(x32), 32, n, h, w, 32, 1, p(wbuf), 0, 8, 8, p(mm), p(part), 2, 0, st), "rf3c_stats slices")
    refused(lib.ly_rf3m_stats(p(x16), 32, n, h, w, 32, 1, p(wbuf), 4, 8, p(mm), p(part), 1, st), "rf3m_stats slices")
    refused(lib.ly_rfcbam_stats(p(x32), 32, n, h, w, 32, 3, 1, p(wbuf), p(None), p(None), 8, 8, p(mm), p(part), 2, 0, st), "rfcbam_stats slices")
    # the fused partials of the lane = pixel pass at stride 3: the staged tile does not hold what the tile owns
    refused(lib.ly_rfcbam_stats(p(x32), 32, n, 6, 6, 32, 3, 3, p(wbuf), p(None), p(None), 2, 2, p(mm), p(part), 1, 0, st), "rfcbam_stats stride 3 with part")
    # ly_rf3m_fwd: fp32 storage, a statistics pass, linear, N no multiple of 64
    refused(lib.ly_rf3m_fwd(ctypes.byref(params(th=4, dtype=R.F32)), st), "rf3m_fwd fp32")
    refused(lib.ly_rf3m_fwd(ctypes.byref(params(th=4, dtype=R.BF16, stats_=stats)), st), "rf3m_fwd stats")
    refused(lib.ly_rf3m_fwd(ctypes.byref(params(th=4, dtype=R.BF16, linear=1)), st), "rf3m_fwd linear")
    refused(lib.ly_rf3m_fwd(ctypes.byref(params(th=4, dtype=R.BF16, n_out=96)), st), "rf3m_fwd N = 96")
    # an inconsistent Ho
    refused(lib.ly_rf3c_fwd(ctypes.byref(params(ho_=7)), p(wbuf), 0, st), "rf3c_fwd Ho")
    refused(lib.ly_rf3m_fwd(ctypes.byref(params(th=4, dtype=R.BF16, ho_=7)), st), "rf3m_fwd Ho")
    refused(lib.ly_rfcbam3_fwd(ctypes.byref(params(ho_=7)), st), "rfcbam3 Ho")
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (mm, part, out, outb, stats))
