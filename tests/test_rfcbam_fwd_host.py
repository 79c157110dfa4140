"""Host side of the RFCBAMConv forward tests (tests/rfcbam_fwd_ref.py): the float64 references composed as RFCBAMConv.forward composes the
kernels against oracle.functional's module in float64, the lattice family's exactness (the float32 evaluation, with the bf16 operand rounding
applied, equals float64 bit for bit), the measured constants, the beacons' dominance, the judges against planted defects (the evidence that
tests/test_gpu_rfcbam_fwd.py would fail on a subtly wrong kernel — no broken kernel is ever built or run) and the kernel each case id claims,
read back through the describe twins.  Every mutant is computed in float64 and rounded as a kernel's result would be stored.  No GPU."""
import ctypes

import pytest
import torch

from tests import rfcbam_fwd_ref as R

BOTH = [pytest.param(R.F32, id="f32"), pytest.param(R.BF16, id="bf16")]
FAM = [pytest.param(f, id=f) for f in R.FAMILIES]
A, B, C_, D, E, F_ = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000       # 16-byte aligned made-up addresses (never dereferenced)


def _rejects(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


def _route(table):
    return "rf3m" if table == "rm" else "rf3c"


def _stored_out(o, x, mode):
    """a reference result as a kernel would leave it: out in the storage type, the sums as one stripe of doubles"""
    got = {}
    if mode != "stats-only":
        got["out"] = o["out"].to(x["storage"])
    if mode.startswith("stats"):
        got["stats"] = torch.cat((o["s1"], o["s2"])).view(1, -1)
    return got


# ---------------------------------------------------------------- the references against the module ------------------------------------------
@pytest.mark.parametrize("n,h,w,c,o,k,s", [(2, 5, 4, 8, 5, 1, 1), (1, 3, 7, 4, 6, 1, 1), (2, 6, 5, 4, 5, 3, 1), (1, 4, 7, 8, 3, 3, 1), (2, 7, 5, 4, 6, 3, 2),
                                           (1, 6, 8, 8, 4, 3, 2)], ids=["k1-a", "k1-b", "k3s1-a", "k3s1-b", "k3s2-odd", "k3s2-even"])
def test_references_compose_to_the_module(n, h, w, c, o, k, s):
    """stats -> mid -> contraction in float64, both forms of `generate`, reproduce oracle.functional.rfcbam (eval) to 1e-12; so do the
    intermediates ca, mm, rfa; the pooling partials fold to the image sum in either slicing"""
    from oracle import functional as OF
    g = torch.Generator().manual_seed(11)
    rn = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64)
    ru = lambda *sh: torch.rand(*sh, generator=g, dtype=torch.float64)
    kk, r = k * k, 3
    st = {"m.se.fc.0.weight": rn(r, c), "m.se.fc.2.weight": rn(c, r), "m.generate.0.weight": rn(c * kk, 1, k, k) * 0.5, "m.generate.1.weight": ru(c * kk) + 0.5,
          "m.generate.1.bias": rn(c * kk) * 0.3, "m.generate.1.running_mean": rn(c * kk) * 0.2, "m.generate.1.running_var": ru(c * kk) + 0.5,
          "m.get_weight.0.weight": rn(1, 2, 3, 3) * 0.5, "m.conv.0.weight": rn(o, c, k, k) * 0.3, "m.conv.0.bias": rn(o) * 0.1, "m.conv.1.weight": ru(o) + 0.5,
          "m.conv.1.bias": rn(o) * 0.3, "m.conv.1.running_mean": rn(o) * 0.2, "m.conv.1.running_var": ru(o) + 0.5}
    x = rn(n, h, w, c)
    want, mid = OF.rfcbam(st, "m.", x.permute(0, 3, 1, 2), k, s, training=False, return_intermediates=True)
    ho, wo = R.out_hw(h, w, k, s)
    a = (st["m.generate.1.weight"] / torch.sqrt(st["m.generate.1.running_var"] + OF.BN_EPS)).view(c, kk)
    b = st["m.generate.1.bias"].view(c, kk) - st["m.generate.1.running_mean"].view(c, kk) * a
    wg = st["m.generate.0.weight"].view(c, kk, kk)
    p = dict(w=wg, a=a, b=b, wf=wg * a.unsqueeze(-1))
    es = st["m.conv.1.weight"] / torch.sqrt(st["m.conv.1.running_var"] + OF.BN_EPS)
    esh = st["m.conv.1.bias"] - st["m.conv.1.running_mean"] * es + st["m.conv.0.bias"] * es
    part = R.part_tiles(x, s, ho, wo, 2, 2) if k == 3 else R.part_slices(x, 3)
    assert float((part.sum(1) - R.part_slices(x, 1)[:, 0]).abs().max()) <= 1e-12
    ca = R.se_ca(part, st["m.se.fc.0.weight"], st["m.se.fc.2.weight"], h * w)["ca"]
    assert float((ca - mid["ca"]).abs().max()) <= 1e-12
    for raw in (False, True):
        v = R.gen_v(x, p, k, s, raw)
        mm = R.mm_of(v, n, ho, wo, k)
        assert float((mm.permute(0, 3, 1, 2) - mid["mm"]).abs().max()) <= 1e-12
        rfa = R.getw_fwd(mm, st["m.get_weight.0.weight"].reshape(18))
        pre, _ = R.rfa_pre(mm, st["m.get_weight.0.weight"].reshape(18))
        assert float((rfa - mid["rfa"][:, 0]).abs().max()) <= 1e-12 and float((torch.sigmoid(pre) - rfa).abs().max()) <= 1e-15
        for rowscale in ((False, True) if k == 1 else (False,)):
            y = R.contract(torch.clamp(v, min=0.0), ca, rfa, st["m.conv.0.weight"].reshape(o, c, kk), es, esh, n, ho, wo, k, rowscale=rowscale)["out"]
            assert float((y.view(n, ho, wo, o).permute(0, 3, 1, 2) - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ---------------------------------------------------------------- measured constants ---------------------------------------------------------
def test_measured_k_holds():
    """every K of tests/rfcbam_fwd_ref.py is at least four times what the reference itself shows in float32 over every rounded case, and no more than twice that"""
    for key, val in R.measure_k().items():
        print(key, val)
        assert 4 * val <= R.K[key] <= 8 * val, (key, val)


# ---------------------------------------------------------------- the lattice is exact --------------------------------------------------------
def _all_cases():
    return [(t, cid) for t, rows in R.TABLES.items() for cid in rows]


@pytest.mark.parametrize("table,cid", _all_cases(), ids=[f"{t}:{c}" for t, c in _all_cases()])
def test_lattice_cases_are_exact(table, cid):
    """float32 evaluation of the references, with the bf16 rounding of the contraction's B operand and of ly_rf3m's generate weights applied,
    equals float64 bit for bit on every lattice case: v, the maximum, the channel SUM (the mean wherever 1 / C is dyadic), the pooling partials,
    B (at most 8 significant bits: one bf16 plane holds it, the lo plane is zero), the accumulator, u and s1"""
    for st in (R.F32, R.BF16):
        if table == "rm" and st == R.F32:
            continue
        x, q = R.case_inputs(table, cid, st, "lattice")
        n, k, s, ho, wo, c = q["n"], q["k"], q["s"], q["ho"], q["wo"], q["c"]
        pq = R.stored_params(x["p"], _route(table))
        assert all(torch.equal(pq[key], R.d(x["p"][key])) for key in pq), "the bf16 rounding of ly_rf3m's weights moves a lattice value"
        p32 = {key: val.float() for key, val in pq.items()}
        xd = R.d(x["x"])
        assert torch.equal(R.d(x["x"].float().to(st)), xd)
        for raw in ((False, True) if table.startswith("rc") else (False,)):
            v, v32 = R.gen_v(xd, pq, k, s, raw), R.gen_v(xd.float(), p32, k, s, raw)
            assert torch.equal(v32.double(), v) and float(v.max()) < 16 and torch.equal((v * 16).round(), v * 16), "v leaves the grid"
            g = torch.clamp(v, min=0.0)
            assert torch.equal(g.float().sum(-1).double(), g.sum(-1))
            mm = R.mm_of(v, n, ho, wo, k)
            if c & (c - 1) == 0:
                assert torch.equal((g.float().sum(-1) * torch.tensor(1.0 / c, dtype=torch.float32)).double(), g.sum(-1) / c)
            else:
                fl = (g.float().sum(-1) * torch.tensor(1.0 / c, dtype=torch.float32)).double()
                assert bool(((fl - g.sum(-1) / c).abs() <= R.ULP_MEAN * (g.sum(-1) / c)).all())
            assert torch.equal(mm.float().double()[..., 0], mm[..., 0])
            a = (R.d(x["ca"]), R.d(x["rfa"]), R.stored_wc(x["wc"], st), R.d(x["es"]), R.d(x["esh"]), n, ho, wo, k)
            assert torch.equal(a[2], R.d(x["wc"])) and torch.equal(R.d(x["wc"].bfloat16()), R.d(x["wc"])), "wc has a lo plane"
            for rs in ((False, True) if k == 1 else (False,)):
                o = R.contract(g, *a, rowscale=rs)
                assert torch.equal(R.d(o["B"].bfloat16()), o["B"]), "B does not fit one bf16 plane"
                a32 = tuple(t.float() if torch.is_tensor(t) else t for t in a)
                o32 = R.contract(g.float().bfloat16().float(), *a32, rowscale=rs)
                assert torch.equal(o32["u"].double(), o["u"]) and torch.equal(o32["s1"].double(), o["s1"])
                acc = (o["u"] - a[4]) / a[3]
                assert float(acc.abs().max()) * 2 ** 8 < 2 ** 24, "the accumulator leaves 24 bits of the grid"
        part = R.part_tiles(xd, s, ho, wo, q["th"], q["tw"]) if k == 3 else R.part_slices(xd, 3)
        assert torch.equal(part.float().double(), part)


@pytest.mark.parametrize("dtype", BOTH)
def test_k1_statistics_and_pooling_lattice_cases_are_exact(dtype):
    """the same for the k = 1 statistics rows (K1_CASES: v, the maximum, the channel sum, the partials in their slicing) and for the inputs of
    ly_colsum / ly_se_fwd (the partials); measure_k walks the rounded twins of the former (the partials are plain sums: a chain, no K)"""
    for cid, row in R.K1_CASES.items():
        x = R.k1_inputs(cid, dtype, "lattice")
        n, hw, c = x["n"], x["wo"], x["c"]
        pq = R.stored_params(x["p"], "rf3c")
        xd = R.d(x["x"])
        v = R.gen_v(xd, pq, 1, 1, False)
        v32 = R.gen_v(xd.float(), {key: val.float() for key, val in pq.items()}, 1, 1, False)
        assert torch.equal(v32.double(), v) and float(v.max()) < 16 and torch.equal((v * 16).round(), v * 16), cid
        g = torch.clamp(v, min=0.0)
        assert torch.equal(g.float().sum(-1).double(), g.sum(-1)) and torch.equal(g.float().amax(-1).double(), g.amax(-1))
        fl = (g.float().sum(-1) * torch.tensor(1.0 / c, dtype=torch.float32)).double()
        assert bool(((fl - g.sum(-1) / c).abs() <= (0.0 if c & (c - 1) == 0 else R.ULP_MEAN) * (g.sum(-1) / c)).all()), cid
        if row[4] != 0:
            part = R.part_slices(xd, R.k1_slices(hw, row[4]))
            assert torch.equal(R.part_slices(xd.float(), R.k1_slices(hw, row[4])).double(), part) and float(part.abs().max()) * 4 < 2 ** 24
    for cid in R.SE_CASES:
        x = R.se_x_inputs(cid, dtype, "lattice")
        xd = R.d(x["x"])
        assert torch.equal(R.part_slices(xd.float(), x["slices"]).double(), R.part_slices(xd, x["slices"])) and torch.equal(R.d(x["x"].float().to(dtype)), xd)


@pytest.mark.parametrize("family", FAM)
@pytest.mark.parametrize("cid", list(R.RM_CASES))
def test_rf3m_reference_weights_are_the_stream(cid, family):
    """the bf16-rounded folded weights and the three-way split shift of the ly_rf3m reference are what pack.rf3m_stream holds, value for value"""
    from lead_yolo_amd import pack
    x, q = R.case_inputs("rm", cid, R.BF16, family)
    c, p = q["c"], x["p"]
    stream = pack.rf3m_stream(p["w"].reshape(c * 9, 1, 3, 3), p["a"].reshape(-1), p["b"].reshape(-1), pool_stride=q["s"])
    wf, sh = R.unpack_rf3m_gen(stream[0], c)
    pq = R.stored_params(p, "rf3m")
    assert torch.equal(wf, pq["wf"]) and torch.equal(sh.sum(-1), pq["b"])
    main = pack.rf3m_stream(p["w"].reshape(c * 9, 1, 3, 3), p["a"].reshape(-1), p["b"].reshape(-1), x["wc"].view(-1, c, 3, 3), 4 if q["n_out"] % 128 == 0 else 2)
    mt = 4 if q["n_out"] % 128 == 0 else 2
    frag = main.double().view(q["n_out"] // (32 * mt), c // 16, -1, 64, 8)
    # main fragment (unit j, k-step s2, tile m): lane (r, h), element e <-> output 32 (g mt + m) + r, generated row 16 s2 + 8 (e // 4) + 4 h + e % 4
    wc = R.stored_wc(x["wc"], R.BF16)
    for gidx, ch, j, s2, m, lane, e in ((0, 0, 0, 0, 0, 0, 0), (0, c // 16 - 1, 3, 1, mt - 1, 63, 7), (q["n_out"] // (32 * mt) - 1, 0, 2, 1, 0, 37, 5)):
        r, hh = lane & 31, lane >> 5
        row = 16 * s2 + 8 * (e >> 2) + 4 * hh + (e & 3)
        assert float(frag[gidx, ch, j * (6 + 2 * mt) + 6 + s2 * mt + m, lane, e]) == float(wc[32 * (gidx * mt + m) + r, 16 * ch + 4 * j + (row >> 3), row & 7])


def test_rf3c_reference_weights_are_the_lane_image():
    """w, a, b and the folded wf = fl32(w a) of the references are what pack.rfcbam_gen_weights_c holds in either form; the lane = pixel images of
    pack.rfcbam_gen_weights hold the same folded values"""
    from lead_yolo_amd import pack
    x, q = R.case_inputs("rc_stats", "c64-s2-odd-7x9-pick", R.F32, "rounded")
    c, p = q["c"], x["p"]
    gw, gs, gb = p["w"].reshape(c * 9, 1, 3, 3), p["a"].reshape(-1), p["b"].reshape(-1)
    raw, fold = R.unpack_wq_c(pack.rfcbam_gen_weights_c(gw, gs, gb, raw=True), c), R.unpack_wq_c(pack.rfcbam_gen_weights_c(gw, gs, gb), c)
    assert torch.equal(raw[:, :81].view(c, 9, 9), p["w"]) and torch.equal(raw[:, 81:90], p["b"]) and torch.equal(raw[:, 90:99], p["a"])
    assert torch.equal(fold[:, :81].view(c, 9, 9), p["wf"]) and torch.equal(fold[:, 81:90], p["b"])
    img = pack.rfcbam_gen_weights(gw, gs, gb, 32, False).view(c // 32, 4, 9, 4, 10, 2)          # [q][wave][t][pair][10][ab]: channel 32 q + wave + 4 (2 pair + ab)
    ch = 32 + 2 + 4 * (2 * 3 + 1)
    assert torch.equal(img[1, 2, :, 3, :9, 1], p["wf"][ch]) and torch.equal(img[1, 2, :, 3, 9, 1], p["b"][ch])


def test_tile_pickers_are_those_of_ops():
    from lead_yolo_amd import ops
    for ho, wo in ((1, 1), (4, 5), (6, 10), (9, 10), (11, 12), (16, 16), (5, 20), (40, 40)):
        assert R.pick_tile(ho, wo) == ops.pick_tile(ho, wo)
        for s in (1, 2):
            assert R.pick_tile_c(ho, wo, s) == ops.pick_tile_c(ho, wo, s) and R.pick_tile_m(ho, wo, s) == ops.pick_tile_m(ho, wo, s)
    for hw in (1, 37, 100, 130, 200, 16500):
        assert R.k1_slices(hw, None) == max(1, min(hw // ops.PRE1_PIXELS, 128))


# ---------------------------------------------------------------- beacons ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", BOTH)
def test_beacons_dominate_their_sums(dtype):
    """every beacon product of every rounded contraction case is more than half of sum |wc B| of its output and more than 100 elementwise bounds;
    the placements cover a padded corner, the last pixel of the first tile, the last pixel of the map, the second image, the last channel chunk"""
    for table in ("rc_fwd", "rm", "rf3", "gemm"):
        for cid in R.TABLES[table]:
            if table == "rm" and dtype == R.F32:
                continue
            x, q = R.case_inputs(table, cid, dtype, "rounded")
            v, _ = R.want_for(x, _route(table), False)
            rep = R.beacon_report(x, v, R.stored_wc(x["wc"], dtype))
            assert all(share > 0.5 and over > 100 for share, over in rep), (table, cid, rep)
            bl = x["beacons"]
            assert bl[0][1:3] == (0, 0) and (q["n"] == 1 or any(b[0] == 1 and b[1:3] == (0, 0) for b in bl))
            assert any(b[1:3] == (q["ho"] - 1, q["wo"] - 1) for b in bl) and (len(bl) == 1 or all(b[4] >= q["c"] - 32 for b in bl[1:]))
            assert len({b[4] for b in bl}) == len(bl) and (q["k"] == 1 or all(b[3] != R.DEAD for b in bl))


# ---------------------------------------------------------------- planted defects -------------------------------------------------------------
STATS_DEFECT_CASE = "c64-s2-odd-7x9-pick"            # two images, odd H and W at stride 2, two channel chunks


@pytest.mark.parametrize("family", FAM)
@pytest.mark.parametrize("dtype", BOTH)
def test_mm_judge_rejects_planted_defects(dtype, family):
    """the [max, mean] judge: a clamped border, an exchanged pair of taps, the last channel chunk missing from the mean, the maximum of the
    pre-ReLU value, the folded weights in the raw form — each rejected on both families; the reference itself, rounded, passes"""
    x, q = R.case_inputs("rc_stats", STATS_DEFECT_CASE, dtype, family)
    n, ho, wo, k = q["n"], q["ho"], q["wo"], 3
    for raw in (False, True):
        v, vm = R.want_for(x, "rf3c", raw)
        R.judge_mm(R.mm_of(v, n, ho, wo, k).float(), x, v, vm, "the reference")
        assert int((R.mm_of(v, n, ho, wo, k)[..., 0] == 0).sum()) >= n * ho * wo - len(x["beacons"]), "the dead tap is not dead"
        for name in ("clamp", "swap_tap") + (("folded_in_raw",) if raw else ()):
            bad, _ = R.want_for(x, "rf3c", raw, **{name: True})
            _rejects(R.judge_mm, R.mm_of(bad, n, ho, wo, k).float(), x, v, vm, name)
        _rejects(R.judge_mm, R.mm_of(v, n, ho, wo, k, drop_chunk=True).float(), x, v, vm, "drop_chunk")
        _rejects(R.judge_mm, R.mm_of(v, n, ho, wo, k, pre_relu_max=True).float(), x, v, vm, "pre_relu_max")


@pytest.mark.parametrize("family", FAM)
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("table,cid", [("rc_fwd", "n256-wide-raw-stats-out"), ("rf3", "c48-n128-mt2-s2-odd-2x2-stats-out"), ("gemm", "k160-n64")])
def test_out_judge_rejects_planted_defects(table, cid, dtype, family):
    """the contraction judge: every generate defect, ca of the neighbouring image, rfa read at (wo, ho), the square sum taken after the ReLU and,
    on the rounded family in fp32 storage, the lo plane of the conv weight dropped"""
    x, q = R.case_inputs(table, cid, dtype, family)
    n, ho, wo, k, rs = q["n"], q["ho"], q["wo"], q["k"], q["k"] == 1
    raw = q["raw"]
    v, vm = R.want_for(x, "rf3c", raw)
    wc = R.stored_wc(x["wc"], dtype)
    a = (R.d(x["ca"]), R.d(x["rfa"]), wc, R.d(x["es"]), R.d(x["esh"]), n, ho, wo, k)
    for mode in ("relu", "stats-out"):
        lin = mode != "relu"
        good = R.contract(torch.clamp(v, min=0.0), *a, linear=lin, rowscale=rs)
        R.judge_out(_stored_out(good, x, mode), x, v, vm, mode, "the reference", rowscale=rs)
        names = (("clamp", "swap_tap") if k == 3 else ()) + (("folded_in_raw",) if raw else ())
        for name in names:
            bad, _ = R.want_for(x, "rf3c", raw, **{name: True})
            _rejects(R.judge_out, _stored_out(R.contract(torch.clamp(bad, min=0.0), *a, linear=lin, rowscale=rs), x, mode), x, v, vm, mode, name, rowscale=rs)
        for name in ("ca_next", "rfa_swapped"):
            bad = R.contract(torch.clamp(v, min=0.0), *a, linear=lin, rowscale=rs, **{name: True})
            _rejects(R.judge_out, _stored_out(bad, x, mode), x, v, vm, mode, name, rowscale=rs)
    bad = R.contract(torch.clamp(v, min=0.0), *a, linear=True, rowscale=rs, sq_after_relu=True)
    _rejects(R.judge_out, dict(stats=_stored_out(bad, x, "stats-only")["stats"]), x, v, vm, "stats-only", "sq_after_relu", rowscale=rs)
    if family == "rounded" and dtype == R.F32:
        a_hi = a[:2] + (R.d(x["wc"].bfloat16()),) + a[3:]
        bad = R.contract(torch.clamp(v, min=0.0), *a_hi, rowscale=rs)
        _rejects(R.judge_out, _stored_out(bad, x, "relu"), x, v, vm, "relu", "lo plane dropped", rowscale=rs)


def test_small_step_judges_reject_planted_defects():
    """ca: the mean taken over one slice too few, the hidden ReLU missing; rfa: the conv's border clamped, its taps transposed; part: a slice
    boundary one pixel off"""
    for cid in ("n3-c160-r10-nq40", "n9-c256-r16-trip-plus-one"):
        x = R.se_inputs_fwd(cid)
        a = (R.d(x["part"]), R.d(x["wa"]), R.d(x["wb"]), x["hw"])
        R.judge_ca(R.se_ca(*a)["ca"].float(), x, cid)
        _rejects(R.judge_ca, R.se_ca(a[0][:, :-1], *a[1:])["ca"].float(), x, cid + " a slice dropped")
        gap = a[0].sum(1) / x["hw"]
        _rejects(R.judge_ca, torch.sigmoid((gap @ a[1].t()) @ a[2].t()).float(), x, cid + " no ReLU")
    for cid in ("halo-four-tiles-17x65", "tail-wk-7", "hk-1"):
        x = R.map_inputs(cid)
        mm, w18 = R.d(x["mm"]), R.d(x["w18"])
        R.judge_rfa(R.getw_fwd(mm, w18).float(), x, cid)
        pad = torch.nn.functional.pad(mm.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate")
        bad = torch.sigmoid(torch.nn.functional.conv2d(pad, w18.view(1, 2, 3, 3)))[:, 0]
        _rejects(R.judge_rfa, bad.float(), x, cid + " clamped")
        _rejects(R.judge_rfa, R.getw_fwd(mm, w18.view(2, 3, 3).transpose(1, 2).reshape(18)).float(), x, cid + " transposed")
    for family in R.FAMILIES:
        x, q = R.case_inputs("rc_stats", "c32-s1-ragged-4x6", R.F32, family)
        xd = R.d(x["x"])
        want, wabs = R.part_tiles(xd, 1, q["ho"], q["wo"], 4, 6), R.part_tiles(xd.abs(), 1, q["ho"], q["wo"], 4, 6)
        R.judge_part(want.float(), x, want, wabs, 12, family)
        _rejects(R.judge_part, R.part_tiles(xd, 1, q["ho"], q["wo"], 4, 5).float()[:, :9], x, want, wabs, 12, family + " tile one column short")


# ---------------------------------------------------------------- case ids take the branch they name ----------------------------------------
def _describe(fn, *args, cap=160):
    from lead_yolo_amd import capi
    name = ctypes.create_string_buffer(cap)
    rc = getattr(capi.lib(), fn)(*[ctypes.byref(a) if isinstance(a, ctypes.Structure) else a for a in args], name, cap)
    assert rc == 0, capi.lib().ly_last_error().decode()
    return name.value.decode()


def _params(q, dtype, mode="relu", wg=True):
    from lead_yolo_amd import capi
    return capi.LyRfcbam3Params(n_img=q["n"], H=q["h"], W=q["w"], C=q["c"], Ho=q["ho"], Wo=q["wo"], N=q["n_out"], s=q["s"], TH=q["th"], TW=q["tw"], x=A, ldx=q["c"],
                                wg=B if wg else None, ca=C_, rfa=C_ + 65536, wp=D, e_scale=E, e_shift=E + 4096, out=None if mode == "stats-only" else F_, ldo=q["n_out"],
                                stats=F_ + (1 << 20) if mode.startswith("stats") else None, linear=int(mode == "linear"), dtype=capi.dtype_code(dtype))


@pytest.mark.parametrize("dtype", BOTH)
def test_case_ids_take_the_kernel_they_name(dtype):
    """ly_rf3c_fwd_describe, ly_rf3m_fwd_describe, ly_rfcbam3_describe, ly_rfcbam_stats_describe and ly_gemm_describe on every case id: the
    kernel and template arguments the dispatch rules (restated in tests/rfcbam_fwd_ref.py from the comments of csrc/) give, and what the id says"""
    from lead_yolo_amd import capi
    code = capi.dtype_code(dtype)
    for cid in R.RC_FWD:
        q = R.case("rc_fwd", cid)
        name = _describe("ly_rf3c_fwd_describe", _params(q, dtype, q["mode"], wg=False), ctypes.c_void_p(B), int(q["raw"]))
        assert name == R.rf3c_claim(dtype, q["n_out"], q["s"], q["raw"]), (cid, name)
        mt_nw = name.split("<")[1].split(", ")[1:3]
        want = {"n64": ["1", "4"], "n72": ["2", "4"], "n80": ["2", "4"], "n128": ["2", "4"], "n256": ["2", "8"] if dtype == R.BF16 else ["2", "4"]}[cid.split("-")[0]]
        assert mt_nw == want and ("raw" in cid) == q["raw"] and (f"-s{q['s']}-" in R.RC_FWD[cid][0]), (cid, name)
    if dtype == R.BF16:
        for cid in R.RM_CASES:
            q = R.case("rm", cid)
            name = _describe("ly_rf3m_fwd_describe", _params(q, dtype, wg=False))
            assert name == R.rf3m_claim(q["n_out"]) and f"-mt{name.split('<')[1][0]}-" in cid, (cid, name)
    for cid in R.RF3_CASES:
        q = R.case("rf3", cid)
        blocks = q["n"] * R._cdiv(q["ho"], q["th"]) * R._cdiv(q["wo"], q["tw"]) * R._cdiv(q["n_out"], 64 * (4 if q["n_out"] > 128 else 2 if q["n_out"] > 64 else 1))
        name = _describe("ly_rfcbam3_describe", _params(q, dtype, q["mode"]))
        assert name == R.rf3_claim(dtype, q["n_out"], blocks), (cid, name)
        assert ("-sw-" in cid) == ("_sw_" in name) and (f"{blocks}-blocks" in cid or "blocks" not in cid), (cid, name, blocks)
        if "-mt" in cid:
            assert f"-mt{name.split(', ')[1][0]}-" in cid, (cid, name)
    for cid, row in R.K1_CASES.items():
        n, hw, c, slices = row[0], row[1], R.k1_c(row, dtype), row[4]
        part = slices != 0
        name = _describe("ly_rfcbam_stats_describe", ctypes.c_void_p(A), c, n, 1, hw, c, 1, 1, None, ctypes.c_void_p(B), ctypes.c_void_p(B + 4096), 1, 64, ctypes.c_void_p(C_),
                         ctypes.c_void_p(D) if part else None, R.k1_slices(hw, slices) if part else 0, code)
        assert name == R.stats1_claim(dtype, c, part), (cid, name)
        if cid.startswith("pre1v"):
            assert name.startswith("ly_rfcbam_pre1v_kernel") and name.rstrip(">").endswith(cid.split("-")[1]), (cid, name)
        elif cid.startswith("pre1-plain"):
            assert name.startswith("ly_rfcbam_pre1_kernel"), (cid, name)
        else:
            assert name.startswith("ly_rfcbam_stats1_kernel"), (cid, name)
    for cid in R.ST3_CASES:
        q = R.case("st3", cid)
        name = _describe("ly_rfcbam_stats_describe", ctypes.c_void_p(A), q["c"], q["n"], q["h"], q["w"], q["c"], 3, q["s"], ctypes.c_void_p(B), None, None, q["th"], q["tw"],
                         ctypes.c_void_p(C_), None, 0, code)
        assert name == f"ly_rfcbam_stats3_kernel<{'__bf16' if dtype == R.BF16 else 'float'}>", (cid, name)
    for cid in R.GEMM_CASES:
        q = R.case("gemm", cid)
        m = q["n"] * q["h"] * q["w"]
        P = capi.LyGemmParams(M=m, H=q["h"], W=q["w"], K=q["c"], N=q["n_out"], a0=A, lda0=q["c"], k0=q["c"], gather=capi.GATHER_ROWS, pro=capi.PRO_AFFINE_RELU_CA, wp=B,
                              p_scale=E, p_shift=E + 4096, p_ca=E + 8192, rowscale=F_, e_scale=C_, e_shift=C_ + 4096, act=capi.ACT_RELU, out=D, ldo=q["n_out"], stats=None, dtype=code)
        name = _describe("ly_gemm_describe", P)
        assert name == R.gemm_claim(dtype, q["c"], q["n_out"]), (cid, name)


def test_block_and_tile_arithmetic_of_the_case_ids():
    """what the ids say about tiles and blocks: ly_rf3m's tile totals against its 8 wave tiles per block, the tiles that read the most input
    positions, ragged tiles, the k = 1 slice counts and the 4096-block cap of the statistics pass without partials"""
    tiles = {}
    for cid in R.RM_CASES:
        q = R.case("rm", cid)
        per = R._cdiv(q["ho"], q["th"]) * R._cdiv(q["wo"], q["tw"])
        tiles[cid] = (per, q["n"] * per, (q["s"] * (q["th"] - 1) + 3) * (q["s"] * (q["tw"] - 1) + 3))
        assert q["th"] * q["tw"] <= 32 and tiles[cid][2] <= 160
    assert tiles["c32-s1-n64-mt2-25-tiles-partial-last-block"][1] == 25
    per, tot, pos = tiles["c64-s2-n128-mt4-4x8-maxpos-3img-straddle"]
    assert pos == 153 and tot % 8 != 0 and per % 8 != 0 and tot > 8, "no block holds tiles of two images"
    assert tiles["c32-s2-n128-mt4-odd-pick-6-tiles-one-partial-block"][1] == 6 and tiles["c64-s1-n64-mt2-pick-1x1-map"][1] == 2
    for cid, pos in (("c64-s2-4x16-maxpos", 9 * 33), ("c96-s2-3img-8x8-maxpos", 17 * 17)):
        q = R.case("rc_stats", cid)
        assert (q["s"] * (q["th"] - 1) + 3) * (q["s"] * (q["tw"] - 1) + 3) == pos <= 320
    q = R.case("rc_stats", "c32-s1-ragged-4x6")
    assert q["ho"] % q["th"] and q["wo"] % q["tw"]
    q = R.case("rc_stats", "c64-s2-odd-7x9-pick")
    assert q["h"] % 2 == 1 and q["w"] % 2 == 1 and (q["th"], q["tw"]) == R.pick_tile_c(q["ho"], q["wo"], 2)
    assert R.case("rc_stats", "c32-s1-1x1-map-tile1x2")["ho"] == 1
    q = R.case("st3", "c48-s3-2x2")
    assert (q["s"] * (q["th"] - 1) + 3) * (q["s"] * (q["tw"] - 1) + 3) * 8 <= 10 * 256
    # the lane = pixel pass pools the inputs a tile owns out of its staged tile: row 1 + (s TH - 1) of s (TH - 1) + 3 staged rows exists for s <= 2 only
    # (the entry refuses the fused partials at a larger stride; tests/test_gpu_rfcbam_fwd.py::test_refusals)
    assert [s for s in (1, 2, 3, 4) if all(s * th <= s * (th - 1) + 2 for th in range(1, 65))] == [1, 2]
    assert R.k1_slices(37, None) == 1 and 200 % 7 != 0 and R.k1_slices(130, None) == 2
    assert (16500 + 3) // 4 > 4096 >= (2 * 37 + 3) // 4
