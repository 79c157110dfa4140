"""What do the device packers write?  ly_frag_pack3, ly_pack_table, ly_rfcbam_tap_moments and ly_rfcbam_gen_prepare against the host.

In training every packed weight image is rebuilt on the device each optimiser step: one ly_pack_table launch reads the fp32 parameters in
place through LyPackDesc index maps, and ly_rfcbam_gen_prepare writes three differently ordered images of the `generate` weights from the
batch statistics.  tests/test_pack_host.py pins the host packers and the descriptor formula to their documented index maps; here the
device images are held to those host packers BIT FOR BIT (layouts are integer maps and the bf16 split is round-to-nearest-even on both
sides: there is no tolerance), and the two statistics kernels to float64 with bounds counted from their fp32 operations.

The freshness tests (tests/test_gpu_freshness.py) check WHEN images are rebuilt; this file checks WHAT is written."""
import math

import numpy as np
import pytest
import torch

from oracle import synth
from tests.test_gpu_modules import _dev
from tests.test_pack_host import PACK3_SHAPES, _rand, _t, emulate, pack3_matrix

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
U = 2.0 ** -24                                          # fp32 unit roundoff


@pytest.fixture(autouse=True)
def _no_sink_left_behind(monkeypatch):
    """a fused optimiser's first step installs a process-wide gradient sink: every test starts without one and puts back what it found"""
    from lead_yolo_amd import ops
    monkeypatch.setattr(ops, "SINK", None)


def _same_bits(got, want, what):
    assert got.dtype == torch.int16 and want.dtype == torch.int16 and got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.cpu(), want
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        planes = sorted(set(bad[:, 2].tolist()))
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ, planes {planes}, first (t, s, plane, lane, j) {bad[:3].tolist()}")


# ---- ly_frag_pack3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", (1, 2))
def test_frag_pack3_device_matches_host(planes):
    """the host shapes (rows_to beyond R among them), then a transposed view and a column slice of a larger matrix (ld_r, ld_k not 1 / K)"""
    from lead_yolo_amd import pack
    dev = _dev()
    for R, K, rows_to in PACK3_SHAPES + ((16, 32, 48),):
        w = torch.from_numpy(pack3_matrix(R, K, 100 + R))
        _same_bits(pack.frag_pack3(w.to(dev), rows_to=rows_to, planes=planes), pack.frag_pack3(w, rows_to=rows_to, planes=planes), (R, K, rows_to))
    w = torch.from_numpy(pack3_matrix(37, 45, 9))
    wd = w.to(dev)
    _same_bits(pack.frag_pack3(wd.t(), rows_to=64, planes=planes), pack.frag_pack3(w.t().contiguous(), rows_to=64, planes=planes), "transposed view")
    _same_bits(pack.frag_pack3(wd[:, 3:40], planes=planes), pack.frag_pack3(w[:, 3:40].contiguous(), planes=planes), "column slice")
    _same_bits(pack.frag_pack3(wd[5:30].t()[2:33], planes=planes), pack.frag_pack3(w[5:30].t()[2:33].contiguous(), planes=planes), "slice of a transposed slice")


# ---- pack.packed / ly_pack_table ----------------------------------------------------------------------------------------------------
def _forms(dev):
    """every descriptor form the code uses -> [(name, device tensors kept alive, parts, K, rows_to, the matrix in plain torch ops)].
    tests/test_pack_host.py holds the same forms to the descriptor formula on the CPU."""
    from lead_yolo_amd import pack
    out = []

    def add(name, ws, make, K, want, rows_to=0):
        wd = [w.to(dev) for w in ws]
        parts = make(*wd)
        out.append((name, wd, parts, K, rows_to, want))

    w = _t((19, 37), 1)
    add("src_matrix", [w], lambda d: pack.src_matrix(d, 19, 37), 37, w)
    add("src_matrix rows_to", [w.clone()], lambda d: pack.src_matrix(d, 19, 37), 37, w, rows_to=48)
    add("src_matrix transposed", [w.clone()], lambda d: pack.src_matrix(d, 37, 19, sr=1, sk=37), 19, w.t())
    add("src_matrix transposed k_pad", [w.clone()], lambda d: pack.src_matrix(d, 37, 19, sr=1, sk=37, k_pad=32), 32, torch.cat((w.t(), torch.zeros(37, 13)), 1))
    for shape, cip in (((5, 6, 3, 3), 8), ((5, 6, 3, 3), 32), ((7, 8, 3, 3), 8)):
        w4 = _t(shape, 3)
        add(f"src_taps {shape} cip {cip}", [w4], lambda d, cip=cip: pack.src_taps(d, cip), 9 * cip, pack.conv_taps_matrix(w4, cip))
    for shape, cop in (((5, 6, 3, 3), 8), ((5, 6, 3, 3), 32), ((8, 7, 3, 3), 8)):
        w4 = _t(shape, 4)
        add(f"src_taps flipped {shape} cop {cop}", [w4], lambda d, cop=cop: pack.src_taps(d, cop, transposed_flipped=True), 9 * cop,
            pack.conv_taps_matrix(w4.permute(1, 0, 2, 3).flip(2, 3), cop))
    w1, w2 = _t((12, 20), 5), _t((12, 20), 6)
    full = torch.cat((w1.t(), w2.t()), 1)
    add("kcat_t", [w1, w2], lambda a, b: pack.src_matrix_kcat_t(a, b), 24, full)
    add("kcat_t rows 5:17", [w1.clone(), w2.clone()], lambda a, b: pack.src_matrix_kcat_t(a, b, 5, 17), 24, full[5:17])
    add("kcat_t rows 8:", [w1.clone(), w2.clone()], lambda a, b: pack.src_matrix_kcat_t(a, b, 8, None), 24, full[8:])
    co, c, k = 10, 6, 2
    w4 = _t((co, c, k, k), 6)
    add("transposed patch matrix", [w4], lambda d: pack.Src(d, k * k * c, nrb=c, sra=1, srb=k * k, nc=co, sc=c * k * k), co,
        w4.reshape(co, c, k * k).permute(2, 1, 0).reshape(k * k * c, co))
    o, c = 7, 32
    w4 = _t((o, c, 3, 3), 7)
    ten = torch.zeros(o, c // 16, 10, 16)
    ten[:, :, :9] = w4.reshape(o, c // 16, 16, 9).transpose(2, 3)
    add("rfcbam ten slots", [w4], lambda d: pack.Src(d, o, srb=c * 9, nb=10, vb=9, nc=16, sa=144, sb=1, sc=9), (c // 16) * 160, ten.reshape(o, -1))
    o, c = 5, 64
    w4 = _t((o, c, 3, 3), 8)
    add("rfcbam lane = channel taps", [w4], lambda d: pack.Src(d, o, srb=c * 9, nb=9, nc=32, sa=288, sb=1, sc=9), 9 * c,
        w4.reshape(o, c // 32, 32, 9).transpose(2, 3).reshape(o, 9 * c))
    # C3_CA's cv1 | cv2: the first part a multiple of 16 rows, the second not, rows_to beyond both
    wa, wb = _t((32, 24), 9), _t((19, 24), 10)
    add("stacked cv1 | cv2", [wa, wb], lambda a, b: [pack.src_matrix(a, 32, 24), pack.src_matrix(b, 19, 24)], 24, torch.cat((wa, wb), 0), rows_to=80)
    # T * S * 64 = 64 < 256: one partly used block
    ws = _t((3, 5), 11)
    add("one partly used block", [ws], lambda d: pack.src_matrix(d, 3, 5), 5, ws)
    return out


@pytest.mark.parametrize("planes", (1, 2))
def test_packed_every_descriptor_form(planes):
    """pack.packed (one ly_pack_table launch per new image) == host frag_pack3 of the matrix the form is meant to be"""
    from lead_yolo_amd import pack
    for name, keep, parts, K, rows_to, want in _forms(_dev()):
        plist = parts if isinstance(parts, list) else [parts]
        assert all(p is not None for p in plist), name
        # the descriptor on the host first: every read inside its tensor (emulate asserts it), and the matrix it is meant to be
        cpu = [w.cpu().numpy().reshape(-1) for w in keep]
        mats = [emulate(p, K, cpu[i]) for i, p in enumerate(plist)] if plist[0]._ref2 is None else [emulate(plist[0], K, cpu[0], flat2=cpu[1])]
        assert np.array_equal(np.concatenate(mats, 0), want.numpy()), name
        got = pack.packed(parts, K, planes, rows_to=rows_to)
        torch.cuda.synchronize()
        _same_bits(got, pack.frag_pack3(want.contiguous(), rows_to=rows_to, planes=planes), name)
        del keep


def test_pack_table_one_refresh_rebuilds_many_images(monkeypatch):
    """six images of different sizes and plane counts (1 to 4 blocks each, last blocks partly used: the blk0 offsets), every source changed
    in place, ONE ly_pack_table launch, every image checked; then a write through `.data` (no version counter moves) + touch_weights()"""
    from lead_yolo_amd import pack
    dev = _dev()
    shapes = ((16, 32, 2), (19, 37, 1), (33, 100, 2), (48, 64, 1), (100, 33, 2), (5, 300, 2))
    ws = [_t((r, k), 20 + i).to(dev) for i, (r, k, _) in enumerate(shapes)]
    host = lambda i: pack.frag_pack3(ws[i].cpu(), planes=shapes[i][2])
    imgs = [pack.packed(pack.src_matrix(w, r, k), k, pl) for w, (r, k, pl) in zip(ws, shapes)]
    assert sorted(math.ceil(im.shape[0] * im.shape[1] * 64 / 256) for im in imgs) == [1, 1, 2, 3, 3, 4]
    for i, im in enumerate(imgs):
        _same_bits(im, host(i), ("first pack", shapes[i]))
    before = [im.clone() for im in imgs]
    for i, w in enumerate(ws):
        w.mul_(-1.25 - i)                                 # in place: the version counters move
    launches = []
    real = pack.PLAN._launch
    monkeypatch.setattr(pack.PLAN, "_launch", lambda table: (launches.append(table[2]), real(table))[1])
    again = [pack.packed(pack.src_matrix(w, r, k), k, pl) for w, (r, k, pl) in zip(ws, shapes)]
    torch.cuda.synchronize()
    assert len(launches) == 1 and launches[0] >= 14, launches
    for i, (im, ag) in enumerate(zip(imgs, again)):
        assert ag.data_ptr() == im.data_ptr()              # the persistent image, rebuilt in place
        assert not torch.equal(im, before[i])
        _same_bits(im, host(i), ("refresh", shapes[i]))
    # a write behind the version counters, announced by touch_weights()
    for i, w in enumerate(ws):
        w.data.copy_(_t(tuple(w.shape), 40 + i))
    pack.touch_weights()
    again = [pack.packed(pack.src_matrix(w, r, k), k, pl) for w, (r, k, pl) in zip(ws, shapes)]
    torch.cuda.synchronize()
    assert len(launches) == 2, launches
    for i, im in enumerate(again):
        _same_bits(im, host(i), ("touch_weights", shapes[i]))


# ---- whole-model sweep ---------------------------------------------------------------------------------------------------------------
def _family(model):
    """parameter (by id) -> (name, family)"""
    import lead_yolo_amd as L
    mods = dict(model.named_modules())
    fam = {}
    for name, p in model.named_parameters():
        parts = name.split(".")
        chain = [mods[".".join(parts[:i])] for i in range(len(parts) - 1, 0, -1)]          # innermost first
        f = None
        for m in chain:
            if isinstance(m, L.MLPBlock):
                f = "MLPBlock " + ("pconv" if "partial_conv3" in name else "mlp.0" if name.endswith("mlp.0.weight") else "mlp.3" if name.endswith("mlp.3.weight") else "other")
            elif isinstance(m, L.RFCBAMConv):
                f = f"RFCBAMConv k={m.kernel_size}"
            elif isinstance(m, L.Detect):
                f = "Detect"
            elif isinstance(m, L.PatchEmbed_FasterNet):
                f = "PatchEmbed"
            elif isinstance(m, L.PatchMerging_FasterNet):
                f = "PatchMerging"
            elif isinstance(m, L.Conv):
                f = f"Conv {m.conv.kernel_size[0]}x{m.conv.kernel_size[0]}"
            if f is not None:
                break
        fam[id(p)] = (name, f or "other")
    return fam


def _form(src):
    if src._ref2 is not None:
        return "kcat"
    if src.sb < 0:
        return "flipped"
    if src.nrb != src.rows or (src.srb == 1 and src.sc != 1):
        return "transposed"
    return "plain"


NEEDED = {("PatchEmbed", "plain"), ("PatchMerging", "plain"), ("MLPBlock pconv", "plain"), ("MLPBlock pconv", "flipped"), ("MLPBlock mlp.0", "plain"),
          ("MLPBlock mlp.0", "transposed"), ("MLPBlock mlp.3", "plain"), ("MLPBlock mlp.3", "transposed"), ("Conv 1x1", "plain"), ("Conv 3x3", "plain"),
          ("C3_CA stack", "plain"), ("C3_CA", "kcat"), ("RFCBAMConv k=1", "plain"), ("RFCBAMConv k=3", "plain"), ("Detect", "plain")}


@pytest.mark.parametrize("amp", (None, BF), ids=("fp32", "bf16"))
def test_every_image_of_the_training_model(amp):
    """lead-yolo-n, 2 x 3 x 64 x 64: one fused-SGD train step (the weights move behind the version counters), then one more forward +
    backward (the first request refreshes every image from the stepped weights).  Every image of pack.PLAN that reads this model's parameters
    is rebuilt on the host — the descriptor formula (tests/test_pack_host.emulate) over the parameters' current values, then the host
    frag_pack3 — and must be the same bits.  None is skipped, and every weight family is among them."""
    import lead_yolo_amd as L
    from lead_yolo_amd import pack
    dev = _dev()
    torch.manual_seed(0)
    cfg = L.load_cfg(scale="n")
    model = L.Model(cfg)
    st = synth.synth_state(synth.shapes_of(model.state_dict()), 4343)
    st["model.23.anchors"] = model.model[-1].anchors.clone()
    model.load_state_dict(st)
    model = model.to(dev).train()
    imgs, tg = synth.synth_images(2, 64, 17).to(dev), synth.synth_targets(2, 18, per_image=3).to(dev)
    opt = L.smart_optimizer(model, "SGD", 0.01, 0.937, 5e-4)
    assert isinstance(opt, L.FusedSGD)
    cl = L.ComputeLoss(model)
    w0 = {k: p.detach().clone() for k, p in model.named_parameters()}
    loss, _ = L.train_step(model, cl, opt, imgs, tg, amp=amp)
    assert math.isfinite(float(loss))
    L.forward_backward(model, cl, imgs, tg, amp=amp)
    torch.cuda.synchronize()
    fam = _family(model)
    moved = sum(not torch.equal(p.detach(), w0[k]) for k, p in model.named_parameters())
    assert moved > 0.9 * len(w0), moved                      # the images below are of the STEPPED weights
    flat = {}

    def values(t):
        if id(t) not in flat:
            flat[id(t)] = t.detach().cpu().numpy().reshape(-1)
        return flat[id(t)]

    covered, names, checked = set(), set(), 0
    for key, e in list(pack.PLAN.entries.items()):
        refs = [(s._ref(), s._ref2() if s._ref2 is not None else None) for s in e["parts"]]
        own = [p is not None and id(p) in fam for p, _ in refs]
        if not any(own):
            continue                                         # another model's image (the plan is process-wide)
        assert all(own) and all(q is None or id(q) in fam for _, q in refs), "an image mixes this model's parameters with foreign sources"
        mats = []
        for s, (p, q) in zip(e["parts"], refs):
            assert s.param is p and p.data_ptr() == s.ptr and p.dtype == torch.float32
            mats.append(emulate(s, e["K"], values(p), flat2=None if q is None else values(q)))
            for t in (p, q):
                if t is not None:
                    name, f = fam[id(t)]
                    names.add(name)
                    covered.add((("C3_CA" if q is not None else f), _form(s)))
            if len(e["parts"]) > 1:
                covered.add(("C3_CA stack", _form(s)))
        want = pack.frag_pack3(torch.from_numpy(np.ascontiguousarray(np.concatenate(mats, 0), dtype=np.float32)), rows_to=key[3], planes=e["planes"])
        _same_bits(e["out"], want, [fam[id(p)][0] for p, _ in refs])
        checked += 1
    print(f"model sweep {'bf16' if amp is BF else 'fp32'}: {checked} images over {len(names)} parameters, planes {sorted({e['planes'] for e in pack.PLAN.entries.values()})}")
    assert checked >= 40 and NEEDED <= covered, f"{checked} images; missing families {sorted(NEEDED - covered)}; parameters covered: {sorted(names)}"


# ---- ly_rfcbam_tap_moments ----------------------------------------------------------------------------------------------------------
def _tap_sums(x, s):
    """float64 [n, H, W, C] -> (moments [54, C], sums of absolute terms [54, C], L = n Ho Wo): 9 first and 45 second moments (row-major
    upper triangle) of the zero-padded stride-s 3 x 3 taps"""
    n, H, W, C = x.shape
    Ho, Wo = (H + 2 - 3) // s + 1, (W + 2 - 3) // s + 1
    xp = np.zeros((n, H + 2, W + 2, C))
    xp[:, 1:H + 1, 1:W + 1] = x
    taps = [xp[:, u // 3: u // 3 + s * (Ho - 1) + 1: s, u % 3: u % 3 + s * (Wo - 1) + 1: s] for u in range(9)]
    assert all(t.shape == (n, Ho, Wo, C) for t in taps)
    terms = list(taps) + [taps[u] * taps[v] for u in range(9) for v in range(u, 9)]
    mom = np.stack([t.sum((0, 1, 2)) for t in terms])
    mag = np.stack([np.abs(t).sum((0, 1, 2)) for t in terms])
    return mom, mag, n * Ho * Wo


def _tiled(s, C, esz):
    """the dispatch of ly_rfcbam_tap_moments for a dense, 16-byte aligned x: the stride-2 LDS-tile kernel, else the per-pixel kernel"""
    return s == 2 and C % (16 // esz) == 0


TAP_CASES = ((1, (2, 9, 11, 24), torch.float32), (2, (2, 13, 18, 32), torch.float32), (2, (1, 17, 17, 96), torch.float32), (2, (2, 13, 18, 40), BF),
             (2, (1, 7, 9, 6), torch.float32), (1, (1, 5, 6, 12), BF))


def test_tap_moment_cases_reach_both_kernels():
    for dt in (torch.float32, BF):
        assert {_tiled(s, shp[3], 4 if dt == torch.float32 else 2) for s, shp, d in TAP_CASES if d == dt} == {True, False}


@pytest.mark.parametrize("s,shape,dt", TAP_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_tap_moments_vs_float64(s, shape, dt):
    """odd sizes, partial 8 x 8 tiles, two channel groups (C = 96), a partly filled group (C = 40); both kernels in both storage types.
    Bound: |got - want| <= L 2^-24 sum |terms| with L = n Ho Wo, the most terms one fp32 accumulator can take (every product of two bf16
    or fp32 taps is rounded once, every addition once; the doubles the partial sums are added into do not count).  A missing tap or pixel
    is about 1 / L of sum |terms|."""
    from lead_yolo_amd import capi
    dev = _dev()
    n, H, W, C = shape
    x = torch.from_numpy(_rand(shape, 60 + C, -2, 2)).to(dt)
    xd = x.to(dev).contiguous()
    mom = torch.zeros(54 * C, dtype=torch.float64, device=dev)
    capi.check(capi.lib().ly_rfcbam_tap_moments(capi.ptr(xd), C, n, H, W, C, s, capi.ptr(mom), capi.dtype_code(xd), capi.stream_ptr()), "ly_rfcbam_tap_moments")
    got = mom.cpu().numpy().reshape(54, C)
    want, mag, L = _tap_sums(x.double().numpy(), s)
    err = np.abs(got - want)
    bound = L * U * mag
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"tap moments s={s} {shape} {dt}: worst error / bound = {worst:.3f}")
    assert np.all(err <= bound), (worst, np.argwhere(err > bound)[:4].tolist())


# ---- ly_rfcbam_gen_prepare ----------------------------------------------------------------------------------------------------------
EPS, MOM = 1e-3, 0.03


@pytest.mark.parametrize("track", (True, False), ids=("tracked", "untracked"))
@pytest.mark.parametrize("k,C", ((3, 32), (3, 40), (1, 24)))
def test_gen_prepare_vs_float64(k, C, track):
    """Train-mode `generate` BatchNorm from moments supplied by the float64 reference (no statistics error mixes in).

    fp32 operations of ly_rfcbam_gen_prepare_kernel per output (everything before them is double arithmetic on the double moments):
      invstd = (float)(1 / sqrt(var + eps))                      1 rounding
      scale  = gamma * invstd                                    2
      mean   = (float)mean                                       1
      shift  = beta - (float)mean * scale                        5: mean 1, scale 2, product 1, difference 1 — relative to |beta| + |mean scale|
      running = (1 - momentum) * running + momentum * (float)x   6: momentum as a float 1, 1 - momentum 1, product 1, x 1, product 1, sum 1
    The bounds are (count + 1) 2^-24: one more for the second-order terms and the float64 reference's own rounding (the data keep
    mean^2 / var far below 2^20, so the cancellation in var = E a^2 - mean^2 costs the doubles nothing that shows at 2^-24)."""
    from lead_yolo_amd import capi, pack
    dev = _dev()
    kk = k * k
    G = C * kk
    gw = _rand((G, 1, k, k), 70 + C, -2, 2)
    zero_g = 2 * kk + (4 if k == 3 else 0)                  # a generate channel with all-zero weights: var = 0, invstd = eps^-1/2
    gw[zero_g] = 0
    gamma, beta = _rand((G,), 71, -1, 2), _rand((G,), 72, -2, 2)
    rmean0, rvar0 = _rand((G,), 73, -2, 2), np.abs(_rand((G,), 74, -2, 2))
    n, H, W, s = 2, 7, 9, 1
    x = _rand((n, H, W, C), 75, -2, 2).astype(np.float64) + 0.25
    w64 = gw.reshape(G, kk).astype(np.float64)
    if k == 3:
        m54, _, count = _tap_sums(x, s)
        momd = torch.from_numpy(m54.reshape(-1).copy())
        stripes = 1
        M = np.zeros((9, 9, C))
        iu = [(u, v) for u in range(9) for v in range(u, 9)]
        for i, (u, v) in enumerate(iu):
            M[u, v] = M[v, u] = m54[9 + i]
        wc = w64.reshape(C, 9, 9)
        s1 = np.einsum("ctu,uc->ct", wc, m54[:9]).reshape(G)
        s2 = np.einsum("ctu,uvc,ctv->ct", wc, M, wc).reshape(G)
    else:
        count = n * H * W
        xs = x.reshape(-1, C)
        stripes = 5                                          # striped [stripes][2C] moments, folded by the kernel in index order
        rows = np.array_split(np.arange(count), stripes)
        st = np.stack([np.concatenate((xs[r].sum(0), (xs[r] ** 2).sum(0))) for r in rows])
        momd = torch.from_numpy(st.reshape(-1).copy())
        m1 = m2 = 0.0
        for i in range(stripes):
            m1, m2 = m1 + st[i, :C], m2 + st[i, C:]
        s1, s2 = w64[:, 0] * m1, w64[:, 0] ** 2 * m2
    eps = float(np.float32(EPS))                             # the C ABI takes eps as a float
    mean = s1 / count
    var = np.maximum(s2 / count - mean * mean, 0.0)
    assert var[zero_g] == 0.0 and np.all(mean * mean <= 2.0 ** 10 * (var + eps))
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma.astype(np.float64) * invstd
    shift = beta.astype(np.float64) - mean * scale

    tt = lambda a, dtp=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dtp).to(dev)
    rmean, rvar, nbt = tt(rmean0), tt(rvar0), torch.tensor(3, dtype=torch.int64, device=dev)
    out8 = torch.full((8, G), float("nan"), device=dev)
    cps, cpm = (C + 31) // 32 * 32, (C + 15) // 16 * 16
    nan = lambda m: torch.full((m,), float("nan"), device=dev)
    a1 = nan(C) if k == 1 else None
    wqs, wqm = (nan(cps * 90), nan(cpm * 90)) if k == 3 else (None, None)
    wqc = nan(C * 100) if k == 3 and C % 32 == 0 else None
    gwd, gd, bd, md = tt(gw), tt(gamma), tt(beta), momd.to(dev)
    p = capi.ptr
    capi.check(capi.lib().ly_rfcbam_gen_prepare(p(md), C, k, p(gwd), p(gd), p(bd), EPS, MOM, float(count), p(rmean if track else None),
                                                p(rvar if track else None), p(nbt if track else None), p(out8), p(a1), p(wqs), p(wqm), p(wqc), stripes,
                                                capi.stream_ptr()), "ly_rfcbam_gen_prepare")
    torch.cuda.synchronize()
    o = out8.cpu()
    assert torch.isfinite(o).all()
    sc_d, sh_d, mean_d, inv_d = (o[i].double().numpy() for i in range(4))

    def close(got, want, mult, ref, what):
        err, bound = np.abs(got - want), mult * U * ref
        print(f"gen_prepare k={k} C={C} {what}: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert np.all(err <= bound), (what, np.argwhere(err > bound)[:4].tolist())

    close(inv_d, invstd, 2, np.abs(invstd), "invstd")
    close(sc_d, scale, 3, np.abs(scale), "scale")
    close(mean_d, mean, 2, np.abs(mean), "mean")
    close(sh_d, shift, 6, np.abs(beta.astype(np.float64)) + np.abs(mean * scale), "shift")
    assert abs(inv_d[zero_g] - 1.0 / math.sqrt(eps)) <= 2 * U / math.sqrt(eps) and mean_d[zero_g] == 0.0 and sh_d[zero_g] == float(beta[zero_g])
    # the same four in [t*C + c] order: the same bits, permuted
    for i in range(4):
        assert torch.equal(o[4 + i].view(kk, C), o[i].view(C, kk).t()), i
    # running statistics: nn.BatchNorm2d's rule (momentum, unbiased variance), or untouched when not tracked
    if track:
        want_m = (1 - MOM) * rmean0.astype(np.float64) + MOM * mean
        want_v = (1 - MOM) * rvar0.astype(np.float64) + MOM * var * count / (count - 1)
        close(rmean.cpu().double().numpy(), want_m, 7, np.abs((1 - MOM) * rmean0) + np.abs(MOM * mean), "running_mean")
        close(rvar.cpu().double().numpy(), want_v, 7, np.abs((1 - MOM) * rvar0) + np.abs(MOM * var * count / (count - 1)), "running_var")
        assert int(nbt) == 4
    else:
        assert np.array_equal(rmean.cpu().numpy(), rmean0) and np.array_equal(rvar.cpu().numpy(), rvar0) and int(nbt) == 3
    # the packed images: the layout, independently of the arithmetic — built on the host from the device's OWN scale / shift
    gwt = torch.from_numpy(gw)
    if k == 3:
        bits = lambda t: t.cpu().view(torch.int32)
        assert torch.equal(bits(wqs), bits(pack.rfcbam_gen_weights(gwt, o[0], o[1], 32, False))), "wq_stats"
        assert torch.equal(bits(wqm), bits(pack.rfcbam_gen_weights(gwt, o[0], o[1], 16, True))), "wq_main"
        if C % 32:
            # no wq_c at this C; the padded channels of wq_stats (up to 64) and wq_main (up to 48) were written, as exact zeros (the two
            # comparisons above hold them to the host's zeros; the buffers started as NaN)
            assert wqc is None and (cps, cpm) == (64, 48)
            assert int((wqs == 0).sum()) == (cps - C) * 90 + 9 and int((wqm == 0).sum()) == (cpm - C) * 90 + 9       # (+ the nine zero weights of `zero_g`)
        else:
            want_c = pack.rfcbam_gen_weights_c(gwt, o[0], o[1], raw=True).view(C // 32, 25, 32, 4)
            got_c = wqc.cpu().view(C // 32, 25, 32, 4)
            live = torch.ones(25, 4, dtype=torch.bool)
            live[24, 3] = False                              # element 99 of a channel: padding the kernel never writes and rc_load_w never uses
            live = live.view(1, 25, 1, 4).expand_as(got_c)
            assert torch.equal(got_c[live].view(torch.int32), want_c[live].view(torch.int32)), "wq_c"
    else:
        assert torch.equal(a1.cpu().view(torch.int32), (gwt.view(C) * o[0]).view(torch.int32)), "a1"
