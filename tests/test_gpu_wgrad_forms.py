"""The gathered and fp32 forms of the weight gradient (csrc/ly_wgrad.hip, ly_wgrad3.hip), each against float64 with a derived per-element bound:
3x3 / stride 1 / pad 1 and 3x3 / stride 2 / pad 1 gathers, the 2x2 / stride 2 patch gather, the 1x1 read through nearest-2x upsampling, the
4x4 / stride 4 gather of an NCHW image, plain rows on the per-lane kernel, in bf16 and fp32 storage, with the slab + fold and the float-atomic
flush.  tests/test_gpu_wgrad1.py holds the bf16 plain-row 1x1 problem the same way; its judge (_judge) is the one used here.

The reference is the header's formula (include/lead_yolo_hip.h, LyWgradParams) in float64, not the kernels' index arithmetic:
        dw[n][ky*ks + kx][c] = sum over m = (img, ho, wo) of du[m][n] * x[img, hi, wi, c],   hi = ho*stride + ky - pad, wi likewise,
a term being zero when (hi, wi) lies outside [0, Hv) x [0, Wv) (Hv = 2 Hin under up2, where the read is at (hi >> 1, wi >> 1)).  Per tap it
gathers the [M, Cin] matrix of source pixels and takes one du^T . Xtap; S is the same sum over |du| |x|.

The bound is derived, not tuned.

bf16 storage.  A product of two bf16 values is exact in fp32, so only fp32 summation errs: every addition rounds by at most 2^-24 of a partial
sum, no partial sum exceeds S, and an addition of an exact zero (a masked pixel, a padded tile slot, an empty accumulator) does not round.  So
        |got - want| <= A * 2^-24 * S,    A = the additions of non-zero terms on the longest path to an element:
at most one per pixel the run contracts (in whole MFMA steps: the chunk's pixels rounded up to steps of at most 128), at most one per partial
result that is folded or added atomically (never more partials than pixels), and the add into dw.  A = 2 * ceil128(M) + 1 covers the slab fold,
the atomic flush, the per-lane kernel's 256-pixel chunks and the 8 x 8 spatial tiles of ly_wgrad3 (whose empty slots are zeros) alike.  With dw
holding `base` and the call made t times: A + t - 1 additions, S_total = |base| + t S.

fp32 storage.  ly_split4 rounds to nearest twice: a = hi + lo + r, |lo| <= 2^-9 |a|, |r| <= 2^-18 |a|, and ly_mfma3 drops lo * lo: per product
at most (2^-18 + 2 * 2^-18 + O(2^-27)) |a b| < 2^-16 |a b| (the header's figure); three MFMAs per step add into the accumulator.  Worst case
        |got - want| <= (2^-16 + 3 A 2^-24) S.
The project documents 2^-14 S for this path (test_bf16x3_adversarial_bounds, tests/test_gpu_modules.py).  The worst-case figure stays inside
it only while 3 A <= 3 * 2^8, i.e. A <= 256, and A >= 257 at every map here: the worst-case summation term alone is then larger than the
documented bound (it grows with M, the split's term does not).  The judge therefore holds the fp32 kernels to the SMALLER of the two,
        |got - want| <= min(2^-16 + 3 A 2^-24, 2^-14) S      (+ (t - 1) 2^-24 S_total for the further calls' adds),
which at these maps is the documented 2^-14 S: never looser than the derivation, never looser than what the project promises.
test_bound_relations states these relations.

Which kernel a case runs on is part of the case list (CASES: the expected name of ly_wgrad_describe stands next to every case and
test_cases_run_on_the_kernels_they_name checks it on the host), so a change of the launch plan cannot leave a kernel untested unnoticed."""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

from tests.test_gpu_wgrad1 import GEOM, _dev, _judge

NAN = float("nan")
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}
TNAME = {"bf16": "__bf16", "f32": "float"}

# output maps (images, H, W): the smallest at which each index path can still go wrong
MAPS = [(1, 5, 7),           # 35 pixels: less than one step
        (3, 9, 13),          # 351: 8-pixel staging groups straddle row and image ends
        (32, 5, 7),          # 1120: three 384-pixel chunks (bf16: 128-pixel steps, fp32: 64), chunks begin mid-row and mid-image; slab fold / atomics
        (4, 1, 9),           # 36: ly_fdiv with H = 1
        (4, 9, 1)]           # 36: ly_fdiv with W = 1
UP2_MAPS = [(2, 6, 10), (3, 10, 14), (8, 12, 12)]          # even maps (the source is half the size); 1152 pixels: three chunks
NCHW_MAPS = [(2, 3, 5), (3, 8, 9), (16, 8, 9)]             # the image is 4x larger; 1152 pixels: five 256-pixel chunks of the per-lane kernel
ROW_MAPS = [GEOM[m] for m in (40, 72, 136, 1440)]          # 1440 pixels: six chunks of the per-lane kernel

# form -> gather, source size of an output size, maps
FORMS = {"k3s1": dict(ks=3, stride=1, pad=1, src=lambda o: o, maps=MAPS),
         "k3s2o": dict(ks=3, stride=2, pad=1, src=lambda o: 2 * o - 1, maps=MAPS),
         "k3s2e": dict(ks=3, stride=2, pad=1, src=lambda o: 2 * o, maps=MAPS),
         "k2s2": dict(ks=2, stride=2, pad=0, src=lambda o: 2 * o, maps=MAPS),
         "up2": dict(ks=1, stride=1, pad=0, up2=True, src=lambda o: o // 2, maps=UP2_MAPS),
         "k4nchw": dict(ks=4, stride=4, pad=0, nchw=True, src=lambda o: 4 * o, maps=NCHW_MAPS),
         "rows": dict(ks=1, stride=1, pad=0, src=lambda o: o, maps=ROW_MAPS)}


def _additions(m):
    return 2 * ((m + 127) // 128 * 128) + 1


def _a_eff(m, fp32, times=1):
    """the judge's factor of 2^-24 * S_total (module docstring)"""
    a = _additions(m)
    if fp32:
        a = min(2 ** 8 + 3 * a, 2 ** 10)
    return a + times - 1


def _reference(du, x, imgs, H, W, ks, stride, pad, up2=False, nchw=False, mutate=None):
    """(want, S) [N, ks*ks, Cin] in float64 from du [M, N] and x [imgs, Hin, Win, Cin] (nchw: [imgs, Cin, Hin, Win]).  mutate: one of the
    wrong gathers the judge has to tell from the right one (test_judge_rejects_wrong_gathers)."""
    du = du.double()
    if nchw:
        _, Cin, Hin, Win = x.shape
        s_img, s_ch, s_row, s_col = Cin * Hin * Win, Hin * Win, Win, 1
    else:
        _, Hin, Win, Cin = x.shape
        s_img, s_row, s_col, s_ch = Hin * Win * Cin, Win * Cin, Cin, 1
    if mutate == "swap":                                   # (e) channel and row taken in the other order: [img][row][channel][column]
        assert nchw
        s_row, s_ch = Cin * Win, Win
    Hv, Wv = (2 * Hin, 2 * Win) if up2 else (Hin, Win)
    flat = x.double().reshape(-1)
    m = torch.arange(imgs * H * W)
    img, ho, wo = m // (H * W), (m // W) % H, m % W
    if mutate == "droplast":                               # (b) the last pixel of the first image is lost
        du = du.clone()
        du[H * W - 1] = 0
    chan = torch.arange(Cin) * s_ch
    want, S = torch.zeros(du.shape[1], ks * ks, Cin, dtype=torch.float64), torch.zeros(du.shape[1], ks * ks, Cin, dtype=torch.float64)
    for tap in range(ks * ks):
        ky, kx = divmod(tap, ks)
        hi, wi = ho * stride + ky - pad, wo * stride + kx - pad
        if mutate == "shift" and tap == ks * ks // 2:      # (c) one tap reads the pixel to the right
            wi = wi + 1
        ok = (hi >= 0) & (hi < Hv) & (wi >= 0) & (wi < Wv)
        if up2:
            if mutate == "parity":                         # (d) (hi + 1) >> 1 in place of hi >> 1
                hi = (hi + 1) >> 1
                ok = ok & (hi < Hin)
            else:
                hi = hi >> 1
            wi = wi >> 1
        off = img * s_img + hi * s_row + wi * s_col
        if mutate == "nowrap":                             # (a) the left padding column reads the pixel before: the previous row's last one
            ok = ok | ((wi == -1) & (hi >= 0) & (hi < Hv) & (off >= 0))
        off = torch.where(ok, off, torch.zeros_like(off))
        xt = flat[off[:, None] + chan[None, :]] * ok[:, None]
        want[:, tap] = du.t() @ xt
        S[:, tap] = du.abs().t() @ xt.abs()
    return want.numpy(), S.numpy()


@functools.lru_cache(maxsize=None)
def _problem(form, n, cin, dtype, geom):
    """(du [M, N], x, want, S) of a form at a map: computed once, shared by every test that needs it, never written"""
    f = FORMS[form]
    imgs, H, W = geom
    Hin, Win = f["src"](H), f["src"](W)
    g = torch.Generator().manual_seed(zlib.crc32(repr((form, n, cin, dtype, geom)).encode()))
    du = torch.randn(imgs * H * W, n, generator=g).to(DTYPES[dtype])
    x = torch.randn((imgs, cin, Hin, Win) if f.get("nchw") else (imgs, Hin, Win, cin), generator=g).to(DTYPES[dtype])
    want, S = _reference(du, x, imgs, H, W, f["ks"], f["stride"], f["pad"], f.get("up2", False), f.get("nchw", False))
    return du, x, want, S


def _gather(form):
    f = FORMS[form]
    return dict(ks=f["ks"], stride=f["stride"], pad=f["pad"], up2=f.get("up2", False), nchw=f.get("nchw", False))


# ---------------------------------------------------------------------------------------------------------------------------------------
# host: the reference, the judge, the bound
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["k3s1", "k3s2o", "k3s2e", "k2s2", "k4nchw", "up2"])
def test_reference_equals_autograd_in_float64(form):
    """the reference == torch.nn.grad.conv2d_weight in float64 (3x3/s1/p1, 3x3/s2/p1 on odd and even inputs, 2x2/s2/p0, 4x4/s4/p0 from
    NHWC and from NCHW storage); under up2 the same function on F.interpolate(x, scale_factor=2, mode="nearest")"""
    import torch.nn.functional as F
    f = FORMS[form]
    n, cin = 5, 3
    for geom in f["maps"]:
        imgs, H, W = geom
        du, x, want, S = _problem(form, n, cin, "f32", geom)
        xc = (x if f.get("nchw") else x.permute(0, 3, 1, 2)).double()
        if f.get("up2"):
            xc = F.interpolate(xc, scale_factor=2, mode="nearest")
        gy = du.double().reshape(imgs, H, W, n).permute(0, 3, 1, 2)
        auto = torch.nn.grad.conv2d_weight(xc, (n, cin, f["ks"], f["ks"]), gy, stride=f["stride"], padding=f["pad"])
        auto = auto.permute(0, 2, 3, 1).reshape(n, f["ks"] ** 2, cin).numpy()
        assert (np.abs(want - auto) <= 2.0 ** -40 * S + 1e-300).all(), (form, geom, float(np.abs(want - auto).max()))
        if f.get("nchw"):                                  # the same sums from the NHWC copy of the image
            again, s2 = _reference(du, x.permute(0, 2, 3, 1).contiguous(), imgs, H, W, f["ks"], f["stride"], f["pad"])
            assert np.array_equal(again, want) and np.array_equal(s2, S)


def test_bound_relations():
    """what the module docstring says of the two fp32 bounds, at every map of this file: the split's per-product error is inside the header's
    2^-16; the judge's fp32 factor is never above the documented 2^-14 nor above the derived worst case; the derived worst case alone
    exceeds 2^-14 at all of them (which is why the smaller is taken); and the bf16 factor counts at least one addition per pixel"""
    assert 3 * 2.0 ** -18 * (1 + 2.0 ** -9) < 2.0 ** -16
    for f in FORMS.values():
        for imgs, H, W in f["maps"]:
            m = imgs * H * W
            a = _additions(m)
            assert a >= m + (m + 511) // 512 + 1 and a >= m + (m + 255) // 256 + 1          # pixels + partials + the add into dw
            assert a >= m + imgs * ((H + 7) // 8) * ((W + 7) // 8) + 1                       # ly_wgrad3: at most one partial per 8 x 8 tile
            derived = 2.0 ** -16 + 3 * a * 2.0 ** -24
            for t in (1, 2):
                used = (_a_eff(m, True, t) - (t - 1)) * 2.0 ** -24
                assert used <= 2.0 ** -14 and used <= derived
            assert derived > 2.0 ** -14
            assert _a_eff(m, False, 2) == a + 1


def _float32_permuted(form, n, cin, dtype, geom):
    """the sums of the reference evaluated in float32 over a permuted pixel order"""
    f = FORMS[form]
    imgs, H, W = geom
    du, x, want, S = _problem(form, n, cin, dtype, geom)
    xn = (x.permute(0, 2, 3, 1) if f.get("nchw") else x).double()
    if f.get("up2"):
        xn = xn.repeat_interleave(2, 1).repeat_interleave(2, 2)
    Hv, Wv = xn.shape[1], xn.shape[2]
    perm = torch.randperm(imgs * H * W, generator=torch.Generator().manual_seed(3))
    img, ho, wo = perm // (H * W), (perm // W) % H, perm % W
    got = np.zeros_like(want)
    for tap in range(f["ks"] ** 2):
        ky, kx = divmod(tap, f["ks"])
        hi, wi = ho * f["stride"] + ky - f["pad"], wo * f["stride"] + kx - f["pad"]
        ok = (hi >= 0) & (hi < Hv) & (wi >= 0) & (wi < Wv)
        xt = xn[img, hi.clamp(0, Hv - 1), wi.clamp(0, Wv - 1)] * ok[:, None]
        got[:, tap] = (du[perm].float().t() @ xt.float()).numpy()
    return got, want, S


@pytest.mark.parametrize("form", list(FORMS))
def test_judge_accepts_float32_sums_in_another_pixel_order(form):
    for geom in FORMS[form]["maps"]:
        m = geom[0] * geom[1] * geom[2]
        for dtype in DTYPES:
            got, want, S = _float32_permuted(form, 24, 16 if form != "k4nchw" else 3, dtype, geom)
            bad = _judge(got, want, S, _a_eff(m, dtype == "f32"), f"{form} {dtype} {geom}")
            assert bad is None, bad


@pytest.mark.parametrize("form,mutate", [("k3s1", "nowrap"), ("k3s1", "droplast"), ("k3s1", "shift"), ("k3s2o", "shift"), ("k2s2", "droplast"),
                                         ("up2", "parity"), ("up2", "droplast"), ("k4nchw", "swap"), ("k4nchw", "droplast"), ("rows", "droplast")])
def test_judge_rejects_wrong_gathers(form, mutate):
    """at every map, with the bf16 and with the fp32 bound: (a) the left zero padding replaced by the previous row's last pixel, (b) the last
    pixel of an image dropped, (c) one tap shifted by a pixel, (d) the upsampled read with the wrong parity, (e) channel and row strides of
    the NCHW image swapped.  Each moves a few border terms out of hundreds; a bound that lets one through is too loose for its map."""
    f = FORMS[form]
    n, cin = 24, 16 if form != "k4nchw" else 3
    for geom in f["maps"]:
        imgs, H, W = geom
        m = imgs * H * W
        for dtype in DTYPES:
            du, x, want, S = _problem(form, n, cin, dtype, geom)
            wrong, _ = _reference(du, x, imgs, H, W, mutate=mutate, **_gather(form))
            assert _judge(wrong, want, S, _a_eff(m, dtype == "f32", 2)) is not None, (form, mutate, geom, dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases: a problem inside poisoned surroundings, and the kernel it has to run on
# ---------------------------------------------------------------------------------------------------------------------------------------
PRE, POST = 8, 5                 # spare NaN rows before / after du and x (8 rows keep the first row's alignment), spare rows around dw: 2 / 2
DU, X, DW, WS = 0x10000000, 0x20000000, 0x30000000, 0x40000000      # 256-byte aligned placeholder addresses of the host description


class _Case:
    """One problem of a form.  du and x are column slices [off, off + N) / [off, off + Cin) of wider buffers with spare rows before and
    after, NaN everywhere outside the slices (an NCHW image: NaN guard planes before and after); dw is a slice (column dw_off, dw_pad spare
    columns, spare rows) of a wider fp32 tensor of random values, which must come back bit-identical outside rows < n_valid and the
    (tap, c < c_valid) positions.  `kernel`: what ly_wgrad_describe must say for it, `w3`: the ly_tune_wgrad3 setting it runs under."""

    def __init__(self, name, form, n, cin, dtype, kernel, w3=1, layouts=("packed", "torch"), du_off=8, du_pad=8, x_off=8, x_pad=8, dw_off=8, dw_pad=8,
                 n_valid=None, c_valid=None, lddw=None):
        self.name, self.form, self.n, self.cin, self.dtype, self.kernel, self.w3 = name, form, n, cin, dtype, kernel, w3
        self.f = FORMS[form]
        self.taps = self.f["ks"] ** 2
        self.layouts = layouts if self.taps > 1 else ("packed",)              # one tap: the two layouts are the same
        self.du_off, self.x_off, self.dw_off = du_off, x_off, dw_off
        self.lddu, self.ldx = du_off + n + du_pad, x_off + cin + x_pad
        self.lddw = lddw or dw_off + self.taps * cin + dw_pad
        self.n_valid, self.c_valid = n_valid or n, c_valid or cin
        self.maps = self.f["maps"]
        self.nchw = bool(self.f.get("nchw"))
        self.family = "ly_wgrad3" if kernel == "ly_wgrad3_kernel" else "tiled" if "tiled" in kernel else "per-lane"

    def __repr__(self):
        return self.name

    def q(self, geom, layout):
        """the integer arguments of ops.wgrad"""
        imgs, H, W = geom
        Hin, Win = self.f["src"](H), self.f["src"](W)
        ts, cs = (self.cin, 1) if layout == "packed" else (1, self.taps)
        x_off = Hin * Win if self.nchw else PRE * self.ldx + self.x_off
        return dict(M=imgs * H * W, H=H, W=W, N=self.n, lddu=self.lddu, ldx=0 if self.nchw else self.ldx, Hin=Hin, Win=Win, Cin=self.cin,
                    lddw=self.lddw, du_off=PRE * self.lddu + self.du_off, x_off=x_off, dw_off=2 * self.lddw + self.dw_off, dw_ts=ts, dw_cs=cs,
                    n_valid=self.n_valid, c_valid=self.c_valid, **_gather(self.form))

    def host_params(self, geom, layout, ws=True):
        """LyWgradParams with placeholder addresses of the alignment the device buffers have (ly_wgrad_describe dereferences none)"""
        from lead_yolo_amd import capi, ops
        q = self.q(geom, layout)
        es = 2 if self.dtype == "bf16" else 4
        return capi.LyWgradParams(M=q["M"], H=q["H"], W=q["W"], N=q["N"], du=DU + es * q["du_off"], lddu=q["lddu"], x=X + es * q["x_off"], ldx=q["ldx"],
                                  Hin=q["Hin"], Win=q["Win"], Cin=q["Cin"], ks=q["ks"], stride=q["stride"], pad=q["pad"], nchw=int(q["nchw"]),
                                  up2=int(q["up2"]), dw=DW + 4 * q["dw_off"], lddw=q["lddw"], dtype=capi.LY_BF16 if self.dtype == "bf16" else capi.LY_F32,
                                  dw_ts=q["dw_ts"], dw_cs=q["dw_cs"], n_valid=q["n_valid"], c_valid=q["c_valid"], x_scale=None, x_shift=None,
                                  ws=WS if ws else None, ws_floats=ops.WGRAD_WS_FLOATS if ws else 0)

    def buffers(self, geom):
        """(du buffer, x buffer) on the device"""
        du, x, _, _ = _problem(self.form, self.n, self.cin, self.dtype, geom)
        dub = torch.full((PRE + du.shape[0] + POST, self.lddu), NAN, dtype=du.dtype)
        dub[PRE:PRE + du.shape[0], self.du_off:self.du_off + self.n] = du
        if self.nchw:
            plane = x.shape[2] * x.shape[3]
            xb = torch.full((x.numel() + 2 * plane,), NAN, dtype=x.dtype)
            xb[plane:plane + x.numel()] = x.reshape(-1)
        else:
            rows = x.numel() // self.cin
            xb = torch.full((PRE + rows + POST, self.ldx), NAN, dtype=x.dtype)
            xb[PRE:PRE + rows, self.x_off:self.x_off + self.cin] = x.reshape(rows, self.cin)
        return dub.to(_dev()), xb.to(_dev())

    def base(self, geom, layout):
        g = torch.Generator().manual_seed(zlib.crc32(repr((self.name, geom, layout)).encode()))
        return torch.randn(2 + self.n + 2, self.lddw, generator=g)

    def check(self, dw, base, geom, layout, what, times=1):
        """the untouched surroundings and the judge; returns the worst |got - want| / bound"""
        _, _, want, S = _problem(self.form, self.n, self.cin, self.dtype, geom)
        q = self.q(geom, layout)
        nv, cv = self.n_valid, self.c_valid
        pos = (q["dw_off"] + np.arange(nv)[:, None, None] * self.lddw + np.arange(self.taps)[None, :, None] * q["dw_ts"]
               + np.arange(cv)[None, None, :] * q["dw_cs"])
        got, was = dw.cpu().numpy().reshape(-1), base.numpy().reshape(-1)
        inside = np.zeros(got.shape, dtype=bool)
        inside[pos] = True
        assert int(inside.sum()) == pos.size
        assert np.array_equal(got[~inside].view(np.uint32), was[~inside].view(np.uint32)), f"{what}: dw was written outside its valid part"
        b = was[pos].astype(np.float64)
        total, s = b + times * want[:nv, :, :cv], np.abs(b) + times * S[:nv, :, :cv]
        a = _a_eff(q["M"], self.dtype == "f32", times)
        bad = _judge(got[pos], total, s, a, what)
        assert bad is None, bad
        return float((np.abs(got[pos].astype(np.float64) - total) / (a * 2.0 ** -24 * s)).max())


def _tiled(dtype, bn, bk, octets=False):
    return f"ly_wgrad_tiled_kernel<{TNAME[dtype]}, {bn}, {bk}, {128 if dtype == 'bf16' else 64}, false, false, {'true' if octets else 'false'}>"


def _lane(dtype, rows):
    return f"ly_wgrad_kernel<{TNAME[dtype]}, {'true' if rows else 'false'}>"


QUAD = dict(du_off=4, du_pad=4, x_off=4, x_pad=4)             # widths and offsets in whole quads that are no whole octets
PARTIAL = dict(n_valid=6, c_valid=6, dw_off=0, dw_pad=0, lddw=54, layouts=("torch",))      # lddu = ldx = 24 from the default offsets
TORCH48 = dict(dw_off=0, dw_pad=0, layouts=("torch",))        # PatchEmbed: lddw = 3 * 16
CASES = []


def _add(name, *args, **kw):
    CASES.append(_Case(name, *args, **kw))


# 3x3 / stride 1 / pad 1.  Tile classes through N and Ktot = 9 Cin: 32 x 128, 64 x 64, 128 x 128, 128 x 128 with two N tiles.
for _n, _c, _bn, _bk in [(24, 16, 32, 128), (64, 4, 64, 64), (72, 40, 128, 128), (136, 32, 128, 128)]:
    _add(f"k3s1-f32-{_n}x{_c}", "k3s1", _n, _c, "f32", _tiled("f32", _bn, _bk))
    # ly_tune_wgrad3(0): octet staging where N, Cin and the widths are whole octets (Cin = 4 is not)
    _add(f"k3s1-bf16-tiled-{_n}x{_c}", "k3s1", _n, _c, "bf16", _tiled("bf16", _bn, _bk, _c % 8 == 0), w3=0)
for _n, _c in [(24, 12), (20, 36)]:                           # quads only: not ly_wgrad3_ok either, the switch does not matter
    _add(f"k3s1-bf16-quads-{_n}x{_c}", "k3s1", _n, _c, "bf16", _tiled("bf16", 32, 128), w3=0, **QUAD)
for _n, _c in [(24, 16), (72, 40), (200, 32)]:
    _add(f"k3s1-bf16-wgrad3-{_n}x{_c}", "k3s1", _n, _c, "bf16", "ly_wgrad3_kernel")
# the MLPBlock's partial conv: 6 valid of 8 padded channels on both sides, the weight in torch's own layout
_add("k3s1-f32-partial", "k3s1", 8, 8, "f32", _tiled("f32", 32, 128), **PARTIAL)
_add("k3s1-bf16-tiled-partial", "k3s1", 8, 8, "bf16", _tiled("bf16", 32, 128, True), w3=0, **PARTIAL)
_add("k3s1-bf16-wgrad3-partial", "k3s1", 8, 8, "bf16", "ly_wgrad3_kernel", **PARTIAL)
# 3x3 / stride 2 / pad 1 on odd and even inputs (the header's contract; no module uses it)
for _form in ("k3s2o", "k3s2e"):
    _add(f"{_form}-f32-40x24", _form, 40, 24, "f32", _tiled("f32", 64, 128))
    _add(f"{_form}-bf16-40x24", _form, 40, 24, "bf16", _tiled("bf16", 64, 128, True))
# 2x2 / stride 2 (PatchMerging)
for _n, _c, _bn in [(40, 24, 64), (136, 8, 128)]:
    _add(f"k2s2-f32-{_n}x{_c}", "k2s2", _n, _c, "f32", _tiled("f32", _bn, 128))
    _add(f"k2s2-bf16-{_n}x{_c}", "k2s2", _n, _c, "bf16", _tiled("bf16", _bn, 128, True))
# 1x1 behind nn.Upsample: x dense, and once as a column slice of a wider map
for _n, _c, _bn, _bk in [(24, 40, 64, 64), (136, 72, 128, 128)]:               # N and Ktot = Cin both <= 64: the 64 x 64 tile
    _add(f"up2-f32-{_n}x{_c}", "up2", _n, _c, "f32", _tiled("f32", _bn, _bk), x_off=0, x_pad=0)
    _add(f"up2-bf16-{_n}x{_c}", "up2", _n, _c, "bf16", _tiled("bf16", _bn, _bk, True), x_off=0, x_pad=0)
_add("up2-bf16-24x40-x-slice", "up2", 24, 40, "bf16", _tiled("bf16", 64, 64, True), x_off=16, x_pad=8)
# 4x4 / stride 4 of an NCHW image (PatchEmbed on a float image): the per-lane kernel
for _n in (16, 24):
    _add(f"k4nchw-f32-{_n}x3", "k4nchw", _n, 3, "f32", _lane("f32", False), **TORCH48)
    _add(f"k4nchw-bf16-{_n}x3", "k4nchw", _n, 3, "bf16", _lane("bf16", False), **TORCH48)
# plain rows that are not vector-friendly: N no multiple of 4 (lddu = N = 18), an odd element offset on rows of odd width (lddu = 27)
for _dt in ("f32", "bf16"):
    _add(f"rows-{_dt}-18x20", "rows", 18, 20, _dt, _lane(_dt, True), du_off=0, du_pad=0)
    _add(f"rows-{_dt}-24x128-odd", "rows", 24, 128, _dt, _lane(_dt, True), du_off=1, du_pad=2)


def _describe(p):
    from lead_yolo_amd import capi
    name = ctypes.create_string_buffer(128)
    rc = capi.lib().ly_wgrad_describe(ctypes.byref(p), 1, name, 128)
    return rc, name.value.decode()


def _switched(case, fn):
    """fn() under the case's ly_tune_wgrad3 setting"""
    from lead_yolo_amd import capi
    was = capi.lib().ly_tune_wgrad3(case.w3)
    try:
        return fn()
    finally:
        capi.lib().ly_tune_wgrad3(was)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_cases_run_on_the_kernels_they_name(case):
    """no device: at every map and dw layout the launch plan puts the case on the kernel written next to it in CASES (family and template
    flags), with and without the scratch"""
    def run():
        for geom in case.maps:
            for layout in case.layouts:
                for ws in (True, False):
                    assert _describe(case.host_params(geom, layout, ws)) == (0, case.kernel), (case, geom, layout, ws)
    _switched(case, run)


def test_case_strides():
    """the strides the modules use: the partial conv reads 8 of 24 columns and writes 6 x 9 weights per row; PatchEmbed's weight rows are
    3 x 16; the per-lane rows cases are N = lddu = 18 and an odd offset on rows of odd width"""
    by = {c.name: c for c in CASES}
    for name in ("k3s1-f32-partial", "k3s1-bf16-tiled-partial", "k3s1-bf16-wgrad3-partial"):
        assert (by[name].lddu, by[name].ldx, by[name].lddw, by[name].layouts) == (24, 24, 54, ("torch",))
    assert all(c.lddw == 48 and c.layouts == ("torch",) for c in CASES if c.form == "k4nchw")
    assert by["rows-bf16-18x20"].lddu == 18
    q = by["rows-f32-24x128-odd"].q(ROW_MAPS[0], "packed")
    assert q["lddu"] % 2 == 1 and q["du_off"] % 2 == 1
    for c in CASES:                                          # octet cases sit on octet boundaries, quad cases on quad boundaries only
        if c.family == "tiled" and c.kernel.endswith("true>"):
            assert all(v % 8 == 0 for v in (c.lddu, c.ldx, c.du_off, c.x_off))
        if "quads" in c.name:
            assert all(v % 4 == 0 for v in (c.lddu, c.ldx, c.du_off, c.x_off)) and c.du_off % 8 and c.x_off % 8


# ---------------------------------------------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------------------------------------------
def _launch(case, geom, layout, bufs, dw):
    from lead_yolo_amd import ops
    ops.wgrad(dw=dw, du=bufs[0], x=bufs[1], _now=True, **case.q(geom, layout))


def _report(case, flush, ratio):
    print(f"\nwgrad-forms ratio: {case.form} {case.dtype} {case.family} {flush} {case.name} {ratio:.4f}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_wgrad_form_against_float64(case):
    """at every map and dw layout of the case, with the default scratch: (i) the judge, (ii) the untouched surroundings, (iii) the call made
    twice onto the random base, (iv) two runs from the same state give the same bits — for the tiled kernels and ly_wgrad3, whose partial
    tiles go through the slab and its fixed-order fold (one chunk: one add per element).  The per-lane kernel adds its chunks with float
    atomics and is exempt from (iv)."""
    from lead_yolo_amd import ops

    def run():
        worst = 0.0
        for geom in case.maps:
            bufs = case.buffers(geom)
            for layout in case.layouts:
                what = f"{case} {geom} {layout}"
                assert ops._wgrad_params(dw=bufs[0], du=bufs[0], x=bufs[1], **case.q(geom, layout)).ws is not None
                base = case.base(geom, layout)
                outs = []
                for i in range(2):
                    dw = base.clone().to(_dev())
                    _launch(case, geom, layout, bufs, dw)
                    if i == 0:
                        once = dw.clone()
                    _launch(case, geom, layout, bufs, dw)
                    outs.append(dw)
                worst = max(worst, case.check(once, base, geom, layout, what), case.check(outs[0], base, geom, layout, what + " twice", times=2))
                if case.family != "per-lane":
                    assert torch.equal(outs[0], outs[1]), f"{what}: two runs from the same state differ"
        return worst
    _report(case, "atomic" if case.family == "per-lane" else "slab", _switched(case, run))


def _several_chunks(case, geom):
    imgs, H, W = geom
    if case.family == "ly_wgrad3":                           # chunks of whole 8 x 8 tiles
        return imgs * ((H + 7) // 8) * ((W + 7) // 8) > 1
    return imgs * H * W > 512                                # the tiled kernels: no chunk below 512 pixels


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c.family != "per-lane"], ids=repr)
def test_wgrad_form_with_the_atomic_flush(case, monkeypatch):
    """the maps of several chunks without scratch (ops.WGRAD_WS_FLOATS = 0, as on the first use inside a graph capture): every chunk adds
    its tile to dw with float atomics.  Judge, surroundings and the doubled call as with the slab; the order of the atomics is not fixed,
    so neither bit equality between runs nor with the slab form is asked."""
    from lead_yolo_amd import ops
    monkeypatch.setattr(ops, "WGRAD_WS_FLOATS", 0)
    monkeypatch.setattr(ops, "_WGRAD_WS", {})

    def run():
        worst = 0.0
        for geom in [g for g in case.maps if _several_chunks(case, g)]:
            bufs = case.buffers(geom)
            for layout in case.layouts:
                what = f"{case} {geom} {layout} atomic"
                p = ops._wgrad_params(dw=bufs[0], du=bufs[0], x=bufs[1], **case.q(geom, layout))
                assert p.ws is None and p.ws_floats == 0
                base = case.base(geom, layout)
                dw = base.clone().to(_dev())
                _launch(case, geom, layout, bufs, dw)
                worst = max(worst, case.check(dw, base, geom, layout, what))
                _launch(case, geom, layout, bufs, dw)
                worst = max(worst, case.check(dw, base, geom, layout, what + " twice", times=2))
        assert worst > 0.0
        return worst
    _report(case, "atomic", _switched(case, run))
    assert not ops._WGRAD_WS
