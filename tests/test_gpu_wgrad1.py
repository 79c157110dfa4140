"""The bf16 plain-row 1x1 weight gradient  dw[n][c] += sum_p du[p][n] * x[p][c]  of csrc/ly_wgrad1.hip ([pixel][channel] LDS tiles, transposed
fragment reads) and, through the same cases, the register-transposing kernel it replaces (ly_tune_wgrad1(0)), against float64.

The judge is derived, not tuned.  A product of two bf16 values is exact in fp32, so the only error of either kernel is fp32 summation: every
addition on the way to an element rounds by at most 2^-24 of a partial sum, and no partial sum exceeds S = sum_p |du[p][n] * x[p][c]|.  With A
additions on the longest path,
        |got - want| <= A * 2^-24 * S            per element, want and S computed in float64 from the inputs.
A = pixels a chunk contracts (the MFMA k-depth, 32, times its MFMAs: the chunk's pixels rounded up to whole steps of at most 128)
    + chunks (the fold of the partial tiles; a launch makes at most ceil(M / 512)) + 1 (the add into dw).
The chunk is bounded by the whole run, so A = ceil128(M) + ceil(M / 512) + 1 holds for every launch form of both kernels."""
import numpy as np
import pytest
import torch

from tests.test_gpu_modules import _dev

NAN = float("nan")
GEOM = {40: (1, 5, 8), 64: (1, 8, 8), 72: (1, 8, 9), 136: (1, 8, 17), 480: (1, 20, 24), 960: (2, 20, 24), 1440: (3, 20, 24)}      # M -> (images, H, W)


def _additions(m):
    return (m + 127) // 128 * 128 + (m + 511) // 512 + 1


def _ref(du, x):
    """(want, S) in float64 from [M, N] and [M, C] tensors"""
    d, v = du.double(), x.double()
    return (d.t() @ v).numpy(), (d.abs().t() @ v.abs()).numpy()


def _judge(got, want, s, a, what=""):
    """None when every element is within a * 2^-24 * s of want, else a description of the worst one"""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != want.shape:
        return f"{what}: shape {got.shape} vs {want.shape}"
    if not np.isfinite(got).all():
        return f"{what}: {int((~np.isfinite(got)).sum())} values are not finite"
    bound = a * 2.0 ** -24 * s
    over = np.abs(got - want) - bound
    i = np.unravel_index(int(np.argmax(over)), over.shape)
    if over[i] > 0:
        return f"{what}: element {i} is off by {abs(got[i] - want[i]):.3e}, bound {bound[i]:.3e} (A = {a})"
    return None


def _inputs(m, n, c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(m, n, generator=g).bfloat16(), torch.randn(m, c, generator=g).bfloat16()


def test_judge_accepts_reordered_sums_and_rejects_lost_or_misplaced_data():
    """the judge itself, on the host: a float32 product summed in another pixel order passes; one pixel row dropped, or one 8-channel piece
    taken from its neighbour, does not"""
    m, n, c = 1440, 72, 200
    du, x = _inputs(m, n, c, 1)
    want, s = _ref(du, x)
    a = _additions(m)
    perm = torch.randperm(m, generator=torch.Generator().manual_seed(2))
    assert _judge((du[perm].float().t() @ x[perm].float()).numpy(), want, s, a) is None
    assert _judge((du.float().t() @ x.float()).numpy(), want, s, a) is None
    dropped = want - np.outer(du[m - 1].double().numpy(), x[m - 1].double().numpy())
    assert _judge(dropped, want, s, a) is not None
    xs = x.clone()
    xs[:, 16:24] = x[:, 24:32]
    assert _judge(_ref(du, xs)[0], want, s, a) is not None
    bad = want.copy()
    bad[3, 5] = np.inf
    assert _judge(bad, want, s, a) is not None


class _Case:
    """One problem with poisoned surroundings: du and x are column slices of wider buffers with spare rows, dw a slice of a wider gradient.
    Everything outside the slices is NaN in the inputs; dw holds `base` (zeros unless given) and must stay as it was outside its valid part."""

    def __init__(self, m, n, c, seed, du_off=8, du_pad=16, x_off=16, x_pad=8, dw_off=0, dw_pad=0, n_valid=None, c_valid=None, base=False):
        dev = _dev()
        self.m, self.n, self.c = m, n, c
        self.n_valid, self.c_valid = n_valid or n, c_valid or c
        self.du, self.x = _inputs(m, n, c, seed)
        self.want, self.s = _ref(self.du[:, :self.n_valid], self.x[:, :self.c_valid])
        lddu, ldx, self.lddw = du_off + n + du_pad, x_off + c + x_pad, dw_off + c + dw_pad
        dub = torch.full((m + 70, lddu), NAN, dtype=torch.bfloat16)
        dub[:m, du_off:du_off + n] = self.du
        xb = torch.full((m + 70, ldx), NAN, dtype=torch.bfloat16)
        xb[:m, x_off:x_off + c] = self.x
        g = torch.Generator().manual_seed(seed + 100)
        self.base = torch.randn(n, self.lddw, generator=g) if base else torch.zeros(n, self.lddw)
        self.dw_off = dw_off
        imgs, h, w = GEOM[m]
        self.dub, self.xb = dub.to(dev), xb.to(dev)
        self.q = dict(M=m, H=h, W=w, N=n, du=self.dub, lddu=lddu, du_off=du_off, x=self.xb, ldx=ldx, x_off=x_off, Hin=h, Win=w, Cin=c,
                      lddw=self.lddw, dw_off=dw_off, n_valid=self.n_valid, c_valid=self.c_valid)

    def fresh(self):
        return self.base.clone().to(_dev())

    def check(self, dw, what, times=1):
        got = dw.cpu().double().numpy()
        base = self.base.double().numpy()
        o, nv, cv = self.dw_off, self.n_valid, self.c_valid
        inside = np.zeros_like(base, dtype=bool)
        inside[:nv, o:o + cv] = True
        assert np.array_equal(got[~inside], base[~inside]), f"{what}: dw was written outside its valid part"
        want = base[:nv, o:o + cv] + times * self.want
        s = np.abs(base[:nv, o:o + cv]) + times * self.s
        bad = _judge(got[:nv, o:o + cv], want, s, _additions(self.m) + times - 1, what)
        assert bad is None, bad


def _both_kernels(run):
    """run(label) with the new kernel, then with ly_tune_wgrad1(0): the old kernel passes the same judge, or the bound is wrong.  What run
    returns (gradients) is the same bits from both: the new kernel keeps the old one's chunks, k-steps and operand positions (w1_row in
    csrc/ly_wgrad1.hip), so switching it on changed no result of the training step."""
    import lead_yolo_amd as L
    was = L.ops.tune_wgrad1(1)
    try:
        new = run("wgrad1")
        L.ops.tune_wgrad1(0)
        old = run("tiled")
    finally:
        L.ops.tune_wgrad1(was)
    for i, (a, b) in enumerate(zip(new or [], old or [])):
        assert torch.equal(a, b), f"result {i}: the two kernels differ in {int((a != b).sum())} elements"


SHAPES = [(24, 128), (40, 72), (64, 64), (72, 200), (136, 8), (256, 136), (20, 36)]      # every tile class, ragged channel tiles; (20, 36): not eligible


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_wgrad1_tile_classes_and_ragged_pixel_runs(shape):
    """every tile class x pixel runs of less than a step, one step, a step + 8, a 128-pixel step + 8 and three chunks (slab + fold), inside
    NaN-poisoned buffers"""
    import lead_yolo_amd as L
    n, c = shape
    wide = n % 8 == 0                                 # (20, 36): quads only, no room for 8-aligned slices: plain buffers
    for m in (40, 64, 72, 136, 1440):
        case = _Case(m, n, c, seed=m + n, **({} if wide else dict(du_off=4, du_pad=4, x_off=4, x_pad=4)))

        def run(label):
            dw = case.fresh()
            L.ops.wgrad(dw=dw, _now=True, **case.q)
            case.check(dw, f"{label} M={m} N={n} Cin={c}")
            return [dw]
        _both_kernels(run)


@pytest.mark.gpu
def test_wgrad_profile_records_carry_the_described_kernel(monkeypatch):
    """with ops.PROFILE recording, ops.wgrad labels its record with what ly_wgrad_describe says for the parameters it launches (the offsets
    folded into the pointers), for an eligible and an ineligible shape; the results are the unprofiled ones' judge"""
    import ctypes
    import lead_yolo_amd as L
    monkeypatch.setattr(L.ops, "PROFILE", [])
    want = []
    for (n, c), name in [(SHAPES[0], "ly_wgrad1_kernel<32, 128, true>"), (SHAPES[-1], "ly_wgrad_tiled_kernel<__bf16, 64, 64, 128, true, false, false>")]:
        case = _Case(1440, n, c, seed=5, **({} if n % 8 == 0 else dict(du_off=4, du_pad=4, x_off=4, x_pad=4)))
        dw = case.fresh()
        L.ops.wgrad(dw=dw, _now=True, **case.q)
        case.check(dw, f"profiled M=1440 N={n} Cin={c}")
        buf = ctypes.create_string_buffer(128)
        assert L.capi.lib().ly_wgrad_describe(ctypes.byref(L.ops._wgrad_params(dw=dw, **case.q)), 1, buf, len(buf)) == 0
        assert buf.value.decode() == name
        want.append(name)
    assert [rec[0] for rec in L.ops.PROFILE] == want


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(du_off=16, du_pad=40, x_off=0, x_pad=0), dict(du_off=0, du_pad=0, x_off=24, x_pad=16),
                                dict(dw_off=40, dw_pad=0), dict(dw_off=8, dw_pad=24, n_valid=18), dict(c_valid=100), dict(n_valid=18, c_valid=3)],
                         ids=["du-slice", "x-slice", "concat-second-source", "n_valid", "c_valid", "both-valid"])
def test_wgrad1_strides_offsets_and_valid_parts(kw):
    """du / x as column slices of wider tensors, dw as the second source's columns of a concat's weight, n_valid < N, c_valid < Cin"""
    import lead_yolo_amd as L
    for m in (72, 1440):
        case = _Case(m, 24, 128, seed=7, **kw)

        def run(label):
            dw = case.fresh()
            L.ops.wgrad(dw=dw, _now=True, **case.q)
            case.check(dw, f"{label} M={m} {kw}")
            return [dw]
        _both_kernels(run)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(24, 128), (256, 136)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_wgrad1_accumulates_and_repeats_bit_for_bit(shape):
    """dw pre-filled and the call made twice: base + 2 x gradient; the same two calls from the same state give the same bits"""
    import lead_yolo_amd as L
    n, c = shape
    for m in (72, 1440):
        case = _Case(m, n, c, seed=11, base=True)

        def run(label):
            outs = []
            for _ in range(2):
                dw = case.fresh()
                L.ops.wgrad(dw=dw, _now=True, **case.q)
                L.ops.wgrad(dw=dw, _now=True, **case.q)
                outs.append(dw)
            case.check(outs[0], f"{label} M={m} twice", times=2)
            assert torch.equal(outs[0], outs[1]), f"{label} M={m}: two runs from the same state differ"
            return outs[:1]
        _both_kernels(run)


@pytest.mark.gpu
@pytest.mark.parametrize("members", [[(1440, 256, 136), (480, 72, 200), (960, 136, 8), (136, 128, 128)], [(1440, 256, 136), (480, 76, 200), (960, 136, 8)]],
                         ids=["eligible", "one-member-not-eligible"])
def test_wgrad1_groups(members):
    """four problems of different M, N, Cin in one launch (one of them with several output tiles) against separate launches and float64;
    with a member whose N is no multiple of 8 the whole group takes the old grouped kernel and is still right"""
    import lead_yolo_amd as L
    cases = [_Case(m, n, c, seed=20 + i, **({} if n % 8 == 0 else dict(du_off=4, du_pad=4))) for i, (m, n, c) in enumerate(members)]

    def run(label):
        grouped = [k.fresh() for k in cases]
        L.ops.wgrad_group([dict(k.q, dw=dw) for k, dw in zip(cases, grouped)], _now=True)
        again = [k.fresh() for k in cases]
        L.ops.wgrad_group([dict(k.q, dw=dw) for k, dw in zip(cases, again)], _now=True)
        alones = []
        for i, (k, dw, dw2) in enumerate(zip(cases, grouped, again)):
            k.check(dw, f"{label} group member {i}")
            assert torch.equal(dw, dw2), f"{label} group member {i}: two launches differ"
            alones.append(k.fresh())
            L.ops.wgrad(dw=alones[-1], _now=True, **k.q)
            k.check(alones[-1], f"{label} member {i} alone")
        return grouped + alones
    _both_kernels(run)
