"""What do the host packers write?  Every packed weight image against a plain restatement of its documented index map, bit for bit.

Every contraction reads its weights from a packed image (pack.frag_pack3 and the descriptor map of ly_pack_table, pack.rfcbam_gen_weights,
pack.rfcbam_gen_weights_c, pack.rf3m_stream), never from the parameter.  The module tests see those images only through outputs at
1e-3-class budgets: a zero lo plane, a dropped shift term or a descriptor that is right only at the model's shapes stays inside them.
Here every element of every image is compared with a reference written as loops from the index maps stated in include/lead_yolo_hip.h,
pack.py's docstrings, csrc/ly_tile.hpp and csrc/ly_rfcbam_att.hip (ly_gw_index).  The references share no code with pack.py: bf16 rounding
is restated on the bits (round to nearest even), gathers are `for` loops, and no view / permute chain of pack.py is repeated.

tests/test_gpu_pack.py holds the device kernels to these host packers; `emulate` (the LyPackDesc formula) is shared with it."""
import numpy as np
import pytest
import torch

from lead_yolo_amd import pack


# ---- bf16 on the bits ---------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """float32 array -> bf16 bit patterns (uint16), round to nearest even; finite inputs"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_val(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def _bits(t):
    """int16 / bf16 torch tensor -> uint16 numpy"""
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return t.cpu().numpy().view(np.uint16)


def _rand(shape, seed, lo=-20, hi=20):
    """finite fp32 values of both signs with magnitudes in [2^lo, 2^hi), all 24 mantissa bits in use, no zero"""
    rng = np.random.default_rng(seed)
    m = 1.0 + rng.random(shape)
    e = rng.integers(lo, hi, shape)
    s = rng.choice([-1.0, 1.0], shape)
    return (s * m * np.exp2(e)).astype(np.float32)


# ---- frag_pack3 ---------------------------------------------------------------------------------------------------------------------
def ref_frag_pack3(w, rows_to=0, planes=2):
    """[T][S][planes][64][8] bf16 bits: lane, j hold row 16t + (lane & 15), k = 32s + 16(j >> 2) + 4(lane >> 4) + (j & 3)"""
    R, K = w.shape
    T, S = (max(R, rows_to) + 15) // 16, (K + 31) // 32
    vals = np.zeros((T, S, 64, 8), dtype=np.float32)
    for t in range(T):
        for s in range(S):
            for lane in range(64):
                for j in range(8):
                    r, k = 16 * t + (lane & 15), 32 * s + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3)
                    if r < R and k < K:
                        vals[t, s, lane, j] = w[r, k]
    hi = bf16_bits(vals)
    out = np.zeros((T, S, planes, 64, 8), dtype=np.uint16)
    out[:, :, 0] = hi
    if planes == 2:
        out[:, :, 1] = bf16_bits(vals - bf16_val(hi))
    return out, vals


TIES = (1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 2.0 ** -20, 2.0 ** 19, 0.5, -4.0, 1.0, 1 + 2.0 ** -7 + 2.0 ** -8)


def pack3_matrix(R, K, seed):
    w = _rand((R, K), seed)
    flat = w.reshape(-1)
    n = min(len(TIES), flat.size)
    flat[:n] = TIES[:n]                                    # exact ties of the bf16 rounding and powers of two
    return w


PACK3_SHAPES = ((19, 37, 33), (1, 4, 0), (16, 32, 0), (33, 100, 0))          # (R, K, rows_to)


@pytest.mark.parametrize("planes", (1, 2))
@pytest.mark.parametrize("R,K,rows_to", PACK3_SHAPES)
def test_frag_pack3_every_element(R, K, rows_to, planes):
    """pack.frag_pack3 (CPU path): every (t, s, plane, lane, j) holds bf16(W) / bf16(W - hi) of the documented (row, k), zeros outside
    the matrix; hi + lo is within 2^-16 |w| of w (bf16 unit roundoff 2^-8, applied twice).
    Contract: finite values with magnitudes in [2^-20, 2^20] and no -0.0; what the split does with denormals or on overflow is not
    part of it and not tested."""
    w = pack3_matrix(R, K, 100 + R)
    got = pack.frag_pack3(torch.from_numpy(w), rows_to=rows_to, planes=planes)
    want, vals = ref_frag_pack3(w, rows_to, planes)
    assert got.dtype == torch.int16 and tuple(got.shape) == want.shape
    g = _bits(got)
    bad = np.argwhere(g != want)
    assert bad.size == 0, f"first differing (t, s, plane, lane, j): {bad[:4].tolist()}"
    if planes == 2:
        full = bf16_val(g[:, :, 0]).astype(np.float64) + bf16_val(g[:, :, 1]).astype(np.float64)
        err = np.abs(full - vals.astype(np.float64))
        assert np.all(err <= 2.0 ** -16 * np.abs(vals.astype(np.float64)))
        assert np.any(g[:, :, 1] != 0)                    # the lo plane carries something
    else:
        assert np.array_equal(g[:, :, 0], want[:, :, 0])


def test_frag_pack3_ties_round_to_even():
    """the reference's own rounding on the exact ties: 1 + 2^-8 -> 1 (lo = 2^-8), 1 + 3 2^-8 -> 1 + 2^-6 (lo = -2^-8)"""
    w = np.array([[1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 0.5]], dtype=np.float32)
    g = _bits(pack.frag_pack3(torch.from_numpy(w)))
    hi, lo = bf16_val(g[0, 0, 0, 0, :4]), bf16_val(g[0, 0, 1, 0, :4])
    assert hi.tolist() == [1.0, 1 + 2.0 ** -6, -1.0, 0.5]
    assert lo.tolist() == [2.0 ** -8, -(2.0 ** -8), -(2.0 ** -8), 0.0]


# ---- conv_taps_matrix ---------------------------------------------------------------------------------------------------------------
def ref_conv_taps(w, cin_pad_to):
    co, ci, kh, kw = w.shape
    cip = (ci + cin_pad_to - 1) // cin_pad_to * cin_pad_to
    m = np.zeros((co, kh * kw * cip), dtype=np.float32)
    for o in range(co):
        for c in range(ci):
            for ky in range(kh):
                for kx in range(kw):
                    m[o, (ky * kw + kx) * cip + c] = w[o, c, ky, kx]
    return m


@pytest.mark.parametrize("cin_pad_to", (4, 32))
@pytest.mark.parametrize("shape", ((5, 3, 3, 3), (6, 8, 3, 3), (3, 32, 3, 3), (4, 3, 4, 4), (7, 5, 1, 1)))
def test_conv_taps_matrix(shape, cin_pad_to):
    """k = tap * cip + c, tap = ky * kw + kx, channels zero padded to cip ((6, 8, 3, 3) at 4 and (3, 32, 3, 3) need no padding)"""
    w = _rand(shape, 7)
    got = pack.conv_taps_matrix(torch.from_numpy(w), cin_pad_to)
    want = ref_conv_taps(w, cin_pad_to)
    assert tuple(got.shape) == want.shape and np.array_equal(got.numpy(), want)


# ---- rfcbam_gen_weights -------------------------------------------------------------------------------------------------------------
def _gen_params(C, seed):
    gw = _rand((C * 9, 1, 3, 3), seed, -3, 3)
    scale = _rand((C * 9,), seed + 1, -2, 2)
    shift = _rand((C * 9,), seed + 2, -2, 2)
    return gw, scale, shift


def ref_gen_weights(gw, scale, shift, chunk, contiguous):
    """element (ch, t, e) at (((((q*4 + w)*9 + t)*(per/2) + p)*10 + e)*2 + ab, with ly_gw_index's q, w, j, p, ab (csrc/ly_rfcbam_att.hip)"""
    C = gw.shape[0] // 9
    cp = (C + chunk - 1) // chunk * chunk
    per = chunk // 4
    out = np.full(cp * 90, np.nan, dtype=np.float32)
    w3 = gw.reshape(C, 9, 9)
    for ch in range(cp):
        q, r = divmod(ch, chunk)
        wv = r // per if contiguous else r & 3
        j = r - wv * per if contiguous else r >> 2
        p, ab = j >> 1, j & 1
        for t in range(9):
            for e in range(10):
                v = np.float32(0)
                if ch < C:
                    v = w3[ch, t, e] * scale[ch * 9 + t] if e < 9 else shift[ch * 9 + t]
                i = (((((q * 4 + wv) * 9 + t) * (per // 2) + p) * 10 + e) * 2 + ab)
                assert np.isnan(out[i])                  # the map is one to one
                out[i] = v
    assert not np.isnan(out).any()                        # ... and onto
    return out


@pytest.mark.parametrize("C", (32, 40))
@pytest.mark.parametrize("chunk,contiguous", ((32, False), (16, True)))
def test_rfcbam_gen_weights(chunk, contiguous, C):
    """both orders the kernels read (32-channel chunks with channel c0 + w + 4j: ly_rfcbam_stats; 16-channel chunks with c0 + 4w + j:
    ly_rfcbam3_fwd); C = 40: padded channels are zero"""
    gw, scale, shift = _gen_params(C, 11)
    got = pack.rfcbam_gen_weights(torch.from_numpy(gw), torch.from_numpy(scale), torch.from_numpy(shift), chunk, contiguous)
    want = ref_gen_weights(gw, scale, shift, chunk, contiguous)
    assert got.dtype == torch.float32 and got.numel() == want.size
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    other = ref_gen_weights(gw, scale, shift, chunk, not contiguous)
    assert not np.array_equal(other, want)               # the two channel orders are different images at this shape


# ---- rfcbam_gen_weights_c -----------------------------------------------------------------------------------------------------------
def ref_gen_weights_c(gw, scale, shift, raw):
    """element i of channel c at ((c/32*25 + i/4)*32 + c%32)*4 + i%4; i = t*9 + u: w[t][u], 81 + t: b[t], 90 + t: a[t], 99: 0"""
    C = gw.shape[0] // 9
    w3 = gw.reshape(C, 9, 9)
    out = np.full(C * 100, np.nan, dtype=np.float32)
    for c in range(C):
        for i in range(100):
            if i < 81:
                t, u = divmod(i, 9)
                v = w3[c, t, u] if raw else w3[c, t, u] * scale[c * 9 + t]
            elif i < 90:
                v = shift[c * 9 + i - 81]
            elif i < 99:
                v = scale[c * 9 + i - 90] if raw else np.float32(1)
            else:
                v = np.float32(0)
            out[((c // 32 * 25 + i // 4) * 32 + c % 32) * 4 + i % 4] = v
    assert not np.isnan(out).any()
    return out


@pytest.mark.parametrize("C", (32, 64))
@pytest.mark.parametrize("raw", (False, True), ids=("folded", "raw"))
def test_rfcbam_gen_weights_c(raw, C):
    gw, scale, shift = _gen_params(C, 21)
    got = pack.rfcbam_gen_weights_c(torch.from_numpy(gw), torch.from_numpy(scale), torch.from_numpy(shift), raw=raw)
    want = ref_gen_weights_c(gw, scale, shift, raw)
    assert got.numel() == want.size and np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))


# ---- rf3m_stream --------------------------------------------------------------------------------------------------------------------
def ref_rf3m_stream(gw, scale, shift, conv_w=None, mt=4, pool_stride=None):
    """every fragment in the order of the docstring, as bf16 bits [gy][chunks][fragments][64][8]:
    per chunk, per unit j: 3 generate fragments, 3 tap-8 fragments, [main] 2 k-steps x mt main fragments (k-step major);
    then [main] mt fragments of the tap-8 tile"""
    C = gw.shape[0] // 9
    nch = C // 16
    wx = np.zeros((C, 9, 12), dtype=np.float32)
    w3 = gw.reshape(C, 9, 9)
    for c in range(C):
        for t in range(9):
            for u in range(9):
                wx[c, t, u] = w3[c, t, u] * scale[c * 9 + t]
            b = np.float32(shift[c * 9 + t])
            bh = bf16_val(bf16_bits(b.reshape(1)))[0]
            bl = bf16_val(bf16_bits((b - bh).reshape(1)))[0]
            bll = bf16_val(bf16_bits(((b - bh) - bl).reshape(1)))[0]
            wx[c, t, 9], wx[c, t, 10], wx[c, t, 11] = bh, bl, bll
    owned = {None: (), 1: (4,), 2: (4, 5, 7, 8)}[pool_stride]
    main = conv_w is not None
    gy = conv_w.shape[0] // (32 * mt) if main else 1
    wc = conv_w.reshape(conv_w.shape[0], C, 9) if main else None
    nfr = 4 * (6 + 2 * mt) + mt if main else 24
    out = np.zeros((gy, nch, nfr, 64, 8), dtype=np.float32)
    for g in range(gy):
        for ch in range(nch):
            f = 0
            for j in range(4):
                for st in range(3):                                           # the (channel 4j + r // 8, tap r % 8) row tile
                    for lane in range(64):
                        r, h = lane & 31, lane >> 5
                        for e in range(8):
                            u, cs = 4 * st + 2 * h + e // 4, e % 4
                            if cs == r // 8:
                                out[g, ch, f, lane, e] = wx[16 * ch + 4 * j + r // 8, r % 8, u]
                    f += 1
                for st in range(3):                                           # the chunk's tap-8 tile, this unit's four channels
                    for lane in range(64):
                        r, h = lane & 31, lane >> 5
                        for e in range(8):
                            u, cs = 4 * st + 2 * h + e // 4, e % 4
                            if r < 16 and r // 4 == j and cs == r % 4:
                                out[g, ch, f, lane, e] = wx[16 * ch + r, 8, u]
                            if r >= 16 and (r - 16) // 4 == j and cs == (r - 16) % 4 and u in owned:
                                out[g, ch, f, lane, e] = 1.0                  # SE pooling rows
                    f += 1
                if main:
                    for s2 in range(2):
                        for m in range(mt):
                            for lane in range(64):
                                r, h = lane & 31, lane >> 5
                                for e in range(8):
                                    row = 16 * s2 + 8 * (e // 4) + 4 * h + e % 4
                                    out[g, ch, f, lane, e] = wc[32 * (g * mt + m) + r, 16 * ch + 4 * j + row // 8, row % 8]
                            f += 1
            if main:
                for m in range(mt):
                    for lane in range(64):
                        r, h = lane & 31, lane >> 5
                        for e in range(8):
                            out[g, ch, f, lane, e] = wc[32 * (g * mt + m) + r, 16 * ch + 8 * (e // 4) + 4 * h + e % 4, 8]
                    f += 1
            assert f == nfr
    return bf16_bits(out), wx


def _check_stream(got, want):
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == want.shape
    bad = np.argwhere(_bits(got) != want)
    assert bad.size == 0, f"first differing (gy, chunk, fragment, lane, e): {bad[:4].tolist()}"


def test_rf3m_stream_main():
    """the main stream at C = 32, O = 256, mt = 4: two blocks of output channels, two chunks, 4 (6 + 8) + 4 fragments each"""
    gw, scale, shift = _gen_params(32, 31)
    cw = _rand((256, 32, 3, 3), 34, -4, 2)
    tt = torch.from_numpy
    got = pack.rf3m_stream(tt(gw), tt(scale), tt(shift), tt(cw), 4)
    want, wx = ref_rf3m_stream(gw, scale, shift, cw, 4)
    assert want.shape == (2, 2, 60, 64, 8)
    assert np.count_nonzero(wx[:, :, 10]) > 0.9 * wx[:, :, 10].size and np.count_nonzero(wx[:, :, 11]) > 0.5 * wx[:, :, 11].size
    _check_stream(got, want)


@pytest.mark.parametrize("pool_stride", (None, 1, 2))
def test_rf3m_stream_stats(pool_stride):
    """the statistics stream: generate fragments only; with pool_stride the tap-8 tile's rows 16 .. 31 hold ones at the owned patch slots
    ({4} at stride 1, {4, 5, 7, 8} at stride 2)"""
    gw, scale, shift = _gen_params(32, 41)
    tt = torch.from_numpy
    got = pack.rf3m_stream(tt(gw), tt(scale), tt(shift), pool_stride=pool_stride)
    want, _ = ref_rf3m_stream(gw, scale, shift, pool_stride=pool_stride)
    assert want.shape == (1, 2, 24, 64, 8)
    pool_rows = [lane for lane in range(64) if (lane & 31) >= 16]
    ones = int(np.count_nonzero(want[0, 0][:, pool_rows, :] == 0x3F80))       # bf16 1.0
    assert ones == {None: 0, 1: 16, 2: 64}[pool_stride]   # 16 channels x owned slots, per chunk
    _check_stream(got, want)


def test_rf3m_stream_pool_rows_need_statistics_stream():
    gw, scale, shift = _gen_params(32, 51)
    tt = torch.from_numpy
    cw = tt(_rand((128, 32, 3, 3), 52))
    with pytest.raises(ValueError):
        pack.rf3m_stream(tt(gw), tt(scale), tt(shift), cw, 4, pool_stride=2)
    with pytest.raises(ValueError):
        pack.rf3m_stream(tt(gw), tt(scale), tt(shift), pool_stride=3)


# ---- the descriptor map of ly_pack_table --------------------------------------------------------------------------------------------
def emulate(src, K, flat, origin=0, flat2=None):
    """The LyPackDesc formula of include/lead_yolo_hip.h applied to a flat float32 array -> [src.rows, K] matrix:
    r = ra*nrb + rb, k = (a*nb + b)*nc + c, element flat[origin + base + ra*sra + rb*srb + a*sa + b*sb + c*sc] where b < vb and c < vc,
    else 0.  flat2: a source over two allocations (pack.src_matrix_kcat_t) — column block b = 1 is read from flat2 at the index without
    b*sb.  Every read that counts must be inside the array."""
    r = np.arange(src.rows, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    ra, rb = r // src.nrb, r % src.nrb
    c, ab = k % src.nc, k // src.nc
    b, a = ab % src.nb, ab // src.nb
    ok = (b < src.vb) & (c < src.vc) & (r < src.rows)
    idx = origin + src.base + ra * src.sra + rb * src.srb + a * src.sa + c * src.sc
    if flat2 is None:
        idx = idx + b * src.sb
        assert idx[ok].min() >= 0 and idx[ok].max() < flat.size, "descriptor reads outside its parameter"
        return np.where(ok, flat[np.where(ok, idx, 0)], np.float32(0))
    assert src.nb == 2 and idx[ok].min() >= 0 and idx[ok].max() < min(flat.size, flat2.size)
    idx = np.where(ok, idx, 0)
    return np.where(ok, np.where(b == 0, flat[idx], flat2[idx]), np.float32(0))


def _t(shape, seed):
    return torch.from_numpy(_rand(shape, seed, -4, 4))


def _emu(src, K, w):
    return torch.from_numpy(emulate(src, K, w.detach().numpy().reshape(-1)))


def test_desc_src_matrix():
    w = _t((19, 37), 1)
    assert torch.equal(_emu(pack.src_matrix(w, 19, 37), 37, w), w)
    # transposed view: W^T [37, 19] read in place
    assert torch.equal(_emu(pack.src_matrix(w, 37, 19, sr=1, sk=37), 19, w), w.t())
    # ... with the columns zero padded to k_pad (the 1x1 data gradient against a wider du)
    want = torch.cat((w.t(), torch.zeros(37, 13)), 1)
    assert torch.equal(_emu(pack.src_matrix(w, 37, 19, sr=1, sk=37, k_pad=32), 32, w), want)
    # a 4-D weight read as [co, ci*kh*kw] (PatchEmbed / PatchMerging)
    w4 = _t((10, 3, 4, 4), 2)
    assert torch.equal(_emu(pack.src_matrix(w4, 10, 48), 48, w4), w4.reshape(10, 48))


@pytest.mark.parametrize("shape,cip", (((5, 6, 3, 3), 8), ((5, 6, 3, 3), 32), ((7, 8, 3, 3), 8), ((4, 3, 2, 2), 4)))
def test_desc_src_taps(shape, cip):
    w = _t(shape, 3)
    t = shape[2] * shape[3]
    assert torch.equal(_emu(pack.src_taps(w, cip), t * cip, w), pack.conv_taps_matrix(w, cip))


@pytest.mark.parametrize("shape,cop", (((5, 6, 3, 3), 8), ((5, 6, 3, 3), 32), ((8, 7, 3, 3), 8)))
def test_desc_src_taps_transposed_flipped(shape, cop):
    """the operand of the stride-1 convolution's data gradient: negative tap stride, base at the last tap"""
    w = _t(shape, 4)
    want = pack.conv_taps_matrix(w.permute(1, 0, 2, 3).flip(2, 3), cop)
    assert torch.equal(_emu(pack.src_taps(w, cop, transposed_flipped=True), 9 * cop, w), want)


@pytest.mark.parametrize("gap", (24, -300))
def test_desc_src_matrix_kcat_t(gap):
    """[W1^T | W2^T] over two allocations: both weights are views of one buffer with a gap between them (W2 before W1 when negative), so
    that the emulator indexes a single array; full, and rows [r0, r1) of it"""
    c_, kin = 12, 20
    n = c_ * kin
    buf = _t((2 * n + 400,), 5)
    o1 = 350 if gap < 0 else 8
    o2 = o1 + n + gap if gap > 0 else o1 + gap
    w1, w2 = buf[o1:o1 + n].view(c_, kin), buf[o2:o2 + n].view(c_, kin)
    full = torch.cat((w1.t(), w2.t()), 1)
    flat = buf.numpy()
    src = pack.src_matrix_kcat_t(w1, w2)
    assert src is not None and src.sb == o2 - o1
    assert torch.equal(torch.from_numpy(emulate(src, 2 * c_, flat, origin=o1)), full)
    for r0, r1 in ((0, 8), (8, None), (5, 17)):
        src = pack.src_matrix_kcat_t(w1, w2, r0, r1)
        assert torch.equal(torch.from_numpy(emulate(src, 2 * c_, flat, origin=o1)), full[r0:r1])
    # the two-array form the device tests use gives the same matrix
    got = emulate(pack.src_matrix_kcat_t(w1, w2, 5, 17), 2 * c_, w1.numpy().reshape(-1), flat2=w2.numpy().reshape(-1))
    assert torch.equal(torch.from_numpy(got), full[5:17])


@pytest.mark.parametrize("k", (1, 2, 3))
def test_desc_transposed_patch_matrix(k):
    """grad.py: Src(w, k*k*c, nrb=c, sra=1, srb=k*k, nc=co, sc=c*k*k) is the transposed patch matrix: row tap*c + ch, column o"""
    co, c = 10, 6
    w = _t((co, c, k, k), 6)
    src = pack.Src(w, k * k * c, nrb=c, sra=1, srb=k * k, nc=co, sc=c * k * k)
    want = w.reshape(co, c, k * k).permute(2, 1, 0).reshape(k * k * c, co)
    assert torch.equal(_emu(src, co, w), want)
    assert torch.equal(want, pack.conv_taps_matrix(w, 1).t())


@pytest.mark.parametrize("c", (16, 48))
def test_desc_rfcbam_main_ten_slots(c):
    """modules.py: conv.0.weight [o, c, 3, 3] as [o][c/16 chunks][10 tap slots][16 channels], k = chunk*160 + t*16 + ch; slot 9 is
    padding (vb = 9 < nb = 10: 144 -> 160 columns per chunk)"""
    o = 7
    w = _t((o, c, 3, 3), 7)
    src = pack.Src(w, o, srb=c * 9, nb=10, vb=9, nc=16, sa=144, sb=1, sc=9)
    want = torch.zeros(o, c // 16, 10, 16)
    want[:, :, :9] = w.reshape(o, c // 16, 16, 9).transpose(2, 3)
    assert torch.equal(_emu(src, (c // 16) * 160, w), want.reshape(o, -1))


@pytest.mark.parametrize("c", (32, 64))
def test_desc_rfcbam_lane_channel_taps(c):
    """modules.py: conv.0.weight [o, c, 3, 3] as [o][c/32 chunks][9 taps][32 channels], k = chunk*288 + t*32 + ch"""
    o = 5
    w = _t((o, c, 3, 3), 8)
    src = pack.Src(w, o, srb=c * 9, nb=9, nc=32, sa=288, sb=1, sc=9)
    want = w.reshape(o, c // 32, 32, 9).transpose(2, 3).reshape(o, 9 * c)
    assert torch.equal(_emu(src, 9 * c, w), want)
