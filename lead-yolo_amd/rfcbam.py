"""RFCBAMConv forward (models/rfa.py:113-129): which of the four kernel families runs (`select`) and the launches of each (`forward`),
stated once for inference (modules.RFCBAMConv.forward) and training (grad.RfcbamFn.forward).  A kernel change edits KINDS and `forward`;
the backward's own route choice stays in grad.RfcbamFn.backward.

route | statistics pass                     | SE pooling partials                      | small maps                   | contraction
k1    | ops.rfcbam_stats(k=1)               | eval: that pass (gap=True)               | eval: rfcbam_mid             | ops.gemm(pro=PRO_AFFINE_RELU_CA, rowscale=rfa)
rf3   | ops.rfcbam_stats(k=3, wg=wq_stats)  | eval: ops.colsum                         | eval: rfcbam_mid             | ops.rfcbam3(wg=wq_main)        lane = pixel
      |                                     | train, k1 and rf3: ops.se_attention      | train, k1 and rf3: rfa_map   |
rf3c  | ops.rf3c_stats(wq_c)                | that pass                                | rfcbam_mid                   | ops.rf3c_fwd(wq_c, wp_c)       lane = channel
rf3m  | ops.rf3m_stats(wm_stats)            | that pass                                | rfcbam_mid                   | ops.rf3m_fwd(wm)               matrix-core generate, eval only"""
import collections

import torch

from . import ops
from .capi import ACT_NONE, ACT_RELU

# tile picker (ho, wo, s) of the route's statistics and contraction kernels | key of the conv weight image in RFCBAMConv._packed / _packed_train
# | the identity epilogue scale of the training contraction, from its shift (the bias): none at k = 1, one cached vector on rf3c, a fresh
# fill on rf3 — the fill is a launch of the step, kept as it is
_Kind = collections.namedtuple("_Kind", "pick wp identity")
KINDS = {
    "k1": _Kind(None, "wp", lambda bias: None),
    "rf3": _Kind(lambda ho, wo, s: ops.pick_tile(ho, wo), "wp", torch.ones_like),
    "rf3c": _Kind(lambda ho, wo, s: ops.pick_tile_c(ho, wo, s), "wp_c", lambda bias: ops.ones_f32(bias.numel(), bias.device)),
    "rf3m": _Kind(lambda ho, wo, s: ops.pick_tile_m(ho, wo, s), "wm", None),
}

# name: a key of KINDS.  th, tw: the tile, when the size was given.  could: every route a module may take once the size is known
Route = collections.namedtuple("Route", "name th tw could")
# what a forward leaves for the backward, beside the output: gen is the dict the generate weights were read from, stats the striped sums
# of a want_stats contraction
Kept = collections.namedtuple("Kept", "ca rfa mm se_part route gen stats")


def select(training, dtype, k, s, c, o, n=None, ho=None, wo=None):
    """The route of an RFCBAMConv(c, o, k, s) forward on `dtype` storage.  Pure: no tensor, no device.  The development switches
    modules.RF3M / RF3C and ops.RF3M_MIN_UNITS / CONCURRENT_PARTS are read now.  Without a size the answer is the route of a large batch, and
    `could` lists what RFCBAMConv._packed / _packed_train build weight images for.  In training that is the route alone.  In eval it is
    rf3, rf3c wherever those kernels cover the module (RF3C and the fp32 exception below are not asked: tools flip the switch between
    calls, and the packed images' cache key does not carry it) and rf3m where the switch and the dtype allow it.
    Answers are remembered per (arguments, switches): an eager forward asks once per call, and the tile searches are Python loops."""
    from . import modules as M
    key = (training, dtype, k, s, c, o, n, ho, wo, M.RF3M, M.RF3C, ops.RF3M_MIN_UNITS, ops.CONCURRENT_PARTS)
    route = _SELECTED.get(key)
    if route is None:
        route = _SELECTED[key] = _select(M, *key[:9])
    return route


_SELECTED = {}


def _select(M, training, dtype, k, s, c, o, n, ho, wo):
    if k == 1:
        return Route("k1", None, None, ("k1",))
    # (inference in fp32 storage with more than 128 output channels: the lane = pixel kernels measure faster — layer 20 at bs=64: 215 vs 289 us —
    # the two-plane operand tile of the lane = channel kernel leaves one block per CU there)
    take_c = ops.rf3c_ok(c, s) and M.RF3C and (training or not (dtype == torch.float32 and o > 128))
    # (bf16, stride 1 / 2 only, and from ops.RF3M_MIN_UNITS wave tiles when the size is given: the measurements stand beside that constant)
    take_m = not training and M.RF3M and ops.rf3m_ok(dtype, c, o, s, n, ho, wo)
    name = "rf3m" if take_m else "rf3c" if take_c else "rf3"
    if n is not None:
        return Route(name, *KINDS[name].pick(ho, wo, s), (name,))
    if training:
        return Route(name, None, None, (name,))
    return Route(name, None, None, ("rf3",) + (("rf3c",) if ops.rf3c_ok(c, s) else ()) + (("rf3m",) if take_m else ()))


def forward(route, xr, ld, k, s, o, *, se, w18, gen, packed, raw, se_first, e_scale, e_shift, want_stats):
    """One RFCBAMConv forward over the rows (xr, ld) on `route` (a sized answer of `select`): statistics, SE / get_weight maps, contraction.
    -> (out, Kept).  What inference and training give differently:
      se = (wa, wb, ratio): SE's two linears, fp32;  w18: get_weight's taps;  packed: the dict holding the route's conv weight image
      gen:      () -> the dict of generate weights, asked behind SE's launch: the folded images of _packed, or (raw) ops.rfcbam_gen_prepare's
      se_first: k1 and rf3 take `ca` and the pooling partials from ops.se_attention, launched in front of `gen`, and the attention map from
                ops.rfa_map (training: the partials are kept for SE's backward in se_attention's slicing)
      e_scale, e_shift: epilogue of the contraction; e_scale None = identity, made the route's way (KINDS) behind the accumulators
      want_stats: the contraction also sums the output BatchNorm's statistics (ops.new_stats) and `out` is the pre-BN value, no activation"""
    n, c, h, w = xr.shape
    ho, wo = ops.rf_out_hw(h, w, k, s)
    name, th, tw = route[:3]
    wa, wb, ratio = se
    ca = part = None
    if se_first and name in ("k1", "rf3"):
        ca, part = ops.se_attention(xr, ld, n, h * w, c, wa, wb, ratio, want_part=True)
    G = gen()
    if name == "k1":
        a1, b1 = G["a1"], G["gb" if raw else "b1"]
        mm = ops.rfcbam_stats(xr, ld, n, h, w, c, 1, 1, a1=a1, b1=b1, gap=ca is None)       # ONE pass over x: [max, mean] map AND SE's partial sums
        if ca is None:
            mm, part = mm
    elif name == "rf3":
        if ca is None:
            part = ops.colsum(xr, ld, n, h * w, c)                                          # k = 3: pooling partials as their own pass
        mm = ops.rfcbam_stats(xr, ld, n, h, w, c, 3, s, wg=G["wq_stats"], th=th, tw=tw)
    elif name == "rf3c":
        # x read twice: statistics + SE pooling partials | SE linears + get_weight conv | regenerate + contraction.  raw: the RAW generate
        # image (u = w.x, v = a*u + b) is what the backward re-evaluates bit for bit
        mm, part = ops.rf3c_stats(xr, ld, n, h, w, c, s, G["wq_c"], th, tw, raw=raw)
    else:
        # `generate` as block-diagonal MFMA products whose accumulators feed the main contraction in registers (csrc/ly_rf3m.hip)
        mm, part = ops.rf3m_stats(xr, ld, n, h, w, c, s, G["wm_stats"], th, tw)
    if ca is None:
        ca, rfa = ops.rfcbam_mid(part, h * w, wa, wb, ratio, mm, w18)
    else:
        rfa = ops.rfa_map(mm, w18)
    stats = ops.new_stats(o, xr.device) if want_stats else None
    out = ops.empty_nhwc(n, o, ho, wo, xr)
    if e_scale is None:
        e_scale = KINDS[name].identity(e_shift)
    wp = packed[KINDS[name].wp]
    if name == "k1":
        ops.gemm(M=n * h * w, H=h, W=w, K=c, N=o, a0=xr, lda0=ld, k0=c, wp=wp, out=out, ldo=o, pro=ops.PRO_AFFINE_RELU_CA, p_scale=a1, p_shift=b1,
                 p_ca=ca, rowscale=rfa, e_scale=e_scale, e_shift=e_shift, act=ACT_NONE if want_stats else ACT_RELU, stats=stats)
    else:
        kw = dict(n=n, h=h, w=w, c=c, ho=ho, wo=wo, N=o, s=s, th=th, tw=tw, x=xr, ldx=ld, ca=ca, rfa=rfa, wp=wp, e_scale=e_scale, e_shift=e_shift,
                  out=out, ldo=o)
        if name == "rf3":
            ops.rfcbam3(wg=G["wq_main"], stats=stats, **kw)
        elif name == "rf3c":
            ops.rf3c_fwd(wq=G["wq_c"], stats=stats, raw=raw, **kw)
        else:
            ops.rf3m_fwd(**kw)
    return out, Kept(ca, rfa, mm, part, route, G, stats)
