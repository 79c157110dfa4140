"""ops.ParamGrad / ops.SmallGrad.group / ops.zero_bias_grad: where a backward node's parameter gradients go (the sink's storage or a fresh
tensor for autograd) and when the gradient listeners are told.  Host logic only: the sink is a real ops.GradSink over CPU tensors, the
rounding launch ly_f64_add is replaced by its definition, as in test_small_grads.py."""
import pytest
import torch

import lead_yolo_amd as L
from lead_yolo_amd import ops, optim
from lead_yolo_amd.ddp import GradReducer


@pytest.fixture
def sink(monkeypatch):
    """an installed GradSink and the list of parameters announced to the gradient listeners"""
    s, told = ops.GradSink(), []
    monkeypatch.setattr(ops, "SINK", s)
    monkeypatch.setattr(ops, "GRAD_LISTENERS", [told.append])
    monkeypatch.setattr(ops, "GRAD_DEFER_LISTENERS", [])
    ops.small_grads_reset()
    yield s, told
    ops.small_grads_reset()


def param(*shape, target=True, sink=None):
    p = torch.nn.Parameter(torch.zeros(*shape))
    if target:
        p.grad = torch.zeros(*shape)
        sink.targets[id(p)] = p.grad
    return p


def tap_major_grad(p):
    co, ci, kh, kw = p.shape
    return torch.zeros(co, kh, kw, ci).permute(0, 3, 1, 2)


# ---- one parameter ----------------------------------------------------------------------------------------------------------------------
def test_direct_buf_is_the_target_and_listeners_are_told_once_at_finish(sink):
    s, told = sink
    p = param(4, 3, sink=s)
    g = ops.ParamGrad(p)
    assert g.direct and g.buf is p.grad and g.targets[0] is p.grad
    assert told == []                                   # not before finish()
    assert g.finish() is None
    assert told == [p]


def test_fresh_is_zeros_of_the_parameters_shape_returned_by_finish_without_a_listener_call(sink):
    s, told = sink
    p = param(4, 3, target=False)
    g = ops.ParamGrad(p)
    assert not g.direct and g.targets == [None]
    assert g.buf.shape == p.shape and g.buf.dtype == torch.float32 and not g.buf.any() and g.buf is g.buf
    g.buf.add_(1.0)
    out = g.finish()
    assert out is g.buf and told == []


def test_without_a_sink_everything_is_fresh(monkeypatch):
    monkeypatch.setattr(ops, "SINK", None)
    p = torch.nn.Parameter(torch.zeros(5))
    p.grad = torch.zeros(5)
    g = ops.ParamGrad(p)
    assert not g.direct and g.finish() is g.buf and g.buf is not p.grad


def test_frozen_parameter_has_no_target_and_nothing_is_announced(sink):
    s, told = sink
    p = param(6, sink=s)
    p.requires_grad_(False)
    g = ops.ParamGrad(p)
    assert not g.direct and g.buf is not p.grad
    assert g.finish() is g.buf and told == []


def test_reassigned_grad_falls_back_to_fresh(sink):
    s, told = sink
    p = param(6, sink=s)
    p.grad = torch.zeros(6)                            # no longer the tensor the sink holds
    g = ops.ParamGrad(p)
    assert not g.direct and g.buf is not p.grad and g.buf is not s.targets[id(p)]
    assert g.finish() is g.buf and told == []


def test_consumer_made_value_goes_through_the_view_and_no_zeros_are_made(sink, monkeypatch):
    s, told = sink
    p = param(2, 3, target=False)
    g = ops.ParamGrad(p, accept=ops.CONTIGUOUS, view=lambda t: t.t())
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: pytest.fail("a value handed to finish() needs no fresh buffer"))
    v = torch.ones(3, 2)
    out = g.finish(v)
    assert out.shape == (2, 3) and out.data_ptr() == v.data_ptr() and told == []


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------
def test_tap_major_target_by_accepted_layout(sink):
    s, told = sink
    p = torch.nn.Parameter(torch.zeros(8, 4, 3, 3))
    p.grad = tap_major_grad(p)
    s.targets[id(p)] = p.grad
    assert ops.tap_major(p.grad)
    own = ops.ParamGrad(p)
    assert own.direct and own.buf is p.grad
    rows = ops.ParamGrad(p, accept=ops.TAP_ROWS)
    assert rows.direct and rows.buf.shape == (8, 36) and rows.buf.is_contiguous() and rows.buf.data_ptr() == p.grad.data_ptr()
    rows.buf[1, 2 * 4 + 3] = 7.0                        # row 1, tap 2, channel 3
    assert p.grad[1, 3, 0, 2] == 7.0
    cont = ops.ParamGrad(p, accept=ops.CONTIGUOUS)      # a contiguous-only consumer cannot write it
    assert not cont.direct and cont.buf.shape == p.shape and cont.buf.is_contiguous() and cont.buf.data_ptr() != p.grad.data_ptr()
    assert told == []
    assert rows.finish() is None and told == [p]


def test_contiguous_targets_offered_to_a_tap_rows_consumer(sink):
    s, told = sink
    k3, k1 = param(8, 4, 3, 3, sink=s), param(8, 4, 1, 1, sink=s)
    g3 = ops.ParamGrad(k3, accept=ops.TAP_ROWS, fresh=lambda: torch.zeros(8, 36), view=lambda t: t.view(8, 9, 4).permute(0, 2, 1).reshape(k3.shape))
    assert not g3.direct and g3.buf.shape == (8, 36)   # [o][c][t] storage is not [o][t][c] rows
    g3.buf[1, 2 * 4 + 3] = 7.0
    out = g3.finish()
    assert out.shape == k3.shape and out[1, 3, 0, 2] == 7.0 and told == []
    g1 = ops.ParamGrad(k1, accept=ops.TAP_ROWS)         # one tap: the weight's own order is the rows
    assert g1.direct and g1.buf is k1.grad


# ---- several parameters one kernel writes together -----------------------------------------------------------------------------------
def test_pair_is_direct_only_when_both_are(sink):
    s, told = sink
    a, b = param(5, sink=s), param(5, sink=s)
    g = ops.ParamGrad(a, b, accept=ops.CONTIGUOUS)
    assert g.direct and g.bufs[0] is a.grad and g.bufs[1] is b.grad and told == []
    assert g.finish() == (None, None) and told == [a, b]
    del told[:]
    c = param(5, target=False)
    g = ops.ParamGrad(a, c, accept=ops.CONTIGUOUS)
    assert not g.direct and g.targets == [None, None]
    assert all(t.shape == (5,) and not t.any() for t in g.bufs) and g.bufs[0] is not a.grad
    out = g.finish()
    assert out[0] is g.bufs[0] and out[1] is g.bufs[1] and told == []
    b.requires_grad_(False)                             # a frozen half: both fresh as well
    assert not ops.ParamGrad(a, b, accept=ops.CONTIGUOUS).direct
    # values of a wrapper that makes its own fresh tensors (ops.bn_bwd_coeffs) pass through
    g = ops.ParamGrad(a, c, accept=ops.CONTIGUOUS)
    v0, v1 = torch.ones(5), torch.ones(5)
    out = g.finish(v0, v1)
    assert out[0] is v0 and out[1] is v1 and told == []
    # no parameters at all (a unit without BatchNorm): nothing direct, the values pass through
    assert ops.ParamGrad(None, None, accept=ops.CONTIGUOUS).finish(v0, None) == (v0, None)


def test_caller_supplied_fresh_storage_is_used_and_not_reallocated(sink, monkeypatch):
    s, told = sink
    a, b, c, d = param(5, target=False), param(5, target=False), param(5, sink=s), param(5, sink=s)
    store, calls = torch.zeros(2, 5), []

    def fresh():
        calls.append(1)
        return store[0], store[1]
    monkeypatch.setattr(torch, "zeros", lambda *a_, **k: pytest.fail("the supplied storage is the fresh storage"))
    g = ops.ParamGrad(a, b, accept=ops.CONTIGUOUS, fresh=fresh)
    assert calls == []                                  # made on first use
    assert g.bufs[0].data_ptr() == store[0].data_ptr() and g.bufs[1].data_ptr() == store[1].data_ptr()
    out = g.finish()
    assert out[0] is g.bufs[0] and out[1] is g.bufs[1] and calls == [1] and told == []
    one = ops.ParamGrad(a, fresh=lambda: store[0])      # one parameter: one tensor
    assert one.buf.data_ptr() == store.data_ptr() and one.finish() is one.buf
    # a direct destination never asks for it
    g = ops.ParamGrad(c, d, accept=ops.CONTIGUOUS, fresh=fresh)
    assert g.bufs[0] is c.grad and g.finish() == (None, None) and calls == [1]


def test_zero_bias_grad(sink):
    s, told = sink
    held, free = param(4, sink=s), param(4, target=False)
    like = torch.ones(4)
    assert ops.zero_bias_grad(like, held) is None and told == []
    for z in (ops.zero_bias_grad(like, free), ops.zero_bias_grad(like)):
        assert z.shape == (4,) and not z.any()
    held.requires_grad_(False)
    assert ops.zero_bias_grad(like, held) is not None


# ---- the sink invariant, and every site's choice for every target the optimisers and the reducer produce ----------------------------------
def _invariant(p, t):
    return tuple(t.shape) == tuple(p.shape) and t.dtype == torch.float32 and (
        t.is_contiguous() or (p.dim() == 4 and p.shape[2] * p.shape[3] > 1 and ops.tap_major(t)))


def _old_tap_major_rows(g):
    """grad._tap_major_rows as the backward nodes spelled it before ops.ParamGrad"""
    if g is None or not ops.tap_major(g):
        return None
    co, ci, kh, kw = g.shape
    rows = g.permute(0, 2, 3, 1)
    return rows.view(co, kh * kw * ci) if rows.is_contiguous() else None


def _reachable_targets():
    """(name, parameter, target) over lead-yolo-n for: the fused optimisers' own storage; a GradReducer's bucket views, which the optimisers
    keep; and contiguous slices of a foreign buffer (a gradient somebody else owns: kept as it is, also for a tap-major-flagged weight)"""
    out = []
    for how in ("optimiser", "reducer", "foreign"):
        torch.manual_seed(0)
        m = L.Model(L.load_cfg(scale="n"))
        ps = list(m.named_parameters())
        if how == "reducer":
            GradReducer([p for _, p in ps])
        elif how == "foreign":
            flat = torch.zeros(sum(p.numel() for _, p in ps))
            off = 0
            for _, p in ps:
                p.grad = flat[off:off + p.numel()].view_as(p)
                off += p.numel()
        opt = optim.FusedSGD([p for _, p in ps])
        for _, p in ps:
            opt._grad_storage(p)                        # (shared by FusedSGD, FusedAdam and FusedAdamW)
        out += [(f"{how}:{k}", p, p.grad) for k, p in ps]
    return out


def test_sink_invariant_and_unchanged_choice_at_every_site(sink):
    s, _ = sink
    cases = _reachable_targets()
    assert any(ops.tap_major(t) for _, _, t in cases) and any(t._base is not None and t.is_contiguous() and t.dim() == 4 for _, _, t in cases)
    assert any(k.startswith("foreign") and p.dim() == 4 and p.shape[2] > 1 and getattr(p, "_ly_tap_major", False) for k, p, _ in cases)
    for k, p, t in cases:
        assert _invariant(p, t), k
        s.targets = {id(p): t}
        view = lambda accept: ops._sink_view(p, accept)
        assert view(ops.OWN) is t, k                                                   # conv_wgrad, MlpBlockFn: "it exists"
        taps = p.shape[2] * p.shape[3] if p.dim() == 4 else 1
        if taps == 1 or not getattr(p, "_ly_tap_major", False):
            # every parameter a contiguous-only consumer is offered (BatchNorm vectors, 1x1 and linear weights, the grouped generate weight):
            # "exists", "numel matches", "is contiguous" all hold, in whatever combination the site spelled them
            assert t.is_contiguous() and t.numel() == p.numel() and view(ops.CONTIGUOUS) is t, k
        if p.dim() == 4:
            # RFCBAM's conv weight: k = 1 "it exists", k = 3 "_tap_major_rows(target) is not None"
            old = t if taps == 1 else _old_tap_major_rows(t)
            new = view(ops.TAP_ROWS)
            assert (old is None) == (new is None), k
            if old is not None:
                assert new.data_ptr() == old.data_ptr() and new.shape == (old.shape if taps > 1 else t.shape) and new.stride() == old.stride(), k


# ---- CoordAtt's group -----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def host_round(monkeypatch):
    """ly_f64_add by its definition, for both of its callers"""
    def flush():
        items, ops._SmallGrads.pending, ops._SmallGrads.task = ops._SmallGrads.pending, [], -1
        for scr, tgt, prm in items:
            tgt += scr.float()
            if prm is not None:
                ops.grad_done(prm)
    monkeypatch.setattr(ops, "flush_small_grads", flush)
    monkeypatch.setattr(ops, "f64_round", lambda scr, shapes: [x.float().view(shp) for x, shp in zip(scr, shapes)])


class _Node(torch.autograd.Function):
    """a backward node that sums 1.0 into every buffer of its group, as a kernel would"""
    @staticmethod
    def forward(ctx, x, params, log):
        ctx.params, ctx.log = params, log
        return x * 2.0

    @staticmethod
    def backward(ctx, g):
        grp = ops.SmallGrad.group(ctx.params, zero=(1,))
        for b in grp.bufs:
            b += 1.0
        ctx.log.append((grp, [b.dtype for b in grp.bufs], grp.values()))
        grp.finish()
        return g * 2.0, None, None


def _coordatt_params(s, targets=True):
    shapes = ((8, 16, 1, 1), (8,), (8,), (8,), (16, 8, 1, 1), (16,), (16, 8, 1, 1), (16,))
    return tuple(param(*shp, target=targets, sink=s) for shp in shapes)


def test_group_defers_float64_scratches_inside_the_engine_when_every_target_is_sunk(sink, host_round):
    s, told = sink
    ps, log = _coordatt_params(s), []
    _Node.apply(torch.ones(3, requires_grad=True), ps, log).sum().backward()
    grp, dtypes, ret = log[0]
    assert grp.deferred and not grp.fresh64 and dtypes == [torch.float64] * 7 and ret == [None] * 8
    assert all(float(p.grad.min()) == 1.0 == float(p.grad.max()) for i, p in enumerate(ps) if i != 1) and not ps[1].grad.any()
    assert told[0] is ps[1] and sorted(map(id, told)) == sorted(map(id, ps)) and len(told) == 8      # the bias at finish(), the rest at the flush


def test_group_frozen_parameter_returns_and_announces_nothing(sink, host_round):
    s, told = sink
    ps, log = _coordatt_params(s), []
    ps[4].requires_grad_(False)
    ps[1].requires_grad_(False)
    _Node.apply(torch.ones(3, requires_grad=True), ps, log).sum().backward()
    grp, dtypes, ret = log[0]
    assert grp.deferred and len(grp.bufs) == 7 and ret == [None] * 8
    assert not ps[4].grad.any() and not any(t is ps[4] or t is ps[1] for t in told) and len(told) == 6


def test_group_rounds_fresh_float64_buffers_when_nothing_is_sunk(sink, host_round):
    s, told = sink
    ps, log = _coordatt_params(s, targets=False), []
    ps[6].requires_grad_(False)
    _Node.apply(torch.ones(3, requires_grad=True), ps, log).sum().backward()
    grp, dtypes, ret = log[0]
    assert grp.fresh64 and not grp.deferred and dtypes == [torch.float64] * 7 and told == []
    assert ret[6] is None and not ret[1].any() and ret[1].shape == ps[1].shape
    for i, (p, r) in enumerate(zip(ps, ret)):
        if i not in (1, 6):
            assert r.dtype == torch.float32 and r.shape == p.shape and float(r.min()) == 1.0 == float(r.max())


@pytest.mark.parametrize("why", ["outside the engine", "one target missing", "not deterministic and no sink"])
def test_group_takes_fp32_targets_as_they_are_otherwise(sink, host_round, monkeypatch, why):
    s, told = sink
    ps = _coordatt_params(s, targets=why != "not deterministic and no sink")
    if why == "one target missing":
        ps[5].grad = torch.zeros(16)                   # re-assigned: the sink gives no target
    if why == "not deterministic and no sink":
        monkeypatch.setattr(ops, "DETERMINISTIC_SMALL_GRADS", False)
    if why == "outside the engine":
        grp = ops.SmallGrad.group(ps, zero=(1,))
        dtypes, ret = [b.dtype for b in grp.bufs], grp.values()
        assert told == []                               # values() announces nothing
        grp.finish()
    else:
        log = []
        _Node.apply(torch.ones(3, requires_grad=True), ps, log).sum().backward()
        grp, dtypes, ret = log[0]
    assert not grp.deferred and not grp.fresh64 and dtypes == [torch.float32] * 7
    live = [p for i, p in enumerate(ps) if i != 1]
    if why == "outside the engine":
        assert ret == [None] * 8 and all(b is p.grad for b, p in zip(grp.bufs, live)) and told == list(ps)      # in the order of the parameters
    elif why == "one target missing":
        assert ret[5] is grp.bufs[4] and ret[5] is not ps[5].grad and [r is None for r in ret] == [i != 5 for i in range(8)]
        assert told == [p for i, p in enumerate(ps) if i != 5]
    else:
        assert told == [] and all(r is b for r, b in zip([r for i, r in enumerate(ret) if i != 1], grp.bufs)) and not ret[1].any()
