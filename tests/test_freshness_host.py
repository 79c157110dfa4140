"""Host-side pins of what the weight caches rest on (pack.PLAN, the `_Prepared` slots, pack.master's shadows, GraphedForward.stale()):
  * which ways of writing a tensor move torch's per-tensor `_version` — every cache key is built from it, so a torch upgrade that
    changes one of these facts has to fail HERE and not as a stale weight image in production;
  * `pack.touch_weights()` is the way out for the writes that move no counter, and reaches pack.master's float32 shadows too;
  * graph.fingerprint — what GraphedForward.stale() compares — moves with every route that changes weights.
CPU only; tests/test_gpu_freshness.py checks the same on the device against cold copies of the modules."""
import copy

import torch

from lead_yolo_amd import graph, pack


def _param(dtype=torch.float32):
    return torch.nn.Parameter(torch.arange(12, dtype=torch.float32).view(3, 4).to(dtype))


def test_version_counter_facts():
    p = _param()
    v = p._version
    p.data.mul_(2)                                   # a write through .data: NO cache key notices it
    assert p._version == v
    p.data.copy_(torch.ones(3, 4))
    assert p._version == v
    p.data[0, 0] = 5.0
    assert p._version == v
    p.detach().add_(1)                               # detach() shares the counter
    assert p._version > v
    v = p._version
    with torch.no_grad():
        p.mul_(2)
    assert p._version > v
    v = p._version
    with torch.no_grad():
        p.copy_(torch.zeros(3, 4))
    assert p._version > v
    lin = torch.nn.Linear(4, 3)
    bn = torch.nn.BatchNorm2d(3)
    v = [t._version for t in (lin.weight, lin.bias, bn.running_mean, bn.running_var)]
    lin.load_state_dict({k: t + 1 for k, t in lin.state_dict().items()})
    bn.load_state_dict({k: t + 1 for k, t in bn.state_dict().items()})
    assert all(t._version > a for t, a in zip((lin.weight, lin.bias, bn.running_mean, bn.running_var), v))
    for make in (lambda ps: torch.optim.SGD(ps, lr=0.1, momentum=0.9, nesterov=True), lambda ps: torch.optim.AdamW(ps, lr=0.1)):
        opt = make(lin.parameters())
        for q in lin.parameters():
            q.grad = torch.ones_like(q)
        v = [q._version for q in lin.parameters()]
        opt.step()
        assert all(q._version > a for q, a in zip(lin.parameters(), v))
    # state_dict() hands out aliases that share address and counter with the live tensors: graph.fingerprint reads them
    sd = bn.state_dict()
    assert sd["running_mean"].data_ptr() == bn.running_mean.data_ptr() and sd["weight"].data_ptr() == bn.weight.data_ptr()
    v = sd["running_mean"]._version, sd["weight"]._version
    with torch.no_grad():
        bn.running_mean.add_(1)
        bn.weight.add_(1)
    assert sd["running_mean"]._version > v[0] and sd["weight"]._version > v[1]


def test_versions_key_moves_with_counter_and_epoch():
    p, q = _param(), _param()
    k0 = pack.versions(p, None, q)
    assert pack.versions(p, None, q) == k0
    with torch.no_grad():
        q.add_(1)
    k1 = pack.versions(p, None, q)
    assert k1 != k0
    p.data.mul_(2)
    assert pack.versions(p, None, q) == k1           # the hole ...
    pack.touch_weights()
    assert pack.versions(p, None, q) != k1           # ... and the documented way out
    k2 = pack.versions(p, None, q)
    pack.touch()
    assert pack.versions(p, None, q) != k2


def test_master_is_the_parameter_itself_in_float32():
    p = _param()
    assert pack.master(p) is p


def test_master_shadow_follows_version_counter():
    p = _param(torch.bfloat16)
    s0 = pack.master(p)
    assert s0.dtype == torch.float32 and s0.is_contiguous() and torch.equal(s0, p.detach().float())
    assert pack.master(p) is s0                       # nothing changed: the same shadow, no copy
    with torch.no_grad():
        p.mul_(2)
    s1 = pack.master(p)
    assert s1 is not s0 and torch.equal(s1, p.detach().float())


def test_master_shadow_follows_touch_weights():
    """the one way out for `.data` writes must reach the shadows: `_Prepared` rebuilds because EPOCH moved, and re-packed the OLD
    shadow when the shadow was keyed on `_version` alone"""
    p = _param(torch.bfloat16)
    s0 = pack.master(p)
    want0 = s0.clone()
    p.data.mul_(2)
    pack.touch_weights()
    s1 = pack.master(p)
    assert torch.equal(s1, p.detach().float()) and torch.equal(s1, 2 * want0)
    assert pack.master(p) is s1


def test_master_shadow_does_not_outlive_its_parameter():
    p = _param(torch.bfloat16)
    pack.master(p)
    k = id(p)
    assert k in pack._SHADOW
    del p
    assert k not in pack._SHADOW


def test_source_whose_parameter_moved_counts_as_dead():
    """pack.Src addresses raw memory: once its parameter lives elsewhere (`.float()`, `.to()`, `p.data = ...`) the description is dead —
    PLAN drops it at the next refresh instead of packing from memory the parameter no longer owns"""
    p = _param()
    s = pack.src_matrix(p, 3, 4)
    assert s.param is p
    with torch.no_grad():
        p.mul_(2)
    assert s.param is p                               # a change of values is the version counter's business
    p.data = p.data.clone()
    assert s.param is None


def test_dtype_and_device_conversions_announce_themselves():
    """`.bfloat16().float()` can put a weight back at its old address with its old version counter and other (rounded) values: the
    modules that keep prepared copies move the write epoch in `_apply`"""
    import lead_yolo_amd as L
    for m in (L.Conv(8, 8, 3, 1), L.BasicStage(16, 1), L.RFCBAMConv(16, 16, 3, 1), L.CoordAtt(32, 32), L.SPPF(16, 16),
              L.PatchMerging_FasterNet(8, 16, 2, 2), L.Detect(nc=1, anchors=((1, 2, 3, 4, 5, 6),), ch=(8,))):
        p = next(m.parameters())
        for convert in (lambda: m.bfloat16(), lambda: m.float(), lambda: m.to("cpu")):
            v, e, w = p._version, pack.EPOCH, pack.W_EPOCH
            convert()
            assert pack.EPOCH > e and pack.W_EPOCH > w, type(m).__name__
            assert p._version == v                    # (the reason: no counter moves)


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(4, 4, 1)
        self.bn = torch.nn.BatchNorm2d(4)


def test_fingerprint_moves_with_every_route():
    m = _Tiny()
    other = {k: v + 1 if v.is_floating_point() else v for k, v in copy.deepcopy(m.state_dict()).items()}
    f = graph.fingerprint(m)
    assert graph.fingerprint(m) == f

    def moved(what):
        nonlocal f
        g = graph.fingerprint(m)
        assert g != f, what
        f = g
    m.load_state_dict(other)
    moved("load_state_dict")
    with torch.no_grad():
        m.conv.weight.copy_(other["conv.weight"])
    moved("no_grad copy_")
    m.bn.running_var.detach().copy_(other["bn.running_var"])
    moved("detach().copy_ on a buffer")
    m.conv.bias.data.copy_(other["conv.bias"])
    assert graph.fingerprint(m) == f                  # `.data` alone is invisible ...
    pack.touch_weights()
    moved(".data + touch_weights")                    # ... the contract makes it visible
    m.bfloat16()
    moved(".bfloat16()")
    m.float()
    moved(".float()")
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    for q in m.parameters():
        q.grad = torch.ones_like(q)
    opt.step()
    moved("optim.step")
    pack.touch()                                       # ly_bn_finalize's signal (running statistics written by a kernel)
    moved("pack.touch")


def test_bn_train_args_refuses_and_touches_only_for_tracked_statistics():
    """ops._bn_train_args, which gathers a train-mode BatchNorm's arguments for the finalize kernels (what any route that shares it must
    keep): momentum=None with tracked statistics is refused (the kernels compute no cumulative average) before anything is announced;
    without tracked statistics the running-stat pointers are null and no cache is invalidated; with them the epoch moves (the kernel
    writes behind torch's version counters)"""
    import pytest

    from lead_yolo_amd import ops
    bn = torch.nn.BatchNorm2d(4, momentum=None).train()
    before = pack.versions()
    with pytest.raises(NotImplementedError):
        ops._bn_train_args(bn)
    assert pack.versions() == before
    with pytest.raises(NotImplementedError):
        ops._bn_train_args(torch.nn.BatchNorm2d(4).train().half())
    assert pack.versions() == before
    for momentum in (None, 0.1):
        free = torch.nn.BatchNorm2d(4, momentum=momentum, track_running_stats=False).train()
        gamma, beta, eps, mom, running_mean, running_var, nbt = ops._bn_train_args(free)
        assert running_mean.value is None and running_var.value is None and nbt.value is None
        assert gamma.value == free.weight.data_ptr() and beta.value == free.bias.data_ptr() and eps == free.eps
        assert pack.versions() == before
    bn = torch.nn.BatchNorm2d(4, momentum=0.25).train()
    gamma, beta, eps, mom, running_mean, running_var, nbt = ops._bn_train_args(bn)
    assert (running_mean.value, running_var.value, nbt.value) == (bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr())
    assert mom == 0.25 and pack.versions() != before
