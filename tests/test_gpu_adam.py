"""GPU tests of the fused Adam / AdamW step (csrc/ly_adam.hip, optim.FusedAdam / FusedAdamW): against torch.optim.Adam / AdamW +
clip_grad_norm_ + ModelEMA.update, checkpoints in both directions, the captured step, bit reproducibility, the data-parallel reducer
and a short training trajectory."""
import copy

import pytest
import torch

from oracle import synth
from tests.test_gpu_backward import _one_rank_group
from tests.test_gpu_modules import _dev

pytestmark = pytest.mark.gpu


def _cfg(scale):
    import lead_yolo_amd as L
    return L.load_cfg(scale=scale)


def _model(seed=5151, scale="n"):
    import lead_yolo_amd as L
    torch.manual_seed(0)
    m = L.Model(_cfg(scale))
    st = synth.synth_state(synth.shapes_of(m.state_dict()), seed)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    m.load_state_dict(st)
    return m.to(_dev()).train()


def _set_grads(m, grads):
    for p, gr in zip(m.parameters(), grads):
        if p.grad is None:
            p.grad = gr.to(_dev()).clone()
        else:
            p.grad.copy_(gr)                      # (a tap-major view or a half of a stacked pair once the fused table exists)


def _torch_step(m, opt, max_norm=10.0):
    norm = torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=max_norm)
    opt.step()
    return norm


def _near(a, b, what, rel=1e-5):
    d = float((a - b).abs().max())
    assert d <= rel * float(b.abs().max()) + 1e-7, (what, d, float(b.abs().max()))


def _moments(opt, m):
    return {n: (opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for n, p in m.named_parameters() if p in opt.state}


@pytest.mark.parametrize("name", ["Adam", "AdamW"])
def test_fused_adam_matches_torch(name):
    """FusedAdam(W) (clip + Adam(W), 3 groups + zero_grad + EMA in three launches) vs torch.optim.Adam(W) + clip_grad_norm_ +
    ModelEMA.update on the same gradients, six steps: clipped and unclipped steps, a new lr every step, new betas once, moving buffers"""
    import lead_yolo_amd as L
    ms = [_model(), _model()]
    opts = [L.smart_optimizer(ms[0], name, 1e-3, 0.937, 5e-4, fused=True), L.smart_optimizer(ms[1], name, 1e-3, 0.937, 5e-4, fused=False)]
    assert type(opts[0]) is (L.FusedAdamW if name == "AdamW" else L.FusedAdam)
    assert type(opts[1]) is (torch.optim.AdamW if name == "AdamW" else torch.optim.Adam)
    emas = [L.ModelEMA(m) for m in ms]
    opts[0].attach_ema(emas[0], ms[0])
    g = torch.Generator().manual_seed(1)
    for step in range(6):
        grads = [torch.randn(p.shape, generator=g) * (1.0 if step % 2 == 0 else 1e-3) for p in ms[0].parameters()]     # clipped / unclipped at 10
        for m in ms:
            _set_grads(m, grads)
            for b in m.buffers():
                if b.dtype.is_floating_point:
                    b.add_(0.01 * (step + 1))
        for gr in opts[0].param_groups + opts[1].param_groups:
            gr["lr"] = 1e-3 / (step + 1)
            if step == 3:
                gr["betas"] = (0.9, 0.99)
        opts[0].step()
        want_norm = _torch_step(ms[1], opts[1])
        emas[1].update(ms[1])
        assert (float(want_norm) > 10.0) == (step % 2 == 0)
        assert abs(float(opts[0].grad_norm) - float(want_norm)) <= 1e-4 * float(want_norm)
        assert all(float(p.grad.abs().max()) == 0.0 for p in ms[0].parameters())
    # the fused table really used the two non-plain gradient layouts
    assert any(L.optim._is_tap_major(p.grad, p) for p in ms[0].parameters())
    assert any(getattr(p, "_ly_grad_pair", None) is not None and p.grad.untyped_storage().data_ptr() == p._ly_grad_pair.grad.untyped_storage().data_ptr()
               for p in ms[0].parameters())
    assert emas[0].updates == emas[1].updates == 6
    for (k, a), b in zip(ms[0].state_dict().items(), ms[1].state_dict().values()):
        if a.dtype.is_floating_point:
            _near(a, b, k)
    for (k, a), b in zip(emas[0].ema.state_dict().items(), emas[1].ema.state_dict().values()):
        if a.dtype.is_floating_point:
            _near(a, b, ("ema", k))
    ma, mb = _moments(opts[0], ms[0]), _moments(opts[1], ms[1])
    assert ma.keys() == mb.keys() and len(ma) > 100
    for k in ma:
        _near(ma[k][0], mb[k][0], ("exp_avg", k))
        _near(ma[k][1], mb[k][1], ("exp_avg_sq", k))
    assert all(float(opts[1].state[p]["step"]) == 6.0 for p in ms[1].parameters())
    assert all(float(st["step"]) == 6.0 for st in opts[0].state_dict()["state"].values())


def test_fused_adamw_checkpoints_both_ways():
    """torch AdamW 3 steps -> state_dict -> FusedAdamW.load_state_dict -> 3 more steps on each agree; FusedAdamW 3 steps -> torch AdamW
    loads step 3.0 and continues alike; a state with one parameter's entry removed: that parameter takes torch's first step, the others
    their seventh"""
    import lead_yolo_amd as L
    a, b = _model(), _model()
    ta = L.smart_optimizer(a, "AdamW", 1e-3, 0.937, 5e-4, fused=False)
    fb = L.smart_optimizer(b, "AdamW", 1e-3, 0.937, 5e-4, fused=True)
    g = torch.Generator().manual_seed(2)
    grads = [[torch.randn(p.shape, generator=g) * 1e-2 for p in a.parameters()] for _ in range(7)]
    for k in range(3):
        _set_grads(a, grads[k])
        _torch_step(a, ta)
        _set_grads(b, grads[k])
        fb.step()
    sd_t, sd_f = copy.deepcopy(ta.state_dict()), copy.deepcopy(fb.state_dict())
    assert all(float(st["step"]) == 3.0 and st["step"].dtype == torch.float32 and not st["step"].is_cuda for st in sd_f["state"].values())
    # torch -> fused (d) and fused -> torch (c), from the torch run's weights
    c, d = _model(), _model()
    c.load_state_dict(a.state_dict())
    d.load_state_dict(a.state_dict())
    tc = L.smart_optimizer(c, "AdamW", 1e-3, 0.937, 5e-4, fused=False)
    tc.load_state_dict(sd_f)
    assert all(float(st["step"]) == 3.0 for st in tc.state.values())
    fd = L.smart_optimizer(d, "AdamW", 1e-3, 0.937, 5e-4, fused=True)
    fd.load_state_dict(sd_t)
    for k in range(3, 6):
        for m, o in ((a, ta), (c, tc)):
            _set_grads(m, grads[k])
            _torch_step(m, o)
        _set_grads(d, grads[k])
        fd.step()
    for (k, x), y, z in zip(a.state_dict().items(), c.state_dict().values(), d.state_dict().values()):
        if x.dtype.is_floating_point:
            _near(z, x, ("torch -> fused", k))
            _near(y, x, ("fused -> torch", k), rel=1e-4)       # (c began from the fused run's moments)
    mt, mf = _moments(ta, a), _moments(fd, d)
    for k in mt:
        _near(mf[k][0], mt[k][0], ("exp_avg", k))
        _near(mf[k][1], mt[k][1], ("exp_avg_sq", k))
    assert all(float(st["step"]) == 6.0 for st in fd.state_dict()["state"].values())
    # one parameter without state
    e, f = _model(), _model()
    e.load_state_dict(a.state_dict())
    f.load_state_dict(a.state_dict())
    sd = copy.deepcopy(ta.state_dict())
    drop = 7
    del sd["state"][drop]
    te = L.smart_optimizer(e, "AdamW", 1e-3, 0.937, 5e-4, fused=False)
    te.load_state_dict(sd)
    ff = L.smart_optimizer(f, "AdamW", 1e-3, 0.937, 5e-4, fused=True)
    ff.load_state_dict(copy.deepcopy(sd))
    _set_grads(e, grads[6])
    _torch_step(e, te)
    _set_grads(f, grads[6])
    ff.step()
    for (k, x), y in zip(e.state_dict().items(), f.state_dict().values()):
        if x.dtype.is_floating_point:
            _near(y, x, ("partial state", k))
    steps = {i: float(st["step"]) for i, st in ff.state_dict()["state"].items()}
    assert steps[drop] == 1.0 and all(s == 7.0 for i, s in steps.items() if i != drop)
    assert steps == {i: float(st["step"]) for i, st in te.state_dict()["state"].items()}


@pytest.mark.parametrize("amp", [None, torch.bfloat16])
def test_graphed_adamw_step_matches_eager(amp):
    """the captured step with FusedAdamW: from one restored state (weights, BatchNorm statistics, Adam moments, EMA, hyper with T), two
    eager steps and one graph replay leave the same bits in every weight, EMA entry and moment"""
    import lead_yolo_amd as L
    from lead_yolo_amd import pack
    m = _model()
    opt = L.smart_optimizer(m, "AdamW", 1e-3, 0.937, 5e-4)
    assert isinstance(opt, L.FusedAdamW)
    ema = L.ModelEMA(m)
    cl = L.ComputeLoss(m)
    batches = [(synth.synth_images(4, 128, 21 + i).to(_dev()), synth.synth_targets(4, 22 + i, per_image=3).to(_dev())) for i in range(2)]
    nt = max(t.shape[0] for _, t in batches) + 2
    batches = [(im, torch.cat((t, torch.full((nt - t.shape[0], 6), -1.0, device=_dev())))) for im, t in batches]
    step = L.GraphedTrainStep(m, cl, opt, *batches[0], ema=ema, amp=amp, warmup=2)

    def tensors():
        return (("weight", {k: v for k, v in m.state_dict().items() if v.is_floating_point()}),
                ("ema", {k: v for k, v in ema.ema.state_dict().items() if v.is_floating_point()}),
                ("exp_avg", {n: opt.state[p]["exp_avg"] for n, p in m.named_parameters() if p in opt.state}),
                ("exp_avg_sq", {n: opt.state[p]["exp_avg_sq"] for n, p in m.named_parameters() if p in opt.state}))

    def snap():
        torch.cuda.synchronize()
        return [{k: v.detach().clone() for k, v in d.items()} for _, d in tensors()], opt._table["hyper"].clone(), ema.updates

    def restore(state):
        with torch.no_grad():
            for (_, live), saved in zip(tensors(), state[0]):
                for k, v in live.items():
                    v.copy_(saved[k])
            opt._table["hyper"].copy_(state[1])
        ema.updates = state[2]
        pack.touch_weights()

    s0 = snap()
    assert float(s0[1][11]) == 2.0                       # T: the two warm-up steps (the capture launched nothing)
    outs = []
    for how in ("eager", "eager", "graph"):
        restore(s0)
        if how == "graph":
            loss, _ = step(*batches[1])
        else:
            loss, _ = L.train_step(m, cl, opt, *batches[1], ema=ema, amp=amp)
        after = snap()
        assert after[2] == s0[2] + 1 and float(after[1][11]) == 3.0
        outs.append((float(loss), after[0]))
    (le, e), (le2, e2), (lg, g) = outs
    tight = 1e-6 if amp is None else 1e-5
    assert abs(le - lg) <= tight * abs(le) and abs(le - le2) <= tight * abs(le), (le, le2, lg)
    for wi, (what, _) in enumerate(tensors()):
        a, a2, b = e[wi], e2[wi], g[wi]
        assert a.keys() == b.keys() == a2.keys() and len(a) > 100
        bad_e = [k for k in a if not torch.equal(a[k], a2[k])]
        bad_g = [k for k in a if not torch.equal(a[k], b[k])]
        assert not bad_e, (what, "two eager steps differ", len(bad_e), bad_e[:6])
        assert not bad_g, (what, "graph replay differs from the eager step", len(bad_g), bad_g[:6])
        moved = sum(not torch.equal(a[k], s0[0][wi][k]) for k in a)
        assert moved > 0.9 * len(a), (what, "the step did not move the state", moved, len(a))


@pytest.mark.parametrize("amp", [None, torch.bfloat16])
def test_adamw_step_is_bit_reproducible(amp):
    """two eager FusedAdamW steps from one state (weights, BatchNorm statistics, moments, EMA, T) leave the same bits"""
    import lead_yolo_amd as L
    m = _model(7373)
    cl = L.ComputeLoss(m)
    opt = L.smart_optimizer(m, "AdamW", 1e-3, 0.937, 5e-4, fused=True)
    ema = L.ModelEMA(m)
    imgs = synth.synth_images(4, 160, 71).to(_dev())
    tg = synth.synth_targets(4, 72, per_image=4).to(_dev())
    L.train_step(m, cl, opt, imgs, tg, ema=ema, amp=amp)
    live = lambda: [m.state_dict(), ema.ema.state_dict(), {n: v for n, (v, _) in _moments(opt, m).items()},           # noqa: E731
                    {n: v for n, (_, v) in _moments(opt, m).items()}]
    s0 = [{k: v.detach().clone() for k, v in d.items()} for d in live()]
    h0, u0 = opt._table["hyper"].clone(), ema.updates
    ends = []
    for _ in range(2):
        with torch.no_grad():
            for d, saved in zip(live(), s0):
                for k, v in d.items():
                    v.copy_(saved[k])
            opt._table["hyper"].copy_(h0)
        ema.updates = u0
        from lead_yolo_amd import pack
        pack.touch_weights()
        L.train_step(m, cl, opt, imgs, tg, ema=ema, amp=amp)
        torch.cuda.synchronize()
        ends.append([{k: v.detach().clone() for k, v in d.items()} for d in live()])
    for what, a, b, s in zip(("weight", "ema", "exp_avg", "exp_avg_sq"), ends[0], ends[1], s0):
        bad = [k for k in a if not torch.equal(a[k], b[k])]
        assert not bad, (what, len(bad), bad[:8])
        assert sum(not torch.equal(a[k], s[k]) for k in a if a[k].is_floating_point()) > 0.5 * len(a), what


@pytest.mark.parametrize("rccl,accumulate,form", [(False, 1, "overlapped"), (True, 1, "overlapped"), (True, 1, "serial"), (False, 1, "serial"),
                                                  (True, 2, "overlapped"), (True, 1, "probe"), (False, 1, "probe")])
def test_graphed_adamw_step_with_reducer_matches_eager(rccl, accumulate, form, monkeypatch):
    """the data-parallel captured step (graph A, per-bucket exchange, graph B = FusedAdamW dividing by the world size) against eager
    train_step with the same reducer, as tests/test_gpu_backward.py checks it with FusedSGD; the exchange probe must put the Adam moments
    and the step counter back exactly"""
    import lead_yolo_amd as L
    dist = _one_rank_group() if rccl else None
    probed = []
    choose = L.GraphedTrainStep._choose_exchange

    def spy(self):
        before = [t.clone() for t in self.optimizer.device_state()]
        choose(self)
        torch.cuda.synchronize()
        after = self.optimizer.device_state()
        probed.append(self.dp_probe is not None)
        assert len(before) == len(after) and all(torch.equal(x, y) for x, y in zip(before, after)), "the probe did not restore the optimiser state"

    monkeypatch.setattr(L.GraphedTrainStep, "_choose_exchange", spy)
    try:
        runs = []
        for graphed in (False, True):
            m = _model()
            red = L.GradReducer(list(m.parameters())).attach()
            red.exchange_single = rccl
            opt = L.smart_optimizer(m, "AdamW", 1e-3, 0.937, 5e-4)
            ema = L.ModelEMA(m)
            cl = L.ComputeLoss(m)
            data = [(synth.synth_images(4, 128, 21 + i).to(_dev()), synth.synth_targets(4, 22, per_image=3).to(_dev())) for i in range(2)]
            losses = []
            if graphed:
                step = L.GraphedTrainStep(m, cl, opt, *data[0], ema=ema, warmup=2, reducer=red, world_size=1, accumulate=accumulate, dp_exchange=form)
                assert float(opt._table["hyper"][11]) == 2.0 and ema.updates == 2
                if form == "probe" and rccl:
                    assert probed == [True] and step.dp_probe["ranks"] == 1
                for _ in range(3):
                    for j in range(accumulate):
                        loss, _ = step(*data[j % 2])
                        assert step.stepped == (j == accumulate - 1)
                    losses.append(float(loss))
            else:
                for i in range(5):
                    if accumulate == 1 or i < 2:
                        loss, _ = L.train_step(m, cl, opt, *data[0], ema=ema, reducer=red)
                    else:
                        red.reset()
                        with red.no_sync():
                            for j in range(accumulate - 1):
                                L.forward_backward(m, cl, *data[j % 2])
                        loss, _ = L.forward_backward(m, cl, *data[(accumulate - 1) % 2])
                        red.wait()
                        L.optimizer_step(m, opt, ema=ema, reducer=red)
                    if i >= 2:
                        losses.append(float(loss))
            red.detach()
            assert float(opt._table["hyper"][11]) == 5.0
            runs.append((losses, {k: v.detach().clone() for k, v in m.state_dict().items() if v.is_floating_point()}, ema.updates))
        (l0, w0, u0), (l1, w1, u1) = runs
        assert u0 == u1 == 5
        for a, b in zip(l0, l1):
            assert abs(a - b) <= 1e-2 * abs(a), runs
        for k in w0:
            assert float((w0[k] - w1[k]).abs().max()) <= 1e-1 * float(w0[k].abs().max()) + 1e-4, k
    finally:
        if dist is not None and dist.is_initialized():
            dist.destroy_process_group()


def test_adamw_training_trajectory_tracks_torch():
    """8 train_steps of lead-yolo-n at 128 px with FusedAdamW (lr 1e-3) against the same steps with torch.optim.AdamW (fused=False) on
    the same HIP forward / backward: the loss falls and the two trajectories agree within the bands of the SGD trajectory test"""
    import lead_yolo_amd as L
    imgs = synth.synth_images(4, 128, 31).to(_dev())
    tg = synth.synth_targets(4, 32, per_image=3).to(_dev())
    traj = []
    for fused in (False, True):
        m = _model(8181)
        opt = L.smart_optimizer(m, "AdamW", 1e-3, 0.937, 5e-4, fused=fused)
        assert isinstance(opt, L.FusedAdamW) == fused
        cl = L.ComputeLoss(m)
        traj.append([float(L.train_step(m, cl, opt, imgs, tg)[0]) for _ in range(8)])
    want, got = traj
    for i, (a, b) in enumerate(zip(got, want)):
        tol = (1e-4, 1e-3, 5e-3)[i] if i < 3 else 3e-2
        assert abs(a - b) <= tol * abs(b), (got, want)
    assert got[-1] < got[0] and want[-1] < want[0], (got, want)
