"""Training with frozen layers (the reference's `--freeze N`: requires_grad = False on `model.0.` .. `model.{N-1}.`, model left in
.train()) — the premises of tests/test_gpu_freeze.py, asserted on the CPU, and the oracle runs that file compares the device with.

The reference of every frozen run is autograd through oracle/functional.py plus its SGD-nesterov restatement, on lead-yolo-n at
128 x 128, batch 4: the recipe of test_training_trajectory_vs_oracle.  A mask is a number of frozen layers; a schedule is one mask per step.
A parameter that starts training later starts without a momentum buffer (torch.optim.SGD's rule for a parameter whose gradient was None)."""
import functools

import pytest
import torch

from oracle import functional as OF
from oracle import synth

LR, MOM, WD, CLIP = 0.01, 0.937, 5e-4, 10.0
BOUNDS = (1e-4, 1e-3, 5e-3, 3e-2)            # per-step relative loss bounds of test_training_trajectory_vs_oracle
# schedules the device tests run: constant masks, (a) one unfrozen step then the backbone frozen, (b) frozen warm-up then everything
SCHEDULES = {"none": (0, 0, 0, 0), "freeze4": (4, 4, 4, 4), "freeze9": (9, 9, 9, 9), "a": (0, 9, 9), "b": (9, 9, 0, 0)}
# the issue's table (four oracle steps, checked on the CPU)
TABLE = {"none": (17.3044, 15.3600, 12.9518, 10.5378), "freeze4": (17.3044, 15.2959, 12.8990, 10.4259), "freeze9": (17.3044, 15.1378, 12.4783, 9.9535)}


def prefixes(n):
    return tuple(f"model.{i}." for i in range(n))


def is_param(k, v):
    return v.is_floating_point() and "running" not in k and not k.endswith("anchors")


@functools.lru_cache(maxsize=None)
def setup():
    """-> (cfg, CPU model, initial state, uint8 images, targets) of the whole-model cases"""
    import lead_yolo_amd as L
    cfg = L.load_cfg(scale="n")
    torch.manual_seed(0)
    m = L.Model(cfg)
    st = synth.synth_state(synth.shapes_of(m.state_dict()), 8181)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    return cfg, m, st, synth.synth_images(4, 128, 31), synth.synth_targets(4, 32, per_image=3)


class Run:
    """one oracle run: losses[i], totals[i] (pre-clip norm over the trainable gradients), grads[i] (of step i, trainable names only),
    states[i] (every state entry after step i)"""

    def __init__(self):
        self.losses, self.totals, self.grads, self.states = [], [], [], []


@functools.lru_cache(maxsize=None)
def oracle_run(schedule):
    """the oracle taking len(schedule) optimisation steps, step i with layers 0 .. schedule[i]-1 frozen.  Computed once per schedule; the
    result is shared and must be left unchanged."""
    cfg, m, st, imgs, tg = setup()
    so = {k: v.clone() for k, v in st.items()}
    names = [k for k, v in so.items() if is_param(k, v)]
    groups = OF.param_groups(list(so))
    bufs, run = {}, Run()
    for nf in schedule:
        train = [k for k in names if not k.startswith(prefixes(nf))]
        for k in names:
            so[k].requires_grad_(k in train)
            so[k].grad = None
        pred = OF.model_forward(so, cfg, imgs.float() / 255, m.stride, training=True)
        loss, _ = OF.compute_loss(pred, tg, so["model.23.anchors"], nc=1)
        loss.backward()
        run.losses.append(float(loss.detach()))
        grads = {k: so[k].grad for k in train}
        run.grads.append({k: g.clone() for k, g in grads.items()})
        total = torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())).float()
        run.totals.append(float(total))
        coef = torch.clamp(CLIP / (total + 1e-6), max=1.0)
        grads = {k: g * coef for k, g in grads.items()}
        with torch.no_grad():
            for gname, dec in (("decay", WD), ("bn", 0.0), ("bias", 0.0)):
                OF.sgd_nesterov_step({k: so[k] for k in groups[gname] if k in grads}, grads, bufs, LR, MOM, dec)
        run.states.append({k: v.detach().clone() for k, v in so.items()})
    return run


def rel(a, b):
    return abs(a - b) / abs(b)


def test_freeze_layers_equals_the_reference_rule():
    """freeze_layers(model, N | list) against the reference's loop written out: `model.{i}.` for i in range(N) (a one-element list means
    the same) or for the listed layers; every other parameter back to True.  186 parameter tensors, 138 trainable at freeze 9, 170 at 4."""
    import lead_yolo_amd as L
    _, m, _, _, _ = setup()
    names = [k for k, _ in m.named_parameters()]
    assert len(names) == 186
    try:
        for arg, want_trainable in ((9, 138), (4, 170), ([9], 138), ([0, 1, 5], None), ([23, 2], None), (0, 186), ([0], 186)):
            freeze = arg if isinstance(arg, list) else [arg]
            pre = [f"model.{x}." for x in (freeze if len(freeze) > 1 else range(freeze[0]))]
            want = {k: not any(x in k for x in pre) for k in names}
            for p in m.parameters():
                p.requires_grad_(False)                      # whatever was set before must not matter
            frozen = L.freeze_layers(m, arg)
            got = {k: p.requires_grad for k, p in m.named_parameters()}
            assert got == want, arg
            assert sorted(frozen) == sorted(k for k, v in want.items() if not v)
            if want_trainable is not None:
                assert sum(got.values()) == want_trainable, (arg, sum(got.values()))
        # the oracle runs below freeze by the same prefixes
        L.freeze_layers(m, 9)
        assert {k for k, p in m.named_parameters() if not p.requires_grad} == {k for k in names if k.startswith(prefixes(9))}
        assert m.training                                    # the mode is not touched
    finally:
        L.freeze_layers(m, 0)


def test_oracle_frozen_trajectories_separate():
    """the issue's table, and what makes it a test: a step that ignored the mask would follow the unfrozen trajectory, which leaves the
    freeze-9 one by more than each step's bound; frozen weights move by exactly 0, the frozen layers' running statistics do move"""
    _, _, st, _, _ = setup()
    for name, want in TABLE.items():
        got = oracle_run(SCHEDULES[name]).losses
        assert all(abs(a - b) <= 1e-3 for a, b in zip(got, want)), (name, got, want)
    none, f9 = oracle_run(SCHEDULES["none"]), oracle_run(SCHEDULES["freeze9"])
    assert none.losses[0] == f9.losses[0]
    sep = [rel(f9.losses[i], none.losses[i]) / BOUNDS[i] for i in range(4)]
    # above the bound at every later step; above TWICE the bound (a device run may sit one bound away from its own trajectory) at two of them
    assert min(sep[1:]) > 1.0 and sep[1] > 2.0 and sep[2] > 2.0, (sep, f9.losses, none.losses)
    for name, nf in (("freeze4", 4), ("freeze9", 9)):
        end = oracle_run(SCHEDULES[name]).states[-1]
        frozen = [k for k, v in st.items() if is_param(k, v) and k.startswith(prefixes(nf))]
        assert len(frozen) == 186 - (170 if nf == 4 else 138)
        assert all(torch.equal(end[k], st[k]) for k in frozen)
        moved = max(float((end[k].float() - st[k].float()).abs().max()) for k in st if k.startswith(prefixes(nf)) and "running" in k)
        assert moved > 0.1, (name, moved)
        assert any(not torch.equal(end[k], st[k]) for k in st if is_param(k, st[k]) and not k.startswith(prefixes(nf)))
    assert 0.4 < max(float((f9.states[-1][k].float() - st[k].float()).abs().max()) for k in st if k.startswith(prefixes(9)) and "running" in k) < 0.6


@pytest.mark.parametrize("name,const", [("a", "none"), ("a", "freeze9"), ("b", "none")])
def test_oracle_schedules_separate_from_constant_masks(name, const):
    """a device step that kept the FIRST mask of a schedule, or never left the other one, follows a constant-mask trajectory: the schedule
    leaves it by more than twice the step's bound (a device run may sit one bound away from its own trajectory) at a step the device test
    compares.
    The fourth pair is missing on purpose.  Schedule (b) can leave the constant freeze-9 run only at its last step, one unfrozen update
    after the two share their state, and that moves the loss by 7.2e-3 (9.9535 -> 10.0253), a quarter of that step's 3e-2 bound: the
    LOSSES of (b) cannot tell "never unfroze" from "unfroze".  The backbone weights can — they move by exactly 0 under the constant mask
    and in both of (b)'s last steps (the next test) — and that is what the device test of (b) asserts next to the loss bounds."""
    run, ref = oracle_run(SCHEDULES[name]).losses, oracle_run(SCHEDULES[const]).losses
    sep = [rel(a, b) / BOUNDS[i] for i, (a, b) in enumerate(zip(run, ref))]
    assert max(sep) > 2.0, (name, const, run, ref, sep)


def test_oracle_schedule_b_loss_stays_inside_the_bound_of_the_constant_freeze():
    """the figure behind the missing pair above, kept as an assertion so that it cannot go stale"""
    run, ref = oracle_run(SCHEDULES["b"]).losses, oracle_run(SCHEDULES["freeze9"]).losses
    assert run[:3] == ref[:3] and 0.1 < rel(run[3], ref[3]) / BOUNDS[3] < 0.5, (run, ref)


def test_oracle_schedule_states_follow_the_mask():
    """(a): the backbone stands still over the two frozen steps after having moved in the first; (b): it stands still for two steps and
    moves in each of the last two"""
    _, _, st, _, _ = setup()
    back = [k for k, v in st.items() if is_param(k, v) and k.startswith(prefixes(9))]
    a, b = oracle_run(SCHEDULES["a"]).states, oracle_run(SCHEDULES["b"]).states
    assert any(not torch.equal(a[0][k], st[k]) for k in back) and all(torch.equal(a[2][k], a[0][k]) for k in back)
    assert all(torch.equal(b[1][k], st[k]) for k in back)
    assert any(not torch.equal(b[2][k], b[1][k]) for k in back) and any(not torch.equal(b[3][k], b[2][k]) for k in back)


def test_oracle_trainable_norm_is_not_the_full_norm():
    """the clip norm of a frozen step covers the trainable gradients only; the trainable gradients themselves do not depend on the mask, so
    the unfrozen run's first gradient restricted to the trainable set is the reference of every mask"""
    none, f9, f4 = (oracle_run(SCHEDULES[k]) for k in ("none", "freeze9", "freeze4"))
    for run, n in ((f9, 138), (f4, 170)):
        assert len(run.grads[0]) == n and len(none.grads[0]) == 186
        for k, g in run.grads[0].items():
            assert torch.equal(g, none.grads[0][k]), k
        assert any(float(g.abs().max()) > 0 for g in run.grads[0].values())
    assert rel(f9.totals[0], none.totals[0]) > 1e-2, (f9.totals[0], none.totals[0])


def test_grad_sink_gives_no_target_for_a_frozen_parameter():
    """ops.GradSink.target: the persistent storage only while the parameter requires grad (a parameter frozen after the optimiser built
    its table keeps its id in `targets` until the next step rebuilds it)"""
    from lead_yolo_amd import ops
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.zeros(3)
    sink = ops.GradSink()
    sink.targets = {id(p): p.grad}
    assert sink.target(p) is p.grad and sink.writes == 1
    p.requires_grad_(False)
    assert sink.target(p) is None and sink.writes == 1
    p.requires_grad_(True)
    assert sink.target(p) is p.grad


def test_reducer_buckets_hold_trainable_parameters_and_refuse_a_changed_mask():
    """ddp.GradReducer: buckets over the parameters that require grad at construction; reset() — the start of every step — raises once the
    flags differ, in both directions, and accepts the old mask again"""
    from lead_yolo_amd.ddp import GradReducer
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in (3, 5, 7)]
    ps[1].requires_grad_(False)
    red = GradReducer(ps)
    assert sum(b["flat"].numel() for b in red.buckets) == 10 and ps[1].grad is None
    red.reset()
    for i in (1, 0):
        ps[i].requires_grad_(not ps[i].requires_grad)
        with pytest.raises(RuntimeError, match="rebuild"):
            red.reset()
        ps[i].requires_grad_(not ps[i].requires_grad)
        red.reset()
