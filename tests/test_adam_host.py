"""Host side of the fused Adam / AdamW optimisers (CPU): smart_optimizer builds the reference's torch objects for every name it knows
(utils/torch_utils.py:318-346) and the fused classes refuse what their kernel does not implement."""
import pytest
import torch

import lead_yolo_amd as L


def _model():
    torch.manual_seed(0)
    return L.Model(L.load_cfg(scale="n"))


@pytest.mark.parametrize("name,cls", [("Adam", torch.optim.Adam), ("AdamW", torch.optim.AdamW)])
def test_smart_optimizer_builds_the_reference_adam_objects(name, cls):
    m = _model()
    opt = L.smart_optimizer(m, name, 1e-3, 0.937, 5e-4, fused=False)
    assert type(opt) is cls
    bias, dec, norm = L.train.param_groups(m)
    assert [g["params"] for g in opt.param_groups] == [bias, dec, norm]
    assert [g["weight_decay"] for g in opt.param_groups] == [0.0, 5e-4, 0.0]        # AdamW's bias group too: explicit 0.0, not 0.01
    for g in opt.param_groups:
        assert tuple(g["betas"]) == (0.937, 0.999) and g["lr"] == 1e-3
        assert not g["amsgrad"]
    assert opt.param_groups[0]["decoupled_weight_decay"] == (name == "AdamW")


def test_smart_optimizer_defaults_to_torch_on_cpu_and_knows_rmsprop():
    m = _model()
    assert type(L.smart_optimizer(m, "AdamW", 1e-3, 0.9, 1e-4)) is torch.optim.AdamW          # fused=None, CPU parameters
    assert type(L.smart_optimizer(m, "SGD", 1e-2, 0.9, 1e-4)) is torch.optim.SGD
    rms = L.smart_optimizer(m, "RMSProp", 1e-3, 0.9, 1e-4, fused=False)
    assert type(rms) is torch.optim.RMSprop
    assert rms.param_groups[0]["momentum"] == 0.9 and [g["weight_decay"] for g in rms.param_groups] == [0, 1e-4, 0.0]
    with pytest.raises(NotImplementedError):
        L.smart_optimizer(m, "RMSProp", 1e-3, 0.9, 1e-4, fused=True)        # no fused RMSProp, and no quiet fall-back to torch
    with pytest.raises(NotImplementedError):
        L.smart_optimizer(m, "Adagrad", 1e-3, 0.9, 1e-4, fused=False)


def test_fused_adam_refuses_what_it_does_not_implement():
    ps = list(_model().parameters())[:4]
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True)):
        with pytest.raises(NotImplementedError):
            L.FusedAdam(ps, lr=1e-3, **kw)
        with pytest.raises(NotImplementedError):
            L.FusedAdamW(ps, lr=1e-3, **kw)
    opt = L.FusedAdamW(ps, lr=1e-3, betas=(0.9, 0.999))
    assert opt.param_groups[0]["decoupled_weight_decay"] and not L.FusedAdam(ps).param_groups[0]["decoupled_weight_decay"]


def test_fused_adam_state_dict_loads_into_torch_adamw_and_back():
    """no step taken, no device needed: the group flags make the fused object's state dict a torch.optim.AdamW one, and a torch state
    dict sets the fused object's step counter and per-parameter offsets"""
    ps = list(_model().parameters())[:3]
    fused = L.FusedAdamW(ps, lr=1e-3, betas=(0.937, 0.999), weight_decay=0.0)
    ref = torch.optim.AdamW(ps, lr=1e-2)
    ref.load_state_dict(fused.state_dict())
    assert ref.param_groups[0]["decoupled_weight_decay"] and ref.param_groups[0]["lr"] == 1e-3
    for p in ps:
        p.grad = torch.randn_like(p)
    ref.step()
    ref.step()
    sd = ref.state_dict()
    del sd["state"][1]                                   # a parameter with no state yet
    fused.load_state_dict(sd)
    assert fused._T == 2 and fused._step0[ps[0]] == 0 and ps[1] not in fused._step0
    back = fused.state_dict()
    assert set(back["state"]) == {0, 2} and float(back["state"][0]["step"]) == 2.0 and back["state"][0]["step"].dtype == torch.float32
