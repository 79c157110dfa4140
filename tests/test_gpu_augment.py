"""Augmented inference (augment=True) on the device path: ly_scale_img against F.interpolate + flip + F.pad, the whole augmented forward
against the reference's _forward_augment restated here over the CPU oracle, bit-exact pins of the pruning and of the descale, the captured
graph, bf16, and the val.py --augment pipeline on SSDD images."""
import copy
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import functional as OF
from oracle import nms as ONMS
from oracle import synth
from tests.test_gpu_bf16 import MAX_REL, REL_L2, _close
from tests.test_gpu_modules import _cfg, _cmp, _dev
from tests.test_val_pipeline import _batch, _iou

pytestmark = pytest.mark.gpu


# ---- the reference, restated (models/yolo.py:127-160 _forward_augment / _descale_pred / _clip_augmented, utils/torch_utils.py scale_img) --
def ref_scale_img(img, ratio=1.0, same_shape=False, gs=32):
    if ratio == 1.0:
        return img
    h, w = img.shape[2:]
    s = (int(h * ratio), int(w * ratio))
    img = F.interpolate(img, size=s, mode="bilinear", align_corners=False)
    if not same_shape:
        h, w = (math.ceil(x * ratio / gs) * gs for x in (h, w))
    return F.pad(img, [0, w - s[1], 0, h - s[0]], value=0.447)


def ref_clip_augmented(y, nl):
    g = sum(4 ** x for x in range(nl))
    e = 1
    i = (y[0].shape[1] // g) * sum(4 ** x for x in range(e))
    y[0] = y[0][:, :-i]
    i = (y[-1].shape[1] // g) * sum(4 ** (nl - 1 - x) for x in range(e))
    y[-1] = y[-1][:, i:]
    return y


def ref_forward_augment(st, cfg, x, stride, nl=3):
    img_size = x.shape[-2:]
    s, f = [1, 0.83, 0.67], [None, 3, None]
    y = []
    for si, fi in zip(s, f):
        xi = ref_scale_img(x.flip(fi) if fi else x, si, gs=int(stride.max()))
        yi = OF.model_forward(copy.deepcopy(st), cfg, xi, stride, training=False)[0]
        yi[..., :4] /= si
        if fi == 3:
            yi[..., 0] = img_size[1] - yi[..., 0]
        y.append(yi)
    y = ref_clip_augmented(y, nl)
    return torch.cat(y, 1)


def _model(scale, seed):
    import lead_yolo_amd as L
    torch.manual_seed(0)
    m = L.Model(_cfg(scale))
    st = synth.synth_state(synth.shapes_of(m.state_dict()), seed)
    st["model.23.anchors"] = m.model[-1].anchors.clone()
    m.load_state_dict(st)
    return m, st


@functools.lru_cache(maxsize=None)
def _oracle(scale, hw, bs, seed):
    m, st = _model(scale, seed)
    x = synth.synth_images(bs, max(hw), 11)[:, :, :hw[0], :hw[1]].float() / 255
    with torch.no_grad():
        zo = ref_forward_augment(st, _cfg(scale), x, m.stride)
    return x, zo


# ---- 4. ly_scale_img ---------------------------------------------------------------------------------------------------------------------
_SPECS = [(0.83, False), (0.83, True), (0.67, False), (0.67, True)]


def _specs(h, w):
    out = []
    for r, fl in _SPECS:
        hs, ws = int(h * r), int(w * r)
        ho, wo = (math.ceil(v * r / 32) * 32 for v in (h, w))
        out.append((hs, ws, ho, wo, fl))
    return out


def _ref_images(x, h, w):
    return [ref_scale_img(x.flip(3) if fl else x, r, gs=32) for r, fl in _SPECS]


@pytest.mark.parametrize("hw", [(640, 640), (320, 320), (640, 480), (96, 160)])
def test_scale_img_fp32_matches_interpolate(hw):
    from lead_yolo_amd import ops
    h, w = hw
    x = torch.rand((2, 3, h, w), generator=torch.Generator().manual_seed(h + w))
    got = ops.scale_img(x.to(_dev()), _specs(h, w))
    for g, want, sp in zip(got, _ref_images(x, h, w), _SPECS):
        assert g.shape == want.shape and g.dtype == torch.float32, (hw, sp)
        err = float((g.cpu() - want).abs().max())
        assert err <= 2e-6, (hw, sp, err)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("hw", [(640, 640), (320, 320), (640, 480), (96, 160)])
def test_scale_img_16bit_within_one_ulp(hw, dtype):
    """a 16-bit image is resampled in fp32 and rounded once: within 1 ulp of the fp32 resample of the same image rounded to the type"""
    from lead_yolo_amd import ops
    h, w = hw
    x = torch.rand((2, 3, h, w), generator=torch.Generator().manual_seed(h * w)).to(dtype)
    got = ops.scale_img(x.to(_dev()), _specs(h, w))
    for g, want, sp in zip(got, _ref_images(x.float(), h, w), _SPECS):
        assert g.dtype == dtype and g.shape == want.shape
        a = g.cpu().view(torch.int16).int()              # values are >= 0: adjacent bit patterns are adjacent values
        b = want.to(dtype).view(torch.int16).int()
        d = int((a - b).abs().max())
        assert d <= 1, (hw, sp, dtype, d)


def test_scale_img_rejects_bad_specs():
    from lead_yolo_amd import capi, ops
    x = torch.rand((1, 3, 64, 64), device=_dev())
    with pytest.raises(capi.HipLibraryError):
        ops.scale_img(x, [(53, 53, 64, 62, False)])                          # Wo not a multiple of 4 fp32 columns
    with pytest.raises(capi.HipLibraryError):
        ops.scale_img(x, [(70, 53, 64, 64, False)])                          # resized larger than the canvas


# ---- 5. whole model, fp32, against the restated reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("scale,hw,bs", [("s", (640, 640), 2), ("n", (640, 480), 2)])
def test_augmented_forward_vs_oracle(scale, hw, bs):
    seed = 7100 + hw[1]
    x, zo = _oracle(scale, hw, bs, seed)
    m, _ = _model(scale, seed)
    m = m.to(_dev()).eval()
    with torch.no_grad():
        z, p = m(x.to(_dev()), augment=True)
    assert p is None and z.dtype == torch.float32
    if hw == (640, 640):
        assert tuple(z.shape) == (bs, 45147, 6)
    _cmp(z, zo, f"augmented {scale} {hw}")


# ---- 6. bit-exact pins -----------------------------------------------------------------------------------------------------------------
def test_augmented_rows_bit_exact_pins():
    """the scale-1 rows are the plain forward's first two levels (the pruned layers change nothing); the 0.83 rows are the plain forward of
    the device-resampled flipped image, descaled with torch's `/=` and img_w - x"""
    from lead_yolo_amd import ops
    m, _ = _model("s", 7200)
    m = m.to(_dev()).eval()
    x = (synth.synth_images(2, 640, 5).float() / 255).to(_dev())
    plan = m.augment_plan(640, 640)
    p0, p1 = plan["passes"][0], plan["passes"][1]
    with torch.no_grad():
        z, _ = m(x, augment=True)
        z_plain = m(x)[0]
        img = ops.scale_img(x, [(*p1["resized"], *p1["size"], True)])[0]
        z1 = m(img)[0].cpu()
    assert torch.equal(z[:, :p0["rows"]], z_plain[:, :p0["rows"]])
    z1[..., :4] /= 0.83                       # on the CPU: a true division, as the reference's CPU and the kernel compute it
    z1[..., 0] = 640 - z1[..., 0]
    got = z[:, p1["offset"]:p1["offset"] + p1["rows"]].cpu()
    assert got.shape == z1.shape and torch.equal(got, z1)


# ---- 7. graph ----------------------------------------------------------------------------------------------------------------------
def test_graphed_augmented_forward_matches_eager():
    import lead_yolo_amd as L
    m, _ = _model("s", 7300)
    m = m.to(_dev()).eval()
    x = (synth.synth_images(4, 320, 21).float() / 255).to(_dev())
    x2 = (synth.synth_images(4, 320, 22).float() / 255).to(_dev())
    with torch.no_grad():
        want = m(x, augment=True)[0].clone()
        want2 = m(x2, augment=True)[0].clone()
        g = L.GraphedForward(m, x, augment=True)
        z, p = g(x)
        assert p is None
        assert torch.equal(z, want)
        z2, _ = g(x2)
        assert torch.equal(z2, want2)
        assert torch.equal(g(x)[0], want)


# ---- 8. bf16 ---------------------------------------------------------------------------------------------------------------------------
def test_augmented_forward_bf16_vs_fp32_oracle():
    seed = 7100 + 480
    x, zo = _oracle("n", (640, 480), 2, seed)
    m, _ = _model("n", seed)
    m = m.to(_dev()).eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        z, _ = m(x.to(_dev()), augment=True)
    assert z.dtype == torch.float32
    _close(z, zo, "augmented n 640x480 bf16", rel=5 * REL_L2, mx=8 * MAX_REL)


# ---- 9. val.py --augment on SSDD images --------------------------------------------------------------------------------------------------
def test_augmented_val_pipeline_boxes_match_oracle():
    import lead_yolo_amd as L
    imgs, _ = _batch()
    m, st = _model("s", 6262)
    st["model.23.m.0.bias"] = st["model.23.m.0.bias"] + 2.0
    m.load_state_dict(st)
    x = imgs.float() / 255
    with torch.no_grad():
        zo = ref_forward_augment(st, _cfg("s"), x, m.stride)
        z, _ = m.to(_dev()).eval()(x.to(_dev()), augment=True)
    want, _ = ONMS.non_max_suppression(zo.numpy(), 0.001, 0.6)
    got = L.non_max_suppression(z, 0.001, 0.6)
    total = matched = 0
    for i in range(16):
        g, w = got[i].cpu().numpy(), want[i]
        assert abs(len(g) - len(w)) <= max(2, 0.03 * len(w)), (i, len(g), len(w))
        if len(w) == 0:
            continue
        iou = _iou(w, g) if len(g) else np.zeros((len(w), 0))
        for r in range(len(w)):
            ok = (iou[r] > 0.98) & (np.abs(g[:, 4] - w[r, 4]) < 1e-3)
            matched += bool(ok.any())
        total += len(w)
    assert total > 200 and matched >= 0.97 * total, (matched, total)


# ---- 10. errors ------------------------------------------------------------------------------------------------------------------------
def test_augmented_forward_errors():
    m, _ = _model("n", 7400)
    m = m.to(_dev())
    x = torch.rand((1, 3, 64, 64), device=_dev())
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="eval"):
            m.train()(x, augment=True)
        m.eval()
        with pytest.raises(TypeError, match="floating-point"):
            m((x * 255).to(torch.uint8), augment=True)
        with pytest.raises(ValueError, match="multiple"):
            m(torch.rand((1, 3, 64, 72), device=_dev()), augment=True)
