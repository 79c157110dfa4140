"""The detect pipeline around the forward, on the device: images in -> boxes on those images out.

What the reference's detect.py does per image on the CPU — `LoadImages.__next__` (utils/dataloaders.py): `letterbox()` (utils/augmentations.py:
cv2.resize INTER_LINEAR + cv2.copyMakeBorder(114)) + `transpose((2, 0, 1))[::-1]`, and after NMS `scale_boxes(...).round()`
(utils/general.py) — as one launch per batch each (csrc/ly_letterbox.hip: ly_letterbox_u8, ly_scale_boxes).

    det = Detector(model.eval(), img_size=640, batch_size=32)
    boxes = det(images)                                   # images: uint8 HWC BGR arrays / tensors of any sizes, host or device
    for b in boxes: ...                                   # [n_i, 6] = xyxy in the pixels of image i, conf, cls

    batch, plan = letterbox(images, 640, out=g.x)         # straight into a GraphedForward's input buffer; no host sync
    v.update(model(batch), targets, shapes=plan.val_shapes)     # Validator scoring in native space

`letterbox_plan` is the host arithmetic alone (no device): the reference's formulas in Python floats, and the two (h0, w0, gain, padw, padh)
tables that take boxes back — detect.py's (scale_boxes without ratio_pad) and val.py's (with ratio_pad; the one Validator.update takes)."""
import ctypes

import numpy as np
import torch

from . import capi
from .graph import GraphedForward
from .nms import nms_padded

FILL = 114                                  # letterbox's border colour
LB_CHW_RGB, LB_HWC_BGR = 0, 1               # `layout` codes of ly_letterbox_u8 (LY_LB_* in the header)


class LetterboxPlan:
    """letterbox's numbers for n images, one entry per image: h0, w0 (source), nh, nw (resized picture: new_unpad), top, left (its corner),
    H, W (canvas) as int arrays; r, dw, dh (ratio and float half-pads) as float64;
    shapes [n, 5] float32     (h0, w0, gain, padw, padh) as detect.py's scale_boxes(im.shape[2:], boxes, im0.shape) computes gain and pad;
    val_shapes [n, 5] float32 the same form from val.py's ratio_pad ((nh / h0, nw / w0), (dw, dh)): what Validator.update(shapes=) takes.
    shapes_dev / val_shapes_dev: the tables on the device when the plan comes from letterbox() (None from letterbox_plan)."""
    _INT = ("h0", "w0", "nh", "nw", "top", "left", "H", "W")
    _FLT = ("r", "dw", "dh")

    def __init__(self, fields, shapes, val_shapes, shapes_dev=None, val_shapes_dev=None):
        for k in self._INT:
            setattr(self, k, np.asarray(fields[k], dtype=np.int64))
        for k in self._FLT:
            setattr(self, k, np.asarray(fields[k], dtype=np.float64))
        self.shapes, self.val_shapes = shapes, val_shapes
        self.shapes_dev, self.val_shapes_dev = shapes_dev, val_shapes_dev
        self.n = len(self.h0)

    @property
    def canvas(self):
        """(H, W) of the batch; raises when the images do not share one canvas"""
        if len(set(zip(self.H.tolist(), self.W.tolist()))) != 1:
            raise ValueError("LetterboxPlan.canvas: the images have different canvases")
        return int(self.H[0]), int(self.W[0])

    @classmethod
    def concat(cls, plans):
        fields = {k: np.concatenate([getattr(p, k) for p in plans]) for k in cls._INT + cls._FLT}
        on_dev = all(p.shapes_dev is not None for p in plans)
        return cls(fields, np.concatenate([p.shapes for p in plans]), np.concatenate([p.val_shapes for p in plans]),
                   torch.cat([p.shapes_dev for p in plans]) if on_dev else None, torch.cat([p.val_shapes_dev for p in plans]) if on_dev else None)


def letterbox_plan(shapes_hw, new_shape=640, auto=False, scaleup=True, stride=32):
    """utils/augmentations.py letterbox (scaleFill=False) for images of sizes shapes_hw = [(h0, w0), ...], in Python floats as the reference
    computes them -> LetterboxPlan.  new_shape: s or (h, w).  auto=True pads to the next multiple of `stride` only (the minimum rectangle),
    so the canvas depends on the image: every image of the batch must then give the same one."""
    ns = (int(new_shape), int(new_shape)) if isinstance(new_shape, (int, np.integer)) else tuple(int(v) for v in new_shape)
    f = {k: [] for k in LetterboxPlan._INT + LetterboxPlan._FLT}
    shapes, val_shapes = [], []
    if len(shapes_hw) == 0:
        raise ValueError("letterbox_plan: no images")
    for i, (h0, w0) in enumerate(shapes_hw):
        h0, w0 = int(h0), int(w0)
        if h0 < 1 or w0 < 1:
            raise ValueError(f"letterbox_plan: image {i} is {h0} x {w0}")
        r = min(ns[0] / h0, ns[1] / w0)
        if not scaleup:
            r = min(r, 1.0)
        nw, nh = int(round(w0 * r)), int(round(h0 * r))                    # new_unpad
        if nh < 1 or nw < 1:
            raise ValueError(f"letterbox_plan: image {i} ({h0} x {w0}) would be resized to {nh} x {nw} on a {ns[0]} x {ns[1]} canvas")
        dw, dh = ns[1] - nw, ns[0] - nh
        if auto:
            dw, dh = dw % stride, dh % stride                               # np.mod
        dw, dh = dw / 2, dh / 2
        top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
        left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
        H, W = nh + top + bottom, nw + left + right
        for k, v in zip(LetterboxPlan._INT + LetterboxPlan._FLT, (h0, w0, nh, nw, top, left, H, W, r, dw, dh)):
            f[k].append(v)
        gain = min(H / h0, W / w0)                                          # scale_boxes, ratio_pad=None
        shapes.append((h0, w0, gain, (W - w0 * gain) / 2, (H - h0 * gain) / 2))
        val_shapes.append((h0, w0, nh / h0, dw, dh))                        # val.py: shapes = (h0, w0), ((h / h0, w / w0), pad)
        if auto and (H, W) != (f["H"][0], f["W"][0]):
            raise ValueError(f"letterbox_plan(auto=True): image {i} ({h0} x {w0}) gives a {H} x {W} canvas, image 0 "
                             f"({f['h0'][0]} x {f['w0'][0]}) a {f['H'][0]} x {f['W'][0]} one: a batch has one shape")
    return LetterboxPlan(f, np.array(shapes, dtype=np.float32).reshape(-1, 5), np.array(val_shapes, dtype=np.float32).reshape(-1, 5))


def load_image_size(h0, w0, img_size):
    """utils/dataloaders.py load_image: the long side to img_size, r = img_size / max(h0, w0), both sides TRUNCATED with int() -> (h, w).  The
    training bank (ImageBank.from_native) and the validation loader (valrun.val_plan) load their images at this size."""
    r = int(img_size) / max(int(h0), int(w0))
    return int(h0 * r), int(w0 * r)


# ---- device plumbing ----------------------------------------------------------------------------------------------------------------------
def _device(device):
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise RuntimeError(f"the HIP path needs a CUDA/ROCm device (got {dev}); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _sources(images, dev, who):
    """uint8 HWC BGR images -> ([(device address, h0, w0)], what must stay referenced until the launch).  Device tensors are addressed where
    they are; host images (numpy arrays, CPU tensors) are packed into ONE pinned block and go up with one non-blocking copy."""
    if len(images) == 0:
        raise ValueError(f"{who}: no images")
    host, at, total = [], [], 0
    for i, im in enumerate(images):
        shape, dtype = tuple(im.shape), im.dtype
        if dtype not in (np.uint8, torch.uint8) or len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"{who}: image {i} must be uint8 HWC with 3 channels (got {dtype} {shape})")
        if isinstance(im, torch.Tensor) and im.is_cuda:
            if im.device != dev or not im.is_contiguous():
                raise ValueError(f"{who}: image {i} must be a contiguous tensor on {dev} (got strides {im.stride()} on {im.device})")
            at.append(im.data_ptr())
        else:
            host.append((i, im.numpy() if isinstance(im, torch.Tensor) else np.asarray(im), total))
            at.append(None)
            total += shape[0] * shape[1] * 3
    keep = [images]
    if host:
        pinned = torch.empty(total, dtype=torch.uint8, pin_memory=True)    # a fresh pinned block: the host allocator keeps it until the copy ran
        hv = pinned.numpy()
        for i, a, off in host:
            hv[off:off + a.size].reshape(a.shape)[...] = a
        staged = torch.empty(total, dtype=torch.uint8, device=dev)
        staged.copy_(pinned, non_blocking=True)
        for i, a, off in host:
            at[i] = staged.data_ptr() + off
        keep.append(staged)
    return [(p, int(im.shape[0]), int(im.shape[1])) for p, im in zip(at, images)], keep


def _upload(table, floats, dev):
    """a ctypes table (+ a float32 array behind it) on the device: one non-blocking copy from a fresh pinned block on the current stream, as
    MosaicAugment.upload -> (uint8 tensor holding the table, float32 view of the array)"""
    tb = ctypes.sizeof(table)
    nbytes = tb + floats.size * 4
    table_dev = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    ctypes.memmove(hv.ctypes.data, table, tb)
    hv[tb:].view(np.float32)[:] = floats.reshape(-1)
    table_dev.copy_(host, non_blocking=True)
    return table_dev, table_dev[tb:].view(torch.float32).view(floats.shape)


def _launch(table_dev, n, maxH, maxW, layout):
    capi.check(capi.lib().ly_letterbox_u8(capi.ptr(table_dev), n, int(maxH), int(maxW), layout, capi.stream_ptr()), "ly_letterbox_u8")


def letterbox(images, new_shape=640, auto=False, scaleup=True, stride=32, out=None, device=None):
    """LoadImages.__next__ for a batch on the device: -> (uint8 [n, 3, H, W] RGB planes, LetterboxPlan), one ly_letterbox_u8 launch on the
    current stream, no host synchronisation.  images: uint8 HWC BGR (cv2.imread's form), any sizes — numpy arrays / CPU tensors (one pinned
    staging block, one copy) or contiguous device tensors (a decoder's output: read where they are).  out: write into this contiguous uint8
    [n, 3, H, W] tensor (a GraphedForward's `.x`, or a slice of it).  W must be a multiple of 16 (any canvas the model takes is)."""
    dev = out.device if out is not None else next((im.device for im in images if isinstance(im, torch.Tensor) and im.is_cuda), None)
    dev = _device(dev if dev is not None else device)
    src, keep = _sources(images, dev, "letterbox")
    plan = letterbox_plan([(h, w) for _, h, w in src], new_shape, auto, scaleup, stride)
    n, (H, W) = plan.n, plan.canvas
    if W % 16:
        raise ValueError(f"letterbox: the canvas is {H} x {W}; the uint8 NCHW layout needs W a multiple of 16")
    if out is None:
        out = torch.empty((n, 3, H, W), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n, 3, H, W) or not out.is_contiguous() or not out.is_cuda or out.data_ptr() % 16:
        raise ValueError(f"letterbox: out must be a contiguous, 16-byte aligned uint8 [{n}, 3, {H}, {W}] device tensor (got {out.dtype} "
                         f"{tuple(out.shape)} on {out.device})")
    table = (capi.LyLetterboxImage * n)()
    for i, (p, h0, w0) in enumerate(src):
        table[i] = capi.LyLetterboxImage(p, out.data_ptr() + i * 3 * H * W, h0, w0, H, W, int(plan.nh[i]), int(plan.nw[i]), int(plan.top[i]),
                                         int(plan.left[i]))
    table_dev, tabs = _upload(table, np.stack([plan.shapes, plan.val_shapes]), dev)
    _launch(table_dev, n, H, W, LB_CHW_RGB)
    plan.shapes_dev, plan.val_shapes_dev = tabs[0], tabs[1]
    del keep
    return out, plan


def scale_boxes(dets, counts, shapes, round_boxes=False, out=None):
    """utils/general.py scale_boxes + clip_boxes (and detect.py's .round()) on what nms_padded returns: dets [bs, max_det, 6] float32, counts
    [bs] int32, shapes [bs, 5] float32 = (h0, w0, gain, padw, padh) on the device -> boxes in the original images' pixels, rows past the
    count zero.  out may be dets itself.  One launch, no host synchronisation."""
    if not (dets.is_cuda and dets.dtype == torch.float32 and dets.is_contiguous() and dets.dim() == 3 and dets.shape[2] == 6):
        raise ValueError(f"scale_boxes: dets must be a contiguous float32 [bs, max_det, 6] device tensor (got {dets.dtype} {tuple(dets.shape)})")
    bs, max_det = dets.shape[0], dets.shape[1]
    counts = counts.to(torch.int32).contiguous()
    shapes = torch.as_tensor(shapes, dtype=torch.float32, device=dets.device).contiguous()
    if counts.shape != (bs,) or shapes.shape != (bs, 5):
        raise ValueError(f"scale_boxes: counts [bs] and shapes [bs, 5] expected (got {tuple(counts.shape)}, {tuple(shapes.shape)})")
    if out is None:
        out = torch.empty_like(dets)
    elif out.dtype != torch.float32 or out.shape != dets.shape or not out.is_contiguous() or out.device != dets.device:
        raise ValueError("scale_boxes: out must be a contiguous float32 tensor of dets' shape on its device")
    capi.check(capi.lib().ly_scale_boxes(capi.ptr(dets), capi.ptr(counts), bs, max_det, capi.ptr(shapes), int(bool(round_boxes)), capi.ptr(out),
                                         capi.stream_ptr()), "ly_scale_boxes")
    return out


class Detector:
    """detect.py's loop as one object: letterbox -> forward -> NMS -> boxes in the original images, everything on the device.

    det(images)          -> list of [n_i, 6] tensors (xyxy in the NATIVE image — rounded to whole pixels with round_boxes, as detect.py —,
                            conf, cls), one per image; one synchronisation at the end (the list needs the counts on the host)
    det.padded(images)   -> (dets [n, max_det, 6], counts [n], LetterboxPlan), no synchronisation.  native=False leaves the boxes on the
                            letterboxed canvas (what Validator.update takes together with shapes=plan.val_shapes)

    Any number of images: they run in chunks of batch_size on one fixed [batch_size, 3, img_size, img_size] batch; the free slots of the last
    chunk are all-114 canvases whose rows are dropped.  The batch goes to the model as uint8 when model.u8_input (augment=True takes a float
    batch), else as batch.to(dtype) / 255.  graphed=True holds one GraphedForward on that batch and letterboxes straight into its input
    buffer; like every GraphedForward it does not follow weight changes: stale() tells (it is not polled per call), refresh() captures
    anew.  auto=True (the minimum rectangle) has a data-dependent canvas: the images of a chunk must share it and the forward runs eagerly.
    The mixed-precision policy is the caller's: construct and call under the autocast context the model should run in."""

    def __init__(self, model, img_size=640, batch_size=32, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, max_det=1000,
                 multi_label=False, augment=False, auto=False, graphed=True, round_boxes=True):
        if model.training:
            raise RuntimeError("Detector runs the inference forward: call model.eval() first")
        self.model = model
        self.stride = int(model.stride.max())
        self.img_size, self.batch_size = int(img_size), int(batch_size)
        if self.img_size < self.stride or self.img_size % self.stride or self.batch_size < 1:
            raise ValueError(f"Detector: img_size {img_size} must be a multiple of the model's stride {self.stride}, batch_size {batch_size} >= 1")
        self.nms = dict(conf_thres=conf_thres, iou_thres=iou_thres, classes=classes, agnostic=agnostic, max_det=int(max_det),
                        multi_label=multi_label)
        self.max_det = int(max_det)
        self.augment, self.auto, self.round_boxes = bool(augment), bool(auto), bool(round_boxes)
        self.graphed = bool(graphed) and not self.auto
        p = next(model.parameters())
        self.device, self.dtype = p.device, p.dtype
        self.u8 = bool(getattr(model, "u8_input", False)) and not self.augment
        shape = (self.batch_size, 3, self.img_size, self.img_size)
        self._u8 = self._x = self._g = None
        if not self.auto:
            self._x = torch.zeros(shape, dtype=torch.uint8 if self.u8 else self.dtype, device=self.device)
            if self.graphed:
                self.refresh()
            self._u8 = self._x if self.u8 else torch.empty(shape, dtype=torch.uint8, device=self.device)

    def stale(self):
        """GraphedForward.stale() of the captured forward (False for the eager forms, which follow the weights by themselves)"""
        return self._g is not None and self._g.stale()

    def refresh(self):
        """capture the forward anew with the weights the model holds now"""
        if self.graphed:
            self._g = None                                  # the old graph's pools go first
            self._g = GraphedForward(self.model, self._x, augment=self.augment)
            self._x = self._g.x
            if self.u8:
                self._u8 = self._x
        return self

    def _forward(self, x):
        if self._g is not None:
            return self._g()[0]
        with torch.no_grad():
            return (self.model(x, augment=True) if self.augment else self.model(x))[0]

    def _chunk(self, images, native):
        k = len(images)
        if self.auto:
            batch, plan = letterbox(images, self.img_size, auto=True, stride=self.stride, device=self.device)
            x = batch if self.u8 else batch.to(self.dtype) / 255
        else:
            _, plan = letterbox(images, self.img_size, stride=self.stride, out=self._u8[:k])
            if k < self.batch_size:
                self._u8[k:].fill_(FILL)
            if not self.u8:
                self._x.copy_(self._u8.to(self.dtype) / 255)
            x = self._x
        dets, counts, _ = nms_padded(self._forward(x), **self.nms)
        dets, counts = dets[:k].contiguous(), counts[:k].contiguous()
        if native:
            scale_boxes(dets, counts, plan.shapes_dev, self.round_boxes, out=dets)
        return dets, counts, plan

    def padded(self, images, native=True):
        images = list(images)
        if not images:
            raise ValueError("Detector: no images")
        bs = self.batch_size
        parts = [self._chunk(images[i:i + bs], native) for i in range(0, len(images), bs)]
        if len(parts) == 1:
            return parts[0]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), LetterboxPlan.concat([p[2] for p in parts])

    def __call__(self, images):
        dets, counts, _ = self.padded(images)
        return [dets[i, :c] for i, c in enumerate(counts.tolist())]         # the one synchronisation
