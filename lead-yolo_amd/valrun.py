"""val.py's run on the device: the validation dataloader's arithmetic, the letterboxed batches resident on the device, and the loop.

    vs = ValSet(images, labels, img_size=640, batch_size=32)       # native uint8 HWC BGR images (host or device), labels [n_i, 5] each
    res = validate(model, vs, compute_loss=ComputeLoss(model))
    res.metrics (ValResult), res.maps [nc], res.loss (box, obj, cls), res.confusion [nc + 1, nc + 1], res.speed (pre, inference, nms) ms / image

  val_plan   `create_dataloader(..., rect=True, pad=0.5)` as train.py and val.py call it (utils/dataloaders.py LoadImagesAndLabels): images
             sorted by aspect ratio, every batch on the smallest stride-multiple canvas that holds it, and per image the TWO-stage letterbox of
             the dataloader — `load_image` (long side to img_size, sizes truncated with int()), then letterbox(auto=False, scaleup=False),
             which only pads.  (letterbox_plan in predict.py is detect.py's one-stage round() form: sizes and pads differ by a pixel.)
  val_labels the label rows of `__getitem__`: xywhn2xyxy with the letterbox ratio and pads, xyxy2xywhn(clip=True, eps=1e-3) on the canvas, in
             float32, collated with the batch-local image index
  ValSet     every batch built ONCE at construction by one ly_letterbox_u8 launch and kept on the device with its targets, val_shapes and
             dataset indices: the reference's `--cache ram`, on the device, as ImageBank is for training
  validate   val.py's `run` loop: eval forward per batch (one GraphedForward per canvas), nms_padded, Validator.update(shapes=) with the confusion
             matrix, the validation loss; one synchronisation at the end

Pure host code up to ValSet: val_plan and val_labels need no device."""
import collections

import numpy as np
import torch

from . import capi, predict
from .graph import GraphedForward
from .metrics import Validator
from .nms import nms_padded
from .predict import LetterboxPlan, load_image_size


class ValPlan:
    """val_plan's numbers.  n images in `order` (dataset indices in the order the loader serves them: aspect ratio ascending with rect), nb
    batches: batch_shapes [nb, 2] = (H, W), batch_index [n] (of every position), and per POSITION a LetterboxPlan `lb` (h0, w0 native; nh, nw
    the picture on the canvas; top, left; H, W; r, dw, dh of the padding letterbox; val_shapes rows (h0, w0, h / h0, dw, dh) as val.py
    receives them from the dataloader) plus h, w: the `load_image` size."""

    def __init__(self, order, batch_size, batch_shapes, lb, h, w):
        self.order, self.batch_size, self.batch_shapes, self.lb = order, int(batch_size), batch_shapes, lb
        self.h, self.w = h, w
        self.n, self.nb = len(order), len(batch_shapes)
        self.batch_index = np.arange(self.n) // self.batch_size

    def batches(self):
        """(lo, hi, (H, W)) of every batch: positions lo..hi-1"""
        for i in range(self.nb):
            lo = i * self.batch_size
            yield lo, min(lo + self.batch_size, self.n), (int(self.batch_shapes[i, 0]), int(self.batch_shapes[i, 1]))


def val_plan(shapes_hw, img_size, batch_size, stride=32, pad=0.5, rect=True):
    """The validation dataloader's geometry for images of native sizes shapes_hw = [(h0, w0), ...] -> ValPlan.  Python floats and float64
    numpy as the reference computes them.  rect=False: dataset order, every canvas img_size x img_size."""
    hw0 = np.asarray(shapes_hw, dtype=np.int64).reshape(-1, 2)
    n, img_size, batch_size, stride = len(hw0), int(img_size), int(batch_size), int(stride)
    if n == 0 or batch_size < 1 or (hw0 < 1).any():
        raise ValueError(f"val_plan: {n} images, batch_size {batch_size}; every image needs h0, w0 >= 1")
    bi = np.arange(n) // batch_size
    nb = int(bi[-1]) + 1
    if rect:                                                               # LoadImagesAndLabels.__init__, `if self.rect:`
        ar = hw0[:, 0] / hw0[:, 1]                                         # h / w of the original shapes
        order = ar.argsort(kind="stable")                                  # (the reference's order among equal ratios is unspecified)
        ar = ar[order]
        shapes = [[1, 1]] * nb
        for i in range(nb):
            ari = ar[bi == i]
            mini, maxi = ari.min(), ari.max()
            if maxi < 1:
                shapes[i] = [maxi, 1]
            elif mini > 1:
                shapes[i] = [1, 1 / mini]
        batch_shapes = np.ceil(np.array(shapes) * img_size / stride + pad).astype(int) * stride
    else:
        order = np.arange(n)
        batch_shapes = np.full((nb, 2), img_size, dtype=int)
    f = {k: [] for k in LetterboxPlan._INT + LetterboxPlan._FLT}
    hs, ws, shapes, val_shapes = [], [], [], []
    for pos, i in enumerate(order):
        h0, w0 = int(hw0[i, 0]), int(hw0[i, 1])
        H, W = (int(v) for v in batch_shapes[bi[pos]])
        h, w = load_image_size(h0, w0, img_size)
        if h < 1 or w < 1:
            raise ValueError(f"val_plan: image {i} ({h0} x {w0}) would be loaded as {h} x {w}")
        r = min(min(H / h, W / w), 1.0)                                    # letterbox(im, (H, W), auto=False, scaleup=False)
        nw, nh = int(round(w * r)), int(round(h * r))
        if nh < 1 or nw < 1:
            raise ValueError(f"val_plan: image {i} ({h0} x {w0}) would be resized to {nh} x {nw} on a {H} x {W} canvas")
        dw, dh = (W - nw) / 2, (H - nh) / 2
        top, left = int(round(dh - 0.1)), int(round(dw - 0.1))
        for k, v in zip(LetterboxPlan._INT + LetterboxPlan._FLT, (h0, w0, nh, nw, top, left, H, W, r, dw, dh)):
            f[k].append(v)
        hs.append(h)
        ws.append(w)
        gain = min(H / h0, W / w0)                                         # detect.py's table, for completeness (scale_boxes without ratio_pad)
        shapes.append((h0, w0, gain, (W - w0 * gain) / 2, (H - h0 * gain) / 2))
        val_shapes.append((h0, w0, h / h0, dw, dh))                        # shapes = (h0, w0), ((h / h0, w / w0), pad)
    lb = LetterboxPlan(f, np.array(shapes, dtype=np.float32).reshape(-1, 5), np.array(val_shapes, dtype=np.float32).reshape(-1, 5))
    return ValPlan(order, batch_size, batch_shapes, lb, np.array(hs, dtype=np.int64), np.array(ws, dtype=np.int64))


def val_labels(labels, plan):
    """`__getitem__`'s label rows and `collate_fn` for every batch of the plan: labels[i] = [n_i, 5] (class, normalised xywh of the native
    image) per DATASET index -> list of float32 [nt_b, 6] arrays (batch-local image, class, normalised xywh of the canvas).  float32
    throughout and in the reference's order: xywhn2xyxy(lab, ratio_w * w, ratio_h * h, padw, padh), then xyxy2xywhn(w=W, h=H, clip=True,
    eps=1e-3)."""
    if len(labels) != plan.n:
        raise ValueError(f"val_labels: {len(labels)} label arrays for {plan.n} images")
    f32 = np.float32
    out = []
    for lo, hi, (H, W) in plan.batches():
        rows = []
        for pos in range(lo, hi):
            lab = np.asarray(labels[plan.order[pos]], dtype=f32).reshape(-1, 5)
            x = lab[:, 1:5]
            r = float(plan.lb.r[pos])
            sw, sh, pw, ph = f32(r * int(plan.w[pos])), f32(r * int(plan.h[pos])), f32(plan.lb.dw[pos]), f32(plan.lb.dh[pos])
            x1, y1 = sw * (x[:, 0] - x[:, 2] / 2) + pw, sh * (x[:, 1] - x[:, 3] / 2) + ph       # xywhn2xyxy (utils/general.py)
            x2, y2 = sw * (x[:, 0] + x[:, 2] / 2) + pw, sh * (x[:, 1] + x[:, 3] / 2) + ph
            cw, ch = f32(W - 1e-3), f32(H - 1e-3)                                                 # clip_boxes(x, (h - eps, w - eps))
            x1, x2, y1, y2 = np.clip(x1, 0, cw), np.clip(x2, 0, cw), np.clip(y1, 0, ch), np.clip(y2, 0, ch)
            Wf, Hf = f32(W), f32(H)
            row = np.stack([np.full(len(lab), pos - lo, f32), lab[:, 0], ((x1 + x2) / 2) / Wf, ((y1 + y2) / 2) / Hf, (x2 - x1) / Wf,
                            (y2 - y1) / Hf], 1).astype(f32)
            rows.append(row.reshape(-1, 6))
        out.append(np.concatenate(rows) if rows else np.zeros((0, 6), f32))
    return out


class ValSet:
    """A validation set as val.py's dataloader serves it, resident on the device.

    images: native uint8 HWC BGR (cv2.imread's form) of any sizes, numpy arrays / CPU tensors or contiguous device tensors; labels: one
    [n_i, 5] array per image (class, normalised xywh).  Every batch of val_plan is built once, here, by one ly_letterbox_u8 launch:
    batch b is `x[b]` uint8 [batch_size, 3, H_b, W_b] (RGB planes; the free slots of the last batch are all-114 canvases), with `targets[b]`
    [nt_b, 6], `val_shapes[b]` [k_b, 5] (what Validator.update(shapes=) takes), `count[b]` = k_b images and `index[b]`, their dataset indices.
    Memory: the batches stay on the device, n * 3 * H * W bytes — validate(graphed=True) adds one batch and the graph's pools per canvas — (5000 images on 384 x 672 canvases: 3.9 GB; the native images are only
    staged batch by batch).
    The picture is resized from the NATIVE image straight to its size on the canvas with INTER_LINEAR (ly_letterbox_u8's contract).  The
    reference's `load_image` takes INTER_AREA when a non-augmenting loader shrinks an image: shrunk sources differ from the reference's
    pixels as every other resize of this package does; sizes, pads and labels are the reference's exactly."""

    def __init__(self, images, labels, img_size=640, batch_size=32, stride=32, pad=0.5, rect=True, device=None):
        if len(images) == 0 or len(images) != len(labels):
            raise ValueError(f"ValSet: {len(images)} images and {len(labels)} label arrays (need the same, non-zero count)")
        if int(stride) % 16:
            raise ValueError(f"ValSet: stride {stride} must be a multiple of 16 (the uint8 NCHW rows are written 16 bytes at a time)")
        dev = next((im.device for im in images if isinstance(im, torch.Tensor) and im.is_cuda), None)
        self.device = predict._device(dev if dev is not None else device)
        self.img_size, self.batch_size, self.stride, self.rect = int(img_size), int(batch_size), int(stride), bool(rect)
        self.plan = plan = val_plan([tuple(im.shape[:2]) for im in images], img_size, batch_size, stride, pad, rect)
        self.n = plan.n
        self.x, self.targets, self.val_shapes, self.count, self.index, self.canvas = [], [], [], [], [], []
        lb = plan.lb
        for (lo, hi, (H, W)), rows in zip(plan.batches(), val_labels(labels, plan)):
            k = hi - lo
            src, keep = predict._sources([images[i] for i in plan.order[lo:hi]], self.device, "ValSet")
            x = torch.empty((self.batch_size, 3, H, W), dtype=torch.uint8, device=self.device)
            table = (capi.LyLetterboxImage * self.batch_size)()
            for j in range(self.batch_size):
                dst = x.data_ptr() + j * 3 * H * W
                if j < k:
                    p, h0, w0 = src[j]
                    table[j] = capi.LyLetterboxImage(p, dst, h0, w0, H, W, int(lb.nh[lo + j]), int(lb.nw[lo + j]), int(lb.top[lo + j]),
                                                     int(lb.left[lo + j]))
                else:
                    table[j] = capi.LyLetterboxImage(None, dst, 0, 0, H, W, 0, 0, 0, 0)          # a slot without a picture: all 114
            table_dev, tabs = predict._upload(table, lb.val_shapes[lo:hi], self.device)
            predict._launch(table_dev, self.batch_size, H, W, predict.LB_CHW_RGB)
            del keep
            self.x.append(x)
            self.val_shapes.append(tabs.clone())                          # `tabs` lives in the table's upload block
            self.targets.append(torch.from_numpy(rows).to(self.device))
            self.count.append(k)
            self.index.append(plan.order[lo:hi].copy())
            self.canvas.append((H, W))
        self._graphs = {}                                                  # canvas -> GraphedForward (validate)

    def __len__(self):
        return len(self.x)

    def nbytes(self):
        return sum(x.numel() for x in self.x)


ValRun = collections.namedtuple("ValRun", "metrics maps loss confusion speed stats")


def _key(x):
    return tuple(x.shape), x.dtype


def _graph_for(vs, model, x, max_graphs):
    """the GraphedForward of x's canvas: built on first use, rebuilt when it belongs to another model or its weights moved; None beyond
    max_graphs canvases (the caller then runs eagerly).  Building one warms up, synchronises the device and captures."""
    key = _key(x)
    g = vs._graphs.get(key)
    if g is not None and (g.model is not model or g.stale()):
        del vs._graphs[key]                                                # its pools go before the new capture
        g = None
    if g is None and len(vs._graphs) < max_graphs:
        g = vs._graphs[key] = GraphedForward(model, x)
    return g


def validate(model, valset, compute_loss=None, conf_thres=0.001, iou_thres=0.6, max_det=300, single_cls=False, confusion=True, graphed=True,
             max_graphs=8):
    """val.py's `run` over a ValSet -> ValRun(metrics: ValResult; maps [nc]: val.py's `maps` (mAP@.5:.95 per class, the mean where a class
    has no labels); loss: (box, obj, cls) float32 numpy, the mean over batches as val.py logs it, or None; confusion: [nc + 1, nc + 1] int64
    or None; speed: (pre, inference, nms) ms per image from HIP events; stats: Validator.stats() — correct [n, 10], conf, cls over all images
    in the order they were served, labels per class).

    Per batch: the eval forward on the resident batch (uint8 straight in when model.u8_input, else batch.to(dtype) / 255), nms_padded with
    multi_label = (the model's nc) > 1 — and, as val.py, agnostic = single_cls —, Validator.update(shapes=val_shapes) — scoring in native space —
    with the confusion matrix behind it, and with `compute_loss` the loss items of the raw maps.  The loop over the batches does not
    synchronise with the host; the one synchronisation is at the end.
    graphed=True holds one GraphedForward per distinct (canvas, dtype) on the ValSet, reused by later calls while the model's weights have
    not moved (GraphedForward.stale); beyond max_graphs canvases the forward runs eagerly.  The graphs a pass needs and does not find — all of
    them on a first pass or after the weights moved — are captured BEFORE the loop (warm-up forwards, a device synchronise and the capture,
    per canvas), outside the intervals `speed` times.  Each graph owns a copy of its input batch and its pools on top of the ValSet's
    resident bytes, and a replay starts with a device copy of the resident batch into that input (counted in `speed`'s inference).  The free slots of the last
    batch are all-114 canvases whose rows are dropped before scoring; for the LOSS a partial batch is run again at its true size, because the
    obj loss averages over every cell of the batch.  The model is run in eval mode and handed back in the mode it came in, weights untouched
    (pass an EMA model as it is).  The mixed-precision policy is the caller's: call under the autocast context the model should run in."""
    vs = valset
    det = model.model[-1]
    nc = 1 if single_cls else int(det.nc)
    p = next(model.parameters())
    u8 = bool(getattr(model, "u8_input", False))
    v = Validator(nc, conf_thres, iou_thres, max_det, capacity_images=vs.n, single_cls=single_cls, device=vs.device, confusion=confusion)
    was_training = model.training
    model.eval()
    loss = torch.zeros(3, device=vs.device) if compute_loss is not None else None
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(len(vs))]

    def feed(b):
        return vs.x[b] if u8 else vs.x[b].to(p.dtype) / 255                                  # val.py:212-214

    try:
        with torch.no_grad():
            graphs = {}
            if graphed:
                for b in range(len(vs)):                                                     # one canvas's batches share a graph
                    key = (tuple(vs.x[b].shape), torch.uint8 if u8 else p.dtype)
                    if key not in graphs:
                        graphs[key] = _graph_for(vs, model, feed(b), max_graphs)
            for b in range(len(vs)):
                k, (H, W), targets = vs.count[b], vs.canvas[b], vs.targets[b]
                if single_cls and len(targets):
                    targets = targets.clone()
                    targets[:, 1] = 0
                ev[b][0].record()
                x = feed(b)
                ev[b][1].record()
                g = graphs.get(_key(x))
                z, train_out = g(x) if g is not None else model(x)
                ev[b][2].record()
                dets, counts, _ = nms_padded(z, conf_thres, iou_thres, agnostic=single_cls, max_det=max_det, multi_label=int(det.nc) > 1)   # val.py:230-234
                ev[b][3].record()
                v.update((dets[:k], counts[:k]), targets, shapes=vs.val_shapes[b], size=(W, H))
                if compute_loss is not None:
                    if k < vs.batch_size:
                        train_out = model(x[:k])[1]
                    loss += compute_loss(train_out, targets)[1]                          # `loss += compute_loss(train_out, targets)[1]`
        stats = v.stats()                                                                # the one synchronisation
        res = v.compute(stats)
    finally:
        model.train(was_training)
    maps = np.zeros(nc) + res.map                                                        # `maps = np.zeros(nc) + map; maps[c] = ap[i]`
    for i, c in enumerate(res.classes[:len(res.ap)]):
        maps[c] = res.ap[i]
    speed = tuple(sum(e[i].elapsed_time(e[i + 1]) for e in ev) / vs.n for i in range(3))
    return ValRun(res, maps, (loss / len(vs)).cpu().numpy() if loss is not None else None, v.confusion.matrix() if confusion else None, speed,
                  stats)
