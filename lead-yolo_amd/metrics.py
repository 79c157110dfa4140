"""Validation metrics: the scoring loop of the reference's val.py (val.py:127-188) with the per-image part on the device.

  match_padded   csrc/ly_metrics.hip `ly_val_match`: labels of every image prepared as val.py:217 / :157-162 do, `process_batch`
                 (val.py:79-101) for the whole batch in one launch on what `nms_padded` returns; no host synchronisation
  Validator      update() per batch (nms_padded -> ly_val_match -> ly_val_advance: sync-free, capturable), compute() once per validation
  ConfusionMatrix  utils/metrics.py `class ConfusionMatrix`: `ly_val_confusion`, its process_batch for a whole batch in one launch, added to
                 a device matrix; Validator(confusion=True) feeds one with what it scores
  ap_per_class   utils/metrics.py:31-95, compute_ap utils/metrics.py:98-123, as float64 numpy

ap_per_class / compute_ap stay on the host on purpose: they run once per validation, after ONE device-to-host copy of the accumulator
(a 16-bit mask, a confidence and a class per detection — about 2.4 KB per image at max_det = 300 — plus the label histogram), and are a sort
and a few cumulative sums over those rows; the reference does the same in numpy.  What costs time in the reference is the per-image loop in
front of them, and that is the part the kernel replaces.

Out of scope: plots (the confusion matrix is returned as numbers), the COCO json and `save_hybrid` labels of val.py."""
import collections

import numpy as np
import torch

from . import capi
from .nms import nms_padded

NIOU = 10                                  # val.py:171 `iouv = torch.linspace(0.5, 0.95, 10)`
MAX_LABELS = capi._DEFINES["LY_VAL_MAX_LABELS"]
OVF_LABELS, OVF_CLASS = 1, 2               # bits of the overflow flag (csrc/ly_metrics.hip)

_p = capi.ptr


# ---------------------------------------------------------------------------------------------------------------- host part (numpy, float64)
def compute_ap(recall, precision):
    """utils/metrics.py:98-123 (method 'interp'): 101-point interpolated area under the precision envelope -> (ap, mpre, mrec)"""
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)
    y = np.interp(x, mrec, mpre)
    return float((np.diff(x) * (y[1:] + y[:-1]) / 2.0).sum()), mpre, mrec           # np.trapz(y, x)


def _smooth(y, f=0.05):
    """utils/metrics.py:23-28: box filter of fraction f"""
    nf = round(len(y) * f * 2) // 2 + 1
    p = np.ones(nf // 2)
    yp = np.concatenate((p * y[0], y, p * y[-1]), 0)
    return np.convolve(yp, np.ones(nf) / nf, mode="valid")


def ap_per_class(tp, conf, pred_cls, target_cls=None, nt_per_class=None, eps=1e-16):
    """utils/metrics.py:31-95 without the plots -> (tp, fp, p, r, f1, ap [classes, 10], classes): precision / recall at the maximum of the
    smoothed mean F1 curve, AP per IoU level, for every class that has labels.  The labels come either as `target_cls` (one entry per
    label, the reference's form) or as `nt_per_class` (labels per class id — all ap_per_class takes from target_cls is np.unique's
    classes and counts).  Runs on the host in float64 numpy, as the reference does (see the module docstring)."""
    if (target_cls is None) == (nt_per_class is None):
        raise ValueError("ap_per_class: give either target_cls or nt_per_class")
    tp, conf, pred_cls = np.asarray(tp), np.asarray(conf), np.asarray(pred_cls)
    i = np.argsort(-conf)
    tp, conf, pred_cls = tp[i], conf[i], pred_cls[i]
    if nt_per_class is None:
        unique_classes, nt = np.unique(target_cls, return_counts=True)
    else:
        nt_per_class = np.asarray(nt_per_class)
        unique_classes = np.nonzero(nt_per_class > 0)[0]
        nt = nt_per_class[unique_classes]
    nc = unique_classes.shape[0]
    px = np.linspace(0, 1, 1000)
    ap, p, r = np.zeros((nc, tp.shape[1])), np.zeros((nc, 1000)), np.zeros((nc, 1000))
    for ci, c in enumerate(unique_classes):
        i = pred_cls == c
        n_l, n_p = nt[ci], i.sum()
        if n_p == 0 or n_l == 0:
            continue
        fpc = (1 - tp[i]).cumsum(0)
        tpc = tp[i].cumsum(0)
        recall = tpc / (n_l + eps)
        r[ci] = np.interp(-px, -conf[i], recall[:, 0], left=0)
        precision = tpc / (tpc + fpc)
        p[ci] = np.interp(-px, -conf[i], precision[:, 0], left=1)
        for j in range(tp.shape[1]):
            ap[ci, j], _, _ = compute_ap(recall[:, j], precision[:, j])
    f1 = 2 * p * r / (p + r + eps)
    i = _smooth(f1.mean(0), 0.1).argmax()
    p, r, f1 = p[:, i], r[:, i], f1[:, i]
    tp = (r * nt).round()
    fp = (tp / (p + eps) - tp).round()
    return tp, fp, p, r, f1, ap, unique_classes.astype(int)


# ---------------------------------------------------------------------------------------------------------------- device part
class MatchAccumulator:
    """The accumulator ly_val_match writes: ONE int32 device buffer (one copy brings all of it to the host) with typed views.
    Per slot (= image) a row of `row_width` detections: correct (16-bit mask, bit i = IoU level i), conf, cls, match_label, match_iou;
    per slot n_det, nt_class [nc], overflow; and the cursor (the next free slot) in front."""
    _ROWS = (("conf", torch.float32), ("cls", torch.float32), ("match_label", torch.int32), ("match_iou", torch.float32))

    def __init__(self, capacity, row_width, nc, device):
        if capacity < 1 or row_width < 1 or not 1 <= nc <= 4096:
            raise ValueError(f"MatchAccumulator: capacity={capacity} row_width={row_width} nc={nc}")
        self.capacity, self.row_width, self.nc = int(capacity), int(row_width), int(nc)
        cells = self.capacity * self.row_width
        sizes = [("cursor", 4), ("n_det", self.capacity), ("overflow", self.capacity), ("nt_class", self.capacity * self.nc)]
        sizes += [(k, cells) for k, _ in self._ROWS] + [("correct", (cells + 1) // 2)]
        self._off, off = {}, 0
        for k, n in sizes:
            self._off[k] = (off, n)
            off += (n + 3) // 4 * 4                               # every section starts on 16 bytes
        self.buf = torch.zeros(off, dtype=torch.int32, device=device)
        self._bind(self, self.buf)

    def _bind(self, obj, buf):
        sec = {k: buf[o:o + n] for k, (o, n) in self._off.items()}
        c, w = self.capacity, self.row_width
        obj.cursor, obj.n_det, obj.overflow = sec["cursor"], sec["n_det"], sec["overflow"]
        obj.nt_class = sec["nt_class"].view(c, self.nc)
        for k, dt in self._ROWS:
            setattr(obj, k, sec[k].view(dt).view(c, w))
        obj.correct = sec["correct"].view(torch.int16)[:c * w].view(c, w)          # the kernel's uint16 (bits 0-9 only)

    def zero_(self):
        self.buf.zero_()
        return self

    def host(self):
        """one synchronisation, one copy -> a namespace of numpy views (correct as uint16)"""
        h = self.buf.cpu()
        out = collections.namedtuple("HostAccumulator", "cursor n_det overflow nt_class conf cls match_label match_iou correct")
        ns = type("ns", (), {})()
        self._bind(ns, h)
        return out(int(ns.cursor[0]), *(getattr(ns, k).numpy() for k in out._fields[1:-1]), ns.correct.numpy().view(np.uint16))


def unpack_correct(mask):
    """uint16 masks [n] -> bool [n, 10] (val.py's `correct`)"""
    return (np.asarray(mask).astype(np.uint16)[:, None] >> np.arange(NIOU, dtype=np.uint16)) & 1 != 0


_LEVELS = {}


def _levels(device):
    key = (device.type, device.index)
    if key not in _LEVELS:
        _LEVELS[key] = torch.linspace(0.5, 0.95, NIOU).to(device)          # val.py:171
    return _LEVELS[key]


def _inputs(who, dets, counts, targets, size, shapes):
    """what both kernels take: -> (dets, counts, targets, shapes as contiguous float32 / int32 device tensors, bs, max_det, W, H)"""
    if not (dets.is_cuda and counts.is_cuda):
        raise RuntimeError(f"{who}: the HIP path needs CUDA/ROCm tensors (got {dets.device}); there is no CPU fallback")
    if dets.dim() != 3 or dets.shape[2] != 6 or counts.shape != (dets.shape[0],):
        raise ValueError(f"{who}: dets [bs, max_det, 6] and counts [bs] expected (got {tuple(dets.shape)}, {tuple(counts.shape)})")
    bs, max_det = dets.shape[0], dets.shape[1]
    W, H = (int(size), int(size)) if isinstance(size, (int, float)) else (int(size[0]), int(size[1]))
    dets = dets.float().contiguous()
    counts = counts.to(torch.int32).contiguous()
    targets = targets.to(dets.device).float().contiguous()
    if targets.dim() != 2 or targets.shape[1] != 6:
        raise ValueError(f"{who}: targets [nt, 6] = (image, class, x, y, w, h) expected (got {tuple(targets.shape)})")
    if shapes is not None:
        shapes = torch.as_tensor(shapes, dtype=torch.float32, device=dets.device).contiguous()
        if shapes.shape != (bs, 5):
            raise ValueError(f"{who}: shapes [bs, 5] = (h0, w0, gain, padw, padh) expected (got {tuple(shapes.shape)})")
    return dets, counts, targets, shapes, bs, max_det, W, H


def _launch(acc, dets, counts, targets, size, shapes, single_cls):
    dets, counts, targets, shapes, bs, max_det, W, H = _inputs("match_padded", dets, counts, targets, size, shapes)
    nt = targets.shape[0]
    lib, st = capi.lib(), capi.stream_ptr()
    capi.check(lib.ly_val_match(_p(dets), _p(counts), bs, max_det, _p(targets) if nt else _p(None), nt, W, H, _p(shapes), _p(_levels(dets.device)),
                                int(bool(single_cls)), acc.nc, _p(acc.cursor), acc.capacity, acc.row_width, _p(acc.correct), _p(acc.conf), _p(acc.cls),
                                _p(acc.match_label), _p(acc.match_iou), _p(acc.n_det), _p(acc.nt_class), _p(acc.overflow), st), "ly_val_match")
    return bs


def match_padded(dets, counts, targets, size, shapes=None, single_cls=False, out=None, nc=1):
    """val.py:150-166 + process_batch (val.py:79-101) for a batch, on the device, without a host synchronisation.
    dets [bs, max_det, 6] / counts [bs] as nms_padded returns them; targets [nt, 6] = (image, class, normalised xywh), the tensor
    ComputeLoss takes (rows of an image in any order and place); size: the network input size, s or (W, H); shapes: None (score at the
    letterboxed size) or [bs, 5] = (h0, w0, gain, padw, padh) per image (score in native space: scale_boxes with ratio_pad, clip_boxes).
    -> MatchAccumulator with one slot per image (fields correct — see unpack_correct —, conf, cls, match_label, match_iou, n_det, nt_class,
    overflow).  out: an accumulator to write at its cursor (the cursor is left where it is; Validator advances it); nc: classes of the
    label histogram when out is None.  An image with more than MAX_LABELS labels sets overflow and is not matched."""
    if out is None:
        out = MatchAccumulator(dets.shape[0], dets.shape[1], nc, dets.device)
    _launch(out, dets, counts, targets, size, shapes, single_cls)
    return out


class ConfusionMatrix:
    """utils/metrics.py `class ConfusionMatrix` on the device: the [nc + 1, nc + 1] matrix (row: predicted class, column: true class, index
    nc: background) that val.py fills per image with `process_batch(predn, labelsn)` at conf 0.25 / IoU 0.45.

        cm = ConfusionMatrix(nc)
        cm.update(nms_padded(z, 0.001, 0.6)[:2], targets, size)      # ly_val_confusion: one launch per batch, no host synchronisation
        m = cm.matrix()                                              # one synchronisation -> int64 numpy

    update takes what Validator.update takes as a (dets, counts) pair and ADDS to the matrix; it is capturable into a hipGraph with static
    inputs.  An image without labels adds nothing (val.py calls process_batch only for images with labels); one with labels and
    no detection above `conf` sends every label to the background row.  Limits: MAX_LABELS labels per image, classes inside [0, nc):
    matrix() raises and names the flag otherwise."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45, device="cuda"):
        if not 1 <= int(nc) <= 4096:
            raise ValueError(f"ConfusionMatrix: nc={nc} outside [1, 4096]")
        self.nc, self.conf, self.iou_thres = int(nc), float(conf), float(iou_thres)
        self.buf = torch.zeros((self.nc + 1) ** 2 + 1, dtype=torch.int32, device=torch.device(device))      # the matrix, then the flag word
        self._m, self._flags = self.buf[:-1], self.buf[-1:]

    def reset(self):
        self.buf.zero_()
        return self

    def update(self, pair, targets, size, shapes=None, single_cls=False):
        dets, counts, targets, shapes, bs, max_det, W, H = _inputs("ConfusionMatrix.update", *pair, targets, size, shapes)
        nt = targets.shape[0]
        capi.check(capi.lib().ly_val_confusion(_p(dets), _p(counts), bs, max_det, _p(targets) if nt else _p(None), nt, W, H, _p(shapes), self.conf,
                                               self.iou_thres, int(bool(single_cls)), self.nc, _p(self._m), _p(self._flags), capi.stream_ptr()),
                   "ly_val_confusion")

    def matrix(self):
        """one synchronisation, one copy -> [nc + 1, nc + 1] int64"""
        h = self.buf.cpu().numpy()
        if h[-1]:
            why = " and ".join(w for bit, w in ((OVF_LABELS, f"overflow of the {MAX_LABELS} labels an image may have (that image is not counted)"),
                                                (OVF_CLASS, f"a label or detection class outside [0, {self.nc})")) if h[-1] & bit)
            raise RuntimeError(f"ConfusionMatrix.matrix: {why}")
        return h[:-1].astype(np.int64).reshape(self.nc + 1, self.nc + 1)

    def tp_fp(self):
        """ConfusionMatrix.tp_fp: (true positives, false positives) per class, background left out"""
        m = self.matrix()
        tp = m.diagonal()
        return tp[:-1], (m.sum(1) - tp)[:-1]


ValResult = collections.namedtuple("ValResult", "mp mr map50 map p r ap50 ap nt classes")


class Validator:
    """val.py's scoring loop (val.py:127-188) with the per-image work on the device.

        v = Validator(nc)
        for imgs, targets in loader:
            v.update(model(imgs), targets)          # no host synchronisation; capturable into a hipGraph with static inputs
        mp, mr, map50, map_ = v.compute()[:4]       # one synchronisation, one copy

    update(pred, targets, shapes=None): pred is Detect's inference output (or the (inference, raw maps) pair of a model in eval mode), run
    through nms_padded with val.py's settings (conf_thres 0.001, iou_thres 0.6, multi_label = nc > 1), or an (dets, counts) pair already
    produced by nms_padded.  The network input size is taken from `size` (needed with a (dets, counts) pair).
    confusion=True: the Validator owns a ConfusionMatrix (`.confusion`, val.py's conf 0.25 / IoU 0.45) and update feeds it the same
    detections, targets and shapes behind ly_val_match; reset() zeroes it too.
    Limits: at most `capacity_images` images between two reset() calls (update raises on the host beyond it), at most MAX_LABELS labels per
    image and label classes inside [0, nc) (compute raises and names the images otherwise), max_det detections per image."""

    def __init__(self, nc, conf_thres=0.001, iou_thres=0.6, max_det=300, capacity_images=5000, single_cls=False, size=None, device="cuda",
                 confusion=False):
        self.nc, self.conf_thres, self.iou_thres, self.max_det, self.single_cls = int(nc), conf_thres, iou_thres, int(max_det), bool(single_cls)
        self.size = size
        self.acc = MatchAccumulator(capacity_images, self.max_det, self.nc, torch.device(device))
        self.confusion = ConfusionMatrix(self.nc, device=device) if confusion else None
        self._seen = 0                       # images handed to update() on the host (graph replays are counted by the device cursor only)

    @property
    def capacity_images(self):
        return self.acc.capacity

    def reset(self):
        self.acc.zero_()
        if self.confusion is not None:
            self.confusion.reset()
        self._seen = 0
        return self

    def update(self, pred, targets, shapes=None, size=None):
        pair = isinstance(pred, (tuple, list)) and len(pred) == 2 and torch.is_tensor(pred[1]) and pred[1].dim() == 1 and not pred[1].is_floating_point()
        size = size if size is not None else self.size
        if pair:
            dets, counts = pred
            if dets.shape[1] > self.max_det:
                raise ValueError(f"Validator.update: dets hold {dets.shape[1]} rows per image, the accumulator max_det = {self.max_det}")
        else:
            z = pred[0] if isinstance(pred, (tuple, list)) else pred
            dets, counts, _ = nms_padded(z, self.conf_thres, self.iou_thres, max_det=self.max_det, multi_label=self.nc > 1)      # val.py:230-234
        if size is None:
            raise ValueError("Validator.update: the network input size is needed (Validator(size=...) or update(..., size=...))")
        bs = dets.shape[0]
        if self._seen + bs > self.acc.capacity:
            raise RuntimeError(f"Validator.update: {self._seen} + {bs} images exceed capacity_images = {self.acc.capacity}")
        _launch(self.acc, dets, counts, targets, size, shapes, self.single_cls)
        capi.check(capi.lib().ly_val_advance(_p(self.acc.cursor), bs, capi.stream_ptr()), "ly_val_advance")
        if self.confusion is not None:
            self.confusion.update((dets, counts), targets, size, shapes, self.single_cls)
        self._seen += bs

    def stats(self):
        """one synchronisation, one copy -> (correct bool [n, 10], conf [n], cls [n], nt_per_class [nc]) over all images, in update order"""
        h = self.acc.host()
        if h.cursor > self.acc.capacity:
            raise RuntimeError(f"Validator: {h.cursor} images were scored into an accumulator of capacity_images = {self.acc.capacity}")
        n = h.cursor
        bad = np.nonzero(h.overflow[:n])[0]
        if len(bad):
            why = [f"image {i}: " + " and ".join(w for bit, w in ((OVF_LABELS, f"overflow of the {MAX_LABELS} labels an image may have"),
                                                                 (OVF_CLASS, f"a label class outside [0, {self.nc})")) if h.overflow[i] & bit)
                   for i in bad[:8]]
            raise RuntimeError(f"Validator.compute: label overflow in {len(bad)} image(s): " + "; ".join(why))
        keep = np.arange(self.acc.row_width)[None, :] < h.n_det[:n, None]
        return unpack_correct(h.correct[:n][keep]), h.conf[:n][keep], h.cls[:n][keep], h.nt_class[:n].sum(0)

    def compute(self, stats=None):
        """-> ValResult(mp, mr, map50, map, p, r, ap50, ap, nt, classes): val.py:183-188; the per-class arrays cover the classes that have
        labels.  Four zeros when no detection is correct (val.py:184).  stats: what stats() returned, when the caller holds it already."""
        correct, conf, cls, nt = stats if stats is not None else self.stats()
        classes = np.nonzero(nt > 0)[0]
        if not (len(correct) and correct.any()):
            e = np.zeros(0)
            return ValResult(0.0, 0.0, 0.0, 0.0, e, e, e, e, nt[classes], classes)
        _, _, p, r, _, ap, classes = ap_per_class(correct, conf, cls, nt_per_class=nt)
        ap50, ap = ap[:, 0], ap.mean(1)
        return ValResult(float(p.mean()), float(r.mean()), float(ap50.mean()), float(ap.mean()), p, r, ap50, ap, nt[classes], classes)
