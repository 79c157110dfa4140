"""Whole scenes: detection on an image far larger than the model's input, at native resolution, on the device.

SAR imagery arrives as scenes of 10 000 to 30 000 pixels a side that carry ships of 10 to 100 pixels; `Detector` would letterbox such a scene
down to 640 pixels and lose every ship.  `SceneDetector` cuts the scene into overlapping tiles (csrc/ly_scene.hip: ly_scene_tiles_u8, straight
into the forward's input buffer), runs them in chunks through the same graphed forward and `nms_padded` as `Detector`, shifts the tiles'
boxes into scene pixels (ly_scene_collect) and removes the duplicates the overlaps produce (one torch.sort, ly_scene_nms) — the host loop a
user of the reference writes around detect.py (slice, pad, transpose, shift, de-duplicate in numpy), without a host round trip per tile.

    sd = SceneDetector(model.eval(), tile=640, overlap=128, batch_size=32)
    boxes = sd(scene)                   # [n, 6] xyxy in scene pixels, conf, cls; one synchronisation
    dets, count = sd.padded(scene)      # [max_det, 6] rows past count zero, count [1] int32; no synchronisation
    tiles = sd.tiles_padded(scene)      # (dets [n_tiles, max_det_tile, 6] in tile pixels, counts, origins): the state before the merge

`scene_plan` is the host arithmetic alone (no device).

Out of scope, each refused where it can be asked for: resizing tiles (scenes run at native resolution: there is no img_size), augment=True,
merging duplicates into their union (a duplicate is dropped, the higher score's box stays as it is), scoring scenes with `Validator`
(padded() returns one scene's boxes, not the per-image rows Validator.update takes), and 16-bit sources (scale to uint8 first)."""
import numpy as np
import torch

from . import capi
from .graph import GraphedForward
from .nms import MAX_NMS, nms_padded
from .predict import FILL, _device

METRICS = {"iou": 0, "ios": 1}              # `metric` codes of ly_scene_nms


def _axis(L, tile, step):
    if L <= tile:
        return [0]
    n = -(-(L - tile) // step) + 1
    return [min(i * step, L - tile) for i in range(n)]


def scene_plan(H, W, tile=640, overlap=128):
    """Tile origins for an H x W scene -> (origins int32 [n, 2] = (y0, x0), row-major with y outer, (ny, nx) the per-axis counts).

    Requires tile > 0 and 0 <= overlap <= tile // 2.  Per axis of length L, with step = tile - overlap: L <= tile gives the single origin 0
    (the tile hangs over the scene's edge: 114-padding); otherwise n = ceil((L - tile) / step) + 1 origins o_i = min(i * step, L - tile) —
    the last tile is pulled back to END on the scene's edge instead of hanging over it.

    Guarantees: every pixel is covered; consecutive tiles share at least `overlap` pixels; any interval of length <= overlap inside [0, L)
    lies wholly inside at least one tile.  So: choose `overlap` at least as large as the largest object, and every object is seen whole by
    some tile."""
    H, W, tile, overlap = int(H), int(W), int(tile), int(overlap)
    if tile <= 0:
        raise ValueError(f"scene_plan: tile {tile} must be positive")
    if not 0 <= overlap <= tile // 2:
        raise ValueError(f"scene_plan: overlap {overlap} outside [0, tile // 2 = {tile // 2}]")
    if H < 1 or W < 1:
        raise ValueError(f"scene_plan: the scene is {H} x {W}")
    ys, xs = _axis(H, tile, tile - overlap), _axis(W, tile, tile - overlap)
    origins = np.array([(y, x) for y in ys for x in xs], dtype=np.int32).reshape(-1, 2)
    return origins, (len(ys), len(xs))


# ---- device plumbing ----------------------------------------------------------------------------------------------------------------------
def _to_device(host, dev):
    """a host array on the device: one non-blocking copy from a fresh pinned block on the current stream (as predict._sources)"""
    pinned = torch.empty(host.shape, dtype={np.uint8: torch.uint8, np.int32: torch.int32}[host.dtype.type], pin_memory=True)
    pinned.numpy()[...] = host
    out = torch.empty(host.shape, dtype=pinned.dtype, device=dev)
    out.copy_(pinned, non_blocking=True)
    return out


def _scene_source(scene, dev, who):
    """a uint8 [H, W, 3] (HWC BGR) or [H, W] (grey) scene -> (device tensor to address — and to keep referenced until the launches ran —,
    H, W, C, row pitch in bytes).  A device tensor is read where it is: it may be a row / column view (a pitch) but its pixels must be packed.
    A host array (numpy, CPU tensor) goes up once through one pinned block."""
    shape, dtype = tuple(scene.shape), scene.dtype
    if dtype in (np.uint16, np.int16, torch.int16, getattr(torch, "uint16", None)):
        raise NotImplementedError(f"{who}: 16-bit sources are out of scope (got {dtype}): scale the amplitudes to uint8 first")
    if dtype not in (np.uint8, torch.uint8) or len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 3) or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{who}: the scene must be uint8 [H, W, 3] (HWC BGR) or [H, W] (grey) (got {dtype} {shape})")
    H, W, C = shape[0], shape[1], 3 if len(shape) == 3 else 1
    if isinstance(scene, torch.Tensor) and scene.is_cuda:
        st = scene.stride()
        if scene.device != dev or st[1] != C or (C == 3 and st[2] != 1) or (H > 1 and st[0] < W * C):
            raise ValueError(f"{who}: a device scene must be on {dev} with unit pixel stride and a row pitch >= W * C (got strides {st} on "
                             f"{scene.device})")
        return scene, H, W, C, max(int(st[0]), W * C)
    host = scene.numpy() if isinstance(scene, torch.Tensor) else np.asarray(scene)
    return _to_device(np.ascontiguousarray(host), dev), H, W, C, W * C


def _launch_tiles(src, H, W, C, pitch, origins_dev, n, T, dst):
    capi.check(capi.lib().ly_scene_tiles_u8(capi.ptr(src), H, W, C, pitch, capi.ptr(origins_dev), n, T, capi.ptr(dst), capi.stream_ptr()),
               "ly_scene_tiles_u8")


def scene_tiles(scene, origins, tile, out=None, device=None):
    """The windows of `scene` at `origins` ([n, 2] (y0, x0), a HOST array: their range is checked here) as the model's input: uint8
    [n, 3, tile, tile] RGB planes, 114 past the scene's edges.  One ly_scene_tiles_u8 launch on the current stream, no host synchronisation.
    out: write into this contiguous, 16-byte aligned uint8 [n, 3, tile, tile] device tensor."""
    dev = out.device if out is not None else scene.device if isinstance(scene, torch.Tensor) and scene.is_cuda else None
    dev = _device(dev if dev is not None else device)
    src, H, W, C, pitch = _scene_source(scene, dev, "scene_tiles")
    origins = np.ascontiguousarray(np.asarray(origins, dtype=np.int32).reshape(-1, 2))
    n, T = len(origins), int(tile)
    if n < 1:
        raise ValueError("scene_tiles: no origins")
    if T < 16 or T % 16:
        raise ValueError(f"scene_tiles: tile {T} must be a multiple of 16")
    bad = (origins < 0).any(1) | (origins[:, 0] >= H) | (origins[:, 1] >= W)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError(f"scene_tiles: origin {k} = {tuple(origins[k].tolist())} is outside the {H} x {W} scene")
    if out is None:
        out = torch.empty((n, 3, T, T), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n, 3, T, T) or not out.is_contiguous() or not out.is_cuda or out.data_ptr() % 16:
        raise ValueError(f"scene_tiles: out must be a contiguous, 16-byte aligned uint8 [{n}, 3, {T}, {T}] device tensor (got {out.dtype} "
                         f"{tuple(out.shape)} on {out.device})")
    _launch_tiles(src, H, W, C, pitch, _to_device(origins, dev), n, T, out)
    return out


def scene_collect(dets, counts, origins, H, W):
    """what nms_padded returned for the tiles (dets [n_tiles, max_det, 6], counts [n_tiles]; tiles of several chunks concatenated) and the
    tiles' origins [n_tiles, 2] int32 on the device -> (boxes [n_tiles * max_det, 6] in scene pixels, clipped to the scene, score: conf, -1
    for the padding rows).  One ly_scene_collect launch, no host synchronisation."""
    if not (dets.is_cuda and dets.dtype == torch.float32 and dets.is_contiguous() and dets.dim() == 3 and dets.shape[2] == 6):
        raise ValueError(f"scene_collect: dets must be a contiguous float32 [n_tiles, max_det, 6] device tensor (got {dets.dtype} {tuple(dets.shape)})")
    n, md = dets.shape[0], dets.shape[1]
    counts = counts.to(torch.int32).contiguous()
    origins = origins.to(torch.int32).contiguous()
    if counts.shape != (n,) or origins.shape != (n, 2) or counts.device != dets.device or origins.device != dets.device:
        raise ValueError(f"scene_collect: counts [n_tiles] and origins [n_tiles, 2] on {dets.device} expected (got {tuple(counts.shape)}, "
                         f"{tuple(origins.shape)})")
    boxes = torch.empty((n * md, 6), dtype=torch.float32, device=dets.device)
    score = torch.empty((n * md,), dtype=torch.float32, device=dets.device)
    capi.check(capi.lib().ly_scene_collect(capi.ptr(dets), capi.ptr(counts), capi.ptr(origins), n, md, int(H), int(W), capi.ptr(boxes), capi.ptr(score),
                                           capi.stream_ptr()), "ly_scene_collect")
    return boxes, score


def scene_merge(boxes, score, max_det_tile, metric="ios", thres=0.5, agnostic=False, max_det=3000, max_merge=MAX_NMS):
    """Greedy suppression across tiles on scene_collect's rows -> (keep [max_det] int32 row indices in kept order, the rest 0, count [1]
    int32).  One stable descending torch.sort and one ly_scene_nms launch (the rule and its fp32 metric: include/lead_yolo_hip.h); no host
    synchronisation."""
    if metric not in METRICS:
        raise ValueError(f"scene_merge: metric must be 'iou' or 'ios' (got {metric!r})")
    if not (boxes.is_cuda and boxes.dtype == torch.float32 and boxes.is_contiguous() and boxes.dim() == 2 and boxes.shape[1] == 6):
        raise ValueError(f"scene_merge: boxes must be a contiguous float32 [N, 6] device tensor (got {boxes.dtype} {tuple(boxes.shape)})")
    N = boxes.shape[0]
    if score.shape != (N,) or score.dtype != torch.float32 or score.device != boxes.device or N < 1:
        raise ValueError(f"scene_merge: score must be float32 [{N}] on {boxes.device} (got {score.dtype} {tuple(score.shape)})")
    svals, order = torch.sort(score.contiguous(), descending=True, stable=True)
    keep = torch.empty((int(max_det),), dtype=torch.int32, device=boxes.device)
    count = torch.empty((1,), dtype=torch.int32, device=boxes.device)
    capi.check(capi.lib().ly_scene_nms(capi.ptr(boxes), capi.ptr(order), capi.ptr(svals), N, int(max_det_tile), METRICS[metric], float(thres),
                                       int(bool(agnostic)), int(max_det), int(max_merge), capi.ptr(keep), capi.ptr(count), capi.stream_ptr()),
               "ly_scene_nms")
    return keep, count


class SceneDetector:
    """detect.py's loop for a scene larger than the model's input: tiles -> forward -> per-tile NMS -> boxes in scene pixels -> cross-tile
    merge, everything on the device.

    sd(scene)              -> [n, 6] tensor (xyxy in scene pixels, conf, cls), by descending confidence; one synchronisation at the end (the
                              slice needs the count on the host).  A list of scenes returns a list (still one synchronisation).
    sd.padded(scene)       -> (dets [max_det, 6] rows past the count zero, count [1] int32), no synchronisation
    sd.tiles_padded(scene) -> (dets [n_tiles, max_det_tile, 6] in TILE pixels, counts [n_tiles], origins [n_tiles, 2] int32 (y0, x0)), all
                              on the device: the state before the merge

    scene: uint8 [H, W, 3] (HWC BGR, cv2.imread's form) or [H, W] (one grey plane — the raw SAR amplitude — fed to all three channels).  A
    device tensor is read where it is and may be a view with a row pitch (a crop of a larger scene) but needs unit pixel stride; a host array
    goes up once through one pinned block.  The scene runs at NATIVE resolution: scene_plan(H, W, tile, overlap) places the tiles — choose
    `overlap` at least as large as the largest object, so that some tile sees it whole.

    The tiles run in chunks of batch_size on one fixed [batch_size, 3, tile, tile] batch, exactly as Detector's images: free slots of the last
    chunk are all-114 tiles whose rows are dropped; the batch goes to the model as uint8 when model.u8_input, else as batch.to(dtype) / 255;
    graphed=True holds one GraphedForward on that batch and ly_scene_tiles_u8 writes straight into its input buffer — it does not follow
    weight changes: stale() tells, refresh() captures anew.  Each chunk goes through nms_padded(conf_thres, iou_thres, classes, agnostic,
    multi_label, max_det=max_det_tile).

    The merge walks all tiles' boxes by descending confidence and drops a box when a kept box of ANOTHER tile and the same class (any class
    with agnostic) overlaps it by more than merge_thres; pairs of one tile are nms_padded's, so a scene of one tile returns what the per-tile
    NMS returned.  metric "ios" (the default) is the intersection over the smaller box: an object cut by a tile border gives a partial box
    inside the full box of the neighbour tile, whose IoU ("iou") is far below any usable threshold.  At most 30000 candidates (by descending confidence)
    enter the merge and max_det boxes leave it.  The host knows the number of tiles from the plan: nothing synchronises before the final count.

    Out of scope: resizing tiles, augment=True (raises), merging boxes into their union, scoring scenes with Validator, 16-bit sources
    (raises).  The mixed-precision policy is the caller's: construct and call under the autocast context the model should run in."""

    def __init__(self, model, tile=640, overlap=128, batch_size=32, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False,
                 multi_label=False, max_det_tile=300, metric="ios", merge_thres=0.5, max_det=3000, graphed=True, augment=False):
        if model.training:
            raise RuntimeError("SceneDetector runs the inference forward: call model.eval() first")
        if augment:
            raise NotImplementedError("SceneDetector: augment=True is out of scope (tiles run through the plain inference forward)")
        if metric not in METRICS:
            raise ValueError(f"SceneDetector: metric must be 'iou' (a duplicate is a box of similar extent) or 'ios' (intersection over the "
                             f"smaller box; merging boxes into their union is out of scope) (got {metric!r})")
        self.model = model
        self.stride = int(model.stride.max())
        self.tile, self.overlap, self.batch_size = int(tile), int(overlap), int(batch_size)
        if self.tile < self.stride or self.tile % self.stride or self.tile % 16 or self.batch_size < 1:
            raise ValueError(f"SceneDetector: tile {tile} must be a multiple of the model's stride {self.stride} (and of 16), batch_size "
                             f"{batch_size} >= 1")
        if not 0 <= self.overlap <= self.tile // 2:
            raise ValueError(f"SceneDetector: overlap {overlap} outside [0, tile // 2 = {self.tile // 2}]")
        if not 0 <= merge_thres <= 1:
            raise ValueError(f"SceneDetector: invalid threshold merge_thres={merge_thres}: valid values are between 0.0 and 1.0")
        self.max_det_tile, self.max_det = int(max_det_tile), int(max_det)
        if self.max_det_tile < 1 or self.max_det < 1:
            raise ValueError(f"SceneDetector: max_det_tile {max_det_tile} and max_det {max_det} must be positive")
        self.nms = dict(conf_thres=conf_thres, iou_thres=iou_thres, classes=classes, agnostic=agnostic, max_det=self.max_det_tile,
                        multi_label=multi_label)
        self.metric, self.merge_thres, self.agnostic = metric, float(merge_thres), bool(agnostic)
        self.graphed = bool(graphed)
        p = next(model.parameters())
        self.device, self.dtype = p.device, p.dtype
        self.u8 = bool(getattr(model, "u8_input", False))
        shape = (self.batch_size, 3, self.tile, self.tile)
        self._g = None
        self._x = torch.zeros(shape, dtype=torch.uint8 if self.u8 else self.dtype, device=self.device)
        if self.graphed:
            self.refresh()
        self._u8 = self._x if self.u8 else torch.empty(shape, dtype=torch.uint8, device=self.device)

    def stale(self):
        """GraphedForward.stale() of the captured forward (False for the eager form, which follows the weights by itself)"""
        return self._g is not None and self._g.stale()

    def refresh(self):
        """capture the forward anew with the weights the model holds now"""
        if self.graphed:
            self._g = None                                  # the old graph's pools go first
            self._g = GraphedForward(self.model, self._x)
            self._x = self._g.x
            if self.u8:
                self._u8 = self._x
        return self

    def _forward(self, x):
        if self._g is not None:
            return self._g()[0]
        with torch.no_grad():
            return self.model(x)[0]

    def _tiles(self, scene):
        src, H, W, C, pitch = _scene_source(scene, self.device, "SceneDetector")
        origins, _ = scene_plan(H, W, self.tile, self.overlap)
        n, bs = len(origins), self.batch_size
        origins_dev = _to_device(origins, self.device)
        dets = torch.empty((n, self.max_det_tile, 6), dtype=torch.float32, device=self.device)
        counts = torch.empty((n,), dtype=torch.int32, device=self.device)
        for lo in range(0, n, bs):
            k = min(bs, n - lo)
            _launch_tiles(src, H, W, C, pitch, origins_dev[lo:lo + k], k, self.tile, self._u8)
            if k < bs:
                self._u8[k:].fill_(FILL)
            if not self.u8:
                self._x.copy_(self._u8.to(self.dtype) / 255)
            d, c, _ = nms_padded(self._forward(self._x), **self.nms)
            dets[lo:lo + k] = d[:k]
            counts[lo:lo + k] = c[:k]
        del src
        return dets, counts, origins_dev, H, W

    def tiles_padded(self, scene):
        return self._tiles(scene)[:3]

    def padded(self, scene):
        dets, counts, origins, H, W = self._tiles(scene)
        boxes, score = scene_collect(dets, counts, origins, H, W)
        keep, count = scene_merge(boxes, score, self.max_det_tile, self.metric, self.merge_thres, self.agnostic, self.max_det)
        rows = boxes[keep.long()]
        valid = torch.arange(self.max_det, device=self.device) < count
        return rows * valid.unsqueeze(-1), count

    def __call__(self, scene):
        many = isinstance(scene, (list, tuple))
        scenes = list(scene) if many else [scene]
        if not scenes:
            raise ValueError("SceneDetector: no scenes")
        parts = [self.padded(s) for s in scenes]
        counts = torch.cat([c for _, c in parts]).tolist()                   # the one synchronisation
        out = [d[:c] for (d, _), c in zip(parts, counts)]
        return out if many else out[0]
