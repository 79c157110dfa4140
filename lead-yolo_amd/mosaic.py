"""On-device training augmentation: the batch LoadImagesAndLabels.__getitem__ + collate_fn build on the CPU (utils/dataloaders.py, augment=True):
load_mosaic (or letterbox), random_perspective, augment_hsv, flipud / fliplr, HWC BGR -> CHW RGB, and the label rows — as two HIP launches per
batch (csrc/ly_mosaic.hip) that write the uint8 NCHW batch and the fixed-shape padded `targets` the training step reads.

    bank = ImageBank.from_dataset(ds)                  # or ImageBank(images, labels, img_size): load_image results, decoded once;
                                                       # or ImageBank.from_native(images, labels, img_size): decoded images, resized on the device
    aug = MosaicAugment(bank, hyp, batch_size=64, seed=0)
    imgs, targets = aug(next_indices)                  # (uint8 [bs, 3, s, s], float32 [aug.capacity, 6]); no host sync
    aug(next_indices, out=(step.imgs, step.targets))   # straight into a GraphedTrainStep's captured buffers; then step()

The random draws happen on the host with the reference's distributions (numpy's generator, not Python's `random`: the same distributions, not the
same stream).  Each draw is turned into one LyMosaicImage entry (placement rectangles with load_mosaic's formulas, M = T @ S @ R @ C and its
float64 inverse, the HSV LUTs of augment_hsv, the flip bits); the table goes to the device with one non-blocking copy from pinned memory.

Mixup (hyp['mixup'] > 0, the reference's medium / high hyper-parameter files) is opt-in: MosaicAugment(..., allow_mixup=True).  A mosaic image
then draws, with that probability, a second independent mosaic and a ratio from beta(32, 32); the device blends the two warped images as
`mixup_blend` states it and appends the second mosaic's label rows, so `capacity` is batch_size * 8 * max_labels: a GraphedTrainStep fed by
such an augmenter is constructed with targets of that shape.  copy_paste and perspective remain refused."""
import ctypes
import math

import numpy as np
import torch

from . import capi

# data/hyps/hyp.scratch-low.yaml: the augmentation keys
HYP_SCRATCH_LOW = dict(hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0, flipud=0.0,
                       fliplr=0.5, mosaic=1.0, mixup=0.0, copy_paste=0.0)
FILL = 114                      # load_mosaic's canvas, letterbox's border and warpAffine's borderValue


class ImageBank:
    """Every training image, decoded and resized once (`load_image` results: uint8 HWC, long side = img_size), in ONE device buffer with a
    per-image (offset, h, w) table, and every image's labels ([n, 5]: cls, normalised xywh) in one flat float64 device array — the
    reference's `--cache ram`, on the device.  bgr=False: the images are RGB and are converted on upload."""

    def __init__(self, images, labels, img_size, bgr=True, device=None):
        if len(images) == 0 or len(images) != len(labels):
            raise ValueError(f"ImageBank: {len(images)} images and {len(labels)} label arrays (need the same, non-zero count)")
        self.img_size = int(img_size)
        dev = torch.device(device if device is not None else "cuda")
        self.device = torch.device("cuda", torch.cuda.current_device()) if dev.type == "cuda" and dev.index is None else dev
        hw, flat, off = [], [], 0
        offs = []
        for i, im in enumerate(images):
            a = im.cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"ImageBank: image {i} must be uint8 HWC with 3 channels (got {a.dtype} {a.shape})")
            if not bgr:
                a = a[..., ::-1]
            a = np.ascontiguousarray(a)
            hw.append(a.shape[:2])
            offs.append(off)
            off += a.size
            flat.append(a.reshape(-1))
        self.hw = np.array(hw, dtype=np.int64).reshape(-1, 2)
        self.off = np.array(offs, dtype=np.int64)
        self.data = torch.from_numpy(np.concatenate(flat)).to(self.device)
        self._set_labels(labels)

    def _set_labels(self, labels):
        labs, lab_off, nlab, r = [], [], [], 0
        for i, lb in enumerate(labels):
            a = np.asarray(lb.cpu().numpy() if isinstance(lb, torch.Tensor) else lb, dtype=np.float64).reshape(-1, 5) if len(lb) else np.zeros((0, 5))
            labs.append(a)
            lab_off.append(r)
            nlab.append(a.shape[0])
            r += a.shape[0]
        self.host_labels = labs
        self.lab_off = np.array(lab_off, dtype=np.int64)
        self.nlab = np.array(nlab, dtype=np.int64)
        self.max_labels = int(self.nlab.max())
        self.labels = torch.from_numpy(np.concatenate(labs, 0) if r else np.zeros((0, 5))).to(self.device)

    @classmethod
    def from_dataset(cls, ds, device=None):
        """a reference LoadImagesAndLabels (duck-typed: len(), load_image(i) -> (im, hw0, hw), .labels, .img_size): every image decoded and
        resized once, as its `--cache ram` does"""
        return cls([ds.load_image(i)[0] for i in range(len(ds))], ds.labels, ds.img_size, bgr=True, device=device)

    @classmethod
    def from_native(cls, images, labels, img_size, device=None):
        """`load_image` on the device: images as decoded (uint8 HWC BGR of any sizes; numpy arrays, CPU tensors or contiguous device tensors),
        each resized so that its long side is img_size — predict.load_image_size, truncated as
        load_image does — by one ly_letterbox_u8 launch (layout HWC BGR) straight into the bank buffer.  The interpolation is always
        INTER_LINEAR, which is what load_image uses for the augment=True loader this bank feeds (it takes INTER_AREA only for a
        non-augmenting loader that shrinks); an image whose long side is img_size already is copied."""
        from . import predict
        if len(images) == 0 or len(images) != len(labels):
            raise ValueError(f"ImageBank: {len(images)} images and {len(labels)} label arrays (need the same, non-zero count)")
        self = cls.__new__(cls)
        self.img_size = int(img_size)
        self.device = predict._device(device)
        src, keep = predict._sources(images, self.device, "ImageBank.from_native")
        n = len(src)
        table = (capi.LyLetterboxImage * n)()
        hw, offs, off = [], [], 0
        for i, (_, h0, w0) in enumerate(src):
            nh, nw = predict.load_image_size(h0, w0, self.img_size)
            if nh < 1 or nw < 1:
                raise ValueError(f"ImageBank.from_native: image {i} ({h0} x {w0}) would be resized to {nh} x {nw}")
            hw.append((nh, nw))
            offs.append(off)
            off += nh * nw * 3
        self.hw = np.array(hw, dtype=np.int64).reshape(-1, 2)
        self.off = np.array(offs, dtype=np.int64)
        self.data = torch.empty(off, dtype=torch.uint8, device=self.device)
        for i, (p, h0, w0) in enumerate(src):
            nh, nw = hw[i]
            table[i] = capi.LyLetterboxImage(p, self.data.data_ptr() + offs[i], h0, w0, nh, nw, nh, nw, 0, 0)
        table_dev, _ = predict._upload(table, np.zeros(0, dtype=np.float32), self.device)
        predict._launch(table_dev, n, int(self.hw[:, 0].max()), int(self.hw[:, 1].max()), predict.LB_HWC_BGR)
        del keep
        self._set_labels(labels)
        return self

    def __len__(self):
        return len(self.hw)


# ---- the reference's host formulas (utils/dataloaders.py load_mosaic, utils/augmentations.py letterbox / random_perspective / augment_hsv) ----
def mosaic_placement(s, xc, yc, hw):
    """load_mosaic's placement of four images of sizes hw[i] = (h, w) around the centre (xc, yc) of the 2s x 2s canvas: per tile
    (x1a, y1a, x2a, y2a) on the canvas and (x1b, y1b, x2b, y2b) in the source"""
    out = []
    for i, (h, w) in enumerate(hw):
        if i == 0:  # top left
            x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
            x1b, y1b, x2b, y2b = w - (x2a - x1a), h - (y2a - y1a), w, h
        elif i == 1:  # top right
            x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, s * 2), yc
            x1b, y1b, x2b, y2b = 0, h - (y2a - y1a), min(w, x2a - x1a), h
        elif i == 2:  # bottom left
            x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(s * 2, yc + h)
            x1b, y1b, x2b, y2b = w - (x2a - x1a), 0, w, min(y2a - y1a, h)
        else:  # bottom right
            x1a, y1a, x2a, y2a = xc, yc, min(xc + w, s * 2), min(s * 2, yc + h)
            x1b, y1b, x2b, y2b = 0, 0, min(w, x2a - x1a), min(y2a - y1a, h)
        out.append((x1a, y1a, x2a, y2a, x1b, y1b, x2b, y2b))
    return out


def letterbox_pads(s, h, w):
    """letterbox(im, s, auto=False) of an image whose long side is already s (load_image): -> (left, top, dw, dh), the integer border and
    the float half-pads the labels are shifted by"""
    r = min(s / h, s / w)
    if r != 1.0:
        raise ValueError(f"letterbox of a {h} x {w} image onto {s}: the device path places load_image results (long side = img_size) without "
                         "resizing them")
    dw, dh = (s - w) / 2, (s - h) / 2
    return int(round(dw - 0.1)), int(round(dh - 0.1)), dw, dh


def perspective_matrix(in_w, in_h, out_w, out_h, degrees, scale, shear_x, shear_y, trans_x, trans_y):
    """random_perspective's M = T @ S @ R @ C (perspective 0) from its draws: rotation `degrees`, `scale`, shear angles in degrees, translate
    draws in [0.5 - t, 0.5 + t] (fractions of the output size); in_w x in_h is the image it warps"""
    C = np.eye(3)
    C[0, 2] = -in_w / 2
    C[1, 2] = -in_h / 2
    R = np.eye(3)
    ang = degrees * math.pi / 180                    # cv2.getRotationMatrix2D(angle, center=(0, 0), scale) in double
    alpha, beta = math.cos(ang) * scale, math.sin(ang) * scale
    R[:2] = [[alpha, beta, 0.0], [-beta, alpha, 0.0]]
    S = np.eye(3)
    S[0, 1] = math.tan(shear_x * math.pi / 180)
    S[1, 0] = math.tan(shear_y * math.pi / 180)
    T = np.eye(3)
    T[0, 2] = trans_x * out_w
    T[1, 2] = trans_y * out_h
    return T @ S @ R @ C


def invert_affine(M):
    """cv2.invertAffineTransform of M[:2] in float64 -> [2, 3] (what warpAffine samples with)"""
    a, b, c = M[0]
    d, e, f = M[1]
    D = a * e - b * d
    D = 1.0 / D if D != 0 else 0.0
    A11, A22, A12, A21 = e * D, a * D, -b * D, -d * D
    return np.array([[A11, A12, -A11 * c - A12 * f], [A21, A22, -A21 * c - A22 * f]])


def hsv_luts(gains):
    """augment_hsv's three LUTs (hue, saturation, value) for the gains r = uniform(-1, 1, 3) * [h, s, v] + 1, float64 as numpy builds them"""
    r = np.asarray(gains, dtype=np.float64)
    x = np.arange(0, 256, dtype=r.dtype)
    return np.stack([((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8), np.clip(x * r[2], 0, 255).astype(np.uint8)])


def mixup_blend(a, b, r):
    """utils/augmentations.py mixup's image: `(im * r + im2 * (1 - r)).astype(np.uint8)` — for uint8 images float64 arithmetic, then
    truncation (r = 0.4105263202137452 takes two 114s to 113.99999999999999, stored as 113)"""
    return (a * r + b * (1 - r)).astype(np.uint8)


class Draw:
    """One output image's random draws.  mosaic: `sources` are the four bank indices in tile order and (xc, yc) the canvas centre; letterbox:
    one source.  degrees / scale / shear = (x, y) / translate = (x, y) as random_perspective draws them; gains: the three HSV gains or None.
    partner: the mosaic Draw of mixup's second image (its own sources, centre and random_perspective draws; no gains and no flips: HSV and
    the flips act on the blended image and are this draw's) or None; ratio: the weight of this image in the blend."""
    __slots__ = ("mosaic", "sources", "xc", "yc", "degrees", "scale", "shear", "translate", "gains", "flipud", "fliplr", "partner", "ratio")

    def __init__(self, mosaic, sources, xc=0, yc=0, degrees=0.0, scale=1.0, shear=(0.0, 0.0), translate=(0.5, 0.5), gains=None, flipud=False,
                 fliplr=False, partner=None, ratio=None):
        if partner is not None and not (mosaic and partner.mosaic and partner.partner is None and ratio is not None):
            raise ValueError("Draw: a mixup partner is a mosaic draw without a partner of its own, for a mosaic draw, with a ratio")
        self.partner, self.ratio = partner, None if ratio is None else float(ratio)
        self.mosaic, self.sources, self.xc, self.yc = bool(mosaic), [int(i) for i in sources], int(xc), int(yc)
        self.degrees, self.scale, self.shear, self.translate = float(degrees), float(scale), tuple(shear), tuple(translate)
        self.gains = None if gains is None else np.asarray(gains, dtype=np.float64)
        self.flipud, self.fliplr = bool(flipud), bool(fliplr)


class Plan:
    """The parameter table of one batch: `table` (ctypes LyMosaicImage array, lut pointers unset), `luts` [n, 3, 256] uint8, the draws, and per
    image the forward matrix M (3 x 3 float64).  Mixup: `partner_table` (LyMosaicImage array, one entry per draw that has a partner, in image
    order; None when there is none) and `mix` (LyMixup * n: partner = n + the position in partner_table, or -1; r = the draw's ratio)"""

    def __init__(self, table, luts, draws, mats, partner_table=None, mix=None):
        self.table, self.luts, self.draws, self.mats = table, luts, draws, mats
        self.n = len(draws)
        self.partner_table = partner_table
        self.k = len(partner_table) if partner_table is not None else 0
        self.mix = mix if mix is not None else (capi.LyMixup * self.n)(*[capi.LyMixup(-1, 0, 0.0) for _ in range(self.n)])


class MosaicAugment:
    """Batches of augmented training images from an ImageBank, built on the device (see the module docstring).  hyp: the reference's keys
    (default hyp.scratch-low); copy_paste and perspective are not implemented, mixup needs allow_mixup=True.  capacity = batch_size * 4 *
    bank.max_labels target rows (* 8 with mixup: two mosaics per image): fixed, so the target tensor has one shape for every batch (rows past
    the batch's labels are padding, image index -1)."""

    def __init__(self, bank, hyp=None, batch_size=16, seed=0, allow_mixup=False):
        h = dict(HYP_SCRATCH_LOW)
        h.update(hyp or {})
        if h["mixup"] > 0 and not allow_mixup:
            raise NotImplementedError("MosaicAugment: mixup > 0 doubles the target rows (capacity = batch_size * 8 * max_labels): pass "
                                      "allow_mixup=True and construct the training step with targets of that capacity")
        if h["copy_paste"] > 0:
            raise NotImplementedError("MosaicAugment: copy_paste > 0 is not implemented on the device path")
        if h["perspective"] != 0:
            raise NotImplementedError("MosaicAugment: perspective != 0 (cv2.warpPerspective) is not implemented on the device path")
        if bank.img_size % 16:
            raise ValueError(f"MosaicAugment: img_size {bank.img_size} must be a multiple of 16")
        self.bank, self.hyp, self.batch_size, self.seed = bank, h, int(batch_size), int(seed)
        self.img_size = bank.img_size
        self.max_labels = max(bank.max_labels, 1)
        self.mixup = h["mixup"] > 0                                    # the mix entry points and the doubled capacity, for every batch
        self.capacity = self.batch_size * (8 if self.mixup else 4) * self.max_labels
        self.rng = np.random.default_rng(self.seed)

    # ---- host: draws -> parameter table ------------------------------------------------------------------------------------------
    def draw(self, index):
        """the random draws of __getitem__(index) with the reference's distributions"""
        h, s, rng, n = self.hyp, self.img_size, self.rng, len(self.bank)
        mosaic = rng.random() < h["mosaic"]
        xc = yc = 0
        if mosaic:
            yc, xc = (int(rng.uniform(s / 2, 2 * s - s / 2)) for _ in range(2))     # mosaic_border = [-s // 2, -s // 2]
            sources = [int(index)] + [int(i) for i in rng.integers(0, n, 3)]        # random.choices(self.indices, k=3)
            rng.shuffle(sources)
        else:
            sources = [int(index)]
        deg = rng.uniform(-h["degrees"], h["degrees"])
        sc = rng.uniform(1 - h["scale"], 1 + h["scale"])
        shear = (rng.uniform(-h["shear"], h["shear"]), rng.uniform(-h["shear"], h["shear"]))
        t = h["translate"]
        trans = (rng.uniform(0.5 - t, 0.5 + t), rng.uniform(0.5 - t, 0.5 + t))
        gains = None
        if h["hsv_h"] or h["hsv_s"] or h["hsv_v"]:
            gains = rng.uniform(-1, 1, 3) * [h["hsv_h"], h["hsv_s"], h["hsv_v"]] + 1
        flipud = rng.random() < h["flipud"]
        fliplr = rng.random() < h["fliplr"]
        partner = ratio = None
        if self.mixup and mosaic and rng.random() < h["mixup"]:      # mixup(img, labels, *self.load_mosaic(random.choice(self.indices)))
            src2 = [int(i) for i in rng.integers(0, n, 4)]          # random.choice(self.indices) and load_mosaic's three more
            rng.shuffle(src2)
            yc2, xc2 = (int(rng.uniform(s / 2, 2 * s - s / 2)) for _ in range(2))
            deg2 = rng.uniform(-h["degrees"], h["degrees"])
            sc2 = rng.uniform(1 - h["scale"], 1 + h["scale"])
            shear2 = (rng.uniform(-h["shear"], h["shear"]), rng.uniform(-h["shear"], h["shear"]))
            trans2 = (rng.uniform(0.5 - t, 0.5 + t), rng.uniform(0.5 - t, 0.5 + t))
            partner = Draw(True, src2, xc2, yc2, deg2, sc2, shear2, trans2)
            ratio = rng.beta(32.0, 32.0)
        return Draw(mosaic, sources, xc, yc, deg, sc, shear, trans, gains, flipud, fliplr, partner, ratio)

    def plan(self, draws):
        """Plan of explicit draws (sample() draws them; tests pass their own)"""
        n = len(draws)
        table = (capi.LyMosaicImage * n)()
        luts = np.zeros((n, 3, 256), dtype=np.uint8)
        mats = [self._entry(table[b], d) for b, d in enumerate(draws)]
        with_hsv = [b for b, d in enumerate(draws) if d.gains is not None]
        if with_hsv:
            r = np.stack([draws[b].gains for b in with_hsv])[:, :, None]       # hsv_luts, all images at once
            x = np.arange(0, 256, dtype=np.float64)
            luts[with_hsv] = np.stack([((x * r[:, 0]) % 180).astype(np.uint8), np.clip(x * r[:, 1], 0, 255).astype(np.uint8),
                                       np.clip(x * r[:, 2], 0, 255).astype(np.uint8)], 1)
        mixed = [b for b, d in enumerate(draws) if d.partner is not None]
        if not mixed:
            return Plan(table, luts, list(draws), mats)
        if not self.mixup:
            raise ValueError("MosaicAugment: a draw has a mixup partner, but this augmenter was constructed with hyp['mixup'] == 0")
        partner_table = (capi.LyMosaicImage * len(mixed))()
        mix = (capi.LyMixup * n)(*[capi.LyMixup(-1, 0, 0.0) for _ in range(n)])
        for k, b in enumerate(mixed):
            self._entry(partner_table[k], draws[b].partner)
            mix[b] = capi.LyMixup(n + k, 0, draws[b].ratio)
        return Plan(table, luts, list(draws), mats, partner_table, mix)

    def _entry(self, e, d):
        """fill the LyMosaicImage `e` from the draw `d` (lut unset) -> the forward matrix M"""
        s, bank = self.img_size, self.bank
        for t in range(4):
            e.tile[t].src = -1
        if d.mosaic:
            if len(d.sources) != 4:
                raise ValueError("a mosaic draw needs four sources")
            hw = [tuple(int(v) for v in bank.hw[i]) for i in d.sources]
            rects = mosaic_placement(s, d.xc, d.yc, hw)
            for t, (src, (x1a, y1a, x2a, y2a, x1b, y1b, _, _)) in enumerate(zip(d.sources, rects)):
                self._tile(e.tile[t], src, x1a, y1a, x2a, y2a, x1b, y1b, x1a - x1b, y1a - y1b)
            M = perspective_matrix(2 * s, 2 * s, s, s, d.degrees, d.scale, *d.shear, *d.translate)
        else:
            src = d.sources[0]
            hh, ww = (int(v) for v in bank.hw[src])
            left, top, dw, dh = letterbox_pads(s, hh, ww)
            self._tile(e.tile[0], src, left, top, left + ww, top + hh, 0, 0, dw, dh)
            M = perspective_matrix(s, s, s, s, d.degrees, d.scale, *d.shear, *d.translate)
        inv = invert_affine(M)
        e.m[:] = [float(v) for v in M[:2].reshape(-1)]
        e.minv[:] = [float(v) for v in inv.reshape(-1).astype(np.float32)]
        e.scale = d.scale
        e.mosaic, e.flipud, e.fliplr = int(d.mosaic), int(d.flipud), int(d.fliplr)
        return M

    def _tile(self, tl, src, x1a, y1a, x2a, y2a, x1b, y1b, padw, padh):
        bank = self.bank
        tl.src, tl.off = int(src), int(bank.off[src])
        tl.h, tl.w = (int(v) for v in bank.hw[src])
        tl.x1a, tl.y1a, tl.x2a, tl.y2a, tl.x1b, tl.y1b = int(x1a), int(y1a), int(x2a), int(y2a), int(x1b), int(y1b)
        tl.lab, tl.nlab = int(bank.lab_off[src]), int(bank.nlab[src])
        tl.padw, tl.padh = float(padw), float(padh)

    def sample(self, indices):
        """draws for a batch of bank indices -> Plan"""
        return self.plan([self.draw(i) for i in indices])

    # ---- device -------------------------------------------------------------------------------------------------------------------
    def __call__(self, indices=None, out=None, plan=None):
        """-> (imgs uint8 [n, 3, s, s], targets float32 [capacity, 6]) on the current stream, no host sync.  out = (imgs, targets): write into
        these (a GraphedTrainStep's captured buffers: step.imgs, step.targets); plan: a Plan from sample() / plan() instead of `indices`."""
        if plan is None:
            plan = self.sample(indices)
        n, s, bank = plan.n, self.img_size, self.bank
        if n > self.batch_size:
            raise ValueError(f"MosaicAugment: {n} images in a batch of {self.batch_size}")
        dev = bank.device
        if out is None:
            imgs = torch.empty((n, 3, s, s), dtype=torch.uint8, device=dev)
            targets = torch.empty((self.capacity, 6), dtype=torch.float32, device=dev)
        else:
            imgs, targets = out
            if imgs.dtype != torch.uint8 or tuple(imgs.shape) != (n, 3, s, s) or not imgs.is_contiguous() or imgs.device != dev:
                raise ValueError(f"MosaicAugment: out[0] must be a contiguous uint8 [{n}, 3, {s}, {s}] tensor on {dev} (got {imgs.dtype} "
                                 f"{tuple(imgs.shape)} on {imgs.device})")
            if targets.dtype != torch.float32 or tuple(targets.shape) != (self.capacity, 6) or not targets.is_contiguous() or targets.device != dev:
                raise ValueError(f"MosaicAugment: out[1] must be a contiguous float32 [{self.capacity}, 6] tensor on {dev} (got {targets.dtype} "
                                 f"{tuple(targets.shape)}): construct the step with targets of the augmenter's capacity")
        self.launch(self.upload(plan), n, imgs, targets, k=plan.k)
        return imgs, targets

    def upload(self, plan):
        """the plan's table (+ with mixup the partner entries behind it and the LyMixup table; + LUTs) on the device: one non-blocking copy
        from a fresh pinned block on the current stream -> uint8 tensor [table | partner_table | mix | luts]"""
        dev = self.bank.device
        n = plan.n
        tb = ctypes.sizeof(plan.table)
        pb = ctypes.sizeof(plan.partner_table) if plan.k else 0
        mb = ctypes.sizeof(plan.mix) if self.mixup else 0
        nbytes = tb + pb + mb + plan.luts.size
        table_dev = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)     # a fresh pinned block: the host allocator keeps it until the copy ran
        hv = host.numpy()
        arr = (capi.LyMosaicImage * n).from_buffer(hv)
        ctypes.memmove(arr, plan.table, tb)
        if pb:
            ctypes.memmove(hv.ctypes.data + tb, plan.partner_table, pb)
        if mb:
            ctypes.memmove(hv.ctypes.data + tb + pb, plan.mix, mb)
        tb += pb + mb
        hv[tb:] = plan.luts.reshape(-1)
        base = table_dev.data_ptr() + tb
        for b, d in enumerate(plan.draws):
            arr[b].lut = base + b * 768 if d.gains is not None else None
        del arr
        table_dev.copy_(host, non_blocking=True)
        return table_dev

    def launch(self, table_dev, n, imgs, targets, which=3, k=0):
        """ly_mosaic_img (which & 1) and ly_mosaic_labels (which & 2) over an uploaded table, on the current stream; an augmenter with mixup
        launches ly_mosaic_mix_img / ly_mosaic_mix_labels instead, for every batch (k: the plan's partner entries, plan.k)"""
        bank, lib, st = self.bank, capi.lib(), capi.stream_ptr()
        tp = ctypes.c_void_p(table_dev.data_ptr())
        labels = capi.ptr(bank.labels) if bank.labels.numel() else ctypes.c_void_p(0)
        if self.mixup:
            mp = ctypes.c_void_p(table_dev.data_ptr() + (n + k) * ctypes.sizeof(capi.LyMosaicImage))
            if which & 1:
                capi.check(lib.ly_mosaic_mix_img(capi.ptr(bank.data), tp, mp, n, n + k, self.img_size, capi.ptr(imgs), st), "ly_mosaic_mix_img")
            if which & 2:
                capi.check(lib.ly_mosaic_mix_labels(labels, tp, mp, n, n + k, self.img_size, bank.max_labels, capi.ptr(targets), self.capacity,
                                                    st), "ly_mosaic_mix_labels")
            return
        if which & 1:
            capi.check(lib.ly_mosaic_img(capi.ptr(bank.data), tp, n, self.img_size, capi.ptr(imgs), st), "ly_mosaic_img")
        if which & 2:
            capi.check(lib.ly_mosaic_labels(labels, tp, n, self.img_size, bank.max_labels, capi.ptr(targets), self.capacity, st),
                       "ly_mosaic_labels")

    # ---- index batches ------------------------------------------------------------------------------------------------------------
    def batches(self, epoch, rank=0, world_size=1):
        """the index batches of one epoch: a permutation seeded by seed + epoch, sharded as DistributedSampler(shuffle=True, seed=seed)
        after set_epoch(epoch) shards it (padded to a multiple of world_size by repeating its head, then every world_size-th index from
        rank), cut into batches of batch_size with drop_last=True (the graphed step has one shape)"""
        n = len(self.bank)
        g = torch.Generator()
        g.manual_seed(self.seed + int(epoch))
        idx = torch.randperm(n, generator=g).tolist()
        total = math.ceil(n / world_size) * world_size
        pad = total - n
        if pad:
            idx += (idx * math.ceil(pad / len(idx)))[:pad]
        idx = idx[rank:total:world_size]
        bs = self.batch_size
        for i in range(0, len(idx) - bs + 1, bs):
            yield idx[i:i + bs]
