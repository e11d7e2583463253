"""The reference's joint image/label transforms (utils/ext_transforms.py there) for BATCHES RESIDENT ON THE MI355X.

Same class names and constructor arguments as the reference, so the driver's transform block reads the same
(main_embedding.py:148-157):

    train_transform = et.ExtCompose([
        et.ExtRandomCrop(size=(768, 768)),
        et.ExtColorJitter(brightness=0.5, contrast=0.5, saturation=0.5),
        et.ExtRandomHorizontalFlip(),
        et.ExtToTensor(),
        et.ExtNormalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225]),
    ])
    images, labels = train_transform(frames_u8, labels_u8)      # [B,H,W,3] / [B,H,W] uint8 CUDA tensors

The reference runs them per sample on PIL images in 16 DataLoader workers; at several hundred images/s per GPU that
host pipeline is the bottleneck.  Here the classes are specifications: ExtCompose draws the
random parameters on the host with the `random` module in the reference's order (crop i, j -> jitter factors ->
shuffle -> flip coin; ext_transforms.py:362-365, 483-499, 229) and runs two HIP kernels (dml_aug_contrast_sum,
dml_aug_apply) that reproduce Pillow's arithmetic bit for bit.  Output: float32 NCHW images and int64 labels (the
reference casts its uint8 labels to long right after the loader, main_embedding.py:463).
There is no CPU fallback: inputs must be CUDA tensors and libdmlnet_hip.so must be present.

The scale-augmented train block and the --crop_val block (main.py / main_embedding.py get_dataset of the reference)

    [ExtRandomScale | ExtScale | ExtResize]  [ExtRandomCrop(padding, pad_if_needed) | ExtCenterCrop]  ...

run one more kernel first (dml_aug_scale_window, utils/scale_window.py): per sample the frame resized to (Hs, Ws) is a
virtual image, padding and cropping reduce to one window origin in it, and the kernel writes that uint8 window -- Pillow's
BILINEAR for the image, its NEAREST for the label, 0 outside -- which the two kernels above then take as their frame.
"""
import ctypes as C
import numbers
import random

import torch

from dmlnet import _lib
from . import scale_window

BILINEAR = 2          # PIL.Image.BILINEAR


def _check_interpolation(interpolation):
    if interpolation != BILINEAR:
        raise NotImplementedError("only interpolation=BILINEAR (2) is implemented; labels always use NEAREST")


def _target(H, W, scale):
    return int(H * scale), int(W * scale)


class ExtRandomScale(object):
    def __init__(self, scale_range, interpolation=BILINEAR):
        _check_interpolation(interpolation)
        self.scale_range = (scale_range[0], scale_range[1])
        self.interpolation = interpolation

    def get_size(self, H, W):
        """(scale, (Hs, Ws)); one random.uniform per sample (ext_transforms.py:110-111)."""
        scale = random.uniform(self.scale_range[0], self.scale_range[1])
        return scale, _target(H, W, scale)


class ExtScale(object):
    def __init__(self, scale, interpolation=BILINEAR):
        _check_interpolation(interpolation)
        self.scale = scale
        self.interpolation = interpolation

    def get_size(self, H, W):
        return self.scale, _target(H, W, self.scale)


class ExtResize(object):
    def __init__(self, size, interpolation=BILINEAR):
        _check_interpolation(interpolation)
        if isinstance(size, numbers.Integral) and not isinstance(size, bool):
            self.size = int(size)
        elif isinstance(size, (tuple, list)) and len(size) == 2:
            self.size = (int(size[0]), int(size[1]))
        else:
            raise TypeError("ExtResize: size is an int or an (h, w) pair")
        self.interpolation = interpolation

    def get_size(self, H, W):
        """torchvision 0.6.0 functional.resize: a pair is (h, w); an int is matched to the smaller edge (no-op when it
        already has that size), the other edge becomes int(size * long / short)."""
        if isinstance(self.size, tuple):
            return None, self.size
        size = self.size
        if (W <= H and W == size) or (H <= W and H == size):
            return None, (H, W)
        if W < H:
            return None, (int(size * H / W), size)
        return None, (size, int(size * W / H))


class ExtCenterCrop(object):
    def __init__(self, size):
        self.size = (int(size), int(size)) if isinstance(size, numbers.Number) else tuple(int(s) for s in size)

    def get_params(self, img_hw):
        """(i, j, th, tw) of torchvision 0.6.0 center_crop; negative when the crop is larger than the image."""
        h, w = img_hw
        th, tw = self.size
        return int(round((h - th) / 2.)), int(round((w - tw) / 2.)), th, tw


class ExtRandomCrop(object):
    def __init__(self, size, padding=0, pad_if_needed=False):
        self.size = (int(size), int(size)) if isinstance(size, numbers.Number) else tuple(int(s) for s in size)
        if not (isinstance(padding, numbers.Integral) and padding >= 0):
            raise NotImplementedError("ExtRandomCrop: padding is one non-negative int (all four borders)")
        self.padding = int(padding)
        self.pad_if_needed = bool(pad_if_needed)

    def padded(self, img_hw):
        """((h, w) after the pads, (py, px) = where the unpadded image's origin lies in the padded one), following
        ext_transforms.py:378-390: `padding`, then ALL FOUR borders by int((1 + tw - w) / 2) if the width is short, then
        the same test for the height on the already padded image."""
        h, w = img_hw
        th, tw = self.size
        py = px = 0
        if self.padding > 0:
            h, w, py, px = h + 2 * self.padding, w + 2 * self.padding, py + self.padding, px + self.padding
        if self.pad_if_needed and w < tw:
            q = int((1 + tw - w) / 2)
            h, w, py, px = h + 2 * q, w + 2 * q, py + q, px + q
        if self.pad_if_needed and h < th:
            q = int((1 + th - h) / 2)
            h, w, py, px = h + 2 * q, w + 2 * q, py + q, px + q
        return (h, w), (py, px)

    @staticmethod
    def get_params(img_hw, output_size):
        """(i, j, th, tw); draws nothing when the frame already has the crop size (ext_transforms.py:357-366)."""
        h, w = img_hw
        th, tw = output_size
        if w == tw and h == th:
            return 0, 0, h, w
        i = random.randint(0, h - th)
        j = random.randint(0, w - tw)
        return i, j, th, tw


class ExtColorJitter(object):
    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        self.brightness = self._check_input(brightness, "brightness")
        self.contrast = self._check_input(contrast, "contrast")
        self.saturation = self._check_input(saturation, "saturation")
        if hue:
            raise NotImplementedError("hue jitter is not used by the reference's drivers and not implemented")

    @staticmethod
    def _check_input(value, name):
        if isinstance(value, numbers.Number):
            if value < 0:
                raise ValueError("If {} is a single number, it must be non negative.".format(name))
            value = [max(1 - value, 0), 1 + value]
        elif isinstance(value, (tuple, list)) and len(value) == 2:
            if not 0 <= value[0] <= value[1]:
                raise ValueError("{} values should be between (0, inf)".format(name))
            value = list(value)
        else:
            raise TypeError("{} should be a single number or a list/tuple with lenght 2.".format(name))
        return None if value[0] == value[1] == 1 else value

    def get_params(self):
        """[(op code, factor), ...] in application order; draws as ext_transforms.py:483-499."""
        ops = []
        for code, rng in ((0, self.brightness), (1, self.contrast), (2, self.saturation)):
            if rng is not None:
                ops.append((code, random.uniform(rng[0], rng[1])))
        random.shuffle(ops)
        return ops


class ExtRandomHorizontalFlip(object):
    def __init__(self, p=0.5):
        self.p = p


class ExtToTensor(object):
    def __init__(self, normalize=True, target_type="uint8"):
        if not normalize:
            raise NotImplementedError("ExtToTensor(normalize=False) is not implemented")


class ExtNormalize(object):
    def __init__(self, mean, std):
        self.mean, self.std = [float(m) for m in mean], [float(s) for s in std]


class ExtCompose(object):
    """[ExtRandomScale | ExtScale | ExtResize]? [ExtRandomCrop | ExtCenterCrop]? [ExtColorJitter]? [ExtRandomHorizontalFlip]?
    ExtToTensor ExtNormalize, fused on the device.  A sequence with a scale / resize stage, a centre crop or a padding random
    crop runs dml_aug_scale_window first (`self.windowed`); any other sequence launches exactly the two kernels it always did."""

    def __init__(self, transforms, label_luts=None):
        """label_luts: optional (lut, lut_true) uint8[256] tables (datasets.Cityscapes.label_luts) -- the dataset's
        encode_target folded into the crop kernel; __call__ then returns (images, labels, labels_true) like the
        reference dataset's __getitem__ (datasets/cityscapes.py:171-197)."""
        self.transforms = list(transforms)
        self.label_luts = label_luts
        self._dev_luts = None
        order = {ExtRandomScale: 0, ExtScale: 0, ExtResize: 0, ExtRandomCrop: 1, ExtCenterCrop: 1, ExtColorJitter: 2,
                 ExtRandomHorizontalFlip: 3, ExtToTensor: 4, ExtNormalize: 5}
        pos = -1
        self.resize = self.crop = self.jitter = self.flip = self.norm = None
        seen_tensor = False
        for t in self.transforms:
            if type(t) not in order or order[type(t)] <= pos:
                raise NotImplementedError("unsupported transform sequence for the device pipeline: %r" % (t,))
            pos = order[type(t)]
            if pos == 0: self.resize = t
            elif pos == 1: self.crop = t
            elif isinstance(t, ExtColorJitter): self.jitter = t
            elif isinstance(t, ExtRandomHorizontalFlip): self.flip = t
            elif isinstance(t, ExtToTensor): seen_tensor = True
            elif isinstance(t, ExtNormalize): self.norm = t
        if not seen_tensor or self.norm is None:
            raise NotImplementedError("the device pipeline ends with ExtToTensor, ExtNormalize")
        self.windowed = (self.resize is not None or isinstance(self.crop, ExtCenterCrop)
                         or (self.crop is not None and (self.crop.padding > 0 or self.crop.pad_if_needed)))
        self.last_params = None

    def sample(self, B, H, W):
        """One dict per image, drawn in the reference's per-sample order (scale, crop i, crop j -- none when the padded size
        equals the crop size --, jitter factors, shuffle, flip coin), and the output size.  Keys: i, j (crop origin; in the
        PADDED image when the crop pads), ops, flip.  A windowed sequence (see the class) adds
          size    (Hs, Ws) of the resized frame, the virtual image
          oy, ox  origin of the output window in the virtual image (negative: the window starts in the padding)
          out     (th, tw) of the output window
        and __call__(params=...) reads only size, oy, ox, out, ops and flip of those."""
        if self.windowed:
            return self._sample_windowed(B, H, W)
        out = []
        for _ in range(B):
            if self.crop is not None:
                i, j, th, tw = ExtRandomCrop.get_params((H, W), self.crop.size)
            else:
                i, j, th, tw = 0, 0, H, W
            ops = self.jitter.get_params() if self.jitter is not None else []
            flip = self.flip is not None and random.random() < self.flip.p
            out.append({"i": i, "j": j, "ops": ops, "flip": bool(flip)})
        return out, (th, tw)

    def _sample_windowed(self, B, H, W):
        if isinstance(self.resize, ExtRandomScale) and self.crop is None and B > 1:
            raise ValueError("ExtRandomScale on a batch needs a following crop: the outputs would differ in size")
        out, size = [], None
        for _ in range(B):
            Hs, Ws = self.resize.get_size(H, W)[1] if self.resize is not None else (H, W)
            if Hs <= 0 or Ws <= 0:
                raise ValueError("the scaled frame is empty (%d x %d)" % (Hs, Ws))
            if isinstance(self.crop, ExtRandomCrop):
                hw, (py, px) = self.crop.padded((Hs, Ws))
                i, j, th, tw = ExtRandomCrop.get_params(hw, self.crop.size)
                oy, ox = i - py, j - px
            elif isinstance(self.crop, ExtCenterCrop):
                i, j, th, tw = self.crop.get_params((Hs, Ws))
                oy, ox = i, j
            else:
                i = j = oy = ox = 0
                th, tw = Hs, Ws
            ops = self.jitter.get_params() if self.jitter is not None else []
            flip = self.flip is not None and random.random() < self.flip.p
            out.append({"i": i, "j": j, "ops": ops, "flip": bool(flip), "size": (Hs, Ws), "oy": oy, "ox": ox,
                        "out": (th, tw)})
            size = (th, tw)
        return out, size

    def _window(self, lib, img, lbl, params, st):
        """dml_aug_scale_window: frames [B,H,W,3] (+ labels) -> the uint8 windows [B,th,tw,3] (+ [B,th,tw])."""
        B, H, W, _ = img.shape
        th, tw = params[0]["out"]
        if any(tuple(p["out"]) != (th, tw) for p in params):
            raise ValueError("the samples of one batch must share the output size")
        buf, band, rows = scale_window.pack([(p["size"][0], p["size"][1], p["oy"], p["ox"]) for p in params], H, W, th, tw)
        dev = torch.from_numpy(buf).to(img.device, non_blocking=False)
        wimg = torch.empty((B, th, tw, 3), dtype=torch.uint8, device=img.device)
        wlbl = torch.empty((B, th, tw), dtype=torch.uint8, device=img.device) if lbl is not None else None
        _lib.check(lib.dml_aug_scale_window(img.data_ptr(), lbl.data_ptr() if lbl is not None else None, dev.data_ptr(),
                                            dev.data_ptr(), buf.size, wimg.data_ptr(),
                                            wlbl.data_ptr() if wlbl is not None else None, B, H, W, th, tw, band, rows, st),
                   "dml_aug_scale_window")
        return wimg, wlbl

    def __call__(self, img, lbl, params=None):
        lib = _lib.load()
        if not (isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.uint8):
            raise TypeError("the device pipeline takes uint8 CUDA tensors [B,H,W,3] (there is no CPU fallback)")
        single = img.dim() == 3
        if single:
            img, lbl = img[None], (lbl[None] if lbl is not None else None)
        B, H, W, Cc = img.shape
        if Cc != 3 or not img.is_contiguous():
            raise ValueError("frames must be contiguous [B,H,W,3]")
        if lbl is not None and (lbl.dtype != torch.uint8 or tuple(lbl.shape) != (B, H, W) or not lbl.is_contiguous()
                                or lbl.device != img.device):
            raise ValueError("labels must be contiguous uint8 [B,H,W] on the frames' device")
        st = torch.cuda.current_stream(img.device).cuda_stream
        if params is None:
            params, (th, tw) = self.sample(B, H, W)
        elif len(params) != B:
            raise ValueError("one parameter dict per frame")
        elif self.windowed:
            th, tw = params[0]["out"]
        else:
            th, tw = self.crop.size if self.crop is not None else (H, W)
        self.last_params = params
        if self.windowed:
            # the window is materialised (B * th * tw * 4 bytes): the contrast pivot is the mean over the crop
            img, lbl = self._window(lib, img, lbl, params, st)
            H, W = th, tw
        arr = (_lib.AugSample * B)()
        for b, p in enumerate(params):
            a = arr[b]
            a.i, a.j = (0, 0) if self.windowed else (p["i"], p["j"])
            a.flip, a.n_ops = int(p["flip"]), len(p["ops"])
            for k, (code, f) in enumerate(p["ops"]):
                a.op[k], a.factor[k] = code, f
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        dev_params = host.to(img.device, non_blocking=False)
        lsum = torch.empty(B, dtype=torch.int32, device=img.device)
        out = torch.empty((B, 3, th, tw), dtype=torch.float32, device=img.device)
        olb = torch.empty((B, th, tw), dtype=torch.int64, device=img.device) if lbl is not None else None
        m, s = self.norm.mean, self.norm.std
        _lib.check(lib.dml_aug_contrast_sum(img.data_ptr(), dev_params.data_ptr(), lsum.data_ptr(), B, H, W, th, tw, st),
                   "dml_aug_contrast_sum")
        if self.label_luts is not None:
            if lbl is None:
                raise ValueError("label tables were given but no labels")
            if self._dev_luts is None or self._dev_luts[0].device != img.device:
                self._dev_luts = tuple(torch.as_tensor(t, dtype=torch.uint8).to(img.device).contiguous()
                                       for t in self.label_luts)
                if any(t.numel() != 256 for t in self._dev_luts):
                    raise ValueError("label tables have 256 entries")
            olt = torch.empty_like(olb)
            _lib.check(lib.dml_aug_apply_encoded(img.data_ptr(), lbl.data_ptr(), dev_params.data_ptr(), lsum.data_ptr(),
                                                 out.data_ptr(), olb.data_ptr(), B, H, W, th, tw, m[0], m[1], m[2], s[0],
                                                 s[1], s[2], self._dev_luts[0].data_ptr(), self._dev_luts[1].data_ptr(),
                                                 olt.data_ptr(), st), "dml_aug_apply_encoded")
            return (out[0], olb[0], olt[0]) if single else (out, olb, olt)
        _lib.check(lib.dml_aug_apply(img.data_ptr(), lbl.data_ptr() if lbl is not None else None, dev_params.data_ptr(),
                                     lsum.data_ptr(), out.data_ptr(), olb.data_ptr() if olb is not None else None, B, H, W,
                                     th, tw, m[0], m[1], m[2], s[0], s[1], s[2], st), "dml_aug_apply")
        if single:
            return out[0], (olb[0] if olb is not None else None)
        return out, olb
