"""Feature extractors with the interface of pyvisim/features/_features.py: `extractor(image) -> (n, output_dim)`
float descriptors plus `.output_dim`.

  SIFT / RootSIFT   OpenCV's detector is third-party CPU code and out of scope; it
                    is imported lazily, so the classes exist without cv2 and fail only when called.  RootSIFT
                    additionally exposes `raw(image)` so that the encoders can hand the *raw* uint8 SIFT rows
                    to the GPU and fuse the RootSIFT tail (d /= sum+1e-7; sqrt, _features.py:112-114) there.
  _DeviceSIFT       private base of the two GPU extractors below: the context, the intake of a batch (checks, pixel kind, upload),
                    buffer ownership and the single-image calls (`raw`, `descriptors`, `__call__`).  A subclass adds its parameters
                    and `device_descriptors(images, ctx)`, which leaves a whole batch's rows on the device for the encoders.
                    They mirror SIFT / RootSIFT: integer valued float32 rows 0..255; `raw(image)` + `fused_rootsift`.
  DenseSIFT /       SIFT descriptors on a regular grid at fixed bin sizes, computed from the pixels by the HIP kernel of
  DenseRootSIFT     csrc/dsift.hip: no detector, no OpenCV.  The row count is known before the call.
  KeypointSIFT /    keypoint SIFT computed from the pixels by csrc/sift.hip: Lowe's scale-space detector,
  KeypointRootSIFT  orientation assignment and rotated descriptors with OpenCV's parameter names and defaults, without OpenCV (and
                    not a bit-for-bit clone of it).  The row count depends on the images: a capacity guess and one retry.
  _hellinger        the RootSIFT tail of all three *RootSIFT classes (the kernels' row tail is csrc/sift_common.hpp).
  Lambda            any user function (the descriptor-level door used by tests and synthetic benchmarks).
  DeepConvFeature   conv feature maps of a torch model on PyTorch-ROCm (torch is plumbing here).  torchvision
                    is absent offline, so the default network is an own VGG16 `features` stack with RANDOM
                    weights unless a model is passed (the reference's default argument downloads weights at
                    import, _features.py:179 -- never attempted).
"""
from __future__ import annotations

from contextlib import contextmanager
from functools import wraps
from typing import Callable

import numpy as np

from .._base_classes import FeatureExtractorBase


def _check_output_shape(func) -> Callable:
    """Extractor outputs must be a 2-D ndarray (n, output_dim); None becomes an empty (0, D) array
    (same contract as the reference wrapper, _features.py:24-51)."""

    @wraps(func)
    def wrapper(self, *args, **kwargs) -> np.ndarray:
        image = args[0]
        if type(image).__module__.startswith("torch"):
            raise TypeError("Torch images are not supported yet. Please convert to NumPy.")
        feats = func(self, *args, **kwargs)
        if feats is None:
            return np.zeros((0, self.output_dim), dtype=np.float32)
        if not isinstance(feats, np.ndarray):
            raise ValueError(f"Expected output to be a NumPy array, got {type(feats)} instead.")
        if feats.ndim != 2:
            raise ValueError(f"Feature extractor output must be 2D. Got shape {feats.shape}.")
        if feats.shape[1] != self.output_dim:
            raise ValueError(f"Expected feat_vecs.shape[1] == {self.output_dim}, but got {feats.shape[1]}.")
        return feats

    return wrapper


def _hellinger(descriptors):
    """RootSIFT's tail on float rows (n, 128), in place where it can: d /= sum + 1e-7; sqrt.  None and empty pass through."""
    if descriptors is not None and descriptors.shape[0]:
        descriptors /= descriptors.sum(axis=1, keepdims=True) + 1e-7
        descriptors = np.sqrt(descriptors)
    return descriptors


def _cv2():
    try:
        import cv2
    except ImportError as e:  # pragma: no cover - cv2 is absent in the build image
        raise ImportError("OpenCV (cv2) is required for SIFT keypoint detection; pass descriptors through "
                          "`Lambda` or `encode_descriptors` instead") from e
    return cv2


class SIFT(FeatureExtractorBase):
    """Lowe's SIFT descriptors (n, 128), integer valued float32, via OpenCV."""

    def __init__(self):
        super().__init__()
        self._output_dim = 128

    @property
    def output_dim(self) -> int:
        return self._output_dim

    @_check_output_shape
    def __call__(self, image: np.ndarray, /) -> np.ndarray:
        super().__call__(image)
        _, descriptors = _cv2().SIFT.create().detectAndCompute(image, None)
        return descriptors

    def __repr__(self):
        return f"SIFT(output_dim={self.output_dim})"


class RootSIFT(FeatureExtractorBase):
    """SIFT + Hellinger normalisation (Arandjelovic & Zisserman 2012)."""
    fused_rootsift = True   # encoders may call raw() and let the GPU apply the RootSIFT tail

    def __init__(self):
        super().__init__()
        self._output_dim = 128

    @property
    def output_dim(self) -> int:
        return self._output_dim

    def raw(self, image: np.ndarray) -> np.ndarray:
        """Raw OpenCV SIFT rows (n, 128) float32 with integer values 0..255 (empty -> (0, 128))."""
        FeatureExtractorBase.__call__(self, image)
        _, descriptors = _cv2().SIFT.create().detectAndCompute(image, None)
        return np.zeros((0, 128), np.float32) if descriptors is None else descriptors

    @_check_output_shape
    def __call__(self, image: np.ndarray, /) -> np.ndarray:
        super().__call__(image)
        _, descriptors = _cv2().SIFT.create().detectAndCompute(image, None)
        return _hellinger(descriptors)

    def __repr__(self):
        return f"RootSIFT(output_dim={self.output_dim})"


class _DeviceSIFT(FeatureExtractorBase):
    """What DenseSIFT and KeypointSIFT share: the context, the intake of a batch of images up to the pixel upload, and the
    single-image calls on top of the subclass's `device_descriptors`."""

    def __init__(self, ctx):
        super().__init__()
        self._ctx = ctx
        self._output_dim = 128

    @property
    def output_dim(self) -> int:
        return self._output_dim

    @property
    def context(self):
        if self._ctx is None:
            from ..engine import default_context
            self._ctx = default_context()
        return self._ctx

    @staticmethod
    def _pixel_kind(images):
        """uint8 images are uploaded as they are, everything else as float32; one kind per batch."""
        from .._ffi import PIX_F32_GRAY, PIX_F32_RGB, PIX_U8_GRAY, PIX_U8_RGB
        gray = {im.ndim == 2 for im in images}
        if len(gray) != 1:
            raise ValueError("a batch must be all gray (H, W) or all colour (H, W, 3) images")
        u8 = all(im.dtype == np.uint8 for im in images)
        if gray.pop():
            return (PIX_U8_GRAY if u8 else PIX_F32_GRAY), (np.uint8 if u8 else np.float32)
        return (PIX_U8_RGB if u8 else PIX_F32_RGB), (np.uint8 if u8 else np.float32)

    def _intake(self, images, ctx, out_kind, _validated):
        """Check a batch and upload its pixels -> (ctx, pixel DeviceBuffer, pixel kind, hw (B, 2) int32, pixels in all, descriptor
        kind, out_kind).  The caller frees the pixel buffer once its readers are done."""
        from .._ffi import DSIFT_F32_QUANT, DSIFT_U8
        from .._utils import is_numpy_image
        from ..engine import DESC_F32, DESC_U8_ROOTSIFT
        images = [images] if isinstance(images, np.ndarray) and images.ndim in (2, 3) and not (
            images.ndim == 3 and images.shape[2] != 3) else list(images)
        if not images:
            raise ValueError("need at least one image")
        for pos, im in enumerate(() if _validated else images):
            if type(im).__module__.startswith("torch"):
                raise TypeError("Torch images are not supported yet. Please convert to NumPy.")
            is_numpy_image(im, pos)
        ctx = ctx if ctx is not None else self.context          # images are refused before anything touches the device
        pix_kind, dt = self._pixel_kind(images)
        fused = getattr(self, "fused_rootsift", False)
        kind = DESC_U8_ROOTSIFT if fused else DESC_F32
        if out_kind is None:            # what the encoders read: uint8 rows, or the same integers as float32 for plain SIFT
            out_kind = DSIFT_U8 if fused else DSIFT_F32_QUANT
        hw = np.array([im.shape[:2] for im in images], dtype=np.int32).reshape(-1, 2)
        n_pix = int((hw[:, 0].astype(np.int64) * hw[:, 1]).sum())
        flat = np.concatenate([np.ascontiguousarray(im, dtype=dt).reshape(-1) for im in images])
        return ctx, ctx.buffer(flat.nbytes).upload(flat), pix_kind, hw, n_pix, kind, out_kind

    @staticmethod
    @contextmanager
    def _owning(pix, outputs):
        """The pixel buffer is freed on the way out, whatever happened; the buffers in the list `outputs` only if the block
        failed (otherwise they are the caller's)."""
        try:
            yield
        except Exception:
            for b in outputs:
                b.free()
            raise
        finally:
            pix.free()

    def _rows(self, image, out_kind, dtype, validated=False, **more):
        got = self.device_descriptors([image], None, out_kind, _validated=validated, **more)
        rows, offs, total, frames = got[0], got[1], got[3], got[6:]
        try:
            out = rows.download((total, 128), dtype)
            return (frames[0].download((total, 6), np.float32), out) if frames else out
        finally:
            for b in (rows, offs) + frames:
                b.free()

    def raw(self, image: np.ndarray) -> np.ndarray:
        """The uint8 rows (n, 128) as the kernel writes them."""
        from .._ffi import DSIFT_U8
        return self._rows(image, DSIFT_U8, np.uint8)          # device_descriptors validates the image

    def descriptors(self, image: np.ndarray, normalised: bool = True) -> np.ndarray:
        """float32 rows before quantisation: the normalised v (default) or the raw accumulators."""
        from .._ffi import DSIFT_F32, DSIFT_F32_RAW
        return self._rows(image, DSIFT_F32 if normalised else DSIFT_F32_RAW, np.float32)

    @_check_output_shape
    def __call__(self, image: np.ndarray, /) -> np.ndarray:
        from .._ffi import DSIFT_U8
        super().__call__(image)
        return self._rows(image, DSIFT_U8, np.uint8, validated=True).astype(np.float32)


class DenseSIFT(_DeviceSIFT):
    """Dense SIFT (n, 128): descriptors at every `step` pixels for each bin size in `sizes` (pixels per spatial bin), integer
    valued float32 rows on OpenCV's 0..255 scale like `SIFT`.  The definition is DESIGN.md section 9; the work is done by
    pvs_dsift_dev on the GPU.  Rows are ordered by (size, y, x); `frames(h, w)` gives their (x, y, size)."""

    def __init__(self, step: int = 16, sizes=(4, 8), contrast_threshold: float = 0.0, ctx=None):
        super().__init__(ctx)
        if isinstance(step, bool) or int(step) != step or step < 1:
            raise ValueError(f"step must be a positive integer, got {step!r}")
        sizes = tuple(sizes)
        if not sizes:
            raise ValueError("sizes must hold at least one bin size")
        for s in sizes:
            if isinstance(s, bool) or int(s) != s or s < 1:
                raise ValueError(f"bin sizes must be positive integers, got {s!r}")
        if not contrast_threshold >= 0:
            raise ValueError(f"contrast_threshold must be >= 0, got {contrast_threshold!r}")
        self.step = int(step)
        self.sizes = tuple(int(s) for s in sizes)
        self.contrast_threshold = float(contrast_threshold)

    def count(self, h: int, w: int) -> int:
        """Descriptor rows of an h x w image."""
        from ..engine import dsift_count
        return dsift_count(h, w, self.step, self.sizes)

    def frames(self, h: int, w: int) -> np.ndarray:
        """(n, 3) float32: x centre, y centre and bin size of every row of an h x w image."""
        from ..engine import dsift_frames
        return dsift_frames(h, w, self.step, self.sizes)

    def device_descriptors(self, images, ctx=None, out_kind=None, _validated=False):
        """Descriptors of a batch of images (mixed sizes allowed), left on the device:
        -> (rows DeviceBuffer, offsets DeviceBuffer (int64, B+1), n_images, total rows, descriptor kind, host offsets).
        The rows are uint8 (kind DESC_U8_ROOTSIFT for DenseRootSIFT: the encoders fuse the RootSIFT tail into their load) or,
        for DenseSIFT, the same integers as float32 (kind DESC_F32); `out_kind` (a pvs_dsift_out value) overrides the row format.
        All images of one call must be gray (H, W) or all colour (H, W, 3): the kernel reads one pixel format per launch
        (the encoders cut their input into such runs).  The caller owns both buffers (`.free()`)."""
        from .._ffi import DSIFT_U8
        ctx, pix, pix_kind, hw, _, kind, out_kind = self._intake(images, ctx, out_kind, _validated)
        held = []
        with self._owning(pix, held):
            h_off = np.zeros(len(hw) + 1, dtype=np.int64)
            np.cumsum([self.count(h, w) for h, w in hw], out=h_off[1:])
            total = int(h_off[-1])
            rows = ctx.buffer(max(total, 1) * 128 * (1 if out_kind == DSIFT_U8 else 4))
            held.append(rows)
            offs = ctx.buffer(h_off.nbytes)
            held.append(offs)
            ctx.dsift_dev(pix.ptr, pix_kind, hw, None, self.step, self.sizes, self.contrast_threshold, out_kind, rows.ptr,
                          total, offs.ptr)
            ctx.sync()                      # the pixel block goes back to the context's cache: its readers must be done
        return rows, offs, len(hw), total, kind, h_off

    def __repr__(self):
        return (f"{type(self).__name__}(step={self.step}, sizes={self.sizes}, contrast_threshold={self.contrast_threshold}, "
                f"output_dim={self.output_dim})")


class DenseRootSIFT(DenseSIFT):
    """Dense SIFT + Hellinger normalisation (d /= sum + 1e-7; sqrt), the dense counterpart of `RootSIFT`.  The encoders take
    its uint8 rows on the device and fuse the RootSIFT tail into their load (kind DESC_U8_ROOTSIFT)."""
    fused_rootsift = True

    def __call__(self, image: np.ndarray, /) -> np.ndarray:
        return _hellinger(super().__call__(image))


class KeypointSIFT(_DeviceSIFT):
    """Keypoint SIFT (n, 128) on the GPU: Lowe's scale-space detector (Gaussian pyramid, DoG extrema, sub-pixel refinement,
    contrast and edge tests), orientation assignment and rotated 4 x 4 x 8 descriptors, integer valued float32 rows on OpenCV's
    0..255 scale like `SIFT`.  OpenCV's parameter names and defaults, but NOT a bit-for-bit clone of cv2.SIFT: the definition is
    DESIGN.md section 10 and the work is done by pvs_sift_dev.  Rows are ordered by (octave, layer, y, x of the extremum,
    orientation); `keypoints(image)` gives their frames (x, y, size, angle, response, octave)."""

    def __init__(self, nfeatures: int = 0, n_octave_layers: int = 3, contrast_threshold: float = 0.04, edge_threshold: float = 10,
                 sigma: float = 1.6, upsample: bool = True, ctx=None):
        super().__init__(ctx)
        if isinstance(nfeatures, bool) or int(nfeatures) != nfeatures or nfeatures < 0:
            raise ValueError(f"nfeatures must be a non-negative integer, got {nfeatures!r}")
        if isinstance(n_octave_layers, bool) or int(n_octave_layers) != n_octave_layers or n_octave_layers < 1:
            raise ValueError(f"n_octave_layers must be a positive integer, got {n_octave_layers!r}")
        if not contrast_threshold >= 0:
            raise ValueError(f"contrast_threshold must be >= 0, got {contrast_threshold!r}")
        if not edge_threshold > 0:
            raise ValueError(f"edge_threshold must be > 0, got {edge_threshold!r}")
        if not (sigma > 0 and np.isfinite(sigma)):
            raise ValueError(f"sigma must be a positive number, got {sigma!r}")
        if not isinstance(upsample, (bool, np.bool_)):
            raise ValueError(f"upsample must be a bool, got {upsample!r}")
        self.nfeatures = int(nfeatures)
        self.n_octave_layers = int(n_octave_layers)
        self.contrast_threshold = float(contrast_threshold)
        self.edge_threshold = float(edge_threshold)
        self.sigma = float(sigma)
        self.upsample = bool(upsample)
        self._rows_per_pixel = 1.0 / 64.0        # capacity guess of the first call; grows with what the images gave

    def device_descriptors(self, images, ctx=None, out_kind=None, _validated=False, frames=False):
        """Descriptors of a batch of images (mixed sizes allowed), left on the device:
        -> (rows DeviceBuffer, offsets DeviceBuffer (int64, B+1), n_images, total rows, descriptor kind, host offsets), the tuple
        of `DenseSIFT.device_descriptors`; with frames=True a seventh item, the DeviceBuffer of the (total, 6) float32 frames.
        The row count depends on the images: the first call guesses a capacity and, when the rows do not fit, one retry with
        the exact total follows (pvs_sift_dev reports it).  The caller owns the buffers (`.free()`)."""
        from .._errors import CapacityError
        from .._ffi import DSIFT_U8
        ctx, pix, pix_kind, hw, n_pix, kind, out_kind = self._intake(images, ctx, out_kind, _validated)
        width = 128 * (1 if out_kind == DSIFT_U8 else 4)
        capacity = max(256, int(n_pix * self._rows_per_pixel))
        if self.nfeatures:
            capacity = min(capacity, self.nfeatures * len(hw))
        held = []
        with self._owning(pix, held):       # pvs_sift_dev waits for the stream: nothing reads the pixels after it
            offs = ctx.buffer((len(hw) + 1) * 8)
            held.append(offs)
            for attempt in (0, 1):
                rows = ctx.buffer(max(capacity, 1) * width)
                held.append(rows)
                frm = ctx.buffer(max(capacity, 1) * 24) if frames else None
                if frames:
                    held.append(frm)
                try:
                    total = ctx.sift_dev(pix.ptr, pix_kind, hw, None, self.nfeatures, self.n_octave_layers, self.contrast_threshold,
                                         self.edge_threshold, self.sigma, self.upsample, out_kind, rows.ptr, capacity,
                                         None if frm is None else frm.ptr, offs.ptr)
                    break
                except CapacityError as e:
                    if attempt:
                        raise
                    while len(held) > 1:    # everything but the offsets: one retry with the exact total
                        held.pop().free()
                    capacity = int(e.args[1])
            h_off = offs.download((len(hw) + 1,), np.int64)
        self._rows_per_pixel = max(self._rows_per_pixel, 1.25 * total / max(n_pix, 1))
        out = (rows, offs, len(hw), total, kind, h_off)
        return out + (frm,) if frames else out

    def detect_and_compute(self, image: np.ndarray):
        """-> (frames (n, 6) float32: x, y, size, angle, response, octave; uint8 rows (n, 128))"""
        from .._ffi import DSIFT_U8
        return self._rows(image, DSIFT_U8, np.uint8, frames=True)

    def keypoints(self, image: np.ndarray) -> np.ndarray:
        """(n, 6) float32 frames in input-image coordinates: x, y, size (diameter), angle (degrees, from +x towards +y),
        response (|interpolated DoG|), octave (0 = the first octave, which is the enlarged image when `upsample`)."""
        return self.detect_and_compute(image)[0]

    def __repr__(self):
        return (f"{type(self).__name__}(nfeatures={self.nfeatures}, n_octave_layers={self.n_octave_layers}, "
                f"contrast_threshold={self.contrast_threshold}, edge_threshold={self.edge_threshold}, sigma={self.sigma}, "
                f"upsample={self.upsample}, output_dim={self.output_dim})")


class KeypointRootSIFT(KeypointSIFT):
    """Keypoint SIFT + Hellinger normalisation (d /= sum + 1e-7; sqrt): the OpenCV-free counterpart of `RootSIFT`, the extractor
    the shipped vocabularies were trained with up to the differences between this definition and cv2.SIFT.
    The encoders take its uint8 rows on the device and fuse the RootSIFT tail into their load (kind DESC_U8_ROOTSIFT)."""
    fused_rootsift = True

    def __call__(self, image: np.ndarray, /) -> np.ndarray:
        return _hellinger(super().__call__(image))


class Lambda(FeatureExtractorBase):
    """Wraps any `func(image) -> (n, output_dim)`."""

    def __init__(self, func: Callable, output_dim: int):
        super().__init__()
        if not callable(func):
            raise ValueError(f"Argument func must be a callable object, got {type(func)} instead")
        self._output_dim = output_dim
        self.func = func

    @property
    def output_dim(self) -> int:
        return self._output_dim

    @_check_output_shape
    def __call__(self, image: np.ndarray, /) -> np.ndarray:
        super().__call__(image)
        return self.func(image)


def _vgg16_features():
    """VGG16 `features` stack (13 conv + 5 max-pool), same module indices as torchvision's (conv at
    0,2,5,7,10,12,14,17,19,21,24,26,28) so that layer_index=-1 hooks `features.28`."""
    import torch.nn as nn
    cfg = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]
    layers, c_in = [], 3
    for v in cfg:
        if v == "M":
            layers.append(nn.MaxPool2d(2, 2))
        else:
            layers += [nn.Conv2d(c_in, v, 3, padding=1), nn.ReLU(inplace=True)]
            c_in = v

    class VGG16Features(nn.Module):
        def __init__(self):
            super().__init__()
            self.features = nn.Sequential(*layers)

        def forward(self, x):
            return self.features(x)

    return VGG16Features()


class DeepConvFeature(FeatureExtractorBase):
    """Feature map of one conv layer, flattened to (H*W, C [+2]) descriptors (reference: _features.py:151-306).

    The hook sits on the Conv2d itself, i.e. PRE-ReLU (:254-261); the default transform is ToTensor +
    Resize(224, 224) with NO mean/std normalisation (:192-194); `spatial_encoding` appends (x/W, y/H).
    `batch(images)` runs many images in one forward and keeps the features on the device."""

    def __init__(self, model=None, target_submodule: str = None, layer_index: int = -1,
                 spatial_encoding: bool = True, device=None, transform=None):
        import torch
        super().__init__()
        if model is None:
            model = _vgg16_features()
        if not isinstance(model, torch.nn.Module):
            raise TypeError(f"Currently, only torch.nn.Module is supported. Got {type(model)} instead.")
        self._model = model
        self.layer_index = layer_index
        self.spatial_encoding = spatial_encoding
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda" if torch.cuda.is_available() else "cpu")
        self.transform = transform
        if target_submodule is not None and not hasattr(model, target_submodule):
            raise AttributeError(f"Model {model._get_name()} has no submodule named {target_submodule}.")
        self._modules = model if target_submodule is None else getattr(model, target_submodule)
        self._conv_layers = self.list_conv_layers()
        if not self._conv_layers:
            raise ValueError(f"No convolutional layers found in model {model._get_name()}.")
        try:
            _, self.selected_layer_name, self.selected_layer_module = self._conv_layers[layer_index]
        except IndexError:
            raise IndexError(f"Model {model._get_name()} has only {len(self._conv_layers)} convolutional layers. "
                             f"Got layer_index={layer_index}.")
        c = self.selected_layer_module.out_channels
        self._output_dim = c + 2 if spatial_encoding else c
        self.buffer = None
        self.hook = self.selected_layer_module.register_forward_hook(self._hook_fn)
        self._model.eval().to(self.device)

    def _hook_fn(self, module, inputs, output):
        self.buffer = output.detach()

    @property
    def output_dim(self) -> int:
        return self._output_dim

    @property
    def model(self):
        return self._model

    def list_conv_layers(self):
        import torch
        out, idx = [], 0
        for name, module in self._modules.named_modules():
            if isinstance(module, torch.nn.Conv2d):
                out.append((idx, name, module))
                idx += 1
        return out

    def _to_tensor(self, image: np.ndarray):
        import torch
        import torch.nn.functional as F
        if self.transform is not None:
            return self.transform(image)
        t = torch.from_numpy(np.ascontiguousarray(image))
        if t.ndim == 2:
            t = t[:, :, None]
        t = t.permute(2, 0, 1)
        t = t.float().div(255) if t.dtype == torch.uint8 else t.float()
        return F.interpolate(t[None], size=(224, 224), mode="bilinear", align_corners=False, antialias=True)[0]

    def batch(self, images):
        """(B, Hf*Wf, D) float32 torch tensor on self.device for a list of images."""
        import torch
        x = torch.stack([self._to_tensor(im) for im in images]).to(self.device)
        with torch.no_grad():
            self._model(x)
        if self.buffer is None:
            raise RuntimeError("Forward hook did not capture any features.")
        fm = self.buffer                                  # (B, C, Hf, Wf)
        b, c, hf, wf = fm.shape
        feats = fm.reshape(b, c, hf * wf).transpose(1, 2)  # (B, Hf*Wf, C), row-major over (y, x)
        if self.spatial_encoding:
            ys, xs = torch.meshgrid(torch.arange(hf, device=fm.device), torch.arange(wf, device=fm.device),
                                    indexing="ij")
            coords = torch.stack([xs.reshape(-1) / wf, ys.reshape(-1) / hf], dim=1).float()
            feats = torch.cat([feats, coords[None].expand(b, -1, -1)], dim=2)
        return feats.contiguous()

    @_check_output_shape
    def __call__(self, image: np.ndarray, /) -> np.ndarray:
        super().__call__(image)
        return self.batch([image])[0].cpu().numpy()

    def __repr__(self):
        return (f"DeepConvFeature(model={self._model._get_name()}, layer_index={self.layer_index}, "
                f"spatial_encoding={self.spatial_encoding}, device={self.device}, "
                f"selected_layer_name={self.selected_layer_name}, output_dim={self.output_dim})")
