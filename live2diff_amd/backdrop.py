"""Backdrop (csrc/backdrop.hip): what stands behind the matte.  The depth matte keeps the real frame where
it does not stylise; with a backdrop that kept part is the room blurred ("portrait mode"), a colour (for a chroma key further
down) or an image instead.  The composite ops do not change: they read the kept part through a pointer, and this module only
decides what that pointer names.

  * `blur_ref`        the arithmetic of L2D_OP_FRAME_BACKDROP_BLUR in numpy, exact integers -- the kernel's oracle, as
                      `matte.edge_ref` and `detail.gains_ref` are.  An iterated box blur of the source frame's egress bytes in
                      which every pixel carries the weight 256 - M, M the raw matte in byte levels: the subject (M = 255) counts
                      1/256 of a background pixel, so its colours do not bleed into the room around the silhouette -- exactly
                      where the matte shows the room;
  * `frame_of`        bytes -> the fp16 frame in [-1, 1] that the egress expression maps back to those bytes: the form in which
                      L2D_OP_FRAME_MATTE takes its kept part;
  * `image_ref`, `color_ref`   an image cropped to the target's aspect ratio and resampled (`resize.resize_ref`), a constant frame;
  * `check_settings`  the argument checks of `StreamAnimateDiffusionDepthWrapper.set_backdrop`;
  * `HipBackdrop`     the static blur frame, the prepared image / colour buffers and the records that go in front of the
                      composite's in its `OpList`.

  P0[c] = steady.source_bytes(source)[c];  M = rint(255 matte_ref(depth, lo, hi, 0, keep));  W0 = 256 - M  (1..256, never 0)
  per pass, n = (2r+1)^2:  D = window_sum(W);  N[c] = window_sum(W P[c]);  P[c] <- (2 N[c] + D) // (2 D);  W <- (D + n - 1) // n

The weight is the raw ramp with `keep` applied and neither feather nor edge refinement: it only has to keep the subject out of
the average; feather and edge shape the transition of the composite, which still uses them."""
import os
from typing import Tuple

import numpy as np
import torch

from . import ops
from .matte import check_settings as check_matte, matte_params, matte_ref
from .resize import check_filter, resize_ref
from .steady import source_bytes, window_sum

MAX_RADIUS = ops.BACKDROP_MAX_R
MAX_PASSES = ops.BACKDROP_MAX_PASSES


# ----------------------------------------------------------------------------- settings
def _is_color(to) -> bool:
    return (isinstance(to, (tuple, list)) and len(to) == 3
            and all(not isinstance(v, bool) and isinstance(v, (int, np.integer)) for v in to))


def check_settings(to="blur", radius=6, passes=3) -> dict:
    """the setting as {to: "blur" | "color" | "image", radius, passes, color}, or ValueError: `to` is "blur", an (r, g, b) triple of
    integers in 0..255, or an image (a uint8 [H,W,3] array, a PIL image, a path, a device tensor); `radius` no integer in 1..8,
    `passes` no integer in 1..3 (both checked whatever `to` is: they are kept for a later "blur")"""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"backdrop: radius={radius!r}: use an integer from 1 to {MAX_RADIUS}")
    if isinstance(passes, bool) or not isinstance(passes, (int, np.integer)) or not 1 <= int(passes) <= MAX_PASSES:
        raise ValueError(f"backdrop: passes={passes!r}: use an integer from 1 to {MAX_PASSES}")
    out = dict(to=None, radius=int(radius), passes=int(passes), color=None)
    if isinstance(to, str) and to == "blur":
        out["to"] = "blur"
    elif _is_color(to):
        if not all(0 <= int(v) <= 255 for v in to):
            raise ValueError(f"backdrop: to={to!r}: a colour is three integers in 0..255")
        out["to"], out["color"] = "color", tuple(int(v) for v in to)
    elif isinstance(to, (tuple, list)):
        raise ValueError(f"backdrop: to={to!r}: a colour is three integers in 0..255")
    elif isinstance(to, (str, os.PathLike)):
        if not os.path.isfile(to):
            raise ValueError(f"backdrop: to={to!r}: use 'blur', an (r, g, b) triple or an image; there is no such file")
        out["to"] = "image"
    elif torch.is_tensor(to):
        ok = (to.dtype == torch.uint8 and to.ndim == 3 and to.shape[-1] == 3) or (to.dtype == torch.float16 and to.ndim == 3 and to.shape[0] == 3)
        if not ok:
            raise ValueError(f"backdrop: to: a tensor is uint8 [H,W,3] (or fp16 [3,H,W] at the stream's size), got {to.dtype} {tuple(to.shape)}")
        out["to"] = "image"
    elif hasattr(to, "convert") and hasattr(to, "size"):
        out["to"] = "image"
    elif isinstance(to, np.ndarray):
        if to.dtype != np.uint8 or to.ndim != 3 or to.shape[-1] != 3 or to.size == 0:
            raise ValueError(f"backdrop: to: an image array is uint8 [H,W,3], got {to.dtype} {to.shape}")
        out["to"] = "image"
    else:
        raise ValueError(f"backdrop: to={to!r}: use 'blur', an (r, g, b) triple of bytes or an image")
    return out


# ----------------------------------------------------------------------------- reference arithmetic (CPU, numpy)
def weight_ref(depth, lo: float, hi: float, keep: str = "near", plane=None) -> np.ndarray:
    """int64 [H,W] in 1..256: W0 = 256 - rint(255 m) with m the raw matte (ramp and `keep`, no feather, no edge), P formed as
    `matte.edge_ref` forms its own.  `plane` (fp32 [H,W]): a ready raw matte in place of the ramp (`mask_io.front_ref`), the
    host twin of L2D_BACKDROP_PLANE; `depth` is then not read."""
    m = matte_ref(depth, lo, hi, 0, keep) if plane is None else matte_ref(depth, lo, hi, 0, keep, plane=plane)
    if m.shape[0] != 1:
        raise ValueError(f"backdrop: expected one [H,W] depth plane, got {m.shape[0]}")
    M = np.rint(m[0] * np.float32(255.0)).astype(np.int64)
    assert 0 <= int(M.min()) and int(M.max()) <= 255
    return 256 - M


def blur_weighted(P0: np.ndarray, W0: np.ndarray, radius: int, passes: int) -> np.ndarray:
    """the passes of `blur_ref` on integer planes: `P0` [3,H,W] in 0..255 and `W0` [H,W] in 1..256 -> uint8 [3,H,W]"""
    r, n = int(radius), (2 * int(radius) + 1) ** 2
    P, W = np.asarray(P0).astype(np.int64), np.asarray(W0).astype(np.int64)
    if P.ndim != 3 or P.shape[0] != 3 or P.shape[1:] != W.shape:
        raise ValueError(f"backdrop: the planes are {P.shape}, the weights {W.shape}")
    assert 0 <= int(P.min()) and int(P.max()) <= 255 and 1 <= int(W.min()) and int(W.max()) <= 256
    for _ in range(int(passes)):
        D = window_sum(W, r)
        N = np.stack([window_sum(W * P[c], r) for c in range(3)])
        assert int((2 * N + D).max()) <= 2 * n * 256 * 255 + 256 * n < 1 << 32 and int(D.min()) >= n
        P = (2 * N + D) // (2 * D)                       # the weighted mean, rounded half up
        W = (D + n - 1) // n                             # the mean weight, rounded up: 1..256 again
        assert 0 <= int(P.min()) and int(P.max()) <= 255 and 1 <= int(W.min()) and int(W.max()) <= 256
    return P.astype(np.uint8)


def blur_ref(source, depth, lo: float, hi: float, keep: str = "near", radius: int = 6, passes: int = 3, plane=None) -> np.ndarray:
    """L2D_OP_FRAME_BACKDROP_BLUR on the host, in front of `frame_of`: the fp16 [3,H,W] `source` frame and its fp16 [H,W] `depth`
    plane under the matte's `lo`, `hi`, `keep` -> uint8 [3,H,W] (planar, as `steady.source_bytes`): the frame's egress bytes
    blurred `passes` times by a (2 radius + 1)^2 box in which a pixel counts 256 - M (module docstring).  `plane`: as
    `weight_ref`'s."""
    s = check_settings("blur", radius, passes)
    P0 = source_bytes(source)
    W0 = weight_ref(depth, lo, hi, keep, plane=plane)
    if W0.shape != P0.shape[1:]:
        raise ValueError(f"blur_ref: the depth plane is {W0.shape}, the source frame {P0.shape[1:]}")
    return blur_weighted(P0, W0, s["radius"], s["passes"])


_TWO_OVER_255 = np.float32(2.0 / 255.0)


def frame_of(b) -> np.ndarray:
    """uint8 [...] -> fp16 [...]: per byte fp16(fp32(b) fp32(2 / 255) - 1), two fp32 operations and one rounding to fp16.
    `frame_io.egress_ref` maps the value back to `b` for all 256 bytes, so a frame made this way and handed to
    L2D_OP_FRAME_MATTE as its kept part shows exactly these bytes where the matte is 0."""
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    if b.dtype != np.uint8:
        raise ValueError(f"frame_of: expected uint8, got {b.dtype}")
    v = b.astype(np.float32) * _TWO_OVER_255
    v = v - np.float32(1.0)
    assert v.dtype == np.float32
    return v.astype(np.float16)


def crop_box(Hs: int, Ws: int, height: int, width: int) -> Tuple[int, int, int, int]:
    """(top, left, ch, cw): the largest centred window of an Hs x Ws image that has the aspect ratio of height x width, in
    integers.  Ws height >= Hs width (the image is the wider one): ch = Hs, cw = max(1, (Hs width) // height); else cw = Ws,
    ch = max(1, (Ws height) // width); top = (Hs - ch) // 2, left = (Ws - cw) // 2."""
    Hs, Ws, height, width = int(Hs), int(Ws), int(height), int(width)
    if min(Hs, Ws, height, width) < 1:
        raise ValueError(f"backdrop: sizes must be positive, got {Hs} x {Ws} -> {height} x {width}")
    if Ws * height >= Hs * width:
        ch, cw = Hs, max(1, (Hs * width) // height)
    else:
        ch, cw = max(1, (Ws * height) // width), Ws
    return (Hs - ch) // 2, (Ws - cw) // 2, ch, cw


def _host_image(image) -> np.ndarray:
    """uint8 [H,W,3] of an array, a PIL image or a path; ValueError where a file or a PIL image cannot be decoded"""
    try:
        if isinstance(image, (str, os.PathLike)):
            from PIL import Image
            with Image.open(image) as im:
                return np.asarray(im.convert("RGB"))
        if hasattr(image, "convert") and hasattr(image, "size") and not isinstance(image, np.ndarray):
            return np.asarray(image.convert("RGB"))
    except (OSError, SyntaxError, EOFError) as e:          # (what Pillow raises on a file that is no image, or a damaged one)
        raise ValueError(f"backdrop: {image!r} cannot be read as an image: {e}") from None
    a = image.detach().cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[-1] != 3 or a.size == 0:
        raise ValueError(f"backdrop: an image is uint8 [H,W,3], got {a.dtype} {a.shape}")
    return a


def load_image(image) -> np.ndarray:
    """a path, a PIL image, a uint8 [H,W,3] array or a tensor on the host -> a contiguous uint8 [H,W,3] array of its own,
    decoded here and now: what `set_backdrop` keeps of an image, so that a file that is no image is refused when it is set"""
    a = np.array(_host_image(image), dtype=np.uint8, order="C")
    if a.ndim != 3 or a.shape[-1] != 3 or a.size == 0:
        raise ValueError(f"backdrop: an image is uint8 [H,W,3], got {a.shape}")
    return a


def check_tensor(t: torch.Tensor, height: int, width: int, out_size=None, on_device: bool = True) -> None:
    """the checks of `set_backdrop` on a tensor that is used in place: contiguous; fp16 [3,H,W] at the stream's size, or uint8
    [H,W,3] at the stream's size or at the output size set at that moment; with `on_device`, on a GPU"""
    sizes = [(int(height), int(width))] + ([(int(out_size[0]), int(out_size[1]))] if out_size is not None else [])
    ok = ((t.dtype == torch.float16 and tuple(t.shape) == (3, height, width))
          or (t.dtype == torch.uint8 and t.ndim == 3 and t.shape[-1] == 3 and tuple(t.shape[:2]) in sizes))
    if not ok or not t.is_contiguous():
        raise ValueError(f"backdrop: a tensor used in place is a contiguous fp16 [3,{height},{width}] or uint8 [h,w,3] with (h, w) in "
                         f"{sizes} (the stream's size, the output size), got {t.dtype} {tuple(t.shape)}")
    if on_device and not t.is_cuda:
        raise ValueError("backdrop: a tensor used in place lives on the stream's device; pass an array for an image on the host")


def image_ref(image, height: int, width: int, resample: str = "lanczos") -> np.ndarray:
    """a uint8 [Hs,Ws,3] array, a PIL image or a path -> uint8 [height,width,3]: the window of `crop_box` (the largest centred
    one of the target's aspect ratio), then `resize.resize_ref` to the target.  Runs on the host, once per image and size."""
    a = _host_image(image)
    top, left, ch, cw = crop_box(a.shape[0], a.shape[1], height, width)
    return resize_ref(np.ascontiguousarray(a[top:top + ch, left:left + cw]), int(height), int(width), check_filter(resample))


def color_ref(rgb, height: int, width: int) -> np.ndarray:
    """uint8 [height,width,3]: the constant frame of one (r, g, b) triple of bytes"""
    s = check_settings(tuple(rgb) if not isinstance(rgb, (tuple, list)) else rgb)
    if s["to"] != "color":
        raise ValueError(f"color_ref: rgb={rgb!r}: use three integers in 0..255")
    out = np.empty((int(height), int(width), 3), np.uint8)
    out[...] = np.asarray(s["color"], np.uint8)
    return out


def bytes_ref(setting: dict, image, height: int, width: int, resample: str = "lanczos") -> np.ndarray:
    """uint8 [height,width,3] of a "color" or "image" setting at one size"""
    if setting["to"] == "color":
        return color_ref(setting["color"], height, width)
    if setting["to"] != "image":
        raise ValueError("bytes_ref: a blur has no bytes of its own: blur_ref makes them of a frame")
    return image_ref(image, height, width, resample)


def stream_ref(setting: dict, image, source, depth, matte: dict, resample: str = "lanczos", plane=None) -> np.ndarray:
    """fp16 [3,H,W]: the backdrop of one frame at the stream's size, as `matte.composite_ref(backdrop=)` takes it -- `frame_of` of
    the blurred source frame under the `matte` settings, of the colour or of the image"""
    H, W = tuple(source.shape[-2:])
    if setting["to"] == "blur":
        return frame_of(blur_ref(source, depth, matte["lo"], matte["hi"], matte["keep"], setting["radius"], setting["passes"], plane=plane))
    if torch.is_tensor(image) and image.dtype == torch.float16:
        return image.detach().cpu().numpy()
    return frame_of(np.ascontiguousarray(bytes_ref(setting, image, H, W, resample).transpose(2, 0, 1)))


def output_ref(setting: dict, image, source, depth, matte: dict, out_height: int, out_width: int, resample: str = "lanczos",
               plane=None) -> np.ndarray:
    """uint8 [Ho,Wo,3]: the backdrop of one frame at an output size, as `matte.composite_up_ref(backdrop=)` takes it.  A blur runs
    at the stream's size and its bytes go through `resize_ref`: a blurred frame loses nothing by being scaled up."""
    if setting["to"] == "blur":
        b = blur_ref(source, depth, matte["lo"], matte["hi"], matte["keep"], setting["radius"], setting["passes"], plane=plane)
        return resize_ref(np.ascontiguousarray(b.transpose(1, 2, 0)), out_height, out_width, resample)
    return bytes_ref(setting, image, out_height, out_width, resample)


# ----------------------------------------------------------------------------- the device side
class HipBackdrop:
    """What one `(H, W)` stream keeps on the device for its backdrop: the static fp16 blur frame, the prepared image or colour
    at the stream's size (fp16, through `frame_of`) and at output sizes (uint8 HWC), and for a blur at an output size a
    `HipResize` of its own (its tables and its byte buffer).  `stream` and `output` return `(tensor, records)`: the tensor
    that goes where the slot's source frame / camera buffer goes in the composite op, and the `(op, keep)` records the
    composite puts in front of its own in the same `OpList` -- the blur launch, and the resize of its frame.  Prepared buffers
    are kept per (image identity, size, filter); a device uint8 tensor that already has the target size is used in place."""

    MAX_PREPARED = 8

    def __init__(self, height: int, width: int, device="cuda:0"):
        if width % 8 or height < 1 or 3 * height * width >= 1 << 31:
            raise ValueError(f"HipBackdrop: width {width} must be a multiple of 8, height {height} at least 1 and 3 H W below 2^31")
        self.height, self.width, self.device = int(height), int(width), torch.device(device)
        self.frame = None                   # fp16 [3,H,W]: the blurred frame, made by the first blur
        self._up = None                     # resize.HipResize of its own: the blurred frame's way to an output size
        self._prepared = {}                 # key -> (tensor, the image it was made of)

    def blur_record(self, slot, matte: dict, setting: dict, plane=None):
        """the record of L2D_OP_FRAME_BACKDROP_BLUR for a `MatteLine` slot under the `matte` settings -> `frame`; with `plane`
        (op 58's raw matte) that plane in place of the depth plane and the ramp"""
        if self.frame is None:
            self.frame = torch.empty(3, self.height, self.width, dtype=torch.float16, device=self.device)
        if plane is not None:
            return ops.frame_backdrop_blur(slot.source, None, self.frame, H=self.height, W=self.width, r=setting["radius"],
                                           passes=setting["passes"], plane=plane)
        check_matte(matte["lo"], matte["hi"], keep=matte["keep"])
        lo32, inv32, hard = matte_params(matte["lo"], matte["hi"])
        return ops.frame_backdrop_blur(slot.source, slot.depth, self.frame, H=self.height, W=self.width, r=setting["radius"],
                                       passes=setting["passes"], lo32=lo32, inv32=inv32, hard=hard, far=matte["keep"] == "far")

    def _prepare(self, key, image, make):
        hit = self._prepared.get(key)
        if hit is not None and hit[1] is image:
            return hit[0]
        if len(self._prepared) >= self.MAX_PREPARED:
            self._prepared.clear()
        t = make()
        self._prepared[key] = (t, image)
        return t

    def _bytes(self, setting: dict, image, height: int, width: int, resample: str) -> torch.Tensor:
        """uint8 [height,width,3] on the device of a "color" or "image" setting"""
        if torch.is_tensor(image) and image.is_cuda:
            if image.dtype != torch.uint8 or tuple(image.shape) != (height, width, 3) or not image.is_contiguous():
                raise ValueError(f"backdrop: a device tensor is used in place and must be a contiguous uint8 [{height},{width},3] here, "
                                 f"got {image.dtype} {tuple(image.shape)}")
            return image
        ident = setting["color"] if setting["to"] == "color" else id(image)
        return self._prepare(("u8", setting["to"], ident, height, width, resample), image,
                             lambda: torch.from_numpy(bytes_ref(setting, image, height, width, resample)).to(self.device))

    def stream(self, slot, matte: dict, setting: dict, image=None, resample: str = "lanczos", plane=None):
        """(fp16 [3,H,W], records): the backdrop of the slot's frame at the stream's size, for `HipMatte.composite(backdrop=)`"""
        H, W = self.height, self.width
        if setting["to"] == "blur":
            blur = self.blur_record(slot, matte, setting, plane)
            return self.frame, [blur]
        if torch.is_tensor(image) and image.is_cuda:
            if image.dtype == torch.float16 and tuple(image.shape) == (3, H, W) and image.is_contiguous():
                return image, []
            b = self._bytes(setting, image, H, W, resample)            # (a video backdrop at the stream's size: the two fp32
            v = b.permute(2, 0, 1).to(torch.float32) * float(_TWO_OVER_255)      # steps of `frame_of`, one rounding each)
            return (v - 1.0).to(torch.float16).contiguous(), []
        ident = setting["color"] if setting["to"] == "color" else id(image)
        t = self._prepare(("f16", setting["to"], ident, H, W, resample), image, lambda: torch.from_numpy(np.ascontiguousarray(
            frame_of(bytes_ref(setting, image, H, W, resample).transpose(2, 0, 1)))).to(self.device))
        return t, []

    def output(self, slot, matte: dict, setting: dict, out_height: int, out_width: int, image=None, resample: str = "lanczos",
               plane=None):
        """(uint8 [Ho,Wo,3], records): the backdrop of the slot's frame at an output size, for `HipMatteUp.composite(backdrop=)`"""
        H, W = self.height, self.width
        if setting["to"] != "blur":
            return self._bytes(setting, image, int(out_height), int(out_width), resample), []
        key = (int(out_height), int(out_width), check_filter(resample))
        rs = self._up
        if rs is None or (rs.out_height, rs.out_width, rs.resample) != key:
            from .resize import HipResize
            rs = self._up = HipResize(H, W, key[0], key[1], key[2], device=self.device)
        blur = self.blur_record(slot, matte, setting, plane)
        up = ops.frame_resize(self.frame, rs.dev, rs.tx, rs.ty, B=1, H=H, W=W, Ho=key[0], Wo=key[1])
        return rs.dev[0], [blur, up]
