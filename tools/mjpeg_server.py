"""A running stream in a browser: frames -> StreamAnimateDiffusionDepthWrapper(output_type="jpeg") -> MJPEG over HTTP.

    python tools/mjpeg_server.py --config configs/toonyou.yaml --input frames/ [--prompt "..."] [--height 512 --width 512]
                                 [--port 8000] [--quality 75]
    python tools/mjpeg_server.py --config configs/toonyou.yaml --input post     # the browser's camera is the input

`/` is a page with one <img>; `/stream` is `multipart/x-mixed-replace; boundary=frame`, every part laid out as the reference's
demo does (demo/util.py:27-37, `jpeg.mjpeg_part`).  The input (a folder of images or an .npy stack, `stream_frames.read_frames`)
is looped for ever.  One producer thread owns the wrapper and the GPU; the HTTP handlers only ever read the latest part, so a
slow viewer drops frames instead of holding the stream back.  Standard library only (http.server).  The frame is encoded on
the device (jpeg_io.HipJpegEncoder): what crosses to the host is the JPEG file.

`--input post` closes the loop of the reference's demo (demo/app.py:81-85: `canvas.toBlob('image/jpeg')` -> websocket ->
`bytes_to_pil`): the page captures the camera with `getUserMedia`, draws it on a canvas and sends every frame as the body of
`POST /frame`; the wrapper takes the bytes as they are (decoded on the device, jpeg_io.HipJpegDecoder).  The first `sink` frames
posted are the warm-up; after that the producer always takes the NEWEST posted frame, and a frame that raises (a damaged file)
is dropped and counted.

`--style NAME=DREAMBOOTH[,LORA:ALPHA...]` (repeatable) registers further styles beside the config's own (`"default"`); their packed
weights stay resident on the device.  `POST /style` with a JSON body `{name: weight}` (up to four names, weights summing to 1)
switches or blends the running stream: the producer thread applies it between two frames (`wrapper.set_style`), without a
re-warm -- unless the body also holds `"rewarm": true` (the sinks are re-warmed on the warm-up window right behind the switch) or
`"rewarm": "recent"` (on the last frames; needs `--keep-recent`); a style cannot be named "rewarm" on this route.  `GET /style`
answers `{"styles": [...], "current": {...}}`.  `POST /rewarm` with `{"source": "warmup"}` or `{"source": "recent"}` re-warms the
sinks alone, between two frames (`wrapper.rewarm`); `GET /rewarm` answers `{"rewarms": n, "failed": m}`.

`--matte LO,HI[,FEATHER[,far]]` stylises only the near side (`far`: the far side) of a ramp over the frame's own depth map and
keeps the real picture elsewhere (`wrapper.set_matte`: composited on the device, in front of the JPEG encoder).  `POST /matte`
with the same text as its body, or `off`, changes it while the stream runs; the producer applies it between two frames.
`GET /matte` answers the current settings as JSON (`null`: off).

`--color-lock source|ema[,STRENGTH[,RATE]]` holds the output's per-channel brightness and contrast to the source frame's or to a
running average of the stream's own (`wrapper.set_color_lock`: two small launches on the device in front of the JPEG encoder).
`POST /color` with the same text as its body, or `off`, changes it while the stream runs; `GET /color` answers the current
settings as JSON (`null`: off).

`--output-size WxH[,FILTER]` serves frames of W x H pixels instead of the UNet's size (`wrapper.set_output_size`: Pillow's
resampling in one launch on the device, in front of a JPEG encoder of that size; FILTER is lanczos, bicubic or bilinear; both
sizes are multiples of 16 and W is at most 1920).  `POST /size` with the same text as its body, or `off`, changes it while the
stream runs; `GET /size` answers the current settings as JSON (`null`: off).

`--matte-source stream|camera` chooses what a matte keeps real under an output size (`wrapper.set_matte_source`): `stream`, the
UNet-sized source frame resampled with the rest of the picture, or `camera`, the posted frame's own pixels resampled to the output
size and composited there.  `POST /matte-source` with one of the two words changes it while the stream runs; `GET /matte-source`
answers the current one as a JSON string.

`--steady LO,HI[,STRENGTH[,RADIUS]]` holds the previous output pixel where the frame's source did not move
(`wrapper.set_steady`: one small launch on the device behind the colour lock; LO and HI are byte levels of the locally averaged
motion).  `POST /steady` with the same text as its body, or `off`, changes it while the stream runs; `GET /steady` answers the
current settings as JSON (`null`: off).

`--steady-follow R[,BIAS]` lets the steady mode follow the source's motion (`wrapper.set_steady_follow`: every 8 x 8 block is
matched against the frame before over up to R pixels, 1..8, and the previous output is held along the vectors -- under a
hand-held camera or a pan, where plain steady holds nothing; BIAS, default 256, keeps noise in flat areas from producing
vectors).  It acts only while `--steady` is set.  `POST /steady-follow` with the same text changes it while the stream runs, an
empty body or `off` clears it; `GET /steady-follow` answers the current settings as JSON.

`--matte-hold LO,HI[,STRENGTH[,RADIUS[,SEARCH[,BIAS]]]]` keeps the matte still where the camera is still
(`wrapper.set_matte_hold`: the matte blended in time with the previous held one by steady's measure of where the source moved;
SEARCH 1..8 follows the source's motion).  It acts only while `--matte` is set.  `POST /matte-hold` with the same text changes
it while the stream runs, an empty body or `off` clears it; `GET /matte-hold` answers the current settings as JSON.

`--matte-edge R[,EPS]` refines the matte by the frame it cuts, so that its edges land on the frame's own edges
(`wrapper.set_matte_edge`: a guided filter of radius R in 1..8 pixels, one more launch in front of the composite; EPS, default
10, is the contrast in byte levels below which a window counts as flat).  It acts only while a matte is set.  `POST /matte-edge`
with the same text as its body, or `off`, changes it while the stream runs; `GET /matte-edge` answers the current settings as
JSON (`null`: off).

`--detail R[,EPS[,STRENGTH[,LIMIT]]]` brings the camera's fine detail into the frame at the output size (`wrapper.set_detail`: the
camera frame's high-pass at the output size, added with the local regression slope of the styled frame on the source frame over
windows of radius R in 1..8 pixels; EPS, default 2, is the contrast in byte levels below which a window counts as flat,
STRENGTH, default 1, scales the injected term and LIMIT, default 64, bounds it in byte levels).  It acts only while an output
size is set.  `POST /detail` with the same text as its body, or `off`, changes it while the stream runs; `GET /detail` answers
the current settings as JSON (`null`: off).

`--backdrop blur[,R[,PASSES]] | RRGGBB | PATH` puts something else behind the matte than the real frame (`wrapper.set_backdrop`):
the room blurred with the subject left out (PASSES boxes of radius R, defaults 6 and 3), a colour as six hex digits (for a
chroma key further down), or an image file, cropped to the frame's aspect ratio.  It acts only while a matte is set.  `POST
/backdrop` with the same text as its body changes it while the stream runs, an empty body (or `off`) clears it; `GET /backdrop`
answers the current settings as JSON (`null`: off).

`--mask PATH` sets a sticky mask (`wrapper.set_mask`: an image of mode L, 1, I;16 or F, of any size, covering the camera frame's
field of view): the matte of every frame, in place of the depth ramp or combined with it -- a fixed region, "only the window".
It needs `--matte`, whose feather and `far` keep acting on it.  `POST /mask` with an image file as its body (decoded on the host)
replaces it while the stream runs, an empty body or `off` clears it; `GET /mask` answers `{"size": [h, w]}` or `null`.
`--mask-input COMBINE[,invert]` says how a mask meets the ramp (`wrapper.set_mask_input`: `replace`, `and` or `or`); `POST
/mask-input` with the same text changes it, `GET /mask-input` answers the current settings as JSON.  A body either route
refuses gets a 400 and is counted (`failed`).

`--matte-key RRGGBB|PATH|capture[,LO,HI[,LUMA[,RADIUS[,COMBINE[,invert]]]]]` cuts the frame by a key (`wrapper.set_matte_key`):
six hex digits are a key colour (a green screen: `00b140`), a path is a clean plate (a picture of the empty room from a camera
that does not move), `capture` takes the plate from the stream's next output.  It needs `--matte` and excludes `--mask`.  `POST
/matte-key` with the same text changes it while the stream runs, an empty body or `off` clears it; `POST /matte-key/capture` (no
body) takes the plate again with the settings kept; `GET /matte-key` answers the current settings as JSON (`to` is the colour,
`"plate"` or, until it has happened, `"capture"`; `null`: off).  A body the routes refuse gets a 400 and is counted.

`--matte-key-adapt RATE[,ABSORB]` lets the plate of the key follow drifting light (`wrapper.set_matte_key_adapt`): after every
frame the plate moves by RATE of the way towards the frame where the key says background, by ABSORB of the way (default 0) where
it says subject; both lie in [0, 0.5].  It needs a `--matte-key` against a plate (a path or `capture`).  `POST /matte-key/adapt`
with the same text changes it while the stream runs, an empty body or `off` clears it; `GET /matte-key` then carries `"adapt":
{"rate": ..., "absorb": ...}`.  `GET /matte-key/plate` answers the plate of this moment as a JPEG file (404 while there is
none): the producer hands it over between two frames.

`--matte-key-gain [LIMIT[,MIN_SHARE]]` lets the key against a plate follow a sudden exposure or white-balance step
(`wrapper.set_matte_key_gain`): every frame measures one gain per channel between the plate and the frame, the median over the
frame's pixels, and is keyed against the plate times that gain.  LIMIT in [1, 3.99] (default 2) bounds the gain, MIN_SHARE in [0,
1] (default 1/16) is the part of the frame a channel needs as valid samples; without a value (or `on`) the defaults.  It needs a
`--matte-key` against a plate and works with or without `--matte-key-adapt`.  `POST /matte-key/gain` with the same text changes it
while the stream runs, an empty body or `off` clears it; `GET /matte-key/gain` answers `{"limit", "min_share", "gain", "share"}`
-- the setting and the last frame's measurement per channel (`null` before the first keyed frame) -- or 404 while it is off: the
producer hands it over between two frames.  The body of `GET /matte-key` does not change.

`--cut-detect [THUMB,HIST[,RATIO[,GAP]]]` finds scene cuts on the device (`wrapper.set_cut_detect`): every
frame that enters the stream is measured against the one before, two small launches and no synchronisation; without a value (or
`on`) the defaults, which are a guess, untuned on footage.  `--auto-rewarm` (implies `--keep-recent`, needs `--cut-detect`) re-warms
the sinks by themselves once the last frames all lie behind a cut (`wrapper.set_auto_rewarm`).  `POST /cut-detect` with the same
text, `on` or `off`, and `POST /auto-rewarm` with `on` or `off`, change them between two frames; `GET /cut-detect` and `GET
/auto-rewarm` answer the current settings, `GET /cuts` answers `{"cuts": [frame indices since prepare], "auto_rewarms": n, "last":
{the newest record}}` as of the last frame."""
import argparse
import json
import os
import sys
import threading
from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

PAGE = (b"<!doctype html><html><head><title>live2diff_amd</title></head>"
        b"<body style=\"margin:0;background:#111\"><img src=\"/stream\" style=\"display:block;margin:auto;max-width:100%\"></body></html>\n")


CAMERA_PAGE = (b"<!doctype html><html><head><title>live2diff_amd</title></head>"
               b"<body style=\"margin:0;background:#111\"><img src=\"/stream\" style=\"display:block;margin:auto;max-width:100%\">"
               b"<video id=\"v\" autoplay playsinline muted style=\"display:none\"></video><canvas id=\"c\" style=\"display:none\"></canvas>"
               b"<script>\n"
               b"const v = document.getElementById('v'), c = document.getElementById('c');\n"
               b"async function send() {\n"
               b"  if (v.videoWidth) {\n"
               b"    c.width = v.videoWidth; c.height = v.videoHeight; c.getContext('2d').drawImage(v, 0, 0);\n"
               b"    const blob = await new Promise(r => c.toBlob(r, 'image/jpeg', 0.9));\n"
               b"    try { await fetch('/frame', {method: 'POST', body: blob}); } catch (e) {}\n"
               b"  }\n"
               b"  setTimeout(send, v.videoWidth ? 0 : 100);\n"
               b"}\n"
               b"navigator.mediaDevices.getUserMedia({video: true}).then(s => { v.srcObject = s; send(); });\n"
               b"</script></body></html>\n")
MAX_POST = 16 << 20            # bytes of one posted frame


class Inbox:
    """What `POST /frame` delivers.  The first `warmup` frames are all kept, in order (`warmup_frames()` blocks until they are
    there); of the later ones only the newest: `take(timeout)` returns it once, or None when nothing new came in time or the
    inbox was closed.  `posted` / `replaced` / `failed` count frames posted, overwritten before anyone took them, and dropped by the
    producer because the wrapper raised."""

    def __init__(self, warmup: int):
        self._cond = threading.Condition()
        self._need, self._warm, self._frame, self._closed = int(warmup), [], None, False
        self.posted = self.replaced = self.failed = 0

    def put(self, data: bytes) -> None:
        with self._cond:
            self.posted += 1
            if len(self._warm) < self._need:
                self._warm.append(data)
            else:
                self.replaced += self._frame is not None
                self._frame = data
            self._cond.notify_all()

    def close(self) -> None:
        with self._cond:
            self._closed = True
            self._cond.notify_all()

    def warmup_frames(self):
        with self._cond:
            self._cond.wait_for(lambda: len(self._warm) >= self._need or self._closed)
            return list(self._warm) if len(self._warm) >= self._need else None

    def take(self, timeout=None):
        with self._cond:
            self._cond.wait_for(lambda: self._frame is not None or self._closed, timeout)
            data, self._frame = self._frame, None
            return data


class StyleBox:
    """What `POST /style` delivers: the newest requested mix, applied by the producer between two frames.  `names` are the styles the
    wrapper knows; `current` is the mix last applied; `failed` counts requests the wrapper refused.  What `POST /rewarm` delivers
    waits here too -- the newest requested source, applied behind a posted style between the same two frames.  `keep_recent`: whether
    the wrapper keeps a recent window ("recent" is refused at the door without one); `rewarms` counts the re-warms done,
    `rewarm_failed` those the wrapper refused (fewer than F frames since `prepare`, say).  `cuts`: the `CutBox` of the cut detector
    and the automatic re-warm, or None; it is applied behind the style and the re-warm, between the same two frames."""

    def __init__(self, names, current=None, keep_recent: bool = False, cuts: "CutBox" = None):
        self.cuts = cuts
        self._lock = threading.Lock()
        self.names, self.current, self._want, self.failed = list(names), dict(current or {}), None, 0
        self._rewarm = False
        self.keep_recent, self._source, self.rewarms, self.rewarm_failed = bool(keep_recent), None, 0, 0

    def put(self, mix: dict, rewarm=False) -> None:
        """`rewarm`: False, True (the warm-up window) or "recent" -- `set_style`'s keyword, for this request"""
        with self._lock:
            self._want, self._rewarm = dict(mix), rewarm

    def take(self):
        with self._lock:
            mix, self._want = self._want, None
            return mix

    def put_rewarm(self, source: str) -> None:
        if source not in REWARM_SOURCES:
            raise ValueError(f"source={source!r}: use 'warmup' or 'recent'")
        if source == "recent" and not self.keep_recent:
            raise ValueError("source 'recent' needs a server started with --keep-recent")
        with self._lock:
            self._source = source

    def apply(self, wrapper) -> None:
        """(producer thread, between frames)"""
        with self._lock:
            mix, rewarm, self._want, self._rewarm = self._want, self._rewarm, None, False
            source, self._source = self._source, None
        if mix is not None:
            try:
                if rewarm:
                    wrapper.set_style(mix, rewarm=rewarm)
                else:
                    wrapper.set_style(mix)
                self.current = dict(wrapper.style)
            except (KeyError, ValueError):
                self.failed += 1
        if source is not None:
            try:
                wrapper.rewarm(source)
                self.rewarms += 1
            except (ValueError, RuntimeError):
                self.rewarm_failed += 1
        if self.cuts is not None:
            self.cuts.apply(wrapper)


REWARM_SOURCES = ("warmup", "recent")


class CutBox:
    """What `POST /cut-detect` and `POST /auto-rewarm` deliver: the newest requested detector settings (`"off"`: none) and the newest
    requested switch, applied by the producer between two frames, the detector first.  `current` is the setting last applied;
    `failed` counts requests the wrapper refused (an automatic re-warm without a detector, say).  `keep_recent`: whether the wrapper
    keeps a recent window (switching the automatic re-warm on is refused at the door without one).  `report` is what `GET /cuts`
    answers, copied from the wrapper by the producer behind every `apply`."""

    _NOTHING = object()

    def __init__(self, current=None, auto: bool = False, keep_recent: bool = False):
        self._lock = threading.Lock()
        self.current, self.auto, self.keep_recent, self.failed = current, bool(auto), bool(keep_recent), 0
        self._want, self._want_auto = self._NOTHING, None
        self.report = {"cuts": [], "auto_rewarms": 0, "last": None}

    def put(self, settings) -> None:
        with self._lock:
            self._want = settings

    def put_auto(self, on: bool) -> None:
        if on and not self.keep_recent:
            raise ValueError("the automatic re-warm needs a server started with --auto-rewarm or --keep-recent")
        with self._lock:
            self._want_auto = bool(on)

    def apply(self, wrapper) -> None:
        """(producer thread, between frames)"""
        with self._lock:
            want, auto, self._want, self._want_auto = self._want, self._want_auto, self._NOTHING, None
        if want is not self._NOTHING:
            try:
                if want is None:
                    wrapper.clear_cut_detect()
                else:
                    wrapper.set_cut_detect(**want)
            except ValueError:
                self.failed += 1
        if auto is not None:
            try:
                wrapper.set_auto_rewarm(auto)
            except ValueError:
                self.failed += 1
        report = {"cuts": [int(n) for n in wrapper.cuts], "auto_rewarms": int(wrapper.auto_rewarms), "last": wrapper.last_cut_record}
        with self._lock:
            self.current, self.auto, self.report = wrapper.cut_detect, bool(wrapper.auto_rewarm), report


def parse_cut_detect_arg(text: str):
    """`on` or `THUMB,HIST[,RATIO[,GAP]]` -> the keywords of `wrapper.set_cut_detect`; `off` -> None; ValueError otherwise"""
    from live2diff_amd.cut import check_settings
    text = text.strip()
    if text == "off":
        return None
    if text == "on":
        return check_settings()
    parts = [p.strip() for p in text.split(",")]
    if not 2 <= len(parts) <= 4 or not all(parts):
        raise ValueError("use on, off or THUMB,HIST[,RATIO[,GAP]]")
    kw = dict(thumb=float(parts[0]), hist=float(parts[1]))
    if len(parts) > 2:
        kw["ratio"] = float(parts[2])
    if len(parts) > 3:
        kw["gap"] = int(parts[3])
    return check_settings(**kw)


def parse_auto_rewarm_arg(text: str) -> bool:
    """`on` / `off` -> True / False; ValueError otherwise"""
    text = text.strip()
    if text not in ("on", "off"):
        raise ValueError("use on or off")
    return text == "on"


def parse_rewarm_body(body: bytes) -> str:
    """the body of `POST /rewarm`, `{"source": "warmup" | "recent"}` -> the source"""
    req = json.loads(body.decode())                       # (json.JSONDecodeError and UnicodeDecodeError are ValueErrors)
    if not isinstance(req, dict) or set(req) != {"source"} or req["source"] not in REWARM_SOURCES:
        raise ValueError('use {"source": "warmup"} or {"source": "recent"}')
    return req["source"]


def parse_style_rewarm(value):
    """the "rewarm" entry of a `POST /style` body -> `set_style`'s keyword"""
    if value is False or value is True or value == "recent":
        return value
    if value == "warmup":
        return True
    raise ValueError('"rewarm": use true, false, "warmup" or "recent"')


def parse_matte_arg(text: str):
    """`LO,HI[,FEATHER[,far]]` -> the keywords of `wrapper.set_matte`, `off` -> None; ValueError otherwise (the wrapper checks the
    ranges once more)"""
    from live2diff_amd.matte import check_settings
    text = text.strip()
    if text == "off":
        return None
    parts = [t.strip() for t in text.split(",")]
    if not 2 <= len(parts) <= 4 or (len(parts) == 4 and parts[3] not in ("far", "near")):
        raise ValueError(f"matte {text!r}: use LO,HI[,FEATHER[,far]] or off")
    try:
        lo, hi = float(parts[0]), float(parts[1])
        feather = int(parts[2]) if len(parts) > 2 else 0
    except ValueError:
        raise ValueError(f"matte {text!r}: LO and HI are numbers in [0, 1], FEATHER an integer from 0 to 8") from None
    s = check_settings(lo, hi, keep=parts[3] if len(parts) == 4 else "near", feather=feather)
    return dict(lo=s["lo"], hi=s["hi"], keep=s["keep"], feather=s["feather"])


class MatteBox:
    """What `POST /matte` delivers: the newest requested matte (a dict of `set_matte` keywords, or None for `off`), applied by the
    producer between two frames.  `current` is what was last applied; `failed` counts requests the wrapper refused."""
    _NOTHING = object()

    def __init__(self, current=None):
        self._lock = threading.Lock()
        self.current, self._want, self.failed = current, self._NOTHING, 0

    def put(self, settings) -> None:
        with self._lock:
            self._want = settings

    def apply(self, wrapper) -> None:
        """(producer thread, between frames)"""
        with self._lock:
            want, self._want = self._want, self._NOTHING
        if want is self._NOTHING:
            return
        try:
            if want is None:
                wrapper.clear_matte()
            else:
                wrapper.set_matte(want["lo"], want["hi"], keep=want["keep"], feather=want["feather"])
            self.current = wrapper.matte
        except ValueError:
            self.failed += 1


def parse_color_arg(text: str):
    """`source|ema[,STRENGTH[,RATE]]` -> the keywords of `wrapper.set_color_lock`, `off` -> None; ValueError otherwise"""
    from live2diff_amd.color_lock import check_settings
    text = text.strip()
    if text == "off":
        return None
    parts = [t.strip() for t in text.split(",")]
    if not 1 <= len(parts) <= 3 or parts[0] not in ("source", "ema"):
        raise ValueError(f"color lock {text!r}: use source|ema[,STRENGTH[,RATE]] or off")
    try:
        strength = float(parts[1]) if len(parts) > 1 else 1.0
        rate = float(parts[2]) if len(parts) > 2 else 0.1
    except ValueError:
        raise ValueError(f"color lock {text!r}: STRENGTH is a number in [0, 1], RATE a number in (0, 1]") from None
    s = check_settings(parts[0], strength, rate)
    return dict(to=s["mode"], strength=s["strength"], rate=s["rate"])


class ColorBox:
    """What `POST /color` delivers: the newest requested colour lock (a dict of `set_color_lock` keywords, or None for `off`),
    applied by the producer between two frames.  `current` is what was last applied; `failed` counts requests the wrapper refused."""
    _NOTHING = object()

    def __init__(self, current=None):
        self._lock = threading.Lock()
        self.current, self._want, self.failed = current, self._NOTHING, 0

    def put(self, settings) -> None:
        with self._lock:
            self._want = settings

    def apply(self, wrapper) -> None:
        """(producer thread, between frames)"""
        with self._lock:
            want, self._want = self._want, self._NOTHING
        if want is self._NOTHING:
            return
        try:
            if want is None:
                wrapper.clear_color_lock()
            else:
                wrapper.set_color_lock(want["to"], strength=want["strength"], rate=want["rate"])
            self.current = wrapper.color_lock
        except ValueError:
            self.failed += 1


def parse_steady_arg(text: str):
    """`LO,HI[,STRENGTH[,RADIUS]]` -> the keywords of `wrapper.set_steady`, `off` -> None; ValueError otherwise"""
    from live2diff_amd.steady import check_settings
    text = text.strip()
    if text == "off":
        return None
    parts = [t.strip() for t in text.split(",")]
    if not 2 <= len(parts) <= 4:
        raise ValueError(f"steady {text!r}: use LO,HI[,STRENGTH[,RADIUS]] or off")
    try:
        lo, hi = float(parts[0]), float(parts[1])
        strength = float(parts[2]) if len(parts) > 2 else 0.8
        radius = int(parts[3]) if len(parts) > 3 else 2
    except ValueError:
        raise ValueError(f"steady {text!r}: LO and HI are numbers in [0, 255], STRENGTH a number in [0, 1], RADIUS an integer "
                         "from 0 to 8") from None
    s = check_settings(lo, hi, strength, radius)
    return dict(lo=s["lo"], hi=s["hi"], strength=s["strength"], radius=s["radius"])


class SteadyBox:
    """What `POST /steady` delivers: the newest requested steady mode (a dict of `set_steady` keywords, or None for `off`),
    applied by the producer between two frames.  `current` is what was last applied; `failed` counts requests the wrapper refused."""
    _NOTHING = object()

    def __init__(self, current=None):
        self._lock = threading.Lock()
        self.current, self._want, self.failed = current, self._NOTHING, 0

    def put(self, settings) -> None:
        with self._lock:
            self._want = settings

    def apply(self, wrapper) -> None:
        """(producer thread, between frames)"""
        with self._lock:
            want, self._want = self._want, self._NOTHING
        if want is self._NOTHING:
            return
        try:
            if want is None:
                wrapper.clear_steady()
            else:
                wrapper.set_steady(want["lo"], want["hi"], strength=want["strength"], radius=want["radius"])
            self.current = wrapper.steady
        except ValueError:
            self.failed += 1


def parse_steady_follow_arg(text: str):
    """`R[,BIAS]` -> the keywords of `wrapper.set_steady_follow`, `off` -> None; ValueError otherwise"""
    from live2diff_amd.steady import FOLLOW_MAX_BIAS, FOLLOW_MAX_SEARCH, check_follow
    text = text.strip()
    if text == "off":
        return None
    parts = [t.strip() for t in text.split(",")]
    if not 1 <= len(parts) <= 2:
        raise ValueError(f"steady follow {text!r}: use R[,BIAS] or off")
    try:
        search = int(parts[0])
        bias = int(parts[1]) if len(parts) > 1 else 256
    except ValueError:
        raise ValueError(f"steady follow {text!r}: R is an integer from 1 to {FOLLOW_MAX_SEARCH}, BIAS an integer from 0 to "
                         f"{FOLLOW_MAX_BIAS}") from None
    return check_follow(search, bias)


class SteadyFollowBox:
    """What `POST /steady-follow` delivers: the newest requested follow setting (a dict of `set_steady_follow` keywords, or None
    for `off` and for an empty body), applied by the producer between two frames.  `current` is what was last applied; `failed`
    counts requests the wrapper refused."""
    _NOTHING = object()

    def __init__(self, current=None):
        self._lock = threading.Lock()
        self.current, self._want, self.failed = current, self._NOTHING, 0

    def put(self, settings) -> None:
        with self._lock:
            self._want = settings

    def apply(self, wrapper) -> None:
        """(producer thread, between frames)"""
        with self._lock:
            want, self._want = self._want, self._NOTHING
        if want is self._NOTHING:
            return
        try:
            if want is None:
                wrapper.clear_steady_follow()
            else:
                wrapper.set_steady_follow(want["search"], want["bias"])
            self.current = wrapper.steady_follow
        except ValueError:
            self.failed += 1


def parse_matte_hold_arg(text: str):
    """`LO,HI[,STRENGTH[,RADIUS[,SEARCH[,BIAS]]]]` -> the keywords of `wrapper.set_matte_hold`, `off` -> None; ValueError otherwise"""
    from live2diff_amd.matte import check_hold
    text = text.strip()
    if text == "off":
        return None
    parts = [t.strip() for t in text.split(",")]
    if not 2 <= len(parts) <= 6:
        raise ValueError(f"matte hold {text!r}: use LO,HI[,STRENGTH[,RADIUS[,SEARCH[,BIAS]]]] or off")
    try:
        lo, hi = float(parts[0]), float(parts[1])
        strength = float(parts[2]) if len(parts) > 2 else 0.8
        radius, search, bias = (int(parts[k]) if len(parts) > k else d for k, d in ((3, 2), (4, 0), (5, 256)))
    except ValueError:
        raise ValueError(f"matte hold {text!r}: LO, HI and STRENGTH are numbers, RADIUS, SEARCH and BIAS integers") from None
    return check_hold(lo, hi, strength, radius, search, bias)


class MatteHoldBox:
    """What `POST /matte-hold` delivers: the newest requested hold (a dict of `set_matte_hold` keywords, or None for `off` and for
    an empty body), applied by the producer between two frames.  `current` is what was last applied; `failed` counts requests
    the wrapper refused."""
    _NOTHING = object()

    def __init__(self, current=None):
        self._lock = threading.Lock()
        self.current, self._want, self.failed = current, self._NOTHING, 0

    def put(self, settings) -> None:
        with self._lock:
            self._want = settings

    def apply(self, wrapper) -> None:
        """(producer thread, between frames)"""
        with self._lock:
            want, self._want = self._want, self._NOTHING
        if want is self._NOTHING:
            return
        try:
            if want is None:
                wrapper.clear_matte_hold()
            else:
                wrapper.set_matte_hold(want["lo"], want["hi"], strength=want["strength"], radius=want["radius"], search=want["search"],
                                       bias=want["bias"])
            self.current = wrapper.matte_hold
        except ValueError:
            self.failed += 1


def parse_mask_input_arg(text: str):
    """`COMBINE[,invert]` -> the keywords of `wrapper.set_mask_input`; ValueError otherwise"""
    from live2diff_amd.mask_io import check_settings
    parts = [t.strip() for t in text.strip().split(",")]
    if not 1 <= len(parts) <= 2 or (len(parts) == 2 and parts[1] != "invert"):
        raise ValueError(f"mask input {text!r}: use replace, and or or, optionally followed by ,invert")
    return check_settings(parts[0], len(parts) == 2)


def parse_mask_body(body: bytes):
    """the body of `POST /mask`: an image file -> its array as `wrapper.set_mask` takes it; empty or `off` -> None; ValueError for
    anything Pillow cannot decode or whose mode is no mask's"""
    import io

    from live2diff_amd.mask_io import _as_mask, load
    if body.strip() in (b"", b"off"):
        return None
    from PIL import Image
    try:
        with Image.open(io.BytesIO(body)) as im:
            im.load()
            return _as_mask(load(im.copy(), "POST /mask"))
    except (OSError, SyntaxError, EOFError) as e:          # (what Pillow raises on a body that is no image, or a damaged one)
        raise ValueError(f"POST /mask: the body cannot be read as an image: {e}") from None


class MaskBox:
    """What `POST /mask` and `POST /mask-input` deliver: the newest requested sticky mask (an array, or None for `off` and for an
    empty body) and the newest requested mask input (a dict of `set_mask_input` keywords), applied by the producer between two
    frames.  `current` / `current_input` are what was last applied; `failed` counts bodies the routes refused with a 400 and
    requests the wrapper refused."""
    _NOTHING = object()

    def __init__(self, current=None, current_input=None):
        self._lock = threading.Lock()
        self.current, self.current_input, self.failed = current, current_input, 0
        self._want = self._want_input = self._NOTHING

    def put(self, mask) -> None:
        with self._lock:
            self._want = mask

    def put_input(self, settings) -> None:
        with self._lock:
            self._want_input = settings

    def refused(self) -> None:
        with self._lock:
            self.failed += 1

    def apply(self, wrapper) -> None:
        """(producer thread, between frames)"""
        with self._lock:
            want, self._want = self._want, self._NOTHING
            want_input, self._want_input = self._want_input, self._NOTHING
        try:
            if want_input is not self._NOTHING:
                wrapper.set_mask_input(**want_input)
                self.current_input = wrapper.mask_input
        except ValueError:
            self.refused()
        try:
            if want is None:
                wrapper.clear_mask()
                self.current = None
            elif want is not self._NOTHING:
                wrapper.set_mask(want)
                self.current = dict(size=[int(want.shape[0]), int(want.shape[1])])
        except ValueError:                         # (no matte, or a geometry the ingest refuses)
            self.refused()


def parse_matte_key_arg(text: str):
    """`RRGGBB|PATH|capture[,LO,HI[,LUMA[,RADIUS[,COMBINE[,invert]]]]]` -> the keywords of `wrapper.set_matte_key` (`to` among
    them: the colour's bytes, the image's uint8 [H,W,3] array, decoded here, or "capture"); `off` or nothing -> None; ValueError
    otherwise.  Fields left out keep the defaults of the kind of key (`matte_key.DEFAULTS`, with luma 0.25 for a plate)."""
    from live2diff_amd.backdrop import load_image
    from live2diff_amd.matte_key import check_settings
    text = text.strip()
    if text in ("", "off"):
        return None
    usage = "use RRGGBB, the path of an image or capture, then [,LO,HI[,LUMA[,RADIUS[,COMBINE[,invert]]]]], or off"
    parts = [t.strip() for t in text.split(",")]
    head, rest = parts[0], parts[1:]
    if len(rest) == 1 or len(rest) > 6 or (len(rest) == 6 and rest[5] != "invert"):
        raise ValueError(f"matte key {text!r}: {usage}")
    if len(head) == 6 and all(c in "0123456789abcdefABCDEF" for c in head):
        to = tuple(int(head[i:i + 2], 16) for i in (0, 2, 4))
    elif head == "capture":
        to = "capture"
    elif os.path.isfile(head):
        to = load_image(head)
    else:
        raise ValueError(f"matte key {text!r}: {usage} (there is no such file)")
    try:
        lo, hi = (float(rest[i]) if len(rest) > i else None for i in (0, 1))
        luma = float(rest[2]) if len(rest) > 2 else None
        radius = int(rest[3]) if len(rest) > 3 else 1
    except ValueError:
        raise ValueError(f"matte key {text!r}: LO, HI and LUMA are numbers, RADIUS an integer from 0 to 4") from None
    s = check_settings(lo, hi, luma, radius, rest[4] if len(rest) > 4 else "replace", len(rest) == 6, plate=not isinstance(to, tuple))
    return dict(s, to=to)


def parse_matte_key_adapt_arg(text: str):
    """`RATE[,ABSORB]` -> the keywords of `wrapper.set_matte_key_adapt`; `off` or nothing -> None; ValueError otherwise"""
    from live2diff_amd.matte_key import check_adapt
    text = text.strip()
    if text in ("", "off"):
        return None
    parts = [t.strip() for t in text.split(",")]
    if not 1 <= len(parts) <= 2:
        raise ValueError(f"matte key adapt {text!r}: use RATE[,ABSORB] or off")
    try:
        rate, absorb = float(parts[0]), (float(parts[1]) if len(parts) > 1 else 0.0)
    except ValueError:
        raise ValueError(f"matte key adapt {text!r}: RATE and ABSORB are numbers in [0, 0.5]") from None
    return check_adapt(rate, absorb)


def parse_matte_key_gain_arg(text: str):
    """`on` or `LIMIT[,MIN_SHARE]` -> the keywords of `wrapper.set_matte_key_gain`; `off` or nothing -> None; ValueError otherwise"""
    from live2diff_amd.matte_key import GAIN_DEFAULTS, check_gain
    text = text.strip()
    if text in ("", "off"):
        return None
    if text == "on":
        return dict(GAIN_DEFAULTS)
    parts = [t.strip() for t in text.split(",")]
    if not 1 <= len(parts) <= 2:
        raise ValueError(f"matte key gain {text!r}: use on, LIMIT[,MIN_SHARE] or off")
    try:
        limit, min_share = float(parts[0]), (float(parts[1]) if len(parts) > 1 else GAIN_DEFAULTS["min_share"])
    except ValueError:
        raise ValueError(f"matte key gain {text!r}: LIMIT is a number in [1, 3.99], MIN_SHARE one in [0, 1]") from None
    return check_gain(limit, min_share)


class MatteKeyBox:
    """What `POST /matte-key` and `POST /matte-key/capture` deliver: the newest requested key (a dict of `set_matte_key` keywords,
    or None for an empty body or `off`) and a request to take the plate again, applied by the producer between two frames.
    `current` is what was last applied (the `matte_key` property, with the colour as a list); `failed` counts bodies the route
    refused with a 400 and requests the wrapper refused (no matte, a sticky mask, a capture without a key).  `POST
    /matte-key/adapt` delivers the adaptive plate's setting the same way (`current` then carries `adapt`), and `GET
    /matte-key/plate` asks the producer for the plate of this moment: `take_plate` waits up to `plate_wait` seconds for it.  `POST
    /matte-key/gain` delivers the plate gain's setting the same way; `current` does not carry it: `GET /matte-key/gain` asks the
    producer for the setting and the last measurement (`take_gain`, which waits as `take_plate` does)."""
    _NOTHING = object()
    plate_wait = 2.0

    def __init__(self, current=None, adapt=None):
        self._lock = threading.Lock()
        self._plate_ready = threading.Condition(self._lock)
        self.current, self._want, self._capture, self.failed = self.view(current, adapt), self._NOTHING, False, 0
        self._adapt, self._want_plate, self._plate = self._NOTHING, False, None
        self._gain, self._want_gain, self._gain_info = self._NOTHING, False, None

    def put_gain(self, settings) -> None:
        with self._lock:
            self._gain = settings

    def take_gain(self):
        """(a handler thread) {limit, min_share, gain, share} as the producer last handed it over, or None: asks for it and waits"""
        with self._plate_ready:
            if self._gain_info is None:
                self._want_gain = True
                self._plate_ready.wait_for(lambda: self._gain_info is not None, timeout=self.plate_wait)
            info, self._gain_info = self._gain_info, None
            return info

    @staticmethod
    def view(key, adapt=None):
        if key is None:
            return None
        out = dict(key, to=list(key["to"]) if isinstance(key["to"], tuple) else key["to"])
        return out if adapt is None else dict(out, adapt=dict(adapt))

    def put_adapt(self, settings) -> None:
        with self._lock:
            self._adapt = settings

    def take_plate(self):
        """(a handler thread) the plate the producer last handed over, uint8 [H,W,3], or None: asks for one and waits for it"""
        with self._plate_ready:
            if self._plate is None:
                self._want_plate = True
                self._plate_ready.wait_for(lambda: self._plate is not None, timeout=self.plate_wait)
            plate, self._plate = self._plate, None
            return plate

    def put(self, settings) -> None:
        with self._lock:
            self._want, self._capture = settings, False       # (a new key supersedes a capture asked for before it)

    def capture(self) -> None:
        with self._lock:
            self._capture = True

    def refused(self) -> None:
        with self._lock:
            self.failed += 1

    def apply(self, wrapper) -> None:
        """(producer thread, between frames)"""
        with self._lock:
            want, self._want = self._want, self._NOTHING
            capture, self._capture = self._capture, False
            adapt, self._adapt = self._adapt, self._NOTHING
            want_plate, self._want_plate = self._want_plate, False
            gain, self._gain = self._gain, self._NOTHING
            want_gain, self._want_gain = self._want_gain, False
        try:
            if want is None:
                wrapper.clear_matte_key()
            elif want is not self._NOTHING:
                wrapper.set_matte_key(**want)
        except ValueError:
            self.refused()
        try:
            if capture:
                wrapper.capture_matte_plate()
        except ValueError:
            self.refused()
        try:
            if adapt is None:
                wrapper.clear_matte_key_adapt()
            elif adapt is not self._NOTHING:
                wrapper.set_matte_key_adapt(**adapt)
        except ValueError:                         # (no key, or a colour key)
            self.refused()
        try:
            if gain is None:
                wrapper.clear_matte_key_gain()
            elif gain is not self._NOTHING:
                wrapper.set_matte_key_gain(**gain)
        except ValueError:                         # (no key, or a colour key)
            self.refused()
        self.current = self.view(wrapper.matte_key, getattr(wrapper, "matte_key_adapt", None))
        if want_gain:
            info = getattr(wrapper, "matte_key_gain", None)     # (None: off -- the request stays unanswered, the route says 404)
            if info is not None:
                try:
                    g, share = wrapper.matte_key_gain_measured()
                    info = dict(info, gain=list(g), share=list(share))
                except ValueError:                 # (no frame has been keyed under it yet)
                    info = dict(info, gain=None, share=None)
            with self._plate_ready:
                self._gain_info = info
                self._plate_ready.notify_all()
        if want_plate:
            try:
                plate = wrapper.matte_key_plate()
            except ValueError:                     # (no plate at this moment: the request stays unanswered, the route says 404)
                plate = None
            with self._plate_ready:
                self._plate = plate
                self._plate_ready.notify_all()


def parse_matte_edge_arg(text: str):
    """`R[,EPS]` -> the keywords of `wrapper.set_matte_edge`, `off` -> None; ValueError otherwise"""
    from live2diff_amd.matte import MAX_EDGE_RADIUS, check_edge
    text = text.strip()
    if text == "off":
        return None
    parts = [t.strip() for t in text.split(",")]
    if not 1 <= len(parts) <= 2:
        raise ValueError(f"matte edge {text!r}: use R[,EPS] or off")
    try:
        radius = int(parts[0])
        eps = float(parts[1]) if len(parts) > 1 else 10.0
    except ValueError:
        raise ValueError(f"matte edge {text!r}: R is an integer from 1 to {MAX_EDGE_RADIUS}, EPS a number of byte levels, at least "
                         "1") from None
    return check_edge(radius, eps)


class MatteEdgeBox:
    """What `POST /matte-edge` delivers: the newest requested edge setting (a dict of `set_matte_edge` keywords, or None for
    `off`), applied by the producer between two frames.  `current` is what was last applied; `failed` counts requests the wrapper
    refused."""
    _NOTHING = object()

    def __init__(self, current=None):
        self._lock = threading.Lock()
        self.current, self._want, self.failed = current, self._NOTHING, 0

    def put(self, settings) -> None:
        with self._lock:
            self._want = settings

    def apply(self, wrapper) -> None:
        """(producer thread, between frames)"""
        with self._lock:
            want, self._want = self._want, self._NOTHING
        if want is self._NOTHING:
            return
        try:
            if want is None:
                wrapper.clear_matte_edge()
            else:
                wrapper.set_matte_edge(want["radius"], want["eps"])
            self.current = wrapper.matte_edge
        except ValueError:
            self.failed += 1


def parse_detail_arg(text: str):
    """`R[,EPS[,STRENGTH[,LIMIT]]]` -> the keywords of `wrapper.set_detail`, `off` -> None; ValueError otherwise"""
    from live2diff_amd.detail import MAX_RADIUS, check_settings
    text = text.strip()
    if text == "off":
        return None
    parts = [t.strip() for t in text.split(",")]
    if not 1 <= len(parts) <= 4:
        raise ValueError(f"detail {text!r}: use R[,EPS[,STRENGTH[,LIMIT]]] or off")
    try:
        radius = int(parts[0])
        eps, strength, limit = (float(parts[i]) if len(parts) > i else d for i, d in ((1, 2.0), (2, 1.0), (3, 64.0)))
    except ValueError:
        raise ValueError(f"detail {text!r}: R is an integer from 1 to {MAX_RADIUS}, EPS (at least 1), STRENGTH (0..4) and LIMIT "
                         "(0..255) are numbers") from None
    return check_settings(radius, eps, strength, limit)


class DetailBox:
    """What `POST /detail` delivers: the newest requested detail setting (a dict of `set_detail` keywords, or None for `off`),
    applied by the producer between two frames.  `current` is what was last applied; `failed` counts requests the wrapper
    refused."""
    _NOTHING = object()

    def __init__(self, current=None):
        self._lock = threading.Lock()
        self.current, self._want, self.failed = current, self._NOTHING, 0

    def put(self, settings) -> None:
        with self._lock:
            self._want = settings

    def apply(self, wrapper) -> None:
        """(producer thread, between frames)"""
        with self._lock:
            want, self._want = self._want, self._NOTHING
        if want is self._NOTHING:
            return
        try:
            if want is None:
                wrapper.clear_detail()
            else:
                wrapper.set_detail(**want)
            self.current = wrapper.detail
        except ValueError:
            self.failed += 1


def parse_backdrop_arg(text: str):
    """`blur[,R[,PASSES]]`, `RRGGBB` (six hex digits) or the path of an image file -> the keywords of `wrapper.set_backdrop`; `off`
    or nothing -> None; ValueError otherwise.  The file is decoded here (`to` is its uint8 [H,W,3] array), so one that is no
    image is refused by the option before anything is loaded and by `POST /backdrop` with a 400."""
    from live2diff_amd.backdrop import MAX_PASSES, MAX_RADIUS, check_settings, load_image
    text = text.strip()
    if text in ("", "off"):
        return None
    parts = [t.strip() for t in text.split(",")]
    if parts[0] == "blur":
        if len(parts) > 3:
            raise ValueError(f"backdrop {text!r}: use blur[,R[,PASSES]], RRGGBB, the path of an image, or off")
        try:
            radius, passes = (int(parts[i]) if len(parts) > i else d for i, d in ((1, 6), (2, 3)))
        except ValueError:
            raise ValueError(f"backdrop {text!r}: R is an integer from 1 to {MAX_RADIUS}, PASSES one from 1 to {MAX_PASSES}") from None
        s = check_settings("blur", radius, passes)
        return dict(to="blur", radius=s["radius"], passes=s["passes"])
    if len(text) == 6 and all(c in "0123456789abcdefABCDEF" for c in text):
        return dict(to=tuple(int(text[i:i + 2], 16) for i in (0, 2, 4)))
    if not os.path.isfile(text):
        raise ValueError(f"backdrop {text!r}: use blur[,R[,PASSES]], RRGGBB, the path of an image, or off (there is no such file)")
    return dict(to=load_image(text))


class BackdropBox:
    """What `POST /backdrop` delivers: the newest requested backdrop (a dict of `set_backdrop` keywords, or None for an empty body
    or `off`), applied by the producer between two frames.  `current` is what was last applied (the `backdrop` property);
    `failed` counts requests the wrapper refused."""
    _NOTHING = object()

    def __init__(self, current=None):
        self._lock = threading.Lock()
        self.current, self._want, self.failed = current, self._NOTHING, 0

    def put(self, settings) -> None:
        with self._lock:
            self._want = settings

    def apply(self, wrapper) -> None:
        """(producer thread, between frames)"""
        with self._lock:
            want, self._want = self._want, self._NOTHING
        if want is self._NOTHING:
            return
        try:
            if want is None:
                wrapper.clear_backdrop()
            else:
                wrapper.set_backdrop(**want)
            self.current = wrapper.backdrop
        except ValueError:                         # (a file that is no image among them: `set_backdrop` decodes it)
            self.failed += 1


def parse_size_arg(text: str):
    """`WxH[,FILTER]` -> the keywords of `wrapper.set_output_size`, `off` -> None; ValueError otherwise (the wrapper, which knows
    the stream's size, checks the ratio once more)"""
    from live2diff_amd.resize import MAX_SIZE, check_filter, check_jpeg_size
    text = text.strip()
    if text == "off":
        return None
    size, comma, resample = text.partition(",")
    w, x, h = size.strip().lower().partition("x")
    try:
        if not x or (comma and not resample.strip()):
            raise ValueError
        width, height = int(w), int(h)
    except ValueError:
        raise ValueError(f"output size {text!r}: use WxH[,FILTER] (two integers, then lanczos, bicubic or bilinear) or off") from None
    if not (1 <= width <= MAX_SIZE and 1 <= height <= MAX_SIZE):
        raise ValueError(f"output size {text!r}: W and H lie in 1..{MAX_SIZE}")
    check_jpeg_size(height, width)
    return dict(height=height, width=width, resample=check_filter(resample.strip() if comma else "lanczos"))


class SizeBox:
    """What `POST /size` delivers: the newest requested output size (a dict of `set_output_size` keywords, or None for `off`),
    applied by the producer between two frames.  `current` is what was last applied; `failed` counts requests the wrapper refused."""
    _NOTHING = object()

    def __init__(self, current=None):
        self._lock = threading.Lock()
        self.current, self._want, self.failed = current, self._NOTHING, 0

    def put(self, settings) -> None:
        with self._lock:
            self._want = settings

    def apply(self, wrapper) -> None:
        """(producer thread, between frames)"""
        with self._lock:
            want, self._want = self._want, self._NOTHING
        if want is self._NOTHING:
            return
        try:
            if want is None:
                wrapper.clear_output_size()
            else:
                wrapper.set_output_size(want["height"], want["width"], resample=want["resample"])
            self.current = wrapper.output_size
        except ValueError:
            self.failed += 1


def parse_matte_source_arg(text: str) -> str:
    """`stream` or `camera` -> the argument of `wrapper.set_matte_source`; ValueError otherwise"""
    text = text.strip()
    if text not in ("stream", "camera"):
        raise ValueError(f"matte source {text!r}: use stream or camera")
    return text


class MatteSourceBox:
    """What `POST /matte-source` delivers: the newest requested source (`stream` or `camera`), applied by the producer between two
    frames.  `current` is what was last applied; `failed` counts requests the wrapper refused."""
    _NOTHING = object()

    def __init__(self, current="stream"):
        self._lock = threading.Lock()
        self.current, self._want, self.failed = current, self._NOTHING, 0

    def put(self, source) -> None:
        with self._lock:
            self._want = source

    def apply(self, wrapper) -> None:
        """(producer thread, between frames)"""
        with self._lock:
            want, self._want = self._want, self._NOTHING
        if want is self._NOTHING:
            return
        try:
            wrapper.set_matte_source(want)
            self.current = wrapper.matte_source
        except ValueError:
            self.failed += 1


def parse_style_arg(text: str):
    """`NAME=DREAMBOOTH[,LORA:ALPHA...]` -> (name, dreambooth path or None, {lora path: alpha})"""
    name, eq, rest = text.partition("=")
    if not eq or not name:
        raise ValueError(f"--style {text!r}: use NAME=DREAMBOOTH[,LORA:ALPHA...]")
    db, *loras = rest.split(",")
    lora_dict = {}
    for item in loras:
        path, colon, alpha = item.rpartition(":")
        if not colon or not path:
            raise ValueError(f"--style {text!r}: a LoRA is written LORA:ALPHA, got {item!r}")
        lora_dict[path] = float(alpha)
    if not db and not lora_dict:
        raise ValueError(f"--style {text!r}: names neither a DreamBooth file nor a LoRA")
    return name, (db or None), lora_dict


class Latest:
    """The newest part and its sequence number.  `put` replaces it; `wait(seen)` blocks until there is a part newer than `seen`
    and returns `(seq, part)`, or None once the stream is closed and nothing newer is left."""

    def __init__(self):
        self._cond = threading.Condition()
        self._seq, self._part, self._closed = 0, None, False

    def put(self, part: bytes) -> None:
        with self._cond:
            self._seq, self._part = self._seq + 1, part
            self._cond.notify_all()

    def close(self) -> None:
        with self._cond:
            self._closed = True
            self._cond.notify_all()

    def wait(self, seen: int):
        with self._cond:
            self._cond.wait_for(lambda: self._seq > seen or self._closed)
            return (self._seq, self._part) if self._seq > seen else None


def make_handler(latest: Latest, inbox: "Inbox" = None, styles: "StyleBox" = None, mattes: "MatteBox" = None, colors: "ColorBox" = None,
                 sizes: "SizeBox" = None, sources: "MatteSourceBox" = None, steadies: "SteadyBox" = None, details: "DetailBox" = None,
                 backdrops: "BackdropBox" = None, follows: "SteadyFollowBox" = None, holds: "MatteHoldBox" = None,
                 masks: "MaskBox" = None, keys: "MatteKeyBox" = None, edges: "MatteEdgeBox" = None):
    # (The cut detector's box rides with the styles' box, as the re-warm's requests do: tests pin `edges` as the last parameter of
    # this function and of the two producers.  It is the one the `StyleBox` was built with.)
    cuts = styles.cuts if styles is not None else None
    boxes = {"/matte-key": keys, "/matte": mattes, "/color": colors, "/size": sizes, "/matte-source": sources, "/steady": steadies, "/matte-edge": edges,
             "/detail": details, "/backdrop": backdrops, "/steady-follow": follows, "/matte-hold": holds}
    page = PAGE if inbox is None else CAMERA_PAGE

    class Handler(BaseHTTPRequestHandler):
        protocol_version = "HTTP/1.0"          # no keep-alive: the stream ends when either side closes the connection

        def log_message(self, fmt, *args):     # (one line per request on stderr is noise beside a 70 fps stream)
            pass

        def do_GET(self):
            if self.path in ("/", "/index.html"):
                self.send_response(200)
                self.send_header("Content-Type", "text/html; charset=utf-8")
                self.send_header("Content-Length", str(len(page)))
                self.end_headers()
                self.wfile.write(page)
            elif self.path == "/stream":
                self.send_response(200)
                self.send_header("Content-Type", "multipart/x-mixed-replace; boundary=frame")
                self.send_header("Cache-Control", "no-store")
                self.end_headers()
                seen = 0
                try:
                    while True:
                        got = latest.wait(seen)
                        if got is None:
                            break
                        seen, part = got
                        self.wfile.write(part)
                        self.wfile.flush()
                except (BrokenPipeError, ConnectionResetError):
                    pass                       # the viewer went away
            elif self.path == "/style" and styles is not None:
                body = json.dumps({"styles": styles.names, "current": styles.current}).encode()
                self.send_response(200)
                self.send_header("Content-Type", "application/json")
                self.send_header("Content-Length", str(len(body)))
                self.end_headers()
                self.wfile.write(body)
            elif self.path == "/rewarm" and styles is not None:
                body = json.dumps({"rewarms": styles.rewarms, "failed": styles.rewarm_failed}).encode()
                self.send_response(200)
                self.send_header("Content-Type", "application/json")
                self.send_header("Content-Length", str(len(body)))
                self.end_headers()
                self.wfile.write(body)
            elif cuts is not None and self.path in ("/cuts", "/cut-detect", "/auto-rewarm"):
                body = json.dumps(cuts.report if self.path == "/cuts" else cuts.current if self.path == "/cut-detect" else cuts.auto).encode()
                self.send_response(200)
                self.send_header("Content-Type", "application/json")
                self.send_header("Cache-Control", "no-store")
                self.send_header("Content-Length", str(len(body)))
                self.end_headers()
                self.wfile.write(body)
            elif self.path == "/matte-key/plate" and keys is not None:
                plate = keys.take_plate()
                if plate is None:
                    self.send_error(404, "no plate at this moment (no key against a plate, a capture that waits, or no stream)")
                    return
                import io

                from PIL import Image
                buf = io.BytesIO()
                Image.fromarray(plate).save(buf, "JPEG", quality=90)
                body = buf.getvalue()
                self.send_response(200)
                self.send_header("Content-Type", "image/jpeg")
                self.send_header("Cache-Control", "no-store")
                self.send_header("Content-Length", str(len(body)))
                self.end_headers()
                self.wfile.write(body)
            elif self.path == "/matte-key/gain" and keys is not None:
                info = keys.take_gain()
                if info is None:
                    self.send_error(404, "no plate gain at this moment (--matte-key-gain / POST /matte-key/gain is off, or no stream)")
                    return
                body = json.dumps(info).encode()
                self.send_response(200)
                self.send_header("Content-Type", "application/json")
                self.send_header("Cache-Control", "no-store")
                self.send_header("Content-Length", str(len(body)))
                self.end_headers()
                self.wfile.write(body)
            elif boxes.get(self.path) is not None or (masks is not None and self.path in ("/mask", "/mask-input")):
                current = (boxes[self.path].current if self.path in boxes else
                           masks.current if self.path == "/mask" else masks.current_input)
                body = json.dumps(current).encode()
                self.send_response(200)
                self.send_header("Content-Type", "application/json")
                self.send_header("Content-Length", str(len(body)))
                self.end_headers()
                self.wfile.write(body)
            else:
                self.send_error(404)

        def do_matte(self, box=None, parse=parse_matte_arg, empty=False):
            box = mattes if box is None else box
            try:
                n = int(self.headers.get("Content-Length", ""))
            except ValueError:
                self.send_error(411)
                return
            if n == 0 and empty:                          # (`/backdrop`, `/steady-follow`: an empty body clears it)
                box.put(None)
                self.send_response(204)
                self.end_headers()
                return
            if not 1 <= n <= 256:
                self.send_error(413 if n > 256 else 400)
                return
            try:
                want = parse(self.rfile.read(n).decode())
            except ValueError as e:                       # (UnicodeDecodeError is a ValueError)
                self.send_error(400, str(e.args[0] if e.args else e)[:200])
                return
            box.put(want)
            self.send_response(204)
            self.end_headers()

        def do_mask(self):
            try:
                n = int(self.headers.get("Content-Length", ""))
            except ValueError:
                self.send_error(411)
                return
            if not 0 <= n <= MAX_POST:
                self.send_error(413 if n > MAX_POST else 400)
                return
            body = self.rfile.read(n) if n else b""
            try:
                if len(body) != n:
                    raise ValueError("the body is shorter than its Content-Length")
                if self.path == "/mask":
                    masks.put(parse_mask_body(body))
                else:
                    masks.put_input(parse_mask_input_arg(body.decode()))
            except ValueError as e:                       # (UnicodeDecodeError is a ValueError)
                masks.refused()
                self.send_error(400, str(e.args[0] if e.args else e)[:200])
                return
            self.send_response(204)
            self.end_headers()

        def do_matte_key(self):
            try:
                n = int(self.headers.get("Content-Length", ""))
            except ValueError:
                self.send_error(411)
                return
            capture = self.path == "/matte-key/capture"
            if not 0 <= n <= 256:
                self.send_error(413 if n > 256 else 400)
                return
            body = self.rfile.read(n) if n else b""
            try:
                if len(body) != n:
                    raise ValueError("the body is shorter than its Content-Length")
                if capture:
                    if body.strip():
                        raise ValueError("POST /matte-key/capture takes no body")
                    keys.capture()
                elif self.path == "/matte-key/adapt":
                    keys.put_adapt(parse_matte_key_adapt_arg(body.decode()))
                elif self.path == "/matte-key/gain":
                    keys.put_gain(parse_matte_key_gain_arg(body.decode()))
                else:
                    keys.put(parse_matte_key_arg(body.decode()))
            except ValueError as e:                       # (UnicodeDecodeError is a ValueError)
                keys.refused()
                self.send_error(400, str(e.args[0] if e.args else e)[:200])
                return
            self.send_response(204)
            self.end_headers()

        def do_style(self):
            from live2diff_amd.style_bank import parse_style
            try:
                n = int(self.headers.get("Content-Length", ""))
            except ValueError:
                self.send_error(411)
                return
            if not 2 <= n <= 4096:
                self.send_error(413 if n > 4096 else 400)
                return
            try:
                req = json.loads(self.rfile.read(n).decode())
                rewarm = parse_style_rewarm(req.pop("rewarm")) if isinstance(req, dict) and "rewarm" in req else False
                if rewarm == "recent" and not styles.keep_recent:
                    raise ValueError('"rewarm": "recent" needs a server started with --keep-recent')
                mix = parse_style(req, styles.names)
            except (KeyError, ValueError) as e:           # (json.JSONDecodeError and UnicodeDecodeError are ValueErrors)
                self.send_error(400, str(e.args[0] if e.args else e)[:200])
                return
            if rewarm:
                styles.put(mix, rewarm=rewarm)
            else:
                styles.put(mix)
            self.send_response(204)
            self.end_headers()

        def do_rewarm(self):
            try:
                n = int(self.headers.get("Content-Length", ""))
            except ValueError:
                self.send_error(411)
                return
            if not 2 <= n <= 256:
                self.send_error(413 if n > 256 else 400)
                return
            try:
                styles.put_rewarm(parse_rewarm_body(self.rfile.read(n)))
            except ValueError as e:
                self.send_error(400, str(e.args[0] if e.args else e)[:200])
                return
            self.send_response(204)
            self.end_headers()

        def do_cut(self):
            try:
                n = int(self.headers.get("Content-Length", ""))
            except ValueError:
                self.send_error(411)
                return
            if not 1 <= n <= 256:
                self.send_error(413 if n > 256 else 400)
                return
            try:
                text = self.rfile.read(n).decode()
                if self.path == "/cut-detect":
                    cuts.put(parse_cut_detect_arg(text))
                else:
                    cuts.put_auto(parse_auto_rewarm_arg(text))
            except ValueError as e:                       # (UnicodeDecodeError is a ValueError)
                self.send_error(400, str(e.args[0] if e.args else e)[:200])
                return
            self.send_response(204)
            self.end_headers()

        def do_POST(self):
            if self.path == "/style" and styles is not None:
                self.do_style()
                return
            if cuts is not None and self.path in ("/cut-detect", "/auto-rewarm"):
                self.do_cut()
                return
            if self.path == "/rewarm" and styles is not None:
                self.do_rewarm()
                return
            if self.path == "/matte" and mattes is not None:
                self.do_matte()
                return
            if self.path == "/color" and colors is not None:
                self.do_matte(colors, parse_color_arg)
                return
            if self.path == "/size" and sizes is not None:
                self.do_matte(sizes, parse_size_arg)
                return
            if self.path == "/matte-source" and sources is not None:
                self.do_matte(sources, parse_matte_source_arg)
                return
            if self.path == "/steady" and steadies is not None:
                self.do_matte(steadies, parse_steady_arg)
                return
            if self.path == "/matte-edge" and edges is not None:
                self.do_matte(edges, parse_matte_edge_arg)
                return
            if self.path == "/steady-follow" and follows is not None:
                self.do_matte(follows, parse_steady_follow_arg, empty=True)
                return
            if self.path == "/matte-hold" and holds is not None:
                self.do_matte(holds, parse_matte_hold_arg, empty=True)
                return
            if self.path == "/detail" and details is not None:
                self.do_matte(details, parse_detail_arg)
                return
            if self.path == "/backdrop" and backdrops is not None:
                self.do_matte(backdrops, parse_backdrop_arg, empty=True)
                return
            if masks is not None and self.path in ("/mask", "/mask-input"):
                self.do_mask()
                return
            if keys is not None and self.path in ("/matte-key", "/matte-key/capture", "/matte-key/adapt", "/matte-key/gain"):
                self.do_matte_key()
                return
            if inbox is None or self.path != "/frame":
                self.send_error(404)
                return
            try:
                n = int(self.headers.get("Content-Length", ""))
            except ValueError:
                self.send_error(411)
                return
            if not 2 <= n <= MAX_POST:
                self.send_error(413 if n > MAX_POST else 400)
                return
            body = self.rfile.read(n)
            if len(body) != n or body[:2] != b"\xff\xd8":
                self.send_error(400, "the body is no JPEG file")
                return
            inbox.put(body)
            self.send_response(204)
            self.end_headers()

    return Handler


def produce(wrapper, frames, latest: Latest, stop: threading.Event, styles: StyleBox = None, mattes: MatteBox = None,
            colors: ColorBox = None, sizes: SizeBox = None, sources: MatteSourceBox = None, steadies: SteadyBox = None,
            details: DetailBox = None, backdrops: BackdropBox = None, follows: SteadyFollowBox = None,
            holds: MatteHoldBox = None, masks: "MaskBox" = None, keys: "MatteKeyBox" = None, edges: MatteEdgeBox = None) -> None:
    """the producer: loops `frames` through the wrapper until `stop` is set; a posted style, re-warm, matte, colour lock, output size,
    matte source, steady mode, follow setting, matte edge, matte hold, detail mode, backdrop, mask, mask input, matte key, cut
    detector or automatic re-warm is applied between two frames"""
    from live2diff_amd.jpeg import mjpeg_part
    try:
        i = 0
        while not stop.is_set():
            if styles is not None:
                styles.apply(wrapper)
            if mattes is not None:
                mattes.apply(wrapper)
            if colors is not None:
                colors.apply(wrapper)
            if sizes is not None:
                sizes.apply(wrapper)
            if sources is not None:
                sources.apply(wrapper)
            if steadies is not None:
                steadies.apply(wrapper)
            if follows is not None:
                follows.apply(wrapper)
            if edges is not None:
                edges.apply(wrapper)
            if holds is not None:
                holds.apply(wrapper)
            if details is not None:
                details.apply(wrapper)
            if backdrops is not None:
                backdrops.apply(wrapper)
            if masks is not None:
                masks.apply(wrapper)
            if keys is not None:
                keys.apply(wrapper)
            latest.put(mjpeg_part(wrapper(frames[i % len(frames)])))
            i += 1
    finally:
        latest.close()


def produce_posted(wrapper, prompt: str, inbox: Inbox, latest: Latest, stop: threading.Event, styles: StyleBox = None,
                   mattes: MatteBox = None, colors: ColorBox = None, sizes: SizeBox = None, sources: MatteSourceBox = None,
                   steadies: SteadyBox = None, details: DetailBox = None, backdrops: BackdropBox = None,
                   follows: SteadyFollowBox = None, holds: "MatteHoldBox" = None,
                   masks: "MaskBox" = None, keys: "MatteKeyBox" = None, edges: MatteEdgeBox = None) -> None:
    """the producer of `--input post`: the first frames posted warm the stream up, then the newest posted frame goes through the
    wrapper, for ever; a frame the wrapper refuses (ValueError: a damaged file) is dropped and counted in `inbox.failed`"""
    from live2diff_amd.jpeg import mjpeg_part
    try:
        warm = inbox.warmup_frames()
        if warm is None:
            return
        wrapper.prepare(warm, prompt)
        while not stop.is_set():
            frame = inbox.take(timeout=0.5)
            if frame is None:
                continue
            if styles is not None:
                styles.apply(wrapper)
            if mattes is not None:
                mattes.apply(wrapper)
            if colors is not None:
                colors.apply(wrapper)
            if sizes is not None:
                sizes.apply(wrapper)
            if sources is not None:
                sources.apply(wrapper)
            if steadies is not None:
                steadies.apply(wrapper)
            if follows is not None:
                follows.apply(wrapper)
            if edges is not None:
                edges.apply(wrapper)
            if holds is not None:
                holds.apply(wrapper)
            if details is not None:
                details.apply(wrapper)
            if backdrops is not None:
                backdrops.apply(wrapper)
            if masks is not None:
                masks.apply(wrapper)
            if keys is not None:
                keys.apply(wrapper)
            try:
                latest.put(mjpeg_part(wrapper(frame)))
            except ValueError:
                inbox.failed += 1
    finally:
        latest.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--input", required=True, help="folder of images, or .npy uint8 [F,H,W,3]; looped -- or `post`: JPEG frames arrive as "
                    "bodies of POST /frame (the page captures the camera)")
    ap.add_argument("--prompt", default=None, help="default: the config's `prompt`")
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--port", type=int, default=8000)
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--engine-dir", default="engines")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--style", action="append", default=[], metavar="NAME=DREAMBOOTH[,LORA:ALPHA...]",
                    help="register a further style (repeatable); POST /style {name: weight} switches or blends between frames")
    ap.add_argument("--keep-recent", action="store_true",
                    help="keep the last frames' latents on the device (two small copies per frame): POST /rewarm {\"source\": \"recent\"} "
                         "and \"rewarm\": \"recent\" in POST /style re-warm the sinks on them")
    ap.add_argument("--cut-detect", default=None, nargs="?", const="on", metavar="THUMB,HIST[,RATIO[,GAP]]",
                    help="find scene cuts on the device: a frame is a cut when its 8 x 8 block luma moved by THUMB byte levels on average "
                         "(default 20) and HIST of its pixels changed histogram bin (default 0.35) and it moved RATIO times as far as the "
                         "frames before (default 3; 0: no such test), GAP frames (default 8) behind a cut none is reported -- defaults that "
                         "are a guess, untuned on footage; POST /cut-detect with the same text, `on` or `off` changes it between two "
                         "frames; GET /cuts answers the cuts found")
    ap.add_argument("--auto-rewarm", action="store_true",
                    help="re-warm the sinks by themselves once the last frames all lie behind a cut (implies --keep-recent; needs "
                         "--cut-detect or a POST /cut-detect); POST /auto-rewarm with `on` or `off` switches it between two frames")
    ap.add_argument("--matte", default=None, metavar="LO,HI[,FEATHER[,far]]",
                    help="stylise only the near (`far`: the far) side of a depth ramp from LO to HI in [0, 1], 1 = nearest; POST /matte "
                         "with the same text, or `off`, changes it between frames")
    ap.add_argument("--color-lock", default=None, metavar="source|ema[,STRENGTH[,RATE]]",
                    help="hold the output's per-channel brightness and contrast to the source frame's (`source`) or to a running average "
                         "of the stream's own (`ema`); POST /color with the same text, or `off`, changes it between frames")
    ap.add_argument("--output-size", default=None, metavar="WxH[,FILTER]",
                    help="serve frames of W x H pixels (multiples of 16, W <= 1920) resampled on the device with lanczos (default), "
                         "bicubic or bilinear; POST /size with the same text, or `off`, changes it between frames")
    ap.add_argument("--matte-source", default="stream", type=parse_matte_source_arg, metavar="stream|camera",
                    help="what a matte keeps real under an output size: the UNet-sized source frame (`stream`) or the input frame's own "
                         "pixels at the output size (`camera`); POST /matte-source with one of the two words changes it between frames")
    ap.add_argument("--steady", default=None, metavar="LO,HI[,STRENGTH[,RADIUS]]",
                    help="hold the previous output pixel where the source moved by LO byte levels or less (moving from HI on), by "
                         "STRENGTH (default 0.8), the motion averaged over a radius of RADIUS pixels (default 2); POST /steady with "
                         "the same text, or `off`, changes it between frames")
    ap.add_argument("--steady-follow", default=None, metavar="R[,BIAS]",
                    help="let the steady mode follow the source's motion: every 8 x 8 block is matched against the frame before over "
                         "displacements of up to R pixels (1..8); BIAS (default 256, 0..4096) keeps noise in flat areas from producing "
                         "vectors; acts while --steady is set; POST /steady-follow with the same text changes it between frames, an "
                         "empty body (or `off`) clears it")
    ap.add_argument("--matte-hold", default=None, metavar="LO,HI[,STRENGTH[,RADIUS[,SEARCH[,BIAS]]]]",
                    help="keep the matte still where the source moved by LO byte levels or less (moving from HI on), by STRENGTH "
                         "(default 0.8), the motion averaged over a radius of RADIUS pixels (default 2); SEARCH 1..8 (default 0: the "
                         "same coordinates) follows the source's motion, with BIAS (default 256); acts while --matte is set; POST "
                         "/matte-hold with the same text changes it between frames, an empty body (or `off`) clears it")
    ap.add_argument("--matte-edge", default=None, metavar="R[,EPS]",
                    help="refine the matte by the frame it cuts (a guided filter of radius R, 1..8 pixels; EPS, default 10: the contrast in "
                         "byte levels below which a window counts as flat); acts while a matte is set; POST /matte-edge with the same "
                         "text, or `off`, changes it between frames")
    ap.add_argument("--detail", default=None, metavar="R[,EPS[,STRENGTH[,LIMIT]]]",
                    help="bring the camera's fine detail into the frame at the output size (windows of radius R, 1..8 pixels; EPS, default "
                         "2: the contrast in byte levels below which a window counts as flat; STRENGTH, default 1; LIMIT, default 64 byte "
                         "levels); acts while an output size is set; POST /detail with the same text, or `off`, changes it between frames")
    ap.add_argument("--backdrop", default=None, metavar="blur[,R[,PASSES]]|RRGGBB|PATH",
                    help="what stands behind the matte in place of the real frame: the room blurred with the subject left out (PASSES "
                         "boxes of radius R, defaults 6 and 3), a colour as six hex digits, or an image file; acts while a matte is set; "
                         "POST /backdrop with the same text changes it between frames, an empty body (or `off`) clears it")
    ap.add_argument("--mask", default=None, metavar="PATH",
                    help="a sticky mask: an image (mode L, 1, I;16 or F, any size) that cuts every frame in place of the depth ramp, or "
                         "combined with it (--mask-input); needs --matte; POST /mask with an image file as its body replaces it between "
                         "frames, an empty body (or `off`) clears it")
    ap.add_argument("--matte-key", default=None, metavar="RRGGBB|PATH|capture[,LO,HI[,LUMA[,RADIUS[,COMBINE[,invert]]]]]",
                    help="cut the frame by a colour (a green screen), by a clean plate (an image of the empty room) or by a plate "
                         "captured from the stream's next output; needs --matte; POST /matte-key with the same text changes it "
                         "between two frames, `off` clears it, POST /matte-key/capture takes the plate again")
    ap.add_argument("--matte-key-adapt", default=None, metavar="RATE[,ABSORB]",
                    help="let the plate of --matte-key follow drifting light: it moves by RATE of the way towards each frame where the key "
                         "says background, by ABSORB (default 0) where it says subject, both in [0, 0.5]; needs a --matte-key against a "
                         "plate (a path or capture); POST /matte-key/adapt with the same text changes it between two frames, `off` clears "
                         "it; GET /matte-key/plate answers the plate of this moment as a JPEG")
    ap.add_argument("--matte-key-gain", default=None, nargs="?", const="on", metavar="LIMIT[,MIN_SHARE]",
                    help="let --matte-key against a plate follow a sudden exposure or white-balance step: every frame measures one gain "
                         "per channel between the plate and the frame (the median over the frame) and is keyed against the plate times "
                         "it; LIMIT in [1, 3.99] (default 2) bounds the gain, MIN_SHARE in [0, 1] (default 1/16) is the part of the frame "
                         "a channel needs as valid samples; POST /matte-key/gain with the same text changes it between two frames, `off` "
                         "clears it; GET /matte-key/gain answers the setting and the last measurement")
    ap.add_argument("--mask-input", default=None, metavar="COMBINE[,invert]",
                    help="how a mask meets the depth ramp: replace (default), and, or; `invert` flips the mask first; POST /mask-input "
                         "with the same text changes it between frames")
    args = ap.parse_args(argv)
    if args.auto_rewarm:
        args.keep_recent = True
    try:
        cut_detect = parse_cut_detect_arg(args.cut_detect) if args.cut_detect else None
    except ValueError as e:
        ap.error("--cut-detect: " + str(e))
    if args.auto_rewarm and cut_detect is None:
        ap.error("--auto-rewarm needs --cut-detect")
    ap_key = args.matte_key
    if ap_key is not None and not args.matte:
        ap.error("--matte-key needs --matte (its feather and `far` act on the key)")
    if ap_key is not None and args.mask is not None:
        ap.error("--matte-key and --mask exclude each other")
    try:
        matte_key = parse_matte_key_arg(ap_key) if ap_key else None
    except ValueError as e:
        ap.error(str(e))
    ap_adapt = args.matte_key_adapt
    if ap_adapt is not None and (matte_key is None or isinstance(matte_key["to"], tuple)):
        ap.error("--matte-key-adapt needs a --matte-key against a plate (a path or capture), not a colour")
    try:
        matte_key_adapt = parse_matte_key_adapt_arg(ap_adapt) if ap_adapt else None
    except ValueError as e:
        ap.error(str(e))
    ap_gain = args.matte_key_gain
    if ap_gain is not None and (matte_key is None or isinstance(matte_key["to"], tuple)):
        ap.error("--matte-key-gain needs a --matte-key against a plate (a path or capture), not a colour")
    try:
        matte_key_gain = parse_matte_key_gain_arg(ap_gain) if ap_gain else None
    except ValueError as e:
        ap.error(str(e))
    if args.mask is not None and not args.matte:
        ap.error("--mask needs --matte (its feather and `far` act on the mask)")
    mask_input = parse_mask_input_arg(args.mask_input) if args.mask_input else None
    style_args = [parse_style_arg(t) for t in args.style]
    matte = parse_matte_arg(args.matte) if args.matte else None
    color = parse_color_arg(args.color_lock) if args.color_lock else None
    size = parse_size_arg(args.output_size) if args.output_size else None
    steady = parse_steady_arg(args.steady) if args.steady else None
    follow = parse_steady_follow_arg(args.steady_follow) if args.steady_follow else None
    edge = parse_matte_edge_arg(args.matte_edge) if args.matte_edge else None
    hold = parse_matte_hold_arg(args.matte_hold) if args.matte_hold else None
    detail = parse_detail_arg(args.detail) if args.detail else None
    backdrop = parse_backdrop_arg(args.backdrop) if args.backdrop else None

    from stream_frames import read_frames

    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper, load_config, stream_sizes
    cfg = load_config(args.config)
    sink = stream_sizes(cfg)[1]
    post = args.input == "post"
    frames = None if post else read_frames(args.input)
    if not post and len(frames) < sink:
        raise ValueError(f"{len(frames)} frames: need at least the {sink} warm-up frames")
    w = StreamAnimateDiffusionDepthWrapper(args.config, few_step_model_type="lcm", num_inference_steps=cfg.get("num_inference_steps", 50),
                                           t_index_list=cfg.get("t_index_list"), strength=cfg.get("strength"), output_type="jpeg",
                                           jpeg_quality=args.quality, height=args.height, width=args.width, seed=args.seed,
                                           engine_dir=args.engine_dir, output_size=size and (size["height"], size["width"]),
                                           output_resample=size["resample"] if size else "lanczos", matte_source=args.matte_source,
                                           keep_recent=args.keep_recent)
    for name, db, loras in style_args:
        w.add_style(name, dreambooth_path=db, lora_dict=loras or None)
    if cut_detect is not None:
        w.set_cut_detect(**cut_detect)
    if args.auto_rewarm:
        w.set_auto_rewarm(True)
    styles = StyleBox(w.styles, w.style, keep_recent=args.keep_recent,
                      cuts=CutBox(w.cut_detect, w.auto_rewarm, keep_recent=args.keep_recent))
    if matte is not None:
        w.set_matte(matte["lo"], matte["hi"], keep=matte["keep"], feather=matte["feather"])      # (before `prepare`: the line is primed)
    mattes = MatteBox(w.matte)
    if color is not None:
        w.set_color_lock(color["to"], strength=color["strength"], rate=color["rate"])        # (before `prepare`, like the matte)
    colors = ColorBox(w.color_lock)
    sizes = SizeBox(w.output_size)
    sources = MatteSourceBox(w.matte_source)
    if steady is not None:
        w.set_steady(steady["lo"], steady["hi"], strength=steady["strength"], radius=steady["radius"])      # (before `prepare` too)
    steadies = SteadyBox(w.steady)
    if follow is not None:
        w.set_steady_follow(follow["search"], follow["bias"])
    follows = SteadyFollowBox(w.steady_follow)
    if edge is not None:
        w.set_matte_edge(edge["radius"], edge["eps"])
    edges = MatteEdgeBox(w.matte_edge)
    if hold is not None:
        w.set_matte_hold(hold["lo"], hold["hi"], strength=hold["strength"], radius=hold["radius"], search=hold["search"], bias=hold["bias"])
    holds = MatteHoldBox(w.matte_hold)
    if detail is not None:
        w.set_detail(**detail)               # (before `prepare`: the line is primed, the first frames carry their camera frame)
    details = DetailBox(w.detail)
    if backdrop is not None:
        w.set_backdrop(**backdrop)
    backdrops = BackdropBox(w.backdrop)
    if mask_input is not None:
        w.set_mask_input(**mask_input)
    mask_size = None
    if args.mask is not None:
        from live2diff_amd.mask_io import _as_mask, load
        sticky = _as_mask(load(args.mask, "--mask"))
        w.set_mask(sticky)                   # (before `prepare`: the primed positions of the delay line carry it)
        mask_size = dict(size=[int(sticky.shape[0]), int(sticky.shape[1])])
    masks = MaskBox(mask_size, w.mask_input)
    if matte_key is not None:
        w.set_matte_key(**matte_key)
    if matte_key_adapt is not None:
        w.set_matte_key_adapt(**matte_key_adapt)
    if matte_key_gain is not None:
        w.set_matte_key_gain(**matte_key_gain)
    keys = MatteKeyBox(w.matte_key, w.matte_key_adapt)
    prompt = args.prompt if args.prompt is not None else str(cfg.get("prompt", ""))
    latest, stop = Latest(), threading.Event()
    inbox = Inbox(sink) if post else None
    if post:
        producer = threading.Thread(target=produce_posted, args=(w, prompt, inbox, latest, stop, styles, mattes, colors, sizes, sources, steadies, details, backdrops, follows, holds, masks, keys, edges), name="producer", daemon=True)
    else:
        w.prepare(frames[:sink], prompt)
        producer = threading.Thread(target=produce, args=(w, frames, latest, stop, styles, mattes, colors, sizes, sources, steadies, details, backdrops, follows, holds, masks, keys, edges), name="producer", daemon=True)
    server = ThreadingHTTPServer((args.host, args.port), make_handler(latest, inbox, styles, mattes, colors, sizes, sources, steadies, details, backdrops, follows, holds, masks, keys, edges))
    server.daemon_threads = True
    producer.start()
    print(f"http://{args.host}:{args.port}/  ({args.height}x{args.width}, quality {args.quality}; Ctrl-C stops)")
    try:
        server.serve_forever()
    except KeyboardInterrupt:
        pass
    finally:
        stop.set()
        if inbox is not None:
            inbox.close()
            print(f"{inbox.posted} frames posted, {inbox.replaced} replaced by a newer one before their turn, {inbox.failed} dropped as damaged")
        server.server_close()
        producer.join(timeout=10)


if __name__ == "__main__":
    main()
