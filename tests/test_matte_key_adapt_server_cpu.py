"""CPU test (-m "not gpu") of the adaptive plate's routes of tools/mjpeg_server.py: `--matte-key-adapt` / `POST /matte-key/adapt`
(`RATE[,ABSORB]`, `off`), `GET /matte-key` reporting it, `GET /matte-key/plate` (a JPEG, or 404), bodies that get a 400 and are
counted, and the producer applying the newest request between two frames."""
import io
import json
import os
import threading

import numpy as np
import pytest

from test_matte_key_server_cpu import ROOT, server
from test_style_bank_cpu import _request


def test_argument_parsing():
    S = server()
    assert S.parse_matte_key_adapt_arg("0.03125") == dict(rate=1 / 32, absorb=0.0)
    assert S.parse_matte_key_adapt_arg(" 0.25 , 0.0078125 ") == dict(rate=0.25, absorb=1 / 128)
    assert S.parse_matte_key_adapt_arg("0,0") == dict(rate=0.0, absorb=0.0) and S.parse_matte_key_adapt_arg("0.5,0.5") == dict(rate=0.5, absorb=0.5)
    assert S.parse_matte_key_adapt_arg("off") is None and S.parse_matte_key_adapt_arg("") is None
    for text in ("fast", "0.6", "-0.1", "0.1,0.6", "0.1,x", "0.1,0.1,0.1", "nan", ","):
        with pytest.raises(ValueError):
            S.parse_matte_key_adapt_arg(text)
    ap_text = open(os.path.join(ROOT, "tools", "mjpeg_server.py")).read()
    assert '"--matte-key-adapt"' in ap_text and "parse_matte_key_adapt_arg(ap_adapt)" in ap_text
    # the grammar of --matte-key stays as it is
    assert S.parse_matte_key_arg("capture,20,60") == dict(lo=20.0, hi=60.0, luma=0.25, radius=1, combine="replace", invert=False, to="capture")


def test_routes_refusals_and_the_producer():
    from PIL import Image
    S = server()
    plate = np.random.default_rng(2).integers(0, 256, (16, 24, 3), dtype=np.uint8)

    class W:
        """the producer's wrapper: echoes the frame, records the setting each frame ran under; posts from inside the loop"""
        matte_key = matte_key_adapt = None

        def __init__(self):
            self.seen, self.got = [], []

        def set_matte_key(self, to, **kw):
            self.matte_key = dict(kw, to=to)

        def clear_matte_key(self):
            self.matte_key = self.matte_key_adapt = None

        def set_matte_key_adapt(self, rate, absorb):
            if self.matte_key is None or isinstance(self.matte_key["to"], tuple):
                raise ValueError("set_matte_key_adapt: refused")
            self.matte_key_adapt = dict(rate=rate, absorb=absorb)

        def clear_matte_key_adapt(self):
            self.matte_key_adapt = None

        def matte_key_plate(self):
            if self.matte_key is None or self.matte_key["to"] != "plate":
                raise ValueError("matte_key_plate: no plate")
            return plate

        def __call__(self, frame):
            if self.matte_key is not None and self.matte_key["to"] == "capture":
                self.matte_key = dict(self.matte_key, to="plate")
            self.seen.append(None if self.matte_key_adapt is None else (self.matte_key_adapt["rate"], self.matte_key_adapt["absorb"]))
            n = len(self.seen)
            if n == 1:
                assert adapt(b"0.125").startswith(b"HTTP/1.0 204")                   # no key yet: the wrapper refuses it
                self.got.append(get_plate())                                         # and there is no plate
            elif n == 2:
                assert key(b"00b140").startswith(b"HTTP/1.0 204")
                assert adapt(b"0.125").startswith(b"HTTP/1.0 204")                   # a colour key: refused too
            elif n == 3:
                assert key(b"capture,20,60").startswith(b"HTTP/1.0 204")
                assert adapt(b"0.125").startswith(b"HTTP/1.0 204")
                assert adapt(b"0.25,0.015625").startswith(b"HTTP/1.0 204")           # the newest request wins
            elif n == 4:
                self.got.append(get_plate())                                         # asks; the producer hands it over behind this frame
            elif n == 5:
                self.got.append(get_plate())                                         # delivered
                assert adapt(b"off").startswith(b"HTTP/1.0 204")
            elif n == 6:
                assert adapt(b"0.5").startswith(b"HTTP/1.0 204")
            elif n == 7:
                assert adapt(b"").startswith(b"HTTP/1.0 204")                        # an empty body clears it
            elif n == 8:
                stop.set()
            return frame

    w = W()
    latest, stop = S.Latest(), threading.Event()
    keys = S.MatteKeyBox(w.matte_key, w.matte_key_adapt)
    keys.plate_wait = 0.0                        # (the producer runs in this thread: nothing could answer while a request waits)
    handler = S.make_handler(latest, keys=keys)
    key = lambda body: _request(handler, "POST", "/matte-key", body)
    adapt = lambda body: _request(handler, "POST", "/matte-key/adapt", body)
    get_plate = lambda: _request(handler, "GET", "/matte-key/plate")
    assert _request(S.make_handler(latest), "POST", "/matte-key/adapt", b"0.1").startswith(b"HTTP/1.0 404")
    assert _request(S.make_handler(latest), "GET", "/matte-key/plate").startswith(b"HTTP/1.0 404")
    assert _request(handler, "GET", "/matte-key/adapt").startswith(b"HTTP/1.0 404")
    assert _request(handler, "POST", "/matte-key/plate", b"").startswith(b"HTTP/1.0 404")
    for body in (b"fast", b"\xff\xfe", b"0.6", b"0.1,0.7", b"0.1,0.1,0.1"):
        assert adapt(body).startswith(b"HTTP/1.0 400"), body
    assert keys.failed == 5
    assert adapt(b"x" * 257).startswith(b"HTTP/1.0 413")
    S.produce(w, [b"\xff\xd8 a", b"\xff\xd8 b"], latest, stop, keys=keys)                # (in this thread)
    assert w.seen == [None, None, None, (0.25, 1 / 64), (0.25, 1 / 64), None, (0.5, 0.0), None]
    assert keys.failed == 7                      # the two requests the wrapper refused
    assert w.got[0].startswith(b"HTTP/1.0 404") and w.got[1].startswith(b"HTTP/1.0 404") and w.got[2].startswith(b"HTTP/1.0 200")
    head, _, body = w.got[2].partition(b"\r\n\r\n")
    assert b"image/jpeg" in head and body[:2] == b"\xff\xd8"
    back = np.asarray(Image.open(io.BytesIO(body)).convert("RGB"))
    assert back.shape == plate.shape
    # GET /matte-key reports the setting beside the key, and stays as it was without one
    base = dict(lo=20.0, hi=60.0, luma=0.25, radius=1, combine="replace", invert=False, to="plate")
    assert keys.current == base
    keys.put_adapt(S.parse_matte_key_adapt_arg("0.0625"))
    keys.apply(w)
    assert keys.current == dict(base, adapt=dict(rate=1 / 16, absorb=0.0))
    assert json.loads(_request(handler, "GET", "/matte-key").partition(b"\r\n\r\n")[2]) == dict(base, adapt=dict(rate=1 / 16, absorb=0.0))
    keys.put(None)
    keys.apply(w)
    assert keys.current is None and w.matte_key_adapt is None
