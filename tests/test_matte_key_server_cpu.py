"""CPU test (-m "not gpu") of the matte key routes of tools/mjpeg_server.py: `--matte-key` / `POST /matte-key` (a colour, the path
of a plate, `capture`, `off`), `POST /matte-key/capture`, `GET /matte-key`, bodies that get a 400 and are counted, and the
producer applying the newest request between two frames."""
import inspect
import json
import os
import sys
import threading

import numpy as np
import pytest

from test_style_bank_cpu import _request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def server():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mjpeg_server as S
    finally:
        sys.path.pop(0)
    return S


def test_argument_parsing(tmp_path):
    from PIL import Image
    S = server()
    colour = dict(lo=40.0, hi=90.0, luma=0.0, radius=1, combine="replace", invert=False)
    assert S.parse_matte_key_arg("00b140") == dict(colour, to=(0, 177, 64))
    assert S.parse_matte_key_arg(" 00B140 , 30 , 80 ") == dict(colour, to=(0, 177, 64), lo=30.0, hi=80.0)
    assert S.parse_matte_key_arg("capture") == dict(colour, luma=0.25, to="capture")
    assert S.parse_matte_key_arg("capture,20,60,0.5,2,and,invert") == dict(lo=20.0, hi=60.0, luma=0.5, radius=2, combine="and", invert=True,
                                                                            to="capture")
    assert S.parse_matte_key_arg("0000ff,20,60,0,0,or") == dict(lo=20.0, hi=60.0, luma=0.0, radius=0, combine="or", invert=False, to=(0, 0, 255))
    assert S.parse_matte_key_arg("off") is None and S.parse_matte_key_arg("") is None
    img = np.random.default_rng(1).integers(0, 256, (30, 54, 3), dtype=np.uint8)
    p = tmp_path / "room.png"
    Image.fromarray(img).save(p)
    got = S.parse_matte_key_arg(f"{p},30,80")
    assert np.array_equal(got.pop("to"), img) and got == dict(colour, lo=30.0, hi=80.0, luma=0.25)
    bad = tmp_path / "bad.png"
    bad.write_bytes(b"no image")
    for text in ("green", "00b14", "00b140,30", "00b140,a,b", "00b140,90,40", "00b140,30,80,2", "00b140,30,80,0,5", "00b140,30,80,0,1.5",
                 "00b140,30,80,0,1,xor", "00b140,30,80,0,1,and,flip", "00b140,30,80,0,1,and,invert,1", str(tmp_path / "none.png"), str(bad),
                 "capture,1025,1026"):
        with pytest.raises(ValueError):
            S.parse_matte_key_arg(text)
    ap_text = open(os.path.join(ROOT, "tools", "mjpeg_server.py")).read()
    assert '"--matte-key"' in ap_text and "parse_matte_key_arg(ap_key)" in ap_text


def test_keys_sits_in_front_of_edges():
    S = server()
    for f in (S.make_handler, S.produce, S.produce_posted):
        names = list(inspect.signature(f).parameters)
        assert names[-2:] == ["keys", "edges"] and names[-3] == "masks", (f.__name__, names)
        assert inspect.signature(f).parameters["keys"].default is None


def test_routes_refusals_and_the_producer():
    S = server()
    green = dict(lo=40.0, hi=90.0, luma=0.0, radius=1, combine="replace", invert=False, to=(0, 177, 64))

    class W:
        """the producer's wrapper: echoes the frame, records the key each frame ran under; posts from inside the loop"""
        matte_key = None
        matte = True

        def __init__(self):
            self.seen = []

        def set_matte_key(self, to, **kw):
            if kw["radius"] == 3:
                raise ValueError("set_matte_key: refused")
            self.matte_key = dict(kw, to=to)

        def capture_matte_plate(self):
            if self.matte_key is None:
                raise ValueError("capture_matte_plate: no matte key is set")
            self.matte_key = dict(self.matte_key, to="capture")

        def clear_matte_key(self):
            self.matte_key = None

        def __call__(self, frame):
            if self.matte_key is not None and self.matte_key["to"] == "capture":
                self.matte_key = dict(self.matte_key, to="plate")                     # the capture happens with the frame
            self.seen.append(None if self.matte_key is None else (self.matte_key["to"], self.matte_key["lo"]))
            n = len(self.seen)
            if n == 1:
                assert post(b"00b140").startswith(b"HTTP/1.0 204")
            elif n == 2:
                assert post(b"00b140,10,20").startswith(b"HTTP/1.0 204")
                assert post(b"0000ff,30,80").startswith(b"HTTP/1.0 204")             # the newest request wins
            elif n == 3:
                assert post(b"00b140,30,80,0,3").startswith(b"HTTP/1.0 204")         # the wrapper refuses it: nothing changes
            elif n == 4:
                assert capture().startswith(b"HTTP/1.0 204")
            elif n == 5:
                assert post(b"").startswith(b"HTTP/1.0 204")                         # an empty body clears it
            elif n == 6:
                assert capture().startswith(b"HTTP/1.0 204")                         # no key: the wrapper refuses
            elif n == 7:
                assert post(b"capture,20,60").startswith(b"HTTP/1.0 204")
            elif n == 8:
                assert post(b"off").startswith(b"HTTP/1.0 204")
            elif n == 9:
                stop.set()
            return frame

    w = W()
    latest, stop = S.Latest(), threading.Event()
    keys = S.MatteKeyBox(w.matte_key)
    handler = S.make_handler(latest, keys=keys)
    post = lambda body: _request(handler, "POST", "/matte-key", body)
    capture = lambda body=b"": _request(handler, "POST", "/matte-key/capture", body)
    for path in ("/matte-key", "/matte-key/capture"):
        assert _request(S.make_handler(latest), "POST", path, b"00b140").startswith(b"HTTP/1.0 404")
    assert _request(S.make_handler(latest), "GET", "/matte-key").startswith(b"HTTP/1.0 404")
    assert _request(handler, "GET", "/matte-key/capture").startswith(b"HTTP/1.0 404")
    # bad bodies: a 400 each, and counted
    for body in (b"green", b"\xff\xfe", b"00b140,30", b"00b140,90,40", b"00b140,30,80,0,9"):
        assert post(body).startswith(b"HTTP/1.0 400"), body
    assert capture(b"now").startswith(b"HTTP/1.0 400")
    assert keys.failed == 6
    assert post(b"x" * 257).startswith(b"HTTP/1.0 413") and capture(b"x" * 257).startswith(b"HTTP/1.0 413")
    assert json.loads(_request(handler, "GET", "/matte-key").partition(b"\r\n\r\n")[2]) is None
    S.produce(w, [b"\xff\xd8 a", b"\xff\xd8 b"], latest, stop, keys=keys)                # (in this thread)
    assert w.seen == [None, ((0, 177, 64), 40.0), ((0, 0, 255), 30.0), ((0, 0, 255), 30.0), ("plate", 30.0), None, None, ("plate", 20.0), None]
    assert keys.failed == 8 and keys.current is None
    keys.put(S.parse_matte_key_arg("00b140"))
    keys.apply(w)
    assert keys.current == dict(green, to=[0, 177, 64])
    assert json.loads(_request(handler, "GET", "/matte-key").partition(b"\r\n\r\n")[2]) == dict(green, to=[0, 177, 64])
    # positional calls of before keep working: the eleven boxes in front of `masks`, then `masks`
    assert S.make_handler(latest, None, None, None, None, None, None, None, None, None, None, None, None) is not None
