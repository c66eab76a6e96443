"""CPU test (-m "not gpu") of the colour-lock route of tools/mjpeg_server.py: `--color-lock` / `POST /color` parsing and the
producer applying the newest request between two frames."""
import json
import os
import sys
import threading

import pytest

from test_style_bank_cpu import _request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mjpeg_server_color_route_and_option():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mjpeg_server as S
    finally:
        sys.path.pop(0)
    assert S.parse_color_arg("source") == dict(to="source", strength=1.0, rate=0.1)
    assert S.parse_color_arg(" ema , 0.5 ") == dict(to="ema", strength=0.5, rate=0.1)
    assert S.parse_color_arg("ema,0,1") == dict(to="ema", strength=0.0, rate=1.0)
    assert S.parse_color_arg("off") is None
    for text in ("", "first", "image", "source,1.5", "ema,-0.1", "ema,0.5,0", "ema,0.5,1.5", "ema,a", "ema,0.5,0.1,3", "0.5"):
        with pytest.raises(ValueError):
            S.parse_color_arg(text)

    class W:
        """the producer's wrapper: echoes the frame, records the lock each frame ran under; posts requests from inside the loop"""
        color_lock = None

        def __init__(self):
            self.seen = []

        def set_color_lock(self, to="source", strength=1.0, rate=0.1):
            if strength == 0.125:
                raise ValueError("refused")
            self.color_lock = dict(to=to, strength=strength, rate=rate)

        def clear_color_lock(self):
            self.color_lock = None

        def __call__(self, frame):
            self.seen.append(self.color_lock and dict(self.color_lock))
            n = len(self.seen)
            if n == 1:
                assert post(b"source").startswith(b"HTTP/1.0 204")
            elif n == 2:
                assert post(b"source,0.5").startswith(b"HTTP/1.0 204")
                assert post(b"ema,0.75,0.2").startswith(b"HTTP/1.0 204")             # the newest request wins
            elif n == 3:
                assert post(b"ema,0.125").startswith(b"HTTP/1.0 204")                # the wrapper refuses it: nothing changes
            elif n == 4:
                assert post(b"off").startswith(b"HTTP/1.0 204")
            elif n == 5:
                stop.set()
            return frame

    w = W()
    latest, stop = S.Latest(), threading.Event()
    colors = S.ColorBox(w.color_lock)
    handler = S.make_handler(latest, None, None, None, colors)
    post = lambda body: _request(handler, "POST", "/color", body)
    assert _request(S.make_handler(latest), "POST", "/color", b"off").startswith(b"HTTP/1.0 404")
    assert _request(S.make_handler(latest), "GET", "/color").startswith(b"HTTP/1.0 404")
    assert _request(handler, "POST", "/matte", b"off").startswith(b"HTTP/1.0 404")       # (no matte box in this handler)
    for body in (b"first", b"source,2", b"\xff\xfe", b"ema,0.5,0"):
        assert post(body).startswith(b"HTTP/1.0 400"), body
    assert post(b"0" * 300).startswith(b"HTTP/1.0 413")
    assert json.loads(_request(handler, "GET", "/color").partition(b"\r\n\r\n")[2]) is None
    S.produce(w, [b"\xff\xd8 a", b"\xff\xd8 b"], latest, stop, None, None, colors)       # (in this thread)
    ema = dict(to="ema", strength=0.75, rate=0.2)
    assert w.seen == [None, dict(to="source", strength=1.0, rate=0.1), ema, ema, None]
    assert colors.failed == 1 and colors.current is None
