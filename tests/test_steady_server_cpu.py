"""CPU test (-m "not gpu") of the steady route of tools/mjpeg_server.py: `--steady` / `POST /steady` parsing and the producer
applying the newest request between two frames."""
import json
import os
import sys
import threading

import pytest

from test_style_bank_cpu import _request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mjpeg_server_steady_route_and_option():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mjpeg_server as S
    finally:
        sys.path.pop(0)
    assert S.parse_steady_arg("2,10") == dict(lo=2.0, hi=10.0, strength=0.8, radius=2)
    assert S.parse_steady_arg(" 1.5 , 6 , 0.5 ") == dict(lo=1.5, hi=6.0, strength=0.5, radius=2)
    assert S.parse_steady_arg("0,255,1,8") == dict(lo=0.0, hi=255.0, strength=1.0, radius=8)
    assert S.parse_steady_arg("4,4,0,0") == dict(lo=4.0, hi=4.0, strength=0.0, radius=0)
    assert S.parse_steady_arg("off") is None
    for text in ("", "2", "on", "10,2", "-1,10", "2,256", "2,10,1.5", "2,10,-0.1", "2,10,0.8,9", "2,10,0.8,-1", "2,10,0.8,1.5", "a,10",
                 "2,10,0.8,2,1"):
        with pytest.raises(ValueError):
            S.parse_steady_arg(text)

    class W:
        """the producer's wrapper: echoes the frame, records the mode each frame ran under; posts requests from inside the loop"""
        steady = None

        def __init__(self):
            self.seen = []

        def set_steady(self, lo=2.0, hi=10.0, *, strength=0.8, radius=2, show=False):
            if strength == 0.125:
                raise ValueError("refused")
            self.steady = dict(lo=lo, hi=hi, strength=strength, radius=radius, show=show)

        def clear_steady(self):
            self.steady = None

        def __call__(self, frame):
            self.seen.append(self.steady and dict(self.steady))
            n = len(self.seen)
            if n == 1:
                assert post(b"2,10").startswith(b"HTTP/1.0 204")
            elif n == 2:
                assert post(b"2,10,0.5").startswith(b"HTTP/1.0 204")
                assert post(b"3,12,0.75,4").startswith(b"HTTP/1.0 204")              # the newest request wins
            elif n == 3:
                assert post(b"2,10,0.125").startswith(b"HTTP/1.0 204")               # the wrapper refuses it: nothing changes
            elif n == 4:
                assert post(b"off").startswith(b"HTTP/1.0 204")
            elif n == 5:
                stop.set()
            return frame

    w = W()
    latest, stop = S.Latest(), threading.Event()
    steadies = S.SteadyBox(w.steady)
    handler = S.make_handler(latest, steadies=steadies)
    post = lambda body: _request(handler, "POST", "/steady", body)
    assert _request(S.make_handler(latest), "POST", "/steady", b"off").startswith(b"HTTP/1.0 404")
    assert _request(S.make_handler(latest), "GET", "/steady").startswith(b"HTTP/1.0 404")
    assert _request(handler, "POST", "/color", b"off").startswith(b"HTTP/1.0 404")       # (no colour box in this handler)
    for body in (b"on", b"10,2", b"\xff\xfe", b"2,10,2"):
        assert post(body).startswith(b"HTTP/1.0 400"), body
    assert post(b"0" * 300).startswith(b"HTTP/1.0 413")
    assert json.loads(_request(handler, "GET", "/steady").partition(b"\r\n\r\n")[2]) is None
    S.produce(w, [b"\xff\xd8 a", b"\xff\xd8 b"], latest, stop, steadies=steadies)        # (in this thread)
    first = dict(lo=2.0, hi=10.0, strength=0.8, radius=2, show=False)
    newest = dict(lo=3.0, hi=12.0, strength=0.75, radius=4, show=False)
    assert w.seen == [None, first, newest, newest, None]
    assert steadies.failed == 1 and steadies.current is None
    steadies.put(S.parse_steady_arg("1,5"))
    steadies.apply(w)
    assert steadies.current == dict(lo=1.0, hi=5.0, strength=0.8, radius=2, show=False)
    handler = S.make_handler(latest, steadies=steadies)
    assert json.loads(_request(handler, "GET", "/steady").partition(b"\r\n\r\n")[2]) == steadies.current
