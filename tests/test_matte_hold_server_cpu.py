"""CPU test (-m "not gpu") of the matte hold route of tools/mjpeg_server.py: `--matte-hold` / `POST /matte-hold` parsing, the empty
body, and the producer applying the newest request between two frames."""
import json
import os
import sys
import threading

import pytest

from test_style_bank_cpu import _request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = dict(lo=2.0, hi=10.0, strength=0.8, radius=2, search=0, bias=256)


def test_mjpeg_server_matte_hold_route_and_option():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mjpeg_server as S
    finally:
        sys.path.pop(0)
    assert S.parse_matte_hold_arg("2,10") == DEFAULT
    assert S.parse_matte_hold_arg(" 1 , 20.5 , 0.5 ") == dict(DEFAULT, lo=1.0, hi=20.5, strength=0.5)
    assert S.parse_matte_hold_arg("0,255,1,8,8,4096") == dict(lo=0.0, hi=255.0, strength=1.0, radius=8, search=8, bias=4096)
    assert S.parse_matte_hold_arg("2,10,0.8,0,4") == dict(DEFAULT, radius=0, search=4)
    assert S.parse_matte_hold_arg("off") is None
    for text in ("", "on", "2", "10,2", "-1,10", "2,256", "2,10,1.5", "2,10,0.8,9", "2,10,0.8,2.0", "2,10,0.8,2,9", "2,10,0.8,2,-1",
                 "2,10,0.8,2,4,4097", "2,10,0.8,2,4,1.5", "a,10", "2,10,0.8,2,4,256,1"):
        with pytest.raises(ValueError):
            S.parse_matte_hold_arg(text)
    ap_text = open(os.path.join(ROOT, "tools", "mjpeg_server.py")).read()
    assert '"--matte-hold"' in ap_text and "parse_matte_hold_arg(args.matte_hold)" in ap_text

    class W:
        """the producer's wrapper: echoes the frame, records the setting each frame ran under; posts requests from inside the loop"""
        matte_hold = None

        def __init__(self):
            self.seen = []

        def set_matte_hold(self, lo=2.0, hi=10.0, *, strength=0.8, radius=2, search=0, bias=256):
            if bias == 7:
                raise ValueError("refused")
            self.matte_hold = dict(lo=lo, hi=hi, strength=strength, radius=radius, search=search, bias=bias)

        def clear_matte_hold(self):
            self.matte_hold = None

        def __call__(self, frame):
            self.seen.append(self.matte_hold and dict(self.matte_hold))
            n = len(self.seen)
            if n == 1:
                assert post(b"2,10").startswith(b"HTTP/1.0 204")
            elif n == 2:
                assert post(b"1,5").startswith(b"HTTP/1.0 204")
                assert post(b"3,12,0.5,1,4,128").startswith(b"HTTP/1.0 204")         # the newest request wins
            elif n == 3:
                assert post(b"2,10,0.8,2,4,7").startswith(b"HTTP/1.0 204")           # the wrapper refuses it: nothing changes
            elif n == 4:
                assert post(b"").startswith(b"HTTP/1.0 204")                         # an empty body clears it
            elif n == 5:
                assert post(b"2,10,0.9").startswith(b"HTTP/1.0 204")
            elif n == 6:
                assert post(b"off").startswith(b"HTTP/1.0 204")
            elif n == 7:
                stop.set()
            return frame

    w = W()
    latest, stop = S.Latest(), threading.Event()
    holds = S.MatteHoldBox(w.matte_hold)
    handler = S.make_handler(latest, holds=holds)
    post = lambda body: _request(handler, "POST", "/matte-hold", body)
    assert _request(S.make_handler(latest), "POST", "/matte-hold", b"2,10").startswith(b"HTTP/1.0 404")
    assert _request(S.make_handler(latest), "GET", "/matte-hold").startswith(b"HTTP/1.0 404")
    assert _request(handler, "POST", "/matte-edge", b"off").startswith(b"HTTP/1.0 404")   # (no edge box in this handler)
    for body in (b"on", b"2", b"\xff\xfe", b"2,10,0.8,1.5"):
        assert post(body).startswith(b"HTTP/1.0 400"), body
    assert post(b"0" * 300).startswith(b"HTTP/1.0 413")
    assert json.loads(_request(handler, "GET", "/matte-hold").partition(b"\r\n\r\n")[2]) is None
    S.produce(w, [b"\xff\xd8 a", b"\xff\xd8 b"], latest, stop, holds=holds)              # (in this thread)
    other = dict(lo=3.0, hi=12.0, strength=0.5, radius=1, search=4, bias=128)
    assert w.seen == [None, DEFAULT, other, other, None, dict(DEFAULT, strength=0.9), None]
    assert holds.failed == 1 and holds.current is None
    holds.put(S.parse_matte_hold_arg("2,10,0.8,2,8"))
    holds.apply(w)
    assert holds.current == dict(DEFAULT, search=8)
    handler = S.make_handler(latest, holds=holds)
    assert json.loads(_request(handler, "GET", "/matte-hold").partition(b"\r\n\r\n")[2]) == holds.current
