"""CPU test (-m "not gpu") of the matte route of tools/mjpeg_server.py: `--matte` / `POST /matte` parsing and the producer applying
the newest request between two frames."""
import json
import os
import sys
import threading

import pytest

from test_style_bank_cpu import _request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mjpeg_server_matte_route_and_option():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mjpeg_server as S
    finally:
        sys.path.pop(0)
    assert S.parse_matte_arg("0.3,0.7") == dict(lo=0.3, hi=0.7, keep="near", feather=0)
    assert S.parse_matte_arg(" 0.5, 0.5, 4 ") == dict(lo=0.5, hi=0.5, keep="near", feather=4)
    assert S.parse_matte_arg("0,1,8,far") == dict(lo=0.0, hi=1.0, keep="far", feather=8)
    assert S.parse_matte_arg("off") is None
    for text in ("", "0.3", "0.7,0.3", "0.3,0.7,9", "0.3,0.7,1.5", "0.3,0.7,2,sideways", "a,b", "0.3,1.2", "0.3,0.7,2,far,1"):
        with pytest.raises(ValueError):
            S.parse_matte_arg(text)

    class W:
        """the producer's wrapper: echoes the frame, records the matte each frame ran under; posts requests from inside the loop"""
        matte = None

        def __init__(self):
            self.seen = []

        def set_matte(self, lo, hi, *, keep="near", feather=0, show=False):
            if feather == 7:
                raise ValueError("refused")
            self.matte = dict(lo=lo, hi=hi, keep=keep, feather=feather, show=show)

        def clear_matte(self):
            self.matte = None

        def __call__(self, frame):
            self.seen.append(self.matte and dict(self.matte))
            n = len(self.seen)
            if n == 1:
                assert post(b"0.3,0.7").startswith(b"HTTP/1.0 204")
            elif n == 2:
                assert post(b"0.2,0.4,1").startswith(b"HTTP/1.0 204")
                assert post(b"0.5,0.5,4,far").startswith(b"HTTP/1.0 204")          # the newest request wins
            elif n == 3:
                assert post(b"0.1,0.2,7").startswith(b"HTTP/1.0 204")               # the wrapper refuses it: nothing changes
            elif n == 4:
                assert post(b"off").startswith(b"HTTP/1.0 204")
            elif n == 5:
                stop.set()
            return frame

    w = W()
    latest, stop = S.Latest(), threading.Event()
    mattes = S.MatteBox(w.matte)
    handler = S.make_handler(latest, None, None, mattes)
    post = lambda body: _request(handler, "POST", "/matte", body)
    assert _request(S.make_handler(latest), "POST", "/matte", b"off").startswith(b"HTTP/1.0 404")
    assert _request(S.make_handler(latest), "GET", "/matte").startswith(b"HTTP/1.0 404")
    for body in (b"0.7,0.3", b"nonsense", b"\xff\xfe", b"0.3,0.7,9"):
        assert post(body).startswith(b"HTTP/1.0 400"), body
    assert post(b"0" * 300).startswith(b"HTTP/1.0 413")
    assert json.loads(_request(handler, "GET", "/matte").partition(b"\r\n\r\n")[2]) is None
    S.produce(w, [b"\xff\xd8 a", b"\xff\xd8 b"], latest, stop, None, mattes)        # (in this thread)
    far = dict(lo=0.5, hi=0.5, keep="far", feather=4, show=False)
    assert w.seen == [None, dict(lo=0.3, hi=0.7, keep="near", feather=0, show=False), far, far, None]
    assert mattes.failed == 1 and mattes.current is None
