"""CPU test (-m "not gpu") of the detail route of tools/mjpeg_server.py: `--detail` / `POST /detail` parsing, 404 without the box,
and the producer applying the newest request between two frames."""
import json
import os
import sys
import threading

import pytest

from test_style_bank_cpu import _request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _settings(radius, eps=2.0, strength=1.0, limit=64.0):
    return dict(radius=radius, eps=eps, strength=strength, limit=limit, show=False)


def test_mjpeg_server_detail_route_and_option():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mjpeg_server as S
    finally:
        sys.path.pop(0)
    assert S.parse_detail_arg("2") == _settings(2)
    assert S.parse_detail_arg(" 8 , 1.5\n") == _settings(8, 1.5)
    assert S.parse_detail_arg("1,1,0.5") == _settings(1, 1.0, 0.5)
    assert S.parse_detail_arg("4,10,4,255") == _settings(4, 10.0, 4.0, 255.0)
    assert S.parse_detail_arg("4,10,0,0") == _settings(4, 10.0, 0.0, 0.0)
    assert S.parse_detail_arg(" off ") is None
    for text in ("", "0", "9", "-1", "2.0", "two", "2,", "2,one", "2,0.5", "2,nan", "2,inf", "2,1,-1", "2,1,4.5", "2,1,nan", "2,1,1,256",
                 "2,1,1,-1", "2,1,1,inf", "2,1,1,64,1", "on"):
        with pytest.raises(ValueError, match="detail"):
            S.parse_detail_arg(text)

    class W:
        """the producer's wrapper: echoes the frame, records the setting each frame ran under; posts requests from inside the loop"""
        detail = None
        refuse = False

        def __init__(self):
            self.seen = []

        def set_detail(self, radius=2, eps=2.0, strength=1.0, limit=64.0, show=False):
            if self.refuse:
                raise ValueError("refused")
            self.detail = dict(radius=radius, eps=eps, strength=strength, limit=limit, show=show)

        def clear_detail(self):
            self.detail = None

        def __call__(self, frame):
            self.seen.append(self.detail)
            n = len(self.seen)
            if n == 1:
                assert post(b"2").startswith(b"HTTP/1.0 204")
            elif n == 2:
                assert post(b"4,3").startswith(b"HTTP/1.0 204")
                assert post(b"8,1.5,2,32").startswith(b"HTTP/1.0 204")       # the newest request wins
            elif n == 3:
                assert post(b"off").startswith(b"HTTP/1.0 204")
            elif n == 4:
                self.refuse = True
                assert post(b"2").startswith(b"HTTP/1.0 204")                # the wrapper refuses it: nothing changes
            elif n == 5:
                stop.set()
            return frame

    w = W()
    latest, stop = S.Latest(), threading.Event()
    details = S.DetailBox(w.detail)
    handler = S.make_handler(latest, details=details)
    post = lambda body: _request(handler, "POST", "/detail", body)
    assert _request(S.make_handler(latest), "POST", "/detail", b"2").startswith(b"HTTP/1.0 404")
    assert _request(S.make_handler(latest), "GET", "/detail").startswith(b"HTTP/1.0 404")
    # (every earlier caller passes at most eight positional arguments: the box is a keyword behind them, None by default)
    assert _request(S.make_handler(latest, None, None, None, None, None, None, None), "GET", "/detail").startswith(b"HTTP/1.0 404")
    assert _request(handler, "GET", "/matte-edge").startswith(b"HTTP/1.0 404")   # (the other routes are not served without their boxes)
    for body in (b"nonsense", b"\xff\xfe", b"0", b"9", b"2,0.5", b"2,1,5", b"2,1,1,300", b"2,1,1,64,0"):
        assert post(body).startswith(b"HTTP/1.0 400"), body
    assert post(b"2" * 300).startswith(b"HTTP/1.0 413")
    assert json.loads(_request(handler, "GET", "/detail").partition(b"\r\n\r\n")[2]) is None
    S.produce(w, [b"\xff\xd8 a", b"\xff\xd8 b"], latest, stop, details=details)      # (in this thread)
    assert w.seen == [None, _settings(2), _settings(8, 1.5, 2.0, 32.0), None, None]
    assert details.failed == 1 and details.current is None
    details.put(_settings(3, 3.0))
    w.refuse = False
    details.apply(w)
    assert json.loads(_request(handler, "GET", "/detail").partition(b"\r\n\r\n")[2]) == _settings(3, 3.0)
    # `produce_posted` takes the box the same way, and works without it as before
    import inspect
    for fn in (S.make_handler, S.produce, S.produce_posted):
        p = inspect.signature(fn).parameters["details"]
        assert p.default is None, fn
    # the option: refused by the same function before anything is loaded
    with pytest.raises(ValueError, match="detail"):
        S.main(["--config", "none.yaml", "--input", "post", "--detail", "9"])
    with pytest.raises(ValueError, match="detail"):
        S.main(["--config", "none.yaml", "--input", "post", "--detail", "2,0"])
