"""CPU test (-m "not gpu") of the follow route of tools/mjpeg_server.py: `--steady-follow` / `POST /steady-follow` parsing, the
empty body, and the producer applying the newest request between two frames."""
import json
import os
import sys
import threading

import pytest

from test_style_bank_cpu import _request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mjpeg_server_steady_follow_route_and_option():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mjpeg_server as S
    finally:
        sys.path.pop(0)
    assert S.parse_steady_follow_arg("4") == dict(search=4, bias=256)
    assert S.parse_steady_follow_arg(" 8 , 0 ") == dict(search=8, bias=0)
    assert S.parse_steady_follow_arg("1,4096") == dict(search=1, bias=4096)
    assert S.parse_steady_follow_arg("off") is None
    for text in ("", "on", "0", "9", "4.0", "4,256.0", "4,-1", "4,4097", "a", "4,b", "4,256,1"):
        with pytest.raises(ValueError):
            S.parse_steady_follow_arg(text)

    class W:
        """the producer's wrapper: echoes the frame, records the setting each frame ran under; posts requests from inside the loop"""
        steady_follow = None

        def __init__(self):
            self.seen = []

        def set_steady_follow(self, search=4, bias=256):
            if bias == 7:
                raise ValueError("refused")
            self.steady_follow = dict(search=search, bias=bias)

        def clear_steady_follow(self):
            self.steady_follow = None

        def __call__(self, frame):
            self.seen.append(self.steady_follow and dict(self.steady_follow))
            n = len(self.seen)
            if n == 1:
                assert post(b"4").startswith(b"HTTP/1.0 204")
            elif n == 2:
                assert post(b"2,64").startswith(b"HTTP/1.0 204")
                assert post(b"8,512").startswith(b"HTTP/1.0 204")                    # the newest request wins
            elif n == 3:
                assert post(b"4,7").startswith(b"HTTP/1.0 204")                      # the wrapper refuses it: nothing changes
            elif n == 4:
                assert post(b"").startswith(b"HTTP/1.0 204")                         # an empty body clears it
            elif n == 5:
                assert post(b"3").startswith(b"HTTP/1.0 204")
            elif n == 6:
                assert post(b"off").startswith(b"HTTP/1.0 204")
            elif n == 7:
                stop.set()
            return frame

    w = W()
    latest, stop = S.Latest(), threading.Event()
    follows = S.SteadyFollowBox(w.steady_follow)
    handler = S.make_handler(latest, follows=follows)
    post = lambda body: _request(handler, "POST", "/steady-follow", body)
    assert _request(S.make_handler(latest), "POST", "/steady-follow", b"4").startswith(b"HTTP/1.0 404")
    assert _request(S.make_handler(latest), "GET", "/steady-follow").startswith(b"HTTP/1.0 404")
    assert _request(handler, "POST", "/steady", b"off").startswith(b"HTTP/1.0 404")      # (no steady box in this handler)
    for body in (b"on", b"9", b"\xff\xfe", b"4,1.5"):
        assert post(body).startswith(b"HTTP/1.0 400"), body
    assert post(b"0" * 300).startswith(b"HTTP/1.0 413")
    assert json.loads(_request(handler, "GET", "/steady-follow").partition(b"\r\n\r\n")[2]) is None
    S.produce(w, [b"\xff\xd8 a", b"\xff\xd8 b"], latest, stop, follows=follows)          # (in this thread)
    assert w.seen == [None, dict(search=4, bias=256), dict(search=8, bias=512), dict(search=8, bias=512), None, dict(search=3, bias=256),
                      None]
    assert follows.failed == 1 and follows.current is None
    follows.put(S.parse_steady_follow_arg("2,128"))
    follows.apply(w)
    assert follows.current == dict(search=2, bias=128)
    handler = S.make_handler(latest, follows=follows)
    assert json.loads(_request(handler, "GET", "/steady-follow").partition(b"\r\n\r\n")[2]) == follows.current
