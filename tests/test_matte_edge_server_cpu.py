"""CPU test (-m "not gpu") of the matte-edge route of tools/mjpeg_server.py: `--matte-edge` / `POST /matte-edge` parsing, 404
without the box, and the producer applying the newest request between two frames."""
import json
import os
import sys
import threading

import pytest

from test_style_bank_cpu import _request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mjpeg_server_matte_edge_route_and_option():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mjpeg_server as S
    finally:
        sys.path.pop(0)
    assert S.parse_matte_edge_arg("4") == dict(radius=4, eps=10.0)
    assert S.parse_matte_edge_arg(" 8 , 2.5\n") == dict(radius=8, eps=2.5)
    assert S.parse_matte_edge_arg("1,1") == dict(radius=1, eps=1.0)
    assert S.parse_matte_edge_arg(" off ") is None
    for text in ("", "0", "9", "-1", "4.0", "four", "4,", "4,ten", "4,0.5", "4,nan", "4,inf", "4,10,2", "on"):
        with pytest.raises(ValueError, match="matte edge"):
            S.parse_matte_edge_arg(text)

    class W:
        """the producer's wrapper: echoes the frame, records the setting each frame ran under; posts requests from inside the loop"""
        matte_edge = None
        refuse = False

        def __init__(self):
            self.seen = []

        def set_matte_edge(self, radius, eps):
            if self.refuse:
                raise ValueError("refused")
            self.matte_edge = dict(radius=radius, eps=eps)

        def clear_matte_edge(self):
            self.matte_edge = None

        def __call__(self, frame):
            self.seen.append(self.matte_edge)
            n = len(self.seen)
            if n == 1:
                assert post(b"4").startswith(b"HTTP/1.0 204")
            elif n == 2:
                assert post(b"2,3").startswith(b"HTTP/1.0 204")
                assert post(b"8,1.5").startswith(b"HTTP/1.0 204")            # the newest request wins
            elif n == 3:
                assert post(b"off").startswith(b"HTTP/1.0 204")
            elif n == 4:
                self.refuse = True
                assert post(b"4").startswith(b"HTTP/1.0 204")                # the wrapper refuses it: nothing changes
            elif n == 5:
                stop.set()
            return frame

    w = W()
    latest, stop = S.Latest(), threading.Event()
    edges = S.MatteEdgeBox(w.matte_edge)
    handler = S.make_handler(latest, edges=edges)
    post = lambda body: _request(handler, "POST", "/matte-edge", body)
    assert _request(S.make_handler(latest), "POST", "/matte-edge", b"4").startswith(b"HTTP/1.0 404")
    assert _request(S.make_handler(latest), "GET", "/matte-edge").startswith(b"HTTP/1.0 404")
    # (every earlier caller passes eight positional arguments: the box is a trailing keyword, None by default)
    assert _request(S.make_handler(latest, None, None, None, None, None, None, None), "GET", "/matte-edge").startswith(b"HTTP/1.0 404")
    assert _request(handler, "GET", "/matte").startswith(b"HTTP/1.0 404")    # (the other routes are not served without their boxes)
    for body in (b"nonsense", b"\xff\xfe", b"0", b"9", b"4,0.5", b"4,10,1"):
        assert post(body).startswith(b"HTTP/1.0 400"), body
    assert post(b"4" * 300).startswith(b"HTTP/1.0 413")
    assert json.loads(_request(handler, "GET", "/matte-edge").partition(b"\r\n\r\n")[2]) is None
    S.produce(w, [b"\xff\xd8 a", b"\xff\xd8 b"], latest, stop, edges=edges)      # (in this thread)
    assert w.seen == [None, dict(radius=4, eps=10.0), dict(radius=8, eps=1.5), None, None]
    assert edges.failed == 1 and edges.current is None
    edges.put(dict(radius=2, eps=3.0))
    w.refuse = False
    edges.apply(w)
    assert json.loads(_request(handler, "GET", "/matte-edge").partition(b"\r\n\r\n")[2]) == dict(radius=2, eps=3.0)
    # `produce_posted` takes the box the same way, and works without it as before
    import inspect
    for fn in (S.make_handler, S.produce, S.produce_posted):
        p = list(inspect.signature(fn).parameters.values())[-1]
        assert p.name == "edges" and p.default is None, fn
    # the option: refused by the same function before anything is loaded
    with pytest.raises(ValueError, match="matte edge"):
        S.main(["--config", "none.yaml", "--input", "post", "--matte-edge", "9"])
    with pytest.raises(ValueError, match="matte edge"):
        S.main(["--config", "none.yaml", "--input", "post", "--matte-edge", "4,0"])
