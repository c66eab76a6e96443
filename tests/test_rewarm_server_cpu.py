"""CPU test (-m "not gpu") of the re-warm routes of tools/mjpeg_server.py: `POST /rewarm`, "rewarm" in the body of `POST /style`,
`--keep-recent`, the 400s, and the producer applying a request between two frames."""
import json
import os
import sys
import threading

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


def test_parsers_and_option():
    S = server()
    assert S.parse_rewarm_body(b'{"source": "warmup"}') == "warmup" and S.parse_rewarm_body(b' {"source":"recent"}\n') == "recent"
    for body in (b"", b"warmup", b'"warmup"', b"{}", b'{"source": "frames"}', b'{"source": 1}', b'{"source": "warmup", "depths": 1}', b"[1]",
                 b"\xff\xfe", b'{"Source": "warmup"}'):
        with pytest.raises(ValueError):
            S.parse_rewarm_body(body)
    assert [S.parse_style_rewarm(v) for v in (True, False, "warmup", "recent")] == [True, False, True, "recent"]
    for v in (1, 0, None, "yes", "frames", [], {}):
        with pytest.raises(ValueError, match='"rewarm"'):
            S.parse_style_rewarm(v)
    text = open(os.path.join(ROOT, "tools", "mjpeg_server.py")).read()
    assert '"--keep-recent"' in text and "keep_recent=args.keep_recent" in text


def test_mjpeg_server_rewarm_route_and_style_rewarm():
    S = server()

    class W:
        """the producer's wrapper: echoes the frame, records what ran before each frame; posts requests from inside the loop"""

        def __init__(self):
            self.style, self.events, self.frames = {"default": 1.0}, [], 0

        def set_style(self, mix, rewarm=False):
            if "broken" in mix:
                raise ValueError("refused")
            self.style = dict(mix)
            self.events.append(("style", dict(mix), rewarm))

        def rewarm(self, source="warmup", *, depths=None):
            if source == "recent" and self.frames < 4:
                raise ValueError("3 frames since prepare, the window needs 8")
            self.events.append(("rewarm", source))

        def __call__(self, frame):
            self.frames += 1
            self.events.append(("frame", self.frames))
            n = self.frames
            if n == 1:
                assert rewarm({"source": "warmup"}).startswith(b"HTTP/1.0 204")
            elif n == 2:
                assert rewarm({"source": "warmup"}).startswith(b"HTTP/1.0 204")
                assert rewarm({"source": "recent"}).startswith(b"HTTP/1.0 204")        # the newest request wins; the wrapper refuses it
            elif n == 3:
                assert style({"b": 1.0, "rewarm": True}).startswith(b"HTTP/1.0 204")
            elif n == 4:
                assert style({"default": 0.5, "b": 0.5, "rewarm": "recent"}).startswith(b"HTTP/1.0 204")
                assert rewarm({"source": "recent"}).startswith(b"HTTP/1.0 204")        # behind the style, between the same two frames
            elif n == 5:
                assert style({"default": 1.0, "rewarm": False}).startswith(b"HTTP/1.0 204")
            elif n == 6:
                assert style({"b": 1.0}).startswith(b"HTTP/1.0 204")
            elif n == 7:
                assert style({"broken": 1.0, "rewarm": "warmup"}).startswith(b"HTTP/1.0 204")
            elif n == 8:
                stop.set()
            return frame

    w = W()
    latest, stop = S.Latest(), threading.Event()
    styles = S.StyleBox(["default", "b", "broken"], w.style, keep_recent=True)
    handler = S.make_handler(latest, styles=styles)
    rewarm = lambda req: _request(handler, "POST", "/rewarm", json.dumps(req).encode())
    style = lambda req: _request(handler, "POST", "/style", json.dumps(req).encode())
    # no box, no route; a bad body is a 400 and queues nothing
    assert _request(S.make_handler(latest), "POST", "/rewarm", b'{"source": "warmup"}').startswith(b"HTTP/1.0 404")
    assert _request(S.make_handler(latest), "GET", "/rewarm").startswith(b"HTTP/1.0 404")
    for body in (b"warmup", b"{}", b'{"source": "frames"}', b'{"source": "warmup", "x": 1}', b"\xff\xfe{}", b"[]"):
        assert _request(handler, "POST", "/rewarm", body).startswith(b"HTTP/1.0 400"), body
    assert _request(handler, "POST", "/rewarm", b" " * 300).startswith(b"HTTP/1.0 413")
    for req in ({"b": 1.0, "rewarm": "soon"}, {"b": 1.0, "rewarm": 1}, {"rewarm": True}, {"b": 0.5, "rewarm": True}, {"nobody": 1.0, "rewarm": True}):
        assert style(req).startswith(b"HTTP/1.0 400"), req
    assert styles.take() is None and styles._source is None
    # without --keep-recent "recent" is refused at the door, on both routes
    plain = S.StyleBox(["default", "b"], w.style)
    h2 = S.make_handler(latest, styles=plain)
    assert _request(h2, "POST", "/rewarm", b'{"source": "recent"}').startswith(b"HTTP/1.0 400")
    assert _request(h2, "POST", "/style", b'{"b": 1.0, "rewarm": "recent"}').startswith(b"HTTP/1.0 400")
    assert plain.take() is None and plain._source is None
    assert _request(h2, "POST", "/rewarm", b'{"source": "warmup"}').startswith(b"HTTP/1.0 204") and plain._source == "warmup"
    assert _request(h2, "POST", "/style", b'{"b": 1.0, "rewarm": true}').startswith(b"HTTP/1.0 204") and plain._rewarm is True
    with pytest.raises(ValueError):
        plain.put_rewarm("frames")
    assert json.loads(_request(handler, "GET", "/rewarm").partition(b"\r\n\r\n")[2]) == {"rewarms": 0, "failed": 0}

    S.produce(w, [b"\xff\xd8 a", b"\xff\xd8 b"], latest, stop, styles=styles)                          # (in this thread)
    assert w.events == [("frame", 1), ("rewarm", "warmup"), ("frame", 2), ("frame", 3), ("style", {"b": 1.0}, True), ("frame", 4),
                        ("style", {"default": 0.5, "b": 0.5}, "recent"), ("rewarm", "recent"), ("frame", 5),
                        ("style", {"default": 1.0}, False), ("frame", 6), ("style", {"b": 1.0}, False), ("frame", 7), ("frame", 8)]
    assert (styles.rewarms, styles.rewarm_failed, styles.failed) == (2, 1, 1) and styles.current == {"b": 1.0}
    assert json.loads(_request(handler, "GET", "/rewarm").partition(b"\r\n\r\n")[2]) == {"rewarms": 2, "failed": 1}
