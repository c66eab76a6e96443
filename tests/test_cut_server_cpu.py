"""CPU test (-m "not gpu") of the cut detector's routes of tools/mjpeg_server.py: `POST /cut-detect`, `POST /auto-rewarm`, `GET
/cuts`, `--cut-detect` / `--auto-rewarm`, the 400s, and the producer applying a request between two frames."""
import json
import os
import threading

import pytest

from test_rewarm_server_cpu import ROOT, server
from test_style_bank_cpu import _request


def body_of(reply):
    return json.loads(reply.partition(b"\r\n\r\n")[2])


def test_parsers_and_options():
    S = server()
    assert S.parse_cut_detect_arg("on") == dict(thumb=20.0, hist=0.35, ratio=3.0, gap=8) and S.parse_cut_detect_arg(" off\n") is None
    assert S.parse_cut_detect_arg("12.5,0.5") == dict(thumb=12.5, hist=0.5, ratio=3.0, gap=8)
    assert S.parse_cut_detect_arg("30, 0.25, 0, 4") == dict(thumb=30.0, hist=0.25, ratio=0.0, gap=4)
    for text in ("", "20", "20,", "a,b", "20,0.3,3,8,1", "20,0.3,3,1.5", "300,0.3", "20,1.5", "20,0.3,0.5", "20,0.3,3,256", "yes"):
        with pytest.raises(ValueError):
            S.parse_cut_detect_arg(text)
    assert S.parse_auto_rewarm_arg("on") is True and S.parse_auto_rewarm_arg("off ") is False
    for text in ("", "1", "true", "On"):
        with pytest.raises(ValueError):
            S.parse_auto_rewarm_arg(text)
    text = open(os.path.join(ROOT, "tools", "mjpeg_server.py")).read()
    assert '"--cut-detect"' in text and '"--auto-rewarm"' in text and "args.keep_recent = True" in text
    frames = open(os.path.join(ROOT, "tools", "stream_frames.py")).read()
    assert '"--cut-detect"' in frames and '"--auto-rewarm"' in frames


class W:
    """the producer's wrapper: echoes the frame, records what ran before each frame; posts requests from inside the loop"""

    def __init__(self, post, stop, keep_recent=True):
        self.events, self.frames, self.post, self.stop, self.keep_recent = [], 0, post, stop, keep_recent
        self.cut_detect, self.auto_rewarm, self.cuts, self.auto_rewarms, self.last_cut_record = None, False, [], 0, None

    def set_cut_detect(self, **kw):
        self.cut_detect = dict(kw)
        self.events.append(("detect", dict(kw)))

    def clear_cut_detect(self):
        self.cut_detect, self.auto_rewarm = None, False
        self.events.append(("detect", None))

    def set_auto_rewarm(self, on=True):
        if on and self.cut_detect is None:
            raise ValueError("auto_rewarm needs a cut detector")
        self.auto_rewarm = on
        self.events.append(("auto", on))

    def __call__(self, frame):
        self.frames += 1
        n = self.frames
        self.events.append(("frame", n))
        if self.cut_detect is not None:
            self.last_cut_record = {"n": n, "cut": n == 4}
            if n == 4:
                self.cuts.append(n)
        post, ok = self.post, b"HTTP/1.0 204"
        if n == 1:
            assert post("/auto-rewarm", b"on").startswith(ok)                # no detector yet: the wrapper refuses it
        elif n == 2:
            assert post("/cut-detect", b"10,0.5").startswith(ok) and post("/cut-detect", b"on").startswith(ok)     # the newest wins
            assert post("/auto-rewarm", b"on").startswith(ok)                # behind the detector, between the same two frames
        elif n == 4:
            assert post("/cut-detect", b"25,0.4,2,3").startswith(ok)
        elif n == 5:
            assert post("/auto-rewarm", b"off").startswith(ok)
        elif n == 6:
            assert post("/cut-detect", b"off").startswith(ok)
        elif n == 7:
            self.stop.set()
        return frame


def test_the_routes_and_the_producer_applying_them_between_frames():
    S = server()
    latest, stop = S.Latest(), threading.Event()
    cuts = S.CutBox(None, False, keep_recent=True)
    styles = S.StyleBox(["default"], {"default": 1.0}, keep_recent=True, cuts=cuts)
    handler = S.make_handler(latest, styles=styles)
    post = lambda path, body: _request(handler, "POST", path, body)
    # no box, no routes
    plain = S.make_handler(latest, styles=S.StyleBox(["default"]))
    for method, path, body in (("POST", "/cut-detect", b"on"), ("POST", "/auto-rewarm", b"on"), ("GET", "/cuts", None), ("GET", "/cut-detect", None)):
        assert _request(plain, method, path, *(() if body is None else (body,))).startswith(b"HTTP/1.0 404"), path
    # a bad body is a 400 and queues nothing
    for body in (b"20", b"a,b", b"300,0.3", b"20,1.5", b"20,0.3,0.5", b"20,0.3,3,256", b"20,0.3,3,8,1", b"\xff\xfe", b"yes"):
        assert post("/cut-detect", body).startswith(b"HTTP/1.0 400"), body
    for body in (b"1", b"true", b"\xff\xfe", b"on off"):
        assert post("/auto-rewarm", body).startswith(b"HTTP/1.0 400"), body
    assert post("/cut-detect", b" " * 300).startswith(b"HTTP/1.0 413") and post("/cut-detect", b"").startswith(b"HTTP/1.0 400")
    assert cuts._want is S.CutBox._NOTHING and cuts._want_auto is None
    # without a recent window the automatic re-warm is refused at the door; switching it off is not
    bare = S.CutBox(None, False)
    h2 = S.make_handler(latest, styles=S.StyleBox(["default"], cuts=bare))
    assert _request(h2, "POST", "/auto-rewarm", b"on").startswith(b"HTTP/1.0 400") and bare._want_auto is None
    assert _request(h2, "POST", "/auto-rewarm", b"off").startswith(b"HTTP/1.0 204") and bare._want_auto is False
    assert body_of(_request(handler, "GET", "/cuts")) == {"cuts": [], "auto_rewarms": 0, "last": None}
    assert body_of(_request(handler, "GET", "/cut-detect")) is None and body_of(_request(handler, "GET", "/auto-rewarm")) is False

    w = W(post, stop)
    S.produce(w, [b"\xff\xd8 a", b"\xff\xd8 b"], latest, stop, styles=styles)                               # (in this thread)
    default = dict(thumb=20.0, hist=0.35, ratio=3.0, gap=8)
    assert w.events == [("frame", 1), ("frame", 2), ("detect", default), ("auto", True), ("frame", 3), ("frame", 4),
                        ("detect", dict(thumb=25.0, hist=0.4, ratio=2.0, gap=3)), ("frame", 5), ("auto", False), ("frame", 6),
                        ("detect", None), ("frame", 7)]
    assert cuts.failed == 1 and cuts.current is None and cuts.auto is False
    # the report is the wrapper's as of the last `apply`, the one in front of frame 7
    assert body_of(_request(handler, "GET", "/cuts")) == {"cuts": [4], "auto_rewarms": 0, "last": {"n": 6, "cut": False}}
