"""CPU test (-m "not gpu") of the plate gain's routes of tools/mjpeg_server.py: `--matte-key-gain` / `POST /matte-key/gain` (`on`,
`LIMIT[,MIN_SHARE]`, `off`), `GET /matte-key/gain` (the setting and the last measurement, or 404), bodies that get a 400 and are
counted, the body of `GET /matte-key` staying as it was, and the producer applying the newest request between two frames."""
import json
import os
import threading

import pytest

from test_matte_key_server_cpu import ROOT, server
from test_style_bank_cpu import _request


def test_argument_parsing():
    S = server()
    assert S.parse_matte_key_gain_arg("on") == dict(limit=2.0, min_share=1 / 16)
    assert S.parse_matte_key_gain_arg("1.5") == dict(limit=1.5, min_share=1 / 16)
    assert S.parse_matte_key_gain_arg(" 3 , 0.25 ") == dict(limit=3.0, min_share=0.25)
    assert S.parse_matte_key_gain_arg("1,0") == dict(limit=1.0, min_share=0.0) and S.parse_matte_key_gain_arg("3.99,1") == dict(limit=3.99, min_share=1.0)
    assert S.parse_matte_key_gain_arg("off") is None and S.parse_matte_key_gain_arg("") is None
    for text in ("auto", "0.9", "4", "2,1.5", "2,-0.1", "2,x", "2,0.1,0.1", "nan", ","):
        with pytest.raises(ValueError):
            S.parse_matte_key_gain_arg(text)
    ap_text = open(os.path.join(ROOT, "tools", "mjpeg_server.py")).read()
    assert '"--matte-key-gain"' in ap_text and 'nargs="?", const="on"' in ap_text and "parse_matte_key_gain_arg(ap_gain)" in ap_text
    # the grammars beside it stay as they are
    assert S.parse_matte_key_adapt_arg("0.25") == dict(rate=0.25, absorb=0.0)
    assert S.parse_matte_key_arg("capture,20,60") == dict(lo=20.0, hi=60.0, luma=0.25, radius=1, combine="replace", invert=False, to="capture")


def test_routes_refusals_and_the_producer():
    S = server()

    class W:
        """the producer's wrapper: echoes the frame, records the setting each frame ran under; posts from inside the loop"""
        matte_key = matte_key_adapt = matte_key_gain = None
        keyed = False

        def __init__(self):
            self.seen, self.got = [], []

        def set_matte_key(self, to, **kw):
            self.matte_key = dict(kw, to=to)

        def clear_matte_key(self):
            self.matte_key = self.matte_key_adapt = self.matte_key_gain = None

        def set_matte_key_gain(self, limit, min_share):
            if self.matte_key is None or isinstance(self.matte_key["to"], tuple):
                raise ValueError("set_matte_key_gain: refused")
            self.matte_key_gain, self.keyed = dict(limit=limit, min_share=min_share), False

        def clear_matte_key_gain(self):
            self.matte_key_gain = None

        def clear_matte_key_adapt(self):
            self.matte_key_adapt = None

        def matte_key_gain_measured(self):
            if self.matte_key_gain is None or not self.keyed:
                raise ValueError("matte_key_gain_measured: nothing yet")
            return (1.3125, 1.0, 0.796875), (0.5, 0.75, 1.0)

        def __call__(self, frame):
            if self.matte_key is not None and self.matte_key["to"] == "capture":
                self.matte_key = dict(self.matte_key, to="plate")
            self.keyed = self.matte_key_gain is not None
            self.seen.append(None if self.matte_key_gain is None else (self.matte_key_gain["limit"], self.matte_key_gain["min_share"]))
            n = len(self.seen)
            if n == 1:
                assert gain(b"on").startswith(b"HTTP/1.0 204")                       # no key yet: the wrapper refuses it
                self.got.append(get_gain())                                          # and there is nothing to report
            elif n == 2:
                assert key(b"00b140").startswith(b"HTTP/1.0 204")
                assert gain(b"on").startswith(b"HTTP/1.0 204")                       # a colour key: refused too
            elif n == 3:
                assert key(b"capture,20,60").startswith(b"HTTP/1.0 204")
                assert gain(b"on").startswith(b"HTTP/1.0 204")
                assert gain(b"1.5,0.125").startswith(b"HTTP/1.0 204")                # the newest request wins
                self.got.append(get_gain())                                          # asks; answered behind this frame: set, nothing keyed
            elif n == 4:
                self.got.append(get_gain())                                          # delivered: the setting, no measurement yet
                self.got.append(get_gain())                                          # asks again: behind this frame there is one
            elif n == 5:
                self.got.append(get_gain())                                          # delivered
                assert gain(b"off").startswith(b"HTTP/1.0 204")
            elif n == 6:
                assert gain(b"3").startswith(b"HTTP/1.0 204")
            elif n == 7:
                assert gain(b"").startswith(b"HTTP/1.0 204")                         # an empty body clears it
            elif n == 8:
                stop.set()
            return frame

    w = W()
    latest, stop = S.Latest(), threading.Event()
    keys = S.MatteKeyBox(w.matte_key, w.matte_key_adapt)
    keys.plate_wait = 0.0                        # (the producer runs in this thread: nothing could answer while a request waits)
    handler = S.make_handler(latest, keys=keys)
    key = lambda body: _request(handler, "POST", "/matte-key", body)
    gain = lambda body: _request(handler, "POST", "/matte-key/gain", body)
    get_gain = lambda: _request(handler, "GET", "/matte-key/gain")
    assert _request(S.make_handler(latest), "POST", "/matte-key/gain", b"on").startswith(b"HTTP/1.0 404")
    assert _request(S.make_handler(latest), "GET", "/matte-key/gain").startswith(b"HTTP/1.0 404")
    assert _request(handler, "POST", "/matte-key/gains", b"on").startswith(b"HTTP/1.0 404")
    for body in (b"auto", b"\xff\xfe", b"0.5", b"2,1.5", b"2,0.1,0.1"):
        assert gain(body).startswith(b"HTTP/1.0 400"), body
    assert keys.failed == 5
    assert gain(b"x" * 257).startswith(b"HTTP/1.0 413")
    S.produce(w, [b"\xff\xd8 a", b"\xff\xd8 b"], latest, stop, keys=keys)                # (in this thread)
    assert w.seen == [None, None, None, (1.5, 0.125), (1.5, 0.125), None, (3.0, 1 / 16), None]
    assert keys.failed == 7                      # the two requests the wrapper refused
    assert [g.split(b" ")[1] for g in w.got] == [b"404", b"404", b"200", b"404", b"200"]
    head, _, body = w.got[2].partition(b"\r\n\r\n")
    assert b"application/json" in head
    assert json.loads(body) == dict(limit=1.5, min_share=0.125, gain=None, share=None)
    assert json.loads(w.got[4].partition(b"\r\n\r\n")[2]) == dict(limit=1.5, min_share=0.125, gain=[1.3125, 1.0, 0.796875], share=[0.5, 0.75, 1.0])
    # GET /matte-key stays as it was: the key, and nothing of the gain
    base = dict(lo=20.0, hi=60.0, luma=0.25, radius=1, combine="replace", invert=False, to="plate")
    keys.put_gain(S.parse_matte_key_gain_arg("on"))
    keys.apply(w)
    assert w.matte_key_gain == dict(limit=2.0, min_share=1 / 16) and keys.current == base
    assert json.loads(_request(handler, "GET", "/matte-key").partition(b"\r\n\r\n")[2]) == base
    keys.put(None)
    keys.apply(w)
    assert keys.current is None and w.matte_key_gain is None
