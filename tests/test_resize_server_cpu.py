"""CPU test (-m "not gpu") of the output-size route of tools/mjpeg_server.py: `--output-size` / `POST /size` parsing and the producer
applying the newest request between two frames."""
import json
import os
import sys
import threading

import pytest

from test_style_bank_cpu import _request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mjpeg_server_size_route_and_option():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mjpeg_server as S
    finally:
        sys.path.pop(0)
    assert S.parse_size_arg("1920x1088") == dict(height=1088, width=1920, resample="lanczos")
    assert S.parse_size_arg(" 1024X768 , bicubic ") == dict(height=768, width=1024, resample="bicubic")
    assert S.parse_size_arg("640x480,bilinear") == dict(height=480, width=640, resample="bilinear")
    assert S.parse_size_arg("off") is None
    for text in ("", "1024", "1024x", "x768", "1024x768x3", "1024,768", "1024x768,", "1024x768,nearest", "10.5x768", "0x768", "1024x4112",
                 "1920x1080", "1000x768", "1936x1088", "axb"):
        with pytest.raises(ValueError):
            S.parse_size_arg(text)

    class W:
        """the producer's wrapper: echoes the frame, records the size each frame ran under; posts requests from inside the loop"""
        output_size = None

        def __init__(self):
            self.seen = []

        def set_output_size(self, height, width, resample="lanczos"):
            if height > 8 * 64:
                raise ValueError("refused")
            self.output_size = dict(height=height, width=width, resample=resample)

        def clear_output_size(self):
            self.output_size = None

        def __call__(self, frame):
            self.seen.append(self.output_size and dict(self.output_size))
            n = len(self.seen)
            if n == 1:
                assert post(b"128x96").startswith(b"HTTP/1.0 204")
            elif n == 2:
                assert post(b"256x256,bilinear").startswith(b"HTTP/1.0 204")
                assert post(b"512x128,bicubic").startswith(b"HTTP/1.0 204")          # the newest request wins
            elif n == 3:
                assert post(b"1920x1088").startswith(b"HTTP/1.0 204")                # the wrapper refuses it: nothing changes
            elif n == 4:
                assert post(b"off").startswith(b"HTTP/1.0 204")
            elif n == 5:
                stop.set()
            return frame

    w = W()
    latest, stop = S.Latest(), threading.Event()
    sizes = S.SizeBox(w.output_size)
    handler = S.make_handler(latest, None, None, None, None, sizes)
    post = lambda body: _request(handler, "POST", "/size", body)
    assert _request(S.make_handler(latest), "POST", "/size", b"off").startswith(b"HTTP/1.0 404")
    assert _request(S.make_handler(latest), "GET", "/size").startswith(b"HTTP/1.0 404")
    assert _request(handler, "GET", "/matte").startswith(b"HTTP/1.0 404")            # (the other routes are not served without their boxes)
    for body in (b"nonsense", b"\xff\xfe", b"1024x768,sharp", b"1000x768", b"128"):
        assert post(body).startswith(b"HTTP/1.0 400"), body
    assert post(b"1" * 300).startswith(b"HTTP/1.0 413")
    assert json.loads(_request(handler, "GET", "/size").partition(b"\r\n\r\n")[2]) is None
    S.produce(w, [b"\xff\xd8 a", b"\xff\xd8 b"], latest, stop, None, None, None, sizes)        # (in this thread)
    last = dict(height=128, width=512, resample="bicubic")
    assert w.seen == [None, dict(height=96, width=128, resample="lanczos"), last, last, None]
    assert sizes.failed == 1 and sizes.current is None
