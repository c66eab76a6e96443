"""CPU test (-m "not gpu") of the matte-source route of tools/mjpeg_server.py: `--matte-source` / `POST /matte-source` parsing and
the producer applying the newest request between two frames."""
import json
import os
import sys
import threading

import pytest

from test_style_bank_cpu import _request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mjpeg_server_matte_source_route_and_option():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mjpeg_server as S
    finally:
        sys.path.pop(0)
    assert S.parse_matte_source_arg("camera") == "camera" and S.parse_matte_source_arg(" stream\n") == "stream"
    for text in ("", "Camera", "host", "camera,stream", "off"):
        with pytest.raises(ValueError, match="use stream or camera"):
            S.parse_matte_source_arg(text)

    class W:
        """the producer's wrapper: echoes the frame, records the source each frame ran under; posts requests from inside the loop"""
        matte_source = "stream"
        refuse = False

        def __init__(self):
            self.seen = []

        def set_matte_source(self, source):
            if self.refuse:
                raise ValueError("refused")
            self.matte_source = source

        def __call__(self, frame):
            self.seen.append(self.matte_source)
            n = len(self.seen)
            if n == 1:
                assert post(b"camera").startswith(b"HTTP/1.0 204")
            elif n == 2:
                assert post(b"camera").startswith(b"HTTP/1.0 204")
                assert post(b"stream").startswith(b"HTTP/1.0 204")           # the newest request wins
            elif n == 3:
                self.refuse = True
                assert post(b"camera").startswith(b"HTTP/1.0 204")           # the wrapper refuses it: nothing changes
            elif n == 4:
                stop.set()
            return frame

    w = W()
    latest, stop = S.Latest(), threading.Event()
    sources = S.MatteSourceBox(w.matte_source)
    handler = S.make_handler(latest, None, None, None, None, None, sources)
    post = lambda body: _request(handler, "POST", "/matte-source", body)
    assert _request(S.make_handler(latest), "POST", "/matte-source", b"camera").startswith(b"HTTP/1.0 404")
    assert _request(S.make_handler(latest), "GET", "/matte-source").startswith(b"HTTP/1.0 404")
    assert _request(handler, "GET", "/size").startswith(b"HTTP/1.0 404")     # (the other routes are not served without their boxes)
    for body in (b"nonsense", b"\xff\xfe", b"off", b"Camera"):
        assert post(body).startswith(b"HTTP/1.0 400"), body
    assert post(b"c" * 300).startswith(b"HTTP/1.0 413")
    assert json.loads(_request(handler, "GET", "/matte-source").partition(b"\r\n\r\n")[2]) == "stream"
    S.produce(w, [b"\xff\xd8 a", b"\xff\xd8 b"], latest, stop, None, None, None, None, sources)      # (in this thread)
    assert w.seen == ["stream", "camera", "stream", "stream"]
    assert sources.failed == 1 and sources.current == "stream"
    assert json.loads(_request(handler, "GET", "/matte-source").partition(b"\r\n\r\n")[2]) == "stream"
    # the option: parsed by the same function, `stream` by default
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--matte-source", default="stream", type=S.parse_matte_source_arg)
    assert ap.parse_args([]).matte_source == "stream" and ap.parse_args(["--matte-source", "camera"]).matte_source == "camera"
    with pytest.raises(SystemExit):
        ap.parse_args(["--matte-source", "both"])
    with pytest.raises(SystemExit):
        S.main(["--config", "none.yaml", "--input", "post", "--matte-source", "both"])
