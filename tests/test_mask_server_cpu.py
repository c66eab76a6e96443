"""CPU test (-m "not gpu") of the mask routes of tools/mjpeg_server.py: `--mask` / `POST /mask` (an image file decoded on the
host, an empty body or `off` clears the sticky mask), `--mask-input` / `POST /mask-input`, bodies that get a 400 and are counted,
and the producer applying the newest request between two frames."""
import io
import json
import os
import sys
import threading

import numpy as np
import pytest

from test_style_bank_cpu import _request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def png(arr) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG")
    return buf.getvalue()


def test_mjpeg_server_mask_routes_and_options():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mjpeg_server as S
    finally:
        sys.path.pop(0)
    assert S.parse_mask_input_arg("replace") == dict(combine="replace", invert=False)
    assert S.parse_mask_input_arg(" and , invert ") == dict(combine="and", invert=True)
    assert S.parse_mask_input_arg("or") == dict(combine="or", invert=False)
    for text in ("", "xor", "and,", "and,flip", "and,invert,invert", "invert", "off"):
        with pytest.raises(ValueError, match="mask input"):
            S.parse_mask_input_arg(text)
    rng = np.random.default_rng(1)
    m8 = rng.integers(0, 256, (30, 54), dtype=np.uint8)
    m16 = rng.integers(0, 65536, (24, 40)).astype(np.uint16)
    assert np.array_equal(S.parse_mask_body(png(m8)), m8)
    got = S.parse_mask_body(png(m16))
    assert got.dtype == np.uint16 and np.array_equal(got, m16)
    assert S.parse_mask_body(b"") is None and S.parse_mask_body(b"off") is None and S.parse_mask_body(b" off\n") is None
    for body in (b"on", b"\x89PNG\r\n\x1a\n garbage", png(np.zeros((8, 8, 3), np.uint8)), png(m8)[:40]):
        with pytest.raises(ValueError):
            S.parse_mask_body(body)
    ap_text = open(os.path.join(ROOT, "tools", "mjpeg_server.py")).read()
    assert '"--mask"' in ap_text and '"--mask-input"' in ap_text and "parse_mask_input_arg(args.mask_input)" in ap_text

    class W:
        """the producer's wrapper: echoes the frame, records the mask and the input each frame ran under; posts from inside the loop"""
        mask_input = dict(combine="replace", invert=False)
        sticky = None

        def __init__(self):
            self.seen = []

        def set_mask(self, mask):
            if mask.shape == (7, 7):
                raise ValueError("mask: refused")
            self.sticky = mask

        def clear_mask(self):
            self.sticky = None

        def set_mask_input(self, combine="replace", invert=False):
            self.mask_input = dict(combine=combine, invert=invert)

        def __call__(self, frame):
            self.seen.append((None if self.sticky is None else self.sticky.shape, dict(self.mask_input)))
            n = len(self.seen)
            if n == 1:
                assert post(png(m8)).startswith(b"HTTP/1.0 204")
            elif n == 2:
                assert post(png(m8)).startswith(b"HTTP/1.0 204")
                assert post(png(m16)).startswith(b"HTTP/1.0 204")                    # the newest request wins
                assert post_input(b"and,invert").startswith(b"HTTP/1.0 204")
            elif n == 3:
                assert post(png(np.zeros((7, 7), np.uint8))).startswith(b"HTTP/1.0 204")      # the wrapper refuses it: nothing changes
            elif n == 4:
                assert post(b"").startswith(b"HTTP/1.0 204")                         # an empty body clears it
            elif n == 5:
                assert post(png(m8)).startswith(b"HTTP/1.0 204")
                assert post_input(b"or").startswith(b"HTTP/1.0 204")
            elif n == 6:
                assert post(b"off").startswith(b"HTTP/1.0 204")
            elif n == 7:
                stop.set()
            return frame

    w = W()
    latest, stop = S.Latest(), threading.Event()
    masks = S.MaskBox(None, w.mask_input)
    handler = S.make_handler(latest, masks=masks)
    post = lambda body: _request(handler, "POST", "/mask", body)
    post_input = lambda body: _request(handler, "POST", "/mask-input", body)
    for path in ("/mask", "/mask-input"):
        assert _request(S.make_handler(latest), "POST", path, b"and").startswith(b"HTTP/1.0 404")
        assert _request(S.make_handler(latest), "GET", path).startswith(b"HTTP/1.0 404")
    # bad bodies: a 400 each, and counted
    for body in (b"on", b"\xff\xfe", png(np.zeros((8, 8, 3), np.uint8)), png(m8)[:40]):
        assert post(body).startswith(b"HTTP/1.0 400"), body
    for body in (b"", b"xor", b"and,flip", b"\xff\xfe"):
        assert post_input(body).startswith(b"HTTP/1.0 400"), body
    assert masks.failed == 8
    assert _request(handler, "POST", "/mask", b"x", length=S.MAX_POST + 1).startswith(b"HTTP/1.0 413")
    assert json.loads(_request(handler, "GET", "/mask").partition(b"\r\n\r\n")[2]) is None
    assert json.loads(_request(handler, "GET", "/mask-input").partition(b"\r\n\r\n")[2]) == dict(combine="replace", invert=False)
    S.produce(w, [b"\xff\xd8 a", b"\xff\xd8 b"], latest, stop, masks=masks)              # (in this thread)
    rep, flipped, either = dict(combine="replace", invert=False), dict(combine="and", invert=True), dict(combine="or", invert=False)
    assert w.seen == [(None, rep), ((30, 54), rep), ((24, 40), flipped), ((24, 40), flipped), (None, flipped), ((30, 54), either),
                      (None, either)]
    assert masks.failed == 9 and masks.current is None and masks.current_input == either
    masks.put(S.parse_mask_body(png(m8)))
    masks.apply(w)
    assert masks.current == dict(size=[30, 54])
    assert json.loads(_request(handler, "GET", "/mask").partition(b"\r\n\r\n")[2]) == dict(size=[30, 54])
    assert json.loads(_request(handler, "GET", "/mask-input").partition(b"\r\n\r\n")[2]) == either
