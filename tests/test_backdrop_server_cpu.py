"""CPU test (-m "not gpu") of the backdrop route of tools/mjpeg_server.py: `--backdrop` / `POST /backdrop` parsing, an empty body
that clears it, 404 without the box, and the producer applying the newest request between two frames."""
import json
import os
import sys
import threading

import numpy as np
import pytest

from test_style_bank_cpu import _request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mjpeg_server_backdrop_route_and_option(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mjpeg_server as S
    finally:
        sys.path.pop(0)
    from PIL import Image
    room = str(tmp_path / "room.png")
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(room)
    assert S.parse_backdrop_arg("blur") == dict(to="blur", radius=6, passes=3)
    assert S.parse_backdrop_arg(" blur , 8\n") == dict(to="blur", radius=8, passes=3)
    assert S.parse_backdrop_arg("blur,1,1") == dict(to="blur", radius=1, passes=1)
    assert S.parse_backdrop_arg("00B140") == dict(to=(0, 177, 64))
    assert S.parse_backdrop_arg("ff00ff") == dict(to=(255, 0, 255))
    room_px = np.random.default_rng(1).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    Image.fromarray(room_px).save(room)
    got = S.parse_backdrop_arg(room)
    assert sorted(got) == ["to"] and got["to"].dtype == np.uint8 and np.array_equal(got["to"], room_px)      # decoded by the parser
    junk = str(tmp_path / "notes.txt")
    with open(junk, "w") as f:
        f.write("an existing file that is no image\n")
    with pytest.raises(ValueError, match="cannot be read as an image"):
        S.parse_backdrop_arg(junk)
    assert S.parse_backdrop_arg(" off ") is None and S.parse_backdrop_arg("") is None
    for text in ("blur,0", "blur,9", "blur,2.0", "blur,two", "blur,6,0", "blur,6,4", "blur,6,3,1", "blur,", "00B14", "00B14G", "#00B140",
                 str(tmp_path / "missing.png"), "on", "blurry"):
        with pytest.raises(ValueError, match="backdrop"):
            S.parse_backdrop_arg(text)

    class W:
        """the producer's wrapper: echoes the frame, records the setting each frame ran under; posts requests from inside the loop"""
        backdrop = None
        refuse = False

        def __init__(self):
            self.seen = []

        def set_backdrop(self, to="blur", *, radius=6, passes=3):
            if self.refuse:
                raise ValueError("refused")
            kind = "blur" if isinstance(to, str) else "color" if isinstance(to, tuple) else "image"
            self.backdrop = dict(to=kind, radius=radius, passes=passes, color=to if kind == "color" else None)

        def clear_backdrop(self):
            self.backdrop = None

        def __call__(self, frame):
            self.seen.append(self.backdrop)
            n = len(self.seen)
            if n == 1:
                assert post(b"blur").startswith(b"HTTP/1.0 204")
            elif n == 2:
                assert post(b"blur,2,1").startswith(b"HTTP/1.0 204")
                assert post(b"00B140").startswith(b"HTTP/1.0 204")           # the newest request wins
            elif n == 3:
                assert post(room.encode()).startswith(b"HTTP/1.0 204")
            elif n == 4:
                assert post(b"").startswith(b"HTTP/1.0 204")                 # an empty body clears it
            elif n == 5:
                self.refuse = True
                assert post(b"blur").startswith(b"HTTP/1.0 204")             # the wrapper refuses it: nothing changes
            elif n == 6:
                stop.set()
            return frame

    def settings(kind, radius=6, passes=3, color=None):
        return dict(to=kind, radius=radius, passes=passes, color=color)

    w = W()
    latest, stop = S.Latest(), threading.Event()
    backdrops = S.BackdropBox(w.backdrop)
    handler = S.make_handler(latest, backdrops=backdrops)
    post = lambda body: _request(handler, "POST", "/backdrop", body)          # noqa: E731
    assert _request(S.make_handler(latest), "POST", "/backdrop", b"blur").startswith(b"HTTP/1.0 404")
    assert _request(S.make_handler(latest), "GET", "/backdrop").startswith(b"HTTP/1.0 404")
    # (every earlier caller passes at most nine positional arguments: the box is a keyword behind them, None by default)
    assert _request(S.make_handler(latest, None, None, None, None, None, None, None, None), "GET", "/backdrop").startswith(b"HTTP/1.0 404")
    assert _request(handler, "GET", "/detail").startswith(b"HTTP/1.0 404")       # (the other routes are not served without their boxes)
    assert _request(S.make_handler(latest, details=S.DetailBox()), "POST", "/detail", b"").startswith(b"HTTP/1.0 400")   # (theirs stay as they were)
    for body in (b"nonsense", b"\xff\xfe", b"blur,0", b"blur,9", b"blur,6,4", b"00B14", b"/no/such/file.png", junk.encode()):
        assert post(body).startswith(b"HTTP/1.0 400"), body
    assert post(b"b" * 300).startswith(b"HTTP/1.0 413")
    assert json.loads(_request(handler, "GET", "/backdrop").partition(b"\r\n\r\n")[2]) is None
    S.produce(w, [b"\xff\xd8 a", b"\xff\xd8 b"], latest, stop, backdrops=backdrops)      # (in this thread)
    assert w.seen == [None, settings("blur"), settings("color", color=(0, 177, 64)), settings("image"), None, None]
    assert backdrops.failed == 1 and backdrops.current is None
    backdrops.put(dict(to="blur", radius=3, passes=2))
    w.refuse = False
    backdrops.apply(w)
    assert json.loads(_request(handler, "GET", "/backdrop").partition(b"\r\n\r\n")[2]) == settings("blur", 3, 2)
    backdrops.put(dict(to=(1, 2, 3)))
    backdrops.apply(w)
    assert json.loads(_request(handler, "GET", "/backdrop").partition(b"\r\n\r\n")[2]) == settings("color", color=[1, 2, 3])
    import inspect
    for fn in (S.make_handler, S.produce, S.produce_posted):
        p = inspect.signature(fn).parameters["backdrops"]
        assert p.default is None, fn
    # the option: refused by the same function before anything is loaded
    with pytest.raises(ValueError, match="backdrop"):
        S.main(["--config", "none.yaml", "--input", "post", "--backdrop", "blur,9"])
    with pytest.raises(ValueError, match="backdrop"):
        S.main(["--config", "none.yaml", "--input", "post", "--backdrop", "no-such-file.png"])
    with pytest.raises(ValueError, match="cannot be read as an image"):
        S.main(["--config", "none.yaml", "--input", "post", "--backdrop", junk])
