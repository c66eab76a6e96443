"""A running stream in a browser: frames -> StreamAnimateDiffusionDepthWrapper(output_type="jpeg") -> MJPEG over HTTP.

    python tools/mjpeg_server.py --config configs/toonyou.yaml --input frames/ [--prompt "..."] [--height 512 --width 512]
                                 [--port 8000] [--quality 75]

`/` is a page with one <img>; `/stream` is `multipart/x-mixed-replace; boundary=frame`, every part laid out as the reference's
demo does (demo/util.py:27-37, `jpeg.mjpeg_part`).  The input (a folder of images or an .npy stack, `stream_frames.read_frames`)
is looped for ever.  One producer thread owns the wrapper and the GPU; the HTTP handlers only ever read the latest part, so a
slow viewer drops frames instead of holding the stream back.  Standard library only (http.server).  The frame is encoded on
the device (jpeg_io.HipJpegEncoder): what crosses to the host is the JPEG file."""
import argparse
import os
import sys
import threading
from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

PAGE = (b"<!doctype html><html><head><title>live2diff_amd</title></head>"
        b"<body style=\"margin:0;background:#111\"><img src=\"/stream\" style=\"display:block;margin:auto;max-width:100%\"></body></html>\n")


class Latest:
    """The newest part and its sequence number.  `put` replaces it; `wait(seen)` blocks until there is a part newer than `seen`
    and returns `(seq, part)`, or None once the stream is closed and nothing newer is left."""

    def __init__(self):
        self._cond = threading.Condition()
        self._seq, self._part, self._closed = 0, None, False

    def put(self, part: bytes) -> None:
        with self._cond:
            self._seq, self._part = self._seq + 1, part
            self._cond.notify_all()

    def close(self) -> None:
        with self._cond:
            self._closed = True
            self._cond.notify_all()

    def wait(self, seen: int):
        with self._cond:
            self._cond.wait_for(lambda: self._seq > seen or self._closed)
            return (self._seq, self._part) if self._seq > seen else None


def make_handler(latest: Latest):
    class Handler(BaseHTTPRequestHandler):
        protocol_version = "HTTP/1.0"          # no keep-alive: the stream ends when either side closes the connection

        def log_message(self, fmt, *args):     # (one line per request on stderr is noise beside a 70 fps stream)
            pass

        def do_GET(self):
            if self.path in ("/", "/index.html"):
                self.send_response(200)
                self.send_header("Content-Type", "text/html; charset=utf-8")
                self.send_header("Content-Length", str(len(PAGE)))
                self.end_headers()
                self.wfile.write(PAGE)
            elif self.path == "/stream":
                self.send_response(200)
                self.send_header("Content-Type", "multipart/x-mixed-replace; boundary=frame")
                self.send_header("Cache-Control", "no-store")
                self.end_headers()
                seen = 0
                try:
                    while True:
                        got = latest.wait(seen)
                        if got is None:
                            break
                        seen, part = got
                        self.wfile.write(part)
                        self.wfile.flush()
                except (BrokenPipeError, ConnectionResetError):
                    pass                       # the viewer went away
            else:
                self.send_error(404)

    return Handler


def produce(wrapper, frames, latest: Latest, stop: threading.Event) -> None:
    """the producer: loops `frames` through the wrapper until `stop` is set"""
    from live2diff_amd.jpeg import mjpeg_part
    try:
        i = 0
        while not stop.is_set():
            latest.put(mjpeg_part(wrapper(frames[i % len(frames)])))
            i += 1
    finally:
        latest.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--input", required=True, help="folder of images, or .npy uint8 [F,H,W,3]; looped")
    ap.add_argument("--prompt", default=None, help="default: the config's `prompt`")
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--port", type=int, default=8000)
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--engine-dir", default="engines")
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args(argv)

    from stream_frames import read_frames

    from live2diff_amd.wrapper import StreamAnimateDiffusionDepthWrapper, load_config, stream_sizes
    cfg = load_config(args.config)
    sink = stream_sizes(cfg)[1]
    frames = read_frames(args.input)
    if len(frames) < sink:
        raise ValueError(f"{len(frames)} frames: need at least the {sink} warm-up frames")
    w = StreamAnimateDiffusionDepthWrapper(args.config, few_step_model_type="lcm", num_inference_steps=cfg.get("num_inference_steps", 50),
                                           t_index_list=cfg.get("t_index_list"), strength=cfg.get("strength"), output_type="jpeg",
                                           jpeg_quality=args.quality, height=args.height, width=args.width, seed=args.seed,
                                           engine_dir=args.engine_dir)
    w.prepare(frames[:sink], args.prompt if args.prompt is not None else str(cfg.get("prompt", "")))
    latest, stop = Latest(), threading.Event()
    producer = threading.Thread(target=produce, args=(w, frames, latest, stop), name="producer", daemon=True)
    server = ThreadingHTTPServer((args.host, args.port), make_handler(latest))
    server.daemon_threads = True
    producer.start()
    print(f"http://{args.host}:{args.port}/  ({args.height}x{args.width}, quality {args.quality}; Ctrl-C stops)")
    try:
        server.serve_forever()
    except KeyboardInterrupt:
        pass
    finally:
        stop.set()
        server.server_close()
        producer.join(timeout=10)


if __name__ == "__main__":
    main()
