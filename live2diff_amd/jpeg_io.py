"""Device-side JPEG output (csrc/jpeg.hip): the decoder's fp16 frame, or a uint8 frame, becomes a JPEG
file in three launches, and only the file crosses to the host.

`HipJpegEncoder` owns what one `(height, width, quality)` needs: the uploaded Huffman tables and header, and per batch size the
coefficient buffer, the row staging buffer, the output buffer, a pinned host buffer and the three-op plan.  Everything runs on
`torch.cuda.current_stream()`.  The format, its host restatement (`encode_ref`, the kernels' oracle) and the size bounds are in
`live2diff_amd/jpeg.py`.
"""
from typing import List, Union

import numpy as np
import torch

from . import _lib, jpeg, ops

FIRST_CHUNK = 64 * 1024        # bytes of the first device-to-host copy until a larger frame has been seen


def _round_up(n: int, m: int) -> int:
    return -(-n // m) * m


class _Batch:
    def __init__(self, enc: "HipJpegEncoder", B: int):
        H, W, dev = enc.height, enc.width, enc.device
        R = H // 16
        self.coef = torch.empty(B * R * (W // 16) * 6 * 64, dtype=torch.int16, device=dev)
        self.staging = torch.empty(B * R * enc.row_stride, dtype=torch.uint8, device=dev)
        self.lengths = torch.zeros(B * R, dtype=torch.int32, device=dev)
        self.out = torch.zeros(B, enc.out_stride, dtype=torch.uint8, device=dev)
        self.host = None if ops.DRY_RUN else torch.zeros(B, enc.out_stride, dtype=torch.uint8).pin_memory()
        self.src_key = None
        self.plan = None


class HipJpegEncoder:
    def __init__(self, height: int, width: int, quality: int = 75, device="cuda:0"):
        jpeg._check(height, width, quality)
        if width > ops.JPEG_MAX_W:
            raise ValueError(f"HipJpegEncoder: width {width} exceeds {ops.JPEG_MAX_W} (an MCU row is entropy-coded in LDS)")
        self.height, self.width, self.quality, self.device = int(height), int(width), int(quality), torch.device(device)
        self.header = jpeg.header(self.height, self.width, self.quality)
        self.row_stride = _round_up(jpeg.row_capacity(self.width), 16)
        self.out_stride = _round_up(ops.JPEG_HDR_OFF + len(self.header) + (self.height // 16) * self.row_stride, 16)
        self._tables = torch.from_numpy(jpeg.tables(self.quality).packed().copy()).to(self.device)
        self._header = torch.frombuffer(bytearray(self.header), dtype=torch.uint8).to(self.device)
        self._batches = {}
        self._chunk = min(FIRST_CHUNK, self.out_stride)
        self.last_copies = 0           # device-to-host copies of the last `encode` (per frame: 1, or 2 after a frame outgrew the chunk)
        self.last_copied_bytes = 0

    def plan(self, src: torch.Tensor, B: int) -> _lib.OpList:
        """the three-op plan of batch size B reading `src` (kept while `src` stays the same buffer: a static decoder output)"""
        bt = self._batches.get(B)
        if bt is None:
            bt = self._batches[B] = _Batch(self, B)
        key = (src.data_ptr(), src.dtype)
        if bt.src_key != key:
            H, W = self.height, self.width
            pl = _lib.OpList()
            pl.append(*_flat(ops.jpeg_dct(src, bt.coef, B=B, H=H, W=W, quality=self.quality)))
            pl.append(*_flat(ops.jpeg_huff(bt.coef, self._tables, bt.staging, bt.lengths, B=B, H=H, W=W, row_stride=self.row_stride)))
            pl.append(*_flat(ops.jpeg_pack(bt.staging, bt.lengths, self._header, bt.out, B=B, H=H, row_stride=self.row_stride,
                                           out_stride=self.out_stride)))
            bt.plan, bt.src_key = pl, key
        return bt.plan

    def _source(self, image: torch.Tensor):
        H, W = self.height, self.width
        if not torch.is_tensor(image) or not (image.is_cuda or ops.DRY_RUN) or image.dtype not in (torch.float16, torch.uint8):
            raise ValueError(f"jpeg encode: expected a device fp16 [3,{H},{W}] / [B,3,{H},{W}] or uint8 [{H},{W},3] / [B,{H},{W},3] tensor, "
                             f"got {getattr(image, 'dtype', type(image))} on {getattr(image, 'device', 'the host')}")
        single = image.ndim == 3
        if single:
            image = image[None]
        want = (3, H, W) if image.dtype == torch.float16 else (H, W, 3)
        if image.ndim != 4 or tuple(image.shape[1:]) != want:
            raise ValueError(f"jpeg encode: expected [B,{', '.join(map(str, want))}] for {image.dtype}, got {tuple(image.shape)}")
        return (image if image.is_contiguous() else image.contiguous()), single

    def encode(self, image: torch.Tensor, to_host: bool = True) -> Union[bytes, List[bytes], tuple]:
        """device fp16 [3,H,W] / [B,3,H,W] in [-1, 1] (encoded as the bytes the egress op would return) or device uint8 [H,W,3] /
        [B,H,W,3] -> the JPEG file as `bytes` (a list for a batch).  `to_host=False`: `(uint8 [capacity] device buffer, int32
        device length)` of the static output slot ([B, capacity] / [B] for a batch), valid until the next encode of that batch size.

        The copy to the host is the file, not the capacity: the length word and the first `chunk` bytes come in one copy; only a
        frame that is larger takes a second copy for the rest (and makes the chunk grow to 1.25 x that frame, so the frames after
        it take one again)."""
        src, single = self._source(image)
        B = src.shape[0]
        self.plan(src, B).run()
        bt = self._batches[B]
        off = ops.JPEG_HDR_OFF
        if not to_host:
            n = bt.out[:, :4].view(torch.int32)[:, 0]
            return (bt.out[0, off:], n[0]) if single else (bt.out[:, off:], n)
        chunk = self._chunk
        cur = torch.cuda.current_stream()
        for b in range(B):
            bt.host[b, :chunk].copy_(bt.out[b, :chunk], non_blocking=True)
        cur.synchronize()
        host = bt.host.numpy()
        sizes = [int(host[b, :4].view(np.int32)[0]) for b in range(B)]
        self.last_copies, self.last_copied_bytes = B, B * chunk
        late = [b for b in range(B) if off + sizes[b] > chunk]
        if late:
            for b in late:
                bt.host[b, chunk:off + sizes[b]].copy_(bt.out[b, chunk:off + sizes[b]], non_blocking=True)
                self.last_copied_bytes += off + sizes[b] - chunk
            cur.synchronize()
            self.last_copies += len(late)
            self._chunk = min(self.out_stride, _round_up((off + max(sizes)) * 5 // 4, 4096))
        files = [host[b, off:off + sizes[b]].tobytes() for b in range(B)]
        return files[0] if single else files


def _flat(op_and_keep):
    op, keep = op_and_keep
    return (op, *keep)
