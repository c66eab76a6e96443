"""Device-side JPEG output and input.  Output (csrc/jpeg.hip): the decoder's fp16 frame, or a uint8 frame,
becomes a JPEG file in three launches, and only the file crosses to the host.  Input (csrc/jpeg_dec.hip, section 8.z2):
`HipJpegDecoder` uploads the compressed file and decodes it in three launches into the uint8 frame the ingest op reads.

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


# ----------------------------------------------------------------------------- the decoder (csrc/jpeg_dec.hip)
DEFAULT_CHUNK_MCUS = 1         # MCUs per lane of the entropy kernel: the fastest of the sweep in profiles/jpeg_dec_time.txt (the
#                                kernel's time is a lane's serial walk, so it grows with the chunk; the index stays small)
GUARD = 16                     # bytes behind every decoder buffer that no kernel writes (the tests keep canaries there)
_BLOB = jpeg.DEC_BLOB_BYTES
_PARAMS = _BLOB                # int32 [4] behind the blob: scan offset, file length, the status word, unused
_OFFSETS = _PARAMS + 16
STATUS_TEXT = {1: "invalid Huffman code", 2: "coefficient index past 63", 4: "a chunk does not end where the next begins", 8: "bad index"}


class _DecSlot:
    """one of the two static slots of a geometry: the pinned staging buffer and its device twin (table blob | parameters and status
    word | index | file), the coefficient, plane and output buffers, the three-op plan"""

    def __init__(self, info: jpeg.JpegInfo, chunk_mcus: int, cap: int, device):
        dry = ops.DRY_RUN
        self.C = C = jpeg.chunk_layout(info.n_mcu, info.restart_interval, chunk_mcus)[3]
        self.pred_off = _OFFSETS + 4 * (C + 1)
        self.file_off = _round_up(self.pred_off + 6 * C, 16)
        self.cap = cap
        total = self.file_off + cap + 16                       # (16 bytes the reader may look ahead into)
        self.staging = torch.zeros(total, dtype=torch.uint8)
        if not dry:
            self.staging = self.staging.pin_memory()
        self.host = self.staging.numpy()
        self.offsets = self.host[_OFFSETS:self.pred_off].view(np.int32)
        self.dc_pred = self.host[self.pred_off:self.pred_off + 6 * C].view(np.int16).reshape(C, 3)
        self.params = self.host[_PARAMS:_PARAMS + 16].view(np.int32)
        self.dev = torch.zeros(total, dtype=torch.uint8, device=device)
        n_coef = info.n_mcu * info.blocks_per_mcu * 64
        H, W = info.height, info.width
        self.coef_buf = torch.zeros(n_coef + GUARD // 2, dtype=torch.int16, device=device)
        self.planes_buf = torch.zeros(n_coef + GUARD, dtype=torch.uint8, device=device)
        self.out_buf = torch.zeros(H * W * 3 + GUARD, dtype=torch.uint8, device=device)
        self.coef, self.planes = self.coef_buf[:n_coef], self.planes_buf[:n_coef]
        self.out = self.out_buf[:H * W * 3].view(H, W, 3)
        self.status_host = torch.zeros(1, dtype=torch.int32)
        if not dry:
            self.status_host = self.status_host.pin_memory()
        self.status_dev = self.dev[_PARAMS + 8:_PARAMS + 12].view(torch.int32)
        self.uploaded = self.checked = self.released = None
        d = self.dev
        pl = _lib.OpList()
        pl.append(*_flat(ops.jpeg_entropy_dec(
            d[self.file_off:], d[_OFFSETS:self.pred_off].view(torch.int32), d[self.pred_off:self.pred_off + 6 * C].view(torch.int16),
            d[:_BLOB], d[_PARAMS:_PARAMS + 8].view(torch.int32), self.coef, self.status_dev, n_mcu=info.n_mcu, ny=info.hs * info.vs,
            restart_interval=info.restart_interval, chunk_mcus=chunk_mcus, C=C, dc_tab=info.dc_tab, ac_tab=info.ac_tab)))
        pl.append(*_flat(ops.jpeg_idct(self.coef, d[jpeg.DEC_QUANT_OFF:_BLOB], self.planes, n_mcu=info.n_mcu, mcus_x=info.mcus_x,
                                       hs=info.hs, vs=info.vs)))
        pl.append(*_flat(ops.jpeg_rgb(self.planes, self.out, H=H, W=W, hs=info.hs, vs=info.vs)))
        self.plan = pl


class HipJpegDecoder:
    """JPEG files in, device uint8 [H,W,3] frames out, three launches per frame; everything runs on `torch.cuda.current_stream()`.

    Per frame the host parses the headers, builds the table blob and the chunk index (`l2d_jpeg_index`) straight into a pinned
    staging buffer beside the file, and ONE host-to-device copy takes all of it over.  `decode` returns a view of one of two
    static slots of the file's geometry, used in turn: valid until the decode after the next of that geometry (`release` takes a
    reader's event, as `HipFrameIO.release`).  Nothing in `decode` waits for the device: a scan the kernels found damaged sets a
    status word that is copied to a pinned word behind the plan and examined by `check()`, which the caller runs where it
    synchronises anyway.  Buffers and plans are cached per (size, sampling, restart interval, tables ids, chunk_mcus); the
    geometry may change from frame to frame.  Files outside the device's subset raise `jpeg.JpegUnsupported` before any work."""

    def __init__(self, device="cuda:0", chunk_mcus: int = DEFAULT_CHUNK_MCUS):
        if int(chunk_mcus) < 1:
            raise ValueError(f"HipJpegDecoder: chunk_mcus={chunk_mcus!r} must be at least 1")
        self.device, self.chunk_mcus = torch.device(device), int(chunk_mcus)
        self._geo = {}                 # key -> [slots, turn]
        self._pending = []             # slots whose status word has not been examined
        self._bad = 0                  # status bits of slots that were reused before a check()
        self.last_info = None

    def _geometry(self, info: jpeg.JpegInfo, nbytes: int) -> list:
        """[slots, turn] of the file's geometry"""
        key = (info.height, info.width, info.hs, info.vs, info.restart_interval, info.dc_tab, info.ac_tab, self.chunk_mcus)
        geo = self._geo.get(key)
        if geo is None or geo[0][0].cap < nbytes:
            # a file is rarely larger than half its raw frame; a larger one (or the first of its geometry) allocates and plans anew
            cap = _round_up(max(nbytes * 5 // 4, info.height * info.width // 2, 4096), 4096)
            if geo is None and len(self._geo) >= 8:            # a stream has one geometry, a test a handful
                self.check()
                self._geo.clear()
            geo = self._geo[key] = [[_DecSlot(info, self.chunk_mcus, cap, self.device) for _ in range(2)], 0]
        return geo

    def plan(self, info: jpeg.JpegInfo, nbytes: int) -> _lib.OpList:
        """the three-op plan of the slot the next file of this geometry goes to (dry-run validation; `decode` runs it)"""
        slots, turn = self._geometry(info, nbytes)
        return slots[turn].plan

    def decode(self, data) -> torch.Tensor:
        d = data if isinstance(data, bytes) else bytes(data)
        info = jpeg.parse(d)
        n = len(d)
        geo = self._geometry(info, n)
        slot = geo[0][geo[1]]
        geo[1] ^= 1
        cur = torch.cuda.current_stream()
        if slot.released is not None:
            cur.wait_event(slot.released)
            slot.released = None
        if slot.uploaded is not None:
            slot.uploaded.synchronize()              # the copy out of this staging buffer two frames ago (long done)
        if slot in self._pending:                    # its status word is about to be reused: look at it (two frames old, long
            self._pending.remove(slot)               # there) and keep what it says for the caller's next check()
            slot.checked.synchronize()
            self._bad |= int(slot.status_host[0])
        h = slot.host
        h[:_BLOB] = jpeg.table_blob(info)
        slot.params[:] = (info.scan_offset, n, 0, 0)
        ops.jpeg_index(info, d, self.chunk_mcus, h[:_BLOB], slot.offsets, slot.dc_pred)      # (ValueError: a damaged scan)
        h[slot.file_off:slot.file_off + n] = np.frombuffer(d, np.uint8)
        used = slot.file_off + n
        slot.dev[:used].copy_(slot.staging[:used], non_blocking=True)
        slot.uploaded = slot.uploaded or torch.cuda.Event()
        slot.uploaded.record(cur)
        slot.plan.run()
        slot.status_host.copy_(slot.status_dev, non_blocking=True)
        slot.checked = slot.checked or torch.cuda.Event()
        slot.checked.record(cur)
        self._pending.append(slot)
        self.last_info = info
        return slot.out

    def check(self) -> None:
        """raise ValueError if a scan decoded since the last check was damaged; waits only for the tiny copies behind those
        decodes, so where the caller has synchronised already (it has the frame's output) it waits for nothing"""
        pending, self._pending = self._pending, []
        bad, self._bad = self._bad, 0
        for slot in pending:
            slot.checked.synchronize()
            bad |= int(slot.status_host[0])
        if bad:
            why = ", ".join(t for b, t in STATUS_TEXT.items() if bad & b)
            raise ValueError(f"jpeg: the scan is damaged (device status {bad}: {why})")

    def release(self, view: torch.Tensor, event) -> None:
        """`event` was recorded behind the last read of `view` (a tensor `decode` returned) on another stream"""
        for slots, _ in self._geo.values():
            for slot in slots:
                if slot.out.data_ptr() == view.data_ptr():
                    slot.released = event
                    return
        raise ValueError("release: not a view of a decoder slot")
