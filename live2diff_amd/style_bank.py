"""Style switch and style blend from resident packed weight sets.

A style is a DreamBooth checkpoint plus LoRAs merged into the UNet and the text encoder.  Every plan of `HipStreamingUNet` and
`HipClipTextEncoder` holds raw pointers into one flat set of packed device tensors, and the packed layout depends on the stream
shape and the kernel choice, not on the style -- so overwriting those tensors in place, in stream order between two frames,
changes the style while plans, hipGraphs, KV caches and the stream batch stay as they are.  An affine combination of packed sets
is a valid network too: a folded LayerNorm pair (gamma * W, colsum, beta W + b) is a linear layer on the normalised input, and
everything else mixes like a weighted-sum checkpoint merge.

  * `blend_ref`      the arithmetic of L2D_OP_WEIGHT_BLEND in numpy float32 -- the kernel's oracle;
  * `WeightBlender`  the table of tile records per (destination, sources) combination, kept on the device, and the one launch;
  * `StyleBank`      named sets (UNet + text encoder) kept resident, and the current mix.
"""
import math
from collections import OrderedDict
from typing import Dict, List, Sequence

import numpy as np
import torch

from . import _lib, ops

MAX_SOURCES = ops.WBLEND_MAX_SRC
SUM_TOL = 1e-6


def check_weights(weights: Sequence[float], n_sources: int) -> List[float]:
    """finite, one per source, summing to 1 within 1e-6, at most four non-zero -> the weights as floats"""
    w = [float(a) for a in weights]
    if len(w) != n_sources or not w:
        raise ValueError(f"{len(w)} weights for {n_sources} sources: need one weight per source and at least one source")
    if not all(math.isfinite(a) for a in w):
        raise ValueError(f"blend weights {w} must be finite")
    if abs(math.fsum(w) - 1.0) > SUM_TOL:
        raise ValueError(f"blend weights {w} sum to {math.fsum(w)!r}, need 1 within {SUM_TOL} (an affine combination)")
    if sum(1 for a in w if a != 0.0) > MAX_SOURCES:
        raise ValueError(f"{sum(1 for a in w if a != 0.0)} non-zero blend weights: at most {MAX_SOURCES} sources per launch")
    return w


def drop_zero_terms(sources: Sequence, weights: Sequence[float]):
    """Terms whose weight is exactly 0 leave before the launch is built: a one-hot mix is then the K = 1 copy, bit for bit
    (-0.0 + 0 * x would turn into +0.0 otherwise)."""
    keep = [(s, a) for s, a in zip(sources, weights) if a != 0.0]
    return [s for s, _ in keep], [a for _, a in keep]


def blend_ref(sources: Sequence[Dict[str, torch.Tensor]], weights: Sequence[float]) -> Dict[str, torch.Tensor]:
    """L2D_OP_WEIGHT_BLEND on the host: per tensor acc = a_0 s_0, then acc = acc + a_k s_k in source order, every product and
    every sum rounded to fp32 on its own (numpy has no fma), one round-to-nearest-even to the tensor's dtype at the end.  Dicts of
    CPU tensors in, a dict of CPU tensors out."""
    w = check_weights(weights, len(sources))
    sources, w = drop_zero_terms(sources, w)
    out = {}
    for name, t0 in sources[0].items():
        if t0.dtype not in ops.WBLEND_DTYPES:
            raise TypeError(f"{name}: dtype {t0.dtype} cannot be blended (fp16 and fp32 only)")
        if len(w) == 1 and np.float32(w[0]) == 1.0:        # the copy moves bits (1 * x would quieten a signalling NaN)
            out[name] = t0.detach().cpu().contiguous().clone()
            continue
        acc = None
        for s, a in zip(sources, w):
            term = np.float32(a) * s[name].detach().cpu().contiguous().numpy().astype(np.float32)
            acc = term if acc is None else acc + term
        assert acc.dtype == np.float32
        out[name] = torch.from_numpy(np.ascontiguousarray(acc.astype(np.float16 if t0.dtype == torch.float16 else np.float32)))
    return out


def _tiles(t: torch.Tensor):
    """byte offsets and element counts of the tiles of one tensor"""
    es = t.element_size()
    nbytes = t.numel() * es
    off = np.arange(0, nbytes, ops.WBLEND_TILE_BYTES, dtype=np.int64)
    n = np.minimum(nbytes - off, ops.WBLEND_TILE_BYTES) // es
    return off, n


class WeightBlender:
    """dst_t = sum_k a_k src_{k,t} over a whole set of tensors in one launch, in place, on the current stream."""

    MAX_TABLES = 8           # (destination, sources) tables kept; the oldest leaves first

    def __init__(self, dst_tensors: Dict[str, torch.Tensor], device=None):
        self.dst = dict(dst_tensors)
        if not self.dst:
            raise ValueError("WeightBlender: empty destination set")
        self.device = torch.device(device) if device is not None else next(iter(self.dst.values())).device
        for name, t in self.dst.items():
            self._check_tensor(name, t, "destination")
        self._tables = OrderedDict()

    def _check_tensor(self, name, t, what):
        if not torch.is_tensor(t) or t.dtype not in ops.WBLEND_DTYPES:
            raise TypeError(f"{what} tensor {name}: dtype {getattr(t, 'dtype', type(t))} cannot be blended (fp16 and fp32 only)")
        if not t.is_contiguous():
            raise ValueError(f"{what} tensor {name} is not contiguous")
        if t.device.type != self.device.type or (t.device.index is not None and self.device.index is not None
                                                 and t.device.index != self.device.index):
            raise ValueError(f"{what} tensor {name} is on {t.device}, the blender on {self.device}")

    def check_source(self, src: Dict[str, torch.Tensor], what: str = "source") -> None:
        """same names, shapes and dtypes as the destination"""
        if set(src) != set(self.dst):
            odd = sorted(set(src) ^ set(self.dst))
            raise ValueError(f"{what} set does not hold the destination's tensors: {len(odd)} names differ, e.g. {odd[:3]}")
        for name, d in self.dst.items():
            s = src[name]
            self._check_tensor(name, s, what)
            if s.dtype != d.dtype:
                raise TypeError(f"{what} tensor {name}: dtype {s.dtype}, the destination has {d.dtype}")
            if tuple(s.shape) != tuple(d.shape):
                raise ValueError(f"{what} tensor {name}: shape {tuple(s.shape)}, the destination has {tuple(d.shape)}")

    def _table(self, sources):
        key = tuple(id(s) for s in sources)
        hit = self._tables.get(key)
        if hit is not None and all(a is b for a, b in zip(hit[2], sources)):
            self._tables.move_to_end(key)
            return hit
        for j, s in enumerate(sources):
            self.check_source(s, f"source {j}")
        parts = []
        for name, d in self.dst.items():
            if d.numel() == 0:
                continue
            off, n = _tiles(d)
            rec = np.zeros(len(off), dtype=ops.WBLEND_REC)
            rec["dst"] = d.data_ptr() + off
            for k, s in enumerate(sources):
                rec["src"][:, k] = s[name].data_ptr() + off
            rec["n"], rec["dtype"] = n, ops.WBLEND_DTYPES[d.dtype]
            parts.append(rec)
        host = np.ascontiguousarray(np.concatenate(parts))
        dev = torch.from_numpy(host.view(np.uint8).reshape(-1).copy()).to(self.device)
        hit = (dev, host, tuple(sources))           # (the sources stay referenced: their ids and pointers stay valid)
        self._tables[key] = hit
        while len(self._tables) > self.MAX_TABLES:
            self._tables.popitem(last=False)
        return hit

    def forget(self, source: Dict[str, torch.Tensor]) -> None:
        """drop every table that reads `source` (a table keeps its sources alive)"""
        for key in [k for k, hit in self._tables.items() if any(s is source for s in hit[2])]:
            del self._tables[key]

    def op(self, sources: Sequence[Dict[str, torch.Tensor]], weights: Sequence[float], nt=None):
        """the launch record (and what it keeps alive) of one blend"""
        w = check_weights(weights, len(sources))
        sources, w = drop_zero_terms(sources, w)
        dev, host, _ = self._table(sources)
        return ops.weight_blend(dev, host, w, nt=nt)

    def apply(self, sources: Sequence[Dict[str, torch.Tensor]], weights: Sequence[float], nt=None) -> None:
        """enqueue the blend on torch.cuda.current_stream(); no host / device synchronisation"""
        ops.run(self.op(sources, weights, nt=nt))

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.dst.values())


def clone_set(packed):
    """a private copy of a `PackedWeights` (the active tensors are scratch that the next switch overwrites)"""
    from .unet_hip import PackedWeights
    return PackedWeights({k: v.detach().clone() for k, v in packed.W.items()}, dict(packed.meta))


def parse_style(style, known) -> Dict[str, float]:
    """a name or {name: weight} -> {name: weight} with checked names and weights"""
    if isinstance(style, str):
        style = {style: 1.0}
    if not isinstance(style, dict) or not style:
        raise ValueError(f"style={style!r}: use a style name or a dict {{name: weight}}")
    if len(style) > MAX_SOURCES:
        raise ValueError(f"style mixes {len(style)} sets: at most {MAX_SOURCES}")
    for name in style:
        if name not in known:
            raise KeyError(f"unknown style {name!r}: registered styles are {sorted(known)}")
    names = list(style)
    try:
        w = [float(style[n]) for n in names]
    except (TypeError, ValueError):
        raise ValueError(f"style={style!r}: weights must be numbers") from None
    return dict(zip(names, check_weights(w, len(names))))


class StyleBank:
    """Named (UNet set, text-encoder set) pairs kept resident, and the current mix."""

    def __init__(self):
        self.sets = OrderedDict()          # name -> (unet PackedWeights, text PackedWeights)
        self.current = {}

    def add(self, name: str, unet_set, text_set) -> None:
        if not isinstance(name, str) or not name:
            raise ValueError(f"style name {name!r}: use a non-empty string")
        if name in self.sets:
            raise ValueError(f"style {name!r} is registered already: remove_style it first")
        self.sets[name] = (unet_set, text_set)

    def remove(self, name: str) -> None:
        if name not in self.sets:
            raise KeyError(f"unknown style {name!r}: registered styles are {sorted(self.sets)}")
        if self.current.get(name, 0.0) != 0.0:
            raise ValueError(f"style {name!r} is part of the current mix {self.current}: set_style another one first")
        del self.sets[name]

    @property
    def names(self) -> List[str]:
        return list(self.sets)
