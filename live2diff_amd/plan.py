"""What the static launch plans of the four networks (UNet, AutoencoderKL, tiny VAE, DPT-Hybrid) share.

A plan is an `_lib.OpList` of `l2d_op` records built once per shape and replayed by the native executor.  The networks keep their
topology; `PlanBuilder` is the plumbing underneath: the op list(s), the arena the intermediates come from, the implicit GEMM with its
schedule, the split-K workspaces and arrival counters of igemm / cconv / wsgemm, and the GroupNorm whose statistics come from the
producing launch where that launch can deliver them.  The builder is also the plan's state: the networks hang their static input /
output buffers on it, and tests and tools read `pl`, `sk_cnt`, `sk_used`, `gn_acc`, `gn_layers`, `arena_bytes`, `n_ops`, `kinds` off it.
"""
from typing import Dict, List, Optional

import torch

from . import _lib, ops
from .ops import round_up


class Arena:
    """Size-keyed free list of device buffers: intermediates of a static plan reuse HBM (and stay hot in the
    256 MB Infinity Cache) instead of every op getting a private allocation."""

    def __init__(self, device):
        self.device = device
        self.free: Dict[tuple, List[torch.Tensor]] = {}
        self.all: List[torch.Tensor] = []

    def alloc(self, numel: int, dtype=torch.float16) -> torch.Tensor:
        key = (int(numel), dtype)
        lst = self.free.get(key)
        if lst:
            return lst.pop()
        t = torch.empty(int(numel), dtype=dtype, device=self.device)
        self.all.append(t)
        return t

    def release(self, t: Optional[torch.Tensor]):
        if t is not None:
            self.free.setdefault((t.numel(), t.dtype), []).append(t)

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.all)


class Act:
    """channels-last activation: buf holds [B*H*W, C] halfs (ld == C); `producer` = the igemm op that wrote it (if any)."""
    __slots__ = ("buf", "C", "H", "W", "producer")

    def __init__(self, buf, C, H, W, producer=None):
        self.buf, self.C, self.H, self.W, self.producer = buf, C, H, W, producer


class PlanBuilder:
    def __init__(self, device, B: int, *, sk_counters: int = 0, gn_layers: int = 0, G: int = 32, xcd_order: bool = True):
        """B: samples on the batch axis.  sk_counters: size of the split-K arrival-counter block (0: this network never splits K).
        gn_layers: GroupNorms that may take their statistics from their producers -- one [B][G][2] int64 accumulator block each,
        zeroed by the plan's first op.  xcd_order: igemm launches pick their XCD tile order by the rule in `gemm`."""
        self.device, self.B, self.G, self.xcd_order = device, B, G, xcd_order
        self.arena = Arena(device)
        self.pl = self._cur = _lib.OpList()
        self.kinds: Dict[int, int] = {}              # launches of `pl` per op kind
        # arrival counters of the split-K launches (fused reduction): zero now, every launch leaves them zero
        self.sk_cnt, self.sk_used = torch.zeros(sk_counters, dtype=torch.int32, device=device), 0
        self.gn_layers, self.gn_self_launches, self.gn_stats_launches = 0, 0, 0
        self.gn_acc = self._zero_op = None
        if gn_layers:
            self.gn_acc = torch.zeros(gn_layers, B, G, 2, dtype=torch.int64, device=device)
            self.gn_zero = torch.zeros_like(self.gn_acc)
            self._zero_op = self.add(ops.copy(self.gn_zero, self.gn_acc, self.gn_acc.numel() * 8))

    # ------------------------------------------------------------------ op lists, buffers
    def use(self, pl):
        """Later ops go to `pl` (the UNet builds its conditioning launches into a list of their own)."""
        self._cur = pl

    def add(self, opk):
        op, keep = opk
        self._cur.append(op, *keep)
        if self._cur is self.pl:
            self.kinds[op.kind] = self.kinds.get(op.kind, 0) + 1
        return op

    def act(self, C, H, W, ld=None) -> Act:
        return Act(self.arena.alloc(self.B * H * W * (ld or C)), C, H, W)

    def free(self, a: Optional[Act]):
        if a is not None:
            self.arena.release(a.buf)

    # ------------------------------------------------------------------ GEMMs with split-K
    def _counters(self, n: int) -> dict:
        off, self.sk_used = self.sk_used, self.sk_used + n
        return dict(cnt=self.sk_cnt, cnt_off=off)

    def gemm(self, x1, wt, out, **kw):
        """igemm with the (tile, split-K, variant) schedule chosen for its shape; the fp32 split-K workspace comes from
        the arena and is released right after (stream order makes the reuse safe)."""
        batch, taps, epi = kw.get("batch", 1), kw.get("taps", 1), kw.get("epi", 0)
        tile, S, variant = ops.igemm_schedule(kw["M"], kw["Nout"], taps * kw["CinP"], batch, epi, taps)
        if variant in (6, 7) and kw["CinP"] % 128:
            variant = 1            # BK = 128 rings need K slices of 128
        if tile == 1 and variant in (7, 8, 9):
            variant = 5            # deep rings exist for the 64x64 tile only (LDS)
        if epi == 1:
            S = 1                  # GEGLU pairs value and gate in one block's registers: no split-K
        if not self.sk_cnt.numel():
            S = 1                  # a network without a counter block never splits K
        ws = None
        if ops.splitk_fused(S):
            n_ws, n_cnt = ops.splitk_sizes(kw["M"], kw["Nout"], S, batch, tile)
            ws = self.arena.alloc(n_ws, torch.float32)
            kw.update(self._counters(n_cnt))
        elif S > 1:
            ws = self.arena.alloc(batch * S * kw["M"] * round_up(kw["Nout"], 4), torch.float32)
        # XCD tile order: weight-tile major when the weight matrix outweighs the activations (L2 fills, see igemm.hip)
        wbytes = kw["Nout"] * taps * kw["CinP"]
        xbytes = kw["M"] * (kw["C1"] + kw.get("C2", 0))
        op = self.add(ops.igemm(x1, wt, out, splitk=S, tile=tile, ws=ws, variant=variant, order=int(self.xcd_order and wbytes > xbytes), **kw))
        self.arena.release(ws)
        return op

    def cconv(self, x1, w, out, *, sched, **kw):
        """ops.cconv with the split-K slabs of its schedule from the arena (released right after) and its arrival counters"""
        ws = None
        if sched[3] > 1:
            n_ws, n_cnt = ops.cconv_sizes(kw["B"], kw["H"], kw["W"], kw["Nout"], sched[0], sched[3])
            ws = self.arena.alloc(n_ws, torch.float32)
            kw.update(ws=ws, **self._counters(n_cnt))
        op = self.add(ops.cconv(x1, w, out, sched=sched, **kw))
        self.arena.release(ws)
        return op

    def wsgemm(self, x1, w, out, *, sched, **kw):
        """ops.wsgemm, likewise"""
        NW, NT, _, S, _ = sched
        ws = None
        if S > 1:
            n_ws, n_cnt = ops.wsgemm_sizes(kw["M"], kw["Nout"], NW, NT, S)
            ws = self.arena.alloc(n_ws, torch.float32)
            kw.update(ws=ws, **self._counters(n_cnt))
        op = self.add(ops.wsgemm(x1, w, out, sched=sched, **kw))
        self.arena.release(ws)
        return op

    # ------------------------------------------------------------------ GroupNorm
    def gn_acc_for(self, producers, *, T: int, cpg: int) -> Optional[int]:
        """Ask the ops that wrote a GroupNorm's input(s) -- `producers` = [(op or None, channel offset of its tensor in the
        normalised channel axis)], two for a concat -- to accumulate its statistics in their epilogues (fixed-point integer atomics:
        no gn_stats launch, no second pass over the tensor).  All of them or none: returns the accumulator pointer, or None with
        nothing attached (a tile straddles samples, both target slots of a producer taken, direct epilogue forced, ...)."""
        if self.gn_layers >= self.gn_acc.shape[0] or any(op is None for op, _ in producers):
            return None
        kws = [dict(T=T, G=self.G, cpg=cpg, choff=off) for _, off in producers]
        if not all(ops.gn_target_ok(op, **k) for (op, _), k in zip(producers, kws)):
            return None
        acc_ptr = self.gn_acc.data_ptr() + self.gn_layers * self.B * self.G * 2 * 8
        for (op, _), k in zip(producers, kws):
            assert ops.gn_target(op, acc_ptr, **k)
        self.gn_layers += 1
        return acc_ptr

    def groupnorm(self, x, gamma, beta, out, *, T, C1, eps, act, acc_ptr=None, x2=None, C2=0, res=None):
        """GroupNorm (+ activation `act`, + `res`) of x | x2.  `acc_ptr` (gn_acc_for): the statistics are there, one apply launch."""
        G = self.G
        kw = dict(B=self.B, T=T, C1=C1, ld1=C1, G=G, x2=x2, C2=C2, ld2=C2)
        if acc_ptr is not None or ops.gn_self_ok(T, C1 + C2, G):
            # without producer statistics, a small tensor (tokens per sample are no whole number of the producers' tiles: any
            # resolution with 12 x 12, 6 x 6, 10 x 10 ... pixel levels) takes statistics + apply in ONE launch, the tensor read once
            self.gn_self_launches += acc_ptr is None
            self.add(ops.gn_apply(x, None, gamma, beta, out, eps=eps, silu=act, nchunk=0, acc_ptr=acc_ptr, res=res, **kw))
            return
        nchunk = max(1, min(64, T // 16))
        partial = self.arena.alloc(self.B * nchunk * G * 2, torch.float32)
        self.gn_stats_launches += 1
        self.add(ops.gn_stats(x, partial, nchunk=nchunk, **kw))
        self.add(ops.gn_apply(x, partial, gamma, beta, out, eps=eps, silu=act, nchunk=nchunk, res=res, **kw))
        self.arena.release(partial)

    # ------------------------------------------------------------------ done
    def finish(self):
        if self._zero_op is not None:
            self._zero_op.l[0] = max(16, self.gn_layers * self.B * self.G * 2 * 8)          # only the blocks in use
        assert self.sk_used <= self.sk_cnt.numel()
        self.arena_bytes = self.arena.nbytes()
        self.n_ops = len(self.pl)
        return self

    def summary(self) -> dict:
        return dict(n_ops=len(self.pl), arena_bytes=self.arena_bytes, gn_fused=self.gn_layers, gn_self_launches=self.gn_self_launches,
                    gn_stats_launches=self.gn_stats_launches, kinds=dict(self.kinds))
