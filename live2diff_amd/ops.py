"""Builders for `l2d_op` records (include/l2d.h) from torch device tensors, plus the one-time weight
packers.  Everything here is plumbing: pointers, sizes and strides; the arithmetic is in csrc/*.hip.

Each builder returns `(op, keepalive_tensors)` so that a plan (`_lib.OpList`) can keep the buffers alive.
"""
import functools
import json
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import L2dOp


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


DRY_RUN = False   # set by the CPU test-suite together with l2d_set_dry_run(1): plans are built and validated, never launched


class Overrides(NamedTuple):
    igemm_force: str
    igemm_no_table: bool
    wsgemm: bool
    wsgemm_force: str
    wsgemm_large_all: bool
    wsgemm_max_m: int
    wsgemm_no_table: bool


def overrides() -> Overrides:
    """The tuning / diagnosis overrides: the only environment variables that change which kernel or schedule a plan takes (defaults
    are the measured best).  Read on every call -- the tools set them mid-process or drive bench.py from the shell.
      L2D_IGEMM_FORCE="tile,S,variant"  every implicit-GEMM launch it fits takes that schedule (tools/igemm_tune_each.py, igemm_pick.py)
      L2D_IGEMM_NO_TABLE=1              ignore igemm_tuned.json: every shape on the fallback rule (tools/tune_igemm.sh)
      L2D_WSGEMM=0                      no weight-streaming GEMM: every level packs and runs the round-3 kernels (the tuners' baseline)
      L2D_WSGEMM_FORCE="NW,NT,NL,S"     every wsgemm launch it fits takes that schedule (tools/wsgemm_tune*.py)
      L2D_WSGEMM_LARGE_ALL=1            every layer of the levels below L2D_WSGEMM_MAX_M is offered the weight-streaming packing (what
                                        the tuners measure); without it the `skip` / `large` lists and the fallback rule decide
      L2D_WSGEMM_MAX_M=4608             most stream tokens (N x pixels) of a level that may take the weight-streaming packing
      L2D_WSGEMM_NO_TABLE=1             ignore wsgemm_tuned.json: cost-model schedules, the fallback rule packs (tools/flip_diag.py)"""
    e = os.environ
    return Overrides(igemm_force=e.get("L2D_IGEMM_FORCE", ""), igemm_no_table=bool(e.get("L2D_IGEMM_NO_TABLE")),
                     wsgemm=e.get("L2D_WSGEMM", "1") != "0", wsgemm_force=e.get("L2D_WSGEMM_FORCE", ""),
                     wsgemm_large_all=bool(e.get("L2D_WSGEMM_LARGE_ALL")), wsgemm_max_m=int(e.get("L2D_WSGEMM_MAX_M", "4608")),
                     wsgemm_no_table=bool(e.get("L2D_WSGEMM_NO_TABLE")))


@functools.lru_cache(maxsize=None)
def _table_file(name: str) -> dict:
    path = os.path.join(os.path.dirname(__file__), name)
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        return json.load(f)


def tuned_table(name: str, no_table: bool = False) -> dict:
    """A table measured on MI355X (`name`: igemm_ / rowgemm_ / wsgemm_tuned.json beside this module, written by the tuners) as
    {"shapes": {...}, ...}; empty when the file is missing or an override's NO_TABLE asks for none."""
    return {} if no_table else _table_file(name)


def _h(t: torch.Tensor) -> torch.Tensor:
    assert t.dtype == torch.float16 and (t.is_cuda or DRY_RUN), (t.dtype, t.device)
    return t


# ----------------------------------------------------------------------------- weight packing (one-time)
def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def pack_conv3x3(w: torch.Tensor) -> torch.Tensor:
    """[Cout,Cin,3,3] -> [Cout, 9*CinP] fp16 with k = tap*CinP + ci, CinP = round_up(Cin, 64) (zero padded)."""
    cout, cin, kh, kw = w.shape
    assert kh == 3 and kw == 3
    cinp = round_up(cin, 64)
    out = torch.zeros(cout, 9, cinp, dtype=torch.float16, device=w.device)
    out[:, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, 9, cin).to(torch.float16)
    return out.reshape(cout, 9 * cinp).contiguous()


def pack_linear(w: torch.Tensor) -> torch.Tensor:
    """[Nout,K] (or [Nout,K,1,1]) -> [Nout, round_up(K,64)] fp16, zero padded."""
    w = w.reshape(w.shape[0], -1)
    n, k = w.shape
    kp = round_up(k, 64)
    out = torch.zeros(n, kp, dtype=torch.float16, device=w.device)
    out[:, :k] = w.to(torch.float16)
    return out.contiguous()


def geglu_perm(c4: int, device) -> torch.Tensor:
    """Row permutation for the GEGLU projection [8C, C]: packed rows are 16 value rows then the 16 matching
    gate rows, so that value and gate of one output column meet in the same MFMA lane (igemm.hip epilogue)."""
    assert c4 % 16 == 0
    blk = torch.arange(c4 // 16, device=device)[:, None] * 16 + torch.arange(16, device=device)[None]
    return torch.stack([blk, blk + c4], dim=1).reshape(-1)


def pack_geglu(w: torch.Tensor, b: torch.Tensor):
    perm = geglu_perm(w.shape[0] // 2, w.device)
    return pack_linear(w[perm]), b[perm].float().contiguous()


def f32(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.float().contiguous()


ROWGEMM_MAX_K = 2048
# widest contraction the plan gives the row GEMM for a Linear with no norm to fuse: at K = 1280 every 32-token block streams 80 KB of
# weights per 32-row tile and igemm is faster (profiles/round3_c_bench_plain640/2048.json); GEGLU projections (LayerNorm fused) up to
# K = 1280 (routing levels 1 / 2 back to LayerNorm + igemm measured 0.6 % slower)
ROWGEMM_PLAIN_MAX_K = 640
ROWGEMM_FF1_MAX_K = 1280


def rowgemm_ok(nout: int, k: int) -> bool:
    """Shapes the token-row GEMM (csrc/rowgemm.hip) takes: whole K resident in LDS, 32-row weight tiles."""
    return k % 64 == 0 and 64 <= k <= ROWGEMM_MAX_K and nout % 32 == 0 and nout >= 32


def rowgemm_geglu_perm(c4: int, device) -> torch.Tensor:
    """Row order of a GEGLU projection [8C -> value | gate] for the 32x32 MFMA tile of rowgemm.hip: a 32-row tile holds 8
    value rows, the 8 matching gate rows, the next 8 value rows and their gate rows, so that value and gate of one output
    channel are the register groups (0, 1) / (2, 3) of the same lane."""
    assert c4 % 16 == 0
    t = torch.arange(c4 // 16, device=device)[:, None, None] * 16            # tile -> first output channel
    h = torch.arange(2, device=device)[None, :, None] * 8                    # half of the tile
    e = torch.arange(8, device=device)[None, None, :]
    val = (t + h + e)                                                        # [tiles, 2, 8]
    return torch.stack([val, val + c4], dim=2).reshape(-1)                   # [tiles, 2, (value, gate), 8]


def pack_rowgemm(w: torch.Tensor, bias: Optional[torch.Tensor] = None, gamma: Optional[torch.Tensor] = None,
                 beta: Optional[torch.Tensor] = None, geglu: bool = False):
    """[Nout, K] (or [Nout, K, 1, 1]) -> (weights in MFMA-fragment order, fp32 bias or None) for rowgemm.hip.

    Fragment order: flat index (((t * S + s) * 64 + lane) * 8 + e) holds W[32 t + lane % 32][16 s + 8 (lane // 32) + e],
    S = K / 16: the A operand of v_mfma_f32_32x32x16_f16 for weight tile t and k step s is one contiguous 1 KB block.
    With `gamma` / `beta` (the affine parameters of the LayerNorm / GroupNorm in front of this layer) the affine map is
    folded into the layer: W' = W diag(gamma), b' = b + W beta (computed in fp32 from the fp16 parameters), so the kernel's
    prologue only normalises.  `geglu`: rows re-ordered by rowgemm_geglu_perm (bias likewise)."""
    w = w.reshape(w.shape[0], -1).float()
    n, k = w.shape
    assert rowgemm_ok(n, k), (n, k)
    b = None if bias is None else bias.float().clone()
    if gamma is not None:
        if beta is not None:
            shift = w @ beta.float()
            b = shift if b is None else b + shift
        w = w * gamma.float()[None, :]
    if geglu:
        perm = rowgemm_geglu_perm(n // 2, w.device)
        w = w[perm]
        b = None if b is None else b[perm]
    S = k // 16
    packed = w.to(torch.float16).view(n // 32, 32, S, 2, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1)
    return packed, (None if b is None else b.contiguous())


def unpack_rowgemm(packed: torch.Tensor, nout: int, k: int) -> torch.Tensor:
    """inverse of the fragment permutation (tests)"""
    S = k // 16
    return packed.view(nout // 32, S, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(nout, k)


# ----------------------------------------------------------------------------- op builders
_ZERO_PAGES = {}


def zero_page(device) -> torch.Tensor:
    """64 KB of zeros per device: the DMA source for conv padding / ragged rows / channel tails (igemm.hip reads 16 bytes of it;
    wsgemm.hip walks up to 2 CinP + 128 bytes of it with the same per-stage stride as real rows)."""
    key = str(device)
    if key not in _ZERO_PAGES:
        _ZERO_PAGES[key] = torch.zeros(32768, dtype=torch.float16, device=device)
    return _ZERO_PAGES[key]


# ---- GroupNorm statistics from a producer's epilogue.  Each GEMM / conv kernel can accumulate sum / sum of squares of its output for
# up to two consumer GroupNorms (include/l2d.h: p[9], p[10] = the accumulators, i[24] / i[25] = T / G shared by both slots,
# i[26 + 2 slot] / i[27 + 2 slot] = channels per group / channel offset of this tensor in the consumer's channel axis).  Per kernel
# only the eligibility differs:
def _igemm_gn_ok(op, T, cpg, choff) -> bool:
    splitk, tile = max(1, op.i[21]), op.i[22] & 15
    fused = bool(op.p[11])
    tm = 64 if ((splitk > 1 and not fused) or tile == 2) else 128
    Nout, ldo, ldr, epi, batch = op.i[14], op.i[15], op.i[16], op.i[19], max(1, op.i[20])
    direct = (op.i[22] >> 5) & 1
    vec_ok = ((not direct) and Nout % 8 == 0 and ldo % 8 == 0 and not (op.p[5] and ldr % 8) and epi != 1
              and (op.p[6] or 0) % 16 == 0 and (op.p[5] or 0) % 16 == 0)     # 16-byte aligned out / residual (sub-views)
    return not (T % tm or batch != 1 or ((splitk == 1 or fused) and not vec_ok) or op.i[13] % T)


def _rowgemm_gn_ok(op, T, cpg, choff) -> bool:
    """(its epilogue accumulates like igemm's LDS-staged one)"""
    MT, ntr, epi = op.i[14], op.i[15], op.i[6]
    return not (T % (32 * MT) or op.i[0] % T or ntr or epi == 1 or (cpg | choff) & 1)


def _patch_gn_ok(op, T, cpg, choff) -> bool:
    """pconv and cconv: a patch never straddles samples"""
    return T == op.i[7] * op.i[8] and not (cpg | choff) & 1


def _rowchain_gn_ok(op, T, cpg, choff) -> bool:
    """(its row phase accumulates like the row GEMM's; a block is 32 tokens of one sample; head segments feed attention, never a
    GroupNorm)"""
    return not (op.i[6] != 0 or T % 32 or op.i[0] % T or (cpg | choff) & 1)


def _wsgemm_gn_ok(op, T, cpg, choff) -> bool:
    """(a 128-token tile may span samples: T % 32)"""
    NW, NT, ntr, epi, M = op.i[9], op.i[10], op.i[21], op.i[19], op.i[13]
    bno = NW * NT * 32
    return not (T % 32 or M % T or ntr or epi == 1 or (cpg | choff) & 1 or 64 * NW < bno // 2)


_GN_PRODUCER_OK = {_lib.OP_IGEMM: _igemm_gn_ok, _lib.OP_ROWGEMM: _rowgemm_gn_ok, _lib.OP_PCONV: _patch_gn_ok, _lib.OP_CCONV: _patch_gn_ok,
                   _lib.OP_ROWCHAIN: _rowchain_gn_ok, _lib.OP_WSGEMM: _wsgemm_gn_ok}


def gn_target_ok(op, *, T: int, G: int, cpg: int, choff: int) -> bool:
    """Would `gn_target` succeed?  Changes nothing: the launch can accumulate these statistics, a slot is free, and an occupied
    slot 0 has the same (T, G)."""
    ok = _GN_PRODUCER_OK.get(op.kind)
    if ok is None or G > 32 or not ok(op, T, cpg, choff):
        return False
    return not op.p[9] or ((op.i[24], op.i[25]) == (T, G) and not op.p[10])


def gn_target(op, acc_ptr: int, *, T: int, G: int, cpg: int, choff: int) -> bool:
    """Ask the GEMM / conv op that produced a tensor to accumulate that tensor's GroupNorm statistics for one consumer GroupNorm
    (up to two per op): `acc_ptr` -> int64 [samples][G][2], cpg / choff = channels per group and channel offset of this tensor in
    the consumer's (concatenated) channel axis.  Returns False when both slots are taken or the launch cannot do it."""
    if not gn_target_ok(op, T=T, G=G, cpg=cpg, choff=choff):
        return False
    slot = 1 if op.p[9] else 0
    op.p[9 + slot] = int(acc_ptr)
    op.i[24], op.i[25] = int(T), int(G)
    op.i[26 + 2 * slot], op.i[27 + 2 * slot] = int(cpg), int(choff)
    return True


def igemm_gn_target(op, acc_ptr: int, *, T: int, G: int, cpg: int, choff: int) -> bool:
    assert op.kind == _lib.OP_IGEMM
    return gn_target(op, acc_ptr, T=T, G=G, cpg=cpg, choff=choff)


def rowchain_head(x, hout, out, *, M, C, wA, bA, wB, bB=None, passes=1, resA=None, gn_acc_ptr=None, T=0, G=0, eps_gn=1e-6, eps_ln=1e-5,
                  out_t=None, ldt=0, st=0, ldx=None, ldrA=None, ldh=None, ldo=None):
    """Head segment of a transformer block (csrc/rowchain.hip, two dependent layers in one launch):
    h = A(norm?(x)) + bA (+ resA) -> hout;  out = B(LayerNorm(h)) + bB, `passes` x C packed rows; with `out_t` the LAST pass is stored
    transposed (V^T[sample][channel][ldt]) and `out` receives the first passes - 1.  gn_acc_ptr: GroupNorm prologue on x (statistics
    [samples][G][2] from x's producers, T tokens per sample).  Weights: pack_rowgemm forms (norm affine folded)."""
    op = L2dOp()
    op.kind = _lib.OP_ROWCHAIN
    assert wA.dtype == torch.float16 and wA.numel() == C * C and wB.dtype == torch.float16 and wB.numel() == passes * C * C
    assert bA.dtype == torch.float32 and bA.numel() == C and (bB is None or (bB.dtype == torch.float32 and bB.numel() == passes * C))
    trl = out_t is not None
    ncol = (passes - (1 if trl else 0)) * C
    op.p[0], op.p[1], op.p[2] = _ptr(_h(x)), (_ptr(_h(resA)) if resA is not None else None), _ptr(_h(hout))
    op.p[3] = _ptr(_h(out)) if out is not None else None
    op.p[4], op.p[5], op.p[6], op.p[7] = _ptr(_h(wA)), _ptr(bA), _ptr(_h(wB)), _ptr(bB)
    op.p[8] = _ptr(_h(out_t)) if trl else None
    op.p[14] = int(gn_acc_ptr) if gn_acc_ptr is not None else None
    op.i[0], op.i[1] = int(M), int(C)
    op.i[2], op.i[3], op.i[4], op.i[5] = int(ldx or C), int(ldrA or C), int(ldh or C), int(ldo or max(ncol, C))
    op.i[6], op.i[7], op.i[8], op.i[9], op.i[10], op.i[11] = 1, int(passes), int(trl), int(ldt), int(T), int(G)
    op.l[0] = int(st)
    op.f[0], op.f[1] = float(eps_ln), float(eps_gn)
    return op, (x, resA, hout, out, out_t, wA, bA, wB, bB)


ROWCHAIN_C = 320                # the width the chain kernel is instantiated for (SD-1.5 level 0)
# M / 32 blocks.  Round 5 set 192 from the BASELINE configs (256+ blocks, or cfg-1's 32); round 6 measured the gap: 144 blocks (384 x 384,
# N = 2) 7.70 -> 7.40 ms, 154 blocks (448 x 704, N = 1) 8.34 -> 7.98 ms, 100 blocks (320 x 320, N = 2) 7.09 -> 7.00 ms with the chain
# (profiles/round6_v_*, round6_w_*); cfg-1 (32 blocks) keeps the separate launches: 5.14 ms against 5.31 with the chain (round6_ab_*)
ROWCHAIN_MIN_BLOCKS = 96


def rowchain_ok(M: int, C: int, T: int) -> bool:
    """Shapes the token-resident block tail (csrc/rowchain.hip) takes"""
    return C == ROWCHAIN_C and M % 32 == 0 and T % 32 == 0 and M // 32 >= ROWCHAIN_MIN_BLOCKS


def rowchain(a, res1, res2, out, *, M, C, w_out, b_out, w_ff1, b_ff1, w_ff2, b_ff2, w_po, b_po, eps=1e-5, lda=None, ldr1=None,
             ldr2=None, ldo=None):
    """Token-resident tail of a transformer block (csrc/rowchain.hip): out = proj_out(FF2(GEGLU(LN(h2))) + h2) + res2 with
    h2 = to_out(a) + res1.  Weights / biases: pack_rowgemm forms (to_out plain; FF1 with the LayerNorm folded and geglu=True; FF2;
    proj_out)."""
    op = L2dOp()
    op.kind = _lib.OP_ROWCHAIN
    for t_, n_ in ((w_out, C * C), (w_ff1, 8 * C * C), (w_ff2, 4 * C * C), (w_po, C * C)):
        assert t_.dtype == torch.float16 and t_.numel() == n_, (t_.shape, n_)
    for t_, n_ in ((b_out, C), (b_ff1, 8 * C), (b_ff2, C), (b_po, C)):
        assert t_.dtype == torch.float32 and t_.numel() == n_, (t_.shape, n_)
    op.p[0], op.p[1], op.p[2], op.p[3] = _ptr(_h(a)), _ptr(_h(res1)), _ptr(_h(res2)), _ptr(_h(out))
    op.p[4], op.p[5], op.p[6], op.p[7] = _ptr(_h(w_out)), _ptr(b_out), _ptr(_h(w_ff1)), _ptr(b_ff1)
    op.p[8], op.p[11], op.p[12], op.p[13] = _ptr(_h(w_ff2)), _ptr(b_ff2), _ptr(_h(w_po)), _ptr(b_po)
    op.i[0], op.i[1] = int(M), int(C)
    op.i[2], op.i[3], op.i[4], op.i[5] = int(lda or C), int(ldr1 or C), int(ldr2 or C), int(ldo or C)
    op.f[0] = float(eps)
    return op, (a, res1, res2, out, w_out, b_out, w_ff1, b_ff1, w_ff2, b_ff2, w_po, b_po)


def pconv_patch(B: int, H: int, W: int, Nout: int, C1: int, C2: int = 0):
    """Patch (PH, PW) for the patch-resident 3x3 conv, or None when the implicit-GEMM kernel should take the launch: the largest
    of 8x16 / 8x8 / 4x8 that tiles the image and yields >= 256 blocks of (patch, 64 output channels).  Not for the lowest
    resolutions: with few tokens the launch is bound by its weight stream (9 C Nout x 2 bytes), which wants split-K."""
    if Nout % 64 or C1 % 64 or C2 % 64 or C1 <= 0:
        return None
    for ph, pw in ((8, 16), (8, 8), (4, 8)):
        if H % ph or W % pw:
            continue
        blocks = B * (H // ph) * (W // pw) * (Nout // 64)
        tokens = B * H * W
        if blocks >= 256 and tokens >= 2048:
            return ph, pw
    return None


def pconv(x1, w, out, *, B, H, W, C1, ldx1, CinP, Nout, ldo, patch, x2=None, C2=0, ldx2=0, bias=None, rowbias=None, ldrb=0,
          rows_per_bias=0, res=None, ldr=0, order=None, epi=0):
    """3x3 stride-1 conv, activation patch resident in LDS (csrc/pconv.hip); `w` = pack_conv3x3 weights (as igemm).
    epi as igemm: 0 none, 2 SiLU, 3 ReLU, 5 GELU, 4 ReLU after the residual add."""
    op = L2dOp()
    op.kind = _lib.OP_PCONV
    zp = zero_page(x1.device)
    op.p[0], op.p[1], op.p[2] = _ptr(_h(x1)), (_ptr(x2) if x2 is not None else None), _ptr(_h(w))
    op.p[3], op.p[4], op.p[5] = _ptr(bias), _ptr(rowbias), (_ptr(_h(res)) if res is not None else None)
    op.p[6], op.p[7] = _ptr(_h(out)), _ptr(zp)
    assert CinP == C1 + C2 and w.shape[1] == 9 * CinP and w.shape[0] == Nout
    if order is None:
        order = int(Nout * 9 * CinP > B * H * W * (C1 + C2))
    vals = {1: C1, 2: C2, 3: ldx1, 4: ldx2, 5: CinP, 6: B, 7: H, 8: W, 9: patch[0], 10: patch[1], 11: order, 14: Nout, 15: ldo,
            16: ldr, 17: ldrb, 18: rows_per_bias, 19: epi}
    for j, v in vals.items():
        op.i[j] = int(v)
    return op, (x1, x2, w, bias, rowbias, res, out, zp)



def _rowgemm_lds(K, NW, NT, MT, epi, pro, ntr, gn):
    BM, BNp = 32 * MT, NW * NT * 32
    BNo = BNp // 2 if epi == 1 else BNp
    xs = BM * K * 2 + BM * 16 + ((2 * K + 64) * 4 if pro == 2 else 0)
    os_ = BM * (BNo + 8) * 2 + (64 * NW * 32 + BNo * 4 if gn else 0)
    if ntr:
        os_ = max(os_, BNp * (BM + 8) * 2)
    return max(xs, os_)


def _rowgemm_mt_ok(mt, nt, K, T):
    """token tiles per block: 1, 2 (NT <= 2) or 4 (NT <= 2, K = 320: 80 KB of LDS); with T given (a norm prologue from group
    statistics, a transposed output or output statistics) a sample must be a whole number of token tiles"""
    if mt == 1:
        return True
    if mt not in (2, 4) or nt > 2 or (mt == 4 and K != 320):
        return False
    return T % (32 * mt) == 0


def rowgemm_schedule(M: int, K: int, Nout: int, ntr: int = 0, epi: int = 0, pro: int = 0, gn: bool = True, T: int = 0):
    """(NW, NT, MT) = waves per block, 32-row weight tiles per wave, 32-token tiles per block for a rowgemm launch.  A table
    measured on MI355X (rowgemm_tuned.json, tools/rowgemm_sweep.py) when it holds the shape, else a small cost model:
    per block one activation-tile load (dependent groups of 5 x 16 B per thread), then per wave NT * K * 64 bytes of weights
    through a ring of ~16 KB (latency bound: ~20 GB/s per wave) or NT * MT * K / 16 MFMAs of 32 cycles, whichever is longer;
    blocks run in rounds of 256 CUs x (blocks per CU by LDS and by 12 waves)."""
    tiles = Nout // 32
    tuned = tuned_table("rowgemm_tuned.json").get("shapes", {}).get(f"{M},{K},{Nout},{ntr},{epi}")
    if tuned and _rowgemm_mt_ok(tuned[2], tuned[1], K, T):
        return tuple(tuned)
    cdiv = lambda a, b: (a + b - 1) // b
    best, best_t = None, None
    for mt in (1, 2):
        if mt == 2 and (M < 4096 or T % 64):        # (a sample must be a whole number of token tiles for prologue 2 / V^T / statistics)
            continue
        for nt in (1, 2, 3, 4):
            if mt == 2 and nt > 2:
                continue
            for nw in range(1, (5 if nt >= 3 else 8) + 1):
                if tiles % (nw * nt) or (ntr // 32) % (nw * nt):
                    continue
                lds = _rowgemm_lds(K, nw, nt, mt, epi, pro, ntr, gn)
                if lds > 163840:
                    continue
                bm = 32 * mt
                blocks = cdiv(M, bm) * (tiles // (nw * nt))
                bpc = max(1, min(163840 // lds, 12 // nw))
                rounds = cdiv(blocks, 256 * bpc)
                lpr = 16 if (64 * nw >= 16 * bm and K % 128 == 0) else 8
                row_passes = cdiv(bm, 64 * nw // lpr)
                t_x = 0.9 * row_passes * cdiv(K // (8 * lpr), 5) + (1.0 if pro == 2 else 0.0) + (0.5 if pro == 1 else 0.0)
                t_w = nt * K * 64 / 20000.0
                t_mm = nt * mt * (K / 16) * 32 * cdiv(nw * bpc, 4) / 2100.0
                t = rounds * (t_x + max(t_w, t_mm) + 0.8)
                if best_t is None or t < best_t - 1e-9 or (abs(t - best_t) <= 1e-9 and blocks < best[3]):
                    best, best_t = (nw, nt, mt, blocks), t
    assert best is not None, (M, K, Nout, ntr)
    return best[:3]


def rowgemm(x, w, out, *, M, K, Nout, ldx, ldo, bias=None, res=None, ldr=0, epi=0, pro=0, eps=1e-5, T=0, G=0, gn_acc_ptr=None,
            out_t=None, ntr=0, ldt=0, st=0, sched=None, order=None, x_off=0, out_off=0, res_off=0):
    """Token-row GEMM (csrc/rowgemm.hip): out[m][n] = epi(sum_k norm(x)[m][k] W[n][k]).  `w` / `bias` come from pack_rowgemm
    (affine of the norm folded in).  pro: 0 none, 1 LayerNorm over K, 2 GroupNorm from the fixed-point accumulators at
    `gn_acc_ptr` (T tokens per sample, G groups).  The LAST `ntr` packed rows are stored transposed into out_t
    [sample][row][ldt] (V^T).  sched = (NW, NT, MT) or None for rowgemm_schedule."""
    op = L2dOp()
    op.kind = _lib.OP_ROWGEMM
    assert w.dtype == torch.float16 and w.numel() == Nout * K, (w.shape, Nout, K)
    if sched is None:
        sched = rowgemm_schedule(M, K, Nout, ntr, epi, pro, T=T)
    NW, NT, MT = sched
    op.p[0] = _ptr(_h(x)) + 2 * x_off
    op.p[1] = _ptr(_h(w))
    op.p[2] = _ptr(bias)
    op.p[3] = (_ptr(_h(res)) + 2 * res_off) if res is not None else None
    op.p[4] = (_ptr(_h(out)) + 2 * out_off) if out is not None else None
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == Nout
    if pro == 2:
        assert gn_acc_ptr is not None
        op.p[7] = int(gn_acc_ptr)
    if ntr:
        assert out_t is not None and ntr % 32 == 0
        op.p[8] = _ptr(_h(out_t))
    if order is None:
        order = int(Nout * K > M * K)                  # weight-band major per XCD when the weights outweigh the activations
    vals = [M, K, Nout, ldx, ldo, ldr, epi, pro, 0, T, G, 0, NW, NT, MT, ntr // 32, ldt, order]
    for j, v in enumerate(vals):
        op.i[j] = int(v)
    op.l[0] = int(st)
    op.f[0] = float(eps)
    return op, (x, w, bias, res, out, out_t)


# ----------------------------------------------------------------------------- weight-streaming GEMM (csrc/wsgemm.hip)
WS_BM = 128


def pack_fragments(w2d: torch.Tensor) -> torch.Tensor:
    """[Nout, K] (Nout % 32 == 0, K % 16 == 0) -> MFMA-fragment order: flat index (((t * S + s) * 64 + lane) * 8 + e) holds
    W[32 t + lane % 32][16 s + 8 (lane // 32) + e] (the A operand of v_mfma_f32_32x32x16_f16 is one contiguous 1 KB block)."""
    n, k = w2d.shape
    assert n % 32 == 0 and k % 16 == 0, (n, k)
    return w2d.to(torch.float16).view(n // 32, 32, k // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1)


def pack_wsgemm(w: torch.Tensor, bias: Optional[torch.Tensor] = None, gamma: Optional[torch.Tensor] = None,
                beta: Optional[torch.Tensor] = None, geglu: bool = False):
    """Linear layer [Nout, K] (K % 64 == 0, any K) for wsgemm.hip -> (fragment-packed fp16 weights, fp32 bias or None, fp32 column
    sums or None).  With `gamma` / `beta` (the LayerNorm in front of the layer) the affine map is folded in (W' = W diag(gamma),
    b' = b + W beta) and `colsum[n] = sum_k fp16(W'[n][k])` is returned for the kernel's accumulator-side normalisation
    out = rstd (x W'^T - mean colsum) + b' -- the sums are taken over the ROUNDED weights, i.e. over exactly what the matrix
    cores multiply.  `geglu`: rows re-ordered by rowgemm_geglu_perm (bias and sums likewise)."""
    w = w.reshape(w.shape[0], -1).float()
    n, k = w.shape
    assert n % 32 == 0 and k % 64 == 0, (n, k)
    b = None if bias is None else bias.float().clone()
    if gamma is not None:
        if beta is not None:
            shift = w @ beta.float()
            b = shift if b is None else b + shift
        w = w * gamma.float()[None, :]
    if geglu:
        perm = rowgemm_geglu_perm(n // 2, w.device)
        w = w[perm]
        b = None if b is None else b[perm]
    w16 = w.to(torch.float16)
    cs = w16.float().sum(1).contiguous() if gamma is not None else None
    return pack_fragments(w16), (None if b is None else b.contiguous()), cs


def pack_wsgemm_conv3x3(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 3, 3] (Cout % 32 == 0) -> fragment-packed weights with k = tap * CinP + ci (CinP = round_up(Cin, 64))."""
    return pack_fragments(pack_conv3x3(w))


def wsgemm_ok(M: int, Nout: int, C1: int, C2: int = 0, T: int = 0) -> bool:
    """Shapes wsgemm.hip takes: 32-row weight tiles, 64-channel chunks per input, samples made of whole 32-token MFMA tiles."""
    return Nout % 32 == 0 and Nout >= 32 and C1 % 64 == 0 and C1 > 0 and C2 % 64 == 0 and (T <= 0 or T % 32 == 0) and M < (1 << 22)


def _ws_lds(NW, NT, epi, ntr, gn):
    BNp = NW * NT * 32
    BNo = BNp // 2 if epi == 1 else BNp
    ring = 4 * WS_BM * 64 * 2
    ep = WS_BM * (BNo + 8) * 2 + ((64 * NW * 32 + BNo * 4) if gn else 0)
    if ntr:
        ep = max(ep, BNp * (WS_BM + 8) * 2)
    return ((max(ring, ep) + 255) // 256) * 256 + 2 * WS_BM * 4 + 64 + 6 * 320 * 4


def wsgemm_schedule(M: int, Ktot: int, Nout: int, ntr: int = 0, epi: int = 0, pro: int = 0, taps: int = 1):
    """(NW, NT, NL, S, ntw) for a wsgemm launch: consumer waves per block, 32-row weight tiles per wave, loader waves, K slices,
    non-temporal weight loads.  The table measured in the frame (wsgemm_tuned.json, tools/wsgemm_tune.py) when it holds the
    shape, else a cost model: a block streams BN x Kc weights (HBM, ~25 B/clk/CU chip-wide 6.4 TB/s) and 128 x Kc activations
    (L2), runs NT * 4 * Kc / 16 MFMAs of 32 cycles per wave; blocks run in rounds over 256 CUs; each slice beyond the first adds
    a slab write + read of 128 x BN fp32 for the last arriver."""
    tiles = Nout // 32
    nm = (M + WS_BM - 1) // WS_BM
    nch = Ktot // 64
    o = overrides()
    ntw = nm == 1
    key = wsgemm_key(taps, M, Ktot, Nout, ntr, epi, pro)
    cands = []
    for nt in (1, 2):                                  # 32-row weight tiles per consumer wave (2: at most 4 consumer waves)
        for nw in range(1, 11 if nt == 1 else 5):
            if tiles % (nw * nt) or (ntr // 32) % (nw * nt):
                continue
            if _ws_lds(nw, nt, epi, ntr, True) > 163840:
                continue
            cands.append((nw, nt))
    assert cands, (M, Ktot, Nout, ntr, epi, pro)
    if o.wsgemm_force:                                 # (applied where it divides the shape)
        nw, nt, nl, S = (int(v) for v in o.wsgemm_force.split(","))
        if (nw, nt) in cands and not (ntr and S > 1):
            return nw, nt, nl, max(1, min(S, nch)), ntw
    tuned = wsgemm_table(o).get("shapes", {})
    if key in tuned:
        nw, nt, nl, S = tuned[key][:4]
        if (nw, nt) in cands:
            return nw, nt, nl, max(1, min(S, nch)), ntw
    # default (shapes the table does not hold): two loader waves; about one block per CU (240-256 blocks); one weight tile per
    # wave; the channel tile grows with the length of the contraction (a long K wants few, fat slices: the activation chunks are
    # re-read by every channel tile) -- the pattern of the in-frame picks at cfg-2 (profiles/round4_a_wsgemm_tune_in_frame_cfg2.txt)
    best, best_c = None, None
    for nw, nt in cands:
        if nt != 1:
            continue
        ny = tiles // nw
        for S in (1, 2, 3, 4, 5, 6, 8, 10, 12, 16):
            if S > 1 and (ntr or nch // S < 4):
                continue
            blocks = nm * ny * S
            import math
            c = abs(math.log(blocks / 248.0)) + 0.12 * math.log2(S) + (0.25 if blocks > 320 else 0.0)
            want_bn = 32 if nch <= 24 else (64 if nch <= 96 else 128)       # K <= 1536: 32 channels per block, K <= 6144: 64, longer: 128
            c += 0.2 * abs(math.log2(32 * nw / want_bn))
            if best_c is None or c < best_c:
                best, best_c = (nw, 1, 2, S, ntw), c
    if best is None:
        nw, nt = cands[0]
        best = (nw, nt, 2, 1, ntw)
    return best


def wsgemm_table(o: Optional[Overrides] = None) -> dict:
    """wsgemm_tuned.json: `shapes` -> schedule; `skip` = few-token shapes (M <= WS_SMALL_M) where the round-3 kernel measured faster;
    `large` = shapes with MORE tokens where the weight-streaming kernel measured faster (there the round-3 kernels are the default:
    opt-in, not opt-out)"""
    return tuned_table("wsgemm_tuned.json", (o or overrides()).wsgemm_no_table)


WS_SMALL_M = 1280


def wsgemm_key(taps: int, M: int, Ktot: int, Nout: int, ntr: int = 0, epi: int = 0, pro: int = 0) -> str:
    return f"{taps},{M},{Ktot},{Nout},{ntr},{epi},{pro}"


def wsgemm_wanted(taps: int, M: int, Ktot: int, Nout: int, ntr: int = 0, epi: int = 0, pro: int = 0) -> bool:
    """Few-token shapes (M <= 1280): True unless the in-frame tuner measured the round-3 kernel (igemm / rowgemm) faster than the best
    wsgemm schedule (`skip` list of wsgemm_tuned.json, tools/wsgemm_tune.py).  Shapes with more tokens (round 5: level 1 of the
    BASELINE configs, 2048-4608 tokens): True only where the tuner measured the weight-streaming kernel faster (`large` list) --
    an untuned resolution keeps the round-3 kernels there.  The packer follows this."""
    key = wsgemm_key(taps, M, Ktot, Nout, ntr, epi, pro)
    o = overrides()
    d = wsgemm_table(o)
    shapes, skip = d.get("shapes", {}), d.get("skip", [])
    # measured by the tuner?  few tokens: every candidate shape it saw is in `shapes` or `skip`; above 1280 tokens it records winners
    # only, so there the token count stands for "this level was offered"
    tuned = (key in shapes or key in skip) if M <= WS_SMALL_M else any(int(k.split(",")[1]) == M for k in list(shapes) + skip)
    if o.wsgemm_large_all:                     # (the tuner offers every shape and measures)
        return key not in skip
    if not tuned:
        return _wsgemm_wanted_rule(taps, M, Ktot, Nout, ntr, epi, pro)
    if M > WS_SMALL_M:
        return key in d.get("large", [])
    return key not in skip


def _wsgemm_wanted_rule(taps: int, M: int, Ktot: int, Nout: int, ntr: int, epi: int, pro: int) -> bool:
    """Token counts the in-frame tuner never saw (any resolution outside the five BASELINE configs): the pattern of its picks there
    (122 of the 150 candidate shapes of the five plans follow it; the rest are within its 3 % threshold either way).  More than 1280
    tokens (level 1): LayerNorm + q|k|v and LayerNorm + GEGLU, the long plain contractions from 3072 tokens on, the long 3x3 convs
    that cconv.hip does not take.  Fewer: everything at the 1280-wide levels; at 640 wide the LayerNorm + q|k|v / GEGLU layers from
    512 tokens on and the 640 -> 1280 shortcuts; nothing at 320 wide (cfg-1: the row GEMM wins every layer of its levels 0 / 1)."""
    K = Ktot // taps
    if M > 4608:                # (beyond every token count the kernel was measured at; the plan's own bound is L2D_WSGEMM_MAX_M)
        return False
    if M > WS_SMALL_M:
        if taps == 9:
            return Ktot >= 5760 or M >= 3072
        if pro == 1:
            return K == 640 and Nout >= 1920
        return epi == 0 and Ktot >= 960 and Nout >= 640 and M >= 3072       # (the 320-wide level was never measured on this kernel)
    if taps == 9:
        return True
    if K <= 320:
        return False
    if K <= 640:
        return (pro == 1 and Nout >= 1920 and M >= 512) or (pro == 0 and epi == 0 and Nout >= 2 * K)
    return True


def wsgemm_sizes(M: int, Nout: int, NW: int, NT: int, S: int):
    """(fp32 workspace elements, int32 counters) of a split-K wsgemm launch: one slab of 128 x BN partial sums + 256 statistics
    floats per (channel tile, row tile, slice)."""
    nm = (M + WS_BM - 1) // WS_BM
    ny = (Nout // 32) // (NW * NT)
    return nm * ny * S * (WS_BM * NW * NT * 32 + 2 * WS_BM), nm * ny


def wsgemm(x1, w, out, *, M, Nout, C1, ldx1, ldo, x2=None, C2=0, ldx2=0, bias=None, colsum=None, rowbias=None, ldrb=0,
           rows_per_bias=0, res=None, ldr=0, taps=1, B=1, H=1, W=1, epi=0, pro=0, eps=1e-5, T=0, out_t=None, ntr=0, ldt=0,
           st=0, sched=None, ws=None, cnt=None, cnt_off=0, x1_off=0, out_off=0, res_off=0):
    """Weight-streaming GEMM (csrc/wsgemm.hip): out[m][n] = epi(sum_k LN?(x)[m][k] W[n][k]) for M <~ 1k tokens; linear layers
    (taps = 1, optional two-input channel concat, LayerNorm fold pro = 1 with `colsum`, GEGLU epi = 1, trailing `ntr` packed rows
    stored transposed into out_t) and 3x3 stride-1 pad-1 convs (taps = 9, x = [B, H, W, C1 (+ C2)], per-sample `rowbias`).
    `w` / `bias` / `colsum` come from pack_wsgemm / pack_wsgemm_conv3x3.  sched = (NW, NT, NL, S, ntw) or None for
    wsgemm_schedule; S > 1 needs `ws` (wsgemm_sizes()[0] floats) and `cnt` (int32 counters, zero, wsgemm_sizes()[1] from cnt_off)."""
    op = L2dOp()
    op.kind = _lib.OP_WSGEMM
    CinP = C1 + C2
    Ktot = taps * CinP
    assert w.dtype == torch.float16 and w.numel() == Nout * Ktot, (w.shape, Nout, Ktot)
    if sched is None:
        sched = wsgemm_schedule(M, Ktot, Nout, ntr, epi, pro, taps)
    NW, NT, NL, S, ntw = sched
    zp = zero_page(x1.device)
    op.p[0] = _ptr(_h(x1)) + 2 * x1_off
    op.p[1] = _ptr(x2) if x2 is not None else None
    op.p[2] = _ptr(_h(w))
    op.p[3], op.p[4] = _ptr(bias), _ptr(rowbias)
    op.p[5] = (_ptr(_h(res)) + 2 * res_off) if res is not None else None
    op.p[6] = (_ptr(_h(out)) + 2 * out_off) if out is not None else None
    op.p[7] = _ptr(zp)
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == Nout
    if pro == 1:
        assert colsum is not None and colsum.dtype == torch.float32 and colsum.numel() == Nout
        op.p[13] = _ptr(colsum)
    if ntr:
        assert out_t is not None and ntr % 32 == 0
        op.p[8] = _ptr(_h(out_t))
    if S > 1:
        need_ws, need_cnt = wsgemm_sizes(M, Nout, NW, NT, S)
        assert ws is not None and ws.dtype == torch.float32 and ws.numel() >= need_ws, (need_ws,)
        assert cnt is not None and cnt.dtype == torch.int32 and cnt.numel() >= cnt_off + need_cnt
        op.p[11] = _ptr(cnt) + 4 * cnt_off
        op.p[12] = _ptr(ws)
    vals = {0: taps, 1: C1, 2: C2, 3: ldx1, 4: ldx2, 5: CinP, 6: B, 7: H, 8: W, 9: NW, 10: NT, 11: NL, 12: S, 13: M, 14: Nout,
            15: ldo, 16: ldr, 17: ldrb, 18: rows_per_bias, 19: epi, 20: pro, 21: ntr // 32, 22: ldt, 23: int(bool(ntw)), 30: T}
    for j, v in vals.items():
        op.i[j] = int(v)
    op.l[0] = int(st)
    op.f[0] = float(eps)
    return op, (x1, x2, w, bias, colsum, rowbias, res, out, out_t, zp, ws, cnt)


# ----------------------------------------------------------------------------- cconv (csrc/cconv.hip, round 6)
CCONV_RING = 9          # weight ring depth of the kernel in k steps: the packed tensor is padded by this many 2 KB steps


def pack_cconv(w: torch.Tensor, KG: int) -> torch.Tensor:
    """[Cout, Cin, 3, 3] (Cout % 64 == 0; Cin padded to a multiple of 64) -> the weight STREAMS of cconv.hip: for every
    (64-channel tile n64, K group kg) one contiguous sequence [chunk c][tap t][u < 4 / KG][half i < 2][64 lanes][8 halfs] holding
    W[64 n64 + 32 i + lane % 32][tap t][64 c + 16 (u KG + kg) + 8 (lane // 32) + e] -- two A operands of
    v_mfma_f32_32x32x16_f16 per k step, in exactly the order a compute wave consumes them.  Padded with CCONV_RING k steps of
    zeros (the ring of a block's last k steps requests beyond its slice)."""
    cout, cin, kh, kw = w.shape
    assert kh == 3 and kw == 3 and cout % 64 == 0 and KG in (1, 2, 4)
    cinp = round_up(cin, 64)
    wp = torch.zeros(cout, 9, cinp, dtype=torch.float16, device=w.device)
    wp[:, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, 9, cin).to(torch.float16)
    upt = 4 // KG
    # [n64][i][r32][t][c][u][kg][lh][e] -> [n64][kg][c][t][u][i][lh][r32][e]
    v = wp.view(cout // 64, 2, 32, 9, cinp // 64, upt, KG, 2, 8).permute(0, 6, 4, 3, 5, 1, 7, 2, 8).contiguous().view(-1)
    return torch.cat([v, torch.zeros(CCONV_RING * 1024, dtype=torch.float16, device=w.device)])


def unpack_cconv(packed: torch.Tensor, cout: int, cinp: int, KG: int) -> torch.Tensor:
    """inverse of pack_cconv (tests): -> [Cout, 9, CinP]"""
    upt = 4 // KG
    v = packed[:cout * 9 * cinp].view(cout // 64, KG, cinp // 64, 9, upt, 2, 2, 32, 8)
    return v.permute(0, 5, 7, 3, 2, 4, 1, 6, 8).reshape(cout, 9, cinp)


def cconv_ok(H: int, W: int, Nout: int, C1: int, C2: int = 0) -> bool:
    """Shapes cconv.hip takes: whole 8 x 16 patches of OUTPUT pixels, 64-channel chunks per input, 64-channel output tiles."""
    return H % 8 == 0 and W % 16 == 0 and Nout % 64 == 0 and C1 % 64 == 0 and C1 > 0 and C2 % 64 == 0


def cconv_schedule(B: int, H: int, W: int, Nout: int, CinP: int, KG: Optional[int] = None):
    """(CG, KG, NLD, S) for a cconv launch: channel tile (64 CG), K groups per tile (CG KG = 4 compute waves), loader waves and
    K slices of whole 64-channel chunks, from a cost model fitted to tools/cconv_time.py / tools/cconv_stamps.py (MI355X): the k loop
    of the longest slice at ~0.7 of the matrix rate, a fixed prologue / epilogue, per split the slab publish and the last arriver's
    sum, and a second round of blocks beyond one per CU.  `KG`: the packing's K-group count when it is already fixed (the warm-up
    plan shares the stream plan's packed weights)."""
    nch = CinP // 64
    npat = B * (H // 8) * (W // 16)
    best = None
    for cg, kg, nld in ((1, 4, 4), (2, 2, 4)):
        if Nout % (64 * cg) or (KG is not None and kg != KG):
            continue
        tiles = npat * (Nout // (64 * cg))
        for S in range(1, min(nch, 8) + 1):
            blocks = tiles * S
            if blocks > 256 and S > 1:
                break
            # shader cycles (tools/cconv_stamps.py): a chunk is 3.1 k (KG = 4: 72 MFMAs per wave) / 6.2 k (KG = 2: 144) cycles, a block
            # pays ~12 k for prologue + K-group reduction + epilogue, a split adds the ticket / publish overlap and one slab read per
            # other slice; blocks beyond one per CU run as a second round
            chunks = -(-nch // S)
            loop = chunks * (3100 if kg == 4 else 6200)
            tail = ((10000 if cg == 2 else 9000) + (S - 1) * (4500 if cg == 2 else 2500)) if S > 1 else 0
            rounds = -(-blocks // 256)
            cost = rounds * (loop + 12000) + tail
            if best is None or cost < best[0]:
                best = (cost, (cg, kg, nld, S))
    assert best is not None, (B, H, W, Nout, CinP, KG)
    return best[1]


def cconv_wanted(B: int, H: int, W: int, Cin: int, Nout: int, ups: int = 0) -> bool:
    """Whether the plan gives a 3x3 stride-1 conv to cconv.hip (H x W = output resolution).  Measured at cfg-2 against the kernel
    each launch had before (tools/cconv_time.py, profiles/round6_a_cconv_time.log): the up-samplers 1.4-1.5 x (igemm), the resnet
    convs of the 640- / 1280-wide levels 1.2-1.6 x (wsgemm); the 320-wide level keeps the patch conv by default (1.02-1.14 x in isolation,
    nothing in the frame: 320 blocks of one 64-channel tile are two rounds over the chip)."""
    if not cconv_ok(H, W, Nout, Cin):
        return False
    return bool(ups) or (B * H * W >= 512 and Nout >= 640)


def cconv_sizes(B: int, H: int, W: int, Nout: int, CG: int, S: int):
    """(fp32 workspace elements, int32 counters) of a split-K cconv launch: one 128 x 64 CG slab per (tile, slice), a ticket and a
    done counter per tile"""
    tiles = B * (H // 8) * (W // 16) * (Nout // (64 * CG))
    return tiles * S * 128 * 64 * CG, 2 * tiles


def cconv(x1, w, out, *, B, H, W, C1, ldx1, Nout, ldo, KG, x2=None, C2=0, ldx2=0, ups=0, bias=None, rowbias=None, ldrb=0,
          rows_per_bias=0, res=None, ldr=0, sched=None, ws=None, cnt=None, cnt_off=0, gn_acc_ptr=None, gn_gamma=None, gn_beta=None,
          gn_G=0, gn_eps=1e-5):
    """3x3 stride-1 pad-1 conv with the activation patch resident in LDS and register-streamed weights (csrc/cconv.hip).
    H x W = OUTPUT resolution; ups = 1: the input is [B, H/2, W/2, C] and is up-sampled x2 (nearest) on the fly (Upsample3D).
    `w` = pack_cconv(weight, KG).  sched = (CG, KG, NLD, S) or None for cconv_schedule (its KG must equal the packing's);
    S > 1 needs `ws` / `cnt` (cconv_sizes).  gn_acc_ptr (+ gn_gamma / gn_beta fp16 [C1 + C2], gn_G, gn_eps): the conv of
    silu(GroupNorm(x)) -- the normalisation runs in the kernel's loader waves from the producers' fixed-point statistics
    (int64 [B][G][2], as gn_apply with nchunk = 0): no GroupNorm launch, no normalised tensor in HBM."""
    op = L2dOp()
    op.kind = _lib.OP_CCONV
    CinP = C1 + C2
    if sched is None:
        sched = cconv_schedule(B, H, W, Nout, CinP)
    CG, KG_, NLD, S = sched
    assert KG_ == KG, (sched, KG)
    assert w.dtype == torch.float16 and w.numel() == Nout * 9 * CinP + CCONV_RING * 1024, (w.shape, Nout, CinP)
    zp = zero_page(x1.device)
    op.p[0], op.p[1], op.p[2] = _ptr(_h(x1)), (_ptr(x2) if x2 is not None else None), _ptr(_h(w))
    op.p[3], op.p[4], op.p[5] = _ptr(bias), _ptr(rowbias), (_ptr(_h(res)) if res is not None else None)
    op.p[6], op.p[7] = _ptr(_h(out)), _ptr(zp)
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == Nout
    if S > 1:
        need_ws, need_cnt = cconv_sizes(B, H, W, Nout, CG, S)
        assert ws is not None and ws.dtype == torch.float32 and ws.numel() >= need_ws, (need_ws,)
        assert cnt is not None and cnt.dtype == torch.int32 and cnt.numel() >= cnt_off + need_cnt
        op.p[11] = _ptr(cnt) + 4 * cnt_off
        op.p[12] = _ptr(ws)
    vals = {1: C1, 2: C2, 3: ldx1, 4: ldx2, 5: CinP, 6: B, 7: H, 8: W, 9: CG, 10: KG, 11: NLD, 12: S, 13: ups, 14: Nout, 15: ldo,
            16: ldr, 17: ldrb, 18: rows_per_bias}
    if gn_acc_ptr is not None:
        assert gn_gamma.dtype == torch.float16 and gn_beta.dtype == torch.float16 and gn_gamma.numel() == CinP and gn_beta.numel() == CinP
        op.p[13], op.p[14], op.p[15] = int(gn_acc_ptr), _ptr(gn_gamma), _ptr(gn_beta)
        vals.update({20: 1, 21: gn_G})
        op.f[0] = float(gn_eps)
    for j, v in vals.items():
        op.i[j] = int(v)
    return op, (x1, x2, w, bias, rowbias, res, out, zp, ws, cnt, gn_gamma, gn_beta)


def igemm_schedule(M: int, Nout: int, Kp: int, batch: int = 1, epi: int = 0, taps: int = 1):
    """(tile, splitk, variant) for an implicit GEMM, from the on-GPU sweep (tools/igemm_sweep.py, profiles/r1b_igemm_sweep.txt).
    tile 1 = 128x128, 2 = 64x64; variant = pipeline shape (igemm.hip launch_p).  These kernels are occupancy /
    latency bound, not DMA-depth bound: what matters is >= ~1.5 waves of blocks over the 256 CUs.
      * >= 384 big tiles: 128x128 (3 blocks/CU with the 48 KB BK32x3 ring when there are >= 768 tiles);
      * otherwise 64x64 tiles if that yields >= 256 blocks;
      * otherwise (low-resolution levels: M = 128..2048 tokens, K up to 23 040) split K over 128x128 tiles
        (>= 8 BK64 steps per split, K >= 2048), reduced by igemm_splitk_epilogue.
    First the per-shape picks measured IN-FRAME (igemm_tuned.json, tools/igemm_pick.py over rocprofv3 traces of whole frames), then
    _igemm_heuristic_r6 for the shapes the table does not hold."""
    key = f"{taps},{M},{Nout},{Kp},{epi},{batch}"
    o = overrides()
    tuned = tuned_table("igemm_tuned.json", o.igemm_no_table).get("shapes", {})
    if o.igemm_force:                                  # (exploration runs of tools/igemm_pick.py)
        t, S, v = (int(x) for x in o.igemm_force.split(","))
        S = max(1, min(S, Kp // 128))
        ok = not (v in (6, 7) and (Kp // taps) % 128) and not (t == 1 and v in (7, 8, 9)) and 0 <= v <= 10
        if ok:
            return t, S, v
    elif key in tuned:
        return tuple(tuned[key])
    return _igemm_heuristic_r6(M, Nout, Kp, batch, epi)


def _igemm_heuristic_r6(M: int, Nout: int, Kp: int, batch: int, epi: int):
    """Fallback schedule for shapes the tuned table does not hold (every resolution outside cfg-2), round 6: the rule that the 60
    in-frame picks of igemm_tuned.json follow, instead of the round-1 sweep's.  What the table says: few-token launches want
    64 x 64 tiles with K split until ~240 blocks exist (~480 for K >= 2560) but never below ~6 BK64 steps per split nor above 6
    splits unless a split would still be longer than ~30 steps; 128 x 128 tiles + split-K only for the long 3x3 contractions
    (K >= 8640) at >= 512 tokens; no split for GEGLU epilogues.  (A/B against the round-1 rule: profiles/round6_u_*.)"""
    cdiv = lambda a, b: (a + b - 1) // b
    nk64 = Kp // 64
    t64 = cdiv(Nout, 64) * cdiv(M, 64) * batch
    t128 = cdiv(Nout, 128) * cdiv(M, 128) * batch
    if Nout <= 64 and M >= 16384:
        return 2, 1, (1 if nk64 <= 18 else 2)
    if t128 >= 384:
        return 1, 1, (4 if t128 >= 768 else 5)
    if epi == 1:
        return 2, 1, 1
    if Kp >= 8640 and M >= 512 and M * Kp >= 8_000_000:
        return 1, max(1, min(480 // t128, nk64 // 8, 16)), 5
    if t64 >= 256:
        return 2, (max(1, min(nk64 // 24, 1280 // t64)) if nk64 >= 64 else 1), 1
    target = 240 if Kp <= 1920 else 480
    return 2, max(1, min(target // t64, max(6, cdiv(nk64, 30)), nk64 // 6, 16)), 1


def igemm(x1, w, out, *, M, Nout, C1, ldx1, CinP, ldo, x2=None, C2=0, ldx2=0, bias=None, rowbias=None, ldrb=0,
          rows_per_bias=0, res=None, ldr=0, taps=1, B=1, Hin=1, Win=1, Hout=1, Wout=1, stride=1, ups=0, epi=0,
          batch=1, sx1=0, sw=0, so=0, sres=0, x1_off=0, w_off=0, out_off=0, res_off=0, splitk=1, tile=0, ws=None,
          variant=5, order=0, pad_same=False, cnt=None, cnt_off=0):
    """Offsets (in elements) allow sub-views of fp16 buffers without creating tensors.
    splitk > 1 needs `ws`: fp32 workspace of batch * splitk * M * round_up(Nout, 4) elements (two-launch reduction), or, with
    `cnt` (int32 arrival counters, zero; this launch uses splitk_sizes(...)[1] of them from cnt_off), the fused reduction's
    splitk_sizes(...)[0] elements: the last-arriving block of a tile reduces and runs the epilogue, no second launch."""
    op = L2dOp()
    op.kind = _lib.OP_IGEMM
    es = 2
    zp = zero_page(x1.device)
    op.p[0] = _ptr(_h(x1)) + x1_off * es
    op.p[1] = _ptr(x2) if x2 is not None else None
    op.p[2] = _ptr(_h(w)) + w_off * es
    op.p[3] = _ptr(bias)
    op.p[4] = _ptr(rowbias)
    op.p[5] = (_ptr(res) + res_off * es) if res is not None else None
    op.p[6] = _ptr(_h(out)) + out_off * es
    op.p[7] = _ptr(zp)
    op.p[8] = _ptr(ws)
    if bias is not None:
        assert bias.dtype == torch.float32
    if rowbias is not None:
        assert rowbias.dtype == torch.float32
    if splitk > 1 and cnt is not None:
        need_ws, need_cnt = splitk_sizes(M, Nout, splitk, batch, tile)
        assert tile in (1, 2) and ws is not None and ws.dtype == torch.float32 and ws.numel() >= need_ws
        assert cnt.dtype == torch.int32 and cnt.numel() >= cnt_off + need_cnt
        op.p[11] = _ptr(cnt) + 4 * cnt_off
    elif splitk > 1:
        assert ws is not None and ws.dtype == torch.float32 and ws.numel() >= batch * splitk * M * round_up(Nout, 4)
    vals = [taps, C1, C2, ldx1, ldx2, CinP, B, Hin, Win, Hout, Wout, stride, ups, M, Nout, ldo, ldr, ldrb,
            rows_per_bias, epi, batch, splitk, int(tile) + 16 * int(order), variant]
    for j, v in enumerate(vals):
        op.i[j] = int(v)
    op.l[0], op.l[1], op.l[2], op.l[3] = int(sx1), int(sw), int(so), int(sres)
    op.i[30] = 1 if pad_same else 0       # TF-"SAME" low-side padding 0 (stride-2 3x3 convs of the ResNetV2 backbone)
    return op, (x1, x2, w, bias, rowbias, res, out, zp, ws, cnt)


def splitk_sizes(M: int, Nout: int, splitk: int, batch: int, tile: int):
    """(fp32 workspace elements, int32 counters) of a split-K igemm with the fused reduction: whole tiles, one slab per split."""
    t = 128 if tile == 1 else 64
    ntiles = ((M + t - 1) // t) * ((Nout + t - 1) // t)
    return batch * ntiles * splitk * t * t, batch * ntiles


SPLITK_FUSED_MAX = 16            # deeper splits keep the reduction launch: ONE block
# per tile sums all S slabs in the fused form, which serialises when a launch has few tiles and many splits (8x8 levels)


def splitk_fused(splitk: int) -> bool:
    return 1 < splitk <= SPLITK_FUSED_MAX


def gn_stats(x1, partial, *, B, T, C1, ld1, G, nchunk, x2=None, C2=0, ld2=0):
    op = L2dOp()
    op.kind = _lib.OP_GN_STATS
    op.p[0], op.p[1], op.p[2] = _ptr(_h(x1)), _ptr(x2), _ptr(partial)
    for j, v in enumerate([B, T, C1, C2, ld1, ld2, G, nchunk, 0]):
        op.i[j] = int(v)
    return op, (x1, x2, partial)


ACT_NONE, ACT_SILU, ACT_RELU, ACT_ADD_RELU = 0, 1, 2, 3


def gn_self_ok(T: int, C: int, G: int) -> bool:
    """Shapes the ONE-launch GroupNorm takes (norm.hip gn_self_kernel: gn_apply with nchunk = 0 and no accumulator): a block holds all T
    pixel rows of a band of whole groups (lcm(cpg, 8) <= 128 channels, <= 4 groups) in registers, <= 16 vectors per thread."""
    if G <= 0 or C % G:
        return False
    cpg = C // G
    band = cpg
    while band % 8:
        band += cpg
    if band > 128 or band // cpg > 4 or C % band:
        return False
    pr = 256 // (band // 8)
    return -(-T // pr) <= 16


def gn_apply(x1, partial, gamma, beta, out, *, B, T, C1, ld1, G, nchunk, eps, silu, x2=None, C2=0, ld2=0, acc_ptr=None, res=None):
    """nchunk = 0 + acc_ptr: the statistics come from the fixed-point accumulators [B][G][2] int64 that the producing igemm
    launches filled (igemm `gn_target`), `partial` is unused (None).  nchunk = 0 WITHOUT acc_ptr (and partial None): the one-launch
    form for small tensors -- statistics inside the launch (gn_self_ok)."""
    op = L2dOp()
    op.kind = _lib.OP_GN_APPLY
    op.p[0], op.p[1], op.p[2] = _ptr(_h(x1)), _ptr(x2), _ptr(partial)
    if acc_ptr is not None:
        assert nchunk == 0
        op.p[6] = int(acc_ptr)
    op.p[3], op.p[4], op.p[5] = _ptr(_h(gamma)), _ptr(_h(beta)), _ptr(_h(out))
    for j, v in enumerate([B, T, C1, C2, ld1, ld2, G, nchunk, int(silu)]):     # silu: bool, or an ACT_* code
        op.i[j] = int(v)
    op.f[0] = float(eps)
    if res is not None:
        op.p[7] = _ptr(_h(res))
    return op, (x1, x2, partial, gamma, beta, out, res)


def layernorm(x, gamma, beta, out, *, rows, C, ldx, ldo, eps=1e-5):
    op = L2dOp()
    op.kind = _lib.OP_LAYERNORM
    op.p[0], op.p[1], op.p[2], op.p[3] = _ptr(_h(x)), _ptr(_h(gamma)), _ptr(_h(beta)), _ptr(_h(out))
    for j, v in enumerate([rows, C, ldx, ldo]):
        op.i[j] = int(v)
    op.f[0] = float(eps)
    return op, (x, gamma, beta, out)


def flash_attn(q, k, vt, out, *, B, H, d, Tq, Tk, ldq, ldk, ldvt, ldo, sq, sk, svt, so, q_off=0, k_off=0, vt_off=0,
               variant=0):
    """variant: 0 auto (LDS-DMA ring kernel), 1 register-staged kernel (round 1), 2 / 3 ring with 32 / 16 query rows per
    wave, 4 ring with 32 rows per wave and the software-pipelined loop (d <= 48; other head sizes run variant 2)."""
    op = L2dOp()
    op.kind = _lib.OP_FLASH_ATTN
    zp = zero_page(q.device)
    op.p[0] = _ptr(_h(q)) + q_off * 2
    op.p[1] = _ptr(_h(k)) + k_off * 2
    op.p[2] = _ptr(_h(vt)) + vt_off * 2
    op.p[3] = _ptr(_h(out))
    op.p[4] = _ptr(zp)
    for j, v in enumerate([B, H, d, Tq, Tk, ldq, ldk, ldvt, ldo, variant]):
        op.i[j] = int(v)
    op.l[0], op.l[1], op.l[2], op.l[3] = int(sq), int(sk), int(svt), int(so)
    return op, (q, k, vt, out, zp)


def tattn_stream(qkv, cache, q_pe, k_pe, v_pe, pe_idx, update_idx, bias, out, *, N, T, C, L, H, variant=0):
    assert cache.dtype == torch.float16 and cache.is_contiguous() and tuple(cache.shape) == (N, 2, T, L, C), \
        (cache.dtype, tuple(cache.shape), (N, 2, T, L, C))
    assert pe_idx.dtype == torch.int64 and update_idx.dtype == torch.int64 and bias.dtype == torch.float16
    op = L2dOp()
    op.kind = _lib.OP_TATTN_STREAM
    zp = zero_page(qkv.device)                      # DMA source of masked slots (ring kernel)
    for j, t in enumerate([qkv, cache, q_pe, k_pe, v_pe, pe_idx, update_idx, bias, out, zp]):
        op.p[j] = _ptr(t)
    for j, v in enumerate([N, T, C, L, H, variant]):
        op.i[j] = int(v)
    return op, (qkv, cache, q_pe, k_pe, v_pe, pe_idx, update_idx, bias, out, zp)


def tattn_warmup(qkv, cache_row, q_pe, k_pe, v_pe, out, *, F, T, C, L, H):
    assert cache_row.dtype == torch.float16 and cache_row.is_contiguous() and tuple(cache_row.shape) == (2, T, L, C)
    op = L2dOp()
    op.kind = _lib.OP_TATTN_WARMUP
    for j, t in enumerate([qkv, cache_row, q_pe, k_pe, v_pe]):
        op.p[j] = _ptr(t)
    op.p[8] = _ptr(out)
    for j, v in enumerate([F, T, C, L, H]):
        op.i[j] = int(v)
    return op, (qkv, cache_row, q_pe, k_pe, v_pe, out)


def skinny_linear(a, w, bias, out, *, M, K, Nout, silu_out=False, ldo=None, lda=0, a_off=0):
    op = L2dOp()
    op.kind = _lib.OP_SKINNY_LINEAR
    op.p[0], op.p[1], op.p[2], op.p[3] = _ptr(_h(a)) + 2 * a_off, _ptr(_h(w)), _ptr(bias), _ptr(out)
    op.l[0] = int(lda)
    is_f = out.dtype == torch.float32
    for j, v in enumerate([M, K, Nout, 1 if silu_out else 0, 1 if is_f else 0, ldo if ldo is not None else Nout]):
        op.i[j] = int(v)
    return op, (a, w, bias, out)


def timestep_embed(t, out, *, N, dim):
    assert t.dtype == torch.int64
    op = L2dOp()
    op.kind = _lib.OP_TIMESTEP_EMBED
    op.p[0], op.p[1] = _ptr(t), _ptr(_h(out))
    op.i[0], op.i[1] = N, dim
    return op, (t, out)


MAP_COPY, MAP_ADD_SCALE, MAP_TANH3, MAP_SCALE_ADD = 0, 1, 2, 3     # element maps of the layout kernels (include/l2d.h)


def nchw_to_nhwc(x, out, *, B, C, HW, Cpad, mode=MAP_COPY, a=1.0, b=0.0):
    op = L2dOp()
    op.kind = _lib.OP_NCHW_TO_NHWC
    op.p[0], op.p[1] = _ptr(_h(x)), _ptr(_h(out))
    for j, v in enumerate([B, C, HW, Cpad, mode]):
        op.i[j] = int(v)
    op.f[0], op.f[1] = float(a), float(b)
    return op, (x, out)


def nhwc_to_nchw(x, out, *, B, C, HW, ld, mode=MAP_COPY, a=1.0, b=0.0):
    op = L2dOp()
    op.kind = _lib.OP_NHWC_TO_NCHW
    op.p[0], op.p[1] = _ptr(_h(x)), _ptr(_h(out))
    for j, v in enumerate([B, C, HW, ld, mode]):
        op.i[j] = int(v)
    op.f[0], op.f[1] = float(a), float(b)
    return op, (x, out)


def stem7x7(img, w, out, *, B, H, W):
    """weight-standardised 7x7 stride-2 SAME conv 3 -> 64 from the NCHW image to channels-last (DPT-Hybrid stem)."""
    op = L2dOp()
    op.kind = _lib.OP_STEM7X7
    op.p[0], op.p[1], op.p[2] = _ptr(_h(img)), _ptr(_h(w)), _ptr(_h(out))
    op.i[0], op.i[1], op.i[2] = int(B), int(H), int(W)
    return op, (img, w, out)


RS_MAXPOOL, RS_SUBSAMPLE, RS_UP2X = 0, 1, 2


def resample_nhwc(x, out, *, B, H, W, C, mode):
    op = L2dOp()
    op.kind = _lib.OP_RESAMPLE_NHWC
    op.p[0], op.p[1] = _ptr(_h(x)), _ptr(_h(out))
    for j, v in enumerate([B, H, W, C, mode]):
        op.i[j] = int(v)
    return op, (x, out)


def ew(a, b, out, out_relu, *, n):
    """s = a (+ b); out = s; out_relu = relu(s) (either output may be None)."""
    op = L2dOp()
    op.kind = _lib.OP_EW
    op.p[0], op.p[1], op.p[2], op.p[3] = _ptr(_h(a)), _ptr(b), _ptr(out), _ptr(out_relu)
    op.l[0] = int(n)
    return op, (a, b, out, out_relu)


def resize_bilinear(x, out, *, planes, Hin, Win, Hout, Wout):
    """F.interpolate(x, (Hout, Wout), mode="bilinear", align_corners=False) on [planes, Hin, Win] fp16."""
    op = L2dOp()
    op.kind = _lib.OP_RESIZE_BILINEAR
    op.p[0], op.p[1] = _ptr(_h(x)), _ptr(_h(out))
    for j, v in enumerate([planes, Hin, Win, Hout, Wout]):
        op.i[j] = int(v)
    return op, (x, out)


def minmax(x, scratch, out, *, n, nb=256):
    """{min, max} of the first n halfs of x -> out float[2] on the device; scratch float[2*nb]."""
    assert scratch.dtype == torch.float32 and scratch.numel() >= 2 * nb and out.dtype == torch.float32 and out.numel() >= 2
    op = L2dOp()
    op.kind = _lib.OP_MINMAX
    op.p[0], op.p[1], op.p[2] = _ptr(_h(x)), _ptr(scratch), _ptr(out)
    op.l[0] = int(n)
    op.i[0] = int(nb)
    return op, (x, scratch, out)


def depth_norm_resize(depth, mm, out, *, B, Hd, Wd, H, W):
    """reference pipeline_stream_animation_depth.py:560-567 in one pass: depth [B,Hd,Wd] fp16 + {min,max} -> [B,3,H,W] fp16."""
    assert mm.dtype == torch.float32
    op = L2dOp()
    op.kind = _lib.OP_DEPTH_NORM_RESIZE
    op.p[0], op.p[1], op.p[2] = _ptr(_h(depth)), _ptr(mm), _ptr(_h(out))
    for j, v in enumerate([B, Hd, Wd, H, W]):
        op.i[j] = int(v)
    return op, (depth, mm, out)


def lcm_step(x, eps, scal, x0, *, N, per):
    op = L2dOp()
    op.kind = _lib.OP_LCM_STEP
    op.p[0], op.p[1], op.p[2], op.p[3] = _ptr(_h(x)), _ptr(_h(eps)), _ptr(scal), _ptr(_h(x0))
    op.i[0], op.i[1] = N, per
    return op, (x, eps, scal, x0)


def ring_update(bias, pe_idx, update_idx, *, N, L, sink, frame_ctr=None):
    """update_attn_bias on the device, in place (reference pipeline_stream_animation_depth.py:416-438)."""
    assert bias.dtype == torch.float16 and pe_idx.dtype == torch.int64 and update_idx.dtype == torch.int64
    assert frame_ctr is None or (frame_ctr.dtype == torch.int64 and frame_ctr.numel() >= 1)
    op = L2dOp()
    op.kind = _lib.OP_RING_UPDATE
    op.p[0], op.p[1], op.p[2], op.p[3] = _ptr(bias), _ptr(pe_idx), _ptr(update_idx), _ptr(frame_ctr)
    op.i[0], op.i[1], op.i[2] = N, L, sink
    return op, (bias, pe_idx, update_idx, frame_ctr)


def stream_shift(x_t, eps, scal, x0_out, *, N, per, noise=None, depth=None):
    """LCM step of the N rows + stream-batch shift register, in place on x_t / depth (reference :387-401, :590-601)."""
    assert scal.dtype == torch.float32 and scal.numel() >= 4 * N
    assert noise is None or noise.numel() >= (N - 1) * per
    op = L2dOp()
    op.kind = _lib.OP_STREAM_SHIFT
    op.p[0], op.p[1], op.p[2], op.p[3] = _ptr(_h(x_t)), _ptr(_h(eps)), _ptr(scal), _ptr(noise)
    op.p[4], op.p[5] = _ptr(_h(x0_out)), _ptr(depth)
    op.i[0], op.i[1] = N, per
    return op, (x_t, eps, scal, noise, x0_out, depth)


def randn(out, *, seed: int, offset: int = 0, frame_ctr=None):
    """Standard-normal fill (Philox4x32-10 + Box-Muller); with `frame_ctr` the stream position advances per frame."""
    op = L2dOp()
    op.kind = _lib.OP_RANDN
    op.p[0], op.p[1] = _ptr(_h(out)), _ptr(frame_ctr)
    op.l[0], op.l[1], op.l[2] = out.numel(), int(seed), int(offset)
    return op, (out, frame_ctr)


def copy(src, dst, nbytes):
    op = L2dOp()
    op.kind = _lib.OP_COPY
    op.p[0], op.p[1] = _ptr(src), _ptr(dst)
    op.l[0] = int(nbytes)
    return op, (src, dst)


# ----------------------------------------------------------------------------- re-warm: the sink commit (sink_commit.hip)
# (stands here, with the stream's own ops, and borrows `_record` and `_got` from the frame section below)
SINK_REC = np.dtype([("dst", "<u8"), ("src", "<u8"), ("lines", "<i8"), ("line_bytes", "<i8"), ("dst_pitch", "<i8"),
                     ("src_pitch", "<i8")])                                         # l2d_sink_rec


def sink_commit_table(dst, src, *, F):
    """The records of `sink_commit` for two lists of KV caches: `dst[j]` the live cache of layer j, contiguous fp16 [N,2,T,L,C];
    `src[j]` its shadow, contiguous fp16 [N,2,T,Ls,C] with F <= Ls (Ls = L: a second cache list; Ls = F: a compact one).  Slots
    0..F-1 of every (row, k|v, token) line are what the launch copies.  -> a numpy array of SINK_REC."""
    dst, src = list(dst), list(src)
    if not dst or len(dst) != len(src):
        raise ValueError(f"sink_commit: {len(dst)} destination caches and {len(src)} source caches: need one source per destination, at least one")
    rec = np.zeros(len(dst), dtype=SINK_REC)
    for j, (d, s) in enumerate(zip(dst, src)):
        for name, t in (("dst", d), ("src", s)):
            if not torch.is_tensor(t) or t.dtype != torch.float16 or t.dim() != 5 or t.shape[1] != 2 or not t.is_contiguous():
                raise ValueError(f"sink_commit: {name}[{j}]: expected a contiguous fp16 [N,2,T,L,C] cache, got {_got(t)}")
        if d.shape[:3] != s.shape[:3] or d.shape[4] != s.shape[4]:
            raise ValueError(f"sink_commit: src[{j}] {tuple(s.shape)} does not hold the lines of dst[{j}] {tuple(d.shape)}")
        if not 1 <= F <= min(d.shape[3], s.shape[3]):
            raise ValueError(f"sink_commit: F = {F} sink slots, dst[{j}] has {d.shape[3]} slots per line and src[{j}] {s.shape[3]}")
        C = d.shape[4]
        rec[j] = (d.data_ptr(), s.data_ptr(), d.shape[0] * 2 * d.shape[2], F * C * 2, d.shape[3] * C * 2, s.shape[3] * C * 2)
    return rec


def sink_commit_check(table_host) -> None:
    """everything the launcher refuses (l2d.h L2D_OP_SINK_COMMIT), as a ValueError that names the record"""
    if not isinstance(table_host, np.ndarray) or table_host.dtype != SINK_REC or table_host.ndim != 1 or not table_host.flags["C_CONTIGUOUS"]:
        raise ValueError("sink_commit: the host table must be a contiguous 1-d numpy array of SINK_REC")
    if len(table_host) == 0:
        raise ValueError("sink_commit: no records")
    for r, c in enumerate(table_host):
        dst, src, lines, nb, dp, sp = (int(c[k]) for k in SINK_REC.names)
        if not dst or not src:
            raise ValueError(f"sink_commit: record {r} has a null {'src' if dst else 'dst'}")
        if (dst | src) % 16:
            raise ValueError(f"sink_commit: record {r}: dst or src is not 16-byte aligned")
        if lines <= 0:
            raise ValueError(f"sink_commit: record {r} has {lines} lines, need at least one")
        if nb <= 0 or dp <= 0 or sp <= 0 or (nb | dp | sp) % 16:
            raise ValueError(f"sink_commit: record {r}: bytes per line {nb}, pitches {dp} / {sp}: need positive multiples of 16")
        if nb > dp or nb > sp:
            raise ValueError(f"sink_commit: record {r}: {nb} bytes per line do not fit the pitches {dp} / {sp}")
        if lines * (max(dp, sp) // 16) >= 1 << 31:
            raise ValueError(f"sink_commit: record {r}: {lines} lines of pitch {max(dp, sp)} do not fit 2^31 16-byte vectors (the kernel's index)")
        if dst < src + (lines - 1) * sp + nb and src < dst + (lines - 1) * dp + nb:
            raise ValueError(f"sink_commit: record {r}: the destination range overlaps the source range")


def sink_commit(table_dev, table_host):
    """Slots 0..F-1 of every line of every record's destination <- its source, one launch, bits as they are.  `table_dev`: the
    l2d_sink_rec records as a uint8 tensor on the device (16-byte aligned); `table_host`: the same records as a numpy array of
    SINK_REC (`sink_commit_table`; the launcher validates on it and sizes the grid from it)."""
    sink_commit_check(table_host)
    if not torch.is_tensor(table_dev) or table_dev.dtype != torch.uint8 or table_dev.numel() != table_host.nbytes \
            or not table_dev.is_contiguous() or table_dev.data_ptr() % 16:
        raise ValueError(f"sink_commit: the device table must be a contiguous, 16-byte aligned uint8 tensor of the host table's "
                         f"{table_host.nbytes} bytes, got {_got(table_dev)}")
    return _record(_lib.OP_SINK_COMMIT, (table_dev,), (len(table_host),), at={1: table_host.ctypes.data}, keep=(table_dev, table_host))


def run(op_and_keep, stream=None):
    """Run a single op immediately (unit tests)."""
    op, keep = op_and_keep
    pl = _lib.OpList()
    pl.append(op, *keep)
    pl.run(stream)


# ----------------------------------------------------------------------------- CLIP text encoder (clip.hip)
CLIP_STEPS = 12          # k steps of 16 per wave and pass of clip_linear_kernel: K % 192 == 0


def pack_clip_linear(w: torch.Tensor) -> torch.Tensor:
    """[Nout, K] -> fp16 in MFMA-fragment order for L2D_OP_CLIP_LINEAR: flat (((t * S + s) * 64 + lane) * 8 + e) holds
    W[32 t + lane % 32][16 s + 8 (lane // 32) + e], S = K / 16 (the permutation of pack_rowgemm, without its K limit)."""
    n, k = w.shape
    assert n % 32 == 0 and k % (16 * CLIP_STEPS) == 0, (n, k)
    S = k // 16
    return w.to(torch.float16).reshape(n // 32, 32, S, 2, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1)


def clip_linear_schedule(M: int, K: int):
    """(NW waves per block, MT token tiles per block): K splits into NW x npass passes of 12 k steps (NW <= 8); the token tiles
    of 32 go to as few blocks as hold them at <= 4 tiles each, spread evenly."""
    n12 = K // (16 * CLIP_STEPS)
    NW = max(d for d in range(1, 9) if n12 % d == 0)
    mtiles = (M + 31) // 32
    groups = (mtiles + 3) // 4
    return NW, (mtiles + groups - 1) // groups


def clip_embed(ids, tok, pos, out, *, rows, T, C, V, P):
    op = L2dOp()
    op.kind = _lib.OP_CLIP_EMBED
    assert ids.dtype == torch.int64 and out.dtype == torch.float32
    op.p[0], op.p[1], op.p[2], op.p[3] = _ptr(ids), _ptr(_h(tok)), _ptr(_h(pos)), _ptr(out)
    for j, v in enumerate([rows, T, C, V, P]):
        op.i[j] = int(v)
    return op, (ids, tok, pos, out)


def clip_attn(qkv, out, *, B, T, H, d, ldq, ldo, scale, causal=True, q_off=0, o_off=0):
    op = L2dOp()
    op.kind = _lib.OP_CLIP_ATTN
    op.p[0], op.p[1] = _ptr(_h(qkv)) + 2 * q_off, _ptr(_h(out)) + 2 * o_off
    for j, v in enumerate([B, T, H, d, ldq, ldo, 1 if causal else 0]):
        op.i[j] = int(v)
    op.f[0] = float(scale)
    return op, (qkv, out)


CLIP_EPI_NONE, CLIP_EPI_QUICK_GELU, CLIP_EPI_RESIDUAL = 0, 1, 2


def clip_linear(x, w, out, *, M, K, Nout, ldx, ldo, bias=None, gamma=None, beta=None, epi=CLIP_EPI_NONE, eps=1e-5,
                NW=None, MT=None):
    """x fp16 [M][ldx], or the fp32 residual stream with gamma / beta given (LayerNorm prologue); out fp16, or fp32 with
    epi = CLIP_EPI_RESIDUAL (out += x W^T + b in place)."""
    op = L2dOp()
    op.kind = _lib.OP_CLIP_LINEAR
    pro = 1 if gamma is not None else 0
    assert x.dtype == (torch.float32 if pro else torch.float16), x.dtype
    assert out.dtype == (torch.float32 if epi == CLIP_EPI_RESIDUAL else torch.float16), out.dtype
    nw, mt = clip_linear_schedule(M, K)
    op.p[0], op.p[1], op.p[2], op.p[3] = _ptr(x), _ptr(_h(w)), _ptr(bias), _ptr(out)
    op.p[4], op.p[5] = _ptr(gamma), _ptr(beta)
    for j, v in enumerate([M, K, Nout, ldx, ldo, pro, epi, NW or nw, MT or mt]):
        op.i[j] = int(v)
    op.f[0] = float(eps)
    return op, (x, w, bias, out, gamma, beta)


def clip_ln(x, gamma, beta, out, *, rows, C, ldx, ldo, eps=1e-5, x_off=0, o_off=0):
    op = L2dOp()
    op.kind = _lib.OP_CLIP_LN
    assert x.dtype == torch.float32 and gamma.dtype == torch.float32
    op.p[0], op.p[1], op.p[2], op.p[3] = _ptr(x) + 4 * x_off, _ptr(gamma), _ptr(beta), _ptr(_h(out)) + 2 * o_off
    for j, v in enumerate([rows, C, ldx, ldo]):
        op.i[j] = int(v)
    op.f[0] = float(eps)
    return op, (x, gamma, beta, out)


# ----------------------------------------------------------------------------- SD AutoencoderKL (csrc/vae_attn.hip)
VAE_ATTN_D = 512        # the one head size vae_attn.hip runs
VAE_ATTN_MAX_SPLITS = 16


def vae_attn_schedule(B: int, T: int) -> int:
    """Key splits per 64-row query tile: enough blocks for ~one round over the 256 CUs, every split at least one 32-key tile."""
    nt, nqt = -(-T // 32), -(-T // 64)
    S = max(1, min(256 // max(1, B * nqt), VAE_ATTN_MAX_SPLITS, nt))
    tps = -(-nt // S)
    return -(-nt // tps)                       # (no empty split)


def vae_attn_sizes(B: int, T: int, S: int):
    """(fp16 tile-image elements, fp32 workspace elements) of one vae_attn launch"""
    nt, nqt = -(-T // 32), -(-T // 64)
    return B * nt * 2 * 32 * VAE_ATTN_D, (S * B * nqt * 64 * (VAE_ATTN_D + 2) if S > 1 else 0)


def vae_attn(qkv, out, img, ws=None, *, B, T, ld, ldo, S=None, scale=VAE_ATTN_D ** -0.5):
    """softmax(Q K^T scale) V for one head of d = 512 per sample: qkv [B*T][ld] fp16 (q | k | v), out [B*T][ldo] fp16.
    `img` / `ws`: workspaces of vae_attn_sizes (fp16 / fp32; ws only with S > 1)."""
    op = L2dOp()
    op.kind = _lib.OP_VAE_ATTN
    S = vae_attn_schedule(B, T) if S is None else S
    n_img, n_ws = vae_attn_sizes(B, T, S)
    assert img.dtype == torch.float16 and img.numel() >= n_img, (img.numel(), n_img)
    assert S == 1 or (ws is not None and ws.dtype == torch.float32 and ws.numel() >= n_ws)
    op.p[0], op.p[1], op.p[2], op.p[3] = _ptr(_h(qkv)), _ptr(_h(out)), _ptr(_h(img)), (_ptr(ws) if S > 1 else None)
    for j, v in enumerate([B, T, ld, ldo, S]):
        op.i[j] = int(v)
    op.f[0] = float(scale)
    return op, (qkv, out, img, ws)


def vae_posterior(moments, eps, out, *, B, HW):
    """z = mean + exp(0.5 clamp(logvar, -30, 20)) eps on NCHW moments [B, 8, HW] (fp16), eps / z [B, 4, HW] fp16"""
    op = L2dOp()
    op.kind = _lib.OP_VAE_POSTERIOR
    assert moments.dtype == eps.dtype == out.dtype == torch.float16
    assert moments.numel() >= B * 8 * HW and eps.numel() >= B * 4 * HW and out.numel() >= B * 4 * HW
    op.p[0], op.p[1], op.p[2] = _ptr(moments), _ptr(eps), _ptr(out)
    op.i[0], op.i[1] = int(B), int(HW)
    return op, (moments, eps, out)


# ----------------------------------------------------------------------------- cut detection (cut.hip)
# (The section below runs to the end of the file and its builders are pinned one by one in tests/test_frame_records_cpu.py; these
# two stand in front of it and use its helpers: `_record`, `_fp16_frame`, `_int_in`, `_overlap`, `_got` and the dtype tuples.)
CUT_BLOCK, CUT_BINS, CUT_TILE, CUT_PARTIAL = 8, 64, 64, 68                                               # l2d.h L2D_CUT_*
CUT_MAX_PIXELS = 1 << 22                          # l2d.h L2D_CUT_MAX_PIXELS: H W at most
CUT_NEVER = 1 << 30                               # l2d.h L2D_CUT_NEVER: `since` before the first cut, and where it saturates
CUT_INIT = 1                                      # l2d.h L2D_CUT_INIT: the first frame, no previous state is read
CUT_MAX_GAP, CUT_MIN_R, CUT_MAX_R = 255, 256, 16384


def frame_cut_tiles(H: int, W: int) -> int:
    """the work-groups of `frame_cut_sig`: one per 64 x 64 pixels, ragged in whole 8 x 8 blocks at the right and the bottom"""
    return ((int(H) + CUT_TILE - 1) // CUT_TILE) * ((int(W) + CUT_TILE - 1) // CUT_TILE)


def _cut_size(name, H, W):
    if H < CUT_BLOCK or W < CUT_BLOCK or H % CUT_BLOCK or W % CUT_BLOCK or H * W > CUT_MAX_PIXELS:
        raise ValueError(f"{name}: {H} x {W}: H and W must be positive multiples of {CUT_BLOCK} with H W <= 2^22")


def _cut_state(name, t, dtypes, shape, what):
    """one tensor of a cut state -- the uint16 [H/8,W/8] thumbnail, the uint32 [64] histogram, the int32 [8] record, or the
    partials: contiguous, 16-byte aligned, of exactly that shape (int16 / int32: the bits of uint16 / uint32 words)"""
    if not torch.is_tensor(t) or t.dtype not in dtypes or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.data_ptr() % 16:
        raise ValueError(f"{name}: expected a contiguous, 16-byte aligned {str(dtypes[0]).replace('torch.', '')} {list(shape)} tensor "
                         f"({what}), got {_got(t)}")


def frame_cut_sig(source, prev_thumb, thumb, partials, *, H, W):
    """fp16 [3,H,W] `source` -> its uint16 [H/8,W/8] `thumb` (cut.signature_ref's) and uint32 [nwg,68] `partials`: per 64 x 64 tile
    the 64 counts of its luma histogram, its share of Dt = sum |thumb - prev_thumb|, three zeros.  `prev_thumb` None: INIT, the
    shares are zero.  Every entry of `thumb` and `partials` is written on every launch."""
    _cut_size("frame_cut_sig", H, W)
    _fp16_frame("frame_cut_sig: source", source, H, W, align=16)
    shape = (H // CUT_BLOCK, W // CUT_BLOCK)
    if prev_thumb is not None:
        _cut_state("frame_cut_sig: prev_thumb", prev_thumb, _STATE_DTYPES, shape, "the thumbnail of the frame before, or None")
    _cut_state("frame_cut_sig: thumb", thumb, _STATE_DTYPES, shape, "the thumbnail")
    nwg = frame_cut_tiles(H, W)
    _cut_state("frame_cut_sig: partials", partials, _COUNT_DTYPES, (nwg, CUT_PARTIAL), f"{nwg} tiles of {CUT_TILE} x {CUT_TILE} pixels")
    outs, reads = (thumb, partials), (source, prev_thumb)
    if any(_overlap(o, r) for o in outs for r in reads) or _overlap(thumb, partials):
        raise ValueError("frame_cut_sig: thumb or the partials overlap the source, prev_thumb or each other: the two states ping-pong")
    return _record(_lib.OP_FRAME_CUT_SIG, (source, prev_thumb, thumb, partials), (H, W, CUT_INIT if prev_thumb is None else 0, nwg))


def frame_cut(partials, prev, state, *, H, W, Tt, Th, R, gap):
    """uint32 [nwg,68] `partials` of an H x W frame and the state `prev` = (thumb, hist, rec) of the frame before -> `state`'s
    uint32 [64] histogram and int32 [8] record (cut.measure_ref).  `prev` None: INIT.  The thumbnails are `frame_cut_sig`'s and
    only checked here; `Tt`, `Th`, `R`, `gap`: `cut.cut_params`."""
    _cut_size("frame_cut", H, W)
    nwg = frame_cut_tiles(H, W)
    _cut_state("frame_cut: partials", partials, _COUNT_DTYPES, (nwg, CUT_PARTIAL), f"{nwg} tiles of {CUT_TILE} x {CUT_TILE} pixels")
    shape = (H // CUT_BLOCK, W // CUT_BLOCK)
    for name, st in (("prev", prev), ("state", state)):
        if st is None and name == "prev":
            continue
        if not isinstance(st, (tuple, list)) or len(st) != 3:
            raise ValueError(f"frame_cut: {name}: expected a (thumb, hist, rec) state, got {st!r}")
        _cut_state(f"frame_cut: {name}: thumb", st[0], _STATE_DTYPES, shape, "the thumbnail")
        _cut_state(f"frame_cut: {name}: hist", st[1], _COUNT_DTYPES, (CUT_BINS,), "the histogram")
        _cut_state(f"frame_cut: {name}: rec", st[2], (torch.int32,), (8,), "the record")
    _int_in("frame_cut: Tt", Tt, 0, 255 * H * W, strict=True)
    _int_in("frame_cut: Th", Th, 0, 2 * H * W, strict=True)
    _int_in("frame_cut: R", R, 0, CUT_MAX_R, strict=True)
    if 0 < R < CUT_MIN_R:
        raise ValueError(f"frame_cut: R={R!r}: use 0 (no level test) or an integer from {CUT_MIN_R} to {CUT_MAX_R}")
    _int_in("frame_cut: gap", gap, 0, CUT_MAX_GAP, strict=True)
    reads = (partials,) + (tuple(prev) if prev is not None else ())
    if any(_overlap(o, r) for o in state for r in reads) or any(_overlap(a, b) for j, a in enumerate(state) for b in state[j + 1:]):
        raise ValueError("frame_cut: the state written overlaps the partials, the state read or itself: the two states ping-pong")
    ph, pr = (None, None) if prev is None else (prev[1], prev[2])
    return _record(_lib.OP_FRAME_CUT, (partials, ph, pr, state[1], state[2]), (H, W, nwg, CUT_INIT if prev is None else 0, Tt, Th, R, gap),
                   keep=(partials,) + (tuple(prev) if prev is not None else ()) + tuple(state))


# ----------------------------------------------------------------------------- frame I/O (frame_io.hip)
# From here to the end of the file every builder checks its operands with the helpers below and ends in one call of `_record`:
#   p   the tensors the kernel reads or writes, in the order of l2d.h's record; None is a null pointer.  A pointer that does not
#       follow the others (the gain record in p[6]) goes in `at`
#   i   sizes, radii and flag words; the bits of an fp32 value where l2d.h says so (`_f32_bits`)
#   l   strides and other 64-bit sizes; the bits of a double where l2d.h says so (`_f64_bits`)
#   f   the ramps and strengths the kernels take as float
#   keep  every tensor whose pointer is in the record, in the record's order: the plan holds them for as long as it lives
# One check per kind of operand, named after what it checks; the first argument is "<builder>: <operand>", the head of the message:
#   _fp16_frame  [3,H,W] fp16 frame            _fp32_plane  [H,W] fp32 plane (matte values)      _int_in  an integer from lo to hi
#   _u8_planes   [3,H,W] planar uint8 record   _fp16_depth  [H,W] fp16 depth plane
#   _u8_frame    [H,W,3] uint8 frame           _i32_planes  [3,H,W] int32 planes
#   _resample_tables  the index and weight tables of depth_ingest / mask_ingest;  _axis_table  one int32 table of an output axis
# `_matte_input` is the `plane=` or `depth=` operand of the ops that cut by a matte, `_ramp_input` the `combine=` / depth pair of
# the ops that write one.  A rejected operand is a ValueError; the frame I/O, JPEG and `frame_matte` builders assert, as they always did.
def _record(kind, ptrs, i=(), l=(), f=(), at=None, keep=None):
    """-> (op, keep): the record of `kind` with `ptrs` in p[0..], `at` ({slot: tensor or host address}) behind them, and the
    `i`, `l` and `f` values in order; `keep`: the tensors to hold when they are not `ptrs` and `at`'s"""
    op = L2dOp()
    op.kind = kind
    op.p[:len(ptrs)] = [None if t is None else t.data_ptr() for t in ptrs]
    if at:
        for j, t in at.items():
            op.p[j] = t if isinstance(t, int) else _ptr(t)
    if i:
        op.i[:len(i)] = [int(v) for v in i]
    if l:
        op.l[:len(l)] = [int(v) for v in l]
    if f:
        op.f[:len(f)] = [float(v) for v in f]
    if keep is None:
        keep = tuple(ptrs) + tuple(at.values()) if at else tuple(ptrs)
    return op, keep


def _f32_bits(v) -> int:
    """the bits of float32(v) as an int32: an fp32 value in an `i` field"""
    return int(np.float32(v).view(np.int32))


def _f64_bits(v) -> int:
    """the bits of float64(v) as an int64: a double in an `l` field"""
    return int(np.float64(v).view(np.int64))


def _got(t) -> str:
    return f"{getattr(t, 'dtype', None)} {tuple(getattr(t, 'shape', ()))}"


def _fp16_frame(name, t, H, W, B=None, align=0):
    """a contiguous fp16 [3,H,W] frame (unit dimensions in front are fine); `B`: a batch of B of them, checked by its size alone;
    `align`: at a multiple of that many bytes -- and with it an operand that is no tensor is refused here too"""
    if B is not None:
        if t.dtype != torch.float16 or t.numel() != B * 3 * H * W or not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous fp16 [{B},3,{H},{W}] frame, got {_got(t)}")
    elif (align and not torch.is_tensor(t)) or t.dtype != torch.float16 or tuple(t.shape[-3:]) != (3, H, W) or t.numel() != 3 * H * W \
            or not t.is_contiguous() or (align and t.data_ptr() % align):
        raise ValueError(f"{name}: expected a contiguous{f', {align}-byte aligned' if align else ''} fp16 [3,{H},{W}] frame, got {_got(t)}")


def _u8_planes(name, t, H, W, what="record", exact=False):
    """a contiguous planar uint8 [3,H,W] tensor: the bytes of a frame; `exact`: with no dimension in front"""
    if t.dtype != torch.uint8 or not t.is_contiguous() or (tuple(t.shape) != (3, H, W) if exact else
                                                          tuple(t.shape[-3:]) != (3, H, W) or t.numel() != 3 * H * W):
        raise ValueError(f"{name}: expected a contiguous planar uint8 [3,{H},{W}] {what}, got {_got(t)}")


def _u8_frame(name, t, H, W):
    """a contiguous interleaved uint8 [H,W,3] frame"""
    if t.dtype != torch.uint8 or tuple(t.shape[-3:]) != (H, W, 3) or t.numel() != H * W * 3 or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous uint8 [{H},{W},3] frame, got {_got(t)}")


def _i32_planes(name, t, H, W):
    """contiguous int32 [3,H,W] planes: the detail gains"""
    if t.dtype != torch.int32 or tuple(t.shape[-3:]) != (3, H, W) or t.numel() != 3 * H * W or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous int32 [3,{H},{W}] planes, got {_got(t)}")


def _fp32_plane(name, t, H, W, B=None, flat=False):
    """a contiguous fp32 [H,W] plane; `flat`: of any shape with that many elements; `B`: B planes, flat"""
    if B is not None:
        if t.dtype != torch.float32 or t.numel() != B * H * W or not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous float32 [{B},{H},{W}] plane, got {_got(t)}")
    elif t.dtype != torch.float32 or t.numel() != H * W or not (flat or tuple(t.shape[-2:]) == (H, W)) or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous float32 [{H},{W}] plane, got {_got(t)}")


def _fp16_depth(name, t, H, W):
    """a contiguous fp16 depth plane of H x W elements; None is refused like any other wrong operand"""
    if t is None or t.dtype != torch.float16 or t.numel() != H * W or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous fp16 [{H},{W}] plane, got {_got(t)}")


def _int_in(name, v, lo, hi, strict=False, note=""):
    """`v` (`name`: "<builder>: <argument>") is an integer from lo to hi: anything with an integer's value, or with `strict` an
    int or a numpy integer; never a bool"""
    if isinstance(v, bool) or (not isinstance(v, (int, np.integer)) if strict else int(v) != v) or not lo <= int(v) <= hi:
        raise ValueError(f"{name}={v!r}: use an integer from {lo} to {hi}{note}")


def _resample_tables(name, xmin, wx, ymin, wy, H, W):
    """the tables of a separable resample to H x W: per axis the int32 [n] first source index and the fp32 [n, taps] weights"""
    for axis, idx, w, n in (("x", xmin, wx, W), ("y", ymin, wy, H)):
        if idx.dtype != torch.int32 or idx.numel() != n or w.dtype != torch.float32 or w.ndim != 2 or w.shape[0] != n \
                or not idx.is_contiguous() or not w.is_contiguous():
            raise ValueError(f"{name}: the {axis} tables must be contiguous int32 [{n}] and fp32 [{n}, taps]")


def _axis_table(name, t, n_out, rows=0):
    """the int32 table of one output axis of `n_out` pixels: `rows` x n_out elements, or with `rows=0` `resize.axis_table`'s
    n_out x (2 + KS) -> KS.  `name`: "<builder>: tx" or "... ty" """
    if t.dtype != torch.int32 or not t.is_contiguous() or (t.numel() != rows * n_out if rows else t.numel() % n_out or t.numel() // n_out < 3):
        raise ValueError(f"{name} must be a contiguous int32 table of {f'{rows} x {n_out}' if rows else f'{n_out} x (2 + KS)'} elements, got "
                         f"{_got(t)}")
    return t.numel() // n_out - 2


def _matte_input(name, depth, plane, hard, far, lo32, inv32, H, W, B=None, stride=0, hard_name="hard"):
    """the matte input of an op that cuts by one -> (operand, lo32, inv32) as they go into the record: the fp16 `depth` under its
    ramp, or `plane=` (fp32, with `depth=None`), ready matte values that carry the ramp, `hard` and `far`.  `B`: B planes `stride`
    elements apart (`frame_matte`, `frame_matte_up`), of at least that size; there the depth is asserted"""
    if plane is None:
        if B is None:
            _fp16_depth(name + ": depth", depth, H, W)
        else:
            assert depth.dtype == torch.float16 and depth.numel() >= (B - 1) * stride + H * W
        return depth, lo32, inv32
    if depth is not None or hard or far:
        raise ValueError(f"{name}: plane= goes with depth=None, and without {hard_name} / far (the plane carries them)")
    if B is None:
        _fp32_plane(name + ": plane", plane, H, W)
    elif plane.dtype != torch.float32 or not plane.is_contiguous() or plane.numel() < (B - 1) * stride + H * W:
        raise ValueError(f"{name}: plane must be a contiguous float32 tensor of at least {(B - 1) * stride + H * W} elements, got {_got(plane)}")
    return plane, 0.0, 0.0


def _ramp_input(name, combine, flags, depth, lo32, inv32, hard, far, H, W):
    """the second input of an op that writes a matte -> (depth, lo32, inv32, hard, far) as they go into the record: `combine` (a
    key of `flags`) "and" / "or" reads the fp16 `depth` plane under the ramp; "replace" reads neither, and drops them"""
    if combine not in flags:
        raise ValueError(f"{name}: combine={combine!r}: use 'replace', 'and' or 'or'")
    if combine == "replace":
        return None, 0.0, 0.0, False, False
    _fp16_depth(name + ": depth", depth, H, W)
    return depth, lo32, inv32, hard, far


def frame_ingest(src, dst, *, B, Hs, Ws, H, W, nh, nw, top, left):
    """uint8 [B,Hs,Ws,3] -> fp16 [B,3,H,W] in [-1, 1]: antialiased resize to (nh, nw) + crop at (top, left) (frame_io.geometry)."""
    assert src.dtype == torch.uint8 and dst.dtype == torch.float16
    return _record(_lib.OP_FRAME_INGEST, (src, dst), (B, Hs, Ws, H, W, nh, nw, top, left))


def frame_egress(src, dst, *, B, H, W):
    """fp16 [B,3,H,W] in [-1, 1] -> uint8 [B,H,W,3] with the reference's rounding points (image_utils.py:13,30)."""
    assert src.dtype == torch.float16 and dst.dtype == torch.uint8
    return _record(_lib.OP_FRAME_EGRESS, (src, dst), (B, H, W))


# ----------------------------------------------------------------------------- baseline JPEG (jpeg.hip, jpeg.py)
JPEG_MAX_W = 1920      # jpeg.hip JPG_MAX_W: an MCU row is entropy-coded in LDS
JPEG_HDR_OFF = 16      # jpeg.hip JPG_HDR_OFF: a frame's slot holds the file's length (int32) and, from byte 16, the file


def jpeg_dct(src, coef, *, B, H, W, quality):
    """fp16 [B,3,H,W] in [-1, 1] (the egress op's bytes first) or uint8 [B,H,W,3] -> int16 [B][H/16][W/16][6][64] quantised
    coefficients, zigzag order (jpeg.coefficients)"""
    assert src.dtype in (torch.float16, torch.uint8) and coef.dtype == torch.int16
    assert src.numel() >= B * H * W * 3 and coef.numel() >= B * H * W * 3 // 2
    return _record(_lib.OP_JPEG_DCT, (src, coef), (B, H, W, src.dtype == torch.uint8, quality))


def jpeg_huff(coef, tables, staging, lengths, *, B, H, W, row_stride):
    """coefficients -> every MCU row entropy-coded, padded, stuffed and closed with its marker, in its slot of `staging`
    (uint8 [B][H/16][row_stride]); `lengths` int32 [B][H/16]; `tables` int32 [544] (jpeg.Tables.packed)"""
    assert coef.dtype == torch.int16 and tables.dtype == torch.int32 and staging.dtype == torch.uint8 and lengths.dtype == torch.int32
    assert tables.numel() >= 544 and staging.numel() >= B * (H // 16) * row_stride and lengths.numel() >= B * (H // 16)
    return _record(_lib.OP_JPEG_HUFF, (coef, tables, staging, lengths), (B, H, W, row_stride))


def jpeg_pack(staging, lengths, header, out, *, B, H, row_stride, out_stride):
    """rows -> per frame `out[b]` = int32 length, 12 unused bytes, header, rows (uint8 [B][out_stride])"""
    assert staging.dtype == header.dtype == out.dtype == torch.uint8 and lengths.dtype == torch.int32
    assert out.numel() >= B * out_stride
    return _record(_lib.OP_JPEG_PACK, (staging, lengths, header, out), (B, H, row_stride, header.numel()), (out_stride,))


# ----------------------------------------------------------------------------- baseline JPEG decoder (jpeg_dec.hip, jpeg.py)
def jpeg_index(info, data, chunk_mcus, blob=None, offsets=None, dc_pred=None):
    """l2d_jpeg_index (host): (bit_offsets int32 [C + 1], dc_pred int16 [C][3]) of `jpeg.index_ref`, written into the given numpy
    arrays when there are any (the decoder's pinned staging buffer).  A damaged scan raises ValueError."""
    from . import jpeg
    C = jpeg.chunk_layout(info.n_mcu, info.restart_interval, chunk_mcus)[3]
    blob = jpeg.table_blob(info) if blob is None else blob
    offsets = np.empty(C + 1, np.int32) if offsets is None else offsets
    dc_pred = np.empty((C, 3), np.int16) if dc_pred is None else dc_pred
    assert offsets.dtype == np.int32 and offsets.size == C + 1 and dc_pred.dtype == np.int16 and dc_pred.size == 3 * C
    assert offsets.flags.c_contiguous and dc_pred.flags.c_contiguous and blob.dtype == np.uint8 and blob.size == jpeg.DEC_BLOB_BYTES
    file = data if isinstance(data, np.ndarray) else np.frombuffer(data, np.uint8)
    lay = np.array([info.scan_offset, info.n_mcu, info.hs * info.vs, info.restart_interval, chunk_mcus, *info.dc_tab, *info.ac_tab, C], np.int32)
    rc = _lib.lib.l2d_jpeg_index(file.ctypes.data, file.size, blob.ctypes.data, lay.ctypes.data, offsets.ctypes.data, dc_pred.ctypes.data)
    if rc != 0:
        raise ValueError(f"jpeg: the scan is damaged: {_lib.lib.l2d_last_error().decode(errors='replace')}")
    return offsets, dc_pred


def jpeg_entropy_dec(file, offsets, dc_pred, blob, params, coef, status, *, n_mcu, ny, restart_interval, chunk_mcus, C, dc_tab, ac_tab):
    """the stuffed scan -> int16 [n_mcu][ny + 2][64] coefficients (jpeg.decode_coefficients_ref), one lane per chunk"""
    assert file.dtype == blob.dtype == torch.uint8 and offsets.dtype == params.dtype == status.dtype == torch.int32
    assert dc_pred.dtype == coef.dtype == torch.int16
    assert offsets.numel() >= C + 1 and dc_pred.numel() >= 3 * C and blob.numel() >= 3648 and params.numel() >= 2
    assert coef.numel() >= n_mcu * (ny + 2) * 64
    return _record(_lib.OP_JPEG_ENTROPY_DEC, (file, offsets, dc_pred, blob, params, coef, status),
                   (n_mcu, ny, restart_interval, chunk_mcus, C, file.numel(), *dc_tab, *ac_tab))


def jpeg_idct(coef, quant, planes, *, n_mcu, mcus_x, hs, vs):
    """coefficients -> the three uint8 component planes at their padded sizes (jpeg.planes_ref); `quant` uint16 [3][64] as bytes"""
    assert coef.dtype == torch.int16 and planes.dtype == torch.uint8 and quant.numel() * quant.element_size() >= 384
    assert coef.numel() >= n_mcu * (hs * vs + 2) * 64 and planes.numel() >= n_mcu * (hs * vs + 2) * 64
    return _record(_lib.OP_JPEG_IDCT, (coef, quant, planes), (n_mcu, mcus_x, hs, vs))


def jpeg_rgb(planes, out, *, H, W, hs, vs):
    """component planes -> uint8 [H][W][3]: fancy up-sampling and colour conversion (jpeg.upsample_ref, jpeg.ycc_to_rgb_ref)"""
    assert planes.dtype == out.dtype == torch.uint8 and out.numel() >= H * W * 3
    assert planes.numel() >= (-(-W // (8 * hs))) * (-(-H // (8 * vs))) * (hs * vs + 2) * 64
    return _record(_lib.OP_JPEG_RGB, (planes, out), (H, W, hs, vs))


# ----------------------------------------------------------------------------- style switch / blend (wblend.hip, style_bank.py)
WBLEND_MAX_SRC = 4              # l2d.h L2D_WBLEND_MAX_SRC
WBLEND_TILE_BYTES = 65536       # l2d.h L2D_WBLEND_TILE_BYTES
WBLEND_DTYPES = {torch.float16: 0, torch.float32: 1}
WBLEND_REC = np.dtype([("dst", "<u8"), ("src", "<u8", (4,)), ("n", "<i8"), ("dtype", "<i4"), ("pad", "<i4", (3,))])    # l2d_wblend_rec
WBLEND_NT = 1                   # cache policy of the launch: 0 plain, 1 non-temporal -- the faster one for K = 1, 2, 3 (profiles/style_switch_time.txt)


def weight_blend(table_dev, table_host, weights, *, nt=None):
    """dst = sum_k weights[k] * src_k over every record of the table, one launch.  `table_dev`: the l2d_wblend_rec records as a
    uint8 tensor on the device; `table_host`: the same records as a numpy array of WBLEND_REC (the launcher validates on it)."""
    assert table_host.dtype == WBLEND_REC and table_host.flags["C_CONTIGUOUS"]
    assert table_dev.dtype == torch.uint8 and table_dev.numel() == table_host.nbytes
    return _record(_lib.OP_WEIGHT_BLEND, (table_dev,), (len(table_host), len(weights), WBLEND_NT if nt is None else nt), f=list(weights)[:4],
                   at={1: table_host.ctypes.data}, keep=(table_dev, table_host))


# ----------------------------------------------------------------------------- depth matte (matte.hip, matte.py)
MATTE_HARD, MATTE_FAR, MATTE_SHOW = 1, 2, 4      # l2d.h L2D_MATTE_*
MATTE_MAX_R = 8                                  # l2d.h L2D_MATTE_MAX_R
MATTE_PLANE = 16                                 # l2d.h L2D_MATTE_PLANE
MATTE_EDGE_MAX_R = 8                             # l2d.h L2D_MATTE_EDGE_MAX_R
MATTE_EDGE_PLANE = 32                            # l2d.h L2D_MATTE_EDGE_PLANE


def frame_matte(styled, source, depth, dst, *, B, H, W, lo32=0.0, inv32=0.0, hard=False, far=False, show=False, r=0, depth_stride=None,
                plane=None):
    """fp16 [B,3,H,W] styled / source + fp16 depth planes ([B,H,W], or channel 0 of a [B,3,H,W] tensor with `depth_stride=3 H W`)
    -> uint8 [B,H,W,3]: the egress bytes of `styled` over those of `source` by the depth matte (matte.composite_ref);
    `lo32, inv32, hard` as `matte.matte_params` returns them.  `plane` (fp32 [B,H,W], with `depth=None`): ready matte values in
    place of the depth planes, as `frame_matte_edge` writes them; the ramp, `hard` and `far` do not apply."""
    assert styled.dtype == source.dtype == torch.float16 and dst.dtype == torch.uint8
    stride = H * W if depth_stride is None else int(depth_stride)
    assert styled.numel() >= B * 3 * H * W and source.numel() >= B * 3 * H * W and dst.numel() >= B * H * W * 3
    matte, lo32, inv32 = _matte_input("frame_matte", depth, plane, hard, far, lo32, inv32, H, W, B, stride)
    flags = ((MATTE_HARD if hard else 0) | (MATTE_FAR if far else 0) | (MATTE_SHOW if show else 0)
             | (MATTE_PLANE if plane is not None else 0))
    return _record(_lib.OP_FRAME_MATTE, (styled, source, matte, dst), (B, H, W, r, flags), (stride,), (lo32, inv32))


def frame_matte_edge(source, depth, out, *, H, W, r, E, lo32=0.0, inv32=0.0, hard=False, far=False, plane=None):
    """fp16 [3,H,W] `source` + fp16 [H,W] `depth` -> fp32 [H,W] `out`: the matte of `frame_matte` in front of its feather, refined
    by the source frame (matte.edge_ref).  `r`: the radius, 1..MATTE_EDGE_MAX_R; `E`: `matte.edge_E(r, eps)`, a Python float;
    `lo32, inv32, hard` as `matte.matte_params` returns them.  `plane` (fp32 [H,W], with `depth=None`): a ready raw matte, as
    `mask_ingest` writes it, in place of the depth plane; the ramp, `hard` and `far` do not apply."""
    _fp16_frame("frame_matte_edge: source", source, H, W)
    matte, lo32, inv32 = _matte_input("frame_matte_edge", depth, plane, hard, far, lo32, inv32, H, W)
    _fp32_plane("frame_matte_edge: out", out, H, W, flat=True)
    _int_in("frame_matte_edge: r", r, 1, MATTE_EDGE_MAX_R)
    flags = (MATTE_HARD if hard else 0) | (MATTE_FAR if far else 0) | (MATTE_EDGE_PLANE if plane is not None else 0)
    return _record(_lib.OP_FRAME_MATTE_EDGE, (source, matte, out), (H, W, r, flags), (_f64_bits(E),), (lo32, inv32))


# ----------------------------------------------------------------------------- backdrop blur (backdrop.hip, backdrop.py)
BACKDROP_MAX_R = 8                               # l2d.h L2D_BACKDROP_MAX_R
BACKDROP_MAX_PASSES = 3                          # l2d.h L2D_BACKDROP_MAX_PASSES
BACKDROP_PLANE = 32                              # l2d.h L2D_BACKDROP_PLANE


def frame_backdrop_blur(source, depth, out, *, H, W, r, passes, lo32=0.0, inv32=0.0, hard=False, far=False, plane=None):
    """fp16 [3,H,W] `source` + fp16 [H,W] `depth` -> fp16 [3,H,W] `out`: the source frame blurred with the matte's subject left
    out, as a frame `frame_matte` takes for its kept part (backdrop.frame_of(backdrop.blur_ref(...))).  `r`: the radius,
    1..BACKDROP_MAX_R; `passes`: 1..BACKDROP_MAX_PASSES; `lo32, inv32, hard` as `matte.matte_params` returns them.  `plane` (fp32
    [H,W], with `depth=None`): a ready raw matte, as `mask_ingest` writes it, in place of the depth plane; the ramp, `hard` and
    `far` do not apply."""
    _fp16_frame("frame_backdrop_blur: source", source, H, W)
    _fp16_frame("frame_backdrop_blur: out", out, H, W)
    matte, lo32, inv32 = _matte_input("frame_backdrop_blur", depth, plane, hard, far, lo32, inv32, H, W)
    _int_in("frame_backdrop_blur: r", r, 1, BACKDROP_MAX_R)
    _int_in("frame_backdrop_blur: passes", passes, 1, BACKDROP_MAX_PASSES)
    flags = (MATTE_HARD if hard else 0) | (MATTE_FAR if far else 0) | (BACKDROP_PLANE if plane is not None else 0)
    return _record(_lib.OP_FRAME_BACKDROP_BLUR, (source, matte, out), (H, W, r, passes, flags), f=(lo32, inv32))


# ----------------------------------------------------------------------------- colour lock (colorlock.hip, color_lock.py)
COLOR_LOCK_INIT, COLOR_LOCK_SOURCE, COLOR_LOCK_FREEZE = 1, 2, 4      # l2d.h L2D_COLOR_LOCK_*
COLOR_LOCK_BLOCK_PIXELS = 4096                                       # l2d.h L2D_COLOR_LOCK_BLOCK_PIXELS
COLOR_LOCK_MAX_PIXELS = 1 << 22                                      # l2d.h L2D_COLOR_LOCK_MAX_PIXELS


def color_lock_blocks(H, W):
    """the number of partial records one tensor of H x W pixels has"""
    return -(-(int(H) * int(W)) // COLOR_LOCK_BLOCK_PIXELS)


def frame_moments(frame, second, partials, *, H, W):
    """fp16 [3,H,W] `frame` (and `second`, or None) -> uint32 (as int32) partials [1 or 2][blocks][6]: per block of
    COLOR_LOCK_BLOCK_PIXELS pixels and per channel the sum and the sum of squares of the egress bytes (color_lock.sums_ref)"""
    nt, nblk = (1 if second is None else 2), color_lock_blocks(H, W)
    _fp16_frame("frame_moments: frame", frame, H, W)
    if second is not None:
        _fp16_frame("frame_moments: second", second, H, W)
    if partials.dtype != torch.int32 or partials.numel() < nt * nblk * 6:
        raise ValueError(f"frame_moments: partials must be int32 with at least {nt * nblk * 6} elements, got {_got(partials)}")
    return _record(_lib.OP_FRAME_MOMENTS, (frame, second, partials), (H, W, nt, nblk))


def color_lock(styled, out, partials, state_in, state_out, coef, *, H, W, strength, rate, init=False, source=False, freeze=False):
    """fp16 [3,H,W] `styled` + the partials `frame_moments` wrote (of `styled`, and with `source` of the target frame behind them)
    + float64 [3,2] `state_in` -> fp16 [3,H,W] `out`, float64 [3,2] `state_out`, float32 [3,3] `coef`: color_lock.lock_ref"""
    nblk = color_lock_blocks(H, W)
    _fp16_frame("color_lock: styled", styled, H, W)
    _fp16_frame("color_lock: out", out, H, W)
    if partials.dtype != torch.int32 or partials.numel() < (2 if source else 1) * nblk * 6:
        raise ValueError(f"color_lock: partials must be int32 with at least {(2 if source else 1) * nblk * 6} elements")
    for name, t in (("state_in", state_in), ("state_out", state_out)):
        if t.dtype != torch.float64 or t.numel() != 6 or not t.is_contiguous():
            raise ValueError(f"color_lock: {name} must be a contiguous float64 [3,2] record, got {_got(t)}")
    if coef.dtype != torch.float32 or coef.numel() != 9 or not coef.is_contiguous():
        raise ValueError(f"color_lock: coef must be a contiguous float32 [3,3] record, got {_got(coef)}")
    flags = (COLOR_LOCK_INIT if init else 0) | (COLOR_LOCK_SOURCE if source else 0) | (COLOR_LOCK_FREEZE if freeze else 0)
    return _record(_lib.OP_COLOR_LOCK, (styled, out, partials, state_in, state_out, coef), (H, W, flags, nblk),
                   (_f64_bits(rate), _f64_bits(strength)))


# ----------------------------------------------------------------------------- output size (resize.hip, resize.py)
RESIZE_MAX_KS = 13              # l2d.h L2D_RESIZE_MAX_KS
RESIZE_MAX_SIZE = 4096          # l2d.h L2D_RESIZE_MAX_SIZE
RESIZE_TILE = 32                # resize.hip RS_TW = RS_TH: a tile reads at most 2 * RESIZE_TILE + RESIZE_MAX_KS source pixels per axis


def frame_resize(src, dst, tx, ty, *, B, H, W, Ho, Wo, src_pitch=None):
    """fp16 [B,3,H,W] in [-1, 1] (the egress op's bytes first) or uint8 [B,H,W,3] -> uint8 [B,Ho,Wo,3], Pillow's resampling
    (resize.resize_ref); `tx`, `ty`: the int32 tables of the two axes as `resize.axis_table` lays them out.  `src_pitch` (uint8,
    B == 1): `src` begins at the first pixel of an H x W window of a frame whose rows are `src_pitch` pixels apart -- a view of the
    frame from that pixel on; None or 0: W."""
    assert src.dtype in (torch.float16, torch.uint8) and dst.dtype == torch.uint8
    pitch = int(src_pitch or 0)
    if pitch:
        avail = src.untyped_storage().nbytes() - src.storage_offset()         # (uint8: bytes from the window's first pixel on)
        assert avail >= ((H - 1) * pitch + W) * 3, (avail, H, W, pitch)
    else:
        assert src.numel() >= B * H * W * 3
    assert dst.numel() >= B * Ho * Wo * 3
    ksx, ksy = _axis_table("frame_resize: tx", tx, Wo), _axis_table("frame_resize: ty", ty, Ho)
    return _record(_lib.OP_FRAME_RESIZE, (src, dst, tx, ty), (B, H, W, Ho, Wo, src.dtype == torch.uint8, ksx, ksy, pitch))


def frame_matte_up(styled, camera, depth, dst, tx, ty, *, B, H, W, Ho, Wo, lo32=0.0, inv32=0.0, hard=False, far=False, show=False, r=0,
                   depth_stride=None, plane=None):
    """uint8 [B,Ho,Wo,3] styled / camera + fp16 depth planes [B,H,W] (`depth_stride` as `frame_matte`'s) -> uint8 [B,Ho,Wo,3]: the
    styled bytes over the camera's by the depth matte sampled at the output size (matte.composite_up_ref); `tx`, `ty`: int32
    [3, n_out] tables of the two axes as `matte.up_table` returns them (i0, i1, the bits of f).  `plane` (fp32 [B,H,W], with
    `depth=None`): as `frame_matte`'s."""
    assert styled.dtype == camera.dtype == dst.dtype == torch.uint8
    stride = H * W if depth_stride is None else int(depth_stride)
    n = B * Ho * Wo * 3
    assert styled.numel() >= n and camera.numel() >= n and dst.numel() >= n
    matte, lo32, inv32 = _matte_input("frame_matte_up", depth, plane, hard, far, lo32, inv32, H, W, B, stride)
    _axis_table("frame_matte_up: tx", tx, Wo, 3)
    _axis_table("frame_matte_up: ty", ty, Ho, 3)
    flags = ((MATTE_HARD if hard else 0) | (MATTE_FAR if far else 0) | (MATTE_SHOW if show else 0)
             | (MATTE_PLANE if plane is not None else 0))
    return _record(_lib.OP_FRAME_MATTE_UP, (styled, camera, matte, dst, tx, ty), (B, H, W, Ho, Wo, r, flags), (stride,), (lo32, inv32))


# ----------------------------------------------------------------------------- steady (steady.hip, steady.py)
STEADY_HARD, STEADY_SHOW, STEADY_INIT = 1, 2, 4      # l2d.h L2D_STEADY_*
STEADY_MAX_R = 8                                     # l2d.h L2D_STEADY_MAX_R


def _steady_picture(name, show, picture, H, W):
    """the fp16 [3,H,W] `picture` of the weight, there exactly with `show`"""
    if bool(show) != (picture is not None):
        raise ValueError(f"{name}: a picture buffer goes with show=True, and with nothing else")
    if picture is not None:
        _fp16_frame(name + ": picture", picture, H, W)


def frame_steady(styled, source, prev_out, prev_bytes, out, next_bytes, *, H, W, lo32, inv32, s32, r=0, hard=False, show=False,
                 init=False, picture=None):
    """fp16 [3,H,W] `styled`, `source`, `prev_out` + planar uint8 [3,H,W] `prev_bytes` -> fp16 [3,H,W] `out`, uint8 [3,H,W]
    `next_bytes` (steady.steady_ref): the previous output held where the source's bytes did not move.  `lo32, inv32, hard` as
    `steady.steady_params` returns them, `s32` the strength; `show` also writes the picture of the weight to `picture`; with
    `init` the two `prev_*` operands are not read and may be None."""
    _fp16_frame("frame_steady: styled", styled, H, W)
    _fp16_frame("frame_steady: source", source, H, W)
    _fp16_frame("frame_steady: out", out, H, W)
    if prev_out is not None or not init:
        _fp16_frame("frame_steady: prev_out", prev_out, H, W)
    if prev_bytes is not None or not init:
        _u8_planes("frame_steady: prev_bytes", prev_bytes, H, W)
    _u8_planes("frame_steady: next_bytes", next_bytes, H, W)
    _steady_picture("frame_steady", show, picture, H, W)
    _int_in("frame_steady: r", r, 0, STEADY_MAX_R)
    flags = (STEADY_HARD if hard else 0) | (STEADY_SHOW if show else 0) | (STEADY_INIT if init else 0)
    return _record(_lib.OP_FRAME_STEADY, (styled, source, prev_out, prev_bytes, out, next_bytes, picture), (H, W, r, flags),
                   f=(lo32, inv32, s32))


# ----------------------------------------------------------------------------- follow (steady_follow.hip, steady.py)
FOLLOW_BLOCK, FOLLOW_APRON = 8, 4                    # l2d.h L2D_FOLLOW_*
FOLLOW_MAX_SEARCH, FOLLOW_MAX_BIAS = 8, 4096


def _follow_field(name, field, H, W):
    shape = ((H + FOLLOW_BLOCK - 1) // FOLLOW_BLOCK, W // FOLLOW_BLOCK, 2)
    if field.dtype != torch.int8 or tuple(field.shape) != shape or not field.is_contiguous():
        raise ValueError(f"{name}: field: expected a contiguous int8 {list(shape)} field, got {_got(field)}")


def frame_motion(source, prev_bytes, field, *, H, W, search, bias):
    """the fp16 [3,H,W] `source` frame + the planar uint8 [3,H,W] `prev_bytes` of the steady state -> int8 [ceil(H/8), W/8, 2]
    `field`: per 8 x 8 block the vector (dy, dx) of the best match of the frame's bytes in the previous ones
    (steady.motion_ref).  `search`: 1..FOLLOW_MAX_SEARCH pixels; `bias`: 0..FOLLOW_MAX_BIAS summed byte levels per pixel of L1
    displacement."""
    _fp16_frame("frame_motion: source", source, H, W)
    _u8_planes("frame_motion: prev_bytes", prev_bytes, H, W)
    _follow_field("frame_motion", field, H, W)
    _int_in("frame_motion: search", search, 1, FOLLOW_MAX_SEARCH)
    _int_in("frame_motion: bias", bias, 0, FOLLOW_MAX_BIAS)
    return _record(_lib.OP_FRAME_MOTION, (source, prev_bytes, field), (H, W, search, bias))


def frame_steady_follow(styled, source, prev_out, prev_bytes, out, next_bytes, field, *, H, W, lo32, inv32, s32, r=0, hard=False,
                        show=False, picture=None):
    """`frame_steady` with the previous record fetched along `field` (`frame_motion`'s; steady.follow_ref): the previous output
    held where the source's bytes did not move relative to where they came from.  No `init`: an init frame is `frame_steady`'s."""
    for name, t in (("styled", styled), ("source", source), ("prev_out", prev_out), ("out", out)):
        _fp16_frame("frame_steady_follow: " + name, t, H, W)
    _u8_planes("frame_steady_follow: prev_bytes", prev_bytes, H, W)
    _u8_planes("frame_steady_follow: next_bytes", next_bytes, H, W)
    _follow_field("frame_steady_follow", field, H, W)
    _steady_picture("frame_steady_follow", show, picture, H, W)
    _int_in("frame_steady_follow: r", r, 0, STEADY_MAX_R)
    flags = (STEADY_HARD if hard else 0) | (STEADY_SHOW if show else 0)
    return _record(_lib.OP_FRAME_STEADY_FOLLOW, (styled, source, prev_out, prev_bytes, out, next_bytes, picture, field), (H, W, r, flags),
                   f=(lo32, inv32, s32))


# ----------------------------------------------------------------------------- matte hold (matte_hold.hip, matte.py)
MATTE_HOLD_HARD, MATTE_HOLD_INIT, MATTE_HOLD_PLANE, MATTE_HOLD_FOLLOW = 1, 4, 16, 32      # l2d.h L2D_MATTE_HOLD_*
MATTE_HOLD_RAMP_HARD, MATTE_HOLD_RAMP_FAR = 64, 128


def frame_matte_hold(source, depth, prev_plane, prev_bytes, out_plane, next_bytes, *, H, W, lo32, inv32, s32, r=0, hard=False,
                     init=False, plane=None, ramp_lo32=0.0, ramp_inv32=0.0, ramp_hard=False, far=False, field=None):
    """the fp16 [3,H,W] `source` frame + the matte input + the previous record (`prev_plane` fp32 [H,W], `prev_bytes` planar uint8
    [3,H,W]) -> the next record (`out_plane`, `next_bytes`): the matte held where the source's bytes did not move
    (matte.hold_ref).  The matte input is the fp16 [H,W] `depth` plane under the ramp `ramp_lo32, ramp_inv32, ramp_hard`
    (`matte.matte_params`) and `far`, or `plane` (fp32 [H,W], with `depth=None`): ready matte values, as `frame_matte_edge` writes
    them.  `lo32, inv32, hard` as `steady.steady_params` returns them, `s32` the strength; `field` (`frame_motion`'s): the
    previous record is fetched along it; with `init` the previous record and the field are not read and may be None."""
    _fp16_frame("frame_matte_hold: source", source, H, W)
    matte, ramp_lo32, ramp_inv32 = _matte_input("frame_matte_hold", depth, plane, ramp_hard, far, ramp_lo32, ramp_inv32, H, W,
                                                hard_name="ramp_hard")
    if prev_plane is not None or not init:
        _fp32_plane("frame_matte_hold: prev_plane", prev_plane, H, W)
    if prev_bytes is not None or not init:
        _u8_planes("frame_matte_hold: prev_bytes", prev_bytes, H, W)
    _fp32_plane("frame_matte_hold: out_plane", out_plane, H, W)
    _u8_planes("frame_matte_hold: next_bytes", next_bytes, H, W)
    if field is not None:
        _follow_field("frame_matte_hold", field, H, W)
    _int_in("frame_matte_hold: r", r, 0, STEADY_MAX_R)
    flags = ((MATTE_HOLD_HARD if hard else 0) | (MATTE_HOLD_INIT if init else 0) | (MATTE_HOLD_PLANE if plane is not None else 0)
             | (MATTE_HOLD_FOLLOW if field is not None else 0) | (MATTE_HOLD_RAMP_HARD if ramp_hard else 0)
             | (MATTE_HOLD_RAMP_FAR if far else 0))
    return _record(_lib.OP_FRAME_MATTE_HOLD, (source, matte, prev_plane, prev_bytes, out_plane, next_bytes, field),
                   (H, W, r, flags, _f32_bits(ramp_lo32), _f32_bits(ramp_inv32)), f=(lo32, inv32, s32))


# ----------------------------------------------------------------------------- detail mode (detail.hip, detail.py)
DETAIL_U8, DETAIL_SHOW = 1, 2                        # l2d.h L2D_DETAIL_*
DETAIL_MAX_GAIN = 261120                             # |A| = |rint(4096 a)| with |a| <= 127.5 / 2 (eps >= 1): detail.hip states it


def frame_detail_gain(frame, source, out, *, H, W, r, E):
    """the frame the resize reads -- fp16 [3,H,W] (its egress bytes) or uint8 [H,W,3] (the matte's frame) -- + the fp16 [3,H,W]
    `source` frame -> int32 [3,H,W] `out`: per channel n 4096 times the mean over the window of the regression slope of the
    frame's bytes on the source frame's luma (detail.gains_ref).  `r`: the radius, 1..MATTE_EDGE_MAX_R; `E`:
    `matte.edge_E(r, eps)`, a Python float."""
    u8 = frame.dtype == torch.uint8
    (_u8_frame if u8 else _fp16_frame)("frame_detail_gain: frame", frame, H, W)
    _fp16_frame("frame_detail_gain: source", source, H, W)
    _i32_planes("frame_detail_gain: out", out, H, W)
    _int_in("frame_detail_gain: r", r, 1, MATTE_EDGE_MAX_R)
    return _record(_lib.OP_FRAME_DETAIL_GAIN, (frame, source, out), (H, W, r, DETAIL_U8 if u8 else 0), (_f64_bits(E),))


def frame_detail(styled, camera, low, gains, tx, ty, dst, *, H, W, Ho, Wo, k, limit, show=False):
    """uint8 [Ho,Wo,3] `styled` (S), `camera` (C) and `low` (L: the source frame through S's resize) + the int32 [3,H,W] `gains`
    of `frame_detail_gain` -> uint8 [Ho,Wo,3] `dst`: S + clamp(g (luma(C) - luma(L)) k, +-limit) with g the gains sampled
    bilinearly (detail.inject_ref).  `tx`, `ty`: int32 [3, n_out] tables as `matte.table_words` builds them; `k`:
    float32(strength / (n 4096)); `show` writes 128 + the injected term."""
    for name, t in (("styled", styled), ("camera", camera), ("low", low), ("dst", dst)):
        _u8_frame("frame_detail: " + name, t, Ho, Wo)
    _i32_planes("frame_detail: gains", gains, H, W)
    _axis_table("frame_detail: tx", tx, Wo, 3)
    _axis_table("frame_detail: ty", ty, Ho, 3)
    for name, t in (("styled", styled), ("camera", camera), ("low", low)):
        if t.data_ptr() == dst.data_ptr():
            raise ValueError(f"frame_detail: dst may not be the {name} frame")
    k, limit = float(k), float(limit)
    if not (np.isfinite(k) and k >= 0.0 and np.isfinite(limit) and limit >= 0.0):
        raise ValueError(f"frame_detail: k={k!r} and limit={limit!r} must be finite and not negative")
    return _record(_lib.OP_FRAME_DETAIL, (styled, camera, low, gains, tx, ty, dst), (H, W, Ho, Wo, DETAIL_SHOW if show else 0), f=(k, limit))


# ----------------------------------------------------------------------------- depth from the caller (depth_in.hip, depth_io.py)
DEPTH_F32, DEPTH_DISTANCE, DEPTH_HAS_INVALID, DEPTH_FIXED_RANGE = 1, 2, 4, 8      # l2d.h L2D_DEPTH_*
DEPTH_TILE_H, DEPTH_TILE_W, DEPTH_MAX_TAPS = 16, 32, 17


def depth_tiles(H: int, W: int) -> int:
    """work-groups (and {min, max, any} partials) of one frame of `depth_ingest`"""
    return ((H + DEPTH_TILE_H - 1) // DEPTH_TILE_H) * ((W + DEPTH_TILE_W - 1) // DEPTH_TILE_W)


def _depth_partials(name, partials, n):
    """the fp32 [n,3] {min, max, any} records of `depth_ingest`, one per tile"""
    if partials.dtype != torch.float32 or partials.numel() != n * 3 or not partials.is_contiguous():
        raise ValueError(f"{name}: partials: expected contiguous fp32 [{n},3], got {_got(partials)}")


def depth_ingest(src, R, partials, xmin, wx, ymin, wy, *, B, Hd, Wd, H, W, nh, nw, top, left, distance, invalid):
    """uint16 / fp32 [B,Hd,Wd] `src` -> fp32 [B,H,W] `R` (the normalised convolution of u = z or 1 / z over the valid samples,
    -1 where a pixel has no value) and fp32 [B tiles, 3] `partials` ({min, max, any} per tile): depth_io.resample_ref.
    `xmin`, `wx`, `ymin`, `wy`: the tables of `depth_io.tables`; `invalid`: the value that marks a hole, or None."""
    f32 = src.dtype == torch.float32
    if not f32 and src.dtype not in (torch.uint16, torch.int16):          # (int16: the bits of uint16 samples)
        raise ValueError(f"depth_ingest: src: expected uint16 or float32 samples, got {src.dtype}")
    if src.numel() != B * Hd * Wd or not src.is_contiguous():
        raise ValueError(f"depth_ingest: src: expected a contiguous [{B},{Hd},{Wd}] frame, got {tuple(src.shape)}")
    _fp32_plane("depth_ingest: R", R, H, W, B)
    _depth_partials("depth_ingest", partials, B * depth_tiles(H, W))
    _resample_tables("depth_ingest", xmin, wx, ymin, wy, H, W)
    flags = (DEPTH_F32 if f32 else 0) | (DEPTH_DISTANCE if distance else 0)
    inv_i, inv_f = 0, 0.0
    if invalid is not None:
        if f32:
            flags |= DEPTH_HAS_INVALID
            inv_f = float(np.float32(invalid))
        elif float(invalid) == int(invalid) and 0 <= int(invalid) <= 65535:     # (no uint16 sample equals any other value)
            flags |= DEPTH_HAS_INVALID
            inv_i = int(invalid)
    return _record(_lib.OP_DEPTH_INGEST, (src, R, partials, xmin, wx, ymin, wy),
                   (B, Hd, Wd, H, W, nh, nw, top, left, wx.shape[1], wy.shape[1], flags, inv_i), f=(inv_f,))


def depth_normalize(R, partials, out, *, B, H, W, fixed=None):
    """fp32 [B,H,W] `R` + the partials of all B frames -> fp16 [B,3,H,W] `out` in [-1, 1]: depth_io.normalize_ref.  `fixed`:
    (mn, mx) as float32 in units of u, or None: min and max over the partials"""
    _fp32_plane("depth_normalize: R", R, H, W, B)
    _fp16_frame("depth_normalize: out", out, H, W, B)
    npart = B * depth_tiles(H, W)
    _depth_partials("depth_normalize", partials, npart)
    return _record(_lib.OP_DEPTH_NORMALIZE, (R, partials, out), (B, H, W, npart, DEPTH_FIXED_RANGE if fixed is not None else 0),
                   f=() if fixed is None else (fixed[0], fixed[1]))


# ----------------------------------------------------------------------------- the matte from the caller (mask_in.hip, mask_io.py)
MASK_U16, MASK_F32, MASK_INVERT, MASK_AND, MASK_OR, MASK_RAMP_HARD, MASK_RAMP_FAR = 1, 2, 4, 8, 16, 64, 128      # l2d.h L2D_MASK_*
MASK_COMBINE = {"replace": 0, "and": MASK_AND, "or": MASK_OR}


def mask_ingest(src, out, depth, xmin, wx, ymin, wy, *, Hm, Wm, H, W, nh, nw, top, left, combine="replace", invert=False, lo32=0.0,
                inv32=0.0, hard=False, far=False):
    """uint8 / uint16 / fp32 [Hm,Wm] `src` -> fp32 [H,W] `out`: the raw matte of a caller's mask (mask_io.front_ref of
    mask_io.mask_ref).  `xmin`, `wx`, `ymin`, `wy`: the tables of `mask_io.tables`; `combine`: "replace", or "and" / "or" with
    the ramp `lo32, inv32, hard` (`matte.matte_params`) and `far` over the fp16 [H,W] `depth` plane, which "replace" does not
    read (it may be None)."""
    kinds = {torch.uint8: 0, torch.uint16: MASK_U16, torch.int16: MASK_U16, torch.float32: MASK_F32}      # (int16: the bits of uint16 samples)
    if src.dtype not in kinds:
        raise ValueError(f"mask_ingest: src: expected uint8, uint16 or float32 samples, got {src.dtype}")
    if src.numel() != Hm * Wm or not src.is_contiguous():
        raise ValueError(f"mask_ingest: src: expected a contiguous [{Hm},{Wm}] mask, got {tuple(src.shape)}")
    _fp32_plane("mask_ingest: out", out, H, W, flat=True)
    depth, lo32, inv32, hard, far = _ramp_input("mask_ingest", combine, MASK_COMBINE, depth, lo32, inv32, hard, far, H, W)
    _resample_tables("mask_ingest", xmin, wx, ymin, wy, H, W)
    flags = (kinds[src.dtype] | MASK_COMBINE[combine] | (MASK_INVERT if invert else 0) | (MASK_RAMP_HARD if hard else 0)
             | (MASK_RAMP_FAR if far else 0))
    return _record(_lib.OP_MASK_INGEST, (src, out, depth, xmin, wx, ymin, wy),
                   (Hm, Wm, H, W, nh, nw, top, left, wx.shape[1], wy.shape[1], flags), f=(lo32, inv32))


# ----------------------------------------------------------------------------- the matte key (matte_key.hip, matte_key.py)
MATTE_KEY_PLATE, MATTE_KEY_HARD, MATTE_KEY_INVERT, MATTE_KEY_AND, MATTE_KEY_OR, MATTE_KEY_RAMP_HARD, MATTE_KEY_RAMP_FAR = \
    1, 2, 4, 8, 16, 64, 128                                                                              # l2d.h L2D_MATTE_KEY_*
MATTE_KEY_MAX_R = 4
MATTE_KEY_GAIN = 512                              # l2d.h L2D_MATTE_KEY_GAIN: ops 59 and 61 key against the plate times the record p6
MATTE_KEY_GAIN_STATE = 1                          # l2d.h L2D_MATTE_KEY_GAIN_STATE: op 62 reads the uint16 state, not the uint8 plate
MATTE_KEY_GAIN_UNITY, MATTE_KEY_GAIN_BINS, MATTE_KEY_GAIN_BLOCK = 128, 512, 4096                         # l2d.h L2D_MATTE_KEY_GAIN_*
MATTE_KEY_COMBINE = {"replace": 0, "and": MATTE_KEY_AND, "or": MATTE_KEY_OR}


def _gain_record(name, gain, out):
    """the checks of a gain record p6 of ops 59 / 61: an int32 [8] tensor, 16-byte aligned, that the plane does not overlap"""
    if not torch.is_tensor(gain) or gain.dtype != torch.int32 or gain.numel() != 8 or not gain.is_contiguous() or gain.data_ptr() % 16:
        raise ValueError(f"{name}: gain: expected a contiguous, 16-byte aligned int32 [8] record (matte_key_gain writes it), got "
                         f"{_got(gain)}")
    if _overlap(out, gain):
        raise ValueError(f"{name}: the plane overlaps the gain record")


def matte_key(source, out, depth, key, *, H, W, r, L, lo2, inv, hard, combine="replace", invert=False, lo32=0.0, inv32=0.0,
              ramp_hard=False, far=False, gain=None):
    """fp16 [3,H,W] `source` -> fp32 [H,W] `out`: the raw matte of a key (mask_io.front_ref of matte_key.key_ref).  `key`: three
    bytes (a colour), or a planar uint8 [3,H,W] tensor (a plate); `r`: the window's radius; `L`: rint(256 luma); `lo2, inv,
    hard`: `matte_key.key_params`; `combine`: "replace", or "and" / "or" with the ramp `lo32, inv32, ramp_hard`
    (`matte.matte_params`) and `far` over the fp16 [H,W] `depth` plane, which "replace" does not read (it may be None).  `gain`: the
    int32 [8] record `matte_key_gain` writes -- the plate's bytes are multiplied by its gains first (a plate only)."""
    depth, plate, flags, colour, f = _key_fields(source, out, depth, key, H, W, r, L, lo2, inv, hard, combine, invert, lo32, inv32, ramp_hard, far)
    if gain is not None:
        if plate is None:
            raise ValueError(f"matte_key: gain with the colour key={key!r}: a gain corrects a plate")
        _gain_record("matte_key", gain, out)
        flags |= MATTE_KEY_GAIN
    return _record(_lib.OP_MATTE_KEY, (source, out, depth, plate), (H, W, r, flags, L, *colour), f=f,
                   at=None if gain is None else {6: gain})


def _key_fields(source, out, depth, key, H, W, r, L, lo2, inv, hard, combine, invert, lo32, inv32, ramp_hard, far):
    """what `matte_key` and `matte_key_adapt` share: every check of `matte_key` but the gain's -> (depth, plate, flags, colour,
    f) as they go into the record, the depth and the plate None where the record has none"""
    _fp16_frame("matte_key: source", source, H, W)
    _fp32_plane("matte_key: out", out, H, W, flat=True)
    if W % 8:
        raise ValueError(f"matte_key: W = {W} must be a multiple of 8")
    depth, lo32, inv32, ramp_hard, far = _ramp_input("matte_key", combine, MATTE_KEY_COMBINE, depth, lo32, inv32, ramp_hard, far, H, W)
    _int_in("matte_key: r", r, 0, MATTE_KEY_MAX_R, strict=True)
    _int_in("matte_key: L", L, 0, 256, strict=True)
    lo2, inv = float(lo2), float(inv)
    if not (np.isfinite(lo2) and lo2 >= 0.0 and np.isfinite(inv) and inv >= 0.0) or bool(hard) != (inv == 0.0):
        raise ValueError(f"matte_key: lo2={lo2!r} and inv={inv!r} must be finite and not negative, inv 0 exactly with hard={hard!r}")
    plate, colour = None, (0, 0, 0)
    if torch.is_tensor(key):
        plate = key
        _u8_planes("matte_key: key", plate, H, W, "tensor (a plate)", exact=True)
    else:
        try:
            colour = tuple(int(c) for c in key)
        except (TypeError, ValueError):
            colour = ()
        if len(colour) != 3 or any(isinstance(c, bool) or int(c) != c for c in key) or not all(0 <= c <= 255 for c in colour):
            raise ValueError(f"matte_key: key={key!r}: use three bytes (r, g, b), or a plate tensor")
    flags = ((MATTE_KEY_PLATE if plate is not None else 0) | (MATTE_KEY_HARD if hard else 0) | MATTE_KEY_COMBINE[combine]
             | (MATTE_KEY_INVERT if invert else 0) | (MATTE_KEY_RAMP_HARD if ramp_hard else 0) | (MATTE_KEY_RAMP_FAR if far else 0))
    return depth, plate, flags, colour, (lo2, inv, lo32, inv32)


MATTE_KEY_ADAPT_INIT = 256                        # l2d.h L2D_MATTE_KEY_ADAPT_INIT
MATTE_KEY_MAX_RATE = 32768                        # l2d.h L2D_MATTE_KEY_MAX_RATE: 65536 times a rate of 1 / 2
_STATE_DTYPES = (torch.uint16, torch.int16)       # (int16: the bits of uint16 words)


def _overlap(a, b) -> bool:
    """do the bytes of two tensors overlap (l2d.h px_overlap)?"""
    if a is None or b is None:
        return False
    x, y = a.data_ptr(), b.data_ptr()
    return x < y + b.numel() * b.element_size() and y < x + a.numel() * a.element_size()


def matte_key_adapt(source, out, depth, plate, state_in, state_out, *, H, W, r, L, lo2, inv, hard, a_bg, a_fg, combine="replace",
                    invert=False, lo32=0.0, inv32=0.0, ramp_hard=False, far=False, gain=None):
    """`matte_key` against a plate that follows drifting light (matte_key.key_adapt_ref): fp16 [3,H,W] `source` -> fp32 [H,W]
    `out`, and the next state.  The state is the plate in 8.8 fixed point, a planar uint16 [3,H,W] tensor (or int16: the same
    bits); `state_in` None: the state starts from `plate` (planar uint8 [3,H,W]; not read otherwise, and may be None then).
    `a_bg`, `a_fg`: `matte_key.adapt_params`; the rest as `matte_key`'s.  `state_out` is the next launch's `state_in`: it may
    overlap nothing the launch reads.  `gain`: as `matte_key`'s -- the key is formed against the state's bytes times the gains;
    the state's update is unchanged."""
    init = state_in is None
    if init and not torch.is_tensor(plate):
        raise ValueError(f"matte_key_adapt: plate={plate!r}: without state_in the state starts from a plate tensor")
    if not init and plate is not None and not torch.is_tensor(plate):
        raise ValueError(f"matte_key_adapt: plate={plate!r}: use a plate tensor or None")
    # (everything `matte_key` refuses; a record that reads a state is checked as one of a colour key)
    depth, plate, flags, _, f = _key_fields(source, out, depth, plate if init else (0, 0, 0), H, W, r, L, lo2, inv, hard, combine, invert, lo32,
                                            inv32, ramp_hard, far)
    for name, v in (("a_bg", a_bg), ("a_fg", a_fg)):
        _int_in("matte_key_adapt: " + name, v, 0, MATTE_KEY_MAX_RATE, strict=True, note=" (65536 times a rate in [0, 0.5])")
    for name, t in (("state_in", state_in), ("state_out", state_out)):
        if t is None and name == "state_in":
            continue
        if not torch.is_tensor(t) or t.dtype not in _STATE_DTYPES or tuple(t.shape) != (3, H, W) or not t.is_contiguous() \
                or t.data_ptr() % 16:
            raise ValueError(f"matte_key_adapt: {name}: expected a contiguous, 16-byte aligned planar uint16 [3,{H},{W}] tensor, got {_got(t)}")
    reads = (source, out, depth, plate, state_in)
    if any(_overlap(state_out, t) for t in reads) or _overlap(out, state_in):
        raise ValueError("matte_key_adapt: state_out overlaps state_in, the source, the plane, the depth plane or the plate (or the plane "
                         "state_in): the two records ping-pong")
    if gain is not None:
        _gain_record("matte_key_adapt", gain, out)
        if _overlap(state_out, gain):
            raise ValueError("matte_key_adapt: state_out overlaps the gain record")
    flags = (flags & ~MATTE_KEY_PLATE) | (MATTE_KEY_ADAPT_INIT if init else 0) | (MATTE_KEY_GAIN if gain is not None else 0)
    return _record(_lib.OP_MATTE_KEY_ADAPT, (source, out, depth, plate, state_in, state_out), (H, W, r, flags, L, a_bg, a_fg, 0), f=f,
                   at=None if gain is None else {6: gain})


_COUNT_DTYPES = (torch.uint32, torch.int32)       # (int32: the bits of uint32 counts)


def matte_key_gain_blocks(H: int, W: int) -> int:
    """the work-groups of `matte_key_gain_hist`: one per MATTE_KEY_GAIN_BLOCK pixels, the last one ragged"""
    return (int(H) * int(W) + MATTE_KEY_GAIN_BLOCK - 1) // MATTE_KEY_GAIN_BLOCK


def _gain_partials(name, partials, H, W) -> int:
    nblk = matte_key_gain_blocks(H, W)
    if not torch.is_tensor(partials) or partials.dtype not in _COUNT_DTYPES or tuple(partials.shape) != (nblk, 3, MATTE_KEY_GAIN_BINS) \
            or not partials.is_contiguous() or partials.data_ptr() % 16:
        raise ValueError(f"{name}: partials: expected a contiguous, 16-byte aligned uint32 [{nblk},3,{MATTE_KEY_GAIN_BINS}] tensor "
                         f"({nblk} blocks of {MATTE_KEY_GAIN_BLOCK} pixels over {H} x {W}), got {_got(partials)}")
    return nblk


def matte_key_gain_hist(source, plate, partials, *, H, W):
    """fp16 [3,H,W] `source` against `plate` -- planar uint8 [3,H,W] bytes, or the adaptive plate's planar uint16 [3,H,W] state
    (int16: the same bits), whose bytes are (s + 128) >> 8 -- -> uint32 [nblk,3,512] `partials`: every block's histogram of the
    per-pixel ratios (matte_key.gain_hist_ref is their sum).  Every entry is written on every launch."""
    if W % 8 or H < 1 or 3 * H * W >= 1 << 31:
        raise ValueError(f"matte_key_gain_hist: W = {W} must be a multiple of 8, H = {H} at least 1 and 3 H W below 2^31")
    _fp16_frame("matte_key_gain_hist: source", source, H, W, align=16)
    state = torch.is_tensor(plate) and plate.dtype in _STATE_DTYPES
    if not torch.is_tensor(plate) or (plate.dtype != torch.uint8 and not state) or tuple(plate.shape) != (3, H, W) \
            or not plate.is_contiguous() or plate.data_ptr() % (16 if state else 8):
        raise ValueError(f"matte_key_gain_hist: plate: expected a contiguous planar [3,{H},{W}] tensor, uint8 (8-byte aligned) or a uint16 "
                         f"state (16-byte aligned), got {_got(plate)}")
    nblk = _gain_partials("matte_key_gain_hist", partials, H, W)
    if _overlap(partials, source) or _overlap(partials, plate):
        raise ValueError("matte_key_gain_hist: the partials overlap the source or the plate")
    return _record(_lib.OP_MATTE_KEY_GAIN_HIST, (source, plate, partials), (H, W, MATTE_KEY_GAIN_STATE if state else 0, nblk))


def matte_key_gain(partials, record, *, H, W, lim, min_count):
    """uint32 [nblk,3,512] `partials` of an H x W frame -> the int32 [8] `record` {g_r, g_g, g_b, n_r, n_g, n_b, 0, 0}
    (matte_key.gain_of of their sum): `lim` = rint(128 limit) in 128..511, `min_count` in 0..H W (`matte_key.gain_params`)"""
    if W % 8 or H < 1 or 3 * H * W >= 1 << 31:
        raise ValueError(f"matte_key_gain: W = {W} must be a multiple of 8, H = {H} at least 1 and 3 H W below 2^31")
    nblk = _gain_partials("matte_key_gain", partials, H, W)
    if not torch.is_tensor(record) or record.dtype != torch.int32 or record.numel() != 8 or not record.is_contiguous() \
            or record.data_ptr() % 16:
        raise ValueError(f"matte_key_gain: record: expected a contiguous, 16-byte aligned int32 [8] tensor, got {_got(record)}")
    _int_in("matte_key_gain: lim", lim, MATTE_KEY_GAIN_UNITY, MATTE_KEY_GAIN_BINS - 1, strict=True)
    _int_in("matte_key_gain: min_count", min_count, 0, H * W, strict=True)
    if _overlap(record, partials):
        raise ValueError("matte_key_gain: the record overlaps the partials")
    return _record(_lib.OP_MATTE_KEY_GAIN, (partials, record), (H, W, nblk, lim, min_count))


def frame_planar_bytes(source, out, *, H, W):
    """fp16 [3,H,W] `source` -> planar uint8 [3,H,W] `out`: its egress bytes (steady.source_bytes) -- the plate capture"""
    _fp16_frame("frame_planar_bytes: source", source, H, W)
    _u8_planes("frame_planar_bytes: out", out, H, W, "tensor", exact=True)
    if W % 8:
        raise ValueError(f"frame_planar_bytes: W = {W} must be a multiple of 8")
    return _record(_lib.OP_FRAME_PLANAR_BYTES, (source, out), (H, W))

