"""Planted-regime inputs, fp64 references, per-element bounds and plain-torch emulations for the attention envelope tests
(test_attn_envelope_cpu.py, test_gpu_attn_envelope.py).

Every other attention test draws q, k, v iid N(0, 1): softmax over unit-Gaussian scores is nearly flat, so every data-dependent path
(the lazy reference raise of the ring kernel, the 2^(m_s - M) weights of the VAE merge, the pad-key mask of a ragged last tile, the
causal limit, the live-slot mask of the KV kernel) sits in its benign state, and one rel-L2 over the whole tensor hides a single wrong
row.  Here every query row follows its own regime (`REGIMES`, `KV_REGIMES`), the layout rotates per head and per sample, and every
output ELEMENT is held to a bound that follows from the arithmetic.  With u = 2^-11 (fp16 unit roundoff):

    D[q]       = max_k ( sum_i |q_i k_i| scale ) ( logit_rel + (d + 2) 2^-24 )                  (natural units; k over visible keys)
    bound[q,c] = u |out[q,c]|                                                                  (the fp16 output rounding)
               + ( 2 p_rel + (Tk + 2) 2^-24 ) sum_k p[q,k] |v[k,c]|                            (P rounding, fp32 sums of PV and of l)
               + expm1(2 D[q]) sum_k p[q,k] |v[k,c] - out[q,c]|                                (logit errors move mass between keys)

A logit error of at most D on every key changes every p_k by a factor within exp(+-2 D) (numerator and normaliser), and
sum_k p_k (f_k - 1) v_k = sum_k p_k (f_k - 1) (v_k - out) + out sum_k p_k (f_k - 1), whose second part the renormalisation removes: hence
the spread sum_k p |v - out|, which vanishes for a row that sees one key.  Masked keys have p = 0 exactly and enter no sum; Tk counts
the visible keys of the row.

The three terms are RELATIVE roundings, which fp16 delivers only in its normal range.  Below 2^-14 the format is a fixed grid of spacing
2^-24, so two absolute terms of half a spacing complete the bound (`SUBNORMAL` = 2^-25, about 3e-8):
    + 2^-25                                            an output element below 6.1e-5 cannot be stored to relative u
    + 2^-25 sum_k ( |v[k,c]| + |out[q,c]| )            where P is fp16 (p_rel = u): a probability below 2^-14 of the row's reference is
                                                       rounded on that grid (flushed below 2^-25); the reference never exceeds the
                                                       row's running maximum, so in units of the final l (>= 1) that is <= 2^-25 per
                                                       visible key, once in the numerator and once in the denominator
Both are far below the relative terms wherever an output is of ordinary size (at Tk = 576 and |v| about 1: 1.4e-5 against 1e-3); they
decide only elements whose reference value is itself about 1e-5 or smaller -- a `diag` row of the first CPU run sat on one key with
v = -3.4e-5 in that channel and missed the purely relative bound by 8e-8.

Switch settings, read from the kernels:

    kernel                                   logit_rel  p_rel   where
    flash variant 1 (flash_attn.hip)         0          u       raw fp32 scores, exp2(fma(s, c, -m c)); `pf[..] = (h16)pv` feeds the PV MFMA
    flash variants 2, 3, 4 (ring)            u          u       `qraw * sc`: Q pre-scaled by (h16)(log2 e / sqrt d) IN fp16; `(h16)pv`
    vae_attn (all split counts)              0          u       fp32 scores times fp32 c; `pf[j] = (h16)e`; the merge is fp32
    tattn_stream (register / chunked / ring) 0          2^-16   fp32 throughout; q + pe, k + pe, v + pe are fp16 adds and part of the
    tattn_warmup                             0          2^-16     operation: the reference rounds them the same way
    clip_attn                                0          2^-16   fp32 throughout

2^-16 covers `__expf` / `expf` / `v_exp_f32` on the fp32 paths; it is far below the output rounding.

Rounding points of the emulations that the short description "P is rounded to fp16 and used for both the sum and PV" does not cover
(the line of the kernel that performs each):
  * the flash kernels sum the ROUNDED P only where the denominator comes from the ones row of V^T (d % 16 != 0: d = 40); at d = 32, 80,
    160 they add the unrounded fp32 value (`if (!Cf::ONES) psum += pv;`), and so does vae_attn (`ps += e; pf[j] = (h16)e;`);
  * the ring kernel's raise is decided per WAVE (`__any(fmaxf(mx[0], mx[1]) > 8.0f)`, 32 rows in variants 2 / 4, 16 in variant 3; variant 1
    decides per 16-row subtile) and then moves every row of the wave to max(row maximum, reference): `delta = fmaxf(mx[qs], 0.f)`.

The KV reference (`kv_reference`, `warmup_reference`) is a plain fp64 restatement of the oracle's `stream_temporal_core` /
`warmup_temporal_core`; `round_pe=False` is the oracle's own operation (fp32 sums, pinned to <= 1e-5 on the CPU), `round_pe=True`, the
default, rounds q + pe, k + pe and v + pe to fp16 as the reference's fp16 module and every kernel do.

A note on the "masked slot fetched anyway" mutant: a kernel that merely LOADS a masked slot still multiplies it by p = 0, so finite
stale contents cannot show.  The mutant therefore drops the slot's mask altogether (fetched and scored); the stale rows are keys that are
strongly aligned with the pixel's query, so such a slot owns the row.
"""
import math

import torch

U = 2.0 ** -11
P32 = 2.0 ** -16
SUBNORMAL = 2.0 ** -25                               # half the spacing of fp16 below 2^-14
LOG2E = 1.4426950408889634
F32 = torch.float32

REGIMES = ("benign", "sink", "last", "edge63", "edge64", "neg", "pos", "ramp_up", "ramp_steep", "ramp_down", "tie", "huge", "diag")
CLIP_REGIMES = REGIMES + ("trap",)
KV_REGIMES = ("benign", "new", "sink", "last", "neg", "pos", "huge", "tie")
RECORDED = ()                                        # nothing had to move out of the asserted set (test_attn_envelope_cpu.py)

# reserved key channels of the shared-key kernels; the others are N(0, 1)
CH_K0, CH_LAST, CH_63, CH_64, CH_ALL, CH_RAMP, CH_TIE = range(7)
NRES = 7
AMP = 4.0                                            # exact in fp16

# (logit_rel, p_rel) per kernel
SWITCHES = {"flash1": (0.0, U), "flash_ring": (U, U), "vae": (0.0, U), "kv": (0.0, P32), "warmup": (0.0, P32), "clip": (0.0, P32)}

# ----------------------------------------------------------------------------- the shapes of the GPU file (the CPU file runs the same)
FLASH_B, FLASH_H, FLASH_TQ = 1, 2, 130               # two 64-row query blocks, the second ragged
FLASH_SHAPES = ((40, 77), (40, 200), (40, 576), (32, 200), (80, 200), (160, 130))       # (d, Tk)
VAE_B, VAE_D, VAE_LD = 2, 512, 1536 + 8
VAE_T = (1, 33, 100, 200, 512)
VAE_EXTRA_S = {200: (3,), 512: (16,)}                # 200 / 3: splits of 3, 3 and 1 tiles, the last one ragged with 8 keys
CLIP_B, CLIP_H, CLIP_D = 2, 2, 64
CLIP_T = (77, 80)
KV_N = 4
# (C, T, L, sink, variant): every variant number test_tattn_stream exercises, at the smallest shape it accepts
KV_CASES = ((64, 13, 16, 8, 0), (64, 13, 24, 8, 0), (320, 16, 16, 8, 2), (320, 20, 24, 8, 3), (320, 20, 16, 8, 6), (64, 13, 12, 4, 7),
            (320, 20, 16, 8, 7), (320, 16, 16, 8, 13), (320, 16, 40, 8, 13))
WARM_F, WARM_L = 8, 16
WARM_CASES = ((64, 20), (320, 16))                   # (C, T)


def vae_splits(T: int, schedule: int):
    """the split counts of one T: 1, 2, the schedule's own, one tile per split, and the extra ones; those the launcher's argument
    check rejects (S > tiles, S > 16, an empty last split) are left out"""
    nt = -(-T // 32)
    want = sorted({1, 2, schedule, nt} | set(VAE_EXTRA_S.get(T, ())))
    return [s for s in want if 1 <= s <= min(16, nt) and (s - 1) * (-(-nt // s)) < nt]


def regime_of(regimes, b: int, h: int, row: int) -> str:
    """the list rotated by one per head and by three per sample: no two (sample, head) pairs of the tests share a layout"""
    return regimes[(row + h + 3 * b) % len(regimes)]


def regime_rows(regimes, B: int, H: int, T: int):
    return [regime_of(regimes, b, h, r) for b in range(B) for h in range(H) for r in range(T)]


# ----------------------------------------------------------------------------- planted inputs, shared keys (flash, vae, clip)
def planted(B: int, H: int, Tq: int, Tk: int, d: int, seed: int, regimes=REGIMES):
    """fp16 q [B, H, Tq, d], k, v [B, H, Tk, d]: query row r of (b, h) follows regime_of(regimes, b, h, r).  Logit targets are in
    natural units at scale 1 / sqrt(d)."""
    assert d > NRES + 8
    gen = torch.Generator().manual_seed(seed)
    scale = d ** -0.5
    k = torch.randn(B, H, Tk, d, generator=gen, dtype=torch.float64)
    q = torch.randn(B, H, Tq, d, generator=gen, dtype=torch.float64)
    v = torch.randn(B, H, Tk, d, generator=gen, dtype=torch.float64)
    k[..., :NRES] = 0.0
    q[..., :NRES] = 0.0
    if Tk >= 4:                                      # two identical keys far apart
        k[:, :, Tk - 2] = k[:, :, 1]
        k[:, :, 1, CH_TIE] = k[:, :, Tk - 2, CH_TIE] = AMP
    k[:, :, 0, CH_K0] = AMP
    k[:, :, Tk - 1, CH_LAST] = AMP
    if Tk > 63:
        k[:, :, 63, CH_63] = AMP
    if Tk > 64:
        k[:, :, 64, CH_64] = AMP
    k[..., CH_ALL] = AMP
    k[..., CH_RAMP] = (torch.arange(Tk) // 64).double()
    k = k.to(torch.float16)
    coef = lambda nat: nat / (AMP * scale)
    ln2 = math.log(2.0)
    for b in range(B):
        for h in range(H):
            for r in range(Tq):
                name, row = regime_of(regimes, b, h, r), q[b, h, r]
                if name == "sink":
                    row[CH_K0] = coef(30.0)
                elif name == "last":
                    row[CH_LAST] = coef(30.0)
                elif name == "edge63":
                    row[CH_63] = coef(30.0)
                elif name == "edge64":
                    row[CH_64] = coef(30.0)
                elif name == "neg":
                    row[CH_ALL] = coef(-70.0)
                elif name == "pos":
                    row[CH_ALL] = coef(70.0)
                elif name == "ramp_up":
                    row[CH_RAMP] = 5.0 * ln2 / scale
                elif name == "ramp_steep":
                    row[CH_RAMP] = 20.0 * ln2 / scale
                elif name == "ramp_down":
                    row[CH_RAMP] = -20.0 * ln2 / scale
                elif name == "tie":
                    row[CH_TIE] = coef(30.0)
                elif name == "huge":
                    row *= 16.0
                elif name in ("diag", "trap"):
                    j = (7 * r) % Tk if name == "diag" else r + 1
                    if j < Tk:                       # (the last row has no key behind it: it stays benign)
                        row[NRES:] = k[b, h, j, NRES:].double() * ((25.0 if name == "diag" else 30.0) * d ** 0.5 / (d - NRES))
                else:
                    assert name == "benign", name
    v[..., 0] += 20.0                                # numerator and denominator must round the same P, or the bias shows here
    return q.to(torch.float16), k, v.to(torch.float16)


def causal_mask(T: int) -> torch.Tensor:
    return torch.ones(T, T, dtype=torch.bool).tril()


# ----------------------------------------------------------------------------- fp64 reference and the bound
def reference(q, k, v, scale: float, mask=None, bias=None):
    """fp64 softmax(q k^T scale [+ bias]) v of the fp16 (or already fp64) operands: (out, p); mask: bool, True = visible"""
    s = q.double() @ k.double().transpose(-1, -2) * scale
    if bias is not None:
        s = s + bias
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, -1)
    return p @ v.double(), p


def bound(q, k, v, out, p, scale: float, logit_rel: float, p_rel: float, visible=None, chunk: int = 32):
    """the per-element bound of the module docstring; visible: bool, broadcastable to p's shape (None: every key)"""
    d, tk = q.shape[-1], k.shape[-2]
    a = q.double().abs() @ k.double().abs().transpose(-1, -2) * scale
    nk = torch.full(p.shape[:-1], float(tk), dtype=torch.float64)
    if visible is not None:
        vis = visible.expand(p.shape)
        a = a.masked_fill(~vis, 0.0)
        nk = vis.sum(-1).double()
    dq = a.amax(-1) * (logit_rel + (d + 2) * 2.0 ** -24)
    vd = v.double()
    av = p @ vd.abs()
    spread = torch.empty_like(out)
    for q0 in range(0, p.shape[-2], chunk):
        pc, oc = p[..., q0:q0 + chunk, :], out[..., q0:q0 + chunk, :]
        spread[..., q0:q0 + chunk, :] = ((vd.unsqueeze(-3) - oc.unsqueeze(-2)).abs() * pc.unsqueeze(-1)).sum(-2)
    floor = torch.full_like(out, SUBNORMAL)
    if p_rel == U:                                   # fp16 P: every visible key once in the numerator and once in the denominator
        ksum = vd.abs().sum(-2, keepdim=True) if visible is None else (vis.double() @ vd.abs())
        floor = floor + SUBNORMAL * (ksum + nk.unsqueeze(-1) * out.abs())
    return (U * out.abs() + (2 * p_rel + (nk + 2) * 2.0 ** -24).unsqueeze(-1) * av + torch.expm1((2 * dq).clamp_max(80.0)).unsqueeze(-1) * spread
            + floor)


def rel_l2(got, ref) -> float:
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).norm() / ref.norm()).item()


def ratios(got, ref, bnd) -> torch.Tensor:
    """per query row: the worst |got - ref| / bound over its elements (non-finite output: inf)"""
    err = (got.double().cpu() - ref).abs()
    r = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = torch.where(torch.isfinite(got.double().cpu()), r, torch.full_like(r, float("inf")))
    return r.amax(-1)


def worst_per_regime(ratio: torch.Tensor, rows):
    worst = {}
    for x, name in zip(ratio.flatten().tolist(), rows):
        worst[name] = max(worst.get(name, 0.0), x)
    return worst


def output_rounding(ref) -> torch.Tensor:
    """the part of the bound that is the one fp16 rounding of the output"""
    return U * ref.abs() + SUBNORMAL


def judge(kernel: str, case: str, got, ref, bnd, rows, limit: float = 1.0, recorded=RECORDED, beyond_rounding: bool = False):
    """got / ref / bnd [..., rows, d], `rows`: the regime of every row in flat order.  Prints the worst |got - ref| / bound per regime,
    asserts finiteness everywhere and ratio <= limit in every regime that is not merely recorded.  Returns the worst ratios.
    beyond_rounding (the CPU file's half-the-bound test of the fp32 paths): the limit is applied to what is left of error and bound
    once the output rounding is taken off both, (|got - ref| - rnd)+ / (bound - rnd) with rnd = output_rounding(ref); the plain ratio must
    still be <= 1."""
    assert tuple(got.shape) == tuple(ref.shape) == tuple(bnd.shape), (got.shape, ref.shape, bnd.shape)
    ratio = ratios(got, ref, bnd)
    assert ratio.numel() == len(rows), (ratio.shape, len(rows))
    worst = worst_per_regime(ratio, rows)
    order = [r for r in dict.fromkeys(CLIP_REGIMES + KV_REGIMES) if r in worst]
    print(f"ENV {kernel} {case}: " + "  ".join(f"{r} {worst[r]:.2f}" for r in order))
    assert torch.isfinite(got.float()).all(), f"{kernel} {case}: non-finite output"
    if beyond_rounding:
        assert max(worst.values()) <= 1.0, (kernel, case, worst)
        rnd = output_rounding(ref)
        ratio = (((got.double().cpu() - ref).abs() - rnd).clamp_min(0.0) / (bnd - rnd)).amax(-1)
        worst = worst_per_regime(ratio, rows)
        print(f"    beyond the output rounding: " + "  ".join(f"{r} {worst[r]:.2f}" for r in order))
    bad = {r: x for r, x in worst.items() if r not in recorded and x > limit}
    if bad:
        flat = ratio.flatten()
        i = int(flat.argmax())
        raise AssertionError(f"{kernel} {case}: |got - ref| beyond {limit:g} x bound: " + ", ".join(f"{r} {x:.2f}" for r, x in bad.items()) +
                             f" (worst row: flat index {i}, regime {rows[i]})")
    return worst


def broken_regimes(got, ref, bnd, rows):
    """the regimes in which `got` leaves the bound (sensitivity tests)"""
    return sorted(r for r, x in worst_per_regime(ratios(got, ref, bnd), rows).items() if not x <= 1.0)


# ----------------------------------------------------------------------------- emulations of the documented arithmetic
def _f32(x: float) -> torch.Tensor:
    return torch.tensor(x, dtype=F32)


def emulate_flash(q, k, v, *, ring: bool, rows_per_wave: int = 32, mutant=None):
    """flash_attn_ring.hip (ring=True; rows_per_wave 32: variants 2 / 4, 16: variant 3) or flash_attn.hip (ring=False, decisions per
    16-row subtile): q [B, H, Tq, d], k, v [B, H, Tk, d] fp16 -> fp16 out.  Per 64-key tile: fp32 scores against the running reference
    (in log2 units), the reference fixed by tile 0 and raised only when a row of the wave exceeds it by 8, P = exp2 rounded to fp16 for
    the PV product, l from the rounded P where the ones row supplies it (d % 16 != 0) and from the fp32 value otherwise, fp32
    accumulation, fp16 output.  mutant: "pad" (the pad keys of a ragged last tile stay unmasked: K = 0, V = 0 there),
    "raise_l" (a raise rescales O but not l)."""
    assert mutant in (None, "pad", "raise_l")
    B, H, Tq, d = q.shape
    Tk = k.shape[2]
    ones = d % 16 != 0
    group = rows_per_wave if ring else 16
    c2e = torch.rsqrt(_f32(float(d))) * _f32(LOG2E)
    qs = (q.float() * c2e.half().float()).half().float() if ring else q.float()      # one fp16 multiply: the exact product, rounded once
    nt = -(-Tk // 64)
    kp = torch.zeros(B, H, nt * 64, d, dtype=F32)
    vp = torch.zeros(B, H, nt * 64, d, dtype=F32)
    kp[:, :, :Tk], vp[:, :, :Tk] = k.float(), v.float()
    o = torch.zeros(B, H, Tq, d, dtype=F32)
    l = torch.zeros(B, H, Tq, dtype=F32)
    mref = torch.zeros(B, H, Tq, dtype=F32) if ring else torch.full((B, H, Tq), -1.0e30, dtype=F32)   # ring: log2 units; else raw
    pad_rows = -Tq % group
    for t in range(nt):
        raw = qs @ kp[:, :, t * 64:(t + 1) * 64].transpose(-1, -2)
        s = raw - mref[..., None] if ring else raw
        if (t + 1) * 64 > Tk and mutant != "pad":
            s[..., Tk - t * 64:] = -3.0e38
        mx = s.amax(-1)
        over = (mx > 8.0) if ring else ((mx - mref) * c2e > 8.0)
        over = torch.nn.functional.pad(over.float(), (0, pad_rows)).view(B, H, -1, group).amax(-1).repeat_interleave(group, -1)[..., :Tq] > 0
        if ring:
            delta = mx if t == 0 else torch.where(over, mx.clamp_min(0.0), torch.zeros_like(mx))
            alpha = torch.exp2(-delta)
            mref = mref + delta
            s = s - delta[..., None]
        else:
            mnew = torch.where(over, torch.maximum(mref, mx), mref)
            alpha = torch.exp2((mref - mnew) * c2e)
            mref = mnew
            s = s * c2e + (-mref * c2e)[..., None]
        if mutant != "raise_l" or t == 0:
            l = l * alpha
        o = o * alpha[..., None]
        p = torch.exp2(s)
        ph = p.half().float()
        l = l + (ph if ones else p).sum(-1)
        o = o + ph @ vp[:, :, t * 64:(t + 1) * 64]
    return (o * (1.0 / l)[..., None]).half()


def emulate_vae(q, k, v, scale: float, S: int, mutant=None):
    """vae_attn.hip: q, k, v [B, T, 512] fp16 -> fp16 out.  S contiguous key splits of ceil(nt / S) 32-key tiles; per tile fp32 scores
    times c = scale log2(e), the eager running maximum, l from the fp32 exponentials, P rounded to fp16 for PV; S = 1 normalises at
    once, otherwise (O, m, l) per split are merged in split order with the weights 2^(m_s - M).  mutant: "pad" (pad keys of the
    ragged last tile unmasked), "merge_m" (a merge that ignores m_s)."""
    assert mutant in (None, "pad", "merge_m")
    B, T, d = q.shape
    nt = -(-T // 32)
    tps = -(-nt // S)
    c = _f32(scale) * _f32(LOG2E)
    kp = torch.zeros(B, nt * 32, d, dtype=F32)
    vp = torch.zeros(B, nt * 32, d, dtype=F32)
    kp[:, :T], vp[:, :T] = k.float(), v.float()
    qf = q.float()
    parts = []
    for sp in range(S):
        m = torch.full((B, T), -1.0e30, dtype=F32)
        l = torch.zeros(B, T, dtype=F32)
        o = torch.zeros(B, T, d, dtype=F32)
        for t in range(sp * tps, min(nt, (sp + 1) * tps)):
            s = (qf @ kp[:, t * 32:(t + 1) * 32].transpose(1, 2)) * c
            if (t + 1) * 32 > T and mutant != "pad":
                s[..., T - t * 32:] = float("-inf")
            mn = torch.maximum(m, s.amax(-1))
            alpha = torch.exp2(m - mn)
            m = mn
            e = torch.exp2(s - mn[..., None])
            l = l * alpha + e.sum(-1)
            o = o * alpha[..., None] + e.half().float() @ vp[:, t * 32:(t + 1) * 32]
        parts.append((o, m, l))
    if S == 1:
        o, m, l = parts[0]
        return (o * (1.0 / l)[..., None]).half()
    big = torch.stack([m for _, m, _ in parts]).amax(0)
    acc = torch.zeros(B, T, d, dtype=F32)
    lsum = torch.zeros(B, T, dtype=F32)
    for o, m, l in parts:
        w = torch.ones_like(m) if mutant == "merge_m" else torch.exp2(m - big)
        lsum = lsum + w * l
        acc = acc + w[..., None] * o
    return (acc * (1.0 / lsum)[..., None]).half()


def emulate_fp32(q, k, v, scale: float, bias=None, mask=None, normalise_p: bool = True):
    """the fp32 paths (tattn.hip, tattn_ring.hip: p * inv before PV; clip.hip: the sum divided at the end): fp32 scores, maximum,
    exp, sum, PV; fp16 output"""
    s = (q.float() @ k.float().transpose(-1, -2)) * _f32(scale)
    if bias is not None:
        s = s + bias.float()
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    e = torch.exp(s - s.amax(-1, keepdim=True))
    den = e.sum(-1, keepdim=True)
    if normalise_p:
        return ((e * (1.0 / den)) @ v.float()).half()
    return ((e @ v.float()) / den).half()


def emulate_clip(q, k, v, scale: float, causal: bool, mutant=None):
    """clip.hip clip_attn_kernel: keys 0 .. i visible to row i (mutant "causal2": 0 .. i + 1)"""
    assert mutant in (None, "causal2")
    T = q.shape[-2]
    mask = None
    if causal:
        mask = torch.ones(T, T, dtype=torch.bool).tril(1 if mutant == "causal2" else 0)
    return emulate_fp32(q, k, v, scale, mask=mask, normalise_p=False)


# ----------------------------------------------------------------------------- KV-cache stream attention
def _h(x):
    return x.to(torch.float16)


def kv_case(C: int, T: int, L: int, S: int, seed: int, N: int = KV_N, H: int = 8):
    """One launch of tattn_stream with N = 4 rows: bias rows all live / tail masked from S + 2 / a non-contiguous mask / everything
    masked except the update slot; every (row, pixel, head) follows KV_REGIMES[(t + h + 3 n) % 8], planted on its own slab.  Masked
    slots and the stale contents of the update slot hold keys strongly aligned with the pixel's query (100 natural units) and values of
    1000: the reference ignores them exactly."""
    assert N == 4 and S + 3 <= L
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    d = C // H
    scale = d ** -0.5
    tabs = [_h(0.5 * rn(L, C)) for _ in range(3)]
    pe_idx = torch.stack([torch.cat([torch.arange(S), S + torch.randperm(L - S, generator=gen)]) for _ in range(N)])
    upd = torch.tensor([L - 1, S + 1, S + 2, S])
    bias = torch.zeros(N, L)
    bias[1, S + 2:] = float("-inf")
    bias[2, 1::3] = float("-inf")
    bias[3, :] = float("-inf")
    for n in range(N):
        bias[n, upd[n]] = 0.0
    q, k_new, v_new = rn(N, T, C), rn(N, T, C), rn(N, T, C)
    ck, cv = rn(N, T, L, C), rn(N, T, L, C)
    rows = [[[regime_of(KV_REGIMES, n, h, t) for h in range(H)] for t in range(T)] for n in range(N)]
    for n in range(N):
        u = int(upd[n])
        live = [l for l in range(L) if bias[n, l] == 0]
        for t in range(T):
            for h in range(H):
                hs = slice(h * d, (h + 1) * d)
                name = rows[n][t][h]
                if name == "huge":
                    q[n, t, hs] *= 16.0
                qp = _h(_h(q[n, t, hs]).float() + tabs[0][pe_idx[n, u], hs].float()).double()       # the query the kernel forms
                unit = qp / (qp.pow(2).sum() * scale)                                              # a key with logit 1

                def put(l, vec):
                    if l == u:
                        k_new[n, t, hs] = vec
                    else:
                        ck[n, t, l, hs] = vec

                if name == "new":
                    put(u, 30.0 * unit)
                elif name == "sink":
                    put(0, 30.0 * unit)
                elif name == "last":
                    put(live[-1], 30.0 * unit)
                elif name == "tie":
                    put(live[0], 30.0 * unit)
                    put(live[-1], 30.0 * unit)
                elif name in ("neg", "pos"):
                    for l in range(L):
                        put(l, (70.0 if name == "pos" else -70.0) * unit + 0.3 * rn(d))
                for l in range(L):
                    if bias[n, l] != 0 or l == u:    # never to be read
                        ck[n, t, l, hs] = 100.0 * unit
                        cv[n, t, l, hs] = 1000.0
    for x in (v_new, cv):
        x[..., 0::d] += 20.0
    cache = _h(torch.stack([ck, cv], 1))             # [N, 2, T, L, C]
    qkv = _h(torch.cat([q, k_new, v_new], -1)).reshape(N * T, 3 * C).contiguous()
    flat_rows = [rows[n][t][h] for n in range(N) for t in range(T) for h in range(H)]
    return dict(C=C, T=T, L=L, S=S, N=N, H=H, d=d, scale=scale, qkv=qkv, cache=cache, tabs=tabs, pe_idx=pe_idx, upd=upd, bias=bias, rows=flat_rows)


def kv_cache_after(case):
    """slot update_idx[n] of row n rewritten with the pre-PE k / v, nothing else touched"""
    N, T, C = case["N"], case["T"], case["C"]
    x = case["qkv"].view(N, T, 3 * C)
    out = case["cache"].clone()
    for n in range(N):
        out[n, 0, :, int(case["upd"][n])] = x[n, :, C:2 * C]
        out[n, 1, :, int(case["upd"][n])] = x[n, :, 2 * C:]
    return out


def kv_operands(case, round_pe: bool = True, mutant=None):
    """(q', k', v', bias) as [N, T, H, 1, d], [N, T, H, L, d] x 2 (fp64 values) and [N, 1, 1, 1, L].  mutant: "fetch_masked" (a masked
    slot is fetched and scored), "slot+1" (the new row stands in for slot update_idx + 1; slot update_idx keeps its stale contents)"""
    assert mutant in (None, "fetch_masked", "slot+1")
    N, T, C, L, H, d = (case[x] for x in "NTCLHd")
    x = case["qkv"].view(N, T, 3 * C).double()
    q, kn, vn = x[..., :C], x[..., C:2 * C], x[..., 2 * C:]
    ck, cv = case["cache"][:, 0].double().clone(), case["cache"][:, 1].double().clone()
    tq, tk, tv = (t.double() for t in case["tabs"])
    for n in range(N):
        u = (int(case["upd"][n]) + (1 if mutant == "slot+1" else 0)) % L
        ck[n, :, u], cv[n, :, u] = kn[n], vn[n]
    qi = torch.stack([case["pe_idx"][n, case["upd"][n]] for n in range(N)])
    rnd = (lambda t: t.to(torch.float16).double()) if round_pe else (lambda t: t)
    qp = rnd(q + tq[qi][:, None])
    kp = rnd(ck + tk[case["pe_idx"]][:, None])
    vp = rnd(cv + tv[case["pe_idx"]][:, None])
    heads = lambda t: t.reshape(*t.shape[:-1], H, d).transpose(-2, -3)           # [..., L, C] -> [..., H, L, d]
    bias = case["bias"].double()
    if mutant == "fetch_masked":
        bias = torch.zeros_like(bias)
    return heads(qp[:, :, None]), heads(kp), heads(vp), bias[:, None, None, None, :]


def _kv_merge(o):
    """[N, T, H, 1, d] -> [N, T, C]"""
    return o.squeeze(-2).reshape(o.shape[0], o.shape[1], -1)


def kv_reference(case, round_pe: bool = True):
    """(out [N, T, H, 1, d], p, bound) in fp64"""
    qp, kp, vp, bias = kv_operands(case, round_pe)
    out, p = reference(qp, kp, vp, case["scale"], bias=bias)
    bnd = bound(qp, kp, vp, out, p, case["scale"], *SWITCHES["kv"], visible=torch.isfinite(bias))
    return out, p, bnd


def kv_emulate(case, mutant=None):
    qp, kp, vp, bias = kv_operands(case, True, mutant)
    return emulate_fp32(qp, kp, vp, case["scale"], bias=bias)


def kv_heads(out_flat, case):
    """kernel output [N * T, C] -> [N, T, H, 1, d]"""
    N, T, H, d = (case[x] for x in "NTHd")
    return out_flat.cpu().view(N, T, H, 1, d)


# ----------------------------------------------------------------------------- warm-up (F x F per pixel)
def warmup_case(C: int, T: int, seed: int, Fr: int = WARM_F, L: int = WARM_L, H: int = 8):
    """tattn_warmup: every (pixel, head) follows KV_REGIMES[(t + h) % 8] over its eight frames ("new": every frame aligned with its own
    key; sink / last: frame 0 / frame 7 dominant for all eight queries, which share a base direction there)"""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    d = C // H
    scale = d ** -0.5
    tabs = [_h(0.5 * rn(L, C)) for _ in range(3)]
    q, k, v = rn(Fr, T, C), rn(Fr, T, C), rn(Fr, T, C)
    rows = [[regime_of(KV_REGIMES, 0, h, t) for h in range(H)] for t in range(T)]
    for t in range(T):
        for h in range(H):
            hs = slice(h * d, (h + 1) * d)
            name = rows[t][h]
            if name == "huge":
                q[:, t, hs] *= 16.0
            elif name == "new":
                for f in range(Fr):
                    k[f, t, hs] = 30.0 * q[f, t, hs] / (q[f, t, hs].pow(2).sum() * scale)
            elif name != "benign":
                base = rn(d)
                q[:, t, hs] = base + 0.25 * rn(Fr, d)
                unit = base / (base.pow(2).sum() * scale)
                if name == "sink":
                    k[0, t, hs] = 30.0 * unit
                elif name == "last":
                    k[Fr - 1, t, hs] = 30.0 * unit
                elif name == "tie":
                    k[2, t, hs] = k[Fr - 3, t, hs] = 30.0 * unit
                else:
                    k[:, t, hs] = (70.0 if name == "pos" else -70.0) * unit + 0.3 * rn(Fr, d)
    v[..., 0::d] += 20.0
    qkv = _h(torch.cat([q, k, v], -1)).reshape(Fr * T, 3 * C).contiguous()
    flat_rows = [rows[t][h] for t in range(T) for h in range(H) for _ in range(Fr)]
    return dict(C=C, T=T, L=L, F=Fr, H=H, d=d, scale=scale, qkv=qkv, tabs=tabs, rows=flat_rows)


def warmup_operands(case, round_pe: bool = True):
    """q', k', v' [T, H, F, d] in fp64"""
    Fr, T, C, H, d = (case[x] for x in "FTCHd")
    x = case["qkv"].view(Fr, T, 3 * C).double()
    rnd = (lambda t: t.to(torch.float16).double()) if round_pe else (lambda t: t)
    ops = []
    for j in range(3):
        y = rnd(x[..., j * C:(j + 1) * C] + case["tabs"][j][:Fr].double()[:, None])       # [F, T, C]
        ops.append(y.view(Fr, T, H, d).permute(1, 2, 0, 3))
    return ops


def warmup_reference(case, round_pe: bool = True):
    qp, kp, vp = warmup_operands(case, round_pe)
    out, p = reference(qp, kp, vp, case["scale"])
    return out, p, bound(qp, kp, vp, out, p, case["scale"], *SWITCHES["warmup"])


def warmup_emulate(case):
    qp, kp, vp = warmup_operands(case)
    return emulate_fp32(qp, kp, vp, case["scale"])


def warmup_heads(out_flat, case):
    """kernel output [F * T, C] -> [T, H, F, d]"""
    Fr, T, H, d = (case[x] for x in "FTHd")
    return out_flat.cpu().view(Fr, T, H, d).permute(1, 2, 0, 3)


def warmup_row_after(case):
    """cache_row [2, T, L, C] after the launch, from zeros: slots 0 .. F - 1 hold the pre-PE k / v"""
    Fr, T, C, L = (case[x] for x in "FTCL")
    x = case["qkv"].view(Fr, T, 3 * C)
    row = torch.zeros(2, T, L, C, dtype=torch.float16)
    row[0, :, :Fr] = x[..., C:2 * C].transpose(0, 1)
    row[1, :, :Fr] = x[..., 2 * C:].transpose(0, 1)
    return row


# ----------------------------------------------------------------------------- the oracle's view of a KV / warm-up case
def oracle_tables(tabs, L: int, C: int):
    """(pe, state dict) with which the oracle's F.linear(pe[:L], W) reproduces the three fp16 tables exactly: pe = [I | 0]"""
    assert L <= C
    pe = torch.zeros(L, C)
    pe[:, :L] = torch.eye(L)
    sd = {}
    for name, t in zip("qkv", tabs):
        w = torch.zeros(C, C)
        w[:, :L] = t.float().t()
        sd[f"to_{name}.weight"] = w
    return pe, sd
