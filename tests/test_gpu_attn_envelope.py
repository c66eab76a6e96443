"""-m gpu: every softmax-attention implementation per output element on planted, non-Gaussian scores (helpers, regimes, the bound and its
derivation: attn_cases.py; the bound is first shown to hold, with half to spare, for plain-torch restatements of each kernel's arithmetic:
test_attn_envelope_cpu.py).

Every other attention test draws q, k, v iid N(0, 1) and judges one rel-L2 over the whole output.  Here every query row (for the KV-cache
kernels: every pixel and head) follows its own regime -- a dominant first / last / tile-boundary key, all logits near -70 or +70, logits
ramping by 5 or 20 log2 units per key tile, two identical keys, logits of several hundred, a diagonal -- the layout rotates per head and
per sample, one channel of v carries an offset of 20, and every ELEMENT of the output is held to attn_cases.bound against fp64 attention
on the same fp16 inputs:
  a. flash_attn variants 1 - 4 (ragged query block; one ragged key tile, four tiles with a ragged last one, nine full tiles);
  b. tattn_stream in every variant number test_tattn_stream uses, four bias rows (all live, tail masked, a non-contiguous mask,
     everything but the update slot masked), masked slots and the stale update slot holding keys aligned with the query; the cache after
     the launch bit-equal to "slot update_idx[n] rewritten, nothing else touched";
  c. tattn_warmup;
  d. vae_attn with 1, 2, the scheduled number, one tile per split and up to 16 key splits, a last split of one ragged tile included;
  e. clip_attn, causal and not, with a regime aligned to the first key a row may NOT see.
Outputs start as NaN; workspaces and the padding columns of V^T hold NaN.  Every case prints an `ENV` line: the worst
|error| / bound per regime.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import attn_cases as ac  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    from live2diff_amd import _lib, ops
    print("device:", _lib.device_name())
    return ops


_CACHE = {}


def shared(key, B, H, Tq, Tk, d, seed, sw, regimes=ac.REGIMES, mask=None):
    """(q, k, v, ref, bound) of one planted shape: computed once, shared by every test and never modified"""
    key = (key, sw)
    if key not in _CACHE:
        inp = ("inputs", B, H, Tq, Tk, d, seed, regimes, mask is None)
        if inp not in _CACHE:
            q, k, v = ac.planted(B, H, Tq, Tk, d, seed, regimes)
            _CACHE[inp] = (q, k, v) + ac.reference(q, k, v, d ** -0.5, mask=mask)
        q, k, v, ref, p = _CACHE[inp]
        _CACHE[key] = (q, k, v, ref, ac.bound(q, k, v, ref, p, d ** -0.5, *ac.SWITCHES[sw], visible=mask))
    return _CACHE[key]


def tokens(x):
    """[B, H, T, d] -> [B, T, H d]"""
    B, H, T, d = x.shape
    return x.transpose(1, 2).reshape(B, T, H * d).contiguous()


def heads(x, H):
    """[B, T, H d] -> [B, H, T, d]"""
    B, T, C = x.shape
    return x.view(B, T, H, C // H).transpose(1, 2)


# ----------------------------------------------------------------------------- a. flash attention
@pytest.mark.parametrize("d,Tk", ac.FLASH_SHAPES)
def test_flash_attn_per_element(L, d, Tk):
    B, H, Tq = ac.FLASH_B, ac.FLASH_H, ac.FLASH_TQ
    C = H * d
    rows = ac.regime_rows(ac.REGIMES, B, H, Tq)
    ldvt = (Tk + 7) // 8 * 8
    outs = {}
    for variant in (1, 2, 3, 4):
        q, k, v, ref, bnd = shared(("flash", d, Tk), B, H, Tq, Tk, d, d + Tk, "flash1" if variant == 1 else "flash_ring")
        vt = torch.full((B, C, ldvt), NAN, dtype=torch.float16)              # the padding columns hold NaN
        vt[:, :, :Tk] = tokens(v).transpose(1, 2)
        out = torch.full((B, Tq, C), NAN, dtype=torch.float16, device=DEV)
        L.run(L.flash_attn(tokens(q).to(DEV), tokens(k).to(DEV), vt.to(DEV), out, B=B, H=H, d=d, Tq=Tq, Tk=Tk, ldq=C, ldk=C, ldvt=ldvt,
                           ldo=C, sq=Tq * C, sk=Tk * C, svt=C * ldvt, so=Tq * C, variant=variant))
        torch.cuda.synchronize()
        outs[variant] = out.cpu()
        ac.judge(f"flash v{variant}", f"d{d} Tk{Tk}", heads(outs[variant], H), ref, bnd, rows)
    assert torch.equal(outs[4], outs[2])             # the pipelined loop reorders instructions, not arithmetic


# ----------------------------------------------------------------------------- b. KV-cache stream attention
def kv_shared(C, T, Lw, S):
    key = ("kv", C, T, Lw, S)
    if key not in _CACHE:
        case = ac.kv_case(C, T, Lw, S, seed=C + T + Lw)
        _CACHE[key] = (case,) + ac.kv_reference(case) + (ac.kv_cache_after(case),)
    return _CACHE[key]


@pytest.mark.parametrize("C,T,Lw,S,variant", ac.KV_CASES)
def test_tattn_stream_per_element(L, C, T, Lw, S, variant):
    case, ref, p, bnd, cache_after = kv_shared(C, T, Lw, S)
    N = case["N"]
    cache = case["cache"].clone().to(DEV)
    out = torch.full((N * T, C), NAN, dtype=torch.float16, device=DEV)
    tabs = [t.to(DEV) for t in case["tabs"]]
    L.run(L.tattn_stream(case["qkv"].to(DEV), cache, tabs[0], tabs[1], tabs[2], case["pe_idx"].to(DEV), case["upd"].to(DEV),
                         case["bias"].half().to(DEV), out, N=N, T=T, C=C, L=Lw, H=8, variant=variant))
    torch.cuda.synchronize()
    ac.judge(f"tattn_stream v{variant}", f"C{C} T{T} L{Lw}", ac.kv_heads(out, case), ref, bnd, case["rows"])
    # row 3 masks everything but the update slot: v_new + v_pe to fp16 rounding (one fp16 add, then p = 1 exactly)
    x = case["qkv"].view(N, T, 3 * C)
    want = (x[3, :, 2 * C:].float() + case["tabs"][2][case["pe_idx"][3, case["upd"][3]]].float()).half()
    assert torch.equal(out.cpu().view(N, T, C)[3], want), "a row that sees only its update slot must return v_new + v_pe"
    assert torch.equal(cache.cpu(), cache_after), "cache: slot update_idx[n] of row n rewritten with the pre-PE k / v, nothing else touched"


# ----------------------------------------------------------------------------- c. KV warm-up
@pytest.mark.parametrize("C,T", ac.WARM_CASES)
def test_tattn_warmup_per_element(L, C, T):
    case = ac.warmup_case(C, T, seed=C + T)
    ref, p, bnd = ac.warmup_reference(case)
    Fr, Lw = case["F"], case["L"]
    row = torch.zeros(2, T, Lw, C, dtype=torch.float16, device=DEV)
    out = torch.full((Fr * T, C), NAN, dtype=torch.float16, device=DEV)
    tabs = [t.to(DEV) for t in case["tabs"]]
    L.run(L.tattn_warmup(case["qkv"].to(DEV), row, tabs[0], tabs[1], tabs[2], out, F=Fr, T=T, C=C, L=Lw, H=8))
    torch.cuda.synchronize()
    ac.judge("tattn_warmup", f"C{C} T{T}", ac.warmup_heads(out, case), ref, bnd, case["rows"])
    assert torch.equal(row.cpu(), ac.warmup_row_after(case))


# ----------------------------------------------------------------------------- d. VAE attention
@pytest.mark.parametrize("T", ac.VAE_T)
def test_vae_attn_per_element_every_split_count(L, T):
    B, d, ld = ac.VAE_B, ac.VAE_D, ac.VAE_LD
    q, k, v, ref, bnd = shared(("vae", T), B, 1, T, T, d, T, "vae")
    rows = ac.regime_rows(ac.REGIMES, B, 1, T)
    qkv = torch.full((B * T, ld), NAN, dtype=torch.float16)                  # (the columns behind q | k | v are never read)
    for j, x in enumerate((q, k, v)):
        qkv[:, j * d:(j + 1) * d] = x[:, 0].reshape(B * T, d)
    qkv = qkv.to(DEV)
    splits = ac.vae_splits(T, L.vae_attn_schedule(B, T))
    assert 1 in splits and (T != 200 or 3 in splits) and (T != 512 or 16 in splits), splits
    for S in splits:
        n_img, n_ws = L.vae_attn_sizes(B, T, S)
        img = torch.full((n_img,), NAN, dtype=torch.float16, device=DEV)
        ws = torch.full((max(n_ws, 1),), NAN, dtype=torch.float32, device=DEV)
        out = torch.full((B * T, d), NAN, dtype=torch.float16, device=DEV)
        L.run(L.vae_attn(qkv, out, img, ws, B=B, T=T, ld=ld, ldo=d, S=S))
        torch.cuda.synchronize()
        ac.judge("vae_attn", f"T{T} S{S}", out.cpu().view(B, 1, T, d), ref, bnd, rows)


# ----------------------------------------------------------------------------- e. CLIP attention
@pytest.mark.parametrize("causal", [1, 0])
@pytest.mark.parametrize("T", ac.CLIP_T)
def test_clip_attn_per_element(L, T, causal):
    B, H, d = ac.CLIP_B, ac.CLIP_H, ac.CLIP_D
    C = H * d
    mask = ac.causal_mask(T) if causal else None
    q, k, v, ref, bnd = shared(("clip", T, causal), B, H, T, T, d, T, "clip", regimes=ac.CLIP_REGIMES, mask=mask)
    qkv = torch.cat([tokens(x) for x in (q, k, v)], -1).reshape(B * T, 3 * C).contiguous()
    out = torch.full((B * T, C), NAN, dtype=torch.float16, device=DEV)
    L.run(L.clip_attn(qkv.to(DEV), out, B=B, T=T, H=H, d=d, ldq=3 * C, ldo=C, scale=d ** -0.5, causal=bool(causal)))
    torch.cuda.synchronize()
    got = heads(out.cpu().view(B, T, C), H)
    ac.judge("clip_attn", f"T{T} causal{causal}", got, ref, bnd, ac.regime_rows(ac.CLIP_REGIMES, B, H, T))
    if causal:
        assert torch.equal(got[:, :, 0], v[:, :, 0]), "row 0 sees one key: its output is v_0"
