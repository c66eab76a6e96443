"""The per-element envelope that test_gpu_attn_envelope.py asserts on the device (attn_cases.bound) is one the documented arithmetic
stays inside: plain-torch emulations of every attention implementation's rounding points (attn_cases.emulate_*), on the planted regimes
and at every shape the GPU file uses, stay within HALF of the bound -- the half leaves the device its own summation order.  Each
emulation also has mutants, and every mutant must leave the bound in at least one regime; and the fp64 restatements of the KV
operations are pinned to the oracle's cores.

Worst |emulation - fp64| / bound per regime, over all shapes of each kernel (measured with this file):
                         benign sink last edge63 edge64 neg  pos  ramp_up ramp_steep ramp_down tie  huge diag trap new
    flash variant 1        0.26  0.00 0.00  0.00   0.00  0.26 0.28  0.30     0.34      0.26    0.32 0.32 0.29   -    -
    flash ring (2, 3, 4)   0.23  0.00 0.00  0.00   0.00  0.09 0.10  0.22     0.23      0.17    0.24 0.29 0.27   -    -
    vae_attn, every S      0.27  0.00 0.00  0.26   0.27  0.25 0.23  0.26     0.27      0.25    0.31 0.31 0.02   -    -
    tattn_stream           0.87  0.00 0.00   -      -    0.76 0.78   -        -         -      0.90 0.91  -     -   0.00
    tattn_warmup           0.89  0.32 0.06   -      -    0.84 0.82   -        -         -      0.92 0.90  -     -   0.91
    clip_attn causal       0.79  0.00 0.78  0.83   0.87  0.81 0.71  0.79     0.85      0.80    0.76 0.93 0.82  0.89  -
    clip_attn causal = 0   0.74  0.00 0.00  0.00   0.00  0.69 0.71  0.80     0.73      0.73    0.88 0.92 0.76  0.47  -
0.00: the row sees one key and returns its v exactly.  The kernels that round P to fp16 (flash, vae) stay at 0.34 or below: their bound
holds 2 u sum p |v| >= 2 u |out| beside the u |out| of the output rounding.  The fp32 kernels cannot stay within half of THEIR bound, and
no correct implementation could: it is little more than u |out|, and the one fp16 rounding of the output reaches that by itself (0.7 to
0.93 above), whatever the summation order.  Neither a rounding point is missing from the model nor is a regime too extreme -- benign rows
show it like all others -- so for these kernels the half is asserted where it can mean something: on what is left of error and bound
once the output rounding is taken off both (attn_cases.judge, beyond_rounding); there the restatements use at most 0.03.  The plain ratio
must still be <= 1, and the device is held to the plain, full bound.  Nothing moved to attn_cases.RECORDED.

Sensitivity.  Regimes in which each mutant leaves the bound, and the whole-tensor rel-L2 it reaches (the only thing the earlier tests
judge, against 2e-3):
    mutant                                          planted: rel-L2, regimes out of bound                       iid N(0, 1): rel-L2
    flash, pad keys of a ragged tile unmasked       0.29-0.30   benign neg ramp_down (ramp_up at one tile)      0.14-0.29
    flash, a raise rescales O but not l             0.55-0.59   nine regimes, ramp_steep and ramp_up among them 2.8e-4 - 5.8e-4: PASSES 2e-3
    vae, pad keys unmasked                          0.22-0.35   benign neg ramp_down (+ edges, ramps at T 33)   0.07-0.37
    vae, merge ignores m_s                          0.52-0.61   all but tie at S 2                              0.35-0.49
    clip, causal limit i + 2                        0.13        all but sink (and tie at T 77), trap among them 0.40-0.47
    kv, a masked slot scored                        121-262     all eight                                       (random stale rows: caught)
    kv, the new row in slot update_idx + 1          140-303     all eight                                       (caught by the cache comparison)
    one row of 130 off by 1 %                       6.4e-4 - 6.8e-4: PASSES 2e-3; 2.3 to 7.0 times the bound in that row's regime only
So the lazy raise is the path a whole-tensor rel-L2 on unit-Gaussian scores never reached (the reference is not raised after tile 0
there), and a single wrong row is what it cannot see at all.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import attn_cases as ac  # noqa: E402

HALF = 0.5
_CACHE = {}


def _say(capsys, text):
    with capsys.disabled():
        print("\n" + text, end="")


def shared(B, H, Tq, Tk, d, seed, regimes=ac.REGIMES, mask=None, key=None):
    """(q, k, v, ref, p) of one planted shape, computed once"""
    key = key or (B, H, Tq, Tk, d, seed, regimes)
    if key not in _CACHE:
        q, k, v = ac.planted(B, H, Tq, Tk, d, seed, regimes)
        ref, p = ac.reference(q, k, v, d ** -0.5, mask=mask)
        _CACHE[key] = (q, k, v, ref, p)
    return _CACHE[key]


def _judge_capture(capsys, *args, **kw):
    with capsys.disabled():
        print()
        return ac.judge(*args, **kw)


# ----------------------------------------------------------------------------- layout
def test_planted_layout_and_regimes():
    """every regime occurs in every (sample, head), no two (sample, head) pairs share a layout, and the planted rows are what the table
    says: the dominant key holds nearly all the mass, `neg` / `pos` leave the distribution of a benign row, the ramps order the tiles"""
    B, H, Tq, Tk, d = 2, 2, 130, 200, 40
    tabs = [[ac.regime_of(ac.REGIMES, b, h, r) for r in range(Tq)] for b in range(B) for h in range(H)]
    for t in tabs:
        assert all(t.count(r) >= 9 for r in ac.REGIMES)
    assert len({tuple(t) for t in tabs}) == B * H
    q, k, v, ref, p = shared(B, H, Tq, Tk, d, seed=1)
    assert torch.isfinite(ref).all()
    want = {"sink": 0, "last": Tk - 1, "edge63": 63, "edge64": 64}
    for b in range(B):
        for h in range(H):
            for r in range(Tq):
                name, row = tabs[b * H + h][r], p[b, h, r]
                if name in want:
                    assert row[want[name]] > 0.999, (name, float(row[want[name]]))
                elif name == "tie":
                    assert abs(row[1] - 0.5) < 1e-3 and abs(row[Tk - 2] - 0.5) < 1e-3
                elif name == "diag":
                    assert int(row.argmax()) == (7 * r) % Tk
                elif name == "ramp_steep":
                    assert row[192:].sum() > 0.9999
                elif name == "ramp_down":
                    assert row[:64].sum() > 0.9999
                elif name in ("neg", "pos", "benign"):
                    assert row.max() < 0.5
    s = q.double() @ k.double().transpose(-1, -2) * d ** -0.5
    rows = ac.regime_rows(ac.REGIMES, B, H, Tq)
    smax = ac.worst_per_regime(s.abs().amax(-1), rows)
    assert smax["neg"] > 60 and smax["pos"] > 60 and smax["huge"] > 40 and smax["benign"] < 8
    assert abs(float(ref[..., 0].mean()) - 20) < 0.5                     # the offset channel of v


# ----------------------------------------------------------------------------- emulation inside half the envelope
@pytest.mark.parametrize("d,Tk", ac.FLASH_SHAPES)
@pytest.mark.parametrize("impl", ["flash1", "ring32", "ring16"])
def test_flash_emulation_within_half_the_bound(impl, d, Tk, capsys):
    q, k, v, ref, p = shared(ac.FLASH_B, ac.FLASH_H, ac.FLASH_TQ, Tk, d, seed=d + Tk)
    sw = ac.SWITCHES["flash1" if impl == "flash1" else "flash_ring"]
    bnd = ac.bound(q, k, v, ref, p, d ** -0.5, *sw)
    out = ac.emulate_flash(q, k, v, ring=impl != "flash1", rows_per_wave=16 if impl == "ring16" else 32)
    _judge_capture(capsys, f"emu-{impl}", f"d{d} Tk{Tk}", out, ref, bnd, ac.regime_rows(ac.REGIMES, ac.FLASH_B, ac.FLASH_H, ac.FLASH_TQ), limit=HALF)


def vae_case(T):
    key = ("vae", T)
    if key not in _CACHE:
        q, k, v, ref, p = shared(ac.VAE_B, 1, T, T, ac.VAE_D, seed=T)
        bnd = ac.bound(q, k, v, ref, p, ac.VAE_D ** -0.5, *ac.SWITCHES["vae"])
        _CACHE[key] = tuple(t[:, 0] for t in (q, k, v, ref, bnd))
    return _CACHE[key]


@pytest.mark.parametrize("T", ac.VAE_T)
def test_vae_emulation_within_half_the_bound(T, capsys):
    from live2diff_amd import ops
    q, k, v, ref, bnd = vae_case(T)
    rows = ac.regime_rows(ac.REGIMES, ac.VAE_B, 1, T)
    splits = ac.vae_splits(T, ops.vae_attn_schedule(ac.VAE_B, T))
    assert 1 in splits and (T != 200 or 3 in splits) and (T != 512 or 16 in splits)
    for S in splits:
        out = ac.emulate_vae(q, k, v, ac.VAE_D ** -0.5, S)
        _judge_capture(capsys, "emu-vae", f"T{T} S{S}", out, ref, bnd, rows, limit=HALF)


@pytest.mark.parametrize("T", ac.CLIP_T)
@pytest.mark.parametrize("causal", [True, False])
def test_clip_emulation_within_half_the_bound(T, causal, capsys):
    q, k, v, ref, bnd, rows = clip_case(T, causal)
    out = ac.emulate_clip(q, k, v, ac.CLIP_D ** -0.5, causal)
    _judge_capture(capsys, "emu-clip", f"T{T} causal{int(causal)}", out, ref, bnd, rows, limit=HALF, beyond_rounding=True)
    if causal:                                       # row 0 sees one key: its output is v_0 to fp16 rounding (here: exactly)
        assert torch.equal(out[:, :, 0], v[:, :, 0])


def clip_case(T, causal):
    key = ("clip", T, causal)
    if key not in _CACHE:
        mask = ac.causal_mask(T) if causal else None
        q, k, v, ref, p = shared(ac.CLIP_B, ac.CLIP_H, T, T, ac.CLIP_D, seed=T, regimes=ac.CLIP_REGIMES, mask=mask, key=key + ("in",))
        bnd = ac.bound(q, k, v, ref, p, ac.CLIP_D ** -0.5, *ac.SWITCHES["clip"], visible=mask)
        _CACHE[key] = (q, k, v, ref, bnd, ac.regime_rows(ac.CLIP_REGIMES, ac.CLIP_B, ac.CLIP_H, T))
    return _CACHE[key]


def kv_case(C, T, L, S):
    key = ("kv", C, T, L, S)
    if key not in _CACHE:
        case = ac.kv_case(C, T, L, S, seed=C + T + L)
        _CACHE[key] = (case,) + ac.kv_reference(case)
    return _CACHE[key]


@pytest.mark.parametrize("C,T,L,S", sorted({c[:4] for c in ac.KV_CASES}))
def test_kv_emulation_within_half_the_bound(C, T, L, S, capsys):
    case, ref, p, bnd = kv_case(C, T, L, S)
    out = ac.kv_emulate(case)
    _judge_capture(capsys, "emu-kv", f"C{C} T{T} L{L}", out, ref, bnd, case["rows"], limit=HALF, beyond_rounding=True)
    # row 3 masks everything but the update slot: the output is v_new + v_pe to fp16 rounding, whatever the regime
    N, C_ = case["N"], case["C"]
    x = case["qkv"].view(N, T, 3 * C_)
    want = (x[3, :, 2 * C_:].float() + case["tabs"][2][case["pe_idx"][3, case["upd"][3]]].float()).half()
    assert torch.equal(ac._kv_merge(out)[3], want)
    assert float((ac._kv_merge(ref)[3] - want.double()).abs().max()) == 0


@pytest.mark.parametrize("C,T", ac.WARM_CASES)
def test_warmup_emulation_within_half_the_bound(C, T, capsys):
    case = ac.warmup_case(C, T, seed=C + T)
    ref, p, bnd = ac.warmup_reference(case)
    _judge_capture(capsys, "emu-warmup", f"C{C} T{T}", ac.warmup_emulate(case), ref, bnd, case["rows"], limit=HALF, beyond_rounding=True)


# ----------------------------------------------------------------------------- sensitivity
def _mutant(capsys, what, out, ref, bnd, rows, gauss=None):
    """gauss: the same mutant's whole-tensor rel-L2 on iid N(0, 1) inputs of the same shape -- what the earlier tests would have seen"""
    broken = ac.broken_regimes(out, ref, bnd, rows)
    g = "" if gauss is None else f" (on iid N(0, 1) inputs: {gauss:.2e}{', PASSES 2e-3' if gauss <= 2e-3 else ''})"
    _say(capsys, f"MUTANT {what}: rel-L2 {ac.rel_l2(out, ref):.2e}{g}, leaves the bound in: {' '.join(broken) or '-'}\n")
    assert broken, f"{what}: the envelope does not see this mutant"
    return broken


def _gauss(B, H, Tq, Tk, d, mask=None):
    key = ("gauss", B, H, Tq, Tk, d, mask is None)
    if key not in _CACHE:
        gen = torch.Generator().manual_seed(5)
        q, k, v = (torch.randn(B, H, t, d, generator=gen).half() for t in (Tq, Tk, Tk))
        _CACHE[key] = (q, k, v, ac.reference(q, k, v, d ** -0.5, mask=mask)[0])
    return _CACHE[key]


def test_one_wrong_row_hides_in_the_whole_tensor_norm_but_not_in_the_bound(capsys):
    """the reason for judging per element: one query row of 130 off by 1 % passes rel-L2 <= 2e-3 and leaves the bound by a factor of 2 to 7"""
    d, Tk = 40, 200
    q, k, v, ref, p = shared(ac.FLASH_B, ac.FLASH_H, ac.FLASH_TQ, Tk, d, seed=d + Tk)
    bnd = ac.bound(q, k, v, ref, p, d ** -0.5, *ac.SWITCHES["flash_ring"])
    rows = ac.regime_rows(ac.REGIMES, ac.FLASH_B, ac.FLASH_H, ac.FLASH_TQ)
    out = ac.emulate_flash(q, k, v, ring=True)
    assert not ac.broken_regimes(out, ref, bnd, rows) and ac.rel_l2(out, ref) <= 2e-3
    for r in (0, 7, 64, 129):
        bad = out.clone()
        bad[0, 1, r] = (bad[0, 1, r].float() * 1.01).half()
        worst = float(ac.ratios(bad, ref, bnd)[0, 1, r])
        _say(capsys, f"row {r} ({rows[ac.FLASH_TQ + r]}) off by 1 %: rel-L2 {ac.rel_l2(bad, ref):.2e}, worst |error| / bound {worst:.1f}\n")
        assert ac.rel_l2(bad, ref) <= 2e-3 and worst > 2.0 and ac.broken_regimes(bad, ref, bnd, rows) == [rows[ac.FLASH_TQ + r]]


@pytest.mark.parametrize("impl", ["flash1", "ring32"])
def test_flash_mutants_leave_the_bound(impl, capsys):
    rows = ac.regime_rows(ac.REGIMES, ac.FLASH_B, ac.FLASH_H, ac.FLASH_TQ)
    sw = ac.SWITCHES["flash1" if impl == "flash1" else "flash_ring"]
    for (d, Tk), mutant in (((40, 77), "pad"), ((40, 200), "pad"), ((32, 200), "raise_l"), ((40, 576), "raise_l")):
        q, k, v, ref, p = shared(ac.FLASH_B, ac.FLASH_H, ac.FLASH_TQ, Tk, d, seed=d + Tk)
        bnd = ac.bound(q, k, v, ref, p, d ** -0.5, *sw)
        out = ac.emulate_flash(q, k, v, ring=impl != "flash1", mutant=mutant)
        gq, gk, gv, gref = _gauss(ac.FLASH_B, ac.FLASH_H, ac.FLASH_TQ, Tk, d)
        gauss = ac.rel_l2(ac.emulate_flash(gq, gk, gv, ring=impl != "flash1", mutant=mutant), gref)
        broken = _mutant(capsys, f"{impl} d{d} Tk{Tk} {mutant}", out, ref, bnd, rows, gauss)
        if mutant == "pad":
            assert "neg" in broken                   # an unmasked pad key (logit 0) owns a row whose logits are all -70
        elif d % 16 == 0:
            assert "ramp_steep" in broken            # (with the ones row, l is an accumulator row of O and cannot be left behind)


def test_vae_mutants_leave_the_bound(capsys):
    for T, S, mutant, must in ((33, 1, "pad", "neg"), (200, 3, "pad", "neg"), (200, 3, "merge_m", "ramp_steep"), (100, 2, "merge_m", "sink"),
                               (512, 16, "merge_m", "last")):
        q, k, v, ref, bnd = vae_case(T)
        out = ac.emulate_vae(q, k, v, ac.VAE_D ** -0.5, S, mutant=mutant)
        gq, gk, gv, gref = (t[:, 0] for t in _gauss(ac.VAE_B, 1, T, T, ac.VAE_D))
        gauss = ac.rel_l2(ac.emulate_vae(gq, gk, gv, ac.VAE_D ** -0.5, S, mutant=mutant), gref)
        assert must in _mutant(capsys, f"vae T{T} S{S} {mutant}", out, ref, bnd, ac.regime_rows(ac.REGIMES, ac.VAE_B, 1, T), gauss)


def test_clip_mutant_leaves_the_bound(capsys):
    for T in ac.CLIP_T:
        q, k, v, ref, bnd, rows = clip_case(T, True)
        out = ac.emulate_clip(q, k, v, ac.CLIP_D ** -0.5, True, mutant="causal2")
        gq, gk, gv, gref = _gauss(ac.CLIP_B, ac.CLIP_H, T, T, ac.CLIP_D, mask=ac.causal_mask(T))
        gauss = ac.rel_l2(ac.emulate_clip(gq, gk, gv, ac.CLIP_D ** -0.5, True, mutant="causal2"), gref)
        assert "trap" in _mutant(capsys, f"clip T{T} causal limit i + 2", out, ref, bnd, rows, gauss)


def test_kv_mutants_leave_the_bound(capsys):
    for C, T, L, S in ((64, 13, 16, 8), (320, 16, 40, 8)):
        case, ref, p, bnd = kv_case(C, T, L, S)
        for mutant in ("fetch_masked", "slot+1"):
            _mutant(capsys, f"kv C{C} L{L} {mutant}", ac.kv_emulate(case, mutant=mutant), ref, bnd, case["rows"])


# ----------------------------------------------------------------------------- the references are the oracle's operations
@pytest.mark.parametrize("C,T,L,S", [(64, 13, 16, 8), (320, 16, 40, 8), (64, 13, 12, 4)])
def test_kv_reference_is_the_oracle_core(C, T, L, S):
    from live2diff_amd.config import tiny_config
    from oracle import unet_ref as O
    case, _, _, _ = kv_case(C, T, L, S)
    N = case["N"]
    pe, sd = ac.oracle_tables(case["tabs"], L, C)
    x = case["qkv"].view(N, T, 3 * C).float()
    cache = case["cache"].clone().float()
    out = O.stream_temporal_core(x[..., :C], x[..., C:2 * C], x[..., 2 * C:], O._W(sd), tiny_config(window_size=L, sink_size=S), cache,
                                 case["bias"], case["pe_idx"], case["upd"], pe)
    mine, _, _ = ac.kv_reference(case, round_pe=False)
    assert ac.rel_l2(ac._kv_merge(mine), out) <= 1e-5
    assert torch.equal(cache.half(), ac.kv_cache_after(case))
    # rounding q + pe, k + pe, v + pe to fp16 (every kernel does, as the reference's fp16 module) is a change of fp16 size, not another operation
    rounded, _, _ = ac.kv_reference(case)
    assert 1e-6 < ac.rel_l2(rounded, mine) < 2e-3


@pytest.mark.parametrize("C,T", ac.WARM_CASES)
def test_warmup_reference_is_the_oracle_core(C, T):
    from live2diff_amd.config import tiny_config
    from oracle import unet_ref as O
    case = ac.warmup_case(C, T, seed=C + T)
    Fr, L = case["F"], case["L"]
    pe, sd = ac.oracle_tables(case["tabs"], L, C)
    x = case["qkv"].view(Fr, T, 3 * C).float().transpose(0, 1)
    row = torch.zeros(2, T, L, C)
    out = O.warmup_temporal_core(x[..., :C], x[..., C:2 * C], x[..., 2 * C:], O._W(sd), tiny_config(window_size=L, sink_size=8), row, pe)
    mine, _, _ = ac.warmup_reference(case, round_pe=False)                   # [T, H, F, d]
    assert ac.rel_l2(mine.transpose(1, 2).reshape(T, Fr, C), out) <= 1e-5
    assert torch.equal(row.half(), ac.warmup_row_after(case))
