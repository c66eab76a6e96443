"""CPU: the fused-form envelope of fused_cases.py before it is applied to the device (test_gpu_fused_envelope.py).

  * the plain-torch restatement of every form stays within the bound on every element, and within HALF of what is left of error and
    bound once the single roundings are taken off both (gemm_cases' convention; here the single roundings include the fp16 rounding
    of every normalised operand and, behind the GroupNorm prologue, the dozen scalar roundings of its statistics);
  * the planted data reaches its regimes and stays finite: every |result| below 3e4, the GEGLU gate targets exact, const rows
    normalise to 0 and return h16(b') bit for bit;
  * every mutant of a restatement leaves the bound on at least one planted element;
  * every launch of the GPU file builds and validates in dry-run.
The fold's r100 rows are recorded only (fused_cases.RECORDED_FOLD); fused_cases.RECORDED is empty.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_cases as fc  # noqa: E402
import gemm_cases as gc  # noqa: E402


@pytest.fixture
def dry():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def _splits(scheds):
    return sorted({s[3] for s in scheds})


ROW_GROUPS = {"rowgemm LN + linear": fc.rowgemm_ln_cases, "rowgemm LN + GEGLU": fc.rowgemm_geglu_cases,
              "rowgemm GN + linear": fc.rowgemm_gn_cases, "rowgemm LN + q|k|V^T": fc.rowgemm_qkv_cases}


def _ws_groups():
    from live2diff_amd import ops
    g, q = fc.wsgemm_geglu_case(), fc.wsgemm_qkv_case()
    return fc.wsgemm_fold_cases() + [(g, fc.wsgemm_geglu_scheds(ops, g)), (q, fc.wsgemm_qkv_scheds(ops, q))]


def _all_expected():
    """(kernel, name, case, S) of every distinct reference the GPU file judges against"""
    out = [("rowgemm", name, case, 1) for name, cases in ROW_GROUPS.items() for case, _g in cases()]
    out += [("wsgemm", "fold", case, S) for case, scheds in _ws_groups() for S in _splits(scheds)]
    return out


def test_recorded_sets():
    assert fc.RECORDED == () and fc.RECORDED_FOLD == ("r100",)


@pytest.mark.parametrize("group", list(ROW_GROUPS))
def test_rowgemm_restatements_use_at_most_half_the_bound(group):
    for case, _geoms in ROW_GROUPS[group]():
        ex, rs = fc.expected(case)
        fc.judge("rowgemm", f"{group} K{case['K']} N{case['Nout']}{' +res' if case['res'] is not None else ''}", rs, ex, limit=0.5, half=True)


def test_wsgemm_fold_restatements_use_at_most_half_the_bound():
    for case, scheds in _ws_groups():
        for S in _splits(scheds):
            ex, rs = fc.expected(case, S)
            fc.judge("wsgemm", f"fold K{case['K']} N{case['Nout']} epi{case['epi']} S{S}", rs, ex, recorded=fc.RECORDED_FOLD, limit=0.5, half=True)


def test_planted_data_reaches_its_regimes_and_stays_finite():
    seen_const = seen_gate = 0
    for kernel, name, case, S in _all_expected():
        ex, rs = fc.expected(case, S)
        what = (kernel, name, case["key"])
        assert torch.isfinite(ex["exact"]).all() and torch.isfinite(ex["bnd"]).all() and (ex["bnd"] > 0).all(), what
        assert ex["exact"].abs().max() < 3e4, (what, float(ex["exact"].abs().max()))
        assert torch.isfinite(rs.float()).all(), what
        if case["pro"] == 1:
            c = fc.const_rows(case["rows"])
            assert c.any(), what
            assert float(ex["n"][c].abs().max()) == 0.0, what                               # a const row normalises to 0 ...
            if case["epi"] == 0:                                                                # ... and returns h16(b') (+ residual)
                want = case["fd"]["b"].half()[None].expand(int(c.sum()), -1)
                if case["res"] is not None:
                    want = (want.float() + case["res"][c].float()).half()
                assert torch.equal(rs[c], want), what
                fc.check_const_rows(kernel, name, rs, rs, case["rows"])
                seen_const += int(c.sum())
        if case["epi"] == 1:                                                                    # the planted gates are exact
            No = case["NoutO"]
            pre = ex["y"] + case["fd"]["b"].double()[None]
            for col, cname in enumerate(case["chans"]):
                if cname.startswith("g"):
                    t = float(cname[1:])
                    g = pre[:, No + col]
                    assert float((g - g[0]).abs().max()) == 0.0 and abs(float(g[0]) - t) < 0.05, (what, col, cname)
                    seen_gate += 1
            v = pre[:, :No]
            assert (v > 1).any() and (v < -1).any(), what
            assert {f"g{t:+.0f}" for t in fc.GATE_TARGETS} <= set(case["chans"]), what
    assert seen_const > 20 and seen_gate > 50, (seen_const, seen_gate)
    # every regime the issue names occurs, in every sample at another row
    x, rows = fc.plant_rows(3, 50, 320)
    assert set(rows) == set(fc.LN_ROWS) and rows[:50] != rows[50:100]
    x, rows = fc.plant_rows(3, 50, 320, fc.FOLD_ROWS)
    assert set(rows) == set(fc.FOLD_ROWS)


def test_geometry_rule_agrees_with_the_rowgemm_tests():
    import test_gpu_rowgemm as t
    for args in ((3,), (2,), (16,), (30,)):
        assert fc.rowgemm_geoms(*args) == t._geoms(*args) and fc.rowgemm_geoms(*args, mt4=True) == t._geoms(*args, mt4=True)
    assert fc.rowgemm_geoms(6, 2, mt_ok=False) == t._geoms(6, 2, mt_ok=False) and fc.rowgemm_geoms(30, 10) == t._geoms(30, 10)


# ----------------------------------------------------------------------------- mutants
def _mutant_setup(mutant):
    """(case, S, restate kwargs) on which the mutant must leave the bound"""
    if mutant in ("geglu_pair_swap", "bias_swap", "tanh_gelu"):
        return fc.ln_case(64, 512, geglu=True, seed=150), 1
    if mutant == "prev_row_mean":
        return fc.ln_case(320, 96), 1
    if mutant == "vt_shift":
        return fc.ln_case(64, 192, B=3, T=32, seed=170, ntr=64), 1
    if mutant == "colsum_unrounded":
        return fc.ln_case(1280, 128, ws=True, res=True, seed=310), 1
    if mutant == "slab0_norm":
        return fc.ln_case(320, 160, ws=True, res=True, seed=300), 2
    if mutant == "gn_neighbour":
        return fc.gn_case(3, 32, 320, 96), 1
    raise KeyError(mutant)


@pytest.mark.parametrize("mutant", [m for m in fc.MUTANTS if m != "ln_unrounded_h"])
def test_every_mutant_leaves_the_bound(mutant):
    case, S = _mutant_setup(mutant)
    ex, rs = fc.expected(case, S)
    keep = torch.tensor([r not in fc.RECORDED_FOLD for r in case["rows"]]) if case["pro"] == "fold" else torch.ones(case["M"], dtype=torch.bool)
    assert gc.leaves_bound(rs[keep], ex["exact"][keep], ex["bnd"][keep]) == 0
    if mutant == "vt_shift":
        B, T, ntr = case["B"], case["T"], case["ntr"]
        got = torch.cat([rs[:, :case["Nout"] - ntr], fc.vt_back(fc.vt_of(rs, B, T, ntr, mutant), B, T)], 1)
        assert torch.equal(torch.cat([rs[:, :case["Nout"] - ntr], fc.vt_back(fc.vt_of(rs, B, T, ntr), B, T)], 1), rs)
    else:
        got = fc.restate(case["x"], case["fd"], pro=case["pro"], eps=case["eps"], epi=case["epi"], res=case["res"], gn=case["gn"], S=S,
                         mutant=mutant)
    ratio = gc.ratios(got[keep], ex["exact"][keep], ex["bnd"][keep])
    n_bad = int((~(ratio <= 1.0)).sum())
    worst = gc.worst_per_regime(ratio, [r for r, k in zip(case["rows"], keep.tolist()) if k], case["chans"])
    print(f"MUTANT {mutant} on {case['key'][:4]}: {n_bad} of {ratio.numel()} planted elements leave the bound; regimes beyond it: " +
          ", ".join(k for k, v in worst.items() if not v <= 1.0) + f"; whole-tensor rel-L2 {gc.rel_l2(got[keep], ex['exact'][keep]):.2e}")
    assert n_bad >= 1


# ----------------------------------------------------------------------------- dry run of every launch of the GPU file
def test_every_rowgemm_launch_validates(dry):
    from live2diff_amd import ops
    n = 0
    for name, cases in ROW_GROUPS.items():
        for case, geoms in cases():
            d = fc.operands(case, "cpu")
            out, vt, ldo, ldt = fc.out_buffers(case, "cpu")
            for sched in geoms:
                for order in (0, 1):
                    ops.run(fc.rowgemm_op(ops, case, d, out, vt, ldo, ldt, sched, order))
                    n += 1
    assert n > 100


def test_every_wsgemm_launch_validates(dry):
    from live2diff_amd import ops
    for case, scheds in _ws_groups():
        d = fc.operands(case, "cpu")
        out, vt, ldo, ldt = fc.out_buffers(case, "cpu")
        for sched in scheds:
            ws, cnt = fc.wsgemm_bufs(ops, case, sched, "cpu")
            ops.run(fc.wsgemm_op(ops, case, d, out, vt, ldo, ldt, sched, ws, cnt))


# ----------------------------------------------------------------------------- rowchain: stage by stage
@pytest.mark.parametrize("B,T", fc.HEAD_SHAPES)
@pytest.mark.parametrize("kind", fc.HEAD_KINDS)
def test_restated_head_segments_use_at_most_half_the_bound(kind, B, T):
    case = fc.head_case(kind, B, T)
    ex1, h = fc.head_stage1(case)
    assert ex1["exact"].abs().max() < 3e4
    fc.judge("rowchain", f"head {kind} B{B} T{T} stage 1", h, ex1, limit=0.5, half=True)
    if not case["gnp"]:
        assert torch.equal(h[::3], case["resA"][::3])
        assert {r for r in case["rows2"]} >= set(fc.LN_ROWS)                               # stage 2 meets the planted rows
    ex2, out = fc.head_stage2(case, h)
    assert ex2["exact"].abs().max() < 3e4
    fc.judge("rowchain", f"head {kind} B{B} T{T} stage 2", out, ex2, limit=0.5, half=True)
    fc.check_const_rows("rowchain", kind, out, out, case["rows2"])


@pytest.mark.parametrize("B,T", fc.TAIL_SHAPES)
def test_restated_tail_stages_use_at_most_half_the_bound(B, T):
    case = fc.tail_case(B, T)
    prev, h2 = case["a"], None
    for i in range(1, 5):
        ex, rs = fc.tail_stage(case, i, prev, h2=h2)
        assert torch.isfinite(ex["exact"]).all() and ex["exact"].abs().max() < 3e4, (i, float(ex["exact"].abs().max()))
        fc.judge("rowchain", f"tail B{B} T{T} stage {i}", rs, ex, limit=0.5, half=True)
        h2 = rs if i == 1 else h2
        prev = rs
    assert torch.equal(h2[::3], case["res1"][::3])


def test_mutant_stage2_layernorm_on_the_unrounded_h_leaves_the_bound():
    case = fc.head_case("res_qkv", 3, 32)
    _ex1, h = fc.head_stage1(case)
    ex2, out = fc.head_stage2(case, h)
    assert gc.leaves_bound(out, ex2["exact"], ex2["bnd"]) == 0
    _ex, got = fc.head_stage2(case, h, mutant="ln_unrounded_h", hf=fc.head_h32(case))
    ratio = gc.ratios(got, ex2["exact"], ex2["bnd"])
    worst = gc.worst_per_regime(ratio, case["rows2"], case["fdB"]["chans"])
    print(f"MUTANT ln_unrounded_h: {int((~(ratio <= 1)).sum())} of {ratio.numel()} elements leave the bound; regimes beyond it: " +
          ", ".join(k for k, v in worst.items() if not v <= 1.0) + f"; whole-tensor rel-L2 {gc.rel_l2(got, ex2['exact']):.2e}")
    assert gc.leaves_bound(got, ex2["exact"], ex2["bnd"]) >= 1


def test_every_rowchain_launch_validates(dry):
    from live2diff_amd import ops
    C = fc.CHAIN_C
    for kind in fc.HEAD_KINDS:
        for B, T in fc.HEAD_SHAPES:
            case = fc.head_case(kind, B, T)
            ld, ldo, ldt = C + 8, case["ncol"] + 8, T + 8
            d = fc.head_operands(case, "cpu", ld)
            h, o = fc.nan_buf(case["M"], ld, "cpu"), fc.nan_buf(case["M"], ldo, "cpu")
            v = fc.nan_buf(B * C, ldt, "cpu") if case["trl"] else None
            for fused in (True, False):
                for op, keep in fc.head_ops(ops, case, d, h, o, v, ld=ld, ldo=ldo, ldt=ldt, fused=fused):
                    ops.run((op, keep))
    for B, T in fc.TAIL_SHAPES:
        case = fc.tail_case(B, T)
        ld, M = C + 8, case["M"]
        d = fc.tail_operands(case, "cpu", ld)
        bufs = [fc.nan_buf(M, ld, "cpu"), fc.nan_buf(M, 4 * C + 8, "cpu"), fc.nan_buf(M, ld, "cpu"), fc.nan_buf(M, ld, "cpu")]
        for op, keep in fc.tail_unfused_ops(ops, case, d, *bufs, ld):
            ops.run((op, keep))
        op, keep = fc.tail_chain_op(ops, case, d, bufs[3], ld)
        acc = torch.zeros(B, fc.G, 2, dtype=torch.int64)
        assert ops.gn_target(op, acc.data_ptr(), T=T, G=fc.G, cpg=C // fc.G, choff=0)
        ops.run((op, keep + (acc,)))


# ----------------------------------------------------------------------------- clip_linear
def test_restated_clip_linear_uses_at_most_half_the_bound():
    for c in fc.clip_cases():
        ex = fc.clip_expect(c)
        assert torch.isfinite(ex["exact"]).all() and ex["exact"].abs().max() < 3e4, c["name"]
        fc.judge("clip_linear", c["name"], fc.clip_restate(c), ex, limit=0.5, half=True)


def test_every_clip_linear_launch_validates(dry):
    from live2diff_amd import ops
    for c in fc.clip_cases():
        ld, ldo = c["K"] + 8, c["Nout"] + 8
        x = fc.guarded(c["x"], ld)
        out = fc.nan_buf(c["M"], ldo, "cpu", torch.float32 if c["epi"] == 2 else torch.float16)
        op, keep = fc.clip_op(ops, c, x, ops.pack_clip_linear(c["w"]), c["bias"], out, c["gamma"], c["beta"], ld, ldo)
        ops.run((op, keep + (x, out)))
