"""CPU: the GEMM / conv envelope of gemm_cases.py before it is applied to the device (test_gpu_gemm_envelope.py).

  * every plain-torch restatement of the kernel's arithmetic stays within HALF the bound on every regime at every launch the GPU file
    makes -- half of what is left of error and bound once the form's single roundings (one fp16 rounding of the output, or two, of the
    pre-residual value and of the sum, for the staged epilogue with a residual; the fp32 bias / row-bias / residual adds, each of which
    can use all of its own term) are taken off both: the convention of DESIGN.md 5;
  * every mutant of the restatement leaves the bound on at least one planted element, and its whole-tensor rel-L2 on the iid inputs of
    test_igemm_linear / test_igemm_conv3x3 is printed next to the old 2e-3 (`MUTANT` lines: which of them the old test passed);
  * the planted operands keep every reference finite and every |out| below 6e4 (big rows below 3e4), `cancel` rows reach
    sum |x w| >= 1e3 |sum x w|, `tiny` rows reach the fp16 subnormal range;
  * staged() agrees with hand-worked cases of the kernel's `vec` condition.
No element is excluded on any regime; gemm_cases.RECORDED (printed only) is empty.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402

GROUPS = {"variants tile 1": lambda: [s for v, (_b, _n, ok) in gc.VARIANTS.items() if ok for s in gc.specs_variants(1, v)],
          "variants tile 2": lambda: [s for v in gc.VARIANTS for s in gc.specs_variants(2, v)],
          "splitk": lambda: gc.specs_splitk(1) + gc.specs_splitk(2), "epilogues": gc.specs_epilogues, "geglu": gc.specs_geglu,
          "geometry": gc.specs_geometry}


@pytest.mark.parametrize("group", list(GROUPS))
def test_restatements_use_at_most_half_the_bound(group):
    assert len(gc.RECORDED) <= 2
    agg, plain = {}, {}
    for s in GROUPS[group]():
        exact, bnd, rnd, rs = gc.expected(s)
        case = gc.case_of(s["key"])
        worst = gc.judge("igemm", s["what"], rs, exact, bnd, case, limit=0.5, rnd=rnd, chans=gc.out_chans(s), show_rnd=rnd)
        for k, v in worst.items():
            agg[k] = max(agg.get(k, 0.0), v)
        for k, v in gc.worst_per_regime(gc.ratios(rs, exact, bnd), case["rows"], gc.out_chans(s)).items():
            plain[k] = max(plain.get(k, 0.0), v)
    print(f"ALL restated {group}: " + "  ".join(f"{k} {v:.2f}" for k, v in plain.items()))
    print(f"ALL restated {group} (beyond the single roundings): " + "  ".join(f"{k} {v:.3f}" for k, v in agg.items()))


def test_restated_skinny_linear_uses_at_most_half_the_bound():
    for s in gc.specs_skinny():
        exact, bnd, rnd, rs = gc.expected_skinny(s)
        gc.judge("skinny_linear", s["what"], rs, exact, bnd, gc.case_of(s["key"]), limit=0.5, rnd=rnd, show_rnd=rnd)


@pytest.mark.parametrize("kernel,key,rowbias", gc.SIBLING_CASES)
def test_restated_siblings_use_at_most_half_the_bound(kernel, key, rowbias):
    exact, bnd, rnd, rs = gc.expected_sibling(kernel, key, rowbias)
    assert torch.isfinite(exact).all() and exact.abs().max() < 6e4
    gc.judge(kernel, f"{key[0]} {key[4]}+{key[5]}{' +rb' if rowbias else ''} +res", rs, exact, bnd, gc.case_of(key), limit=0.5, rnd=rnd, show_rnd=rnd)


def test_planted_operands_stay_finite_and_reach_their_regimes():
    seen_sub, seen_cancel = 0, 0
    for s in gc.all_specs():
        case = gc.case_of(s["key"])
        exact, bnd, _rnd, _rs = gc.expected(s)
        assert torch.isfinite(exact).all() and torch.isfinite(bnd).all() and torch.isfinite(case["y"]).all(), s["what"]
        assert exact.abs().max() < 6e4, (s["what"], exact.abs().max())
        rows = case["rows"]
        big = torch.tensor([r == "big" for r in rows])
        if big.any():
            assert exact[big].abs().max() < 3e4, (s["what"], exact[big].abs().max())
        if s["epi"] == 0 and not s["res"] and not s["rowbias"] and not case["conv"]:
            dense = torch.tensor([c in ("benign", "bigbias", "alt") for c in case["chans"]])
            canc = torch.tensor([r == "cancel" for r in rows])
            y, A = case["y"][canc][:, dense], case["A"][canc][:, dense]
            assert (A >= 1e3 * y.abs()).all(), (s["what"], (A / y.abs()).min())
            seen_cancel += int(canc.sum())
            tiny = torch.tensor([r == "tiny" for r in rows])
            alt = torch.tensor([c == "alt" for c in case["chans"]])
            seen_sub += int((exact[tiny][:, alt].abs() < 2.0 ** -14).sum())
    assert seen_cancel > 0 and seen_sub > 100, (seen_cancel, seen_sub)


# (mutant, spec on which it must leave the bound, kwargs of the iid case on which its rel-L2 is printed)
KEY_TAIL = gc.lin_key(C1=72, CinP=128, seed=4)
MUTANT_SPECS = {
    "wrap": gc.spec("conv", gc.conv_key(("wall", "benign", "hot"), seed=10)),
    "drop_stage": gc.spec("lin K72 in 128", KEY_TAIL),
    "double_stage": gc.spec("lin K320", gc.lin_key(C1=320), S=3, fused=True),
    "rowbias_first": gc.spec("lin rowbias", gc.lin_key(C1=128, seed=7), rowbias=True),
    "res_before_act": gc.spec("lin", gc.lin_key(C1=128, seed=7), epi=2, res=True),
    "bias_after_round": gc.spec("lin", gc.lin_key(C1=128, seed=7)),
    "ragged_shift": gc.spec("lin N70", gc.lin_key(C1=128, Nout=gc.NOUT_B, seed=7), ldo_pad=4),
    # (a staged launch computed the direct way cannot leave the wider staged bound: that direction is pinned by bit-equality on the device)
    "swap_round": gc.spec("lin", gc.lin_key(C1=128, seed=7), res=True, direct=True),
    "x2_at_c": gc.spec("conv concat", gc.conv_key(C1=8, C2=72, CinP=128, seed=3)),
}
OLD_TOL = 2e-3


def _iid(mutant):
    """the iid cases of the old tests on which the mutant applies: (name, case, restate kwargs)"""
    if mutant in ("wrap",):
        return [("conv 96->64 9x7", gc.iid_conv(2, 96, 64, 9, 7), {}), ("conv 320->320 32x32", gc.iid_conv(2, 320, 320, 32, 32), {})]
    if mutant == "x2_at_c":
        return [("conv 64+32->64 9x7 (concat)", gc.iid_conv(2, 96, 64, 9, 7, C2=32), {})]
    lin = [("linear 300x96x68", gc.iid_linear(300, 96, 68)), ("linear 154x768x1280", gc.iid_linear(154, 768, 1280)),
           ("linear 512x2560x320", gc.iid_linear(512, 2560, 320))]
    kw = {"double_stage": dict(S=3), "rowbias_first": dict(rowbias=True), "res_before_act": dict(epi=2, res=True),
          "swap_round": dict(res=True)}.get(mutant, {})
    if mutant == "ragged_shift":                     # (none of test_igemm_linear's shapes is ragged: the operands of test_igemm_splitk's)
        lin = [("linear 300x1024x70", gc.iid_linear(300, 1024, 70))]
    return [(n, c, kw) for n, c in lin]


@pytest.mark.parametrize("mutant", gc.MUTANTS)
def test_every_mutant_leaves_the_bound(mutant):
    s = MUTANT_SPECS[mutant]
    case = gc.case_of(s["key"])
    exact, bnd, _rnd, rs = gc.expected(s)
    assert gc.leaves_bound(rs, exact, bnd) == 0
    got = gc.restate(case, bk=s["bk"], S=s["S"], tile=s["tile"], is_staged=s["staged"], epi=s["epi"], bias=s["bias"], rowbias=s["rowbias"],
                     res=s["res"], mutant=mutant)
    n_bad = gc.leaves_bound(got, exact, bnd)
    ratio = gc.ratios(got, exact, bnd)
    worst = gc.worst_per_regime(ratio, case["rows"], gc.out_chans(s))
    print(f"MUTANT {mutant} on {s['what']}: {n_bad} of {ratio.numel()} planted elements leave the bound; regimes beyond it: " +
          ", ".join(k for k, v in worst.items() if not v <= 1.0))
    assert n_bad >= 1
    for name, icase, kw in _iid(mutant):
        y, _A = gc.reference(icase)
        flags = dict(epi=kw.get("epi", 0), bias=True, rowbias=kw.get("rowbias", False), res=kw.get("res", False))
        ref, _b, _r = gc.exact_and_bound(icase, y, _A, S=kw.get("S", 1), **flags)
        plain = gc.restate(icase, bk=64, S=kw.get("S", 1), **flags)
        mut = gc.restate(icase, bk=64, S=kw.get("S", 1), mutant=mutant, **flags)
        e0, e1 = gc.rel_l2(plain, ref), gc.rel_l2(mut, ref)
        print(f"MUTANT {mutant} iid {name}: rel-L2 {e1:.2e} (unmutated {e0:.2e}) -> the old {OLD_TOL:g} test "
              f"{'PASSES it' if e1 <= OLD_TOL else 'catches it'}")
        assert e0 <= OLD_TOL


@pytest.mark.parametrize("kw,want", [
    (dict(ldo=144, Nout=136), True),                                    # everything aligned: staged
    (dict(ldo=140, Nout=136), False),                                   # ldo % 8 = 4
    (dict(ldo=72, Nout=70), False),                                     # Nout % 8 = 6
    (dict(ldo=144, Nout=136, out_off=4), False),                        # the output pointer 8 bytes off
    (dict(ldo=144, Nout=136, out_off=8), True),                         # ... 16 bytes off: aligned again
    (dict(ldo=144, Nout=136, direct=True), False),                      # tile + 32
    (dict(ldo=144, Nout=136, splitk=4), False),                         # two-launch split-K: igemm_splitk_epilogue, never staged
    (dict(ldo=144, Nout=136, splitk=4, fused=True), True),              # fused split-K: the last block runs the staged epilogue
    (dict(ldo=140, Nout=136, splitk=4, fused=True), False),
    (dict(ldo=144, Nout=136, res=True, ldr=144), True),
    (dict(ldo=144, Nout=136, res=True, ldr=140), False),                # the residual pitch decides too
    (dict(ldo=144, Nout=136, res=True, ldr=144, res_off=4), False),
    (dict(ldo=88, Nout=160, epi=1), True),                              # GEGLU: the OUTPUT width 80 counts
    (dict(ldo=72, Nout=136, epi=1), False),                             # GEGLU with 68 output columns
    (dict(ldo=56, Nout=50, so=128 * 56, z=1), False),                   # swapped V^T with odd T
    (dict(ldo=56, Nout=56, so=100, z=1), False),                        # a batch stride that misaligns entry 1 ...
    (dict(ldo=56, Nout=56, so=100, z=0), True),                         # ... but not entry 0
])
def test_staged_restates_the_vec_condition(kw, want):
    assert gc.staged(**kw) is want
