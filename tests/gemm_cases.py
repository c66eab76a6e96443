"""Planted operands, fp64 reference, per-element bound, plain-torch restatements and mutants for the GEMM / conv envelope tests
(test_gemm_envelope_cpu.py, test_gpu_gemm_envelope.py).

Every other GEMM / conv test draws iid N(0, 1) operands and judges one rel-L2 of 2e-3 over the whole tensor: one wrong element in
8192 x 640 moves that by 4e-4, a token row off by 10 % by 1e-3, a border pixel that reads its neighbour row is invisible.  Here every
token row and, independently, every output channel follows its own regime, the row layout rotates per sample, and every output ELEMENT
is held to a bound that follows from the arithmetic of the kernel.

Row regimes (linear forms; `ROW_REGIMES`): benign; hot (ONE non-zero input element, at k from `hot_ks`: 0, both sides of every BK
boundary 31|32, 63|64, 127|128, C1 - 1, the first channel of x2, the last real k); cancel (x = 128 at k = 1 and k = K - 2, whose weight
columns are exact negatives of each other, plus 2^-6 at K / 2: sum |x w| >= 1e3 |sum x w|, the halves in the first and the last K stage /
split); big (x 4096: |out| to 2e4); tiny (x 2^-8, which on the `alt` channels -- weights x 2^-8, no bias -- gives outputs in the fp16
subnormal range); offset (row mean 20).  Conv forms plant per SAMPLE (`CONV_REGIMES`): benign; hot (an impulse image: the output is the
flipped tap set of w); wall (the sample's border ring holds +-1e3: what a wrap across a row end or a sample end would reach); big;
tiny; offset.  Channel regimes (`CH_REGIMES`): benign; zero (weight row 0: out = epi(bias) exactly); hotw (one-hot weight row);
bigbias (|bias| about 1e3 over a product of about 1: an fp16 bias add is 0.5 absolute here; the residual there is about -bias); alt (alternating signs, x 2^-8, bias 0).
An element of a hot row (sample), or of a zero / hotw channel, is a single product: the fp32 accumulator holds it exactly whatever the
stage or split order, so for epi 0, 3, 4 the device must return the restatement's bits.

Reference: fp64 on the same fp16 operands, y = sum x w and A = sum |x w|.  With u = 2^-11, e = 2^-24:

    pre  = y + bias + rowbias
    E0   = (Kt + S + 2) e A                                fp16 x fp16 is exact in fp32; fp32 sums in any order over the Kt real terms
                                                           and the S slabs; + 2 as for the MFMA dot products of the attention bound
         + n_add e (|y| + |bias| + |rowbias|)              the bias / row-bias adds (n_add = how many are present)
    E1   = Lip E0 + C_act |pre|                            activation: Lip = 1 (none, ReLU), 1.1 (SiLU), 1.13 (GELU); C_act: the device
                                                           function's own error, MEASURED (`C_SILU`, `C_GELU`) x 2; |act(x)| <= |x|
    direct epilogue (igemm_epilogue(): residual added in fp32, one rounding):
    bound = (E1 + [e |a + r|]) (1 + u) + u |out| + 2^-25
    staged epilogue with a residual (igemm.hip `ot[...] = (h16)v`, then `v = v + resv` in fp16):
    bound = E1 (1 + 2 u) + u |a| + 2^-25 + u |a + r| + 2^-25
    GEGLU (v = value + bias, g = gate + bias, out = v gelu(g)):
    bound = (|gelu g| Ev + |v| Eg' + Ev Eg' + e |out|) (1 + u) + u |out| + 2^-25,   Eg' = 1.13 Eg + C_GELU |g|

a = act(pre), r the residual, out the exact result; epi 4 applies ReLU after the residual (Lipschitz 1, exact on fp16).  2^-25 is half
the fp16 spacing below 2^-14.  `SWITCHES[(kernel, form)]` = (double rounding with a residual?, fp32 output?).  `staged()` restates
the kernel's `vec` condition: which of the two roundings a launch gets.

Restatement (`restate`): plain torch, fp32: accumulation in BK-sized stages, S slabs [nk y / S, nk (y + 1) / S) summed in order 0 .. S - 1,
bias, then row bias (the 128 x 128 staged tile that lies in one sample adds bias + rowbias first: `b += rbp[n]` in load_bias), then the
activation, then the residual, the staged double rounding, and the row-bias source per row when a tile crosses a sample.

Elsewhere: the norm-folding prologues of rowgemm / wsgemm (pro != 0, the LayerNorm fold), their GEGLU and V^T forms, the rowchain
stages and clip_linear are held to the same kind of bound in fused_cases.py (test_fused_envelope_cpu.py, test_gpu_fused_envelope.py),
which widens this module's terms by the norm's own (`extra` of exact_and_bound); the GroupNorm-statistics epilogue has
norm_cases.check_acc.
"""
import math

import torch

U = 2.0 ** -11
E32 = 2.0 ** -24
SUBNORMAL = 2.0 ** -25
F32 = torch.float32
F64 = torch.float64

ROW_REGIMES = ("benign", "hot", "cancel", "big", "tiny", "offset")
CONV_REGIMES = ("benign", "hot", "wall", "big", "tiny", "offset")
CH_REGIMES = ("benign", "zero", "hotw", "bigbias", "alt")
RECORDED = ()                                        # no regime had to move out of the asserted set

# the device functions' own error as a multiple of |x| (|act(x)| <= |x| for both): measured once on an MI355X through existing epilogues
# with zero weight rows and a dense bias sweep over +-0.01 / 1 / 4 / 8 / 30 against fp64.  l2d_silu: 1.438e-7
# (2.41 x 2^-24), the fp32 value that skinny_linear stores, 4 M points; l2d_gelu: 1.767e-7 (2.96 x 2^-24), the excess of igemm epi 5's
# fp16 output over half an fp16 spacing of the exact value, 2.6 M points -- a lower estimate (the same method gives 1.005e-7 for SiLU,
# 0.7 of the direct figure).  Times 2, because only the sweep's grid was sampled.
SILU_MEASURED, GELU_MEASURED, ACT_MARGIN = 1.438e-7, 1.767e-7, 2.0
C_SILU, C_GELU = ACT_MARGIN * SILU_MEASURED, ACT_MARGIN * GELU_MEASURED
LIP = {0: 1.0, 2: 1.1, 3: 1.0, 4: 1.0, 5: 1.13}
C_ACT = {0: 0.0, 2: C_SILU, 3: 0.0, 4: 0.0, 5: C_GELU}

# (kernel, epilogue form) -> (the output is rounded to fp16 BEFORE the residual add as well as after it, the output is fp32)
SWITCHES = {("igemm", "staged"): (True, False), ("igemm", "direct"): (False, False), ("igemm", "splitk2"): (False, False),
            ("skinny", "f16"): (False, False), ("skinny", "f32"): (False, True),
            # the siblings always stage the fp16 tile in LDS and add the residual in fp16 (wsgemm.hip `os[...] = (h16)(acc ... + b2[e])`,
            # rowgemm.hip `(h16)(acc + bb[e])`, pconv.hip `o[r] = (h16)v[r]`, cconv.hip `(h16)(own + bv[e])`, then `v = v + resv`)
            ("wsgemm", "staged"): (True, False), ("rowgemm", "staged"): (True, False), ("pconv", "staged"): (True, False),
            ("cconv", "staged"): (True, False)}

# ----------------------------------------------------------------------------- the shapes of the GPU file (the CPU file runs the same)
B_, T_ = 3, 50                                       # M = 150: ragged in both tile sizes, a tile crosses samples
NOUT_A, NOUT_B = 136, 70                             # two / three channel tiles with a last one 8 wide; Nout % 4 == 2
IMG = (7, 6)
# pipeline variant -> (BK, ring stages, available for the 128 x 128 tile)
VARIANTS = {0: (32, 4, True), 1: (64, 3, True), 2: (64, 4, True), 3: (32, 6, True), 4: (32, 3, True), 5: (64, 2, True), 6: (128, 2, True),
            7: (128, 3, False), 8: (64, 6, False), 9: (64, 4, False), 10: (32, 2, True)}


def variant_cins(variant: int):
    """CinP values per variant so that the linear K loop runs 1, about NS - 1, NS and NS + 2 or more steps (CinP = 64 / 128 / 320;
    128 / 384 for the BK 128 shapes); the 3 x 3 forms multiply the step count by 9"""
    bk = VARIANTS[variant][0]
    return (128, 384) if bk == 128 else (64, 128, 320)


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def row_regime(b: int, t: int) -> str:
    return ROW_REGIMES[(t + 3 * b) % len(ROW_REGIMES)]


def hot_ks(K: int, C1: int):
    """the k of the hot rows: 0, both sides of every BK boundary, C1 - 1, the first channel of x2, the last real k"""
    return sorted({k for k in (0, 31, 32, 63, 64, 127, 128, C1 - 1, C1, K - 1) if 0 <= k < K})


# ----------------------------------------------------------------------------- planted operands
def _finish(case, gen, big_bias: float):
    """channel regimes on w [Nout, Kr] (Kr = taps * K real terms), bias, row bias, residual"""
    Nout, Kr, M, B = case["Nout"], case["w"].shape[1], case["M"], case["B"]
    w = case["w"]
    chans = [CH_REGIMES[n % len(CH_REGIMES)] for n in range(Nout)]
    bias = torch.randn(Nout, generator=gen, dtype=F64)
    scale = Kr ** -0.5
    hk = case["hot_kr"]
    k1, k2 = case["cancel_kr"]
    j = 0
    for n, name in enumerate(chans):
        if name == "zero":
            w[n] = 0.0
        elif name == "hotw":
            w[n] = 0.0
            w[n, hk[j % len(hk)]] = (0.5 + (j % 7) / 8.0) * (-1.0) ** j
            j += 1
        elif name == "bigbias":
            bias[n] = big_bias * (1.0 + 0.37 * math.sin(n)) * (-1.0) ** n
        elif name == "alt":
            w[n] = w[n].abs() * (1.0 - 2.0 * (torch.arange(Kr) % 2).double()) * 2.0 ** -8
            bias[n] = 0.0
        if name not in ("zero", "hotw"):             # the cancelling pair of columns: exact negatives, never small
            s = scale * (2.0 ** -8 if name == "alt" else 1.0)
            w[n, k1] = s * (0.5 + abs(float(w[n, k1])) / s) * (1.0 if n % 2 else -1.0)
            w[n, k2] = -w[n, k1]
    case["w"] = w.to(torch.float16)
    dense = torch.tensor([name not in ("zero", "hotw") for name in chans])
    case["w"][dense, k2] = -case["w"][dense, k1]     # (after the rounding: exact negatives)
    case["chans"] = chans
    case["bias"] = bias.to(F32)
    case["rowbias"] = torch.randn(B, Nout, generator=gen, dtype=F64).to(F32)
    res = torch.randn(M, Nout, generator=gen, dtype=F64)
    for m, name in enumerate(case["rows"]):
        if name == "tiny":
            res[m] *= 2.0 ** -16
    for n, name in enumerate(chans):                 # the residual cancels the big bias: the staged form's first rounding (u |a|, 0.5 here)
        if name == "bigbias":                        # against an output of about 1 -- the two epilogues differ by 500 x the direct bound
            res[:, n] += -bias[n]
    case["res"] = res.to(torch.float16)
    return case


def plant_linear(B: int, T: int, C1: int, C2: int, CinP: int, Nout: int, seed: int, big: float = 4096.0, big_bias: float = 1000.0):
    """x1 [M, C1], x2 [M, C2] fp16 (M = B T), w [Nout, K] fp16 (K = C1 + C2 <= CinP), bias / rowbias fp32, res fp16 [M, Nout]"""
    K, M = C1 + C2, B * T
    assert 16 <= K <= CinP and CinP % 64 == 0
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=gen, dtype=F64)
    w = torch.randn(Nout, K, generator=gen, dtype=F64) * K ** -0.5
    hk = hot_ks(K, C1)
    k1, k2, k3 = 1, K - 2, K // 2
    rows, j = [], 0
    for b in range(B):
        for t in range(T):
            name, m = row_regime(b, t), b * T + t
            rows.append(name)
            if name == "hot":
                x[m] = 0.0
                x[m, hk[j % len(hk)]] = (1.0 + (j % 8) / 8.0) * (-1.0) ** j
                j += 1
            elif name == "cancel":
                x[m] = 0.0
                x[m, k1] = x[m, k2] = 128.0
                x[m, k3] = 2.0 ** -6
            elif name == "big":
                x[m] *= big
            elif name == "tiny":
                x[m] *= 2.0 ** -8
            elif name == "offset":
                x[m] += 20.0
    x = x.to(torch.float16)
    case = dict(conv=False, B=B, T=T, M=M, C1=C1, C2=C2, K=K, CinP=CinP, taps=1, Nout=Nout, x1=x[:, :C1].contiguous(),
                x2=x[:, C1:].contiguous() if C2 else None, w=w, rows=rows, hot_kr=hk, cancel_kr=(k1, k2), rows_per_bias=T)
    return _finish(case, gen, big_bias)


def conv_out(n: int, stride: int, ups: int, pad_same: bool) -> int:
    n <<= ups
    if stride == 1:
        return n
    return n // 2 if pad_same else (n - 1) // 2 + 1


def plant_conv(regimes, H: int, W: int, C1: int, C2: int, CinP: int, Nout: int, seed: int, stride: int = 1, ups: int = 0,
               pad_same: bool = False):
    """x1 [B H W, C1], x2 [B H W, C2] fp16 channels-last, w [Nout, 9 K] with k = tap K + c; sample b follows regimes[b]"""
    B, K = len(regimes), C1 + C2
    assert 8 <= K <= CinP and CinP % 64 == 0 and not (pad_same and (stride != 2 or H % 2 or W % 2))
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, K, generator=gen, dtype=F64)
    w = torch.randn(Nout, 9 * K, generator=gen, dtype=F64) * (9 * K) ** -0.5
    hc = hot_ks(K, C1)
    for b, name in enumerate(regimes):
        if name == "hot":
            x[b] = 0.0
            x[b, (H // 2 + b) % H, (W - 1 - b) % W, hc[(seed + b) % len(hc)]] = 1.5
        elif name == "wall":
            ring = torch.zeros(H, W, dtype=torch.bool)
            ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
            x[b][ring] = 1000.0 * (1.0 - 2.0 * (torch.arange(K) % 2).double())
        elif name == "big":
            x[b] *= 2048.0
        elif name == "tiny":
            x[b] *= 2.0 ** -8
        elif name == "offset":
            x[b] += 20.0
        else:
            assert name == "benign", name
    x = x.to(torch.float16).view(B * H * W, K)
    Ho, Wo = conv_out(H, stride, ups, pad_same), conv_out(W, stride, ups, pad_same)
    rows = [regimes[b] for b in range(B) for _ in range(Ho * Wo)]
    hk = sorted({t * K + c for t in (0, 4, 8) for c in hc})
    case = dict(conv=True, B=B, Hin=H, Win=W, Hout=Ho, Wout=Wo, stride=stride, ups=ups, pad=0 if pad_same else 1, M=B * Ho * Wo, C1=C1,
                C2=C2, K=K, CinP=CinP, taps=9, Nout=Nout, x1=x[:, :C1].contiguous(), x2=x[:, C1:].contiguous() if C2 else None, w=w,
                rows=rows, hot_kr=hk, cancel_kr=(1, 9 * K - 2), rows_per_bias=Ho * Wo)
    return _finish(case, gen, 1000.0)


def weight_nchw(case) -> torch.Tensor:
    """[Nout, K, 3, 3] (what ops.pack_conv3x3 / pack_cconv take)"""
    return case["w"].view(case["Nout"], 3, 3, case["K"]).permute(0, 3, 1, 2).contiguous()


def packed_weight(case) -> torch.Tensor:
    """[Nout, taps * CinP] fp16, k = tap * CinP + c, zero padded: the layout of ops.pack_linear / pack_conv3x3"""
    Nout, taps, K, CinP = case["Nout"], case["taps"], case["K"], case["CinP"]
    wp = torch.zeros(Nout, taps, CinP, dtype=torch.float16)
    wp[:, :, :K] = case["w"].view(Nout, taps, K)
    return wp.view(Nout, taps * CinP)


def single_product(case) -> torch.Tensor:
    """bool [M, Nout]: the elements whose sum has at most one non-zero product"""
    r = torch.tensor([name == "hot" for name in case["rows"]])
    c = torch.tensor([name in ("zero", "hotw") for name in case["chans"]])
    return r[:, None] | c[None, :]


# ----------------------------------------------------------------------------- the operand matrix
def gather(case, mutant=None) -> torch.Tensor:
    """[M, taps, K] fp64: what the GEMM contracts with w.  mutant: "wrap" (a border tap is taken from the wrapped neighbour -- the flat
    pixel index without the bounds test -- instead of zero), "x2_at_c" (x2 read at channel c instead of c - C1: into the NaN gap of
    its rows)"""
    C1, C2, K = case["C1"], case["C2"], case["K"]
    x2 = case["x2"]
    if mutant == "x2_at_c":
        assert C2
        ext = torch.full((x2.shape[0], K + C2), float("nan"), dtype=torch.float16)
        ext[:, :C2] = x2
        x2 = ext[:, C1:C1 + C2]
    xc = (torch.cat([case["x1"], x2], 1) if C2 else case["x1"]).double()
    if not case["conv"]:
        return xc[:, None, :]
    B, H, W, Ho, Wo, st, ups, pad = (case[k] for k in ("B", "Hin", "Win", "Hout", "Wout", "stride", "ups", "pad"))
    m = torch.arange(case["M"])
    b, oy, ox = m // (Ho * Wo), (m % (Ho * Wo)) // Wo, m % Wo
    t = torch.arange(9)
    iy = oy[:, None] * st + (t // 3)[None] - pad
    ix = ox[:, None] * st + (t % 3)[None] - pad
    ok = (iy >= 0) & (ix >= 0) & (iy < (H << ups)) & (ix < (W << ups))
    pix = (b[:, None] * H + (iy >> ups)) * W + (ix >> ups)
    X = xc[pix.clamp(0, B * H * W - 1)] * ok[..., None]
    if mutant == "wrap":
        assert ups == 0
        inb = (pix >= 0) & (pix < B * H * W) & ~ok
        X = torch.where(inb[..., None], xc[pix.clamp(0, B * H * W - 1)], X)
    return X


def reference(case):
    """fp64 (y, A) [M, Nout]: y = sum x w, A = sum |x w|"""
    X = gather(case).reshape(case["M"], -1)
    w = case["w"].double()
    return X @ w.t(), X.abs() @ w.abs().t()


def act64(x, epi):
    if epi == 2:
        return x / (1.0 + torch.exp(-x))
    if epi == 3:
        return x.clamp_min(0.0)
    if epi == 5:
        return 0.5 * x * torch.erfc(-x / math.sqrt(2.0))
    return x


def exact_and_bound(case, y, A, *, epi=0, bias=True, rowbias=False, res=False, S=1, form=("igemm", "direct"), extra=None):
    """(exact result, bound, the single-rounding part of the bound) fp64 [M, NoutO], per the module docstring.  The third value is what
    the form's SINGLE roundings contribute -- the fp16 store(s) and the fp32 bias / row-bias / residual adds, each of which may use all of
    its term whatever the order of anything else: the CPU file's half-the-bound test applies to what is left beyond it, the
    accumulation and activation terms, whose order a restatement cannot know.  extra (fused_cases.py): what a norm in front of the GEMM
    adds to the error of the pre-activation value, [M, Nout]."""
    double_round, out_f32 = SWITCHES[form]
    M, Nout = case["M"], case["Nout"]
    b = case["bias"].double()[None].expand(M, Nout) if bias else torch.zeros(M, Nout, dtype=F64)
    rb = torch.zeros(M, Nout, dtype=F64)
    if rowbias:
        rb = case["rowbias"].double()[torch.arange(M) // case["rows_per_bias"]]
    pre = y + b + rb
    adds = (int(bias) + int(rowbias)) * E32 * (y.abs() + b.abs() + rb.abs())
    e0 = (case["taps"] * case["K"] + S + 2) * E32 * A + adds
    if extra is not None:
        e0 = e0 + extra
    if epi == 1:
        No = Nout // 2
        v, g, ev, eg = pre[:, :No], pre[:, No:], e0[:, :No], e0[:, No:]
        gl = act64(g, 5)
        egl = LIP[5] * eg + C_GELU * g.abs()
        out = v * gl
        rnd = U * out.abs() + SUBNORMAL
        single = gl.abs() * adds[:, :No] + v.abs() * LIP[5] * adds[:, No:] + E32 * out.abs()
        return out, (gl.abs() * ev + v.abs() * egl + ev * egl + E32 * out.abs()) * (1 + U) + rnd, rnd + single
    a = act64(pre, epi)
    e1 = LIP[epi] * e0 + C_ACT[epi] * pre.abs()
    r = case["res"].double() if res else torch.zeros_like(a)
    pre_relu = a + r
    out = pre_relu.clamp_min(0.0) if epi == 4 else pre_relu
    if out_f32:
        return out, e1 + E32 * out.abs(), LIP[epi] * adds + E32 * out.abs()
    if res and double_round:
        rnd = U * a.abs() + SUBNORMAL + U * pre_relu.abs() + SUBNORMAL
        return out, e1 * (1 + 2 * U) + rnd, rnd + LIP[epi] * adds
    rnd = U * out.abs() + SUBNORMAL
    add_r = E32 * pre_relu.abs() if res else 0.0
    return out, (e1 + add_r) * (1 + U) + rnd, rnd + LIP[epi] * adds + add_r


def staged(*, ldo: int, Nout: int, epi: int = 0, out_off: int = 0, splitk: int = 1, fused: bool = False, direct: bool = False,
           res: bool = False, ldr: int = 0, res_off: int = 0, so: int = 0, sres: int = 0, z: int = 0) -> bool:
    """igemm.hip `vec`: does batch entry z of this launch take the LDS-staged epilogue?  Offsets and strides in elements from 16-byte
    aligned allocations.  The two-launch split-K reduction always runs igemm_epilogue() (direct)."""
    nout_o = Nout // 2 if epi == 1 else Nout
    if direct or (splitk > 1 and not fused):
        return False
    if (ldo | nout_o) & 7 or (out_off + z * so) % 8:
        return False
    return not res or (ldr % 8 == 0 and (res_off + z * sres) % 8 == 0)


# ----------------------------------------------------------------------------- restatement and mutants
MUTANTS = ("wrap", "drop_stage", "double_stage", "rowbias_first", "res_before_act", "bias_after_round", "ragged_shift", "swap_round",
           "x2_at_c")


def split_ranges(nk: int, S: int):
    return [(nk * y // S, nk * (y + 1) // S) for y in range(S)]


def restate(case, *, bk: int = 64, S: int = 1, tile: int = 2, is_staged: bool = False, epi: int = 0, bias: bool = True,
            rowbias: bool = False, res: bool = False, mutant=None, out_f32: bool = False, rb_first: bool = False) -> torch.Tensor:
    """the kernel's arithmetic in plain fp32 torch -> fp16 [M, NoutO] (module docstring).  tile: 1 = 128 x 128, 2 = 64 x 64.
    rb_first: acc + (bias + rowbias) everywhere (the sibling kernels: `bv += rb` before the accumulator is touched)."""
    assert mutant is None or mutant in MUTANTS
    M, Nout, taps, K, CinP = case["M"], case["Nout"], case["taps"], case["K"], case["CinP"]
    X = torch.zeros(M, taps, CinP, dtype=F32)
    X[:, :, :K] = gather(case, mutant if mutant in ("wrap", "x2_at_c") else None).float()
    X = X.view(M, taps * CinP)
    Wp = packed_weight(case).float()
    Kp = taps * CinP
    assert Kp % bk == 0
    acc = None
    for y, (kb, ke) in enumerate(split_ranges(Kp // bk, S)):
        if y == 0 and mutant == "drop_stage" and ke > kb:
            ke -= 1
        if y == 0 and mutant == "double_stage":
            assert S > 1
            ke += 1
        part = torch.zeros(M, Nout, dtype=F32)
        for s in range(kb, ke):
            part = part + X[:, s * bk:(s + 1) * bk] @ Wp[:, s * bk:(s + 1) * bk].t()
        acc = part if acc is None else acc + part
    tm = 128 if tile == 1 else 64
    rpb = case["rows_per_bias"]
    m = torch.arange(M)
    b = case["bias"][None] if bias else None
    if mutant == "bias_after_round":
        acc = (acc.half() + case["bias"].half()[None]).float() if bias else acc
        b = None
    pre = acc
    if rowbias:
        smp = ((m // tm) * tm) // rpb if mutant == "rowbias_first" else m // rpb
        rb = case["rowbias"][smp]
        if rb_first and b is not None:
            pre = acc + (b + rb)
        elif is_staged and tile == 1 and b is not None:
            m0 = (m // tm) * tm
            one = (torch.minimum(m0 + tm, torch.tensor(M)) - 1) // rpb == m0 // rpb          # the tile lies in one sample: b += rb first
            pre = torch.where(one[:, None], acc + (b + rb), (acc + b) + rb)
        else:
            pre = (acc + b if b is not None else acc) + rb
    elif b is not None:
        pre = acc + b
    r = case["res"].float() if res else None
    if epi == 1:
        No = Nout // 2
        return (pre[:, :No] * act64(pre[:, No:].double(), 5).float()).half()
    if mutant == "res_before_act" and r is not None:
        pre, r = pre + r, None
    a = act64(pre.double(), epi).float()             # the activation correctly rounded to fp32 (torch's fp32 gelu cancels in the tail)
    if out_f32:
        return a
    if is_staged != (mutant == "swap_round"):
        o = a.half()
        if r is not None:
            o = (o.float() + r).half()
    else:
        o = (a + r if r is not None else a).half()
    if epi == 4:
        o = o.clamp_min(0.0)
    if mutant == "ragged_shift":
        assert Nout % 4
        g0 = Nout - Nout % 4
        o = o.clone()
        o[:, g0:] = torch.roll(o[:, g0:], -1, 1)
    return o


# ----------------------------------------------------------------------------- judging
def rel_l2(got, ref) -> float:
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).norm() / ref.norm()).item()


def _div(err, bnd) -> torch.Tensor:
    """err / bnd with 0 / 0 = 0 and err / 0 = inf"""
    return torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


def ratios(got, ref, bnd) -> torch.Tensor:
    """|got - ref| / bound per element (non-finite output: inf)"""
    g = got.double().cpu()
    r = _div((g - ref).abs(), bnd)
    return torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))


def beyond(got, ref, bnd, rnd) -> torch.Tensor:
    """what is left of |got - ref| beyond the single roundings `rnd`, over what is left of the bound (an element whose bound is nothing but
    its roundings -- a zero weight row without bias -- has nothing left: 0 if its error stays within them)"""
    g = got.double().cpu()
    r = _div(((g - ref).abs() - rnd).clamp_min(0.0), (bnd - rnd).clamp_min(0.0))
    return torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))


def worst_per_regime(ratio, rows, chans):
    worst = {}
    rr, cc = ratio.amax(1).tolist(), ratio.amax(0).tolist()
    for x, name in zip(rr, rows):
        worst[name] = max(worst.get(name, 0.0), x)
    for x, name in zip(cc, chans):
        worst["c:" + name] = max(worst.get("c:" + name, 0.0), x)
    return worst


def judge(kernel, what, got, ref, bnd, case, limit: float = 1.0, rnd=None, chans=None, quiet: bool = False, show_rnd=None):
    """Prints one ENV line -- the worst |got - ref| / bound per row regime and (c:) per channel regime -- and asserts every element
    finite and within `limit` x bound; no element is excluded.  With rnd (the CPU file's half-the-bound test): the plain ratio must be
    <= 1 and the limit applies to what is left of error and bound once the single roundings `rnd` are taken off both.  show_rnd (the
    GPU file): the same figure, worst over all elements, is appended to the ENV line and not asserted -- the plain ratio of an fp16
    output is mostly its own rounding."""
    chans = case["chans"] if chans is None else chans
    assert tuple(got.shape) == tuple(ref.shape) == tuple(bnd.shape), (got.shape, ref.shape, bnd.shape)
    ratio = ratios(got, ref, bnd)
    worst = worst_per_regime(ratio, case["rows"], chans)
    if not quiet:
        tail = ""
        if show_rnd is not None:
            tail = f"  | beyond the single roundings {float(beyond(got, ref, bnd, show_rnd).max()):.3f}"
        print(f"ENV {kernel} {what}: " + "  ".join(f"{r} {x:.2f}" for r, x in worst.items()) + tail)
    if rnd is not None:
        assert max(worst.values()) <= 1.0, (kernel, what, worst)
        ratio = beyond(got, ref, bnd, rnd)
        worst = worst_per_regime(ratio, case["rows"], chans)
        if not quiet:
            print("    beyond the single roundings: " + "  ".join(f"{r} {x:.2f}" for r, x in worst.items()))
    bad = {r: x for r, x in worst.items() if r.replace("c:", "") not in RECORDED and not x <= limit}
    if bad:
        i = int(ratio.flatten().argmax())
        m, n = divmod(i, ratio.shape[1])
        raise AssertionError(f"{kernel} {what}: |got - ref| beyond {limit:g} x bound: " + ", ".join(f"{r} {x:.2f}" for r, x in bad.items()) +
                             f" (worst element: row {m} ({case['rows'][m]}), channel {n} ({chans[n]}), got {float(got[m, n])!r}, "
                             f"exact {float(ref[m, n])!r}, bound {float(bnd[m, n]):.3e})")
    return worst


def leaves_bound(got, ref, bnd) -> int:
    """how many elements of `got` leave the bound (mutant tests)"""
    return int((~(ratios(got, ref, bnd) <= 1.0)).sum())


# ----------------------------------------------------------------------------- cases and launch specs shared by the CPU and the GPU file
_CASES = {}


def lin_key(C1=128, C2=0, CinP=None, Nout=NOUT_A, seed=1, big=4096.0, big_bias=1000.0, B=B_, T=T_):
    return ("lin", B, T, C1, C2, CinP if CinP else round_up(C1 + C2, 64), Nout, seed, big, big_bias)


def conv_key(regimes=("wall", "hot", "benign"), H=IMG[0], W=IMG[1], C1=64, C2=0, CinP=None, Nout=NOUT_A, seed=2, stride=1, ups=0,
             pad_same=False):
    return ("conv", tuple(regimes), H, W, C1, C2, CinP if CinP else round_up(C1 + C2, 64), Nout, seed, stride, ups, pad_same)


def case_of(key):
    """the planted case of a key with its fp64 reference (y, A): computed once, shared, never modified"""
    if key not in _CASES:
        case = plant_linear(*key[1:]) if key[0] == "lin" else plant_conv(*key[1:])
        case["y"], case["A"] = reference(case)
        case["key"] = key
        _CASES[key] = case
    return _CASES[key]


def spec(name, key, *, variant=5, tile=2, S=1, fused=False, epi=0, bias=True, rowbias=False, res=False, direct=False, ldo_pad=8,
         out_off=0, ldr_pad=8, res_off=0):
    """one igemm launch.  ldo = round_up(NoutO, 4) + ldo_pad, ldr likewise; offsets in halfs on top of a 16-byte aligned NaN guard."""
    nout = key[6] if key[0] == "lin" else key[7]
    nout_o = nout // 2 if epi == 1 else nout
    s = dict(name=name, key=key, variant=variant, bk=VARIANTS[variant][0], tile=tile, S=S, fused=fused, epi=epi, bias=bias, rowbias=rowbias,
             res=res, direct=direct, Nout=nout, NoutO=nout_o, ldo=round_up(nout_o, 4) + ldo_pad, out_off=out_off,
             ldr=round_up(nout, 4) + ldr_pad, res_off=res_off)
    s["staged"] = staged(ldo=s["ldo"], Nout=nout, epi=epi, out_off=out_off, splitk=S, fused=fused, direct=direct, res=res, ldr=s["ldr"],
                         res_off=res_off)
    s["form"] = ("igemm", "staged" if s["staged"] else ("splitk2" if S > 1 and not fused else "direct"))
    s["what"] = (f"{name} t{tile} v{variant} S{S}{'f' if fused and S > 1 else ''} epi{epi}{'+rb' if rowbias else ''}{'+res' if res else ''} "
                 f"{'staged' if s['staged'] else 'direct'}")
    return s


_EXPECT = {}


def expected(s):
    """(exact, bound, unavoidable rounding, restatement) of a spec; cached on what each depends on"""
    case = case_of(s["key"])
    kb = (s["key"], s["epi"], s["bias"], s["rowbias"], s["res"], s["S"], s["form"])
    if kb not in _EXPECT:
        _EXPECT[kb] = exact_and_bound(case, case["y"], case["A"], epi=s["epi"], bias=s["bias"], rowbias=s["rowbias"], res=s["res"], S=s["S"],
                                      form=s["form"])
    kr = kb + (s["bk"], s["tile"] if s["rowbias"] and s["staged"] else 0, s["staged"])
    if kr not in _EXPECT:
        _EXPECT[kr] = restate(case, bk=s["bk"], S=s["S"], tile=s["tile"], is_staged=s["staged"], epi=s["epi"], bias=s["bias"],
                              rowbias=s["rowbias"], res=s["res"])
    return _EXPECT[kb] + (_EXPECT[kr],)


def out_chans(s):
    """the channel regimes of the output columns (GEGLU: those of the value half)"""
    return case_of(s["key"])["chans"][:s["NoutO"]]


def specs_variants(tile: int, variant: int):
    """a. one pipeline shape on one tile: linear, 3x3 fast gather, 3x3 generic (concat; ups = 1), K loop of 1 ... NS + 2 and more steps"""
    out = []
    cins = variant_cins(variant)
    for cin in cins:
        out.append(spec(f"lin K{cin}", lin_key(C1=cin), variant=variant, tile=tile))
        out.append(spec(f"conv3x3 C{cin}", conv_key(C1=cin), variant=variant, tile=tile))
        out.append(spec(f"conv3x3 concat 8+{cin - 16}", conv_key(C1=8, C2=cin - 16, CinP=cin, seed=3), variant=variant, tile=tile))
    out.append(spec("lin K72 in 128", lin_key(C1=72, CinP=128, seed=4), variant=variant, tile=tile))
    out.append(spec("conv3x3 C72 in 128", conv_key(C1=72, CinP=128, seed=5), variant=variant, tile=tile))
    out.append(spec(f"conv3x3 ups C{cins[0]}", conv_key(C1=cins[0], ups=1, seed=6), variant=variant, tile=tile))
    return out


def specs_splitk(tile: int):
    """b. uneven shares, a split shorter than the ring, splits that own no step (S = Kp / 64 on a BK 128 shape), both reductions"""
    out = []
    for fused in (False, True):
        kw = dict(tile=tile, fused=fused, epi=2, res=True)
        out.append(spec("lin K320", lin_key(C1=320), variant=5, S=3, **kw))                        # 5 steps: 1, 2, 2
        out.append(spec("lin K320", lin_key(C1=320), variant=3, S=4, **kw))                        # 10 steps of 32: 2, 3, 2, 3 < 6 stages
        out.append(spec("lin K384", lin_key(C1=384), variant=6, S=6, **kw))                        # 3 steps of 128 for 6 splits
        out.append(spec("lin K72 in 128 N70", lin_key(C1=72, CinP=128, Nout=NOUT_B, seed=4), variant=5, S=2, tile=tile, fused=fused,
                        epi=0, res=True, ldo_pad=4))
        out.append(spec("conv3x3 C64", conv_key(C1=64), variant=1, S=4, **kw))                     # 9 steps: 2, 2, 2, 3
        out.append(spec("conv3x3 C128", conv_key(C1=128), variant=6, S=18, tile=tile, fused=fused, epi=4, res=True))   # 9 steps, 18 splits
        out.append(spec("conv3x3 concat 8+72", conv_key(C1=8, C2=72, CinP=128, seed=3), variant=0, S=5, **kw))
    return out


def specs_epilogues():
    """c. epi 0 - 5 with and without residual; the staged form and the three ways to the direct one; row bias crossing tiles"""
    out = []
    for nout in (NOUT_A, NOUT_B):
        key = lin_key(C1=128, Nout=nout, seed=7)
        for epi in (0, 2, 3, 4, 5):
            for res in (False, True):
                forms = [dict(direct=True), dict(ldo_pad=4), dict(out_off=4)]
                if nout % 8 == 0:
                    forms.insert(0, dict())
                    if res:
                        forms.append(dict(ldr_pad=4))            # an unaligned residual pitch alone sends the launch to the direct form
                for f in forms:
                    out.append(spec(f"lin N{nout}", key, epi=epi, res=res, **f))
        out.append(spec(f"lin N{nout}", key, tile=1, epi=2, res=True))
        out.append(spec(f"lin N{nout}", key, tile=1, epi=4, res=True, direct=True))
        out.append(spec(f"lin N{nout} no bias", key, bias=False, epi=0, res=True))
    for tile in (1, 2):
        for kw in (dict(), dict(direct=True)):
            for epi, res in ((0, True), (2, False), (4, True)):
                out.append(spec("lin rowbias", lin_key(C1=128, seed=7), tile=tile, rowbias=True, epi=epi, res=res, **kw))
            out.append(spec("conv rowbias", conv_key(C1=64), tile=tile, rowbias=True, epi=0, res=True, **kw))
    return out


GEGLU_KEY = lin_key(C1=128, Nout=160, seed=8, big=32.0, big_bias=60.0)


def specs_geglu():
    return [spec("geglu N160", GEGLU_KEY, tile=tile, epi=1, **kw) for tile in (1, 2) for kw in (dict(), dict(direct=True), dict(ldo_pad=4))]


def specs_geometry():
    """d. stride 2 on odd and even sizes, pad_same, ups, concat 8 + 72, 1 x 1 and 1 x W images, the wall sample first / middle / last"""
    out = []
    for i, regs in enumerate((("wall", "benign", "hot"), ("hot", "wall", "benign"), ("benign", "hot", "wall"), ("big", "tiny", "offset"))):
        out.append(spec(f"conv {'/'.join(regs)}", conv_key(regs, seed=10 + i), variant=1))
        out.append(spec(f"conv s2 7x6 {'/'.join(regs)}", conv_key(regs, stride=2, seed=10 + i), variant=5))
    for tile in (1, 2):
        out.append(spec("conv s2 6x5", conv_key(H=6, W=5, stride=2, seed=20), tile=tile))
        out.append(spec("conv s2 pad_same 8x6", conv_key(H=8, W=6, stride=2, pad_same=True, seed=21), tile=tile))
        out.append(spec("conv ups 7x6", conv_key(ups=1, seed=22), tile=tile, epi=2))
        out.append(spec("conv ups concat 8+72", conv_key(C1=8, C2=72, CinP=128, ups=1, seed=23), tile=tile))
        out.append(spec("conv concat 8+72 N70", conv_key(C1=8, C2=72, CinP=128, Nout=NOUT_B, seed=24), tile=tile, ldo_pad=4, res=True))
        out.append(spec("conv 1x1 image", conv_key(("wall", "hot", "benign", "offset", "big"), H=1, W=1, seed=25), tile=tile))
        out.append(spec("conv 1x6 image", conv_key(H=1, W=6, seed=26), tile=tile))
        out.append(spec("conv 7x1 image s2", conv_key(H=7, W=1, stride=2, seed=27), tile=tile))
    return out


def all_specs():
    out = []
    for tile in (1, 2):
        for v, (_bk, _ns, big_ok) in VARIANTS.items():
            if tile == 2 or big_ok:
                out += specs_variants(tile, v)
        out += specs_splitk(tile)
    return out + specs_epilogues() + specs_geglu() + specs_geometry()


def iid_linear(M: int, K: int, N: int):
    """the operands of test_gpu_kernels.test_igemm_linear as a case (every row and channel benign)"""
    def rnd(*shape, seed, scale=1.0):
        return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(torch.float16)
    case = dict(conv=False, B=1, T=M, M=M, C1=K, C2=0, K=K, CinP=round_up(K, 64), taps=1, Nout=N, x1=rnd(M, K, seed=1), x2=None,
                w=rnd(N, K, seed=2, scale=K ** -0.5), bias=rnd(N, seed=3).float(), res=rnd(M, N, seed=4), rows=["benign"] * M,
                chans=["benign"] * N, rows_per_bias=50, rowbias=rnd(-(-M // 50), N, seed=5).float())
    return case


def iid_conv(B: int, cin: int, cout: int, H: int, W: int, C2: int = 0):
    """the operands of test_gpu_kernels.test_igemm_conv3x3 (stride 1) as a case"""
    def rnd(*shape, seed, scale=1.0):
        return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(torch.float16)
    x = rnd(B, cin, H, W, seed=1).permute(0, 2, 3, 1).reshape(B * H * W, cin)
    w = rnd(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5).permute(0, 2, 3, 1).reshape(cout, 9 * cin)
    M = B * H * W
    C1 = cin - C2
    return dict(conv=True, B=B, Hin=H, Win=W, Hout=H, Wout=W, stride=1, ups=0, pad=1, M=M, C1=C1, C2=C2, K=cin, CinP=round_up(cin, 64),
                taps=9, Nout=cout, x1=x[:, :C1].contiguous(), x2=x[:, C1:].contiguous() if C2 else None, w=w.contiguous(),
                bias=rnd(cout, seed=3).float(), res=rnd(M, cout, seed=4), rows=["benign"] * M, chans=["benign"] * cout,
                rows_per_bias=H * W, rowbias=rnd(B, cout, seed=5).float())


# ----------------------------------------------------------------------------- skinny_linear (misc.hip): M <= 8, one wave per column
SKINNY_KEY = lin_key(C1=136, CinP=192, Nout=NOUT_B, seed=9, B=1, T=6)        # six rows: every row regime once; K % 64 != 0


def specs_skinny():
    return [dict(key=SKINNY_KEY, silu=silu, f32=f32, what=f"6x136x70{' silu' if silu else ''} {'fp32' if f32 else 'fp16'} out")
            for silu in (False, True) for f32 in (False, True)]


def expected_skinny(s):
    """v_dot2_f32_f16 chains per lane and a wave sum: fp32 sums in some order, bias, SiLU, one store (fp16: rounded once; fp32: as is)"""
    case = case_of(s["key"])
    epi = 2 if s["silu"] else 0
    exact, bnd, rnd = exact_and_bound(case, case["y"], case["A"], epi=epi, form=("skinny", "f32" if s["f32"] else "f16"))
    return exact, bnd, rnd, restate(case, bk=64, epi=epi, out_f32=s["f32"])


# ----------------------------------------------------------------------------- the sibling kernels, plain paths (pro = 0)
SIB_LIN = lin_key(C1=192, Nout=192, seed=40, B=3, T=64)                       # rowgemm_ok / wsgemm_ok: K % 64, Nout % 32, T % 32
SIB_LIN_CAT = lin_key(C1=128, C2=64, Nout=192, seed=41, B=3, T=64)
SIB_CONV = conv_key(("wall", "hot", "benign"), H=8, W=16, C1=64, Nout=128, seed=42)            # cconv_ok: one 8 x 16 patch per sample
SIB_CONV_CAT = conv_key(("benign", "wall", "hot"), H=8, W=16, C1=64, C2=64, Nout=128, seed=43)
SIBLING_CASES = (("wsgemm", SIB_LIN, False), ("wsgemm", SIB_LIN_CAT, False), ("wsgemm", SIB_CONV, True), ("wsgemm", SIB_CONV_CAT, True),
                 ("rowgemm", SIB_LIN, False), ("pconv", SIB_CONV, True), ("pconv", SIB_CONV_CAT, True), ("cconv", SIB_CONV, True),
                 ("cconv", SIB_CONV_CAT, True))                               # (kernel, case, with the per-sample row bias)


def expected_sibling(kernel, key, rowbias: bool, S: int = 1):
    """bias (+ row bias) + residual through the staged epilogue; S = K slices x K groups of the schedule (the bound's slab count)"""
    case = case_of(key)
    kb = (kernel, key, rowbias, S)
    if kb not in _EXPECT:
        _EXPECT[kb] = exact_and_bound(case, case["y"], case["A"], rowbias=rowbias, res=True, S=S, form=(kernel, "staged"))
    kr = ("sibling restated", key, rowbias)
    if kr not in _EXPECT:
        _EXPECT[kr] = restate(case, bk=64, is_staged=True, rowbias=rowbias, res=True, rb_first=True)
    return _EXPECT[kb] + (_EXPECT[kr],)
