"""Planted operands, fp64 references, per-element bounds, plain-torch restatements and mutants for the FUSED forms of the row kernels
(test_fused_envelope_cpu.py, test_gpu_fused_envelope.py): rowgemm behind its LayerNorm (pro = 1) and GroupNorm (pro = 2) prologues, with
GEGLU (epi = 1) and with the transposed V^T store (out_t / ntr); wsgemm with the accumulator-side LayerNorm fold (pro = 1 + colsum), with
GEGLU, V^T and split-K; the rowchain head segments and the rowchain tail, stage by stage.  gemm_cases.py pins the same kernels on their
plain paths, norm_cases.py pins the normalisations with identity weights; here dense planted weights sit behind planted statistics.

Data.  LayerNorm rows follow norm_cases.planted_rows regimes (`LN_ROWS`: benign, r10, r30, small, small_off, large, const, outlier, ramp
and, on the two-pass paths, r100; the fold runs `FOLD_ROWS`), the layout rotates per sample; GroupNorm inputs are norm_cases.planted
(every (sample, group) its own regime).  Weights are dense (scale K^-0.5) with gemm_cases.CH_REGIMES per output channel (zero, hotw,
bigbias, alt), gamma / beta are norm_cases.affine.  GEGLU: every second gate channel is a zero weight row whose bias is one of
`GATE_TARGETS` (-8, -2, 0, 2, 8): the gate pre-activation is that bias exactly, whatever the row.

Reference.  fp64 on the same fp16 operands: n = F.layer_norm / F.group_norm in fp64 without affine, y = n W'^T + b' with W' and b' (and
colsum) read back from what ops.pack_rowgemm / ops.pack_wsgemm produced -- what the matrix cores multiply.  eps is the fp32 value
the launch record carries.

Bound.  u = 2^-11, e = 2^-24, c_r = `C_RSQ` (rsqrtf: measured).  The error dn_k of one normalised fp16 operand, then
E_pro = sum_k dn_k |w'_k|, handed to gemm_cases.exact_and_bound as `extra` next to its own terms over A = sum |n w'| + E_pro.

  two-pass LayerNorm (rowgemm.hip consume_group `o[e] = (h16)(((float)v[u][e] - mean) * rstd)` and the same line of finish_row_lds;
  rowchain's LayerNorm is bit-identical):
    mean_d = fp32 sum of K terms in some order / K:            |mean_d - mean| <= dm = K e mean|x|
    q_d = fp32 sum of fl(d^2), d = fl(x - mean_d):             q_d / K in [var (1 - th), (var + dm^2) (1 + th)], th = (K + 2) e
    rstd_d = rsqrtf(fl(q_d / K + eps)):                        rstd_d / rstd in [1 - rho, 1 + rho], from the interval of the argument
                                                               widened by 2 e (divide, add) and by c_r; rho is about (K / 2 + c_r) e
    dn_k = u |n_k| + 2^-25 + (|n_k| (rho + 2 e) + dm rstd_hi) (1 + u)
  (the issue's c e (|n_k| + |mean| rstd) with c about K, and mean|x| >= |mean| in its place: the sum's error is over sum |x|.)

  GroupNorm prologue (rowgemm.hip `const float var = fmaxf(q * inv - mean * mean, 0.f)`, `shf_s[tid] = -mean * rstd`,
  `o[e] = (h16)((float)v[u][e] * sa[e] + ha[e])`) on norm_cases.exact_acc accumulators (quanta 2^-20, 2^-12; cnt = T cpg):
    |mean_d - mean| <= dmean = 3 e |mean| + 2^-21 / cnt        (int -> float, 1 / cnt, the product)
    |var_d - var| <= dvar = e (4 var + 11 mean^2) + 2^-13 / cnt + 2^-20 |mean| / cnt          -- the cancellation: e (1 + mean^2 / var) on rstd
    rho from [max(var - dvar, 0) + eps, var + dvar + eps] as above
    dn_k = u |n_k| + 2^-25 + (|n_k| (rho + e) + rstd_hi (dmean + e (2 |mean| + 2 |x_k|))) (1 + u)

  wsgemm fold (wsgemm.hip `const float var = fmaxf(stat[2 * tid + 1] * inv - mean * mean, 0.f)`, `stat[2 * tid + 1] = -mean * rstd`,
  `o[e] = (h16)(acc[i][mt][4 * g4 + e] * rsd[mt] + nmr[mt] * cs[e] + b2[e])`); P = sum x w', Ax = sum |x w'|, single-pass sums over K
  terms and S slabs:
    dm = (K + 2) e mean|x|,  dvar = (K + 3) e E[x^2] + 2 |mean| dm + dm^2 + e (mean^2 + var)           -- e (mean^2 + var) / var on rstd
    z = rstd (P - mean colsum64) = n W'^T exactly; the device takes colsum32 = ops.pack_wsgemm's fp32 sum:
    E_z = rho |z| + rstd_hi ((K + S + 2) e Ax + dm |colsum| + |mean| |colsum32 - colsum64|) + e rstd_hi (2 |P| + 3 |mean colsum|)
  and E_z is the `extra` of exact_and_bound with A = 0.  `RECORDED_FOLD` = (r100): |mean| / std = 100 makes dvar about var itself; the
  project accepts 2e-2 per row there (norm_cases.TOL_R100), the rows are printed and asserted finite.  `RECORDED` is empty: no other
  regime had to leave the asserted set.

  GEGLU: gemm_cases' bound with Ev, Eg carrying E_pro.  V^T: the row-major bound (`(h16)(acc[i][mt][4 * g4 + e] + bb[e])`, a store path).
  Plain stages of the chains (pro = 0): gemm_cases' staged bound as it stands (E_pro = 0).

  clip_linear (clip.hip `r[e] = (h16)fmaf((v0[e] - mean) * rstd, g0[e], b0[e])`, `stat[r][1] = 1.0f / sqrtf(q / (float)a.K + a.eps)`,
  `for (int w = 0; w < NW; ++w) v += red[w][j][ln]`, `if (a.epi == 1) v = v / (1.0f + expf(-1.702f * v))`): the two-pass terms with
  c_r = 2 e (a correctly rounded square root and quotient) in front of the affine map, a_k = n_k gamma_k + beta_k:
    da_k = u |a_k| + 2^-25 + (dn32_k |gamma_k| + e |a_k|) (1 + u),   dn32_k = dn_k without its fp16 rounding
  S = NW partial sums; one rounding of the output (fp16), or none but the fp32 add (`out[o] = out[o] + v`).  quick_gelu(v) =
  v sigma(1.702 v): Lipschitz 1.1 (as SiLU), own relative error (c_exp + 1.702 |v| + 4) e -- the argument's product, expf, the sum, the
  quotient and the argument error 1.702 |v| e of the exponential -- with c_exp = 4: expf is documented at 1 ulp = 2 e in HIP's math
  API; not measured here, hence the factor 2 of gemm_cases.ACT_MARGIN.  Against u |out| this term is 1e-3 of the bound.

A const row normalises to 0 exactly on the two-pass paths (the fp32 sum of K equal fp16 values and its quotient are exact), so its
output is h16(b') (+ residual in fp16) bit for bit: `const_rows`.
"""
import math

import torch
import torch.nn.functional as F

import gemm_cases as gc
import norm_cases as nc

U, E32, SUB = gc.U, gc.E32, gc.SUBNORMAL
F32, F64 = torch.float32, torch.float64

# rsqrtf as hipcc emits it for gfx950 (v_rsq_f32): relative error, measured on an MI355X through gn_apply (mean 0, var planted exactly
# through the fixed-point accumulator, eps 0, gamma 1, beta 0: out = fp16(x rstd)) against fp64 at 8 x 8.4 M points over var in
# [8e-4, 2.6e5] with full 24-bit mantissas in both exponent parities (what the cases produce lies inside) -- the excess of the fp16
# output over half an fp16 spacing of the exact x rstd, as gemm_cases.GELU_MEASURED: 1.203e-7 = 2.02 x 2^-24; it includes the fp32
# rounding of the product.  Times gemm_cases.ACT_MARGIN, because only the sweep's grid was sampled.
RSQ_MEASURED = 1.203e-7
C_RSQ = gc.ACT_MARGIN * RSQ_MEASURED

LN_ROWS = ("benign", "r10", "r30", "small", "small_off", "large", "const", "outlier", "ramp", "r100")
FOLD_ROWS = ("benign", "small", "small_off", "large", "r30", "r100")
RECORDED = ()
RECORDED_FOLD = ("r100",)
GATE_TARGETS = (-8.0, -2.0, 0.0, 2.0, 8.0)
EPS_LN, EPS_GN = 1e-5, 1e-6
G = 32


def eps32(eps: float) -> float:
    return float(torch.tensor(eps, dtype=F32))


# ----------------------------------------------------------------------------- planted operands
def plant_rows(B: int, T: int, K: int, regimes=LN_ROWS, seed: int = 1):
    """(fp16 [B T, K], regime per row): sample b runs the regime list rotated by b, with its own draw"""
    Kp = gc.round_up(K, 10)
    xs, names = [], []
    for b in range(B):
        regs = tuple(regimes[(i + b) % len(regimes)] for i in range(len(regimes)))
        xs.append(nc.planted_rows(T, Kp, seed + 17 * b, regs)[:, :K])
        names += nc.row_regimes(T, regs)
    return torch.cat(xs).contiguous(), names


def plant_weights(Nout: int, K: int, seed: int, big_bias: float = 1000.0, geglu: bool = False, hot=None):
    """(w fp16 [Nout, K], bias fp32 [Nout], channel regime per OUTPUT column).  geglu: rows [0, Nout / 2) are the value channels
    (gemm_cases.CH_REGIMES), row Nout / 2 + c the gate of column c: for even c a zero row with bias GATE_TARGETS[...] (the column is
    then named after the target), for odd c dense"""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(Nout, K, generator=gen, dtype=F64) * K ** -0.5
    bias = torch.randn(Nout, generator=gen, dtype=F64)
    nv = Nout // 2 if geglu else Nout
    hk = gc.hot_ks(K, K) if hot is None else list(hot)
    chans, j = [], 0
    for n in range(nv):
        name = gc.CH_REGIMES[n % len(gc.CH_REGIMES)]
        chans.append(name)
        if name == "zero":
            w[n] = 0.0
        elif name == "hotw":
            w[n] = 0.0
            w[n, hk[j % len(hk)]] = (0.5 + (j % 7) / 8.0) * (-1.0) ** j
            j += 1
        elif name == "bigbias":
            bias[n] = big_bias * (1.0 + 0.37 * math.sin(n)) * (-1.0) ** n
        elif name == "alt":
            w[n] = w[n].abs() * (1.0 - 2.0 * (torch.arange(K) % 2).double()) * 2.0 ** -8
            bias[n] = 0.0
    if geglu:
        for c in range(nv):
            if c % 2 == 0:
                t = GATE_TARGETS[(c // 2 + c // 10) % len(GATE_TARGETS)]
                w[nv + c] = 0.0
                bias[nv + c] = t + 0.01 * float(torch.randn(1, generator=gen, dtype=F64))
                chans[c] = f"g{t:+.0f}"
    return w.to(torch.float16), bias.to(F32), chans


def plant_residual(M: int, Nout: int, bias, chans, seed: int):
    """fp16 [M, Nout]; on the bigbias channels it cancels the bias (the staged epilogue's first rounding is then 0.5 absolute)"""
    res = torch.randn(M, Nout, generator=torch.Generator().manual_seed(seed), dtype=F64)
    for n, name in enumerate(chans):
        if name == "bigbias":
            res[:, n] += -float(bias[n])
    return res.to(torch.float16)


def fold_pack(w16, bias, gamma=None, beta=None, *, geglu: bool = False, ws: bool = False):
    """what the packer makes of a layer, on the CPU: dict(wp, bp, cs: as the launch takes them; W fp16 [Nout, K], b fp32, cs32: the
    same read back in the natural row order (GEGLU: value rows, then gate rows))"""
    from live2diff_amd import ops
    n, k = w16.shape
    if ws:
        wp, bp, cs = ops.pack_wsgemm(w16, bias, gamma, beta, geglu)
    else:
        (wp, bp), cs = ops.pack_rowgemm(w16, bias, gamma, beta, geglu), None
    W, b, c = ops.unpack_rowgemm(wp, n, k), bp, cs
    if geglu:
        perm = ops.rowgemm_geglu_perm(n // 2, "cpu")
        W, b = torch.empty_like(W).index_copy_(0, perm, W), torch.empty_like(bp).index_copy_(0, perm, bp)
        c = None if cs is None else torch.empty_like(cs).index_copy_(0, perm, cs)
    return dict(wp=wp, bp=bp, cs=cs, W=W.contiguous(), b=b, cs32=c, geglu=geglu, Nout=n, K=k)


# ----------------------------------------------------------------------------- the norms: exact value and error of the fp16 operand
def _rho(v_lo, v_hi, v, eps, c_r=C_RSQ):
    """(relative half-width of rstd_d around rstd, rstd_hi) for an argument in [v_lo + eps, v_hi + eps] before its own two roundings"""
    rstd = (v + eps) ** -0.5
    hi = ((v_lo + eps) * (1 - 2 * E32)) ** -0.5 * (1 + c_r)
    lo = ((v_hi + eps) * (1 + 2 * E32)) ** -0.5 * (1 - c_r)
    return torch.maximum(hi / rstd - 1, 1 - lo / rstd), hi


def ln_two_pass(x16, eps: float = EPS_LN, c_r=C_RSQ, fp32_part: bool = False):
    """(n, dn) fp64 [M, K] (module docstring).  fp32_part: dn without the fp16 rounding of n (clip_linear rounds after its affine map)"""
    eps = eps32(eps)
    x = x16.double()
    K = x.shape[1]
    n = F.layer_norm(x, (K,), None, None, eps)
    var = x.var(1, unbiased=False, keepdim=True)
    dm = K * E32 * x.abs().mean(1, keepdim=True)
    th = (K + 2) * E32
    rho, hi = _rho(var * (1 - th), (var + dm * dm) * (1 + th), var, eps, c_r)
    d32 = n.abs() * (rho + 2 * E32) + dm * hi
    return n, (d32 if fp32_part else U * n.abs() + SUB + d32 * (1 + U))


def gn_prologue(x16, B: int, T: int, eps: float = EPS_GN, ng: int = G):
    """(n, dn) fp64 [B T, C] for the GroupNorm prologue on norm_cases.exact_acc accumulators"""
    eps = eps32(eps)
    C = x16.shape[-1]
    cpg = C // ng
    x = x16.double().view(B, T, C)
    n = F.group_norm(x.permute(0, 2, 1), ng, None, None, eps).permute(0, 2, 1)
    xs = x.view(B, T, ng, cpg)
    cnt = T * cpg
    mean, var = xs.mean((1, 3)), xs.var((1, 3), unbiased=False)
    dmean = 3 * E32 * mean.abs() + 2.0 ** -21 / cnt
    dvar = E32 * (4 * var + 11 * mean ** 2) + 2.0 ** -13 / cnt + 2.0 ** -20 * mean.abs() / cnt
    rho, hi = _rho((var - dvar).clamp_min(0.0), var + dvar, var, eps)
    ex = lambda t: t[:, None, :, None].expand(B, T, ng, cpg).reshape(B, T, C)       # per group -> per element
    dn = U * n.abs() + SUB + (n.abs() * (ex(rho) + E32) + ex(hi) * (ex(dmean) + E32 * (2 * ex(mean.abs()) + 2 * x.abs()))) * (1 + U)
    return n.reshape(B * T, C), dn.reshape(B * T, C)


def fold_error(x16, W16, cs32, eps: float, S: int):
    """(z = n W'^T, E_z) fp64 [M, Nout] for the accumulator-side fold"""
    eps = eps32(eps)
    x, W = x16.double(), W16.double()
    K = x.shape[1]
    z = F.layer_norm(x, (K,), None, None, eps) @ W.t()
    mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    dm = (K + 2) * E32 * x.abs().mean(1, keepdim=True)
    dvar = (K + 3) * E32 * (x * x).mean(1, keepdim=True) + 2 * mean.abs() * dm + dm * dm + E32 * (mean ** 2 + var)
    rho, hi = _rho((var - dvar).clamp_min(0.0), var + dvar, var, eps)
    P, Ax = x @ W.t(), x.abs() @ W.abs().t()
    cs = cs32.double()[None]
    dcs = (cs - W.sum(1)[None]).abs()
    ez = rho * z.abs() + hi * ((K + S + 2) * E32 * Ax + dm * cs.abs() + mean.abs() * dcs) + E32 * hi * (2 * P.abs() + 3 * (mean * cs).abs())
    return z, ez


# ----------------------------------------------------------------------------- exact result and bound of one launch
def expect(x16, fd, *, pro=0, eps=None, epi=0, res=None, gn=None, S=1, form=("rowgemm", "staged"), rows=None, chans=None):
    """One launch on the fp16 input x16 [M, K] (the device's own previous stage in the chains) with the packed layer fd (fold_pack).
    pro: 0 plain, 1 two-pass LayerNorm, 2 GroupNorm prologue (gn = (B, T)), "fold".  Returns dict(exact, bnd, rnd, n, case): `case`
    serves gemm_cases.judge (rows, chans)."""
    M, K = x16.shape
    Nout = fd["Nout"]
    W = fd["W"].double()
    if pro == "fold":
        y, extra = fold_error(x16, fd["W"], fd["cs32"], eps, S)
        A, n, rn = torch.zeros_like(y), None, None
    else:
        if pro == 0:
            n, dn = x16.double(), None
        elif pro == 1:
            n, dn = ln_two_pass(x16, eps)
        else:
            n, dn = gn_prologue(x16, gn[0], gn[1], eps)
        y, A = n @ W.t(), n.abs() @ W.abs().t()
        extra, rn = None, None
        if dn is not None:
            extra = dn @ W.abs().t()
            A = A + extra
            # single roundings, each of which may use all of its term: the operands' own fp16 roundings; behind the GroupNorm prologue
            # every term of dn (a dozen roundings of per-group scalars, no sum whose order is open)
            rn = extra if pro == 2 else (U * n.abs() + SUB) @ W.abs().t()
    case = dict(M=M, Nout=Nout, K=K, taps=1, bias=fd["b"], rows_per_bias=M, res=res, rows=rows or ["benign"] * M,
                chans=chans or ["benign"] * (Nout // 2 if epi == 1 else Nout))
    exact, bnd, rnd = gc.exact_and_bound(case, y, A, epi=epi, res=res is not None, S=1 if pro == "fold" else S, form=form, extra=extra)
    if rn is not None:
        if epi == 1:
            No = Nout // 2
            pre = y + fd["b"].double()[None]
            rnd = rnd + gc.act64(pre[:, No:], 5).abs() * rn[:, :No] + pre[:, :No].abs() * gc.LIP[5] * rn[:, No:]
        else:
            rnd = rnd + rn * (1 + 2 * U)
    return dict(exact=exact, bnd=bnd, rnd=rnd, n=n, case=case, y=y)


def const_rows(rows):
    return torch.tensor([r == "const" for r in rows])


# ----------------------------------------------------------------------------- restatements (plain torch, fp32) and their mutants
MUTANTS = ("geglu_pair_swap", "bias_swap", "tanh_gelu", "prev_row_mean", "vt_shift", "colsum_unrounded", "slab0_norm", "gn_neighbour",
           "ln_unrounded_h")


def restate_ln(x16, eps: float = EPS_LN, mutant=None, xf=None):
    """rowgemm.hip's two-pass LayerNorm -> fp16 operand.  xf: the fp32 row to normalise instead (mutant ln_unrounded_h)"""
    x = x16.float() if xf is None else xf
    K = x.shape[1]
    mean = x.sum(1, keepdim=True) / K
    if mutant == "prev_row_mean":                     # the rows of the ragged last tile take their neighbour's mean
        M = x.shape[0]
        assert M % 32
        mean = mean.clone()
        mean[M - M % 32 + 1:] = mean[M - M % 32:-1].clone()
    d = x - mean
    rstd = torch.rsqrt((d * d).sum(1, keepdim=True) / K + torch.tensor(eps, dtype=F32))
    return (d * rstd).half()


def restate_gn(x16, B: int, T: int, eps: float = EPS_GN, mutant=None, ng: int = G):
    """the prologue's decode of exact accumulators (norm_cases.decode with the affine part in the weights)"""
    C = x16.shape[-1]
    acc = nc.exact_acc(x16.view(B, T, C), ng)
    if mutant == "gn_neighbour":
        acc = torch.roll(acc, 1, 0)
    one, zero = torch.ones(C, dtype=F32), torch.zeros(C, dtype=F32)
    return nc.decode(x16.view(B, T, C), acc, ng, one, zero, eps).view(B * T, C)


def _gelu32(g, tanh: bool):
    if tanh:
        gd = g.double()
        return (0.5 * gd * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (gd + 0.044715 * gd ** 3)))).float()
    return gc.act64(g.double(), 5).float()


def _epilogue(pre, fd, epi, res, mutant):
    """fp32 pre-activation [M, Nout] (bias included) -> fp16 output; GEGLU pairs column c with column Nout / 2 + c"""
    if epi == 1:
        No = fd["Nout"] // 2
        v, g = pre[:, :No], pre[:, No:]
        o = (v * _gelu32(g, mutant == "tanh_gelu")).half()
        if mutant == "geglu_pair_swap":               # one 16-channel group of the second 32-row tile
            r0, c0 = 32, 16 * ((No // 16) // 2)
            o = o.clone()
            o[r0:r0 + 32, c0:c0 + 16] = (g[r0:r0 + 32, c0:c0 + 16] * _gelu32(v[r0:r0 + 32, c0:c0 + 16], False)).half()
        return o
    o = pre.half()
    return o if res is None else (o.float() + res.float()).half()


def restate(x16, fd, *, pro=0, eps=None, epi=0, res=None, gn=None, S=1, mutant=None, xf=None):
    """the kernel's arithmetic in plain fp32 torch -> fp16 [M, NoutO]"""
    assert mutant is None or mutant in MUTANTS
    W, b = fd["W"].float(), fd["b"]
    if mutant == "bias_swap":
        No = fd["Nout"] // 2
        b = torch.cat([b[No:], b[:No]])
    if pro == "fold":
        x = x16.float()
        K = x.shape[1]
        nk = K // 64
        parts = [(x[:, 64 * lo:64 * hi], W[:, 64 * lo:64 * hi]) for lo, hi in gc.split_ranges(nk, S)]
        accs = [xs @ ws.t() for xs, ws in parts]
        sx, sq = sum(xs.sum(1, keepdim=True) for xs, _ in parts), sum((xs * xs).sum(1, keepdim=True) for xs, _ in parts)
        inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(K), dtype=F32)
        mean = sx * inv
        var = (sq * inv - mean * mean).clamp_min(0.0)
        rsd = torch.rsqrt(var + torch.tensor(eps, dtype=F32))
        nmr = -mean * rsd
        cs = fd["cs32"]
        if mutant == "colsum_unrounded":
            cs = fd["cs_unrounded"]
        if mutant == "slab0_norm":
            assert S > 1
            pre = accs[0] * rsd + sum(accs[1:]) + nmr * cs[None] + b[None]
        else:
            pre = sum(accs) * rsd + nmr * cs[None] + b[None]
        return _epilogue(pre, fd, epi, res, mutant)
    if pro == 0:
        n16 = x16
    elif pro == 1:
        n16 = restate_ln(x16, eps, mutant, xf)
    else:
        n16 = restate_gn(x16, gn[0], gn[1], eps, mutant)
    return _epilogue(n16.float() @ W.t() + b[None], fd, epi, res, mutant)


def vt_of(full, B: int, T: int, ntr: int, mutant=None):
    """the V^T tensor [B, ntr, T] a launch stores for the last ntr columns of `full` [B T, Nout]"""
    v = full[:, full.shape[1] - ntr:].reshape(B, T, ntr).permute(0, 2, 1).contiguous()
    if mutant == "vt_shift":
        v[B - 1] = torch.roll(v[B - 1], 1, 1)
    return v


def vt_back(vt, B: int, T: int):
    """[B, ntr, >= T] -> [B T, ntr]"""
    return vt[:, :, :T].permute(0, 2, 1).reshape(B * T, vt.shape[1])


# ----------------------------------------------------------------------------- judging (gemm_cases.judge with a recorded set)
def judge(kernel, what, got, ex, recorded=RECORDED, limit: float = 1.0, half: bool = False, quiet: bool = False):
    """gemm_cases.judge on an `expect` result.  Rows of a `recorded` regime are printed and asserted finite only.  half (the CPU file):
    the limit applies beyond the single roundings."""
    case = ex["case"]
    keep = torch.tensor([r not in recorded for r in case["rows"]])
    worst = {}
    if not keep.all():
        rec = gc.ratios(got[~keep], ex["exact"][~keep], ex["bnd"][~keep])
        assert torch.isfinite(got[~keep].float()).all(), f"{kernel} {what}: non-finite output on a recorded regime"
        names = [r for r in case["rows"] if r in recorded]
        if not quiet:
            print(f"ENV {kernel} {what} RECORDED: " + "  ".join(f"{r} {x:.2f}" for r, x in gc.worst_per_regime(rec, names, case["chans"]).items()
                                                                 if not r.startswith("c:")))
    sub = dict(case, rows=[r for r in case["rows"] if r not in recorded])
    worst.update(gc.judge(kernel, what, got[keep], ex["exact"][keep], ex["bnd"][keep], sub, limit=limit,
                          rnd=ex["rnd"][keep] if half else None, show_rnd=ex["rnd"][keep], quiet=quiet))
    return worst


def check_const_rows(kernel, what, got, restated, rows):
    """the const rows (n = 0 exactly) must carry the restatement's bits"""
    c = const_rows(rows)
    if c.any():
        same = (got[c].view(torch.int16) == restated[c].view(torch.int16)) | ((got[c] == 0) & (restated[c] == 0))
        assert same.all(), f"{kernel} {what}: {int((~same).sum())} elements of const rows differ from h16(b')"


# ----------------------------------------------------------------------------- geometries
def rowgemm_geoms(tiles: int, ntr_tiles: int = 0, mt_ok: bool = True, mt4: bool = False):
    """the rule of test_gpu_rowgemm._geoms (the CPU file asserts that the two agree)"""
    out = []
    for mt in (1, 2, 4):
        if (mt == 2 and not mt_ok) or (mt == 4 and not mt4):
            continue
        for nt in (1, 2, 3, 4):
            if mt >= 2 and nt > 2:
                continue
            for nw in range(1, (5 if nt >= 3 else 8) + 1):
                if tiles % (nw * nt) == 0 and ntr_tiles % (nw * nt) == 0:
                    out.append((nw, nt, mt))
    return out


GEGLU_GEOMS_320 = ((8, 2, 2), (4, 2, 2), (5, 4, 1), (8, 1, 1), (4, 1, 2), (5, 2, 4), (8, 1, 4), (4, 2, 4), (5, 1, 4))

# ----------------------------------------------------------------------------- the cases (built once, shared, never modified)
_CASES = {}
B_, T_ = 3, 50                                       # M = 150: ragged, the 32-row tiles cross samples


def _affine(K, seed):
    Kp = gc.round_up(K, 10)
    gm, bt = nc.affine(Kp, seed)
    return gm[:K].contiguous(), bt[:K].contiguous()


def ln_case(K: int, Nout: int, *, geglu: bool = False, ws: bool = False, B: int = B_, T: int = T_, res: bool = False, seed: int = 100,
            regimes=None, ntr: int = 0):
    """LayerNorm + linear / GEGLU / q|k|V^T on planted rows, for rowgemm (two-pass) or wsgemm (fold)"""
    key = ("ln", K, Nout, geglu, ws, B, T, res, seed, regimes, ntr)
    if key not in _CASES:
        regimes_ = regimes or (FOLD_ROWS if ws else LN_ROWS)
        x, rows = plant_rows(B, T, K, regimes_, seed)
        w, bias, chans = plant_weights(Nout, K, seed + 1, big_bias=60.0 if geglu else 1000.0, geglu=geglu)
        gm, bt = _affine(K, seed + 2)
        fd = fold_pack(w, bias, gm, bt, geglu=geglu, ws=ws)
        if ws:
            wf = w.float() * gm.float()[None]
            fd["cs_unrounded"] = wf.sum(1)
        r = plant_residual(B * T, Nout, fd["b"], chans, seed + 3) if res else None
        _CASES[key] = dict(x=x, rows=rows, chans=chans, fd=fd, res=r, B=B, T=T, M=B * T, K=K, Nout=Nout, NoutO=Nout // 2 if geglu else Nout,
                           epi=1 if geglu else 0, pro="fold" if ws else 1, eps=EPS_LN, ntr=ntr, gn=None, key=key)
    return _CASES[key]


def gn_case(B: int, T: int, C: int, Nout: int, seed: int = 200):
    """GroupNorm(32) + linear on norm_cases.planted; the hotw channels pick one k in every group in turn"""
    key = ("gn", B, T, C, Nout, seed)
    if key not in _CASES:
        cpg = C // G
        x = nc.planted(B, T, C, G, seed).view(B * T, C)
        w, bias, chans = plant_weights(Nout, C, seed + 1, hot=[g * cpg + g % cpg for g in range(G)])
        gm, bt = _affine(C, seed + 2)
        fd = fold_pack(w, bias, gm, bt)
        rows = [f"s{b}" for b in range(B) for _ in range(T)]
        _CASES[key] = dict(x=x, rows=rows, chans=chans, fd=fd, res=None, B=B, T=T, M=B * T, K=C, Nout=Nout, NoutO=Nout, epi=0, pro=2,
                           eps=EPS_GN, ntr=0, gn=(B, T), key=key)
    return _CASES[key]


_EXPECT = {}


def expected(case, S: int = 1, form=None):
    """(`expect` result, restatement) of a case; cached"""
    k = (case["key"], S, form)
    if k not in _EXPECT:
        form_ = form or (("wsgemm", "staged") if case["pro"] == "fold" else ("rowgemm", "staged"))
        kw = dict(pro=case["pro"], eps=case["eps"], epi=case["epi"], res=case["res"], gn=case["gn"], S=S)
        ex = expect(case["x"], case["fd"], form=form_, rows=case["rows"], chans=case["chans"], **kw)
        _EXPECT[k] = (ex, restate(case["x"], case["fd"], **kw))
    return _EXPECT[k]


# cases 1 - 4: rowgemm
def rowgemm_ln_cases():
    """(case, geometries, mt4) -- K = 320: the row in registers; K = 1280, Nout = 64: through LDS (128 threads); K = 1280, Nout = 256 with
    8 waves: 16 lanes per row, in registers again; K = 64: the generic k loop"""
    out = []
    for res in (False, True):
        out.append((ln_case(320, 96, res=res), rowgemm_geoms(3, mt4=True)))
        out.append((ln_case(1280, 64, res=res, seed=110), rowgemm_geoms(2, mt_ok=False)))      # (64 rows of K = 1280 do not fit the LDS)
        out.append((ln_case(64, 96, res=res, seed=120), rowgemm_geoms(3)))
        out.append((ln_case(64, 64, res=res, seed=130), rowgemm_geoms(2)))
    out.append((ln_case(1280, 256, seed=140), [(8, 1, 1), (4, 2, 1), (4, 1, 1)]))
    return out


def rowgemm_geglu_cases():
    return [(ln_case(64, 512, geglu=True, seed=150), rowgemm_geoms(16)[::3]),
            (ln_case(320, 2560, geglu=True, seed=160), list(GEGLU_GEOMS_320))]


def rowgemm_gn_cases():
    return [(gn_case(3, 32, 320, 96), [g for g in rowgemm_geoms(3) if g[2] == 1]),
            (gn_case(2, 64, 64, 96, seed=210), [g for g in rowgemm_geoms(3) if g[2] in (1, 2)])]


def rowgemm_qkv_cases():
    """(B, T, C) = (3, 32, 64) and (2, 64, 320): Nout = 3 C, the last C packed rows leave as V^T with ldt = T + 8"""
    out = []
    for (B, T, C), seed in (((3, 32, 64), 170), ((2, 64, 320), 180)):
        case = ln_case(C, 3 * C, B=B, T=T, seed=seed, ntr=C)
        geoms = rowgemm_geoms(3 * C // 32, C // 32, mt_ok=(T % 64 == 0))[:10]
        out.append((case, [None] + geoms))
    return out


# cases 5, 6: wsgemm
def wsgemm_fold_cases():
    """(case, schedules (NW, NT, NL, S, ntw))"""
    a = ln_case(320, 160, ws=True, res=True, seed=300)
    b = ln_case(1280, 128, ws=True, res=True, seed=310)
    return [(a, [(5, 1, 1, 1, False), (5, 1, 2, 1, True), (1, 1, 1, 2, False), (5, 1, 2, 5, False)]),
            (b, [(4, 1, 1, 1, False), (2, 1, 2, 4, False), (2, 1, 2, 3, False), (2, 2, 1, 7, True)])]


def wsgemm_geglu_case():
    return ln_case(320, 32, geglu=True, ws=True, seed=320)


def wsgemm_qkv_case():
    """fold + V^T: T % 128 == 0 (a 128-token tile lies in one sample); split-K is refused with a transposed part"""
    return ln_case(320, 96, ws=True, B=2, T=128, seed=330, ntr=32)


# ----------------------------------------------------------------------------- op builders shared by the GPU file and the CPU dry run
FRONT = 16                                           # halfs of NaN in front of every guarded operand: keeps 16-byte alignment


def guarded(t2d, ld: int, off: int = FRONT, back: int = 64):
    """t2d [rows, cols] -> a flat buffer of NaN with row r at [off + r ld, off + r ld + cols)"""
    rows, cols = t2d.shape
    assert ld >= cols
    buf = torch.full((off + rows * ld + back,), float("nan"), dtype=t2d.dtype)
    buf[off:off + rows * ld].view(rows, ld)[:, :cols] = t2d
    return buf


def operands(case, dev):
    """x (and the residual) behind NaN guards with 8 NaN halfs in every row's gap, the packed layer, the exact accumulators"""
    fd = case["fd"]
    d = dict(x=guarded(case["x"], case["K"] + 8).to(dev), wp=fd["wp"].to(dev), bp=fd["bp"].to(dev),
             cs=None if fd["cs"] is None else fd["cs"].to(dev))
    if case["res"] is not None:
        d["res"] = guarded(case["res"], case["Nout"] + 8).to(dev)
    if case["pro"] == 2:
        d["acc"] = nc.exact_acc(case["x"].view(case["B"], case["T"], case["K"]), G).to(dev)
    return d


def out_buffers(case, dev):
    """(out prototype, V^T prototype or None, ldo, ldt): NaN-filled, ld = cols + 8"""
    nrm = case["NoutO"] - case["ntr"]
    ldo, ldt = nrm + 8, case["T"] + 8
    nan = lambda rows, ld: torch.full((FRONT + rows * ld + 64,), float("nan"), dtype=torch.float16, device=dev)
    return nan(case["M"], ldo), (nan(case["B"] * case["ntr"], ldt) if case["ntr"] else None), ldo, ldt


def rowgemm_op(L, case, d, out, vt, ldo, ldt, sched, order):
    K, ntr, T = case["K"], case["ntr"], case["T"]
    kw = dict(M=case["M"], K=K, Nout=case["Nout"], ldx=K + 8, ldo=ldo, bias=d["bp"], pro=case["pro"], eps=case["eps"], epi=case["epi"],
              x_off=FRONT, out_off=FRONT, sched=sched, order=order)
    if case["res"] is not None:
        kw.update(res=d["res"], ldr=case["Nout"] + 8, res_off=FRONT)
    if case["pro"] == 2:
        kw.update(T=T, G=G, gn_acc_ptr=d["acc"].data_ptr())
    if ntr:
        kw.update(T=T, out_t=vt[FRONT:], ntr=ntr, ldt=ldt, st=ntr * ldt)
    op, keep = L.rowgemm(d["x"], d["wp"], out, **kw)
    return op, keep + ((d["acc"],) if case["pro"] == 2 else ())


def wsgemm_bufs(L, case, sched, dev):
    NW, NT, _NL, S, _ntw = sched
    if S <= 1:
        return None, None
    nws, ncnt = L.wsgemm_sizes(case["M"], case["Nout"], NW, NT, S)
    return torch.full((nws,), float("nan"), dtype=F32, device=dev), torch.zeros(ncnt + 4, dtype=torch.int32, device=dev)


def wsgemm_op(L, case, d, out, vt, ldo, ldt, sched, ws, cnt):
    K, N, ntr = case["K"], case["Nout"], case["ntr"]
    kw = dict(M=case["M"], Nout=N, C1=K, ldx1=K + 8, ldo=ldo, bias=d["bp"], colsum=d["cs"], pro=1, eps=case["eps"], epi=case["epi"],
              x1_off=FRONT, out_off=FRONT, sched=sched)
    if case["res"] is not None:
        kw.update(res=d["res"], ldr=N + 8, res_off=FRONT)
    if ntr:
        kw.update(T=case["T"], out_t=vt[FRONT:], ntr=ntr, ldt=ldt, st=ntr * ldt)
    if ws is not None:
        kw.update(ws=ws, cnt=cnt, cnt_off=4)
    return L.wsgemm(d["x"], d["wp"], out, **kw)


def wsgemm_geglu_scheds(L, case):
    return [tuple(L.wsgemm_schedule(case["M"], case["K"], case["Nout"], 0, 1, 1)), (1, 1, 2, 2, False), (1, 1, 1, 5, True)]


def wsgemm_qkv_scheds(L, case):
    return [tuple(L.wsgemm_schedule(case["M"], case["K"], case["Nout"], case["ntr"], 0, 1)), (1, 1, 1, 1, False), (1, 1, 2, 1, True)]


# ----------------------------------------------------------------------------- 7, 8. rowchain (C = 320): the stages and their layers
CHAIN_C = 320
HEAD_KINDS = ("gn_qkv", "res_qkv", "gn_qkvT", "res_q")
HEAD_SHAPES = ((3, 32), (1, 64))
TAIL_SHAPES = ((3, 32), (1, 32))


def layer(Nout: int, K: int, seed: int, *, norm: bool = False, geglu: bool = False, zero_bias: bool = False, hot=None, big_bias: float = 1000.0):
    """a planted layer through the packer: fold_pack's dict + chans"""
    w, b, chans = plant_weights(Nout, K, seed, big_bias=big_bias, geglu=geglu, hot=hot)
    if zero_bias:
        b = torch.zeros_like(b)
    gm, bt = _affine(K, seed + 1) if norm else (None, None)
    fd = fold_pack(w, b, gm, bt, geglu=geglu)
    fd["chans"] = chans
    return fd


def sparse_rows(M: int, K: int, seed: int):
    """benign fp16 rows with every third row zero"""
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(seed), dtype=F64)
    x[::3] = 0.0
    return x.to(torch.float16)


def head_case(kind: str, B: int, T: int):
    """h = A(GroupNorm(x)) + bA, or A(x) + resA with bA = 0 and every third x row zero (h = resA, the planted rows, there);
    out = B(LayerNorm(h)) + bB over `passes` x C packed rows, the last pass as V^T for gn_qkvT"""
    key = ("head", kind, B, T)
    if key not in _CASES:
        C, M = CHAIN_C, B * T
        gnp, passes, trl = kind.startswith("gn"), (1 if kind == "res_q" else 3), kind == "gn_qkvT"
        seed = 400 + 10 * HEAD_KINDS.index(kind) + B
        if gnp:
            x = nc.planted(B, T, C, G, seed).view(M, C)
            fdA = layer(C, C, seed + 1, norm=True, hot=[g * (C // G) + g % (C // G) for g in range(G)], big_bias=30.0)
            resA, rows1 = None, [f"s{b}" for b in range(B) for _ in range(T)]
            rows2 = rows1
        else:
            x = sparse_rows(M, C, seed)
            fdA = layer(C, C, seed + 1, zero_bias=True)
            resA, names = plant_rows(B, T, C, LN_ROWS, seed + 2)
            rows1 = ["zero x" if m % 3 == 0 else "benign" for m in range(M)]
            rows2 = [names[m] if m % 3 == 0 else "mixed" for m in range(M)]
        fdB = layer(passes * C, C, seed + 3, norm=True)
        _CASES[key] = dict(kind=kind, B=B, T=T, M=M, C=C, gnp=gnp, passes=passes, trl=trl, x=x, resA=resA, fdA=fdA, fdB=fdB, rows1=rows1,
                           rows2=rows2, ncol=(passes - int(trl)) * C, key=key)
    return _CASES[key]


def head_stage1(case, x=None):
    """(expect result, restatement) of h from the inputs"""
    x = case["x"] if x is None else x
    kw = dict(pro=2, eps=EPS_GN, gn=(case["B"], case["T"])) if case["gnp"] else dict(pro=0, res=case["resA"])
    return (expect(x, case["fdA"], rows=case["rows1"], chans=case["fdA"]["chans"], **kw), restate(x, case["fdA"], **kw))


def head_stage2(case, h16, mutant=None, hf=None):
    """(expect result, restatement) of out | V^T as one [M, passes C] matrix from the stored h"""
    return (expect(h16, case["fdB"], pro=1, eps=EPS_LN, rows=case["rows2"], chans=case["fdB"]["chans"]),
            restate(h16, case["fdB"], pro=1, eps=EPS_LN, mutant=mutant, xf=hf))


def head_h32(case):
    """the fp32 value of h before its fp16 store (res kinds: the sum of the rounded GEMM output and the residual)"""
    fd = case["fdA"]
    assert not case["gnp"]
    return (case["x"].float() @ fd["W"].float().t() + fd["b"][None]).half().float() + case["resA"].float()


def tail_case(B: int, T: int):
    """h2 = to_out(a) + res1 with b_out = 0 and every third row of a zero (h2 = res1, the planted rows, there); hid = GEGLU(LN(h2));
    h3 = FF2(hid) + h2; out = proj_out(h3) + res2"""
    key = ("tail", B, T)
    if key not in _CASES:
        C, M = CHAIN_C, B * T
        seed = 500 + B
        res1, names = plant_rows(B, T, C, LN_ROWS, seed + 1)
        ff2 = layer(C, 4 * C, seed + 6, big_bias=100.0)
        _CASES[key] = dict(B=B, T=T, M=M, C=C, a=sparse_rows(M, C, seed), res1=res1,
                           res2=torch.randn(M, C, generator=torch.Generator().manual_seed(seed + 2), dtype=F64).to(torch.float16),
                           out=layer(C, C, seed + 3, zero_bias=True), ff1=layer(8 * C, C, seed + 4, norm=True, geglu=True, big_bias=60.0),
                           ff2=ff2, po=layer(C, C, seed + 8, big_bias=100.0),
                           rows1=["zero a" if m % 3 == 0 else "benign" for m in range(M)],
                           rows2=[names[m] if m % 3 == 0 else "mixed" for m in range(M)], key=key)
    return _CASES[key]


def tail_stage(case, i: int, prev, h2=None):
    """(expect result, restatement) of stage i = 1 .. 4 of the tail from the previous stage's fp16 output `prev` (stage 1: a); h2 is
    stage 3's residual"""
    rows = case["rows1"] if i == 1 else case["rows2"]
    fd, kw = {1: (case["out"], dict(pro=0, res=case["res1"])), 2: (case["ff1"], dict(pro=1, eps=EPS_LN, epi=1)),
              3: (case["ff2"], dict(pro=0, res=h2)), 4: (case["po"], dict(pro=0, res=case["res2"]))}[i]
    form = ("igemm", "staged") if i == 3 else ("rowgemm", "staged")
    return expect(prev, fd, form=form, rows=rows, chans=fd["chans"], **kw), restate(prev, fd, **kw)


def tail_packed(case, dev):
    pk = {}
    for name, k in (("out", "out"), ("ff1", "ff1"), ("ff2", "ff2"), ("po", "po")):
        pk["w_" + name], pk["b_" + name] = case[k]["wp"].to(dev), case[k]["bp"].to(dev)
    return pk


def head_ops(L, case, d, hout, out, vt, *, ld, ldo, ldt, fused: bool):
    """the head segment (fused) or the two rowgemm launches it replaces; d: x, resA (guarded, pitch ld), wA, bA, wB, bB, acc"""
    C, M, T, passes, trl = case["C"], case["M"], case["T"], case["passes"], case["trl"]
    tr = dict(out_t=vt[FRONT:], ldt=ldt, st=C * ldt) if trl else {}
    if fused:
        kw = dict(M=M, C=C, wA=d["wA"], bA=d["bA"], wB=d["wB"], bB=d["bB"], passes=passes, T=T, G=G, eps_gn=EPS_GN, eps_ln=EPS_LN, ldx=ld, ldh=ld,
                  ldo=ldo, **tr)
        if case["gnp"]:
            kw.update(gn_acc_ptr=d["acc"].data_ptr())
        else:
            kw.update(resA=d["resA"][FRONT:], ldrA=ld)
        op, keep = L.rowchain_head(d["x"][FRONT:], hout[FRONT:], out[FRONT:], **kw)
        return [(op, keep + (d.get("acc"), d["x"], hout, out, vt, d.get("resA")))]
    a = dict(M=M, K=C, Nout=C, ldx=ld, ldo=ld, bias=d["bA"], x_off=FRONT, out_off=FRONT)
    if case["gnp"]:
        a.update(pro=2, eps=EPS_GN, T=T, G=G, gn_acc_ptr=d["acc"].data_ptr())
    else:
        a.update(res=d["resA"], ldr=ld, res_off=FRONT)
    b = dict(M=M, K=C, Nout=passes * C, ldx=ld, ldo=ldo, bias=d["bB"], pro=1, eps=EPS_LN, T=T, x_off=FRONT, out_off=FRONT)
    if trl:
        b.update(ntr=C, **tr)
    op1, k1 = L.rowgemm(d["x"], d["wA"], hout, **a)
    op2, k2 = L.rowgemm(hout, d["wB"], out, **b)
    return [(op1, k1 + (d.get("acc"),)), (op2, k2)]


def head_operands(case, dev, ld):
    d = dict(x=guarded(case["x"], ld).to(dev), wA=case["fdA"]["wp"].to(dev), bA=case["fdA"]["bp"].to(dev), wB=case["fdB"]["wp"].to(dev),
             bB=case["fdB"]["bp"].to(dev))
    if case["gnp"]:
        d["acc"] = nc.exact_acc(case["x"].view(case["B"], case["T"], case["C"]), G).to(dev)
    else:
        d["resA"] = guarded(case["resA"], ld).to(dev)
    return d


def nan_buf(rows: int, ld: int, dev, dtype=torch.float16):
    return torch.full((FRONT + rows * ld + 64,), float("nan"), dtype=dtype, device=dev)


def tail_operands(case, dev, ld):
    d = dict(a=guarded(case["a"], ld).to(dev), res1=guarded(case["res1"], ld).to(dev), res2=guarded(case["res2"], ld).to(dev),
             w2l=None, b2=case["ff2"]["b"].to(dev), **tail_packed(case, dev))
    return d


def tail_unfused_ops(L, case, d, h2, hid, h3, o4, ld):
    """the four launches the chain replaces: row GEMM + residual, row GEMM with LayerNorm + GEGLU, implicit GEMM + residual, row GEMM +
    residual; every buffer guarded (FRONT halfs in front, pitch ld, hid: 4 C + 8)"""
    C, M = case["C"], case["M"]
    if d["w2l"] is None:
        d["w2l"] = L.pack_linear(case["ff2"]["W"].to(d["a"].device))
    io = dict(x_off=FRONT, out_off=FRONT)
    return [L.rowgemm(d["a"], d["w_out"], h2, M=M, K=C, Nout=C, ldx=ld, ldo=ld, bias=d["b_out"], res=d["res1"], ldr=ld, res_off=FRONT, **io),
            L.rowgemm(h2, d["w_ff1"], hid, M=M, K=C, Nout=8 * C, ldx=ld, ldo=4 * C + 8, bias=d["b_ff1"], pro=1, eps=EPS_LN, epi=1, **io),
            L.igemm(hid, d["w2l"], h3, M=M, Nout=C, C1=4 * C, ldx1=4 * C + 8, CinP=d["w2l"].shape[1], ldo=ld, bias=d["b2"], res=h2, ldr=ld,
                    tile=2, variant=1, x1_off=FRONT, out_off=FRONT, res_off=FRONT),
            L.rowgemm(h3, d["w_po"], o4, M=M, K=C, Nout=C, ldx=ld, ldo=ld, bias=d["b_po"], res=d["res2"], ldr=ld, res_off=FRONT, **io)]


def tail_chain_op(L, case, d, out, ld):
    pk = {k: d[k] for k in ("w_out", "b_out", "w_ff1", "b_ff1", "w_ff2", "b_ff2", "w_po", "b_po")}
    op, keep = L.rowchain(d["a"][FRONT:], d["res1"][FRONT:], d["res2"][FRONT:], out[FRONT:], M=case["M"], C=case["C"], eps=EPS_LN, lda=ld, ldr1=ld,
                          ldr2=ld, ldo=ld, **pk)
    return op, keep + (d["a"], d["res1"], d["res2"], out)


# ----------------------------------------------------------------------------- 9. clip_linear
CLIP_KEY = gc.lin_key(C1=192, Nout=160, seed=50)     # K % 192 == 0: the smallest K the kernel takes; gemm_cases' planted rows and channels
C_EXP, LIP_QGELU = 4.0, 1.1


def clip_cases():
    """plain: bias with each epilogue (none, quick_gelu, the fp32 residual stream); LayerNorm form at K = 192 (one wave) and 384 (two)"""
    if "clip" not in _CASES:
        from live2diff_amd import ops
        g = gc.case_of(CLIP_KEY)
        out = []
        for epi in (0, 1, 2):
            out.append(dict(name=f"plain epi{epi}", ln=False, x=g["x1"], w=g["w"], bias=g["bias"], gamma=None, beta=None, epi=epi,
                            res32=g["res"].float() * 1.0009765625 if epi == 2 else None, rows=g["rows"], chans=g["chans"], eps=EPS_LN))
        for K, seed in ((192, 600), (384, 610)):
            x, rows = plant_rows(B_, T_, K, LN_ROWS, seed)
            w, bias, chans = plant_weights(160, K, seed + 1)
            gm, bt = _affine(K, seed + 2)
            for epi in (0, 1):
                out.append(dict(name=f"LN K{K} epi{epi}", ln=True, x=x.float(), w=w, bias=bias, gamma=gm.float(), beta=bt.float(), epi=epi,
                                res32=None, rows=rows, chans=chans, eps=EPS_LN))
        for c in out:
            c["M"], c["K"] = c["x"].shape
            c["Nout"] = c["w"].shape[0]
            c["NW"], c["MT"] = ops.clip_linear_schedule(c["M"], c["K"])
        _CASES["clip"] = out
    return _CASES["clip"]


def _qgelu(v):
    return v / (1.0 + torch.exp(-1.702 * v))


def clip_expect(c):
    """`expect` for clip_linear (module docstring)"""
    if "ex" in c:
        return c["ex"]
    W, K, M, S = c["w"].double(), c["K"], c["M"], c["NW"]
    extra = rn = n = None
    if c["ln"]:
        n, dn32 = ln_two_pass(c["x"], c["eps"], c_r=2 * E32, fp32_part=True)
        g, b = c["gamma"].double()[None], c["beta"].double()[None]
        a = n * g + b
        da = U * a.abs() + SUB + (dn32 * g.abs() + E32 * a.abs()) * (1 + U)
        extra, rn = da @ W.abs().t(), (U * a.abs() + SUB) @ W.abs().t()
        y, A = a @ W.t(), a.abs() @ W.abs().t() + extra
    else:
        x = c["x"].double()
        y, A = x @ W.t(), x.abs() @ W.abs().t()
    case = dict(M=M, Nout=c["Nout"], K=K, taps=1, bias=c["bias"], rows_per_bias=M, res=c["res32"], rows=c["rows"], chans=c["chans"])
    if c["epi"] == 1:
        b = c["bias"].double()[None]
        pre = y + b
        adds = E32 * (y.abs() + b.abs())
        e0 = (K + S + 2) * E32 * A + adds + (0.0 if extra is None else extra)
        exact = _qgelu(pre)
        e1 = LIP_QGELU * e0 + (C_EXP + 1.702 * pre.abs() + 4) * E32 * exact.abs()
        rnd = U * exact.abs() + SUB
        bnd, rnd = e1 * (1 + U) + rnd, rnd + LIP_QGELU * adds
    else:
        exact, bnd, rnd = gc.exact_and_bound(case, y, A, res=c["epi"] == 2, S=S, form=("skinny", "f32" if c["epi"] == 2 else "f16"), extra=extra)
    if rn is not None:
        rnd = rnd + LIP_QGELU * rn * (1 + 2 * U)
    c["ex"] = dict(exact=exact, bnd=bnd, rnd=rnd, n=n, case=case, y=y)
    return c["ex"]


def clip_restate(c):
    """clip.hip in plain fp32 torch: per-wave partial sums over K / NW added in wave order, bias, epilogue"""
    W = c["w"].float()
    if c["ln"]:
        x, K = c["x"], c["K"]
        mean = x.sum(1, keepdim=True) / K
        d = x - mean
        rstd = 1.0 / torch.sqrt((d * d).sum(1, keepdim=True) / K + torch.tensor(c["eps"], dtype=F32))
        a = torch.addcmul(c["beta"][None], d * rstd, c["gamma"][None]).half().float()
    else:
        a = c["x"].float()
    kw = c["K"] // c["NW"]
    v = sum(a[:, i * kw:(i + 1) * kw] @ W[:, i * kw:(i + 1) * kw].t() for i in range(c["NW"])) + c["bias"][None]
    if c["epi"] == 2:
        return c["res32"] + v
    return (_qgelu(v.double()).float() if c["epi"] == 1 else v).half()


def clip_op(L, c, x_buf, w_packed, bias, out_buf, gamma, beta, ld, ldo):
    return L.clip_linear(x_buf[FRONT:], w_packed, out_buf[FRONT:], M=c["M"], K=c["K"], Nout=c["Nout"], ldx=ld, ldo=ldo, bias=bias, gamma=gamma,
                         beta=beta, epi=c["epi"], eps=c["eps"])
