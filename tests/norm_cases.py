"""Planted-statistics activations for the GroupNorm / LayerNorm envelope tests (test_norm_envelope_cpu.py, test_gpu_norm_envelope.py).

Every GroupNorm of the frame takes its statistics from single-pass sums: the producer accumulates sum x and sum x^2 of what it stores in
fp32 per tile, flushes them as integers in units of 2^-20 and 2^-12 (csrc/common.h l2d_gn_flush) and the consumer forms
var = q / n - mean^2 in fp32.  Two things can go wrong there that iid N(0, 1) data never shows: the subtraction cancels like
(mean / std)^2, and the 2^-12 quantum of sum x^2 is coarse for a group whose energy per flush is a few hundred quanta.  `planted` gives
every (sample, group) its own regime of (mean, std), `group_errors` judges every (sample, group) on its own, `acc_bounds` bounds the two
accumulators per group from the arithmetic, and `emulate` restates the documented arithmetic in plain torch, so that the envelope asserted
on the GPU is one the arithmetic itself stays inside.  The envelope comes from the arithmetic: per-group (mean / std) of real SD-1.5
activations has not been measured in this project.

The builders at the end construct every producer and fused consumer with identity weights (centre-tap identity for the convs): a
producer then stores the planted tensor bit for bit, and output channel c of a fused consumer is the normalised input channel c.  They
take the device as a parameter: the CPU suite builds the same ops in dry-run and checks that every producer accepts the statistics request.
"""
import torch
import torch.nn.functional as F

# (mean, std) of mean + std * z; the three constructions are in `planted`
MU_SIGMA = {"benign": (0.0, 1.0), "r10": (10.0, 1.0), "r30": (30.0, 1.0), "r100": (-100.0, 1.0), "small": (0.0, 0.02),
            "small_off": (0.2, 0.02), "large": (0.0, 100.0), "large_off": (3000.0, 100.0),
            "s0.01": (0.0, 0.01), "s0.003": (0.0, 0.003), "r300": (300.0, 1.0)}
ASSERTED = ("benign", "r10", "r30", "r100", "small", "small_off", "large", "large_off", "const", "outlier", "ramp")
RECORDED = ("s0.01", "s0.003", "r300")              # measured and printed, finiteness asserted: see test_norm_envelope_cpu.py
REGIMES = ASSERTED + RECORDED                       # 14: with G = 32 every regime occurs at least twice per sample
CONST = 7.3

# the shape of the GPU tests: the smallest one that all seven producers and five consumers accept (rowchain is C = 320 only, cconv
# needs H % 8 and W % 16, igemm's 128-row tile needs T % 128); cpg = 10 straddles 8-channel vectors and 64-channel tiles
B, H, W, T, C, G = 2, 16, 16, 256, 320, 32
EPS_RESNET, EPS_TRANSFORMER = 1e-5, 1e-6
TOL = 2e-3                                          # the per-kernel bound, here per (sample, group)
TOL_R100 = 2e-2                                     # |mean| / std = 100: what the project accepts there for the LayerNorm fold


def tol_of(regime: str) -> float:
    """2e-3, except r100: the emulation of the documented arithmetic does not stay within half of 2e-3 there (1.3e-3 at eps 1e-5,
    test_norm_envelope_cpu.py), so that regime is held to the 2e-2 of test_wsgemm_layernorm_fold_rows_with_a_large_mean"""
    return TOL_R100 if regime == "r100" else TOL


def regime_of(b: int, g: int) -> str:
    """the list rotated by one per sample: two samples never share a layout, so a wrong sample index shows"""
    return REGIMES[(g + b) % len(REGIMES)]


def regime_table(nb: int, ng: int):
    return [[regime_of(b, g) for g in range(ng)] for b in range(nb)]


def planted(nb: int, nt: int, nc: int, ng: int, seed: int) -> torch.Tensor:
    """fp16 [nb, nt, nc]: group g of sample b follows regime_of(b, g)"""
    gen = torch.Generator().manual_seed(seed)
    cpg = nc // ng
    assert cpg * ng == nc and cpg >= 2
    z = torch.randn(nb, nt, ng, cpg, generator=gen, dtype=torch.float64)
    x = torch.empty_like(z)
    t = torch.arange(nt, dtype=torch.float64)[:, None]
    for b in range(nb):
        for g in range(ng):
            name, zz = regime_of(b, g), z[b, :, g]
            if name in MU_SIGMA:
                mu, sg = MU_SIGMA[name]
                v = mu + sg * zz
            elif name == "const":
                v = torch.full_like(zz, CONST)
            elif name == "outlier":                 # cpg - 1 channels N(0, 1) and one N(60, 1)
                v = zz.clone()
                v[:, -1] += 60.0
            else:                                   # token ramp: the per-tile partial sums differ by orders of magnitude
                assert name == "ramp"
                v = 8.0 * t / nt - 4.0 + 0.05 * zz
            x[b, :, g] = v
    return x.reshape(nb, nt, nc).to(torch.float16)


def planted_rows(rows: int, nc: int, seed: int, regimes=REGIMES) -> torch.Tensor:
    """fp16 [rows, nc] for the LayerNorm paths: row m follows regimes[m % len(regimes)] (a row is laid out as nc / 10 'tokens' of 10
    'channels': the outlier is every tenth element, the ramp runs along the row)"""
    assert nc % 10 == 0
    full = planted(1, nc // 10, 10 * len(REGIMES), len(REGIMES), seed)[0].view(nc // 10, len(REGIMES), 10).permute(1, 0, 2).reshape(len(REGIMES), nc)
    idx = [REGIMES.index(regimes[m % len(regimes)]) for m in range(rows)]
    out = full[idx].clone()
    # (rows of one regime differ: roll them by the row index, which keeps every row's statistics)
    for m in range(rows):
        out[m] = torch.roll(out[m], 10 * (m // len(regimes)))
    return out.contiguous()


def row_regimes(rows: int, regimes=REGIMES):
    return [regimes[m % len(regimes)] for m in range(rows)]


def reference(x: torch.Tensor, ng: int, gamma, beta, eps: float, silu: bool = False) -> torch.Tensor:
    """fp64 GroupNorm (+ SiLU) of the fp16 tensor [nb, nt, nc]"""
    y = F.group_norm(x.double().permute(0, 2, 1), ng, gamma.double(), beta.double(), eps).permute(0, 2, 1)
    return F.silu(y) if silu else y


def reference_rows(x: torch.Tensor, gamma, beta, eps: float) -> torch.Tensor:
    return F.layer_norm(x.double(), (x.shape[-1],), gamma.double(), beta.double(), eps)


def group_errors(out: torch.Tensor, ref: torch.Tensor, ng: int) -> torch.Tensor:
    """[nb, ng] float64: RMS of out - ref over each (sample, group), in units of the RMS of ref over the WHOLE tensor (the reference
    of the constant group is just beta, so a group's own RMS cannot serve as the denominator)"""
    nb, nt, nc = ref.shape
    d = (out.double().cpu().reshape(nb, nt, ng, nc // ng) - ref.double().cpu().reshape(nb, nt, ng, nc // ng)) ** 2
    return d.mean((1, 3)).sqrt() / ref.double().pow(2).mean().sqrt()


def row_errors(out: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """[rows] float64: the same per row"""
    d = (out.double().cpu() - ref.double().cpu()) ** 2
    return d.mean(1).sqrt() / ref.double().pow(2).mean().sqrt()


def exact_acc(x: torch.Tensor, ng: int) -> torch.Tensor:
    """int64 [nb, ng, 2]: the accumulators a producer with exact sums would leave (fp64 sums, rounded once to the two quanta)"""
    nb, nt, nc = x.shape
    xs = x.double().view(nb, nt, ng, nc // ng)
    return torch.stack([(xs.sum((1, 3)) * 2 ** 20).round(), ((xs ** 2).sum((1, 3)) * 2 ** 12).round()], -1).to(torch.int64)


def acc_bounds(stored: torch.Tensor, ng: int, cpg: int, choff: int = 0, tokens_per_flush: int = 32, max_flush_tokens: int = 128,
               channel_tile: int = 64):
    """Rigorous per-group bounds on the two fixed-point accumulators of one consumer (ng groups of cpg channels; the stored tensor
    [nb, nt, nc] occupies channels [choff, choff + nc) of the consumer's axis) against fp64 sums over the tensor the producer stored.
    Returns (s, q, s_bound, q_bound), each [nb, ng] float64, with
        |S / 2^20 - sum x|   <= n_f 2^-21 + n 2^-24 sum |x|
        |Q / 2^12 - sum x^2| <= n_f 2^-13 + (n + 1) 2^-24 sum x^2
    n_f = flush pieces of the group: every producer flushes per (token tile, channel tile) with token tiles of at least 32 tokens and
    channel tiles that are multiples of 64 channels, so n_f <= (nt / 32) (1 + 64-channel boundaries the group crosses); each flush
    rounds once to the quantum (half a quantum).  (rowgemm / wsgemm tiles of 32 NW NT channels that are no multiple of 64 are 160
    wide in every schedule the tests use; 160 is a group boundary for every group size in use: 10, 20, 40, 80.)  n = most elements one flush sums in fp32: no producer's tile holds more than 128
    tokens (igemm 128 x 128, cconv 8 x 16 pixels, wsgemm 128), so n <= 128 x the group's channels in this tensor; a fp32 sum of n
    terms in any order is within (n - 1) 2^-24 sum |x| of the exact one, and the square of an fp16 value is exact in fp32 (the + 1
    covers a fused or unfused product all the same).  A group the tensor does not touch must stay exactly zero."""
    nb, nt, nc = stored.shape
    assert nt % tokens_per_flush == 0
    xd = stored.double().cpu()
    s, q = torch.zeros(nb, ng, dtype=torch.float64), torch.zeros(nb, ng, dtype=torch.float64)
    sb, qb = torch.zeros(nb, ng, dtype=torch.float64), torch.zeros(nb, ng, dtype=torch.float64)
    for g in range(ng):
        lo, hi = max(g * cpg, choff) - choff, min((g + 1) * cpg, choff + nc) - choff        # channels of the stored tensor
        if hi <= lo:
            continue
        part = xd[:, :, lo:hi]
        crossings = (hi - 1) // channel_tile - lo // channel_tile
        n_f = (nt // tokens_per_flush) * (1 + crossings)
        n = max_flush_tokens * (hi - lo)
        s[:, g], q[:, g] = part.sum((1, 2)), (part ** 2).sum((1, 2))
        sb[:, g] = n_f * 2.0 ** -21 + n * 2.0 ** -24 * part.abs().sum((1, 2))
        qb[:, g] = n_f * 2.0 ** -13 + (n + 1) * 2.0 ** -24 * q[:, g]
    return s, q, sb, qb


def check_acc(acc: torch.Tensor, stored: torch.Tensor, ng: int, cpg: int, choff: int = 0, what: str = ""):
    """every group of both accumulators (int64 [nb, ng, 2]) within acc_bounds"""
    s, q, sb, qb = acc_bounds(stored, ng, cpg, choff)
    a = acc.cpu().double()
    es, eq = (a[..., 0] / 2 ** 20 - s).abs(), (a[..., 1] / 2 ** 12 - q).abs()
    bad_s, bad_q = (es > sb).nonzero().tolist(), (eq > qb).nonzero().tolist()
    assert not bad_s, f"{what}: sum x off in (sample, group) {bad_s[:4]}: error {es[tuple(bad_s[0])]:.3e} > bound {sb[tuple(bad_s[0])]:.3e}"
    assert not bad_q, f"{what}: sum x^2 off in (sample, group) {bad_q[:4]}: error {eq[tuple(bad_q[0])]:.3e} > bound {qb[tuple(bad_q[0])]:.3e}"


def emulate_acc(x: torch.Tensor, ng: int, tokens_per_flush: int = 32, channel_tile: int = 64) -> torch.Tensor:
    """int64 [nb, ng, 2]: the producers' documented arithmetic -- per flush piece (tokens_per_flush tokens x the group's channels
    inside one channel tile) sequential fp32 sums (per channel over the tokens, then over the channels), each rounded to its quantum,
    exact integer adds"""
    nb, nt, nc = x.shape
    cpg, tpf = nc // ng, tokens_per_flush
    assert nt % tpf == 0
    xf = x.float().view(nb, nt // tpf, tpf, nc)
    cs = torch.zeros(nb, nt // tpf, nc, dtype=torch.float32)
    cq = torch.zeros_like(cs)
    for i in range(tpf):
        v = xf[:, :, i]
        cs = cs + v
        cq = cq + v * v
    acc = torch.zeros(nb, ng, 2, dtype=torch.int64)
    for g in range(ng):
        c = g * cpg
        while c < (g + 1) * cpg:
            e = min((g + 1) * cpg, (c // channel_tile + 1) * channel_tile)
            s = torch.zeros(nb, nt // tpf, dtype=torch.float32)
            q = torch.zeros_like(s)
            for ch in range(c, e):
                s = s + cs[:, :, ch]
                q = q + cq[:, :, ch]
            acc[:, g, 0] += (s.double() * 2 ** 20).round().to(torch.int64).sum(1)
            acc[:, g, 1] += (q.double() * 2 ** 12).round().to(torch.int64).sum(1)
            c = e
    return acc


def decode(x: torch.Tensor, acc: torch.Tensor, ng: int, gamma, beta, eps: float, silu: bool = False) -> torch.Tensor:
    """the consumers' documented arithmetic on integer accumulators: double -> float, mean = s inv, var = max(q inv - mean^2, 0),
    rsqrt(var + eps), y = x (rstd gamma) + (beta - mean rstd gamma) in fp32, fp16 output"""
    nb, nt, nc = x.shape
    cpg = nc // ng
    f32 = torch.float32
    s, q = (acc[..., 0].double() / 2 ** 20).to(f32), (acc[..., 1].double() / 2 ** 12).to(f32)
    inv = torch.tensor(1.0, dtype=f32) / (torch.tensor(float(nt), dtype=f32) * torch.tensor(float(cpg), dtype=f32))
    mean = s * inv
    var = (q * inv - mean * mean).clamp_min(0.0)
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=f32))
    gi = torch.arange(nc) // cpg
    sc = rstd[:, gi] * gamma.float()[None]
    sh = beta.float()[None] - mean[:, gi] * sc
    y = x.float() * sc[:, None] + sh[:, None]
    if silu:
        y = y / (1.0 + torch.exp(-y))
    return y.to(torch.float16)


def emulate(x: torch.Tensor, ng: int, gamma, beta, eps: float, silu: bool = False, tokens_per_flush: int = 32, channel_tile: int = 64):
    return decode(x, emulate_acc(x, ng, tokens_per_flush, channel_tile), ng, gamma, beta, eps, silu)


def affine(nc: int, seed: int = 3):
    """(gamma, beta) fp16 near (1, 0): the whole-tensor RMS of the reference, the unit of the error, is then about 1"""
    gen = torch.Generator().manual_seed(seed)
    return (1 + 0.1 * torch.randn(nc, generator=gen)).half(), (0.1 * torch.randn(nc, generator=gen)).half()


def _rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(torch.float16)


def identity_conv(nc: int) -> torch.Tensor:
    w = torch.zeros(nc, nc, 3, 3, dtype=torch.float16)
    w[:, :, 1, 1] = torch.eye(nc, dtype=torch.float16)
    return w


# ----------------------------------------------------------------------------- producers: one per flush site
PRODUCERS_320 = ("igemm128", "igemm64", "igemm_splitk", "igemm_splitk_fused", "rowgemm", "wsgemm", "wsgemm_splitk", "wsgemm3x3", "pconv",
                 "cconv_1x4", "rowchain")
PRODUCERS_640 = ("rowgemm", "cconv_2x2_splitk")      # rowgemm's generic k loop (K = 320 is a straight-line one); cconv's 128-channel tile


def build_producer(L, name: str, x: torch.Tensor, dev, nan=float("nan")):
    """(op, keep, out) of the launch `name` that stores x [nb, nt, nc] (the convs: 16 x 16 pixels per sample) unchanged into `out` [nb * nt, nc].
    Split-K slabs are NaN-poisoned as the kernels' own tests do; `out` starts as NaN."""
    nb, nt, nc = x.shape
    hh, ww = H, W
    assert nt == hh * ww or not ("conv" in name or "3x3" in name)
    M = nb * nt
    xd = x.reshape(M, nc).contiguous().to(dev)
    out = torch.full((M, nc), nan, dtype=torch.float16, device=dev)
    eye = torch.eye(nc, dtype=torch.float16)
    if name.startswith("igemm"):
        if "splitk" in name:                        # K = 8 C with W = [I | 0 ...] and random data in the dead columns
            fused, S = name.endswith("fused"), 4
            tile = 1 if fused else 2
            xin = torch.cat([x.reshape(M, nc), _rnd(M, 7 * nc, seed=71)], 1).to(dev)
            wp = L.pack_linear(torch.cat([eye, torch.zeros(nc, 7 * nc, dtype=torch.float16)], 1).to(dev))
            n_ws, n_cnt = L.splitk_sizes(M, nc, S, 1, tile) if fused else (S * M * nc, 0)
            ws = torch.full((n_ws,), nan, dtype=torch.float32, device=dev)
            cnt = torch.zeros(n_cnt, dtype=torch.int32, device=dev) if fused else None
            op, keep = L.igemm(xin, wp, out, M=M, Nout=nc, C1=8 * nc, ldx1=8 * nc, CinP=wp.shape[1], ldo=nc, splitk=S, tile=tile, ws=ws,
                               variant=1, cnt=cnt)
        else:
            wp = L.pack_linear(eye.to(dev))
            op, keep = L.igemm(xd, wp, out, M=M, Nout=nc, C1=nc, ldx1=nc, CinP=wp.shape[1], ldo=nc, tile=(1 if name == "igemm128" else 2),
                               variant=1)
    elif name == "rowgemm":
        wp, _ = L.pack_rowgemm(eye.to(dev))
        op, keep = L.rowgemm(xd, wp, out, M=M, K=nc, Nout=nc, ldx=nc, ldo=nc)
    elif name in ("wsgemm", "wsgemm_splitk"):
        wp, _, _ = L.pack_wsgemm(eye.to(dev))
        sched = (5, 1, 1, 1, False) if name == "wsgemm" else (2, 1, 2, 4, False)
        kw = {}
        if sched[3] > 1:
            n_ws, n_cnt = L.wsgemm_sizes(M, nc, sched[0], sched[1], sched[3])
            kw = dict(ws=torch.full((n_ws,), nan, dtype=torch.float32, device=dev), cnt=torch.zeros(n_cnt, dtype=torch.int32, device=dev))
        op, keep = L.wsgemm(xd, wp, out, M=M, Nout=nc, C1=nc, ldx1=nc, ldo=nc, T=nt, sched=sched, **kw)
    elif name == "wsgemm3x3":
        wp = L.pack_wsgemm_conv3x3(identity_conv(nc).to(dev))
        op, keep = L.wsgemm(xd, wp, out, M=M, Nout=nc, C1=nc, ldx1=nc, ldo=nc, taps=9, B=nb, H=hh, W=ww, T=nt, sched=(5, 1, 1, 1, False))
    elif name == "pconv":
        wp = L.pack_conv3x3(identity_conv(nc).to(dev))
        op, keep = L.pconv(xd, wp, out, B=nb, H=hh, W=ww, C1=nc, ldx1=nc, CinP=nc, Nout=nc, ldo=nc, patch=(8, 8))
    elif name.startswith("cconv"):
        sched = (1, 4, 2, 1) if name == "cconv_1x4" else (2, 2, 1, 3)
        CG, KG, _, S = sched
        wp = L.pack_cconv(identity_conv(nc).to(dev), KG)
        ws = cnt = None
        if S > 1:
            n_ws, n_cnt = L.cconv_sizes(nb, hh, ww, nc, CG, S)
            ws = torch.full((n_ws,), nan, dtype=torch.float32, device=dev)
            cnt = torch.zeros(n_cnt + 3, dtype=torch.int32, device=dev)
        op, keep = L.cconv(xd, wp, out, B=nb, H=hh, W=ww, C1=nc, ldx1=nc, Nout=nc, ldo=nc, KG=KG, sched=sched, ws=ws, cnt=cnt, cnt_off=3)
    elif name == "rowchain":                        # zero proj_out weights and bias: out = res2
        assert nc == 320
        gm, bt = affine(nc, seed=72)
        pk = dict(zip(("w_out", "b_out"), L.pack_rowgemm(_rnd(nc, nc, seed=73, scale=nc ** -0.5).to(dev), torch.zeros(nc, device=dev))))
        pk.update(zip(("w_ff1", "b_ff1"), L.pack_rowgemm(_rnd(8 * nc, nc, seed=74, scale=nc ** -0.5).to(dev), torch.zeros(8 * nc, device=dev),
                                                           gm.to(dev), bt.to(dev), geglu=True)))
        pk.update(zip(("w_ff2", "b_ff2"), L.pack_rowgemm(_rnd(nc, 4 * nc, seed=75, scale=(4 * nc) ** -0.5).to(dev), torch.zeros(nc, device=dev))))
        pk.update(zip(("w_po", "b_po"), L.pack_rowgemm(torch.zeros(nc, nc, dtype=torch.float16, device=dev), torch.zeros(nc, device=dev))))
        op, keep = L.rowchain(_rnd(M, nc, seed=76).to(dev), _rnd(M, nc, seed=77).to(dev), xd, out, M=M, C=nc, eps=1e-5, **pk)
    else:
        raise KeyError(name)
    return op, keep, out


def consumers_of(nc: int):
    """the two consumers every producer case registers: its own GroupNorm (choff 0) and the upper half of a 2 nc-wide concat"""
    return (dict(cpg=nc // G, choff=0), dict(cpg=2 * nc // G, choff=nc))


# ----------------------------------------------------------------------------- fused consumers, identity weights
def build_consumer(L, name: str, x: torch.Tensor, acc: torch.Tensor, gamma, beta, eps: float, dev):
    """(op, keep, out, silu) of the fused consumer `name` over x [nb, nt, nc] on `dev` with the statistics in acc (int64 [nb, G, 2] on
    `dev`): out [nb * nt, nc] = GroupNorm(x) (+ SiLU where the kernel fuses it)"""
    nb, nt, nc = x.shape
    M = nb * nt
    xd = x.reshape(M, nc).to(dev)
    gd, bd = gamma.to(dev), beta.to(dev)
    out = torch.full((M, nc), float("nan"), dtype=torch.float16, device=dev)
    eye = torch.eye(nc, dtype=torch.float16, device=dev)
    if name in ("gn_apply", "gn_apply_silu"):
        silu = name.endswith("silu")
        op, keep = L.gn_apply(xd, None, gd, bd, out, B=nb, T=nt, C1=nc, ld1=nc, G=G, nchunk=0, eps=eps, silu=silu, acc_ptr=acc.data_ptr())
    elif name == "rowgemm_pro2":
        silu = False
        wp, bp = L.pack_rowgemm(eye, torch.zeros(nc, device=dev), gd, bd)
        op, keep = L.rowgemm(xd, wp, out, M=M, K=nc, Nout=nc, ldx=nc, ldo=nc, bias=bp, pro=2, eps=eps, T=nt, G=G, gn_acc_ptr=acc.data_ptr())
    elif name == "rowchain_head":                   # judged on hout
        silu = False
        wpa, bpa = L.pack_rowgemm(eye, torch.zeros(nc, device=dev), gd, bd)
        gl, btl = affine(nc, seed=81)
        wpb, bpb = L.pack_rowgemm(_rnd(nc, nc, seed=82, scale=nc ** -0.5).to(dev), None, gl.to(dev), btl.to(dev))
        o2 = torch.zeros(M, nc, dtype=torch.float16, device=dev)
        op, keep = L.rowchain_head(xd, out, o2, M=M, C=nc, wA=wpa, bA=bpa, wB=wpb, bB=bpb, passes=1, T=nt, G=G, eps_gn=eps, eps_ln=1e-5,
                                   ldo=nc, gn_acc_ptr=acc.data_ptr())
    elif name.startswith("cconv_pro"):
        silu = True
        sched = (1, 4, 2, 1) if name == "cconv_pro_1x4" else (2, 2, 1, 3)
        CG, KG, _, S = sched
        wp = L.pack_cconv(identity_conv(nc).to(dev), KG)
        ws = cnt = None
        if S > 1:
            n_ws, n_cnt = L.cconv_sizes(nb, H, W, nc, CG, S)
            ws = torch.full((n_ws,), float("nan"), dtype=torch.float32, device=dev)
            cnt = torch.zeros(n_cnt + 3, dtype=torch.int32, device=dev)
        op, keep = L.cconv(xd, wp, out, B=nb, H=H, W=W, C1=nc, ldx1=nc, Nout=nc, ldo=nc, KG=KG, sched=sched, ws=ws, cnt=cnt, cnt_off=3,
                           gn_acc_ptr=acc.data_ptr(), gn_gamma=gd, gn_beta=bd, gn_G=G, gn_eps=eps)
    else:
        raise KeyError(name)
    return op, keep + (acc,), out, silu


CONSUMERS_320 = ("gn_apply", "gn_apply_silu", "rowgemm_pro2", "rowchain_head", "cconv_pro_1x4")
CONSUMERS_640 = ("gn_apply_silu", "rowgemm_pro2", "cconv_pro_2x2_splitk")
