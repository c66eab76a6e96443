"""-m gpu: the output stores of the frame's kernels (csrc/common.h l2d_st8 / l2d_st8_wt and the 4- / 8-byte epilogue paths),
one smallest shape per store site.  The cache policy of a store cannot change a value, so every case asks three things: (1) the
result against the fp32 reference at the tolerance that family's own test file uses, (2) a second run torch.equal to the first,
(3) the bytes AROUND the output untouched -- the output lives inside a buffer filled with a sentinel: guard lines before the
first and behind the last row, and columns beyond N in a wider ldo (a tail that shares a cache line with the 16-byte stores).
Outputs whose rows or base are not 16-byte aligned must keep taking the plain 8-byte path (igemm's direct epilogue)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -1234.0            # exactly representable in fp16, far outside every result here
PAD = 64                      # halfs of guard in front of and behind the output: one 128-byte line each


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.float16)


@pytest.fixture(scope="module")
def L():
    from live2diff_amd import _lib, ops
    print("device:", _lib.device_name())
    return ops


class Guarded:
    """rows x ld halfs inside a sentinel-filled buffer, `off` halfs behind the guard (off = 4: a base that is only 8-byte aligned)"""

    def __init__(self, rows, n, ld, off=0):
        self.rows, self.n, self.ld, self.off = rows, n, ld, off
        self.buf = torch.empty(PAD + off + rows * ld + PAD, dtype=torch.float16, device=DEV)
        self.view = self.buf[PAD + off:PAD + off + rows * ld].view(rows, ld)
        self.reset()

    def reset(self):
        self.buf.fill_(SENTINEL)

    def result(self):
        return self.view[:, :self.n].clone()

    def guards_intact(self):
        b = self.buf.clone()
        b[PAD + self.off:PAD + self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.n] = SENTINEL
        return bool((b == SENTINEL).all())


def _verify(launch, outs, refs, tol, what):
    """outs: Guarded buffers, refs: fp32 references (None: only repeatability and guards), launch(): runs the op(s) once"""
    launch()
    torch.cuda.synchronize()
    first = [o.result() for o in outs]
    for o, r, f in zip(outs, refs, first):
        assert o.guards_intact(), f"{what}: bytes outside the output were written"
        assert torch.isfinite(f.float()).all() and not (f == SENTINEL).any(), f"{what}: output not fully written"
        if r is not None:
            e = relerr(f, r)
            assert e <= tol, f"{what}: rel-L2 {e:.3e} > {tol:.1e}"
    for o in outs:
        o.reset()
    launch()
    torch.cuda.synchronize()
    for o, f in zip(outs, first):
        assert torch.equal(o.result(), f), f"{what}: second run differs"
        assert o.guards_intact(), f"{what}: bytes outside the output were written (second run)"


# ----------------------------------------------------------------------------------------------------- norm.hip
@pytest.mark.parametrize("one_launch", [False, True])
def test_gn_apply_stores(L, one_launch):
    """gn_apply_kernel (statistics from gn_stats) and gn_self_kernel (one launch): B 2, T 64, C 320"""
    B, T, C, G, eps = 2, 64, 320, 32, 1e-5
    x = rnd(B, T, C, seed=1) + 0.5
    gm, bt = (1 + 0.1 * rnd(C, seed=3).float()).half(), (0.1 * rnd(C, seed=4).float()).half()
    ref = F.silu(F.group_norm(x.float().permute(0, 2, 1), G, gm.float(), bt.float(), eps).permute(0, 2, 1)).reshape(B * T, C)
    xd, gmd, btd = x.to(DEV), gm.to(DEV), bt.to(DEV)
    out = Guarded(B * T, C, C)
    kw = dict(B=B, T=T, C1=C, ld1=C, G=G)
    if one_launch:
        assert L.gn_self_ok(T, C, G)
        ops_ = [L.gn_apply(xd, None, gmd, btd, out.view, eps=eps, silu=True, nchunk=0, **kw)]
    else:
        nchunk = 4
        partial = torch.empty(B * nchunk * G * 2, dtype=torch.float32, device=DEV)
        ops_ = [L.gn_stats(xd, partial, nchunk=nchunk, **kw), L.gn_apply(xd, partial, gmd, btd, out.view, eps=eps, silu=True, nchunk=nchunk, **kw)]
    _verify(lambda: [L.run(o) for o in ops_], [out], [ref], 2e-3, f"gn_apply one_launch={one_launch}")


# ----------------------------------------------------------------------------------------------------- igemm.hip
@pytest.mark.parametrize("N,ld,off,path", [(64, 72, 0, "staged 16-byte rows"), (36, 40, 0, "direct 8-byte pieces: N % 8"),
                                           (64, 72, 4, "direct 8-byte pieces: base only 8-byte aligned"),
                                           (64, 68, 0, "direct 8-byte pieces: rows only 8-byte aligned")])
def test_igemm_stores(L, N, ld, off, path):
    """M 64, K 64: the LDS-staged vector epilogue, and the outputs it must refuse (they keep the plain 8-byte stores)"""
    M, K = 64, 64
    x, w, b, r = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3).float(), rnd(M, N, seed=4)
    ref = x.float() @ w.float().t() + b + r.float()
    wp = L.pack_linear(w.to(DEV))
    out = Guarded(M, N, ld, off)
    rp = torch.zeros(M, ld, dtype=torch.float16)
    rp[:, :N] = r
    op = L.igemm(x.to(DEV), wp, out.view, M=M, Nout=N, C1=K, ldx1=K, CinP=wp.shape[1], ldo=ld, bias=b.to(DEV), res=rp.to(DEV), ldr=ld, tile=2)
    _verify(lambda: L.run(op), [out], [ref], 2e-3, f"igemm {path}")


# ----------------------------------------------------------------------------------------------------- rowgemm.hip
def test_rowgemm_row_stores(L):
    """M 32, K = N = 320, bias + residual, ldo wider than N"""
    M, K, N = 32, 320, 320
    x, w, b, r = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3).float(), rnd(M, N, seed=4)
    ref = (x.float() @ w.float().t() + b).half().float() + r.float()
    wp, bp = L.pack_rowgemm(w.to(DEV), b.to(DEV))
    out = Guarded(M, N, N + 8)
    op = L.rowgemm(x.to(DEV), wp, out.view, M=M, K=K, Nout=N, ldx=K, ldo=N + 8, bias=bp, res=r.to(DEV), ldr=N)
    _verify(lambda: L.run(op), [out], [ref], 2e-3, "rowgemm rows")


def test_rowgemm_transposed_v_stores(L):
    """q | k rows and V^T[sample][channel][ldt] pieces: B 2, T 32, C 320, ldt wider than T"""
    B, T, C = 2, 32, 320
    M, ldt = B * T, T + 8
    x, w = rnd(M, C, seed=51), rnd(3 * C, C, seed=52, scale=C ** -0.5)
    gm, bt = (1 + 0.2 * rnd(C, seed=53).float()).half(), (0.2 * rnd(C, seed=54).float()).half()
    ref = F.layer_norm(x.float(), (C,), gm.float(), bt.float(), 1e-5) @ w.float().t()
    wp, bp = L.pack_rowgemm(w.to(DEV), None, gm.to(DEV), bt.to(DEV))
    qk, vt = Guarded(M, 2 * C, 2 * C + 8), Guarded(B * C, T, ldt)
    op = L.rowgemm(x.to(DEV), wp, qk.view, M=M, K=C, Nout=3 * C, ldx=C, ldo=2 * C + 8, bias=bp, pro=1, eps=1e-5, T=T, out_t=vt.view, ntr=C,
                   ldt=ldt, st=C * ldt)
    vref = ref[:, 2 * C:].view(B, T, C).permute(0, 2, 1).reshape(B * C, T)
    _verify(lambda: L.run(op), [qk, vt], [ref[:, :2 * C], vref], 3e-3, "rowgemm q|k + V^T")


# ----------------------------------------------------------------------------------------------------- wsgemm.hip
@pytest.mark.parametrize("S", [1, 2])
def test_wsgemm_row_stores(L, S):
    """M 128, N 64, K 128, whole-row stores of the unsplit launch (S = 1) and behind the split-K reduction (S = 2); wsgemm has one
    epilogue, the LDS-staged one (fp16 tile, residual added in fp16)"""
    M, K, N = 128, 128, 64
    x, w, b, r = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3).float(), rnd(M, N, seed=4)
    ref = (x.float() @ w.float().t() + b).half().float() + r.float()
    wp, bp, _ = L.pack_wsgemm(w.to(DEV), b.to(DEV))
    sched = (2, 1, 1, S, False)
    bufs = {}
    if S > 1:
        nws, ncnt = L.wsgemm_sizes(M, N, 2, 1, S)
        bufs = dict(ws=torch.full((nws,), float("nan"), dtype=torch.float32, device=DEV), cnt=torch.zeros(ncnt, dtype=torch.int32, device=DEV))
    out = Guarded(M, N, N + 8)
    op = L.wsgemm(x.to(DEV), wp, out.view, M=M, Nout=N, C1=K, ldx1=K, ldo=N + 8, bias=bp, res=r.to(DEV), ldr=N, sched=sched, **bufs)
    _verify(lambda: L.run(op), [out], [ref], 2e-3, f"wsgemm rows S={S}")
    if S > 1:
        assert int(bufs["cnt"].abs().sum()) == 0


def test_wsgemm_transposed_v_stores(L):
    """q | k rows and the V^T rows: B 1, T 128, C 128 behind the LayerNorm fold"""
    B, T, C = 1, 128, 128
    M, ldt = B * T, T + 8
    x, w = rnd(M, C, seed=51), rnd(3 * C, C, seed=52, scale=C ** -0.5)
    gm, bt = (1 + 0.2 * rnd(C, seed=53).float()).half(), (0.2 * rnd(C, seed=54).float()).half()
    ref = F.layer_norm(x.float(), (C,), gm.float(), bt.float(), 1e-5) @ w.float().t()
    wp, bp, cs = L.pack_wsgemm(w.to(DEV), None, gm.to(DEV), bt.to(DEV))
    qk, vt = Guarded(M, 2 * C, 2 * C + 8), Guarded(B * C, T, ldt)
    op = L.wsgemm(x.to(DEV), wp, qk.view, M=M, Nout=3 * C, C1=C, ldx1=C, ldo=2 * C + 8, bias=bp, colsum=cs, pro=1, eps=1e-5, T=T, out_t=vt.view,
                  ntr=C, ldt=ldt, st=C * ldt, sched=(4, 1, 1, 1, False))
    vref = ref[:, 2 * C:].view(B, T, C).permute(0, 2, 1).reshape(B * C, T)
    _verify(lambda: L.run(op), [qk, vt], [ref[:, :2 * C], vref], 3e-3, "wsgemm q|k + V^T")


# ----------------------------------------------------------------------------------------------------- rowchain.hip
def test_rowchain_tail_stores(L):
    """block tail, M 64, C 320: the last layer's rows into a wider ldo"""
    C, M = 320, 64
    f = lambda t: t.float()
    w = dict(wo=rnd(C, C, seed=1, scale=C ** -0.5), bo=rnd(C, seed=2, scale=0.1).float(),
             gm=(1 + 0.2 * rnd(C, seed=3).float()).half(), bt=(0.2 * rnd(C, seed=4).float()).half(),
             w1=rnd(8 * C, C, seed=5, scale=C ** -0.5), b1=rnd(8 * C, seed=6, scale=0.1).float(),
             w2=rnd(C, 4 * C, seed=7, scale=(4 * C) ** -0.5), b2=rnd(C, seed=8, scale=0.1).float(),
             wp=rnd(C, C, seed=9, scale=C ** -0.5), bp=rnd(C, seed=10, scale=0.1).float())
    d = {k: v.to(DEV) for k, v in w.items()}
    pk = dict(zip(("w_out", "b_out"), L.pack_rowgemm(d["wo"], d["bo"])))
    pk.update(zip(("w_ff1", "b_ff1"), L.pack_rowgemm(d["w1"], d["b1"], d["gm"], d["bt"], geglu=True)))
    pk.update(zip(("w_ff2", "b_ff2"), L.pack_rowgemm(d["w2"], d["b2"])))
    pk.update(zip(("w_po", "b_po"), L.pack_rowgemm(d["wp"], d["bp"])))
    a, r1, r2 = rnd(M, C, seed=11), rnd(M, C, seed=12), rnd(M, C, seed=13)
    h2 = ((f(a) @ f(w["wo"]).t() + w["bo"]).half().float() + f(r1)).half().float()
    v, g = (F.layer_norm(h2, (C,), f(w["gm"]), f(w["bt"]), 1e-5) @ f(w["w1"]).t() + w["b1"]).chunk(2, dim=-1)
    h3 = (((v * F.gelu(g)).half().float() @ f(w["w2"]).t() + w["b2"]).half().float() + h2).half().float()
    ref = (h3 @ f(w["wp"]).t() + w["bp"]).half().float() + f(r2)
    out = Guarded(M, C, C + 8)
    op = L.rowchain(a.to(DEV), r1.to(DEV), r2.to(DEV), out.view, M=M, C=C, eps=1e-5, ldo=C + 8, **pk)
    _verify(lambda: L.run(op), [out], [ref], 3e-3, "rowchain tail")


@pytest.mark.parametrize("transposed", [False, True])
def test_rowchain_head_stores(L, transposed):
    """head segment, B 2, T 32, C 320: h rows, the projection columns (q | k | v, or q | k + V^T pieces)"""
    C, B, T = 320, 2, 32
    M, ldt = B * T, T + 8
    f = lambda t: t.float()
    x, res = rnd(M, C, seed=31), rnd(M, C, seed=32)
    wa, ba = rnd(C, C, seed=33, scale=C ** -0.5), rnd(C, seed=34, scale=0.1).float()
    wb = rnd(3 * C, C, seed=37, scale=C ** -0.5)
    gl, btl = (1 + 0.2 * rnd(C, seed=38).float()).half(), (0.2 * rnd(C, seed=39).float()).half()
    h = ((f(x) @ f(wa).t() + ba).half().float() + f(res)).half().float()
    ref = F.layer_norm(h, (C,), f(gl), f(btl), 1e-5) @ f(wb).t()
    wpa, bpa = L.pack_rowgemm(wa.to(DEV), ba.to(DEV))
    wpb, bpb = L.pack_rowgemm(wb.to(DEV), None, gl.to(DEV), btl.to(DEV))
    ncol = (2 if transposed else 3) * C
    hout, out = Guarded(M, C, C + 8), Guarded(M, ncol, ncol + 8)
    outs, refs = [hout, out], [h, ref[:, :ncol]]
    kw = dict(M=M, C=C, wA=wpa, bA=bpa, wB=wpb, bB=bpb, passes=3, T=T, resA=res.to(DEV), eps_ln=1e-5, ldh=C + 8, ldo=ncol + 8)
    if transposed:
        vt = Guarded(B * C, T, ldt)
        kw.update(out_t=vt.view, ldt=ldt, st=C * ldt)
        outs.append(vt)
        refs.append(ref[:, 2 * C:].view(B, T, C).permute(0, 2, 1).reshape(B * C, T))
    op = L.rowchain_head(x.to(DEV), hout.view, out.view, **kw)
    _verify(lambda: L.run(op), outs, refs, 3e-3, f"rowchain head transposed={transposed}")


# ----------------------------------------------------------------------------------------------------- pconv.hip / cconv.hip
def _conv_case(C, N):
    B, H, W = 1, 8, 16
    x, w, b = rnd(B, H, W, C, seed=1), rnd(N, C, 3, 3, seed=2, scale=(9 * C) ** -0.5), rnd(N, seed=3).float()
    r = rnd(B * H * W, N, seed=5)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.float(), b, padding=1).permute(0, 2, 3, 1).reshape(B * H * W, N).half().float() + r.float()
    return B, H, W, x, w, b, r, ref


def test_pconv_stores(L):
    """B 1, H 8, W 16, C 64, N 64: one patch, rows into a wider ldo"""
    C = N = 64
    B, H, W, x, w, b, r, ref = _conv_case(C, N)
    wp = L.pack_conv3x3(w.to(DEV))
    out = Guarded(B * H * W, N, N + 8)
    op = L.pconv(x.to(DEV), wp, out.view, B=B, H=H, W=W, C1=C, ldx1=C, CinP=C, Nout=N, ldo=N + 8, patch=(8, 16), bias=b.to(DEV), res=r.to(DEV), ldr=N)
    _verify(lambda: L.run(op), [out], [ref], 2e-3, "pconv")


@pytest.mark.parametrize("C,sched", [(64, (1, 4, 1, 1)), (128, (1, 4, 1, 2))])
def test_cconv_stores(L, C, sched):
    """B 1, H 8, W 16, N 64: the staged tile of the unsplit launch and behind the split-K reduction (S = 2 needs two 64-channel chunks:
    C 128); cconv has one epilogue, the LDS-staged one"""
    N = 64
    CG, KG, NLD, S = sched
    B, H, W, x, w, b, r, ref = _conv_case(C, N)
    wp = L.pack_cconv(w.to(DEV), KG)
    ws = cnt = None
    if S > 1:
        n_ws, n_cnt = L.cconv_sizes(B, H, W, N, CG, S)
        ws = torch.full((n_ws,), float("nan"), dtype=torch.float32, device=DEV)
        cnt = torch.zeros(n_cnt, dtype=torch.int32, device=DEV)
    out = Guarded(B * H * W, N, N + 8)
    op = L.cconv(x.to(DEV), wp, out.view, B=B, H=H, W=W, C1=C, ldx1=C, Nout=N, ldo=N + 8, KG=KG, bias=b.to(DEV), res=r.to(DEV), ldr=N, sched=sched,
                 ws=ws, cnt=cnt)
    _verify(lambda: L.run(op), [out], [ref], 2e-3, f"cconv {sched}")
    assert cnt is None or int(cnt.abs().sum()) == 0


# ----------------------------------------------------------------------------------------------------- flash_attn_ring.hip
@pytest.mark.parametrize("variant", [0, 3])
def test_flash_o_rows(L, variant):
    """B 1, H 8, d 40, Tq 64, Tk 77: the O rows leave as 8-byte pieces of the accumulator layout (plain stores)"""
    B, H, d, Tq, Tk = 1, 8, 40, 64, 77
    C = H * d
    q, k, v = rnd(B, Tq, C, seed=1), rnd(B, Tk, C, seed=2), rnd(B, Tk, C, seed=3)
    qh, kh, vh = (t.float().view(B, -1, H, d).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B * Tq, C)
    ldvt = (Tk + 7) // 8 * 8
    vt = torch.zeros(B, C, ldvt, dtype=torch.float16)
    vt[:, :, :Tk] = v.transpose(1, 2)
    out = Guarded(B * Tq, C, C + 8)
    op = L.flash_attn(q.to(DEV), k.to(DEV), vt.to(DEV), out.view, B=B, H=H, d=d, Tq=Tq, Tk=Tk, ldq=C, ldk=C, ldvt=ldvt, ldo=C + 8,
                      sq=Tq * C, sk=Tk * C, svt=C * ldvt, so=Tq * (C + 8), variant=variant)
    _verify(lambda: L.run(op), [out], [ref], 2e-3, f"flash variant {variant}")


# ----------------------------------------------------------------------------------------------------- tattn_ring.hip
@pytest.mark.parametrize("Lw", [16, 40])          # the two kernels of tattn_ring.hip: scores in registers / in LDS
def test_tattn_stream_stores(L, Lw):
    """N 1, T 8, C 320: the attention rows, and the new cache rows bit-exact with every other cache byte untouched"""
    from live2diff_amd.config import tiny_config
    from oracle import unet_ref as O
    N, T, C, S = 1, 8, 320, 8
    cfg = tiny_config(window_size=Lw, sink_size=S)
    g = torch.Generator().manual_seed(7)
    pe_idx = torch.stack([torch.cat([torch.arange(S), S + torch.randperm(Lw - S, generator=g)]) for _ in range(N)])
    upd = torch.randint(S, Lw, (N,), generator=g)
    bias = torch.zeros(N, Lw)
    q, k, v = rnd(N, T, C, seed=1), rnd(N, T, C, seed=2), rnd(N, T, C, seed=3)
    cache0 = rnd(N, 2, T, Lw, C, seed=4)
    sd = {f"to_{n}.weight": rnd(C, C, seed=10 + i, scale=C ** -0.5) for i, n in enumerate("qkv")}
    pe = O.sinusoid_pe(max(24, Lw), C)
    tabs = [(pe[:Lw] @ sd[f"to_{n}.weight"].float().t()).half().to(DEV) for n in "qkv"]
    cache_ref = cache0.clone().float()
    ref = O.stream_temporal_core(q.float(), k.float(), v.float(), O._W({k_: v_.float() for k_, v_ in sd.items()}), cfg, cache_ref, bias,
                                 pe_idx, upd, pe).reshape(N * T, C)
    qkv = torch.cat([q, k, v], -1).reshape(N * T, 3 * C).contiguous().to(DEV)
    out = Guarded(N * T, C, C)
    cbuf = torch.full((PAD + cache0.numel() + PAD,), SENTINEL, dtype=torch.float16, device=DEV)
    cache = cbuf[PAD:PAD + cache0.numel()].view(N, 2, T, Lw, C)
    op = L.tattn_stream(qkv, cache, tabs[0], tabs[1], tabs[2], pe_idx.to(DEV), upd.to(DEV), bias.half().to(DEV), out.view,
                        N=N, T=T, C=C, L=Lw, H=8, variant=13)

    def launch():
        cache.copy_(cache0)
        L.run(op)
        torch.cuda.synchronize()
        assert torch.equal(cache.cpu(), cache_ref.half()), "cache rows differ from the reference update"
        assert bool((cbuf[:PAD] == SENTINEL).all()) and bool((cbuf[-PAD:] == SENTINEL).all()), "bytes around the cache were written"

    _verify(launch, [out], [ref], 3e-3, f"tattn_stream L={Lw}")
