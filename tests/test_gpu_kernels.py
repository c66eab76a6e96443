"""-m gpu: every HIP kernel, called through the C ABI (libl2d_hip.so), against fp32 references.
(The igemm tests here launch pipeline variants 5 and 1, token-tile-major order and whichever epilogue the shape's alignment gives --
the references round once whichever that is; every variant, both orders and both epilogues, each against its own rounding, per element:
test_gpu_gemm_envelope.py.)

Tolerances (fp16 storage, fp32 accumulate): per-op rel-L2 <= 2e-3 against the fp32 reference evaluated on the
SAME fp16-rounded inputs.  Nothing here reads /root/reference.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_cases  # noqa: E402  (per-group accumulator bounds)

pytestmark = pytest.mark.gpu

DEV = "cuda"


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def check(a, b, tol=2e-3, what=""):
    assert torch.isfinite(a.float()).all(), f"{what}: non-finite output"
    e = relerr(a, b)
    assert e <= tol, f"{what}: rel-L2 {e:.3e} > {tol:.1e}"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.float16)


@pytest.fixture(scope="module")
def L():
    from live2diff_amd import _lib, ops
    print("device:", _lib.device_name())
    return ops


# ----------------------------------------------------------------------------- igemm: linear
@pytest.mark.parametrize("M,K,N", [(128, 64, 128), (8192, 320, 640), (300, 96, 68), (154, 768, 1280), (2048, 1280, 1280),
                                   (77, 320, 4), (512, 2560, 320)])
def test_igemm_linear(L, M, K, N):
    x = rnd(M, K, seed=1)
    w = rnd(N, K, seed=2, scale=K ** -0.5)
    b = rnd(N, seed=3).float()
    r = rnd(M, N, seed=4)
    ref = x.float() @ w.float().t() + b + r.float()
    wp = L.pack_linear(w.to(DEV))
    out = torch.empty(M, N, dtype=torch.float16, device=DEV)
    L.run(L.igemm(x.to(DEV), wp, out, M=M, Nout=N, C1=K, ldx1=K, CinP=wp.shape[1], ldo=N, bias=b.to(DEV), res=r.to(DEV), ldr=N))
    torch.cuda.synchronize()
    check(out, ref, what=f"linear {M}x{K}x{N}")


def test_igemm_geglu(L):
    M, C = 300, 64
    x = rnd(M, C, seed=1)
    w = rnd(8 * C, C, seed=2, scale=C ** -0.5)
    b = rnd(8 * C, seed=3)
    hg = x.float() @ w.float().t() + b.float()
    ref = hg[:, :4 * C] * F.gelu(hg[:, 4 * C:])
    wp, bp = L.pack_geglu(w.to(DEV), b.to(DEV))
    out = torch.empty(M, 4 * C, dtype=torch.float16, device=DEV)
    L.run(L.igemm(x.to(DEV), wp, out, M=M, Nout=8 * C, C1=C, ldx1=C, CinP=wp.shape[1], ldo=4 * C, bias=bp, epi=1))
    torch.cuda.synchronize()
    check(out, ref, what="geglu")
    # big-tile path
    M, C = 4096, 320
    x = rnd(M, C, seed=5)
    w = rnd(8 * C, C, seed=6, scale=C ** -0.5)
    b = rnd(8 * C, seed=7)
    hg = x.float() @ w.float().t() + b.float()
    ref = hg[:, :4 * C] * F.gelu(hg[:, 4 * C:])
    wp, bp = L.pack_geglu(w.to(DEV), b.to(DEV))
    out = torch.empty(M, 4 * C, dtype=torch.float16, device=DEV)
    L.run(L.igemm(x.to(DEV), wp, out, M=M, Nout=8 * C, C1=C, ldx1=C, CinP=wp.shape[1], ldo=4 * C, bias=bp, epi=1))
    torch.cuda.synchronize()
    check(out, ref, what="geglu big")


def test_igemm_concat_linear(L):
    M, C1, C2, N = 520, 128, 64, 96
    x1, x2 = rnd(M, C1, seed=1), rnd(M, C2, seed=2)
    w = rnd(N, C1 + C2, seed=3, scale=(C1 + C2) ** -0.5)
    ref = torch.cat([x1, x2], 1).float() @ w.float().t()
    wp = L.pack_linear(w.to(DEV))
    out = torch.empty(M, N, dtype=torch.float16, device=DEV)
    L.run(L.igemm(x1.to(DEV), wp, out, M=M, Nout=N, C1=C1, ldx1=C1, CinP=wp.shape[1], ldo=N, x2=x2.to(DEV), C2=C2, ldx2=C2))
    torch.cuda.synchronize()
    check(out, ref, what="concat linear")


def test_igemm_swapped_batched(L):
    """V^T[b] = Wv . X[b]^T (operand roles swapped, batch over grid.z)"""
    B, T, C = 2, 260, 128
    x = rnd(B, T, C, seed=1)
    wv = rnd(C, C, seed=2, scale=C ** -0.5)
    ref = torch.einsum("ck,btk->bct", wv.float(), x.float())
    ld = (T + 7) // 8 * 8
    out = torch.zeros(B, C, ld, dtype=torch.float16, device=DEV)
    wp = L.pack_linear(wv.to(DEV))
    L.run(L.igemm(wp, x.to(DEV), out, M=C, Nout=T, C1=C, ldx1=wp.shape[1], CinP=C, ldo=ld, batch=B, sx1=0, sw=T * C, so=C * ld))
    torch.cuda.synchronize()
    check(out[:, :, :T], ref, what="swapped batched")


@pytest.mark.parametrize("M,K,N,S,tile", [(128, 2560, 1280, 8, 1), (512, 1280, 320, 4, 2), (2048, 640, 640, 2, 1),
                                          (300, 1024, 70, 5, 2), (128, 11520, 256, 24, 1), (16, 2560, 1280, 8, 1),
                                          (16, 5120, 640, 32, 2), (80, 2560, 320, 7, 1)])
@pytest.mark.parametrize("fused", [False, True])
def test_igemm_splitk(L, M, K, N, S, tile, fused):
    """fused: the last-arriving block of a tile reduces the S partial tiles (fixed order) and runs the epilogue -- one launch;
    otherwise the separate reduction launch of round 1.  Both must leave the same bits on repeated runs.
    Which epilogue: ldr = round_up(N + 2, 4) is never a multiple of 8 for these N, so BOTH forms end in the direct epilogue
    (igemm_epilogue(): residual added in fp32, one rounding) -- the kernel's `vec` condition needs ldr % 8 == 0.  The fused reduction in
    front of the LDS-staged epilogue (what the plan launches) is run per element by test_gpu_gemm_envelope.py::test_igemm_splitk."""
    x = rnd(M, K, seed=1)
    w = rnd(N, K, seed=2, scale=K ** -0.5)
    b = rnd(N, seed=3).float()
    r = rnd(M, N + 2, seed=4)
    ref = F.silu(x.float() @ w.float().t() + b) + r.float()[:, :N]
    wp = L.pack_linear(w.to(DEV))
    ldo = (N + 3) // 4 * 4
    out = torch.zeros(M, ldo, dtype=torch.float16, device=DEV)
    n_ws, n_cnt = L.splitk_sizes(M, N, S, 1, tile) if fused else (S * M * ldo, 0)
    ws = torch.full((n_ws,), float("nan"), dtype=torch.float32, device=DEV)
    cnt = torch.zeros(3 + n_cnt, dtype=torch.int32, device=DEV) if fused else None
    ldr = (N + 2 + 3) // 4 * 4
    rp = torch.zeros(M, ldr, dtype=torch.float16)
    rp[:, :N + 2] = r
    outs = []
    for rep in range(3):
        out.zero_()
        L.run(L.igemm(x.to(DEV), wp, out, M=M, Nout=N, C1=K, ldx1=K, CinP=wp.shape[1], ldo=ldo, bias=b.to(DEV), res=rp.to(DEV),
                      ldr=ldr, epi=2, splitk=S, tile=tile, ws=ws, cnt=cnt, cnt_off=3))
        torch.cuda.synchronize()
        outs.append(out.clone())
        assert cnt is None or int(cnt.abs().sum()) == 0            # every launch leaves its arrival counters at zero
    check(out[:, :N], ref, what=f"splitk {M}x{K}x{N} S{S}")
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_igemm_schedule_matches_plain(L):
    """the (tile, split-K) schedule picked for the UNet's conv shapes gives the same result as tile=2, S=1"""
    from live2diff_amd.ops import igemm_schedule
    B, cin, cout, H, W = 2, 320, 128, 8, 8
    x = rnd(B, H, W, cin, seed=1).to(DEV)
    wp = L.pack_conv3x3(rnd(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5).to(DEV))
    M = B * H * W
    tile, S, _v = igemm_schedule(M, cout, wp.shape[1], 1, 0)
    assert S > 1
    outs = []
    for (t_, s_) in ((2, 1), (tile, S), (1, 3)):
        out = torch.empty(M, cout, dtype=torch.float16, device=DEV)
        ws = torch.empty(s_ * M * cout, dtype=torch.float32, device=DEV) if s_ > 1 else None
        L.run(L.igemm(x, wp, out, M=M, Nout=cout, C1=cin, ldx1=cin, CinP=wp.shape[1] // 9, ldo=cout, taps=9, B=B, Hin=H, Win=W,
                      Hout=H, Wout=W, splitk=s_, tile=t_, ws=ws))
        torch.cuda.synchronize()
        outs.append(out.float().cpu())
    check(outs[1], outs[0], tol=1e-3, what="schedule vs plain")
    check(outs[2], outs[0], tol=1e-3, what="big split vs plain")


# ----------------------------------------------------------------------------- igemm: conv
@pytest.mark.parametrize("cin,cout,H,W,stride,ups", [(64, 64, 8, 8, 1, 0), (8, 64, 12, 10, 1, 0), (96, 64, 9, 7, 1, 0),
                                                     (64, 128, 12, 10, 2, 0), (64, 64, 5, 6, 1, 1), (320, 320, 32, 32, 1, 0),
                                                     (16, 16, 8, 8, 1, 0), (320, 4, 16, 16, 1, 0)])
def test_igemm_conv3x3(L, cin, cout, H, W, stride, ups):
    B = 2
    x = rnd(B, cin, H, W, seed=1)
    w = rnd(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5)
    b = rnd(cout, seed=3).float()
    xin = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if ups else x.float()
    ref = F.conv2d(xin, w.float(), b, stride=stride, padding=1)
    Ho, Wo = ref.shape[-2:]
    xl = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wp = L.pack_conv3x3(w.to(DEV))
    out = torch.empty(B * Ho * Wo, cout, dtype=torch.float16, device=DEV)
    L.run(L.igemm(xl, wp, out, M=B * Ho * Wo, Nout=cout, C1=cin, ldx1=cin, CinP=wp.shape[1] // 9, ldo=cout, bias=b.to(DEV),
                  taps=9, B=B, Hin=H, Win=W, Hout=Ho, Wout=Wo, stride=stride, ups=ups))
    torch.cuda.synchronize()
    check(out.view(B, Ho, Wo, cout).permute(0, 3, 1, 2), ref, what=f"conv {cin}->{cout} s{stride} u{ups}")


def test_igemm_conv_rowbias_res_silu(L):
    B, cin, cout, H, W = 3, 64, 64, 6, 5
    x = rnd(B, cin, H, W, seed=1)
    w = rnd(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5)
    b = rnd(cout, seed=3).float()
    rb = rnd(B, 200, seed=4).float()
    off = 72
    res = rnd(B, cout, H, W, seed=5)
    ref = F.conv2d(x.float(), w.float(), b, padding=1) + rb[:, off:off + cout, None, None] + res.float()
    wp = L.pack_conv3x3(w.to(DEV))
    out = torch.empty(B * H * W, cout, dtype=torch.float16, device=DEV)
    rbd = rb.to(DEV)
    opk = L.igemm(x.permute(0, 2, 3, 1).contiguous().to(DEV), wp, out, M=B * H * W, Nout=cout, C1=cin, ldx1=cin,
                  CinP=wp.shape[1] // 9, ldo=cout, bias=b.to(DEV), rowbias=rbd, ldrb=200, rows_per_bias=H * W,
                  res=res.permute(0, 2, 3, 1).contiguous().to(DEV), ldr=cout, taps=9, B=B, Hin=H, Win=W, Hout=H, Wout=W)
    opk[0].p[4] = rbd.data_ptr() + 4 * off
    L.run(opk)
    torch.cuda.synchronize()
    check(out.view(B, H, W, cout).permute(0, 3, 1, 2), ref, what="conv rowbias+res")
    ref2 = F.silu(F.conv2d(x.float(), w.float(), b, padding=1))
    L.run(L.igemm(x.permute(0, 2, 3, 1).contiguous().to(DEV), wp, out, M=B * H * W, Nout=cout, C1=cin, ldx1=cin,
                  CinP=wp.shape[1] // 9, ldo=cout, bias=b.to(DEV), taps=9, B=B, Hin=H, Win=W, Hout=H, Wout=W, epi=2))
    torch.cuda.synchronize()
    check(out.view(B, H, W, cout).permute(0, 3, 1, 2), ref2, what="conv silu")


# ----------------------------------------------------------------------------- norms
@pytest.mark.parametrize("C1,C2,T,silu", [(64, 0, 16, True), (320, 0, 4096, True), (640, 320, 1024, True), (1280, 640, 256, False),
                                          (1280, 1280, 64, True), (128, 64, 300, False)])
def test_groupnorm(L, C1, C2, T, silu):
    B, G, eps = 2, 32, 1e-5
    C = C1 + C2
    x1 = rnd(B, T, C1, seed=1) + 0.5
    x2 = rnd(B, T, C2, seed=2) * 2 if C2 else None
    gm, bt = (1 + 0.1 * rnd(C, seed=3).float()).half(), (0.1 * rnd(C, seed=4).float()).half()
    xc = torch.cat([x1, x2], -1) if C2 else x1
    ref = F.group_norm(xc.float().permute(0, 2, 1), G, gm.float(), bt.float(), eps).permute(0, 2, 1)
    if silu:
        ref = F.silu(ref)
    nchunk = max(1, min(128, T // 16))
    partial = torch.empty(B * nchunk * G * 2, dtype=torch.float32, device=DEV)
    out = torch.empty(B, T, C, dtype=torch.float16, device=DEV)
    kw = dict(B=B, T=T, C1=C1, ld1=C1, G=G, nchunk=nchunk, x2=(x2.to(DEV) if C2 else None), C2=C2, ld2=C2)
    x1d = x1.to(DEV)
    L.run(L.gn_stats(x1d, partial, **kw))
    L.run(L.gn_apply(x1d, partial, gm.to(DEV), bt.to(DEV), out, eps=eps, silu=silu, **kw))
    torch.cuda.synchronize()
    check(out, ref, what=f"groupnorm {C1}+{C2} T{T}")


@pytest.mark.parametrize("C1,C2,T,silu", [(1280, 0, 144, True), (1280, 1280, 36, True), (1280, 640, 144, True), (640, 0, 576, True),
                                          (320, 0, 100, False), (640, 320, 144, True), (64, 0, 16, False), (2560, 0, 400, True)])
def test_groupnorm_one_launch(L, C1, C2, T, silu):
    """gn_apply with nchunk = 0 and no accumulator (norm.hip gn_self_kernel, round 6): statistics and apply in one launch for the small
    tensors whose producers cannot deliver the statistics (pixel counts per sample that are no whole GEMM tiles: 12 x 12, 6 x 6, 10 x 10,
    20 x 20 ...).  Group sizes 2 / 10 / 20 / 30 / 40 / 60 / 80 (bands of 1-4 whole groups, a group may straddle the two inputs of a
    concat).  Against F.group_norm in fp32, against the two-launch path, and bit-repeatable."""
    B, G, eps = 2, 32, 1e-5
    C = C1 + C2
    assert L.gn_self_ok(T, C, G)
    x1 = rnd(B, T, C1, seed=1) + 0.5
    x2 = rnd(B, T, C2, seed=2) * 2 if C2 else None
    gm, bt = (1 + 0.1 * rnd(C, seed=3).float()).half(), (0.1 * rnd(C, seed=4).float()).half()
    xc = torch.cat([x1, x2], -1) if C2 else x1
    ref = F.group_norm(xc.float().permute(0, 2, 1), G, gm.float(), bt.float(), eps).permute(0, 2, 1)
    if silu:
        ref = F.silu(ref)
    x1d, x2d, gmd, btd = x1.to(DEV), (x2.to(DEV) if C2 else None), gm.to(DEV), bt.to(DEV)
    kw = dict(B=B, T=T, C1=C1, ld1=C1, G=G, x2=x2d, C2=C2, ld2=C2)
    out = torch.full((B, T, C), float("nan"), dtype=torch.float16, device=DEV)
    L.run(L.gn_apply(x1d, None, gmd, btd, out, eps=eps, silu=silu, nchunk=0, **kw))
    torch.cuda.synchronize()
    check(out, ref, what=f"one-launch groupnorm {C1}+{C2} T{T}")
    out2 = torch.full((B, T, C), float("nan"), dtype=torch.float16, device=DEV)
    L.run(L.gn_apply(x1d, None, gmd, btd, out2, eps=eps, silu=silu, nchunk=0, **kw))
    torch.cuda.synchronize()
    assert torch.equal(out, out2)
    nchunk = max(1, min(64, T // 16))
    partial = torch.empty(B * nchunk * G * 2, dtype=torch.float32, device=DEV)
    out3 = torch.empty(B, T, C, dtype=torch.float16, device=DEV)
    L.run(L.gn_stats(x1d, partial, nchunk=nchunk, **kw))
    L.run(L.gn_apply(x1d, partial, gmd, btd, out3, eps=eps, silu=silu, nchunk=nchunk, **kw))
    torch.cuda.synchronize()
    assert (out.float() - out3.float()).abs().max().item() <= 4e-3 * max(1.0, out3.float().abs().max().item())


def test_groupnorm_one_launch_refuses_what_does_not_fit(L):
    """T * band / 8 beyond 16 vectors per thread, or an odd group size whose band would hold more than four groups: EINVAL with a message,
    never a silent wrong launch; ops.gn_self_ok agrees with the library."""
    from live2diff_amd import _lib
    for (C, T) in ((1280, 4096), (1920, 400), (160, 64)):
        assert not L.gn_self_ok(T, C, 32)
        x = rnd(1, T, C, seed=1).to(DEV)
        g = torch.ones(C, dtype=torch.float16, device=DEV)
        out = torch.empty_like(x)
        with pytest.raises(_lib.L2DError):
            L.run(L.gn_apply(x, None, g, g, out, eps=1e-5, silu=False, B=1, T=T, C1=C, ld1=C, G=32, nchunk=0))


@pytest.mark.parametrize("B,T,K,C,tile,splitk,choff2,Ccat", [
    (2, 4096, 320, 320, 1, 1, 0, 640),        # 128x128 tile, cpg 10 / 20: groups straddle the 128-channel tiles
    (2, 1024, 640, 640, 2, 1, 640, 1280),     # 64x64 tile; second consumer sees this tensor as the upper half of a concat
    (2, 256, 1280, 640, 2, 1, 1280, 1920),    # the 640-channel half of a 1280 + 640 concat: cpg 60, a group straddles the inputs
    (2, 64, 2560, 1280, 2, 4, 0, 2560),       # split-K: statistics from the (tiled) split-K epilogue, T = 64
    (2, 64, 2560, 1280, 2, -4, 0, 2560),      # split-K with the fused reduction (negative = fused): the last block of a tile
    (2, 256, 5120, 1280, 1, -6, 0, 2560),     # ... 128x128 tiles, T = 256
    (8, 64, 320, 320, 2, 1, 0, 640),          # warm-up batch: 8 samples
])
def test_igemm_groupnorm_statistics_from_the_producer(L, B, T, K, C, tile, splitk, choff2, Ccat):
    """The producer GEMM accumulates sum / sum of squares of its OUTPUT per (sample, group) for up to two consumer GroupNorms
    as fixed-point integer atomics (include/l2d.h, igemm `gn` fields); gn_apply with nchunk = 0 normalises from them.
    Checked against sums over the fp16 tensor the GEMM wrote, and against F.group_norm; repeated launches are bit-identical."""
    from live2diff_amd import _lib
    G, M = 32, B * T
    x = rnd(M, K, seed=1)
    w = rnd(C, K, seed=2, scale=K ** -0.5)
    b = rnd(C, seed=3).float()
    r = rnd(M, C, seed=4)
    wp = L.pack_linear(w.to(DEV))
    out = torch.empty(M, C, dtype=torch.float16, device=DEV)
    fused, splitk = splitk < 0, abs(splitk)
    ws = torch.empty(L.splitk_sizes(M, C, splitk, 1, tile)[0] if fused else splitk * M * C, dtype=torch.float32, device=DEV) if splitk > 1 else None
    cnt = torch.zeros(L.splitk_sizes(M, C, splitk, 1, tile)[1], dtype=torch.int32, device=DEV) if fused else None
    acc = torch.zeros(2, B, G, 2, dtype=torch.int64, device=DEV)
    cpg1, cpg2 = C // G, Ccat // G
    accs = []
    for rep in range(2):
        acc.zero_()
        op, keep = L.igemm(x.to(DEV), wp, out, M=M, Nout=C, C1=K, ldx1=K, CinP=wp.shape[1], ldo=C, bias=b.to(DEV), res=r.to(DEV), ldr=C,
                           splitk=splitk, tile=tile, ws=ws, variant=1, cnt=cnt)
        assert L.igemm_gn_target(op, acc[0].data_ptr(), T=T, G=G, cpg=cpg1, choff=0)
        assert L.igemm_gn_target(op, acc[1].data_ptr(), T=T, G=G, cpg=cpg2, choff=choff2)
        assert not L.igemm_gn_target(op, acc[1].data_ptr(), T=T, G=G, cpg=cpg2, choff=0)      # both slots taken
        L.run((op, keep + (acc,)))
        torch.cuda.synchronize()
        accs.append(acc.clone())
    assert torch.equal(accs[0], accs[1])                                   # integer accumulation: order-independent
    o = out.float().cpu().view(B, T, C)
    ref = x.float() @ w.float().t() + b + r.float()
    check(out, ref, what="gemm output")
    a0 = accs[0].cpu().double()
    s1 = o.double().view(B, T, G, cpg1).sum((1, 3))
    s2 = (o.double() ** 2).view(B, T, G, cpg1).sum((1, 3))
    assert (a0[0, :, :, 0] / 2 ** 20 - s1).abs().max() <= 1e-3 * max(1.0, s1.abs().max().item())
    assert (a0[0, :, :, 1] / 2 ** 12 - s2).abs().max() <= 1e-3 * s2.abs().max().item()
    # consumer 2: this tensor occupies channels [choff2, choff2 + C) of a Ccat-channel concat
    full = torch.zeros(B, T, Ccat, dtype=torch.float64)
    full[:, :, choff2:choff2 + C] = o.double()
    t1 = full.view(B, T, G, cpg2).sum((1, 3))
    t2 = (full ** 2).view(B, T, G, cpg2).sum((1, 3))
    assert (a0[1, :, :, 0] / 2 ** 20 - t1).abs().max() <= 1e-3 * max(1.0, t1.abs().max().item())
    assert (a0[1, :, :, 1] / 2 ** 12 - t2).abs().max() <= 1e-3 * t2.abs().max().item()
    # ... and every group on its own, against the bounds of the arithmetic (the two lines above see the largest group only)
    norm_cases.check_acc(accs[0][0], out.cpu().view(B, T, C), G, cpg1, 0, what="igemm consumer 1")
    norm_cases.check_acc(accs[0][1], out.cpu().view(B, T, C), G, cpg2, choff2, what="igemm consumer 2")
    # gn_apply from the accumulators == GroupNorm of the stored tensor
    gm, bt = (1 + 0.1 * rnd(C, seed=5).float()).half(), (0.1 * rnd(C, seed=6).float()).half()
    y = torch.empty(M, C, dtype=torch.float16, device=DEV)
    L.run(L.gn_apply(out, None, gm.to(DEV), bt.to(DEV), y, B=B, T=T, C1=C, ld1=C, G=G, nchunk=0, eps=1e-5, silu=True,
                     acc_ptr=accs[0][0].contiguous().data_ptr() if False else acc[0].data_ptr()))
    torch.cuda.synchronize()
    gref = F.silu(F.group_norm(o.permute(0, 2, 1), G, gm.float(), bt.float(), 1e-5)).permute(0, 2, 1).reshape(M, C)
    check(y, gref, what="gn_apply from producer statistics")


@pytest.mark.parametrize("rows,C", [(7, 64), (8192, 320), (100, 1280), (33, 640)])
def test_layernorm(L, rows, C):
    x = rnd(rows, C, seed=1) * 3 + 1
    gm, bt = (1 + 0.1 * rnd(C, seed=3).float()).half(), (0.1 * rnd(C, seed=4).float()).half()
    ref = F.layer_norm(x.float(), (C,), gm.float(), bt.float(), 1e-5)
    out = torch.empty(rows, C, dtype=torch.float16, device=DEV)
    L.run(L.layernorm(x.to(DEV), gm.to(DEV), bt.to(DEV), out, rows=rows, C=C, ldx=C, ldo=C))
    torch.cuda.synchronize()
    check(out, ref, what="layernorm")


# ----------------------------------------------------------------------------- flash attention
@pytest.mark.parametrize("d,Tq,Tk", [(8, 256, 256), (16, 64, 64), (32, 100, 77), (40, 1024, 1024), (40, 4096, 77),
                                     (80, 1024, 1024), (160, 256, 256), (160, 64, 77), (40, 130, 200), (80, 144, 144)])
def test_flash_attn(L, d, Tq, Tk):
    B, H = 2, 8
    C = H * d
    q, k, v = rnd(B, Tq, C, seed=1), rnd(B, Tk, C, seed=2), rnd(B, Tk, C, seed=3)
    qh, kh, vh = (t.float().view(B, -1, H, d).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, Tq, C)
    ldvt = (Tk + 7) // 8 * 8
    vt = torch.full((B, C, ldvt), float("nan"), dtype=torch.float16)     # padding columns hold garbage
    vt[:, :, :Tk] = v.transpose(1, 2)
    outs = {}
    for variant in (1, 2, 3, 4):    # register-staged kernel, LDS-DMA ring kernel with 32 / 16 query rows per wave, pipelined loop
        out = torch.full((B, Tq, C), float("nan"), dtype=torch.float16, device=DEV)
        L.run(L.flash_attn(q.to(DEV), k.to(DEV), vt.to(DEV), out, B=B, H=H, d=d, Tq=Tq, Tk=Tk, ldq=C, ldk=C, ldvt=ldvt, ldo=C,
                           sq=Tq * C, sk=Tk * C, svt=C * ldvt, so=Tq * C, variant=variant))
        torch.cuda.synchronize()
        check(out, ref, what=f"flash d{d} {Tq}x{Tk} v{variant}")
        outs[variant] = out
    assert torch.equal(outs[4], outs[2])    # the pipelined loop reorders instructions, not arithmetic


@pytest.mark.parametrize("d", [40, 32, 16])
@pytest.mark.parametrize("Tk", [8, 40, 64, 77, 128, 130, 192, 200, 256, 300, 320, 384, 391, 448, 460, 512, 576, 1000])
def test_flash_attn_pipelined_tile_counts(L, d, Tk):
    """The pipelined loop (variant 4) has its own prologue / refill / drain structure: every key-tile count from 1 to 9 and
    ragged last tiles (Tk % 64, Tk % 8 != 0), bit-identical to the plain ring loop (variant 2) and within tolerance of fp32."""
    B, H, Tq = 2, 8, 200
    C = H * d
    q, k, v = rnd(B, Tq, C, seed=31), rnd(B, Tk, C, seed=32), rnd(B, Tk, C, seed=33)
    qh, kh, vh = (t.float().view(B, -1, H, d).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, Tq, C)
    ldvt = (Tk + 7) // 8 * 8
    vt = torch.full((B, C, ldvt), float("nan"), dtype=torch.float16)
    vt[:, :, :Tk] = v.transpose(1, 2)
    outs = {}
    for variant in (2, 4):
        out = torch.full((B, Tq, C), float("nan"), dtype=torch.float16, device=DEV)
        L.run(L.flash_attn(q.to(DEV), k.to(DEV), vt.to(DEV), out, B=B, H=H, d=d, Tq=Tq, Tk=Tk, ldq=C, ldk=C, ldvt=ldvt, ldo=C,
                           sq=Tq * C, sk=Tk * C, svt=C * ldvt, so=Tq * C, variant=variant))
        torch.cuda.synchronize()
        check(out, ref, what=f"flash pipelined d{d} Tk{Tk} v{variant}")
        outs[variant] = out
    assert torch.equal(outs[4], outs[2])


def _sdpa_ref_blocks(q, k, v, H, blk=1024):
    """fp32 softmax(QK^T/sqrt d)V on the device in query blocks (a [H,blk,Tk] score slab at a time)."""
    B, Tq, C = q.shape
    d = C // H
    out = torch.empty(B, Tq, C, dtype=torch.float32, device=q.device)
    for b in range(B):
        kh = k[b].float().view(-1, H, d).permute(1, 2, 0)            # [H,d,Tk]
        vh = v[b].float().view(-1, H, d).permute(1, 0, 2)            # [H,Tk,d]
        for q0 in range(0, Tq, blk):
            qh = q[b, q0:q0 + blk].float().view(-1, H, d).permute(1, 0, 2)
            p = torch.softmax(torch.matmul(qh, kh) * d ** -0.5, dim=-1)
            out[b, q0:q0 + blk] = torch.matmul(p, vh).permute(1, 0, 2).reshape(-1, C)
    return out


@pytest.mark.parametrize("d,T", [(40, 6144), (40, 9216), (80, 2304), (160, 576)])
def test_flash_attn_long_sequences(L, d, T):
    """Self-attention lengths of BASELINE cfg-3 (64x96 latent: T = 6144 / 1536 / 384) and cfg-5 (72x128: T = 9216 / 2304 /
    576) at the SD-1.5 head sizes, N = 2 stream rows, against fp32 attention on the same fp16 inputs."""
    B, H = 2, 8
    C = H * d
    g = torch.Generator(device=DEV).manual_seed(11)
    q, k, v = (torch.randn(B, T, C, generator=g, device=DEV, dtype=torch.float16) for _ in range(3))
    ref = _sdpa_ref_blocks(q, k, v, H)
    vt = v.transpose(1, 2).contiguous()
    outs = {}
    for variant in (1, 2, 3, 4):
        out = torch.empty(B, T, C, dtype=torch.float16, device=DEV)
        L.run(L.flash_attn(q, k, vt, out, B=B, H=H, d=d, Tq=T, Tk=T, ldq=C, ldk=C, ldvt=T, ldo=C, sq=T * C, sk=T * C, svt=C * T,
                           so=T * C, variant=variant))
        torch.cuda.synchronize()
        check(out, ref, what=f"flash long d{d} T{T} v{variant}")
        outs[variant] = out
    assert torch.equal(outs[4], outs[2])


@pytest.mark.parametrize("d", [40, 80, 160])
@pytest.mark.parametrize("scale,spike_tile", [(0.25, None), (4.0, 0), (4.0, 5), (16.0, 3)])
def test_flash_attn_forced_rescale(L, d, scale, spike_tile):
    """The lazy running-max rescale (only when a row's maximum grows by more than 2^8) is a rare, data-dependent branch:
    force it.  Logits are scaled by `scale`^2 and one key (in key tile `spike_tile`) is aligned with a block of queries so
    that their maximum jumps far past the threshold exactly there -- early tiles (0), mid-stream (5) and with huge logits
    (16).  fp64 reference on the same fp16 inputs; every row is compared, not a sample."""
    B, H, T = 1, 8, 640
    C = H * d
    q, k, v = rnd(B, T, C, seed=21) * scale, rnd(B, T, C, seed=22) * scale, rnd(B, T, C, seed=23)
    if spike_tile is not None:
        key = spike_tile * 64 + 17
        k[0, key] = (q[0, 100:164].float().mean(0) * 6).half()      # strongly aligned with 64 consecutive queries
        q[0, 300] = (k[0, key].float() * 0.5).half()                  # and one query aligned even harder
    qh, kh, vh = (t.double().view(B, -1, H, d).transpose(1, 2) for t in (q, k, v))
    ref = torch.softmax(qh @ kh.transpose(-1, -2) * d ** -0.5, -1) @ vh
    ref = ref.transpose(1, 2).reshape(B, T, C)
    vt = v.transpose(1, 2).contiguous()
    for variant in (1, 2, 3, 4):
        out = torch.empty(B, T, C, dtype=torch.float16, device=DEV)
        L.run(L.flash_attn(q.to(DEV), k.to(DEV), vt.to(DEV), out, B=B, H=H, d=d, Tq=T, Tk=T, ldq=C, ldk=C, ldvt=T, ldo=C,
                           sq=T * C, sk=T * C, svt=C * T, so=T * C, variant=variant))
        torch.cuda.synchronize()
        # the ring kernel pre-scales Q by log2(e)/sqrt(d) in fp16: one more rounding of the size Q already carries; at logit
        # magnitudes of ~1e3 (scale 16) that is ~0.1 absolute in the exponent, hence the wider bound for that synthetic case
        tol = 4e-3 if (variant == 1 or scale < 16) else 2e-2
        check(out, ref, tol=tol, what=f"flash forced rescale d{d} x{scale} tile {spike_tile} v{variant}")
        worst = (out.double().cpu() - ref).abs().max().item()
        lim = (2e-2 if tol == 4e-3 else 1e-1) * max(1.0, v.float().abs().max().item())
        assert worst <= lim, (variant, worst)      # no O(1)-wrong row hiding inside the L2 norm


def test_flash_attn_softmax_stress(L):
    """large logits + one dominant key per row: exercises the running-max rescale across tiles"""
    B, H, d, T = 1, 8, 40, 512
    C = H * d
    q, k, v = rnd(B, T, C, seed=1) * 4, rnd(B, T, C, seed=2) * 4, rnd(B, T, C, seed=3)
    k[:, 300] *= 3
    qh, kh, vh = (t.float().view(B, -1, H, d).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, T, C)
    vt = v.transpose(1, 2).contiguous()
    out = torch.empty(B, T, C, dtype=torch.float16, device=DEV)
    L.run(L.flash_attn(q.to(DEV), k.to(DEV), vt.to(DEV), out, B=B, H=H, d=d, Tq=T, Tk=T, ldq=C, ldk=C, ldvt=T, ldo=C,
                       sq=T * C, sk=T * C, svt=C * T, so=T * C))
    torch.cuda.synchronize()
    check(out, ref, tol=4e-3, what="flash stress")


# ----------------------------------------------------------------------------- temporal attention
def _tattn_case(C, T, Lw, S, N, seed, ramp=True):
    g = torch.Generator().manual_seed(seed)
    pe_idx = torch.stack([torch.cat([torch.arange(S), S + torch.randperm(Lw - S, generator=g)]) for _ in range(N)])
    upd = torch.randint(S, Lw, (N,), generator=g)
    bias = torch.zeros(N, Lw)
    if ramp:
        for n in range(N):
            if n % 2 == 1:
                bias[n, S + 2:] = float("-inf")
    return pe_idx, upd, bias


@pytest.mark.parametrize("C,T,Lw,S,N,variant", [(64, 16, 16, 8, 2, 0), (64, 50, 12, 4, 1, 0), (128, 8, 24, 8, 4, 0),
                                                (64, 4, 40, 8, 2, 0), (320, 256, 16, 8, 2, 0), (320, 256, 16, 8, 2, 2),
                                                (320, 100, 16, 8, 2, 3), (640, 64, 16, 8, 2, 0), (1280, 16, 16, 8, 2, 0),
                                                (1280, 64, 40, 8, 2, 0), (256, 37, 24, 8, 3, 0),
                                                (320, 256, 16, 8, 2, 7), (640, 64, 16, 8, 2, 7), (1280, 16, 16, 8, 2, 7),
                                                (64, 50, 12, 4, 1, 7), (256, 37, 16, 8, 3, 7), (320, 100, 16, 8, 2, 6),
                                                (320, 256, 16, 8, 2, 13), (640, 64, 16, 8, 2, 13), (1280, 16, 16, 8, 2, 13),
                                                (320, 1024, 16, 8, 3, 13), (640, 104, 12, 4, 2, 13), (1280, 8, 12, 4, 1, 13),
                                                (320, 4096, 16, 8, 2, 13), (1280, 64, 16, 8, 2, 13), (640, 1024, 16, 8, 2, 13),
                                                # BASELINE cfg-3 (L = 24) / cfg-5 (L = 40) windows at the SD-1.5 widths: the
                                                # chunked kernel's real shapes (T = a slice of the 64x96 / 72x128 levels)
                                                (320, 384, 24, 8, 2, 0), (640, 96, 24, 8, 2, 0), (1280, 24, 24, 8, 2, 0),
                                                (320, 144, 40, 8, 2, 0), (640, 36, 40, 8, 2, 0), (1280, 9, 40, 8, 2, 0),
                                                (320, 100, 24, 8, 4, 3), (640, 50, 40, 8, 2, 3),
                                                # L = 40 through the loader-wave ring kernel's long-window form (scores in LDS)
                                                (320, 1152, 40, 8, 2, 13), (640, 72, 40, 8, 2, 13), (1280, 16, 40, 8, 1, 13),
                                                (320, 144, 40, 8, 3, 13), (320, 384, 24, 8, 2, 13)])
def test_tattn_stream(L, C, T, Lw, S, N, variant):
    from live2diff_amd.config import tiny_config
    from oracle import unet_ref as O
    cfg = tiny_config(window_size=Lw, sink_size=S)
    pe_idx, upd, bias = _tattn_case(C, T, Lw, S, N, seed=7)
    q, k, v = rnd(N, T, C, seed=1), rnd(N, T, C, seed=2), rnd(N, T, C, seed=3)
    cache0 = rnd(N, 2, T, Lw, C, seed=4)
    sd = {f"to_{n}.weight": rnd(C, C, seed=10 + i, scale=C ** -0.5) for i, n in enumerate("qkv")}
    pe = O.sinusoid_pe(max(24, Lw), C)
    tabs = [(pe[:Lw] @ sd[f"to_{n}.weight"].float().t()).half() for n in "qkv"]
    # the reference's tables are fp16 buffers: the oracle core sees the fp16-rounded tables via an identity "weight"
    cache_ref = cache0.clone().float()
    w_ = O._W({k_: v_.float() for k_, v_ in sd.items()})
    ref = O.stream_temporal_core(q.float(), k.float(), v.float(), w_, cfg, cache_ref, bias, pe_idx, upd, pe)
    qkv = torch.cat([q, k, v], -1).reshape(N * T, 3 * C).contiguous().to(DEV)
    cache = cache0.clone().to(DEV)
    out = torch.empty(N * T, C, dtype=torch.float16, device=DEV)
    L.run(L.tattn_stream(qkv, cache, tabs[0].to(DEV), tabs[1].to(DEV), tabs[2].to(DEV), pe_idx.to(DEV), upd.to(DEV),
                         bias.half().to(DEV), out, N=N, T=T, C=C, L=Lw, H=8, variant=variant))
    torch.cuda.synchronize()
    check(out.view(N, T, C), ref, tol=3e-3, what=f"tattn_stream C{C} L{Lw} v{variant}")
    # cache: exactly slot update_idx[n] of row n rewritten with the (pre-PE) k / v, everything else untouched
    assert torch.equal(cache.cpu(), cache_ref.half()), "cache contents differ from the reference update"


def test_tattn_stream_slot_permutation_full_size(L):
    """BASELINE size of the largest KV-cache launch (N=2, T=4096, C=320, L=16; 168 MB cache), no oracle: softmax
    attention over the L slots does not care about slot ORDER, so permuting the cache slots together with pe_idx, the
    bias row and update_idx leaves the output unchanged (fp32 summation order only) and writes the new row to the
    permuted slot."""
    N, T, C, Lw = 2, 4096, 320, 16
    g = torch.Generator(device=DEV).manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV, dtype=torch.float16)
    qkv, cache = rn(N * T, 3 * C), rn(N, 2, T, Lw, C)
    tabs = [rn(24, C) * 0.5 for _ in range(3)]
    pe_idx = torch.stack([torch.randperm(Lw, generator=torch.Generator().manual_seed(n)) for n in range(N)]).to(DEV)
    upd = torch.tensor([9, 13], device=DEV)
    bias = torch.zeros(N, Lw, dtype=torch.float16, device=DEV)
    bias[1, 14:] = float("-inf")                                   # row 1: two masked slots
    perm = torch.randperm(Lw, generator=torch.Generator().manual_seed(99)).to(DEV)   # new slot j holds old slot perm[j]
    inv = torch.argsort(perm)
    outs, caches = [], []
    for permuted in (False, True):
        c = cache.clone()
        p_, b_, u_ = pe_idx, bias, upd
        if permuted:
            c = c[:, :, :, perm].contiguous()
            p_, b_, u_ = pe_idx[:, perm].contiguous(), bias[:, perm].contiguous(), inv[upd]
        out = torch.empty(N * T, C, dtype=torch.float16, device=DEV)
        L.run(L.tattn_stream(qkv, c, tabs[0], tabs[1], tabs[2], p_, u_, b_, out, N=N, T=T, C=C, L=Lw, H=8))
        torch.cuda.synchronize()
        outs.append(out.float())
        caches.append(c[:, :, :, inv].contiguous() if permuted else c)
    assert torch.isfinite(outs[0]).all()
    e = relerr(outs[1], outs[0])
    assert e <= 1e-3, e                                            # fp16 output rounding of differently ordered fp32 sums
    assert torch.equal(caches[0], caches[1]), "the new row must land in the permuted slot, nothing else may change"
    k_new = qkv.view(N, T, 3 * C)[:, :, C:2 * C]
    for n in range(N):
        assert torch.equal(caches[0][n, 0, :, int(upd[n])], k_new[n])


def test_tattn_stream_golden(L, golden):
    """directly against the fixture captured from the reference's StreamTemporalAttention (incl. projections
    done on the host in fp32 -> the kernel sees fp16-rounded q,k,v)."""
    from live2diff_amd.config import tiny_config
    from live2diff_amd.weights import _fill
    from oracle import unet_ref as O
    for ci in range(4):
        g = golden(f"stream_attn_{ci}")
        C, T, Lw, S, N = [int(v) for v in g["meta"]]
        sd = {k: _fill(f"sta{ci}." + k, shp, 1.0) for k, shp in
              {"to_q.weight": (C, C), "to_k.weight": (C, C), "to_v.weight": (C, C), "to_out.0.weight": (C, C), "to_out.0.bias": (C,)}.items()}
        x = torch.from_numpy(g["x"])
        q, k, v = (x @ sd[f"to_{n}.weight"].t() for n in "qkv")
        pe = O.sinusoid_pe(max(24, Lw), C)
        tabs = [(pe[:Lw] @ sd[f"to_{n}.weight"].t()).half().to(DEV) for n in "qkv"]
        qkv = torch.cat([q, k, v], -1).reshape(N * T, 3 * C).half().contiguous().to(DEV)
        cache = torch.from_numpy(g["cache_in"]).half().to(DEV)
        out = torch.empty(N * T, C, dtype=torch.float16, device=DEV)
        L.run(L.tattn_stream(qkv, cache, *tabs, torch.from_numpy(g["pe_idx"]).to(DEV), torch.from_numpy(g["update_idx"]).to(DEV),
                             torch.from_numpy(g["bias"]).half().to(DEV), out, N=N, T=T, C=C, L=Lw, H=8))
        torch.cuda.synchronize()
        full = out.float().cpu().view(N, T, C) @ sd["to_out.0.weight"].t() + sd["to_out.0.bias"]
        check(full, torch.from_numpy(g["out"]), tol=5e-3, what=f"golden stream_attn_{ci}")
        check(cache, torch.from_numpy(g["cache_out"]), tol=1e-3, what=f"golden cache {ci}")


@pytest.mark.parametrize("C,T", [(64, 20), (128, 16), (320, 64), (640, 16), (1280, 9), (256, 16)])
def test_tattn_warmup(L, C, T):
    from live2diff_amd.config import tiny_config
    from oracle import unet_ref as O
    Fr, Lw = 8, 16
    cfg = tiny_config(window_size=Lw, sink_size=8)
    q, k, v = rnd(Fr, T, C, seed=1), rnd(Fr, T, C, seed=2), rnd(Fr, T, C, seed=3)
    sd = {f"to_{n}.weight": rnd(C, C, seed=10 + i, scale=C ** -0.5) for i, n in enumerate("qkv")}
    pe = O.sinusoid_pe(24, C)
    tabs = [(pe[:Lw] @ sd[f"to_{n}.weight"].float().t()).half() for n in "qkv"]
    row_ref = torch.zeros(2, T, Lw, C)
    w_ = O._W({k_: v_.float() for k_, v_ in sd.items()})
    ref = O.warmup_temporal_core(q.float().transpose(0, 1), k.float().transpose(0, 1), v.float().transpose(0, 1), w_, cfg,
                                 row_ref, pe).transpose(0, 1)
    qkv = torch.cat([q, k, v], -1).reshape(Fr * T, 3 * C).contiguous().to(DEV)
    row = torch.zeros(2, T, Lw, C, dtype=torch.float16, device=DEV)
    out = torch.empty(Fr * T, C, dtype=torch.float16, device=DEV)
    L.run(L.tattn_warmup(qkv, row, tabs[0].to(DEV), tabs[1].to(DEV), tabs[2].to(DEV), out, F=Fr, T=T, C=C, L=Lw, H=8))
    torch.cuda.synchronize()
    check(out.view(Fr, T, C), ref, tol=3e-3, what=f"tattn_warmup C{C}")
    assert torch.equal(row.cpu(), row_ref.half())


# ----------------------------------------------------------------------------- small kernels
def test_timestep_and_skinny(L):
    from oracle import unet_ref as O
    t = torch.tensor([399, 199, 999, 0], dtype=torch.int64)
    out = torch.empty(4, 320, dtype=torch.float16, device=DEV)
    L.run(L.timestep_embed(t.to(DEV), out, N=4, dim=320))
    torch.cuda.synchronize()
    ref = O.timestep_sinusoid(t, 320)
    assert (out.float().cpu() - ref).abs().max() < 2e-3
    for M, K, N, silu, isf in [(2, 320, 1280, True, False), (4, 1280, 1000, False, True), (1, 64, 7, False, False), (8, 1280, 64, True, True)]:
        a, w, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3).float()
        ref = a.float() @ w.float().t() + b
        if silu:
            ref = F.silu(ref)
        o = torch.empty(M, N, dtype=torch.float32 if isf else torch.float16, device=DEV)
        L.run(L.skinny_linear(a.to(DEV), w.to(DEV), b.to(DEV), o, M=M, K=K, Nout=N, silu_out=silu))
        torch.cuda.synchronize()
        check(o, ref, what=f"skinny {M}x{K}x{N}")


def test_layout_and_lcm(L, golden):
    x = rnd(3, 4, 35, seed=1)
    o = torch.empty(3, 35, 8, dtype=torch.float16, device=DEV)
    L.run(L.nchw_to_nhwc(x.to(DEV), o, B=3, C=4, HW=35, Cpad=8))
    torch.cuda.synchronize()
    assert torch.equal(o[:, :, :4].cpu(), x.transpose(1, 2)) and (o[:, :, 4:] == 0).all()
    y = rnd(3, 35, 4, seed=2)
    o2 = torch.empty(3, 4, 35, dtype=torch.float16, device=DEV)
    L.run(L.nhwc_to_nchw(y.to(DEV), o2, B=3, C=4, HW=35, ld=4))
    torch.cuda.synchronize()
    assert torch.equal(o2.cpu(), y.transpose(1, 2))
    g = golden("state_machine")
    xs, eps = torch.from_numpy(g["lcm_x"]).half(), torch.from_numpy(g["lcm_eps"]).half()
    scal = torch.stack([torch.from_numpy(g[k]).flatten() for k in ("lcm_alpha", "lcm_beta", "lcm_c_skip", "lcm_c_out")], 1).float()
    x0 = torch.empty_like(xs, device=DEV)
    L.run(L.lcm_step(xs.to(DEV), eps.to(DEV), scal.contiguous().to(DEV), x0, N=3, per=xs[0].numel()))
    torch.cuda.synchronize()
    check(x0, torch.from_numpy(g["lcm_x0"]), tol=3e-3, what="lcm step")
