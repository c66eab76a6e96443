"""-m gpu: igemm (every pipeline shape, both tiles, the three gather modes, split-K in both forms, every epilogue in its staged and its
direct form, the conv geometries) and skinny_linear per output ELEMENT on planted operands (helpers, regimes, the bound and its
derivation: gemm_cases.py; the bound is first shown to hold, with half to spare, for plain-torch restatements of the kernel's arithmetic:
test_gemm_envelope_cpu.py).

Every other GEMM / conv test draws iid N(0, 1) operands and judges one rel-L2 of 2e-3 over the whole tensor.  Here every token row
(conv: every sample) and every output channel follows its own regime -- one non-zero input element at k = 0, either side of a BK
boundary, C1 - 1, the first channel of x2, the last real k; an impulse image; a cancelling pair of products in the first and last K
stage; outputs of 2e4 and in the fp16 subnormal range; a row mean of 20; a border ring of +-1e3; a zero, a one-hot, an alternating
weight row; a bias of 1e3 cancelled by the residual -- and every element is held to gemm_cases.exact_and_bound against fp64 on the same
fp16 operands.  Elements with a single product must equal the fp32 restatement bit for bit (epi 0, 3, 4), which also pins WHICH of the
two epilogue roundings a launch gets (gemm_cases.staged).  Around the operands: ldx1 > C1 and ldx2 > C2 with NaN in the gap, NaN in front
of and behind every operand in its allocation, outputs start as NaN with ldo > Nout and keep that bit pattern outside [M) x [Nout),
split-K workspaces start as NaN, arrival counters are zero before and after.  Every case prints an `ENV` line: the worst
|error| / bound per row regime and (c:) per channel regime.

The sibling kernels run their plain paths (bias, the per-sample row bias of the convs, residual; pro = 0) on one planted linear and
one planted conv shape each, in every schedule / geometry / patch / K-group count / order their own GPU tests enumerate.  Where two
kernels are documented as bit-identical (wsgemm and rowgemm fragment packing, rowchain against its unfused launches) the existing
torch.equal tests stay the check.

Elsewhere: the norm-folding prologues (pro != 0, the LayerNorm fold) with their GEGLU and V^T forms, the rowchain stages and
clip_linear have test_gpu_fused_envelope.py (fused_cases.py); the GroupNorm-statistics epilogue has norm_cases.check_acc.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gemm_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
FRONT = 16                                           # halfs (fp32 operands: floats) of NaN in front of every operand: keeps 16-byte alignment


@pytest.fixture(scope="module")
def L():
    from live2diff_amd import _lib, ops
    print("device:", _lib.device_name())
    return ops


def guarded(t2d, ld: int, off: int = FRONT, back: int = 64):
    """t2d [rows, cols] -> a flat device buffer of NaN with row r at [off + r ld, off + r ld + cols)"""
    rows, cols = t2d.shape
    assert ld >= cols
    buf = torch.full((off + rows * ld + back,), NAN, dtype=t2d.dtype)
    buf[off:off + rows * ld].view(rows, ld)[:, :cols] = t2d
    return buf.to(DEV)


_DEV = {}


def operands(case):
    """the device side of a case: x1 / x2 with 8 NaN halfs behind every row, the packed weights, bias, row bias (pitch 200, shifted by
    72 floats as the UNet's time-embedding table is) -- uploaded once per case"""
    key = case["key"]
    if key not in _DEV:
        C1, C2 = case["C1"], case["C2"]
        d = dict(x1=guarded(case["x1"], C1 + 8), w=guarded(gc.packed_weight(case), case["taps"] * case["CinP"]),
                 bias=guarded(case["bias"][None], case["Nout"]), rowbias=guarded(case["rowbias"], 200, off=FRONT + 72))
        d["x2"] = guarded(case["x2"], C2 + 8) if C2 else None
        _DEV[key] = d
    return _DEV[key]


def launch(L, s, case=None, order=0, reps=1, w_dev=None, bias_dev=None):
    """runs one spec; returns the [M, NoutO] output (after checking everything around it) of every repeat"""
    case = gc.case_of(s["key"]) if case is None else case
    d = operands(case)
    M, Nout, NoutO, ldo, C1, C2 = case["M"], case["Nout"], s["NoutO"], s["ldo"], case["C1"], case["C2"]
    S, fused, tile = s["S"], s["fused"], s["tile"]
    off = FRONT + s["out_off"]
    kw = dict(M=M, Nout=Nout, C1=C1, ldx1=C1 + 8, CinP=case["CinP"], ldo=ldo, x1_off=FRONT, w_off=FRONT, out_off=off, epi=s["epi"],
              splitk=S, tile=tile + (32 if s["direct"] else 0), variant=s["variant"], order=order)
    if C2:
        kw.update(x2=d["x2"][FRONT:], C2=C2, ldx2=C2 + 8)
    if case["conv"]:
        kw.update(taps=9, B=case["B"], Hin=case["Hin"], Win=case["Win"], Hout=case["Hout"], Wout=case["Wout"], stride=case["stride"],
                  ups=case["ups"], pad_same=case["pad"] == 0)
    if s["bias"]:
        kw["bias"] = (d["bias"] if bias_dev is None else bias_dev)[FRONT:]
    if s["rowbias"]:
        kw.update(rowbias=d["rowbias"][FRONT + 72:], ldrb=200, rows_per_bias=case["rows_per_bias"])
    if s["res"]:
        rkey = (case["key"], "res", s["ldr"], s["res_off"])
        if rkey not in _DEV:
            _DEV[rkey] = guarded(case["res"], s["ldr"], off=FRONT + s["res_off"])
        kw.update(res=_DEV[rkey], ldr=s["ldr"], res_off=FRONT + s["res_off"])
    cnt = None
    if S > 1:
        n_ws, n_cnt = L.splitk_sizes(M, Nout, S, 1, tile) if fused else (S * M * gc.round_up(Nout, 4), 0)
        kw["ws"] = torch.full((n_ws,), NAN, dtype=torch.float32, device=DEV)
        if fused:
            cnt = torch.zeros(3 + n_cnt, dtype=torch.int32, device=DEV)
            kw.update(cnt=cnt, cnt_off=3)
    proto = torch.full((off + M * ldo + 64,), NAN, dtype=torch.float16, device=DEV)
    outs = []
    for _ in range(reps):
        out = proto.clone()
        L.run(L.igemm(d["x1"], d["w"] if w_dev is None else w_dev, out, **kw))
        torch.cuda.synchronize()
        assert cnt is None or int(cnt.abs().sum()) == 0, f"{s['what']}: arrival counters not back at zero"
        body = out[off:off + M * ldo].view(M, ldo)
        got = body[:, :NoutO].clone()
        body[:, :NoutO] = NAN
        assert torch.equal(out.view(torch.int16), proto.view(torch.int16)), f"{s['what']}: a half outside [M) x [Nout) was written"
        outs.append(got.cpu())
    return outs


def check(L, s, orders=(0, 1), reps=1, agg=None, **kw):
    """one spec on the device: every element within the bound, single-product elements bit-equal to the restatement (epi 0, 3, 4),
    both tile orders and all repeats bit-equal"""
    case = gc.case_of(s["key"])
    exact, bnd, rnd, restated = gc.expected(s)
    outs = [o for order in orders for o in launch(L, s, order=order, reps=reps, **kw)]
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), f"{s['what']}: tile orders / repeats differ"
    got = outs[0]
    worst = gc.judge("igemm", s["what"], got, exact, bnd, case, chans=gc.out_chans(s), show_rnd=rnd)
    if s["epi"] in (0, 3, 4):
        one = gc.single_product(case)
        same = got.view(torch.int16) == restated.view(torch.int16)
        same |= (got == 0) & (restated == 0)                                   # (+0 / -0)
        bad = one & ~same
        assert not bad.any(), (f"{s['what']}: {int(bad.sum())} single-product elements differ from the {'staged' if s['staged'] else 'direct'} "
                               f"restatement, first at {bad.nonzero()[0].tolist()}: got {float(got[bad][0])!r}, restated {float(restated[bad][0])!r}")
    if agg is not None:
        for k, v in worst.items():
            agg[k] = max(agg.get(k, 0.0), v)
    return got


# ----------------------------------------------------------------------------- a. every pipeline shape
@pytest.mark.parametrize("tile,variant", [(t, v) for t in (1, 2) for v, (_bk, _ns, big) in gc.VARIANTS.items() if t == 2 or big])
def test_igemm_every_pipeline_shape(L, tile, variant):
    """BK 32 / 64 / 128 with 2 to 6 ring stages on both tiles: linear, the fast 3x3 gather, the generic one (concat, ups = 1); K loops from
    one step (fewer than the ring has stages: the prologue's `if (kb + s < ke)` and the drain alone) to 90; the channel tail C1 = 72 in
    CinP = 128; token-tile-major and weight-tile-major order bit-equal"""
    for s in gc.specs_variants(tile, variant):
        check(L, s)


def test_igemm_refuses_what_launch_p_does_not_offer(L):
    from live2diff_amd import _lib
    for variant, (_bk, _ns, big) in gc.VARIANTS.items():
        if not big:
            with pytest.raises(_lib.L2DError):
                launch(L, gc.spec("lin K128", gc.lin_key(C1=128), variant=variant, tile=1))
    with pytest.raises(_lib.L2DError):                                          # BK 128 needs CinP % 128 == 0
        launch(L, gc.spec("lin K64", gc.lin_key(C1=64), variant=6))


# ----------------------------------------------------------------------------- b. split-K
@pytest.mark.parametrize("tile", [1, 2])
def test_igemm_splitk(L, tile):
    """two-launch and fused reduction: uneven shares, a split shorter than the ring, splits that own no K step at all (S = Kp / 64 on a
    BK 128 shape passes the launcher's validation: the kernel guards every issue with `kb < ke` and parks a zero tile); three repeats
    bit-equal; the fused form -- staged epilogue, two roundings around the residual -- is held to its own restatement"""
    for s in gc.specs_splitk(tile):
        check(L, s, orders=(0,), reps=3)


# ----------------------------------------------------------------------------- c. epilogues
def test_igemm_epilogues_staged_and_direct(L):
    """epi 0, 2, 3, 4, 5 with and without residual at Nout = 136 (staged; direct by tile + 32, by ldo % 8 = 4, by an output pointer 8 bytes
    off, by a residual pitch % 8 = 4) and Nout = 70 (always direct, ragged last channel group); row bias every 50 rows across 64- and
    128-row tiles through a shifted pointer"""
    for s in gc.specs_epilogues():
        check(L, s, orders=(0,))


def test_igemm_geglu(L):
    for s in gc.specs_geglu():
        case = gc.case_of(s["key"])
        key = (s["key"], "geglu")
        if key not in _DEV:
            wp, bp = L.pack_geglu(gc.packed_weight(case).to(DEV), case["bias"].to(DEV))
            _DEV[key] = (guarded(wp.cpu(), wp.shape[1]), guarded(bp.cpu()[None], case["Nout"]))
        check(L, s, orders=(0,), w_dev=_DEV[key][0], bias_dev=_DEV[key][1])


def test_igemm_swapped_batched_odd_t(L):
    """V^T[b] = Wv X[b]^T with T = 49: operand roles swapped, batch over grid.z, Nout = 49 (the ragged direct epilogue, `so` a multiple
    of 8).  The planted `rows` are the rows of Wv, the `channels` the 3 x 49 tokens."""
    Bz, T, C = 3, 49, 128
    key = gc.lin_key(C1=C, Nout=Bz * T, seed=30, B=1, T=C)
    case = gc.case_of(key)
    y, A = case["y"], case["A"]
    exact, bnd, rnd = gc.exact_and_bound(case, y, A, bias=False)
    assert not gc.staged(ldo=56, Nout=T, so=C * 56, z=1)
    restated = gc.restate(case, bk=64, bias=False)
    d = operands(case)
    ld = 56
    proto = torch.full((FRONT + Bz * C * ld + 64,), NAN, dtype=torch.float16, device=DEV)
    for tile in (1, 2):
        out = proto.clone()
        L.run(L.igemm(d["x1"], d["w"], out, M=C, Nout=T, C1=C, ldx1=C + 8, CinP=C, ldo=ld, batch=Bz, sx1=0, sw=T * C, so=C * ld,
                      x1_off=FRONT, w_off=FRONT, out_off=FRONT, tile=tile))
        torch.cuda.synchronize()
        body = out[FRONT:FRONT + Bz * C * ld].view(Bz, C, ld)
        got = body[:, :, :T].permute(1, 0, 2).reshape(C, Bz * T).cpu()
        body[:, :, :T] = NAN
        assert torch.equal(out.view(torch.int16), proto.view(torch.int16))
        gc.judge("igemm", f"swapped batched V^T T49 t{tile}", got, exact, bnd, case, show_rnd=rnd)
        one = gc.single_product(case)
        assert torch.equal(got[one], restated[one])


# ----------------------------------------------------------------------------- d. conv geometry
def test_igemm_conv_geometry(L):
    """stride 2 on odd and even sizes, TF-SAME low-side padding, nearest-2x upsampling, the 8 + 72 concat, 1 x 1 / 1 x 6 / 7 x 1 images,
    the +-1e3 wall sample first, in the middle and last in the batch"""
    for s in gc.specs_geometry():
        check(L, s)


# ----------------------------------------------------------------------------- e. skinny_linear (the siblings follow below)
def test_skinny_linear(L):
    for s in gc.specs_skinny():
        case = gc.case_of(s["key"])
        exact, bnd, rnd, restated = gc.expected_skinny(s)
        M, K, N = case["M"], case["K"], case["Nout"]
        a = guarded(case["x1"], K + 8)
        w = case["w"].contiguous().to(DEV)
        ldo = N + 2
        proto = torch.full((M * ldo,), NAN, dtype=torch.float32 if s["f32"] else torch.float16, device=DEV)
        out = proto.clone()
        L.run(L.skinny_linear(a, w, case["bias"].to(DEV), out, M=M, K=K, Nout=N, silu_out=s["silu"], ldo=ldo, lda=K + 8, a_off=FRONT))
        torch.cuda.synchronize()
        body = out.view(M, ldo)
        got = body[:, :N].clone().cpu()
        body[:, :N] = NAN
        itype = torch.int32 if s["f32"] else torch.int16
        assert torch.equal(out.view(itype), proto.view(itype))
        gc.judge("skinny_linear", s["what"], got, exact, bnd, case, show_rnd=rnd)
        if not s["silu"]:
            one = gc.single_product(case)
            assert torch.equal(got[one], restated[one])


# ----------------------------------------------------------------------------- e. the sibling kernels, plain paths
def sibling_io(case, rowbias):
    """x1 / x2 / residual / bias / row bias behind NaN guards and with NaN in every row's gap; pointers stay 16-byte aligned"""
    d = operands(case)
    rkey = (case["key"], "res", case["Nout"] + 8, 0)
    if rkey not in _DEV:
        _DEV[rkey] = guarded(case["res"], case["Nout"] + 8)
    io = dict(x1=d["x1"][FRONT:], ldx1=case["C1"] + 8, res=_DEV[rkey][FRONT:], ldr=case["Nout"] + 8, bias=d["bias"][FRONT:FRONT + case["Nout"]])
    if case["C2"]:
        io.update(x2=d["x2"][FRONT:], C2=case["C2"], ldx2=case["C2"] + 8)
    if rowbias:
        io.update(rowbias=d["rowbias"][FRONT + 72:], ldrb=200, rows_per_bias=case["rows_per_bias"])
    return io


def sibling_check(kernel, what, run, case, rowbias, S=1, reps=1):
    """run(out_view, ldo) launches into a NaN-filled output with ldo = Nout + 8"""
    M, N = case["M"], case["Nout"]
    ldo = N + 8
    exact, bnd, rnd, restated = gc.expected_sibling(kernel, case["key"], rowbias, S)
    proto = torch.full((FRONT + M * ldo + 64,), NAN, dtype=torch.float16, device=DEV)
    first = None
    for _ in range(reps):
        out = proto.clone()
        run(out[FRONT:], ldo)
        torch.cuda.synchronize()
        body = out[FRONT:FRONT + M * ldo].view(M, ldo)
        got = body[:, :N].clone().cpu()
        body[:, :N] = NAN
        assert torch.equal(out.view(torch.int16), proto.view(torch.int16)), f"{kernel} {what}: a half outside [M) x [Nout) was written"
        assert first is None or torch.equal(got.view(torch.int16), first.view(torch.int16)), f"{kernel} {what}: repeats differ"
        first = got
    gc.judge(kernel, what, first, exact, bnd, case, show_rnd=rnd)
    one = gc.single_product(case)
    same = (first.view(torch.int16) == restated.view(torch.int16)) | ((first == 0) & (restated == 0))
    assert not (one & ~same).any(), f"{kernel} {what}: {int((one & ~same).sum())} single-product elements differ from the staged restatement"


def _ws_geoms(tiles):
    return [(nw, nt) for nt in (1, 2) for nw in range(1, 11 if nt == 1 else 5) if tiles % (nw * nt) == 0]


def _ws_bufs(L, M, N, sched):
    NW, NT, _NL, S, _ntw = sched
    if S <= 1:
        return {}
    nws, ncnt = L.wsgemm_sizes(M, N, NW, NT, S)
    return dict(ws=torch.full((nws,), NAN, dtype=torch.float32, device=DEV), cnt=torch.zeros(ncnt + 4, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("key", [gc.SIB_LIN, gc.SIB_LIN_CAT])
def test_wsgemm_linear(L, key):
    """every (NW, NT) block geometry with one / two loader waves, temporal / non-temporal weight loads and 1, 2, 3 K slices (K = 192: three
    64-channel chunks), as test_wsgemm_every_geometry enumerates them"""
    case = gc.case_of(key)
    io = sibling_io(case, False)
    M, N, K = case["M"], case["Nout"], case["K"]
    wp, bp, _ = L.pack_wsgemm(case["w"].to(DEV), io.pop("bias"))
    for nw, nt in _ws_geoms(N // 32):
        for nl, S, ntw in ((1, 1, False), (2, 1, True), (1, 3, True), (2, K // 64, False), (1, 2, False)):
            sched = (nw, nt, nl, S, ntw)
            bufs = _ws_bufs(L, M, N, sched)

            def run(out, ldo):
                L.run(L.wsgemm(io["x1"], wp, out, M=M, Nout=N, C1=case["C1"], ldx1=io["ldx1"], ldo=ldo, x2=io.get("x2"), C2=case["C2"],
                               ldx2=io.get("ldx2", 0), bias=bp, res=io["res"], ldr=io["ldr"], sched=sched, **bufs))
                assert not bufs or int(bufs["cnt"].abs().sum()) == 0
            sibling_check("wsgemm", f"lin {case['C1']}+{case['C2']} sched {sched}", run, case, False, S=S, reps=2 if S > 1 else 1)


@pytest.mark.parametrize("key", [gc.SIB_CONV, gc.SIB_CONV_CAT])
def test_wsgemm_conv3x3(L, key):
    case = gc.case_of(key)
    io = sibling_io(case, True)
    M, N, K = case["M"], case["Nout"], case["K"]
    wp = L.pack_wsgemm_conv3x3(gc.weight_nchw(case).to(DEV))
    bias = io.pop("bias").contiguous()
    scheds = [L.wsgemm_schedule(M, 9 * K, N, taps=9)] + [(nw, nt, nl, S, False) for (nw, nt), nl, S in
                                                          zip(_ws_geoms(N // 32)[:4], (1, 2, 1, 2), (1, 5, 9, 2))]
    for sched in scheds:
        bufs = _ws_bufs(L, M, N, sched)

        def run(out, ldo):
            L.run(L.wsgemm(io["x1"], wp, out, M=M, Nout=N, C1=case["C1"], ldx1=io["ldx1"], ldo=ldo, x2=io.get("x2"), C2=case["C2"],
                           ldx2=io.get("ldx2", 0), bias=bias, rowbias=io["rowbias"], ldrb=io["ldrb"], rows_per_bias=io["rows_per_bias"],
                           res=io["res"], ldr=io["ldr"], taps=9, B=case["B"], H=case["Hin"], W=case["Win"], sched=sched, **bufs))
            assert not bufs or int(bufs["cnt"].abs().sum()) == 0
        sibling_check("wsgemm", f"conv {case['C1']}+{case['C2']} sched {tuple(sched)}", run, case, True, S=sched[3], reps=2 if sched[3] > 1 else 1)


def test_rowgemm_linear(L):
    """pro = 0, every (NW, NT, MT) geometry of test_rowgemm_every_geometry's rule, both tile orders"""
    case = gc.case_of(gc.SIB_LIN)
    io = sibling_io(case, False)
    M, N, K = case["M"], case["Nout"], case["K"]
    assert L.rowgemm_ok(N, K)
    wp, bp = L.pack_rowgemm(case["w"].to(DEV), io.pop("bias"))
    tiles = N // 32
    geoms = [(nw, nt, mt) for mt in (1, 2) for nt in (1, 2, 3, 4) if not (mt >= 2 and nt > 2) for nw in range(1, (5 if nt >= 3 else 8) + 1)
             if tiles % (nw * nt) == 0]
    assert len(geoms) >= 8
    for sched in geoms:
        for order in (0, 1):
            def run(out, ldo):
                L.run(L.rowgemm(io["x1"], wp, out, M=M, K=K, Nout=N, ldx=io["ldx1"], ldo=ldo, bias=bp, res=io["res"], ldr=io["ldr"],
                                sched=sched, order=order))
            sibling_check("rowgemm", f"lin sched {sched} order {order}", run, case, False)


@pytest.mark.parametrize("key", [gc.SIB_CONV, gc.SIB_CONV_CAT])
def test_pconv(L, key):
    case = gc.case_of(key)
    io = sibling_io(case, True)
    N = case["Nout"]
    wp = L.pack_conv3x3(gc.weight_nchw(case).to(DEV))
    bias = io.pop("bias").contiguous()
    for patch in ((8, 16), (8, 8), (4, 8)):
        for order in (0, 1):
            def run(out, ldo):
                L.run(L.pconv(io["x1"], wp, out, B=case["B"], H=case["Hin"], W=case["Win"], C1=case["C1"], ldx1=io["ldx1"], CinP=case["K"],
                              Nout=N, ldo=ldo, patch=patch, x2=io.get("x2"), C2=case["C2"], ldx2=io.get("ldx2", 0), bias=bias,
                              rowbias=io["rowbias"], ldrb=io["ldrb"], rows_per_bias=io["rows_per_bias"], res=io["res"], ldr=io["ldr"],
                              order=order))
            sibling_check("pconv", f"conv {case['C1']}+{case['C2']} patch {patch} order {order}", run, case, True)


@pytest.mark.parametrize("key", [gc.SIB_CONV, gc.SIB_CONV_CAT])
def test_cconv(L, key):
    """(CG, KG) = (1, 4) and (2, 2) with 1, 2, 4 loader waves; K slices over the two chunks of the concat case"""
    case = gc.case_of(key)
    io = sibling_io(case, True)
    N, nch = case["Nout"], case["K"] // 64
    assert L.cconv_ok(case["Hin"], case["Win"], N, case["C1"], case["C2"])
    bias = io.pop("bias").contiguous()
    packed = {kg: L.pack_cconv(gc.weight_nchw(case).to(DEV), kg) for kg in (2, 4)}
    for cg, kg in ((1, 4), (2, 2)):
        for nld in (1, 2, 4):
            for S in range(1, nch + 1):
                sched = (cg, kg, nld, S)
                ws = cnt = None
                if S > 1:
                    nws, ncnt = L.cconv_sizes(case["B"], case["Hin"], case["Win"], N, cg, S)
                    ws = torch.full((nws,), NAN, dtype=torch.float32, device=DEV)
                    cnt = torch.zeros(ncnt + 3, dtype=torch.int32, device=DEV)

                def run(out, ldo):
                    L.run(L.cconv(io["x1"], packed[kg], out, B=case["B"], H=case["Hin"], W=case["Win"], C1=case["C1"], ldx1=io["ldx1"], Nout=N,
                                  ldo=ldo, KG=kg, x2=io.get("x2"), C2=case["C2"], ldx2=io.get("ldx2", 0), bias=bias, rowbias=io["rowbias"],
                                  ldrb=io["ldrb"], rows_per_bias=io["rows_per_bias"], res=io["res"], ldr=io["ldr"], sched=sched, ws=ws,
                                  cnt=cnt, cnt_off=3))
                    assert cnt is None or int(cnt.abs().sum()) == 0
                sibling_check("cconv", f"conv {case['C1']}+{case['C2']} sched {sched}", run, case, True, S=S * kg, reps=2 if S > 1 else 1)
