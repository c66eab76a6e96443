"""-m gpu: the fused forms of the row kernels per output ELEMENT on planted data, through the C ABI (helpers, regimes, references, the
bound and its derivation: fused_cases.py; the bound is first shown to hold for plain-torch restatements and to catch every mutant:
test_fused_envelope_cpu.py).

rowgemm behind its LayerNorm and GroupNorm prologues, with GEGLU and with the transposed V^T part; wsgemm with the accumulator-side
LayerNorm fold, with GEGLU, V^T and split-K; the four rowchain head segments and the rowchain tail, each stage against fp64 from the
device's own previous stage and the whole bit-identical to the launches it replaces; clip_linear.  Around the operands: NaN in front
of and behind every activation and residual and in every row's pitch gap (ld = cols + 8), outputs start as NaN and keep that bit
pattern outside [M) x [Nout), V^T columns >= T keep it too, split-K slabs start as NaN, arrival counters are zero afterwards, and a
split-K launch runs twice with bit-equal results.  Every case prints one `ENV` line: the worst |got - ref| / bound per row regime and
(c:) per channel regime.  No element is excluded; the fold's r100 rows are printed and asserted finite (fused_cases.RECORDED_FOLD).
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import fused_cases as fc  # noqa: E402
import gemm_cases as gc  # noqa: E402
import norm_cases as nc  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
FRONT = fc.FRONT


@pytest.fixture(scope="module")
def L():
    from live2diff_amd import _lib, ops
    print("device:", _lib.device_name())
    return ops


def take(out, proto, rows: int, ld: int, cols: int, what: str):
    """the [rows, cols] body of a guarded output; everything else must still carry the prototype's bits"""
    body = out[FRONT:FRONT + rows * ld].view(rows, ld)
    got = body[:, :cols].clone()
    body[:, :cols] = NAN
    itype = torch.int16 if out.dtype == torch.float16 else torch.int32
    assert torch.equal(out.view(itype), proto.view(itype)), f"{what}: an element outside [M) x [Nout) was written"
    return got.cpu()


_DEV = {}


def dev_case(case):
    """the device side of a case, uploaded once"""
    if case["key"] not in _DEV:
        _DEV[case["key"]] = fc.operands(case, DEV)
    return _DEV[case["key"]]


def same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def launch_rows(L, case, what, build):
    """One launch of a case into NaN-filled outputs.  build(out, vt, ldo, ldt) returns the op.  Returns got [M, NoutO] with the V^T
    part transposed back behind the row-major columns."""
    M, B, T, ntr = case["M"], case["B"], case["T"], case["ntr"]
    proto, vproto, ldo, ldt = fc.out_buffers(case, DEV)
    out, vt = proto.clone(), (vproto.clone() if ntr else None)
    L.run(build(out, vt, ldo, ldt))
    torch.cuda.synchronize()
    got = take(out, proto, M, ldo, case["NoutO"] - ntr, what)
    if ntr:
        gv = take(vt, vproto, B * ntr, ldt, T, what + " V^T (columns >= T)").view(B, ntr, T)
        got = torch.cat([got, fc.vt_back(gv, B, T)], 1)
    return got


def rowgemm_launch(L, case, sched, order):
    d = dev_case(case)
    return launch_rows(L, case, f"{case['key'][:3]} sched {sched} order {order}",
                       lambda out, vt, ldo, ldt: fc.rowgemm_op(L, case, d, out, vt, ldo, ldt, sched, order))


def rowgemm_check(L, name, case, geoms, orders=(0, 1)):
    """every geometry and order of one case: each output judged per element; one ENV line for the first and for every output whose
    bits differ from it"""
    ex, restated = fc.expected(case)
    first = None
    for sched in geoms:
        for order in orders:
            got = rowgemm_launch(L, case, sched, order)
            new = first is None or not same_bits(got, first)
            fc.judge("rowgemm", f"{name} K{case['K']} N{case['Nout']}{' +res' if case['res'] is not None else ''} sched {sched} order {order}",
                     got, ex, quiet=not new)
            if case["pro"] == 1 and case["epi"] == 0:
                fc.check_const_rows("rowgemm", f"{name} sched {sched}", got, restated, case["rows"])
            first = got if first is None else first


# ----------------------------------------------------------------------------- 1. rowgemm LayerNorm + linear
@pytest.mark.parametrize("i", range(9))
def test_rowgemm_layernorm_linear(L, i):
    """pro = 1 at M = 150: K = 320 (the row in registers), K = 1280 / Nout = 64 (through LDS), K = 1280 with 8 waves (16 lanes per row),
    K = 64 (generic k loop); every (NW, NT, MT) geometry for Nout = 96 / 64 in both orders; bias, and bias + residual"""
    case, geoms = fc.rowgemm_ln_cases()[i]
    rowgemm_check(L, "LN + linear", case, geoms)


# ----------------------------------------------------------------------------- 2. rowgemm LayerNorm + GEGLU
@pytest.mark.parametrize("i", range(2))
def test_rowgemm_layernorm_geglu(L, i):
    case, geoms = fc.rowgemm_geglu_cases()[i]
    rowgemm_check(L, "LN + GEGLU", case, geoms, orders=(0,) if i else (0, 1))


# ----------------------------------------------------------------------------- 3. rowgemm GroupNorm + linear
@pytest.mark.parametrize("i", range(2))
def test_rowgemm_groupnorm_linear(L, i):
    """pro = 2 on exact accumulators: (B, T, C) = (3, 32, 320) and (2, 64, 64), every (sample, group) its own regime"""
    case, geoms = fc.rowgemm_gn_cases()[i]
    rowgemm_check(L, "GN + linear", case, geoms)


# ----------------------------------------------------------------------------- 4. rowgemm q | k | V^T
@pytest.mark.parametrize("i", range(2))
def test_rowgemm_qkv_with_transposed_v(L, i):
    """ldt = T + 8: the V^T columns >= T keep their NaN; V^T is judged with the row-major bound (a store path)"""
    case, geoms = fc.rowgemm_qkv_cases()[i]
    rowgemm_check(L, "LN + q|k|V^T", case, geoms, orders=(0,))


# ----------------------------------------------------------------------------- 5, 6. wsgemm fold
def wsgemm_check(L, name, case, scheds):
    d = dev_case(case)
    for sched in scheds:
        S = sched[3]
        ex, _restated = fc.expected(case, S)
        what = f"{name} K{case['K']} N{case['Nout']} sched {tuple(sched)}"
        ws, cnt = fc.wsgemm_bufs(L, case, sched, DEV)
        outs = []
        for _ in range(2 if S > 1 else 1):
            if S > 1:
                ws.fill_(NAN)
            outs.append(launch_rows(L, case, what, lambda out, vt, ldo, ldt: fc.wsgemm_op(L, case, d, out, vt, ldo, ldt, sched, ws, cnt)))
            assert cnt is None or int(cnt.abs().sum()) == 0, f"{what}: arrival counters not back at zero"
        assert len(outs) == 1 or same_bits(outs[0], outs[1]), f"{what}: two launches differ"
        fc.judge("wsgemm", what, outs[0], ex, recorded=fc.RECORDED_FOLD)


@pytest.mark.parametrize("i", range(2))
def test_wsgemm_fold_linear(L, i):
    """K = 320 and 1280 at M = 150 with bias + residual: both loader counts, temporal and non-temporal weight loads, split-K with even
    and uneven shares of the 64-channel chunks"""
    case, scheds = fc.wsgemm_fold_cases()[i]
    wsgemm_check(L, "fold + linear", case, scheds)


def test_wsgemm_fold_geglu(L):
    """Nout = 32 (16 output columns): the smallest the packer accepts; the default schedule and two forced split-K ones"""
    case = fc.wsgemm_geglu_case()
    wsgemm_check(L, "fold + GEGLU", case, fc.wsgemm_geglu_scheds(L, case))


def test_wsgemm_fold_transposed_v(L):
    """q | k | V^T behind the fold; the launcher refuses split-K with a transposed part, so the forced schedules vary loaders and loads"""
    from live2diff_amd import _lib
    case = fc.wsgemm_qkv_case()
    wsgemm_check(L, "fold + q|k|V^T", case, fc.wsgemm_qkv_scheds(L, case))
    with pytest.raises(_lib.L2DError):
        wsgemm_check(L, "fold + q|k|V^T", case, [(1, 1, 1, 2, False)])


# ----------------------------------------------------------------------------- 7. rowchain head segments
def _run_ops(ops_and_keeps):
    from live2diff_amd import _lib
    pl = _lib.OpList()
    for op, keep in ops_and_keeps:
        pl.append(op, *keep)
    pl.run()
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,T", fc.HEAD_SHAPES)
@pytest.mark.parametrize("kind", fc.HEAD_KINDS)
def test_rowchain_head_segments(L, kind, B, T):
    """h is stored and judged per element against fp64 from the inputs; out | V^T against fp64 from the device's own h, so that
    nothing compounds.  The res kinds run bA = 0 with every third x row zero: h = resA there bit for bit, and the LayerNorm of stage 2
    meets the planted row regimes.  Then everything bit-identical to the two rowgemm launches the segment replaces."""
    case = fc.head_case(kind, B, T)
    C, M, trl, ncol = case["C"], case["M"], case["trl"], case["ncol"]
    ld, ldo, ldt = C + 8, ncol + 8, T + 8
    d = fc.head_operands(case, DEV, ld)
    protos = (fc.nan_buf(M, ld, DEV), fc.nan_buf(M, ldo, DEV), fc.nan_buf(B * C, ldt, DEV) if trl else None)

    def run(fused):
        h, o, v = (None if p is None else p.clone() for p in protos)
        _run_ops(fc.head_ops(L, case, d, h, o, v, ld=ld, ldo=ldo, ldt=ldt, fused=fused))
        what = f"{kind} B{B} T{T} {'fused' if fused else 'two launches'}"
        gh, go = take(h, protos[0], M, ld, C, what + " h"), take(o, protos[1], M, ldo, ncol, what + " out")
        if trl:
            gv = take(v, protos[2], B * C, ldt, T, what + " V^T (columns >= T)").view(B, C, T)
            go = torch.cat([go, fc.vt_back(gv, B, T)], 1)
        return gh, go
    gh, go = run(True)
    ex1, _ = fc.head_stage1(case)
    fc.judge("rowchain", f"head {kind} B{B} T{T} stage 1 (h)", gh, ex1)
    if not case["gnp"]:
        assert same_bits(gh[::3], case["resA"][::3]), "a zero x row with bA = 0 must store resA"
    ex2, rs2 = fc.head_stage2(case, gh)
    fc.judge("rowchain", f"head {kind} B{B} T{T} stage 2 (out{' | V^T' if trl else ''})", go, ex2)
    fc.check_const_rows("rowchain", f"head {kind} stage 2", go, rs2, case["rows2"])
    uh, uo = run(False)
    assert same_bits(gh, uh) and same_bits(go, uo), f"head {kind}: not bit-identical to the two rowgemm launches"


# ----------------------------------------------------------------------------- 8. rowchain tail
@pytest.mark.parametrize("B,T", fc.TAIL_SHAPES)
def test_rowchain_tail(L, B, T):
    """The chain stores no intermediates: the four unfused launches run on the same planted data and every stage is judged per element
    against fp64 from the device's previous stage; then the chain's out must carry o4's bits -- also through column-sliced operands
    (ld > C) -- and its GroupNorm accumulators stay within norm_cases.check_acc."""
    case = fc.tail_case(B, T)
    C, M = case["C"], case["M"]
    ld = C + 8
    d = fc.tail_operands(case, DEV, ld)
    protos = [fc.nan_buf(M, ld, DEV), fc.nan_buf(M, 4 * C + 8, DEV), fc.nan_buf(M, ld, DEV), fc.nan_buf(M, ld, DEV)]
    bufs = [p.clone() for p in protos]
    _run_ops(fc.tail_unfused_ops(L, case, d, *bufs, ld))
    assert gc.staged(ldo=ld, Nout=C, res=True, ldr=ld, out_off=FRONT, res_off=FRONT)
    stages = [take(b.clone(), p, M, l, c, f"tail stage {i + 1}") for i, (b, p, l, c) in
              enumerate(zip(bufs, protos, (ld, 4 * C + 8, ld, ld), (C, 4 * C, C, C)))]
    prev = case["a"]
    for i, got in enumerate(stages, 1):
        ex, rs = fc.tail_stage(case, i, prev, h2=stages[0])
        fc.judge("rowchain", f"tail B{B} T{T} stage {i} ({('h2', 'hid', 'h3', 'o4')[i - 1]})", got, ex)
        prev = got
    assert same_bits(stages[0][::3], case["res1"][::3]), "a zero row of a with b_out = 0 must give h2 = res1"
    o4 = stages[3]
    # the chain, with its GroupNorm statistics
    out = protos[3].clone()
    acc = torch.zeros(B, fc.G, 2, dtype=torch.int64, device=DEV)
    op, keep = fc.tail_chain_op(L, case, d, out, ld)
    assert L.gn_target(op, acc.data_ptr(), T=T, G=fc.G, cpg=C // fc.G, choff=0)
    _run_ops([(op, keep + (acc,))])
    got = take(out, protos[3], M, ld, C, "tail chain")
    assert same_bits(got, o4), f"rowchain vs the four separate launches: not bit-identical (rel-L2 {gc.rel_l2(got, o4):.3e})"
    nc.check_acc(acc, got.view(B, T, C), fc.G, C // fc.G, 0, what="rowchain tail statistics")
    # operands that are column slices of wider buffers
    wide = lambda t, cols, at: torch.full((M, cols), NAN, dtype=torch.float16).index_copy_(1, torch.arange(at, at + C), t).to(DEV)
    A, R1, R2 = wide(case["a"], 3 * C, C), wide(case["res1"], 2 * C, 0), wide(case["res2"], C + 64, 0)
    O = torch.full((M, 2 * C), NAN, dtype=torch.float16, device=DEV)
    pk = {k: d[k] for k in ("w_out", "b_out", "w_ff1", "b_ff1", "w_ff2", "b_ff2", "w_po", "b_po")}
    op, keep = L.rowchain(A, R1, R2, O, M=M, C=C, eps=fc.EPS_LN, lda=3 * C, ldr1=2 * C, ldr2=C + 64, ldo=2 * C, **pk)
    op.p[0] = A.data_ptr() + 2 * C
    op.p[3] = O.data_ptr() + 2 * C
    _run_ops([(op, keep)])
    Oc = O.cpu()
    assert same_bits(Oc[:, C:].contiguous(), o4), "column-sliced operands: not the bits of the four launches"
    assert torch.isnan(Oc[:, :C]).all(), "column-sliced output: a column outside the slice was written"


# ----------------------------------------------------------------------------- 9. clip_linear
@pytest.mark.parametrize("i", range(7))
def test_clip_linear(L, i):
    """the CLIP encoder's GEMM on gemm_cases' planted rows and channels at K = 192: bias with no epilogue, with quick_gelu and into the
    fp32 residual stream; its LayerNorm form (fp32 rows, gamma / beta in the kernel) on the planted LayerNorm rows at K = 192 and 384"""
    c = fc.clip_cases()[i]
    M, K, N = c["M"], c["K"], c["Nout"]
    ld, ldo = K + 8, N + 8
    f32_out = c["epi"] == 2
    x = fc.guarded(c["x"], ld).to(DEV)
    proto = fc.nan_buf(M, ldo, DEV, torch.float32 if f32_out else torch.float16)
    out = proto.clone()
    if f32_out:
        out[FRONT:FRONT + M * ldo].view(M, ldo)[:, :N] = c["res32"].to(DEV)
    dv = lambda t: None if t is None else t.to(DEV)
    op, keep = fc.clip_op(L, c, x, L.pack_clip_linear(c["w"].to(DEV)), c["bias"].to(DEV), out, dv(c["gamma"]), dv(c["beta"]), ld, ldo)
    L.run((op, keep + (x, out)))
    torch.cuda.synchronize()
    got = take(out, proto, M, ldo, N, f"clip_linear {c['name']}")
    ex = fc.clip_expect(c)
    fc.judge("clip_linear", c["name"], got, ex)
    if c["epi"] == 0 and not c["ln"]:                # single-product elements: the restatement's bits
        rs = fc.clip_restate(c)
        one = gc.single_product(dict(rows=c["rows"], chans=c["chans"]))
        same = (got.view(torch.int16) == rs.view(torch.int16)) | ((got == 0) & (rs == 0))
        assert not (one & ~same).any(), f"clip_linear {c['name']}: {int((one & ~same).sum())} single-product elements differ from the restatement"
