"""The envelope that test_gpu_norm_envelope.py asserts per (sample, group) is one the documented arithmetic stays inside: a plain torch
restatement of the single-pass fixed-point GroupNorm statistics (norm_cases.emulate) against fp64 GroupNorm on the planted tensor, at the
GPU test's shapes, must stay at or below HALF the GPU tolerance for every asserted regime and both eps values in use.  A regime that does
not is not asserted on the GPU either: it is listed in norm_cases.RECORDED and only measured there.  Also here: every producer accepts
the statistics request at the GPU test's shapes (a producer that declines would turn its GPU case into a no-op), and the identity-weight
packings the GPU tests rely on unpack to what the tests assume.

Measured with this helper at these shapes (B 2, T 256, C 320 / 640, G 32; worst (sample, group) error in units of the whole-tensor RMS
of the reference, over both widths, both eps values, with and without SiLU):
    benign 2.3e-4   r10 2.3e-4   r30 2.7e-4   r100 1.5e-3   small 3.2e-4   small_off 3.1e-4   large 2.4e-4   large_off 2.3e-4
    const 2.3e-4    outlier 4.6e-4   ramp 2.2e-4
    recorded only: s0.01 1.0e-3, s0.003 1.3e-2, r300 1.9e-2
Everything but r100 is at the floor of the fp16 output rounding.  r = 100 (1.2e-3 to 1.5e-3) does NOT stay within half of 2e-3: at
mean^2 = 1e4 one fp32 ulp of q / n and of mean^2 is 1e-3 of the variance each.  It therefore stays asserted, here and on the GPU,
against the 2e-2 that the project already accepts at |mean| / std = 100 for the LayerNorm fold (norm_cases.tol_of).  The
recorded-only regimes: std 0.003 (variance 9e-6: the size of eps and of the 2^-12 quantum per flush) and r = 300 miss the
half-tolerance by an order of magnitude; std 0.01 sits on it (1.0e-3 at C = 320, eps 1e-6).
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import norm_cases as nc  # noqa: E402


@pytest.fixture
def dry():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def _by_regime(err, nb, ng):
    worst = {}
    for b in range(nb):
        for g in range(ng):
            r = nc.regime_of(b, g)
            worst[r] = max(worst.get(r, 0.0), float(err[b, g]))
    return worst


def test_planted_layout():
    """every regime at least twice per sample, no two samples with the same layout, and the planted statistics are what the table says"""
    tab = nc.regime_table(nc.B, nc.G)
    for row in tab:
        for r in nc.REGIMES:
            assert row.count(r) >= 2, r
    assert tab[0] != tab[1]
    x = nc.planted(nc.B, nc.T, nc.C, nc.G, seed=1).double().view(nc.B, nc.T, nc.G, nc.C // nc.G)
    assert torch.isfinite(x).all()
    mean, std = x.mean((1, 3)), x.std((1, 3))
    for b in range(nc.B):
        for g in range(nc.G):
            r = nc.regime_of(b, g)
            if r in nc.MU_SIGMA:
                mu, sg = nc.MU_SIGMA[r]
                assert abs(mean[b, g] - mu) <= 0.1 * sg + 1e-3 * abs(mu) and abs(std[b, g] / sg - 1) <= 0.1, (r, mean[b, g], std[b, g])
            elif r == "const":
                assert std[b, g] == 0 and abs(mean[b, g] - nc.CONST) < 4e-3
    rows = nc.planted_rows(28, 320, seed=2)
    assert rows.shape == (28, 320) and not torch.equal(rows[0], rows[14])
    assert abs(rows[3].double().mean() + 100) < 0.5 and rows[8].double().std() == 0


@pytest.mark.parametrize("C", [320, 640])
@pytest.mark.parametrize("eps", [nc.EPS_RESNET, nc.EPS_TRANSFORMER])
@pytest.mark.parametrize("silu", [False, True])
def test_emulation_stays_within_half_the_gpu_tolerance(C, eps, silu, capsys):
    x = nc.planted(nc.B, nc.T, C, nc.G, seed=1)
    gm, bt = nc.affine(C)
    ref = nc.reference(x, nc.G, gm, bt, eps, silu)
    out = nc.emulate(x, nc.G, gm, bt, eps, silu)
    assert torch.isfinite(out.float()).all()
    worst = _by_regime(nc.group_errors(out, ref, nc.G), nc.B, nc.G)
    with capsys.disabled():
        print(f"\nemulation C {C} eps {eps:g} silu {int(silu)}: " + "  ".join(f"{r} {worst[r]:.2e}" for r in nc.REGIMES))
    for r in nc.ASSERTED:
        assert worst[r] <= nc.tol_of(r) / 2, f"{r}: {worst[r]:.3e} > {nc.tol_of(r) / 2:.1e}"
    # exact accumulators through the same decode: what part b of the GPU test feeds the consumers
    out2 = nc.decode(x, nc.exact_acc(x, nc.G), nc.G, gm, bt, eps, silu)
    worst2 = _by_regime(nc.group_errors(out2, ref, nc.G), nc.B, nc.G)
    for r in nc.ASSERTED:
        assert worst2[r] <= nc.tol_of(r) / 2, f"{r} (exact accumulators): {worst2[r]:.3e}"


def test_emulated_accumulators_are_inside_their_own_bounds():
    """acc_bounds is meant to hold for any fp32 summation order: the emulation, at 32 and at 128 tokens per flush, is one"""
    x = nc.planted(nc.B, nc.T, nc.C, nc.G, seed=1)
    for tpf in (32, 128):
        nc.check_acc(nc.emulate_acc(x, nc.G, tokens_per_flush=tpf), x, nc.G, nc.C // nc.G, 0, what=f"emulation {tpf}")
    s, q, sb, qb = nc.acc_bounds(x, nc.G, 2 * nc.C // nc.G, nc.C)
    assert float(s[:, :16].abs().max()) == 0 and float(sb[:, :16].max()) == 0 and float(qb[:, 16:].min()) > 0
    # a coarser quantum of sum x^2 (2^-8 instead of 2^-12) must NOT pass: the bound is tight enough to see it
    acc = nc.emulate_acc(x, nc.G)
    coarse = acc.clone()
    xf = x.double().view(nc.B, nc.T // 32, 32, nc.G, nc.C // nc.G)
    coarse[..., 1] = ((xf ** 2).sum((2, 4)) * 2 ** 8).round().sum(1).to(torch.int64) * 2 ** 4
    with pytest.raises(AssertionError):
        nc.check_acc(coarse, x, nc.G, nc.C // nc.G, 0)


@pytest.mark.parametrize("width,names", [(320, nc.PRODUCERS_320), (640, nc.PRODUCERS_640)])
def test_every_producer_accepts_the_statistics_request(dry, width, names):
    from live2diff_amd import ops
    x = nc.planted(nc.B, nc.T, width, nc.G, seed=1)
    for name in names:
        op, keep, out = nc.build_producer(ops, name, x, "cpu")
        acc = torch.zeros(2, nc.B, nc.G, 2, dtype=torch.int64)
        for j, kw in enumerate(nc.consumers_of(width)):
            assert ops.gn_target(op, acc[j].data_ptr(), T=nc.T, G=nc.G, **kw), f"{name} declines GroupNorm statistics for {kw}"
        ops.run((op, keep + (acc,)))                   # the library validates the launch with both consumers attached


@pytest.mark.parametrize("C1,C2,nt,p1,p2", [(320, 320, 256, "pconv", "rowgemm"), (1280, 640, 64, "igemm64", "rowgemm")])
def test_concat_producers_accept_the_statistics_request(dry, C1, C2, nt, p1, p2):
    from live2diff_amd import ops
    x = nc.planted(nc.B, nt, C1 + C2, nc.G, seed=1)
    acc = torch.zeros(nc.B, nc.G, 2, dtype=torch.int64)
    for part, name, choff in ((x[..., :C1].contiguous(), p1, 0), (x[..., C1:].contiguous(), p2, C1)):
        op, keep, out = nc.build_producer(ops, name, part, "cpu")
        assert ops.gn_target(op, acc.data_ptr(), T=nt, G=nc.G, cpg=(C1 + C2) // nc.G, choff=choff), (name, choff)
        ops.run((op, keep + (acc,)))


@pytest.mark.parametrize("width,names", [(320, nc.CONSUMERS_320), (640, nc.CONSUMERS_640)])
def test_every_fused_consumer_validates(dry, width, names):
    from live2diff_amd import ops
    x = nc.planted(nc.B, nc.T, width, nc.G, seed=1)
    gm, bt = nc.affine(width)
    for name in names:
        op, keep, out, silu = nc.build_consumer(ops, name, x, nc.exact_acc(x, nc.G), gm, bt, 1e-5, "cpu")
        ops.run((op, keep))
    assert ops.gn_self_ok(nc.T, width, nc.G)


def test_identity_weight_packings():
    from live2diff_amd import ops
    for C in (320, 640, 1280):
        gm, bt = nc.affine(C)
        wp, bp = ops.pack_rowgemm(torch.eye(C, dtype=torch.float16), torch.zeros(C), gm, bt)
        assert torch.equal(ops.unpack_rowgemm(wp, C, C), torch.diag(gm)) and torch.equal(bp, bt.float())
        wp, bp, cs = ops.pack_wsgemm(torch.eye(C, dtype=torch.float16), None, gm, bt)
        assert torch.equal(ops.unpack_rowgemm(wp, C, C), torch.diag(gm)) and torch.equal(bp, bt.float()) and torch.equal(cs, gm.float())
    for C in (320, 640):
        w = nc.identity_conv(C)
        want = w.permute(0, 2, 3, 1).reshape(C, 9, C)
        assert float(want[:, 4].sub(torch.eye(C)).abs().max()) == 0 and float(want.abs().sum()) == C      # centre tap only
        for KG in (4, 2):
            assert torch.equal(ops.unpack_cconv(ops.pack_cconv(w, KG), C, C, KG), want)
        assert torch.equal(ops.pack_conv3x3(w).view(C, 9, C), want)
