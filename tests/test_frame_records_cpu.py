"""CPU tests (-m "not gpu") of the frame-side record builders of live2diff_amd/ops.py, from `frame_ingest` to the end of the file:
every builder's record, field by field, and every rejection, type and message, against tests/golden/frame_records.json.

A table holds, per builder, the base call over small CPU tensors (H x W = 16 x 32: W % 8 == 0, one 16 x 32 depth / mask tile, a
2 x 4 follow field, one block of `frame_moments`, `color_lock` and `matte_key_gain_hist`; 32 x 64 where an op has an output
size), one accepting case per branch that changes the record and one rejecting case per check.  An accepted call is reduced to
plain data -- `kind`, the 16 pointer slots as null or [operand, byte offset from its data_ptr], the `i` and `l` fields, the bit
patterns of the `f` fields and the operands' names in `keep` -- and its record also runs through the library's launcher check
(dry-run).  A rejected call is reduced to [exception type, message].  Nothing here has a tolerance.

`python tests/test_frame_records_cpu.py` rewrites the fixture from the builders as they are."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_records.json")
H, W, Ho, Wo = 16, 32, 32, 64
Hs, Ws = 24, 48                     # a source that is not the frame's size (frame, depth and mask ingest)
W36 = 36                            # a width that is no multiple of 8


@pytest.fixture
def dry_run():
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    yield
    _lib.set_dry_run(False)


def z(dtype, *shape):
    return torch.zeros(*shape, dtype=dtype)


f16, f32, f64 = (functools.partial(z, d) for d in (torch.float16, torch.float32, torch.float64))
u8, i8, i16, u16, i32, u32 = (functools.partial(z, d) for d in (torch.uint8, torch.int8, torch.int16, torch.uint16, torch.int32, torch.uint32))


def off16(t):
    """`t`'s values at an address that is no multiple of 16: a view one element into a longer buffer"""
    return torch.zeros(t.numel() + 1, dtype=t.dtype)[1:].view(t.shape)


def strided(t):
    """`t`'s shape over memory that is not contiguous"""
    return torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype)[..., ::2]


def within(t, dtype, n):
    """`n` elements of `dtype` at the start of `t`'s memory"""
    return t.view(-1).view(dtype)[:n]


# ----------------------------------------------------------------------------- the cases
# name -> (base arguments, {accepting case: changes}, {rejecting case: changes}).  A change that is a function is called with the
# arguments as changed so far (an operand that aliases another); an argument whose name begins with "_" only holds memory.
@functools.lru_cache(maxsize=None)
def table():
    from live2diff_amd import jpeg as J
    from live2diff_amd import matte as MT
    from live2diff_amd import ops
    E = MT.edge_E(2, 4.0)
    ramp = dict(lo32=-0.4, inv32=1.25)
    rs = J.row_capacity(W)
    hdr = len(J.header(H, W))
    stride = -(-(16 + hdr + (H // 16) * rs) // 4) * 4
    t = {}

    t["frame_ingest"] = (
        dict(src=u8(1, Hs, Ws, 3), dst=f16(1, 3, H, W), B=1, Hs=Hs, Ws=Ws, H=H, W=W, nh=H, nw=W, top=0, left=0),
        {"crop": dict(nh=20, nw=40, top=2, left=4)},
        {"src_dtype": dict(src=f16(1, Hs, Ws, 3)), "dst_dtype": dict(dst=u8(1, 3, H, W))})
    t["frame_egress"] = (
        dict(src=f16(1, 3, H, W), dst=u8(1, H, W, 3), B=1, H=H, W=W), {},
        {"src_dtype": dict(src=f32(1, 3, H, W)), "dst_dtype": dict(dst=f16(1, H, W, 3))})

    t["jpeg_dct"] = (
        dict(src=f16(1, 3, H, W), coef=i16(H * W * 3 // 2), B=1, H=H, W=W, quality=75),
        {"u8": dict(src=u8(1, H, W, 3))},
        {"src_dtype": dict(src=f32(1, 3, H, W)), "coef_dtype": dict(coef=i32(H * W * 3 // 2)), "src_small": dict(src=f16(1, 3, H, W - 1)),
         "coef_small": dict(coef=i16(H * W * 3 // 2 - 1))})
    t["jpeg_huff"] = (
        dict(coef=i16(H * W * 3 // 2), tables=i32(544), staging=u8(rs), lengths=i32(1), B=1, H=H, W=W, row_stride=rs), {},
        {"coef_dtype": dict(coef=i32(H * W * 3 // 2)), "lengths_dtype": dict(lengths=i16(1)), "tables_small": dict(tables=i32(543)),
         "staging_small": dict(staging=u8(rs - 1)), "lengths_small": dict(B=2, staging=u8(2 * rs))})
    t["jpeg_pack"] = (
        dict(staging=u8(rs), lengths=i32(1), header=u8(hdr), out=u8(1, stride), B=1, H=H, row_stride=rs, out_stride=stride), {},
        {"header_dtype": dict(header=i8(hdr)), "lengths_dtype": dict(lengths=i16(1)), "out_small": dict(out=u8(1, stride - 1))})
    n_mcu, ny, C = 2, 4, 2          # 16 x 32 at 4:2:0: two MCUs of 4 + 2 blocks, one chunk each
    t["jpeg_entropy_dec"] = (
        dict(file=u8(4096), offsets=i32(16), dc_pred=i16(64), blob=u8(4032), params=i32(4), coef=i16(n_mcu * (ny + 2) * 64 + 8), status=i32(4),
             n_mcu=n_mcu, ny=ny, restart_interval=0, chunk_mcus=1, C=C, dc_tab=(0, 1, 1), ac_tab=(0, 1, 1)),
        {"restart": dict(restart_interval=1, chunk_mcus=2)},
        {"file_dtype": dict(file=i8(4096)), "status_dtype": dict(status=i16(4)), "dc_pred_dtype": dict(dc_pred=i32(64)),
         "offsets_small": dict(offsets=i32(C)), "blob_small": dict(blob=u8(3647)), "coef_small": dict(coef=i16(n_mcu * (ny + 2) * 64 - 1))})
    t["jpeg_idct"] = (
        dict(coef=i16(n_mcu * 6 * 64), quant=u8(384), planes=u8(n_mcu * 6 * 64), n_mcu=n_mcu, mcus_x=2, hs=2, vs=2),
        {"quant_u16": dict(quant=u16(192))},
        {"coef_dtype": dict(coef=i32(n_mcu * 6 * 64)), "quant_small": dict(quant=u8(383)), "planes_small": dict(planes=u8(n_mcu * 6 * 64 - 1))})
    t["jpeg_rgb"] = (
        dict(planes=u8(n_mcu * 6 * 64), out=u8(H, W, 3), H=H, W=W, hs=2, vs=2), {},
        {"out_dtype": dict(out=i8(H, W, 3)), "out_small": dict(out=u8(H, W, 3)[1:]), "planes_small": dict(planes=u8(n_mcu * 6 * 64 - 1))})

    d, s0, s1 = f16(64), f16(64), f16(64)
    host = np.zeros(2, ops.WBLEND_REC)
    host["dst"], host["n"] = (d.data_ptr(), d.data_ptr() + 64), 32
    host["src"][:, 0], host["src"][:, 1] = (s0.data_ptr(), s0.data_ptr() + 64), (s1.data_ptr(), s1.data_ptr() + 64)
    t["weight_blend"] = (
        dict(table_dev=torch.from_numpy(host.view(np.uint8).reshape(-1).copy()), table_host=host, weights=[0.25, 0.75], _dst=d, _src0=s0, _src1=s1),
        {"nt0": dict(nt=0), "nt1": dict(nt=1), "one_source": dict(weights=(1.0,))},
        {"host_dtype": dict(table_host=host.view(np.uint8)), "host_strided": dict(table_host=np.zeros(4, ops.WBLEND_REC)[::2]),
         "dev_dtype": dict(table_dev=i8(host.nbytes)), "dev_size": dict(table_dev=u8(host.nbytes + 1))})

    matte_flags = {"hard": dict(hard=True, inv32=0.0), "far": dict(far=True), "show": dict(show=True), "r": dict(r=2)}
    t["frame_matte"] = (
        dict(styled=f16(1, 3, H, W), source=f16(1, 3, H, W), depth=f16(1, H, W), dst=u8(1, H, W, 3), B=1, H=H, W=W, **ramp),
        {**matte_flags, "no_ramp": dict(lo32=0.0, inv32=0.0, hard=True), "depth_stride": dict(depth=f16(1, 3, H, W), depth_stride=3 * H * W),
         "plane": dict(depth=None, plane=f32(1, H, W)), "plane_show_r": dict(depth=None, plane=f32(1, H, W), show=True, r=1)},
        {"styled_dtype": dict(styled=f32(1, 3, H, W)), "dst_dtype": dict(dst=f16(1, H, W, 3)), "source_small": dict(source=f16(1, 3, H, W - 1)),
         "dst_small": dict(dst=u8(1, H, W - 1, 3)), "plane_and_depth": dict(plane=f32(1, H, W)), "plane_and_hard": dict(depth=None, plane=f32(1, H, W), hard=True),
         "plane_and_far": dict(depth=None, plane=f32(1, H, W), far=True), "plane_dtype": dict(depth=None, plane=f16(1, H, W)),
         "plane_strided": dict(depth=None, plane=strided(f32(1, H, W))), "plane_small": dict(depth=None, plane=f32(1, H, W - 1)),
         "depth_dtype": dict(depth=f32(1, H, W)), "depth_small": dict(depth=f16(1, H, W), depth_stride=3 * H * W, B=2,
                                                                     styled=f16(2, 3, H, W), source=f16(2, 3, H, W), dst=u8(2, H, W, 3))})

    def frame_rejects(name, make=f16, other=f32):
        """the rejections of a [3,H,W] operand `name`: its type, its shape, its size and its layout"""
        return {f"{name}_dtype": {name: other(3, H, W)}, f"{name}_shape": {name: make(H, 3, W)}, f"{name}_small": {name: make(3, H, W - 1)},
                f"{name}_strided": {name: strided(make(3, H, W))}}

    def plane_rejects(name, make=f32, other=f16, none=False):
        """the rejections of an [H,W] operand `name`"""
        r = {f"{name}_dtype": {name: other(H, W)}, f"{name}_small": {name: make(H, W - 1)}, f"{name}_strided": {name: strided(make(H, W))}}
        if none:
            r[f"{name}_none"] = {name: None}
        return r

    def int_rejects(name, lo, hi):
        """the rejections of an integer `name` from lo to hi"""
        return {f"{name}_low": {name: lo - 1}, f"{name}_high": {name: hi + 1}, f"{name}_bool": {name: True}, f"{name}_fraction": {name: lo + 0.5}}

    def matte_input_rejects(hard="hard"):
        """the rejections of the `plane=` / `depth=` pair of the ops that take either"""
        pl = dict(depth=None, plane=f32(H, W))
        return {"plane_and_depth": dict(plane=f32(H, W)), "plane_and_hard": {**pl, hard: True}, "plane_and_far": dict(pl, far=True),
                **{k: dict(depth=None, **v) for k, v in plane_rejects("plane").items()}, "plane_shape": dict(depth=None, plane=f32(W, H)),
                **plane_rejects("depth", f16, f32, none=True)}

    t["frame_matte_edge"] = (
        dict(source=f16(3, H, W), depth=f16(H, W), out=f32(H, W), H=H, W=W, r=2, E=E, **ramp),
        {"hard": dict(hard=True, inv32=0.0), "far": dict(far=True), "r_max": dict(r=8, E=MT.edge_E(8, 1.0)), "r_float": dict(r=2.0),
         "plane": dict(depth=None, plane=f32(H, W))},
        {**frame_rejects("source"), **matte_input_rejects(), **plane_rejects("out"), **int_rejects("r", 1, ops.MATTE_EDGE_MAX_R)})
    t["frame_backdrop_blur"] = (
        dict(source=f16(3, H, W), depth=f16(H, W), out=f16(3, H, W), H=H, W=W, r=2, passes=2, **ramp),
        {"hard": dict(hard=True, inv32=0.0), "far": dict(far=True), "passes": dict(passes=3, r=8), "plane": dict(depth=None, plane=f32(H, W))},
        {**frame_rejects("source"), **frame_rejects("out"), **matte_input_rejects(), **int_rejects("r", 1, ops.BACKDROP_MAX_R),
         **int_rejects("passes", 1, ops.BACKDROP_MAX_PASSES)})

    t["frame_moments"] = (
        dict(frame=f16(3, H, W), second=None, partials=i32(1, 1, 6), H=H, W=W),
        {"second": dict(second=f16(3, H, W), partials=i32(2, 1, 6))},
        {**frame_rejects("frame"), **{k: dict(v, partials=i32(2, 1, 6)) for k, v in frame_rejects("second").items()},
         "partials_dtype": dict(partials=f32(1, 1, 6)), "partials_small": dict(partials=i32(5)),
         "partials_small_second": dict(second=f16(3, H, W), partials=i32(11))})
    t["color_lock"] = (
        dict(styled=f16(3, H, W), out=f16(3, H, W), partials=i32(2, 1, 6), state_in=f64(3, 2), state_out=f64(3, 2), coef=f32(3, 3), H=H, W=W,
             strength=0.75, rate=0.125),
        {"init": dict(init=True), "source": dict(source=True), "freeze": dict(freeze=True), "one_partial": dict(partials=i32(1, 1, 6))},
        {**frame_rejects("styled"), **frame_rejects("out"), "partials_dtype": dict(partials=f32(2, 1, 6)), "partials_small": dict(partials=i32(5)),
         "partials_small_source": dict(partials=i32(11), source=True),
         "state_in_dtype": dict(state_in=f32(3, 2)), "state_in_size": dict(state_in=f64(3, 3)), "state_in_strided": dict(state_in=strided(f64(3, 2))),
         "state_out_dtype": dict(state_out=f32(3, 2)), "state_out_size": dict(state_out=f64(2, 2)),
         "coef_dtype": dict(coef=f64(3, 3)), "coef_size": dict(coef=f32(3, 2)), "coef_strided": dict(coef=strided(f32(3, 3)))})

    ks = 4
    wide = u8(Hs, Ws, 3)
    window = wide.view(-1)[(2 * Ws + 8) * 3:]                     # the H x W window of the Hs x Ws frame at (2, 8)

    def table_rejects(name, n_out, good):
        return {f"{name}_dtype": {name: f32(*good)}, f"{name}_strided": {name: strided(i32(*good))}, f"{name}_size": {name: i32(good[0], good[1] + 1)}}

    t["frame_resize"] = (
        dict(src=f16(1, 3, H, W), dst=u8(1, Ho, Wo, 3), tx=i32(Wo * (2 + ks)), ty=i32(Ho * (2 + ks + 1)), B=1, H=H, W=W, Ho=Ho, Wo=Wo),
        {"u8": dict(src=u8(1, H, W, 3)), "pitch_0": dict(src=u8(1, H, W, 3), src_pitch=0),
         "pitch": dict(src=window, src_pitch=Ws, _frame=wide)},
        {"src_dtype": dict(src=f32(1, 3, H, W)), "dst_dtype": dict(dst=f16(1, Ho, Wo, 3)), "pitch_past_end": dict(src=window, src_pitch=Ws + 24, _frame=wide),
         "src_small": dict(src=f16(1, 3, H, W - 1)), "dst_small": dict(dst=u8(1, Ho, Wo - 1, 3)),
         "tx_dtype": dict(tx=f32(Wo * 6)), "tx_strided": dict(tx=strided(i32(Wo * 6))), "tx_ragged": dict(tx=i32(Wo * 6 + 1)), "tx_short": dict(tx=i32(Wo * 2)),
         "ty_dtype": dict(ty=f32(Ho * 7)), "ty_ragged": dict(ty=i32(Ho * 7 + 1)), "ty_short": dict(ty=i32(Ho * 2))})
    t["frame_matte_up"] = (
        dict(styled=u8(1, Ho, Wo, 3), camera=u8(1, Ho, Wo, 3), depth=f16(1, H, W), dst=u8(1, Ho, Wo, 3), tx=i32(3, Wo), ty=i32(3, Ho), B=1, H=H, W=W,
             Ho=Ho, Wo=Wo, **ramp),
        {**matte_flags, "depth_stride": dict(depth=f16(1, 3, H, W), depth_stride=3 * H * W), "plane": dict(depth=None, plane=f32(1, H, W)),
         "plane_show_r": dict(depth=None, plane=f32(1, H, W), show=True, r=1)},
        {"styled_dtype": dict(styled=f16(1, Ho, Wo, 3)), "dst_dtype": dict(dst=i8(1, Ho, Wo, 3)), "camera_small": dict(camera=u8(1, Ho, Wo - 1, 3)),
         "dst_small": dict(dst=u8(1, Ho - 1, Wo, 3)), "plane_and_depth": dict(plane=f32(1, H, W)),
         "plane_and_hard": dict(depth=None, plane=f32(1, H, W), hard=True), "plane_and_far": dict(depth=None, plane=f32(1, H, W), far=True),
         "plane_dtype": dict(depth=None, plane=f16(1, H, W)), "plane_strided": dict(depth=None, plane=strided(f32(1, H, W))),
         "plane_small": dict(depth=None, plane=f32(1, H, W - 1)), "depth_dtype": dict(depth=f32(1, H, W)), "depth_small": dict(depth=f16(1, H, W - 1)),
         **table_rejects("tx", Wo, (3, Wo)), **table_rejects("ty", Ho, (3, Ho))})

    steady = dict(styled=f16(3, H, W), source=f16(3, H, W), prev_out=f16(3, H, W), prev_bytes=u8(3, H, W), out=f16(3, H, W), next_bytes=u8(3, H, W),
                  H=H, W=W, lo32=2.0, inv32=0.125, s32=0.875)
    steady_flags = {"r": dict(r=3), "r_max": dict(r=ops.STEADY_MAX_R), "hard": dict(hard=True, inv32=0.0), "show": dict(show=True, picture=f16(3, H, W))}
    steady_rejects = {**frame_rejects("styled"), **frame_rejects("source"), **frame_rejects("out"), **frame_rejects("prev_out"),
                      **frame_rejects("prev_bytes", u8, i8), **frame_rejects("next_bytes", u8, i8), "show_without_picture": dict(show=True),
                      "picture_without_show": dict(picture=f16(3, H, W)),
                      **{k: dict(v, show=True) for k, v in frame_rejects("picture").items()}, **int_rejects("r", 0, ops.STEADY_MAX_R)}
    t["frame_steady"] = (
        steady,
        {**steady_flags, "init": dict(init=True), "init_none": dict(init=True, prev_out=None, prev_bytes=None),
         "init_show": dict(init=True, prev_out=None, prev_bytes=None, show=True, picture=f16(3, H, W))},
        {**steady_rejects, "init_prev_out_dtype": dict(init=True, prev_out=f32(3, H, W)), "init_prev_bytes_dtype": dict(init=True, prev_bytes=i8(3, H, W))})

    def field_rejects():
        return {"field_dtype": dict(field=u8(H // 8, W // 8, 2)), "field_shape": dict(field=i8(H // 8, W // 8 + 1, 2)),
                "field_strided": dict(field=strided(i8(H // 8, W // 8, 2)))}

    t["frame_motion"] = (
        dict(source=f16(3, H, W), prev_bytes=u8(3, H, W), field=i8(H // 8, W // 8, 2), H=H, W=W, search=4, bias=16),
        {"limits": dict(search=ops.FOLLOW_MAX_SEARCH, bias=ops.FOLLOW_MAX_BIAS), "bias_0": dict(search=1, bias=0)},
        {**frame_rejects("source"), **frame_rejects("prev_bytes", u8, i8), **field_rejects(), **int_rejects("search", 1, ops.FOLLOW_MAX_SEARCH),
         **int_rejects("bias", 0, ops.FOLLOW_MAX_BIAS)})
    t["frame_steady_follow"] = (
        dict(steady, field=i8(H // 8, W // 8, 2)), steady_flags, {**steady_rejects, **field_rejects()})

    t["frame_matte_hold"] = (
        dict(source=f16(3, H, W), depth=f16(H, W), prev_plane=f32(H, W), prev_bytes=u8(3, H, W), out_plane=f32(H, W), next_bytes=u8(3, H, W), H=H, W=W,
             lo32=2.0, inv32=0.125, s32=0.875, ramp_lo32=-0.4, ramp_inv32=1.25),
        {"r": dict(r=3), "hard": dict(hard=True, inv32=0.0), "init": dict(init=True), "init_none": dict(init=True, prev_plane=None, prev_bytes=None),
         "plane": dict(depth=None, plane=f32(H, W)), "ramp_hard": dict(ramp_hard=True, ramp_inv32=0.0), "far": dict(far=True),
         "field": dict(field=i8(H // 8, W // 8, 2)), "plane_field": dict(depth=None, plane=f32(H, W), field=i8(H // 8, W // 8, 2))},
        {**frame_rejects("source"), **matte_input_rejects("ramp_hard"), **plane_rejects("prev_plane"), **frame_rejects("prev_bytes", u8, i8),
         "init_prev_plane_dtype": dict(init=True, prev_plane=f16(H, W)), "init_prev_bytes_dtype": dict(init=True, prev_bytes=i8(3, H, W)),
         **plane_rejects("out_plane"), "out_plane_shape": dict(out_plane=f32(W, H)), **frame_rejects("next_bytes", u8, i8), **field_rejects(),
         **int_rejects("r", 0, ops.STEADY_MAX_R)})

    t["frame_detail_gain"] = (
        dict(frame=f16(3, H, W), source=f16(3, H, W), out=i32(3, H, W), H=H, W=W, r=2, E=E),
        {"u8": dict(frame=u8(H, W, 3)), "r_max": dict(r=8, E=MT.edge_E(8, 1.0))},
        {**frame_rejects("frame"), "frame_u8_shape": dict(frame=u8(3, H, W)), "frame_u8_small": dict(frame=u8(H, W - 1, 3)),
         "frame_u8_strided": dict(frame=strided(u8(H, W, 3))), **frame_rejects("source"), **frame_rejects("out", i32, f32),
         **int_rejects("r", 1, ops.MATTE_EDGE_MAX_R)})

    def out_frame_rejects(name):
        return {f"{name}_dtype": {name: i8(Ho, Wo, 3)}, f"{name}_shape": {name: u8(3, Ho, Wo)}, f"{name}_small": {name: u8(Ho, Wo - 1, 3)},
                f"{name}_strided": {name: strided(u8(Ho, Wo, 3))}}

    t["frame_detail"] = (
        dict(styled=u8(Ho, Wo, 3), camera=u8(Ho, Wo, 3), low=u8(Ho, Wo, 3), gains=i32(3, H, W), tx=i32(3, Wo), ty=i32(3, Ho), dst=u8(Ho, Wo, 3),
             H=H, W=W, Ho=Ho, Wo=Wo, k=0.0003, limit=24.0),
        {"show": dict(show=True), "zero": dict(k=0.0, limit=0.0)},
        {**out_frame_rejects("styled"), **out_frame_rejects("camera"), **out_frame_rejects("low"), **out_frame_rejects("dst"),
         **frame_rejects("gains", i32, f32), **table_rejects("tx", Wo, (3, Wo)), **table_rejects("ty", Ho, (3, Ho)),
         "dst_is_styled": dict(dst=lambda a: a["styled"]), "dst_is_camera": dict(dst=lambda a: a["camera"]), "dst_is_low": dict(dst=lambda a: a["low"]),
         "k_negative": dict(k=-1.0), "k_nan": dict(k=float("nan")), "limit_negative": dict(limit=-1.0), "limit_inf": dict(limit=float("inf"))})

    taps = 3

    def resample_rejects():
        return {"xmin_dtype": dict(xmin=f32(W)), "xmin_size": dict(xmin=i32(W + 1)), "xmin_strided": dict(xmin=strided(i32(W))),
                "wx_dtype": dict(wx=f16(W, taps)), "wx_ndim": dict(wx=f32(W * taps)), "wx_rows": dict(wx=f32(W + 1, taps)), "wx_strided": dict(wx=strided(f32(W, taps))),
                "ymin_dtype": dict(ymin=f32(H)), "ymin_size": dict(ymin=i32(H + 1)), "wy_dtype": dict(wy=f16(H, taps)), "wy_rows": dict(wy=f32(H - 1, taps))}

    t["depth_ingest"] = (
        dict(src=u16(1, Hs, Ws), R=f32(1, H, W), partials=f32(1, 3), xmin=i32(W), wx=f32(W, taps), ymin=i32(H), wy=f32(H, taps + 1), B=1, Hd=Hs, Wd=Ws,
             H=H, W=W, nh=H, nw=W, top=0, left=0, distance=False, invalid=None),
        {"i16": dict(src=i16(1, Hs, Ws)), "f32": dict(src=f32(1, Hs, Ws)), "distance": dict(distance=True), "invalid_u16": dict(invalid=65535),
         "invalid_u16_float": dict(invalid=7.0), "invalid_u16_never": dict(invalid=65536), "invalid_u16_fraction": dict(invalid=0.5),
         "invalid_f32": dict(src=f32(1, Hs, Ws), invalid=0.1), "invalid_f32_distance": dict(src=f32(1, Hs, Ws), invalid=0.0, distance=True),
         "crop": dict(nh=20, nw=40, top=2, left=4)},
        {"src_dtype": dict(src=u8(1, Hs, Ws)), "src_size": dict(src=u16(1, Hs, Ws - 1)), "src_strided": dict(src=strided(u16(1, Hs, Ws))),
         "R_dtype": dict(R=f16(1, H, W)), "R_size": dict(R=f32(1, H, W + 1)), "R_strided": dict(R=strided(f32(1, H, W))),
         "partials_dtype": dict(partials=f64(1, 3)), "partials_size": dict(partials=f32(2, 3)), "partials_strided": dict(partials=strided(f32(1, 3))),
         **resample_rejects()})
    t["depth_normalize"] = (
        dict(R=f32(1, H, W), partials=f32(1, 3), out=f16(1, 3, H, W), B=1, H=H, W=W),
        {"fixed": dict(fixed=(0.25, 0.75)), "fixed_np": dict(fixed=np.array([0.1, 0.9], np.float32))},
        {"R_dtype": dict(R=f16(1, H, W)), "R_size": dict(R=f32(1, H, W + 1)), "R_strided": dict(R=strided(f32(1, H, W))),
         "out_dtype": dict(out=f32(1, 3, H, W)), "out_size": dict(out=f16(1, H, W)), "out_strided": dict(out=strided(f16(1, 3, H, W))),
         "partials_dtype": dict(partials=f64(1, 3)), "partials_size": dict(partials=f32(2, 3)), "partials_strided": dict(partials=strided(f32(1, 3)))})

    combined = dict(combine="and", **ramp)
    t["mask_ingest"] = (
        dict(src=u8(Hs, Ws), out=f32(H, W), depth=f16(H, W), xmin=i32(W), wx=f32(W, taps), ymin=i32(H), wy=f32(H, taps + 1), Hm=Hs, Wm=Ws, H=H, W=W,
             nh=H, nw=W, top=0, left=0),
        {"u16": dict(src=u16(Hs, Ws)), "i16": dict(src=i16(Hs, Ws)), "f32": dict(src=f32(Hs, Ws)), "invert": dict(invert=True),
         "replace_drops": dict(hard=True, far=True, **ramp), "replace_none": dict(depth=None), "and": combined, "or": dict(combined, combine="or"),
         "and_hard": dict(combined, hard=True, inv32=0.0), "or_far_invert": dict(combined, combine="or", far=True, invert=True),
         "crop": dict(nh=20, nw=40, top=2, left=4)},
        {"src_dtype": dict(src=i32(Hs, Ws)), "src_size": dict(src=u8(Hs, Ws - 1)), "src_strided": dict(src=strided(u8(Hs, Ws))), **plane_rejects("out"),
         "combine": dict(combine="xor"), **{k: dict(combined, **v) for k, v in plane_rejects("depth", f16, f32, none=True).items()}, **resample_rejects()})

    key = dict(source=f16(3, H, W), out=f32(H, W), depth=f16(H, W), key=(0, 255, 64), H=H, W=W, r=1, L=128, lo2=100.0, inv=0.0125, hard=False)
    plate = dict(key=u8(3, H, W))
    and_ramp = dict(combine="and", **ramp)
    key_accepts = {"hard": dict(hard=True, inv=0.0), "invert": dict(invert=True), "replace_drops": dict(ramp_hard=True, far=True, **ramp),
                   "replace_none": dict(depth=None), "and": and_ramp, "or": dict(and_ramp, combine="or"),
                   "and_ramp_hard": dict(and_ramp, ramp_hard=True, inv32=0.0), "or_far": dict(and_ramp, combine="or", far=True),
                   "r_0": dict(r=0, L=0), "r_max": dict(r=ops.MATTE_KEY_MAX_R, L=256), "r_np": dict(r=np.int64(2), L=np.int32(77))}
    key_rejects = {**frame_rejects("source"), **plane_rejects("out"),
                   "W_odd": dict(W=W36, source=f16(3, H, W36), out=f32(H, W36)), "combine": dict(combine="xor"),
                   **{k: dict(and_ramp, **v) for k, v in plane_rejects("depth", f16, f32, none=True).items()},
                   "r_low": dict(r=-1), "r_high": dict(r=ops.MATTE_KEY_MAX_R + 1), "r_bool": dict(r=True), "r_float": dict(r=1.0),
                   "L_low": dict(L=-1), "L_high": dict(L=257), "L_bool": dict(L=False), "L_float": dict(L=128.0),
                   "lo2_negative": dict(lo2=-1.0), "lo2_nan": dict(lo2=float("nan")), "inv_negative": dict(inv=-0.5), "inv_inf": dict(inv=float("inf")),
                   "hard_with_inv": dict(hard=True), "inv_0_not_hard": dict(inv=0.0)}
    gain = dict(gain=i32(8))
    t["matte_key"] = (
        key,
        {**key_accepts, "colour_list": dict(key=[1, 2, 3]), "colour_np": dict(key=np.array([255, 0, 255], np.uint8)), "plate": plate,
         "plate_or_invert": dict(and_ramp, combine="or", invert=True, **plate), "plate_gain": dict(plate, **gain),
         "plate_gain_and": dict(and_ramp, **plate, **gain)},
        {**key_rejects, "plate_dtype": dict(key=i8(3, H, W)), "plate_shape": dict(key=u8(1, 3, H, W)), "plate_strided": dict(key=strided(u8(3, H, W))),
         "colour_two": dict(key=(1, 2)), "colour_high": dict(key=(0, 0, 256)), "colour_low": dict(key=(-1, 0, 0)), "colour_bool": dict(key=(True, 0, 0)),
         "colour_fraction": dict(key=(0.5, 0, 0)), "colour_text": dict(key="red"), "colour_none": dict(key=None), "colour_names": dict(key=("r", "g", "b")),
         "gain_with_colour": gain, "gain_dtype": dict(plate, gain=f32(8)), "gain_size": dict(plate, gain=i32(9)), "gain_strided": dict(plate, gain=strided(i32(8))),
         "gain_unaligned": dict(plate, gain=off16(i32(8))), "gain_list": dict(plate, gain=[128] * 8),
         "gain_in_plane": dict(plate, gain=lambda a: within(a["out"], torch.int32, 8))})

    adapt = dict(key, plate=u8(3, H, W), state_in=None, state_out=u16(3, H, W), a_bg=1024, a_fg=16)
    del adapt["key"]
    running = dict(plate=None, state_in=u16(3, H, W))
    t["matte_key_adapt"] = (
        adapt,
        {**key_accepts, "running": running, "running_plate": dict(state_in=u16(3, H, W)), "running_i16": dict(plate=None, state_in=i16(3, H, W), state_out=i16(3, H, W)),
         "rates": dict(a_bg=0, a_fg=ops.MATTE_KEY_MAX_RATE), "rates_np": dict(a_bg=np.int32(5), a_fg=np.int64(6)), "gain": gain,
         "running_gain_or": dict(and_ramp, combine="or", **running, **gain)},
        {"init_plate_none": dict(plate=None), "init_plate_colour": dict(plate=(0, 255, 0)), "running_plate_colour": dict(state_in=u16(3, H, W), plate=(0, 255, 0)),
         **key_rejects, "plate_dtype": dict(plate=i8(3, H, W)), "plate_shape": dict(plate=u8(1, 3, H, W)),
         **int_rejects("a_bg", 0, ops.MATTE_KEY_MAX_RATE), **int_rejects("a_fg", 0, ops.MATTE_KEY_MAX_RATE), "a_bg_float": dict(a_bg=1024.0),
         "state_in_dtype": dict(state_in=u8(3, H, W)), "state_in_shape": dict(state_in=u16(1, 3, H, W)), "state_in_unaligned": dict(state_in=off16(u16(3, H, W))),
         "state_out_none": dict(state_out=None), "state_out_dtype": dict(state_out=i32(3, H, W)), "state_out_strided": dict(state_out=strided(u16(3, H, W))),
         "state_out_unaligned": dict(state_out=off16(u16(3, H, W))),
         "state_out_is_state_in": dict(running, state_out=lambda a: a["state_in"]), "state_out_in_source": dict(state_out=lambda a: a["source"].view(torch.uint16)),
         "state_out_in_plate": dict(plate=u8(6, H, W)[:3], state_out=lambda a: a["plate"]._base.view(-1).view(torch.uint16).view(3, H, W)),
         "state_out_in_depth": dict(and_ramp, depth=f16(3 * H, W)[:H], state_out=lambda a: a["depth"]._base.view(torch.uint16).view(3, H, W)),
         "state_in_in_plane": dict(plate=None, out=f32(2 * H, W)[:H], state_in=lambda a: a["out"]._base.view(-1).view(torch.uint16)[:3 * H * W].view(3, H, W)),
         "gain_dtype": dict(gain=f32(8)), "gain_unaligned": dict(gain=off16(i32(8))), "gain_in_plane": dict(gain=lambda a: within(a["out"], torch.int32, 8)),
         "gain_in_state_out": dict(gain=lambda a: within(a["state_out"], torch.int32, 8))})

    t["matte_key_gain_hist"] = (
        dict(source=f16(3, H, W), plate=u8(3, H, W), partials=u32(1, 3, ops.MATTE_KEY_GAIN_BINS), H=H, W=W),
        {"state": dict(plate=u16(3, H, W)), "state_i16": dict(plate=i16(3, H, W)), "partials_i32": dict(partials=i32(1, 3, ops.MATTE_KEY_GAIN_BINS))},
        {"W_odd": dict(W=W36, source=f16(3, H, W36), plate=u8(3, H, W36)), "H_0": dict(H=0), **frame_rejects("source"), "source_unaligned": dict(source=off16(f16(3, H, W))),
         "source_list": dict(source=[0.0]), **frame_rejects("plate", u8, i8), "plate_none": dict(plate=None),
         "plate_u8_unaligned": dict(plate=torch.zeros(3 * H * W + 4, dtype=torch.uint8)[4:].view(3, H, W)), "plate_state_unaligned": dict(plate=off16(u16(3, H, W))),
         "partials_dtype": dict(partials=f32(1, 3, ops.MATTE_KEY_GAIN_BINS)), "partials_blocks": dict(partials=u32(2, 3, ops.MATTE_KEY_GAIN_BINS)),
         "partials_strided": dict(partials=strided(u32(1, 3, ops.MATTE_KEY_GAIN_BINS))), "partials_unaligned": dict(partials=off16(u32(1, 3, ops.MATTE_KEY_GAIN_BINS))),
         "partials_none": dict(partials=None),
         "partials_in_source": dict(source=f16(6, H, W)[:3], partials=lambda a: a["source"]._base.view(-1).view(torch.int32)[:3 * 512].view(1, 3, 512)),
         "partials_in_plate": dict(plate=u16(6, H, W)[:3], partials=lambda a: a["plate"]._base.view(-1).view(torch.int32)[:3 * 512].view(1, 3, 512))})
    t["matte_key_gain"] = (
        dict(partials=u32(1, 3, ops.MATTE_KEY_GAIN_BINS), record=i32(8), H=H, W=W, lim=256, min_count=64),
        {"limits": dict(lim=ops.MATTE_KEY_GAIN_BINS - 1, min_count=H * W), "limits_low": dict(lim=ops.MATTE_KEY_GAIN_UNITY, min_count=0),
         "np": dict(lim=np.int64(300), min_count=np.int32(5)), "partials_i32": dict(partials=i32(1, 3, ops.MATTE_KEY_GAIN_BINS))},
        {"W_odd": dict(W=W36), "H_0": dict(H=0), "partials_dtype": dict(partials=f32(1, 3, ops.MATTE_KEY_GAIN_BINS)),
         "partials_blocks": dict(partials=u32(2, 3, ops.MATTE_KEY_GAIN_BINS)), "record_dtype": dict(record=f32(8)), "record_size": dict(record=i32(4)),
         "record_strided": dict(record=strided(i32(8))), "record_unaligned": dict(record=off16(i32(8))), "record_list": dict(record=[0] * 8),
         **int_rejects("lim", ops.MATTE_KEY_GAIN_UNITY, ops.MATTE_KEY_GAIN_BINS - 1), **int_rejects("min_count", 0, H * W), "lim_float": dict(lim=256.0),
         "record_in_partials": dict(record=lambda a: within(a["partials"], torch.int32, 8))})
    t["frame_planar_bytes"] = (
        dict(source=f16(3, H, W), out=u8(3, H, W), H=H, W=W), {},
        {**frame_rejects("source"), **frame_rejects("out", u8, i8), "out_batch": dict(out=u8(1, 3, H, W)),
         "W_odd": dict(W=W36, source=f16(3, H, W36), out=u8(3, H, W36))})
    return t


def arguments(name, case):
    """the arguments of one case, with its changes applied in order"""
    base, accepts, rejects = table()[name]
    a = dict(base)
    for k, v in ({} if case == "base" else accepts.get(case, rejects.get(case))).items():
        a[k] = v(a) if callable(v) else v
    return a


def call(name, a):
    from live2diff_amd import ops
    return getattr(ops, name)(**{k: v for k, v in a.items() if not k.startswith("_")})


def span(v):
    """(address, bytes) of an operand's memory, or None"""
    if torch.is_tensor(v):
        return v.data_ptr(), v.numel() * v.element_size()
    if isinstance(v, np.ndarray):
        return v.ctypes.data, v.nbytes
    return None


def reduce_record(op, keep, a):
    """the record and its keep tuple as plain data"""
    spans = [(k, *span(v)) for k, v in a.items() if span(v) is not None]

    def where(ptr):
        if ptr is None:
            return None
        for k, base, n in spans:
            if base <= ptr < base + max(n, 1):
                return [k, ptr - base]
        raise AssertionError(f"pointer {ptr:#x} lies in no operand")

    def who(t):
        if t is None:
            return None
        return next(k for k, v in a.items() if v is t)

    return {"kind": int(op.kind), "p": [where(op.p[j]) for j in range(16)], "i": [int(v) for v in op.i], "l": [int(v) for v in op.l],
            "f": np.array(list(op.f), np.float32).view(np.int32).tolist(), "keep": [who(t) for t in keep]}


def accepted(name, case):
    from live2diff_amd import _lib
    a = arguments(name, case)
    op, keep = call(name, a)
    got = reduce_record(op, keep, a)
    pl = _lib.OpList()                                     # the launcher's own check of the record
    pl.append(op, *keep)
    pl.run()
    return got


def rejected(name, case):
    a = arguments(name, case)
    try:
        call(name, a)
    except Exception as e:                                 # (whatever it is: the type is part of what is pinned)
        return [type(e).__name__, str(e)]
    raise AssertionError(f"{name}[{case}] was not rejected")


# `jpeg_index` (host work, no record) has the section's three other checks
@functools.lru_cache(maxsize=None)
def jpeg_file():
    from live2diff_amd import jpeg as J
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_dec_pillow.npz"))
    data = g[sorted(k for k in g if k.startswith("f_"))[0]].tobytes()
    return J.parse(data), data


def jpeg_index_rejected(case):
    from live2diff_amd import jpeg as J
    from live2diff_amd import ops
    info, data = jpeg_file()
    C = J.chunk_layout(info.n_mcu, info.restart_interval, 3)[3]
    kw = {"offsets_dtype": dict(offsets=np.empty(C + 1, np.int64)), "offsets_size": dict(offsets=np.empty(C, np.int32)),
          "dc_pred_dtype": dict(dc_pred=np.empty((C, 3), np.int32)), "dc_pred_strided": dict(dc_pred=np.empty((C, 6), np.int16)[:, ::2]),
          "blob_size": dict(blob=np.zeros(J.DEC_BLOB_BYTES - 1, np.uint8)), "blob_dtype": dict(blob=np.zeros(J.DEC_BLOB_BYTES, np.int8)),
          "damaged": dict()}[case]
    try:
        ops.jpeg_index(info, data[:(info.scan_offset + info.scan_end) // 2] if case == "damaged" else data, 3, **kw)
    except Exception as e:
        return [type(e).__name__, str(e)]
    raise AssertionError(f"jpeg_index[{case}] was not rejected")


JPEG_INDEX_CASES = ("offsets_dtype", "offsets_size", "dc_pred_dtype", "dc_pred_strided", "blob_size", "blob_dtype", "damaged")


def current():
    """everything the fixture holds, from the builders as they are"""
    out = {}
    for name, (base, accepts, rejects) in table().items():
        out[name] = {"accept": {c: accepted(name, c) for c in ("base", *accepts)}, "reject": {c: rejected(name, c) for c in rejects}}
    out["jpeg_index"] = {"accept": {}, "reject": {c: jpeg_index_rejected(c) for c in JPEG_INDEX_CASES}}
    return out


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


BUILDERS = ("frame_ingest", "frame_egress", "jpeg_dct", "jpeg_huff", "jpeg_pack", "jpeg_entropy_dec", "jpeg_idct", "jpeg_rgb", "weight_blend",
            "frame_matte", "frame_matte_edge", "frame_backdrop_blur", "frame_moments", "color_lock", "frame_resize", "frame_matte_up", "frame_steady",
            "frame_motion", "frame_steady_follow", "frame_matte_hold", "frame_detail_gain", "frame_detail", "depth_ingest", "depth_normalize",
            "mask_ingest", "matte_key", "matte_key_adapt", "matte_key_gain_hist", "matte_key_gain", "frame_planar_bytes")


def test_the_table_names_every_builder_of_the_section():
    import inspect
    from live2diff_amd import ops
    src = inspect.getsource(ops)
    section = src[src.index("frame I/O (frame_io.hip)"):]
    names = [ln[4:ln.index("(")] for ln in section.splitlines() if ln.startswith("def ") and not ln.startswith("def _")]
    helpers = {"jpeg_index", "color_lock_blocks", "depth_tiles", "matte_key_gain_blocks"}          # (no record comes out of these)
    assert [n for n in names if n not in helpers] == list(BUILDERS) == list(table())
    assert sorted(golden()) == sorted((*BUILDERS, "jpeg_index"))


@pytest.mark.parametrize("name", BUILDERS)
def test_records(dry_run, name):
    base, accepts, rejects = table()[name]
    want = golden()[name]
    assert list(want["accept"]) == ["base", *accepts] and list(want["reject"]) == list(rejects)
    for case in want["accept"]:
        assert accepted(name, case) == want["accept"][case], f"{name}[{case}]"
    for case in want["reject"]:
        assert rejected(name, case) == want["reject"][case], f"{name}[{case}]"


def test_jpeg_index_rejections():
    want = golden()["jpeg_index"]["reject"]
    assert list(want) == list(JPEG_INDEX_CASES)
    for case in JPEG_INDEX_CASES:
        assert jpeg_index_rejected(case) == want[case], case


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from live2diff_amd import _lib
    _lib.set_dry_run(True)
    with open(GOLDEN, "w") as f:                          # one case per line
        f.write("{\n" + ",\n".join(
            f"{json.dumps(name)}: {{\n" + ",\n".join(
                f" {json.dumps(part)}: {{\n" + ",\n".join(f"  {json.dumps(c)}: {json.dumps(v, separators=(',', ':'))}" for c, v in cases.items()) + "\n }"
                for part, cases in parts.items()) + "\n}" for name, parts in current().items()) + "\n}\n")
    n = {k: sum(len(v[k]) for v in golden().values()) for k in ("accept", "reject")}
    print(f"{GOLDEN}: {n['accept']} accepted records, {n['reject']} rejections, {os.path.getsize(GOLDEN)} bytes")
