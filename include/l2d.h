/*
 * l2d.h -- C ABI of libl2d_hip.so: the MI355X (gfx950) backend for Live2Diff's streaming UNet step.
 *
 * Drop-in boundary being replaced (reference, Python):
 *   - `stream.unet(sample, timestep, encoder_hidden_states=..., temporal_attention_mask=...,
 *      depth_sample=..., kv_cache=..., pe_idx=..., update_idx=...)`
 *        live2diff/pipeline_stream_animation_depth.py:456-466 (per frame), :355-365 (engine warm-up)
 *   - the accelerator object swapped in at live2diff/utils/wrapper.py:613-626, whose contract is
 *        live2diff/acceleration/tensorrt/engine.py:142-185 (UNet2DConditionModelDepthEngine.__call__)
 *        and whose runtime is live2diff/acceleration/tensorrt/utilities.py:247-294 (Engine.infer).
 * The reference has no FFI of its own (it is 100 % Python driving PyTorch / TensorRT); this header is
 * what a ctypes binding on the reference side binds instead of `Engine.infer`.
 *
 * Conventions
 *   - plain C: pointers are DEVICE pointers (HBM) unless stated; sizes are ints; no torch types.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream). Nothing here synchronises.
 *   - every function returns 0 on success, a negative L2D_E* code otherwise; l2d_last_error() gives text.
 *   - activations are channels-last fp16: a tensor "[B,T,C]" is B*T rows of C contiguous halfs.
 *   - KV caches use the reference interchange layout [N,2,T,L,C] fp16
 *        (live2diff/animatediff/models/stream_motion_module.py:57-77).
 *
 * A UNet step is a static *plan*: an array of l2d_op records (one per kernel launch) that the host
 * builds once per (H,W,N,L) and that l2d_run_ops()/l2d_graph_* replay every frame.
 */
#ifndef L2D_H
#define L2D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L2D_ABI_VERSION 6

enum {
    L2D_OK = 0,
    L2D_EINVAL = -1,   /* bad argument / unsupported shape */
    L2D_ELAUNCH = -2,  /* HIP launch or runtime error */
    L2D_ENODEV = -3,   /* no gfx950 device */
};

/* op kinds ---------------------------------------------------------------------------------------
 * Field meaning per kind (p = pointers, i = ints, f = floats); unused fields must be 0.
 *
 * L2D_OP_IGEMM   implicit GEMM on MFMA: linear / 1x1 conv / 3x3 conv (stride 1|2, optional nearest-2x
 *                upsample folded into the gather, optional channel-concat of two inputs), fused epilogue.
 *                out[m][n] = epi( sum_k X[m][k] * W[n][k] )        (reference: nn.Linear / InflatedConv3d,
 *                resnet.py:57-65,112,141; attention.py:62,89; motion_module.py:182,207)
 *   p0 x1 [B,Hin,Win,C1] half   p1 x2 [.., C2] half or 0        p2 w packed [Nout][taps*CinP] half
 *   p3 bias[Nout] float or 0    p4 rowbias [*, ldrb] float or 0 p5 residual [M][ldr] half or 0
 *   p6 out [M][ldo] half
 *   i0 taps(1|9) i1 C1 i2 C2 i3 ldx1 i4 ldx2 i5 CinP i6 B i7 Hin i8 Win i9 Hout i10 Wout i11 stride
 *   i12 ups(0|1) i13 M i14 Nout i15 ldo i16 ldr i17 ldrb i18 rows_per_bias i19 epi (0 none, 1 GEGLU, 2 SiLU)
 *   i20 batch (grid.z) ; l0..l3 = per-batch element strides of x1, w, out, residual
 *   p7 16-byte zero page (padding source)   p8 split-K workspace [batch][S][M][round_up(Nout,4)] float
 *   i21 splitk (S, 1 = off: S > 1 adds the igemm_splitk_epilogue launch unless p11 is set)
 *   p11 (split-K only) int32 arrival counters, one per (batch, tile), ZERO before the launch and left zero by it: the
 *   reduction is fused -- the block that arrives last at a tile's counter sums the S partial tiles in the fixed order
 *   0..S-1 and runs the epilogue; p8 is then [batch][tile][S][tile_n * tile_m] float (whole tiles) and i22's tile must be
 *   explicit (1 or 2).  Results are bit-identical between runs (the order of the sum does not depend on the arrival order).
 *   i22 tile (0 auto, 1 = 128x128,
 *   2 = 64x64; + 16 = weight-tile-major block order: each XCD's L2 holds a band of output channels, for
 *   GroupNorm statistics of the OUTPUT, accumulated by the producer (replaces the consumer's L2D_OP_GN_STATS launch):
 *   p9 / p10 accumulators int64 [samples][G][2] of up to two consumer GroupNorms, or 0 ; i24 T (tokens per sample)
 *   i25 G ; i26 / i27 channels per group and channel offset of this tensor inside consumer 1's (concatenated) channel axis
 *   i28 / i29 the same for consumer 2.  Sums are deterministic fixed-point atomics: sum x in units of 2^-20, sum x^2 in
 *   units of 2^-12 (cannot overflow int64 for fp16 data at these sizes); the accumulators must be zero before the launch.
 *   Needs the LDS-staged epilogue (Nout % 8 == 0 ...) or split-K, and tiles that do not straddle samples (T % 128 == 0,
 *   or T % 64 == 0 with the 64x64 tile / split-K).
 *   i22 also: + 32 = direct register -> global epilogue (8-byte pieces) instead of the default one that
 *   transposes the tile through LDS and stores whole rows with 16 bytes per lane) i23 pipeline variant (igemm.hip launch_p)
 *
 * L2D_OP_GN_STATS / L2D_OP_GN_APPLY   GroupNorm over channels-last [B,T,C1(+C2)] (two-input = concat),
 *                optional SiLU (reference: InflatedGroupNorm resnet.py:68-76, F.silu :233,249)
 *   p0 x1 p1 x2|0 p2 partial[B][nchunk][G][2] float  (apply: p3 gamma half, p4 beta half, p5 out half)
 *   i0 B i1 T i2 C1 i3 C2 i4 ld1 i5 ld2 i6 G i7 nchunk i8 silu  f0 eps
 *   GN_APPLY with nchunk = 0: p6 = int64 [B][G][2] fixed-point accumulators filled by the producing igemm launches (above)
 *   GN_APPLY with nchunk = 0 and p6 = 0 (p2 unused): the one-launch form for small tensors -- a block holds all T rows of a band of whole
 *   groups (lcm(C / G, 8) <= 128 channels, <= 4 groups) in registers, statistics and apply in the same launch; refused (L2D_EINVAL) when
 *   T * band / 8 exceeds 16 vectors per thread of 256
 *
 * L2D_OP_LAYERNORM  p0 x [rows][ld] p1 gamma p2 beta p3 out [rows][C] ; i0 rows i1 C i2 ldx i3 ldo; f0 eps
 *
 * L2D_OP_FLASH_ATTN  softmax(QK^T/sqrt(d))V on MFMA (spatial self / text cross attention;
 *                reference call sites attention.py:243,250-255)
 *   p0 q [B][Tq][ldq] p1 k [B][Tk][ldk] p2 vt [B][H*d][ldvt] (V transposed) p3 out [B][Tq][ldo]
 *   i0 B i1 H i2 d i3 Tq i4 Tk i5 ldq i6 ldk i7 ldvt i8 ldo ; l0 q batch stride l1 k l2 vt l3 out
 *   p4 16-byte zero page (DMA source of keys beyond Tk; 0 selects the register-staged kernel)
 *   i9 variant: 0 auto (LDS-DMA ring kernel, flash_attn_ring.hip), 1 register-staged kernel (flash_attn.hip: the fallback for
 *   K / V^T operands that are not 16-byte aligned), 2 / 3 ring kernel with 32 / 16 query rows per wave, 4 ring kernel with 32
 *   rows per wave and the software-pipelined key-tile loop (d <= 48; bit-identical to 2; what auto picks where 2 was picked
 *   before; larger d run 2).  V^T columns in [Tk, ldvt) may hold anything.
 *
 * L2D_OP_TATTN_STREAM  fused streaming temporal attention with multi-timestep KV-cache
 *                (reference stream_motion_module.py:99-213)
 *   p0 qkv [N*T][3C] half p1 cache [N,2,T,L,C] half (in-place) p2 q_pe p3 k_pe p4 v_pe [maxlen][C] half
 *   p5 pe_idx [N][L] int64 p6 update_idx [N] int64 p7 bias [N][L] half p8 out [N*T][C] half
 *   p9 16-byte zero page (DMA source of masked slots; required by the ring kernel, may be 0 otherwise)
 *   i0 N i1 T i2 C i3 L i4 H i5 variant (0 auto: the loader-wave LDS-DMA ring kernel (tattn_ring.hip) for C in {320,640,1280},
 *   L in {12,16,24,40}, T % 8 == 0, else register-resident (L <= 16) / chunked; 1 register-resident, 2/3 chunked CH=8/4,
 *   13 = the ring kernel, refused when the shape does not fit it)
 *
 * L2D_OP_TATTN_WARMUP  bidirectional warm-up temporal attention + cache fill
 *                (reference motion_module.py:469-530)
 *   p0 qkv [F*T][3C] p1 cache_row [2,T,L,C] p2 q_pe p3 k_pe p4 v_pe p8 out [F*T][C]
 *   i0 F i1 T i2 C i3 L i4 H
 *
 * L2D_OP_SKINNY_LINEAR  out[m][n] = act( sum_k A[m][k] W[n][k] + b[n] ), m < 8 (time embedding path,
 *                reference unet_depth_streaming.py:499-505, resnet.py:238)
 *   p0 A half [M][K] p1 W half [Nout][K] p2 bias float p3 out (half or float) ; i0 M i1 K i2 Nout
 *   i3 silu_out i4 out_is_float i5 ldo
 * L2D_OP_TIMESTEP_EMBED  p0 timesteps (int64 [N]) p1 out half [N][dim]; i0 N i1 dim
 * L2D_OP_NCHW_TO_NHWC  p0 in half [B][C][HW] p1 out half [B][HW][Cpad]; i0 B i1 C i2 HW i3 Cpad
 * L2D_OP_NHWC_TO_NCHW  p0 in half [B][HW][ld] p1 out half [B][C][HW]; i0 B i1 C i2 HW i3 ld
 *   both: i4 element map, fp16 rounding after each step: 0 copy, 1 (x + f1) * f0, 2 tanh(x / 3) * 3, 3 x * f0 + f1
 *   (the input / output scalings of diffusers' EncoderTiny / DecoderTiny, reference swap point wrapper.py:468-470)
 * L2D_OP_LCM_STEP   x0 = c_out*(x - beta*eps)/alpha + c_skip*x  (reference pipeline :387-401)
 *   p0 x p1 eps p2 scal float [N][4]={alpha,beta,c_skip,c_out} p3 x0 ; i0 N i1 per_sample_elems
 * L2D_OP_COPY       p0 src p1 dst ; l0 bytes   (device-to-device, on the stream)
 *
 * Per-frame pipeline glue on the device (stream_glue.hip):
 * L2D_OP_RING_UPDATE  update_attn_bias (reference pipeline_stream_animation_depth.py:416-438), in place:
 *   p0 bias [N][L] half (0 / -inf) p1 pe_idx [N][L] int64 p2 update_idx [N] int64 p3 frame counter uint64* or 0
 *   (incremented by one); i0 N i1 L i2 sink (= warm-up frames)
 * L2D_OP_STREAM_SHIFT scheduler_step_batch + stream-batch shift register (reference :387-401, :590-601):
 *   p0 x_t [N][per] half (in: the batch the UNet just saw; out: rows 1..N-1 = next frame's buffer)
 *   p1 eps [N][per] half (UNet output) p2 scal [N][4] float {alpha, beta, c_skip, c_out} p3 noise [N-1][per] half or 0
 *   p4 x0_out [per] half (x0 prediction of the last row) p5 depth [N][per] half or 0 (row i+1 <- row i)
 *   i0 N (<= 8) i1 per (elements per row)
 * L2D_OP_RANDN      p0 out [n] half, standard normal (Philox4x32-10 + Box-Muller) p1 frame counter uint64* or 0
 *   l0 n l1 seed l2 offset (in Philox blocks of 4); element i = normal i%4 of block offset + frame*ceil(n/4) + i/4
 *
 * Depth-path glue (glue.hip; reference pipeline_stream_animation_depth.py:553,560-567):
 * L2D_OP_RESIZE_BILINEAR  F.interpolate(mode="bilinear", align_corners=False) on fp16 planes:
 *   p0 in [planes][Hin][Win] half p1 out [planes][Hout][Wout] half ; i0 planes i1 Hin i2 Win i3 Hout i4 Wout
 * L2D_OP_MINMAX  min and max of a fp16 tensor, left on the device: p0 x half (16-byte aligned) p1 scratch float [2*nb]
 *   p2 out float[2] = {min, max} ; l0 n ; i0 nb (blocks of the partial pass, <= 1024)
 * L2D_OP_DEPTH_NORM_RESIZE  ((d - min) / (max - min)) -> 3 channels -> * 2 - 1 -> bilinear resize, fp16 rounding after each
 *   reference tensor op:  p0 depth [B][Hd][Wd] half p1 {min, max} float[2] p2 out [B][3][H][W] half ; i0 B i1 Hd i2 Wd i3 H i4 W
 *
 * Depth detector (DPT-Hybrid; reference depth_utils.py:11-32): its GEMM-shaped work runs on L2D_OP_IGEMM
 * (i30 = 1: TF-"SAME" low-side padding 0 for stride-2 3x3 convs; epi 5 = GELU) / L2D_OP_FLASH_ATTN (d = 64) /
 * L2D_OP_GN_APPLY (i8 activation: 0 none, 1 SiLU, 2 ReLU, 3 ReLU(norm(x) + p7 residual)) / L2D_OP_LAYERNORM /
 * L2D_OP_SKINNY_LINEAR (l0 = row stride of A, 0 = dense); the rest:
 * L2D_OP_STEM7X7   weight-standardised 7x7 stride-2 SAME conv, 3 -> 64: p0 image [B,3,H,W] half (NCHW) p1 w [64][3][7][7] half
 *   p2 out [B,ceil(H/2),ceil(W/2),64] half ; i0 B i1 H i2 W
 * L2D_OP_RESAMPLE_NHWC  channels-last p0 in [B,H,W,C] -> p1 out ; i0 B i1 H i2 W i3 C (% 8) i4 mode: 0 = 3x3 stride-2 max pool
 *   (SAME), 1 = stride-2 subsample, 2 = bilinear x2 upsample with align_corners=True
 * L2D_OP_EW        s = p0 (+ p1); p2 = s (if given); p3 = relu(s) (if given) ; l0 n halfs (% 8)
 *
 * L2D_OP_ROWGEMM   token-row GEMM for the transformer linear layers, with the normalisation in front of them fused:
 *                out[m][n] = epi( sum_k T(x)[m][k] * W[n][k] ),  K % 64 == 0, K <= 2048  (rowgemm.hip; reference: nn.LayerNorm /
 *                GroupNorm + nn.Linear, attention.py:57-62,89,102-110,173-205; motion_module.py:181-182,207,273-279,355-361)
 *   p0 x [M][ldx] half   p1 w half, packed in MFMA-fragment order [Nout/32][K/16][64 lanes][8] (ops.pack_rowgemm; GEGLU: rows
 *   permuted so that a 32-row tile holds 8 value / 8 gate / 8 value / 8 gate rows of 16 output channels)
 *   p2 bias float [Nout] (packed order) or 0   p3 residual [M][ldr] half or 0   p4 out [M][ldo] half
 *   (the affine part of the prologue norm is folded into p1 / p2 at pack time: the kernel takes no gamma / beta; p5, p6 unused)
 *   p7 prologue 2: int64 [samples][G][2] fixed-point statistics of x
 *   p8 outT half: output of the LAST i15 weight tiles, stored transposed [sample][channel][ldt] (V^T for the flash kernel)
 *   p9 / p10, i24..i29: GroupNorm statistics of the output for up to two consumers, exactly as L2D_OP_IGEMM
 *   i0 M i1 K i2 Nout (packed rows, % 32) i3 ldx i4 ldo i5 ldr i6 epi (0 none, 1 GEGLU: Nout / 2 output columns)
 *   i7 prologue (0 none, 1 LayerNorm over K, 2 GroupNorm normalisation from p7)   (i8 unused)
 *   i9 T tokens per sample (prologue 2, transposed output, output statistics: T % (32 MT) == 0) i10 G groups of prologue 2
 *   i12 NW waves per block (1..8; 1..5 when NT >= 3) i13 NT weight tiles per wave (1..4) i14 MT token tiles per block
 *   (1 | 2 | 4; MT >= 2 needs NT <= 2, MT = 4 needs K = 320): a block computes 32 MT tokens x 32 NW NT packed rows;
 *   (Nout / 32) % (NW NT) == 0 (ops.rowgemm_schedule)
 *   i15 trailing weight tiles stored transposed to p8 (% (NW NT)) i16 ldt i17 block order (1 = weight-band major per XCD)
 *   l0 elements between samples in p8 ; f0 eps of the prologue norm
 *
 * L2D_OP_PCONV     3x3 stride-1 pad-1 convolution with the haloed activation patch resident in LDS (pconv.hip; reference
 *                InflatedConv3d resnet.py:57-65 as used by ResnetBlock3D :194,214): same result as L2D_OP_IGEMM with taps = 9,
 *                stride 1, no upsample, epi 0; the activations are fetched once per 64-channel chunk instead of once per tap
 *   p0 x1 [B,H,W,C1] half   p1 x2 [B,H,W,C2] half or 0 (channel concat)   p2 w packed [Nout][9 * CinP] half (ops.pack_conv3x3)
 *   p3 bias float [Nout] or 0   p4 rowbias float [*][ldrb] or 0 (row = first token of the sample / i18)   p5 residual [M][ldr] half
 *   or 0   p6 out [M][ldo] half   p7 16-byte zero page   p9 / p10, i24..i29 GroupNorm statistics of the output as L2D_OP_IGEMM
 *   i1 C1 i2 C2 (both % 64) i3 ldx1 i4 ldx2 i5 CinP (= C1 + C2) i6 B i7 H i8 W i9 / i10 patch height / width (8x16, 8x8 or 4x8;
 *   H % PH == 0, W % PW == 0) i11 block order (1 = weight-tile major) i14 Nout (% 64) i15 ldo i16 ldr i17 ldrb i18 rows_per_bias
 *
 * L2D_OP_WSGEMM    weight-streaming GEMM for the levels with few tokens (M = N * T <~ 1k): linear layers and 3x3 stride-1 pad-1
 *                convs with 128-token row tiles; every weight byte is fetched by one wave per row tile, straight into registers
 *                (wsgemm.hip; reference: resnet.py:194,214 via InflatedConv3d :57-65; attention.py:173-205,258;
 *                motion_module.py:360; stream_motion_module.py:99-147).  out[m][n] = epi( sum_k LN?(x)[m][k] * W[n][k] )
 *   p0 x1 [M][ldx1] half (conv: [B,H,W,C1])   p1 x2 [M][ldx2] half or 0 (channel concat)   p2 w half, MFMA-fragment order
 *   [Nout/32][taps*CinP/16][64 lanes][8] with k = tap * CinP + channel (ops.pack_wsgemm / pack_wsgemm_conv3x3; GEGLU rows permuted
 *   as for L2D_OP_ROWGEMM)   p3 bias float [Nout] (packed order) or 0   p4 rowbias float [*][ldrb] or 0 (row = token / i18)
 *   p5 residual [M][ldr] half or 0   p6 out [M][ldo] half   p7 zero region, >= 2 * CinP + 256 zero bytes (padding / ragged rows)
 *   p8 outT half: output of the LAST i21 weight tiles, stored transposed [sample][channel][ldt] (V^T; T % 128 == 0)
 *   p9 / p10, i24..i29 GroupNorm statistics of the output as L2D_OP_IGEMM (a tile may span samples: T % 32 == 0)
 *   p11 split-K arrival counters (int32, one per (channel tile, row tile), zero before and after)   p12 split-K workspace float
 *   [tiles][S][128 * 32 NW NT + 256]   p13 colsum float [Nout]: sum_k fp16(W'[n][k]) for the LayerNorm fold (i20 = 1)
 *   i0 taps (1 | 9) i1 C1 i2 C2 (% 64) i3 ldx1 i4 ldx2 i5 CinP (= C1 + C2) i6 B i7 H i8 W (conv; W >= 8, M = B H W)
 *   i9 NW consumer waves (1..10; 9 / 10 since round 6: 3 / 3 / 2 / 2 consumers per SIMD, one block per CU) i10 NT weight tiles per wave (1 | 2; 2: NW <= 4) i11 NL loader waves (1 | 2) i12 S K slices
 *   (fused reduction: the last arriving block sums the S slabs in order 0..S-1 -- bit-repeatable -- and runs the epilogue)
 *   i13 M i14 Nout (packed rows, % 32; (Nout / 32) % (NW NT) == 0) i15 ldo i16 ldr i17 ldrb i18 rows_per_bias (% 32)
 *   i19 epi (0 none, 1 GEGLU: Nout / 2 output columns) i20 pro (0 none, 1 LayerNorm over K folded: gamma / beta live in p2 / p3,
 *   out = rstd (acc - mean colsum) + bias with the row statistics taken in the kernel) i21 trailing weight tiles stored transposed
 *   i22 ldt i23 non-temporal weight loads (single row tile) i30 T tokens per sample (p8)   l0 elements between samples in p8
 *   f0 eps of the LayerNorm
 *
 * L2D_OP_CCONV     3x3 stride-1 pad-1 convolution with the haloed activation patch resident in LDS AND the weights streamed straight into
 *                registers (cconv.hip, round 6; reference InflatedConv3d resnet.py:57-65 as used by ResnetBlock3D :194,214 and by
 *                Upsample3D :94-127): same result as L2D_OP_IGEMM with taps = 9, stride 1 (optionally the nearest-x2 up-sampling folded into
 *                the gather), epi 0.  A block owns an 8 x 16 patch of OUTPUT pixels x 64 CG channels x one K slice of whole 64-channel chunks.
 *   p0 x1 [B,Hs,Ws,C1] half   p1 x2 [B,Hs,Ws,C2] half or 0 (channel concat)   p2 w half: the weight streams of ops.pack_cconv(weight, KG)
 *   ([Nout/64][KG][chunk][tap][u < 4/KG][half 2][64 lanes][8], k step kk = u KG + kg; + 9 k steps (18 KB) of zero padding)
 *   p3 bias float [Nout] or 0   p4 rowbias float [*][ldrb] or 0 (row = first token of the sample / i18)   p5 residual [M][ldr] half or 0
 *   p6 out [M][ldo] half   p7 16-byte zero page   p9 / p10, i24..i29 GroupNorm statistics of the OUTPUT as L2D_OP_IGEMM
 *   p11 split-K counters (int32, TWO per (channel tile, patch): tickets and done; zero before and after)   p12 split-K workspace float
 *   [tiles][S][128 * 64 CG]   (S > 1: the block with the last ticket sums the S partial tiles in the fixed order 0..S-1 with its own
 *   registers at its own position -- bit-repeatable; it neither publishes nor re-reads its own tile)
 *   p13 / p14 / p15, i20 = 1, i21 G, f0 eps: the conv of silu(GroupNorm(x1 | x2)) -- statistics int64 [B][G][2] as L2D_OP_GN_APPLY with
 *   nchunk = 0, gamma / beta half [C1 + C2]; the normalisation runs in the loader waves (no GroupNorm launch, no normalised tensor)
 *   i1 C1 i2 C2 (both % 64) i3 ldx1 i4 ldx2 i5 CinP (= C1 + C2) i6 B i7 H i8 W (OUTPUT resolution: H % 8 == 0, W % 16 == 0; the input is
 *   [B, H >> i13, W >> i13, C]) i9 CG i10 KG ((2, 2) or (1, 4): CG KG = 4 compute waves) i11 NLD loader waves (1 | 2 | 4) i12 S K slices
 *   (<= CinP / 64) i13 ups (0 | 1: nearest x2 of Upsample3D) i14 Nout (% 64 CG) i15 ldo i16 ldr i17 ldrb i18 rows_per_bias
 *
 * L2D_OP_ROWCHAIN  token-resident tail of a transformer block, ONE launch (rowchain.hip; reference attention.py:243-270,125-133;
 *                motion_module.py:401-435,290-297):   h2 = to_out(a) + res1;  h3 = FF2(GEGLU(LayerNorm(h2))) + h2;
 *                out = proj_out(h3) + res2.   C = 320 (the level whose M / 32 blocks fill the chip), M % 32 == 0.
 *   p0 a [M][lda] half (attention output)   p1 res1 [M][ldr1] half (residual stream)   p2 res2 [M][ldr2] half (block input)
 *   p3 out [M][ldo] half   p4 / p5 to_out weights (L2D_OP_ROWGEMM fragment order, ops.pack_rowgemm) / fp32 bias
 *   p6 / p7 GEGLU projection (LayerNorm gamma / beta folded, value / gate rows interleaved as for L2D_OP_ROWGEMM epi 1) / bias
 *   p8 / p11 FF2 weights / bias   p12 / p13 proj_out weights / bias   p9 / p10, i24..i29 GroupNorm statistics of `out` as
 *   L2D_OP_IGEMM (T % 32 == 0)
 *   i0 M i1 C i2 lda i3 ldr1 i4 ldr2 i5 ldo i6 = 0   f0 eps of the LayerNorm
 *   i6 = 1: HEAD SEGMENT, two dependent layers in one launch (attention.py:102-110,221-250; motion_module.py:273-279,401-427):
 *                h = A(norm?(x)) + bA (+ resA) -> p2;   out = B(LayerNorm(h)) + bB, i7 passes of C packed rows each
 *   p0 x [M][i2] half   p1 resA [M][i3] half or 0   p2 h out [M][i4] half   p3 out [M][i5] half: the first (i7 - i8) passes, C columns each
 *   p4 / p5 layer A weights (fragment order; a GroupNorm's affine folded) / fp32 bias   p6 / p7 layer B weights (LayerNorm folded) /
 *   fp32 bias or 0   p8 outT half: with i8 = 1 the LAST pass is stored transposed [sample][channel][i9] (V^T), l0 elements between
 *   samples   p14 GroupNorm prologue on x: int64 [samples][G][2] fixed-point statistics filled by x's producers (as L2D_OP_ROWGEMM
 *   prologue 2), or 0   i7 passes (1 | 3) i8 transposed last pass (needs i7 = 3) i9 ldt i10 T tokens per sample i11 G
 *   f0 eps of the LayerNorm f1 eps of the GroupNorm
 *
 * CLIP text encoder (clip.hip; reference: transformers' CLIPTextModel as called by
 * pipeline_animatediff_depth.py:149-248).  The residual stream is fp32 [rows][C]; everything else is fp16.
 * L2D_OP_CLIP_EMBED  out[r][c] = float(tok[ids[r]][c]) + float(pos[r % T][c]):  p0 ids int64 [rows] p1 tok [V][C] half
 *   p2 pos [P][C] half p3 out [rows][C] float ; i0 rows (% T) i1 T (<= P) i2 C (% 8) i3 V i4 P
 * L2D_OP_CLIP_ATTN   causal (i6 = 1) or full softmax(Q K^T scale) V per (prompt, head), all T rows computed:  p0 qkv [B*T][ldq] half
 *   (q | k | v at columns 0, H d, 2 H d) p1 out [B*T][ldo] half ; i0 B i1 T (<= 128) i2 H i3 d (= 64) i4 ldq (% 8) i5 ldo i6 causal
 *   f0 scale
 * L2D_OP_CLIP_LINEAR out[m][n] = epi( sum_k pro(x)[m][k] W[n][k] + b[n] ) for small M (weight streaming, MFMA; K <= 1024 with i5 = 1):
 *   p0 x: [M][ldx] half (i5 = 0) or the fp32 residual stream [M][ldx] float (i5 = 1: LayerNorm over K with p4 / p5 applied)
 *   p1 w half in MFMA-fragment order [Nout/32][K/16][64 lanes][8] (ops.pack_clip_linear)  p2 bias float [Nout] or 0
 *   p3 out: half [M][ldo] (i6 = 0 none, 1 quick-GELU v sigmoid(1.702 v)) or float [M][ldo] (i6 = 2: out += v, in place)
 *   p4 gamma p5 beta float [K] (i5 = 1) ; i0 M i1 K i2 Nout (% 32) i3 ldx (% 8) i4 ldo i5 pro i6 epi i7 NW waves per block
 *   (1..8) i8 MT token tiles of 32 per block (1..4) ; K = NW * npass * 192 ; f0 eps
 * L2D_OP_CLIP_LN     LayerNorm, fp32 in, fp16 out: p0 x [rows][ldx] float p1 gamma p2 beta float [C] p3 out [rows][ldo] half ;
 *   i0 rows i1 C (<= 1024) i2 ldx i3 ldo ; f0 eps
 *
 * SD AutoencoderKL (vae_attn.hip; reference: diffusers' AutoencoderKL, the `stream.vae` of a pipeline without the tiny VAE).
 * L2D_OP_VAE_ATTN    single-head attention of d = 512, O = softmax(Q K^T f0) V per sample, masked tails, flash form with the keys
 *   split over S blocks per query tile (merged in split-index order: bit-repeatable):  p0 qkv [B*T][ld] half (q | k | v at
 *   columns 0, 512, 1024) p1 out [B*T][ldo] half p2 tile images half [B][ceil(T/32)][2][32*512] p3 (S > 1) fp32 workspace
 *   [S][B][64 ceil(T/64)][514] ; i0 B i1 T i2 ld (>= 1536, % 8) i3 ldo (>= 512, % 8) i4 S (1..16, <= ceil(T/32), no split empty) ;
 *   f0 scale
 * L2D_OP_VAE_POSTERIOR  z = mean + exp(0.5 clamp(logvar, -30, 20)) eps:  p0 moments [B][8][HW] half (mean = channels 0-3,
 *   logvar = 4-7) p1 eps [B][4][HW] half p2 z [B][4][HW] half ; i0 B i1 HW
 *
 * Frame I/O (frame_io.hip; reference: what the callers of wrapper.py do on the host, test.py:106-112 and image_utils.py:9-37).
 * L2D_OP_FRAME_INGEST  uint8 HWC frame -> the stream's fp16 NCHW input in [-1, 1], one launch: torchvision's Resize(min(H, W),
 *   antialias=True) + CenterCrop((H, W)) geometry, antialiased bilinear filter (F.interpolate(mode="bilinear", antialias=True):
 *   per axis scale = n_in / n_out, support = max(scale, 1), centre = scale (i + 0.5), taps [max(0, int(c - support + 0.5)),
 *   min(n_in, int(c + support + 0.5))), w_j = max(0, 1 - |(j - c + 0.5) / support|) normalised), fp32 accumulation,
 *   value = fp16(2 sum / 255 - 1):  p0 src uint8 [B][Hs][Ws][3] (RGB, dense) p1 dst half [B][3][H][W] (16-byte aligned) ;
 *   i0 B i1 Hs i2 Ws i3 H i4 W (% 8) i5 nh i6 nw (size of the resized image) i7 top i8 left (crop window inside it: refused
 *   otherwise).  Refused: Hs / nh or Ws / nw above 8 (17 taps), B Hs Ws 3 >= 2^31.  Hs == nh == H, Ws == nw == W is the identity.
 * L2D_OP_FRAME_EGRESS  the decoder's fp16 NCHW output -> uint8 HWC: u = rint(255 clamp(fp16(fp16(x / 2) + 0.5), 0, 1)), round half
 *   to even:  p0 src half [B][3][H][W] p1 dst uint8 [B][H][W][3] (both 16-byte aligned) ; i0 B i1 H i2 W (H W % 16 == 0)
 *
 * Baseline JPEG (jpeg.hip; reference: demo/util.py:27-37 encodes every output frame on the host).  8-bit YCbCr 4:2:0, MCU = 16 x 16
 *   pixels = Y00 Y01 Y10 Y11 Cb Cr, libjpeg's accurate integer DCT, Annex K tables scaled by libjpeg's quality rule, Annex K.3 Huffman
 *   tables, one restart interval per MCU row; integer arithmetic throughout -- the file equals live2diff_amd/jpeg.py `encode_ref`
 *   (and Pillow's `save(format="JPEG", quality=q, restart_marker_rows=1)`) byte for byte.  H and W are multiples of 16 and
 *   W <= 1920 in all three (refused otherwise); R = H / 16 MCU rows, M = W / 16 MCUs per row.
 * L2D_OP_JPEG_DCT  colour conversion, 2 x 2 chroma down-sampling, both DCT passes and quantisation, one launch:  p0 src, either
 *   half [B][3][H][W] in [-1, 1] (4-byte aligned; mapped to bytes with L2D_OP_FRAME_EGRESS' expression first) or uint8 [B][H][W][3]
 *   p1 coef int16 [B][R][M][6][64], every block in zigzag order (16-byte aligned) ; i0 B i1 H i2 W i3 source kind (0 half, 1 uint8)
 *   i4 quality (1..100: s = 5000 / q below 50, 200 - 2 q from 50; Q = clamp((base s + 50) / 100, 1, 255); divisor 8 Q)
 * L2D_OP_JPEG_HUFF  entropy coding, one work-group per (frame, MCU row): Huffman codes, the last byte filled with 1-bits, 0x00
 *   behind every 0xFF, then RSTn (EOI behind the last row):  p0 coef (as above) p1 tables uint32 [544]: dc [2][16] then ac [2][256],
 *   `length << 16 | code` per symbol (jpeg.Tables.packed) p2 staging uint8 [B][R][row_stride] p3 len int32 [B][R] (bytes of every
 *   row, marker included) ; i0 B i1 H i2 W i3 row_stride (>= M 6 432 + 4: 64 symbols of 27 bits per block, doubled by stuffing)
 * L2D_OP_JPEG_PACK  the file:  p0 staging p1 len p2 header uint8 [hdr_len] (jpeg.header) p3 out uint8 [B][out_stride] (4-byte
 *   aligned): per frame an int32 with the file's length, the file itself from byte 16 ; i0 B i1 H i2 row_stride i3 hdr_len ;
 *   l0 out_stride (% 4, >= 16 + hdr_len + R row_stride)
 *
 * Baseline JPEG decoder (jpeg_dec.hip; reference: demo/app.py:81-85 and demo/util.py:22 decode every input frame on the host).
 *   8-bit Y Cb Cr, SOF0, one interleaved scan, luminance sampling 1 x 1 / 2 x 1 / 2 x 2 (ny = 1 / 2 / 4 luminance blocks per MCU,
 *   then Cb, Cr), any Huffman tables, any size, with or without restart markers; integer arithmetic throughout -- the frame equals
 *   live2diff_amd/jpeg.py `decode_ref` (and Pillow's decode) byte for byte.  The scan is cut into CHUNKS of `chunk_mcus` consecutive
 *   MCUs, counted from the start of every restart interval (jpeg.chunk_layout: a chunk never spans a restart marker); the host
 *   finds where each begins (l2d_jpeg_index below), the device does the rest.
 * L2D_OP_JPEG_ENTROPY_DEC  one lane per chunk:  p0 file uint8 [capacity] p1 bit_offsets int32 [C + 1] p2 dc_pred int16 [C][3]
 *   (both as l2d_jpeg_index writes them) p3 table blob uint8 [4032] (jpeg.table_blob; 4-byte aligned) p4 params int32 [2] =
 *   {byte offset of the scan in the file, length of the file}, read by the kernel and clamped to the capacity p5 coef int16
 *   [n_mcu][ny + 2][64], DC absolute, natural order, every element written (16-byte aligned) p6 status int32, OR-ed into: 1 invalid
 *   code, 2 coefficient index past 63, 4 a chunk does not end where the next begins, 8 bad index; zero before the launch ;
 *   i0 n_mcu i1 ny i2 restart interval (0 none) i3 chunk_mcus i4 C (refused unless it follows from i0, i2, i3) i5 capacity of p0 in
 *   bytes (< 2^28) i6..i8 DC table id of Y, Cb, Cr i9..i11 AC table id (0 | 1)
 * L2D_OP_JPEG_IDCT  dequantisation and libjpeg's accurate integer IDCT (jidctint: 13 constant bits, 2 extra bits behind the column
 *   pass, clamp(x + 128, 0, 255); 32-bit arithmetic that wraps: equal to libjpeg for |dequantised coefficient| <= 1024, which every
 *   picture is far inside; beyond it -- only a damaged file -- the result is defined and repeatable but libjpeg's 64-bit one may differ):
 *   p0 coef (as above) p1 quantisation tables uint16 [3][64], natural order (the blob at byte 3648)
 *   p2 planes uint8 (8-byte aligned): Y [my vs 8][mx hs 8], Cb and Cr [my 8][mx 8] behind one another ; i0 n_mcu i1 mx (MCUs per
 *   row) i2 hs i3 vs
 * L2D_OP_JPEG_RGB  libjpeg's "fancy" chroma up-sampling (h2v1: (3 a + b + 1) >> 2 / (3 a + b + 2) >> 2; h2v2: 3 near + far, then
 *   (3 this + last + 8) >> 4 / (3 this + next + 7) >> 4; edges copied, the bottom edge from the last REAL row; replication for planes
 *   of one or two columns) and its 16-bit fixed-point colour conversion:  p0 planes (as above, mx = ceil(W / 8 hs), my = ceil(H / 8 vs))
 *   p1 out uint8 [H][W][3] ; i0 H i1 W i2 hs i3 vs
 *
 * Style switch / style blend (wblend.hip; the reference changes style by building a new wrapper and a new engine).
 * L2D_OP_WEIGHT_BLEND  dst_t = sum_k a_k src_{k,t} over every tensor t of a packed weight set, ONE launch however many tensors:
 *   p0 table of l2d_wblend_rec in DEVICE memory (16-byte aligned) p1 the same table in HOST memory (read by the launcher only, to
 *   validate) ; i0 number of records i1 K (1..4 sources) i2 cache policy (0 plain loads / stores, 1 non-temporal) ; f0..f3 the
 *   weights a_k (finite).  A record is one TILE of one tensor (below): the host cuts every tensor into tiles of at most
 *   L2D_WBLEND_TILE_BYTES, a work-group takes records blockIdx.x, blockIdx.x + gridDim.x, ...  Arithmetic, fixed so that numpy restates
 *   it bit for bit (style_bank.blend_ref): acc = a_0 s_0, then acc = acc + a_k s_k for k = 1, 2, ... in source order, every product
 *   and every sum rounded to fp32 on its own (no fma), one round-to-nearest-even to the tensor's dtype at the end; K = 1 with
 *   a_0 = 1 is a copy, and moves the bits as they are (1 x would quieten a signalling NaN in padding nobody initialised).  16-byte accesses over the whole vectors of a tile, one lane per element for the up to 7 elements behind
 *   them; nothing outside [dst, dst + n elements) is written.  Refused: a null or not 16-byte aligned dst / src[k < K], n <= 0 or
 *   more than a tile, an unknown dtype, K outside 1..4, a non-finite weight.  dst may be one of the sources (same offsets only).
 *
 * Depth matte (matte.hip; no counterpart in the reference, which drops its depth map behind the conditioning encode).
 * L2D_OP_FRAME_MATTE  the stream's output composited over its source frame by a matte of the frame's depth map, as the uint8 HWC
 *   frame L2D_OP_FRAME_EGRESS writes, one launch:  p0 styled half [B][3][H][W] p1 source half [B][3][H][W] p2 depth half, plane b at
 *   p2 + b l0 elements, [H][W], in [-1, 1] with 1 nearest p3 dst uint8 [B][H][W][3] (all four 16-byte aligned) ; i0 B i1 H i2 W
 *   (W % 8 == 0, H W % 16 == 0) i3 r (feather radius, 0..L2D_MATTE_MAX_R) i4 flags (L2D_MATTE_HARD | _FAR | _SHOW) ; l0 depth plane
 *   stride in elements (>= H W, % 8: 3 H W reads channel 0 of a [B][3][H][W] tensor in place) ; f0 lo (in [-1, 1]) f1 inv (1 / (hi -
 *   lo); 0 exactly when HARD is set).  Arithmetic, every step one fp32 operation with one rounding and no fma, so that numpy restates
 *   it bit for bit (live2diff_amd/matte.py composite_ref): t = clamp((d - lo) inv, 0, 1) (HARD: d >= lo ? 1 : 0);
 *   m = (t t) (3 - 2 t); FAR: m = 1 - m; r > 0: a (2r+1) x (2r+1) box filter as a horizontal then a vertical pass, coordinates
 *   clamped to the image, the taps added in increasing coordinate order, each pass divided (correctly rounded) by float(2r + 1);
 *   v = clamp(fp16(fp16(x / 2) + 0.5), 0, 1) on styled and source (L2D_OP_FRAME_EGRESS' chain); o = v_c + m (v_s - v_c);
 *   byte = rint(255 o), half to even.  SHOW writes rint(255 m) to all three channels and reads neither frame.  m == 1 gives
 *   L2D_OP_FRAME_EGRESS(styled) and m == 0 L2D_OP_FRAME_EGRESS(source) byte for byte.  Refused: B H W 3 >= 2^31, B > 65535.
 *   L2D_MATTE_PLANE (this op and L2D_OP_FRAME_MATTE_UP): p2 is a float plane [H][W] of ready matte values in [0, 1] (plane b at
 *   p2 + b l0 floats; L2D_OP_FRAME_MATTE_EDGE writes one), 16-byte aligned here and 4-byte aligned there.  The ramp, HARD and FAR
 *   are skipped -- f0, f1 and those two bits are not read --, the feather, the blend and SHOW work on the plane's values as on m.
 *   A compile-time variant of the kernels: with the flag clear nothing of the paths above changes.
 *
 * Colour lock (colorlock.hip; no counterpart in the reference).  The per-channel mean and variance of the BYTES a frame leaves as
 *   (b = L2D_OP_FRAME_EGRESS' byte of a pixel) are measured in exact integers and held to a target by one gain and one offset per
 *   channel; the result is an fp16 frame in the decoder's convention that every outlet consumes unchanged.  Both ops: i0 H i1 W
 *   (W % 8 == 0, H W % 16 == 0, H W <= L2D_COLOR_LOCK_MAX_PIXELS) i3 nblk = ceil(H W / L2D_COLOR_LOCK_BLOCK_PIXELS).
 * L2D_OP_FRAME_MOMENTS  p0 half [3][H][W] p1 a second such tensor, or null p2 partials uint32 [i2][nblk][6] (all 16-byte aligned)
 *   ; i2 number of tensors (1 | 2).  partials[t][k][0..2] = sum of b, partials[t][k][3..5] = sum of b^2 over pixels
 *   [k BLOCK_PIXELS, (k + 1) BLOCK_PIXELS) of channel 0, 1, 2 of tensor t.  Every entry is written by a plain store on every
 *   launch: nothing has to be zeroed, there are no atomics, and integer sums do not depend on any order.
 * L2D_OP_COLOR_LOCK  p0 styled half [3][H][W] p1 out half [3][H][W] (not overlapping p0) p2 partials as above, tensor 0 = p0's (and
 *   tensor 1 = the target frame's with L2D_COLOR_LOCK_SOURCE) p3 state_in double [3][2] = (mean, var) per channel p4 state_out
 *   likewise (not overlapping p3: block 0 writes it while other blocks read p3) p5 coefficient record float [3][3] = (g, s, t) per
 *   channel ; i2 flags ; l0, l1 the BITS of two doubles: the rate beta in (0, 1] and the strength a in [0, 1].  Arithmetic, every step
 *   one correctly rounded operation and no fma, so that numpy restates it bit for bit (live2diff_amd/color_lock.py): with S1, S2 the
 *   sums over the frame and n = H W, mean = double(S1) / double(n), var = double(n S2 - S1^2) / double(n n) (int64, exact); the new
 *   state is the moments of tensor 1 (SOURCE), state_in (FREEZE), else the styled frame's moments c (INIT) or t + beta (c - t) in
 *   three operations per value; per channel g = sqrt(var_t / var_s), 1 where either variance is 0, clamped to [1/4, 4], then
 *   g = 1 + a (g - 1); m = mean_s + a (mean_t - mean_s); g32 = float(g), s32 = float(2 mean_s / 255 - 1), t32 = float(2 m / 255 - 1);
 *   per pixel o = ((float(x) - s32) g32) + t32 in three fp32 operations, out = half(clamp(o, -1, 1)), round to nearest even.
 *   Inputs are finite.
 *
 * Output size (resize.hip; the reference's callers resize the PIL image they get on the host).  Pillow's `Image.resize` on 8-bit
 *   images, integer arithmetic throughout -- the frame equals live2diff_amd/resize.py `resize_ref` (and Pillow) byte for byte.
 * L2D_OP_FRAME_RESIZE  source patch to bytes, horizontal pass, vertical pass, one launch:  p0 src, either half [B][3][H][W] in
 *   [-1, 1] (4-byte aligned; mapped to bytes with L2D_OP_FRAME_EGRESS' expression first) or uint8 [B][H][W][3] p1 dst uint8
 *   [B][Ho][Wo][3] (any alignment) p2 table of the x axis p3 table of the y axis (int32, 4-byte aligned; for an axis of n_out
 *   outputs: xmin [n_out], count [n_out], k [n_out][KS] behind one another, as resize.coefficients builds them: output xx reads
 *   inputs xmin[xx] .. xmin[xx] + count[xx] - 1 with the weights k[xx][0 .. count[xx]), 22 fractional bits) ; i0 B i1 H i2 W
 *   i3 Ho i4 Wo i5 source kind (0 half, 1 uint8) i6 KS of the x table i7 KS of the y table (1..L2D_RESIZE_MAX_KS) i8 the source's
 *   row pitch in pixels (0: W; uint8 sources with B == 1 only: p0 is then the first pixel of an H x W window of a wider frame, at
 *   any byte).  One pass:
 *   out = clip((2^21 + sum_x in[xmin + x] k[xx][x]) >> 22, 0, 255), arithmetic shift, in 32-bit integers (the host asserts
 *   255 sum |k| + 2^21 < 2^31 for every row); x first, rounded to a uint8 image, then y.  An axis that keeps its size carries
 *   the identity table (KS 1, k = 2^22).  What the kernel reads from a table is clamped to the image and to KS.  Only bytes of
 *   [dst, dst + B Ho Wo 3) are written, by plain stores (whole dwords where the address allows, bytes at the ends of a row).
 *   Refused: Ho, Wo outside 1..L2D_RESIZE_MAX_SIZE or outside [n_in / 2, 8 n_in], KS outside 1..L2D_RESIZE_MAX_KS,
 *   B Ho Wo 3 >= 2^31, B > 65535, a null or misaligned table, an fp16 source that is not 4-byte aligned, a pitch below W or one
 *   beside an fp16 source or B > 1.
 *
 * Matte at the output size (matte.hip; no counterpart in the reference).
 * L2D_OP_FRAME_MATTE_UP  the styled frame at the output size composited over the camera's own pixels at that size by the matte of
 *   the stream-sized depth plane, one launch:  p0 styled uint8 [B][Ho][Wo][3] p1 camera uint8 [B][Ho][Wo][3] p2 depth half, plane
 *   b at p2 + b l0 elements, [H][W] p3 dst uint8 [B][Ho][Wo][3] (any alignment, as are p0 and p1) p4 table of the x axis p5 table
 *   of the y axis (int32, 4-byte aligned; for an axis of n_out outputs: i0 [n_out], i1 [n_out], the bits of the fp32 weight f
 *   [n_out] behind one another, as matte.up_table builds them: half-pixel bilinear taps) ; i0 B i1 H i2 W i3 Ho i4 Wo i5 r i6 flags
 *   (both as L2D_OP_FRAME_MATTE's) ; l0 depth plane stride in elements (>= H W) ; f0 lo f1 inv (as L2D_OP_FRAME_MATTE's).
 *   Arithmetic, every step one fp32 operation with one rounding and no fma (live2diff_amd/matte.py composite_up_ref): m as
 *   L2D_OP_FRAME_MATTE forms it at H x W, box filter included; a_y = m[y][x0] + fx (m[y][x1] - m[y][x0]) on rows y0 and y1;
 *   M = a_y0 + fy (a_y1 - a_y0); o = C + M (S - C) on the bytes; byte = rint(o), half to even.  SHOW writes rint(255 M) to all
 *   three channels and reads neither frame.  M == 1 gives p0's bytes, M == 0 p1's.  What the kernel reads from a table is
 *   clamped to the image, to the tile's patch and to [0, 1].  Only bytes of [dst, dst + B Ho Wo 3) are written, by plain stores
 *   (whole dwords where the address allows, bytes at the ends of a row).  Refused: a null pointer, Ho, Wo outside
 *   1..L2D_RESIZE_MAX_SIZE or outside [n_in / 2, 8 n_in], B Ho Wo 3 >= 2^31, B > 65535, r outside 0..L2D_MATTE_MAX_R, unknown
 *   flags, a depth stride below H W, a misaligned table, lo / inv as L2D_OP_FRAME_MATTE refuses them.
 *
 * Edge-aware matte (matte_edge.hip; no counterpart in the reference): the matte re-fitted locally as a linear function of the
 *   frame it cuts (a guided filter, He et al.), so that its edges land on the frame's own edges.
 * L2D_OP_FRAME_MATTE_EDGE  one launch:  p0 source half [3][H][W] p1 depth half [H][W] p2 out float [H][W] (all 16-byte aligned) ;
 *   i0 H i1 W (W % 8 == 0, 3 H W < 2^31) i2 r (1..L2D_MATTE_EDGE_MAX_R) i3 flags (L2D_MATTE_HARD | _FAR) ; l0 the BITS of the
 *   double E = double(n n) eps eps with n = (2r+1)^2 and eps >= 1 in byte levels (so E >= n n) ; f0 lo f1 inv (as
 *   L2D_OP_FRAME_MATTE's).  Arithmetic, exact integers and a few individually rounded fp64 operations, no fma, so that numpy
 *   restates it bit for bit (live2diff_amd/matte.py edge_ref): P = rint(255 m) with m as L2D_OP_FRAME_MATTE forms it in front
 *   of the feather; b = L2D_OP_FRAME_EGRESS' bytes of p0; Y = (77 R + 150 G + 29 B + 128) >> 8; S_I, S_P, S_II, S_IP the sums of
 *   Y, P, Y Y, Y P over the (2r+1) x (2r+1) window, coordinates clamped to the image; cov = n S_IP - S_I S_P and var = n S_II -
 *   S_I S_I in int64; a = double(cov) / (double(var) + E); A = rint(4096 a); bc = (double(S_P) - a double(S_I)) / double(n);
 *   B = rint(4096 bc) (both fit int32: |a| <= 127.5 / (2 eps)); Q = window_sum(A) Y + window_sum(B) in int64; q = double(Q) /
 *   double(n 4096 255); out = float(min(max(q, 0), 1)).  One work-group per 16 x 64 tile; Y and P of the tile and a halo of 2r as
 *   bytes in LDS, the sums separably.  Every element of p2 is written by a plain store on every launch: nothing has to be zeroed.
 *   Refused: a null or misaligned pointer, W % 8 != 0, 3 H W >= 2^31, r outside 1..L2D_MATTE_EDGE_MAX_R, unknown flags, an E
 *   that is not finite or below n n, lo / inv as L2D_OP_FRAME_MATTE refuses them.
 *   L2D_MATTE_EDGE_PLANE: p1 is a float plane [H][W] of ready matte values (p1 of L2D_OP_MASK_INGEST), 16-byte aligned, read
 *   where the tile and its halo are staged: P = rint(255 min(max(p1, 0), 1)); HARD, FAR, f0 and f1 are not read (HARD or FAR
 *   beside it is refused, and so is p2 overlapping p1).  With the flag clear every bit is as before.
 *
 * Steady (steady.hip; no counterpart in the reference).  Where the frame's source did not move since the source of the output
 *   before, the previous output pixel is held (a per-pixel EMA); where it moved, the styled pixel passes untouched.  The result is
 *   an fp16 frame in the decoder's convention that every outlet consumes unchanged, like L2D_OP_COLOR_LOCK's.
 * L2D_OP_FRAME_STEADY  one launch:  p0 styled half [3][H][W] p1 source half [3][H][W] p2 prev_out half [3][H][W] p3 prev_bytes uint8
 *   [3][H][W] (PLANAR: the bytes of the previous output's source, channel by channel) p4 out half [3][H][W] p5 next_bytes uint8
 *   [3][H][W] p6 picture half [3][H][W] (read as a pointer only with L2D_STEADY_SHOW; the half frames 16-byte aligned, the byte
 *   planes 8) ; i0 H i1 W (W % 8 == 0, 3 H W < 2^31) i2 r (0..L2D_STEADY_MAX_R) i3 flags (L2D_STEADY_HARD | _SHOW | _INIT) ; f0 lo
 *   f1 inv (1 / (hi - lo), both in byte levels; finite, not negative) f2 s (the strength, in [0, 1]).  Arithmetic, the motion in
 *   exact integers and every floating-point step one fp32 operation with one rounding and no fma, so that numpy restates it bit
 *   for bit (live2diff_amd/steady.py steady_ref): b = L2D_OP_FRAME_EGRESS' byte of p1; d = max over the channels of |b - p3|;
 *   D = the sum of d over the (2r+1) x (2r+1) window, coordinates clamped to the image; dbar = float(D) / float((2r+1)^2), one
 *   correctly rounded division; t = clamp((dbar - lo) inv, 0, 1) (HARD: dbar >= lo ? 1 : 0); w = (t t) (3 - 2 t) (1 moving,
 *   0 still); a = 1 - s (1 - w); o = half(P + a (S - P)), round to nearest even, and S's own bits where a == 1.  p4 = o and
 *   p5 = b are the next launch's p2 and p3: (p4, p5) ping-pong against (p2, p3), because a tile's halo reads its neighbours'
 *   previous bytes.  Every element of p4 and p5 is written by a plain store on every launch: nothing has to be zeroed.  SHOW
 *   also writes half(2 w - 1) to all three channels of p6 (the state p4 stays the blend).  INIT (the first frame of a sequence):
 *   o = S (p6 too), p5 = b, and p2 / p3 are not read -- they may be null or hold anything.  Inputs are finite.  r == 0 and INIT:
 *   one lane per 8 pixels; r > 0: one work-group per 16 x 64 tile, d of the tile and its halo, then the row sums, in LDS.
 *   Refused: a null pointer (p2 / p3 only with INIT, p6 only without SHOW), a misaligned one, W % 8 != 0, 3 H W >= 2^31, r
 *   outside 0..L2D_STEADY_MAX_R, unknown flags, p4 (or p6) overlapping p0, p1, p2 or one another, p5 overlapping p3, a
 *   non-finite or negative lo / inv, s outside [0, 1].
 *
 * Detail mode (detail.hip; no counterpart in the reference): the camera's fine detail in the frame at the output size, by the
 *   regression-based detail injection of pan-sharpening.  The styled frame is the low-resolution colour image, the camera's luma
 *   at the output size the high-resolution band, the gain the local regression slope of each styled channel on the source
 *   frame's luma (stage 1 of L2D_OP_FRAME_MATTE_EDGE's guided filter).  Exact integers and individually rounded operations, no
 *   fma, so that numpy restates both ops bit for bit (live2diff_amd/detail.py gains_ref, inject_ref).
 * L2D_OP_FRAME_DETAIL_GAIN  one launch:  p0 the frame L2D_OP_FRAME_RESIZE is about to read, half [3][H][W] (mapped to bytes with
 *   L2D_OP_FRAME_EGRESS' expression first) or, with L2D_DETAIL_U8, uint8 [H][W][3] p1 source half [3][H][W] p2 out int32 [3][H][W]
 *   (all 16-byte aligned) ; i0 H i1 W (W % 8 == 0, 3 H W < 2^31) i2 r (1..L2D_MATTE_EDGE_MAX_R) i3 flags (L2D_DETAIL_U8) ; l0 the
 *   BITS of the double E = double(n n) eps eps, as L2D_OP_FRAME_MATTE_EDGE's.  P[c] = the bytes of channel c of p0; Y = (77 R +
 *   150 G + 29 B + 128) >> 8 of L2D_OP_FRAME_EGRESS' bytes of p1; S_I, S_II, S_P, S_IP the sums of Y, Y Y, P, Y P over the
 *   (2r+1) x (2r+1) window, coordinates clamped to the image; cov = n S_IP - S_I S_P and var = n S_II - S_I S_I in int64;
 *   a = double(cov) / (double(var) + E); A = rint(4096 a) (|A| <= 261120); out[c] = the window sum of A, coordinates clamped:
 *   n 4096 times the mean gain, |out| <= 261120 n < 2^31.  One work-group per 16 x 64 tile; Y and the three P planes of the tile
 *   and a halo of 2r as bytes in LDS; S_I and S_II are formed once, S_P, S_IP, A and its sums channel by channel through one
 *   set of row-sum buffers.  Every element of p2 is written by a plain store on every launch: nothing has to be zeroed.
 *   Refused: a null or misaligned pointer, W % 8 != 0, 3 H W >= 2^31, r outside 1..L2D_MATTE_EDGE_MAX_R, unknown flags, an E
 *   that is not finite or below n n.
 * L2D_OP_FRAME_DETAIL  one launch:  p0 S, the styled frame at the output size p1 C, the camera's own pixels at that size p2 L, the
 *   source frame through the resize S went through (all uint8 [Ho][Wo][3], any alignment) p3 G int32 [3][H][W], p2 of
 *   L2D_OP_FRAME_DETAIL_GAIN p4 table of the x axis p5 table of the y axis (int32, 4-byte aligned, as L2D_OP_FRAME_MATTE_UP's) p6
 *   dst uint8 [Ho][Wo][3] (any alignment; overlapping none of p0..p2) ; i0 H i1 W i2 Ho i3 Wo i4 flags (L2D_DETAIL_SHOW) ; f0
 *   k = float(strength / (n 4096)) f1 limit (byte levels).  luma(x) = (77 R + 150 G + 29 B + 128) >> 8; d = luma(C) - luma(L);
 *   g = the bilinear taps of float(G[c]): a_y = g[y][x0] + fx (g[y][x1] - g[y][x0]) on rows y0 and y1, a_y0 + fy (a_y1 - a_y0);
 *   t = g float(d); u = t k; u = min(max(u, -limit), limit); o = min(max(float(S) + u, 0), 255); byte = rint(o), half to even,
 *   every step one fp32 operation.  SHOW writes rint(min(max(128 + u, 0), 255)) per channel and does not read p0.  C == L, k == 0
 *   and G == 0 each give p0's bytes; |byte - S| <= ceil(limit).  One work-group per 32 x 32 output tile, the gains its taps
 *   reach staged in LDS as floats.  What the kernel reads from a table is clamped to the image, to the tile's patch and to
 *   [0, 1].  Only bytes of [dst, dst + Ho Wo 3) are written, by plain stores (whole dwords where the address allows, bytes at
 *   the ends of a row).  Refused: a null pointer, Ho, Wo outside 1..L2D_RESIZE_MAX_SIZE or outside [n_in / 2, 8 n_in], Ho Wo 3 or
 *   3 H W >= 2^31, misaligned tables or G, unknown flags, a limit or k that is not finite or negative, dst overlapping an input.
 *
 * Depth from the caller (depth_in.hip; no counterpart in the reference): a depth frame in place of the detector's.  Individually
 *   rounded fp32 operations, no fma, so that numpy restates both ops bit for bit (live2diff_amd/depth_io.py resample_ref,
 *   normalize_ref).
 * L2D_OP_DEPTH_INGEST  one launch:  p0 src uint16 or (L2D_DEPTH_F32) float [B][Hd][Wd] p1 R float [B][H][W] (16-byte aligned) p2
 *   partials float [B tiles][3] p3 xmin int32 [W] p4 wx float [W][Kx] p5 ymin int32 [H] p6 wy float [H][Ky] (rows [left, left + W)
 *   and [top, top + H) of frame_io.aa_weights(Wd, nw) / (Hd, nh); a tap past a row's own count has weight 0) ; i0 B i1 Hd i2 Wd i3 H
 *   i4 W i5 nh i6 nw i7 top i8 left (L2D_OP_FRAME_INGEST's geometry, of the depth frame's own size) i9 Kx i10 Ky (1..
 *   L2D_DEPTH_MAX_TAPS) i11 flags i12 the invalid uint16 value ; f0 the invalid fp32 value.  Per sample: valid when (uint16) z !=
 *   invalid or (fp32) z finite and != invalid -- with L2D_DEPTH_HAS_INVALID, else no value is excluded --, and u finite and >= 0,
 *   u = float(z) or (L2D_DEPTH_DISTANCE) 1 / float(z); u = 0, v = 0 where not valid, v = 1 where valid.  num = sum_y wy (sum_x wx
 *   u), den = sum_y wy (sum_x wx v), taps ascending, every product and sum rounded to fp32; R = num / den where den > 0, else -1.
 *   partials[(b tiles_y + ty) tiles_x + tx] = {min, max, any} of R over the valued pixels of tile (ty, tx) of L2D_DEPTH_TILE_H x
 *   L2D_DEPTH_TILE_W pixels ({+inf, -1, 0} where there is none).  Every element of p1 and p2 is written by a plain store on
 *   every launch: nothing has to be zeroed.  Table entries are clamped to the image.  Refused: a null or misaligned pointer, a
 *   non-positive size, B Hd Wd or B H W >= 2^31, B > 65535, a window outside the resized image, a scale above 8, taps outside
 *   1..L2D_DEPTH_MAX_TAPS, unknown flags, an invalid value that is no uint16.
 * L2D_OP_DEPTH_NORMALIZE  one launch:  p0 R float [B][H][W] p1 partials (of all B frames) p2 out half [B][3][H][W] (p0, p2 16-byte
 *   aligned) ; i0 B i1 H i2 W (H W % 8 == 0) i3 the number of partials (B tiles) i4 flags (L2D_DEPTH_FIXED_RANGE) ; f0 mn f1 mx of
 *   the fixed range.  mn, mx = min, max over all partials (every block, in a fixed order), or f0, f1; n = min(max((R - mn) / (mx -
 *   mn), 0), 1); out = half(2 n - 1) on the three planes; -1 where R < 0, and everywhere where the map is flat: with the partials,
 *   no pixel has a value or float(mx - mn) <= float(mx 2^-14) (that holds mx <= mn and the rounding noise of the resampling of a
 *   constant frame); with L2D_DEPTH_FIXED_RANGE, mx <= mn only.
 *   Refused: a null or misaligned pointer, a non-positive size, H W % 8 != 0, 3 B H W >= 2^31, unknown flags, a partial count
 *   that is not B tiles, a NaN in the fixed range.
 *
 * Backdrop (backdrop.hip; no counterpart in the reference): the source frame blurred with the subject left out, as the kept part
 *   of the matte composite -- p1 of L2D_OP_FRAME_MATTE, or through L2D_OP_FRAME_RESIZE p1 of L2D_OP_FRAME_MATTE_UP.
 * L2D_OP_FRAME_BACKDROP_BLUR  one launch:  p0 source half [3][H][W] p1 depth half [H][W] p2 out half [3][H][W] (all 16-byte
 *   aligned; p2 overlaps neither input) ; i0 H i1 W (W % 8 == 0, 3 H W < 2^31) i2 r (1..L2D_BACKDROP_MAX_R) i3 passes
 *   (1..L2D_BACKDROP_MAX_PASSES) i4 flags (L2D_MATTE_HARD | _FAR) ; f0 lo f1 inv (as L2D_OP_FRAME_MATTE's).  Exact integers, so
 *   that numpy restates it bit for bit (live2diff_amd/backdrop.py blur_ref, frame_of): P[c] = L2D_OP_FRAME_EGRESS' bytes of
 *   channel c of p0; M = rint(255 m) with m as L2D_OP_FRAME_MATTE forms it in front of the feather; W = 256 - M, 1..256, never 0;
 *   then `passes` times, with n = (2r+1)^2 and sums over the (2r+1) x (2r+1) window, coordinates clamped to the image:
 *   D = sum W, N[c] = sum W P[c], P[c] = (2 N[c] + D) / (2 D) (floor: the weighted mean, rounded half up), W = (D + n - 1) / n
 *   (floor: 1..256 again); 2 N + D <= 2 n 256 255 + 256 n < 2^32.  out[c] = half(float(P[c]) float(2 / 255) - 1), two fp32
 *   operations and one rounding: the value L2D_OP_FRAME_EGRESS' expression maps back to the byte P[c].  One work-group per
 *   16 x 64 tile; the three byte planes and W - 1 as a byte of the tile and a halo of passes r in LDS, every pass there on a
 *   region that shrinks by r, the sums separably.  Every element of p2 is written by a plain 16-byte store on every launch:
 *   nothing has to be zeroed.  Refused: a null or misaligned pointer, W % 8 != 0, 3 H W >= 2^31, r outside
 *   1..L2D_BACKDROP_MAX_R, passes outside 1..L2D_BACKDROP_MAX_PASSES, unknown flags, p2 overlapping p0 or p1, lo / inv as
 *   L2D_OP_FRAME_MATTE refuses them.
 *   L2D_BACKDROP_PLANE: p1 is a float plane [H][W] of ready matte values (p1 of L2D_OP_MASK_INGEST), 16-byte aligned, read
 *   where the tile and its halo are staged: W = 256 - rint(255 min(max(p1, 0), 1)); HARD, FAR, f0 and f1 are not read (HARD or
 *   FAR beside it is refused).  With the flag clear every bit is as before.
 *
 * Follow (steady_follow.hip; no counterpart in the reference): steady along the source's motion.  L2D_OP_FRAME_STEADY compares the
 *   source bytes at the same coordinates, so under a moving camera it holds nothing; these two ops find, per 8 x 8 block, where in
 *   the previous frame to look, and run the same arithmetic there.  Exact integers in the search, L2D_OP_FRAME_STEADY's operations
 *   behind it, so that numpy restates both bit for bit (live2diff_amd/steady.py motion_ref, follow_ref).
 * L2D_OP_FRAME_MOTION  one launch:  p0 source half [3][H][W] (16-byte aligned) p1 prev_bytes uint8 [3][H][W] (planar, 8-byte aligned:
 *   p3 of L2D_OP_FRAME_STEADY) p2 field int8 [ceil(H/8)][W/8][2] (dy, dx per block; any alignment) ; i0 H i1 W (W % 8 == 0, 3 H W <
 *   2^31) i2 search R (1..L2D_FOLLOW_MAX_SEARCH) i3 bias (0..L2D_FOLLOW_MAX_BIAS).  now = L2D_OP_FRAME_EGRESS' bytes of p0.  The
 *   window of block (i, j) is rows 8i - L2D_FOLLOW_APRON .. 8i + 11 and columns 8j - 4 .. 8j + 11; cost(dy, dx) = the sum over the
 *   window and the three channels of |now[c][cl(y)][cl(x)] - p1[c][cl(y + dy)][cl(x + dx)]|, every coordinate clamped to the image
 *   on its own (<= 768 * 255); key = (cost + bias (|dy| + |dx|)) 512 + rank, rank the position of (dy, dx) among [-R, R]^2 in the
 *   order (|dy| + |dx|, dy, dx) (key < 2^27); the block's vector is the candidate of the smallest key: ties go to the shortest
 *   vector, then the smaller dy, then the smaller dx, and the zero vector wins any tie.  bias is in summed byte levels per pixel of
 *   L1 displacement.  One work-group per strip of eight blocks: now of its windows (16 x 72 x 3 bytes) and p1 with the search
 *   margin (at most 32 x 88 x 3) staged once in LDS, clamped while staged; 32 lanes per block take the candidates, four
 *   neighbouring dx at a time, with v_sad_u8; the minimum over the packed keys goes through LDS -- no atomics, any order gives
 *   the same field.  Every block of p2 is written by plain stores on every launch: nothing has to be zeroed.  Refused: a null or
 *   misaligned pointer, W % 8 != 0, 3 H W >= 2^31, R or bias out of range, p2 overlapping p0 or p1.
 * L2D_OP_FRAME_STEADY_FOLLOW  one launch:  p0 .. p6 as L2D_OP_FRAME_STEADY's p7 field int8 [ceil(H/8)][W/8][2] (p2 of
 *   L2D_OP_FRAME_MOTION; any alignment) ; i0 H i1 W i2 r (0..L2D_STEADY_MAX_R) i3 flags (L2D_STEADY_HARD | _SHOW; an init frame is
 *   L2D_OP_FRAME_STEADY's: it looks nowhere) ; f0 lo f1 inv f2 s.  With (dy, dx) the vector of block (y / 8, x / 8):
 *   bp[c][y][x] = p3[c][cl(y + dy)][cl(x + dx)] and P[c][y][x] = p2[c][cl(y + dy)][cl(x + dx)]; then L2D_OP_FRAME_STEADY's
 *   arithmetic on them, operation for operation: d = max_c |b - bp| (each pixel with its own block's vector), its window sum with
 *   clamped coordinates, dbar, t, w, a, o = half(P + a (S - P)) and S's own bits where a == 1, SHOW.  p4 = o and p5 = b (the
 *   bytes of p1 where they are, not displaced) are the next frame's p2 and p3.  An all-zero field gives L2D_OP_FRAME_STEADY's
 *   bits.  A vector is used only through clamped coordinates: whatever p7 holds, nothing outside p2 and p3 is read.  One
 *   work-group per 16 x 64 tile, d of the tile and its halo, then the row sums, in LDS, as L2D_OP_FRAME_STEADY's tile form (r = 0
 *   takes the same kernel); an 8-aligned pixel group lies inside one block, so it has one vector.  Every element of p4 and p5 is
 *   written by a plain store on every launch.  Refused: a null pointer (p6 only without SHOW), a misaligned one, W % 8 != 0,
 *   3 H W >= 2^31, r out of range, unknown flags (INIT among them), p4 (or p6) overlapping p0 .. p3 or one another, p5
 *   overlapping p0 .. p3, p7 overlapping p4, p5 or p6, lo / inv / s as L2D_OP_FRAME_STEADY refuses them.
 *
 * Matte hold (matte_hold.hip; no counterpart in the reference): the matte filtered in time where the camera holds still.  The
 *   depth matte is a fresh draw in every frame, so its silhouette crawls while nothing moves; this op blends the frame's matte,
 *   in front of the feather, with the previous held one by L2D_OP_FRAME_STEADY's measure of where the source moved.  Its output
 *   plane is what L2D_OP_FRAME_MATTE and L2D_OP_FRAME_MATTE_UP then read under L2D_MATTE_PLANE.
 * L2D_OP_FRAME_MATTE_HOLD  one launch:  p0 source half [3][H][W] p1 the matte input: depth half [H][W], or with
 *   L2D_MATTE_HOLD_PLANE float [H][W] (p2 of L2D_OP_FRAME_MATTE_EDGE) p2 prev_plane float [H][W] p3 prev_bytes uint8 [3][H][W]
 *   (planar) p4 out_plane float [H][W] p5 next_bytes uint8 [3][H][W] p6 field int8 [ceil(H/8)][W/8][2] (p2 of L2D_OP_FRAME_MOTION,
 *   read only with L2D_MATTE_HOLD_FOLLOW; any alignment; the planes and the frame 16-byte aligned, the byte planes 8) ; i0 H i1 W
 *   (W % 8 == 0, 3 H W < 2^31) i2 r (0..L2D_STEADY_MAX_R) i3 flags (L2D_MATTE_HOLD_*) i4 i5 the BITS of the floats lo and inv of
 *   the depth ramp (as L2D_OP_FRAME_MATTE's f0 f1; not read with PLANE) ; f0 lo f1 inv f2 s (as L2D_OP_FRAME_STEADY's: the motion
 *   ramp in byte levels and the strength).  Arithmetic, the motion in exact integers and every floating-point step one fp32
 *   operation with one rounding and no fma, so that numpy restates it bit for bit (live2diff_amd/matte.py hold_ref): m0 = the
 *   matte as L2D_OP_FRAME_MATTE forms it in front of the feather (RAMP_HARD, RAMP_FAR), or p1's values; b, d, D, dbar, t, w as
 *   L2D_OP_FRAME_STEADY's with p3 as the previous bytes (HARD); a = 1 - s (1 - w); h = P + a (m0 - P) with P = p2; h = min(max(h,
 *   min(m0, P)), max(m0, P)) -- the fp32 blend may leave the interval by an ulp, the clamp is part of the arithmetic: h stays in
 *   [0, 1], and exactly 0 or 1 where m0 and P both are --; m0's own bits where a == 1.  FOLLOW: P and the previous bytes are
 *   fetched at (cl(y + dy), cl(x + dx)) with (dy, dx) the vector of block (y / 8, x / 8), as L2D_OP_FRAME_STEADY_FOLLOW's; every
 *   coordinate is clamped on its own, so whatever p6 holds, nothing outside p2 and p3 is read.  p4 = h and p5 = b (where they
 *   are, not displaced) are the next launch's p2 and p3: the two records ping-pong, because a tile's halo and a displaced fetch
 *   read what a neighbour would write.  INIT: h = m0, p5 = b, and p2, p3 and p6 are not read -- they may be null.  One
 *   work-group per 16 x 64 tile for every r, 8 pixels per lane: the lane's source, matte input and previous record are loaded
 *   first (16-byte accesses to the planes, 8-byte to the bytes; displaced element loads under FOLLOW), d of the tile and its
 *   halo, then the row sums, go through 6,656 bytes of LDS.  Every element of p4 and p5 is written by a plain store on every
 *   launch: nothing has to be zeroed, no atomics.  Refused: a null pointer (p2, p3 only with INIT, p6 with INIT or without
 *   FOLLOW), a misaligned one, W % 8 != 0, 3 H W >= 2^31, r out of range, unknown flags, ramp flags beside PLANE, lo / inv / s as
 *   L2D_OP_FRAME_STEADY refuses them, the depth ramp as L2D_OP_FRAME_MATTE refuses it, p4 or p5 overlapping p0 .. p3 or each
 *   other, p6 overlapping p4 or p5.
 *
 * The matte from the caller (mask_in.hip; no counterpart in the reference): a mask of any size and sample type becomes the raw
 *   matte plane at the stream's size, in place of the depth ramp or combined with it.  Individually rounded fp32 operations, no
 *   fma, so that numpy restates it bit for bit (live2diff_amd/mask_io.py mask_ref, front_ref).
 * L2D_OP_MASK_INGEST  one launch:  p0 mask uint8, (L2D_MASK_U16) uint16 or (L2D_MASK_F32) float [Hm][Wm] (aligned to its element)
 *   p1 out float [H][W] (16-byte aligned) p2 depth half [H][W] (read only with L2D_MASK_AND / _OR; may be null without) p3 xmin
 *   int32 [W] p4 wx float [W][Kx] p5 ymin int32 [H] p6 wy float [H][Ky] (the tables of L2D_OP_DEPTH_INGEST, of the mask's own
 *   size) ; i0 Hm i1 Wm i2 H i3 W i4 nh i5 nw i6 top i7 left (L2D_OP_FRAME_INGEST's geometry, of the mask's own size) i8 Kx i9 Ky
 *   (1..L2D_DEPTH_MAX_TAPS) i10 flags (L2D_MASK_*) ; f0 lo f1 inv of the depth ramp (as L2D_OP_FRAME_MATTE's; read only with AND /
 *   OR).  Per sample v = float(s) / 255 (uint8), float(s) / 65535 (uint16), min(max(x, 0), 1) with NaN -> 0 (float).  r = sum_y wy
 *   (sum_x wx v), the horizontal pass first, taps ascending, every product and sum rounded to fp32; P = rint(255 min(max(r, 0),
 *   1)), half to even; INVERT: P = 255 - P; mu = float(P) / 255; out = mu, or with AND min(m_r, mu), with OR max(m_r, mu), m_r
 *   the matte as L2D_OP_FRAME_MATTE forms it of p2 in front of the feather (RAMP_HARD, RAMP_FAR).  The mask is quantised to byte
 *   levels at the stream's size: a constant mask comes back exactly 0 or 1, and rint(255 out) of a replacing mask is P.  One
 *   work-group per L2D_DEPTH_TILE_H x L2D_DEPTH_TILE_W output tile, the horizontal sums of the source rows its taps reach in
 *   20,736 bytes of LDS, then the vertical pass.  Every element of p1 is written by a plain store on every launch: nothing has
 *   to be zeroed, no atomics; W may be any width.  Table entries are clamped to the image.  Refused: a null or misaligned
 *   pointer, a non-positive size, Hm Wm or H W >= 2^31, a window outside the resized image, a scale above 8, taps outside
 *   1..L2D_DEPTH_MAX_TAPS, unknown flags, two sample types or two combines at once, ramp flags without AND / OR, the ramp as
 *   L2D_OP_FRAME_MATTE refuses it, p1 overlapping p0 or p2.
 *
 * Matte key (matte_key.hip; no counterpart in the reference): the raw matte plane from a comparison of the frame's source, on
 *   the bytes a viewer would see, against a key colour or a clean plate -- the third source of a matte beside the depth ramp and
 *   L2D_OP_MASK_INGEST, and written exactly as that op writes its plane.  Exact integers, then individually rounded fp32
 *   operations, no fma, so that numpy restates it bit for bit (live2diff_amd/matte_key.py key_ref, mask_io.front_ref).
 * L2D_OP_MATTE_KEY  one launch:  p0 source half [3][H][W] p1 out float [H][W] p2 depth half [H][W] (read only with
 *   L2D_MATTE_KEY_AND / _OR; may be null without) p3 plate uint8 [3][H][W], planar (read only with L2D_MATTE_KEY_PLATE; may be
 *   null without; 8-byte aligned, the others 16) ; i0 H i1 W (W % 8 == 0, 3 H W < 2^31) i2 r (0..L2D_MATTE_KEY_MAX_R) i3 flags
 *   (L2D_MATTE_KEY_*) i4 L = rint(256 luma) (0..256) i5 i6 i7 the key colour's bytes R G B (not read with PLATE) ; f0 lo2 f1 inv
 *   of the key's ramp over the mean squared distance (lo2 = lo^2, inv = 1 / (hi^2 - lo^2), lo and hi in byte levels) f2 lo f3
 *   inv of the depth ramp (as L2D_OP_FRAME_MATTE's f0 f1; read only with AND / OR).  b = the egress bytes of p0, k = the key;
 *   dR, dG, dB = b - k; dy = (77 dR + 150 dG + 29 dB + 128) >> 8 (arithmetic shift); cb = dB - dy, cr = dR - dy; D = cb^2 + cr^2
 *   + ((L dy^2 + 128) >> 8) <= 585,225 < 2^20; S = the sum of D over the (2 r + 1)^2 window, coordinates clamped to the image
 *   (< 2^31); mean = float(S) / float((2 r + 1)^2); t = clamp((mean - lo2) inv, 0, 1) (HARD: mean >= lo2); m = t t (3 - 2 t); P
 *   = rint(255 m), half to even; INVERT: P = 255 - P; mu = float(P) / 255; out = mu, or with AND min(m_r, mu), with OR max(m_r,
 *   mu), m_r the matte as L2D_OP_FRAME_MATTE forms it of p2 in front of the feather (RAMP_HARD, RAMP_FAR).  One work-group per
 *   16 x 64 tile for every r, 8 pixels per lane; D of the tile and its halo, then the row sums, go through 13,824 bytes of LDS
 *   as 32-bit integers.  Every element of p1 is written by a plain store on every launch: nothing has to be zeroed, no atomics.
 *   Refused: a null or misaligned pointer, W % 8 != 0, 3 H W >= 2^31, r, L or a key byte out of range, unknown flags, two
 *   combines at once, ramp flags without AND / OR, lo2 or inv negative or not finite, inv == 0 without HARD or HARD with inv !=
 *   0, the depth ramp as L2D_OP_FRAME_MATTE refuses it, p1 overlapping p0, p2 or p3.
 * L2D_OP_FRAME_PLANAR_BYTES  one launch (the plate capture):  p0 source half [3][H][W] p1 out uint8 [3][H][W], planar (both
 *   16-byte aligned) ; i0 H i1 W (W % 8 == 0, 3 H W < 2^31).  out = the egress bytes of p0 (L2D_OP_FRAME_EGRESS's byte), one
 *   lane per 8 pixels, plain stores.  Refused: a null or misaligned pointer, W % 8 != 0, 3 H W >= 2^31, p1 overlapping p0.
 * L2D_OP_MATTE_KEY_ADAPT  one launch (the plate key over a plate that follows drifting light; live2diff_amd/matte_key.py
 *   key_adapt_ref):  p0 source p1 out p2 depth as L2D_OP_MATTE_KEY's p3 plate uint8 [3][H][W], planar (read only with
 *   L2D_MATTE_KEY_ADAPT_INIT; may be null without; 8-byte aligned) p4 state in uint16 [3][H][W], planar (null under INIT) p5 state
 *   out uint16 [3][H][W] (both 16-byte aligned) ; i0 H i1 W i2 r i3 flags (L2D_OP_MATTE_KEY's -- L2D_MATTE_KEY_PLATE is not read:
 *   there is always a plate -- and L2D_MATTE_KEY_ADAPT_INIT) i4 L i5 a_bg = rint(65536 rate) i6 a_fg = rint(65536 absorb) (both
 *   0..L2D_MATTE_KEY_MAX_RATE) ; f0 lo2 f1 inv f2 lo f3 inv as L2D_OP_MATTE_KEY's.  The state s is the plate in 8.8 fixed point, 0
 *   <= s <= 65280 (INIT: s = 256 p3); the key's byte is k = (s + 128) >> 8, and p1 is formed and written exactly as
 *   L2D_OP_MATTE_KEY with a plate of those bytes writes it.  P0 = P in front of INVERT (an integer 0..255); a = (a_bg (255 - P0) +
 *   a_fg P0 + 127) / 255; per channel, with b the egress byte of p0: e = 256 b - s, s' = s + ((a e + 32768) >> 16) (arithmetic
 *   shift); |a e| + 32768 <= 2,139,127,808 < 2^31 and s' stays in 0..65280.  p5 = s' is the next launch's p4: the two records
 *   ping-pong, because a tile's halo reads what a neighbour would write.  L2D_OP_MATTE_KEY's tile form (13,824 bytes of LDS);
 *   behind the plane's stores each lane writes the three channels of its 8 pixels with 16-byte stores; the state is read with
 *   16-byte loads (element loads for the edge pixel a group beside the image repeats).  Every element of p1 and p5 is written by
 *   a plain store on every launch: nothing has to be zeroed, no atomics.  Refused: everything L2D_OP_MATTE_KEY refuses, a rate out
 *   of range, p5 (without INIT also p4) null or misaligned, INIT without p3, p5 overlapping p0 .. p4, p1 overlapping p4.
 * L2D_OP_MATTE_KEY_GAIN_HIST  one launch (the plate gain's samples; live2diff_amd/matte_key.py gain_hist_ref):  p0 source half
 *   [3][H][W] (16-byte aligned) p1 plate uint8 [3][H][W], planar (8-byte aligned), or with L2D_MATTE_KEY_GAIN_STATE the state
 *   uint16 [3][H][W] of L2D_OP_MATTE_KEY_ADAPT (16-byte aligned), whose byte is k = (s + 128) >> 8 p2 partials uint32
 *   [nblk][3][512] (16-byte aligned) ; i0 H i1 W (W % 8 == 0, 3 H W < 2^31) i2 flags (L2D_MATTE_KEY_GAIN_STATE) i3 nblk =
 *   ceil(H W / L2D_MATTE_KEY_GAIN_BLOCK).  Per pixel and channel, with b the egress byte of p0: the sample is valid when 16 <= k
 *   <= 239 and 4 <= b <= 251; q = min(511, (128 b + (k >> 1)) / k), the floor exactly; partial[block][c][q] counts the block's
 *   valid samples.  One work-group of 512 lanes per L2D_MATTE_KEY_GAIN_BLOCK consecutive pixels (the last one ragged), 8 pixels
 *   per lane: 16-byte loads of the fp16 rows, 8-byte loads of the plate (16-byte loads of the state); the block's
 *   histogram is held in 6,144 bytes of LDS under integer LDS atomics (sums do not depend on order) and every entry of its
 *   partial is written by a plain store: nothing has to be zeroed, no atomics on global memory.  Refused: a null or misaligned
 *   pointer, W % 8 != 0, 3 H W >= 2^31, unknown flags, an nblk that is not ceil(H W / L2D_MATTE_KEY_GAIN_BLOCK), p2 overlapping
 *   p0 or p1.
 * L2D_OP_MATTE_KEY_GAIN  one launch (the plate gain; live2diff_amd/matte_key.py gain_of):  p0 partials uint32 [nblk][3][512] p1
 *   record int32 [8] (both 16-byte aligned) ; i0 H i1 W i2 nblk (as L2D_OP_MATTE_KEY_GAIN_HIST's) i3 lim = rint(128 limit)
 *   (128..511) i4 min_count (0..H W).  hist[c][q] = the sum of the partials; n_c = the sum of hist[c]; g_c = 128 if n_c <
 *   min_count, else the smallest q with 2 cum_c(q) >= n_c (the lower median) clamped to [ceil(16384 / lim), lim]; the record is
 *   {g_r, g_g, g_b, n_r, n_g, n_b, 0, 0}, in units of 1 / 128.  One work-group of 1,024 lanes: lanes j and 512 + j sum bin j of each
 *   channel over the even and the odd partials, an inclusive scan in 6,144 bytes of LDS finds the medians; plain stores.  Every count is at most H W < 2^31
 *   / 3, so 2 cum fits 32 bits.  Refused: a null or misaligned pointer, W % 8 != 0, 3 H W >= 2^31, an nblk that does not match H
 *   W, lim or min_count out of range, p1 overlapping p0.
 * L2D_MATTE_KEY_GAIN on L2D_OP_MATTE_KEY (with L2D_MATTE_KEY_PLATE) and L2D_OP_MATTE_KEY_ADAPT:  p6 record int32 [8] of
 *   L2D_OP_MATTE_KEY_GAIN (16-byte aligned; g_c in 0..511, read by ordinary loads).  The key's byte becomes k' = min(255, (g_c k +
 *   64) >> 7) (g_c k + 64 <= 511 * 255 + 64 < 2^17; g_c = 128: k' = k, the unflagged launch bit for bit) and everything else is as
 *   without: under L2D_OP_MATTE_KEY_ADAPT the state still moves towards the source's own bytes, e = 256 b - s.  Compile-time
 *   variants of the same tile body (13,824 bytes of LDS).  Refused: the flag with a colour key, p6 null or misaligned, p1
 *   (L2D_OP_MATTE_KEY_ADAPT: or p5) overlapping p6.
 *
 * Re-warm (sink_commit.hip; the reference rewrites the sink slots only by running `prepare` again).
 * L2D_OP_SINK_COMMIT  the sink slots 0..F-1 of every (row, k|v, token) line of every layer's KV cache copied from a source cache
 *   list into a destination list, ONE launch however many layers:  p0 table of l2d_sink_rec in DEVICE memory (16-byte aligned) p1
 *   the same table in HOST memory (read by the launcher only, to validate and to size the grid) ; i0 number of records.  A record is
 *   one layer (below): `lines` = N * 2 * h * w lines, of which the first `line_bytes` = F * C * 2 bytes are copied; line j of the
 *   destination starts at dst + j * dst_pitch (L * C * 2), of the source at src + j * src_pitch (the same, or F * C * 2 for a compact
 *   source).  Every work-group walks all records and takes the 16-byte vectors blockIdx.x * 256 + lane, + gridDim.x * 256, ... of
 *   each; offsets are int32 counts of 16-byte vectors.  16-byte loads and stores only; bits are moved as they are: no arithmetic, no
 *   atomics, nothing zeroed, and nothing outside the first line_bytes of a destination line is written.  Refused: a null or not
 *   16-byte aligned table, dst or src; no records; lines <= 0; line_bytes or a pitch that is not a positive multiple of 16;
 *   line_bytes above either pitch; lines * pitch / 16 >= 2^31 for either pitch; a record whose destination range [dst, dst +
 *   (lines - 1) dst_pitch + line_bytes) overlaps its source range.
 *
 * Cut detection (cut.hip; live2diff_amd/cut.py is the arithmetic, held to equality; not in the reference).  A state is (thumb
 * uint16 [H/8][W/8], hist uint32 [64], rec int32 [8]); two of them ping-pong.  H and W are multiples of 8 and H W <= 2^22.
 * L2D_OP_FRAME_CUT_SIG  one launch (cut.signature_ref and the shares of Dt):  p0 source half [3][H][W] p1 the thumbnail of the frame
 *   before, uint16 [H/8][W/8] (NULL and not read under L2D_CUT_INIT) p2 thumbnail out p3 partials uint32 [nwg][68] (all 16-byte
 *   aligned) ; i0 H i1 W i2 flags (L2D_CUT_INIT) i3 nwg = ceil(H / 64) ceil(W / 64).  Per pixel Y = the integer luma (77 R + 150 G +
 *   29 B + 128) >> 8 of the egress bytes of p0; p2[by][bx] = the sum of Y over the 8 x 8 block (<= 16,320); partial[tile] = {the 64
 *   counts of Y >> 2 over the tile, the tile's share of Dt = sum |p2 - p1| (0 under INIT), 0, 0, 0}.  One work-group of 512 lanes
 *   per 64 x 64 pixels, ragged in whole blocks at the right and the bottom: a wave is one row of 8 blocks, a lane one 8-pixel row
 *   of a block (16-byte loads), the block sums are cross-lane adds, the histogram and the share live in 272 bytes of LDS under
 *   integer LDS adds.  Every entry of p2 and p3 is written by a plain store on every launch: nothing has to be zeroed, no atomics
 *   on global memory.  Refused: a size that is not a positive multiple of 8 or H W > 2^22, a wrong nwg, unknown flags, a null
 *   (p1: without INIT) or misaligned pointer, p2 or p3 overlapping p0, p1 or each other.
 * L2D_OP_FRAME_CUT  one launch (cut.measure_ref):  p0 partials p1 hist of the frame before, uint32 [64] p2 its record, int32 [8]
 *   (p1, p2: NULL and not read under L2D_CUT_INIT) p3 hist out p4 record out (all 16-byte aligned) ; i0 H i1 W i2 nwg i3 flags
 *   (L2D_CUT_INIT) i4 Tt (0..255 H W) i5 Th (0..2 H W) i6 R (0, or 256..16384: 256 times the ratio) i7 gap (0..255).  hist = the
 *   partials' sum, Dt = the shares' sum (64-bit), Dh = sum |hist - p1|; the record is {cut, Dt, Dh, since, n, E_lo, E_hi, flags}: E
 *   an int64 in units of 256 Dt, the running level over the frames that were not cuts, bit 0 of flags "has a level".  INIT writes
 *   {0, 0, 0, L2D_CUT_NEVER, 0, 0, 0, 0}.  Otherwise s = min(since' + 1, 2^30), cut = Dt >= Tt and Dh >= Th and s > gap and (R == 0
 *   or no level or 65536 Dt >= R E); on a cut since = 0 and E stays; else since = s and E = 256 Dt without a level, E + ((256 Dt -
 *   E) >> 3) (a floor shift) with one; n = n' + 1.  One work-group of 256 lanes, 1,056 bytes of LDS; plain stores.  Refused: what
 *   L2D_OP_FRAME_CUT_SIG refuses of the size, nwg and the flags, a null (p1, p2: without INIT) or misaligned pointer, a threshold
 *   out of range, p3 or p4 overlapping p0, p1, p2 or each other.
 */
enum {
    L2D_OP_IGEMM = 1,
    L2D_OP_GN_STATS = 2,
    L2D_OP_GN_APPLY = 3,
    L2D_OP_LAYERNORM = 4,
    L2D_OP_FLASH_ATTN = 5,
    L2D_OP_TATTN_STREAM = 6,
    L2D_OP_TATTN_WARMUP = 7,
    L2D_OP_SKINNY_LINEAR = 8,
    L2D_OP_TIMESTEP_EMBED = 9,
    L2D_OP_NCHW_TO_NHWC = 10,
    L2D_OP_NHWC_TO_NCHW = 11,
    L2D_OP_LCM_STEP = 12,
    L2D_OP_COPY = 13,
    L2D_OP_RING_UPDATE = 14,
    L2D_OP_STREAM_SHIFT = 15,
    L2D_OP_RANDN = 16,
    L2D_OP_RESIZE_BILINEAR = 17,
    L2D_OP_MINMAX = 18,
    L2D_OP_DEPTH_NORM_RESIZE = 19,
    L2D_OP_STEM7X7 = 20,
    L2D_OP_RESAMPLE_NHWC = 21,
    L2D_OP_EW = 22,
    L2D_OP_ROWGEMM = 23,
    L2D_OP_PCONV = 24,
    L2D_OP_WSGEMM = 25,
    L2D_OP_ROWCHAIN = 26,
    L2D_OP_CCONV = 27,
    L2D_OP_CLIP_EMBED = 28,
    L2D_OP_CLIP_ATTN = 29,
    L2D_OP_CLIP_LINEAR = 30,
    L2D_OP_CLIP_LN = 31,
    L2D_OP_VAE_ATTN = 32,
    L2D_OP_VAE_POSTERIOR = 33,
    L2D_OP_FRAME_INGEST = 34,
    L2D_OP_FRAME_EGRESS = 35,
    L2D_OP_JPEG_DCT = 36,
    L2D_OP_JPEG_HUFF = 37,
    L2D_OP_JPEG_PACK = 38,
    L2D_OP_JPEG_ENTROPY_DEC = 39,
    L2D_OP_JPEG_IDCT = 40,
    L2D_OP_JPEG_RGB = 41,
    L2D_OP_WEIGHT_BLEND = 42,
    L2D_OP_FRAME_MATTE = 43,
    L2D_OP_FRAME_MOMENTS = 44,
    L2D_OP_COLOR_LOCK = 45,
    L2D_OP_FRAME_RESIZE = 46,
    L2D_OP_FRAME_MATTE_UP = 47,
    L2D_OP_FRAME_STEADY = 48,
    L2D_OP_FRAME_MATTE_EDGE = 49,
    L2D_OP_FRAME_DETAIL_GAIN = 50,
    L2D_OP_FRAME_DETAIL = 51,
    L2D_OP_DEPTH_INGEST = 52,
    L2D_OP_DEPTH_NORMALIZE = 53,
    L2D_OP_FRAME_BACKDROP_BLUR = 54,
    L2D_OP_FRAME_MOTION = 55,
    L2D_OP_FRAME_STEADY_FOLLOW = 56,
    L2D_OP_FRAME_MATTE_HOLD = 57,
    L2D_OP_MASK_INGEST = 58,
    L2D_OP_MATTE_KEY = 59,
    L2D_OP_FRAME_PLANAR_BYTES = 60,
    L2D_OP_MATTE_KEY_ADAPT = 61,
    L2D_OP_MATTE_KEY_GAIN_HIST = 62,
    L2D_OP_MATTE_KEY_GAIN = 63,
    L2D_OP_SINK_COMMIT = 64,
    L2D_OP_FRAME_CUT_SIG = 65,
    L2D_OP_FRAME_CUT = 66,
};

/* flag bits of L2D_OP_FRAME_MATTE (i4) and L2D_OP_FRAME_MATTE_UP (i6); HARD and FAR also of L2D_OP_FRAME_MATTE_EDGE (i3) */
#define L2D_MATTE_HARD 1
#define L2D_MATTE_FAR 2
#define L2D_MATTE_SHOW 4
#define L2D_MATTE_PLANE 16 /* p2 is a float plane of ready matte values (8 is not assigned) */
#define L2D_MATTE_MAX_R 8
#define L2D_MATTE_EDGE_MAX_R 8 /* the largest radius of L2D_OP_FRAME_MATTE_EDGE */
#define L2D_MATTE_EDGE_PLANE 32 /* L2D_OP_FRAME_MATTE_EDGE: p1 is a float plane of ready matte values (what L2D_MATTE_PLANE is to
                                   L2D_OP_FRAME_MATTE; 4 and 16 are not assigned here and stay refused) */

/* sizes of L2D_OP_FRAME_BACKDROP_BLUR (its flags, i4, are L2D_MATTE_HARD | _FAR, or L2D_BACKDROP_PLANE) */
#define L2D_BACKDROP_PLANE 32 /* p1 is a float plane of ready matte values (as L2D_MATTE_EDGE_PLANE; 4 and 16 stay refused) */
#define L2D_BACKDROP_MAX_R 8
#define L2D_BACKDROP_MAX_PASSES 3

/* flag bits of L2D_OP_COLOR_LOCK (i2), and the sizes both colour-lock ops share */
#define L2D_COLOR_LOCK_INIT 1
#define L2D_COLOR_LOCK_SOURCE 2
#define L2D_COLOR_LOCK_FREEZE 4
#define L2D_COLOR_LOCK_BLOCK_PIXELS 4096 /* x 255^2 < 2^32: a block's sum of squares fits uint32 */
#define L2D_COLOR_LOCK_MAX_PIXELS 4194304 /* 2^22: n S2 - S1^2 stays inside int64 */

/* flag bits of L2D_OP_FRAME_STEADY (i3), and its largest radius */
#define L2D_STEADY_HARD 1
#define L2D_STEADY_SHOW 2
#define L2D_STEADY_INIT 4
#define L2D_STEADY_MAX_R 8

/* sizes of L2D_OP_FRAME_MOTION and L2D_OP_FRAME_STEADY_FOLLOW (the flags of the latter, i3, are L2D_STEADY_HARD | _SHOW) */
#define L2D_FOLLOW_BLOCK 8 /* one vector per 8 x 8 pixels */
#define L2D_FOLLOW_APRON 4 /* the matching window is the block and 4 pixels around it: 16 x 16 */
#define L2D_FOLLOW_MAX_SEARCH 8
#define L2D_FOLLOW_MAX_BIAS 4096

/* flag bits of L2D_OP_FRAME_MATTE_HOLD (i3); its radius is L2D_OP_FRAME_STEADY's, its field L2D_OP_FRAME_MOTION's */
#define L2D_MATTE_HOLD_HARD 1 /* the motion ramp is a step (L2D_STEADY_HARD) */
#define L2D_MATTE_HOLD_INIT 4 /* the first frame of a sequence (L2D_STEADY_INIT) */
#define L2D_MATTE_HOLD_PLANE 16 /* p1 is a float plane of ready matte values (L2D_MATTE_PLANE) */
#define L2D_MATTE_HOLD_FOLLOW 32 /* p6 is a field: the previous record is fetched along it */
#define L2D_MATTE_HOLD_RAMP_HARD 64 /* L2D_MATTE_HARD of the depth ramp */
#define L2D_MATTE_HOLD_RAMP_FAR 128 /* L2D_MATTE_FAR of the depth ramp */

/* flag bits of L2D_OP_FRAME_DETAIL_GAIN (i3: U8) and L2D_OP_FRAME_DETAIL (i4: SHOW) */
#define L2D_DETAIL_U8 1 /* p0 is the uint8 [H][W][3] frame of the matte, not the half frame */
#define L2D_DETAIL_SHOW 2

/* flag bits of L2D_OP_DEPTH_INGEST (i11: F32, DISTANCE, HAS_INVALID) and L2D_OP_DEPTH_NORMALIZE (i4: FIXED_RANGE), and their sizes */
#define L2D_DEPTH_F32 1 /* p0 holds fp32 samples, not uint16 */
#define L2D_DEPTH_DISTANCE 2 /* u = 1 / z (metric distance in), not z (inverse depth in) */
#define L2D_DEPTH_HAS_INVALID 4 /* samples equal to i12 (uint16) / f0 (fp32) are holes */
#define L2D_DEPTH_FIXED_RANGE 8 /* mn = f0, mx = f1 instead of the partials */
#define L2D_DEPTH_TILE_H 16 /* the output tile of one work-group: one {min, max, any} partial each */
#define L2D_DEPTH_TILE_W 32
#define L2D_DEPTH_MAX_TAPS 17 /* per axis, at a down-scale of 8 */

/* flag bits of L2D_OP_MASK_INGEST (i10); its tile and its taps are L2D_OP_DEPTH_INGEST's */
#define L2D_MASK_U16 1 /* p0 holds uint16 samples (neither U16 nor F32: uint8) */
#define L2D_MASK_F32 2 /* p0 holds fp32 samples */
#define L2D_MASK_INVERT 4 /* P = 255 - P */
#define L2D_MASK_AND 8 /* out = min(ramp, mask) (neither AND nor OR: the mask replaces the ramp) */
#define L2D_MASK_OR 16 /* out = max(ramp, mask) */
#define L2D_MASK_RAMP_HARD 64 /* L2D_MATTE_HARD of the depth ramp */
#define L2D_MASK_RAMP_FAR 128 /* L2D_MATTE_FAR of the depth ramp */

/* flag bits of L2D_OP_MATTE_KEY (i3), and its largest radius; its tile is L2D_OP_FRAME_MATTE_HOLD's */
#define L2D_MATTE_KEY_PLATE 1 /* the key is the plate p3, not the colour i5 i6 i7 */
#define L2D_MATTE_KEY_HARD 2 /* the key's ramp is a step */
#define L2D_MATTE_KEY_INVERT 4 /* P = 255 - P */
#define L2D_MATTE_KEY_AND 8 /* out = min(ramp, key) (neither AND nor OR: the key replaces the ramp) */
#define L2D_MATTE_KEY_OR 16 /* out = max(ramp, key) */
#define L2D_MATTE_KEY_RAMP_HARD 64 /* L2D_MATTE_HARD of the depth ramp */
#define L2D_MATTE_KEY_RAMP_FAR 128 /* L2D_MATTE_FAR of the depth ramp */
#define L2D_MATTE_KEY_MAX_R 4
/* L2D_OP_MATTE_KEY_ADAPT: its flags (i3) are L2D_OP_MATTE_KEY's and INIT; its largest rate */
#define L2D_MATTE_KEY_ADAPT_INIT 256 /* the state starts from the plate p3: s = 256 k, and p4 is not read */
#define L2D_MATTE_KEY_MAX_RATE 32768 /* 65536 times a rate of 1 / 2 */
/* the plate gain: a flag of L2D_OP_MATTE_KEY and L2D_OP_MATTE_KEY_ADAPT (i3), the flag of L2D_OP_MATTE_KEY_GAIN_HIST (i2), sizes */
#define L2D_MATTE_KEY_GAIN 512 /* the key is formed against the plate's bytes times the gains of the record p6 */
#define L2D_MATTE_KEY_GAIN_STATE 1 /* L2D_OP_MATTE_KEY_GAIN_HIST: p1 is the uint16 state, not the uint8 plate */
#define L2D_MATTE_KEY_GAIN_UNITY 128 /* a gain is an integer in units of 1 / 128 */
#define L2D_MATTE_KEY_GAIN_BINS 512 /* the ratios 0..511; 511 holds everything above */
#define L2D_MATTE_KEY_GAIN_BLOCK 4096 /* pixels per work-group of L2D_OP_MATTE_KEY_GAIN_HIST: 64 blocks at 512 x 512 */
/* cut detection: the flag of L2D_OP_FRAME_CUT_SIG (i2) and L2D_OP_FRAME_CUT (i3), sizes and ranges */
#define L2D_CUT_INIT 1 /* the first frame: no previous state is read */
#define L2D_CUT_BLOCK 8 /* a thumbnail entry is 8 x 8 pixels */
#define L2D_CUT_BINS 64 /* histogram bins of Y >> 2 */
#define L2D_CUT_TILE 64 /* pixels per side of a work-group's tile: 64 tiles at 512 x 512 */
#define L2D_CUT_PARTIAL 68 /* uint32 words of a partial: 64 counts, the share of Dt, three zeros */
#define L2D_CUT_MAX_PIXELS 4194304 /* H W at most: 2^22 */
#define L2D_CUT_NEVER 1073741824 /* `since` before the first cut, and where it saturates: 2^30 */
#define L2D_CUT_MIN_R 256
#define L2D_CUT_MAX_R 16384
#define L2D_CUT_MAX_GAP 255

/* sizes of L2D_OP_FRAME_RESIZE */
#define L2D_RESIZE_MAX_KS 13 /* taps per output: Lanczos (support 3) at a 2x down-scale, 2 * 6 + 1 */
#define L2D_RESIZE_MAX_SIZE 4096

typedef struct l2d_op {
    int32_t kind;
    int32_t tag;          /* free for the host (plan index / layer id); echoed in error messages */
    void *p[16];
    int32_t i[32];
    int64_t l[4];
    float f[4];
} l2d_op;

/* One record of L2D_OP_WEIGHT_BLEND's table: one tile of one tensor, 64 bytes.  src[k] for k >= K is ignored. */
#define L2D_WBLEND_MAX_SRC 4
#define L2D_WBLEND_TILE_BYTES 65536 /* a multiple of 16: every tile of an aligned tensor is aligned */
#define L2D_WBLEND_F16 0
#define L2D_WBLEND_F32 1
typedef struct l2d_wblend_rec {
    void *dst;
    const void *src[L2D_WBLEND_MAX_SRC];
    int64_t n;            /* elements of this tile: 1 .. L2D_WBLEND_TILE_BYTES / element size */
    int32_t dtype;        /* L2D_WBLEND_F16 | L2D_WBLEND_F32 */
    int32_t pad[3];
} l2d_wblend_rec;

/* One record of L2D_OP_SINK_COMMIT's table: the KV cache of one layer, 48 bytes. */
typedef struct l2d_sink_rec {
    void *dst;
    const void *src;
    int64_t lines;        /* N * 2 * h * w */
    int64_t line_bytes;   /* F * C * 2: what is copied of a line, a multiple of 16 */
    int64_t dst_pitch;    /* bytes from one destination line to the next: L * C * 2 */
    int64_t src_pitch;    /* ... of the source: >= line_bytes */
} l2d_sink_rec;

/* library / device ------------------------------------------------------------------------------ */
int l2d_abi_version(void);
const char *l2d_last_error(void);
/* 0 if the current HIP device is a gfx950 part; fills name (<= 63 chars) when non-NULL. */
int l2d_device_check(char *name, int name_len);

/* Validate-only mode: when on, l2d_run_ops checks every op's arguments exactly as a real launch would and
 * returns without touching the device (used by the CPU test-suite to check whole plans). */
int l2d_set_dry_run(int on);

/* execution ------------------------------------------------------------------------------------- */
/* Launch ops[0..n) in order on `stream`. */
int l2d_run_ops(const l2d_op *ops, int n, void *stream);
/* Capture ops[0..n) into a hipGraph on `stream` (stream capture) and instantiate it. */
int l2d_graph_create(const l2d_op *ops, int n, void *stream, void **graph_out);
int l2d_graph_launch(void *graph, void *stream);
int l2d_graph_destroy(void *graph);

/* timing helper for bench.py: hipEvent pair around `reps` runs of the ops on `stream`; returns ms. */
int l2d_time_ops(const l2d_op *ops, int n, void *stream, int reps, float *ms_out);

/* per-launch timing inside the op sequence (an event in front of every op, `reps` passes): us_out[n] = mean microseconds
 * from op i's start marker to op i+1's (launch + the gap behind it).  For tools (schedule tuning, in-frame breakdowns). */
int l2d_time_each(const l2d_op *ops, int n, void *stream, int reps, float *us_out);

/* HBM copy microbenchmark (device-to-device float4 copy kernel), used to state the measured HBM peak
 * next to the datasheet number: copies `bytes` from src to dst `reps` times, returns GB/s (read+write). */
int l2d_copy_bench(const void *src, void *dst, int64_t bytes, int reps, void *stream, float *gbps_out);

/* HBM read probe: streaming 16-byte loads, `unroll` (1,2,4,8,16) independent loads in flight per thread,
 * 256 x blocks_per_cu blocks of 256 threads; returns GB/s read. */
int l2d_read_bench(const void *src, void *sink, int64_t bytes, int unroll, int blocks_per_cu, int reps, void *stream,
                   float *gbps_out);

/* The host part of the JPEG decoder (plain C++, no device work): the entry point of every chunk of a baseline scan.
 * file / len: the whole file (HOST memory); blob: jpeg.table_blob (host); layout int32 [12] = {byte offset of the scan, n_mcu, ny,
 * restart interval, chunk_mcus, DC table id x 3, AC table id x 3, C}; out: bit_offsets int32 [C + 1] (bit offsets into the stuffed
 * scan; the last is the EOI marker's) and dc_pred int16 [C][3].  Where every chunk is a whole restart interval the entries come
 * from a byte search for the markers; otherwise from one walk over the Huffman symbols (code lengths and DC values only), which
 * also validates the scan end to end.  Returns 0, or: -1 arguments, -2 invalid code, -3 coefficient index past 63, -4 the bits run
 * out, -5 markers or MCU count do not match the frame.  Never reads outside [file, file + len). */
int l2d_jpeg_index(const uint8_t *file, int64_t len, const uint8_t *blob, const int32_t *layout, int32_t *bit_offsets, int16_t *dc_pred);
/* The lanes of L2D_OP_JPEG_ENTROPY_DEC run one after the other on the HOST: `op` is the record the kernel would be launched with,
 * every pointer in it a host pointer.  The kernel's lane body is a host-and-device function, so this is the same code: the model
 * the CPU test-suite checks the kernel's loop bounds, its writes and its status word with, on machines without a device. */
int l2d_jpeg_entropy_model(const l2d_op *op);

#ifdef __cplusplus
}
#endif
#endif /* L2D_H */
