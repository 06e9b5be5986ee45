/*
 * srx.h -- C ABI of the MI355X (gfx950) SRGAN/ESRGAN hot-path library `libsrx_hip.so`.
 *
 * This is the drop-in boundary (level 2).  The reference
 * (roclark/torchsr) has no FFI of its own: every FLOP of its hot path is issued
 * through `torch.nn` modules.  Each entry point below therefore cites the
 * reference construct (file:line under /root/reference) whose device work it
 * replaces.  The Python host (`torchsr_amd/`) binds these with ctypes and wraps
 * them in `torch.autograd.Function`s behind the reference's own
 * `Generator` / `Discriminator` / `VGGLoss` / trainer surface.
 *
 * Conventions
 *  - plain pointers and sizes only; no torch / HIP types in signatures
 *    (`stream` is a `hipStream_t` passed as `void*`; NULL = default stream).
 *  - all tensors are fp32, activations are NHWC ([N][H][W][C_s]) with a channel
 *    stride C_s that is a multiple of 4 (3-channel images are stored with C_s=4,
 *    4th channel zero).  Parameters stay in the reference's own layouts
 *    (Conv2d OIHW, Linear [out][in]) so `state_dict()` is byte compatible;
 *    MFMA-friendly packed copies are produced by `srx_conv2d_pack`.
 *  - every call is asynchronous on `stream`, allocates nothing, never
 *    synchronises and is hipGraph-capture safe.  Scratch memory is handed in by
 *    the caller (`*_ws_floats` queries say how much).
 *  - return value: 0 = ok, otherwise an SRX_E_* code; a thread-local message is
 *    available through `srx_last_error`.
 *  - re-entrant: no mutable global state except kernel attributes set once.
 */
#ifndef SRX_H
#define SRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRX_VERSION 100 /* 0.1.0, mirrors torchsr/__version__.py:13 */

enum {
  SRX_OK = 0,
  SRX_E_BADARG = 1,      /* shape / alignment / null pointer problem */
  SRX_E_UNSUPPORTED = 2, /* configuration outside what the kernels implement */
  SRX_E_HIP = 3,         /* a HIP runtime call failed */
  SRX_E_WORKSPACE = 4    /* workspace too small */
};

enum { SRX_ACT_NONE = 0, SRX_ACT_RELU = 1, SRX_ACT_LRELU = 2, SRX_ACT_PRELU = 3 };

int srx_version(void);
/* copies the calling thread's last error message (NUL terminated) into buf */
int srx_last_error(char* buf, size_t n);
/* sha256 (64 hex digits) of the sources this binary was compiled from -- the build's identity: the host refuses (or
 * rebuilds) a library whose digest differs from the sources lying next to it (torchsr_amd/_lib.py).  No reference counterpart. */
int srx_build_info(char* buf, size_t n);
/* number of compute units of the current device (used by the host for launch heuristics) */
int srx_device_cus(void);
/* Compute units the launch plans may count on = srx_device_cus() less `k` reserved ones (0..128).  Data-parallel training
 * overlaps the gradient all-reduce (torchsr/srgan/trainer.py:142-157: DistributedDataParallel) with the backward pass, and
 * RCCL's channel workgroups then hold CUs: a grid cut for exactly 256 CUs runs two rounds on 248.  May be set and reset at
 * any time between calls (ddp.GradBuckets does so inside every step, around its communication windows); also
 * SRX_RESERVED_CUS at load time.  Every plan-dependent size -- the *_ws_floats queries, the row counts of BatchNorm partial
 * tables (srx_conv2d_stat_rows, srx_conv2d_bwd_data_bn_rows, srx_wino_stat_rows), srx_conv2d_plan / srx_wino_plan /
 * srx_conv3x3_c64_bf16_plan -- follows the count of the moment, and a launch plans with the count at ITS call (the packed
 * weight sizes and layouts depend on the layer alone).  What callers must keep: query the sizes a launch needs in the same
 * call sequence as that launch, with no srx_set_reserved_cus in between, as functional.py does (it asks right before each
 * launch and keeps no size across calls); a size queried under another reservation may be too small for the launch or
 * describe a table of other rows.  A replayed hipGraph keeps the plans it was captured with.  srx_plan_cus() returns the
 * count the plans use. */
int srx_set_reserved_cus(int k);
int srx_plan_cus(void);
/* Measurement aid (bench.py's data-parallel rehearsal; no reference counterpart): occupies `k` compute units -- k workgroups that each
 * claim a whole CU's LDS, so nothing else becomes resident there (`whole_cu` != 0), or k co-resident workgroups that only
 * spin (`whole_cu` == 0) -- until *stop_flag (host-visible, 4 bytes) is non-zero or `max_ms` milliseconds have passed on
 * the device clock, whichever comes first; every wave reaches that exit. */
int srx_occupy_cus(int k, int whole_cu, const int* stop_flag, int max_ms, void* stream);
/* Per-launch timing of the convolution kernels (measurement aid for bench.py's roofline leg; no
 * reference counterpart).  Between start and stop every conv kernel is dispatched with its own start /
 * stop HIP events on its stream (hipExtLaunchKernelGGL) -- the main kernel only, not its fix-up / reduce
 * companion.  Not to be used inside a hipGraph capture.  srx_prof_stop returns the number of records; srx_prof_get
 * (after stop) synchronises on record i and returns its kernel name, duration and FLOPs.
 * srx_prof_start_aux: the same, and the slab reductions behind the weight-gradient kernels (wgrad_reduce_rows_kernel,
 * wgrad_reduce_kernel) get records of their own, 0 FLOPs each: what a test needs that accounts for every launch of a step. */
int srx_prof_start(int max_launches);
int srx_prof_start_aux(int max_launches);
int srx_prof_stop(void);
int srx_prof_get(int i, char* name, size_t n, float* ms, double* flops);

/* ------------------------------------------------------------------ layout */
/* NCHW [N][C][H][W] -> NHWC [N][H][W][Cs] (channels C..Cs-1 written as 0).
 * Replaces the implicit NCHW contract of every reference module's forward
 * (srgan/generator.py:60, srgan/discriminator.py:71, srgan/loss.py:36). */
int srx_nchw_to_nhwc(const float* src, float* dst, int N, int C, int H, int W, int Cs, void* stream);
/* NHWC [N][H][W][Cs] -> NCHW [N][C][H][W]; also `torch.flatten(out, 1)` in NCHW
 * order for the discriminator head (srgan/discriminator.py:86). */
int srx_nhwc_to_nchw(const float* src, float* dst, int N, int C, int H, int W, int Cs, void* stream);
/* One of the eight flips / transposes of an image (the dihedral group), with scaling and accumulation -- the geometry of
 * the self-ensemble of test.upscale(self_ensemble=n), `torchsr test --self-ensemble`; no reference counterpart
 * (torchsr/test.py:57-62 runs the generator once).  src: [planes][H][W] (NCHW with planes = N * C); k in 0..7 -- bit 0
 * transpose, bit 1 horizontal flip, bit 2 vertical flip, the transpose first: source element (y, x) goes to (u, v) = (x, y)
 * in a dst of [planes][H' = W][W' = H] with bit 0, else (y, x) in [planes][H' = H][W' = W]; then v = W' - 1 - v with
 * bit 1 and u = H' - 1 - u with bit 2;
 *   dst[p][u][v] = alpha * src[p][y][x] + beta * dst[p][u][v]   (one fma; beta == 0: dst is not read).
 * The inverse of k is k itself without bit 0 and k with bits 1 and 2 swapped with it.  src and dst must not overlap;
 * alpha, beta finite.  Any H, W, 64-bit offsets throughout (planes * H * W may pass 2^31). */
int srx_dihedral_planes(const float* src, float* dst, int64_t planes, int H, int W, int k, float alpha, float beta,
                        void* stream);
/* Separable resize of fp32 planes with the weight tables as operands -- the `outscale` of test.upscale, `torchsr test
 * --outscale` (functional.resize_bicubic_aa; the tables of functional.resample_tables make it the antialiased Keys bicubic
 * the training data is reduced with); no reference counterpart (torchsr/test.py:57-62 writes the x4 result).
 * src: [planes][H][W] -> dst: [planes][OH][OW], any mix of reduction and enlargement per axis.  Per axis (y: n_in = H,
 * n_out = OH; x: n_in = W, n_out = OW) start[n_out] (int32) and weight[n_out][K] (fp32, rows padded with 0), all in device memory:
 *   tmp[p][oy][x]  = sum_t weight_y[oy][t] * src[p][min(start_y[oy] + t, H - 1)][x]     t = 0 .. Ky - 1
 *   dst[p][oy][ox] = sum_t weight_x[ox][t] * tmp[p][oy][min(start_x[ox] + t, W - 1)]    t = 0 .. Kx - 1
 * in fp32, fmas in ascending t from 0 (two launches, no atomics: the same bits from every call, a plane's bits whatever
 * the other planes are).  Every start is clamped to [0, n_in - 1]: no table content reads outside src.
 * ws: the workspace tmp, ws_floats >= planes * OH * W.  1 <= Ky, Kx <= 66 (a 16:1 reduction); H * W, OH * OW and OH * W
 * < 2^31, 64-bit plane bases (planes * H * W may pass 2^31); src, dst and ws 4-byte aligned (16-byte accesses when W % 4 == 0
 * and src and ws are 16-byte aligned) and disjoint. */
int srx_resample_planes(const float* src, float* dst, int64_t planes, int H, int W, int OH, int OW, const int* start_y,
                        const float* weight_y, int Ky, const int* start_x, const float* weight_x, int Kx, float* ws,
                        size_t ws_floats, void* stream);
/* Colour fix of a super-resolved frame against its input -- the `color_fix` of test.upscale, `torchsr test --color-fix`
 * (functional.color_fix_wavelet / color_fix_adain; csrc/colorfix.hip); no reference counterpart.  All tensors are
 * [planes][H][W] fp32, every plane alone; H * W < 2^31, planes < 2^28, 64-bit plane bases, any H, W >= 1.
 *
 * One level of the a-trous blur with [1 2 1]^T [1 2 1] / 16 at dilation `radius` (1..32768), replicate padding, cl = clamp to
 * the plane:
 *   D         = sub ? src - sub : src                                               (one rounding)
 *   t[y][x]   = 0.25f * (D[y][cl(x - radius)] + D[y][cl(x + radius)]) + 0.5f * D[y][x]
 *   v[y][x]   = 0.25f * (t[cl(y - radius)][x] + t[cl(y + radius)][x]) + 0.5f * t[y][x]
 *   dst       = add ? add + v : v                                                   (one rounding)
 * in one launch, with the intermediate values of separate passes (two roundings per pass): the same bits from every call and
 * alignment.  sub and add may be null; dst must overlap no operand.  The wavelet colour fix with `levels` levels is level 0 with
 * src = the enlarged input and sub = sr, the levels between from one workspace to another, the last with add = sr:
 * out = sr + B(U - sr).  4-byte aligned pointers; 16-byte accesses when W % 4 == 0, every pointer given is 16-byte aligned and
 * radius is 1, 2 or a multiple of 4. */
int srx_color_fix_wavelet_level(const float* src, const float* sub, const float* add, float* dst, int64_t planes, int H, int W,
                                int radius, void* stream);
/* Mean and unbiased variance (0 for H * W == 1) of every plane in fp64: stats[planes][2] = {mean, variance}.  Sums of
 * d = x - x[p][0] and of d * d per workgroup into fixed slots of part ([planes][B][2] doubles, B = srx_plane_moments_blocks(H, W),
 * part_doubles >= planes * B * 2), then added in index order by one wave per plane -- two launches, no atomics; an element's
 * place in the sum depends on H * W alone: the same bits from every call, batch and alignment.  x, part and stats disjoint. */
int srx_plane_moments_blocks(int H, int W); /* 0 for sizes srx_plane_moments refuses */
int srx_plane_moments(const float* x, int64_t planes, int H, int W, double* part, size_t part_doubles, double* stats, void* stream);
/* AdaIN colour fix: dst = fmaf(sr, s, b) per plane with s = sqrt(var_lr + 1e-5) / sqrt(var_sr + 1e-5) and b = mean_lr - mean_sr * s
 * formed in fp64 from the two srx_plane_moments results (the input's at its own size) and rounded once to fp32.  dst must overlap
 * no operand. */
int srx_color_fix_adain_apply(const float* sr, float* dst, int64_t planes, int H, int W, const double* stats_sr,
                              const double* stats_lr, void* stream);

/* ------------------------------------------------------------------ conv2d */
/* One nn.Conv2d instance: srgan/residual.py:27,64,67; srgan/generator.py:38,48,58;
 * srgan/discriminator.py:32-59; torchvision VGG19 cfg 'E' (srgan/loss.py:30-31);
 * esrgan/residual.py:31-56; esrgan/generator.py:36-52. */
typedef struct srx_conv2d {
  int32_t N, H, W;    /* input batch / spatial size */
  int32_t Cin;        /* Conv2d.in_channels  */
  int32_t Cin_s;      /* channel stride of the input tensor  (>= Cin, multiple of 4) */
  int32_t Cout;       /* Conv2d.out_channels */
  int32_t Cout_s;     /* channel stride of the output tensor (>= Cout, multiple of 4);
                         with shuffle=2 this is the stride of the shuffled tensor (>= Cout/4) */
  int32_t KH, KW, stride, pad;
  int32_t shuffle;    /* 0, or 2: nn.PixelShuffle(2) fused into the store
                         (srgan/residual.py:28): output is [N][2Ho][2Wo][Cout/4] */
  int32_t act;        /* fused epilogue: SRX_ACT_NONE / RELU / LRELU (after bias) */
  float   slope;      /* LeakyReLU negative_slope */
  int32_t up;         /* 0/1, or 2: F.interpolate(scale_factor=2, mode='nearest') of the
                         input fused into the gather (esrgan/generator.py:73,76): the forward reads
                         pixel (h >> 1, w >> 1), the upsampled tensor is never written; H,W are then
                         the size of the tensor BEFORE upsampling (stride 1, no shuffle).  The data
                         gradient is taken at the upsampled size in scratch and summed per 2x2 block,
                         the weight gradient reads a scratch copy (both from `ws`) */
  int32_t precision;  /* 0: exact fp32 MFMAs.  1: bf16 products with fp32 accumulation for the forward
                         and the stride-1 data gradient -- the reference's torch.cuda.amp.autocast
                         region (srgan/trainer.py:379-383, esrgan/trainer.py:418-484); tensors stay
                         fp32 in memory, operands are rounded when staged into LDS; strided data
                         gradients and the 3-channel (thin) layers remain fp32.  2: only on the forward
                         of a 64 -> <= 4 channel layer (the generators' output conv): bf16 products there
                         as well -- inference with every conv in bf16 (test.upscale(precision='bf16')).
                         3: fp16 inference (test.upscale(precision='fp16')), forward only and only for a
                         <= 4-channel INPUT layer (Cin_s = 4, no shuffle / up): fp16 products with fp32
                         accumulation, tensors fp32 in memory (operands rounded to nearest even when
                         staged into LDS, like 1); the generator's 64-channel layers run on the _f16
                         entry points below.  The host refuses 3 with autograd enabled or outside eval
                         mode, the library on every backward entry point */
} srx_conv2d_t;

/* sizes (in floats) of the packed weight copies and of scratch buffers */
size_t srx_conv2d_packed_fwd_floats(const srx_conv2d_t* d);
size_t srx_conv2d_packed_bwd_floats(const srx_conv2d_t* d);
size_t srx_conv2d_fwd_ws_floats(const srx_conv2d_t* d);
size_t srx_conv2d_bwd_data_ws_floats(const srx_conv2d_t* d);
size_t srx_conv2d_bwd_weight_ws_floats(const srx_conv2d_t* d);
/* rows of the per-channel (sum, sum of squares) partial table written by
 * srx_conv2d_fwd when `bn_partials` is non-NULL: table is [rows][Cout][2] */
int srx_conv2d_stat_rows(const srx_conv2d_t* d);

/* launch plan the library will use (for profiling / the bench's roofline bookkeeping):
 * which = 0 forward, 1 data gradient; out[6] = {tile rows BM, tile cols BN, tail split-K factor, workgroups,
 * KS (wave groups splitting K inside a workgroup), multi (1: stride-parity classes in one launch; 2: in one workgroup per tile, gconv_s2f_kernel)}.
 * BM = 144 is the 128 + 16 row tile, BM = 36 the row-tile kernel of rowtile.hip. */
int srx_conv2d_plan(const srx_conv2d_t* d, int which, int* out);

/* Plan overrides for tests and tile experiments (no reference counterpart).  They hold for every later call of this process until
 * reset with zeros (srx_wgrad_force: (-1, 0), srx_wgrad_force_kernels: (-1, -1, -1)); the environment seeds them at load
 * (SRX_FORCE_PLAN="BM,BN,split,ks", SRX_S2_MODE bit 0, SRX_NO_WGRAD_LIN, SRX_WGRAD_NSPLIT, SRX_WGRAD_ROWS_NSPLIT, SRX_NO_WGRAD_DMA,
 * SRX_NO_WGRAD_ROWS, SRX_OLD_WGRAD_REDUCE, SRX_THIN_FWD_ROWS; srx_linear_force has no environment seed).  srx_conv2d_plan, srx_thin_plan,
 * srx_linear_plan, srx_wgrad_plan and the workspace queries report what a forced call runs.  A forced form a
 * layer has no kernel for (tile not instantiated at the layer's arithmetic, BN not dividing the padded columns, 144 rows with bf16
 * products, the fused kernel on a layer it cannot run, more row splits than the rows allow, 4 rows per wave on a 3-channel output
 * layer with bf16 products, the fast linear form on a launch that cannot take it, more linear splits than there are trips) is
 * refused with SRX_E_UNSUPPORTED and a message when that layer is planned or called, before anything is launched.
 * srx_conv2d_force_plan: every gconv_kernel / gconv_multi_kernel plan (not the whole-frame calls above 2^24 pixels) is BM x BN
 *   (BM = 144: the 128 + 16 row tile), every tile K-split `split` ways where the output is linear (strided / shuffled outputs run
 *   unsplit), KS = 2: two wave groups on the 64 x 64 tile (64 x 32 always has 2, or 4 with bf16 products).
 * srx_conv2d_force_s2: strided data gradients -- mode 0 the cost model, 1 always gconv_multi_kernel (tile from the model or
 *   srx_conv2d_force_plan), 2 always gconv_s2f_kernel on tile BM x BN ((2, 0, 0): the model's fused tile).
 * srx_wgrad_force: weight gradients -- lin 0: never the LIN form of wgrad_dma_kernel (fp32), 1 / -1: wherever it is eligible (the
 *   default); nsplit > 0: that many row splits, 0: the model's.  The generic kernels (wgrad_kernel, wgrad_dma_kernel) split the
 *   M = N Ho Wo output pixels into whole 32-row chunks of at least 128 rows; the image-row kernel (wgrad_rows_bf16_kernel) splits
 *   the N H image rows into whole rows: v is taken iff v <= N H and cdiv(N H, cdiv(N H, v)) == v.  SRX_WGRAD_NSPLIT seeds the
 *   former, SRX_WGRAD_ROWS_NSPLIT the latter; this call sets both.
 * srx_wgrad_force_kernels: which weight-gradient kernels run, each argument -1 (default) / 0 (off) / 1 (on where eligible, which is
 *   the default) -- dma 0: fp32 layers run wgrad_kernel<0> (register-staged) instead of wgrad_dma_kernel; rows 0: the layers of
 *   the image-row bf16 kernel run wgrad_kernel<1>; reduce 0: wgrad_reduce_kernel sums every layer's slabs (otherwise only K > 12288).
 * srx_thin_force_rows: the 3-channel output kernel (forward of the 64 -> <= 4 channel layers, data gradient of the <= 4 -> 64
 *   ones) -- 3, 4 or 6 output rows per wave, i.e. tiles of 12, 16 or 24 rows x 32 pixels; 0: the model's (6 from four tiles of
 *   24 rows per plan CU on, else 3).  Any other value is refused (SRX_THIN_FWD_ROWS: ignored with a line on stderr); the
 *   kernel with bf16 products (precision = 2) exists with 3 and 6 rows.
 * srx_linear_force: nn.Linear (linear.hip) -- form 0 the model's choice, 1 always the plain kernels (linear_*_kernel), 2 the fast
 *   kernels (linear_*_fast_kernel) wherever they may run: K a multiple of 64, J a multiple of 16 for the two gradients, at most
 *   32 rows in a 64-row launch of the forward / data gradient; a launch that cannot is refused, never downgraded.  splits > 0:
 *   that many K splits of the forward / J splits of the data gradient before the rounding to whole trips of 256 / 16 (more than
 *   cdiv(K, 256) / cdiv(J, 16) is refused by that pass), 0: the model's.  Reset with (0, 0). */
int srx_conv2d_force_plan(int bm, int bn, int split, int ks);
int srx_conv2d_force_s2(int mode, int bm, int bn);
int srx_wgrad_force(int lin, int nsplit);
int srx_wgrad_force_kernels(int dma, int rows, int reduce);
int srx_thin_force_rows(int rows);
int srx_linear_force(int form, int splits);

/* Launch plan of the kernels with a <= 4-channel side (thin.hip), computed by the function the launches themselves plan with;
 * host code only.  which = 0 forward of a 64 -> <= 4 channel layer, 1 data gradient of a <= 4 -> 64 channel layer (both
 * thin_fwd2_kernel / thin_fwd2_bf16_kernel): out[4] = {rows per wave R, row tiles of 4 R rows, column tiles of 32 pixels,
 * workgroups}.  2 weight gradient of either (thin_wgrad_kernel): out[5] = {groups of kernel rows, segments of 16 pixels of one
 * image row, segments per wave range, ranges that hold a segment, workgroups per group = slabs the reduction sums}; the launch
 * has groups x slabs workgroups of four wave ranges, the ranges past the fourth entry are empty.  3 forward of a 3x3 <= 4 -> 64
 * channel layer (first3x3_fwd_kernel): out[2] = {tiles of 32 pixels, workgroups}; a wave walks tile = 4 workgroup + wave, += 4
 * workgroups.  SRX_E_UNSUPPORTED when the layer does not take that path, or is forced to a form it has no kernel for. */
int srx_thin_plan(const srx_conv2d_t* d, int which, int* out);

/* RRDBNet's x2 input layer (unshuffle.hip): y = conv3x3_pad1(pixel_unshuffle(pad(x), 2), w) + bias in one launch, nothing in
 * between written.  x: the NHWC-4 image [N][H][W][4] (channel 3 is not read); an odd H / W is padded by one reflected row /
 * column at the bottom / right inside the gather (RealESRGANer.pre_process): Hp = H + (H & 1), Wp = W + (W & 1); y: fp32
 * [N][Hp / 2][Wp / 2][64]; bias [64] or NULL; no activation.  The layer is the 6x6 / stride 2 / pad 2 conv over the image with
 * v[o][c][2 ky + dy][2 kx + dx] = w[o][4 c + 2 dy + dx][ky][kx].
 *   pack: w OIHW fp32 [64][12][3][3] -> wpk, srx_unshuffle2_conv_packed_floats() = 108 x 64 floats ([k = (tap, channel)][64]).
 *   fwd:  precision 0: exact fp32 MFMAs; 1: operands rounded to bf16, fp32 products and sums.  Recorded for srx_prof_get as
 *         "unshuffle2_conv_fwd_kernel<precision> MxNxK=<N Hp/2 Wp/2>x64x108".
 *   plan: host only, by the function the launch plans with (under srx_set_reserved_cus): out[2] = {tiles of 32 output pixels,
 *         workgroups}; a wave walks tile = 4 workgroup + wave, += 4 workgroups.
 * Refused with SRX_E_BADARG, nothing launched: a null x / wpk / y, N, H or W < 1, an odd H or W below 3 (no row to reflect),
 * N Hp Wp >= 2^24 pixels, a precision other than 0 / 1. */
size_t srx_unshuffle2_conv_packed_floats(void);
int srx_unshuffle2_conv_pack(const float* w_oihw, float* wpk, void* stream);
int srx_unshuffle2_conv_fwd(int N, int H, int W, const float* x, const float* wpk, const float* bias, float* y, int precision,
                            void* stream);
int srx_unshuffle2_conv_plan(int N, int H, int W, int* out);

/* Weight gradient of that layer (unshuffle.hip; training RRDBNet at x2).  x: the image the forward read, dy: fp32
 * [N][Hp / 2][Wp / 2][64], dw_oihw: the module's [64][12][3][3]; accumulate != 0 adds to it.  dV[o][c][ty][tx] = sum over
 * (n, Y, X) of dy[n][Y][X][o] * x[n][r(2 Y - 2 + ty)][q(2 X - 2 + tx)][c] with the forward's gather (zero outside [0, Hp),
 * index H -> H - 2; columns alike) and dw[o][4 c + 2 (ty & 1) + (tx & 1)][ty >> 1][tx >> 1] = dV[o][c][ty][tx].  Exact fp32
 * MFMAs whatever the layer's precision.  There is no data gradient: the input is the image.  The bias gradient is the column
 * sum of dy (srx_colsum).
 *   ws_floats: the workspace the call needs for this shape (slabs x 4 x 36 x 64), 0 for a shape the call refuses.
 *   plan: host only, by the function the launch plans with (under srx_set_reserved_cus): out[5] = {segments of 16 output pixels
 *         of one output row, wave ranges that hold a segment, segments per range, slabs the reduction sums = workgroups per group,
 *         groups of tap rows}; the launch has groups x slabs workgroups of four wave ranges, ranges past the second entry are
 *         empty.
 * Refused, nothing launched: SRX_E_BADARG for a null x / dy / dw / ws and for the shapes the forward refuses; SRX_E_WORKSPACE for
 * ws_floats below srx_unshuffle2_conv_wgrad_ws_floats(N, H, W). */
size_t srx_unshuffle2_conv_wgrad_ws_floats(int N, int H, int W);
int srx_unshuffle2_conv_wgrad_plan(int N, int H, int W, int* out);
int srx_unshuffle2_conv_bwd_weight(int N, int H, int W, const float* x, const float* dy, float* dw_oihw, int accumulate, float* ws,
                                   size_t ws_floats, void* stream);

/* Launch plan of nn.Linear (linear.hip), computed by the function the launches themselves plan with; host code only.  which = 0
 * forward, 1 data gradient: out[6] = {splits launched (slabs of partial sums), contraction elements per split (k / j), launches
 * of up to 64 rows, 16-row blocks NB of the last launch, form of the first launch (1 plain, 2 fast), form of the last launch}.
 * which = 2 weight gradient: out[6] = {1, 0, 1, batch trips of 32 rows, form, form}.  SRX_E_UNSUPPORTED for what srx_linear_force
 * asked for and the shape cannot run. */
int srx_linear_plan(int B, int K, int J, int which, int* out);

/* Launch plan of srx_conv2d_bwd_weight* (wgrad.hip) for `nprob` problems of this geometry, `per_out` of them summed into one
 * output, under the current overrides and reservation; computed by the function the launch and the workspace query plan with;
 * host code only.  out[6] = {slab kernel: 0 wgrad_kernel<0>, 1 wgrad_dma_kernel<0, 0>, 2 wgrad_dma_kernel<1, 0> (WIDE),
 * 3 wgrad_dma_kernel<1, 1> (WIDE + LIN), 4 wgrad_kernel<1>, 5 wgrad_rows_bf16_kernel<32>, 6 wgrad_rows_bf16_kernel<16>, 7 the
 * 3-channel path of thin.hip (the other entries are 0: srx_thin_plan(d, 2, .) has its plan); row splits; output pixels per
 * split; reduce kernel: 0 wgrad_reduce_kernel, 1 wgrad_reduce_rows_kernel; workgroups of the slab kernel; slabs summed into one
 * output (splits x per_out)}.  The workspace is Cnw (Kw + 1) x splits x nprob floats, Cnw / Kw = Cout / K in whole tiles of 64.
 * up = 2: the plan of the upsampled descriptor.  SRX_E_UNSUPPORTED for a forced row split the rows cannot take. */
int srx_wgrad_plan(const srx_conv2d_t* d, int nprob, int per_out, int* out);

/* OIHW master weights -> packed forward ([Cout_p][K_p], K=(kh,kw,ci)) and, when
 * wpk_bwd != NULL, packed data-gradient operands (per stride-parity class,
 * taps flipped, [Cin_p][K'_p], K'=(tap,co)). */
int srx_conv2d_pack(const srx_conv2d_t* d, const float* w_oihw, float* wpk_fwd, float* wpk_bwd, void* stream);

/* The same for every conv of a model in ONE launch (after an optimiser step): build fills a host buffer of
 * srx_pack_table_bytes(n) bytes with one record per packed operand; the caller keeps a copy of it in
 * device memory (all pointers and sizes in it are fixed) and replays it with srx_pack_table_run.
 * wpk_bwd[i] may be NULL (layer whose input needs no gradient). */
size_t srx_pack_table_bytes(int n_layers);
int srx_pack_table_build(const srx_conv2d_t* descs, int n, const float* const* w_oihw, float* const* wpk_fwd,
                         float* const* wpk_bwd, void* host_table, int* n_records, long long* max_elems);
int srx_pack_table_run(const void* dev_table, int n_records, long long max_elems, void* stream);
/* appends to a host table under construction (srx_pack_table_build's output; room: srx_pack_table_bytes) the record that refreshes a
 * layer's Winograd-domain weights (srx_wino_pack(d, w, upk, transpose)) in the same launch */
int srx_pack_table_add_wino(void* host_table, int* nrec, long long* max_elems, const srx_conv2d_t* d, const float* w, float* upk,
                            int transpose);

/* y = act(conv(x, W) + bias).  bias may be NULL.  bn_partials may be NULL; when
 * given it receives per-row-block sums for the training-mode BatchNorm that
 * follows (srgan/residual.py:65,68; srgan/discriminator.py:36-60). */
int srx_conv2d_fwd(const srx_conv2d_t* d, const float* x, const float* wpk_fwd, const float* bias,
                   float* y, float* bn_partials, float* ws, size_t ws_floats, void* stream);
/* ---------------------------------------------------------------- bf16-native inference chain (round 4) */
/* `torchsr test` (torchsr/test.py:57-62) with --precision bf16: from the first conv's output to the last conv's input the
 * generator's activations are STORED as bf16 NHWC (128 bytes per 64-channel pixel).  Entry points take `void*` bf16 tensors.
 *
 * srx_conv3x3_c64_bf16_*: nn.Conv2d(64, Cout, 3, 1, 1) with Cout a multiple of 64 -- the residual blocks' convs with the
 * eval-mode BatchNorm folded in (srgan/residual.py:64-68,86-91), the generator's conv2 (srgan/generator.py:48,76-78) and
 * the sub-pixel layers (srgan/residual.py:27-29, Cout = 256 with PixelShuffle(2) in the store).
 *   pack: w OIHW fp32 [Cout][64][3][3], bias [Cout] or NULL, out_scale [Cout] or NULL (multiplies the weights of each
 *         output channel: the folded BatchNorm's gamma / sqrt(var + eps)); wpk: srx_conv3x3_c64_bf16_packed_bytes(Cout) bytes.
 *   fwd:  y = act(conv(x) + bias) [+ residual], act(v) = v > 0 ? v : v * slope (none: slope = 1, PReLU: its parameter);
 *         x: bf16 [N][H][W][64]; y: bf16 [N][H][W][y_cs] (shuffle = 2: [N][2H][2W][y_cs], channels 0..63), y_cs a multiple of
 *         8; residual: bf16 laid out like y, a tensor of its own, not with shuffle.  Any H, W; tensors above 4 GiB are fine
 *         (64-bit row bases). */
size_t srx_conv3x3_c64_bf16_packed_bytes(int Cout);
int srx_conv3x3_c64_bf16_pack(const float* w, const float* bias, const float* out_scale, int Cout, int shuffle, void* wpk,
                              void* stream);
int srx_conv3x3_c64_bf16_fwd(int N, int H, int W, int Cout, int shuffle, const void* x, const void* wpk, float slope,
                             const void* residual, void* y, int y_cs, void* stream);
/* host only: out[3] = {rows per chunk, chunks per column strip, column strips} of the launch _fwd makes at this size.  A chunk is
 * addressed with 32-bit byte offsets from its first row, so rows per chunk x W x 128 bytes stays below 4 GiB (shorter chunks) */
int srx_conv3x3_c64_bf16_plan(int N, int H, int W, int Cout, int* out);
/* fp32 <-> bf16 (round to nearest even), n elements, a multiple of 4: the two ends of the chain */
int srx_f32_to_bf16(const float* x, void* y, int64_t n, void* stream);
int srx_bf16_to_f32(const void* x, float* y, int64_t n, void* stream);
/* The generator's output conv (nn.Conv2d(64, 3, 9, 1, 4), srgan/generator.py:58,80) reading a bf16 input: d->precision
 * must be 2 (bf16 products in the 64 -> 3 layer); y is fp32 [N][H][W][4]. */
int srx_conv2d_fwd_bf16in(const srx_conv2d_t* d, const void* x_bf16, const float* wpk_fwd, const float* bias, float* y,
                          void* stream);

/* The same conv (nn.Conv2d(64, Cout <= 3, 9, 1, 4), srgan/generator.py:58,80) as a GEMM whose N is supplied by the taps -- 9
 * row taps x 3 channels = 27 MFMA rows, K = 9 column taps x 64 channels -- on v_mfma_f32_32x32x16_bf16 (thin9.hip): x bf16
 * [N][H][W][64], y fp32 [N][H][W][4] (channels >= Cout written as 0), bf16 products, fp32 accumulation; any H, W.
 * pack: w OIHW fp32 [Cout][64][9][9], bias [Cout] or NULL -> srx_conv9x9_c64_thin_bf16_packed_bytes() bytes. */
size_t srx_conv9x9_c64_thin_bf16_packed_bytes(void);
int srx_conv9x9_c64_thin_bf16_pack(const float* w, const float* bias, int Cout, void* wpk, void* stream);
int srx_conv9x9_c64_thin_bf16_fwd(int N, int H, int W, const void* x, const void* wpk, float* y, void* stream);

/* ---------------------------------------------------------------- fp16-native inference chain */
/* `torchsr test --precision fp16` (test.upscale(precision='fp16'), srx_conv2d_t::precision = 3): the same chain with the
 * activations STORED as fp16 -- 11 significant bits instead of bf16's 8 at the same bytes per pixel, range +-65504 (the host
 * checks the output for overflow).  Every entry point mirrors its bf16 namesake above: same arguments, same validation, same
 * layouts and launch geometry, `void*` tensors hold fp16; packed weights are fp16 (BatchNorm scale applied in fp32 first),
 * products are fp16 x fp16 on v_mfma_f32_32x32x16_f16, sums fp32, every rounding to fp16 is to nearest even.
 * srx_conv3x3_c64_bf16_plan describes the fp16 launches too (same geometry). */
size_t srx_conv3x3_c64_f16_packed_bytes(int Cout);
int srx_conv3x3_c64_f16_pack(const float* w, const float* bias, const float* out_scale, int Cout, int shuffle, void* wpk,
                             void* stream);
/* y (fp16) = act(conv(x) + bias) [+ residual (fp16)], rounded once */
int srx_conv3x3_c64_f16_fwd(int N, int H, int W, int Cout, int shuffle, const void* x, const void* wpk, float slope,
                            const void* residual, void* y, int y_cs, void* stream);
/* The 64 -> 64k layers with one PReLU slope per output channel (the compact generator's body): the arguments of
 * srx_conv3x3_c64_{bf16,f16}_fwd with a device array slopes[Cout] (16-byte aligned) in place of the scalar;
 * y = v > 0 ? v : slopes[c] * v with v = conv(x) + bias, then the optional addend, rounded once.  shuffle must be 0.  A kernel
 * instantiation of its own: the scalar entry points keep their code and bits. */
int srx_conv3x3_c64_bf16_fwd_slopes(int N, int H, int W, int Cout, int shuffle, const void* x, const void* wpk,
                                    const float* slopes, const void* residual, void* y, int y_cs, void* stream);
int srx_conv3x3_c64_f16_fwd_slopes(int N, int H, int W, int Cout, int shuffle, const void* x, const void* wpk,
                                   const float* slopes, const void* residual, void* y, int y_cs, void* stream);
/* fp32 -> fp16 rounds to nearest even (beyond 65519.99..: +-inf); fp16 -> fp32 is exact; n a positive multiple of 4 */
int srx_f32_to_f16(const float* x, void* y, int64_t n, void* stream);
int srx_f16_to_f32(const void* x, float* y, int64_t n, void* stream);
/* the 9x9 64 -> <= 3 output conv on an fp16 input: fp16 products, fp32 accumulation, y fp32 [N][H][W][4] */
size_t srx_conv9x9_c64_thin_f16_packed_bytes(void);
int srx_conv9x9_c64_thin_f16_pack(const float* w, const float* bias, int Cout, void* wpk, void* stream);
int srx_conv9x9_c64_thin_f16_fwd(int N, int H, int W, const void* x, const void* wpk, float* y, void* stream);

/* y = act(conv(x, W) + bias) * out_scale + residual, residual laid out like y (not for shuffle layers).
 * With the eval-mode BatchNorm folded into W and bias by the host this is a whole `x + BN(conv(.))` of the
 * residual block (srgan/residual.py:86-91, srgan/generator.py:77-78) in one kernel; with out_scale = 0.2 it
 * is `conv5 * scale_ratio + x` of the dense block (esrgan/residual.py:86). */
int srx_conv2d_fwd_residual(const srx_conv2d_t* d, const float* x, const float* wpk_fwd, const float* bias,
                            const float* residual, float out_scale, float* y, float* ws, size_t ws_floats, void* stream);
/* dx = conv_transpose(dy, W)  (autograd of nn.Conv2d wrt its input).  accumulate != 0 adds into dx
 * (stride-1 layers on the generic kernel): the dense block's convs share one 192-channel input buffer
 * (channel stride Cin_s, the first Cin channels are this layer's input), so their input gradients sum in
 * place of the torch.cat adjoint (esrgan/residual.py:81-85). */
int srx_conv2d_bwd_data(const srx_conv2d_t* d, const float* dy, const float* wpk_bwd, float* dx,
                        int accumulate, float* ws, size_t ws_floats, void* stream);
/* dx = conv_transpose(dy, W) + addend (laid out like dx, not dx itself): the gradient of `x` in `x + f(conv(x))` --
 * the skip connection of the residual block (srgan/residual.py:86-91) -- without autograd's separate add pass.
 * Stride-1 layers. */
int srx_conv2d_bwd_data_add(const srx_conv2d_t* d, const float* dy, const float* wpk_bwd, const float* addend,
                            float* dx, float* ws, size_t ws_floats, void* stream);
/* The same followed by the backward of the activation that PRODUCED this conv's input, for the input channels
 * [c_lo, c_hi): dx[.., c] = (accumulate ? dx[.., c] : 0) + conv_transpose(dy, W)[.., c], then for c in the range
 * dx[.., c] *= (x[.., c] > 0 ? 1 : slope), x = that activation's output = the conv's saved input (laid out like dx).
 * In the VGG19 feature stack (srgan/loss.py:30-31,52: conv, ReLU, conv, ReLU, ...) every ReLU backward then rides
 * in the epilogue of the data gradient above it (range = all channels); in ESRGAN's dense block
 * (esrgan/residual.py:81-85) the conv that completes the gradient of a 32-channel slice of the shared buffer also
 * applies that slice's LeakyReLU backward.  Stride-1 layers, generic kernel; range in whole channel quads. */
int srx_conv2d_bwd_data_act(const srx_conv2d_t* d, const float* dy, const float* wpk_bwd, const float* x, float slope,
                            int c_lo, int c_hi, int accumulate, float* dx, float* ws, size_t ws_floats, void* stream);
/* The general form of the three calls above, for a chain of blocks whose tensors have different channel strides:
 *   dx[m][c] = (accumulate ? dx[m][c] : 0) + out_scale * conv_transpose(dy, W)[m][c]
 *              + (c < addend_channels ? addend_scale * addend[m * addend_ld + c] : 0),
 * followed by the activation backward on [c_lo, c_hi) when act_out is given.  ESRGAN's RRDB trunk (esrgan/generator.py:
 * 54-56,70; esrgan/residual.py:81-86,125-128) keeps every dense block's input in the first 64 channels of that block's
 * 192-channel buffer: with this call conv5's data gradient takes `scale_ratio` and the block's own output gradient
 * (the `+ x` of :86, a dense 64-channel tensor) in its epilogue, and conv1's writes the block's input gradient as a
 * dense tensor, adding what the other four convs left in the first 64 channels of the shared gradient buffer --
 * the three elementwise passes per block that autograd runs for `out * 0.2 + x` are gone.  Zero fields mean: no
 * accumulate, scales 1, addend laid out like dx, all channels.  Stride-1 layers on the generic kernel; an addend
 * excludes accumulate; strides and channel counts in whole quads. */
typedef struct srx_dgrad_epilogue {
  int accumulate;
  float out_scale;
  const float* addend;
  int addend_ld;
  int addend_channels;
  float addend_scale;
  const float* act_out;
  float act_slope;
  int c_lo, c_hi;
} srx_dgrad_epilogue_t;
int srx_conv2d_bwd_data_ex(const srx_conv2d_t* d, const float* dy, const float* wpk_bwd, float* dx,
                           const srx_dgrad_epilogue_t* e, float* ws, size_t ws_floats, void* stream);
/* dx = conv^T(dy) [+ addend] AND, in the same launch, the first pass of the backward of the BatchNorm (+ PReLU) layer whose
 * output gradient dx is -- the layer that fed this conv in the forward pass (srgan/residual.py:86-90: conv2's data gradient
 * arrives at bn1 + prelu, conv1's (plus the skip gradient) at the previous block's bn2): table[row block][2C+4] = per-channel
 * sums of dz = dx * act'(bn(y)) and dz * xhat, and the PReLU slope partial in columns 2C and 2C+1.  bn_prelu: the slope
 * (device scalar) or NULL for a BatchNorm without activation.  Finish with srx_bn_act_bwd_finish(..., rows, 2, ...).
 * Only layers for which srx_conv2d_bwd_data_bn_rows returns non-zero (3x3, 64 -> 64, stride 1, few pixels: the residual tower). */
int srx_conv2d_bwd_data_bn_rows(const srx_conv2d_t* d);
int srx_conv2d_bwd_data_bn(const srx_conv2d_t* d, const float* dy, const float* wpk_bwd, const float* addend, float* dx,
                           const float* bn_y, const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                           const float* bn_beta, const float* bn_prelu, float* table, void* stream);
/* srx_conv2d_bwd_data_bn with the conv's output gradient produced on the way in: dout is the gradient arriving at the OUTPUT of
 * the BatchNorm (+ PReLU) layer above this conv (in_*: that layer's forward input y, statistics, parameters, slope or NULL, and
 * its finalised backward sums from srx_bn_act_bwd_finish(..., dy = NULL)); the second pass of that layer's backward runs while
 * the data gradient stages its input, and dy_out receives the conv's output gradient (its weight gradient reads it).
 * table == NULL: no BatchNorm below (then the bn_* pointers are ignored).  Same layers as srx_conv2d_bwd_data_bn. */
int srx_conv2d_bwd_data_bn_in_ok(const srx_conv2d_t* d);
int srx_conv2d_bwd_data_bn_in(const srx_conv2d_t* d, const float* dout, const float* in_y, const float* in_mean,
                              const float* in_invstd, const float* in_gamma, const float* in_beta, const float* in_prelu,
                              const float* in_sums, float* dy_out, const float* wpk_bwd, const float* addend, float* dx,
                              const float* bn_y, const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                              const float* bn_beta, const float* bn_prelu, float* table, void* stream);
/* y = conv(act(BatchNorm(y_in))) in ONE launch: y_in is the output of the conv below (srgan/residual.py:86-88: conv1 -> bn1 ->
 * prelu -> conv2), the training-mode statistics are already finalised (srx_bn_finalize), and the normalise + activate pass
 * runs while the conv stages its input; act_out receives the activation tensor (what srx_bn_act_fwd would have written: the
 * backward pass and the weight gradient of this conv read it).  bn_prelu: the slope (device scalar) or NULL for no
 * activation.  bn_residual: NULL, or a tensor added behind the activation -- `x + bn2(conv2(.))` at the end of a residual block
 * (srgan/residual.py:90-91) formed while the NEXT block's conv1 stages its input (a second patch load).  bn_partials as in srx_conv2d_fwd.  Only layers for which srx_conv2d_fwd_bn_in_ok returns 1 (3x3, 64 -> 64,
 * stride 1, few pixels: the residual tower at training sizes). */
int srx_conv2d_fwd_bn_in_ok(const srx_conv2d_t* d);
int srx_conv2d_fwd_bn_in(const srx_conv2d_t* d, const float* y_in, const float* bn_mean, const float* bn_invstd,
                         const float* bn_gamma, const float* bn_beta, const float* bn_prelu, const float* bn_residual,
                         float* act_out, const float* wpk, const float* bias, float* y, float* bn_partials, void* stream);
int srx_bn_act_bwd_finish(const float* dout, const float* y, const float* mean, const float* invstd, const float* gamma,
                          const float* beta, const float* table, int rows, int prelu_cols, float* sums, float* dy, int64_t M,
                          int C, int act, float slope, const float* prelu, float* dgamma_acc, float* dbeta_acc,
                          float* dprelu_acc, void* stream);
/* dw (OIHW) = autograd of nn.Conv2d wrt its weight; accumulate != 0 adds into dw (a .grad buffer)
 * instead of overwriting it.  db (may be NULL) receives the bias gradient
 * sum_m dy[m][co] under the same flag: the kernel stages every dy row anyway.  The same flag exists on srx_colsum, srx_linear_bwd_weight,
 * srx_prelu_bwd; srx_bn_act_bwd_reduce takes optional accumulation targets. */
int srx_conv2d_bwd_weight(const srx_conv2d_t* d, const float* x, const float* dy, float* dw_oihw,
                          int accumulate, float* db, float* ws, size_t ws_floats, void* stream);
/* The same for `nprob` (<= 72) problems of ONE geometry in one launch.  Autograd produces the weight gradients of
 * the generator's 33 identical 3x3 64->64 convs (srgan/residual.py:64,67; srgan/generator.py:48) one by one
 * between the data gradients, each 0.68 GFLOP -- too small to fill the chip -- and nothing reads them before
 * optimizer.step() (srgan/trainer.py:386-387,468-469), so the host may collect (x, dy) pairs during the backward
 * pass and hand them over together.  `per_out` consecutive problems are segments of one gradient and are summed
 * into one output (the discriminator's real and fake passes, srgan/trainer.py:446-450): xs / dys hold nprob
 * pointers, dws / dbs hold nprob / per_out (dbs, or single entries of it, may be NULL). */
size_t srx_conv2d_bwd_weight_multi_ws_floats(const srx_conv2d_t* d, int nprob);
int srx_conv2d_bwd_weight_multi(const srx_conv2d_t* d, int nprob, int per_out, const float* const* xs,
                                const float* const* dys, float* const* dws, int accumulate, float* const* dbs,
                                float* ws, size_t ws_floats, void* stream);
/* The same with one multiplier per output (out_scales: nprob / per_out host floats, NULL = all 1), applied to the
 * weight and the bias gradient: the dy handed over stands for out_scale * dy.  The dense block's conv5 sees the
 * block's output gradient times scale_ratio (esrgan/residual.py:86), which then is never written out. */
int srx_conv2d_bwd_weight_multi_scaled(const srx_conv2d_t* d, int nprob, int per_out, const float* const* xs,
                                       const float* const* dys, float* const* dws, int accumulate, float* const* dbs,
                                       const float* out_scales, float* ws, size_t ws_floats, void* stream);
/* Pairs: every problem is TWO convs of d->Cout / 2 output channels each that read the same input buffer and whose
 * output gradients are adjacent channel slices of one tensor -- conv1 + conv2 and conv3 + conv4 of a dense block
 * (esrgan/residual.py:81-85: conv k reads the first 64 + 32 (k - 1) channels of the block's buffer and its output gradient
 * is the next 32-channel slice of the gradient buffer).  d describes the pair as one layer: Cin = the larger input
 * width, Cout = both slices; the first conv has only cin_lo input channels, the rest of its rows is not written.
 * Alone, a 32-column problem leaves half of every 64-column MFMA tile multiplying padding; paired, 10-17 % of the tile
 * is unused.  dws_lo / dws_hi (and dbs_lo / dbs_hi, both or neither) hold nprob pointers each. */
int srx_conv2d_bwd_weight_multi_pair(const srx_conv2d_t* d, int nprob, const float* const* xs, const float* const* dys,
                                     float* const* dws_lo, float* const* dws_hi, int cin_lo, int accumulate,
                                     float* const* dbs_lo, float* const* dbs_hi, float* ws, size_t ws_floats, void* stream);

/* ------------------------------------------------- elementwise / reductions */
/* out[c] = sum_m x[m][c]  (bias gradient of Conv2d / Linear); ws >= 2*rows*C floats */
size_t srx_colsum_ws_floats(int64_t M, int C);
int srx_colsum(const float* x, float* out, int64_t M, int C, int Cs, int accumulate, float* ws, size_t ws_floats,
               void* stream);
/* dx = dy * act'(y) for sign-recoverable activations fused into a conv epilogue (ReLU, LeakyReLU) */
int srx_act_bwd_from_out(const float* dy, const float* y, float* dx, int64_t n, int act, float slope, void* stream);
/* the same on a channel slice of wider NHWC tensors (rows M, channels [0, C), row strides ldy / ly / ldx in
 * floats; dx may alias dy): the LeakyReLU of the dense block's conv1..4, whose outputs and gradients live
 * in shared 192-channel buffers instead of torch.cat copies (esrgan/residual.py:81-85) */
int srx_act_bwd_from_out_strided(const float* dy, int ldy, const float* y, int ly, float* dx, int ldx, int64_t M, int C,
                                 int act, float slope, void* stream);
/* nn.PReLU (one shared slope): srgan/generator.py:39, srgan/residual.py:29,66 */
int srx_prelu_fwd(const float* x, const float* slope, float* y, int64_t n, void* stream);
/* dx and d(slope); ws >= 1024 floats */
int srx_prelu_bwd(const float* dy, const float* x, const float* slope, float* dx, float* dslope,
                  int accumulate, int64_t n, float* ws, void* stream);
/* nn.PReLU(C), one slope per channel, on NHWC rows (csrc/compact.hip): x, y [M][Cs], slopes [C];
 * y = x > 0 ? x : slopes[c] * x for c < C, channels C .. Cs - 1 pass through.  y == x is allowed.  16-byte accesses:
 * C % 4 == 0, Cs % 4 == 0, C <= Cs, C <= 512, Cs <= 1024, or the call is refused before any launch. */
int srx_prelu_channels_fwd(const float* x, const float* slopes, float* y, int64_t M, int C, int Cs, void* stream);
/* dx = x > 0 ? dy : slopes[c] * dy (channels past C: dy) and dslopes[c] (+)= sum over rows of (x > 0 ? 0 : x * dy).  The sum
 * runs in fp64 per lane, per-workgroup partials go to fixed workspace slots and are added in index order -- no atomics, the
 * same bits from every call.  ws: 8-byte aligned, ws_floats >= srx_prelu_channels_ws_floats(M, C).  dx, dy, x disjoint. */
size_t srx_prelu_channels_ws_floats(int64_t M, int C);
int srx_prelu_channels_bwd(const float* dy, const float* x, const float* slopes, float* dx, float* dslopes, int accumulate,
                           int64_t M, int C, int Cs, float* ws, size_t ws_floats, void* stream);
/* The compact generator's tail in one pass: y4[n][s y + i][s x + j][c] = t[n][y][x][c s^2 + i s + j] + x4[n][y][x][c] for
 * c < 3, channel 3 of y4 = 0 -- PixelShuffle(s) of t's first 3 s^2 channels plus the nearest-enlarged input.  t: [N][h][w][t_cs],
 * t_dtype 0 fp32, 1 bf16, 2 fp16, t_cs >= 3 s^2 and a multiple of 4; x4 [N][h][w][4] and y4 [N][s h][s w][4] fp32; s = 2, 3, 4.
 * One fp32 add per element.  Every store is a whole NHWC-4 pixel, consecutive lanes along the output row. */
int srx_shuffle_add_nearest_fwd(const void* t, int t_dtype, int t_cs, const float* x4, float* y4, int N, int h, int w, int s,
                                void* stream);
/* The inverse permutation: dt[n][y][x][c s^2 + i s + j] = dy4[n][s y + i][s x + j][c], channels 3 s^2 .. t_cs - 1 of dt = 0
 * (fp32 dt; the input image takes no gradient). */
int srx_shuffle_add_nearest_bwd(const float* dy4, float* dt, int t_cs, int N, int h, int w, int s, void* stream);
/* nn.LeakyReLU as a standalone op (ESRGAN, esrgan/residual.py:36-55) */
int srx_lrelu_fwd(const float* x, float* y, int64_t n, float slope, void* stream);
/* y = a*x + b*z  (residual scaling of esrgan/residual.py:86,128; torch.add of srgan/generator.py:78) */
int srx_axpby(const float* x, const float* z, float* y, int64_t n, float a, float b, void* stream);
/* ESRGAN ResidualDenseBlock.forward (esrgan/residual.py:65-86) as ONE launch, bf16 products / fp32 accumulate:
 *   c_k = LeakyReLU(conv_k(cat(x, c_1..c_{k-1})) + b_k, slope), k = 1..4;  out = (conv_5(cat(x, c_1..c_4)) + b_5) * scale + x
 * buf: NHWC [N][H][W][ld], ld >= 192: x in channels 0..63 on entry; c_1..c_4 (fp32, what the backward pass reads) are
 * written to channels 64..191.  out: [N][H][W][out_ld], channels 0..63 (the next block's buffer in an RRDB chain).
 * wpk: this block's stream of srx_rdb_packed_bytes() bytes written by srx_rdb_pack; bias5: HOST array of the five
 * device bias pointers (32, 32, 32, 32, 64 floats).  One workgroup per 8x8 pixel tile; any H, W. */
size_t srx_rdb_packed_bytes(void);
/* w_table_dev: DEVICE array of 5 * nblk pointers to the OIHW fp32 weights (conv1..conv5 of block 0, of block 1, ...);
 * dst: nblk * srx_rdb_packed_bytes() bytes.  One launch for all blocks (after an optimiser step). */
int srx_rdb_pack(const float* const* w_table_dev, int nblk, void* dst, void* stream);
/* extra (may be NULL): out = (that) * post_scale + extra -- the `out * 0.2 + x` that ends a ResidualInResidualDenseBlock
 * (esrgan/residual.py:128) in the epilogue of its third dense block; [N][H][W][extra_ld], channels 0..63.  `extra` may be an
 * OLDER block's buffer but never `out`, and `out` is never `buf` itself (neighbouring tiles read their halo from it while
 * this one writes): both are refused. */
int srx_rdb_fwd(int N, int H, int W, float* buf, int ld, const void* wpk, const float* const* bias5, float scale,
                float slope, float post_scale, const float* extra, int extra_ld, float* out, int out_ld, void* stream);
/* The block's data-gradient chain (autograd of the five convs and four LeakyReLUs of esrgan/residual.py:81-86 with
 * respect to their inputs) as ONE launch, the forward's schedule run in reverse:
 *   g5 = scale * dy;  g_j = LeakyReLU'(c_j) * sum_{k > j} conv_k^T(g_k)[c_j], j = 4..1;  dx = sum_k conv_k^T(g_k)[x] + skip_scale * skip
 * dy: [N][H][W][dy_ld] (the gradient of the block's output; `scale` = the block's scale_ratio times whatever factor the
 * caller's chain rule has collected); buf: the block's saved buffer (x, c1..c4, ld >= 192: read for the masks);
 * gbuf: [N][H][W][gld >= 192], receives g1..g4 (fp32) at channels 64..191 -- the output gradients the convs' weight
 * gradients are computed from (srx_conv2d_bwd_weight_multi_pair / _scaled; conv5's is dy); skip: [N][H][W][skip_ld]: the
 * gradient that reaches x around the convs (`+ x` of :86); dx: [N][H][W][dx_ld] channels 0..63, must not alias dy / skip.
 * wpk_bwd: this block's stream written by srx_rdb_pack_bwd (transposed, tap-flipped; same size as the forward's). */
int srx_rdb_pack_bwd(const float* const* w_table_dev, int nblk, void* dst, void* stream);
/* extra (may be NULL): a second gradient added to dx as it is (the RRDB's own skip connection reaching its first block) */
int srx_rdb_bwd(int N, int H, int W, const float* dy, int dy_ld, float scale, const float* buf, int ld, const void* wpk_bwd,
                float slope, float* gbuf, int gld, const float* skip, int skip_ld, float skip_scale, const float* extra,
                int extra_ld, float* dx, int dx_ld, void* stream);
/* Per-step scalars without a per-step device->host sync: append n <= 4 device scalars (*a, *b, *c, *d) as one
 * 4-float record to ring[(*counter % cap) * 4 ...] and increment *counter (device int32).  The launch is the same every
 * step, so it sits inside the replayed hipGraph; the host reads `cap` records back in one copy.  Replaces the
 * reference's `wandb.log({... 'train-loss': loss}, step)` tensor -> host read on every step
 * (srgan/trainer.py:393-399,459-466; esrgan/trainer.py:393-399,471-478) */
int srx_ring_push(const float* a, const float* b, const float* c, const float* d, int n, float* ring, int* counter,
                  int cap, void* stream);
/* y[m][y_off+c] = a*x[m][x_off+c] + b*z[m][z_off+c], c < C: the same on channel slices of tensors with their own
 * channel strides (`out * 0.2 + x` of an RRDB, esrgan/residual.py:128, between two dense-block buffers) */
int srx_axpby_channels(const float* x, int x_cs, int x_off, const float* z, int z_cs, int z_off, float* y, int y_cs,
                       int y_off, int C, int64_t M, float a, float b, void* stream);
/* channel concat / split of NHWC tensors: dst[m][dst_off+c] (+)= src[m][src_off+c], c < C
 * (torch.cat((x, conv1, ...), dim=1) of the dense block, esrgan/residual.py:82-85, and its adjoint) */
int srx_copy_channels(const float* src, int src_cs, int src_off, float* dst, int dst_cs, int dst_off, int C,
                      int64_t M, int accumulate, void* stream);
/* F.interpolate(scale_factor=2, mode='nearest') (esrgan/generator.py:73,76) and its adjoint; x is [N][H][W][C] */
int srx_upsample_nearest2x_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int srx_upsample_nearest2x_bwd(const float* dy, float* dx, int N, int H, int W, int C, void* stream);
/* F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) and its adjoint on NHWC fp32: x is
 * [N][H][W][Cs], y [N][2H][2W][Cs]; the first C channels (rounded up to whole quads, which must fit in
 * Cs) are computed, the others are left alone.  Weights 0.75 / 0.25 per direction, the neighbour clamped
 * at the border.  The adjoint is a gather (every input pixel adds its at most 4 x 4 output pixels in a
 * fixed order): no atomics, repeatable bits.  Cs a multiple of 4, tensors 16-byte aligned. */
int srx_upsample_bilinear2x_fwd(const float* x, float* y, int N, int H, int W, int C, int Cs, void* stream);
int srx_upsample_bilinear2x_bwd(const float* dy, float* dx, int N, int H, int W, int C, int Cs, void* stream);
/* nn.Sigmoid of the SRGAN discriminator head (srgan/discriminator.py:68) */
int srx_sigmoid_fwd(const float* x, float* y, int64_t n, void* stream);
int srx_sigmoid_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream);

/* ------------------------------------------------ on-device data pipeline */
/* TrainData.__getitem__ of the reference (dataset.py:88-99,121-125: RandomCrop, RandomHorizontalFlip,
 * RandomVerticalFlip, ToTensor) for a batch of decoded images resident in device memory.
 * imgs: device array of N pointers to HWC uint8 RGB images; meta: device int32 [N][6] =
 * {H, W, top, left, hflip, vflip}; out: [N][3][crop][crop] float in [0, 1]. */
int srx_crop_flip_u8(const void* const* imgs, const int32_t* meta, float* out_nchw, int N, int crop, void* stream);
/* Resize(crop // scale, BICUBIC) of the reference's low-resolution branch (dataset.py:93-96): antialiased
 * Keys bicubic (a = -0.5) reduction by an integer factor on NCHW floats; quantize != 0 rounds the result
 * to 8 bits like the PIL image the reference converts back with ToTensor. */
int srx_bicubic_down(const float* in_nchw, float* out_nchw, int N, int C, int H, int W, int scale, int quantize,
                     void* stream);

/* ------------------------------------------ blind degradation (degrade.hip) */
/* The first-order degradation model of BSRGAN / Real-ESRGAN around srx_bicubic_down: blur, resize, noise, JPEG
 * ('Blind degradation').  Images are float NCHW in [0, 1] with 3 channels; per-sample parameters are DEVICE
 * arrays, read by the kernels, which are safe for any value they find there.
 *
 * Each sample correlated with its own normalised Gaussian: out[y][x] = sum_ij w[i][j] in[y + i - r][x + j - r], r = ksize / 2,
 * w[i][j] ~ exp(-v' S^-1 v / 2), v = (j - r, i - r), S = R(theta) diag(sigma_x^2, sigma_y^2) R(theta)', sum w = 1; borders are
 * reflected (-k -> k, as F.pad(mode='reflect')).  parm: float [N][4] = {sigma_x, sigma_y, theta, unused}; ksize: int32 [N],
 * 0 (the sample is copied) or odd in 1..21 -- any other value is clamped: <= 0 to 0, even to the next odd, > 21 to 21.
 * Refused: C != 3, H <= 10 or W <= 10 (a 21-tap reflect needs 11 rows), out == in, N > 65535. */
int srx_blur_aniso(const float* in_nchw, float* out_nchw, const float* parm, const int32_t* ksize, int N, int C, int H,
                   int W, void* stream);
/* Each sample correlated with a kernel given as an operand -- the second-order model's sinc, generalised Gaussian and plateau
 * kernels ('Second-order degradation'): out[n][c][y][x] = sum_ij w_n[i][j] in[n][c][y + i - r][x + j - r], r = ks / 2,
 * borders reflected as srx_blur_aniso's.  weights: DEVICE float [N][21][21]; sample n's ks x ks kernel sits centred in its slot
 * (rows and columns 10 - r .. 10 + r) and only that window is read.  The weights are used as given: neither normalised nor
 * clamped (sinc weights are negative in places).  ksize: int32 [N], clamped like srx_blur_aniso's; 0 copies the sample.
 * quantize != 0 clamps the result (a copied sample too) to [0, 1] and rounds it to 8 bits as srx_add_gaussian_noise does.
 * fmas in ascending (i, j), no atomics, no device state: the same bits from every call.
 * Refused: null pointers, C != 3, H <= 10 or W <= 10, out == in, N outside 1..65535. */
int srx_filter2d(const float* in_nchw, float* out_nchw, const float* weights, const int32_t* ksize, int N, int C, int H, int W,
                 int quantize, void* stream);
/* out[n][c][p] = in[n][c][p] + sigma[n] z_c, p = y W + x.  Philox4x32-10 with counter (p, n, 0, 0) and key (seed_lo, seed_hi)
 * gives r0..r3; u_k = ((r_k >> 8) + 0.5) 2^-24; z_0 = sqrt(-2 ln u_0) cos(2 pi u_1), z_1 = sqrt(-2 ln u_0) sin(2 pi u_1),
 * z_2 = sqrt(-2 ln u_2) cos(2 pi u_3); gray[n] != 0: all three channels get z_0.  Stateless: the same seed gives the same bits.
 * sigma: float [N]; gray: int32 [N]; [N][3][H][W]; quantize != 0 clamps to [0, 1] and rounds to 8 bits. */
int srx_add_gaussian_noise(const float* in_nchw, float* out_nchw, const float* sigma, const int32_t* gray, uint32_t seed_lo,
                           uint32_t seed_hi, int N, int H, int W, int quantize, void* stream);
/* Signal-dependent (shot) noise, Real-ESRGAN's generate_poisson_noise_pt per sample ('Poisson noise').  With
 * q = rint(clamp(x, 0, 1) 255) of a value x, vals = the number of distinct q over the sample's three channels rounded up to a
 * power of two (1..256), k ~ Poisson(q vals / 255): out = in + scale[n] (k / vals - q / 255) -- q (float) times 1.0f / 255.0f,
 * the difference and one fma, k / vals exact.  gray[n] != 0: q comes from the luma fadd(fadd(fmul(.299f, r), fmul(.587f, g)),
 * fmul(.114f, b)) (each operation rounded once: the kernels switch contraction off there), vals counts the luma levels and one k per pixel feeds the three
 * channels.  scale[n] == 0 copies the sample bit for bit.
 * The draw: Philox4x32-10 with counter (p, n, 1, 0) and key (seed_lo, seed_hi) gives r0..r3, word c for channel c (word 0 for
 * all three of a grey sample); k = first[v][q] + the number of entries of win[v][q][0..255] that are <= r >> 1, v = log2(vals).
 * tables: DEVICE int32, first[9][256] followed by the uint32 thresholds win[9][256][256] -- what degradation.
 * poisson_table_words() builds on the host in float64, so that no device float decides an integer.
 * levels: DEVICE int32 [N][8], an OUTPUT: the call clears it, then sets bit q of sample n's 256-bit mask for every level q the
 * sample holds (merged with atomicOr; a sample with scale 0 keeps an empty mask).  scale: float [N]; gray: int32 [N];
 * [N][3][H][W]; quantize as in srx_add_gaussian_noise.  A clear and two launches; stateless: the same seed gives the same bits.
 * Refused before anything is issued: a null pointer, N outside 1..65535, H or W < 1, H W >= 2^31. */
int srx_add_poisson_noise(const float* in_nchw, float* out_nchw, const float* scale, const int32_t* gray, const int32_t* tables,
                          int32_t* levels, uint32_t seed_lo, uint32_t seed_hi, int N, int H, int W, int quantize, void* stream);
/* What a baseline JPEG codec at quality[n] (int32 [N], libjpeg's scale) does to the pixels of a 4:4:4 image: 8-bit samples,
 * libjpeg's integer RGB -> YCbCr, orthonormal 8 x 8 DCT, the Annex K tables scaled by libjpeg's rule, rounding, the inverse
 * transform (decoded samples unrounded), float YCbCr -> RGB, / 255, clamp.  No chroma subsampling; entropy coding is
 * lossless and left out.  A quality outside 1..100 copies the sample.  [N][3][H][W], H and W multiples of 8 (others are
 * refused), N <= 65535; quantize != 0 rounds the result to 8 bits. */
int srx_jpeg_sim(const float* in_nchw, float* out_nchw, const int32_t* quality, int N, int H, int W, int quantize,
                 void* stream);
/* srx_jpeg_sim with 4:2:0 chroma subsampling per sample ('Chroma subsampling').  chroma420: int32 [N].
 * chroma420[n] == 0: sample n gets srx_jpeg_sim's arithmetic and its bits.  Any other value: Y is coded as there; the integer
 * Cb and Cr are averaged 2 x 2 as libjpeg's h2v2_downsample does -- (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2, ... along
 * each row of the H/2 x W/2 plane -- the plane is edge-replicated to whole 8 x 8 blocks (a partial 16 x 16 MCU), coded with the
 * chrominance table, and brought back by libjpeg's h2v2_fancy_upsample in floating point: with c the decoded sample over a
 * pixel, v and h its vertical and horizontal neighbours on the pixel's side and d the diagonal one, each the plane's edge
 * sample where it would lie outside the H/2 x W/2 plane, fma(3, fma(3, c, v), fma(3, h, d)) / 16.  A quality outside 1..100
 * copies the sample whatever its flag.
 * workspace: DEVICE, at least srx_jpeg_sim2_workspace(N, H, W) bytes, the decoded chroma planes between the two launches;
 * every word that is read is written first, so its contents before the call do not matter.  The library allocates nothing.
 * quot_out: nullable; DEVICE float [N][3][H W], coefficient / step before the rounding, block after block in raster order, 64
 * values [vertical][horizontal frequency] each: a 4:4:4 sample's Y, Cb and Cr blocks from [n][0], [n][1] and [n][2]; a 4:2:0
 * sample's Y blocks from [n][0] and the ceil(H / 16) x ceil(W / 16) blocks of Cb from [n][1] and of Cr from [n][2], the rest
 * of those two planes untouched, as is all of a copied sample's.
 * A chroma and a luma launch.  Refused before either: a null pointer other than quot_out and stream, N outside 1..65535, H or W
 * not a positive multiple of 8, H / 8 > 65535, H W >= 2^31, a workspace that is too small. */
size_t srx_jpeg_sim2_workspace(int N, int H, int W);
int srx_jpeg_sim2(const float* in_nchw, float* out_nchw, const int32_t* quality, const int32_t* chroma420, int N, int H, int W,
                  int quantize, void* workspace, size_t workspace_bytes, float* quot_out, void* stream);

/* ------------------------------------------------- sharpened targets (usm.hip) */
/* Real-ESRGAN's USMSharp on float planes in [0, 1] ('Sharpened targets').  G is the separable correlation with
 * g (x) g, g = taps (DEVICE float [ksize], used as given), borders reflected (-k -> k, as F.pad(mode='reflect')):
 *   blur = G(in); res = in - blur; mask = |res| 255 > threshold ? 1 : 0; soft = G(mask);
 *   out = in + soft (clamp(in + weight res, 0, 1) - in)
 * the last line one fma, so that weight = 0 on inputs in [0, 1], and a threshold no residual reaches, give out == in bit for bit.
 * in, out, blur, mask: [planes][H][W]; blur and mask are caller buffers that are left holding their planes (mask exactly 0.0 or
 * 1.0).  Two launches; fmas in ascending tap order, horizontal pass first; no atomics, no device state: the same bits from
 * every call.
 * Refused before any launch: a null pointer; ksize even, < 3 or > 51; H or W <= ksize / 2 (the reflection needs ksize / 2 + 1
 * samples); planes < 1; planes * H * W >= 2^31; a non-finite weight or threshold; out, blur or mask overlapping in or each
 * other. */
int srx_usm_sharpen(const float* in, float* out, float* blur, float* mask, const float* taps, int ksize, int64_t planes, int H,
                    int W, float weight, float threshold, void* stream);

/* ------------------------------------------------- training pair pool (pool.hip) */
/* Real-ESRGAN's training pair pool (_dequeue_and_enqueue) in one launch ('Training pair pool').  pool_a: float
 * [cap][elems_a], batch_a: float [n][elems_a]; the _b pair likewise with elems_b floats per sample.  _a is the low-resolution
 * side and _b the target; both are moved by the SAME launch, so a low-resolution sample and its target never part.
 * pool_b == batch_b == NULL with elems_b == 0: one tensor only.  slots: DEVICE int32 [n].
 *   mode 0 (store):    pool[slots[i]] = batch[i]; the batch is left untouched
 *   mode 1 (exchange): pool[slots[i]] and batch[i] change places in place (both read into registers, then both written)
 * Values are moved as 32-bit words, 16 bytes at a time where elems % 4 == 0 and the bases are 16-byte aligned: every bit
 * pattern arrives unchanged.  The kernel is safe for any value it finds in slots: a slot outside [0, cap) leaves sample i and
 * the pool untouched.  DUPLICATE slots are a caller error: which of the samples ends up in the slot, and what the batch holds
 * afterwards, is unspecified -- but every access stays inside the two buffers.  No atomics, no device state; the grid is sized
 * from elems and n alone.
 * Refused before anything is issued: a null pool_a, batch_a or slots; exactly one of pool_b / batch_b null, or a null pair with
 * elems_b != 0 (or a given one with elems_b == 0); elems_a < 1 or elems_b < 0; n outside 1..65535; cap < 1 or n > cap;
 * cap * elems >= 2^31 for either side; mode not 0 or 1; any two of the pool and batch ranges overlapping. */
int srx_pool_exchange(float* pool_a, float* batch_a, int64_t elems_a, float* pool_b, float* batch_b, int64_t elems_b,
                      const int32_t* slots, int n, int cap, int mode, void* stream);

/* -------------------------------------------------------------- batch norm */
/* nn.BatchNorm2d(C), eps 1e-5, momentum 0.1 (srgan/residual.py:65,68;
 * srgan/generator.py:49; srgan/discriminator.py:36-60).
 * stats from an activation tensor: partial table [rows][C][2] */
int srx_bn_stat_rows(int64_t M);
int srx_bn_rows_per_block(int64_t M);  /* rows summed per partial row (and per row block of the backward reduction) */
int srx_bn_partial_stats(const float* y, float* partials, int64_t M, int C, void* stream);
/* reduce partials -> save_mean, save_invstd (biased variance); update running stats
 * (unbiased variance, momentum) and num_batches_tracked (int64) when non-NULL */
int srx_bn_finalize(const float* partials, int rows, int64_t M, int C, float eps, float momentum,
                    float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                    int64_t* num_batches_tracked, void* stream);
/* eval mode: save_mean = running_mean, save_invstd = rsqrt(running_var + eps) */
int srx_bn_eval_stats(const float* running_mean, const float* running_var, int C, float eps,
                      float* save_mean, float* save_invstd, void* stream);
/* out = act(gamma*(y-mean)*invstd + beta) [+ residual];  act: NONE / LRELU(slope) / PRELU(*prelu) */
int srx_bn_act_fwd(const float* y, const float* mean, const float* invstd, const float* gamma,
                   const float* beta, const float* residual, float* out, int64_t M, int C, int act,
                   float slope, const float* prelu, void* stream);
/* backward, pass 1: sums[0..C) = sum dz, sums[C..2C) = sum dz*xhat, sums[2C] = d(prelu slope)
 * (dz = dout * act'(bn(y))).  ws >= srx_bn_bwd_ws_floats */
size_t srx_bn_bwd_ws_floats(int64_t M, int C);
int srx_bn_act_bwd_reduce(const float* dout, const float* y, const float* mean, const float* invstd,
                          const float* gamma, const float* beta, float* sums, int64_t M, int C, int act,
                          float slope, const float* prelu, float* dgamma_acc, float* dbeta_acc,
                          float* dprelu_acc, float* ws, size_t ws_floats, void* stream);
/* backward, pass 2: dy = gamma*invstd*(dz - sum_dz/M - xhat*sum_dzxhat/M) (training) or
 * dy = gamma*invstd*dz (eval, training=0) */
int srx_bn_act_bwd_apply(const float* dout, const float* y, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, const float* sums, float* dy, int64_t M,
                         int C, int act, float slope, const float* prelu, int training, void* stream);

/* one-call forms used by the trainers.  `groups` > 1: the M rows are `groups` equal consecutive row ranges that are
 * normalised independently -- several forward calls of the reference run as one batch (the discriminator on the real
 * and on the fake images, srgan/trainer.py:446-447): save_mean / save_invstd are [groups][C], sums [groups][2C+4],
 * the running statistics are updated once per group in order, num_batches_tracked advances by `groups`, and the
 * parameter gradients sum over the groups.  Row blocks (conv tiles, srx_bn_stat_rows) must not straddle groups. */
int srx_bn_train_fwd(const float* y, const float* partials, int rows, int64_t M, int C, int groups, float eps,
                     float momentum, const float* gamma, const float* beta, const float* residual, float* out, int act,
                     float slope, const float* prelu, float* save_mean, float* save_invstd, float* running_mean,
                     float* running_var, int64_t* num_batches_tracked, void* stream);
int srx_bn_act_bwd(const float* dout, const float* y, const float* mean, const float* invstd, const float* gamma,
                   const float* beta, float* sums, float* dy, int64_t M, int C, int groups, int act, float slope,
                   const float* prelu, int training, float* dgamma_acc, float* dbeta_acc, float* dprelu_acc,
                   float* ws, size_t ws_floats, void* stream);

/* ------------------------------------------------- Winograd F(2x2, 3x3) (round 5) */
/* nn.Conv2d(Cin, Cout, 3, 1, 1) of wide layers -- the VGG19 feature extractor of the perceptual loss (srgan/loss.py:30-54;
 * torchvision cfg 'E') -- with 2.25x fewer multiplications than the direct form, all in fp32 (results differ from the direct
 * fp32 convolution by rounding only: ~5e-7 of the tensor's scale).  Layers: 3x3 / stride 1 / pad 1, precision 0, Cin and Cout
 * multiples of 32 with channel strides equal to them, even H and W, act NONE or RELU (srx_wino_applicable).
 *   pack:     upk = G g G^T of every channel pair, srx_wino_packed_floats(d) floats, in the order the kernel's waves load it;
 *             transpose = 1 packs the layer's DATA GRADIENT (a 3x3 / pad 1 conv of dy with the channels swapped and the taps flipped)
 *   fwd:      y = act(conv(x) + bias)
 *   bwd_data: dx = conv^T(dy), multiplied by the ReLU mask (relu_out > 0, laid out like dx; NULL: none) of the layer below -- the
 *             fold srx_conv2d_bwd_data_act does for the direct kernel
 * ws: srx_wino_ws_floats(d, which) floats; non-zero when the planner splits the input channels over several workgroups, or cuts
 * the tiles of the last, partly filled round of the chip along them.  x != y.  `which` names the launch, as the launch itself plans:
 *   0  srx_wino_fwd (bias, ReLU): any plan;
 *   1  srx_wino_bwd_data: any plan, Cin and Cout swapped;
 *   2  srx_wino_fwd_stats: no split of every tile (statistics come from whole outputs); the last round's tiles may be cut;
 *   3  srx_wino_fwd_act with a LeakyReLU, an addend or a PixelShuffle store (the only `which` a shuffle layer's plan can be asked
 *      with): neither split nor cut tiles -- the fix-up passes know none of the three -- so the workspace is 0 floats and may be
 *      NULL.  (A srx_wino_fwd_act call with none of the three plans as which = 0; a shuffle layer plans as 3 under any forward which.)
 * srx_wino_plan(d, which, out): out[6] = {BN, channel splits of every tile, workgroups, tile blocks, chunks per workgroup, parts per
 * tile of the last round (1: none)} of that launch (host only); any other `which` is refused.
 * Launch records: wino_kernel<BN> under srx_prof_start; the passes behind it -- "wino_fixup_kernel" (sums a channel split) and
 * "wino_tail_fixup_kernel<32>" / "<64>" (finishes the cut tiles) -- only under srx_prof_start_aux, as the weight gradient's reduce
 * kernels. */
int srx_wino_applicable(const srx_conv2d_t* d);
size_t srx_wino_packed_floats(const srx_conv2d_t* d);
size_t srx_wino_ws_floats(const srx_conv2d_t* d, int which);
int srx_wino_plan(const srx_conv2d_t* d, int which, int* out);
int srx_wino_pack(const srx_conv2d_t* d, const float* w_oihw, float* upk, int transpose, void* stream);
int srx_wino_fwd(const srx_conv2d_t* d, const float* x, const float* upk, const float* bias, float* y, float* ws, size_t ws_floats,
                 void* stream);
int srx_wino_bwd_data(const srx_conv2d_t* d, const float* dy, const float* upk_t, const float* relu_out, float* dx, float* ws,
                      size_t ws_floats, void* stream);
/* forward of a linear layer that a training-mode BatchNorm2d follows (srgan/discriminator.py:35-61): stats
 * [srx_wino_stat_rows(d)][Cout][2] = per tile block of 128 output pixels (32 consecutive 2x2 tiles, image-major) the per-channel
 * (sum, sum of squares) of y -- the table srx_bn_finalize / srx_bn_train_fwd take, as srx_conv2d_fwd's bn_partials */
int srx_wino_stat_rows(const srx_conv2d_t* d);
int srx_wino_fwd_stats(const srx_conv2d_t* d, const float* x, const float* upk, const float* bias, float* y, float* stats,
                       float* ws /* srx_wino_ws_floats(d, 2) floats */, size_t ws_floats, void* stream);
/* inference (functional.FoldedConv: conv with the eval-mode BatchNorm folded into weights and bias, srgan/residual.py:86-91):
 * y = act(conv(x) + bias) [+ residual], act = none / ReLU / LeakyReLU(d->slope) (a single-parameter PReLU is that); residual laid
 * out like y, a tensor of its own, may be NULL.  srx_wino_infer_applicable: as srx_wino_applicable, also for the 64 -> 64
 * layers the training path leaves to its row-tile kernel */
int srx_wino_infer_applicable(const srx_conv2d_t* d);
int srx_wino_fwd_act(const srx_conv2d_t* d, const float* x, const float* upk, const float* bias, const float* residual, float* y,
                     float* ws, size_t ws_floats, void* stream);
/* Measurement aid (tools/lab/wino_sweep.cpp: the sweep the planner's cost constants are fitted from; no reference counterpart): until
 * called again with (0, 0, 0), every Winograd plan of this process is (BN 32 / 64, channel splits of every tile, parts per tile of the
 * last round) instead of the planner's choice -- srx_wino_ws_floats / srx_wino_plan / the launches all follow it; combinations a
 * layer cannot run (BN not dividing Cout, more splits than 32-channel chunks, splits of a statistics / inference launch) fall back
 * to the planner. */
int srx_wino_force_plan(int bn, int zsplit, int tsplit);

/* ------------------------------------------------- bf16 storage of activations on the training path (round 5) */
/* Under autocast (esrgan/trainer.py:446,461) the reference's convs read and write half tensors.  These entry points keep the
 * activations and gradients BETWEEN the 3x3 / stride 1 / pad 1 convs of a frozen stack (VGG19[:36], srgan/loss.py:30-34,52-53)
 * as bf16 NHWC tensors.  The arithmetic is that of precision = 1 (bf16 products, fp32 accumulation): an operand is rounded
 * once, by its producer, instead of by every consumer's loader.  d->precision must be 1, Cin and Cout multiples of 64.
 * Packed weights are bf16: srx_conv3x3_bf16s_packed_bytes(d) bytes per copy (forward; data gradient = transposed, taps flipped).
 * which: 0 forward, 1 data gradient.  Tensors: `void*` = bf16. */
int srx_conv3x3_bf16s_applicable(const srx_conv2d_t* d);
size_t srx_conv3x3_bf16s_packed_bytes(const srx_conv2d_t* d);
int srx_conv3x3_bf16s_pack(const srx_conv2d_t* d, const float* w, void* wpk_fwd, void* wpk_bwd /* may be NULL */, void* stream);
size_t srx_conv3x3_bf16s_ws_floats(const srx_conv2d_t* d, int which);
/* y = [relu](conv(x) + bias): x bf16 [N][H][W][Cin]; y bf16 (y_is_bf16) or fp32 [N][H][W][Cout] */
int srx_conv3x3_bf16s_fwd(const srx_conv2d_t* d, const void* x, const void* wpk_fwd, const float* bias, int relu, void* y,
                          int y_is_bf16, float* ws, size_t ws_floats, void* stream);
/* dx = conv^T(dy) [* (relu_out > 0)]: dy bf16 [N][H][W][Cout]; relu_out (may be NULL): the bf16 output of the ReLU that produced
 * this layer's input; dx bf16 (dx_is_bf16) or fp32 [N][H][W][Cin] */
int srx_conv3x3_bf16s_bwd_data(const srx_conv2d_t* d, const void* dy, const void* wpk_bwd, const void* relu_out, void* dx,
                               int dx_is_bf16, float* ws, size_t ws_floats, void* stream);
/* the 3 -> 64 first layer in front of such a stack: srx_conv2d_fwd's kernel for it (precision = 1) with a bf16 output;
 * x fp32 [N][H][W][4], wpk_fwd: the layer's ordinary forward pack, y bf16 [N][H][W][64] */
int srx_conv2d_fwd_first3_to_bf16(const srx_conv2d_t* d, const float* x, const float* wpk_fwd, const float* bias, void* y,
                                  void* stream);
/* pools and the topmost activation backward of such a stack.  The pools read the fp32 output of the conv below them (the
 * choice of the maximum must not depend on bf16 rounding) and round what they hand on. */
int srx_maxpool2x2_fwd_to_bf16(const float* x, void* y, int N, int H, int W, int C, void* stream);
int srx_maxpool2x2_relu_bwd_bf16(const void* dy, const float* x, void* dx, int N, int H, int W, int C, void* stream);
int srx_act_bwd_from_out_to_bf16(const float* dy, const float* y, void* dx, int64_t n, int act, float slope, void* stream);

/* ----------------------------------------------------------------- pooling */
/* nn.MaxPool2d(2,2) of VGG19 (torchvision cfg 'E', srgan/loss.py:30-31); H, W even */
int srx_maxpool2x2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int srx_maxpool2x2_bwd(const float* dy, const float* x, float* dx, int N, int H, int W, int C, void* stream);
/* max-pool backward followed by the backward of the ReLU that produced x (conv, ReLU, MaxPool in cfg 'E') */
int srx_maxpool2x2_relu_bwd(const float* dy, const float* x, float* dx, int N, int H, int W, int C, void* stream);

/* ------------------------------------------- multi-layer perceptual loss (csrc/percep.hip) */
/* Real-ESRGAN's perceptual loss (BasicSR PerceptualLoss: conv1_2, conv2_2, conv3_4, conv4_4, conv5_4 of VGG19 BEFORE their ReLU,
 * ImageNet-normalised inputs, weighted L1).  In cfg 'E' every tap but the last sits in front of a max-pool, and ReLU and max
 * commute (maxpool(relu(x)) == relu(maxpool(x))), so a tap conv writes its pre-activation once and the pool applies the ReLU.
 * These are the streaming kernels around the taps; the convs are the stack's own.  No floating-point atomics, fixed grids and
 * fixed reduction trees: every result is a fixed function of its arguments.  `void*` tensors are fp32 or bf16 as their flag says. */
/* out[0:N] = (src - mean) * inv_std, out[N:2N] = the same of tgt (tgt NULL: a batch of N); [.,H,W,4] images, channel 3 written as 0.
 * The product is formed in fp64 and rounded once. */
int srx_normalize_pair_nhwc4(const float* src, const float* tgt, float* out, int N, int H, int W, const float mean[3],
                             const float inv_std[3], void* stream);
/* dsrc = dout * inv_std per channel (dout: the first N images' gradient), channel 3 written as 0 */
int srx_normalize_nhwc4_bwd(const float* dout, float* dsrc, int N, int H, int W, const float inv_std[3], void* stream);
/* y = relu(maxpool2x2(x)): x fp32 [N_tot][H][W][C] pre-ReLU, y [N_tot][H/2][W/2][C] fp32 or bf16 (the maximum is chosen on the fp32
 * values and rounded once).  partial != NULL (needs N_tot == 2 * N_src): a workgroup takes sample i together with sample i + N_src
 * and writes partial[workgroup] = its sum of |x[i] - x[i + N_src]| over the windows it loaded; srx_tap_blocks workgroups. */
int srx_tap_blocks(int N_src, int H, int W, int C);
int srx_maxpool2x2_relu_fwd_tap(const float* x, void* y, int y_is_bf16, int N_src, int N_tot, int H, int W, int C, float* partial,
                                void* stream);
/* loss[0] = (accumulate ? loss[0] : 0) + (float)(scale * sum(partial[0:n_partial])); the sum is an fp64 tree of one workgroup */
int srx_tap_l1_finalize(const float* partial, int n_partial, double scale, float* loss, int accumulate, void* stream);
/* the tap without a pool behind it, and taps against precomputed target features:
 * loss[0] = (accumulate ? loss[0] : 0) + weight * mean|a - b|; n a multiple of 4, ws >= 1024 floats */
int srx_tap_l1_fwd(const float* a, const float* b, int64_t n, double weight, float* loss, int accumulate, float* ws, void* stream);
/* dx = poolrelu_bwd(dy; x_src) + coef * gscale[0] * sign(x_src - x_tgt): the first term is srx_maxpool2x2_relu_bwd's on the
 * pre-ReLU x_src (gradient to the first maximum in scan order when that maximum is > 0), the second srx_l1_bwd's (sign(0) = 0).
 * dy [N_src][H/2][W/2][C], x_src, x_tgt fp32 and dx [N_src][H][W][C]; bf16 forms: the sum is formed in fp32 and rounded once. */
int srx_maxpool2x2_relu_bwd_tap(const void* dy, int dy_is_bf16, const float* x_src, const float* x_tgt, void* dx, int dx_is_bf16,
                                float coef, const float* gscale, int N_src, int H, int W, int C, void* stream);
/* g = coef * gscale[0] * sign(fs - ft): the gradient entering at the last tap; n a multiple of 4 */
int srx_tap_l1_bwd_top(const float* fs, const float* ft, void* g, int g_is_bf16, float coef, const float* gscale, int64_t n,
                       void* stream);

/* ------------------------------------------------------------------ linear */
/* nn.Linear (srgan/discriminator.py:65,67; esrgan/discriminator.py:73,75).
 * x [B][K], w [J][K] (reference layout), y [B][J] = act(x w^T + bias)
 * ws: srx_linear_ws_floats floats -- the slabs of the forward's and the data gradient's splits, under srx_linear_force those
 * of the forced plan */
size_t srx_linear_ws_floats(int B, int K, int J);
int srx_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int K, int J,
                   int act, float slope, float* ws, size_t ws_floats, void* stream);
int srx_linear_bwd_data(const float* dy, const float* w, float* dx, int B, int K, int J, float* ws,
                        size_t ws_floats, void* stream);
int srx_linear_bwd_weight(const float* x, const float* dy, float* dw, int accumulate, int B, int K, int J,
                          void* stream);

/* ------------------------------------------------------------------ losses */
/* all losses reduce with mean; `loss` is one float on the device; ws >= 2048 floats.
 * nn.MSELoss (srgan/trainer.py:163,384), nn.L1Loss / F.l1_loss (srgan/loss.py:52; esrgan/trainer.py:163) */
int srx_mse_fwd(const float* a, const float* b, float* loss, int64_t n, float* ws, void* stream);
int srx_l1_fwd(const float* a, const float* b, float* loss, int64_t n, float* ws, void* stream);
/* da = gscale[0] * d(mean loss)/da ; db (if non-NULL) = -da */
int srx_mse_bwd(const float* a, const float* b, const float* gscale, float* da, float* db, int64_t n, void* stream);
int srx_l1_bwd(const float* a, const float* b, const float* gscale, float* da, float* db, int64_t n, void* stream);
/* F.l1_loss with an explicit divisor `count` (<= n): NHWC images carry a zero padding channel (3 of 4 stored channels are
 * real), and the reference's mean (esrgan/trainer.py:466) runs over the real elements only */
int srx_l1_fwd_count(const float* a, const float* b, float* loss, int64_t n, int64_t count, float* ws, void* stream);
int srx_l1_bwd_count(const float* a, const float* b, const float* gscale, float* da, float* db, int64_t n, int64_t count,
                     void* stream);
/* nn.BCELoss on probabilities against a constant label (srgan/trainer.py:164,446-447,456);
 * log terms clamped at -100 as torch does */
int srx_bce_fwd(const float* p, float target, float* loss, int64_t n, float* ws, void* stream);
int srx_bce_bwd(const float* p, float target, const float* gscale, float* dp, int64_t n, void* stream);
/* nn.BCEWithLogitsLoss(x - shift[0], target) (esrgan/trainer.py:164,451-453,468); shift may be NULL */
int srx_bce_logits_fwd(const float* x, const float* shift, float target, float* loss, int64_t n, float* ws, void* stream);
int srx_bce_logits_bwd(const float* x, const float* shift, float target, const float* gscale, float* dx, int64_t n, void* stream);
/* torch.mean over all elements (esrgan/trainer.py:451-452,468); ws >= 2048 floats */
int srx_mean_fwd(const float* x, float* out, int64_t n, float* ws, void* stream);
int srx_mean_bwd(const float* x, const float* gscale, float* dx, int64_t n, void* stream);
/* sum of squared error -> used for PSNR (srgan/trainer.py:296) is srx_mse_fwd */

/* ------------------------------------------------- discriminator head + loss */
/* The end of a discriminator pass inside the GAN steps -- last Linear layer -> [Sigmoid] -> adversarial loss -- as ONE
 * forward and ONE backward launch (as separate operators: ~25 one-workgroup launches per discriminator update).
 *   SRX_HEAD_SRGAN_D  srgan/discriminator.py:67-68 + srgan/trainer.py:446-448: rows [0, n_first) = D(real), the rest =
 *                     D(fake); out[0] = BCELoss(sigmoid(z_real), 1) + BCELoss(sigmoid(z_fake), 0), out[1], out[2] the terms
 *   SRX_HEAD_SRGAN_G  srgan/trainer.py:456-457: out[1] = BCELoss(sigmoid(z), 1), out[0] = addend[0] + adv_weight * out[1]
 *   SRX_HEAD_ESRGAN_D esrgan/discriminator.py:75 + esrgan/trainer.py:451-453: out[0] = (BCEWithLogits(z_real - mean(z_fake), 1)
 *                     + BCEWithLogits(z_fake - mean(z_real), 0)) / 2, both means differentiated; out[4], out[5] the means
 *   SRX_HEAD_ESRGAN_G esrgan/trainer.py:468-469: out[1] = BCEWithLogits(z - shift[0], 1) (shift = mean(D(real)), no
 *                     gradient), out[0] = addend[0] + adv_weight * out[1]
 * hidden [B][J] is the OUTPUT of the hidden layer's LeakyReLU(slope); z = hidden w2 + b2.  zp [B] receives what the backward
 * needs (probabilities for the SRGAN modes, logits for the ESRGAN ones), out at least 8 floats; loss (may be NULL) receives
 * out[0] once more (a tensor of its own for the caller's autograd tape).  B <= 256.
 * Backward, given g[0] = d(loss)/d(out[0]) on the device: dpre [B][J] = gradient of the hidden layer's PRE-activation
 * (LeakyReLU backward applied), dw2 [J], db2 [1], db1 [J] = column sums of dpre (the hidden layer's bias gradient); any of
 * the three may be NULL; accumulate != 0 adds to them.  (The gradient of `addend` is g[0] itself.) */
enum { SRX_HEAD_SRGAN_D = 0, SRX_HEAD_SRGAN_G = 1, SRX_HEAD_ESRGAN_D = 2, SRX_HEAD_ESRGAN_G = 3 };
typedef struct {
  int32_t mode, B, J, n_first;
  float slope, adv_weight;
} srx_gan_head_t;
int srx_gan_head_fwd(const srx_gan_head_t* h, const float* hidden, const float* w2, const float* b2, const float* shift,
                     const float* addend, float* zp, float* out, float* loss, void* stream);
int srx_gan_head_bwd(const srx_gan_head_t* h, const float* hidden, const float* w2, const float* zp, const float* out,
                     const float* shift, const float* g, float* dpre, float* dw2, float* db2, float* db1, int accumulate,
                     void* stream);

/* --------------------------------------------------------------- optimiser */
/* torch.optim.Adam(lr, betas, eps, weight_decay=0) over one flat buffer
 * (srgan/trainer.py:171-185).  `step` (int64 on device) is incremented first;
 * `lr` is a float on the device so StepLR (srgan/trainer.py:186-195) can change
 * it without re-capturing a graph.  grad_scale multiplies g first (1/world_size
 * after an all-reduce SUM). */
int srx_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* lr, float beta1,
                  float beta2, float eps, float grad_scale, int64_t* step, void* stream);

/* Gradient guard: what torch.cuda.amp.GradScaler's skipped step (srgan/trainer.py:196,382-388) and
 * torch.nn.utils.clip_grad_norm_ do, decided on the device so that the pair of calls below replays
 * from a captured graph.  The state lives in DEVICE memory; the host zeroes it once. */
typedef struct {
  float   scale;    /* multiplies the gradient in srx_adam_step_guarded, on top of grad_scale */
  int32_t skip;     /* 1: this step is skipped */
  float   norm;     /* l2 norm of grad_scale * g of the last call (fp64 sum, rounded once; +inf / NaN
                       when g is not finite) */
  int32_t reserved;
  int64_t skipped;  /* running count of skipped steps */
  int64_t clipped;  /* running count of steps with scale < 1 (a skipped step has scale 0: it counts) */
} srx_grad_guard_t;

/* One streaming read of g[0..n) and a one-workgroup finalise.  Squares and sums are fp64 throughout,
 * so the sum is finite exactly when every g[i] is; the order of the sum is a fixed function of n
 * (no floating-point atomics): two calls on the same buffer write the same bits.
 *   norm  = |grad_scale| * sqrt(sum g^2)
 *   skip  = skip_nonfinite && the sum is not finite
 *   scale = 0 when skip; else min(1, max_norm / (norm + 1e-6)) for a finite max_norm > 0 (NaN stays
 *           NaN, as in clip_grad_norm_ with error_if_nonfinite=False); else 1
 * max_norm <= 0 or +inf: no clipping.  ws: srx_grad_guard_ws_bytes(n) bytes, 8-byte aligned, needs
 * no initialisation; g 16-byte, state 8-byte aligned. */
size_t srx_grad_guard_ws_bytes(int64_t n);
int srx_grad_guard(const float* g, int64_t n, float grad_scale, float max_norm, int skip_nonfinite,
                   void* ws, size_t ws_bytes, srx_grad_guard_t* state, void* stream);
/* srx_adam_step behind the guard's decision, read from `state` on the device: with state->skip set
 * neither *step nor p, m, v change; otherwise g is multiplied by grad_scale * state->scale (one fp32
 * product: with scale == 1 the results are srx_adam_step's bit for bit). */
int srx_adam_step_guarded(float* p, const float* g, float* m, float* v, int64_t n, const float* lr, float beta1,
                          float beta2, float eps, float grad_scale, int64_t* step,
                          const srx_grad_guard_t* state, void* stream);

/* Exponential moving average of a flat parameter buffer, in place on `ema` (Real-ESRGAN's
 * ema_decay):  ema[i] = decay * ema[i] + one_minus_decay * p[i]  for i in [0, n), fp32, two products
 * and one sum, each rounded once (never contracted into an fma).  The caller forms one_minus_decay in
 * double and rounds it once.  decay == 0 copies p bit for bit.  One launch, 16-byte accesses.
 * Refused: null pointers, n <= 0, ema or p not 16-byte aligned, ema == p, a decay outside [0, 1) or
 * not finite, a one_minus_decay outside (0, 1] or not finite. */
int srx_ema_update(float* ema, const float* p, int64_t n, float decay, float one_minus_decay, void* stream);

/* Spectral normalisation of a weight W [rows][cols] (a conv's [Cout][Cin * KH * KW]), the semantics of
 * torch.nn.utils.spectral_norm with n_power_iterations = 1 and eps = 1e-12.
 *   train != 0:  v <- W^T u / max(|W^T u|, eps);  u <- W v / max(|W v|, eps)   (u, v updated in place)
 *   always:      sigma = u . (W v);  W_sn = W / sigma
 * uv_keep (optional, roundup(rows, 4) + cols floats): the u and v this call used for sigma, for the
 * backward -- u and v themselves move on with the next training call.  The training call reads W three
 * times and writes W_sn once.  Grids and reduction trees are fixed functions of (rows, cols) and there
 * are no floating-point atomics: the same inputs give the same bits.
 * Refused: null pointers, W / v / W_sn / ws / uv_keep not 16-byte aligned, cols not a multiple of 4,
 * rows * cols >= 2^31, ws shorter than srx_spectral_norm_ws_floats(rows, cols). */
size_t srx_spectral_norm_ws_floats(int rows, int cols);
int srx_spectral_norm_fwd(const float* W, float* u, float* v, float* W_sn, float* sigma, float* uv_keep, int rows,
                          int cols, int train, float* ws, size_t ws_floats, void* stream);
/* Its backward: with G = dL/dW_sn and W_sn = W / sigma (formed on the fly from W, so the caller's W_sn
 * buffer may have been overwritten since),  dW (+)= (G - <G, W_sn> u v^T) / sigma;  u, v, sigma: those
 * of the forward (uv_keep).  accumulate != 0 adds to dW.  Same refusals and the same workspace size. */
int srx_spectral_norm_bwd(const float* G, const float* W, const float* u, const float* v, const float* sigma,
                          float* dW, int accumulate, int rows, int cols, float* ws, size_t ws_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SRX_H */
