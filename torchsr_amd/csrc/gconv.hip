// Convolution as a gather-GEMM on the fp32 matrix cores of gfx950 (MI355X).
//
//   out[opix(m)][n] = epilogue( sum_k A(m,k) * B[n][k] ),   A(m,k) = in[ipix(m)+tap(k)][chan(k)]  (0 outside)
//
// One kernel serves nn.Conv2d forward (any kernel size / stride / padding), the
// data gradient (run per stride-parity class with flipped taps, so stride-2
// layers do no wasted work) and -- through in_shuffle / out_shuffle addressing --
// the PixelShuffle(2) of the SRGAN sub-pixel layer (srgan/residual.py:27-28).
// The weight gradient dW[n][k] = sum_m dy[m][n] A(m,k) has kernels of its own (wgrad.hip); convpack.hip packs the weights.
//
// Data layout: activations NHWC fp32 (channel stride multiple of 4), packed
// weights [N_pad][K_pad] with K = (tap, channel) contiguous, so both MFMA
// operands are "k-contiguous rows" and are staged into XOR-swizzled LDS rows of
// 32 floats read back with conflict-free ds_read_b128.
// MFMA: v_mfma_f32_32x32x2_f32 (exact fp32, 64 FLOP/clk/SIMD = 157.3 TFLOP/s chip peak), plus
// v_mfma_f32_16x16x4_f32 for the 16 extra rows of the 144-row tiles and v_mfma_f32_32x32x16_bf16 for
// the bf16-product mode (srx_conv2d_t::precision).
#include "conv_host.h"
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

namespace {

struct GArgs {
  const float* in; const float* w; const float* bias; float* out; float* part;
  int N, Hi, Wi, Ci;
  int Hm, Wm, M, HmWm;
  float inv_HmWm, inv_Wm;
  int in_stride, nth, ntw, dh0, dw0, Ck, K, Kp;
  int Cn, Cs;
  int Ho, Wo, Co;
  int out_stride, oh_off, ow_off;
  int out_shuffle, in_shuffle;
  // up != 0: the conv reads a nearest-neighbour x2 upsampling of `in` that is never materialised (esrgan/generator.py:73,76:
  // F.interpolate(scale_factor=2) feeding a conv).  Hi, Wi are the UPSAMPLED extents (bounds of the taps); the pixel
  // (ih, iw) is fetched from (ih >> 1, iw >> 1) of the stored [N][Hi/2][Wi/2][Ci] tensor.
  int up;
  int act; float slope;
  int linear_out;
  int mtiles;
  // work decomposition: workgroups [0, full_tiles) each own one whole output tile; the remaining
  // (tail) tiles are cut tail_split ways along K so that the last, partially filled "round" of the
  // chip still keeps every CU busy; their raw partial tiles go to `ws` and tail_fixup_kernel
  // finishes them (sum, bias, activation, BatchNorm partials).
  int kchunks, kc_per_split, full_tiles, tail_split;
  float* ws;
  // sizes of the `in` and `w` buffers: both are read through raw buffer descriptors, whose range
  // check returns 0 for the padding taps (no branch, no select, statically countable loads).  The input descriptor is based
  // at the first byte the TILE can touch (round 4: a 64-bit base per workgroup, 32-bit offsets inside it), so a call is
  // not capped at 4 GiB of input; `big`: M >= 2^24, pixel indices are split by exact integer division instead of the float one
  size_t in_bytes;
  unsigned w_bytes;
  int big;
  unsigned in_margin;  // bytes the most negative tap reaches in front of a row's centre pixel
  // epilogue addend, laid out like `out` (null: none): `out` itself when a data gradient is summed into a
  // shared dense-block buffer, or the skip input of a residual block in eval mode (BatchNorm folded into the
  // conv, `x + conv(...)` in one kernel).  Linear outputs only.
  const float* add;
  float oscale;  // applied to act(acc + bias) before the addend (conv5 * 0.2 + x of the dense block); 1 otherwise
  // The addend may have a row stride of its own (add_ld floats; linear outputs only -- otherwise it equals Co), may cover
  // only the leading columns [0, add_hi), and is scaled by ascale: out = act(acc + bias) * oscale + add * ascale.  ESRGAN's
  // trunk keeps every dense block's input in the first 64 of a 192-channel buffer (stride 192) while block gradients
  // are dense 64-channel tensors, and the gradient entering a block is added to the block's input gradient there.
  int add_ld, add_hi;
  float ascale;
  // mask (null: none): the OUTPUT of the activation that produced this conv's input, laid out like `out`.  The data
  // gradient is multiplied by that activation's derivative on its way out, v * (mask[i] > 0 ? 1 : mask_slope), for
  // the output columns [mask_lo, mask_hi) -- the ReLU / LeakyReLU backward of the layer below without a pass of its
  // own.  Applied after the addend: in ESRGAN's dense block the convs' input gradients accumulate in one shared
  // buffer and the conv that completes a 32-channel slice also applies that slice's LeakyReLU mask.
  const float* mask;
  float mask_slope;
  int mask_lo, mask_hi;
  // PR = 2 (bf16 STORAGE, round 5): `in` and `w` hold bf16 values -- described to the kernel as fp32 tensors of half the
  // channel count, so every gather offset below is the fp32 code's -- and `out` / `mask` are bf16 tensors when these are set
  int out16, mask16;
};

constexpr int INVALID = -20000;  // coordinate that fails every bounds check

// ---------------------------------------------------------------------------
// forward / data-gradient gather-GEMM.  256 threads = 4 waves, wave tile WMxWN.
// ---------------------------------------------------------------------------
// KS > 1: the k-chunks of the tile are dealt round-robin to KS groups of waves (each group owns a
// private pair of LDS staging buffers and covers the whole BM x BN tile); the groups' accumulators are
// folded through LDS at the end.  Used when a launch has fewer tiles than CUs (e.g. the 16x24x24
// residual convs: 144 tiles): it halves the serial chunk chain per wave and puts two waves on a SIMD.
//
// XR = 16: the tile carries 16 more rows (BM + 16 = 144), multiplied on v_mfma_f32_16x16x4_f32 as BN/16
// blocks of 16x16 by the first BN/16 waves.  The SRGAN shapes have M = 2304 * 4^j pixels: with 144-row
// tiles every layer cuts into a power-of-two number of tiles, i.e. whole rounds of the 256 CUs, where
// 128-row tiles leave 12-25 % of a round idle and need the K-split fix-up pass.
//
// PR = 1: bf16 products, fp32 accumulation (srx_conv2d_t::precision).  Global memory stays fp32; a chunk's
// 32 k-values are rounded to bf16 when they are written to LDS (64-byte rows) and multiplied by two
// v_mfma_f32_32x32x16_bf16 per 32x32 block instead of sixteen fp32 MFMAs -- the loop is then bound by the
// L2 -> LDS stream, not by the matrix pipe.
// BIG = 1 (round 4): calls above 2^24 pixels / 4 GiB of input (whole-frame inference).  The input descriptor is based at the
// first byte the TILE can touch -- a 64-bit base per workgroup, 32-bit offsets inside it -- and pixel indices are split by
// exact integer division.  A separate instantiation: with the per-tile base in the common kernel the SRGAN step lost 1 %
// (same-box A/B, 8.87 vs 8.97 ms), so BIG = 0 is the code of round 3 to the letter.
template <int BM, int BN, int WM, int WN, int KS, int XR, int PR, int UP = 0, int BIG = 0>
__device__ __forceinline__ void gconv_body(const GArgs& a, const int bid) {
  static_assert(XR == 0 || (XR == 16 && KS == 1), "extra rows: 16, without the in-workgroup K split");
  static_assert(PR == 0 || XR == 0, "the 16-row extension is fp32 only");
  constexpr bool H16 = PR == 1 || PR == 3;  // 16-bit products of fp32-stored tensors: bf16 (PR = 1) or fp16 (PR = 3)
  constexpr int BKL = H16 ? BK / 2 : BK;  // floats per LDS row
  constexpr int NS = H16 ? 2 : 4;         // MFMA sub-steps per chunk
  constexpr int BMT = BM + XR;  // rows of the tile
  constexpr int TM = WM / 32, TN = WN / 32;
  constexpr int WAVES_N = BN / WN;
  constexpr int WAVES_M = BM / WM;
  constexpr int GT = WAVES_M * WAVES_N * 64;  // threads of one k-group
  constexpr int NT = GT * KS;                 // 256 or 512 threads: the big tiles run 8 waves so that every
                                              // SIMD holds two and one's MFMAs cover the other's loads/barriers
  static_assert(NT == 256 || NT == 512, "4 or 8 waves per workgroup");
  constexpr int RPP = GT / 8;                 // tile rows staged per pass (8 threads x float4 = one 128-byte row)
  constexpr int RA = (BMT + RPP - 1) / RPP, RB = BN / RPP;  // the last A pass may be partly past the tile
  static_assert(RA >= 1 && RB >= 1, "tile too small for the thread count");
  static_assert(XR == 0 || BN / 16 <= GT / 64, "one extra 16x16 block per wave at most");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // wave-uniform quantities are forced into SGPRs (readfirstlane): loop control then compiles to
  // scalar branches instead of exec-mask juggling around the MFMA blocks
  const int ks = KS == 1 ? 0 : srx_uniform(threadIdx.x / GT);  // k-group of this wave (groups are contiguous)
  const int tid = threadIdx.x - ks * GT, lane = tid & 63, wave = srx_uniform(tid >> 6);
  constexpr int RING = 3;  // LDS chunk buffers per k-group
  float* sA = reinterpret_cast<float*>(smem) + ks * RING * (BMT + BN) * BKL;
  float* sB = sA + RING * BMT * BKL;
  int2* ktab = reinterpret_cast<int2*>(reinterpret_cast<float*>(smem) + KS * RING * (BMT + BN) * BKL);
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  int tile = bid, kc_beg = 0, kc_end = a.kchunks;
  bool raw = false;
  float* slab = nullptr;
  if (bid >= a.full_tiles) {
    const int t = bid - a.full_tiles;
    tile = a.full_tiles + t / a.tail_split;
    if (a.tail_split > 1) {
      kc_beg = (t % a.tail_split) * a.kc_per_split;
      kc_end = min(a.kchunks, kc_beg + a.kc_per_split);
      raw = true;
      slab = a.ws + (size_t)t * (BMT * BN);
    }
  }
  tile = srx_uniform(tile); kc_beg = srx_uniform(kc_beg); kc_end = srx_uniform(kc_end);
  const int nt = srx_uniform(tile / a.mtiles), mt = tile - nt * a.mtiles;
  const int m0 = mt * BMT, n0 = nt * BN;
  const int q = tid & 7, r0 = tid >> 3;
  auto split_row = [&](int m, int& n, int& mh, int& mw) {  // m -> (image, row, column) of the M grid
    if constexpr (BIG) {  // exact: the float reciprocal trick holds below 2^24 only
      n = m / a.HmWm;
      const int rem = m - n * a.HmWm;
      mh = rem / a.Wm;
      mw = rem - mh * a.Wm;
    } else {
      int rem;
      srx_divmod(m, a.HmWm, a.inv_HmWm, n, rem);
      srx_divmod(rem, a.Wm, a.inv_Wm, mh, mw);
    }
  };
  // byte offset of row m's centre pixel in the input tensor (monotonic in m)
  auto centre = [&](int n, int ih0, int iw0) -> size_t {
    return 4 * (UP ? (size_t)n * (a.Hi >> 1) * (a.Wi >> 1) * a.Ci
                   : a.in_shuffle ? (((size_t)n * 2 * a.Hi + 2 * ih0) * (2 * a.Wi) + 2 * iw0) * a.Ci
                                  : (((size_t)n * a.Hi + ih0) * a.Wi + iw0) * a.Ci);
  };
  size_t tbase = 0;  // BIG: first byte this tile can touch: its first row's centre less the reach of the most negative tap
  if constexpr (BIG) {
    int n, mh, mw;
    split_row(min(m0, a.M - 1), n, mh, mw);
    const size_t c0 = centre(n, mh * a.in_stride, mw * a.in_stride);
    tbase = c0 > a.in_margin ? c0 - a.in_margin : 0;
    const unsigned tb_in_lo = (unsigned)srx_uniform((int)(unsigned)(tbase & 0xffffffffu));
    const unsigned tb_in_hi = (unsigned)srx_uniform((int)(unsigned)(tbase >> 32));
    tbase = ((size_t)tb_in_hi << 32) | tb_in_lo;
  }
  const size_t in_left = a.in_bytes - tbase;
  const __amdgpu_buffer_rsrc_t rin = BIG ? srx_rsrc(reinterpret_cast<const char*>(a.in) + tbase, in_left > 0xfffffff0ull ? 0xfffffff0u : (unsigned)in_left)
                                         : srx_rsrc(a.in, (unsigned)a.in_bytes);
  const __amdgpu_buffer_rsrc_t rw = srx_rsrc(a.w, a.w_bytes);

  // ---- k table: (dh, dw) and linear input offset for every float4 of K in range
  for (int e = kc_beg * 8 + (int)threadIdx.x; e < kc_end * 8; e += NT) {
    const int k = 4 * e;
    int2 ent;
    if (k < a.K) {
      const int tap = k / a.Ck, c = k - tap * a.Ck;
      const int th = tap / a.ntw, tw = tap - th * a.ntw;
      const int dh = a.dh0 + th, dw = a.dw0 + tw;
      int koff;
      if (UP) {
        koff = c;  // the pixel part of the offset depends on the row's parity: added per load (gload)
      } else if (a.in_shuffle) {
        const int ij = c / a.in_shuffle, cc = c - ij * a.in_shuffle;
        koff = ((2 * dh + (ij >> 1)) * (2 * a.Wi) + 2 * dw + (ij & 1)) * a.Ci + cc;
      } else {
        koff = (dh * a.Wi + dw) * a.Ci + c;
      }
      ent.x = (int)((unsigned)(dh & 0xffff) | ((unsigned)dw << 16));
      ent.y = koff * 4;  // bytes
    } else {
      ent.x = (INVALID & 0xffff);
      ent.y = 0;
    }
    ktab[e - kc_beg * 8] = ent;
  }

  // ---- per-thread rows of the A tile (fixed for the whole k loop)
  int rih[RA], riw[RA];
  unsigned rbase[RA];  // byte offset of the row's centre pixel
#pragma unroll
  for (int p = 0; p < RA; ++p) {
    const int m = m0 + r0 + RPP * p;
    if (m < a.M && r0 + RPP * p < BMT) {
      int n, mh, mw;
      split_row(m, n, mh, mw);
      const int ih0 = mh * a.in_stride, iw0 = mw * a.in_stride;
      rih[p] = ih0;
      riw[p] = iw0;
      if constexpr (BIG) {
        rbase[p] = (unsigned)(centre(n, ih0, iw0) - tbase);  // (relative to the tile's base: a tile spans a few image rows)
      } else {
        rbase[p] = 4u * (unsigned)(UP ? n * (a.Hi >> 1) * (a.Wi >> 1) * a.Ci
                                   : a.in_shuffle ? ((n * 2 * a.Hi + 2 * ih0) * (2 * a.Wi) + 2 * iw0) * a.Ci
                                                  : ((n * a.Hi + ih0) * a.Wi + iw0) * a.Ci);
      }
    } else {
      rih[p] = INVALID; riw[p] = 0; rbase[p] = 0;
    }
  }
  unsigned wvoff[RB];
#pragma unroll
  for (int p = 0; p < RB; ++p) wvoff[p] = 4u * ((unsigned)(n0 + r0 + RPP * p) * (unsigned)a.Kp + q * 4);
  __syncthreads();

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // Three register stages: while chunk k is multiplied out of LDS, chunk k+1 is being written to the
  // ring and the loads of chunks k+2 and k+3 are in flight (a load has two full steps to arrive).  With
  // one workgroup per CU a single stage leaves ~0.5 us of L2/HBM latency exposed per chunk.
  f32x4 ra0[RA], rb0[RB], ra1[RA], rb1[RB], ra2[RA], rb2[RB];
  // Every step issues the same RA + RB loads -- past the end of the k range they are pointed out of
  // range and cost nothing -- so that the compiler can count outstanding loads exactly (s_waitcnt
  // vmcnt(N) for the older register stage only) instead of draining both stages at every step.
  auto gload = [&](int kc, f32x4 (&ra)[RA], f32x4 (&rb)[RB]) {
    const bool live = kc < kc_end;  // wave-uniform
    const int2 kt = ktab[(live ? kc - kc_beg : 0) * 8 + q];
    const int dh = (int)(short)(kt.x & 0xffff), dw = kt.x >> 16;
    if (UP) {  // compile time: a run-time test here, even a scalar one, cost the fp32 step 1.2 % (same-box A/B)
#pragma unroll
      for (int p = 0; p < RA; ++p) {
        const int ih = rih[p] + dh, iw = riw[p] + dw;
        const bool ok = live && ((unsigned)ih < (unsigned)a.Hi) && ((unsigned)iw < (unsigned)a.Wi);
        const unsigned pix = 4u * (unsigned)(((ih >> 1) * (a.Wi >> 1) + (iw >> 1)) * a.Ci);  // source pixel of the upsampled one
        ra[p] = srx_bload(rin, ok ? rbase[p] + pix + (unsigned)kt.y : 0xffffffffu, 0);
      }
    } else {
#pragma unroll
      for (int p = 0; p < RA; ++p) {
        const int ih = rih[p] + dh, iw = riw[p] + dw;
        const bool ok = live && ((unsigned)ih < (unsigned)a.Hi) && ((unsigned)iw < (unsigned)a.Wi);
        ra[p] = srx_bload(rin, ok ? rbase[p] + (unsigned)kt.y : 0xffffffffu, 0);  // out of range reads 0
      }
    }
#pragma unroll
    for (int p = 0; p < RB; ++p)
      rb[p] = srx_bload(rw, live ? wvoff[p] : 0xffffffffu, (unsigned)srx_uniform(live ? kc * (BK * 4) : 0));
  };
  // fp32: 16-byte quad q of the row at quad q ^ ((row>>1)&7).  bf16: the quad shrinks to 8 bytes; quads 2g, 2g+1
  // form the 16-byte group g (k = 8g..8g+7, one MFMA operand), stored at group g ^ ((row>>2)&3).
  const int wchunk = H16 ? (((q >> 1) ^ ((r0 >> 2) & 3)) * 4 + (q & 1) * 2) : (q ^ ((r0 >> 1) & 7)) * 4;
  auto put = [&](float* dst, const f32x4& v) {
    if (PR == 3) {  // fp16 products (inference, the 3-channel input conv): the same layout, rounded to fp16
      typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
      const f16x2 lo = {(_Float16)v[0], (_Float16)v[1]}, hi = {(_Float16)v[2], (_Float16)v[3]};
      *reinterpret_cast<uint2*>(dst) = make_uint2(__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi));
    } else if (PR == 1) {
      typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
      const bf16x2 lo = {(__bf16)v[0], (__bf16)v[1]}, hi = {(__bf16)v[2], (__bf16)v[3]};
      *reinterpret_cast<uint2*>(dst) = make_uint2(__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi));
    } else {
      *reinterpret_cast<f32x4*>(dst) = v;
    }
  };
  auto swrite = [&](int buf, const f32x4 (&ra)[RA], const f32x4 (&rb)[RB]) {
    float* dA = sA + buf * BMT * BKL;
    float* dB = sB + buf * BN * BKL;
#pragma unroll
    for (int p = 0; p < RA; ++p)
      if (RPP * (p + 1) <= BMT || r0 + RPP * p < BMT)  // (compile-time true except in a partial last pass)
        put(dA + (r0 + RPP * p) * BKL + wchunk, ra[p]);
#pragma unroll
    for (int p = 0; p < RB; ++p) put(dB + (r0 + RPP * p) * BKL + wchunk, rb[p]);
  };

  const int h = lane >> 5, l31 = lane & 31;
  const int xr = H16 ? (l31 >> 2) & 3 : (l31 >> 1) & 7;
  const int arow = (wm * WM + l31) * BKL, brow = (wn * WN + l31) * BKL;
  // extra 16 rows: wave w < BN/16 owns the 16x16 block of columns 16w..16w+15
  //   v_mfma_f32_16x16x4_f32: A[i = l&15][k = l>>4], B[k = l>>4][j = l&15], D: col = l&15, row = 4(l>>4) + reg
  const bool has_x = XR > 0 && wave < BN / 16;
  const int xi = lane & 15, xg = lane >> 4;
  const int xra = BM + xi, xrb = 16 * wave + xi;  // LDS rows of this lane's A / B fragments
  f32x4 accx = {0.f, 0.f, 0.f, 0.f};
  // ---- the pipelined k loop -----------------------------------------------------------------
  // LDS holds a ring of three chunk buffers.  In step k a wave
  //   1. writes chunk k+1 (in registers since the previous step) into ring slot (k+1) % 3,
  //   2. requests chunk k+3 from global memory into the register stage that just became free (three
  //      stages: a load has two full steps to arrive before it is written to LDS),
  //   3. multiplies chunk k out of slot k % 3, with the step's ONE barrier in the middle.
  // Chunk k+1 is therefore complete in LDS half a step before anyone needs it: the barrier has slack
  // for skew between waves instead of standing between the last MFMA of a chunk and the first LDS
  // read of the next, and that first read (fragment 0 of chunk k+1) is issued under the last MFMAs of
  // chunk k.  Slot (k+1) % 3 was last read in step k-2; the barrier of step k-1 separates the two.
  // (With two slots the write had to wait for the end of the step and every chunk boundary cost the
  // matrix pipe a barrier + a write + a read latency: 28 % idle with one workgroup per CU.)
  f32x4 af[2][TM], bf[2][TN];  // fragment register sets: step s+1 is read while step s is multiplied
  auto frag = [&](int slot, int s, int set) {
    const float* cA = sA + slot * BMT * BKL + arow;
    const float* cB = sB + slot * BN * BKL + brow;
    const int ch = ((2 * s + h) ^ xr) * 4;  // fp32: quad of 4 k;  bf16: group of 8 k (one 32x32x16 operand)
#pragma unroll
    for (int i = 0; i < TM; ++i) af[set][i] = *reinterpret_cast<const f32x4*>(cA + i * 32 * BKL + ch);
#pragma unroll
    for (int j = 0; j < TN; ++j) bf[set][j] = *reinterpret_cast<const f32x4*>(cB + j * 32 * BKL + ch);
  };
  auto mma = [&](int set) {
    __builtin_amdgcn_s_setprio(1);
    if (PR == 3) {
      typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, af[set][i]),
                                                             __builtin_bit_cast(f16x8, bf[set][j]), acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      return;
    }
    if (PR) {  // (PR = 2: a 16-byte quad of the stored tensor IS eight bf16 k-values, one MFMA operand)
      typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[set][i]),
                                                              __builtin_bit_cast(bf16x8, bf[set][j]), acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[set][i][e], bf[set][j][e], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };
  auto extra = [&](int slot) {  // each b128 holds k = 4Q..4Q+3 of one row; MFMA e of read u contracts k = {4(g + 4u) + e}
    const float* xA = sA + slot * BMT * BKL + xra * BKL;
    const float* xB = sB + slot * BN * BKL + xrb * BKL;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const f32x4 fa = *reinterpret_cast<const f32x4*>(xA + (((xg + 4 * u) ^ ((xra >> 1) & 7)) * 4));
      const f32x4 fb = *reinterpret_cast<const f32x4*>(xB + (((xg + 4 * u) ^ ((xrb >> 1) & 7)) * 4));
#pragma unroll
      for (int e = 0; e < 4; ++e) accx = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[e], fb[e], accx, 0, 0, 0);
    }
  };
  // one step; `slot` = ring slot of chunk kc, fragment 0 of which already sits in register set 0
  auto step = [&](int kc, int slot, f32x4 (&ra_next)[RA], f32x4 (&rb_next)[RB], f32x4 (&ra_free)[RA], f32x4 (&rb_free)[RB]) {
    const int nslot = slot == 2 ? 0 : slot + 1;
    swrite(nslot, ra_next, rb_next);          // chunk kc + KS (zeros past the end of the range: never multiplied)
    gload(kc + 3 * KS, ra_free, rb_free);
    const bool live = kc < kc_end;            // wave-uniform
    if (NS == 2) {  // bf16: two MFMA sub-steps per chunk
      frag(slot, 1, 1);
      if (live) mma(0);
      __syncthreads();
      frag(nslot, 0, 0);
      if (live) mma(1);
      return;
    }
    frag(slot, 1, 1);
    if (live) mma(0);
    frag(slot, 2, 0);
    if (live) mma(1);
    __syncthreads();
    frag(slot, 3, 1);
    if (live) mma(0);
    frag(nslot, 0, 0);
    if (XR > 0 && has_x && live) extra(slot);
    if (live) mma(1);
  };

  // this group's chunks: kc_beg + ks, + KS, ...; every group runs the same number of steps (barriers)
  const int c0 = kc_beg + ks;
  const int nsteps = (kc_end - kc_beg + KS - 1) / KS;
  gload(c0, ra0, rb0);
  gload(c0 + KS, ra1, rb1);
  gload(c0 + 2 * KS, ra2, rb2);
  swrite(0, ra0, rb0);
  __syncthreads();
  frag(0, 0, 0);
  // three steps per trip (ring slots and register stages rotate statically); all three run even past
  // the end of the range: an early exit would make the loop's load count path-dependent and cost the
  // exact vmcnt waits
  for (int j = 0; j < nsteps; j += 3) {
    const int kc = c0 + j * KS;
    step(kc, 0, ra1, rb1, ra0, rb0);
    step(kc + KS, 1, ra2, rb2, ra1, rb1);
    step(kc + 2 * KS, 2, ra0, rb0, ra2, rb2);
  }
  __syncthreads();  // the ring is reused below (fold / statistics)

  if (KS > 1) {  // fold the k-groups' accumulators into group 0 (staging buffers are free now)
    float* fold = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int g = 1; g < KS; ++g) {
      if (ks == g) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int jj = 0; jj < TN; ++jj)
#pragma unroll
            for (int r = 0; r < 16; ++r) fold[((wave * TM * TN + i * TN + jj) * 16 + r) * 64 + lane] = acc[i][jj][r];
      }
      __syncthreads();
      if (ks == 0) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int jj = 0; jj < TN; ++jj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][jj][r] += fold[((wave * TM * TN + i * TN + jj) * 16 + r) * 64 + lane];
      }
      __syncthreads();
    }
  }
  const bool lead = (ks == 0);

  // ------------------------------------------------------------- epilogue
  // accumulator map (32x32 MFMA): col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
  if (raw) {  // tile-local [BM][BN] partial; each half wave writes 128 contiguous bytes
    if (!lead) return;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          slab[row * BN + wn * WN + j * 32 + l31] = acc[i][j][r];
        }
    if (XR > 0 && has_x) {
#pragma unroll
      for (int r = 0; r < 4; ++r) slab[(BM + 4 * xg + r) * BN + 16 * wave + xi] = accx[r];
    }
    return;
  }
  // Straight-line epilogue: the activation is a select on a host-prepared slope (none 1, ReLU 0), rows
  // past M and padding columns are stored through a descriptor at an out-of-range offset (dropped by
  // the hardware) instead of being branched around -- per-element branches used to cost more than
  // the arithmetic.
  auto out_elem = [&](int m) -> size_t {  // element offset of output row m
    if (a.linear_out) return (size_t)m * a.Co;
    int n, mh, mw;
    split_row(m, n, mh, mw);
    const int oh = mh * a.out_stride + a.oh_off, ow = mw * a.out_stride + a.ow_off;
    if constexpr (BIG) return (((size_t)n * a.Ho + oh) * a.Wo + ow) * a.Co;
    else return ((size_t)(n * a.Ho + oh) * a.Wo + ow) * a.Co;
  };
  // descriptor based at the tile's first row: offsets inside a tile are small and never negative
  // (output rows are laid out in increasing m), so 32 bits are enough whatever the tensor size
  const size_t tile_base = out_elem(m0);
  const unsigned tb_lo = (unsigned)srx_uniform((int)(unsigned)(tile_base & 0xffffffffu));
  const unsigned tb_hi = (unsigned)srx_uniform((int)(unsigned)(tile_base >> 32));
  // (PR = 2: bf16 outputs / masks -- offsets below stay 4 x the element index and are halved at the access)
  // (a bf16-storage launch's mask is always bf16; its output type picks one of two copies of the epilogue below)
  const bool out16 = PR == 2 && a.out16;
  constexpr bool mask16 = PR == 2;
  const __amdgpu_buffer_rsrc_t rout = srx_rsrc(reinterpret_cast<char*>(a.out) + ((((size_t)tb_hi << 32) | tb_lo) << (out16 ? 1 : 2)), 0xfffffff0u);
  // (the addend's tile base differs from the output's when it has its own row stride -- linear outputs only; built
  // inside the add-mode paths so that the other epilogues do not carry its scalars)
  auto make_radd = [&]() {
    const size_t add_base = a.linear_out ? (size_t)m0 * a.add_ld : tile_base;
    const unsigned ab_lo = (unsigned)srx_uniform((int)(unsigned)(add_base & 0xffffffffu));
    const unsigned ab_hi = (unsigned)srx_uniform((int)(unsigned)(add_base >> 32));
    return srx_rsrc(a.add + (((size_t)ab_hi << 32) | ab_lo), 0xfffffff0u);
  };
  const __amdgpu_buffer_rsrc_t rmask = srx_rsrc(reinterpret_cast<const char*>(a.mask ? a.mask : a.out) +
                                                    ((((size_t)tb_hi << 32) | tb_lo) << (mask16 ? 1 : 2)), 0xfffffff0u);

  // Row offsets of a pixel-mapped output (strided data gradients, PixelShuffle): ONE thread per tile row works out the row's byte
  // offset (two divisions by a float multiply, the output pixel, ~25 VALU instructions) and parks it in LDS; the epilogue below reads
  // its 16 rows back with four ds_read_b128.  Round 6: every lane used to recompute all 16 of its rows -- 400 VALU instructions per
  // wave and 32-row block, i.e. matrix time (the f32 MFMA runs on the vector ALUs, tools/probe/mfma_valu.hip), 70 % of the launch on
  // the short-K parity classes of the discriminator's first stride-2 data gradient (PMC).  The table sits at the end of the staging
  // ring (free since the barrier behind the k loop; the fold and the statistics use its start).
  unsigned* rowtab = reinterpret_cast<unsigned*>(reinterpret_cast<float*>(smem) + KS * RING * (BMT + BN) * BKL) - ((BMT + 3) & ~3);
  if (!a.linear_out) {
    for (int rr = (int)threadIdx.x; rr < BMT; rr += NT) {
      const int m = m0 + rr;
      rowtab[rr] = m < a.M ? 4u * (unsigned)(out_elem(m) - tile_base) : 4u * (unsigned)(out_elem(m0) - tile_base);
    }
    __syncthreads();
  }
  float bv[TN];
  unsigned ocol[TN];  // byte offset of the column inside its output row
  bool cok[TN];       // this lane stores the column
  bool cmk[TN];       // ... and the column takes the activation mask
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn * WN + j * 32 + l31;
    cmk[j] = col >= a.mask_lo && col < a.mask_hi;
    int bidx = col, oc = col;
    if (a.out_shuffle) {
      const int ij = col / a.out_shuffle, cc = col - ij * a.out_shuffle;
      bidx = cc * 4 + ij;
      oc = (((ij >> 1) * a.Wo) + (ij & 1)) * a.Co + cc;  // offset inside the 2x2 output block
    }
    ocol[j] = 4u * (unsigned)oc;
    cok[j] = lead && col < a.Cs;
    bv[j] = (a.bias && col < a.Cn) ? a.bias[bidx] : 0.f;
  }
  float csum[TN], csq[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) { csum[j] = 0.f; csq[j] = 0.f; }

  auto store_tile = [&](auto linear, auto accum, auto o16) {  // one copy per addressing / epilogue mode (bit 0: addend, bit 1: mask), chosen by ONE branch
    constexpr int MODE = decltype(accum)::value;
    constexpr bool OUT16 = decltype(o16)::value;
    __amdgpu_buffer_rsrc_t radd = rout;
    bool cak[TN];  // the column takes the addend
    if constexpr ((MODE & 1) != 0) {
      radd = make_radd();
#pragma unroll
      for (int j = 0; j < TN; ++j) cak[j] = n0 + wn * WN + j * 32 + l31 < a.add_hi;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      // Addend / mask values of the whole 32-row block are requested BEFORE the first store: vmcnt retires in issue
      // order, so a load issued behind a store cannot be consumed until that store has landed, and an epilogue that
      // alternates load -> store per element pays a full memory round trip for each of its 16 x TN elements
      // (+4.5 us on a 15 us dense-block data gradient).
      unsigned offs[16][TN];
      float av[MODE & 1 ? 16 : 1][TN], mv[MODE & 2 ? 16 : 1][TN];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const bool mok = m < a.M;
        const unsigned rowoff = decltype(linear)::value ? 4u * (unsigned)((m - m0) * a.Co) : rowtab[m - m0];
        const unsigned arow = decltype(linear)::value ? 4u * (unsigned)((m - m0) * a.add_ld) : rowoff;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const unsigned off = (mok && cok[j]) ? rowoff + ocol[j] : 0xffffffffu;
          offs[r][j] = off;
          // (a column past add_hi reads nothing -- an out-of-range offset returns 0)
          if (MODE & 1)
            av[r][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                radd, (int)((mok && cok[j] && cak[j]) ? arow + ocol[j] : 0xffffffffu), 0, 0));
          // (a column outside the mask range reads nothing: its offset is pointed out of range)
          if (MODE & 2) {
            const unsigned moff = cmk[j] ? off : 0xffffffffu;
            if (mask16)
              mv[r][j] = __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_raw_buffer_load_b16(rmask, (int)(moff == 0xffffffffu ? moff : moff >> 1), 0, 0) << 16);
            else
              mv[r][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rmask, (int)moff, 0, 0));
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const bool mok = m < a.M;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          float v = acc[i][j][r] + bv[j];
          const float vs = mok ? v : 0.f;
          csum[j] += vs;
          csq[j] += vs * vs;
          v = v > 0.f ? v : v * a.slope;
          if (MODE & 1) v = v * a.oscale + av[r][j] * a.ascale;
          if (MODE & 2) v = (cmk[j] && !(mv[r][j] > 0.f)) ? v * a.mask_slope : v;
          if (OUT16)
            __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (__bf16)v), rout,
                                                  (int)(offs[r][j] == 0xffffffffu ? 0xffffffffu : offs[r][j] >> 1), 0, 0);
          else
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rout, offs[r][j], 0, 0);
        }
      }
    }
  };
  using M0 = std::integral_constant<int, 0>; using M1 = std::integral_constant<int, 1>;
  using M2 = std::integral_constant<int, 2>; using M3 = std::integral_constant<int, 3>;
  const int emode = (a.add ? 1 : 0) | (a.mask ? 2 : 0);
  if constexpr (PR == 2) {  // bf16 storage: linear outputs, no addend (the host code asks for nothing else)
    if (out16) {
      if (emode & 2) store_tile(std::true_type{}, M2{}, std::true_type{});
      else store_tile(std::true_type{}, M0{}, std::true_type{});
    } else {
      if (emode & 2) store_tile(std::true_type{}, M2{}, std::false_type{});
      else store_tile(std::true_type{}, M0{}, std::false_type{});
    }
  } else if (a.linear_out) {
    if (emode == 0) store_tile(std::true_type{}, M0{}, std::false_type{});
    else if (emode == 1) store_tile(std::true_type{}, M1{}, std::false_type{});
    else if (emode == 2) store_tile(std::true_type{}, M2{}, std::false_type{});
    else store_tile(std::true_type{}, M3{}, std::false_type{});
  } else {
    if (emode == 0) store_tile(std::false_type{}, M0{}, std::false_type{});
    else if (emode == 1) store_tile(std::false_type{}, M1{}, std::false_type{});
    else if (emode == 2) store_tile(std::false_type{}, M2{}, std::false_type{});
    else store_tile(std::false_type{}, M3{}, std::false_type{});
  }

  float xs1 = 0.f, xs2 = 0.f;
  if (XR > 0 && has_x) {  // the extra 16x16 block: rows BM + 4(l>>4) + reg, column 16 wave + (l&15)
    const int col = n0 + 16 * wave + xi;
    int bidx = col, oc = col;
    if (a.out_shuffle) {
      const int ij = col / a.out_shuffle, cc = col - ij * a.out_shuffle;
      bidx = cc * 4 + ij;
      oc = (((ij >> 1) * a.Wo) + (ij & 1)) * a.Co + cc;
    }
    const float xb = (a.bias && col < a.Cn) ? a.bias[bidx] : 0.f;
    const bool xok = col < a.Cs;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + BM + 4 * xg + r;
      const bool mok = m < a.M;
      const unsigned rowoff = a.linear_out ? 4u * (unsigned)((m - m0) * a.Co) : rowtab[m - m0];
      float v = accx[r] + xb;
      const float vs = mok ? v : 0.f;
      xs1 += vs;
      xs2 += vs * vs;
      v = v > 0.f ? v : v * a.slope;
      const unsigned off = (mok && xok) ? rowoff + 4u * (unsigned)oc : 0xffffffffu;
      if (a.add) {
        const __amdgpu_buffer_rsrc_t radd = make_radd();
        const unsigned arow = a.linear_out ? 4u * (unsigned)((m - m0) * a.add_ld) : rowoff;
        const unsigned aoff = (mok && xok && col < a.add_hi) ? arow + 4u * (unsigned)oc : 0xffffffffu;
        v = v * a.oscale + a.ascale * __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(radd, (int)aoff, 0, 0));
      }
      if (a.mask && col >= a.mask_lo && col < a.mask_hi) {
        const float mv = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rmask, (int)off, 0, 0));
        v = mv > 0.f ? v : v * a.mask_slope;
      }
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rout, off, 0, 0);
    }
  }

  if (a.part) {  // per-channel sum / sum of squares of this row block (training-mode BatchNorm)
    constexpr int RED_ROWS = WAVES_M + (XR > 0 ? 1 : 0);
    __syncthreads();  // everyone is done with the staging buffers
    float* red = reinterpret_cast<float*>(smem);  // [RED_ROWS][BN][2]
    if (XR > 0 && has_x) {
      xs1 += __shfl_xor(xs1, 16, 64); xs1 += __shfl_xor(xs1, 32, 64);
      xs2 += __shfl_xor(xs2, 16, 64); xs2 += __shfl_xor(xs2, 32, 64);
      if (xg == 0) {
        red[(WAVES_M * BN + 16 * wave + xi) * 2 + 0] = xs1;
        red[(WAVES_M * BN + 16 * wave + xi) * 2 + 1] = xs2;
      }
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      float s = csum[j] + __shfl_xor(csum[j], 32, 64);
      float s2 = csq[j] + __shfl_xor(csq[j], 32, 64);
      if (lead && h == 0) {
        const int c = wn * WN + j * 32 + l31;
        red[(wm * BN + c) * 2 + 0] = s;
        red[(wm * BN + c) * 2 + 1] = s2;
      }
    }
    __syncthreads();
    if (lead && tid < BN) {
      float s = 0.f, s2 = 0.f;
#pragma unroll
      for (int w = 0; w < RED_ROWS; ++w) { s += red[(w * BN + tid) * 2]; s2 += red[(w * BN + tid) * 2 + 1]; }
      const int col = n0 + tid;
      if (col < a.Cn) {
        a.part[((size_t)mt * a.Cn + col) * 2 + 0] = s;
        a.part[((size_t)mt * a.Cn + col) * 2 + 1] = s2;
      }
    }
  }
}

template <int BM, int BN, int WM, int WN, int KS, int XR, int PR, int BIG = 0>
__global__ __launch_bounds__((BM / WM) * (BN / WN) * 64 * KS) void gconv_kernel(const GArgs a) {
  // the fused-upsample gather is a second copy of the body, entered by ONE scalar branch: the common loop is untouched
  if (a.up) gconv_body<BM, BN, WM, WN, KS, XR, PR, 1, BIG>(a, blockIdx.x);
  else gconv_body<BM, BN, WM, WN, KS, XR, PR, 0, BIG>(a, blockIdx.x);
}

// several independent gather-GEMMs in one launch: the stride-parity classes of a strided data
// gradient (four small problems that would each under-fill the chip and pay a kernel boundary)
struct GMulti {
  int n;
  int first[5];  // first[i] = first workgroup of problem i; first[n] = grid size
  GArgs g[4];
};
// KS = 2 (round 6, the 64 x 64 tile only): two wave groups share a tile's k-chunks (gconv_body) -- the deep, small-M classes of
// the discriminators' last strided layers (576..4608 rows, K up to 2048 per class) are bound by the serial chunk chain of their
// heaviest class's workgroups, not by the chip: 64 x 64 tiles give four times the workgroups of 128 x 64 and the in-workgroup
// split halves each chain.
template <int BM, int BN, int WM, int WN, int XR, int PR = 0, int KS = 1>
__global__ __launch_bounds__((BM / WM) * (BN / WN) * 64 * KS) void gconv_multi_kernel(const GMulti m) {
  int ci = 0;
  while (ci + 1 < m.n && (int)blockIdx.x >= m.first[ci + 1]) ++ci;
  const GArgs a = m.g[ci];
  gconv_body<BM, BN, WM, WN, KS, XR, PR>(a, blockIdx.x - m.first[ci]);
}

// ---------------------------------------------------------------------------
// Strided data gradient, all stride-parity classes of a tile in ONE workgroup and ONE pipelined K loop (round 6).
//
// gconv_multi_kernel runs the classes as separate workgroups: for the 3x3 / stride-2 layers of the discriminators that is four
// gather-GEMMs with 1, 2, 2 and 4 taps -- K loops of 2..8 chunks at 64 channels, each with its own k table, row set-up, pipeline
// fill and epilogue (34-44 % MFMA-busy under the counters).  The classes of a layer whose extents are multiples of the stride
// share EVERYTHING but their taps, their weight matrix and a constant output offset: the same M grid (one row per gradient
// pixel neighbourhood), hence the same A rows, bounds and row offsets.  Here a workgroup owns one (row tile, column tile) and
// walks the classes back to back: one chunk sequence -- each class's chunks padded to whole trips of the three-slot ring, the
// padding chunks loading nothing and multiplying nothing --, one table entry per chunk (tap coordinates, gather offset, the
// chunk's place in its class's weight matrix: wave-uniform, so they live in SGPRs and the per-thread k table of gconv_body
// disappears), the loads of class c+1 already in flight while class c's accumulators are stored.  A chunk lies inside one tap
// (channels per tap a multiple of 32: checked on the host; other layers keep gconv_multi_kernel).
// ---------------------------------------------------------------------------
struct S2Class {
  int nth, ntw, dh0, dw0;  // taps of the class and its most negative tap
  int chunks, pstart;      // k-chunks (32 floats) of the class; its first chunk in the padded sequence
  int oh_off, ow_off;      // output parity
  unsigned wbase, kpb;     // byte offset of the class's weight matrix in the packed buffer; bytes per row of it (Kp * 4)
};
struct GFused {
  GArgs g;                 // what the classes share (w / w_bytes: the WHOLE packed data-gradient buffer)
  int nclass, cpt, ptotal; // classes; chunks per tap (Ck / 32); chunks of the padded sequence
  S2Class c[4];
};

// (the 64-column tiles: at most 128 registers, so that two 8-wave workgroups share a CU -- one's epilogues and dead steps
// under the other's MFMAs)
template <int BM, int BN, int WM, int WN, int XR, int PR>
__global__ __launch_bounds__((BM / WM) * (BN / WN) * 64, (BM / WM) * (BN / WN) == 8 && BN == 64 ? 4 : 1) void gconv_s2f_kernel(const GFused f) {
  static_assert(PR == 0 || (PR == 1 && XR == 0), "fp32, or bf16 products without the 16-row extension");
  const GArgs& a = f.g;
  constexpr int BKL = PR == 1 ? BK / 2 : BK;
  constexpr int NS = PR == 1 ? 2 : 4;
  constexpr int BMT = BM + XR;
  constexpr int TM = WM / 32, TN = WN / 32;
  constexpr int WAVES_N = BN / WN, WAVES_M = BM / WM;
  constexpr int NT = WAVES_M * WAVES_N * 64;
  constexpr int RPP = NT / 8;
  constexpr int RA = (BMT + RPP - 1) / RPP, RB = BN / RPP;
  static_assert(RA >= 1 && RB >= 1, "tile too small for the thread count");
  static_assert(XR == 0 || BN / 16 <= NT / 64, "one extra 16x16 block per wave at most");
  constexpr int RING = 3;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = srx_uniform(tid >> 6);
  float* sA = reinterpret_cast<float*>(smem);
  float* sB = sA + RING * BMT * BKL;
  int4* ctab = reinterpret_cast<int4*>(sA + RING * (BMT + BN) * BKL);        // [ptotal + 3]
  unsigned* rowtab = reinterpret_cast<unsigned*>(ctab + (f.ptotal + 3));      // [BMT]
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int tile = srx_uniform((int)blockIdx.x);
  const int nt = srx_uniform(tile / a.mtiles), mt = tile - nt * a.mtiles;
  const int m0 = mt * BMT, n0 = nt * BN;
  const int q = tid & 7, r0 = tid >> 3;
  auto split_row = [&](int m, int& n, int& mh, int& mw) {
    int rem;
    srx_divmod(m, a.HmWm, a.inv_HmWm, n, rem);
    srx_divmod(rem, a.Wm, a.inv_Wm, mh, mw);
  };
  const __amdgpu_buffer_rsrc_t rin = srx_rsrc(a.in, (unsigned)a.in_bytes);
  const __amdgpu_buffer_rsrc_t rw = srx_rsrc(a.w, a.w_bytes);

  // ---- chunk table: one entry per chunk of the padded sequence (+ 3 dead ones the pipeline runs ahead into)
  for (int e = tid; e < f.ptotal + 3; e += NT) {
    int4 ent = {(int)(INVALID & 0xffff), 0, 0, 0};  // dead: taps out of every image, weight row pitch 0
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < f.nclass) {
        const S2Class& k = f.c[c];
        const int j = e - k.pstart;
        if (j >= 0 && j < k.chunks) {
          const int tap = j / f.cpt, cin = j - tap * f.cpt;
          const int th = tap / k.ntw, tw = tap - th * k.ntw;
          const int dh = k.dh0 + th, dw = k.dw0 + tw;
          ent.x = (int)((unsigned)(dh & 0xffff) | ((unsigned)dw << 16));
          ent.y = ((dh * a.Wi + dw) * a.Ci + cin * BK) * 4;
          ent.z = (int)(k.wbase + (unsigned)j * (BK * 4));
          ent.w = (int)k.kpb;
        }
      }
    }
    ctab[e] = ent;
  }
  // ---- per-thread rows of the A tile: the same for every class
  int rih[RA], riw[RA];
  unsigned rbase[RA];
#pragma unroll
  for (int p = 0; p < RA; ++p) {
    const int m = m0 + r0 + RPP * p;
    if (m < a.M && r0 + RPP * p < BMT) {
      int n, mh, mw;
      split_row(m, n, mh, mw);
      rih[p] = mh; riw[p] = mw;
      rbase[p] = 4u * (unsigned)(((n * a.Hi + mh) * a.Wi + mw) * a.Ci) + 16u * (unsigned)q;
    } else {
      rih[p] = INVALID; riw[p] = 0; rbase[p] = 0;
    }
  }
  unsigned wrow[RB];
#pragma unroll
  for (int p = 0; p < RB; ++p) wrow[p] = (unsigned)(n0 + r0 + RPP * p);
  // ---- byte offsets of the tile's output rows for parity (0, 0), relative to the tile's first row (a class adds a constant)
  auto out_elem = [&](int m) -> size_t {
    int n, mh, mw;
    split_row(m, n, mh, mw);
    return ((size_t)(n * a.Ho + mh * a.out_stride) * a.Wo + mw * a.out_stride) * a.Co;
  };
  const size_t tile_base = out_elem(m0);
  for (int rr = tid; rr < BMT; rr += NT) {
    const int m = m0 + rr;
    rowtab[rr] = m < a.M ? 4u * (unsigned)(out_elem(m) - tile_base) : 0u;
  }
  __syncthreads();

  f32x16 acc[TM][TN];
  f32x4 accx = {0.f, 0.f, 0.f, 0.f};
  f32x4 ra0[RA], rb0[RB], ra1[RA], rb1[RB], ra2[RA], rb2[RB];
  auto gload = [&](int kc, f32x4 (&ra)[RA], f32x4 (&rb)[RB]) {
    const int4 ct = ctab[kc];  // (one address for the whole wave: a broadcast read)
    const int cx = srx_uniform(ct.x), cy = srx_uniform(ct.y), cz = srx_uniform(ct.z), cw = srx_uniform(ct.w);
    const int dh = (int)(short)(cx & 0xffff), dw = cx >> 16;
#pragma unroll
    for (int p = 0; p < RA; ++p) {
      const int ih = rih[p] + dh, iw = riw[p] + dw;
      const bool ok = ((unsigned)ih < (unsigned)a.Hi) && ((unsigned)iw < (unsigned)a.Wi);
      ra[p] = srx_bload(rin, ok ? rbase[p] + (unsigned)cy : 0xffffffffu, 0);  // out of range (padding taps, dead chunks) reads 0
    }
#pragma unroll
    for (int p = 0; p < RB; ++p)
      rb[p] = srx_bload(rw, cw ? wrow[p] * (unsigned)cw + 16u * (unsigned)q : 0xffffffffu, (unsigned)cz);
  };
  const int wchunk = PR == 1 ? (((q >> 1) ^ ((r0 >> 2) & 3)) * 4 + (q & 1) * 2) : (q ^ ((r0 >> 1) & 7)) * 4;
  auto put = [&](float* dst, const f32x4& v) {
    if (PR == 1) {
      typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
      const bf16x2 lo = {(__bf16)v[0], (__bf16)v[1]}, hi = {(__bf16)v[2], (__bf16)v[3]};
      *reinterpret_cast<uint2*>(dst) = make_uint2(__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi));
    } else {
      *reinterpret_cast<f32x4*>(dst) = v;
    }
  };
  auto swrite = [&](int buf, const f32x4 (&ra)[RA], const f32x4 (&rb)[RB]) {
    float* dA = sA + buf * BMT * BKL;
    float* dB = sB + buf * BN * BKL;
#pragma unroll
    for (int p = 0; p < RA; ++p)
      if (RPP * (p + 1) <= BMT || r0 + RPP * p < BMT) put(dA + (r0 + RPP * p) * BKL + wchunk, ra[p]);
#pragma unroll
    for (int p = 0; p < RB; ++p) put(dB + (r0 + RPP * p) * BKL + wchunk, rb[p]);
  };
  const int h = lane >> 5, l31 = lane & 31;
  const int xr = PR == 1 ? (l31 >> 2) & 3 : (l31 >> 1) & 7;
  const int arow = (wm * WM + l31) * BKL, brow = (wn * WN + l31) * BKL;
  const bool has_x = XR > 0 && wave < BN / 16;
  const int xi = lane & 15, xg = lane >> 4;
  const int xra = BM + xi, xrb = 16 * wave + xi;
  f32x4 af[2][TM], bf[2][TN];
  auto frag = [&](int slot, int s, int set) {
    const float* cA = sA + slot * BMT * BKL + arow;
    const float* cB = sB + slot * BN * BKL + brow;
    const int ch = ((2 * s + h) ^ xr) * 4;
#pragma unroll
    for (int i = 0; i < TM; ++i) af[set][i] = *reinterpret_cast<const f32x4*>(cA + i * 32 * BKL + ch);
#pragma unroll
    for (int j = 0; j < TN; ++j) bf[set][j] = *reinterpret_cast<const f32x4*>(cB + j * 32 * BKL + ch);
  };
  auto mma = [&](int set) {
    __builtin_amdgcn_s_setprio(1);
    if (PR) {
      typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[set][i]),
                                                              __builtin_bit_cast(bf16x8, bf[set][j]), acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[set][i][e], bf[set][j][e], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };
  auto extra = [&](int slot) {
    const float* xA = sA + slot * BMT * BKL + xra * BKL;
    const float* xB = sB + slot * BN * BKL + xrb * BKL;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const f32x4 fa = *reinterpret_cast<const f32x4*>(xA + (((xg + 4 * u) ^ ((xra >> 1) & 7)) * 4));
      const f32x4 fb = *reinterpret_cast<const f32x4*>(xB + (((xg + 4 * u) ^ ((xrb >> 1) & 7)) * 4));
#pragma unroll
      for (int e = 0; e < 4; ++e) accx = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[e], fb[e], accx, 0, 0, 0);
    }
  };
  // one step of gconv_body's pipeline (see there); `live`: the chunk is a real one of the class
  auto step = [&](int kc, int slot, f32x4 (&ra_next)[RA], f32x4 (&rb_next)[RB], f32x4 (&ra_free)[RA], f32x4 (&rb_free)[RB]) {
    const int nslot = slot == 2 ? 0 : slot + 1;
    swrite(nslot, ra_next, rb_next);
    gload(kc + 3, ra_free, rb_free);
    const bool live = srx_uniform(ctab[kc].w) != 0;
    if (NS == 2) {
      frag(slot, 1, 1);
      if (live) mma(0);
      __syncthreads();
      frag(nslot, 0, 0);
      if (live) mma(1);
      return;
    }
    frag(slot, 1, 1);
    if (live) mma(0);
    frag(slot, 2, 0);
    if (live) mma(1);
    __syncthreads();
    frag(slot, 3, 1);
    if (live) mma(0);
    frag(nslot, 0, 0);
    if (XR > 0 && has_x && live) extra(slot);
    if (live) mma(1);
  };

  // ---- epilogue constants (class-independent)
  const unsigned tb_lo = (unsigned)srx_uniform((int)(unsigned)(tile_base & 0xffffffffu));
  const unsigned tb_hi = (unsigned)srx_uniform((int)(unsigned)(tile_base >> 32));
  unsigned ocol[TN];
  bool cok[TN], cmk[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn * WN + j * 32 + l31;
    cmk[j] = col >= a.mask_lo && col < a.mask_hi;
    ocol[j] = 4u * (unsigned)col;
    cok[j] = col < a.Cs;
  }
  auto store_class = [&](auto masked, const __amdgpu_buffer_rsrc_t rout, const __amdgpu_buffer_rsrc_t rmask) {
    constexpr bool MASK = decltype(masked)::value;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int hr = 0; hr < 16; hr += 8) {  // eight rows at a time: the offsets and mask values of a half block are what the
        unsigned offs[8][TN];               // epilogue holds on top of the three load stages in flight (two workgroups per CU)
        float mv[MASK ? 8 : 1][TN];
#pragma unroll
        for (int r8 = 0; r8 < 8; ++r8) {  // (every mask value of the half block is requested before its first store: see gconv_body)
          const int r = hr + r8;
          const int rl = wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          const bool mok = m0 + rl < a.M;
          const unsigned rowoff = rowtab[rl];
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const unsigned off = (mok && cok[j]) ? rowoff + ocol[j] : 0xffffffffu;
            offs[r8][j] = off;
            if (MASK) mv[r8][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rmask, (int)(cmk[j] ? off : 0xffffffffu), 0, 0));
          }
        }
#pragma unroll
        for (int r8 = 0; r8 < 8; ++r8)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            float v = acc[i][j][hr + r8];
            if (MASK) v = (cmk[j] && !(mv[r8][j] > 0.f)) ? v * a.mask_slope : v;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rout, offs[r8][j], 0, 0);
          }
      }
    if (XR > 0 && has_x) {  // the extra 16x16 block: rows BM + 4(l>>4) + reg, column 16 wave + (l&15)
      const int col = n0 + 16 * wave + xi;
      const bool xok = col < a.Cs;
      const bool xmk = MASK && col >= a.mask_lo && col < a.mask_hi;
      unsigned xoff[4];
      float xm[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = BM + 4 * xg + r;
        xoff[r] = (m0 + rl < a.M && xok) ? rowtab[rl] + 4u * (unsigned)col : 0xffffffffu;
        xm[r] = MASK ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rmask, (int)(xmk ? xoff[r] : 0xffffffffu), 0, 0)) : 1.f;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = accx[r];
        if (MASK) v = (xmk && !(xm[r] > 0.f)) ? v * a.mask_slope : v;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rout, xoff[r], 0, 0);
      }
    }
  };

  // ---- the pipelined loop over the padded chunk sequence, class by class
  gload(0, ra0, rb0);
  gload(1, ra1, rb1);
  gload(2, ra2, rb2);
  swrite(0, ra0, rb0);
  __syncthreads();
  frag(0, 0, 0);
  int kc = 0;
  for (int c = 0; c < f.nclass; ++c) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    accx = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kend = srx_uniform(c + 1 < f.nclass ? f.c[c + 1].pstart : f.ptotal);
    for (; kc < kend; kc += 3) {  // whole trips of the ring (a class's chunks are padded to a multiple of three)
      step(kc, 0, ra1, rb1, ra0, rb0);
      step(kc + 1, 1, ra2, rb2, ra1, rb1);
      step(kc + 2, 2, ra0, rb0, ra2, rb2);
    }
    // this class's outputs: parity (oh_off, ow_off) of the tile's 2x2 (stride x stride) output blocks
    const S2Class& k = f.c[c];
    const size_t delta = ((size_t)k.oh_off * a.Wo + k.ow_off) * a.Co;
    const size_t cbase = ((((size_t)tb_hi << 32) | tb_lo) + delta) << 2;
    const unsigned cb_lo = (unsigned)srx_uniform((int)(unsigned)(cbase & 0xffffffffu));
    const unsigned cb_hi = (unsigned)srx_uniform((int)(unsigned)(cbase >> 32));
    const size_t cb = ((size_t)cb_hi << 32) | cb_lo;
    const __amdgpu_buffer_rsrc_t rout = srx_rsrc(reinterpret_cast<char*>(a.out) + cb, 0xfffffff0u);
    const __amdgpu_buffer_rsrc_t rmask = srx_rsrc(reinterpret_cast<const char*>(a.mask ? a.mask : a.out) + cb, 0xfffffff0u);
    if (a.mask) store_class(std::true_type{}, rout, rmask);
    else store_class(std::false_type{}, rout, rmask);
  }
}

// finishes the K-split tail tiles: out = act(sum_z partial[z] + bias) and, when asked, the tile's
// per-channel (sum, sum of squares) row of the BatchNorm partial table.  One workgroup per
// (tile, 16-column group): every column's statistics stay inside one workgroup, and a tile with
// many K splits is still drained by BN/16 workgroups rather than one.
template <int BM, int BN>
__global__ __launch_bounds__(256) void tail_fixup_kernel(const GArgs a) {
  constexpr int CG = BN / 16;
  __shared__ f32x4 red[2][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = tid & 3, rl = tid >> 2;  // 4 float4 quads x 64 row lanes
  const int t = blockIdx.x / CG, cg = blockIdx.x % CG;
  const int tile = a.full_tiles + t;
  const int mt = tile % a.mtiles, nt = tile / a.mtiles;
  const int m0 = mt * BM, n0 = nt * BN;
  const float* slab = a.ws + (size_t)t * a.tail_split * (BM * BN);
  const int lc = cg * 16 + q * 4;  // column inside the tile
  const int col = n0 + lc;
  f32x4 bv = {0.f, 0.f, 0.f, 0.f};
  if (a.bias) {
#pragma unroll
    for (int e = 0; e < 4; ++e) bv[e] = (col + e < a.Cn) ? a.bias[col + e] : 0.f;
  }
  f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
  // All loads first, without branches around them (rows past the tile or the image read a valid row and are dropped
  // afterwards): the K-split partials four at a time, the addend and the mask -- the launch is a few load round trips long,
  // and a load behind a data-dependent branch or a runtime-count loop waits for the one before it (8 -> ~5 us per launch).
  // The partials are added in the order z = 0, 1, 2, ... as before.
  constexpr int NR = (BM + 63) / 64;
  f32x4 v[NR], av[NR], mv[NR];
  bool ok[NR];
  const bool has_add = a.add != nullptr && col < a.Cs && col < a.add_hi;
  const bool has_mask = a.mask != nullptr && col < a.Cs && col >= a.mask_lo && col < a.mask_hi;
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int r = rl + 64 * j;
    ok[j] = r < BM && m0 + r < a.M;
    const int mc = min(m0 + (r < BM ? r : rl), a.M - 1);
    av[j] = has_add ? *reinterpret_cast<const f32x4*>(a.add + (size_t)mc * a.add_ld + col) : (f32x4){0.f, 0.f, 0.f, 0.f};
    if (has_mask && a.mask16) {  // (bf16 mask tensor: four values in 8 bytes)
      const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(a.mask) + (size_t)mc * a.Co + col);
      mv[j] = (f32x4){__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xffff0000u),
                      __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xffff0000u)};
    } else {
      mv[j] = has_mask ? *reinterpret_cast<const f32x4*>(a.mask + (size_t)mc * a.Co + col) : (f32x4){1.f, 1.f, 1.f, 1.f};
    }
    v[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  for (int z0 = 0; z0 < a.tail_split; z0 += 4) {
    f32x4 t[NR][4];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int rc = rl + 64 * j < BM ? rl + 64 * j : rl;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        t[j][u] = *reinterpret_cast<const f32x4*>(slab + (size_t)min(z0 + u, a.tail_split - 1) * (BM * BN) + rc * BN + lc);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (z0 + u < a.tail_split) {
#pragma unroll
        for (int j = 0; j < NR; ++j) v[j] = (z0 + u == 0) ? t[j][u] : v[j] + t[j][u];
      }
  }
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    if (!ok[j]) continue;
    const int m = m0 + rl + 64 * j;
    f32x4 w = v[j] + bv;
    s1 += w;
    s2 += w * w;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = w[e] > 0.f ? w[e] : w[e] * a.slope;
    if (col < a.Cs) {  // Cs is a multiple of 4
      if (a.add) {  // (add_hi is a multiple of 4 or covers every column)
        w = w * a.oscale;
        if (col < a.add_hi) w += av[j] * a.ascale;
      }
      if (has_mask) {  // (mask ranges are whole quads: channel counts are multiples of 4)
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = mv[j][e] > 0.f ? w[e] : w[e] * a.mask_slope;
      }
      if (a.out16) {
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        const bf16x2 lo = {(__bf16)w[0], (__bf16)w[1]}, hi = {(__bf16)w[2], (__bf16)w[3]};
        *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(a.out) + (size_t)m * a.Co + col) =
            make_uint2(__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi));
      } else {
        *reinterpret_cast<f32x4*>(a.out + (size_t)m * a.Co + col) = w;
      }
    }
  }
  if (a.part) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int o = 4; o < 64; o <<= 1) { s1[e] += __shfl_xor(s1[e], o, 64); s2[e] += __shfl_xor(s2[e], o, 64); }
    if (lane < 4) { red[0][wave * 4 + lane] = s1; red[1][wave * 4 + lane] = s2; }
    __syncthreads();
    if (tid < 4) {
      const f32x4 t1 = red[0][tid] + red[0][4 + tid] + red[0][8 + tid] + red[0][12 + tid];
      const f32x4 t2 = red[1][tid] + red[1][4 + tid] + red[1][8 + tid] + red[1][12 + tid];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (col + e < a.Cn) {
          a.part[((size_t)mt * a.Cn + col + e) * 2 + 0] = t1[e];
          a.part[((size_t)mt * a.Cn + col + e) * 2 + 1] = t2[e];
        }
    }
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// host side: first what wgrad.hip and convpack.hip use too (declared in conv_host.h)
// ---------------------------------------------------------------------------
int check_desc(const srx_conv2d_t* d) {
  SRX_REQUIRE(d, "conv2d: null descriptor");
  SRX_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0, "conv2d: non-positive size");
  SRX_REQUIRE(d->Cin_s >= d->Cin && d->Cin_s % 4 == 0, "conv2d: Cin_s must be a multiple of 4 and >= Cin");
  SRX_REQUIRE(d->KH > 0 && d->KW > 0 && d->stride > 0 && d->pad >= 0, "conv2d: bad kernel geometry");
  SRX_REQUIRE(d->shuffle == 0 || d->shuffle == 2, "conv2d: shuffle must be 0 or 2");
  SRX_REQUIRE(d->up == 0 || d->up == 1 || d->up == 2, "conv2d: up must be 0 / 1 (none) or 2 (nearest x2 in the gather)");
  if (d->up == 2) SRX_REQUIRE(d->stride == 1 && !d->shuffle, "conv2d: up = 2 needs stride 1 and no PixelShuffle");
  if (d->shuffle) {
    SRX_REQUIRE(d->Cout % 16 == 0, "conv2d: shuffle needs Cout multiple of 16");
    SRX_REQUIRE(d->Cout_s >= d->Cout / 4 && d->Cout_s % 4 == 0, "conv2d: bad Cout_s for shuffle");
    SRX_REQUIRE(d->stride == 1, "conv2d: shuffle needs stride 1");
  } else {
    SRX_REQUIRE(d->Cout_s >= d->Cout && d->Cout_s % 4 == 0, "conv2d: Cout_s must be a multiple of 4 and >= Cout");
  }
  SRX_REQUIRE(d->act == SRX_ACT_NONE || d->act == SRX_ACT_RELU || d->act == SRX_ACT_LRELU, "conv2d: bad act");
  SRX_REQUIRE(d->precision == 0 || d->precision == 1 || (d->precision == 2 && srx_thin_fwd_applicable(d)) ||
                  (d->precision == 3 && d->Cin_s == 4 && !d->shuffle && d->up != 2),
              "conv2d: precision must be 0 (fp32), 1 (bf16 products) or, for the forward of a 64 -> <= 4 channel layer, 2 (bf16 products there too), "
              "or, for the forward of a <= 4-channel input layer, 3 (fp16 products)");
  const int uf = d->up == 2 ? 2 : 1;
  const int Ho = (uf * d->H + 2 * d->pad - d->KH) / d->stride + 1, Wo = (uf * d->W + 2 * d->pad - d->KW) / d->stride + 1;
  SRX_REQUIRE(Ho > 0 && Wo > 0, "conv2d: empty output");
  // (the generic forward / data-gradient kernel addresses by 64-bit tile bases and splits pixel indices exactly above 2^24;
  // the kernels that do not -- weight gradients, the row tile, the 3-channel input layers -- check `small_enough` themselves)
  SRX_REQUIRE((int64_t)d->N * uf * d->H * uf * d->W < (1LL << 31) - 1024 && (int64_t)d->N * Ho * Wo < (1LL << 31) - 1024,
              "conv2d: more than 2^31 pixels per call; tile the image");
  SRX_REQUIRE((int64_t)uf * d->W * d->Cin_s * 4 * (d->KH + 160) < (1LL << 32), "conv2d: image rows too long for 32-bit offsets inside a tile");
  SRX_REQUIRE(d->pad < 16000 && d->KH < 16000, "conv2d: kernel too large");
  return SRX_OK;
}

// below 2^24 pixels and 4 GiB of input: what the kernels with 32-bit tensor offsets / float index division can take
bool small_enough(const srx_conv2d_t* d) {
  const int uf = d->up == 2 ? 2 : 1;
  const int Ho = (uf * d->H + 2 * d->pad - d->KH) / d->stride + 1, Wo = (uf * d->W + 2 * d->pad - d->KW) / d->stride + 1;
  return (int64_t)d->N * uf * d->H * uf * d->W < (1 << 24) && (int64_t)d->N * Ho * Wo < (1 << 24) &&
         (int64_t)d->N * d->H * d->W * d->Cin_s < (1LL << 30) - 4;
}

int pad_rows(int c) { return c <= 32 ? 32 : (int)srx_roundup(c, 64); }  // rows of a packed operand: whole 64-column tiles (32 for the narrow tile)

Geo fwd_geo(const srx_conv2d_t* d) {
  Geo g;
  const int uf = d->up == 2 ? 2 : 1;  // extents the conv sees
  g.Ho = (uf * d->H + 2 * d->pad - d->KH) / d->stride + 1;
  g.Wo = (uf * d->W + 2 * d->pad - d->KW) / d->stride + 1;
  g.Ck = (int)srx_roundup(d->Cin, 4);  // k-space channels; the tensor's channel stride Cin_s may be larger
  g.K = d->KH * d->KW * g.Ck;
  g.Kp = (int)srx_roundup(g.K, BK);
  g.Cnp = pad_rows(d->Cout);
  g.cps = d->shuffle ? d->Cout / 4 : 0;
  return g;
}

// taps of class `par` along one axis: kernel size Kd; returns count, sets dmin
static int class_taps(int par, int pad, int stride, int Kd, int& dmin) {
  const int kfirst = (par + pad) % stride;
  if (kfirst >= Kd) { dmin = 0; return 0; }
  const int cnt = (Kd - 1 - kfirst) / stride + 1;
  const int dmax = (par + pad - kfirst) / stride;
  dmin = dmax - (cnt - 1);
  return cnt;
}

// channels per tap of the data gradient's K axis: the layer's output channels, NOT the channel stride of
// the gradient tensor (a conv may write a 32-channel slice of a 192-channel dense-block buffer)
int bwd_ck(const srx_conv2d_t* d) { return d->shuffle ? d->Cout : (int)srx_roundup(d->Cout, 4); }

int bwd_classes(const srx_conv2d_t* d, BwdClass* cls, size_t& total_floats) {
  const int Ck = bwd_ck(d);
  const int Cnp = pad_rows(d->Cin);
  int n = 0;
  total_floats = 0;
  for (int ph = 0; ph < d->stride; ++ph)
    for (int pw = 0; pw < d->stride; ++pw) {
      BwdClass c;
      c.ph = ph; c.pw = pw;
      c.nth = class_taps(ph, d->pad, d->stride, d->KH, c.dminh);
      c.ntw = class_taps(pw, d->pad, d->stride, d->KW, c.dminw);
      c.Hm = (d->H - ph + d->stride - 1) / d->stride;
      c.Wm = (d->W - pw + d->stride - 1) / d->stride;
      c.K = c.nth * c.ntw * Ck;
      c.Kp = (int)srx_roundup(c.K > 0 ? c.K : 1, BK);
      c.woff = total_floats;
      total_floats += (size_t)Cnp * c.Kp;
      cls[n++] = c;
    }
  return n;
}

// up = 2 outside the forward pass: the data gradient is taken at the upsampled size into scratch and summed over each
// 2x2 block (the adjoint of nearest upsampling), the weight gradient reads a scratch copy of the upsampled input.
srx_conv2d_t upsampled_desc(const srx_conv2d_t* d) {
  srx_conv2d_t h = *d;
  h.up = 0; h.H = 2 * d->H; h.W = 2 * d->W;
  return h;
}
size_t upsampled_floats(const srx_conv2d_t* d) { return (size_t)d->N * 2 * d->H * 2 * d->W * d->Cin_s; }

// The one instance of the planners' overrides (conv_host.h), seeded from the environment switches at first use.
ConvForce& conv_force() {
  static ConvForce* f = [] {
    ConvForce* s = new ConvForce;
    const SrxDevSwitches& e = srx_dev();
    for (int i = 0; i < 4; ++i) s->plan[i].store(e.force_plan ? e.plan[i] : 0);
    s->s2[0].store((e.s2_mode & 1) ? 1 : 0); s->s2[1].store(0); s->s2[2].store(0);
    s->wg[0].store(e.no_wgrad_lin ? 0 : -1); s->wg[1].store(e.wgrad_nsplit > 0 && e.wgrad_nsplit <= 64 ? e.wgrad_nsplit : 0);
    s->wg_rows.store(e.wgrad_rows_nsplit > 0 && e.wgrad_rows_nsplit <= 64 ? e.wgrad_rows_nsplit : 0);
    s->wk[0].store(e.no_wgrad_dma ? 0 : -1); s->wk[1].store(e.no_wgrad_rows ? 0 : -1); s->wk[2].store(e.old_wgrad_reduce ? 0 : -1);
    return s;
  }();
  return *f;
}

namespace {

// Launch plan.  The chip finishes when its busiest CU does, and a CU's matrix pipes are shared by
// whatever workgroups sit on it, so time ~ (tiles on the busiest CU) x (tile work).  With T equal
// tiles on P CUs that is ceil(T/P): 288 tiles cost as much as 512.  The plan therefore runs the
// first floor(T/P)*P tiles whole and cuts the remaining r = T mod P tiles `split` ways along K so
// that the last round is r*split <= ~P small workgroups (a data-parallel + split-K-tail hybrid);
// only those r tiles take the partial-sum round trip through HBM.  Larger tiles are preferred
// (fewer L2->LDS bytes per MFMA: the 64x64 tile moves 16 B/clk/workgroup and stalls on L1/L2)
// unless they leave the chip under-filled.
struct Plan { int BM, BN, mtiles, ntiles, tiles, full, tail, split, kc_per_split, ks; float cost; bool refused; };

// The tile table: every (BM, BN) tile a plan may name, the template head it launches and the instantiations that exist.  The
// planners, the forced-plan refusals, the argument checks of srx_conv2d_force_plan / srx_conv2d_force_s2 and the dispatchers
// read this table and nothing else: a new instantiation is one more entry in a row's `ks`, a new tile one more row.  The ORDER
// is the planners' candidate order -- they pick with a strict <, so the earlier row wins a tie.
enum Family { F_GCONV, F_BIG, F_MULTI, F_S2F, NFAM };  // gconv_kernel, gconv_kernel BIG, gconv_multi_kernel, gconv_s2f_kernel
constexpr unsigned char K1 = 1, K2 = 2, K4 = 4, K12 = K1 | K2;  // sets of wave-group counts KS: a bit's value is the count
struct Tile {
  int BM, BN, WM, WN, XR;  // the planner's tile, rows x columns per wave, extension rows: the template head is <BM - XR, BN, WM, WN, .., XR>
  float eff;               // measured MFMA efficiency in steady state
  unsigned char ks[NFAM][4];  // [family][PR = 0 fp32, 1 bf16 products, 2 bf16 storage, 3 fp16 products]: the KS instantiated; 0: none
};
// (144, *): 128 rows + a 16-row extension, fp32 only
// (64, 32): narrow layers (the 32-channel growth convs of ESRGAN's dense blocks) on twice as many tiles, the
// k-chunks of each tile split over 2 (fp32) / 4 (bf16) wave groups inside the workgroup -- no fix-up pass
// (256, 128), bf16 only (round 4): 64 x 64 per wave, one LDS fragment read per MFMA instead of 1.5 -- the bf16 loop is bound
// by LDS traffic: 256 -> 256 at 32 x 32 x 32 pixels 560 -> 650 TFLOP/s, 128 -> 256 at 64^2 484 -> 546; with fp32 products the
// same tile LOSES a third (72 vs 110 TFLOP/s: 212 registers, and nothing there was LDS-bound) and is never planned
constexpr Tile kTiles[] = {
    // BM, BN, WM, WN, XR, eff, {gconv_kernel, its BIG form (whole frames), gconv_multi_kernel, gconv_s2f_kernel}
    {144, 128, 64, 32, 16, 0.91f, {{K1}, {}, {K1}, {K1}}},
    {144, 64, 32, 32, 16, 0.82f, {{K1}, {}, {K1}, {K1}}},
    {128, 128, 64, 32, 0, 0.95f, {{K1, K1, K1, K1}, {K1, K1, 0, K1}, {K1, K1}, {K1, K1}}},
    {128, 64, 32, 32, 0, 0.85f, {{K1, K1, K1, K1}, {K1, K1, 0, K1}, {K1, K1}, {K1, K1}}},
    {64, 64, 32, 32, 0, 0.60f, {{K12, K12, K12, K12}, {}, {K12, K12}, {K1, K1}}},
    {128, 32, 32, 32, 0, 0.50f, {{K1, K1, 0, K1}, {K1, K1, 0, K1}, {K1, K1}, {}}},
    {64, 32, 32, 32, 0, 0.50f, {{K2, K4, 0, K4}}},
    {256, 128, 64, 64, 0, 1.08f, {{0, K1, K1, K1}}},
};
constexpr int NTILES = sizeof(kTiles) / sizeof(kTiles[0]);

const Tile* find_tile(int bm, int bn) {
  const Tile* t = std::find_if(kTiles, kTiles + NTILES, [&](const Tile& x) { return x.BM == bm && x.BN == bn; });
  return t != kTiles + NTILES ? t : nullptr;
}
// does family f have tile bm x bn with ks (1 / 2 / 4; 0: any number of) wave groups at arithmetic pr?
bool has_tile(Family f, int bm, int bn, int ks, int pr) {
  const Tile* t = find_tile(bm, bn);
  return t && (t->ks[f][pr] & (ks ? ks : K1 | K2 | K4)) != 0;
}
// bm is the rows of one of family f's tiles and bn the columns of one: what the force calls take (whether the pair is a tile,
// and one the layer can run, is answered per layer, with a reason)
bool tile_sides_known(Family f, int bm, int bn) {
  bool rows = false, cols = false;
  for (const Tile& t : kTiles)
    if (t.ks[f][0] | t.ks[f][1] | t.ks[f][2] | t.ks[f][3]) { rows |= t.BM == bm; cols |= t.BN == bn; }
  return rows && cols;
}
// wave groups of tile t in family f at arithmetic pr: the one count it is instantiated with (64 x 32: 2 in fp32, 4 in bf16) or,
// where it has one and two (64 x 64), two when `two` says so
int tile_ks(const Tile& t, Family f, int pr, bool two) {
  const int have = t.ks[f][pr];
  return have == K12 ? (two ? 2 : 1) : have ? have : 1;
}
// the 32-column tiles are for the layers of 32 padded columns, which take no other; elsewhere the tile's columns divide the layer's
bool columns_fit(int Cnp, int bn) { return Cnp == 32 ? bn == 32 : (bn != 32 && Cnp % bn == 0); }

// microseconds for one whole tile of `chunks` k-chunks on an otherwise idle CU (4 SIMDs x 64 FLOP/clk at ~2.1 GHz).  bf16 products:
// the loop is bound by the fp32 operand stream, not by the matrix pipe, and runs ~3x the fp32 rate (measured
// 240-360 vs ~105 TFLOP/s on the VGG layers) -- the fixed cost of a K-split fix-up pass weighs 3x more
float tile_us(int bm, int bn, int chunks, float eff, bool bf16) {
  return 2.0f * bm * bn * (float)chunks * BK / (4 * 64 * 2.1e3f) / eff / (bf16 ? 3.0f : 1.0f);
}

// dynamic LDS of a launch: KS x 3 stages of the tile's operand rows (2-byte elements under bf16 / fp16 products) and, for
// gconv_kernel / gconv_multi_kernel, the k-table of the longest K range; for gconv_s2f_kernel, the classes' k-positions and a word per row
size_t stage_bytes(int bm, int bn, int ks, int pr) { return (size_t)(ks * 3 * (bm + bn) * BK) * (pr == 1 || pr == 3 ? 2 : 4); }
size_t gconv_lds_bytes(int bm, int bn, int ks, int pr, int chunks) { return stage_bytes(bm, bn, ks, pr) + (size_t)chunks * 8 * sizeof(int2); }
size_t s2f_lds_bytes(int bm, int bn, int pr, int pos) { return stage_bytes(bm, bn, 1, pr) + (size_t)(pos + 3) * sizeof(int4) + (size_t)srx_roundup(bm, 4) * 4; }

bool forced_plan(int& bm, int& bn, int& sp, int& ks) {
  ConvForce& f = conv_force();
  bn = f.plan[1].load(std::memory_order_relaxed);
  bm = f.plan[0].load(std::memory_order_relaxed); sp = f.plan[2].load(std::memory_order_relaxed); ks = f.plan[3].load(std::memory_order_relaxed);
  return bn > 0;
}

// nullptr: family f (gconv_kernel / gconv_multi_kernel) has an instantiation for tile bm x bn with ks wave
// groups at this arithmetic and the tile's columns divide the layer's padded ones; otherwise why not
const char* forced_tile_refusal(Family f, int bm, int bn, int ks, int Cnp, bool bf16) {
  if (Cnp % bn != 0) return "the tile's columns do not divide the layer's padded output columns";
  const Tile* t = find_tile(bm, bn);
  if (ks == 2 && !(t && (t->ks[F_GCONV][0] & (K2 | K4)))) return "two wave groups (KS = 2) on a tile other than 64 x 64 / 64 x 32";
  if (bf16 && bm == 144) return "no 144-row tile with bf16 products";
  if (!bf16 && bm == 256) return "no 256-row tile with fp32 products";
  return has_tile(f, bm, bn, 0, bf16 ? 1 : 0) ? nullptr : "no instantiation of this tile";
}

Plan make_plan(int M, int Cnp, int kchunks, bool can_split, bool bf16 = false, bool big = false) {
  const int P = srx_plan_cus();  // the device's CUs less the reserved ones (api.cpp)
  const Family fam = big ? F_BIG : F_GCONV;  // (whole-frame calls, the BIG instantiations: 128 x {128, 64, 32})
  const int pr = bf16 ? 1 : 0;
  Plan best{};
  best.cost = 1e30f;
  for (const Tile& t : kTiles) {
    const int bm = t.BM, bn = t.BN;
    if (!t.ks[fam][pr] || !columns_fit(Cnp, bn)) continue;
    Plan p{};
    p.BM = bm; p.BN = bn; p.mtiles = (int)srx_cdiv(M, bm); p.ntiles = Cnp / bn; p.tiles = p.mtiles * p.ntiles;
    const float t_tile = tile_us(bm, bn, kchunks, t.eff, bf16);
    const int rounds = p.tiles / P, r = p.tiles % P;
    p.full = rounds * P; p.tail = r; p.split = 1; p.kc_per_split = kchunks;
    float tail_cost = r ? t_tile : 0.f;
    if (r && can_split && !big) {
      const int smax = kchunks / 4 < 16 ? kchunks / 4 : 16;
      for (int s = 2; s <= smax; ++s) {
        const int kcs = (int)srx_cdiv(kchunks, s);
        const int s_eff = (int)srx_cdiv(kchunks, kcs);
        const float busiest = (float)srx_cdiv((int64_t)r * s_eff, P) * kcs / (float)kchunks;
        // fix-up: (s+1) passes over the tail tiles at ~3 TB/s plus one more kernel boundary
        const float fix = 4.0f + (float)r * (s_eff + 1) * bm * bn * 4.0f / 3.0e6f + (float)s_eff * bm * 64.0f / 40.0e3f;
        const float c = busiest * t_tile + fix;
        if (c < tail_cost) { tail_cost = c; p.split = s_eff; p.kc_per_split = kcs; }
      }
    }
    p.cost = rounds * t_tile + tail_cost;
    if (p.cost < best.cost) best = p;
  }
  // forced plan (srx_conv2d_force_plan, SRX_FORCE_PLAN="BM,BN,split,ks"; split: K-split of ALL tiles where the output is linear,
  // strided / shuffled outputs run unsplit).  A tile without a kernel is refused (`refused`, message set), never replaced.
  int bm, bn, sp, ks;
  if (!big && forced_plan(bm, bn, sp, ks)) {
    Plan p{};
    if (const char* why = forced_tile_refusal(F_GCONV, bm, bn, ks, Cnp, bf16)) {
      srx_set_error("conv2d: forced plan %d x %d (KS %d) refused: %s (%d padded columns, %s products)", bm, bn, ks, why, Cnp,
                    bf16 ? "bf16" : "fp32");
      p.refused = true;
      return p;
    }
    p.BM = bm; p.BN = bn; p.mtiles = (int)srx_cdiv(M, bm); p.ntiles = Cnp / bn; p.tiles = p.mtiles * p.ntiles;
    if (sp > 1 && can_split) { p.full = 0; p.tail = p.tiles; p.kc_per_split = (int)srx_cdiv(kchunks, sp); p.split = (int)srx_cdiv(kchunks, p.kc_per_split); }
    else { p.full = p.tiles; p.tail = 0; p.split = 1; p.kc_per_split = kchunks; }
    p.ks = tile_ks(*find_tile(bm, bn), F_GCONV, pr, ks == 2);
    return p;
  }
  // fewer workgroups than CUs and a 4-wave tile (64 x 64): split its k-chunks over two wave groups (KS = 2)
  const Tile* t = find_tile(best.BM, best.BN);
  best.ks = t ? tile_ks(*t, fam, pr, best.full + best.tail * best.split <= P && best.kc_per_split >= 4) : 1;
  return best;
}

size_t plan_ws_floats(const Plan& p) { return p.split > 1 ? (size_t)p.tail * p.split * p.BM * p.BN : 0; }

template <int BM, int BN, int WM, int WN, int KS, int XR, int PR = 0, int BIG = 0>
int launch_gconv(const GArgs& a, const Plan& p, hipStream_t st) {
  const int ktab_chunks = p.full > 0 || p.split == 1 ? a.kchunks : p.kc_per_split;
  const size_t lds = gconv_lds_bytes(BM + XR, BN, KS, PR, ktab_chunks);
  if (lds > 160 * 1024) SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d: K range needs %zu bytes of LDS", lds);
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gconv_kernel<BM, BN, WM, WN, KS, XR, PR, BIG>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  });
  dim3 grid(p.full + p.tail * p.split);
  char nm[112];  // kernel + GEMM shape: the roofline leg of bench.py groups launches by both
  if (srx_prof_on())
    snprintf(nm, sizeof(nm), "gconv_kernel<%d, %d, %d, %d, %d, %d, %d%s> MxNxK=%dx%dx%d", BM, BN, WM, WN, KS, XR, PR, BIG ? ", big" : "",
             a.M, a.Cn, PR == 2 ? 2 * a.K : a.K);  // (PR = 2: K counts floats = pairs of bf16 values)
  SRX_LAUNCH_PROF(nm, 2.0 * a.M * a.Cn * (PR == 2 ? 2 * a.K : a.K), (gconv_kernel<BM, BN, WM, WN, KS, XR, PR, BIG>), grid,
                  dim3((BM / WM) * (BN / WN) * 64 * KS), lds, st, a);
  SRX_CHECK_LAUNCH("gconv_kernel");
  if (p.split > 1) {
    hipLaunchKernelGGL((tail_fixup_kernel<BM + XR, BN>), dim3(p.tail * (BN / 16)), dim3(256), 0, st, a);
    SRX_CHECK_LAUNCH("tail_fixup_kernel");
  }
  return SRX_OK;
}

template <int BM, int BN, int WM, int WN, int XR, int PR = 0, int KS = 1>
int launch_gconv_multi(const GMulti& m, size_t lds, hipStream_t st) {
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gconv_multi_kernel<BM, BN, WM, WN, XR, PR, KS>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  });
  char nm[64];
  double fl = 0.0;
  if (srx_prof_on()) {
    snprintf(nm, sizeof(nm), "gconv_multi_kernel<%d, %d, %d, %d, %d, %d, %d>", BM, BN, WM, WN, XR, PR, KS);
    for (int i = 0; i < m.n; ++i) fl += 2.0 * m.g[i].M * m.g[i].Cn * m.g[i].K;
  }
  SRX_LAUNCH_PROF(nm, fl, (gconv_multi_kernel<BM, BN, WM, WN, XR, PR, KS>), dim3(m.first[m.n]), dim3((BM / WM) * (BN / WN) * 64 * KS),
                  lds, st, m);
  SRX_CHECK_LAUNCH("gconv_multi_kernel");
  return SRX_OK;
}

template <int BM, int BN, int WM, int WN, int XR, int PR>
int launch_gconv_s2f(const GFused& f, dim3 grid, size_t lds, double fl, hipStream_t st) {
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gconv_s2f_kernel<BM, BN, WM, WN, XR, PR>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  });
  char nm[64];
  if (srx_prof_on()) snprintf(nm, sizeof(nm), "gconv_s2f_kernel<%d, %d, %d, %d, %d, %d>", BM, BN, WM, WN, XR, PR);
  SRX_LAUNCH_PROF(nm, fl, (gconv_s2f_kernel<BM, BN, WM, WN, XR, PR>), grid, dim3((BM / WM) * (BN / WN) * 64), lds, st, f);
  SRX_CHECK_LAUNCH("gconv_s2f_kernel");
  return SRX_OK;
}

// Dispatch: the run-time (BM, BN, KS, PR) of a plan to the one instantiation of family F the table lists for it -- and only the
// listed ones are instantiated (every gconv_kernel costs seconds of build time).  `args` are the launcher's own.
struct TileKey { int bm, bn, ks, pr; };

// instantiation (row I, PR, KS) of family F: launched (status in rc) if the table has it and k names it; false: not this one
template <int F, int I, int PR, int KS, class... A>
bool launch_if(const TileKey& k, int& rc, const A&... args) {
  constexpr Tile t = kTiles[I];
  if constexpr ((t.ks[F][PR] & KS) != 0) {
    if (k.bm != t.BM || k.bn != t.BN || k.ks != KS || k.pr != PR) return false;
    if constexpr (F == F_MULTI) rc = launch_gconv_multi<t.BM - t.XR, t.BN, t.WM, t.WN, t.XR, PR, KS>(args...);
    else if constexpr (F == F_S2F) rc = launch_gconv_s2f<t.BM - t.XR, t.BN, t.WM, t.WN, t.XR, PR>(args...);
    else rc = launch_gconv<t.BM - t.XR, t.BN, t.WM, t.WN, KS, t.XR, PR, F == F_BIG>(args...);
    return true;
  }
  return false;
}
// every (row, PR, KS) the table could list, J = (row * 4 + PR) * 3 + log2 KS; false: family F has no kernel for k, nothing launched
using Listable = std::make_integer_sequence<int, NTILES * 12>;
template <int F, int... J, class... A>
bool launch_tile(std::integer_sequence<int, J...>, const TileKey& k, int& rc, const A&... args) {
  return (launch_if<F, J / 12, J / 3 % 4, 1 << J % 3>(k, rc, args...) || ...);
}

// Tile for a multi-problem launch.  The stride-parity classes of a data gradient have the same M but
// 1x..4x different K, and their strided outputs cannot take the split-K fix-up path, so balance comes
// from the tile size alone: every candidate's workgroups are list-scheduled heavy-first (the order
// run_gconv_multi launches them in) over the CUs and the shortest makespan wins.  A forced plan (srx_conv2d_force_plan) costs 0;
// one without a gconv_multi_kernel instantiation returns -1 with the message set.
float multi_tile(const GMulti& m, int Cnp, int& BM, int& BN, int& KS, bool bf16 = false) {
  const int P = srx_plan_cus();
  const int pr = bf16 ? 1 : 0;
  float best = 1e30f;
  BM = 128; BN = Cnp == 32 ? 32 : 64; KS = 1;
  int fbm, fbn, fsp, fks;
  if (forced_plan(fbm, fbn, fsp, fks)) {
    if (const char* why = forced_tile_refusal(F_MULTI, fbm, fbn, fks, Cnp, bf16)) {
      srx_set_error("conv2d_bwd_data: forced plan %d x %d (KS %d) refused for gconv_multi_kernel: %s (%d padded columns, %s products)",
                    fbm, fbn, fks, why, Cnp, bf16 ? "bf16" : "fp32");
      return -1.f;
    }
    BM = fbm; BN = fbn; KS = tile_ks(*find_tile(fbm, fbn), F_MULTI, pr, fks == 2);
    return 0.f;
  }
  std::vector<float> heap;
  // every tile on one wave group; then, last, the tiles that have two (64 x 64: the k-chunks of a tile dealt to two wave
  // groups -- half the chain, one workgroup per CU)
  for (int i = 0; i < 2 * NTILES; ++i) {
    const Tile& tile = kTiles[i % NTILES];
    const int bm = tile.BM, bn = tile.BN, ks = 1 + i / NTILES;
    if (!(tile.ks[F_MULTI][pr] & ks) || !columns_fit(Cnp, bn)) continue;
    if (ks == 2 && (srx_dev().s2_mode & 2)) continue;
    heap.assign(P, 0.f);  // min-heap of CU finish times
    auto later = [](float x, float y) { return x > y; };
    float makespan = 0.f;
    for (int pass = 4; pass >= 1; --pass)  // heavy-first: K of a class is 1..4 tap groups; order by chunk count
      for (int c = 0; c < m.n; ++c) {
        const int kch = m.g[c].Kp / BK;
        int rank = 1;
        for (int o = 0; o < m.n; ++o) rank += (m.g[o].Kp < m.g[c].Kp);
        if (rank != pass) continue;
        // (see make_plan; the two-group tile: half the chain at 0.8, and a fixed cost nothing overlaps -- set-up and fold of a
        // 512-thread workgroup that has the CU to itself: measured ~6.5 us on the discriminator's layers)
        const float t = tile_us(bm, bn, kch, 1.0f, bf16);
        const float cost = ks == 2 ? 6.5f + 0.5f * t / 0.8f : 1.0f + t / tile.eff;
        const int tiles = (int)srx_cdiv(m.g[c].M, bm) * (int)srx_cdiv(m.g[c].Cn, bn);
        for (int t = 0; t < tiles; ++t) {
          std::pop_heap(heap.begin(), heap.end(), later);
          heap.back() += cost;
          if (heap.back() > makespan) makespan = heap.back();
          std::push_heap(heap.begin(), heap.end(), later);
        }
      }
    if (makespan < best) { best = makespan; BM = bm; BN = bn; KS = ks; }
  }
  return best;
}

// all problems use tile (BM, BN); no K split.  Problems are launched heaviest (largest K) first.
int run_gconv_multi(GMulti& m, int BM, int BN, int KS, hipStream_t st, int precision = 0) {
  std::stable_sort(m.g, m.g + m.n, [](const GArgs& x, const GArgs& y) { return x.Kp > y.Kp; });
  int maxk = 0;
  m.first[0] = 0;
  for (int i = 0; i < m.n; ++i) {
    GArgs& a = m.g[i];
    a.kchunks = a.Kp / BK;
    a.mtiles = (int)srx_cdiv(a.M, BM);
    a.kc_per_split = a.kchunks;
    a.tail_split = 1;
    a.ws = nullptr;
    const int tiles = a.mtiles * (int)srx_cdiv(a.Cn, BN);
    a.full_tiles = tiles;
    m.first[i + 1] = m.first[i] + tiles;
    if (a.kchunks > maxk) maxk = a.kchunks;
  }
  const int pr = precision ? 1 : 0;  // (bf16 products, round 4: the stride-parity classes of a strided data gradient too)
  const size_t lds = gconv_lds_bytes(BM, BN, KS, pr, maxk);
  if (lds > 160 * 1024) SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d: K range needs %zu bytes of LDS", lds);
  int rc = SRX_OK;
  if (launch_tile<F_MULTI>(Listable{}, {BM, BN, KS, pr}, rc, m, lds, st)) return rc;
  SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_bwd_data: no%s gconv_multi_kernel for tile %d x %d", pr ? " bf16" : "", BM, BN);
}

// ---- the fused-class strided data gradient (gconv_s2f_kernel) ----
// Eligible: 2..4 non-empty classes on ONE M grid (extents multiples of the stride), whole chunks per tap, plain gather.
bool s2f_eligible(const srx_conv2d_t* d, const BwdClass* cls, int nc) {
  if (nc < 2 || nc > 4 || d->shuffle || d->up || d->precision > 1) return false;
  if (bwd_ck(d) % BK != 0 || pad_rows(d->Cin) % 64 != 0) return false;
  for (int i = 0; i < nc; ++i)
    if (cls[i].K == 0 || cls[i].Hm != cls[0].Hm || cls[i].Wm != cls[0].Wm || cls[i].Hm <= 0 || cls[i].Wm <= 0) return false;
  return true;
}

// tile of the fused launch and its estimated time (the model of make_plan / multi_tile: one workgroup slot per CU); a
// workgroup pays one set-up, one pipeline fill and an epilogue per class
float s2f_tile(const srx_conv2d_t* d, const BwdClass* cls, int nc, int& BM, int& BN) {
  const int P = srx_plan_cus();
  const bool bf16 = d->precision != 0;
  const int Cnp = pad_rows(d->Cin);
  const int M = d->N * cls[0].Hm * cls[0].Wm;
  int chunks = 0;
  for (int i = 0; i < nc; ++i) chunks += cls[i].K / BK;
  float best = 1e30f;
  BM = 0; BN = 0;
  for (const Tile& tile : kTiles) {
    const int bm = tile.BM, bn = tile.BN;
    if (!tile.ks[F_S2F][bf16 ? 1 : 0] || Cnp % bn != 0) continue;
    const float t = tile_us(bm, bn, chunks, tile.eff, bf16);
    const int64_t tiles = srx_cdiv(M, bm) * (Cnp / bn);
    const float cost = (float)srx_cdiv(tiles, P) * (1.5f + 0.7f * nc * (bm * bn / 8192.0f) + t);
    if (cost < best) { best = cost; BM = bm; BN = bn; }
  }
  return best;
}

// `shared`: the launch arguments of any one class (gconv_multi's), `wpk` / `wfloats`: the whole packed data-gradient buffer
int run_gconv_s2f(const srx_conv2d_t* d, const GArgs& shared, const BwdClass* cls, int nc, const float* wpk, size_t wfloats,
                  int BM, int BN, hipStream_t st) {
  GFused f{};
  f.g = shared;
  f.g.w = wpk;
  if (wfloats * sizeof(float) >= 0xfffffff0ull) SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_bwd_data: packed weights above 4 GiB");
  f.g.w_bytes = (unsigned)(wfloats * sizeof(float));
  f.g.mtiles = (int)srx_cdiv(shared.M, BM);
  f.nclass = nc;
  f.cpt = bwd_ck(d) / BK;
  int pos = 0;
  double fl = 0.0;
  for (int i = 0; i < nc; ++i) {
    S2Class& k = f.c[i];
    k.nth = cls[i].nth; k.ntw = cls[i].ntw; k.dh0 = cls[i].dminh; k.dw0 = cls[i].dminw;
    k.chunks = cls[i].K / BK; k.pstart = pos;
    k.oh_off = cls[i].ph; k.ow_off = cls[i].pw;
    k.wbase = (unsigned)(cls[i].woff * sizeof(float)); k.kpb = (unsigned)(cls[i].Kp * sizeof(float));
    pos += (int)srx_roundup(k.chunks, 3);
    fl += 2.0 * shared.M * shared.Cn * cls[i].K;
  }
  f.ptotal = pos;
  const int Cnp = pad_rows(d->Cin);
  const int pr = d->precision != 0 ? 1 : 0;
  const size_t lds = s2f_lds_bytes(BM, BN, pr, pos);
  if (lds > 160 * 1024) SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_bwd_data: K range needs %zu bytes of LDS", lds);
  const dim3 grid((unsigned)(f.g.mtiles * (Cnp / BN)));
  int rc = SRX_OK;
  if (launch_tile<F_S2F>(Listable{}, {BM, BN, 1, pr}, rc, f, grid, lds, fl, st)) return rc;
  SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_bwd_data: internal: no fused-class instantiation for tile %d x %d", BM, BN);
}

// The launch of a strided data gradient whose stride-parity classes are m's problems: one gconv_s2f_kernel launch (fused) or one
// gconv_multi_kernel launch, on tile BM x BN with KS wave groups -- the cost model's choice, or the forced one
// (srx_conv2d_force_s2 / srx_conv2d_force_plan).  A forced form the layer has no kernel for is refused here, before any launch;
// srx_conv2d_plan reports what this returns.
int strided_dgrad_plan(const srx_conv2d_t* d, const BwdClass* cls, int nc, const GMulti& m, int& BM, int& BN, int& KS, bool& fused) {
  ConvForce& f = conv_force();
  const int mode = f.s2[0].load(std::memory_order_relaxed);
  const bool bf16 = d->precision != 0;
  const int Cnp = pad_rows(d->Cin);
  const bool eligible = m.n == nc && s2f_eligible(d, cls, nc);
  fused = false;
  if (mode == 2) {
    if (!eligible)
      SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_bwd_data: forced gconv_s2f_kernel refused: the layer needs 2..4 non-empty stride-parity "
                                  "classes on one grid (extents multiples of the stride), Cout and Cin in whole chunks, no shuffle / upsample");
    int bm = f.s2[1].load(std::memory_order_relaxed), bn = f.s2[2].load(std::memory_order_relaxed);
    if (bm == 0) {
      s2f_tile(d, cls, nc, bm, bn);
    } else {
      const bool known = has_tile(F_S2F, bm, bn, 1, bf16 ? 1 : 0);
      if (!known || Cnp % bn != 0)
        SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_bwd_data: forced gconv_s2f_kernel tile %d x %d refused: %s (%d padded columns, %s products)",
                 bm, bn, known ? "the tile's columns do not divide the layer's" : "no instantiation of this tile", Cnp, bf16 ? "bf16" : "fp32");
    }
    BM = bm; BN = bn; KS = 1; fused = true;
    return SRX_OK;
  }
  const float t_multi = multi_tile(m, Cnp, BM, BN, KS, bf16);
  if (t_multi < 0.f) return SRX_E_UNSUPPORTED;
  if (mode == 0 && eligible) {  // all classes of a tile in one workgroup, when that is the shorter launch
    int fbm, fbn;
    const float t_fused = s2f_tile(d, cls, nc, fbm, fbn);
    if (fbm > 0 && (0.97f * t_fused < t_multi || (srx_dev().s2_mode & 4))) {  // (a tie goes to the fused launch: measured)
      BM = fbm; BN = fbn; KS = 1; fused = true;
    }
  }
  return SRX_OK;
}

int run_gconv(GArgs& a, const Plan& p, float* ws, size_t ws_floats, hipStream_t st, int precision = 0) {
  if (p.refused) return SRX_E_UNSUPPORTED;  // (a forced plan the layer has no kernel for: make_plan set the message)
  a.kchunks = a.Kp / BK;
  const size_t need = plan_ws_floats(p);
  if (need && (!ws || need > ws_floats))
    SRX_FAIL(SRX_E_WORKSPACE, "conv2d: split-K workspace %zu < %zu floats", ws_floats, need);
  if (p.split > 1 && !a.linear_out) SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d: internal: split plan on a strided output");
  a.mtiles = p.mtiles;
  a.kc_per_split = p.kc_per_split;
  a.full_tiles = p.full;
  a.tail_split = p.split;
  a.ws = ws;
  int rc = SRX_OK;
  if (a.big) {  // whole-frame calls: fp32, bf16 or fp16 products, no K split (plans made with `big` ask for nothing else)
    if (p.split > 1) SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d: internal: split plan on a call above 2^24 pixels");
    if (launch_tile<F_BIG>(Listable{}, {p.BM, p.BN, p.ks, precision == 3 ? 3 : precision ? 1 : 0}, rc, a, p, st)) return rc;
    SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d: no whole-frame kernel for tile %dx%d", p.BM, p.BN);
  }
  // (precision 2, bf16 storage: the tensors hold bf16, a chunk is 64 k-values; 3, fp16 products: the input conv of fp16 inference)
  if (launch_tile<F_GCONV>(Listable{}, {p.BM, p.BN, p.ks, precision}, rc, a, p, st)) return rc;
  static const char* const arith[4] = {"fp32", "bf16", "bf16-storage", "fp16"};
  SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d: no %s kernel for tile %dx%d", arith[precision & 3], p.BM, p.BN);
}

void set_mgrid(GArgs& a, int N, int Hm, int Wm) {
  a.N = N; a.Hm = Hm; a.Wm = Wm; a.HmWm = Hm * Wm; a.M = N * Hm * Wm;
  a.inv_HmWm = 1.0f / (float)a.HmWm;
  a.inv_Wm = 1.0f / (float)Wm;
}

// above 2^24 pixels or 4 GiB of input: the BIG instantiations (64-bit tile bases, exact index division)
bool is_big(const srx_conv2d_t* d) { return !small_enough(d); }

Plan fwd_plan(const srx_conv2d_t* d, const Geo& g) {
  return make_plan(d->N * g.Ho * g.Wo, g.Cnp, g.Kp / BK, !d->shuffle, d->precision != 0, is_big(d));
}

Plan bwd_plan(const srx_conv2d_t* d, const BwdClass& c) {
  return make_plan(d->N * c.Hm * c.Wm, pad_rows(d->Cin), c.Kp / BK, d->stride == 1, d->precision != 0);
}

int stat_rows_for(const srx_conv2d_t* d) {
  if (srx_rt36_applicable(d)) return srx_rt36_rows(d);
  const Geo g = fwd_geo(d);
  return fwd_plan(d, g).mtiles;
}

}  // namespace

extern "C" size_t srx_conv2d_packed_fwd_floats(const srx_conv2d_t* d) {
  if (check_desc(d)) return 0;
  const Geo g = fwd_geo(d);
  return (size_t)g.Cnp * g.Kp;
}

extern "C" size_t srx_conv2d_packed_bwd_floats(const srx_conv2d_t* d) {
  if (check_desc(d)) return 0;
  if (d->stride > 4) return 0;
  BwdClass cls[16];
  size_t total;
  bwd_classes(d, cls, total);
  return total;
}

extern "C" size_t srx_conv2d_fwd_ws_floats(const srx_conv2d_t* d) {
  if (check_desc(d)) return 0;
  if (srx_rt36_applicable(d)) return 0;
  const Geo g = fwd_geo(d);
  return plan_ws_floats(fwd_plan(d, g));
}

extern "C" size_t srx_conv2d_bwd_data_ws_floats(const srx_conv2d_t* d) {
  if (check_desc(d)) return 0;
  if (d->up == 2) { const srx_conv2d_t h = upsampled_desc(d); return upsampled_floats(d) + srx_conv2d_bwd_data_ws_floats(&h); }
  if (d->stride != 1) return 0;
  BwdClass cls[16];
  size_t total;
  bwd_classes(d, cls, total);
  return plan_ws_floats(bwd_plan(d, cls[0]));  // (also covers srx_conv2d_bwd_data_act, which never takes the row-tile path)
}

extern "C" int srx_conv2d_stat_rows(const srx_conv2d_t* d) {
  if (check_desc(d)) return 0;
  return stat_rows_for(d);
}

// which: 0 = forward, 1 = data gradient.  out[6] = {BM, BN, tail split, workgroups, KS, multi}
// (multi = 1: the stride-parity classes run as one gconv_multi_kernel launch; 2: as one gconv_s2f_kernel launch)
extern "C" int srx_conv2d_plan(const srx_conv2d_t* d, int which, int* out) {
  if (int rc = check_desc(d)) return rc;
  SRX_REQUIRE(out, "conv2d_plan: null pointer");
  Plan p;
  int multi = 0;
  if (srx_rt36_applicable(d)) {  // 36-pixel row tiles (rowtile.hip), forward and data gradient alike
    const int rows = srx_rt36_rows(d);
    out[0] = (int)((int64_t)d->N * d->H * d->W / rows); out[1] = 64; out[2] = 1; out[3] = rows; out[4] = 1; out[5] = 0;
    return SRX_OK;
  }
  if (which == 0) {
    p = fwd_plan(d, fwd_geo(d));
    if (p.refused) return SRX_E_UNSUPPORTED;
  } else {
    SRX_REQUIRE(d->stride <= 4, "conv2d_plan: stride > 4 unsupported");
    BwdClass cls[16];
    size_t total;
    const int nc = bwd_classes(d, cls, total);
    if (d->stride > 1 && nc <= 4) {
      GMulti m{};
      for (int i = 0; i < nc; ++i) {
        if (cls[i].K == 0 || cls[i].Hm <= 0 || cls[i].Wm <= 0) continue;
        m.g[m.n].M = d->N * cls[i].Hm * cls[i].Wm;
        m.g[m.n].Cn = d->Cin;
        m.g[m.n++].Kp = cls[i].Kp;
      }
      p = Plan{};
      bool fused = false;
      if (int rc = strided_dgrad_plan(d, cls, nc, m, p.BM, p.BN, p.ks, fused)) return rc;
      p.split = 1; p.tail = 0;
      if (fused) {  // (multi = 2: all classes of a tile in one workgroup, gconv_s2f_kernel)
        p.full = (int)srx_cdiv(m.g[0].M, p.BM) * (pad_rows(d->Cin) / p.BN);
        multi = 2;
      } else {
        for (int i = 0; i < m.n; ++i) p.full += (int)srx_cdiv(m.g[i].M, p.BM) * (int)srx_cdiv(d->Cin, p.BN);
        multi = 1;
      }
    } else {
      p = bwd_plan(d, cls[0]);
      if (p.refused) return SRX_E_UNSUPPORTED;
    }
  }
  out[0] = p.BM; out[1] = p.BN; out[2] = p.split; out[3] = p.full + p.tail * p.split; out[4] = p.ks; out[5] = multi;
  return SRX_OK;
}

extern "C" int srx_conv2d_force_plan(int bm, int bn, int split, int ks) {
  SRX_REQUIRE((bm == 0 && bn == 0 && split == 0 && ks == 0) ||
              (tile_sides_known(F_GCONV, bm, bn) && split >= 1 && split <= 16 && (ks == 1 || ks == 2)),
              "conv2d_force_plan: (0, 0, 0, 0) or BM 64 / 128 / 144 / 256, BN 32 / 64 / 128, split 1..16, KS 1 / 2");
  ConvForce& f = conv_force();
  f.plan[1].store(0);  // (off while the others change)
  f.plan[0].store(bm); f.plan[2].store(split); f.plan[3].store(ks); f.plan[1].store(bn);
  return SRX_OK;
}

extern "C" int srx_conv2d_force_s2(int mode, int bm, int bn) {
  SRX_REQUIRE(((mode == 0 || mode == 1) && bm == 0 && bn == 0) ||
              (mode == 2 && ((bm == 0 && bn == 0) || tile_sides_known(F_S2F, bm, bn))),
              "conv2d_force_s2: (0, 0, 0), (1, 0, 0) or (2, BM 64 / 128 / 144, BN 64 / 128) -- (2, 0, 0): the model's fused tile");
  ConvForce& f = conv_force();
  f.s2[0].store(0);
  f.s2[1].store(bm); f.s2[2].store(bn); f.s2[0].store(mode);
  return SRX_OK;
}

extern "C" int srx_wgrad_force(int lin, int nsplit) {
  SRX_REQUIRE(lin >= -1 && lin <= 1 && nsplit >= 0 && nsplit <= 64, "wgrad_force: LIN -1 / 0 / 1, 0..64 row splits");
  ConvForce& f = conv_force();
  f.wg[0].store(lin); f.wg[1].store(nsplit); f.wg_rows.store(nsplit);
  return SRX_OK;
}

extern "C" int srx_wgrad_force_kernels(int dma, int rows, int reduce) {
  SRX_REQUIRE(dma >= -1 && dma <= 1 && rows >= -1 && rows <= 1 && reduce >= -1 && reduce <= 1,
              "wgrad_force_kernels: DMA staging, image-row kernel, row-wise reduction: each -1 / 0 / 1");
  ConvForce& f = conv_force();
  f.wk[0].store(dma); f.wk[1].store(rows); f.wk[2].store(reduce);
  return SRX_OK;
}

static int conv_fwd_impl(const srx_conv2d_t* d, const float* x, const float* wpk, const float* bias, const float* residual,
                         float out_scale, float* y, float* bn_partials, float* ws, size_t ws_floats, void* stream) {
  if (int rc = check_desc(d)) return rc;
  SRX_REQUIRE(x && wpk && y, "conv2d_fwd: null pointer");
  if (residual && d->shuffle) SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_fwd: residual with PixelShuffle is not implemented");
  hipStream_t st = srx_stream(stream);
  if (srx_thin_fwd_applicable(d) && !bn_partials && !residual && d->up != 2) return srx_thin_fwd(d, x, wpk, bias, y, d->Cout, st);
  if (srx_first3_fwd_applicable(d) && d->precision != 3 && !bn_partials && !residual && d->act != SRX_ACT_PRELU)
    return srx_first3_fwd(d, x, wpk, fwd_geo(d).Kp, bias, y, st);
  if (srx_rt36_applicable(d) && out_scale == 1.f)
    return srx_rt36_run(d, x, wpk, bias, residual, y, bn_partials, d->act, d->slope, st);
  if (srx_rt36_applicable(d)) SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_fwd_residual: out_scale != 1 on the 36-pixel row tile");
  const Geo g = fwd_geo(d);
  GArgs a{};
  a.in = x; a.w = wpk; a.bias = bias; a.part = nullptr;
  set_mgrid(a, d->N, g.Ho, g.Wo);
  a.up = d->up == 2;
  a.Hi = (a.up ? 2 : 1) * d->H; a.Wi = (a.up ? 2 : 1) * d->W; a.Ci = d->Cin_s;
  a.in_stride = d->stride; a.nth = d->KH; a.ntw = d->KW; a.dh0 = -d->pad; a.dw0 = -d->pad;
  a.Ck = g.Ck; a.K = g.K; a.Kp = g.Kp;
  a.Cn = d->Cout;
  a.act = d->act;
  a.slope = d->act == SRX_ACT_RELU ? 0.f : (d->act == SRX_ACT_LRELU ? d->slope : 1.f);  // v > 0 ? v : v * slope
  a.in_shuffle = 0;
  if (d->shuffle) {
    a.out_shuffle = g.cps; a.Cs = d->Cout; a.Ho = 2 * g.Ho; a.Wo = 2 * g.Wo; a.Co = d->Cout_s;
    a.out_stride = 2; a.oh_off = 0; a.ow_off = 0; a.linear_out = 0;
  } else {
    a.out_shuffle = 0; a.Cs = (int)srx_roundup(d->Cout, 4); a.Ho = g.Ho; a.Wo = g.Wo; a.Co = d->Cout_s;
    a.out_stride = 1; a.oh_off = 0; a.ow_off = 0; a.linear_out = 1;
  }
  a.part = bn_partials;
  a.out = y;
  a.add = residual;
  a.oscale = out_scale;
  a.add_ld = a.Co; a.add_hi = 0x7fffffff; a.ascale = 1.f;
  a.in_bytes = (size_t)d->N * d->H * d->W * d->Cin_s * sizeof(float);
  a.w_bytes = (unsigned)((size_t)g.Cnp * g.Kp * sizeof(float));
  a.big = is_big(d);
  a.in_margin = a.up ? 0u : 4u * (unsigned)((d->pad * a.Wi + d->pad) * a.Ci);  // taps start `pad` rows and columns before the centre
  return run_gconv(a, fwd_plan(d, g), ws, ws_floats, st, d->precision);
}

extern "C" int srx_conv2d_fwd(const srx_conv2d_t* d, const float* x, const float* wpk, const float* bias, float* y,
                              float* bn_partials, float* ws, size_t ws_floats, void* stream) {
  return conv_fwd_impl(d, x, wpk, bias, nullptr, 1.f, y, bn_partials, ws, ws_floats, stream);
}

// The forward of a 64 -> <= 4 channel layer (the generator's output conv, srgan/generator.py:58) whose INPUT is a bf16 NHWC
// tensor -- the end of the bf16-native inference chain (c64.hip); precision must be 2 (bf16 products), y is fp32.
extern "C" int srx_conv2d_fwd_bf16in(const srx_conv2d_t* d, const void* x_bf16, const float* wpk, const float* bias, float* y,
                                     void* stream) {
  if (int rc = check_desc(d)) return rc;
  SRX_REQUIRE(x_bf16 && wpk && y, "conv2d_fwd_bf16in: null pointer");
  if (!srx_thin_fwd_applicable(d) || d->precision != 2 || d->up == 2)
    SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_fwd_bf16in: 64 -> <= 4 channel layers with precision = 2 only");
  SRX_REQUIRE((int64_t)d->N * d->H * d->W * 128 < (1LL << 32), "conv2d_fwd_bf16in: input above 4 GiB; tile the image");
  return srx_thin_fwd(d, static_cast<const float*>(x_bf16), wpk, bias, y, d->Cout, srx_stream(stream), 1);
}

extern "C" int srx_conv2d_fwd_residual(const srx_conv2d_t* d, const float* x, const float* wpk, const float* bias,
                                       const float* residual, float out_scale, float* y, float* ws, size_t ws_floats,
                                       void* stream) {
  SRX_REQUIRE(residual, "conv2d_fwd_residual: null residual");
  return conv_fwd_impl(d, x, wpk, bias, residual, out_scale, y, nullptr, ws, ws_floats, stream);
}

static int conv_bwd_data_impl(const srx_conv2d_t* d, const float* dy, const float* wpk_bwd, float* dx, int accumulate,
                              const float* act_out, float act_slope, int c_lo, int c_hi, float* ws, size_t ws_floats,
                              void* stream, const float* addend = nullptr, int addend_ld = 0, int addend_channels = 0,
                              float addend_scale = 1.f, float out_scale = 1.f) {
  if (int rc = check_desc(d)) return rc;
  SRX_REQUIRE(d->precision != 3, "conv2d: precision 3 (fp16 products) is forward-only");
  SRX_REQUIRE(dy && wpk_bwd && dx, "conv2d_bwd_data: null pointer");
  SRX_REQUIRE(d->stride <= 4, "conv2d_bwd_data: stride > 4 unsupported");
  if (addend_ld == 0) addend_ld = d->Cin_s;
  if (addend_channels == 0) addend_channels = 0x7fffffff;
  const bool plain_addend = addend_ld == d->Cin_s && addend_channels >= d->Cin && addend_scale == 1.f && out_scale == 1.f;
  if (!plain_addend) {
    SRX_REQUIRE(addend && !accumulate, "conv2d_bwd_data_ex: addend stride / channels / scales without an addend");
    SRX_REQUIRE(addend_ld >= 4 && addend_ld % 4 == 0 && (addend_channels % 4 == 0 || addend_channels >= d->Cin),
                "conv2d_bwd_data_ex: the addend's stride and channel count must be made of whole quads");
    // the epilogue reads min(addend_channels, Cin rounded up to a quad) floats of every addend row: more than the
    // row stride would walk into the next pixel and, on the last rows, past the end of the addend tensor
    SRX_REQUIRE(addend_channels > 0 && (addend_channels < d->Cin ? addend_channels : (int)srx_roundup(d->Cin, 4)) <= addend_ld,
                "conv2d_bwd_data_ex: the addend has %d channels per row but a row stride of %d floats",
                addend_channels < d->Cin ? addend_channels : (int)srx_roundup(d->Cin, 4), addend_ld);
  }
  if (d->up == 2) {
    if (accumulate || act_out || addend)
      SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_bwd_data: up = 2 with accumulate / an addend / a folded activation");
    SRX_REQUIRE(small_enough(d), "conv2d_bwd_data: up = 2 above 2^24 pixels (the 2x2 block sum keeps 32-bit offsets)");
    const srx_conv2d_t h = upsampled_desc(d);
    const size_t tmp = upsampled_floats(d);
    SRX_REQUIRE(ws && ws_floats >= tmp + srx_conv2d_bwd_data_ws_floats(&h), "conv2d_bwd_data: workspace too small for up = 2");
    if (int rc = conv_bwd_data_impl(&h, dy, wpk_bwd, ws, 0, nullptr, 1.f, 0, 0, ws + tmp, ws_floats - tmp, stream)) return rc;
    return srx_upsample_nearest2x_bwd(ws, dx, d->N, d->H, d->W, d->Cin_s, stream);
  }
  // (the row-tile kernel has neither a masked epilogue nor a strided / scaled addend)
  const bool rt36 = srx_rt36_applicable(d) && !act_out && plain_addend;
  if (addend && (accumulate || d->stride != 1 || srx_thin_dgrad_applicable(d) || d->up == 2))
    SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_bwd_data_add: stride-1 layers without accumulate only");
  if (accumulate && (d->stride != 1 || srx_thin_dgrad_applicable(d) || rt36))
    SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_bwd_data: accumulate is implemented for stride-1 layers on the generic kernel only");
  if (act_out && (srx_thin_dgrad_applicable(d) || (d->stride != 1 && accumulate)))
    SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_bwd_data_act: layers on the generic kernel only (strided ones without accumulate)");
  if (act_out) SRX_REQUIRE(c_lo >= 0 && c_lo < c_hi && c_lo % 4 == 0 && (c_hi % 4 == 0 || c_hi >= d->Cin) && c_lo < d->Cin_s,
                           "conv2d_bwd_data_act: the masked channel range must be made of whole quads inside the row");
  hipStream_t st = srx_stream(stream);
  if (srx_thin_dgrad_applicable(d)) return srx_thin_fwd(d, dy, wpk_bwd, nullptr, dx, d->Cin, st);
  const Geo g = fwd_geo(d);
  BwdClass cls[16];
  size_t total;
  const int nc = bwd_classes(d, cls, total);
  if (rt36)  // 3x3 / stride 1 / pad 1: one class, same geometry as the forward, flipped taps
    return srx_rt36_run(d, dy, wpk_bwd + cls[0].woff, nullptr, addend, dx, nullptr, SRX_ACT_NONE, 0.f, st);
  bool any_empty = false;
  for (int i = 0; i < nc; ++i) any_empty |= (cls[i].K == 0);
  const size_t dy_bytes = (size_t)d->N * g.Ho * g.Wo * (d->shuffle ? 4 : 1) * d->Cout_s * sizeof(float);
  SRX_REQUIRE(small_enough(d) && dy_bytes < 0xfffffff0ull,
              "conv2d_bwd_data: more than 2^24 pixels or 4 GiB per tensor (data gradients keep 32-bit offsets: training crops, not whole frames)");

  // every launch is planned (and a refused forced plan reported) before dx is touched
  GMulti multi{};
  GArgs single[16];
  Plan single_plan[16];
  int ns = 0;
  for (int i = 0; i < nc; ++i) {
    const BwdClass& c = cls[i];
    if (c.K == 0 || c.Hm <= 0 || c.Wm <= 0) continue;
    GArgs a{};
    a.in = dy; a.w = wpk_bwd + c.woff; a.bias = nullptr; a.part = nullptr;
    set_mgrid(a, d->N, c.Hm, c.Wm);
    a.Hi = g.Ho; a.Wi = g.Wo; a.Ci = d->Cout_s;
    a.in_stride = 1; a.nth = c.nth; a.ntw = c.ntw; a.dh0 = c.dminh; a.dw0 = c.dminw;
    a.Ck = bwd_ck(d);
    a.K = c.K; a.Kp = c.Kp;
    a.in_shuffle = g.cps;
    a.Cn = d->Cin; a.Cs = (int)srx_roundup(d->Cin, 4);
    a.Ho = d->H; a.Wo = d->W; a.Co = d->Cin_s;
    a.out_stride = d->stride; a.oh_off = c.ph; a.ow_off = c.pw;
    a.out_shuffle = 0;
    a.act = SRX_ACT_NONE; a.slope = 1.f;
    a.linear_out = (d->stride == 1);
    a.out = dx;
    a.in_bytes = dy_bytes;
    a.big = 0;
    {  // the most negative tap of this class: dminh rows / dminw columns (in units of the gradient tensor's pixels, x2 when shuffled)
      const long long o = g.cps ? ((2LL * c.dminh) * (2 * a.Wi) + 2LL * c.dminw) * a.Ci : ((long long)c.dminh * a.Wi + c.dminw) * a.Ci;
      // A class's grid (Hm x Wm) may be larger than the gradient image (pad = 0: the last input rows / columns see no output):
      // such rows' "centre" lies past their image, so a LATER row (the next image's first) can sit lower in memory -- the
      // tile's base must leave room for that overshoot too
      const long long over_h = std::max(0, c.Hm - a.Hi), over_w = std::max(0, c.Wm - a.Wi);
      const long long over = g.cps ? ((2 * over_h) * (2LL * a.Wi) + 2 * over_w) * a.Ci : (over_h * a.Wi + over_w) * a.Ci;
      a.in_margin = (unsigned)(((o < 0 ? -o : 0) + over) * 4);
    }
    a.w_bytes = (unsigned)((size_t)pad_rows(d->Cin) * c.Kp * sizeof(float));
    a.add = accumulate ? dx : addend;
    a.oscale = out_scale;
    a.add_ld = accumulate ? a.Co : addend_ld; a.add_hi = accumulate ? 0x7fffffff : addend_channels;
    a.ascale = accumulate ? 1.f : addend_scale;
    if (act_out) { a.mask = act_out; a.mask_slope = act_slope; a.mask_lo = c_lo; a.mask_hi = c_hi; }
    if (d->stride != 1 && nc <= 4) {
      multi.g[multi.n++] = a;
    } else {  // stride 1, or stride > 2: one launch per class (with the layer's arithmetic: bf16 products under precision = 1)
      single_plan[ns] = bwd_plan(d, c);
      if (single_plan[ns].refused) return SRX_E_UNSUPPORTED;
      single[ns++] = a;
    }
  }
  int bm = 0, bn = 0, ks = 1;
  bool fused = false;
  if (multi.n > 0)
    if (int rc = strided_dgrad_plan(d, cls, nc, multi, bm, bn, ks, fused)) return rc;
  if (any_empty) {
    if (hipMemsetAsync(dx, 0, (size_t)d->N * d->H * d->W * d->Cin_s * sizeof(float), st) != hipSuccess)
      SRX_FAIL(SRX_E_HIP, "conv2d_bwd_data: memset failed");
  }
  for (int i = 0; i < ns; ++i)
    if (int rc = run_gconv(single[i], single_plan[i], ws, ws_floats, st, d->precision)) return rc;
  if (multi.n > 0) {
    if (fused) return run_gconv_s2f(d, multi.g[0], cls, nc, wpk_bwd, total, bm, bn, st);
    if (int rc = run_gconv_multi(multi, bm, bn, ks, st, d->precision)) return rc;
  }
  return SRX_OK;
}

extern "C" int srx_conv2d_bwd_data(const srx_conv2d_t* d, const float* dy, const float* wpk_bwd, float* dx,
                                   int accumulate, float* ws, size_t ws_floats, void* stream) {
  return conv_bwd_data_impl(d, dy, wpk_bwd, dx, accumulate, nullptr, 1.f, 0, 0, ws, ws_floats, stream);
}

extern "C" int srx_conv2d_bwd_data_add(const srx_conv2d_t* d, const float* dy, const float* wpk_bwd, const float* addend,
                                       float* dx, float* ws, size_t ws_floats, void* stream) {
  SRX_REQUIRE(addend && addend != dx, "conv2d_bwd_data_add: the addend must be a tensor of its own");
  return conv_bwd_data_impl(d, dy, wpk_bwd, dx, 0, nullptr, 1.f, 0, 0, ws, ws_floats, stream, addend);
}

extern "C" int srx_conv2d_bwd_data_act(const srx_conv2d_t* d, const float* dy, const float* wpk_bwd, const float* x,
                                       float slope, int c_lo, int c_hi, int accumulate, float* dx, float* ws,
                                       size_t ws_floats, void* stream) {
  SRX_REQUIRE(x, "conv2d_bwd_data_act: null activation tensor");
  return conv_bwd_data_impl(d, dy, wpk_bwd, dx, accumulate, x, slope, c_lo, c_hi, ws, ws_floats, stream);
}

// Rows of the BatchNorm-backward partial table srx_conv2d_bwd_data_bn writes for this layer; 0: the layer does not run on the
// kernel that has that epilogue (the 36-pixel row tile) and the caller keeps the separate srx_bn_act_bwd
extern "C" int srx_conv2d_bwd_data_bn_rows(const srx_conv2d_t* d) {
  if (check_desc(d) != SRX_OK || !srx_rt36_applicable(d) || d->Cin != 64) return 0;
  return srx_rt36_rows(d);
}

extern "C" int srx_conv2d_bwd_data_bn(const srx_conv2d_t* d, const float* dy, const float* wpk_bwd, const float* addend, float* dx,
                                      const float* bn_y, const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                                      const float* bn_beta, const float* bn_prelu, float* table, void* stream) {
  if (int rc = check_desc(d)) return rc;
  SRX_REQUIRE(d->precision != 3, "conv2d: precision 3 (fp16 products) is forward-only");
  SRX_REQUIRE(dy && wpk_bwd && dx && bn_y && bn_mean && bn_invstd && bn_gamma && bn_beta && table, "conv2d_bwd_data_bn: null pointer");
  SRX_REQUIRE(!addend || addend != dx, "conv2d_bwd_data_bn: the addend must be a tensor of its own");
  if (srx_conv2d_bwd_data_bn_rows(d) == 0)
    SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_bwd_data_bn: 3x3 / 64 -> 64 / stride 1 layers on the 36-pixel row tile only (srx_conv2d_bwd_data_bn_rows)");
  BwdClass cls[16];
  size_t total;
  (void)bwd_classes(d, cls, total);
  const srx_rt36_bn_t bn{bn_y, bn_mean, bn_invstd, bn_gamma, bn_beta, bn_prelu, table};
  return srx_rt36_run(d, dy, wpk_bwd + cls[0].woff, nullptr, addend, dx, nullptr, SRX_ACT_NONE, 0.f, srx_stream(stream), &bn);
}

// srx_conv2d_bwd_data_bn whose INPUT is not yet the conv's output gradient but the gradient arriving at the output of the
// BatchNorm (+ PReLU) layer ABOVE the conv (srgan/residual.py:89-90 / :87-88 read backwards): the second pass of that layer's
// backward (sums finalised: srx_bn_act_bwd_finish with dy = NULL) runs while the patch is staged, dy_out receives the conv's
// output gradient for its weight gradient.  table == NULL: no BatchNorm below (plain data gradient + addend).
extern "C" int srx_conv2d_bwd_data_bn_in_ok(const srx_conv2d_t* d) {
  return (!srx_dev().no_bn_bwd_fuse && srx_conv2d_bwd_data_bn_rows(d) != 0) ? 1 : 0;
}

extern "C" int srx_conv2d_bwd_data_bn_in(const srx_conv2d_t* d, const float* dout, const float* in_y, const float* in_mean,
                                         const float* in_invstd, const float* in_gamma, const float* in_beta, const float* in_prelu,
                                         const float* in_sums, float* dy_out, const float* wpk_bwd, const float* addend, float* dx,
                                         const float* bn_y, const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                                         const float* bn_beta, const float* bn_prelu, float* table, void* stream) {
  if (int rc = check_desc(d)) return rc;
  SRX_REQUIRE(d->precision != 3, "conv2d: precision 3 (fp16 products) is forward-only");
  SRX_REQUIRE(dout && in_y && in_mean && in_invstd && in_gamma && in_beta && in_sums && dy_out && wpk_bwd && dx,
              "conv2d_bwd_data_bn_in: null pointer");
  SRX_REQUIRE(dy_out != dout && dy_out != dx && dx != dout && (!addend || addend != dx), "conv2d_bwd_data_bn_in: dout, dy_out, dx and the addend must be tensors of their own");
  SRX_REQUIRE(!table || (bn_y && bn_mean && bn_invstd && bn_gamma && bn_beta), "conv2d_bwd_data_bn_in: a table needs the BatchNorm below");
  if (!srx_conv2d_bwd_data_bn_in_ok(d))
    SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_bwd_data_bn_in: 3x3 / 64 -> 64 / stride 1 layers on the 36-pixel row tile only (srx_conv2d_bwd_data_bn_in_ok)");
  BwdClass cls[16];
  size_t total;
  (void)bwd_classes(d, cls, total);
  const srx_rt36_bn_t bn{bn_y, bn_mean, bn_invstd, bn_gamma, bn_beta, bn_prelu, table};
  const srx_rt36_bnb_t bnb{in_y, in_mean, in_invstd, in_gamma, in_beta, in_prelu, in_sums,
                           1.0f / (float)((int64_t)d->N * d->H * d->W), dy_out};
  return srx_rt36_run(d, dout, wpk_bwd + cls[0].woff, nullptr, addend, dx, nullptr, SRX_ACT_NONE, 0.f, srx_stream(stream),
                      table ? &bn : nullptr, nullptr, &bnb);
}

// The forward of a conv whose INPUT is act(BatchNorm(y_in)) [+ residual] of the conv below (training mode, statistics finalised): the
// normalise + activate pass runs while the input patch is staged, and act_out receives the tensor that pass would have
// written.  1: this layer can (the 36-pixel row tile: 3x3, 64 -> 64, stride 1, few pixels); 0: keep srx_bn_act_fwd + srx_conv2d_fwd.
extern "C" int srx_conv2d_fwd_bn_in_ok(const srx_conv2d_t* d) {
  return (!srx_dev().no_bn_fwd_fuse && check_desc(d) == SRX_OK && srx_rt36_applicable(d)) ? 1 : 0;
}

extern "C" int srx_conv2d_fwd_bn_in(const srx_conv2d_t* d, const float* y_in, const float* bn_mean, const float* bn_invstd,
                                    const float* bn_gamma, const float* bn_beta, const float* bn_prelu, const float* bn_residual,
                                    float* act_out, const float* wpk, const float* bias, float* y, float* bn_partials, void* stream) {
  if (int rc = check_desc(d)) return rc;
  SRX_REQUIRE(y_in && bn_mean && bn_invstd && bn_gamma && bn_beta && act_out && wpk && y, "conv2d_fwd_bn_in: null pointer");
  SRX_REQUIRE(act_out != y_in && act_out != y && y != y_in && act_out != bn_residual && y != bn_residual,
              "conv2d_fwd_bn_in: y_in, act_out, y and the residual must be tensors of their own");
  if (!srx_conv2d_fwd_bn_in_ok(d))
    SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_fwd_bn_in: 3x3 / 64 -> 64 / stride 1 layers on the 36-pixel row tile only (srx_conv2d_fwd_bn_in_ok)");
  const srx_rt36_bnl_t bnl{bn_mean, bn_invstd, bn_gamma, bn_beta, bn_prelu, bn_residual, act_out};
  return srx_rt36_run(d, y_in, wpk, bias, nullptr, y, bn_partials, d->act, d->slope, srx_stream(stream), nullptr, &bnl);
}

extern "C" int srx_conv2d_bwd_data_ex(const srx_conv2d_t* d, const float* dy, const float* wpk_bwd, float* dx,
                                      const srx_dgrad_epilogue_t* e, float* ws, size_t ws_floats, void* stream) {
  SRX_REQUIRE(e, "conv2d_bwd_data_ex: null epilogue");
  SRX_REQUIRE(!e->addend || e->addend != dx, "conv2d_bwd_data_ex: the addend must be a tensor of its own (use accumulate)");
  return conv_bwd_data_impl(d, dy, wpk_bwd, dx, e->accumulate, e->act_out, e->act_slope, e->c_lo, e->c_hi, ws, ws_floats,
                            stream, e->addend, e->addend_ld, e->addend_channels, e->addend_scale == 0.f ? 1.f : e->addend_scale,
                            e->out_scale == 0.f ? 1.f : e->out_scale);
}

// ------------------------------------------------------------------------------------------------------------------
// bf16 STORAGE of activations on the training path (round 5; round-4 review, item 2): 3x3 / stride 1 / pad 1 layers whose
// input AND output tensors are bf16 NHWC.  The arithmetic is the bf16-product recipe of precision = 1 to the letter -- every
// operand of such a layer was rounded to bf16 when it was staged; here the PRODUCER rounds it once instead of every consumer
// -- so the oracle and its tolerances do not change; what changes is the traffic (half the bytes, no fp32 -> bf16 conversion
// in the loader: 18.8 VALU instructions per MFMA on the 64-column layers, profiles/r04_pmc_esrgan.txt).  The kernel is
// gconv_kernel<..., PR = 2>: the bf16 tensors are described as fp32 tensors of HALF the channel count, so a 128-byte k-chunk
// is 64 channels of one tap and every gather offset is the fp32 code's; a 16-byte quad is one v_mfma_f32_32x32x16_bf16 operand.
// Used by the frozen VGG19 stack of the perceptual loss under autocast (esrgan/trainer.py:461-467, srgan/loss.py:52-53).
// ------------------------------------------------------------------------------------------------------------------
namespace {

bool bf16s_shape_ok(const srx_conv2d_t* d) {
  return d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad == 1 && !d->shuffle && d->up != 2 && d->precision == 1 &&
         d->Cin % 64 == 0 && d->Cout % 64 == 0 && d->Cin_s == d->Cin && d->Cout_s == d->Cout &&
         (int64_t)d->N * d->H * d->W < (1 << 24) && (int64_t)d->N * d->H * d->W * std::max(d->Cin, d->Cout) < (1LL << 30);
}

// wf[co][(kh, kw, ci)] = bf16(w[co][ci][kh][kw]);  wb[ci][(kh, kw, co)] = bf16(w[co][ci][2 - kh][2 - kw])
__global__ void bf16s_pack_kernel(const float* __restrict__ w, __bf16* __restrict__ wf, __bf16* __restrict__ wb, int Cout, int Cin) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)Cout * Cin * 9) return;
  const int ci = (int)(idx % Cin);
  const int t = (int)((idx / Cin) % 9);
  const int co = (int)(idx / ((int64_t)Cin * 9));
  const __bf16 v = (__bf16)w[((size_t)co * Cin + ci) * 9 + t];
  wf[idx] = v;  // ((co * 9 + t) * Cin + ci)
  if (wb) wb[((size_t)ci * 9 + (8 - t)) * Cout + co] = v;
}

Plan bf16s_plan(const srx_conv2d_t* d, int which) {
  const int cc = which ? d->Cout : d->Cin, cn = which ? d->Cin : d->Cout;
  return make_plan(d->N * d->H * d->W, cn, 9 * cc / 64, true, true, false);
}

int bf16s_run(const srx_conv2d_t* d, int which, const void* in16, const void* wpk16, const float* bias, int relu,
              const void* mask16, void* out, int out_is_bf16, float* ws, size_t ws_floats, void* stream) {
  if (int rc = check_desc(d)) return rc;
  SRX_REQUIRE(in16 && wpk16 && out && in16 != out, "conv3x3_bf16s: null pointer / in place");
  if (!bf16s_shape_ok(d))
    SRX_FAIL(SRX_E_UNSUPPORTED, "conv3x3_bf16s: 3x3 / stride 1 / pad 1 layers with precision = 1 and channel counts that are multiples of 64 only");
  const int cc = which ? d->Cout : d->Cin, cn = which ? d->Cin : d->Cout;
  GArgs a{};
  a.in = static_cast<const float*>(in16); a.w = static_cast<const float*>(wpk16); a.bias = bias;
  set_mgrid(a, d->N, d->H, d->W);
  a.Hi = d->H; a.Wi = d->W; a.Ci = cc / 2;  // (floats = pairs of bf16 channels)
  a.in_stride = 1; a.nth = 3; a.ntw = 3; a.dh0 = -1; a.dw0 = -1;
  a.Ck = cc / 2; a.K = 9 * cc / 2; a.Kp = a.K;
  a.Cn = cn; a.Cs = cn; a.Ho = d->H; a.Wo = d->W; a.Co = cn;
  a.out_stride = 1; a.linear_out = 1;
  a.act = relu ? SRX_ACT_RELU : SRX_ACT_NONE;
  a.slope = relu ? 0.f : 1.f;
  a.out = static_cast<float*>(out);
  a.out16 = out_is_bf16 ? 1 : 0;
  a.oscale = 1.f; a.add_ld = cn; a.add_hi = 0x7fffffff; a.ascale = 1.f;
  if (mask16) { a.mask = static_cast<const float*>(mask16); a.mask16 = 1; a.mask_slope = 0.f; a.mask_lo = 0; a.mask_hi = cn; }
  a.in_bytes = (size_t)d->N * d->H * d->W * cc * 2;
  a.w_bytes = (unsigned)((size_t)cn * 9 * cc * 2);
  a.in_margin = 4u * (unsigned)((a.Wi + 1) * a.Ci);
  return run_gconv(a, bf16s_plan(d, which), ws, ws_floats, srx_stream(stream), 2);
}

}  // namespace

extern "C" int srx_conv3x3_bf16s_applicable(const srx_conv2d_t* d) { return d && check_desc(d) == SRX_OK && bf16s_shape_ok(d) ? 1 : 0; }

// bytes of ONE packed copy (forward or data gradient): Cout x 9 x Cin bf16 values
extern "C" size_t srx_conv3x3_bf16s_packed_bytes(const srx_conv2d_t* d) {
  return (d && bf16s_shape_ok(d)) ? (size_t)d->Cout * 9 * d->Cin * 2 : 0;
}

extern "C" int srx_conv3x3_bf16s_pack(const srx_conv2d_t* d, const float* w, void* wpk_fwd, void* wpk_bwd, void* stream) {
  if (int rc = check_desc(d)) return rc;
  SRX_REQUIRE(w && wpk_fwd, "conv3x3_bf16s_pack: null pointer");
  if (!bf16s_shape_ok(d)) SRX_FAIL(SRX_E_UNSUPPORTED, "conv3x3_bf16s_pack: not a bf16-storage layer");
  const int64_t n = (int64_t)d->Cout * d->Cin * 9;
  hipLaunchKernelGGL(bf16s_pack_kernel, dim3((unsigned)srx_cdiv(n, 256)), dim3(256), 0, srx_stream(stream), w,
                     static_cast<__bf16*>(wpk_fwd), static_cast<__bf16*>(wpk_bwd), d->Cout, d->Cin);
  SRX_CHECK_LAUNCH("bf16s_pack_kernel");
  return SRX_OK;
}

// workspace (floats) of the forward (which = 0) / data gradient (which = 1): K-split partial tiles of the last round
extern "C" size_t srx_conv3x3_bf16s_ws_floats(const srx_conv2d_t* d, int which) {
  if (!d || check_desc(d) != SRX_OK || !bf16s_shape_ok(d)) return 0;
  return plan_ws_floats(bf16s_plan(d, which));
}

// the 3 -> 64 first layer in front of such a stack (srx_conv2d_fwd's first3x3 kernel, precision = 1) writing a bf16 tensor:
// x fp32 [N][H][W][4], wpk: the layer's ordinary forward pack, y bf16 [N][H][W][64]
extern "C" int srx_conv2d_fwd_first3_to_bf16(const srx_conv2d_t* d, const float* x, const float* wpk_fwd, const float* bias, void* y,
                                             void* stream) {
  if (int rc = check_desc(d)) return rc;
  SRX_REQUIRE(x && wpk_fwd && y, "conv2d_fwd_first3_to_bf16: null pointer");
  if (!srx_first3_fwd_applicable(d) || d->precision != 1 || d->act == SRX_ACT_PRELU)
    SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_fwd_first3_to_bf16: 3x3 / stride 1 / pad 1 layers from <= 4 to 64 channels with precision = 1 only");
  return srx_first3_fwd(d, x, wpk_fwd, fwd_geo(d).Kp, bias, static_cast<float*>(y), srx_stream(stream), 1);
}

// y = [relu](conv(x) + bias): x bf16 [N][H][W][Cin]; y bf16 or fp32 [N][H][W][Cout]
extern "C" int srx_conv3x3_bf16s_fwd(const srx_conv2d_t* d, const void* x, const void* wpk_fwd, const float* bias, int relu,
                                     void* y, int y_is_bf16, float* ws, size_t ws_floats, void* stream) {
  return bf16s_run(d, 0, x, wpk_fwd, bias, relu, nullptr, y, y_is_bf16, ws, ws_floats, stream);
}

// dx = conv^T(dy) [* (relu_out > 0)]: dy bf16 [N][H][W][Cout]; relu_out: the bf16 OUTPUT of the ReLU that produced this layer's
// input (null: none) -- that activation's backward on the way out; dx bf16 or fp32 [N][H][W][Cin]
extern "C" int srx_conv3x3_bf16s_bwd_data(const srx_conv2d_t* d, const void* dy, const void* wpk_bwd, const void* relu_out,
                                          void* dx, int dx_is_bf16, float* ws, size_t ws_floats, void* stream) {
  return bf16s_run(d, 1, dy, wpk_bwd, nullptr, 0, relu_out, dx, dx_is_bf16, ws, ws_floats, stream);
}
