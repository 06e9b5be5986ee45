// RRDBNet's x2 input layer: pixel_unshuffle(x, 2) followed by the 3x3 / pad 1 conv over its 12 channels, image -> 64 channels,
// bias, no activation (Real-ESRGAN's conv_first behind RealESRGANer.pre_process's reflect pad of an odd axis).  The two are ONE
// 6x6 / stride 2 / pad 2 conv over the 3-channel image,
//   v[o][c][2 ky + dy][2 kx + dx] = w[o][4 c + 2 dy + dx][ky][kx],
// so neither the unshuffled nor the padded tensor is ever written: output pixel (Y, X) reads image rows r = 2 Y - 2 + ty,
// ty = 0..5 (columns alike).  r < 0 or r >= Hp = H + (H & 1) is the conv's zero padding in the unshuffled domain; r == H (H odd
// only) is the reflected pad row and reads row H - 2.
// The kernel is first3x3_fwd_kernel (thin.hip) with 36 taps: a wave owns 32 output pixels x 64 columns (two 32x32x2 fp32
// accumulators), each lane reads its pixel's 36 16-byte neighbours straight into registers (lane = pixel; both lane halves load
// the same quad and pick their k parity's channel) and the result leaves as a write stream of 256 bytes per pixel.  K = 36 taps
// x 3 channels = 108 -- the pack drops the stored zero channel, 54 k-steps instead of 72 -- so a k-step's two elements may sit
// in two taps; which, is known at compile time.  The 108 x 64 weights (27 KB) would fill 108 registers per lane next to 144 of
// pixels, so they stay in LDS ([k][64]: a lane half reads 32 consecutive floats, no bank conflict) and every MFMA fetches its B
// operand from there, one ds_read under a 64-cycle instruction.  The pixels come one tap row at a time (6 quads = 18 k = 9
// k-steps, the next row's loads issued ahead of this row's MFMAs): 109 registers, so four waves share a SIMD and one's loads and
// stores run under the others' MFMAs (all 36 quads at once: 173 registers, two waves, 88 us at 1080p where this form takes
// 76, profiles/rrdbnet_x2_times.txt).  Address arithmetic: six row and six column byte offsets per tile, then one add per
// tap -- an offset outside the image carries 2^30, which the buffer descriptor turns into a zero (in_bytes < 2^28).
// PR: operands rounded to bf16 when staged (the weights on their way into LDS, the pixels on their way into the MFMA), products
// and sums fp32 -- first3x3_fwd_kernel's switch.
#include "srx_common.h"

#include <algorithm>
#include <cstdio>

namespace {

constexpr int U2_K = 108;  // (ty * 6 + tx) * 3 + c

struct Unshuffle2 {
  const float* in; const float* w; const float* bias; float* out;
  int H, W, Hp, Wp, Wo, HoWo, M, ntiles;
  float inv_HoWo, inv_Wo;
  unsigned in_bytes, out_bytes;
};

template <int PR>
__global__ __launch_bounds__(256, 4) void unshuffle2_conv_fwd_kernel(const Unshuffle2 a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i31 = lane & 31, h2 = lane >> 5;
  const __amdgpu_buffer_rsrc_t rin = srx_rsrc(a.in, a.in_bytes);
  const __amdgpu_buffer_rsrc_t rout = srx_rsrc(a.out, a.out_bytes);
  auto rnd = [](float v) { return PR ? (float)(__bf16)v : v; };
  __shared__ float sw[U2_K * 64];
  for (int i = threadIdx.x; i < U2_K * 64; i += 256) sw[i] = rnd(a.w[i]);
  __syncthreads();
  float bv[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) bv[j] = a.bias ? a.bias[32 * j + i31] : 0.f;
  const float* swl = sw + h2 * 64 + i31;  // B[k = 2 s + h2][column 32 j + i31]
  for (int tile = blockIdx.x * 4 + wave; tile < a.ntiles; tile += gridDim.x * 4) {
    const int p = tile * 32 + i31;
    int n, rem, Y, X;
    srx_divmod(min(p, a.M - 1), a.HoWo, a.inv_HoWo, n, rem);
    srx_divmod(rem, a.Wo, a.inv_Wo, Y, X);
    unsigned roff[6], coff[6];
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      int r = 2 * Y - 2 + t, c = 2 * X - 2 + t;
      const bool rok = p < a.M && r >= 0 && r < a.Hp, cok = c >= 0 && c < a.Wp;
      r = r == a.H ? a.H - 2 : r;  // the reflected pad row / column of an odd axis
      c = c == a.W ? a.W - 2 : c;
      roff[t] = rok ? (unsigned)((n * a.H + r) * a.W) * 16u : 0x40000000u;
      coff[t] = cok ? (unsigned)c * 16u : 0x40000000u;
    }
    // one tap row (6 quads, 18 k = 9 k-steps) at a time, the next row's loads issued ahead of this row's MFMAs
    f32x4 v[2][6];
#pragma unroll
    for (int t = 0; t < 6; ++t) v[0][t] = srx_bload(rin, roff[0] + coff[t], 0);
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
#pragma unroll
    for (int ty = 0; ty < 6; ++ty) {
      __builtin_amdgcn_sched_barrier(0);  // (keeps the scheduler from hoisting all 36 loads to the top: 144 registers of pixels)
      if (ty < 5) {
#pragma unroll
        for (int t = 0; t < 6; ++t) v[(ty + 1) & 1][t] = srx_bload(rin, roff[ty + 1] + coff[t], 0);
      }
#pragma unroll
      for (int s = 0; s < 9; ++s) {  // k = 18 ty + 2 s + h2 = 3 (6 ty + tx) + channel
        const float av = rnd(h2 ? v[ty & 1][(2 * s + 1) / 3][(2 * s + 1) % 3] : v[ty & 1][(2 * s) / 3][(2 * s) % 3]);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, swl[(9 * ty + s) * 128], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, swl[(9 * ty + s) * 128 + 32], acc1, 0, 0, 0);
      }
    }
    // 32x32 accumulator: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5); rows past M fall outside the descriptor
    const unsigned obase = ((unsigned)tile * 32u * 64u + (unsigned)i31 + 256u * h2) * 4u;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ro = ((r & 3) + 8 * (r >> 2)) * 256;
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, acc0[r] + bv[0]), rout, (int)obase, ro, 0);
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, acc1[r] + bv[1]), rout, (int)obase, ro + 128, 0);
    }
  }
}

// p[(ty * 6 + tx) * 3 + c][o] = w[o][4 c + 2 (ty & 1) + (tx & 1)][ty >> 1][tx >> 1], w OIHW [64][12][3][3]
__global__ void unshuffle2_pack_kernel(const float* __restrict__ w, float* __restrict__ p) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= U2_K * 64) return;
  const int o = idx & 63, k = idx >> 6, c = k % 3, tap = k / 3, ty = tap / 6, tx = tap % 6;
  p[idx] = w[((o * 12 + 4 * c + 2 * (ty & 1) + (tx & 1)) * 3 + (ty >> 1)) * 3 + (tx >> 1)];
}

// ---- weight gradient (training the x2 net) ----
// dV[o][c][ty][tx] = sum over (n, Y, X) of dy[n][Y][X][o] * x[n][r(2 Y - 2 + ty)][q(2 X - 2 + tx)][c] with the forward's gather r / q
// (zero below 0 and from Hp / Wp on, index H / W -> H - 2 / W - 2), left in the module's layout by the reduce kernel:
//   dw[o][4 c + 2 (ty & 1) + (tx & 1)][ty >> 1][tx >> 1] = dV[o][c][ty][tx].
// This is thin_wgrad_kernel<KH, KW, GROUPS, +1> (thin.hip) at stride 2, for that kernel's reasons: on gfx950 the f32 MFMAs and the
// VALU instructions of one SIMD never overlap, so address arithmetic is counted, not hidden.  A segment is 16 output pixels of
// one output row; the wave holds their 16 dy rows in registers (lane = output channel) and, per tap row, the 36 image values it
// slides over (columns 2 X0 - 2 .. 2 X0 + 33, lane & 3 = image channel), so the 16 x 6 v_mfma_f32_4x4x1f32 of a tap row take
// tv[2 j + tx] with static indices and no LDS.  Every address is wave-uniform up to the lane's channel, so both operands come
// through buffer descriptors cut per row (scalar work, a handful of instructions a row): the pixel is the instruction's constant
// offset, a padding position (a pad row, a column past the row, an output column past Wo) falls outside the descriptor and reads
// 0, the reflected row is a scalar select and the reflected column a scalar offset.  The six tap rows are split over GROUPS = 2
// workgroups (3 rows = 18 f32x4 accumulators a wave); the four waves of a workgroup take four consecutive segment ranges and fold
// through LDS into one slab [4][36][64], of which this group writes its 18 taps.
// Compiler's resource usage for gfx950 (-Rpass-analysis=kernel-resource-usage): 84 VGPRs + 72 AGPRs (the accumulators) = 156
// registers, 93 SGPRs, no scratch, no spill, three waves per SIMD; the segment loop holds 288 MFMAs, 124 loads and no other vector
// instruction.  (GROUPS = 1 would be 144 accumulator registers next to the same operands: one wave per SIMD less.)
// Exact fp32 at either precision: the 3-channel layers' weight gradients are fp32 in both phases of training.
constexpr int U2W_GROUPS = 2;
constexpr int U2W_MIN_SEGS = 4;  // a wave's share of the 36 KB slab is what ~4 segments read (16 x 256 B of dy, 3 x 36 x 16 B of image)

struct Unshuffle2W {
  const float* x; const float* dy; float* slab;
  int H, W, Hp, Wp, Ho, Wo, wsegs, nseg, segs_per_range;
  unsigned x_bytes, dy_bytes;
};

__global__ __launch_bounds__(256) void unshuffle2_conv_wgrad_kernel(const Unshuffle2W a) {
  constexpr int RPG = 6 / U2W_GROUPS;
  __shared__ float fold[2][RPG * 6 * 4 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int group = blockIdx.x % U2W_GROUPS, rb = blockIdx.x / U2W_GROUPS;
  const int range = rb * 4 + wave;
  const int sbeg = min(a.nseg, range * a.segs_per_range);  // ranges past the end are empty
  const int send = min(a.nseg, sbeg + a.segs_per_range);

  f32x4 acc[RPG * 6];
#pragma unroll
  for (int t = 0; t < RPG * 6; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const unsigned wlane = 4u * (unsigned)lane, tlane = 4u * (unsigned)(lane & 3);
  const int s0 = srx_uniform(sbeg), s1 = srx_uniform(send);
  for (int s = s0; s < s1; ++s) {
    const int cb = s % a.wsegs;
    const int Y = (s / a.wsegs) % a.Ho;
    const int n = s / (a.wsegs * a.Ho);
    const int X0 = cb * 16, cbase = 2 * X0 - 2;
    // dy: a descriptor over the rest of this output row, so pixel j is the instruction's immediate offset and a column past Wo reads 0
    const __amdgpu_buffer_rsrc_t rdy = srx_rsrc(a.dy + (size_t)((n * a.Ho + Y) * a.Wo + X0) * 64, (unsigned)(a.Wo - X0) * 256u);
    float wv[16];
#pragma unroll
    for (int j = 0; j < 16; ++j)
      wv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rdy, (int)(wlane + 256u * j), 0, 0));
    // image: a descriptor per row that starts 32 bytes before column cbase and ends with the row, so column cbase + t is the
    // immediate offset 16 t behind a scalar offset of 32, a column from W on reads 0, the reflected column W (W odd) is column
    // cbase + t - 2: scalar offset 0, and the two columns left of the image (X0 = 0) carry 2^30.  A pad row is an empty descriptor.
    const int tstar = (a.W & 1) ? a.W - cbase : -1;
    unsigned so[36];
#pragma unroll
    for (int t = 0; t < 36; ++t) so[t] = (t < 2 && cbase < 0) ? 0x40000000u : (t == tstar ? 0u : 32u);
#pragma unroll
    for (int dr = 0; dr < RPG; ++dr) {
      __builtin_amdgcn_sched_barrier(0);  // (one tap row's 36 values at a time)
      int r = 2 * Y - 2 + group * RPG + dr;
      const bool rok = r >= 0 && r < a.Hp;
      r = r == a.H ? a.H - 2 : r;  // the reflected pad row of an odd H
      const char* xrow = (const char*)a.x + ((int64_t)((n * a.H + (rok ? r : 0)) * a.W + cbase) * 16 - 32);
      const __amdgpu_buffer_rsrc_t rx = srx_rsrc(xrow, rok ? (unsigned)(a.W - cbase) * 16u + 32u : 0u);
      float tv[36];
#pragma unroll
      for (int t = 0; t < 36; ++t)
        tv[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, (int)(tlane + 16u * t), (int)so[t], 0));
#pragma unroll
      for (int j = 0; j < 16; ++j)
#pragma unroll
        for (int tx = 0; tx < 6; ++tx)
          acc[dr * 6 + tx] = __builtin_amdgcn_mfma_f32_4x4x1f32(tv[2 * j + tx], wv[j], acc[dr * 6 + tx], 0, 0, 0);
    }
  }
  // fold: waves 2,3 -> LDS, waves 0,1 add; wave 1 -> LDS, wave 0 adds and writes the slab
  auto put = [&](int slot) {
#pragma unroll
    for (int t = 0; t < RPG * 6; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) fold[slot][(t * 4 + c) * 64 + lane] = acc[t][c];
  };
  auto add = [&](int slot) {
#pragma unroll
    for (int t = 0; t < RPG * 6; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[t][c] += fold[slot][(t * 4 + c) * 64 + lane];
  };
  if (wave >= 2) put(wave - 2);
  __syncthreads();
  if (wave < 2) add(wave);
  __syncthreads();
  if (wave == 1) put(0);
  __syncthreads();
  if (wave != 0) return;
  add(0);
  float* o = a.slab + (size_t)rb * (4 * 36 * 64);
#pragma unroll
  for (int t = 0; t < RPG * 6; ++t)
#pragma unroll
    for (int c = 0; c < 3; ++c) o[((size_t)c * 36 + group * (RPG * 6) + t) * 64 + lane] = acc[t][c];
}

// slab sums -> OIHW [64][12][3][3] with the permutation above.  One workgroup per (c, tap): 64 channels x 4 slab lanes, LDS fold.
__global__ __launch_bounds__(256) void unshuffle2_conv_wgrad_reduce_kernel(const float* __restrict__ slab, int nslabs,
                                                                           float* __restrict__ dw, int accumulate) {
  __shared__ float red[4][64];
  const int o = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int tap = blockIdx.x % 36, c = blockIdx.x / 36, ty = tap / 6, tx = tap % 6;
  const float* p = slab + ((size_t)c * 36 + tap) * 64 + o;
  float s = 0.f;
  for (int r = part; r < nslabs; r += 4) s += p[(size_t)r * (4 * 36 * 64)];
  red[part][o] = s;
  __syncthreads();
  if (part == 0) {
    const float v = (red[0][o] + red[1][o]) + (red[2][o] + red[3][o]);
    float* q = dw + ((o * 12 + 4 * c + 2 * (ty & 1) + (tx & 1)) * 3 + (ty >> 1)) * 3 + (tx >> 1);
    *q = accumulate ? *q + v : v;
  }
}

// tiles of 32 output pixels, a wave walks tile = 4 workgroup + wave, += 4 workgroups.  The ONE place that cuts the plan.
struct Unshuffle2Plan { int Hp, Wp, M, ntiles, workgroups; };
int unshuffle2_plan(int N, int H, int W, Unshuffle2Plan& p) {
  SRX_REQUIRE(N > 0 && H > 0 && W > 0, "unshuffle2_conv: N, H and W must be positive (got %d, %d, %d)", N, H, W);
  SRX_REQUIRE(!(H & 1) || H >= 3, "unshuffle2_conv: an odd H is padded by a reflected row and must be at least 3 (got %d)", H);
  SRX_REQUIRE(!(W & 1) || W >= 3, "unshuffle2_conv: an odd W is padded by a reflected column and must be at least 3 (got %d)", W);
  p.Hp = H + (H & 1); p.Wp = W + (W & 1);
  // (srx_divmod's range, and 16-byte pixels behind 32-bit buffer offsets with room for the 2^30 marks)
  SRX_REQUIRE((int64_t)N * p.Hp * p.Wp < (1 << 24), "unshuffle2_conv: N * Hp * Wp = %lld passes the 2^24 pixels of one call",
              (long long)N * p.Hp * p.Wp);
  p.M = N * (p.Hp / 2) * (p.Wp / 2);
  p.ntiles = (int)srx_cdiv(p.M, 32);
  // four workgroups per CU (<= 128 registers: four waves per SIMD; 4 x 27 KB of LDS), each wave walking its share of the tiles
  p.workgroups = (int)std::min<int64_t>(srx_cdiv(p.ntiles, 4), (int64_t)srx_plan_cus() * 4);
  return SRX_OK;
}

// weight gradient: segments = (image, output row, 16-column block); a wave takes `segs_per_range` consecutive ones, the four waves
// of a workgroup four consecutive ranges (one slab per workgroup; U2W_GROUPS workgroups, one per group of tap rows, share it);
// ranges past `nranges` are empty.  The ONE place that cuts this plan.
struct Unshuffle2WPlan { int Hp, Wp, Ho, Wo, wsegs, nseg, segs_per_range, nranges, nslabs; };
int unshuffle2_wgrad_plan(int N, int H, int W, Unshuffle2WPlan& p) {
  Unshuffle2Plan f;
  if (int rc = unshuffle2_plan(N, H, W, f)) return rc;
  p.Hp = f.Hp; p.Wp = f.Wp; p.Ho = f.Hp / 2; p.Wo = f.Wp / 2;
  p.wsegs = (int)srx_cdiv(p.Wo, 16);
  p.nseg = N * p.Ho * p.wsegs;
  // about two waves per SIMD (one's loads hide under the other's MFMAs), and no fewer than U2W_MIN_SEGS segments behind a slab share
  int ranges = (int)std::min<int64_t>((srx_plan_cus() * 8) / U2W_GROUPS, srx_cdiv(p.nseg, U2W_MIN_SEGS));
  if (ranges < 1) ranges = 1;
  p.segs_per_range = (int)srx_cdiv(p.nseg, ranges);
  p.nranges = (int)srx_cdiv(p.nseg, p.segs_per_range);
  p.nslabs = (int)srx_cdiv(p.nranges, 4);
  return SRX_OK;
}

}  // namespace

extern "C" size_t srx_unshuffle2_conv_packed_floats(void) { return (size_t)U2_K * 64; }

extern "C" int srx_unshuffle2_conv_pack(const float* w_oihw, float* wpk, void* stream) {
  SRX_REQUIRE(w_oihw && wpk, "unshuffle2_conv_pack: null pointer (w %p, wpk %p)", (const void*)w_oihw, (void*)wpk);
  hipLaunchKernelGGL(unshuffle2_pack_kernel, dim3((unsigned)srx_cdiv(U2_K * 64, 256)), dim3(256), 0, srx_stream(stream), w_oihw, wpk);
  SRX_CHECK_LAUNCH("unshuffle2_pack_kernel");
  return SRX_OK;
}

extern "C" int srx_unshuffle2_conv_plan(int N, int H, int W, int* out) {
  SRX_REQUIRE(out, "unshuffle2_conv_plan: a result array");
  Unshuffle2Plan p;
  if (int rc = unshuffle2_plan(N, H, W, p)) return rc;
  out[0] = p.ntiles; out[1] = p.workgroups;
  return SRX_OK;
}

extern "C" int srx_unshuffle2_conv_fwd(int N, int H, int W, const float* x, const float* wpk, const float* bias, float* y,
                                       int precision, void* stream) {
  SRX_REQUIRE(x && wpk && y, "unshuffle2_conv_fwd: null pointer (x %p, wpk %p, y %p)", (const void*)x, (const void*)wpk, (void*)y);
  SRX_REQUIRE(precision == 0 || precision == 1, "unshuffle2_conv_fwd: precision %d (0: fp32, 1: bf16 operands)", precision);
  Unshuffle2Plan p;
  if (int rc = unshuffle2_plan(N, H, W, p)) return rc;
  Unshuffle2 a;
  a.in = x; a.w = wpk; a.bias = bias; a.out = y;
  a.H = H; a.W = W; a.Hp = p.Hp; a.Wp = p.Wp; a.Wo = p.Wp / 2; a.HoWo = (p.Hp / 2) * a.Wo; a.M = p.M; a.ntiles = p.ntiles;
  a.inv_HoWo = 1.0f / (float)a.HoWo; a.inv_Wo = 1.0f / (float)a.Wo;
  a.in_bytes = (unsigned)((size_t)N * H * W * 4 * sizeof(float));
  a.out_bytes = (unsigned)((size_t)a.M * 64 * sizeof(float));
  hipStream_t st = srx_stream(stream);
  const unsigned grid = (unsigned)p.workgroups;
  char nm[64];
  if (srx_prof_on()) snprintf(nm, sizeof(nm), "unshuffle2_conv_fwd_kernel<%d> MxNxK=%dx64x%d", precision, a.M, U2_K);
  if (precision) SRX_LAUNCH_PROF(nm, 2.0 * a.M * 64 * U2_K, unshuffle2_conv_fwd_kernel<1>, dim3(grid), dim3(256), 0, st, a);
  else SRX_LAUNCH_PROF(nm, 2.0 * a.M * 64 * U2_K, unshuffle2_conv_fwd_kernel<0>, dim3(grid), dim3(256), 0, st, a);
  SRX_CHECK_LAUNCH("unshuffle2_conv_fwd_kernel");
  return SRX_OK;
}

extern "C" size_t srx_unshuffle2_conv_wgrad_ws_floats(int N, int H, int W) {
  Unshuffle2WPlan p;
  if (unshuffle2_wgrad_plan(N, H, W, p)) return 0;
  return (size_t)p.nslabs * 4 * 36 * 64;
}

extern "C" int srx_unshuffle2_conv_wgrad_plan(int N, int H, int W, int* out) {
  SRX_REQUIRE(out, "unshuffle2_conv_wgrad_plan: a result array");
  Unshuffle2WPlan p;
  if (int rc = unshuffle2_wgrad_plan(N, H, W, p)) return rc;
  out[0] = p.nseg; out[1] = p.nranges; out[2] = p.segs_per_range; out[3] = p.nslabs; out[4] = U2W_GROUPS;
  return SRX_OK;
}

extern "C" int srx_unshuffle2_conv_bwd_weight(int N, int H, int W, const float* x, const float* dy, float* dw_oihw, int accumulate,
                                              float* ws, size_t ws_floats, void* stream) {
  SRX_REQUIRE(x && dy && dw_oihw && ws, "unshuffle2_conv_bwd_weight: null pointer (x %p, dy %p, dw %p, ws %p)", (const void*)x,
              (const void*)dy, (void*)dw_oihw, (void*)ws);
  Unshuffle2WPlan p;
  if (int rc = unshuffle2_wgrad_plan(N, H, W, p)) return rc;
  if ((size_t)p.nslabs * 4 * 36 * 64 > ws_floats)
    SRX_FAIL(SRX_E_WORKSPACE, "unshuffle2_conv_bwd_weight: workspace of %zu floats, %zu needed", ws_floats, (size_t)p.nslabs * 4 * 36 * 64);
  Unshuffle2W a;
  a.x = x; a.dy = dy; a.slab = ws;
  a.H = H; a.W = W; a.Hp = p.Hp; a.Wp = p.Wp; a.Ho = p.Ho; a.Wo = p.Wo;
  a.wsegs = p.wsegs; a.nseg = p.nseg; a.segs_per_range = p.segs_per_range;
  a.x_bytes = (unsigned)((size_t)N * H * W * 4 * sizeof(float));  // (N Hp Wp < 2^24: below 2^28 and 2^30 bytes)
  a.dy_bytes = (unsigned)((size_t)N * p.Ho * p.Wo * 64 * sizeof(float));
  hipStream_t st = srx_stream(stream);
  SRX_LAUNCH_PROF("unshuffle2_conv_wgrad_kernel", 2.0 * N * p.Ho * p.Wo * 64 * U2_K, unshuffle2_conv_wgrad_kernel,
                  dim3((unsigned)(p.nslabs * U2W_GROUPS)), dim3(256), 0, st, a);
  SRX_CHECK_LAUNCH("unshuffle2_conv_wgrad_kernel");
  hipLaunchKernelGGL(unshuffle2_conv_wgrad_reduce_kernel, dim3(3 * 36), dim3(256), 0, st, ws, p.nslabs, dw_oihw, accumulate);
  SRX_CHECK_LAUNCH("unshuffle2_conv_wgrad_reduce_kernel");
  return SRX_OK;
}
