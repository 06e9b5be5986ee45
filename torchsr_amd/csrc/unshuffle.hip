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
