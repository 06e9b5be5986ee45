// Separable resize of fp32 planes with the weight tables as operands (functional.resample_tables: the antialiased Keys
// bicubic of the training data, for any mix of reduction and enlargement per axis) -- the `outscale` of test.upscale:
//   tmp[p][oy][x]  = sum_t wy[oy][t] * src[p][min(sy[oy] + t, H - 1)][x]      t = 0 .. Ky - 1   (rows pass)
//   dst[p][oy][ox] = sum_t wx[ox][t] * tmp[p][oy][min(sx[ox] + t, W - 1)]     t = 0 .. Kx - 1   (columns pass)
// Two launches through the workspace tmp [planes][OH][W]; the order is fixed (rows first), so the summation order is too.
// Every start is clamped to [0, n_in - 1] and every tap to n_in - 1: no table content reads outside src / tmp, and the
// padded taps of a row (weight 0) add 0.  No polynomial, division or normalisation on the device: each output is two
// dot products, fmas in ascending t from 0 -- no atomics, no dependence on the other planes of the call, the scalar and
// the 16-byte form of the rows pass in the same order: the same bits from every call and every alignment.
//  - rows pass: lanes along x, each tap one row-contiguous load -- 16 bytes per lane when W % 4 == 0 and src and tmp are
//    16-byte aligned (then every row is), 4 otherwise -- and its weight a wave-uniform (scalar) load.  A work item is RV = 8
//    consecutive output rows of a 256-lane column chunk, walked in order: at 2:1 the 64 row reads of an item touch 22 source
//    rows, the repeats served by the CU's own L1 / its XCD's L2 instead of by four workgroups on four XCDs.
//  - columns pass: lanes along ox, RH = 4 rows per lane behind one load of start and of each weight.  Lane l reads
//    tmp[sx[ox0 + l] + t]: at a reduction r consecutive lanes are r floats apart, a wave's load spans 64 r floats of one row
//    and the Kx = 4 r taps of the loop use every byte of those lines out of L1; an enlargement reads each float from several
//    lanes (a broadcast).  At 16:1 that is one 64-byte line per 1 lane per tap, the worst case: still row-wise, never wrong.
//    Stores are one dword per lane, 256 contiguous bytes per wave.  No LDS: the staging a tile would need (256 outputs x 16
//    + 66 floats per row at 16:1) buys back only the L1 hits.
// Work items are a linear index walked with a grid-stride loop, every plane / row base 64-bit (a batch of 8K frames passes
// 2^31 elements; one plane must stay below it).
// gfx950, -O3 (-Rpass-analysis=kernel-resource-usage): resample_rows_kernel<f32x4> 30 VGPRs, <float> 18; resample_cols_kernel
// 30 VGPRs; no AGPRs, no scratch, no LDS, occupancy 8 waves / SIMD each.
#include "srx_common.h"

namespace {

constexpr int RV = 8;       // output rows per work item of the rows pass
constexpr int RH = 4;       // rows per lane of the columns pass
constexpr int MAX_TAPS = 66;  // 16:1 reduction: 4 * 16 + 2

__device__ __forceinline__ float fma_v(float w, float v, float acc) { return __fmaf_rn(w, v, acc); }
__device__ __forceinline__ f32x4 fma_v(float w, f32x4 v, f32x4 acc) {
  return f32x4{__fmaf_rn(w, v[0], acc[0]), __fmaf_rn(w, v[1], acc[1]), __fmaf_rn(w, v[2], acc[2]), __fmaf_rn(w, v[3], acc[3])};
}
__device__ __forceinline__ int clamp_start(int s, int n_in) { return min(max(s, 0), n_in - 1); }

// V = float: Wv = W; V = f32x4: Wv = W / 4.  Work item = (plane, group of RV output rows, 256-lane chunk of a row).
template <typename V>
__global__ __launch_bounds__(256) void resample_rows_kernel(const V* __restrict__ src, V* __restrict__ tmp, int64_t planes, int H,
                                                            int OH, int Wv, const int* __restrict__ start,
                                                            const float* __restrict__ weight, int K) {
  const int cpr = (Wv + 255) / 256, gpp = (OH + RV - 1) / RV;
  const int64_t items = planes * gpp * cpr;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t g = it / cpr;
    const int x = (int)(it - g * cpr) * 256 + (int)threadIdx.x;
    if (x >= Wv) continue;
    const int64_t p = g / gpp;
    const int oy0 = (int)(g - p * gpp) * RV, oy1 = min(oy0 + RV, OH);
    const V* sp = src + p * H * Wv;
    V* tp = tmp + p * OH * Wv;
    for (int oy = oy0; oy < oy1; ++oy) {
      const int s = clamp_start(start[oy], H);
      const float* w = weight + (int64_t)oy * K;
      V acc = V{};
#pragma unroll 4  // four taps' loads in flight; the fma chain keeps its order
      for (int t = 0; t < K; ++t) acc = fma_v(w[t], sp[(int64_t)min(s + t, H - 1) * Wv + x], acc);
      tp[(int64_t)oy * Wv + x] = acc;
    }
  }
}

// rows = planes * OH rows of tmp ([rows][W]) and of dst ([rows][OW]).  Work item = (group of RH rows, 256-lane chunk of a row).
__global__ __launch_bounds__(256) void resample_cols_kernel(const float* __restrict__ tmp, float* __restrict__ dst, int64_t rows,
                                                            int W, int OW, const int* __restrict__ start,
                                                            const float* __restrict__ weight, int K) {
  const int cpr = (OW + 255) / 256;
  const int64_t items = ((rows + RH - 1) / RH) * cpr;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t g = it / cpr;
    const int ox = (int)(it - g * cpr) * 256 + (int)threadIdx.x;
    if (ox >= OW) continue;
    const int64_t r0 = g * RH;
    const float* rp[RH];  // a ragged last group reads its last row again and stores nothing for it
#pragma unroll
    for (int r = 0; r < RH; ++r) rp[r] = tmp + min(r0 + r, rows - 1) * W;
    const int s = clamp_start(start[ox], W);
    const float* w = weight + (int64_t)ox * K;
    float acc[RH] = {};
#pragma unroll 2
    for (int t = 0; t < K; ++t) {
      const int x = min(s + t, W - 1);
      const float wt = w[t];
#pragma unroll
      for (int r = 0; r < RH; ++r) acc[r] = __fmaf_rn(wt, rp[r][x], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < RH; ++r)
      if (r0 + r < rows) dst[(r0 + r) * OW + ox] = acc[r];
  }
}

unsigned item_grid(int64_t items) {
  const int64_t cap = 16384;  // 256 CUs x 8 workgroups x 8 rounds, as dihedral.hip
  return (unsigned)(items < cap ? items : cap);
}

bool apart(uintptr_t a, uintptr_t a_bytes, uintptr_t b, uintptr_t b_bytes) { return a + a_bytes <= b || b + b_bytes <= a; }

}  // namespace

extern "C" int srx_resample_planes(const float* src, float* dst, int64_t planes, int H, int W, int OH, int OW, const int* start_y,
                                   const float* weight_y, int Ky, const int* start_x, const float* weight_x, int Kx, float* ws,
                                   size_t ws_floats, void* stream) {
  SRX_REQUIRE(src && dst && ws && start_y && weight_y && start_x && weight_x,
              "resample_planes: null pointer (src %p, dst %p, ws %p, start_y %p, weight_y %p, start_x %p, weight_x %p)",
              (const void*)src, (void*)dst, (void*)ws, (const void*)start_y, (const void*)weight_y, (const void*)start_x,
              (const void*)weight_x);
  SRX_REQUIRE(planes > 0 && H > 0 && W > 0 && OH > 0 && OW > 0,
              "resample_planes: planes, H, W, OH and OW must be positive (got %lld, %d, %d, %d, %d)", (long long)planes, H, W, OH,
              OW);
  SRX_REQUIRE(Ky >= 1 && Ky <= MAX_TAPS && Kx >= 1 && Kx <= MAX_TAPS,
              "resample_planes: tap counts must be in 1..%d (got Ky = %d, Kx = %d)", MAX_TAPS, Ky, Kx);
  const int64_t lim = (int64_t)1 << 31;
  SRX_REQUIRE((int64_t)H * W < lim && (int64_t)OH * OW < lim && (int64_t)OH * W < lim,
              "resample_planes: a plane must stay below 2^31 elements (H * W = %lld, OH * OW = %lld, workspace OH * W = %lld)",
              (long long)((int64_t)H * W), (long long)((int64_t)OH * OW), (long long)((int64_t)OH * W));
  SRX_REQUIRE(planes < ((int64_t)1 << 28), "resample_planes: planes = %lld passes 2^28", (long long)planes);  // x 2^31 x 4 bytes < 2^61
  const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst, w0 = (uintptr_t)ws;
  SRX_REQUIRE(s0 % 4 == 0 && d0 % 4 == 0 && w0 % 4 == 0 && (uintptr_t)start_y % 4 == 0 && (uintptr_t)weight_y % 4 == 0 &&
                  (uintptr_t)start_x % 4 == 0 && (uintptr_t)weight_x % 4 == 0,
              "resample_planes: src, dst, the workspace and the tables must be 4-byte aligned");
  const uint64_t need = (uint64_t)planes * OH * W;
  SRX_REQUIRE(ws_floats >= need, "resample_planes: the workspace holds %zu floats, [planes][OH][W] needs %llu", ws_floats,
              (unsigned long long)need);
  const uintptr_t sb = (uintptr_t)planes * H * W * 4, db = (uintptr_t)planes * OH * OW * 4, wb = (uintptr_t)need * 4;
  SRX_REQUIRE(apart(s0, sb, d0, db) && apart(s0, sb, w0, wb) && apart(d0, db, w0, wb),
              "resample_planes: src, dst and the workspace overlap (src %p + %zu, dst %p + %zu, ws %p + %zu bytes)",
              (const void*)src, (size_t)sb, (void*)dst, (size_t)db, (void*)ws, (size_t)wb);
  hipStream_t st = srx_stream(stream);
  const int64_t groups = planes * srx_cdiv(OH, RV);
  if (W % 4 == 0 && s0 % 16 == 0 && w0 % 16 == 0) {
    hipLaunchKernelGGL(resample_rows_kernel<f32x4>, dim3(item_grid(groups * srx_cdiv(W / 4, 256))), dim3(256), 0, st,
                       reinterpret_cast<const f32x4*>(src), reinterpret_cast<f32x4*>(ws), planes, H, OH, W / 4, start_y, weight_y, Ky);
  } else {
    hipLaunchKernelGGL(resample_rows_kernel<float>, dim3(item_grid(groups * srx_cdiv(W, 256))), dim3(256), 0, st, src, ws, planes, H,
                       OH, W, start_y, weight_y, Ky);
  }
  SRX_CHECK_LAUNCH("resample_rows_kernel");
  const int64_t rows = planes * OH;
  hipLaunchKernelGGL(resample_cols_kernel, dim3(item_grid(srx_cdiv(rows, RH) * srx_cdiv(OW, 256))), dim3(256), 0, st, ws, dst, rows, W,
                     OW, start_x, weight_x, Kx);
  SRX_CHECK_LAUNCH("resample_cols_kernel");
  return SRX_OK;
}
