// The eight flips / transposes of an image plane (the dihedral group D4) as one HBM-bound pass with the scaling and the
// accumulation of the geometric self-ensemble folded in (test.upscale(self_ensemble=n)):
//   dst[p][u][v] = alpha * src[p][y][x] + beta * dst[p][u][v],   (u, v) = T_k(y, x)
// k bit 0: transpose ((u, v) = (x, y), dst is [W][H]); then bit 1: v = W' - 1 - v; bit 2: u = H' - 1 - u.
// One read of src, one read-modify-write of dst (no read with beta == 0), rows on both sides:
//  - bit 0 clear: a row of src is a row of dst (reversed for bit 1, at another height for bit 2).  16-byte accesses when
//    W % 4 == 0 and both bases are 16-byte aligned (then every row is), the hflip reversing the quads of a row and the lanes of
//    a quad; scalar otherwise.
//  - bit 0 set: 64 x 64 tiles through LDS.  A wave stores one tile row (64 consecutive floats of a src row) and reads one tile
//    column; at a row pitch of 65 floats lane c of the column read sits on bank (c * 65 + r) % 32 = (c + r) % 32: 32 banks per
//    32-lane half, no conflict (pitch 64: all 64 lanes on one bank).  Ragged edge tiles are masked on both sides.
// Work items are a LINEAR index (tiles, or 256-wide row chunks) walked with a grid-stride loop -- no count in gridDim.y/z --
// and every plane / row base is 64-bit: a batch of 22 8K frames (three planes each) passes 2^31 elements.
// The sum is one fma per element, in a fixed place: two calls on the same buffers write the same bits.
#include "srx_common.h"

#include <cmath>

namespace {

constexpr int DT = 64;        // tile edge of the transposing form
constexpr int DT_PITCH = 65;  // LDS row pitch in floats (odd: see above)

__device__ __forceinline__ float blend(float s, float d, float alpha, float beta) { return __fmaf_rn(alpha, s, beta * d); }

// bit 0 clear, scalar.  Work item = (plane row, 256-element chunk of it).
template <bool READ_DST>
__global__ __launch_bounds__(256) void dihedral_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t rows,
                                                            int H, int W, int hflip, int vflip, float alpha, float beta) {
  const int cpr = (W + 255) / 256;
  const int64_t items = rows * cpr;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t row = it / cpr;
    const int x = (int)(it - row * cpr) * 256 + (int)threadIdx.x;
    if (x >= W) continue;
    const int64_t p = row / H;
    const int y = (int)(row - p * H);
    const int u = vflip ? H - 1 - y : y, v = hflip ? W - 1 - x : x;
    const float s = src[row * W + x];
    float* o = dst + (p * H + u) * W + v;
    *o = READ_DST ? blend(s, *o, alpha, beta) : alpha * s;
  }
}

// bit 0 clear, 16-byte accesses: W4 = W / 4 quads per row
template <bool READ_DST>
__global__ __launch_bounds__(256) void dihedral_rows4_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t rows,
                                                             int H, int W4, int hflip, int vflip, float alpha, float beta) {
  const int cpr = (W4 + 255) / 256;
  const int64_t items = rows * cpr;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t row = it / cpr;
    const int q = (int)(it - row * cpr) * 256 + (int)threadIdx.x;
    if (q >= W4) continue;
    const int64_t p = row / H;
    const int y = (int)(row - p * H);
    const int u = vflip ? H - 1 - y : y, v = hflip ? W4 - 1 - q : q;
    f32x4 s = *reinterpret_cast<const f32x4*>(src + (row * W4 + q) * 4);
    if (hflip) s = f32x4{s[3], s[2], s[1], s[0]};
    f32x4* o = reinterpret_cast<f32x4*>(dst + ((p * H + u) * W4 + v) * 4);
    f32x4 r;
    if (READ_DST) {
      const f32x4 d = *o;
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = blend(s[e], d[e], alpha, beta);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = alpha * s[e];
    }
    *o = r;
  }
}

// bit 0 set: src [planes][H][W] -> dst [planes][W][H].  Work item = (plane, tile row, tile column) of src.
template <bool READ_DST>
__global__ __launch_bounds__(256) void dihedral_transpose_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                 int64_t planes, int H, int W, int hflip, int vflip, float alpha,
                                                                 float beta) {
  __shared__ float tile[DT * DT_PITCH];
  const int ty = (H + DT - 1) / DT, tx = (W + DT - 1) / DT;
  const int64_t per_plane = (int64_t)ty * tx, items = planes * per_plane;
  const int lane = threadIdx.x & (DT - 1), r0 = threadIdx.x / DT;  // r0: 0..3, one wave each
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t p = it / per_plane;
    const int t = (int)(it - p * per_plane);
    const int y0 = (t / tx) * DT, x0 = (t % tx) * DT;
    const float* sp = src + p * H * W;
    float* dp = dst + p * H * W;
    const bool full = y0 + DT <= H && x0 + DT <= W;  // (uniform) no masks: all 16 loads of a thread in flight together
    // tile[r][c] = src[y0 + r][x0 + c]: a wave reads 64 consecutive floats of one src row
    if (full) {
      float v[DT / 4];
#pragma unroll
      for (int i = 0; i < DT / 4; ++i) v[i] = sp[(int64_t)(y0 + r0 + 4 * i) * W + x0 + lane];
#pragma unroll
      for (int i = 0; i < DT / 4; ++i) tile[(r0 + 4 * i) * DT_PITCH + lane] = v[i];
    } else if (x0 + lane < W) {
      for (int r = r0; r < DT && y0 + r < H; r += 4) tile[r * DT_PITCH + lane] = sp[(int64_t)(y0 + r) * W + x0 + lane];
    }
    __syncthreads();
    // dst row u comes from src column x0 + r, dst column v from src row y0 + lane: a wave writes 64 consecutive floats of one
    // dst row (descending with hflip).  dst is [W][H]: H' = W, W' = H.
    const int v = hflip ? H - 1 - (y0 + lane) : y0 + lane;
    if (full) {
      float* o[DT / 4];
      float d[DT / 4];
#pragma unroll
      for (int i = 0; i < DT / 4; ++i) {
        const int r = r0 + 4 * i, u = vflip ? W - 1 - (x0 + r) : x0 + r;
        o[i] = dp + (int64_t)u * H + v;
        if (READ_DST) d[i] = *o[i];
      }
#pragma unroll
      for (int i = 0; i < DT / 4; ++i) {
        const float s = tile[lane * DT_PITCH + r0 + 4 * i];
        *o[i] = READ_DST ? blend(s, d[i], alpha, beta) : alpha * s;
      }
    } else if (y0 + lane < H) {
      for (int r = r0; r < DT && x0 + r < W; r += 4) {
        const int u = vflip ? W - 1 - (x0 + r) : x0 + r;
        const float s = tile[lane * DT_PITCH + r];
        float* o = dp + (int64_t)u * H + v;
        *o = READ_DST ? blend(s, *o, alpha, beta) : alpha * s;
      }
    }
    __syncthreads();  // the next item overwrites the tile
  }
}

unsigned item_grid(int64_t items) {
  const int64_t cap = 16384;  // 256 CUs x 8 workgroups x 8 rounds: short items, a tail of 1 / 8 round at the most
  return (unsigned)(items < cap ? items : cap);
}

}  // namespace

extern "C" int srx_dihedral_planes(const float* src, float* dst, int64_t planes, int H, int W, int k, float alpha, float beta,
                                   void* stream) {
  SRX_REQUIRE(src && dst, "dihedral_planes: null pointer (src %p, dst %p)", (const void*)src, (void*)dst);
  SRX_REQUIRE(planes > 0 && H > 0 && W > 0, "dihedral_planes: planes, H and W must be positive (got %lld, %d, %d)",
              (long long)planes, H, W);
  SRX_REQUIRE(k >= 0 && k <= 7, "dihedral_planes: k = %d is no group element (0..7: bit 0 transpose, 1 hflip, 2 vflip)", k);
  SRX_REQUIRE(std::isfinite(alpha) && std::isfinite(beta), "dihedral_planes: alpha and beta must be finite (got %g, %g)",
              (double)alpha, (double)beta);
  SRX_REQUIRE((int64_t)H * W <= ((int64_t)1 << 60) / planes, "dihedral_planes: planes * H * W passes 2^60 elements");
  const int64_t n = planes * H * W;
  const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst, bytes = (uintptr_t)n * sizeof(float);
  SRX_REQUIRE(s0 % 4 == 0 && d0 % 4 == 0, "dihedral_planes: src and dst must be 4-byte aligned");
  SRX_REQUIRE(s0 + bytes <= d0 || d0 + bytes <= s0,
              "dihedral_planes: src and dst overlap (in place is not possible: a transposing element would read what it wrote)");
  hipStream_t st = srx_stream(stream);
  const int hflip = (k >> 1) & 1, vflip = (k >> 2) & 1;
  const bool rd = beta != 0.f;
  if (k & 1) {
    const int64_t items = planes * srx_cdiv(H, DT) * srx_cdiv(W, DT);
    if (rd)
      hipLaunchKernelGGL(dihedral_transpose_kernel<true>, dim3(item_grid(items)), dim3(256), 0, st, src, dst, planes, H, W, hflip,
                         vflip, alpha, beta);
    else
      hipLaunchKernelGGL(dihedral_transpose_kernel<false>, dim3(item_grid(items)), dim3(256), 0, st, src, dst, planes, H, W, hflip,
                         vflip, alpha, beta);
    SRX_CHECK_LAUNCH("dihedral_transpose_kernel");
    return SRX_OK;
  }
  const int64_t rows = planes * H;
  if (W % 4 == 0 && s0 % 16 == 0 && d0 % 16 == 0) {
    const int64_t items = rows * srx_cdiv(W / 4, 256);
    if (rd)
      hipLaunchKernelGGL(dihedral_rows4_kernel<true>, dim3(item_grid(items)), dim3(256), 0, st, src, dst, rows, H, W / 4, hflip, vflip,
                         alpha, beta);
    else
      hipLaunchKernelGGL(dihedral_rows4_kernel<false>, dim3(item_grid(items)), dim3(256), 0, st, src, dst, rows, H, W / 4, hflip, vflip,
                         alpha, beta);
    SRX_CHECK_LAUNCH("dihedral_rows4_kernel");
    return SRX_OK;
  }
  const int64_t items = rows * srx_cdiv(W, 256);
  if (rd)
    hipLaunchKernelGGL(dihedral_rows_kernel<true>, dim3(item_grid(items)), dim3(256), 0, st, src, dst, rows, H, W, hflip, vflip, alpha,
                       beta);
  else
    hipLaunchKernelGGL(dihedral_rows_kernel<false>, dim3(item_grid(items)), dim3(256), 0, st, src, dst, rows, H, W, hflip, vflip, alpha,
                       beta);
  SRX_CHECK_LAUNCH("dihedral_rows_kernel");
  return SRX_OK;
}
