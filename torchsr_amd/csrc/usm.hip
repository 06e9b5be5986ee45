// Unsharp-masked training targets on the device ('Sharpened targets'): Real-ESRGAN's USMSharp on float planes in
// [0, 1].  blur = G(x), mask = |x - blur| 255 > threshold, soft = G(mask), out = x + soft (clamp(x + weight (x - blur)) - x), with
// G the separable correlation with g (x) g of up to 51 taps, borders reflected.  Two launches, each one separable pass pair
// over a 32 x 32 tile: no atomics, no device state, fmas in ascending tap order -- the same bits from every call.
#include <cmath>

#include "srx_common.h"

namespace {

constexpr int kUsmMaxK = 51;                           // largest tap count; legal: the odd 3..51
constexpr int kUsmTile = 32;                           // a workgroup's outputs: 32 x 32 pixels of one plane
constexpr int kUsmExt = kUsmTile + kUsmMaxK - 1;       // the tile with its halo: 82 x 82
// pitch of the staged tile.  The horizontal pass reads it with ds_read_b32 from 4 rows x 8 column quads per 32-lane group:
// 83 mod 32 = 19 puts the four rows on banks 0, 19, 6, 25 -- one residue mod 4 each -- and the quads step by 4, so the 32
// addresses of a group fall on 32 banks (at the plain pitch of 82 rows 0 and 2 would share theirs)
constexpr int kUsmPitch = kUsmExt + 1;
// the horizontal pass's result, [82][32]: the vertical pass reads 32 consecutive floats of one row per 32-lane group, which is
// conflict-free at this pitch, so it needs no padding
constexpr int kUsmMidPitch = kUsmTile;

// reflect padding (torch's mode='reflect'): -k -> k, n-1+k -> n-1-k; exact for the k <= n-1 the host admits, and clamped so
// that the rows of a border tile that feed no output still read inside the plane
__device__ __forceinline__ int usm_reflect(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return min(max(i, 0), n - 1);
}

// G(src) on the workgroup's tile: thread t gets the four outputs of column (t & 31), rows 4 (t >> 5) .. + 3 of the tile in
// acc[].  Leaves the staged tile (halo r, pitch kUsmPitch) in ``tile`` for the caller.  256 threads; ends on a barrier-free
// read phase, so the caller may read ``tile`` but must not write LDS before its own barrier.
__device__ __forceinline__ void usm_tile_blur(const float* __restrict__ src, const float* __restrict__ taps, int ks, int H, int W,
                                              int ty0, int tx0, float* tile, float* mid, float* g, float acc[4]) {
  const int t = threadIdx.x, r = ks >> 1, ext = kUsmTile + 2 * r;
  if (t < ks) g[t] = taps[t];
  for (int i = t; i < ext * ext; i += 256) {
    const int py = i / ext, px = i - py * ext;
    tile[py * kUsmPitch + px] = src[(size_t)usm_reflect(ty0 - r + py, H) * W + usm_reflect(tx0 - r + px, W)];
  }
  __syncthreads();
  // horizontal: mid[py][x] = sum_j g[j] tile[py][x + j], thread t owns 4 columns of the rows t / 8, t / 8 + 32, ...
  const int lx = (t & 7) * 4;
  for (int py = t >> 3; py < ext; py += 32) {
    const float* row = tile + py * kUsmPitch + lx;  // columns lx .. lx + ks + 2 <= ext - 1
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    float v0 = row[0], v1 = row[1], v2 = row[2];
    for (int j = 0; j < ks; ++j) {
      const float v3 = row[j + 3], w = g[j];
      a0 = fmaf(w, v0, a0);
      a1 = fmaf(w, v1, a1);
      a2 = fmaf(w, v2, a2);
      a3 = fmaf(w, v3, a3);
      v0 = v1, v1 = v2, v2 = v3;
    }
    float* m = mid + py * kUsmMidPitch + lx;
    m[0] = a0, m[1] = a1, m[2] = a2, m[3] = a3;
  }
  __syncthreads();
  // vertical: out[y][x] = sum_i g[i] mid[y + i][x], thread t owns 4 rows of one column
  const float* col = mid + (t >> 5) * 4 * kUsmMidPitch + (t & 31);  // rows 4 (t >> 5) .. + ks + 2 <= ext - 1
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  float v0 = col[0], v1 = col[kUsmMidPitch], v2 = col[2 * kUsmMidPitch];
  for (int i = 0; i < ks; ++i) {
    const float v3 = col[(i + 3) * kUsmMidPitch], w = g[i];
    a0 = fmaf(w, v0, a0);
    a1 = fmaf(w, v1, a1);
    a2 = fmaf(w, v2, a2);
    a3 = fmaf(w, v3, a3);
    v0 = v1, v1 = v2, v2 = v3;
  }
  acc[0] = a0, acc[1] = a1, acc[2] = a2, acc[3] = a3;
}

// blur = G(in); mask = 1 where |in - blur| 255 > threshold, else 0.  grid: planes x tiles, 256 threads.
__global__ __launch_bounds__(256) void usm_blur_mask_kernel(const float* __restrict__ in, float* __restrict__ blur,
                                                            float* __restrict__ mask, const float* __restrict__ taps, int ks,
                                                            int H, int W, int tiles_x, int tiles, float threshold) {
  __shared__ float g[kUsmMaxK];
  __shared__ float tile[kUsmExt * kUsmPitch];
  __shared__ float mid[kUsmExt * kUsmMidPitch];
  const int64_t plane = blockIdx.x / (unsigned)tiles;
  const int tl = (int)(blockIdx.x - plane * tiles), t = threadIdx.x, r = ks >> 1;
  const int ty0 = (tl / tiles_x) * kUsmTile, tx0 = (tl % tiles_x) * kUsmTile;
  const size_t base = (size_t)plane * H * W;
  float acc[4];
  usm_tile_blur(in + base, taps, ks, H, W, ty0, tx0, tile, mid, g, acc);
  const int lx = t & 31, ly = (t >> 5) * 4, x = tx0 + lx;
  if (x >= W) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int y = ty0 + ly + e;
    if (y >= H) break;
    const float v = tile[(r + ly + e) * kUsmPitch + r + lx];  // the pixel itself: the centre of the staged tile
    const size_t at = base + (size_t)y * W + x;
    blur[at] = acc[e];
    mask[at] = fabsf(v - acc[e]) * 255.f > threshold ? 1.f : 0.f;
  }
}

// soft = G(mask); out = x + soft (clamp(x + weight (x - blur), 0, 1) - x).  grid: planes x tiles, 256 threads.
__global__ __launch_bounds__(256) void usm_blend_kernel(const float* __restrict__ in, const float* __restrict__ blur,
                                                        const float* __restrict__ mask, float* __restrict__ out,
                                                        const float* __restrict__ taps, int ks, int H, int W, int tiles_x,
                                                        int tiles, float weight) {
  __shared__ float g[kUsmMaxK];
  __shared__ float tile[kUsmExt * kUsmPitch];
  __shared__ float mid[kUsmExt * kUsmMidPitch];
  const int64_t plane = blockIdx.x / (unsigned)tiles;
  const int tl = (int)(blockIdx.x - plane * tiles), t = threadIdx.x;
  const int ty0 = (tl / tiles_x) * kUsmTile, tx0 = (tl % tiles_x) * kUsmTile;
  const size_t base = (size_t)plane * H * W;
  float soft[4];
  usm_tile_blur(mask + base, taps, ks, H, W, ty0, tx0, tile, mid, g, soft);
  const int lx = t & 31, ly = (t >> 5) * 4, x = tx0 + lx;
  if (x >= W) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int y = ty0 + ly + e;
    if (y >= H) break;
    const size_t at = base + (size_t)y * W + x;
    const float v = in[at];
    const float sharp = fminf(fmaxf(fmaf(weight, v - blur[at], v), 0.f), 1.f);
    out[at] = fmaf(soft[e], sharp - v, v);  // weight = 0 or soft = 0: v itself, bit for bit
  }
}

bool usm_apart(uintptr_t a, uintptr_t b, uintptr_t bytes) { return a + bytes <= b || b + bytes <= a; }

}  // namespace

extern "C" int srx_usm_sharpen(const float* in, float* out, float* blur, float* mask, const float* taps, int ksize,
                               int64_t planes, int H, int W, float weight, float threshold, void* stream) {
  SRX_REQUIRE(in && out && blur && mask && taps, "usm_sharpen: null pointer (in %p, out %p, blur %p, mask %p, taps %p)",
              (const void*)in, (void*)out, (void*)blur, (void*)mask, (const void*)taps);
  SRX_REQUIRE(ksize >= 3 && ksize <= kUsmMaxK && (ksize & 1), "usm_sharpen: ksize must be odd and in 3..%d, got %d", kUsmMaxK,
              ksize);
  SRX_REQUIRE(H > ksize / 2 && W > ksize / 2, "usm_sharpen: %d x %d planes: a %d-tap reflect needs %d rows and columns", H, W,
              ksize, ksize / 2 + 1);
  SRX_REQUIRE(planes >= 1, "usm_sharpen: planes must be positive, got %lld", (long long)planes);
  const int64_t lim = (int64_t)1 << 31, hw = (int64_t)H * W;
  SRX_REQUIRE(hw < lim && planes <= (lim - 1) / hw, "usm_sharpen: planes * H * W must stay below 2^31 (got %lld x %d x %d)",
              (long long)planes, H, W);
  SRX_REQUIRE(std::isfinite(weight) && std::isfinite(threshold), "usm_sharpen: weight and threshold must be finite (got %g, %g)",
              (double)weight, (double)threshold);
  const uintptr_t bytes = (uintptr_t)(planes * hw) * 4;
  const uintptr_t p[4] = {(uintptr_t)in, (uintptr_t)out, (uintptr_t)blur, (uintptr_t)mask};
  for (int a = 0; a < 4; ++a)
    for (int b = a + 1; b < 4; ++b)
      SRX_REQUIRE(usm_apart(p[a], p[b], bytes), "usm_sharpen: in, out, blur and mask must not overlap (in %p, out %p, blur %p, mask %p, %zu bytes each)",
                  (const void*)in, (void*)out, (void*)blur, (void*)mask, (size_t)bytes);
  const int tiles_x = (int)srx_cdiv(W, kUsmTile), tiles = tiles_x * (int)srx_cdiv(H, kUsmTile);  // <= H W < 2^31
  const int64_t blocks = planes * tiles;                                                          // <= planes H W < 2^31
  hipStream_t st = srx_stream(stream);
  hipLaunchKernelGGL(usm_blur_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, st, in, blur, mask, taps, ksize, H, W, tiles_x,
                     tiles, threshold);
  SRX_CHECK_LAUNCH("usm_blur_mask_kernel");
  hipLaunchKernelGGL(usm_blend_kernel, dim3((unsigned)blocks), dim3(256), 0, st, in, blur, mask, out, taps, ksize, H, W, tiles_x,
                     tiles, weight);
  SRX_CHECK_LAUNCH("usm_blend_kernel");
  return SRX_OK;
}
