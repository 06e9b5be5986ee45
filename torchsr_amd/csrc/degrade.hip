// Blind degradation of the training data on the device ('Blind degradation'): the first-order model of
// BSRGAN / Real-ESRGAN -- blur, resize, sensor noise, JPEG -- around augment.hip's srx_bicubic_down, and the table-driven
// filter of its second-order model ('Second-order degradation'), its Poisson noise ('Poisson noise') and its 4:2:0 JPEG
// ('Chroma subsampling').  Kernels over a
// batch of float NCHW images in [0, 1]; every per-sample parameter is read on the device, so each kernel is safe for any
// value it finds there (a kernel size outside the legal set is clamped into it, a quality outside 1..100 passes through).
#include "srx_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ anisotropic Gaussian blur
constexpr int kBlurMaxK = 21;                             // largest kernel size; legal sizes: 0 (copy) and the odd 1..21
constexpr int kBlurTile = 32;                             // a workgroup's outputs: 32 x 32 pixels of one plane
constexpr int kBlurPitch = kBlurTile + kBlurMaxK - 1;     // the tile with its halo: 52 x 52

__device__ __forceinline__ int blur_legal_ksize(int k) {
  if (k <= 0) return 0;
  k |= 1;
  return k > kBlurMaxK ? kBlurMaxK : k;
}

// reflect padding (torch's mode='reflect'): -k -> k, n-1+k -> n-1-k; exact for the k <= n-1 the host admits, and clamped so
// that the rows of a border tile that feed no output still read inside the plane
__device__ __forceinline__ int blur_reflect(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return min(max(i, 0), n - 1);
}

// out[n][c][y][x] = sum_ij w_n[i][j] in[n][c][y + i - r][x + j - r], w_n = exp(-v' S^-1 v / 2) / sum, v = (j - r, i - r),
// S = R(theta) diag(sx^2, sy^2) R(theta)'.  grid (tiles, C, N), 256 threads: thread t owns 4 pixels of row t / 8.
__global__ __launch_bounds__(256) void blur_aniso_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                         const float* __restrict__ parm, const int* __restrict__ ksize,
                                                         int C, int H, int W, int tiles_x) {
  __shared__ float wl[kBlurMaxK * kBlurMaxK];
  __shared__ float tile[kBlurPitch * kBlurPitch];
  __shared__ float wpart[4];
  const int n = blockIdx.z, c = blockIdx.y, t = threadIdx.x;
  const int ty0 = (int)(blockIdx.x / tiles_x) * kBlurTile, tx0 = (int)(blockIdx.x % tiles_x) * kBlurTile;
  const int ks = blur_legal_ksize(ksize[n]), r = ks >> 1;
  const float* src = in + ((size_t)n * C + c) * H * W;
  float* dst = out + ((size_t)n * C + c) * H * W;
  const int lx = (t & 7) * 4, ly = t >> 3;
  const int y = ty0 + ly;
  if (ks == 0) {  // the sample passes through, bit for bit
    if (y < H)
      for (int e = 0; e < 4; ++e)
        if (tx0 + lx + e < W) dst[(size_t)y * W + tx0 + lx + e] = src[(size_t)y * W + tx0 + lx + e];
    return;
  }
  // the sample's weights, once per workgroup
  const float sx = fmaxf(parm[4 * n], 1e-6f), sy = fmaxf(parm[4 * n + 1], 1e-6f);
  float sn, cs;
  sincosf(parm[4 * n + 2], &sn, &cs);
  float part = 0.f;
  for (int i = t; i < ks * ks; i += 256) {
    const int ti = i / ks, tj = i - ti * ks;
    const float dx = (float)(tj - r), dy = (float)(ti - r);
    const float a = (cs * dx + sn * dy) / sx, b = (cs * dy - sn * dx) / sy;  // R' v, scaled by the axes
    const float w = expf(-0.5f * (a * a + b * b));
    wl[i] = w;
    part += w;
  }
  part = srx_wave_sum(part);
  if ((t & 63) == 0) wpart[t >> 6] = part;
  // the tile and its halo of r pixels, reflected at the plane's borders
  const int ext = kBlurTile + 2 * r;
  for (int i = t; i < ext * ext; i += 256) {
    const int py = i / ext, px = i - py * ext;
    tile[py * kBlurPitch + px] = src[(size_t)blur_reflect(ty0 - r + py, H) * W + blur_reflect(tx0 - r + px, W)];
  }
  __syncthreads();
  const float total = (wpart[0] + wpart[1]) + (wpart[2] + wpart[3]);  // >= 1: the centre tap is exp(0)
  __syncthreads();
  for (int i = t; i < ks * ks; i += 256) wl[i] = wl[i] / total;
  __syncthreads();
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int i = 0; i < ks; ++i) {
    const float* row = tile + (ly + i) * kBlurPitch + lx;  // columns lx .. lx + ks + 2 <= ext - 1
    const float* wr = wl + i * ks;
    float v0 = row[0], v1 = row[1], v2 = row[2];
    for (int j = 0; j < ks; ++j) {
      const float v3 = row[j + 3], w = wr[j];
      a0 = fmaf(w, v0, a0);
      a1 = fmaf(w, v1, a1);
      a2 = fmaf(w, v2, a2);
      a3 = fmaf(w, v3, a3);
      v0 = v1, v1 = v2, v2 = v3;
    }
  }
  if (y < H) {
    const float acc[4] = {a0, a1, a2, a3};
    for (int e = 0; e < 4; ++e)
      if (tx0 + lx + e < W) dst[(size_t)y * W + tx0 + lx + e] = acc[e];
  }
}

// ------------------------------------------------------------------------------------------------ per-sample 2-D filter
// out[n][c][y][x] = sum_ij w_n[i][j] in[n][c][y + i - r][x + j - r] with the weights as an operand: sample n's ks x ks kernel sits
// centred in its 21 x 21 slot of ``weights`` and is used as given (sinc kernels have negative lobes), nothing outside that
// window is read.  blur_aniso_kernel's tiling and order of fmas; the weight phase is a load.  grid (tiles, C, N), 256 threads.
__device__ __forceinline__ float filter_quantize(float v) { return rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f) * (1.0f / 255.0f); }

__global__ __launch_bounds__(256) void filter2d_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                       const float* __restrict__ weights, const int* __restrict__ ksize,
                                                       int C, int H, int W, int tiles_x, int quantize) {
  __shared__ float wl[kBlurMaxK * kBlurMaxK];
  __shared__ float tile[kBlurPitch * kBlurPitch];
  const int n = blockIdx.z, c = blockIdx.y, t = threadIdx.x;
  const int ty0 = (int)(blockIdx.x / tiles_x) * kBlurTile, tx0 = (int)(blockIdx.x % tiles_x) * kBlurTile;
  const int ks = blur_legal_ksize(ksize[n]), r = ks >> 1;
  const float* src = in + ((size_t)n * C + c) * H * W;
  float* dst = out + ((size_t)n * C + c) * H * W;
  const int lx = (t & 7) * 4, ly = t >> 3;
  const int y = ty0 + ly;
  if (ks == 0) {  // the sample passes through: bit for bit, or rounded to 8 bits
    if (y < H)
      for (int e = 0; e < 4; ++e)
        if (tx0 + lx + e < W) {
          const float v = src[(size_t)y * W + tx0 + lx + e];
          dst[(size_t)y * W + tx0 + lx + e] = quantize ? filter_quantize(v) : v;
        }
    return;
  }
  // the centred ks x ks window of the sample's slot, once per workgroup
  const float* slot = weights + (size_t)n * (kBlurMaxK * kBlurMaxK) + (kBlurMaxK / 2 - r) * (kBlurMaxK + 1);
  for (int i = t; i < ks * ks; i += 256) {
    const int ti = i / ks, tj = i - ti * ks;
    wl[i] = slot[ti * kBlurMaxK + tj];
  }
  // the tile and its halo of r pixels, reflected at the plane's borders
  const int ext = kBlurTile + 2 * r;
  for (int i = t; i < ext * ext; i += 256) {
    const int py = i / ext, px = i - py * ext;
    tile[py * kBlurPitch + px] = src[(size_t)blur_reflect(ty0 - r + py, H) * W + blur_reflect(tx0 - r + px, W)];
  }
  __syncthreads();
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int i = 0; i < ks; ++i) {
    const float* row = tile + (ly + i) * kBlurPitch + lx;  // columns lx .. lx + ks + 2 <= ext - 1
    const float* wr = wl + i * ks;
    float v0 = row[0], v1 = row[1], v2 = row[2];
    for (int j = 0; j < ks; ++j) {
      const float v3 = row[j + 3], w = wr[j];
      a0 = fmaf(w, v0, a0);
      a1 = fmaf(w, v1, a1);
      a2 = fmaf(w, v2, a2);
      a3 = fmaf(w, v3, a3);
      v0 = v1, v1 = v2, v2 = v3;
    }
  }
  if (y < H) {
    const float acc[4] = {a0, a1, a2, a3};
    for (int e = 0; e < 4; ++e)
      if (tx0 + lx + e < W) dst[(size_t)y * W + tx0 + lx + e] = quantize ? filter_quantize(acc[e]) : acc[e];
  }
}

// ------------------------------------------------------------------------------------------------ Gaussian noise, Philox4x32-10
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t r[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  r[0] = c0, r[1] = c1, r[2] = c2, r[3] = c3;
}

// u = ((r >> 8) + 0.5) 2^-24 lies in (0, 1), but the upper half of those values has 25 significant bits.  Both helpers
// therefore hand their library function an argument that IS exact in fp32: u itself below 1/2, u - 1 above.
__device__ __forceinline__ float philox_log_u(uint32_t r) {  // ln u
  const uint32_t m = r >> 8;
  if (m < (1u << 23)) return logf(((float)m + 0.5f) * 0x1p-24f);
  return log1pf(-((float)(0xFFFFFFu - m) + 0.5f) * 0x1p-24f);
}
__device__ __forceinline__ void philox_sincos_u(uint32_t r, float* s, float* c) {  // sin, cos of 2 pi u = those of 2 pi (u - 1)
  const uint32_t m = r >> 8;
  const float u = m < (1u << 23) ? ((float)m + 0.5f) * 0x1p-24f : -((float)(0xFFFFFFu - m) + 0.5f) * 0x1p-24f;
  sincosf(6.283185307179586f * u, s, c);
}

// out[n][c][p] = in[n][c][p] + sigma[n] z_c(n, p); one Philox call per pixel: counter (p, n, 0, 0), key (seed_lo, seed_hi)
__global__ void add_gaussian_noise_kernel(const float* __restrict__ in, float* __restrict__ out,
                                          const float* __restrict__ sigma, const int* __restrict__ gray, uint32_t seed_lo,
                                          uint32_t seed_hi, int N, int HW, int quantize) {
  const int64_t total = (int64_t)N * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i / HW), p = (int)(i - (int64_t)n * HW);
    uint32_t r[4];
    philox4x32_10((uint32_t)p, (uint32_t)n, 0u, 0u, seed_lo, seed_hi, r);
    float s01, c01, s23, c23;
    philox_sincos_u(r[1], &s01, &c01);
    philox_sincos_u(r[3], &s23, &c23);
    const float rad0 = sqrtf(-2.f * philox_log_u(r[0])), rad2 = sqrtf(-2.f * philox_log_u(r[2]));
    const bool g = gray[n] != 0;
    const float z[3] = {rad0 * c01, g ? rad0 * c01 : rad0 * s01, g ? rad0 * c01 : rad2 * c23};
    const float sg = sigma[n];
    const size_t base = (size_t)n * 3 * HW + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = in[base + (size_t)c * HW] + sg * z[c];
      if (quantize) v = rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f) * (1.0f / 255.0f);
      out[base + (size_t)c * HW] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------ Poisson noise, table-driven
// Real-ESRGAN's generate_poisson_noise_pt per sample: q = the 8-bit level of a value (of its BT.601 luma when the sample is
// grey), vals = the number of distinct q of the whole sample rounded up to a power of two, k ~ Poisson(q vals / 255),
// out = in + scale (k / vals - q / 255).  Two kernels: which levels a sample holds, then one draw per value from host-made
// threshold tables (degradation.poisson_table_words), so that no float decides an integer on the device.
constexpr int kPoissonWindow = 256;                    // thresholds per packed row
constexpr int kPoissonFirstWords = 9 * 256;            // first[9][256] in front of win[9][256][kPoissonWindow]

// The three helpers below switch contraction off: hipcc's default would fuse their products and sums into fmas (the __f*_rn
// intrinsics are plain operators to it), differently in each kernel that inlines them.  With it off every operation is rounded
// once, both kernels get the same level for a value, and a float32 restatement gets the same bits.
__device__ __forceinline__ int poisson_level(float v) {  // 0..255, NaN: 0
#pragma clang fp contract(off)
  return (int)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f);
}
__device__ __forceinline__ float poisson_luma(float r, float g, float b) {
#pragma clang fp contract(off)
  const float pr = .299f * r, pg = .587f * g, pb = .114f * b;
  return (pr + pg) + pb;
}
// k / vals - q / 255: k inv is exact (inv a power of two), the product with 1 / 255 and the difference are rounded once each
__device__ __forceinline__ float poisson_offset(int k, float inv, int q) {
#pragma clang fp contract(off)
  const float a = (float)k * inv, t = (float)q * (1.0f / 255.0f);
  return a - t;
}

// levels[n][8]: bit q of the 256-bit mask is set when some value of sample n has level q.  The caller cleared it.  A
// workgroup collects its pixels' levels in LDS and merges at most 8 words.  grid (blocks, N), 256 threads.
__global__ __launch_bounds__(256) void poisson_levels_kernel(const float* __restrict__ in, const float* __restrict__ scale,
                                                             const int* __restrict__ gray, int* __restrict__ levels, int HW) {
  __shared__ unsigned int mask[8];
  const int n = blockIdx.y, t = threadIdx.x;
  if (scale[n] == 0.f) return;  // the sample is copied: nothing reads its mask (the whole workgroup leaves)
  if (t < 8) mask[t] = 0u;
  __syncthreads();
  const bool g = gray[n] != 0;
  const float* src = in + (size_t)n * 3 * HW;
  for (int64_t p = (int64_t)blockIdx.x * 256 + t; p < HW; p += (int64_t)gridDim.x * 256) {
    const float r = src[p], gg = src[p + (size_t)HW], b = src[p + 2 * (size_t)HW];
    if (g) {
      const int q = poisson_level(poisson_luma(r, gg, b));
      atomicOr(&mask[q >> 5], 1u << (q & 31));
    } else {
      const int q0 = poisson_level(r), q1 = poisson_level(gg), q2 = poisson_level(b);
      atomicOr(&mask[q0 >> 5], 1u << (q0 & 31));
      atomicOr(&mask[q1 >> 5], 1u << (q1 & 31));
      atomicOr(&mask[q2 >> 5], 1u << (q2 & 31));
    }
  }
  __syncthreads();
  if (t < 8 && mask[t]) atomicOr(reinterpret_cast<unsigned int*>(levels) + (size_t)n * 8 + t, mask[t]);
}

// the smallest k with u < T[level][k]: first + the number of the window's (non-decreasing) thresholds that are <= u
__device__ __forceinline__ int poisson_draw(const int* __restrict__ tables, int v, int level, uint32_t r) {
  const int rowi = v * 256 + level;
  const uint32_t* row = reinterpret_cast<const uint32_t*>(tables) + kPoissonFirstWords + (size_t)rowi * kPoissonWindow;
  const uint32_t u = r >> 1;
  int lo = 0, hi = kPoissonWindow;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;  // <= 255
    if (row[mid] <= u) lo = mid + 1; else hi = mid;
  }
  return tables[rowi] + lo;
}

// one thread per pixel; one Philox call per pixel: counter (p, n, 1, 0), key (seed_lo, seed_hi); word c feeds channel c, word 0
// all three of a grey sample
__global__ void add_poisson_noise_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ scale,
                                         const int* __restrict__ gray, const int* __restrict__ tables,
                                         const int* __restrict__ levels, uint32_t seed_lo, uint32_t seed_hi, int N, int HW,
                                         int quantize) {
  const int64_t total = (int64_t)N * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i / HW), p = (int)(i - (int64_t)n * HW);
    const size_t base = (size_t)n * 3 * HW + p;
    const float x[3] = {in[base], in[base + (size_t)HW], in[base + 2 * (size_t)HW]};
    const float sc = scale[n];
    if (sc == 0.f) {  // bit for bit
#pragma unroll
      for (int c = 0; c < 3; ++c) out[base + (size_t)c * HW] = x[c];
      continue;
    }
    int count = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) count += __popc((unsigned int)levels[(size_t)n * 8 + w]);
    // vals = count rounded up to a power of two = 2^v, v in 0..8 (count is 1..256 for a sample the levels kernel has seen)
    const int v = count <= 1 ? 0 : min(32 - __clz(count - 1), 8);
    const float inv = 1.0f / (float)(1 << v);  // exact
    uint32_t r[4];
    philox4x32_10((uint32_t)p, (uint32_t)n, 1u, 0u, seed_lo, seed_hi, r);
    const bool g = gray[n] != 0;
    float noise[3];
    if (g) {
      const int q = poisson_level(poisson_luma(x[0], x[1], x[2]));
      const int k = poisson_draw(tables, v, q, r[0]);
      noise[0] = noise[1] = noise[2] = poisson_offset(k, inv, q);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int q = poisson_level(x[c]);
        const int k = poisson_draw(tables, v, q, r[c]);
        noise[c] = poisson_offset(k, inv, q);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float o = fmaf(sc, noise[c], x[c]);  // three roundings in all: q / 255, the difference, this one (k / vals is exact)
      if (quantize) o = rintf(fminf(fmaxf(o, 0.f), 1.f) * 255.f) * (1.0f / 255.0f);
      out[base + (size_t)c * HW] = o;
    }
  }
}

// ------------------------------------------------------------------------------------------------ JPEG, 4:4:4, no entropy coding
// D[k][n] = c_k / 2 cos((2 n + 1) k pi / 16), c_0 = 1 / sqrt(2): the orthonormal 8-point DCT-II, rounded to fp32
__constant__ float kDct[64] = {
    0.3535533845424652f, 0.3535533845424652f, 0.3535533845424652f, 0.3535533845424652f, 0.3535533845424652f, 0.3535533845424652f, 0.3535533845424652f, 0.3535533845424652f,
    0.49039262533187866f, 0.41573479771614075f, 0.27778512239456177f, 0.09754516184329987f, -0.09754516184329987f, -0.27778512239456177f, -0.41573479771614075f, -0.49039262533187866f,
    0.4619397521018982f, 0.19134171307086945f, -0.19134171307086945f, -0.4619397521018982f, -0.4619397521018982f, -0.19134171307086945f, 0.19134171307086945f, 0.4619397521018982f,
    0.41573479771614075f, -0.09754516184329987f, -0.49039262533187866f, -0.27778512239456177f, 0.27778512239456177f, 0.49039262533187866f, 0.09754516184329987f, -0.41573479771614075f,
    0.3535533845424652f, -0.3535533845424652f, -0.3535533845424652f, 0.3535533845424652f, 0.3535533845424652f, -0.3535533845424652f, -0.3535533845424652f, 0.3535533845424652f,
    0.27778512239456177f, -0.49039262533187866f, 0.09754516184329987f, 0.41573479771614075f, -0.41573479771614075f, -0.09754516184329987f, 0.49039262533187866f, -0.27778512239456177f,
    0.19134171307086945f, -0.4619397521018982f, 0.4619397521018982f, -0.19134171307086945f, -0.19134171307086945f, 0.4619397521018982f, -0.4619397521018982f, 0.19134171307086945f,
    0.09754516184329987f, -0.27778512239456177f, 0.41573479771614075f, -0.49039262533187866f, 0.49039262533187866f, -0.41573479771614075f, 0.27778512239456177f, -0.09754516184329987f};
// ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), row-major: [vertical frequency][horizontal frequency]
__constant__ int kJpegBase[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// One wave per 8 x 8 block, lane = (row a, column b) = lane / 8, lane % 8, holding the block's three planes; the two 8-point
// passes of each transform go through LDS.  grid (W / 8, H / 8, N), 64 threads.
__global__ __launch_bounds__(64) void jpeg_sim_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                      const int* __restrict__ quality, int H, int W, int quantize) {
  __shared__ float buf[3][64];
  const int n = blockIdx.z, lane = threadIdx.x, a = lane >> 3, b = lane & 7;
  const size_t HW = (size_t)H * W;
  const size_t at = (size_t)n * 3 * HW + (size_t)(blockIdx.y * 8 + a) * W + blockIdx.x * 8 + b;
  const float fr = in[at], fg = in[at + HW], fb = in[at + 2 * HW];
  const int q = quality[n];
  if (q < 1 || q > 100) {  // not a JPEG quality: the sample passes through, bit for bit (the whole wave takes this branch)
    out[at] = fr, out[at + HW] = fg, out[at + 2 * HW] = fb;
    return;
  }
  const int R = (int)fminf(fmaxf(rintf(fr * 255.f), 0.f), 255.f), G = (int)fminf(fmaxf(rintf(fg * 255.f), 0.f), 255.f),
            B = (int)fminf(fmaxf(rintf(fb * 255.f), 0.f), 255.f);
  // libjpeg's rgb_ycc_convert, 16-bit fixed point
  float v[3];
  v[0] = (float)(((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128);
  v[1] = (float)(((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16) - 128);
  v[2] = (float)(((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16) - 128);
  const int scale = q < 50 ? 5000 / q : 200 - 2 * q;  // libjpeg's jpeg_quality_scaling
#pragma unroll
  for (int p = 0; p < 3; ++p) buf[p][lane] = v[p];
  __syncthreads();
  // forward, columns: T[a][b] = sum_m D[a][m] X[m][b]
  float t[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int p = 0; p < 3; ++p) t[p] = fmaf(kDct[a * 8 + m], buf[p][m * 8 + b], t[p]);
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 3; ++p) buf[p][lane] = t[p];
  __syncthreads();
  // forward, rows: F[a][b] = sum_m T[a][m] D[b][m]; then quantise and dequantise
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    float f = 0.f;
#pragma unroll
    for (int m = 0; m < 8; ++m) f = fmaf(buf[p][a * 8 + m], kDct[b * 8 + m], f);
    const int step = min(max((kJpegBase[p ? 1 : 0][lane] * scale + 50) / 100, 1), 255);
    t[p] = rintf(f / (float)step) * (float)step;
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 3; ++p) buf[p][lane] = t[p];
  __syncthreads();
  // inverse, columns: U[a][b] = sum_k D[k][a] F[k][b]
#pragma unroll
  for (int p = 0; p < 3; ++p) t[p] = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k)
#pragma unroll
    for (int p = 0; p < 3; ++p) t[p] = fmaf(kDct[k * 8 + a], buf[p][k * 8 + b], t[p]);
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 3; ++p) buf[p][lane] = t[p];
  __syncthreads();
  // inverse, rows: X[a][b] = sum_k U[a][k] D[k][b]; the decoded samples stay unrounded
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    float x = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) x = fmaf(buf[p][a * 8 + k], kDct[k * 8 + b], x);
    v[p] = x;  // Y - 128, Cb - 128, Cr - 128
  }
  const float yy = v[0] + 128.f;
  float rgb[3] = {yy + 1.402f * v[2], yy - 0.344136286f * v[1] - 0.714136286f * v[2], yy + 1.772f * v[1]};
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    float o = fminf(fmaxf(rgb[p] * (1.0f / 255.0f), 0.f), 1.f);
    if (quantize) o = rintf(o * 255.f) * (1.0f / 255.0f);
    out[at + p * HW] = o;
  }
}

// ------------------------------------------------------------------------------------------------ JPEG, 4:2:0 per sample
// srx_jpeg_sim2 ('Chroma subsampling').  The pieces below restate jpeg_sim_kernel's arithmetic expression for
// expression, so that a sample whose flag is 0 leaves srx_jpeg_sim2 with the bits srx_jpeg_sim gives it.
__device__ __forceinline__ int jpeg_level(float f) { return (int)fminf(fmaxf(rintf(f * 255.f), 0.f), 255.f); }

// The codec of P planes of one 8 x 8 block held one sample per lane in v[]: DCT, quantise, dequantise, inverse DCT, in place.
// Plane p takes the chrominance table when first_table + p > 0.  quot (nullable): coefficient / step before the rounding goes
// to quot[p * quot_stride + lane].  Every lane of the workgroup's one wave must arrive (the passes meet at barriers).
template <int P>
__device__ __forceinline__ void jpeg_codec(float (*buf)[64], float (&v)[P], int lane, int scale, int first_table,
                                           float* __restrict__ quot, size_t quot_stride) {
  const int a = lane >> 3, b = lane & 7;
#pragma unroll
  for (int p = 0; p < P; ++p) buf[p][lane] = v[p];
  __syncthreads();
  // forward, columns: T[a][b] = sum_m D[a][m] X[m][b]
  float t[P];
#pragma unroll
  for (int p = 0; p < P; ++p) t[p] = 0.f;
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int p = 0; p < P; ++p) t[p] = fmaf(kDct[a * 8 + m], buf[p][m * 8 + b], t[p]);
  __syncthreads();
#pragma unroll
  for (int p = 0; p < P; ++p) buf[p][lane] = t[p];
  __syncthreads();
  // forward, rows: F[a][b] = sum_m T[a][m] D[b][m]; then quantise and dequantise
#pragma unroll
  for (int p = 0; p < P; ++p) {
    float f = 0.f;
#pragma unroll
    for (int m = 0; m < 8; ++m) f = fmaf(buf[p][a * 8 + m], kDct[b * 8 + m], f);
    const int step = min(max((kJpegBase[(first_table + p) ? 1 : 0][lane] * scale + 50) / 100, 1), 255);
    const float quotient = f / (float)step;
    if (quot) quot[p * quot_stride + lane] = quotient;
    t[p] = rintf(quotient) * (float)step;
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < P; ++p) buf[p][lane] = t[p];
  __syncthreads();
  // inverse, columns: U[a][b] = sum_k D[k][a] F[k][b]
#pragma unroll
  for (int p = 0; p < P; ++p) t[p] = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k)
#pragma unroll
    for (int p = 0; p < P; ++p) t[p] = fmaf(kDct[k * 8 + a], buf[p][k * 8 + b], t[p]);
  __syncthreads();
#pragma unroll
  for (int p = 0; p < P; ++p) buf[p][lane] = t[p];
  __syncthreads();
  // inverse, rows: X[a][b] = sum_k U[a][k] D[k][b]; the decoded samples stay unrounded
#pragma unroll
  for (int p = 0; p < P; ++p) {
    float x = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) x = fmaf(buf[p][a * 8 + k], kDct[k * 8 + b], x);
    v[p] = x;
  }
}

// The padded chroma planes of srx_jpeg_sim2's workspace: float [N][2][8 CHB][8 CWB], CHB = ceil(H / 16), CWB = ceil(W / 16)
__host__ __device__ __forceinline__ int jpeg420_blocks(int extent) { return (extent + 15) / 16; }

// The chroma launch: one wave per 8 x 8 block of the padded H/2 x W/2 chroma planes, lane = sample.  A lane gathers the 2 x 2
// pixels under its sample -- under the plane's edge sample where the block reaches past the plane: the replication that
// pads a partial 16 x 16 MCU -- averages their integer Cb and Cr as libjpeg's h2v2_downsample does, and writes the decoded
// block to ws.  Samples that are not 4:2:0 (flag 0, or a quality outside 1..100) are left to the luma launch.
// grid (CWB, CHB, N), 64 threads.
__global__ __launch_bounds__(64) void jpeg420_chroma_kernel(const float* __restrict__ in, const int* __restrict__ quality,
                                                            const int* __restrict__ chroma420, float* __restrict__ ws,
                                                            float* __restrict__ quot_out, int H, int W) {
  __shared__ float buf[2][64];
  const int n = blockIdx.z, lane = threadIdx.x, a = lane >> 3, b = lane & 7;
  const int q = quality[n];
  if (q < 1 || q > 100 || chroma420[n] == 0) return;  // the whole wave
  const size_t HW = (size_t)H * W;
  const int cy = min((int)blockIdx.y * 8 + a, H / 2 - 1), cx = min((int)blockIdx.x * 8 + b, W / 2 - 1);
  const float* src = in + (size_t)n * 3 * HW + (size_t)(2 * cy) * W + 2 * cx;
  int cb = 0, cr = 0;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int R = jpeg_level(src[i * W + j]), G = jpeg_level(src[HW + i * W + j]), B = jpeg_level(src[2 * HW + i * W + j]);
      cb += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
      cr += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
    }
  const int bias = 1 + (cx & 1);  // 1, 2, 1, 2, ... along a row
  float v[2] = {(float)(((cb + bias) >> 2) - 128), (float)(((cr + bias) >> 2) - 128)};
  const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
  const int cwb = gridDim.x, chb = gridDim.y;
  float* quot = quot_out ? quot_out + (size_t)n * 3 * HW + HW + (size_t)(blockIdx.y * cwb + blockIdx.x) * 64 : nullptr;
  jpeg_codec<2>(buf, v, lane, scale, 1, quot, HW);
  const size_t plane = (size_t)chb * cwb * 64;
  float* dst = ws + (size_t)n * 2 * plane + (size_t)(blockIdx.y * 8 + a) * (cwb * 8) + blockIdx.x * 8 + b;
  dst[0] = v[0], dst[plane] = v[1];
}

// The luma launch: one wave per 8 x 8 block of the image, lane = pixel.  A 4:4:4 sample takes jpeg_sim_kernel's path; a 4:2:0
// sample codes Y alone and takes its chroma from ws through libjpeg's h2v2_fancy_upsample in floating point: with c the
// sample over the pixel, v and h its vertical and horizontal neighbours on the pixel's side and d the diagonal one (the
// plane's edge sample beyond the H/2 x W/2 plane), fma(3, fma(3, c, v), fma(3, h, d)) / 16.  grid (W / 8, H / 8, N), 64 threads.
__global__ __launch_bounds__(64) void jpeg420_luma_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                          const int* __restrict__ quality, const int* __restrict__ chroma420,
                                                          const float* __restrict__ ws, float* __restrict__ quot_out, int H,
                                                          int W, int quantize) {
  __shared__ float buf[3][64];
  const int n = blockIdx.z, lane = threadIdx.x, a = lane >> 3, b = lane & 7;
  const size_t HW = (size_t)H * W;
  const int y = blockIdx.y * 8 + a, x = blockIdx.x * 8 + b;
  const size_t at = (size_t)n * 3 * HW + (size_t)y * W + x;
  const float fr = in[at], fg = in[at + HW], fb = in[at + 2 * HW];
  const int q = quality[n];
  if (q < 1 || q > 100) {  // not a JPEG quality: the sample passes through, bit for bit (the whole wave takes this branch)
    out[at] = fr, out[at + HW] = fg, out[at + 2 * HW] = fb;
    return;
  }
  const int R = jpeg_level(fr), G = jpeg_level(fg), B = jpeg_level(fb);
  const int scale = q < 50 ? 5000 / q : 200 - 2 * q;  // libjpeg's jpeg_quality_scaling
  float* quot = quot_out ? quot_out + (size_t)n * 3 * HW + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 64 : nullptr;
  float v[3];
  if (chroma420[n] == 0) {  // the whole wave
    v[0] = (float)(((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128);
    v[1] = (float)(((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16) - 128);
    v[2] = (float)(((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16) - 128);
    jpeg_codec<3>(buf, v, lane, scale, 0, quot, HW);
  } else {
    float luma[1] = {(float)(((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128)};
    jpeg_codec<1>(buf, luma, lane, scale, 0, quot, HW);
    v[0] = luma[0];
    const int pitch = jpeg420_blocks(W) * 8;
    const size_t plane = (size_t)jpeg420_blocks(H) * 8 * pitch;
    const int cy = y >> 1, cx = x >> 1;
    const int ny = min(max(cy + ((y & 1) ? 1 : -1), 0), H / 2 - 1), nx = min(max(cx + ((x & 1) ? 1 : -1), 0), W / 2 - 1);
    const float* cw = ws + (size_t)n * 2 * plane;
#pragma unroll
    for (int p = 0; p < 2; ++p, cw += plane) {
      const float c = cw[(size_t)cy * pitch + cx], vn = cw[(size_t)ny * pitch + cx], hn = cw[(size_t)cy * pitch + nx],
                  dn = cw[(size_t)ny * pitch + nx];
      v[1 + p] = fmaf(3.f, fmaf(3.f, c, vn), fmaf(3.f, hn, dn)) * 0.0625f;
    }
  }
  const float yy = v[0] + 128.f;
  float rgb[3] = {yy + 1.402f * v[2], yy - 0.344136286f * v[1] - 0.714136286f * v[2], yy + 1.772f * v[1]};
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    float o = fminf(fmaxf(rgb[p] * (1.0f / 255.0f), 0.f), 1.f);
    if (quantize) o = rintf(o * 255.f) * (1.0f / 255.0f);
    out[at + p * HW] = o;
  }
}

unsigned grid_for(int64_t n) {
  int64_t b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 65535 ? 65535 : b));
}

}  // namespace

extern "C" int srx_blur_aniso(const float* in_nchw, float* out_nchw, const float* parm, const int32_t* ksize, int N, int C,
                              int H, int W, void* stream) {
  SRX_REQUIRE(in_nchw && out_nchw && parm && ksize, "blur_aniso: null pointer");
  SRX_REQUIRE(in_nchw != out_nchw, "blur_aniso: the output must not be the input");
  SRX_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, "blur_aniso: bad shape");
  SRX_REQUIRE(C == 3, "blur_aniso: C = %d, the images have 3 channels", C);
  SRX_REQUIRE(H > 10 && W > 10, "blur_aniso: %d x %d planes: a 21-tap reflect needs 11 rows and columns", H, W);
  const int64_t tiles_x = srx_cdiv(W, kBlurTile), tiles = tiles_x * srx_cdiv(H, kBlurTile);
  SRX_REQUIRE(tiles <= 0x7fffffff && (int64_t)H * W <= 0x7fffffff, "blur_aniso: planes too large");
  hipLaunchKernelGGL(blur_aniso_kernel, dim3((unsigned)tiles, C, N), dim3(256), 0, srx_stream(stream), in_nchw, out_nchw,
                     parm, ksize, C, H, W, (int)tiles_x);
  SRX_CHECK_LAUNCH("blur_aniso_kernel");
  return SRX_OK;
}

extern "C" int srx_filter2d(const float* in_nchw, float* out_nchw, const float* weights, const int32_t* ksize, int N, int C,
                            int H, int W, int quantize, void* stream) {
  SRX_REQUIRE(in_nchw && out_nchw && weights && ksize, "filter2d: null pointer");
  SRX_REQUIRE(in_nchw != out_nchw, "filter2d: the output must not be the input");
  SRX_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, "filter2d: bad shape");
  SRX_REQUIRE(C == 3, "filter2d: C = %d, the images have 3 channels", C);
  SRX_REQUIRE(H > 10 && W > 10, "filter2d: %d x %d planes: a 21-tap reflect needs 11 rows and columns", H, W);
  const int64_t tiles_x = srx_cdiv(W, kBlurTile), tiles = tiles_x * srx_cdiv(H, kBlurTile);
  SRX_REQUIRE(tiles <= 0x7fffffff && (int64_t)H * W <= 0x7fffffff, "filter2d: planes too large");
  hipLaunchKernelGGL(filter2d_kernel, dim3((unsigned)tiles, C, N), dim3(256), 0, srx_stream(stream), in_nchw, out_nchw,
                     weights, ksize, C, H, W, (int)tiles_x, quantize);
  SRX_CHECK_LAUNCH("filter2d_kernel");
  return SRX_OK;
}

extern "C" int srx_add_gaussian_noise(const float* in_nchw, float* out_nchw, const float* sigma, const int32_t* gray,
                                      uint32_t seed_lo, uint32_t seed_hi, int N, int H, int W, int quantize, void* stream) {
  SRX_REQUIRE(in_nchw && out_nchw && sigma && gray, "add_gaussian_noise: null pointer");
  SRX_REQUIRE(N > 0 && H > 0 && W > 0, "add_gaussian_noise: bad shape");
  SRX_REQUIRE((int64_t)H * W <= 0x7fffffff, "add_gaussian_noise: planes too large");
  hipLaunchKernelGGL(add_gaussian_noise_kernel, dim3(grid_for((int64_t)N * H * W)), dim3(256), 0, srx_stream(stream),
                     in_nchw, out_nchw, sigma, gray, seed_lo, seed_hi, N, H * W, quantize);
  SRX_CHECK_LAUNCH("add_gaussian_noise_kernel");
  return SRX_OK;
}

extern "C" int srx_add_poisson_noise(const float* in_nchw, float* out_nchw, const float* scale, const int32_t* gray,
                                     const int32_t* tables, int32_t* levels, uint32_t seed_lo, uint32_t seed_hi, int N, int H,
                                     int W, int quantize, void* stream) {
  SRX_REQUIRE(in_nchw && out_nchw && scale && gray && tables && levels, "add_poisson_noise: null pointer");
  SRX_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, "add_poisson_noise: bad shape (N %d of 1..65535, %d x %d planes)", N, H, W);
  SRX_REQUIRE((int64_t)H * W <= 0x7fffffff, "add_poisson_noise: planes too large");
  hipStream_t st = srx_stream(stream);
  const int HW = H * W;
  if (hipMemsetAsync(levels, 0, (size_t)N * 8 * sizeof(int32_t), st) != hipSuccess)
    SRX_FAIL(SRX_E_HIP, "add_poisson_noise: memset failed");
  const int64_t per_sample = srx_cdiv(HW, 1024);  // four pixels per thread before a sample gets another workgroup
  hipLaunchKernelGGL(poisson_levels_kernel, dim3((unsigned)(per_sample > 64 ? 64 : per_sample), N), dim3(256), 0, st, in_nchw,
                     scale, gray, levels, HW);
  SRX_CHECK_LAUNCH("poisson_levels_kernel");
  hipLaunchKernelGGL(add_poisson_noise_kernel, dim3(grid_for((int64_t)N * HW)), dim3(256), 0, st, in_nchw, out_nchw, scale, gray,
                     tables, levels, seed_lo, seed_hi, N, HW, quantize);
  SRX_CHECK_LAUNCH("add_poisson_noise_kernel");
  return SRX_OK;
}

extern "C" int srx_jpeg_sim(const float* in_nchw, float* out_nchw, const int32_t* quality, int N, int H, int W,
                            int quantize, void* stream) {
  SRX_REQUIRE(in_nchw && out_nchw && quality, "jpeg_sim: null pointer");
  SRX_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, "jpeg_sim: bad shape");
  SRX_REQUIRE(H % 8 == 0 && W % 8 == 0, "jpeg_sim: %d x %d planes: whole 8 x 8 blocks only", H, W);
  SRX_REQUIRE(H / 8 <= 65535 && (int64_t)H * W <= 0x7fffffff, "jpeg_sim: planes too large");
  hipLaunchKernelGGL(jpeg_sim_kernel, dim3(W / 8, H / 8, N), dim3(64), 0, srx_stream(stream), in_nchw, out_nchw, quality, H,
                     W, quantize);
  SRX_CHECK_LAUNCH("jpeg_sim_kernel");
  return SRX_OK;
}

extern "C" size_t srx_jpeg_sim2_workspace(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * 2 * jpeg420_blocks(H) * 8 * jpeg420_blocks(W) * 8 * sizeof(float);
}

extern "C" int srx_jpeg_sim2(const float* in_nchw, float* out_nchw, const int32_t* quality, const int32_t* chroma420, int N,
                             int H, int W, int quantize, void* workspace, size_t workspace_bytes, float* quot_out,
                             void* stream) {
  SRX_REQUIRE(in_nchw && out_nchw && quality && chroma420 && workspace, "jpeg_sim2: null pointer");
  SRX_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, "jpeg_sim2: bad shape");
  SRX_REQUIRE(H % 8 == 0 && W % 8 == 0, "jpeg_sim2: %d x %d planes: whole 8 x 8 blocks only", H, W);
  SRX_REQUIRE(H / 8 <= 65535 && (int64_t)H * W <= 0x7fffffff, "jpeg_sim2: planes too large");
  const size_t need = srx_jpeg_sim2_workspace(N, H, W);
  SRX_REQUIRE(workspace_bytes >= need, "jpeg_sim2: workspace of %zu bytes, %zu needed (srx_jpeg_sim2_workspace)", workspace_bytes,
              need);
  hipStream_t st = srx_stream(stream);
  hipLaunchKernelGGL(jpeg420_chroma_kernel, dim3(jpeg420_blocks(W), jpeg420_blocks(H), N), dim3(64), 0, st, in_nchw, quality,
                     chroma420, (float*)workspace, quot_out, H, W);
  SRX_CHECK_LAUNCH("jpeg420_chroma_kernel");
  hipLaunchKernelGGL(jpeg420_luma_kernel, dim3(W / 8, H / 8, N), dim3(64), 0, st, in_nchw, out_nchw, quality, chroma420,
                     (const float*)workspace, quot_out, H, W, quantize);
  SRX_CHECK_LAUNCH("jpeg420_luma_kernel");
  return SRX_OK;
}
