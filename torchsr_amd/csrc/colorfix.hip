// Colour correction of a super-resolved frame against its low-resolution input (test.upscale(color_fix=), `torchsr test
// --color-fix`): the wavelet and the AdaIN "colour fix" of StableSR on [planes][H][W] fp32, every plane alone.
//
// wavelet: out = sr + B(U - sr), U the enlarged input and B the product of `levels` a-trous blurs with [1 2 1]^T [1 2 1] / 16 at
// the radii r = 1, 2, 4, ... and replicate padding.  One launch per level (srx_color_fix_wavelet_level), both passes in it:
//   t[y][x]   = 0.25f * (D[y][cl(x - r)] + D[y][cl(x + r)]) + 0.5f * D[y][x]          (along W)
//   dst[y][x] = 0.25f * (t[cl(y - r)][x] + t[cl(y + r)][x]) + 0.5f * t[y][x]          (along H)
// with D = src - sub where sub is given (the first level: U - sr) and dst = add + ... where add is given (the last: sr + D).
// The products by 0.25 and 0.5 are exact, so every pass is two roundings whether or not an fma is formed, and t has the values
// a separate W pass would have stored: the bits are those of ten passes through memory.
//  - A work item walks the rows y, y + r, y + 2 r, ... of one residue class: the t of row y + r is the `next` of output row y,
//    the `centre` of y + r and the `previous` of y + 2 r, so it is computed ONCE and kept in registers -- three row reads per
//    output row instead of nine, and every row of D is read by one workgroup (two at the ends of a segment of SEG rows),
//    wherever the hardware places the others: HBM sees one read and one write of the planes per level.
//  - Lanes along x.  16 bytes per lane when W % 4 == 0, every base is 16-byte aligned and r is 1, 2 or a multiple of 4 (the
//    +-r neighbours are then whole quads, or two elements of the adjacent quad): three 16-byte loads per row, the neighbours'
//    out of L1.  Scalar otherwise: the same expression per element, the same bits.
// adain: out = fmaf(sr, s, b) per plane, s = sqrt(var_lr + 1e-5) / sqrt(var_sr + 1e-5), b = mean_lr - mean_sr * s in fp64, each
// rounded once to fp32.  srx_plane_moments: mean and unbiased variance in fp64 from sums of d = x - x[0] and d^2 (exact
// differences: a constant plane has variance exactly 0), per-workgroup partials in fixed slots, reduced in index order by one
// wave per plane -- no atomics, an element's place in the sum depends on the plane's size alone: the same bits from every call,
// every batch and every alignment.
// Work items are a linear index walked with a grid-stride loop, every plane base 64-bit; one plane stays below 2^31 elements.
#include "srx_common.h"

namespace {

constexpr int SEG = 16;          // output rows a work item of the level kernel walks (+ 2 rows read at its ends)
constexpr int MAX_RADIUS = 32768;
constexpr int MOM_QUADS = 8;     // quads per thread a moments workgroup is sized for ...
constexpr int MOM_MAX_BLOCKS = 512;  // ... up to this many workgroups per plane
constexpr int APPLY_MAX_BLOCKS = 512;

__device__ __forceinline__ f32x4 splat(float v) { return f32x4{v, v, v, v}; }

template <bool FIRST>
__device__ __forceinline__ float ld1(const float* __restrict__ a, const float* __restrict__ b, int64_t i) {
  return FIRST ? a[i] - b[i] : a[i];
}
template <bool FIRST>
__device__ __forceinline__ f32x4 ld4(const float* __restrict__ a, const float* __restrict__ b, int64_t i) {
  const f32x4 v = *reinterpret_cast<const f32x4*>(a + i);
  return FIRST ? v - *reinterpret_cast<const f32x4*>(b + i) : v;
}

// t of one row at lane position q (an element, or a quad): row = element offset of the row's start
template <bool FIRST>
__device__ __forceinline__ float hpass(const float* __restrict__ a, const float* __restrict__ b, int64_t row, int q, int W, int r, float) {
  const float c = ld1<FIRST>(a, b, row + q);
  const float l = ld1<FIRST>(a, b, row + max(q - r, 0)), rt = ld1<FIRST>(a, b, row + min(q + r, W - 1));
  return 0.25f * (l + rt) + 0.5f * c;
}
template <bool FIRST>
__device__ __forceinline__ f32x4 hpass(const float* __restrict__ a, const float* __restrict__ b, int64_t row, int q, int W, int r, f32x4) {
  const int W4 = W >> 2, k = r < 4 ? 1 : r >> 2;  // r is 1, 2 or a multiple of 4 (the host's condition for this form)
  const f32x4 c = ld4<FIRST>(a, b, row + 4 * (int64_t)q);
  f32x4 L = ld4<FIRST>(a, b, row + 4 * (int64_t)max(q - k, 0)), R = ld4<FIRST>(a, b, row + 4 * (int64_t)min(q + k, W4 - 1));
  if (q < k) L = splat(L[0]);            // quad 0 was loaded: everything left of the row is its first element
  if (q + k >= W4) R = splat(R[3]);      // quad W4 - 1: its last
  f32x4 l = L, rt = R;
  if (r == 1) {
    l = f32x4{L[3], c[0], c[1], c[2]};
    rt = f32x4{c[1], c[2], c[3], R[0]};
  } else if (r == 2) {
    l = f32x4{L[2], L[3], c[0], c[1]};
    rt = f32x4{c[2], c[3], R[0], R[1]};
  }
  return 0.25f * (l + rt) + 0.5f * c;
}

// V = float: lanes are elements; V = f32x4: quads.  Work item = (plane, residue class of y mod r, segment of SEG rows of the
// class, 256-lane chunk of a row).
template <typename V, bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void atrous_level_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           const float* __restrict__ add, float* __restrict__ dst, int64_t planes,
                                                           int H, int W, int r) {
  constexpr int E = sizeof(V) / sizeof(float);
  const int Wv = W / E, cpr = (Wv + 255) / 256;
  const int classes = min(r, H);
  const int spc = ((H + r - 1) / r + SEG - 1) / SEG;  // segments of the longest class (class 0)
  const int64_t items = planes * classes * spc * cpr, step = (int64_t)SEG * r;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t g = it / cpr;
    const int q = (int)(it - g * cpr) * 256 + (int)threadIdx.x;
    if (q >= Wv) continue;
    const int64_t g2 = g / spc, p = g2 / classes;
    const int64_t y0 = (g2 - p * classes) + (g - g2 * spc) * step;
    if (y0 >= H) continue;  // a shorter class
    const int64_t y1 = min((int64_t)H, y0 + step), base = p * H * W;
    V tp = hpass<FIRST>(a, b, base + max(y0 - r, (int64_t)0) * W, q, W, r, V{});
    V tc = hpass<FIRST>(a, b, base + y0 * W, q, W, r, V{});
#pragma unroll 2
    for (int64_t y = y0; y < y1; y += r) {
      const V tn = hpass<FIRST>(a, b, base + min(y + r, (int64_t)H - 1) * W, q, W, r, V{});
      V o = 0.25f * (tp + tn) + 0.5f * tc;
      const int64_t at = base + y * W + (int64_t)E * q;
      if (LAST) o = *reinterpret_cast<const V*>(add + at) + o;
      *reinterpret_cast<V*>(dst + at) = o;
      tp = tc;
      tc = tn;
    }
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// part[(p * B + blk) * 2 + {0, 1}] = sums of d and d^2, d = x - x[p][0], over the quads [blk * qpb, (blk + 1) * qpb) of plane p:
// thread t takes the quads blk * qpb + t, + 256, ... and adds their elements in ascending order.  VEC: one 16-byte load per quad
// (n % 4 == 0, 16-byte aligned base); the sums are formed in the same order either way.
template <bool VEC>
__global__ __launch_bounds__(256) void moments_partial_kernel(const float* __restrict__ x, int64_t planes, int64_t n, int B,
                                                              double* __restrict__ part) {
  __shared__ double red[4][2];
  const int tid = (int)threadIdx.x;
  const int64_t nq = (n + 3) / 4, qpb = (nq + B - 1) / B, items = planes * B;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t p = it / B, blk = it - p * B;
    const float* xp = x + p * n;
    const double K = (double)xp[0];
    const int64_t q1 = min(nq, (blk + 1) * qpb);
    double s1 = 0.0, s2 = 0.0;
    for (int64_t q = blk * qpb + tid; q < q1; q += 256) {
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      const int cnt = (int)min((int64_t)4, n - 4 * q);
      if (VEC) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(xp + 4 * q);
        v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < cnt) v[e] = xp[4 * q + e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) {
          const double d = (double)v[e] - K;
          s1 += d;
          s2 = __fma_rn(d, d, s2);
        }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if ((tid & 63) == 0) red[tid >> 6][0] = s1, red[tid >> 6][1] = s2;
    __syncthreads();
    if (tid == 0) {
      part[it * 2] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
      part[it * 2 + 1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    }
    __syncthreads();  // the next item overwrites red
  }
}

// one wave per plane: lane l adds the partials l, l + 64, ... in order, then the xor tree.  stats[p] = {mean, unbiased variance}
__global__ __launch_bounds__(64) void moments_final_kernel(const float* __restrict__ x, int64_t planes, int64_t n, int B,
                                                           const double* __restrict__ part, double* __restrict__ stats) {
  for (int64_t p = blockIdx.x; p < planes; p += gridDim.x) {
    double s1 = 0.0, s2 = 0.0;
    for (int i = (int)threadIdx.x; i < B; i += 64) {
      s1 += part[(p * B + i) * 2];
      s2 += part[(p * B + i) * 2 + 1];
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (threadIdx.x == 0) {
      const double dn = (double)n;
      stats[p * 2] = (double)x[p * n] + s1 / dn;
      stats[p * 2 + 1] = n > 1 ? fmax((s2 - s1 * s1 / dn) / (dn - 1.0), 0.0) : 0.0;
    }
  }
}

// Work item = (plane, workgroup g of G): the 256-quad chunks g, g + G, ... of the plane, behind one evaluation of (s, b)
template <bool VEC>
__global__ __launch_bounds__(256) void adain_apply_kernel(const float* __restrict__ sr, float* __restrict__ dst, int64_t planes,
                                                          int64_t n, int G, const double* __restrict__ st_sr,
                                                          const double* __restrict__ st_lr) {
  const int64_t nq = (n + 3) / 4, items = planes * G;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t p = it / G, g = it - p * G;
    const double s64 = sqrt(st_lr[p * 2 + 1] + 1e-5) / sqrt(st_sr[p * 2 + 1] + 1e-5);
    const double b64 = st_lr[p * 2] - st_sr[p * 2] * s64;
    const float s = (float)s64, b = (float)b64;
    const float* sp = sr + p * n;
    float* dp = dst + p * n;
    for (int64_t q = g * 256 + (int64_t)threadIdx.x; q < nq; q += (int64_t)G * 256) {
      if (VEC) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(sp + 4 * q);
        *reinterpret_cast<f32x4*>(dp + 4 * q) =
            f32x4{__fmaf_rn(v[0], s, b), __fmaf_rn(v[1], s, b), __fmaf_rn(v[2], s, b), __fmaf_rn(v[3], s, b)};
      } else {
        const int cnt = (int)min((int64_t)4, n - 4 * q);
        for (int e = 0; e < cnt; ++e) dp[4 * q + e] = __fmaf_rn(sp[4 * q + e], s, b);
      }
    }
  }
}

unsigned item_grid(int64_t items) {
  const int64_t cap = 16384;  // 256 CUs x 8 workgroups x 8 rounds, as dihedral.hip
  return (unsigned)(items < cap ? items : cap);
}

bool apart(uintptr_t a, uintptr_t a_bytes, uintptr_t b, uintptr_t b_bytes) { return a + a_bytes <= b || b + b_bytes <= a; }

int moments_blocks(int64_t n) {
  const int64_t b = srx_cdiv(srx_cdiv(n, 4), 256 * MOM_QUADS);
  return (int)(b < MOM_MAX_BLOCKS ? b : MOM_MAX_BLOCKS);
}

template <typename V>
void launch_level(bool first, bool last, unsigned grid, hipStream_t st, const float* a, const float* b, const float* add, float* dst,
                  int64_t planes, int H, int W, int r) {
  if (first && last)
    hipLaunchKernelGGL((atrous_level_kernel<V, true, true>), dim3(grid), dim3(256), 0, st, a, b, add, dst, planes, H, W, r);
  else if (first)
    hipLaunchKernelGGL((atrous_level_kernel<V, true, false>), dim3(grid), dim3(256), 0, st, a, b, add, dst, planes, H, W, r);
  else if (last)
    hipLaunchKernelGGL((atrous_level_kernel<V, false, true>), dim3(grid), dim3(256), 0, st, a, b, add, dst, planes, H, W, r);
  else
    hipLaunchKernelGGL((atrous_level_kernel<V, false, false>), dim3(grid), dim3(256), 0, st, a, b, add, dst, planes, H, W, r);
}

bool plane_sizes_ok(const char* who, int64_t planes, int H, int W) {
  if (!(planes > 0 && H > 0 && W > 0)) {
    srx_set_error("%s: planes, H and W must be positive (got %lld, %d, %d)", who, (long long)planes, H, W);
    return false;
  }
  if ((int64_t)H * W >= ((int64_t)1 << 31)) {
    srx_set_error("%s: a plane must stay below 2^31 elements (H * W = %lld)", who, (long long)((int64_t)H * W));
    return false;
  }
  if (planes >= ((int64_t)1 << 28)) {  // x 2^31 x 4 bytes < 2^61
    srx_set_error("%s: planes = %lld passes 2^28", who, (long long)planes);
    return false;
  }
  return true;
}

}  // namespace

extern "C" int srx_color_fix_wavelet_level(const float* src, const float* sub, const float* add, float* dst, int64_t planes, int H,
                                           int W, int radius, void* stream) {
  SRX_REQUIRE(src && dst, "color_fix_wavelet_level: null pointer (src %p, dst %p)", (const void*)src, (void*)dst);
  if (!plane_sizes_ok("color_fix_wavelet_level", planes, H, W)) return SRX_E_BADARG;
  SRX_REQUIRE(radius >= 1 && radius <= MAX_RADIUS, "color_fix_wavelet_level: radius must be in 1..%d (got %d)", MAX_RADIUS, radius);
  const uintptr_t s0 = (uintptr_t)src, b0 = (uintptr_t)sub, a0 = (uintptr_t)add, d0 = (uintptr_t)dst;
  SRX_REQUIRE(s0 % 4 == 0 && b0 % 4 == 0 && a0 % 4 == 0 && d0 % 4 == 0,
              "color_fix_wavelet_level: src, sub, add and dst must be 4-byte aligned");
  const uintptr_t bytes = (uintptr_t)planes * H * W * 4;
  SRX_REQUIRE(apart(d0, bytes, s0, bytes) && (!sub || apart(d0, bytes, b0, bytes)) && (!add || apart(d0, bytes, a0, bytes)),
              "color_fix_wavelet_level: dst overlaps an operand (dst %p, src %p, sub %p, add %p, %zu bytes each): a level reads "
              "neighbours, in place is not possible",
              (void*)dst, (const void*)src, (const void*)sub, (const void*)add, (size_t)bytes);
  hipStream_t st = srx_stream(stream);
  const int64_t groups = planes * (radius < H ? radius : H) * srx_cdiv(srx_cdiv(H, radius), SEG);
  const bool quads = W % 4 == 0 && s0 % 16 == 0 && b0 % 16 == 0 && a0 % 16 == 0 && d0 % 16 == 0 && (radius <= 2 || radius % 4 == 0);
  if (quads)
    launch_level<f32x4>(sub != nullptr, add != nullptr, item_grid(groups * srx_cdiv(W / 4, 256)), st, src, sub, add, dst, planes, H, W,
                        radius);
  else
    launch_level<float>(sub != nullptr, add != nullptr, item_grid(groups * srx_cdiv(W, 256)), st, src, sub, add, dst, planes, H, W,
                        radius);
  SRX_CHECK_LAUNCH("atrous_level_kernel");
  return SRX_OK;
}

extern "C" int srx_plane_moments_blocks(int H, int W) {
  if (H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31)) return 0;
  return moments_blocks((int64_t)H * W);
}

extern "C" int srx_plane_moments(const float* x, int64_t planes, int H, int W, double* part, size_t part_doubles, double* stats,
                                 void* stream) {
  SRX_REQUIRE(x && part && stats, "plane_moments: null pointer (x %p, part %p, stats %p)", (const void*)x, (void*)part, (void*)stats);
  if (!plane_sizes_ok("plane_moments", planes, H, W)) return SRX_E_BADARG;
  const int64_t n = (int64_t)H * W;
  const int B = moments_blocks(n);
  const uintptr_t x0 = (uintptr_t)x, p0 = (uintptr_t)part, t0 = (uintptr_t)stats;
  SRX_REQUIRE(x0 % 4 == 0 && p0 % 8 == 0 && t0 % 8 == 0, "plane_moments: x must be 4-byte, part and stats 8-byte aligned");
  const uint64_t need = (uint64_t)planes * B * 2;
  SRX_REQUIRE(part_doubles >= need, "plane_moments: the workspace holds %zu doubles, [planes][%d][2] needs %llu", part_doubles, B,
              (unsigned long long)need);
  const uintptr_t xb = (uintptr_t)planes * n * 4, pb = (uintptr_t)need * 8, tb = (uintptr_t)planes * 16;
  SRX_REQUIRE(apart(x0, xb, p0, pb) && apart(x0, xb, t0, tb) && apart(p0, pb, t0, tb),
              "plane_moments: x, part and stats overlap (x %p + %zu, part %p + %zu, stats %p + %zu bytes)", (const void*)x, (size_t)xb,
              (void*)part, (size_t)pb, (void*)stats, (size_t)tb);
  hipStream_t st = srx_stream(stream);
  if (n % 4 == 0 && x0 % 16 == 0)
    hipLaunchKernelGGL(moments_partial_kernel<true>, dim3(item_grid(planes * B)), dim3(256), 0, st, x, planes, n, B, part);
  else
    hipLaunchKernelGGL(moments_partial_kernel<false>, dim3(item_grid(planes * B)), dim3(256), 0, st, x, planes, n, B, part);
  SRX_CHECK_LAUNCH("moments_partial_kernel");
  hipLaunchKernelGGL(moments_final_kernel, dim3(item_grid(planes)), dim3(64), 0, st, x, planes, n, B, part, stats);
  SRX_CHECK_LAUNCH("moments_final_kernel");
  return SRX_OK;
}

extern "C" int srx_color_fix_adain_apply(const float* sr, float* dst, int64_t planes, int H, int W, const double* stats_sr,
                                         const double* stats_lr, void* stream) {
  SRX_REQUIRE(sr && dst && stats_sr && stats_lr, "color_fix_adain_apply: null pointer (sr %p, dst %p, stats_sr %p, stats_lr %p)",
              (const void*)sr, (void*)dst, (const void*)stats_sr, (const void*)stats_lr);
  if (!plane_sizes_ok("color_fix_adain_apply", planes, H, W)) return SRX_E_BADARG;
  const int64_t n = (int64_t)H * W;
  const uintptr_t s0 = (uintptr_t)sr, d0 = (uintptr_t)dst, m0 = (uintptr_t)stats_sr, l0 = (uintptr_t)stats_lr;
  SRX_REQUIRE(s0 % 4 == 0 && d0 % 4 == 0 && m0 % 8 == 0 && l0 % 8 == 0,
              "color_fix_adain_apply: sr and dst must be 4-byte, the statistics 8-byte aligned");
  const uintptr_t bytes = (uintptr_t)planes * n * 4, tb = (uintptr_t)planes * 16;
  SRX_REQUIRE(apart(s0, bytes, d0, bytes) && apart(d0, bytes, m0, tb) && apart(d0, bytes, l0, tb),
              "color_fix_adain_apply: dst overlaps an operand (dst %p, sr %p, stats_sr %p, stats_lr %p)", (void*)dst, (const void*)sr,
              (const void*)stats_sr, (const void*)stats_lr);
  hipStream_t st = srx_stream(stream);
  const int64_t chunks = srx_cdiv(srx_cdiv(n, 4), 256);
  const int G = (int)(chunks < APPLY_MAX_BLOCKS ? chunks : APPLY_MAX_BLOCKS);
  if (n % 4 == 0 && s0 % 16 == 0 && d0 % 16 == 0)
    hipLaunchKernelGGL(adain_apply_kernel<true>, dim3(item_grid(planes * G)), dim3(256), 0, st, sr, dst, planes, n, G, stats_sr, stats_lr);
  else
    hipLaunchKernelGGL(adain_apply_kernel<false>, dim3(item_grid(planes * G)), dim3(256), 0, st, sr, dst, planes, n, G, stats_sr,
                       stats_lr);
  SRX_CHECK_LAUNCH("adain_apply_kernel");
  return SRX_OK;
}
