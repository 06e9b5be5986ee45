// Streaming kernels of the multi-layer perceptual loss (Real-ESRGAN / BasicSR PerceptualLoss: five VGG19 layers before their ReLU,
// ImageNet-normalised inputs, weighted L1).  The convs are the frozen stack's own; this file is the memory-bound work around the
// taps: the input normalisation that also builds the [source; target] batch, the pool that applies the tap's ReLU (ReLU and max
// commute) and sums |fs - ft| over the values it has loaded anyway, and the pool backward that adds the tap's L1 gradient.
// 16-byte accesses, grid-stride loops over fixed grids, wave reduction + LDS tree, fp64 one-workgroup finalise: no atomics,
// every result is a fixed function of the arguments.
#include "srx_common.h"

namespace {

enum { TAP_MAX_BLOCKS = 1024 };

unsigned stream_grid(int64_t n) {
  int64_t b = srx_cdiv(n, 256);
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (unsigned)b;
}
unsigned tap_grid(int64_t items) {
  int64_t b = srx_cdiv(items, 256);
  if (b > TAP_MAX_BLOCKS) b = TAP_MAX_BLOCKS;
  if (b < 1) b = 1;
  return (unsigned)b;
}

#define GRID_STRIDE(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint2 pack_bf16x4(const f32x4& v) {
  const bf16x2_t lo = {(__bf16)v[0], (__bf16)v[1]}, hi = {(__bf16)v[2], (__bf16)v[3]};
  return make_uint2(__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi));
}
__device__ __forceinline__ f32x4 unpack_bf16x4(const uint2 u) {
  return (f32x4){__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xffff0000u),
                 __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xffff0000u)};
}
__device__ __forceinline__ void store4(void* p, int64_t at, const f32x4& v, bool bf16) {
  if (bf16) *reinterpret_cast<uint2*>(static_cast<unsigned short*>(p) + at) = pack_bf16x4(v);
  else *reinterpret_cast<f32x4*>(static_cast<float*>(p) + at) = v;
}
__device__ __forceinline__ float sign_of(float t) { return t > 0.f ? 1.f : (t < 0.f ? -1.f : 0.f); }

struct Vec3 { float v[3]; };

// ---------------------------------------------------------------- input normalisation
// pix: pixels of one image batch (N * H * W); pixel i < pix comes from src, the rest from tgt
__global__ void normalize_pair_kernel(const float* __restrict__ src, const float* __restrict__ tgt, float* __restrict__ out,
                                      int64_t pix, int64_t total, Vec3 mean, Vec3 inv_std) {
  GRID_STRIDE(i, total) {
    const f32x4 v = i < pix ? *reinterpret_cast<const f32x4*>(src + i * 4) : *reinterpret_cast<const f32x4*>(tgt + (i - pix) * 4);
    f32x4 r;
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = (float)(((double)v[c] - (double)mean.v[c]) * (double)inv_std.v[c]);
    r[3] = 0.f;
    *reinterpret_cast<f32x4*>(out + i * 4) = r;
  }
}

__global__ void normalize_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dsrc, int64_t pix, Vec3 inv_std) {
  GRID_STRIDE(i, pix) {
    const f32x4 g = *reinterpret_cast<const f32x4*>(dout + i * 4);
    const f32x4 r = {g[0] * inv_std.v[0], g[1] * inv_std.v[1], g[2] * inv_std.v[2], 0.f};
    *reinterpret_cast<f32x4*>(dsrc + i * 4) = r;
  }
}

// ---------------------------------------------------------------- reductions
// the workgroup's sum of `acc` into partial[blockIdx.x]: wave butterfly, then the four wave sums in a fixed order
__device__ __forceinline__ void block_partial(float acc, float* __restrict__ partial) {
  __shared__ float red[4];
  acc = srx_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void tap_finalize_kernel(const float* __restrict__ partial, int nb, double scale,
                                                           float* __restrict__ loss, int accumulate) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) s += (double)partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float t = (float)(red[0] * scale);
    loss[0] = accumulate ? loss[0] + t : t;
  }
}

__global__ __launch_bounds__(256) void tap_l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                             float* __restrict__ partial, int64_t n4) {
  float acc = 0.f;
  GRID_STRIDE(i, n4) {
    const f32x4 u = *reinterpret_cast<const f32x4*>(a + i * 4);
    const f32x4 v = *reinterpret_cast<const f32x4*>(b + i * 4);
    acc += (fabsf(u[0] - v[0]) + fabsf(u[1] - v[1])) + (fabsf(u[2] - v[2]) + fabsf(u[3] - v[3]));
  }
  block_partial(acc, partial);
}

// ---------------------------------------------------------------- pool + ReLU forward at a tap
struct Window { f32x4 a, b, c, d; };
__device__ __forceinline__ Window load_window(const float* __restrict__ x, int64_t base, int W, int C) {
  Window w;
  w.a = *reinterpret_cast<const f32x4*>(x + base);
  w.b = *reinterpret_cast<const f32x4*>(x + base + C);
  w.c = *reinterpret_cast<const f32x4*>(x + base + (int64_t)W * C);
  w.d = *reinterpret_cast<const f32x4*>(x + base + (int64_t)W * C + C);
  return w;
}
__device__ __forceinline__ f32x4 pool_relu(const Window& w) {
  f32x4 m;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float t = fmaxf(fmaxf(w.a[e], w.b[e]), fmaxf(w.c[e], w.d[e]));
    m[e] = t > 0.f ? t : 0.f;
  }
  return m;
}
// item i of [N][Ho][Wo][C / 4] -> the float offset of its window's first entry in [N][H][W][C]
__device__ __forceinline__ int64_t window_base(int64_t i, int H, int W, int C) {
  const int Ho = H / 2, Wo = W / 2, cq = C / 4;
  const int q = (int)(i % cq);
  int64_t t = i / cq;
  const int ow = (int)(t % Wo);
  t /= Wo;
  const int oh = (int)(t % Ho);
  const int64_t n = t / Ho;
  return ((n * H + 2 * oh) * W + 2 * ow) * C + q * 4;
}

// PAIR: items run over the SOURCE samples; the thread also takes the same window of sample n + N_src and sums |difference|
template <bool PAIR>
__global__ __launch_bounds__(256) void pool_relu_fwd_tap_kernel(const float* __restrict__ x, void* __restrict__ y, int y_bf16,
                                                                int64_t items, int H, int W, int C, float* __restrict__ partial) {
  const int64_t half_in = items * 16, half_out = items * 4;  // floats of the source half: items * 4 window entries * 4 channels
  float acc = 0.f;
  GRID_STRIDE(i, items) {
    const int64_t base = window_base(i, H, W, C);
    const Window s = load_window(x, base, W, C);
    store4(y, i * 4, pool_relu(s), y_bf16);
    if (PAIR) {
      const Window t = load_window(x, base + half_in, W, C);
      store4(y, i * 4 + half_out, pool_relu(t), y_bf16);
      float p = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        p += (fabsf(s.a[e] - t.a[e]) + fabsf(s.b[e] - t.b[e])) + (fabsf(s.c[e] - t.c[e]) + fabsf(s.d[e] - t.d[e]));
      acc += p;
    }
  }
  if (PAIR) block_partial(acc, partial);
}

// ---------------------------------------------------------------- pool + ReLU backward plus the tap's L1 gradient
__global__ __launch_bounds__(256) void pool_relu_bwd_tap_kernel(const void* __restrict__ dy, int dy_bf16,
                                                                const float* __restrict__ xs, const float* __restrict__ xt,
                                                                void* __restrict__ dx, int dx_bf16, float coef,
                                                                const float* __restrict__ gscale, int64_t items, int H, int W, int C) {
  const float cg = coef * gscale[0];
  GRID_STRIDE(i, items) {
    const int64_t base = window_base(i, H, W, C);
    const Window s = load_window(xs, base, W, C), t = load_window(xt, base, W, C);
    const f32x4 g = dy_bf16 ? unpack_bf16x4(*reinterpret_cast<const uint2*>(static_cast<const unsigned short*>(dy) + i * 4))
                            : *reinterpret_cast<const f32x4*>(static_cast<const float*>(dy) + i * 4);
    f32x4 ga, gb, gc, gd;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // first maximum in scan order, nothing through a window whose maximum is not positive (maxpool_bwd_kernel<true>)
      int idx = 0;
      float m = s.a[e];
      if (s.b[e] > m) { m = s.b[e]; idx = 1; }
      if (s.c[e] > m) { m = s.c[e]; idx = 2; }
      if (s.d[e] > m) { m = s.d[e]; idx = 3; }
      if (!(m > 0.f)) idx = -1;
      ga[e] = (idx == 0 ? g[e] : 0.f) + cg * sign_of(s.a[e] - t.a[e]);
      gb[e] = (idx == 1 ? g[e] : 0.f) + cg * sign_of(s.b[e] - t.b[e]);
      gc[e] = (idx == 2 ? g[e] : 0.f) + cg * sign_of(s.c[e] - t.c[e]);
      gd[e] = (idx == 3 ? g[e] : 0.f) + cg * sign_of(s.d[e] - t.d[e]);
    }
    store4(dx, base, ga, dx_bf16);
    store4(dx, base + C, gb, dx_bf16);
    store4(dx, base + (int64_t)W * C, gc, dx_bf16);
    store4(dx, base + (int64_t)W * C + C, gd, dx_bf16);
  }
}

__global__ void tap_l1_bwd_top_kernel(const float* __restrict__ fs, const float* __restrict__ ft, void* __restrict__ g, int g_bf16,
                                      float coef, const float* __restrict__ gscale, int64_t n4) {
  const float cg = coef * gscale[0];
  GRID_STRIDE(i, n4) {
    const f32x4 u = *reinterpret_cast<const f32x4*>(fs + i * 4);
    const f32x4 v = *reinterpret_cast<const f32x4*>(ft + i * 4);
    const f32x4 r = {cg * sign_of(u[0] - v[0]), cg * sign_of(u[1] - v[1]), cg * sign_of(u[2] - v[2]), cg * sign_of(u[3] - v[3])};
    store4(g, i * 4, r, g_bf16);
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace

extern "C" int srx_normalize_pair_nhwc4(const float* src, const float* tgt, float* out, int N, int H, int W, const float mean[3],
                                        const float inv_std[3], void* stream) {
  SRX_REQUIRE(src && out && mean && inv_std && N > 0 && H > 0 && W > 0, "normalize_pair_nhwc4: bad argument");
  SRX_REQUIRE(aligned16(src) && aligned16(tgt) && aligned16(out), "normalize_pair_nhwc4: tensors must be 16-byte aligned");
  const int64_t pix = (int64_t)N * H * W, total = tgt ? 2 * pix : pix;
  Vec3 m, s;
  for (int c = 0; c < 3; ++c) { m.v[c] = mean[c]; s.v[c] = inv_std[c]; }
  hipLaunchKernelGGL(normalize_pair_kernel, dim3(stream_grid(total)), dim3(256), 0, srx_stream(stream), src, tgt, out, pix, total, m, s);
  SRX_CHECK_LAUNCH("normalize_pair_kernel");
  return SRX_OK;
}

extern "C" int srx_normalize_nhwc4_bwd(const float* dout, float* dsrc, int N, int H, int W, const float inv_std[3], void* stream) {
  SRX_REQUIRE(dout && dsrc && inv_std && N > 0 && H > 0 && W > 0, "normalize_nhwc4_bwd: bad argument");
  SRX_REQUIRE(aligned16(dout) && aligned16(dsrc), "normalize_nhwc4_bwd: tensors must be 16-byte aligned");
  const int64_t pix = (int64_t)N * H * W;
  Vec3 s;
  for (int c = 0; c < 3; ++c) s.v[c] = inv_std[c];
  hipLaunchKernelGGL(normalize_bwd_kernel, dim3(stream_grid(pix)), dim3(256), 0, srx_stream(stream), dout, dsrc, pix, s);
  SRX_CHECK_LAUNCH("normalize_bwd_kernel");
  return SRX_OK;
}

extern "C" int srx_tap_blocks(int N_src, int H, int W, int C) {
  if (N_src <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
  return (int)tap_grid((int64_t)N_src * (H / 2) * (W / 2) * (C / 4));
}

extern "C" int srx_maxpool2x2_relu_fwd_tap(const float* x, void* y, int y_is_bf16, int N_src, int N_tot, int H, int W, int C,
                                           float* partial, void* stream) {
  SRX_REQUIRE(x && y && N_src > 0 && H > 0 && W > 0 && C > 0, "maxpool2x2_relu_fwd_tap: bad argument");
  SRX_REQUIRE(H % 2 == 0 && W % 2 == 0 && C % 4 == 0, "maxpool2x2_relu_fwd_tap: H, W must be even and C a multiple of 4");
  SRX_REQUIRE(N_tot == N_src || N_tot == 2 * N_src, "maxpool2x2_relu_fwd_tap: N_tot must be N_src or 2 * N_src");
  SRX_REQUIRE(!partial || N_tot == 2 * N_src, "maxpool2x2_relu_fwd_tap: partial sums need the [source; target] batch");
  SRX_REQUIRE(aligned16(x) && ((uintptr_t)y % 8) == 0 && (y_is_bf16 || aligned16(y)), "maxpool2x2_relu_fwd_tap: misaligned tensor");
  hipStream_t st = srx_stream(stream);
  if (partial) {
    const int64_t items = (int64_t)N_src * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(pool_relu_fwd_tap_kernel<true>, dim3(tap_grid(items)), dim3(256), 0, st, x, y, y_is_bf16, items, H, W, C,
                       partial);
  } else {
    const int64_t items = (int64_t)N_tot * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(pool_relu_fwd_tap_kernel<false>, dim3(stream_grid(items)), dim3(256), 0, st, x, y, y_is_bf16, items, H, W, C,
                       (float*)nullptr);
  }
  SRX_CHECK_LAUNCH("pool_relu_fwd_tap_kernel");
  return SRX_OK;
}

extern "C" int srx_tap_l1_finalize(const float* partial, int n_partial, double scale, float* loss, int accumulate, void* stream) {
  SRX_REQUIRE(partial && loss && n_partial > 0 && n_partial <= TAP_MAX_BLOCKS, "tap_l1_finalize: bad argument");
  hipLaunchKernelGGL(tap_finalize_kernel, dim3(1), dim3(256), 0, srx_stream(stream), partial, n_partial, scale, loss, accumulate);
  SRX_CHECK_LAUNCH("tap_finalize_kernel");
  return SRX_OK;
}

extern "C" int srx_tap_l1_fwd(const float* a, const float* b, int64_t n, double weight, float* loss, int accumulate, float* ws,
                              void* stream) {
  SRX_REQUIRE(a && b && loss && ws && n > 0 && n % 4 == 0, "tap_l1_fwd: bad argument");
  SRX_REQUIRE(aligned16(a) && aligned16(b), "tap_l1_fwd: tensors must be 16-byte aligned");
  const unsigned nb = tap_grid(n / 4);
  hipStream_t st = srx_stream(stream);
  hipLaunchKernelGGL(tap_l1_partial_kernel, dim3(nb), dim3(256), 0, st, a, b, ws, n / 4);
  SRX_CHECK_LAUNCH("tap_l1_partial_kernel");
  hipLaunchKernelGGL(tap_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, (int)nb, weight / (double)n, loss, accumulate);
  SRX_CHECK_LAUNCH("tap_finalize_kernel");
  return SRX_OK;
}

extern "C" int srx_maxpool2x2_relu_bwd_tap(const void* dy, int dy_is_bf16, const float* x_src, const float* x_tgt, void* dx,
                                           int dx_is_bf16, float coef, const float* gscale, int N_src, int H, int W, int C,
                                           void* stream) {
  SRX_REQUIRE(dy && x_src && x_tgt && dx && gscale && N_src > 0 && H > 0 && W > 0 && C > 0, "maxpool2x2_relu_bwd_tap: bad argument");
  SRX_REQUIRE(H % 2 == 0 && W % 2 == 0 && C % 4 == 0, "maxpool2x2_relu_bwd_tap: H, W must be even and C a multiple of 4");
  SRX_REQUIRE(aligned16(x_src) && aligned16(x_tgt) && ((uintptr_t)dy % 8) == 0 && ((uintptr_t)dx % 8) == 0 &&
                  (dy_is_bf16 || aligned16(dy)) && (dx_is_bf16 || aligned16(dx)),
              "maxpool2x2_relu_bwd_tap: misaligned tensor");
  const int64_t items = (int64_t)N_src * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL(pool_relu_bwd_tap_kernel, dim3(stream_grid(items)), dim3(256), 0, srx_stream(stream), dy, dy_is_bf16, x_src, x_tgt,
                     dx, dx_is_bf16, coef, gscale, items, H, W, C);
  SRX_CHECK_LAUNCH("pool_relu_bwd_tap_kernel");
  return SRX_OK;
}

extern "C" int srx_tap_l1_bwd_top(const float* fs, const float* ft, void* g, int g_is_bf16, float coef, const float* gscale, int64_t n,
                                  void* stream) {
  SRX_REQUIRE(fs && ft && g && gscale && n > 0 && n % 4 == 0, "tap_l1_bwd_top: bad argument");
  SRX_REQUIRE(aligned16(fs) && aligned16(ft) && ((uintptr_t)g % 8) == 0 && (g_is_bf16 || aligned16(g)), "tap_l1_bwd_top: misaligned tensor");
  hipLaunchKernelGGL(tap_l1_bwd_top_kernel, dim3(stream_grid(n / 4)), dim3(256), 0, srx_stream(stream), fs, ft, g, g_is_bf16, coef,
                     gscale, n / 4);
  SRX_CHECK_LAUNCH("tap_l1_bwd_top_kernel");
  return SRX_OK;
}
