// Spectral normalisation of a conv weight (torch.nn.utils.spectral_norm, one power iteration, eps = 1e-12) for the U-Net
// discriminator.  W is [rows = Cout][cols = Cin * KH * KW] fp32; the passes are HBM-bound streams over W (17 MB for the eight
// layers of the network), so the training forward reads W three times and writes it once:
//   1. W^T u          column sums over row chunks, one partial row per chunk   (read 1)
//   2. v              the partials added in chunk order, normalised            (one workgroup)
//   3. s = W v        one wave per row                                         (read 2)
//   4. u, sigma, W/s  every workgroup forms u = s / |s| and sigma = u . s from the R values of s on its own -- the same
//                     operations in the same order, so the same bits -- and scales its share of W   (read 3, write 1)
// No floating-point atomics anywhere: grids, chunking and reduction trees are fixed functions of (rows, cols), so two calls on
// the same inputs write the same bits (the training step is captured in a hipGraph and compared bitwise with the eager one).
#include "srx_common.h"

namespace {

constexpr int SN_THREADS = 256;
constexpr int SN_WAVES = SN_THREADS / 64;
constexpr int SN_MAX_CHUNKS = 32;  // row chunks of pass 1
constexpr int SN_DOT_BLOCKS = 256; // partial sums of the backward's <G, W_sn>

int sn_chunks(int rows) { return (int)(srx_cdiv(rows, 16) < SN_MAX_CHUNKS ? srx_cdiv(rows, 16) : SN_MAX_CHUNKS); }

// sum over the workgroup in a fixed tree: xor-shuffles inside each wave, then the wave sums added in wave order by everyone
__device__ __forceinline__ float block_sum(float v, float* lds) {
  v = srx_wave_sum(v);
  __syncthreads();  // (lds may still be read from the previous call)
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < SN_WAVES; ++w) s += lds[w];
  return s;
}

// pass 1: part[chunk][k] = sum over the chunk's rows of W[r][k] * u[r]; a thread owns four columns
__global__ __launch_bounds__(128) void sn_wtu_kernel(const float* __restrict__ W, const float* __restrict__ u,
                                                     float* __restrict__ part, int rows, int cols, int rows_per_chunk) {
  const int q = blockIdx.x * 128 + threadIdx.x;
  if (q * 4 >= cols) return;
  const int r0 = blockIdx.y * rows_per_chunk;
  const int r1 = r0 + rows_per_chunk < rows ? r0 + rows_per_chunk : rows;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int r = r0; r < r1; ++r) acc += *reinterpret_cast<const f32x4*>(W + (size_t)r * cols + q * 4) * u[r];
  *reinterpret_cast<f32x4*>(part + (size_t)blockIdx.y * cols + q * 4) = acc;
}

// pass 2 (one workgroup): t = sum of the partials in chunk order; v = t / max(|t|, eps), also kept in v_keep
__global__ __launch_bounds__(SN_THREADS) void sn_v_kernel(const float* __restrict__ part, int chunks, int cols, float eps,
                                                          float* __restrict__ v, float* __restrict__ v_keep) {
  __shared__ float lds[SN_WAVES];
  float sq = 0.f;
  for (int q = threadIdx.x; q * 4 < cols; q += SN_THREADS) {
    f32x4 t = *reinterpret_cast<const f32x4*>(part + q * 4);
    for (int c = 1; c < chunks; ++c) t += *reinterpret_cast<const f32x4*>(part + (size_t)c * cols + q * 4);
    *reinterpret_cast<f32x4*>(v + q * 4) = t;
    sq += t.x * t.x + t.y * t.y + t.z * t.z + t.w * t.w;
  }
  const float d = fmaxf(sqrtf(block_sum(sq, lds)), eps);
  for (int q = threadIdx.x; q * 4 < cols; q += SN_THREADS) {  // (each thread: the quads it wrote itself)
    f32x4 t = *reinterpret_cast<const f32x4*>(v + q * 4);
    t.x /= d; t.y /= d; t.z /= d; t.w /= d;
    *reinterpret_cast<f32x4*>(v + q * 4) = t;
    if (v_keep) *reinterpret_cast<f32x4*>(v_keep + q * 4) = t;
  }
}

// pass 3: s[r] = W[r] . v, one wave per row
__global__ __launch_bounds__(SN_THREADS) void sn_wv_kernel(const float* __restrict__ W, const float* __restrict__ v,
                                                           float* __restrict__ s, int rows, int cols) {
  const int r = blockIdx.x * SN_WAVES + (threadIdx.x >> 6);
  if (r >= rows) return;  // (whole waves leave: no shuffle below misses a lane)
  const float* w = W + (size_t)r * cols;
  float acc = 0.f;
  for (int q = threadIdx.x & 63; q * 4 < cols; q += 64) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(w + q * 4), b = *reinterpret_cast<const f32x4*>(v + q * 4);
    acc += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
  }
  acc = srx_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s[r] = acc;
}

// pass 4: sigma from s (train: u = s / max(|s|, eps) first; eval: the stored u), then W_sn = W / sigma.  Every workgroup
// computes sigma itself; workgroup 0 publishes u, u_keep and sigma.
__global__ __launch_bounds__(SN_THREADS) void sn_scale_kernel(const float* __restrict__ W, const float* __restrict__ s,
                                                              float* __restrict__ u, float* __restrict__ u_keep,
                                                              float* __restrict__ sigma, float* __restrict__ Wsn, int rows,
                                                              int64_t quads, int train, float eps) {
  __shared__ float lds[SN_WAVES];
  float d = 1.f;
  if (train) {
    float sq = 0.f;
    for (int r = threadIdx.x; r < rows; r += SN_THREADS) sq += s[r] * s[r];
    d = fmaxf(sqrtf(block_sum(sq, lds)), eps);
  }
  float dot = 0.f;
  for (int r = threadIdx.x; r < rows; r += SN_THREADS) {
    const float sr = s[r], ur = train ? sr / d : u[r];
    dot += ur * sr;
    if (blockIdx.x == 0) {
      if (train) u[r] = ur;
      if (u_keep) u_keep[r] = ur;
    }
  }
  const float sg = block_sum(dot, lds);
  if (blockIdx.x == 0 && threadIdx.x == 0) *sigma = sg;
  for (int64_t q = (int64_t)blockIdx.x * SN_THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * SN_THREADS) {
    f32x4 w = *reinterpret_cast<const f32x4*>(W + q * 4);
    w.x /= sg; w.y /= sg; w.z /= sg; w.w /= sg;
    *reinterpret_cast<f32x4*>(Wsn + q * 4) = w;
  }
}

// backward, pass 1: part[b] = sum over the workgroup's quads of G * (W / sigma)
__global__ __launch_bounds__(SN_THREADS) void sn_dot_kernel(const float* __restrict__ G, const float* __restrict__ W,
                                                            const float* __restrict__ sigma, float* __restrict__ part,
                                                            int64_t quads) {
  __shared__ float lds[SN_WAVES];
  const float sg = *sigma;
  float acc = 0.f;
  for (int64_t q = (int64_t)blockIdx.x * SN_THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * SN_THREADS) {
    const f32x4 g = *reinterpret_cast<const f32x4*>(G + q * 4), w = *reinterpret_cast<const f32x4*>(W + q * 4);
    acc += g.x * (w.x / sg) + g.y * (w.y / sg) + g.z * (w.z / sg) + g.w * (w.w / sg);
  }
  acc = block_sum(acc, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// backward, pass 2: c = sum of the (<= 256) partials in the workgroup's fixed tree (every workgroup on its own, the same bits);
// dW (+)= (G - c u v^T) / sigma
__global__ __launch_bounds__(SN_THREADS) void sn_bwd_kernel(const float* __restrict__ G, const float* __restrict__ u,
                                                            const float* __restrict__ v, const float* __restrict__ sigma,
                                                            const float* __restrict__ part, int nparts, float* __restrict__ dW,
                                                            int accumulate, int cols, int64_t quads) {
  __shared__ float lds[SN_WAVES];
  static_assert(SN_DOT_BLOCKS <= SN_THREADS, "one partial per thread");
  const float c = block_sum((int)threadIdx.x < nparts ? part[threadIdx.x] : 0.f, lds), sg = *sigma;
  const int cq = cols / 4;
  for (int64_t q = (int64_t)blockIdx.x * SN_THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * SN_THREADS) {
    const int r = (int)(q / cq), k = (int)(q - (int64_t)r * cq) * 4;
    const f32x4 g = *reinterpret_cast<const f32x4*>(G + q * 4), vv = *reinterpret_cast<const f32x4*>(v + k);
    const float cu = c * u[r];
    f32x4 o;
    o.x = (g.x - cu * vv.x) / sg; o.y = (g.y - cu * vv.y) / sg; o.z = (g.z - cu * vv.z) / sg; o.w = (g.w - cu * vv.w) / sg;
    if (accumulate) o += *reinterpret_cast<const f32x4*>(dW + q * 4);
    *reinterpret_cast<f32x4*>(dW + q * 4) = o;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

unsigned stream_blocks(int64_t quads) {
  int64_t b = srx_cdiv(quads, SN_THREADS);
  return (unsigned)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

int check_shape(int rows, int cols, const char* who) {
  SRX_REQUIRE(rows > 0 && cols > 0 && cols % 4 == 0, "%s: rows and cols must be positive and cols a multiple of 4", who);
  SRX_REQUIRE((int64_t)rows * cols < (1LL << 31), "%s: rows * cols must stay below 2^31", who);
  return SRX_OK;
}

}  // namespace

extern "C" size_t srx_spectral_norm_ws_floats(int rows, int cols) {
  if (rows <= 0 || cols <= 0) return 0;
  const size_t fwd = (size_t)sn_chunks(rows) * (size_t)srx_roundup(cols, 4) + (size_t)srx_roundup(rows, 4);
  return fwd > SN_DOT_BLOCKS ? fwd : SN_DOT_BLOCKS;
}

extern "C" int srx_spectral_norm_fwd(const float* W, float* u, float* v, float* W_sn, float* sigma, float* uv_keep, int rows,
                                     int cols, int train, float* ws, size_t ws_floats, void* stream) {
  if (int rc = check_shape(rows, cols, "spectral_norm_fwd")) return rc;
  SRX_REQUIRE(W && u && v && W_sn && sigma && ws, "spectral_norm_fwd: null pointer");
  SRX_REQUIRE(aligned16(W) && aligned16(v) && aligned16(W_sn) && aligned16(ws) && aligned4(u) && aligned4(sigma) &&
                  (!uv_keep || aligned16(uv_keep)),
              "spectral_norm_fwd: W, v, W_sn, ws and uv_keep must be 16-byte aligned, u and sigma 4-byte");
  SRX_REQUIRE(W != W_sn, "spectral_norm_fwd: W_sn must not be W");
  SRX_REQUIRE(ws_floats >= srx_spectral_norm_ws_floats(rows, cols), "spectral_norm_fwd: workspace too small (%zu < %zu floats)",
              ws_floats, srx_spectral_norm_ws_floats(rows, cols));
  hipStream_t st = srx_stream(stream);
  const float eps = 1e-12f;
  const int chunks = sn_chunks(rows), rpc = (int)srx_cdiv(rows, chunks);
  float* part = ws;
  float* s = ws + (size_t)chunks * cols;
  // uv_keep: [roundup(rows, 4)] u then [cols] v of THIS forward, for the backward (u and v themselves move on with the next call)
  float* u_keep = uv_keep;
  float* v_keep = uv_keep ? uv_keep + srx_roundup(rows, 4) : nullptr;
  const float* vsrc = v;
  if (train) {
    hipLaunchKernelGGL(sn_wtu_kernel, dim3((unsigned)srx_cdiv(cols / 4, 128), (unsigned)srx_cdiv(rows, rpc)), dim3(128), 0, st, W, u,
                       part, rows, cols, rpc);
    SRX_CHECK_LAUNCH("sn_wtu_kernel");
    hipLaunchKernelGGL(sn_v_kernel, dim3(1), dim3(SN_THREADS), 0, st, part, (int)srx_cdiv(rows, rpc), cols, eps, v, v_keep);
    SRX_CHECK_LAUNCH("sn_v_kernel");
  } else if (v_keep) {
    if (hipMemcpyAsync(v_keep, v, (size_t)cols * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
      SRX_FAIL(SRX_E_HIP, "spectral_norm_fwd: copy of v failed");
  }
  hipLaunchKernelGGL(sn_wv_kernel, dim3((unsigned)srx_cdiv(rows, SN_WAVES)), dim3(SN_THREADS), 0, st, W, vsrc, s, rows, cols);
  SRX_CHECK_LAUNCH("sn_wv_kernel");
  const int64_t quads = (int64_t)rows * cols / 4;
  hipLaunchKernelGGL(sn_scale_kernel, dim3(stream_blocks(quads)), dim3(SN_THREADS), 0, st, W, s, u, u_keep, sigma, W_sn, rows,
                     quads, train ? 1 : 0, eps);
  SRX_CHECK_LAUNCH("sn_scale_kernel");
  return SRX_OK;
}

extern "C" int srx_spectral_norm_bwd(const float* G, const float* W, const float* u, const float* v, const float* sigma,
                                     float* dW, int accumulate, int rows, int cols, float* ws, size_t ws_floats, void* stream) {
  if (int rc = check_shape(rows, cols, "spectral_norm_bwd")) return rc;
  SRX_REQUIRE(G && W && u && v && sigma && dW && ws, "spectral_norm_bwd: null pointer");
  SRX_REQUIRE(aligned16(G) && aligned16(W) && aligned16(v) && aligned16(dW) && aligned4(u) && aligned4(sigma) && aligned4(ws),
              "spectral_norm_bwd: G, W, v and dW must be 16-byte aligned, u, sigma and ws 4-byte");
  SRX_REQUIRE(ws_floats >= srx_spectral_norm_ws_floats(rows, cols), "spectral_norm_bwd: workspace too small (%zu < %zu floats)",
              ws_floats, srx_spectral_norm_ws_floats(rows, cols));
  hipStream_t st = srx_stream(stream);
  const int64_t quads = (int64_t)rows * cols / 4;
  int64_t nb = srx_cdiv(quads, SN_THREADS * 4);
  if (nb > SN_DOT_BLOCKS) nb = SN_DOT_BLOCKS;
  if (nb < 1) nb = 1;
  hipLaunchKernelGGL(sn_dot_kernel, dim3((unsigned)nb), dim3(SN_THREADS), 0, st, G, W, sigma, ws, quads);
  SRX_CHECK_LAUNCH("sn_dot_kernel");
  hipLaunchKernelGGL(sn_bwd_kernel, dim3(stream_blocks(quads)), dim3(SN_THREADS), 0, st, G, u, v, sigma, ws, (int)nb, dW,
                     accumulate ? 1 : 0, cols, quads);
  SRX_CHECK_LAUNCH("sn_bwd_kernel");
  return SRX_OK;
}
