// The compact generator's (SRVGGNetCompact) own kernels: per-channel PReLU on NHWC fp32, forward and backward, and the
// network's tail -- PixelShuffle(s) of the last conv's 3 s^2 channels plus the nearest-enlarged input image -- forward and
// backward.  All four move every byte once; none uses an atomic, so a call repeats its bits.
//
//   * PReLU: a lane owns one 16-byte quad of channels.  Forward: quads are walked with a grid stride, the quad's column is
//     advanced by (stride mod quads per row) instead of a division per element.  Backward: a workgroup owns a contiguous range
//     of rows and a lane keeps ONE quad column for all of them, so its four slope-gradient sums stay in registers (fp64: the
//     products x * dy are exact there and the sum's error is the final rounding); the lanes of a column are added in lane
//     order through LDS, the workgroup's C sums go to slot [workgroup][C] of the workspace, and a second launch adds the slots
//     in index order.  The number of workgroups depends on M alone.
//   * Tail: a workgroup stages the 3 s^2 values of 64 low-resolution pixels of one image row (and their input pixels) in LDS
//     and then writes the s output rows they cover; consecutive lanes write consecutive NHWC-4 pixels, 16 bytes each.  The
//     backward kernel is the same walk the other way round: 16-byte loads along the high-resolution rows, LDS, 16-byte stores
//     of whole channel quads of dt (channels past 3 s^2 as zeros).
#include "srx_common.h"
#include <algorithm>
#include <cstdint>

namespace {

constexpr int PC_MAX_C = 512;      // channels with a slope
constexpr int PC_MAX_CS = 1024;    // channel stride: a row's quads fit one 256-lane workgroup
constexpr int PC_MAX_BLOCKS = 1024;
constexpr int PC_ROWS = 64;        // rows per backward workgroup until PC_MAX_BLOCKS is reached

__global__ __launch_bounds__(256) void prelu_channels_fwd_kernel(const float* __restrict__ x, const float* __restrict__ slopes,
                                                                 float* __restrict__ y, int64_t total, int Q, int QC) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int sq = (int)(stride % Q);
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int q = (int)(i % Q);
  for (; i < total; i += stride) {
    f32x4 v = *reinterpret_cast<const f32x4*>(x + i * 4);
    if (q < QC) {  // (the channels between C and Cs pass through)
      const f32x4 a = *reinterpret_cast<const f32x4*>(slopes + q * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : a[e] * v[e];
    }
    *reinterpret_cast<f32x4*>(y + i * 4) = v;
    q += sq;
    q = q >= Q ? q - Q : q;
  }
}

// part[blockIdx.x][C]: this workgroup's sums over its rows [blockIdx.x * rows_per_block, ...)
__global__ __launch_bounds__(256) void prelu_channels_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                 const float* __restrict__ slopes, float* __restrict__ dx,
                                                                 double* __restrict__ part, int64_t M, int64_t rows_per_block,
                                                                 int Q, int QC) {
  __shared__ double red[256][4];
  const int rpb = 256 / Q;                       // rows one pass of the workgroup covers
  const int r = threadIdx.x / Q, q = threadIdx.x - r * Q;
  const int64_t row0 = (int64_t)blockIdx.x * rows_per_block, row1 = min(M, row0 + rows_per_block);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (r < rpb) {
    const bool real = q < QC;
    const f32x4 a = real ? *reinterpret_cast<const f32x4*>(slopes + q * 4) : f32x4{1.f, 1.f, 1.f, 1.f};
    for (int64_t row = row0 + r; row < row1; row += rpb) {
      const size_t at = ((size_t)row * Q + q) * 4;
      const f32x4 g = *reinterpret_cast<const f32x4*>(dy + at);
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + at);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool pos = v[e] > 0.f || !real;
        o[e] = pos ? g[e] : a[e] * g[e];
        acc[e] += pos ? 0.0 : (double)v[e] * (double)g[e];
      }
      *reinterpret_cast<f32x4*>(dx + at) = o;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[threadIdx.x][e] = acc[e];
  __syncthreads();
  if (threadIdx.x < QC) {  // row 0 of the lane grid: add the column's lanes in order
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double s = 0.0;
      for (int rr = 0; rr < rpb; ++rr) s += red[rr * Q + threadIdx.x][e];
      part[(size_t)blockIdx.x * (QC * 4) + threadIdx.x * 4 + e] = s;
    }
  }
}

__global__ __launch_bounds__(256) void prelu_channels_sum_kernel(const double* __restrict__ part, int nb, int C,
                                                                 float* __restrict__ dslopes, int accumulate) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += part[(size_t)b * C + c];
  dslopes[c] = (accumulate ? dslopes[c] : 0.f) + (float)s;
}

int pc_blocks(int64_t M) { return (int)std::min<int64_t>(srx_cdiv(M, PC_ROWS), PC_MAX_BLOCKS); }

// ---------------------------------------------------------------------------------------------------------------- tail
constexpr int TAIL_SEG = 64;  // low-resolution pixels per workgroup

template <typename T> struct Quad;
template <> struct Quad<float> {
  static __device__ __forceinline__ f32x4 load(const void* p) { return *reinterpret_cast<const f32x4*>(p); }
};
template <> struct Quad<__bf16> {
  static __device__ __forceinline__ f32x4 load(const void* p) {
    typedef __bf16 v4 __attribute__((ext_vector_type(4)));
    const v4 v = __builtin_bit_cast(v4, *reinterpret_cast<const uint2*>(p));
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
  }
};
template <> struct Quad<_Float16> {
  static __device__ __forceinline__ f32x4 load(const void* p) {
    typedef _Float16 v4 __attribute__((ext_vector_type(4)));
    const v4 v = __builtin_bit_cast(v4, *reinterpret_cast<const uint2*>(p));
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
  }
};

// LDS floats per staged pixel: >= 4 ceil(3 s^2 / 4), a multiple of 4 (16-byte rows) and = 4 mod 16, which spreads the pixels
// of a half wave over the banks (s = 4: conflict-free; s = 2, 3: two-way)
__host__ __device__ constexpr int tail_pitch(int s) { return 16 * s - 12; }

template <typename T, int S>
__global__ __launch_bounds__(256) void shuffle_add_nearest_fwd_kernel(const T* __restrict__ t, int t_cs, const float* __restrict__ x4,
                                                                      float* __restrict__ y4, int h, int w, int segs) {
  constexpr int K = 3 * S * S, NQ = (K + 3) / 4, PITCH = tail_pitch(S);
  __shared__ __attribute__((aligned(16))) float vals[TAIL_SEG * PITCH];
  __shared__ __attribute__((aligned(16))) float img[TAIL_SEG * 4];
  int b = blockIdx.x;
  const int seg = b % segs; b /= segs;
  const int yy = b % h, n = b / h;
  const int x0 = seg * TAIL_SEG, npix = min(TAIL_SEG, w - x0);
  const size_t lr_row = ((size_t)n * h + yy) * w + x0;  // first low-resolution pixel of the segment
  for (int e = threadIdx.x; e < npix * NQ; e += 256) {
    const int p = e / NQ, k = e - p * NQ;
    *reinterpret_cast<f32x4*>(vals + p * PITCH + 4 * k) = Quad<T>::load(t + (lr_row + p) * (size_t)t_cs + 4 * k);
  }
  if ((int)threadIdx.x < npix)
    *reinterpret_cast<f32x4*>(img + 4 * threadIdx.x) = *reinterpret_cast<const f32x4*>(x4 + (lr_row + threadIdx.x) * 4);
  __syncthreads();
  const int nout = npix * S;  // output pixels per output row of the segment
  for (int e = threadIdx.x; e < nout * S; e += 256) {
    const int i = e / nout, X = e - i * nout;
    const int p = X / S, j = X - p * S;
    const float* v = vals + p * PITCH + i * S + j;
    const f32x4 in = *reinterpret_cast<const f32x4*>(img + 4 * p);
    const f32x4 o = {v[0] + in[0], v[S * S] + in[1], v[2 * S * S] + in[2], 0.f};
    const size_t orow = ((size_t)n * h * S + (size_t)yy * S + i) * ((size_t)w * S) + (size_t)x0 * S;
    *reinterpret_cast<f32x4*>(y4 + (orow + X) * 4) = o;
  }
}

template <int S>
__global__ __launch_bounds__(256) void shuffle_add_nearest_bwd_kernel(const float* __restrict__ dy4, float* __restrict__ dt, int t_cs,
                                                                      int h, int w, int segs) {
  constexpr int K = 3 * S * S, PITCH = tail_pitch(S);
  __shared__ __attribute__((aligned(16))) float vals[TAIL_SEG * PITCH];
  int b = blockIdx.x;
  const int seg = b % segs; b /= segs;
  const int yy = b % h, n = b / h;
  const int x0 = seg * TAIL_SEG, npix = min(TAIL_SEG, w - x0);
  const size_t lr_row = ((size_t)n * h + yy) * w + x0;
  const int nout = npix * S;
  for (int e = threadIdx.x; e < nout * S; e += 256) {
    const int i = e / nout, X = e - i * nout;
    const int p = X / S, j = X - p * S;
    const size_t orow = ((size_t)n * h * S + (size_t)yy * S + i) * ((size_t)w * S) + (size_t)x0 * S;
    const f32x4 g = *reinterpret_cast<const f32x4*>(dy4 + (orow + X) * 4);
    float* v = vals + p * PITCH + i * S + j;
    v[0] = g[0]; v[S * S] = g[1]; v[2 * S * S] = g[2];
  }
  __syncthreads();
  const int tq = t_cs / 4;
  for (int e = threadIdx.x; e < npix * tq; e += 256) {
    const int p = e / tq, k = e - p * tq;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (4 * k < K) {
      o = *reinterpret_cast<const f32x4*>(vals + p * PITCH + 4 * k);
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = 4 * k + c < K ? o[c] : 0.f;
    }
    *reinterpret_cast<f32x4*>(dt + (lr_row + p) * (size_t)t_cs + 4 * k) = o;
  }
}

template <typename T>
int launch_tail_fwd(const void* t, int t_cs, const float* x4, float* y4, int N, int h, int w, int s, hipStream_t st) {
  const int segs = (int)srx_cdiv(w, TAIL_SEG);
  const dim3 grid((unsigned)((int64_t)N * h * segs));
  const T* tp = static_cast<const T*>(t);
  if (s == 2) hipLaunchKernelGGL((shuffle_add_nearest_fwd_kernel<T, 2>), grid, dim3(256), 0, st, tp, t_cs, x4, y4, h, w, segs);
  else if (s == 3) hipLaunchKernelGGL((shuffle_add_nearest_fwd_kernel<T, 3>), grid, dim3(256), 0, st, tp, t_cs, x4, y4, h, w, segs);
  else hipLaunchKernelGGL((shuffle_add_nearest_fwd_kernel<T, 4>), grid, dim3(256), 0, st, tp, t_cs, x4, y4, h, w, segs);
  SRX_CHECK_LAUNCH("shuffle_add_nearest_fwd_kernel");
  return SRX_OK;
}

int tail_check(const char* fn, int t_cs, int N, int h, int w, int s) {
  SRX_REQUIRE(s >= 2 && s <= 4, "%s: the scale must be 2, 3 or 4, got %d", fn, s);
  SRX_REQUIRE(N > 0 && h > 0 && w > 0, "%s: bad size", fn);
  SRX_REQUIRE(t_cs >= 3 * s * s && t_cs % 4 == 0, "%s: the channel stride %d must hold 3 s^2 = %d channels in whole quads", fn, t_cs, 3 * s * s);
  SRX_REQUIRE((int64_t)N * h * srx_cdiv(w, TAIL_SEG) < (1LL << 31), "%s: too many row segments for one launch", fn);
  return SRX_OK;
}

}  // namespace

extern "C" size_t srx_prelu_channels_ws_floats(int64_t M, int C) {
  return M > 0 && C > 0 ? (size_t)pc_blocks(M) * C * 2 : 0;  // fp64 slots
}

static bool pc_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int pc_check(const char* fn, int64_t M, int C, int Cs) {
  SRX_REQUIRE(M > 0 && C > 0, "%s: bad size", fn);
  SRX_REQUIRE(C % 4 == 0 && Cs % 4 == 0, "%s: C = %d and Cs = %d must be multiples of 4 (16-byte accesses)", fn, C, Cs);
  SRX_REQUIRE(C <= Cs, "%s: C = %d exceeds the channel stride %d", fn, C, Cs);
  SRX_REQUIRE(C <= PC_MAX_C && Cs <= PC_MAX_CS, "%s: at most %d channels with a stride of at most %d", fn, PC_MAX_C, PC_MAX_CS);
  return SRX_OK;
}

extern "C" int srx_prelu_channels_fwd(const float* x, const float* slopes, float* y, int64_t M, int C, int Cs, void* stream) {
  SRX_REQUIRE(x && slopes && y, "prelu_channels_fwd: null pointer");
  SRX_REQUIRE(pc_aligned(x) && pc_aligned(slopes) && pc_aligned(y), "prelu_channels_fwd: pointers must be 16-byte aligned");
  if (int rc = pc_check("prelu_channels_fwd", M, C, Cs)) return rc;
  const int Q = Cs / 4;
  const int64_t total = M * Q;
  const unsigned grid = (unsigned)std::min<int64_t>(srx_cdiv(total, 256), 8192);
  hipLaunchKernelGGL(prelu_channels_fwd_kernel, dim3(grid), dim3(256), 0, srx_stream(stream), x, slopes, y, total, Q, C / 4);
  SRX_CHECK_LAUNCH("prelu_channels_fwd_kernel");
  return SRX_OK;
}

extern "C" int srx_prelu_channels_bwd(const float* dy, const float* x, const float* slopes, float* dx, float* dslopes, int accumulate,
                                      int64_t M, int C, int Cs, float* ws, size_t ws_floats, void* stream) {
  SRX_REQUIRE(dy && x && slopes && dx && dslopes && ws, "prelu_channels_bwd: null pointer");
  SRX_REQUIRE(pc_aligned(dy) && pc_aligned(x) && pc_aligned(slopes) && pc_aligned(dx), "prelu_channels_bwd: pointers must be 16-byte aligned");
  if (int rc = pc_check("prelu_channels_bwd", M, C, Cs)) return rc;
  SRX_REQUIRE(ws_floats >= srx_prelu_channels_ws_floats(M, C), "prelu_channels_bwd: workspace of %zu floats, %zu needed", ws_floats,
              srx_prelu_channels_ws_floats(M, C));
  SRX_REQUIRE(((uintptr_t)ws & 7) == 0, "prelu_channels_bwd: the workspace must be 8-byte aligned");
  const int nb = pc_blocks(M);
  const int64_t rows_per_block = srx_cdiv(M, nb);
  hipStream_t st = srx_stream(stream);
  double* part = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(prelu_channels_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, st, dy, x, slopes, dx, part, M, rows_per_block, Cs / 4,
                     C / 4);
  SRX_CHECK_LAUNCH("prelu_channels_bwd_kernel");
  hipLaunchKernelGGL(prelu_channels_sum_kernel, dim3((unsigned)srx_cdiv(C, 256)), dim3(256), 0, st, part, nb, C, dslopes, accumulate);
  SRX_CHECK_LAUNCH("prelu_channels_sum_kernel");
  return SRX_OK;
}

extern "C" int srx_shuffle_add_nearest_fwd(const void* t, int t_dtype, int t_cs, const float* x4, float* y4, int N, int h, int w, int s,
                                           void* stream) {
  SRX_REQUIRE(t && x4 && y4, "shuffle_add_nearest_fwd: null pointer");
  SRX_REQUIRE(((uintptr_t)t & (t_dtype == 0 ? 15 : 7)) == 0 && ((uintptr_t)x4 & 15) == 0 && ((uintptr_t)y4 & 15) == 0,
              "shuffle_add_nearest_fwd: pointers must be 16-byte aligned (8 for a 16-bit t)");
  SRX_REQUIRE(t_dtype >= 0 && t_dtype <= 2, "shuffle_add_nearest_fwd: t_dtype must be 0 (fp32), 1 (bf16) or 2 (fp16), got %d", t_dtype);
  if (int rc = tail_check("shuffle_add_nearest_fwd", t_cs, N, h, w, s)) return rc;
  hipStream_t st = srx_stream(stream);
  if (t_dtype == 0) return launch_tail_fwd<float>(t, t_cs, x4, y4, N, h, w, s, st);
  if (t_dtype == 1) return launch_tail_fwd<__bf16>(t, t_cs, x4, y4, N, h, w, s, st);
  return launch_tail_fwd<_Float16>(t, t_cs, x4, y4, N, h, w, s, st);
}

extern "C" int srx_shuffle_add_nearest_bwd(const float* dy4, float* dt, int t_cs, int N, int h, int w, int s, void* stream) {
  SRX_REQUIRE(dy4 && dt, "shuffle_add_nearest_bwd: null pointer");
  SRX_REQUIRE(((uintptr_t)dy4 & 15) == 0 && ((uintptr_t)dt & 15) == 0, "shuffle_add_nearest_bwd: pointers must be 16-byte aligned");
  if (int rc = tail_check("shuffle_add_nearest_bwd", t_cs, N, h, w, s)) return rc;
  hipStream_t st = srx_stream(stream);
  const int segs = (int)srx_cdiv(w, TAIL_SEG);
  const dim3 grid((unsigned)((int64_t)N * h * segs));
  if (s == 2) hipLaunchKernelGGL(shuffle_add_nearest_bwd_kernel<2>, grid, dim3(256), 0, st, dy4, dt, t_cs, h, w, segs);
  else if (s == 3) hipLaunchKernelGGL(shuffle_add_nearest_bwd_kernel<3>, grid, dim3(256), 0, st, dy4, dt, t_cs, h, w, segs);
  else hipLaunchKernelGGL(shuffle_add_nearest_bwd_kernel<4>, grid, dim3(256), 0, st, dy4, dt, t_cs, h, w, segs);
  SRX_CHECK_LAUNCH("shuffle_add_nearest_bwd_kernel");
  return SRX_OK;
}
