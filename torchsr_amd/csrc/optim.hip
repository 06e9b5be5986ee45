// torch.optim.Adam (lr 1e-4, betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad) as the
// reference configures it three times (srgan/trainer.py:171-185), run over ONE flat parameter
// buffer per model: a single HBM-bound streaming pass (p, g, m, v read; p, m, v written) instead
// of ~150 per-tensor launches.  The step counter and the learning rate live on the device so a
// captured hipGraph of the train step stays valid across steps and StepLR updates.
//
// The gradient guard (srx_grad_guard + srx_adam_step_guarded) stands where the reference has torch.cuda.amp.GradScaler
// (srgan/trainer.py:196,382-388): one more streaming read of g decides ON THE DEVICE whether the step is skipped (a non-finite
// gradient) and by how much the gradient is scaled down (torch.nn.utils.clip_grad_norm_); the guarded Adam reads that decision
// from device memory, so the pair replays from the step's graph with no host code in between.
#include "srx_common.h"
#include <math.h>

namespace {

__global__ void adam_tick_kernel(int64_t* step) { *step += 1; }

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                   const float* __restrict__ lr_ptr, float beta1, float beta2,
                                                   float eps, float gscale, const int64_t* __restrict__ step_ptr) {
  // same operation order as torch/optim/adam.py (_single_tensor_adam):
  //   m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g
  //   step_size = lr/(1-b1^t) ; denom = sqrt(v)/sqrt(1-b2^t) + eps ; p -= step_size * m/denom
  const double t = (double)(*step_ptr);
  const float bc1 = (float)(1.0 - pow((double)beta1, t));
  const float bc2 = (float)(1.0 - pow((double)beta2, t));
  const float step_size = lr_ptr[0] / bc1;
  const float bc2_sqrt = sqrtf(bc2);
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    f32x4 pv = *reinterpret_cast<const f32x4*>(p + i * 4);
    f32x4 gv = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 mv = *reinterpret_cast<const f32x4*>(m + i * 4);
    f32x4 vv = *reinterpret_cast<const f32x4*>(v + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gg = gv[e] * gscale;
      mv[e] = beta1 * mv[e] + (1.f - beta1) * gg;
      vv[e] = beta2 * vv[e] + (1.f - beta2) * gg * gg;
      const float denom = sqrtf(vv[e]) / bc2_sqrt + eps;
      pv[e] -= step_size * (mv[e] / denom);
    }
    *reinterpret_cast<f32x4*>(p + i * 4) = pv;
    *reinterpret_cast<f32x4*>(m + i * 4) = mv;
    *reinterpret_cast<f32x4*>(v + i * 4) = vv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t i = n4 * 4 + threadIdx.x;
    const float gg = g[i] * gscale;
    const float mm = beta1 * m[i] + (1.f - beta1) * gg;
    const float vv = beta2 * v[i] + (1.f - beta2) * gg * gg;
    m[i] = mm;
    v[i] = vv;
    p[i] -= step_size * (mm / (sqrtf(vv) / bc2_sqrt + eps));
  }
}

// ---- gradient guard ------------------------------------------------------------------------------------------------------
// sum of g[i]^2 in fp64 from the first element on: an fp32 square is exact in fp64 and 2^31 of them cannot overflow, so the sum is
// finite exactly when every g[i] is -- one pass gives the norm AND the non-finite test.  Fixed order everywhere (no floating-
// point atomics): a thread adds its grid-stride quads in order, lanes combine in a butterfly, the four waves in index order, and
// the workgroup's partial goes to ws[blockIdx.x]; guard_finalize_kernel combines those in a fixed tree of its own.
__device__ __forceinline__ double guard_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void guard_sumsq_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ part) {
  __shared__ double red[4];
  const int64_t n4 = n / 4;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double x = (double)gv[e];
      acc += x * x;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const double x = (double)g[n4 * 4 + threadIdx.x];
    acc += x * x;
  }
  acc = guard_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one workgroup: thread t adds the partials [t * per, (t + 1) * per) in index order, then lanes and waves as above
__global__ __launch_bounds__(256) void guard_finalize_kernel(const double* __restrict__ part, int parts, float grad_scale,
                                                             float max_norm, int skip_nonfinite, srx_grad_guard_t* state) {
  __shared__ double red[4];
  const int per = (parts + 255) / 256;
  double acc = 0.0;
  for (int k = 0; k < per; ++k) {
    const int i = (int)threadIdx.x * per + k;
    if (i < parts) acc += part[i];
  }
  acc = guard_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double sum = ((red[0] + red[1]) + red[2]) + red[3];
  const double norm64 = fabs((double)grad_scale) * sqrt(sum);
  const bool nonfinite = !isfinite(sum);
  const int skip = (nonfinite && skip_nonfinite) ? 1 : 0;
  // torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False): clamp(max_norm / (total_norm + 1e-6), max=1); a NaN stays a NaN
  double coef = 1.0;
  if (isfinite(max_norm) && max_norm > 0.f) {
    coef = (double)max_norm / (norm64 + 1e-6);
    if (coef > 1.0) coef = 1.0;
  }
  const float scale = skip ? 0.f : (float)coef;
  state->scale = scale;
  state->skip = skip;
  state->norm = (float)norm64;
  state->skipped += skip;
  state->clipped += scale < 1.f ? 1 : 0;
}

// adam_tick_kernel / adam_kernel behind the guard's decision.  Kernels of their own: the unguarded pair above stays as it is,
// instruction for instruction.  With state->scale == 1 the multiplier is grad_scale exactly and the results are adam_kernel's.
__global__ void adam_tick_guarded_kernel(int64_t* step, const srx_grad_guard_t* __restrict__ state) {
  if (!state->skip) *step += 1;
}

__global__ __launch_bounds__(256) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                           const float* __restrict__ lr_ptr, float beta1, float beta2,
                                                           float eps, float grad_scale, const int64_t* __restrict__ step_ptr,
                                                           const srx_grad_guard_t* __restrict__ state) {
  if (state->skip) return;  // uniform over the grid: p, m, v stay as they are
  const float gscale = grad_scale * state->scale;
  const double t = (double)(*step_ptr);
  const float bc1 = (float)(1.0 - pow((double)beta1, t));
  const float bc2 = (float)(1.0 - pow((double)beta2, t));
  const float step_size = lr_ptr[0] / bc1;
  const float bc2_sqrt = sqrtf(bc2);
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    f32x4 pv = *reinterpret_cast<const f32x4*>(p + i * 4);
    f32x4 gv = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 mv = *reinterpret_cast<const f32x4*>(m + i * 4);
    f32x4 vv = *reinterpret_cast<const f32x4*>(v + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gg = gv[e] * gscale;
      mv[e] = beta1 * mv[e] + (1.f - beta1) * gg;
      vv[e] = beta2 * vv[e] + (1.f - beta2) * gg * gg;
      const float denom = sqrtf(vv[e]) / bc2_sqrt + eps;
      pv[e] -= step_size * (mv[e] / denom);
    }
    *reinterpret_cast<f32x4*>(p + i * 4) = pv;
    *reinterpret_cast<f32x4*>(m + i * 4) = mv;
    *reinterpret_cast<f32x4*>(v + i * 4) = vv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t i = n4 * 4 + threadIdx.x;
    const float gg = g[i] * gscale;
    const float mm = beta1 * m[i] + (1.f - beta1) * gg;
    const float vv = beta2 * v[i] + (1.f - beta2) * gg * gg;
    m[i] = mm;
    v[i] = vv;
    p[i] -= step_size * (mm / (sqrtf(vv) / bc2_sqrt + eps));
  }
}

// workgroups of the guard's and the guarded Adam's streaming passes over n floats: a fixed function of n that mirrors the grid
// srx_adam_step computes for itself below (that entry point is left as it was, so it keeps its own three lines)
inline int64_t stream_blocks(int64_t n) {
  int64_t blocks = srx_cdiv(n / 4, 256);
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  return blocks;
}

// ---- generator weight average ---------------------------------------------------------------------------------------------
// ema = d * ema + (1 - d) * p over a flat parameter buffer, in place on ema (srx_axpby's pointers are __restrict__: it may not
// run in place).  Two products and one sum, each rounded once -- the intrinsics keep the compiler from contracting them into an
// fma, so the bits are a function of the operands alone.  Three streams of 4n bytes; shaped like axpby_kernel.
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, int64_t n,
                                                         float d, float omd) {
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    f32x4 ev = *reinterpret_cast<const f32x4*>(ema + i * 4);
    const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) ev[e] = __fadd_rn(__fmul_rn(d, ev[e]), __fmul_rn(omd, pv[e]));
    *reinterpret_cast<f32x4*>(ema + i * 4) = ev;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t i = n4 * 4 + threadIdx.x;
    ema[i] = __fadd_rn(__fmul_rn(d, ema[i]), __fmul_rn(omd, p[i]));
  }
}

}  // namespace

extern "C" int srx_ema_update(float* ema, const float* p, int64_t n, float decay, float one_minus_decay, void* stream) {
  SRX_REQUIRE(ema && p && n > 0, "ema_update: bad argument (null pointer or n <= 0)");
  SRX_REQUIRE(((uintptr_t)ema % 16 == 0) && ((uintptr_t)p % 16 == 0), "ema_update: buffers must be 16-byte aligned");
  SRX_REQUIRE((const float*)ema != p, "ema_update: ema and p are the same buffer (the average is a buffer of its own)");
  SRX_REQUIRE(isfinite(decay) && decay >= 0.f && decay < 1.f, "ema_update: decay must be in [0, 1), got %g", (double)decay);
  SRX_REQUIRE(isfinite(one_minus_decay) && one_minus_decay > 0.f && one_minus_decay <= 1.f,
              "ema_update: one_minus_decay must be in (0, 1], got %g", (double)one_minus_decay);
  hipStream_t st = srx_stream(stream);
  SRX_LAUNCH_PROF("ema_update_kernel", 0.0, ema_update_kernel, dim3((unsigned)stream_blocks(n)), dim3(256), 0, st, ema, p, n,
                  decay, one_minus_decay);
  SRX_CHECK_LAUNCH("ema_update_kernel");
  return SRX_OK;
}

extern "C" int srx_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* lr, float beta1,
                             float beta2, float eps, float grad_scale, int64_t* step, void* stream) {
  SRX_REQUIRE(p && g && m && v && lr && step && n > 0, "adam_step: bad argument");
  SRX_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)m % 16 == 0) &&
                  ((uintptr_t)v % 16 == 0),
              "adam_step: buffers must be 16-byte aligned");
  hipStream_t st = srx_stream(stream);
  hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, st, step);
  SRX_CHECK_LAUNCH("adam_tick_kernel");
  int64_t blocks = srx_cdiv(n / 4, 256);
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p, g, m, v, n, lr, beta1, beta2, eps,
                     grad_scale, step);
  SRX_CHECK_LAUNCH("adam_kernel");
  return SRX_OK;
}

extern "C" size_t srx_grad_guard_ws_bytes(int64_t n) { return n > 0 ? (size_t)stream_blocks(n) * sizeof(double) : 0; }

extern "C" int srx_grad_guard(const float* g, int64_t n, float grad_scale, float max_norm, int skip_nonfinite, void* ws,
                              size_t ws_bytes, srx_grad_guard_t* state, void* stream) {
  static_assert(sizeof(srx_grad_guard_t) == 32, "srx_grad_guard_t is 32 bytes");
  SRX_REQUIRE(g && ws && state && n > 0, "grad_guard: bad argument (null pointer or n <= 0)");
  SRX_REQUIRE(isfinite(grad_scale) && grad_scale != 0.f, "grad_guard: grad_scale must be finite and non-zero");
  SRX_REQUIRE(!isnan(max_norm), "grad_guard: max_norm is NaN (<= 0 or inf: no clipping)");
  SRX_REQUIRE(ws_bytes >= srx_grad_guard_ws_bytes(n), "grad_guard: workspace too small (%zu < %zu bytes)", ws_bytes,
              srx_grad_guard_ws_bytes(n));
  SRX_REQUIRE(((uintptr_t)g % 16 == 0) && ((uintptr_t)ws % 8 == 0) && ((uintptr_t)state % 8 == 0),
              "grad_guard: g must be 16-byte, ws and state 8-byte aligned");
  hipStream_t st = srx_stream(stream);
  const int64_t blocks = stream_blocks(n);
  hipLaunchKernelGGL(guard_sumsq_kernel, dim3((unsigned)blocks), dim3(256), 0, st, g, n, (double*)ws);
  SRX_CHECK_LAUNCH("guard_sumsq_kernel");
  hipLaunchKernelGGL(guard_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, (int)blocks, grad_scale, max_norm,
                     skip_nonfinite ? 1 : 0, state);
  SRX_CHECK_LAUNCH("guard_finalize_kernel");
  return SRX_OK;
}

extern "C" int srx_adam_step_guarded(float* p, const float* g, float* m, float* v, int64_t n, const float* lr, float beta1,
                                     float beta2, float eps, float grad_scale, int64_t* step,
                                     const srx_grad_guard_t* state, void* stream) {
  SRX_REQUIRE(p && g && m && v && lr && step && state && n > 0, "adam_step_guarded: bad argument");
  SRX_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)m % 16 == 0) &&
                  ((uintptr_t)v % 16 == 0) && ((uintptr_t)state % 8 == 0),
              "adam_step_guarded: buffers must be 16-byte, state 8-byte aligned");
  hipStream_t st = srx_stream(stream);
  hipLaunchKernelGGL(adam_tick_guarded_kernel, dim3(1), dim3(1), 0, st, step, state);
  SRX_CHECK_LAUNCH("adam_tick_guarded_kernel");
  hipLaunchKernelGGL(adam_guarded_kernel, dim3((unsigned)stream_blocks(n)), dim3(256), 0, st, p, g, m, v, n, lr, beta1,
                     beta2, eps, grad_scale, step, state);
  SRX_CHECK_LAUNCH("adam_guarded_kernel");
  return SRX_OK;
}
