// The training pair pool on the device ('Training pair pool'): Real-ESRGAN's _dequeue_and_enqueue as one launch.
// Sample i of a batch and slot slots[i] of a pool change places (or the sample is stored there), the low-resolution side and
// its target in the SAME launch, so that a pair never parts.  The kernel only moves 32-bit words: no arithmetic touches a
// value, so every bit pattern (NaN payloads, -0.0, denormals) arrives as it left.  No atomics, no device state; the grid
// comes from the element counts and the batch size alone, never from the device or the planner's reserved compute units.
#include "srx_common.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kPoolThreads = 256;
constexpr int kPoolUnitsPerThread = 2;   // units (16 bytes, or one float on the scalar path) a thread moves when the grid is not capped
constexpr int kPoolMaxBlocks = 64;       // blocks per sample and side; the grid-stride loop takes what is left

// units of ``T`` of ONE sample; ``first`` .. : this block's share of the grid-stride loop.  mode 0: pool <- batch; 1: exchange
// (both sides read into registers, then both written: a unit is owned by exactly one thread, so nothing is read after it changed)
template <typename T>
__device__ __forceinline__ void pool_move(T* __restrict__ pool, T* __restrict__ batch, unsigned units, unsigned first,
                                          unsigned stride, int mode) {
  // unsigned: units < 2^31 and stride <= 2^14, so i + stride cannot wrap
  if (mode == 0) {
    for (unsigned i = first; i < units; i += stride) pool[i] = batch[i];
  } else {
    for (unsigned i = first; i < units; i += stride) {
      const T p = pool[i], b = batch[i];
      pool[i] = b;
      batch[i] = p;
    }
  }
}

// grid: (blocks_a + blocks_b, n); blocks with blockIdx.x < blocks_a move side a of sample blockIdx.y, the others side b.
// vec_x: side x is moved in 16-byte units (elems_x % 4 == 0 and both bases 16-byte aligned: checked on the host).
__global__ __launch_bounds__(kPoolThreads) void pool_exchange_kernel(float* pool_a, float* batch_a, int elems_a, int vec_a,
                                                                     int blocks_a, float* pool_b, float* batch_b, int elems_b,
                                                                     int vec_b, int blocks_b, const int32_t* __restrict__ slots,
                                                                     int cap, int mode) {
  const int n = blockIdx.y;
  const int slot = slots[n];
  if ((unsigned)slot >= (unsigned)cap) return;  // any value is safe: the sample and the pool stay as they are
  const bool a = (int)blockIdx.x < blocks_a;
  float* pool = a ? pool_a : pool_b;
  float* batch = a ? batch_a : batch_b;
  const int elems = a ? elems_a : elems_b, vec = a ? vec_a : vec_b, blocks = a ? blocks_a : blocks_b;
  const int bx = a ? (int)blockIdx.x : (int)blockIdx.x - blocks_a;
  pool += (size_t)slot * elems;   // < cap * elems < 2^31 floats
  batch += (size_t)n * elems;
  const unsigned first = (unsigned)bx * kPoolThreads + threadIdx.x, stride = (unsigned)blocks * kPoolThreads;  // <= 2^14
  if (vec)
    pool_move(reinterpret_cast<u32x4*>(pool), reinterpret_cast<u32x4*>(batch), (unsigned)elems >> 2, first, stride, mode);
  else
    pool_move(reinterpret_cast<uint32_t*>(pool), reinterpret_cast<uint32_t*>(batch), (unsigned)elems, first, stride, mode);
}

bool pool_apart(uintptr_t a, uintptr_t a_bytes, uintptr_t b, uintptr_t b_bytes) { return a + a_bytes <= b || b + b_bytes <= a; }

int pool_blocks(int64_t units) {
  const int64_t b = srx_cdiv(units, (int64_t)kPoolThreads * kPoolUnitsPerThread);
  return (int)(b < 1 ? 1 : b > kPoolMaxBlocks ? kPoolMaxBlocks : b);
}

}  // namespace

extern "C" int srx_pool_exchange(float* pool_a, float* batch_a, int64_t elems_a, float* pool_b, float* batch_b, int64_t elems_b,
                                 const int32_t* slots, int n, int cap, int mode, void* stream) {
  SRX_REQUIRE(pool_a && batch_a && slots, "pool_exchange: null pointer (pool_a %p, batch_a %p, slots %p)", (void*)pool_a,
              (void*)batch_a, (const void*)slots);
  SRX_REQUIRE((pool_b == nullptr) == (batch_b == nullptr), "pool_exchange: pool_b and batch_b must both be given or both be null "
              "(pool_b %p, batch_b %p)", (void*)pool_b, (void*)batch_b);
  SRX_REQUIRE(elems_a >= 1 && elems_b >= 0, "pool_exchange: bad element counts: elems_a must be >= 1 and elems_b >= 0, got %lld and %lld",
              (long long)elems_a, (long long)elems_b);
  SRX_REQUIRE((pool_b != nullptr) == (elems_b != 0), "pool_exchange: a null _b pair goes with elems_b == 0 and a given one with "
              "elems_b >= 1 (pool_b %p, elems_b %lld)", (void*)pool_b, (long long)elems_b);
  SRX_REQUIRE(n >= 1 && n <= 65535, "pool_exchange: n must be in 1..65535, got %d", n);
  SRX_REQUIRE(cap >= 1 && n <= cap, "pool_exchange: cap must be >= 1 and hold a batch: cap %d, n %d", cap, n);
  const int64_t lim = (int64_t)1 << 31;
  SRX_REQUIRE(elems_a <= (lim - 1) / cap && elems_b <= (lim - 1) / cap, "pool_exchange: too large: cap * elems must stay below 2^31 "
              "(cap %d, elems %lld and %lld)", cap, (long long)elems_a, (long long)elems_b);
  // the four (or two) ranges must lie apart: a batch inside its pool, or one side inside the other, would be moved twice
  const uintptr_t base[4] = {(uintptr_t)pool_a, (uintptr_t)batch_a, (uintptr_t)pool_b, (uintptr_t)batch_b};
  const uintptr_t bytes[4] = {(uintptr_t)(cap * elems_a) * 4, (uintptr_t)(n * elems_a) * 4, (uintptr_t)(cap * elems_b) * 4,
                              (uintptr_t)(n * elems_b) * 4};
  for (int i = 0; i < (pool_b ? 4 : 2); ++i)
    for (int j = i + 1; j < (pool_b ? 4 : 2); ++j)
      SRX_REQUIRE(pool_apart(base[i], bytes[i], base[j], bytes[j]), "pool_exchange: the pool and batch ranges must not overlap "
                  "(pool_a %p + %zu, batch_a %p + %zu, pool_b %p + %zu, batch_b %p + %zu bytes)", (void*)pool_a, (size_t)bytes[0],
                  (void*)batch_a, (size_t)bytes[1], (void*)pool_b, (size_t)bytes[2], (void*)batch_b, (size_t)bytes[3]);
  SRX_REQUIRE(mode == 0 || mode == 1, "pool_exchange: mode must be 0 (store) or 1 (exchange), got %d", mode);
  // 16-byte units where every sample base is 16-byte aligned: elems % 4 == 0 on aligned tensors; else one float at a time
  const int vec_a = elems_a % 4 == 0 && base[0] % 16 == 0 && base[1] % 16 == 0;
  const int vec_b = pool_b && elems_b % 4 == 0 && base[2] % 16 == 0 && base[3] % 16 == 0;
  const int blocks_a = pool_blocks(vec_a ? elems_a / 4 : elems_a);
  const int blocks_b = pool_b ? pool_blocks(vec_b ? elems_b / 4 : elems_b) : 0;
  hipLaunchKernelGGL(pool_exchange_kernel, dim3((unsigned)(blocks_a + blocks_b), (unsigned)n), dim3(kPoolThreads), 0,
                     srx_stream(stream), pool_a, batch_a, (int)elems_a, vec_a, blocks_a, pool_b, batch_b, (int)elems_b, vec_b,
                     blocks_b, slots, cap, mode);
  SRX_CHECK_LAUNCH("pool_exchange_kernel");
  return SRX_OK;
}
