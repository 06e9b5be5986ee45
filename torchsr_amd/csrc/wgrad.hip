// Weight gradient of the gather-GEMM convolution (gconv.hip) on gfx950 (MI355X):
//
//   dW[n][k] = sum_m dy[m][n] * A(m,k),   A(m,k) = in[ipix(m)+tap(k)][chan(k)]  (0 outside)
//
// The pixel axis m is cut into row splits that write partial slabs; a reduce kernel sums them into the OIHW gradient
// (and the bias gradient).  Several problems of one geometry run in one launch.
#include "conv_host.h"
#include <cstdio>

namespace {

// ---------------------------------------------------------------------------
// weight gradient: slab[z][n][k] = sum_{m in split z} dy[m][n] * A(m,k)
// workgroup tile 64(n) x 64(k), 4 waves of 32x32, m consumed 32 rows at a time.
// ---------------------------------------------------------------------------
struct WArgs {
  const float* in; const float* dy; float* slab;
  int N, Hi, Wi, Ci, Hm, Wm, M, HmWm;
  float inv_HmWm, inv_Wm;
  int in_stride, nth, ntw, dh0, dw0, Ck, K, Kw;
  int Cd, Cdv, dy_shuffle, Cnw;
  int rows_per_split, ktiles;
  unsigned in_bytes, dy_bytes;  // raw-buffer ranges (see GArgs)
  // A thread's rows advance by 32 per chunk; its pixel coordinates and both element offsets follow
  // incrementally from these host-computed steps (no division in the loop):
  //   s_c = 32 % Wm, s_rm = (32 / Wm) % Hm; dX0/dD0 plain step, dX1/dD1 extra on a column wrap
  //   (mw -= Wm, mh += 1), dX2 extra on a row wrap (mh -= Hm, next image)
  int s_c, s_rm, dX0, dX1, dX2, dD0, dD1;
  // bias gradient db[n] = sum_m dy[m][n]: the k-tile-0 workgroups already stage every dy row of their
  // row split, so they add the column sums up on the way and write one [Cnw] row per split here
  // (null: not wanted); wgrad_reduce_kernel sums the rows.  Replaces two column-sum launches per layer.
  float* bslab;
  int nsplit, nprob;
};

// Several weight-gradient problems of ONE geometry in one launch (blockIdx.y = problem): the 33 residual convs
// of the SRGAN generator are 0.68 GFLOP each -- alone, such a problem is all pipeline fill and slab reduction
// (19 + 5 us for 4.3 us of matrix work) -- and nothing downstream waits for a weight gradient before the
// optimiser, so the host collects them during the backward pass and issues them together: long loops, every CU
// holding several workgroups, one reduction.  Problems may also be SEGMENTS of one gradient (the discriminator's
// real and fake passes): `per_out` consecutive problems are summed into one output.
constexpr int WG_MAXP = 72;
struct WMulti {
  WArgs a;
  const float* x[WG_MAXP];
  const float* dy[WG_MAXP];
};
struct WReduce {
  float* dw[WG_MAXP];
  float* db[WG_MAXP];  // entries may be null
  // multiplies the output's weight and bias gradient: the layer's dy tensor stands for scale * dy (a dense block's conv5
  // sees the block's output gradient times scale_ratio, which is then never written out)
  float scale[WG_MAXP];
  // Paired problems (rows_lo > 0): the tile rows [0, rows_lo) are the gradient of one conv (dw, db; cin_lo input channels)
  // and the rows above that of a second conv (dw_hi, db_hi; Cin input channels) that reads the SAME input buffer and
  // whose output gradient is the adjacent channel slice -- two convs of a dense block (esrgan/residual.py:81-85), which
  // alone are 32 columns wide and would each leave half of every 64-column tile multiplying padding.
  float* dw_hi[WG_MAXP];
  float* db_hi[WG_MAXP];
  int rows_lo, cin_lo;
};

// PR = 1: bf16 products (the autocast mode).  The contraction runs over pixels, so an MFMA operand is eight
// CONSECUTIVE ROWS of one column.  A thread therefore loads two adjacent rows (2 r0, 2 r0 + 1), rounds them
// to bf16 and stores them interleaved -- one 32-bit word per (row pair, column) -- so that a lane collects
// its eight rows as four words; two v_mfma_f32_32x32x16_bf16 per chunk replace sixteen fp32 MFMAs.
template <int PR>
__global__ __launch_bounds__(256) void wgrad_kernel(const WMulti mp) {
  const WArgs& a = mp.a;
  // Work item = (tile, problem, row split), tile fastest.  The (up to 9 x Cout/64) tiles of one problem's row split read the
  // same dy and x rows, so they should share an L2: workgroups are dealt round-robin over the 8 XCDs, and this remap gives
  // every XCD a contiguous range of work items (MI355X_MICROARCH.md, XCD placement; a speed matter only -- with the plain
  // order the 33-problem group read 1.23 GB through the fabric per launch, 8x its operands).
  int wi;
  {
    const int W = (int)gridDim.x, b = (int)blockIdx.x, xcd = b & 7, slot = b >> 3, q = W >> 3, r = W & 7;
    wi = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
  }
  const int tiles_ = a.ktiles * (a.Cnw / 64);
  const int tile_id = wi % tiles_, rest_ = wi / tiles_;
  const int prob = srx_uniform(rest_ % a.nprob), zsplit = srx_uniform(rest_ / a.nprob);
  // LDS image of a chunk (32 pixels x 64 columns).  fp32: [pixel][64] floats.  bf16: [pixel][64] bf16 in rows of PSTR = 192
  // bytes (the 64-byte pad puts the four rows of a transposing read on different banks): operands are stored as they
  // arrive -- one 8-byte store per loaded quad -- and an MFMA operand (eight consecutive PIXELS of one column) is two
  // ds_read_b64_tr_b16, the hardware's transposing read, instead of four scalar reads of hand-interleaved row pairs
  constexpr int PSTR = 192;
  constexpr int BUF_FLOATS = PR ? 32 * PSTR / 4 : 32 * 64;
  __shared__ __attribute__((aligned(16))) float sD[2][BUF_FLOATS];
  __shared__ __attribute__((aligned(16))) float sX[2][BUF_FLOATS];
  const int tid = threadIdx.x, lane = tid & 63, wave = srx_uniform(tid >> 6);
  const int ntile = srx_uniform(tile_id / a.ktiles), kt = srx_uniform(tile_id - ntile * a.ktiles);
  const int k0 = kt * 64, n0 = ntile * 64;
  const int q = tid & 15, r0 = tid >> 4;
  const __amdgpu_buffer_rsrc_t rx_ = srx_rsrc(mp.x[prob], a.in_bytes), rd_ = srx_rsrc(mp.dy[prob], a.dy_bytes);

  // this thread's fixed k (A gather) and fixed dy column
  const int k = k0 + 4 * q;
  const bool kvalid = k < a.K;
  int dh = 0, dw = 0, kc = 0;
  if (kvalid) {
    const int tap = k / a.Ck;
    kc = k - tap * a.Ck;
    const int th = tap / a.ntw, tw = tap - th * a.ntw;
    dh = a.dh0 + th;
    dw = a.dw0 + tw;
  }
  const int col = n0 + 4 * q;
  const bool cvalid = col < a.Cdv;
  int sh_i = 0, sh_j = 0, sh_c = col;
  if (a.dy_shuffle) {
    const int ij = col / a.dy_shuffle;
    sh_c = col - ij * a.dy_shuffle;
    sh_i = ij >> 1;
    sh_j = ij & 1;
  }

  const int mbeg = zsplit * a.rows_per_split;
  const int mend = min(a.M, mbeg + a.rows_per_split);

  // Four register stages: a workgroup that is alone on its CU (small layers: one row split per CU)
  // multiplies a chunk in ~0.45 us but waits ~2 us for a load, so chunk c+4 is requested while c runs.
  f32x4 rd0[2], rx0[2], rd1[2], rx1[2], rd2[2], rx2[2], rd3[2], rx3[2];
  // row state of this thread's two rows (r0 + 16p of the current chunk; 2 r0 + p for bf16); chunks are
  // requested strictly in order, so every gload advances the state by one chunk
  int rm[2], rmh[2], rmw[2];
  unsigned rox[2], rod[2];  // element offsets: x at (n, mh*stride + dh, mw*stride + dw, kc); dy at the thread's column
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int m = PR ? mbeg + 2 * r0 + p : mbeg + r0 + 16 * p;
    int n, rem, mh, mw;
    srx_divmod(m, a.HmWm, a.inv_HmWm, n, rem);
    srx_divmod(rem, a.Wm, a.inv_Wm, mh, mw);
    rm[p] = m; rmh[p] = mh; rmw[p] = mw;
    rox[p] = (unsigned)(((n * a.Hi + mh * a.in_stride + dh) * a.Wi + mw * a.in_stride + dw) * a.Ci + kc);
    rod[p] = (unsigned)(a.dy_shuffle ? ((n * 2 * a.Hm + 2 * mh + sh_i) * (2 * a.Wm) + 2 * mw + sh_j) * a.Cd + sh_c
                                     : m * a.Cd + col);
  }
  auto gload = [&](f32x4 (&rd)[2], f32x4 (&rx)[2]) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const bool valid = rm[p] < mend;
      const int ih = rmh[p] * a.in_stride + dh, iw = rmw[p] * a.in_stride + dw;
      const bool okx = valid && kvalid && ((unsigned)ih < (unsigned)a.Hi) && ((unsigned)iw < (unsigned)a.Wi);
      rx[p] = srx_bload(rx_, okx ? 4u * rox[p] : 0xffffffffu, 0);  // out of range reads 0
      rd[p] = srx_bload(rd_, (valid && cvalid) ? 4u * rod[p] : 0xffffffffu, 0);
      // advance 32 rows
      rm[p] += 32; rmw[p] += a.s_c; rmh[p] += a.s_rm; rox[p] += (unsigned)a.dX0; rod[p] += (unsigned)a.dD0;
      const bool wc = rmw[p] >= a.Wm;
      rmw[p] -= wc ? a.Wm : 0; rmh[p] += wc ? 1 : 0;
      rox[p] += wc ? (unsigned)a.dX1 : 0u; rod[p] += wc ? (unsigned)a.dD1 : 0u;
      const bool wr = rmh[p] >= a.Hm;
      rmh[p] -= wr ? a.Hm : 0;
      rox[p] += wr ? (unsigned)a.dX2 : 0u;
    }
  };
  const bool want_bias = a.bslab != nullptr && kt == 0;  // workgroup-uniform
  f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
  auto swrite = [&](int buf, const f32x4 (&rd)[2], const f32x4 (&rx)[2]) {
    if (want_bias) bsum += rd[0] + rd[1];  // (fp32 values, whatever the product precision)
    if (PR) {  // row 2 r0 + p, columns 4q .. 4q + 3, rounded to bf16
      typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const bf16x4 pd = {(__bf16)rd[p][0], (__bf16)rd[p][1], (__bf16)rd[p][2], (__bf16)rd[p][3]};
        const bf16x4 px = {(__bf16)rx[p][0], (__bf16)rx[p][1], (__bf16)rx[p][2], (__bf16)rx[p][3]};
        unsigned char* bD = reinterpret_cast<unsigned char*>(&sD[buf][0]) + (2 * r0 + p) * PSTR + 8 * q;
        unsigned char* bX = reinterpret_cast<unsigned char*>(&sX[buf][0]) + (2 * r0 + p) * PSTR + 8 * q;
        *reinterpret_cast<bf16x4*>(bD) = pd;
        *reinterpret_cast<bf16x4*>(bX) = px;
      }
      return;
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      *reinterpret_cast<f32x4*>(&sD[buf][(r0 + 16 * p) * 64 + q * 4]) = rd[p];
      *reinterpret_cast<f32x4*>(&sX[buf][(r0 + 16 * p) * 64 + q * 4]) = rx[p];
    }
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int h = lane >> 5, l31 = lane & 31;
  const int wn = wave >> 1, wk = wave & 1;

  auto compute = [&](int buf) {
    if (PR) {  // MFMA s contracts pixels 16 s + 8 h .. + 7: two transposing reads of 4 pixels x 16 columns per 16-lane group
      typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
      typedef short s16x4 __attribute__((ext_vector_type(4)));
      typedef short s16x8 __attribute__((ext_vector_type(8)));
      typedef s16x4 __attribute__((address_space(3))) * lds_s16x4;
      const int li = lane & 15, colh = 16 * ((lane >> 4) & 1) + 4 * (li & 3), rq = li >> 2;
      const unsigned char* bD = reinterpret_cast<const unsigned char*>(&sD[buf][0]) + (8 * h + rq) * PSTR + 2 * (wn * 32 + colh);
      const unsigned char* bX = reinterpret_cast<const unsigned char*>(&sX[buf][0]) + (8 * h + rq) * PSTR + 2 * (wk * 32 + colh);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const s16x4 d0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(bD + (16 * s) * PSTR));
        const s16x4 d1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(bD + (16 * s + 4) * PSTR));
        const s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(bX + (16 * s) * PSTR));
        const s16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(bX + (16 * s + 4) * PSTR));
        const s16x8 fd = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
        const s16x8 fx = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fd), __builtin_bit_cast(bf16x8, fx), acc, 0, 0, 0);
      }
      return;
    }
    const float* cD = &sD[buf][h * 64 + wn * 32 + l31];
    const float* cX = &sX[buf][h * 64 + wk * 32 + l31];
    // Operands run two MFMA pairs ahead of the multiplies (one ds_read2st64_b32 fetches a pair's d or x): left to itself
    // the compiler read each pair right before its MFMAs and waited for it -- an LDS round trip per 128 MFMA cycles, which
    // three waves per SIMD did not hide (PMC, round 3: MFMA pipe 54 % busy, 61 % of wave time in s_waitcnt)
    float dv[16], xv[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) { dv[s] = cD[s * 128]; xv[s] = cX[s * 128]; }
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[s], xv[s], acc, 0, 0, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      if (i < 6) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    }
  };
  // every step issues the same four loads (rows past `mend` are pointed out of range and read 0), so
  // the prefetch waits are exact vmcnt counts -- see gconv_body
  gload(rd0, rx0);
  gload(rd1, rx1);
  gload(rd2, rx2);
  gload(rd3, rx3);
  swrite(0, rd0, rx0);
  __syncthreads();
  for (int mb = mbeg; mb < mend; mb += 128) {
    gload(rd0, rx0);  // chunk at mb + 128
    compute(0);
    swrite(1, rd1, rx1);
    __syncthreads();
    gload(rd1, rx1);
    if (mb + 32 < mend) compute(1);
    swrite(0, rd2, rx2);
    __syncthreads();
    gload(rd2, rx2);
    if (mb + 64 < mend) compute(0);
    swrite(1, rd3, rx3);
    __syncthreads();
    gload(rd3, rx3);
    if (mb + 96 < mend) compute(1);
    swrite(0, rd0, rx0);
    __syncthreads();
  }
  const size_t slab_id = (size_t)prob * a.nsplit + zsplit;
  float* slab = a.slab + slab_id * a.Cnw * a.Kw;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = n0 + wn * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    slab[(size_t)row * a.Kw + k0 + wk * 32 + l31] = acc[r];
  }
  if (want_bias) {  // 16 row lanes x 16 column quads -> 64 column sums of this row split
    f32x4* red = reinterpret_cast<f32x4*>(&sD[0][0]);  // (the loop ended on a barrier: the buffers are free)
    red[r0 * 16 + q] = bsum;
    __syncthreads();
    if (tid < 16) {
      f32x4 t = red[tid];
#pragma unroll
      for (int r = 1; r < 16; ++r) t += red[r * 16 + tid];
      *reinterpret_cast<f32x4*>(a.bslab + slab_id * a.Cnw + n0 + 4 * tid) = t;
    }
  }
}

// ---------------------------------------------------------------------------
// fp32 weight gradient with LDS-DMA staging (round 4).  wgrad_kernel<0> moves every chunk global -> registers (four stages
// of 16 VGPRs) -> ds_write_b128 -> LDS and spends 61 % of its wave time in s_waitcnt at 66 % MFMA-busy
// (profiles/r03_pmc_wgrad.txt).  Both operands are "row r0 = tid / 16, quad tid % 16" images of [32 rows][64 floats]: byte
// 16 * tid of the chunk buffer, i.e. lane-linear -- so buffer_load_dwordx4 ... lds can land them in LDS directly (per-lane
// SOURCE address = the gather; rows past the split and padding taps are pointed out of range and arrive as zeros), with no
// staging registers, no LDS stores and a ring of three chunk buffers: chunk c + 2 is requested while chunk c is multiplied,
// and the only wait in the loop is a counted vmcnt that leaves the newest chunk's four requests in flight.
// Same work decomposition, slab layout and bias rows as wgrad_kernel<0>: the reduction kernel is shared.
// ---------------------------------------------------------------------------
// WIDE (round 6): on gfx950 the f32 MFMA runs on the vector ALUs -- every VALU instruction of the gather's bookkeeping is matrix time
// lost (tools/probe/mfma_valu.hip) -- and the row state (pixel coordinates, two element offsets, three wrap tests: ~25 instructions)
// was advanced for TWO rows per thread and chunk.  When a tap's channels come in multiples of 64 (every layer of the SRGAN step that
// runs here) a thread owns ONE row of the chunk and both 32-float halves of it (same tap, same validity: the second request is the
// first + 32 elements), and the chunk image in LDS is [half][32 rows][32 floats] -- still lane-linear for the DMA, and a wave's MFMA
// operand is exactly one half.  Half the bookkeeping per MFMA.
// LIN (round 6, with WIDE): stride 1, output as large as the input, no PixelShuffle on dy, K and the dy columns in whole tiles of 64.
// Then both element offsets are LINEAR in the row m -- x: (m + dh Wi + dw) Ci + kc, dy: m Cd + col -- and all that is left of the row
// state is one bit per row: does tap (dh, dw) of pixel m fall inside the image.  The workgroup's tap is uniform (a k-tile of 64 lies
// inside one tap), so the bits of its row split are built ONCE per workgroup -- one ballot per 64 rows -- into an LDS table of one word
// per chunk, and a request is a bit test, two selects and three adds where it was ~40 instructions of coordinates and wrap tests
// (every one of them matrix time: the f32 MFMA shares the vector ALUs).  Same loads in the same order: bit-identical slabs.
constexpr int WG_MASKW = 768;  // chunks (incl. the two look-ahead requests) a LIN workgroup can index: 3 KB next to the 48 KB ring
template <bool WIDE, bool LIN = false>
__global__ __launch_bounds__(256) void wgrad_dma_kernel(const WMulti mp) {
  static_assert(!LIN || WIDE, "LIN is a form of WIDE");
  const WArgs& a = mp.a;
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  int wi;
  {  // XCD-contiguous work order (see wgrad_kernel)
    const int W = (int)gridDim.x, b = (int)blockIdx.x, xcd = b & 7, slot = b >> 3, q = W >> 3, r = W & 7;
    wi = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
  }
  const int tiles_ = a.ktiles * (a.Cnw / 64);
  const int tile_id = wi % tiles_, rest_ = wi / tiles_;
  const int prob = srx_uniform(rest_ % a.nprob), zsplit = srx_uniform(rest_ / a.nprob);
  constexpr int NSLOT = 3, CHUNK = 32 * 64;  // floats per operand and chunk
  __shared__ __attribute__((aligned(16))) float sD[NSLOT][CHUNK];
  __shared__ __attribute__((aligned(16))) float sX[NSLOT][CHUNK];
  const int tid = threadIdx.x, lane = tid & 63, wave = srx_uniform(tid >> 6);
  const int ntile = srx_uniform(tile_id / a.ktiles), kt = srx_uniform(tile_id - ntile * a.ktiles);
  const int k0 = kt * 64, n0 = ntile * 64;
  constexpr int NP = WIDE ? 1 : 2;                  // row states per thread
  const int q = WIDE ? (tid & 7) : (tid & 15), r0 = WIDE ? (tid >> 3) : (tid >> 4);
  auto make_rsrc = [](const void* p, unsigned bytes) {
    const unsigned long long v = (unsigned long long)p;
    u32x4 r;
    r[0] = (unsigned)srx_uniform((int)(unsigned)v);
    r[1] = (unsigned)srx_uniform((int)((unsigned)(v >> 32) & 0xffffu));
    r[2] = bytes;
    r[3] = 0x00020000u;
    return r;
  };
  const u32x4 rx_ = make_rsrc(mp.x[prob], a.in_bytes), rd_ = make_rsrc(mp.dy[prob], a.dy_bytes);

  // this thread's fixed k (A gather) and fixed dy column (WIDE: of the first half; the second half is 32 further, same tap)
  const int k = k0 + 4 * q;
  const bool kvalid = k < a.K, kvalid1 = WIDE && k + 32 < a.K;
  int dh = 0, dw = 0, kc = 0;
  if (kvalid) {
    const int tap = k / a.Ck;
    kc = k - tap * a.Ck;
    const int th = tap / a.ntw, tw = tap - th * a.ntw;
    dh = a.dh0 + th;
    dw = a.dw0 + tw;
  }
  const int col = n0 + 4 * q;
  const bool cvalid = col < a.Cdv, cvalid1 = WIDE && col + 32 < a.Cdv;
  int sh_i = 0, sh_j = 0, sh_c = col;
  if (a.dy_shuffle) {  // (WIDE: a sub-pixel's channels come in multiples of 64 too, checked on the host: both halves in one sub-pixel)
    const int ij = col / a.dy_shuffle;
    sh_c = col - ij * a.dy_shuffle;
    sh_i = ij >> 1;
    sh_j = ij & 1;
  }
  const int mbeg = zsplit * a.rows_per_split;
  const int mend = min(a.M, mbeg + a.rows_per_split);

  __shared__ unsigned okmask[LIN ? WG_MASKW : 1];
  if constexpr (LIN) {  // bit r of word c: tap (dh, dw) of row mbeg + 32 c + r is inside the image (and the row inside the split)
    // (chunks + 3 words: request() reads the word after the last look-ahead's too; the host keeps chunks + 3 <= WG_MASKW)
    const int nrows = (((mend - mbeg + 31) / 32 + 3) * 32 + 63) & ~63;
    for (int base = wave * 64; base < nrows; base += 256) {
      const int m = mbeg + base + lane;
      int n, rem, mh, mw;
      srx_divmod(m, a.HmWm, a.inv_HmWm, n, rem);
      srx_divmod(rem, a.Wm, a.inv_Wm, mh, mw);
      const bool ok = m < mend && ((unsigned)(mh + dh) < (unsigned)a.Hi) && ((unsigned)(mw + dw) < (unsigned)a.Wi);
      const unsigned long long bits = __ballot(ok);
      if (lane == 0) { okmask[base >> 5] = (unsigned)bits; okmask[(base >> 5) + 1] = (unsigned)(bits >> 32); }
    }
    __syncthreads();
  }
  // row state of this thread's rows (r0 [+ 16 p] of the current chunk), advanced by one chunk per request
  int rm[NP], rmh[NP], rmw[NP];
  unsigned rox[NP], rod[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int m = mbeg + r0 + 16 * p;
    int n, rem, mh, mw;
    srx_divmod(m, a.HmWm, a.inv_HmWm, n, rem);
    srx_divmod(rem, a.Wm, a.inv_Wm, mh, mw);
    rm[p] = m; rmh[p] = mh; rmw[p] = mw;
    rox[p] = (unsigned)(((n * a.Hi + mh * a.in_stride + dh) * a.Wi + mw * a.in_stride + dw) * a.Ci + kc);
    rod[p] = (unsigned)(a.dy_shuffle ? ((n * 2 * a.Hm + 2 * mh + sh_i) * (2 * a.Wm) + 2 * mw + sh_j) * a.Cd + sh_c
                                     : m * a.Cd + col);
  }
  const unsigned ldsX = (unsigned)(size_t)&sX[0][0], ldsD = (unsigned)(size_t)&sD[0][0];
  auto dma = [&](const u32x4& rs, unsigned voff, unsigned dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(dst), "s"(rs) : "memory");
  };
  // four requests per wave and chunk, always (so that the waits can be counted).  Two rows per thread: the thread's 16 bytes of row
  // r0 + 16 p land at byte 16 tid + 4096 p of the slot ([32 rows][64 floats]).  WIDE: the thread's 16 bytes of half hf of row r0 land
  // at byte 16 tid + 4096 hf ([half][32 rows][32 floats])
  constexpr unsigned OORL = 0xfffff000u;  // (an out-of-range offset that stays out of range with the second half's 128 bytes added)
  unsigned lin_x = 0, lin_d = 0, lin_w = 0;
  int lin_c = 0;
  if constexpr (LIN) {
    lin_x = 4u * (unsigned)((mbeg + r0 + dh * a.Wi + dw) * a.Ci + kc);  // (wraps for rows whose tap lies in front of the tensor: masked)
    lin_d = 4u * (unsigned)((mbeg + r0) * a.Cd + col);
    lin_w = okmask[0];
  }
  const unsigned lin_sx = 128u * (unsigned)a.Ci, lin_sd = 128u * (unsigned)a.Cd;  // 32 rows further, in bytes
  auto request = [&](int slot) {
    if constexpr (LIN) {
      const bool okx = (lin_w >> r0) & 1u;
      const bool okd = rm[0] < mend;
      const unsigned vx = okx ? lin_x : OORL, vd = okd ? lin_d : OORL;
      const unsigned dst = (unsigned)srx_uniform((int)((unsigned)(slot * CHUNK * 4) + (unsigned)(wave * 1024)));
      dma(rx_, vx, ldsX + dst);
      dma(rd_, vd, ldsD + dst);
      dma(rx_, vx + 128u, ldsX + dst + 4096u);
      dma(rd_, vd + 128u, ldsD + dst + 4096u);
      rm[0] += 32; lin_x += lin_sx; lin_d += lin_sd;
      lin_c += 1;
      lin_w = okmask[lin_c];  // (the next request's word: back long before it is tested)
      return;
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const bool valid = rm[p] < mend;
      const int ih = rmh[p] * a.in_stride + dh, iw = rmw[p] * a.in_stride + dw;
      const bool okx = valid && kvalid && ((unsigned)ih < (unsigned)a.Hi) && ((unsigned)iw < (unsigned)a.Wi);
      const unsigned dst = (unsigned)srx_uniform((int)((unsigned)(slot * CHUNK * 4) + (unsigned)(p * 4096 + wave * 1024)));
      dma(rx_, okx ? 4u * rox[p] : 0xffffffffu, ldsX + dst);
      dma(rd_, (valid && cvalid) ? 4u * rod[p] : 0xffffffffu, ldsD + dst);
      if constexpr (WIDE) {
        dma(rx_, (okx && kvalid1) ? 4u * rox[p] + 128u : 0xffffffffu, ldsX + dst + 4096u);
        dma(rd_, (valid && cvalid1) ? 4u * rod[p] + 128u : 0xffffffffu, ldsD + dst + 4096u);
      }
      rm[p] += 32; rmw[p] += a.s_c; rmh[p] += a.s_rm; rox[p] += (unsigned)a.dX0; rod[p] += (unsigned)a.dD0;
      const bool wc = rmw[p] >= a.Wm;
      rmw[p] -= wc ? a.Wm : 0; rmh[p] += wc ? 1 : 0;
      rox[p] += wc ? (unsigned)a.dX1 : 0u; rod[p] += wc ? (unsigned)a.dD1 : 0u;
      const bool wr = rmh[p] >= a.Hm;
      rmh[p] -= wr ? a.Hm : 0;
      rox[p] += wr ? (unsigned)a.dX2 : 0u;
    }
  };
  const bool want_bias = a.bslab != nullptr && kt == 0;  // workgroup-uniform
  f32x4 bsum = {0.f, 0.f, 0.f, 0.f}, bsum1 = {0.f, 0.f, 0.f, 0.f};
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int h = lane >> 5, l31 = lane & 31;
  const int wn = wave >> 1, wk = wave & 1;
  // MFMA step s multiplies rows 2 s + h of the chunk: floats between two steps / between the two lane halves / to this wave's columns
  constexpr int SSTEP = WIDE ? 64 : 128, HSTEP = WIDE ? 32 : 64, WSTEP = WIDE ? 1024 : 32;
  auto compute = [&](int slot) {
    const float* cD = &sD[0][0] + slot * CHUNK + h * HSTEP + wn * WSTEP + l31;
    const float* cX = &sX[0][0] + slot * CHUNK + h * HSTEP + wk * WSTEP + l31;
    if (want_bias) {  // (fp32 values of this thread's two dy quads, as wgrad_kernel<0> adds them)
      if constexpr (WIDE) {
        const float* bd = &sD[0][0] + slot * CHUNK + r0 * 32 + q * 4;
        bsum += *reinterpret_cast<const f32x4*>(bd);
        bsum1 += *reinterpret_cast<const f32x4*>(bd + 1024);
      } else {
        const float* bd = &sD[0][0] + slot * CHUNK + r0 * 64 + q * 4;
        bsum += *reinterpret_cast<const f32x4*>(bd) + *reinterpret_cast<const f32x4*>(bd + 16 * 64);
      }
    }
    float dv[16], xv[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) { dv[s] = cD[s * SSTEP]; xv[s] = cX[s * SSTEP]; }
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[s], xv[s], acc, 0, 0, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      if (i < 6) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    }
  };
  const int nchunks = (mend - mbeg + 31) / 32;
  request(0);
  request(1);  // (past the split's end: every lane out of range, zeros land -- never multiplied)
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // chunk 0 has landed, chunk 1 flies on
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  int slot = 0;
  for (int c = 0; c < nchunks; ++c) {
    int s2 = slot + 2; s2 = s2 >= NSLOT ? s2 - NSLOT : s2;
    request(s2);    // chunk c + 2 into the slot chunk c - 1 was read from (free since the barrier)
    compute(slot);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // chunk c + 1 has landed; the four requests of chunk c + 2 fly on
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    slot = slot + 1 == NSLOT ? 0 : slot + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the trailing requests write LDS: land before the slots are reused below)
  const size_t slab_id = (size_t)prob * a.nsplit + zsplit;
  float* slab = a.slab + slab_id * a.Cnw * a.Kw;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = n0 + wn * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    slab[(size_t)row * a.Kw + k0 + wk * 32 + l31] = acc[r];
  }
  if (want_bias) {  // row lanes x 16 column quads -> 64 column sums of this row split
    __syncthreads();
    f32x4* red = reinterpret_cast<f32x4*>(&sD[0][0]);
    constexpr int NR = WIDE ? 32 : 16;  // row lanes
    if constexpr (WIDE) { red[r0 * 16 + q] = bsum; red[r0 * 16 + 8 + q] = bsum1; }
    else red[r0 * 16 + q] = bsum;
    __syncthreads();
    if (tid < 16) {
      f32x4 t = red[tid];
#pragma unroll
      for (int r = 1; r < NR; ++r) t += red[r * 16 + tid];
      *reinterpret_cast<f32x4*>(a.bslab + slab_id * a.Cnw + n0 + 4 * tid) = t;
    }
  }
}

// ---------------------------------------------------------------------------
// bf16 weight gradient of 3x3 / stride 1 / pad 1 convs with 64 output columns, on WHOLE IMAGE ROWS (round 3).
// wgrad_kernel above gathers one (tap, channel) k-tile per workgroup: every tap re-reads the same x pixels and every k-tile
// re-reads the dy tile -- 16 FLOP per byte pulled through the L2s, and with bf16 MFMAs (16x the fp32 rate) ESRGAN's 207
// dense-block problems per step (32 GB of reads) ran at the speed of that traffic: 205 TFLOP/s, unmoved by a 4x longer
// chunk per barrier or by half the LDS instructions (tools/experiments/README.md).  Here a workgroup owns 32 input channels
// of one problem and ALL NINE taps: per image row it loads one new x row (the window of three rows rolls through four LDS
// slots, zero columns left and right) and one dy row, rounds them to bf16 as they arrive, and multiplies
// dy[row]^T (64 columns) with the nine shifted views of the window -- 95 FLOP per byte.  Operands are pixel-major in LDS
// and an MFMA operand (eight consecutive PIXELS of one column) is two ds_read_b64_tr_b16; a tap is an address offset.
// Wave (wn, th): output-column half wn, taps 0..4 (th = 0) or 5..8 (th = 1): 5 / 4 accumulators of 32 columns x 32 channels.
// Rows outside the image are skipped tap-wise (the slots hold the neighbouring image's rows).  The slab layout is
// wgrad_kernel's ([n][tap * Ck + channel]), so wgrad_reduce_kernel, the pairs and the scales work unchanged.
// ---------------------------------------------------------------------------
template <int WPX>
__global__ __launch_bounds__(256) void wgrad_rows_bf16_kernel(const WMulti mp) {
  const WArgs& a = mp.a;
  typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
  typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  typedef s16x4 __attribute__((address_space(3))) * lds_s16x4;
  constexpr int XPS = 64, XROW = (WPX + 2) * XPS;  // window: bytes per pixel (32 channels), per row (one zero pixel each side)
  constexpr int DPS = 192, DROW = WPX * DPS;       // dy: bytes per pixel (64 columns + pad: see wgrad_kernel), per row
  constexpr int XR = (WPX * 8 + 255) / 256, DR = (WPX * 16 + 255) / 256, KS = WPX / 16;
  __shared__ __attribute__((aligned(16))) unsigned char sX[5 * XROW];  // four window slots + a row of zeros (slot 4)
  __shared__ __attribute__((aligned(16))) unsigned char sD[2 * DROW > 4096 ? 2 * DROW : 4096];
  const int groups = a.Ck >> 5;
  int wi;
  {  // XCD-contiguous work order (see wgrad_kernel): the channel groups of one (problem, row split) share their dy rows
    const int G = (int)gridDim.x, b = (int)blockIdx.x, xcd = b & 7, slot = b >> 3, q = G >> 3, r = G & 7;
    wi = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
  }
  const int cg = srx_uniform(wi % groups), rest = wi / groups;
  const int prob = srx_uniform(rest % a.nprob), zsplit = srx_uniform(rest / a.nprob);
  const int tid = threadIdx.x, lane = tid & 63, wave = srx_uniform(tid >> 6);
  const int h = lane >> 5, l31 = lane & 31, wn = wave & 1, th = wave >> 1;
  const int rbeg = zsplit * a.rows_per_split / WPX;
  const int rend = min(a.M, (zsplit + 1) * a.rows_per_split) / WPX;  // global image rows [rbeg, rend)
  const int totrows = a.N * a.Hi;
  const __amdgpu_buffer_rsrc_t rx_ = srx_rsrc(mp.x[prob], a.in_bytes), rd_ = srx_rsrc(mp.dy[prob], a.dy_bytes);
  const bool want_bias = a.bslab != nullptr && cg == 0;  // workgroup-uniform
  f32x4 bsum = {0.f, 0.f, 0.f, 0.f};

  auto xload = [&](int gr, f32x4 (&v)[XR]) {
#pragma unroll
    for (int u = 0; u < XR; ++u) {
      const int idx = u * 256 + tid, px = idx >> 3, quad = idx & 7;
      const bool ok = idx < WPX * 8 && (unsigned)gr < (unsigned)totrows;
      v[u] = srx_bload(rx_, ok ? 4u * (unsigned)((gr * WPX + px) * a.Ci + 32 * cg + 4 * quad) : 0xffffffffu, 0);
    }
  };
  auto xstore = [&](int gr, const f32x4 (&v)[XR]) {
#pragma unroll
    for (int u = 0; u < XR; ++u) {
      const int idx = u * 256 + tid, px = idx >> 3, quad = idx & 7;
      if (idx >= WPX * 8) continue;
      const bf16x4 pk = {(__bf16)v[u][0], (__bf16)v[u][1], (__bf16)v[u][2], (__bf16)v[u][3]};
      *reinterpret_cast<bf16x4*>(sX + (gr & 3) * XROW + (px + 1) * XPS + 8 * quad) = pk;
    }
  };
  auto dload = [&](int gr, f32x4 (&v)[DR]) {
#pragma unroll
    for (int u = 0; u < DR; ++u) {
      const int idx = u * 256 + tid, px = idx >> 4, quad = idx & 15;
      const bool ok = idx < WPX * 16 && (unsigned)gr < (unsigned)totrows;
      v[u] = srx_bload(rd_, ok ? 4u * (unsigned)((gr * WPX + px) * a.Cd + 4 * quad) : 0xffffffffu, 0);
    }
  };
  auto dstore = [&](int gr, const f32x4 (&v)[DR]) {
#pragma unroll
    for (int u = 0; u < DR; ++u) {
      const int idx = u * 256 + tid, px = idx >> 4, quad = idx & 15;
      if (idx >= WPX * 16) continue;
      if (want_bias && gr < rend) bsum += v[u];  // (fp32 values, whatever the product precision)
      const bf16x4 pk = {(__bf16)v[u][0], (__bf16)v[u][1], (__bf16)v[u][2], (__bf16)v[u][3]};
      *reinterpret_cast<bf16x4*>(sD + (gr & 1) * DROW + px * DPS + 8 * quad) = pk;
    }
  };

  f32x16 acc[5];
#pragma unroll
  for (int t = 0; t < 5; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const int li = lane & 15, colh = 16 * ((lane >> 4) & 1) + 4 * (li & 3), rq = li >> 2;

  // taps T0 .. T0 + NT - 1 of output row gr
  auto compute = [&](int gr, auto t0_c, auto nt_c) {
    constexpr int T0 = decltype(t0_c)::value, NT = decltype(nt_c)::value;
    const int ih = gr % a.Hi;
    const unsigned char* dbase = sD + (gr & 1) * DROW + (8 * h + rq) * DPS + 2 * (32 * wn + colh);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const s16x4 d0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(dbase + (16 * s) * DPS));
      const s16x4 d1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(dbase + (16 * s + 4) * DPS));
      const s16x8 fd = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
#pragma unroll
      for (int ti = 0; ti < NT; ++ti) {
        constexpr int dummy = 0; (void)dummy;
        const int t = T0 + ti, ty = t / 3 - 1, tx = t % 3 - 1;
        // (wave-uniform) the row above / below lies outside the image: the tap multiplies the row of zeros.  Branch-free on
        // purpose -- with a `continue` here hipcc kept the five accumulators in different AGPRs on the two paths and moved
        // them at every join (16 v_accvgpr_mov per accumulator and row: 20 VALU instructions per MFMA, profiles/r04_pmc_esrgan.txt)
        const int slot = (unsigned)(ih + ty) < (unsigned)a.Hi ? ((gr + ty) & 3) : 4;
        const unsigned char* xb = sX + slot * XROW + (16 * s + 8 * h + rq + tx + 1) * XPS + 2 * colh;
        const s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(xb));
        const s16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(xb + 4 * XPS));
        const s16x8 fx = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
        acc[ti] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fd), __builtin_bit_cast(bf16x8, fx), acc[ti], 0, 0, 0);
      }
    }
  };

  // the row of zeros; zero columns left and right of every window slot
  if (tid < XROW / 16) *reinterpret_cast<f32x4*>(sX + 4 * XROW + 16 * tid) = f32x4{0.f, 0.f, 0.f, 0.f};
  if (tid < 32) {
    const int slot = tid >> 3, side = (tid >> 2) & 1, part = tid & 3;
    *reinterpret_cast<f32x4*>(sX + slot * XROW + (side ? (WPX + 1) * XPS : 0) + 16 * part) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  f32x4 xa[XR], xb2[XR], xc[XR], da[DR];
  xload(rbeg - 1, xa);
  xload(rbeg, xb2);
  xload(rbeg + 1, xc);
  dload(rbeg, da);
  xstore(rbeg - 1, xa);
  xstore(rbeg, xb2);
  xstore(rbeg + 1, xc);
  dstore(rbeg, da);
  xload(rbeg + 2, xa);
  dload(rbeg + 1, da);
  // one copy of the row loop per tap range (th is wave-uniform): with the choice INSIDE the loop the two paths kept the
  // accumulators in different AGPRs and every row paid 80 v_accvgpr_mov to bring them back together
  auto rows = [&](auto t0_c, auto nt_c) {
    for (int gr = rbeg; gr < rend; ++gr) {
      __syncthreads();  // rows gr - 1 .. gr + 1 and dy row gr are in LDS; the slots of x row gr - 2 and dy row gr - 1 are free
      xstore(gr + 2, xa);
      dstore(gr + 1, da);
      xload(gr + 3, xa);
      dload(gr + 2, da);
      compute(gr, t0_c, nt_c);
    }
  };
  if (th == 0) rows(std::integral_constant<int, 0>{}, std::integral_constant<int, 5>{});
  else rows(std::integral_constant<int, 5>{}, std::integral_constant<int, 4>{});
  const size_t slab_id = (size_t)prob * a.nsplit + zsplit;
  float* slab = a.slab + slab_id * a.Cnw * a.Kw;
#pragma unroll
  for (int ti = 0; ti < 5; ++ti) {
    const int t = 5 * th + ti;
    if (t >= 9) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wn * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      slab[(size_t)row * a.Kw + t * a.Ck + 32 * cg + l31] = acc[ti][r];
    }
  }
  if (want_bias) {  // 16 pixel lanes x 16 column quads -> 64 column sums of this row split
    __syncthreads();  // (every wave is done with the dy slots)
    f32x4* red = reinterpret_cast<f32x4*>(sD);
    red[tid] = bsum;
    __syncthreads();
    if (tid < 16) {
      f32x4 t = red[tid];
#pragma unroll
      for (int r = 1; r < 16; ++r) t += red[r * 16 + tid];
      *reinterpret_cast<f32x4*>(a.bslab + slab_id * a.Cnw + 4 * tid) = t;
    }
  }
}

// slab sums -> OIHW gradient.  blockIdx.y = output; its `nslab` slabs (row splits x segments) are consecutive.
__global__ void wgrad_reduce_kernel(const float* __restrict__ slab_all, int nslab, int Cnw, int Kw, int K, int Ck,
                                    int Cout, int Cin, int KH, int KW, int shuffle_cps, const WReduce outs,
                                    int accumulate, const float* __restrict__ bslab_all) {
  const int o = blockIdx.y;
  float* __restrict__ dw = outs.dw[o];
  float* __restrict__ db = outs.db[o];
  const float* __restrict__ slab = slab_all + (size_t)o * nslab * Cnw * Kw;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int rows_lo = outs.rows_lo;  // 0: one conv per output
  if (idx < Cout) {  // bias gradient: the slabs' column sums (the grid has >= Cout threads)
    float* __restrict__ dbp = (rows_lo && idx >= rows_lo) ? outs.db_hi[o] : db;
    if (dbp) {
      const float* __restrict__ bslab = bslab_all + (size_t)o * nslab * Cnw;
      float s = 0.f;
      for (int z = 0; z < nslab; ++z) s += bslab[(size_t)z * Cnw + idx];
      s *= outs.scale[o];
      int bi = (rows_lo && idx >= rows_lo) ? (int)idx - rows_lo : (int)idx;
      // PixelShuffle layers: the slab's columns are in packed (sub-pixel, channel) order, the bias in the conv's own
      if (shuffle_cps) { const int ij = (int)idx / shuffle_cps, cc = (int)idx - ij * shuffle_cps; bi = cc * 4 + ij; }
      dbp[bi] = accumulate ? dbp[bi] + s : s;
    }
  }
  if (idx >= (int64_t)Cout * K) return;
  const int srow = (int)(idx / K);  // row of the slab
  const int k = (int)(idx - (int64_t)srow * K);
  const int tap = k / Ck, ci = k - tap * Ck;
  int np = srow;                    // output channel of the conv the row belongs to
  if (rows_lo) {  // (no PixelShuffle on paired problems)
    if (np < rows_lo) { Cin = outs.cin_lo; } else { np -= rows_lo; dw = outs.dw_hi[o]; }
  }
  if (ci >= Cin) return;
  const float* sp = slab + (size_t)srow * Kw + k;
  const size_t zs = (size_t)Cnw * Kw;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int z = 0;
  for (; z + 3 < nslab; z += 4) {
    s0 += sp[(size_t)z * zs];
    s1 += sp[(size_t)(z + 1) * zs];
    s2 += sp[(size_t)(z + 2) * zs];
    s3 += sp[(size_t)(z + 3) * zs];
  }
  for (; z < nslab; ++z) s0 += sp[(size_t)z * zs];
  const float s = ((s0 + s1) + (s2 + s3)) * outs.scale[o];
  int co = np;
  if (shuffle_cps) { const int ij = np / shuffle_cps, cc = np - ij * shuffle_cps; co = cc * 4 + ij; }
  const int kh = tap / KW, kw = tap - kh * KW;
  float* op = dw + (((size_t)co * Cin + ci) * KH + kh) * KW + kw;
  *op = accumulate ? *op + s : s;
}

// The same reduction, one workgroup per slab ROW (round 5): the row's K sums are formed with coalesced reads ([k] contiguous in every
// slab), parked in LDS, and written out in the gradient's own order -- OIHW, (ci, kh, kw) contiguous per output channel --
// so the stores are coalesced too.  The kernel above writes 4-byte elements 36 bytes apart (k = (tap, ci) -> address
// (ci * 9 + tap)): 28 us per launch on ESRGAN's grouped gradients for 50 MB of traffic (1.8 TB/s).  Same sums in the same
// order: bit-identical results.  blockIdx.x = slab row, blockIdx.y = output; dynamic LDS: K floats.
__global__ __launch_bounds__(256) void wgrad_reduce_rows_kernel(const float* __restrict__ slab_all, int nslab, int Cnw, int Kw, int K, int Ck,
                                                                int Cout, int Cin, int KH, int KW, int shuffle_cps, const WReduce outs,
                                                                int accumulate, const float* __restrict__ bslab_all) {
  extern __shared__ __attribute__((aligned(16))) float rsum[];
  const int o = blockIdx.y, srow = blockIdx.x, tid = threadIdx.x;
  const float* __restrict__ slab = slab_all + (size_t)o * nslab * Cnw * Kw + (size_t)srow * Kw;
  const size_t zs = (size_t)Cnw * Kw;
  const float scale = outs.scale[o];
  const int rows_lo = outs.rows_lo;  // 0: one conv per output
  float* __restrict__ dw = outs.dw[o];
  float* __restrict__ dbp = outs.db[o];
  int np = srow;
  if (rows_lo) {  // (no PixelShuffle on paired problems)
    if (np < rows_lo) { Cin = outs.cin_lo; } else { np -= rows_lo; dw = outs.dw_hi[o]; dbp = outs.db_hi[o]; }
  }
  int co = np;
  if (shuffle_cps) { const int ij = np / shuffle_cps, cc = np - ij * shuffle_cps; co = cc * 4 + ij; }
  const int T = KH * KW, nE = Cin * T;
  float* __restrict__ orow = dw + (size_t)co * Cin * T;
  // round 6: a workgroup lives for three dependent round trips (slab rows, then -- accumulating -- the gradient's old values, then
  // the bias slabs one after the other in thread 0) and moves ~17 KB; the old values and the bias column are requested FIRST, next
  // to the slab rows.  Same sums in the same order.
  constexpr int PRE = 8;  // old values held in registers (Cin * T <= 2048: every layer of the two models)
  float oldv[PRE];
#pragma unroll
  for (int i = 0; i < PRE; ++i) {
    const int e = tid + 256 * i;
    oldv[i] = (accumulate && e < nE) ? orow[e] : 0.f;
  }
  // bias gradient of this row: the slabs' column sums, one slab per lane of the last wave (summed in slab order below)
  float bpart = 0.f;
  const bool bias_wave = dbp != nullptr && tid >= 192;
  if (bias_wave && nslab <= 64 && tid - 192 < nslab) bpart = bslab_all[((size_t)o * nslab + (tid - 192)) * Cnw + srow];
  // (four consecutive k per thread, 16-byte loads: K and the slab pitch Kw are multiples of 4; with one float per thread the pass was
  // bound by the few bytes it kept in flight, not by its stores: 27 us per launch either way)
  for (int k = 4 * tid; k < K; k += 1024) {
    const float* sp = slab + k;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
    int z = 0;
    for (; z + 3 < nslab; z += 4) {
      s0 += *reinterpret_cast<const f32x4*>(sp + (size_t)z * zs);
      s1 += *reinterpret_cast<const f32x4*>(sp + (size_t)(z + 1) * zs);
      s2 += *reinterpret_cast<const f32x4*>(sp + (size_t)(z + 2) * zs);
      s3 += *reinterpret_cast<const f32x4*>(sp + (size_t)(z + 3) * zs);
    }
    for (; z < nslab; ++z) s0 += *reinterpret_cast<const f32x4*>(sp + (size_t)z * zs);
    *reinterpret_cast<f32x4*>(rsum + k) = ((s0 + s1) + (s2 + s3)) * scale;
  }
  if (bias_wave) {
    float s = 0.f;
    if (nslab <= 64) {
      for (int z = 0; z < nslab; ++z) s += __shfl(bpart, z, 64);
    } else {
      const float* __restrict__ bslab = bslab_all + (size_t)o * nslab * Cnw + srow;
      for (int z = 0; z < nslab; ++z) s += bslab[(size_t)z * Cnw];
    }
    if (tid == 192) {
      s *= scale;
      int bi = np;
      if (shuffle_cps) { const int ij = srow / shuffle_cps, cc = srow - ij * shuffle_cps; bi = cc * 4 + ij; }
      dbp[bi] = accumulate ? dbp[bi] + s : s;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < PRE; ++i) {
    const int e = tid + 256 * i;
    if (e < nE) {
      const int ci = e / T, tap = e - ci * T;
      const float v = rsum[tap * Ck + ci];
      orow[e] = accumulate ? oldv[i] + v : v;
    }
  }
  for (int e = tid + 256 * PRE; e < nE; e += 256) {
    const int ci = e / T, tap = e - ci * T;
    const float v = rsum[tap * Ck + ci];
    orow[e] = accumulate ? orow[e] + v : v;
  }
}

}  // namespace

// Row splits of a (group of) weight-gradient problem(s): the slabs cost a write + a read each, and workgroup counts just
// above a whole round of resident workgroups leave a nearly empty last round.  Calibrated on the SRGAN layer shapes
// (bf16: tools/bench_kernels.py --graph, round 1; fp32: tools/wgrad_sweep.sh, round 3); SRX_WGRAD_NSPLIT overrides for experiments.
static int wgrad_nsplit(int M, int64_t tiles, int nprob, int Cnw, int Kw, int precision) {
  const int cus = srx_plan_cus();
  const int max_by_rows = (int)srx_cdiv(M, 128);  // at least 128 rows per split
  int nsplit = 1;
  float best_cost = 1e30f;
  for (int ns = 1; ns <= 64 && ns <= max_by_rows; ++ns) {
    const int rps = (int)srx_roundup(srx_cdiv(M, ns), 32);
    if ((int)srx_cdiv(M, rps) != ns) continue;  // not reachable after rounding to whole chunks
    float cost;
    if (precision == 0) {
      // fp32 (round 3, least-squares fit of 57 in-graph timings of the SRGAN layer shapes, `tools/wgrad_sweep.sh`, rms 4.7 us):
      // three workgroups are resident per CU (VGPRs); a round of three takes 1.70 us per 32-row chunk, a last round of two
      // 1.18 us, of one 0.63 us -- so a workgroup count just ABOVE a multiple of three per CU pays a whole extra round
      // (73728 x 128 x 576: 111 us with 42 splits = 2.95 per CU, 146 us with 43) -- plus 3.5 chunks of fill per round.
      const int w = (int)srx_cdiv(tiles * nprob * ns, cus), f = w / 3, r = w - 3 * f;
      cost = (rps / 32 + 3.5f) * (f * 1.696f + (r == 1 ? 0.633f : r == 2 ? 1.177f : 0.f)) + (float)nprob * ns * Cnw * Kw * 8.0f / 50.0e6f;
    } else {
      const int L = (int)srx_cdiv(tiles * nprob * ns, cus);
      const float hide = L >= 4 ? 0.65f : (L == 3 ? 0.7f : (L == 2 ? 0.8f : 1.0f));
      cost = 1.07f * L * (rps / 32 + 6) * hide + (float)nprob * ns * Cnw * Kw * 8.0f / 3.0e6f;
    }
    if (cost < best_cost) { best_cost = cost; nsplit = ns; }
  }
  if (const int v = conv_force().wg[1].load(std::memory_order_relaxed); v > 0) {  // srx_wgrad_force / SRX_WGRAD_NSPLIT
    const int rps = (int)srx_roundup(srx_cdiv(M, v), 32);
    if (v > max_by_rows || (int)srx_cdiv(M, rps) != v) {
      srx_set_error("conv2d_bwd_weight: forced %d row splits refused: %d rows split into whole 32-row chunks of at least 128 rows "
                    "give %d splits", v, M, v > max_by_rows ? max_by_rows : (int)srx_cdiv(M, rps));
      return -1;
    }
    nsplit = v;
  }
  const int rps = (int)srx_roundup(srx_cdiv(M, nsplit), 32);
  return (int)srx_cdiv(M, rps);
}

// bf16 products, 3x3 / stride 1 / pad 1, 64 output columns, whole 32-channel groups, image rows of 16 or 32 pixels (ESRGAN's
// dense blocks at the training crop size): the image-row kernel (wgrad_rows_bf16_kernel)
static bool wgrad_rows_ok(const srx_conv2d_t* d) {
  // (srx_wgrad_force_kernels(., 0, .) / SRX_NO_WGRAD_ROWS: such layers run wgrad_kernel<1>)
  if (conv_force().wk[1].load(std::memory_order_relaxed) == 0 || !d->precision || d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad != 1 || d->shuffle || d->up == 2) return false;
  return d->Cout == 64 && srx_roundup(d->Cin, 4) % 32 == 0 && (d->W == 32 || d->W == 16);
}
// row splits of the image-row kernel: workgroups = channel groups x problems x splits, four resident per CU.  -1: a forced split
// (srx_wgrad_force / SRX_WGRAD_ROWS_NSPLIT, in image rows) the rows cannot take, message set
static int wgrad_rows_nsplit(const srx_conv2d_t* d, int nprob) {
  const int cus = srx_plan_cus();
  const int groups = (int)srx_roundup(d->Cin, 4) / 32, rows = d->N * d->H;
  int best = 1;
  float best_cost = 1e30f;
  for (int ns = 1; ns <= 32 && ns <= rows; ++ns) {
    const int rps = (int)srx_cdiv(rows, ns);
    if ((int)srx_cdiv(rows, rps) != ns) continue;
    const int rounds = (int)srx_cdiv((int64_t)groups * nprob * ns, 4 * cus);
    const float cost = rounds * (rps + 8.0f) + 0.25f * ns;  // (+ the slab reduction grows with the splits)
    if (cost < best_cost) { best_cost = cost; best = ns; }
  }
  if (const int v = conv_force().wg_rows.load(std::memory_order_relaxed); v > 0) {
    if (v > rows || (int)srx_cdiv(rows, srx_cdiv(rows, v)) != v) {
      srx_set_error("conv2d_bwd_weight: forced %d row splits refused: %d image rows split into whole rows give %d splits", v, rows,
                    v > rows ? rows : (int)srx_cdiv(rows, srx_cdiv(rows, v)));
      return -1;
    }
    best = v;
  }
  const int rps = (int)srx_cdiv(rows, best);
  return (int)srx_cdiv(rows, rps);
}

// ---- launch plan.  The ONE place that cuts it: srx_wgrad_plan, the workspace query and wgrad_multi_impl read wgrad_plan and nothing
// else, so what the query reports is what the call launches. ----
enum { WK_F32 = 0, WK_DMA = 1, WK_DMA_WIDE = 2, WK_DMA_LIN = 3, WK_BF16 = 4, WK_ROWS32 = 5, WK_ROWS16 = 6, WK_THIN = 7 };
struct WgradPlan {
  int kernel;          // WK_*: wgrad_kernel<0>, wgrad_dma_kernel<0, 0> / <1, 0> (WIDE) / <1, 1> (WIDE + LIN: offsets linear in the row, validity
                       // from a per-workgroup bit table, see wgrad_dma_kernel), wgrad_kernel<1>, wgrad_rows_bf16_kernel<32> / <16>
  int nsplit;          // row splits = slabs per problem
  int rows_per_split;  // output pixels per split (the image-row kernel: whole image rows)
  int reduce;          // 0 wgrad_reduce_kernel, 1 wgrad_reduce_rows_kernel
  int workgroups;      // of the slab kernel
  int Cnw, Kw;         // slab extents: output columns and K in whole tiles of 64
};
// `d`: a checked descriptor without a fused upsample (up = 2: plan upsampled_desc(d)) whose gradient is not thin.hip's.  Returns SRX_OK,
// or SRX_E_UNSUPPORTED for a forced row split the rows cannot take (message set).
static int wgrad_plan(const srx_conv2d_t* d, int nprob, WgradPlan& p) {
  const Geo g = fwd_geo(d);
  const ConvForce& f = conv_force();
  p.Cnw = (int)srx_roundup(d->Cout, 64);
  p.Kw = (int)srx_roundup(g.K, 64);
  const int M = d->N * g.Ho * g.Wo;
  const int64_t tiles = (int64_t)(p.Kw / 64) * (p.Cnw / 64);
  if (wgrad_rows_ok(d)) {
    p.nsplit = wgrad_rows_nsplit(d, nprob);
    if (p.nsplit < 0) return SRX_E_UNSUPPORTED;
    p.kernel = d->W == 32 ? WK_ROWS32 : WK_ROWS16;
    p.rows_per_split = (int)srx_cdiv(d->N * d->H, p.nsplit) * d->W;
    p.workgroups = (g.Ck / 32) * nprob * p.nsplit;
  } else {
    p.nsplit = wgrad_nsplit(M, tiles, nprob, p.Cnw, p.Kw, d->precision);
    if (p.nsplit < 0) return SRX_E_UNSUPPORTED;
    p.rows_per_split = (int)srx_roundup(srx_cdiv(M, p.nsplit), 32);
    p.workgroups = (int)(tiles * nprob * p.nsplit);
    if (d->precision) {
      p.kernel = WK_BF16;
    } else if (f.wk[0].load(std::memory_order_relaxed) == 0) {  // srx_wgrad_force_kernels(0, ., .) / SRX_NO_WGRAD_DMA
      p.kernel = WK_F32;
    } else {
      p.kernel = WK_DMA;
      const int Cdv = bwd_ck(d);
      if (g.Ck % 64 == 0 && Cdv % 64 == 0 && (!g.cps || g.cps % 64 == 0)) {
        const size_t in_bytes = (size_t)d->N * d->H * d->W * d->Cin_s * sizeof(float);
        const size_t dy_bytes = (size_t)M * (d->shuffle ? 4 : 1) * d->Cout_s * sizeof(float);
        const bool lin = f.wg[0].load(std::memory_order_relaxed) != 0 && d->stride == 1 && d->H == g.Ho && d->W == g.Wo && !g.cps &&
                         g.K % 64 == 0 && p.rows_per_split / 32 + 3 <= WG_MASKW && in_bytes < 0xfff00000ull && dy_bytes < 0xfff00000ull;
        p.kernel = lin ? WK_DMA_LIN : WK_DMA_WIDE;  // (srx_wgrad_force(0, .) turns LIN off)
      }
    }
  }
  // wgrad_reduce_rows_kernel parks a slab row's K sums in LDS; srx_wgrad_force_kernels(., ., 0) / SRX_OLD_WGRAD_REDUCE: never
  p.reduce = (f.wk[2].load(std::memory_order_relaxed) == 0 || (size_t)g.K * sizeof(float) > 48 * 1024) ? 0 : 1;
  return SRX_OK;
}

extern "C" int srx_wgrad_plan(const srx_conv2d_t* d, int nprob, int per_out, int* out) {
  if (int rc = check_desc(d)) return rc;
  SRX_REQUIRE(out && nprob >= 1 && nprob <= WG_MAXP && per_out >= 1 && nprob % per_out == 0,
              "wgrad_plan: a result array, 1..%d problems, a whole number of outputs", WG_MAXP);
  SRX_REQUIRE(d->precision != 3, "conv2d: precision 3 (fp16 products) is forward-only");
  if (d->up == 2) { const srx_conv2d_t h = upsampled_desc(d); return srx_wgrad_plan(&h, nprob, per_out, out); }
  for (int i = 0; i < 6; ++i) out[i] = 0;
  if (srx_thin_wgrad_applicable(d)) { out[0] = WK_THIN; return SRX_OK; }  // (thin.hip plans it: srx_thin_plan(d, 2, .))
  WgradPlan p;
  if (int rc = wgrad_plan(d, nprob, p)) return rc;
  out[0] = p.kernel; out[1] = p.nsplit; out[2] = p.rows_per_split; out[3] = p.reduce; out[4] = p.workgroups; out[5] = p.nsplit * per_out;
  return SRX_OK;
}

extern "C" size_t srx_conv2d_bwd_weight_multi_ws_floats(const srx_conv2d_t* d, int nprob) {
  if (check_desc(d) || nprob < 1 || nprob > WG_MAXP) return 0;
  if (d->up == 2) { const srx_conv2d_t h = upsampled_desc(d); return nprob * upsampled_floats(d) + srx_conv2d_bwd_weight_multi_ws_floats(&h, nprob); }
  if (srx_thin_wgrad_applicable(d))  // (one call per problem) + the column-sum scratch of an optional bias gradient
    return srx_thin_wgrad_ws_floats(d) + srx_colsum_ws_floats((int64_t)d->N * d->H * d->W, d->Cout);
  WgradPlan p;
  if (wgrad_plan(d, nprob, p)) return 0;  // (a refused forced split: the call reports it)
  return (size_t)p.Cnw * ((size_t)p.Kw + 1) * (size_t)p.nsplit * nprob;  // one slab (+ one bias row) per problem and row split
}

extern "C" size_t srx_conv2d_bwd_weight_ws_floats(const srx_conv2d_t* d) { return srx_conv2d_bwd_weight_multi_ws_floats(d, 1); }

static int wgrad_multi_impl(const srx_conv2d_t* d, int nprob, int per_out, const float* const* xs, const float* const* dys,
                            float* const* dws, int accumulate, float* const* dbs, const float* out_scales,
                            float* const* dws_hi, float* const* dbs_hi, int cin_lo, float* ws, size_t ws_floats,
                            void* stream) {
  if (int rc = check_desc(d)) return rc;
  SRX_REQUIRE(d->precision != 3, "conv2d: precision 3 (fp16 products) is forward-only");
  SRX_REQUIRE(nprob >= 1 && nprob <= WG_MAXP && per_out >= 1 && nprob % per_out == 0,
              "conv2d_bwd_weight_multi: 1..%d problems, a whole number of outputs", WG_MAXP);
  SRX_REQUIRE(xs && dys && dws && ws, "conv2d_bwd_weight: null pointer");
  SRX_REQUIRE(small_enough(d), "conv2d_bwd_weight: more than 2^24 pixels or 4 GiB of input per problem (the weight-gradient kernels "
                               "keep 32-bit tensor offsets: training crops, not whole frames)");
  if (d->up == 2) {
    const srx_conv2d_t h = upsampled_desc(d);
    const size_t tmp = upsampled_floats(d);
    SRX_REQUIRE(ws_floats >= nprob * tmp + srx_conv2d_bwd_weight_multi_ws_floats(&h, nprob), "conv2d_bwd_weight: workspace too small for up = 2");
    const float* up_x[WG_MAXP];
    for (int i = 0; i < nprob; ++i) {
      SRX_REQUIRE(xs[i], "conv2d_bwd_weight: null tensor in problem %d", i);
      up_x[i] = ws + (size_t)i * tmp;
      if (int rc = srx_upsample_nearest2x_fwd(xs[i], ws + (size_t)i * tmp, d->N, d->H, d->W, d->Cin_s, stream)) return rc;
    }
    return wgrad_multi_impl(&h, nprob, per_out, up_x, dys, dws, accumulate, dbs, out_scales, nullptr, nullptr, 0,
                            ws + nprob * tmp, ws_floats - nprob * tmp, stream);
  }
  const int nout = nprob / per_out;
  bool any_db = false;
  for (int i = 0; i < nprob; ++i) SRX_REQUIRE(xs[i] && dys[i], "conv2d_bwd_weight: null tensor in problem %d", i);
  for (int o = 0; o < nout; ++o) {
    SRX_REQUIRE(dws[o] && (!dws_hi || dws_hi[o]), "conv2d_bwd_weight: null gradient pointer for output %d", o);
    any_db |= (dbs && dbs[o]) || (dbs_hi && dbs_hi[o]);
  }
  hipStream_t st = srx_stream(stream);
  if (srx_thin_wgrad_applicable(d)) {  // 3-channel layers: their own kernel, one problem at a time
    for (int o = 0; out_scales && o < nout; ++o)
      if (out_scales[o] != 1.f) SRX_FAIL(SRX_E_UNSUPPORTED, "conv2d_bwd_weight: output scales on a 3-channel layer");
    const size_t thin_ws = srx_thin_wgrad_ws_floats(d);
    const int64_t m = (int64_t)d->N * d->H * d->W;  // thin layers are stride 1, same size
    for (int i = 0; i < nprob; ++i) {
      const int o = i / per_out;
      const int acc = accumulate || (i % per_out) > 0;
      if (int rc = srx_thin_wgrad(d, xs[i], dys[i], dws[o], acc, ws, ws_floats, st)) return rc;
      if (!(dbs && dbs[o])) continue;
      SRX_REQUIRE(ws_floats >= thin_ws + srx_colsum_ws_floats(m, d->Cout), "conv2d_bwd_weight: workspace too small");
      if (int rc = srx_colsum(dys[i], dbs[o], m, d->Cout, d->Cout_s, acc, ws + thin_ws, ws_floats - thin_ws, stream)) return rc;
    }
    return SRX_OK;
  }
  const Geo g = fwd_geo(d);
  WMulti mp{};
  WArgs& a = mp.a;
  a.in = xs[0]; a.dy = dys[0]; a.slab = ws;
  a.N = d->N; a.Hi = d->H; a.Wi = d->W; a.Ci = d->Cin_s;
  a.Hm = g.Ho; a.Wm = g.Wo; a.HmWm = g.Ho * g.Wo; a.M = d->N * g.Ho * g.Wo;
  a.inv_HmWm = 1.0f / (float)a.HmWm; a.inv_Wm = 1.0f / (float)g.Wo;
  a.in_stride = d->stride; a.nth = d->KH; a.ntw = d->KW; a.dh0 = -d->pad; a.dw0 = -d->pad;
  a.Ck = g.Ck; a.K = g.K;
  a.Kw = (int)srx_roundup(g.K, 64);
  a.Cnw = (int)srx_roundup(d->Cout, 64);
  a.Cd = d->Cout_s;
  a.dy_shuffle = g.cps;
  a.Cdv = bwd_ck(d);
  a.ktiles = a.Kw / 64;
  const size_t dyb = (size_t)d->N * g.Ho * g.Wo * (d->shuffle ? 4 : 1) * d->Cout_s * sizeof(float);
  SRX_REQUIRE(dyb < 0xfffffff0ull, "conv2d_bwd_weight: gradient tensor above 4 GiB; tile the image");
  a.in_bytes = (unsigned)((size_t)d->N * d->H * d->W * d->Cin_s * sizeof(float));
  a.dy_bytes = (unsigned)dyb;
  {
    const int s = d->stride, s_r = 32 / a.Wm, s_n = s_r / a.Hm;
    a.s_c = 32 % a.Wm; a.s_rm = s_r % a.Hm;
    a.dX0 = ((s_n * a.Hi + a.s_rm * s) * a.Wi + a.s_c * s) * a.Ci;
    a.dX1 = (s * a.Wi - a.Wm * s) * a.Ci;
    a.dX2 = (a.Hi - a.Hm * s) * a.Wi * a.Ci;
    if (a.dy_shuffle) {
      a.dD0 = ((s_n * 2 * a.Hm + 2 * a.s_rm) * (2 * a.Wm) + 2 * a.s_c) * a.Cd;
      a.dD1 = 2 * a.Wm * a.Cd;
    } else {
      a.dD0 = 32 * a.Cd;
      a.dD1 = 0;
    }
  }
  WgradPlan plan;
  if (int rc = wgrad_plan(d, nprob, plan)) return rc;  // (a refused forced split: the planner set the message)
  const bool rows_kernel = plan.kernel == WK_ROWS32 || plan.kernel == WK_ROWS16;
  const int nsplit = plan.nsplit;
  a.rows_per_split = plan.rows_per_split;
  a.nsplit = nsplit;
  a.nprob = nprob;
  const size_t nslabs = (size_t)nsplit * nprob;
  const size_t need = nslabs * a.Cnw * a.Kw + (any_db ? nslabs * a.Cnw : 0);
  if (need > ws_floats) SRX_FAIL(SRX_E_WORKSPACE, "conv2d_bwd_weight: workspace %zu < %zu floats", ws_floats, need);
  a.bslab = any_db ? ws + nslabs * a.Cnw * a.Kw : nullptr;
  WReduce outs{};
  for (int i = 0; i < nprob; ++i) { mp.x[i] = xs[i]; mp.dy[i] = dys[i]; }
  for (int o = 0; o < nout; ++o) {
    outs.dw[o] = dws[o]; outs.db[o] = dbs ? dbs[o] : nullptr; outs.scale[o] = out_scales ? out_scales[o] : 1.f;
    SRX_REQUIRE(outs.scale[o] == outs.scale[o] && outs.scale[o] - outs.scale[o] == 0.f,
                "conv2d_bwd_weight_multi_scaled: output scale %d is not finite (out_scales is a HOST array of nprob / per_out floats)", o);
    outs.dw_hi[o] = dws_hi ? dws_hi[o] : nullptr; outs.db_hi[o] = dbs_hi ? dbs_hi[o] : nullptr;
  }
  outs.rows_lo = dws_hi ? d->Cout / 2 : 0;
  outs.cin_lo = cin_lo;
  const dim3 grid((unsigned)plan.workgroups);
  const double wfl = 2.0 * a.M * d->Cout * a.K * nprob;
  char nm[112];
  if (rows_kernel) {
    if (srx_prof_on()) snprintf(nm, sizeof(nm), "wgrad_rows_bf16_kernel<%d> MxNxK=%dx%dx%d x%d", d->W, a.M, d->Cout, a.K, nprob);
    if (plan.kernel == WK_ROWS32) SRX_LAUNCH_PROF(nm, wfl, wgrad_rows_bf16_kernel<32>, grid, dim3(256), 0, st, mp);
    else SRX_LAUNCH_PROF(nm, wfl, wgrad_rows_bf16_kernel<16>, grid, dim3(256), 0, st, mp);
    SRX_CHECK_LAUNCH("wgrad_rows_bf16_kernel");
  } else {
    const int form = plan.kernel;
    if (srx_prof_on()) {
      if (form == WK_F32 || form == WK_BF16) snprintf(nm, sizeof(nm), "wgrad_kernel<%d> MxNxK=%dx%dx%d x%d", form == WK_BF16 ? 1 : 0, a.M, d->Cout, a.K, nprob);
      else snprintf(nm, sizeof(nm), "wgrad_dma_kernel<%d, %d> MxNxK=%dx%dx%d x%d", form >= WK_DMA_WIDE ? 1 : 0, form == WK_DMA_LIN ? 1 : 0, a.M, d->Cout, a.K, nprob);
    }
    if (form == WK_BF16) SRX_LAUNCH_PROF(nm, wfl, wgrad_kernel<1>, grid, dim3(256), 0, st, mp);
    else if (form == WK_F32) SRX_LAUNCH_PROF(nm, wfl, wgrad_kernel<0>, grid, dim3(256), 0, st, mp);
    else if (form == WK_DMA_LIN) SRX_LAUNCH_PROF(nm, wfl, (wgrad_dma_kernel<true, true>), grid, dim3(256), 0, st, mp);
    else if (form == WK_DMA_WIDE) SRX_LAUNCH_PROF(nm, wfl, wgrad_dma_kernel<true>, grid, dim3(256), 0, st, mp);
    else SRX_LAUNCH_PROF(nm, wfl, wgrad_dma_kernel<false>, grid, dim3(256), 0, st, mp);
    SRX_CHECK_LAUNCH("wgrad_kernel");
  }
  if (plan.reduce == 0) {
    const int64_t n = (int64_t)d->Cout * g.K;
    SRX_LAUNCH_PROF_AUX("wgrad_reduce_kernel", wgrad_reduce_kernel, dim3((unsigned)srx_cdiv(n, 256), (unsigned)nout), dim3(256), 0, st, ws,
                    nsplit * per_out, a.Cnw, a.Kw, g.K, g.Ck, d->Cout, d->Cin, d->KH, d->KW, g.cps, outs, accumulate,
                    a.bslab);
  } else {
    SRX_LAUNCH_PROF_AUX("wgrad_reduce_rows_kernel", wgrad_reduce_rows_kernel, dim3((unsigned)d->Cout, (unsigned)nout), dim3(256),
                    (size_t)g.K * sizeof(float), st, ws, nsplit * per_out, a.Cnw, a.Kw, g.K, g.Ck, d->Cout, d->Cin, d->KH, d->KW, g.cps,
                    outs, accumulate, a.bslab);
  }
  SRX_CHECK_LAUNCH("wgrad_reduce_kernel");
  return SRX_OK;
}

extern "C" int srx_conv2d_bwd_weight_multi_scaled(const srx_conv2d_t* d, int nprob, int per_out, const float* const* xs,
                                                  const float* const* dys, float* const* dws, int accumulate,
                                                  float* const* dbs, const float* out_scales, float* ws, size_t ws_floats,
                                                  void* stream) {
  return wgrad_multi_impl(d, nprob, per_out, xs, dys, dws, accumulate, dbs, out_scales, nullptr, nullptr, 0, ws, ws_floats,
                          stream);
}

extern "C" int srx_conv2d_bwd_weight_multi(const srx_conv2d_t* d, int nprob, int per_out, const float* const* xs,
                                           const float* const* dys, float* const* dws, int accumulate, float* const* dbs,
                                           float* ws, size_t ws_floats, void* stream) {
  return srx_conv2d_bwd_weight_multi_scaled(d, nprob, per_out, xs, dys, dws, accumulate, dbs, nullptr, ws, ws_floats, stream);
}

extern "C" int srx_conv2d_bwd_weight_multi_pair(const srx_conv2d_t* d, int nprob, const float* const* xs,
                                                const float* const* dys, float* const* dws_lo, float* const* dws_hi,
                                                int cin_lo, int accumulate, float* const* dbs_lo, float* const* dbs_hi,
                                                float* ws, size_t ws_floats, void* stream) {
  SRX_REQUIRE(d && dws_hi, "conv2d_bwd_weight_multi_pair: null pointer");
  SRX_REQUIRE(d->Cout % 8 == 0 && !d->shuffle && d->up != 2 && cin_lo > 0 && cin_lo <= d->Cin && !srx_thin_wgrad_applicable(d),
              "conv2d_bwd_weight_multi_pair: two convs of Cout / 2 output channels each (a multiple of 4), no PixelShuffle, "
              "no fused upsample, 0 < cin_lo <= Cin");
  SRX_REQUIRE((dbs_lo == nullptr) == (dbs_hi == nullptr), "conv2d_bwd_weight_multi_pair: bias gradients for both convs or neither");
  SRX_REQUIRE(cin_lo % 4 == 0 || cin_lo == d->Cin, "conv2d_bwd_weight_multi_pair: cin_lo must be a whole number of quads");
  return wgrad_multi_impl(d, nprob, 1, xs, dys, dws_lo, accumulate, dbs_lo, nullptr, dws_hi, dbs_hi, cin_lo, ws, ws_floats, stream);
}

extern "C" int srx_conv2d_bwd_weight(const srx_conv2d_t* d, const float* x, const float* dy, float* dw, int accumulate,
                                     float* db, float* ws, size_t ws_floats, void* stream) {
  SRX_REQUIRE(x && dy && dw && ws, "conv2d_bwd_weight: null pointer");
  return srx_conv2d_bwd_weight_multi(d, 1, 1, &x, &dy, &dw, accumulate, db ? &db : nullptr, ws, ws_floats, stream);
}
