// Weight packing for the gather-GEMM convolution (gconv.hip): OIHW weights into the k-contiguous [N_pad][K_pad] rows of the
// forward pass and of every stride-parity class of the data gradient -- per layer (srx_conv2d_pack) or for a whole model
// from a record table in one launch (srx_pack_table_*).
#include "conv_host.h"

namespace {

// ---------------------------------------------------------------------------
// weight packing
// ---------------------------------------------------------------------------
__global__ void pack_fwd_kernel(const float* __restrict__ w, float* __restrict__ p, int Cout, int Cin, int KH, int KW,
                                int Ck, int K, int Kp, int Cnp, int shuffle_cps) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)Cnp * Kp) return;
  const int np = (int)(idx / Kp), k = (int)(idx - (int64_t)np * Kp);
  float v = 0.f;
  if (np < Cout && k < K) {
    const int tap = k / Ck, ci = k - tap * Ck;
    if (ci < Cin) {
      int co = np;
      if (shuffle_cps) { const int ij = np / shuffle_cps, cc = np - ij * shuffle_cps; co = cc * 4 + ij; }
      const int kh = tap / KW, kw = tap - kh * KW;
      v = w[(((size_t)co * Cin + ci) * KH + kh) * KW + kw];
    }
  }
  p[idx] = v;
}

// one stride-parity class of the data gradient: B[ci][(th,tw,c)] = W[co(c)][ci][kh(th)][kw(tw)]
__global__ void pack_bwd_kernel(const float* __restrict__ w, float* __restrict__ p, int Cout, int Cin, int KH, int KW,
                                int stride, int pad, int ph, int pw, int dminh, int dminw, int ntw, int Ck, int K,
                                int Kp, int Cnp, int shuffle_cps) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)Cnp * Kp) return;
  const int ci = (int)(idx / Kp), k = (int)(idx - (int64_t)ci * Kp);
  float v = 0.f;
  if (ci < Cin && k < K) {
    const int tap = k / Ck, c = k - tap * Ck;
    if (c < Cout) {
      const int th = tap / ntw, tw = tap - th * ntw;
      const int kh = ph + pad - stride * (dminh + th), kw = pw + pad - stride * (dminw + tw);
      int co = c;
      if (shuffle_cps) { const int ij = c / shuffle_cps, cc = c - ij * shuffle_cps; co = cc * 4 + ij; }
      v = w[(((size_t)co * Cin + ci) * KH + kh) * KW + kw];
    }
  }
  p[idx] = v;
}

// forward pack and every data-gradient class in ONE launch (blockIdx.y = segment): a repack after each
// optimiser step used to be 1 + stride^2 tiny launches per layer, ~130 per train step
struct PackSeg { float* dst; int rows, K, Kp, Ck, bwd, ph, pw, dminh, dminw, ntw; };
struct PackArgs {
  const float* w;
  int Cout, Cin, KH, KW, stride, pad, cps, nseg;
  PackSeg seg[17];
};
__global__ void pack_all_kernel(const PackArgs a) {
  const PackSeg sg = a.seg[blockIdx.y];
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)sg.rows * sg.Kp) return;
  const int row = (int)(idx / sg.Kp), k = (int)(idx - (int64_t)row * sg.Kp);
  float v = 0.f;
  if (k < sg.K) {
    const int tap = k / sg.Ck, c = k - tap * sg.Ck;
    if (!sg.bwd) {  // row = packed output channel n', c = input channel
      if (row < a.Cout && c < a.Cin) {
        int co = row;
        if (a.cps) { const int ij = row / a.cps, cc = row - ij * a.cps; co = cc * 4 + ij; }
        const int kh = tap / a.KW, kw = tap - kh * a.KW;
        v = a.w[(((size_t)co * a.Cin + c) * a.KH + kh) * a.KW + kw];
      }
    } else {        // row = input channel ci, c = (packed) output channel
      if (row < a.Cin && c < a.Cout) {
        const int th = tap / sg.ntw, tw = tap - th * sg.ntw;
        const int kh = sg.ph + a.pad - a.stride * (sg.dminh + th), kw = sg.pw + a.pad - a.stride * (sg.dminw + tw);
        int co = c;
        if (a.cps) { const int ij = c / a.cps, cc = c - ij * a.cps; co = cc * 4 + ij; }
        v = a.w[(((size_t)co * a.Cin + row) * a.KH + kh) * a.KW + kw];
      }
    }
  }
  sg.dst[idx] = v;
}

}  // namespace

extern "C" int srx_conv2d_pack(const srx_conv2d_t* d, const float* w, float* wpk_fwd, float* wpk_bwd, void* stream) {
  if (int rc = check_desc(d)) return rc;
  SRX_REQUIRE(w && wpk_fwd, "conv2d_pack: null pointer");
  hipStream_t st = srx_stream(stream);
  const Geo g = fwd_geo(d);
  PackArgs pa{};
  pa.w = w; pa.Cout = d->Cout; pa.Cin = d->Cin; pa.KH = d->KH; pa.KW = d->KW; pa.stride = d->stride; pa.pad = d->pad;
  pa.cps = g.cps;
  int64_t maxn = 0;
  if (srx_thin_fwd_applicable(d)) {
    if (int rc = srx_thin_pack(d, w, wpk_fwd, 0, st)) return rc;
  } else {
    PackSeg& sg = pa.seg[pa.nseg++];
    sg = PackSeg{wpk_fwd, g.Cnp, g.K, g.Kp, g.Ck, 0, 0, 0, 0, 0, 1};
    maxn = (int64_t)g.Cnp * g.Kp;
  }
  if (wpk_bwd && srx_thin_dgrad_applicable(d)) {
    if (int rc = srx_thin_pack(d, w, wpk_bwd, 1, st)) return rc;
  } else if (wpk_bwd) {
    SRX_REQUIRE(d->stride <= 4, "conv2d_pack: stride > 4 unsupported for the data gradient");
    BwdClass cls[16];
    size_t total;
    const int nc = bwd_classes(d, cls, total);
    const int Ck = bwd_ck(d);
    const int Cnp = pad_rows(d->Cin);
    for (int i = 0; i < nc; ++i) {
      const BwdClass& c = cls[i];
      PackSeg& sg = pa.seg[pa.nseg++];
      sg = PackSeg{wpk_bwd + c.woff, Cnp, c.K, c.Kp, Ck, 1, c.ph, c.pw, c.dminh, c.dminw, c.ntw > 0 ? c.ntw : 1};
      if ((int64_t)Cnp * c.Kp > maxn) maxn = (int64_t)Cnp * c.Kp;
    }
  }
  if (pa.nseg > 0) {
    hipLaunchKernelGGL(pack_all_kernel, dim3((unsigned)srx_cdiv(maxn, 256), pa.nseg), dim3(256), 0, st, pa);
    SRX_CHECK_LAUNCH("pack_all_kernel");
  }
  return SRX_OK;
}

// ---------------------------------------------------------------------------
// All layers of a model repacked by ONE launch.  The record table is built once on the host (every
// pointer and size in it is fixed for the life of the model), kept in device memory by the caller and
// replayed after each optimiser step: 37 + 8 pack launches per SRGAN step, ~370 per ESRGAN step, become 2.
// ---------------------------------------------------------------------------
struct PackRec {
  float* dst; const float* w;
  long long n_elems;
  int kind;  // 0 forward, 1 data-gradient class, 2 thin forward, 3 thin data gradient
  int rows, K, Kp, Ck, ph, pw, dminh, dminw, ntw;
  int Cout, Cin, KH, KW, stride, pad, cps, pad_;
};

__global__ void pack_table_kernel(const PackRec* __restrict__ table) {
  const PackRec r = table[blockIdx.y];
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= r.n_elems) return;
  float v = 0.f;
  if (r.kind >= 4) {  // Winograd-domain weights (wino.hip): 4 the layer, 5 its data gradient, 6 the layer with a PixelShuffle store
    srx_wino_pack_one(r.w, r.dst, r.Cout, r.Cin, r.kind == 5 ? 1 : (r.kind == 6 ? 2 : 0), idx);
    return;
  }
  if (r.kind >= 2) {  // thin.hip layout: p[c][tap][ch]
    const int taps = r.KH * r.KW;
    const int ch = (int)(idx & 63), tap = (int)((idx >> 6) % taps), c = (int)(idx / (64 * taps));
    const int Cthin = r.kind == 2 ? r.Cout : r.Cin;
    if (c < Cthin) {
      const int kh = tap / r.KW, kw = tap - kh * r.KW;
      v = r.kind == 2 ? r.w[(((size_t)c * 64 + ch) * r.KH + kh) * r.KW + kw]
                      : r.w[(((size_t)ch * Cthin + c) * r.KH + (r.KH - 1 - kh)) * r.KW + (r.KW - 1 - kw)];
    }
    r.dst[idx] = v;
    return;
  }
  // One thread per (packed row, channel): it reads the channel's taps -- adjacent floats of the OIHW weight, so a wave reads one
  // contiguous stretch once -- and writes each to its k = tap * Ck + channel (a wave: 256 contiguous bytes per tap).  One thread
  // per DESTINATION element made every tap's wave pull the same lines through the L2 again (9x the weight bytes for 3x3).
  // The threads behind the (row, channel) range zero the K .. Kp padding.
  const int taps = r.K / r.Ck;  // K = taps * Ck
  const int64_t nmain = (int64_t)r.rows * r.Ck;
  if (idx >= nmain) {
    const int padk = r.Kp - r.K;
    const int64_t j = idx - nmain;
    if (padk > 0 && j < (int64_t)r.rows * padk) {
      const int row = (int)(j / padk);
      r.dst[(size_t)row * r.Kp + r.K + (int)(j - (int64_t)row * padk)] = 0.f;
    }
    return;
  }
  const int row = (int)(idx / r.Ck), c = (int)(idx - (int64_t)row * r.Ck);
  float* d = r.dst + (size_t)row * r.Kp + c;
  const bool live = r.kind == 0 ? (row < r.Cout && c < r.Cin) : (row < r.Cin && c < r.Cout);
  int co = r.kind == 0 ? row : c;  // the conv's output channel this element belongs to
  if (r.cps) { const int ij = co / r.cps, cc = co - ij * r.cps; co = cc * 4 + ij; }
  const float* src = r.w + ((size_t)co * r.Cin + (r.kind == 0 ? c : row)) * (r.KH * r.KW);
  for (int t0 = 0; t0 < taps; t0 += 9) {
    float v[9];
#pragma unroll
    for (int u = 0; u < 9; ++u) {
      const int tap = min(t0 + u, taps - 1);
      int off = tap;  // forward: k runs over (kh, kw) in the weight's own order
      if (r.kind == 1) {
        const int th = tap / r.ntw, tw = tap - th * r.ntw;
        off = (r.ph + r.pad - r.stride * (r.dminh + th)) * r.KW + (r.pw + r.pad - r.stride * (r.dminw + tw));
      }
      v[u] = live ? src[off] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 9; ++u)
      if (t0 + u < taps) d[(size_t)(t0 + u) * r.Ck] = v[u];
  }
}

extern "C" size_t srx_pack_table_bytes(int n_layers) { return (size_t)n_layers * 17 * sizeof(PackRec); }

extern "C" int srx_pack_table_build(const srx_conv2d_t* descs, int n, const float* const* w, float* const* wpk_fwd,
                                    float* const* wpk_bwd, void* host_table, int* nrec_out, long long* max_elems_out) {
  SRX_REQUIRE(descs && w && wpk_fwd && wpk_bwd && host_table && nrec_out && max_elems_out && n > 0,
              "pack_table_build: bad argument");
  PackRec* out = static_cast<PackRec*>(host_table);
  int nrec = 0;
  long long maxn = 0;
  for (int i = 0; i < n; ++i) {
    const srx_conv2d_t* d = descs + i;
    if (int rc = check_desc(d)) return rc;
    SRX_REQUIRE(w[i] && wpk_fwd[i], "pack_table_build: null pointer in layer %d", i);
    const Geo g = fwd_geo(d);
    PackRec base{};
    base.w = w[i];
    base.Cout = d->Cout; base.Cin = d->Cin; base.KH = d->KH; base.KW = d->KW; base.stride = d->stride; base.pad = d->pad;
    base.cps = g.cps;
    auto emit = [&](PackRec r) {
      if (r.n_elems > maxn) maxn = r.n_elems;
      out[nrec++] = r;
    };
    if (srx_thin_fwd_applicable(d)) {
      PackRec r = base; r.kind = 2; r.dst = wpk_fwd[i]; r.n_elems = 4LL * d->KH * d->KW * 64; emit(r);
    } else {
      PackRec r = base; r.kind = 0; r.dst = wpk_fwd[i]; r.rows = g.Cnp; r.K = g.K; r.Kp = g.Kp; r.Ck = g.Ck; r.ntw = 1;
      r.n_elems = (long long)g.Cnp * (g.Ck + g.Kp - g.K); emit(r);  // work items: (row, channel) pairs + the K..Kp padding
    }
    if (!wpk_bwd[i]) continue;
    if (srx_thin_dgrad_applicable(d)) {
      PackRec r = base; r.kind = 3; r.dst = wpk_bwd[i]; r.n_elems = 4LL * d->KH * d->KW * 64; emit(r);
      continue;
    }
    SRX_REQUIRE(d->stride <= 4, "pack_table_build: stride > 4 unsupported for the data gradient");
    BwdClass cls[16];
    size_t total;
    const int nc = bwd_classes(d, cls, total);
    const int Cnp = pad_rows(d->Cin);
    for (int c = 0; c < nc; ++c) {
      PackRec r = base; r.kind = 1; r.dst = wpk_bwd[i] + cls[c].woff;
      r.rows = Cnp; r.K = cls[c].K; r.Kp = cls[c].Kp; r.Ck = bwd_ck(d);
      r.ph = cls[c].ph; r.pw = cls[c].pw; r.dminh = cls[c].dminh; r.dminw = cls[c].dminw;
      r.ntw = cls[c].ntw > 0 ? cls[c].ntw : 1;
      r.n_elems = (long long)Cnp * (r.Ck + cls[c].Kp - cls[c].K);
      emit(r);
    }
  }
  *nrec_out = nrec;
  *max_elems_out = maxn;
  return SRX_OK;
}

// appends the record that refreshes a layer's Winograd-domain weights (srx_wino_pack) to a host table under construction
extern "C" int srx_pack_table_add_wino(void* host_table, int* nrec, long long* max_elems, const srx_conv2d_t* d, const float* w,
                                       float* upk, int transpose) {
  SRX_REQUIRE(host_table && nrec && max_elems && d && w && upk && *nrec >= 0, "pack_table_add_wino: bad argument");
  SRX_REQUIRE(srx_wino_applicable(d) || srx_wino_packed_floats(d) > 0, "pack_table_add_wino: not a Winograd layer");
  PackRec r{};
  SRX_REQUIRE(!(transpose && d->shuffle), "pack_table_add_wino: a PixelShuffle layer has no Winograd data gradient");
  r.dst = upk; r.w = w; r.kind = transpose ? 5 : (d->shuffle ? 6 : 4);
  r.Cout = d->Cout; r.Cin = d->Cin; r.KH = 3; r.KW = 3; r.stride = 1; r.pad = 1;
  r.n_elems = (long long)d->Cout * d->Cin;
  static_cast<PackRec*>(host_table)[(*nrec)++] = r;
  if (r.n_elems > *max_elems) *max_elems = r.n_elems;
  return SRX_OK;
}

extern "C" int srx_pack_table_run(const void* dev_table, int nrec, long long max_elems, void* stream) {
  SRX_REQUIRE(dev_table && nrec > 0 && nrec <= 65535 && max_elems > 0, "pack_table_run: bad argument");
  hipLaunchKernelGGL(pack_table_kernel, dim3((unsigned)srx_cdiv(max_elems, 256), (unsigned)nrec), dim3(256), 0,
                     srx_stream(stream), static_cast<const PackRec*>(dev_table));
  SRX_CHECK_LAUNCH("pack_table_kernel");
  return SRX_OK;
}
