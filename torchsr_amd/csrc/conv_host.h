// Host-side geometry and forced-plan state that more than one convolution unit needs (gconv.hip, wgrad.hip, convpack.hip).
// Every function declared here has its one definition in gconv.hip.
#pragma once
#include "srx_common.h"
#include <atomic>

constexpr int BK = 32;  // floats per k-chunk (one 128-byte LDS row)

struct Geo {  // derived sizes of one conv
  int Ho, Wo, Ck, K, Kp, Cnp, cps;
};

struct BwdClass {  // one stride-parity class of the data gradient
  int ph, pw, nth, ntw, dminh, dminw, Hm, Wm, K, Kp;
  size_t woff;  // offset (floats) into the packed bwd buffer
};

int check_desc(const srx_conv2d_t* d);
bool small_enough(const srx_conv2d_t* d);
int pad_rows(int c);
Geo fwd_geo(const srx_conv2d_t* d);
int bwd_ck(const srx_conv2d_t* d);
int bwd_classes(const srx_conv2d_t* d, BwdClass* cls, size_t& total_floats);
srx_conv2d_t upsampled_desc(const srx_conv2d_t* d);
size_t upsampled_floats(const srx_conv2d_t* d);

// In-process overrides of the planners (srx_conv2d_force_plan / srx_conv2d_force_s2 / srx_wgrad_force / srx_wgrad_force_kernels):
// tests switch kernel paths inside one process with them.  Seeded from SRX_FORCE_PLAN, SRX_S2_MODE (bit 0), SRX_NO_WGRAD_LIN,
// SRX_WGRAD_NSPLIT, SRX_WGRAD_ROWS_NSPLIT, SRX_NO_WGRAD_DMA, SRX_NO_WGRAD_ROWS and SRX_OLD_WGRAD_REDUCE at first use: srx_dev() is
// the seed, the planners read this.
struct ConvForce {
  std::atomic<int> plan[4];  // BM, BN, split, KS of every gconv plan; BN = 0: off
  std::atomic<int> s2[3];    // strided data gradients: mode (0 model, 1 gconv_multi_kernel, 2 gconv_s2f_kernel), BM, BN (mode 2)
  std::atomic<int> wg[2];    // weight gradient: LIN (-1 default, 0 never, 1 where eligible), row splits (0: the model's)
  std::atomic<int> wg_rows;  // row splits of the image-row kernel, counted in image rows (0: the model's)
  // weight-gradient kernels, each -1 default / 0 off / 1 on where eligible: LDS-DMA staging of the fp32 kernel (off: wgrad_kernel<0>),
  // the image-row bf16 kernel (off: wgrad_kernel<1>), the row-wise slab reduction (off: wgrad_reduce_kernel)
  std::atomic<int> wk[3];
};
ConvForce& conv_force();  // one process-wide instance: written by the srx_*_force entry points, read by every planner
