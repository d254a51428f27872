// Training-mode hand-off between two wide binarised conv layers: BatchNorm2d -> Hardtanh ->
// (MaxPool2d(2, 2)) -> sign of the fp32 conv output z, written as the consumer layer's FP4 planes (layout:
// bnn.h, "planes") instead of the fp32 activation that conv_wide_pack_x_k would read next.  Two steps:
//
//  1. the batch statistics, the running-statistics update and save_mean / save_invstd: the launches of
//     bnn_bn2d_fwd_train (bn2d_fwd_stats in bnn_bn.hip), so the same bits.
//  2. bn2d_apply_planes_k<POOL>  one workgroup per (row of the consumer's padded grid, 64-channel block).  A
//     row inside the image is one output row of the (pooled) map: the block's 64 channels x (1 or 2) rows
//     of z are read along W in passes of up to 64 output columns, y = bn_y1(z) is formed per element (the
//     expression of the BatchNorm2d forward apply; the Hardtanh keeps every sign and is left out) and
//     folded into the window's code: 0 if some y is NaN, else +1 if some y > 0, else 0 if some y == 0, else
//     -1 (conv_wide_bnsign_k's rule; without a NaN it is the sign of the chain's pooled activation).  The
//     codes are transposed through an LDS tile ([w][64 B + 4]: a wave's byte writes run along w at a stride
//     of 17 dwords) and stored as two 16-B halves per position.  The row's halo columns, whole halo rows
//     and -- by the last C / 64 workgroups -- the planes' tails are zero-filled, so every byte of the planes
//     is written by exactly one thread of every call.  No atomics.
#include "bnn_conv_wide.h"

#include "bnn.h"
#include "bnn_bn2d.h"

namespace bnn {
namespace {

struct HandoffPlan {
  int pool, PH, PW, pad2, Hp2, Wp2, ncb;
  int64_t P2, Ppad2;   // positions of the consumer's padded grid, positions per plane
};

// The one decision function of the entry and its query.
bool handoff_plan(int64_t N, int64_t C, int64_t H, int64_t W, int32_t pool, int64_t KH2, int64_t KW2, int32_t pad2,
                  HandoffPlan* out) {
  if (N < 0 || C <= 0 || C % 64 != 0 || !bn2d_shape_ok(std::max<int64_t>(N, 1), C, H, W, pool)) return false;
  HandoffPlan p{};
  p.pool = pool, p.PH = (int)(pool ? H / 2 : H), p.PW = (int)(pool ? W / 2 : W);
  const int64_t bytes = bnn_conv2d_wide_planes_bytes(N, C, p.PH, p.PW, KH2, KW2, pad2);
  if (bytes <= 0) return false;   // also bounds the grid: (N Hp2 + 1) C / 64 < 2^31
  p.pad2 = pad2, p.Hp2 = p.PH + 2 * pad2, p.Wp2 = p.PW + 2 * pad2, p.ncb = (int)(C / 64);
  p.P2 = N * p.Hp2 * p.Wp2, p.Ppad2 = bytes / (p.ncb * 32);
  *out = p;
  return true;
}

struct HandoffArgs {
  const float* z;
  const float *mean, *invstd, *gamma, *beta;
  uint8_t* planes;
  int64_t C, P2, Ppad2, rows;   // rows = N Hp2
  int H, W, PH, PW, pad2, Hp2, Wp2, ncb;
};

// the FP4 code of a window from its three flags
__device__ __forceinline__ uint32_t window_code(bool pos, bool zero, bool nan) {
  return nan ? 0u : (pos ? 0x2u : (zero ? 0u : 0xAu));
}

template <int POOL>
__global__ __launch_bounds__(WD_T) void bn2d_apply_planes_k(HandoffArgs a) {
#pragma clang fp contract(off)
  __shared__ uint32_t tile[64 * 17];
  __shared__ Bn2Chan chan[64];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (b >= a.rows * a.ncb) {
    uint8_t* dst = a.planes + ((b - a.rows * a.ncb) * a.Ppad2 + a.P2) * 32;
    for (int64_t i = tid; i < (a.Ppad2 - a.P2) * 2; i += WD_T) store_zero16(dst + i * 16);
    return;
  }
  const int cb = (int)(b % a.ncb);
  const int64_t row = b / a.ncb, n = row / a.Hp2;
  const int ph = (int)(row - n * a.Hp2) - a.pad2;
  uint8_t* dst = a.planes + ((int64_t)cb * a.Ppad2 + row * a.Wp2) * 32;
  if (ph < 0 || ph >= a.PH) {
    for (int i = tid; i < 2 * a.Wp2; i += WD_T) store_zero16(dst + i * 16);
    return;
  }
  for (int i = tid; i < 4 * a.pad2; i += WD_T) store_zero16(dst + (i < 2 * a.pad2 ? i : 2 * a.PW + i) * 16);
  if (tid < 64) chan[tid] = bn2_chan((int64_t)cb * 64 + tid, a.mean, a.invstd, a.gamma, a.beta);
  __syncthreads();
  const int64_t HW = (int64_t)a.H * a.W;
  const float* zr = a.z + ((n * a.C + (int64_t)cb * 64) * a.H + (POOL ? 2 * ph : ph)) * a.W;
  uint8_t* tb = reinterpret_cast<uint8_t*>(tile);
  for (int w0 = 0; w0 < a.PW; w0 += 64) {
    const int wc = min(64, a.PW - w0);
    for (int i = tid; i < 64 * wc; i += WD_T) {
      const int c = i / wc, w = i - c * wc;
      const Bn2Chan k = chan[c];
      bool pos, zero, nan;
      if constexpr (POOL != 0) {
        const float* s = zr + c * HW + 2 * (w0 + w);
        const float2 top = *reinterpret_cast<const float2*>(s), bot = *reinterpret_cast<const float2*>(s + a.W);
        const float y0 = bn_y1(top.x, k.mu, 0.f, k.is, k.ga, k.be), y1 = bn_y1(top.y, k.mu, 0.f, k.is, k.ga, k.be);
        const float y2 = bn_y1(bot.x, k.mu, 0.f, k.is, k.ga, k.be), y3 = bn_y1(bot.y, k.mu, 0.f, k.is, k.ga, k.be);
        pos = (y0 > 0.f) | (y1 > 0.f) | (y2 > 0.f) | (y3 > 0.f);
        zero = (y0 == 0.f) | (y1 == 0.f) | (y2 == 0.f) | (y3 == 0.f);
        nan = (y0 != y0) | (y1 != y1) | (y2 != y2) | (y3 != y3);
      } else {
        const float y = bn_y1(zr[c * HW + w0 + w], k.mu, 0.f, k.is, k.ga, k.be);
        pos = y > 0.f, zero = y == 0.f, nan = y != y;
      }
      tb[w * 68 + c] = (uint8_t)window_code(pos, zero, nan);
    }
    __syncthreads();
    if (tid < 2 * wc) {
      const uint32_t* s = tile + (tid >> 1) * 17 + (tid & 1) * 8;
      uint4 o;
      o.x = squeeze4(s[0]) | squeeze4(s[1]) << 16;
      o.y = squeeze4(s[2]) | squeeze4(s[3]) << 16;
      o.z = squeeze4(s[4]) | squeeze4(s[5]) << 16;
      o.w = squeeze4(s[6]) | squeeze4(s[7]) << 16;
      *reinterpret_cast<uint4*>(dst + (2 * (a.pad2 + w0) + tid) * 16) = o;
    }
    __syncthreads();
  }
}

}  // namespace
}  // namespace bnn

using namespace bnn;

BNN_API int bnn_bn2d_fwd_train_planes_ok(int64_t N, int64_t C, int64_t H, int64_t W, int32_t pool, int64_t KH2,
                                         int64_t KW2, int32_t pad2) {
  HandoffPlan p;
  return handoff_plan(N, C, H, W, pool, KH2, KW2, pad2, &p) ? 1 : 0;
}

BNN_API int bnn_bn2d_fwd_train_planes(const float* z, int64_t N, int64_t C, int64_t H, int64_t W, const float* gamma,
                                      const float* beta, float* running_mean, float* running_var, float momentum,
                                      float eps, float* save_mean, float* save_invstd, void* planes, int32_t pool,
                                      int64_t KH2, int64_t KW2, int32_t pad2, void* work, void* stream) {
  HandoffPlan p;
  if (!handoff_plan(N, C, H, W, pool, KH2, KW2, pad2, &p)) {
    set_error("bnn_bn2d_fwd_train_planes: shape not taken (C %% 64 == 0, H W %% 4 == 0, pool 0 or 2 with even H and "
              "W, and a consumer geometry bnn_conv2d_wide_planes_bytes takes for the (pooled) map)");
    return kErrInval;
  }
  if (!z || !aligned16(z) || !save_mean || !save_invstd || !planes || !aligned16(planes) || !work ||
      (running_mean == nullptr) != (running_var == nullptr)) {
    set_error("bnn_bn2d_fwd_train_planes: null pointer, z or planes not 16-B aligned, or one running statistic "
              "without the other");
    return kErrInval;
  }
  if (N == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  bn2d_fwd_stats(X2{z, nullptr}, 0, N, C, H, W, running_mean, running_var, momentum, eps, save_mean, save_invstd,
                 work, st);
  const HandoffArgs a{z, save_mean, save_invstd, gamma, beta, static_cast<uint8_t*>(planes), C, p.P2, p.Ppad2,
                      N * p.Hp2, (int)H, (int)W, p.PH, p.PW, p.pad2, p.Hp2, p.Wp2, p.ncb};
  const dim3 grid((unsigned)((a.rows + 1) * p.ncb));
  if (pool) hipLaunchKernelGGL(bn2d_apply_planes_k<2>, grid, dim3(WD_T), 0, st, a);
  else hipLaunchKernelGGL(bn2d_apply_planes_k<0>, grid, dim3(WD_T), 0, st, a);
  return check_launch("bnn_bn2d_fwd_train_planes");
}
