// Frozen wide-channel binary conv2d: the FP4-MFMA implicit GEMM of bnn_conv_wide.hip with
// eval-mode BatchNorm2d -> Hardtanh -> (MaxPool2d(2, 2)) -> sign in its epilogue.  Both operands arrive
// packed -- the activation as the FP4 planes a producer layer (or bnn_conv2d_wide_pack_x) wrote, the weight
// as bnn_conv2d_wide_pack_w packed it once -- and the output is either the next wide layer's planes on that
// layer's zero-padded grid (out_form 0: half a byte per element, halo and tail zero-filled by this kernel)
// or int8 signs NCHW (out_form 1).  One launch per layer: no fp32 map, no BatchNorm pass, no pack.
//
// The k-loop is conv_wide_gemm_k's: per 64-channel block one LDS-DMA stage copy of a contiguous run of
// plane rows plus the block's weights of every tap, one MFMA per 32 x 32 tile and tap, the next tap's
// fragments read under the current MFMAs.  What differs is which positions a lane's two sub-tiles hold:
//
//   pool 0   128 consecutive padded-grid positions per workgroup; sub-tile u of wave column wn holds
//            position p0 + 64 wn + 32 u + r.
//   pool 2   64 consecutive window tops e per workgroup, e running over N x OH/2 x Wpe (Wpe = Wp rounded up
//            to even, so a window's two columns are lanes r and r ^ 1); sub-tile 0 holds the top position
//            p_top(e) = (n Hp + 2 pr) Wp + wp, sub-tile 1 p_top + Wp.  A window's vertical pair is two
//            accumulators of one lane and its horizontal pair one DPP quad_perm away.  The staged run starts
//            at the workgroup's first top; rows of the plane past its end are clamped (they feed only
//            positions that are not stored).
//
// Epilogue: per accumulator element x = fl(I + bias[co]), y = bn_y1(x, mean, 0, invstd, gamma, beta) -- the
// expression of bnn_conv2d_fwd_bnsign_pool -- folded into three bit masks per lane (y > 0, y == 0, NaN), one
// bit per channel the lane holds; pooling ORs masks, never values.  The result is +1 if some y > 0, else 0
// if some y == 0, else -1, and 0 if the window holds a NaN.  A wave's two channel tiles are one 64-channel
// block: lane (r, h) holds nibbles 4 h .. 4 h + 3 of each dword of both 16-B halves of its position's row, so
// one v_permlane32_swap per dword hands lane h the whole of half h, stored with one 16-B store.
#include "bnn_conv_wide.h"

#include <cstdio>

#include "bnn.h"

namespace bnn {
namespace {

constexpr int WI_TW = 64;   // window tops of a pooled workgroup

struct InferPlan {
  int64_t N, C, H, W, Co;
  int KH, KW, pad, Hp, Wp, Wpe, OH, OW, PH, PW, taps, ncb, nct, Cop, pool, form;
  int arows, nbuf;
  int64_t Ppad, ntile, lds;
  int Hp2, Wp2, pad2, ncb2;   // out_form 0: the consumer's padded grid
  int64_t P2, Ppad2;
};

// The one decision function of the entry and its two queries.  It starts from the training forward's: a
// geometry bnn_conv2d_fwd_wide_ok refuses is refused here, except that a 64 -> 64 layer is taken too (the
// training dispatch leaves it to the narrow kernels; it runs here as the 128-row tile it half fills).
bool infer_plan(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride,
                int32_t pad, int32_t dil, int32_t groups, int32_t pool, int32_t form, int64_t KH2, int64_t KW2,
                int32_t pad2, InferPlan* out) {
  if (Co <= 0 || !bnn_conv2d_fwd_wide_ok(N, C, H, W, std::max<int64_t>(Co, 65), KH, KW, stride, pad, dil, groups))
    return false;
  if ((pool != 0 && pool != 2) || (form != 0 && form != 1)) return false;
  InferPlan p{};
  p.N = N, p.C = C, p.H = H, p.W = W, p.Co = Co;
  p.KH = (int)KH, p.KW = (int)KW, p.pad = pad, p.pool = pool, p.form = form;
  p.Hp = (int)H + 2 * pad, p.Wp = (int)W + 2 * pad, p.Wpe = (p.Wp + 1) & ~1;
  p.OH = p.Hp - p.KH + 1, p.OW = p.Wp - p.KW + 1;
  if (pool == 2 && ((p.OH | p.OW) & 1)) return false;
  p.PH = pool ? p.OH / 2 : p.OH, p.PW = pool ? p.OW / 2 : p.OW;
  p.taps = p.KH * p.KW, p.ncb = (int)(C / 64);
  p.Cop = (int)round_up(Co, WD_TC), p.nct = p.Cop / WD_TC;
  p.Ppad = bnn_conv2d_wide_planes_bytes(N, C, H, W, KH, KW, pad) / (p.ncb * 32);
  const int64_t tail = (int64_t)(p.KH - 1) * p.Wp + p.KW - 1;
  int64_t span = WD_TP;
  if (pool) {
    // 64 consecutive tops cross at most dr rows of windows, each a step of at most Wp + 1 positions, and dn
    // image boundaries, each (Hp - OH) Wp positions more; the bottom positions lie Wp further
    const int64_t dr = (WI_TW - 1 + p.Wpe - 1) / p.Wpe, dn = (dr + p.PH - 1) / p.PH;
    span = WI_TW + dr * p.Wp + dn * (p.Hp - p.OH) * p.Wp + p.Wp;
    p.ntile = (N * p.PH * p.Wpe + WI_TW - 1) / WI_TW;
  } else {
    p.ntile = (N * p.Hp * p.Wp + WD_TP - 1) / WD_TP;
  }
  const int64_t arows = round_up(span + tail, 32);
  p.lds = (arows + (int64_t)p.taps * WD_TC) * 32;
  if (p.lds > kWideMaxLds || p.ntile * p.nct >= (1ll << 31)) return false;
  p.arows = (int)arows;
  p.nbuf = 2 * p.lds <= kWideMaxLds ? 2 : 1;
  p.lds *= p.nbuf;
  if (form == 0) {
    if (Co % 64 != 0) return false;
    const int64_t bytes = bnn_conv2d_wide_planes_bytes(N, Co, p.PH, p.PW, KH2, KW2, pad2);
    if (bytes == 0) return false;
    p.ncb2 = (int)(Co / 64), p.pad2 = pad2;
    p.Hp2 = p.PH + 2 * pad2, p.Wp2 = p.PW + 2 * pad2;
    p.P2 = N * p.Hp2 * p.Wp2, p.Ppad2 = bytes / (p.ncb2 * 32);
  }
  *out = p;
  return true;
}

struct WideInfer {
  const uint8_t* xq;
  const uint8_t* wq;
  const float *bias, *mean, *invstd, *gamma, *beta;
  void* out;
  int64_t N, Ppad, Co, P2, Ppad2;
  int Hp, Wp, Wpe, PH, PW, Cop, KW, taps, ncb, nct, arows, Hp2, Wp2, pad2, ncb2;
};

// The worst fragment read over every tap, by the bank model, for the lanes' rows as the kernel forms them:
// pool 0 reads consecutive rows (wide_frag_cycles); pool 2 reads rows that jump at the ends of window rows
// and images, evaluated over the lane patterns of up to 1024 workgroups (the pattern repeats with the image).
int infer_frag_cycles(const InferPlan& p) {
  if (!p.pool) return wide_frag_cycles(p.KH, p.KW, p.Wp);
  int worst = 0;
  const int64_t per = (int64_t)p.PH * p.Wpe;
  auto top = [&](int64_t e) {
    const int64_t n = e / per, rem = e - n * per;
    return (n * p.Hp + 2 * (rem / p.Wpe)) * p.Wp + rem % p.Wpe;
  };
  for (int64_t tile = 0; tile < std::min<int64_t>(std::max<int64_t>(p.ntile, 1), 1024); ++tile)
    for (int wn = 0; wn < 2; ++wn)
      for (int u = 0; u < 2; ++u)
        for (int kh = 0; kh < p.KH; ++kh)
          for (int kw = 0; kw < p.KW; ++kw) {
            int addr[64];
            for (int l = 0; l < 64; ++l)
              addr[l] = wide_row_off((int)(top(tile * WI_TW + wn * 32 + (l & 31)) - top(tile * WI_TW)) + u * p.Wp +
                                         kh * p.Wp + kw, l >> 5);
            worst = std::max(worst, lds_b128_cycles(addr));
          }
  return worst;
}

__device__ __forceinline__ uint32_t dpp_xor1(uint32_t v) {   // lane ^ 1: quad_perm [1, 0, 3, 2]
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);
}

// 4 waves as 2 (output channels) x 2 (positions), each 64 channels x 2 sub-tiles of 32 lanes' positions.
// Register i of tile (t, u) is channel 32 t + (i & 3) + 8 (i >> 2) + 4 h of the wave's 64, bit 16 t + i of
// the lane's masks.
template <int NBUF, int POOL, int FORM>
__global__ __launch_bounds__(WD_T) void conv_wide_bnsign_k(WideInfer a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t wide_smem[];
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int ct = (int)(blockIdx.x % a.nct);
  const int64_t pt = blockIdx.x / a.nct;
  const int stage = (a.arows + a.taps * WD_TC) * 32;
  const int na = a.arows / 32, np = na + 4 * a.taps;

  // out_form 0: the halo and the tail of the consumer's planes, 16 B per item, shared out over the grid
  if constexpr (FORM == 0) {
    uint8_t* planes = static_cast<uint8_t*>(a.out);
    const int64_t items = a.ncb2 * a.Ppad2 * 2, HpWp2 = (int64_t)a.Hp2 * a.Wp2;
    for (int64_t it = (int64_t)blockIdx.x * WD_T + threadIdx.x; it < items; it += (int64_t)gridDim.x * WD_T) {
      const int64_t p2 = (it >> 1) % a.Ppad2;
      const int rem = (int)(p2 % HpWp2), hp = rem / a.Wp2 - a.pad2, wp = rem % a.Wp2 - a.pad2;
      if (p2 >= a.P2 || hp < 0 || hp >= a.PH || wp < 0 || wp >= a.PW) store_zero16(planes + it * 16);
    }
  }

  // the positions of this lane's sub-tiles as rows of the staged run, and where its results go
  int64_t pbase, on[2];
  int arow[2], oh[2], ow[2];
  if constexpr (POOL == 0) {
    pbase = pt * WD_TP;
    const int64_t HpWp = (int64_t)a.Hp * a.Wp;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      arow[u] = wn * 64 + u * 32 + r;
      const int64_t p = pbase + arow[u];
      on[u] = p / HpWp;
      const int rem = (int)(p - on[u] * HpWp);
      oh[u] = rem / a.Wp, ow[u] = rem - oh[u] * a.Wp;
    }
  } else {
    const int64_t per = (int64_t)a.PH * a.Wpe;
    auto top = [&](int64_t e, int64_t& n, int& pr, int& wp) {
      n = e / per;
      const int rem = (int)(e - n * per);
      pr = rem / a.Wpe, wp = rem - pr * a.Wpe;
      return (n * a.Hp + 2 * pr) * a.Wp + wp;
    };
    pbase = top(pt * WI_TW, on[1], oh[1], ow[1]);
    arow[0] = (int)(top(pt * WI_TW + wn * 32 + r, on[0], oh[0], ow[0]) - pbase);
    arow[1] = arow[0] + a.Wp;
    on[1] = on[0], oh[1] = oh[0], ow[1] = ow[0];
  }

  // the global chunk that belongs in LDS chunk `lane` of a 32-row piece; plane rows are clamped to the plane
  const int sw = 16 * ((lane & 1) ^ ((lane >> 4) & 1));
  auto issue = [&](int cb, uint8_t* dst) {
    const uint8_t* xs = a.xq + (int64_t)cb * a.Ppad * 32 + sw;
    const uint8_t* ws = a.wq + ((int64_t)cb * a.taps * a.Cop + ct * WD_TC) * 32 + (lane >> 1) * 32 + sw;
    for (int pc = wave; pc < np; pc += 4) {
      const int q = pc - na;
      int64_t row = pbase + pc * 32 + (lane >> 1);
      row = row < a.Ppad ? row : a.Ppad - 1;
      glds16(pc < na ? xs + row * 32 : ws + ((int64_t)(q >> 2) * a.Cop + (q & 3) * 32) * 32, dst + pc * 1024);
    }
  };

  v16f acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][u][i] = 0.f;

  const int woff = a.arows * 32 + wide_row_off(wm * 64 + r, h);   // + 4096 per tap, + 1024 per tile
  auto frags = [&](const uint8_t* buf, int tap, int shift, v4i (&wf)[2], v4i (&af)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t) wf[t] = *reinterpret_cast<const v4i*>(buf + woff + tap * 4096 + t * 1024);
#pragma unroll
    for (int u = 0; u < 2; ++u) af[u] = *reinterpret_cast<const v4i*>(buf + wide_row_off(arow[u] + shift, h));
  };
  auto compute = [&](const uint8_t* buf) {
    v4i wf[2], af[2], wnx[2], anx[2];
    frags(buf, 0, 0, wf, af);
    int kw = 0, shift = 0;
    for (int tap = 0; tap < a.taps; ++tap) {
      const bool more = tap + 1 < a.taps;
      if (more) {   // the next tap's fragments are read under this tap's MFMAs
        ++kw, ++shift;
        if (kw == a.KW) kw = 0, shift += a.Wp - a.KW;
        frags(buf, tap + 1, shift, wnx, anx);
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const v8i xa = {wf[t].x, wf[t].y, wf[t].z, wf[t].w, 0, 0, 0, 0};
          const v8i yb = {af[u].x, af[u].y, af[u].z, af[u].w, 0, 0, 0, 0};
          acc[t][u] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(xa, yb, acc[t][u], 4, 4, 0, 127, 0, 127);
        }
      if (more) {
#pragma unroll
        for (int t = 0; t < 2; ++t) wf[t] = wnx[t], af[t] = anx[t];
      }
    }
  };

  if constexpr (NBUF == 2) {
    issue(0, wide_smem);
    for (int cb = 0; cb < a.ncb; ++cb) {
      wide_wait_dma();
      wide_barrier();   // block cb is in LDS; every wave has left block cb-1, whose buffer is refilled next
      if (cb + 1 < a.ncb) issue(cb + 1, wide_smem + ((cb + 1) & 1) * stage);
      compute(wide_smem + (cb & 1) * stage);
    }
  } else {
    for (int cb = 0; cb < a.ncb; ++cb) {
      if (cb > 0) wide_barrier();
      issue(cb, wide_smem);
      wide_wait_dma();
      wide_barrier();
      compute(wide_smem);
    }
  }

  // BatchNorm and the three masks; a channel past Co leaves its bits clear (never stored)
  const int cw = ct * WD_TC + wm * 64;   // the wave's first output channel
  uint32_t mp[2] = {0u, 0u}, mz[2] = {0u, 0u}, mn[2] = {0u, 0u};
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int co = cw + t * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (co >= a.Co) continue;
        const float b = a.bias ? a.bias[co] : 0.f, mu = a.mean[co], is = a.invstd[co];
        const float ga = a.gamma ? a.gamma[co] : 1.f, be = a.beta ? a.beta[co] : 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const float x = acc[t][u][i] + b;
          const float y = bn_y1(x, mu, 0.f, is, ga, be);
          mp[u] |= (uint32_t)(y > 0.f) << (16 * t + i);
          mz[u] |= (uint32_t)(y == 0.f) << (16 * t + i);
          mn[u] |= (uint32_t)(y != y) << (16 * t + i);
        }
      }
  }
  constexpr int NO = POOL ? 1 : 2;   // results per lane
  if constexpr (POOL == 2) {
    mp[0] |= mp[1], mz[0] |= mz[1], mn[0] |= mn[1];
    mp[0] |= dpp_xor1(mp[0]), mz[0] |= dpp_xor1(mz[0]), mn[0] |= dpp_xor1(mn[0]);
  }

#pragma unroll
  for (int u = 0; u < NO; ++u) {
    const uint32_t nz = ~(mn[u] | (mz[u] & ~mp[u]));       // the sign is not 0
    const uint32_t ng = nz & ~mp[u];                       // the sign is -1
    const bool live = on[u] < a.N && oh[u] < a.PH && (POOL ? (ow[u] & 1) == 0 && (ow[u] >> 1) < a.PW : ow[u] < a.PW);
    const int pw = POOL ? ow[u] >> 1 : ow[u];
    if constexpr (FORM == 0) {
      // this lane's nibbles of both halves in place, then half 1 - h to the lane that stores it
      uint32_t d[2][4];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          uint32_t w = 0u;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int bit = 16 * t + 4 * k + c;
            w |= (((nz >> bit) & 1u) * 2u | ((ng >> bit) & 1u) * 8u) << (4 * c);
          }
          d[t][k] = w << (16 * h);
        }
      uint4 o;
      uint32_t* ov = reinterpret_cast<uint32_t*>(&o);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // lanes 32-63 of the first operand change places with lanes 0-31 of the second: both registers of a
        // lane then belong to its own half
        const auto s = __builtin_amdgcn_permlane32_swap(d[0][k], d[1][k], false, false);
        ov[k] = s[0] | s[1];
      }
      const int cbo = ct * 2 + wm;
      if (live && cbo < a.ncb2) {
        const int64_t p2 = (on[u] * a.Hp2 + oh[u] + a.pad2) * a.Wp2 + pw + a.pad2;
        *reinterpret_cast<uint4*>(static_cast<uint8_t*>(a.out) + (cbo * a.Ppad2 + p2) * 32 + 16 * h) = o;
      }
    } else {
      if (!live) continue;
      const int64_t plane = (int64_t)a.PH * a.PW;
      int8_t* op = static_cast<int8_t*>(a.out) + on[u] * a.Co * plane + (int64_t)oh[u] * a.PW + pw;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int co = cw + t * 32 + (i & 3) + 8 * (i >> 2) + 4 * h, bit = 16 * t + i;
          if (co < a.Co) op[co * plane] = (int8_t)((int)((nz >> bit) & 1u) - 2 * (int)((ng >> bit) & 1u));
        }
    }
  }
}

template <int NBUF, int POOL, int FORM>
void infer_launch(const InferPlan& p, const WideInfer& a, hipStream_t st) {
  if (p.lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wide_bnsign_k<NBUF, POOL, FORM>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
  hipLaunchKernelGGL((conv_wide_bnsign_k<NBUF, POOL, FORM>), dim3((unsigned)(p.ntile * p.nct)), dim3(WD_T),
                     (size_t)p.lds, st, a);
}

}  // namespace
}  // namespace bnn

using namespace bnn;

BNN_API int bnn_conv2d_fwd_wide_bnsign_ok(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH,
                                          int64_t KW, int32_t stride, int32_t pad, int32_t dil, int32_t groups,
                                          int32_t pool, int32_t out_form, int64_t KH2, int64_t KW2, int32_t pad2) {
  InferPlan p;
  return infer_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, pool, out_form, KH2, KW2, pad2, &p) ? 1 : 0;
}

BNN_API const char* bnn_conv2d_fwd_wide_bnsign_kernel(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co,
                                                      int64_t KH, int64_t KW, int32_t stride, int32_t pad,
                                                      int32_t dil, int32_t groups, int32_t pool, int32_t out_form,
                                                      int64_t KH2, int64_t KW2, int32_t pad2) {
  static thread_local char buf[96];
  InferPlan p;
  if (!infer_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, pool, out_form, KH2, KW2, pad2, &p)) return "";
  snprintf(buf, sizeof(buf), "conv_wide_bnsign_k<%d,%d,%d> lds=%lld b128=%d", p.nbuf, p.pool, p.form,
           (long long)p.lds, infer_frag_cycles(p));
  return buf;
}

BNN_API int bnn_conv2d_fwd_wide_bnsign(const void* planes, const void* wq, const float* bias, const float* mean,
                                       const float* invstd, const float* gamma, const float* beta, void* out,
                                       int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW,
                                       int32_t pad, int32_t pool, int32_t out_form, int64_t KH2, int64_t KW2,
                                       int32_t pad2, void* stream) {
  InferPlan p;
  if (!infer_plan(N, C, H, W, Co, KH, KW, 1, pad, 1, 1, pool, out_form, KH2, KW2, pad2, &p)) {
    set_error("bnn_conv2d_fwd_wide_bnsign: shape not taken (a geometry of bnn_conv2d_fwd_wide or 64 -> 64 "
              "channels, pool 0 or 2 with even OH and OW, the staged window within the LDS; out_form 0 needs "
              "Co %% 64 == 0 and a consumer geometry bnn_conv2d_wide_planes_bytes takes)");
    return kErrInval;
  }
  if (!planes || !wq || !mean || !invstd || !out || !aligned16(planes) || !aligned16(wq) ||
      (out_form == 0 && !aligned16(out))) {
    set_error("bnn_conv2d_fwd_wide_bnsign: null pointer, or planes / wq / output planes not 16-B aligned");
    return kErrInval;
  }
  if (N == 0) return 0;
  const WideInfer a{static_cast<const uint8_t*>(planes), static_cast<const uint8_t*>(wq), bias, mean, invstd,
                    gamma, beta, out, N, p.Ppad, Co, p.P2, p.Ppad2, p.Hp, p.Wp, p.Wpe, p.PH, p.PW, p.Cop, p.KW,
                    p.taps, p.ncb, p.nct, p.arows, p.Hp2, p.Wp2, p.pad2, p.ncb2};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define BNN_WI(NB_, PL_, FM_) \
  if (p.nbuf == NB_ && p.pool == PL_ && p.form == FM_) infer_launch<NB_, PL_, FM_>(p, a, st)
  BNN_WI(2, 0, 0); BNN_WI(2, 0, 1); BNN_WI(2, 2, 0); BNN_WI(2, 2, 1);
  BNN_WI(1, 0, 0); BNN_WI(1, 0, 1); BNN_WI(1, 2, 0); BNN_WI(1, 2, 1);
#undef BNN_WI
  return check_launch("bnn_conv2d_fwd_wide_bnsign");
}
