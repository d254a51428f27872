// Wide-channel binary conv2d input gradient (the shapes bnn_conv2d_fwd_wide takes):
//   dx[n,c,ih,iw] = sum_{co,kh,kw} dy[n,co,ih+pad-kh,iw+pad-kw] * tsign(w[co,c,kh,kw])
// as an implicit GEMM on v_mfma_f32_32x32x16_bf16.  The fp32 operand dY is split exactly into three
// bf16 planes (bf16x3_split) and the weights are ternary bf16, so every product is exact and the only
// rounding is the MFMA's fp32 accumulation.  Three launches per call:
//
//  1. conv_wide_bwd_pack_dy_k  dy fp32 NCHW -> dq [ceil(Co/16)][3 planes][Ppad][32 B] on the grid padded to
//                              Hq = H + KH-1, Wq = W + KW-1: dy(oh, ow) sits at (oh + KH-1-pad, ow + KW-1-pad),
//                              position p = (n Hq + hq) Wq + wq, one 32-B row = 16 output channels of one
//                              plane.  Halo, channel tail and plane tails are written as zeros on every call.
//  2. conv_wide_bwd_pack_w_k   latent w [Co][C][KH][KW] -> wq [ceil(Co/16)][KH KW shifts][Cp][32 B], the filter
//                              flipped: shift (a, b) holds tap (KH-1-a, KW-1-b).  Rows C .. Cp-1 and the
//                              channel tail are zero.
//  3. conv_wide_bwd_data_k     dX at (ih, iw) has base position p = (n Hq + ih) Wq + iw and needs, for shift
//                              (a, b), packed position p + a Wq + b -- a constant shift per tap, zero halo is
//                              bf16 0, no border is special.  A workgroup owns 128 consecutive positions x 128
//                              input channels; per block of 16 output channels it copies the three planes'
//                              windows and the block's weights of every shift into LDS with
//                              global_load_lds_dwordx4 and runs the shifts out of LDS, 12 MFMAs per wave and
//                              shift.  No atomics, no split: deterministic.
//
// Rows, the half swizzle and the fragment geometry are those of the forward (bnn_conv_wide.h): a 32-B
// row of 16 bf16 read as lane (r, h) -> half h of row base + r is the 32x32x16 bf16 operand.
#include "bnn_conv_wide.h"

#include <cstdio>

#include "bnn.h"

namespace bnn {
namespace {

struct WideBwdPlan {
  int64_t N, C, H, W, Co;
  int KH, KW, pad, Hq, Wq, OH, OW, taps, nkb, nct, Cp;
  int hh, hw;     // KH-1-pad, KW-1-pad: the zero halo above / left of dY (and below / right of it)
  int arows;      // dY rows a workgroup stages per plane and output-channel block, a multiple of 32
  int nbuf;       // LDS stages: 2 = the next block's copy runs under this block's MFMAs, 1 = it does not fit
  int cycles;     // modelled LDS cycles of the worst fragment ds_read_b128 (4 = conflict-free)
  int64_t P;      // N Hq Wq positions of the padded grid
  int64_t Ppad;   // positions per plane: the last tile's window stays inside it
  int64_t ntile, lds, wq_off, work_bytes;
};

// The one decision function: bnn_conv2d_bwd_data_wide_ok, the workspace and kernel queries and the launch.
// The set is the forward's, less what the three-plane stage, a grid or an index does not hold.
bool wide_bwd_plan(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride,
                   int32_t pad, int32_t dil, int32_t groups, WideBwdPlan* out) {
  if (!bnn_conv2d_fwd_wide_ok(N, C, H, W, Co, KH, KW, stride, pad, dil, groups)) return false;
  WideBwdPlan p{};
  p.N = N, p.C = C, p.H = H, p.W = W, p.Co = Co;
  p.KH = (int)KH, p.KW = (int)KW, p.pad = pad;
  p.Hq = (int)(H + KH - 1), p.Wq = (int)(W + KW - 1);
  p.OH = (int)(H + 2 * pad - KH + 1), p.OW = (int)(W + 2 * pad - KW + 1);
  p.hh = p.KH - 1 - pad, p.hw = p.KW - 1 - pad;
  p.taps = p.KH * p.KW, p.nkb = (int)((Co + 15) / 16);
  p.Cp = (int)round_up(C, WD_TC), p.nct = p.Cp / WD_TC;
  const int64_t tail = (int64_t)(p.KH - 1) * p.Wq + p.KW - 1;
  const int64_t arows = round_up(WD_TP + tail, 32);
  p.lds = (3 * arows + (int64_t)p.taps * WD_TC) * 32;
  if (p.lds > kWideMaxLds || (int64_t)p.Hq * p.Wq >= (1ll << 31)) return false;
  p.arows = (int)arows;
  p.nbuf = 2 * p.lds <= kWideMaxLds ? 2 : 1;
  p.lds *= p.nbuf;
  p.cycles = wide_frag_cycles(p.KH, p.KW, p.Wq);
  p.P = N * p.Hq * p.Wq;
  p.ntile = (p.P + WD_TP - 1) / WD_TP;
  p.Ppad = p.ntile * WD_TP - WD_TP + arows;
  // grids are 1-D: GEMM tiles, one dY pack block per padded row and channel block, the weight pack's threads
  if (p.ntile * p.nct >= (1ll << 31) || (N * p.Hq + 1) * p.nkb >= (1ll << 31) ||
      (int64_t)p.nkb * 2 * p.Cp * p.taps / WD_T >= (1ll << 31) - 1 || C * H * W >= (1ll << 31))
    return false;
  p.wq_off = round_up((int64_t)p.nkb * 3 * p.Ppad * 32, 256);
  p.work_bytes = p.wq_off + (int64_t)p.nkb * p.taps * p.Cp * 32;
  *out = p;
  return true;
}

struct WideBwdPackDy {
  int64_t Co, P, Ppad, rows;   // rows = N Hq
  int OH, OW, Hq, Wq, hh, hw, nkb;
};

constexpr int DY_PITCH = 18;   // bf16 per LDS tile row: 16 + 2, a wave's 2-B writes along ow run at 9 dwords

// One workgroup per (padded row, block of 16 output channels): 16 channels x up to 64 columns at a time
// are read along ow, split into the three planes, transposed through LDS and stored as 16-B halves,
// 32 B per position and plane.  The row's halo columns, whole halo rows, and -- by the last nkb
// workgroups -- the planes' tails are zero-filled.
__global__ __launch_bounds__(WD_T) void conv_wide_bwd_pack_dy_k(const float* __restrict__ dy, uint8_t* __restrict__ dq,
                                                                 WideBwdPackDy a) {
  __shared__ __attribute__((aligned(16))) unsigned short tile[3][64 * DY_PITCH];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (b >= a.rows * a.nkb) {
    const int64_t kb = b - a.rows * a.nkb;
    const int64_t n16 = (a.Ppad - a.P) * 2;
    for (int pl = 0; pl < 3; ++pl) {
      uint8_t* dst = dq + ((kb * 3 + pl) * a.Ppad + a.P) * 32;
      for (int64_t i = tid; i < n16; i += WD_T) store_zero16(dst + i * 16);
    }
    return;
  }
  const int kb = (int)(b % a.nkb);
  const int64_t row = b / a.nkb, n = row / a.Hq;
  const int oh = (int)(row - n * a.Hq) - a.hh;
  const int64_t plane = a.Ppad * 32;
  uint8_t* dst = dq + ((int64_t)kb * 3 * a.Ppad + row * a.Wq) * 32;   // plane 0 of this row
  if (oh < 0 || oh >= a.OH) {
    for (int i = tid; i < 6 * a.Wq; i += WD_T) {
      const int pl = i / (2 * a.Wq);
      store_zero16(dst + pl * plane + (i - pl * 2 * a.Wq) * 16);
    }
    return;
  }
  for (int i = tid; i < 12 * a.hw; i += WD_T) {   // hw halo columns on either side, two halves, three planes
    const int pl = i / (4 * a.hw), j = i - pl * 4 * a.hw;
    store_zero16(dst + pl * plane + (j < 2 * a.hw ? j : 2 * a.OW + j) * 16);
  }
  const int64_t ohw = (int64_t)a.OH * a.OW;
  const int cn = (int)min((int64_t)16, a.Co - kb * 16);   // live channels of this block
  const float* yr = dy + ((n * a.Co + kb * 16) * a.OH + oh) * a.OW;
  for (int w0 = 0; w0 < a.OW; w0 += 64) {
    const int wc = min(64, a.OW - w0);
    for (int i = tid; i < 16 * wc; i += WD_T) {
      const int c = i / wc, w = i - c * wc;
      unsigned short d1, d2, d3;
      bf16x3_split(c < cn ? yr[c * ohw + w0 + w] : 0.f, d1, d2, d3);
      tile[0][w * DY_PITCH + c] = d1;
      tile[1][w * DY_PITCH + c] = d2;
      tile[2][w * DY_PITCH + c] = d3;
    }
    __syncthreads();
    for (int i = tid; i < 6 * wc; i += WD_T) {
      const int pl = i / (2 * wc), j = i - pl * 2 * wc;   // j = 2 w + half
      const uint32_t* s = reinterpret_cast<const uint32_t*>(&tile[pl][(j >> 1) * DY_PITCH + (j & 1) * 8]);
      *reinterpret_cast<uint4*>(dst + pl * plane + (2 * (a.hw + w0) + j) * 16) = make_uint4(s[0], s[1], s[2], s[3]);
    }
    __syncthreads();
  }
}

// One thread per 16-B half row of wq (8 output channels of one input channel and shift); the tap runs
// fastest over the threads, then the input channel, so a wave's 8 strided reads each sweep one contiguous
// piece of the latent weight.
__global__ __launch_bounds__(WD_T) void conv_wide_bwd_pack_w_k(const float* __restrict__ w, uint8_t* __restrict__ wq,
                                                                int64_t C, int64_t Co, int Cp, int taps, int nkb) {
  const int64_t idx = (int64_t)blockIdx.x * WD_T + threadIdx.x;
  if (idx >= (int64_t)nkb * 2 * Cp * taps) return;
  const int tap = (int)(idx % taps);
  int64_t q = idx / taps;
  const int c = (int)(q % Cp);
  q /= Cp;
  const int half = (int)(q & 1);
  const int64_t kb = q >> 1;
  uint32_t o[4] = {0u, 0u, 0u, 0u};
  if (c < C) {
    const int64_t co0 = kb * 16 + half * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int sv = co0 + j < Co ? tsign(w[((co0 + j) * C + c) * taps + tap]) : 0;
      o[j >> 1] |= (sv > 0 ? 0x3F80u : (sv < 0 ? 0xBF80u : 0u)) << (16 * (j & 1));
    }
  }
  // the flip: shift (a, b) = tap (KH-1-a, KW-1-b), i.e. shift index taps-1-tap
  *reinterpret_cast<uint4*>(wq + ((kb * taps + (taps - 1 - tap)) * Cp + c) * 32 + half * 16) =
      make_uint4(o[0], o[1], o[2], o[3]);
}

struct WideBwdGemm {
  const uint8_t* dq;
  const uint8_t* wq;
  float* dx;
  int64_t P, Ppad, HqWq, C, HW;
  int Wq, H, W, Cp, KW, taps, nkb, nct, arows;
};

// 4 waves as 2 (input channels) x 2 (positions), each 64 x 64 as 2 x 2 MFMA tiles.  The weights are the
// MFMA's first operand and the positions its second, so an accumulator register is an input channel and
// the lanes run along positions: register i of tile (t, u) is channel 32 t + (i & 3) + 8 (i >> 2) + 4 h at
// position 32 u + (lane & 31), and an NCHW store is a run along iw.  A stage is the three planes' windows
// (arows rows each), then taps x 128 weight rows.
template <int NBUF>
__global__ __launch_bounds__(WD_T) void conv_wide_bwd_data_k(WideBwdGemm a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t wide_bwd_smem[];
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int ct = (int)(blockIdx.x % a.nct);
  const int64_t p0 = (int64_t)(blockIdx.x / a.nct) * WD_TP;
  const int aplane = a.arows * 32;
  const int stage = 3 * aplane + a.taps * WD_TC * 32;
  const int na = a.arows / 32, np = 3 * na + 4 * a.taps;   // 1-KiB pieces (32 rows): 3 windows, then 4 per shift
  // the global chunk that belongs in LDS chunk `lane` of a piece (pieces start on multiples of 32 rows)
  const int soff = (lane >> 1) * 32 + 16 * ((lane & 1) ^ ((lane >> 4) & 1));

  auto issue = [&](int kb, uint8_t* dst) {
    const uint8_t* ds = a.dq + ((int64_t)kb * 3 * a.Ppad + p0) * 32 + soff;
    const uint8_t* ws = a.wq + ((int64_t)kb * a.taps * a.Cp + ct * WD_TC) * 32 + soff;
    for (int pc = wave; pc < np; pc += 4) {
      const int pl = (pc >= na) + (pc >= 2 * na), q = pc - 3 * na;
      glds16(q < 0 ? ds + (int64_t)pl * a.Ppad * 32 + (pc - pl * na) * 1024
                   : ws + ((int64_t)(q >> 2) * a.Cp + (q & 3) * 32) * 32,
             dst + pc * 1024);
    }
  };

  v16f acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][u][i] = 0.f;

  // a wave whose 64 channels lie beyond C (C % 128 == 64, last channel tile) copies and waits, no more
  const bool live = ct * WD_TC + wm * 64 < a.C;
  const int woff = 3 * aplane + wide_row_off(wm * 64 + r, h);   // + 4096 per shift, + 1024 per tile
  const int arow = wn * 64 + r;
  auto frags = [&](const uint8_t* buf, int tap, int shift, v4i (&wf)[2], v4i (&af)[3][2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t) wf[t] = *reinterpret_cast<const v4i*>(buf + woff + tap * 4096 + t * 1024);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int o = wide_row_off(arow + shift + u * 32, h);
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) af[pl][u] = *reinterpret_cast<const v4i*>(buf + pl * aplane + o);
    }
  };
  auto compute = [&](const uint8_t* buf) {
    v4i wf[2], af[3][2], wnx[2], anx[3][2];
    frags(buf, 0, 0, wf, af);
    int kw = 0, shift = 0;
    for (int tap = 0; tap < a.taps; ++tap) {
      const bool more = tap + 1 < a.taps;
      if (more) {   // the next shift's 8 fragments are read under this shift's 12 MFMAs
        ++kw, ++shift;
        if (kw == a.KW) kw = 0, shift += a.Wq - a.KW;
        frags(buf, tap + 1, shift, wnx, anx);
      }
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)   // fixed plane order: d1, d2, d3
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int u = 0; u < 2; ++u)
            acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, wf[t]),
                                                                __builtin_bit_cast(v8bf, af[pl][u]), acc[t][u], 0, 0, 0);
      if (more) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          wf[t] = wnx[t];
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) af[pl][t] = anx[pl][t];
        }
      }
    }
  };

  if constexpr (NBUF == 2) {
    issue(0, wide_bwd_smem);
    for (int kb = 0; kb < a.nkb; ++kb) {
      wide_wait_dma();
      wide_barrier();   // block kb is in LDS; every wave has left block kb-1, whose buffer is refilled next
      if (kb + 1 < a.nkb) issue(kb + 1, wide_bwd_smem + ((kb + 1) & 1) * stage);
      if (live) compute(wide_bwd_smem + (kb & 1) * stage);
    }
  } else {
    for (int kb = 0; kb < a.nkb; ++kb) {
      if (kb > 0) wide_barrier();
      issue(kb, wide_bwd_smem);
      wide_wait_dma();
      wide_barrier();
      if (live) compute(wide_bwd_smem);
    }
  }
  if (!live) return;

  // positions of the halo (ih >= H or iw >= W) and beyond P are computed and not stored
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int64_t p = p0 + wn * 64 + u * 32 + r;
    const int64_t n = p / a.HqWq;
    const int rem = (int)(p - n * a.HqWq), ih = rem / a.Wq, iw = rem - ih * a.Wq;
    if (p >= a.P || ih >= a.H || iw >= a.W) continue;
    float* xp = a.dx + (n * a.C + ct * WD_TC + wm * 64 + 4 * h) * a.HW + ih * a.W + iw;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) xp[(t * 32 + (i & 3) + 8 * (i >> 2)) * a.HW] = acc[t][u][i];
  }
}

int g_wide_bwd_stages = 7;   // bnn_conv2d_bwd_data_wide_set_stages

const char* wide_bwd_name(const WideBwdPlan& p) { return p.nbuf == 2 ? "conv_wide_bwd_data_k<2>" : "conv_wide_bwd_data_k<1>"; }

template <int NBUF>
void wide_bwd_launch(const WideBwdPlan& p, const WideBwdGemm& a, hipStream_t st) {
  if (p.lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wide_bwd_data_k<NBUF>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
  hipLaunchKernelGGL((conv_wide_bwd_data_k<NBUF>), dim3((unsigned)(p.ntile * p.nct)), dim3(WD_T), (size_t)p.lds, st, a);
}

}  // namespace
}  // namespace bnn

using namespace bnn;

BNN_API int bnn_conv2d_bwd_data_wide_ok(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH,
                                        int64_t KW, int32_t stride, int32_t pad, int32_t dil, int32_t groups) {
  WideBwdPlan p;
  return wide_bwd_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p) ? 1 : 0;
}

BNN_API int64_t bnn_conv2d_bwd_data_wide_workspace(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH,
                                                   int64_t KW, int32_t pad) {
  WideBwdPlan p;
  return wide_bwd_plan(N, C, H, W, Co, KH, KW, 1, pad, 1, 1, &p) ? p.work_bytes : 0;
}

BNN_API const char* bnn_conv2d_bwd_data_wide_kernel(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co,
                                                    int64_t KH, int64_t KW, int32_t stride, int32_t pad, int32_t dil,
                                                    int32_t groups) {
  static thread_local char buf[96];
  WideBwdPlan p;
  if (!wide_bwd_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p)) return "";
  snprintf(buf, sizeof(buf), "%s lds=%lld b128=%d", wide_bwd_name(p), (long long)p.lds, p.cycles);
  return buf;
}

BNN_API int bnn_conv2d_bwd_data_wide_set_stages(int32_t mask) {
  if (mask >= 0) g_wide_bwd_stages = mask & 7;
  return g_wide_bwd_stages;
}

BNN_API int bnn_conv2d_bwd_data_wide(const float* dy, const float* w_latent, float* dx, int64_t N, int64_t C,
                                     int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride,
                                     int32_t pad, int32_t dil, int32_t groups, void* work, int64_t work_bytes,
                                     void* stream) {
  WideBwdPlan p;
  if (!wide_bwd_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p)) {
    set_error("bnn_conv2d_bwd_data_wide: shape not taken (a shape of bnn_conv2d_fwd_wide whose three dY windows "
              "and KH KW x 128 weight rows of one 16-channel block fit the LDS)");
    return kErrInval;
  }
  if (!dy || !w_latent || !dx || !work || !aligned16(work) || work_bytes < p.work_bytes) {
    set_error("bnn_conv2d_bwd_data_wide: null pointer, or a workspace not 16-B aligned or below "
              "bnn_conv2d_bwd_data_wide_workspace = %lld bytes", (long long)p.work_bytes);
    return kErrInval;
  }
  if (N == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint8_t* dq = static_cast<uint8_t*>(work);
  uint8_t* wq = dq + p.wq_off;
  const WideBwdPackDy py{Co, p.P, p.Ppad, N * p.Hq, p.OH, p.OW, p.Hq, p.Wq, p.hh, p.hw, p.nkb};
  if (g_wide_bwd_stages & 1)
    hipLaunchKernelGGL(conv_wide_bwd_pack_dy_k, dim3((unsigned)((py.rows + 1) * p.nkb)), dim3(WD_T), 0, st, dy, dq,
                       py);
  const int64_t nw = (int64_t)p.nkb * 2 * p.Cp * p.taps;
  if (g_wide_bwd_stages & 2)
    hipLaunchKernelGGL(conv_wide_bwd_pack_w_k, dim3((unsigned)((nw + WD_T - 1) / WD_T)), dim3(WD_T), 0, st, w_latent,
                       wq, C, Co, p.Cp, p.taps, p.nkb);
  const WideBwdGemm g{dq, wq, dx, p.P, p.Ppad, (int64_t)p.Hq * p.Wq, C, H * W,
                      p.Wq, (int)H, (int)W, p.Cp, p.KW, p.taps, p.nkb, p.nct, p.arows};
  if (!(g_wide_bwd_stages & 4)) return check_launch("bnn_conv2d_bwd_data_wide");
  if (p.nbuf == 2) wide_bwd_launch<2>(p, g, st);
  else wide_bwd_launch<1>(p, g, st);
  return check_launch("bnn_conv2d_bwd_data_wide");
}
