// Wide-channel binary conv2d input gradient at stride 2 (the shapes bnn_conv2d_fwd_wide_s2 takes):
//   dx[n,c,ih,iw] = sum_{co,kh,kw} dy[n,co,oh,ow] * tsign(w[co,c,kh,kw]),  2 oh + kh = ih + pad, 2 ow + kw = iw + pad
// as an implicit GEMM on v_mfma_f32_32x32x16_bf16, dY as the three exact bf16 planes of bf16x3_split and the
// weights ternary bf16 as in §20: every product is exact, the only rounding is the MFMA's fp32 accumulation.
//
// dX is split by the parity of the padded input pixel: hp = ih + pad = 2 i + a, wp = iw + pad = 2 j + b.  Only the
// taps kh = 2 s + a, kw = 2 t + b reach phase (a, b), and tap (2 s + a, 2 t + b) reads dy(i - s, j - t): each of
// the four phases is a stride-1 shifted-window sum over its own sub-filter, and the taps that share (s, t) -- a
// shift group, up to four of them, one per phase -- read the same dY.  dY lies on one grid of Gh = Hq + mh rows
// and Gw = Wq + mw columns (Hq = ceil(Hp / 2), Wq = ceil(Wp / 2), mh = (KH-1) >> 1, mw = (KW-1) >> 1) with
// dy(oh, ow) at (oh + mh, ow + mw) and bf16 0 elsewhere; position p = (n Gh + g) Gw + gw, cell (i, j) has base
// position (n Gh + i) Gw + j and group (s, t) reads p + (mh - s) Gw + (mw - t): a constant shift, no border is
// special, and a shift never leaves the row of a cell that is stored (j < Wq).  Three launches per call:
//
//  1. conv_wide_bwd_pack_dy_s2_k  dy fp32 NCHW -> dq [ceil(Co/16)][3 planes][Ppad][32 B], §20's rows on this grid
//                                 (mw halo columns on the left, Gw - mw - OW on the right).  Halo, channel tail
//                                 and plane tails are written as zeros on every call.
//  2. conv_wide_bwd_pack_w_s2_k   latent w [Co][C][KH][KW] -> wq [ceil(Co/16)][KH KW taps][C][32 B], the taps
//                                 ordered by shift group (s, t), then by phase (a, b); no flip (the shift holds it).
//  3. conv_wide_bwd_data_s2_k     a workgroup owns 128 consecutive positions x 64 input channels x all four
//                                 phases.  Per block of 16 output channels it copies the three planes' windows
//                                 and the block's KH KW x 64 weight rows into LDS with global_load_lds_dwordx4
//                                 and walks the shift groups: six dY fragments per group, then per phase that
//                                 owns a tap of the group one weight fragment and 6 MFMAs into that phase's
//                                 accumulators.  No atomics, no split: deterministic.
//
// Rows, the half swizzle and the fragment geometry are those of bnn_conv_wide.h and §20.
#include "bnn_conv_wide.h"

#include <cstdio>

#include "bnn.h"

namespace bnn {
namespace {

constexpr int S2B_TC = 64;   // input channels of a GEMM workgroup (x 4 phases = 256 accumulator rows)

struct S2BwdPlan {
  int64_t N, C, H, W, Co;
  int KH, KW, pad, Hq, Wq, Gh, Gw, mh, mw, OH, OW, taps, nkb, nct;
  int arows;      // dY rows a workgroup stages per plane and output-channel block, a multiple of 32
  int nbuf;       // LDS stages: 2 = the next block's copy runs under this block's MFMAs, 1 = it does not fit
  int cycles;     // modelled LDS cycles of the worst fragment ds_read_b128 (4 = conflict-free)
  int64_t P;      // N Gh Gw positions of the dY grid
  int64_t Ppad;   // positions per plane: the last tile's window stays inside it
  int64_t ntile, lds, wq_off, work_bytes;
};

// The one decision function: bnn_conv2d_bwd_data_wide_s2_ok, the workspace and kernel queries and the launch.
// The set is the stride-2 forward's, less what the three-plane stage, a grid or an index does not hold.
bool s2_bwd_plan(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride,
                 int32_t pad, int32_t dil, int32_t groups, S2BwdPlan* out) {
  if (!bnn_conv2d_fwd_wide_s2_ok(N, C, H, W, Co, KH, KW, stride, pad, dil, groups)) return false;
  S2BwdPlan p{};
  p.N = N, p.C = C, p.H = H, p.W = W, p.Co = Co;
  p.KH = (int)KH, p.KW = (int)KW, p.pad = pad;
  const int Hp = (int)H + 2 * pad, Wp = (int)W + 2 * pad;
  p.Hq = (Hp + 1) / 2, p.Wq = (Wp + 1) / 2;
  p.OH = (Hp - p.KH) / 2 + 1, p.OW = (Wp - p.KW) / 2 + 1;
  p.mh = (p.KH - 1) >> 1, p.mw = (p.KW - 1) >> 1;
  p.Gh = p.Hq + p.mh, p.Gw = p.Wq + p.mw;
  p.taps = p.KH * p.KW, p.nkb = (int)((Co + 15) / 16), p.nct = (int)(C / S2B_TC);
  const int64_t arows = round_up(WD_TP + (int64_t)p.mh * p.Gw + p.mw, 32);
  p.lds = (3 * arows + (int64_t)p.taps * S2B_TC) * 32;
  if (p.lds > kWideMaxLds || (int64_t)p.Gh * p.Gw >= (1ll << 31)) return false;
  p.arows = (int)arows;
  p.nbuf = 2 * p.lds <= kWideMaxLds ? 2 : 1;
  p.lds *= p.nbuf;
  for (int s = 0; s <= p.mh; ++s)   // every shift group's real base row
    for (int t = 0; t <= p.mw; ++t) {
      int addr[64];
      for (int l = 0; l < 64; ++l) addr[l] = wide_row_off((p.mh - s) * p.Gw + p.mw - t + (l & 31), l >> 5);
      p.cycles = std::max(p.cycles, lds_b128_cycles(addr));
    }
  p.P = N * p.Gh * p.Gw;
  p.ntile = (p.P + WD_TP - 1) / WD_TP;
  p.Ppad = p.ntile * WD_TP - WD_TP + arows;
  // grids are 1-D: GEMM tiles, one dY pack block per grid row and channel block, the weight pack's threads
  if (p.ntile * p.nct >= (1ll << 31) || (N * p.Gh + 1) * p.nkb >= (1ll << 31) ||
      (int64_t)p.nkb * 2 * C * p.taps / WD_T >= (1ll << 31) - 1 || C * H * W >= (1ll << 31) ||
      Co * p.OH * p.OW >= (1ll << 31))
    return false;
  p.wq_off = round_up((int64_t)p.nkb * 3 * p.Ppad * 32, 256);
  p.work_bytes = p.wq_off + (int64_t)p.nkb * p.taps * C * 32;
  *out = p;
  return true;
}

struct S2BwdPackDy {
  int64_t Co, P, Ppad, rows;   // rows = N Gh
  int OH, OW, Gh, Gw, mh, mw, nkb;
};

constexpr int DY_PITCH = 18;   // bf16 per LDS tile row: 16 + 2, a wave's 2-B writes along ow run at 9 dwords

// §20's dY pack with unequal halos.  One workgroup per (grid row, block of 16 output channels): 16 channels x
// up to 64 columns at a time are read along ow, split into the three planes, transposed through LDS and stored
// as 16-B halves, 32 B per position and plane.  The mw columns left of dY and the Gw - mw - OW right of it, whole
// halo rows, and -- by the last nkb workgroups -- the planes' tails are zero-filled.
__global__ __launch_bounds__(WD_T) void conv_wide_bwd_pack_dy_s2_k(const float* __restrict__ dy,
                                                                    uint8_t* __restrict__ dq, S2BwdPackDy a) {
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
  const int64_t row = b / a.nkb, n = row / a.Gh;
  const int oh = (int)(row - n * a.Gh) - a.mh;
  const int64_t plane = a.Ppad * 32;
  uint8_t* dst = dq + ((int64_t)kb * 3 * a.Ppad + row * a.Gw) * 32;   // plane 0 of this row
  if (oh < 0 || oh >= a.OH) {
    for (int i = tid; i < 6 * a.Gw; i += WD_T) {
      const int pl = i / (2 * a.Gw);
      store_zero16(dst + pl * plane + (i - pl * 2 * a.Gw) * 16);
    }
    return;
  }
  const int nz = 2 * (a.Gw - a.OW);   // halo halves of one plane's row: 2 mw on the left, the rest on the right
  for (int i = tid; i < 3 * nz; i += WD_T) {
    const int pl = i / nz, j = i - pl * nz;
    store_zero16(dst + pl * plane + (j < 2 * a.mw ? j : 2 * a.OW + j) * 16);
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
      *reinterpret_cast<uint4*>(dst + pl * plane + (2 * (a.mw + w0) + j) * 16) = make_uint4(s[0], s[1], s[2], s[3]);
    }
    __syncthreads();
  }
}

// One thread per 16-B half row of wq (8 output channels of one input channel and tap); the tap runs fastest
// over the threads, then the input channel, so a wave's 8 strided reads each sweep one contiguous piece of the
// latent weight.  Tap (kh, kw) = (2 s + a, 2 t + b) goes to row block 2 s KW + min(2, KH - 2 s) 2 t +
// a min(2, KW - 2 t) + b: the groups (s, t) in order, the taps of a group by (a, b).
__global__ __launch_bounds__(WD_T) void conv_wide_bwd_pack_w_s2_k(const float* __restrict__ w,
                                                                   uint8_t* __restrict__ wq, int64_t C, int64_t Co,
                                                                   int KH, int KW, int nkb) {
  const int taps = KH * KW;
  const int64_t idx = (int64_t)blockIdx.x * WD_T + threadIdx.x;
  if (idx >= (int64_t)nkb * 2 * C * taps) return;
  const int tap = (int)(idx % taps);
  int64_t q = idx / taps;
  const int64_t c = q % C;
  q /= C;
  const int half = (int)(q & 1);
  const int64_t kb = q >> 1;
  const int64_t co0 = kb * 16 + half * 8;
  uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int sv = co0 + j < Co ? tsign(w[((co0 + j) * C + c) * taps + tap]) : 0;
    o[j >> 1] |= (sv > 0 ? 0x3F80u : (sv < 0 ? 0xBF80u : 0u)) << (16 * (j & 1));
  }
  const int kh = tap / KW, kw = tap - kh * KW;
  const int ti = (kh & ~1) * KW + min(2, KH - (kh & ~1)) * (kw & ~1) + (kh & 1) * min(2, KW - (kw & ~1)) + (kw & 1);
  *reinterpret_cast<uint4*>(wq + ((kb * taps + ti) * C + c) * 32 + half * 16) = make_uint4(o[0], o[1], o[2], o[3]);
}

struct S2BwdGemm {
  const uint8_t* dq;
  const uint8_t* wq;
  float* dx;
  int64_t P, Ppad, GhGw, C, HW;
  int Gw, Hq, Wq, H, W, KH, KW, pad, mh, mw, taps, nkb, nct, arows;
};

// One shift group's operands: the weight fragment of each phase (a phase without a tap in the group repeats
// an earlier row block and is not used) and the six dY fragments, planes x position tiles.
struct S2BwdFrag {
  v4i w[4];
  v4i d[3][2];
};

// 4 waves as 2 (channel halves of 32) x 2 (position halves of 64); a wave holds, for each of the four phases,
// one 32-channel weight tile x two 32-position tiles: 8 accumulators.  As in §20 the weights are the MFMA's
// first operand and the positions its second, so register i of accumulator (phase, u) is channel (i & 3) +
// 8 (i >> 2) + 4 h of the wave's 32 at position 32 u + (lane & 31).  A stage is the three planes' windows (arows
// rows each), then taps x 64 weight rows.  The second launch bound keeps accumulators and fragments within 256
// registers, so that two workgroups share a CU where their stages do.
template <int NBUF>
__global__ __launch_bounds__(WD_T, 2) void conv_wide_bwd_data_s2_k(S2BwdGemm a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t wide_bwd_s2_smem[];
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int ct = (int)(blockIdx.x % a.nct);
  const int64_t p0 = (int64_t)(blockIdx.x / a.nct) * WD_TP;
  const int aplane = a.arows * 32;
  const int stage = 3 * aplane + a.taps * S2B_TC * 32;
  const int na = a.arows / 32, np = 3 * na + 2 * a.taps;   // 1-KiB pieces (32 rows): 3 windows, then 2 per tap
  // the global chunk that belongs in LDS chunk `lane` of a piece (pieces start on multiples of 32 rows)
  const int soff = (lane >> 1) * 32 + 16 * ((lane & 1) ^ ((lane >> 4) & 1));

  auto issue = [&](int kb, uint8_t* dst) {
    const uint8_t* ds = a.dq + ((int64_t)kb * 3 * a.Ppad + p0) * 32 + soff;
    const uint8_t* ws = a.wq + ((int64_t)kb * a.taps * a.C + ct * S2B_TC) * 32 + soff;
    for (int pc = wave; pc < np; pc += 4) {
      const int pl = (pc >= na) + (pc >= 2 * na), q = pc - 3 * na;
      glds16(q < 0 ? ds + (int64_t)pl * a.Ppad * 32 + (pc - pl * na) * 1024
                   : ws + ((int64_t)(q >> 1) * a.C + (q & 1) * 32) * 32,
             dst + pc * 1024);
    }
  };

  v16f acc[4][2];
#pragma unroll
  for (int ph = 0; ph < 4; ++ph)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[ph][u][i] = 0.f;

  const int woff = 3 * aplane + wide_row_off(wm * 32 + r, h);   // + 2048 per tap
  const int arow = wn * 64 + r;
  // group (s, t): the phases (0, 1), (1, 0), (1, 1) own a tap iff eb, ea, ea && eb; the group's taps are
  // consecutive 64-row blocks from tap index ti in that order
  auto load = [&](const uint8_t* buf, int s, int t, int ti, S2BwdFrag& f) {
    const int shift = (a.mh - s) * a.Gw + a.mw - t;
    const int ea = 2 * s + 1 < a.KH, eb = 2 * t + 1 < a.KW;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int o = wide_row_off(arow + shift + u * 32, h);
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) f.d[pl][u] = *reinterpret_cast<const v4i*>(buf + pl * aplane + o);
    }
    const uint8_t* wp = buf + woff + ti * 2048;
    f.w[0] = *reinterpret_cast<const v4i*>(wp);
    f.w[1] = *reinterpret_cast<const v4i*>(wp + eb * 2048);
    f.w[2] = *reinterpret_cast<const v4i*>(wp + ea * (1 + eb) * 2048);
    f.w[3] = *reinterpret_cast<const v4i*>(wp + (ea & eb) * 3 * 2048);
  };
  auto mac = [&](int s, int t, const S2BwdFrag& f) {
    const bool ea = 2 * s + 1 < a.KH, eb = 2 * t + 1 < a.KW;
#pragma unroll
    for (int ph = 0; ph < 4; ++ph) {   // static: a run-time phase index would put the accumulators in scratch
      if ((ph & 2) && !ea) continue;   // wave-uniform: this tap exists
      if ((ph & 1) && !eb) continue;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)   // fixed plane order: d1, d2, d3
#pragma unroll
        for (int u = 0; u < 2; ++u)
          acc[ph][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, f.w[ph]),
                                                               __builtin_bit_cast(v8bf, f.d[pl][u]), acc[ph][u], 0, 0, 0);
    }
  };
  // the walk over the groups, two per trip so that the two fragment sets swap roles without copies: the next
  // group's ten fragments are read under the current group's MFMAs
  auto compute = [&](const uint8_t* buf) {
    S2BwdFrag f0, f1;
    int s = 0, t = 0, ti = 0;
    auto next = [&](int& s1, int& t1, int& ti1) {
      ti1 = ti + (1 + (2 * s + 1 < a.KH)) * (1 + (2 * t + 1 < a.KW));
      s1 = s, t1 = t + 1;
      if (t1 > a.mw) t1 = 0, ++s1;
    };
    load(buf, 0, 0, 0, f0);
    for (;;) {
      int s1, t1, ti1;
      next(s1, t1, ti1);
      const bool more1 = s1 <= a.mh;
      if (more1) load(buf, s1, t1, ti1, f1);
      mac(s, t, f0);
      if (!more1) break;
      s = s1, t = t1, ti = ti1;
      next(s1, t1, ti1);
      const bool more0 = s1 <= a.mh;
      if (more0) load(buf, s1, t1, ti1, f0);
      mac(s, t, f1);
      if (!more0) break;
      s = s1, t = t1, ti = ti1;
    }
  };

  if constexpr (NBUF == 2) {
    issue(0, wide_bwd_s2_smem);
    for (int kb = 0; kb < a.nkb; ++kb) {
      wide_wait_dma();
      wide_barrier();   // block kb is in LDS; every wave has left block kb-1, whose buffer is refilled next
      if (kb + 1 < a.nkb) issue(kb + 1, wide_bwd_s2_smem + ((kb + 1) & 1) * stage);
      compute(wide_bwd_s2_smem + (kb & 1) * stage);
    }
  } else {
    for (int kb = 0; kb < a.nkb; ++kb) {
      if (kb > 0) wide_barrier();
      issue(kb, wide_bwd_s2_smem);
      wide_wait_dma();
      wide_barrier();
      compute(wide_bwd_s2_smem);
    }
  }

  // cell (i, j) of phase (a, b) is input pixel (2 i + a - pad, 2 j + b - pad); cells beyond Hq x Wq or P and
  // pixels outside the image are computed and not stored.  A phase without taps stores its zeros.
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int64_t p = p0 + wn * 64 + u * 32 + r;
    const int64_t n = p / a.GhGw;
    const int rem = (int)(p - n * a.GhGw), i = rem / a.Gw, j = rem - i * a.Gw;
    if (p >= a.P || i >= a.Hq || j >= a.Wq) continue;
    float* xn = a.dx + (n * a.C + ct * S2B_TC + wm * 32 + 4 * h) * a.HW;
#pragma unroll
    for (int ph = 0; ph < 4; ++ph) {
      const int ih = 2 * i + (ph >> 1) - a.pad, iw = 2 * j + (ph & 1) - a.pad;
      if (ih < 0 || ih >= a.H || iw < 0 || iw >= a.W) continue;
      float* xp = xn + ih * a.W + iw;
#pragma unroll
      for (int k = 0; k < 16; ++k) xp[((k & 3) + 8 * (k >> 2)) * a.HW] = acc[ph][u][k];
    }
  }
}

int g_s2_bwd_stages = 7;   // bnn_conv2d_bwd_data_wide_s2_set_stages

template <int NBUF>
void s2_bwd_launch(const S2BwdPlan& p, const S2BwdGemm& a, hipStream_t st) {
  if (p.lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wide_bwd_data_s2_k<NBUF>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
  hipLaunchKernelGGL((conv_wide_bwd_data_s2_k<NBUF>), dim3((unsigned)(p.ntile * p.nct)), dim3(WD_T), (size_t)p.lds, st,
                     a);
}

}  // namespace
}  // namespace bnn

using namespace bnn;

BNN_API int bnn_conv2d_bwd_data_wide_s2_ok(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH,
                                           int64_t KW, int32_t stride, int32_t pad, int32_t dil, int32_t groups) {
  S2BwdPlan p;
  return s2_bwd_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p) ? 1 : 0;
}

BNN_API int64_t bnn_conv2d_bwd_data_wide_s2_workspace(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co,
                                                      int64_t KH, int64_t KW, int32_t pad) {
  S2BwdPlan p;
  return s2_bwd_plan(N, C, H, W, Co, KH, KW, 2, pad, 1, 1, &p) ? p.work_bytes : 0;
}

BNN_API const char* bnn_conv2d_bwd_data_wide_s2_kernel(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co,
                                                       int64_t KH, int64_t KW, int32_t stride, int32_t pad,
                                                       int32_t dil, int32_t groups) {
  static thread_local char buf[96];
  S2BwdPlan p;
  if (!s2_bwd_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p)) return "";
  snprintf(buf, sizeof(buf), "conv_wide_bwd_data_s2_k<%d> lds=%lld b128=%d", p.nbuf, (long long)p.lds, p.cycles);
  return buf;
}

BNN_API int bnn_conv2d_bwd_data_wide_s2_set_stages(int32_t mask) {
  if (mask >= 0) g_s2_bwd_stages = mask & 7;
  return g_s2_bwd_stages;
}

BNN_API int bnn_conv2d_bwd_data_wide_s2(const float* dy, const float* w_latent, float* dx, int64_t N, int64_t C,
                                        int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride,
                                        int32_t pad, int32_t dil, int32_t groups, void* work, int64_t work_bytes,
                                        void* stream) {
  S2BwdPlan p;
  if (!s2_bwd_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p)) {
    set_error("bnn_conv2d_bwd_data_wide_s2: shape not taken (a shape of bnn_conv2d_fwd_wide_s2 whose three dY "
              "windows and KH KW x 64 weight rows of one 16-channel block fit the LDS)");
    return kErrInval;
  }
  if (!dy || !w_latent || !dx || !work || !aligned16(work) || work_bytes < p.work_bytes) {
    set_error("bnn_conv2d_bwd_data_wide_s2: null pointer, or a workspace not 16-B aligned or below "
              "bnn_conv2d_bwd_data_wide_s2_workspace = %lld bytes", (long long)p.work_bytes);
    return kErrInval;
  }
  if (N == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint8_t* dq = static_cast<uint8_t*>(work);
  uint8_t* wq = dq + p.wq_off;
  const S2BwdPackDy py{Co, p.P, p.Ppad, N * p.Gh, p.OH, p.OW, p.Gh, p.Gw, p.mh, p.mw, p.nkb};
  if (g_s2_bwd_stages & 1)
    hipLaunchKernelGGL(conv_wide_bwd_pack_dy_s2_k, dim3((unsigned)((py.rows + 1) * p.nkb)), dim3(WD_T), 0, st, dy, dq,
                       py);
  const int64_t nw = (int64_t)p.nkb * 2 * C * p.taps;
  if (g_s2_bwd_stages & 2)
    hipLaunchKernelGGL(conv_wide_bwd_pack_w_s2_k, dim3((unsigned)((nw + WD_T - 1) / WD_T)), dim3(WD_T), 0, st,
                       w_latent, wq, C, Co, p.KH, p.KW, p.nkb);
  const S2BwdGemm g{dq,   wq,   dx,   p.P, p.Ppad, (int64_t)p.Gh * p.Gw, C,    H * W,  p.Gw,   p.Hq,  p.Wq,
                    (int)H, (int)W, p.KH, p.KW, p.pad,  p.mh,                 p.mw, p.taps, p.nkb, p.nct, p.arows};
  if (!(g_s2_bwd_stages & 4)) return check_launch("bnn_conv2d_bwd_data_wide_s2");
  if (p.nbuf == 2) s2_bwd_launch<2>(p, g, st);
  else s2_bwd_launch<1>(p, g, st);
  return check_launch("bnn_conv2d_bwd_data_wide_s2");
}
