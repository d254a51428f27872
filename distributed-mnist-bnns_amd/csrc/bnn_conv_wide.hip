// Wide-channel binary conv2d forward (C % 64 == 0, C > 64 or Co > 64; stride 1, dilation 1, one
// group): BinarizeConv2d.forward (models/binarized_modules.py:93-107) with a binarised input, as a
// ternary implicit GEMM on v_mfma_scale_f32_32x32x64_f8f6f4 with FP4 (e2m1) operands and unit scales
// (DESIGN.md §19).  Three launches per call:
//
//  1. conv_wide_pack_x_k   x fp32 NCHW -> FP4 codes on the zero-padded grid, one plane per 64-channel
//                          block: xq [C/64][Ppad][32 B], position p = (n Hp + hp) Wp + wp.  Halo
//                          positions and the tail P .. Ppad-1 are written as zeros on every call.
//  2. conv_wide_pack_w_k   latent w fp32 [Co][C][KH][KW] -> wq [C/64][KH KW][Cop][32 B], rows Co .. Cop-1 zero.
//  3. conv_wide_gemm_k     shifted-window GEMM on the padded grid: output position p needs, for tap
//                          (kh, kw), packed position p + kh Wp + kw -- zero padding is FP4 code 0, so no
//                          border is special.  A workgroup owns 128 consecutive positions x 128 output
//                          channels; per channel block it copies the positions p0 .. p0 + arows - 1 (one
//                          contiguous run of the plane) and the block's weights of every tap into LDS
//                          with global_load_lds_dwordx4, then runs the KH KW taps out of LDS, one MFMA
//                          per 32 x 32 tile and tap.  Products of codes are exact and |sum| < 2^24, so the
//                          fp32 accumulator holds the exact integer I; y = fl(I + bias[co]).
//
// LDS rows are 32 B (one position or one output channel of a 64-channel block).  A fragment read is
// one ds_read_b128 per lane: lane (r = lane & 31, h = lane >> 5) reads half h of row base + r.  Plain
// 32-B rows put rows r and r + 8 of a 16-lane group on the same banks; storing half h of row R in
// chunk h ^ ((R >> 3) & 1) separates them for every base, i.e. every tap shift (wide_frag_cycles
// checks this with the bank model of bnn_lds_model.h).  The LDS-DMA writes 1 KiB runs, so the
// swizzle is applied on the global side of the copy.
#include "bnn_conv_wide.h"

#include <cstdio>

#include "bnn.h"

namespace bnn {
namespace {

struct WidePlan {
  int64_t N, C, H, W, Co;
  int KH, KW, pad, Hp, Wp, OH, OW, taps, ncb, nct, Cop;
  int tail;       // (KH-1) Wp + KW-1: the largest tap shift
  int arows;      // activation rows a workgroup stages per channel block, a multiple of 32
  int nbuf;       // LDS stages: 2 = the next block's copy runs under this block's MFMAs, 1 = it does not fit
  int cycles;     // modelled LDS cycles of the worst fragment ds_read_b128 (4 = conflict-free)
  int64_t P;      // N Hp Wp positions of the padded grid
  int64_t Ppad;   // positions per plane: the last tile's window stays inside it
  int64_t ntile, lds, wq_off, work_bytes;
};

// The one decision function: bnn_conv2d_fwd_wide_ok, the workspace and kernel queries and the launch.
bool wide_plan(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride,
               int32_t pad, int32_t dil, int32_t groups, WidePlan* out) {
  if (N < 0 || C <= 0 || H <= 0 || W <= 0 || Co <= 0 || KH <= 0 || KW <= 0 || pad < 0) return false;
  if (groups != 1 || stride != 1 || dil != 1 || pad > std::min(KH, KW) - 1) return false;
  if (C % 64 != 0 || (C <= 64 && Co <= 64) || C * KH * KW >= (1 << 24)) return false;
  if (H + 2 * pad < KH || W + 2 * pad < KW || H > (1 << 20) || W > (1 << 20) || KH > 64 || KW > 64 ||
      N >= (1ll << 31) || Co > (1 << 20) || (H + 2 * pad) * (W + 2 * pad) >= (1ll << 31))
    return false;
  WidePlan p{};
  p.N = N, p.C = C, p.H = H, p.W = W, p.Co = Co;
  p.KH = (int)KH, p.KW = (int)KW, p.pad = pad;
  p.Hp = (int)H + 2 * pad, p.Wp = (int)W + 2 * pad;
  p.OH = p.Hp - p.KH + 1, p.OW = p.Wp - p.KW + 1;
  p.taps = p.KH * p.KW, p.ncb = (int)(C / 64);
  p.Cop = (int)round_up(Co, WD_TC), p.nct = p.Cop / WD_TC;
  const int64_t tail = (int64_t)(p.KH - 1) * p.Wp + p.KW - 1;
  const int64_t arows = round_up(WD_TP + tail, 32);
  p.lds = (arows + (int64_t)p.taps * WD_TC) * 32;
  if (p.lds > kWideMaxLds) return false;
  p.tail = (int)tail, p.arows = (int)arows;
  p.nbuf = 2 * p.lds <= kWideMaxLds ? 2 : 1;
  p.lds *= p.nbuf;
  p.cycles = wide_frag_cycles(p.KH, p.KW, p.Wp);
  p.P = N * p.Hp * p.Wp;
  p.ntile = (p.P + WD_TP - 1) / WD_TP;
  p.Ppad = p.ntile * WD_TP - WD_TP + arows;
  // grids are 1-D: GEMM tiles, and one pack block per padded row and channel block
  if (p.ntile * p.nct >= (1ll << 31) || (N * p.Hp + 1) * p.ncb >= (1ll << 31) || Co * p.OH * p.OW >= (1ll << 31))
    return false;
  p.wq_off = round_up((int64_t)p.ncb * p.Ppad * 32, 256);
  p.work_bytes = p.wq_off + (int64_t)p.ncb * p.taps * p.Cop * 32;
  *out = p;
  return true;
}

struct WidePackX {
  int64_t C, H, W, P, Ppad, rows;   // rows = N Hp
  int pad, Hp, Wp, ncb;
};

// One workgroup per (padded row, channel block): 64 channels x up to 64 columns at a time are read
// along W, turned into codes, transposed through LDS ([w][64 B + 4]: the byte writes of a wave run
// along w at a stride of 17 dwords) and stored as two 16-B halves per position.  The row's halo
// columns, whole halo rows, and -- by the last ncb workgroups -- the planes' tails are zero-filled.
__global__ __launch_bounds__(WD_T) void conv_wide_pack_x_k(const float* __restrict__ x, uint8_t* __restrict__ xq,
                                                            WidePackX a) {
  __shared__ uint32_t tile[64 * 17];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (b >= a.rows * a.ncb) {
    uint8_t* dst = xq + ((b - a.rows * a.ncb) * a.Ppad + a.P) * 32;
    for (int64_t i = tid; i < (a.Ppad - a.P) * 2; i += WD_T) store_zero16(dst + i * 16);
    return;
  }
  const int cb = (int)(b % a.ncb);
  const int64_t row = b / a.ncb, n = row / a.Hp;
  const int ih = (int)(row - n * a.Hp) - a.pad;
  uint8_t* dst = xq + ((int64_t)cb * a.Ppad + row * a.Wp) * 32;
  if (ih < 0 || ih >= a.H) {
    for (int i = tid; i < 2 * a.Wp; i += WD_T) store_zero16(dst + i * 16);
    return;
  }
  for (int i = tid; i < 4 * a.pad; i += WD_T)
    store_zero16(dst + (i < 2 * a.pad ? i : 2 * (int)a.W + i) * 16);
  const int64_t HW = a.H * a.W;
  const float* xr = x + ((n * a.C + cb * 64) * a.H + ih) * a.W;
  uint8_t* tb = reinterpret_cast<uint8_t*>(tile);
  for (int w0 = 0; w0 < a.W; w0 += 64) {
    const int wc = min(64, (int)a.W - w0);
    for (int i = tid; i < 64 * wc; i += WD_T) {
      const int c = i / wc, w = i - c * wc;
      tb[w * 68 + c] = (uint8_t)fp4_code(tsign(xr[c * HW + w0 + w]));
    }
    __syncthreads();
    if (tid < 2 * wc) {
      const uint32_t* s = tile + (tid >> 1) * 17 + (tid & 1) * 8;
      uint4 o;
      o.x = squeeze4(s[0]) | squeeze4(s[1]) << 16;
      o.y = squeeze4(s[2]) | squeeze4(s[3]) << 16;
      o.z = squeeze4(s[4]) | squeeze4(s[5]) << 16;
      o.w = squeeze4(s[6]) | squeeze4(s[7]) << 16;
      *reinterpret_cast<uint4*>(dst + (2 * (a.pad + w0) + tid) * 16) = o;
    }
    __syncthreads();
  }
}

// One thread per 16-B half row of wq; the tap runs fastest over the threads, so a wave's 32 strided
// reads sweep one contiguous piece of the latent weight.
__global__ __launch_bounds__(WD_T) void conv_wide_pack_w_k(const float* __restrict__ w, uint8_t* __restrict__ wq,
                                                            int64_t C, int64_t Co, int Cop, int taps, int ncb) {
  const int64_t idx = (int64_t)blockIdx.x * WD_T + threadIdx.x;
  if (idx >= (int64_t)Cop * ncb * 2 * taps) return;
  const int tap = (int)(idx % taps);
  int64_t q = idx / taps;
  const int half = (int)(q & 1);
  q >>= 1;
  const int cb = (int)(q % ncb);
  const int64_t co = q / ncb;
  uint32_t o[4] = {0u, 0u, 0u, 0u};
  if (co < Co) {
    const float* s = w + (co * C + cb * 64 + half * 32) * taps + tap;
#pragma unroll
    for (int j = 0; j < 32; ++j) o[j >> 3] |= fp4_code(tsign(s[(int64_t)j * taps])) << (4 * (j & 7));
  }
  *reinterpret_cast<uint4*>(wq + (((int64_t)cb * taps + tap) * Cop + co) * 32 + half * 16) = make_uint4(o[0], o[1], o[2], o[3]);
}

struct WideGemm {
  const uint8_t* xq;
  const uint8_t* wq;
  const float* bias;
  float* y;
  int64_t P, Ppad, HpWp, Co, OHW;
  int Wp, OH, OW, Cop, KW, taps, ncb, nct, arows;
};

// 4 waves as 2 (output channels) x 2 (positions), each 64 x 64 as 2 x 2 MFMA tiles.  The weights are
// the MFMA's first operand and the positions its second, so an accumulator register is an output
// channel and the lanes run along positions: register i of tile (t, u) is channel
// 32 t + (i & 3) + 8 (i >> 2) + 4 h at position 32 u + (lane & 31), and an NCHW store is a run along ow.
template <int NBUF>
__global__ __launch_bounds__(WD_T) void conv_wide_gemm_k(WideGemm a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t wide_smem[];
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int ct = (int)(blockIdx.x % a.nct);
  const int64_t p0 = (int64_t)(blockIdx.x / a.nct) * WD_TP;
  const int stage = (a.arows + a.taps * WD_TC) * 32;
  const int na = a.arows / 32, np = na + 4 * a.taps;   // 1-KiB pieces (32 rows): activations, then 4 per tap
  // the global chunk that belongs in LDS chunk `lane` of a piece (pieces start on multiples of 32 rows)
  const int soff = (lane >> 1) * 32 + 16 * ((lane & 1) ^ ((lane >> 4) & 1));

  auto issue = [&](int cb, uint8_t* dst) {
    const uint8_t* xs = a.xq + ((int64_t)cb * a.Ppad + p0) * 32 + soff;
    const uint8_t* ws = a.wq + ((int64_t)cb * a.taps * a.Cop + ct * WD_TC) * 32 + soff;
    for (int pc = wave; pc < np; pc += 4) {
      const int q = pc - na;
      glds16(pc < na ? xs + pc * 1024 : ws + ((int64_t)(q >> 2) * a.Cop + (q & 3) * 32) * 32, dst + pc * 1024);
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
  const int arow = wn * 64 + r;
  auto frags = [&](const uint8_t* buf, int tap, int shift, v4i (&wf)[2], v4i (&af)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t) wf[t] = *reinterpret_cast<const v4i*>(buf + woff + tap * 4096 + t * 1024);
#pragma unroll
    for (int u = 0; u < 2; ++u) af[u] = *reinterpret_cast<const v4i*>(buf + wide_row_off(arow + shift + u * 32, h));
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

  // positions of the halo (oh >= OH or ow >= OW) and beyond P are computed and not stored
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int64_t p = p0 + wn * 64 + u * 32 + r;
    const int64_t n = p / a.HpWp;
    const int rem = (int)(p - n * a.HpWp), oh = rem / a.Wp, ow = rem - oh * a.Wp;
    if (p >= a.P || oh >= a.OH || ow >= a.OW) continue;
    float* yp = a.y + n * a.Co * a.OHW + oh * a.OW + ow;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int co = ct * WD_TC + wm * 64 + t * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (co < a.Co) yp[co * a.OHW] = a.bias != nullptr ? acc[t][u][i] + a.bias[co] : acc[t][u][i];
      }
  }
}

int g_wide_stages = 7;   // bnn_conv2d_fwd_wide_set_stages

const char* wide_gemm_name(const WidePlan& p) { return p.nbuf == 2 ? "conv_wide_gemm_k<2>" : "conv_wide_gemm_k<1>"; }

template <int NBUF>
void wide_gemm_launch(const WidePlan& p, const WideGemm& a, hipStream_t st) {
  if (p.lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wide_gemm_k<NBUF>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
  hipLaunchKernelGGL((conv_wide_gemm_k<NBUF>), dim3((unsigned)(p.ntile * p.nct)), dim3(WD_T), (size_t)p.lds, st, a);
}

}  // namespace
}  // namespace bnn

using namespace bnn;

BNN_API int bnn_conv2d_fwd_wide_ok(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW,
                                   int32_t stride, int32_t pad, int32_t dil, int32_t groups) {
  WidePlan p;
  return wide_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p) ? 1 : 0;
}

BNN_API int64_t bnn_conv2d_fwd_wide_workspace(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH,
                                              int64_t KW, int32_t pad) {
  WidePlan p;
  return wide_plan(N, C, H, W, Co, KH, KW, 1, pad, 1, 1, &p) ? p.work_bytes : 0;
}

BNN_API const char* bnn_conv2d_fwd_wide_kernel(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH,
                                               int64_t KW, int32_t stride, int32_t pad, int32_t dil, int32_t groups) {
  static thread_local char buf[96];
  WidePlan p;
  if (!wide_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p)) return "";
  snprintf(buf, sizeof(buf), "%s lds=%lld b128=%d", wide_gemm_name(p), (long long)p.lds, p.cycles);
  return buf;
}

// The two packed operands as entries of their own (frozen inference packs a weight once and an input only
// in front of the first layer, bnn_conv_wide_infer.hip): the layouts, sizes and kernels of this unit.  The
// planes of an activation do not depend on the consumer's Co, so its plan is made for one 128-row tile.
BNN_API int64_t bnn_conv2d_wide_planes_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t KH, int64_t KW,
                                             int32_t pad) {
  WidePlan p;
  return wide_plan(N, C, H, W, WD_TC, KH, KW, 1, pad, 1, 1, &p) ? (int64_t)p.ncb * p.Ppad * 32 : 0;
}

BNN_API int64_t bnn_conv2d_wide_wq_bytes(int64_t C, int64_t Co, int64_t KH, int64_t KW) {
  if (C <= 0 || C % 64 != 0 || Co <= 0 || Co > (1 << 20) || KH <= 0 || KW <= 0 || KH > 64 || KW > 64 ||
      C * KH * KW >= (1 << 24))
    return 0;
  return C / 64 * KH * KW * round_up(Co, WD_TC) * 32;
}

BNN_API int bnn_conv2d_wide_pack_w(const float* w_latent, void* wq, int64_t C, int64_t Co, int64_t KH, int64_t KW,
                                   void* stream) {
  if (bnn_conv2d_wide_wq_bytes(C, Co, KH, KW) == 0 || !w_latent || !wq || !aligned16(wq)) {
    set_error("bnn_conv2d_wide_pack_w: null or unaligned pointer, or C %% 64 != 0 / C KH KW >= 2^24");
    return kErrInval;
  }
  const int Cop = (int)round_up(Co, WD_TC), taps = (int)(KH * KW), ncb = (int)(C / 64);
  const int64_t nw = (int64_t)Cop * ncb * 2 * taps;
  hipLaunchKernelGGL(conv_wide_pack_w_k, dim3((unsigned)((nw + WD_T - 1) / WD_T)), dim3(WD_T), 0,
                     reinterpret_cast<hipStream_t>(stream), w_latent, static_cast<uint8_t*>(wq), C, Co, Cop, taps, ncb);
  return check_launch("bnn_conv2d_wide_pack_w");
}

BNN_API int bnn_conv2d_wide_pack_x(const float* x, void* planes, int64_t N, int64_t C, int64_t H, int64_t W,
                                   int64_t KH, int64_t KW, int32_t pad, void* stream) {
  WidePlan p;
  if (!wide_plan(N, C, H, W, WD_TC, KH, KW, 1, pad, 1, 1, &p) || !x || !planes || !aligned16(planes)) {
    set_error("bnn_conv2d_wide_pack_x: null or unaligned pointer, or a geometry bnn_conv2d_wide_planes_bytes "
              "gives 0 bytes for");
    return kErrInval;
  }
  if (N == 0) return 0;
  const WidePackX px{C, H, W, p.P, p.Ppad, N * p.Hp, p.pad, p.Hp, p.Wp, p.ncb};
  hipLaunchKernelGGL(conv_wide_pack_x_k, dim3((unsigned)((px.rows + 1) * p.ncb)), dim3(WD_T), 0,
                     reinterpret_cast<hipStream_t>(stream), x, static_cast<uint8_t*>(planes), px);
  return check_launch("bnn_conv2d_wide_pack_x");
}

BNN_API int bnn_conv2d_fwd_wide_set_stages(int32_t mask) {
  if (mask >= 0) g_wide_stages = mask & 7;
  return g_wide_stages;
}

BNN_API int bnn_conv2d_fwd_wide(const float* x, const float* w_latent, const float* bias, float* y, int64_t N,
                                int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride,
                                int32_t pad, int32_t dil, int32_t groups, void* work, int64_t work_bytes,
                                void* stream) {
  WidePlan p;
  if (!wide_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p)) {
    set_error("bnn_conv2d_fwd_wide: shape not taken (stride 1, dilation 1, one group, pad <= K - 1, C %% 64 == 0, "
              "C > 64 or Co > 64, C KH KW < 2^24, one channel block's window and taps within the LDS)");
    return kErrInval;
  }
  if (!x || !w_latent || !y || !work || !aligned16(work) || work_bytes < p.work_bytes) {
    set_error("bnn_conv2d_fwd_wide: null pointer, or a workspace not 16-B aligned or below "
              "bnn_conv2d_fwd_wide_workspace = %lld bytes", (long long)p.work_bytes);
    return kErrInval;
  }
  if (N == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint8_t* xq = static_cast<uint8_t*>(work);
  uint8_t* wq = xq + p.wq_off;
  const WidePackX px{C, H, W, p.P, p.Ppad, N * p.Hp, p.pad, p.Hp, p.Wp, p.ncb};
  if (g_wide_stages & 1)
    hipLaunchKernelGGL(conv_wide_pack_x_k, dim3((unsigned)((px.rows + 1) * p.ncb)), dim3(WD_T), 0, st, x, xq,
                       px);
  const int64_t nw = (int64_t)p.Cop * p.ncb * 2 * p.taps;
  if (g_wide_stages & 2)
    hipLaunchKernelGGL(conv_wide_pack_w_k, dim3((unsigned)((nw + WD_T - 1) / WD_T)), dim3(WD_T), 0, st, w_latent, wq,
                       C, Co, p.Cop, p.taps, p.ncb);
  const WideGemm g{xq, wq, bias, y, p.P, p.Ppad, (int64_t)p.Hp * p.Wp, Co, (int64_t)p.OH * p.OW,
                   p.Wp, p.OH, p.OW, p.Cop, p.KW, p.taps, p.ncb, p.nct, p.arows};
  if (!(g_wide_stages & 4)) return check_launch("bnn_conv2d_fwd_wide");
  if (p.nbuf == 2) wide_gemm_launch<2>(p, g, st);
  else wide_gemm_launch<1>(p, g, st);
  return check_launch("bnn_conv2d_fwd_wide");
}

// The same forward on planes the caller owns (the training hand-off, bnn_conv_wide_handoff.hip): the weight
// pack and the GEMM above, the workspace holding wq only.
BNN_API int64_t bnn_conv2d_fwd_wide_planes_workspace(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co,
                                                     int64_t KH, int64_t KW, int32_t pad) {
  WidePlan p;
  return wide_plan(N, C, H, W, Co, KH, KW, 1, pad, 1, 1, &p) ? p.work_bytes - p.wq_off : 0;
}

BNN_API int bnn_conv2d_fwd_wide_planes(const void* planes, const float* w_latent, const float* bias, float* y,
                                       int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW,
                                       int32_t pad, void* work, int64_t work_bytes, void* stream) {
  WidePlan p;
  if (!wide_plan(N, C, H, W, Co, KH, KW, 1, pad, 1, 1, &p)) {
    set_error("bnn_conv2d_fwd_wide_planes: shape not taken (the shapes of bnn_conv2d_fwd_wide at stride 1, "
              "dilation 1, one group)");
    return kErrInval;
  }
  if (!planes || !aligned16(planes) || !w_latent || !y || !work || !aligned16(work) ||
      work_bytes < p.work_bytes - p.wq_off) {
    set_error("bnn_conv2d_fwd_wide_planes: null pointer, planes not 16-B aligned, or a workspace not 16-B aligned "
              "or below bnn_conv2d_fwd_wide_planes_workspace = %lld bytes", (long long)(p.work_bytes - p.wq_off));
    return kErrInval;
  }
  if (N == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint8_t* wq = static_cast<uint8_t*>(work);
  const int64_t nw = (int64_t)p.Cop * p.ncb * 2 * p.taps;
  hipLaunchKernelGGL(conv_wide_pack_w_k, dim3((unsigned)((nw + WD_T - 1) / WD_T)), dim3(WD_T), 0, st, w_latent, wq, C,
                     Co, p.Cop, p.taps, p.ncb);
  const WideGemm g{static_cast<const uint8_t*>(planes), wq, bias, y, p.P, p.Ppad, (int64_t)p.Hp * p.Wp, Co,
                   (int64_t)p.OH * p.OW, p.Wp, p.OH, p.OW, p.Cop, p.KW, p.taps, p.ncb, p.nct, p.arows};
  if (p.nbuf == 2) wide_gemm_launch<2>(p, g, st);
  else wide_gemm_launch<1>(p, g, st);
  return check_launch("bnn_conv2d_fwd_wide_planes");
}
