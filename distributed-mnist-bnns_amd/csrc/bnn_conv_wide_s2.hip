// Wide-channel binary conv2d forward at stride 2 (C % 64 == 0, C > 64 or Co > 64; dilation 1, one group):
// the downsampling 3x3 / 1x1 layers of the ResNet-style binarized networks, as a ternary implicit GEMM on
// v_mfma_scale_f32_32x32x64_f8f6f4 with FP4 (e2m1) operands and unit scales.
//
// On the padded grid a stride-2 output does not see its taps at a constant offset from a contiguous run of
// outputs, so the padded input is split into its four parity phases: phase (a, b) holds padded pixel
// (2i + a, 2j + b) at phase-grid cell (i, j), Hq = ceil(Hp / 2) x Wq = ceil(Wp / 2) cells per image.  Output
// (i, j), tap (kh, kw) reads padded pixel (2i + kh, 2j + kw) = phase (kh & 1, kw & 1), cell (i + (kh >> 1),
// j + (kw >> 1)): with q = (n Hq + i) Wq + j every tap is one phase plus the constant shift
// (kh >> 1) Wq + (kw >> 1), zero padding is FP4 code 0, and a tile's outputs are consecutive q.
//
// Three launches per call:
//  1. conv_wide_pack_x_s2_k  x fp32 NCHW -> xs [C/64][nph][Qpad][32 B], nph = min(KH, 2) min(KW, 2) phases
//                            that own a tap, phase index f = (kh & 1) min(KW, 2) + (kw & 1).  Halo cells, the
//                            extra row / column of an odd Hp / Wp and the tails Q .. Qpad-1 are zeros.
//  2. conv_wide_pack_w_k     (bnn_conv_wide.hip, through bnn_conv2d_wide_pack_w) -> wq [C/64][KH KW][Cop][32 B].
//  3. conv_wide_gemm_s2_k    a workgroup owns 128 consecutive q x 128 output channels; per channel block it
//                            copies nph windows of arows positions (one per phase, each a contiguous run of
//                            its plane from the tile's q0) and the block's weights of every tap into LDS with
//                            global_load_lds_dwordx4, then runs the KH KW taps out of LDS, one MFMA per 32 x 32
//                            tile and tap.  y = fl(I + bias[co]) with I the exact integer sum.
//
// LDS rows, the half swizzle and the fragment reads are bnn_conv_wide.hip's; arows is a multiple of 32, so a
// phase base changes no bit 3 of a row and the swizzle stays conflict-free for every (phase, shift).
#include "bnn_conv_wide.h"

#include <cstdio>

#include "bnn.h"

namespace bnn {
namespace {

struct S2Plan {
  int64_t N, C, H, W, Co;
  int KH, KW, pad, Hp, Wp, Hq, Wq, OH, OW, taps, ncb, nct, Cop;
  int nphw, nph;  // phases along kw that own a tap, and in all
  int arows;      // rows of one phase window, a multiple of 32
  int nbuf;       // LDS stages
  int cycles;     // modelled LDS cycles of the worst fragment ds_read_b128 (4 = conflict-free)
  int64_t Q;      // N Hq Wq positions of the phase grid
  int64_t Qpad;   // positions per plane: the last tile's window stays inside it
  int64_t ntile, lds, wq_off, work_bytes;
};

// LDS row of tap (kh, kw)'s activation fragment base: its phase's window plus its shift
inline int s2_tap_row(int kh, int kw, int nphw, int arows, int Wq) {
  return ((kh & 1) * nphw + (kw & 1)) * arows + (kh >> 1) * Wq + (kw >> 1);
}

// The one decision function: bnn_conv2d_fwd_wide_s2_ok, the workspace and kernel queries and the launch.
// pad <= max(KH, KW) - 1: a 1 x 3 kernel with pad 1 is a shape of the family (the layout has no use for a
// bound on pad; the wq pack and §19's integer bounds are shared).
bool wide_s2_plan(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride,
                  int32_t pad, int32_t dil, int32_t groups, S2Plan* out) {
  if (N < 0 || C <= 0 || H <= 0 || W <= 0 || Co <= 0 || KH <= 0 || KW <= 0 || pad < 0) return false;
  if (groups != 1 || stride != 2 || dil != 1 || pad > std::max(KH, KW) - 1) return false;
  if (C % 64 != 0 || (C <= 64 && Co <= 64) || C * KH * KW >= (1 << 24)) return false;
  if (H + 2 * pad < KH || W + 2 * pad < KW || H > (1 << 20) || W > (1 << 20) || KH > 64 || KW > 64 ||
      N >= (1ll << 31) || Co > (1 << 20) || (H + 2 * pad) * (W + 2 * pad) >= (1ll << 31))
    return false;
  S2Plan p{};
  p.N = N, p.C = C, p.H = H, p.W = W, p.Co = Co;
  p.KH = (int)KH, p.KW = (int)KW, p.pad = pad;
  p.Hp = (int)H + 2 * pad, p.Wp = (int)W + 2 * pad;
  p.Hq = (p.Hp + 1) / 2, p.Wq = (p.Wp + 1) / 2;
  p.OH = (p.Hp - p.KH) / 2 + 1, p.OW = (p.Wp - p.KW) / 2 + 1;
  p.taps = p.KH * p.KW, p.ncb = (int)(C / 64);
  p.Cop = (int)round_up(Co, WD_TC), p.nct = p.Cop / WD_TC;
  p.nphw = std::min(p.KW, 2), p.nph = std::min(p.KH, 2) * p.nphw;
  const int64_t tail = (int64_t)((p.KH - 1) >> 1) * p.Wq + ((p.KW - 1) >> 1);
  const int64_t arows = round_up(WD_TP + tail, 32);
  p.lds = (p.nph * arows + (int64_t)p.taps * WD_TC) * 32;
  if (p.lds > kWideMaxLds) return false;
  p.arows = (int)arows;
  p.nbuf = 2 * p.lds <= kWideMaxLds ? 2 : 1;
  p.lds *= p.nbuf;
  for (int kh = 0; kh < p.KH; ++kh)
    for (int kw = 0; kw < p.KW; ++kw) {
      int addr[64];
      for (int l = 0; l < 64; ++l)
        addr[l] = wide_row_off(s2_tap_row(kh, kw, p.nphw, p.arows, p.Wq) + (l & 31), l >> 5);
      p.cycles = std::max(p.cycles, lds_b128_cycles(addr));
    }
  p.Q = N * p.Hq * p.Wq;
  p.ntile = (p.Q + WD_TP - 1) / WD_TP;
  p.Qpad = p.ntile * WD_TP - WD_TP + arows;
  // grids are 1-D: GEMM tiles, and one pack block per phase-grid row pair and channel block
  if (p.ntile * p.nct >= (1ll << 31) || (N * 2 * p.Hq + p.nph) * p.ncb >= (1ll << 31) ||
      Co * p.OH * p.OW >= (1ll << 31))
    return false;
  p.wq_off = round_up((int64_t)p.ncb * p.nph * p.Qpad * 32, 256);
  p.work_bytes = p.wq_off + (int64_t)p.ncb * p.taps * p.Cop * 32;
  *out = p;
  return true;
}

struct S2PackX {
  int64_t C, H, W, Q, Qpad, rows;   // rows = N 2 Hq: every padded row and, for an odd Hp, one more of zeros
  int pad, Hq, Wq, ncb, nph, nphw, KH;
};

// One workgroup per (padded row hp of an image, channel block): the row belongs to the phases a = hp & 1,
// b = 0 / 1 at phase-grid row i = hp >> 1, and column wp goes to phase b = wp & 1, cell j = wp >> 1.  64
// channels x up to 64 columns at a time are read along W, turned into codes and transposed through LDS as in
// conv_wide_pack_x_k; the threads that store are ordered even columns first, so the stores of one parity are
// one run along j.  The halo columns (the column 2 Wq - 1 of an odd Wp among them), whole halo rows and -- by
// the last ncb nph workgroups -- the planes' tails are zero-filled.  A phase no tap reads (a = 1 when KH = 1,
// b = 1 when KW = 1) is neither stored nor part of the workspace.
__global__ __launch_bounds__(WD_T) void conv_wide_pack_x_s2_k(const float* __restrict__ x, uint8_t* __restrict__ xs,
                                                               S2PackX a) {
  __shared__ uint32_t tile[64 * 17];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (b >= a.rows * a.ncb) {
    uint8_t* dst = xs + ((b - a.rows * a.ncb) * a.Qpad + a.Q) * 32;
    for (int64_t i = tid; i < (a.Qpad - a.Q) * 2; i += WD_T) store_zero16(dst + i * 16);
    return;
  }
  const int cb = (int)(b % a.ncb);
  const int64_t row = b / a.ncb, n = row / (2 * a.Hq);
  const int hp = (int)(row - n * 2 * a.Hq), ih = hp - a.pad;
  if (a.KH == 1 && (hp & 1)) return;
  // phase (hp & 1, 0) at cell (n, hp >> 1, 0); phase (hp & 1, 1) is one plane further
  uint8_t* dst = xs + (((int64_t)cb * a.nph + (hp & 1) * a.nphw) * a.Qpad + (n * a.Hq + (hp >> 1)) * a.Wq) * 32;
  const int64_t pstep = a.Qpad * 32;
  const int odd = a.nphw - 1;   // 1: the odd columns are stored, 0: dropped
  auto at = [&](int wp, int half) { return dst + (wp & 1) * pstep + (wp >> 1) * 32 + half * 16; };
  if (ih < 0 || ih >= a.H) {
    for (int i = tid; i < 4 * a.Wq; i += WD_T)
      if (!((i >> 1) & 1) || odd) store_zero16(at(i >> 1, i & 1));
    return;
  }
  for (int i = tid; i < 2 * (2 * a.Wq - (int)a.W); i += WD_T) {
    const int e = i >> 1, wp = e < a.pad ? e : (int)a.W + e;
    if (!(wp & 1) || odd) store_zero16(at(wp, i & 1));
  }
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
      const int k = tid >> 1, ne = (wc + 1) >> 1;
      const int w = k < ne ? 2 * k : 2 * (k - ne) + 1, wp = a.pad + w0 + w;   // w0 is even: one parity of w is one of wp
      if (!(wp & 1) || odd) {
        const uint32_t* s = tile + w * 17 + (tid & 1) * 8;
        uint4 o;
        o.x = squeeze4(s[0]) | squeeze4(s[1]) << 16;
        o.y = squeeze4(s[2]) | squeeze4(s[3]) << 16;
        o.z = squeeze4(s[4]) | squeeze4(s[5]) << 16;
        o.w = squeeze4(s[6]) | squeeze4(s[7]) << 16;
        *reinterpret_cast<uint4*>(at(wp, tid & 1)) = o;
      }
    }
    __syncthreads();
  }
}

struct S2Gemm {
  const uint8_t* xs;
  const uint8_t* wq;
  const float* bias;
  float* y;
  int64_t Q, Qpad, HqWq, Co, OHW;
  int Wq, OH, OW, Cop, KW, taps, ncb, nct, arows, nph, nphw;
};

// 4 waves as 2 (output channels) x 2 (positions), each 64 x 64 as 2 x 2 MFMA tiles; operands, accumulator
// layout and the NCHW store as in conv_wide_gemm_k.  The stage is nph windows of arows rows, then 128 weight
// rows per tap.
template <int NBUF>
__global__ __launch_bounds__(WD_T) void conv_wide_gemm_s2_k(S2Gemm a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t wide_s2_smem[];
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int ct = (int)(blockIdx.x % a.nct);
  const int64_t q0 = (int64_t)(blockIdx.x / a.nct) * WD_TP;
  const int wrows = a.nph * a.arows;                    // activation rows of a stage
  const int stage = (wrows + a.taps * WD_TC) * 32;
  const int na = a.arows / 32, nx = a.nph * na, np = nx + 4 * a.taps;   // 1-KiB pieces: na per phase, then 4 per tap
  // the global chunk that belongs in LDS chunk `lane` of a piece (pieces start on multiples of 32 rows)
  const int soff = (lane >> 1) * 32 + 16 * ((lane & 1) ^ ((lane >> 4) & 1));

  auto issue = [&](int cb, uint8_t* dst) {
    const uint8_t* xs = a.xs + ((int64_t)cb * a.nph * a.Qpad + q0) * 32 + soff;
    const uint8_t* ws = a.wq + ((int64_t)cb * a.taps * a.Cop + ct * WD_TC) * 32 + soff;
    for (int pc = wave; pc < np; pc += 4) {
      const int f = pc / na, q = pc - nx;
      glds16(pc < nx ? xs + (int64_t)f * a.Qpad * 32 + (pc - f * na) * 1024
                     : ws + ((int64_t)(q >> 2) * a.Cop + (q & 3) * 32) * 32,
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

  const int woff = wrows * 32 + wide_row_off(wm * 64 + r, h);   // + 4096 per tap, + 1024 per tile
  const int arow = wn * 64 + r;
  auto frags = [&](const uint8_t* buf, int tap, int base, v4i (&wf)[2], v4i (&af)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t) wf[t] = *reinterpret_cast<const v4i*>(buf + woff + tap * 4096 + t * 1024);
#pragma unroll
    for (int u = 0; u < 2; ++u) af[u] = *reinterpret_cast<const v4i*>(buf + wide_row_off(arow + base + u * 32, h));
  };
  // the row / column parts of s2_tap_row, stepped: an odd kh or kw is one or nphw windows on, an even one the
  // next cell of the first
  const int kwodd = a.arows, kweven = 1 - a.arows;
  const int khodd = a.nphw * a.arows, kheven = a.Wq - khodd;
  auto compute = [&](const uint8_t* buf) {
    v4i wf[2], af[2], wnx[2], anx[2];
    frags(buf, 0, 0, wf, af);
    int kh = 0, kw = 0, rb = 0, cbase = 0;
    for (int tap = 0; tap < a.taps; ++tap) {
      const bool more = tap + 1 < a.taps;
      if (more) {   // the next tap's fragments are read under this tap's MFMAs
        ++kw;
        cbase += (kw & 1) ? kwodd : kweven;
        if (kw == a.KW) {
          kw = 0, cbase = 0, ++kh;
          rb += (kh & 1) ? khodd : kheven;
        }
        frags(buf, tap + 1, rb + cbase, wnx, anx);
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
    issue(0, wide_s2_smem);
    for (int cb = 0; cb < a.ncb; ++cb) {
      wide_wait_dma();
      wide_barrier();   // block cb is in LDS; every wave has left block cb-1, whose buffer is refilled next
      if (cb + 1 < a.ncb) issue(cb + 1, wide_s2_smem + ((cb + 1) & 1) * stage);
      compute(wide_s2_smem + (cb & 1) * stage);
    }
  } else {
    for (int cb = 0; cb < a.ncb; ++cb) {
      if (cb > 0) wide_barrier();
      issue(cb, wide_s2_smem);
      wide_wait_dma();
      wide_barrier();
      compute(wide_s2_smem);
    }
  }

  // cells of the phase grid past the output map (i >= OH or j >= OW) and beyond Q are computed and not stored
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int64_t q = q0 + wn * 64 + u * 32 + r;
    const int64_t n = q / a.HqWq;
    const int rem = (int)(q - n * a.HqWq), i = rem / a.Wq, j = rem - i * a.Wq;
    if (q >= a.Q || i >= a.OH || j >= a.OW) continue;
    float* yp = a.y + n * a.Co * a.OHW + i * a.OW + j;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int co = ct * WD_TC + wm * 64 + t * 32 + (k & 3) + 8 * (k >> 2) + 4 * h;
        if (co < a.Co) yp[co * a.OHW] = a.bias != nullptr ? acc[t][u][k] + a.bias[co] : acc[t][u][k];
      }
  }
}

int g_s2_stages = 7;   // bnn_conv2d_fwd_wide_s2_set_stages

template <int NBUF>
void s2_gemm_launch(const S2Plan& p, const S2Gemm& a, hipStream_t st) {
  if (p.lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wide_gemm_s2_k<NBUF>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
  hipLaunchKernelGGL((conv_wide_gemm_s2_k<NBUF>), dim3((unsigned)(p.ntile * p.nct)), dim3(WD_T), (size_t)p.lds, st, a);
}

}  // namespace
}  // namespace bnn

using namespace bnn;

BNN_API int bnn_conv2d_fwd_wide_s2_ok(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW,
                                      int32_t stride, int32_t pad, int32_t dil, int32_t groups) {
  S2Plan p;
  return wide_s2_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p) ? 1 : 0;
}

BNN_API int64_t bnn_conv2d_fwd_wide_s2_workspace(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH,
                                                 int64_t KW, int32_t pad) {
  S2Plan p;
  return wide_s2_plan(N, C, H, W, Co, KH, KW, 2, pad, 1, 1, &p) ? p.work_bytes : 0;
}

BNN_API const char* bnn_conv2d_fwd_wide_s2_kernel(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH,
                                                  int64_t KW, int32_t stride, int32_t pad, int32_t dil,
                                                  int32_t groups) {
  static thread_local char buf[96];
  S2Plan p;
  if (!wide_s2_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p)) return "";
  snprintf(buf, sizeof(buf), "conv_wide_gemm_s2_k<%d> lds=%lld b128=%d nph=%d", p.nbuf, (long long)p.lds, p.cycles,
           p.nph);
  return buf;
}

BNN_API int bnn_conv2d_fwd_wide_s2_set_stages(int32_t mask) {
  if (mask >= 0) g_s2_stages = mask & 7;
  return g_s2_stages;
}

BNN_API int bnn_conv2d_fwd_wide_s2(const float* x, const float* w_latent, const float* bias, float* y, int64_t N,
                                   int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW,
                                   int32_t stride, int32_t pad, int32_t dil, int32_t groups, void* work,
                                   int64_t work_bytes, void* stream) {
  S2Plan p;
  if (!wide_s2_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p)) {
    set_error("bnn_conv2d_fwd_wide_s2: shape not taken (stride 2, dilation 1, one group, pad <= K - 1, C %% 64 == 0, "
              "C > 64 or Co > 64, C KH KW < 2^24, one channel block's phase windows and taps within the LDS)");
    return kErrInval;
  }
  if (!x || !w_latent || !y || !work || !aligned16(work) || work_bytes < p.work_bytes) {
    set_error("bnn_conv2d_fwd_wide_s2: null pointer, or a workspace not 16-B aligned or below "
              "bnn_conv2d_fwd_wide_s2_workspace = %lld bytes", (long long)p.work_bytes);
    return kErrInval;
  }
  if (N == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint8_t* xs = static_cast<uint8_t*>(work);
  uint8_t* wq = xs + p.wq_off;
  const S2PackX px{C, H, W, p.Q, p.Qpad, N * 2 * p.Hq, p.pad, p.Hq, p.Wq, p.ncb, p.nph, p.nphw, p.KH};
  if (g_s2_stages & 1)
    hipLaunchKernelGGL(conv_wide_pack_x_s2_k, dim3((unsigned)((px.rows + p.nph) * p.ncb)), dim3(WD_T), 0, st, x, xs,
                       px);
  if (g_s2_stages & 2) {
    const int rc = bnn_conv2d_wide_pack_w(w_latent, wq, C, Co, KH, KW, stream);
    if (rc != 0) return rc;
  }
  const S2Gemm g{xs, wq, bias, y, p.Q, p.Qpad, (int64_t)p.Hq * p.Wq, Co, (int64_t)p.OH * p.OW,
                 p.Wq, p.OH, p.OW, p.Cop, p.KW, p.taps, p.ncb, p.nct, p.arows, p.nph, p.nphw};
  if (!(g_s2_stages & 4)) return check_launch("bnn_conv2d_fwd_wide_s2");
  if (p.nbuf == 2) s2_gemm_launch<2>(p, g, st);
  else s2_gemm_launch<1>(p, g, st);
  return check_launch("bnn_conv2d_fwd_wide_s2");
}
