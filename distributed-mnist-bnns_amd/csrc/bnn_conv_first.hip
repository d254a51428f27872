// First-layer (real-input) binary conv2d: forward and filter / bias gradient for few input channels and wide
// output (1 <= C <= 4, C KH KW <= 80, Co > 64, stride 1) -- the RGB layer of the BinaryNet /
// VGG-style CIFAR stacks, whose input is never binarised:
//   y[n,co,oh,ow]   = fl( sum_{c,kh,kw} x[n,c,oh+kh-pad,ow+kw-pad] * tsign(w[co,c,kh,kw]) + bias[co] )
//   dw[co,c,kh,kw]  = sum_{n,oh,ow} dy[n,co,oh,ow] * x[n,c,oh+kh-pad,ow+kw-pad]         db[co] = sum dy[n,co,oh,ow]
//
// Forward, conv_first_fwd_k<KS>: one launch, no workspace.  A workgroup owns 128 consecutive output positions
// q = oh OW + ow of one image and loops over Co in tiles of 128.  The halo window C x (rows + KH-1) x Wp of
// the tile is read from NCHW, zero-filled outside the image, split into its exact three bf16 planes
// (bf16x3_split) and stored to LDS once; the ternary weights of a channel tile are built from the latent weight
// in the kernel as bf16 [co][Kp], Kp = round_up(Kt, 16), double-buffered.  The GEMM runs on
// v_mfma_f32_32x32x16_bf16 with the weights as first operand: a register of the accumulator is an output
// channel and the lanes run along positions, so a store is a 128-B run along ow.  A wave owns 32 positions and
// all four 32-channel blocks of the tile: it gathers its 3 KS position fragments once (a lane reads its eight
// k-values of a k-step at the taps' offsets from its own position) and keeps them in registers over the Co
// loop -- each input element is staged, split and gathered once per position tile.  Every product is exact; the
// roundings are the fp32 accumulation and the bias add.
//
// Filter and bias gradient: two launches.
//  1. conv_first_bwd_filter_k<NB, VEC>  a GEMM on v_mfma_f32_32x32x2_f32 whose contraction runs over positions,
//     both operands straight from their fp32 form.  M = 128 output channels per workgroup (four waves x 32), N =
//     the taps padded to Kp = round_up(Kt + 1, 32) columns: column Kt reads a plane of 1.0, so db falls out of
//     the same accumulators.  The N OH output rows are cut into slices of whole rows; a workgroup walks its
//     slice in chunks of at most 64 positions (whole rows of one image, or a 64-column piece of a long row),
//     staging the chunk's dy for its 128 channels and the input window those positions reach in LDS.  fp32
//     partials -> part [slices][ceil(Co/128) 128][Kp], every element written by every call.
//  2. conv_first_bwd_filter_reduce_k    the slices summed in double in a fixed order, one rounding.
// No atomics: deterministic.
#include "bnn_conv_first.h"

#include <cstdio>

#include "bnn.h"

namespace bnn {
namespace {

constexpr int kFirstRounds = 2;    // the K split aims at this many rounds of workgroups on kFirstCUs CUs
constexpr int kFirstCUs = 256;
constexpr int FG_POS = 64;         // positions of a filter-gradient chunk at most
constexpr int FR_EL = 16, FR_ST = 16;   // the reduce: elements x strands of a workgroup

struct FirstPlan {
  int64_t N, C, H, W, Co;
  int KH, KW, pad, OH, OW, Wp, Kt, ctiles;
  // forward
  int ks, kp;          // k-steps of 16 and Kp = 16 ks
  int wp;              // bf16 per weight row in LDS: Kp + 8 j, the j of the fewest modelled cycles
  int rmax, rw;        // output rows a position tile can touch, window rows rmax + KH - 1
  int plane;           // bf16 per plane of the window: C rw Wp + the zero slot, rounded up to 8
  int cycles;          // modelled LDS cycles of the weight fragment ds_read_b128 (4 = conflict-free)
  int64_t ptiles, fwd_lds;
  // filter gradient
  int kpf, nb;         // Kp = round_up(Kt + 1, 32) columns, 32-column blocks
  int cr, cw, cwe;     // rows and columns of a chunk, columns rounded up to 2
  int dp;              // floats per channel of the dy stage (odd: the lanes of a read run down the channels)
  int xp, xpl;         // floats per row and per plane of the input window: cw + KW, (cr + KH - 1) xp
  int vec;             // dy is staged with 16-B loads (OW % 4 == 0)
  int64_t rows, rps, splits, cop, flt_lds, work_bytes;
};

bool first_plan_make(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride,
                     int32_t pad, int32_t dil, int32_t groups, FirstPlan* out) {
  const int64_t lim = 1ll << 31;
  if (groups != 1 || stride != 1 || dil != 1 || N < 0 || C < 1 || C > kFirstMaxC || Co <= 64 || Co >= lim) return false;
  if (KH < 1 || KW < 1 || KH > kFirstMaxKt || KW > kFirstMaxKt || C * KH * KW > kFirstMaxKt) return false;
  if (pad < 0 || pad > std::min(KH, KW) - 1 || H < 1 || W < 1 || H >= lim || W >= lim) return false;
  FirstPlan p{};
  p.N = N, p.C = C, p.H = H, p.W = W, p.Co = Co;
  p.KH = (int)KH, p.KW = (int)KW, p.pad = pad, p.Kt = (int)(C * KH * KW);
  const int64_t OH = H + 2 * pad - KH + 1, OW = W + 2 * pad - KW + 1;
  if (OH < 1 || OW < 1 || C * H * W >= lim || OH * OW >= lim - 128) return false;   // per-image offsets are ints
  p.OH = (int)OH, p.OW = (int)OW, p.Wp = (int)W + 2 * pad;
  p.ctiles = (int)((Co + 127) / 128);
  // forward: the window, the tap table, two weight tiles with their bias
  p.kp = (p.Kt + 15) / 16 * 16, p.ks = p.kp / 16;
  p.rmax = (int)std::min<int64_t>(OH, 126 / OW + 2);
  p.rw = p.rmax + p.KH - 1;
  const int64_t win = C * p.rw * p.Wp;
  if (win >= (1 << 20)) return false;
  p.plane = (int)round_up(win + 1, 8);
  first_weight_pitch(p.kp, &p.wp, &p.cycles);
  p.fwd_lds = 2ll * 128 * p.wp * 2 + 2 * 128 * 4 + p.kp * 4 + 3ll * p.plane * 2;
  p.ptiles = (OH * OW + 127) / 128;
  if (p.fwd_lds > kWideMaxLds || N * p.ptiles >= lim) return false;
  // filter gradient: the chunk, its stage, the K split over rows
  p.kpf = (p.Kt + 1 + 31) / 32 * 32, p.nb = p.kpf / 32;
  const int owe = (p.OW + 1) & ~1;
  if (owe <= FG_POS) p.cw = p.OW, p.cwe = owe, p.cr = std::max(1, std::min(p.OH, FG_POS / owe));
  else p.cw = FG_POS, p.cwe = FG_POS, p.cr = 1;
  p.dp = (p.cr * p.cwe) | 1;
  p.xp = p.cw + p.KW, p.xpl = (p.cr + p.KH - 1) * p.xp;
  p.vec = p.OW % 4 == 0;
  p.flt_lds = (128ll * p.dp + (C + 1) * p.xpl) * 4;
  if (p.flt_lds > kWideMaxLds) return false;
  p.rows = N * OH;
  // the K split: channel tiles x slices is about kFirstRounds rounds of one workgroup per CU
  const int64_t want = std::min(p.rows, std::max<int64_t>(1, (kFirstRounds * kFirstCUs + p.ctiles - 1) / p.ctiles));
  p.rps = p.rows ? (p.rows + want - 1) / want : 0;
  p.splits = p.rows ? (p.rows + p.rps - 1) / p.rps : 0;
  p.cop = (int64_t)p.ctiles * 128;
  if (p.ctiles * p.splits >= lim || Co * (p.Kt + 1) / FR_EL + 1 >= lim) return false;
  p.work_bytes = round_up(p.splits * p.cop * p.kpf * 4, 256);
  *out = p;
  return true;
}

// The one decision function: the _ok, workspace and kernel queries and both launches.  The last answer is
// kept per thread: a training step asks several times for one shape.
bool first_plan(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride,
                int32_t pad, int32_t dil, int32_t groups, FirstPlan* out) {
  static thread_local struct {
    int64_t key[11];
    bool valid, ok;
    FirstPlan plan;
  } memo{};
  const int64_t key[11] = {N, C, H, W, Co, KH, KW, stride, pad, dil, groups};
  if (!memo.valid || !std::equal(key, key + 11, memo.key)) {
    memo.ok = first_plan_make(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &memo.plan);
    std::copy(key, key + 11, memo.key);
    memo.valid = true;
  }
  if (memo.ok) *out = memo.plan;
  return memo.ok;
}

struct FirstFwd {
  const float* x;
  const float* w;
  const float* bias;   // nullable
  float* y;
  int64_t Co;
  int C, H, W, KH, KW, pad, OH, OW, Wp, Kt, wp, rw, plane, ptiles, ctiles;
};

// LDS: ws [2][128][wp] bf16 weight tiles, bs [2][128] fp32 bias, taps [Kp] window offsets (-1 beyond Kt),
// xs [3][plane] bf16 window planes -- element `win` of each plane is the zero every k >= Kt reads.
template <int KS>
__global__ __launch_bounds__(WD_T) void conv_first_fwd_k(FirstFwd a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t first_smem[];
  constexpr int KP = 16 * KS;
  unsigned short* const ws = reinterpret_cast<unsigned short*>(first_smem);
  float* const bs = reinterpret_cast<float*>(first_smem + 2 * 128 * a.wp * 2);
  int* const taps = reinterpret_cast<int*>(bs + 2 * 128);
  unsigned short* const xs = reinterpret_cast<unsigned short*>(taps + KP);
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(), r = lane & 31, h = lane >> 5;
  const int64_t n = blockIdx.x / a.ptiles;
  const int q0 = (int)(blockIdx.x - n * a.ptiles) * 128, OHW = a.OH * a.OW, oh0 = q0 / a.OW;
  const int win = a.C * a.rw * a.Wp, taps_hw = a.KH * a.KW;

  auto stage_w = [&](int ct, int buf) {
    for (int e = tid; e < 128 * KP; e += WD_T) {
      const int cl = e / KP, k = e - cl * KP;
      const int64_t co = (int64_t)ct * 128 + cl;
      ws[(buf * 128 + cl) * a.wp + k] = co < a.Co && k < a.Kt ? tsign_bf16(a.w[co * a.Kt + k]) : (unsigned short)0;
    }
    if (tid < 128) {
      const int64_t co = (int64_t)ct * 128 + tid;
      bs[buf * 128 + tid] = a.bias != nullptr && co < a.Co ? a.bias[co] : 0.f;
    }
  };

  for (int k = tid; k < KP; k += WD_T) {
    const int c = k / taps_hw, t = k - c * taps_hw, kh = t / a.KW;
    taps[k] = k < a.Kt ? (c * a.rw + kh) * a.Wp + (t - kh * a.KW) : -1;
  }
  const float* xn = a.x + n * a.C * a.H * a.W;
  for (int i = tid; i < win; i += WD_T) {
    const int c = i / (a.rw * a.Wp), rem = i - c * a.rw * a.Wp, lr = rem / a.Wp;
    const int ih = oh0 - a.pad + lr, iw = rem - lr * a.Wp - a.pad;
    const float v = ih >= 0 && ih < a.H && iw >= 0 && iw < a.W ? xn[(c * a.H + ih) * a.W + iw] : 0.f;
    bf16x3_split(v, xs[i], xs[a.plane + i], xs[2 * a.plane + i]);
  }
  if (tid < 3) xs[tid * a.plane + win] = 0;
  stage_w(0, 0);
  wide_barrier();

  // this lane's position (clamped past the image's last: gathered, never stored) and its 3 KS fragments
  const int q = q0 + 32 * wave + r, qc = min(q, OHW - 1), oh = qc / a.OW;
  const int base = (oh - oh0) * a.Wp + (qc - oh * a.OW);
  const bool live = q < OHW;
  v4i xf[3][KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    uint32_t e[3][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int off = taps[16 * ks + 8 * h + j], ad = off < 0 ? win : base + off;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) e[pl][j] = xs[pl * a.plane + ad];
    }
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
      xf[pl][ks] = v4i{(int)(e[pl][0] | e[pl][1] << 16), (int)(e[pl][2] | e[pl][3] << 16),
                       (int)(e[pl][4] | e[pl][5] << 16), (int)(e[pl][6] | e[pl][7] << 16)};
  }

  float* const yq = a.y + n * a.Co * OHW + q;
  for (int ct = 0; ct < a.ctiles; ++ct) {
    const int buf = ct & 1;
    if (ct + 1 < a.ctiles) stage_w(ct + 1, buf ^ 1);   // the next tile's weights under this tile's MFMAs
    v16f acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[m][i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const v8bf wf = __builtin_bit_cast(
            v8bf, *reinterpret_cast<const v4i*>(ws + (buf * 128 + 32 * m + r) * a.wp + 16 * ks + 8 * h));
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)   // fixed plane order: d1, d2, d3
          acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, __builtin_bit_cast(v8bf, xf[pl][ks]), acc[m], 0, 0, 0);
      }
    // register i of block m is channel 32 m + (i & 3) + 8 (i >> 2) + 4 h; the lanes of a half wave are 32
    // consecutive positions: non-temporal 128-B runs, left in flight under the next tile's MFMAs
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cl = 32 * m + 8 * g + 4 * h;
        const float4 b4 = *reinterpret_cast<const float4*>(bs + buf * 128 + cl);
        const float bj[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t co = (int64_t)ct * 128 + cl + j;
          if (live && co < a.Co) __builtin_nontemporal_store(acc[m][4 * g + j] + bj[j], yq + co * OHW);
        }
      }
    if (ct + 1 < a.ctiles) wide_barrier();   // tile ct+1 is staged; every wave has left buffer `buf`
  }
}

struct FirstFilt {
  const float* dy;
  const float* x;
  float* part;
  int64_t rows, rps, Co, cop;
  int C, H, W, KH, KW, pad, OH, OW, Kt, kpf, ctiles, cr, cw, cwe, dp, xp, xpl;
};

// LDS: ds [128][dp] the chunk's dy, channel-major, row lr of the chunk at lr cwe; xs [C + 1][xpl] the input
// window of the chunk, row pitch xp = cw + KW (the columns past cw + KW - 1 are zero: an odd chunk width's
// spare position reads them), plane C all 1.0.  Lane (r, h) of MFMA step s holds position 2 s + h of a chunk
// row: dy of channel 32 wave + r as first operand, the input at tap 32 nb + r's offset as second.
template <int NB, bool VEC>
__global__ __launch_bounds__(WD_T) void conv_first_bwd_filter_k(FirstFilt a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t first_smem[];
  float* const ds = reinterpret_cast<float*>(first_smem);
  float* const xs = ds + 128 * a.dp;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(), r = lane & 31, h = lane >> 5;
  const int cot = (int)(blockIdx.x % a.ctiles);
  const int64_t slice = blockIdx.x / a.ctiles;
  const int64_t g0 = slice * a.rps, g1 = min(a.rows, g0 + a.rps);
  const int64_t OHW = (int64_t)a.OH * a.OW;

  for (int i = tid; i < a.xpl; i += WD_T) xs[a.C * a.xpl + i] = 1.f;
  int bb[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int k = 32 * nb + r, thw = a.KH * a.KW, c = k / thw, t = k - c * thw, kh = t / a.KW;
    bb[nb] = (k < a.Kt ? c * a.xpl + kh * a.xp + (t - kh * a.KW) : a.C * a.xpl) + h;   // k >= Kt: the ones
  }
  const int ab = (32 * wave + r) * a.dp + h;
  v16f acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;

  for (int64_t g = g0; g < g1;) {
    const int64_t n = g / a.OH;
    const int oh = (int)(g - n * a.OH);
    const int cr = (int)min((int64_t)min(a.cr, a.OH - oh), g1 - g);
    const float* const dyn = a.dy + (n * a.Co + (int64_t)cot * 128) * OHW + (int64_t)oh * a.OW;
    const float* const xn = a.x + n * a.C * a.H * a.W;
    const int cn = (int)min((int64_t)128, a.Co - (int64_t)cot * 128);   // live channels of this tile
    for (int ow0 = 0; ow0 < a.OW; ow0 += a.cw) {
      const int cw = min(a.cw, a.OW - ow0), cwe = (cw + 1) & ~1;
      wide_barrier();   // every wave has left the previous chunk
      if constexpr (VEC) {
        const int c4 = cw >> 2, per = cr * c4;
        for (int i = tid; i < 128 * per; i += WD_T) {
          const int cl = i / per, rem = i - cl * per, lr = rem / c4, j = (rem - lr * c4) * 4;
          const float4 v = cl < cn ? *reinterpret_cast<const float4*>(dyn + cl * OHW + lr * a.OW + ow0 + j)
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
          float* d = ds + cl * a.dp + lr * a.cwe + j;
          d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        }
      } else {
        const int per = cr * cwe;
        for (int i = tid; i < 128 * per; i += WD_T) {
          const int cl = i / per, rem = i - cl * per, lr = rem / cwe, j = rem - lr * cwe;
          ds[cl * a.dp + lr * a.cwe + j] = cl < cn && j < cw ? dyn[cl * OHW + lr * a.OW + ow0 + j] : 0.f;
        }
      }
      const int wrows = cr + a.KH - 1, per = wrows * a.xp;
      for (int i = tid; i < a.C * per; i += WD_T) {
        const int c = i / per, rem = i - c * per, lr = rem / a.xp, col = rem - lr * a.xp;
        const int ih = oh + lr - a.pad, iw = ow0 + col - a.pad;
        xs[c * a.xpl + rem] = col < cw + a.KW - 1 && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W
                                  ? xn[(c * a.H + ih) * a.W + iw] : 0.f;
      }
      wide_barrier();
      for (int lr = 0; lr < cr; ++lr) {
        const float* const dl = ds + ab + lr * a.cwe;
        const int xo = lr * a.xp;
        float dv = dl[0], xv[NB], dn, xn2[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) xv[nb] = xs[bb[nb] + xo];
        for (int s = 0; s < cwe; s += 2) {
          const int s2 = s + 2 < cwe ? s + 2 : s;   // the next step's reads under this one's MFMAs
          dn = dl[s2];
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) xn2[nb] = xs[bb[nb] + xo + s2];
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv, xv[nb], acc[nb], 0, 0, 0);
          dv = dn;
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) xv[nb] = xn2[nb];
        }
      }
    }
    g += cr;
  }

  // fp32 partials, the rows of the Co tail and every padding column included: a register is a 128-B run
  float* const pp = a.part + ((slice * a.cop + (int64_t)cot * 128 + 32 * wave + 4 * h) * a.kpf + r);
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) pp[(int64_t)((i & 3) + 8 * (i >> 2)) * a.kpf + 32 * nb] = acc[nb][i];
}

struct FirstReduce {
  const float* part;
  float* dw;
  float* db;   // nullable
  int64_t Co, cop, splits;
  int Kt, kpf;
};

// A workgroup sums FR_EL elements (co, k <= Kt) over FR_ST strands of slices: strand j adds slices j, j +
// FR_ST, ... in index order in double, then the strands are added in index order and the sum is rounded
// once.  Column Kt is db.  splits = 0 zero-fills (the empty batch).
__global__ __launch_bounds__(WD_T) void conv_first_bwd_filter_reduce_k(FirstReduce a) {
  __shared__ double red[FR_ST][FR_EL];
  const int tid = threadIdx.x, e = tid % FR_EL, st = tid / FR_EL;
  const int64_t el = (int64_t)blockIdx.x * FR_EL + e, co = el / (a.Kt + 1);
  const int k = (int)(el - co * (a.Kt + 1));
  double s = 0.0;
  if (co < a.Co) {
    const float* p = a.part + co * a.kpf + k;
#pragma unroll 4
    for (int64_t sp = st; sp < a.splits; sp += FR_ST) s += (double)p[sp * a.cop * a.kpf];
  }
  red[st][e] = s;
  __syncthreads();
  if (st == 0 && co < a.Co) {
    double t = 0.0;
    for (int j = 0; j < FR_ST; ++j) t += red[j][e];
    if (k < a.Kt) a.dw[co * a.Kt + k] = (float)t;
    else if (a.db != nullptr) a.db[co] = (float)t;
  }
}

template <typename K>
void first_lds_attr(K kernel, int64_t lds) {
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

template <int KS>
void first_fwd_launch(const FirstPlan& p, const FirstFwd& a, hipStream_t st) {
  first_lds_attr(conv_first_fwd_k<KS>, p.fwd_lds);
  hipLaunchKernelGGL(conv_first_fwd_k<KS>, dim3((unsigned)(p.N * p.ptiles)), dim3(WD_T), (size_t)p.fwd_lds, st, a);
}

template <int NB, bool VEC>
void first_filt_launch(const FirstPlan& p, const FirstFilt& a, hipStream_t st) {
  first_lds_attr(conv_first_bwd_filter_k<NB, VEC>, p.flt_lds);
  hipLaunchKernelGGL((conv_first_bwd_filter_k<NB, VEC>), dim3((unsigned)(p.ctiles * p.splits)), dim3(WD_T),
                     (size_t)p.flt_lds, st, a);
}

template <int NB>
void first_filt_launch_nb(const FirstPlan& p, const FirstFilt& a, hipStream_t st) {
  if (p.vec && aligned16(a.dy)) first_filt_launch<NB, true>(p, a, st);   // OW % 4 == 0: every run starts 16-B aligned
  else first_filt_launch<NB, false>(p, a, st);
}

const char* const kFirstShapes =
    "shape not taken (one group, stride 1, dilation 1, pad <= min(KH, KW) - 1, 1 <= C <= 4, C KH KW <= 80, Co > 64, "
    "the forward's window stage within 160 KiB of LDS, grids and per-image sizes below 2^31)";

}  // namespace
}  // namespace bnn

using namespace bnn;

BNN_API int bnn_conv2d_fwd_first_ok(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW,
                                    int32_t stride, int32_t pad, int32_t dil, int32_t groups) {
  FirstPlan p;
  return first_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p) ? 1 : 0;
}

BNN_API const char* bnn_conv2d_fwd_first_kernel(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH,
                                                int64_t KW, int32_t stride, int32_t pad, int32_t dil,
                                                int32_t groups) {
  static thread_local char buf[160];
  FirstPlan p;
  if (!first_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p)) return "";
  snprintf(buf, sizeof(buf), "conv_first_fwd_k<%d> lds=%lld rows=%d Kp=%d pitch=%d b128=%d", p.ks, (long long)p.fwd_lds,
           p.rw, p.kp, p.wp, p.cycles);
  return buf;
}

BNN_API int bnn_conv2d_fwd_first(const float* x, const float* w_latent, const float* bias, float* y, int64_t N,
                                 int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride,
                                 int32_t pad, int32_t dil, int32_t groups, void* stream) {
  FirstPlan p;
  if (!first_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p)) {
    set_error("bnn_conv2d_fwd_first: %s", kFirstShapes);
    return kErrInval;
  }
  if (N == 0) return 0;   // the empty batch: nothing to write
  if (!x || !w_latent || !y) {
    set_error("bnn_conv2d_fwd_first: null pointer");
    return kErrInval;
  }
  const FirstFwd a{x, w_latent, bias, y, Co, (int)C, (int)H, (int)W, p.KH, p.KW, p.pad, p.OH, p.OW, p.Wp, p.Kt,
                   p.wp, p.rw, p.plane, (int)p.ptiles, p.ctiles};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (p.ks) {
    case 1: first_fwd_launch<1>(p, a, st); break;
    case 2: first_fwd_launch<2>(p, a, st); break;
    case 3: first_fwd_launch<3>(p, a, st); break;
    case 4: first_fwd_launch<4>(p, a, st); break;
    default: first_fwd_launch<5>(p, a, st); break;
  }
  return check_launch("bnn_conv2d_fwd_first");
}

BNN_API int bnn_conv2d_bwd_filter_first_ok(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH,
                                           int64_t KW, int32_t stride, int32_t pad, int32_t dil, int32_t groups) {
  return bnn_conv2d_fwd_first_ok(N, C, H, W, Co, KH, KW, stride, pad, dil, groups);
}

BNN_API int64_t bnn_conv2d_bwd_filter_first_workspace(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co,
                                                      int64_t KH, int64_t KW, int32_t pad) {
  FirstPlan p;
  return first_plan(N, C, H, W, Co, KH, KW, 1, pad, 1, 1, &p) ? p.work_bytes : 0;
}

BNN_API const char* bnn_conv2d_bwd_filter_first_kernel(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co,
                                                       int64_t KH, int64_t KW, int32_t stride, int32_t pad,
                                                       int32_t dil, int32_t groups) {
  static thread_local char buf[160];
  FirstPlan p;
  if (!first_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p)) return "";
  snprintf(buf, sizeof(buf), "conv_first_bwd_filter_k<%d, %d> lds=%lld chunk=%dx%d rows=%lld slice=%lld splits=%lld Kp=%d",
           p.nb, p.vec, (long long)p.flt_lds, p.cr, p.cw, (long long)p.rows, (long long)p.rps, (long long)p.splits,
           p.kpf);
  return buf;
}

BNN_API int bnn_conv2d_bwd_filter_first(const float* dy, const float* x, float* dw, float* db, int64_t N, int64_t C,
                                        int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride,
                                        int32_t pad, int32_t dil, int32_t groups, void* work, int64_t work_bytes,
                                        void* stream) {
  FirstPlan p;
  if (!first_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p)) {
    set_error("bnn_conv2d_bwd_filter_first: %s", kFirstShapes);
    return kErrInval;
  }
  if (!dy || !x || !dw || (p.work_bytes > 0 && (!work || !aligned16(work))) || work_bytes < p.work_bytes) {
    set_error("bnn_conv2d_bwd_filter_first: null pointer, or a workspace not 16-B aligned or below "
              "bnn_conv2d_bwd_filter_first_workspace = %lld bytes", (long long)p.work_bytes);
    return kErrInval;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(work);
  if (p.splits > 0) {
    const FirstFilt g{dy, x, part, p.rows, p.rps, Co, p.cop, (int)C, (int)H, (int)W, p.KH, p.KW, p.pad, p.OH, p.OW,
                      p.Kt, p.kpf, p.ctiles, p.cr, p.cw, p.cwe, p.dp, p.xp, p.xpl};
    switch (p.nb) {
      case 1: first_filt_launch_nb<1>(p, g, st); break;
      case 2: first_filt_launch_nb<2>(p, g, st); break;
      default: first_filt_launch_nb<3>(p, g, st); break;
    }
  }
  // the empty batch: zeros, by the reduce over no slices
  const FirstReduce rd{part, dw, db, Co, p.cop, p.splits, p.Kt, p.kpf};
  hipLaunchKernelGGL(conv_first_bwd_filter_reduce_k, dim3((unsigned)((Co * (p.Kt + 1) + FR_EL - 1) / FR_EL)),
                     dim3(WD_T), 0, st, rd);
  return check_launch("bnn_conv2d_bwd_filter_first");
}
