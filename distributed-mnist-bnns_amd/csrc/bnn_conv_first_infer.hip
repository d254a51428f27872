// Frozen first-layer (real-input) binary conv2d: the bf16-MFMA implicit GEMM of
// bnn_conv_first.hip's forward with eval-mode BatchNorm2d -> Hardtanh -> (MaxPool2d(2, 2)) -> sign in its
// epilogue.  The input is fp32 NCHW (1 <= C <= 4, never binarised) and the weight the latent fp32 weight; the
// output is either the next wide layer's FP4 planes on that layer's zero-padded grid (out_form 0: half a byte
// per element, halo and tail zero-filled by this kernel) or int8 signs NCHW (out_form 1).  One launch: no
// fp32 map, no BatchNorm pass, no pack, no workspace.
//
// conv_first_bnsign_k<KS, POOL>: the staging, the weight build and the k-loop are conv_first_fwd_k<KS>'s -- the
// halo window of a position tile as its exact three bf16 planes in LDS, ternary bf16 weights built per
// 128-channel tile (double-buffered, here with the tile's bias / mean / invstd / gamma / beta beside them), a
// wave's 32 positions' fragments gathered once and kept in registers over the Co loop, four 32 x 32
// accumulators per wave.  What differs is which position a lane holds and what leaves the accumulators:
//
//   pool 0   128 consecutive output positions q = oh OW + ow of one image per workgroup; lane r of wave w is
//            q0 + 32 w + r.
//   pool 2   32 consecutive pooling windows v = ph PW + pw of one image per workgroup; lane r of wave w is
//            element (r >> 1 & 1, r & 1) of window v0 + 8 w + (r >> 2).  A window is one lane quad: the OR
//            over it is two DPP quad_perm steps, no LDS.  The staged window has 2 (30 / PW + 2) + KH - 1 rows.
//
// Epilogue, per channel tile: register 4 g + j of accumulator m is channel 32 m + 8 g + 4 h + j, so accumulators
// 2 b and 2 b + 1 are the 64-channel block b of the tile in exactly the map bnn_conv_wide_infer.hip's epilogue
// consumes.  x = fl(I + bias[co]), y = bn_y1(x, mean, 0, invstd, gamma, beta), folded into three bit masks per
// lane and block (y > 0, y == 0, NaN); pooling ORs masks, never values: +1 if some y > 0, else 0 if some
// y == 0, else -1, and 0 if the window holds a NaN.  out_form 0 builds the lane's nibbles in place, one
// v_permlane32_swap per dword hands lane half h the whole of 16-B half h of the position's 32-B plane row, and
// the row goes out with one 16-B store per lane: a wave's four accumulators are two plane rows per position.
#include "bnn_conv_first.h"

#include <cstdio>

#include "bnn.h"

namespace bnn {
namespace {

constexpr int FI_TW = 32;   // pooling windows of a pooled workgroup

struct FirstInferPlan {
  int64_t N, C, H, W, Co;
  int KH, KW, pad, OH, OW, PH, PW, Wp, Kt, ctiles, pool, form;
  int ks, kp, wp, cycles;   // k-steps of 16, Kp = 16 ks, the weight rows' pitch and its modelled read cycles
  int rmax, rw, plane;      // output rows a tile can touch, window rows rmax + KH - 1, bf16 per window plane
  int64_t tiles, lds;       // position tiles per image
  int Hp2, Wp2, pad2, ncb2;   // out_form 0: the consumer's padded grid
  int64_t P2, Ppad2;
};

// The one decision function of the entry and its two queries.  It starts from the training forward's: a
// geometry bnn_conv2d_fwd_first_ok refuses is refused here.
bool first_infer_plan(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride,
                      int32_t pad, int32_t dil, int32_t groups, int32_t pool, int32_t form, int64_t KH2, int64_t KW2,
                      int32_t pad2, FirstInferPlan* out) {
  if (!bnn_conv2d_fwd_first_ok(N, C, H, W, Co, KH, KW, stride, pad, dil, groups)) return false;
  if ((pool != 0 && pool != 2) || (form != 0 && form != 1)) return false;
  FirstInferPlan p{};
  p.N = N, p.C = C, p.H = H, p.W = W, p.Co = Co;
  p.KH = (int)KH, p.KW = (int)KW, p.pad = pad, p.pool = pool, p.form = form, p.Kt = (int)(C * KH * KW);
  p.Wp = (int)W + 2 * pad;
  p.OH = (int)H + 2 * pad - p.KH + 1, p.OW = p.Wp - p.KW + 1;
  if (pool == 2 && ((p.OH | p.OW) & 1)) return false;
  p.PH = pool ? p.OH / 2 : p.OH, p.PW = pool ? p.OW / 2 : p.OW;
  p.ctiles = (int)((Co + 127) / 128);
  p.kp = (p.Kt + 15) / 16 * 16, p.ks = p.kp / 16;
  first_weight_pitch(p.kp, &p.wp, &p.cycles);
  if (pool) {
    // 32 consecutive windows cross at most 30 / PW + 2 window rows, two output rows each
    p.rmax = 2 * std::min(p.PH, (FI_TW - 2) / p.PW + 2);
    p.tiles = ((int64_t)p.PH * p.PW + FI_TW - 1) / FI_TW;
  } else {
    p.rmax = std::min(p.OH, (WD_TP - 2) / p.OW + 2);
    p.tiles = ((int64_t)p.OH * p.OW + WD_TP - 1) / WD_TP;
  }
  p.rw = p.rmax + p.KH - 1;
  const int64_t win = C * p.rw * p.Wp;
  if (win >= (1 << 20)) return false;
  p.plane = (int)round_up(win + 1, 8);
  // two weight tiles, two sets of the five per-channel vectors, the tap table, the window
  p.lds = 2ll * 128 * p.wp * 2 + 2 * 5 * 128 * 4 + p.kp * 4 + 3ll * p.plane * 2;
  if (p.lds > kWideMaxLds || N * p.tiles >= (1ll << 31)) return false;
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

struct FirstInfer {
  const float* x;
  const float* w;
  const float *bias, *mean, *invstd, *gamma, *beta;   // bias, gamma and beta nullable
  void* out;
  int64_t Co, P2, Ppad2;
  int C, H, W, KH, KW, pad, OH, OW, PH, PW, Wp, Kt, wp, rw, plane, tiles, ctiles, form, Hp2, Wp2, pad2, ncb2;
};

__device__ __forceinline__ uint32_t quad_or(uint32_t v) {   // the OR over the lane's quad
  v |= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);   // quad_perm [1, 0, 3, 2]
  v |= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);   // quad_perm [2, 3, 0, 1]
  return v;
}

// LDS: ws [2][128][wp] bf16 weight tiles, ps [2][5][128] fp32 bias / mean / invstd / gamma / beta of the tile
// (0 / 0 / 0 / 1 / 0 where null or past Co), taps [Kp] window offsets (-1 beyond Kt), xs [3][plane] bf16 window
// planes -- element `win` of each plane is the zero every k >= Kt reads.
template <int KS, int POOL>
__global__ __launch_bounds__(WD_T, KS <= 3 ? 3 : 2) void conv_first_bnsign_k(FirstInfer a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t first_infer_smem[];
  constexpr int KP = 16 * KS;
  unsigned short* const ws = reinterpret_cast<unsigned short*>(first_infer_smem);
  float* const ps = reinterpret_cast<float*>(first_infer_smem + 2 * 128 * a.wp * 2);
  int* const taps = reinterpret_cast<int*>(ps + 2 * 5 * 128);
  unsigned short* const xs = reinterpret_cast<unsigned short*>(taps + KP);
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(), r = lane & 31, h = lane >> 5;
  const int64_t n = blockIdx.x / a.tiles;
  const int tile = (int)(blockIdx.x - n * a.tiles);
  const int win = a.C * a.rw * a.Wp, taps_hw = a.KH * a.KW;

  // out_form 0: the halo and the tail of the consumer's planes, 16 B per item, shared out over the grid
  if (a.form == 0) {
    uint8_t* planes = static_cast<uint8_t*>(a.out);
    const int64_t items = a.ncb2 * a.Ppad2 * 2, HpWp2 = (int64_t)a.Hp2 * a.Wp2;
    for (int64_t it = (int64_t)blockIdx.x * WD_T + tid; it < items; it += (int64_t)gridDim.x * WD_T) {
      const int64_t p2 = (it >> 1) % a.Ppad2;
      const int rem = (int)(p2 % HpWp2), hp = rem / a.Wp2 - a.pad2, wp = rem % a.Wp2 - a.pad2;
      if (p2 >= a.P2 || hp < 0 || hp >= a.PH || wp < 0 || wp >= a.PW) store_zero16(planes + it * 16);
    }
  }

  // this lane's output position (clamped past the image's last: gathered, never stored), the element of the
  // (pooled) map its result belongs to, and the tile's first output row
  int oh0, oh, ow, ph, pw;
  bool live;
  if constexpr (POOL == 0) {
    const int q0 = tile * WD_TP, OHW = a.OH * a.OW, q = q0 + 32 * wave + r, qc = min(q, OHW - 1);
    oh0 = q0 / a.OW, oh = qc / a.OW, ow = qc - oh * a.OW;
    ph = oh, pw = ow, live = q < OHW;
  } else {
    const int v0 = tile * FI_TW, PHW = a.PH * a.PW, v = v0 + 8 * wave + (r >> 2), vc = min(v, PHW - 1);
    ph = vc / a.PW, pw = vc - ph * a.PW;
    oh0 = 2 * (v0 / a.PW), oh = 2 * ph + ((r >> 1) & 1), ow = 2 * pw + (r & 1);
    live = v < PHW && (r & 3) == 0;   // a quad's first lane stores the window
  }

  auto stage_w = [&](int ct, int buf) {
    for (int e = tid; e < 128 * KP; e += WD_T) {
      const int cl = e / KP, k = e - cl * KP;
      const int64_t co = (int64_t)ct * 128 + cl;
      ws[(buf * 128 + cl) * a.wp + k] = co < a.Co && k < a.Kt ? tsign_bf16(a.w[co * a.Kt + k]) : (unsigned short)0;
    }
    for (int e = tid; e < 5 * 128; e += WD_T) {
      const int v = e >> 7;
      const int64_t co = (int64_t)ct * 128 + (e & 127);
      const float* src = v == 0 ? a.bias : v == 1 ? a.mean : v == 2 ? a.invstd : v == 3 ? a.gamma : a.beta;
      ps[buf * 5 * 128 + e] = src != nullptr && co < a.Co ? src[co] : (v == 3 ? 1.f : 0.f);
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

  // the lane's 3 KS position fragments, gathered once
  const int base = (oh - oh0) * a.Wp + ow;
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

  const int64_t pmap = (int64_t)a.PH * a.PW;
  const int64_t p2 = (n * a.Hp2 + ph + a.pad2) * a.Wp2 + pw + a.pad2;         // out_form 0: the position's row
  int8_t* const op = static_cast<int8_t*>(a.out) + n * a.Co * pmap + (int64_t)ph * a.PW + pw;   // out_form 1
  for (int ct = 0; ct < a.ctiles; ++ct) {
    const int buf = ct & 1;
    int64_t pm = pmap;
    asm volatile("" : "+s"(pm));   // opaque per tile: the 32 channel offsets are not kept in registers over the loop
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

    // BatchNorm and the three masks: bit 16 t + 4 g + j of block b is register 4 g + j of accumulator 2 b + t.
    // A channel past Co has zero weights and the neutral vectors: its bits are never stored.
    uint32_t mp[2] = {0u, 0u}, mz[2] = {0u, 0u}, mn[2] = {0u, 0u};
    {
#pragma clang fp contract(off)
      const float* const pt = ps + buf * 5 * 128;
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int cl = 32 * m + 8 * g + 4 * h;
          // one group's twenty values in registers at a time: the masks so far are pinned here, so the reads
          // below do not rise above the arithmetic of the group before
          asm volatile("" : "+v"(mp[m >> 1]), "+v"(mz[m >> 1]), "+v"(mn[m >> 1])::"memory");
          float v[5][4];
#pragma unroll
          for (int k = 0; k < 5; ++k) {
            const float4 f = *reinterpret_cast<const float4*>(pt + k * 128 + cl);
            v[k][0] = f.x, v[k][1] = f.y, v[k][2] = f.z, v[k][3] = f.w;
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float x = acc[m][4 * g + j] + v[0][j];
            const float y = bn_y1(x, v[1][j], 0.f, v[2][j], v[3][j], v[4][j]);
            const int bit = 16 * (m & 1) + 4 * g + j;
            mp[m >> 1] |= (uint32_t)(y > 0.f) << bit;
            mz[m >> 1] |= (uint32_t)(y == 0.f) << bit;
            mn[m >> 1] |= (uint32_t)(y != y) << bit;
          }
        }
    }

#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if constexpr (POOL == 2) mp[b] = quad_or(mp[b]), mz[b] = quad_or(mz[b]), mn[b] = quad_or(mn[b]);
      const uint32_t nz = ~(mn[b] | (mz[b] & ~mp[b]));       // the sign is not 0
      const uint32_t ng = nz & ~mp[b];                       // the sign is -1
      if (a.form == 0) {
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
        const int cbo = ct * 2 + b;
        if (live && cbo < a.ncb2)
          *reinterpret_cast<uint4*>(static_cast<uint8_t*>(a.out) + (cbo * a.Ppad2 + p2) * 32 + 16 * h) = o;
      } else if (live) {
        // the lane's 32 channels of the block in rising order, the pointer stepped from channel to channel
        const int64_t c0 = (int64_t)ct * 128 + 64 * b + 4 * h;
        int8_t* pq = op + c0 * pm;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int bit = 16 * t + 4 * g + j;
              if (c0 + 32 * t + 8 * g + j < a.Co)
                pq[j * pm] = (int8_t)((int)((nz >> bit) & 1u) - 2 * (int)((ng >> bit) & 1u));
            }
            pq += 8 * pm;
          }
      }
    }
    if (ct + 1 < a.ctiles) wide_barrier();   // tile ct+1 is staged; every wave has left buffer `buf`
  }
}

template <int KS, int POOL>
void first_infer_launch(const FirstInferPlan& p, const FirstInfer& a, hipStream_t st) {
  if (p.lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_first_bnsign_k<KS, POOL>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
  hipLaunchKernelGGL((conv_first_bnsign_k<KS, POOL>), dim3((unsigned)(p.N * p.tiles)), dim3(WD_T), (size_t)p.lds, st, a);
}

}  // namespace
}  // namespace bnn

using namespace bnn;

BNN_API int bnn_conv2d_fwd_first_bnsign_ok(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH,
                                           int64_t KW, int32_t stride, int32_t pad, int32_t dil, int32_t groups,
                                           int32_t pool, int32_t out_form, int64_t KH2, int64_t KW2, int32_t pad2) {
  FirstInferPlan p;
  return first_infer_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, pool, out_form, KH2, KW2, pad2, &p) ? 1 : 0;
}

BNN_API const char* bnn_conv2d_fwd_first_bnsign_kernel(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co,
                                                       int64_t KH, int64_t KW, int32_t stride, int32_t pad,
                                                       int32_t dil, int32_t groups, int32_t pool, int32_t out_form,
                                                       int64_t KH2, int64_t KW2, int32_t pad2) {
  static thread_local char buf[160];
  FirstInferPlan p;
  if (!first_infer_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, pool, out_form, KH2, KW2, pad2, &p)) return "";
  snprintf(buf, sizeof(buf), "conv_first_bnsign_k<%d,%d> form=%d lds=%lld rows=%d Kp=%d pitch=%d b128=%d", p.ks, p.pool,
           p.form, (long long)p.lds, p.rw, p.kp, p.wp, p.cycles);
  return buf;
}

BNN_API int bnn_conv2d_fwd_first_bnsign(const float* x, const float* w_latent, const float* bias, const float* mean,
                                        const float* invstd, const float* gamma, const float* beta, void* out,
                                        int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW,
                                        int32_t pad, int32_t pool, int32_t out_form, int64_t KH2, int64_t KW2,
                                        int32_t pad2, void* stream) {
  FirstInferPlan p;
  if (!first_infer_plan(N, C, H, W, Co, KH, KW, 1, pad, 1, 1, pool, out_form, KH2, KW2, pad2, &p)) {
    set_error("bnn_conv2d_fwd_first_bnsign: shape not taken (a geometry of bnn_conv2d_fwd_first, pool 0 or 2 with "
              "even OH and OW, the staged window within the LDS; out_form 0 needs Co %% 64 == 0 and a consumer "
              "geometry bnn_conv2d_wide_planes_bytes takes)");
    return kErrInval;
  }
  if (!x || !w_latent || !mean || !invstd || !out || (out_form == 0 && !aligned16(out))) {
    set_error("bnn_conv2d_fwd_first_bnsign: null pointer, or output planes not 16-B aligned");
    return kErrInval;
  }
  if (N == 0) return 0;
  const FirstInfer a{x, w_latent, bias, mean, invstd, gamma, beta, out, Co, p.P2, p.Ppad2, (int)C, (int)H, (int)W,
                     p.KH, p.KW, p.pad, p.OH, p.OW, p.PH, p.PW, p.Wp, p.Kt, p.wp, p.rw, p.plane, (int)p.tiles,
                     p.ctiles, p.form, p.Hp2, p.Wp2, p.pad2, p.ncb2};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define BNN_FI(KS_) \
  case KS_: p.pool ? first_infer_launch<KS_, 2>(p, a, st) : first_infer_launch<KS_, 0>(p, a, st); break
  switch (p.ks) {
    BNN_FI(1); BNN_FI(2); BNN_FI(3); BNN_FI(4);
    default: p.pool ? first_infer_launch<5, 2>(p, a, st) : first_infer_launch<5, 0>(p, a, st); break;
  }
#undef BNN_FI
  return check_launch("bnn_conv2d_fwd_first_bnsign");
}
