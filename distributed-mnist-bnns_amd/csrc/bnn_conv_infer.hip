// Frozen-model inference of the binarized CNN layers (bnn_amd.inference.FrozenCNN): the binary
// convolution with its eval-mode BatchNorm2d -> Hardtanh -> MaxPool2d(2, 2) folded into the epilogue.
//
//   bnn_conv2d_fwd_bnsign_pool    -> the next layer's ternary operand, int8 channels-innermost
//                                    [N][OH/2][OW/2][round_up(Co, 16)] (1 B per pooled element)
//   bnn_conv2d_fwd_bn_pool_linear -> the ten logits of Linear(Co PH PW -> 10) on the pooled map,
//                                    which is never written
//
// Hardtanh and max-pool are monotone, so sign(maxpool(hardtanh(bn(z)))) is the window maximum of
// sign(bn(z)), and bn on running statistics is a per-channel function of the conv's exact integer sum.
// The tile columns (MFMA) / lanes (dot4) are ordered by pooling window -- pixel index q = 4 window + j,
// j = 2 (oh & 1) + (ow & 1) -- so a window is a quad of adjacent lanes and its maximum is two DPP
// quad_perm steps.  Weights arrive packed (int8 signs, packed once at freeze time): the kernels stage
// them with straight 16-B copies and run no tsign per forward.  New kernel bodies: the training
// kernels of bnn_conv.hip are untouched.
#include <algorithm>

#include "bnn_common.h"

namespace bnn {
namespace {

constexpr int IF_T = 256;          // 4 waves
constexpr int IF_IPB_SIGN = 8;     // samples per workgroup (the weight staging amortises)
constexpr int IF_IPB_HEAD = 16;    // the head also stages the classifier weight (62.7 KB for the BinCNN)
constexpr int IF_C1_IPB = 4;
constexpr int IF_NOUT = 10;        // classifier outputs
constexpr int IF_OSLOT = 12;       // per (window, channel): outputs o = j + 4 k at slot 3 j + k (10, 11 zero)
constexpr int64_t kMaxInferLds = 160 * 1024;

struct BnP {   // conv bias and the BatchNorm's per-channel vectors (bias / gamma / beta nullable)
  const float *bias, *mean, *invstd, *gamma, *beta;
};

struct InfGeo {
  int C, H, W, Co, Cop, KH, KW, OH, OW, PH, PW, pad, Hp, Wp, CB, KC, KCp, ntile;
  int Wq, KWG;   // C == 1: row pitch of the sign bytes, dot4 groups per filter row
};

// quad_perm [1,0,3,2] / [2,3,0,1]: the other lanes of a pooling window
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_quad(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t quad_or(uint32_t v) {
  v |= dpp_quad<0xB1>(v);
  v |= dpp_quad<0x4E>(v);
  return v;
}
__device__ __forceinline__ double dpp_quad_d(double v, bool second) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = second ? dpp_quad<0x4E>((uint32_t)u) : dpp_quad<0xB1>((uint32_t)u);
  const uint32_t hi = second ? dpp_quad<0x4E>((uint32_t)(u >> 32)) : dpp_quad<0xB1>((uint32_t)(u >> 32));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ double quad_max(double v) {
  v = fmax(v, dpp_quad_d(v, false));
  return fmax(v, dpp_quad_d(v, true));
}

// y of one element as conv + bnn_bn2d_fwd_eval form it: x = fl(I + bias), then the shared element bn_y1
// (bnn_common.h), which bn2_window goes through as well
__device__ __forceinline__ float bn_y(int I, float b, float mu, float is, float ga, float be) {
#pragma clang fp contract(off)
  const float x = (float)I + b;
  return bn_y1(x, mu, 0.f, is, ga, be);
}

// bit r of a nibble -> bit 8 r (the four terms occupy disjoint bits: no carries)
__device__ __forceinline__ uint32_t spread4(uint32_t nib) { return (nib * 0x00204081u) & 0x01010101u; }

// 4 sign bytes of 4 channels from their window masks: positive somewhere -> +1; else a zero
// somewhere -> 0; else -1; a NaN anywhere in the window (or a pad channel) -> 0
__device__ __forceinline__ uint32_t sign_bytes4(uint32_t pos, uint32_t zero, uint32_t nan) {
  const uint32_t p = pos & ~nan & 0xFu, ng = ~(pos | zero | nan) & 0xFu;
  return spread4(p) | spread4(ng) * 0xFFu;
}

// The pixel of window-ordered index q (q < OH OW): q = 4 (ph PW + pw) + 2 dy + dx
__device__ __forceinline__ void window_pixel(int q, int PW, int* oh, int* ow, int* win) {
  const int w = q >> 2, ph = w / PW, pw = w - ph * PW;
  *win = w;
  *oh = 2 * ph + ((q >> 1) & 1);
  *ow = 2 * pw + (q & 1);
}

// ------------------------------------------------------------------ C == 1: dot4
// Sign bytes [Hp][Wq] and weight words [KH][KWG][CO] as conv_fwd_bin_c1_k (bnn_conv.hip), the words
// read ready-made from wq.  XIN 0: fp32 pixels, 1: u8 pixels through the 256-entry sign table, 2: int8 signs.
template <int CO, int KWG, int XIN>
__global__ __launch_bounds__(IF_T) void conv_bnsign_pool_c1_k(const void* __restrict__ x,
                                                              const int8_t* __restrict__ table,
                                                              const int* __restrict__ wq, BnP bn,
                                                              int8_t* __restrict__ out, int64_t N, InfGeo g) {
  extern __shared__ __attribute__((aligned(16))) int lds[];
  int* ws = lds;                                   // [KH][KWG][CO]
  int* tab = ws + g.KH * KWG * CO;                 // 256 sign bytes
  int* xw = tab + 64;                              // [Hp][Wq / 4] words of sign bytes (+ 16 slack bytes)
  const int t = threadIdx.x;
  const int nw = g.KH * KWG * CO, nxw = (g.Hp * g.Wq + 16) / 4;
  for (int i = t; i < nw; i += IF_T) ws[i] = wq[i];
  if (XIN == 1 && t < 64) tab[t] = reinterpret_cast<const int*>(table)[t];
  for (int i = t; i < nxw; i += IF_T) xw[i] = 0;
  int8_t* xb = reinterpret_cast<int8_t*>(xw);
  const int8_t* tb = reinterpret_cast<const int8_t*>(tab);
  const int nin = g.H * g.W, OHW = g.OH * g.OW, nchunk = g.Cop / 16;
  constexpr int NW = (CO + 31) / 32;
  const uint64_t padmask = g.Co >= 64 ? 0ull : ~((1ull << g.Co) - 1ull);
  const int64_t n0 = (int64_t)blockIdx.x * IF_C1_IPB, n1 = (n0 + IF_C1_IPB < N) ? n0 + IF_C1_IPB : N;
  for (int64_t n = n0; n < n1; ++n) {
    __syncthreads();   // the previous sample's reads are done (and the set-up above on entry)
    for (int i0 = t; i0 < nin; i0 += 4 * IF_T) {
      int s[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {   // clamped, unconditional loads: they batch
        const int64_t idx = n * nin + min(i0 + j * IF_T, nin - 1);
        if (XIN == 0) s[j] = tsign(reinterpret_cast<const float*>(x)[idx]);
        else if (XIN == 1) s[j] = reinterpret_cast<const uint8_t*>(x)[idx];
        else s[j] = reinterpret_cast<const int8_t*>(x)[idx];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = i0 + j * IF_T, ih = i / g.W, iw = i - ih * g.W;
        if (i < nin) xb[(ih + g.pad) * g.Wq + iw + g.pad] = (int8_t)(XIN == 1 ? tb[s[j]] : s[j]);
      }
    }
    __syncthreads();
    for (int q0 = 0; q0 < OHW; q0 += IF_T) {
      const int q = q0 + t;
      const bool valid = q < OHW;
      int oh, ow, win;
      window_pixel(valid ? q : 0, g.PW, &oh, &ow, &win);
      int acc[CO];
#pragma unroll
      for (int co = 0; co < CO; ++co) acc[co] = 0;
      for (int kh = 0; kh < g.KH; ++kh) {
        const int b = (oh + kh) * g.Wq + ow, sh = b & 3;
        const int* src = xw + (b >> 2);
        int d[KWG + 1];
#pragma unroll
        for (int k = 0; k <= KWG; ++k) d[k] = src[k];
        const int* wr = ws + kh * KWG * CO;
#pragma unroll
        for (int kg = 0; kg < KWG; ++kg) {
          const int xv = (int)__builtin_amdgcn_alignbyte((unsigned)d[kg + 1], (unsigned)d[kg], (unsigned)sh);
#pragma unroll
          for (int co = 0; co < CO; ++co) acc[co] = __builtin_amdgcn_sdot4(xv, wr[kg * CO + co], acc[co], false);
        }
      }
      uint32_t P[NW], Z[NW], Q[NW];
#pragma unroll
      for (int w = 0; w < NW; ++w) P[w] = 0, Z[w] = 0, Q[w] = (uint32_t)(padmask >> (32 * w));
#pragma unroll
      for (int co = 0; co < CO; ++co) {
        const int cc = min(co, g.Co - 1);   // pad channels: a valid address, their bit already set in Q
        const float y = bn_y(acc[co], bn.bias ? bn.bias[cc] : 0.f, bn.mean[cc], bn.invstd[cc],
                             bn.gamma ? bn.gamma[cc] : 1.f, bn.beta ? bn.beta[cc] : 0.f);
        P[co >> 5] |= (uint32_t)(y > 0.f) << (co & 31);
        Z[co >> 5] |= (uint32_t)(y == 0.f) << (co & 31);
        Q[co >> 5] |= (uint32_t)(y != y) << (co & 31);
      }
#pragma unroll
      for (int w = 0; w < NW; ++w) P[w] = quad_or(P[w]), Z[w] = quad_or(Z[w]), Q[w] = quad_or(Q[w]);
      // lane j of the window writes channels 16 j .. 16 j + 15
      const int j = q & 3, hw = (NW > 1) ? (j >> 1) : 0, sh16 = 16 * (j & 1);
      const uint32_t p16 = (hw ? P[NW - 1] : P[0]) >> sh16, z16 = (hw ? Z[NW - 1] : Z[0]) >> sh16,
                     n16 = (hw ? Q[NW - 1] : Q[0]) >> sh16;
      if (valid && j < nchunk) {
        v4i o;
        o.x = (int)sign_bytes4(p16, z16, n16);
        o.y = (int)sign_bytes4(p16 >> 4, z16 >> 4, n16 >> 4);
        o.z = (int)sign_bytes4(p16 >> 8, z16 >> 8, n16 >> 8);
        o.w = (int)sign_bytes4(p16 >> 12, z16 >> 12, n16 >> 12);
        *reinterpret_cast<v4i*>(out + ((n * g.PH * g.PW + win) * (int64_t)g.Cop + 16 * j)) = o;
      }
    }
  }
}

// ------------------------------------------------------------------ C % 16 == 0: int8 MFMA
// The implicit GEMM of conv_fwd_i8mfma_k (bnn_conv.hip): ws[COT 16][KCp 16] x xs[Hp][Wp][C], K order
// (tap, 16-channel chunk), D row = channel 4 (l >> 4) + r of tile a, D column = pixel (l & 15).

// packed weight rows [round_up(Co, 16)][KCp 16] -> ws (rows beyond them zero), 16-B copies
template <int COT>
__device__ __forceinline__ void stage_weights(const int8_t* __restrict__ wq, int8_t* ws, const InfGeo& g) {
  const int n16 = COT * 16 * g.KCp, have = g.Cop * g.KCp;
  const v4i* src = reinterpret_cast<const v4i*>(wq);
  v4i* dst = reinterpret_cast<v4i*>(ws);
  for (int i = threadIdx.x; i < n16; i += IF_T) dst[i] = i < have ? src[i] : v4i{0, 0, 0, 0};
}

// per-channel vectors -> prm[5][CT] (bias, mean, invstd, gamma, beta); pad channels all zero (y = 0)
__device__ __forceinline__ void stage_params(const BnP& bn, float* prm, int CT, int Co) {
  for (int i = threadIdx.x; i < 5 * CT; i += IF_T) {
    const int k = i / CT, c = i - k * CT, cc = min(c, Co - 1);
    float v;
    if (k == 0) v = bn.bias ? bn.bias[cc] : 0.f;
    else if (k == 1) v = bn.mean[cc];
    else if (k == 2) v = bn.invstd[cc];
    else if (k == 3) v = bn.gamma ? bn.gamma[cc] : 1.f;
    else v = bn.beta ? bn.beta[cc] : 0.f;
    prm[i] = c < Co ? v : 0.f;
  }
}

// one sample's image into the zero-haloed xs[Hp][Wp][C].  XIN 2: int8 channels-innermost signs, a row
// is W C contiguous bytes on both sides -> 16-B copies; XIN 0: fp32 NCHW, binarised here.
template <int XIN>
__device__ __forceinline__ void stage_image(const void* __restrict__ x, int64_t n, int8_t* xs, const InfGeo& g) {
  const int t = threadIdx.x;
  if (XIN == 2) {
    const int rowc = g.W * g.C / 16, tot = g.H * rowc;
    const v4i* src = reinterpret_cast<const v4i*>(reinterpret_cast<const int8_t*>(x) + n * (int64_t)(g.H * g.W * g.C));
    for (int i = t; i < tot; i += IF_T) {
      const int ih = i / rowc, k = i - ih * rowc;
      *reinterpret_cast<v4i*>(xs + ((ih + g.pad) * g.Wp + g.pad) * g.C + 16 * k) = src[i];
    }
  } else {
    const int HW = g.H * g.W, tot = g.C * HW;
    const float* xn = reinterpret_cast<const float*>(x) + n * (int64_t)tot;
    for (int i0 = t; i0 < tot; i0 += 8 * IF_T) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = xn[min(i0 + k * IF_T, tot - 1)];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int i = i0 + k * IF_T, c = i / HW, r = i - c * HW, ih = r / g.W, iw = r - ih * g.W;
        if (i < tot) xs[((ih + g.pad) * g.Wp + iw + g.pad) * g.C + c] = (int8_t)tsign(v[k]);
      }
    }
  }
}

// this wave's tiles wv, wv + 4, wv + 8, wv + 12 in window order: LDS offset of each lane's pixel
// (clamped: computed, never used) and its window
struct TileMap {
  int pbase[4], win[4];
  bool valid[4];
};

__device__ __forceinline__ TileMap tile_map(const InfGeo& g, int wv, int lane) {
  TileMap m;
  const int OHW = g.OH * g.OW;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = (wv + 4 * i) * 16 + (lane & 15);
    m.valid[i] = q < OHW;
    int oh, ow;
    window_pixel(m.valid[i] ? q : 0, g.PW, &oh, &ow, &m.win[i]);
    m.pbase[i] = (oh * g.Wp + ow) * g.C;
  }
  return m;
}

template <int COT>
__device__ __forceinline__ void conv_tiles(const int8_t* ws, const int8_t* xs, const InfGeo& g, const TileMap& tm,
                                           int lane, v4i (&acc)[COT][4]) {
  const int h = lane >> 4, rowb = g.KCp * 16;
#pragma unroll
  for (int a = 0; a < COT; ++a)
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[a][m] = v4i{0, 0, 0, 0};
  for (int ks = 0; ks < g.KCp / 4; ++ks) {
    const int ch = min(4 * ks + h, g.KC - 1);   // padded chunks: zero weights, valid address
    const int tap = ch / g.CB, cb = ch - tap * g.CB;
    const int kh = tap / g.KW, kw = tap - kh * g.KW;
    const int xo = (kh * g.Wp + kw) * g.C + cb * 16;
    v4i av[COT], bv[4];
#pragma unroll
    for (int a = 0; a < COT; ++a)
      av[a] = *reinterpret_cast<const v4i*>(ws + (a * 16 + (lane & 15)) * rowb + (4 * ks + h) * 16);
#pragma unroll
    for (int m = 0; m < 4; ++m) bv[m] = *reinterpret_cast<const v4i*>(xs + tm.pbase[m] + xo);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int a = 0; a < COT; ++a)
        acc[a][m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[a], bv[m], acc[a][m], 0, 0, 0);
  }
}

__device__ __forceinline__ void ld4f(const float* p, float (&v)[4]) {
  const float4 f = *reinterpret_cast<const float4*>(p);
  v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
}

template <int COT, int XIN>
__global__ __launch_bounds__(IF_T) void conv_bnsign_pool_mfma_k(const void* __restrict__ x,
                                                                const int8_t* __restrict__ wq, BnP bn,
                                                                int8_t* __restrict__ out, int64_t N, InfGeo g) {
  extern __shared__ __attribute__((aligned(16))) float ldsf[];
  constexpr int CT = COT * 16;
  float* prm = ldsf;                                            // [5][CT]
  int8_t* ws = reinterpret_cast<int8_t*>(prm + 5 * CT);         // [CT][KCp 16]
  int8_t* xs = ws + CT * g.KCp * 16;                            // [Hp][Wp][C]
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, h = lane >> 4;
  stage_weights<COT>(wq, ws, g);
  stage_params(bn, prm, CT, g.Co);
  const int nxs = g.Hp * g.Wp * g.C;
  for (int i = t; i < nxs / 4; i += IF_T) reinterpret_cast<int*>(xs)[i] = 0;
  const TileMap tm = tile_map(g, wv, lane);
  const int cot = g.Cop / 16, jj = lane & 3;
  const int64_t n0 = (int64_t)blockIdx.x * IF_IPB_SIGN, n1 = (n0 + IF_IPB_SIGN < N) ? n0 + IF_IPB_SIGN : N;
  for (int64_t n = n0; n < n1; ++n) {
    __syncthreads();   // the previous sample's fragment reads are done (and the set-up above on entry)
    stage_image<XIN>(x, n, xs, g);
    __syncthreads();
    v4i acc[COT][4];
    conv_tiles<COT>(ws, xs, g, tm, lane, acc);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      uint32_t P = 0, ZQ = 0;   // bit 4 a + r: positive; zero | NaN-or-pad << 16
#pragma unroll
      for (int a = 0; a < COT; ++a) {
        float b[4], mu[4], is[4], ga[4], be[4];
        const int c0 = a * 16 + 4 * h;
        ld4f(prm + c0, b), ld4f(prm + CT + c0, mu), ld4f(prm + 2 * CT + c0, is), ld4f(prm + 3 * CT + c0, ga);
        ld4f(prm + 4 * CT + c0, be);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float y = bn_y(acc[a][m][r], b[r], mu[r], is[r], ga[r], be[r]);
          const int bit = 4 * a + r;
          P |= (uint32_t)(y > 0.f) << bit;
          ZQ |= (uint32_t)(y == 0.f) << bit;
          ZQ |= (uint32_t)(y != y || c0 + r >= g.Co) << (16 + bit);
        }
      }
      P = quad_or(P), ZQ = quad_or(ZQ);
      // lane jj of the window writes the 4 channels 16 jj + 4 h .. + 3 of channel tile a = jj
      if (tm.valid[m] && jj < cot) {
        const uint32_t word = sign_bytes4(P >> (4 * jj), ZQ >> (4 * jj), ZQ >> (16 + 4 * jj));
        *reinterpret_cast<uint32_t*>(out + ((n * g.PH * g.PW + tm.win[m]) * (int64_t)g.Cop + 16 * jj + 4 * h)) = word;
      }
    }
  }
}

// conv -> BatchNorm2d -> Hardtanh -> MaxPool2d(2, 2) -> Linear(Co PH PW -> 10).  From the exact integer
// sum on, every step is in double (x = fl(I + bias) is the one fp32 rounding), so a logit carries the
// final rounding to fp32 and nothing else.  Reduction order, fixed: per lane over its tiles, channel
// tiles and rows; the 16 lanes of a wave holding the same outputs by xor-shuffles 4, 8, 16, 32; the
// 4 waves in order; the bias last.  No atomics; a sample's logits depend on that sample alone.
template <int COT>
__global__ __launch_bounds__(IF_T) void conv_bn_pool_linear_k(const int8_t* __restrict__ x,
                                                              const int8_t* __restrict__ wq, BnP bn,
                                                              const float* __restrict__ fcw,
                                                              const float* __restrict__ fcb,
                                                              float* __restrict__ logits, int64_t N, InfGeo g,
                                                              int ipb) {
  extern __shared__ __attribute__((aligned(16))) float ldsf[];
  constexpr int CT = COT * 16;
  const int PP = g.PH * g.PW, WS = CT * IF_OSLOT + 4;           // window stride of fcl (floats)
  double* red = reinterpret_cast<double*>(ldsf);                // [IF_IPB_HEAD][4 waves][IF_OSLOT]
  float* prm = reinterpret_cast<float*>(red + IF_IPB_HEAD * 4 * IF_OSLOT);   // [5][CT]
  float* fcl = prm + 5 * CT;                                    // [PP][WS]: (window, channel, slot)
  int8_t* ws = reinterpret_cast<int8_t*>(fcl + PP * WS);        // [CT][KCp 16]
  int8_t* xs = ws + CT * g.KCp * 16;                            // [Hp][Wp][C]
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, h = lane >> 4, jj = lane & 3;
  stage_weights<COT>(wq, ws, g);
  stage_params(bn, prm, CT, g.Co);
  const int nxs = g.Hp * g.Wp * g.C;
  for (int i = t; i < nxs / 4; i += IF_T) reinterpret_cast<int*>(xs)[i] = 0;
  for (int i = t; i < PP * WS; i += IF_T) fcl[i] = 0.f;
  __syncthreads();
  {   // torch's [10][Co PP] (NCHW flatten: feature co PP + window), read in memory order
    const int F = g.Co * PP;
    for (int i = t; i < IF_NOUT * F; i += IF_T) {
      const int o = i / F, f = i - o * F, co = f / PP, w = f - co * PP;
      fcl[w * WS + co * IF_OSLOT + (o & 3) * 3 + (o >> 2)] = fcw[i];
    }
  }
  const TileMap tm = tile_map(g, wv, lane);
  const int64_t n0 = (int64_t)blockIdx.x * ipb, n1 = (n0 + ipb < N) ? n0 + ipb : N;
  for (int64_t n = n0; n < n1; ++n) {
    __syncthreads();
    stage_image<2>(x, n, xs, g);
    __syncthreads();
    v4i acc[COT][4];
    conv_tiles<COT>(ws, xs, g, tm, lane, acc);
    double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
      for (int a = 0; a < COT; ++a) {
        float b[4], mu[4], is[4], ga[4], be[4];
        const int c0 = a * 16 + 4 * h;
        ld4f(prm + c0, b), ld4f(prm + CT + c0, mu), ld4f(prm + 2 * CT + c0, is), ld4f(prm + 3 * CT + c0, ga);
        ld4f(prm + 4 * CT + c0, be);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float xf = (float)acc[a][m][r] + b[r];
          const double y = fma(((double)xf - (double)mu[r]) * (double)is[r], (double)ga[r], (double)be[r]);
          double f = quad_max(fmin(fmax(y, -1.0), 1.0));
          if (!tm.valid[m]) f = 0.0;
          const float* wp = fcl + tm.win[m] * WS + (c0 + r) * IF_OSLOT + 3 * jj;
#pragma unroll
          for (int k = 0; k < 3; ++k) s[k] = fma(f, (double)wp[k], s[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int o = 4; o < 64; o <<= 1) s[k] += __shfl_xor(s[k], o, 64);
    }
    if (lane < 4) {
#pragma unroll
      for (int k = 0; k < 3; ++k) red[((int)(n - n0) * 4 + wv) * IF_OSLOT + 3 * lane + k] = s[k];
    }
  }
  __syncthreads();
  const int ns = (int)(n1 - n0);
  if (t < ns * IF_NOUT) {
    const int sidx = t / IF_NOUT, o = t - sidx * IF_NOUT, slot = (o & 3) * 3 + (o >> 2);
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < 4; ++w) v += red[(sidx * 4 + w) * IF_OSLOT + slot];
    v += fcb ? (double)fcb[o] : 0.0;
    logits[(n0 + sidx) * IF_NOUT + o] = (float)v;
  }
}

// ------------------------------------------------------------------ host side
inline int pick_co(int64_t co) { return co <= 8 ? 8 : co <= 16 ? 16 : co <= 32 ? 32 : 64; }

// geometry both entries take (bnn.h): 0 = refused, 1 = the int8-MFMA kernels, 2 = the single-channel dot4 kernel
int infer_geom(int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride, int32_t pad,
               int32_t dil, int32_t groups, InfGeo* out) {
  if (C <= 0 || H <= 0 || W <= 0 || Co <= 0 || KH <= 0 || KW <= 0 || pad < 0) return 0;
  if (stride != 1 || dil != 1 || groups != 1 || Co > 64 || pad > KH - 1 || pad > KW - 1) return 0;
  if (H > 4096 || W > 4096 || KH > 64 || KW > 64) return 0;
  const int64_t OH = H + 2 * pad - KH + 1, OW = W + 2 * pad - KW + 1;
  if (OH <= 0 || OW <= 0 || OH % 2 != 0 || OW % 2 != 0) return 0;
  InfGeo d{};
  d.C = (int)C, d.H = (int)H, d.W = (int)W, d.Co = (int)Co, d.Cop = (int)round_up(Co, 16);
  d.KH = (int)KH, d.KW = (int)KW, d.OH = (int)OH, d.OW = (int)OW, d.PH = (int)OH / 2, d.PW = (int)OW / 2;
  d.pad = pad, d.Hp = d.H + 2 * pad, d.Wp = d.W + 2 * pad;
  if (C == 1) {
    if (KW > 8 || (int64_t)d.Hp * d.Wp > (1 << 20)) return 0;
    d.Wq = (int)round_up(d.Wp, 4);
    d.KWG = KW <= 4 ? 1 : 2;
    *out = d;
    return 2;
  }
  if (C % 16 != 0 || C > 64) return 0;
  d.CB = d.C / 16;
  d.KC = d.KH * d.KW * d.CB;
  d.KCp = (int)round_up(d.KC, 4);
  d.ntile = (d.OH * d.OW + 15) / 16;
  if (d.ntile > 16 || (int64_t)d.C * d.H * d.W >= (1 << 20)) return 0;
  // gathered pixel (oh + kh, ow + kw) stays inside the padded image
  if (d.OH - 1 + d.KH - 1 >= d.Hp || d.OW - 1 + d.KW - 1 >= d.Wp) return 0;
  *out = d;
  return 1;
}

inline int cot_of(const InfGeo& g) { return g.Cop / 16 == 3 ? 4 : g.Cop / 16; }

inline int64_t c1_lds(const InfGeo& g) {
  return ((int64_t)g.KH * g.KWG * pick_co(g.Co) + 64) * 4 + (int64_t)g.Hp * g.Wq + 16;
}
inline int64_t mfma_lds(const InfGeo& g) {
  const int64_t ct = cot_of(g) * 16;
  return 5 * ct * 4 + ct * g.KCp * 16 + round_up((int64_t)g.Hp * g.Wp * g.C, 16);
}
inline int64_t head_lds(const InfGeo& g) {
  const int64_t ct = cot_of(g) * 16;
  return (int64_t)IF_IPB_HEAD * 4 * IF_OSLOT * 8 + (int64_t)g.PH * g.PW * (ct * IF_OSLOT + 4) * 4 + mfma_lds(g);
}

template <typename K>
inline void allow_lds(K kernel, int64_t bytes) {
  if (bytes > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)bytes);
}

#define BNN_IF_LAUNCH(KER, grid, lds, st, ...) \
  do { allow_lds(KER, (int64_t)(lds)); hipLaunchKernelGGL(KER, grid, dim3(IF_T), (size_t)(lds), st, __VA_ARGS__); } while (0)

bool sign_pool_path(int32_t xfmt, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride,
                    int32_t pad, int32_t dil, int32_t groups, InfGeo* g, int* path) {
  if (xfmt < 0 || xfmt > 2) return false;
  *path = infer_geom(C, H, W, Co, KH, KW, stride, pad, dil, groups, g);
  if (*path == 0) return false;
  if (xfmt == 1 && *path != 2) return false;   // u8 pixels: one channel
  return (*path == 2 ? c1_lds(*g) : mfma_lds(*g)) <= kMaxInferLds;
}

bool head_path(int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride, int32_t pad,
               int32_t dil, int32_t groups, int64_t n_out, InfGeo* g) {
  if (n_out != IF_NOUT) return false;
  if (infer_geom(C, H, W, Co, KH, KW, stride, pad, dil, groups, g) != 1) return false;
  return head_lds(*g) <= kMaxInferLds;
}

template <int XIN>
void launch_c1(const void* x, const int8_t* table, const int8_t* wq, const BnP& bn, int8_t* out, int64_t N,
               const InfGeo& g, hipStream_t st) {
  const dim3 grid((unsigned)((N + IF_C1_IPB - 1) / IF_C1_IPB));
  const int64_t lds = c1_lds(g);
  const int* w = reinterpret_cast<const int*>(wq);
#define BNN_IF_C1(CO_, KG_) BNN_IF_LAUNCH((conv_bnsign_pool_c1_k<CO_, KG_, XIN>), grid, lds, st, x, table, w, bn, out, N, g)
  switch (pick_co(g.Co) * 4 + g.KWG) {
    case 8 * 4 + 1: BNN_IF_C1(8, 1); break;
    case 8 * 4 + 2: BNN_IF_C1(8, 2); break;
    case 16 * 4 + 1: BNN_IF_C1(16, 1); break;
    case 16 * 4 + 2: BNN_IF_C1(16, 2); break;
    case 32 * 4 + 1: BNN_IF_C1(32, 1); break;
    case 32 * 4 + 2: BNN_IF_C1(32, 2); break;
    case 64 * 4 + 1: BNN_IF_C1(64, 1); break;
    default: BNN_IF_C1(64, 2); break;
  }
#undef BNN_IF_C1
}

template <int XIN>
void launch_mfma(const void* x, const int8_t* wq, const BnP& bn, int8_t* out, int64_t N, const InfGeo& g,
                 hipStream_t st) {
  const dim3 grid((unsigned)((N + IF_IPB_SIGN - 1) / IF_IPB_SIGN));
  const int64_t lds = mfma_lds(g);
  switch (cot_of(g)) {
    case 1: BNN_IF_LAUNCH((conv_bnsign_pool_mfma_k<1, XIN>), grid, lds, st, x, wq, bn, out, N, g); break;
    case 2: BNN_IF_LAUNCH((conv_bnsign_pool_mfma_k<2, XIN>), grid, lds, st, x, wq, bn, out, N, g); break;
    default: BNN_IF_LAUNCH((conv_bnsign_pool_mfma_k<4, XIN>), grid, lds, st, x, wq, bn, out, N, g); break;
  }
}

}  // namespace
}  // namespace bnn

using namespace bnn;

BNN_API int bnn_conv2d_fwd_bnsign_pool_ok(int32_t xfmt, int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co,
                                          int64_t KH, int64_t KW, int32_t stride, int32_t pad, int32_t dil,
                                          int32_t groups) {
  InfGeo g;
  int path = 0;
  return N >= 0 && sign_pool_path(xfmt, C, H, W, Co, KH, KW, stride, pad, dil, groups, &g, &path) ? 1 : 0;
}

BNN_API int bnn_conv2d_fwd_bnsign_pool(const void* x, int32_t xfmt, const int8_t* table, const int8_t* wq,
                                       const float* bias, const float* mean, const float* invstd, const float* gamma,
                                       const float* beta, int8_t* out, int64_t N, int64_t C, int64_t H, int64_t W,
                                       int64_t Co, int64_t KH, int64_t KW, int32_t stride, int32_t pad, int32_t dil,
                                       int32_t groups, void* stream) {
  InfGeo g;
  int path = 0;
  if (!x || !wq || !mean || !invstd || !out || N < 0 || !aligned16(out) || !aligned16(wq) ||
      (xfmt == 1 && (!table || (reinterpret_cast<uintptr_t>(table) & 3u))) ||
      (xfmt == 0 && (reinterpret_cast<uintptr_t>(x) & 3u)) ||
      !sign_pool_path(xfmt, C, H, W, Co, KH, KW, stride, pad, dil, groups, &g, &path) ||
      (xfmt == 2 && path == 1 && !aligned16(x))) {
    set_error("bnn_conv2d_fwd_bnsign_pool: bad arguments (xfmt 0 fp32 NCHW / 1 u8 pixels + table, C == 1 / 2 int8 "
              "channels-innermost signs; stride 1, dilation 1, groups 1, C == 1 or C %% 16 == 0 up to 64, Co <= 64, "
              "pad <= K - 1, even OH and OW, at most 256 output pixels for C > 1; wq, out 16-B aligned)");
    return kErrInval;
  }
  if (N == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const BnP bn{bias, mean, invstd, gamma, beta};
  if (path == 2) {
    if (xfmt == 0) launch_c1<0>(x, table, wq, bn, out, N, g, st);
    else if (xfmt == 1) launch_c1<1>(x, table, wq, bn, out, N, g, st);
    else launch_c1<2>(x, table, wq, bn, out, N, g, st);
  } else {
    if (xfmt == 0) launch_mfma<0>(x, wq, bn, out, N, g, st);
    else launch_mfma<2>(x, wq, bn, out, N, g, st);
  }
  return check_launch("bnn_conv2d_fwd_bnsign_pool");
}

BNN_API int bnn_conv2d_fwd_bn_pool_linear_ok(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH,
                                             int64_t KW, int32_t stride, int32_t pad, int32_t dil, int32_t groups,
                                             int32_t n_out) {
  InfGeo g;
  return N >= 0 && head_path(C, H, W, Co, KH, KW, stride, pad, dil, groups, n_out, &g) ? 1 : 0;
}

BNN_API int bnn_conv2d_fwd_bn_pool_linear(const int8_t* x, const int8_t* wq, const float* bias, const float* mean,
                                          const float* invstd, const float* gamma, const float* beta,
                                          const float* fcw, const float* fcb, int32_t n_out, float* logits, int64_t N,
                                          int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW,
                                          int32_t stride, int32_t pad, int32_t dil, int32_t groups, void* stream) {
  InfGeo g;
  if (!x || !wq || !mean || !invstd || !fcw || !logits || N < 0 || !aligned16(x) || !aligned16(wq) ||
      (reinterpret_cast<uintptr_t>(logits) & 3u) || (reinterpret_cast<uintptr_t>(fcw) & 3u) ||
      !head_path(C, H, W, Co, KH, KW, stride, pad, dil, groups, n_out, &g)) {
    set_error("bnn_conv2d_fwd_bn_pool_linear: bad arguments (int8 channels-innermost signs, C %% 16 == 0 up to 64, "
              "Co <= 64, stride 1, dilation 1, groups 1, pad <= K - 1, even OH and OW, at most 256 output pixels, "
              "n_out == 10, conv weights + image + classifier weight within one workgroup's LDS; x, wq 16-B aligned)");
    return kErrInval;
  }
  if (N == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const BnP bn{bias, mean, invstd, gamma, beta};
  // samples per workgroup: the classifier weight's staging amortises, small batches still spread over the CUs
  const int ipb = N >= 4096 ? IF_IPB_HEAD : N >= 1024 ? 8 : 4;
  const dim3 grid((unsigned)((N + ipb - 1) / ipb));
  const int64_t lds = head_lds(g);
  switch (cot_of(g)) {
    case 1: BNN_IF_LAUNCH((conv_bn_pool_linear_k<1>), grid, lds, st, x, wq, bn, fcw, fcb, logits, N, g, ipb); break;
    case 2: BNN_IF_LAUNCH((conv_bn_pool_linear_k<2>), grid, lds, st, x, wq, bn, fcw, fcb, logits, N, g, ipb); break;
    default: BNN_IF_LAUNCH((conv_bn_pool_linear_k<4>), grid, lds, st, x, wq, bn, fcw, fcb, logits, N, g, ipb); break;
  }
  return check_launch("bnn_conv2d_fwd_bn_pool_linear");
}
