// Wide-channel binary conv2d filter and bias gradient (the shapes bnn_conv2d_fwd_wide takes):
//   dw[co,c,kh,kw] = sum_{n,oh,ow} dy[n,co,oh,ow] * tsign(x[n,c,oh+kh-pad,ow+kw-pad])      db[co] = sum dy[n,co,oh,ow]
// as a GEMM on v_mfma_f32_32x32x16_bf16 whose contraction runs over positions.  dY enters as its exact
// three-plane bf16 split (bf16x3_split) and x as ternary bf16, so every product is exact; the roundings are
// the MFMA's fp32 accumulation, the fp32 partials and one final rounding.  No atomics: deterministic.
//
// K grid: k = (n Hp + hp) OWq + j with Hp = H + 2 pad rows per sample and OWq = round_up(OW, 8) columns.
// dy(oh, ow) sits at (oh, ow); rows hp >= OH and columns j >= OW are zero.  x is stored KW times: copy kw
// holds at (hp, j) the value tsign(x[n, c, hp - pad, j + kw - pad]) (zero outside the image), so tap (kh, kw)
// at dy position k reads copy kw at k + kh OWq -- a shift by whole 8-position pieces, no border special.
// Both operands are stored piece-major: per 64-channel block and piece of 8 consecutive k one contiguous
// KiB, channel ch at byte 16 ch:  dq [3 planes][ceil(Co/64)][Kp][1 KiB],  xq [KW][C/64][Kp][1 KiB].
// A fragment read -- lane (r, h) -> piece p + h, channel 32 w + r, one ds_read_b128 -- is then the MFMA
// operand "8 consecutive k of one channel" and covers 512 contiguous bytes per half wave.
//
// Four launches per call:
//  1. conv_wide_bwd_filter_pack_dy_k  fp32 NCHW -> the three planes; the row's per-channel sums -> bsum [N OH][Co].
//  2. conv_wide_bwd_filter_pack_x_k   fp32 NCHW -> the KW shifted ternary copies (bnn_conv2d_bwd_filter_wide_planes:
//                                     conv_wide_bwd_filter_pack_x_planes_k, the same copies from the layer's FP4 planes).
//  3. conv_wide_bwd_filter_k<NT, NBUF>  a workgroup owns 64 output x 64 input channels x one tap group x one
//                                     K slice; fp32 partials -> part [split][tap][Co64][C].
//  4. conv_wide_bwd_filter_reduce_k   the slices summed in index order in double, bsum over its rows in
//                                     double, one rounding to fp32.
// Every call writes every byte of dq and xq (halo, Co tail, columns j >= OW, rows hp >= OH, plane tails).
#include "bnn_conv_wide.h"

#include <cstdio>
#include <type_traits>

#include "bnn.h"

namespace bnn {
namespace {

constexpr int kFiltRounds = 2;     // the K split aims at this many rounds of workgroups on kFiltCUs CUs
constexpr int kFiltCUs = 256;
constexpr int kFiltMaxChunk = 16;  // pieces per chunk at most (a slice is a whole number of chunks)

struct WideFiltPlan {
  int64_t N, C, H, W, Co;
  int KH, KW, pad, Hp, OH, OW, OWq8, taps;
  int nco, ncb;        // 64-channel blocks of Co (rounded up) and of C
  int grows, ngroup;   // kh rows of a tap group, tap groups
  int nt;              // compiled accumulator sets: the smallest of 1, 3, 5, 9 that holds grows KW taps
  int ch;              // pieces per chunk (even: a k-step is two pieces)
  int nbuf;            // 2 = the next chunk's copy runs under this chunk's MFMAs, 1 = it does not fit
  int ring;            // ring slots (pieces) per x copy: nbuf ch + the group's halo
  int cycles;          // modelled LDS cycles of the worst fragment ds_read_b128 (4 = conflict-free)
  int64_t T;           // live pieces N Hp OWq / 8
  int64_t cps, splits; // chunks per K slice, K slices
  int64_t Kp;          // pieces per block and plane / copy: splits cps ch + (KH-1) OWq / 8
  int64_t lds, xq_off, part_off, bsum_off, work_bytes;
};

// Every fragment read of the shape through the bank model: the three dY planes, and every kh row of a tap
// group with its two pieces in neighbouring ring slots and across the ring's wrap, for both wave columns.
int wide_filt_frag_cycles(const WideFiltPlan& p) {
  int worst = 0, addr[64];
  for (int w = 0; w < 2; ++w) {
    for (int pl = 0; pl < 3; ++pl) {
      for (int l = 0; l < 64; ++l) addr[l] = (pl * p.ch + (l >> 5)) * 1024 + (32 * w + (l & 31)) * 16;
      worst = std::max(worst, lds_b128_cycles(addr));
    }
    for (int kh = 0; kh < p.grows; ++kh)
      for (int wrap = 0; wrap < 2; ++wrap) {
        const int s0 = wrap ? p.ring - 1 : (kh * p.OWq8) % p.ring, s1 = (s0 + 1) % p.ring;
        for (int l = 0; l < 64; ++l) addr[l] = ((l >> 5) ? s1 : s0) * 1024 + (32 * w + (l & 31)) * 16;
        worst = std::max(worst, lds_b128_cycles(addr));
      }
  }
  return worst;
}

bool wide_filt_plan_make(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW,
                         int32_t stride, int32_t pad, int32_t dil, int32_t groups, WideFiltPlan* out) {
  if (!bnn_conv2d_fwd_wide_ok(N, C, H, W, Co, KH, KW, stride, pad, dil, groups) || KW > 9) return false;
  WideFiltPlan p{};
  p.N = N, p.C = C, p.H = H, p.W = W, p.Co = Co;
  p.KH = (int)KH, p.KW = (int)KW, p.pad = pad, p.taps = p.KH * p.KW;
  p.Hp = (int)H + 2 * pad, p.OH = p.Hp - p.KH + 1, p.OW = (int)W + 2 * pad - p.KW + 1;
  p.OWq8 = (p.OW + 7) / 8;
  p.nco = (int)((Co + 63) / 64), p.ncb = (int)(C / 64);
  // tap groups: whole kh rows, at most 9 taps
  p.grows = std::min(p.KH, std::max(1, 9 / p.KW));
  p.ngroup = (p.KH + p.grows - 1) / p.grows;
  const int cnt = p.grows * p.KW;
  p.nt = cnt <= 1 ? 1 : cnt <= 3 ? 3 : cnt <= 5 ? 5 : 9;
  // the stage: nbuf x three planes x ch pieces of dY, and per copy a ring of nbuf ch + halo pieces
  const int64_t hq = (int64_t)(p.grows - 1) * p.OWq8;
  const int64_t cap = kWideMaxLds / 1024;
  for (p.nbuf = 2; p.nbuf >= 1; --p.nbuf) {
    int64_t ch = (cap - p.KW * hq) / (p.nbuf * (3 + p.KW));   // nbuf (3 + KW) ch + KW hq <= 160 KiB
    ch = std::min<int64_t>(ch & ~1ll, kFiltMaxChunk);
    if (ch >= (p.nbuf == 2 ? 4 : 2)) {
      p.ch = (int)ch;
      break;
    }
  }
  if (p.nbuf < 1) return false;   // two pieces of dY and the ring of a single stage do not fit
  p.ring = p.nbuf * p.ch + (int)hq;
  p.lds = ((int64_t)p.nbuf * 3 * p.ch + (int64_t)p.KW * p.ring) * 1024;
  p.cycles = wide_filt_frag_cycles(p);
  // the K split: tiles x slices is about kFiltRounds rounds of one workgroup per CU
  p.T = N * p.Hp * p.OWq8;
  const int64_t chunks = std::max<int64_t>(1, (p.T + p.ch - 1) / p.ch);
  const int64_t tiles = (int64_t)p.nco * p.ncb * p.ngroup;
  const int64_t want = std::min(chunks, std::max<int64_t>(1, (kFiltRounds * kFiltCUs + tiles - 1) / tiles));
  p.cps = (chunks + want - 1) / want;
  p.splits = (chunks + p.cps - 1) / p.cps;
  p.Kp = p.splits * p.cps * p.ch + (int64_t)(p.KH - 1) * p.OWq8;
  // grids are 1-D: the packs' row x block workgroups, the GEMM's tiles x slices, the reduce's threads
  const int64_t lim = 1ll << 31;
  if (p.Kp >= lim || (N * p.Hp + 1) * std::max(p.nco, p.ncb) >= lim || tiles * p.splits >= lim ||
      Co * C * p.taps / WD_T + Co + 1 >= lim)
    return false;
  p.xq_off = 3 * p.nco * p.Kp * 1024;
  p.part_off = p.xq_off + (int64_t)p.KW * p.ncb * p.Kp * 1024;
  p.bsum_off = p.part_off + round_up(p.splits * p.taps * p.nco * 64 * C * 4, 256);
  p.work_bytes = p.bsum_off + round_up(N * p.OH * Co * 4, 256);
  *out = p;
  return true;
}

// The one decision function: bnn_conv2d_bwd_filter_wide_ok, the workspace and kernel queries and the
// launch.  The last answer is kept per thread: a backward asks three times for one shape.
bool wide_filt_plan(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride,
                    int32_t pad, int32_t dil, int32_t groups, WideFiltPlan* out) {
  static thread_local struct {
    int64_t key[11];
    bool valid, ok;
    WideFiltPlan plan;
  } memo{};
  const int64_t key[11] = {N, C, H, W, Co, KH, KW, stride, pad, dil, groups};
  if (!memo.valid || !std::equal(key, key + 11, memo.key)) {
    memo.ok = wide_filt_plan_make(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &memo.plan);
    std::copy(key, key + 11, memo.key);
    memo.valid = true;
  }
  if (memo.ok) *out = memo.plan;
  return memo.ok;
}

struct WideFiltPackDy {
  float* bsum;   // null: db is not wanted
  int64_t Co, Kp, T, rows;   // rows = N Hp
  int OH, OW, Hp, OWq8, nco;
};

constexpr int FD_PITCH = 72;   // bf16 per dY tile row: 64 + 8, so a wave's 16-B reads down the channels run at 36 dwords
constexpr int FD_FP = 65;      // floats per row of the fp32 tile the row sums are taken from
constexpr int FX_PITCH = 74;   // bf16 per x tile row: 64 + KW-1 <= 72 columns at an odd dword pitch (37)

// One workgroup per (grid row, block of 64 output channels): 64 channels x up to 64 columns at a time are
// read along ow and split into [channel][ow] LDS tiles; a piece is then 16 contiguous bytes of a tile row
// and a wave stores whole KiB.  Columns OW .. OWq-1, the channel tail, rows hp >= OH and -- by the last nco
// workgroups -- the pieces T .. Kp-1 are zero-filled.  The row's channel sums: four threads per channel add
// 16 columns each in index order and combine as (s0 + s1) + (s2 + s3).
__global__ __launch_bounds__(WD_T) void conv_wide_bwd_filter_pack_dy_k(const float* __restrict__ dy,
                                                                        uint8_t* __restrict__ dq, WideFiltPackDy a) {
  __shared__ __attribute__((aligned(16))) unsigned short tile[3][64 * FD_PITCH];
  __shared__ float ftile[64 * FD_FP];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int64_t plane = (int64_t)a.nco * a.Kp * 1024;
  if (b >= a.rows * a.nco) {
    const int64_t cob = b - a.rows * a.nco, n16 = (a.Kp - a.T) * 64;
    for (int pl = 0; pl < 3; ++pl) {
      uint8_t* dst = dq + pl * plane + (cob * a.Kp + a.T) * 1024;
      for (int64_t i = tid; i < n16; i += WD_T) store_zero16(dst + i * 16);
    }
    return;
  }
  const int cob = (int)(b % a.nco);
  const int64_t row = b / a.nco, n = row / a.Hp;
  const int oh = (int)(row - n * a.Hp);
  uint8_t* dst = dq + ((int64_t)cob * a.Kp + row * a.OWq8) * 1024;   // plane 0 of this row
  if (oh >= a.OH) {
    const int n16 = a.OWq8 * 64;
    for (int i = tid; i < 3 * n16; i += WD_T) {
      const int pl = i / n16;
      store_zero16(dst + pl * plane + (int64_t)(i - pl * n16) * 16);
    }
    return;
  }
  const int64_t ohw = (int64_t)a.OH * a.OW;
  const int cn = (int)min((int64_t)64, a.Co - (int64_t)cob * 64);   // live channels of this block
  const float* yr = dy + ((n * a.Co + (int64_t)cob * 64) * a.OH + oh) * a.OW;
  float rs = 0.f;
  for (int w0 = 0; w0 < a.OW; w0 += 64) {
    const int wc = min(64, a.OW - w0), wq = (wc + 7) & ~7;
    for (int i = tid; i < 64 * wq; i += WD_T) {
      const int c = i / wq, w = i - c * wq;
      const float v = c < cn && w < wc ? yr[c * ohw + w0 + w] : 0.f;
      unsigned short d1, d2, d3;
      bf16x3_split(v, d1, d2, d3);
      tile[0][c * FD_PITCH + w] = d1;
      tile[1][c * FD_PITCH + w] = d2;
      tile[2][c * FD_PITCH + w] = d3;
      ftile[c * FD_FP + w] = v;
    }
    __syncthreads();
    const int np = wq >> 3;
    for (int i = tid; i < 3 * np * 64; i += WD_T) {
      const int ch = i & 63, q = i >> 6, pl = q / np, jp = q - pl * np;
      *reinterpret_cast<uint4*>(dst + pl * plane + (int64_t)((w0 >> 3) + jp) * 1024 + ch * 16) =
          *reinterpret_cast<const uint4*>(&tile[pl][ch * FD_PITCH + jp * 8]);
    }
    const int c = tid >> 2, q0 = (tid & 3) * 16;
    float s = 0.f;
    for (int w = q0; w < min(wc, q0 + 16); ++w) s += ftile[c * FD_FP + w];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    rs += s;
    __syncthreads();
  }
  if (a.bsum != nullptr && (tid & 3) == 0 && (tid >> 2) < cn)
    a.bsum[(n * a.OH + oh) * a.Co + (int64_t)cob * 64 + (tid >> 2)] = rs;
}

struct WideFiltPackX {
  int64_t C, H, W, Kp, T, rows;   // rows = N Hp
  int pad, Hp, OWq8, ncb, KW;
};

// One workgroup per (grid row, block of 64 input channels): the input row hp - pad is read along iw as
// ternary bf16 into a [channel][column] LDS tile that starts pad columns left of the image, and copy kw's
// piece jp is the 8 tile columns from 8 jp + kw on.  Rows outside the image and the pieces T .. Kp-1 are zeros.
__global__ __launch_bounds__(WD_T) void conv_wide_bwd_filter_pack_x_k(const float* __restrict__ x,
                                                                       uint8_t* __restrict__ xq, WideFiltPackX a) {
  __shared__ unsigned short tile[64 * FX_PITCH];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int64_t copy = (int64_t)a.ncb * a.Kp * 1024;
  if (b >= a.rows * a.ncb) {
    const int64_t cb = b - a.rows * a.ncb, n16 = (a.Kp - a.T) * 64;
    for (int kw = 0; kw < a.KW; ++kw) {
      uint8_t* dst = xq + kw * copy + (cb * a.Kp + a.T) * 1024;
      for (int64_t i = tid; i < n16; i += WD_T) store_zero16(dst + i * 16);
    }
    return;
  }
  const int cb = (int)(b % a.ncb);
  const int64_t row = b / a.ncb, n = row / a.Hp;
  const int ih = (int)(row - n * a.Hp) - a.pad;
  uint8_t* dst = xq + ((int64_t)cb * a.Kp + row * a.OWq8) * 1024;   // copy 0 of this row
  if (ih < 0 || ih >= a.H) {
    const int n16 = a.OWq8 * 64;
    for (int i = tid; i < a.KW * n16; i += WD_T) {
      const int kw = i / n16;
      store_zero16(dst + kw * copy + (int64_t)(i - kw * n16) * 16);
    }
    return;
  }
  const int64_t HW = a.H * a.W;
  const float* xr = x + ((n * a.C + (int64_t)cb * 64) * a.H + ih) * a.W;
  for (int j0 = 0; j0 < a.OWq8 * 8; j0 += 64) {
    const int jc = min(64, a.OWq8 * 8 - j0), uc = jc + a.KW - 1;
    for (int i = tid; i < 64 * uc; i += WD_T) {
      const int c = i / uc, u = i - c * uc, iw = j0 + u - a.pad;
      const int sv = iw >= 0 && iw < a.W ? tsign(xr[c * HW + iw]) : 0;
      tile[c * FX_PITCH + u] = sv > 0 ? 0x3F80 : (sv < 0 ? 0xBF80 : 0);
    }
    __syncthreads();
    const int np = jc >> 3;
    for (int i = tid; i < a.KW * np * 64; i += WD_T) {
      const int ch = i & 63, q = i >> 6, kw = q / np, jp = q - kw * np;
      const unsigned short* s = &tile[ch * FX_PITCH + jp * 8 + kw];
      *reinterpret_cast<uint4*>(dst + kw * copy + (int64_t)((j0 >> 3) + jp) * 1024 + ch * 16) =
          make_uint4(s[0] | (uint32_t)s[1] << 16, s[2] | (uint32_t)s[3] << 16, s[4] | (uint32_t)s[5] << 16,
                     s[6] | (uint32_t)s[7] << 16);
    }
    __syncthreads();
  }
}

// ternary bf16 of the FP4 code in the low nibble of n: 0x2 = +1 -> 0x3F80, 0xA = -1 -> 0xBF80, 0 -> 0
__device__ __forceinline__ uint32_t fp4_bf16(uint32_t n) { return (n & 0x2u) ? 0x3F80u | ((n & 0x8u) << 12) : 0u; }

constexpr int FXP_PITCH = 37;   // dwords (column pairs) per channel row of the planes pack's tile: odd, >= 72 / 2

// The x pack of bnn_conv2d_bwd_filter_wide_planes: the same copies from the layer's own FP4 planes
// (bnn.h, "planes", on this layer's (KH, KW, pad) grid) instead of fp32 x.  Grid row `row` of the K grid is
// row `row` of the padded grid, and copy kw at column j is the padded column j + kw: a shift along the row,
// the planes' halo supplying the zeros left and right of the image.  One workgroup per (grid row, block of 64
// input channels): per pass of 64 columns, thread (half, column pair) reads that 16-B half of its two
// positions along the padded row and writes the 32 channels' bf16 pairs down a [channel][column pair] LDS
// tile (lanes along the pairs, odd dword pitch: conflict-free); the copies leave the tile as in
// conv_wide_bwd_filter_pack_x_k.  Rows outside the image and the pieces T .. Kp-1 are zero-filled.
__global__ __launch_bounds__(WD_T) void conv_wide_bwd_filter_pack_x_planes_k(const uint8_t* __restrict__ planes,
                                                                              uint8_t* __restrict__ xq,
                                                                              WideFiltPackX a, int64_t Ppad, int Wp) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[64 * FXP_PITCH];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int64_t copy = (int64_t)a.ncb * a.Kp * 1024;
  if (b >= a.rows * a.ncb) {
    const int64_t cb = b - a.rows * a.ncb, n16 = (a.Kp - a.T) * 64;
    for (int kw = 0; kw < a.KW; ++kw) {
      uint8_t* dst = xq + kw * copy + (cb * a.Kp + a.T) * 1024;
      for (int64_t i = tid; i < n16; i += WD_T) store_zero16(dst + i * 16);
    }
    return;
  }
  const int cb = (int)(b % a.ncb);
  const int64_t row = b / a.ncb, n = row / a.Hp;
  const int ih = (int)(row - n * a.Hp) - a.pad;
  uint8_t* dst = xq + ((int64_t)cb * a.Kp + row * a.OWq8) * 1024;   // copy 0 of this row
  if (ih < 0 || ih >= a.H) {
    const int n16 = a.OWq8 * 64;
    for (int i = tid; i < a.KW * n16; i += WD_T) {
      const int kw = i / n16;
      store_zero16(dst + kw * copy + (int64_t)(i - kw * n16) * 16);
    }
    return;
  }
  const uint8_t* src = planes + ((int64_t)cb * Ppad + row * Wp) * 32;
  const unsigned short* t16 = reinterpret_cast<const unsigned short*>(tile);
  for (int j0 = 0; j0 < a.OWq8 * 8; j0 += 64) {
    const int jc = min(64, a.OWq8 * 8 - j0), uc = jc + a.KW - 1, up = (uc + 1) >> 1;
    if (tid < 2 * up) {
      const int half = tid >= up, q = tid - half * up, u = j0 + 2 * q;   // padded columns u, u + 1
      uint4 v0 = make_uint4(0u, 0u, 0u, 0u), v1 = v0;
      if (u < Wp) v0 = *reinterpret_cast<const uint4*>(src + (int64_t)u * 32 + half * 16);
      if (u + 1 < Wp) v1 = *reinterpret_cast<const uint4*>(src + (int64_t)(u + 1) * 32 + half * 16);
      const uint32_t w0[4] = {v0.x, v0.y, v0.z, v0.w}, w1[4] = {v1.x, v1.y, v1.z, v1.w};
      uint32_t* t = tile + half * 32 * FXP_PITCH + q;
#pragma unroll
      for (int c = 0; c < 32; ++c) {
        const int sh = 4 * (c & 7);
        t[c * FXP_PITCH] = fp4_bf16(w0[c >> 3] >> sh) | fp4_bf16(w1[c >> 3] >> sh) << 16;
      }
    }
    __syncthreads();
    const int np = jc >> 3;
    for (int i = tid; i < a.KW * np * 64; i += WD_T) {
      const int ch = i & 63, q = i >> 6, kw = q / np, jp = q - kw * np;
      const unsigned short* s = &t16[ch * (2 * FXP_PITCH) + jp * 8 + kw];
      *reinterpret_cast<uint4*>(dst + kw * copy + (int64_t)((j0 >> 3) + jp) * 1024 + ch * 16) =
          make_uint4(s[0] | (uint32_t)s[1] << 16, s[2] | (uint32_t)s[3] << 16, s[4] | (uint32_t)s[5] << 16,
                     s[6] | (uint32_t)s[7] << 16);
    }
    __syncthreads();
  }
}

struct WideFiltGemm {
  const uint8_t* dq;
  const uint8_t* xq;
  float* part;
  int64_t Kp, C, Co64;
  int cps, nco, ncb, ngroup, grows, KH, KW, OWq8, ch, ring, taps;
};

// 4 waves as 2 (output channels) x 2 (input channels), each one 32 x 32 MFMA tile per tap: NT accumulators.
// dY is the MFMA's first operand and x its second, so register i of a tap's accumulator is output channel
// (i & 3) + 8 (i >> 2) + 4 h of the wave's 32 and the lanes run along input channels.  LDS: NBUF x [3 planes]
// [ch pieces] of dY, then per x copy a ring of `ring` pieces; piece g of the slice (counted from the
// group's first kh row) lives in slot g % ring, and chunk i fetches only pieces hq + i ch .. hq + (i+1) ch - 1
// -- the hq halo pieces its last kh row reaches are what the next chunk starts with.
template <int NT, int NBUF>
__global__ __launch_bounds__(WD_T) void conv_wide_bwd_filter_k(WideFiltGemm a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t wide_filt_smem[];
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  int64_t b = blockIdx.x;
  const int cb = (int)(b % a.ncb);
  b /= a.ncb;
  const int cob = (int)(b % a.nco);
  b /= a.nco;
  const int grp = (int)(b % a.ngroup);
  const int64_t slice = b / a.ngroup;
  const int kh0 = grp * a.grows, rows = min(a.grows, a.KH - kh0), cnt = rows * a.KW;
  const int hq = (rows - 1) * a.OWq8;   // halo pieces of this group
  const int CH = a.ch, R = a.ring;
  const int dybytes = 3 * CH * 1024;
  uint8_t* const xring = wide_filt_smem + NBUF * dybytes;
  const int64_t P0 = slice * a.cps * CH;
  const int64_t dplane = (int64_t)a.nco * a.Kp * 1024, xcopy = (int64_t)a.ncb * a.Kp * 1024;
  const uint8_t* const dsrc = a.dq + ((int64_t)cob * a.Kp + P0) * 1024 + lane * 16;
  const uint8_t* const xsrc = a.xq + ((int64_t)cb * a.Kp + P0 + (int64_t)kh0 * a.OWq8) * 1024 + lane * 16;

  // pieces r0 .. r0 + n - 1 of every copy into the ring from slot s0 on; one glds16 of a wave is one piece
  auto issue_x = [&](int64_t r0, int n, int s0) {
    for (int kw = 0; kw < a.KW; ++kw)
      for (int j = (wave + kw) & 3; j < n; j += 4) {
        int s = s0 + j;
        if (s >= R) s -= R;
        glds16(xsrc + kw * xcopy + (r0 + j) * 1024, xring + (kw * R + s) * 1024);
      }
  };
  auto issue_dy = [&](int c, uint8_t* dst) {
    for (int pl = 0; pl < 3; ++pl)
      for (int j = (wave + pl + a.KW) & 3; j < CH; j += 4)
        glds16(dsrc + pl * dplane + ((int64_t)c * CH + j) * 1024, dst + (pl * CH + j) * 1024);
  };
  auto adv = [&](int s) {
    s += CH;
    return s >= R ? s - R : s;
  };

  int rowoff[NT], cpoff[NT];   // per tap of the group: its kh row's piece shift and its copy's ring
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int kh = t / a.KW;
    rowoff[t] = kh * a.OWq8, cpoff[t] = (t - kh * a.KW) * R * 1024;
  }

  v16f acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  const int dyl = h * 1024 + (wm * 32 + r) * 16, xl = (wn * 32 + r) * 16;
  // the fragments of k-step ks of the chunk in `db` whose first piece is in ring slot cs
  auto frags = [&](auto full, const uint8_t* db, int ks, int cs, v4i (&df)[3], v4i (&xf)[NT]) {
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) df[pl] = *reinterpret_cast<const v4i*>(db + (pl * CH + 2 * ks) * 1024 + dyl);
    int s = cs + 2 * ks;
    if (s >= R) s -= R;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (decltype(full)::value || t < cnt) {
        int s0 = s + rowoff[t];
        if (s0 >= R) s0 -= R;
        const int s1 = s0 + 1 == R ? 0 : s0 + 1;
        xf[t] = *reinterpret_cast<const v4i*>(xring + cpoff[t] + (h ? s1 : s0) * 1024 + xl);
      }
  };
  auto compute = [&](auto full, const uint8_t* db, int cs) {
    v4i df[3], xf[NT] = {}, dn[3], xn[NT] = {};
    frags(full, db, 0, cs, df, xf);
    const int nks = CH >> 1;
    for (int ks = 0; ks < nks; ++ks) {
      const bool more = ks + 1 < nks;
      if (more) frags(full, db, ks + 1, cs, dn, xn);   // the next k-step's reads under this one's MFMAs
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)   // fixed plane order: d1, d2, d3
#pragma unroll
        for (int t = 0; t < NT; ++t)
          if (decltype(full)::value || t < cnt)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, df[pl]),
                                                             __builtin_bit_cast(v8bf, xf[t]), acc[t], 0, 0, 0);
      if (more) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) df[pl] = dn[pl];
#pragma unroll
        for (int t = 0; t < NT; ++t) xf[t] = xn[t];
      }
    }
  };
  auto run = [&](const uint8_t* db, int cs) {
    if (cnt == NT) compute(std::true_type{}, db, cs);
    else compute(std::false_type{}, db, cs);   // a group of fewer taps: the rest skipped, wave-uniform
  };

  int cs = 0, fs = hq;   // ring slots of the chunk's first piece and of its first new piece
  if (hq > 0) issue_x(0, hq, 0);
  if constexpr (NBUF == 2) {
    issue_x(hq, CH, fs);
    issue_dy(0, wide_filt_smem);
    fs = adv(fs);
    for (int c = 0; c < a.cps; ++c) {
      wide_wait_dma();
      wide_barrier();   // chunk c is in LDS; every wave has left chunk c-1, whose buffer and slots are refilled next
      if (c + 1 < a.cps) {
        issue_x(hq + (int64_t)(c + 1) * CH, CH, fs);
        issue_dy(c + 1, wide_filt_smem + ((c + 1) & 1) * dybytes);
        fs = adv(fs);
      }
      run(wide_filt_smem + (c & 1) * dybytes, cs);
      cs = adv(cs);
    }
  } else {
    for (int c = 0; c < a.cps; ++c) {
      if (c > 0) wide_barrier();
      issue_x(hq + (int64_t)c * CH, CH, fs);
      issue_dy(c, wide_filt_smem);
      fs = adv(fs);
      wide_wait_dma();
      wide_barrier();
      run(wide_filt_smem, cs);
      cs = adv(cs);
    }
  }

  // fp32 partials, rows of the Co tail included (they are zeros): a register is a 128-B run along c
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t >= cnt) continue;
    float* pp = a.part + (((slice * a.taps + kh0 * a.KW + t) * a.Co64 + cob * 64 + wm * 32 + 4 * h) * a.C + cb * 64 +
                          wn * 32 + r);
#pragma unroll
    for (int i = 0; i < 16; ++i) pp[((i & 3) + 8 * (i >> 2)) * a.C] = acc[t][i];
  }
}

struct WideFiltReduce {
  const float* part;
  const float* bsum;
  float* dw;
  float* db;   // nullable
  int64_t Co, C, Co64, brows, nwblk;   // brows = N OH rows of bsum; nwblk workgroups of dw threads, then db's
  int taps, splits;
};

constexpr int FR_CH = 4;   // channels of a db workgroup: WD_T / FR_CH strands of bsum rows each

// dw: one thread per element, c fastest so that the partial reads are coalesced; the slices in index order
// in double, one rounding.  db: a workgroup per FR_CH channels, 64 strands of bsum rows (a column of bsum
// is N OH loads one after the other: few channels per workgroup keep the strands short), each in index
// order in double, then the strands in index order.  splits = 0 and brows = 0 zero-fill (the empty batch).
__global__ __launch_bounds__(WD_T) void conv_wide_bwd_filter_reduce_k(WideFiltReduce a) {
  __shared__ double red[WD_T];
  const int tid = threadIdx.x;
  if ((int64_t)blockIdx.x < a.nwblk) {
    const int64_t idx = (int64_t)blockIdx.x * WD_T + tid;
    if (idx >= a.Co * a.taps * a.C) return;
    const int64_t c = idx % a.C, q = idx / a.C, co = q / a.taps;
    const int tap = (int)(q - co * a.taps);
    const int64_t stride = (int64_t)a.taps * a.Co64 * a.C;
    const float* p = a.part + (tap * a.Co64 + co) * a.C + c;
    double s = 0.0;
    for (int sp = 0; sp < a.splits; ++sp) s += (double)p[sp * stride];
    a.dw[(co * a.C + c) * a.taps + tap] = (float)s;
    return;
  }
  const int64_t co = ((int64_t)blockIdx.x - a.nwblk) * FR_CH + (tid % FR_CH);
  double s = 0.0;
  if (co < a.Co) {
#pragma unroll 8
    for (int64_t rw = tid / FR_CH; rw < a.brows; rw += WD_T / FR_CH) s += (double)a.bsum[rw * a.Co + co];
  }
  red[tid] = s;
  __syncthreads();
  if (tid < FR_CH && co < a.Co) {
    double t = 0.0;
    for (int i = 0; i < WD_T / FR_CH; ++i) t += red[i * FR_CH + tid];
    a.db[co] = (float)t;
  }
}

int g_wide_filt_stages = 15;   // bnn_conv2d_bwd_filter_wide_set_stages

template <int NT, int NBUF>
void wide_filt_launch(const WideFiltPlan& p, const WideFiltGemm& a, hipStream_t st) {
  if (p.lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wide_bwd_filter_k<NT, NBUF>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
  const int64_t grid = (int64_t)p.nco * p.ncb * p.ngroup * p.splits;
  hipLaunchKernelGGL((conv_wide_bwd_filter_k<NT, NBUF>), dim3((unsigned)grid), dim3(WD_T), (size_t)p.lds, st, a);
}

template <int NT>
void wide_filt_launch_nt(const WideFiltPlan& p, const WideFiltGemm& a, hipStream_t st) {
  if (p.nbuf == 2) wide_filt_launch<NT, 2>(p, a, st);
  else wide_filt_launch<NT, 1>(p, a, st);
}

void wide_filt_reduce(const WideFiltPlan& p, const float* part, const float* bsum, float* dw, float* db,
                      int splits, int64_t brows, hipStream_t st) {
  const int64_t nwblk = (p.Co * p.C * p.taps + WD_T - 1) / WD_T;
  const WideFiltReduce rd{part, bsum, dw, db, p.Co, p.C, (int64_t)p.nco * 64, brows, nwblk, p.taps, splits};
  hipLaunchKernelGGL(conv_wide_bwd_filter_reduce_k, dim3((unsigned)(nwblk + (db != nullptr ? (p.Co + FR_CH - 1) / FR_CH : 0))),
                     dim3(WD_T), 0, st, rd);
}

}  // namespace
}  // namespace bnn

using namespace bnn;

BNN_API int bnn_conv2d_bwd_filter_wide_ok(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH,
                                          int64_t KW, int32_t stride, int32_t pad, int32_t dil, int32_t groups) {
  WideFiltPlan p;
  return wide_filt_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p) ? 1 : 0;
}

BNN_API int64_t bnn_conv2d_bwd_filter_wide_workspace(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co,
                                                     int64_t KH, int64_t KW, int32_t pad) {
  WideFiltPlan p;
  return wide_filt_plan(N, C, H, W, Co, KH, KW, 1, pad, 1, 1, &p) ? p.work_bytes : 0;
}

BNN_API const char* bnn_conv2d_bwd_filter_wide_kernel(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co,
                                                      int64_t KH, int64_t KW, int32_t stride, int32_t pad,
                                                      int32_t dil, int32_t groups) {
  static thread_local char buf[160];
  WideFiltPlan p;
  if (!wide_filt_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p)) return "";
  snprintf(buf, sizeof(buf), "conv_wide_bwd_filter_k<%d, %d> lds=%lld groups=%d chunk=%d splits=%lld slice=%lld pieces=%lld b128=%d",
           p.nt, p.nbuf, (long long)p.lds, p.ngroup, p.ch, (long long)p.splits, (long long)(p.cps * p.ch),
           (long long)p.T, p.cycles);
  return buf;
}

BNN_API int bnn_conv2d_bwd_filter_wide_set_stages(int32_t mask) {
  if (mask >= 0) g_wide_filt_stages = mask & 15;
  return g_wide_filt_stages;
}

// The two entries: x as fp32 NCHW (planes null) or as the layer's FP4 planes (x null) -- only the x pack differs.
static int wide_filt_run(const char* who, const float* dy, const float* x, const void* planes, float* dw, float* db,
                         int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW,
                         int32_t stride, int32_t pad, int32_t dil, int32_t groups, void* work, int64_t work_bytes,
                         void* stream) {
  WideFiltPlan p;
  if (!wide_filt_plan(N, C, H, W, Co, KH, KW, stride, pad, dil, groups, &p)) {
    set_error("%s: shape not taken (a shape of bnn_conv2d_fwd_wide with KW <= 9 whose "
              "stage -- three planes of two dY pieces and KW rings of two pieces plus (rows - 1) OWq / 8 halo "
              "pieces, 1 KiB each -- fits the LDS, and whose grids and piece count stay below 2^31)", who);
    return kErrInval;
  }
  if (!dy || (!x && !planes) || !aligned16(planes) || !dw || !work || !aligned16(work) || work_bytes < p.work_bytes) {
    set_error("%s: null pointer, planes not 16-B aligned, or a workspace not 16-B aligned or below "
              "bnn_conv2d_bwd_filter_wide_workspace = %lld bytes", who, (long long)p.work_bytes);
    return kErrInval;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint8_t* dq = static_cast<uint8_t*>(work);
  uint8_t* xq = dq + p.xq_off;
  float* part = reinterpret_cast<float*>(dq + p.part_off);
  float* bsum = reinterpret_cast<float*>(dq + p.bsum_off);
  if (N == 0) {   // the empty batch: zeros, by the reduce over no slices and no rows
    wide_filt_reduce(p, part, bsum, dw, db, 0, 0, st);
    return check_launch(who);
  }
  const int64_t rows = N * p.Hp;
  if (g_wide_filt_stages & 1) {
    const WideFiltPackDy py{db != nullptr ? bsum : nullptr, Co, p.Kp, p.T, rows, p.OH, p.OW, p.Hp, p.OWq8, p.nco};
    hipLaunchKernelGGL(conv_wide_bwd_filter_pack_dy_k, dim3((unsigned)((rows + 1) * p.nco)), dim3(WD_T), 0, st, dy,
                       dq, py);
  }
  if (g_wide_filt_stages & 2) {
    const WideFiltPackX px{C, H, W, p.Kp, p.T, rows, p.pad, p.Hp, p.OWq8, p.ncb, p.KW};
    const dim3 grid((unsigned)((rows + 1) * p.ncb));
    if (planes != nullptr)
      hipLaunchKernelGGL(conv_wide_bwd_filter_pack_x_planes_k, grid, dim3(WD_T), 0, st,
                         static_cast<const uint8_t*>(planes), xq, px,
                         bnn_conv2d_wide_planes_bytes(N, C, H, W, KH, KW, pad) / (p.ncb * 32), (int)W + 2 * pad);
    else
      hipLaunchKernelGGL(conv_wide_bwd_filter_pack_x_k, grid, dim3(WD_T), 0, st, x, xq, px);
  }
  if (g_wide_filt_stages & 4) {
    const WideFiltGemm g{dq, xq, part, p.Kp, C, (int64_t)p.nco * 64, (int)p.cps, p.nco, p.ncb, p.ngroup, p.grows,
                         p.KH, p.KW, p.OWq8, p.ch, p.ring, p.taps};
    switch (p.nt) {
      case 1: wide_filt_launch_nt<1>(p, g, st); break;
      case 3: wide_filt_launch_nt<3>(p, g, st); break;
      case 5: wide_filt_launch_nt<5>(p, g, st); break;
      default: wide_filt_launch_nt<9>(p, g, st); break;
    }
  }
  if (g_wide_filt_stages & 8) wide_filt_reduce(p, part, bsum, dw, db, (int)p.splits, N * p.OH, st);
  return check_launch(who);
}

BNN_API int bnn_conv2d_bwd_filter_wide(const float* dy, const float* x, float* dw, float* db, int64_t N, int64_t C,
                                       int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW, int32_t stride,
                                       int32_t pad, int32_t dil, int32_t groups, void* work, int64_t work_bytes,
                                       void* stream) {
  if (!x) {
    set_error("bnn_conv2d_bwd_filter_wide: null pointer");
    return kErrInval;
  }
  return wide_filt_run("bnn_conv2d_bwd_filter_wide", dy, x, nullptr, dw, db, N, C, H, W, Co, KH, KW, stride, pad, dil,
                       groups, work, work_bytes, stream);
}

BNN_API int bnn_conv2d_bwd_filter_wide_planes(const float* dy, const void* planes, float* dw, float* db, int64_t N,
                                              int64_t C, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW,
                                              int32_t stride, int32_t pad, int32_t dil, int32_t groups, void* work,
                                              int64_t work_bytes, void* stream) {
  if (!planes) {
    set_error("bnn_conv2d_bwd_filter_wide_planes: null pointer");
    return kErrInval;
  }
  return wide_filt_run("bnn_conv2d_bwd_filter_wide_planes", dy, nullptr, planes, dw, db, N, C, H, W, Co, KH, KW,
                       stride, pad, dil, groups, work, work_bytes, stream);
}
