// Shared by the wide-channel convolution units (bnn_conv_wide.hip: forward, DESIGN.md §19;
// bnn_conv_wide_bwd.hip: input gradient, §20; bnn_conv_wide_bwd_filter.hip: filter gradient, §21;
// bnn_conv_wide_infer.hip: frozen layers, §22; bnn_conv_wide_handoff.hip: training hand-off, §25): the 32-B
// LDS row with its half swizzle, the bank-model check of the fragment reads, the LDS-DMA stage copy's
// primitives, and the bf16 MFMA operand type of the two backward units.
#pragma once
#include "bnn_common.h"
#include "bnn_lds_model.h"

namespace bnn {

constexpr int WD_T = 256;                     // threads of every kernel of both units
constexpr int WD_TP = 128, WD_TC = 128;       // positions x channels of a GEMM workgroup
constexpr int64_t kWideMaxLds = 160 * 1024;   // a single workgroup may own the CU's whole LDS

typedef __bf16 v8bf __attribute__((ext_vector_type(8)));   // one lane's operand of v_mfma_f32_32x32x16_bf16

// byte offset of half h of LDS row `row` (rows of 32 B, halves swizzled by bit 3 of the row)
__host__ __device__ __forceinline__ int wide_row_off(int row, int h) { return row * 32 + 16 * (h ^ ((row >> 3) & 1)); }

// The worst fragment read of the GEMM over every tap shift, by the bank model.
inline int wide_frag_cycles(int KH, int KW, int Wp) {
  int worst = 0;
  for (int kh = 0; kh < KH; ++kh)
    for (int kw = 0; kw < KW; ++kw) {
      int addr[64];
      for (int l = 0; l < 64; ++l) addr[l] = wide_row_off(kh * Wp + kw + (l & 31), l >> 5);
      worst = std::max(worst, lds_b128_cycles(addr));
    }
  return worst;
}

__device__ __forceinline__ void store_zero16(uint8_t* p) { *reinterpret_cast<uint4*>(p) = make_uint4(0u, 0u, 0u, 0u); }

// four FP4 codes held one per byte -> 16 bits, byte j in nibble j (the planes' packs: conv_wide_pack_x_k,
// bn2d_apply_planes_k)
__device__ __forceinline__ uint32_t squeeze4(uint32_t v) {
  v = (v | (v >> 4)) & 0x00FF00FFu;
  return (v | (v >> 8)) & 0xFFFFu;
}

__device__ __forceinline__ void glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

__device__ __forceinline__ void wide_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// every LDS-DMA piece of this wave has landed (s_waitcnt vmcnt(0), the other counters left alone)
__device__ __forceinline__ void wide_wait_dma() { __builtin_amdgcn_s_waitcnt(0 | (7 << 4) | (15 << 8) | (0 << 14)); }

}  // namespace bnn
