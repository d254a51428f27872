// Shared by the first-layer (real-input) convolution units (bnn_conv_first.hip: forward and filter gradient,
// DESIGN.md §23; bnn_conv_first_infer.hip: the frozen forward, §24): the shape limits, the ternary bf16 weight
// and the weight rows' LDS pitch with its bank-model check.
#pragma once
#include "bnn_conv_wide.h"

namespace bnn {

constexpr int kFirstMaxC = 4, kFirstMaxKt = 80;

// the weight fragment read of the forward through the bank model: lane (r, h) reads 16 B of row r at k = 8 h
inline int first_wfrag_cycles(int wp) {
  int addr[64];
  for (int l = 0; l < 64; ++l) addr[l] = ((l & 31) * wp + 8 * (l >> 5)) * 2;
  return lds_b128_cycles(addr);
}

// bf16 per weight row in LDS: Kp + 8 j, the j <= 4 of the fewest modelled cycles (4 = conflict-free)
inline void first_weight_pitch(int kp, int* wp, int* cycles) {
  *cycles = 1 << 30;
  for (int j = 1; j <= 4; ++j) {
    const int c = first_wfrag_cycles(kp + 8 * j);
    if (c < *cycles) *cycles = c, *wp = kp + 8 * j;
  }
}

__device__ __forceinline__ unsigned short tsign_bf16(float v) {
  const int s = tsign(v);
  return s > 0 ? 0x3F80 : (s < 0 ? 0xBF80 : 0);
}

}  // namespace bnn
