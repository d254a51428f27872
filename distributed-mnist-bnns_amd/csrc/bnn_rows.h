// What the per-row kernels on the classifier's [M][C] output share (bnn_loss.hip: the criteria;
// bnn_metrics.hip: the evaluation metrics): the class counts they are instantiated for, the launch
// shapes with the one-workgroup bound, a row's log-sum-exp and the fixed-order workgroup sum.  One
// definition each, so a row term of the metrics is the criterion's bit for bit and both take the
// one-launch path up to the same M.
#pragma once
#include "bnn_common.h"

namespace bnn {

constexpr int CE_T = 256;              // rows per workgroup of the block + fold path
constexpr int CE_T1 = 1024;            // threads of the one-workgroup path
constexpr int64_t CE_ONE_MAX = 16384;  // ... which takes M up to this

// the class counts of bnn_cross_entropy_ok
#define BNN_CE_SWITCH(C, ...)                        \
  switch (C) {                                       \
    case 10: { constexpr int CV = 10; __VA_ARGS__; } break; \
    case 2: { constexpr int CV = 2; __VA_ARGS__; } break;   \
    case 16: { constexpr int CV = 16; __VA_ARGS__; } break; \
    case 32: { constexpr int CV = 32; __VA_ARGS__; } break; \
    case 64: { constexpr int CV = 64; __VA_ARGS__; } break; \
    default: break;                                  \
  }

// v = the row, returns max + log(sum exp(v - max)) in fp32, as torch's log_softmax
template <int C>
__device__ __forceinline__ float row_lse(const float* __restrict__ pr, float (&v)[C]) {
#pragma unroll
  for (int j = 0; j < C; ++j) v[j] = pr[j];
  float mx = v[0];
#pragma unroll
  for (int j = 1; j < C; ++j) mx = fmaxf(mx, v[j]);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < C; ++j) s += expf(v[j] - mx);
  return mx + logf(s);
}

// a workgroup's sum in thread order: a fixed shuffle tree per wave, then the waves in order (thread 0
// returns the sum)
template <int T>
__device__ __forceinline__ double block_sum_in_order(double l) {
  const int t = threadIdx.x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) l += __shfl_xor(l, o, 64);
  __shared__ double ws[T / 64];
  if ((t & 63) == 0) ws[t >> 6] = l;
  __syncthreads();
  double s = 0.0;
  if (t == 0) {
#pragma unroll
    for (int w = 0; w < T / 64; ++w) s += ws[w];
  }
  return s;
}

}  // namespace bnn
