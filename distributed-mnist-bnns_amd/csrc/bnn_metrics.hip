// Evaluation metrics of a classifier's output (utils.py:142-155 accuracy(output, target, topk), and the
// criterion of a test loop): for z [M][C] fp32 (logits or log-probabilities) and int64 labels y, one call
// adds into device accumulators
//
//   loss_sum[0]            += sum over the counted rows of lse(z_i) - z_i[y_i]
//   counts[0]              += the counted rows (y_i != ignore_index)
//   counts[1], counts[2]   += those with rank 0 / rank < k
//   counts[3 + y C + pred] += 1 per counted row with y in [0, C)       (the confusion matrix)
//
// and writes pred[i], the top-ranked column, for every row.  Order of values: a ranks above b when
// a > b, a NaN above every non-NaN; equal values (and two NaNs) by the lower column first.  rank = the
// number of columns that rank above column y_i.
//
// One thread per row, the row in registers.  The row term is bnn_loss.hip's: row_lse<C> then one fp32
// subtraction, a label outside [0, C) making it NaN.  The terms are summed in double in an order that
// depends on M only -- 256-row blocks in row order folded in block order by a one-workgroup kernel, or,
// up to CE_ONE_MAX rows, one 1024-thread workgroup doing both (the launch plan of bnn_cross_entropy_fwd)
// -- and one thread adds the call's sum to loss_sum[0]: no floating-point atomics anywhere.  The counts
// are integers, exact in any order: each workgroup counts in LDS (wave-reduced totals, an LDS histogram
// of the C x C cells) and adds its non-zero cells to the accumulators, with vector atomics where several
// workgroups run.
#include "bnn_rows.h"
#include "bnn.h"

namespace bnn {
namespace {

__device__ __forceinline__ bool above(float a, float b) { return a > b || (a != a && b == b); }

struct RowEval {
  float term;   // lse - z[y] (NaN for a label outside [0, C))
  int pred;     // the top-ranked column
  int counted;  // y != ignore_index
  int top1;     // counted, label in range, rank 0
  int topk;     // counted, label in range, rank < k
  int cell;     // y C + pred, or -1 (ignored row / label out of range)
};

template <int C>
__device__ __forceinline__ RowEval row_eval(const float* __restrict__ z, const int64_t* __restrict__ y, int64_t i,
                                            int k, int64_t ignore) {
  float v[C];
  const float ls = row_lse<C>(z + i * C, v);
  const int64_t yi = y[i];
  RowEval r;
  float bv = v[0];
  r.pred = 0;
#pragma unroll
  for (int j = 1; j < C; ++j) {
    const bool up = above(v[j], bv);
    bv = up ? v[j] : bv;
    r.pred = up ? j : r.pred;
  }
  float vy = __builtin_nanf("");   // a label outside [0, C) makes the term NaN
#pragma unroll
  for (int j = 0; j < C; ++j) vy = (j == yi) ? v[j] : vy;
  r.term = ls - vy;
  const bool in_range = yi >= 0 && yi < C;
  int rank = 0;
#pragma unroll
  for (int j = 0; j < C; ++j) rank += (j < yi ? !above(vy, v[j]) : above(v[j], vy)) ? 1 : 0;
  r.counted = yi != ignore;
  const bool hit = r.counted && in_range;
  r.top1 = hit && rank == 0;
  r.topk = hit && rank < k;
  r.cell = hit ? (int)yi * C + r.pred : -1;
  return r;
}

// a workgroup's counting state in LDS: [0..2] rows / top-1 / top-k, [3 ..] the C x C cells
template <int C>
__device__ __forceinline__ void counts_clear(unsigned* __restrict__ h, int T) {
  for (int c = threadIdx.x; c < 3 + C * C; c += T) h[c] = 0u;
  __syncthreads();
}

// the totals wave-reduced first (one LDS add per wave and total), the cells added per row
__device__ __forceinline__ void counts_add(unsigned* __restrict__ h, int n, int h1, int hk) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    n += __shfl_xor(n, o, 64);
    h1 += __shfl_xor(h1, o, 64);
    hk += __shfl_xor(hk, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (n) atomicAdd(&h[0], (unsigned)n);
    if (h1) atomicAdd(&h[1], (unsigned)h1);
    if (hk) atomicAdd(&h[2], (unsigned)hk);
  }
}

// SOLE: the only workgroup of the launch adds with plain read-modify-writes (calls on one stream are ordered)
template <int C, bool SOLE>
__device__ __forceinline__ void counts_flush(const unsigned* __restrict__ h, int64_t* __restrict__ counts, int T) {
  __syncthreads();
  for (int c = threadIdx.x; c < 3 + C * C; c += T) {
    const unsigned a = h[c];
    if (a == 0u) continue;
    if constexpr (SOLE) counts[c] += (int64_t)a;
    else atomicAdd(reinterpret_cast<unsigned long long*>(counts + c), (unsigned long long)a);
  }
}

template <int C>
__global__ __launch_bounds__(CE_T) void metrics_k(const float* __restrict__ z, const int64_t* __restrict__ y, int64_t M,
                                                 int k, int64_t ignore, int64_t* __restrict__ counts,
                                                 int32_t* __restrict__ pred, double* __restrict__ part) {
  __shared__ unsigned h[3 + C * C];
  counts_clear<C>(h, CE_T);
  const int64_t i = (int64_t)blockIdx.x * CE_T + threadIdx.x;
  double l = 0.0;
  int n = 0, h1 = 0, hk = 0;
  if (i < M) {
    const RowEval r = row_eval<C>(z, y, i, k, ignore);
    if (pred) pred[i] = r.pred;
    if (r.counted) l = (double)r.term;
    n = r.counted;
    h1 = r.top1;
    hk = r.topk;
    if (r.cell >= 0) atomicAdd(&h[3 + r.cell], 1u);
  }
  counts_add(h, n, h1, hk);
  counts_flush<C, false>(h, counts, CE_T);
  const double s = block_sum_in_order<CE_T>(l);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(CE_T) void metrics_fold_k(const double* __restrict__ part, int64_t nb,
                                                      double* __restrict__ loss_sum) {
  // one workgroup: thread t sums blocks t, t + 256, ... in order, then the fixed tree over threads
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += CE_T) s += part[b];
  s = block_sum_in_order<CE_T>(s);
  if (threadIdx.x == 0) loss_sum[0] += s;
}

// M <= CE_ONE_MAX: ONE workgroup of 1024 threads, thread t taking rows t, t + 1024, ... in order
template <int C>
__global__ __launch_bounds__(CE_T1) void metrics1_k(const float* __restrict__ z, const int64_t* __restrict__ y,
                                                   int64_t M, int k, int64_t ignore, double* __restrict__ loss_sum,
                                                   int64_t* __restrict__ counts, int32_t* __restrict__ pred) {
  __shared__ unsigned h[3 + C * C];
  counts_clear<C>(h, CE_T1);
  const int t = threadIdx.x;
  double l = 0.0;
  int n = 0, h1 = 0, hk = 0;
  // U rows per trip, read unconditionally (clamped) so their loads are all in flight together; used in
  // the same row order as one at a time
  constexpr int U = C <= 16 ? 4 : 1;
  for (int64_t i0 = t; i0 < M; i0 += U * CE_T1) {
    RowEval r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) r[u] = row_eval<C>(z, y, min(i0 + (int64_t)u * CE_T1, M - 1), k, ignore);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + (int64_t)u * CE_T1;
      if (i >= M) break;
      if (pred) pred[i] = r[u].pred;
      if (r[u].counted) l += (double)r[u].term;
      n += r[u].counted;
      h1 += r[u].top1;
      hk += r[u].topk;
      if (r[u].cell >= 0) atomicAdd(&h[3 + r[u].cell], 1u);
    }
  }
  counts_add(h, n, h1, hk);
  counts_flush<C, true>(h, counts, CE_T1);
  const double s = block_sum_in_order<CE_T1>(l);
  if (t == 0) loss_sum[0] += s;
}

}  // namespace
}  // namespace bnn

using namespace bnn;

BNN_API int bnn_eval_metrics_ok(int64_t C) { return bnn_cross_entropy_ok(C); }

// workspace: one double per 256-row block (the block + fold path's partial sums)
BNN_API int64_t bnn_eval_metrics_workspace(int64_t M) {
  if (M <= 0) return 0;
  return ((M + CE_T - 1) / CE_T) * (int64_t)sizeof(double);
}

BNN_API int bnn_eval_metrics(const float* z, const int64_t* y, int64_t M, int64_t C, int32_t k, int64_t ignore_index,
                             double* loss_sum, int64_t* counts, int32_t* pred, void* work, int64_t work_bytes,
                             void* stream) {
  if (M == 0) return 0;
  if (M < 0 || !z || !y || !loss_sum || !counts || !work || !bnn_eval_metrics_ok(C) || k < 1 || k > C ||
      work_bytes < bnn_eval_metrics_workspace(M)) {
    set_error("bnn_eval_metrics: bad arguments (M=%lld C=%lld k=%d work=%lld; M >= 0, non-null z / y / loss_sum / "
              "counts / work, C in {2,10,16,32,64}, 1 <= k <= C, workspace bnn_eval_metrics_workspace(M))",
              (long long)M, (long long)C, (int)k, (long long)work_bytes);
    return kErrInval;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (M <= CE_ONE_MAX) {
    BNN_CE_SWITCH((int)C, hipLaunchKernelGGL((metrics1_k<CV>), dim3(1), dim3(CE_T1), 0, s, z, y, M, (int)k, ignore_index,
                                              loss_sum, counts, pred));
    return check_launch("bnn_eval_metrics");
  }
  double* part = reinterpret_cast<double*>(work);
  const int64_t nb = (M + CE_T - 1) / CE_T;
  BNN_CE_SWITCH((int)C, hipLaunchKernelGGL((metrics_k<CV>), dim3((unsigned)nb), dim3(CE_T), 0, s, z, y, M, (int)k,
                                            ignore_index, counts, pred, part));
  hipLaunchKernelGGL(metrics_fold_k, dim3(1), dim3(CE_T), 0, s, part, nb, loss_sum);
  return check_launch("bnn_eval_metrics");
}
