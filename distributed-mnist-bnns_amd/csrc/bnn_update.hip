// Subsystem (3) helpers: Hardtanh STE mask and the fused latent-weight update.
//
// The reference's caller protocol (mnist-dist2.py:131-137) is
//     p.data.copy_(p.org); optimizer.step(); p.org.copy_(p.data.clamp_(-1,1))
// around torch.optim.Adam (mnist-dist2.py:91).  bnn_adam_clamp applies Adam to the latent
// weight and clamps it in one HBM pass (7 fp32 streams: p, g, m, v read; p, m, v written).
//
// Every flat and multi-tensor pass here -- Adam, SGD, Bop -- is the one span below driven by an update
// policy (bnn_update.h), the same policies the packing kernels of bnn_pack.hip fuse with the re-pack.
#include <algorithm>
#include <cmath>

#include "bnn_common.h"
#include "bnn_update.h"

namespace bnn {
namespace {

__global__ __launch_bounds__(256) void hardtanh_bwd_k(const float* __restrict__ x,
                                                      const float* __restrict__ g,
                                                      float* __restrict__ out, int64_t n, int vec) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  auto f = [](float xv, float gv) { return (xv > -1.f && xv < 1.f) ? gv : 0.f; };
  int64_t tail = 0;
  if (vec) {
    const int64_t n4 = n / 4;
    for (int64_t i = i0; i < n4; i += stride) {
      const float4 xv = reinterpret_cast<const float4*>(x)[i];
      const float4 gv = reinterpret_cast<const float4*>(g)[i];
      reinterpret_cast<float4*>(out)[i] =
          make_float4(f(xv.x, gv.x), f(xv.y, gv.y), f(xv.z, gv.z), f(xv.w, gv.w));
    }
    tail = n4 * 4;
  }
  for (int64_t i = tail + i0; i < n; i += stride) out[i] = f(x[i], g[i]);
}

// Threads per block of every update launch.  A constant, not blockDim.x: with blockDim.x in the span every
// instance compiled to the remainder-workgroup form of the block size (a dependent global_load_ushort at each
// wave's start), as the parent's sgd_span kernels did and its kernels that read blockDim.x themselves did not.
constexpr int UPD_THREADS = 256;

// One tensor's grid-stride pass of update policy U over p[0 .. n) and the policy's streams (a flat tensor is
// one row of the policies' layout).  vec: p and every stream 16-B aligned -> float4 runs and a scalar tail,
// else scalar throughout.  Both go through the same element, so the result does not depend on vec.
template <class U>
__device__ __forceinline__ void update_span(float* __restrict__ p, int64_t n, const typename U::Args& a, int vec,
                                            typename U::Acc& acc) {
  const int64_t stride = (int64_t)gridDim.x * UPD_THREADS;
  const int64_t i0 = (int64_t)blockIdx.x * UPD_THREADS + threadIdx.x;
  int64_t tail = 0;
  if (vec) {
    const int64_t n4 = n / 4;
    for (int64_t i = i0; i < n4; i += stride) U::run4(p, 0, 4 * i, a, acc);
    tail = n4 * 4;
  }
  for (int64_t i = tail + i0; i < n; i += stride) U::run1(p, 0, i, a, acc);
}

template <class U>
__global__ __launch_bounds__(UPD_THREADS) void update_flat_k(float* __restrict__ p, int64_t n, typename U::Args a0, int vec) {
  const typename U::Args a = U::resolve(a0);
  typename U::Acc acc{};
  update_span<U>(p, n, a, vec, acc);
  U::finish(acc, a);
}

// Multi-tensor form: up to ADAM_MT tensors (the small parameters -- biases, BatchNorm affine
// parameters, the head -- each of which would otherwise be its own launch of a few microseconds)
// in ONE launch, blockIdx.y = tensor, each with its own arguments (Adam: its bias corrections or the
// device-step table; SGD: its first and clamp flags).
constexpr int ADAM_MT = 16;
template <class U>
struct UpdateMulti {
  float* p[ADAM_MT];
  int64_t n[ADAM_MT];
  typename U::Args a[ADAM_MT];
  int vec[ADAM_MT];
};
static_assert(sizeof(UpdateMulti<AdamUpdate>) <= 4096 && sizeof(UpdateMulti<SgdUpdate<-1>>) <= 4096,
              "a kernel takes at most 4 KB of arguments");

template <class U>
__global__ __launch_bounds__(UPD_THREADS) void update_multi_k(UpdateMulti<U> um) {
  const int j = blockIdx.y;
  const typename U::Args a = U::resolve(um.a[j]);
  typename U::Acc acc{};
  update_span<U>(um.p[j], um.n[j], a, um.vec[j], acc);
  U::finish(acc, a);
}

}  // namespace

// torch computes the bias corrections as Python floats (double) from the step count.
void adam_bias_correction(float lr, float beta1, float beta2, int64_t step, float* step_size, float* bc2_sqrt) {
  const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
  const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
  *step_size = (float)((double)lr / bc1);
  *bc2_sqrt = (float)std::sqrt(bc2);
}

namespace {

inline int grid_for(int64_t n) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192));
}

// A flat pass's pointers and length are good: an empty tensor is nothing to do, whatever its pointers.
template <class U>
bool update_flat_ok(const float* p, int64_t n, const typename U::Args& a) {
  return n >= 0 && (n == 0 || (p && !U::null(a)));
}

// The flat pass of policy U: one argument contract and one launch for every flat entry.  ok = the entry's
// own hyper-parameter check.
template <class U>
int update_flat_impl(const char* name, float* p, int64_t n, const typename U::Args& a, bool ok, void* stream) {
  if (!ok || !update_flat_ok<U>(p, n, a)) {
    set_error("%s: bad arguments", name);
    return kErrInval;
  }
  if (n == 0) return 0;
  const int vec = aligned16(p) && U::vec(a);
  hipLaunchKernelGGL(update_flat_k<U>, dim3(grid_for(vec ? (n + 3) / 4 : n)), dim3(UPD_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), p, n, a, vec);
  return check_launch(name);
}

// The multi-tensor pass of policy U.  ok = the entry's check of its own arrays and hyper-parameters;
// args_of(j, a) fills tensor j's arguments, false: they are bad.  Empty tensors are left out of the launch.
template <class U, class ArgsOf>
int update_multi_impl(const char* name, int32_t count, float* const* p, const int64_t* n, bool ok, ArgsOf args_of,
                      void* stream) {
  if (!ok || count < 0 || count > ADAM_MT || (count > 0 && (!p || !n))) {
    set_error("%s: bad arguments (count %d, at most %d tensors per launch)", name, count, ADAM_MT);
    return kErrInval;
  }
  UpdateMulti<U> um{};
  int64_t work = 0;      // the most threads a tensor can use
  int k = 0;
  for (int j = 0; j < count; ++j) {
    typename U::Args a{};
    if (n[j] < 0 || !args_of(j, a) || (n[j] > 0 && (!p[j] || U::null(a)))) {
      set_error("%s: bad tensor %d", name, j);
      return kErrInval;
    }
    if (n[j] == 0) continue;
    um.p[k] = p[j], um.n[k] = n[j], um.a[k] = a, um.vec[k] = aligned16(p[j]) && U::vec(a);
    work = std::max(work, um.vec[k] ? (n[j] + 3) / 4 : n[j]);
    ++k;
  }
  if (k == 0) return 0;
  const unsigned gx = (unsigned)std::min<int64_t>((work + UPD_THREADS - 1) / UPD_THREADS, 1024);
  hipLaunchKernelGGL(update_multi_k<U>, dim3(gx, (unsigned)k), dim3(UPD_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     um);
  return check_launch(name);
}

}  // namespace
}  // namespace bnn

using namespace bnn;

BNN_API int bnn_hardtanh_bwd(const float* x, const float* g, float* out, int64_t n, void* stream) {
  if (!x || !g || !out || n < 0) {
    set_error("bnn_hardtanh_bwd: bad arguments");
    return kErrInval;
  }
  if (n == 0) return 0;
  const int vec = aligned16(x) && aligned16(g) && aligned16(out);
  hipLaunchKernelGGL(hardtanh_bwd_k, dim3(grid_for(n / 4)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, g, out, n, vec);
  return check_launch("bnn_hardtanh_bwd");
}

// Adam + clamp (math: adam_elem in bnn_common.h), per-launch bias corrections or the device-step table.
BNN_API int bnn_adam_clamp(float* p, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                           float lr, float beta1, float beta2, float eps, int64_t step,
                           float grad_scale, int32_t clamp, void* stream) {
  AdamArgs a{grad, exp_avg, exp_avg_sq, beta1, beta2, eps, 0.f, 1.f, grad_scale, clamp};
  if (step >= 1) adam_bias_correction(lr, beta1, beta2, step, &a.step_size, &a.bc2_sqrt);
  return update_flat_impl<AdamUpdate>("bnn_adam_clamp", p, n, a, step >= 1, stream);
}

BNN_API int bnn_adam_clamp_sched(float* p, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                 float beta1, float beta2, float eps, const float* sched, const int64_t* ctr,
                                 float grad_scale, int32_t clamp, void* stream) {
  AdamArgs a{grad, exp_avg, exp_avg_sq, beta1, beta2, eps, 0.f, 1.f, grad_scale, clamp};
  a.sched = sched;
  a.ctr = ctr;
  return update_flat_impl<AdamUpdate>("bnn_adam_clamp_sched", p, n, a, sched && ctr, stream);
}

BNN_API int bnn_adam_clamp_multi(int32_t count, float* const* p, const float* const* grad, float* const* exp_avg,
                                 float* const* exp_avg_sq, const int64_t* n, const int64_t* step,
                                 const int32_t* clamp, float lr, float beta1, float beta2, float eps,
                                 const float* sched, const int64_t* ctr, float grad_scale, void* stream) {
  const bool ok = (count <= 0 || (grad && exp_avg && exp_avg_sq && step && clamp)) && ((sched == nullptr) == (ctr == nullptr));
  return update_multi_impl<AdamUpdate>("bnn_adam_clamp_multi", count, p, n, ok, [&](int j, AdamArgs& a) {
    if (!sched && step[j] < 1) return false;
    a = AdamArgs{grad[j], exp_avg[j], exp_avg_sq[j], beta1, beta2, eps, 0.f, 1.f, grad_scale, clamp[j]};
    a.sched = sched;       // the device-step table, else this tensor's own bias corrections
    a.ctr = ctr;
    if (!sched) adam_bias_correction(lr, beta1, beta2, step[j], &a.step_size, &a.bc2_sqrt);
    return true;
  }, stream);
}

// torch.optim.SGD + clamp (math: sgd_elem in bnn_common.h): 5 fp32 streams (p, g, buf read; p, buf
// written), 2 + 1 without momentum.  Nothing depends on the step count, so a captured step replays
// these launches as they are.  SgdUpdate<-1>: the buffer is read / written as a.mu and a.first say.
BNN_API int bnn_sgd_clamp(float* p, const float* grad, float* buf, int64_t n, float lr, float momentum, float omd,
                          float weight_decay, int32_t nesterov, int32_t first, float grad_scale, int32_t clamp,
                          void* stream) {
  const SgdArgs a{grad, buf, lr, momentum, omd, weight_decay, grad_scale, nesterov != 0, first != 0, clamp};
  const bool ok = (momentum == 0.f || buf) && sgd_hyper_ok(lr, momentum, omd, weight_decay, nesterov);
  return update_flat_impl<SgdUpdate<-1>>("bnn_sgd_clamp", p, n, a, ok, stream);
}

BNN_API int bnn_sgd_clamp_multi(int32_t count, float* const* p, const float* const* grad, float* const* buf,
                                const int64_t* n, const int32_t* first, const int32_t* clamp, float lr,
                                float momentum, float omd, float weight_decay, int32_t nesterov, float grad_scale,
                                void* stream) {
  const bool ok = (count <= 0 || (grad && first && clamp && (momentum == 0.f || buf))) &&
                  sgd_hyper_ok(lr, momentum, omd, weight_decay, nesterov);
  return update_multi_impl<SgdUpdate<-1>>("bnn_sgd_clamp_multi", count, p, n, ok, [&](int j, SgdArgs& a) {
    a = SgdArgs{grad[j], momentum != 0.f ? buf[j] : nullptr, lr, momentum, omd, weight_decay, grad_scale,
                nesterov != 0, first[j] != 0, clamp[j]};
    return true;
  }, stream);
}

// Bop (math: bop_elem in bnn_common.h): 5 fp32 streams (w, g, m read; w, m written).
BNN_API int bnn_bop(float* w, const float* grad, float* m, int64_t n, float gamma, float threshold, float grad_scale,
                    int64_t* flips, void* stream) {
  const BopArgs a{grad, m, gamma, threshold, grad_scale, flips};
  if (!bop_hyper_ok(gamma, threshold) || !update_flat_ok<BopUpdate>(w, n, a)) {    // its own, fuller text
    set_error("bnn_bop: bad arguments (n=%lld gamma=%g threshold=%g)", (long long)n, (double)gamma, (double)threshold);
    return kErrInval;
  }
  return update_flat_impl<BopUpdate>("bnn_bop", w, n, a, true, stream);
}

BNN_API int bnn_adam_schedule(float lr, float beta1, float beta2, int64_t step0, int64_t n, float* out) {
  if (!out || n < 0 || step0 < 1) {
    set_error("bnn_adam_schedule: bad arguments");
    return kErrInval;
  }
  for (int64_t i = 0; i < n; ++i) adam_bias_correction(lr, beta1, beta2, step0 + i, &out[2 * i], &out[2 * i + 1]);
  return 0;
}

namespace bnn {
namespace {
__global__ void counter_add_k(int64_t* ctr, int64_t v) {
  if (threadIdx.x == 0) ctr[0] += v;
}
}  // namespace
}  // namespace bnn

BNN_API int bnn_counter_add(int64_t* ctr, int64_t v, void* stream) {
  if (!ctr) {
    set_error("bnn_counter_add: null counter");
    return kErrInval;
  }
  hipLaunchKernelGGL(counter_add_k, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), ctr, v);
  return check_launch("bnn_counter_add");
}
