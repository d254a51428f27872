// The latent-update policies: what an optimizer does to an element, and all that the kernels which run one
// know of it -- the flat and multi-tensor passes (bnn_update.hip: update_span) and the packing kernels that
// fuse the update with the weight re-pack (bnn_pack.hip: sign_pack_tile_k / adam_pack_fp4_k).  The element
// math itself (adam_elem, sgd_elem, bop_elem and their Args) is in bnn_common.h.
//
// An update policy U says which element runs and which state streams it loads and stores.  The weight and
// the policy's streams share one row-major layout: prow = the weight's row, off = that row's offset in the
// streams, k = the column (a flat tensor is one row: prow = p, off = 0, k = the element).
//   U::Args                  the kernel argument (gradient, state streams, hyper-parameters)
//   U::resolve(a)            the arguments of this launch (device-step table lookups)
//   U::run4(prow, off, k, a, acc) updates the weights prow[k .. k+3] and their state in place (16-B
//                            aligned float4 runs),
//   U::run1(prow, off, k, a, acc) or one element; both return the new weight(s)
//   U::Acc                   what a thread accumulates over all of its runs (Bop: its flip count), and
//   U::finish(acc, a)        what becomes of it, called once by every thread when its last run is done;
//                            NoAcc = nothing: an empty struct and an empty call, which compile to no code
//   U::null(a), U::vec(a)    host: a needed pointer is null / every stream is 16-B aligned
// NoUpdate marks the kernels that only pack.
#pragma once

#include "bnn_common.h"

namespace bnn {

struct NoAcc {
  struct Acc {};
  template <class A>
  static __device__ __forceinline__ void finish(const Acc&, const A&) {}
};

struct NoUpdate : NoAcc {
  struct Args {};
};

// Adam + clamp (adam_elem): g, m, v read; m, v written -- 7 fp32 streams with p
struct AdamUpdate : NoAcc {
  using Args = AdamArgs;
  static __device__ __forceinline__ Args resolve(const Args& a) { return adam_resolve(a); }
  static __device__ __forceinline__ float4 run4(float* prow, int64_t off, int64_t k, const Args& a, Acc&) {
    const float4 pv = *reinterpret_cast<const float4*>(prow + k);
    const float4 gv = *reinterpret_cast<const float4*>(a.g + off + k);
    float4 mv = *reinterpret_cast<const float4*>(a.m + off + k);
    float4 vv = *reinterpret_cast<const float4*>(a.v + off + k);
    float4 np;
    np.x = adam_elem(pv.x, gv.x, mv.x, vv.x, a);
    np.y = adam_elem(pv.y, gv.y, mv.y, vv.y, a);
    np.z = adam_elem(pv.z, gv.z, mv.z, vv.z, a);
    np.w = adam_elem(pv.w, gv.w, mv.w, vv.w, a);
    *reinterpret_cast<float4*>(prow + k) = np;
    *reinterpret_cast<float4*>(a.m + off + k) = mv;
    *reinterpret_cast<float4*>(a.v + off + k) = vv;
    return np;
  }
  static __device__ __forceinline__ float run1(float* prow, int64_t off, int64_t k, const Args& a, Acc&) {
    float mm = a.m[off + k], vv = a.v[off + k];
    const float np = adam_elem(prow[k], a.g[off + k], mm, vv, a);
    prow[k] = np;
    a.m[off + k] = mm;
    a.v[off + k] = vv;
    return np;
  }
  static bool null(const Args& a) { return !a.g || !a.m || !a.v; }
  static bool vec(const Args& a) { return aligned16(a.g) && aligned16(a.m) && aligned16(a.v); }
};

// SGD + clamp (sgd_elem).  BUF = what happens to the momentum buffer: 0 none (momentum 0: g read, 3 fp32
// streams with p), 1 written only (a parameter's first step: 4 streams), 2 read and written (5 streams).
// A template parameter, not a branch on a.mu / a.first: the loads of an unrolled run stay together (the
// packing kernels).  BUF = -1 takes both from a.mu and a.first at run time: the flat and multi-tensor
// passes, where `first` differs from tensor to tensor.  wr / rd below = the buffer is written / read:
// compile-time constants for BUF 0 / 1 / 2.
template <int BUF>
struct SgdUpdate : NoAcc {
  using Args = SgdArgs;
  static __device__ __forceinline__ Args resolve(const Args& a) { return a; }
  static __device__ __forceinline__ float4 run4(float* prow, int64_t off, int64_t k, const Args& a, Acc&) {
    const float4 pv = *reinterpret_cast<const float4*>(prow + k);
    const float4 gv = *reinterpret_cast<const float4*>(a.g + off + k);
    const bool wr = BUF < 0 ? a.mu != 0.f : BUF != 0, rd = BUF < 0 ? wr && !a.first : BUF == 2;
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rd) bv = *reinterpret_cast<const float4*>(a.buf + off + k);
    float4 np;
    np.x = sgd_elem(pv.x, gv.x, bv.x, a);
    np.y = sgd_elem(pv.y, gv.y, bv.y, a);
    np.z = sgd_elem(pv.z, gv.z, bv.z, a);
    np.w = sgd_elem(pv.w, gv.w, bv.w, a);
    *reinterpret_cast<float4*>(prow + k) = np;
    if (wr) *reinterpret_cast<float4*>(a.buf + off + k) = bv;
    return np;
  }
  static __device__ __forceinline__ float run1(float* prow, int64_t off, int64_t k, const Args& a, Acc&) {
    const bool wr = BUF < 0 ? a.mu != 0.f : BUF != 0, rd = BUF < 0 ? wr && !a.first : BUF == 2;
    float bb = 0.f;
    if (rd) bb = a.buf[off + k];
    const float np = sgd_elem(prow[k], a.g[off + k], bb, a);
    prow[k] = np;
    if (wr) a.buf[off + k] = bb;
    return np;
  }
  static bool wr(const Args& a) { return BUF < 0 ? a.mu != 0.f : BUF != 0; }
  static bool null(const Args& a) { return !a.g || (wr(a) && !a.buf); }
  static bool vec(const Args& a) { return aligned16(a.g) && (!wr(a) || aligned16(a.buf)); }
};

// Bop (bop_elem): g, m read; m written -- 5 fp32 streams with w.  Acc = the thread's flip count, added to
// a.flips once per wave by finish (bop_flush).
struct BopUpdate {
  using Args = BopArgs;
  struct Acc {
    int n = 0;
  };
  static __device__ __forceinline__ Args resolve(const Args& a) { return a; }
  static __device__ __forceinline__ float4 run4(float* prow, int64_t off, int64_t k, const Args& a, Acc& acc) {
    const float4 pv = *reinterpret_cast<const float4*>(prow + k);
    const float4 gv = *reinterpret_cast<const float4*>(a.g + off + k);
    float4 mv = *reinterpret_cast<const float4*>(a.m + off + k);
    float4 np;
    np.x = bop_elem(pv.x, gv.x, mv.x, a, acc.n);
    np.y = bop_elem(pv.y, gv.y, mv.y, a, acc.n);
    np.z = bop_elem(pv.z, gv.z, mv.z, a, acc.n);
    np.w = bop_elem(pv.w, gv.w, mv.w, a, acc.n);
    *reinterpret_cast<float4*>(prow + k) = np;
    *reinterpret_cast<float4*>(a.m + off + k) = mv;
    return np;
  }
  static __device__ __forceinline__ float run1(float* prow, int64_t off, int64_t k, const Args& a, Acc& acc) {
    float mm = a.m[off + k];
    const float np = bop_elem(prow[k], a.g[off + k], mm, a, acc.n);
    prow[k] = np;
    a.m[off + k] = mm;
    return np;
  }
  static __device__ __forceinline__ void finish(const Acc& acc, const Args& a) { bop_flush(acc.n, a.flips); }
  static bool null(const Args& a) { return !a.g || !a.m; }
  static bool vec(const Args& a) { return aligned16(a.g) && aligned16(a.m); }
};

}  // namespace bnn
