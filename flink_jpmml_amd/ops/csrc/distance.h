// Distance helpers shared by the k-NN kernels (knn.hip) and the ranked-entity kernels (entities.hip):
// the per-field comparison, the raw sum of one entity, its finish, and the sorted register list.
// `Args` is the kernel's argument struct: n_feat, cfun, scales, weights, qweights and p are read.
#pragma once
#include "common.h"

namespace {

enum : int { M_SQEUCLID = 0, M_EUCLID = 1, M_CITY = 2, M_CHEBY = 3, M_MINKOWSKI = 4 };
enum : int { CF_ABSDIFF = 0, CF_GAUSS = 1, CF_DELTA = 2, CF_EQUAL = 3 };

__device__ __forceinline__ float compare(int cf, float d, float s) {
  switch (cf) {
    case CF_GAUSS: return __expf(-0.69314718056f * d * d / (s * s));
    case CF_DELTA: return d != 0.f ? 1.f : 0.f;
    case CF_EQUAL: return d == 0.f ? 1.f : 0.f;
    default: return fabsf(d);
  }
}

// Insert (ck, ci) into the sorted list key/id of length k (ties: lower instance index first).
template <int KMAX>
__device__ __forceinline__ void topk_insert(float (&key)[KMAX], int (&id)[KMAX], int k, float ck, int ci) {
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    if (j < k) {
      const bool sw = ck < key[j] || (ck == key[j] && ci < id[j]);
      const float tk = key[j];
      const int ti = id[j];
      key[j] = sw ? ck : tk;
      id[j] = sw ? ci : ti;
      ck = sw ? tk : ck;
      ci = sw ? ti : ci;
    }
  }
}

// Last (k-th) entry of the sorted list, written as a running max over the live prefix: an
// `index == k - 1` select chain is folded by LLVM into a dynamic array index (-> scratch memory).
template <int KMAX>
__device__ __forceinline__ float kth(const float (&key)[KMAX], int k) {
  float w = -__builtin_inff();
#pragma unroll
  for (int j = 0; j < KMAX; ++j) w = (j < k) ? fmaxf(w, key[j]) : w;
  return w;
}

// (key, id) of the k-th entry under the list's lexicographic order.
template <int KMAX>
__device__ __forceinline__ void kth_pair(const float (&key)[KMAX], const int (&id)[KMAX], int k, float* wk,
                                         int* wi) {
  float w = -__builtin_inff();
  int wid = -1;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    const bool later = j < k && (key[j] > w || (key[j] == w && id[j] > wid));
    w = later ? key[j] : w;
    wid = later ? id[j] : wid;
  }
  *wk = w;
  *wi = wid;
}

// Raw sum of one instance (before rescale / root); `feat` points at the row's LDS column.
template <int METRIC, class Args>
__device__ __forceinline__ float raw_distance(const Args& a, const float* feat, int stride, const float* c) {
  float s = 0.f;
  for (int f = 0; f < a.n_feat; ++f) {
    const float x = feat[f * stride];
    if (x != x) continue;
    const float v = compare(a.cfun[f], x - c[f], a.scales[f]);
    const float w = a.weights[f];
    if (METRIC == M_SQEUCLID || METRIC == M_EUCLID) s = fmaf(w * v, v, s);
    else if (METRIC == M_CITY) s = fmaf(w, v, s);
    else if (METRIC == M_CHEBY) s = fmaxf(s, w * v);
    else s = fmaf(w, __powf(v, a.p), s);
  }
  return s;
}

// Finished distance of a raw sum (the oracle's value: rescaled, rooted; similarity keeps its sign).
__device__ __forceinline__ float finish_distance(int metric, float s, float adj, float p) {
  if (metric != M_CHEBY) s *= adj;
  if (metric == M_EUCLID) s = sqrtf(fmaxf(s, 0.f));
  else if (metric == M_MINKOWSKI) s = __powf(s, 1.0f / p);
  return s;
}

template <class Args>
__device__ __forceinline__ float row_adjust(const Args& a, const float* feat, int stride, float* qpresent_out) {
  float qsum = 0.f, qpresent = 0.f;
  for (int f = 0; f < a.n_feat; ++f) {
    const float q = a.qweights[f];
    qsum += q;
    if (feat[f * stride] == feat[f * stride]) qpresent += q;
  }
  *qpresent_out = qpresent;
  return qpresent > 0.f ? qsum / qpresent : __builtin_nanf("");
}

}  // namespace
