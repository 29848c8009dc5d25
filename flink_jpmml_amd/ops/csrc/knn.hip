// NearestNeighborModel with k > 1: per-row distances to the training instances, a register top-k,
// then the PMML aggregation (majority / weighted majority vote, average / median / weighted average).
//
// Same comparison machinery as the clustering kernels (cluster.hip): metric x compareFunction x
// fieldWeight, missing inputs skipped. Two observations keep the inner loop lean:
//   * the missing-value rescale Σq/Σq_present, the final sqrt (euclidean) and the 1/p power
//     (minkowski) are monotone per row, so the top-k is selected on the raw sums and only the k
//     winners are finished;
//   * the top-k list is a fixed-size register array (KMAX in {8, 32}, runtime k <= KMAX) kept
//     sorted by (key, instance index) — a candidate that does not beat the current k-th key costs
//     one compare; a winner bubbles in with an unrolled, predicated compare-exchange chain (no
//     dynamic register indexing, so nothing spills to scratch).
//
// VALU path: instances are read with wave-uniform addresses (scalar loads, broadcast), rows are
// staged in LDS [F][256]. MFMA path (squared / plain euclidean, absDiff, distance measure, many
// instances): Σ_f w_f (x_f - c_if)² = ‖x‖²_w − 2 x·(w∘c_i) + ‖c_i‖²_w with the cross term on the
// matrix cores (v_mfma_f32_32x32x2_f32, instances on M, rows on N). Each lane then holds 16
// instance distances of one row per 32-instance tile and feeds them into its own top-k; the two
// half-waves' lists of a row are merged through lane^32 shuffles. Rows with a missing value redo
// the exact form in the same wave.
//
// Class outputs (CLASSES = true, picked when KnnArgs::probs is set): the same vote also leaves the
// winner as a class index (class_table null) and every class's vote share in probs [rows][n_class].
// The workgroup first zeroes its contiguous slice of probs with coalesced 16-byte stores; after the
// staging barriers each lane scatters the <= k non-zero shares of its row from the vote loop it runs
// anyway (a class's total is emitted at the class's first rank), and rows without neighbours are
// overwritten with NaN by the lanes of their wave together. No barrier is added, so the early
// returns stay. Nothing loops over n_class per lane.
#include "common.h"
#include "distance.h"
#include "epilogue.h"

namespace {

constexpr int TB = 256;

enum : int { AGG_MAJORITY = 0, AGG_WMAJORITY = 1, AGG_AVERAGE = 2, AGG_MEDIAN = 3, AGG_WAVERAGE = 4 };

struct KnnArgs {
  const float* X;
  int n_rows, n_feat, ldx, n_inst;
  const FieldPrep* prep;
  const float* inst;        // [N][F] training instances
  const float* weights;     // [F]
  const float* scales;      // [F] gaussSim similarity scale
  const float* qweights;    // [F] missing-value weights
  const int* cfun;          // [F] compare function codes
  const float* inst_value;  // [N] regression target of each instance
  const int* inst_class;    // [N] class index of each instance (classification)
  const float* class_table; // [C] class label parsed as double (NaN = not numeric)
  int metric, similarity;   // similarity: larger is nearer
  float p;                  // minkowski p
  int k;                    // neighbours (<= KMAX, <= n_inst)
  int agg;                  // AGG_*
  float threshold;          // weighting: 1 / (d + threshold)
  Epilogue epi;             // Target stage of a regression value (tgt flags only)
  float* score;
  uint8_t* valid;
  float* probs;             // [n_rows][n_class] vote shares (class outputs), or null
  int n_class;
};

// Class outputs: zero the workgroup's contiguous [rows x n_class] slice of probs (scalar head / tail
// around the 16-byte aligned body). The staging barriers that follow order it before the scatter.
__device__ __forceinline__ void zero_probs(const KnnArgs& a, int row0) {
  const int tid = threadIdx.x;
  float* base = a.probs + (size_t)row0 * a.n_class;
  const int total = min(TB, a.n_rows - row0) * a.n_class;  // <= 256 * 256
  const int head = min(total, (int)((16 - (reinterpret_cast<uintptr_t>(base) & 15)) & 15) >> 2);
  const int n4 = (total - head) >> 2;
  float4* body = reinterpret_cast<float4*>(base + head);
  if (tid < head) base[tid] = 0.f;
  for (int q = tid; q < n4; q += TB) body[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int tail = head + 4 * n4 + tid;
  if (tail < total) base[tail] = 0.f;
}

// Class outputs: NaN in every column of the rows in `mask` (bit b = row rbase + b), a wave-uniform
// ballot of the lanes that call this together. Those lanes (any subset of the wave: lanes past
// n_rows and the MFMA kernel's upper half-wave have returned) share each row's columns by their
// rank among themselves, so no barrier and no returned lane is needed.
__device__ __forceinline__ void nan_rows(const KnnArgs& a, unsigned long long mask, int rbase) {
  const unsigned long long active = __ballot(true);
  const int n_active = __popcll(active);
  const int rank = __popcll(active & ((1ull << (threadIdx.x & 63)) - 1));
  while (mask) {
    const int b = __ffsll(mask) - 1;
    mask &= mask - 1;
    float* p = a.probs + (size_t)(rbase + b) * a.n_class;
    for (int c = rank; c < a.n_class; c += n_active) p[c] = __builtin_nanf("");
  }
}

// Aggregate the k nearest (sorted by key) into the row's score / validity. CLASSES: also the row's
// vote shares; returns whether the row voted (its neighbours are valid).
template <int KMAX, bool CLASSES = false>
__device__ __forceinline__ bool knn_finish(const KnnArgs& a, const float (&key)[KMAX], const int (&id)[KMAX],
                                           float adj, bool ok, int row) {
  const int k = a.k;
  float d[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    // key is the raw sum (distance) or minus the raw sum (similarity)
    const float raw = a.similarity ? -key[j] : key[j];
    d[j] = finish_distance(a.metric, raw, adj, a.p);
    if (j < k) ok = ok && __builtin_isfinite(d[j]) && id[j] >= 0 && id[j] < a.n_inst;
  }
  float s = __builtin_nanf("");
  const bool voted = ok;
  if (ok) {
    if (a.agg == AGG_MAJORITY || a.agg == AGG_WMAJORITY) {
      int cls[KMAX];
      float w[KMAX];
      bool any_exact = false;
#pragma unroll
      for (int j = 0; j < KMAX; ++j) {
        cls[j] = j < k ? a.inst_class[id[j]] : -1;
        w[j] = a.agg == AGG_WMAJORITY ? 1.0f / (fabsf(d[j]) + a.threshold) : 1.0f;
        any_exact = any_exact || (j < k && !__builtin_isfinite(w[j]));
      }
      // an exact match (weight 1 / (0 + threshold 0)) dominates: the weighted vote's limit is the
      // vote of the exact neighbours alone, each counting once (models/knn.py, same rule)
#pragma unroll
      for (int j = 0; j < KMAX; ++j)
        if (any_exact) w[j] = __builtin_isfinite(w[j]) ? 0.f : 1.f;
      // votes of neighbour j's class, summed in rank order; the first rank reaching the maximum
      // names the winner (= the tied class whose best member ranks first)
      float best = -1.f;
      int best_c = -1;
      [[maybe_unused]] float total = 0.f;  // class outputs: Σ votes, in rank order
      if constexpr (CLASSES) {
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
          if (j < k) total += w[j];
      }
#pragma unroll
      for (int j = 0; j < KMAX; ++j) {
        if (j < k) {
          float v = 0.f;
          [[maybe_unused]] bool first = true;  // no better-ranked neighbour of this class
#pragma unroll
          for (int i = 0; i < KMAX; ++i) {
            if (i < k && cls[i] == cls[j]) {
              v += w[i];
              if constexpr (CLASSES) first = first && i >= j;
            }
          }
          if (v > best) {
            best = v;
            best_c = cls[j];
          }
          if constexpr (CLASSES) {  // a class's share is emitted once, at its first rank
            if (first && (unsigned)cls[j] < (unsigned)a.n_class)
              a.probs[(size_t)row * a.n_class + cls[j]] = v / total;
          }
        }
      }
      if constexpr (CLASSES)  // no table: the winner's index (the index mode of the output plans)
        s = best_c < 0 ? __builtin_nanf("") : a.class_table ? a.class_table[best_c] : (float)best_c;
      else
        s = best_c >= 0 ? a.class_table[best_c] : __builtin_nanf("");
      ok = s == s;
    } else {
      float y[KMAX];
#pragma unroll
      for (int j = 0; j < KMAX; ++j) y[j] = j < k ? a.inst_value[id[j]] : __builtin_inff();
      if (a.agg == AGG_AVERAGE) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
          if (j < k) acc += y[j];
        s = acc / (float)k;
      } else if (a.agg == AGG_WAVERAGE) {
        float num = 0.f, den = 0.f, num0 = 0.f, den0 = 0.f;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
          if (j < k) {
            const float w = 1.0f / (fabsf(d[j]) + a.threshold);
            if (__builtin_isfinite(w)) {
              num = fmaf(w, y[j], num);
              den += w;
            } else {  // exact match: see the vote above
              num0 += y[j];
              den0 += 1.f;
            }
          }
        }
        s = den0 > 0.f ? num0 / den0 : num / den;
      } else {  // median: odd-even transposition sort of the k values (+inf padding sorts last)
#pragma unroll
        for (int pass = 0; pass < KMAX; ++pass) {
#pragma unroll
          for (int j = pass & 1; j + 1 < KMAX; j += 2) {
            const float lo = fminf(y[j], y[j + 1]), hi = fmaxf(y[j], y[j + 1]);
            y[j] = lo;
            y[j + 1] = hi;
          }
        }
        // sorted ascending: the (k-1)/2-th and k/2-th values are maxima of prefixes (no dynamic index)
        float m0 = -__builtin_inff(), m1 = -__builtin_inff();
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
          m0 = j <= (k - 1) / 2 ? fmaxf(m0, y[j]) : m0;
          m1 = j <= k / 2 ? fmaxf(m1, y[j]) : m1;
        }
        s = (k & 1) ? m0 : 0.5f * (m0 + m1);
      }
      ok = __builtin_isfinite(s);
    }
  }
  if (a.agg >= AGG_AVERAGE && a.epi.tgt) {
    if (ok) s = apply_target(a.epi, s);
    if (!ok && (a.epi.tgt & TGT_DEFAULT)) {
      s = a.epi.dflt;
      ok = true;
    }
  }
  a.score[row] = ok ? s : __builtin_nanf("");
  a.valid[row] = ok ? 1 : 0;
  return voted;
}

template <int METRIC, int KMAX, bool CLASSES>
__global__ __launch_bounds__(TB) void knn_kernel(KnnArgs a) {
  extern __shared__ __align__(16) uint32_t smem[];
  float* feat = reinterpret_cast<float*>(smem);
  int* bad = reinterpret_cast<int*>(smem + a.n_feat * TB);
  const int row0 = blockIdx.x * TB;
  if constexpr (CLASSES) zero_probs(a, row0);
  stage_rows_T<TB>(a.X, a.n_rows, a.n_feat, a.ldx, a.prep, feat, bad, row0);
  const int tid = threadIdx.x;
  const int row = row0 + tid;
  if (row >= a.n_rows) return;
  const float* fr = feat + tid;
  float qpresent;
  const float adj = row_adjust(a, fr, TB, &qpresent);
  float key[KMAX];
  int id[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    key[j] = __builtin_inff();
    id[j] = 0x7fffffff;
  }
  // instances arrive in increasing index, so a tie with the k-th entry never displaces it
  float worst = __builtin_inff();
  for (int i = 0; i < a.n_inst; ++i) {
    const float s = raw_distance<METRIC>(a, fr, TB, a.inst + (size_t)i * a.n_feat);
    const float ck = a.similarity ? -s : s;
    if (ck < worst) {
      topk_insert<KMAX>(key, id, a.k, ck, i);
      worst = kth<KMAX>(key, a.k);
    }
  }
  const bool voted = knn_finish<KMAX, CLASSES>(a, key, id, adj, bad[tid] == 0 && qpresent > 0.f, row);
  if constexpr (CLASSES) nan_rows(a, __ballot(!voted), row0 + (tid & ~63));
}

typedef float f32x16_t __attribute__((ext_vector_type(16)));

// One row of the MFMA kernel: keep the expansion's top-k, or redo it exactly for a row with a
// missing value (skip missing fields, rescale by Σq / Σq_present).
template <int KMAX, bool CLASSES>
__device__ __forceinline__ bool mfma_row_finish(const KnnArgs& a, const float* feat, const int* bad,
                                                float (&key)[KMAX], int (&id)[KMAX], bool missing, int rl,
                                                int row0) {
  const int row = row0 + rl;
  if (row >= a.n_rows) return true;
  float qpresent = 1.f, adj = 1.f;
  if (missing) {
    adj = row_adjust(a, feat + rl, TB, &qpresent);
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      key[j] = __builtin_inff();
      id[j] = 0x7fffffff;
    }
    float worst = __builtin_inff();
    for (int i = 0; i < a.n_inst; ++i) {
      const float s = raw_distance<M_SQEUCLID>(a, feat + rl, TB, a.inst + (size_t)i * a.n_feat);
      if (s < worst) {
        topk_insert<KMAX>(key, id, a.k, s, i);
        worst = kth<KMAX>(key, a.k);
      }
    }
  }
  return knn_finish<KMAX, CLASSES>(a, key, id, adj, bad[rl] == 0 && qpresent > 0.f, row);
}

template <int KMAX, bool CLASSES>
__global__ __launch_bounds__(TB) void knn_mfma_kernel(KnnArgs a, const float* __restrict__ wc,
                                                      const float* __restrict__ cc, int Np, int Fp) {
  extern __shared__ __align__(16) uint32_t smem[];
  float* feat = reinterpret_cast<float*>(smem);
  int* bad = reinterpret_cast<int*>(smem + a.n_feat * TB);
  const int row0 = blockIdx.x * TB;
  if constexpr (CLASSES) zero_probs(a, row0);
  stage_rows_T<TB>(a.X, a.n_rows, a.n_feat, a.ldx, a.prep, feat, bad, row0);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int half = lane >> 5;
  const int F = a.n_feat;
  const int k = a.k;
  const int rb = wave * 64 + (lane & 31);  // this lane's two rows: rb, rb + 32
  float xx[2] = {0.f, 0.f};
  bool missing[2] = {false, false};
  for (int f = 0; f < F; ++f) {
    const float w = a.weights[f];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float x = feat[f * TB + rb + 32 * h];
      missing[h] = missing[h] || (x != x);
      xx[h] = fmaf(w * x, x, xx[h]);
    }
  }
  float key0[KMAX], key1[KMAX];
  int id0[KMAX], id1[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    key0[j] = key1[j] = __builtin_inff();
    id0[j] = id1[j] = 0x7fffffff;
  }
  float worst0 = __builtin_inff(), worst1 = __builtin_inff();
  for (int i0 = 0; i0 < Np; i0 += 32) {
    f32x16_t acc0 = {}, acc1 = {};
    const float* wrow = wc + (size_t)(i0 + (lane & 31)) * Fp;
    for (int f0 = 0; f0 < Fp; f0 += 2) {
      const int f = f0 + half;
      float x0 = f < F ? feat[f * TB + rb] : 0.f;
      float x1 = f < F ? feat[f * TB + rb + 32] : 0.f;
      x0 = (x0 != x0) ? 0.f : x0;  // rows with missing values are redone exactly below
      x1 = (x1 != x1) ? 0.f : x1;
      const float av = wrow[f];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, x0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, x1, acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {  // D[instance (r&3)+8(r>>2)+4*half][row lane&31]
      const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const float ci = cc[i];
      const float d0 = fmaxf(fmaf(-2.f, acc0[r], xx[0]) + ci, 0.f);
      const float d1 = fmaxf(fmaf(-2.f, acc1[r], xx[1]) + ci, 0.f);
      // within a lane instances arrive in increasing index: strict < keeps the lower index on ties
      if (d0 < worst0) {
        topk_insert<KMAX>(key0, id0, k, d0, i);
        worst0 = kth<KMAX>(key0, k);
      }
      if (d1 < worst1) {
        topk_insert<KMAX>(key1, id1, k, d1, i);
        worst1 = kth<KMAX>(key1, k);
      }
    }
  }
  // merge the partner half-wave's lists (same rows, the other instances of every tile)
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    const float o0 = __shfl_xor(key0[j], 32);
    const int p0 = __shfl_xor(id0[j], 32);
    const float o1 = __shfl_xor(key1[j], 32);
    const int p1 = __shfl_xor(id1[j], 32);
    if (half == 0 && j < k) {
      float w0, w1;
      int i0, i1;
      kth_pair<KMAX>(key0, id0, k, &w0, &i0);
      kth_pair<KMAX>(key1, id1, k, &w1, &i1);
      if (o0 < w0 || (o0 == w0 && p0 < i0)) topk_insert<KMAX>(key0, id0, k, o0, p0);
      if (o1 < w1 || (o1 == w1 && p1 < i1)) topk_insert<KMAX>(key1, id1, k, o1, p1);
    }
  }
  if (half != 0) return;
  const bool v0 = mfma_row_finish<KMAX, CLASSES>(a, feat, bad, key0, id0, missing[0], rb, row0);
  const bool v1 = mfma_row_finish<KMAX, CLASSES>(a, feat, bad, key1, id1, missing[1], rb + 32, row0);
  if constexpr (CLASSES) {  // the lower half-wave's bit b: rows wave * 64 + b and + 32 + b
    nan_rows(a, __ballot(!v0), row0 + wave * 64);
    nan_rows(a, __ballot(!v1), row0 + wave * 64 + 32);
  }
}

template <int KMAX, bool CLASSES>
int launch_valu(hipStream_t stream, const KnnArgs& a, dim3 grid, size_t lds) {
  switch (a.metric) {
    case M_SQEUCLID:
      hipLaunchKernelGGL((knn_kernel<M_SQEUCLID, KMAX, CLASSES>), grid, dim3(TB), lds, stream, a);
      break;
    case M_EUCLID: hipLaunchKernelGGL((knn_kernel<M_EUCLID, KMAX, CLASSES>), grid, dim3(TB), lds, stream, a); break;
    case M_CITY: hipLaunchKernelGGL((knn_kernel<M_CITY, KMAX, CLASSES>), grid, dim3(TB), lds, stream, a); break;
    case M_CHEBY: hipLaunchKernelGGL((knn_kernel<M_CHEBY, KMAX, CLASSES>), grid, dim3(TB), lds, stream, a); break;
    case M_MINKOWSKI:
      hipLaunchKernelGGL((knn_kernel<M_MINKOWSKI, KMAX, CLASSES>), grid, dim3(TB), lds, stream, a);
      break;
    default: return -6;
  }
  return 0;
}

template <int KMAX, bool CLASSES>
void launch_mfma(hipStream_t stream, const KnnArgs& a, dim3 grid, size_t lds, const float* wc, const float* cc,
                 int Np, int Fp) {
  hipLaunchKernelGGL((knn_mfma_kernel<KMAX, CLASSES>), grid, dim3(TB), lds, stream, a, wc, cc, Np, Fp);
}
}  // namespace

PMML_API int pmml_knn_args_size() { return (int)sizeof(KnnArgs); }

// wc / cc: MFMA operands (see ClusterPlan.mfma_operands: wc [Np][Fp] = w∘c zero padded, cc [Np] =
// Σ_f w_f c_f² with +inf on padded instances) or null for the VALU kernel.
PMML_API int pmml_knn_launch(hipStream_t stream, const KnnArgs* args, const float* wc, const float* cc, int Np,
                             int Fp) {
  const KnnArgs a = *args;
  if (a.n_rows <= 0) return 0;
  if (a.n_feat > 128 || a.k < 1 || a.k > 32 || a.k > a.n_inst || a.agg < 0 || a.agg > AGG_WAVERAGE) return -4;
  const bool classes = a.probs != nullptr;  // class outputs: votes only, at most 256 classes
  if (classes && (a.agg > AGG_WMAJORITY || a.n_class < 1 || a.n_class > 256)) return -4;
  if (!classes && a.agg <= AGG_WMAJORITY && !a.class_table) return -4;  // the index mode needs probs
  const size_t lds = (size_t)a.n_feat * TB * 4 + TB * 4;
  dim3 grid((a.n_rows + TB - 1) / TB);
  int rc = 0;
  if (wc) {
    if ((Np & 31) || (Fp & 1) || Fp < a.n_feat || Np < a.n_inst || a.similarity) return -4;
    if (a.metric != M_SQEUCLID && a.metric != M_EUCLID) return -6;
    if (a.k <= 8) {
      if (classes) launch_mfma<8, true>(stream, a, grid, lds, wc, cc, Np, Fp);
      else launch_mfma<8, false>(stream, a, grid, lds, wc, cc, Np, Fp);
    } else {
      if (classes) launch_mfma<32, true>(stream, a, grid, lds, wc, cc, Np, Fp);
      else launch_mfma<32, false>(stream, a, grid, lds, wc, cc, Np, Fp);
    }
  } else if (a.k <= 8) {
    rc = classes ? launch_valu<8, true>(stream, a, grid, lds) : launch_valu<8, false>(stream, a, grid, lds);
  } else {
    rc = classes ? launch_valu<32, true>(stream, a, grid, lds) : launch_valu<32, false>(stream, a, grid, lds);
  }
  if (rc) return rc;
  return hipGetLastError() == hipSuccess ? 0 : -7;
}
