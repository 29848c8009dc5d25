// Scorecard reason codes of a scored batch, ranked per row (gfx950 / CDNA4, wave64).
//
// One lane owns one row, as in tree.hip::tree_general_kernel, and reads the same matrix that
// kernel scored: the raw [n, F] fp32 rows plus the FieldPrep table (prep_value applied while
// staging), or the prepared tile a derive pass wrote (no prep). For every characteristic in
// document order the lane takes the first attribute whose predicate program is TRUE (the
// preds / pool encoding and three-valued logic of tree.hip::gen_eval, restated here; UNKNOWN does
// not match), forms the attribute's point difference to the baseline in float64 and adds it to its
// reason code. The codes are ranked by descending sum; ties go to the code touched first on this
// row (the oracle's stable sort over dict insertion order).
//
//   DISJOINT (no code belongs to two characteristics): every sum has one addend, so the top K
//     live in registers as an unrolled compare-insert chain, strict >, offered in characteristic
//     order. No accumulators, no scratch.
//   SHARED: per-lane float64 sums [R][rows] and first-touch numbers [R][rows] in LDS (lane-strided:
//     conflict free whatever code each lane holds), then K selection passes.
//
// Each requested column {rank, table offset, destination column} receives tables[off + code]
// (the fp32 schema.lookup encoding of the code for that Output field), NaN where valid[row] == 0
// or the row has fewer codes than the rank. Only those columns of the [n, ldo] matrix are written.
#include "common.h"

struct ReasonArgs {
  const float* X;          // [n_rows, ldx] raw rows (prep != null) or the prepared tile
  const FieldPrep* prep;   // [n_feat] or null
  const uint8_t* valid;    // [n_rows] what the score plan wrote
  const int2* chars;       // [n_char] {first attribute, attribute count}
  const int4* attrs;       // {pred offset, code index or -1, value column or -1, 0}
  const double* dval;      // per attribute: the difference d, or the baseline of a value column
  const int4* preds;       // {op | neg << 8, field or n, pool offset / count, T bits}
  const float* pool;       // SimpleSetPredicate values
  const int4* cols;        // [n_col] {rank, table offset, destination column, 0}
  const float* tables;     // [n_tables] per column: the encodings of the n_code codes
  float* out;              // [n_rows, ldo]
  int n_rows, n_feat, ldx, ldo;
  int n_char, n_code, n_col, k;
  int above, shared, feat_lds, rows;
  int n_tables, pad;
};

namespace {

enum : int { P_END = 0, P_TRUE, P_FALSE, P_GE, P_EQ, P_ISMISS, P_NOTMISS, P_SET, P_AND, P_OR, P_XOR, P_SURR };
constexpr uint32_t V_F = 0u, V_T = 1u, V_U = 2u;

constexpr int RC_MAX_K = 8;
constexpr int RC_MAX_CODES = 64;
constexpr int RC_MAX_COLS = 64;
constexpr int RC_LDS_BYTES = 64 * 1024;  // one workgroup's request: two workgroups share a CU

template <bool FEAT_LDS>
__device__ __forceinline__ float rc_feature(const ReasonArgs& a, const float* feat_lane, int TB, const float* xrow,
                                            int f) {
  if (FEAT_LDS) return feat_lane[f * TB];
  float x = xrow[f];
  if (a.prep) {
    bool b = false;
    x = prep_value(x, a.prep[f], &b);
  }
  return x;
}

// tree.hip::gen_eval: a postfix program over TRUE / FALSE / UNKNOWN, 2 bits per stack entry.
template <bool FEAT_LDS>
__device__ uint32_t rc_eval(const ReasonArgs& a, int pc, const float* feat_lane, int TB, const float* xrow) {
  uint64_t st = 0;
  for (;; ++pc) {
    const int4 in = a.preds[pc];
    const int op = in.x & 0xFF;
    const uint32_t neg = (uint32_t)(in.x >> 8) & 1u;
    uint32_t v;
    if (op == P_END) return (uint32_t)(st & 3u);
    if (op >= P_AND) {
      const int n = in.y;
      bool any_t = false, any_f = false, any_u = false;
      uint32_t par = 0u, sur = V_U;
      for (int i = 0; i < n; ++i) {
        const uint32_t e = (uint32_t)(st & 3u);
        st >>= 2;
        any_t |= e == V_T;
        any_f |= e == V_F;
        any_u |= e == V_U;
        par ^= (e == V_T) ? 1u : 0u;
        if (e != V_U) sur = e;  // popped top-down: ends at the first (bottom-most) known value
      }
      if (op == P_AND) v = any_f ? V_F : (any_u ? V_U : V_T);
      else if (op == P_OR) v = any_t ? V_T : (any_u ? V_U : V_F);
      else if (op == P_XOR) v = any_u ? V_U : par;
      else v = sur;
    } else if (op == P_TRUE) {
      v = V_T;
    } else if (op == P_FALSE) {
      v = V_F;
    } else {
      const float x = rc_feature<FEAT_LDS>(a, feat_lane, TB, xrow, in.y);
      const bool miss = x != x;
      if (op == P_ISMISS) {
        v = miss ? V_T : V_F;
      } else if (op == P_NOTMISS) {
        v = miss ? V_F : V_T;
      } else if (miss) {
        v = V_U;
      } else {
        bool r;
        if (op == P_GE) {
          r = x >= __int_as_float(in.w);
        } else if (op == P_EQ) {
          r = x == __int_as_float(in.w);
        } else {  // P_SET
          r = false;
          for (int i = 0; i < in.w; ++i) r = r || (a.pool[in.z + i] == x);
        }
        v = (r ? 1u : 0u) ^ neg;
      }
    }
    st = (st << 2) | v;
  }
}

// The K largest (difference, code) pairs offered so far, largest first. An equal difference never
// displaces an earlier offer; empty slots carry code -1. (outputs.hip::TopK over float64.)
template <int K>
struct TopCodes {
  double v[K];
  int i[K];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < K; ++j) { v[j] = 0.0; i[j] = -1; }
  }
  __device__ __forceinline__ void offer(double p, int c) {
    bool taken = false;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const bool take = taken || i[j] < 0 || p > v[j];
      const double tv = v[j];
      const int ti = i[j];
      if (take) { v[j] = p; i[j] = c; p = tv; c = ti; taken = true; }
    }
  }
  __device__ __forceinline__ int get(int r) const {
    int y = -1;
#pragma unroll
    for (int j = 0; j < K; ++j) if (j == r) y = i[j];
    return y;
  }
};

// This lane's row staged as plane f, lane-strided: feat[f * TB + lane]. 16-byte loads when the
// rows allow. Ends with a barrier.
__device__ __forceinline__ void rc_stage(const ReasonArgs& a, float* feat, int TB, int row) {
  const int r = threadIdx.x;
  const bool in = row < a.n_rows;
  const int F = a.n_feat;
  const float nan = __builtin_nanf("");
  bool b = false;
  if ((a.ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(a.X) & 15) == 0) {
    const int F4 = F >> 2;  // whole float4s inside the row; the tail goes a column at a time
    for (int fq = 0; fq < F4; ++fq) {
      float4 v = make_float4(nan, nan, nan, nan);
      if (in) v = *reinterpret_cast<const float4*>(a.X + (size_t)row * a.ldx + 4 * fq);
      const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int f = 4 * fq + e;
        float x = vv[e];
        if (in && a.prep) x = prep_value(x, a.prep[f], &b);
        feat[f * TB + r] = x;
      }
    }
    for (int f = 4 * F4; f < F; ++f) {
      float x = in ? a.X[(size_t)row * a.ldx + f] : nan;
      if (in && a.prep) x = prep_value(x, a.prep[f], &b);
      feat[f * TB + r] = x;
    }
  } else {
    for (int f = 0; f < F; ++f) {
      float x = in ? a.X[(size_t)row * a.ldx + f] : nan;
      if (in && a.prep) x = prep_value(x, a.prep[f], &b);
      feat[f * TB + r] = x;
    }
  }
  __syncthreads();
}

template <int K, bool SHARED, bool FEAT_LDS>
__global__ __launch_bounds__(256) void reasons_kernel(ReasonArgs a) {
  extern __shared__ __attribute__((aligned(16))) char rc_smem[];
  const int TB = blockDim.x;
  const int tid = threadIdx.x;
  const int row = blockIdx.x * TB + tid;
  float* feat = reinterpret_cast<float*>(rc_smem);
  const size_t feat_bytes = FEAT_LDS ? (size_t)a.n_feat * TB * 4 : 0;
  double* acc = reinterpret_cast<double*>(rc_smem + feat_bytes);  // [n_code][TB]
  int* touch = reinterpret_cast<int*>(rc_smem + feat_bytes + (size_t)a.n_code * TB * 8);  // [n_code][TB]
  if (FEAT_LDS) rc_stage(a, feat, TB, row);
  if (row >= a.n_rows) return;  // no barrier follows: a lane only reads what it staged itself

  const float* feat_lane = feat + tid;
  const float* xrow = a.X + (size_t)row * a.ldx;
  const bool ok = a.valid[row] != 0;
  TopCodes<K> top;
  top.clear();
  if (ok) {
    int n_touched = 0;
    if (SHARED) {
      for (int c = 0; c < a.n_code; ++c) { acc[c * TB + tid] = 0.0; touch[c * TB + tid] = 0; }
    }
    for (int c = 0; c < a.n_char; ++c) {
      const int2 ch = a.chars[c];
      int pick = -1;
      for (int j = 0; j < ch.y; ++j) {
        if (rc_eval<FEAT_LDS>(a, a.attrs[ch.x + j].x, feat_lane, TB, xrow) == V_T) { pick = ch.x + j; break; }
      }
      if (pick < 0) continue;
      const int4 at = a.attrs[pick];
      const int code = at.y;
      if (code < 0 || code >= a.n_code) continue;
      double d = a.dval[pick];
      if (at.z >= 0 && at.z < a.n_feat) {
        const double x = (double)rc_feature<FEAT_LDS>(a, feat_lane, TB, xrow, at.z);
        d = a.above ? x - d : d - x;
      }
      if (SHARED) {
        acc[code * TB + tid] += d;
        if (touch[code * TB + tid] == 0) touch[code * TB + tid] = ++n_touched;
      } else {
        top.offer(d, code);
      }
    }
    if (SHARED) {
      // K selection passes: the largest sum among the touched codes not yet taken, ties to the
      // smaller first-touch number
#pragma unroll
      for (int r = 0; r < K; ++r) {
        int best = -1, bt = 0;
        double bv = 0.0;
        for (int c = 0; c < a.n_code; ++c) {
          const int t = touch[c * TB + tid];
          if (t <= 0) continue;
          const double v = acc[c * TB + tid];
          if (best < 0 || v > bv || (v == bv && t < bt)) { best = c; bv = v; bt = t; }
        }
        top.i[r] = best;
        if (best >= 0) touch[best * TB + tid] = -1;
      }
    }
  }
  float* orow = a.out + (size_t)row * a.ldo;
  for (int j = 0; j < a.n_col; ++j) {
    const int4 col = a.cols[j];
    float x = __builtin_nanf("");
    const int code = (ok && col.x >= 0 && col.x < a.k) ? top.get(col.x) : -1;
    if (code >= 0) {
      const long long pos = (long long)col.y + code;
      if (col.y >= 0 && pos < a.n_tables) x = a.tables[pos];
    }
    if (col.z >= 0 && col.z < a.ldo) orow[col.z] = x;
  }
}

size_t rc_lds_bytes(int n_feat, int n_code, int rows, bool shared, bool feat_lds) {
  return (feat_lds ? (size_t)n_feat * rows * 4 : 0) + (shared ? (size_t)n_code * rows * 12 : 0);
}

template <int K>
void rc_launch(const ReasonArgs& a, dim3 grid, size_t lds, hipStream_t stream) {
  if (a.shared) {
    if (a.feat_lds) hipLaunchKernelGGL((reasons_kernel<K, true, true>), grid, dim3(a.rows), lds, stream, a);
    else hipLaunchKernelGGL((reasons_kernel<K, true, false>), grid, dim3(a.rows), lds, stream, a);
  } else {
    if (a.feat_lds) hipLaunchKernelGGL((reasons_kernel<K, false, true>), grid, dim3(a.rows), lds, stream, a);
    else hipLaunchKernelGGL((reasons_kernel<K, false, false>), grid, dim3(a.rows), lds, stream, a);
  }
}

}  // namespace

PMML_API int pmml_reasons_args_size() { return (int)sizeof(ReasonArgs); }

// LDS request of one workgroup (ops/reasons.py mirrors this); -1: not a shape the kernel takes.
PMML_API long long pmml_reasons_lds_bytes(int n_feat, int n_code, int rows, int shared, int feat_lds) {
  if (n_feat < 1 || n_code < 1 || n_code > RC_MAX_CODES || (rows != 64 && rows != 128 && rows != 256)) return -1;
  return (long long)rc_lds_bytes(n_feat, n_code, rows, shared != 0, feat_lds != 0);
}

PMML_API int pmml_reasons_launch(hipStream_t stream, const ReasonArgs* args) {
  const ReasonArgs a = *args;
  if (a.n_rows < 0 || a.n_feat < 1 || a.n_char < 0 || a.n_tables < 0) return -1;
  if (a.k < 1 || a.k > RC_MAX_K || a.n_code < 1 || a.n_code > RC_MAX_CODES || a.n_col < 1 || a.n_col > RC_MAX_COLS)
    return -1;
  if (a.rows != 64 && a.rows != 128 && a.rows != 256) return -1;
  if (a.n_rows == 0) return 0;
  if (!a.X || !a.valid || !a.chars || !a.attrs || !a.dval || !a.preds || !a.pool || !a.cols || !a.tables || !a.out)
    return -2;
  if (a.ldx < a.n_feat || a.ldo < 1) return -3;
  const size_t lds = rc_lds_bytes(a.n_feat, a.n_code, a.rows, a.shared != 0, a.feat_lds != 0);
  if (lds > (size_t)RC_LDS_BYTES) return -4;
  const dim3 grid((a.n_rows + a.rows - 1) / a.rows);
  if (a.k == 1) rc_launch<1>(a, grid, lds, stream);
  else if (a.k == 2) rc_launch<2>(a, grid, lds, stream);
  else if (a.k <= 4) rc_launch<4>(a, grid, lds, stream);
  else rc_launch<8>(a, grid, lds, stream);
  return hipGetLastError() == hipSuccess ? 0 : -7;
}
