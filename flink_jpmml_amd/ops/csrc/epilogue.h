// Fused per-row epilogue: ensemble/linear accumulators -> PMML target value (+ probabilities).
#pragma once
#include "common.h"

__device__ __forceinline__ float apply_target(const Epilogue& e, float s) {
  double v = (double)s;
  if ((e.tgt & TGT_LO) && v < e.lo) v = e.lo;  // compare form: a NaN stays NaN (no prediction)
  if ((e.tgt & TGT_HI) && v > e.hi) v = e.hi;
  v = v * e.ta + e.tb;
  switch ((e.tgt >> TGT_CAST_SHIFT) & 3) {
    case CAST_ROUND: v = floor(v + 0.5); break;
    case CAST_CEIL: v = ceil(v); break;
    case CAST_FLOOR: v = floor(v); break;
    default: break;
  }
  return (float)v;
}

// The oracle's float64 link, in its own forms (models/regression.py::link): the tie-break below
// must saturate exactly where the oracle does (1 / (1 + e^-40) == 1.0, so (40, 50) is a tie there too).
__device__ __attribute__((noinline)) double apply_link_f64(int link, double y) {
  switch (link) {
    case LINK_LOGIT: return 1.0 / (1.0 + exp(-y));
    case LINK_EXP: return exp(y);
    case LINK_PROBIT: return 0.5 * (1.0 + erf(y / 1.4142135623730951));
    case LINK_CLOGLOG: return 1.0 - exp(-exp(y));
    case LINK_LOGLOG: return exp(-exp(-y));
    case LINK_CAUCHIT: return 0.5 + atan(y) / 3.141592653589793;
    default: return y;
  }
}

// EPI_LINKMAX / EPI_CUMULATIVE, two or more classes on the largest fp32 probability `best`: classes
// that saturate to one fp32 value (logit of 20 and of 30 are both 1.0f; 0.5f - 2e-9f == 0.5f) are
// still told apart by the float64 oracle, so the tied classes are compared in float64; the first
// maximum there wins.
template <typename Acc>
__device__ __forceinline__ int tie_break_f64(const Epilogue& e, Acc acc, float best, int label) {
  const int C = e.n_classes;
  const bool cumulative = e.mode == EPI_CUMULATIVE;
  double bd = -__builtin_inf(), prevd = 0.0;
  float prev = 0.f;
  for (int c = 0; c < C; ++c) {
    const bool last = cumulative && c == C - 1;
    const float cum = last ? 1.0f : apply_link(e.link, acc(c));
    const float pv = cum - prev;
    if (cumulative) prev = cum;
    if (!cumulative && pv != best) continue;
    const double cumd = last ? 1.0 : apply_link_f64(e.link, (double)acc(c));
    const double pd = cumd - prevd;
    if (cumulative) prevd = cumd;
    if (pv == best && pd > bd) { bd = pd; label = c; }
  }
  return label;
}

// acc: C accumulator values of this row (registers or LDS, read through the accessor).
// F64_TIES: compile the float64 tie-break of EPI_LINKMAX / EPI_CUMULATIVE. Only LinearPlan lowers
// those two modes (runtime/plans.py), so only linear.hip opts in; a kernel that starts to use them
// must pass <true>. Inlined into every kernel, the float64 exp / erf / atan raised the tree kernels
// to about 120 VGPRs (hipcc -Rpass-analysis=kernel-resource-usage: tree_pointer_kernel 55 -> 119,
// tree_lds_kernel 62 -> 124, tree_reduce_kernel 34 -> 130), which is 7 -> 4 and 8 -> 3 waves per SIMD.
template <bool F64_TIES = false, typename Acc>
__device__ __forceinline__ void apply_epilogue(const Epilogue& e, Acc acc, bool row_ok, int row, int n_rows,
                                               float* __restrict__ score, uint8_t* __restrict__ valid,
                                               float* __restrict__ probs) {
  float s = __builtin_nanf("");
  bool ok = row_ok;
  int label = 0;
  if (e.mode == EPI_AFFINE) {
    s = apply_link(e.link, fmaf(e.a, acc(0), e.b));
    ok = ok && __builtin_isfinite(s);  // the oracle's regression rule: a non-finite value is no prediction
    if (e.tgt) s = apply_target(e, s);  // on the model value, after its validity (oracle order)
    if (!ok && (e.tgt & TGT_DEFAULT)) {
      s = e.dflt;
      ok = true;
    }
    if (e.write_probs && probs) probs[row] = s;
  } else if (e.mode == EPI_LOGISTIC2) {
    float p0 = apply_link(e.link, fmaf(e.a, acc(0), e.b));
    label = (p0 >= e.thr) ? 0 : 1;
    if (e.write_probs && probs) {
      probs[(size_t)row * 2 + 0] = p0;
      probs[(size_t)row * 2 + 1] = 1.0f - p0;
    }
    ok = ok && __builtin_isfinite(p0);  // the oracle: p0 and 1 - p0 finite
  } else if (e.mode == EPI_LINKMAX) {
    const int C = e.n_classes;
    float best = -__builtin_inff();
    int ties = 0;
    for (int c = 0; c < C; ++c) {
      const float pv = apply_link(e.link, acc(c));
      if (pv > best) { best = pv; label = c; ties = 1; }  // NaN never wins (the oracle's nan -> -inf)
      else if (pv == best) ++ties;
      ok = ok && __builtin_isfinite(pv);
      if (e.write_probs && probs) probs[(size_t)row * C + c] = pv;
    }
    if (F64_TIES && ties > 1) label = tie_break_f64(e, acc, best, label);
  } else if (e.mode == EPI_CUMULATIVE) {
    const int C = e.n_classes;
    float best = -__builtin_inff();
    float prev = 0.f;
    int ties = 0;
    for (int c = 0; c < C; ++c) {
      const float cum = c < C - 1 ? apply_link(e.link, acc(c)) : 1.0f;
      const float pv = cum - prev;
      prev = cum;
      if (pv > best) { best = pv; label = c; ties = 1; }
      else if (pv == best) ++ties;
      ok = ok && (pv == pv);
      if (e.write_probs && probs) probs[(size_t)row * C + c] = pv;
    }
    if (F64_TIES && ties > 1) label = tie_break_f64(e, acc, best, label);
  } else {
    const int C = e.n_classes;
    float best = -__builtin_inff();
    float mx = -__builtin_inff();
    bool fin = true;  // the oracle voids a row unless every probability is finite
    for (int c = 0; c < C; ++c) {
      const float v = acc(c);
      mx = fmaxf(mx, v);
      // softmax: a NaN or +inf logit gives inf - inf; a -inf logit is probability 0
      fin = fin && (e.mode == EPI_SOFTMAX ? v < __builtin_inff() : __builtin_isfinite(v));
    }
    float denom = 0.f;
    if (e.mode == EPI_SOFTMAX) {
      // summed in float64 and rounded once: C - 1 fp32 additions onto the 1.0 of the largest class
      // lose up to (C - 1) 2^-24 of a probability near 1 (measured 13 x 2^-24 at 16 classes)
      double d = 0.0;
      for (int c = 0; c < C; ++c) d += (double)__expf(acc(c) - mx);
      denom = (float)d;
    }
    for (int c = 0; c < C; ++c) {
      float v = acc(c);
      if (v > best) { best = v; label = c; }
      if (e.write_probs && probs) {
        float pv = (e.mode == EPI_SOFTMAX) ? __expf(v - mx) / denom : v * e.a;
        probs[(size_t)row * C + c] = pv;
      }
    }
    ok = ok && fin && (best > -__builtin_inff());
  }
  if (e.mode != EPI_AFFINE) {
    s = e.has_table ? e.table[label] : (float)label;
    ok = ok && (s == s);
  }
  const float so = ok ? s : __builtin_nanf("");
  score[row] = so;
  valid[row] = ok ? 1 : 0;
  if (e.score2) {
    e.score2[row] = so;
    e.valid2[row] = ok ? 1 : 0;
  }
}
