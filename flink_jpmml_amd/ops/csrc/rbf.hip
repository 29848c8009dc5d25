// Radial-basis-function NeuralNetwork (a radialBasis hidden layer + one dense output layer), fused
// in one pass per row tile on the exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32):
//
//   x    = input stage (gather by in_index, scale / shift, missing replacement)        n_in <= 128
//   d_j  = |x - w_j|^2 = |x|^2 - 2 G_j + |w_j|^2,   G = Wc . x^T   (product 1: units on M, rows on N)
//   a_j  = exp(c_j - g_j d_j)          c_j = fanIn ln(altitude_j),  g_j = 1 / (2 width_j^2)
//   a~   = a | exp(a - A_max) / sum | a / sum           (the hidden layer's normalizationMethod)
//   o_k  = act(sum_j v_kj a~_j + b_k)                    (product 2: outputs on M, rows on N)
//   then the network decode of mlp.hip: softmax / simplemax + label table, or affine + Target.
//
// Work split: a 256-thread workgroup owns 256 rows, each wave 64 rows as two 32-row N tiles that
// share every A-operand read (cluster_mfma_kernel's split). The row tile's B fragments stay in
// VGPRs for the whole kernel. Per 32-unit hidden tile the host packs one *panel*: the centre
// fragments, the tile's c / g / |w|^2 and its 32 x 32 slice of the output weights, all in the order
// the lanes consume them, so a lane reads 16 bytes per ds_read. Panels stream through a two-slot
// LDS ring shared by the four waves: panel t + 1 is fetched into registers before tile t's MFMAs
// and stored after them, one barrier per tile.
//
// k order of product 1: k-step s = 4 q + e of lane half h carries input 8 q + 4 h + e, so a lane's
// four consecutive steps are one 16-byte piece of its row (vector load when the input map is the
// identity) and one 16-byte piece of its centre.
// Product 2 consumes product 1's accumulator registers as its B operand: register r of lane half
// h holds unit (r & 3) + 8 (r >> 2) + 4 h of the tile, and the output weights are stored in that order.
//
// The hidden normalisations need no second pass: both divide by a per-row scalar, so the products
// run on the unnormalised terms, the sum is kept beside them (lane-local, one lane ^ 32 exchange)
// and the output accumulators are divided once. softmax needs no running maximum because
// a_j <= A_max = max_j altitude_j^fanIn is known at lowering (the host refuses A_max > 64).
// Padded units carry |w|^2 = +inf (a = 0) and zero output weights; under softmax their
// exp(0 - A_max) is masked out of the sum.
#include "common.h"
#include "epilogue.h"
#include "nn_act.h"

namespace {

constexpr int TB = 256;
constexpr int NIN = 128;             // max inputs
constexpr int TAIL = 1024 + 128;     // panel floats after the centre fragments: V slice, then c | g | |w|^2 (+ pad)

typedef float f32x16 __attribute__((ext_vector_type(16)));

enum : int { HN_NONE = 0, HN_SOFTMAX = 1, HN_SIMPLEMAX = 2 };

struct RbfArgs {
  const float* X;
  int n_rows, n_feat, ldx, n_in;
  const float* in_scale;    // [n_in]
  const float* in_shift;    // [n_in] shift - centroid
  const float* in_missing;  // [n_in] replacement - centroid (NaN = the row has no prediction)
  const int* in_index;      // [n_in] column of each input
  const float* panels;      // [n_tiles][kp * 32 + TAIL]
  const float* out_bias;    // [32]
  int kp, n_tiles;          // padded inputs (16 | 32 | 64 | 128), 32-unit hidden tiles
  int hidden_norm, out_act;
  float out_thr, a_max;
  int final_norm, n_out;    // final_norm: 0 none, 1 softmax, 2 simplemax
  int classification, contiguous;  // contiguous: in_index[k] == k
  Epilogue epi;
  float* score;
  uint8_t* valid;
  float* probs;             // [n, n_out] (nullable)
};

// unit of a 32x32 accumulator tile held by register r of lane half h
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// np.argmax order: a NaN is the maximum, the first of equals wins
__device__ __forceinline__ bool beats(float v, int u, float bv, int bu) {
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;
  if (vn || v == bv) return u < bu;
  return v > bv;
}

// One 32-row N tile after the last hidden tile: hidden normalisation, bias + output activation,
// output normalisation and the decode. Every lane of the wave runs it (lane ^ 32 exchanges).
__device__ __forceinline__ void rbf_finish(const RbfArgs& a, f32x16 out, float sum, int nbad, int row, int h) {
  nbad += __shfl_xor(nbad, 32);
  const bool bad = nbad != 0;
  const bool in_range = row < a.n_rows;
  if (a.hidden_norm != HN_NONE) sum += __shfl_xor(sum, 32);
  float p[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float z = out[r];
    if (a.hidden_norm != HN_NONE) z /= sum;  // 0 / 0: every unit underflowed, the row has no value
    p[r] = activate(a.out_act, z + a.out_bias[acc_row(r, h)], a.out_thr);
  }
  if (a.final_norm != 0) {
    float mx = -__builtin_inff();
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (acc_row(r, h) < a.n_out) mx = fmaxf(mx, p[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float fs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (a.final_norm == 1) p[r] = __expf(p[r] - mx);
      fs += acc_row(r, h) < a.n_out ? p[r] : 0.f;
    }
    fs += __shfl_xor(fs, 32);
#pragma unroll
    for (int r = 0; r < 16; ++r) p[r] /= fs;
  }
  if (!a.classification) {  // one output neuron: unit 0 = register 0 of lane half 0
    if (h == 0 && in_range)
      apply_epilogue(a.epi, [&](int) { return p[0]; }, !bad, row, a.n_rows, a.score, a.valid, a.probs);
    return;
  }
  float best = -__builtin_inff();
  int best_u = 1 << 30;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int u = acc_row(r, h);
    if (u < a.n_out) {
      if (beats(p[r], u, best, best_u)) { best = p[r]; best_u = u; }
      if (a.probs && in_range) a.probs[(size_t)row * a.n_out + u] = bad ? __builtin_nanf("") : p[r];
    }
  }
  const float ob = __shfl_xor(best, 32);
  const int ou = __shfl_xor(best_u, 32);
  if (beats(ob, ou, best, best_u)) { best = ob; best_u = ou; }
  if (h == 0 && in_range) {
    bool ok = !bad && best_u < a.n_out;
    float sc = ok ? (a.epi.has_table ? a.epi.table[best_u] : (float)best_u) : __builtin_nanf("");
    ok = ok && (sc == sc);
    sc = ok ? sc : __builtin_nanf("");
    a.score[row] = sc;
    a.valid[row] = ok ? 1 : 0;
    if (a.epi.score2) {
      a.epi.score2[row] = sc;
      a.epi.valid2[row] = ok ? 1 : 0;
    }
  }
}

template <int KS>  // k-steps of product 1: kp / 2
__global__ __launch_bounds__(TB) void rbf_kernel(RbfArgs a) {
  constexpr int PV = (KS * 64 + TAIL) / 4;   // float4 per panel
  constexpr int NV = (PV + TB - 1) / TB;     // float4 per thread per panel copy
  extern __shared__ __align__(16) float4 smem4[];
  float4* ring = smem4;                      // [2][PV]
  float* s_sc = reinterpret_cast<float*>(ring + 2 * PV);
  float* s_sh = s_sc + NIN;
  float* s_ms = s_sh + NIN;
  int* s_ix = reinterpret_cast<int*>(s_ms + NIN);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int h = lane >> 5;
  const int col = lane & 31;

  for (int k = tid; k < NIN; k += TB) {
    const bool u = k < a.n_in;
    s_sc[k] = u ? a.in_scale[k] : 0.f;
    s_sh[k] = u ? a.in_shift[k] : 0.f;
    s_ms[k] = u ? a.in_missing[k] : 0.f;
    s_ix[k] = u ? a.in_index[k] : 0;
  }
  {
    const float4* g = reinterpret_cast<const float4*>(a.panels);
    for (int i = tid; i < PV; i += TB) ring[i] = g[i];
  }
  __syncthreads();

  // ---- input stage: the B fragments of both N tiles, |x|^2 and the missing-input count
  const int rb = blockIdx.x * TB + wave * 64 + col;
  float xb[2][KS];
  float xx[2] = {0.f, 0.f};
  int nbad[2] = {0, 0};
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int row = rb + 32 * t;
    const float* xrow = a.X + (size_t)(row < a.n_rows ? row : 0) * a.ldx;
#pragma unroll
    for (int q = 0; q < KS / 4; ++q) {
      const int kb = 8 * q + 4 * h;
      float v[4];
      if (a.contiguous && kb + 3 < a.n_in) {
        const float4 f = *reinterpret_cast<const float4*>(xrow + kb);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
      } else {  // padded inputs re-read the last real one and are masked to 0 below
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = xrow[s_ix[min(kb + e, a.n_in - 1)]];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = min(kb + e, a.n_in - 1);
        float y = (v[e] != v[e]) ? s_ms[k] : fmaf(v[e], s_sc[k], s_sh[k]);
        // k < n_in as an integer mask, not a select: 128 selects' lane masks, kept live across both
        // N tiles, would not fit the scalar registers
        y = __int_as_float(__float_as_int(y) & ((kb + e - a.n_in) >> 31));
        nbad[t] += (y != y) ? 1 : 0;
        y = (y != y) ? 0.f : y;  // a row with a missing input computes on zeros and is written invalid
        xb[t][4 * q + e] = y;
        xx[t] = fmaf(y, y, xx[t]);
      }
    }
    xx[t] += __shfl_xor(xx[t], 32);
  }

  f32x16 out0 = {}, out1 = {};
  float sum0 = 0.f, sum1 = 0.f;
  const float inf = __builtin_inff();
#pragma unroll 1
  for (int t = 0; t < a.n_tiles; ++t) {
    const float4* P = ring + (t & 1) * PV;
    const bool more = t + 1 < a.n_tiles;
    // unconditional loads (the last tile re-reads itself, a thread past the panel its last piece):
    // a conditionally filled register array goes to scratch
    float4 pre[NV];
    {
      const float4* g = reinterpret_cast<const float4*>(a.panels) + (size_t)(more ? t + 1 : t) * PV;
#pragma unroll
      for (int i = 0; i < NV; ++i) pre[i] = g[min(tid + i * TB, PV - 1)];
    }
    // ---- product 1: G = Wc . x^T for this tile's 32 units
    f32x16 acc0 = {}, acc1 = {};
#pragma unroll
    for (int q = 0; q < KS / 4; ++q) {
      const float4 w = P[q * 64 + lane];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, xb[0][4 * q + 0], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, xb[1][4 * q + 0], acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, xb[0][4 * q + 1], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, xb[1][4 * q + 1], acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, xb[0][4 * q + 2], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, xb[1][4 * q + 2], acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, xb[0][4 * q + 3], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, xb[1][4 * q + 3], acc1, 0, 0, 0);
    }
    // ---- activation on the accumulators: register r of this lane half is unit acc_row(r, h)
    const float4* V4 = P + KS * 16;
    const float4* C4 = V4 + 256 + 4 * h;  // c[2][16] | g[2][16] | wn[2][16]
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const float4 c4 = C4[r4], g4 = C4[8 + r4], n4 = C4[16 + r4];
      const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, gg[4] = {g4.x, g4.y, g4.z, g4.w},
                  wn[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * r4 + e;
        float d0 = fmaf(-2.f, acc0[r], xx[0]) + wn[e];
        float d1 = fmaf(-2.f, acc1[r], xx[1]) + wn[e];
        d0 = d0 < 0.f ? 0.f : d0;  // the expansion can dip below 0 by rounding at a centre
        d1 = d1 < 0.f ? 0.f : d1;
        d0 = d0 != d0 ? inf : d0;  // inf - inf of an overflowed |x|^2: infinitely far
        d1 = d1 != d1 ? inf : d1;
        float b0 = __expf(cc[e] - gg[e] * d0);
        float b1 = __expf(cc[e] - gg[e] * d1);
        if (a.hidden_norm == HN_SOFTMAX) {
          const bool unit = wn[e] < inf;  // a padded unit's exp(0 - A_max) stays out of the sum
          b0 = unit ? __expf(b0 - a.a_max) : 0.f;
          b1 = unit ? __expf(b1 - a.a_max) : 0.f;
        }
        sum0 += b0;
        sum1 += b1;
        acc0[r] = b0;
        acc1[r] = b1;
      }
    }
    // ---- product 2: out += V[:, tile] . a, the B operand is product 1's register file
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const float4 v = V4[r4 * 64 + lane];
      out0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v.x, acc0[4 * r4 + 0], out0, 0, 0, 0);
      out1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v.x, acc1[4 * r4 + 0], out1, 0, 0, 0);
      out0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v.y, acc0[4 * r4 + 1], out0, 0, 0, 0);
      out1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v.y, acc1[4 * r4 + 1], out1, 0, 0, 0);
      out0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v.z, acc0[4 * r4 + 2], out0, 0, 0, 0);
      out1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v.z, acc1[4 * r4 + 2], out1, 0, 0, 0);
      out0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v.w, acc0[4 * r4 + 3], out0, 0, 0, 0);
      out1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v.w, acc1[4 * r4 + 3], out1, 0, 0, 0);
    }
    // ---- panel t + 1 into the slot tile t - 1 was read from (every wave passed that tile's barrier)
    if (more) {
      float4* dst = ring + ((t + 1) & 1) * PV;
#pragma unroll
      for (int i = 0; i < NV; ++i)
        if (tid + i * TB < PV) dst[tid + i * TB] = pre[i];
    }
    __syncthreads();
  }
  rbf_finish(a, out0, sum0, nbad[0], rb, h);
  rbf_finish(a, out1, sum1, nbad[1], rb + 32, h);
}

template <int KS>
int launch(hipStream_t stream, const RbfArgs& a) {
  const size_t lds = (size_t)2 * (KS * 64 + TAIL) * 4 + 4 * NIN * 4;
  dim3 grid((a.n_rows + TB - 1) / TB);
  hipLaunchKernelGGL(rbf_kernel<KS>, grid, dim3(TB), lds, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -7;
}

}  // namespace

PMML_API int pmml_rbf_args_size() { return (int)sizeof(RbfArgs); }

PMML_API int pmml_rbf_launch(hipStream_t stream, const RbfArgs* args) {
  const RbfArgs a = *args;
  if (a.n_rows <= 0) return 0;
  if (a.n_in < 1 || a.n_in > NIN || a.n_in > a.kp || a.n_tiles < 1 || a.n_tiles > 32 || a.n_out < 1 ||
      a.n_out > 32 || a.hidden_norm < 0 || a.hidden_norm > 2 || a.final_norm < 0 || a.final_norm > 2)
    return -4;
  if (a.contiguous && (a.n_feat < a.n_in || (a.ldx & 3) != 0 || ((uintptr_t)a.X & 15) != 0)) return -4;
  switch (a.kp) {
    case 16: return launch<8>(stream, a);
    case 32: return launch<16>(stream, a);
    case 64: return launch<32>(stream, a);
    case 128: return launch<64>(stream, a);
    default: return -4;
  }
}
