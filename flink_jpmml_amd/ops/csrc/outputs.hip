// PMML <Output> columns and top-k classes of a scored batch (gfx950 / CDNA4, wave64).
//
// A model plan launched in index mode leaves, per row, a raw result: the regression value or the
// class / cluster INDEX, a validity byte, optionally C class probabilities and the winning entity's
// affinity. This kernel turns them into the n_col output columns of the model's <Output> element
// in one pass, plus the reference score (the label parsed as a double) the plan's own epilogue
// would have written with its label table on. It only moves bits: no arithmetic touches a value.
//
// One 256-thread workgroup owns R consecutive rows. Their R x C probabilities are staged in LDS by
// coalesced loads (16 bytes per lane when base and stride allow), with the row stride padded to an
// odd dword count so the one-row-per-lane ds_read_b32 scan is bank-conflict free. Lane t scans
// row t once, keeping the top-k in registers (a fully unrolled compare-insert chain, no
// dynamically indexed array: nothing goes to scratch), evaluates the column program into an LDS
// output tile (odd stride again), and the tile streams out coalesced.
#include "common.h"

struct OutputArgs {
  const float* score;        // [m] regression value, or class / cluster index
  const uint8_t* valid;      // [m]
  const float* probs;        // [m, C] row stride ldp, or null
  const float* affinity;     // [m] or null
  const int* prog;           // [n_col][4] {op, arg, table_off, 0}
  const float* tables;       // [n_tables] label / entity encodings and constants
  const float* label_table;  // [C_label + 1], last entry NaN; null: score passes through
  float* out;                // [m, n_col] row stride ldo
  float* score_out;          // [m] or null
  uint8_t* valid_out;        // [m] or null
  int m, C, ldp, n_col, ldo, k, n_tables, n_labels;
};

enum : int { OUT_VALUE = 0, OUT_TABLE = 1, OUT_PROB = 2, OUT_PROB_WINNER = 3, OUT_AFFINITY = 4, OUT_CONST = 5,
             OUT_NAN = 6, OUT_TOPK_INDEX = 7, OUT_TOPK_PROB = 8 };

constexpr int OUT_TB = 256;
constexpr int OUT_TILE_BYTES = 64 * 1024;  // both tiles of one workgroup: two workgroups per CU
constexpr int OUT_MAX_C = 256;             // SEG_MAXC
constexpr int OUT_MAX_COLS = 64;
constexpr int OUT_MAX_K = 8;

static inline int out_rows(int C, int n_col) {
  const int words = (C > 0 ? (C | 1) : 0) + (n_col | 1);
  const int r = OUT_TILE_BYTES / (4 * words);
  return r < 1 ? 1 : (r > OUT_TB ? OUT_TB : r);
}

// The K best (value, class) pairs seen so far, best first. An equal value never displaces an
// earlier (lower) class, a NaN is never offered; empty slots carry class -1.
template <int K>
struct TopK {
  float v[K > 0 ? K : 1];
  int i[K > 0 ? K : 1];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < K; ++j) { v[j] = __builtin_nanf(""); i[j] = -1; }
  }
  __device__ __forceinline__ void offer(float p, int c) {
    if (!(p == p)) return;
    bool taken = false;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const bool take = taken || i[j] < 0 || p > v[j];
      const float tv = v[j];
      const int ti = i[j];
      if (take) { v[j] = p; i[j] = c; p = tv; c = ti; taken = true; }
    }
  }
  __device__ __forceinline__ void get(int r, float* pv, int* pi) const {
    float x = __builtin_nanf("");
    int y = -1;
#pragma unroll
    for (int j = 0; j < K; ++j) if (j == r) { x = v[j]; y = i[j]; }
    *pv = x;
    *pi = y;
  }
};

template <int K>
__global__ __launch_bounds__(OUT_TB) void outputs_kernel(OutputArgs a, int R) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int C = a.probs ? a.C : 0;
  const int SP = C > 0 ? (C | 1) : 0;
  const int n_col = a.n_col;
  const int SO = n_col | 1;
  float* ps = reinterpret_cast<float*>(smem);  // [R, SP]
  float* os = ps + (size_t)R * SP;             // [R, SO]
  const int r0 = blockIdx.x * R;
  const int nr = min(R, a.m - r0);
  const int t = threadIdx.x;
  const float nan = __builtin_nanf("");

  if (C > 0) {
    const float* src = a.probs + (size_t)r0 * a.ldp;
    const int count = nr * C;
    if (a.ldp == C && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
      const int c4 = count >> 2;
      for (int q = t; q < c4; q += OUT_TB) {
        const float4 v = reinterpret_cast<const float4*>(src)[q];
        const float vv[4] = {v.x, v.y, v.z, v.w};
        int r = (4 * q) / C;
        int c = 4 * q - r * C;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          ps[r * SP + c] = vv[e];
          if (++c == C) { c = 0; ++r; }
        }
      }
      for (int i = 4 * c4 + t; i < count; i += OUT_TB) {
        const int r = i / C;
        ps[r * SP + (i - r * C)] = src[i];
      }
    } else {
      for (int i = t; i < count; i += OUT_TB) {
        const int r = i / C;
        const int c = i - r * C;
        ps[r * SP + c] = src[(size_t)r * a.ldp + c];
      }
    }
    __syncthreads();
  }

  if (t < nr) {
    const int row = r0 + t;
    const float s = a.score[row];
    const bool ok = a.valid[row] != 0;
    const bool okidx = ok && (s == s);
    const float* prow = ps + t * SP;
    TopK<K> top;
    top.clear();
    if (K > 0 && ok) {
      for (int c = 0; c < C; ++c) top.offer(prow[c], c);
    }
    for (int j = 0; j < n_col; ++j) {
      const int op = a.prog[4 * j + 0];
      const int arg = a.prog[4 * j + 1];
      const int off = a.prog[4 * j + 2];
      float x = nan;
      switch (op) {
        case OUT_VALUE:
          if (ok) x = s;
          break;
        case OUT_TABLE: {
          const int idx = (okidx && s >= 0.f && s < (float)arg) ? (int)s : arg;
          const long long pos = (long long)off + idx;
          if (arg >= 0 && off >= 0 && pos < a.n_tables) x = a.tables[pos];
          break;
        }
        case OUT_PROB:
          if (ok && arg >= 0 && arg < C) x = prow[arg];
          break;
        case OUT_PROB_WINNER:
          if (ok && C > 0) x = prow[(okidx && s >= 0.f && s < (float)C) ? (int)s : 0];
          break;
        case OUT_AFFINITY:
          if (ok && a.affinity) x = a.affinity[row];
          break;
        case OUT_CONST:
          if (off >= 0 && off < a.n_tables) x = a.tables[off];
          break;
        case OUT_TOPK_INDEX:
        case OUT_TOPK_PROB: {
          float pv;
          int pi;
          top.get(arg < a.k ? arg : -1, &pv, &pi);
          if (op == OUT_TOPK_PROB) x = pv;
          else if (pi >= 0) x = (float)pi;
          break;
        }
        default:
          break;
      }
      os[t * SO + j] = x;
    }
    if (a.score_out) {
      float so = s;
      bool vo = ok;
      if (a.label_table) {
        const int L = a.n_labels;
        so = a.label_table[(okidx && s >= 0.f && s < (float)L) ? (int)s : L];
        vo = ok && (so == so);
        if (!vo) so = nan;
      }
      a.score_out[row] = so;
      if (a.valid_out) a.valid_out[row] = vo ? 1 : 0;
    }
  }
  __syncthreads();

  float* dst = a.out + (size_t)r0 * a.ldo;
  const int count = nr * n_col;
  if (a.ldo == n_col && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    const int c4 = count >> 2;
    for (int q = t; q < c4; q += OUT_TB) {
      int r = (4 * q) / n_col;
      int c = 4 * q - r * n_col;
      float vv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        vv[e] = os[r * SO + c];
        if (++c == n_col) { c = 0; ++r; }
      }
      reinterpret_cast<float4*>(dst)[q] = make_float4(vv[0], vv[1], vv[2], vv[3]);
    }
    for (int i = 4 * c4 + t; i < count; i += OUT_TB) {
      const int r = i / n_col;
      dst[i] = os[r * SO + (i - r * n_col)];
    }
  } else {
    for (int i = t; i < count; i += OUT_TB) {
      const int r = i / n_col;
      const int c = i - r * n_col;
      dst[(size_t)r * a.ldo + c] = os[r * SO + c];
    }
  }
}

PMML_API int pmml_outputs_args_size() { return (int)sizeof(OutputArgs); }

// Rows of one workgroup for C probability columns and n_col outputs (ops/outputs.py mirrors this).
PMML_API int pmml_outputs_rows(int C, int n_col) {
  return (C < 0 || C > OUT_MAX_C || n_col < 1 || n_col > OUT_MAX_COLS) ? 0 : out_rows(C, n_col);
}

PMML_API int pmml_outputs_launch(hipStream_t stream, const OutputArgs* args) {
  OutputArgs a = *args;
  if (a.m < 0 || a.C < 0 || a.C > OUT_MAX_C || a.n_col < 1 || a.n_col > OUT_MAX_COLS) return -1;
  if (a.k < 0 || a.k > OUT_MAX_K || a.n_tables < 0 || a.n_labels < 0) return -1;
  if (a.m == 0) return 0;
  if (!a.score || !a.valid || !a.prog || !a.out || (a.n_tables > 0 && !a.tables)) return -2;
  if (a.ldo < a.n_col || (a.probs && a.ldp < a.C)) return -3;
  if (!a.probs) a.C = 0;
  if (a.C == 0) { a.probs = nullptr; a.k = 0; }
  const int R = out_rows(a.C, a.n_col);
  const size_t lds = (size_t)R * ((a.C > 0 ? (a.C | 1) : 0) + (a.n_col | 1)) * 4;
  const dim3 grid((a.m + R - 1) / R), block(OUT_TB);
  if (a.k == 0) hipLaunchKernelGGL(outputs_kernel<0>, grid, block, lds, stream, a, R);
  else if (a.k == 1) hipLaunchKernelGGL(outputs_kernel<1>, grid, block, lds, stream, a, R);
  else if (a.k == 2) hipLaunchKernelGGL(outputs_kernel<2>, grid, block, lds, stream, a, R);
  else if (a.k <= 4) hipLaunchKernelGGL(outputs_kernel<4>, grid, block, lds, stream, a, R);
  else hipLaunchKernelGGL(outputs_kernel<8>, grid, block, lds, stream, a, R);
  return hipGetLastError() == hipSuccess ? 0 : -7;
}
