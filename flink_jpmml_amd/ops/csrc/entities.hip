// Ranked entities of the two distance families (gfx950 / CDNA4, wave64): per row, the R nearest
// clusters of a ClusteringModel or the k neighbours of a NearestNeighborModel, as entity ids and
// affinities, plus the affinity of every entity an Output field names.
//
// The kernel reads what the model's own kernel read — the raw [n, F] fp32 rows, FieldPrep applied
// while staging with stage_rows_T — and the plan's own tensors (entities [N][F], weights, scales,
// qweights, cfun, metric, similarity, p; wc / cc for the expansion). It repeats the plan's
// arithmetic statement for statement, so rank 1 is the plan's own winner and affinity bit for bit:
//
//   VALU, knn = 0 (cluster.hip::cluster_kernel): every sum is finished (Σq/Σq_present rescale,
//     root, 1/p power) and the finished values are compared, strict <, entities in index order.
//   VALU, knn = 1 (knn.hip::knn_kernel): the raw sums are compared; only the entries reported and
//     the named entities are finished.
//   MFMA (cluster_mfma_kernel / knn_mfma_kernel: squared / plain euclidean, absDiff, distance):
//     fmaf(-2, acc, xx) + cc per entity, 16 entities of one row per lane per 32-entity tile into the
//     lane's own list, the two half-waves' lists merged through lane^32; knn = 1 clamps at 0 before
//     the comparison, knn = 0 after it. A row with a missing value is redone in the VALU form.
//
// The list is knn.hip's (distance.h): KMAX in {8, 32} registers kept sorted by (key, entity index)
// with an unrolled compare-exchange chain; a rank is read back with a select chain. Nothing is
// indexed dynamically, nothing goes to scratch.
//
// Columns {op, arg, table offset, destination}: ENT_ID writes tables[offset + entity] of rank arg,
// ENT_AFFINITY its finished affinity, ENT_NAMED the finished affinity of entity arg. named[N] maps
// an entity to the tile column of the first field naming it (-1: none), so the distance loop drops
// a named value where it computes it and 64 named clusters cost no second pass. A row is valid
// when no field preparation rejected it, Σq_present > 0 and rank 1 is finite (knn = 1: all k
// neighbours are, the oracle's rule); its columns are NaN otherwise, as is a rank past the list or
// with a non-finite affinity. The tile [rows][n_col | 1] is staged in LDS and streams out with
// consecutive lanes on consecutive columns; only the kernel's own columns of out are written.
#include "common.h"
#include "distance.h"

struct EntityArgs {
  const float* X;          // [n_rows, ldx] raw rows
  const FieldPrep* prep;   // [n_feat] or null
  const float* ent;        // [n_ent][n_feat] centres / training instances
  const float* weights;    // [n_feat]
  const float* scales;     // [n_feat] gaussSim similarity scale
  const float* qweights;   // [n_feat] missing-value weights
  const int* cfun;         // [n_feat] compare function codes
  const float* wc;         // [Np][Fp] w∘c zero padded, or null (VALU)
  const float* cc;         // [Np] Σ w c², +inf on padding
  const int4* cols;        // [n_col] {op, arg, table offset, destination column}
  const int* named;        // [n_ent] tile column of a named entity, or -1
  const float* tables;     // [n_tables] id encodings, n_ent per ENT_ID column
  float* out;              // [n_rows, ldo]
  int n_rows, n_feat, ldx, ldo;
  int n_ent, metric, similarity, k;
  int knn, n_col, n_tables, rows;
  int Np, Fp;
  float p;
  int pad;
};

namespace {

enum : int { ENT_ID = 0, ENT_AFFINITY = 1, ENT_NAMED = 2 };

constexpr int ENT_MAX_COLS = 64;
constexpr int ENT_MAX_F = 128;
constexpr int ENT_LDS_BYTES = 64 * 1024;  // one workgroup's request: two workgroups share a CU

template <int KMAX>
__device__ __forceinline__ void list_clear(float (&key)[KMAX], int (&id)[KMAX]) {
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    key[j] = __builtin_inff();
    id[j] = 0x7fffffff;
  }
}

// ---- one row

// The exact (VALU) form of one row: the list over all entities and the named entities' columns.
// METRIC names the raw sum, a.metric the finish (the expansion redoes a euclidean row as squared
// sums). Returns Σq_present > 0; *adj_out takes the rescale of the entries still to be finished.
template <int METRIC, int KMAX>
__device__ __forceinline__ bool exact_row(const EntityArgs& a, const float* fr, int stride, float (&key)[KMAX],
                                          int (&id)[KMAX], float* orow, float* adj_out) {
  float qpresent;
  const float adj = row_adjust(a, fr, stride, &qpresent);
  list_clear<KMAX>(key, id);
  // entities arrive in increasing index, so a tie with the k-th entry never displaces it
  float worst = __builtin_inff();
  for (int i = 0; i < a.n_ent; ++i) {
    const float s = raw_distance<METRIC>(a, fr, stride, a.ent + (size_t)i * a.n_feat);
    const int nc = a.named[i];
    float fin = s;
    if (!a.knn || nc >= 0) fin = finish_distance(a.metric, s, adj, a.p);
    if (nc >= 0) orow[nc] = fin;
    float ck = a.knn ? s : fin;
    ck = a.similarity ? -ck : ck;
    if (ck < worst) {
      topk_insert<KMAX>(key, id, a.k, ck, i);
      worst = kth<KMAX>(key, a.k);
    }
  }
  *adj_out = adj;
  return qpresent > 0.f;
}

// The affinity a list key stands for: the sign of a similarity undone, the expansion's clamp, the
// finish of a raw sum.
__device__ __forceinline__ float key_affinity(const EntityArgs& a, float key, float adj, bool finished, bool clamp) {
  float v = a.similarity ? -key : key;
  if (clamp) v = fmaxf(v, 0.f);
  return finished ? v : finish_distance(a.metric, v, adj, a.p);
}

// The row's columns into its tile row. The named columns already hold their affinities.
template <int KMAX>
__device__ __forceinline__ void write_columns(const EntityArgs& a, const float (&key)[KMAX], const int (&id)[KMAX],
                                              float adj, bool finished, bool clamp, bool ok, float* orow) {
  bool all = true, first = false;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    const float v = key_affinity(a, key[j], adj, finished, clamp);
    const bool live = __builtin_isfinite(v) && id[j] >= 0 && id[j] < a.n_ent;
    if (j < a.k) all = all && live;
    if (j == 0) first = live;
  }
  ok = ok && (a.knn ? all : first);
  const float nan = __builtin_nanf("");
  for (int c = 0; c < a.n_col; ++c) {
    const int4 col = a.cols[c];
    float x = nan;
    if (col.x == ENT_NAMED) {
      const int src = (col.y >= 0 && col.y < a.n_ent) ? a.named[col.y] : -1;
      if (ok && src >= 0 && src <= c) x = orow[src];
    } else {
      float kv = __builtin_inff();
      int ki = -1;
#pragma unroll
      for (int j = 0; j < KMAX; ++j) {
        const bool hit = j == col.y && j < a.k;
        kv = hit ? key[j] : kv;
        ki = hit ? id[j] : ki;
      }
      const float v = key_affinity(a, kv, adj, finished, clamp);
      if (ok && ki >= 0 && ki < a.n_ent && __builtin_isfinite(v)) {
        if (col.x == ENT_AFFINITY) {
          x = v;
        } else {
          const long long pos = (long long)col.z + ki;
          if (col.z >= 0 && pos < a.n_tables) x = a.tables[pos];
        }
      }
    }
    orow[c] = x;
  }
}

// The tile's rows into their columns of out: consecutive lanes, consecutive columns of one row.
template <int TB>
__device__ __forceinline__ void stream_out(const EntityArgs& a, const float* os, int SO, int row0) {
  const int nr = min(TB, a.n_rows - row0);
  const int count = nr * a.n_col;
  for (int e = threadIdx.x; e < count; e += TB) {
    const int r = e / a.n_col;
    const int c = e - r * a.n_col;
    const int dst = a.cols[c].w;
    if (dst >= 0 && dst < a.ldo) a.out[(size_t)(row0 + r) * a.ldo + dst] = os[r * SO + c];
  }
}

// ---- kernels

template <int METRIC, int KMAX, int TB>
__global__ __launch_bounds__(TB) void entities_kernel(EntityArgs a) {
  extern __shared__ __align__(16) uint32_t smem[];
  float* feat = reinterpret_cast<float*>(smem);               // [F][TB]
  int* bad = reinterpret_cast<int*>(smem + a.n_feat * TB);    // [TB]
  float* os = reinterpret_cast<float*>(smem + a.n_feat * TB + TB);  // [TB][SO]
  const int SO = a.n_col | 1;
  const int row0 = blockIdx.x * TB;
  stage_rows_T<TB>(a.X, a.n_rows, a.n_feat, a.ldx, a.prep, feat, bad, row0);
  const int tid = threadIdx.x;
  if (row0 + tid < a.n_rows) {
    float key[KMAX];
    int id[KMAX];
    float adj;
    float* orow = os + tid * SO;
    const bool present = exact_row<METRIC, KMAX>(a, feat + tid, TB, key, id, orow, &adj);
    write_columns<KMAX>(a, key, id, adj, !a.knn, false, present && bad[tid] == 0, orow);
  }
  __syncthreads();
  stream_out<TB>(a, os, SO, row0);
}

typedef float f32x16_t __attribute__((ext_vector_type(16)));

template <int KMAX>
__device__ __forceinline__ void mfma_row_finish(const EntityArgs& a, const float* feat, const int* bad, int stride,
                                                float (&key)[KMAX], int (&id)[KMAX], bool missing, int rl, int row0,
                                                float* orow) {
  if (row0 + rl >= a.n_rows) return;
  if (missing) {
    float adj;
    const bool present = exact_row<M_SQEUCLID, KMAX>(a, feat + rl, stride, key, id, orow, &adj);
    write_columns<KMAX>(a, key, id, adj, !a.knn, false, present && bad[rl] == 0, orow);
  } else {
    write_columns<KMAX>(a, key, id, 1.f, false, true, bad[rl] == 0, orow);
  }
}

template <int KMAX, int TB>
__global__ __launch_bounds__(TB) void entities_mfma_kernel(EntityArgs a) {
  extern __shared__ __align__(16) uint32_t smem[];
  float* feat = reinterpret_cast<float*>(smem);
  int* bad = reinterpret_cast<int*>(smem + a.n_feat * TB);
  float* os = reinterpret_cast<float*>(smem + a.n_feat * TB + TB);
  const int SO = a.n_col | 1;
  const int row0 = blockIdx.x * TB;
  stage_rows_T<TB>(a.X, a.n_rows, a.n_feat, a.ldx, a.prep, feat, bad, row0);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int half = lane >> 5;
  const int F = a.n_feat;
  const int Fp = a.Fp;
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
  list_clear<KMAX>(key0, id0);
  list_clear<KMAX>(key1, id1);
  float worst0 = __builtin_inff(), worst1 = __builtin_inff();
  for (int i0 = 0; i0 < a.Np; i0 += 32) {
    f32x16_t acc0 = {}, acc1 = {};
    const float* wrow = a.wc + (size_t)(i0 + (lane & 31)) * Fp;
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
    for (int r = 0; r < 16; ++r) {  // D[entity (r&3)+8(r>>2)+4*half][row lane&31]
      const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const float ci = a.cc[i];
      float d0 = fmaf(-2.f, acc0[r], xx[0]) + ci;
      float d1 = fmaf(-2.f, acc1[r], xx[1]) + ci;
      if (a.knn) {  // knn_mfma_kernel compares the clamped value, cluster_mfma_kernel clamps its winner
        d0 = fmaxf(d0, 0.f);
        d1 = fmaxf(d1, 0.f);
      }
      const int nc = i < a.n_ent ? a.named[i] : -1;
      if (nc >= 0) {
        os[rb * SO + nc] = finish_distance(a.metric, fmaxf(d0, 0.f), 1.f, a.p);
        os[(rb + 32) * SO + nc] = finish_distance(a.metric, fmaxf(d1, 0.f), 1.f, a.p);
      }
      // within a lane entities arrive in increasing index: strict < keeps the lower index on ties
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
  // merge the partner half-wave's lists (same rows, the other entities of every tile)
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
  __syncthreads();  // the partner half-wave's named columns of these rows are in the tile
  if (half == 0) {
    mfma_row_finish<KMAX>(a, feat, bad, TB, key0, id0, missing[0], rb, row0, os + rb * SO);
    mfma_row_finish<KMAX>(a, feat, bad, TB, key1, id1, missing[1], rb + 32, row0, os + (rb + 32) * SO);
  }
  __syncthreads();
  stream_out<TB>(a, os, SO, row0);
}

size_t ent_lds_bytes(int n_feat, int n_col, int rows) {
  return (size_t)n_feat * rows * 4 + (size_t)rows * 4 + (size_t)rows * (n_col | 1) * 4;
}

template <int KMAX, int TB>
int launch_valu(hipStream_t stream, const EntityArgs& a, dim3 grid, size_t lds) {
  switch (a.metric) {
    case M_SQEUCLID: hipLaunchKernelGGL((entities_kernel<M_SQEUCLID, KMAX, TB>), grid, dim3(TB), lds, stream, a); break;
    case M_EUCLID: hipLaunchKernelGGL((entities_kernel<M_EUCLID, KMAX, TB>), grid, dim3(TB), lds, stream, a); break;
    case M_CITY: hipLaunchKernelGGL((entities_kernel<M_CITY, KMAX, TB>), grid, dim3(TB), lds, stream, a); break;
    case M_CHEBY: hipLaunchKernelGGL((entities_kernel<M_CHEBY, KMAX, TB>), grid, dim3(TB), lds, stream, a); break;
    case M_MINKOWSKI: hipLaunchKernelGGL((entities_kernel<M_MINKOWSKI, KMAX, TB>), grid, dim3(TB), lds, stream, a); break;
    default: return -6;
  }
  return 0;
}

template <int TB>
int launch_rows(hipStream_t stream, const EntityArgs& a, size_t lds) {
  const dim3 grid((a.n_rows + TB - 1) / TB);
  if (a.wc) {
    if (a.k <= 8) hipLaunchKernelGGL((entities_mfma_kernel<8, TB>), grid, dim3(TB), lds, stream, a);
    else hipLaunchKernelGGL((entities_mfma_kernel<32, TB>), grid, dim3(TB), lds, stream, a);
    return 0;
  }
  return a.k <= 8 ? launch_valu<8, TB>(stream, a, grid, lds) : launch_valu<32, TB>(stream, a, grid, lds);
}

}  // namespace

PMML_API int pmml_entities_args_size() { return (int)sizeof(EntityArgs); }

// LDS request of one workgroup (ops/entities.py mirrors this); -1: not a shape the kernel takes.
PMML_API long long pmml_entities_lds_bytes(int n_feat, int n_col, int rows) {
  if (n_feat < 1 || n_feat > ENT_MAX_F || n_col < 1 || n_col > ENT_MAX_COLS ||
      (rows != 64 && rows != 128 && rows != 256))
    return -1;
  return (long long)ent_lds_bytes(n_feat, n_col, rows);
}

PMML_API int pmml_entities_launch(hipStream_t stream, const EntityArgs* args) {
  const EntityArgs a = *args;
  if (a.n_rows < 0 || a.n_feat < 1 || a.n_feat > ENT_MAX_F || a.n_ent < 1 || a.n_tables < 0) return -1;
  if (a.k < 1 || a.k > 32 || a.k > a.n_ent || a.n_col < 1 || a.n_col > ENT_MAX_COLS) return -1;
  if (a.rows != 64 && a.rows != 128 && a.rows != 256) return -1;
  if (a.n_rows == 0) return 0;
  if (!a.X || !a.ent || !a.weights || !a.scales || !a.qweights || !a.cfun || !a.cols || !a.named || !a.tables ||
      !a.out)
    return -2;
  if (a.ldx < a.n_feat || a.ldo < 1) return -3;
  if (a.wc) {
    if (!a.cc || (a.Np & 31) || (a.Fp & 1) || a.Fp < a.n_feat || a.Np < a.n_ent || a.similarity) return -4;
    if (a.metric != M_SQEUCLID && a.metric != M_EUCLID) return -6;
  }
  const size_t lds = ent_lds_bytes(a.n_feat, a.n_col, a.rows);
  if (lds > (size_t)ENT_LDS_BYTES) return -4;
  int rc;
  if (a.rows == 256) rc = launch_rows<256>(stream, a, lds);
  else if (a.rows == 128) rc = launch_rows<128>(stream, a, lds);
  else rc = launch_rows<64>(stream, a, lds);
  if (rc) return rc;
  return hipGetLastError() == hipSuccess ? 0 : -7;
}
