// Tree ensembles with 17 to 256 class slots (runtime/class_forest.py, ClassForestPlan): forests of
// votes or class-probability leaves and K-class boosted chains past the 16 accumulators of the
// other tree kernels, whose C x 256 LDS accumulators would need 256 KiB at 256 classes.
//
// Classes AND rows are tiled: a 256-thread workgroup owns 64 rows. LDS:
//   feat [Fs][64]     the prepared columns the trees read (feat_map, Fs <= 256)
//   acc  [Cp][64]     fp32 class accumulators, Cp = C rounded up to 16 (each class quarter is whole
//                     float4s of a DENSE leaf row), at most 64 KiB
//   hits [2][32][64]  leaf ids of one chunk of 32 trees, double buffered
//   bad  [64]         rows their preparation rejects
// Per chunk of 32 trees, two phases and ONE barrier between them:
//  1. walk: wave w takes trees 8w .. 8w+7 of the chunk, lane l is row l; the eight walks run in
//     lock-step over the 16-byte pointer nodes {T bits, meta, left, right} (tree.hip::pointer_walk's
//     node step: features from LDS, nodes gathered from L2, finished walks re-load node 0). A walk
//     stores its leaf id in hits, or -1 when a null-on-missing tree met a missing value.
//  2. accumulate: thread t is row t & 63 and class quarter t >> 6 (classes [q Cp/4, (q+1) Cp/4)).
//     It reads its row's hits in tree order and adds into its quarter's cells only:
//       PAIR leaves  one 8-byte {slot, value} gather per hit (a vote: {class, tree weight}; a chain
//                    tree: {its class slot, weight x leaf}); slot < 0: a leaf without a class;
//       DENSE leaves its Cp / 4 floats of the leaf's (weight-scaled) probability row, as float4s.
//     Every accumulator cell has one owner and one order: results are reproducible bit for bit.
//     The next chunk's walks write the other hit buffer, which every thread finished reading
//     before it passed this chunk's barrier.
// After the last chunk threads 0 .. 63 run the shared epilogue over acc[c * 64 + row].
// No matrix instructions: a gather-and-compare walk, nothing in it is a product.
#include "tree_walk.h"

namespace pmml_tree {

struct ClassTreeArgs {
  const float* X;
  int n_rows, n_feat, ldx, n_stage;
  const FieldPrep* prep;        // nullable
  const uint8_t* row_valid_in;  // nullable
  const int* feat_map;          // [n_stage] staged column j -> X column
  const uint4* nodes;           // pointer nodes; meta & 0xFFFF = staged column * 256 (its plane's byte offset)
  const int* roots;             // [n_trees] root code (>= 0 node, < 0 ~leaf)
  const void* leaves;           // PAIR: int2 [n_leaves] {slot, value bits}; DENSE: float [n_leaves][Cp]
  const float* acc_init;        // nullable: [C] initial accumulators (chain intercepts)
  int n_trees, C, Cp, dense;
  Epilogue epi;
  float* score;
  uint8_t* valid;
  float* probs;
};

namespace {

constexpr int CR = 64;      // rows per workgroup
constexpr int CCHUNK = 32;  // trees per chunk
constexpr int CW = 8;       // lock-step walks per lane
constexpr int CLS_MAX = 256, CLS_STAGE_MAX = 256;

constexpr size_t class_lds_bytes(int n_stage, int Cp) {
  return (size_t)(n_stage + Cp) * CR * 4 + 2 * CCHUNK * CR * 4 + CR * 4;
}

template <bool DENSE>
__global__ __launch_bounds__(TB) void tree_classes_kernel(ClassTreeArgs a) {
  extern __shared__ __align__(16) uint32_t smem[];
  float* feat = reinterpret_cast<float*>(smem);
  float* acc = feat + a.n_stage * CR;
  int* hits = reinterpret_cast<int*>(acc + a.Cp * CR);
  int* bad = hits + 2 * CCHUNK * CR;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * CR;

  if (tid < CR) bad[tid] = 0;
  for (int e = tid; e < a.Cp * CR; e += TB) {
    const int c = e >> 6;
    acc[e] = (a.acc_init && c < a.C) ? a.acc_init[c] : 0.f;
  }
  __syncthreads();
  // stage [Fs][64] with field preparation: 64 consecutive rows of one plane per wave (distinct
  // banks); rows past the end are zero (never "missing")
  for (int e = tid; e < a.n_stage * CR; e += TB) {
    const int f = e >> 6;
    const int r = e & 63;
    const int row = row0 + r;
    float x = 0.f;
    bool b = false;
    if (row < a.n_rows) {
      const int col = a.feat_map[f];
      x = a.X[(size_t)row * a.ldx + col];
      if (a.prep) x = prep_value(x, a.prep[col], &b);
    }
    feat[e] = x;
    if (b) bad[r] = 1;
  }
  __syncthreads();

  const char* feat_lane = reinterpret_cast<const char*>(feat + lane);
  const int Cq = a.Cp >> 2;   // classes per quarter (a multiple of 4)
  const int c_lo = wave * Cq;  // this thread's quarter (wave-uniform)
  bool voided = false;
  int chunk = 0;
  for (int t0 = 0; t0 < a.n_trees; t0 += CCHUNK, ++chunk) {
    const int nt = min(CCHUNK, a.n_trees - t0);
    int* hb = hits + (chunk & 1) * CCHUNK * CR;
    // ---- walk: this wave's eight trees of the chunk, in lock-step
    const int k0 = wave * CW;
    if (k0 < nt) {
      int code[CW];
      bool pz[CW];
#pragma unroll
      for (int i = 0; i < CW; ++i) {
        code[i] = k0 + i < nt ? a.roots[t0 + k0 + i] : -1;
        pz[i] = false;
      }
      bool live = true;
      while (live) {
        uint4 nd[CW];
#pragma unroll
        for (int i = 0; i < CW; ++i) nd[i] = a.nodes[max(code[i], 0)];
        live = false;
#pragma unroll
        for (int i = 0; i < CW; ++i) {  // branch-free: finished walks compute on node 0 and keep their leaf
          const bool act = code[i] >= 0;
          const float x = *reinterpret_cast<const float*>(feat_lane + (nd[i].y & 0xFFFFu));
          const bool isn = (x != x);
          const bool nulled = act && isn && ((nd[i].y >> 30) & 1u);  // null prediction: the walk ends
          const bool right = (x >= __uint_as_float(nd[i].x)) || (isn && (nd[i].y >> 31));
          const int nc = right ? (int)nd[i].w : (int)nd[i].z;
          pz[i] = pz[i] || nulled;
          code[i] = act ? (nulled ? -1 : nc) : code[i];
          live = live || code[i] >= 0;
        }
      }
#pragma unroll
      for (int i = 0; i < CW; ++i)
        if (k0 + i < nt) hb[(k0 + i) * CR + lane] = pz[i] ? -1 : ~code[i];
    }
    __syncthreads();
    // ---- accumulate: this row's hits in tree order, into this thread's class quarter
    for (int k = 0; k < nt; ++k) {
      const int h = hb[k * CR + lane];
      if (h < 0) {
        voided = true;
        continue;
      }
      if (DENSE) {
        const float4* lp = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(a.leaves) +
                                                           (size_t)h * a.Cp + c_lo);
        for (int j = 0; j < (Cq >> 2); ++j) {
          const float4 v = lp[j];
          float* cell = acc + (c_lo + 4 * j) * CR + lane;
          cell[0] += v.x;
          cell[CR] += v.y;
          cell[2 * CR] += v.z;
          cell[3 * CR] += v.w;
        }
      } else {
        const int2 lv = reinterpret_cast<const int2*>(a.leaves)[h];
        if (lv.x < 0) voided = true;  // a leaf without a class: the tree has no prediction
        else if (lv.x >= c_lo && lv.x < c_lo + Cq) acc[lv.x * CR + lane] += __int_as_float(lv.y);
      }
    }
  }
  __syncthreads();
  // quarter 0's threads saw every hit of their row: their verdict is the row's
  const int row = row0 + tid;
  if (tid < CR && row < a.n_rows) {
    bool row_ok = bad[tid] == 0 && !voided;
    if (a.row_valid_in) row_ok = row_ok && a.row_valid_in[row];
    apply_epilogue(a.epi, [&](int c) { return acc[c * CR + tid]; }, row_ok, row, a.n_rows, a.score, a.valid,
                   a.probs);
  }
}

}  // namespace
}  // namespace pmml_tree

using namespace pmml_tree;

PMML_API int pmml_tree_classes_args_size() { return (int)sizeof(ClassTreeArgs); }

// 0, a HIP error code, or: -2 bad sizes, -3 class count, -4 staged columns, -5 LDS, -7 launch.
PMML_API int pmml_tree_classes_launch(hipStream_t stream, const ClassTreeArgs* args) {
  const ClassTreeArgs& a = *args;
  if (a.n_rows <= 0) return 0;
  if (a.n_trees < 1 || a.n_feat < 1 || a.ldx < a.n_feat || !a.nodes || !a.roots || !a.leaves || !a.feat_map) return -2;
  if (a.C < 1 || a.C > CLS_MAX || a.Cp < a.C || a.Cp > CLS_MAX || (a.Cp & 15) || a.epi.n_classes > a.C) return -3;
  if (a.n_stage < 1 || a.n_stage > CLS_STAGE_MAX) return -4;
  const size_t lds = class_lds_bytes(a.n_stage, a.Cp);
  if (lds > 160 * 1024) return -5;
  dim3 grid((a.n_rows + CR - 1) / CR);
  const int err = a.dense ? launch_k(tree_classes_kernel<true>, grid, dim3(TB), lds, stream, a)
                          : launch_k(tree_classes_kernel<false>, grid, dim3(TB), lds, stream, a);
  if (err) return err;
  return hipGetLastError() == hipSuccess ? 0 : -7;
}
