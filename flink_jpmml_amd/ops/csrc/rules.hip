// Association rules of a batch of baskets, ranked per row (gfx950 / CDNA4, wave64).
//
// One lane owns one row. The workgroup stages its TB rows as [F][TB] fp32 planes in LDS with the
// MiningField preparation applied (common.h::stage_rows_T, the helper cluster.hip calls); a row the
// preparation rejects gets NaN in every rule column. Each lane then builds its basket: a bit set
// over the model's items, one bit per distinct item value. A field contributes the item its value
// names: a table over the vocabulary codes of a string field, an exact search in the sorted fp32
// values of a numeric field; a missing value and a value that names no item set nothing.
//
//   REG  (<= 128 items): the 4 basket words live in registers, indexed by unrolled selects only.
//   !REG (<= 1024 items): the words live in the lane's own LDS column [W][TB] (lane-strided:
//        conflict free whatever word each lane touches).
//
// Itemsets are word-sparse lists of {word, mask} pairs, so a two-item antecedent among 1024 items
// costs one or two tests. The rule tables are read at wave-uniform addresses (scalar loads).
// Per scan group (algorithm, rankBasis, rankOrder) the rules are walked in the order the host sorted
// them with the oracle's key, one 16-byte record per step at consecutive addresses (the rule's index
// and the pair ranges of its two itemsets, so a step chases nothing but the pairs themselves).
// The r-th match IS the rank-r rule: its index is kept in an unrolled
// register chain of R slots, and the walk ends as soon as no lane of the wave still lacks a match
// the group's columns ask for. Column j of a row is tables[off_j + rule index], entry n_rules (NaN)
// when the row has fewer matches. Only those columns of the [n, ldo] matrix are written.
#include "common.h"

struct RuleArgs {
  const float* X;          // [n_rows, ldx] raw rows
  const FieldPrep* prep;   // [n_feat] or null
  const int4* fields;      // [n_feat] {kind, imap offset, count, nvals offset}
  const int* imap;         // item index (or -1) per vocabulary code / per sorted numeric value
  const float* nvals;      // sorted fp32 item values of the numeric fields
  const uint2* pairs;      // [n_pair] {basket word, mask}
  const int4* scan;        // [n_group][n_rules] best rank first: {rule index, first antecedent pair,
                           // first consequent pair, antecedent pairs | consequent pairs << 8}
  const int2* groups;      // [n_group] {algorithm, ranks its columns need}
  const int4* cols;        // [n_col] {group, rank (0-based), table offset, destination column}
  const float* tables;     // [n_tables] per column: n_rules values and a NaN
  float* out;              // [n_rows, ldo]
  int n_rows, n_feat, ldx, ldo;
  int n_items, n_rules, n_group, n_col;
  int k, rows, n_tables, n_pair;
  int n_map, n_vals, pad0, pad1;
};

namespace {

enum : int { ALG_RECOMMENDATION = 0, ALG_EXCLUSIVE = 1, ALG_ASSOCIATION = 2 };
enum : int { FIELD_NONE = 0, FIELD_CODES = 1, FIELD_VALUES = 2 };

constexpr int RL_MAX_ITEMS = 1024;
constexpr int RL_MAX_RULES = 4096;
constexpr int RL_MAX_FIELDS = 128;
constexpr int RL_MAX_RANK = 8;
constexpr int RL_MAX_GROUPS = 4;
constexpr int RL_MAX_COLS = 64;
constexpr int RL_REG_WORDS = 4;
constexpr int RL_LDS_BYTES = 64 * 1024;  // one workgroup's request: two workgroups share a CU

// The register basket: RL_REG_WORDS named words, never an indexed array (that would be scratch).
struct RegBasket {
  uint32_t w0, w1, w2, w3;
};

// Word w of this lane's basket. w is wave uniform.
template <int TB, bool REG>
__device__ __forceinline__ uint32_t rl_word(const RegBasket& b, const uint32_t* lane, uint32_t w) {
  if (REG) return w == 0u ? b.w0 : (w == 1u ? b.w1 : (w == 2u ? b.w2 : b.w3));
  return lane[w * TB];
}

// The itemset (count pairs from first) is a subset of the basket; an empty itemset is a subset of
// everything.
template <int TB, bool REG>
__device__ __forceinline__ bool rl_subset(const RuleArgs& a, const RegBasket& b, const uint32_t* lane, int first,
                                          int count) {
  bool r = true;
  for (int p = 0; p < count; ++p) {
    const uint2 pr = a.pairs[first + p];
    r &= (rl_word<TB, REG>(b, lane, pr.x) & pr.y) == pr.y;
  }
  return r;
}

template <int TB, int R, bool REG>
__global__ __launch_bounds__(TB) void rules_kernel(RuleArgs a) {
  extern __shared__ __attribute__((aligned(16))) char rl_smem[];
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * TB;
  const int row = row0 + tid;
  const int F = a.n_feat;
  const int W = (a.n_items + 31) >> 5;
  float* feat = reinterpret_cast<float*>(rl_smem);            // [F][TB]
  int* bad = reinterpret_cast<int*>(feat + (size_t)F * TB);   // [TB]
  uint32_t* lane = reinterpret_cast<uint32_t*>(bad + TB) + tid;  // [W][TB], !REG only
  stage_rows_T<TB>(a.X, a.n_rows, F, a.ldx, a.prep, feat, bad, row0);  // the last barrier
  const bool live = row < a.n_rows;
  const bool ok = live && bad[tid] == 0;

  // the basket
  RegBasket b = {0u, 0u, 0u, 0u};
  if (!REG) {
    for (int w = 0; w < W; ++w) lane[w * TB] = 0u;
  }
  for (int f = 0; f < F; ++f) {
    const int4 fd = a.fields[f];
    if (fd.x == FIELD_NONE) continue;
    const float x = feat[f * TB + tid];
    int item = -1;
    if (fd.x == FIELD_CODES) {
      // the oracle decodes a code with int(): truncation toward zero
      if (x > -1.0f && x < (float)fd.z) item = a.imap[fd.y + (int)x];
    } else {
      int lo = 0, hi = fd.z;  // first value that is not below x
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.nvals[fd.w + mid] < x) lo = mid + 1;
        else hi = mid;
      }
      if (lo < fd.z && a.nvals[fd.w + lo] == x) item = a.imap[fd.y + lo];
    }
    if (item >= 0 && item < a.n_items) {
      const uint32_t w = (uint32_t)item >> 5;
      const uint32_t bit = 1u << (item & 31);
      if (REG) {
        b.w0 |= w == 0u ? bit : 0u;
        b.w1 |= w == 1u ? bit : 0u;
        b.w2 |= w == 2u ? bit : 0u;
        b.w3 |= w == 3u ? bit : 0u;
      } else {
        lane[w * TB] |= bit;
      }
    }
  }

  float* orow = a.out + (size_t)row * a.ldo;
  const float nan = __builtin_nanf("");
  for (int g = 0; g < a.n_group; ++g) {
    const int2 grp = a.groups[g];
    const int4* scan = a.scan + (size_t)g * a.n_rules;
    int m[R];
#pragma unroll
    for (int j = 0; j < R; ++j) m[j] = -1;
    int cnt = 0;
    for (int i = 0; i < a.n_rules; ++i) {
      if (!__any(ok && cnt < grp.y)) break;  // every lane of the wave has the matches its columns read
      const int4 rule = scan[i];  // one sequential record per step: nothing to chase but its pairs
      const int k = rule.x;
      bool hit = ok && rl_subset<TB, REG>(a, b, lane, rule.y, rule.w & 0xFF);
      if (grp.x != ALG_RECOMMENDATION && __any(hit)) {
        const bool inside = rl_subset<TB, REG>(a, b, lane, rule.z, (rule.w >> 8) & 0xFF);  // the WHOLE consequent
        hit = hit && (grp.x == ALG_EXCLUSIVE ? !inside : inside);
      }
      if (hit) {
#pragma unroll
        for (int j = 0; j < R; ++j) if (cnt == j) m[j] = k;
        ++cnt;
      }
    }
    for (int j = 0; j < a.n_col; ++j) {
      const int4 col = a.cols[j];
      if (col.x != g) continue;
      int idx = -1;
#pragma unroll
      for (int r = 0; r < R; ++r) if (col.y == r) idx = m[r];
      float x = nan;
      const long long pos = (long long)col.z + (idx >= 0 ? idx : a.n_rules);
      if (col.z >= 0 && pos < a.n_tables) x = a.tables[pos];
      if (live && col.w >= 0 && col.w < a.ldo) orow[col.w] = x;
    }
  }
}

size_t rl_lds_bytes(int n_feat, int n_items, int rows) {
  const int W = (n_items + 31) / 32;
  return ((size_t)n_feat + 1 + (W > RL_REG_WORDS ? W : 0)) * rows * 4;
}

template <int TB, int R>
void rl_launch_r(const RuleArgs& a, dim3 grid, size_t lds, hipStream_t stream) {
  if ((a.n_items + 31) / 32 <= RL_REG_WORDS)
    hipLaunchKernelGGL((rules_kernel<TB, R, true>), grid, dim3(TB), lds, stream, a);
  else
    hipLaunchKernelGGL((rules_kernel<TB, R, false>), grid, dim3(TB), lds, stream, a);
}

template <int TB>
void rl_launch(const RuleArgs& a, size_t lds, hipStream_t stream) {
  const dim3 grid((a.n_rows + TB - 1) / TB);
  if (a.k == 1) rl_launch_r<TB, 1>(a, grid, lds, stream);
  else if (a.k == 2) rl_launch_r<TB, 2>(a, grid, lds, stream);
  else if (a.k <= 4) rl_launch_r<TB, 4>(a, grid, lds, stream);
  else rl_launch_r<TB, 8>(a, grid, lds, stream);
}

}  // namespace

PMML_API int pmml_rules_args_size() { return (int)sizeof(RuleArgs); }

// LDS request of one workgroup (ops/rules.py mirrors this); -1: not a shape the kernel takes.
PMML_API long long pmml_rules_lds_bytes(int n_feat, int n_items, int rows) {
  if (n_feat < 1 || n_feat > RL_MAX_FIELDS || n_items < 1 || n_items > RL_MAX_ITEMS ||
      (rows != 64 && rows != 128 && rows != 256))
    return -1;
  return (long long)rl_lds_bytes(n_feat, n_items, rows);
}

PMML_API int pmml_rules_launch(hipStream_t stream, const RuleArgs* args) {
  const RuleArgs a = *args;
  if (a.n_rows < 0 || a.n_feat < 1 || a.n_feat > RL_MAX_FIELDS || a.n_items < 1 || a.n_items > RL_MAX_ITEMS) return -1;
  if (a.n_rules < 1 || a.n_rules > RL_MAX_RULES || a.n_group < 1 || a.n_group > RL_MAX_GROUPS) return -1;
  if (a.k < 1 || a.k > RL_MAX_RANK || a.n_col < 1 || a.n_col > RL_MAX_COLS) return -1;
  if (a.n_pair < 0 || a.n_map < 0 || a.n_vals < 0 || a.n_tables < 0) return -1;
  if (a.rows != 64 && a.rows != 128 && a.rows != 256) return -1;
  if (a.n_rows == 0) return 0;
  if (!a.X || !a.fields || !a.imap || !a.nvals || !a.pairs || !a.scan || !a.groups || !a.cols || !a.tables || !a.out)
    return -2;
  if (a.ldx < a.n_feat || a.ldo < 1) return -3;
  const size_t lds = rl_lds_bytes(a.n_feat, a.n_items, a.rows);
  if (lds > (size_t)RL_LDS_BYTES) return -4;
  if (a.rows == 256) rl_launch<256>(a, lds, stream);
  else if (a.rows == 128) rl_launch<128>(a, lds, stream);
  else rl_launch<64>(a, lds, stream);
  return hipGetLastError() == hipSuccess ? 0 : -7;
}
