// What the launchers of the tree WALK kernels share (tree.hip, tree_hybrid.hip, tree_lds.hip): one
// "prepare, then launch" and a runtime-bool-to-template-argument dispatcher. Not included by
// tree_common.h: the per-depth PERFECT units (tree_d<D>.hip) need none of it. Device-side helpers
// of the walks belong here too once they keep registers and speed (profiles/tree_walk_helpers.md).
#pragma once
#include <type_traits>

#include "tree_common.h"

namespace pmml_tree {
namespace {

// ------------------------------------------------------------------------------ launch
template <typename K, typename A>
int launch_k(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A& args) {
  int err = prepare_launch(kernel, lds);
  if (!err) hipLaunchKernelGGL(kernel, grid, block, lds, stream, args);
  return err;
}

// A runtime bool as a template argument: f(std::true_type) or f(std::false_type); nest for two.
template <typename F>
int dispatch_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

}  // namespace
}  // namespace pmml_tree
