// WHERE trees: validation and normalisation of the gpuq_where_node list
// (include/gpuq.h) — the AND/OR groups of the reference's filter builder
// (Conditions, alerts/alert_structs.rs:195-203; get_filter_string,
// alerts/alerts_utils.rs:390-424). Shared by the scan planner (gpuq.cpp) and
// the catalog planner (catalog.cpp) so both see the same normal form.
#pragma once
#include "../../include/gpuq.h"
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace gpuq {

constexpr int WHERE_MAX_LEAVES = 32;
constexpr int WHERE_MAX_OR_DEPTH = 4;

struct WNode {
  int kind = GPUQ_NODE_LEAF;  // gpuq_node_kind
  int pred = -1;              // LEAF: index into preds
  std::vector<int> kids;      // AND / OR: indices into WhereTree::nodes
};

// Normal form: the root is an AND, no child has its parent's kind, no group
// has a single child. `conj` marks a pure conjunction — the flat predicate
// list every plan had before trees existed; planners then take exactly the
// flat path.
struct WhereTree {
  std::vector<WNode> nodes;
  int root = -1;
  bool conj = true;
  int depth = 0;                 // OR nesting depth
  std::vector<int> root_leaves;  // preds that are conjuncts of the root
};

namespace where_detail {
inline int norm(const std::vector<std::vector<int>>& kids_in,
                const gpuq_where_node* in, int i, WhereTree& t) {
  if (in[i].kind == GPUQ_NODE_LEAF) {
    WNode n;
    n.pred = in[i].pred;
    t.nodes.push_back(n);
    return (int)t.nodes.size() - 1;
  }
  std::vector<int> kids;
  for (int c : kids_in[i]) {
    int k = norm(kids_in, in, c, t);
    if (t.nodes[k].kind == in[i].kind)  // same kind as the parent: flatten
      kids.insert(kids.end(), t.nodes[k].kids.begin(), t.nodes[k].kids.end());
    else
      kids.push_back(k);
  }
  if (kids.size() == 1) return kids[0];  // single-child group collapses
  WNode n;
  n.kind = in[i].kind;
  n.kids = std::move(kids);
  t.nodes.push_back(std::move(n));
  return (int)t.nodes.size() - 1;
}
// copy the subtree below `i` into `out` (children before parents)
inline int compact(const std::vector<WNode>& in, int i, std::vector<WNode>& out) {
  WNode n = in[i];
  for (int& k : n.kids) k = compact(in, k, out);
  out.push_back(std::move(n));
  return (int)out.size() - 1;
}
inline int or_depth(const WhereTree& t, int i) {
  const WNode& n = t.nodes[i];
  int d = 0;
  for (int k : n.kids) d = std::max(d, or_depth(t, k));
  return d + (n.kind == GPUQ_NODE_OR ? 1 : 0);
}
}  // namespace where_detail

namespace where_detail {
// One tree of a query (the WHERE tree or an aggregate's filter tree): `used`
// counts the leaves naming each pred and `leaves` the leaves seen, both
// across all trees of the query. n_nodes == 0: the AND of the preds no tree
// has used so far.
inline WhereTree normalise_one(const gpuq_where_node* in, int32_t n_nodes,
                               int32_t n_preds, std::vector<int>& used,
                               int& leaves) {
  WhereTree t;
  if (n_nodes < 0 || (n_nodes > 0 && !in))
    throw std::runtime_error("where: bad node list");
  if (n_nodes == 0) {
    WNode r;
    r.kind = GPUQ_NODE_AND;
    for (int p = 0; p < n_preds; p++) {
      if (used[p]++) continue;
      WNode l;
      l.pred = p;
      t.nodes.push_back(l);
      r.kids.push_back((int)t.nodes.size() - 1);
      t.root_leaves.push_back(p);
      leaves++;
    }
    t.nodes.push_back(r);
    t.root = (int)t.nodes.size() - 1;
    return t;
  }
  std::vector<std::vector<int>> kids(n_nodes);
  for (int i = 0; i < n_nodes; i++) {
    const auto& n = in[i];
    if (n.kind < GPUQ_NODE_LEAF || n.kind > GPUQ_NODE_OR)
      throw std::runtime_error("where: unknown node kind at node " +
                               std::to_string(i));
    if (i == 0) {
      if (n.parent != -1)
        throw std::runtime_error("where: node 0 is the root, its parent must be -1");
    } else {
      if (n.parent < 0 || n.parent >= i)
        throw std::runtime_error("where: malformed parent link at node " +
                                 std::to_string(i) +
                                 " (0 <= parent < own index)");
      if (in[n.parent].kind == GPUQ_NODE_LEAF)
        throw std::runtime_error("where: parent of node " + std::to_string(i) +
                                 " is a leaf (must be AND or OR)");
      kids[n.parent].push_back(i);
    }
    if (n.kind == GPUQ_NODE_LEAF) {
      if (n.pred < 0 || n.pred >= n_preds)
        throw std::runtime_error("where: leaf " + std::to_string(i) +
                                 " names no predicate");
      if (used[n.pred]++)
        throw std::runtime_error("where: predicate " + std::to_string(n.pred) +
                                 " is used by more than one leaf");
      leaves++;
    }
  }
  for (int i = 0; i < n_nodes; i++)
    if (in[i].kind != GPUQ_NODE_LEAF && kids[i].empty())
      throw std::runtime_error(
          "where: conditions must have at least one condition or group "
          "(childless group at node " + std::to_string(i) + ")");
  if (leaves > WHERE_MAX_LEAVES)
    throw std::runtime_error("where: more than 32 leaves");
  int r = where_detail::norm(kids, in, 0, t);
  if (t.nodes[r].kind != GPUQ_NODE_AND) {  // a non-AND root is wrapped
    WNode w;
    w.kind = GPUQ_NODE_AND;
    w.kids.push_back(r);
    t.nodes.push_back(w);
    r = (int)t.nodes.size() - 1;
  }
  // flattening and collapsing leave nodes behind that nothing refers to:
  // keep the reachable ones only, so that walking `nodes` is walking the tree
  {
    std::vector<WNode> kept;
    r = where_detail::compact(t.nodes, r, kept);
    t.nodes = std::move(kept);
  }
  t.root = r;
  for (int k : t.nodes[r].kids) {
    if (t.nodes[k].kind == GPUQ_NODE_LEAF) t.root_leaves.push_back(t.nodes[k].pred);
    else t.conj = false;
  }
  t.depth = where_detail::or_depth(t, r);
  if (t.depth > WHERE_MAX_OR_DEPTH)
    throw std::runtime_error("where: OR nesting depth above 4");
  return t;
}
inline void check_all_used(const std::vector<int>& used) {
  for (size_t p = 0; p < used.size(); p++)
    if (!used[p])
      throw std::runtime_error("where: predicate " + std::to_string(p) +
                               " is used by no leaf");
}
}  // namespace where_detail

// n_nodes == 0: the AND of all preds. Throws std::runtime_error on every
// malformed input (see gpuq_plan_build_where).
inline WhereTree where_normalise(const gpuq_where_node* in, int32_t n_nodes,
                                 int32_t n_preds) {
  std::vector<int> used(std::max(n_preds, 0), 0);
  int leaves = 0;
  WhereTree t = where_detail::normalise_one(in, n_nodes, n_preds, used, leaves);
  where_detail::check_all_used(used);
  return t;
}

// A query's WHERE tree plus one filter tree per filtered aggregate
// (gpuq_agg_filter): all leaves index the one preds array, every pred is
// used by exactly one leaf of exactly one tree, and the 32-leaf cap holds
// for all trees together. With n_nodes == 0 WHERE is the AND of the preds
// no filter uses. Filter trees take the same normal form as WHERE.
struct FilterTree { int agg = -1; WhereTree tree; };
struct QueryTrees {
  WhereTree where;
  std::vector<FilterTree> filters;
};
inline QueryTrees where_normalise_filtered(
    const gpuq_where_node* in, int32_t n_nodes, int32_t n_preds,
    const gpuq_agg_filter* filters, int32_t n_filters, int32_t n_aggs,
    bool projection) {
  QueryTrees q;
  if (n_filters < 0 || (n_filters > 0 && !filters))
    throw std::runtime_error("filter: bad filter list");
  if (n_filters > 0 && projection)
    throw std::runtime_error(
        "filter: an aggregate filter is not allowed in a projection plan");
  std::vector<int> used(std::max(n_preds, 0), 0);
  int leaves = 0;
  if (n_nodes != 0)
    q.where = where_detail::normalise_one(in, n_nodes, n_preds, used, leaves);
  std::vector<char> seen(std::max(n_aggs, 0), 0);
  for (int j = 0; j < n_filters; j++) {
    const auto& f = filters[j];
    if (f.agg < 0 || f.agg >= n_aggs)
      throw std::runtime_error("filter " + std::to_string(j) +
                               ": agg index out of range");
    if (seen[f.agg]++)
      throw std::runtime_error("filter " + std::to_string(j) +
                               ": aggregate " + std::to_string(f.agg) +
                               " already has a filter");
    if (f.n_nodes < 1)
      throw std::runtime_error("filter " + std::to_string(j) +
                               ": a filter tree needs at least one node");
    FilterTree ft;
    ft.agg = f.agg;
    ft.tree = where_detail::normalise_one(f.nodes, f.n_nodes, n_preds, used,
                                          leaves);
    q.filters.push_back(std::move(ft));
  }
  if (n_nodes == 0)
    q.where = where_detail::normalise_one(nullptr, 0, n_preds, used, leaves);
  if (n_filters > 0 && leaves > WHERE_MAX_LEAVES)
    throw std::runtime_error("where: more than 32 leaves");
  where_detail::check_all_used(used);
  return q;
}

// Appends `src` to `dst.nodes` (a forest: nothing of dst refers to the new
// nodes) and returns the index of src's root there. The planners' tree walks
// (LUT folding, context assignment) then serve filter trees unchanged, while
// everything that starts at dst.root — pruning above all — sees WHERE alone.
inline int where_append(WhereTree& dst, const WhereTree& src) {
  const int base = (int)dst.nodes.size();
  for (WNode n : src.nodes) {
    for (int& k : n.kids) k += base;
    dst.nodes.push_back(std::move(n));
  }
  return base + src.root;
}

// Pruning as a tree evaluation. leaf_none(pred) says "no row of this file /
// row group can satisfy the leaf". An AND is NONE if any child is, an OR
// only if every child is.
template <class F>
bool where_none(const WhereTree& t, int i, F&& leaf_none) {
  const WNode& n = t.nodes[i];
  if (n.kind == GPUQ_NODE_LEAF) return leaf_none(n.pred);
  if (n.kind == GPUQ_NODE_AND) {
    for (int k : n.kids)
      if (where_none(t, k, leaf_none)) return true;
    return false;
  }
  for (int k : n.kids)
    if (!where_none(t, k, leaf_none)) return false;
  return true;
}

// "0 AND (1 OR (2 AND 3))": the normalised expression over pred indices
inline std::string where_expr(const WhereTree& t, int i, bool top = true) {
  const WNode& n = t.nodes[i];
  if (n.kind == GPUQ_NODE_LEAF) return std::to_string(n.pred);
  std::string s;
  for (size_t k = 0; k < n.kids.size(); k++) {
    if (k) s += n.kind == GPUQ_NODE_AND ? " AND " : " OR ";
    s += where_expr(t, n.kids[k], false);
  }
  return top ? s : "(" + s + ")";
}

}  // namespace gpuq
