// Stand-alone host check of the WHERE-tree / aggregate-filter validation
// (parseable_amd/csrc/where.h). CPU only: no HIP, no GPU, no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       scripts/aggfilter_host_check.cpp -o /tmp/aggfilter_host_check && \
//       /tmp/aggfilter_host_check
//
// Feeds where_normalise_filtered the malformed arrays the plan builders must
// refuse and a few well-formed ones. Every node list lives in an exactly
// sized heap buffer, so a read before or after it is an AddressSanitizer
// report. Exits non-zero when a case is not refused with the expected
// message, or a good one is refused.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../parseable_amd/csrc/where.h"

using namespace gpuq;

namespace {

enum { LEAF = GPUQ_NODE_LEAF, AND = GPUQ_NODE_AND, OR = GPUQ_NODE_OR };
using Nodes = std::vector<gpuq_where_node>;
struct Filter { int agg; Nodes nodes; };

int failures = 0;

std::unique_ptr<gpuq_where_node[]> exact(const Nodes& n) {
  std::unique_ptr<gpuq_where_node[]> p(new gpuq_where_node[n.size()]);
  if (!n.empty()) memcpy(p.get(), n.data(), n.size() * sizeof(gpuq_where_node));
  return p;
}

// expect == nullptr: must build; else the message must contain it
QueryTrees run(const char* name, const Nodes& where, int n_preds,
               const std::vector<Filter>& filters, int n_aggs, bool projection,
               const char* expect) {
  auto w = exact(where);
  std::vector<std::unique_ptr<gpuq_where_node[]>> keep;
  std::unique_ptr<gpuq_agg_filter[]> cf(new gpuq_agg_filter[filters.size()]);
  for (size_t j = 0; j < filters.size(); j++) {
    keep.push_back(exact(filters[j].nodes));
    cf[j].agg = filters[j].agg;
    cf[j].nodes = keep.back().get();
    cf[j].n_nodes = (int32_t)filters[j].nodes.size();
  }
  QueryTrees q;
  std::string got;
  try {
    q = where_normalise_filtered(where.empty() ? nullptr : w.get(),
                                 (int32_t)where.size(), n_preds, cf.get(),
                                 (int32_t)filters.size(), n_aggs, projection);
  } catch (const std::exception& e) {
    got = e.what();
    if (got.empty()) got = "?";
  }
  bool ok = expect ? got.find(expect) != std::string::npos : got.empty();
  if (!ok) {
    failures++;
    fprintf(stderr, "FAIL %s: expected %s, got %s\n", name,
            expect ? expect : "a plan", got.empty() ? "a plan" : got.c_str());
  }
  return q;
}

Nodes one(int pred) { return {{LEAF, -1, pred}}; }

// OR(leaf, AND(leaf, OR(...))) with n_or OR levels over preds first..
Nodes or_chain(int n_or, int first, int* n_preds) {
  Nodes n;
  int parent = -1, p = first;
  for (int d = 0; d < n_or; d++) {
    n.push_back({OR, parent, -1});
    int o = (int)n.size() - 1;
    n.push_back({LEAF, o, p++});
    n.push_back({AND, o, -1});
    int a = (int)n.size() - 1;
    n.push_back({LEAF, a, p++});
    parent = a;
  }
  n.push_back({LEAF, parent, p++});
  *n_preds = p;
  return n;
}

}  // namespace

int main() {
  run("bad agg index", one(0), 2, {{2, one(1)}}, 2, false, "agg index out of range");
  run("negative agg", one(0), 2, {{-1, one(1)}}, 2, false, "agg index out of range");
  run("two filters on one agg", one(0), 3, {{1, one(1)}, {1, one(2)}}, 2, false,
      "already has a filter");
  run("pred shared with where", {{AND, -1, -1}, {LEAF, 0, 0}, {LEAF, 0, 1}}, 2,
      {{0, one(1)}}, 2, false, "more than one leaf");
  run("pred shared by two filters", one(0), 2, {{0, one(1)}, {1, one(1)}}, 2,
      false, "more than one leaf");
  run("unused pred", one(0), 3, {{0, one(1)}}, 2, false, "used by no leaf");
  run("childless group in a filter", one(0), 2,
      {{0, {{AND, -1, -1}, {LEAF, 0, 1}, {OR, 0, -1}}}}, 2, false,
      "at least one condition or group");
  run("empty filter tree", one(0), 1, {{0, {}}}, 1, false, "at least one node");
  run("filter root with a parent", one(0), 2, {{0, {{LEAF, 0, 1}}}}, 1, false,
      "parent must be -1");
  run("filter pred out of range", one(0), 1, {{0, one(1)}}, 1, false,
      "names no predicate");
  run("forward parent in a filter", one(0), 3,
      {{0, {{OR, -1, -1}, {LEAF, 2, 1}, {LEAF, 0, 2}}}}, 1, false,
      "malformed parent link");
  run("filter with a projection", {}, 1, {{0, one(0)}}, 1, true,
      "not allowed in a projection plan");
  {
    // 33 leaves over WHERE and one filter; 32 build; also with the implied WHERE
    Nodes where{{AND, -1, -1}};
    for (int i = 0; i < 20; i++) where.push_back({LEAF, 0, i});
    Nodes f33{{OR, -1, -1}}, f32{{OR, -1, -1}};
    for (int i = 20; i < 33; i++) f33.push_back({LEAF, 0, i});
    for (int i = 20; i < 32; i++) f32.push_back({LEAF, 0, i});
    run("33 leaves", where, 33, {{0, f33}}, 1, false, "more than 32 leaves");
    run("32 leaves", where, 32, {{0, f32}}, 1, false, nullptr);
    run("33 leaves, implied where", {}, 33, {{0, f33}}, 1, false,
        "more than 32 leaves");
    QueryTrees q = run("32 leaves, implied where", {}, 32, {{0, f32}}, 1, false,
                       nullptr);
    if (q.where.root_leaves.size() != 20 || !q.where.conj) {
      failures++;
      fprintf(stderr, "FAIL implied where: %zu root leaves\n",
              q.where.root_leaves.size());
    }
  }
  {
    int np = 0, np2 = 0;
    Nodes w = or_chain(4, 0, &np);
    Nodes f5 = or_chain(5, np, &np2);
    run("OR depth 5 in a filter", w, np2, {{0, f5}}, 1, false,
        "OR nesting depth above 4");
    Nodes f4 = or_chain(4, np, &np2);
    QueryTrees q = run("OR depth 4 in a filter", w, np2, {{0, f4}}, 1, false,
                       nullptr);
    if (q.filters.size() != 1 || q.filters[0].tree.depth != 4) failures++;
    // the forest: appended nodes keep their shape, the WHERE root its span
    WhereTree forest = q.where;
    const size_t before = forest.nodes.size();
    int root = where_append(forest, q.filters[0].tree);
    if (forest.root != q.where.root ||
        forest.nodes.size() != before + q.filters[0].tree.nodes.size() ||
        where_expr(forest, root) != where_expr(q.filters[0].tree,
                                               q.filters[0].tree.root)) {
      failures++;
      fprintf(stderr, "FAIL where_append\n");
    }
  }
  {
    // eight filters, one per aggregate; a single-leaf filter is wrapped
    std::vector<Filter> fs;
    for (int i = 0; i < 8; i++) fs.push_back({i, one(i)});
    QueryTrees q = run("eight filters", {}, 8, fs, 8, false, nullptr);
    if (q.filters.size() != 8 || !q.where.root_leaves.empty()) failures++;
    for (auto& f : q.filters)
      if (f.tree.nodes[f.tree.root].kind != AND || !f.tree.conj) failures++;
  }
  run("no filters: the where tree alone", {{OR, -1, -1}, {LEAF, 0, 0}, {LEAF, 0, 1}},
      2, {}, 1, false, nullptr);
  if (failures) {
    fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  printf("aggfilter_host_check OK\n");
  return 0;
}
