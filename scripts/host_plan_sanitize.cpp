// Plan build under host sanitizers: a stand-alone program (not part of
// pytest) that builds and destroys plans over the generated golden fixtures
// for three shapes — the flat c2 query, a WHERE tree with a non-folded OR
// over a column with PLAIN string pages (the contains window build) and a
// group-by on the dictionary-overflow fixture (hash mode). Plan building is
// pure host work, so it runs without a GPU (GPUQ_FAKE_DEVICE).
// Build + run from the repository root (fixtures: run the CPU tests once):
//   cd parseable_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -Xarch_host -fsanitize=address,undefined \
//     ../../scripts/host_plan_sanitize.cpp kernels.hip gpuq.cpp meta.cpp \
//     catalog.cpp -o /tmp/host_plan_sanitize && cd ../.. && \
//   /tmp/host_plan_sanitize tests/golden/data
#include "../include/gpuq.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <string>
#include <vector>

namespace fs = std::filesystem;

static std::vector<std::string> parquet_files(const std::string& dir) {
  std::vector<std::string> out;
  for (auto& e : fs::recursive_directory_iterator(dir))
    if (e.is_regular_file() && e.path().extension() == ".parquet")
      out.push_back(e.path().string());
  std::sort(out.begin(), out.end());
  return out;
}

static gpuq_pred pred(const char* col, int op, int lit_kind) {
  gpuq_pred p{};
  p.column = col;
  p.op = op;
  p.lit_kind = lit_kind;
  return p;
}

static int build(gpuq_ctx* ctx, const char* what, const std::string& dir,
                 std::vector<gpuq_pred> preds,
                 std::vector<const char*> group_by, std::vector<gpuq_agg> aggs,
                 std::vector<gpuq_where_node> nodes) {
  std::vector<std::string> paths = parquet_files(dir);
  std::vector<gpuq_file> files;
  for (auto& p : paths) files.push_back({p.c_str(), nullptr, -1});
  gpuq_plan* plan = gpuq_plan_build_where(
      ctx, files.data(), (int32_t)files.size(), nullptr, 0, preds.data(),
      (int32_t)preds.size(), group_by.data(), (int32_t)group_by.size(),
      aggs.data(), (int32_t)aggs.size(), -1,
      nodes.empty() ? nullptr : nodes.data(), (int32_t)nodes.size());
  if (!plan) {
    fprintf(stderr, "%s: plan build failed: %s\n", what, gpuq_last_error(ctx));
    return 1;
  }
  gpuq_metrics m{};
  gpuq_plan_metrics(plan, &m);
  printf("%s: %zu files, %lld rows planned\n", what, files.size(),
         (long long)m.rows_scanned);
  gpuq_plan_destroy(plan);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <golden data dir>\n", argv[0]);
    return 2;
  }
  setenv("GPUQ_FAKE_DEVICE", "1", 1);
  const std::string root = argv[1];
  gpuq_ctx* ctx = gpuq_session_create(0);
  int bad = 0;

  // flat c2: GROUP BY host, count(*) + max(latency), BETWEEN on p_timestamp
  {
    gpuq_pred ts = pred("p_timestamp", GPUQ_BETWEEN, GPUQ_LIT_I64);
    ts.i64[0] = 1756684800000 + 30000;
    ts.i64[1] = 1756684800000 + 120000;
    ts.hi_exclusive = 1;
    bad += build(ctx, "flat c2", root + "/g_c1", {ts}, {"host"},
                 {{GPUQ_AGG_COUNT_STAR, nullptr}, {GPUQ_AGG_MAX, "latency"}},
                 {});
  }
  // non-folded OR over a column with PLAIN string pages: the window build
  {
    gpuq_pred like = pred("message", GPUQ_CONTAINS, GPUQ_LIT_STR);
    like.str = "error";
    gpuq_pred lt = pred("latency", GPUQ_LT, GPUQ_LIT_I64);
    lt.i64[0] = 1000;
    bad += build(ctx, "where tree (window build)", root + "/g_c3", {like, lt},
                 {"level"}, {{GPUQ_AGG_COUNT_STAR, nullptr}},
                 {{GPUQ_NODE_OR, -1, -1},
                  {GPUQ_NODE_LEAF, 0, 0},
                  {GPUQ_NODE_LEAF, 0, 1}});
  }
  // group-by on the dictionary-overflow fixture: hash mode
  bad += build(ctx, "hash-mode group-by", root + "/g_c5", {}, {"trace"},
               {{GPUQ_AGG_COUNT_STAR, nullptr}, {GPUQ_AGG_MAX, "latency"}},
               {});

  gpuq_session_destroy(ctx);
  return bad ? 1 : 0;
}
