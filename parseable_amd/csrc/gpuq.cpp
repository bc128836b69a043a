// gpuq host runtime: the C-ABI behind include/gpuq.h.
//
// Replaces the reference's DataFusion physical-plan execution for
// filter/aggregate scans: plan building mirrors
// StandardTableProvider::scan (stream_schema_provider.rs:616-753) — row-group
// pruning via footer min/max stats (the row-group analog of
// can_be_pruned/satisfy_constraints, :1049-1137), byte-balanced shard
// assignment (balanced_file_groups, :146-165) — and execution mirrors the
// DataSourceExec -> FilterExec -> AggregateExec(Partial) pipeline
// (SURVEY.md §3a step 7), with the per-row work on the GPU and the
// Partial->Final merge left to the caller (one RCCL reduce across GPUs).
#include "../../include/gpuq.h"
#include "catalog.h"
#include "where.h"
#include "meta.h"
#include "kernels_api.h"
#include "dev_types.h"
#include "like.h"

#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <functional>
#include <cstring>
#include <thread>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

using namespace gpuq;

#define HIP_TRY(call)                                                        \
  do {                                                                       \
    hipError_t _e = (call);                                                  \
    if (_e != hipSuccess)                                                    \
      throw std::runtime_error(std::string("HIP error: ") +                  \
                               hipGetErrorString(_e) + " at " #call);        \
  } while (0)

// ------------------------------------------------------------------
struct gpuq_ctx {
  std::vector<int> devices;
  std::mutex mu;
  std::string last_error;
  void set_error(const std::string& e) {
    std::lock_guard<std::mutex> g(mu);
    last_error = e;
  }
  // Cross-query GPU-resident hot tier (keyed like the
  // reference's hot tier keys files, hottier.rs:1405-1417): decompressed
  // chunk images cached in HBM per (path, size, mtime, row group, column).
  // A later plan over the same chunks skips the raw upload, the host LZ4
  // structure walk AND the device decompression — repeat queries start
  // from the decompressed arena at HBM rates. LRU eviction under
  // GPUQ_HOT_TIER_BYTES (default 64 GB); entries pinned while a live plan
  // references them.
  struct CacheEntry {
    void* dev = nullptr;
    size_t bytes = 0;
    int device = -1;
    uint64_t last_use = 0;
    int refs = 0;
  };
  std::mutex cache_mu;
  std::unordered_map<std::string, CacheEntry> cache;
  size_t cache_bytes = 0;
  size_t cache_budget = 64ull << 30;
  uint64_t cache_clock = 0;
  int64_t cache_hits_bytes_total = 0;
  gpuq_ctx() {
    if (const char* e = getenv("GPUQ_HOT_TIER_BYTES"))
      cache_budget = strtoull(e, nullptr, 10);
  }
  ~gpuq_ctx() {
    for (auto& kv : cache)
      if (kv.second.dev) {
        (void)hipSetDevice(kv.second.device);
        (void)hipFree(kv.second.dev);
      }
  }
  // returns true and pins the entry when present AND its image length
  // matches the requesting plan's span (defense in depth: the key already
  // encodes the layout mode, see the ":h" suffix for hash-mode chunks
  // whose span includes the dict-page image)
  bool cache_pin(const std::string& key, size_t expect_bytes) {
    std::lock_guard<std::mutex> g(cache_mu);
    auto it = cache.find(key);
    if (it == cache.end() || it->second.bytes != expect_bytes) return false;
    it->second.refs++;
    it->second.last_use = ++cache_clock;
    return true;
  }
  void cache_unpin(const std::string& key) {
    std::lock_guard<std::mutex> g(cache_mu);
    auto it = cache.find(key);
    if (it != cache.end() && it->second.refs > 0) it->second.refs--;
  }
  void* cache_get(const std::string& key) {
    std::lock_guard<std::mutex> g(cache_mu);
    auto it = cache.find(key);
    return it == cache.end() ? nullptr : it->second.dev;
  }
  // insert (copies nothing; caller provides a device allocation it gives up)
  void cache_put(const std::string& key, void* dev, size_t bytes, int device) {
    std::lock_guard<std::mutex> g(cache_mu);
    if (cache.count(key)) { (void)hipFree(dev); return; }
    // LRU eviction (never evicts pinned entries)
    while (cache_bytes + bytes > cache_budget) {
      auto victim = cache.end();
      for (auto it = cache.begin(); it != cache.end(); ++it)
        if (it->second.refs == 0 &&
            (victim == cache.end() ||
             it->second.last_use < victim->second.last_use))
          victim = it;
      if (victim == cache.end()) break;  // everything pinned: over-commit
      (void)hipSetDevice(victim->second.device);
      (void)hipFree(victim->second.dev);
      cache_bytes -= victim->second.bytes;
      cache.erase(victim);
    }
    CacheEntry e;
    e.dev = dev;
    e.bytes = bytes;
    e.device = device;
    e.last_use = ++cache_clock;
    cache.emplace(key, e);
    cache_bytes += bytes;
  }
};

namespace {

struct MappedFile {
  std::string path;
  int fd = -1;
  const uint8_t* data = nullptr;
  size_t size = 0;
  int64_t mtime_ns = 0;
  FileMeta meta;
  ~MappedFile() {
    if (data) munmap((void*)data, size);
    if (fd >= 0) close(fd);
  }
};

// plan-level column info
struct ColPlan {
  std::string name;
  int phys = -1;
  bool optional = false;
  // required representations
  bool need_gid = false;    // group key (utf8 dict) or COUNT(utf8 col)
  bool need_val = false;    // i64/f64 row-aligned values + valid
  bool val_always = false;  // values feed aggs/bins/projection — decode every
                            // chunk (false = predicate-only: chunks whose
                            // footer stats prove the predicate for all rows
                            // skip decode entirely)
  // raw-byte utf8 mode: the column has PLAIN-fallback data pages (dict
  // overflow, parseable/streams.rs writer defaults) but is used as a group
  // key / min-max / non-LIKE predicate — the dict-only gid path cannot
  // cover it. Rows carry STRREFs (dec-arena offsets) in d_val; group ids
  // come from the device hash build (k_hash_build/lookup); min/max and
  // predicates compare bytes in the arena. Mirrors DataFusion's row-hash
  // aggregation over arbitrary keys (stream_schema_provider.rs:219-225
  // hands the plan to that engine).
  bool hash_mode = false;
  // numeric (i64/i32/timestamp) group key: dense gids from the value hash
  // (k_numhash_*); d_val carries the key values, d_gid the assigned gids
  bool numeric_key = false;
  bool need_gid_valid = false;  // validity bytes alongside gid (COUNT(utf8))
  // COUNT(DISTINCT col): decoded exactly as a hidden group key (need_gid /
  // hash_mode / numeric_key give a dense per-partition gid, 0 = NULL) but
  // never part of group_cols, n_groups or the cascade
  bool distinct_val = false;
  // predicate routing
  std::vector<int> lut_preds;      // preds evaluated per-dict-entry (utf8)
  std::vector<int> cmp_preds;      // preds on the decoded i64 array
  std::vector<int> contains_preds; // LIKE-family preds (window path on PLAIN
                                   // byte_array pages)
  std::vector<int> null_preds;     // IS [NOT] NULL (def levels only)
  // WHERE-tree mask contexts (gpuq_plan::ctxs) holding a LUT of this column,
  // ascending: the column's LUT slot j serves context lut_ctxs[j]. {0} for
  // a flat conjunction — one LUT, the AND of lut_preds
  std::vector<int> lut_ctxs;
  bool need_rank = false;   // utf8 min/max: values decoded as dict sort-ranks
  bool is_bin = false;       // DATE_BIN pseudo-column (query/mod.rs:665-735)
  int bin_src = -1;          // source column index (p_timestamp)
  int64_t bin_stride = 0, bin_origin = 0, bin_min_idx = 0;
  int32_t nbins = 0;
  std::vector<int32_t> rank_to_gid;  // rank -> gid (1-based), for export
  // global dictionary (need_gid): gid 1.. ; 0 = NULL
  std::vector<std::string> gdict;
  std::unordered_map<std::string, int32_t> gmap;
  int32_t gid_of(const std::string& s) {
    auto it = gmap.find(s);
    if (it != gmap.end()) return it->second;
    gdict.push_back(s);
    int32_t id = (int32_t)gdict.size();  // 1-based
    gmap.emplace(gdict.back(), id);
    return id;
  }
};

struct PredPlan {
  gpuq_pred p;
  std::string col, str_lit;
  // the op as the caller gave it. A GPUQ_LIKE-family pattern that is one of
  // the fixed shapes is rewritten at plan build: p.op becomes the existing op
  // and str_lit its bare literal. A general pattern keeps its op, and str_lit
  // holds the compiled LikePat (like.h) byte for byte.
  int orig_op = 0;
};

struct AggPlan {
  int op;             // gpuq_agg_op
  std::string col;    // empty for count_star
  int col_idx = -1;   // into plan.cols
  int kind = 0;       // AGGK_*
  bool is_f64 = false;
  bool cnt_is_presence = false;  // every chunk's footer null_count == 0:
                                 // the non-null count IS the presence count
  int fsum_idx = -1;             // AGGK_SUM_F64 -> superaccumulator table idx
  int filter = -1;               // index into gpuq_plan::filters, -1 = none
};

// one column chunk of one selected row group
struct ChunkTask {
  int file_idx, rg_idx, col_idx;
  size_t dictv_pool_base = (size_t)-1;  // for the utf8-rank post-pass
  uint64_t raw_off = 0;            // into partition d_raw
  const ColumnChunkMeta* cm = nullptr;
  std::vector<PageInfo> pages;
  // dict-derived per-chunk aux (host-built)
  std::vector<int32_t> remap;      // local dict id -> gid
  std::vector<int64_t> dictv;      // local dict values (i64 / f64 bits)
  std::vector<uint8_t> lut;        // combined pred LUT (AND of lut_preds);
                                   // with a WHERE tree: slot 0 of lut_ctxs
  std::vector<std::vector<uint8_t>> lut_x;  // LUT slots 1.. (ColPlan::lut_ctxs)
  bool has_plain_data_pages = false;
  // hash-mode (raw-byte utf8) extras:
  std::vector<int64_t> strof;      // dict entries: page-relative [len] offsets
  std::vector<int64_t> pvals;      // PLAIN pages: page-relative value offsets
  std::vector<uint32_t> pval_page_n;  // per PLAIN data page: #values in pvals
  std::vector<uint32_t> pval_base;    // per PLAIN data page: dictv-pool base
  uint64_t dict_dst = (uint64_t)-1;   // dec-arena dst of the dict page image
  // hot-tier state (gpuq_ctx cache): dec-arena span of this chunk's images
  std::string cache_key;
  bool cached = false;                // dec image comes from the session cache
  uint64_t dec_base = 0, dec_len = 0;
};

struct RgRef {
  int file_idx, rg_idx;
  int64_t rows = 0, needed_bytes = 0, total_bytes = 0;
  uint32_t row_start = 0;  // partition-global
};

// decode-task lists per (kind,col); ids index into the partition's page array
enum TaskKind { TK_DICT_GID, TK_DICT_VAL, TK_PLAIN_VAL, TK_DELTA_VAL,
                TK_DICT_MASK, TK_BYTES_CONTAINS, TK_POOL_VAL,
                TK_IS_NULL, TK_IS_NOT_NULL,  // def levels of any encoding
                TK_N };
// A mask-writing task (TK_DICT_MASK, TK_BYTES_CONTAINS, TK_IS_[NOT_]NULL) of
// a WHERE-tree context other than 0 carries the context above the kind, so
// the (kind, col) task key of context 0 — every task of a flat conjunction —
// is what it always was.
constexpr int TK_CTX_SHIFT = 8;
inline int tk_ctx(int kind, int ctx) { return kind | (ctx << TK_CTX_SHIFT); }
inline int tk_kind(int key) { return key & ((1 << TK_CTX_SHIFT) - 1); }
inline int tk_ctx_of(int key) { return key >> TK_CTX_SHIFT; }

// decompress record vectors: what one planning unit (chunk) fills, and the
// merged sets of a partition (launch_decompress consumes their device view)
struct DecompRecs {
  std::vector<DevSeg> segs;
  std::vector<DevBr> brs;
  std::vector<DevPageBr> pagebrs;
  std::vector<DevBrRes> res_lane, res_wave;
  std::vector<DevPiece> piece_pool;
  std::vector<DevSeq> seqs;          // litpar sequence records ...
  std::vector<DevSeqTile> tiles;     // ... and the tiles that own them
  std::vector<DevLit> lits_wave;     // litpar literal runs > 256 B
  // host-decompressed page images staged straight into the dec arena
  // (snappy piece-explosion fallback — no serial snappy device kernel)
  std::vector<std::pair<uint64_t, std::vector<uint8_t>>> himgs;
};

// device-side view of the decompress records, in launch order
struct DecompDev {
  const uint8_t* d_raw;
  uint8_t* d_dec;
  const DevSeg* d_segs; int n_segs;
  const DevSeq* d_seqs;
  const DevSeqTile* d_tiles; int n_tiles;
  int seq_batch;   // tiles per block: 1 | 2 | 4 | 8
  const DevLit* d_lits_wave; int n_lits_wave;
  const DevBrRes* d_res_lane; int64_t n_res_lane;
  const DevBrRes* d_res_wave; int n_res_wave;
  const DevPiece* d_piece_pool;
  const DevBr* d_brs;
  const DevPageBr* d_pagebrs; int n_pagebrs;
  int32_t* d_err;
};

// Partition's own DecompRecs base is the main record set (main stream).
struct Partition : DecompRecs {
  int device = -1;
  std::vector<RgRef> rgs;
  int64_t n_rows = 0;
  std::vector<ChunkTask> chunks;
  // host-built device images
  std::vector<DevPage> pages;                 // data pages only
  std::map<std::pair<int,int>, std::vector<int32_t>> tasks;  // (kind,col)->page ids
  std::vector<int32_t> remap_pool;
  std::vector<int64_t> dictv_pool;
  std::vector<uint8_t> lut_pool;
  // LUT slots 1.. of the WHERE-tree contexts: pool j+1 has lut_pool's layout
  // (a page's aux_lut addresses every slot), zero where a column has fewer
  std::vector<std::vector<uint8_t>> lut_pool_x;
  // Delta fork: columns whose decompress records, delta
  // decode and comparisons run on the side stream, and the decompress
  // records of their chunks, kept out of the main set
  std::vector<int> fork_cols;
  DecompRecs early;
  // contains windows (host length-chain walk at load time; dev_types.h)
  std::vector<DevCWin> cwins;
  std::vector<uint16_t> cstarts;
  std::map<int, std::pair<uint32_t, uint32_t>> cwin_ranges;  // col -> (off, n)
  uint64_t raw_bytes = 0, dec_bytes = 0;
  int64_t bytes_scanned = 0, rowgroup_bytes_total = 0;
  int64_t bytes_cache_hit = 0;     // compressed bytes served from the hot tier
  bool populated = false;          // hot-tier insertion done (first execute)
  // per-pred row ranges still needing per-row evaluation (chunk-stats
  // elision, pred_all_true): merged-adjacent [start, start+len) pairs
  std::map<int, std::vector<std::pair<int64_t, int64_t>>> pred_ranges;

  // device state
  bool loaded = false;
  hipStream_t stream = nullptr;
  hipStream_t side = nullptr;      // delta fork; only with fork_cols
  DecompDev d_early{};             // device view of `early` (owned pointers)
  uint8_t *d_raw = nullptr, *d_dec = nullptr;
  DevPage* d_pages = nullptr;
  int32_t* d_remap = nullptr;
  int64_t* d_dictv = nullptr;
  uint8_t* d_lut = nullptr;
  uint8_t* d_mask = nullptr;
  // one 1 B/row buffer per aggregate filter (gpuq_plan::filters), allocated
  // at load only when the plan has filters
  std::vector<uint8_t*> d_fbufs;
  // acc / tmp pairs of the non-folded OR groups, one pair per nesting level
  std::vector<uint8_t*> d_wbufs;
  int32_t* d_err = nullptr;
  uint64_t* d_table = nullptr;
  uint64_t* d_fsum = nullptr;    // [n_fsum][n_groups][4] superacc limbs
  // raw-byte utf8 hash state (shared table, rebuilt per hash column)
  uint64_t* d_hkeys = nullptr;   // open-addressing slots (strref keys)
  int32_t* d_hgids = nullptr;
  uint32_t* d_hcount = nullptr;
  std::map<int, uint64_t*> d_gid2ref;   // hash col -> gid -> strref
  std::map<int, uint32_t> hash_claimed; // hash col -> claimed count (last exec)
  int32_t* d_cgid = nullptr;            // cascaded combined gid per row
  std::vector<uint64_t*> d_gid2pair;    // per cascade level: gid -> packed pair
  int32_t* d_agg_kind = nullptr;
  uint8_t* d_needle = nullptr;        // concatenated CONTAINS needles
  std::vector<uint32_t> needle_off;   // per plan-pred offset into the pool
  uint32_t* d_rowof = nullptr;     // dense->row map for null-bearing pages
  uint32_t* d_rank = nullptr;      // row->dense rank (expansion pass)
  uint8_t* d_scr = nullptr;        // dense decode scratch (8B/row)
  uint32_t* d_present = nullptr;   // per-page dense counts
  uint8_t* d_tmpvalid = nullptr;   // scratch validity for gid/mask-only cols
  int32_t* d_all_ids = nullptr;   // identity page-id list for the LZ4 sweep
  DevSeg* d_segs = nullptr;
  DevBr* d_brs = nullptr;
  DevPageBr* d_pagebrs = nullptr;
  DevBrRes* d_res_lane = nullptr;
  DevBrRes* d_res_wave = nullptr;
  DevSeq* d_seqs = nullptr;
  DevSeqTile* d_tiles = nullptr;
  DevPiece* d_piece_pool = nullptr;
  DevLit* d_lits_wave = nullptr;
  DevCWin* d_cwins = nullptr;
  uint16_t* d_cstarts = nullptr;
  // projection-scan buffers
  int64_t* d_keys = nullptr;
  int64_t* d_keys_sorted = nullptr;
  uint32_t* d_rows = nullptr;
  uint32_t* d_rows_sorted = nullptr;
  unsigned long long* d_count = nullptr;
  void* d_sort_temp = nullptr;
  size_t sort_temp_bytes = 0;
  std::map<std::pair<int,int>, int32_t*> d_ids;     // (kind,col) -> ids
  std::map<int, int32_t*> d_gid;                    // col -> gid array
  std::map<int, int64_t*> d_val;                    // col -> value array
  std::map<int, uint8_t*> d_valid;                  // col -> valid array
  // footer-proven null-free columns (every chunk of the column in this
  // partition has null_count == 0): their tasks launch the direct decode
  // only (mode 2), no k_def_levels / scratch decode / k_expand
  std::vector<uint8_t> col_null_free;               // by plan col index
  // fused value-decode + aggregate (gpuq_plan::fused_valagg): the agg
  // column's dict and PLAIN page ids merged in page order
  std::vector<int32_t> valagg_ids;
  int32_t* d_valagg_ids = nullptr;
  // COUNT(DISTINCT): the bitmap (distinct_bitmap_bits, shared by the
  // passes), and per distinct agg the claimed-key list and its counter
  uint64_t* d_dbitmap = nullptr;
  std::vector<uint64_t*> d_dpairs;
  uint32_t* d_dcount = nullptr;
  int64_t load_ns = 0;
};

// H2D staging ring: pinned buffers filled from host memory (mmap'd files /
// pool vectors) by a parallel memcpy, async-copied to the device.
// hipMemcpyAsync straight from pageable mmap pages was fault + staging
// bound (~1.3 GB/s measured); the 1 B-row shards move tens of GB of raw
// chunks plus multi-GB aux pools (literal records, dictionary values), so
// every bulk upload in gpuq_plan_load goes through this ring at PCIe-class
// rates.
struct Ring {
  static constexpr size_t BUFSZ = 256ull << 20;
  static constexpr int NBUF = 4;
  void* bufs[NBUF] = {};
  hipEvent_t evts[NBUF] = {};
  hipStream_t stream;
  int b = 0;
  explicit Ring(hipStream_t st);
  ~Ring();
  struct Span { const uint8_t* src; uint64_t len; };
  void copy_spans(uint8_t* d_dst, const std::vector<Span>& spans);
  void copy(void* d_dst, const void* src, size_t len);
};

}  // namespace

namespace {
constexpr int HASH_LOG2 = 24;          // shared open-addressing table slots
constexpr int32_t GID_CAP = 1 << 22;   // max distinct groups (per col & total)
// COUNT(DISTINCT): claimed (group, value) pairs per partition — load factor
// 0.5 of the shared table — and the bitmap path's default size (32 MB)
constexpr uint32_t DISTINCT_PAIR_CAP = 1u << 23;
constexpr uint64_t DISTINCT_BITMAP_BITS = 1ull << 28;
// bitmaps up to this size are marked through a block-local LDS copy (16 KiB:
// small enough to keep the CU full of blocks); at most 64 KiB of LDS
constexpr uint64_t DISTINCT_LDS_BITS = 1ull << 17;
}  // namespace

struct gpuq_plan {
  gpuq_ctx* ctx = nullptr;
  std::vector<std::unique_ptr<MappedFile>> files;
  std::vector<ColPlan> cols;
  std::vector<PredPlan> preds;
  std::vector<AggPlan> aggs;
  std::vector<int> group_cols;   // indices into cols
  std::vector<int> projection;   // projection-scan mode (ORDER BY ts DESC LIMIT k)
  bool is_projection = false;
  int ts_col = -1;               // sort key (p_timestamp) col index
  int64_t limit = -1;
  std::vector<Partition> parts;
  int32_t n_groups = 0;          // product of key sizes (incl null slots)
  int32_t n_fsum = 0;            // number of exact-f64-sum side tables
  bool has_hash = false;         // some column runs raw-byte utf8 hash mode
  bool needs_cascade = false;    // dense key product exceeds GID_CAP
  bool has_numkey = false;       // some group key is numeric (value-hashed)
  std::vector<std::string> pinned_keys;  // hot-tier entries pinned by this plan
  int64_t m_cache_hit_bytes = 0;
  bool fused_count = false;      // single dict key + count(*)-only + no preds
  // single key + {count(*), one i64 sum/min/max over a null-free column
  // nothing else reads}: the value column is aggregated where it is decoded
  // (k_val_agg) instead of materialised for k_agg_fast
  bool fused_valagg = false;
  int valagg_col = -1;           // the aggregated column (index into cols)
  bool valagg_late = false;      // group count known only at execute (hash /
                                 // numeric key): the old kernels stay armed
  int valagg_blocks = 1024;      // persistent grid cap (GPUQ_VALAGG_BLOCKS)
  bool no_fused_valagg = false;  // GPUQ_NO_FUSED_VALAGG
  // dictionary-index decoders (kernels_api.h serial_walk), read at plan build:
  // GPUQ_DICT_WALK=serial forces the one-header-per-step walk
  bool dict_serial = false;
  // sequence tiles per block (k_seq_tile<K>), GPUQ_SEQ_TILE_BATCH at build
  int seq_tile_batch = SEQ_TILE_BATCH_DEFAULT;
  bool no_delta_fork = false;    // GPUQ_NO_DELTA_FORK: serial order
  bool exec_dbg = false;         // GPUQ_PLAN_DEBUG at build: log the agg path
  // COUNT(DISTINCT) (read at plan build): aggs of that kind in agg order;
  // bitmap path when n_groups x padded value cardinality fits
  // distinct_bitmap_bits (GPUQ_DISTINCT_BITMAP_BITS) and
  // GPUQ_DISTINCT_FORCE_HASH is unset; the claimed-pair list holds
  // distinct_pair_cap keys (GPUQ_DISTINCT_PAIR_CAP lowers it)
  std::vector<int> distinct_aggs;
  // WHERE tree (where.h). A pure conjunction leaves has_tree false and
  // everything below empty: the flat plan, context 0 = d_mask alone.
  //  - a context is one AND-evaluation unit writing one mask buffer: the
  //    root AND (context 0, d_mask) and every term of a non-folded OR;
  //  - pred_ctx[p]: the context leaf p evaluates in, -1 when its OR group
  //    was folded into a single-column LUT (WFold);
  //  - a WOr at nesting level L accumulates in d_wbufs[2L] and evaluates its
  //    later terms in d_wbufs[2L+1].
  bool has_tree = false;
  WhereTree where;
  std::vector<int> pred_ctx;
  struct WOr { int node; int ctx; int level; std::vector<int> terms; };
  struct WFold { int node; int ctx; int col; };
  struct WCtx { std::vector<int> ors; };   // indices into wors
  std::vector<WCtx> ctxs;
  std::vector<WOr> wors;
  std::vector<WFold> wfolds;
  int n_wbufs = 0;
  int ctx_of(int pidx) const { return has_tree ? pred_ctx[pidx] : 0; }
  bool no_fcount = false;  // GPUQ_NO_FCOUNT: k_agg<.., true> where k_agg_fcount
                           // would run (A/B timing, tests)
  // Aggregate filters (gpuq_agg_filter). Filter trees are appended to
  // where.nodes as a forest (where_append) — where.root still spans WHERE
  // alone, so pruning never sees a filter leaf — and each becomes one more
  // context, evaluated into Partition::d_fbufs[j] after d_mask is final. A
  // plan with filters always has has_tree set.
  struct AggFilter { int agg; int root; int ctx; int depth; };
  std::vector<AggFilter> filters;
  std::vector<int> pred_filter;  // per pred: its filter, -1 for a WHERE leaf
  uint64_t distinct_bitmap_bits = DISTINCT_BITMAP_BITS;
  uint64_t distinct_lds_bits = DISTINCT_LDS_BITS;  // GPUQ_DISTINCT_LDS_BITS
  uint32_t distinct_pair_cap = DISTINCT_PAIR_CAP;
  bool distinct_force_hash = false;
  std::mutex mu;
  // metrics
  int64_t m_rows_scanned = 0, m_rows_out = 0, m_kernel_ns = 0, m_exec_ns = 0,
          m_load_ns = 0, m_decomp_ns = 0, m_hbm_est = 0;
  ~gpuq_plan();
};

// ------------------------------------------------------------------
// C ABI: session
// ------------------------------------------------------------------
extern "C" gpuq_ctx* gpuq_session_create(uint64_t device_mask) {
  auto* c = new gpuq_ctx();
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  if (n == 0 && getenv("GPUQ_FAKE_DEVICE")) n = 1;  // host-plan debugging ONLY:
  // plan_build is pure host work; load/execute still fail at the first HIP call.
  for (int i = 0; i < 64 && i < n; i++)
    if (device_mask & (1ull << i)) c->devices.push_back(i);
  if (c->devices.empty() && device_mask == 0 && n > 0) c->devices.push_back(0);
  return c;
}
extern "C" void gpuq_session_destroy(gpuq_ctx* c) { delete c; }
namespace {
// error text of calls made without a session (test-support entry only)
thread_local std::string g_null_ctx_error = "null ctx";
}  // namespace
extern "C" const char* gpuq_last_error(gpuq_ctx* c) {
  return c ? c->last_error.c_str() : g_null_ctx_error.c_str();
}
extern "C" int32_t gpuq_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return -1;
  return n;
}

// ------------------------------------------------------------------
// plan building
// ------------------------------------------------------------------
namespace {

// GPUQ_SEQ_TILE_BATCH=1|2|4|8: sequence tiles per block; anything else is
// the default
int seq_tile_batch_env() {
  if (const char* e = getenv("GPUQ_SEQ_TILE_BATCH")) {
    const int k = atoi(e);
    if (k == 1 || k == 2 || k == 4 || k == 8) return k;
  }
  return SEQ_TILE_BATCH_DEFAULT;
}

// Delta fork, plan level: may column ci's decompress, decode and compare run
// on the side stream? Only a column that nothing but numeric comparisons of
// WHERE context 0 reads: no key, aggregate, distinct value, DATE_BIN source
// or projection (val_always), no LUT / null predicate, no filter leaf.
bool fork_col(const gpuq_plan& plan, int ci) {
  const ColPlan& c = plan.cols[ci];
  if (!c.need_val || c.val_always || c.need_gid || c.hash_mode ||
      c.numeric_key || c.distinct_val || c.is_bin || c.cmp_preds.empty() ||
      !c.lut_preds.empty() || !c.null_preds.empty())
    return false;
  for (int pidx : c.cmp_preds)
    if (plan.ctx_of(pidx) != 0 || plan.pred_filter[pidx] >= 0) return false;
  return true;
}

// environment knobs, read once into the plan
void read_env_knobs(gpuq_plan* plan) {
  plan->exec_dbg = getenv("GPUQ_PLAN_DEBUG") != nullptr;
  plan->no_fused_valagg = getenv("GPUQ_NO_FUSED_VALAGG") != nullptr;
  plan->no_fcount = getenv("GPUQ_NO_FCOUNT") != nullptr;
  if (const char* e = getenv("GPUQ_VALAGG_BLOCKS"))
    plan->valagg_blocks = std::max(1, atoi(e));
  if (const char* e = getenv("GPUQ_DICT_WALK"))
    plan->dict_serial = strcmp(e, "serial") == 0;
  plan->seq_tile_batch = seq_tile_batch_env();
  plan->no_delta_fork = getenv("GPUQ_NO_DELTA_FORK") != nullptr;
  // COUNT(DISTINCT) knobs. The bitmap stays below 2^31 bits so the emit
  // pass's u32 list cursor cannot wrap; the pair cap can only be lowered.
  if (const char* e = getenv("GPUQ_DISTINCT_BITMAP_BITS"))
    plan->distinct_bitmap_bits =
        std::min<uint64_t>(strtoull(e, nullptr, 10), 1ull << 31);
  if (const char* e = getenv("GPUQ_DISTINCT_LDS_BITS"))
    plan->distinct_lds_bits =
        std::min<uint64_t>(strtoull(e, nullptr, 10), 64 * 1024 * 8);
  if (const char* e = getenv("GPUQ_DISTINCT_PAIR_CAP"))
    plan->distinct_pair_cap = (uint32_t)std::min<uint64_t>(
        std::max<uint64_t>(strtoull(e, nullptr, 10), 1), DISTINCT_PAIR_CAP);
  if (const char* e = getenv("GPUQ_DISTINCT_FORCE_HASH"))
    plan->distinct_force_hash = atoi(e) != 0;
}

int find_or_add_col(std::vector<ColPlan>& cols, const std::string& name) {
  for (size_t i = 0; i < cols.size(); i++)
    if (cols[i].name == name) return (int)i;
  cols.push_back(ColPlan{});
  cols.back().name = name;
  return (int)cols.size() - 1;
}

// LIKE family (CONTAINS, the seven ops added after it and the four general
// pattern ops): utf8 only, routed to the LUT / window / hash paths, never
// pruned or elided by min/max stats
bool op_is_pattern(int op) { return op >= GPUQ_LIKE && op <= GPUQ_NOT_ILIKE; }
bool op_is_like(int op) {
  return op == GPUQ_CONTAINS ||
         (op >= GPUQ_ICONTAINS && op <= GPUQ_NOT_ENDS_WITH) || op_is_pattern(op);
}
bool op_is_null(int op) { return op == GPUQ_IS_NULL || op == GPUQ_IS_NOT_NULL; }
// kernel match mode (dev_types.h StrKind | STRF_*) of a LIKE-family op
int like_mode(int op) {
  switch (op) {
    case GPUQ_ICONTAINS: return STR_CONTAINS | STRF_FOLD;
    case GPUQ_STARTS_WITH: return STR_PREFIX;
    case GPUQ_ENDS_WITH: return STR_SUFFIX;
    case GPUQ_NOT_CONTAINS: return STR_CONTAINS | STRF_NEG;
    case GPUQ_NOT_ICONTAINS: return STR_CONTAINS | STRF_FOLD | STRF_NEG;
    case GPUQ_NOT_STARTS_WITH: return STR_PREFIX | STRF_NEG;
    case GPUQ_NOT_ENDS_WITH: return STR_SUFFIX | STRF_NEG;
    case GPUQ_LIKE: return STR_PATTERN;
    case GPUQ_NOT_LIKE: return STR_PATTERN | STRF_NEG;
    case GPUQ_ILIKE: return STR_PATTERN | STRF_FOLD;
    case GPUQ_NOT_ILIKE: return STR_PATTERN | STRF_FOLD | STRF_NEG;
    default: return STR_CONTAINS;
  }
}
const char* op_name(int op) {
  static const char* names[] = {
      "eq", "ne", "lt", "le", "gt", "ge", "between", "contains", "icontains",
      "starts_with", "ends_with", "not_contains", "not_icontains",
      "not_starts_with", "not_ends_with", "is_null", "is_not_null",
      "like", "not_like", "ilike", "not_ilike"};
  return (op >= 0 && op <= GPUQ_NOT_ILIKE) ? names[op] : "?";
}

// IS [NOT] NULL against one chunk's footer: null_count == 0 (or a required
// column) proves IS NOT NULL and makes IS NULL unsatisfiable; null_count ==
// num_values is the mirror image; anything else needs the per-row task.
enum NullState { NULLP_EVAL = 0, NULLP_PROVEN, NULLP_UNSAT };
NullState null_pred_state(int op, const ColumnChunkMeta& cm, bool optional) {
  const bool none_null = !optional || cm.null_count == 0;
  const bool all_null = optional && cm.null_count >= 0 &&
                        cm.null_count == cm.num_values && cm.num_values > 0;
  if (op == GPUQ_IS_NOT_NULL)
    return none_null ? NULLP_PROVEN : all_null ? NULLP_UNSAT : NULLP_EVAL;
  return none_null ? NULLP_UNSAT : all_null ? NULLP_PROVEN : NULLP_EVAL;
}

// row-group-level min/max pruning for i64 comparisons — the row-group analog
// of ManifestExt::can_be_pruned + satisfy_constraints
// (stream_schema_provider.rs:1049-1137): prune when the predicate can match
// NO value in [min,max]. The LIKE family never prunes; IS [NOT] NULL prunes
// on the footer null_count alone (its literal fields are undefined).
// One leaf: TRUE when no row of the row group can satisfy it.
bool leaf_rg_none(const PredPlan& pp, const FileMeta& fm,
                  const RowGroupMeta& rg) {
  if (op_is_like(pp.p.op)) return false;
  if (op_is_null(pp.p.op)) {
    int ci = fm.col_index(pp.col);
    return ci >= 0 && null_pred_state(pp.p.op, rg.chunks[ci],
                                      fm.columns[ci].optional) == NULLP_UNSAT;
  }
  if (pp.p.lit_kind != GPUQ_LIT_I64) return false;
  int ci = fm.col_index(pp.col);
  if (ci < 0) return false;
  const auto& cm = rg.chunks[ci];
  if (!cm.has_i64_stats) return false;
  int64_t mn = cm.stat_min, mx = cm.stat_max;
  bool can_match = true;
  switch (pp.p.op) {
    case GPUQ_EQ: can_match = pp.p.i64[0] >= mn && pp.p.i64[0] <= mx; break;
    case GPUQ_LT: can_match = mn < pp.p.i64[0]; break;
    case GPUQ_LE: can_match = mn <= pp.p.i64[0]; break;
    case GPUQ_GT: can_match = mx > pp.p.i64[0]; break;
    case GPUQ_GE: can_match = mx >= pp.p.i64[0]; break;
    case GPUQ_BETWEEN:
      can_match = (pp.p.hi_exclusive ? mn < pp.p.i64[1] : mn <= pp.p.i64[1]) &&
                  mx >= pp.p.i64[0];
      break;
    default: break;
  }
  return !can_match;
}
// The row group goes away when the WHERE root can match no row: any leaf of
// a flat conjunction; with a tree an AND if any child cannot, an OR only if
// no child can (where_none).
bool rg_pruned_by_stats(const gpuq_plan& plan, const FileMeta& fm,
                        const RowGroupMeta& rg) {
  if (!plan.has_tree) {
    for (const auto& pp : plan.preds)
      if (leaf_rg_none(pp, fm, rg)) return true;
    return false;
  }
  return where_none(plan.where, plan.where.root, [&](int pi) {
    return leaf_rg_none(plan.preds[pi], fm, rg);
  });
}

// Chunk-stats predicate elision: TRUE when the footer stats prove EVERY row
// of the chunk satisfies the predicate — the exactness the reference's
// engine gets from its minute-aligned pruning predicates
// (build_parquet_scan_components, stream_schema_provider.rs:127-144:
// files fully inside the window are scanned with the Exact filter already
// satisfied, so DataFusion never evaluates it per row). Such chunks keep
// their memset-1 selection mask and, when the column is predicate-only,
// are never decoded at all. Requires null_count == 0: a NULL row must not
// satisfy any predicate.
bool pred_all_true(const gpuq_pred& p, const ColumnChunkMeta& cm,
                   bool optional) {
  // explicit, not by accident of default: a null op's zero-initialised
  // lit_kind reads as GPUQ_LIT_I64 with a meaningless literal
  if (op_is_like(p.op)) return false;
  if (op_is_null(p.op)) return null_pred_state(p.op, cm, optional) == NULLP_PROVEN;
  if (p.lit_kind != GPUQ_LIT_I64 || !cm.has_i64_stats) return false;
  if (cm.null_count != 0) return false;
  int64_t mn = cm.stat_min, mx = cm.stat_max;
  switch (p.op) {
    case GPUQ_EQ: return mn == p.i64[0] && mx == p.i64[0];
    case GPUQ_NE: return p.i64[0] < mn || p.i64[0] > mx;
    case GPUQ_LT: return mx < p.i64[0];
    case GPUQ_LE: return mx <= p.i64[0];
    case GPUQ_GT: return mn > p.i64[0];
    case GPUQ_GE: return mn >= p.i64[0];
    case GPUQ_BETWEEN:
      return mn >= p.i64[0] &&
             (p.hi_exclusive ? mx < p.i64[1] : mx <= p.i64[1]);
    default: return false;
  }
}

// GPUQ_LIKE family at plan build: compile the pattern, then either rewrite
// the predicate to the existing op whose shape it has — so LIKE '%error%'
// builds exactly the CONTAINS plan and runs in the tuned k_contains_win<>
// kernel — or keep the op and carry the compiled LikePat in str_lit (the
// needle pool uploads it like any literal).
//   '%lit%'          -> [NOT_][I]CONTAINS lit
//   'lit%' / '%lit'  -> [NOT_]STARTS_WITH / ENDS_WITH lit   (LIKE only)
//   '%' ('%%', ..)   -> [NOT_]CONTAINS '': every non-null row, or none
// Anything else is general: any '_', an inner '%', no '%' at all (not EQ: EQ
// on a column with PLAIN pages forces hash mode, the window path does not),
// and the ILIKE prefix / suffix shapes.
void compile_pattern_pred(PredPlan& pp) {
  const int op = pp.p.op;
  const bool fold = op == GPUQ_ILIKE || op == GPUQ_NOT_ILIKE;
  const bool neg = op == GPUQ_NOT_LIKE || op == GPUQ_NOT_ILIKE;
  LikePat P;
  if (const char* why = like_compile(pp.str_lit.data(), pp.str_lit.size(),
                                     fold, &P)) {
    const std::string w = why, name = op_name(op);
    if (w == "non-ascii")  // the wording of the ICONTAINS rule
      throw std::runtime_error(name + " literal must be ASCII "
                               "(case folding is ASCII-only): " + pp.col);
    if (w == "trailing backslash")
      throw std::runtime_error(name + " pattern ends in a lone backslash: " +
                               pp.col);
    if (w == "too many elements")
      throw std::runtime_error(name + " pattern has more than 255 elements: " +
                               pp.col);
    throw std::runtime_error(name + " pattern has more than 16 %-separated "
                             "segments: " + pp.col);
  }
  std::string lit;
  int as = -1;
  switch (like_shape(P, &lit)) {
    case LIKE_SHAPE_CONTAINS:
      as = fold ? (neg ? GPUQ_NOT_ICONTAINS : GPUQ_ICONTAINS)
                : (neg ? GPUQ_NOT_CONTAINS : GPUQ_CONTAINS);
      break;
    case LIKE_SHAPE_PREFIX:
      if (!fold) as = neg ? GPUQ_NOT_STARTS_WITH : GPUQ_STARTS_WITH;
      break;
    case LIKE_SHAPE_SUFFIX:
      if (!fold) as = neg ? GPUQ_NOT_ENDS_WITH : GPUQ_ENDS_WITH;
      break;
    case LIKE_SHAPE_ALL:
      as = neg ? GPUQ_NOT_CONTAINS : GPUQ_CONTAINS;
      break;
    default: break;
  }
  if (as >= 0) {
    pp.p.op = as;
    pp.str_lit = lit;  // already lower-cased for the folding ops
  } else {
    pp.str_lit.assign(reinterpret_cast<const char*>(&P), sizeof(P));
  }
}

// evaluate a string predicate against one dict entry (host; LUT build)
bool eval_str_pred(const gpuq_pred& p, const std::string& lit,
                   const uint8_t* s, uint32_t len) {
  if (op_is_like(p.op)) {
    // same semantics as k_contains_win<> / k_affix_win<> / k_cmp_str, so the
    // dict pages and the PLAIN pages of one chunk agree; `lit` is already
    // lower-cased for the folding ops. The LUT covers dict entries only —
    // NULL rows are zeroed by the expand mode, negated ops included.
    const int m = like_mode(p.op);
    bool ok = false;
    if ((m & STRF_KIND) == STR_PATTERN) {
      // general pattern: `lit` is the compiled LikePat, matched by the one
      // function the kernels call (like.h)
      const LikePat& P = *reinterpret_cast<const LikePat*>(lit.data());
      auto get = [&](uint32_t i) { return s[i]; };
      ok = (m & STRF_FOLD) ? like_match<true>(P, get, len)
                           : like_match<false>(P, get, len);
    } else if (lit.empty()) ok = true;
    else if (len >= lit.size()) {
      const size_t nl = lit.size();
      auto fc = [&](uint8_t c) -> uint8_t {
        return ((m & STRF_FOLD) && c >= 'A' && c <= 'Z') ? (uint8_t)(c | 0x20) : c;
      };
      auto at = [&](const uint8_t* b) {
        for (size_t k = 0; k < nl; k++)
          if (fc(b[k]) != (uint8_t)lit[k]) return false;
        return true;
      };
      switch (m & STRF_KIND) {
        case STR_PREFIX: ok = at(s); break;
        case STR_SUFFIX: ok = at(s + len - nl); break;
        default:
          if (!(m & STRF_FOLD)) ok = memmem(s, len, lit.data(), nl) != nullptr;
          else for (size_t j = 0; j + nl <= len && !ok; j++) ok = at(s + j);
          break;
      }
    }
    return (m & STRF_NEG) ? !ok : ok;
  }
  int c = memcmp(s, lit.data(), std::min((size_t)len, lit.size()));
  if (c == 0) c = (len < lit.size()) ? -1 : (len > lit.size() ? 1 : 0);
  switch (p.op) {
    case GPUQ_EQ: return c == 0;
    case GPUQ_NE: return c != 0;
    case GPUQ_LT: return c < 0;
    case GPUQ_LE: return c <= 0;
    case GPUQ_GT: return c > 0;
    case GPUQ_GE: return c >= 0;
  }
  return false;
}

// decompress one page payload on the host (dict pages / plan-time walks):
// LZ4_RAW, snappy, or stored raw
const uint8_t* host_page_payload(int codec, const uint8_t* src, uint32_t comp,
                                 uint32_t uncomp, std::vector<uint8_t>& buf) {
  if (codec == CODEC_UNCOMPRESSED) return src;
  buf.resize(uncomp);
  if (codec == CODEC_LZ4_RAW) {
    // ALWAYS try LZ4 first: the writer compresses every v1 page, and
    // comp_size may coincidentally equal uncomp_size; only a failed decode
    // of an equal-size page means the page was stored raw
    int n = lz4_decompress_host(src, comp, buf.data(), buf.size());
    if (n == (int)uncomp) return buf.data();
    if (comp == uncomp) return src;
    throw std::runtime_error("page lz4 failure");
  }
  if (codec == CODEC_SNAPPY) {
    int n = snappy_decompress_host(src, comp, buf.data(), buf.size());
    if (n == (int)uncomp) return buf.data();
    throw std::runtime_error("page snappy failure");
  }
  throw std::runtime_error("unsupported codec");
}

// parse a v1 data page's def levels (bit-width-1 RLE/bit-packed hybrid,
// parquet-format RLE); returns the payload offset after the levels and
// fills defs (1 = value present)
uint32_t parse_def1(const uint8_t* data, uint32_t nv, std::vector<uint8_t>& defs) {
  uint32_t dl;
  memcpy(&dl, data, 4);
  defs.assign(nv, 1);
  const uint8_t* p = data + 4;
  const uint8_t* end = p + dl;
  uint32_t v = 0;
  while (v < nv && p < end) {
    uint64_t hdr = 0;
    int sh = 0;
    for (;;) {
      uint8_t b = *p++;
      hdr |= (uint64_t)(b & 0x7f) << sh;
      if (!(b & 0x80)) break;
      sh += 7;
    }
    if (hdr & 1) {
      uint32_t groups = (uint32_t)(hdr >> 1);
      for (uint32_t g = 0; g < groups; g++) {
        uint8_t byte = p[g];
        for (int j = 0; j < 8; j++) {
          uint32_t idx = v + g * 8 + j;
          if (idx < nv) defs[idx] = (byte >> j) & 1;
        }
      }
      p += groups;
      uint32_t add = groups * 8;
      v += add > nv - v ? nv - v : add;
    } else {
      uint32_t cnt = (uint32_t)(hdr >> 1);
      uint8_t val = *p++;
      if (cnt > nv - v) cnt = nv - v;
      std::fill(defs.begin() + v, defs.begin() + v + cnt, val);
      v += cnt;
    }
  }
  return 4 + dl;
}

// One PLAIN byte-array page: the [u32 len][bytes] chain behind the optional
// def levels. visit(pos, len) per non-null value, pos the page-relative
// offset of its length field. Positions are 64-bit, so a length that would
// wrap 32-bit arithmetic is an overrun like any other: returns false.
template <class Visit>
bool walk_plain_bytes(const uint8_t* data, uint32_t uncomp_size,
                      uint32_t num_values, bool optional, Visit&& visit) {
  std::vector<uint8_t> defs;
  uint64_t pos = optional ? parse_def1(data, num_values, defs) : 0;
  for (uint32_t v = 0; v < num_values; v++) {
    if (optional && !defs[v]) continue;
    if (pos + 4 > uncomp_size) return false;
    uint32_t len;
    memcpy(&len, data + pos, 4);
    const uint64_t rec = 4ull + len;
    if (pos + rec > uncomp_size) return false;
    visit((uint32_t)pos, len);
    pos += rec;
  }
  return true;
}

int64_t now_ns() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (int64_t)ts.tv_sec * 1000000000 + ts.tv_nsec;
}

// Simple parallel-for over [0, n): the 1 B-row configs have thousands of
// files/chunks whose footer parses, dict decompresses and LZ4 structure
// walks are independent — serial host planning was the wall at that scale.
// Rethrows the first worker exception on the calling thread.
template <class F>
void parallel_for(size_t n, F&& fn, size_t max_threads = 0) {
  if (n == 0) return;
  size_t hw = std::thread::hardware_concurrency();
  if (hw == 0) hw = 8;
  // one-process-per-GPU launches cap their host planning threads so eight
  // ranks don't spawn 8 x cores workers (GPUQ_HOST_THREADS; bench.py sets it)
  static const size_t env_cap = [] {
    const char* e = getenv("GPUQ_HOST_THREADS");
    return e ? (size_t)strtoul(e, nullptr, 10) : (size_t)0;
  }();
  if (env_cap) hw = std::min(hw, env_cap);
  if (max_threads) hw = std::min(hw, max_threads);
  size_t nthreads = std::min(n, hw);
  if (nthreads <= 1) {
    for (size_t i = 0; i < n; i++) fn(i);
    return;
  }
  std::atomic<size_t> next{0};
  std::mutex emu;
  std::exception_ptr eptr;
  auto worker = [&]() {
    for (;;) {
      size_t i = next.fetch_add(1);
      if (i >= n) return;
      try {
        fn(i);
      } catch (...) {
        std::lock_guard<std::mutex> g(emu);
        if (!eptr) eptr = std::current_exception();
        next.store(n);  // drain
        return;
      }
    }
  };
  std::vector<std::thread> pool;
  pool.reserve(nthreads);
  for (size_t t = 0; t < nthreads; t++) pool.emplace_back(worker);
  for (auto& th : pool) th.join();
  if (eptr) std::rethrow_exception(eptr);
}

// One record stream of the phase-5 merge: offsets by prefix sum, resize,
// then every chunk copies its slice in parallel, rebase(element, chunk)
// applied on the way where the records carry indices into another merged
// stream. Returns the per-chunk offsets (what such a rebase adds).
template <class C, class T, class B, class Rebase>
std::vector<size_t> merge_stream(std::vector<C>& cbs, std::vector<T> B::*src,
                                 std::vector<T>& dst, Rebase&& rebase) {
  const size_t nc = cbs.size();
  std::vector<size_t> off(nc + 1, 0);
  for (size_t i = 0; i < nc; i++) off[i + 1] = off[i] + (cbs[i].*src).size();
  dst.resize(off[nc]);
  parallel_for(nc, [&](size_t i) {
    const std::vector<T>& s = cbs[i].*src;
    for (size_t j = 0; j < s.size(); j++) {
      T e = s[j];
      rebase(e, i);
      dst[off[i] + j] = e;
    }
  });
  return off;
}
template <class C, class T, class B>
std::vector<size_t> merge_stream(std::vector<C>& cbs, std::vector<T> B::*src,
                                 std::vector<T>& dst) {
  return merge_stream(cbs, src, dst, [](T&, size_t) {});
}

// the decompress record streams of every chunk, merged in chunk order
template <class C>
void merge_decomp_recs(std::vector<C>& cbs, DecompRecs& dst) {
  merge_stream(cbs, &DecompRecs::segs, dst.segs);
  const auto o_brs = merge_stream(cbs, &DecompRecs::brs, dst.brs);
  merge_stream(cbs, &DecompRecs::pagebrs, dst.pagebrs,
               [&](DevPageBr& pb, size_t i) { pb.start += (uint32_t)o_brs[i]; });
  const auto o_pp = merge_stream(cbs, &DecompRecs::piece_pool, dst.piece_pool);
  auto piece_rebase = [&](DevBrRes& r, size_t i) {
    r.piece_start += (uint32_t)o_pp[i];
  };
  merge_stream(cbs, &DecompRecs::res_lane, dst.res_lane, piece_rebase);
  merge_stream(cbs, &DecompRecs::res_wave, dst.res_wave, piece_rebase);
  const auto o_sq = merge_stream(cbs, &DecompRecs::seqs, dst.seqs);
  merge_stream(cbs, &DecompRecs::tiles, dst.tiles,
               [&](DevSeqTile& t, size_t i) { t.rec0 += o_sq[i]; });
  merge_stream(cbs, &DecompRecs::lits_wave, dst.lits_wave);
}

Ring::Ring(hipStream_t st) : stream(st) {
  for (int i = 0; i < NBUF; i++) {
    HIP_TRY(hipHostMalloc(&bufs[i], BUFSZ));
    HIP_TRY(hipEventCreate(&evts[i]));
    HIP_TRY(hipEventRecord(evts[i], stream));
  }
}
Ring::~Ring() {
  for (int i = 0; i < NBUF; i++) {
    if (bufs[i]) (void)hipHostFree(bufs[i]);
    if (evts[i]) (void)hipEventDestroy(evts[i]);
  }
}
// copy the concatenation of spans to d_dst (device), pipelined: fill of
// buffer b overlaps the in-flight H2D copies of the other ring slots
void Ring::copy_spans(uint8_t* d_dst, const std::vector<Span>& spans) {
  size_t si = 0;
  uint64_t soff = 0, dst = 0;
  while (si < spans.size()) {
    if (spans[si].len == 0) { si++; continue; }
    HIP_TRY(hipEventSynchronize(evts[b]));
    struct Fill { const uint8_t* src; uint8_t* dstp; size_t len; };
    std::vector<Fill> fills;
    size_t filled = 0;
    while (si < spans.size() && filled < BUFSZ) {
      uint64_t take = std::min<uint64_t>(spans[si].len - soff, BUFSZ - filled);
      while (take > 0) {  // slice so the parallel fill balances
        uint64_t piece = std::min<uint64_t>(take, 4ull << 20);
        fills.push_back({spans[si].src + soff, (uint8_t*)bufs[b] + filled,
                         piece});
        filled += piece;
        soff += piece;
        take -= piece;
      }
      if (soff == spans[si].len) { si++; soff = 0; }
    }
    parallel_for(fills.size(), [&](size_t f) {
      memcpy(fills[f].dstp, fills[f].src, fills[f].len);
    }, 32);
    HIP_TRY(hipMemcpyAsync(d_dst + dst, bufs[b], filled,
                           hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(evts[b], stream));
    dst += filled;
    b = (b + 1) % NBUF;
  }
}
void Ring::copy(void* d_dst, const void* src, size_t len) {
  if (len) copy_spans((uint8_t*)d_dst, {{(const uint8_t*)src, len}});
}

// ------------------------------------------------------------------
// page decompression planning + launches (shared by plan build / execute
// and the gpuq_test_decompress test-support entry)
// ------------------------------------------------------------------
constexpr uint32_t BR_FAR = 16384 / 2;  // kernels.hip BR_WIN / 2

// decompress planning for one page image (data or hash-col dict):
// segment walk + litpar/backref records, exactly the round-1 logic.
// force: GPUQ_DECOMP_* plan mode (plan build passes AUTO); st (optional)
// receives the path taken and the record counts.
void plan_decomp_page(DecompRecs& cb, int codec, const uint8_t* praw,
                      uint64_t src_abs, uint64_t dst_abs, uint32_t comp,
                      uint32_t uncomp, bool raw_page,
                      int force = GPUQ_DECOMP_AUTO,
                      gpuq_decomp_stats* st = nullptr) {
  Lz4Plan lp;
  if (st) *st = gpuq_decomp_stats{};
  if (!raw_page && codec == CODEC_SNAPPY) {
    lp = snappy_walk(praw, comp, uncomp);
    if (st) st->n_seq = lp.n_seq;
    if (lp.fallback) {
      // piece explosion (rare): host-decompress the page and stage
      // its image straight into the dec arena at load
      std::vector<uint8_t> img(uncomp);
      if (snappy_decompress_host(praw, comp, img.data(), uncomp) !=
          (int)uncomp)
        throw std::runtime_error("snappy page decode failure");
      cb.himgs.emplace_back(dst_abs, std::move(img));
      if (st) st->mode = GPUQ_DECOMP_PAGE_HOST_IMAGE;
      return;
    }
  } else if (!raw_page) {
    // test knob: exercise the serial windowed fallback kernel on
    // arbitrary content
    static const bool env_fb =
        std::getenv("GPUQ_FORCE_LZ4_FALLBACK") != nullptr;
    const bool force_fb = force == GPUQ_DECOMP_FORCE_FALLBACK ||
                          (force == GPUQ_DECOMP_AUTO && env_fb);
    try {
      lp = lz4_walk(praw, comp, uncomp, 8192);
      if (force_fb) {
        lp.fallback = true;
        lp.resolved.clear();
        lp.pieces.clear();
      }
      // dense short-sequence pages (LZ4 over near-random dict
      // indices) degenerate the segment kernel into a serial token
      // parse — switch those to the all-literal/all-resolved plan
      const bool want_litpar =
          force == GPUQ_DECOMP_FORCE_LITPAR ||
          (force == GPUQ_DECOMP_AUTO && lp.n_seq >= 256 &&
           uncomp / lp.n_seq < 96);
      if (!lp.fallback && want_litpar) {
        Lz4Plan lp2 = lz4_walk(praw, comp, uncomp, 8192, /*litpar=*/true);
        if (!lp2.fallback) lp = std::move(lp2);
      }
    } catch (const std::exception&) {
      if (comp == uncomp) raw_page = true;  // stored raw
      else throw;
    }
    if (st) st->n_seq = lp.n_seq;
  }
  if (raw_page) {
    DevSeg sgl{};
    sgl.src_off = src_abs;
    sgl.dst_off = dst_abs;
    sgl.comp_len = comp;
    sgl.out_len = uncomp;
    sgl.raw = 1;
    cb.segs.push_back(sgl);
    if (st) {
      st->mode = GPUQ_DECOMP_PAGE_RAW;
      st->n_seq = 0;
      st->n_segs = 1;
    }
    return;
  }
  if (st) {
    st->mode = lp.fallback ? GPUQ_DECOMP_PAGE_FALLBACK
               : lp.litpar ? GPUQ_DECOMP_PAGE_LITPAR
                           : GPUQ_DECOMP_PAGE_SEGMENT;
    st->n_segs = (uint32_t)lp.segs.size();
    for (const auto& sg : lp.segs) st->n_big += sg.big != 0;
  }
  for (const auto& sg : lp.segs) {
    DevSeg d2{};
    d2.src_off = src_abs + sg.s_off;
    d2.dst_off = dst_abs + sg.d_off;
    d2.comp_len = sg.comp_len;
    d2.out_len = sg.out_len;
    d2.big = sg.big;
    cb.segs.push_back(d2);
  }
  if (lp.fallback) {
    // piece explosion: serial windowed wave per page
    DevPageBr pb{(uint32_t)cb.brs.size(), (uint32_t)lp.backrefs.size()};
    cb.pagebrs.push_back(pb);
    for (const auto& br : lp.backrefs) {
      cb.brs.push_back({dst_abs + br.dst, dst_abs + br.src, br.len, 0});
      if (st) {
        st->n_backrefs++;
        st->n_far += (br.dst - br.src) + br.len > BR_FAR;
      }
    }
    return;
  }
  // litpar pieces are literal-backed: the host can read any
  // pattern of <= 8 bytes straight from the compressed stream
  // and inline it — the replay then never touches dec sources
  auto lit_bytes = [&](uint32_t src, uint32_t len, uint8_t* out) -> bool {
    const auto& Ls = lp.lits;   // dst-ascending by construction
    size_t lo = 0, hi = Ls.size();
    while (lo < hi) {
      size_t mid = (lo + hi) / 2;
      if (Ls[mid].dst <= src) lo = mid + 1;
      else hi = mid;
    }
    if (lo == 0) return false;
    const Lz4Lit& L = Ls[lo - 1];
    if (src < L.dst || src + len > L.dst + L.len) return false;
    std::memcpy(out, praw + L.src + (src - L.dst), len);
    return true;
  };
  auto try_inline = [&](const Lz4Resolved& rr, uint64_t* pat,
                        uint32_t* period) -> bool {
    uint32_t pat_len = 0;
    for (uint32_t k = 0; k < rr.piece_n; k++)
      pat_len += lp.pieces[rr.piece_start + k].len;
    if (!lp.litpar || pat_len == 0 || pat_len > 8 || rr.len > 256)
      return false;
    uint8_t buf[8] = {0};
    uint32_t o = 0;
    for (uint32_t k = 0; k < rr.piece_n; k++) {
      const Lz4Piece& pc = lp.pieces[rr.piece_start + k];
      if (!lit_bytes(pc.src, pc.len, buf + o)) return false;
      o += pc.len;
    }
    std::memcpy(pat, buf, 8);
    *period = pat_len;
    return true;
  };
  auto push_resolved = [&](const Lz4Resolved& rr) {
    uint32_t ps = (uint32_t)cb.piece_pool.size();
    for (uint32_t k = 0; k < rr.piece_n; k++) {
      const Lz4Piece& pc = lp.pieces[rr.piece_start + k];
      cb.piece_pool.push_back({dst_abs + pc.src, pc.len, 0});
    }
    DevBrRes rec{dst_abs + rr.dst, rr.len, rr.off, ps, rr.piece_n};
    if (rr.len <= 256) cb.res_lane.push_back(rec);
    else cb.res_wave.push_back(rec);
    if (st) {
      (rr.len <= 256 ? st->n_res_lane : st->n_res_wave)++;
      st->n_pieces += rr.piece_n;
    }
  };
  // sequence tiles: a short literal run and the inlinable match behind it
  // share one record, and records with contiguous output share a tile (the
  // tile stays open across calls only through `open`, so it ends with the
  // page). Anything else interrupts the output run and so closes the tile.
  bool open = false;
  auto push_seq = [&](uint64_t dst, const DevSeq& rec, uint32_t len) {
    if (open) {
      const DevSeqTile& t = cb.tiles.back();
      if (t.dst0 + t.out_len != dst || t.n_rec == SEQ_TILE_RECS ||
          t.out_len + len > SEQ_TILE_BYTES)
        open = false;
    }
    if (!open) {
      cb.tiles.push_back({dst, (uint64_t)cb.seqs.size(), 0, 0});
      open = true;
      if (st) st->n_tile++;
    }
    cb.seqs.push_back(rec);
    cb.tiles.back().n_rec++;
    cb.tiles.back().out_len += len;
    if (st) st->n_tile_rec++;
  };
  auto match_bits = [](uint32_t len, uint32_t period) {
    return ((uint64_t)len << 49) | ((uint64_t)period << 58);
  };
  // lits and resolved are each dst-ascending and together tile the page
  size_t li = 0, ri = 0;
  const size_t nl = lp.lits.size(), nr = lp.resolved.size();
  while (li < nl || ri < nr) {
    uint64_t pat = 0;
    uint32_t period = 0;
    if (ri >= nr || (li < nl && lp.lits[li].dst < lp.resolved[ri].dst)) {
      const Lz4Lit& lt = lp.lits[li++];
      if (lt.len > 256) {
        cb.lits_wave.push_back({(src_abs + lt.src) | ((uint64_t)lt.len << 40),
                                dst_abs + lt.dst});
        if (st) st->n_lit_wave++;
        continue;
      }
      if (st) st->n_lit_lane++;
      DevSeq rec{(src_abs + lt.src) | ((uint64_t)lt.len << 40), 0};
      uint32_t len = lt.len;
      if (ri < nr && lp.resolved[ri].dst == lt.dst + lt.len &&
          try_inline(lp.resolved[ri], &pat, &period)) {
        const Lz4Resolved& rr = lp.resolved[ri++];
        rec.a |= match_bits(rr.len, period);
        rec.pat = pat;
        len += rr.len;
        if (st) st->n_inl++;
      }
      push_seq(dst_abs + lt.dst, rec, len);
    } else {
      const Lz4Resolved& rr = lp.resolved[ri++];
      if (try_inline(rr, &pat, &period)) {
        push_seq(dst_abs + rr.dst, {src_abs | match_bits(rr.len, period), pat},
                 rr.len);
        if (st) st->n_inl++;
      } else {
        push_resolved(rr);
      }
    }
  }
}

// decompress: parallel segments, then ordered backref resolution
void launch_decompress(hipStream_t st, const DecompDev& d) {
  launch_lz4_seg(st, d.d_raw, d.d_dec, d.d_segs, d.n_segs, d.d_err);
  // litpar pages: sequence tiles (short literals + inlined matches) and
  // flat long-literal copies, independent of the segment pass
  launch_seq_tile(st, d.d_raw, d.d_dec, d.d_seqs, d.d_tiles, d.n_tiles,
                  d.seq_batch);
  launch_lit_wave(st, d.d_raw, d.d_dec, d.d_lits_wave, d.n_lits_wave);
  // deferred-match resolution: host-resolved records are independent —
  // one launch each (kernel boundary after phase 1 gives coherence; their
  // pieces read bytes the tiles produce); piece-explosion pages fall back
  // to the serial windowed wave
  launch_brres_lane(st, d.d_dec, d.d_res_lane, d.d_piece_pool, d.n_res_lane);
  launch_brres_wave(st, d.d_dec, d.d_res_wave, d.d_piece_pool, d.n_res_wave);
  launch_lz4_backrefs(st, d.d_dec, d.d_brs, d.d_pagebrs, d.n_pagebrs);
}

// GPUQ_PLAN_DEBUG report
void plan_debug_report(gpuq_plan* plan,
                       std::map<size_t, std::array<int64_t, 3>>& null_dbg,
                       const std::vector<std::array<int64_t, 2>>& leaf_dbg,
                       const std::vector<char>& or_path) {
  fprintf(stderr, "[gpuq plan] fused_count=%d fused_valagg=%d%s\n",
          (int)plan->fused_count, (int)plan->fused_valagg,
          plan->fused_valagg && plan->valagg_late
              ? " (group count checked at execute)" : "");
  for (int ai : plan->distinct_aggs) {
    const auto& c = plan->cols[plan->aggs[ai].col_idx];
    fprintf(stderr, "[gpuq plan] distinct agg=%d col=%s gids=%s\n", ai,
            c.name.c_str(),
            c.numeric_key ? "numeric" : c.hash_mode ? "hash" : "dict");
  }
  for (size_t p = 0; p < plan->parts.size(); p++) {
    const auto& pt = plan->parts[p];
    // matches an 8 B record could hold: minimal period <= 3
    size_t period_le3 = 0;
    for (const DevSeq& r : pt.seqs) {
      const uint32_t ml = (uint32_t)(r.a >> 49) & 0x1ff;
      const uint32_t n = std::min(ml, (uint32_t)(r.a >> 58));
      for (uint32_t q = 1; q <= 3 && ml; q++) {
        bool ok = true;
        for (uint32_t j = q; j < n && ok; j++)
          ok = (uint8_t)(r.pat >> (j * 8)) == (uint8_t)(r.pat >> ((j - q) * 8));
        if (ok) { period_le3++; break; }
      }
    }
    fprintf(stderr,
            "[gpuq plan] part %zu: rows=%lld chunks=%zu pages=%zu segs=%zu "
            "tiles=%zu tile_recs=%zu period_le3=%zu lits_wave=%zu "
            "res=%zu/%zu pieces=%zu raw=%.2fGB "
            "dec=%.2fGB cwins=%zu fork_cols=%zu early_segs=%zu "
            "early_tiles=%zu early_tile_recs=%zu early_lits_wave=%zu "
            "early_res=%zu/%zu early_pagebrs=%zu\n",
            p, (long long)pt.n_rows, pt.chunks.size(), pt.pages.size(),
            pt.segs.size(), pt.tiles.size(), pt.seqs.size(), period_le3,
            pt.lits_wave.size(), pt.res_lane.size(), pt.res_wave.size(),
            pt.piece_pool.size(), pt.raw_bytes / 1e9, pt.dec_bytes / 1e9,
            pt.cwins.size(), pt.fork_cols.size(), pt.early.segs.size(),
            pt.early.tiles.size(), pt.early.seqs.size(),
            pt.early.lits_wave.size(), pt.early.res_lane.size(),
            pt.early.res_wave.size(), pt.early.pagebrs.size());
  }
  // one line per string / null predicate: the path that evaluates it
  for (size_t pi = 0; pi < plan->preds.size(); pi++) {
    const auto& pp = plan->preds[pi];
    std::string path;
    if (op_is_like(pp.p.op)) {
      int ci = find_or_add_col(plan->cols, pp.col);
      if (plan->cols[ci].hash_mode) {
        path = "hash";
      } else {
        bool lut = false, win = false;
        int k = plan->ctx_of((int)pi);
        if (k < 0)  // folded into the LUT of its OR group's context
          for (auto& f : plan->wfolds)
            if (f.col == ci) k = f.ctx;
        for (auto& part : plan->parts) {
          lut |= part.tasks.count({tk_ctx(TK_DICT_MASK, k), ci}) != 0;
          win |= part.tasks.count({tk_ctx(TK_BYTES_CONTAINS, k), ci}) != 0;
        }
        path = lut && win ? "lut+window" : win ? "window" : lut ? "lut" : "pruned";
      }
      // op= is the op as given; a canonicalised pattern names the op it runs as
      std::string as;
      if (pp.orig_op != pp.p.op) as = std::string(" as=") + op_name(pp.p.op);
      fprintf(stderr, "[gpuq plan] pred %zu col=%s op=%s path=%s%s\n", pi,
              pp.col.c_str(), op_name(pp.orig_op), path.c_str(), as.c_str());
    } else if (op_is_null(pp.p.op)) {
      const auto& n = null_dbg[pi];
      static const char* nm[] = {"nulltask", "proven", "pruned"};
      for (int k = 0; k < 3; k++)
        if (n[k]) path += (path.empty() ? "" : "+") + std::string(nm[k]);
      if (path.empty()) path = "pruned";
      fprintf(stderr,
              "[gpuq plan] pred %zu col=%s op=%s path=%s rowgroups: "
              "nulltask=%lld proven=%lld pruned=%lld\n",
              pi, pp.col.c_str(), op_name(pp.p.op), path.c_str(),
              (long long)n[0], (long long)n[1], (long long)n[2]);
    }
  }
  if (plan->has_tree) {
    fprintf(stderr, "[gpuq plan] where %s contexts=%zu depth=%d\n",
            where_expr(plan->where, plan->where.root).c_str(),
            plan->ctxs.size(), plan->where.depth);
    for (const auto& f : plan->filters)
      fprintf(stderr, "[gpuq plan] agg %d filter %s ctx=%d depth=%d\n", f.agg,
              where_expr(plan->where, f.root).c_str(), f.ctx, f.depth);
    // per leaf: its mask context (-1: folded into a LUT) and how many row
    // groups evaluate it per row — elision holds inside an OR as well
    for (size_t pi = 0; pi < plan->preds.size(); pi++)
      fprintf(stderr,
              "[gpuq plan] where pred %zu col=%s op=%s ctx=%d rowgroups: "
              "eval=%lld elided=%lld\n",
              pi, plan->preds[pi].col.c_str(),
              op_name(plan->preds[pi].orig_op), plan->pred_ctx[pi],
              (long long)leaf_dbg[pi][0],
              (long long)leaf_dbg[pi][1]);
    for (size_t ni = 0; ni < plan->where.nodes.size(); ni++)
      if (plan->where.nodes[ni].kind == GPUQ_NODE_OR)
        fprintf(stderr, "[gpuq plan] or node=%zu terms=%zu path=%s\n", ni,
                plan->where.nodes[ni].kids.size(),
                or_path[ni] == 'l' ? "lut" : "mask");
  }
}

}  // namespace

extern "C" gpuq_plan* gpuq_plan_build(
    gpuq_ctx* ctx, const gpuq_file* files, int32_t n_files,
    const char* const* projection, int32_t n_projection,
    const gpuq_pred* preds, int32_t n_preds,
    const char* const* group_by, int32_t n_group_by,
    const gpuq_agg* aggs, int32_t n_aggs, int64_t limit) {
  return gpuq_plan_build_where(ctx, files, n_files, projection, n_projection,
                               preds, n_preds, group_by, n_group_by, aggs,
                               n_aggs, limit, nullptr, 0);
}

extern "C" gpuq_plan* gpuq_plan_build_where(
    gpuq_ctx* ctx, const gpuq_file* files, int32_t n_files,
    const char* const* projection, int32_t n_projection,
    const gpuq_pred* preds, int32_t n_preds,
    const char* const* group_by, int32_t n_group_by,
    const gpuq_agg* aggs, int32_t n_aggs, int64_t limit,
    const gpuq_where_node* nodes, int32_t n_nodes) {
  return gpuq_plan_build_filtered(ctx, files, n_files, projection,
                                  n_projection, preds, n_preds, group_by,
                                  n_group_by, aggs, n_aggs, limit, nodes,
                                  n_nodes, nullptr, 0);
}

extern "C" gpuq_plan* gpuq_plan_build_filtered(
    gpuq_ctx* ctx, const gpuq_file* files, int32_t n_files,
    const char* const* projection, int32_t n_projection,
    const gpuq_pred* preds, int32_t n_preds,
    const char* const* group_by, int32_t n_group_by,
    const gpuq_agg* aggs, int32_t n_aggs, int64_t limit,
    const gpuq_where_node* nodes, int32_t n_nodes,
    const gpuq_agg_filter* filters, int32_t n_filters) try {
  (void)projection; (void)n_projection;
  auto plan = std::make_unique<gpuq_plan>();
  plan->ctx = ctx;
  plan->limit = limit;
  read_env_knobs(plan.get());
  if (ctx->devices.empty())
    throw std::runtime_error("no GPU devices in session (gpuq never falls back to CPU)");
  if (n_files <= 0)
    throw std::runtime_error("empty file list: caller should use the empty-relation path "
                             "(provider returns the empty aggregate without a scan)");

  // --- map files + parse footers (parallel: 1 B rows ≈ 3,815 files) ---
  plan->files.resize(n_files);
  parallel_for((size_t)n_files, [&](size_t i) {
    auto mf = std::make_unique<MappedFile>();
    mf->path = files[i].path;
    mf->fd = open(files[i].path, O_RDONLY);
    if (mf->fd < 0) throw std::runtime_error("cannot open " + mf->path);
    struct stat st;
    fstat(mf->fd, &st);
    mf->size = st.st_size;
    mf->mtime_ns = (int64_t)st.st_mtim.tv_sec * 1000000000 + st.st_mtim.tv_nsec;
    mf->data = (const uint8_t*)mmap(nullptr, mf->size, PROT_READ, MAP_PRIVATE, mf->fd, 0);
    if (mf->data == MAP_FAILED) throw std::runtime_error("mmap failed: " + mf->path);
    mf->meta = parse_footer(mf->data, mf->size);
    plan->files[i] = std::move(mf);
  });
  const FileMeta& fm0 = plan->files[0]->meta;

  // --- query spec -> column roles ---
  for (int32_t i = 0; i < n_preds; i++) {
    PredPlan pp;
    pp.p = preds[i];
    pp.col = preds[i].column;
    if (pp.p.op < GPUQ_EQ || pp.p.op > GPUQ_NOT_ILIKE)
      throw std::runtime_error("unknown predicate op on " + pp.col);
    pp.orig_op = pp.p.op;
    // a null op carries no literal: its lit_kind/str/i64/f64 are not read
    if (!op_is_null(pp.p.op) && preds[i].str) pp.str_lit = preds[i].str;
    plan->preds.push_back(std::move(pp));
  }
  // WHERE tree: validated always; kept only when it is not a pure
  // conjunction, so such a tree builds exactly the flat plan
  // Filter trees join the WHERE tree's node list as a forest; a plan with
  // filters keeps its tree even when WHERE is a pure conjunction.
  std::vector<int> filter_of_agg(std::max(n_aggs, 0), -1);
  {
    QueryTrees qt = where_normalise_filtered(nodes, n_nodes, n_preds, filters,
                                             n_filters, n_aggs,
                                             n_projection > 0);
    if (!qt.where.conj || !qt.filters.empty()) {
      plan->has_tree = true;
      plan->where = std::move(qt.where);
    }
    plan->pred_filter.assign(plan->preds.size(), -1);
    for (auto& ft : qt.filters) {
      const int j = (int)plan->filters.size();
      const int base = (int)plan->where.nodes.size();
      const int root = where_append(plan->where, ft.tree);
      for (size_t ni = base; ni < plan->where.nodes.size(); ni++)
        if (plan->where.nodes[ni].kind == GPUQ_NODE_LEAF)
          plan->pred_filter[plan->where.nodes[ni].pred] = j;
      plan->filters.push_back({ft.agg, root, -1, ft.tree.depth});
      filter_of_agg[ft.agg] = j;
    }
  }
  for (int32_t i = 0; i < n_group_by; i++) {
    std::string g = group_by[i];
    if (g.rfind("__bin:", 0) == 0) {
      // "__bin:<col>:<stride_ms>:<origin>" — DATE_BIN time bins
      size_t a = 6, b = g.find(':', a), c2 = g.find(':', b + 1);
      std::string src = g.substr(a, b - a);
      int ci = find_or_add_col(plan->cols, g);
      auto& bc = plan->cols[ci];
      bc.is_bin = true;
      bc.bin_stride = std::stoll(g.substr(b + 1, c2 - b - 1));
      bc.bin_origin = std::stoll(g.substr(c2 + 1));
      if (bc.bin_stride <= 0) throw std::runtime_error("bad bin stride");
      int si = find_or_add_col(plan->cols, src);
      plan->cols[si].need_val = true;
      plan->cols[si].val_always = true;
      plan->cols[ci].bin_src = si;
      plan->group_cols.push_back(ci);
      continue;
    }
    int ci = find_or_add_col(plan->cols, g);
    plan->cols[ci].need_gid = true;
    plan->group_cols.push_back(ci);
  }
  for (int32_t i = 0; i < n_aggs; i++) {
    AggPlan ap;
    ap.op = aggs[i].op;
    ap.filter = filter_of_agg[i];
    if (aggs[i].op == GPUQ_AGG_COUNT_DISTINCT) {
      if (!aggs[i].column)
        throw std::runtime_error("count_distinct needs a column");
      if (n_projection > 0)
        throw std::runtime_error(
            "count_distinct is not allowed in a projection plan");
    }
    if (aggs[i].op != GPUQ_AGG_COUNT_STAR) {
      ap.col = aggs[i].column;
      ap.col_idx = find_or_add_col(plan->cols, ap.col);
    }
    plan->aggs.push_back(std::move(ap));
  }
  // resolve column phys types from schema + route predicates
  for (auto& c : plan->cols) {
    if (c.is_bin) continue;
    int si = fm0.col_index(c.name);
    if (si < 0) throw std::runtime_error("no such column: " + c.name);
    c.phys = fm0.columns[si].phys_type;
    c.optional = fm0.columns[si].optional;
    if (c.need_gid && c.phys != PT_BYTE_ARRAY) {
      if (c.phys == PT_INT64 || c.phys == PT_INT32 || c.phys == PT_DOUBLE) {
        // numeric group key: DataFusion's row-hash groups by any column —
        // dense gids come from hashing the decoded values (k_numhash_*)
        c.need_gid = false;
        c.numeric_key = true;
        c.need_val = true;
        c.val_always = true;
        plan->has_numkey = true;
      } else {
        throw std::runtime_error(
            "unsupported group-key type (utf8/i64/i32/f64/timestamp): " +
            c.name);
      }
    }
  }
  for (size_t pi = 0; pi < plan->preds.size(); pi++) {
    auto& pp = plan->preds[pi];
    int ci = find_or_add_col(plan->cols, pp.col);
    auto& c = plan->cols[ci];
    if (c.phys == -1) {
      int si = fm0.col_index(c.name);
      if (si < 0) throw std::runtime_error("no such column: " + c.name);
      c.phys = fm0.columns[si].phys_type;
      c.optional = fm0.columns[si].optional;
    }
    if (op_is_null(pp.p.op)) {
      if (c.phys != PT_BYTE_ARRAY && c.phys != PT_INT64 &&
          c.phys != PT_INT32 && c.phys != PT_DOUBLE)
        throw std::runtime_error("unsupported predicate column type: " + pp.col);
      c.null_preds.push_back((int)pi);
      continue;
    }
    if (op_is_pattern(pp.p.op) && pp.p.lit_kind != GPUQ_LIT_STR)
      throw std::runtime_error(std::string(op_name(pp.p.op)) +
                               " needs a string literal: " + pp.col);
    if (op_is_like(pp.p.op) && pp.p.op != GPUQ_CONTAINS &&
        c.phys != PT_BYTE_ARRAY)
      throw std::runtime_error(std::string("string predicate ") +
                               op_name(pp.p.op) + " on non-utf8 column: " +
                               pp.col);
    if (c.phys == PT_BYTE_ARRAY) {
      if (pp.p.lit_kind != GPUQ_LIT_STR)
        throw std::runtime_error("string column needs string literal: " + pp.col);
      if (op_is_pattern(pp.p.op)) {
        compile_pattern_pred(pp);
      } else if (op_is_like(pp.p.op) && (like_mode(pp.p.op) & STRF_FOLD)) {
        // ASCII-only folding: lower-case the needle once here; a literal
        // with a byte >= 0x80 would need Unicode case mapping on both sides
        for (char& ch : pp.str_lit) {
          if ((unsigned char)ch >= 0x80)
            throw std::runtime_error(
                std::string(op_name(pp.p.op)) + " literal must be ASCII "
                "(case folding is ASCII-only): " + pp.col);
          if (ch >= 'A' && ch <= 'Z') ch = (char)(ch | 0x20);
        }
      }
      if (op_is_like(pp.p.op)) c.contains_preds.push_back((int)pi);
      c.lut_preds.push_back((int)pi);   // dict pages via LUT (incl. contains)
    } else if (c.phys == PT_INT64 || c.phys == PT_INT32) {
      if (pp.p.lit_kind != GPUQ_LIT_I64)
        throw std::runtime_error("int column needs int literal: " + pp.col);
      c.cmp_preds.push_back((int)pi);
      c.need_val = true;
    } else if (c.phys == PT_DOUBLE) {
      if (pp.p.lit_kind != GPUQ_LIT_F64)
        throw std::runtime_error("double column needs float literal: " + pp.col);
      c.cmp_preds.push_back((int)pi);
      c.need_val = true;
    } else {
      throw std::runtime_error("unsupported predicate column type: " + pp.col);
    }
  }
  // aggregate kinds
  for (auto& ap : plan->aggs) {
    if (ap.op == GPUQ_AGG_COUNT_STAR) {
      // a filtered count(*) is not the presence count: it counts into its own
      // count slot, as a count over a column without a validity array does
      ap.kind = ap.filter >= 0 ? AGGK_COUNT : AGGK_COUNT_STAR;
      continue;
    }
    auto& c = plan->cols[ap.col_idx];
    ap.is_f64 = (c.phys == PT_DOUBLE || c.phys == PT_FLOAT);
    if (ap.op == GPUQ_AGG_COUNT_DISTINCT) {
      // the value column gets a dense gid per row the way a group key does:
      // dict utf8 via the global dictionary (hash mode is decided below,
      // with the keys), numeric via the value hash
      ap.kind = AGGK_COUNT_DISTINCT;
      c.distinct_val = true;
      if (c.phys == PT_BYTE_ARRAY) {
        c.need_gid = true;
      } else if (c.phys == PT_INT64 || c.phys == PT_INT32 ||
                 c.phys == PT_DOUBLE) {
        c.numeric_key = true;
        c.need_val = true;
        c.val_always = true;
        plan->has_numkey = true;
      } else {
        throw std::runtime_error(
            "unsupported count_distinct column type "
            "(utf8/i64/i32/f64/timestamp): " + ap.col);
      }
      plan->distinct_aggs.push_back((int)(&ap - plan->aggs.data()));
      continue;
    }
    if (c.phys == PT_BYTE_ARRAY && ap.op == GPUQ_AGG_SUM)
      throw std::runtime_error("sum over utf8 column: " + ap.col);
    if (c.phys == PT_BYTE_ARRAY) {
      if (ap.op == GPUQ_AGG_COUNT) {        // COUNT(utf8): validity only
        c.need_gid = true;
        c.need_gid_valid = true;
      } else {                              // utf8 min/max via dict sort-ranks
        c.need_val = true;
        c.val_always = true;
        c.need_rank = true;
      }
    } else {
      c.need_val = true;
      c.val_always = true;
    }
    switch (ap.op) {
      case GPUQ_AGG_COUNT: ap.kind = AGGK_COUNT; break;
      case GPUQ_AGG_SUM:
        ap.kind = ap.is_f64 ? AGGK_SUM_F64 : AGGK_SUM_I64;
        if (ap.is_f64) ap.fsum_idx = plan->n_fsum++;
        break;
      case GPUQ_AGG_MIN:
        ap.kind = (c.phys == PT_BYTE_ARRAY) ? AGGK_MIN_RANK
                  : ap.is_f64 ? AGGK_MIN_F64 : AGGK_MIN_I64;
        break;
      case GPUQ_AGG_MAX:
        ap.kind = (c.phys == PT_BYTE_ARRAY) ? AGGK_MAX_RANK
                  : ap.is_f64 ? AGGK_MAX_F64 : AGGK_MAX_I64;
        break;
      default: throw std::runtime_error("bad agg op");
    }
  }
  if (plan->aggs.empty()) {
    // projection scan: SELECT cols ... ORDER BY p_timestamp DESC LIMIT k
    // (the console's default query; ordering contract
    // stream_schema_provider.rs:181-204 — time-DESC is implied)
    if (n_projection <= 0)
      throw std::runtime_error("projection scans need a column list");
    // limit < 0 = unlimited: the result is exported as a true multi-batch
    // ArrowArrayStream in 20k-row batches (P_EXECUTION_BATCH_SIZE,
    // cli.rs:476-482) — see execute_projection
    plan->is_projection = true;
    for (int32_t i = 0; i < n_projection; i++) {
      int ci = find_or_add_col(plan->cols, projection[i]);
      plan->projection.push_back(ci);
      auto& c = plan->cols[ci];
      if (c.phys == -1) {
        int si = fm0.col_index(c.name);
        if (si < 0) throw std::runtime_error("no such column: " + c.name);
        c.phys = fm0.columns[si].phys_type;
        c.optional = fm0.columns[si].optional;
      }
      if (c.phys == PT_BYTE_ARRAY) c.need_gid = true;     // export via dict
      else { c.need_val = true; c.val_always = true; }    // i64/f64 direct
    }
    int tci = find_or_add_col(plan->cols, "p_timestamp");
    {
      auto& tc = plan->cols[tci];
      if (tc.phys == -1) {
        int si = fm0.col_index("p_timestamp");
        if (si < 0) throw std::runtime_error("no p_timestamp column");
        tc.phys = fm0.columns[si].phys_type;
        tc.optional = fm0.columns[si].optional;
      }
      tc.need_val = true;
      tc.val_always = true;
    }
    plan->ts_col = tci;
  }
  if (plan->group_cols.size() > (size_t)MAX_KEYS || plan->aggs.size() > (size_t)MAX_AGGS)
    throw std::runtime_error("too many keys/aggregates");
  // the value decoders read INT32, INT64 and DOUBLE (4- or 8-byte PLAIN,
  // dictionary, delta for the ints) and BYTE_ARRAY; BOOLEAN's bit-packed
  // values, FLOAT, INT96 and fixed-length byte arrays have no decoder, and
  // the 8-byte copy would return garbage for them
  for (const auto& c : plan->cols) {
    if (c.is_bin || c.phys == -1) continue;
    if (c.phys != PT_INT32 && c.phys != PT_INT64 && c.phys != PT_DOUBLE &&
        c.phys != PT_BYTE_ARRAY) {
      static const char* names[] = {"BOOLEAN", "INT32", "INT64", "INT96",
                                    "FLOAT", "DOUBLE", "BYTE_ARRAY",
                                    "FIXED_LEN_BYTE_ARRAY"};
      throw std::runtime_error(
          "unsupported column type " +
          std::string(c.phys >= 0 && c.phys < 8 ? names[c.phys] : "?") +
          " (INT32/INT64/DOUBLE/BYTE_ARRAY only): " + c.name);
    }
  }

  // --- select row groups (caller's list + footer-stats pruning) ---
  std::vector<RgRef> selected;
  // per null predicate: row groups by NullState (plan debug line)
  std::map<size_t, std::array<int64_t, 3>> null_dbg;
  // per leaf: row groups evaluated per row / proven by chunk stats (the
  // WHERE-tree plan debug lines)
  std::vector<std::array<int64_t, 2>> leaf_dbg(plan->preds.size(),
                                               std::array<int64_t, 2>{0, 0});
  for (int32_t i = 0; i < n_files; i++) {
    const auto& mf = *plan->files[i];
    std::vector<int32_t> rg_list;
    if (files[i].row_groups && files[i].n_row_groups >= 0)
      rg_list.assign(files[i].row_groups, files[i].row_groups + files[i].n_row_groups);
    else
      for (size_t g = 0; g < mf.meta.row_groups.size(); g++) rg_list.push_back((int32_t)g);
    for (int32_t g : rg_list) {
      const auto& rg = mf.meta.row_groups[g];
      if (rg_pruned_by_stats(*plan, mf.meta, rg)) {
        // debug accounting: which null predicates dropped this row group
        for (size_t pi = 0; pi < plan->preds.size(); pi++) {
          const auto& pp = plan->preds[pi];
          if (!op_is_null(pp.p.op)) continue;
          int si = mf.meta.col_index(pp.col);
          if (si >= 0 && null_pred_state(pp.p.op, rg.chunks[si],
                                         mf.meta.columns[si].optional) == NULLP_UNSAT)
            null_dbg[pi][NULLP_UNSAT]++;
        }
        continue;
      }
      RgRef r;
      r.file_idx = i;
      r.rg_idx = g;
      r.rows = rg.num_rows;
      r.total_bytes = rg.total_compressed_size;
      for (auto& c : plan->cols) {
        int si = mf.meta.col_index(c.name);
        if (si >= 0) r.needed_bytes += rg.chunks[si].total_compressed_size;
      }
      selected.push_back(r);
    }
  }

  // --- byte-balanced assignment to devices (balanced_file_groups,
  //     stream_schema_provider.rs:146-165: greedy into least-loaded group) ---
  int n_parts = (int)ctx->devices.size();
  plan->parts.resize(n_parts);
  for (int p = 0; p < n_parts; p++) plan->parts[p].device = ctx->devices[p];
  std::vector<int64_t> load(n_parts, 0);
  std::stable_sort(selected.begin(), selected.end(),
                   [](const RgRef& a, const RgRef& b) { return a.needed_bytes > b.needed_bytes; });
  for (auto& r : selected) {
    int best = 0;
    for (int p = 1; p < n_parts; p++) if (load[p] < load[best]) best = p;
    load[best] += r.needed_bytes;
    plan->parts[best].rgs.push_back(r);
  }

  // --- raw-byte utf8 (hash-mode) detection: a utf8 column used as group
  // key / min-max / non-LIKE predicate whose selected chunks contain
  // PLAIN-fallback data pages cannot ride the dict-only gid path. Decided
  // BEFORE the per-partition build so every partition routes consistently.
  // (LIKE alone stays on the contains-window path: it handles PLAIN pages
  // already and is much faster than per-row byte scans.) ---
  // The same walk tells whether an OR group over one utf8 column can fold
  // into that column's LUT (below): only a column without PLAIN pages can.
  // or_col(node): the one utf8 column whose string ops are all the leaves
  // below `node`, else -1.
  std::function<int(int)> or_col = [&](int ni) -> int {
    const WNode& n = plan->where.nodes[ni];
    if (n.kind == GPUQ_NODE_LEAF) {
      const auto& pp = plan->preds[n.pred];
      if (op_is_null(pp.p.op)) return -1;
      int ci = find_or_add_col(plan->cols, pp.col);
      return plan->cols[ci].phys == PT_BYTE_ARRAY ? ci : -1;
    }
    int col = -2;
    for (int k : n.kids) {
      int kc = or_col(k);
      if (kc < 0 || (col != -2 && kc != col)) return -1;
      col = kc;
    }
    return col;
  };
  std::vector<uint8_t> fold_cand(plan->cols.size(), 0),
      probe_hash(plan->cols.size(), 0), col_plain(plan->cols.size(), 0);
  if (plan->has_tree)
    for (size_t ni = 0; ni < plan->where.nodes.size(); ni++)
      if (plan->where.nodes[ni].kind == GPUQ_NODE_OR) {
        int ci = or_col((int)ni);
        if (ci >= 0) fold_cand[ci] = 1;
      }
  {
    struct Probe { int col; const MappedFile* mf; const ColumnChunkMeta* cm; int64_t rows; };
    std::vector<Probe> probes;
    for (size_t ci = 0; ci < plan->cols.size(); ci++) {
      auto& c = plan->cols[ci];
      if (c.is_bin || c.phys != PT_BYTE_ARRAY) continue;
      bool non_like = false;
      for (int pidx : c.lut_preds)
        non_like |= !op_is_like(plan->preds[pidx].p.op);
      if (!(c.need_gid || c.need_rank || non_like || fold_cand[ci])) continue;
      probe_hash[ci] = c.need_gid || c.need_rank || non_like;
      for (auto& r : selected) {
        const auto& mf = *plan->files[r.file_idx];
        int si = mf.meta.col_index(c.name);
        if (si < 0) continue;
        probes.push_back({(int)ci, &mf,
                          &mf.meta.row_groups[r.rg_idx].chunks[si],
                          mf.meta.row_groups[r.rg_idx].num_rows});
      }
    }
    std::vector<uint8_t> plain(probes.size(), 0);
    parallel_for(probes.size(), [&](size_t i) {
      auto pages = walk_pages(probes[i].mf->data, *probes[i].cm, probes[i].rows);
      for (auto& pi : pages)
        if (pi.type == PAGE_DATA && pi.encoding == ENC_PLAIN) plain[i] = 1;
    });
    for (size_t i = 0; i < probes.size(); i++)
      if (plain[i]) {
        col_plain[probes[i].col] = 1;
        if (probe_hash[probes[i].col]) plan->cols[probes[i].col].hash_mode = true;
      }
    for (size_t ci = 0; ci < plan->cols.size(); ci++) {
      auto& c = plan->cols[ci];
      if (!c.hash_mode) continue;
      plan->has_hash = true;
      c.need_val = true;       // d_val carries row strrefs
      c.val_always = true;
      if (c.need_rank) {       // min/max via strref byte compares
        c.need_rank = false;
        for (auto& ap : plan->aggs)
          if (ap.col_idx == (int)ci) {
            if (ap.kind == AGGK_MIN_RANK) ap.kind = AGGK_MIN_STR;
            if (ap.kind == AGGK_MAX_RANK) ap.kind = AGGK_MAX_STR;
          }
      }
      bool is_key = c.distinct_val;  // gids from the hash build, like a key
      for (int gci : plan->group_cols) is_key |= (gci == (int)ci);
      if (!is_key) { c.need_gid = false; c.need_gid_valid = false; }
    }
  }

  // --- WHERE tree -> mask contexts. Every term of an OR group becomes a
  // context of its own (one mask buffer evaluation), except an OR group
  // over a single LUT-only utf8 column: that one folds into the column's
  // LUT in the parent's context — the tree is evaluated per dictionary
  // entry at plan build and costs one TK_DICT_MASK task, no buffer, no
  // combine pass (the IN-list shape, level = 'a' OR level = 'b'). ---
  std::vector<char> or_path(plan->where.nodes.size(), 0);  // 'l' lut, 'm' mask
  if (plan->has_tree) {
    plan->pred_ctx.assign(plan->preds.size(), 0);
    plan->ctxs.emplace_back();
    std::function<void(int, char)> mark_folded = [&](int ni, char tag) {
      const WNode& n = plan->where.nodes[ni];
      if (n.kind == GPUQ_NODE_LEAF) { plan->pred_ctx[n.pred] = -1; return; }
      if (n.kind == GPUQ_NODE_OR) or_path[ni] = tag;
      for (int k : n.kids) mark_folded(k, tag);
    };
    // ni: an AND group or a single leaf evaluated in context k, whose OR
    // children sit at nesting level `level`
    std::function<void(int, int, int)> assign = [&](int ni, int k, int level) {
      const WNode& n = plan->where.nodes[ni];
      if (n.kind == GPUQ_NODE_LEAF) { plan->pred_ctx[n.pred] = k; return; }
      for (int kid : n.kids) {
        const WNode& kn = plan->where.nodes[kid];
        if (kn.kind == GPUQ_NODE_LEAF) { plan->pred_ctx[kn.pred] = k; continue; }
        // normal form: the child of an AND is an OR
        int fc = or_col(kid);
        if (fc >= 0 && !plan->cols[fc].hash_mode && !col_plain[fc]) {
          mark_folded(kid, 'l');
          plan->wfolds.push_back({kid, k, fc});
          continue;
        }
        or_path[kid] = 'm';
        gpuq_plan::WOr wo;
        wo.node = kid; wo.ctx = k; wo.level = level;
        plan->n_wbufs = std::max(plan->n_wbufs, 2 * (level + 1));
        for (int term : kn.kids) {
          int k2 = (int)plan->ctxs.size();
          plan->ctxs.emplace_back();
          wo.terms.push_back(k2);
          assign(term, k2, level + 1);
        }
        plan->wors.push_back(std::move(wo));
        plan->ctxs[k].ors.push_back((int)plan->wors.size() - 1);
      }
    };
    assign(plan->where.root, 0, 0);
    // one context per filter; its nested ORs reuse the level pairs of
    // d_wbufs, trees being evaluated one after another
    for (auto& f : plan->filters) {
      f.ctx = (int)plan->ctxs.size();
      plan->ctxs.emplace_back();
      assign(f.root, f.ctx, 0);
    }
  }
  // LUT slots per column: the contexts holding a LUT leaf or a folded group
  for (size_t ci = 0; ci < plan->cols.size(); ci++) {
    auto& c = plan->cols[ci];
    if (c.lut_preds.empty()) continue;
    if (!plan->has_tree) { c.lut_ctxs = {0}; continue; }
    for (int pidx : c.lut_preds)
      if (plan->pred_ctx[pidx] >= 0) c.lut_ctxs.push_back(plan->pred_ctx[pidx]);
    for (auto& f : plan->wfolds)
      if (f.col == (int)ci) c.lut_ctxs.push_back(f.ctx);
    std::sort(c.lut_ctxs.begin(), c.lut_ctxs.end());
    c.lut_ctxs.erase(std::unique(c.lut_ctxs.begin(), c.lut_ctxs.end()),
                     c.lut_ctxs.end());
  }
  // one dictionary entry against the LUT of (column ci, context k): the AND
  // of the context's leaves on the column and of its folded groups
  std::function<bool(int, const uint8_t*, uint32_t)> eval_fold =
      [&](int ni, const uint8_t* q, uint32_t l) -> bool {
    const WNode& n = plan->where.nodes[ni];
    if (n.kind == GPUQ_NODE_LEAF) {
      const auto& pp = plan->preds[n.pred];
      return eval_str_pred(pp.p, pp.str_lit, q, l);
    }
    for (int k : n.kids) {
      bool v = eval_fold(k, q, l);
      if (n.kind == GPUQ_NODE_OR ? v : !v) return v;
    }
    return n.kind == GPUQ_NODE_AND;
  };
  auto lut_entry = [&](int ci, int k, const uint8_t* q, uint32_t l) -> uint8_t {
    for (int pidx : plan->cols[ci].lut_preds) {
      if (plan->ctx_of(pidx) != k) continue;
      const auto& pp = plan->preds[pidx];
      if (!eval_str_pred(pp.p, pp.str_lit, q, l)) return 0;
    }
    for (auto& f : plan->wfolds)
      if (f.col == ci && f.ctx == k && !eval_fold(f.node, q, l)) return 0;
    return 1;
  };

  // --- per-partition host build: page walks, dict processing, device
  // images. The 1 B-row configs have thousands of (row-group x column)
  // chunks: every per-chunk pass below (page-header walks, dict-page
  // decompress, LZ4 structure walks) runs parallel across host cores, with
  // serial phases only for global-dict id assignment and the
  // order-preserving merges into the device pools. ---
  int64_t tphase = now_ns();
  auto phase_mark = [&](const char* name) {
    if (!plan->exec_dbg) return;
    int64_t t = now_ns();
    fprintf(stderr, "[gpuq plan] %-22s %7.1f ms\n", name,
            (t - tphase) / 1e6);
    tphase = t;
  };
  for (auto& part : plan->parts) {
    uint32_t row_cursor = 0;
    for (auto& r : part.rgs) {
      r.row_start = row_cursor;
      row_cursor += (uint32_t)r.rows;
      part.rowgroup_bytes_total += r.total_bytes;
    }
    part.n_rows = row_cursor;

    // chunk stubs (serial, cheap): raw-arena offsets + byte accounting +
    // chunk-stats predicate elision (pred_all_true): a predicate proven for
    // every row of a row group keeps the memset-1 mask there — no per-row
    // evaluation, and predicate-only columns skip decode for that chunk.
    struct Stub {
      int file_idx, rg_idx, col_idx;
      const ColumnChunkMeta* cm;
      uint64_t raw_off;
      uint32_t rstart;
      bool need_val_decode;
      // null preds the footer left open: (TK_IS_NULL | TK_IS_NOT_NULL,
      // mask context), each once
      std::vector<std::pair<int, int>> null_tasks;
    };
    std::vector<Stub> stubs;
    for (auto& r : part.rgs) {
      const auto& mf = *plan->files[r.file_idx];
      const auto& rg = mf.meta.row_groups[r.rg_idx];
      // which predicates still need per-row evaluation in this row group
      std::vector<bool> pred_eval(plan->preds.size(), false);
      for (size_t pi2 = 0; pi2 < plan->preds.size(); pi2++) {
        const auto& pp = plan->preds[pi2];
        int si = mf.meta.col_index(pp.col);
        bool elided = false;
        if (si >= 0)
          elided = pred_all_true(pp.p, rg.chunks[si],
                                 mf.meta.columns[si].optional);
        pred_eval[pi2] = !elided;
        leaf_dbg[pi2][elided ? 1 : 0]++;
        if (op_is_null(pp.p.op))
          null_dbg[pi2][elided ? NULLP_PROVEN : NULLP_EVAL]++;
        if (!elided) {
          auto& rv = part.pred_ranges[(int)pi2];
          int64_t lo2 = r.row_start, n2 = r.rows;
          if (!rv.empty() && rv.back().first + rv.back().second == lo2)
            rv.back().second += n2;  // merge adjacent row groups
          else
            rv.emplace_back(lo2, n2);
        }
      }
      for (size_t ci = 0; ci < plan->cols.size(); ci++) {
        auto& c = plan->cols[ci];
        if (c.is_bin) continue;
        int si = mf.meta.col_index(c.name);
        if (si < 0) throw std::runtime_error("column missing in file: " + c.name);
        const auto& cm = rg.chunks[si];
        bool needs_val = c.val_always;
        for (int pidx : c.cmp_preds) needs_val |= pred_eval[pidx];
        std::vector<std::pair<int, int>> null_tasks;
        for (int pidx : c.null_preds) {
          if (!pred_eval[pidx]) continue;
          std::pair<int, int> nt{plan->preds[pidx].p.op == GPUQ_IS_NULL
                                     ? TK_IS_NULL : TK_IS_NOT_NULL,
                                 plan->ctx_of(pidx)};
          if (std::find(null_tasks.begin(), null_tasks.end(), nt) ==
              null_tasks.end())
            null_tasks.push_back(nt);
        }
        std::sort(null_tasks.begin(), null_tasks.end());
        stubs.push_back({r.file_idx, r.rg_idx, (int)ci, &cm, part.raw_bytes,
                         r.row_start, needs_val, std::move(null_tasks)});
        part.raw_bytes += cm.total_compressed_size;
        part.bytes_scanned += cm.total_compressed_size;
      }
    }

    // phase 1 (parallel): page walks + dict-page decompress/processing —
    // everything except global-dictionary id assignment (shared state)
    part.chunks.resize(stubs.size());
    std::vector<std::vector<std::string>> dict_strs(stubs.size());
    parallel_for(stubs.size(), [&](size_t i) {
      const Stub& s = stubs[i];
      const auto& mf = *plan->files[s.file_idx];
      const auto& cm = *s.cm;
      auto& c = plan->cols[s.col_idx];
      ChunkTask t;
      t.file_idx = s.file_idx; t.rg_idx = s.rg_idx; t.col_idx = s.col_idx;
      t.cm = s.cm;
      t.raw_off = s.raw_off;
      t.pages = walk_pages(mf.data, cm, mf.meta.row_groups[s.rg_idx].num_rows);

      // host-side dictionary processing
      for (auto& pi : t.pages) {
        if (pi.type != PAGE_DICT) continue;
        std::vector<uint8_t> dbuf;
        const uint8_t* d = host_page_payload(cm.codec, mf.data + pi.payload_off,
                                             pi.comp_size, pi.uncomp_size, dbuf);
        if (c.phys == PT_BYTE_ARRAY) {
          const uint8_t* q = d;
          if (!c.hash_mode && (c.need_gid || c.need_rank))
            dict_strs[i].reserve(pi.num_values);
          for (int32_t k = 0; k < pi.num_values; k++) {
            uint32_t l; memcpy(&l, q, 4); q += 4;
            if (c.hash_mode)
              t.strof.push_back((int64_t)(q - d) - 4);  // page-relative [len]
            else if (c.need_gid || c.need_rank)
              dict_strs[i].emplace_back((const char*)q, l);
            if (!c.hash_mode && !c.lut_preds.empty()) {
              t.lut_x.resize(c.lut_ctxs.size() - 1);
              for (size_t j = 0; j < c.lut_ctxs.size(); j++)
                (j ? t.lut_x[j - 1] : t.lut)
                    .push_back(lut_entry(s.col_idx, c.lut_ctxs[j], q, l));
            }
            q += l;
          }
        } else if (c.phys == PT_INT64) {
          t.dictv.resize(pi.num_values);
          memcpy(t.dictv.data(), d, 8 * (size_t)pi.num_values);
        } else if (c.phys == PT_INT32) {
          t.dictv.resize(pi.num_values);
          for (int32_t k = 0; k < pi.num_values; k++) {
            int32_t v; memcpy(&v, d + 4 * (size_t)k, 4); t.dictv[k] = v;
          }
        } else if (c.phys == PT_DOUBLE) {
          t.dictv.resize(pi.num_values);
          memcpy(t.dictv.data(), d, 8 * (size_t)pi.num_values);
        }
      }
      for (auto& pi : t.pages)
        if (pi.type == PAGE_DATA && pi.encoding == ENC_PLAIN)
          t.has_plain_data_pages = true;
      if (c.hash_mode) {
        // PLAIN pages: walk the [u32 len][bytes] chain once (def-level
        // aware) and record each non-null value's page-relative offset —
        // made absolute in phase 3 once page dst slots are known
        std::vector<uint8_t> img;
        bool optional = false;
        {
          int si2 = mf.meta.col_index(c.name);
          if (si2 >= 0) optional = mf.meta.columns[si2].optional;
        }
        for (auto& pi : t.pages) {
          if (pi.type != PAGE_DATA || pi.encoding != ENC_PLAIN) continue;
          const uint8_t* data = host_page_payload(
              cm.codec, mf.data + pi.payload_off, pi.comp_size,
              pi.uncomp_size, img);
          uint32_t cnt0 = (uint32_t)t.pvals.size();
          if (!walk_plain_bytes(data, (uint32_t)pi.uncomp_size,
                                (uint32_t)pi.num_values, optional,
                                [&](uint32_t pos, uint32_t) {
                                  t.pvals.push_back((int64_t)pos);
                                }))
            throw std::runtime_error("plain page overrun (hash col)");
          t.pval_page_n.push_back((uint32_t)t.pvals.size() - cnt0);
        }
      }
      if (t.has_plain_data_pages && !c.hash_mode &&
          (c.need_gid || c.need_rank))
        throw std::runtime_error("dict-only utf8 operation with PLAIN fallback pages "
                                 "outside hash mode — " + c.name);
      part.chunks[i] = std::move(t);
    });
    phase_mark("phase1 walk+dicts");

    // phase 2 (serial): global-dictionary gid assignment per chunk, in order
    for (size_t i = 0; i < part.chunks.size(); i++) {
      auto& t = part.chunks[i];
      auto& c = plan->cols[t.col_idx];
      if (c.phys != PT_BYTE_ARRAY || dict_strs[i].empty()) continue;
      if (c.need_gid) t.remap.reserve(dict_strs[i].size());
      if (c.need_rank) t.dictv.reserve(dict_strs[i].size());
      for (auto& sv : dict_strs[i]) {
        int32_t g = c.gid_of(sv);
        if (c.need_gid) t.remap.push_back(g);
        if (c.need_rank) t.dictv.push_back(g);  // post-pass rewrites gid->rank
      }
      dict_strs[i].clear();
      dict_strs[i].shrink_to_fit();
    }
    phase_mark("phase2 gids");

    // phase 3 (serial): pool / page-id / dec-arena bases per chunk
    struct Bases {
      uint32_t remap, dictv, lut;
      uint64_t dec;
      int32_t pid;
    };
    std::vector<Bases> bases(part.chunks.size());
    int32_t pid_cursor = 0;
    for (size_t i = 0; i < part.chunks.size(); i++) {
      auto& t = part.chunks[i];
      auto& c = plan->cols[t.col_idx];
      bases[i] = {(uint32_t)part.remap_pool.size(),
                  (uint32_t)part.dictv_pool.size(),
                  (uint32_t)part.lut_pool.size(), part.dec_bytes, pid_cursor};
      t.dictv_pool_base = bases[i].dictv;
      part.remap_pool.insert(part.remap_pool.end(), t.remap.begin(), t.remap.end());
      if (!c.hash_mode)
        part.dictv_pool.insert(part.dictv_pool.end(), t.dictv.begin(), t.dictv.end());
      part.lut_pool.insert(part.lut_pool.end(), t.lut.begin(), t.lut.end());
      if (part.lut_pool_x.size() < t.lut_x.size())
        part.lut_pool_x.resize(t.lut_x.size());
      for (size_t j = 0; j < part.lut_pool_x.size(); j++) {
        auto& px = part.lut_pool_x[j];
        px.resize(bases[i].lut, 0);  // zero where earlier chunks had no slot
        if (j < t.lut_x.size())
          px.insert(px.end(), t.lut_x[j].begin(), t.lut_x[j].end());
      }
      t.dec_base = part.dec_bytes;
      if (c.hash_mode) {
        // the dict page image joins the dec arena (device-side strings);
        // its entry offsets become absolute strrefs in the dictv pool
        for (auto& pi : t.pages)
          if (pi.type == PAGE_DICT) {
            t.dict_dst = part.dec_bytes;
            part.dec_bytes += ((uint64_t)pi.uncomp_size + 15) & ~15ull;
          }
        for (int64_t rel : t.strof)
          part.dictv_pool.push_back((int64_t)(t.dict_dst + (uint64_t)rel));
      }
      size_t plain_i = 0, pv_off = 0;
      for (auto& pi : t.pages) {
        if (pi.type != PAGE_DATA) continue;
        uint64_t pg_dst = part.dec_bytes;
        pid_cursor++;
        // 16-align page images so dst and LDS-ring offsets share alignment
        part.dec_bytes += ((uint64_t)pi.uncomp_size + 15) & ~15ull;
        if (c.hash_mode && pi.encoding == ENC_PLAIN) {
          t.pval_base.push_back((uint32_t)part.dictv_pool.size());
          uint32_t nvp = t.pval_page_n[plain_i++];
          for (uint32_t k = 0; k < nvp; k++)
            part.dictv_pool.push_back((int64_t)(pg_dst + (uint64_t)t.pvals[pv_off + k]));
          pv_off += nvp;
        }
      }
      t.dec_len = part.dec_bytes - t.dec_base;
      // hot tier: the decompressed chunk image may already be resident
      {
        const auto& mf2 = *plan->files[t.file_idx];
        // layout-qualified key: a hash-mode chunk's image includes the
        // decompressed dict page, a dict/LUT-mode chunk's does not — the
        // same (file, rg, col) caches separately per layout
        t.cache_key = mf2.path + "\x01" + std::to_string(mf2.size) + ":" +
                      std::to_string(mf2.mtime_ns) + ":" +
                      std::to_string(t.rg_idx) + ":" + c.name +
                      (c.hash_mode ? ":h" : "");
        if (ctx->cache_pin(t.cache_key, (size_t)t.dec_len)) {
          t.cached = true;
          plan->pinned_keys.push_back(t.cache_key);
          part.bytes_cache_hit += (int64_t)t.cm->total_compressed_size;
        }
      }
    }

    for (auto& px : part.lut_pool_x) px.resize(part.lut_pool.size(), 0);
    phase_mark("phase3 pools+cache");

    // phase 4 (parallel): per-chunk device images — DevPage descriptors,
    // LZ4 structure walks, seg/lit/backref records, task-list routing
    struct CItem {
      const uint8_t* praw;
      int32_t comp, uncomp, page_id;
      uint64_t dst_off;
      uint32_t num_values;
      bool optional;
      int codec;
      int col;
    };
    std::vector<CItem> citems;
    struct CB : DecompRecs {
      std::vector<DevPage> pages;
      std::map<std::pair<int,int>, std::vector<int32_t>> tasks;
      std::vector<CItem> citems;
    };
    std::vector<CB> cbs(part.chunks.size());
    parallel_for(part.chunks.size(), [&](size_t ti) {
      auto& t = part.chunks[ti];
      auto& c = plan->cols[t.col_idx];
      auto& cb = cbs[ti];
      const auto& mf = *plan->files[t.file_idx];
      const uint32_t remap_base = bases[ti].remap;
      const uint32_t dictv_base = bases[ti].dictv;
      const uint32_t lut_base = bases[ti].lut;
      uint64_t dec_off = bases[ti].dec;
      int32_t page_id = bases[ti].pid;
      const uint32_t rstart = stubs[ti].rstart;

      // decompress planning for one page image (data or hash-col dict)
      const int chunk_codec = t.cm->codec;
      auto plan_decomp = [&](const uint8_t* praw, uint64_t src_abs,
                             uint64_t dst_abs, uint32_t comp, uint32_t uncomp,
                             bool raw_page) {
        plan_decomp_page(cb, chunk_codec, praw, src_abs, dst_abs, comp, uncomp,
                         raw_page);
      };

      // hash-mode dict page: decompress its image into the reserved slot
      if (c.hash_mode) {
        for (auto& pi : t.pages) {
          if (pi.type != PAGE_DICT) continue;
          if (!t.cached)
            plan_decomp(mf.data + pi.payload_off,
                        t.raw_off + (uint64_t)(pi.payload_off - t.cm->start_offset()),
                        t.dict_dst, pi.comp_size, pi.uncomp_size,
                        t.cm->codec == CODEC_UNCOMPRESSED);
          dec_off += ((uint64_t)pi.uncomp_size + 15) & ~15ull;
        }
      }

      uint32_t row_in_rg = 0;
      size_t plain_i4 = 0;
      for (auto& pi : t.pages) {
        if (pi.type != PAGE_DATA) continue;
        DevPage dp{};
        dp.src_off = t.raw_off + (uint64_t)(pi.payload_off - t.cm->start_offset());
        dp.dst_off = dec_off;
        dec_off += ((uint64_t)pi.uncomp_size + 15) & ~15ull;
        dp.comp_size = pi.comp_size;
        dp.uncomp_size = pi.uncomp_size;
        dp.num_values = pi.num_values;
        dp.row_start = rstart + row_in_rg;
        row_in_rg += pi.num_values;
        dp.optional = mf.meta.columns[mf.meta.col_index(c.name)].optional;
        dp.raw_copy = (t.cm->codec == CODEC_UNCOMPRESSED);
        dp.dict_n = (uint32_t)std::max(
            {t.remap.size(), t.dictv.size(), t.lut.size(), t.strof.size()});
        dp.encoding = (uint8_t)pi.encoding;
        dp.phys = (uint8_t)c.phys;
        const int32_t this_pid = page_id++;
        // host LZ4 structure walk -> parallel segments + backref records
        // (cached chunks arrive decompressed from the hot tier instead)
        if (!t.cached)
          plan_decomp(mf.data + pi.payload_off, dp.src_off, dp.dst_off,
                      pi.comp_size, pi.uncomp_size, dp.raw_copy != 0);
        bool dict_enc = (pi.encoding == ENC_RLE_DICT || pi.encoding == ENC_PLAIN_DICT);
        // aux (remap / gid), aux_val (dict values or utf8 sort-ranks) and
        // aux_lut (predicate LUT) are independent slots: one utf8 column
        // can be group key + min/max agg + predicate at once (found by the
        // query fuzzer — aliasing aux produced garbage gids and OOB table
        // writes).
        if (c.need_gid && dict_enc && !c.hash_mode) {
          dp.aux = remap_base;
          cb.tasks[{TK_DICT_GID, t.col_idx}].push_back(this_pid);
        }
        if (c.need_val && stubs[ti].need_val_decode) {
          if (c.hash_mode) {
            // d_val carries strrefs: dict pages gather the chunk's absolute
            // entry offsets; PLAIN pages copy the host-walked value offsets
            if (dict_enc) {
              dp.aux_val = dictv_base;
              cb.tasks[{TK_DICT_VAL, t.col_idx}].push_back(this_pid);
            } else if (pi.encoding == ENC_PLAIN) {
              dp.aux_val = t.pval_base[plain_i4++];
              cb.tasks[{TK_POOL_VAL, t.col_idx}].push_back(this_pid);
            } else throw std::runtime_error("unsupported encoding for hash col");
          } else if (dict_enc) {
            dp.aux_val = dictv_base;
            cb.tasks[{TK_DICT_VAL, t.col_idx}].push_back(this_pid);
          } else if (pi.encoding == ENC_PLAIN) {
            cb.tasks[{TK_PLAIN_VAL, t.col_idx}].push_back(this_pid);
          } else if (pi.encoding == ENC_DELTA_BP) {
            cb.tasks[{TK_DELTA_VAL, t.col_idx}].push_back(this_pid);
          } else throw std::runtime_error("unsupported encoding for values");
        }
        if (!c.lut_preds.empty() && !c.hash_mode) {
          // (hash-mode columns evaluate every predicate over row strrefs
          // with k_cmp_str at execute — no LUT/window tasks)
          // one task per mask context with a LUT of this column (flat
          // conjunction: context 0 alone)
          if (dict_enc) {
            dp.aux_lut = lut_base;
            for (int k : c.lut_ctxs)
              cb.tasks[{tk_ctx(TK_DICT_MASK, k), t.col_idx}].push_back(this_pid);
          } else if (pi.encoding == ENC_PLAIN) {
            // PLAIN fallback page of a string column: the LIKE family only
            // (an EQ..GE predicate would have put the column in hash mode,
            // and an OR group folds only on a column without PLAIN pages)
            if ((int)c.contains_preds.size() != (int)c.lut_preds.size())
              throw std::runtime_error("non-LIKE predicate on PLAIN utf8 pages: next row");
            for (auto& f : plan->wfolds)
              if (f.col == t.col_idx)
                throw std::runtime_error("folded OR group on PLAIN utf8 pages");
            for (int k : c.lut_ctxs)
              cb.tasks[{tk_ctx(TK_BYTES_CONTAINS, k), t.col_idx}].push_back(this_pid);
            cb.citems.push_back({mf.data + pi.payload_off, pi.comp_size,
                                 pi.uncomp_size, this_pid, dp.dst_off,
                                 (uint32_t)pi.num_values, dp.optional != 0,
                                 t.cm->codec, t.col_idx});
          } else throw std::runtime_error("unsupported encoding for string predicate");
        }
        // IS [NOT] NULL reads the def levels alone: every data page of the
        // chunk, whatever its value encoding
        for (auto& nt : stubs[ti].null_tasks)
          cb.tasks[{tk_ctx(nt.first, nt.second), t.col_idx}].push_back(this_pid);
        cb.pages.push_back(dp);
      }
      if (row_in_rg != (uint32_t)mf.meta.row_groups[t.rg_idx].num_rows)
        throw std::runtime_error("page rows mismatch");
    });

    phase_mark("phase4 lz4 walks");

    // phase 5: order-preserving merge of the per-chunk images, PARALLEL —
    // the record streams total ~8 GB at 1 B rows and serial vector inserts
    // took ~3 s of the plan build. Offsets by prefix sum, then every chunk
    // copies (with its piece/backref index bases applied) into its slice.
    {
      const size_t nc = cbs.size();
      merge_stream(cbs, &CB::pages, part.pages);
      // Delta fork: a column forks when the plan allows it (fork_col) and
      // every chunk of it that is decoded here is DELTA_BINARY_PACKED
      // throughout, so its only value task is TK_DELTA_VAL, which touches
      // none of decode_values' shared scratch. The decompress records of
      // those chunks move to the early set; host-staged images stay with
      // the main set (they are uploaded at load, not launched).
      std::vector<DecompRecs> ecbs(nc);
      if (!plan->no_delta_fork) {
        std::vector<char> forks(plan->cols.size(), 0), seen = forks;
        for (size_t ci = 0; ci < plan->cols.size(); ci++)
          forks[ci] = fork_col(*plan, (int)ci);
        for (size_t i = 0; i < nc; i++) {
          const auto& t = part.chunks[i];
          if (!forks[t.col_idx] || !stubs[i].need_val_decode) continue;
          seen[t.col_idx] = 1;
          for (const auto& pi : t.pages)
            if (pi.type == PAGE_DATA && pi.encoding != ENC_DELTA_BP)
              forks[t.col_idx] = 0;
        }
        for (size_t ci = 0; ci < plan->cols.size(); ci++)
          if (forks[ci] && seen[ci]) part.fork_cols.push_back((int)ci);
        for (size_t i = 0; i < nc; i++) {
          const int ci = part.chunks[i].col_idx;
          if (!forks[ci] || !seen[ci] || !stubs[i].need_val_decode) continue;
          DecompRecs& all = cbs[i];
          auto himgs = std::move(all.himgs);
          ecbs[i] = std::move(all);
          all = DecompRecs{};
          all.himgs = std::move(himgs);
        }
      }
      merge_decomp_recs(cbs, part);
      merge_decomp_recs(ecbs, part.early);
      // small, order-sensitive leftovers stay serial
      for (size_t i = 0; i < nc; i++) {
        auto& cb = cbs[i];
        for (auto& [key, ids] : cb.tasks) {
          auto& dstv = part.tasks[key];
          dstv.insert(dstv.end(), ids.begin(), ids.end());
        }
        citems.insert(citems.end(), cb.citems.begin(), cb.citems.end());
        for (auto& h : cb.himgs)
          part.himgs.emplace_back(h.first, std::move(h.second));
      }
    }
    phase_mark("phase5 merge");
    part.dec_bytes += 16384 + 64;  // over-read pad: contains window + unpackers

    // CONTAINS window build: decompress each PLAIN byte-array page once on
    // the host (load-time, parallel over pages), walk the [u32 len][bytes]
    // chain, and emit value-aligned <=16KB windows + a u16 start offset per
    // value — the kernel-side serial length walk disappears entirely.
    if (!citems.empty()) {
      struct CLocal {
        std::vector<DevCWin> wins;
        std::vector<uint16_t> starts;
      };
      std::vector<CLocal> locals(citems.size());
      const char* const corrupt = "contains window walk failed (corrupt page)";
      parallel_for(citems.size(), [&](size_t i) {
        const auto& it = citems[i];
        auto& L = locals[i];
        std::vector<uint8_t> img;
        const uint8_t* data;
        try {
          data = host_page_payload(it.codec, it.praw, it.comp, it.uncomp, img);
        } catch (const std::exception&) {
          throw std::runtime_error(corrupt);
        }
        uint32_t dense = 0;
        int64_t wfirst = -1;
        uint32_t wbytes = 0, wvals = 0, wdense0 = 0;
        auto flush = [&]() {
          if (wfirst < 0) return;
          L.wins.push_back({it.dst_off + (uint64_t)wfirst,
                            (uint64_t)(L.starts.size() - wvals), wbytes,
                            wvals, wdense0, it.page_id});
          wfirst = -1;
          wbytes = wvals = 0;
        };
        if (!walk_plain_bytes(
                data, (uint32_t)it.uncomp, it.num_values, it.optional,
                [&](uint32_t pos, uint32_t len) {
                  const uint64_t rec = 4ull + len;
                  if (rec > 16384) {  // oversized value: its own window
                    flush();
                    L.starts.push_back(0);
                    L.wins.push_back({it.dst_off + pos, L.starts.size() - 1,
                                      (uint32_t)rec, 1, dense, it.page_id});
                  } else {
                    if (wfirst >= 0 && wbytes + rec > 16384) flush();
                    if (wfirst < 0) { wfirst = pos; wdense0 = dense; }
                    L.starts.push_back((uint16_t)(pos - wfirst));
                    wbytes += (uint32_t)rec;
                    wvals++;
                  }
                  dense++;
                }))
          throw std::runtime_error(corrupt);
        flush();
      });
      // append in task order, per column
      std::map<int32_t, size_t> by_page;
      for (size_t i = 0; i < citems.size(); i++) by_page[citems[i].page_id] = i;
      for (auto& [key, ids] : part.tasks) {
        // the windows belong to the column: every context's task lists the
        // same pages, the first one builds them
        if (tk_kind(key.first) != TK_BYTES_CONTAINS ||
            part.cwin_ranges.count(key.second))
          continue;
        uint32_t off = (uint32_t)part.cwins.size();
        for (int32_t pid : ids) {
          const auto& L = locals[by_page.at(pid)];
          uint64_t sbase = part.cstarts.size();
          part.cstarts.insert(part.cstarts.end(), L.starts.begin(),
                              L.starts.end());
          for (DevCWin w : L.wins) {
            w.starts += sbase;
            part.cwins.push_back(w);
          }
        }
        part.cwin_ranges[key.second] = {off, (uint32_t)part.cwins.size() - off};
      }
    }
  }

  // bin bounds from row-group footer stats of the source column
  for (auto& c : plan->cols) {
    if (!c.is_bin) continue;
    const auto& src = plan->cols[c.bin_src];
    bool any = false;
    int64_t mn = 0, mx = 0;
    for (auto& part : plan->parts)
      for (auto& r : part.rgs) {
        const auto& mf = *plan->files[r.file_idx];
        int si = mf.meta.col_index(src.name);
        const auto& cm = mf.meta.row_groups[r.rg_idx].chunks[si];
        if (!cm.has_i64_stats)
          throw std::runtime_error("DATE_BIN needs footer i64 stats on " + src.name);
        if (!any) { mn = cm.stat_min; mx = cm.stat_max; any = true; }
        else { mn = std::min(mn, cm.stat_min); mx = std::max(mx, cm.stat_max); }
      }
    auto fdiv = [](int64_t v, int64_t s) {
      return v >= 0 ? v / s : -((-v + s - 1) / s);
    };
    c.bin_min_idx = any ? fdiv(mn - c.bin_origin, c.bin_stride) : 0;
    int64_t max_idx = any ? fdiv(mx - c.bin_origin, c.bin_stride) : 0;
    int64_t nb = max_idx - c.bin_min_idx + 1;
    if (nb > (1 << 21)) throw std::runtime_error("too many DATE_BIN bins");
    c.nbins = (int32_t)std::max<int64_t>(nb, 1);
  }

  // group table size (saturating product; a product beyond GID_CAP takes
  // the exact pair-cascade path at execute, like very-high-cardinality
  // hash keys)
  int64_t g = 1;
  for (int ci : plan->group_cols) {
    const auto& c = plan->cols[ci];
    int64_t sz = c.is_bin ? (int64_t)c.nbins + 1 : (int64_t)c.gdict.size() + 1;
    g = (g > (int64_t)GID_CAP) ? g : g * sz;
  }
  if (g > (int64_t)GID_CAP) {
    plan->needs_cascade = true;
    g = GID_CAP;
  }
  plan->n_groups = (int32_t)g;

  for (auto& part : plan->parts)
    plan->m_rows_scanned += part.n_rows;

  // count-slot elision (footer stats): when every chunk of an aggregate's
  // column has null_count == 0, its non-null count equals the presence
  // count — k_agg skips the per-row count atomics and the validity read,
  // and the export reads slot 0 instead (the same trick the reference's
  // engine gets from its statistics-based null handling).
  for (auto& ap : plan->aggs) {
    if (ap.op == GPUQ_AGG_COUNT_STAR || ap.col_idx < 0) continue;
    // a filtered aggregate's count is not the presence count
    if (ap.filter >= 0) continue;
    bool all0 = true;
    for (auto& part : plan->parts)
      for (auto& t : part.chunks)
        if (t.col_idx == ap.col_idx && t.cm->null_count != 0) all0 = false;
    ap.cnt_is_presence = all0;
  }

  // utf8 min/max post-pass: with every chunk registered, the global dict is
  // final — compute each rank column's lexicographic sort ranks and rewrite
  // its per-chunk dictionary-value pools from gid to rank.
  for (size_t ci = 0; ci < plan->cols.size(); ci++) {
    auto& c = plan->cols[ci];
    if (!c.need_rank) continue;
    std::vector<int32_t> order((size_t)c.gdict.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = (int32_t)i;
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
      return c.gdict[a] < c.gdict[b];
    });
    std::vector<int64_t> rank_of_gid(c.gdict.size() + 1, 0);
    c.rank_to_gid.assign(c.gdict.size(), 0);
    for (size_t r = 0; r < order.size(); r++) {
      rank_of_gid[(size_t)order[r] + 1] = (int64_t)r;
      c.rank_to_gid[r] = order[r] + 1;
    }
    for (auto& part : plan->parts)
      for (auto& t : part.chunks)
        if (t.col_idx == (int)ci && t.dictv_pool_base != (size_t)-1)
          for (size_t k = 0; k < t.dictv.size(); k++)
            part.dictv_pool[t.dictv_pool_base + k] =
                rank_of_gid[(size_t)part.dictv_pool[t.dictv_pool_base + k]];
  }

  // fused count path: GROUP BY <one dict col>, count(*)-only, no predicates
  {
    bool aggs_ok = true;
    for (auto& ap : plan->aggs) aggs_ok &= (ap.kind == AGGK_COUNT_STAR);
    plan->fused_count = plan->group_cols.size() == 1 && aggs_ok &&
                        plan->preds.empty() && plan->filters.empty() && plan->n_groups <= 8192 &&
                        !plan->cols[plan->group_cols[0]].is_bin &&
                        !plan->cols[plan->group_cols[0]].hash_mode &&
                        !plan->cols[plan->group_cols[0]].numeric_key;
  }

  // footer-proven null-free columns, per partition
  for (auto& part : plan->parts) {
    part.col_null_free.assign(plan->cols.size(), 1);
    for (auto& t : part.chunks)
      if (t.cm->null_count != 0) part.col_null_free[t.col_idx] = 0;
  }

  // a distinct agg keeps the plan off both fused paths (their shapes admit
  // no third kind of aggregate; stated here so a later shape cannot let one in)
  if (!plan->distinct_aggs.empty()) plan->fused_count = false;
  // fused value-decode + aggregate: exactly the shape launch_agg's fast path
  // takes with two aggregates, over a column that only the aggregate reads
  // and whose pages are all dict-encoded or PLAIN 8-byte
  if (!plan->is_projection && !plan->no_fused_valagg &&
      plan->distinct_aggs.empty() && plan->filters.empty() &&
      plan->group_cols.size() == 1 && plan->aggs.size() == 2 &&
      plan->aggs[0].kind == AGGK_COUNT_STAR && plan->n_fsum == 0 &&
      (plan->aggs[1].kind == AGGK_SUM_I64 || plan->aggs[1].kind == AGGK_MIN_I64 ||
       plan->aggs[1].kind == AGGK_MAX_I64) &&
      plan->aggs[1].cnt_is_presence && !plan->needs_cascade) {
    const int vc = plan->aggs[1].col_idx;
    const auto& c = plan->cols[vc];
    const auto& kc = plan->cols[plan->group_cols[0]];
    bool ok = c.phys == PT_INT64 && !c.is_bin && !c.hash_mode &&
              !c.numeric_key && !c.need_gid && !c.need_rank &&
              c.cmp_preds.empty() && c.lut_preds.empty() &&
              c.null_preds.empty() &&
              plan->group_cols[0] != vc;
    for (auto& o : plan->cols) ok &= !(o.is_bin && o.bin_src == vc);
    const bool late = kc.hash_mode || kc.numeric_key;
    if (!late) ok &= (int64_t)plan->n_groups * 16 <= 64 * 1024;
    for (auto& part : plan->parts) {
      if (!ok) break;
      for (auto& kv : part.tasks) {
        if (kv.first.second != vc) continue;
        if (kv.first.first != TK_DICT_VAL && kv.first.first != TK_PLAIN_VAL)
          ok = false;  // delta-encoded (or any other) pages: old path
      }
    }
    if (ok) {
      plan->fused_valagg = true;
      plan->valagg_col = vc;
      plan->valagg_late = late;
      for (auto& part : plan->parts) {
        for (int k : {TK_DICT_VAL, TK_PLAIN_VAL}) {
          auto it = part.tasks.find({k, vc});
          if (it != part.tasks.end())
            part.valagg_ids.insert(part.valagg_ids.end(), it->second.begin(),
                                   it->second.end());
        }
        std::sort(part.valagg_ids.begin(), part.valagg_ids.end());
      }
    }
  }

  if (plan->exec_dbg)
    plan_debug_report(plan.get(), null_dbg, leaf_dbg, or_path);
  return plan.release();
} catch (const std::exception& e) {
  if (ctx) ctx->set_error(e.what());
  return nullptr;
}

// §8f row 1: native catalog planner — plan straight from Parseable's
// stream.json/manifest.json (catalog.cpp). fast_count out-param:
//   >= 0  answered from manifest num_rows sums (no plan returned)
//   -1    a scan plan was built (or an error occurred: check return)
//   -2    every file pruned: empty relation, no plan
extern "C" gpuq_plan* gpuq_plan_build_from_stream(
    gpuq_ctx* ctx, const char* stream_dir,
    const char* const* projection, int32_t n_projection,
    const gpuq_pred* preds, int32_t n_preds,
    const char* const* group_by, int32_t n_group_by,
    const gpuq_agg* aggs, int32_t n_aggs, int64_t limit,
    int64_t* fast_count) {
  return gpuq_plan_build_from_stream_where(
      ctx, stream_dir, projection, n_projection, preds, n_preds, group_by,
      n_group_by, aggs, n_aggs, limit, fast_count, nullptr, 0);
}

extern "C" gpuq_plan* gpuq_plan_build_from_stream_where(
    gpuq_ctx* ctx, const char* stream_dir,
    const char* const* projection, int32_t n_projection,
    const gpuq_pred* preds, int32_t n_preds,
    const char* const* group_by, int32_t n_group_by,
    const gpuq_agg* aggs, int32_t n_aggs, int64_t limit,
    int64_t* fast_count,
    const gpuq_where_node* nodes, int32_t n_nodes) {
  return gpuq_plan_build_from_stream_filtered(
      ctx, stream_dir, projection, n_projection, preds, n_preds, group_by,
      n_group_by, aggs, n_aggs, limit, fast_count, nodes, n_nodes, nullptr, 0);
}

extern "C" gpuq_plan* gpuq_plan_build_from_stream_filtered(
    gpuq_ctx* ctx, const char* stream_dir,
    const char* const* projection, int32_t n_projection,
    const gpuq_pred* preds, int32_t n_preds,
    const char* const* group_by, int32_t n_group_by,
    const gpuq_agg* aggs, int32_t n_aggs, int64_t limit,
    int64_t* fast_count,
    const gpuq_where_node* nodes, int32_t n_nodes,
    const gpuq_agg_filter* filters, int32_t n_filters) try {
  if (fast_count) *fast_count = -1;
  // a filtered count(*) cannot be answered from num_rows
  bool bare = (n_aggs == 1 && aggs && aggs[0].op == GPUQ_AGG_COUNT_STAR &&
               n_group_by == 0 && n_filters == 0);
  CatalogPlanInput in = catalog_plan(stream_dir, preds, n_preds, bare, nodes,
                                     n_nodes, filters, n_filters, n_aggs,
                                     n_projection > 0);
  if (in.fast_count >= 0) {
    if (fast_count) *fast_count = in.fast_count;
    return nullptr;
  }
  if (in.files.empty()) {
    if (fast_count) *fast_count = -2;
    return nullptr;
  }
  std::vector<gpuq_file> files(in.files.size());
  for (size_t i = 0; i < in.files.size(); i++) {
    files[i].path = in.files[i].c_str();
    files[i].row_groups = nullptr;
    files[i].n_row_groups = -1;
  }
  gpuq_plan* plan = gpuq_plan_build_filtered(
      ctx, files.data(), (int32_t)files.size(), projection, n_projection,
      preds, n_preds, group_by, n_group_by, aggs, n_aggs, limit, nodes,
      n_nodes, filters, n_filters);
  // footer null counts can drop every row group of every kept file (IS NULL
  // on a required column): the empty relation, like an all-pruned file list
  bool null_pred = false;
  for (int32_t i = 0; i < n_preds; i++) null_pred |= op_is_null(preds[i].op);
  if (plan && null_pred && plan->m_rows_scanned == 0) {
    gpuq_plan_destroy(plan);
    if (fast_count) *fast_count = -2;
    return nullptr;
  }
  return plan;
} catch (const std::exception& e) {
  if (ctx) ctx->set_error(e.what());
  return nullptr;
}

extern "C" int32_t gpuq_plan_partition_count(gpuq_plan* p) {
  return p ? (int32_t)p->parts.size() : 0;
}

// ------------------------------------------------------------------
// load: stage raw chunks + aux pools into HBM
// ------------------------------------------------------------------
extern "C" int32_t gpuq_plan_load(gpuq_plan* plan, int32_t pi) try {
  if (!plan || pi < 0 || pi >= (int32_t)plan->parts.size()) return -1;
  Partition& part = plan->parts[pi];
  if (part.loaded) return 0;
  int64_t t0 = now_ns();
  HIP_TRY(hipSetDevice(part.device));
  HIP_TRY(hipStreamCreateWithFlags(&part.stream, hipStreamNonBlocking));
  // the side stream of the delta fork, for partitions that have one: an
  // idle second stream is not free (§7: +0.2 ms of host time per step)
  if (!part.fork_cols.empty())
    HIP_TRY(hipStreamCreateWithFlags(&part.side, hipStreamNonBlocking));

  // slack: the LZ4 input-window refill may read up to LZ4_IN+256 past the
  // last chunk's end (see kernels.hip refill note)
  HIP_TRY(hipMalloc(&part.d_raw, std::max<uint64_t>(part.raw_bytes + 8192, 16)));
  HIP_TRY(hipMalloc(&part.d_dec, std::max<uint64_t>(part.dec_bytes, 16)));
  // H2D staging through a ring of pinned buffers (Ring, above): raw chunks
  // are packed contiguously into d_raw (raw_off cumulative), and every
  // multi-GB aux pool below rides the same ring.
  Ring ring(part.stream);
  {
    // stage raw bytes only for chunks NOT served by the hot tier (cached
    // chunks' raw regions are never read — their dec images arrive below)
    std::vector<Ring::Span> run;
    uint64_t run_dst = 0, cursor = 0;
    auto flush = [&]() {
      if (!run.empty()) {
        ring.copy_spans(part.d_raw + run_dst, run);
        run.clear();
      }
    };
    for (auto& t : part.chunks) {
      const auto& mf = *plan->files[t.file_idx];
      uint64_t len = (uint64_t)t.cm->total_compressed_size;
      if (t.cached) {
        flush();
      } else {
        if (run.empty()) run_dst = cursor;
        run.push_back({mf.data + t.cm->start_offset(), len});
      }
      cursor += len;
    }
    flush();
    for (auto& t : part.chunks) {
      if (!t.cached || !t.dec_len) continue;
      void* src = plan->ctx->cache_get(t.cache_key);
      if (!src) throw std::runtime_error("hot-tier entry vanished while pinned");
      HIP_TRY(hipMemcpyAsync(part.d_dec + t.dec_base, src, t.dec_len,
                             hipMemcpyDeviceToDevice, part.stream));
    }
    // host-decompressed page images (snappy fallback pages)
    for (auto& h : part.himgs)
      ring.copy(part.d_dec + h.first, h.second.data(), h.second.size());
  }
  HIP_TRY(hipMalloc(&part.d_pages, std::max<size_t>(part.pages.size() * sizeof(DevPage), 16)));
  HIP_TRY(hipMemcpyAsync(part.d_pages, part.pages.data(),
                         part.pages.size() * sizeof(DevPage), hipMemcpyHostToDevice,
                         part.stream));
  auto upload_pool = [&](const void* src, size_t bytes, void** dst) {
    HIP_TRY(hipMalloc(dst, std::max<size_t>(bytes, 16)));
    if (bytes) ring.copy(*dst, src, bytes);
  };
  upload_pool(part.remap_pool.data(), part.remap_pool.size() * 4, (void**)&part.d_remap);
  upload_pool(part.dictv_pool.data(), part.dictv_pool.size() * 8, (void**)&part.d_dictv);
  if (part.lut_pool_x.empty()) {
    upload_pool(part.lut_pool.data(), part.lut_pool.size(), (void**)&part.d_lut);
  } else {
    // WHERE-tree LUT slots: slot j at d_lut + j * lut_pool.size()
    std::vector<uint8_t> all(part.lut_pool);
    for (auto& px : part.lut_pool_x) all.insert(all.end(), px.begin(), px.end());
    upload_pool(all.data(), all.size(), (void**)&part.d_lut);
    HIP_TRY(hipStreamSynchronize(part.stream));  // `all` dies with this scope
  }
  for (auto& kv : part.tasks) {
    int32_t* d = nullptr;
    upload_pool(kv.second.data(), kv.second.size() * 4, (void**)&d);
    part.d_ids[kv.first] = d;
  }
  if (plan->fused_valagg)
    upload_pool(part.valagg_ids.data(), part.valagg_ids.size() * 4,
                (void**)&part.d_valagg_ids);
  // column outputs
  for (size_t ci = 0; ci < plan->cols.size(); ci++) {
    auto& c = plan->cols[ci];
    if (c.is_bin || c.numeric_key) {
      int32_t* d; HIP_TRY(hipMalloc(&d, std::max<int64_t>(part.n_rows * 4, 16)));
      part.d_gid[(int)ci] = d;
      if (c.is_bin) continue;
    }
    if (c.need_gid) {
      int32_t* d; HIP_TRY(hipMalloc(&d, std::max<int64_t>(part.n_rows * 4, 16)));
      part.d_gid[(int)ci] = d;
      if (c.need_gid_valid) {
        uint8_t* v; HIP_TRY(hipMalloc(&v, std::max<int64_t>(part.n_rows, 16)));
        part.d_valid[(int)ci] = v;
      }
    }
    // the fused path never materialises its value column (9 B/row of HBM),
    // unless the execute-time group-count check can still fall back
    if (plan->fused_valagg && !plan->valagg_late && (int)ci == plan->valagg_col)
      continue;
    if (c.need_val) {
      int64_t* d; HIP_TRY(hipMalloc(&d, std::max<int64_t>(part.n_rows * 8, 16)));
      part.d_val[(int)ci] = d;
      uint8_t* v; HIP_TRY(hipMalloc(&v, std::max<int64_t>(part.n_rows, 16)));
      part.d_valid[(int)ci] = v;
    }
  }
  HIP_TRY(hipMalloc(&part.d_mask, std::max<int64_t>(part.n_rows, 16)));
  // acc / tmp pairs of the non-folded OR groups (none for a flat plan)
  part.d_wbufs.assign(plan->n_wbufs, nullptr);
  for (auto& wb : part.d_wbufs)
    HIP_TRY(hipMalloc(&wb, std::max<int64_t>(part.n_rows, 16)));
  part.d_fbufs.assign(plan->filters.size(), nullptr);
  for (auto& fb : part.d_fbufs)
    HIP_TRY(hipMalloc(&fb, std::max<int64_t>(part.n_rows, 16)));
  HIP_TRY(hipMalloc(&part.d_rowof, std::max<int64_t>(part.n_rows * 4, 16)));
  HIP_TRY(hipMalloc(&part.d_rank, std::max<int64_t>(part.n_rows * 4, 16)));
  HIP_TRY(hipMalloc(&part.d_scr, std::max<int64_t>(part.n_rows * 8, 16)));
  HIP_TRY(hipMalloc(&part.d_present, std::max<size_t>(part.pages.size() * 4, 16)));
  HIP_TRY(hipMalloc(&part.d_tmpvalid, std::max<int64_t>(part.n_rows, 16)));
  if (plan->is_projection) {
    int64_t n = std::max<int64_t>(part.n_rows, 16);
    HIP_TRY(hipMalloc(&part.d_keys, n * 8));
    HIP_TRY(hipMalloc(&part.d_keys_sorted, n * 8));
    HIP_TRY(hipMalloc(&part.d_rows, n * 4));
    HIP_TRY(hipMalloc(&part.d_rows_sorted, n * 4));
    HIP_TRY(hipMalloc(&part.d_count, 8));
    part.sort_temp_bytes = sort_pairs_desc(part.stream, nullptr, 0, part.d_keys,
                                           part.d_keys_sorted, part.d_rows,
                                           part.d_rows_sorted, part.n_rows);
    HIP_TRY(hipMalloc(&part.d_sort_temp, std::max<size_t>(part.sort_temp_bytes, 16)));
  }
  HIP_TRY(hipMalloc(&part.d_err, 4));
  // with hash-mode group keys the cardinality is only known at execute:
  // size the tables for the cap
  bool hash_machinery = plan->has_hash || plan->needs_cascade ||
                        plan->has_numkey;
  size_t groups_cap = hash_machinery ? (size_t)GID_CAP : (size_t)plan->n_groups;
  size_t tsz = groups_cap * (1 + 2 * plan->aggs.size()) * 8;
  HIP_TRY(hipMalloc(&part.d_table, std::max<size_t>(tsz, 16)));
  size_t fsz = (size_t)plan->n_fsum * groups_cap * 4 * 8;
  HIP_TRY(hipMalloc(&part.d_fsum, std::max<size_t>(fsz, 16)));
  if (hash_machinery) {
    // +1 entry: the numeric-key overflow slot for the value that equals
    // the EMPTY sentinel (k_numhash_build)
    HIP_TRY(hipMalloc(&part.d_hkeys, ((1ull << HASH_LOG2) + 1) * 8));
    HIP_TRY(hipMalloc(&part.d_hgids, ((1ull << HASH_LOG2) + 1) * 4));
    HIP_TRY(hipMalloc(&part.d_hcount, 4));
    for (int ci : plan->group_cols)
      if (plan->cols[ci].hash_mode || plan->cols[ci].numeric_key) {
        uint64_t* g2r = nullptr;
        HIP_TRY(hipMalloc(&g2r, (size_t)GID_CAP * 8));
        part.d_gid2ref[ci] = g2r;
      }
    if (plan->group_cols.size() >= 2) {
      HIP_TRY(hipMalloc(&part.d_cgid, std::max<int64_t>(part.n_rows * 4, 16)));
      part.d_gid2pair.resize(plan->group_cols.size() - 1, nullptr);
      for (auto& ptr : part.d_gid2pair)
        HIP_TRY(hipMalloc(&ptr, (size_t)GID_CAP * 8));
    }
  }
  if (!plan->distinct_aggs.empty()) {
    // the hash-set path claims in the shared table (any cardinality can
    // fall to it); hash / numeric value columns resolve gids through a
    // gid2ref map of their own, like keys
    if (!part.d_hkeys)
      HIP_TRY(hipMalloc(&part.d_hkeys, ((1ull << HASH_LOG2) + 1) * 8));
    for (int ai : plan->distinct_aggs) {
      int ci = plan->aggs[ai].col_idx;
      const auto& c = plan->cols[ci];
      if ((c.hash_mode || c.numeric_key) && !part.d_gid2ref.count(ci)) {
        uint64_t* g2r = nullptr;
        HIP_TRY(hipMalloc(&g2r, (size_t)GID_CAP * 8));
        part.d_gid2ref[ci] = g2r;
      }
      uint64_t* pl = nullptr;
      HIP_TRY(hipMalloc(&pl, (size_t)plan->distinct_pair_cap * 8));
      part.d_dpairs.push_back(pl);
    }
    HIP_TRY(hipMalloc(&part.d_dcount, plan->distinct_aggs.size() * 4));
    if (!plan->distinct_force_hash)
      HIP_TRY(hipMalloc(&part.d_dbitmap,
                        std::max<uint64_t>(plan->distinct_bitmap_bits / 8 + 8, 16)));
  }
  std::vector<int32_t> kinds;
  for (auto& a : plan->aggs) kinds.push_back(a.kind);
  upload_pool(kinds.data(), kinds.size() * 4, (void**)&part.d_agg_kind);
  upload_pool(part.segs.data(), part.segs.size() * sizeof(DevSeg),
              (void**)&part.d_segs);
  upload_pool(part.brs.data(), part.brs.size() * sizeof(DevBr),
              (void**)&part.d_brs);
  upload_pool(part.pagebrs.data(), part.pagebrs.size() * sizeof(DevPageBr),
              (void**)&part.d_pagebrs);
  upload_pool(part.res_lane.data(), part.res_lane.size() * sizeof(DevBrRes),
              (void**)&part.d_res_lane);
  upload_pool(part.res_wave.data(), part.res_wave.size() * sizeof(DevBrRes),
              (void**)&part.d_res_wave);
  upload_pool(part.piece_pool.data(), part.piece_pool.size() * sizeof(DevPiece),
              (void**)&part.d_piece_pool);
  upload_pool(part.seqs.data(), part.seqs.size() * sizeof(DevSeq),
              (void**)&part.d_seqs);
  upload_pool(part.tiles.data(), part.tiles.size() * sizeof(DevSeqTile),
              (void**)&part.d_tiles);
  upload_pool(part.lits_wave.data(), part.lits_wave.size() * sizeof(DevLit),
              (void**)&part.d_lits_wave);
  if (!part.fork_cols.empty()) {
    // the early record set (delta fork), same shape as the main one
    const DecompRecs& E = part.early;
    DecompDev& D = part.d_early;
    auto up = [&](const auto& v, auto** dst) {
      upload_pool(v.data(), v.size() * sizeof(v[0]), (void**)dst);
    };
    up(E.segs, &D.d_segs); D.n_segs = (int)E.segs.size();
    up(E.seqs, &D.d_seqs);
    up(E.tiles, &D.d_tiles); D.n_tiles = (int)E.tiles.size();
    up(E.lits_wave, &D.d_lits_wave); D.n_lits_wave = (int)E.lits_wave.size();
    up(E.res_lane, &D.d_res_lane); D.n_res_lane = (int64_t)E.res_lane.size();
    up(E.res_wave, &D.d_res_wave); D.n_res_wave = (int)E.res_wave.size();
    up(E.piece_pool, &D.d_piece_pool);
    up(E.brs, &D.d_brs);
    up(E.pagebrs, &D.d_pagebrs); D.n_pagebrs = (int)E.pagebrs.size();
    D.seq_batch = plan->seq_tile_batch;
  }
  upload_pool(part.cwins.data(), part.cwins.size() * sizeof(DevCWin),
              (void**)&part.d_cwins);
  upload_pool(part.cstarts.data(), part.cstarts.size() * sizeof(uint16_t),
              (void**)&part.d_cstarts);
  // needle pool: every CONTAINS pred's literal, addressed per pred index
  // (two LIKE predicates — same or different columns — each launch with
  // their own needle)
  std::string needle;
  part.needle_off.assign(plan->preds.size(), 0);
  {
    std::string pool;
    for (size_t i = 0; i < plan->preds.size(); i++) {
      if (plan->preds[i].p.lit_kind == GPUQ_LIT_STR) {
        part.needle_off[i] = (uint32_t)pool.size();
        pool += plan->preds[i].str_lit;
        pool.push_back('\0');
      }
    }
    needle = pool;
  }
  upload_pool(needle.data(), needle.size() + 1, (void**)&part.d_needle);

  HIP_TRY(hipStreamSynchronize(part.stream));
  part.loaded = true;
  part.load_ns = now_ns() - t0;
  {
    std::lock_guard<std::mutex> g(plan->mu);
    plan->m_load_ns += part.load_ns;
  }
  return 0;
} catch (const std::exception& e) {
  if (plan && plan->ctx) plan->ctx->set_error(e.what());
  return -1;
}

// ------------------------------------------------------------------
// execute
// ------------------------------------------------------------------
namespace {

// Arrow C export helpers ------------------------------------------------
struct ExportedBatch {
  // buffers we hand to Arrow; freed on release
  std::vector<void*> allocs;
  void* grab(size_t n) {
    void* p = malloc(n ? n : 1);
    allocs.push_back(p);
    return p;
  }
};

void release_schema(struct ArrowSchema* s) {
  if (!s || !s->release) return;
  for (int64_t i = 0; i < s->n_children; i++)
    if (s->children[i]) { release_schema(s->children[i]); free(s->children[i]); }
  free(s->children);
  free((void*)s->format);
  free((void*)s->name);
  s->release = nullptr;
}
void release_array(struct ArrowArray* a) {
  if (!a || !a->release) return;
  for (int64_t i = 0; i < a->n_children; i++)
    if (a->children[i]) { release_array(a->children[i]); free(a->children[i]); }
  free(a->children);
  if (a->private_data) {
    auto* eb = (ExportedBatch*)a->private_data;
    for (void* p : eb->allocs) free(p);
    delete eb;
  }
  free(a->buffers);
  a->release = nullptr;
}

void make_schema_field(struct ArrowSchema* s, const char* fmt, const std::string& name) {
  memset(s, 0, sizeof(*s));
  s->format = strdup(fmt);
  s->name = strdup(name.c_str());
  s->flags = 2;  // ARROW_FLAG_NULLABLE
  s->release = release_schema;
}

struct StreamState {
  struct ArrowSchema schema;
  bool schema_moved = false;
  struct ArrowArray batch;
  bool batch_taken = false;
  std::string err;
};

int ss_get_schema(struct ArrowArrayStream* st, struct ArrowSchema* out) {
  auto* s = (StreamState*)st->private_data;
  // deep-ish copy: rebuild (simplest: move once; pyarrow calls once)
  *out = s->schema;
  s->schema_moved = true;
  s->schema.release = nullptr;
  return 0;
}
int ss_get_next(struct ArrowArrayStream* st, struct ArrowArray* out) {
  auto* s = (StreamState*)st->private_data;
  if (s->batch_taken) {
    memset(out, 0, sizeof(*out));
    out->release = nullptr;
    return 0;
  }
  *out = s->batch;
  s->batch.release = nullptr;
  s->batch_taken = true;
  return 0;
}
const char* ss_get_last_error(struct ArrowArrayStream* st) {
  auto* s = (StreamState*)st->private_data;
  return s->err.empty() ? nullptr : s->err.c_str();
}
void stream_state_free(StreamState* s) {
  if (s->schema.release) release_schema(&s->schema);
  if (s->batch.release) release_array(&s->batch);
  delete s;
}
void ss_release(struct ArrowArrayStream* st) {
  auto* s = (StreamState*)st->private_data;
  if (s) stream_state_free(s);
  st->release = nullptr;
}

// Fetch the [len][bytes] strings behind a list of strrefs from the device
// dec arena (export side of the raw-byte utf8 path): lens kernel -> host
// prefix -> gather kernel -> one packed D2H.
std::vector<std::string> fetch_ref_strings(Partition& part, hipStream_t st,
                                           const std::vector<uint64_t>& refs) {
  int64_t n = (int64_t)refs.size();
  std::vector<std::string> out(n);
  if (!n) return out;
  uint64_t* d_refs = nullptr;
  uint32_t* d_lens = nullptr;
  HIP_TRY(hipMalloc(&d_refs, n * 8));
  HIP_TRY(hipMalloc(&d_lens, n * 4));
  HIP_TRY(hipMemcpyAsync(d_refs, refs.data(), n * 8, hipMemcpyHostToDevice, st));
  launch_ref_lens(st, part.d_dec, d_refs, n, d_lens);
  std::vector<uint32_t> lens(n);
  HIP_TRY(hipMemcpyAsync(lens.data(), d_lens, n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  std::vector<uint64_t> offs(n);
  uint64_t total = 0;
  for (int64_t i = 0; i < n; i++) { offs[i] = total; total += lens[i]; }
  uint64_t* d_offs = nullptr;
  uint8_t* d_out = nullptr;
  HIP_TRY(hipMalloc(&d_offs, n * 8));
  HIP_TRY(hipMalloc(&d_out, std::max<uint64_t>(total, 16)));
  HIP_TRY(hipMemcpyAsync(d_offs, offs.data(), n * 8, hipMemcpyHostToDevice, st));
  launch_ref_gather(st, part.d_dec, d_refs, d_offs, n, d_out);
  std::vector<uint8_t> bytes(total);
  if (total)
    HIP_TRY(hipMemcpyAsync(bytes.data(), d_out, total, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int64_t i = 0; i < n; i++)
    out[i].assign((const char*)bytes.data() + offs[i], lens[i]);
  (void)hipFree(d_refs); (void)hipFree(d_lens);
  (void)hipFree(d_offs); (void)hipFree(d_out);
  return out;
}

// Hot-tier population: after the first execute of a partition (arena now
// holds every decompressed chunk image), copy uncached chunk images into
// the session cache (D2D at HBM rates).
void hot_tier_populate(gpuq_plan* plan, Partition& part, hipStream_t st) {
  if (part.populated) return;
  part.populated = true;
  bool any = false;
  for (auto& t : part.chunks) {
    if (t.cached || !t.dec_len) continue;
    void* dev = nullptr;
    if (hipMalloc(&dev, t.dec_len) != hipSuccess) break;  // HBM full: stop
    HIP_TRY(hipMemcpyAsync(dev, part.d_dec + t.dec_base, t.dec_len,
                           hipMemcpyDeviceToDevice, st));
    plan->ctx->cache_put(t.cache_key, dev, t.dec_len, part.device);
    any = true;
  }
  if (any) HIP_TRY(hipStreamSynchronize(st));
}

// Round the exact 256-bit two's-complement fixed-point sum (lsb weight
// 2^-160; kernels.hip acc256_*) to the nearest double, ties to even —
// the once-per-query rounding that makes f64 SUM order-independent and
// within 1 ULP of the correctly rounded exact sum (BASELINE parity gate).
double acc256_to_double(const uint64_t li[4]) {
  uint64_t l[4] = {li[0], li[1], li[2], li[3]};
  bool neg = (l[3] >> 63) != 0;
  if (neg) {
    uint64_t c = 1;
    for (int i = 0; i < 4; i++) { l[i] = ~l[i] + c; c = (c && l[i] == 0) ? 1 : 0; }
  }
  int t = -1;
  for (int i = 3; i >= 0; i--)
    if (l[i]) { t = i * 64 + 63 - __builtin_clzll(l[i]); break; }
  if (t < 0) return 0.0;
  double d;
  if (t <= 52) {  // every bit fits the mantissa: exact
    d = ldexp((double)l[0], -160);
  } else {
    int sh = t - 52;  // keep bits [sh, t]; bits below are round/sticky
    auto word = [&](int i) -> uint64_t { return (i >= 0 && i < 4) ? l[i] : 0; };
    int wi = sh >> 6, sb = sh & 63;
    uint64_t mant = sb ? ((word(wi) >> sb) | (word(wi + 1) << (64 - sb)))
                       : word(wi);
    int rb = (int)((word((sh - 1) >> 6) >> ((sh - 1) & 63)) & 1);
    bool sticky = false;
    for (int i = 0; i < 4 && !sticky; i++) {
      int lo = i * 64;
      int top = sh - 2;  // highest sticky bit
      if (top < lo) break;
      uint64_t m = (top - lo >= 63) ? ~0ull : ((1ull << (top - lo + 1)) - 1);
      if (l[i] & m) sticky = true;
    }
    if (rb && (sticky || (mant & 1))) mant++;
    d = ldexp((double)mant, sh - 160);
  }
  return neg ? -d : d;
}

// ---- projection scans --------------------------------------------------
// Selected rows sorted by p_timestamp DESC (the console ordering contract,
// stream_schema_provider.rs:181-204). With a LIMIT the stream holds the
// top-k; without one it is a TRUE multi-batch ArrowArrayStream: each
// get_next gathers the next P_EXECUTION_BATCH_SIZE rows (20,000 — the
// reference batch size, cli.rs:476-482) from the device-resident sorted row
// list, so host and device memory stay bounded regardless of result size.
// The stream borrows the plan's device state: drain it before
// gpuq_plan_destroy.
namespace {
constexpr int64_t PROJ_BATCH = 20000;

struct ProjState {
  gpuq_plan* plan = nullptr;
  Partition* part = nullptr;
  int64_t total = 0, cursor = 0;
  struct ArrowSchema schema;
  bool schema_moved = false;
  std::string err;
  int64_t* d_g64 = nullptr;
  int32_t* d_g32 = nullptr;
  uint8_t* d_g8 = nullptr;
};

int proj_get_schema(struct ArrowArrayStream* st0, struct ArrowSchema* out) {
  auto* s = (ProjState*)st0->private_data;
  *out = s->schema;
  s->schema_moved = true;
  s->schema.release = nullptr;
  return 0;
}
const char* proj_get_last_error(struct ArrowArrayStream* st0) {
  auto* s = (ProjState*)st0->private_data;
  return s->err.empty() ? nullptr : s->err.c_str();
}
void proj_state_free(ProjState* s) {
  if (s->schema.release) release_schema(&s->schema);
  if (s->d_g64) (void)hipFree(s->d_g64);
  if (s->d_g32) (void)hipFree(s->d_g32);
  if (s->d_g8) (void)hipFree(s->d_g8);
  delete s;
}
void proj_release(struct ArrowArrayStream* st0) {
  auto* s = (ProjState*)st0->private_data;
  if (s) proj_state_free(s);
  st0->release = nullptr;
}

int proj_get_next(struct ArrowArrayStream* st0, struct ArrowArray* out) try {
  auto* s = (ProjState*)st0->private_data;
  gpuq_plan* plan = s->plan;
  Partition& part = *s->part;
  if (s->cursor >= s->total) {
    memset(out, 0, sizeof(*out));
    out->release = nullptr;
    return 0;
  }
  HIP_TRY(hipSetDevice(part.device));
  hipStream_t st = part.stream;
  const int64_t k = std::min<int64_t>(PROJ_BATCH, s->total - s->cursor);
  const uint32_t* rows = part.d_rows_sorted + s->cursor;
  int np = (int)plan->projection.size();

  std::vector<std::vector<int64_t>> vals(np);
  std::vector<std::vector<int32_t>> gids(np);
  std::vector<std::vector<uint8_t>> valids(np);
  std::vector<std::vector<std::string>> pstrs(np);
  for (int p = 0; p < np; p++) {
    int ci = plan->projection[p];
    auto& c = plan->cols[ci];
    if (c.phys == PT_BYTE_ARRAY && c.hash_mode) {
      std::vector<int64_t> refs(k);
      valids[p].assign(k, 1);
      launch_gather_i64(st, rows, k, part.d_val[ci], s->d_g64);
      HIP_TRY(hipMemcpyAsync(refs.data(), s->d_g64, k * 8,
                             hipMemcpyDeviceToHost, st));
      auto itv = part.d_valid.find(ci);
      if (itv != part.d_valid.end()) {
        launch_gather_u8(st, rows, k, itv->second, s->d_g8);
        HIP_TRY(hipMemcpyAsync(valids[p].data(), s->d_g8, k,
                               hipMemcpyDeviceToHost, st));
      }
      HIP_TRY(hipStreamSynchronize(st));
      std::vector<uint64_t> vr;
      std::vector<int64_t> vrow;
      for (int64_t r = 0; r < k; r++)
        if (valids[p][r]) { vr.push_back((uint64_t)refs[r]); vrow.push_back(r); }
      auto strs = fetch_ref_strings(part, st, vr);
      pstrs[p].assign(k, std::string());
      for (size_t j = 0; j < vrow.size(); j++)
        pstrs[p][vrow[j]] = std::move(strs[j]);
    } else if (c.phys == PT_BYTE_ARRAY) {
      gids[p].resize(k);
      launch_gather_i32(st, rows, k, part.d_gid[ci], s->d_g32);
      HIP_TRY(hipMemcpyAsync(gids[p].data(), s->d_g32, k * 4,
                             hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    } else {
      vals[p].resize(k);
      valids[p].assign(k, 1);
      launch_gather_i64(st, rows, k, part.d_val[ci], s->d_g64);
      HIP_TRY(hipMemcpyAsync(vals[p].data(), s->d_g64, k * 8,
                             hipMemcpyDeviceToHost, st));
      auto itv = part.d_valid.find(ci);
      if (itv != part.d_valid.end()) {
        launch_gather_u8(st, rows, k, itv->second, s->d_g8);
        HIP_TRY(hipMemcpyAsync(valids[p].data(), s->d_g8, k,
                               hipMemcpyDeviceToHost, st));
      }
      HIP_TRY(hipStreamSynchronize(st));
    }
  }

  auto* eb = new ExportedBatch();
  memset(out, 0, sizeof(*out));
  out->length = k;
  out->n_buffers = 1;
  out->buffers = (const void**)calloc(1, sizeof(void*));
  out->n_children = np;
  out->children = (struct ArrowArray**)calloc(np, sizeof(void*));
  out->release = release_array;
  out->private_data = eb;
  for (int p = 0; p < np; p++) {
    auto* ch = (struct ArrowArray*)calloc(1, sizeof(struct ArrowArray));
    out->children[p] = ch;
    ch->length = k;
    ch->release = release_array;
    auto& c = plan->cols[plan->projection[p]];
    if (c.phys == PT_BYTE_ARRAY) {
      bool via_ref = c.hash_mode;
      auto str_at = [&](int64_t r) -> const std::string* {
        if (via_ref) return valids[p][r] ? &pstrs[p][r] : nullptr;
        int32_t g = gids[p][r];
        return g > 0 ? &c.gdict[g - 1] : nullptr;
      };
      ch->n_buffers = 3;
      ch->buffers = (const void**)calloc(3, sizeof(void*));
      uint8_t* validity = (uint8_t*)eb->grab((k + 7) / 8);
      memset(validity, 0xff, std::max<int64_t>((k + 7) / 8, 1));
      int32_t* offs = (int32_t*)eb->grab((k + 1) * 4);
      size_t total = 0;
      for (int64_t r = 0; r < k; r++)
        if (const std::string* sp = str_at(r)) total += sp->size();
      char* data = (char*)eb->grab(total);
      size_t off = 0;
      int64_t nulls = 0;
      for (int64_t r = 0; r < k; r++) {
        offs[r] = (int32_t)off;
        if (const std::string* sp = str_at(r)) {
          memcpy(data + off, sp->data(), sp->size());
          off += sp->size();
        } else {
          validity[r / 8] &= (uint8_t)~(1 << (r % 8));
          nulls++;
        }
      }
      offs[k] = (int32_t)off;
      if (nulls) { ch->buffers[0] = validity; ch->null_count = nulls; }
      ch->buffers[1] = offs;
      ch->buffers[2] = data;
    } else {
      ch->n_buffers = 2;
      ch->buffers = (const void**)calloc(2, sizeof(void*));
      int64_t* v = (int64_t*)eb->grab(std::max<int64_t>(k * 8, 1));
      uint8_t* validity = (uint8_t*)eb->grab(std::max<int64_t>((k + 7) / 8, 1));
      memset(validity, 0xff, std::max<int64_t>((k + 7) / 8, 1));
      int64_t nulls = 0;
      for (int64_t r = 0; r < k; r++) {
        v[r] = vals[p][r];
        if (!valids[p][r]) {
          validity[r / 8] &= (uint8_t)~(1 << (r % 8));
          nulls++;
        }
      }
      if (nulls) { ch->buffers[0] = validity; ch->null_count = nulls; }
      ch->buffers[1] = v;
    }
  }
  s->cursor += k;
  return 0;
} catch (const std::exception& e) {
  auto* s = (ProjState*)st0->private_data;
  s->err = e.what();
  return 1;
}

}  // namespace

// The events of one execute: created at entry, destroyed on every exit.
// A delta fork in flight is part of that state: fork_side() starts the side
// stream behind the main stream's work so far, join_side() makes the main
// stream wait for it, and an exit between the two (a throw) drains the side
// stream first, so no launch outlives the call.
struct ExecEvents {
  hipEvent_t ev0 = nullptr, ev1 = nullptr, decomp = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  hipStream_t side = nullptr;   // non-null between fork_side and join_side
  ExecEvents() = default;
  ExecEvents(const ExecEvents&) = delete;
  ExecEvents& operator=(const ExecEvents&) = delete;
  void create() {
    HIP_TRY(hipEventCreate(&ev0));
    HIP_TRY(hipEventCreate(&ev1));
    HIP_TRY(hipEventCreate(&decomp));
  }
  void fork_side(hipStream_t main, hipStream_t sd) {
    HIP_TRY(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&join, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(fork, main));
    HIP_TRY(hipStreamWaitEvent(sd, fork, 0));
    side = sd;
  }
  void join_side(hipStream_t main) {
    if (!side) return;
    HIP_TRY(hipEventRecord(join, side));
    HIP_TRY(hipStreamWaitEvent(main, join, 0));
    side = nullptr;
  }
  ~ExecEvents() {
    if (side) (void)hipStreamSynchronize(side);
    for (hipEvent_t e : {ev0, ev1, decomp, fork, join})
      if (e) (void)hipEventDestroy(e);
  }
};

// GPUQ_EQ..GE -> CMP_*; -1 for every other op (the callers own BETWEEN and
// the LIKE family)
int cmp_mode_of(int op) {
  switch (op) {
    case GPUQ_EQ: return CMP_EQ;
    case GPUQ_NE: return CMP_NE;
    case GPUQ_LT: return CMP_LT;
    case GPUQ_LE: return CMP_LE;
    case GPUQ_GT: return CMP_GT;
    case GPUQ_GE: return CMP_GE;
    default: return -1;
  }
}

// ---- Arrow column builders over ExportedBatch::grab ----------------------
// Each fills n_buffers / buffers / null_count of a child whose length is
// set; buffers[0] stays nullptr when the column has no nulls.

// int64 (or f64 bit pattern) values; valid: one byte per row, 0 = NULL
// (nullptr: no nulls)
void set_i64_column(ExportedBatch& eb, struct ArrowArray* ch,
                    const std::vector<int64_t>& vals,
                    const std::vector<uint8_t>* valid = nullptr) {
  const size_t n = vals.size();
  ch->n_buffers = 2;
  ch->buffers = (const void**)calloc(2, sizeof(void*));
  int64_t* v = (int64_t*)eb.grab(n * 8);
  if (n) memcpy(v, vals.data(), n * 8);
  ch->buffers[1] = v;
  if (!valid) return;
  uint8_t* validity = (uint8_t*)eb.grab((n + 7) / 8);
  memset(validity, 0xff, (n + 7) / 8);
  int64_t nulls = 0;
  for (size_t r = 0; r < n; r++)
    if (!(*valid)[r]) {
      validity[r / 8] &= (uint8_t)~(1 << (r % 8));
      nulls++;
    }
  if (nulls) { ch->buffers[0] = validity; ch->null_count = nulls; }
}

// utf8 from one string pointer per row, NULL where it is nullptr
void set_utf8_column(ExportedBatch& eb, struct ArrowArray* ch,
                     const std::vector<const std::string*>& strs) {
  const size_t n = strs.size();
  ch->n_buffers = 3;
  ch->buffers = (const void**)calloc(3, sizeof(void*));
  uint8_t* validity = (uint8_t*)eb.grab((n + 7) / 8);
  memset(validity, 0xff, (n + 7) / 8);
  int32_t* offs = (int32_t*)eb.grab((n + 1) * 4);
  size_t total = 0;
  for (const std::string* s : strs)
    if (s) total += s->size();
  char* data = (char*)eb.grab(total);
  size_t off = 0;
  int64_t nulls = 0;
  for (size_t r = 0; r < n; r++) {
    offs[r] = (int32_t)off;
    if (strs[r]) {
      memcpy(data + off, strs[r]->data(), strs[r]->size());
      off += strs[r]->size();
    } else {
      validity[r / 8] &= (uint8_t)~(1 << (r % 8));
      nulls++;
    }
  }
  offs[n] = (int32_t)off;
  if (nulls) { ch->buffers[0] = validity; ch->null_count = nulls; }
  ch->buffers[1] = offs;
  ch->buffers[2] = data;
}

// list offsets (rows + 1 entries); the caller attaches the item child
void set_list_offsets(ExportedBatch& eb, struct ArrowArray* ch,
                      const std::vector<int32_t>& offs) {
  ch->n_buffers = 2;
  ch->buffers = (const void**)calloc(2, sizeof(void*));
  int32_t* o = (int32_t*)eb.grab(offs.size() * 4);
  memcpy(o, offs.data(), offs.size() * 4);
  ch->buffers[1] = o;
}

// the count slot of aggregate i in one group's table row (base = its first
// slot). count(*) == presence: k_agg spends no atomics on its slots; same
// for any agg whose column is footer-proven null-free (cnt_is_presence)
uint64_t agg_count(const std::vector<uint64_t>& table, size_t base, int i,
                   int kind, bool cnt_is_presence) {
  return (kind == AGGK_COUNT_STAR || cnt_is_presence) ? table[base]
                                                      : table[base + 2 + 2 * i];
}

// reset the shared open-addressing table (keys, gids, claim counter) over
// `slots` entries: each site keeps its own size
void reset_hash_table(Partition& part, hipStream_t st, uint64_t slots) {
  HIP_TRY(hipMemsetAsync(part.d_hkeys, 0xFF, slots * 8, st));
  HIP_TRY(hipMemsetAsync(part.d_hgids, 0xFF, slots * 4, st));
  HIP_TRY(hipMemsetAsync(part.d_hcount, 0, 4, st));
}
// the claimed count of the build just enqueued (synchronises the stream)
uint32_t read_claimed(Partition& part, hipStream_t st) {
  uint32_t claimed = 0;
  HIP_TRY(hipMemcpyAsync(&claimed, part.d_hcount, 4, hipMemcpyDeviceToHost,
                         st));
  HIP_TRY(hipStreamSynchronize(st));
  return claimed;
}

// One of the four value-decode kinds (TK_DICT_GID, TK_DICT_VAL, TK_PLAIN_VAL,
// TK_POOL_VAL) through its launcher launch(dst, valid, present, mode).
// Footer-proven null-free column: the direct decode alone, validity asserted
// (mode 2) — the def-level pass, the scratch decode and the expansion would
// each find nothing to do. Otherwise def levels, the direct decode of
// null-free pages (mode 0), the dense decode of the others into d_scr
// (mode 1) and its expansion to row positions.
template <class Launch>
void decode_values(Partition& part, hipStream_t st, const int32_t* ids, int n,
                   bool null_free, Launch&& launch, void* dst, uint8_t* valid,
                   uint8_t* levels_valid, int expand_mode) {
  if (null_free) {
    launch(dst, valid, nullptr, 2);
    return;
  }
  launch_def_levels(st, part.d_dec, part.d_pages, ids, n, levels_valid,
                    nullptr, nullptr, part.d_rank, part.d_present, part.d_err);
  launch(dst, valid, part.d_present, 0);
  launch(part.d_scr, nullptr, part.d_present, 1);
  launch_expand(st, part.d_dec, part.d_pages, ids, n, part.d_scr, part.d_rank,
                levels_valid, (uint8_t*)dst, expand_mode);
}

int32_t execute_projection(gpuq_plan* plan, Partition& part,
                           const ExecEvents& events, int64_t t0,
                           bool need_mask, struct ArrowArrayStream* out) {
  hipStream_t st = part.stream;
  const hipEvent_t ev0 = events.ev0, ev1 = events.ev1,
                   ev_decomp = events.decomp;
  // compact selected (ts,row) pairs -> radix sort desc -> batched gather
  HIP_TRY(hipMemsetAsync(part.d_count, 0, 8, st));
  launch_compact(st, need_mask ? part.d_mask : nullptr,
                 part.d_val[plan->ts_col], part.n_rows, part.d_keys,
                 part.d_rows, part.d_count);
  unsigned long long cnt = 0;
  HIP_TRY(hipMemcpyAsync(&cnt, part.d_count, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (cnt)
    sort_pairs_desc(st, part.d_sort_temp, part.sort_temp_bytes, part.d_keys,
                    part.d_keys_sorted, part.d_rows, part.d_rows_sorted,
                    (int64_t)cnt);
  int64_t k = plan->limit > 0 ? std::min<int64_t>((int64_t)cnt, plan->limit)
                              : (int64_t)cnt;

  HIP_TRY(hipEventRecord(ev1, st));
  int32_t herr = 0;
  HIP_TRY(hipMemcpyAsync(&herr, part.d_err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (herr != 0)
    throw std::runtime_error("kernel error code " + std::to_string(herr));
  hot_tier_populate(plan, part, st);
  float ms_total = 0, ms_decomp = 0;
  HIP_TRY(hipEventElapsedTime(&ms_total, ev0, ev1));
  HIP_TRY(hipEventElapsedTime(&ms_decomp, ev0, ev_decomp));

  int np = (int)plan->projection.size();
  // owned here until `out` takes it: a throw below frees the schema and the
  // three device buffers through the stream's own release path
  std::unique_ptr<ProjState, void (*)(ProjState*)> ps(new ProjState(),
                                                      proj_state_free);
  memset(&ps->schema, 0, sizeof(ps->schema));
  ps->plan = plan;
  ps->part = &part;
  ps->total = k;
  HIP_TRY(hipMalloc(&ps->d_g64, PROJ_BATCH * 8));
  HIP_TRY(hipMalloc(&ps->d_g32, PROJ_BATCH * 4));
  HIP_TRY(hipMalloc(&ps->d_g8, PROJ_BATCH));
  ps->schema.format = strdup("+s");
  ps->schema.name = strdup("");
  ps->schema.release = release_schema;
  ps->schema.n_children = np;
  ps->schema.children = (struct ArrowSchema**)calloc(np, sizeof(void*));
  for (int p = 0; p < np; p++) {
    auto& c = plan->cols[plan->projection[p]];
    const char* fmt = (c.phys == PT_BYTE_ARRAY) ? "u"
                      : (c.phys == PT_DOUBLE) ? "g" : "l";
    ps->schema.children[p] = (struct ArrowSchema*)malloc(sizeof(struct ArrowSchema));
    make_schema_field(ps->schema.children[p], fmt, c.name);
  }
  memset(out, 0, sizeof(*out));
  out->get_schema = proj_get_schema;
  out->get_next = proj_get_next;
  out->get_last_error = proj_get_last_error;
  out->release = proj_release;
  out->private_data = ps.release();

  {
    std::lock_guard<std::mutex> g(plan->mu);
    plan->m_kernel_ns += (int64_t)(ms_total * 1e6);
    plan->m_decomp_ns += (int64_t)(ms_decomp * 1e6);
    plan->m_exec_ns += now_ns() - t0;
    plan->m_rows_out += k;
  }
  return 0;
}

}  // namespace

extern "C" int32_t gpuq_plan_execute(gpuq_plan* plan, int32_t pi,
                                     struct ArrowArrayStream* out) try {
  if (!plan || pi < 0 || pi >= (int32_t)plan->parts.size()) return -1;
  Partition& part = plan->parts[pi];
  if (!part.loaded) {
    if (gpuq_plan_load(plan, pi) != 0) return -1;
  }
  HIP_TRY(hipSetDevice(part.device));
  hipStream_t st = part.stream;
  int64_t t0 = now_ns();
  const bool dw = plan->dict_serial;  // serial_walk of the dict launches

  ExecEvents events;  // destroyed on every exit, a throw included
  events.create();
  const hipEvent_t ev0 = events.ev0, ev1 = events.ev1,
                   ev_decomp = events.decomp;

  // a query whose every predicate is chunk-stats-proven everywhere needs no
  // selection mask at all (string/contains preds are never elided, so their
  // presence keeps pred_ranges non-empty)
  // Filter leaves do not count: the WHERE mask may be absent while filter
  // buffers exist.
  bool need_mask = false;
  for (const auto& pr : part.pred_ranges)
    need_mask |= plan->pred_filter[pr.first] < 0;
  HIP_TRY(hipMemsetAsync(part.d_err, 0, 4, st));
  if (need_mask) HIP_TRY(hipMemsetAsync(part.d_mask, 1, part.n_rows, st));
  // group count with hash keys is only known after the hash build, so the
  // table init moves to just before aggregation; n_groups_exec tracks it
  int64_t n_groups_exec = plan->n_groups;
  bool cascaded = false;
  std::vector<uint32_t> level_claimed;
  // per distinct agg: 0 = the hash-set path ran, 1 = the bitmap path marking
  // in global memory, 2 = the bitmap path marking through LDS
  std::vector<char> distinct_bitmap(plan->distinct_aggs.size(), 0);
  auto key_card = [&](int ci) -> int64_t {
    const auto& kc = plan->cols[ci];
    return kc.is_bin ? (int64_t)kc.nbins + 1
           : (kc.hash_mode || kc.numeric_key)
               ? (int64_t)part.hash_claimed[ci] + 1
               : (int64_t)kc.gdict.size() + 1;
  };
  if (plan->fused_count)
    launch_init_table(st, part.d_table, plan->n_groups, (int)plan->aggs.size(),
                      part.d_agg_kind);

  HIP_TRY(hipEventRecord(ev0, st));
  // i64 / f64 comparisons of column ci in WHERE context k, into mk
  auto cmp_col = [&](hipStream_t s, int ci, int k, uint8_t* mk) {
    auto& c = plan->cols[ci];
    for (int pidx : c.cmp_preds) {
      if (plan->ctx_of(pidx) != k) continue;
      const auto& pp = plan->preds[pidx];
      int mode = pp.p.op == GPUQ_BETWEEN ? CMP_RANGE : cmp_mode_of(pp.p.op);
      if (mode < 0) throw std::runtime_error("bad cmp op");
      int is_f64 = (c.phys == PT_DOUBLE) ? 1 : 0;
      int64_t lo = pp.p.i64[0], hi = pp.p.i64[1];
      if (is_f64) {
        memcpy(&lo, &pp.p.f64[0], 8);
        memcpy(&hi, &pp.p.f64[1], 8);
      }
      // evaluate only over the row ranges the chunk stats could not prove
      // (pred_all_true); proven rows keep their memset-1 mask
      auto rit = part.pred_ranges.find(pidx);
      if (rit == part.pred_ranges.end()) continue;
      for (const auto& [row0, nrows] : rit->second)
        launch_cmp_i64(s, part.d_val[ci] + row0, part.d_valid[ci] + row0,
                       lo, hi, mode, pp.p.hi_exclusive, is_f64,
                       mk + row0, nrows);
    }
  };
  // 0. delta fork: behind the memsets above, the side stream
  // decompresses the early set, delta-decodes the fork columns and evaluates
  // their comparisons into d_mask, beside the main stream's decompress and
  // key / value decode. The main stream joins before its first launch that
  // touches d_mask (mask tasks, row_preds) and in every case before ev1.
  const bool forked = !part.fork_cols.empty();
  auto is_fork_col = [&](int ci) {
    return std::find(part.fork_cols.begin(), part.fork_cols.end(), ci) !=
           part.fork_cols.end();
  };
  if (forked) {
    hipStream_t sd = part.side;
    events.fork_side(st, sd);
    DecompDev E = part.d_early;
    E.d_raw = part.d_raw;
    E.d_dec = part.d_dec;
    E.d_err = part.d_err;
    launch_decompress(sd, E);
    for (int ci : part.fork_cols) {
      auto it = part.tasks.find({TK_DELTA_VAL, ci});
      if (it != part.tasks.end())
        launch_delta_i64(sd, part.d_dec, part.d_pages, part.d_ids[it->first],
                         (int)it->second.size(), part.d_val[ci],
                         part.d_valid[ci], part.d_err);
      cmp_col(sd, ci, 0, part.d_mask);
    }
    if (plan->exec_dbg)
      fprintf(stderr, "[gpuq exec] part %d: delta fork cols=%zu\n", (int)pi,
              part.fork_cols.size());
  }
  // 1. decompress: parallel segments, then ordered backref resolution
  // (launch_decompress, shared with the test-support entry)
  launch_decompress(st, DecompDev{
      part.d_raw, part.d_dec,
      part.d_segs, (int)part.segs.size(),
      part.d_seqs, part.d_tiles, (int)part.tiles.size(), plan->seq_tile_batch,
      part.d_lits_wave, (int)part.lits_wave.size(),
      part.d_res_lane, (int64_t)part.res_lane.size(),
      part.d_res_wave, (int)part.res_wave.size(),
      part.d_piece_pool, part.d_brs,
      part.d_pagebrs, (int)part.pagebrs.size(), part.d_err});
  HIP_TRY(hipEventRecord(ev_decomp, st));

  // 2. decode + predicate kernels (or the fused count path)
  if (plan->fused_count) {
    int key_col = plan->group_cols[0];
    auto it = part.tasks.find({TK_DICT_GID, key_col});
    if (it != part.tasks.end())
      launch_dict_count(st, part.d_dec, part.d_pages, part.d_ids[it->first],
                        (int)it->second.size(), part.d_remap, part.d_table,
                        plan->n_groups, (int)plan->aggs.size(), part.d_err);
    events.join_side(st);
    HIP_TRY(hipEventRecord(ev1, st));
  } else {
  auto run_task = [&](const std::pair<const std::pair<int, int>,
                                      std::vector<int32_t>>& kv,
                      uint8_t* mk) {
    // mk: the mask buffer of the task's WHERE context (d_mask for context
    // 0); d_lut: that context's LUT slot of the column
    const int kind = tk_kind(kv.first.first), kctx = tk_ctx_of(kv.first.first);
    const int col = kv.first.second;
    int n = (int)kv.second.size();
    int32_t* ids = part.d_ids[kv.first];
    const uint8_t* d_lut = part.d_lut;
    if (plan->exec_dbg &&
        (kind == TK_DICT_GID || kind == TK_DICT_VAL || kind == TK_DICT_MASK))
      fprintf(stderr,
              "[gpuq exec] part %d: dict decode col=%s pages=%d dict_walk=%s\n",
              pi, plan->cols[col].name.c_str(), n,
              dw ? "serial" : "scan");
    if (kind == TK_DICT_MASK) {
      const auto& lc = plan->cols[col].lut_ctxs;
      d_lut += (size_t)(std::find(lc.begin(), lc.end(), kctx) - lc.begin()) *
               part.lut_pool.size();
    }
    // footer-proven null-free column: the direct decode alone (mode 2)
    const bool null_free = part.col_null_free[col] != 0;
    switch (kind) {
      case TK_DICT_GID: {
        // a column without a validity array of its own (gid only) still
        // needs one for the def levels and the expansion: d_tmpvalid
        auto it = part.d_valid.find(col);
        uint8_t* valid = it != part.d_valid.end() ? it->second : nullptr;
        decode_values(
            part, st, ids, n, null_free,
            [&](void* dst, uint8_t* v, const uint32_t* present, int mode) {
              launch_dict_gid(st, part.d_dec, part.d_pages, ids, n,
                              part.d_remap, (int32_t*)dst, v, present, mode,
                              dw, part.d_err);
            },
            part.d_gid[col], valid, valid ? valid : part.d_tmpvalid, 1);
        break;
      }
      case TK_DICT_VAL:
        decode_values(
            part, st, ids, n, null_free,
            [&](void* dst, uint8_t* v, const uint32_t* present, int mode) {
              launch_dict_i64(st, part.d_dec, part.d_pages, ids, n,
                              part.d_dictv, (int64_t*)dst, v, present, mode,
                              dw, part.d_err);
            },
            part.d_val[col], part.d_valid[col], part.d_valid[col], 0);
        break;
      case TK_PLAIN_VAL:
        decode_values(
            part, st, ids, n, null_free,
            [&](void* dst, uint8_t* v, const uint32_t* present, int mode) {
              launch_plain_fixed(st, part.d_dec, part.d_pages, ids, n,
                                 (int64_t*)dst, v, present, mode, part.d_err);
            },
            part.d_val[col], part.d_valid[col], part.d_valid[col], 0);
        break;
      case TK_POOL_VAL:  // PLAIN byte-array pages of hash cols -> strrefs
        decode_values(
            part, st, ids, n, null_free,
            [&](void* dst, uint8_t* v, const uint32_t* present, int mode) {
              launch_pool_vals(st, part.d_dec, part.d_pages, ids, n,
                               part.d_dictv, (int64_t*)dst, v, present, mode);
            },
            part.d_val[col], part.d_valid[col], part.d_valid[col], 0);
        break;
      case TK_DELTA_VAL:
        launch_delta_i64(st, part.d_dec, part.d_pages, ids, n,
                         part.d_val[col], part.d_valid[col], part.d_err);
        break;
      case TK_DICT_MASK:
        if (null_free) {
          launch_dict_mask(st, part.d_dec, part.d_pages, ids, n, d_lut, mk, 2,
                           dw, part.d_err);
          break;
        }
        // the scratch pass is the LUT byte per dense value, not a decode
        launch_def_levels(st, part.d_dec, part.d_pages, ids, n,
                          part.d_tmpvalid, nullptr, nullptr,
                          part.d_rank, part.d_present, part.d_err);
        launch_dict_mask(st, part.d_dec, part.d_pages, ids, n, d_lut,
                         mk, 0, dw, part.d_err);
        launch_dict_lut_scr(st, part.d_dec, part.d_pages, ids, n, d_lut,
                            part.d_scr, part.d_present, dw, part.d_err);
        launch_expand(st, part.d_dec, part.d_pages, ids, n, part.d_scr,
                      part.d_rank, part.d_tmpvalid, mk, 2);
        break;
      case TK_BYTES_CONTAINS: {
        // def levels zero null rows in the mask and build the dense->row
        // map; the window kernel then has no serial work at all
        launch_def_levels(st, part.d_dec, part.d_pages, ids, n,
                          part.d_tmpvalid, mk, part.d_rowof,
                          part.d_rank, part.d_present, part.d_err);
        auto rng = part.cwin_ranges.at(col);
        // one launch per LIKE-family pred, each with its own needle (mask &=)
        for (int pidx : plan->cols[col].contains_preds) {
          if (plan->ctx_of(pidx) != kctx) continue;
          const std::string& lit = plan->preds[pidx].str_lit;
          launch_str_win(st, part.d_dec, part.d_cwins + rng.first,
                         (int)rng.second, part.d_pages, part.d_cstarts,
                         part.d_needle + part.needle_off[pidx],
                         (int)lit.size(), like_mode(plan->preds[pidx].p.op),
                         part.d_rowof, mk);
        }
        break;
      }
      case TK_IS_NOT_NULL:
        // the null_mask output clears NULL rows; all-valid pages return early
        launch_def_levels(st, part.d_dec, part.d_pages, ids, n,
                          part.d_tmpvalid, mk, nullptr, nullptr,
                          part.d_present, part.d_err);
        break;
      case TK_IS_NULL:
        launch_def_levels(st, part.d_dec, part.d_pages, ids, n,
                          part.d_tmpvalid, nullptr, nullptr, nullptr,
                          part.d_present, part.d_err);
        launch_null_clear_valid(st, part.d_dec, part.d_pages, ids, n,
                                part.d_tmpvalid, mk);
        break;
    }
  };
  for (auto& kv : part.tasks) {
    // the fused path aggregates this column where it decodes it (step 3)
    if (plan->fused_valagg && kv.first.second == plan->valagg_col) continue;
    // mask tasks of the other WHERE contexts run with their OR group below
    if (tk_ctx_of(kv.first.first) != 0) continue;
    const int kind = tk_kind(kv.first.first);
    if (forked && kind == TK_DELTA_VAL && is_fork_col(kv.first.second))
      continue;  // ran on the side stream
    // value / gid tasks sort before the mask-writing kinds: the join sits
    // before the first of those
    if (kind == TK_DICT_MASK || kind == TK_BYTES_CONTAINS ||
        kind == TK_IS_NULL || kind == TK_IS_NOT_NULL)
      events.join_side(st);
    run_task(kv, part.d_mask);
  }
  // raw-byte utf8: device hash build assigns dense gids per hash-mode
  // group key (one shared table, rebuilt per column); string predicates
  // evaluate over the row strrefs
  if (plan->has_hash || plan->has_numkey) {
    // group keys, then the value columns of distinct aggs that are not keys
    std::vector<int> gid_cols = plan->group_cols;
    for (int ai : plan->distinct_aggs) {
      int ci = plan->aggs[ai].col_idx;
      if (std::find(gid_cols.begin(), gid_cols.end(), ci) == gid_cols.end())
        gid_cols.push_back(ci);
    }
    for (int ci : gid_cols) {
      auto& c = plan->cols[ci];
      if (!c.hash_mode && !c.numeric_key) continue;
      // +1 entry: the numeric-key overflow slot (gpuq_plan_load)
      reset_hash_table(part, st, (1ull << HASH_LOG2) + 1);
      auto itv = part.d_valid.find(ci);
      uint8_t* v = itv != part.d_valid.end() ? itv->second : nullptr;
      if (c.numeric_key) {
        int kf64 = (c.phys == PT_DOUBLE) ? 1 : 0;
        launch_numhash_build(st, part.d_val[ci], v, part.n_rows,
                             part.d_hkeys, part.d_hgids, HASH_LOG2,
                             part.d_hcount, part.d_gid2ref[ci], GID_CAP,
                             kf64, part.d_err);
        launch_numhash_lookup(st, part.d_val[ci], v, part.n_rows,
                              part.d_hkeys, part.d_hgids, HASH_LOG2, kf64,
                              part.d_gid[ci]);
      } else {
        launch_hash_build(st, part.d_dec, part.d_val[ci], v, part.n_rows,
                          part.d_hkeys, part.d_hgids, HASH_LOG2, part.d_hcount,
                          part.d_gid2ref[ci], GID_CAP, part.d_err);
        launch_hash_lookup(st, part.d_dec, part.d_val[ci], v, part.n_rows,
                           part.d_hkeys, part.d_hgids, HASH_LOG2,
                           part.d_gid[ci]);
      }
      part.hash_claimed[ci] = read_claimed(part, st);
    }
  }
  // string predicates of hash-mode columns and numeric comparisons of WHERE
  // context k, over whole decoded columns, into the context's buffer mk
  auto row_preds = [&](int k, uint8_t* mk) {
    for (size_t ci = 0; ci < plan->cols.size(); ci++) {
      auto& c = plan->cols[ci];
      if (!c.hash_mode || c.lut_preds.empty()) continue;
      for (int pidx : c.lut_preds) {
        if (plan->ctx_of(pidx) != k) continue;
        const auto& pp = plan->preds[pidx];
        int op = cmp_mode_of(pp.p.op);
        if (op < 0) op = cmp_str_like(like_mode(pp.p.op));  // LIKE family
        auto itv = part.d_valid.find((int)ci);
        launch_cmp_str(st, part.d_dec, part.d_val[(int)ci],
                       itv != part.d_valid.end() ? itv->second : nullptr,
                       part.d_needle + part.needle_off[pidx],
                       (uint32_t)pp.str_lit.size(), op, mk,
                       part.n_rows);
      }
    }

    // i64 comparisons on decoded arrays (the fork columns' ran on the side
    // stream)
    for (size_t ci = 0; ci < plan->cols.size(); ci++)
      if (!forked || !is_fork_col((int)ci)) cmp_col(st, (int)ci, k, mk);
  };
  // the side stream wrote d_mask (plain byte read-modify-writes): nothing on
  // the main stream touches it before the join
  events.join_side(st);
  row_preds(0, part.d_mask);

  // OR groups (WHERE tree): acc is set to 1 and the first term evaluates
  // straight into it; every later term evaluates into tmp (all ones on
  // entry) and k_mask_or_reset folds it in and re-arms tmp in one pass;
  // k_mask_and folds acc into the parent's buffer. A term that is an AND
  // group evaluates all its leaves into the one buffer; a nested OR recurses
  // with the pair of the next level. d_mask is final after this block.
  // Aggregate filters: each tree then evaluates the same way into a buffer
  // of its own (set to 1 first), reusing the level pairs — every tmp buffer
  // is all ones again when an OR group is done. A filter whose every leaf is
  // chunk-stats-proven everywhere passes no buffer at all.
  int where_combines = 0;
  std::vector<const uint8_t*> fbuf(plan->filters.size(), nullptr);
  if (plan->has_tree && (need_mask || !plan->filters.empty())) {
    for (size_t b = 1; b < part.d_wbufs.size(); b += 2)
      HIP_TRY(hipMemsetAsync(part.d_wbufs[b], 1, part.n_rows, st));
    std::function<void(int, uint8_t*)> eval_ors;
    auto eval_ctx = [&](int k, uint8_t* mk) {
      for (auto& kv : part.tasks)
        if (tk_ctx_of(kv.first.first) == k) run_task(kv, mk);
      row_preds(k, mk);
      eval_ors(k, mk);
    };
    eval_ors = [&](int k, uint8_t* mk) {
      for (int oi : plan->ctxs[k].ors) {
        const auto& wo = plan->wors[oi];
        uint8_t* acc = part.d_wbufs[2 * wo.level];
        uint8_t* tmp = part.d_wbufs[2 * wo.level + 1];
        HIP_TRY(hipMemsetAsync(acc, 1, part.n_rows, st));
        eval_ctx(wo.terms[0], acc);
        for (size_t t = 1; t < wo.terms.size(); t++) {
          eval_ctx(wo.terms[t], tmp);
          launch_mask_or_reset(st, acc, tmp, part.n_rows);
          where_combines++;
        }
        launch_mask_and(st, mk, acc, part.n_rows);
        where_combines++;
      }
    };
    if (need_mask) eval_ors(0, part.d_mask);
    for (size_t j = 0; j < plan->filters.size(); j++) {
      bool open = false;
      for (const auto& pr : part.pred_ranges)
        open |= plan->pred_filter[pr.first] == (int)j;
      if (!open) continue;
      HIP_TRY(hipMemsetAsync(part.d_fbufs[j], 1, part.n_rows, st));
      eval_ctx(plan->filters[j].ctx, part.d_fbufs[j]);
      fbuf[j] = part.d_fbufs[j];
    }
  }
  if (plan->has_tree && plan->exec_dbg)
    fprintf(stderr, "[gpuq exec] part %d: where bufs=%zu combines=%d\n", (int)pi,
            part.d_wbufs.size(), where_combines);

  // 2b. DATE_BIN key materialization
  for (size_t ci = 0; ci < plan->cols.size(); ci++) {
    auto& c = plan->cols[ci];
    if (!c.is_bin) continue;
    launch_bin_i64(st, part.d_val[c.bin_src], part.d_valid[c.bin_src],
                   c.bin_origin, c.bin_stride, c.bin_min_idx, c.nbins,
                   part.d_gid[(int)ci], part.n_rows);
  }

  // 2c. group sizing: with hash keys the cardinality is per-execute; if
  // the dense product space exceeds GID_CAP, combine keys exactly with the
  // pair cascade (two at a time, single-u64 CAS claims) and aggregate on
  // the dense combined gid — DataFusion's row-hash over arbitrary tuples.
  if (!plan->group_cols.empty()) {
    int64_t g2 = 1;
    for (int ci : plan->group_cols) {
      g2 *= key_card(ci);
      if (g2 > (int64_t)GID_CAP * 2) break;  // saturate
    }
    if (g2 > (int64_t)GID_CAP) {
      if (plan->group_cols.size() < 2 || !part.d_cgid)
        throw std::runtime_error("group-key cardinality exceeds the 2^22 cap");
      const int32_t* cur = part.d_gid[plan->group_cols[0]];
      for (size_t k = 1; k < plan->group_cols.size(); k++) {
        reset_hash_table(part, st, 1ull << HASH_LOG2);
        const int32_t* nxt = part.d_gid[plan->group_cols[k]];
        launch_pair_build(st, cur, nxt, part.n_rows, part.d_hkeys,
                          part.d_hgids, HASH_LOG2, part.d_hcount,
                          part.d_gid2pair[k - 1], GID_CAP, part.d_err);
        launch_pair_lookup(st, cur, nxt, part.n_rows, part.d_hkeys,
                           part.d_hgids, HASH_LOG2, part.d_cgid);
        level_claimed.push_back(read_claimed(part, st));
        cur = part.d_cgid;
      }
      cascaded = true;
      n_groups_exec = level_claimed.back();
    } else {
      n_groups_exec = g2;
    }
  }

  if (plan->is_projection)
    return execute_projection(plan, part, events, t0, need_mask, out);

  // 3. aggregate
  AggArgs a{};
  a.mask = part.d_mask;
  a.n_rows = part.n_rows;
  if (cascaded) {
    // the cascade already produced a dense combined gid per row
    a.n_keys = 1;
    a.key_gid[0] = part.d_cgid;
    a.key_size[0] = (int32_t)n_groups_exec;
  } else {
    a.n_keys = (int)plan->group_cols.size();
    for (int k = 0; k < a.n_keys; k++) {
      int ci = plan->group_cols[k];
      a.key_gid[k] = part.d_gid[ci];
      a.key_size[k] = (int32_t)key_card(ci);
    }
  }
  a.n_aggs = (int)plan->aggs.size();
  for (int i = 0; i < a.n_aggs; i++) {
    const auto& ap = plan->aggs[i];
    a.agg_kind[i] = ap.kind;
    a.cnt_skip[i] = ap.cnt_is_presence ? 1 : 0;
    a.agg_filter[i] = ap.filter >= 0 ? fbuf[ap.filter] : nullptr;
    a.fsum_idx[i] = ap.fsum_idx;
    if (ap.col_idx >= 0) {
      auto itv = part.d_val.find(ap.col_idx);
      a.agg_val[i] = itv != part.d_val.end() ? itv->second : nullptr;
      // null-free column (footer-proven): skip the validity read entirely
      auto itd = part.d_valid.find(ap.col_idx);
      a.agg_valid[i] = (ap.cnt_is_presence || itd == part.d_valid.end())
                           ? nullptr : itd->second;
    }
  }
  a.mask = need_mask ? part.d_mask : nullptr;
  a.fsum_n = plan->n_fsum;
  a.fsum = part.d_fsum;
  a.err = part.d_err;
  a.dec = part.d_dec;
  a.table = part.d_table;
  a.n_groups = (int32_t)n_groups_exec;
  launch_init_table(st, part.d_table, (int32_t)n_groups_exec,
                    (int)plan->aggs.size(), part.d_agg_kind);
  if (plan->n_fsum)
    HIP_TRY(hipMemsetAsync(part.d_fsum, 0,
                           (size_t)plan->n_fsum * n_groups_exec * 4 * 8, st));
  // masks and key gids are final here: the fused kernel decodes the value
  // column straight into the table, unless a hash/numeric key produced more
  // groups than its LDS table holds — then the column is materialised now
  // and the old kernels run
  bool fused = plan->fused_valagg && n_groups_exec * 16 <= 64 * 1024;
  if (plan->fused_valagg && plan->exec_dbg)
    fprintf(stderr,
            "[gpuq exec] part %d: valagg=%s n_groups=%lld dict_walk=%s\n", pi,
            fused ? "fused" : "fallback", (long long)n_groups_exec,
            dw ? "serial" : "scan");
  if (fused) {
    launch_val_agg(st, part.d_dec, part.d_pages, part.d_valagg_ids,
                   (int)part.valagg_ids.size(), part.d_dictv, a.key_gid[0],
                   a.mask, part.d_table, (int32_t)n_groups_exec, a.n_aggs,
                   plan->aggs[1].kind, plan->valagg_blocks, dw, part.d_err);
  } else {
    if (plan->fused_valagg)
      for (auto& kv : part.tasks)
        if (kv.first.second == plan->valagg_col) run_task(kv, part.d_mask);
    const char* agg_path = launch_agg(st, a, plan->no_fcount);
    if (plan->exec_dbg && !plan->filters.empty()) {
      int live = 0;
      for (auto* fb : fbuf) live += fb != nullptr;
      fprintf(stderr,
              "[gpuq exec] part %d: agg=%s filters=%zu filter_bufs=%d "
              "n_groups=%lld table_bytes=%lld\n",
              pi, agg_path, plan->filters.size(), live,
              (long long)n_groups_exec,
              (long long)((n_groups_exec * (1 + 2 * a.n_aggs) +
                           (int64_t)a.fsum_n * n_groups_exec * 4) * 8));
    }
  }
  // 3b. COUNT(DISTINCT): one set pass per distinct agg over the same final
  // masks and group index; the shared table is free again (cascade done)
  for (size_t di = 0; di < plan->distinct_aggs.size(); di++) {
    const int ci = plan->aggs[plan->distinct_aggs[di]].col_idx;
    DistinctArgs d{};
    d.mask = a.mask;
    d.n_rows = part.n_rows;
    d.n_keys = a.n_keys;
    for (int k = 0; k < a.n_keys; k++) {
      d.key_gid[k] = a.key_gid[k];
      d.key_size[k] = a.key_size[k];
    }
    d.n_groups = (int32_t)n_groups_exec;
    d.vgid = part.d_gid[ci];
    {
      const int fj = plan->aggs[plan->distinct_aggs[di]].filter;
      d.filter = fj >= 0 ? fbuf[fj] : nullptr;
    }
    d.vcard = (int32_t)key_card(ci);
    d.pairs = part.d_dpairs[di];
    d.count = part.d_dcount + di;
    d.pair_cap = plan->distinct_pair_cap;
    d.err = part.d_err;
    const uint64_t vpad = ((uint64_t)d.vcard + 63) & ~63ull;
    const uint64_t bits = (uint64_t)n_groups_exec * vpad;
    if (!plan->distinct_force_hash && part.d_dbitmap &&
        bits <= plan->distinct_bitmap_bits)
      distinct_bitmap[di] = bits <= plan->distinct_lds_bits ? 2 : 1;
    HIP_TRY(hipMemsetAsync(d.count, 0, 4, st));
    if (distinct_bitmap[di]) {
      HIP_TRY(hipMemsetAsync(part.d_dbitmap, 0, bits / 8, st));
      launch_distinct_bitmap(st, d, part.d_dbitmap, (uint32_t)vpad,
                             distinct_bitmap[di] == 2);
    } else {
      HIP_TRY(hipMemsetAsync(part.d_hkeys, 0xFF, (1ull << HASH_LOG2) * 8, st));
      launch_distinct_claim(st, d, part.d_hkeys, HASH_LOG2);
    }
  }
  HIP_TRY(hipEventRecord(ev1, st));
  }  // !fused_count

  // 4. D2H results
  size_t tsz = (size_t)n_groups_exec * (1 + 2 * plan->aggs.size());
  std::vector<uint64_t> table(tsz);
  HIP_TRY(hipMemcpyAsync(table.data(), part.d_table, tsz * 8,
                         hipMemcpyDeviceToHost, st));
  std::vector<uint64_t> fsums((size_t)plan->n_fsum * n_groups_exec * 4);
  if (!fsums.empty())
    HIP_TRY(hipMemcpyAsync(fsums.data(), part.d_fsum, fsums.size() * 8,
                           hipMemcpyDeviceToHost, st));
  int32_t herr = 0;
  HIP_TRY(hipMemcpyAsync(&herr, part.d_err, 4, hipMemcpyDeviceToHost, st));
  const size_t n_distinct = plan->distinct_aggs.size();
  std::vector<uint32_t> dcounts(n_distinct, 0);
  if (n_distinct)
    HIP_TRY(hipMemcpyAsync(dcounts.data(), part.d_dcount, n_distinct * 4,
                           hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (herr == ERR_DISTINCT_CAP)
    throw std::runtime_error(
        "count_distinct: more than " + std::to_string(plan->distinct_pair_cap) +
        " distinct (group, value) pairs in one partition (the pair cap, "
        "GPUQ_DISTINCT_PAIR_CAP) — kernel error code " + std::to_string(herr));
  if (herr == ERR_DISTINCT_PROBE)
    throw std::runtime_error(
        "count_distinct: hash-set probe exhausted — kernel error code " +
        std::to_string(herr));
  if (herr != 0)
    throw std::runtime_error("kernel error code " + std::to_string(herr));
  // the claimed (g << 32 | vgid) lists, sorted: group order == live order
  std::vector<std::vector<uint64_t>> dpairs(n_distinct);
  for (size_t di = 0; di < n_distinct; di++) {
    if (dcounts[di] > plan->distinct_pair_cap)
      throw std::runtime_error("count_distinct: pair count beyond the cap");
    dpairs[di].resize(dcounts[di]);
    if (dcounts[di])
      HIP_TRY(hipMemcpy(dpairs[di].data(), part.d_dpairs[di],
                        (size_t)dcounts[di] * 8, hipMemcpyDeviceToHost));
    std::sort(dpairs[di].begin(), dpairs[di].end());
    if (plan->exec_dbg) {
      const int ai = plan->distinct_aggs[di];
      const int ci = plan->aggs[ai].col_idx;
      fprintf(stderr,
              "[gpuq exec] part %d: distinct agg=%d col=%s path=%s groups=%lld "
              "card=%lld pairs=%u%s\n",
              pi, ai, plan->cols[ci].name.c_str(),
              distinct_bitmap[di] ? "bitmap" : "hash",
              (long long)n_groups_exec, (long long)key_card(ci) - 1,
              dcounts[di],
              distinct_bitmap[di] == 2   ? " mark=lds"
              : distinct_bitmap[di] == 1 ? " mark=global" : "");
    }
  }
  hot_tier_populate(plan, part, st);

  float ms_total = 0, ms_decomp = 0;
  HIP_TRY(hipEventElapsedTime(&ms_total, ev0, ev1));
  HIP_TRY(hipEventElapsedTime(&ms_decomp, ev0, ev_decomp));

  // 5. assemble the PARTIAL aggregate batch
  int n_keys = (int)plan->group_cols.size();
  int n_aggs = (int)plan->aggs.size();
  int slots = 1 + 2 * n_aggs;
  std::vector<int64_t> live;  // group ids with presence > 0
  for (int64_t g = 0; g < n_groups_exec; g++)
    if (table[(size_t)g * slots]) live.push_back(g);
  int64_t nr = (int64_t)live.size();
  // no-group aggregate over empty selection: emit the single empty row
  bool empty_aggregate_row = (n_keys == 0 && nr == 0);
  if (empty_aggregate_row) { live.push_back(0); nr = 1; }

  // owned here until `out` takes it: a throw below frees the schema and the
  // batch built so far through the stream's own release path
  std::unique_ptr<StreamState, void (*)(StreamState*)> ss(new StreamState(),
                                                          stream_state_free);
  memset(&ss->schema, 0, sizeof(ss->schema));
  memset(&ss->batch, 0, sizeof(ss->batch));
  ss->schema.format = strdup("+s");
  ss->schema.name = strdup("");
  ss->schema.release = release_schema;
  // fixed positional layout, then one agg{i}_set list per distinct agg
  int n_fields = n_keys + 1 + 2 * n_aggs + (int)n_distinct;
  auto distinct_fmt = [&](int ai) {
    const auto& c = plan->cols[plan->aggs[ai].col_idx];
    return c.phys == PT_BYTE_ARRAY ? "u" : c.phys == PT_DOUBLE ? "g" : "l";
  };
  ss->schema.n_children = n_fields;
  ss->schema.children = (struct ArrowSchema**)calloc(n_fields, sizeof(void*));
  int f = 0;
  for (int k = 0; k < n_keys; k++) {
    ss->schema.children[f] = (struct ArrowSchema*)malloc(sizeof(struct ArrowSchema));
    const auto& kc = plan->cols[plan->group_cols[k]];
    make_schema_field(ss->schema.children[f],
                      (kc.numeric_key && kc.phys == PT_DOUBLE) ? "g"
                      : (kc.is_bin || kc.numeric_key) ? "l" : "u",
                      kc.is_bin ? "date_bin" : kc.name.c_str());
    f++;
  }
  ss->schema.children[f] = (struct ArrowSchema*)malloc(sizeof(struct ArrowSchema));
  make_schema_field(ss->schema.children[f], "l", "__presence");
  f++;
  for (int i = 0; i < n_aggs; i++) {
    ss->schema.children[f] = (struct ArrowSchema*)malloc(sizeof(struct ArrowSchema));
    int ki = plan->aggs[i].kind;
    const char* fmt = (ki == AGGK_SUM_F64 || ki == AGGK_MIN_F64 || ki == AGGK_MAX_F64)
                          ? "g"
                      : (ki == AGGK_MIN_RANK || ki == AGGK_MAX_RANK ||
                         ki == AGGK_MIN_STR || ki == AGGK_MAX_STR) ? "u" : "l";
    make_schema_field(ss->schema.children[f], fmt, "agg" + std::to_string(i));
    f++;
    ss->schema.children[f] = (struct ArrowSchema*)malloc(sizeof(struct ArrowSchema));
    make_schema_field(ss->schema.children[f], "l", "agg" + std::to_string(i) + "_count");
    f++;
  }
  for (int ai : plan->distinct_aggs) {
    auto* ls = (struct ArrowSchema*)malloc(sizeof(struct ArrowSchema));
    ss->schema.children[f++] = ls;
    make_schema_field(ls, "+l", "agg" + std::to_string(ai) + "_set");
    ls->n_children = 1;
    ls->children = (struct ArrowSchema**)calloc(1, sizeof(void*));
    ls->children[0] = (struct ArrowSchema*)malloc(sizeof(struct ArrowSchema));
    make_schema_field(ls->children[0], distinct_fmt(ai), "item");
  }

  ss->batch.length = nr;
  ss->batch.n_buffers = 1;
  ss->batch.buffers = (const void**)calloc(1, sizeof(void*));
  ss->batch.n_children = n_fields;
  ss->batch.children = (struct ArrowArray**)calloc(n_fields, sizeof(void*));
  ss->batch.release = release_array;
  auto* eb = new ExportedBatch();  // the batch owns it from the next line on
  ss->batch.private_data = eb;

  auto make_child = [&](int idx) {
    auto* ch = (struct ArrowArray*)calloc(1, sizeof(struct ArrowArray));
    ss->batch.children[idx] = ch;
    ch->length = nr;
    ch->release = release_array;
    return ch;
  };
  // non-null count of aggregate i in the group whose table row starts at base
  auto row_count = [&](size_t base, int i) -> uint64_t {
    const auto& ap = plan->aggs[i];
    return empty_aggregate_row
               ? 0 : agg_count(table, base, i, ap.kind, ap.cnt_is_presence);
  };

  // decode combined gid -> per-key local gids
  std::vector<std::vector<int32_t>> key_gids(n_keys, std::vector<int32_t>(nr));
  if (cascaded) {
    // unwind the pair cascade: level maps are (prev_combined << 32) | gid_k
    std::vector<std::vector<uint64_t>> pair_maps(level_claimed.size());
    for (size_t L = 0; L < level_claimed.size(); L++) {
      pair_maps[L].resize(level_claimed[L]);
      if (level_claimed[L])
        HIP_TRY(hipMemcpy(pair_maps[L].data(), part.d_gid2pair[L],
                          (size_t)level_claimed[L] * 8,
                          hipMemcpyDeviceToHost));
    }
    for (int64_t r = 0; r < nr; r++) {
      int64_t g = live[r];
      for (int k = n_keys - 1; k >= 1; k--) {
        uint64_t pr = pair_maps[(size_t)k - 1][(size_t)g];
        key_gids[k][r] = (int32_t)(uint32_t)pr;
        g = (int64_t)(pr >> 32);
      }
      key_gids[0][r] = (int32_t)g;
    }
  } else
  for (int64_t r = 0; r < nr; r++) {
    int64_t g = live[r];
    for (int k = n_keys - 1; k >= 0; k--) {
      int32_t sz = (int32_t)key_card(plan->group_cols[k]);
      key_gids[k][r] = (int32_t)(g % sz);
      g /= sz;
    }
  }
  // hash-mode key columns: fetch the strings for the local gids that
  // actually appear (gid -> gid2ref -> dec-arena bytes)
  std::map<int, std::unordered_map<int32_t, std::string>> hash_names;
  std::map<int, std::vector<uint64_t>> num_keys;  // numeric key: gid -> value
  for (int k = 0; k < n_keys; k++) {
    int ci = plan->group_cols[k];
    const auto& kc = plan->cols[ci];
    if (kc.numeric_key) {
      uint32_t claimed = part.hash_claimed[ci];
      auto& g2k = num_keys[ci];
      g2k.resize(claimed);
      if (claimed)
        HIP_TRY(hipMemcpy(g2k.data(), part.d_gid2ref[ci],
                          (size_t)claimed * 8, hipMemcpyDeviceToHost));
      continue;
    }
    if (!kc.hash_mode) continue;
    std::vector<int32_t> need;
    {
      std::unordered_map<int32_t, char> seen;
      for (int64_t r = 0; r < nr; r++) {
        int32_t gid = key_gids[k][r];
        if (gid > 0 && !seen.count(gid)) { seen[gid] = 1; need.push_back(gid); }
      }
    }
    uint32_t claimed = part.hash_claimed[ci];
    std::vector<uint64_t> g2r(claimed);
    if (claimed)
      HIP_TRY(hipMemcpy(g2r.data(), part.d_gid2ref[ci], (size_t)claimed * 8,
                        hipMemcpyDeviceToHost));
    std::vector<uint64_t> refs;
    refs.reserve(need.size());
    for (int32_t gid : need) refs.push_back(g2r[(size_t)gid - 1]);
    auto strs = fetch_ref_strings(part, st, refs);
    auto& m = hash_names[ci];
    for (size_t i2 = 0; i2 < need.size(); i2++) m[need[i2]] = std::move(strs[i2]);
  }
  f = 0;
  // keys: bin start timestamps (ms), numeric key values from the claim
  // table, utf8 from the global dictionary or (hash mode) the dec arena;
  // the NULL group is gid 0
  for (int k = 0; k < n_keys; k++) {
    auto* ch = make_child(f++);
    auto& c = plan->cols[plan->group_cols[k]];
    const auto& gids = key_gids[k];
    if (c.is_bin || c.numeric_key) {
      const auto& g2k = num_keys[plan->group_cols[k]];
      std::vector<int64_t> v(nr, 0);
      std::vector<uint8_t> valid(nr, 0);
      for (int64_t r = 0; r < nr; r++) {
        const int32_t gid = gids[r];
        if (gid <= 0) continue;
        valid[r] = 1;
        v[r] = c.is_bin
                   ? c.bin_origin + (c.bin_min_idx + gid - 1) * c.bin_stride
                   : (int64_t)g2k[(size_t)gid - 1];
      }
      set_i64_column(*eb, ch, v, &valid);
      continue;
    }
    std::vector<const std::string*> strs(nr, nullptr);
    for (int64_t r = 0; r < nr; r++)
      if (gids[r] > 0)
        strs[r] = c.hash_mode ? &hash_names[plan->group_cols[k]][gids[r]]
                              : &c.gdict[gids[r] - 1];
    set_utf8_column(*eb, ch, strs);
  }
  // presence
  int64_t rows_out_total = 0;
  {
    std::vector<int64_t> v(nr);
    for (int64_t r = 0; r < nr; r++) {
      v[r] = empty_aggregate_row ? 0 : (int64_t)table[(size_t)live[r] * slots];
      rows_out_total += v[r];
    }
    set_i64_column(*eb, make_child(f++), v);
  }
  // distinct aggs: row r owns the sorted pairs [doffs[r], doffs[r + 1]) —
  // list offsets and, by difference, the partition-local distinct counts
  std::vector<std::vector<int32_t>> doffs(n_distinct);
  for (size_t di = 0; di < n_distinct; di++) {
    const auto& pr = dpairs[di];
    auto& off = doffs[di];
    off.assign((size_t)nr + 1, 0);
    size_t p = 0;
    for (int64_t r = 0; r < nr; r++) {
      off[r] = (int32_t)p;
      while (p < pr.size() && (int64_t)(pr[p] >> 32) == live[r]) p++;
    }
    off[nr] = (int32_t)p;
    if (p != pr.size())
      throw std::runtime_error("count_distinct: pair outside the live groups");
  }
  // aggs: agg{i} then agg{i}_count
  std::vector<int64_t> cnt(nr);
  for (int i = 0; i < n_aggs; i++) {
    auto* chv = make_child(f++);
    const auto& ap = plan->aggs[i];
    const int kind = ap.kind;
    if (kind == AGGK_COUNT_DISTINCT) {
      // both columns carry the partition-local distinct count
      size_t di = std::find(plan->distinct_aggs.begin(),
                            plan->distinct_aggs.end(), i) -
                  plan->distinct_aggs.begin();
      for (int64_t r = 0; r < nr; r++)
        cnt[r] = doffs[di][r + 1] - doffs[di][r];
      set_i64_column(*eb, chv, cnt);
      set_i64_column(*eb, make_child(f++), cnt);
      continue;
    }
    for (int64_t r = 0; r < nr; r++)
      cnt[r] = (int64_t)row_count((size_t)live[r] * slots, i);
    if (kind == AGGK_MIN_STR || kind == AGGK_MAX_STR) {
      // hash-mode utf8 min/max: strref -> dec-arena bytes
      std::vector<uint64_t> refs;
      std::vector<int64_t> ref_rows;
      for (int64_t r = 0; r < nr; r++) {
        uint64_t ref = table[(size_t)live[r] * slots + 1 + 2 * i];
        if (cnt[r] && ref != ~0ull) { refs.push_back(ref); ref_rows.push_back(r); }
      }
      auto ref_strs = fetch_ref_strings(part, st, refs);
      std::vector<const std::string*> strs(nr, nullptr);
      for (size_t j = 0; j < ref_rows.size(); j++)
        strs[ref_rows[j]] = &ref_strs[j];
      set_utf8_column(*eb, chv, strs);
    } else if (kind == AGGK_MIN_RANK || kind == AGGK_MAX_RANK) {
      // dict utf8 min/max: rank -> dictionary string
      const auto& c = plan->cols[ap.col_idx];
      std::vector<const std::string*> strs(nr, nullptr);
      for (int64_t r = 0; r < nr; r++) {
        if (!cnt[r]) continue;
        int64_t rankv = (int64_t)table[(size_t)live[r] * slots + 1 + 2 * i];
        if (rankv >= 0 && rankv < (int64_t)c.rank_to_gid.size())
          strs[r] = &c.gdict[(size_t)c.rank_to_gid[(size_t)rankv] - 1];
      }
      set_utf8_column(*eb, chv, strs);
    } else {
      std::vector<int64_t> vv(nr, 0);
      std::vector<uint8_t> valid(nr, 1);
      for (int64_t r = 0; r < nr; r++) {
        if (kind == AGGK_COUNT_STAR || kind == AGGK_COUNT) {
          vv[r] = cnt[r];
        } else if (cnt[r] == 0) {
          valid[r] = 0;
        } else if (kind == AGGK_SUM_F64) {
          // exact 256-bit superaccumulator, rounded once (acc256_to_double)
          double d = acc256_to_double(
              &fsums[((size_t)ap.fsum_idx * n_groups_exec +
                      (size_t)live[r]) * 4]);
          memcpy(&vv[r], &d, 8);
        } else {
          vv[r] = (int64_t)table[(size_t)live[r] * slots + 1 + 2 * i];
        }
      }
      set_i64_column(*eb, chv, vv, &valid);
    }
    set_i64_column(*eb, make_child(f++), cnt);
  }
  // agg{i}_set: the partial state of a distinct agg — per row the list of
  // its distinct values, vgid resolved through the global dictionary (dict
  // utf8), gid2ref + the dec arena (hash-mode utf8) or gid2ref (numeric)
  for (size_t di = 0; di < n_distinct; di++) {
    const int ci = plan->aggs[plan->distinct_aggs[di]].col_idx;
    const auto& c = plan->cols[ci];
    const auto& pr = dpairs[di];
    const int64_t np = (int64_t)pr.size();
    auto* chl = make_child(f++);
    set_list_offsets(*eb, chl, doffs[di]);
    chl->n_children = 1;
    chl->children = (struct ArrowArray**)calloc(1, sizeof(void*));
    auto* item = (struct ArrowArray*)calloc(1, sizeof(struct ArrowArray));
    chl->children[0] = item;
    item->length = np;
    item->release = release_array;
    std::vector<uint64_t> g2r;  // gid - 1 -> strref / value bits
    if (c.hash_mode || c.numeric_key) {
      g2r.resize(part.hash_claimed[ci]);
      if (!g2r.empty())
        HIP_TRY(hipMemcpy(g2r.data(), part.d_gid2ref[ci], g2r.size() * 8,
                          hipMemcpyDeviceToHost));
    }
    auto vgid_of = [&](int64_t p) { return (size_t)(uint32_t)pr[(size_t)p]; };
    if (c.numeric_key) {
      std::vector<int64_t> v((size_t)np);
      for (int64_t p = 0; p < np; p++) v[p] = (int64_t)g2r.at(vgid_of(p) - 1);
      set_i64_column(*eb, item, v);
      continue;
    }
    std::vector<std::string> ref_strs;
    if (c.hash_mode) {
      std::vector<uint64_t> refs((size_t)np);
      for (int64_t p = 0; p < np; p++) refs[(size_t)p] = g2r.at(vgid_of(p) - 1);
      ref_strs = fetch_ref_strings(part, st, refs);
    }
    std::vector<const std::string*> strs((size_t)np);
    size_t total = 0;
    for (int64_t p = 0; p < np; p++) {
      strs[p] = c.hash_mode ? &ref_strs[(size_t)p]
                            : &c.gdict.at(vgid_of(p) - 1);
      total += strs[p]->size();
    }
    if (total > (size_t)INT32_MAX)
      throw std::runtime_error("count_distinct: set column beyond 2 GiB");
    set_utf8_column(*eb, item, strs);
  }

  memset(out, 0, sizeof(*out));
  out->get_schema = ss_get_schema;
  out->get_next = ss_get_next;
  out->get_last_error = ss_get_last_error;
  out->release = ss_release;
  out->private_data = ss.release();

  {
    std::lock_guard<std::mutex> g(plan->mu);
    plan->m_kernel_ns += (int64_t)(ms_total * 1e6);
    plan->m_decomp_ns += (int64_t)(ms_decomp * 1e6);
    plan->m_exec_ns += now_ns() - t0;
    plan->m_rows_out += rows_out_total;
  }
  return 0;
} catch (const std::exception& e) {
  if (plan && plan->ctx) plan->ctx->set_error(e.what());
  return -1;
}

extern "C" int32_t gpuq_plan_metrics(gpuq_plan* p, gpuq_metrics* out) {
  if (!p || !out) return -1;
  std::lock_guard<std::mutex> g(p->mu);
  memset(out, 0, sizeof(*out));
  out->rows_scanned = p->m_rows_scanned;
  out->rows_out = p->m_rows_out;
  for (auto& part : p->parts) {
    out->bytes_scanned += part.bytes_scanned;
    out->rowgroup_bytes_total += part.rowgroup_bytes_total;
    out->hbm_bytes_est += (int64_t)(part.raw_bytes + 2 * part.dec_bytes);
    out->cache_hit_bytes += part.bytes_cache_hit;
  }
  out->kernel_ns = p->m_kernel_ns;
  out->exec_ns = p->m_exec_ns;
  out->load_ns = p->m_load_ns;
  out->decomp_ns = p->m_decomp_ns;
  return 0;
}

gpuq_plan::~gpuq_plan() {
  if (ctx)
    for (auto& k : pinned_keys) ctx->cache_unpin(k);
  for (auto& part : parts) {
    if (!part.loaded) continue;
    (void)hipSetDevice(part.device);
    auto F = [](void* p) { if (p) (void)hipFree(p); };
    F(part.d_raw); F(part.d_dec); F(part.d_pages); F(part.d_remap);
    F(part.d_dictv); F(part.d_lut); F(part.d_mask); F(part.d_err);
    for (auto* wb : part.d_wbufs) F(wb);
    for (auto* fb : part.d_fbufs) F(fb);
    F(part.d_table); F(part.d_fsum); F(part.d_agg_kind);
    F(part.d_hkeys); F(part.d_hgids); F(part.d_hcount); F(part.d_cgid);
    for (auto& kv : part.d_gid2ref) F(kv.second);
    for (auto* ptr : part.d_gid2pair) F(ptr); F(part.d_needle); F(part.d_all_ids);
    F(part.d_rowof); F(part.d_rank); F(part.d_scr);
    F(part.d_present); F(part.d_tmpvalid);
    F(part.d_seqs); F(part.d_tiles); F(part.d_lits_wave);
    F(part.d_cwins); F(part.d_cstarts);
    F(part.d_segs); F(part.d_brs); F(part.d_pagebrs);
    F(part.d_res_lane); F(part.d_res_wave); F(part.d_piece_pool);
    F(part.d_keys); F(part.d_keys_sorted); F(part.d_rows);
    F(part.d_rows_sorted); F(part.d_count); F(part.d_sort_temp);
    for (auto& kv : part.d_ids) F(kv.second);
    F(part.d_valagg_ids);
    F(part.d_dbitmap); F(part.d_dcount);
    for (auto* ptr : part.d_dpairs) F(ptr);
    for (auto& kv : part.d_gid) F(kv.second);
    for (auto& kv : part.d_val) F(kv.second);
    for (auto& kv : part.d_valid) F(kv.second);
    const DecompDev& E = part.d_early;
    for (const void* ptr : {(const void*)E.d_segs, (const void*)E.d_seqs,
                            (const void*)E.d_tiles, (const void*)E.d_lits_wave,
                            (const void*)E.d_res_lane, (const void*)E.d_res_wave,
                            (const void*)E.d_piece_pool, (const void*)E.d_brs,
                            (const void*)E.d_pagebrs})
      F(const_cast<void*>(ptr));
    if (part.side) (void)hipStreamDestroy(part.side);
    if (part.stream) (void)hipStreamDestroy(part.stream);
  }
}

extern "C" void gpuq_plan_destroy(gpuq_plan* p) { delete p; }

// ------------------------------------------------------------------
// test support: decompress caller-supplied blocks (include/gpuq.h)
// ------------------------------------------------------------------
namespace {

constexpr uint64_t DEC_PAD = 16384 + 64;  // plan build's over-read pad
constexpr uint64_t RAW_SLACK = 8192;      // gpuq_plan_load's d_raw slack

// serial host replay of the planned records over a host arena, one loop per
// kernel, in launch order. Deferred-match gaps in a segment are left alone
// (the kernel flushes arbitrary LDS bytes there), so an unresolved gap
// keeps the caller's sentinel.
void replay_decompress(const uint8_t* raw, uint8_t* dec, const DecompRecs& R) {
  for (const DevSeg& sg : R.segs) {
    const uint8_t* src = raw + sg.src_off;
    uint8_t* dst = dec + sg.dst_off;
    if (sg.raw) {
      std::memcpy(dst, src, sg.out_len);
      continue;
    }
    uint32_t s = 0, d = 0;
    while (s < sg.comp_len && d < sg.out_len) {
      uint32_t token = src[s++];
      uint32_t lit = token >> 4;
      if (lit == 15) {
        uint32_t b;
        do { b = src[s++]; lit += b; } while (b == 255);
      }
      if (s + lit > sg.comp_len || d + lit > sg.out_len)
        throw std::runtime_error("replay: segment literal overrun");
      std::memcpy(dst + d, src + s, lit);
      s += lit;
      d += lit;
      if (s >= sg.comp_len) break;
      uint32_t off = src[s] | ((uint32_t)src[s + 1] << 8);
      s += 2;
      uint32_t ml = token & 0xf;
      if (ml == 15) {
        uint32_t b;
        do { b = src[s++]; ml += b; } while (b == 255);
      }
      ml += 4;
      if (d + ml > sg.out_len)
        throw std::runtime_error("replay: segment match overrun");
      if (!sg.big && off <= d)
        for (uint32_t i = 0; i < ml; i++) dst[d + i] = dst[d + i - off];
      d += ml;
    }
    if (d != sg.out_len) throw std::runtime_error("replay: segment size mismatch");
  }
  // tiles: a record's offset is the prefix sum of the lengths before it
  for (const DevSeqTile& t : R.tiles) {
    uint8_t* o = dec + t.dst0;
    for (uint32_t k = 0; k < t.n_rec; k++) {
      const DevSeq& r = R.seqs[t.rec0 + k];
      const uint32_t lit = (uint32_t)(r.a >> 40) & 0x1ff;
      const uint32_t ml = (uint32_t)(r.a >> 49) & 0x1ff;
      const uint32_t period = (uint32_t)(r.a >> 58);
      std::memcpy(o, raw + (r.a & ((1ull << 40) - 1)), lit);
      o += lit;
      for (uint32_t j = 0; j < ml; j++)
        o[j] = (uint8_t)(r.pat >> ((j % period) * 8));
      o += ml;
    }
  }
  for (const DevLit& L : R.lits_wave)
    std::memcpy(dec + L.b, raw + (L.a & ((1ull << 40) - 1)), L.a >> 40);
  for (const auto* recs : {&R.res_lane, &R.res_wave})
    for (const DevBrRes& rec : *recs) {
      uint32_t pat_off = 0;
      for (uint32_t k = 0; k < rec.piece_n; k++) {
        const DevPiece& pc = R.piece_pool[rec.piece_start + k];
        for (uint32_t base = pat_off; base < rec.len; base += rec.off) {
          uint32_t m = std::min(pc.len, rec.len - base);
          for (uint32_t j = 0; j < m; j++)
            dec[rec.dst + base + j] = dec[pc.src + j];
        }
        pat_off += pc.len;
      }
    }
  for (const DevPageBr& pb : R.pagebrs)
    for (uint32_t r = 0; r < pb.count; r++) {
      const DevBr& br = R.brs[pb.start + r];
      for (uint32_t i = 0; i < br.len; i++) dec[br.dst + i] = dec[br.src + i];
    }
}

// every record must stay inside the raw buffer / the image part of the
// arena before anything is launched
void check_decomp_bounds(const DecompRecs& R, uint64_t raw_len,
                         uint64_t img_len) {
  auto need = [](bool ok) {
    if (!ok) throw std::runtime_error("decompress record out of bounds");
  };
  for (const DevSeg& s : R.segs)
    need(s.src_off + s.comp_len <= raw_len && s.dst_off + s.out_len <= img_len);
  for (const DevLit& L : R.lits_wave)
    need((L.a & ((1ull << 40) - 1)) + (L.a >> 40) <= raw_len &&
         L.b + (L.a >> 40) <= img_len);
  for (const DevSeqTile& t : R.tiles) {
    need(t.n_rec >= 1 && t.n_rec <= SEQ_TILE_RECS &&
         t.out_len <= SEQ_TILE_BYTES && t.rec0 + t.n_rec <= R.seqs.size() &&
         t.dst0 + t.out_len <= img_len);
    uint64_t sum = 0;
    for (uint32_t k = 0; k < t.n_rec; k++) {
      const DevSeq& r = R.seqs[t.rec0 + k];
      const uint64_t lit = (r.a >> 40) & 0x1ff, ml = (r.a >> 49) & 0x1ff;
      const uint64_t period = r.a >> 58;
      need(lit <= 256 && ml <= 256 &&
           (r.a & ((1ull << 40) - 1)) + lit <= raw_len &&
           (ml == 0 || (period >= 1 && period <= 8)));
      sum += lit + ml;
    }
    need(sum == t.out_len);
  }
  for (const auto* recs : {&R.res_lane, &R.res_wave})
    for (const DevBrRes& r : *recs) {
      need(r.off >= 1 && r.dst + r.len <= img_len &&
           (uint64_t)r.piece_start + r.piece_n <= R.piece_pool.size());
      for (uint32_t k = 0; k < r.piece_n; k++) {
        const DevPiece& pc = R.piece_pool[r.piece_start + k];
        need(pc.src + pc.len <= img_len);
      }
    }
  for (const DevPageBr& pb : R.pagebrs) {
    need((uint64_t)pb.start + pb.count <= R.brs.size());
    for (uint32_t r = 0; r < pb.count; r++) {
      const DevBr& br = R.brs[pb.start + r];
      need(br.src < br.dst && br.dst + br.len <= img_len);
    }
  }
  for (const auto& h : R.himgs) need(h.first + h.second.size() <= img_len);
}

struct DevBufs {
  std::vector<void*> ptrs;
  hipStream_t stream = nullptr;
  template <class T> T* alloc(size_t bytes) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, std::max<size_t>(bytes, 16)));
    ptrs.push_back(p);
    return (T*)p;
  }
  template <class T> T* upload(const std::vector<T>& v) {
    T* d = alloc<T>(v.size() * sizeof(T));
    if (!v.empty())
      HIP_TRY(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T),
                             hipMemcpyHostToDevice, stream));
    return d;
  }
  ~DevBufs() {
    for (void* p : ptrs) (void)hipFree(p);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

}  // namespace

extern "C" int32_t gpuq_test_decompress(
    gpuq_ctx* ctx, const gpuq_decomp_page* pages, int32_t n_pages,
    int32_t raw_lead, int32_t mode, uint8_t sentinel, uint8_t* out,
    uint64_t out_cap, uint64_t* arena_len, uint64_t* guard_len,
    gpuq_decomp_stats* stats, int32_t* d_err) try {
  const int pmode = mode & 0xff;
  const bool host_only = mode & (GPUQ_DECOMP_HOST_ONLY | GPUQ_DECOMP_HOST_REPLAY);
  const bool replay = mode & GPUQ_DECOMP_HOST_REPLAY;
  if (!pages || n_pages < 0 || raw_lead < 0 || raw_lead > 15 || !out ||
      !stats || pmode > GPUQ_DECOMP_FORCE_FALLBACK ||
      (mode & ~(0xff | GPUQ_DECOMP_HOST_ONLY | GPUQ_DECOMP_HOST_REPLAY)))
    throw std::runtime_error("gpuq_test_decompress: bad argument");
  if (!host_only && (!ctx || ctx->devices.empty()))
    throw std::runtime_error("gpuq_test_decompress: device mode needs a session");

  // layout: blocks packed after raw_lead; images 16-aligned, pad after
  std::vector<uint64_t> src_off(n_pages), dst_off(n_pages);
  uint64_t raw_len = (uint64_t)raw_lead, img_len = 0;
  for (int32_t i = 0; i < n_pages; i++) {
    const int codec = pages[i].codec;
    if (codec != CODEC_UNCOMPRESSED && codec != CODEC_SNAPPY &&
        codec != CODEC_LZ4_RAW)
      throw std::runtime_error("gpuq_test_decompress: unsupported codec");
    if (codec == CODEC_UNCOMPRESSED && pages[i].comp_len != pages[i].uncomp_len)
      throw std::runtime_error("gpuq_test_decompress: uncompressed size mismatch");
    src_off[i] = raw_len;
    dst_off[i] = img_len;
    raw_len += pages[i].comp_len;
    img_len += ((uint64_t)pages[i].uncomp_len + 15) & ~15ull;
  }
  const uint64_t arena = img_len + DEC_PAD;
  if (arena_len) *arena_len = arena;
  if (guard_len) *guard_len = DEC_PAD;
  if (d_err) *d_err = 0;
  if (out_cap < arena)
    throw std::runtime_error("gpuq_test_decompress: output buffer too small");

  // plan every page first: a stream the walk rejects throws here, before
  // anything is allocated or enqueued
  DecompRecs R;
  for (int32_t i = 0; i < n_pages; i++)
    plan_decomp_page(R, pages[i].codec, pages[i].comp, src_off[i], dst_off[i],
                     pages[i].comp_len, pages[i].uncomp_len,
                     pages[i].codec == CODEC_UNCOMPRESSED, pmode, &stats[i]);
  check_decomp_bounds(R, raw_len, img_len);

  std::vector<uint8_t> raw;
  if (!host_only || replay) {
    raw.assign(raw_len + (replay ? RAW_SLACK : 0), 0);
    for (int32_t i = 0; i < n_pages; i++)
      if (pages[i].comp_len)
        std::memcpy(raw.data() + src_off[i], pages[i].comp, pages[i].comp_len);
  }

  if (host_only) {
    std::memset(out, sentinel, arena);
    if (replay) {
      replay_decompress(raw.data(), out, R);
      for (const auto& h : R.himgs)
        std::memcpy(out + h.first, h.second.data(), h.second.size());
      return 0;
    }
    for (int32_t i = 0; i < n_pages; i++) {
      const gpuq_decomp_page& p = pages[i];
      uint8_t* o = out + dst_off[i];
      int got;
      if (stats[i].mode == GPUQ_DECOMP_PAGE_RAW) {
        if (p.uncomp_len) std::memcpy(o, p.comp, p.uncomp_len);
        got = (int)p.uncomp_len;
      } else if (p.codec == CODEC_SNAPPY) {
        got = snappy_decompress_host(p.comp, p.comp_len, o, p.uncomp_len);
      } else {
        got = lz4_decompress_host(p.comp, p.comp_len, o, p.uncomp_len);
      }
      if (got != (int)p.uncomp_len)
        throw std::runtime_error("gpuq_test_decompress: host decode failure");
    }
    return 0;
  }

  HIP_TRY(hipSetDevice(ctx->devices[0]));
  DevBufs B;
  HIP_TRY(hipStreamCreateWithFlags(&B.stream, hipStreamNonBlocking));
  uint8_t* d_raw = B.alloc<uint8_t>(raw_len + RAW_SLACK);
  uint8_t* d_dec = B.alloc<uint8_t>(arena);
  int32_t* d_e = B.alloc<int32_t>(4);
  HIP_TRY(hipMemsetAsync(d_dec, sentinel, arena, B.stream));
  HIP_TRY(hipMemsetAsync(d_e, 0, 4, B.stream));
  if (raw_len)
    HIP_TRY(hipMemcpyAsync(d_raw, raw.data(), raw_len, hipMemcpyHostToDevice,
                           B.stream));
  for (const auto& h : R.himgs)
    if (!h.second.empty())
      HIP_TRY(hipMemcpyAsync(d_dec + h.first, h.second.data(), h.second.size(),
                             hipMemcpyHostToDevice, B.stream));
  DecompDev D{
      d_raw, d_dec,
      B.upload(R.segs), (int)R.segs.size(),
      B.upload(R.seqs), B.upload(R.tiles), (int)R.tiles.size(),
      seq_tile_batch_env(),   // read per call: one process can run every K
      B.upload(R.lits_wave), (int)R.lits_wave.size(),
      B.upload(R.res_lane), (int64_t)R.res_lane.size(),
      B.upload(R.res_wave), (int)R.res_wave.size(),
      B.upload(R.piece_pool), B.upload(R.brs),
      B.upload(R.pagebrs), (int)R.pagebrs.size(), d_e};
  launch_decompress(B.stream, D);
  HIP_TRY(hipGetLastError());
  int32_t err = 0;
  HIP_TRY(hipMemcpyAsync(out, d_dec, arena, hipMemcpyDeviceToHost, B.stream));
  HIP_TRY(hipMemcpyAsync(&err, d_e, 4, hipMemcpyDeviceToHost, B.stream));
  HIP_TRY(hipStreamSynchronize(B.stream));
  if (d_err) *d_err = err;
  return 0;
} catch (const std::exception& e) {
  if (ctx) ctx->set_error(e.what());
  else g_null_ctx_error = e.what();
  return -1;
}

// ------------------------------------------------------------------
// test support: the WHERE-tree mask-combine kernels on caller-supplied bytes
// (include/gpuq.h gpuq_test_mask_ops)
// ------------------------------------------------------------------
// test support: like_compile + like_match (like.h) on one value — the very
// function eval_str_pred, k_like_win<> and k_cmp_str call
extern "C" int32_t gpuq_test_like_match(const char* pattern,
                                        uint32_t pattern_len, int32_t fold,
                                        const uint8_t* value, uint32_t len) {
  LikePat P;
  if (like_compile(pattern, pattern_len, fold != 0, &P)) return -1;
  auto get = [&](uint32_t i) { return value[i]; };
  return fold ? like_match<true>(P, get, len) : like_match<false>(P, get, len);
}

extern "C" int32_t gpuq_test_mask_ops(gpuq_ctx* ctx, int32_t op,
                                      const uint8_t* a, const uint8_t* b,
                                      int64_t n, int32_t a_lead,
                                      int32_t b_lead, uint8_t* out_a,
                                      uint8_t* out_b) try {
  if (n < 0 || (n > 0 && (!a || !b)) || !out_a || !out_b || a_lead < 0 ||
      a_lead > 15 || b_lead < 0 || b_lead > 15 ||
      (op != GPUQ_MASK_OR_RESET && op != GPUQ_MASK_AND))
    throw std::runtime_error("gpuq_test_mask_ops: bad argument");
  if (!ctx || ctx->devices.empty())
    throw std::runtime_error("gpuq_test_mask_ops: needs a session");
  HIP_TRY(hipSetDevice(ctx->devices[0]));
  struct Bufs {
    uint8_t* d[2] = {nullptr, nullptr};
    hipStream_t stream = nullptr;
    ~Bufs() {
      for (auto* p : d) if (p) (void)hipFree(p);
      if (stream) (void)hipStreamDestroy(stream);
    }
  } B;
  HIP_TRY(hipStreamCreateWithFlags(&B.stream, hipStreamNonBlocking));
  // hipMalloc returns 256 B-aligned memory and the margin is a multiple of
  // 16: the data lands at an address with (address % 16) == lead
  const uint8_t* src[2] = {a, b};
  const int32_t lead[2] = {a_lead, b_lead};
  size_t len[2];
  for (int i = 0; i < 2; i++) {
    len[i] = 2 * (size_t)GPUQ_MASK_TEST_MARGIN + (size_t)lead[i] + (size_t)n;
    HIP_TRY(hipMalloc(&B.d[i], len[i]));
    HIP_TRY(hipMemsetAsync(B.d[i], GPUQ_MASK_TEST_SENTINEL, len[i], B.stream));
    if (n)
      HIP_TRY(hipMemcpyAsync(B.d[i] + GPUQ_MASK_TEST_MARGIN + lead[i], src[i],
                             (size_t)n, hipMemcpyHostToDevice, B.stream));
  }
  uint8_t* da = B.d[0] + GPUQ_MASK_TEST_MARGIN + a_lead;
  uint8_t* db = B.d[1] + GPUQ_MASK_TEST_MARGIN + b_lead;
  if (op == GPUQ_MASK_OR_RESET) launch_mask_or_reset(B.stream, da, db, n);
  else launch_mask_and(B.stream, da, db, n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_a, B.d[0], len[0], hipMemcpyDeviceToHost, B.stream));
  HIP_TRY(hipMemcpyAsync(out_b, B.d[1], len[1], hipMemcpyDeviceToHost, B.stream));
  HIP_TRY(hipStreamSynchronize(B.stream));
  return 0;
} catch (const std::exception& e) {
  if (ctx) ctx->set_error(e.what());
  else g_null_ctx_error = e.what();
  return -1;
}
