/* gpuq — MI355X-native query-execution path for Parseable log streams.
 *
 * C-ABI drop-in boundary for the DataFusion physical-plan execution used by
 * the reference's src/query. Each entry point states the reference interface
 * it replaces (file:line in parseablehq/parseable v2.9.5). A Rust
 * `ExecutionPlan` shim can wrap this unchanged (see INTEGRATION.md for the
 * binding stub a maintainer would add); today the C++/Python host harness in
 * parseable_amd/ drives it exactly where the reference's Rust would.
 *
 * Threading: all calls are thread-safe; gpuq_plan_execute may be called
 * concurrently for different partitions (mirrors DataFusion's
 * one-stream-per-partition polling, src/query/mod.rs:341-363).
 * Ownership: the library owns device memory; exported batches are host
 * Arrow buffers released via the ArrowArrayStream release callback
 * (Arrow C Stream Interface).
 */
#ifndef GPUQ_H
#define GPUQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuq_ctx gpuq_ctx;
typedef struct gpuq_plan gpuq_plan;

/* ---- Arrow C Data/Stream Interface (stable ABI, restated per spec) ---- */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
struct ArrowSchema {
  const char* format;
  const char* name;
  const char* metadata;
  int64_t flags;
  int64_t n_children;
  struct ArrowSchema** children;
  struct ArrowSchema* dictionary;
  void (*release)(struct ArrowSchema*);
  void* private_data;
};
struct ArrowArray {
  int64_t length;
  int64_t null_count;
  int64_t offset;
  int64_t n_buffers;
  int64_t n_children;
  const void** buffers;
  struct ArrowArray** children;
  struct ArrowArray* dictionary;
  void (*release)(struct ArrowArray*);
  void* private_data;
};
#endif
#ifndef ARROW_C_STREAM_INTERFACE
#define ARROW_C_STREAM_INTERFACE
struct ArrowArrayStream {
  int (*get_schema)(struct ArrowArrayStream*, struct ArrowSchema* out);
  int (*get_next)(struct ArrowArrayStream*, struct ArrowArray* out);
  const char* (*get_last_error)(struct ArrowArrayStream*);
  void (*release)(struct ArrowArrayStream*);
  void* private_data;
};
#endif

/* ---- plan inputs (the predicate/aggregate IR of SURVEY.md §8b) ---- */

/* One parquet file of the stream, with the row groups selected by the
 * planner after manifest/min-max pruning — the product of
 * StandardTableProvider::scan's collect_from_snapshot + pruning
 * (stream_schema_provider.rs:505-600,1049-1137). row_groups==NULL selects
 * all row groups. */
typedef struct {
  const char* path;
  const int32_t* row_groups;
  int32_t n_row_groups;
} gpuq_file;

typedef enum {
  GPUQ_EQ = 0, GPUQ_NE, GPUQ_LT, GPUQ_LE, GPUQ_GT, GPUQ_GE,
  GPUQ_BETWEEN,       /* lo <= x <= hi (SQL BETWEEN); with hi_exclusive:
                         lo <= x < hi — the injected time filter shape of
                         query/mod.rs:829-888 */
  GPUQ_CONTAINS,      /* LIKE '%lit%' byte substring
                         (WhereConfigOperator::Contains,
                         alerts/alerts_utils.rs:620-622) */
  /* The rest of the filter builder's operator set (scalar_condition_expr,
   * alerts/alerts_utils.rs:612-640; condition_to_expr :426-441).
   * Semantics shared by the seven string ops:
   *  - the literal is the already-unescaped byte string: '%' and '_' in it
   *    are ordinary bytes (the caller strips ESCAPE '\' and the leading /
   *    trailing '%');
   *  - a NULL row satisfies none of them, the negated ones included (NOT
   *    LIKE on NULL is NULL, the row is dropped) — only IS_NULL selects
   *    NULL rows;
   *  - an empty literal: the positive ops match every non-null row, the
   *    negated ops match no row;
   *  - the column must be utf8 and the literal GPUQ_LIT_STR, anything else
   *    is a plan-build error;
   *  - none of them prunes a file or a row group by min/max statistics. */
  GPUQ_ICONTAINS = 8, /* ILIKE '%lit%' (alerts_utils.rs:626-628). ASCII
                         case-insensitive: bytes 'A'-'Z' fold to 'a'-'z' on
                         both sides, every other byte compares exactly. A
                         literal holding a byte >= 0x80 is rejected at plan
                         build; haystack bytes >= 0x80 are never folded
                         (differs from Unicode ILIKE for U+212A and U+017F
                         only) */
  GPUQ_STARTS_WITH,   /* LIKE 'lit%'        (alerts_utils.rs:629-631) */
  GPUQ_ENDS_WITH,     /* LIKE '%lit'        (alerts_utils.rs:635-637) */
  GPUQ_NOT_CONTAINS,  /* NOT LIKE '%lit%'   (alerts_utils.rs:623-625) */
  GPUQ_NOT_ICONTAINS, /* NOT ILIKE '%lit%'  (negation of :626-628; same
                         folding rule as GPUQ_ICONTAINS) */
  GPUQ_NOT_STARTS_WITH, /* NOT LIKE 'lit%'  (alerts_utils.rs:632-634) */
  GPUQ_NOT_ENDS_WITH, /* NOT LIKE '%lit'    (alerts_utils.rs:638-640) */
  GPUQ_IS_NULL,       /* col IS NULL (alerts_utils.rs:428-440). No literal:
                         lit_kind/str/i64/f64 are ignored. Any decodable
                         column type (utf8, i64, i32, f64, timestamp); on a
                         required column it selects nothing */
  GPUQ_IS_NOT_NULL,   /* col IS NOT NULL (alerts_utils.rs:428-440); a no-op
                         on a required column */
  /* General patterns: col [NOT] LIKE / ILIKE 'pattern' ESCAPE '\'. Unlike
   * the seven ops above, `str` is the SQL pattern AS WRITTEN:
   *  - '%' matches any byte sequence, the empty one included; '_' matches
   *    exactly one character: one byte plus every directly following byte in
   *    0x80..0xBF — one code point on valid UTF-8, deterministic on any bytes;
   *  - the escape character is always backslash (what the filter builder
   *    emits, alerts_utils.rs:621-640, and the engine's default): it makes
   *    the next character literal — \% \_ \\ and any other character too; a
   *    lone trailing backslash is a plan-build error;
   *  - the match is anchored at both ends: LIKE 'abc' is equality and
   *    LIKE '' matches only the empty string (the empty LITERAL of CONTAINS
   *    matches every non-null row instead);
   *  - a NULL row satisfies none of the four, the negated ones included;
   *  - ILIKE / NOT ILIKE fold ASCII 'A'-'Z' on both sides exactly like
   *    GPUQ_ICONTAINS: the pattern's literal bytes are lower-cased at plan
   *    build, a literal byte >= 0x80 in the pattern is a plan-build error,
   *    haystack bytes >= 0x80 are never folded;
   *  - the column must be utf8 and the literal GPUQ_LIT_STR, anything else
   *    is a plan-build error;
   *  - none of them prunes a file or a row group, or is elided by chunk
   *    statistics;
   *  - limits (plan-build errors): at most 255 literal-or-'_' elements and
   *    at most 16 '%'-separated segments, counting the empty segment before
   *    a leading and after a trailing '%' (consecutive '%' collapse);
   *  - a pattern that is exactly '%lit%', 'lit%' or '%lit' without '_'
   *    (ILIKE: '%lit%' only), or nothing but '%', builds the plan of the
   *    matching op above. */
  GPUQ_LIKE = 17,
  GPUQ_NOT_LIKE,
  GPUQ_ILIKE,
  GPUQ_NOT_ILIKE
} gpuq_op;

typedef enum { GPUQ_LIT_I64 = 0, GPUQ_LIT_F64, GPUQ_LIT_STR } gpuq_lit;

typedef struct {
  const char* column;
  int32_t op;          /* gpuq_op */
  int32_t lit_kind;    /* gpuq_lit */
  int64_t i64[2];      /* literal / BETWEEN bounds */
  double f64[2];
  const char* str;     /* utf8 literal (EQ.. / CONTAINS) */
  int32_t hi_exclusive;/* BETWEEN only */
} gpuq_pred;

/* WHERE tree over `preds`: the AND / OR groups of the filter builder
 * (Conditions { operator, condition_config, groups },
 * alerts/alert_structs.rs:195-203; get_filter_string joins a group's
 * conditions and parenthesised nested groups with " AND " / " OR ",
 * alerts/alerts_utils.rs:390-424).
 *  - node 0 is the root and has parent = -1; every other node has
 *    0 <= parent < own index, and its parent is an AND or an OR;
 *  - `pred` indexes `preds` and is read for LEAF nodes only; every pred is
 *    used by exactly one leaf;
 *  - an AND or OR without a child is an error (the reference's "conditions
 *    must have at least one condition or group"), as are more than 32 leaves
 *    and an OR nesting depth above 4 after normalisation;
 *  - normalisation: a child of its parent's kind is flattened into it, a
 *    single-child group collapses, a non-AND root is wrapped in an AND. A
 *    tree that normalises to a pure conjunction builds exactly the plan the
 *    flat `preds` list builds.
 * There is no NOT node (negation lives in the leaf ops), so the formula is
 * monotone and SQL's three-valued logic under WHERE reduces to the leaf
 * rule: a leaf is 0 on a NULL row (IS_NULL excepted) and the tree combines
 * 0/1 bytes — a row is selected iff the tree over those bytes is 1. */
typedef enum { GPUQ_NODE_LEAF = 0, GPUQ_NODE_AND, GPUQ_NODE_OR } gpuq_node_kind;
typedef struct { int32_t kind; int32_t parent; int32_t pred; } gpuq_where_node;

typedef enum {
  GPUQ_AGG_COUNT_STAR = 0, GPUQ_AGG_COUNT, GPUQ_AGG_SUM,
  GPUQ_AGG_MIN, GPUQ_AGG_MAX,
  /* COUNT(DISTINCT column) (AggregateFunction::CountDistinct,
   * alerts/alert_enums.rs:300, alerts/mod.rs:341-346): the number of
   * distinct non-NULL values of `column` among the selected rows of the
   * group.
   *  - NULLs are ignored; a group (or the no-group row) with no non-NULL
   *    selected value gives 0 — the result is never NULL;
   *  - utf8 compares by bytes; i64 / i32 / timestamp by value; f64 under the
   *    normalisation of f64 group keys (-0.0 folds into +0.0, every NaN into
   *    one canonical NaN — a possible difference from an engine that
   *    compares raw bits);
   *  - column == NULL or a missing column is a plan-build error; the agg is
   *    not allowed together with a projection; a bare count_distinct never
   *    takes the manifest count fast path;
   *  - it does not merge by + / min / max: the partial batch carries, after
   *    all fixed columns, one `agg{i}_set` list column per distinct agg with
   *    the group's distinct values, and the Final merge unions them (see
   *    gpuq_plan_execute). */
  GPUQ_AGG_COUNT_DISTINCT
} gpuq_agg_op;

typedef struct { int32_t op; const char* column; } gpuq_agg;

/* ---- session -------------------------------------------------------- */

/* device_mask: bit i selects HIP device i. Replaces the per-query session
 * setup of Query::execute (query/mod.rs:152-165,291-372). */
gpuq_ctx* gpuq_session_create(uint64_t device_mask);
void gpuq_session_destroy(gpuq_ctx*);
const char* gpuq_last_error(gpuq_ctx*);

/* ---- plan ----------------------------------------------------------- */

/* Build the physical plan. Mirrors TableProvider::scan
 * (stream_schema_provider.rs:616-753): file list + projection + pushed-down
 * predicate conjunction + group-by/aggregate spec -> executable plan.
 * Schema is taken from the parquet footers (merged; must agree).
 * projection lists output columns for non-aggregate scans (may be NULL when
 * group_by/aggs are given); with no aggregates, a projection + limit runs a
 * TOP-K scan ordered by p_timestamp DESC (the console default; ordering
 * contract stream_schema_provider.rs:181-204) and the exported batch holds
 * the projected rows. limit < 0 means none. Returns NULL on error
 * (see gpuq_last_error). */
gpuq_plan* gpuq_plan_build(gpuq_ctx*,
    const gpuq_file* files, int32_t n_files,
    const char* const* projection, int32_t n_projection,
    const gpuq_pred* preds, int32_t n_preds,
    const char* const* group_by, int32_t n_group_by,
    const gpuq_agg* aggs, int32_t n_aggs,
    int64_t limit);

/* Plan straight from Parseable's catalog metadata:
 * parses <stream_dir>/stream.json (ObjectStoreFormat snapshot,
 * storage/mod.rs:335-380) and the daily manifest JSON
 * (catalog/manifest.rs:143-157), selects manifests by the time window
 * (Snapshot::manifests, catalog/snapshot.rs:42-71), prunes files by
 * per-column min/max TypedStatistics (can_be_pruned/satisfy_constraints,
 * stream_schema_provider.rs:1049-1137), and answers bare count(*) from
 * manifest num_rows sums (query.rs:189-256). The injected time range is
 * passed as a hi_exclusive BETWEEN on p_timestamp among `preds`.
 * *fast_count: >=0 manifest-answered count (no plan); -1 plan returned
 * (or error: check return + gpuq_last_error); -2 empty relation. */
gpuq_plan* gpuq_plan_build_from_stream(gpuq_ctx*, const char* stream_dir,
    const char* const* projection, int32_t n_projection,
    const gpuq_pred* preds, int32_t n_preds,
    const char* const* group_by, int32_t n_group_by,
    const gpuq_agg* aggs, int32_t n_aggs, int64_t limit,
    int64_t* fast_count);

/* gpuq_plan_build / gpuq_plan_build_from_stream with a WHERE tree over
 * `preds` (gpuq_where_node above; Conditions, alerts/alert_structs.rs:195-203,
 * joined as get_filter_string does, alerts/alerts_utils.rs:390-424).
 * n_nodes == 0 means the AND of all preds — what the two entry points above
 * pass. Pruning evaluates the tree: a file or row group goes away only when
 * the root can match no row (an AND if any child cannot, an OR only if no
 * child can). Only leaves that are conjuncts of the root on p_timestamp
 * bound the manifest time window, and any leaf elsewhere in the tree keeps
 * the plan off the manifest count fast path. A malformed tree is a
 * plan-build error (NULL + gpuq_last_error). */
gpuq_plan* gpuq_plan_build_where(gpuq_ctx*,
    const gpuq_file* files, int32_t n_files,
    const char* const* projection, int32_t n_projection,
    const gpuq_pred* preds, int32_t n_preds,
    const char* const* group_by, int32_t n_group_by,
    const gpuq_agg* aggs, int32_t n_aggs,
    int64_t limit,
    const gpuq_where_node* nodes, int32_t n_nodes);
gpuq_plan* gpuq_plan_build_from_stream_where(gpuq_ctx*, const char* stream_dir,
    const char* const* projection, int32_t n_projection,
    const gpuq_pred* preds, int32_t n_preds,
    const char* const* group_by, int32_t n_group_by,
    const gpuq_agg* aggs, int32_t n_aggs, int64_t limit,
    int64_t* fast_count,
    const gpuq_where_node* nodes, int32_t n_nodes);

/* Per-aggregate filter: agg(x) FILTER (WHERE f), the same thing as
 * agg(CASE WHEN f THEN x END) — the spelling the reference's own SQL uses
 * (SUM(CASE WHEN .. THEN 1 ELSE 0 END), MAX(CASE WHEN ..), COUNT(DISTINCT
 * CASE WHEN .. END), handlers/http/traces.rs:492,560,591).
 *  - a row contributes to aggregate `agg` iff the WHERE selection is 1 and
 *    the filter tree is 1. The tree follows the rules of gpuq_where_node:
 *    AND / OR groups, no NOT, node 0 the root with parent -1, a leaf 0 on a
 *    NULL row (IS_NULL excepted); it combines 0/1 bytes, so three-valued
 *    logic reduces to the leaf rule as for WHERE. A single LEAF node is a
 *    one-pred filter. Normalisation is the WHERE tree's;
 *  - groups are decided by WHERE alone: __presence counts WHERE-selected
 *    rows, and a group whose rows all fail a filter stays in the result with
 *    0 for count_star / count / count_distinct and NULL for sum / min / max
 *    (and avg, its sum and count). With no group-by there is always one row;
 *  - an aggregate without a filter behaves exactly as without this call;
 *  - filter leaves never prune a file or a row group and never bound the
 *    manifest time window, a p_timestamp leaf included; a query with any
 *    filter never takes the manifest count fast path. Per-leaf chunk-stats
 *    elision still applies inside a filter (proven rows keep the 1 their
 *    buffer starts with);
 *  - a filter on count_distinct builds the distinct set from the rows
 *    passing WHERE and the filter;
 *  - all leaves of WHERE and of every filter index the one `preds` array;
 *    with n_nodes == 0 WHERE is the AND of the preds no filter uses;
 *  - plan-build errors: a filter together with a projection; more than
 *    MAX_AGGS (8) filters, `agg` out of range or two filters on one
 *    aggregate; more than 32 leaves over WHERE and all filters together; an
 *    OR depth above 4 in any one tree; a malformed filter tree (as for
 *    WHERE); a pred used by two leaves anywhere, or by none.
 * n_filters == 0 builds exactly the plan gpuq_plan_build_where builds. */
typedef struct {
  int32_t agg;                   /* index into aggs */
  const gpuq_where_node* nodes;  /* a tree of its own: node 0 root, parent -1 */
  int32_t n_nodes;               /* >= 1 */
} gpuq_agg_filter;

gpuq_plan* gpuq_plan_build_filtered(gpuq_ctx*,
    const gpuq_file* files, int32_t n_files,
    const char* const* projection, int32_t n_projection,
    const gpuq_pred* preds, int32_t n_preds,
    const char* const* group_by, int32_t n_group_by,
    const gpuq_agg* aggs, int32_t n_aggs,
    int64_t limit,
    const gpuq_where_node* nodes, int32_t n_nodes,
    const gpuq_agg_filter* filters, int32_t n_filters);
gpuq_plan* gpuq_plan_build_from_stream_filtered(gpuq_ctx*, const char* stream_dir,
    const char* const* projection, int32_t n_projection,
    const gpuq_pred* preds, int32_t n_preds,
    const char* const* group_by, int32_t n_group_by,
    const gpuq_agg* aggs, int32_t n_aggs, int64_t limit,
    int64_t* fast_count,
    const gpuq_where_node* nodes, int32_t n_nodes,
    const gpuq_agg_filter* filters, int32_t n_filters);

/* Independent output partitions, one per selected device (the byte-balanced
 * row-group shards of balanced_file_groups, stream_schema_provider.rs:146-165,
 * collapsed to one stream per GPU). */
int32_t gpuq_plan_partition_count(gpuq_plan*);

/* Stage the partition's raw column chunks into device HBM (the hot-tier
 * residency step; excluded from the timed execute — PCIe-inclusive rates are
 * reported separately). Idempotent. */
int32_t gpuq_plan_load(gpuq_plan*, int32_t partition);

/* Execute one partition on its GPU: decompress -> decode -> filter ->
 * partial hash-aggregate, and export the PARTIAL aggregate table (or
 * projected rows) as one Arrow record batch through `out`. The caller
 * merges partials across partitions/nodes — the AggregateExec
 * Partial->Final split of the reference's engine.
 * Replaces ExecutionPlan::execute(partition, ctx) -> RecordBatch stream.
 * Partial layout: keys..., __presence, then agg{i}, agg{i}_count per
 * aggregate. For GPUQ_AGG_COUNT_DISTINCT both are the int64 partition-local
 * distinct count (final when there is one partial), and after all of those
 * columns follows, per distinct agg in agg order, agg{i}_set: a never-null
 * list<utf8 | int64 | float64> of the group's distinct non-NULL values in
 * unspecified order (empty for none) — DataFusion's distinct-count
 * accumulator state is a list too. */
int32_t gpuq_plan_execute(gpuq_plan*, int32_t partition,
                          struct ArrowArrayStream* out);

/* Plan metrics, summed over executed partitions. bytes_scanned = compressed
 * bytes of the column chunks read (the reference's ParquetExec
 * `bytes_scanned` plan metric, query/mod.rs:466-481);
 * rowgroup_bytes_total = total file bytes of scanned row groups (all
 * columns). kernel_ns = GPU time inside kernels (HIP events). */
typedef struct {
  int64_t rows_scanned;
  int64_t rows_out;
  int64_t bytes_scanned;
  int64_t rowgroup_bytes_total;
  int64_t hbm_bytes_est;      /* algorithmic HBM traffic estimate */
  int64_t kernel_ns;
  int64_t exec_ns;
  int64_t load_ns;
  int64_t decomp_ns;          /* decompression kernels only */
  int64_t cache_hit_bytes;    /* compressed bytes served from the GPU-resident
                                 hot tier (decompressed chunk images cached
                                 across plans/queries, SURVEY §8f-3;
                                 keyed like hottier.rs:1405-1417) */
} gpuq_metrics;
int32_t gpuq_plan_metrics(gpuq_plan*, gpuq_metrics* out);

void gpuq_plan_destroy(gpuq_plan*);

/* Library self-description: number of visible HIP devices (-1 on failure —
 * callers on GPU hosts must treat failure as fatal, never fall back). */
int32_t gpuq_device_count(void);

/* ---- test support (NOT part of the drop-in surface) ------------------ */

/* Runs the page-decompression planning of gpuq_plan_build and the
 * decompress launches of gpuq_plan_execute on caller-supplied compressed
 * blocks, so a test can compare the decompressed arena byte for byte with
 * an independent decoder and see which path every page took. */

typedef struct {
  int32_t codec;            /* parquet codec id: 0 uncompressed, 1 snappy,
                               7 LZ4_RAW */
  const uint8_t* comp;      /* compressed block */
  uint32_t comp_len;
  uint32_t uncomp_len;      /* the page header's uncompressed size */
} gpuq_decomp_page;

/* plan mode (low byte of `mode`) */
enum {
  GPUQ_DECOMP_AUTO = 0,         /* what plan build chooses */
  GPUQ_DECOMP_FORCE_SEGMENT,    /* segment plan, litpar heuristic off */
  GPUQ_DECOMP_FORCE_LITPAR,     /* litpar plan when its walk succeeds, else
                                   the segment plan (as AUTO does) */
  GPUQ_DECOMP_FORCE_FALLBACK    /* segment plan + serial windowed resolver */
};
/* or'ed onto the plan mode: no device work, no session needed. `out` gets
 * the host scalar decoders' bytes; with REPLAY it gets a serial host replay
 * of the planned device records instead (segments, sequence tiles, literal
 * copies, resolved / windowed matches, in launch order). */
#define GPUQ_DECOMP_HOST_ONLY   0x100
#define GPUQ_DECOMP_HOST_REPLAY 0x200

/* path a page took (gpuq_decomp_stats.mode) */
enum {
  GPUQ_DECOMP_PAGE_SEGMENT = 0, /* segments + literal-resolved records */
  GPUQ_DECOMP_PAGE_LITPAR,      /* literal records + resolved records */
  GPUQ_DECOMP_PAGE_FALLBACK,    /* segments + serial windowed backrefs */
  GPUQ_DECOMP_PAGE_RAW,         /* stored uncompressed: plain copy */
  GPUQ_DECOMP_PAGE_HOST_IMAGE   /* host-decompressed image staged directly */
};

typedef struct {
  int32_t mode;                 /* GPUQ_DECOMP_PAGE_* */
  uint32_t n_seq;               /* sequences (snappy: elements) walked */
  uint32_t n_segs, n_big;       /* segments; of those, giant single-sequence */
  uint32_t n_lit_lane, n_lit_wave;
  uint32_t n_inl;               /* host-inlined pattern records */
  uint32_t n_res_lane, n_res_wave;
  uint32_t n_pieces;
  uint32_t n_backrefs, n_far;   /* windowed records; of those, far branch */
  uint32_t n_tile, n_tile_rec;  /* litpar sequence tiles and their records:
                                   every n_lit_lane run and n_inl match is
                                   in one, an adjacent pair sharing it */
} gpuq_decomp_stats;

/* The blocks are packed back to back into the raw buffer after `raw_lead`
 * (0..15) pad bytes. The decompressed arena is laid out as plan build lays
 * it out: every image starts 16-aligned, and the over-read pad follows the
 * last image. The whole arena is filled with `sentinel` before any kernel
 * runs, so the padding between images and the trailing pad double as guard
 * regions; *guard_len is the size of the trailing one, *arena_len the bytes
 * written to `out` (images + padding + guard). stats has n_pages entries.
 * *d_err receives the kernels' error word (0 in host-only modes). A stream
 * the host walk rejects is an error (-1, message via gpuq_last_error — with
 * a NULL session, gpuq_last_error(NULL)) and nothing is launched. */
int32_t gpuq_test_decompress(gpuq_ctx*, const gpuq_decomp_page* pages,
                             int32_t n_pages, int32_t raw_lead, int32_t mode,
                             uint8_t sentinel, uint8_t* out, uint64_t out_cap,
                             uint64_t* arena_len, uint64_t* guard_len,
                             gpuq_decomp_stats* stats, int32_t* d_err);

/* Runs one of the two mask-combine kernels of the WHERE-tree path on
 * caller-supplied byte arrays. op GPUQ_MASK_OR_RESET: a |= b, then b = 1
 * (k_mask_or_reset); GPUQ_MASK_AND: a &= b, b unchanged (k_mask_and). Each
 * array is copied to a device address with (address % 16) == its lead
 * (0..15), inside a buffer filled with the sentinel 0xA5: out_a / out_b
 * receive GPUQ_MASK_TEST_MARGIN + lead + n + GPUQ_MASK_TEST_MARGIN bytes,
 * the data starting at offset GPUQ_MASK_TEST_MARGIN + lead. Returns 0, or
 * -1 with the message in gpuq_last_error. */
enum { GPUQ_MASK_OR_RESET = 0, GPUQ_MASK_AND = 1 };
#define GPUQ_MASK_TEST_MARGIN 32
#define GPUQ_MASK_TEST_SENTINEL 0xA5
int32_t gpuq_test_mask_ops(gpuq_ctx*, int32_t op, const uint8_t* a,
                           const uint8_t* b, int64_t n, int32_t a_lead,
                           int32_t b_lead, uint8_t* out_a, uint8_t* out_b);

/* Compiles `pattern` (pattern_len bytes, GPUQ_LIKE syntax; fold != 0 for the
 * ILIKE rules) and runs the matcher the kernels and the LUT build share on
 * value[0, len). No canonicalisation, no device, no session. Returns 1 / 0,
 * or -1 when the pattern does not compile. */
int32_t gpuq_test_like_match(const char* pattern, uint32_t pattern_len,
                             int32_t fold, const uint8_t* value, uint32_t len);

#ifdef __cplusplus
}
#endif
#endif /* GPUQ_H */
