// Launch wrappers implemented in kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_types.h"

namespace gpuq {
void launch_lz4_seg(hipStream_t, const uint8_t* raw, uint8_t* dec,
                    const DevSeg*, int n, int32_t* d_err);
// batch: tiles per block, 1 | 2 | 4 | 8 (k_seq_tile<K>)
constexpr int SEQ_TILE_BATCH_DEFAULT = 2;
void launch_seq_tile(hipStream_t, const uint8_t* raw, uint8_t* dec,
                     const DevSeq* seqs, const DevSeqTile* tiles, int n,
                     int batch);
void launch_lit_wave(hipStream_t, const uint8_t* raw, uint8_t* dec,
                     const DevLit* lits, int n);
void launch_lz4_backrefs(hipStream_t, uint8_t* dec, const DevBr*,
                         const DevPageBr*, int n);
void launch_brres_lane(hipStream_t, uint8_t* dec, const DevBrRes*,
                       const DevPiece*, int64_t n);
void launch_brres_wave(hipStream_t, uint8_t* dec, const DevBrRes*,
                       const DevPiece*, int n);
void launch_def_levels(hipStream_t, const uint8_t* dec, const DevPage*,
                       const int32_t* ids, int n, uint8_t* valid,
                       uint8_t* null_mask, uint32_t* rowof, uint32_t* rank,
                       uint32_t* present, int32_t* d_err);
// every LIKE-family mode over PLAIN-page windows (mode: StrKind | STRF_*,
// dev_types.h): k_contains_win<FOLD, NEG> for the substring modes,
// k_affix_win<SUFFIX> for prefix/suffix, k_like_win<FOLD> for STR_PATTERN
// (needle = a compiled LikePat, like.h); a STRF_FOLD needle is lower-cased
void launch_str_win(hipStream_t, const uint8_t* dec, const DevCWin* wins,
                    int n, const DevPage* pages, const uint16_t* starts_pool,
                    const uint8_t* needle, int nlen, int mode,
                    const uint32_t* rowof, uint8_t* mask);
// IS NULL: clear the valid rows of the listed pages from the mask (after
// launch_def_levels wrote `valid` for their null-bearing pages)
void launch_null_clear_valid(hipStream_t, const uint8_t* dec, const DevPage*,
                             const int32_t* ids, int n, const uint8_t* valid,
                             uint8_t* mask);
// serial_walk (the dictionary-index decoders): parse one RLE run header per
// step instead of probing 64 positions at once (GPUQ_DICT_WALK=serial)
void launch_dict_gid(hipStream_t, const uint8_t* dec, const DevPage*,
                     const int32_t* ids, int n, const int32_t* remap_pool,
                     int32_t* out, uint8_t* valid, const uint32_t* present,
                     int mode, bool serial_walk, int32_t* d_err);
void launch_dict_i64(hipStream_t, const uint8_t* dec, const DevPage*,
                     const int32_t* ids, int n, const int64_t* dictv_pool,
                     int64_t* out, uint8_t* valid, const uint32_t* present,
                     int mode, bool serial_walk, int32_t* d_err);
void launch_dict_mask(hipStream_t, const uint8_t* dec, const DevPage*,
                      const int32_t* ids, int n, const uint8_t* lut_pool,
                      uint8_t* mask, int mode, bool serial_walk, int32_t* d_err);
void launch_dict_lut_scr(hipStream_t, const uint8_t* dec, const DevPage*,
                         const int32_t* ids, int n, const uint8_t* lut_pool,
                         uint8_t* scr, const uint32_t* present,
                         bool serial_walk, int32_t* d_err);
void launch_plain_fixed(hipStream_t, const uint8_t* dec, const DevPage*,
                        const int32_t* ids, int n, int64_t* out, uint8_t* valid,
                        const uint32_t* present, int mode, int32_t* d_err);
void launch_expand(hipStream_t, const uint8_t* dec, const DevPage*,
                   const int32_t* ids, int n, const uint8_t* scr,
                   const uint32_t* rank, const uint8_t* valid, uint8_t* out,
                   int mode);
void launch_delta_i64(hipStream_t, const uint8_t* dec, const DevPage*,
                      const int32_t* ids, int n, int64_t* out, uint8_t* valid,
                      int32_t* d_err);
void launch_cmp_i64(hipStream_t, const int64_t* col, const uint8_t* valid,
                    int64_t lo, int64_t hi, int mode, int hi_excl, int is_f64,
                    uint8_t* mask, int64_t n);
// WHERE-tree mask combines over n 0/1 bytes (any alignment, any relative
// misalignment): acc |= tmp then tmp = 1 (k_mask_or_reset); dst &= acc
// (k_mask_and)
void launch_mask_or_reset(hipStream_t, uint8_t* acc, uint8_t* tmp, int64_t n);
void launch_mask_and(hipStream_t, uint8_t* dst, const uint8_t* acc, int64_t n);
void launch_bin_i64(hipStream_t, const int64_t* col, const uint8_t* valid,
                    int64_t origin, int64_t stride, int64_t min_idx,
                    int32_t nbins, int32_t* out, int64_t n);
void launch_init_table(hipStream_t, uint64_t* table, int32_t n_groups,
                       int n_aggs, const int32_t* d_agg_kind);
void launch_dict_count(hipStream_t, const uint8_t* dec, const DevPage*,
                       const int32_t* ids, int n, const int32_t* remap_pool,
                       uint64_t* table, int32_t n_groups, int n_aggs,
                       int32_t* d_err);
// fused value decode + aggregate (kernels.hip k_val_agg): ids lists the agg
// column's dict AND PLAIN data pages; kind is AGGK_SUM/MIN/MAX_I64
void launch_val_agg(hipStream_t, const uint8_t* dec, const DevPage*,
                    const int32_t* ids, int n, const int64_t* dictv_pool,
                    const int32_t* gid, const uint8_t* mask, uint64_t* table,
                    int32_t n_groups, int n_aggs, int kind, int max_blocks,
                    bool serial_walk, int32_t* d_err);
// -> the kernel family that ran: "fast", "general", and for a plan with
// filters "fcount" (k_agg_fcount) or "general+filter" (k_agg<.., true>);
// no_fcount keeps the error-rate shape on the general kernel
const char* launch_agg(hipStream_t, const AggArgs&, bool no_fcount = false);
void launch_pool_vals(hipStream_t, const uint8_t* dec, const DevPage*,
                      const int32_t* ids, int n, const int64_t* pool,
                      int64_t* out, uint8_t* valid, const uint32_t* present,
                      int mode);
void launch_hash_build(hipStream_t, const uint8_t* dec, const int64_t* refs,
                       const uint8_t* valid, int64_t n_rows, uint64_t* hkeys,
                       int32_t* hgids, int clog2, uint32_t* counter,
                       uint64_t* gid2ref, int32_t gid_cap, int32_t* d_err);
void launch_hash_lookup(hipStream_t, const uint8_t* dec, const int64_t* refs,
                        const uint8_t* valid, int64_t n_rows,
                        const uint64_t* hkeys, const int32_t* hgids, int clog2,
                        int32_t* out_gid);
void launch_pair_build(hipStream_t, const int32_t* a, const int32_t* b,
                       int64_t n_rows, uint64_t* hkeys, int32_t* hgids,
                       int clog2, uint32_t* counter, uint64_t* gid2pair,
                       int32_t gid_cap, int32_t* d_err);
void launch_pair_lookup(hipStream_t, const int32_t* a, const int32_t* b,
                        int64_t n_rows, const uint64_t* hkeys,
                        const int32_t* hgids, int clog2, int32_t* out);
void launch_numhash_build(hipStream_t, const int64_t* vals,
                          const uint8_t* valid, int64_t n_rows,
                          uint64_t* hkeys, int32_t* hgids, int clog2,
                          uint32_t* counter, uint64_t* gid2key,
                          int32_t gid_cap, int is_f64, int32_t* d_err);
void launch_numhash_lookup(hipStream_t, const int64_t* vals,
                           const uint8_t* valid, int64_t n_rows,
                           const uint64_t* hkeys, const int32_t* hgids,
                           int clog2, int is_f64, int32_t* out_gid);
// COUNT(DISTINCT): both leave d.pairs / d.count filled (count zeroed by the
// caller). bitmap: n_groups * vpad zeroed bits, vpad a multiple of 64
// (k_distinct_mark + k_distinct_emit; use_lds: mark through a block-local LDS
// copy of the bitmap, which must fit 64 KiB). claim: hkeys filled with 0xFF
// (k_distinct_claim).
void launch_distinct_bitmap(hipStream_t, const DistinctArgs& d,
                            uint64_t* bitmap, uint32_t vpad, bool use_lds);
void launch_distinct_claim(hipStream_t, const DistinctArgs& d, uint64_t* hkeys,
                           int clog2);
void launch_cmp_str(hipStream_t, const uint8_t* dec, const int64_t* refs,
                    const uint8_t* valid, const uint8_t* lit, uint32_t lit_len,
                    int op, uint8_t* mask, int64_t n_rows);
void launch_ref_lens(hipStream_t, const uint8_t* dec, const uint64_t* refs,
                     int64_t n, uint32_t* lens);
void launch_ref_gather(hipStream_t, const uint8_t* dec, const uint64_t* refs,
                       const uint64_t* offs, int64_t n, uint8_t* out);
void launch_compact(hipStream_t, const uint8_t* mask, const int64_t* key_col,
                    int64_t n_rows, int64_t* out_keys, uint32_t* out_rows,
                    unsigned long long* counter);
void launch_gather_i64(hipStream_t, const uint32_t* rows, int64_t k,
                       const int64_t* col, int64_t* out);
void launch_gather_i32(hipStream_t, const uint32_t* rows, int64_t k,
                       const int32_t* col, int32_t* out);
void launch_gather_u8(hipStream_t, const uint32_t* rows, int64_t k,
                      const uint8_t* col, uint8_t* out);
size_t sort_pairs_desc(hipStream_t, void* d_temp, size_t temp_bytes,
                       const int64_t* keys_in, int64_t* keys_out,
                       const uint32_t* rows_in, uint32_t* rows_out, int64_t n);
}  // namespace gpuq
