// General LIKE / ILIKE patterns (GPUQ_LIKE .. GPUQ_NOT_ILIKE, gpuq.h): the
// compiled pattern and the ONE matcher every path calls — the host LUT build
// (eval_str_pred), the window kernel (k_like_win<>, its oversized-value
// branch included) and the hash-mode kernel (k_cmp_str). Compiles as plain
// C++ (g++) and as HIP; no allocation, no recursion, no backtracking.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#if defined(__HIP__) || defined(__CUDACC__)
#define LIKE_HD __host__ __device__ __forceinline__
#else
#define LIKE_HD inline
#endif

namespace gpuq {

constexpr int LIKE_MAX_ELEMS = 255;  // literal-or-'_' elements
constexpr int LIKE_MAX_SEGS = 16;    // '%'-separated pieces, the empty
                                     // leading / trailing ones included
enum { LIKE_SEG_PCT_BEFORE = 1, LIKE_SEG_PCT_AFTER = 2 };

// Compiled pattern: a flat element array (literal byte, or ANY = '_') cut
// into segments at every run of '%'. Escapes are resolved and consecutive
// '%' collapsed by like_compile, so a middle segment is never empty; the
// first and the last may be ('%abc' has an empty first segment). Bytes only:
// the struct has alignment 1 and travels in the needle pool as is.
struct LikePat {
  uint8_t n_seg;                     // 1 (no '%') .. LIKE_MAX_SEGS
  uint8_t n_elem;
  uint8_t seg_start[LIKE_MAX_SEGS];  // first element of the segment
  uint8_t seg_len[LIKE_MAX_SEGS];
  uint8_t seg_flags[LIKE_MAX_SEGS];  // LIKE_SEG_PCT_*
  uint8_t any[32];                   // bit e: element e is '_'
  uint8_t lit[LIKE_MAX_ELEMS];       // element e's byte (lower-cased for
                                     // ILIKE); 0 for '_'
};

constexpr uint32_t LIKE_FAIL = 0xFFFFFFFFu;

LIKE_HD bool like_is_any(const LikePat& P, uint32_t e) {
  return (P.any[e >> 3] >> (e & 7)) & 1;
}
// ASCII fold, as GPUQ_ICONTAINS: 'A'-'Z' only, bytes >= 0x80 untouched
LIKE_HD uint8_t like_fold(uint8_t c) {
  return (uint8_t)(c - 'A') < 26u ? (uint8_t)(c | 0x20) : c;
}
LIKE_HD bool like_is_cont(uint8_t c) { return (c & 0xC0) == 0x80; }

// Segment s forward from pos, never reading at or past `limit`: the end
// position, or LIKE_FAIL. '_' takes one byte plus the continuation bytes
// (0x80..0xBF) that directly follow it below `limit`.
template <bool FOLD, class Get>
LIKE_HD uint32_t like_seg_fwd(const LikePat& P, uint32_t s, Get get,
                              uint32_t pos, uint32_t limit) {
  uint32_t e = P.seg_start[s];
  const uint32_t ee = e + P.seg_len[s];
  for (; e < ee; e++) {
    if (pos >= limit) return LIKE_FAIL;  // bound first, then the byte
    const uint8_t c = get(pos);
    pos++;
    if (like_is_any(P, e)) {
      while (pos < limit && like_is_cont(get(pos))) pos++;
    } else if ((FOLD ? like_fold(c) : c) != P.lit[e]) {
      return LIKE_FAIL;
    }
  }
  return pos;
}

// Segment s backward from p (exclusive end), never reading below 0: the
// start position, or LIKE_FAIL. A literal compares v[p-1]; '_' steps back
// over continuation bytes to the lead byte (or to byte 0).
template <bool FOLD, class Get>
LIKE_HD uint32_t like_seg_bwd(const LikePat& P, uint32_t s, Get get,
                              uint32_t p) {
  const uint32_t e0 = P.seg_start[s];
  for (uint32_t e = e0 + P.seg_len[s]; e > e0; e--) {
    if (p == 0) return LIKE_FAIL;  // bound first, then the byte
    p--;
    uint8_t c = get(p);
    if (like_is_any(P, e - 1)) {
      while (p > 0 && like_is_cont(c)) { p--; c = get(p); }
    } else if ((FOLD ? like_fold(c) : c) != P.lit[e - 1]) {
      return LIKE_FAIL;
    }
  }
  return p;
}

// Leftmost start q in [pos, tail] from which middle segment s matches and
// ends at or before tail: the END of that match, or LIKE_FAIL. Every element
// takes at least one byte, so no start after tail - seg_len can match; and
// since every element takes exactly one character, the leftmost start is
// also the earliest end.
template <bool FOLD, class Get>
LIKE_HD uint32_t like_seg_find(const LikePat& P, uint32_t s, Get get,
                               uint32_t pos, uint32_t tail) {
  const uint32_t sl = P.seg_len[s];
  for (uint32_t q = pos; q <= tail && sl <= tail - q; q++) {
    const uint32_t e = like_seg_fwd<FOLD>(P, s, get, q, tail);
    if (e != LIKE_FAIL) return e;
  }
  return LIKE_FAIL;
}

// Does the whole value v[0, len) (read through get(i), i < len only) match?
// Anchored at both ends. No '%': the single segment must end at len.
// Otherwise the first segment matches forward from 0 (-> pos), the last
// backward from len (-> tail), they must not overlap, and each middle
// segment takes its leftmost match inside [pos, tail].
template <bool FOLD, class Get>
LIKE_HD bool like_match(const LikePat& P, Get get, uint32_t len) {
  uint32_t pos = like_seg_fwd<FOLD>(P, 0, get, 0, len);
  if (P.n_seg == 1) return pos == len;
  if (pos == LIKE_FAIL) return false;
  const uint32_t last = P.n_seg - 1u;
  const uint32_t tail = like_seg_bwd<FOLD>(P, last, get, len);
  if (tail == LIKE_FAIL || tail < pos) return false;
  for (uint32_t s = 1; s < last; s++) {
    pos = like_seg_find<FOLD>(P, s, get, pos, tail);
    if (pos == LIKE_FAIL) return false;
  }
  return true;
}

// ---- host only: pattern compile and canonical shapes -------------------

// SQL pattern as written -> LikePat. '%' any byte sequence, '_' one
// character, backslash makes the next byte literal. fold: lower-case the
// literal bytes ('A'-'Z'); a literal byte >= 0x80 is then an error. Returns
// nullptr, or the reason: "trailing backslash", "too many elements",
// "too many segments", "non-ascii".
inline const char* like_compile(const char* pat, size_t n, bool fold,
                                LikePat* out) {
  LikePat P{};
  P.n_seg = 1;
  bool last_pct = false;
  for (size_t i = 0; i < n; i++) {
    uint8_t c = (uint8_t)pat[i];
    bool lit = true;
    if (c == '\\') {
      if (i + 1 >= n) return "trailing backslash";
      c = (uint8_t)pat[++i];
    } else if (c == '%') {
      if (last_pct) continue;  // '%%' == '%'
      last_pct = true;
      if (P.n_seg >= LIKE_MAX_SEGS) return "too many segments";
      P.seg_flags[P.n_seg - 1] |= LIKE_SEG_PCT_AFTER;
      P.seg_start[P.n_seg] = P.n_elem;
      P.seg_flags[P.n_seg] = LIKE_SEG_PCT_BEFORE;
      P.n_seg++;
      continue;
    } else if (c == '_') {
      lit = false;
    }
    last_pct = false;
    if (P.n_elem >= LIKE_MAX_ELEMS) return "too many elements";
    const uint32_t e = P.n_elem++;
    P.seg_len[P.n_seg - 1]++;
    if (!lit) {
      P.any[e >> 3] |= (uint8_t)(1u << (e & 7));
    } else {
      if (fold && c >= 0x80) return "non-ascii";
      P.lit[e] = fold ? like_fold(c) : c;
    }
  }
  *out = P;
  return nullptr;
}

// A pattern that IS one of the fixed shapes, so the plan can run the
// existing op: '%lit%' (LIKE_SHAPE_CONTAINS, lit non-empty), 'lit%', '%lit',
// or nothing but '%' (LIKE_SHAPE_ALL). Any '_' makes it LIKE_SHAPE_GENERAL,
// as does an inner '%' or no '%' at all. *lit receives the bare literal.
enum LikeShape { LIKE_SHAPE_GENERAL = 0, LIKE_SHAPE_CONTAINS, LIKE_SHAPE_PREFIX,
                 LIKE_SHAPE_SUFFIX, LIKE_SHAPE_ALL };
inline LikeShape like_shape(const LikePat& P, std::string* lit) {
  for (uint32_t e = 0; e < P.n_elem; e++)
    if (like_is_any(P, e)) return LIKE_SHAPE_GENERAL;
  lit->assign((const char*)P.lit, P.n_elem);
  if (P.n_seg == 2) {
    if (P.n_elem == 0) return LIKE_SHAPE_ALL;
    if (P.seg_len[1] == 0) return LIKE_SHAPE_PREFIX;
    if (P.seg_len[0] == 0) return LIKE_SHAPE_SUFFIX;
  } else if (P.n_seg == 3 && P.seg_len[0] == 0 && P.seg_len[2] == 0) {
    return LIKE_SHAPE_CONTAINS;
  }
  return LIKE_SHAPE_GENERAL;
}

}  // namespace gpuq
