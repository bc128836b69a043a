// Stand-alone host check of the shared LIKE matcher (parseable_amd/csrc/like.h).
// CPU only: no HIP, no GPU, no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       scripts/like_host_check.cpp -o /tmp/like_host_check && /tmp/like_host_check
//
// Random pattern / value pairs over an alphabet with 1-, 2- and 3-byte
// characters, both ASCII cases and the three metacharacters go through
// like_compile + like_match and through a naive recursive backtracking matcher
// written here. Every value (and pattern) lives in an exactly-sized heap
// buffer, so a read before or after it is an AddressSanitizer report. Exits
// non-zero on any disagreement.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../parseable_amd/csrc/like.h"

using namespace gpuq;

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {  // xorshift64*, deterministic
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n;
}

uint8_t lower(uint8_t c) { return c >= 'A' && c <= 'Z' ? c | 0x20 : c; }
bool cont(uint8_t c) { return (c & 0xC0) == 0x80; }

// The semantics, stated the slow way. '%' tries every character boundary of
// the rest; '_' takes one byte and the continuation bytes after it; a
// backslash makes the next byte literal (the caller rejected a trailing one).
bool naive(const uint8_t* p, size_t pn, const uint8_t* v, size_t vn, bool fold) {
  if (pn == 0) return vn == 0;
  if (p[0] == '%') {
    for (size_t k = 0; k <= vn; k++) {
      if (k < vn && k > 0 && cont(v[k])) continue;
      if (naive(p + 1, pn - 1, v + k, vn - k, fold)) return true;
    }
    return false;
  }
  if (p[0] == '_') {
    if (vn == 0) return false;
    size_t k = 1;
    while (k < vn && cont(v[k])) k++;
    return naive(p + 1, pn - 1, v + k, vn - k, fold);
  }
  const size_t adv = p[0] == '\\' ? 2 : 1;
  const uint8_t lit = p[adv - 1];
  if (vn == 0) return false;
  if ((fold ? lower(v[0]) : v[0]) != (fold ? lower(lit) : lit)) return false;
  return naive(p + adv, pn - adv, v + 1, vn - 1, fold);
}

// what like_compile must say, worked out from the raw pattern
const char* naive_error(const std::string& p, bool fold) {
  size_t elems = 0, segs = 1;
  bool pct = false;
  for (size_t i = 0; i < p.size(); i++) {
    uint8_t c = (uint8_t)p[i];
    if (c == '%') {
      if (!pct && ++segs > (size_t)LIKE_MAX_SEGS) return "too many segments";
      pct = true;
      continue;
    }
    pct = false;
    bool lit = c != '_';
    if (c == '\\') {
      if (i + 1 == p.size()) return "trailing backslash";
      c = (uint8_t)p[++i];
    }
    if (++elems > (size_t)LIKE_MAX_ELEMS) return "too many elements";
    if (lit && fold && c >= 0x80) return "non-ascii";
  }
  return nullptr;
}

const char* const PAT_ALPHA[] = {"a", "b", "A", "\xC3\xA9", "\xE6\x97\xA5",
                                 "=", "%", "_", "\\"};
const char* const VAL_ALPHA[] = {"a", "b", "A", "B", "\xC3\xA9", "\xE6\x97\xA5",
                                 "=", "%", "_", "\\"};
constexpr uint32_t N_PAT = sizeof(PAT_ALPHA) / sizeof(*PAT_ALPHA);
constexpr uint32_t N_VAL = sizeof(VAL_ALPHA) / sizeof(*VAL_ALPHA);

std::unique_ptr<uint8_t[]> exact(const std::string& s) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[s.size()]);
  if (!s.empty()) memcpy(b.get(), s.data(), s.size());
  return b;
}

long n_pairs = 0, n_match = 0, n_err = 0, n_bad = 0;

void check(const std::string& pat, const std::string& val, bool fold) {
  auto pb = exact(pat);
  auto vb = exact(val);
  LikePat P;
  const char* why =
      like_compile((const char*)pb.get(), pat.size(), fold, &P);
  const char* want_why = naive_error(pat, fold);
  n_pairs++;
  if (why || want_why) {
    n_err++;
    if (!why || !want_why || strcmp(why, want_why)) {
      fprintf(stderr, "compile: pattern '%s' fold=%d: got %s, want %s\n",
              pat.c_str(), fold, why ? why : "ok", want_why ? want_why : "ok");
      n_bad++;
    }
    return;
  }
  const uint8_t* v = vb.get();
  auto get = [&](uint32_t i) { return v[i]; };
  const bool got = fold ? like_match<true>(P, get, (uint32_t)val.size())
                        : like_match<false>(P, get, (uint32_t)val.size());
  const bool want = naive(pb.get(), pat.size(), v, val.size(), fold);
  n_match += got;
  if (got != want) {
    fprintf(stderr, "match: pattern '%s' value '%s' fold=%d: got %d, want %d\n",
            pat.c_str(), val.c_str(), fold, got, want);
    n_bad++;
  }
}

}  // namespace

int main() {
  for (int it = 0; it < 200000; it++) {
    std::string val, pat;
    for (uint32_t k = rnd(9); k > 0; k--) val += VAL_ALPHA[rnd(N_VAL)];
    if (it & 1) {
      for (uint32_t k = rnd(7); k > 0; k--) pat += PAT_ALPHA[rnd(N_PAT)];
    } else {
      // derived from the value: keep a byte (escaped when it is a
      // metacharacter), '_' for a character, '%' over a run, or noise
      for (size_t i = 0; i < val.size();) {
        size_t cl = 1;
        while (i + cl < val.size() && cont((uint8_t)val[i + cl])) cl++;
        const uint32_t r = rnd(100);
        if (r < 45) {
          if (strchr("%_\\", val[i])) pat += '\\';
          pat.append(val, i, cl);
        } else if (r < 65) {
          pat += '_';
        } else if (r < 90) {
          pat += '%';
          if (rnd(2)) continue;  // '%' matching nothing
          for (uint32_t skip = rnd(3); skip > 0 && i + cl < val.size(); skip--) {
            i += cl;
            cl = 1;
            while (i + cl < val.size() && cont((uint8_t)val[i + cl])) cl++;
          }
        } else {
          pat += PAT_ALPHA[rnd(N_PAT)];
        }
        i += cl;
      }
    }
    check(pat, val, it % 3 == 0);
  }
  // the limits, from both sides
  check(std::string(255, 'a'), std::string(255, 'a'), false);
  check(std::string(256, 'a'), "a", false);
  check("%" + std::string(255, '_'), std::string(300, 'x'), true);
  {
    std::string p15, p16;
    for (int i = 0; i < 15; i++) p15 += "a%";
    p16 = p15 + "a%";
    check(p15 + "a", "aaaaaaaaaaaaaaaaaaaa", false);  // 16 segments
    check(p16 + "a", "aaaaaaaaaaaaaaaaaaaa", false);  // 17
    check(p15, "aaaaaaaaaaaaaaa", false);             // 16, the last one empty
    check("%" + p15, "aaaaaaaaaaaaaaa", false);       // 17
  }
  // a long value with every segment kind: head, middles, tail
  {
    std::string big = "Error " + std::string(40000, 'x') + " TIMEOUT";
    check("Error%TIMEOUT", big, false);
    check("%rror%x_x%TIMEOUT%", big, false);
    check("error%_%timeout", big, true);
    check("%Error%y%TIMEOUT", big, false);
  }
  printf("like_host_check: %ld pairs, %ld matches, %ld pattern errors, "
         "%ld disagreements\n", n_pairs, n_match, n_err, n_bad);
  return n_bad ? 1 : 0;
}
