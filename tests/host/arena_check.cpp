// Stand-alone host check of FsfArena (csrc/common.h): a measuring arena and a real arena over a malloc'ed block of exactly the measured
// size agree on every slice; one byte less poisons the real one from the failing take onward.  Built with hipcc and the host
// address / undefined-behaviour sanitizers by tests/test_workspace_layout_cpu.py; host code only, no HIP call is made.
//
//   arena_check [sequences]   -> "sequences=S takes=T mismatches=M" and exit status 0 iff M == 0
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../fullysparsefusion_amd/csrc/common.h"

namespace {

struct B1 { char b[1]; };
struct B3 { char b[3]; };
struct B12 { char b[12]; };
struct B16 { char b[16]; };

// one take of `count` elements of the type `kind` selects (1 to 16 bytes), or a take_bytes
void* take(FsfArena& a, int kind, int64_t count) {
  switch (kind) {
    case 0: return a.take<B1>(count);
    case 1: return a.take<uint16_t>(count);
    case 2: return a.take<B3>(count);
    case 3: return a.take<uint32_t>(count);
    case 4: return a.take<uint64_t>(count);
    case 5: return a.take<B12>(count);
    case 6: return a.take<B16>(count);
    default: return a.take_bytes(count);
  }
}
int64_t elem_bytes(int kind) {
  static const int64_t b[8] = {1, 2, 3, 4, 8, 12, 16, 1};
  return b[kind];
}

}  // namespace

int main(int argc, char** argv) {
  const int sequences = argc > 1 ? atoi(argv[1]) : 300;
  std::mt19937_64 rng(7);
  int64_t mismatches = 0, takes = 0;
  for (int s = 0; s < sequences; ++s) {
    const int len = 1 + (int)(rng() % 12);
    std::vector<int> kind(len);
    std::vector<int64_t> count(len), at(len), bytes(len);
    FsfArena m = FsfArena::measure();
    for (int i = 0; i < len; ++i) {
      kind[i] = (int)(rng() % 8);
      const uint64_t r = rng() % 10;
      count[i] = r == 0 ? 0 : (r == 1 ? -(int64_t)(rng() % 1000) - 1 : (r < 6 ? (int64_t)(rng() % 70) : (int64_t)(rng() % 5000)));
      at[i] = m.offset();
      if (take(m, kind[i], count[i]) != nullptr) ++mismatches;  // measuring: no memory behind it
      bytes[i] = m.offset() - at[i];
      // the arena's one rounding rule: count < 1 is one element, slices are whole multiples of 256 bytes
      const int64_t want = ((count[i] > 0 ? count[i] : 1) * elem_bytes(kind[i]) + 255) / 256 * 256;
      if (bytes[i] != want || at[i] % 256 != 0 || !m.ok()) ++mismatches;
    }
    takes += len;
    if (m.used != m.offset()) ++mismatches;
    // exactly the measured size: every slice where the measuring arena put it, inside the block, writable end to end
    char* block = (char*)malloc((size_t)m.used);
    {
      FsfArena a(block, m.used);
      for (int i = 0; i < len; ++i) {
        if (a.offset() != at[i]) ++mismatches;
        char* p = (char*)take(a, kind[i], count[i]);
        if (p != block + at[i] || !a.ok()) {
          ++mismatches;
          continue;
        }
        p[0] = 1;
        p[bytes[i] - 1] = 1;  // (the sanitizer watches the block's end)
      }
      if (a.used != m.used || !a.ok()) ++mismatches;
    }
    // one byte less: the take that no longer fits returns null and so does every take after it
    {
      FsfArena a(block, m.used - 1);
      bool failed = false;
      for (int i = 0; i < len; ++i) {
        void* p = take(a, kind[i], count[i]);
        if (!failed && at[i] + bytes[i] > m.used - 1) failed = true;
        if (failed ? (p != nullptr || a.ok()) : (p != block + at[i] || !a.ok())) ++mismatches;
      }
      if (!failed || a.ok()) ++mismatches;
    }
    // no memory at all behind a real arena: poisoned by its first take
    {
      FsfArena a(nullptr, m.used);
      if (take(a, kind[0], count[0]) != nullptr || a.ok()) ++mismatches;
    }
    free(block);
  }
  printf("sequences=%d takes=%lld mismatches=%lld\n", sequences, (long long)takes, (long long)mismatches);
  return mismatches == 0 ? 0 : 1;
}
