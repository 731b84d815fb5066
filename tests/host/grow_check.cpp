// grow_check.cpp -- host-only check of how the library's device buffers grow
// (gpemu_host_alloc.hpp: realloc_buf, grow_to) against a stub allocator that can fail.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I gp_emu_uqsa_amd/csrc tests/host/grow_check.cpp
//
// No HIP runtime call and no GPU.  Prints "grow_check OK" when every check holds.
#include <cstdio>
#include <cstdlib>

#include "gpemu_host_alloc.hpp"

namespace {

int g_fail = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

// malloc / free with a byte limit (requests beyond it fail with status 2) and counters
struct StubAlloc {
  size_t limit;
  int mallocs = 0, frees = 0, live = 0;
  int malloc(void** p, size_t bytes) {
    if (bytes > limit) return 2;
    *p = std::malloc(bytes);
    ++mallocs;
    ++live;
    return *p ? 0 : 2;
  }
  void free(void* p) {
    std::free(p);
    ++frees;
    --live;
  }
};

}  // namespace

int main() {
  StubAlloc al{1000 * sizeof(double)};
  double* p = nullptr;
  size_t cap = 0;
  CHECK(gpe::grow_to(al, &p, &cap, (size_t)100) == 0 && p && cap == 100 && al.mallocs == 1);
  p[99] = 1.0;   // (the sanitizer sees a short buffer)
  // a request within capacity does not reallocate
  double* const p0 = p;
  CHECK(gpe::grow_to(al, &p, &cap, (size_t)100) == 0 && gpe::grow_to(al, &p, &cap, (size_t)7) == 0);
  CHECK(p == p0 && cap == 100 && al.mallocs == 1 && al.frees == 0);
  // after a failed grow the pointer is null, the capacity 0 and the old buffer freed
  CHECK(gpe::grow_to(al, &p, &cap, (size_t)5000) == 2);
  CHECK(p == nullptr && cap == 0 && al.live == 0);
  // so the next smaller request allocates (a stale cap of 100 would have skipped it)
  CHECK(gpe::grow_to(al, &p, &cap, (size_t)50) == 0 && p && cap == 50 && al.live == 1);
  p[49] = 2.0;
  // growth replaces the buffer
  CHECK(gpe::grow_to(al, &p, &cap, (size_t)1000) == 0 && p && cap == 1000 && al.live == 1);
  p[999] = 3.0;
  // another element type; realloc_buf to count 0 frees and leaves null
  float* f = nullptr;
  size_t fcap = 0;
  CHECK(gpe::grow_to(al, &f, &fcap, (size_t)2000) == 0 && f && fcap == 2000);   // 8000 bytes: fits
  CHECK(gpe::grow_to(al, &f, &fcap, (size_t)2001) == 2 && !f && fcap == 0);
  CHECK(gpe::realloc_buf(al, &p, (size_t)0) == 0 && p == nullptr && al.live == 0);
  if (g_fail) {
    std::printf("grow_check: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("grow_check OK\n");
  return 0;
}
