// gpemu_host_alloc.hpp -- host code: how the library's device buffers are replaced and grown.
// No HIP call here: the allocator is a parameter (gpemu.hip passes hipMalloc / hipFree,
// tests/host/grow_check.cpp a stub that can fail), so the rules below are checked on the CPU.
//   Alloc: int malloc(void** p, size_t bytes) (0: success), void free(void* p).
#pragma once

#include <cstddef>

namespace gpe {

// Replace *p by a fresh buffer of count elements (contents not kept; count 0: no buffer).
// Returns the allocator's status; on failure *p is null.
template <class Alloc, class T>
int realloc_buf(Alloc& al, T** p, size_t count) {
  if (*p) {
    al.free(*p);
    *p = nullptr;
  }
  if (count == 0) return 0;
  void* q = nullptr;
  const int e = al.malloc(&q, count * sizeof(T));
  if (e != 0) return e;
  *p = static_cast<T*>(q);
  return 0;
}

// Grow *p to at least need elements (contents not kept); *cap is its capacity.  The cap is
// zeroed before the reallocation: a failed one leaves the buffer null, and the next call must
// not find the old, larger cap and skip it.
template <class Alloc, class T>
int grow_to(Alloc& al, T** p, size_t* cap, size_t need) {
  if (need <= *cap) return 0;
  *cap = 0;
  const int e = realloc_buf(al, p, need);
  if (e == 0) *cap = need;
  return e;
}

}  // namespace gpe
