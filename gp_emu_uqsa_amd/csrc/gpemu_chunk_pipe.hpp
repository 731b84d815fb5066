// gpemu_chunk_pipe.hpp -- the two-slot chunk pipeline of the posterior paths (the diagonal
// variance with its gradients, the groups' blocks, the mean for one and for p outputs): chunk
// i's device work is queued before the host turns chunk i - 1's results into outputs, so the GPU
// does not idle on the host between chunks.  Host only (no HIP header), so
// tests/host/chunk_pipe_check.cpp runs it without a GPU.
#pragma once

namespace gpe {

// The points [0, m) in chunks of `chunk`, chunk i through slot i % 2:
//   dev(s0, slot)   queues the device work of the chunk that starts at s0, the copy of its
//                   results into pinned slot `slot` and that slot's event record;
//   wait(slot)      waits for that event;
//   host(s0, slot)  reads the chunk's results out of the pinned slot.
// dev(i) is followed by wait and host of chunk i - 1, and the last chunk's after the loop.  dev
// and wait return 0 or a failure; the first failure stops the loop (no later dev, wait or host),
// calls drain() once and is returned: a failed step may leave copies into the pinned slots
// queued, and they must have ended before the staging buffer can be reused or regrown.
template <class Dev, class Wait, class Host, class Drain>
int chunk_pipeline(long long m, long long chunk, Dev&& dev, Wait&& wait, Host&& host, Drain&& drain) {
  int rc = 0, slot = 0;
  long long prev = -1;
  for (long long s0 = 0; rc == 0 && s0 < m; s0 += chunk, slot ^= 1) {
    rc = dev(s0, slot);
    if (rc == 0 && prev >= 0 && (rc = wait(slot ^ 1)) == 0) host(prev, slot ^ 1);
    prev = s0;
  }
  if (rc == 0 && prev >= 0 && (rc = wait(slot ^ 1)) == 0) host(prev, slot ^ 1);
  if (rc != 0) drain();
  return rc;
}

}  // namespace gpe
