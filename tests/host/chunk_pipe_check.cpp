// Stand-alone driver of csrc/gpemu_chunk_pipe.hpp for tests/test_chunk_pipe_host.py: any C++17
// compiler, no HIP, no GPU.  Each input line
//   run <m> <chunk> <fail> <at> <code>
// runs chunk_pipeline over m points in chunks of `chunk` with recording callbacks and prints the
// calls in order: d<i>/<slot> (dev of chunk i = s0 / chunk), w<slot>, h<i>/<slot>, drain, then
// rc <value>.  fail is none, dev or wait: the dev of chunk `at`, or the wait for chunk `at`,
// returns `code` instead of 0.  The callbacks also check what they are given: s0 a multiple of
// chunk below m, slot 0 or 1.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gpemu_chunk_pipe.hpp"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string cmd, fail;
    long long m = 0, chunk = 0, at = 0;
    int code = 0;
    in >> cmd >> m >> chunk >> fail >> at >> code;
    if (!in || cmd != "run" || chunk < 1 || (fail != "none" && fail != "dev" && fail != "wait")) {
      std::fprintf(stderr, "bad command: %s\n", line.c_str());
      return 2;
    }
    std::ostringstream out;
    std::vector<long long> in_slot(2, -1);   // the chunk whose results each pinned slot holds
    auto arg_ok = [&](long long s0, int slot) {
      if (s0 < 0 || s0 >= m || s0 % chunk != 0 || (slot != 0 && slot != 1)) {
        std::fprintf(stderr, "bad callback arguments: s0 %lld slot %d\n", s0, slot);
        std::exit(3);
      }
    };
    const int rc = gpe::chunk_pipeline(
        m, chunk,
        [&](long long s0, int slot) {
          arg_ok(s0, slot);
          out << "d" << s0 / chunk << "/" << slot << " ";
          in_slot[slot] = s0 / chunk;
          return fail == "dev" && s0 / chunk == at ? code : 0;
        },
        [&](int slot) {
          arg_ok(0, slot);
          out << "w" << slot << " ";
          return fail == "wait" && in_slot[slot] == at ? code : 0;
        },
        [&](long long s0, int slot) {
          arg_ok(s0, slot);
          out << "h" << s0 / chunk << "/" << slot << " ";
        },
        [&] { out << "drain "; });
    std::printf("%src %d\n", out.str().c_str(), rc);
  }
  std::printf("chunk_pipe_check OK\n");
  return 0;
}
