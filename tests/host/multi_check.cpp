// multi_check.cpp -- the separable multi-output objective's host arithmetic
// (small_multi_from_gram and small_multi_t2 of csrc/gpemu_small.hpp, objective_value_multi of
// csrc/gpemu_objective.hpp) driven from stdin by tests/test_multi_output_host.py: no HIP, no
// GPU, any C++17 compiler.  One command per record, whitespace-separated, doubles as strtod
// reads them (hex floats); one line of output per command, doubles as %a:
//   multi p q d kernel nu fitnug n n_hp logdetA G[(p+q)^2] red[d+3]
//       -> "multi ok llh <1> cfac <1> gscale <1> Sigma <p*p> B <q*p> T2 <(p+q)^2> grad <n_hp>"
//          or "multi notpd <message>"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "gpemu_objective.hpp"

using namespace gpe;

static double rd() {
  std::string t;
  if (!(std::cin >> t)) {
    std::fprintf(stderr, "multi_check: input ended inside a record\n");
    std::exit(2);
  }
  char* end = nullptr;
  const double v = std::strtod(t.c_str(), &end);
  if (end == t.c_str() || *end) {
    std::fprintf(stderr, "multi_check: not a number: %s\n", t.c_str());
    std::exit(2);
  }
  return v;
}
static int ri() { return (int)rd(); }
static std::vector<double> rv(int m) {
  std::vector<double> v((size_t)(m > 0 ? m : 0));
  for (double& x : v) x = rd();
  return v;
}
static void put(const char* tag, const double* v, int m) {
  std::printf(" %s", tag);
  for (int i = 0; i < m; ++i) std::printf(" %a", v[i]);
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd != "multi") {
      std::fprintf(stderr, "multi_check: unknown command %s\n", cmd.c_str());
      return 2;
    }
    const int p = ri(), q = ri(), d = ri(), kernel = ri();
    const double nu = rd();
    const bool fitnug = ri() != 0;
    const double n = rd();
    const int n_hp = ri();
    const double logdetA = rd();
    const int P = p + q;
    const std::vector<double> G = rv(P * P), red = rv(d + 3);
    const SmallMulti sm = small_multi_from_gram(G, p, q);
    if (!sm.ok()) {
      std::printf("multi notpd %s\n", sm.refused == 1 ? Q_NOT_PD : S_NOT_PD);
      continue;
    }
    const ObjValueMulti v = objective_value_multi(sm, logdetA, n);
    const std::vector<double> T2 = small_multi_t2(sm, v.cfac);
    std::vector<double> grad((size_t)n_hp, 0.0);
    objective_grad(red.data(), d, kernel, nu, fitnug, false, v.gscale, 1.0, n_hp, grad.data(), false);
    std::printf("multi ok");
    put("llh", &v.llh, 1);
    put("cfac", &v.cfac, 1);
    put("gscale", &v.gscale, 1);
    put("Sigma", v.Sigma.data(), p * p);
    put("B", sm.B.data(), q * p);
    put("T2", T2.data(), P * P);
    put("grad", grad.data(), n_hp);
    std::printf("\n");
  }
  std::printf("multi_check OK\n");
  return 0;
}
