// objective_check.cpp -- the objective's host arithmetic (csrc/gpemu_objective.hpp with
// gpemu_small.hpp) driven from stdin by tests/test_objective_host.py: no HIP, no GPU, any
// C++17 compiler.  One command per record, whitespace-separated, doubles as strtod reads them
// (hex floats, nan, inf); one line of output per command, doubles as %a:
//   value P d kernel nu fitnug gp4ml s2 n n_hp std_r logdetA G[P*P] red[d+3]
//       -> small_from_gram, objective_value, small_t2, objective_grad
//   args variant kernel d n_hp nu_fixed m hp[m]          -> objective_args
//   inv d hp[d]                                          -> inv_length_scales (out preset to 7)
//   read P d nld nh tag name m h[m]                      -> OneLaunchResult
//   kernel code predict nu                               -> kernel_ok / _alt / _fam / _consts
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
    std::fprintf(stderr, "objective_check: input ended inside a record\n");
    std::exit(2);
  }
  char* end = nullptr;
  const double v = std::strtod(t.c_str(), &end);
  if (end == t.c_str() || *end) {
    std::fprintf(stderr, "objective_check: not a number: %s\n", t.c_str());
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
    if (cmd == "value") {
      const int P = ri(), d = ri(), kernel = ri();
      const double nu = rd();
      const bool fitnug = ri() != 0, gp4ml = ri() != 0;
      const double s2 = rd(), n = rd();
      const int n_hp = ri();
      const bool std_r = ri() != 0;
      const double logdetA = rd();
      const std::vector<double> G = rv(P * P), red = rv(d + 3);
      const SmallAlgebra sa = small_from_gram(G, P);
      if (!sa.ok) {
        std::printf("value notpd %s\n", Q_NOT_PD);
        continue;
      }
      const ObjValue v = objective_value(sa, logdetA, n, P - 1, gp4ml, s2);
      const std::vector<double> T2 = small_t2(sa, P - 1, v.cfac);
      std::vector<double> grad((size_t)n_hp, 0.0);
      objective_grad(red.data(), d, kernel, nu, fitnug, gp4ml, v.gscale, s2, n_hp, grad.data(), std_r);
      const double val[4] = {v.llh, v.sig2, v.cfac, v.gscale};
      std::printf("value ok");
      put("val", val, 4);
      put("T2", T2.data(), (int)T2.size());
      put("grad", grad.data(), n_hp);
      std::printf("\n");
    } else if (cmd == "args") {
      const int variant = ri(), kernel = ri(), d = ri(), n_hp = ri();
      const double nu_fixed = rd();
      const std::vector<double> hp = rv(ri());   // (exactly as long as the caller's: a read past it is the sanitizer's)
      ObjArgs a;
      std::string err;
      const int rc = objective_args(variant, kernel, d, hp.data(), n_hp, nu_fixed, &a, &err);
      if (rc != GPE_OK) {
        std::printf("args %d %s\n", rc, err.c_str());
        continue;
      }
      const double val[3] = {a.nu, a.s2, a.rscale};
      std::printf("args 0 %d %d", (int)a.gp4ml, (int)a.fitnug);
      put("val", val, 3);
      std::printf("\n");
    } else if (cmd == "inv") {
      const int d = ri();
      const std::vector<double> hp = rv(d);
      std::vector<double> out((size_t)d, 7.0);
      const int bad = inv_length_scales(hp.data(), d, out.data());
      std::printf("inv %d", bad);
      put("out", out.data(), d);
      std::printf(" msg %s\n", bad >= 0 ? bad_length_scale(bad).c_str() : "-");
    } else if (cmd == "read") {
      const int P = ri(), d = ri(), nld = ri(), nh = ri();
      const double tag = rd();
      std::string name;
      std::cin >> name;
      const std::vector<double> h = rv(ri());
      const OneLaunchResult r{h.data(), P, d, nld, nh, tag, name.c_str()};
      std::string err;
      const int rc = r.status(&err);
      if (rc != GPE_OK) {
        std::printf("read status %d %s\n", rc, err.c_str());
        continue;
      }
      const double ld = r.logdetA();
      std::printf("read status 0");
      put("logdetA", &ld, 1);
      std::printf(" q_refused %d", (int)r.q_refused());
      std::vector<double> red((size_t)d + 3, 0.0);
      const int rs = r.sums(red.data(), &err);
      if (rs != GPE_OK) {
        std::printf(" sums %d %s\n", rs, err.c_str());
        continue;
      }
      put("sums 0 red", red.data(), d + 3);
      std::printf("\n");
    } else if (cmd == "kernel") {
      const int code = ri();
      const bool predict = ri() != 0;
      const double nu = rd();
      double c[2];
      kernel_consts(code, nu, predict, &c[0], &c[1]);
      std::printf("kernel %d %d %d", (int)kernel_ok(code), (int)kernel_alt(code), kernel_fam(code));
      put("consts", c, 2);
      std::printf("\n");
    } else {
      std::fprintf(stderr, "objective_check: unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  std::printf("objective_check OK\n");
  return 0;
}
