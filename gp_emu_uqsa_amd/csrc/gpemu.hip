// gpemu.hip -- host side of libgpemu.so: context, HBM buffers, launch schedule
// and the C-ABI declared in include/gpemu.h.
//
// One objective evaluation (gp4ml / MUCM, value + gradient) runs as:
//   scale points -> K-build (lower tiles) -> right-looking blocked Cholesky
//   (per 128-column step: diagonal-block factor+inverse, panel GEMM, trailing
//   SYRK GEMM) -> recursive triangular inverse (grouped GEMM per level) ->
//   [f H] skinny solve + Gram -> host q x q algebra -> A^-1 = L^-T L^-1 (one
//   grouped GEMM) -> [alpha, W] skinny product -> fused gradient contraction.
// See DESIGN.md for the flop / byte accounting of each step.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <map>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/gpemu.h"
#include "gpemu_kernels.hpp"
#include "gpemu_gemm_sched.hpp"
#include "gpemu_chol_sched.hpp"
#include "gpemu_objective.hpp"   // (with gpemu_small.hpp)
#include "gpemu_chunk_pipe.hpp"
#include "gpemu_tiny.hpp"
#include "gpemu_snb.hpp"
#include "gpemu_ozaki.hpp"
#include "gpemu_pivchol.hpp"
#include "gpemu_imse.hpp"
#include "gpemu_postgrad.hpp"
#include "gpemu_postmean.hpp"
#include "gpemu_postmean_multi.hpp"
#include "gpemu_postgroup.hpp"
#include "gpemu_hm.hpp"
#include "gpemu_hm_mv.hpp"
#include "gpemu_hm_cand.hpp"
#include "gpemu_host_alloc.hpp"

using namespace gpe;

namespace {

thread_local std::string g_create_error;

constexpr int MAX_PROBS = 1 << 16;
constexpr int AUX_DESC_BASE = 1 << 15;
constexpr int ADHOC_DESC_BASE = MAX_PROBS - 64;

// Descriptor slots of the GEMMs outside the cached plans (adhoc_gemm), each named for its
// owner.  Live within one call: gpe_noise_sample and gpe_posterior_pivchol run the posterior
// first (ADHOC_POST_V, then the ADHOC_COV pair, re-uploaded per chunk and per block) and then
// their own slot; ADHOC_PIVCHOL is uploaded once and launched after every panel of that call,
// as is ADHOC_IMSE by gpe_posterior_imse;
// gpe_posterior_grad re-uploads the ADHOC_POST_U pair per chunk, behind that chunk's ADHOC_POST_V.
// The test and bench GEMMs stand alone.
enum AdhocSlot {
  ADHOC_POST_V = ADHOC_DESC_BASE + 0,     // posterior: V = L^-1 K* of one chunk
  ADHOC_COV = ADHOC_DESC_BASE + 1,        // cov_block: -s2 V^T V, then +s2 T T^T (two slots)
  ADHOC_NOISE = ADHOC_DESC_BASE + 3,      // gpe_noise_sample: the draws L U^T
  ADHOC_PIVCHOL = ADHOC_DESC_BASE + 4,    // gpe_posterior_pivchol: the trailing update S -= W W^T
  ADHOC_POST_U = ADHOC_DESC_BASE + 5,     // gpe_posterior_grad: U = L^-T V, then U += G tau^T (two slots)
  ADHOC_IMSE = ADHOC_DESC_BASE + 7,       // gpe_posterior_imse: the trailing update over the candidates
  ADHOC_TEST = ADHOC_DESC_BASE + 8,       // gpe_test_gemm
  ADHOC_BENCH = ADHOC_DESC_BASE + 16,     // gpe_bench_gemm
};

// rows of the Schur complement from which the objective's Cholesky is split and S runs on the
// int8 cores (GPEMU_OZAKI_CHOL_MIN)
constexpr int OZ_CHOL_MIN = 8192;
// n_pad from which the objective's int8 products carry a 15-moduli certificate
// (GPEMU_OZAKI_CERT_MIN_NP).  Below 6144 the int8 path runs only with its own thresholds lowered;
// measured there with all of them at their floors, one evaluation gains 1%
// at n_pad 4096 and 5120 and nothing at 2944 (3.58 against 3.60 ms), where the k_oz_cert launches
// and the sums cost what the sixteenth modulus saves
constexpr int OZ_CERT_MIN_NP = 4096;
// rows of the trapezoid (those from the inner split column q on) from which the split sweep's
// first phase is split once more (GPEMU_OZAKI_CHOL_NEST_MIN)
constexpr int OZ_CHOL_NEST_MIN = 12288;

// one TRTRI block pair on the int8 cores (trtri_pair_ozaki): rows of X11 / X22 (Ra / Rb),
// padded to 256 (Pa / Pb), and its two products' tile lists in dozl

// A factorisation workspace: two n_pad x n_pad buffers and their GEMM schedule.
struct Fact {
  long long n_pad = 0;
  int NB = 0;
  double* A = nullptr;   // K-build -> L -> A^-1
  double* B = nullptr;   // Dinv tiles -> L^-1 (strictly-upper tiles: scratch)
  size_t cap = 0;
  double* logdet = nullptr;  // NB per-block log-determinant parts
  int* flags = nullptr;      // FACT_FLAG_INTS x NB: flags, counters, tickets (fused Cholesky)
  int* tflags = nullptr;     // row counter and row ticket of the forward substitution (k_trsv_lower)
  // augmented tile row ([f H]^T under the matrix, TILE x n_pad, ld TILE): carried by the
  // fused Cholesky's panels and trailing updates, it ends as (L^-1 [f H])^T (training
  // workspace only)
  bool aug = false;
  double* Faug = nullptr;
  // split-K scratch of the TRTRI / LAUUM launches with few tiles (k_gemm ksplit):
  // SPLIT_SLOTS partial tiles and one counter per tile of a launch
  double* part = nullptr;
  int* tcnt = nullptr;
  // B's diagonal tiles hold the full X_tt = L_tt^-1 (k_xasm ran after the last sweep), by side
  // of the last sweep's column xh: tiles [0, xh) and [xh, NB) (xh = 0: every tile on side 1)
  bool xdone[2] = {false, false};
  int xh = 0;
  // B(0:x11, 0:x11) holds X11 = L11^-1 of the last sweep (tri_ahead; tile units, 0: not), and
  // the int8 scratch block the top pair's T = L21 X11
  int x11 = 0;
  bool t_ahead = false;
  void xclear(int h = 0) { xdone[0] = xdone[1] = t_ahead = false; x11 = 0; xh = h; }
  int desc_base = 0;         // first slot of its descriptors in the device array
  Plan plan;
};

}  // namespace

struct gpe_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;

  long long n = 0, n_pad = 0;
  int d = 0, q = 0, NB = 0;
  bool has_r = false;

  double* dX = nullptr;      // n_pad x d row-major (raw)
  double* dXw = nullptr;     // scaled by 1/delta
  double* dF = nullptr;      // n_pad x (q+1) col-major: [f H]
  double* dr = nullptr;      // n_pad
  Fact tr;                   // training matrix workspace
  Fact aux;                  // gpe_cholesky workspace

  int* dinfo = nullptr;
  double* dinvdelta = nullptr;
  double* dZ = nullptr;      // n_pad x max(SK_PMAX, q + 1)
  double* dR2 = nullptr;     // n_pad x max(SK_PMAX, q + 1)
  double* dWa = nullptr;     // n_pad x max(SK_PMAX, q + 1)
  double* dskp = nullptr;    // skinny partials
  size_t skp_cap = 0;
  double* dgpart = nullptr;  // gram partials
  double* dgram = nullptr;   // P^2 (P = q + 1 basis columns)
  double* dT2 = nullptr;     // P^2
  double* dcpart = nullptr;  // contraction partials
  size_t cpart_cap = 0;
  size_t invd_cap = 0, csum_cap = 0, gram_cap = 0, t2_cap = 0;   // dinvdelta (d), dcsum (d + 3), dgram, dT2 (P^2)
  double* dcsum = nullptr;   // d+3
  GemmProb* dprobs = nullptr;
  unsigned* dtiles = nullptr;    // tile lists: training plan [0, cap/2), aux plan [cap/2, cap)
  size_t tiles_cap = 0;

  // posterior workspace
  double* dW1 = nullptr;
  double* dW2 = nullptr;
  size_t w1_cap = 0, w2_cap = 0;
  double* dW3 = nullptr;     // full posterior covariance
  size_t w3_cap = 0;
  double* dXs = nullptr;
  double* dXsw = nullptr;
  size_t xs_cap = 0, xsw_cap = 0;
  double* dsmall = nullptr;  // generic small device scratch
  double* dtiny = nullptr;   // n <= 128 path: X's image, W, the helpers' partials
  int tiny_ek = 0, tiny_eg = 0;   // k_tiny's call ordinals (its sync words in dinfo[1..4])
  bool tiny_dirty = true;         // zero dinfo[1..5] before the next k_tiny
  double* dsnb = nullptr;         // 2-4 tiles (k_snb): X^T, [f H]^T, Z^T, W, T2, scratch, partials
  long long snb_np = 0;
  int snb_hc = 0, snb_mf = 0;   // k_snb's counters (dinfo[8..9]; abort dinfo[10])
  bool snb_dirty = true;
  double onel_tag = 0.0;          // the one-launch objectives' call tag (never repeats)
  // the objective's A^-1 on the int8 matrix cores (gpemu_ozaki.hpp): GPEMU_OZAKI=0 keeps the
  // fp64 LAUUM; GPEMU_OZAKI_MODULI sets the number of moduli (default 16: 53-bit operands)
  int oz_on = 1, oz_nmod = OZ_MAXMOD;
  int oz_min_np = 6144;           // OZ_MIN_NP (GPEMU_OZAKI_MIN_NP)
  int oz_np2 = 0, oz_list_len = 0;
  long long oz_npad = 0;          // the n_pad the cached plan (oz_tri, the lists, oz_c) was made for
  OzConst oz_c{};
  int8_t* dozp = nullptr;         // the N int8 planes of X (lower 256-column panels)
  int8_t* dozr = nullptr;         // the N residue bytes of every lower 256-tile entry
  int* dozx = nullptr;            // per-column exponents
  // the 15-moduli certificate of the objective's products (gpemu_ozaki.hpp; GPEMU_OZAKI_CERT=0:
  // 16 moduli everywhere; only where the context runs 16): the operands' row sums beside dozx
  // (same indices, same lifetime), one flag per product of an evaluation, the 15-moduli constants.
  // From n_pad oz_cert_min_np (GPEMU_OZAKI_CERT_MIN_NP, default OZ_CERT_MIN_NP; tests lower it to 512)
  int oz_cert_on = 1, oz_cert_min_np = OZ_CERT_MIN_NP;
  unsigned long long* dozs = nullptr;
  int* dozf = nullptr;
  unsigned long long* dozm = nullptr;   // per flag: A = max s_a, B = max s_b (gpe_oz_cert_sums)
  int oz_flag_cap = 0, oz_cert_used = 0;   // flags: allocated, taken by the last evaluation's products
  OzConst oz_c15{};
  std::vector<std::pair<int, double>> oz_cert_ops;   // profiling: a product's flag and its int8 ops
  unsigned* dozl = nullptr;       // k_oz_gemm's tile lists (the LAUUM's, then every TRTRI pair's)
  double* dozt = nullptr;         // the TRTRI pairs' T = L21 X11
  hipEvent_t ev_oz = nullptr;     // the first int8 TRTRI pair's L21 planes are ready (stream2)
  std::vector<OzTriPair> oz_tri;  // the TRTRI pairs on the int8 cores
  int oz_tri_min = 8192;          // rows of a TRTRI level's blocks from which it runs there
  double oz_lauum_ops = 0.0;      // int8 ops of the LAUUM product (every modulus)
  // the objective's Cholesky split at tile column h (the top TRTRI pair's), its Schur
  // complement S = A22 - L21 L21^T one int8 product (chol_schur).  oz_chol: 0 off
  // (GPEMU_OZAKI_CHOL=0), 1 the gradient evaluations, 2 the value-only ones too, 3 also
  // gpe_factor's sweep (tests: the only way to read a split sweep's L out again); from
  // oz_chol_min rows of S (GPEMU_OZAKI_CHOL_MIN)
  int oz_chol = 1, oz_chol_min = OZ_CHOL_MIN;
  // gradient evaluations with the split sweep: X11 = L11^-1 (the TRTRI's pairs inside [0, h))
  // and the top pair's T = L21 X11 on the context stream beside the sweep's second phase
  // (tri_ahead; GPEMU_TRTRI_AHEAD=0: after the sweep, as every other caller)
  int tri_ahead_on = 1;
  hipEvent_t ev_l11 = nullptr, ev_schur = nullptr;   // L11 is final / chol_schur is through (the sweep's stream)
  OzTriPair oz_chol_q{};          // the pair (0, h, NB): L21's planes and exponents as the TRTRI's
  long long oz_chol_loff = 0;     // the lower tile list of S in dozl
  int oz_chol_llen = 0;
  double oz_chol_ops = 0.0;
  bool oz_chol_ready = false;     // oz_chol_q and the list are planned for this n_pad
  // the split sweep's first phase split once more at q = h / 2, the trapezoid's update by the
  // columns [0, q) a second int8 product (OzCholNest, chol_schur at q).  oz_nest: 0 off
  // (GPEMU_OZAKI_CHOL_NEST=0: the two-phase sweep); on only with the split itself, for the
  // gradient evaluations (and gpe_factor's sweep under oz_chol 3), from oz_nest_min rows of the
  // trapezoid (GPEMU_OZAKI_CHOL_NEST_MIN)
  int oz_nest = 1, oz_nest_min = OZ_CHOL_NEST_MIN;
  OzCholNest oz_nest_q{};         // its plan, the list in dozl and its int8 operations
  long long oz_nest_loff = 0;
  int oz_nest_llen = 0;
  double oz_nest_ops = 0.0;
  bool oz_nest_ready = false;
  // dozp / dozx[0, Pb) hold L21's planes and exponents of the resident factor (written by
  // chol_schur; cleared by everything else that writes them and by gpe_set_data)
  bool oz_l21_valid = false;
  // profiling (gpe_ozaki_stats): events around the k_oz_gemm launches of the last objective
  std::vector<hipEvent_t> oev;
  size_t oev_used = 0;
  double oz_ms = 0.0, oz_launches = 0.0, oz_ops = 0.0, oz_flops64 = 0.0;
  int dbg_skip_wait = -1;         // GPEMU_DEBUG_SKIP_WAIT (tests): a helper gives up its first wait
  size_t small_cap = 0;

  // pinned host staging
  double* hpin = nullptr;
  size_t hpin_cap = 0;

  // fp32 posterior (precision 32): copy of L^-1 and per-chunk K*, V
  float* dX32 = nullptr;
  size_t x32_cap = 0;
  bool x32_valid = false;
  float* dK32 = nullptr;
  size_t k32_cap = 0;
  hipEvent_t ev_pipe[2] = {nullptr, nullptr};   // the diagonal posterior's chunk pipeline
  // posterior V = L^-1 K* on the int8 cores (posterior_oz): planes of L^-1's rows and their
  // exponents (formed once per factor and moduli count), each chunk's K* planes, exponents
  // and residues, the tile list
  int8_t* dpxp = nullptr;
  int* dpxe = nullptr;
  int8_t* dpkp = nullptr;
  int* dpke = nullptr;
  int8_t* dpres = nullptr;
  unsigned* dpl = nullptr;
  size_t pxp_cap = 0, pxe_cap = 0, pkp_cap = 0, pke_cap = 0, pres_cap = 0, pl_cap = 0;
  int px_nmod = 0, pl_nti = 0, pl_ntj = 0, pl_len = 0;
  bool px_valid = false;

  // sensitivity workspace (gpe_sense_pairs / gpe_gauss_transform)
  double* dSU = nullptr;     // J x n_pad per-point factors
  double* dSZ = nullptr;     // n_pad x p
  double* dSW = nullptr;     // J x d weights
  double* dSpart = nullptr;  // per-wave partials
  double* dSout = nullptr;
  size_t su_cap = 0, sz_cap = 0, sw_cap = 0, spart_cap = 0, sout_cap = 0;

  // noise_fit workspace (gpe_noise_sample): Dnew's r, the draws U^T, L U^T, e, z
  double* dRn = nullptr;
  size_t rn_cap = 0;
  // full posterior covariance beyond one chunk: V = L^-1 K*, scaled points and
  // T Kq^-T for every point, kept until the blocks of the m x m result are formed
  double* dVall = nullptr;
  double* dXall = nullptr;
  double* dTall = nullptr;
  size_t vall_cap = 0, xall_cap = 0, tall_cap = 0;
  double* dNU = nullptr;
  size_t nu_cap = 0;
  // pivoted Cholesky of the posterior covariance (gpe_posterior_pivchol): the state, pivots,
  // variances, d, flags and partials in one buffer; the panel W (m_pad x 128), then L (m x k)
  double* dPc = nullptr;
  double* dPcL = nullptr;
  size_t pc_cap = 0, pcl_cap = 0;
  // integrated-variance design (gpe_posterior_imse): the state, outputs, d, lambda, w, flags and
  // partials in one buffer; C (the reference x candidate cross-covariance); the panel W is dPcL
  double* dIm = nullptr;
  double* dImC = nullptr;
  size_t im_cap = 0, imc_cap = 0;
  // gradient of the posterior (gpe_posterior_grad): the chunk's basis and its derivative, tau,
  // Q^-1, beta, hdim, the results, k_post_grad's partial sums and G padded to the GEMM's K step
  double* dPg = nullptr;
  size_t pg_cap = 0;
  // the posterior mean alone (gpe_posterior_mean): k_post_mean's segment sums and the chunk's
  // result; the points of a chunk (GPEMU_MEAN_CHUNK, a multiple of 128)
  double* dPm = nullptr;
  size_t pm_cap = 0;
  long long mean_chunk = 65536;
  // p outputs on the resident data (gpe_set_outputs; 0: none): [F H] (n_pad x (p + q),
  // column-major), its images Z, R2 and W of the multi-output objective (as dZ, dR2, dWa for
  // [f H]; the first p columns of dWm are Gamma for gpe_posterior_mean_multi), and
  // k_post_mean_multi's segment sums and chunk result
  int mo_p = 0;
  double* dFm = nullptr;
  double* dZm = nullptr;
  double* dR2m = nullptr;
  double* dWm = nullptr;
  size_t fm_cap = 0, zm_cap = 0, r2m_cap = 0, wm_cap = 0;
  double* dPmm = nullptr;
  size_t pmm_cap = 0;
  // the covariance inside groups (gpe_posterior_groups): k_post_groupgram's segment sums
  double* dPgc = nullptr;
  size_t pgc_cap = 0;

  // resident factor (gpe_factor)
  bool factor_valid = false;
  bool linv_valid = false;   // tr.B holds L^-1 (TRTRI of the resident L; run on demand)
  bool zaug_valid = false;   // tr.Faug holds (L^-1 [f H])^T from the last factorisation
  bool ainv_valid = false;   // tr.A holds A^-1 (LAUUM of the resident L^-1)
  int f_kernel = 0;
  std::vector<double> f_delta;
  double f_nu = 0.0;
  double f_rscale = 0.0;     // coefficient of diag(r) in the resident A (gpe_loo takes it out again)

  // how the fused Cholesky is cut into launches: per step and by column groups, the group
  // widths, the super-blocks (GPEMU_POTRF, GPEMU_GROUP_P0, GPEMU_GROUP_STRIDE, GPEMU_POTRF_W,
  // GPEMU_POTRF_SB; gpemu_chol_sched.hpp)
  CholSchedParams sched;
  // 0 auto: group launches while this is the only objective evaluation in flight on the
  // device, one launch per step when others run beside it (their tiles fill the per-step
  // drains, and the group launches' waiting chain tiles would hold slots they could use);
  // 1 always group (GPEMU_POTRF=group), 2 always per step (GPEMU_POTRF=fused)
  int potrf_mode = 0;
  // the fused Cholesky on the context's high-priority stream (default 1; 0: on the
  // context stream, GPEMU_CHOL_PRIO=0)
  int chol_prio = 1;
  // n <= 128: the objective in one one-workgroup launch (gpemu_tiny.hpp; GPEMU_TINY=0 off)
  bool tiny = true;
  hipStream_t stream2 = nullptr;   // the high-priority stream
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_host = nullptr;   // host-visible results of the value part are in hpin

  // profiling
  bool prof = false;
  hipEvent_t ev[16] = {};
  std::vector<hipEvent_t> gev;  // pool of event pairs around GEMM launches
  size_t gev_used = 0;
  double phase_ms[8] = {0};
  double gemm_ms = 0.0, gemm_launches = 0.0, gemm_flops = 0.0;
};

namespace {

#define HIPCHK(ctx, expr)                                                          \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) {                                                        \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);              \
      return GPE_ERR_HIP;                                                          \
    }                                                                              \
  } while (0)

#define CHK(expr)                    \
  do {                               \
    int rc_ = (expr);                \
    if (rc_ != GPE_OK) return rc_;   \
  } while (0)

int fail(gpe_ctx* c, int code, const std::string& msg) {
  c->err = msg;
  return code;
}

// the device allocator of realloc_buf / grow_to (gpemu_host_alloc.hpp)
struct HipAlloc {
  int malloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
  void free(void* p) { (void)hipFree(p); }
};

int alloc_failed(gpe_ctx* c, int e, size_t bytes) {
  return fail(c, GPE_ERR_ALLOC, std::string("hipMalloc failed: ") + hipGetErrorString((hipError_t)e) + " (" +
                                    std::to_string(bytes) + " bytes)");
}

// replace *p by a fresh buffer of count elements (contents not kept; NULL on failure)
template <typename T>
int dalloc(gpe_ctx* c, T** p, size_t count) {
  HipAlloc al;
  const int e = realloc_buf(al, p, count);
  return e ? alloc_failed(c, e, count * sizeof(T)) : GPE_OK;
}

// grow a device buffer to at least need elements (contents not kept): the one way the
// context's buffers grow (grow_to: a failed allocation leaves no stale capacity behind)
template <class T>
int grow_buf(gpe_ctx* c, T** p, size_t* cap, size_t need) {
  HipAlloc al;
  const int e = grow_to(al, p, cap, need);
  return e ? alloc_failed(c, e, need * sizeof(T)) : GPE_OK;
}

// the per-dimension and per-basis-column device buffers, grown to the shape in use: the
// reference takes any d and any basis (_emulatorkernels.py:39-50), and so does the library
// (d > 32 and P > 33 run the LDS-staged wide kernels)
int ensure_shape_bufs(gpe_ctx* c, int d, int P) {
  CHK(grow_buf(c, &c->dinvdelta, &c->invd_cap, (size_t)d));
  CHK(grow_buf(c, &c->dcsum, &c->csum_cap, (size_t)d + 3));
  CHK(grow_buf(c, &c->dgram, &c->gram_cap, (size_t)P * P));
  CHK(grow_buf(c, &c->dT2, &c->t2_cap, (size_t)P * P));
  return GPE_OK;
}

int ensure_pinned(gpe_ctx* c, size_t doubles) {
  if (doubles <= c->hpin_cap) return GPE_OK;
  if (c->hpin) hipHostFree(c->hpin);
  c->hpin = nullptr;
  size_t cap = std::max<size_t>(doubles, 1 << 16);
  HIPCHK(c, hipHostMalloc((void**)&c->hpin, cap * sizeof(double), hipHostMallocDefault));
  c->hpin_cap = cap;
  return GPE_OK;
}

int ensure_small(gpe_ctx* c, size_t doubles) {
  return grow_buf(c, &c->dsmall, &c->small_cap, doubles);
}

// ------------------------------------------------------------------ launches
// f(std::integral_constant<int, FAM>()) for the correlation family fam (a FAM_*; any other
// value runs FAM_GAUSS, the kernels as they were before the Matern families): the one place
// where a run-time family becomes a kernel's template argument
template <class F>
static void with_fam(int fam, F&& f) {
  if (fam == FAM_MATERN32) f(std::integral_constant<int, FAM_MATERN32>());
  else if (fam == FAM_MATERN52) f(std::integral_constant<int, FAM_MATERN52>());
  else f(std::integral_constant<int, FAM_GAUSS>());
}

// The register widths (DMAX) the kernels are instantiated for: the pair kernel's, and those of
// the one-launch objectives and the fused posterior kernels (their d > 32 has a wide instance
// of its own, chosen by the launcher).
// (Widest first: the compiler emits the instances of a list's last width first, and the code
// object keeps them in ascending order, as the chains of `d <= W` this replaces left them.)
using PairWidths = std::integer_sequence<int, 32, 24, 20, 16, 12, 10, 8, 6, 4, 2>;
using RegWidths = std::integer_sequence<int, 32, 16, 12, 8, 4>;
// f(std::integral_constant<int, W>()) for the smallest W of the list with d <= W (zero-padded
// dimensions cost one FMA each), the widest beyond it: the one place where a run-time input
// width becomes a kernel's template argument
template <int... Ws, class F>
static void with_width(std::integer_sequence<int, Ws...>, int d, F&& f) {
  int w = std::max({Ws...});
  ((w = d <= Ws && Ws < w ? Ws : w), ...);
  (void)((w == Ws && (f(std::integral_constant<int, Ws>()), true)) || ...);
}

// k_tiny<DM, FAM> / k_snb<DM, FAM> for the padded width DM >= d of the one-launch kernels
template <int FAM>
static void launch_tiny_fam(int d, size_t lds, hipStream_t st, const TinyArgs& a) {
  const dim3 g(1 + TINY_NH), b(256);
  with_width(RegWidths(), d, [&](auto W) { hipLaunchKernelGGL((k_tiny<decltype(W)::value, FAM>), g, b, lds, st, a); });
}
template <int FAM>
static void launch_snb_fam(int d, size_t lds, hipStream_t st, const SnbArgs& a) {
  const dim3 g(1 + SNB_NH), b(256);
  with_width(RegWidths(), d, [&](auto W) { hipLaunchKernelGGL((k_snb<decltype(W)::value, FAM>), g, b, lds, st, a); });
}
// the dynamic LDS sizes of every width of one family's k_tiny and k_snb
template <int FAM, int... Ws>
static bool onel_lds_attr(std::integer_sequence<int, Ws...>, int tiny_bytes, int snb_bytes) {
  const auto at = hipFuncAttributeMaxDynamicSharedMemorySize;
  return ((hipFuncSetAttribute((const void*)k_tiny<Ws, FAM>, at, tiny_bytes) == hipSuccess) && ...) &&
         ((hipFuncSetAttribute((const void*)k_snb<Ws, FAM>, at, snb_bytes) == hipSuccess) && ...);
}

int launch_pairs(gpe_ctx* c, const PairArgs& a, int nblocks) {
  if (a.fam != FAM_GAUSS && a.fam != FAM_MATERN32 && a.fam != FAM_MATERN52)
    return fail(c, GPE_ERR_ARG, "internal error: bad correlation family");
  if (a.d > 32) {   // any d: coordinates staged through LDS in chunks of 32
    const dim3 g(nblocks), b(256);
    with_fam(a.fam, [&](auto F) { hipLaunchKernelGGL(k_pairs_wide<decltype(F)::value>, g, b, 0, c->stream, a); });
    HIPCHK(c, hipGetLastError());
    return GPE_OK;
  }
  // launches of few tiles (small n) split each tile's columns over up to 4 workgroups
  // (same values: every entry is computed as before, by another workgroup)
  PairArgs a2 = a;
  while (a2.csplit < 4 && nblocks * a2.csplit * 2 <= 512) a2.csplit *= 2;
  const dim3 g(nblocks * a2.csplit), b(256);
  with_fam(a.fam, [&](auto F) {
    with_width(PairWidths(), a.d, [&](auto W) {
      hipLaunchKernelGGL((k_pairs<decltype(W)::value, decltype(F)::value>), g, b, 0, c->stream, a2);
    });
  });
  HIPCHK(c, hipGetLastError());
  return GPE_OK;
}

// The gradient contraction of gpe_objective for one correlation family: k_contract<.., FAM>
// by bucket of d and the P columns of W (q + 1; p + q for p outputs), k_contract_wide<FAM> beyond
// the register-resident sizes.
template <int FAM>
static void launch_contract(gpe_ctx* c, int d, int P, dim3 gc, int nblk, const double* rdiag, int cs, const double* Wa) {
  const long long np = c->n_pad;
  const int bucket = std::max(d, P);
  if (d > 32 || P > 33) {   // any d and q: staged through LDS in chunks of 32
    hipLaunchKernelGGL(k_contract_wide<FAM>, dim3(nblk), dim3(256), 0, c->stream, c->tr.A, np, c->dXw, d, Wa, np, P, (int)c->n, c->dcpart, c->dinfo, 0, 0ll, rdiag);
  } else if (d == 10 && P <= 13) {   // the headline configuration: no padded dimensions
    hipLaunchKernelGGL((k_contract<10, 13, FAM>), gc, dim3(256), 0, c->stream, c->tr.A, np, c->dXw, d, Wa, np, P, (int)c->n, c->dcpart, c->dinfo, 0, 0ll, rdiag, cs);
  } else if (bucket <= 8) {
    hipLaunchKernelGGL((k_contract<8, 9, FAM>), gc, dim3(256), 0, c->stream, c->tr.A, np, c->dXw, d, Wa, np, P, (int)c->n, c->dcpart, c->dinfo, 0, 0ll, rdiag, cs);
  } else if (bucket <= 16) {
    hipLaunchKernelGGL((k_contract<16, 17, FAM>), gc, dim3(256), 0, c->stream, c->tr.A, np, c->dXw, d, Wa, np, P, (int)c->n, c->dcpart, c->dinfo, 0, 0ll, rdiag, cs);
  } else {
    hipLaunchKernelGGL((k_contract<32, 33, FAM>), gc, dim3(256), 0, c->stream, c->tr.A, np, c->dXw, d, Wa, np, P, (int)c->n, c->dcpart, c->dinfo, 0, 0ll, rdiag, cs);
  }
}

int launch_gemm_range(gpe_ctx* c, const GemmLaunch& L, hipStream_t st = nullptr) {
  if (!st) st = c->stream;
  if (c->prof) {
    if (c->gev_used + 2 > c->gev.size()) {
      for (int i = 0; i < 256; ++i) {
        hipEvent_t e;
        HIPCHK(c, hipEventCreate(&e));
        c->gev.push_back(e);
      }
    }
    HIPCHK(c, hipEventRecord(c->gev[c->gev_used], st));
  }
  HIPCHK(c, launch_k_gemm(L, c->dprobs, c->dtiles, c->dinfo, st));
  if (c->prof) {
    HIPCHK(c, hipEventRecord(c->gev[c->gev_used + 1], st));
    c->gev_used += 2;
    c->gemm_launches += 1.0;
    c->gemm_flops += L.flops;
  }
  return GPE_OK;
}

bool oz_use(const gpe_ctx* c);
int oz_chol_split(const gpe_ctx* c, const Fact& F);
int oz_chol_nest_split(const gpe_ctx* c, const Fact& F, int h);

// objective evaluations in flight per device (gpe_objective), for the auto Cholesky schedule
std::atomic<int> g_inflight[64];

struct InflightGuard {
  int dev;
  explicit InflightGuard(int d) : dev(d & 63) { g_inflight[dev].fetch_add(1); }
  ~InflightGuard() { g_inflight[dev].fetch_sub(1); }
};

// GEMMs outside the cached plans: g[i] (k_gemm instance `kind`, every tile of p in the
// implicit order) is a launch of its own and takes descriptor slot + i.  The descriptors are
// uploaded in one copy on the context's stream, then each launch is issued in order, or with
// `out` handed back (out[i]) for a caller that launches later or more than once.  standalone
// (the test and bench GEMMs): a blocking upload and k_gemm's CDEF instance where the problem
// takes it.
struct AdhocGemm { GemmKind kind; GemmProb p; };
int adhoc_gemm(gpe_ctx* c, AdhocSlot slot, const std::vector<AdhocGemm>& g, GemmLaunch* out = nullptr,
               bool standalone = false) {
  std::vector<GemmProb> d;
  std::vector<GemmLaunch> launches;
  for (const AdhocGemm& e : g) {
    GemmLaunch L = begin_launch(e.kind, d);
    push_prob(L, d, e.p, standalone);
    L.first += slot;
    launches.push_back(L);
  }
  if (standalone)
    HIPCHK(c, hipMemcpy(c->dprobs + slot, d.data(), d.size() * sizeof(GemmProb), hipMemcpyHostToDevice));
  else
    HIPCHK(c, hipMemcpyAsync(c->dprobs + slot, d.data(), d.size() * sizeof(GemmProb), hipMemcpyHostToDevice,
                             c->stream));
  for (size_t i = 0; i < g.size(); ++i) {
    if (out) out[i] = launches[i];
    else CHK(launch_gemm_range(c, launches[i]));
  }
  return GPE_OK;
}

// Build the (n_pad-dependent, data-independent) GEMM schedule (build_chol_plan,
// gpemu_chol_sched.hpp) and upload it.
int build_plan(gpe_ctx* c, Fact& F) {
  Plan& pl = F.plan;
  if (pl.n_pad == F.n_pad && pl.a_ptr == F.A && pl.b_ptr == F.B && !pl.launches.empty()) return GPE_OK;
  const FactBufs fb = {F.A, F.B, F.aug ? F.Faug : nullptr, F.n_pad, F.NB, F.flags, F.logdet, F.part, F.tcnt};
  // the training matrix's sweep may be split, and its first phase once more
  const int h = (&F == &c->tr) ? oz_chol_split(c, F) : 0;
  const int q = h ? oz_chol_nest_split(c, F, h) : 0;
  const int limit = (F.desc_base == 0) ? AUX_DESC_BASE : ADHOC_DESC_BASE - AUX_DESC_BASE;
  const bool built = build_chol_plan(pl, fb, c->sched, h, q, limit);
  const bool fits = (int)pl.probs.size() <= limit;
  if (!built || !fits) {
    pl = Plan();   // (not a plan to find cached at the next call)
    return built ? fail(c, GPE_ERR_UNSUPPORTED, "GEMM schedule too large")
                 : fail(c, GPE_ERR_HIP, "internal error: group schedule waits on a later tile");
  }
  for (auto& L : pl.launches) L.first += F.desc_base;
  HIPCHK(c, hipMemcpy(c->dprobs + F.desc_base, pl.probs.data(), pl.probs.size() * sizeof(GemmProb),
                      hipMemcpyHostToDevice));
  // tile lists: each workspace owns half of the list array
  const size_t half = pl.tiles.size() + 1;
  const size_t need = 2 * half;
  const bool regrow = need > c->tiles_cap;
  CHK(grow_buf(c, &c->dtiles, &c->tiles_cap, need));
  if (regrow) {
    // growing invalidates the other plan's uploaded lists: force its rebuild
    Fact& other = (&F == &c->tr) ? c->aux : c->tr;
    other.plan = Plan();
  }
  const size_t base = (F.desc_base == 0) ? 0 : c->tiles_cap / 2;
  if (pl.tiles.size() > c->tiles_cap / 2) return fail(c, GPE_ERR_STATE, "tile list overflow");
  for (auto& L : pl.launches)
    if (L.list >= 0) L.list += (long long)base;
  if (!pl.tiles.empty())
    HIPCHK(c, hipMemcpy(c->dtiles + base, pl.tiles.data(), pl.tiles.size() * sizeof(unsigned),
                        hipMemcpyHostToDevice));
  return GPE_OK;
}

// (re)allocate a workspace for an n_pad x n_pad problem
int ensure_fact(gpe_ctx* c, Fact& F, long long n_pad) {
  const size_t big = (size_t)n_pad * n_pad;
  if (big > F.cap) {
    CHK(dalloc(c, &F.A, 0));
    CHK(dalloc(c, &F.B, 0));
    CHK(dalloc(c, &F.A, big));
    CHK(dalloc(c, &F.B, big));
    F.cap = big;
    F.plan = Plan();
  }
  if (F.n_pad != n_pad) {
    F.n_pad = n_pad;
    F.NB = (int)(n_pad / TILE);
    CHK(dalloc(c, &F.logdet, (size_t)F.NB));
    CHK(dalloc(c, &F.flags, FACT_FLAG_INTS * (size_t)F.NB));
    CHK(dalloc(c, &F.tflags, 2));   // k_trsv_lower: row counter, list ticket
    if (!F.part) {
      CHK(dalloc(c, &F.part, (size_t)SPLIT_SLOTS * TILE * TILE));
      CHK(dalloc(c, &F.tcnt, (size_t)SPLIT_SLOTS));
      HIPCHK(c, hipMemset(F.tcnt, 0, SPLIT_SLOTS * sizeof(int)));
    }
    if (F.aug) CHK(dalloc(c, &F.Faug, (size_t)n_pad * TILE));
    F.plan = Plan();
  }
  return GPE_OK;
}

// scaled points for the training set
int scale_training(gpe_ctx* c, const double* delta) {
  CHK(ensure_pinned(c, (size_t)c->d + 64));
  const int bad = inv_length_scales(delta, c->d, c->hpin);
  if (bad >= 0) return fail(c, GPE_NOT_PD, bad_length_scale(bad));
  HIPCHK(c, hipMemcpyAsync(c->dinvdelta, c->hpin, c->d * sizeof(double), hipMemcpyHostToDevice,
                           c->stream));
  const long long tot = c->n_pad * c->d;
  hipLaunchKernelGGL(k_scale_points, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream,
                     c->dX, c->dinvdelta, c->d, (int)c->n, (int)c->n_pad, c->dXw);
  HIPCHK(c, hipGetLastError());
  return GPE_OK;
}

// K-build of the training matrix into dA (lower tiles)
int kbuild(gpe_ctx* c, int kernel, double nu, double s2, double rscale) {
  PairArgs a;
  a.xr = c->dXw; a.xc = c->dXw; a.out = c->tr.A; a.ld = c->n_pad;
  a.d = c->d; a.nr_valid = (int)c->n; a.nc_valid = (int)c->n;
  a.mt = c->NB; a.nt = c->NB; a.mode = 1 | 2;
  double coff, cdiag;
  kernel_consts(kernel, nu, true, &coff, &cdiag);
  a.s2 = s2; a.coff = coff; a.cdiag = cdiag;
  a.rscale = rscale; a.r = (c->has_r && rscale != 0.0) ? c->dr : nullptr;
  a.fam = kernel_fam(kernel);
  return launch_pairs(c, a, c->NB * (c->NB + 1) / 2);
}

// Right-looking blocked Cholesky, fused: one launch per column step (or per column group,
// Plan::idx); the diagonal tile of each step is factored by the first workgroup of its
// launch and the step's panel tiles follow in-launch (add_sweep, gpemu_chol_sched.hpp).
// Every launcher of a workspace's schedule first makes sure it is built: growing the
// tile-list array for one workspace's plan resets the other's (build_plan), e.g. the
// aux plan of gpe_noise_sample between gpe_factor and a later on-demand TRTRI / LAUUM.
int oz_prepare(gpe_ctx* c, Fact& F);
int chol_schur(gpe_ctx* c, Fact& F, hipStream_t st, bool with_aug, int at);
int trtri(gpe_ctx* c, Fact& F, bool ozaki = false, bool ahead = false);

// split: the objective's sweep of the training matrix, in two phases around the int8 Schur
// complement where the plan has them (Plan::split_h, chol_schur); ahead: the caller inverts
// next, so X11 and the top pair's T start on the context stream while the second phase runs
// on the high-priority one (trtri's ahead)
// nest: with the split, its first phase split once more where the plan has that (Plan::split_q,
// chol_schur at q)
int potrf(gpe_ctx* c, Fact& F, bool with_aug = false, bool split = false, bool ahead = false, bool nest = false) {
  CHK(build_plan(c, F));
  const int hs = split ? F.plan.split_h : 0;
  if (hs) CHK(oz_prepare(c, F));   // (may rebuild the plan: before pl is taken)
  const Plan& pl = F.plan;
  if (hs != (split ? pl.split_h : 0)) return fail(c, GPE_ERR_STATE, "internal error: split plan changed");
  const int qs = (hs && nest) ? pl.split_q : 0;
  const int NB = F.NB;
  // flags, the group schedule's counters and the launches' list tickets start at zero
  HIPCHK(c, hipMemsetAsync(F.flags, 0, FACT_FLAG_INTS * (size_t)NB * sizeof(int), c->stream));
  const bool wa = with_aug && pl.aug;
  const bool tri_ahead = hs && ahead && pl.sides && c->tri_ahead_on && c->chol_prio;
  F.xclear(tri_ahead ? hs : 0);   // the sweep leaves only X's diagonal 16 x 16 blocks (ensure_xdiag)
  const bool grp = c->sched.group &&
                   (c->potrf_mode == 1 || (c->potrf_mode == 0 && g_inflight[c->device & 63].load() <= 1));
  const std::vector<int>& fidx = pl.steps(qs ? SWEEP_NESTED : hs ? SWEEP_SPLIT : SWEEP_WHOLE, grp, wa);
  if (c->chol_prio) {
    // the whole sweep on the context's high-priority stream: with two tries in flight
    // its chain workgroups are dispatched ahead of the other try's inverse tiles
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    for (int t = 0; t < NB; ++t) {
      if (qs && t == qs) CHK(chol_schur(c, F, c->stream2, wa, qs));
      if (hs && t == hs) {
        if (tri_ahead) HIPCHK(c, hipEventRecord(c->ev_l11, c->stream2));
        CHK(chol_schur(c, F, c->stream2, wa, hs));
        if (tri_ahead) {
          HIPCHK(c, hipEventRecord(c->ev_schur, c->stream2));
          CHK(trtri(c, F, true, true));
        }
      }
      if (fidx[t] >= 0) CHK(launch_gemm_range(c, pl.launches[fidx[t]], c->stream2));
    }
    HIPCHK(c, hipEventRecord(c->ev_join, c->stream2));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    return GPE_OK;
  }
#ifdef GEMM_TTRACE
  if (const char* es = std::getenv("GPEMU_DEBUG_STOP_STEP")) {
    const int stop = std::atoi(es);
    // back to back as in the sweep, every launch traced (the host resets the count)
    for (int t = 0; t <= stop && t < NB; ++t)
      if (fidx[t] >= 0) CHK(launch_gemm_range(c, pl.launches[fidx[t]]));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return fail(c, GPE_ERR_STATE, "debug stop after Cholesky launch " + std::to_string(stop));
  }
#endif
  for (int t = 0; t < NB; ++t) {
    if (qs && t == qs) CHK(chol_schur(c, F, c->stream, wa, qs));
    if (hs && t == hs) CHK(chol_schur(c, F, c->stream, wa, hs));
    if (fidx[t] >= 0) CHK(launch_gemm_range(c, pl.launches[fidx[t]]));
  }
  return GPE_OK;
}

void ev_rec(gpe_ctx* c, int i);

// A^-1 = X^T X over L (the plan's LAUUM launch)
int lauum(gpe_ctx* c, Fact& F) {
  CHK(build_plan(c, F));
  return launch_gemm_range(c, F.plan.launches[F.plan.lauum]);
}

// the full diagonal-tile inverses X_tt in B (k_xasm) after a sweep: the TRTRI's leaves and
// the forward substitution's D_t.  side: -1 every tile, else the tiles on that side of the
// sweep's column F.xh (0: [0, xh), 1: [xh, NB))
int ensure_xdiag(gpe_ctx* c, Fact& F, int side = -1) {
  const bool want0 = side != 1 && !F.xdone[0], want1 = side != 0 && !F.xdone[1];
  const int a = want0 ? 0 : F.xh, b = want1 ? F.NB : F.xh;   // (the tiles still due are one range)
  if (b > a) {
    const long long off = (long long)a * TILE * (F.n_pad + 1);
    hipLaunchKernelGGL(k_xasm, dim3(b - a), dim3(256), DB_LDS_DOUBLES * sizeof(double), c->stream, F.A + off, F.B + off,
                       (long long)F.n_pad);
    HIPCHK(c, hipGetLastError());
  }
  F.xdone[0] = F.xdone[0] || want0;
  F.xdone[1] = F.xdone[1] || want1;
  return GPE_OK;
}

int trtri_pair_ozaki(gpe_ctx* c, Fact& F, int t0, int h, int t1, int l21, int part = 0);
int oz_l21_ahead(gpe_ctx* c, Fact& F, int t0, int h, int t1);
bool oz_tri_level(const gpe_ctx* c, const std::vector<std::array<int, 3>>& prs);

// X = L^-1 by levels; with ozaki (the objective's gradient) the levels whose blocks are at
// least oz_tri_min rows run their two products on the int8 matrix cores (trtri_pair_ozaki).
// ahead (potrf, between the phases of the split sweep at column hs, which goes on on the
// high-priority stream): on the context stream, from L11 final on (ev_l11), X11 -- the levels
// below the top one over the pairs inside [0, hs) -- and, once chol_schur is through (ev_schur:
// the int8 buffers are free, L21's planes there), the top pair's T = L21 X11, unless a pair
// inside [hs, NB) runs on the int8 cores too and would write over T's scratch block.
// After such a sweep (F.x11) the call that follows does what is left: the pairs inside
// [hs, NB), then the top pair or its second product.  The operations and their operands are
// those of the whole TRTRI after the sweep: the same X, bit for bit.
int trtri(gpe_ctx* c, Fact& F, bool ozaki, bool ahead) {
  CHK(build_plan(c, F));
  const Plan& pl = F.plan;
  const int hs = pl.split_h;
  const bool rest = !ahead && F.x11 > 0 && pl.sides && F.x11 == hs && F.xh == hs;
  if (ahead && !(pl.sides && F.xh == hs)) return fail(c, GPE_ERR_STATE, "internal error: TRTRI by side without its plan");
  const int side = ahead ? 0 : (rest ? 1 : -1);   // of the levels below the top one (-1: whole levels)
  const auto is_top = [&](size_t lv) { return side >= 0 && pl.tri_pairs[lv][0][0] < hs && pl.tri_pairs[lv][0][2] > hs; };
  const auto pairs_of = [&](size_t lv, int sd) {
    return (sd < 0 || is_top(lv)) ? pl.tri_pairs[lv] : trtri_side_pairs(pl.tri_pairs[lv], hs, sd);
  };
  const auto int8_level = [&](size_t lv) { return ozaki && oz_tri_level(c, pl.tri_pairs[lv]); };
  // int8 pairs inside [0, hs) / [hs, NB), and the top level there
  bool int8_side[2] = {false, false}, int8_top = false;
  for (size_t lv = 0; lv < pl.tri_pairs.size() && side >= 0; ++lv) {
    if (!int8_level(lv)) continue;
    if (is_top(lv)) int8_top = true;
    else for (int sd = 0; sd < 2; ++sd) int8_side[sd] = int8_side[sd] || !pairs_of(lv, sd).empty();
  }
  if (ahead) HIPCHK(c, hipStreamWaitEvent(c->stream, int8_side[0] ? c->ev_schur : c->ev_l11, 0));
  CHK(ensure_xdiag(c, F, side));
  // the first int8 pair's L21 (final since the Cholesky) is converted on the second stream
  // while the fp64 levels below it run (not ahead: the sweep is on that stream)
  int first = -1;
  for (size_t lv = 0; lv < pl.tri_pairs.size() && !ahead && first < 0; ++lv)
    if (int8_level(lv) && !pairs_of(lv, side).empty() && !(is_top(lv) && F.t_ahead)) first = (int)lv;
  // ... unless the split sweep left them (chol_schur) and no int8 level below wrote over them
  bool have = false;
  if (first >= 0) {
    const auto pr = pairs_of((size_t)first, side)[0];
    have = c->oz_l21_valid && &F == &c->tr && hs > 0 && pr[0] == 0 && pr[1] == hs && pr[2] == F.NB;
    if (!have) CHK(oz_l21_ahead(c, F, pr[0], pr[1], pr[2]));
  }
  for (size_t lv = 0; lv < pl.tri_pairs.size(); ++lv) {
    const bool top = is_top(lv);
    if (top && ahead) {
      if (!int8_top || int8_side[1]) break;
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_schur, 0));
      const auto& pr = pl.tri_pairs[lv][0];
      CHK(trtri_pair_ozaki(c, F, pr[0], pr[1], pr[2], c->oz_l21_valid ? 2 : 0, 1));
      F.t_ahead = true;
      break;
    }
    const std::vector<std::array<int, 3>> prs = pairs_of(lv, side);
    if (prs.empty()) continue;
    if (int8_level(lv)) {
      for (size_t i = 0; i < prs.size(); ++i) {
        const auto& pr = prs[i];
        const int l21 = ((int)lv == first && i == 0) ? (have ? 2 : 1) : 0;
        CHK(trtri_pair_ozaki(c, F, pr[0], pr[1], pr[2], l21, (top && F.t_ahead) ? 2 : 0));
      }
      continue;
    }
    const bool whole = side < 0 || top;
    CHK(launch_gemm_range(c, pl.launches[whole ? pl.trtri[2 * lv] : pl.trtri_side[lv][2 * side]]));
    CHK(launch_gemm_range(c, pl.launches[whole ? pl.trtri[2 * lv + 1] : pl.trtri_side[lv][2 * side + 1]]));
  }
  if (ahead) F.x11 = hs;
  return GPE_OK;
}

// Y(0:n_rows, 0:P) = op(M) x R  with M lower-tiled (ld = n_pad) or full
int skinny(gpe_ctx* c, bool transposed, const double* M, long long ldm, int ntr, int nit,
           bool lower, const double* R, long long ldr, int P, double* Y, long long ldy) {
  if (P > SK_PMAX) {   // columns are independent: 32 at a time
    for (int c0 = 0; c0 < P; c0 += SK_PMAX)
      CHK(skinny(c, transposed, M, ldm, ntr, nit, lower, R + (long long)c0 * ldr, ldr, std::min(SK_PMAX, P - c0),
                 Y + (long long)c0 * ldy, ldy));
    return GPE_OK;
  }
  // k chunks of chk tiles: SK_CH, or fewer when the launch has few output tiles (small n:
  // 8 row tiles with one chunk each left 8 workgroups walking all of K, ~35 us at n = 1024)
  const int kext = lower ? std::max(ntr, nit) : ntr;
  const int want = (256 + nit - 1) / nit;   // chunks per output tile for ~256 workgroups
  const int chk = std::max(1, std::min(SK_CH, (kext + want - 1) / want));
  const int nch = (kext + chk - 1) / chk;
  const long long rows = (long long)nit * TILE;
  CHK(grow_buf(c, &c->dskp, &c->skp_cap, (size_t)nch * rows * P));
  SkinnyArgs a;
  a.M = M; a.ldm = ldm; a.R = R; a.ldr = ldr; a.part = c->dskp; a.ldp = rows;
  a.pstride = rows * P; a.P = P; a.ntr = ntr; a.lower = lower ? 1 : 0; a.nit = nit;
  a.abort_flag = c->dinfo;
  a.chk = chk;
  dim3 grid(nit * nch);
  const bool p16 = P <= 16;
  if (!transposed) {
    if (p16) hipLaunchKernelGGL((k_skinny_mfma<16, false>), grid, dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL((k_skinny_mfma<32, false>), grid, dim3(256), 0, c->stream, a);
  } else {
    if (p16) hipLaunchKernelGGL((k_skinny_mfma<16, true>), grid, dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL((k_skinny_mfma<32, true>), grid, dim3(256), 0, c->stream, a);
  }
  HIPCHK(c, hipGetLastError());
  const int mode = lower ? (transposed ? 1 : 0) : 2;
  const long long tot = rows * P;
  // partial layout is [ch][p][rows]; reduce into Y (ld = ldy >= rows)
  if (ldy != rows) return fail(c, GPE_ERR_STATE, "skinny: output ld mismatch");
  hipLaunchKernelGGL(k_reduce_chunks, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream,
                     c->dskp, (long long)(rows * P), Y, rows, P, (int)rows, ntr, mode, c->dinfo, chk);
  HIPCHK(c, hipGetLastError());
  return GPE_OK;
}

// Y = M^T R as skinny(transposed, lower) over the nt x nt tiles of M, and in the same pass
// asq(i) = sum_{i <= k < n_valid} M(k, i)^2: the launch of the first 32 columns carries the
// squares as one more partial column (k_skinny_mfma<., true, true>), so M is read once for
// both; further column chunks are plain skinny products.  Both outputs are sums in a fixed
// order (no atomics): repeated calls give the same bits.
int skinny_t_sq(gpe_ctx* c, const double* M, long long ldm, int nt, long long n_valid, const double* R,
                long long ldr, int P, double* Y, long long ldy, double* asq) {
  const int pc = std::min(SK_PMAX, P);
  const int want = (256 + nt - 1) / nt;   // chunks per output tile for ~256 workgroups (as skinny)
  const int chk = std::max(1, std::min(SK_CH, (nt + want - 1) / want));
  const int nch = (nt + chk - 1) / chk;
  const long long rows = (long long)nt * TILE;
  if (ldy != rows) return fail(c, GPE_ERR_STATE, "skinny: output ld mismatch");
  CHK(grow_buf(c, &c->dskp, &c->skp_cap, (size_t)nch * rows * (pc + 1)));
  SkinnyArgs a;
  a.M = M; a.ldm = ldm; a.R = R; a.ldr = ldr; a.part = c->dskp; a.ldp = rows;
  a.pstride = rows * (pc + 1); a.P = pc; a.ntr = nt; a.lower = 1; a.nit = nt;
  a.abort_flag = c->dinfo;
  a.chk = chk;
  a.n_valid = (int)n_valid;
  dim3 grid(nt * nch);
  if (pc <= 16) hipLaunchKernelGGL((k_skinny_mfma<16, true, true>), grid, dim3(256), 0, c->stream, a);
  else hipLaunchKernelGGL((k_skinny_mfma<32, true, true>), grid, dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_reduce_chunks, dim3((unsigned)((rows * pc + 255) / 256)), dim3(256), 0, c->stream,
                     c->dskp, a.pstride, Y, rows, pc, (int)rows, nt, 1, c->dinfo, chk);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_reduce_chunks, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, c->stream,
                     c->dskp + rows * pc, a.pstride, asq, rows, 1, (int)rows, nt, 1, c->dinfo, chk);
  HIPCHK(c, hipGetLastError());
  if (P > pc)
    CHK(skinny(c, true, M, ldm, nt, nt, true, R + (long long)pc * ldr, ldr, P - pc, Y + (long long)pc * ldy, ldy));
  return GPE_OK;
}

// Y = Z T (Z nrows x P, T P x Pout column-major)
int apply_small(gpe_ctx* c, const double* Z, long long ldz, int P, const double* T, int Pout, double* Y,
                long long ldy, int nrows, const int* abort_flag) {
  const dim3 g((unsigned)((nrows + 255) / 256));
  if (P <= SK_PMAX)
    hipLaunchKernelGGL(k_apply_small, g, dim3(256), 0, c->stream, Z, ldz, P, T, Pout, Y, ldy, nrows, abort_flag);
  else
    hipLaunchKernelGGL(k_apply_big, g, dim3(256), 0, c->stream, Z, ldz, P, T, Pout, Y, ldy, nrows, abort_flag);
  HIPCHK(c, hipGetLastError());
  return GPE_OK;
}

inline int gram_pairs(int P) {
  const int nch = (P + SK_PMAX - 1) / SK_PMAX;
  return nch * (nch + 1) / 2;
}

// G = Z^T Z (P x P) on the host (doubles, row-major == col-major: symmetric)
int gram(gpe_ctx* c, const double* Z, long long ldz, int P, int nrows, double* host_out) {
  const int nblk = (nrows + 255) / 256;
  const size_t need = (size_t)nblk * P * P;
  CHK(ensure_small(c, need + P * P));
  hipLaunchKernelGGL(k_gram, dim3(nblk, gram_pairs(P)), dim3(256), 0, c->stream, Z, ldz, P, nrows, c->dsmall,
                     c->dinfo);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_reduce_rows, dim3(P * P), dim3(256), 0, c->stream, c->dsmall, nblk, P * P,
                     c->dgram);
  HIPCHK(c, hipGetLastError());
  CHK(ensure_pinned(c, (size_t)P * P + 8));
  HIPCHK(c, hipMemcpyAsync(c->hpin, c->dgram, (size_t)P * P * sizeof(double), hipMemcpyDeviceToHost,
                           c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memcpy(host_out, c->hpin, (size_t)P * P * sizeof(double));
  return GPE_OK;
}

// Gram of Z (P x P) into hpin[0, P*P) without waiting; the caller syncs on an event
int gram_async(gpe_ctx* c, const double* Z, long long ldz, int P, int nrows) {
  const int nblk = (nrows + 255) / 256;
  const size_t need = (size_t)nblk * P * P;
  CHK(ensure_small(c, need + P * P));
  hipLaunchKernelGGL(k_gram, dim3(nblk, gram_pairs(P)), dim3(256), 0, c->stream, Z, ldz, P, nrows, c->dsmall,
                     c->dinfo);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_reduce_rows, dim3(P * P), dim3(256), 0, c->stream, c->dsmall, nblk, P * P,
                     c->dgram);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->hpin, c->dgram, (size_t)P * P * sizeof(double), hipMemcpyDeviceToHost,
                           c->stream));
  return GPE_OK;
}

int read_info_logdet(gpe_ctx* c, const Fact& F, int* info, double* logdetA) {
  CHK(ensure_pinned(c, (size_t)F.NB + 8));
  HIPCHK(c, hipMemcpyAsync(c->hpin, F.logdet, F.NB * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->hpin + F.NB, c->dinfo, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memcpy(info, c->hpin + F.NB, sizeof(int));
  if (*info == GEMM_WAIT_TIMEOUT)
    return fail(c, GPE_ERR_HIP, "internal error: Cholesky panel wait timed out");
  double s = 0.0;
  for (int k = 0; k < F.NB; ++k) s += c->hpin[k];
  *logdetA = 2.0 * s;
  return GPE_OK;
}

int check_ready(gpe_ctx* c) {
  if (!c) return GPE_ERR_ARG;
  if (c->n <= 0) return fail(c, GPE_ERR_STATE, "gpe_set_data has not been called");
  HIPCHK(c, hipSetDevice(c->device));
  return GPE_OK;
}

void ev_rec(gpe_ctx* c, int i) {
  if (c->prof) hipEventRecord(c->ev[i], c->stream);
}

// The columns a factorisation carries and solves for: [f H] of gpe_set_data into dZ (the
// default everywhere), or [F H] of gpe_set_outputs into dZm (the multi-output entries)
struct Cols {
  const double* F;
  int P;
  double* Z;
};
int z_from_factor(gpe_ctx* c, const Cols* cols = nullptr, bool cols_in_aug = false);
int trsv_lower(gpe_ctx* c, Fact& F, const double* R, long long ldr, int P, double* Y, long long ldy);

// K-build and Cholesky of the training matrix; with invert, also X = L^-1 (TRTRI) into
// tr.B.  Without it tr.B keeps only the diagonal-tile inverses, which is all the forward
// substitution (trsv_lower) needs: the value-only objective and gpe_beta skip the n^3/3
// flops of the inverse, and the posterior-side entries run it on demand (ensure_linv).
int factor_and_invert(gpe_ctx* c, int kernel, const double* delta, double nu, double s2,
                      double rscale, bool invert = true, bool objective = false, const Cols* cols = nullptr) {
  c->linv_valid = false;
  c->oz_l21_valid = false;
  c->oz_cert_used = 0;   // (every int8 product with a certificate follows from here: its flags from the first)
  c->oz_cert_ops.clear();
  // a call that failed inside the sweep may have left Cholesky launches on the
  // high-priority stream (the join is recorded only after the last one): drain them
  // before this call's memsets and K-build touch the same buffers
  HIPCHK(c, hipStreamSynchronize(c->stream2));
  HIPCHK(c, hipMemsetAsync(c->dinfo, 0, sizeof(int), c->stream));
  CHK(build_plan(c, c->tr));
  ev_rec(c, 0);
  CHK(scale_training(c, delta));
  CHK(kbuild(c, kernel, nu, s2, rscale));
  const int P = cols ? cols->P : c->q + 1;
  // without the inverse (value only, gpe_factor) the sweep carries [f H]^T in the
  // augmented row and leaves L^-1 [f H] there; with it, L^-1 [f H] is one skinny product
  // with L^-1 and the sweep stays lean
  const bool aug = !invert && c->tr.plan.aug && P <= TILE;   // the row holds at most 128 columns
  c->zaug_valid = aug && !cols;   // (other columns in the row are their caller's alone)
  if (aug) {
    const long long tot = c->n_pad * TILE;
    hipLaunchKernelGGL(k_aug_init, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream,
                       cols ? cols->F : c->dF, c->n_pad, P, c->n_pad, c->tr.Faug);
    HIPCHK(c, hipGetLastError());
  }
  ev_rec(c, 1);
  CHK(build_plan(c, c->tr));
  // the objective's sweep may split (its gradient evaluations; the value-only ones when asked)
  // ... and nest with its gradient evaluations (and gpe_factor's sweep under the test switch 3)
  CHK(potrf(c, c->tr, aug, objective && (invert || c->oz_chol >= 2), objective && invert,
            objective && (invert || c->oz_chol == 3)));
  if (kernel_fam(kernel) != FAM_GAUSS) {
    // Matern families: a pivot within the factorisation's backward error of zero is not
    // positive definite (k_pivot_floor).  The Gaussian kernels keep the reference's LAPACK
    // rule alone, to which their not-PD decisions are pinned.
    double coff, cdiag;
    kernel_consts(kernel, nu, true, &coff, &cdiag);
    const double floor_rel = 4.0 * (double)c->n_pad * std::numeric_limits<double>::epsilon();
    const double* r = (c->has_r && rscale != 0.0) ? c->dr : nullptr;
    hipLaunchKernelGGL(k_pivot_floor, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream, c->tr.A,
                       c->n_pad, (int)c->n, floor_rel, s2 * cdiag, r, rscale, c->dinfo);
    HIPCHK(c, hipGetLastError());
  }
  ev_rec(c, 2);
  if (invert) {
    CHK(trtri(c, c->tr, true));   // (only the objective's gradient inverts here)
    c->linv_valid = true;
  }
  CHK(z_from_factor(c, cols, aug));
  ev_rec(c, 3);
  return GPE_OK;
}

// Z = L^-1 [f H] of the resident factor into c->dZ (n_pad x P, column-major): from the
// augmented row when the fused sweep carried it, else as L^-1 times [f H] when L^-1 is
// resident, else by forward substitution
int z_from_factor(gpe_ctx* c, const Cols* cols, bool cols_in_aug) {
  const int P = cols ? cols->P : c->q + 1;
  const double* F = cols ? cols->F : c->dF;
  double* Z = cols ? cols->Z : c->dZ;
  const long long np = c->n_pad;
  if (cols ? cols_in_aug : c->zaug_valid) {
    const long long tot = np * P;
    hipLaunchKernelGGL(k_aug_to_cols, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream,
                       c->tr.Faug, P, np, Z, np);
    HIPCHK(c, hipGetLastError());
    return GPE_OK;
  }
  if (c->linv_valid) return skinny(c, false, c->tr.B, np, c->NB, c->NB, true, F, np, P, Z, np);
  return trsv_lower(c, c->tr, F, np, P, Z, np);
}

// X = L^-1 of the resident factor into tr.B if the factorisation skipped it
int ensure_linv(gpe_ctx* c) {
  if (c->linv_valid) return GPE_OK;
  CHK(trtri(c, c->tr));
  c->linv_valid = true;
  c->x32_valid = false;
  c->px_valid = false;
  return GPE_OK;
}

// Y = L^-1 R (n_pad x P, column-major) from the Cholesky factor in F.A and the diagonal
// inverses in F.B: k_trsv_lower, one launch per TS_PM columns
int trsv_lower(gpe_ctx* c, Fact& F, const double* R, long long ldr, int P, double* Y, long long ldy) {
  CHK(ensure_xdiag(c, F));
  for (int c0 = 0; c0 < P; c0 += TS_PM) {
    const int pc = std::min(TS_PM, P - c0);
    HIPCHK(c, hipMemsetAsync(F.tflags, 0, 2 * sizeof(int), c->stream));   // the row counter and ticket
    hipLaunchKernelGGL(k_trsv_lower, dim3(F.NB), dim3(512), 0, c->stream, F.A, (long long)F.n_pad, F.B,
                       R + (long long)c0 * ldr, ldr, Y + (long long)c0 * ldy, ldy, pc, F.tflags, F.tflags + 1,
                       c->dinfo);
    HIPCHK(c, hipGetLastError());
  }
  return GPE_OK;
}

// ---------------------------------------------------------------- A^-1 on the int8 cores
// (gpemu_ozaki.hpp).  Used by the objective's gradient for OZ_MIN_NP <= n_pad <= OZ_MAX_NP:
// below, the fp64 LAUUM is a few short launches.  At the top, n_pad = 65536 (BASELINE
// configs[3] on one GPU), the K = 65536 sums still fit the int32 accumulators (2^30) and 16
// moduli still give 53-bit operands, and the planes, residues and T scratch take 77 GB beside
// the 69 GB of A and B (of the 288 GB).  The posterior's product keeps OZ_POST_MAX_NP: its
// planes of the whole square L^-1 (N n_pad^2 bytes) would add 69 GB more there.
// The lower ends are where the int8 path starts paying (`profiles/oz_crossover_r06.log`): the
// objective's A^-1 from n_pad 6144 (0.31 against 0.13 ms at 2048, 1.25 against 1.30 at 6144,
// 2.33 against 2.82 at 8192), the posterior's product from 4096 (GPEMU_OZAKI_MIN_NP lowers
// both, for tests).
constexpr int OZ_MIN_NP = 6144, OZ_POST_MIN_NP = 4096, OZ_MAX_NP = 65536, OZ_POST_MAX_NP = 32768;
// every sum here is at most np2 = n_pad rounded up to 256 long (k_oz_gemm's int32 / fp32 bound)
static_assert(OZ_MAX_NP % OZ_T == 0 && OZ_MAX_NP <= OZ_MAX_K && OZ_POST_MAX_NP <= OZ_MAX_K, "int8 sums too long");
bool oz_use(const gpe_ctx* c) { return c->oz_on && c->n_pad >= c->oz_min_np && c->n_pad <= OZ_MAX_NP; }

// The tile column h at which the objective's Cholesky of the training matrix is split (0:
// not split): the largest power of two below NB, the top TRTRI pair's (0, h, NB), so L21's
// planes serve both; only where the int8 path runs at all and S has at least oz_chol_min rows
int oz_chol_split(const gpe_ctx* c, const Fact& F) {
  if (!c->oz_chol || !oz_use(c) || F.n_pad != c->n_pad || F.NB < 2) return 0;
  int h = 1;
  while (2 * h < F.NB) h *= 2;
  return (F.NB - h) * TILE >= c->oz_chol_min ? h : 0;
}

// The tile column q = h / 2 at which the split sweep's first phase is split once more (0: not):
// q even, so the product's sums and the trapezoid's columns are whole 256-tiles, and the
// trapezoid's rows [q, NB) at least oz_nest_min
int oz_chol_nest_split(const gpe_ctx* c, const Fact& F, int h) {
  if (!c->oz_nest || h < 4 || (h / 2) % 2) return 0;
  return (F.NB - h / 2) * TILE >= c->oz_nest_min ? h / 2 : 0;
}

// the TRTRI levels on the int8 cores: every pair of a level whose blocks have at least
// oz_tri_min rows (GPEMU_OZAKI_TRI_MIN; the levels below stay fp64: their products are a
// few short tiles)
bool oz_tri_level(const gpe_ctx* c, const std::vector<std::array<int, 3>>& prs) {
  return oz_use(c) && !prs.empty() && (prs[0][1] - prs[0][0]) * TILE >= c->oz_tri_min;
}

// planes, residues, exponents, scratch and the tile lists (the LAUUM's and every Ozaki
// TRTRI pair's) for this n_pad
int oz_prepare(gpe_ctx* c, Fact& F) {
  const int np2 = (int)(((c->n_pad + OZ_T - 1) / OZ_T) * OZ_T);
  // keyed on n_pad, not np2: two n_pad sharing one np2 (1152 and 1280; 8320 and 8448) have
  // different TRTRI pairs (the last block's t1)
  if (c->n_pad == c->oz_npad && np2 == c->oz_np2 && c->oz_c.nmod == c->oz_nmod) return GPE_OK;
  c->oz_np2 = 0;
  c->oz_npad = 0;
  c->oz_chol_ready = false;
  c->oz_nest_ready = false;
  c->oz_l21_valid = false;
  CHK(build_plan(c, F));
  const int N = c->oz_nmod;
  size_t planes = (size_t)oz_plane_bytes(np2) * N;
  size_t resid = (size_t)oz_lauum_shape(np2).res_bytes() * N;
  size_t scratch = 0, nex = (size_t)np2;
  std::vector<unsigned> all = oz_lauum_shape(np2).list();
  c->oz_list_len = (int)all.size();
  c->oz_lauum_ops = oz_lauum_shape(np2).ops(N);
  c->oz_tri.clear();
  for (const auto& prs : F.plan.tri_pairs) {
    if (!oz_tri_level(c, prs)) continue;
    for (const auto& pr : prs) {
      const OzTriPair q = oz_tri_pair_plan(pr[0], pr[1], pr[2], N, all);
      planes = std::max(planes, q.planes_bytes(N));
      resid = std::max(resid, q.resid_bytes(N));
      scratch = std::max(scratch, (size_t)q.Pa * q.Pb);
      nex = std::max(nex, (size_t)(q.Pa + q.Pb));
      c->oz_tri.push_back(q);
    }
  }
  // the split Cholesky's Schur complement (chol_schur): the top TRTRI pair's plan (its own
  // when that level stays fp64) and the lower tile list of S = L21 L21^T, every sum K = Pa
  if (const int hs = (&F == &c->tr) ? F.plan.split_h : 0) {
    const OzTriPair* have = nullptr;
    for (const OzTriPair& q : c->oz_tri)
      if (q.t0 == 0 && q.h == hs && q.t1 == F.NB) have = &q;
    const OzTriPair q = have ? *have : oz_tri_pair_plan(0, hs, F.NB, N, all);
    const std::vector<unsigned> ls = q.shape_schur().list();
    c->oz_chol_q = q;
    c->oz_chol_loff = (long long)all.size();
    c->oz_chol_llen = (int)ls.size();
    all.insert(all.end(), ls.begin(), ls.end());
    c->oz_chol_ops = q.shape_schur().ops(N);
    planes = std::max(planes, (size_t)N * q.Pb * q.Pa);
    resid = std::max(resid, (size_t)q.shape_schur().res_bytes() * N);
    nex = std::max(nex, (size_t)q.Pb);
    c->oz_chol_ready = true;
    // the nested split's product (OzCholNest): its list after S's
    if (const int qs = F.plan.split_q) {
      const OzCholNest nq = oz_chol_nest_plan(qs, hs, F.NB);
      const std::vector<unsigned> ln = nq.shape().list();
      c->oz_nest_q = nq;
      c->oz_nest_loff = (long long)all.size();
      c->oz_nest_llen = (int)ln.size();
      all.insert(all.end(), ln.begin(), ln.end());
      c->oz_nest_ops = nq.shape().ops(N);
      planes = std::max(planes, nq.planes_bytes(N));
      resid = std::max(resid, nq.resid_bytes(N));
      nex = std::max(nex, (size_t)nq.Pb);
      c->oz_nest_ready = true;
    }
  }
  CHK(dalloc(c, &c->dozp, planes));
  CHK(dalloc(c, &c->dozr, resid));
  CHK(dalloc(c, &c->dozx, nex));
  // a flag per product an evaluation can launch: S, the trapezoid, two per TRTRI pair (the top
  // pair's own when its level stays fp64), the LAUUM
  c->oz_flag_cap = 0;
  c->oz_cert_used = 0;
  if (c->oz_cert_on && N == OZ_MAXMOD && c->n_pad >= c->oz_cert_min_np) {
    const size_t nflag = 2 * c->oz_tri.size() + 8;
    CHK(dalloc(c, &c->dozs, nex));
    CHK(dalloc(c, &c->dozf, nflag));
    CHK(dalloc(c, &c->dozm, 2 * nflag));
    HIPCHK(c, hipMemset(c->dozm, 0, 2 * nflag * sizeof(unsigned long long)));
    HIPCHK(c, hipMemset(c->dozs, 0, nex * sizeof(unsigned long long)));
    HIPCHK(c, hipMemset(c->dozf, 0, nflag * sizeof(int)));
    c->oz_flag_cap = (int)nflag;
    c->oz_c15 = oz_consts_cert(np2);
  }
  CHK(dalloc(c, &c->dozt, scratch));
  CHK(dalloc(c, &c->dozl, all.size()));
  HIPCHK(c, hipMemcpy(c->dozl, all.data(), all.size() * sizeof(unsigned), hipMemcpyHostToDevice));
  c->oz_c = oz_consts(N, np2);   // (beta for sums of length np2: valid for every product here)
  c->oz_np2 = np2;
  c->oz_npad = c->n_pad;
  return GPE_OK;
}

// the certificate of the evaluation's next product (row sums sa[0, na), sb[0, nb) in dozs), or
// none: switched off, fewer than 16 moduli, or no flag left
OzCert oz_cert(gpe_ctx* c, const unsigned long long* sa, int na, const unsigned long long* sb, int nb) {
  if (!c->oz_flag_cap || c->oz_cert_used >= c->oz_flag_cap) return OzCert{};
  const int slot = c->oz_cert_used++;
  return OzCert{sa, na, sb, nb, c->dozf + slot, &c->oz_c15, c->dozm + 2 * slot};
}
// the row sums beside dozx (null: no certificates)
unsigned long long* oz_sums(gpe_ctx* c) { return c->oz_flag_cap ? c->dozs : nullptr; }

// one product (oz_product_launch) on stream st (null: the context's); while profiling, between
// two events of the pool, and counted in gpe_ozaki_stats
int oz_gemm_crt(gpe_ctx* c, const OzConst& k, const OzProduct& p, double ops, double flops64,
                hipStream_t st = nullptr) {
  if (!st) st = c->stream;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (c->prof) {
    while (c->oev_used + 2 > c->oev.size()) {
      hipEvent_t e;
      HIPCHK(c, hipEventCreate(&e));
      c->oev.push_back(e);
    }
    e0 = c->oev[c->oev_used];
    e1 = c->oev[c->oev_used + 1];
  }
  HIPCHK(c, oz_product_launch(st, k, p, e0, e1));
  if (c->prof) {
    c->oev_used += 2;
    c->oz_launches += 1.0;
    c->oz_ops += ops;
    c->oz_flops64 += flops64;
    // (the moduli that ran are known once the flag is read back: objective_phase_times)
    if (p.cert.flag && k.nmod == OZ_MAXMOD) c->oz_cert_ops.emplace_back((int)(p.cert.flag - c->dozf), ops);
  }
  return GPE_OK;
}

// Between the phases of the split sweep (potrf), in its stream order on st: L11 and L21 are
// final, A22 still holds the training matrix's trailing block.  With the augmented row, its
// tiles [h, NB) take the first h columns' update (one fp64 launch); L21's rows go to int8
// planes (as for the top TRTRI pair's first product, which then reuses them: oz_l21_valid);
// S = A22 - L21 L21^T: one product over the lower 256-tiles, K = Pa, and its reconstruction
// subtracted from A22's lower 128-tiles in place.
// at: the split column h, or the nested split's q (Plan::split_q) -- there L's columns [0, q) are
// final over all rows and the same steps update the trapezoid {rows [q, NB), columns [q, h)}: the
// augmented row's tiles [q, h) by the first q columns, the rows [q, NB) of those columns to
// planes, serving as both operands (OzCholNest), the product over the triangle capped at
// column h subtracted in place.  The product at h then converts L21 over those planes.
int chol_schur(gpe_ctx* c, Fact& F, hipStream_t st, bool with_aug, int at) {
  const Plan& pl = F.plan;
  if (at != pl.split_h) {
    const OzCholNest& n = c->oz_nest_q;
    if (!c->oz_nest_ready || at != pl.split_q || n.q != at || n.h != pl.split_h)
      return fail(c, GPE_ERR_STATE, "internal error: nested split Cholesky without an int8 plan");
    if (with_aug) CHK(launch_gemm_range(c, pl.launches[pl.aug_q], st));
    const long long ld = F.n_pad;
    c->oz_l21_valid = false;
    oz_operand(st, c->oz_c, n.src(F.A + (long long)n.q * TILE, ld), n.Pb, n.K, c->dozx, c->dozp, oz_sums(c));
    HIPCHK(c, hipGetLastError());
    const OzShape s = n.shape();
    const OzOpnd l{c->dozp, (long long)n.Pb * n.K, n.K, 0};
    return oz_gemm_crt(c, c->oz_c,
                       OzProduct{s, l, l, c->dozl + c->oz_nest_loff, c->oz_nest_llen, c->dozr, s.res_bytes(),
                                 OzOut{c->dozx, c->dozx, F.A + (long long)n.q * TILE * (ld + 1), ld, n.Rb, n.cols, 1, -1.0, 1},
                                 oz_cert(c, c->dozs, n.Pb, c->dozs, n.Pb)},
                       c->oz_nest_ops, (double)n.cols * (2.0 * n.Rb - n.cols) * n.K, st);
  }
  const OzTriPair& q = c->oz_chol_q;
  if (!c->oz_chol_ready || q.h != pl.split_h) return fail(c, GPE_ERR_STATE, "internal error: split Cholesky without an int8 plan");
  if (with_aug) CHK(launch_gemm_range(c, pl.launches[pl.aug_mid], st));
  const long long ld = F.n_pad;
  oz_operand(st, c->oz_c, q.l21(F.A + (long long)q.h * TILE, ld), q.Pb, q.Pa, c->dozx, c->dozp, oz_sums(c));
  HIPCHK(c, hipGetLastError());
  const OzShape s = q.shape_schur();
  const OzOpnd l21{c->dozp, (long long)q.Pb * q.Pa, q.Pa, 0};
  CHK(oz_gemm_crt(c, c->oz_c,
                  OzProduct{s, l21, l21, c->dozl + c->oz_chol_loff, c->oz_chol_llen, c->dozr, s.res_bytes(),
                            OzOut{c->dozx, c->dozx, F.A + (long long)q.h * TILE * (ld + 1), ld, q.Rb, q.Rb, 1, -1.0, 1},
                            oz_cert(c, c->dozs, q.Pb, c->dozs, q.Pb)},
                  c->oz_chol_ops, (double)q.Rb * q.Rb * q.Ra, st));
  c->oz_l21_valid = true;
  return GPE_OK;
}

// A^-1 = X^T X (lower 128-tiles) of the workspace's X = L^-1 (F.B) into F.A
int lauum_ozaki(gpe_ctx* c, Fact& F) {
  CHK(oz_prepare(c, F));
  const int np = (int)F.n_pad, np2 = c->oz_np2;
  c->oz_l21_valid = false;
  oz_operand_packed(c->stream, c->oz_c, F.B, (long long)F.n_pad, np, np2, c->dozx, c->dozp, oz_sums(c));
  const OzShape s = oz_lauum_shape(np2);
  const OzOpnd x{c->dozp, oz_plane_bytes(np2), 0, np2};
  return oz_gemm_crt(c, c->oz_c,
                     OzProduct{s, x, x, c->dozl, c->oz_list_len, c->dozr, s.res_bytes(),
                               OzOut{c->dozx, c->dozx, F.A, (long long)F.n_pad, np, np, 1, 1.0},
                               oz_cert(c, c->dozs, np2, c->dozs, np2)},
                     c->oz_lauum_ops, (double)np * np * np / 3.0);
}

// the int8 plan of TRTRI pair (t0, h, t1) (oz_prepare)
const OzTriPair* oz_pair(const gpe_ctx* c, int t0, int h, int t1) {
  for (const OzTriPair& q : c->oz_tri)
    if (q.t0 == t0 && q.h == h && q.t1 == t1) return &q;
  return nullptr;
}

// the first product's L21 side (OzTriPair::l21) on stream st
int oz_l21(gpe_ctx* c, Fact& F, const OzTriPair& q, hipStream_t st) {
  c->oz_l21_valid = false;
  oz_operand(st, c->oz_c, q.l21(F.A + (long long)q.h * TILE + (long long)q.t0 * TILE * F.n_pad, F.n_pad), q.Pb, q.Pa,
             c->dozx, c->dozp, oz_sums(c));
  HIPCHK(c, hipGetLastError());
  return GPE_OK;
}

// oz_l21 of a pair on the second stream, forked from the context stream (L is final there)
int oz_l21_ahead(gpe_ctx* c, Fact& F, int t0, int h, int t1) {
  CHK(oz_prepare(c, F));
  const OzTriPair* q = oz_pair(c, t0, h, t1);
  if (!q) return fail(c, GPE_ERR_STATE, "internal error: TRTRI pair without an int8 plan");
  if (!c->ev_oz) HIPCHK(c, hipEventCreateWithFlags(&c->ev_oz, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
  CHK(oz_l21(c, F, *q, c->stream2));
  HIPCHK(c, hipEventRecord(c->ev_oz, c->stream2));
  return GPE_OK;
}

// One pair (t0, h, t1) of a TRTRI level on the int8 cores (oz_tri_pair_launches): L21 from
// A, X11 / X22 / X21 in B, T in the scratch block.  l21: 1 oz_l21_ahead ran, 2 the planes
// are the split sweep's (chol_schur, earlier on this stream), 0 neither.  part: 0 both products,
// 1 the first alone, 2 the second alone (oz_tri_pair_launches).
int trtri_pair_ozaki(gpe_ctx* c, Fact& F, int t0, int h, int t1, int l21, int part) {
  CHK(oz_prepare(c, F));
  const OzTriPair* qp = oz_pair(c, t0, h, t1);
  if (!qp) return fail(c, GPE_ERR_STATE, "internal error: TRTRI pair without an int8 plan");
  const long long ld = F.n_pad;
  auto tile = [&](double* M, int i, int j) { return M + (long long)i * TILE + (long long)j * TILE * ld; };
  if (l21 == 1) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_oz, 0));
  if (part != 1) c->oz_l21_valid = false;   // the second product's planes go over them
  int rc = GPE_OK;
  oz_tri_pair_launches(c->stream, c->oz_c, *qp, c->dozl, tile(F.A, h, t0), tile(F.B, t0, t0), tile(F.B, h, h),
                       tile(F.B, h, t0), ld, c->dozt, c->dozp, c->dozr, c->dozx, l21 != 0,
                       [&](const OzProduct& p, double ops, double fl) {
                         if (rc == GPE_OK) rc = oz_gemm_crt(c, c->oz_c, p, ops, fl);
                       }, part, oz_sums(c),
                       [&](const unsigned long long* sa, int na, const unsigned long long* sb, int nb) {
                         return oz_cert(c, sa, na, sb, nb);
                       });
  CHK(rc);
  HIPCHK(c, hipGetLastError());
  return GPE_OK;
}

}  // namespace

// the look-ahead stream gets the highest priority so the critical-path kernels
// are dispatched ahead of queued trailing-update workgroups
bool create_priority_stream(hipStream_t* st) {
  int lo = 0, hi = 0;
  if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) return false;
  return hipStreamCreateWithPriority(st, hipStreamNonBlocking, hi) == hipSuccess;
}

// =====================================================================  C-ABI
extern "C" {

#ifdef GEMM_TRACE
// dev build only: copy the fused-Cholesky timeline out (8 slots per column step)
int gpe_debug_trace(uint64_t* out, int32_t n) {
  if (n > 8 * 4096) n = 8 * 4096;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(gemm_trace), (size_t)n * 8) == hipSuccess ? 0 : -2;
}
#endif

#ifdef GEMM_TTRACE
// dev build only: copy the per-tile timeline of the last k_gemm launch out (8 slots per
// workgroup: start, C + first stage / panel's inverse seen, K loop done, end, HW_ID,
// XCC_ID, kind, K); GPEMU_DEBUG_STOP_STEP=t ends the objective after Cholesky launch t
int gpe_debug_ttrace(uint64_t* out, int32_t n) {
  if (n > 8 * (int)GEMM_TTRACE_MAX) n = 8 * (int)GEMM_TTRACE_MAX;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(gemm_ttrace), (size_t)n * 8) == hipSuccess ? 0 : -2;
}
// number of workgroups traced since the last reset; reset = 1 zeroes the count and trace
int gpe_debug_ttrace_count(int32_t reset) {
  unsigned n = 0;
  if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(gemm_ttrace_n), sizeof(n)) != hipSuccess) return -2;
  if (reset) {
    const unsigned z = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(gemm_ttrace_n), &z, sizeof(z)) != hipSuccess) return -2;
    void* tt = nullptr;
    if (hipGetSymbolAddress(&tt, HIP_SYMBOL(gemm_ttrace)) != hipSuccess ||
        hipMemset(tt, 0, sizeof(unsigned long long) * 8 * GEMM_TTRACE_MAX) != hipSuccess) return -2;
  }
  return (int)n;
}
#endif

int gpe_abi_version(void) { return GPE_ABI_VERSION; }

#ifndef GPE_SOURCE_HASH
#define GPE_SOURCE_HASH "unknown"
#endif
const char* gpe_build_id(void) { return GPE_SOURCE_HASH; }

int gpe_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int gpe_device_synchronize(int32_t device) {
  if (hipSetDevice(device) != hipSuccess) return GPE_ERR_HIP;
  return hipDeviceSynchronize() == hipSuccess ? GPE_OK : GPE_ERR_HIP;
}

gpe_ctx* gpe_create(int32_t device) {
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    g_create_error = std::string("no HIP device available: ") + hipGetErrorString(e);
    return nullptr;
  }
  if (device < 0 || device >= ndev) {
    g_create_error = "device index out of range";
    return nullptr;
  }
  gpe_ctx* c = new gpe_ctx();
  c->device = device;
  c->aux.desc_base = AUX_DESC_BASE;
  // the training factorisation carries [f H]^T (L^-1 [f H] from the sweep); GPEMU_AUG=0
  // (A/B switch) takes L^-1 [f H] from the forward substitution instead
  {
    const char* ea = std::getenv("GPEMU_AUG");
    c->tr.aug = !(ea && std::string(ea) == "0");
  }
  {
    const char* e2 = std::getenv("GPEMU_POTRF");
    if (e2) {
      const std::string m(e2);
      c->sched.group = m == "group" || m == "auto";
      c->potrf_mode = m == "group" ? 1 : (m == "auto" ? 0 : 2);
    }
    if (const char* eg = std::getenv("GPEMU_GROUP_P0")) c->sched.grp_p0 = std::max(1, std::atoi(eg));
    if (const char* eg = std::getenv("GPEMU_GROUP_STRIDE")) c->sched.grp_stride = std::max(0, std::atoi(eg));
    if (const char* ep = std::getenv("GPEMU_CHOL_PRIO")) c->chol_prio = std::atoi(ep) != 0;
    if (const char* et = std::getenv("GPEMU_TINY")) c->tiny = std::atoi(et) != 0;
    if (const char* ed = std::getenv("GPEMU_DEBUG_SKIP_WAIT")) c->dbg_skip_wait = std::atoi(ed);
    if (const char* em = std::getenv("GPEMU_MEAN_CHUNK")) c->mean_chunk = std::max(1, std::atoi(em) / 128) * 128LL;
    if (const char* eo = std::getenv("GPEMU_OZAKI")) c->oz_on = std::atoi(eo) != 0;
    if (const char* en = std::getenv("GPEMU_OZAKI_MIN_NP")) c->oz_min_np = std::max(512, std::atoi(en));
    if (const char* em = std::getenv("GPEMU_OZAKI_MODULI")) c->oz_nmod = std::max(8, std::min(OZ_MAXMOD, std::atoi(em)));
    if (const char* et = std::getenv("GPEMU_OZAKI_TRI_MIN")) c->oz_tri_min = std::max(512, std::atoi(et));
    if (const char* ec = std::getenv("GPEMU_OZAKI_CHOL")) c->oz_chol = std::max(0, std::min(3, std::atoi(ec)));
    if (const char* ec = std::getenv("GPEMU_OZAKI_CHOL_MIN")) c->oz_chol_min = std::max(256, std::atoi(ec));
    if (const char* ec = std::getenv("GPEMU_OZAKI_CHOL_NEST")) c->oz_nest = std::atoi(ec) != 0;
    if (const char* ec = std::getenv("GPEMU_OZAKI_CHOL_NEST_MIN")) c->oz_nest_min = std::max(256, std::atoi(ec));
    if (const char* ec = std::getenv("GPEMU_OZAKI_CERT")) c->oz_cert_on = std::atoi(ec) != 0;
    if (const char* ec = std::getenv("GPEMU_OZAKI_CERT_MIN_NP")) c->oz_cert_min_np = std::max(512, std::atoi(ec));
    if (const char* ea = std::getenv("GPEMU_TRTRI_AHEAD")) c->tri_ahead_on = std::atoi(ea) != 0;
    if (const char* es = std::getenv("GPEMU_POTRF_SB")) {
      c->sched.sb = std::max(1, std::min(8, std::atoi(es)));
      if (const char* colon = std::strchr(es, ':')) c->sched.sb_min = std::max(0, std::atoi(colon + 1));
    }
    if (const char* e3 = std::getenv("GPEMU_POTRF_W")) {
      c->sched.groups.clear();
      std::string spec(e3);
      size_t pos = 0;
      while (pos < spec.size()) {
        size_t end = spec.find(',', pos);
        if (end == std::string::npos) end = spec.size();
        const std::string item = spec.substr(pos, end - pos);
        const size_t colon = item.find(':');
        const int w = std::atoi(item.substr(0, colon).c_str());
        const int lim = colon == std::string::npos ? 0 : std::atoi(item.substr(colon + 1).c_str());
        if (w >= 1 && w <= 8) c->sched.groups.push_back({w, lim});
        pos = end + 1;
      }
    }
  }
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      !create_priority_stream(&c->stream2) ||
      hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_l11, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_schur, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_host, hipEventDisableTiming) != hipSuccess) {
    g_create_error = "failed to initialise device/stream";
    delete c;
    return nullptr;
  }
  bool ok = dalloc(c, &c->dinfo, 12) == GPE_OK && dalloc(c, &c->dprobs, MAX_PROBS) == GPE_OK &&
            ensure_shape_bufs(c, GPE_MAX_DIMS, GPE_MAX_COLS) == GPE_OK;
  for (int i = 0; i < 16 && ok; ++i) ok = hipEventCreate(&c->ev[i]) == hipSuccess;
  if (ok) {
    const int gl = G_LDS_DOUBLES * (int)sizeof(double);
    ok = hipFuncSetAttribute((const void*)k_gemm<false, false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, gl) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_gemm<true, false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, gl) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_gemm<true, true, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, gl) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_gemm<false, true, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, gl) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_gemm<false, false, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, gl) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_gemm<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, gl) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_gemm<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, gl) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_gemm<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, gl) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_gemm<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, gl) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_gemm<false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, gl) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_xasm, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)(DB_LDS_DOUBLES * sizeof(double))) == hipSuccess;
    const int tl = (G_LDS_LAUNCH_DOUBLES + 2 * TILE * TINY_ZP) * (int)sizeof(double);
    // every family's instances, not one chosen at run time as with_fam does
    const RegWidths w;
    ok = ok && onel_lds_attr<FAM_GAUSS>(w, tl, SNB_LDS_DOUBLES * 8) && onel_lds_attr<FAM_MATERN32>(w, tl, SNB_LDS_DOUBLES * 8) &&
         onel_lds_attr<FAM_MATERN52>(w, tl, SNB_LDS_DOUBLES * 8);
    if (!ok) c->err = "hipFuncSetAttribute(max dynamic LDS) failed";
  }
  if (!ok) {
    g_create_error = c->err;
    gpe_destroy(c);
    return nullptr;
  }
  return c;
}

void gpe_destroy(gpe_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  double* bufs[] = {c->dSU, c->dSZ, c->dSW, c->dSpart, c->dSout,
                    c->dX, c->dXw, c->dF, c->dr, c->tr.A, c->tr.B, c->tr.logdet, c->aux.A, c->aux.B,
                    c->aux.logdet, c->dinvdelta, c->dZ,
                    c->dR2, c->dWa, c->dskp, c->dgpart, c->dgram, c->dT2, c->dcpart, c->dcsum,
                    c->dW1, c->dW2, c->dW3, c->dXs, c->dXsw, c->dsmall, c->dtiny, c->dsnb, c->dRn, c->dNU,
                    c->dVall, c->dXall, c->dTall, c->dPc, c->dPcL, c->dIm, c->dImC, c->dPg, c->dPm, c->dPgc,
                    c->dFm, c->dZm, c->dR2m, c->dWm, c->dPmm};
  for (double* b : bufs)
    if (b) hipFree(b);
  if (c->dinfo) hipFree(c->dinfo);
  if (c->dX32) hipFree(c->dX32);
  if (c->dK32) hipFree(c->dK32);
  for (void* b : {(void*)c->dpxp, (void*)c->dpxe, (void*)c->dpkp, (void*)c->dpke, (void*)c->dpres, (void*)c->dpl})
    if (b) hipFree(b);
  if (c->tr.flags) hipFree(c->tr.flags);
  if (c->aux.flags) hipFree(c->aux.flags);
  for (Fact* F : {&c->tr, &c->aux}) {
    if (F->part) hipFree(F->part);
    if (F->tcnt) hipFree(F->tcnt);
  }
  if (c->tr.tflags) hipFree(c->tr.tflags);
  if (c->dozp) hipFree(c->dozp);
  if (c->dozr) hipFree(c->dozr);
  if (c->dozx) hipFree(c->dozx);
  if (c->dozs) hipFree(c->dozs);
  if (c->dozf) hipFree(c->dozf);
  if (c->dozm) hipFree(c->dozm);
  if (c->dozl) hipFree(c->dozl);
  if (c->dozt) hipFree(c->dozt);
  if (c->ev_oz) hipEventDestroy(c->ev_oz);
  for (hipEvent_t e : c->oev) hipEventDestroy(e);
  if (c->tr.Faug) hipFree(c->tr.Faug);
  if (c->aux.tflags) hipFree(c->aux.tflags);
  if (c->dprobs) hipFree(c->dprobs);
  if (c->dtiles) hipFree(c->dtiles);
  if (c->hpin) hipHostFree(c->hpin);
  for (auto& e : c->ev)
    if (e) hipEventDestroy(e);
  for (auto& e : c->gev) (void)hipEventDestroy(e);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  for (hipEvent_t e : c->ev_pipe)
    if (e) (void)hipEventDestroy(e);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->ev_l11) (void)hipEventDestroy(c->ev_l11);
  if (c->ev_schur) (void)hipEventDestroy(c->ev_schur);
  if (c->ev_host) (void)hipEventDestroy(c->ev_host);
  if (c->stream2) {
    (void)hipStreamSynchronize(c->stream2);
    (void)hipStreamDestroy(c->stream2);
  }
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

const char* gpe_last_error(const gpe_ctx* c) {
  if (!c) return g_create_error.c_str();
  return c->err.c_str();
}

int gpe_set_data(gpe_ctx* c, int64_t n, int32_t d, int32_t q, const double* X, const double* f,
                 const double* H, const double* r) {
  if (!c) return GPE_ERR_ARG;
  if (n <= 0 || d <= 0 || q <= 0 || !X || !f || !H) return fail(c, GPE_ERR_ARG, "bad data arguments");
  if (n > (1LL << 20)) return fail(c, GPE_ERR_UNSUPPORTED, "n too large");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHK(ensure_shape_bufs(c, d, q + 1));
  const long long n_pad = ((n + TILE - 1) / TILE) * TILE;
  const bool resize = (n_pad != c->n_pad) || (d != c->d) || (q != c->q);
  c->n = n; c->d = d; c->q = q; c->n_pad = n_pad; c->NB = (int)(n_pad / TILE);
  c->mo_p = 0;   // (outputs belong to the data they were set for)
  c->factor_valid = false;
  c->ainv_valid = false;
  c->x32_valid = false;
  c->px_valid = false;
  c->zaug_valid = false;
  c->linv_valid = false;
  c->oz_l21_valid = false;
  if (resize) {
    CHK(ensure_fact(c, c->tr, n_pad));
    CHK(dalloc(c, &c->dX, (size_t)n_pad * d));
    CHK(dalloc(c, &c->dXw, (size_t)n_pad * d));
    CHK(dalloc(c, &c->dF, (size_t)n_pad * (q + 1)));
    CHK(dalloc(c, &c->dr, (size_t)n_pad));
    const size_t cols = (size_t)std::max(SK_PMAX, q + 1);
    CHK(dalloc(c, &c->dZ, (size_t)n_pad * cols));
    CHK(dalloc(c, &c->dR2, (size_t)n_pad * cols));
    CHK(dalloc(c, &c->dWa, (size_t)n_pad * cols));
    const size_t cp = (size_t)c->NB * (c->NB + 1) / 2 * (d + 3) * 4;   // (up to 4 per tile: k_contract csplit)
    CHK(dalloc(c, &c->dcpart, cp));
    c->cpart_cap = cp;
  }
  // stage: X (row-major, padded rows 0), F = [f H] column-major, r
  const size_t nx = (size_t)n_pad * d, nf = (size_t)n_pad * (q + 1);
  CHK(ensure_pinned(c, std::max(nx, nf) + n_pad));
  std::memset(c->hpin, 0, nx * sizeof(double));
  std::memcpy(c->hpin, X, (size_t)n * d * sizeof(double));
  HIPCHK(c, hipMemcpy(c->dX, c->hpin, nx * sizeof(double), hipMemcpyHostToDevice));
  std::memset(c->hpin, 0, nf * sizeof(double));
  for (long long i = 0; i < n; ++i) {
    c->hpin[i] = f[i];
    for (int p = 0; p < q; ++p) c->hpin[i + (long long)(p + 1) * n_pad] = H[i * q + p];
  }
  HIPCHK(c, hipMemcpy(c->dF, c->hpin, nf * sizeof(double), hipMemcpyHostToDevice));
  c->has_r = (r != nullptr);
  std::memset(c->hpin, 0, n_pad * sizeof(double));
  if (r) std::memcpy(c->hpin, r, (size_t)n * sizeof(double));
  HIPCHK(c, hipMemcpy(c->dr, c->hpin, n_pad * sizeof(double), hipMemcpyHostToDevice));
  return GPE_OK;
}

int gpe_set_profiling(gpe_ctx* c, int32_t on) {
  if (!c) return GPE_ERR_ARG;
  c->prof = on != 0;
  return GPE_OK;
}

int gpe_phase_times(gpe_ctx* c, double* ms_out, int32_t n) {
  if (!c || !ms_out) return GPE_ERR_ARG;
  for (int i = 0; i < n && i < 8; ++i) ms_out[i] = c->phase_ms[i];
  return GPE_OK;
}

int gpe_ozaki_stats(gpe_ctx* c, double* ms_out, double* launches_out, double* int8_ops_out, double* fp64_flops_out) {
  if (!c) return GPE_ERR_ARG;
  if (ms_out) *ms_out = c->oz_ms;
  if (launches_out) *launches_out = c->oz_launches;
  if (int8_ops_out) *int8_ops_out = c->oz_ops;
  if (fp64_flops_out) *fp64_flops_out = c->oz_flops64;
  return GPE_OK;
}

int gpe_oz_cert_stats(gpe_ctx* c, int32_t* products_out, int32_t* certified_out) {
  if (!c) return GPE_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  int cert = 0;
  if (c->oz_cert_used > 0) {
    std::vector<int> fl((size_t)c->oz_cert_used);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream2));
    HIPCHK(c, hipMemcpy(fl.data(), c->dozf, fl.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (const int f : fl) cert += f != 0;
  }
  if (products_out) *products_out = c->oz_cert_used;
  if (certified_out) *certified_out = cert;
  return GPE_OK;
}

int gpe_oz_cert_sums(gpe_ctx* c, int32_t cap, uint64_t* a_out, uint64_t* b_out) {
  if (!c) return GPE_ERR_ARG;
  if (cap < 0 || (cap > 0 && (!a_out || !b_out))) return fail(c, GPE_ERR_ARG, "gpe_oz_cert_sums: NULL output");
  HIPCHK(c, hipSetDevice(c->device));
  const int n = std::min((int)cap, c->oz_cert_used);
  if (n > 0) {
    std::vector<unsigned long long> m(2 * (size_t)n);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream2));
    HIPCHK(c, hipMemcpy(m.data(), c->dozm, m.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
      a_out[i] = m[2 * (size_t)i];
      b_out[i] = m[2 * (size_t)i + 1];
    }
  }
  return GPE_OK;
}

int gpe_gemm_stats(gpe_ctx* c, double* ms_out, double* launches_out, double* flops_out) {
  if (!c) return GPE_ERR_ARG;
  if (ms_out) *ms_out = c->gemm_ms;
  if (launches_out) *launches_out = c->gemm_launches;
  if (flops_out) *flops_out = c->gemm_flops;
  return GPE_OK;
}

}  // extern "C"

namespace {

// What the two one-launch objectives (tiny_objective, snb_objective) do before their own
// workspace and sync-word bookkeeping: the length scales (as scale_training), the cached state
// an evaluation invalidates, the second stream's drain, the pinned result buffer of `pinned`
// doubles, and the fields TinyArgs and SnbArgs have in common.
template <class Args>
int onel_prologue(gpe_ctx* c, const ObjArgs& o, int kernel, const double* hp, bool want_grad, size_t pinned, Args& a) {
  const int d = c->d;
  const int bad = inv_length_scales(hp, d, a.invd);
  if (bad >= 0) return fail(c, GPE_NOT_PD, bad_length_scale(bad));
  for (int k = d; k < TINY_DM; ++k) a.invd[k] = 0.0;
  c->linv_valid = false;
  c->zaug_valid = false;
  c->tr.xclear();
  HIPCHK(c, hipStreamSynchronize(c->stream2));   // (a failed sweep's leftovers, as factor_and_invert)
  CHK(ensure_pinned(c, pinned));
  a.X = c->dX; a.F = c->dF; a.xw = c->dXw; a.small = c->hpin;
  a.r = (c->has_r && o.rscale != 0.0) ? c->dr : nullptr;
  a.rdiag = (o.gp4ml && !kernel_alt(kernel) && c->has_r) ? c->dr : nullptr;
  a.n = (int)c->n; a.d = d; a.P = c->q + 1; a.want_grad = want_grad ? 1 : 0; a.mucm = o.gp4ml ? 0 : 1;
  a.s2 = o.s2; a.rscale = o.rscale;
  a.dbg_skip = c->dbg_skip_wait;
  a.tag = ++c->onel_tag;
  kernel_consts(kernel, o.nu, true, &a.coff, &a.cdiag);
  // (the Matern families' pivot floor, as factor_and_invert's k_pivot_floor)
  a.floor_rel = 4.0 * (double)c->n_pad * std::numeric_limits<double>::epsilon();
  return GPE_OK;
}

// What they share after the launch: the kernel's outputs are in the pinned buffer r reads
// (OneLaunchResult, gpemu_objective.hpp) once the stream has drained; the host's
// small_from_gram / objective_value / objective_grad (the general path's) give the LLH and
// the gradient.  One profiling phase: the whole evaluation.
int onel_epilogue(gpe_ctx* c, const ObjArgs& o, int kernel, int n_hp, bool want_grad, const OneLaunchResult& r,
                  bool std_r, double* llh_out, double* grad_out, double* sigma2_out) {
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));   // (the kernel wrote its outputs to hpin)
  CHK(r.status(&c->err));   // (on failure the caller's dirty flag stays set: the next call zeroes the sync words)
  const SmallAlgebra sa = small_from_gram(std::vector<double>(r.h, r.h + (size_t)r.P * r.P), r.P);
  if (!sa.ok) return fail(c, GPE_NOT_PD, Q_NOT_PD);
  const ObjValue v = objective_value(sa, r.logdetA(), (double)c->n, c->q, o.gp4ml, o.s2);
  *llh_out = v.llh;
  if (sigma2_out) *sigma2_out = v.sig2;
  if (want_grad) {   // (the device's T2 carries sqrt(cfac))
    // the device's own Cholesky of Q (same arithmetic) refusing a Q the host's accepted
    if (r.q_refused()) return fail(c, GPE_NOT_PD, Q_NOT_PD);
    double red[TINY_DM + 3];
    CHK(r.sums(red, &c->err));
    objective_grad(red, r.d, kernel, o.nu, o.fitnug, o.gp4ml, v.gscale, o.s2, n_hp, grad_out, std_r);
  }
  if (c->prof) {
    ev_rec(c, 7);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[7]);
    for (int i = 0; i < 8; ++i) c->phase_ms[i] = 0.0;
    c->phase_ms[6] = ms;
  }
  return GPE_OK;
}

// The objective of a training set of at most 128 points (gpemu_tiny.hpp): ONE launch of
// k_tiny (workgroup 0: L, X = L^-1, Z, Gram and, with the gradient, the q x q algebra and W;
// nine helper workgroups: the K-build and the contraction of M = A^-1 - W W^T), which
// writes Gram, log|L|, the failed column and the d + 3 sums straight into the pinned host
// buffer (onel_epilogue).  No memset (the sync words count up over the calls; zeroed only
// after a call that did not end cleanly) and no copy.
int tiny_objective(gpe_ctx* c, const ObjArgs& o, int kernel, const double* hp, int n_hp, bool want_grad,
                   double* llh_out, double* grad_out, double* sigma2_out) {
  const int d = c->d, P = c->q + 1;
  TinyArgs a;
  CHK(onel_prologue(c, o, kernel, hp, want_grad, (size_t)P * P + 2 * d + 64 + TINY_NH * 64, a));
  constexpr size_t tiny_doubles = 36 * DB_BS + TILE * 32;
  if (!c->dtiny) CHK(dalloc(c, &c->dtiny, tiny_doubles));
  if (c->tiny_dirty || c->tiny_ek > (1 << 26)) {   // the sync words and the abort flag
    HIPCHK(c, hipMemsetAsync(c->dinfo + 1, 0, (TINY_SYNC_INTS + 1) * sizeof(int), c->stream));
    c->tiny_ek = c->tiny_eg = 0;
    c->tiny_dirty = false;
  }
  ev_rec(c, 0);
  a.L = c->tr.A; a.Xo = c->tr.B; a.Z = c->dZ; a.abort_flag = c->dinfo + 1 + TINY_SYNC_INTS;
  a.K = c->tr.A; a.Xp = c->dtiny; a.Wg = c->dtiny + 36 * DB_BS; a.sync = c->dinfo + 1;
  a.ek = ++c->tiny_ek;
  a.eg = want_grad ? ++c->tiny_eg : c->tiny_eg;
  const size_t lds = (G_LDS_LAUNCH_DOUBLES + 2 * TILE * TINY_ZP) * sizeof(double);
  c->hpin[P * P + 1] = -2.0;   // (workgroup 0 overwrites it on every path; -2: it did not)
  c->tiny_dirty = true;   // (until this call has ended cleanly: its sync words are then consistent)
  with_fam(kernel_fam(kernel), [&](auto F) { launch_tiny_fam<decltype(F)::value>(d, lds, c->stream, a); });
  CHK(onel_epilogue(c, o, kernel, n_hp, want_grad, OneLaunchResult{c->hpin, P, d, 1, TINY_NH, a.tag, "k_tiny"},
                    a.rdiag != nullptr, llh_out, grad_out, sigma2_out));
  c->tiny_dirty = false;
  return GPE_OK;
}

// The objective of 2-4 tiles (128 < n <= 512, gpemu_snb.hpp): ONE launch of k_snb
// (workgroup 0: the diagonal factors, the Gram and the q x q algebra; SNB_NH = 48 helper workgroups:
// K-build, panels and updates with [f H]^T as an augmented row, X = L^-1, W and the
// contraction), outputs straight into the pinned host buffer (onel_epilogue).
int snb_objective(gpe_ctx* c, const ObjArgs& o, int kernel, const double* hp, int n_hp, bool want_grad,
                  double* llh_out, double* grad_out, double* sigma2_out) {
  const int d = c->d, P = c->q + 1, NB = c->NB;
  const long long np = c->n_pad;
  SnbArgs a;
  CHK(onel_prologue(c, o, kernel, hp, want_grad, (size_t)P * P + NB + 2 * d + 64 + SNB_NH * 64, a));
  if (c->snb_np != np) {
    c->snb_np = 0;
    CHK(dalloc(c, &c->dsnb, (size_t)np * np + 3 * 32 * (size_t)np + TINY_DM * TINY_ZP + TILE * TILE));
    c->snb_np = np;
  }
  if (c->snb_dirty || c->snb_hc > (1 << 24)) {
    HIPCHK(c, hipMemsetAsync(c->dinfo + 8, 0, (SNB_SYNC_INTS + 1) * sizeof(int), c->stream));
    c->snb_hc = c->snb_mf = 0;
    c->snb_dirty = false;
  }
  ev_rec(c, 0);
  a.A = c->tr.A; a.Lb = c->tr.B; a.Xt = c->dsnb;
  a.Zt = a.Xt + np * np; a.Zo = a.Zt + 32 * np; a.Wg = a.Zo + 32 * np; a.T2g = a.Wg + 32 * np;
  a.Xscr = a.T2g + TINY_DM * TINY_ZP;
  a.sync = c->dinfo + 8; a.abort_flag = c->dinfo + 8 + SNB_SYNC_INTS;
  a.np = (int)np; a.NB = NB;
  a.hcb = c->snb_hc; a.mfb = c->snb_mf;
  const size_t lds = SNB_LDS_DOUBLES * sizeof(double);
  c->hpin[P * P + NB] = -2.0;   // (workgroup 0 overwrites it on every path; -2: it did not)
  c->snb_dirty = true;   // (until this call has ended cleanly)
  with_fam(kernel_fam(kernel), [&](auto F) { launch_snb_fam<decltype(F)::value>(d, lds, c->stream, a); });
  CHK(onel_epilogue(c, o, kernel, n_hp, want_grad, OneLaunchResult{c->hpin, P, d, NB, SNB_NH, a.tag, "k_snb"},
                    a.rdiag != nullptr, llh_out, grad_out, sigma2_out));
  c->snb_hc += want_grad ? 4 * NB - 1 : 2 * NB;
  c->snb_mf += NB + (want_grad ? 1 : 0);
  c->snb_dirty = false;
  return GPE_OK;
}

// gpe_phase_times / gpe_gemm_stats / gpe_ozaki_stats of a general-path objective call whose
// work is queued (profiling on; nothing otherwise)
int objective_phase_times(gpe_ctx* c) {
  if (!c->prof) return GPE_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float ms;
  // kbuild, cholesky, trtri, inverse (LAUUM), skinny (L^-1 [f H] + Gram), contract
  // (L^-T R2 + the fused contraction), total
  const int pairs[7][2] = {{0, 1}, {1, 2}, {2, 3}, {4, 5}, {3, 4}, {5, 7}, {0, 7}};
  for (int i = 0; i < 7; ++i) {
    ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ev[pairs[i][0]], c->ev[pairs[i][1]]);
    c->phase_ms[i] = ms;
  }
  double g = 0.0;
  for (size_t i = 0; i + 1 < c->gev_used; i += 2) {
    ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->gev[i], c->gev[i + 1]);
    g += ms;
  }
  c->gemm_ms = g;
  g = 0.0;
  for (size_t i = 0; i + 1 < c->oev_used; i += 2) {
    ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->oev[i], c->oev[i + 1]);
    g += ms;
  }
  c->oz_ms = g;
  // the int8 operations that ran: a certified product's sixteenth modulus did not
  if (!c->oz_cert_ops.empty()) {
    std::vector<int> fl((size_t)c->oz_flag_cap);
    HIPCHK(c, hipMemcpy(fl.data(), c->dozf, fl.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (const auto& po : c->oz_cert_ops)
      if (fl[(size_t)po.first]) c->oz_ops -= po.second / OZ_MAXMOD;
    c->oz_cert_ops.clear();
  }
  return GPE_OK;
}

}  // namespace

extern "C" {

int gpe_objective(gpe_ctx* c, int32_t variant, int32_t kernel, const double* hp, int32_t n_hp,
                  double nu_fixed, int32_t want_grad, double* llh_out, double* grad_out,
                  double* sigma2_out) {
  CHK(check_ready(c));
  const InflightGuard inflight(c->device);
  if (!hp || !llh_out) return fail(c, GPE_ERR_ARG, "null output");
  const int d = c->d, q = c->q;
  ObjArgs o;
  CHK(objective_args(variant, kernel, d, hp, n_hp, nu_fixed, &o, &c->err));
  if (!kernel_ok(kernel)) return fail(c, GPE_ERR_ARG, "bad kernel");
  if (want_grad && !grad_out) return fail(c, GPE_ERR_ARG, "grad_out is NULL");
  c->factor_valid = false;
  c->ainv_valid = false;
  c->x32_valid = false;
  c->px_valid = false;
  if (c->prof) {
    c->gev_used = 0;
    c->gemm_launches = c->gemm_flops = c->gemm_ms = 0.0;
    c->oev_used = 0;
    c->oz_ms = c->oz_launches = c->oz_ops = c->oz_flops64 = 0.0;
    c->oz_cert_ops.clear();
  }
  const bool one_launch = c->tiny;
  if (one_launch && c->NB == 1 && d <= TINY_DM && q + 1 <= TINY_DM)
    return tiny_objective(c, o, kernel, hp, n_hp, want_grad != 0, llh_out, grad_out, sigma2_out);
  if (one_launch && c->NB >= 2 && c->NB <= SNB_MAXNB && d <= TINY_DM && q + 1 <= TINY_DM)
    return snb_objective(c, o, kernel, hp, n_hp, want_grad != 0, llh_out, grad_out, sigma2_out);

  // z, w = L^-1 [f H] come out of the factorisation (augmented row); value only runs
  // no L^-1 at all
  CHK(factor_and_invert(c, kernel, hp, o.nu, o.s2, o.rscale, want_grad != 0, true));
  const int P = q + 1;
  const long long np = c->n_pad;
  const int NBt = c->tr.NB;
  // Gram, log-determinant parts and the failure flag go to the host behind an event;
  // A^-1 = L^-T L^-1 (22 ms at n=16384, independent of the host algebra) is queued
  // before the host waits, so the GPU does not idle over the round trip
  CHK(ensure_pinned(c, (size_t)P * P + NBt + 64));
  CHK(gram_async(c, c->dZ, np, P, (int)np));
  HIPCHK(c, hipMemcpyAsync(c->hpin + P * P, c->tr.logdet, NBt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->hpin + P * P + NBt, c->dinfo, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_host, c->stream));
  ev_rec(c, 4);
  if (want_grad) CHK(oz_use(c) ? lauum_ozaki(c, c->tr) : lauum(c, c->tr));
  ev_rec(c, 5);
  HIPCHK(c, hipEventSynchronize(c->ev_host));
  std::vector<double> G(c->hpin, c->hpin + (size_t)P * P);
  int info = 0;
  std::memcpy(&info, c->hpin + P * P + NBt, sizeof(int));
  if (info == GEMM_WAIT_TIMEOUT) return fail(c, GPE_ERR_HIP, "internal error: Cholesky panel wait timed out");
  double logdetA = 0.0;
  for (int k = 0; k < NBt; ++k) logdetA += c->hpin[P * P + k];
  logdetA *= 2.0;
  if (info != 0) return fail(c, GPE_NOT_PD, not_pd_pivot(info));
  const SmallAlgebra sa = small_from_gram(G, P);
  if (!sa.ok) return fail(c, GPE_NOT_PD, Q_NOT_PD);
  const ObjValue v = objective_value(sa, logdetA, (double)c->n, q, o.gp4ml, o.s2);
  *llh_out = v.llh;
  if (sigma2_out) *sigma2_out = v.sig2;
  if (!want_grad) {
    ev_rec(c, 6);
    ev_rec(c, 7);
    goto done;
  }
  {
    // R2 = [sqrt(c)(z - w B), w Kq^-T] ; [sqrt(c) alpha, W] = L^-T R2
    CHK(ensure_pinned(c, (size_t)P * P + 8));
    const std::vector<double> T2 = small_t2(sa, q, v.cfac);
    std::memcpy(c->hpin, T2.data(), T2.size() * sizeof(double));
    HIPCHK(c, hipMemcpyAsync(c->dT2, c->hpin, T2.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHK(apply_small(c, c->dZ, np, P, c->dT2, P, c->dR2, np, (int)np, c->dinfo));
    CHK(skinny(c, true, c->tr.B, np, c->NB, c->NB, true, c->dR2, np, P, c->dWa, np));
    ev_rec(c, 6);
    // contraction; sum_i M_ii r_i for the std kernel's sigma gradient when r is set
    const double* rdiag = (o.gp4ml && !kernel_alt(kernel) && c->has_r) ? c->dr : nullptr;
    const int nblk = c->NB * (c->NB + 1) / 2;
    int cs = 1;   // few tiles (small n): each tile's columns over up to 4 workgroups
    if (!(d > 32 || P > 33))
      while (cs < 4 && nblk * cs * 2 <= 512) cs *= 2;
    const dim3 gc(nblk * cs);
    with_fam(kernel_fam(kernel), [&](auto F) { launch_contract<decltype(F)::value>(c, d, P, gc, nblk, rdiag, cs, c->dWa); });
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_reduce_rows, dim3(d + 3), dim3(256), 0, c->stream, c->dcpart, nblk * cs, d + 3, c->dcsum);
    HIPCHK(c, hipGetLastError());
    ev_rec(c, 7);
    HIPCHK(c, hipMemcpyAsync(c->hpin, c->dcsum, (d + 3) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    objective_grad(c->hpin, d, kernel, o.nu, o.fitnug, o.gp4ml, v.gscale, o.s2, n_hp, grad_out, rdiag != nullptr);
  }
done:
  return objective_phase_times(c);
}

int gpe_set_outputs(gpe_ctx* c, int32_t p, const double* F) {
  CHK(check_ready(c));
  const int q = c->q;
  const long long n = c->n, np = c->n_pad;
  if (p < 1 || p > PMM_MAXP || !F) return fail(c, GPE_ERR_ARG, "bad outputs (1 <= p <= 64, F not NULL)");
  if (n < (long long)p + q + 3) return fail(c, GPE_ERR_ARG, "p outputs need n >= p + q + 3 training points");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->mo_p = 0;
  const int P = p + q;
  const size_t cols = (size_t)np * std::max(SK_PMAX, P);
  CHK(ensure_shape_bufs(c, c->d, P));
  CHK(grow_buf(c, &c->dFm, &c->fm_cap, (size_t)np * P));
  CHK(grow_buf(c, &c->dZm, &c->zm_cap, cols));
  CHK(grow_buf(c, &c->dR2m, &c->r2m_cap, cols));
  CHK(grow_buf(c, &c->dWm, &c->wm_cap, cols));
  // [F H] column-major, padded rows 0: F from the host, H as gpe_set_data left it in [f H]
  const size_t nf = (size_t)np * p;
  CHK(ensure_pinned(c, nf));
  std::memset(c->hpin, 0, nf * sizeof(double));
  for (long long i = 0; i < n; ++i)
    for (int a = 0; a < p; ++a) c->hpin[i + (long long)a * np] = F[i * p + a];
  HIPCHK(c, hipMemcpy(c->dFm, c->hpin, nf * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->dFm + nf, c->dF + np, (size_t)np * q * sizeof(double), hipMemcpyDeviceToDevice));
  c->mo_p = p;
  return GPE_OK;
}

int gpe_objective_multi(gpe_ctx* c, int32_t kernel, const double* hp, int32_t n_hp, double nu_fixed,
                        int32_t want_grad, double* llh_out, double* grad_out, double* Sigma_out, double* B_out) {
  CHK(check_ready(c));
  if (!c->mo_p) return fail(c, GPE_ERR_STATE, "gpe_set_outputs has not been called for this data");
  const InflightGuard inflight(c->device);
  if (!hp || !llh_out || !Sigma_out) return fail(c, GPE_ERR_ARG, "null output");
  const int d = c->d, q = c->q, p = c->mo_p, P = p + q;
  ObjArgs o;
  CHK(objective_args(GPE_MUCM, kernel, d, hp, n_hp, nu_fixed, &o, &c->err));
  if (!kernel_ok(kernel)) return fail(c, GPE_ERR_ARG, "bad kernel");
  if (want_grad && !grad_out) return fail(c, GPE_ERR_ARG, "grad_out is NULL");
  c->factor_valid = false;
  c->ainv_valid = false;
  c->x32_valid = false;
  c->px_valid = false;
  if (c->prof) {
    c->gev_used = 0;
    c->gemm_launches = c->gemm_flops = c->gemm_ms = 0.0;
    c->oev_used = 0;
    c->oz_ms = c->oz_launches = c->oz_ops = c->oz_flops64 = 0.0;
    c->oz_cert_ops.clear();
  }
  // the general path of gpe_objective at every n, on the p + q columns of [F H]
  const Cols cols{c->dFm, P, c->dZm};
  CHK(factor_and_invert(c, kernel, hp, o.nu, o.s2, o.rscale, want_grad != 0, true, &cols));
  const long long np = c->n_pad;
  const int NBt = c->tr.NB;
  CHK(ensure_pinned(c, (size_t)P * P + NBt + 64));
  CHK(gram_async(c, c->dZm, np, P, (int)np));
  HIPCHK(c, hipMemcpyAsync(c->hpin + P * P, c->tr.logdet, NBt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->hpin + P * P + NBt, c->dinfo, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_host, c->stream));
  ev_rec(c, 4);
  if (want_grad) CHK(oz_use(c) ? lauum_ozaki(c, c->tr) : lauum(c, c->tr));
  ev_rec(c, 5);
  HIPCHK(c, hipEventSynchronize(c->ev_host));
  const std::vector<double> G(c->hpin, c->hpin + (size_t)P * P);
  int info = 0;
  std::memcpy(&info, c->hpin + P * P + NBt, sizeof(int));
  if (info == GEMM_WAIT_TIMEOUT) return fail(c, GPE_ERR_HIP, "internal error: Cholesky panel wait timed out");
  double logdetA = 0.0;
  for (int k = 0; k < NBt; ++k) logdetA += c->hpin[P * P + k];
  logdetA *= 2.0;
  if (info != 0) return fail(c, GPE_NOT_PD, not_pd_pivot(info));
  const SmallMulti sm = small_multi_from_gram(G, p, q);
  if (!sm.ok()) return fail(c, GPE_NOT_PD, sm.refused == 1 ? Q_NOT_PD : S_NOT_PD);
  const ObjValueMulti v = objective_value_multi(sm, logdetA, (double)c->n);
  *llh_out = v.llh;
  std::memcpy(Sigma_out, v.Sigma.data(), v.Sigma.size() * sizeof(double));
  if (B_out) std::memcpy(B_out, sm.B.data(), sm.B.size() * sizeof(double));
  if (!want_grad) {
    ev_rec(c, 6);
    ev_rec(c, 7);
    return objective_phase_times(c);
  }
  // W = L^-T Z T2 = [sqrt((n - q) / p) P F C^-T, G Kq^-T], then the contraction of
  // M = A^-1 - W W^T as for one output
  CHK(ensure_pinned(c, (size_t)P * P + 8));
  const std::vector<double> T2 = small_multi_t2(sm, v.cfac);
  std::memcpy(c->hpin, T2.data(), T2.size() * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(c->dT2, c->hpin, T2.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  CHK(apply_small(c, c->dZm, np, P, c->dT2, P, c->dR2m, np, (int)np, c->dinfo));
  CHK(skinny(c, true, c->tr.B, np, c->NB, c->NB, true, c->dR2m, np, P, c->dWm, np));
  ev_rec(c, 6);
  const int nblk = c->NB * (c->NB + 1) / 2;
  int cs = 1;   // few tiles (small n): each tile's columns over up to 4 workgroups
  if (!(d > 32 || P > 33))
    while (cs < 4 && nblk * cs * 2 <= 512) cs *= 2;
  const dim3 gc(nblk * cs);
  with_fam(kernel_fam(kernel),
           [&](auto F) { launch_contract<decltype(F)::value>(c, d, P, gc, nblk, nullptr, cs, c->dWm); });
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_reduce_rows, dim3(d + 3), dim3(256), 0, c->stream, c->dcpart, nblk * cs, d + 3, c->dcsum);
  HIPCHK(c, hipGetLastError());
  ev_rec(c, 7);
  HIPCHK(c, hipMemcpyAsync(c->hpin, c->dcsum, (d + 3) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  objective_grad(c->hpin, d, kernel, o.nu, o.fitnug, false, v.gscale, 1.0, n_hp, grad_out, false);
  return objective_phase_times(c);
}

int gpe_factor(gpe_ctx* c, int32_t kernel, const double* delta, double nu, double s2, double r_scale) {
  CHK(check_ready(c));
  if (!delta) return fail(c, GPE_ERR_ARG, "null delta");
  if (!kernel_ok(kernel)) return fail(c, GPE_ERR_ARG, "bad kernel");
  c->factor_valid = false;
  c->ainv_valid = false;
  c->x32_valid = false;
  c->px_valid = false;
  CHK(factor_and_invert(c, kernel, delta, nu, s2, r_scale, false, c->oz_chol == 3));   // L^-1 on demand
  int info = 0;
  double logdet = 0.0;
  CHK(read_info_logdet(c, c->tr, &info, &logdet));
  if (info != 0) return fail(c, GPE_NOT_PD, not_pd_pivot(info));
  c->factor_valid = true;
  c->x32_valid = false;
  c->px_valid = false;
  c->f_kernel = kernel;
  c->f_delta.assign(delta, delta + c->d);
  c->f_nu = nu;
  c->f_rscale = r_scale;
  return GPE_OK;
}

// ---------------------------------------------------------------- sensitivity
// moduli of the posterior's int8 product: 16 for precision 64 (53-bit operands at n_pad <=
// 16384, as the objective's), for precision 32 the fewest whose operands keep >= 24 bits (the
// fp32 significand: 8 at n_pad <= 16384) -- exact products of operands as precise as fp32's
static int posterior_nmod(int np2, bool f32) {
  if (!f32) return OZ_MAXMOD;
  int bits = 24;
  if (const char* e = std::getenv("GPEMU_OZAKI_POST32_BITS")) bits = std::max(16, std::min(53, std::atoi(e)));
  for (int N = 6; N < OZ_MAXMOD; ++N)
    if (oz_consts(N, np2).beta >= bits) return N;
  return OZ_MAXMOD;
}

// V = L^-1 K* (n_pad x mp, fp64, ld n_pad) on the int8 cores (gpemu_ozaki.hpp): op(A) = the
// rows of L^-1 (k <= the row: kend = 256 (ti + 1)), op(B) = the chunk's points (columns of K*,
// contiguous in k), N moduli, CRT straight into V.  Replaces the fp64 k_gemm product
// (precision 64, 62 TF/s) and the fp32 one (precision 32, 129 TF/s); the column norms and the
// full-covariance blocks read V as before.
static int posterior_oz(gpe_ctx* c, bool f32, const double* Ks, long long mp, double* V) {
  const int np = (int)c->n_pad, np2 = (np + OZ_T - 1) / OZ_T * OZ_T;
  const int mp2 = (int)((mp + OZ_T - 1) / OZ_T * OZ_T);
  const int N = posterior_nmod(np2, f32), nti = np2 / OZ_T, ntj = mp2 / OZ_T;
  const OzConst k = oz_consts(N, np2);
  const OzShape s = OzShape::rect(nti, ntj, np2, 0, 1);
  hipStream_t st = c->stream;
  if (!c->px_valid || c->px_nmod != N) {
    CHK(grow_buf(c, &c->dpxp, &c->pxp_cap, (size_t)N * np2 * np2));
    CHK(grow_buf(c, &c->dpxe, &c->pxe_cap, (size_t)np2));
    oz_operand(st, k, OzSrc{c->tr.B, (long long)np, np, np, 2, true}, np2, np2, c->dpxe, c->dpxp);
    HIPCHK(c, hipGetLastError());
    c->px_valid = true;
    c->px_nmod = N;
  }
  const long long pB = (long long)mp2 * np2, rb = s.res_bytes();
  // (the diagonal posterior queues chunk i + 1 while chunk i runs: a new tile list or larger
  // buffers wait for it)
  if (c->pl_nti != nti || c->pl_ntj != ntj || (size_t)N * pB > c->pkp_cap || (size_t)mp2 > c->pke_cap ||
      (size_t)N * rb > c->pres_cap)
    HIPCHK(c, hipStreamSynchronize(st));
  if (c->pl_nti != nti || c->pl_ntj != ntj) {
    const std::vector<unsigned> l = s.list();
    c->pl_nti = c->pl_ntj = 0;
    CHK(grow_buf(c, &c->dpl, &c->pl_cap, l.size()));
    HIPCHK(c, hipMemcpy(c->dpl, l.data(), l.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    c->pl_len = (int)l.size();
    c->pl_nti = nti;
    c->pl_ntj = ntj;
  }
  CHK(grow_buf(c, &c->dpkp, &c->pkp_cap, (size_t)N * pB));
  CHK(grow_buf(c, &c->dpke, &c->pke_cap, (size_t)mp2));
  CHK(grow_buf(c, &c->dpres, &c->pres_cap, (size_t)N * rb));
  oz_operand(st, k, OzSrc{Ks, (long long)np, (int)mp, np, 0, false}, mp2, np2, c->dpke, c->dpkp);
  // (no events: not a product of the objective, kept out of gpe_ozaki_stats)
  const OzOpnd linv{c->dpxp, (long long)np2 * np2, np2, 0}, kstar{c->dpkp, pB, np2, 0};
  HIPCHK(c, oz_product_launch(st, k,
                              OzProduct{s, linv, kstar, c->dpl, c->pl_len, c->dpres, rb,
                                        OzOut{c->dpxe, c->dpke, V, (long long)np, np, (int)mp, 0, 1.0}}));
  return GPE_OK;
}

// A^-1 = L^-T L^-1 of the resident factor into tr.A (the LAUUM launch of the plan)
static int ensure_ainv(gpe_ctx* c) {
  if (c->ainv_valid) return GPE_OK;
  CHK(ensure_linv(c));
  CHK(lauum(c, c->tr));
  c->ainv_valid = true;
  return GPE_OK;
}

int gpe_solve(gpe_ctx* c, int32_t ncols, const double* B, double* X) {
  CHK(check_ready(c));
  if (!c->factor_valid) return fail(c, GPE_ERR_STATE, "no resident factor (call gpe_factor)");
  if (ncols <= 0 || !B || !X) return fail(c, GPE_ERR_ARG, "bad solve args");
  CHK(ensure_linv(c));
  const long long np = c->n_pad, n = c->n;
  for (int c0 = 0; c0 < ncols; c0 += SK_PMAX) {
    const int cc = std::min(SK_PMAX, ncols - c0);
    CHK(ensure_pinned(c, (size_t)np * cc + 64));
    std::memset(c->hpin, 0, (size_t)np * cc * sizeof(double));
    for (long long i = 0; i < n; ++i)
      for (int k = 0; k < cc; ++k) c->hpin[i + k * np] = B[i * ncols + c0 + k];
    HIPCHK(c, hipMemcpyAsync(c->dR2, c->hpin, (size_t)np * cc * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHK(skinny(c, false, c->tr.B, np, c->NB, c->NB, true, c->dR2, np, cc, c->dZ, np));   // L^-1 B
    CHK(skinny(c, true, c->tr.B, np, c->NB, c->NB, true, c->dZ, np, cc, c->dWa, np));    // L^-T L^-1 B
    HIPCHK(c, hipMemcpyAsync(c->hpin, c->dWa, (size_t)np * cc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (long long i = 0; i < n; ++i)
      for (int k = 0; k < cc; ++k) X[i * ncols + c0 + k] = c->hpin[i + k * np];
  }
  return GPE_OK;
}

int gpe_sense_pairs(gpe_ctx* c, int32_t J, const double* w, const double* u, int32_t p, const double* Z,
                    double* trace_out, double* quad_out) {
  CHK(check_ready(c));
  if (!c->factor_valid) return fail(c, GPE_ERR_STATE, "no resident factor (call gpe_factor)");
  if (J <= 0 || J > 65535 || p <= 0 || !w || !u || !Z || !trace_out || !quad_out)
    return fail(c, GPE_ERR_ARG, "bad sense_pairs args");
  const int d = c->d;
  // Z columns in chunks of at most 32 (one launch each; PMAX = the chunk bucket + 2);
  // d > 32: k_sense_pairs_wide (coordinates staged through LDS in chunks of 32)
  const int pchunk = std::min(p, 32);
  const bool wide = d > 32;
  const long long np = c->n_pad, n = c->n;
  const int NB = c->NB;
  CHK(ensure_ainv(c));
  const long long ldp = (long long)J * (1 + p * p);
  CHK(grow_buf(c, &c->dSU, &c->su_cap, (size_t)J * np));
  CHK(grow_buf(c, &c->dSZ, &c->sz_cap, (size_t)np * p));
  CHK(grow_buf(c, &c->dSW, &c->sw_cap, (size_t)J * d));
  // column slices: enough workgroups to fill the chip (>= 2048) when J is small
  const int ct = wide ? SPW_CT : SP_CT;
  const int nct = (int)((n + ct - 1) / ct);
  const int CS = std::max(1, std::min(nct, (2048 + NB * J - 1) / (NB * J)));
  const int cslice = ((nct + CS - 1) / CS) * ct;
  CHK(grow_buf(c, &c->dSpart, &c->spart_cap, (size_t)NB * CS * 4 * ldp));
  CHK(grow_buf(c, &c->dSout, &c->sout_cap, (size_t)ldp));
  CHK(ensure_pinned(c, std::max<size_t>({(size_t)J * np, (size_t)np * p, (size_t)J * d, (size_t)ldp}) + 64));
  // w, u (J x n_pad, zero padded), Z (n_pad x p column-major): staged one at a time
  std::memcpy(c->hpin, w, (size_t)J * d * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(c->dSW, c->hpin, (size_t)J * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memset(c->hpin, 0, (size_t)J * np * sizeof(double));
  for (int j = 0; j < J; ++j) std::memcpy(c->hpin + (size_t)j * np, u + (size_t)j * n, (size_t)n * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(c->dSU, c->hpin, (size_t)J * np * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memset(c->hpin, 0, (size_t)np * p * sizeof(double));
  for (long long i = 0; i < n; ++i)
    for (int k = 0; k < p; ++k) c->hpin[i + k * np] = Z[i * p + k];
  HIPCHK(c, hipMemcpyAsync(c->dSZ, c->hpin, (size_t)np * p * sizeof(double), hipMemcpyHostToDevice, c->stream));
  const dim3 grid((unsigned)NB, (unsigned)J, (unsigned)CS);
  const int need_d = std::max(d, pchunk - 2);
  for (int zc0 = 0; zc0 < p; zc0 += pchunk) {
    const int pc = std::min(pchunk, p - zc0);
#define SENSE_LAUNCH(DM, PM)                                                                              \
  hipLaunchKernelGGL((k_sense_pairs<DM, PM>), grid, dim3(256), 0, c->stream, c->tr.A, np, c->dX, d, c->dSW, \
                     c->dSU, np, c->dSZ, np, p, (int)n, cslice, c->dSpart, ldp, zc0, pc)
#define SENSE_LAUNCH_WIDE(PM)                                                                               \
  hipLaunchKernelGGL((k_sense_pairs_wide<PM>), grid, dim3(256), 0, c->stream, c->tr.A, np, c->dX, d, c->dSW, \
                     c->dSU, np, c->dSZ, np, p, (int)n, cslice, c->dSpart, ldp, zc0, pc)
    if (wide) {
      if (pc <= 8) SENSE_LAUNCH_WIDE(8);
      else if (pc <= 16) SENSE_LAUNCH_WIDE(16);
      else SENSE_LAUNCH_WIDE(32);
    } else if (need_d <= 4) SENSE_LAUNCH(4, 6);
    else if (need_d <= 8) SENSE_LAUNCH(8, 10);
    else if (need_d <= 16) SENSE_LAUNCH(16, 18);
    else SENSE_LAUNCH(32, 34);
#undef SENSE_LAUNCH
#undef SENSE_LAUNCH_WIDE
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_reduce_rows, dim3((unsigned)ldp), dim3(256), 0, c->stream, c->dSpart, NB * CS * 4,
                     (int)ldp, c->dSout);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->hpin, c->dSout, (size_t)ldp * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int j = 0; j < J; ++j) {
    const double* o = c->hpin + (size_t)j * (1 + p * p);
    trace_out[j] = o[0];
    std::memcpy(quad_out + (size_t)j * p * p, o + 1, (size_t)p * p * sizeof(double));
  }
  return GPE_OK;
}

int gpe_gauss_transform(gpe_ctx* c, int64_t m, int32_t ns, const int32_t* dims, const double* cw, const double* Y,
                        const double* a, double* out) {
  CHK(check_ready(c));
  if (m <= 0 || m > (int64_t)1 << 30 || ns <= 0 || ns > 4 || !dims || !cw || !Y || !a || !out)
    return fail(c, GPE_ERR_ARG, "bad gauss_transform args");
  for (int s = 0; s < ns; ++s)
    if (dims[s] < 0 || dims[s] >= c->d) return fail(c, GPE_ERR_ARG, "dims out of range");
  const long long n = c->n;
  // device layout: a (n) | Y (m x ns) | out (m)
  const size_t need = (size_t)n + (size_t)m * ns + (size_t)m;
  CHK(grow_buf(c, &c->dSout, &c->sout_cap, need));
  CHK(ensure_pinned(c, need + 64));
  std::memcpy(c->hpin, a, (size_t)n * sizeof(double));
  std::memcpy(c->hpin + n, Y, (size_t)m * ns * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(c->dSout, c->hpin, (n + (size_t)m * ns) * sizeof(double), hipMemcpyHostToDevice, c->stream));
  GaussArgs g;
  g.x = c->dX; g.a = c->dSout; g.Y = c->dSout + n; g.out = c->dSout + n + (size_t)m * ns;
  g.d = c->d; g.n = (int)n; g.m = (int)m; g.ns = ns;
  for (int s = 0; s < 4; ++s) {
    g.dims[s] = s < ns ? dims[s] : 0;
    g.c[s] = s < ns ? cw[s] : 0.0;
  }
  hipLaunchKernelGGL(k_gauss_transform, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, c->stream, g);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->hpin, g.out, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memcpy(out, c->hpin, (size_t)m * sizeof(double));
  return GPE_OK;
}

int gpe_beta(gpe_ctx* c, double* beta_out) {
  CHK(check_ready(c));
  if (!c->factor_valid) return fail(c, GPE_ERR_STATE, "no resident factor (call gpe_factor)");
  const int P = c->q + 1;
  const long long np = c->n_pad;
  CHK(z_from_factor(c));   // dZ is scratch of other entries: re-formed from the factor
  std::vector<double> G((size_t)P * P);
  CHK(gram(c, c->dZ, np, P, (int)np, G.data()));
  SmallAlgebra sa = small_from_gram(G, P);
  if (!sa.ok) return fail(c, GPE_NOT_PD, Q_NOT_PD);
  for (int i = 0; i < c->q; ++i) beta_out[i] = sa.beta[i];
  return GPE_OK;
}

int gpe_beta_multi(gpe_ctx* c, double* B_out) {
  CHK(check_ready(c));
  if (!c->factor_valid) return fail(c, GPE_ERR_STATE, "no resident factor (call gpe_factor)");
  if (!c->mo_p) return fail(c, GPE_ERR_STATE, "gpe_set_outputs has not been called for this data");
  if (!B_out) return fail(c, GPE_ERR_ARG, "B_out is NULL");
  const int p = c->mo_p, P = p + c->q;
  const long long np = c->n_pad;
  const Cols cols{c->dFm, P, c->dZm};
  CHK(z_from_factor(c, &cols));
  std::vector<double> G((size_t)P * P);
  CHK(gram(c, c->dZm, np, P, (int)np, G.data()));
  const SmallMulti sm = small_multi_from_gram(G, p, c->q);
  if (sm.refused == 1) return fail(c, GPE_NOT_PD, Q_NOT_PD);   // (B needs Q alone)
  std::memcpy(B_out, sm.B.data(), sm.B.size() * sizeof(double));
  return GPE_OK;
}

// Leave-one-out mean and variance at every training point (include/gpemu.h; derivation in
// DESIGN.md).  With X = L^-1, Z = X [f H], Kq Kq^T = Z_H^T Z_H and T2 = small_t2(cfac = 1):
//   X^T (Z T2) = A^-1 [f - H beta, H Kq^-T]   and   (A^-1)_ii = sum_k X(k, i)^2,
// both from one sweep over L^-1 (skinny_t_sq); k_loo_finish forms P_ii, the mean and the
// variance on the device.
int gpe_loo(gpe_ctx* c, double sigma, double* mean_out, double* var_out, double* beta_out) {
  CHK(check_ready(c));
  if (!c->factor_valid) return fail(c, GPE_ERR_STATE, "no resident factor (call gpe_factor)");
  if (!mean_out || !var_out) return fail(c, GPE_ERR_ARG, "bad loo args");
  const int q = c->q, P = q + 1;
  const long long np = c->n_pad, n = c->n;
  if (n < q + 2) return fail(c, GPE_ERR_ARG, "leave-one-out needs n >= q + 2 training points");
  CHK(ensure_linv(c));
  CHK(z_from_factor(c));   // dZ is scratch of other entries: re-formed from the factor
  std::vector<double> G((size_t)P * P);
  CHK(gram(c, c->dZ, np, P, (int)np, G.data()));
  SmallAlgebra sa = small_from_gram(G, P);
  if (!sa.ok) return fail(c, GPE_NOT_PD, Q_NOT_PD);
  CHK(ensure_pinned(c, (size_t)std::max<long long>(2 * np, (long long)P * P) + 8));
  const std::vector<double> T2 = small_t2(sa, q, 1.0);
  std::memcpy(c->hpin, T2.data(), T2.size() * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(c->dT2, c->hpin, T2.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  CHK(apply_small(c, c->dZ, np, P, c->dT2, P, c->dR2, np, (int)np, c->dinfo));
  CHK(ensure_small(c, (size_t)3 * np));   // (A^-1)_ii, mean, var (gram's partials are consumed)
  double* asq = c->dsmall;
  double* dmean = c->dsmall + np;
  double* dvar = c->dsmall + 2 * np;
  CHK(skinny_t_sq(c, c->tr.B, np, c->NB, n, c->dR2, np, P, c->dWa, np, asq));
  const double* r = (c->has_r && c->f_rscale != 0.0) ? c->dr : nullptr;
  hipLaunchKernelGGL(k_loo_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, asq, c->dWa, np, q,
                     c->dF, r, c->f_rscale, sigma * sigma, (int)n, dmean, dvar);
  HIPCHK(c, hipGetLastError());
  // mean and var are adjacent: one copy
  HIPCHK(c, hipMemcpyAsync(c->hpin, dmean, (size_t)2 * np * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memcpy(mean_out, c->hpin, (size_t)n * sizeof(double));
  std::memcpy(var_out, c->hpin + np, (size_t)n * sizeof(double));
  if (beta_out)
    for (int i = 0; i < q; ++i) beta_out[i] = sa.beta[i];
  return GPE_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ posterior
// Posterior mean and variance at m points for the resident factor: gpe_posterior, and the
// covariance that gpe_noise_sample and gpe_posterior_pivchol go on from (posterior_impl).
namespace {

// points per chunk: the full variance forms one chunk pair's block at a time, the diagonal
// pipeline holds two chunks in flight
constexpr long long POST_CHUNK_FULL = 16384, POST_CHUNK_DIAG = 8192;

inline long long pad_to(long long v, long long unit) { return ((v + unit - 1) / unit) * unit; }

// 1 / delta of the resident factor, through d doubles of the pinned buffer, into c->dinvdelta
int upload_invdelta(gpe_ctx* c, double* pin) {
  for (int k = 0; k < c->d; ++k) pin[k] = 1.0 / c->f_delta[k];
  HIPCHK(c, hipMemcpyAsync(c->dinvdelta, pin, c->d * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return GPE_OK;
}

// The chunk pipelines' events, one per pinned result slot (made at the first use), and
// chunk_pipeline's wait and drain for them
int pipe_events(gpe_ctx* c) {
  if (!c->ev_pipe[0])
    for (hipEvent_t& e : c->ev_pipe) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return GPE_OK;
}
int pipe_wait(gpe_ctx* c, int slot) {
  HIPCHK(c, hipEventSynchronize(c->ev_pipe[slot]));
  return GPE_OK;
}
template <class Dev, class Host>
int run_chunks(gpe_ctx* c, long long m, long long chunk, Dev&& dev, Host&& host) {
  return chunk_pipeline(m, chunk, dev, [&](int slot) { return pipe_wait(c, slot); }, host,
                        [&] { (void)hipStreamSynchronize(c->stream); });
}

// The per-chunk profiling bracket: the device time of what is queued between the two calls is
// added to phase_ms[0], and 1 to phase_ms[1].  Nothing unless c->prof (profiling only: one
// synchronisation per chunk).
int chunk_prof_begin(gpe_ctx* c) {
  if (c->prof) HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  return GPE_OK;
}
int chunk_prof_end(gpe_ctx* c) {
  if (!c->prof) return GPE_OK;
  float ms = 0.f;
  HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
  HIPCHK(c, hipEventSynchronize(c->ev[5]));
  (void)hipEventElapsedTime(&ms, c->ev[4], c->ev[5]);
  c->phase_ms[0] += ms;
  c->phase_ms[1] += 1.0;
  return GPE_OK;
}

// where the variance goes (on the device: column-major, ld = m rounded up to TILE, identity
// padding)
enum class PostVar {
  DIAG,       // its diagonal to var_out (m)
  FULL,       // m x m to var_out
  FULL_DW3,   // m x m left in c->dW3: one chunk (m <= POST_CHUNK_FULL)
  FULL_DEV,   // m x m into dev_out, beyond one chunk: the lower triangle of chunk blocks
  GROUPS,     // the group x group blocks of consecutive points to var_out (m / group of them)
};

struct PostReq {
  int64_t m = 0;
  const double* Xs = nullptr;     // points (m x d)
  const double* Hs = nullptr;     // their basis (m x q)
  const double* beta = nullptr;
  double sigma = 0.0;
  int precision = 64;             // 32: the diagonal variance only
  double* mean_out = nullptr;
  PostVar var = PostVar::DIAG;
  double* var_out = nullptr;      // host (DIAG, FULL)
  double* dev_out = nullptr;      // device (FULL_DEV)
  // rnew (m, host; the device copy is made here) adds s2 * rnew_scale * rnew to the full
  // variance's diagonal: Dnew's own r/s2 in Dnew.A (_emulatorclasses.py:572-575, :625)
  const double* rnew = nullptr;
  double rnew_scale = 0.0;
  // gpe_posterior_grad (DIAG, precision 64): dmean_out set asks for the gradients.  dHs
  // (m x q): each basis column's derivative in its own input hdim[j] (-1: a constant column)
  const double* dHs = nullptr;
  const int32_t* hdim = nullptr;
  double* dmean_out = nullptr;    // m x d
  double* dvar_out = nullptr;     // m x d, or NULL: the second product is skipped
  int group = 0;                  // GROUPS: points per group (m a multiple of it)
};

// k_post_grad<DMAX, FAM, WIDE, WB> for d inputs: the register widths of d <= 32, beyond that
// the wide instance with one workgroup column per 32 dimensions (grid.z)
template <int FAM, bool WB>
void launch_post_grad_fam(int d, dim3 g, hipStream_t st, const PostGradArgs& a) {
  const dim3 b(PG_PTS);
  if (d > 32) hipLaunchKernelGGL((k_post_grad<PG_WIDE, FAM, true, WB>), g, b, 0, st, a);
  else
    with_width(RegWidths(), d, [&](auto W) {
      hipLaunchKernelGGL((k_post_grad<decltype(W)::value, FAM, false, WB>), g, b, 0, st, a);
    });
}

template <bool WB>
void launch_post_grad(int fam, int d, dim3 g, hipStream_t st, const PostGradArgs& a) {
  with_fam(fam, [&](auto F) { launch_post_grad_fam<decltype(F)::value, WB>(d, g, st, a); });
}

// One chunk of points as cov_block reads it
struct CovSide {
  const double* X;   // scaled points (mp x d)
  const double* V;   // L^-1 K* (np x mp, ld np)
  double* T;         // T Kq^-T (mp x kq column-major, ld ldt)
  long long ldt;
  long long s0, mc, mp;   // first point, points, points padded to TILE
};

// One call: the request, its sizes, what setup() and workspace() derive, and the steps.
struct Posterior : PostReq {
  gpe_ctx* c;
  const bool full, f32, ozp;   // full variance; fp32 product; V on the int8 cores (posterior_oz)
  const bool groups;           // the blocks of groups of points, through the diagonal pipeline
  const int d, q, P, kq;       // kq: q rounded up to the GEMM's K step
  const long long np, CHUNK;
  const bool big;              // a full variance of more than one chunk
  const long long mtot, mp0;   // m padded; the largest chunk (the first) padded
  int fam = 0;                 // the resident factor's correlation family
  double coff = 0.0, cdiag = 0.0, s2 = 0.0;
  std::vector<double> Kinv;    // Kq^-1, Kq Kq^T = H^T A^-1 H
  size_t rs = 0;               // one result slot: Y (mp x P), then the column norms
  double *pin_in[2] = {}, *pin_out[2] = {};   // pinned staging: two slots of points, two of results
  // the gradients (grad): pinned slots of [Hs, dHs] and of [dmean, dvar], the parts of c->dPg
  const bool grad;
  double *gpin_in[2] = {}, *gpin_out[2] = {};
  struct {
    double *Hs, *dHs, *tau, *Qinv, *beta, *dmean, *dvar, *part, *Gq;
    int* hdim;
  } g = {};

  Posterior(gpe_ctx* ctx, const PostReq& r)
      : PostReq(r), c(ctx), full(var != PostVar::DIAG && var != PostVar::GROUPS), f32(precision == 32),
        ozp(c->oz_on && c->n_pad >= std::min(c->oz_min_np, OZ_POST_MIN_NP) && c->n_pad <= OZ_POST_MAX_NP),
        groups(var == PostVar::GROUPS), d(c->d), q(c->q), P(q + 1), kq(((q + 15) / 16) * 16), np(c->n_pad),
        // (whole groups per chunk: a group never straddles two)
        CHUNK(full ? POST_CHUNK_FULL : groups ? (POST_CHUNK_DIAG / group) * group : POST_CHUNK_DIAG),
        big(full && m > CHUNK), mtot(pad_to(m, TILE)),
        mp0(pad_to(std::min<long long>(CHUNK, m), TILE)), grad(r.dmean_out != nullptr) {}

  // Setup: the fp32 copy of L^-1 where the fp32 product needs it, [gamma, G] =
  // A^-1 [f - H beta, H] (in dWa; L^-1 [..] in dZ), Kq and its inverse, the kernel's constants.
  int setup() {
    if (f32 && !ozp && !c->x32_valid) {
      // fp32 copy of L^-1 (the full square: the GEMM reads only k <= its row tile)
      CHK(grow_buf(c, &c->dX32, &c->x32_cap, (size_t)np * np));
      hipLaunchKernelGGL(k_to_f32, dim3((unsigned)((np * np + 255) / 256)), dim3(256), 0, c->stream, c->tr.B, np,
                         c->dX32, np, np, (int)np);
      HIPCHK(c, hipGetLastError());
      c->x32_valid = true;
    }
    CHK(ensure_pinned(c, (size_t)P * P + 64));
    std::vector<double> T((size_t)P * P, 0.0);  // col-major
    T[0] = 1.0;
    for (int i = 0; i < q; ++i) {
      T[(i + 1) + 0 * P] = -beta[i];
      T[(i + 1) + (i + 1) * P] = 1.0;
    }
    std::memcpy(c->hpin, T.data(), T.size() * sizeof(double));
    HIPCHK(c, hipMemcpyAsync(c->dT2, c->hpin, T.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHK(apply_small(c, c->dF, np, P, c->dT2, P, c->dR2, np, (int)np, nullptr));
    CHK(skinny(c, false, c->tr.B, np, c->NB, c->NB, true, c->dR2, np, P, c->dZ, np));   // L^-1 [f-Hb, H]
    CHK(skinny(c, true, c->tr.B, np, c->NB, c->NB, true, c->dZ, np, P, c->dWa, np));   // A^-1 [f-Hb, H]
    std::vector<double> G((size_t)P * P);
    CHK(gram(c, c->dZ, np, P, (int)np, G.data()));
    // Q = H^T A^-1 H = G[1:,1:]
    std::vector<double> Kq((size_t)q * q);
    for (int i = 0; i < q; ++i)
      for (int j = 0; j < q; ++j) Kq[i * q + j] = G[(i + 1) * P + (j + 1)];
    if (!small_chol(Kq, q)) return fail(c, GPE_NOT_PD, Q_NOT_PD);
    Kinv = small_trinv(Kq, q);
    kernel_consts(c->f_kernel, c->f_nu, true, &coff, &cdiag);
    fam = kernel_fam(c->f_kernel);
    s2 = sigma * sigma;
    return GPE_OK;
  }

  // Workspace for the largest chunk (the first): K* (np x mp) and V (np x mp), the chunk's
  // points, two pinned staging slots of points and two of results, two device result slots;
  // 1 / delta on the device.  A full covariance of more than one chunk also keeps every
  // chunk's V, scaled points and T Kq^-T on the device until its blocks are formed.
  int workspace() {
    if (big) {
      CHK(grow_buf(c, &c->dVall, &c->vall_cap, (size_t)np * mtot));
      CHK(grow_buf(c, &c->dXall, &c->xall_cap, (size_t)mtot * d));
      CHK(grow_buf(c, &c->dTall, &c->tall_cap, (size_t)mtot * kq));
    }
    CHK(grow_buf(c, &c->dW1, &c->w1_cap, (size_t)np * mp0));
    CHK(grow_buf(c, &c->dW2, &c->w2_cap, (size_t)np * mp0));
    CHK(grow_buf(c, &c->dXs, &c->xs_cap, (size_t)mp0 * d));
    CHK(grow_buf(c, &c->dXsw, &c->xsw_cap, (size_t)mp0 * d));
    // (the groups' blocks take the place of the column norms: group values per point)
    rs = (size_t)mp0 * P + (groups ? (size_t)std::min<long long>(CHUNK, m) * group : (size_t)mp0);
    if (groups)
      CHK(grow_buf(c, &c->dPgc, &c->pgc_cap, (size_t)pgc_nseg(np) * std::min<long long>(CHUNK, m) * group));
    CHK(ensure_small(c, 2 * rs + 64));
    // (the full covariance also stages T Kq^-T, mp x kq, at the front: the capacity is set
    // here once, so the slots never move)
    // (the gradients add two slots of [Hs, dHs] and two of [dmean, dvar] behind 1 / delta)
    const size_t gsl = grad ? 2 * (size_t)mp0 * q + 2 * (size_t)mp0 * d : 0;
    CHK(ensure_pinned(c, std::max<size_t>(2 * (size_t)mp0 * d + 2 * rs + d + 2 * gsl, (size_t)mp0 * kq) + 64));
    pin_in[0] = c->hpin, pin_in[1] = pin_in[0] + (size_t)mp0 * d;
    pin_out[0] = pin_in[1] + (size_t)mp0 * d, pin_out[1] = pin_out[0] + rs;
    double* pin_dl = pin_out[1] + rs;   // 1 / delta
    CHK(upload_invdelta(c, pin_dl));
    if (grad) {
      for (int i = 0; i < 2; ++i) {
        gpin_in[i] = pin_dl + d + i * gsl;
        gpin_out[i] = gpin_in[i] + 2 * (size_t)mp0 * q;
      }
      CHK(grad_workspace());
    }
    return pipe_events(c);
  }

  // One chunk's device work: its points from the pinned slot pin, K*, Y = K*^T [gamma, G]
  // into dY, V = L^-1 K* into vdst (fp32 path: into dK32).
  int dev_chunk(long long s0, double* pin, double* dY, double* vdst) {
    const long long mc = std::min(CHUNK, m - s0), mp = pad_to(mc, TILE);
    const int mt = (int)(mp / TILE);
    std::memset(pin, 0, (size_t)mp * d * sizeof(double));
    std::memcpy(pin, Xs + s0 * d, (size_t)mc * d * sizeof(double));
    HIPCHK(c, hipMemcpyAsync(c->dXs, pin, (size_t)mp * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_scale_points, dim3((unsigned)((mp * d + 255) / 256)), dim3(256), 0, c->stream,
                       c->dXs, c->dinvdelta, d, (int)mc, (int)mp, c->dXsw);
    HIPCHK(c, hipGetLastError());
    // K*(i, s) = coff * exp(-|x_i - xs_s|^2), padded rows/cols 0
    PairArgs a;
    a.xr = c->dXw; a.xc = c->dXsw; a.out = c->dW1; a.ld = np; a.d = d;
    a.nr_valid = (int)c->n; a.nc_valid = (int)mc; a.mt = c->NB; a.nt = mt; a.mode = 0;
    a.s2 = 1.0; a.coff = coff; a.cdiag = cdiag; a.rscale = 0.0; a.r = nullptr;
    a.fam = fam;
    CHK(launch_pairs(c, a, c->NB * mt));
    // Y = K*^T [gamma, G]  (mp x P)
    // skinny transposed over a full matrix: M = K* (np x mp), k tiles = NB, out tiles = mt;
    // 32 columns of [gamma, G] at a time
    for (int c0 = 0; c0 < P; c0 += SK_PMAX) {
      const int pc = std::min(SK_PMAX, P - c0);
      const int nch = (c->NB + SK_CH - 1) / SK_CH;
      CHK(grow_buf(c, &c->dskp, &c->skp_cap, (size_t)nch * mp * pc));
      SkinnyArgs k;
      k.M = c->dW1; k.ldm = np; k.R = c->dWa + (long long)c0 * np; k.ldr = np; k.part = c->dskp; k.ldp = mp;
      k.pstride = mp * pc; k.P = pc; k.ntr = c->NB; k.lower = 0; k.nit = mt; k.abort_flag = nullptr;
      k.chk = SK_CH;
      const dim3 grid(mt * nch);
      if (pc <= 16) hipLaunchKernelGGL((k_skinny_mfma<16, true>), grid, dim3(256), 0, c->stream, k);
      else hipLaunchKernelGGL((k_skinny_mfma<32, true>), grid, dim3(256), 0, c->stream, k);
      HIPCHK(c, hipGetLastError());
      const long long tot = mp * pc;
      hipLaunchKernelGGL(k_reduce_chunks, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream,
                         c->dskp, (long long)(mp * pc), dY + (long long)c0 * mp, mp, pc, (int)mp, c->NB, 2,
                         nullptr, SK_CH);
      HIPCHK(c, hipGetLastError());
    }
    // V = L^-1 K*   (np x mp), X lower-triangular -> kend = (ti+1)*128
    if (ozp) return posterior_oz(c, f32, c->dW1, mp, vdst);
    if (!f32)
      return adhoc_gemm(c, ADHOC_POST_V,
                        {{GEMM_BK, mkprob(c->tr.B, np, c->dW1, np, vdst, np, c->NB, mt, (int)np, G_KEND_TI, 1.0, 0.0)}});
    CHK(grow_buf(c, &c->dK32, &c->k32_cap, 2 * (size_t)np * mp));
    float *K32 = c->dK32, *V32 = c->dK32 + (size_t)np * mp;
    hipLaunchKernelGGL(k_to_f32, dim3((unsigned)((np * mp + 255) / 256)), dim3(256), 0, c->stream, c->dW1, np,
                       K32, np, np, (int)mp);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_gemm_f32, dim3((unsigned)(c->NB * mt)), dim3(256), 2 * F32_STAGE * sizeof(float),
                       c->stream, c->dX32, np, K32, np, V32, np, c->NB, (int)np, 1);
    HIPCHK(c, hipGetLastError());
    return GPE_OK;
  }

  // k_post_grad's split of the training rows for a chunk of mp points: about 1024 workgroups
  // (two per SIMD pair of the chip), at most 64 partial sums per point and dimension
  int grad_nsplit(long long mp) const {
    const long long cols = (mp / PG_PTS) * (d > 32 ? (d + PG_WIDE - 1) / PG_WIDE : 1);
    return (int)std::max<long long>(1, std::min<long long>({np / PG_RI, 64, 1024 / cols}));
  }

  // The gradients' device workspace (the parts of c->dPg, U in dW3) and what does not change
  // from chunk to chunk: Q^-1 = Kq^-T Kq^-1, beta, hdim, and G = dWa's columns 1..q copied
  // into kq zero-padded columns, the first operand of the rank-q update.
  int grad_workspace() {
    const long long mpl = pad_to(m - ((m - 1) / CHUNK) * CHUNK, TILE);   // the last chunk
    const size_t nhd = (size_t)q / 2 + 1;
    // (a and b sums of every split; a short last chunk may split its rows further than the first)
    const size_t npart =
        2 * (size_t)d * std::max<size_t>((size_t)grad_nsplit(mp0) * mp0, (size_t)grad_nsplit(mpl) * mpl);
    const size_t sz[] = {(size_t)mp0 * q, (size_t)mp0 * q, (size_t)mp0 * kq, (size_t)q * q, (size_t)q, nhd,
                         (size_t)mp0 * d, (size_t)mp0 * d, npart, (size_t)np * kq};
    size_t tot = 0;
    for (size_t s : sz) tot += s;
    CHK(grow_buf(c, &c->dPg, &c->pg_cap, tot));
    double* p = c->dPg;
    g.Hs = p, p += sz[0];
    g.dHs = p, p += sz[1];
    g.tau = p, p += sz[2];
    g.Qinv = p, p += sz[3];
    g.beta = p, p += sz[4];
    g.hdim = reinterpret_cast<int*>(p), p += sz[5];
    g.dmean = p, p += sz[6];
    g.dvar = p, p += sz[7];
    g.part = p, p += sz[8];
    g.Gq = p;
    std::vector<double> hc((size_t)q * q + q + nhd, 0.0);
    for (int a = 0; a < q; ++a)
      for (int b = 0; b < q; ++b) {
        double acc = 0.0;
        for (int o = 0; o < q; ++o) acc += Kinv[o * q + a] * Kinv[o * q + b];
        hc[(size_t)a * q + b] = acc;
      }
    for (int i = 0; i < q; ++i) hc[(size_t)q * q + i] = beta[i];
    std::memcpy(hc.data() + (size_t)q * q + q, hdim, (size_t)q * sizeof(int32_t));
    // (Q^-1, beta and hdim lie together; a blocking copy, once per call)
    HIPCHK(c, hipMemcpy(g.Qinv, hc.data(), hc.size() * sizeof(double), hipMemcpyHostToDevice));
    if (!dvar_out) return GPE_OK;
    CHK(grow_buf(c, &c->dW3, &c->w3_cap, (size_t)np * mp0));
    HIPCHK(c, hipMemsetAsync(g.Gq, 0, (size_t)np * kq * sizeof(double), c->stream));
    HIPCHK(c, hipMemcpyAsync(g.Gq, c->dWa + np, (size_t)np * q * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return GPE_OK;
  }

  // One chunk's gradients, queued behind its dev_chunk (Y in dY, V in dW2): tau on the
  // device from Y (no host round trip, so the two-chunk pipeline stays as it is), U =
  // L^-T V + G tau^T in dW3, the fused sums, the epilogue, and the copy of [dmean, dvar] into
  // the pinned slot.  L^-1 is read K-contiguous from its row tile on, as the LAUUM reads it.
  int grad_chunk(long long s0, int slot, const double* dY) {
    const long long mc = std::min(CHUNK, m - s0), mp = pad_to(mc, TILE);
    const int mt = (int)(mp / TILE);
    const size_t hq = (size_t)mc * q, md = (size_t)mp * d;
    double* hin = gpin_in[slot];
    std::memcpy(hin, Hs + s0 * q, hq * sizeof(double));
    std::memcpy(hin + (size_t)mp0 * q, dHs + s0 * q, hq * sizeof(double));
    HIPCHK(c, hipMemcpyAsync(g.Hs, hin, hq * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(g.dHs, hin + (size_t)mp0 * q, hq * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const bool wb = dvar_out != nullptr;
    if (wb) {
      hipLaunchKernelGGL(k_post_tau, dim3((unsigned)((mp * kq + 255) / 256)), dim3(256), 0, c->stream, dY, (int)mp,
                         (int)mc, q, kq, g.Hs, g.Qinv, g.tau);
      HIPCHK(c, hipGetLastError());
      CHK(adhoc_gemm(c, ADHOC_POST_U,
                     {{GEMM_AK_BK, mkprob(c->tr.B, np, c->dW2, np, c->dW3, np, c->NB, mt, (int)np, G_KBEG_TI, 1.0, 0.0)},
                      {GEMM_PLAIN, mkprob(g.Gq, np, g.tau, mp, c->dW3, np, c->NB, mt, kq, 0, 1.0, 1.0)}}));
    }
    PostGradArgs a;
    a.xw = c->dXw; a.xsw = c->dXsw; a.gam = c->dWa; a.U = wb ? c->dW3 : nullptr; a.ldu = np;
    a.part = g.part; a.n = (int)c->n; a.np = (int)np; a.mp = (int)mp; a.d = d; a.nsplit = grad_nsplit(mp);
    const dim3 grid((unsigned)(mp / PG_PTS), (unsigned)a.nsplit, (unsigned)(d > 32 ? (d + PG_WIDE - 1) / PG_WIDE : 1));
    CHK(chunk_prof_begin(c));
    if (wb) launch_post_grad<true>(fam, d, grid, c->stream, a);
    else launch_post_grad<false>(fam, d, grid, c->stream, a);
    HIPCHK(c, hipGetLastError());
    CHK(chunk_prof_end(c));
    PostGradFin f;
    f.part = g.part; f.invdelta = c->dinvdelta; f.dHs = g.dHs; f.hdim = g.hdim; f.beta = g.beta; f.tau = g.tau;
    f.dmean = g.dmean; f.dvar = wb ? g.dvar : nullptr; f.coff = coff; f.s2 = s2;
    f.nsplit = a.nsplit; f.mp = (int)mp; f.mc = (int)mc; f.d = d; f.q = q;
    hipLaunchKernelGGL(k_post_grad_fin, dim3((unsigned)((md + 255) / 256)), dim3(256), 0, c->stream, f);
    HIPCHK(c, hipGetLastError());
    // (dmean and dvar are adjacent: mp0 x d each)
    HIPCHK(c, hipMemcpyAsync(gpin_out[slot], g.dmean, md * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (wb)
      HIPCHK(c, hipMemcpyAsync(gpin_out[slot] + (size_t)mp0 * d, g.dvar, md * sizeof(double), hipMemcpyDeviceToHost,
                               c->stream));
    return GPE_OK;
  }

  // Per-point host algebra, from the chunk's Y = K*^T [gamma, G] (Yh, mp x P column-major):
  // the mean Y_0 + hs . beta into mean_out, and row(o, (T Kq^-T)_o) for o < q, T = Hs - K*^T G.
  template <class Row>
  void point(const double* Yh, long long mp, long long s0, long long s, Row&& row) const {
    const double* hs = Hs + (s0 + s) * q;
    double mu = Yh[s];
    for (int i = 0; i < q; ++i) mu += hs[i] * beta[i];
    mean_out[s0 + s] = mu;
    for (int o = 0; o < q; ++o) {
      double acc = 0.0;
      for (int i = 0; i < q; ++i) acc += (hs[i] - Yh[s + (long long)(i + 1) * mp]) * Kinv[o * q + i];
      row(o, acc);
    }
  }

  // Diagonal variance, pipelined: chunk i's device work (and the copy of its Y and column
  // norms into pinned slot i % 2) is queued before the host turns chunk i - 1's results
  // into means and variances, so the GPU does not idle on the host between chunks.
  int diag() {
    auto host_chunk = [&](long long s0, const double* out) {
      const long long mc = std::min(CHUNK, m - s0), mp = pad_to(mc, TILE);
      const double* nrm = out + (size_t)mp * P;
      for (long long s = 0; s < mc; ++s) {
        double tq = 0.0;   // |T Kq^-T|^2
        point(out, mp, s0, s, [&](int, double acc) { tq += acc * acc; });
        var_out[s0 + s] = s2 * (cdiag - nrm[s] + tq);
      }
    };
    // the chunk's gradients out of its pinned slot (row-major, the points contiguous)
    auto host_grad = [&](long long s0, const double* out) {
      const size_t cnt = (size_t)std::min(CHUNK, m - s0) * d;
      std::memcpy(dmean_out + s0 * d, out, cnt * sizeof(double));
      if (dvar_out) std::memcpy(dvar_out + s0 * d, out + (size_t)mp0 * d, cnt * sizeof(double));
    };
    auto dev = [&](long long s0, int slot) -> int {
      const long long mp = pad_to(std::min(CHUNK, m - s0), TILE);
      double* dY = c->dsmall + slot * rs;
      double* dn = dY + (size_t)mp * P;
      CHK(dev_chunk(s0, pin_in[slot], dY, c->dW2));
      if (f32 && !ozp)
        hipLaunchKernelGGL(k_colnorm2_f32, dim3((unsigned)((mp + 3) / 4)), dim3(256), 0, c->stream,
                           c->dK32 + (size_t)np * mp, np, (int)np, (int)mp, dn);
      else
        hipLaunchKernelGGL(k_colnorm2, dim3((unsigned)((mp + 3) / 4)), dim3(256), 0, c->stream, c->dW2, np,
                           (int)np, (int)mp, dn);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(pin_out[slot], dY, ((size_t)mp * P + mp) * sizeof(double), hipMemcpyDeviceToHost,
                               c->stream));
      if (grad) CHK(grad_chunk(s0, slot, dY));
      HIPCHK(c, hipEventRecord(c->ev_pipe[slot], c->stream));
      return GPE_OK;
    };
    return run_chunks(c, m, CHUNK, dev, [&](long long s0, int slot) {
      host_chunk(s0, pin_out[slot]);
      if (grad) host_grad(s0, gpin_out[slot]);
    });
  }

  // k_post_groupgram<NT> for items of cw columns
  void launch_groupgram(int cw, dim3 g, const GroupGramArgs& a) {
    const dim3 b(256);
    if (cw <= 16) hipLaunchKernelGGL(k_post_groupgram<1>, g, b, 0, c->stream, a);
    else if (cw <= 32) hipLaunchKernelGGL(k_post_groupgram<2>, g, b, 0, c->stream, a);
    else if (cw <= 48) hipLaunchKernelGGL(k_post_groupgram<3>, g, b, 0, c->stream, a);
    else hipLaunchKernelGGL(k_post_groupgram<4>, g, b, 0, c->stream, a);
  }

  // The blocks of groups of points, through diag()'s pipeline: behind a chunk's dev_chunk the
  // two kernels of gpemu_postgroup.hpp leave coff rho - v_a . v_b (cdiag - |v_a|^2 on the
  // diagonal) behind Y in the result slot; the host adds t_a . t_b, t = T Kq^-T of point(),
  // and scales by s2, keeping the rows of T of one group at a time.
  int group_blocks() {
    const int G = group;
    const long long GG = (long long)G * G;
    std::vector<double> Tg((size_t)G * q);
    auto host_chunk = [&](long long s0, const double* out) {
      const long long mc = std::min(CHUNK, m - s0), mp = pad_to(mc, TILE);
      const double* cv = out + (size_t)mp * P;
      for (long long g = 0; g < mc / G; ++g) {
        for (int a = 0; a < G; ++a)
          point(out, mp, s0, g * G + a, [&](int o, double acc) { Tg[(size_t)a * q + o] = acc; });
        const double* src = cv + g * GG;
        double* dst = var_out + (s0 / G + g) * GG;
        for (int a = 0; a < G; ++a)
          for (int b = 0; b <= a; ++b) {
            double tt = 0.0;
            for (int o = 0; o < q; ++o) tt += Tg[(size_t)a * q + o] * Tg[(size_t)b * q + o];
            const double v = s2 * (src[a * G + b] + tt);
            dst[a * G + b] = v;
            dst[b * G + a] = v;
          }
      }
    };
    auto dev = [&](long long s0, int slot) -> int {
      const long long mc = std::min(CHUNK, m - s0), mp = pad_to(mc, TILE);
      double* dY = c->dsmall + slot * rs;
      double* dcov = dY + (size_t)mp * P;
      CHK(dev_chunk(s0, pin_in[slot], dY, c->dW2));
      GroupGramArgs a;
      a.V = c->dW2; a.ldv = np; a.part = c->dPgc; a.np = (int)np; a.G = G; a.gpi = pgc_gpi(G);
      a.ngroups = (int)(mc / G);
      GroupCovArgs f;
      f.part = c->dPgc; f.xsw = c->dXsw; f.cov = dcov; f.coff = coff; f.cdiag = cdiag;
      f.nseg = pgc_nseg(np); f.ngroups = a.ngroups; f.G = G; f.d = d;
      CHK(chunk_prof_begin(c));
      launch_groupgram(a.gpi * G, dim3((unsigned)((a.ngroups + a.gpi - 1) / a.gpi), (unsigned)f.nseg), a);
      HIPCHK(c, hipGetLastError());
      const dim3 fg((unsigned)((a.ngroups * GG + 255) / 256));
      with_fam(fam, [&](auto F) { hipLaunchKernelGGL(k_post_groupcov<decltype(F)::value>, fg, dim3(256), 0, c->stream, f); });
      HIPCHK(c, hipGetLastError());
      CHK(chunk_prof_end(c));
      HIPCHK(c, hipMemcpyAsync(pin_out[slot], dY, ((size_t)mp * P + (size_t)mc * G) * sizeof(double),
                               hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipEventRecord(c->ev_pipe[slot], c->stream));
      return GPE_OK;
    };
    return run_chunks(c, m, CHUNK, dev, [&](long long s0, int slot) { host_chunk(s0, pin_out[slot]); });
  }

  // One block of the covariance, dst (ld) = s2 (A** - V_R^T V_C + T_R T_C^T) for the points R
  // (rows) and C (columns): the pair kernel (dg: a diagonal block, its lower tiles mirrored,
  // identity padding and s2 * rnew_scale * rnew on the diagonal), then the two products.
  // t_stage > 0: that many doubles of R.T wait in the pinned buffer and are uploaded behind
  // the pair kernel (the single chunk, whose T lives behind the block).
  int cov_block(const CovSide& R, const CovSide& C, double* dst, long long ld, bool dg, size_t t_stage = 0) {
    const int mt = (int)(R.mp / TILE), nt = (int)(C.mp / TILE);
    PairArgs a;
    a.xr = R.X; a.xc = C.X; a.out = dst; a.ld = ld; a.d = d;
    a.nr_valid = (int)R.mc; a.nc_valid = (int)C.mc; a.mt = mt; a.nt = nt; a.mode = dg ? (1 | 2 | 4) : 0;
    a.s2 = s2; a.coff = coff; a.cdiag = cdiag; a.rscale = 0.0; a.r = nullptr;
    a.fam = fam;
    if (dg && rnew) {
      CHK(grow_buf(c, &c->dRn, &c->rn_cap, (size_t)R.mp));
      // (synchronous copy; padded rows do not read r)
      HIPCHK(c, hipMemcpy(c->dRn, rnew + R.s0, (size_t)R.mc * sizeof(double), hipMemcpyHostToDevice));
      a.r = c->dRn;
      a.rscale = s2 * rnew_scale;
    }
    CHK(launch_pairs(c, a, dg ? mt * (mt + 1) / 2 : mt * nt));
    if (t_stage)
      HIPCHK(c, hipMemcpyAsync(R.T, c->hpin, t_stage * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return adhoc_gemm(c, ADHOC_COV, {{GEMM_AK_BK, mkprob(R.V, np, C.V, np, dst, ld, mt, nt, (int)np, 0, -s2, 1.0)},
                                     {GEMM_PLAIN, mkprob(R.T, R.ldt, C.T, C.ldt, dst, ld, mt, nt, kq, 0, s2, 1.0)}});
  }

  // Full variance.  One chunk: its block in dW3, copied out unless it stays there.  More:
  // every chunk's V, scaled points and T Kq^-T are kept, then the blocks of the lower
  // (FULL_DEV) or upper (FULL, mirrored on the host) triangle of chunk pairs are formed.
  int full_var() {
    std::vector<double> Th;   // every point's T Kq^-T (mtot x kq column-major)
    if (big) Th.assign((size_t)mtot * kq, 0.0);
    for (long long s0 = 0; s0 < m; s0 += CHUNK) {
      const long long mc = std::min(CHUNK, m - s0), mp = pad_to(mc, TILE);
      double* dY = c->dsmall;
      CHK(dev_chunk(s0, pin_in[0], dY, big ? c->dVall + s0 * np : c->dW2));
      std::vector<double> Yh((size_t)mp * P);
      HIPCHK(c, hipMemcpyAsync(pin_out[0], dY, (size_t)mp * P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      std::memcpy(Yh.data(), pin_out[0], Yh.size() * sizeof(double));
      if (big) {
        // keep this chunk's scaled points and T Kq^-T for the blocks formed after the loop
        HIPCHK(c, hipMemcpyAsync(c->dXall + s0 * d, c->dXsw, (size_t)mp * d * sizeof(double),
                                 hipMemcpyDeviceToDevice, c->stream));
        for (long long s = 0; s < mc; ++s)
          point(Yh.data(), mp, s0, s, [&](int o, double acc) { Th[(s0 + s) + (size_t)o * mtot] = acc; });
        continue;
      }
      // C (mp x mp, all tiles: full symmetric), then T Kq^-T (mp x kq column-major) behind it
      const size_t needc = (size_t)mp * mp, nt = (size_t)mp * kq;
      CHK(grow_buf(c, &c->dW3, &c->w3_cap, needc + nt));
      double* dC = c->dW3;
      CHK(ensure_pinned(c, nt + 64));
      std::memset(c->hpin, 0, nt * sizeof(double));
      for (long long s = 0; s < mc; ++s)
        point(Yh.data(), mp, s0, s, [&](int o, double acc) { c->hpin[s + (size_t)o * mp] = acc; });
      const CovSide side{c->dXsw, c->dW2, dC + needc, mp, s0, mc, mp};
      CHK(cov_block(side, side, dC, mp, true, nt));
      // (FULL_DW3: the caller reuses the pinned staging buffer)
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if (var == PostVar::FULL_DW3) return GPE_OK;
      // copy out m x m (col-major == row-major for the symmetric result)
      std::vector<double> hc((size_t)mp * mc);
      HIPCHK(c, hipMemcpy(hc.data(), dC, hc.size() * sizeof(double), hipMemcpyDeviceToHost));
      for (long long j = 0; j < mc; ++j)
        std::memcpy(var_out + j * m, hc.data() + (size_t)j * mp, (size_t)mc * sizeof(double));
    }
    if (big) CHK(blocks(Th));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GPE_OK;
  }

  // the chunk-pair blocks of a full variance of more than one chunk (Th: every point's T Kq^-T)
  int blocks(const std::vector<double>& Th) {
    HIPCHK(c, hipMemcpyAsync(c->dTall, Th.data(), Th.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const bool dev = var == PostVar::FULL_DEV;
    if (!dev) CHK(grow_buf(c, &c->dW3, &c->w3_cap, (size_t)CHUNK * CHUNK));
    double* dC = c->dW3;
    std::vector<double> hc;
    auto side = [&](long long s0) {
      const long long mc = std::min(CHUNK, m - s0);
      return CovSide{c->dXall + s0 * d, c->dVall + s0 * np, c->dTall + s0, mtot, s0, mc, pad_to(mc, TILE)};
    };
    for (long long a0 = 0; a0 < m; a0 += CHUNK)
      for (long long b0 = a0; b0 < m; b0 += CHUNK) {
        const CovSide A = side(a0), B = side(b0);
        const bool dg = a0 == b0;
        if (dev) {
          // block (b, a) of the lower triangle straight into dev_out (ld = mtot): rows of
          // chunk b, columns of chunk a.  Padded rows / columns come out 0 off the
          // diagonal (zero K*, V and T there) and identity on it (the pair kernel).
          CHK(cov_block(B, A, dev_out + b0 + a0 * mtot, mtot, dg));
          // the descriptors are re-uploaded for the next block: drain before overwriting
          HIPCHK(c, hipStreamSynchronize(c->stream));
          continue;
        }
        // block (a, b) in dW3 (ld = mpa), written to the host at rows a, columns b (and mirrored)
        CHK(cov_block(A, B, dC, A.mp, dg));
        hc.resize((size_t)A.mp * B.mp);
        HIPCHK(c, hipMemcpyAsync(hc.data(), dC, hc.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        // dC(i, j) = C(a0 + i, b0 + j), column-major; var_out row-major m x m
        for (long long j = 0; j < B.mc; ++j)
          for (long long i = 0; i < A.mc; ++i) {
            const double v = hc[(size_t)i + (size_t)j * A.mp];
            var_out[(a0 + i) * m + (b0 + j)] = v;
            if (!dg) var_out[(b0 + j) * m + (a0 + i)] = v;
          }
      }
    return GPE_OK;
  }
};

int posterior_impl(gpe_ctx* c, const PostReq& r) {
  CHK(check_ready(c));
  if (!c->factor_valid) return fail(c, GPE_ERR_STATE, "no resident factor (call gpe_factor)");
  const bool to_host = r.var == PostVar::DIAG || r.var == PostVar::FULL || r.var == PostVar::GROUPS;
  if (r.m <= 0 || !r.Xs || !r.Hs || !r.beta || !r.mean_out || (to_host && !r.var_out))
    return fail(c, GPE_ERR_ARG, "bad posterior args");
  if ((r.var == PostVar::FULL_DW3 && r.m > POST_CHUNK_FULL) ||
      (r.var == PostVar::FULL_DEV && (r.m <= POST_CHUNK_FULL || !r.dev_out)))
    return fail(c, GPE_ERR_ARG, "device-resident variance: one chunk in place, beyond one chunk a device target");
  if (r.var == PostVar::GROUPS && (r.group < 1 || r.group > PGC_MAXG || r.m % r.group != 0 || r.precision != 64))
    return fail(c, GPE_ERR_ARG, "bad posterior_groups args (1 <= G <= 64, m a multiple of G)");
  if (r.precision != 64 && r.precision != 32) return fail(c, GPE_ERR_ARG, "precision must be 64 or 32");
  if (r.precision == 32 && r.var != PostVar::DIAG)
    return fail(c, GPE_ERR_UNSUPPORTED, "precision 32 is for the diagonal variance");
  if (r.dmean_out) {
    if (r.var != PostVar::DIAG || r.precision != 64 || !r.dHs || !r.hdim)
      return fail(c, GPE_ERR_ARG, "bad posterior_grad args");
    for (int j = 0; j < c->q; ++j)
      if (r.hdim[j] < -1 || r.hdim[j] >= c->d)
        return fail(c, GPE_ERR_ARG, "hdim[" + std::to_string(j) + "] is outside [-1, d)");
  }
  CHK(ensure_linv(c));
  Posterior S(c, r);
  CHK(S.setup());
  CHK(S.workspace());
  return S.full ? S.full_var() : S.groups ? S.group_blocks() : S.diag();
}

// k_post_mean<DMAX, FAM, WIDE> for d inputs (the widths of launch_post_grad_fam)
template <int FAM>
void launch_post_mean_fam(int d, dim3 g, hipStream_t st, const PostMeanArgs& a) {
  const dim3 b(PM_LANES);
  if (d > 32) hipLaunchKernelGGL((k_post_mean<PM_WIDE, FAM, true>), g, b, 0, st, a);
  else
    with_width(RegWidths(), d, [&](auto W) {
      hipLaunchKernelGGL((k_post_mean<decltype(W)::value, FAM, false>), g, b, 0, st, a);
    });
}

// k_post_mean_multi<DMAX, FAM, WIDE, NCB> for d inputs (launch_post_mean_fam's widths) and p
// outputs in NCB blocks of 16
template <int FAM, int NCB>
void launch_post_mean_multi_ncb(int d, dim3 g, hipStream_t st, const PostMeanMultiArgs& a) {
  const dim3 b(PM_LANES);
  if (d > 32) hipLaunchKernelGGL((k_post_mean_multi<PM_WIDE, FAM, true, NCB>), g, b, 0, st, a);
  else
    with_width(RegWidths(), d, [&](auto W) {
      hipLaunchKernelGGL((k_post_mean_multi<decltype(W)::value, FAM, false, NCB>), g, b, 0, st, a);
    });
}
template <int FAM>
void launch_post_mean_multi_fam(int d, dim3 g, hipStream_t st, const PostMeanMultiArgs& a) {
  switch ((a.p + 15) / 16) {
    case 1: launch_post_mean_multi_ncb<FAM, 1>(d, g, st, a); break;
    case 2: launch_post_mean_multi_ncb<FAM, 2>(d, g, st, a); break;
    case 3: launch_post_mean_multi_ncb<FAM, 3>(d, g, st, a); break;
    default: launch_post_mean_multi_ncb<FAM, 4>(d, g, st, a); break;
  }
}

// What gpe_posterior_mean and gpe_posterior_mean_multi differ in, for posterior_means()
struct MeanKind {
  int p;                // values per point
  double** part;        // the partial sums, (nseg + 1) p per point: c->dPm, c->dPmm
  size_t* part_cap;
  const double* coef;   // the host adds hs . coef: beta (q), B (q x p row-major)
  size_t pin_route;     // pinned doubles behind 1 / delta for the route to gamma
};

// The posterior means of one kind at m points, with gamma resident or queued by route().  Per
// chunk: the points' upload, k_scale_points, kernels(mp, nseg, part, dY, coff, fam) -- the
// kind's fused kernel inside the profiling bracket and its finishing kernel -- and the copy of
// y into a pinned slot; the host adds hs . coef as Posterior::point does.  Two pinned slots of
// points and two of results: chunk i + 1's upload and kernels are queued before the host
// finishes chunk i.  Device workspace: the chunk's points twice and its (nseg + 1) p sums per
// point.  route(pin) runs behind the upload of 1 / delta, with pin_route pinned doubles.
// P1: the kind's p where the compiler is to know it (1: the host's loop over 1e6 points is then
// the single-output one, measurably faster than the general one at p = 1), 0 for any p.
template <int P1, class Route, class Kernels>
int posterior_means(gpe_ctx* c, const MeanKind& k, int64_t m, const double* Xs, const double* Hs, double* mean_out,
                    Route&& route, Kernels&& kernels) {
  const int d = c->d, q = c->q, p = P1 ? P1 : k.p;
  const long long np = c->n_pad, CH = c->mean_chunk;
  const long long mp0 = pad_to(std::min<long long>(CH, m), PM_PTS);
  const int nrt = (int)(np / PM_RI), nseg = (nrt + PM_SEG - 1) / PM_SEG;
  CHK(grow_buf(c, &c->dXs, &c->xs_cap, (size_t)mp0 * d));
  CHK(grow_buf(c, &c->dXsw, &c->xsw_cap, (size_t)mp0 * d));
  CHK(grow_buf(c, k.part, k.part_cap, (size_t)(nseg + 1) * p * mp0));
  double* dY = *k.part + (size_t)nseg * p * mp0;
  CHK(ensure_pinned(c, 2 * (size_t)mp0 * d + 2 * (size_t)mp0 * p + d + k.pin_route + 64));
  double* pin_in[2] = {c->hpin, c->hpin + (size_t)mp0 * d};
  double* pin_out[2] = {pin_in[1] + (size_t)mp0 * d, pin_in[1] + (size_t)mp0 * d + (size_t)mp0 * p};
  double* pin_dl = pin_out[1] + (size_t)mp0 * p;   // 1 / delta
  CHK(upload_invdelta(c, pin_dl));
  CHK(route(pin_dl + d));
  double coff, cdiag;
  kernel_consts(c->f_kernel, c->f_nu, true, &coff, &cdiag);
  const int fam = kernel_fam(c->f_kernel);
  CHK(pipe_events(c));
  auto dev_chunk = [&](long long s0, int slot) -> int {
    const long long mc = std::min(CH, m - s0), mp = pad_to(mc, PM_PTS);
    std::memcpy(pin_in[slot], Xs + s0 * d, (size_t)mc * d * sizeof(double));
    // (k_scale_points reads the mc points only and writes zeros for the padded ones)
    HIPCHK(c, hipMemcpyAsync(c->dXs, pin_in[slot], (size_t)mc * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_scale_points, dim3((unsigned)((mp * d + 255) / 256)), dim3(256), 0, c->stream, c->dXs,
                       c->dinvdelta, d, (int)mc, (int)mp, c->dXsw);
    HIPCHK(c, hipGetLastError());
    CHK(kernels(mp, nseg, *k.part, dY, coff, fam));
    HIPCHK(c, hipMemcpyAsync(pin_out[slot], dY, (size_t)mc * p * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_pipe[slot], c->stream));
    return GPE_OK;
  };
  return run_chunks(c, m, CH, dev_chunk, [&](long long s0, int slot) {
    const long long mc = std::min(CH, m - s0);
    const double* y = pin_out[slot];
    for (long long s = 0; s < mc; ++s) {
      const double* hs = Hs + (s0 + s) * q;
      for (int a = 0; a < p; ++a) {
        double mu = y[s * p + a];
        for (int i = 0; i < q; ++i) mu += hs[i] * k.coef[i * p + a];
        mean_out[(s0 + s) * p + a] = mu;
      }
    }
  });
}

// The posterior mean alone (gpe_posterior_mean): gamma from Posterior::setup(), k_post_mean
// with one workgroup per column of points and segment of rows.
int posterior_mean_impl(gpe_ctx* c, int64_t m, const double* Xs, const double* Hs, const double* beta,
                        double* mean_out) {
  CHK(check_ready(c));
  if (!c->factor_valid) return fail(c, GPE_ERR_STATE, "no resident factor (call gpe_factor)");
  if (m <= 0 || !Xs || !Hs || !beta || !mean_out)
    return fail(c, GPE_ERR_ARG, "bad posterior_mean args (m >= 1; Xs, Hs, beta and mean_out not NULL)");
  if (c->prof)   // phase 0: k_post_mean's device time over the chunks, phase 1: the chunks
    for (int i = 0; i < 8; ++i) c->phase_ms[i] = 0.0;
  CHK(ensure_linv(c));
  PostReq r{m, Xs, Hs, beta, 1.0, 64, mean_out, PostVar::DIAG, nullptr};
  Posterior S(c, r);
  CHK(S.setup());   // gamma in dWa's first column
  const int d = c->d;
  const MeanKind kind{1, &c->dPm, &c->pm_cap, beta, 0};
  return posterior_means<1>(
      c, kind, m, Xs, Hs, mean_out, [](double*) { return GPE_OK; },
      [&](long long mp, int nseg, double* part, double* dY, double coff, int fam) -> int {
        PostMeanArgs a;
        a.xw = c->dXw; a.xsw = c->dXsw; a.gam = c->dWa; a.part = part; a.coff = coff;
        a.n = (int)c->n; a.np = (int)c->n_pad; a.mp = (int)mp; a.d = d;
        const dim3 grid((unsigned)(mp / (d > 32 ? PM_LANES : PM_PTS)), (unsigned)nseg);
        CHK(chunk_prof_begin(c));
        with_fam(fam, [&](auto F) { launch_post_mean_fam<decltype(F)::value>(d, grid, c->stream, a); });
        HIPCHK(c, hipGetLastError());
        CHK(chunk_prof_end(c));
        hipLaunchKernelGGL(k_post_mean_fin, dim3((unsigned)((mp + 255) / 256)), dim3(256), 0, c->stream, part, nseg,
                           (int)mp, dY);
        HIPCHK(c, hipGetLastError());
        return GPE_OK;
      });
}

// Gamma = A^-1 (F - H B) of the p outputs of gpe_set_outputs into the first p columns of dWm, by
// Posterior::setup()'s route to gamma (L^-1, then L^-T, of the columns); queued on the
// context's stream.  pin_t: (p + q) p pinned doubles for [I; -B].  L^-1 must be resident
// (ensure_linv).  For gpe_posterior_mean_multi and gpe_hm_add_multi.
int multi_gamma(gpe_ctx* c, const double* B, double* pin_t) {
  const int q = c->q, p = c->mo_p, P = p + q;
  const long long np = c->n_pad;
  std::memset(pin_t, 0, (size_t)P * p * sizeof(double));   // [I; -B] (P x p, column-major)
  for (int a = 0; a < p; ++a) {
    pin_t[a + (size_t)a * P] = 1.0;
    for (int i = 0; i < q; ++i) pin_t[(p + i) + (size_t)a * P] = -B[i * p + a];
  }
  HIPCHK(c, hipMemcpyAsync(c->dT2, pin_t, (size_t)P * p * sizeof(double), hipMemcpyHostToDevice, c->stream));
  CHK(apply_small(c, c->dFm, np, P, c->dT2, p, c->dR2m, np, (int)np, nullptr));
  CHK(skinny(c, false, c->tr.B, np, c->NB, c->NB, true, c->dR2m, np, p, c->dZm, np));   // L^-1 (F - H B)
  return skinny(c, true, c->tr.B, np, c->NB, c->NB, true, c->dZm, np, p, c->dWm, np);   // Gamma
}

// The posterior means of the p outputs of gpe_set_outputs (gpe_posterior_mean_multi): Gamma by
// multi_gamma, k_post_mean_multi with one workgroup per PMM_PTS points and segment of rows.
int posterior_mean_multi_impl(gpe_ctx* c, int64_t m, const double* Xs, const double* Hs, const double* B,
                              double* mean_out) {
  CHK(check_ready(c));
  if (!c->factor_valid) return fail(c, GPE_ERR_STATE, "no resident factor (call gpe_factor)");
  if (!c->mo_p) return fail(c, GPE_ERR_STATE, "gpe_set_outputs has not been called for this data");
  if (m <= 0 || !Xs || !Hs || !B || !mean_out)
    return fail(c, GPE_ERR_ARG, "bad posterior_mean_multi args (m >= 1; Xs, Hs, B and mean_out not NULL)");
  if (c->prof)   // phase 0: k_post_mean_multi's device time over the chunks, phase 1: the chunks
    for (int i = 0; i < 8; ++i) c->phase_ms[i] = 0.0;
  CHK(ensure_linv(c));
  const int d = c->d, p = c->mo_p, P = p + c->q;
  const long long np = c->n_pad;
  static_assert(PM_PTS % PMM_PTS == 0, "a padded chunk is whole workgroups of k_post_mean_multi");
  const MeanKind kind{p, &c->dPmm, &c->pmm_cap, B, (size_t)P * p};
  return posterior_means<0>(
      c, kind, m, Xs, Hs, mean_out,
      [&](double* pin_t) -> int { return multi_gamma(c, B, pin_t); },
      [&](long long mp, int nseg, double* part, double* dY, double coff, int fam) -> int {
        PostMeanMultiArgs a;
        a.xw = c->dXw; a.xsw = c->dXsw; a.gam = c->dWm; a.part = part; a.coff = coff;
        a.n = (int)c->n; a.np = (int)np; a.mp = (int)mp; a.d = d; a.p = p;
        const dim3 grid((unsigned)(mp / PMM_PTS), (unsigned)nseg);
        CHK(chunk_prof_begin(c));
        with_fam(fam, [&](auto F) { launch_post_mean_multi_fam<decltype(F)::value>(d, grid, c->stream, a); });
        HIPCHK(c, hipGetLastError());
        CHK(chunk_prof_end(c));
        hipLaunchKernelGGL(k_post_mean_multi_fin, dim3((unsigned)((mp * p + 255) / 256)), dim3(256), 0, c->stream,
                           part, nseg, p, (int)mp, dY);
        HIPCHK(c, hipGetLastError());
        return GPE_OK;
      });
}

// The greedy selections' profiling (gpe_posterior_pivchol, gpe_posterior_imse): what ran since
// ev[0], the covariance and the set-up, into phase_ms[0]; ev[1] then opens the first panel.
int panels_prof_begin(gpe_ctx* c) {
  if (!c->prof) return GPE_OK;
  float ms = 0.f;
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipEventSynchronize(c->ev[1]));
  (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
  c->phase_ms[0] = ms;
  return GPE_OK;
}

// Their k steps in panels of PC_PANEL columns: step(t0, j) for the panel's columns, the
// trailing update Lt if steps remain, then tail(t0, cols).  Profiling adds the steps' device
// time to phase_ms[1] and the update's and tail's to phase_ms[2] (one synchronisation per panel).
template <class Step, class Tail>
int run_panels(gpe_ctx* c, long long k, const GemmLaunch& Lt, Step&& step, Tail&& tail) {
  for (long long t0 = 0; t0 < k; t0 += PC_PANEL) {
    const int cols = (int)std::min<long long>(PC_PANEL, k - t0);
    for (int j = 0; j < cols; ++j) CHK(step(t0, j));
    if (c->prof) HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    if (t0 + cols < k) CHK(launch_gemm_range(c, Lt));
    CHK(tail(t0, cols));
    if (c->prof) {
      float ms = 0.f;
      HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
      HIPCHK(c, hipEventSynchronize(c->ev[3]));
      (void)hipEventElapsedTime(&ms, c->ev[1], c->ev[2]);
      c->phase_ms[1] += ms;
      (void)hipEventElapsedTime(&ms, c->ev[2], c->ev[3]);
      c->phase_ms[2] += ms;
      HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    }
  }
  return GPE_OK;
}

}  // namespace

extern "C" {

int gpe_posterior_mean_multi(gpe_ctx* c, int64_t m, const double* Xs, const double* Hs, const double* B,
                             double* mean_out) {
  return posterior_mean_multi_impl(c, m, Xs, Hs, B, mean_out);
}

int gpe_posterior(gpe_ctx* c, int64_t m, const double* Xs, const double* Hs, const double* beta,
                  double sigma, int32_t full_var, int32_t precision, double* mean_out, double* var_out) {
  PostReq r{m, Xs, Hs, beta, sigma, precision, mean_out, full_var ? PostVar::FULL : PostVar::DIAG, var_out};
  return posterior_impl(c, r);
}

int gpe_posterior_grad(gpe_ctx* c, int64_t m, const double* Xs, const double* Hs, const double* dHs,
                       const int32_t* hdim, const double* beta, double sigma, double* mean_out, double* var_out,
                       double* dmean_out, double* dvar_out) {
  CHK(check_ready(c));
  if (!c->factor_valid) return fail(c, GPE_ERR_STATE, "no resident factor (call gpe_factor)");
  if (!dHs || !hdim || !dmean_out) return fail(c, GPE_ERR_ARG, "bad posterior_grad args");
  if (c->prof)   // phase 0: k_post_grad's device time over the chunks, phase 1: the chunks
    for (int i = 0; i < 8; ++i) c->phase_ms[i] = 0.0;
  PostReq r{m, Xs, Hs, beta, sigma, 64, mean_out, PostVar::DIAG, var_out};
  r.dHs = dHs;
  r.hdim = hdim;
  r.dmean_out = dmean_out;
  r.dvar_out = dvar_out;
  return posterior_impl(c, r);
}

int gpe_posterior_mean(gpe_ctx* c, int64_t m, const double* Xs, const double* Hs, const double* beta,
                       double* mean_out) {
  return posterior_mean_impl(c, m, Xs, Hs, beta, mean_out);
}

int gpe_posterior_groups(gpe_ctx* c, int64_t m, int32_t G, const double* Xs, const double* Hs, const double* beta,
                         double sigma, double* mean_out, double* cov_out) {
  CHK(check_ready(c));
  if (c->prof)   // phase 0: the group kernels' device time over the chunks, phase 1: the chunks
    for (int i = 0; i < 8; ++i) c->phase_ms[i] = 0.0;
  PostReq r{m, Xs, Hs, beta, sigma, 64, mean_out, PostVar::GROUPS, cov_out};
  r.group = G;
  return posterior_impl(c, r);
}

int gpe_noise_sample(gpe_ctx* c, int64_t m, const double* Xs, const double* Hs, const double* beta,
                     double sigma, const double* r_new, double r_scale, const double* t, int32_t s,
                     const double* U, double* mean_out, double* z_out) {
  CHK(check_ready(c));
  if (m <= 0 || m > (1LL << 20) || s <= 0 || !t || !U || !z_out)
    return fail(c, GPE_ERR_ARG, "bad noise_sample args (1 <= m <= 2^20, s >= 1)");
  const long long mp = ((m + TILE - 1) / TILE) * TILE;
  const int mt = (int)(mp / TILE);
  const long long sp = ((s + TILE - 1) / TILE) * TILE;
  const int st = (int)(sp / TILE);
  // V = posterior covariance at Xs (mp x mp, identity padding) into the aux workspace,
  // then L = chol(V) there (np.linalg.cholesky(post.var), noise_fit.py:131).  One chunk
  // (m <= 16384): formed in c->dW3 and copied; beyond, formed block by block in place.
  Fact& F = c->aux;
  CHK(ensure_fact(c, F, mp));
  CHK(build_plan(c, F));
  const bool one = m <= POST_CHUNK_FULL;
  PostReq r{m, Xs, Hs, beta, sigma, 64, mean_out, one ? PostVar::FULL_DW3 : PostVar::FULL_DEV, nullptr,
            one ? nullptr : F.A, r_new, r_scale};
  CHK(posterior_impl(c, r));
  if (one)
    HIPCHK(c, hipMemcpyAsync(F.A, c->dW3, (size_t)mp * mp * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(c->dinfo, 0, sizeof(int), c->stream));
  CHK(potrf(c, F));
  int info = 0;
  double logdet = 0.0;
  CHK(read_info_logdet(c, F, &info, &logdet));
  if (info != 0) {
    c->err = "posterior covariance not positive definite (pivot " + std::to_string(info) + ")";
    return GPE_NOT_PD;
  }
  hipLaunchKernelGGL(k_zero_upper_diag_tiles, dim3((unsigned)mt), dim3(256), 0, c->stream, F.A, mp);
  HIPCHK(c, hipGetLastError());
  // U^T (mp x sp, column j = draw j, zero padding) and e = t - mean
  CHK(grow_buf(c, &c->dNU, &c->nu_cap, 2 * (size_t)mp * sp + 2 * (size_t)mp));
  double* dU = c->dNU;
  double* dY = c->dNU + (size_t)mp * sp;
  double* dE = dY + (size_t)mp * sp;
  double* dZs = dE + mp;
  CHK(ensure_pinned(c, (size_t)mp * sp + 64));
  std::memset(c->hpin, 0, (size_t)mp * sp * sizeof(double));
  for (int j = 0; j < s; ++j) std::memcpy(c->hpin + (size_t)j * mp, U + (size_t)j * m, (size_t)m * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(dU, c->hpin, (size_t)mp * sp * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memset(c->hpin, 0, (size_t)mp * sizeof(double));
  for (long long i = 0; i < m; ++i) c->hpin[i] = t[i] - mean_out[i];
  HIPCHK(c, hipMemcpyAsync(dE, c->hpin, (size_t)mp * sizeof(double), hipMemcpyHostToDevice, c->stream));
  // Y = L U^T: the s draws L.dot(u) of noise_fit.py:135-136 as one MFMA GEMM
  CHK(adhoc_gemm(c, ADHOC_NOISE, {{GEMM_BK, mkprob(F.A, mp, dU, mp, dY, mp, mt, st, (int)mp, G_KEND_TI, 1.0, 0.0)}}));
  // z_i = sum_j 0.5 (e_i - Y_ij)^2  (noise_fit.py:137)
  hipLaunchKernelGGL(k_noise_sq, dim3((unsigned)(mp / 256 + 1)), dim3(256), 0, c->stream, dY, mp, s, dE,
                     (int)m, dZs);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->hpin, dZs, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memcpy(z_out, c->hpin, (size_t)m * sizeof(double));
  return GPE_OK;
}

// Greedy pivoted Cholesky of the posterior covariance (include/gpemu.h).  The
// covariance is formed in c->dW3 as for gpe_noise_sample, then one k_pc_step launch per pivot
// (gpemu_pivchol.hpp) works in panels of PC_PANEL columns: after a full panel with steps left,
// S -= W W^T over the whole m_pad x m_pad matrix (rows and columns already chosen receive
// values nobody reads), so a step reads at most PC_PANEL earlier columns; with L_out, every
// panel is then transposed into the row-major device copy of L (k_pc_panel_out).  All k steps
// are queued without a synchronisation; the stop rule is the device's, and the rank, the
// pivots and their variances are read once at the end.
int gpe_posterior_pivchol(gpe_ctx* c, int64_t m, const double* Xs, const double* Hs, const double* beta,
                          double sigma, const double* r_new, double r_scale, int64_t k, double tol,
                          double* mean_out, int64_t* piv_out, double* pivvar_out, double* L_out,
                          int64_t* rank_out) {
  CHK(check_ready(c));
  if (!c->factor_valid) return fail(c, GPE_ERR_STATE, "no resident factor (call gpe_factor)");
  if (m <= 0 || !Xs || !Hs || !beta || !mean_out || !piv_out || !pivvar_out || !rank_out)
    return fail(c, GPE_ERR_ARG, "bad pivchol args");
  if (m > 16384)
    return fail(c, GPE_ERR_UNSUPPORTED, "pivoted Cholesky takes at most 16384 points (one posterior chunk)");
  if (k < 1 || k > m || !(tol >= 0.0)) return fail(c, GPE_ERR_ARG, "bad pivchol args (1 <= k <= m, tol >= 0)");
  const long long mp = ((m + TILE - 1) / TILE) * TILE;
  const int mt = (int)(mp / TILE);
  const int G = (int)(mp / PC_ROWS);
  if (c->prof) {
    for (int i = 0; i < 8; ++i) c->phase_ms[i] = 0.0;
    HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  }
  PostReq r{m, Xs, Hs, beta, sigma, 64, mean_out, PostVar::FULL_DW3, nullptr, nullptr, r_new, r_scale};
  CHK(posterior_impl(c, r));
  // workspace: [state | pivvar (k) | piv (k ints)] (read back in one copy), d (m_pad), the
  // partial maxima (2 G), then the ints: flags (m_pad) and partial indices (2 G)
  const size_t kh = (size_t)(k + 1) / 2;
  const size_t head = 2 + (size_t)k + kh;
  CHK(grow_buf(c, &c->dPc, &c->pc_cap, head + (size_t)mp + 2 * (size_t)G + (size_t)mp / 2 + (size_t)G));
  const size_t wsz = (size_t)mp * PC_PANEL;
  CHK(grow_buf(c, &c->dPcL, &c->pcl_cap, wsz + (L_out ? (size_t)m * (size_t)k : 0)));
  double* W = c->dPcL;
  double* Ld = c->dPcL + wsz;
  PcArgs a;
  a.S = c->dW3; a.ld = mp; a.m = (int)m; a.G = G;
  a.st = reinterpret_cast<PcState*>(c->dPc);
  a.pivvar = c->dPc + 2;
  a.piv = reinterpret_cast<int*>(c->dPc + 2 + k);
  a.d = c->dPc + head;
  a.pmax = a.d + mp;
  a.chosen = reinterpret_cast<int*>(a.pmax + 2 * (size_t)G);
  a.pidx = a.chosen + mp;
  a.tol = tol;
  static_assert(sizeof(PcState) == 2 * sizeof(double), "PcState");
  // the trailing update's descriptor: S -= W W^T, every tile, K = PC_PANEL (the same for every panel)
  GemmLaunch Lt{};
  if (k > PC_PANEL) {
    CHK(adhoc_gemm(c, ADHOC_PIVCHOL, {{GEMM_PLAIN, mkprob(W, mp, W, mp, c->dW3, mp, mt, mt, PC_PANEL, 0, -1.0, 1.0)}}, &Lt));
    Lt.flops = 2.0 * (double)mp * (double)mp * PC_PANEL;
  }
  hipLaunchKernelGGL(k_pc_init, dim3(G), dim3(PC_ROWS), 0, c->stream, a, (int)k);
  HIPCHK(c, hipGetLastError());
  CHK(panels_prof_begin(c));
  CHK(run_panels(
      c, k, Lt,
      [&](long long t0, int j) -> int {
        hipLaunchKernelGGL(k_pc_step, dim3(G), dim3(256), 0, c->stream, a, W, (int)(t0 + j), j);
        HIPCHK(c, hipGetLastError());
        return GPE_OK;
      },
      [&](long long t0, int cols) -> int {
        if (!L_out) return GPE_OK;
        // the panel into the row-major device copy of L (zeros beyond the rank)
        hipLaunchKernelGGL(k_pc_panel_out, dim3(G, (cols + 63) / 64), dim3(256), 0, c->stream, W, mp, (int)m, cols,
                           a.st, Ld, (long long)k, t0);
        HIPCHK(c, hipGetLastError());
        return GPE_OK;
      }));
  CHK(ensure_pinned(c, head + 8));
  HIPCHK(c, hipMemcpyAsync(c->hpin, c->dPc, head * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) c->phase_ms[6] = c->phase_ms[0] + c->phase_ms[1] + c->phase_ms[2];
  PcState st;
  std::memcpy(&st, c->hpin, sizeof(st));
  const long long rank = st.rank;
  if (rank < 0 || rank > k) return fail(c, GPE_ERR_HIP, "internal error: pivoted Cholesky rank out of range");
  const int* pv32 = reinterpret_cast<const int*>(c->hpin + 2 + k);
  for (long long t = 0; t < k; ++t) {
    piv_out[t] = t < rank ? pv32[t] : -1;
    pivvar_out[t] = t < rank ? c->hpin[2 + t] : 0.0;
  }
  *rank_out = rank;
  // the device copy is row-major m x k like L_out, columns >= rank written as zeros
  if (L_out) HIPCHK(c, hipMemcpy(L_out, Ld, (size_t)m * (size_t)k * sizeof(double), hipMemcpyDeviceToHost));
  return GPE_OK;
}

// Greedy integrated-variance (IMSE) batch among the first mc of the m points (include/gpemu.h;
// DESIGN.md).  The covariance is formed in c->dW3 as for gpe_posterior_pivchol; C, the
// reference rows of the candidate columns, is copied out of it, and then two launches per pick
// (gpemu_imse.hpp: k_im_col, k_im_sweep) work in panels of PC_PANEL picks: after a full panel
// with steps left, S -= W W^T over the candidate tiles, so k_im_col reads at most PC_PANEL
// earlier columns.  All k steps are queued without a synchronisation; the stop rule is the
// device's, and the state, picks, gains and variances are read once at the end.
int gpe_posterior_imse(gpe_ctx* c, int64_t m, int64_t mc, const double* Xs, const double* Hs, const double* beta,
                       double sigma, const double* r_new, double r_scale, const double* w, int64_t k, double tol,
                       double* mean_out, int64_t* piv_out, double* gain_out, double* pivvar_out,
                       double* imse0_out, int64_t* rank_out) {
  CHK(check_ready(c));
  if (!c->factor_valid) return fail(c, GPE_ERR_STATE, "no resident factor (call gpe_factor)");
  if (m <= 0 || !Xs || !Hs || !beta || !mean_out || !piv_out || !gain_out || !pivvar_out || !imse0_out || !rank_out)
    return fail(c, GPE_ERR_ARG, "bad imse args");
  if (m > 16384)
    return fail(c, GPE_ERR_UNSUPPORTED, "the integrated-variance design takes at most 16384 points (one posterior chunk)");
  if (mc < 1 || m - mc < 1 || k < 1 || k > mc || !(tol >= 0.0))
    return fail(c, GPE_ERR_ARG, "bad imse args (1 <= mc < m, 1 <= k <= mc, tol >= 0)");
  const long long mr = m - mc;
  if (w)
    for (long long r = 0; r < mr; ++r)
      if (!(w[r] >= 0.0)) return fail(c, GPE_ERR_ARG, "bad imse args (a weight is negative or NaN)");
  const long long mp = ((m + TILE - 1) / TILE) * TILE;
  const int mct = (int)((mc + TILE - 1) / TILE);
  const int Gc = mct * (TILE / PC_ROWS);
  const int Gs = (int)((mc + IM_NC - 1) / IM_NC);
  const long long mcp = (long long)Gc * PC_ROWS;
  const long long ldc = (mr + 1) / 2 * 2;
  if (c->prof) {
    for (int i = 0; i < 8; ++i) c->phase_ms[i] = 0.0;
    HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  }
  PostReq r{m, Xs, Hs, beta, sigma, 64, mean_out, PostVar::FULL_DW3, nullptr, nullptr, r_new, r_scale};
  CHK(posterior_impl(c, r));
  // workspace: [state | pivvar (k) | gain (k) | piv (k ints)] (read back in one copy, padded to
  // an even number of doubles: lambda and w are read 16 bytes at a time), d (mcp), lambda (ldc),
  // w (ldc), the partial scores (2 Gs), then the ints: flags (mcp) and partial indices (2 Gs)
  static_assert(sizeof(ImState) == 3 * sizeof(double), "ImState");
  const size_t kh = (size_t)(k + 1) / 2;
  const size_t head = (3 + 2 * (size_t)k + kh + 1) / 2 * 2;
  CHK(grow_buf(c, &c->dIm, &c->im_cap,
               head + (size_t)mcp + 2 * (size_t)ldc + 2 * (size_t)Gs + ((size_t)mcp + 2 * (size_t)Gs + 1) / 2));
  CHK(grow_buf(c, &c->dImC, &c->imc_cap, (size_t)ldc * (size_t)Gs * IM_NC));
  CHK(grow_buf(c, &c->dPcL, &c->pcl_cap, (size_t)mp * PC_PANEL));
  CHK(ensure_pinned(c, std::max<size_t>(head + 8, (size_t)ldc)));
  double* W = c->dPcL;
  ImArgs a;
  a.S = c->dW3; a.ld = mp; a.mc = (int)mc; a.mr = (int)mr; a.Gc = Gc; a.Gs = Gs;
  a.C = c->dImC; a.ldc = ldc;
  a.st = reinterpret_cast<ImState*>(c->dIm);
  a.pivvar = c->dIm + 3;
  a.gain = c->dIm + 3 + k;
  a.piv = reinterpret_cast<int*>(c->dIm + 3 + 2 * k);
  a.d = c->dIm + head;
  a.lam = a.d + mcp;
  double* dw = a.lam + ldc;
  a.w = dw;
  a.psc = dw + ldc;
  a.chosen = reinterpret_cast<int*>(a.psc + 2 * (size_t)Gs);
  a.pidx = a.chosen + mcp;
  a.tol = tol;
  // the weights (NULL: 1 / m_r each), zero in the padding
  for (long long i = 0; i < ldc; ++i) c->hpin[i] = i < mr ? (w ? w[i] : 1.0 / (double)mr) : 0.0;
  HIPCHK(c, hipMemcpyAsync(dw, c->hpin, (size_t)ldc * sizeof(double), hipMemcpyHostToDevice, c->stream));
  // the trailing update's descriptor: S -= W W^T over the candidates' tiles, K = PC_PANEL
  GemmLaunch Lt{};
  if (k > PC_PANEL) {
    CHK(adhoc_gemm(c, ADHOC_IMSE, {{GEMM_PLAIN, mkprob(W, mp, W, mp, c->dW3, mp, mct, mct, PC_PANEL, 0, -1.0, 1.0)}}, &Lt));
    Lt.flops = 2.0 * (double)mct * TILE * (double)mct * TILE * PC_PANEL;
  }
  hipLaunchKernelGGL(k_im_init, dim3(1), dim3(256), 0, c->stream, a, (int)k);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_im_copy, dim3((unsigned)((ldc + 255) / 256), (unsigned)(Gs * IM_NC)), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  CHK(panels_prof_begin(c));
  // step 0's scores: the sweep without a downdate
  hipLaunchKernelGGL(k_im_sweep<false>, dim3(Gs), dim3(256), 0, c->stream, a, (const double*)W, -1);
  HIPCHK(c, hipGetLastError());
  CHK(run_panels(
      c, k, Lt,
      [&](long long t0, int j) -> int {
        hipLaunchKernelGGL(k_im_col, dim3(Gc), dim3(256), 0, c->stream, a, W, (int)(t0 + j), j);
        HIPCHK(c, hipGetLastError());
        if (t0 + j + 1 < k) {   // (the last pick's downdate would feed a step that is not taken)
          hipLaunchKernelGGL(k_im_sweep<true>, dim3(Gs), dim3(256), 0, c->stream, a,
                             (const double*)(W + (size_t)j * mp), (int)(t0 + j));
          HIPCHK(c, hipGetLastError());
        }
        return GPE_OK;
      },
      [](long long, int) { return GPE_OK; }));
  HIPCHK(c, hipMemcpyAsync(c->hpin, c->dIm, head * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) c->phase_ms[6] = c->phase_ms[0] + c->phase_ms[1] + c->phase_ms[2];
  ImState st;
  std::memcpy(&st, c->hpin, sizeof(st));
  const long long rank = st.rank;
  if (rank < 0 || rank > k) return fail(c, GPE_ERR_HIP, "internal error: integrated-variance design rank out of range");
  const int* pv32 = reinterpret_cast<const int*>(c->hpin + 3 + 2 * k);
  for (long long t = 0; t < k; ++t) {
    piv_out[t] = t < rank ? pv32[t] : -1;
    pivvar_out[t] = t < rank ? c->hpin[3 + t] : 0.0;
    gain_out[t] = t < rank ? c->hpin[3 + k + t] : 0.0;
  }
  *imse0_out = st.imse0;
  *rank_out = rank;
  return GPE_OK;
}

}  // extern "C"

// hipMemcpy whose failure is kept in rc (the first failure wins, later copies are skipped)
static void copy_checked(gpe_ctx* c, int& rc, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (rc != GPE_OK) return;
  const hipError_t e = hipMemcpy(dst, src, bytes, kind);
  if (e != hipSuccess) rc = fail(c, GPE_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
}

extern "C" {

int gpe_kernel_var(gpe_ctx* c, int32_t kernel, const double* delta, int32_t d, double nu,
                   int32_t predict, int64_t m, const double* X, const double* r, double r_scale,
                   double* A_out) {
  if (!c) return GPE_ERR_ARG;
  if (!delta || !X || !A_out || m <= 0 || d <= 0) return fail(c, GPE_ERR_ARG, "bad kernel_var args");
  if (!kernel_ok(kernel)) return fail(c, GPE_ERR_ARG, "bad kernel");
  HIPCHK(c, hipSetDevice(c->device));
  CHK(ensure_shape_bufs(c, d, 1));
  const long long mp = ((m + TILE - 1) / TILE) * TILE;
  const int mt = (int)(mp / TILE);
  double *dx = nullptr, *dxw = nullptr, *dout = nullptr, *dr = nullptr;
  CHK(dalloc(c, &dx, (size_t)mp * d));
  CHK(dalloc(c, &dxw, (size_t)mp * d));
  int rc = dalloc(c, &dout, (size_t)mp * mp);
  if (rc == GPE_OK && r) rc = dalloc(c, &dr, (size_t)mp);
  if (rc == GPE_OK) {
    rc = ensure_pinned(c, (size_t)mp * d + 64 + (size_t)mp);
  }
  if (rc == GPE_OK) {
    std::memset(c->hpin, 0, (size_t)mp * d * sizeof(double));
    std::memcpy(c->hpin, X, (size_t)m * d * sizeof(double));
    for (int k = 0; k < d; ++k) c->hpin[(size_t)mp * d + k] = 1.0 / delta[k];
    copy_checked(c, rc, dx, c->hpin, (size_t)mp * d * sizeof(double), hipMemcpyHostToDevice);
    copy_checked(c, rc, c->dinvdelta, c->hpin + (size_t)mp * d, d * sizeof(double), hipMemcpyHostToDevice);
    if (r) {
      std::memset(c->hpin, 0, (size_t)mp * sizeof(double));
      std::memcpy(c->hpin, r, (size_t)m * sizeof(double));
      copy_checked(c, rc, dr, c->hpin, (size_t)mp * sizeof(double), hipMemcpyHostToDevice);
    }
    const long long tot = mp * d;
    hipLaunchKernelGGL(k_scale_points, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream,
                       dx, c->dinvdelta, d, (int)m, (int)mp, dxw);
    PairArgs a;
    a.xr = dxw; a.xc = dxw; a.out = dout; a.ld = mp; a.d = d; a.nr_valid = (int)m; a.nc_valid = (int)m;
    a.mt = mt; a.nt = mt; a.mode = 1 | 2 | 4;
    double coff, cdiag;
    kernel_consts(kernel, nu, predict != 0, &coff, &cdiag);
    a.s2 = 1.0; a.coff = coff; a.cdiag = cdiag; a.rscale = r_scale; a.r = dr;
    a.fam = kernel_fam(kernel);
    rc = launch_pairs(c, a, mt * (mt + 1) / 2);
    if (rc == GPE_OK) {
      hipError_t e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) rc = fail(c, GPE_ERR_HIP, hipGetErrorString(e));
    }
    if (rc == GPE_OK) {
      for (long long j = 0; j < m; ++j)
        copy_checked(c, rc, A_out + j * m, dout + j * mp, (size_t)m * sizeof(double), hipMemcpyDeviceToHost);
    }
  }
  (void)hipFree(dx);
  (void)hipFree(dxw);
  if (dout) hipFree(dout);
  if (dr) hipFree(dr);
  return rc;
}

// gpe_kernel_grad / gpe_kernel_grad_k for the correlation family fam (FAM_*): with a column
// the family's derivative factor g is written, without one its correlation rho
static int kernel_grad_fam(gpe_ctx* c, int fam, const double* delta, int32_t d, int64_t m, const double* X,
                           const double* col, double col_scale, double pre, double* G_out) {
  if (!delta || !X || !G_out || m <= 0 || d <= 0) return fail(c, GPE_ERR_ARG, "bad kernel_grad args");
  HIPCHK(c, hipSetDevice(c->device));
  CHK(ensure_shape_bufs(c, d, 1));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const long long mp = ((m + TILE - 1) / TILE) * TILE;
  const int mt = (int)(mp / TILE);
  double *dx = nullptr, *dxw = nullptr, *dout = nullptr, *dcol = nullptr;
  CHK(dalloc(c, &dx, (size_t)mp * d));
  CHK(dalloc(c, &dxw, (size_t)mp * d));
  int rc = dalloc(c, &dout, (size_t)mp * mp);
  if (rc == GPE_OK && col) rc = dalloc(c, &dcol, (size_t)mp);
  if (rc == GPE_OK) rc = ensure_pinned(c, (size_t)mp * d + 64 + (size_t)mp);
  if (rc == GPE_OK) {
    std::memset(c->hpin, 0, (size_t)mp * d * sizeof(double));
    std::memcpy(c->hpin, X, (size_t)m * d * sizeof(double));
    for (int k = 0; k < d; ++k) c->hpin[(size_t)mp * d + k] = 1.0 / delta[k];
    copy_checked(c, rc, dx, c->hpin, (size_t)mp * d * sizeof(double), hipMemcpyHostToDevice);
    copy_checked(c, rc, c->dinvdelta, c->hpin + (size_t)mp * d, d * sizeof(double), hipMemcpyHostToDevice);
    if (col) {
      std::memset(c->hpin, 0, (size_t)mp * sizeof(double));
      std::memcpy(c->hpin, col, (size_t)m * sizeof(double));
      copy_checked(c, rc, dcol, c->hpin, (size_t)mp * sizeof(double), hipMemcpyHostToDevice);
    }
    const long long tot = mp * d;
    hipLaunchKernelGGL(k_scale_points, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream,
                       dx, c->dinvdelta, d, (int)m, (int)mp, dxw);
    PairArgs a;
    a.xr = dxw; a.xc = dxw; a.out = dout; a.ld = mp; a.d = d; a.nr_valid = (int)m; a.nc_valid = (int)m;
    a.mt = mt; a.nt = mt; a.mode = 1 | 4 | 8;
    a.s2 = 1.0; a.coff = pre; a.cdiag = 0.0; a.rscale = 0.0; a.r = nullptr;
    a.fcol = dcol; a.fscale = col_scale;
    a.fam = fam; a.wg = col ? 1 : 0;
    rc = launch_pairs(c, a, mt * (mt + 1) / 2);
    if (rc == GPE_OK) {
      hipError_t e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) rc = fail(c, GPE_ERR_HIP, hipGetErrorString(e));
    }
    if (rc == GPE_OK) {
      for (long long j = 0; j < m; ++j)
        copy_checked(c, rc, G_out + j * m, dout + j * mp, (size_t)m * sizeof(double), hipMemcpyDeviceToHost);
    }
  }
  (void)hipFree(dx);
  (void)hipFree(dxw);
  if (dout) hipFree(dout);
  if (dcol) hipFree(dcol);
  return rc;
}

int gpe_kernel_grad(gpe_ctx* c, const double* delta, int32_t d, int64_t m, const double* X,
                    const double* col, double col_scale, double pre, double* G_out) {
  if (!c) return GPE_ERR_ARG;
  return kernel_grad_fam(c, FAM_GAUSS, delta, d, m, X, col, col_scale, pre, G_out);
}

int gpe_kernel_grad_k(gpe_ctx* c, int32_t kernel, const double* delta, int32_t d, int64_t m, const double* X,
                      const double* col, double col_scale, double pre, double* G_out) {
  if (!c) return GPE_ERR_ARG;
  if (!kernel_ok(kernel)) return fail(c, GPE_ERR_ARG, "bad kernel");
  return kernel_grad_fam(c, kernel_fam(kernel), delta, d, m, X, col, col_scale, pre, G_out);
}

int gpe_lhc_maximin(gpe_ctx* c, int32_t N, int64_t n, int32_t dim, const double* designs, int64_t ne,
                    const double* fextra, int64_t* idx_out) {
  if (!c) return GPE_ERR_ARG;
  if (!designs || !idx_out || N <= 0 || n <= 0 || dim <= 0 || ne < 0 || (ne > 0 && !fextra) ||
      n + ne < 2 || n + ne > 0x7fffffffLL)
    return fail(c, GPE_ERR_ARG, "bad lhc_maximin args");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int m = (int)(n + ne);
  // designs per launch: grid.y <= 65535 and <= 1 GiB of design points on the device
  const long long per = std::max(1LL, (1LL << 27) / (n * (long long)dim));
  const int K = (int)std::min<long long>({(long long)N, 65535LL, per});
  const int tiles = (int)((n + LHC_R - 1) / LHC_R);
  const int ftiles = ne > 1 ? (int)((ne - 1 + LHC_R - 1) / LHC_R) : 0;
  const bool use_lds = dim <= LHC_LDS_DIM;
  const size_t lds = use_lds ? (size_t)LHC_R * dim * sizeof(double) : 0;
  auto rowmin = use_lds ? k_lhc_rowmin<true> : k_lhc_rowmin<false>;
  const size_t nbuf = std::max((size_t)K * tiles, (size_t)ftiles);
  double *dD = nullptr, *dE = nullptr, *bd = nullptr;
  long long *bi = nullptr, *oi = nullptr;
  int rc = dalloc(c, &dD, (size_t)K * n * dim);
  if (rc == GPE_OK && ne > 0) rc = dalloc(c, &dE, (size_t)ne * dim);
  if (rc == GPE_OK) rc = dalloc(c, &bd, nbuf + 1);  // slot nbuf: the fextra-fextra minimum
  if (rc == GPE_OK) rc = dalloc(c, &bi, nbuf + 1);
  if (rc == GPE_OK) rc = dalloc(c, &oi, (size_t)K);
  if (ne > 0) copy_checked(c, rc, dE, fextra, (size_t)ne * dim * sizeof(double), hipMemcpyHostToDevice);
  const bool ff = ftiles > 0;
  if (rc == GPE_OK && ff) {
    // pairs among the fextra points (rows n .. m-2) are the same for every design
    hipLaunchKernelGGL(rowmin, dim3(ftiles, 1), dim3(256), lds, c->stream, dD, 0LL, (int)n, dE,
                       (int)ne, dim, (int)n, m - 1, bd, bi);
    hipLaunchKernelGGL(k_lhc_reduce, dim3(1), dim3(256), 0, c->stream, bd, bi, ftiles,
                       (const double*)nullptr, (const long long*)nullptr, bd + nbuf, bi + nbuf);
  }
  for (int k0 = 0; rc == GPE_OK && k0 < N; k0 += K) {
    const int kb = std::min(K, N - k0);
    copy_checked(c, rc, dD, designs + (size_t)k0 * n * dim, (size_t)kb * n * dim * sizeof(double),
                 hipMemcpyHostToDevice);
    if (rc != GPE_OK) break;
    // rows 0 .. n-1 of each design (a design's last row has pairs only with fextra)
    const int row_end = (int)std::min<long long>(n, m - 1);
    const int tl = (row_end + LHC_R - 1) / LHC_R;
    hipLaunchKernelGGL(rowmin, dim3(tl, kb), dim3(256), lds, c->stream, dD, n * (long long)dim, (int)n,
                       dE, (int)ne, dim, 0, row_end, bd, bi);
    hipLaunchKernelGGL(k_lhc_reduce, dim3(kb), dim3(256), 0, c->stream, bd, bi, tl,
                       ff ? (const double*)(bd + nbuf) : nullptr, ff ? (const long long*)(bi + nbuf) : nullptr,
                       (double*)nullptr, oi);
    // the copies are synchronous on the null stream, which does not order with c->stream
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(c, GPE_ERR_HIP, std::string("lhc_maximin: ") + hipGetErrorString(e));
    copy_checked(c, rc, idx_out + k0, oi, (size_t)kb * sizeof(long long), hipMemcpyDeviceToHost);
  }
  if (rc != GPE_OK) (void)hipStreamSynchronize(c->stream);
  if (dD) hipFree(dD);
  if (dE) hipFree(dE);
  if (bd) hipFree(bd);
  if (bi) hipFree(bi);
  if (oi) hipFree(oi);
  return rc;
}

int gpe_kernel_covar(gpe_ctx* c, int32_t kernel, const double* delta, int32_t d, double nu,
                     int64_t n, const double* XT, int64_t m, const double* XV, double* C_out) {
  if (!c) return GPE_ERR_ARG;
  if (!delta || !XT || !XV || !C_out || n <= 0 || m <= 0 || d <= 0)
    return fail(c, GPE_ERR_ARG, "bad kernel_covar args");
  if (!kernel_ok(kernel)) return fail(c, GPE_ERR_ARG, "bad kernel");
  HIPCHK(c, hipSetDevice(c->device));
  CHK(ensure_shape_bufs(c, d, 1));
  // compute C^T (m x n, column-major == n x m row-major)
  const long long mp = ((m + TILE - 1) / TILE) * TILE, np = ((n + TILE - 1) / TILE) * TILE;
  double *dxt = nullptr, *dxv = nullptr, *dxtw = nullptr, *dxvw = nullptr, *dout = nullptr;
  int rc = GPE_OK;
  rc = dalloc(c, &dxt, (size_t)np * d);
  if (rc == GPE_OK) rc = dalloc(c, &dxtw, (size_t)np * d);
  if (rc == GPE_OK) rc = dalloc(c, &dxv, (size_t)mp * d);
  if (rc == GPE_OK) rc = dalloc(c, &dxvw, (size_t)mp * d);
  if (rc == GPE_OK) rc = dalloc(c, &dout, (size_t)mp * np);
  if (rc == GPE_OK) rc = ensure_pinned(c, (size_t)std::max(np, mp) * d + 64);
  if (rc == GPE_OK) {
    for (int k = 0; k < d; ++k) c->hpin[k] = 1.0 / delta[k];
    copy_checked(c, rc, c->dinvdelta, c->hpin, d * sizeof(double), hipMemcpyHostToDevice);
    std::memset(c->hpin, 0, (size_t)np * d * sizeof(double));
    std::memcpy(c->hpin, XT, (size_t)n * d * sizeof(double));
    copy_checked(c, rc, dxt, c->hpin, (size_t)np * d * sizeof(double), hipMemcpyHostToDevice);
    std::memset(c->hpin, 0, (size_t)mp * d * sizeof(double));
    std::memcpy(c->hpin, XV, (size_t)m * d * sizeof(double));
    copy_checked(c, rc, dxv, c->hpin, (size_t)mp * d * sizeof(double), hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_scale_points, dim3((unsigned)((np * d + 255) / 256)), dim3(256), 0, c->stream,
                       dxt, c->dinvdelta, d, (int)n, (int)np, dxtw);
    hipLaunchKernelGGL(k_scale_points, dim3((unsigned)((mp * d + 255) / 256)), dim3(256), 0, c->stream,
                       dxv, c->dinvdelta, d, (int)m, (int)mp, dxvw);
    PairArgs a;
    a.xr = dxvw; a.xc = dxtw; a.out = dout; a.ld = mp; a.d = d; a.nr_valid = (int)m; a.nc_valid = (int)n;
    a.mt = (int)(mp / TILE); a.nt = (int)(np / TILE); a.mode = 0;
    double coff, cdiag;
    kernel_consts(kernel, nu, true, &coff, &cdiag);
    a.s2 = 1.0; a.coff = coff; a.cdiag = cdiag; a.rscale = 0.0; a.r = nullptr;
    a.fam = kernel_fam(kernel);
    rc = launch_pairs(c, a, a.mt * a.nt);
    if (rc == GPE_OK) {
      hipError_t e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) rc = fail(c, GPE_ERR_HIP, hipGetErrorString(e));
    }
    if (rc == GPE_OK) {
      // dout column j (= training point j) holds C[j, 0:m]
      for (long long j = 0; j < n; ++j)
        copy_checked(c, rc, C_out + j * m, dout + j * mp, (size_t)m * sizeof(double), hipMemcpyDeviceToHost);
    }
  }
  (void)hipFree(dxt); hipFree(dxtw); hipFree(dxv); hipFree(dxvw);
  if (dout) hipFree(dout);
  return rc;
}

int gpe_cholesky(gpe_ctx* c, int64_t m, const double* A, double* L_out, double* Linv_out,
                 double* Ainv_out, double* logdet_out) {
  if (!c) return GPE_ERR_ARG;
  if (!A || m <= 0) return fail(c, GPE_ERR_ARG, "bad cholesky args");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const long long mp = ((m + TILE - 1) / TILE) * TILE;
  Fact& F = c->aux;
  CHK(ensure_fact(c, F, mp));
  CHK(build_plan(c, F));
  // stage the lower triangle column-major, identity padding
  const size_t tot = (size_t)mp * mp;
  CHK(ensure_pinned(c, tot));
  std::memset(c->hpin, 0, tot * sizeof(double));
  for (long long j = 0; j < m; ++j)
    for (long long i = j; i < m; ++i) c->hpin[i + j * mp] = A[i * m + j];
  for (long long i = m; i < mp; ++i) c->hpin[i + i * mp] = 1.0;
  HIPCHK(c, hipMemcpy(F.A, c->hpin, tot * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemsetAsync(c->dinfo, 0, sizeof(int), c->stream));
  CHK(potrf(c, F));
  int info = 0;
  double logdet = 0.0;
  CHK(read_info_logdet(c, F, &info, &logdet));
  if (info != 0) return fail(c, GPE_NOT_PD, not_pd_pivot(info));
  if (logdet_out) *logdet_out = logdet;
  auto fetch_lower = [&](const double* dsrc, double* out, bool full_sym) -> int {
    HIPCHK(c, hipMemcpy(c->hpin, dsrc, tot * sizeof(double), hipMemcpyDeviceToHost));
    for (long long i = 0; i < m; ++i)
      for (long long j = 0; j < m; ++j) {
        double v;
        if (j <= i) v = c->hpin[i + j * mp];
        else v = full_sym ? c->hpin[j + i * mp] : 0.0;
        out[i * m + j] = v;
      }
    return GPE_OK;
  };
  if (L_out) CHK(fetch_lower(F.A, L_out, false));
  if (Linv_out || Ainv_out) {
    CHK(trtri(c, F));
    if (Linv_out) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      CHK(fetch_lower(F.B, Linv_out, false));
    }
    if (Ainv_out) {
      CHK(lauum(c, F));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      CHK(fetch_lower(F.A, Ainv_out, true));
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GPE_OK;
}

int gpe_test_gemm(gpe_ctx* c, int32_t trans_a, int32_t trans_b, int64_t M, int64_t N, int64_t K,
                  const double* A, const double* B, double* C, double alpha, double beta) {
  if (!c) return GPE_ERR_ARG;
  if (M <= 0 || N <= 0 || K <= 0 || M % TILE || N % TILE || K % GK || !A || !B || !C)
    return fail(c, GPE_ERR_ARG, "gpe_test_gemm: M, N must be multiples of 128 and K of 16");
  HIPCHK(c, hipSetDevice(c->device));
  double *da = nullptr, *db = nullptr, *dc = nullptr;
  int rc = dalloc(c, &da, (size_t)M * K);
  if (rc == GPE_OK) rc = dalloc(c, &db, (size_t)K * N);
  if (rc == GPE_OK) rc = dalloc(c, &dc, (size_t)M * N);
  if (rc == GPE_OK) {
    std::vector<double> ha((size_t)M * K), hb((size_t)K * N), hc((size_t)M * N);
    long long lda, ldb;
    if (trans_a) { for (long long m = 0; m < M; ++m) for (long long k = 0; k < K; ++k) ha[k + m * K] = A[m * K + k]; lda = K; }
    else { for (long long m = 0; m < M; ++m) for (long long k = 0; k < K; ++k) ha[m + k * M] = A[m * K + k]; lda = M; }
    if (trans_b) { for (long long k = 0; k < K; ++k) for (long long n = 0; n < N; ++n) hb[k + n * K] = B[k * N + n]; ldb = K; }
    else { for (long long k = 0; k < K; ++k) for (long long n = 0; n < N; ++n) hb[n + k * N] = B[k * N + n]; ldb = N; }
    for (long long m = 0; m < M; ++m) for (long long n = 0; n < N; ++n) hc[m + n * M] = C[m * N + n];
    copy_checked(c, rc, da, ha.data(), ha.size() * sizeof(double), hipMemcpyHostToDevice);
    copy_checked(c, rc, db, hb.data(), hb.size() * sizeof(double), hipMemcpyHostToDevice);
    copy_checked(c, rc, dc, hc.data(), hc.size() * sizeof(double), hipMemcpyHostToDevice);
    const GemmProb p = mkprob(da, lda, db, ldb, dc, M, (int)(M / TILE), (int)(N / TILE), (int)K, 0, alpha, beta);
    const GemmKind kind = gemm_kind(trans_a != 0, trans_b != 0);
    GemmLaunch L{};
    if (rc == GPE_OK) rc = adhoc_gemm(c, ADHOC_TEST, {{kind, p}}, &L, true);
    HIPCHK(c, hipMemsetAsync(c->dinfo, 0, sizeof(int), c->stream));
    if (rc == GPE_OK) rc = launch_gemm_range(c, L);
    if (rc == GPE_OK) {
      hipError_t e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) rc = fail(c, GPE_ERR_HIP, hipGetErrorString(e));
    }
    if (rc == GPE_OK) {
      copy_checked(c, rc, hc.data(), dc, hc.size() * sizeof(double), hipMemcpyDeviceToHost);
      for (long long m = 0; m < M; ++m) for (long long n = 0; n < N; ++n) C[m * N + n] = hc[m + n * M];
    }
  }
  if (da) (void)hipFree(da);
  if (db) (void)hipFree(db);
  if (dc) (void)hipFree(dc);
  return rc;
}

// ---- gpe_test_oz_product: one int8 product on buffers of its own
struct OzTestBufs {   // (freed on every way out)
  double *sa = nullptr, *sb = nullptr, *C = nullptr;
  int *exa = nullptr, *exb = nullptr;
  int8_t *pa = nullptr, *pb = nullptr, *res = nullptr;
  unsigned* list = nullptr;
  unsigned long long *suma = nullptr, *sumb = nullptr;   // (gpe_test_oz_product_cert: the row sums and the flag)
  int* flag = nullptr;
  ~OzTestBufs() {
    for (void* p : {(void*)sa, (void*)sb, (void*)C, (void*)exa, (void*)exb, (void*)pa, (void*)pb, (void*)res, (void*)list,
                    (void*)suma, (void*)sumb, (void*)flag})
      if (p) (void)hipFree(p);
  }
};

// the doubles of src that op(r, k), r < R, k < Kv, spans from offset on (0: the window is bad)
static long long oz_test_extent(const gpe_oz_operand& o, int R, int Kv) {
  if (!o.src || o.len <= 0 || o.offset < 0 || o.ld < 1 || R < 1 || Kv < 1) return 0;
  const long long ext = o.trans ? (long long)(Kv - 1) * o.ld + R : (long long)(R - 1) * o.ld + Kv;
  return ext <= o.len - o.offset ? ext : 0;
}

// a rectangular operand: source to the device, row exponents, planes (P rows of Kp bytes per
// modulus) by oz_operand, the call every production site converts its operands with
// (dsum: null, or where the certificate's row sums go, P of them)
static int oz_test_operand(gpe_ctx* c, const gpe_oz_operand& o, const OzConst& k, int P, int Kp, double** dsrc, int** dex,
                           int8_t** dpl, unsigned long long** dsum = nullptr) {
  if (dsum) CHK(dalloc(c, dsum, (size_t)P));
  CHK(dalloc(c, dsrc, (size_t)o.len));
  CHK(dalloc(c, dex, (size_t)P));
  CHK(dalloc(c, dpl, (size_t)k.nmod * P * Kp));
  HIPCHK(c, hipMemcpy(*dsrc, o.src, (size_t)o.len * sizeof(double), hipMemcpyHostToDevice));
  oz_operand(c->stream, k, OzSrc{*dsrc + o.offset, (long long)o.ld, o.R, o.Kv, o.mask, o.trans != 0}, P, Kp, *dex, *dpl,
             dsum ? *dsum : nullptr);
  HIPCHK(c, hipGetLastError());
  return GPE_OK;
}

// (nmod_used_out: null, or the product runs with a certificate and the moduli it used go there)
static int oz_test_product(gpe_ctx* c, const gpe_oz_operand& a, const gpe_oz_operand* b, gpe_oz_params p, double* C,
                           int32_t* exa_out, int32_t* exb_out, int8_t* res_out, int32_t* nmod_used_out = nullptr) {
  const auto bad = [&](const char* what) { return fail(c, GPE_ERR_ARG, std::string("gpe_test_oz_product: ") + what); };
  if (p.nmod < 6 || p.nmod > OZ_MAXMOD) return bad("nmod outside [6, 16]");
  const bool cert = nmod_used_out != nullptr;
  if (cert && p.nmod != OZ_MAXMOD) return bad("a certificate needs nmod = 16");
  if (res_out && (p.res_mod < 0 || p.res_mod >= p.nmod)) return bad("res_mod is not a modulus number");
  if (a.R < 1 || a.R > (1 << 20)) return bad("bad operand rows");
  const int Pa = (a.R + OZ_T - 1) / OZ_T * OZ_T;
  int Pb = Pa;
  if (p.packed) {
    // k_oz_split's 16-byte loads: every column of X starts 16-byte aligned
    if (a.R % TILE || (a.offset & 1) || (a.ld & 1) || a.ld < a.R || !oz_test_extent(a, 1, 1) ||
        (long long)(a.R - 1) * a.ld + a.R > a.len - a.offset)
      return bad("packed: X is R x R, R a multiple of 128, ld >= R and offset even, inside src");
    p.K = Pa; p.kbeg = 1; p.kend = 0; p.kdiv = 1; p.ti0 = 0; p.tri = 1; p.lower128 = 1;
    p.rows = p.cols = a.R;
    b = nullptr;
  } else {
    if (p.K < OZ_SK || p.K % OZ_SK || p.K > OZ_MAX_K) return bad("K is not a multiple of 64 in [64, 2^17 - 128]");
    if (a.mask < 0 || a.mask > 2 || a.Kv > p.K || !oz_test_extent(a, a.R, a.Kv)) return bad("operand A outside its source");
    if (b) {
      if (b->R < 1 || b->R > (1 << 20) || b->mask < 0 || b->mask > 2 || b->Kv > p.K || !oz_test_extent(*b, b->R, b->Kv))
        return bad("operand B outside its source");
      Pb = (b->R + OZ_T - 1) / OZ_T * OZ_T;
    }
    if (p.kbeg < 0 || p.kbeg > 3 || p.kend < 0 || p.kend > 1 || p.kdiv < 1) return bad("bad kbeg / kend / kdiv");
    if (p.ti0 < 0 || p.ti0 >= Pa / OZ_T) return bad("ti0 past the last tile row");
    // tri with fewer tile rows in B than in A: the triangle capped at B's (OzShape::lower_capped)
    if (p.tri && Pb < Pa && p.ti0 != 0) return bad("tri: B has fewer tile rows than A and ti0 > 0");
  }
  if (p.rows <= OZ_T * p.ti0 || p.rows > Pa || p.cols < 1 || p.cols > Pb) return bad("rows / cols outside the product");
  if (!C || p.ldc < 1 || p.c_len < 1 || (long long)(p.rows - 1 - OZ_T * p.ti0) + (long long)(p.cols - 1) * p.ldc >= p.c_len)
    return bad("C too small for rows x cols at ldc");
  const int K = p.K, ti0 = p.ti0, nti = Pa / OZ_T - ti0, ntj = Pb / OZ_T;
  const OzConst k = oz_consts(p.nmod, K);
  const OzConst k15 = oz_consts_cert(K);
  const OzShape s{nti, p.tri ? (Pb < Pa ? ntj : 0) : ntj, ti0, p.tri ? 1 : 0, K, p.kbeg, p.kend, p.kdiv};
  OzTestBufs d;
  hipStream_t st = c->stream;
  OzOpnd oa, ob;
  if (p.packed) {
    CHK(dalloc(c, &d.sa, (size_t)a.len));
    CHK(dalloc(c, &d.exa, (size_t)Pa));
    CHK(dalloc(c, &d.pa, (size_t)k.nmod * oz_plane_bytes(Pa)));
    if (cert) CHK(dalloc(c, &d.suma, (size_t)Pa));
    HIPCHK(c, hipMemcpy(d.sa, a.src, (size_t)a.len * sizeof(double), hipMemcpyHostToDevice));
    oz_operand_packed(st, k, d.sa + a.offset, (long long)a.ld, a.R, Pa, d.exa, d.pa, d.suma);
    HIPCHK(c, hipGetLastError());
    oa = ob = OzOpnd{d.pa, oz_plane_bytes(Pa), 0, Pa};
  } else {
    CHK(oz_test_operand(c, a, k, Pa, K, &d.sa, &d.exa, &d.pa, cert ? &d.suma : nullptr));
    oa = ob = OzOpnd{d.pa, (long long)Pa * K, K, 0};
    if (b) {
      CHK(oz_test_operand(c, *b, k, Pb, K, &d.sb, &d.exb, &d.pb, cert ? &d.sumb : nullptr));
      ob = OzOpnd{d.pb, (long long)Pb * K, K, 0};
    }
  }
  const std::vector<unsigned> list = s.list();
  const long long rb = s.res_bytes();
  CHK(dalloc(c, &d.list, list.size()));
  CHK(dalloc(c, &d.res, (size_t)k.nmod * rb));
  CHK(dalloc(c, &d.C, (size_t)p.c_len));
  HIPCHK(c, hipMemcpy(d.list, list.data(), list.size() * sizeof(unsigned), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(d.C, C, (size_t)p.c_len * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemsetAsync(d.res, 0, (size_t)k.nmod * rb, st));
  const OzOut out{d.exa, b ? d.exb : d.exa, d.C, (long long)p.ldc, p.rows, p.cols, p.lower128 ? 1 : 0, p.alpha, p.acc ? 1 : 0};
  OzCert ct{};
  if (cert) {
    CHK(dalloc(c, &d.flag, (size_t)1));
    HIPCHK(c, hipMemsetAsync(d.flag, 0, sizeof(int), st));
    ct = OzCert{d.suma, Pa, b ? d.sumb : d.suma, Pb, d.flag, &k15};
  }
  CHK(oz_gemm_crt(c, k, OzProduct{s, oa, ob, d.list, (int)list.size(), d.res, rb, out, ct}, 0.0, 0.0));
  HIPCHK(c, hipStreamSynchronize(st));
  if (cert) {
    int fl = 0;
    HIPCHK(c, hipMemcpy(&fl, d.flag, sizeof(int), hipMemcpyDeviceToHost));
    *nmod_used_out = fl ? OZ_CERT_NMOD : OZ_MAXMOD;
  }
  HIPCHK(c, hipMemcpy(C, d.C, (size_t)p.c_len * sizeof(double), hipMemcpyDeviceToHost));
  if (exa_out) HIPCHK(c, hipMemcpy(exa_out, d.exa, (size_t)Pa * sizeof(int), hipMemcpyDeviceToHost));
  if (exb_out) HIPCHK(c, hipMemcpy(exb_out, b ? d.exb : d.exa, (size_t)Pb * sizeof(int), hipMemcpyDeviceToHost));
  if (res_out) {
    // k_oz_gemm's order (see there and k_oz_crt) -> (row, column)
    std::vector<int8_t> h((size_t)rb);
    HIPCHK(c, hipMemcpy(h.data(), d.res + (long long)p.res_mod * rb, (size_t)rb, hipMemcpyDeviceToHost));
    std::memset(res_out, 0, (size_t)nti * OZ_T * Pb);
    for (const unsigned ent : list) {
      if (ent == 0xffffffffu) continue;
      const int ti = (int)(ent >> 16), tj = (int)(ent & 0xffffu);
      const int8_t* t = h.data() + s.res_tile(ti, tj) * (OZ_T * OZ_T);
      for (int u = 0; u < OZ_T * OZ_T / 16; ++u) {
        const int wave = u >> 10, blk = (u >> 6) & 15, lane = u & 63;
        const long long gm = OZ_T * (ti - ti0) + (wave >> 1) * 128 + 32 * (blk >> 2) + (lane & 31);
        const long long gn0 = OZ_T * tj + (wave & 1) * 128 + 32 * (blk & 3) + 4 * (lane >> 5);
        for (int q = 0; q < 16; ++q) res_out[gm * Pb + gn0 + (q & 3) + 8 * (q >> 2)] = t[(long long)u * 16 + q];
      }
    }
  }
  return GPE_OK;
}

int gpe_test_oz_product(gpe_ctx* c, const gpe_oz_operand* a, const gpe_oz_operand* b, const gpe_oz_params* p, double* C,
                        int32_t* exa_out, int32_t* exb_out, int8_t* res_out) {
  if (!c) return GPE_ERR_ARG;
  if (!a || !p) return fail(c, GPE_ERR_ARG, "gpe_test_oz_product: NULL operand or parameters");
  HIPCHK(c, hipSetDevice(c->device));
  const bool prof = c->prof;   // (not a product of the objective: kept out of gpe_ozaki_stats)
  c->prof = false;
  const int rc = oz_test_product(c, *a, b, *p, C, exa_out, exb_out, res_out);
  c->prof = prof;
  return rc;
}

int gpe_test_oz_product_cert(gpe_ctx* c, const gpe_oz_operand* a, const gpe_oz_operand* b, const gpe_oz_params* p, double* C,
                             int32_t* exa_out, int32_t* exb_out, int8_t* res_out, int32_t* nmod_used_out) {
  if (!c) return GPE_ERR_ARG;
  if (!a || !p || !nmod_used_out) return fail(c, GPE_ERR_ARG, "gpe_test_oz_product_cert: NULL operand, parameters or nmod_used_out");
  HIPCHK(c, hipSetDevice(c->device));
  const bool prof = c->prof;
  c->prof = false;
  const int rc = oz_test_product(c, *a, b, *p, C, exa_out, exb_out, res_out, nmod_used_out);
  c->prof = prof;
  return rc;
}

// ---- gpe_test_oz_planes: one operand's exponents and int8 planes, on buffers of its own
static int oz_test_planes(gpe_ctx* c, const gpe_oz_operand& a, int packed, int K, int nmod, int32_t* ex_out, int8_t* planes_out) {
  const auto bad = [&](const char* what) { return fail(c, GPE_ERR_ARG, std::string("gpe_test_oz_planes: ") + what); };
  if (nmod < 6 || nmod > OZ_MAXMOD) return bad("nmod outside [6, 16]");
  if (a.R < 1 || a.R > (1 << 20)) return bad("bad operand rows");
  if (!ex_out || !planes_out) return bad("NULL output");
  const int P = (a.R + OZ_T - 1) / OZ_T * OZ_T;
  if (packed) {
    if (a.R % TILE || (a.offset & 1) || (a.ld & 1) || a.ld < a.R || !oz_test_extent(a, 1, 1) ||
        (long long)(a.R - 1) * a.ld + a.R > a.len - a.offset)
      return bad("packed: X is R x R, R a multiple of 128, ld >= R and offset even, inside src");
    K = P;
  } else {
    if (K < OZ_SK || K % OZ_SK || K > OZ_MAX_K) return bad("K is not a multiple of 64 in [64, 2^17 - 128]");
    if (a.mask < 0 || a.mask > 2 || a.Kv > K || !oz_test_extent(a, a.R, a.Kv)) return bad("operand outside its source");
  }
  const OzConst k = oz_consts(nmod, K);
  OzTestBufs d;
  if (packed) {
    const long long pb = oz_plane_bytes(P);
    CHK(dalloc(c, &d.sa, (size_t)a.len));
    CHK(dalloc(c, &d.exa, (size_t)P));
    CHK(dalloc(c, &d.pa, (size_t)nmod * pb));
    HIPCHK(c, hipMemcpy(d.sa, a.src, (size_t)a.len * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(d.pa, 0x55, (size_t)nmod * pb, c->stream));   // (every byte is to be written)
    oz_operand_packed(c->stream, k, d.sa + a.offset, (long long)a.ld, a.R, P, d.exa, d.pa);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int8_t> h((size_t)nmod * pb);
    HIPCHK(c, hipMemcpy(h.data(), d.pa, h.size(), hipMemcpyDeviceToHost));
    std::memset(planes_out, 0, (size_t)nmod * P * P);
    for (int l = 0; l < nmod; ++l)
      for (int j = 0; j < P; ++j) {   // column j of X: rows 256 (j / 256) .. P of its panel
        const int r0 = j / OZ_T * OZ_T;
        std::memcpy(planes_out + ((size_t)l * P + j) * P + r0,
                    h.data() + (size_t)l * pb + oz_panel_off(j / OZ_T, P) + (long long)(j - r0) * (P - r0), (size_t)(P - r0));
      }
  } else {
    CHK(dalloc(c, &d.sa, (size_t)a.len));
    CHK(dalloc(c, &d.exa, (size_t)P));
    CHK(dalloc(c, &d.pa, (size_t)nmod * P * K));
    HIPCHK(c, hipMemcpy(d.sa, a.src, (size_t)a.len * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(d.pa, 0x55, (size_t)nmod * P * K, c->stream));
    oz_operand(c->stream, k, OzSrc{d.sa + a.offset, (long long)a.ld, a.R, a.Kv, a.mask, a.trans != 0}, P, K, d.exa, d.pa);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(planes_out, d.pa, (size_t)nmod * P * K, hipMemcpyDeviceToHost));
  }
  HIPCHK(c, hipMemcpy(ex_out, d.exa, (size_t)P * sizeof(int), hipMemcpyDeviceToHost));
  return GPE_OK;
}

int gpe_test_oz_planes(gpe_ctx* c, const gpe_oz_operand* a, int32_t packed, int32_t K, int32_t nmod, int32_t* ex_out,
                       int8_t* planes_out) {
  if (!c) return GPE_ERR_ARG;
  if (!a) return fail(c, GPE_ERR_ARG, "gpe_test_oz_planes: NULL operand");
  HIPCHK(c, hipSetDevice(c->device));
  return oz_test_planes(c, *a, packed, K, nmod, ex_out, planes_out);
}

// ---- gpe_test_gemm_group: one k_gemm launch on a group of problems, on buffers of its own
struct GemmGroupBufs {   // (freed, and the context's descriptor / list arrays put back, on every way out)
  gpe_ctx* c;
  GemmProb* ctx_probs;
  unsigned* ctx_tiles;
  bool prof;
  std::vector<double*> dev, keep;   // the buffers, and the inputs of those that hold a C
  GemmProb* probs = nullptr;
  unsigned* tiles = nullptr;
  double* part = nullptr;
  int* tcnt = nullptr;
  explicit GemmGroupBufs(gpe_ctx* ctx) : c(ctx), ctx_probs(ctx->dprobs), ctx_tiles(ctx->dtiles), prof(ctx->prof) {}
  ~GemmGroupBufs() {
    c->dprobs = ctx_probs;
    c->dtiles = ctx_tiles;
    c->prof = prof;
    for (double* p : dev) if (p) (void)hipFree(p);
    for (double* p : keep) if (p) (void)hipFree(p);
    for (void* p : {(void*)probs, (void*)tiles, (void*)part, (void*)tcnt}) if (p) (void)hipFree(p);
  }
};

static int gemm_group_test(gpe_ctx* c, int nbuf, double* const* bufs, const int64_t* lens, int nprob,
                           const gpe_gemm_group_prob* gp, const gpe_gemm_group_launch& gl, int32_t* ksplit_out,
                           int32_t* info_out, uint32_t* tiles_out, int64_t tiles_cap) {
  const auto bad = [&](const std::string& what) { return fail(c, GPE_ERR_ARG, "gpe_test_gemm_group: " + what); };
  if (nbuf < 1 || nbuf > 64 || nprob < 1 || nprob > 1024) return bad("1 to 64 buffers, 1 to 1024 problems");
  for (int i = 0; i < nbuf; ++i)
    if (!bufs[i] || lens[i] < 1) return bad("NULL or empty buffer " + std::to_string(i));
  if (gl.kind < GEMM_PLAIN || gl.kind > GEMM_BK || (gl.split & ~1) || (gl.listed & ~1) || gl.reps < 1 || gl.reps > 16)
    return bad("kind 0..3, split 0 / 1, listed 0 / 1, reps 1..16");
  if (gl.listed && nprob >= 256) return bad("a tile list names at most 255 problems");
  if (tiles_cap < 0 || (tiles_cap > 0 && !tiles_out)) return bad("tiles_out is NULL");
  const GemmKind kind = (GemmKind)gl.kind;
  const bool AK = gemm_instance(kind).ak, BK = gemm_instance(kind).bk;
  long long total = 0;
  std::vector<char> holds_c(nbuf, 0);
  for (int p = 0; p < nprob; ++p) {
    const gpe_gemm_group_prob& g = gp[p];
    const std::string who = "problem " + std::to_string(p) + ": ";
    if (g.flags & ~(G_CLOWER | G_KBEG_TI | G_KEND_TI)) return bad(who + "only G_CLOWER, G_KBEG_TI, G_KEND_TI (no fused flag)");
    if (g.K < GK || g.K % GK || g.K > (1 << 24)) return bad(who + "K is not a positive multiple of 16");
    if (!(g.alpha != 0.0) || !std::isfinite(g.alpha) || std::isnan(g.beta)) return bad(who + "alpha is 0 or not finite (beta / alpha)");
    if (g.mt < 1 || g.mt > 4096 || g.nt < 1 || g.nt > 4096) return bad(who + "mt, nt outside [1, 4096]");
    if (g.kti_mul < 0 || g.kti_off < 0 || g.kti_mul > 4096 || g.kti_off > 4096) return bad(who + "kti_mul, kti_off outside [0, 4096]");
    if (g.a_buf < 0 || g.a_buf >= nbuf || g.b_buf < 0 || g.b_buf >= nbuf || g.c_buf < 0 || g.c_buf >= nbuf)
      return bad(who + "buffer index");
    if (g.a_off < 0 || g.b_off < 0 || g.c_off < 0 || ((g.a_off | g.b_off | g.c_off) & 1)) return bad(who + "odd or negative offset");
    if (g.lda < 2 || g.ldb < 2 || g.ldc < 2 || ((g.lda | g.ldb | g.ldc) & 1)) return bad(who + "odd leading dimension");
    if (g.ldc > (1ll << 21)) return bad(who + "ldc > 2^21");
    if (std::max({g.lda, g.ldb}) > (1ll << 40)) return bad(who + "leading dimension");
    total += (g.flags & G_CLOWER) ? (long long)g.mt * (g.mt + 1) / 2 : (long long)g.mt * g.nt;
    if (total > 65536) return bad("more than 65536 tiles");
    holds_c[g.c_buf] = 1;
    // every tile's windows: the operand panels over its own K range, its C tile
    const long long la = lens[g.a_buf], lb = lens[g.b_buf], lc = lens[g.c_buf];
    for (int ti = 0; ti < g.mt; ++ti) {
      const long long kb = (g.flags & G_KBEG_TI) ? (long long)ti * TILE : 0;
      const long long ke = (g.flags & G_KEND_TI) ? std::min<long long>(g.K, ((long long)ti * g.kti_mul + g.kti_off + 1) * TILE) : g.K;
      const long long r1 = (long long)ti * TILE + TILE - 1;
      if (ke > kb && g.a_off + (AK ? r1 * g.lda + ke - 1 : (ke - 1) * g.lda + r1) >= la)
        return bad(who + "A leaves its buffer at tile row " + std::to_string(ti));
      const int tjn = (g.flags & G_CLOWER) ? ti + 1 : g.nt;   // (G_CLOWER: tj <= ti, whatever nt)
      const long long c1 = (long long)(tjn - 1) * TILE + TILE - 1;
      if (ke > kb && g.b_off + (BK ? c1 * g.ldb + ke - 1 : (ke - 1) * g.ldb + c1) >= lb)
        return bad(who + "B leaves its buffer at tile row " + std::to_string(ti));
      if (g.c_off + r1 + c1 * g.ldc >= lc) return bad(who + "C leaves its buffer at tile row " + std::to_string(ti));
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  GemmGroupBufs d(c);
  c->prof = false;   // (not a launch of the objective: kept out of gpe_gemm_stats)
  d.dev.assign(nbuf, nullptr);
  d.keep.assign(nbuf, nullptr);
  for (int i = 0; i < nbuf; ++i) {
    CHK(dalloc(c, &d.dev[i], (size_t)lens[i]));
    HIPCHK(c, hipMemcpy(d.dev[i], bufs[i], (size_t)lens[i] * sizeof(double), hipMemcpyHostToDevice));
    if (holds_c[i] && gl.reps > 1) {
      CHK(dalloc(c, &d.keep[i], (size_t)lens[i]));
      HIPCHK(c, hipMemcpy(d.keep[i], d.dev[i], (size_t)lens[i] * sizeof(double), hipMemcpyDeviceToDevice));
    }
  }
  std::vector<GemmProb> probs;
  for (int p = 0; p < nprob; ++p) {
    const gpe_gemm_group_prob& g = gp[p];
    GemmProb q = mkprob(d.dev[g.a_buf] + g.a_off, g.lda, d.dev[g.b_buf] + g.b_off, g.ldb, d.dev[g.c_buf] + g.c_off, g.ldc,
                        g.mt, g.nt, g.K, g.flags, g.alpha, g.beta);
    q.kti_mul = g.kti_mul;
    q.kti_off = g.kti_off;
    probs.push_back(q);
  }
  if (gl.split) {
    // the partials start as NaN: a slot the sum reads but no share wrote shows in C
    CHK(dalloc(c, &d.part, (size_t)SPLIT_SLOTS * TILE * TILE));
    CHK(dalloc(c, &d.tcnt, (size_t)SPLIT_SLOTS));
    HIPCHK(c, hipMemset(d.part, 0xff, (size_t)SPLIT_SLOTS * TILE * TILE * sizeof(double)));
    HIPCHK(c, hipMemset(d.tcnt, 0, (size_t)SPLIT_SLOTS * sizeof(int)));
    split_k(probs, d.part, d.tcnt);
  }
  Plan pl;
  add_launch(pl, kind, probs, 0.0);
  GemmLaunch L = pl.launches[0];
  if (!gl.listed) L.list = -1;
  if (L.list >= 0 && (long long)pl.tiles.size() > tiles_cap) return bad("the tile list does not fit tiles_cap");
  CHK(dalloc(c, &d.probs, pl.probs.size()));
  HIPCHK(c, hipMemcpy(d.probs, pl.probs.data(), pl.probs.size() * sizeof(GemmProb), hipMemcpyHostToDevice));
  if (L.list >= 0) {
    CHK(dalloc(c, &d.tiles, pl.tiles.size()));
    HIPCHK(c, hipMemcpy(d.tiles, pl.tiles.data(), pl.tiles.size() * sizeof(unsigned), hipMemcpyHostToDevice));
  }
  // launch_gemm_range reads the context's descriptor and list arrays: the hook's stand in
  // for them until it returns (GemmGroupBufs puts the context's back)
  c->dprobs = d.probs;
  c->dtiles = d.tiles;
  HIPCHK(c, hipMemsetAsync(c->dinfo, 0, sizeof(int), c->stream));
  for (int r = 0; r < gl.reps; ++r) {
    if (r > 0)
      for (int i = 0; i < nbuf; ++i)
        if (d.keep[i])
          HIPCHK(c, hipMemcpyAsync(d.dev[i], d.keep[i], (size_t)lens[i] * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    CHK(launch_gemm_range(c, L));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < nbuf; ++i)
    HIPCHK(c, hipMemcpy(bufs[i], d.dev[i], (size_t)lens[i] * sizeof(double), hipMemcpyDeviceToHost));
  for (int p = 0; p < nprob; ++p) ksplit_out[p] = pl.probs[p].ksplit;
  info_out[0] = L.list >= 0;
  info_out[1] = L.cdef;
  info_out[2] = L.tiles;
  if (L.list >= 0) std::copy(pl.tiles.begin(), pl.tiles.end(), tiles_out);
  return GPE_OK;
}

int gpe_test_gemm_group(gpe_ctx* c, int32_t nbuf, double* const* bufs, const int64_t* lens, int32_t nprob,
                        const gpe_gemm_group_prob* probs, const gpe_gemm_group_launch* launch, int32_t* ksplit_out,
                        int32_t* info_out, uint32_t* tiles_out, int64_t tiles_cap) {
  if (!c) return GPE_ERR_ARG;
  if (!bufs || !lens || !probs || !launch || !ksplit_out || !info_out)
    return fail(c, GPE_ERR_ARG, "gpe_test_gemm_group: NULL argument");
  return gemm_group_test(c, nbuf, bufs, lens, nprob, probs, *launch, ksplit_out, info_out, tiles_out, tiles_cap);
}

int gpe_bench_gemm(gpe_ctx* c, int32_t trans_a, int32_t trans_b, int32_t mt, int32_t nt, int32_t K,
                   int32_t lower, double beta, int32_t reps, double* ms_out) {
  if (!c || !ms_out || mt <= 0 || nt <= 0 || K <= 0 || K % GK || reps <= 0) return GPE_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const long long M = (long long)mt * TILE, N = (long long)nt * TILE;
  double *da = nullptr, *db = nullptr, *dc = nullptr;
  int rc = dalloc(c, &da, (size_t)M * K);
  if (rc == GPE_OK) rc = dalloc(c, &db, (size_t)K * N);
  if (rc == GPE_OK) rc = dalloc(c, &dc, (size_t)M * N);
  if (rc == GPE_OK) {
    // deterministic non-trivial fill via the pair kernel is overkill: a memset-free pattern
    std::vector<double> h((size_t)std::max<long long>(M, N) * 64);
    for (size_t i = 0; i < h.size(); ++i) h[i] = std::sin(0.37 * (double)i) * 0.5;
    auto fill = [&](double* dp, size_t cnt) {
      for (size_t off = 0; off < cnt; off += h.size())
        (void)hipMemcpy(dp + off, h.data(), std::min(h.size(), cnt - off) * sizeof(double), hipMemcpyHostToDevice);
    };
    fill(da, (size_t)M * K);
    fill(db, (size_t)K * N);
    fill(dc, (size_t)M * N);
    long long lda = trans_a ? K : M, ldb = trans_b ? K : N;
    // diagnostics: GPEMU_BENCH_HOT=1 cache-resident operands (every k re-reads the same
    // 128 values); =2 operands from a window of (tiles + K) x 128 doubles (ld = 128: L2-
    // resident, every k still reads other values, so the MFMA inputs toggle as when cold)
    if (const char* hot = std::getenv("GPEMU_BENCH_HOT")) lda = ldb = (std::atoi(hot) == 2) ? TILE : 0;
    const GemmProb p = mkprob(da, lda, db, ldb, dc, M, mt, nt, K, lower ? G_CLOWER : 0, -1.0, beta);
    const GemmKind kind = gemm_kind(trans_a != 0, trans_b != 0);
    GemmLaunch L{};
    rc = adhoc_gemm(c, ADHOC_BENCH, {{kind, p}}, &L, true);
    HIPCHK(c, hipMemsetAsync(c->dinfo, 0, sizeof(int), c->stream));
    const bool prof = c->prof;
    c->prof = false;
    if (rc == GPE_OK) rc = launch_gemm_range(c, L);   // warm-up
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, c->stream);
    for (int r = 0; r < reps && rc == GPE_OK; ++r) rc = launch_gemm_range(c, L);
    (void)hipEventRecord(e1, c->stream);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    *ms_out = ms / reps;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    c->prof = prof;
  }
  if (da) (void)hipFree(da);
  if (db) (void)hipFree(db);
  if (dc) (void)hipFree(dc);
  return rc;
}

}  // extern "C"


// ---------------------------------------------------------------- history matching
// A set of emulators resident on one GPU (gpe_hm_*; kernels in gpemu_hm.hpp, layouts and sizes
// in gpemu_hm_plan.hpp).  gpe_hm_add snapshots what the posterior of a context's resident factor
// needs into buffers the set owns; gpe_hm_implausibility runs the candidates through every
// emulator chunk by chunk on the set's own stream.

namespace {

// One emulator: its device buffer (dev, one allocation) and the arrays inside it
// (a member): p = 0 an emulator of gpe_hm_add, p >= 1 the p outputs of gpe_hm_add_multi, whose
// beta holds B (q x p row-major) and whose sdiag Sigma's diagonal; first: its first output's
// place among the set's outputs
struct HmEmul {
  int n = 0, d = 0, q = 0, fam = 0, pt = 0, maxact = 0, p = 0, first = 0;
  double s2 = 0.0, coff = 0.0, cdiag = 0.0;
  double* dev = nullptr;
  double *xw = nullptr, *invdelta = nullptr, *W = nullptr, *beta = nullptr, *kinv = nullptr, *hval = nullptr,
         *sdiag = nullptr;
  int *active = nullptr, *hdim = nullptr;
  std::vector<double> Sigma;   // p x p (host: the joint measure's diagonalisation, once per call)
  int outputs() const { return p ? p : 1; }
};

}  // namespace

struct gpe_hm {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  std::vector<HmEmul> em;
  int outputs = 0;           // the members' outputs together: at most HM_MAX_EMUL
  long long chunk = HM_CHUNK_DEFAULT;
  hipEvent_t ev_ctx = nullptr, ev_set = nullptr;   // gpe_hm_add: the context's stream <-> the set's
  hipEvent_t ev_pipe[2] = {nullptr, nullptr};      // the chunk pipeline's result slots
  double* dwork = nullptr;   // one chunk: the points, I^2, the parts, the selection
  size_t work_cap = 0;
  double* hpin = nullptr;    // two slots of points, two of results
  size_t hpin_cap = 0;
};

namespace {

thread_local std::string g_hm_create_error;

int hm_fail(gpe_hm* h, int code, const std::string& msg) {
  h->err = msg;
  return code;
}

#define HM_HIPCHK(h, expr)                                                  \
  do {                                                                      \
    hipError_t e_ = (expr);                                                 \
    if (e_ != hipSuccess) {                                                 \
      (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);         \
      return GPE_ERR_HIP;                                                   \
    }                                                                       \
  } while (0)

template <int FAM, int PT>
bool hm_lds_attr_one() {
  return hipFuncSetAttribute((const void*)k_hm_post<FAM, PT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             HM_LDS_BYTES) == hipSuccess &&
         hipFuncSetAttribute((const void*)k_hm_post<FAM, PT, HmPostMultiArgs>,
                             hipFuncAttributeMaxDynamicSharedMemorySize, HM_LDS_BYTES) == hipSuccess;
}
template <int FAM>
bool hm_lds_attr() {
  return hm_lds_attr_one<FAM, HM_PT_WIDE>() && hm_lds_attr_one<FAM, HM_PT_NARROW>();
}

// k_hm_post<FAM, PT, Args> for one member and one chunk (Args: HmPostArgs, HmPostMultiArgs)
template <class Args>
void hm_launch_post(const HmEmul& e, dim3 g, size_t lds, hipStream_t st, const Args& a) {
  with_fam(e.fam, [&](auto F) {
    constexpr int FAM = decltype(F)::value;
    if (e.pt == HM_PT_WIDE) hipLaunchKernelGGL((k_hm_post<FAM, HM_PT_WIDE, Args>), g, dim3(HM_LANES), lds, st, a);
    else hipLaunchKernelGGL((k_hm_post<FAM, HM_PT_NARROW, Args>), g, dim3(HM_LANES), lds, st, a);
  });
}

// What every k_hm_post instance reads of a member, for a chunk of mc candidates at dX
void hm_post_args(const HmEmul& e, const double* dX, int D, long long mc, HmPostArgs& a) {
  a.xw = e.xw; a.invdelta = e.invdelta; a.active = e.active; a.W = e.W; a.hdim = e.hdim; a.hval = e.hval;
  a.beta = e.beta; a.kinv = e.kinv; a.Xs = dX;
  a.s2 = e.s2; a.coff = e.coff; a.cdiag = e.cdiag;
  a.n = e.n; a.d = e.d; a.q = e.q; a.D = D; a.mc = (int)mc;
}
void hm_multi_args(const HmEmul& e, HmPostMultiArgs& a) {
  a.B = e.beta; a.sdiag = e.sdiag; a.Wj = nullptr; a.lam = nullptr; a.p = e.p;
}

// The univariate post kernels of one chunk of mc candidates at dX: every member whose bit of `use`
// is set (a member's bit is its first output's) writes its outputs' I^2 to dI2 (p x cl) and, where
// dparts is given, its means and variances to dparts (mean p x cl, then var p x cl).
int hm_post_all(gpe_hm* h, const double* dX, int D, long long mc, long long cl, const double* z, const double* var_extra,
                unsigned use, double* dI2, double* dparts) {
  const int p = h->outputs;
  for (const HmEmul& e : h->em) {
    const int o = e.first;
    if (!((use >> o) & 1u)) continue;
    const dim3 grid((unsigned)hm_tiles(mc, e.pt));
    const size_t lds = (size_t)hm_lds_doubles(e.n, e.pt) * sizeof(double);
    if (e.p) {
      HmPostMultiArgs a = {};
      hm_post_args(e, dX, D, mc, a);
      hm_multi_args(e, a);
      a.i2 = dI2 + o * cl; a.ldo = cl; a.joint = 0;
      a.mean = dparts ? dparts + o * cl : nullptr;
      a.var = dparts ? dparts + (p + o) * cl : nullptr;
      for (int j = 0; j < e.p; ++j) a.zs[j] = z[o + j], a.ves[j] = var_extra[o + j];
      hm_launch_post(e, grid, lds, h->stream, a);
    } else {
      HmPostArgs a;
      hm_post_args(e, dX, D, mc, a);
      a.i2 = dI2 + o * cl;
      a.mean = dparts ? dparts + o * cl : nullptr;
      a.var = dparts ? dparts + (p + o) * cl : nullptr;
      a.z = z[o]; a.ve = var_extra[o];
      hm_launch_post(e, grid, lds, h->stream, a);
    }
    HM_HIPCHK(h, hipGetLastError());
  }
  return GPE_OK;
}

// The set's chunk buffers: dev doubles on the device, pin pinned doubles, grown when too small
int hm_workspace(gpe_hm* h, size_t dev, size_t pin) {
  if (dev > h->work_cap) {
    if (h->dwork) (void)hipFree(h->dwork);
    h->dwork = nullptr, h->work_cap = 0;
    HM_HIPCHK(h, hipMalloc((void**)&h->dwork, dev * sizeof(double)));
    h->work_cap = dev;
  }
  if (pin > h->hpin_cap) {
    if (h->hpin) (void)hipHostFree(h->hpin);
    h->hpin = nullptr, h->hpin_cap = 0;
    HM_HIPCHK(h, hipHostMalloc((void**)&h->hpin, pin * sizeof(double), hipHostMallocDefault));
    h->hpin_cap = pin;
  }
  return GPE_OK;
}

// The snapshot of gpe_hm_add, behind the checks: [gamma, G], Kq^-1 and the kernel's constants
// by Posterior::setup() on the context (scratch buffers only: what gpe_posterior itself
// overwrites on every call), then the copies on the set's stream, ordered behind the context's
// stream by ev_ctx; the context's stream waits for them (ev_set) before it goes on.
// pm = 0: an emulator of gpe_hm_add (beta, sigma).  pm >= 1: the pm outputs of gpe_hm_add_multi:
// beta is B (q x pm), Sigma pm x pm; G and Kq^-1 come from setup() at sigma = 1 (they do not
// depend on its beta, taken as zero), Gamma from multi_gamma() into dWm.
int hm_snapshot(gpe_hm* h, gpe_ctx* c, const int32_t* active, const int32_t* hdim, const double* hval,
                const double* beta, double sigma, int pm, const double* Sigma, HmEmul& e) {
  const int n = (int)c->n, d = c->d, q = c->q;
  const long long np = c->n_pad;
  const std::vector<double> zero((size_t)q, 0.0);
  PostReq r{0, nullptr, nullptr, pm ? zero.data() : beta, sigma, 64, nullptr, PostVar::DIAG, nullptr};
  Posterior S(c, r);
  CHK(S.setup());
  if (pm) {   // (setup() has waited for the stream: the pinned buffer is free)
    CHK(ensure_pinned(c, (size_t)(pm + q) * pm + 64));
    CHK(multi_gamma(c, beta, c->hpin));
  }
  e.n = n; e.d = d; e.q = q; e.fam = S.fam; e.pt = hm_pt(n); e.p = pm;
  e.s2 = S.s2; e.coff = S.coff; e.cdiag = S.cdiag;
  e.maxact = 0;
  for (int k = 0; k < d; ++k) e.maxact = std::max(e.maxact, (int)active[k]);
  const int rows = pm ? pm + q : 1 + q;
  const size_t nW = (size_t)hm_packed_size_rows(n, rows), nint = ((size_t)d + q + 1) / 2 + 1;
  const size_t nbeta = pm ? (size_t)q * pm : (size_t)q;
  const size_t sz[] = {(size_t)n * d, (size_t)d, nW, nbeta, (size_t)q * q, (size_t)q, (size_t)pm, nint};
  size_t tot = 0;
  for (size_t s : sz) tot += s;
  HM_HIPCHK(h, hipMalloc((void**)&e.dev, tot * sizeof(double)));
  double* p = e.dev;
  e.xw = p, p += sz[0];
  e.invdelta = p, p += sz[1];
  e.W = p, p += sz[2];
  e.beta = p, p += sz[3];
  e.kinv = p, p += sz[4];
  e.hval = p, p += sz[5];
  e.sdiag = p, p += sz[6];
  e.active = reinterpret_cast<int*>(p);
  e.hdim = e.active + d;
  // the small arrays lie together behind W: one blocking copy
  std::vector<double> hs(sz[3] + sz[4] + sz[5] + sz[6] + sz[7], 0.0);
  double* hp = hs.data();
  std::memcpy(hp, beta, nbeta * sizeof(double)), hp += nbeta;
  std::memcpy(hp, S.Kinv.data(), (size_t)q * q * sizeof(double)), hp += (size_t)q * q;
  std::memcpy(hp, hval, (size_t)q * sizeof(double)), hp += q;
  for (int a = 0; a < pm; ++a) *hp++ = Sigma[(size_t)a * pm + a];
  if (pm) e.Sigma.assign(Sigma, Sigma + (size_t)pm * pm);
  int* hi = reinterpret_cast<int*>(hp);
  for (int k = 0; k < d; ++k) hi[k] = active[k];
  for (int j = 0; j < q; ++j) hi[d + j] = hdim[j];
  HM_HIPCHK(h, hipMemcpy(e.beta, hs.data(), hs.size() * sizeof(double), hipMemcpyHostToDevice));
  std::vector<double> idl((size_t)d);
  for (int k = 0; k < d; ++k) idl[k] = 1.0 / c->f_delta[k];   // (as upload_invdelta)
  HM_HIPCHK(h, hipMemcpy(e.invdelta, idl.data(), (size_t)d * sizeof(double), hipMemcpyHostToDevice));
  HM_HIPCHK(h, hipEventRecord(h->ev_ctx, c->stream));
  HM_HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_ctx, 0));
  HM_HIPCHK(h, hipMemcpyAsync(e.xw, c->dXw, (size_t)n * d * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  // [gamma, G] is dWa; [Gamma, G] is dWm's first pm columns and dWa's columns 1 .. q
  hipLaunchKernelGGL(k_hm_pack, dim3((unsigned)hm_nblocks_rows(n, rows)), dim3(256), 0, h->stream, c->tr.B,
                     pm ? c->dWm : c->dWa, c->dWa + np, np, n, pm ? pm : 1, q, e.W);
  HM_HIPCHK(h, hipGetLastError());
  HM_HIPCHK(h, hipEventRecord(h->ev_set, h->stream));
  HM_HIPCHK(h, hipStreamWaitEvent(c->stream, h->ev_set, 0));
  HM_HIPCHK(h, hipStreamSynchronize(h->stream));
  return GPE_OK;
}

// gpe_hm_add and gpe_hm_add_multi behind their own checks: active and hdim, the triangular
// inverse, the snapshot; the member joins the set only when all of it succeeded.
int hm_add_member(gpe_hm* h, gpe_ctx* c, int d, const int32_t* active, int q, const int32_t* hdim,
                  const double* hval, const double* beta, double sigma, int pm, const double* Sigma) {
  for (int k = 0; k < d; ++k)
    if (active[k] < 0) return hm_fail(h, GPE_ERR_ARG, "active[" + std::to_string(k) + "] is negative");
  for (int j = 0; j < q; ++j)
    if (hdim[j] < -1 || hdim[j] >= d) return hm_fail(h, GPE_ERR_ARG, "hdim[" + std::to_string(j) + "] is outside [-1, d)");
  HM_HIPCHK(h, hipSetDevice(h->device));
  HmEmul e;
  int rc = ensure_linv(c);
  if (rc == GPE_OK) rc = hm_snapshot(h, c, active, hdim, hval, beta, sigma, pm, Sigma, e);
  if (rc != GPE_OK) {
    // (the copies may be queued: they end before the buffer goes)
    (void)hipStreamSynchronize(h->stream);
    if (e.dev) (void)hipFree(e.dev);
    if (h->err.empty()) h->err = c->err;
    return rc;
  }
  e.first = h->outputs;
  h->outputs += e.outputs();
  h->em.push_back(e);
  return (int)h->em.size() - 1;
}

}  // namespace

extern "C" {

gpe_hm* gpe_hm_create(int32_t device) {
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    g_hm_create_error = std::string("no HIP device available: ") + hipGetErrorString(e);
    return nullptr;
  }
  if (device < 0 || device >= ndev) {
    g_hm_create_error = "device index out of range";
    return nullptr;
  }
  gpe_hm* h = new gpe_hm();
  h->device = device;
  if (const char* ec = std::getenv("GPEMU_HM_CHUNK")) h->chunk = hm_chunk(std::atoll(ec));
  bool ok = hipSetDevice(device) == hipSuccess &&
            hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&h->ev_ctx, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&h->ev_set, hipEventDisableTiming) == hipSuccess;
  for (hipEvent_t& ev : h->ev_pipe) ok = ok && hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess;
  ok = ok && hm_lds_attr<FAM_GAUSS>() && hm_lds_attr<FAM_MATERN32>() && hm_lds_attr<FAM_MATERN52>();
  if (!ok) {
    g_hm_create_error = "failed to initialise the set's stream, events or kernels";
    gpe_hm_destroy(h);
    return nullptr;
  }
  return h;
}

void gpe_hm_destroy(gpe_hm* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (HmEmul& e : h->em)
    if (e.dev) (void)hipFree(e.dev);
  if (h->dwork) (void)hipFree(h->dwork);
  if (h->hpin) (void)hipHostFree(h->hpin);
  for (hipEvent_t ev : {h->ev_ctx, h->ev_set, h->ev_pipe[0], h->ev_pipe[1]})
    if (ev) (void)hipEventDestroy(ev);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

const char* gpe_hm_last_error(const gpe_hm* h) {
  if (!h) return g_hm_create_error.c_str();
  return h->err.c_str();
}

int gpe_hm_count(const gpe_hm* h) { return h ? (int)h->em.size() : GPE_ERR_ARG; }

int gpe_hm_add(gpe_hm* h, gpe_ctx* c, int32_t d, const int32_t* active, int32_t q, const int32_t* hdim,
               const double* hval, const double* beta, double sigma) {
  if (!h) return GPE_ERR_ARG;
  h->err.clear();
  if (!c || !active || !hdim || !hval || !beta) return hm_fail(h, GPE_ERR_ARG, "bad hm_add args (a NULL pointer)");
  if (c->device != h->device) return hm_fail(h, GPE_ERR_ARG, "the context is on another device than the set");
  if (c->n <= 0 || !c->factor_valid) return hm_fail(h, GPE_ERR_STATE, "no resident factor (call gpe_factor)");
  if (d != c->d || q != c->q) return hm_fail(h, GPE_ERR_ARG, "d and q must be those of the context's data");
  if (c->n > HM_MAX_N || d > HM_MAX_D || q > HM_MAX_Q || h->outputs >= HM_MAX_EMUL)
    return hm_fail(h, GPE_ERR_UNSUPPORTED, "an emulator of a set has n <= 512, d <= 32, q <= 16; a set at most 32");
  return hm_add_member(h, c, d, active, q, hdim, hval, beta, sigma, 0, nullptr);
}

int gpe_hm_add_multi(gpe_hm* h, gpe_ctx* c, int32_t d, const int32_t* active, int32_t q, const int32_t* hdim,
                     const double* hval, int32_t p, const double* B, const double* Sigma) {
  if (!h) return GPE_ERR_ARG;
  h->err.clear();
  if (!c || !active || !hdim || !hval || !B || !Sigma)
    return hm_fail(h, GPE_ERR_ARG, "bad hm_add_multi args (a NULL pointer)");
  if (c->device != h->device) return hm_fail(h, GPE_ERR_ARG, "the context is on another device than the set");
  if (c->n <= 0 || !c->factor_valid) return hm_fail(h, GPE_ERR_STATE, "no resident factor (call gpe_factor)");
  if (!c->mo_p) return hm_fail(h, GPE_ERR_STATE, "gpe_set_outputs has not been called for this data");
  if (d != c->d || q != c->q) return hm_fail(h, GPE_ERR_ARG, "d and q must be those of the context's data");
  if (p != c->mo_p) return hm_fail(h, GPE_ERR_ARG, "p must be the number of outputs of gpe_set_outputs");
  if (c->n > HM_MAX_N || d > HM_MAX_D || q > HM_MAX_Q || p + q > HM_MAX_ROWS || h->outputs + p > HM_MAX_EMUL)
    return hm_fail(h, GPE_ERR_UNSUPPORTED,
                   "a multi-output member of a set has n <= 512, d <= 32, q <= 16, p + q <= 32; a set at most 32 outputs");
  return hm_add_member(h, c, d, active, q, hdim, hval, B, 1.0, p, Sigma);
}

int gpe_hm_outputs(const gpe_hm* h) { return h ? h->outputs : GPE_ERR_ARG; }

int gpe_hm_member_outputs(const gpe_hm* h, int32_t member) {
  if (!h || member < 0 || member >= (int)h->em.size()) return GPE_ERR_ARG;
  return h->em[member].outputs();
}

int gpe_hm_implausibility(gpe_hm* h, int64_t m, int32_t D, const double* Xs, const double* z, const double* var_extra,
                          int32_t maxno, double* imax_out, double* mean_out, double* var_out) {
  if (!h) return GPE_ERR_ARG;
  const int p = h->outputs;   // (the members' outputs: the emulators of a set of gpe_hm_add members)
  if (p == 0) return hm_fail(h, GPE_ERR_STATE, "the set is empty (call gpe_hm_add)");
  if (m <= 0 || !Xs || !z || !var_extra || !imax_out)
    return hm_fail(h, GPE_ERR_ARG, "bad hm_implausibility args (m >= 1; Xs, z, var_extra and imax_out not NULL)");
  if (maxno < 1 || maxno > p) return hm_fail(h, GPE_ERR_ARG, "maxno must be in [1, emulators of the set]");
  for (const HmEmul& e : h->em)
    if (D <= e.maxact) return hm_fail(h, GPE_ERR_ARG, "D is smaller than an emulator's largest active index + 1");
  if ((mean_out == nullptr) != (var_out == nullptr))
    return hm_fail(h, GPE_ERR_ARG, "mean_out and var_out go together (both or neither)");
  HM_HIPCHK(h, hipSetDevice(h->device));
  const bool parts = mean_out != nullptr;
  const long long CH = h->chunk, cl = std::min<long long>(CH, m);
  const HmWork w = hm_work(cl, D, p, maxno, parts);
  if (int rc = hm_workspace(h, (size_t)w.dev(), 2 * (size_t)(w.pin_in() + w.pin_out()))) return rc;
  double* dX = h->dwork;
  double* dI2 = dX + w.pts;
  double* dparts = dI2 + w.i2;       // mean (p x cl), then var (p x cl)
  double* dsel = dparts + w.parts;
  double* pin_in[2] = {h->hpin, h->hpin + w.pin_in()};
  double* pin_out[2] = {pin_in[1] + w.pin_in(), pin_in[1] + w.pin_in() + w.pin_out()};
  auto dev = [&](long long s0, int slot) -> int {
    const long long mc = std::min(CH, m - s0);
    std::memcpy(pin_in[slot], Xs + s0 * D, (size_t)mc * D * sizeof(double));
    HM_HIPCHK(h, hipMemcpyAsync(dX, pin_in[slot], (size_t)mc * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (int rc = hm_post_all(h, dX, D, mc, cl, z, var_extra, ~0u, dI2, parts ? dparts : nullptr)) return rc;
    hipLaunchKernelGGL(k_hm_select, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, h->stream, dI2, cl, p, (int)maxno,
                       (int)mc, dsel);
    HM_HIPCHK(h, hipGetLastError());
    // (the parts keep the leading dimension cl on both sides: one copy whatever mc is)
    HM_HIPCHK(h, hipMemcpyAsync(pin_out[slot], dsel, (size_t)mc * maxno * sizeof(double), hipMemcpyDeviceToHost,
                                h->stream));
    if (parts)
      HM_HIPCHK(h, hipMemcpyAsync(pin_out[slot] + w.sel, dparts, (size_t)w.parts * sizeof(double), hipMemcpyDeviceToHost,
                                  h->stream));
    HM_HIPCHK(h, hipEventRecord(h->ev_pipe[slot], h->stream));
    return GPE_OK;
  };
  auto host = [&](long long s0, int slot) {
    const long long mc = std::min(CH, m - s0);
    std::memcpy(imax_out + s0 * maxno, pin_out[slot], (size_t)mc * maxno * sizeof(double));
    if (!parts) return;
    const double* src = pin_out[slot] + w.sel;
    for (int o = 0; o < p; ++o) {
      std::memcpy(mean_out + (long long)o * m + s0, src + o * cl, (size_t)mc * sizeof(double));
      std::memcpy(var_out + (long long)o * m + s0, src + (p + o) * cl, (size_t)mc * sizeof(double));
    }
  };
  return chunk_pipeline(
      m, CH, dev,
      [&](int slot) -> int {
        HM_HIPCHK(h, hipEventSynchronize(h->ev_pipe[slot]));
        return GPE_OK;
      },
      host, [&] { (void)hipStreamSynchronize(h->stream); });
}

int gpe_hm_implausibility_mv(gpe_hm* h, int32_t member, int64_t m, int32_t D, const double* Xs, const double* z,
                             const double* V, double* i2_out, double* mean_out, double* c_out) {
  if (!h) return GPE_ERR_ARG;
  h->err.clear();
  if (member < 0 || member >= (int)h->em.size() || h->em[member].p == 0)
    return hm_fail(h, GPE_ERR_ARG, "member must be a multi-output member of the set (gpe_hm_add_multi)");
  if (m <= 0 || !Xs || !z || !V || !i2_out)
    return hm_fail(h, GPE_ERR_ARG, "bad hm_implausibility_mv args (m >= 1; Xs, z, V and i2_out not NULL)");
  const HmEmul& e = h->em[member];
  if (D <= e.maxact) return hm_fail(h, GPE_ERR_ARG, "D is smaller than the member's largest active index + 1");
  if ((mean_out == nullptr) != (c_out == nullptr))
    return hm_fail(h, GPE_ERR_ARG, "mean_out and c_out go together (both or neither)");
  const int p = e.p;
  // W^T V W = I, W^T Sigma W = Lambda: [W (p x p), lambda (p)] behind the chunk's buffers
  std::vector<double> wl((size_t)p * p + p);
  if (hm_mv_prepare(p, e.Sigma.data(), V, wl.data(), wl.data() + (size_t)p * p))
    return hm_fail(h, GPE_NOT_PD, "V is not positive definite");
  HM_HIPCHK(h, hipSetDevice(h->device));
  const bool parts = mean_out != nullptr;
  const long long CH = h->chunk, cl = std::min<long long>(CH, m);
  const HmWork w = hm_work_mv(cl, D, p, parts);
  if (int rc = hm_workspace(h, (size_t)w.dev() + wl.size(), 2 * (size_t)(w.pin_in() + w.pin_out()))) return rc;
  double* dX = h->dwork;
  double* dparts = dX + w.pts;       // mean (p x cl), then c (cl)
  double* dI2 = dparts + w.parts;
  double* dW = dI2 + w.sel;
  // (every earlier call has ended: a blocking copy, once per call)
  HM_HIPCHK(h, hipMemcpy(dW, wl.data(), wl.size() * sizeof(double), hipMemcpyHostToDevice));
  double* pin_in[2] = {h->hpin, h->hpin + w.pin_in()};
  double* pin_out[2] = {pin_in[1] + w.pin_in(), pin_in[1] + w.pin_in() + w.pin_out()};
  auto dev = [&](long long s0, int slot) -> int {
    const long long mc = std::min(CH, m - s0);
    std::memcpy(pin_in[slot], Xs + s0 * D, (size_t)mc * D * sizeof(double));
    HM_HIPCHK(h, hipMemcpyAsync(dX, pin_in[slot], (size_t)mc * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HmPostMultiArgs a = {};
    hm_post_args(e, dX, D, mc, a);
    hm_multi_args(e, a);
    a.Wj = dW; a.lam = dW + (size_t)p * p; a.joint = 1;
    a.i2 = dI2; a.ldo = cl;
    a.mean = parts ? dparts : nullptr;
    a.var = parts ? dparts + (long long)p * cl : nullptr;
    for (int j = 0; j < p; ++j) a.zs[j] = z[j];
    hm_launch_post(e, dim3((unsigned)hm_tiles(mc, e.pt)), (size_t)hm_lds_doubles(e.n, e.pt) * sizeof(double), h->stream,
                   a);
    HM_HIPCHK(h, hipGetLastError());
    HM_HIPCHK(h, hipMemcpyAsync(pin_out[slot], dI2, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (parts)
      HM_HIPCHK(h, hipMemcpyAsync(pin_out[slot] + w.sel, dparts, (size_t)w.parts * sizeof(double), hipMemcpyDeviceToHost,
                                  h->stream));
    HM_HIPCHK(h, hipEventRecord(h->ev_pipe[slot], h->stream));
    return GPE_OK;
  };
  auto host = [&](long long s0, int slot) {
    const long long mc = std::min(CH, m - s0);
    std::memcpy(i2_out + s0, pin_out[slot], (size_t)mc * sizeof(double));
    if (!parts) return;
    const double* src = pin_out[slot] + w.sel;
    for (int o = 0; o < p; ++o) std::memcpy(mean_out + (long long)o * m + s0, src + o * cl, (size_t)mc * sizeof(double));
    std::memcpy(c_out + s0, src + (long long)p * cl, (size_t)mc * sizeof(double));
  };
  return chunk_pipeline(
      m, CH, dev,
      [&](int slot) -> int {
        HM_HIPCHK(h, hipEventSynchronize(h->ev_pipe[slot]));
        return GPE_OK;
      },
      host, [&] { (void)hipStreamSynchronize(h->stream); });
}

}  // extern "C"

// ---- candidates made and reduced on the device (kernels in gpemu_hm_cand.hpp) ----
namespace {

struct HmMesh {
  int32_t D, ca, cb, g1, g2;
  const double *x1, *x2, *others;
  int64_t ns;
};

// what gpe_hm_cells and gpe_hm_cells_mv check of the mesh, before any device work
int hm_mesh_check(gpe_hm* h, const HmMesh& m, const double* imp_out, const int64_t* below_out) {
  if (m.g1 < 1 || m.g2 < 1 || m.ns < 1) return hm_fail(h, GPE_ERR_ARG, "g1, g2 and ns must be at least 1");
  if (m.D < 2 || m.ca < 0 || m.cb < 0 || m.ca >= m.D || m.cb >= m.D || m.ca == m.cb)
    return hm_fail(h, GPE_ERR_ARG, "ca and cb must be two different columns in [0, D), D >= 2");
  if (!m.x1 || !m.x2 || !imp_out || !below_out || (m.D > 2 && !m.others))
    return hm_fail(h, GPE_ERR_ARG, "bad hm_cells args (a NULL pointer)");
  if ((double)m.g1 * (double)m.g2 * (double)m.ns >= (double)HM_CELLS_MAX)
    return hm_fail(h, GPE_ERR_ARG, "g1 g2 ns must be below 2^40");
  return GPE_OK;
}

// The chunks of a mesh: generator, `post` (the caller's post kernels: dX, mc -> dI2), reducer,
// queued one after the other with no synchronisation; then the accumulators come back.
// p outputs in dI2 (leading dimension cl; p = 0: the one row of the joint measure), `use` their
// flags; extra: words behind the workspace
// for the caller (their place is returned in *dextra before the first chunk).
template <class Post>
int hm_cells_run(gpe_hm* h, const HmMesh& m, int p, int maxno, unsigned use, double cm, long long extra,
                 const double* extra_host, double** dextra, double* imp_out, int64_t* below_out, Post post) {
  HM_HIPCHK(h, hipSetDevice(h->device));
  const long long cells = (long long)m.g1 * m.g2, M = cells * m.ns;
  const long long CH = h->chunk, cl = std::min<long long>(CH, M);
  const HmCellsWork w = hm_work_cells(cl, m.D, p, maxno, m.g1, m.g2, m.ns, extra);
  if (int rc = hm_workspace(h, (size_t)w.dev(), 0)) return rc;
  double* dX = h->dwork;
  double* dI2 = dX + w.pts;
  double* dx1 = dI2 + w.i2;
  double* dx2 = dx1 + m.g1;
  double* doth = dx2 + m.g2;
  double* dimp = dx1 + w.mesh;
  long long* dbelow = reinterpret_cast<long long*>(dimp + w.acc);
  *dextra = dimp + 2 * w.acc;
  // (every earlier call has ended: blocking copies, once per call)
  HM_HIPCHK(h, hipMemcpy(dx1, m.x1, (size_t)m.g1 * sizeof(double), hipMemcpyHostToDevice));
  HM_HIPCHK(h, hipMemcpy(dx2, m.x2, (size_t)m.g2 * sizeof(double), hipMemcpyHostToDevice));
  if (m.D > 2)
    HM_HIPCHK(h, hipMemcpy(doth, m.others, (size_t)m.ns * (m.D - 2) * sizeof(double), hipMemcpyHostToDevice));
  if (extra) HM_HIPCHK(h, hipMemcpy(*dextra, extra_host, (size_t)extra * sizeof(double), hipMemcpyHostToDevice));
  int rc = GPE_OK;
  for (long long s0 = 0; s0 < M && rc == GPE_OK; s0 += CH) {
    const long long mc = std::min(CH, M - s0);
    hipLaunchKernelGGL(k_hm_mesh, dim3((unsigned)((mc * m.D + 255) / 256)), dim3(256), 0, h->stream, dx1, dx2, doth,
                       (int)m.D, (int)m.ca, (int)m.cb, (long long)m.g2, (long long)m.ns, s0, mc, dX);
    rc = post(dX, dI2, cl, mc);
    if (rc != GPE_OK) break;
    const dim3 pieces((unsigned)hm_pieces(s0, mc, m.ns));
    if (hm_top_slots(maxno) == HM_TOP_FEW)
      hipLaunchKernelGGL(k_hm_cells<HM_TOP_FEW>, pieces, dim3(HM_LANES), 0, h->stream, dI2, cl, p ? p : 1, maxno, use, cm,
                         s0, mc, (long long)m.ns, cells, dimp, dbelow);
    else
      hipLaunchKernelGGL(k_hm_cells<HM_MAX_EMUL>, pieces, dim3(HM_LANES), 0, h->stream, dI2, cl, p ? p : 1, maxno, use, cm,
                         s0, mc, (long long)m.ns, cells, dimp, dbelow);
    if (hipGetLastError() != hipSuccess) rc = hm_fail(h, GPE_ERR_HIP, "a launch of gpe_hm_cells failed");
  }
  hipError_t e = hipStreamSynchronize(h->stream);
  if (rc != GPE_OK) return rc;
  HM_HIPCHK(h, e);
  HM_HIPCHK(h, hipMemcpy(imp_out, dimp, (size_t)w.acc * sizeof(double), hipMemcpyDeviceToHost));
  HM_HIPCHK(h, hipMemcpy(below_out, dbelow, (size_t)w.acc * sizeof(long long), hipMemcpyDeviceToHost));
  return GPE_OK;
}

}  // namespace

extern "C" {

int gpe_hm_cells(gpe_hm* h, int32_t D, int32_t ca, int32_t cb, int32_t g1, const double* x1, int32_t g2, const double* x2,
                 int64_t ns, const double* others, const int32_t* use, const double* z, const double* var_extra,
                 int32_t maxno, double cm, double* imp_out, int64_t* below_out) {
  if (!h) return GPE_ERR_ARG;
  h->err.clear();
  const int p = h->outputs;
  if (p == 0) return hm_fail(h, GPE_ERR_STATE, "the set is empty (call gpe_hm_add)");
  const HmMesh m{D, ca, cb, g1, g2, x1, x2, others, ns};
  if (int rc = hm_mesh_check(h, m, imp_out, below_out)) return rc;
  if (!z || !var_extra) return hm_fail(h, GPE_ERR_ARG, "bad hm_cells args (z and var_extra not NULL)");
  if (maxno < 1 || maxno > p) return hm_fail(h, GPE_ERR_ARG, "maxno must be in [1, outputs of the set]");
  for (const HmEmul& e : h->em)
    if (D <= e.maxact) return hm_fail(h, GPE_ERR_ARG, "D is smaller than an emulator's largest active index + 1");
  // a member's flag is its first output's, for all its outputs
  unsigned mask = 0;
  for (const HmEmul& e : h->em)
    if (!use || use[e.first])
      for (int j = 0; j < e.outputs(); ++j) mask |= 1u << (e.first + j);
  double* dextra = nullptr;
  return hm_cells_run(h, m, p, (int)maxno, mask, cm, 0, nullptr, &dextra, imp_out, below_out,
                      [&](const double* dX, double* dI2, long long cl, long long mc) {
                        return hm_post_all(h, dX, D, mc, cl, z, var_extra, mask, dI2, nullptr);
                      });
}

int gpe_hm_cells_mv(gpe_hm* h, int32_t member, int32_t D, int32_t ca, int32_t cb, int32_t g1, const double* x1,
                    int32_t g2, const double* x2, int64_t ns, const double* others, const double* z, const double* V,
                    double cm, double* imp_out, int64_t* below_out) {
  if (!h) return GPE_ERR_ARG;
  h->err.clear();
  if (h->outputs == 0) return hm_fail(h, GPE_ERR_STATE, "the set is empty (call gpe_hm_add)");
  if (member < 0 || member >= (int)h->em.size() || h->em[member].p == 0)
    return hm_fail(h, GPE_ERR_ARG, "member must be a multi-output member of the set (gpe_hm_add_multi)");
  const HmMesh m{D, ca, cb, g1, g2, x1, x2, others, ns};
  if (int rc = hm_mesh_check(h, m, imp_out, below_out)) return rc;
  if (!z || !V) return hm_fail(h, GPE_ERR_ARG, "bad hm_cells_mv args (z and V not NULL)");
  const HmEmul& e = h->em[member];
  if (D <= e.maxact) return hm_fail(h, GPE_ERR_ARG, "D is smaller than the member's largest active index + 1");
  const int p = e.p;
  std::vector<double> wl((size_t)p * p + p);
  if (hm_mv_prepare(p, e.Sigma.data(), V, wl.data(), wl.data() + (size_t)p * p))
    return hm_fail(h, GPE_NOT_PD, "V is not positive definite");
  double* dW = nullptr;
  return hm_cells_run(h, m, 0, 1, 1u, cm, (long long)wl.size(), wl.data(), &dW, imp_out, below_out,
                      [&](const double* dX, double* dI2, long long cl, long long mc) -> int {
                        HmPostMultiArgs a = {};
                        hm_post_args(e, dX, D, mc, a);
                        hm_multi_args(e, a);
                        a.Wj = dW; a.lam = dW + (size_t)p * p; a.joint = 1;
                        a.i2 = dI2; a.ldo = cl; a.mean = nullptr; a.var = nullptr;
                        for (int j = 0; j < p; ++j) a.zs[j] = z[j];
                        hm_launch_post(e, dim3((unsigned)hm_tiles(mc, e.pt)),
                                       (size_t)hm_lds_doubles(e.n, e.pt) * sizeof(double), h->stream, a);
                        HM_HIPCHK(h, hipGetLastError());
                        return GPE_OK;
                      });
}

int gpe_hm_sample(gpe_hm* h, int32_t D, const double* lo, const double* hi, const uint64_t state[2],
                  const uint64_t inc[2], int64_t first, int64_t m, const double* z, const double* var_extra,
                  int32_t maxno, double cm, int64_t cap, double* pts_out, int64_t* idx_out, int64_t* accepted_out) {
  if (!h) return GPE_ERR_ARG;
  h->err.clear();
  const int p = h->outputs;
  if (p == 0) return hm_fail(h, GPE_ERR_STATE, "the set is empty (call gpe_hm_add)");
  if (m < 1 || first < 0 || cap < 0 || D < 1) return hm_fail(h, GPE_ERR_ARG, "bad hm_sample args (m >= 1, first >= 0, cap >= 0)");
  if (!lo || !hi || !state || !inc || !z || !var_extra || !accepted_out || (cap > 0 && (!pts_out || !idx_out)))
    return hm_fail(h, GPE_ERR_ARG, "bad hm_sample args (a NULL pointer)");
  if (((hm_u128)first + (hm_u128)m) * (hm_u128)D >= (hm_u128)1 << 63)
    return hm_fail(h, GPE_ERR_ARG, "(first + m) D must be below 2^63");
  if (maxno < 1 || maxno > p) return hm_fail(h, GPE_ERR_ARG, "maxno must be in [1, outputs of the set]");
  for (const HmEmul& e : h->em)
    if (D <= e.maxact) return hm_fail(h, GPE_ERR_ARG, "D is smaller than an emulator's largest active index + 1");
  HM_HIPCHK(h, hipSetDevice(h->device));
  const long long CH = h->chunk, cl = std::min<long long>(CH, m), rows = std::min<long long>(cap, m);
  const HmSampleWork w = hm_work_sample(cl, D, p, rows);
  if (int rc = hm_workspace(h, (size_t)w.dev(), 0)) return rc;
  double* dX = h->dwork;
  double* dI2 = dX + w.pts;
  long long* dranks = reinterpret_cast<long long*>(dI2 + w.i2);
  long long* dtotal = dranks + (w.ranks - 1);
  uint64_t* dtable = reinterpret_cast<uint64_t*>(dranks + w.ranks);
  double* dbox = reinterpret_cast<double*>(dtable + w.table);
  double* dpts = dbox + w.box;
  long long* didx = reinterpret_cast<long long*>(dpts + w.out_pts);
  const hm_u128 s128 = hm_u128_of(state[0], state[1]), i128 = hm_u128_of(inc[0], inc[1]);
  const int digits = hm_digits(cl);
  std::vector<uint64_t> table((size_t)w.table);
  hm_jump_table(D, i128, digits, table.data());
  std::vector<double> box((size_t)2 * D);
  for (int k = 0; k < D; ++k) box[k] = lo[k], box[D + k] = hi[k];
  // (every earlier call has ended: blocking copies, once per call)
  HM_HIPCHK(h, hipMemcpy(dtable, table.data(), table.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  HM_HIPCHK(h, hipMemcpy(dbox, box.data(), box.size() * sizeof(double), hipMemcpyHostToDevice));
  HM_HIPCHK(h, hipMemsetAsync(dtotal, 0, sizeof(long long), h->stream));
  const unsigned all = ~0u;
  int rc = GPE_OK;
  for (long long s0 = 0; s0 < m && rc == GPE_OK; s0 += CH) {
    const long long mc = std::min(CH, m - s0);
    const hm_u128 start = hm_pcg_apply(hm_jump((uint64_t)(first + s0) * (uint64_t)D, i128), s128);
    const unsigned nb = (unsigned)hm_acc_blocks(mc);
    hipLaunchKernelGGL(k_hm_draw, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, h->stream, dtable, digits,
                       (uint64_t)(start >> 64), (uint64_t)start, inc[0], inc[1], dbox, (int)D, mc, dX);
    rc = hm_post_all(h, dX, D, mc, cl, z, var_extra, all, dI2, nullptr);
    if (rc != GPE_OK) break;
    const bool few = hm_top_slots(maxno) == HM_TOP_FEW;
    if (few)
      hipLaunchKernelGGL(k_hm_count<HM_TOP_FEW>, dim3(nb), dim3(HM_ACC_BLOCK), 0, h->stream, dI2, cl, p, (int)maxno, cm, mc,
                         dranks);
    else
      hipLaunchKernelGGL(k_hm_count<HM_MAX_EMUL>, dim3(nb), dim3(HM_ACC_BLOCK), 0, h->stream, dI2, cl, p, (int)maxno, cm, mc,
                         dranks);
    hipLaunchKernelGGL(k_hm_ranks, dim3(1), dim3(256), 0, h->stream, dranks, (long long)nb, dtotal);
    if (few)
      hipLaunchKernelGGL(k_hm_scatter<HM_TOP_FEW>, dim3(nb), dim3(HM_ACC_BLOCK), 0, h->stream, dI2, cl, p, (int)maxno, cm,
                         mc, dX, (int)D, (long long)(first + s0), dranks, (long long)rows, dpts, didx);
    else
      hipLaunchKernelGGL(k_hm_scatter<HM_MAX_EMUL>, dim3(nb), dim3(HM_ACC_BLOCK), 0, h->stream, dI2, cl, p, (int)maxno, cm,
                         mc, dX, (int)D, (long long)(first + s0), dranks, (long long)rows, dpts, didx);
    if (hipGetLastError() != hipSuccess) rc = hm_fail(h, GPE_ERR_HIP, "a launch of gpe_hm_sample failed");
  }
  hipError_t e = hipStreamSynchronize(h->stream);
  if (rc != GPE_OK) return rc;
  HM_HIPCHK(h, e);
  long long total = 0;
  HM_HIPCHK(h, hipMemcpy(&total, dtotal, sizeof(long long), hipMemcpyDeviceToHost));
  *accepted_out = total;
  const long long got = std::min(total, rows);
  if (got > 0) {
    HM_HIPCHK(h, hipMemcpy(pts_out, dpts, (size_t)got * D * sizeof(double), hipMemcpyDeviceToHost));
    HM_HIPCHK(h, hipMemcpy(idx_out, didx, (size_t)got * sizeof(long long), hipMemcpyDeviceToHost));
  }
  return GPE_OK;
}

}  // extern "C"
