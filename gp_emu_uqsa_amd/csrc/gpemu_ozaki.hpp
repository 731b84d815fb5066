// gpemu_ozaki.hpp -- A^-1 = X^T X (the LAUUM of the objective's gradient, X = L^-1 lower
// triangular) on the int8 matrix cores, exact integer products reconstructed to fp64 by the
// Chinese remainder theorem (the Ozaki scheme II construction: Ozaki, Uchino, Imamura 2024).
//
// Why: on gfx950 the 32 x 32 x 32 i8 MFMA does 32768 integer multiply-adds per 32 cycles per
// SIMD against 2048 flops per 64 cycles for the 16 x 16 x 4 f64 MFMA: 32 x the fp64 rate per
// clock (measured on random operands, where the chip holds a lower clock: 2.2-2.4 POPS against
// the fp64 GEMM's 70 TF/s, tools/hip/i8_probe.hip).  With N = 16 moduli the product is exact
// and the operands carry 53 bits: the result has fp64 accuracy.
//
// The arithmetic, per column j of X (the rows of both operands of X^T X):
//   e_j     = 52 - ilogb(max_k |X(k,j)|), so X'(k,j) = rint(X(k,j) 2^e_j) is an integer with
//             |X'| <= 2^53 (beta bits: 53 with 16 moduli for every n_pad up to 131072, fewer
//             with fewer moduli: oz_consts on the host, checked by tests/host/oz_plan_check.cpp);
//   C'(i,j) = sum_k X'(k,i) X'(k,j), exact, |C'| <= n 2^(2 beta) < M / 2 (M = prod m_l);
//   for each modulus m_l (pairwise coprime, <= 256): X'_l = X' mod m_l in [-128, 127]
//             (int8), C'_l = X'_l^T X'_l on the i8 MFMA (int32, exact: |.| <= n 2^14 < 2^31),
//             c_l = C'_l mod m_l (centred, stored as one byte);
//   C'/M    = sum_l c_l y_l / m_l  (mod 1), y_l = (M / m_l)^-1 mod m_l: the centred fraction
//             v of that sum, formed exactly on a 2^-41 grid (hi parts) plus the lo parts,
//             gives C' = v M and A^-1(i,j) = v M 2^-(e_i + e_j).
// Kernels: k_oz_colexp (e_j), k_oz_split (X -> N int8 planes, lower 256-column panels),
// k_oz_gemm (grouped over moduli: 256 x 256 tiles of the lower triangle, K from the tile
// row's diagonal block), k_oz_crt (N residue bytes per element -> fp64, lower 128-tiles).
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

namespace gpe {

constexpr int OZ_T = 256;                  // output tile, and the planes' column panels
constexpr int OZ_SK = 64;                  // k (bytes) per LDS stage: two 32-deep k-steps
constexpr int OZ_NBUF = 4;                 // stage ring (stage s + 4 is issued from stage s's barrier on)
constexpr int OZ_OPND = OZ_T * OZ_SK;      // one operand's stage image (16 KB)
constexpr int OZ_LDS = OZ_NBUF * 2 * OZ_OPND;   // 128 KB: one workgroup per CU
constexpr int OZ_MAXMOD = 16;
// longest sum of a product: the int32 accumulators hold K 2^14 < 2^31 and k_oz_gemm's epilogue
// reduces them exactly in fp32 (|t| < 2^23, see there) for K up to this
constexpr int OZ_MAX_K = (1 << 17) - 128;

// moduli (pairwise coprime; the odd ones <= 253 so a rounded centred residue stays in int8)
// and the reconstruction constants (host: oz_consts)
struct OzConst {
  int m[OZ_MAXMOD];        // modulus
  int c16[OZ_MAXMOD];      // 2^16 mod m
  float inv[OZ_MAXMOD];    // 1 / m
  int wlo[OZ_MAXMOD];      // centred 256^i mod m as int8, i = 0 .. 3 from the low byte (oz_residues)
  int whi[OZ_MAXMOD];      // i = 4 .. 6, the top byte 0
  double rhi[OZ_MAXMOD];   // y / m rounded to a multiple of 2^-41 (y = (M / m)^-1 mod m)
  double rlo[OZ_MAXMOD];   // y / m - rhi
  double Md;               // M = prod m (rounded)
  double Mlo;              // 0, or (oz_consts_cert) what Md lacks: the scale is Md + Mlo
  int nmod;
  int beta;                // operand bits
};

typedef int oz_v4i __attribute__((ext_vector_type(4)));
typedef int oz_v16i __attribute__((ext_vector_type(16)));

// A row (or column) holding a NaN or an infinity gets the exponent OZ_EX_NAN: its planes are
// zero and every product entry in its row (column) comes out NaN, as an fp64 GEMM's would
// (k_oz_il_to_ex: an atomically max-ed OZ_IL_BAD)
constexpr int OZ_EX_NAN = -(1 << 20), OZ_IL_BAD = 1 << 29;
// max that keeps a NaN of either side
__device__ __forceinline__ double oz_pmax(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ int oz_ex_of(double mx, int beta) {
  return !(mx <= 1.7976931348623157e308) ? OZ_EX_NAN : (mx > 0.0 ? (beta - 1) - ilogb(mx) : 0);
}

// byte offset of column-panel cb in the planes: panel cb holds columns [256 cb, 256 cb + 256),
// rows [256 cb, np2), column-major with ld np2 - 256 cb
__host__ __device__ __forceinline__ long long oz_panel_off(int cb, int np2) {
  return (long long)OZ_T * ((long long)cb * np2 - (long long)OZ_T * cb * (cb - 1) / 2);
}
__host__ __device__ __forceinline__ long long oz_plane_bytes(int np2) { return oz_panel_off(np2 / OZ_T, np2); }

// ---- an operand entry -> its residue bytes (k_oz_split, k_oz_split_rect; compiled for the
// host too: tests/host/oz_residue_check.cpp holds it against 128-bit integers).
// x = rint(ldexp(., e)) is an integer-valued double, |x| <= 2^53.  Once per entry:
//   X = (long long)x = sum_i d_i 256^i, seven balanced digits d_i in [-128, 127]: byte i of
//       (X + c) ^ c, c = 0x0080808080808080 (one addition puts 128 on every digit and carries;
//       the eighth digit would be 0 for -c <= X < 2^56 - c).
// Per modulus:
//   t = sum_i d_i w_i, w_i the centred 256^i mod m (OzConst::wlo, whi; (1, 0, ..) for 256):
//       t = X (mod m), |t| <= 7 128 128 < 2^17, two 4 x int8 dot products;
//   r = t - m rint(t / m), the tile end's reduction (oz_store_residues: q from fl(t (1 / m)) +
//       1.5 2^23, two roundings, then a 24-bit multiply-add; only the low byte is kept).
//       |fl(t (1 / m)) - t / m| <= 2^-23 |t| / m < 1e-4, and for odd m t / m is at least
//       1 / (2 m) > 1.9e-3 from a tie: q is exact and r the one centred residue,
//       |r| <= (m - 1) / 2.  For m = 256 (1 / m exact) q may go either way at a tie, and
//       r = t (mod 256) regardless: the low byte of t.
struct OzDigits {
  int lo, hi;   // d_0 .. d_3 and d_4 .. d_6 (top byte 0), as packed int8
};
__host__ __device__ __forceinline__ OzDigits oz_digits(double x) {
  const unsigned long long c = 0x0080808080808080ull;
  const unsigned long long b = ((unsigned long long)(long long)x + c) ^ c;
  return OzDigits{(int)(unsigned)b, (int)(unsigned)(b >> 32)};
}
// c + sum of the four int8 products of a's and b's bytes
__host__ __device__ __forceinline__ int oz_dot4(int a, int b, int c) {
#if __HIP_DEVICE_COMPILE__
  return __builtin_amdgcn_sdot4(a, b, c, false);
#else
  for (int i = 0; i < 4; ++i) c += (int)(int8_t)((unsigned)a >> (8 * i)) * (int)(int8_t)((unsigned)b >> (8 * i));
  return c;
#endif
}
// the product of the low 24 bits (signed) of a and b, its low 32 bits
__host__ __device__ __forceinline__ int oz_mul24(int a, int b) {
#if __HIP_DEVICE_COMPILE__
  return __mul24(a, b);
#else
  const int a24 = (int)((unsigned)a << 8) >> 8, b24 = (int)((unsigned)b << 8) >> 8;
  return (int)((unsigned)a24 * (unsigned)b24);
#endif
}
__host__ __device__ __forceinline__ int oz_float_bits(float f) {
#if __HIP_DEVICE_COMPILE__
  return __float_as_int(f);
#else
  int i;
  std::memcpy(&i, &f, sizeof i);
  return i;
#endif
}
__host__ __device__ __forceinline__ int oz_digit_sum(OzDigits d, int wlo, int whi) {   // t
  return oz_dot4(d.lo, wlo, oz_dot4(d.hi, whi, 0));
}
// the centred residue of t modulo m = -nm in the low byte (the rest is not the residue's)
__host__ __device__ __forceinline__ unsigned oz_reduce(int t, float inv, int nm) {
#pragma clang fp contract(off)
  const float qf = (float)t * inv + 12582912.0f;
  return (unsigned)(oz_mul24(oz_float_bits(qf), nm) + t);
}
// the low bytes of v0 .. v3, lowest first
__host__ __device__ __forceinline__ unsigned oz_pack4(unsigned v0, unsigned v1, unsigned v2, unsigned v3) {
#if __HIP_DEVICE_COMPILE__
  return __builtin_amdgcn_perm(__builtin_amdgcn_perm(v3, v2, 0x0c0c0400u), __builtin_amdgcn_perm(v1, v0, 0x0c0c0400u),
                               0x05040100u);
#else
  return (v0 & 0xffu) | (v1 & 0xffu) << 8 | (v2 & 0xffu) << 16 | v3 << 24;
#endif
}
// the residues of x modulo cst's moduli, one int8 each
__host__ __device__ inline void oz_residues(double x, const OzConst& cst, int8_t* out) {
  const OzDigits d = oz_digits(x);
  for (int l = 0; l < cst.nmod; ++l)
    out[l] = (int8_t)(oz_reduce(oz_digit_sum(d, cst.wlo[l], cst.whi[l]), cst.inv[l], -cst.m[l]) & 0xffu);
}
// the same for 8 entries (their digits) and modulus number l: two words, entry 0 in the lowest byte
__host__ __device__ __forceinline__ uint2 oz_residues8(const OzDigits (&d)[8], const OzConst& cst, int l) {
  const int wlo = cst.wlo[l], whi = cst.whi[l], nm = -cst.m[l];
  const float inv = cst.inv[l];
  unsigned v[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) v[u] = oz_reduce(oz_digit_sum(d[u], wlo, whi), inv, nm);
  return make_uint2(oz_pack4(v[0], v[1], v[2], v[3]), oz_pack4(v[4], v[5], v[6], v[7]));
}

// ---- the certificate: a product whose operands' rows are short in the 2-norm is exact on the
// first 15 moduli (191 dropped), with the operands still at 53 bits.  The data-independent bound
// |C'| <= K 2^(2 beta) puts every entry of both rows at the row maximum; Cauchy-Schwarz needs
// the rows' 2-norms only.  Per operand row r the split kernels sum, in integers,
//   s_r = sum_k y_k^2,  y = (|x'| >> 32) + 1  (x' = rint(ldexp(x, e)), |x'| <= 2^53),
// so |x'| <= 2^32 y and ||a'_r||_2 <= 2^32 sqrt(s_r); s_r < 2^17 (2^21 + 1)^2 < 2^60 for
// K <= OZ_MAX_K: no overflow.  With A = max_r s_a, B = max_r s_b and any k range,
//   |C'_ij| <= ||a'_i|| ||b'_j|| <= 2^64 sqrt(A B) < M15 / 2  iff  A B < M15^2 / 2^130,
// M15 the product of the first 15 moduli of oz_consts: A B < T15 = floor(M15^2 / 2^130) =
// 34409203667017820043519436844158 ~ 2^104.76 (A B is an integer).  Then C' is its own centred
// residue modulo M15 and k_oz_crt reconstructs it from 15 residues (oz_consts_cert).  Integer
// sums are the same in any order, so the decision is the same from run to run.  Zero, masked
// and padded entries may add their y = 1 or nothing: the bound holds either way.  Checked on the
// host against 128-bit integers: tests/host/oz_cert_check.cpp.
constexpr int OZ_CERT_NMOD = OZ_MAXMOD - 1;
constexpr unsigned long long OZ_T15_HI = 0x1b24e222aafull, OZ_T15_LO = 0xd866408f6fe8ec7eull;   // T15 = HI 2^64 + LO
// y^2 of an integer-valued x', |x'| <= 2^53 (the scaling is exact and the conversion truncates)
__host__ __device__ __forceinline__ unsigned long long oz_cert_term(double xr) {
  const unsigned y = (unsigned)(fabs(xr) * 0x1p-32) + 1u;
  return (unsigned long long)y * y;
}
// A B < T15, the 128-bit product from 32-bit halves
__host__ __device__ inline bool oz_cert_ok(unsigned long long A, unsigned long long B) {
  const unsigned long long a0 = A & 0xffffffffull, a1 = A >> 32, b0 = B & 0xffffffffull, b1 = B >> 32;
  const unsigned long long p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const unsigned long long mid = (p00 >> 32) + (p01 & 0xffffffffull) + (p10 & 0xffffffffull);
  const unsigned long long lo = (p00 & 0xffffffffull) | (mid << 32);
  const unsigned long long hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
  return hi < OZ_T15_HI || (hi == OZ_T15_HI && lo < OZ_T15_LO);
}
// a workgroup's partial row sum into sum[r]: v summed over the workgroup's 256 threads (every
// thread of the workgroup calls this), one atomic if anything was added
__device__ __forceinline__ void oz_cert_block_add(unsigned long long v, unsigned long long* __restrict__ sum, int r) {
  __shared__ unsigned long long part[4];
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    v = part[0] + part[1] + part[2] + part[3];
    if (v) atomicAdd(sum + r, v);
  }
}
// One workgroup: the flag of a product from its operands' row sums (na rows of sa, nb of sb);
// mx (or null): the two maxima A and B for a read-back (gpe_oz_cert_sums)
static __global__ void __launch_bounds__(256) k_oz_cert(const unsigned long long* __restrict__ sa, int na,
                                                        const unsigned long long* __restrict__ sb, int nb,
                                                        int* __restrict__ flag, unsigned long long* __restrict__ mx) {
  __shared__ unsigned long long pa[4], pb[4];
  unsigned long long A = 0, B = 0;
  for (int r = threadIdx.x; r < na; r += 256) A = sa[r] > A ? sa[r] : A;
  for (int r = threadIdx.x; r < nb; r += 256) B = sb[r] > B ? sb[r] : B;
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long oa = __shfl_xor(A, off, 64), ob = __shfl_xor(B, off, 64);
    A = oa > A ? oa : A;
    B = ob > B ? ob : B;
  }
  if ((threadIdx.x & 63) == 0) {
    pa[threadIdx.x >> 6] = A;
    pb[threadIdx.x >> 6] = B;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      A = pa[w] > A ? pa[w] : A;
      B = pb[w] > B ? pb[w] : B;
    }
    *flag = oz_cert_ok(A, B) ? 1 : 0;
    if (mx) {
      mx[0] = A;
      mx[1] = B;
    }
  }
}

// e_j for every column j < np2 (one wave per column, rows k >= j; columns past np: 0); sum (the
// certificate's row sums, or null): zeroed where the exponent is written
static __global__ void __launch_bounds__(256) k_oz_colexp(const double* __restrict__ X, long long ldx, int np,
                                                          int np2, int beta, int* __restrict__ ex,
                                                          unsigned long long* __restrict__ sum) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= np2) return;
  double mx = 0.0;
  if (j < np)
    for (int k = j + lane; k < np; k += 64) mx = oz_pmax(mx, fabs(X[k + (long long)j * ldx]));
  for (int off = 32; off > 0; off >>= 1) mx = oz_pmax(mx, __shfl_xor(mx, off, 64));
  if (lane == 0) {
    ex[j] = oz_ex_of(mx, beta);
    if (sum) sum[j] = 0ull;
  }
}

// X -> the N int8 planes: thread = 8 consecutive rows of one column (a wave reads 4 KB of
// the column and writes 512 contiguous bytes per plane); entries above the diagonal (and past
// np) are zero, and a thread whose 8 rows are all such writes its zeros and nothing else; the
// residues by oz_residues8.  Precondition: X is 16-byte aligned and ldx even (every column starts on a
// 16-byte boundary: the double2 loads below; the callers' ldx is n_pad, a multiple of 128).
// Entries above the diagonal are never read.  oz_split_thread: one thread's 8 rows of column j;
// with CERT it returns their share of the column's certificate sum (0 where it stored zeros
// alone).  sum (or null): the workgroup's share goes to sum[j], one atomic per workgroup.
constexpr int OZ_SPLIT_ROWS = 8;
template <bool CERT>
__device__ __forceinline__ unsigned long long oz_split_thread(const double* __restrict__ X, long long ldx, int np, int np2,
                                                              const int* __restrict__ ex, int8_t* __restrict__ planes,
                                                              long long plane_bytes, const OzConst& cst, int j) {
  const int cb = j / OZ_T, r0 = cb * OZ_T;
  const int k0 = r0 + OZ_SPLIT_ROWS * ((int)blockIdx.y * 256 + (int)threadIdx.x);
  if (k0 >= np2) return 0ull;
  const int e = ex[j];
  const long long ld = np2 - r0;
  int8_t* dst = planes + oz_panel_off(cb, np2) + (long long)(j - r0) * ld + (k0 - r0);
  if (j >= np || k0 >= np || k0 + OZ_SPLIT_ROWS <= j || e == OZ_EX_NAN) {   // all 8 zero: the stores alone
    for (int l = 0; l < cst.nmod; ++l) *reinterpret_cast<uint2*>(dst + (long long)l * plane_bytes) = make_uint2(0u, 0u);
    return 0ull;
  }
  double xs[OZ_SPLIT_ROWS];
  if (k0 + OZ_SPLIT_ROWS <= np && k0 >= j) {   // (16-byte loads: k0 is a multiple of 8)
#pragma unroll
    for (int u = 0; u < OZ_SPLIT_ROWS; u += 2) {
      const double2 v = *reinterpret_cast<const double2*>(X + k0 + u + (long long)j * ldx);
      xs[u] = v.x;
      xs[u + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int u = 0; u < OZ_SPLIT_ROWS; ++u) {
      const int k = k0 + u;
      xs[u] = (k >= j && k < np) ? X[k + (long long)j * ldx] : 0.0;
    }
  }
  OzDigits d[OZ_SPLIT_ROWS];
  unsigned long long s = 0ull;
#pragma unroll
  for (int u = 0; u < OZ_SPLIT_ROWS; ++u) {
    const double xr = rint(ldexp(xs[u], e));   // |.| <= 2^beta
    d[u] = oz_digits(xr);
    if constexpr (CERT) s += oz_cert_term(xr);
  }
  for (int l = 0; l < cst.nmod; ++l) *reinterpret_cast<uint2*>(dst + (long long)l * plane_bytes) = oz_residues8(d, cst, l);
  return s;
}
static __global__ void __launch_bounds__(256) k_oz_split(const double* __restrict__ X, long long ldx, int np,
                                                         int np2, const int* __restrict__ ex, int8_t* __restrict__ planes,
                                                         long long plane_bytes, OzConst cst,
                                                         unsigned long long* __restrict__ sum) {
  const int j = blockIdx.x;
  if (sum) oz_cert_block_add(oz_split_thread<true>(X, ldx, np, np2, ex, planes, plane_bytes, cst, j), sum, j);
  else oz_split_thread<false>(X, ldx, np, np2, ex, planes, plane_bytes, cst, j);
}

__device__ __forceinline__ void oz_glds16(const int8_t* src, int8_t* dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}
// p, the same in every lane, held in scalar registers: what is added to it per stage is then
// scalar arithmetic, and a load's address one vector add of the lane's offset
__device__ __forceinline__ const int8_t* oz_uniform(const int8_t* p) {
  const unsigned long long u = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  return (const int8_t*)(((unsigned long long)hi << 32) | lo);
}
template <int N> __device__ __forceinline__ void oz_vmwait() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

// One operand of a product, as int8 planes (one per modulus, plane_bytes apart): row r of
// 256-row tile t at depth k is
//   packed (the LAUUM's lower column panels of X): oz_panel_off(t, np2) + r (np2 - 256 t) + k - 256 t
//   rectangular: (256 t + r) ld + k
struct OzOpnd {
  const int8_t* p;
  long long plane_bytes;
  long long ld;    // rectangular row pitch (bytes); 0: packed
  int np2;         // packed: the padded order
};
__device__ __forceinline__ const int8_t* oz_tile_rows(const OzOpnd& o, int t, int k, long long& ld) {
  if (o.ld == 0) {
    ld = o.np2 - OZ_T * t;
    return o.p + oz_panel_off(t, o.np2) + (k - OZ_T * t);
  }
  ld = o.ld;
  return o.p + (long long)OZ_T * t * o.ld + k;
}

// A product C'_l = A'_l B'_l^T over the 256 x 256 tiles of a list (entries ti << 16 | tj, the
// list's length a multiple of 8 so position % 8 is the XCD under round-robin dispatch,
// 0xffffffff padding the bins), blockIdx.x = l * list_len + position.  K range of tile
// (ti, tj): from 0, 256 ti, 256 tj or 128 floor(2 ti / kdiv) (kbeg 0 / 1 / 2 / 3) to K or
// 256 (ti + 1) (kend 0 / 1): the triangular operands' nonzero k (kbeg 3: the rows of a
// lower-triangular X dealt cyclically by 128-row tiles over kdiv ranks, seen from one rank).
// Tile rows from ti0 (the residues of tile (ti, tj) at its index less that of (ti0, 0)).
// Preconditions: every k range a multiple of 64 long (K and the range starts are multiples of
// 128 or 256 at every call site; a remainder would be dropped without a word: the test hook
// gpe_test_oz_product refuses such a K), K <= OZ_MAX_K, and the operands zero on the k a
// range skips.  One product at a time against exact integers: tests/test_gpu_oz_product.py.
struct OzGemm {
  OzOpnd a, b;
  const unsigned* list;
  int list_len;
  int K, kbeg, kend;
  int tri, ntj;    // residue tile of (ti, tj): oz_res_tile
  int8_t* res;
  long long res_bytes;
  int kdiv = 1;
  int ti0 = 0;
  // the certificate's flag (k_oz_cert), or null: where it is set, modulus OZ_CERT_NMOD's
  // workgroups (the grid's last list_len) have nothing to do
  const int* flag = nullptr;
};
// residue tile of (ti, tj): ti ntj + tj, or (tri) ti (ti + 1) / 2 + tj over the lower triangle;
// tri with ntj > 0: the lower triangle capped at ntj tile columns (tj <= min(ti, ntj - 1)), the
// rows from ntj on ntj tiles each
__host__ __device__ __forceinline__ long long oz_res_tile(int tri, int ntj, int ti, int tj) {
  if (!tri) return (long long)ti * ntj + tj;
  if (ntj > 0 && ti >= ntj) return (long long)ntj * (ntj + 1) / 2 + (long long)(ti - ntj) * ntj + tj;
  return (long long)ti * (ti + 1) / 2 + tj;
}
// the k range [kb, ke) of tile (ti, tj) (above): the one statement of the rule, for k_oz_gemm
// and for the host's tile weights and operation counts (OzShape::klen)
__host__ __device__ __forceinline__ void oz_k_range(int kbeg, int kend, int kdiv, int K, int ti, int tj, int& kb, int& ke) {
  kb = kbeg == 1 ? OZ_T * ti : (kbeg == 2 ? OZ_T * tj : (kbeg == 3 ? 128 * ((2 * ti) / kdiv) : 0));
  ke = kend == 1 ? (K < OZ_T * (ti + 1) ? K : OZ_T * (ti + 1)) : K;
}

// wait until at most `stages` whole stages (8 direct loads each) of this wave are in flight
__device__ __forceinline__ void oz_vmwait_stages(int stages) {
  static_assert(OZ_NBUF <= 5, "one case per stage that can be in flight");
  if (stages >= 4) oz_vmwait<32>();
  else if (stages == 3) oz_vmwait<24>();
  else if (stages == 2) oz_vmwait<16>();
  else if (stages == 1) oz_vmwait<8>();
  else oz_vmwait<0>();
}

// The tile end: the centred residue of each of a lane's 256 accumulators as one byte, 16 bytes
// per MFMA block in the block's own order.  Only the low byte of a result is kept, so every
// step needs to be right modulo 256 only, except the quotient q:
//   t = (a >> 16) (2^16 mod m) + (a & 0xffff) = a + (a >> 16) (c16 - 2^16): one 24-bit
//       multiply-add (|a >> 16| <= K / 4 < 2^15 and |c16 - 2^16| <= 2^16; |t| < 2^23 for
//       K <= OZ_MAX_K < 2^17: |a| <= K 2^14, so |a >> 16| (2^16 mod m) <= (K / 4) 252, plus 2^16),
//       so t is exact in fp32;
//   q = rint(t / m) to within 3e-4, as p = fl(t (1 / m)) rounded to an integer by adding
//       1.5 2^23: |p| < 2^22, so the sum lies in [2^23, 2^24) where fp32 numbers are the
//       integers and the addition itself rounds p to nearest, ties to even (the constant is
//       even, so the tie goes where rintf(p) puts it: the same q, bit for bit).  The sum's low
//       24 bits are 2^22 + q.  The product and the sum are two roundings: no contraction here;
//   r = t - q m in [-m/2 - 1, m/2 + 1], formed as t + (2^22 + q)(-m) by a second 24-bit
//       multiply-add: off by 2^22 m, a multiple of 256.
// M256: m = 256, the low byte of a itself.
template <bool M256>
__device__ __forceinline__ void oz_store_residues(const oz_v16i (&acc)[4][4], int m, int c16, float inv, int8_t* out) {
#pragma clang fp contract(off)
  const int cm = c16 - 65536, nm = -m;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int a = acc[i][j][r];
        if constexpr (M256) {
          v[r] = (unsigned)a;
        } else {
          const int t = __mul24(a >> 16, cm) + a;
          const float qf = (float)t * inv + 12582912.0f;
          v[r] = (unsigned)(__mul24(__float_as_int(qf), nm) + t);
        }
      }
      oz_v4i w;
#pragma unroll
      for (int u = 0; u < 4; ++u) {   // bytes 0 of v[4 u .. 4 u + 3], lowest first
        const unsigned lo = __builtin_amdgcn_perm(v[4 * u + 1], v[4 * u], 0x0c0c0400u);
        const unsigned hi = __builtin_amdgcn_perm(v[4 * u + 3], v[4 * u + 2], 0x0c0c0400u);
        w[u] = (int)__builtin_amdgcn_perm(hi, lo, 0x05040100u);
      }
      *reinterpret_cast<oz_v4i*>(out + (long long)(4 * i + j) * 64 * 16) = w;
    }
}

// 4 waves of 128 x 128 (4 x 4 blocks of the 32 x 32 x 32 i8 MFMA, operands swapped so lane &
// 31 runs along the tile's rows); stages of 64 k (two 32-deep k-steps) through a 4-deep LDS
// ring filled by direct global -> LDS loads.  The stage image of each operand is [row][64 B]
// with granule g of row r at slot g ^ ((r >> 2) & 3): conflict-free for ds_read_b128's lane
// groups.  Steady state, stage s in buffer s % 4, nothing but the barrier between two MFMAs:
//   k-step 0: 16 MFMAs; a fragment read of (s, k-step 1) behind each of the first 8, a direct
//             load of stage s + 3 (its second half) behind every other one of the last 8;
//   boundary: vmcnt(16) (this wave's loads of stage s + 1 have landed; s + 2 and s + 3 stay
//             in flight), lgkmcnt(0), s_barrier: every wave is done reading buffer s % 4 and
//             stage s + 1 is whole;
//   k-step 1: 16 MFMAs; the reads of (s + 1, k-step 0) behind the first 8, the first half of
//             the loads of stage s + 4, into buffer s % 4, behind the last 8.
// So a k-step's reads have 8 MFMAs to land before the next k-step needs them, and no k-step
// carries more than one direct load per four MFMAs.  The last 4 stages (and a tile shorter than
// the ring) run the same step without the loads that no longer exist and with the count of what
// is still in flight (tests/test_gpu_oz_pipeline.py).  Output: the centred residue of every entry, one
// byte, in the MFMA's own order (lane l of block b of wave w: 16 bytes at ((w 16 + b) 64 + l)
// 16 of the tile's 64 KB).  Precondition besides OzGemm's: 256 rows of an operand span less
// than 2^32 bytes (ld < 2^24: every call site's is a padded order or K, at most 2^17).
static __global__ void __launch_bounds__(256, 1) k_oz_gemm(OzGemm g, OzConst cst) {
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  int8_t* lds = reinterpret_cast<int8_t*>(lds_d);
  const int l = (int)blockIdx.x / g.list_len;
  if (l == OZ_CERT_NMOD && g.flag && *g.flag) return;   // certified: 15 moduli carry the product
  const unsigned ent = g.list[(int)blockIdx.x - l * g.list_len];
  if (ent == 0xffffffffu) return;
  const int ti = (int)(ent >> 16), tj = (int)(ent & 0xffffu);
  int kb, ke;
  oz_k_range(g.kbeg, g.kend, g.kdiv, g.K, ti, tj, kb, ke);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = (wave >> 1) * 128, wn = (wave & 1) * 128;
  OzOpnd oa = g.a, ob = g.b;
  oa.p += (long long)l * oa.plane_bytes;
  ob.p += (long long)l * ob.plane_bytes;
  long long lda, ldb;
  const int kp = (lane & 3) ^ ((lane >> 4) & 3);
  // a direct load's source: the tile's first row at the stage's k (the same for every lane, so
  // it advances in scalar registers) plus this lane's 32-bit offset, fixed for the tile
  const int8_t* ua = oz_tile_rows(oa, ti, kb, lda);
  const int8_t* ub = oz_tile_rows(ob, tj, kb, ldb);
  unsigned va[4], vb[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const unsigned row = (unsigned)(16 * wave + (lane >> 2) + 64 * p);
    va[p] = row * (unsigned)lda + 16u * (unsigned)kp;
    vb[p] = row * (unsigned)ldb + 16u * (unsigned)kp;
  }
  // load u of stage s: 16 rows of A (u even) or B (u odd), rows 16 w .. 16 w + 15 with w the
  // wave-instruction index wave + 4 (u / 2)
  auto load1 = [&](int s, int u) {
    int8_t* dst = lds + ((unsigned)s % OZ_NBUF) * 2 * OZ_OPND + (u & 1) * OZ_OPND + 16 * (wave + 4 * (u >> 1)) * OZ_SK;
    const int8_t* src = oz_uniform(((u & 1) ? ub : ua) + (long long)s * OZ_SK);
    oz_glds16(src + ((u & 1) ? vb[u >> 1] : va[u >> 1]), dst);
  };
  oz_v16i acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = oz_v16i{};
  const int ns = max(0, ke - kb) / OZ_SK;
  const int r32 = lane & 31, h = lane >> 5, sw = (r32 >> 2) & 3;
  // fragment u of k-step ks of stage s: A's (u < 4) or B's
  auto frag1 = [&](int s, int ks, int u, oz_v4i (&af)[4], oz_v4i (&bf)[4]) {
    const int8_t* As = lds + ((unsigned)s % OZ_NBUF) * 2 * OZ_OPND;
    const int8_t* Bs = As + OZ_OPND;
    const int slot = ((2 * ks + h) ^ sw) * 16;
    if (u < 4) af[u] = *reinterpret_cast<const oz_v4i*>(As + (wm + 32 * u + r32) * OZ_SK + slot);
    else bf[u - 4] = *reinterpret_cast<const oz_v4i*>(Bs + (wn + 32 * (u - 4) + r32) * OZ_SK + slot);
  };
  auto frags = [&](int s, int ks, oz_v4i (&af)[4], oz_v4i (&bf)[4]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) frag1(s, ks, u, af, bf);
  };
  auto mfmas = [&](const oz_v4i (&af)[4], const oz_v4i (&bf)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(bf[j], af[i], acc[i][j], 0, 0, 0);
  };
  if (ns > 0) {
    oz_v4i ca[4], cb[4], na[4], nb[4];
    // One k-step: the 16 MFMAs on (xa, xb); with READ, the 8 fragment reads of k-step rks of
    // stage rs into (ya, yb), one behind each of the first 8 MFMAs (an MFMA leaves the wave's
    // issue free for most of its 32 cycles, and the reads have the last 8 MFMAs to land); with
    // LOAD, the direct loads u0 .. u0 + 3 of stage ls, one behind every other of the last 8.
    auto kstep = [&](const oz_v4i (&xa)[4], const oz_v4i (&xb)[4], auto READ, int rs, int rks, oz_v4i (&ya)[4],
                     oz_v4i (&yb)[4], auto LOAD, int ls, int u0) {
      mfmas(xa, xb);
      if constexpr (decltype(READ)::value) {
        frags(rs, rks, ya, yb);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // one MFMA
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // one LDS read
        }
      } else {
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
      }
      if constexpr (decltype(LOAD)::value) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          load1(ls, u0 + u);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // one direct load
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        }
      } else {
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    // One stage, s in buffer s % OZ_NBUF.  Its first k-step carries the second half of the
    // loads of stage s + OZ_NBUF - 1 (LOADA: that stage exists and the ring is full), its second
    // k-step the first half of those of stage s + OZ_NBUF (LOADB): one direct load per four
    // MFMAs throughout.  Between the two, if stage s + 1 exists (NEXT), the one barrier.
    // Hazards: loads go into buffer s % OZ_NBUF only after the barrier of stage s, which every
    // wave passes with its reads of stage s retired (lgkmcnt(0)); stage s + 1 is read after
    // that same barrier, which every wave passes with its own loads of stage s + 1 landed.
    // Loads retire in order, so the count is that of the loads issued after them: the stages
    // up to s + OZ_NBUF - 1, or to the tile's last.
    auto step = [&](int s, auto NEXT, auto LOADA, auto LOADB) {
      kstep(ca, cb, std::true_type{}, s, 1, na, nb, LOADA, s + OZ_NBUF - 1, 4);
      if constexpr (decltype(NEXT)::value) {
        if constexpr (decltype(LOADB)::value) oz_vmwait<8 * (OZ_NBUF - 2)>();
        else oz_vmwait_stages(ns - s - 2);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
      }
      kstep(na, nb, NEXT, s + 1, 0, ca, cb, LOADB, s + OZ_NBUF, 0);
    };
    constexpr std::true_type Y{};
    constexpr std::false_type N{};
    // prologue: a tile shorter than the ring whole; else the ring less the second half of its
    // last stage, which the first step brings (20 loads may stay in flight behind stage 0)
    if (ns < OZ_NBUF) {
      for (int s = 0; s < ns; ++s)
#pragma unroll
        for (int u = 0; u < 8; ++u) load1(s, u);
      oz_vmwait_stages(ns - 1);
    } else {
#pragma unroll
      for (int s = 0; s < OZ_NBUF; ++s)
#pragma unroll
        for (int u = 0; u < (s == OZ_NBUF - 1 ? 4 : 8); ++u) load1(s, u);
      oz_vmwait<8 * (OZ_NBUF - 2) + 4>();
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    frags(0, 0, ca, cb);
    int s = 0;
    for (; s + OZ_NBUF < ns; ++s) step(s, Y, Y, Y);
    if (ns >= OZ_NBUF) step(s++, Y, Y, N);   // (OZ_NBUF >= 2: stage s + 1 exists)
    for (; s + 1 < ns; ++s) step(s, Y, N, N);
    if (s < ns) step(s, N, N, N);
  }
  const int m = cst.m[l];
  int8_t* out = g.res + (long long)l * g.res_bytes +
                (oz_res_tile(g.tri, g.ntj, ti, tj) - oz_res_tile(g.tri, g.ntj, g.ti0, 0)) * (OZ_T * OZ_T) +
                ((long long)(wave * 16) * 64 + lane) * 16;
  if (m == 256) oz_store_residues<true>(acc, m, 0, 0.0f, out);
  else oz_store_residues<false>(acc, m, cst.c16[l], cst.inv[l], out);
}

// fp64 entries from the residues: C(r, c) = alpha v M 2^-(exr[r] + exc[c]), v = C'/M the
// centred fraction of sum_l c_l y_l / m_l.  Thread u of tile t (16 workgroups per tile) =
// wave u / 1024, block (u / 64) % 16, lane u % 64 of k_oz_gemm's order, 16 entries; rows
// < rows and columns < cols only, and with lower128 only the lower 128-tiles.  Tile rows
// from ti0 (as OzGemm); row gm of the product goes to row gm - 256 ti0 of C.  acc: the entry
// is added to C's (C = C + alpha ..., one rounding, written once) instead of replacing it.
struct OzCrt {
  const int8_t* res;
  long long res_bytes;
  int tri, ntj;
  const int* exr;
  const int* exc;
  double* C;
  long long ldc;
  int rows, cols, lower128;
  double alpha;
  int ti0 = 0;
  int acc = 0;
};
// A thread's loads -- its 16 residue bytes of every modulus (16 bytes each), its row exponent and
// its 16 column exponents (columns gn0 + 8 q + {0 .. 3}: four 16-byte loads) -- are all issued
// before the first is used, so a wave has nmod + 5 loads (nmod KB of residues) in flight, not
// one: the sums wait for memory once.  NM: the number of moduli at compile time (16, the default's), or 0: cst.nmod
// (6 .. 15), the same code with the moduli past nmod skipped.  The sums themselves run over
// l = 0 .. nmod - 1 in that order for every entry.
// M2: the scale is Md + Mlo (oz_consts_cert), the low part entering by one more fma.
template <int NM, bool M2 = false>
__device__ __forceinline__ void oz_crt_entries(const OzCrt& g, const OzConst& cst) {
  const int nmod = NM ? NM : cst.nmod;
  const int t = (int)blockIdx.x >> 4;
  const int u = ((int)blockIdx.x & 15) * 256 + (int)threadIdx.x;
  int ti, tj;
  if (g.tri) {
    const int ta = t + (int)oz_res_tile(1, g.ntj, g.ti0, 0), cap = g.ntj * (g.ntj + 1) / 2;
    if (g.ntj > 0 && ta >= cap) {   // the capped triangle's full rows (oz_res_tile)
      ti = g.ntj + (ta - cap) / g.ntj;
      tj = (ta - cap) % g.ntj;
    } else {
      ti = g.ti0;
      while ((ti + 1) * (ti + 2) / 2 <= ta) ++ti;
      tj = ta - ti * (ti + 1) / 2;
    }
  } else {
    ti = g.ti0 + t / g.ntj;
    tj = t % g.ntj;
  }
  const int wave = u >> 10, blk = (u >> 6) & 15, lane = u & 63;
  const int i = blk >> 2, j = blk & 3;
  const int gm = OZ_T * ti + (wave >> 1) * 128 + 32 * i + (lane & 31);
  const int gn0 = OZ_T * tj + (wave & 1) * 128 + 32 * j + 4 * (lane >> 5);
  if (gm >= g.rows || gn0 >= g.cols) return;
  const int8_t* src = g.res + (long long)t * (OZ_T * OZ_T) + (long long)u * 16;
  oz_v4i w[OZ_MAXMOD];
#pragma unroll
  for (int l = 0; l < OZ_MAXMOD; ++l)
    if (l < nmod) w[l] = *reinterpret_cast<const oz_v4i*>(src + (long long)l * g.res_bytes);
  const int em = g.exr[gm];
  oz_v4i ec[4];   // (gn0 is a multiple of 4; the 16-byte load only where all four columns exist and exc allows it)
  const bool ec16 = (reinterpret_cast<uintptr_t>(g.exc) & 15) == 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int gn = gn0 + 8 * q;
    if (ec16 && gn + 3 < g.cols) {
      ec[q] = *reinterpret_cast<const oz_v4i*>(g.exc + gn);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) ec[q][i] = gn + i < g.cols ? g.exc[gn + i] : 0;
    }
  }
  double shi[16], slo[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) shi[r] = slo[r] = 0.0;
#pragma unroll
  for (int l = 0; l < OZ_MAXMOD; ++l)
    if (l < nmod) {
      const double rh = cst.rhi[l], rl = cst.rlo[l];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const double cv = (double)(int)(int8_t)((unsigned)w[l][r >> 2] >> (8 * (r & 3)));
        shi[r] = fma(cv, rh, shi[r]);   // exact: multiples of 2^-41 below 2^11
        slo[r] = fma(cv, rl, slo[r]);
      }
    }
  const double sc = g.alpha * cst.Md, scl = g.alpha * cst.Mlo;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int gn = gn0 + (r & 3) + 8 * (r >> 2);
    if (gn >= g.cols || (g.lower128 && (gm >> 7) < (gn >> 7))) continue;
    const double v = (shi[r] - rint(shi[r])) + slo[r];   // C' / M, centred
    const int en = ec[r >> 2][r & 3];
    double* dst = g.C + (gm - OZ_T * g.ti0 + (long long)gn * g.ldc);
    const double s = ldexp(sc, -(em + en));
    if (em == OZ_EX_NAN || en == OZ_EX_NAN) {
      *dst = __builtin_nan("");
    } else if constexpr (M2) {   // v (s + sl): sl below half an ulp of s, its term rounded into the result
      const double sl = ldexp(scl, -(em + en));
      if (g.acc) {
        // C + v (s + sl) to one rounding (and a second-order term): p + pe = v (s + sl), t + err = C + p,
        // both error-free.  A plain fma(v, sl, fma(v, s, C)) loses v sl wherever |C| is not far below
        // |v s|, which leaves every entry with the scale s alone: the common factor that oz_consts_cert
        // exists to remove
        const double c0 = *dst;
        const double p = __dmul_rn(v, s), pe = fma(v, sl, fma(v, s, -p));
        const double t = __dadd_rn(c0, p), bb = __dsub_rn(t, c0);
        const double err = __dadd_rn(__dsub_rn(c0, __dsub_rn(t, bb)), __dsub_rn(p, bb));
        *dst = __dadd_rn(t, __dadd_rn(err, pe));
      } else {
        *dst = fma(v, s, v * sl);
      }
    } else {
      *dst = g.acc ? fma(v, s, *dst) : v * s;
    }
  }
}
template <int NM>
static __global__ void __launch_bounds__(256) k_oz_crt(OzCrt g, OzConst cst) {
  oz_crt_entries<NM>(g, cst);
}
// A product with a certificate (N = 16): where the flag is set, the same sums over l = 0 .. 14
// with the 15-moduli constants c15 (oz_consts_cert: rhi, rlo and the scale Md + Mlo = M15 as
// the 16-moduli Md rounds it; the sixteenth residue is not read); where it is not,
// k_oz_crt<16>'s arithmetic
static __global__ void __launch_bounds__(256) k_oz_crt_cert(OzCrt g, OzConst cst, OzConst c15, const int* __restrict__ flag) {
  if (*flag) oz_crt_entries<OZ_CERT_NMOD, true>(g, c15);
  else oz_crt_entries<OZ_MAXMOD>(g, cst);
}

// ---- rectangular operands (the TRTRI's products): op(r, k) of an fp64 block src (ld) is
// src[k + r ld] (TRANS false: the rows are the block's columns) or src[r + k ld] (TRANS
// true), r < R, k < Kv; zero outside, and (mask) where k < r (1) or k > r (2): the lower
// triangle's nonzeros seen from a column (1) or a row (2).
__device__ __forceinline__ bool oz_keep(int mask, int r, int k) {
  return mask == 1 ? k >= r : (mask == 2 ? k <= r : true);
}

// per-row exponents e_r = beta - 1 - ilogb(max_k |op(r, k)|), rows r < Rp (0 past R or for a
// zero row).  TRANS false: one wave per row.  TRANS true: workgroup = 64 rows x 256 k (the
// lanes along r: coalesced), its maximum's ilogb + 2048 atomically max-ed into il (zeroed
// before), then k_oz_il_to_ex.
template <bool TRANS>
static __global__ void __launch_bounds__(256) k_oz_rowexp(const double* __restrict__ src, long long ld, int R, int Rp,
                                                          int Kv, int mask, int beta, int* __restrict__ ex,
                                                          unsigned long long* __restrict__ sum) {
  if constexpr (!TRANS) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= Rp) return;
    double mx = 0.0;
    if (r < R)
      for (int k = lane; k < Kv; k += 64)
        if (oz_keep(mask, r, k)) mx = oz_pmax(mx, fabs(src[k + (long long)r * ld]));
    for (int off = 32; off > 0; off >>= 1) mx = oz_pmax(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) {
      ex[r] = oz_ex_of(mx, beta);
      if (sum) sum[r] = 0ull;   // (the certificate's row sums: zeroed where the exponent is written)
    }
  } else {
    __shared__ double red[4][64];
    const int rl = threadIdx.x & 63, q = threadIdx.x >> 6, r = blockIdx.x * 64 + rl;
    const int k0 = blockIdx.y * 256;
    double mx = 0.0;
    if (r < R)
#pragma unroll 8
      for (int u = 0; u < 64; ++u) {
        const int k = k0 + 4 * u + q;
        if (k < Kv && oz_keep(mask, r, k)) mx = oz_pmax(mx, fabs(src[r + (long long)k * ld]));
      }
    red[q][rl] = mx;
    __syncthreads();
    if (q == 0 && r < R) {
      mx = oz_pmax(oz_pmax(red[0][rl], red[1][rl]), oz_pmax(red[2][rl], red[3][rl]));
      if (!(mx <= 1.7976931348623157e308)) atomicMax(ex + r, OZ_IL_BAD);
      else if (mx > 0.0) atomicMax(ex + r, ilogb(mx) + 2048);
    }
  }
}
static __global__ void __launch_bounds__(256) k_oz_il_to_ex(int* __restrict__ ex, int Rp, int beta,
                                                            unsigned long long* __restrict__ sum) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < Rp) {
    ex[r] = ex[r] >= OZ_IL_BAD ? OZ_EX_NAN : (ex[r] > 0 ? (beta - 1) - (ex[r] - 2048) : 0);
    if (sum) sum[r] = 0ull;
  }
}

// op -> the N int8 planes, rectangular (row r at r ldp + k, k < Kp; zero past R / Kv and
// masked), the residues by oz_residues8.  TRANS false: thread = 8 consecutive k of one row
// (contiguous in src: four 16-byte loads when the 8 are in range and on one side of the
// mask's diagonal); a thread whose 8 are all dropped writes its zeros and nothing else.
// TRANS true: workgroup = 64 rows x 64 k, thread = 2 adjacent rows x 8 consecutive k (each
// load 16 bytes, the lanes along r); the planes' 64 x 64 bytes go through LDS four planes a
// round (two barriers per round) so the stores run along k (4 threads per row, 16 bytes
// each); a block wholly dropped writes zeros without the LDS rounds.  The zeros are stored
// because a product's k range may cover them.
template <bool TRANS>
static __global__ void __launch_bounds__(256) k_oz_split_rect(const double* __restrict__ src, long long ld, int R,
                                                              int Kv, int mask, const int* __restrict__ ex,
                                                              int8_t* __restrict__ planes, long long plane_bytes,
                                                              long long ldp, int Kp, OzConst cst,
                                                              unsigned long long* __restrict__ sum) {
  if constexpr (!TRANS) {
    const int r = blockIdx.x;
    // this thread's 8 entries; its share of the row's certificate sum (0 where it stores zeros alone)
    const auto thread8 = [&]() -> unsigned long long {
    const int k0 = ((int)blockIdx.y * 256 + (int)threadIdx.x) * 8;
    if (k0 >= Kp) return 0ull;
    const int e = ex[r];
    const double* p = src + k0 + (long long)r * ld;
    // the mask's diagonal k = r: all 8 kept (1), all dropped (0), or mixed (2)
    const int side = mask == 1 ? (k0 >= r ? 1 : (k0 + 7 < r ? 0 : 2))
                   : (mask == 2 ? (k0 + 7 <= r ? 1 : (k0 > r ? 0 : 2)) : 1);
    int8_t* dst = planes + (long long)r * ldp + k0;
    if (side == 0 || r >= R || k0 >= Kv || e == OZ_EX_NAN) {   // all 8 zero: the stores alone
      for (int l = 0; l < cst.nmod; ++l) *reinterpret_cast<uint2*>(dst + (long long)l * plane_bytes) = make_uint2(0u, 0u);
      return 0ull;
    }
    double xs[8];
    if (k0 + 8 <= Kv && side == 1 && ((reinterpret_cast<uintptr_t>(p) & 15) == 0)) {
#pragma unroll
      for (int u = 0; u < 8; u += 2) {
        const double2 v = *reinterpret_cast<const double2*>(p + u);
        xs[u] = v.x;
        xs[u + 1] = v.y;
      }
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + u;
        xs[u] = (k < Kv && oz_keep(mask, r, k)) ? p[u] : 0.0;
      }
    }
    OzDigits d[8];
    unsigned long long s = 0ull;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double xr = rint(ldexp(xs[u], e));
      d[u] = oz_digits(xr);
      if (sum) s += oz_cert_term(xr);
    }
    for (int l = 0; l < cst.nmod; ++l) *reinterpret_cast<uint2*>(dst + (long long)l * plane_bytes) = oz_residues8(d, cst, l);
    return s;
    };
    const unsigned long long s = thread8();
    if (sum) oz_cert_block_add(s, sum, r);   // (sum: the same for the whole workgroup) one atomic per workgroup
  } else {
    constexpr int PL = 4;   // planes per LDS round
    __shared__ __attribute__((aligned(16))) unsigned tr[PL][64 * 20];   // [plane][row][16 words + 4 pad]
    const int lane = threadIdx.x & 63, rp = lane & 31, kg = (int)threadIdx.x >> 5;
    const int wr = (int)threadIdx.x >> 2, wp = (int)threadIdx.x & 3;   // row wr, piece wp of the block
    int8_t* dst = planes + ((long long)blockIdx.x * 64 + wr) * ldp + (long long)blockIdx.y * 64 + 16 * wp;
    {   // a block wholly past R / Kv or on the mask's dropped side (the same for the whole workgroup): zeros alone
      const int rb = (int)blockIdx.x * 64, kb = (int)blockIdx.y * 64;
      if (rb >= R || kb >= Kv || (mask == 1 && kb + 63 < rb) || (mask == 2 && kb > rb + 63)) {
        for (int l = 0; l < cst.nmod; ++l) *reinterpret_cast<uint4*>(dst + (long long)l * plane_bytes) = make_uint4(0u, 0u, 0u, 0u);
        return;
      }
    }
    const int r = (int)blockIdx.x * 64 + 2 * rp;          // rows r, r + 1
    const int k0 = (int)blockIdx.y * 64 + 8 * kg;         // k0 .. k0 + 7
    const int e0 = ex[r], e1 = ex[r + 1];
    double x0[8], x1[8];
    const double* p = src + r + (long long)k0 * ld;
    const bool vec = r + 1 < R && ((reinterpret_cast<uintptr_t>(src + r) & 15) == 0) && (ld & 1) == 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = k0 + u;
      double a = 0.0, b = 0.0;
      if (k < Kv) {
        if (vec) {
          const double2 v = *reinterpret_cast<const double2*>(p + (long long)u * ld);
          a = v.x;
          b = v.y;
        } else {
          if (r < R) a = p[(long long)u * ld];
          if (r + 1 < R) b = p[(long long)u * ld + 1];
        }
      }
      x0[u] = oz_keep(mask, r, k) ? a : 0.0;
      x1[u] = oz_keep(mask, r + 1, k) ? b : 0.0;
    }
    OzDigits d0[8], d1[8];
    unsigned long long s0 = 0ull, s1 = 0ull;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double xr0 = e0 == OZ_EX_NAN ? 0.0 : rint(ldexp(x0[u], e0));
      const double xr1 = e1 == OZ_EX_NAN ? 0.0 : rint(ldexp(x1[u], e1));
      d0[u] = oz_digits(xr0);
      d1[u] = oz_digits(xr1);
      if (sum) {
        s0 += oz_cert_term(xr0);
        s1 += oz_cert_term(xr1);
      }
    }
    if (sum) {   // (the same for the whole workgroup) the 64 rows' certificate sums: one atomic per row
      __shared__ unsigned long long rs[8][64];
      rs[kg][2 * rp] = s0;
      rs[kg][2 * rp + 1] = s1;
      __syncthreads();
      if (threadIdx.x < 64) {
        unsigned long long t = 0ull;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += rs[q][threadIdx.x];
        atomicAdd(sum + (long long)blockIdx.x * 64 + threadIdx.x, t);
      }
    }
    for (int l0 = 0; l0 < cst.nmod; l0 += PL) {
      if (l0 > 0) __syncthreads();   // (the previous round's reads done)
#pragma unroll
      for (int q = 0; q < PL; ++q)
        if (l0 + q < cst.nmod) {
          *reinterpret_cast<uint2*>(tr[q] + (2 * rp) * 20 + 2 * kg) = oz_residues8(d0, cst, l0 + q);
          *reinterpret_cast<uint2*>(tr[q] + (2 * rp + 1) * 20 + 2 * kg) = oz_residues8(d1, cst, l0 + q);
        }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < PL; ++q)
        if (l0 + q < cst.nmod)
          *reinterpret_cast<uint4*>(dst + (long long)(l0 + q) * plane_bytes) =
              *reinterpret_cast<const uint4*>(tr[q] + wr * 20 + 4 * wp);
    }
  }
}

// ---- host side (gpemu.hip, gpemu_dist.hip)

// moduli and reconstruction constants for operand sums of length up to np2
inline OzConst oz_consts(int nmod, int np2) {
  static const int mods[OZ_MAXMOD] = {256, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217, 211, 199, 197, 193, 191};
  OzConst k{};
  k.nmod = nmod;
  double log2M = 0.0, Md = 1.0;
  for (int l = 0; l < nmod; ++l) {
    log2M += std::log2((double)mods[l]);
    Md *= (double)mods[l];
  }
  k.Md = Md;
  // |C'| <= np2 2^(2 beta) < M / 2
  k.beta = std::min(53, (int)std::floor((log2M - 1.0 - std::log2((double)np2) - 1e-9) / 2.0));
  for (int l = 0; l < nmod; ++l) {
    const int m = mods[l];
    k.m[l] = m;
    k.c16[l] = 65536 % m;
    k.inv[l] = 1.0f / (float)m;
    unsigned w[2] = {0u, 0u};   // centred 256^i mod m, i = 0 .. 6, one int8 each
    for (int i = 0, p = 1; i < 7; ++i, p = (p * 256) % m) {
      const int wc = p > m / 2 ? p - m : p;   // (m = 256: 1, 0, ..; odd m: |wc| <= 126)
      w[i >> 2] |= ((unsigned)wc & 0xffu) << (8 * (i & 3));
    }
    k.wlo[l] = (int)w[0];
    k.whi[l] = (int)w[1];
    long long Mm = 1;   // (M / m) mod m
    for (int j = 0; j < nmod; ++j)
      if (j != l) Mm = (Mm * (mods[j] % m)) % m;
    int y = 1;          // its inverse mod m
    while ((Mm * y) % m != 1) ++y;
    // y / m = rhi + rlo, rhi on the 2^-41 grid (exact products and sums in k_oz_crt)
    const long long num = (long long)y << 41;
    const long long Q = num / m, R = num - Q * m;
    k.rhi[l] = std::ldexp((double)Q, -41);
    k.rlo[l] = std::ldexp((double)R / (double)m, -41);
  }
  return k;
}

// The reconstruction constants of a certified product: the first 15 moduli with the operands
// still at 53 bits.  oz_consts(15, .) alone would lower beta to what 15 moduli carry without a
// certificate (|C'| <= np2 2^(2 beta) < M15 / 2: 51 bits at np2 = 16384); here the certificate
// bounds |C'|, beta stays the 16-moduli context's, and only rhi, rlo and the scale are used
// (k_oz_crt_cert) -- the moduli, weights and reciprocals are the first 15 of the 16.
// The scale: Md is one rounding of M, the same relative error e in every entry of a product (of
// 16 moduli: 1.13 2^-53; of 15 alone: -0.66 2^-53 or so), and the objective's gradient, a
// difference of large terms, magnifies what is common to all entries (measured at n = 1100:
// 15-moduli products scaled by fl(M15) moved the gradient 2.1e-13 of its scale from the
// 16-moduli result, three times the 16-moduli result's own distance from the fp64 path).  So a
// certified product is scaled by Md16 / 191 carried in two doubles (Md + Mlo, exact to 2^-105):
// M15 with the 16-moduli constant's own e, and a product's value does not depend on whether it
// was certified beyond the reconstruction's last roundings.
inline OzConst oz_consts_cert(int np2) {
  OzConst k = oz_consts(OZ_CERT_NMOD, np2);
  const OzConst k16 = oz_consts(OZ_MAXMOD, np2);
  const double last = (double)k16.m[OZ_CERT_NMOD];
  k.beta = k16.beta;
  k.Md = k16.Md / last;
  k.Mlo = std::fma(-k.Md, last, k16.Md) / last;   // (the division's remainder is exact)
  return k;
}

// A product's tile list: blocks of OZ_BR tile rows x OZ_BC tile columns (8 x 4; GPEMU_OZ_BLOCK
// "RxC" for A/B runs: 4 x 8, 16 x 2 and 8 x 8 measured within 1%, the LAUUM ~0.15 ms slower
// at 4 x 8, profiles/ozblock_ab_r06*.log) (clipped to the lower
// triangle when lower), heaviest first, greedily binned by work into 8 XCD bins, interleaved
// position by position (bin = position % 8, the XCD under round-robin dispatch), bins padded
// to one length with 0xffffffff; tile rows ti0 .. ti0 + nti - 1.  An XCD's 32 CUs then run one
// block at a time: its tiles share 8 A panels and 4 B panels (a whole tile row on one XCD
// shared one A panel among 32 different B panels: L2 hit rate ~0.5)
template <class W>
std::vector<unsigned> oz_list(int nti, int ntj, bool lower, W work, int ti0 = 0) {
  static const std::pair<int, int> blk = [] {   // (A/B: GPEMU_OZ_BLOCK="RxC")
    int r = 8, c = 4;
    if (const char* e = std::getenv("GPEMU_OZ_BLOCK")) {
      const int rr = std::atoi(e);
      const char* x = std::strchr(e, 'x');
      if (rr > 0 && x && std::atoi(x + 1) > 0) { r = rr; c = std::atoi(x + 1); }
    }
    return std::make_pair(r, c);
  }();
  const int OZ_BR = blk.first, OZ_BC = blk.second;
  struct Blk { double w; std::vector<unsigned> t; };
  std::vector<Blk> blks;
  for (int r0 = ti0; r0 < ti0 + nti; r0 += OZ_BR)
    for (int c0 = 0; c0 < ntj && (!lower || c0 <= r0 + OZ_BR - 1); c0 += OZ_BC) {
      Blk b{0.0, {}};
      for (int ti = r0; ti < std::min(ti0 + nti, r0 + OZ_BR); ++ti)
        for (int tj = c0; tj < std::min(std::min(lower ? ti + 1 : ntj, ntj), c0 + OZ_BC); ++tj) {
          b.t.push_back(((unsigned)ti << 16) | (unsigned)tj);
          b.w += work(ti, tj);
        }
      if (!b.t.empty()) blks.push_back(std::move(b));
    }
  std::stable_sort(blks.begin(), blks.end(), [](const Blk& x, const Blk& y) { return x.w / x.t.size() > y.w / y.t.size(); });
  std::vector<std::vector<unsigned>> bins(8);
  std::vector<double> load(8, 0.0);
  for (const Blk& b : blks) {
    const int x = (int)(std::min_element(load.begin(), load.end()) - load.begin());
    load[x] += b.w;
    bins[x].insert(bins[x].end(), b.t.begin(), b.t.end());
  }
  size_t longest = 0;
  for (auto& b : bins) longest = std::max(longest, b.size());
  std::vector<unsigned> list(8 * longest, 0xffffffffu);
  for (int x = 0; x < 8; ++x)
    for (size_t q = 0; q < bins[x].size(); ++q) list[8 * q + x] = bins[x][q];
  return list;
}

// ---- the launch layer: every int8 product of gpemu.hip and gpemu_dist.hip (and the test hook
// gpe_test_oz_product) converts its operands, builds its tile list and launches through here.

// A rectangular operand's source (op(r, k), R, Kv, mask as above k_oz_rowexp; trans = TRANS)
struct OzSrc {
  const double* src;
  long long ld;
  int R, Kv, mask;
  bool trans;
};
// its row exponents into ex[0, P) (P = R padded to 256) ...
// (sum, here and below: the certificate's row sums beside ex, or null)
inline void oz_operand_exp(hipStream_t st, const OzConst& k, const OzSrc& o, int P, int* ex,
                           unsigned long long* sum = nullptr) {
  if (o.trans) {
    (void)hipMemsetAsync(ex, 0, (size_t)P * sizeof(int), st);
    hipLaunchKernelGGL(k_oz_rowexp<true>, dim3(P / 64, (o.Kv + 255) / 256), dim3(256), 0, st, o.src, o.ld, o.R, P, o.Kv,
                       o.mask, k.beta, ex, sum);
    hipLaunchKernelGGL(k_oz_il_to_ex, dim3((P + 255) / 256), dim3(256), 0, st, ex, P, k.beta, sum);
  } else {
    hipLaunchKernelGGL(k_oz_rowexp<false>, dim3(P / 4), dim3(256), 0, st, o.src, o.ld, o.R, P, o.Kv, o.mask, k.beta, ex,
                       sum);
  }
}
// ... and its planes: P rows of Kp bytes (a multiple of 64) per modulus, P Kp bytes apart
inline void oz_operand_split(hipStream_t st, const OzConst& k, const OzSrc& o, int P, int Kp, const int* ex, int8_t* planes,
                             unsigned long long* sum = nullptr) {
  if (o.trans)
    hipLaunchKernelGGL(k_oz_split_rect<true>, dim3(P / 64, Kp / 64), dim3(256), 0, st, o.src, o.ld, o.R, o.Kv, o.mask, ex,
                       planes, (long long)P * Kp, (long long)Kp, Kp, k, sum);
  else
    hipLaunchKernelGGL(k_oz_split_rect<false>, dim3(P, (Kp + 2047) / 2048), dim3(256), 0, st, o.src, o.ld, o.R, o.Kv,
                       o.mask, ex, planes, (long long)P * Kp, (long long)Kp, Kp, k, sum);
}
inline void oz_operand(hipStream_t st, const OzConst& k, const OzSrc& o, int P, int Kp, int* ex, int8_t* planes,
                       unsigned long long* sum = nullptr) {
  oz_operand_exp(st, k, o, P, ex, sum);
  oz_operand_split(st, k, o, P, Kp, ex, planes, sum);
}
// the packed operand (the LAUUM's): column exponents and the lower column panels of X (np x np
// of the padded order np2, ld ldx), oz_plane_bytes(np2) per modulus
inline void oz_operand_packed(hipStream_t st, const OzConst& k, const double* X, long long ldx, int np, int np2, int* ex,
                              int8_t* planes, unsigned long long* sum = nullptr) {
  hipLaunchKernelGGL(k_oz_colexp, dim3((np2 + 3) / 4), dim3(256), 0, st, X, ldx, np, np2, k.beta, ex, sum);
  hipLaunchKernelGGL(k_oz_split, dim3(np2, (np2 + 256 * OZ_SPLIT_ROWS - 1) / (256 * OZ_SPLIT_ROWS)), dim3(256), 0, st, X,
                     ldx, np, np2, ex, planes, oz_plane_bytes(np2), k, sum);
}

// A product's shape, stated once: tile rows [ti0, ti0 + nti) against ntj tile columns, or (tri)
// against the lower triangle's tj <= ti, whole (ntj 0) or capped at ntj tile columns (a
// trapezoid: tj <= min(ti, ntj - 1)); K, kbeg, kend, kdiv as OzGemm's
struct OzShape {
  int nti, ntj, ti0, tri, K, kbeg, kend, kdiv;
  static OzShape lower(int nti, int ti0, int K, int kbeg, int kdiv = 1) { return {nti, 0, ti0, 1, K, kbeg, 0, kdiv}; }
  static OzShape lower_capped(int nti, int cap, int K) { return {nti, cap < nti ? cap : 0, 0, 1, K, 0, 0, 1}; }
  static OzShape rect(int nti, int ntj, int K, int kbeg, int kend) { return {nti, ntj, 0, 0, K, kbeg, kend, 1}; }
  // tile columns of tile row ti
  int row_tiles(int ti) const { return tri ? (ntj > 0 ? std::min(ti + 1, ntj) : ti + 1) : ntj; }
  // length of tile (ti, tj)'s k range: its weight in the list, its share of the operations
  int klen(int ti, int tj) const {
    int kb, ke;
    oz_k_range(kbeg, kend, kdiv, K, ti, tj, kb, ke);
    return std::max(0, ke - kb);
  }
  std::vector<unsigned> list() const {
    return oz_list(nti, tri && ntj == 0 ? ti0 + nti : ntj, tri != 0, [&](int ti, int tj) { return (double)klen(ti, tj); }, ti0);
  }
  // residue tile of (ti, tj) less that of the shape's first (k_oz_gemm's and k_oz_crt's index)
  long long res_tile(int ti, int tj) const { return oz_res_tile(tri, ntj, ti, tj) - oz_res_tile(tri, ntj, ti0, 0); }
  // residue tiles (tri: the lower tiles of the rows up to ti0 + nti less those above ti0)
  long long tiles() const { return tri ? oz_res_tile(1, ntj, ti0 + nti, 0) - oz_res_tile(1, ntj, ti0, 0) : (long long)nti * ntj; }
  long long res_bytes() const { return tiles() * OZ_T * OZ_T; }   // per modulus
  // int8 operations with N moduli
  double ops(int N) const {
    double s = 0.0;
    for (int ti = ti0; ti < ti0 + nti; ++ti)
      for (int tj = 0; tj < row_tiles(ti); ++tj) s += klen(ti, tj);
    return 2.0 * OZ_T * OZ_T * s * N;
  }
};

// the LAUUM's X^T X at the padded order np2: the lower tiles, tile row ti's sums from its
// diagonal block on
inline OzShape oz_lauum_shape(int np2) { return OzShape::lower(np2 / OZ_T, 0, np2, 1); }
// the row-block A^-1 partial's slab of 128-tile rows [a0, a1) (a0 even) over Kp local rows of
// one of P ranks: 256-tile row ti's sums from local row 128 floor(2 ti / P) on
inline OzShape oz_slab_shape(int a0, int a1, int Kp, int P) {
  return OzShape::lower((a1 + 1) / 2 - a0 / 2, a0 / 2, Kp, 3, P);
}

// where a product's reconstruction goes (as OzCrt)
struct OzOut {
  const int* exr;
  const int* exc;
  double* C;
  long long ldc;
  int rows, cols, lower128;
  double alpha;
  int acc = 0;
};
// A product's certificate (optional; flag null: none, the product runs on every modulus of the
// context): the operands' row sums (na rows of a's, nb of b's: every row the product may read),
// a device int for its flag and the 15-moduli constants (oz_consts_cert).  Used only where the
// context runs 16 moduli.
struct OzCert {
  const unsigned long long* sa = nullptr;
  int na = 0;
  const unsigned long long* sb = nullptr;
  int nb = 0;
  int* flag = nullptr;
  const OzConst* c15 = nullptr;
  unsigned long long* maxima = nullptr;   // (optional) A = max s_a and B = max s_b go here
};
// One product: its shape, the operands' planes, the shape's list on the device, the residue
// buffer (res_bytes per modulus, at least s.res_bytes()) and the output
struct OzProduct {
  OzShape s;
  OzOpnd a, b;
  const unsigned* list;
  int list_len;
  int8_t* res;
  long long res_bytes;
  OzOut out;
  OzCert cert{};
};
// The one launch of k_oz_gemm (a workgroup per modulus and list position, the whole ring as
// dynamic LDS: one workgroup per CU) and of k_oz_crt (16 workgroups per residue tile) behind
// it.  e0, e1: events recorded just before and after k_oz_gemm (gpe_ozaki_stats times it alone).
// With a certificate, k_oz_cert first (after the conversions, in stream order): the flag stays on
// the device, where k_oz_gemm's last list_len workgroups and k_oz_crt_cert read it; the host
// never waits for it.
inline hipError_t oz_product_launch(hipStream_t st, const OzConst& k, const OzProduct& p, hipEvent_t e0 = nullptr,
                                    hipEvent_t e1 = nullptr) {
  const OzShape& s = p.s;
  const int ntj = s.ntj;   // (tri: 0, or the cap)
  const OzCert& ct = p.cert;
  const bool cert = ct.flag && ct.c15 && k.nmod == OZ_MAXMOD;
  const OzGemm g{p.a, p.b, p.list, p.list_len, s.K, s.kbeg, s.kend, s.tri, ntj, p.res, p.res_bytes, s.kdiv, s.ti0,
                 cert ? ct.flag : nullptr};
  const OzOut& o = p.out;
  const OzCrt r{p.res, p.res_bytes, s.tri, ntj, o.exr, o.exc, o.C, o.ldc, o.rows, o.cols, o.lower128, o.alpha, s.ti0, o.acc};
  hipError_t e;
  if (cert) hipLaunchKernelGGL(k_oz_cert, dim3(1), dim3(256), 0, st, ct.sa, ct.na, ct.sb, ct.nb, ct.flag,
                             ct.maxima);
  if (e0 && (e = hipEventRecord(e0, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_oz_gemm, dim3((unsigned)(k.nmod * g.list_len)), dim3(256), OZ_LDS, st, g, k);
  if (e1 && (e = hipEventRecord(e1, st)) != hipSuccess) return e;
  if (cert) hipLaunchKernelGGL(k_oz_crt_cert, dim3((unsigned)(s.tiles() * 16)), dim3(256), 0, st, r, k, *ct.c15, ct.flag);
  else if (k.nmod == OZ_MAXMOD) hipLaunchKernelGGL(k_oz_crt<OZ_MAXMOD>, dim3((unsigned)(s.tiles() * 16)), dim3(256), 0, st, r, k);
  else hipLaunchKernelGGL(k_oz_crt<0>, dim3((unsigned)(s.tiles() * 16)), dim3(256), 0, st, r, k);
  return hipGetLastError();
}

// The block pairs (t0, h, t1) of the TRTRI level of span s tiles (s = 2, 4, ... while
// s / 2 < NB; tile units of 128): X(t0:h, t0:h) and X(h:t1, h:t1) are inverted, the level fills
// X(h:t1, t0:h).  The last pair of a level is ragged (t1 = NB) and a block without a lower
// half has no pair.  One definition for the fp64 schedule (build_chol_plan) and the int8 plans.
inline std::vector<std::array<int, 3>> trtri_level_pairs(int NB, int s) {
  std::vector<std::array<int, 3>> prs;
  for (int t0 = 0; t0 < NB; t0 += s) {
    const int h = t0 + s / 2;
    if (h >= NB) continue;
    prs.push_back({t0, h, std::min(t0 + s, NB)});
  }
  return prs;
}

// A level's pairs on one side of tile column hs (the split Cholesky's, a power of two): side 0
// those inside [0, hs), side 1 those inside [hs, NB).  A pair that straddles hs, the top one
// (0, hs, NB), is on neither side.
inline std::vector<std::array<int, 3>> trtri_side_pairs(const std::vector<std::array<int, 3>>& prs, int hs, int side) {
  std::vector<std::array<int, 3>> out;
  for (const auto& pr : prs)
    if (!(pr[0] < hs && pr[2] > hs) && (pr[0] >= hs) == (side == 1)) out.push_back(pr);
  return out;
}

// ---- one block pair (t0, h, t1) of a TRTRI level (tile units of 128) on the int8 cores:
// the blocks X11 = X(t0:h, t0:h) and X22 = X(h:t1, h:t1) already inverted, L21 = L(h:t1,
// t0:h):
//   T   = L21 X11      (rows of L21 against columns of X11, k >= the column: kbeg = 256 tj)
//   X21 = -X22 T       (rows of X22, k <= the row: kend = 256 (ti + 1), against columns of T)
// T goes to a scratch block (column-major, ld Pb, so its columns are the second product's
// rows).  Plan (host): the rows of each block (Ra, Rb), padded to 256 (Pa, Pb), the two
// products' shapes, their tile lists' offsets in a list array, and their int8 operations
// (every modulus).
struct OzTriPair {
  int t0, h, t1, Ra, Rb, Pa, Pb;
  long long la_off, lb_off;
  int la_len, lb_len;
  double ops_a, ops_b;
  OzShape shape_a() const { return OzShape::rect(Pb / OZ_T, Pa / OZ_T, Pa, 2, 0); }
  OzShape shape_b() const { return OzShape::rect(Pb / OZ_T, Pa / OZ_T, Pb, 0, 1); }
  // the split Cholesky's S = A22 - L21 L21^T on the pair (0, h, NB): the lower tiles, every sum K = Pa
  OzShape shape_schur() const { return OzShape::lower(Pb / OZ_T, 0, Pa, 0); }
  size_t planes_bytes(int N) const { return (size_t)N * Pa * (Pa + Pb); }
  size_t resid_bytes(int N) const { return (size_t)N * shape_a().res_bytes(); }   // (shape_b's too)
  // the first product's L21 side
  OzSrc l21(const double* L21, long long ld) const { return {L21, ld, Rb, Ra, 0, true}; }
};
inline OzTriPair oz_tri_pair_plan(int t0, int h, int t1, int N, std::vector<unsigned>& lists) {
  OzTriPair q;
  q.t0 = t0; q.h = h; q.t1 = t1;
  q.Ra = (h - t0) * TILE;
  q.Rb = (t1 - h) * TILE;
  q.Pa = (q.Ra + OZ_T - 1) / OZ_T * OZ_T;
  q.Pb = (q.Rb + OZ_T - 1) / OZ_T * OZ_T;
  const std::vector<unsigned> la = q.shape_a().list(), lb = q.shape_b().list();
  q.ops_a = q.shape_a().ops(N);
  q.ops_b = q.shape_b().ops(N);
  q.la_off = (long long)lists.size();
  q.la_len = (int)la.size();
  lists.insert(lists.end(), la.begin(), la.end());
  q.lb_off = (long long)lists.size();
  q.lb_len = (int)lb.size();
  lists.insert(lists.end(), lb.begin(), lb.end());
  return q;
}

// ---- the split Cholesky's first phase split once more at tile column q = h / 2 (q even): the
// trapezoid {rows [q, NB), columns [q, h), column <= row} of A takes the update by columns
// [0, q) as one product.  The one operand, used on both sides, is the rows [q, NB) of L's
// columns [0, q) (Rb rows padded to Pb, every sum K = 128 q long; b's rows are a's first
// 128 (h - q)); the shape is the lower triangle capped at (h - q) / 2 tile columns.
struct OzCholNest {
  int q, h, NB, Rb, Pb, K, cols;
  OzShape shape() const { return OzShape::lower_capped(Pb / OZ_T, (h - q) / 2, K); }
  OzSrc src(const double* Lq0, long long ld) const { return {Lq0, ld, Rb, K, 0, true}; }
  size_t planes_bytes(int N) const { return (size_t)N * Pb * K; }
  size_t resid_bytes(int N) const { return (size_t)N * shape().res_bytes(); }
};
inline OzCholNest oz_chol_nest_plan(int q, int h, int NB) {
  OzCholNest n;
  n.q = q; n.h = h; n.NB = NB;
  n.Rb = (NB - q) * TILE;
  n.Pb = (n.Rb + OZ_T - 1) / OZ_T * OZ_T;
  n.K = q * TILE;
  n.cols = (h - q) * TILE;
  return n;
}

// both products of the pair on stream st (X blocks and L21 with leading dimension ld; T:
// Pb x Pa doubles; planes: q.planes_bytes(N); res: q.resid_bytes(N); ex: Pa + Pb ints;
// lists: the list array of oz_tri_pair_plan, on the device).  l21_done: L21's operand
// (q.l21: planes at planes, exponents at ex) is already there (ordered before st's work by the
// caller).  gc(p, ops, flops64) launches one product (oz_product_launch).  part: 0 both
// products, 1 the first alone (T, which needs X11 and not X22), 2 the second alone (T is there).
// sum (or null): the certificate's row sums beside ex (Pa + Pb; with l21_done L21's are there as
// its exponents are); cert(sa, na, sb, nb) then makes each product's certificate.
template <class GC, class CT>
void oz_tri_pair_launches(hipStream_t st, const OzConst& k, const OzTriPair& q, const unsigned* lists, const double* L21,
                          const double* X11, const double* X22, double* X21, long long ld, double* T, int8_t* planes,
                          int8_t* res, int* ex, bool l21_done, GC gc, int part, unsigned long long* sum, CT cert) {
  int* exA = ex;
  int* exB = ex + q.Pb;
  unsigned long long* sA = sum;
  unsigned long long* sB = sum ? sum + q.Pb : nullptr;
  int8_t* PA = planes;
  const long long rb = q.shape_a().res_bytes();
  if (part != 2) {   // T = L21 X11
    const long long pA = (long long)q.Pb * q.Pa, pB = (long long)q.Pa * q.Pa;
    int8_t* PB = planes + (size_t)k.nmod * pA;
    if (!l21_done) oz_operand(st, k, q.l21(L21, ld), q.Pb, q.Pa, exA, PA, sA);
    oz_operand(st, k, OzSrc{X11, ld, q.Ra, q.Ra, 1, false}, q.Pa, q.Pa, exB, PB, sB);
    gc(OzProduct{q.shape_a(), OzOpnd{PA, pA, q.Pa, 0}, OzOpnd{PB, pB, q.Pa, 0}, lists + q.la_off, q.la_len, res, rb,
                 OzOut{exA, exB, T, (long long)q.Pb, q.Rb, q.Ra, 0, 1.0}, sum ? cert(sA, q.Pb, sB, q.Pa) : OzCert{}},
       q.ops_a, (double)q.Ra * q.Ra * q.Rb);
  }
  if (part != 1) {   // X21 = -X22 T (both operands' exponents, then both operands' planes)
    const long long pA = (long long)q.Pb * q.Pb, pB = (long long)q.Pa * q.Pb;
    int8_t* PB = planes + (size_t)k.nmod * pA;
    const OzSrc x22{X22, ld, q.Rb, q.Rb, 2, true}, t{T, (long long)q.Pb, q.Ra, q.Rb, 0, false};
    oz_operand_exp(st, k, x22, q.Pb, exA, sA);
    oz_operand_exp(st, k, t, q.Pa, exB, sB);
    oz_operand_split(st, k, x22, q.Pb, q.Pb, exA, PA, sA);
    oz_operand_split(st, k, t, q.Pa, q.Pb, exB, PB, sB);
    gc(OzProduct{q.shape_b(), OzOpnd{PA, pA, q.Pb, 0}, OzOpnd{PB, pB, q.Pb, 0}, lists + q.lb_off, q.lb_len, res, rb,
                 OzOut{exA, exB, X21, ld, q.Rb, q.Ra, 0, -1.0}, sum ? cert(sA, q.Pb, sB, q.Pa) : OzCert{}},
       q.ops_b, (double)q.Rb * q.Rb * q.Ra);
  }
}

// (without certificates: the row-block path)
template <class GC>
void oz_tri_pair_launches(hipStream_t st, const OzConst& k, const OzTriPair& q, const unsigned* lists, const double* L21,
                          const double* X11, const double* X22, double* X21, long long ld, double* T, int8_t* planes,
                          int8_t* res, int* ex, bool l21_done, GC gc, int part = 0) {
  oz_tri_pair_launches(st, k, q, lists, L21, X11, X22, X21, ld, T, planes, res, ex, l21_done, gc, part, nullptr,
                       [](const unsigned long long*, int, const unsigned long long*, int) { return OzCert{}; });
}

}  // namespace gpe
