"""ctypes binding of libgpemu.so (the HIP/gfx950 hot path, include/gpemu.h).

There is no CPU fallback: if the library cannot be loaded, or no GPU is
visible, every entry point raises ``NativeUnavailable``.  The reference's
arithmetic (NumPy/SciPy, _emulatorkernels.py / _emulatoroptimise.py /
_emulatorclasses.py) is replaced here, not mirrored.
"""
from __future__ import annotations

import ctypes as _ct
import hashlib as _hashlib
import os as _os
import threading as _threading

import numpy as _np

_HERE = _os.path.dirname(_os.path.abspath(__file__))
_DEFAULT_LIB = _os.path.join(_HERE, "libgpemu.so")
LIB_PATH = _os.environ.get("GPEMU_LIB", _DEFAULT_LIB)

GPE_OK = 0
GPE_NOT_PD = 1
KERNEL_STD = 0
KERNEL_ALT_NUG = 1
KERNEL_MATERN32 = 0x10   # correlation family, OR-ed with the nugget code (0: Gaussian)
KERNEL_MATERN52 = 0x20
GP4ML = 0
MUCM = 1

_D = _ct.POINTER(_ct.c_double)
_VP = _ct.c_void_p

class OzOperand(_ct.Structure):
    """gpe_oz_operand (gpe_test_oz_product)"""
    _fields_ = [("src", _D), ("len", _ct.c_int64), ("offset", _ct.c_int64), ("ld", _ct.c_int64),
                ("trans", _ct.c_int32), ("R", _ct.c_int32), ("Kv", _ct.c_int32), ("mask", _ct.c_int32)]


class OzParams(_ct.Structure):
    """gpe_oz_params (gpe_test_oz_product)"""
    _fields_ = [(n, _ct.c_int32) for n in ("packed", "K", "kbeg", "kend", "kdiv", "ti0", "tri", "lower128", "acc",
                                           "nmod", "rows", "cols", "res_mod")] + \
               [("ldc", _ct.c_int64), ("c_len", _ct.c_int64), ("alpha", _ct.c_double)]


class GemmGroupProb(_ct.Structure):
    """gpe_gemm_group_prob (gpe_test_gemm_group)"""
    _fields_ = [(n, _ct.c_int32) for n in ("a_buf", "b_buf", "c_buf", "mt", "nt", "K", "flags", "kti_mul",
                                           "kti_off")] + \
               [(n, _ct.c_int64) for n in ("a_off", "lda", "b_off", "ldb", "c_off", "ldc")] + \
               [("alpha", _ct.c_double), ("beta", _ct.c_double)]


class GemmGroupLaunch(_ct.Structure):
    """gpe_gemm_group_launch (gpe_test_gemm_group)"""
    _fields_ = [(n, _ct.c_int32) for n in ("kind", "split", "listed", "reps")]


G_CLOWER, G_KBEG_TI, G_KEND_TI = 1, 2, 4   # gpe_gemm_group_prob.flags

# name -> (restype, argtypes); the full exported surface of include/gpemu.h
SIGNATURES = {
    "gpe_test_gemm_group": (_ct.c_int, [_VP, _ct.c_int32, _ct.POINTER(_D), _ct.POINTER(_ct.c_int64), _ct.c_int32,
                                        _ct.POINTER(GemmGroupProb), _ct.POINTER(GemmGroupLaunch),
                                        _ct.POINTER(_ct.c_int32), _ct.POINTER(_ct.c_int32),
                                        _ct.POINTER(_ct.c_uint32), _ct.c_int64]),
    "gpe_test_oz_product": (_ct.c_int, [_VP, _ct.POINTER(OzOperand), _ct.POINTER(OzOperand),
                                        _ct.POINTER(OzParams), _D, _ct.POINTER(_ct.c_int32),
                                        _ct.POINTER(_ct.c_int32), _ct.POINTER(_ct.c_int8)]),
    "gpe_test_oz_product_cert": (_ct.c_int, [_VP, _ct.POINTER(OzOperand), _ct.POINTER(OzOperand),
                                             _ct.POINTER(OzParams), _D, _ct.POINTER(_ct.c_int32),
                                             _ct.POINTER(_ct.c_int32), _ct.POINTER(_ct.c_int8),
                                             _ct.POINTER(_ct.c_int32)]),
    "gpe_test_oz_planes": (_ct.c_int, [_VP, _ct.POINTER(OzOperand), _ct.c_int32, _ct.c_int32, _ct.c_int32,
                                       _ct.POINTER(_ct.c_int32), _ct.POINTER(_ct.c_int8)]),
    "gpe_abi_version": (_ct.c_int, []),
    "gpe_build_id": (_ct.c_char_p, []),
    "gpe_device_count": (_ct.c_int, []),
    "gpe_device_synchronize": (_ct.c_int, [_ct.c_int32]),
    "gpe_create": (_VP, [_ct.c_int32]),
    "gpe_destroy": (None, [_VP]),
    "gpe_last_error": (_ct.c_char_p, [_VP]),
    "gpe_set_data": (_ct.c_int, [_VP, _ct.c_int64, _ct.c_int32, _ct.c_int32, _D, _D, _D, _D]),
    "gpe_objective": (_ct.c_int, [_VP, _ct.c_int32, _ct.c_int32, _D, _ct.c_int32, _ct.c_double,
                                  _ct.c_int32, _D, _D, _D]),
    "gpe_factor": (_ct.c_int, [_VP, _ct.c_int32, _D, _ct.c_double, _ct.c_double, _ct.c_double]),
    "gpe_beta": (_ct.c_int, [_VP, _D]),
    "gpe_loo": (_ct.c_int, [_VP, _ct.c_double, _D, _D, _D]),
    "gpe_posterior": (_ct.c_int, [_VP, _ct.c_int64, _D, _D, _D, _ct.c_double, _ct.c_int32, _ct.c_int32,
                                  _D, _D]),
    "gpe_posterior_grad": (_ct.c_int, [_VP, _ct.c_int64, _D, _D, _D, _ct.POINTER(_ct.c_int32), _D, _ct.c_double,
                                       _D, _D, _D, _D]),
    "gpe_posterior_mean": (_ct.c_int, [_VP, _ct.c_int64, _D, _D, _D, _D]),
    "gpe_set_outputs": (_ct.c_int, [_VP, _ct.c_int32, _D]),
    "gpe_objective_multi": (_ct.c_int, [_VP, _ct.c_int32, _D, _ct.c_int32, _ct.c_double, _ct.c_int32, _D, _D, _D,
                                        _D]),
    "gpe_beta_multi": (_ct.c_int, [_VP, _D]),
    "gpe_posterior_mean_multi": (_ct.c_int, [_VP, _ct.c_int64, _D, _D, _D, _D]),
    "gpe_posterior_groups": (_ct.c_int, [_VP, _ct.c_int64, _ct.c_int32, _D, _D, _D, _ct.c_double, _D, _D]),
    "gpe_noise_sample": (_ct.c_int, [_VP, _ct.c_int64, _D, _D, _D, _ct.c_double, _D, _ct.c_double,
                                     _D, _ct.c_int32, _D, _D, _D]),
    "gpe_posterior_pivchol": (_ct.c_int, [_VP, _ct.c_int64, _D, _D, _D, _ct.c_double, _D, _ct.c_double,
                                          _ct.c_int64, _ct.c_double, _D, _ct.POINTER(_ct.c_int64), _D, _D,
                                          _ct.POINTER(_ct.c_int64)]),
    "gpe_posterior_imse": (_ct.c_int, [_VP, _ct.c_int64, _ct.c_int64, _D, _D, _D, _ct.c_double, _D, _ct.c_double,
                                       _D, _ct.c_int64, _ct.c_double, _D, _ct.POINTER(_ct.c_int64), _D, _D, _D,
                                       _ct.POINTER(_ct.c_int64)]),
    "gpe_hm_destroy": (None, [_VP]),
    "gpe_hm_last_error": (_ct.c_char_p, [_VP]),
    "gpe_hm_add": (_ct.c_int, [_VP, _VP, _ct.c_int32, _ct.POINTER(_ct.c_int32), _ct.c_int32,
                               _ct.POINTER(_ct.c_int32), _D, _D, _ct.c_double]),
    "gpe_hm_count": (_ct.c_int, [_VP]),
    "gpe_hm_implausibility": (_ct.c_int, [_VP, _ct.c_int64, _ct.c_int32, _D, _D, _D, _ct.c_int32, _D, _D, _D]),
    "gpe_hm_add_multi": (_ct.c_int, [_VP, _VP, _ct.c_int32, _ct.POINTER(_ct.c_int32), _ct.c_int32,
                                     _ct.POINTER(_ct.c_int32), _D, _ct.c_int32, _D, _D]),
    "gpe_hm_outputs": (_ct.c_int, [_VP]),
    "gpe_hm_member_outputs": (_ct.c_int, [_VP, _ct.c_int32]),
    "gpe_hm_implausibility_mv": (_ct.c_int, [_VP, _ct.c_int32, _ct.c_int64, _ct.c_int32, _D, _D, _D, _D, _D, _D]),
    "gpe_hm_cells": (_ct.c_int, [_VP, _ct.c_int32, _ct.c_int32, _ct.c_int32, _ct.c_int32, _D, _ct.c_int32, _D,
                                 _ct.c_int64, _D, _ct.POINTER(_ct.c_int32), _D, _D, _ct.c_int32, _ct.c_double, _D,
                                 _ct.POINTER(_ct.c_int64)]),
    "gpe_hm_cells_mv": (_ct.c_int, [_VP, _ct.c_int32, _ct.c_int32, _ct.c_int32, _ct.c_int32, _ct.c_int32, _D,
                                    _ct.c_int32, _D, _ct.c_int64, _D, _D, _D, _ct.c_double, _D,
                                    _ct.POINTER(_ct.c_int64)]),
    "gpe_hm_sample": (_ct.c_int, [_VP, _ct.c_int32, _D, _D, _ct.POINTER(_ct.c_uint64), _ct.POINTER(_ct.c_uint64),
                                  _ct.c_int64, _ct.c_int64, _D, _D, _ct.c_int32, _ct.c_double, _ct.c_int64, _D,
                                  _ct.POINTER(_ct.c_int64), _ct.POINTER(_ct.c_int64)]),
    "gpe_solve": (_ct.c_int, [_VP, _ct.c_int32, _D, _D]),
    "gpe_sense_pairs": (_ct.c_int, [_VP, _ct.c_int32, _D, _D, _ct.c_int32, _D, _D, _D]),
    "gpe_gauss_transform": (_ct.c_int, [_VP, _ct.c_int64, _ct.c_int32, _ct.POINTER(_ct.c_int32), _D, _D, _D,
                                        _D]),
    "gpe_kernel_var": (_ct.c_int, [_VP, _ct.c_int32, _D, _ct.c_int32, _ct.c_double, _ct.c_int32,
                                   _ct.c_int64, _D, _D, _ct.c_double, _D]),
    "gpe_kernel_covar": (_ct.c_int, [_VP, _ct.c_int32, _D, _ct.c_int32, _ct.c_double, _ct.c_int64,
                                     _D, _ct.c_int64, _D, _D]),
    "gpe_kernel_grad": (_ct.c_int, [_VP, _D, _ct.c_int32, _ct.c_int64, _D, _D, _ct.c_double, _ct.c_double, _D]),
    "gpe_kernel_grad_k": (_ct.c_int, [_VP, _ct.c_int32, _D, _ct.c_int32, _ct.c_int64, _D, _D, _ct.c_double,
                                      _ct.c_double, _D]),
    "gpe_lhc_maximin": (_ct.c_int, [_VP, _ct.c_int32, _ct.c_int64, _ct.c_int32, _D, _ct.c_int64, _D,
                                    _ct.POINTER(_ct.c_int64)]),
    "gpe_cholesky": (_ct.c_int, [_VP, _ct.c_int64, _D, _D, _D, _D, _D]),
    "gpe_test_gemm": (_ct.c_int, [_VP, _ct.c_int32, _ct.c_int32, _ct.c_int64, _ct.c_int64,
                                  _ct.c_int64, _D, _D, _D, _ct.c_double, _ct.c_double]),
    "gpe_bench_gemm": (_ct.c_int, [_VP, _ct.c_int32, _ct.c_int32, _ct.c_int32, _ct.c_int32,
                                   _ct.c_int32, _ct.c_int32, _ct.c_double, _ct.c_int32, _D]),
    "gpe_set_profiling": (_ct.c_int, [_VP, _ct.c_int32]),
    "gpe_phase_times": (_ct.c_int, [_VP, _D, _ct.c_int32]),
    "gpe_gemm_stats": (_ct.c_int, [_VP, _D, _D, _D]),
    "gpe_ozaki_stats": (_ct.c_int, [_VP, _D, _D, _D, _D]),
    "gpe_oz_cert_stats": (_ct.c_int, [_VP, _ct.POINTER(_ct.c_int32), _ct.POINTER(_ct.c_int32)]),
    "gpe_oz_cert_sums": (_ct.c_int, [_VP, _ct.c_int32, _ct.POINTER(_ct.c_uint64), _ct.POINTER(_ct.c_uint64)]),
    # include/gpemu_dist.h: row-block distributed value objective (RCCL / loopback)
    "gpe_dist_unique_id": (_ct.c_int, [_ct.c_char_p, _ct.c_int32]),
    "gpe_dist_create": (_VP, [_ct.c_int32, _ct.c_int32, _ct.c_int32, _ct.c_char_p]),
    "gpe_dist_destroy": (None, [_VP]),
    "gpe_dist_last_error": (_ct.c_char_p, [_VP]),
    "gpe_dist_set_data": (_ct.c_int, [_VP, _ct.c_int64, _ct.c_int32, _ct.c_int32, _D, _D, _D, _D]),
    "gpe_dist_objective": (_ct.c_int, [_VP, _ct.c_int32, _ct.c_int32, _D, _ct.c_int32, _ct.c_double,
                                       _ct.c_int32, _D, _D, _D]),
    "gpe_dist_owner": (_ct.c_int32, [_ct.c_int32, _ct.c_int32]),
    "gpe_dist_local_rows": (_ct.c_int32, [_ct.c_int64, _ct.c_int32, _ct.c_int32, _ct.c_int32]),
    "gpe_dist_times": (_ct.c_int, [_VP, _D, _D]),
    "gpe_dist_rank_bytes": (_ct.c_int, [_VP, _ct.c_int32, _ct.POINTER(_ct.c_int64)]),
}

# constructors that return a handle type of their own (SIGNATURES lists the entries whose
# return type is int, void, const char* or one of the two context handles)
HANDLE_SIGNATURES = {
    "gpe_hm_create": (_VP, [_ct.c_int32]),
}

UNIQUE_ID_BYTES = 128


class NativeUnavailable(RuntimeError):
    """libgpemu.so is missing or no HIP device is visible (no CPU fallback)."""


class NotPositiveDefinite(ArithmeticError):
    """Cholesky met a non-positive / NaN pivot (the reference's LinAlgError)."""


_lib = None
_lib_lock = _threading.Lock()


def load_library(path: str | None = None):
    """Load and type the shared library (idempotent)."""
    global _lib
    with _lib_lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not _os.path.exists(p):
            raise NativeUnavailable(
                f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = _ct.CDLL(p)
        for name, (res, args) in list(SIGNATURES.items()) + list(HANDLE_SIGNATURES.items()):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        # provenance: the in-tree library must be built from the sources beside it (a
        # probe build named by GPEMU_LIB or `path` is the caller's choice)
        from . import buildinfo
        want = buildinfo.source_hash() if p == _DEFAULT_LIB else None
        have = lib.gpe_build_id().decode()
        if want is not None and have != want:
            raise NativeUnavailable(
                f"{p} was built from other sources (build id {have[:12]}, sources {want[:12]}): "
                "rebuild it with `python -c 'import __graft_entry__ as g; g.build()'`")
        if path is None:
            _lib = lib
        return lib


def build_id() -> str:
    """SHA-256 of the sources the loaded library was built from."""
    return load_library().gpe_build_id().decode()


def _ptr(a):
    if a is None:
        return None
    return a.ctypes.data_as(_D)


def _f64(a, shape=None):
    arr = _np.ascontiguousarray(a, dtype=_np.float64)
    if shape is not None:
        arr = arr.reshape(shape)
    return arr


class Context:
    """One GPU, one HIP stream, resident training data (gpe_ctx)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        if self.lib.gpe_device_count() <= 0:
            raise NativeUnavailable("no HIP device visible to libgpemu.so")
        h = self.lib.gpe_create(int(device))
        if not h:
            raise NativeUnavailable("gpe_create failed: " + self.lib.gpe_last_error(None).decode())
        self._h = h
        self.device = device
        self.n = self.d = self.q = 0
        self.p = 0                         # outputs of set_outputs (0: none)
        self._data_key = None
        self._out_key = None
        self._factor_key = None

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None):
            self.lib.gpe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc == GPE_OK:
            return
        msg = self.lib.gpe_last_error(self._h).decode()
        if rc == GPE_NOT_PD:
            raise NotPositiveDefinite(f"{what}: {msg}")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")

    # -- data
    def set_data(self, X, f, H, r=None):
        X = _f64(X)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        n, d = X.shape
        f = _f64(f, (n,))
        H = _f64(H)
        if H.ndim == 1:
            H = H.reshape(n, -1)
        q = H.shape[1]
        rr = None if r is None or _np.isscalar(r) else _f64(r, (n,))
        self._keep = (X, f, H, rr)
        self._data_key = None
        self._factor_key = None
        self._out_key = None               # (gpe_set_data drops the outputs)
        self.p = 0
        self._check(self.lib.gpe_set_data(self._h, n, d, q, _ptr(X), _ptr(f), _ptr(H), _ptr(rr)),
                    "gpe_set_data")
        self.n, self.d, self.q = n, d, q

    @staticmethod
    def _digest(*arrays):
        h = _hashlib.blake2b(digest_size=16)
        for a in arrays:
            if a is None:
                h.update(b"-")
            else:
                a = _np.ascontiguousarray(a, dtype=_np.float64)
                h.update(str(a.shape).encode())
                h.update(a.tobytes())
        return h.hexdigest()

    def ensure_data(self, X, f, H, r=None):
        """set_data unless this exact (X, f, H, r) is already resident."""
        key = self._digest(X, f, H, r)
        if key != self._data_key:
            self.set_data(X, f, H, r)
            self._data_key = key

    def ensure_factor(self, kernel, delta, nu, s2=1.0, r_scale=0.0):
        """factor() unless the same factor of the resident data is already held."""
        key = (int(kernel), tuple(_np.asarray(delta, float).ravel().tolist()), float(nu), float(s2),
               float(r_scale), self._data_key)
        if key != self._factor_key or self._data_key is None:
            self._factor_key = None
            self.factor(kernel, delta, nu, s2, r_scale)
            self._factor_key = key

    # -- p outputs sharing one correlation matrix (the separable multi-output emulator)
    def set_outputs(self, F):
        """The outputs F (n x p, 1 <= p <= 64) of the resident data (gpe_set_outputs); the
        data's own f, its digest and the resident factor stay as they are."""
        F = _f64(F)
        if F.ndim == 1:
            F = F.reshape(-1, 1)
        if self.n and F.shape[0] != self.n:   # (without data the library answers GPE_ERR_STATE)
            raise ValueError("set_outputs: F must have one row per training point")
        self._out_key = None
        self.p = 0
        self._check(self.lib.gpe_set_outputs(self._h, F.shape[1], _ptr(F)), "gpe_set_outputs")
        self.p = F.shape[1]

    def ensure_outputs(self, F):
        """set_outputs unless this exact F is already resident for the resident data."""
        key = (self._digest(F), self._data_key)
        if key != self._out_key or self._data_key is None:
            self.set_outputs(F)
            self._out_key = key

    def objective_multi(self, kernel, hp, nu_fixed=0.0, want_grad=True):
        """(llh, grad or None, Sigma (p x p), B (q x p)) of the multi-output objective
        (gpe_objective_multi; hp = [delta, nu if fitted]); raises NotPositiveDefinite."""
        hp = _f64(hp).ravel()
        llh = _ct.c_double(0.0)
        grad = _np.zeros(hp.size) if want_grad else None
        Sigma = _np.zeros((max(self.p, 1), max(self.p, 1)))
        B = _np.zeros((self.q, max(self.p, 1)))
        self._factor_key = None            # the objective reuses the factor buffers
        rc = self.lib.gpe_objective_multi(self._h, int(kernel), _ptr(hp), hp.size, float(nu_fixed),
                                          1 if want_grad else 0, _ct.byref(llh), _ptr(grad), _ptr(Sigma), _ptr(B))
        self._check(rc, "gpe_objective_multi")
        return llh.value, grad, Sigma, B

    def beta_multi(self):
        """B (q x p) of the resident factor and outputs (gpe_beta_multi)."""
        out = _np.zeros((self.q, max(self.p, 1)))
        self._check(self.lib.gpe_beta_multi(self._h, _ptr(out)), "gpe_beta_multi")
        return out

    def posterior_mean_multi(self, Xs, Hs, B):
        """The posterior means of the p outputs at Xs (m x p; gpe_posterior_mean_multi): one fused
        kernel forms every correlation once for all p outputs; any m, the result does not
        depend on the chunk length."""
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = Xs.reshape(-1, 1)
        m = Xs.shape[0]
        Hs = _f64(Hs, (m, self.q))
        B = _f64(B, (self.q, max(self.p, 1)))
        mean = _np.zeros((m, max(self.p, 1)))
        self._check(self.lib.gpe_posterior_mean_multi(self._h, m, _ptr(Xs), _ptr(Hs), _ptr(B), _ptr(mean)),
                    "gpe_posterior_mean_multi")
        return mean

    # -- objective
    def objective(self, variant, kernel, hp, nu_fixed=0.0, want_grad=True):
        """Returns (llh, grad or None, sigma2); raises NotPositiveDefinite."""
        hp = _f64(hp).ravel()
        llh = _ct.c_double(0.0)
        s2 = _ct.c_double(0.0)
        grad = _np.zeros(hp.size) if want_grad else None
        self._factor_key = None            # the objective reuses the factor buffers
        rc = self.lib.gpe_objective(self._h, int(variant), int(kernel), _ptr(hp), hp.size,
                                    float(nu_fixed), 1 if want_grad else 0, _ct.byref(llh),
                                    _ptr(grad), _ct.byref(s2))
        self._check(rc, "gpe_objective")
        return llh.value, grad, s2.value

    def factor(self, kernel, delta, nu, s2=1.0, r_scale=0.0):
        self._factor_key = None
        delta = _f64(delta).ravel()
        self._check(self.lib.gpe_factor(self._h, int(kernel), _ptr(delta), float(nu), float(s2),
                                        float(r_scale)), "gpe_factor")

    def beta(self):
        out = _np.zeros(self.q)
        self._check(self.lib.gpe_beta(self._h, _ptr(out)), "gpe_beta")
        return out

    def loo(self, sigma):
        """Leave-one-out (mean, var, beta) of the resident factor: the posterior at every
        training point given the other n - 1, hyperparameters fixed and beta re-estimated
        without the point; beta is the GLS beta of all n points."""
        mean = _np.zeros(self.n)
        var = _np.zeros(self.n)
        beta = _np.zeros(self.q)
        self._check(self.lib.gpe_loo(self._h, float(sigma), _ptr(mean), _ptr(var), _ptr(beta)), "gpe_loo")
        return mean, var, beta

    def posterior(self, Xs, Hs, beta, sigma, full_var=True, precision=64):
        """(mean, var): var is m x m when full_var, else its diagonal.  The L^-1 K* product
        runs as exact int8 products (4096 <= n_pad <= 32768): of 53-bit operands at precision
        64, of 24-bit ones at precision=32 (diagonal variance only; fp32 MFMA outside that
        range or with GPEMU_OZAKI=0)."""
        if precision not in (32, 64):
            raise ValueError("precision must be 32 or 64")
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = Xs.reshape(-1, 1)
        m = Xs.shape[0]
        Hs = _f64(Hs, (m, self.q))
        beta = _f64(beta).ravel()
        mean = _np.zeros(m)
        var = _np.zeros((m, m)) if full_var else _np.zeros(m)
        self._check(self.lib.gpe_posterior(self._h, m, _ptr(Xs), _ptr(Hs), _ptr(beta), float(sigma),
                                           1 if full_var else 0, int(precision), _ptr(mean), _ptr(var)),
                    "gpe_posterior")
        return mean, var

    def posterior_grad(self, Xs, Hs, dHs, hdim, beta, sigma, want_var=True):
        """(mean, var, dmean, dvar): the posterior mean and diagonal variance at Xs, bit for bit
        those of posterior(full_var=False), and their gradients in the point (m x d each, in
        the coordinates of Xs).  dHs (m x q) is each basis column's derivative in its own
        input hdim[j] (-1: a constant column).  want_var=False skips the variance gradient's
        n^2 m product; dvar is then None."""
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = Xs.reshape(-1, 1)
        m = Xs.shape[0]
        Hs = _f64(Hs, (m, self.q))
        dHs = _f64(dHs, (m, self.q))
        hdim = _np.ascontiguousarray(hdim, dtype=_np.int32).reshape(self.q)
        beta = _f64(beta).ravel()
        mean = _np.zeros(m)
        var = _np.zeros(m)
        dmean = _np.zeros((m, self.d))
        dvar = _np.zeros((m, self.d)) if want_var else None
        self._check(self.lib.gpe_posterior_grad(self._h, m, _ptr(Xs), _ptr(Hs), _ptr(dHs),
                                                hdim.ctypes.data_as(_ct.POINTER(_ct.c_int32)), _ptr(beta),
                                                float(sigma), _ptr(mean), _ptr(var), _ptr(dmean), _ptr(dvar)),
                    "gpe_posterior_grad")
        return mean, var, dmean, dvar

    def posterior_mean(self, Xs, Hs, beta):
        """The posterior mean alone at Xs (gpe_posterior_mean): hs . beta + sum_i gamma_i K*_i from
        one fused kernel, without K*, L^-1 K* or the variance.  It agrees with posterior()'s
        mean to the rounding of an n-term sum (same gamma, same terms, another summation
        order) and does not depend on the chunk length; any m."""
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = Xs.reshape(-1, 1)
        m = Xs.shape[0]
        Hs = _f64(Hs, (m, self.q))
        beta = _f64(beta).ravel()
        mean = _np.zeros(m)
        self._check(self.lib.gpe_posterior_mean(self._h, m, _ptr(Xs), _ptr(Hs), _ptr(beta), _ptr(mean)),
                    "gpe_posterior_mean")
        return mean

    def posterior_groups(self, Xs, Hs, beta, sigma, group):
        """(mean (m), cov (m // group, group, group)): the posterior covariance inside groups of
        `group` consecutive points (gpe_posterior_groups), the block diagonal of
        posterior(full_var=True)'s matrix without its other entries; any m that is a multiple
        of group, 1 <= group <= 64.  Blocks are exactly symmetric, a group's block does not
        depend on the other groups, and repeated calls return the same bits."""
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = Xs.reshape(-1, 1)
        m = Xs.shape[0]
        group = int(group)
        Hs = _f64(Hs, (m, self.q))
        beta = _f64(beta).ravel()
        mean = _np.zeros(m)
        ng = m // group if group >= 1 and m % group == 0 else 0   # (the library rejects the rest)
        cov = _np.zeros((ng, max(group, 0), max(group, 0)))
        self._check(self.lib.gpe_posterior_groups(self._h, m, group, _ptr(Xs), _ptr(Hs), _ptr(beta), float(sigma),
                                                  _ptr(mean), _ptr(cov)), "gpe_posterior_groups")
        return mean, cov

    def noise_sample(self, Xs, Hs, beta, sigma, t, U, r_new=None, r_scale=0.0):
        """noise_fit's estimation step for the resident factor: the posterior at Xs
        (full covariance V, plus r_scale * r_new on its diagonal), L = chol(V) and
        sum_j 0.5 (t - mean - L U[j])^2 over the rows of U (s x m).  Returns
        (mean, that sum).  NotPositiveDefinite when V is not."""
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = Xs.reshape(-1, 1)
        m = Xs.shape[0]
        Hs = _f64(Hs, (m, self.q))
        beta = _f64(beta).ravel()
        t = _f64(t, (m,))
        U = _f64(U)
        U = U.reshape(-1, m)
        rn = None if r_new is None else _f64(r_new, (m,))
        mean = _np.zeros(m)
        z = _np.zeros(m)
        self._check(self.lib.gpe_noise_sample(self._h, m, _ptr(Xs), _ptr(Hs), _ptr(beta), float(sigma),
                                              _ptr(rn), float(r_scale), _ptr(t), U.shape[0], _ptr(U),
                                              _ptr(mean), _ptr(z)), "gpe_noise_sample")
        return mean, z

    def posterior_pivchol(self, Xs, Hs, beta, sigma, k=None, tol=0.0, r_new=None, r_scale=0.0, want_L=True):
        """Greedy pivoted Cholesky of the posterior covariance at Xs (plus sigma^2 r_scale r_new
        on its diagonal) for the resident factor: up to k steps (None: all m), each taking the
        point with the largest remaining conditional variance, stopping once that is
        <= tol * the largest prior one.  Returns (mean, piv, pivvar, L, rank) trimmed to rank:
        piv (rank,) the points in the order chosen, pivvar their conditional variances, L
        (m x rank, None without want_L) in the original point order.  At most 16384 points."""
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = Xs.reshape(-1, 1)
        m = Xs.shape[0]
        k = m if k is None else int(k)
        Hs = _f64(Hs, (m, self.q))
        beta = _f64(beta).ravel()
        rn = None if r_new is None else _f64(r_new, (m,))
        kk = max(k, 1)
        mean = _np.zeros(m)
        piv = _np.zeros(kk, dtype=_np.int64)
        pivvar = _np.zeros(kk)
        # (not allocated for a call the library refuses)
        L = _np.zeros((m, kk)) if want_L and 1 <= k <= m <= 16384 else None
        rank = _ct.c_int64(0)
        self._check(self.lib.gpe_posterior_pivchol(self._h, m, _ptr(Xs), _ptr(Hs), _ptr(beta), float(sigma),
                                                   _ptr(rn), float(r_scale), k, float(tol), _ptr(mean),
                                                   piv.ctypes.data_as(_ct.POINTER(_ct.c_int64)), _ptr(pivvar),
                                                   _ptr(L), _ct.byref(rank)), "gpe_posterior_pivchol")
        r = int(rank.value)
        return mean, piv[:r].copy(), pivvar[:r].copy(), (L[:, :r].copy() if L is not None else None), r

    def posterior_imse(self, Xs, Hs, beta, sigma, mc, k, w=None, tol=1e-8, r_new=None, r_scale=0.0):
        """Greedy integrated-variance (IMSE) batch for the resident factor: the first mc rows of
        Xs are candidates, the rest a reference sample with weights w (None: equal).  Up to k
        picks, each the candidate whose run most reduces the w-weighted posterior variance of
        the reference points given the picks before it; a candidate whose remaining variance
        is <= tol * the largest initial one is no longer eligible.  Returns
        (mean, piv, gain, pivvar, imse0, rank) trimmed to rank: piv (rank,) the candidates in the
        order chosen, gain the reduction each bought, pivvar their conditional variances, imse0
        the weighted variance before any pick.  At most 16384 points in all."""
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = Xs.reshape(-1, 1)
        m = Xs.shape[0]
        mc, k = int(mc), int(k)
        Hs = _f64(Hs, (m, self.q))
        beta = _f64(beta).ravel()
        rn = None if r_new is None else _f64(r_new, (m,))
        wv = None if w is None else _f64(w, (max(m - mc, 0),))
        kk = max(k, 1)
        mean = _np.zeros(m)
        piv = _np.zeros(kk, dtype=_np.int64)
        gain = _np.zeros(kk)
        pivvar = _np.zeros(kk)
        imse0 = _ct.c_double(0.0)
        rank = _ct.c_int64(0)
        self._check(self.lib.gpe_posterior_imse(self._h, m, mc, _ptr(Xs), _ptr(Hs), _ptr(beta), float(sigma),
                                                _ptr(rn), float(r_scale), _ptr(wv), k, float(tol), _ptr(mean),
                                                piv.ctypes.data_as(_ct.POINTER(_ct.c_int64)), _ptr(gain),
                                                _ptr(pivvar), _ct.byref(imse0), _ct.byref(rank)),
                    "gpe_posterior_imse")
        r = int(rank.value)
        return mean, piv[:r].copy(), gain[:r].copy(), pivvar[:r].copy(), float(imse0.value), r

    # -- sensitivity building blocks (resident factor)
    def solve(self, B):
        """A^-1 B for the resident factor (B: n or n x k)."""
        B = _f64(B)
        vec = B.ndim == 1
        B2 = B.reshape(self.n, -1)
        B2 = _np.ascontiguousarray(B2)
        X = _np.zeros_like(B2)
        self._check(self.lib.gpe_solve(self._h, B2.shape[1], _ptr(B2), _ptr(X)), "gpe_solve")
        return X.ravel() if vec else X

    def sense_pairs(self, w, u, Z):
        """For K_j(k,l) = u[j,k] u[j,l] exp(-sum_i w[j,i] (x_ki - x_li)^2):
        (tr(A^-1 K_j) for each j, Z^T K_j Z for each j)."""
        w = _np.ascontiguousarray(_f64(w).reshape(-1, self.d))
        J = w.shape[0]
        u = _np.ascontiguousarray(_f64(u).reshape(J, self.n))
        Z = _np.ascontiguousarray(_f64(Z).reshape(self.n, -1))
        p = Z.shape[1]
        tr = _np.zeros(J)
        quad = _np.zeros((J, p, p))
        self._check(self.lib.gpe_sense_pairs(self._h, J, _ptr(w), _ptr(u), p, _ptr(Z), _ptr(tr), _ptr(quad)),
                    "gpe_sense_pairs")
        return tr, quad

    def gauss_transform(self, dims, c, Y, a):
        """out[t] = sum_k a[k] exp(-sum_s c[s] (Y[t,s] - x[k, dims[s]])^2)."""
        dims_a = _np.ascontiguousarray(_np.asarray(dims, dtype=_np.int32).ravel())
        ns = dims_a.size
        c = _np.ascontiguousarray(_f64(c).ravel())
        Y = _np.ascontiguousarray(_f64(Y).reshape(-1, ns))
        a = _np.ascontiguousarray(_f64(a).ravel())
        if a.size != self.n or c.size != ns:
            raise ValueError("gauss_transform: a must have n entries and c one per dimension")
        out = _np.zeros(Y.shape[0])
        self._check(self.lib.gpe_gauss_transform(self._h, Y.shape[0], ns,
                                                 dims_a.ctypes.data_as(_ct.POINTER(_ct.c_int32)), _ptr(c),
                                                 _ptr(Y), _ptr(a), _ptr(out)), "gpe_gauss_transform")
        return out

    def kernel_var(self, kernel, delta, nu, X, predict=True, r=None, r_scale=0.0):
        X = _f64(X)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        m, d = X.shape
        delta = _f64(delta).ravel()
        rr = None if r is None or _np.isscalar(r) else _f64(r, (m,))
        out = _np.zeros((m, m))
        self._check(self.lib.gpe_kernel_var(self._h, int(kernel), _ptr(delta), d, float(nu),
                                            1 if predict else 0, m, _ptr(X), _ptr(rr),
                                            float(r_scale), _ptr(out)), "gpe_kernel_var")
        return out

    def kernel_covar(self, kernel, delta, nu, XT, XV):
        XT = _f64(XT)
        XV = _f64(XV)
        if XT.ndim == 1:
            XT = XT.reshape(-1, 1)
        if XV.ndim == 1:
            XV = XV.reshape(-1, 1)
        n, d = XT.shape
        m = XV.shape[0]
        delta = _f64(delta).ravel()
        out = _np.zeros((n, m))
        self._check(self.lib.gpe_kernel_covar(self._h, int(kernel), _ptr(delta), d, float(nu), n,
                                              _ptr(XT), m, _ptr(XV), _ptr(out)), "gpe_kernel_covar")
        return out

    def kernel_grad(self, delta, X, col, col_scale, pre):
        """pre * ((col_k - col_l) col_scale)^2 * exp(-|(x_k - x_l)/delta|^2), zero
        diagonal (col None: no squared factor); m x m."""
        X = _f64(X)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        m, d = X.shape
        delta = _f64(delta).ravel()
        cc = None if col is None else _f64(col, (m,))
        out = _np.zeros((m, m))
        self._check(self.lib.gpe_kernel_grad(self._h, _ptr(delta), d, m, _ptr(X), _ptr(cc),
                                             float(col_scale), float(pre), _ptr(out)), "gpe_kernel_grad")
        return out

    def kernel_grad_k(self, kernel, delta, X, col, col_scale, pre):
        """kernel_grad for the correlation family of `kernel`: pre * ((col_k - col_l)
        col_scale)^2 * g(s) with the family's derivative factor g, or pre * rho(s) without
        col; zero diagonal, m x m."""
        X = _f64(X)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        m, d = X.shape
        delta = _f64(delta).ravel()
        cc = None if col is None else _f64(col, (m,))
        out = _np.zeros((m, m))
        self._check(self.lib.gpe_kernel_grad_k(self._h, int(kernel), _ptr(delta), d, m, _ptr(X), _ptr(cc),
                                               float(col_scale), float(pre), _ptr(out)), "gpe_kernel_grad_k")
        return out

    def lhc_maximin(self, designs, fextra=None):
        """np.argmin(pdist([designs[k]; fextra], 'sqeuclidean')) for every candidate
        design k (designs: N x n x dim) -> int64 array of N condensed indices."""
        designs = _f64(designs)
        N, n, dim = designs.shape
        fe = None if fextra is None else _f64(fextra).reshape(-1, dim)
        ne = 0 if fe is None else fe.shape[0]
        out = _np.zeros(N, dtype=_np.int64)
        self._check(self.lib.gpe_lhc_maximin(self._h, N, n, dim, _ptr(designs), ne, _ptr(fe),
                                             out.ctypes.data_as(_ct.POINTER(_ct.c_int64))), "gpe_lhc_maximin")
        return out

    def cholesky(self, A, want=("L",)):
        A = _f64(A)
        m = A.shape[0]
        outs = {k: _np.zeros((m, m)) for k in want if k in ("L", "Linv", "Ainv")}
        ld = _ct.c_double(0.0)
        self._check(self.lib.gpe_cholesky(self._h, m, _ptr(A), _ptr(outs.get("L")),
                                          _ptr(outs.get("Linv")), _ptr(outs.get("Ainv")),
                                          _ct.byref(ld)), "gpe_cholesky")
        outs["logdet"] = ld.value
        return outs

    def test_gemm(self, A, B, C, alpha=1.0, beta=0.0, trans_a=0, trans_b=0):
        A = _f64(A)
        B = _f64(B)
        C = _f64(C).copy()
        M, K = A.shape
        N = B.shape[1]
        self._check(self.lib.gpe_test_gemm(self._h, int(trans_a), int(trans_b), M, N, K, _ptr(A),
                                           _ptr(B), _ptr(C), float(alpha), float(beta)),
                    "gpe_test_gemm")
        return C

    def test_oz_product(self, a, b=None, *, C, ldc, packed=False, K=0, kbeg=0, kend=0, kdiv=1, ti0=0,
                        tri=False, lower128=False, alpha=1.0, acc=False, nmod=16, rows=0, cols=0,
                        res_mod=None, cert=False):
        """One exact int8 product through the production kernels (gpe_test_oz_product, a test
        hook).  a, b: dicts with src (1-d fp64 array, sent as it is), ld and optionally offset,
        trans, R, Kv, mask; b None: B is A.  C: 1-d fp64 array, the column-major output with
        leading dimension ldc (copied, read when acc).  Returns dict(C, exa, exb, res): the
        new C, the row exponents of both operands (padded to 256) and, with res_mod, the
        centred residues of that modulus as int8 (padded rows from tile row ti0 x padded
        columns).  cert: through gpe_test_oz_product_cert, the same product with a 15-moduli
        certificate; the dict then also holds nmod_used (15 certified, 16 refused)."""
        keep = []

        def opnd(o):
            src = _np.ascontiguousarray(o["src"], dtype=_np.float64).ravel()
            keep.append(src)
            return OzOperand(_ptr(src), src.size, int(o.get("offset", 0)), int(o["ld"]), int(o.get("trans", 0)),
                             int(o.get("R", 0)), int(o.get("Kv", 0)), int(o.get("mask", 0)))

        oa = opnd(a)
        ob = opnd(b) if b is not None else None
        pad = lambda r: (r + 255) // 256 * 256
        Pa = pad(oa.R)
        Pb = pad(ob.R) if ob is not None else Pa
        Cc = _np.array(C, dtype=_np.float64).ravel()
        p = OzParams(int(bool(packed)), int(K), int(kbeg), int(kend), int(kdiv), int(ti0), int(bool(tri)),
                     int(bool(lower128)), int(bool(acc)), int(nmod), int(rows), int(cols),
                     -1 if res_mod is None else int(res_mod), int(ldc), Cc.size, float(alpha))
        exa = _np.zeros(max(Pa, 1), dtype=_np.int32)
        exb = _np.zeros(max(Pb, 1), dtype=_np.int32)
        res = None if res_mod is None else _np.zeros((max(Pa - 256 * int(ti0), 1), max(Pb, 1)), dtype=_np.int8)
        i32 = _ct.POINTER(_ct.c_int32)
        args = (self._h, _ct.byref(oa), _ct.byref(ob) if ob is not None else None, _ct.byref(p), _ptr(Cc),
                exa.ctypes.data_as(i32), exb.ctypes.data_as(i32),
                None if res is None else res.ctypes.data_as(_ct.POINTER(_ct.c_int8)))
        if cert:
            used = _ct.c_int32(0)
            self._check(self.lib.gpe_test_oz_product_cert(*args, _ct.byref(used)), "gpe_test_oz_product_cert")
            return {"C": Cc, "exa": exa, "exb": exb, "res": res, "nmod_used": used.value}
        self._check(self.lib.gpe_test_oz_product(*args), "gpe_test_oz_product")
        return {"C": Cc, "exa": exa, "exb": exb, "res": res}

    def test_oz_planes(self, a, *, packed=False, K=0, nmod=16):
        """One operand through the production conversion (gpe_test_oz_planes, a test hook).
        a: as test_oz_product's.  Returns dict(ex, planes): the exponents of the rows padded to
        P = 256 ceil(R / 256) and the int8 planes, nmod x P x K (packed: nmod x P x P, row j the
        column j of X, zero above its 256-row panel)."""
        src = _np.ascontiguousarray(a["src"], dtype=_np.float64).ravel()
        oa = OzOperand(_ptr(src), src.size, int(a.get("offset", 0)), int(a["ld"]), int(a.get("trans", 0)),
                       int(a.get("R", 0)), int(a.get("Kv", 0)), int(a.get("mask", 0)))
        P = (oa.R + 255) // 256 * 256
        ex = _np.zeros(max(P, 1), dtype=_np.int32)
        planes = _np.zeros((int(nmod), max(P, 1), max(P if packed else int(K), 1)), dtype=_np.int8)
        self._check(self.lib.gpe_test_oz_planes(
            self._h, _ct.byref(oa), int(bool(packed)), int(K), int(nmod), ex.ctypes.data_as(_ct.POINTER(_ct.c_int32)),
            planes.ctypes.data_as(_ct.POINTER(_ct.c_int8))), "gpe_test_oz_planes")
        return {"ex": ex, "planes": planes}

    def test_gemm_group(self, bufs, probs, *, kind, split=False, listed=False, reps=1):
        """One launch of the grouped fp64 GEMM on a group of problems through the production
        routines (gpe_test_gemm_group, a test hook).  bufs: 1-d fp64 arrays, sent as they are
        (copied here).  probs: dicts with a, b, c = (buffer index, element offset, leading
        dimension), mt, nt, K and optionally flags, kti_mul, kti_off, alpha, beta.  Returns
        dict(bufs, ksplit, listed, cdef, workgroups, tiles): the buffers afterwards, the split
        each problem got, whether the launch had a tile list and ran the CDEF instance, its
        workgroup count and the tile list (codes p << 24 | ti << 12 | tj; None without one)."""
        out = [_np.array(b, dtype=_np.float64).ravel() for b in bufs]
        ptrs = (_D * len(out))(*[_ptr(b) for b in out])
        lens = (_ct.c_int64 * len(out))(*[b.size for b in out])
        ps = (GemmGroupProb * max(len(probs), 1))()
        cap = 0
        for q, p in zip(ps, probs):
            (q.a_buf, q.a_off, q.lda), (q.b_buf, q.b_off, q.ldb), (q.c_buf, q.c_off, q.ldc) = \
                [tuple(int(v) for v in p[k]) for k in ("a", "b", "c")]
            q.mt, q.nt, q.K, q.flags = int(p["mt"]), int(p["nt"]), int(p["K"]), int(p.get("flags", 0))
            q.kti_mul, q.kti_off = int(p.get("kti_mul", 1)), int(p.get("kti_off", 0))
            q.alpha, q.beta = float(p.get("alpha", 1.0)), float(p.get("beta", 0.0))
            if 0 < q.mt <= 4096 and 0 < q.nt <= 4096:
                cap += q.mt * (q.mt + 1) // 2 if q.flags & G_CLOWER else q.mt * q.nt
        gl = GemmGroupLaunch(int(kind), int(split), int(listed), int(reps))
        ksplit = _np.zeros(max(len(probs), 1), dtype=_np.int32)
        info = _np.zeros(3, dtype=_np.int32)
        tiles = _np.zeros(max(cap, 1), dtype=_np.uint32)
        i32 = _ct.POINTER(_ct.c_int32)
        self._check(self.lib.gpe_test_gemm_group(
            self._h, len(out), ptrs, lens, len(probs), ps, _ct.byref(gl), ksplit.ctypes.data_as(i32),
            info.ctypes.data_as(i32), tiles.ctypes.data_as(_ct.POINTER(_ct.c_uint32)), cap), "gpe_test_gemm_group")
        return {"bufs": out, "ksplit": ksplit[:len(probs)], "listed": bool(info[0]), "cdef": bool(info[1]),
                "workgroups": int(info[2]), "tiles": tiles[:cap].copy() if info[0] else None}

    def bench_gemm(self, mt, nt, K, trans_a=0, trans_b=0, lower=False, beta=1.0, reps=5):
        ms = _ct.c_double()
        self._check(self.lib.gpe_bench_gemm(self._h, int(trans_a), int(trans_b), int(mt), int(nt),
                                            int(K), 1 if lower else 0, float(beta), int(reps),
                                            _ct.byref(ms)), "gpe_bench_gemm")
        return ms.value

    # -- profiling
    def set_profiling(self, on=True):
        self._check(self.lib.gpe_set_profiling(self._h, 1 if on else 0), "gpe_set_profiling")

    def phase_times(self):
        out = _np.zeros(8)
        self._check(self.lib.gpe_phase_times(self._h, _ptr(out), 8), "gpe_phase_times")
        keys = ["kbuild", "cholesky", "trtri", "inverse", "skinny", "contract", "total"]
        return dict(zip(keys, out[:7].tolist()))

    def gemm_stats(self):
        ms, nl, fl = _ct.c_double(), _ct.c_double(), _ct.c_double()
        self._check(self.lib.gpe_gemm_stats(self._h, _ct.byref(ms), _ct.byref(nl), _ct.byref(fl)),
                    "gpe_gemm_stats")
        return {"ms": ms.value, "launches": nl.value, "flops": fl.value}

    def ozaki_stats(self):
        """k_oz_gemm launches of the most recent objective (profiling on): ms, launches,
        int8 ops and the fp64 flops of the products they emulate."""
        ms, nl, ops, fl = _ct.c_double(), _ct.c_double(), _ct.c_double(), _ct.c_double()
        self._check(self.lib.gpe_ozaki_stats(self._h, _ct.byref(ms), _ct.byref(nl), _ct.byref(ops), _ct.byref(fl)),
                    "gpe_ozaki_stats")
        return {"ms": ms.value, "launches": nl.value, "int8_ops": ops.value, "fp64_flops": fl.value}

    def oz_cert_stats(self):
        """The 15-moduli certificates of the most recent objective's int8 products: how many
        products carried one and how many were certified (gpe_oz_cert_stats)."""
        n, k = _ct.c_int32(0), _ct.c_int32(0)
        self._check(self.lib.gpe_oz_cert_stats(self._h, _ct.byref(n), _ct.byref(k)), "gpe_oz_cert_stats")
        return {"products": n.value, "certified": k.value}

    def oz_cert_sums(self):
        """(A, B) = (max s_a, max s_b) of each of those products, in launch order, as Python ints
        (gpe_oz_cert_sums, a debug read-back); certified iff A B < T15."""
        n = self.oz_cert_stats()["products"]
        a, b = _np.zeros(max(n, 1), dtype=_np.uint64), _np.zeros(max(n, 1), dtype=_np.uint64)
        u64 = _ct.POINTER(_ct.c_uint64)
        self._check(self.lib.gpe_oz_cert_sums(self._h, n, a.ctypes.data_as(u64), b.ctypes.data_as(u64)),
                    "gpe_oz_cert_sums")
        return [(int(a[i]), int(b[i])) for i in range(n)]


_default_ctx = None
_ctx_lock = _threading.Lock()


_tls = _threading.local()
_extra_ctxs: list = []


class EmulatorSet:
    """Emulators resident on one GPU together for history matching (gpe_hm).  ``add`` snapshots
    a context's resident factor; ``implausibility`` runs candidates through every emulator of
    the set, one fused kernel per emulator and chunk, without forming K* or L^-1 K*."""

    MAX_N, MAX_D, MAX_Q, MAX_EMUL = 512, 32, 16, 32

    def __init__(self, device: int = 0):
        self.lib = load_library()
        if self.lib.gpe_device_count() <= 0:
            raise NativeUnavailable("no HIP device visible to libgpemu.so")
        h = self.lib.gpe_hm_create(int(device))
        if not h:
            raise NativeUnavailable("gpe_hm_create failed: " + self.lib.gpe_hm_last_error(None).decode())
        self._h = h
        self.device = device
        self._maxact = -1

    def close(self):
        if getattr(self, "_h", None):
            self.lib.gpe_hm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self.lib.gpe_hm_count(self._h))

    def _check(self, rc, what):
        if rc == GPE_OK:
            return
        msg = self.lib.gpe_hm_last_error(self._h).decode()
        if rc == GPE_NOT_PD:
            raise NotPositiveDefinite(f"{what}: {msg}")
        err = RuntimeError(f"{what} failed ({rc}): {msg}")
        err.status = rc
        raise err

    def add(self, ctx, active, hdim, hval, beta, sigma):
        """Snapshot ctx's resident factor as the next emulator; returns its number.  active:
        the columns of the candidate rows it reads, in the order of its inputs; basis column j
        is the constant hval[j] where hdim[j] == -1, else the emulator's input hdim[j]."""
        i32 = _ct.POINTER(_ct.c_int32)
        active = _np.ascontiguousarray(active, dtype=_np.int32).ravel()
        hdim = _np.ascontiguousarray(hdim, dtype=_np.int32).ravel()
        hval = _f64(hval).ravel()
        beta = _f64(beta).ravel()
        if not (hdim.size == hval.size == beta.size):
            raise ValueError("hdim, hval and beta have one entry per basis column")
        rc = self.lib.gpe_hm_add(self._h, ctx._h, active.size, active.ctypes.data_as(i32), hdim.size,
                                 hdim.ctypes.data_as(i32), _ptr(hval), _ptr(beta), float(sigma))
        # (the return value 1 is emulator number 1 unless the set left an error text: GPE_NOT_PD)
        if rc < 0 or (rc == GPE_NOT_PD and self.lib.gpe_hm_last_error(self._h)):
            self._check(rc, "gpe_hm_add")
        return rc

    def add_multi(self, ctx, active, hdim, hval, B, Sigma):
        """Snapshot ctx's resident factor and outputs (set_outputs, p of them) as one member of
        p outputs; returns the member's number.  B (q x p, beta_multi's) and Sigma (p x p);
        active, hdim and hval as ``add``.  The member takes p consecutive places among the
        set's outputs."""
        i32 = _ct.POINTER(_ct.c_int32)
        active = _np.ascontiguousarray(active, dtype=_np.int32).ravel()
        hdim = _np.ascontiguousarray(hdim, dtype=_np.int32).ravel()
        hval = _f64(hval).ravel()
        B = _f64(B)
        Sigma = _f64(Sigma)
        if B.ndim != 2 or B.shape[0] != hdim.size or hval.size != hdim.size:
            raise ValueError("hdim, hval and B have one entry (row) per basis column")
        p = B.shape[1]
        if Sigma.shape != (p, p):
            raise ValueError("Sigma is p x p for the p columns of B")
        rc = self.lib.gpe_hm_add_multi(self._h, ctx._h, active.size, active.ctypes.data_as(i32), hdim.size,
                                       hdim.ctypes.data_as(i32), _ptr(hval), p, _ptr(B), _ptr(Sigma))
        if rc < 0 or (rc == GPE_NOT_PD and self.lib.gpe_hm_last_error(self._h)):
            self._check(rc, "gpe_hm_add_multi")
        return rc

    @property
    def outputs(self):
        """The members' outputs together: 1 per ``add`` member, p per ``add_multi`` member."""
        return int(self.lib.gpe_hm_outputs(self._h))

    def member_outputs(self, member):
        return int(self.lib.gpe_hm_member_outputs(self._h, int(member)))

    def implausibility_mv(self, member, Xs, z, V, parts=False):
        """I^2 (m): the joint implausibility (z - mean)^T (c Sigma + V)^-1 (z - mean) of one
        multi-output member, no square root.  z (p), V (p x p, symmetric positive definite).
        parts=True: (I^2, mean p x m, c m)."""
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = Xs.reshape(-1, 1)
        m, D = Xs.shape
        p = self.member_outputs(member)
        z = _f64(z).ravel()
        V = _f64(V)
        if p > 0 and (z.size != p or V.shape != (p, p)):
            raise ValueError("z has one entry per output of the member, and V is p x p")
        i2 = _np.zeros(m)
        mean = _np.zeros((max(p, 1), m)) if parts else None
        c = _np.zeros(m) if parts else None
        self._check(self.lib.gpe_hm_implausibility_mv(self._h, int(member), m, D, _ptr(Xs), _ptr(z), _ptr(V), _ptr(i2),
                                                      _ptr(mean), _ptr(c)), "gpe_hm_implausibility_mv")
        return (i2, mean, c) if parts else i2

    def implausibility(self, Xs, z, var_extra, maxno=1, parts=False):
        """imax (m x maxno): per candidate the maxno largest implausibilities over the
        set's outputs (its emulators, and every output of a multi-output member), ascending,
        NaN last.  parts=True: (imax, mean, var) with mean and var p x m, p = ``outputs``.
        Xs is m x D in the scaled coordinates posterior() takes."""
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = Xs.reshape(-1, 1)
        m, D = Xs.shape
        p = self.outputs
        z = _f64(z).ravel()
        ve = _f64(var_extra).ravel()
        if z.size != p or ve.size != p:
            raise ValueError("z and var_extra have one entry per emulator of the set")
        maxno = int(maxno)
        imax = _np.zeros((m, max(maxno, 1)))
        mean = _np.zeros((p, m)) if parts else None
        var = _np.zeros((p, m)) if parts else None
        self._check(self.lib.gpe_hm_implausibility(self._h, m, D, _ptr(Xs), _ptr(z), _ptr(ve), maxno, _ptr(imax),
                                                   _ptr(mean), _ptr(var)), "gpe_hm_implausibility")
        return (imax, mean, var) if parts else imax

    @staticmethod
    def _mesh(D, pair, x1, x2, others):
        D, ca, cb = int(D), int(pair[0]), int(pair[1])
        x1, x2 = _f64(x1).ravel(), _f64(x2).ravel()
        others = _f64(others)
        if others.ndim == 1:
            others = others.reshape(-1, 1) if D != 2 else _np.zeros((others.size, 0))
        if others.ndim != 2 or others.shape[1] != max(D - 2, 0):
            raise ValueError("others is ns x (D - 2): one row per sample of a cell")
        return D, ca, cb, x1, x2, others

    def cells(self, D, pair, x1, x2, others, z, var_extra, cm, maxno=1, use=None):
        """Minimum-implausibility and count maps over the mesh x1 x x2 of the input pair
        ``pair`` = (ca, cb), the candidates made and reduced on the device (gpe_hm_cells).
        Candidate (i, j, t) has x1[i] in column ca, x2[j] in column cb and others[t] (ns x
        (D - 2)) in the other columns in ascending order.  Returns (imp, below), each maxno x
        g1 x g2: per level l (the (l + 1)-th largest implausibility over the outputs) the minimum
        over a cell's ns samples (NaN if any is NaN) and the number of samples below cm.
        use: one flag per output (None: all); an output switched off enters with I^2 = 0."""
        D, ca, cb, x1, x2, others = self._mesh(D, pair, x1, x2, others)
        p = self.outputs
        z, ve = _f64(z).ravel(), _f64(var_extra).ravel()
        if z.size != p or ve.size != p:
            raise ValueError("z and var_extra have one entry per output of the set")
        flags = None
        if use is not None:
            flags = _np.ascontiguousarray(_np.asarray(use) != 0, dtype=_np.int32).ravel()
            if flags.size != p:
                raise ValueError("use has one flag per output of the set")
        maxno = int(maxno)
        g1, g2 = x1.size, x2.size
        imp = _np.zeros((max(maxno, 1), g1, g2))
        below = _np.zeros((max(maxno, 1), g1, g2), dtype=_np.int64)
        self._check(self.lib.gpe_hm_cells(
            self._h, D, ca, cb, g1, _ptr(x1), g2, _ptr(x2), others.shape[0], _ptr(others) if D > 2 else None,
            flags.ctypes.data_as(_ct.POINTER(_ct.c_int32)) if flags is not None else None, _ptr(z), _ptr(ve), maxno,
            float(cm), _ptr(imp), below.ctypes.data_as(_ct.POINTER(_ct.c_int64))), "gpe_hm_cells")
        return imp, below

    def cells_mv(self, member, D, pair, x1, x2, others, z, V, cm):
        """``cells`` for the joint measure of one multi-output member (gpe_hm_cells_mv): one
        level, I = sqrt(I^2) of ``implausibility_mv``.  Returns (imp, below), each g1 x g2."""
        D, ca, cb, x1, x2, others = self._mesh(D, pair, x1, x2, others)
        p = self.member_outputs(member)
        z, V = _f64(z).ravel(), _f64(V)
        if p > 0 and (z.size != p or V.shape != (p, p)):
            raise ValueError("z has one entry per output of the member, and V is p x p")
        g1, g2 = x1.size, x2.size
        imp = _np.zeros((g1, g2))
        below = _np.zeros((g1, g2), dtype=_np.int64)
        self._check(self.lib.gpe_hm_cells_mv(
            self._h, int(member), D, ca, cb, g1, _ptr(x1), g2, _ptr(x2), others.shape[0],
            _ptr(others) if D > 2 else None, _ptr(z), _ptr(V), float(cm), _ptr(imp),
            below.ctypes.data_as(_ct.POINTER(_ct.c_int64))), "gpe_hm_cells_mv")
        return imp, below

    def sample(self, lo, hi, state, inc, first, m, z, var_extra, cm, maxno=1, cap=None):
        """Rejection sampling on the device (gpe_hm_sample): candidates number first ..
        first + m - 1 of the PCG64 stream with 128-bit ``state`` and ``inc`` (Python ints:
        ``default_rng(seed).bit_generator.state["state"]``), mapped into the box [lo, hi) as
        ``lo + rng.random((., D)) * (hi - lo)``, accepted where the maxno-th largest
        implausibility is below cm.  Returns (points, idx, accepted): the first ``cap`` (None: m)
        accepted rows in stream order, their candidate numbers, and the count of all accepted."""
        lo, hi = _f64(lo).ravel(), _f64(hi).ravel()
        if lo.size != hi.size:
            raise ValueError("lo and hi have one entry per input")
        D, p = lo.size, self.outputs
        z, ve = _f64(z).ravel(), _f64(var_extra).ravel()
        if z.size != p or ve.size != p:
            raise ValueError("z and var_extra have one entry per output of the set")
        m = int(m)
        cap = m if cap is None else int(cap)
        rows = max(0, min(cap, m))
        pts = _np.zeros((rows, D))
        idx = _np.zeros(rows, dtype=_np.int64)
        mask = (1 << 64) - 1
        st = (_ct.c_uint64 * 2)((int(state) >> 64) & mask, int(state) & mask)
        ic = (_ct.c_uint64 * 2)((int(inc) >> 64) & mask, int(inc) & mask)
        acc = _ct.c_int64(0)
        self._check(self.lib.gpe_hm_sample(
            self._h, D, _ptr(lo), _ptr(hi), st, ic, int(first), m, _ptr(z), _ptr(ve), int(maxno), float(cm), cap,
            _ptr(pts) if rows else None, idx.ctypes.data_as(_ct.POINTER(_ct.c_int64)) if rows else None,
            _ct.byref(acc)), "gpe_hm_sample")
        got = min(int(acc.value), rows)
        return pts[:got], idx[:got], int(acc.value)


def default_context() -> Context:
    """The calling thread's bound context (bind_context), else the process-wide
    context on the GPU chosen by GPEMU_DEVICE / LOCAL_RANK (or 0)."""
    bound = getattr(_tls, "ctx", None)
    if bound is not None:
        return bound
    global _default_ctx
    with _ctx_lock:
        if _default_ctx is None:
            dev = int(_os.environ.get("GPEMU_DEVICE", _os.environ.get("LOCAL_RANK", "0")))
            _default_ctx = Context(dev)
        return _default_ctx


class bind_context:
    """Route default_context() of the current thread to `ctx` inside the block
    (worker threads of concurrent multistart tries, optimize.py)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.prev = getattr(_tls, "ctx", None)
        _tls.ctx = self.ctx
        return self.ctx

    def __exit__(self, *exc):
        _tls.ctx = self.prev
        return False


def worker_contexts(k: int) -> list:
    """k contexts on the default context's GPU: the default one plus k-1 extra,
    created once and kept (each has its own HIP stream and workspaces)."""
    base = default_context()
    with _ctx_lock:
        while len(_extra_ctxs) < k - 1:
            _extra_ctxs.append(Context(base.device))
        return [base] + _extra_ctxs[:k - 1]


class DistContext:
    """Row-block distributed objective and gradient over P GPUs (include/gpemu_dist.h).

    unique_id=None selects the in-process loopback transport: all `nranks`
    logical ranks run in this process on `device` (same partition and schedule,
    device copies instead of RCCL).  With a unique id (bytes from
    ``dist_unique_id()`` on rank 0, shared by the host, see distributed.py) this
    process is rank `rank` of an RCCL communicator of `nranks` GPUs.
    """

    def __init__(self, device: int, nranks: int, rank: int = 0, unique_id: bytes | None = None):
        self.lib = load_library()
        if self.lib.gpe_device_count() <= 0:
            raise NativeUnavailable("no HIP device visible to libgpemu.so")
        if unique_id is not None and len(unique_id) != UNIQUE_ID_BYTES:
            raise ValueError("unique_id must be 128 bytes")
        h = self.lib.gpe_dist_create(int(device), int(nranks), int(rank), unique_id)
        if not h:
            raise NativeUnavailable("gpe_dist_create failed")
        self._h = h
        self.nranks, self.rank, self.loopback = nranks, rank, unique_id is None

    def close(self):
        if getattr(self, "_h", None):
            self.lib.gpe_dist_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc == GPE_OK:
            return
        msg = self.lib.gpe_dist_last_error(self._h).decode()
        if rc == GPE_NOT_PD:
            raise NotPositiveDefinite(f"{what}: {msg}")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")

    def set_data(self, X, f, H, r=None):
        X = _f64(X)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        n, d = X.shape
        f = _f64(f, (n,))
        H = _f64(H)
        if H.ndim == 1:
            H = H.reshape(n, -1)
        rr = None if r is None or _np.isscalar(r) else _f64(r, (n,))
        self._keep = (X, f, H, rr)
        self._check(self.lib.gpe_dist_set_data(self._h, n, d, H.shape[1], _ptr(X), _ptr(f), _ptr(H),
                                               _ptr(rr)), "gpe_dist_set_data")

    def objective(self, variant, kernel, hp, nu_fixed=0.0, want_grad=False):
        """Objective (collective over all ranks): (llh, sigma2), or (llh, grad, sigma2)
        with want_grad."""
        hp = _f64(hp).ravel()
        llh, s2 = _ct.c_double(0.0), _ct.c_double(0.0)
        grad = _np.zeros(hp.size) if want_grad else None
        self._check(self.lib.gpe_dist_objective(self._h, int(variant), int(kernel), _ptr(hp), hp.size,
                                                float(nu_fixed), int(bool(want_grad)), _ct.byref(llh),
                                                _ptr(grad), _ct.byref(s2)),
                    "gpe_dist_objective")
        if want_grad:
            return llh.value, grad, s2.value
        return llh.value, s2.value

    def times(self):
        tot, comm = _ct.c_double(0.0), _ct.c_double(0.0)
        self._check(self.lib.gpe_dist_times(self._h, _ct.byref(tot), _ct.byref(comm)), "gpe_dist_times")
        return {"total_ms": tot.value, "comm_ms": comm.value}

    def rank_bytes(self, rank: int | None = None) -> int:
        """Device bytes held for `rank` (default: this process's rank; any logical
        rank in loopback)."""
        b = _ct.c_int64(0)
        r = self.rank if rank is None else int(rank)
        self._check(self.lib.gpe_dist_rank_bytes(self._h, r, _ct.byref(b)), "gpe_dist_rank_bytes")
        return int(b.value)


def device_synchronize(device: int) -> None:
    """Wait for all work on GPU `device` (no PyTorch in the process)."""
    rc = load_library().gpe_device_synchronize(int(device))
    if rc != GPE_OK:
        raise RuntimeError(f"gpe_device_synchronize({device}) failed ({rc})")


def dist_unique_id() -> bytes:
    """A fresh RCCL communicator id (rank 0 only)."""
    lib = load_library()
    buf = _ct.create_string_buffer(UNIQUE_ID_BYTES)
    rc = lib.gpe_dist_unique_id(buf, UNIQUE_ID_BYTES)
    if rc != GPE_OK:
        raise RuntimeError(f"gpe_dist_unique_id failed ({rc})")
    return buf.raw


def dist_owner(nranks: int, tile_row: int) -> int:
    """Rank that stores 128-row tile row `tile_row` (pure; no GPU)."""
    return int(load_library().gpe_dist_owner(int(nranks), int(tile_row)))


def dist_local_rows(n: int, nranks: int, rank: int, q: int = 0) -> int:
    """Tile rows rank `rank` stores for n points and q basis columns, including its
    share of the ceil((q+1)/128) augmented [f H]^T rows (pure; no GPU)."""
    return int(load_library().gpe_dist_local_rows(int(n), int(q), int(nranks), int(rank)))
