"""ORACLE — test infrastructure only.

ctypes access to the OpenBLAS that numpy ships (0.3.29, DYNAMIC_ARCH; SkylakeX kernels on this
host) through its Fortran interface -- dgemm_64_ / dgemv_64_ / ddot_64_, the ILP64 entry points
Julia's LinearAlgebra.BLAS ccalls.  It is the ground truth that pins oracle/or_blas.h (the rounding
of the reference's BLAS-dispatched products) in tests/test_oracle_blas.py and the Julia-dispatch
products of tools/ilqr_ulp_sources.py / tools/blas_replay.py.  Its LAPACK (dgetrf_64_ / dgetri_64_ / dpotrf_64_ /
dtrtrs_64_, called as Julia's LAPACK.getrf! / getri! / potrf! / trtrs! call them) pins inv(Σ) and cholesky(Σ) of
the MPPI plan in tests/test_mppi_ref.py.  Never used by the product.
"""
import ctypes
import glob
import os

import numpy as np

_lib = None
_i64 = ctypes.c_int64
_dp = ctypes.POINTER(ctypes.c_double)


def lib():
    """The numpy-bundled libscipy_openblas64_ (None when this numpy links another BLAS)."""
    global _lib
    if _lib is None:
        d = os.path.join(os.path.dirname(np.__file__), os.pardir, "numpy.libs")
        cands = sorted(glob.glob(os.path.join(d, "libscipy_openblas64_*.so")))
        if not cands:
            return None
        _lib = ctypes.CDLL(cands[0])
        _lib.scipy_ddot_64_.restype = ctypes.c_double
        f = _lib.scipy_openblas_get_config64_
        f.restype = ctypes.c_char_p
    return _lib


def config():
    L = lib()
    return None if L is None else L.scipy_openblas_get_config64_().decode()


def _p(a):
    return a.ctypes.data_as(_dp)


def _r(v):
    return ctypes.byref(_i64(v))


def gemm(A, B, ta=False, tb=False):
    """BLAS.gemm!('T'/'N', 'T'/'N', 1.0, A, B, 0.0, C) exactly as Julia calls it: op(A) * op(B),
    A and B given untransposed (column-major copies are made, the values are the same)."""
    A = np.asfortranarray(A, np.float64)
    B = np.asfortranarray(B, np.float64)
    if A.ndim == 1:
        A = A.reshape(-1, 1, order="F")
    if B.ndim == 1:
        B = B.reshape(-1, 1, order="F")
    m = A.shape[1] if ta else A.shape[0]
    k = A.shape[0] if ta else A.shape[1]
    n = B.shape[0] if tb else B.shape[1]
    assert (B.shape[1] if tb else B.shape[0]) == k
    C = np.zeros((m, n), order="F")
    one, zero = ctypes.c_double(1.0), ctypes.c_double(0.0)
    lib().scipy_dgemm_64_(ctypes.c_char_p(b"T" if ta else b"N"), ctypes.c_char_p(b"T" if tb else b"N"),
                          _r(m), _r(n), _r(k), ctypes.byref(one), _p(A), _r(A.shape[0]), _p(B), _r(B.shape[0]),
                          ctypes.byref(zero), _p(C), _r(m), ctypes.c_size_t(1), ctypes.c_size_t(1))
    return np.ascontiguousarray(C)


def gemv(A, x, t=False):
    """BLAS.gemv!('T'/'N', 1.0, A, x, 0.0, y): op(A) * x for a matrix A and a vector x."""
    A = np.asfortranarray(A, np.float64)
    x = np.ascontiguousarray(x, np.float64).ravel()
    m, n = A.shape
    assert len(x) == (m if t else n)
    y = np.zeros(n if t else m)
    one, zero = ctypes.c_double(1.0), ctypes.c_double(0.0)
    lib().scipy_dgemv_64_(ctypes.c_char_p(b"T" if t else b"N"), _r(m), _r(n), ctypes.byref(one), _p(A), _r(m),
                          _p(x), _r(1), ctypes.byref(zero), _p(y), _r(1), ctypes.c_size_t(1))
    return y


def getrf_getri(A):
    """inv(A) of a general square matrix as Julia's inv!(lu(A)) gets it: LAPACK.getrf!(A) then
    LAPACK.getri!(A, ipiv) (workspace query with lwork = -1 first, as getri! does).
    Returns (inv(A), ipiv) with ipiv LAPACK's 1-based row interchanges."""
    A = np.array(A, np.float64, order="F")
    n = A.shape[0]
    assert A.shape == (n, n)
    ipiv = np.zeros(n, np.int64)
    info = _i64(0)
    pi = ipiv.ctypes.data_as(ctypes.POINTER(_i64))
    lib().scipy_dgetrf_64_(_r(n), _r(n), _p(A), _r(max(1, n)), pi, ctypes.byref(info))
    if info.value:
        raise np.linalg.LinAlgError("dgetrf info = %d" % info.value)
    work = np.zeros(1)
    lwork = -1
    for _ in range(2):
        lib().scipy_dgetri_64_(_r(n), _p(A), _r(max(1, n)), pi, _p(work), _r(lwork), ctypes.byref(info))
        if info.value:
            raise np.linalg.LinAlgError("dgetri info = %d" % info.value)
        if lwork < 0:
            lwork = int(work[0])
            work = np.zeros(max(1, lwork))
    return np.ascontiguousarray(A), ipiv


def potrf(A, uplo="U"):
    """LAPACK.potrf!(uplo, A): the Cholesky factor in the `uplo` triangle (the other triangle zeroed
    here).  Julia's cholesky(A) factors Hermitian(A, :U), i.e. potrf('U'), and .L is its transpose."""
    A = np.array(A, np.float64, order="F")
    n = A.shape[0]
    assert A.shape == (n, n) and uplo in ("U", "L")
    info = _i64(0)
    lib().scipy_dpotrf_64_(ctypes.c_char_p(uplo.encode()), _r(n), _p(A), _r(max(1, n)), ctypes.byref(info),
                           ctypes.c_size_t(1))
    if info.value:
        raise np.linalg.LinAlgError("dpotrf info = %d" % info.value)
    return np.ascontiguousarray(np.triu(A) if uplo == "U" else np.tril(A))


def trtrs_identity(A, uplo="U"):
    """inv of a triangular matrix as Julia's inv(UpperTriangular(A)) / inv(LowerTriangular(A)) gets it:
    LAPACK.trtrs!(uplo, 'N', 'N', A, Matrix(I)) -- the path Julia's inv(A) takes when istriu(A) or
    istril(A) holds, a diagonal Σ included."""
    A = np.array(A, np.float64, order="F")
    n = A.shape[0]
    B = np.asfortranarray(np.eye(n))
    info = _i64(0)
    c = ctypes.c_char_p
    lib().scipy_dtrtrs_64_(c(uplo.encode()), c(b"N"), c(b"N"), _r(n), _r(n), _p(A), _r(max(1, n)), _p(B),
                           _r(max(1, n)), ctypes.byref(info), ctypes.c_size_t(1), ctypes.c_size_t(1),
                           ctypes.c_size_t(1))
    if info.value:
        raise np.linalg.LinAlgError("dtrtrs info = %d" % info.value)
    return np.ascontiguousarray(B)


def dot(x, y):
    """BLAS.dot(x, y) (LinearAlgebra.dot of two Float64 vectors)."""
    x = np.ascontiguousarray(x, np.float64).ravel()
    y = np.ascontiguousarray(y, np.float64).ravel()
    return lib().scipy_ddot_64_(_r(len(x)), _p(x), _r(1), _p(y), _r(1))
