"""GPU: the fp32 device CSR operator (arpack_hip_csr_create_f32) and the
single-precision family's free run on it (arpack_hip_ssaupd_csr, _csr_cycles,
arpack_hip_snaupd_csr_cycles).

Product.  The SELL form sums every row in fp64 in column order and rounds once,
and a product of two floats is exact in fp64, so y must equal
(A32.astype(f64) @ x.astype(f64)).astype(f32) bit for bit -- on a partly filled
slice, several superblocks, multi-range windows (the 3-D Laplacian at m = 72,
the smallest m whose rows span more than one 10,240-column window:
2 m^2 + 1 = 10,369 > 10,240 >= 10,083 at m = 71) and a hand-made matrix around
the kernel's chunk lengths U = 4 and 6.  The vector fallback sums lane partials
in a fixed tree: bound = one fp32 rounding + two fp64 sums of L_i terms in
different orders, and bitwise equal from launch to launch.

Solves.  The free run against the reference's float fixtures s1-s7 with the
criteria of tests/test_gpu_single.py (helpers copied from there), against the
library's own reverse-communication path with the same product, parking by
cycles, eigsh / eigs, the fault-injection convention, and every refusal between
the fp32 operator and the fp64 entries (and the other way round).  One start
vector on which sneupd's Schur order used to disagree with snaupd's is pinned.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import matrices as M

pytestmark = pytest.mark.gpu
EPS_F = float(np.finfo(np.float32).eps) / 2
SELL, VECTOR = 11, 0


# ---- helpers copied from tests/test_gpu_single.py ---------------------------
def _mat(spec):
    k = str(spec[0])
    if k == "diag":
        return M.diag(int(spec[1]))
    if k == "laplace2d":
        return M.laplace2d(int(spec[1]), float(spec[2]))
    if k == "anderson":
        return M.anderson(int(spec[1]), int(spec[2]), float(spec[3]), int(spec[4]))
    if k == "banded_sym":
        return M.banded_sym(int(spec[1]), int(spec[2]), int(spec[3]), int(spec[4]))
    if k == "convdiff2d":
        return M.convdiff2d(int(spec[1]), float(spec[2]))
    raise KeyError(k)


def _tol(g):
    """10 max(tol, eps_f), floored at 1e-5: at tol = 0 the reference's own float
    eigenvalues carry ~1e2 eps_f of rounding (s5: 992 comes back as 991.99835)."""
    return max(10 * max(float(g["tol"]), EPS_F), 1e-5)


def _resid(A, z, d):
    anorm = abs(A).sum(axis=0).max()
    return max(np.linalg.norm(A @ z[:, k] - d[k] * z[:, k]) / (anorm * np.linalg.norm(z[:, k]))
               for k in range(len(d)))


def _counts(g, s):
    assert int(s.info[0]) == int(g["info"]) == 0
    assert int(s.iparam[4]) == int(g["iparam"][4])
    it, ref = int(s.iparam[2]), int(g["iparam"][2])
    assert abs(it - ref) <= max(2, 0.25 * ref), (it, ref)


# ---- product ---------------------------------------------------------------
def _x32(n, seed=7):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def _spmv(pkg, A, x):
    xb = pkg.DeviceBuffer.from_numpy(x)
    yb = pkg.DeviceBuffer(A.n, np.float32)
    A.matvec_device(xb, yb)
    return yb.numpy()


def _ref64(rp, col, val32, x):
    """The contract's right-hand side before its one rounding: fp64 SciPy on A32."""
    return M.to_scipy(rp, col, val32.astype(np.float64)) @ x.astype(np.float64)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _handmade():
    """4,096 rows of lengths 0, 1, U-1, U, U+1, 2U+1 for U = 4 and U = 6 (the
    kernel's two chunk lengths) in turn, columns from the diagonal on; row 2000
    holds 1,000 entries inside its window; the first and the last row are empty."""
    n = 4096
    lens = np.array([0, 1, 3, 4, 5, 9, 5, 6, 7, 13])[np.arange(n) % 10]
    lens[0] = lens[n - 1] = 0
    lens[2000] = 1000
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    col = np.empty(rp[-1], np.int32)
    for i in range(n):
        start = 1500 if i == 2000 else min(i, n - lens[i])
        col[rp[i]:rp[i + 1]] = start + np.arange(lens[i])
    val = np.random.default_rng(11).standard_normal(rp[-1])
    return rp, col, val


def _lap3d_72():
    return M.laplace3d(72)


CASES = {
    "laplace2d_10": lambda: M.laplace2d(10, 121.0),        # n = 100: one partly filled slice
    "banded_20000": lambda: M.banded_sym(20000, 1234, 512, 25),  # several superblocks
    "laplace3d_72": _lap3d_72,                              # multi-range windows
    "handmade_4096": _handmade,
    "convdiff2d_30": lambda: M.convdiff2d(30, 10.0),        # values not representable in fp32
}


@pytest.mark.parametrize("name", list(CASES))
def test_sell_product_bitwise(pkg, name):
    rp, col, val = CASES[name]()
    val32 = val.astype(np.float32)
    A = pkg.CSR.from_arrays(rp, col, val, dtype=np.float32)
    assert A.dtype == np.float32 and A.kernel == SELL
    assert pkg.lib().arpack_hip_csr_precision(A.h) == ord("s")
    x = _x32(A.n)
    ref = _ref64(rp, col, val32, x).astype(np.float32)
    for tile in (6, 4):  # the default chunk length, then the short one
        A.set_kernel(SELL, tile)
        y = _spmv(pkg, A, x)
        assert np.array_equal(_bits(y), _bits(ref)), (name, tile, np.abs(y - ref).max())
        assert np.array_equal(_bits(_spmv(pkg, A, x)), _bits(y))  # a second launch
    r2, c2, v2 = A.download()
    assert v2.dtype == np.float32 and np.array_equal(_bits(v2), _bits(val32))
    assert np.array_equal(r2, rp) and np.array_equal(c2, col)


def test_multirange_threshold_is_m72(pkg):
    """The fp64 plan of the same matrices: m = 72 has multi-range windows (only
    the SELL kernel reads them, so the single-window forms are refused), m = 71
    still fits one window a superblock."""
    A72 = pkg.CSR.laplace3d(72)
    assert A72.kernel == SELL
    with pytest.raises(RuntimeError):
        A72.set_kernel(8)
    A71 = pkg.CSR.laplace3d(71)
    assert A71.kernel == SELL
    A71.set_kernel(8)


def _scattered():
    """30,000 rows, 5 uniformly random columns a row: no window plan accepts it."""
    n, L = 30000, 5
    rng = np.random.default_rng(5)
    col = np.sort(rng.integers(0, n, size=(n, L)), axis=1).astype(np.int32).ravel()
    rp = np.arange(n + 1, dtype=np.int64) * L
    return rp, col, rng.standard_normal(n * L)


def test_vector_fallback(pkg):
    rp, col, val = _scattered()
    val32 = val.astype(np.float32)
    A = pkg.CSR.from_arrays(rp, col, val, dtype=np.float32)
    assert A.kernel == VECTOR
    x = _x32(A.n)
    y = _spmv(pkg, A, x).astype(np.float64)
    r = _ref64(rp, col, val32, x)
    absA = M.to_scipy(rp, col, np.abs(val32).astype(np.float64))
    L = np.diff(rp).astype(np.float64)
    bound = 2.0 ** -24 * np.abs(r) + 2.0 * L * 2.0 ** -53 * (absA @ np.abs(x).astype(np.float64))
    err = np.abs(y - r)
    print("vector fallback: max err / bound", (err / np.maximum(bound, 1e-300)).max())
    assert np.all(err <= bound)
    assert np.array_equal(_bits(_spmv(pkg, A, x)), _bits(y.astype(np.float32)))
    with pytest.raises(RuntimeError):  # no SELL layout was built
        A.set_kernel(SELL)
    assert A.kernel == VECTOR


def test_sell_operator_runs_the_fallback_on_request(pkg):
    """set_kernel(0) on an operator with a SELL layout: the fallback's bound."""
    rp, col, val = M.banded_sym(20000, 1234, 512, 25)
    val32 = val.astype(np.float32)
    A = pkg.CSR.from_arrays(rp, col, val, dtype=np.float32)
    A.set_kernel(VECTOR)
    assert A.kernel == VECTOR
    x = _x32(A.n)
    y = _spmv(pkg, A, x).astype(np.float64)
    r = _ref64(rp, col, val32, x)
    absA = M.to_scipy(rp, col, np.abs(val32).astype(np.float64))
    bound = 2.0 ** -24 * np.abs(r) + 2.0 * np.diff(rp) * 2.0 ** -53 * (absA @ np.abs(x).astype(np.float64))
    assert np.all(np.abs(y - r) <= bound)
    A.set_kernel(SELL)
    assert np.array_equal(_bits(_spmv(pkg, A, x)), _bits(r.astype(np.float32)))


# ---- refusals --------------------------------------------------------------
def _c_aupd(pkg, fn, A, s):
    """The C entry itself (SymRci / NsRci refuse a mismatch before the call)."""
    tol = (C.c_float if s.prec == "s" else C.c_double)(s.tol)
    args = [A.h]
    if fn.endswith("_cycles"):
        args.append(-1)
    args += [s.ido.ctypes.data_as(C.POINTER(C.c_int)), s.bmat.encode(), s.n, s.which.encode(),
             s.nev, C.byref(tol) if fn.endswith("_cycles") else tol, s.resid.ctypes.data, s.ncv,
             s.v.ctypes.data, s.ldv, s.iparam.ctypes.data_as(C.POINTER(C.c_int)),
             s.ipntr.ctypes.data_as(C.POINTER(C.c_int)), s.workd.ctypes.data, s.workl.ctypes.data,
             s.lworkl, s.info.ctypes.data_as(C.POINTER(C.c_int))]
    getattr(pkg.lib(), fn)(*args)
    return int(s.ido[0]), int(s.info[0])


def test_refusals(pkg):
    L = pkg.lib()
    rp, col, val = M.laplace2d(10, 121.0)
    n = len(rp) - 1
    A32 = pkg.CSR.from_arrays(rp, col, val, dtype=np.float32)
    A64 = pkg.CSR.from_arrays(rp, col, val.astype(np.float32))  # dtype=None: promoted, as before
    assert A64.dtype == np.float64 and A64.download()[2].dtype == np.float64
    x = _x32(n)
    ref = _ref64(rp, col, val.astype(np.float32), x).astype(np.float32)
    x64, y64 = pkg.DeviceBuffer.from_numpy(x.astype(np.float64)), pkg.DeviceBuffer(n)
    x32, y32 = pkg.DeviceBuffer.from_numpy(x), pkg.DeviceBuffer(n, np.float32)

    def still_works():
        assert np.array_equal(_bits(_spmv(pkg, A32, x)), _bits(ref))
        A64.matvec_device(x64, y64)
        assert np.array_equal(y64.numpy(), M.to_scipy(rp, col, val) @ x.astype(np.float64))

    # fp64 entries on the fp32 operator
    assert L.arpack_hip_csr_spmv(A32.h, x64.ptr, y64.ptr) == -1
    still_works()
    assert L.arpack_hip_csr_time(A32.h, x64.ptr, y64.ptr, 2) == -1.0
    still_works()
    assert L.arpack_hip_csr_download(A32.h, None, None, None) == -1
    with pytest.raises(ValueError):
        A32.matvec_device(x64, y64)
    with pytest.raises(RuntimeError):
        A32.set_symmetric(True)
    assert A32.last_rc == -1
    still_works()
    assert L.arpack_hip_csr_set_sym_accumulator(A32.h, 0) == -1
    still_works()
    for kern in (1, 2, 3, 5, 8, 9, 10, 12):  # forms without an fp32 kernel
        assert L.arpack_hip_csr_set_kernel(A32.h, kern, 4096) == -1
    assert A32.kernel == SELL
    still_works()
    with pytest.raises(RuntimeError):
        pkg.DShift(A32, 0.5)
    still_works()
    with pytest.raises(RuntimeError):
        pkg.DGen(A32, A64, 2)
    with pytest.raises(RuntimeError):
        pkg.DGen(A64, A32, 2)
    still_works()
    with pytest.raises(RuntimeError):
        pkg.SVDOp(A32)
    still_works()
    pkg.comm_init(1, 0, pkg.comm_unique_id(), 0)
    try:
        with pytest.raises(RuntimeError):
            pkg.DistOp(A32, n, 0)
    finally:
        pkg.comm_destroy()
    still_works()
    # d* solver entries on the fp32 operator: info = -11 before anything runs
    for cls, fn in ((pkg.SymRci, "arpack_hip_dsaupd_csr"), (pkg.SymRci, "arpack_hip_dsaupd_csr_cycles"),
                    (pkg.NsRci, "arpack_hip_dnaupd_csr_cycles")):
        s = cls(n, 4, 20, "LM", 0.0)
        assert _c_aupd(pkg, fn, A32, s) == (99, -11), fn
        with pytest.raises(ValueError):
            s.aupd_csr(A32)
        with pytest.raises(ValueError):
            s.aupd_cycles(A32, 2)
        still_works()
    # fp32 entries on the fp64 operator
    assert L.arpack_hip_csr_spmv_f32(A64.h, x32.ptr, y32.ptr) == -1
    assert L.arpack_hip_csr_time_f32(A64.h, x32.ptr, y32.ptr, 2) == -1.0
    assert L.arpack_hip_csr_download_f32(A64.h, None, None, None) == -1
    with pytest.raises(ValueError):
        A64.matvec_device(x32, y32)
    still_works()
    for cls, fn in ((pkg.SymRci, "arpack_hip_ssaupd_csr"), (pkg.SymRci, "arpack_hip_ssaupd_csr_cycles"),
                    (pkg.NsRci, "arpack_hip_snaupd_csr_cycles")):
        s = cls(n, 4, 20, "LM", 0.0, prec="s")
        assert _c_aupd(pkg, fn, A64, s) == (99, -11), fn
        with pytest.raises(ValueError):
            s.aupd_csr(A64)
        still_works()
    # Python-level refusals
    with pytest.raises(ValueError):
        pkg.CSR.from_arrays(rp, col, val, shape=(n, n), dtype=np.float32)
    with pytest.raises(ValueError):
        pkg.eigsh(A32, n, 4, sigma=900.0)
    with pytest.raises(ValueError):
        pkg.eigs(A32, n, 4, sigma=900.0)
    still_works()
    # a bad index is refused at creation
    bad = col.copy()
    bad[3] = n
    h = C.c_void_p()
    v32 = val.astype(np.float32)
    assert L.arpack_hip_csr_create_f32(C.byref(h), n, len(col), rp.ctypes.data, bad.ctypes.data,
                                       v32.ctypes.data) == -1
    still_works()


# ---- solves ----------------------------------------------------------------
_OPS = {}


def _case(pkg, golden, name):
    """(fixture, SciPy A in fp64, the fp32 device operator), built once a name."""
    if name not in _OPS:
        g = golden(name)
        rp, col, val = _mat(g["spec"])
        _OPS[name] = (g, M.to_scipy(rp, col, val), pkg.CSR.from_arrays(rp, col, val, dtype=np.float32))
    return _OPS[name]


def _sym(pkg, g, n, device, **kw):
    return pkg.SymRci(n, int(g["nev"]), int(g["ncv"]), str(g["which"]), float(g["tol"]),
                      mxiter=int(g["mxiter"]), v0=g["v0"], device=device, prec="s", **kw)


def _ns(pkg, g, n, device=False):
    return pkg.NsRci(n, int(g["nev"]), int(g["ncv"]), str(g["which"]), float(g["tol"]),
                     mxiter=int(g["mxiter"]), v0=g["v0"], device=device, prec="s")


@pytest.mark.parametrize("name,device", [("s1_sssimp", False), ("s3_anderson3d", False),
                                         ("s3_anderson3d", True), ("s4_banded", True)])
def test_ssaupd_free_run(pkg, golden, name, device):
    g, A, A32 = _case(pkg, golden, name)
    n = A.shape[0]
    s = _sym(pkg, g, n, device)
    assert s.aupd_csr(A32) == 99
    _counts(g, s)
    d, z, nconv = s.eupd()
    assert d.dtype == np.float32
    dref = g["d"].astype(np.float64)
    scale = np.abs(A).sum(axis=0).max()
    for x in dref:
        assert np.abs(d.astype(np.float64) - x).min() <= _tol(g) * scale
    z = (z.numpy() if device else z).reshape(int(g["nev"]), n)[:nconv].T.astype(np.float64)
    ours = _resid(A, z, d.astype(np.float64))
    if "z" in g:
        theirs = _resid(A, g["z"].astype(np.float64), dref)
        assert ours <= max(10 * theirs, 1e-6), (ours, theirs)
    else:
        assert ours <= max(10 * float(g["tol"]), 1e-6), ours


KEYS = {"LM": np.abs, "LR": np.real}


@pytest.mark.parametrize("name", ["s6_snsimp", "s7_convdiff_lr"])
def test_snaupd_free_run(pkg, golden, name):
    g, A, A32 = _case(pkg, golden, name)
    n = A.shape[0]
    s = _ns(pkg, g, n)
    assert s.aupd_csr(A32) == 99
    _counts(g, s)
    dr, di, z, nconv = s.eupd()
    assert dr.dtype == np.float32
    lam = dr.astype(np.float64) + 1j * di.astype(np.float64)
    ref = g["dr"].astype(np.float64) + 1j * g["di"].astype(np.float64)
    key = KEYS[str(g["which"])]
    scale = np.abs(A).sum(axis=0).max()
    tol = _tol(g) * scale
    print(name, "max |lam - ref| / ||A||_1", max(np.abs(lam - x).min() for x in ref) / scale)
    np.testing.assert_allclose(np.sort(key(lam)), np.sort(key(ref)), rtol=0, atol=tol)
    for x in ref:
        assert np.abs(lam - x).min() <= tol, (x, lam)
    zz = z.reshape(int(g["nev"]) + 1, n)[:nconv].T.astype(np.float64)
    real = np.abs(di) == 0
    if real.any():  # real Ritz pairs: column k is the eigenvector
        ours = _resid(A, zz[:, real], dr[real].astype(np.float64))
        assert ours <= 1e-5, ours


@pytest.mark.parametrize("name", ["s3_anderson3d", "s6_snsimp"])
def test_free_run_equals_own_rci(pkg, golden, name):
    """The same solve through aupd() with OP = matvec_device on the workd
    slices: the float family's steps are the plain ones on both routes."""
    g, A, A32 = _case(pkg, golden, name)
    n = A.shape[0]
    make = _ns if name == "s6_snsimp" else _sym
    free = make(pkg, g, n, True)
    assert free.aupd_csr(A32) == 99 and int(free.info[0]) == 0
    rci = make(pkg, g, n, True)
    while True:
        ido = rci.aupd()
        if ido in (-1, 1):
            A32.matvec_device(rci.slice(0), rci.slice(1))
        else:
            assert ido == 99, ido
            break
    assert int(rci.info[0]) == 0
    for k in (2, 4, 8):
        assert int(free.iparam[k]) == int(rci.iparam[k]), (k, free.iparam, rci.iparam)
    scale = np.abs(A).sum(axis=0).max()
    a, b = free.eupd(rvec=False), rci.eupd(rvec=False)
    if name == "s6_snsimp":
        la, lb = a[0] + 1j * a[1], b[0] + 1j * b[1]
    else:
        la, lb = a[0], b[0]
    assert np.abs(np.sort_complex(la.astype(np.complex128)) -
                  np.sort_complex(lb.astype(np.complex128))).max() <= _tol(g) * scale
    again = make(pkg, g, n, True)
    assert again.aupd_csr(A32) == 99
    c = again.eupd(rvec=False)
    assert np.array_equal(_bits(c[0]), _bits(a[0]))
    if name == "s6_snsimp":
        assert np.array_equal(_bits(c[1]), _bits(a[1]))


def test_park_and_resume(pkg, golden):
    g, A, A32 = _case(pkg, golden, "s4_banded")
    n = A.shape[0]
    whole = _sym(pkg, g, n, True)
    assert whole.aupd_cycles(A32, -1) == 99 and int(whole.info[0]) == 0
    s = _sym(pkg, g, n, True)
    assert s.aupd_cycles(A32, 2) == 98
    assert s.aupd_cycles(A32, -1) == 99
    assert int(s.info[0]) == 0
    assert np.array_equal(s.iparam, whole.iparam)
    _counts(g, s)


def test_eigsh_eigs_float32(pkg, golden):
    g = golden("s1_sssimp")
    rp, col, val = M.laplace2d(10, 121.0)
    A = M.to_scipy(rp, col, val)
    A32 = pkg.CSR.from_arrays(rp, col, val, dtype=np.float32)
    d, Z, res = pkg.eigsh(A32, 100, nev=4, which="LM")
    assert d.dtype == np.float32 and Z.dtype == np.float32 and res["info"] == 0
    scale = np.abs(A).sum(axis=0).max()
    for x in g["d"].astype(np.float64):
        assert np.abs(d.astype(np.float64) - x).min() <= _tol(g) * scale
    g = golden("s6_snsimp")
    rp, col, val = M.convdiff2d(10, 10.0)
    A = M.to_scipy(rp, col, val)
    A32 = pkg.CSR.from_arrays(rp, col, val, dtype=np.float32)
    d, Z, res = pkg.eigs(A32, 100, nev=4, which="LM", tol=float(g["tol"]))
    assert d.dtype == np.complex64 and Z.dtype == np.complex64 and res["info"] == 0
    scale = np.abs(A).sum(axis=0).max()
    ref = g["dr"].astype(np.float64) + 1j * g["di"].astype(np.float64)
    for x in ref:
        assert np.abs(d.astype(np.complex128) - x).min() <= _tol(g) * scale


def test_sneupd_vectors_from_the_start_that_reordered(pkg, golden):
    """slarnv draws 101-200 of seed (1, 3, 5, 7) as the start vector of s6's
    problem: H rounded to the caller's float workl deflates in another order
    than snaupd's fp64 H did, and sneupd with rvec = 1 used to return an unwanted
    Ritz value (265.76) in place of 923.02.  The reference's snaupd_/sneupd_ give
    923.02106, 897.5335, 894.408, 868.9183 from this start (4 cycles, 64 OP*x)."""
    g, A, A32 = _case(pkg, golden, "s6_snsimp")
    iseed = np.array([1, 3, 5, 7], np.int32)
    x = np.zeros(200, np.float32)
    pkg.lib().arpack_hip_kit_slarnv(iseed.ctypes.data_as(C.POINTER(C.c_int)), 200,
                                    x.ctypes.data_as(C.c_void_p))
    s = pkg.NsRci(100, 4, 20, "LM", 1e-5, v0=x[100:], prec="s")
    assert s.aupd_csr(A32) == 99 and int(s.info[0]) == 0
    assert (int(s.iparam[2]), int(s.iparam[4]), int(s.iparam[8])) == (4, 4, 64)
    dr, di, z, nconv = s.eupd(rvec=True)
    ref = np.array([923.02106, 897.5335, 894.408, 868.9183])
    scale = np.abs(A).sum(axis=0).max()
    assert np.abs(np.sort(dr.astype(np.float64)) - np.sort(ref)).max() <= _tol(g) * scale, dr
    assert np.all(di == 0)
    zz = z.reshape(5, 100)[:nconv].T.astype(np.float64)
    # 10x the reference's own largest Ritz residual from this start (1.12e-6)
    ours = _resid(A, zz, dr.astype(np.float64))
    print("reordered start: Ritz residual", ours)
    assert ours <= 10 * 1.12e-6, ours


def test_fault_injection_ends_in_9999(pkg, golden):
    """The convention of tests/test_gpu_faults.py: one early injected failure of
    a checked HIP call ends the free run with info = -9999; the next solve is
    whole again."""
    g, A, A32 = _case(pkg, golden, "s1_sssimp")
    n = A.shape[0]
    pkg.fault_inject(0)
    s = _sym(pkg, g, n, False)
    try:
        pkg.fault_inject(5)
        assert s.aupd_csr(A32) == 99
    finally:
        pkg.fault_inject(0)
    assert int(s.info[0]) == -9999
    s = _sym(pkg, g, n, False)
    assert s.aupd_csr(A32) == 99
    _counts(g, s)
