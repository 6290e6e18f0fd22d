"""GPU: truncated SVD on the device -- rectangular CSR, the normal operator
y = B'(B x) in its two-product and fused forms (spmv_normal.hip), the free run
arpack_hip_dsaupd_svd, the post-processing and svds.

A is m x n, k = min(m, n), B the tall orientation (B = A if m >= n, else A').
Fixtures tests/golden/v*.npz (make_golden_svd.py): the reference's dsaupd on
OP = B'(B x) with SciPy's products, tol = 0.

Bounds.  gamma_r = r u / (1 - r u), u = 2^-53.
  * rectangular SpMV: bitwise SciPy's A @ x where the plan reports the SELL
    kernel (11), else |y - A x| <= gamma_p |A||x| (p the longest row).
  * normal product: |y - yhat| <= 2 gamma_{p+q} |B|'(|B||x|), yhat SciPy's
    float64 Bt @ (B @ x), p the longest row and q the longest column of B:
    gamma_p for w and gamma_q for y compose to gamma_{p+q} in any summation
    order; the factor 2 covers yhat's own error.
  * Ritz values: 1e-10 max|d_ref| (the project's tolerance,
    tests/test_gpu_fullsize.py); svds against numpy.linalg.svd: 1e-10 sigma_max.

"No stale output", the empty columns of v3: v3 is 200 x 1000, so B = A' and y
has k = 200 entries, none of which belongs to a column of A.  The 22 empty
columns of A are empty ROWS of B; what they index is the 1000-long side, so the
exact zeros are asserted there (the rectangular product A' x and the vectors
arpack_hip_dsvd_vectors returns), and a y entry no row touches is asserted on
matrices that have one on the short side: v6 (20 empty columns, two-product)
and the long-row matrix below (column 7 empty, both forms).
"""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
FIX = {"v1": "v1_dsvd", "v2": "v2_tall_257", "v3": "v3_wide_200", "v4": "v4_slice_sm",
       "v5": "v5_small", "v6": "v6_two_product"}
FUSED_OK = ["v1", "v2", "v3", "v4", "v5"]  # k <= fused_kmax; v6 (k = 12000) is two-product only
_cache = {}


def gamma(r):
    return r * U / (1.0 - r * U)


class Case:
    """One matrix: SciPy A, B, Bt, its device CSR, a fixed x and the references,
    computed once and left unchanged."""

    def __init__(self, pkg, A, g=None):
        A = A.tocsr()
        A.sort_indices()
        self.A, self.g = A, g
        self.m, self.n = A.shape
        self.k = min(A.shape)
        self.B = A if self.m >= self.n else A.T.tocsr()
        self.B.sort_indices()
        self.Bt = self.B.T.tocsr()
        self.Bt.sort_indices()
        self.dev = pkg.CSR.from_arrays(A.indptr, A.indices, A.data, shape=A.shape)
        rng = np.random.default_rng(17)
        self.x1 = rng.uniform(-1, 1, self.k)
        self.x2 = rng.uniform(-1, 1, self.k)
        p = int(np.diff(self.B.indptr).max())
        q = int(np.diff(self.Bt.indptr).max())
        self.pq = p + q
        self._ops = {}

    def yhat(self, x):
        return self.Bt @ (self.B @ x)

    def bound(self, x):
        return 2.0 * gamma(self.pq) * (abs(self.Bt) @ (abs(self.B) @ np.abs(x)))

    def op(self, pkg, form):
        if form not in self._ops:
            self._ops[form] = pkg.SVDOp(self.dev, form)
        return self._ops[form]


def fixture_case(pkg, golden, name):
    if name not in _cache:
        g = golden(FIX[name])
        m, n = (int(v) for v in g["shape"])
        _cache[name] = Case(pkg, sp.csr_matrix((g["val"], g["col"], g["rowptr"]), shape=(m, n)), g)
    return _cache[name]


def five_a_row(rows, cols, seed):
    rng = np.random.default_rng(seed)
    w = cols // 5  # one column from each fifth of the width: distinct, sorted, full span
    col = np.arange(5)[None, :] * w + rng.integers(0, w, (rows, 5))
    col[:, 4] = np.maximum(col[:, 4], rng.integers(4 * w, cols, rows))
    val = rng.uniform(-1, 1, (rows, 5))
    return sp.csr_matrix((val.ravel(), col.ravel(), np.arange(0, 5 * rows + 1, 5)), shape=(rows, cols))


def kmax_case(pkg, extra):
    """(K + 37) x (K + extra), 5 entries a row, K = fused_kmax as dsvd_info reports it."""
    key = "kmax%d" % extra
    if key not in _cache:
        K = fused_kmax(pkg)
        _cache[key] = Case(pkg, five_a_row(K + 37, K + extra, 40 + extra))
    return _cache[key]


def fused_kmax(pkg):
    if "K" not in _cache:
        tiny = pkg.CSR.from_arrays([0, 1, 2], [0, 0], [1.0, 2.0], shape=(2, 1))
        _cache["K"] = pkg.SVDOp(tiny, "two_product").fused_kmax
    return _cache["K"]


def long_row_case(pkg):
    """400 x 350: row 5 has 300 entries (past the fused kernel's register
    budget: the re-read path), rows 0 and 399 are empty, column 7 is empty."""
    if "long" not in _cache:
        rng = np.random.default_rng(23)
        A = sp.random(400, 350, 0.02, random_state=rng, data_rvs=lambda c: rng.uniform(-1, 1, c),
                      format="lil")
        cols = np.setdiff1d(np.arange(350), [7])[:300]
        A[5, :] = 0.0
        A[5, cols] = rng.uniform(0.5, 1, 300)
        A[0, :] = 0.0
        A[399, :] = 0.0
        A[:, 7] = 0.0
        A = A.tocsr()
        A.eliminate_zeros()
        assert np.diff(A.indptr)[5] == 300 and 7 not in A.indices
        _cache["long"] = Case(pkg, A)
    return _cache["long"]


def apply_into(op, x, yb=None, pkg=None):
    xb = pkg.DeviceBuffer.from_numpy(x)
    yb = yb if yb is not None else pkg.DeviceBuffer(len(x))
    op.apply(xb, yb)
    return yb.numpy(), yb


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ------------------------------------------------------------ 1. rectangular SpMV
def _rect_spmv(pkg, c, Asp, dev):
    x = np.random.default_rng(5).uniform(-1, 1, Asp.shape[1])
    xb, yb = pkg.DeviceBuffer.from_numpy(x), pkg.DeviceBuffer(Asp.shape[0])
    yb.write(np.full(Asp.shape[0], 7.0))  # stale content must not survive
    dev.matvec_device(xb, yb)
    y, ref = yb.numpy(), Asp @ x
    print("rect spmv", Asp.shape, "kernel", dev.kernel, "max|y - ref|", np.abs(y - ref).max())
    if dev.kernel == 11:
        assert np.array_equal(bits(y), bits(ref))
        return True
    p = int(np.diff(Asp.indptr).max())
    assert np.all(np.abs(y - ref) <= gamma(p) * (abs(Asp) @ np.abs(x)))
    return False


@pytest.mark.parametrize("name", ["v2", "v3"])
def test_rect_spmv(pkg, golden, name):
    c = fixture_case(pkg, golden, name)
    assert c.dev.shape == (c.m, c.n) and c.dev.n == c.m
    _rect_spmv(pkg, c, c.A, c.dev)
    # the stored transpose's product, through the host transpose builder
    rp, col, val = pkg.csr_transpose(c.A.indptr, c.A.indices, c.A.data, c.A.shape)
    At = c.A.T.tocsr()
    At.sort_indices()
    Td = pkg.CSR.from_arrays(rp, col, val, shape=At.shape)
    _rect_spmv(pkg, c, At, Td)
    if name == "v3":  # rows of A' for the 22 empty columns of A: exactly 0
        empty = np.flatnonzero(np.bincount(c.A.indices, minlength=c.n) == 0)
        assert len(empty) == 22
        x = np.random.default_rng(6).uniform(-1, 1, c.m)
        yb = pkg.DeviceBuffer(c.n)
        yb.write(np.full(c.n, 3.0))
        Td.matvec_device(pkg.DeviceBuffer.from_numpy(x), yb)
        assert np.all(yb.numpy()[empty] == 0.0)


def test_rect_create_rejects_bad_input(pkg):
    with pytest.raises(RuntimeError):  # column 4 of a 2 x 4 matrix
        pkg.CSR.from_arrays([0, 1, 2], [0, 4], [1.0, 1.0], shape=(2, 4))
    with pytest.raises(RuntimeError):
        pkg.CSR.from_arrays([0, 1, 2], [0, 1], [1.0, 1.0], shape=(2, 0))


# ------------------------------------------------------- 2. normal product, both forms
def _check_product(pkg, c, form, expect_form):
    op = c.op(pkg, form)
    assert op.form == expect_form, (op.form, expect_form)
    assert (op.m, op.n, op.k) == (c.m, c.n, c.k)
    y, _ = apply_into(op, c.x1, pkg=pkg)
    yhat, bound = c.yhat(c.x1), c.bound(c.x1)
    err = np.abs(y - yhat)
    print("normal product", c.A.shape, op.form, "max err/bound",
          (err / np.maximum(bound, 1e-300)).max(), "p+q", c.pq)
    assert np.all(err <= bound)
    if op.form == "two_product":
        y2, _ = apply_into(op, c.x1, pkg=pkg)
        assert np.array_equal(bits(y), bits(y2))
        # bitwise yhat where both products run the SELL kernel (test 1's property)
        if "Td" not in c.__dict__:
            rp, col, val = pkg.csr_transpose(c.A.indptr, c.A.indices, c.A.data, c.A.shape)
            c.Td = pkg.CSR.from_arrays(rp, col, val, shape=(c.n, c.m))
        print("  kernels", c.dev.kernel, c.Td.kernel)
        if c.dev.kernel == 11 and c.Td.kernel == 11:
            assert np.array_equal(bits(y), bits(yhat))
    return op


@pytest.mark.parametrize("name", list(FIX))
def test_normal_two_product(pkg, golden, name):
    _check_product(pkg, fixture_case(pkg, golden, name), "two_product", "two_product")


@pytest.mark.parametrize("name", FUSED_OK)
def test_normal_fused(pkg, golden, name):
    _check_product(pkg, fixture_case(pkg, golden, name), "fused", "fused")


def test_normal_at_fused_kmax(pkg):
    K = fused_kmax(pkg)
    assert K == 10240
    c = kmax_case(pkg, 0)  # (K + 37) x K: the largest k the fused form serves
    _check_product(pkg, c, "auto", "fused")
    _check_product(pkg, c, "two_product", "two_product")


def test_normal_past_fused_kmax(pkg):
    c = kmax_case(pkg, 1)  # (K + 37) x (K + 1)
    _check_product(pkg, c, "auto", "two_product")
    with pytest.raises(pkg.ArpackError) as e:
        pkg.SVDOp(c.dev, "fused")
    assert e.value.info == -1


def test_fused_refused_for_v6(pkg, golden):
    c = fixture_case(pkg, golden, "v6")
    with pytest.raises(pkg.ArpackError) as e:
        pkg.SVDOp(c.dev, "fused")
    assert e.value.info == -1


# ------------------------------------------------------------- 3. no stale output
def _no_stale(pkg, c, form):
    op = c.op(pkg, form)
    _, yb = apply_into(op, c.x1, pkg=pkg)
    y2, _ = apply_into(op, c.x2, yb=yb, pkg=pkg)  # into the buffer that holds B'B x1
    fresh, _ = apply_into(op, c.x2, pkg=pkg)
    if form == "two_product":
        assert np.array_equal(bits(y2), bits(fresh))
    else:
        assert np.all(np.abs(y2 - fresh) <= c.bound(c.x2))
        assert np.all(np.abs(y2 - c.yhat(c.x2)) <= c.bound(c.x2))
    return y2


@pytest.mark.parametrize("form", ["two_product", "fused"])
@pytest.mark.parametrize("name", ["v2", "v3"])
def test_no_stale_output(pkg, golden, name, form):
    _no_stale(pkg, fixture_case(pkg, golden, name), form)


@pytest.mark.parametrize("form", ["two_product", "fused"])
def test_long_row_and_untouched_column(pkg, form):
    """One row of 300 entries (the fused kernel's re-read path), empty rows, and
    a column no row touches: its y is exactly 0 on every apply."""
    c = long_row_case(pkg)
    op = c.op(pkg, form)
    yb = pkg.DeviceBuffer(c.k)
    yb.write(np.full(c.k, 5.0))
    y1, _ = apply_into(op, c.x1, yb=yb, pkg=pkg)
    assert y1[7] == 0.0
    assert np.all(np.abs(y1 - c.yhat(c.x1)) <= c.bound(c.x1))
    y2 = _no_stale(pkg, c, form)
    assert y2[7] == 0.0


def test_untouched_columns_v6(pkg, golden):
    c = fixture_case(pkg, golden, "v6")
    empty = np.flatnonzero(np.bincount(c.A.indices, minlength=c.n) == 0)
    assert len(empty) == 20
    y2 = _no_stale(pkg, c, "two_product")
    assert np.all(y2[empty] == 0.0)


def test_vectors_zero_on_empty_columns_v3(pkg, golden):
    """v3 (200 x 1000): the long side's vectors B z / ||B z|| are exactly 0 in
    the rows of A's 22 empty columns, in a buffer that held other values."""
    c = fixture_case(pkg, golden, "v3")
    empty = np.flatnonzero(np.bincount(c.A.indices, minlength=c.n) == 0)
    z = c.g["z"]
    zb = pkg.DeviceBuffer.from_numpy(np.ascontiguousarray(z.T))
    for form in ("two_product", "fused"):
        sig, uo, res = c.op(pkg, form).vectors(c.g["d"], zb, c.k)
        assert uo.shape == (1000, len(c.g["d"]))
        assert np.all(uo[empty] == 0.0)
        assert np.allclose(sig, np.sqrt(c.g["d"]), rtol=1e-15, atol=0)


# ------------------------------------------------------------------ 4. solve parity
def _solve(pkg, c, form):
    g = c.g
    s = pkg.SymRci(c.k, int(g["nev"]), int(g["ncv"]), str(g["which"]), 0.0, v0=g["v0"], device=True)
    op = c.op(pkg, form)
    s.aupd_svd(op)
    return s, op


@pytest.mark.parametrize("form", ["auto", "two_product"])
@pytest.mark.parametrize("name", list(FIX))
def test_solve_parity(pkg, golden, name, form):
    c = fixture_case(pkg, golden, name)
    g = c.g
    s, op = _solve(pkg, c, form)
    if form == "auto":
        assert op.form == ("two_product" if name == "v6" else "fused")
    else:
        assert op.form == "two_product"
    print(name, op.form, "info", int(s.info[0]), "nconv", int(s.iparam[4]), "iters", int(s.iparam[2]),
          "nopx", int(s.iparam[8]), "ref", int(g["iparam"][2]), int(g["nopx"]))
    assert int(s.ido[0]) == 99
    assert int(s.info[0]) == int(g["info"])
    assert int(s.iparam[4]) == int(g["nconv"])
    assert int(s.iparam[2]) == int(g["iparam"][2])
    assert int(s.iparam[8]) == int(g["nopx"]) == int(g["iparam"][8])
    d, _, nconv = s.eupd()
    print("  max|d - d_ref| / max|d_ref|", np.abs(d - g["d"]).max() / np.abs(g["d"]).max())
    assert np.all(np.abs(d - g["d"]) <= 1e-10 * np.abs(g["d"]).max())


def test_solve_rejects_other_modes(pkg, golden):
    c = fixture_case(pkg, golden, "v5")
    op = c.op(pkg, "two_product")
    for kw, n in ((dict(mode=3), c.k), (dict(bmat="G", mode=2), c.k), (dict(), c.k + 1)):
        s = pkg.SymRci(n, 3, 12, "LM", 0.0, **kw)
        s.aupd_svd(op)
        assert int(s.ido[0]) == 99 and int(s.info[0]) == -11, (kw, n, s.info)


# ------------------------------------------------------------- 5. svds end to end
@pytest.mark.parametrize("name", FUSED_OK)
def test_svds(pkg, golden, name):
    c = fixture_case(pkg, golden, name)
    g = c.g
    if "sv" not in c.__dict__:
        c.sv = np.linalg.svd(c.A.toarray(), compute_uv=False)  # descending
    smax = c.sv[0]
    k, which = int(g["nev"]), str(g["which"])
    Uu, s, Vt, info = pkg.svds(c.dev, k=k, ncv=int(g["ncv"]), which=which, v0=g["v0"])
    assert info["form"] == "fused" and info["nconv"] == k and info["iters"] == int(g["iparam"][2])
    assert Uu.shape == (c.m, k) and Vt.shape == (k, c.n) and s.shape == (k,)
    assert np.all(np.diff(s) >= 0)  # ascending, as ARPACK returns the Ritz values
    ref = np.sort(c.sv[:k] if which == "LM" else c.sv[-k:])
    print(name, "max|s - s_numpy|/smax", np.abs(s - ref).max() / smax)
    assert np.all(np.abs(s - ref) <= 1e-10 * smax)
    r = np.linalg.norm(c.A.T @ Uu - Vt.T * s, axis=0).max()
    ou = np.abs(Uu.T @ Uu - np.eye(k)).max()
    ov = np.abs(Vt @ Vt.T - np.eye(k)).max()
    print("  max||A'u - s v||/smax", r / smax, "|U'U - I|", ou, "|VV' - I|", ov, "resid/smax",
          info["resid"].max() / smax)
    assert r <= 1e-10 * smax
    assert ou <= 1e-10 and ov <= 1e-10
    assert np.all(info["resid"] <= 1e-10 * smax)


def test_svds_values_only_and_scipy_input(pkg, golden):
    c = fixture_case(pkg, golden, "v5")
    g = c.g
    Uu, s, Vt, info = pkg.svds(c.A, k=3, ncv=12, v0=g["v0"], return_singular_vectors=False)
    assert Uu is None and Vt is None
    assert np.all(np.abs(s ** 2 - g["d"]) <= 1e-10 * np.abs(g["d"]).max())


# ----------------------------------------------------------- 6. deterministic mode
def test_svds_deterministic(pkg, golden):
    c = fixture_case(pkg, golden, "v2")
    g = c.g
    pkg.set_deterministic(True)
    try:
        runs = [pkg.svds(c.dev, k=int(g["nev"]), ncv=int(g["ncv"]), v0=g["v0"]) for _ in range(2)]
    finally:
        pkg.set_deterministic(False)
    (U1, s1, V1, i1), (U2, s2, V2, i2) = runs
    assert i1["form"] == "two_product" and i2["form"] == "two_product"
    assert i1["iters"] == int(g["iparam"][2])
    assert np.array_equal(bits(s1), bits(s2))
    assert np.array_equal(bits(U1), bits(U2))
    assert np.array_equal(bits(V1), bits(V2))


# --------------------------------------------------------------------- 7. refusals
def test_square_entries_refuse_rectangular(pkg, golden):
    """No kernel runs: the bad-argument codes come back before any work."""
    c = fixture_case(pkg, golden, "v5")  # 70 x 33
    with pytest.raises(RuntimeError):
        c.dev.set_symmetric(True)
    assert c.dev.last_rc == -1
    assert c.dev.sym_form == "full"
    with pytest.raises(pkg.ArpackError) as e:
        pkg.eigsh(c.dev, c.m, 3, 12)
    assert e.value.info == -1
    s = pkg.SymRci(c.m, 3, 12, "LM", 0.0)
    assert s.aupd_csr(c.dev) == 99 and int(s.info[0]) == -1
    s = pkg.NsRci(c.m, 3, 12, "LM", 0.0)
    assert s.aupd_csr(c.dev) == 99 and int(s.info[0]) == -1
    with pytest.raises(RuntimeError):
        pkg.DShift(c.dev, 0.5)


def test_square_through_rect_constructor_solves(pkg):
    """nrows == ncols through arpack_hip_csr_create_rect is a square operator."""
    n = 40
    T = sp.diags([np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0)], [-1, 0, 1]).tocsr()
    Sq = pkg.CSR.from_arrays(T.indptr, T.indices, T.data, shape=(n, n))
    d, _, res = pkg.eigsh(Sq, n, 3, 12, "LA")
    ref = np.sort(np.linalg.eigvalsh(T.toarray()))[-3:]
    assert np.all(np.abs(np.sort(d) - ref) <= 1e-10 * ref.max())
