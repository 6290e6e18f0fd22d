"""Generate the truncated-SVD fixtures (tests/golden/v*.npz) from the REAL
reference (oracle/_ref).

Run in the build container (where the reference is built), like make_golden.py:
    make -C oracle && python tests/golden/make_golden_svd.py

A is m x n, k = min(m, n) and B the tall orientation (B = A if m >= n, else
A').  Each fixture holds the CSR arrays of A, the start vector v0 =
default_rng(2).uniform(-1, 1, k), and the reference's dsaupd/dseupd on
OP = B'(B x) with SciPy's products at tol = 0 (the calling pattern of
EXAMPLES/SVD/dsvd.f): info, nconv, iparam, nopx, d, z.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def dsvd_matrix(m, n):
    """The operator of EXAMPLES/SVD/dsvd.f (its comment, dsvd.f:518-523): the
    discretised kernel K(s,t) = s(t-1) for s <= t, t(s-1) otherwise, A(i,j) =
    k si (tj - 1) for i <= j and k tj (si - 1) for i > j with si = i/(m+1),
    tj = j/(n+1), k = 1/(n+1); stored dense as CSR."""
    s = np.arange(1, m + 1, dtype=np.float64)[:, None] / (m + 1)
    t = np.arange(1, n + 1, dtype=np.float64)[None, :] / (n + 1)
    k = 1.0 / (n + 1)
    i = np.arange(1, m + 1)[:, None]
    j = np.arange(1, n + 1)[None, :]
    return sp.csr_matrix(np.where(i <= j, k * s * (t - 1.0), k * t * (s - 1.0)))


def random_matrix(m, n, density, seed):
    rng = np.random.default_rng(seed)
    return sp.random(m, n, density, random_state=rng, data_rvs=lambda c: rng.uniform(-1, 1, c),
                     format="csr")


CASES = [
    # name, matrix, nev, ncv, which
    ("v1_dsvd", lambda: dsvd_matrix(500, 100), 4, 10, "LM"),
    ("v2_tall_257", lambda: random_matrix(3000, 257, 0.02, 3), 5, 20, "LM"),
    ("v3_wide_200", lambda: random_matrix(200, 1000, 0.02, 4), 4, 16, "LM"),
    ("v4_slice_sm", lambda: random_matrix(1000, 64, 0.1, 5), 3, 12, "SM"),
    ("v5_small", lambda: random_matrix(70, 33, 0.3, 6), 3, 12, "LM"),
    ("v6_two_product", lambda: random_matrix(13000, 12000, 0.0005, 8), 4, 16, "LM"),
]


def run(name, A, nev, ncv, which):
    A = A.tocsr()
    A.sort_indices()
    m, n = A.shape
    k = min(m, n)
    B = A if m >= n else A.T.tocsr()
    Bt = B.T.tocsr()
    v0 = np.random.default_rng(2).uniform(-1, 1, k)
    r = ref.dsaupd_solve(lambda x, *_: Bt @ (B @ x), k, nev, ncv, which, 0.0, v0=v0)
    assert r["info"] >= 0, r
    # (z of the largest case is left out: the file stays under the 1 MB limit)
    z = r["z"] if k <= 4096 else np.zeros((0, 0))
    np.savez_compressed(
        os.path.join(OUT, name + ".npz"), shape=np.array([m, n], np.int64),
        rowptr=A.indptr.astype(np.int64), col=A.indices.astype(np.int32),
        val=A.data.astype(np.float64), v0=v0, nev=nev, ncv=ncv, which=np.array(which),
        info=r["info"], nconv=r["nconv"], iparam=r["iparam"], nopx=r["stats"]["nopx"], d=r["d"],
        z=z)
    print(name, A.shape, "nnz", A.nnz, "info", r["info"], "iters", int(r["iparam"][2]), "nopx",
          r["stats"]["nopx"], "empty rows", int((np.diff(A.indptr) == 0).sum()), "empty cols",
          int((np.bincount(A.indices, minlength=n) == 0).sum()))


if __name__ == "__main__":
    for name, mk, nev, ncv, which in CASES:
        run(name, mk(), nev, ncv, which)
