"""A/B of the SVD normal operator's two forms (SVDOp.time) on a tall-skinny
matrix: two-product (w = B x, y = B' w: the matrix streamed twice) against
fused (spmv_normal.hip: streamed once, x and y in LDS).

    python tools/svd_bench.py [--rows M] [--cols N] [--per-row P] [--reps R] [--rounds K]
                              [--out profiles/svd_forms_ab.json]

The generator: M rows of P entries, one column drawn from each P-th of the N
columns (distinct, sorted), values U(-1, 1), default_rng(seed).  The defaults
put 12 B x nnz well past the 256 MB Infinity Cache, so both forms stream from
HBM.  The forms are timed alternately, `rounds` times `reps` applies each
(device events around back-to-back applies), and one apply of each is checked
against SciPy's Bt @ (B @ x) with the tests' bound before any time counts.

Algorithmic bytes of one apply: fused 12 nnz + 16 n (the matrix once, x, y);
two-product 2 x 12 nnz + 16 m + 16 n (B and B', w written and read, x, y).
`hbm_fraction` = algorithmic bytes / time / 8 TB/s.  Needs a GPU; there is no
CPU fallback for a time.
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_pkg  # noqa: E402

HBM = 8.0e12  # B/s, MI355X peak


def tall_skinny(m, n, per_row, seed):
    rng = np.random.default_rng(seed)
    w = n // per_row
    col = (np.arange(per_row, dtype=np.int64)[None, :] * w + rng.integers(0, w, (m, per_row)))
    val = rng.uniform(-1, 1, (m, per_row))
    rp = np.arange(0, per_row * m + 1, per_row, dtype=np.int64)
    return sp.csr_matrix((val.ravel(), col.ravel().astype(np.int32), rp), shape=(m, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--cols", type=int, default=4096)
    ap.add_argument("--per-row", type=int, default=10)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svd_forms_ab.json"))
    a = ap.parse_args()
    pkg = load_pkg()
    if pkg.device_count() < 1:
        raise SystemExit("svd_bench: no GPU -- a time is measured on the device or not at all")
    B = tall_skinny(a.rows, a.cols, a.per_row, a.seed)
    m, n, nnz = B.shape[0], B.shape[1], int(B.nnz)
    A = pkg.CSR.from_arrays(B.indptr, B.indices, B.data, shape=B.shape)
    ops = {f: pkg.SVDOp(A, f) for f in ("two_product", "fused")}
    # both forms compute the same thing, at this size, before any time counts
    x = np.random.default_rng(1).uniform(-1, 1, n)
    Bt = B.T.tocsr()
    yhat = Bt @ (B @ x)
    p, q = int(np.diff(B.indptr).max()), int(np.diff(Bt.indptr).max())
    u = 2.0 ** -53
    bound = 2.0 * ((p + q) * u / (1.0 - (p + q) * u)) * (abs(Bt) @ (abs(B) @ np.abs(x)))
    err = {}
    for f, op in ops.items():
        e = np.abs(op.apply(x) - yhat)
        err[f] = float((e / np.maximum(bound, 1e-300)).max())
        if not np.all(e <= bound):
            raise SystemExit("svd_bench: form %s misses the bound (%g)" % (f, err[f]))
    times = {f: [] for f in ops}
    for _ in range(a.rounds):  # alternately: a drift of the box hits both forms
        for f, op in ops.items():
            times[f].append(op.time(a.reps))
    bytes_ = {"fused": 12.0 * nnz + 16.0 * n, "two_product": 24.0 * nnz + 16.0 * m + 16.0 * n}
    doc = dict(workload=dict(workload="svd_tall_skinny", m=m, n=n, nnz=nnz, per_row=a.per_row,
                             seed=a.seed, kernels=dict(B=A.kernel)),
               reps=a.reps, rounds=a.rounds, hbm_peak_bytes_per_s=HBM, forms={})
    for f in ops:
        t = np.array(times[f])
        med = float(np.median(t))
        doc["forms"][f] = dict(ms_median=med, ms_min=float(t.min()), ms_max=float(t.max()),
                               ms_rounds=[float(v) for v in t], algorithmic_bytes=bytes_[f],
                               bytes_per_s=bytes_[f] / (med * 1e-3),
                               hbm_fraction=bytes_[f] / (med * 1e-3) / HBM,
                               err_over_bound=err[f])
    doc["fused_speedup"] = doc["forms"]["two_product"]["ms_median"] / doc["forms"]["fused"]["ms_median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
