"""A/B of the fp32 CSR product (k_csr_sell_f32, 6 B a stored entry) against the
fp64 SELL product (10 B) of the SAME matrix, then one ssaupd free run against
one dsaupd free run of the same operator.

    python tools/spmv_f32_bench.py [--n N] [--m M] [--reps R] [--rounds K]
                                   [--out profiles/spmv_f32_ab.json]

Matrices: banded_sym at n = 10^6, 25 a row, and the 3-D Laplacian at m = 215
(multi-range windows).  Both have values exact in fp32 (checked), so the fp64
operator built by the generator and the fp32 one built from its downloaded
arrays are the same matrix.  Before any time counts, the fp32 product of each
is compared bit for bit with (A32 in fp64) @ (x in fp64) rounded to fp32.

Forms timed alternately, `rounds` times `reps` back-to-back launches each
(hipEvents, CSR.time_spmv): fp32 with 6 and with 4 column steps a chunk, fp64
SELL (the default kernel).  Algorithmic bytes of one product, the stored
entries plus the 4-B row map plus each vector once:
    fp32  6 nnz + 4 n + 4 n (x) + 4 n (y)
    fp64 10 nnz + 4 n + 8 n (x) + 8 n (y)
`hbm_fraction` = algorithmic bytes / time / 8 TB/s; the byte model promises at
most the ratio of the two byte counts.  The solves: nev = 10, ncv = 30, "LA",
tol = 1e-5 on the banded operator, device arrays, one warm-up solve then one
timed (host clock around the free run, which ends in a device synchronise);
cycles/s = restart cycles / time.  The dsaupd run takes its usual chained and
folded steps, the ssaupd run the plain ones.  Needs a GPU; there is no CPU
fallback for a time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_pkg  # noqa: E402
from oracle import matrices as M  # noqa: E402

HBM = 8.0e12  # B/s, MI355X peak
SELL = 11


def pair(pkg, A64):
    """(fp64 operator, fp32 operator of the same matrix, host arrays)."""
    rp, col, val = A64.download()
    v32 = val.astype(np.float32)
    exact = bool(np.array_equal(v32.astype(np.float64), val))
    A32 = pkg.CSR.from_arrays(rp, col, v32, dtype=np.float32)
    return A32, (rp, col, v32), exact


def check_bitwise(pkg, A32, arrs):
    rp, col, v32 = arrs
    x = np.random.default_rng(7).standard_normal(A32.n).astype(np.float32)
    ref = (M.to_scipy(rp, col, v32.astype(np.float64)) @ x.astype(np.float64)).astype(np.float32)
    xb, yb = pkg.DeviceBuffer.from_numpy(x), pkg.DeviceBuffer(A32.n, np.float32)
    for tile in (4, 6):
        A32.set_kernel(SELL, tile)
        A32.matvec_device(xb, yb)
        if not np.array_equal(yb.numpy().view(np.uint32), ref.view(np.uint32)):
            raise SystemExit("spmv_f32_bench: the fp32 product (U = %d) is not bitwise the contract's" % tile)


def product_ab(pkg, name, A64, reps, rounds):
    A32, arrs, exact = pair(pkg, A64)
    if A64.kernel != SELL or A32.kernel != SELL:
        raise SystemExit("spmv_f32_bench: %s did not plan the SELL form" % name)
    check_bitwise(pkg, A32, arrs)
    n, nnz = A64.n, A64.nnz
    forms = {"fp32_u6": (A32, 6), "fp32_u4": (A32, 4), "fp64_sell": (A64, None)}
    bytes_ = {"fp32_u6": 6.0 * nnz + 12.0 * n, "fp32_u4": 6.0 * nnz + 12.0 * n,
              "fp64_sell": 10.0 * nnz + 20.0 * n}
    times = {f: [] for f in forms}
    for _ in range(rounds):  # alternately: a drift of the box hits every form
        for f, (A, tile) in forms.items():
            if tile:
                A.set_kernel(SELL, tile)
            times[f].append(A.time_spmv(reps))
    A32.set_kernel(SELL, 6)
    out = dict(n=n, nnz=nnz, values_exact_in_fp32=exact, bitwise_checked=True, forms={})
    for f in forms:
        t = np.array(times[f])
        med = float(np.median(t))
        out["forms"][f] = dict(ms_median=med, ms_min=float(t.min()), ms_max=float(t.max()),
                               ms_rounds=[float(v) for v in t], algorithmic_bytes=bytes_[f],
                               bytes_per_s=bytes_[f] / (med * 1e-3),
                               hbm_fraction=bytes_[f] / (med * 1e-3) / HBM)
    best = min(("fp32_u6", "fp32_u4"), key=lambda f: out["forms"][f]["ms_median"])
    out["fp32_best"] = best
    out["fp32_speedup"] = out["forms"]["fp64_sell"]["ms_median"] / out["forms"][best]["ms_median"]
    out["byte_model_speedup"] = bytes_["fp64_sell"] / bytes_[best]
    return out, A32


def solve(pkg, A, prec, n, tol):
    def once():
        s = pkg.SymRci(n, 10, 30, "LA", tol, mxiter=3000, v0=np.linspace(-1, 1, n), device=True,
                       prec=prec)
        pkg.synchronize()
        t0 = time.perf_counter()
        s.aupd_csr(A)
        dt = time.perf_counter() - t0
        if int(s.info[0]) != 0:
            raise SystemExit("spmv_f32_bench: %ssaupd free run ended with info = %d" % (prec, s.info[0]))
        return s, dt
    once()  # warm-up: code objects, workspace
    s, dt = once()
    d = s.eupd(rvec=False)[0]
    return dict(seconds_to_converge=dt, cycles=int(s.iparam[2]), nconv=int(s.iparam[4]),
                opx=int(s.iparam[8]), cycles_per_s=int(s.iparam[2]) / dt,
                largest=float(np.max(d)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=215)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmv_f32_ab.json"))
    a = ap.parse_args()
    pkg = load_pkg()
    if pkg.device_count() < 1:
        raise SystemExit("spmv_f32_bench: no GPU -- a time is measured on the device or not at all")
    doc = dict(reps=a.reps, rounds=a.rounds, hbm_peak_bytes_per_s=HBM, matrices={})
    B64 = pkg.CSR.banded_sym(a.n, per_row=25)
    doc["matrices"]["banded_sym"], B32 = product_ab(pkg, "banded_sym", B64, a.reps, a.rounds)
    doc["solves"] = dict(workload="banded_sym n=%d, nev=10 ncv=30 LA tol=%g" % (a.n, a.tol),
                         ssaupd_f32=solve(pkg, B32, "s", a.n, a.tol),
                         dsaupd_f64=solve(pkg, B64, "d", a.n, a.tol))
    del B32, B64
    L64 = pkg.CSR.laplace3d(a.m)
    doc["matrices"]["laplace3d"], _ = product_ab(pkg, "laplace3d", L64, a.reps, a.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
