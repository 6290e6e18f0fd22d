// Truncated SVD on the device: the normal-operator object (dsvd.hpp) -- plan,
// two-product apply, post-processing -- and the host transpose builder.  The
// fused one-pass kernel is spmv_normal.hip.
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/arpack_hip.h"
#include "csr_internal.hpp"
#include "dsvd.hpp"

const ahip::dev::Csr* ahip_csr_view(const arpack_hip_csr* A);  // csr.hip

namespace ahip::dev {

namespace {
inline bool hok(hipError_t e) { return fault_filter(e) == hipSuccess; }

// AHIP_SVD_AUTO=fused / two: the form auto takes where both serve (same-box A/B)
int auto_form() {
    const char* e = getenv("AHIP_SVD_AUTO");
    if (e && e[0] == 't') return kSvdTwoProduct;
    if (e && e[0] == 'f') return kSvdFused;
    // the measured default (tools/svd_bench.py, profiles/svd_forms_ab.json;
    // DESIGN.md, the SVD section)
    return kSvdFused;
}
}  // namespace

int csr_transpose_host(int64_t nrows, int64_t ncols, const int64_t* rowptr, const int32_t* col,
                       const double* val, int64_t* trowptr, int32_t* tcol, double* tval) {
    if (nrows < 1 || ncols < 1 || nrows > (int64_t)INT32_MAX || !rowptr || !trowptr || rowptr[0] != 0)
        return -1;
    const int64_t nnz = rowptr[nrows];
    if (nnz < 0 || (nnz > 0 && (!col || !val || !tcol || !tval))) return -1;
    for (int64_t i = 0; i < nrows; ++i)
        if (rowptr[i + 1] < rowptr[i]) return -1;
    // counting sort on the column index: counts, exclusive scan, then the rows
    // in increasing order, so every output row keeps increasing source rows
    std::memset(trowptr, 0, sizeof(int64_t) * (size_t)(ncols + 1));
    for (int64_t k = 0; k < nnz; ++k) {
        if (col[k] < 0 || col[k] >= ncols) return -1;
        ++trowptr[col[k] + 1];
    }
    for (int64_t c = 0; c < ncols; ++c) trowptr[c + 1] += trowptr[c];
    std::vector<int64_t> next(trowptr, trowptr + ncols);
    for (int64_t i = 0; i < nrows; ++i)
        for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
            const int64_t p = next[col[k]]++;
            tcol[p] = (int32_t)i;
            tval[p] = val[k];
        }
    return 0;
}

int dsvd_create(DSvd& S, const arpack_hip_csr* A, int form) {
    S = DSvd{};
    if (!A || form < kSvdAuto || form > kSvdFused) return -1;
    const Csr& M = *ahip_csr_view(A);
    if (M.prec == 's') return -1;  // an fp32 operator: the normal operator is fp64
    const int64_t m = M.n, n = ahip_csr_ncols(A), nnz = M.nnz;
    if (m < 1 || n < 1 || m > (int64_t)INT32_MAX || n > (int64_t)INT32_MAX) return -1;
    const int64_t k = m < n ? m : n, rows = m < n ? n : m;
    if (form == kSvdFused && k > kNormalKmax) return -1;
    // the transpose, on the host (construction-time work, like the SpMV plans)
    std::vector<int64_t> rp((size_t)m + 1), trp((size_t)n + 1);
    std::vector<int32_t> col((size_t)nnz), tcol((size_t)nnz);
    std::vector<double> val((size_t)nnz), tval((size_t)nnz);
    if (!hok(hipMemcpy(rp.data(), M.rowptr, sizeof(int64_t) * (m + 1), hipMemcpyDeviceToHost)) ||
        (nnz > 0 && (!hok(hipMemcpy(col.data(), M.col, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost)) ||
                     !hok(hipMemcpy(val.data(), M.val, sizeof(double) * nnz, hipMemcpyDeviceToHost)))))
        return -2;
    // (a bad column index of a matrix that was registered unchecked stops here)
    if (csr_transpose_host(m, n, rp.data(), col.data(), val.data(), trp.data(), tcol.data(), tval.data()) != 0)
        return -1;
    arpack_hip_csr* T = nullptr;
    const int rc = arpack_hip_csr_create_rect(&T, n, m, nnz, trp.data(), tcol.data(), tval.data());
    if (rc != 0) return rc == -1 ? -2 : rc;  // (the arrays were checked: -1 here is the upload)
    S.owned = T;
    S.m = m;
    S.n = n;
    S.k = k;
    S.rows = rows;
    S.B = m >= n ? A : T;
    S.Bt = m >= n ? T : A;
    if (!hok(hipMalloc(&S.w, sizeof(double) * (size_t)rows))) {
        dsvd_destroy(S);
        return -2;
    }
    // deterministic mode (read here, as arpack_hip_csr_set_symmetric reads it
    // when the storage is chosen) always takes the fixed-order form
    int f = form;
    if (f == kSvdAuto) f = (k > kNormalKmax || deterministic()) ? kSvdTwoProduct : auto_form();
    S.form = f;
    if (f == kSvdFused) {
        const bool tall = m >= n;  // B's CSR arrays on the host
        const int brc = normal_build(S, rows, k, tall ? rp.data() : trp.data(),
                                     tall ? col.data() : tcol.data(), tall ? val.data() : tval.data());
        if (brc != 0) {
            dsvd_destroy(S);
            return brc;
        }
    }
    return 0;
}

void dsvd_destroy(DSvd& S) {
    if (S.owned) arpack_hip_csr_destroy(S.owned);
    if (S.w) (void)hipFree(S.w);
    if (S.f_owned) (void)hipFree(S.f_owned);
    if (S.f_part) (void)hipFree(S.f_part);
    S = DSvd{};
}

int dsvd_apply(DSvd& S, hipStream_t s, const double* x, double* y) {
    if (S.form == kSvdFused) {
        normal_apply(S, s, x, y);
    } else {
        csr_spmv(s, *ahip_csr_view(S.B), x, S.w);
        csr_spmv(s, *ahip_csr_view(S.Bt), S.w, y);
    }
    return hok(hipGetLastError()) ? 0 : -2;
}

double dsvd_bytes(const DSvd& S) {
    const double nnz = (double)ahip_csr_view(S.B)->nnz;
    if (S.form == kSvdFused)  // the matrix once, x, the partials written and read, y
        return 12.0 * nnz + 8.0 * (double)S.k * (2.0 + 2.0 * (double)S.f_nwg);
    return csr_bytes(*ahip_csr_view(S.B)) + csr_bytes(*ahip_csr_view(S.Bt));
}

int dsvd_vectors(DSvd& S, int nconv, const double* d, const double* Z, int64_t ldz, double* sigma_out,
                 double* Uother, int64_t ldu, double* resid_out) {
    if (nconv < 0 || !d || !Z || !sigma_out || !Uother || !resid_out || ldz < S.k || ldu < S.rows)
        return -1;
    if (nconv == 0) return 0;
    // the engine's norm: fixed-order partial sums (dots) + the kFinNorm finalize
    Workspace ws;
    hipStream_t st = nullptr;
    if (!hok(hipStreamCreate(&st))) return -2;
    if (!hok(ws_create(ws, S.rows, 2, st))) {
        (void)hipStreamDestroy(st);
        return -2;
    }
    const Csr& B = *ahip_csr_view(S.B);
    bool ok = hok(hipDeviceSynchronize());  // Z may come from another stream's work
    auto norm = [&](const double* x, double* out) {
        dots(ws, S.rows, 0, x, S.rows, x, x, -1);
        finalize(ws, 1, kFinNorm, 0, 0, -1);
        ok = ok && hok(hipMemcpyAsync(ws.st_host, ws.st, sizeof(LzState), hipMemcpyDeviceToHost, st)) &&
             hok(hipStreamSynchronize(st));
        *out = ws.st_host->rnorm;
    };
    for (int j = 0; j < nconv && ok; ++j) {
        const double sigma = std::sqrt(d[j] > 0.0 ? d[j] : 0.0);
        double* u = Uother + (int64_t)j * ldu;
        double nrm = 0.0, res = 0.0;
        csr_spmv(st, B, Z + (int64_t)j * ldz, S.w);  // t = B z_j
        copy<double>(st, S.rows, S.w, u);
        norm(u, &nrm);
        if (nrm > 0.0) scal<double>(st, S.rows, 1.0 / nrm, u);  // u_j = t / ||t||   (dsvd.f:416-431)
        axpby<double>(st, S.rows, 1.0, S.w, -sigma, u);        // t - sigma_j u_j  (dsvd.f:450)
        norm(S.w, &res);
        sigma_out[j] = sigma;
        resid_out[j] = res;
    }
    ok = ok && hok(hipStreamSynchronize(st)) && hok(hipGetLastError());
    ws_destroy(ws);
    (void)hipStreamDestroy(st);
    return ok ? 0 : -2;
}

}  // namespace ahip::dev
