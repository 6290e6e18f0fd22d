// Normal operator of the truncated SVD (EXAMPLES/SVD/dsvd.f: dsaupd on
// OP = A'A, sigma = sqrt(lambda), u = A v / ||A v||).
//
// A is m x n, k = min(m, n), B the tall orientation (B = A if m >= n, else A'),
// and the Lanczos problem is B'B on R^k.  Two forms of y = B'(B x):
//
//   two-product  w = B x, y = B' w with the stored transpose and the
//                full-storage kernels (csr_spmv): fixed order, bitwise
//                reproducible, any shape; streams the matrix twice.
//   fused        spmv_normal.hip: one pass over B.  x and y live in LDS
//                (2 x 8 B x k <= 160 KB, so k <= kNormalKmax = 10240, the
//                kSymWin of spmv_sym.hip); every workgroup writes its k-length
//                partial y to scratch and a second small kernel sums the
//                partials in block order.  The LDS adds run in wave-schedule
//                order: reproducible to rounding, not bitwise.
//
// Memory: B and B' are both resident (2 x 12 B an entry; the caller's A is one
// of them), the fused layout adds 10 B a stored entry, plus the partials
// (workgroups x k doubles) and one vector of B's rows.  The scratch belongs to
// the object: one stream per object at a time.
#pragma once
#include <cstdint>

#include "device.hpp"

struct arpack_hip_csr;

namespace ahip::dev {

// largest k the fused form serves: x and y windows of k doubles in the 160 KB
// of LDS a workgroup can have (163840 B / (2 * 8 B))
constexpr int kNormalKmax = 10240;
// entries of a row kept in registers between forming w_i and scattering
// a_ij w_i; a longer row is read a second time
constexpr int kNormalRegs = 32;

enum DSvdForm : int { kSvdAuto = 0, kSvdTwoProduct = 1, kSvdFused = 2 };

struct DSvd {
    int64_t m = 0, n = 0, k = 0, rows = 0;  // A is m x n; B is rows x k
    int form = kSvdTwoProduct;             // the form apply runs (never kSvdAuto)
    const arpack_hip_csr* B = nullptr;     // rows x k
    const arpack_hip_csr* Bt = nullptr;    // k x rows
    arpack_hip_csr* owned = nullptr;       // the one of B / Bt built here (the other is the caller's A)
    double* w = nullptr;                   // rows doubles: B x (two-product, dsvd_vectors)
    // fused layout (spmv_normal.hip): workgroup g walks slices
    // [f_slice0[g], f_slice0[g + 1]); slice s holds 64 rows, one a lane,
    // column-step-major, at f_val / f_col + f_ptr[s]; padding is (0.0, column 0)
    void* f_owned = nullptr;
    const int64_t* f_slice0 = nullptr;
    const int64_t* f_ptr = nullptr;
    const double* f_val = nullptr;
    const uint16_t* f_col = nullptr;
    int64_t f_nwg = 0, f_padded = 0;
    double* f_part = nullptr;  // f_nwg x k partial sums
};

// -1: bad argument (form 2 with k > kNormalKmax, a bad column index); -2: a HIP
// call or a plan failed.  A must outlive S.
int dsvd_create(DSvd& S, const arpack_hip_csr* A, int form);
void dsvd_destroy(DSvd& S);
// y = B'(B x), x and y device vectors of k doubles (x != y); enqueues on s.
// 0, or -2 when a launch failed.
int dsvd_apply(DSvd& S, hipStream_t s, const double* x, double* y);
// algorithmic HBM bytes of one apply in S's form
double dsvd_bytes(const DSvd& S);

// the fused layout and kernels (spmv_normal.hip)
int normal_build(DSvd& S, int64_t rows, int64_t k, const int64_t* rowptr, const int32_t* col,
                 const double* val);
void normal_apply(const DSvd& S, hipStream_t s, const double* x, double* y);

// Host transpose of an nrows x ncols CSR matrix by a stable counting sort:
// within each output row the entries keep increasing source-row order.
// trowptr: ncols + 1, tcol / tval: nnz.  -1 on a bad shape or column index.
int csr_transpose_host(int64_t nrows, int64_t ncols, const int64_t* rowptr, const int32_t* col,
                       const double* val, int64_t* trowptr, int32_t* tcol, double* tval);

// Post-processing of a converged solve (dsvd.f:416-450): for j < nconv,
// sigma_j = sqrt(max(d_j, 0)), the other side's vector B z_j / ||B z_j|| ->
// Uother(:, j) (rows long) and the residual ||B z_j - sigma_j u_j||.  d,
// sigma_out, resid_out host arrays; Z (k x nconv, ldz) and Uother (rows x
// nconv, ldu) device arrays.  0, -1 bad argument, -2 HIP error.
int dsvd_vectors(DSvd& S, int nconv, const double* d, const double* Z, int64_t ldz, double* sigma_out,
                 double* Uother, int64_t ldu, double* resid_out);

}  // namespace ahip::dev
