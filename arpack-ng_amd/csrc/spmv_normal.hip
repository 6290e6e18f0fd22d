// Fused normal-operator product y = B'(B x) of the truncated SVD (dsvd.hpp):
// B (rows x k, tall) is streamed ONCE, where w = B x, y = B' w streams it twice.
//
// The idea is spmv_sym.hip's: gather x from an LDS window, scatter the
// transposed terms into an LDS y window.  Here both windows are the whole
// vectors (k <= kNormalKmax = 10240 doubles each, 2 x 80 KB = the 160 KB of
// LDS), so a workgroup needs nothing from any other:
//
//   k_normal_fused  workgroup g stages x into LDS, zeroes its LDS y, and walks
//                   its slices (SELL-64: 64 rows, one a lane, column-step-major
//                   so a wave reads 64 consecutive values, 8 B value + 2 B
//                   column).  A lane forms w_i = sum_k a_ik x_k with its row's
//                   entries held in registers (rows of <= kNormalRegs entries;
//                   a longer row is read a second time), then adds a_ij w_i
//                   into y_lds[j] (LDS fp64 atomics, wave-schedule order).  The
//                   workgroup's k-length partial goes to part[g].
//   k_normal_sum    y_j = sum_g part[g][j] in block order g = 0, 1, ...; every
//                   y_j is written (a column no row touches gives 0).
//
// No workgroup waits on another: no grid barrier, no flag, two launches.
// Row order does not matter to either sum, so the layout drops empty rows and
// sorts each workgroup's rows by length (less padding); nothing maps a lane
// back to its row.  Padding entries are (0.0, column 0) and are not scattered.
//
// Byte model of one apply: 10 B a stored entry (12 B counted as algorithmic:
// the CSR's 4-B index) + 8 k (x, per workgroup from L2) + 2 x 8 k nwg (the
// partials written and read) + 8 k (y).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "dsvd.hpp"

namespace ahip::dev {

namespace {

inline bool hok(hipError_t e) { return fault_filter(e) == hipSuccess; }

constexpr int kNrmThreads = 1024;
constexpr int kNrmWaves = kNrmThreads / 64;
// slices a workgroup walks at least (two a wave), and the grid's cap (two
// workgroups a CU at k <= 5120): bounds the partials' traffic, 16 k nwg bytes
constexpr int64_t kNrmMinSlices = 32;
constexpr int64_t kNrmMaxWg = 512;

// one slice of width w <= W, its entries in registers between the two sums
template <int W>
__device__ __forceinline__ void slice_regs(const double* __restrict__ sv, const uint16_t* __restrict__ sc,
                                           int w, const double* xw, double* yw) {
    double v[W];
    int c[W];
#pragma unroll
    for (int u = 0; u < W; ++u) {
        const bool in = u < w;
        v[u] = in ? __builtin_nontemporal_load(sv + u * 64) : 0.0;
        c[u] = in ? (int)__builtin_nontemporal_load(sc + u * 64) : 0;
    }
    double wi = 0.0;
#pragma unroll
    for (int u = 0; u < W; ++u) wi += v[u] * xw[c[u]];
#pragma unroll
    for (int u = 0; u < W; ++u)
        if (v[u] != 0.0) atomicAdd(&yw[c[u]], v[u] * wi);
}

__global__ __launch_bounds__(kNrmThreads) void k_normal_fused(
    const int64_t* __restrict__ slice0, const int64_t* __restrict__ sptr,
    const double* __restrict__ sval, const uint16_t* __restrict__ scol, const double* __restrict__ x,
    double* __restrict__ part, int k) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* xw = lds;
    double* yw = lds + k;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    for (int i = t; i < k; i += kNrmThreads) {
        xw[i] = x[i];
        yw[i] = 0.0;
    }
    __syncthreads();
    const int64_t s1 = slice0[blockIdx.x + 1];
    for (int64_t s = slice0[blockIdx.x] + wave; s < s1; s += kNrmWaves) {
        const int64_t base = sptr[s];
        const int w = (int)((sptr[s + 1] - base) >> 6);
        const double* sv = sval + base + lane;
        const uint16_t* sc = scol + base + lane;
        if (w <= 4) slice_regs<4>(sv, sc, w, xw, yw);
        else if (w <= 8) slice_regs<8>(sv, sc, w, xw, yw);
        else if (w <= 16) slice_regs<16>(sv, sc, w, xw, yw);
        else if (w <= kNormalRegs) slice_regs<kNormalRegs>(sv, sc, w, xw, yw);
        else {
            // a row past the register budget: w_i first, then the row again
            // (from L2, it was just read) for the scatter
            double wi = 0.0;
            for (int k0 = 0; k0 < w; k0 += 8) {
                double v[8];
                int c[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const bool in = k0 + u < w;
                    v[u] = in ? sv[(int64_t)(k0 + u) * 64] : 0.0;
                    c[u] = in ? (int)sc[(int64_t)(k0 + u) * 64] : 0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) wi += v[u] * xw[c[u]];
            }
            for (int k0 = 0; k0 < w; k0 += 8) {
                double v[8];
                int c[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const bool in = k0 + u < w;
                    v[u] = in ? sv[(int64_t)(k0 + u) * 64] : 0.0;
                    c[u] = in ? (int)sc[(int64_t)(k0 + u) * 64] : 0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (v[u] != 0.0) atomicAdd(&yw[c[u]], v[u] * wi);
            }
        }
    }
    __syncthreads();
    double* p = part + (int64_t)blockIdx.x * k;
    for (int i = t; i < k; i += kNrmThreads) p[i] = yw[i];
}

__global__ __launch_bounds__(256) void k_normal_sum(const double* __restrict__ part, int64_t nwg, int k,
                                                    double* __restrict__ y) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    double s = 0.0;
    for (int64_t g = 0; g < nwg; ++g) s += part[g * k + j];
    y[j] = s;
}

}  // namespace

int normal_build(DSvd& S, int64_t rows, int64_t k, const int64_t* rp, const int32_t* col,
                 const double* val) {
    if (k < 1 || k > kNormalKmax || rows < 1) return -1;
    // every index the kernel gathers or scatters with is checked here
    for (int64_t i = 0; i < rows; ++i)
        if (rp[i + 1] < rp[i]) return -1;
    for (int64_t q = 0; q < rp[rows]; ++q)
        if (col[q] < 0 || col[q] >= k) return -1;
    std::vector<int32_t> live;  // the rows with entries
    for (int64_t i = 0; i < rows; ++i)
        if (rp[i + 1] > rp[i]) live.push_back((int32_t)i);
    const int64_t nlive = (int64_t)live.size(), nsl = (nlive + 63) / 64;
    const int64_t per = std::max<int64_t>(kNrmMinSlices, (nsl + kNrmMaxWg - 1) / kNrmMaxWg);
    const int64_t nwg = std::max<int64_t>(1, (nsl + per - 1) / per);
    auto len = [&](int32_t r) { return rp[r + 1] - rp[r]; };
    std::vector<int64_t> slice0{0}, sptr{0};
    for (int64_t g = 0; g < nwg; ++g) {
        const int64_t a = std::min(nlive, g * per * 64), b = std::min(nlive, (g + 1) * per * 64);
        // longest rows first (stable): a slice's width is its first row's length
        std::stable_sort(live.begin() + a, live.begin() + b,
                         [&](int32_t p, int32_t q) { return len(p) > len(q); });
        for (int64_t q = a; q < b; q += 64) sptr.push_back(sptr.back() + 64 * len(live[q]));
        slice0.push_back((int64_t)sptr.size() - 1);
    }
    const int64_t ns = (int64_t)sptr.size() - 1, padded = sptr.back();
    std::vector<double> sv((size_t)(padded ? padded : 1), 0.0);
    std::vector<uint16_t> sc((size_t)(padded ? padded : 1), 0);
    for (int64_t s = 0; s < ns; ++s)
        for (int64_t l = 0; l < 64 && s * 64 + l < nlive; ++l) {
            // (slices are 64 consecutive entries of `live`: every workgroup but
            // the last holds a multiple of 64 rows)
            const int32_t r = live[s * 64 + l];
            for (int64_t q = rp[r]; q < rp[r + 1]; ++q) {
                sv[sptr[s] + (q - rp[r]) * 64 + l] = val[q];
                sc[sptr[s] + (q - rp[r]) * 64 + l] = (uint16_t)col[q];
            }
        }
    const size_t b0 = sizeof(int64_t) * slice0.size(), b1 = sizeof(int64_t) * sptr.size(),
                 bv = sizeof(double) * sv.size(), bc = sizeof(uint16_t) * sc.size();
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    char* d = nullptr;
    if (!hok(hipMalloc(&d, up(b0) + up(b1) + up(bv) + up(bc)))) return -2;
    char* p0 = d;
    char* p1 = p0 + up(b0);
    char* pv = p1 + up(b1);
    char* pc = pv + up(bv);
    double* part = nullptr;
    if (!hok(hipMemcpy(p0, slice0.data(), b0, hipMemcpyHostToDevice)) ||
        !hok(hipMemcpy(p1, sptr.data(), b1, hipMemcpyHostToDevice)) ||
        !hok(hipMemcpy(pv, sv.data(), bv, hipMemcpyHostToDevice)) ||
        !hok(hipMemcpy(pc, sc.data(), bc, hipMemcpyHostToDevice)) ||
        !hok(hipMalloc(&part, sizeof(double) * (size_t)(nwg * k)))) {
        (void)hipFree(d);
        return -2;
    }
    S.f_owned = d;
    S.f_slice0 = (const int64_t*)p0;
    S.f_ptr = (const int64_t*)p1;
    S.f_val = (const double*)pv;
    S.f_col = (const uint16_t*)pc;
    S.f_nwg = nwg;
    S.f_padded = padded;
    S.f_part = part;
    return 0;
}

void normal_apply(const DSvd& S, hipStream_t s, const double* x, double* y) {
    const int k = (int)S.k;
    const size_t lds = sizeof(double) * 2 * (size_t)k;
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void*)k_normal_fused, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(sizeof(double) * 2 * kNormalKmax));
        attr = true;
    }
    AHIP_LAUNCH(k_normal_fused, dim3((unsigned)S.f_nwg), dim3(kNrmThreads), lds, s, S.f_slice0, S.f_ptr,
                S.f_val, S.f_col, x, S.f_part, k);
    AHIP_LAUNCH(k_normal_sum, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, s,
                (const double*)S.f_part, S.f_nwg, k, y);
}

}  // namespace ahip::dev
