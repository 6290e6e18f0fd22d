// Symmetric implicitly restarted Lanczos: the dsaupd -> dsaup2 -> dsaitr /
// dgetv0 / dsapps control flow, re-hosted as coroutines that drive the HIP
// kernels of kernels.hip.  Host work is O(ncv^2) per restart cycle; all
// n-length data stays in HBM.
//
// Reference map:
//   Solver::run    SRC/dsaupd.f:408-690 + SRC/dsaup2.f:179-851
//   Solver::saitr  SRC/dsaitr.f:204-853   (Lanczos steps, CGS + DGKS)
//   Solver::getv0  SRC/dgetv0.f:119-421   (start / restart vector)
//   Solver::sapps  SRC/dsapps.f:131-518   (shifts on T host-side, V*Q on device)
#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "engine.hpp"

namespace ahip {

// ------------------------------------------------------------------ Arrays ---

bool is_device_pointer(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

template <class R>
int ArraysT<R>::attach(int64_t nn, int nc, R* resid, R* v, int ldv, R* workd) {
    n = nn;
    ncv = nc;
    const bool dr = is_device_pointer(resid), dv = is_device_pointer(v), dw = is_device_pointer(workd);
    if (dr != dv || dv != dw) return -1;
    host_mode = !dr;
    h_resid = resid;
    h_v = v;
    h_ldv = ldv;
    h_workd = workd;
    stream = default_stream();
    if (!stream) {
        if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return -2;
        own_stream = true;
    }
    if (host_mode) {
        // columns start on 128-B lines: an odd n (config 4's 215^3) put every
        // other column off a line and cost the V passes 8-12% (profiles/r03am)
        constexpr int64_t al = 128 / (int64_t)sizeof(R);
        d_ld = (n + al - 1) / al * al;
        if (hipMalloc(&d_v, sizeof(R) * (size_t)d_ld * ncv) != hipSuccess) return -2;
        if (hipMalloc(&d_resid, sizeof(R) * (size_t)n) != hipSuccess) return -2;
        if (hipMalloc(&d_workd, sizeof(R) * 3 * (size_t)n) != hipSuccess) return -2;
        ck(hipMemsetAsync(d_v, 0, sizeof(R) * (size_t)d_ld * ncv, stream));
        ck(hipMemsetAsync(d_workd, 0, sizeof(R) * 3 * (size_t)n, stream));
        ck(hipMemsetAsync(d_resid, 0, sizeof(R) * (size_t)n, stream));
    } else {
        d_v = v;
        d_ld = ldv;
        d_resid = resid;
        d_workd = workd;
        // device-pointer mode: the caller may have written V, resid (info = 1)
        // or workd with its own GPU work on any stream, still in flight -- the
        // engine's non-blocking stream does not order behind it, and the RCI
        // contract (SRC/dsaupd.f:228-234) is that the arrays are complete when
        // *aupd / *eupd is called: make it so before the engine touches them
        ck(hipDeviceSynchronize());
    }
    return 0;
}

template <class R>
void ArraysT<R>::release() {
    if (host_mode) {
        if (d_v) (void)hipFree(d_v);
        if (d_resid) (void)hipFree(d_resid);
        if (d_workd) (void)hipFree(d_workd);
    }
    if (own_stream && stream) (void)hipStreamDestroy(stream);
    d_v = d_resid = d_workd = nullptr;
    stream = nullptr;
    own_stream = false;
}

template <class R>
void ArraysT<R>::upload_resid() {
    if (host_mode) ck(hipMemcpyAsync(d_resid, h_resid, sizeof(R) * n, hipMemcpyHostToDevice, stream));
}

template <class R>
void ArraysT<R>::d2h_workd(int64_t off, int64_t len) {
    if (host_mode && off >= 0)
        ck(hipMemcpyAsync(h_workd + off, d_workd + off, sizeof(R) * len, hipMemcpyDeviceToHost, stream));
}

template <class R>
void ArraysT<R>::h2d_workd(int64_t off, int64_t len) {
    if (host_mode && off >= 0)
        ck(hipMemcpyAsync(d_workd + off, h_workd + off, sizeof(R) * len, hipMemcpyHostToDevice, stream));
    // device-pointer mode: the caller produced workd(off) with its own GPU work,
    // possibly still in flight on another stream (the engine's stream does not
    // order against them) -- the reverse-communication contract is that the
    // request is complete when *aupd is called again, so make it so
    if (!host_mode && off >= 0) ck(hipDeviceSynchronize());
}

template <class R>
void ArraysT<R>::download_all() {
    if (!host_mode) return;
    ck(hipMemcpy2DAsync(h_v, sizeof(R) * h_ldv, d_v, sizeof(R) * d_ld, sizeof(R) * n, ncv,
                        hipMemcpyDeviceToHost, stream));
    ck(hipMemcpyAsync(h_resid, d_resid, sizeof(R) * n, hipMemcpyDeviceToHost, stream));
    ck(hipMemcpyAsync(h_workd, d_workd, sizeof(R) * 3 * n, hipMemcpyDeviceToHost, stream));
}

template <class R>
void ArraysT<R>::sync() {
    dev::flush_deferred_finalize(defq, stream);  // (none outlives a sync)
    ck(hipStreamSynchronize(stream));
}

// ------------------------------------------------------------- Solver ---

template <class R>
SolverT<R>::~SolverT() {
    // no kernel of this solve may still be writing the caller's arrays
    if (op_stream) (void)hipStreamSynchronize(op_stream);
    if (a.stream) (void)hipStreamSynchronize(a.stream);
    if (x_ev) (void)hipEventDestroy(x_ev);
    if (y_ev) (void)hipEventDestroy(y_ev);
    if (op_stream) (void)hipStreamDestroy(op_stream);
    if (ybuf) (void)hipFree(ybuf);
    root.reset();
    dev::ws_destroy(ws);
    a.release();
}

// The overlapped distributed SpMV (opt-in, AHIP_DIST_OVERLAP=1) needs RCCL's
// separate p2p communicator.  Off by default: measured on a 1-rank RCCL
// communicator at a rank's share of the north star (1.25e6 rows), the two
// cross-stream event waits per step cost ~20 us of scheduling latency
// (255-282 vs 301-313 cycles/s) -- about what an 8-rank allreduce + finalize
// would hide, so the overlap cannot be shown to pay without a multi-GPU run.
template <class R>
bool SolverT<R>::overlap_ready() {
    static const bool off = [] {
        const char* e = getenv("AHIP_DIST_OVERLAP");
        return !(e && e[0] == '1');
    }();
    if (off || !dist || !dist->A || !comm_has_p2p(dist->comm)) return false;
    if (!op_stream) {
        if (hipStreamCreateWithFlags(&op_stream, hipStreamNonBlocking) != hipSuccess) {
            op_stream = nullptr;
            return false;
        }
        if (hipEventCreateWithFlags(&x_ev, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&y_ev, hipEventDisableTiming) != hipSuccess)
            return false;
    }
    return x_ev && y_ev;
}

template <class R>
bool SolverT<R>::check_halt() {
    bool bad = a.err.bad();
    if (dist && comm_size(dist->comm) > 1) bad = !dist_all_ok(dist->comm, !bad);
    halted = halted || bad;
    return halted;
}

template <class R>
RciAwait SolverT<R>::rci(int ido, int64_t x, int64_t y, int64_t bx) {
    op_x = nullptr;
    op_y = nullptr;
    return RciAwait{&ctx, RciReq{ido, x, y, bx}};
}

template <class R>
RciAwait SolverT<R>::op(int ido, int64_t x, int64_t y, int64_t bx, const R* xp, R* yp) {
    op_x = xp;
    op_y = yp;
    return RciAwait{&ctx, RciReq{ido, x, y, bx}};
}

// The second DGKS refinement of step j (SRC/dsaitr.f:753-781), gated on the
// device decision, and the give-up zeroing of r.
template <class R>
void SolverT<R>::dgks2_tail(int j, int rstart) {
    dev::update(ws, (int64_t)n, j, a.d_v, a.d_ld, 2, a.d_resid, a.d_resid, true, 2);
    fin(j + 1, dev::kFinDgks2, j, rstart, 2);
    dev::zero_if(ws, (int64_t)n, a.d_resid);
}

template <class R>
R* SolverT<R>::dist_x() {
    if constexpr (std::is_same_v<R, double>)
        return (dist && dist->x_ext) ? dist->x_mid() : nullptr;
    else
        return nullptr;  // the float family runs on one GPU
}

// Finalize of a reduction; with a multi-GPU distribution the local sums are
// allreduced across ranks (one RCCL collective) before the phase logic runs.
template <class R>
void SolverT<R>::fin(int m, dev::FinPhase ph, int j, int rstart, int gate, int m2, int rstart_prev,
                     bool defer) {
    if (dist && dist->comm) {
        dev::finalize(ws, m, dev::kFinRaw, j, rstart, gate, false, m2);
        comm_allreduce_sum(dist->comm, ws.sums, m + m2, a.stream);
        // the phase logic on the allreduced sums may ride in the next SpMV too
        // (not with the overlapped SpMV: that one runs on op_stream)
        if (ph != dev::kFinRaw)
            dev::finalize(ws, m, ph, j, rstart, gate, true, m2, rstart_prev, defer && !op_stream);
    } else {
        dev::finalize(ws, m, ph, j, rstart, gate, false, m2, rstart_prev, defer);
    }
}

template <class R>
void SolverT<R>::read_state() {
    dev::flush_deferred_finalize(ws.defq, a.stream);
    a.ck(hipMemcpyAsync(ws.st_host, ws.st, sizeof(dev::LzState), hipMemcpyDeviceToHost, a.stream));
    a.sync();
}

template <class R>
void SolverT<R>::write_state() {
    a.ck(hipMemcpyAsync(ws.st, ws.st_host, sizeof(dev::LzState), hipMemcpyHostToDevice, a.stream));
}

// dgetv0: generate (or take) a start vector, force it into range(OP), and for
// j > 1 B-orthogonalise it against V(:,1:j-1) with <= 5 refinement sweeps.
// On exit st.rnorm and this->rnorm hold its B-norm.
template <class R>
Task SolverT<R>::getv0(bool initv, int j, int itry, int& ierr) {
    const int64_t nn = n;
    R* wd = a.d_workd;
    ierr = 0;
    if (!initv) {  // dlarnv(idist=2, iseed, n, resid) — SRC/dgetv0.f:234-237
        constexpr char fam = std::is_same_v<R, double> ? 'd' : 's';
        if (dist && dist->seed_mode == 1) {
            // PARPACK: each rank draws its n local values from its own stream
            // (PARPACK/SRC/MPI/pdgetv0.f:234-245, 276)
            uint64_t& sd = pgetv0_seed(fam, comm_rank(dist->comm));
            sd = dev::larnv_uniform(ws, nn, sd, a.d_resid, 0);
        } else {  // one stream; a rank takes its rows' slice (P-invariant start)
            uint64_t& sd = getv0_seed(fam);
            const uint64_t s1 = dev::larnv_uniform(ws, nn, sd, a.d_resid, row0);
            sd = dist ? lcg_advance(sd, (uint64_t)dist->n_global) : s1;
        }
    }
    if (itry == 1) {  // force into the range of OP (SRC/dgetv0.f:245-251)
        g_stats.nopx += 1;
        dev::copy(a.stream, nn, a.d_resid, wd);
        co_await op(-1, 0, nn, -1, wd, wd + nn);
        dev::copy(a.stream, nn, wd + nn, a.d_resid);
    } else if (bmat == 'G') {
        dev::copy(a.stream, nn, a.d_resid, wd + nn);
    }
    // B-norm of the start vector (SRC/dgetv0.f:279-306)
    if (bmat == 'G') {
        g_stats.nbx += 1;
        if (itry == 1) dev::copy(a.stream, nn, a.d_resid, wd + nn);
        co_await rci(2, nn, 0);
    } else {
        dev::copy(a.stream, nn, a.d_resid, wd);
    }
    ws.st_host->abort = 0;
    write_state();
    dev::dots(ws, nn, 0, a.d_v, a.d_ld, wd, a.d_resid, -1);
    fin(1, dev::kFinNorm, 0, 0, -1);
    read_state();
    double rnorm0 = ws.st_host->rnorm;
    rnorm = rnorm0;
    if (j == 1) co_return;

    // iterative classical Gram-Schmidt against V(:,1:j-1) (SRC/dgetv0.f:326-397)
    for (int iter = 0;;) {
        dev::dots(ws, nn, j - 1, a.d_v, a.d_ld, wd, a.d_resid, -1);
        fin(j, dev::kFinCoef, 0, 0, -1);
        dev::update(ws, nn, j - 1, a.d_v, a.d_ld, 0, a.d_resid, a.d_resid, bmat != 'G', -1);
        if (bmat == 'G') {
            g_stats.nbx += 1;
            dev::copy(a.stream, nn, a.d_resid, wd + nn);
            co_await rci(2, nn, 0);
            dev::dots(ws, nn, 0, a.d_v, a.d_ld, wd, a.d_resid, -1);
            fin(1, dev::kFinNorm, 0, 0, -1);
        } else {
            dev::copy(a.stream, nn, a.d_resid, wd);
            fin(j, dev::kFinNorm, 0, 0, -1);
        }
        read_state();
        rnorm = ws.st_host->rnorm;
        if (rnorm > 0.717 * rnorm0) break;
        ++iter;
        if (iter <= 5) {
            rnorm0 = rnorm;
            continue;
        }
        dev::fill(a.stream, nn, 0.0, a.d_resid);
        rnorm = 0.0;
        ws.st_host->rnorm = 0.0;
        write_state();
        ierr = -1;
        break;
    }
    co_return;
}

// dsaitr: extend a k-step Lanczos factorization to k+npk steps.
template <class R>
Task SolverT<R>::saitr(int k, int npk, int& iinfo) {
    const int64_t nn = n;
    R* wd = a.d_workd;
    const int64_t ipj = 0, irj = nn, ivj = 2 * nn;
    const bool bI = (bmat == 'I');
    iinfo = 0;
    // OP's output y = workd(irj): at ARPACK's fixed offset n, off the 128-B
    // lines when n is odd (config 4: n = 215^3), which costs every pass that
    // streams it.  The free-running engine, whose caller never sees
    // y between requests, keeps it in an aligned vector of its own instead and
    // copies it to workd(irj) when the solve ends (run()).
    if (free_run && bI && !ybuf && (reinterpret_cast<uintptr_t>(wd + irj) & 127) != 0 &&
        hipMalloc(&ybuf, sizeof(R) * (size_t)nn) != hipSuccess)
        ybuf = nullptr;
    R* const yv = (free_run && bI && ybuf) ? ybuf : wd + irj;
    int j = k + 1;
    // rnorm_stale: the restart's rnorm was left on the device (run()); a zero
    // there parks the cycle at its first step (k_place: st.abort = 1)
    bool restart_pending = !rnorm_stale && !(rnorm > 0.0);
    rnorm_stale = false;
    int rstart_j = -1;  // step at which a restart happened (h(j,1) = 0)
    // Chained steps (free-running engine, bmat = 'I', ncv <= 64): step j's DGKS
    // sweep also stores its residual r as the RAW column V(:,j+1) (and the x of a
    // row-distributed SpMV); step j+1 then runs OP on r instead of forming
    // v_{j+1} = r/rnorm first, and ONE finalize (kFinCgsChained) takes step j's
    // deferred refinement decision and step j+1's rescaled CGS coefficients; the
    // update pass normalises V(:,j+1) in place.  Per step that drops the
    // k_place pass, one finalize launch and -- on a row distribution -- one
    // allreduce (3 -> 2).  AHIP_CHAIN=0 disables it.  Lanczos (dsaupd) only: the
    // rounding of A r / rnorm differs from A (r / rnorm) in the last bit, and the
    // non-normal operators the Arnoldi path serves (n3: conv-diff, rho = 100) turn
    // that into a different restart count (42 vs the reference's 40 at tol 1e-10),
    // while every symmetric fixture keeps the reference's cycles and OP*x counts.
    static const bool chain_env = [] {
        const char* e = getenv("AHIP_CHAIN");
        return !(e && e[0] == '0');
    }();
    // (not for the SVD's normal operator B'B, nor for the float family's free
    // run on an fp32 operator: their steps stay the plain ones)
    const bool chain_base = chain_env && free_run && bI && mode == 1 && ncv <= 64 && !svd &&
                            std::is_same_v<R, double>;
    const bool chain_ok = chain_base && !arnoldi;
    // Folded steps (on top of chaining; AHIP_FOLD=0 disables): step j-1's DGKS
    // sweep is not a pass of its own.  Its update pass leaves r (before the
    // sweep) in resid, the SpMV runs on r, and step j's first pass over V
    // (dev::fold_dots, reads only) forms r' = r - V s in registers, rebuilds
    // A r' from A r with the Lanczos relation, and sums the CGS coefficients of
    // step j and r''r' (step j-1's deferred refinement check); the second pass
    // (dev::fold_update) forms them again, stores v_j = r'/rnorm and r_j.  Two V
    // passes per step instead of three.  The last step of a cycle takes its
    // sweep as usual.
    static const bool fold_env = [] {
        const char* e = getenv("AHIP_FOLD");
        return !(e && e[0] == '0');
    }();
    // Arnoldi (dnaupd): t = H s with the full Hessenberg records (exact: the
    // Arnoldi relation holds column by column).  The raw-residual chaining is
    // NOT used for Arnoldi (its last-bit differences changed n3's restart
    // count); the fold keeps the reference's cycles on every dnaupd fixture
    // and C3 at full size (tests/test_gpu_fold.py, test_gpu_ns.py,
    // test_gpu_fullsize.py).  AHIP_FOLD_NS=0 disables it.
    static const bool fold_ns_env = [] {
        const char* e = getenv("AHIP_FOLD_NS");
        return !(e && e[0] == '0');
    }();
    const bool fold_ok = chain_base && fold_env && (!arnoldi || fold_ns_env);
    bool chained = false;  // V(:,j) holds the raw residual of step j-1
    bool folded = false;   // ... which step j's fold pass forms from resid (step j-1's r)
    int rstart_prev = 0;
    if (fold_ok && k > 0) {
        // T(1:k,1:k) (H for Arnoldi) after dsapps/dnapps for the fold's t = T s:
        // the device records hold only this cycle's new steps
        double* hs = ws.host_scratch + 4 * (size_t)ws.stride;  // its own tail: 2 (ncv+1)
        const double* h = workl + ih;
        if (!arnoldi) {  // rec = (alpha_i, beta_i)
            for (int i = 1; i <= k; ++i) {
                hs[2 * (i - 1)] = h[(i - 1) + ncv];
                hs[2 * (i - 1) + 1] = h[i - 1];
            }
        } else {  // rec(2i-1) = h(i,i-1); columns 1..k of H -> hcol (pinned staging)
            for (int i = 1; i <= k; ++i) {
                hs[2 * (i - 1)] = h[(i - 1) + (size_t)(i - 1) * ncv];
                hs[2 * (i - 1) + 1] = i > 1 ? h[(i - 1) + (size_t)(i - 2) * ncv] : 0.0;
            }
            double* hc = ws.host_hcol;
            for (int c = 0; c < k; ++c)
                for (int i = 0; i < ncv; ++i) hc[(size_t)c * ncv + i] = i <= c ? h[i + (size_t)c * ncv] : 0.0;
            a.ck(hipMemcpyAsync(ws.hcol, hc, sizeof(double) * (size_t)k * ncv, hipMemcpyHostToDevice,
                              a.stream));
        }
        a.ck(hipMemcpyAsync(ws.rec, hs, sizeof(double) * 2 * k, hipMemcpyHostToDevice, a.stream));
    }

    for (;;) {
        while (j <= k + npk) {
            int rstart = 0;
            if (restart_pending) {
                // invariant subspace: new start vector orthogonal to V_j (SRC/dsaitr.f:378-427)
                g_stats.nrstrt += 1;
                int itry = 1, ierr = 0;
                for (;;) {
                    co_await getv0(false, j, itry, ierr);
                    if (ierr >= 0) break;
                    if (++itry <= 3) continue;
                    iinfo = j - 1;
                    co_return;
                }
                restart_pending = false;
                chained = false;
                rstart = 1;
                rstart_j = j;
                ws.st_host->abort = 0;
                ws.st_host->rnorm = rnorm;
                write_state();
            }
            // STEP 2: v_j = r/rnorm; p_j scaled too for bmat='G' (SRC/dsaitr.f:438-454)
            R* xop = dist_x() ? dist_x() : (free_run ? (folded ? a.d_resid : vcol(j)) : wd + ivj);
            if (!chained && !folded)
                dev::place(ws, nn, a.d_resid, vcol(j), xop == vcol(j) ? nullptr : xop,
                           bI ? nullptr : wd + ipj, j);
            // STEP 3: r_j = OP*v_j (SRC/dsaitr.f:461-474)
            g_stats.nopx += 1;
            co_await op(1, ivj, irj, ipj, xop, yv);
            // STEP 4: B*OP*v_j (skipped in mode 2: WORKD(IVJ) holds A*v_j)
            const R* u;
            if (mode == 2 && !arnoldi) {  // dsaitr only; dnaitr has no mode-2 shortcut
                u = wd + ivj;
            } else if (!bI) {
                g_stats.nbx += 1;
                co_await rci(2, irj, ipj);
                u = wd + ipj;
            } else {
                u = yv;
            }
            // wnorm and the CGS coefficients h = V_j' B r (SRC/dsaitr.f:538-594)
            if (folded) {  // + forms r' = V(:,j) and A r' (see fold_ok)
                dev::fold_dots(ws, nn, j, a.d_v, a.d_ld, a.d_resid, u);
                fin(j + 1, dev::kFinCgsFolded, j, rstart, -1, 1, rstart_prev);
            } else {
                dev::dots(ws, nn, j, a.d_v, a.d_ld, u, yv, -1);
                if (chained)  // + the deferred refinement decision of step j-1 (region 2)
                    fin(j + 1, dev::kFinCgsChained, j, rstart, -1, j, rstart_prev);
                else
                    fin(j + 1, dev::kFinCgs, j, rstart, -1);
            }
            // r_j = OP*v_j - V_j h; for bmat='I' the same pass also produces the
            // DGKS coefficients V_j' r_j and r_j' r_j (SRC/dsaitr.f:582-639)
            const bool next_folded = fold_ok && j < k + npk;
            // a folded next step's SpMV reads r from resid, or from the
            // distributed operator's x window
            if (folded) {
                dev::fold_update(ws, nn, j, a.d_v, a.d_ld, yv, a.d_resid,
                                 next_folded ? dist_x() : nullptr);
                // the next step's SpMV input (the distributed x window) is
                // complete here: its halo + SpMV may overlap this step's finalize
                if (next_folded && dist_x() && overlap_ready())
                    x_ready = hipEventRecord(x_ev, a.stream) == hipSuccess;
            } else {
                dev::UpdateChain<R> x;
                x.chained = chained;
                if (next_folded) x.raw2 = dist_x();
                dev::update(ws, nn, j, a.d_v, a.d_ld, 0, yv, a.d_resid, bI, -1, x);
            }
            if (bI && next_folded) {
                // + t = T s, st.fold; free-running, the next step's SpMV follows at
                // once and carries it (the symmetric SpMV's combine launch)
                fin(j + 1, dev::kFinPostCgsFold, j, rstart, -1, 0, 0, free_run);
                chained = false;
                folded = true;
                rstart_prev = rstart;
            } else if (bI) {
                fin(j + 1, dev::kFinPostCgs, j, rstart, -1);
                const bool next_chained = chain_ok && j < k + npk;
                if (next_chained) {
                    // the DGKS sweep (or, without one, a copy) also stores r as the
                    // raw V(:,j+1); its decision waits for step j+1's finalize
                    dev::UpdateChain<R> x;
                    x.raw1 = vcol(j + 1);
                    x.raw2 = dist_x();
                    x.part = ws.part + (size_t)ws.nblk * ws.stride;
                    dev::update(ws, nn, j, a.d_v, a.d_ld, 1, a.d_resid, a.d_resid, true, 1, x);
                } else {
                    // refinement sweeps, each gated on the device-side decision
                    dev::update(ws, nn, j, a.d_v, a.d_ld, 1, a.d_resid, a.d_resid, true, 1);
                    // free-running: the second refinement (rare) is not enqueued; if
                    // step j needs it, the finalize parks the cycle (abort = 2) and
                    // the host finishes the step below
                    const bool lazy = free_run;
                    fin(j + 1, lazy ? dev::kFinDgks1Lazy : dev::kFinDgks1, j, rstart, 1);
                    if (!lazy) dgks2_tail(j, rstart);
                }
                chained = next_chained;
                folded = false;
                rstart_prev = rstart;
            } else {
                // generalized problem: every B*r is a reverse-communication request,
                // so the refinement decisions are taken on the host.
                g_stats.nbx += 1;
                dev::copy(a.stream, nn, a.d_resid, wd + irj);
                co_await rci(2, irj, ipj);
                dev::dots(ws, nn, j, a.d_v, a.d_ld, wd + ipj, a.d_resid, -1);
                fin(j + 1, dev::kFinPostCgs, j, rstart, -1);
                read_state();
                for (int sweep = 1; sweep <= 2 && ws.st_host->dgks == sweep; ++sweep) {
                    dev::update(ws, nn, j, a.d_v, a.d_ld, sweep, a.d_resid, a.d_resid, false, sweep);
                    g_stats.nbx += 1;
                    dev::copy(a.stream, nn, a.d_resid, wd + irj);
                    co_await rci(2, irj, ipj);
                    dev::dots(ws, nn, j, a.d_v, a.d_ld, wd + ipj, a.d_resid, -1);
                    fin(j + 1, sweep == 1 ? dev::kFinDgks1 : dev::kFinDgks2, j, rstart, sweep);
                    read_state();
                }
                dev::zero_if(ws, nn, a.d_resid);
                // workd(ipj) must hold B*r for the next step (SRC/dsaitr.f:361)
                if (ws.st_host->zero) dev::fill(a.stream, nn, 0.0, wd + ipj);
            }
            ++j;
            if (!free_run) {
                read_state();
                rnorm = ws.st_host->rnorm;
                if (!(rnorm > 0.0)) restart_pending = true;
            }
        }
        // the new steps' T / H records travel with the state: one host sync
        // for both (the abort paths below loop back and fetch them again)
        double* rec_h = ws.host_scratch;
        dev::flush_deferred_finalize(ws.defq, a.stream);
        a.ck(hipMemcpyAsync(rec_h, ws.rec, sizeof(double) * 2 * (k + npk), hipMemcpyDeviceToHost,
                            a.stream));
        if (arnoldi) {
            hcol_h.resize((size_t)ncv * npk);
            a.ck(hipMemcpyAsync(hcol_h.data(), ws.hcol + (size_t)k * ncv, sizeof(double) * hcol_h.size(),
                                hipMemcpyDeviceToHost, a.stream));
        }
        read_state();
        if (check_halt()) co_return;  // run() ends the solve with info = -9999
        // a park inside a folded cycle leaves resid = r of the step before the
        // parked one, BEFORE its DGKS sweep (st.fold: the sweep was taken)
        const bool was_folded = fold_ok;
        chained = false;
        folded = false;  // a resumed cycle restarts with a formed v_j
        auto unfold = [&](int jprev) {  // resid = r' = r - V(:,1:jprev) s
            if (was_folded && ws.st_host->fold)
                dev::update(ws, nn, jprev, a.d_v, a.d_ld, 1, a.d_resid, a.d_resid, false, -1);
        };
        if (ws.st_host->abort == 2) {  // step abort_j needs its second DGKS sweep
            const int ja = ws.st_host->abort_j;
            g_stats.nopx -= (k + npk) - ja;  // the later steps were skipped
            ws.st_host->abort = 0;
            write_state();
            if (was_folded && ja < k + npk) {
                // parked by step ja+1's kFinCgsFolded: r' was formed only in
                // registers and the second sweep's coefficients V_ja' r' not summed
                unfold(ja);
                dev::dots(ws, nn, ja, a.d_v, a.d_ld, a.d_resid, a.d_resid, -1);
                fin(ja + 1, dev::kFinFoldCoef2, ja, ja == rstart_j ? 1 : 0, -1);
            }
            dgks2_tail(ja, ja == rstart_j ? 1 : 0);
            j = ja + 1;
            continue;
        }
        if (ws.st_host->abort == 3) {  // chained step abort_j: rnorm outside the raw
            const int ja = ws.st_host->abort_j;  // range -- redo it with v_j formed
            g_stats.nopx -= (k + npk) - ja + 1;
            ws.st_host->abort = 0;
            write_state();
            unfold(ja - 1);  // r' of step ja-1
            j = ja;
            continue;
        }
        if (ws.st_host->abort) {  // free-running cycle hit rnorm == 0 at step abort_j
            const int ja = ws.st_host->abort_j;
            g_stats.nopx -= (k + npk) - ja + 1;  // those OP*x were never applied
            j = ja;
            restart_pending = true;
            continue;
        }
        break;
    }
    rnorm = ws.st_host->rnorm;
    g_stats.nrorth += ws.st_host->nrorth;
    g_stats.nitref += ws.st_host->nitref;
    ws.st_host->nrorth = ws.st_host->nitref = 0;
    write_state();
    // assemble the new columns of H from the per-step device records (on the
    // host since the cycle-end sync above)
    const double* rec = ws.host_scratch;
    double* h = workl + ih;
    if (!arnoldi) {  // T(ncv,2): h(:,1) subdiagonal, h(:,2) diagonal
        for (int jj = k + 1; jj <= k + npk; ++jj) {
            h[(jj - 1) + ncv] = rec[2 * (jj - 1)];
            h[jj - 1] = rec[2 * (jj - 1) + 1];
        }
    } else {  // H(ncv,ncv): h(1:j,j) from the device, h(j,j-1) = beta_j (SRC/dnaitr.f:566-590)
        const std::vector<double>& hc = hcol_h;
        for (int jj = k + 1; jj <= k + npk; ++jj) {
            double* col = h + (size_t)(jj - 1) * ncv;
            std::memcpy(col, hc.data() + (size_t)(jj - 1 - k) * ncv, sizeof(double) * jj);
            if (jj > 1) h[(jj - 1) + (size_t)(jj - 2) * ncv] = rec[2 * (jj - 1) + 1];  // h(jj,jj-1)
        }
        // negligible subdiagonals of the new Hessenberg block (SRC/dnaitr.f:820-838)
        const double ulp = 2.0 * eps;  // dlamch / slamch('precision')
        const double smlnum = safmin * ((double)n_global / ulp);
        const int kp = k + npk;
        for (int i = std::max(1, k); i <= kp - 1; ++i) {
            double tst1 = std::fabs(h[(i - 1) + (size_t)(i - 1) * ncv]) + std::fabs(h[i + (size_t)i * ncv]);
            if (tst1 == 0.0) tst1 = la::lanhs1(kp, h, ncv);
            double& sub = h[i + (size_t)(i - 1) * ncv];
            if (std::fabs(sub) <= std::max(ulp * tst1, smlnum)) sub = 0.0;
        }
    }
    (void)rstart_j;
    co_return;
}

// dsapps: bulge chase on the host, V*Q and the residual update on the device.
template <class R>
void SolverT<R>::sapps(int kev, int npk) {
    const int kplusp = kev + npk;
    double* h = workl + ih;
    double* q = workl + iq;
    la::dsapps_host(kev, npk, workl + iritz, h, ncv, q, ncv);
    if (npk == 0) return;
    const double sigmak = q[(kplusp - 1) + (size_t)(kev - 1) * ncv];
    const double betak = h[kev];  // h(kev+1,1)
    vq_device(kev, kplusp, sigmak, betak);
}

// V(:,1:kev) = V(:,1:kplusp) * Q(:,1:kev); v_{kev+1} = V*Q(:,kev+1) if betak > 0;
// resid = sigmak*resid + betak*v_{kev+1} (SRC/dsapps.f:450-493, dnapps.f:583-640).
// Q is the host matrix at workl(iq) (ld ncv).
template <class R>
void SolverT<R>::vq_device(int kev, int kplusp, double sigmak, double betak) {
    const double* q = workl + iq;
    // Q(:,1:kev+1) compact (ld = kplusp). ncv <= 64: staged in the pinned
    // ws.host_q (ncv^2 >= kplusp (kev+1)), so the copy is asynchronous and the
    // kFinNorm finalize and the next cycle queue behind V*Q without a host
    // wait; its next writer is the next restart, after that cycle's end sync.
    const size_t m = (size_t)kplusp * (kev + 1);
    std::vector<double> qvec;
    double* qbuf = ws.host_q;
    if (!qbuf) {
        qvec.resize(m);
        qbuf = qvec.data();
    }
    for (int c = 0; c <= kev && c < kplusp; ++c)
        for (int r = 0; r < kplusp; ++r) qbuf[(size_t)c * kplusp + r] = q[r + (size_t)c * ncv];
    a.ck(hipMemcpyAsync(ws.q, qbuf, sizeof(double) * m, hipMemcpyHostToDevice, a.stream));
    dev::vq_update(ws, n, a.d_v, a.d_ld, kplusp, kev, sigmak, betak, a.d_resid);
    if (!ws.host_q) a.sync();  // pageable qvec: its lifetime
}

template <class R>
Task SolverT<R>::run() {
    // ---- dsaup2 initialisation (SRC/dsaup2.f:258-317)
    const double eps23 = std::pow(eps, 2.0 / 3.0);
    int nev = nev0;
    const int np0 = np;
    const int kplusp = nev0 + np0;
    int nconv = 0, iter = 0;
    const bool initv = (info != 0);
    info = 0;
    double* h = workl + ih;
    double* ritz = workl + iritz;
    double* bounds = workl + ibounds;
    double* wl = workl + iw;
    int ierr = 0;
    int sinfo = 0;

    if (initv) a.upload_resid();
    co_await getv0(initv, 1, 1, ierr);
    if (check_halt()) goto fault;
    if (rnorm == 0.0) {
        info = -9;
        goto done;
    }
    ws.st_host->rnorm = rnorm;
    ws.st_host->abort = 0;
    write_state();

    co_await saitr(0, nev0, sinfo);
    if (halted) goto fault;
    if (sinfo > 0) {
        np = sinfo;
        mxiter = iter;
        info = -9999;
        goto done;
    }

    for (;;) {  // MAIN LANCZOS ITERATION LOOP (SRC/dsaup2.f:400-821)
        if (pause_budget == 0) co_await rci(kPauseIdo, -1, -1);
        if (pause_budget > 0) --pause_budget;
        ++iter;
        co_await saitr(nev, np, sinfo);
        if (halted) goto fault;
        if (sinfo > 0) {
            np = sinfo;
            mxiter = iter;
            info = -9999;
            goto done;
        }
        if (la::dseigt(rnorm, kplusp, h, ncv, ritz, bounds, wl) != 0) {
            info = -8;
            goto done;
        }
        std::memcpy(wl + kplusp, ritz, sizeof(double) * kplusp);
        std::memcpy(wl + 2 * kplusp, bounds, sizeof(double) * kplusp);
        nev = nev0;
        np = np0;
        la::dsgets(ishift, which, nev, np, ritz, bounds, wl);
        std::memcpy(wl + np, bounds + np, sizeof(double) * nev);
        nconv = la::dsconv(nev, ritz + np, wl + np, tol, eps);
        {
            const int nptemp = np;
            for (int jj = 0; jj < nptemp; ++jj)
                if (bounds[jj] == 0.0) {
                    --np;
                    ++nev;
                }
        }
        if (nconv >= nev0 || iter > mxiter || np == 0) {
            // prepare to exit: sort converged Ritz values first (SRC/dsaup2.f:536-667)
            if (which == la::Which::BE) {
                la::dsortr(la::Which::SA, true, kplusp, ritz, bounds);
                const int nevd2 = nev0 / 2, nevm2 = nev0 - nevd2;
                if (nev > 1) {
                    np = kplusp - nev0;
                    const int cnt = std::min(nevd2, np);
                    const int dst = std::max(kplusp - nevd2, kplusp - np);
                    for (int t = 0; t < cnt; ++t) {
                        std::swap(ritz[nevm2 + t], ritz[dst + t]);
                        std::swap(bounds[nevm2 + t], bounds[dst + t]);
                    }
                }
            } else {
                la::Which wp = la::Which::SM;
                if (which == la::Which::LM) wp = la::Which::SM;
                if (which == la::Which::SM) wp = la::Which::LM;
                if (which == la::Which::LA) wp = la::Which::SA;
                if (which == la::Which::SA) wp = la::Which::LA;
                la::dsortr(wp, true, kplusp, ritz, bounds);
            }
            for (int jj = 0; jj < nev0; ++jj) bounds[jj] /= std::max(eps23, std::fabs(ritz[jj]));
            la::dsortr(la::Which::LA, true, nev0, bounds, ritz);
            for (int jj = 0; jj < nev0; ++jj) bounds[jj] *= std::max(eps23, std::fabs(ritz[jj]));
            if (which == la::Which::BE) la::dsortr(la::Which::LA, true, nconv, ritz, bounds);
            else la::dsortr(which, true, nconv, ritz, bounds);
            h[0] = rnorm;  // communicates rnorm to dseupd (SRC/dsaup2.f:645)
            if (iter > mxiter && nconv < nev) info = 1;
            if (np == 0 && nconv < nev0) info = 2;
            np = nconv;
            mxiter = iter;
            nev = nconv;
            goto done;
        } else if (nconv < nev && ishift == 1) {
            // anti-stagnation: grow nev (SRC/dsaup2.f:669-694)
            const int nevbef = nev;
            nev += std::min(nconv, np / 2);
            if (nev == 1 && kplusp >= 6) nev = kplusp / 2;
            else if (nev == 1 && kplusp > 2) nev = 2;
            np = kplusp - nev;
            if (nevbef < nev) la::dsgets(ishift, which, nev, np, ritz, bounds, wl);
        }
        if (ishift == 0) {  // user shifts through reverse communication (ido = 3)
            iparam[7] = np;
            co_await rci(3, -1, -1);
            std::memcpy(ritz, wl, sizeof(double) * np);
        }
        sapps(nev, np);
        // B-norm of the updated residual (SRC/dsaup2.f:773-809)
        if (bmat == 'G') {
            g_stats.nbx += 1;
            dev::copy(a.stream, n, a.d_resid, a.d_workd + n);
            co_await rci(2, n, 0);
            dev::dots(ws, n, 0, a.d_v, a.d_ld, a.d_workd, a.d_resid, -1);
            fin(1, dev::kFinNorm, 0, 0, -1);
        } else {
            fin(1, dev::kFinNorm, 0, 0, -1);  // r'r partials came with V*Q
        }
        if (free_run && bmat != 'G') {
            // no host round trip between V*Q and the next cycle: its steps are
            // enqueued behind the kFinNorm finalize, which leaves rnorm on the
            // device (rnorm_stale; saitr).  A failure is caught by that
            // cycle's check.
            rnorm_stale = true;
            continue;
        }
        read_state();  // (a failure here is caught by the next cycle's check)
        rnorm = ws.st_host->rnorm;
    }
fault:  // a failed HIP call: the device state is not trustworthy
    if (halted) {
        mxiter = iter;
        info = -9999;
    }
done:
    if (ybuf) dev::copy(a.stream, n, ybuf, a.d_workd + n);  // workd(irj) = the last OP x (saitr)
    nev0 = nev;
    iparam[2] = mxiter;
    co_return;
}

template struct ArraysT<double>;
template struct ArraysT<float>;
template class SolverT<double>;
template class SolverT<float>;

}  // namespace ahip
