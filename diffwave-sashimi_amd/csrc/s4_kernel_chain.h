// S4 convolution-kernel generation (`s4.py:704-807`) and its adjoint as ONE chain of launches over `rows` rows of state: the H
// rows of a single block, or the n H rows of a group of same-shaped blocks stacked along H.  Every launch of the chain is
// indexed by a row, so a block on its own is a group of one whose "stacked buffers" are the block's own tensors.
#pragma once
#include <rocfft/rocfft.h>

#include <mutex>
#include <tuple>

#include "model.h"

namespace dws {

#define DWS_FFT(expr)                                                                                  \
    do {                                                                                               \
        rocfft_status _r = (expr);                                                                     \
        if (_r != rocfft_status_success)                                                               \
            return set_error(DWS_ERR_HIP, "%s failed: rocfft_status %d (%s:%d)", #expr, (int)_r, __FILE__, __LINE__); \
    } while (0)

// rocFFT, through its native API: batched 1-D real transforms, out of place, unscaled, rows packed back to back (the
// defaults of a plan without a description: input distance n reals / n/2+1 complex, output the other way round).  Used
// where the fused LDS FFT does not apply: the irfft(n = L) of the kernel generation (`s4.py:796-805`) and its adjoint,
// and the R2C / C2R pair of stage lengths the fused kernels do not cover (odd lengths; more than 16384 taps).
// A plan owns its work buffer and execution info, so rocfft_execute never allocates (it may run inside a stream capture).
struct RocfftPlan {
    rocfft_plan plan = nullptr;
    rocfft_execution_info info = nullptr;
    DevBuf work;
};

// rocfft_setup() / rocfft_cleanup() act on process-global state (plan repository, RTC cache, logging): set up once per
// process; never torn down from a model's destructor -- another model in the process may still hold plans.
inline int rocfft_setup_once() {
    static std::once_flag once;
    static rocfft_status st = rocfft_status_success;
    std::call_once(once, [] { st = rocfft_setup(); });
    if (st != rocfft_status_success) return set_error(DWS_ERR_HIP, "rocfft_setup failed: rocfft_status %d", (int)st);
    return DWS_OK;
}

struct FftPlans {
    std::map<std::tuple<int, int, int>, RocfftPlan*> plans;  // (type, n, batch)
    ~FftPlans() {
        for (auto& kv : plans) {
            if (kv.second->info) rocfft_execution_info_destroy(kv.second->info);
            if (kv.second->plan) rocfft_plan_destroy(kv.second->plan);
            delete kv.second;
        }
    }
    // type 0: R2C rows of n reals (dist n) -> n/2+1 complex; type 1: C2R n/2+1 complex -> n reals (dist n)
    int get(int type, int n, int batch, RocfftPlan** out) {
        auto key = std::make_tuple(type, n, batch);
        auto it = plans.find(key);
        if (it == plans.end()) {
            DWS_TRY(rocfft_setup_once());
            RocfftPlan* p = new RocfftPlan();
            it = plans.emplace(key, p).first;      // owned by the map from here on (freed with it, also after an error)
            const size_t len[1] = {(size_t)n};
            DWS_FFT(rocfft_plan_create(&p->plan, rocfft_placement_notinplace,
                                       type == 0 ? rocfft_transform_type_real_forward : rocfft_transform_type_real_inverse,
                                       rocfft_precision_single, 1, len, (size_t)batch, nullptr));
            size_t wbytes = 0;
            DWS_FFT(rocfft_plan_get_work_buffer_size(p->plan, &wbytes));
            DWS_FFT(rocfft_execution_info_create(&p->info));
            if (wbytes) {
                DWS_TRY(p->work.ensure(wbytes));
                DWS_FFT(rocfft_execution_info_set_work_buffer(p->info, p->work.p, wbytes));
            }
        }
        DWS_CHECK(it->second->plan && it->second->info, DWS_ERR_HIP, "rocFFT plan (type %d, n %d, batch %d) was not created", type, n, batch);
        *out = it->second;
        return DWS_OK;
    }
    // one batched transform on stream s (the real inverse may use its input as scratch, as rocFFT documents)
    int exec(int type, int n, int batch, void* in, void* out, hipStream_t s) {
        RocfftPlan* p = nullptr;
        DWS_TRY(get(type, n, batch, &p));
        DWS_FFT(rocfft_execution_info_set_stream(p->info, (void*)s));
        void* ib[1] = {in};
        void* ob[1] = {out};
        DWS_FFT(rocfft_execute(p->plan, ib, ob, p->info));
        return DWS_OK;
    }
};

struct FftTables {
    DevBuf tw, twn, twp;
};

// v, w dt, dt of s4_prep and r = Cauchy(v, z, w dt) (`s4.py:740-775`): [6][rows][N] complex, [rows][N] complex, [rows],
// [6][rows][Lk/2+1] complex
struct S4Products { DevBuf v, wdt, dt, r; };

// What the chains of one model share: the rocFFT plans, the twiddle tables of the fused LDS FFT, and the scratch of one run of
// the chain (chains run one after the other on one stream).
struct S4Workspace {
    FftPlans fft;
    std::map<int, FftTables*> tables;  // by log2(M)
    S4Products scratch;                // Cauchy products of a chain that does not keep its own (sampling commits)
    DevBuf ckf, ck, cK, cKf;           // taps forward / spectrum: kf [2][rows][Lk/2+1], taps k [2][rows][Lk], K [rows][2M], K_f
    DevBuf dKt, dkt, dkf;              // spectrum adjoint: dK [rows][2M], dk [2][rows][Lk], dkf [2][rows][Lk/2+1]
    DevBuf cgr, cgv, cgw, cpdt;        // adjoint of Woodbury / Cauchy / s4_prep
    ~S4Workspace() { for (auto& kv : tables) delete kv.second; }
    int get_tables(int log2m, FftTables** out, hipStream_t s);
};

// The six tensors of an S4 kernel (`s4.py:704-739`) over a chain's rows, or their gradients: C [2][rows][N] complex, B and P
// [rows][N] complex, inv_w_real and w_imag [rows][N], log_dt [rows].  A block's C is [2][H][N] and a group's stack
// [2][n H][N]: they coincide for n = 1, so a single block's tensors are used where they are.
struct S4Tensors { float *C, *B, *P, *inv_w_real, *w_imag, *log_dt; };

constexpr uint64_t S4_NOT_KEPT = ~0ull;    // S4Chain::version of products that live in the workspace's scratch

// What a chain runs on, and what it has to remember between the commit and the backward.
struct S4Chain {
    int rows = 0, N = 0, Lk = 0;                  // H or n H; state size; kernel length (taps per direction)
    S4Tensors par{};
    const float *z = nullptr, *omega = nullptr;   // the FFT nodes of length Lk (`s4.py:561-565`)
    // the Cauchy products, kept from a training commit so that the adjoint does not regenerate them (one Cauchy forward per
    // chain and step less); valid for the commit numbered `version`
    S4Products kept;
    uint64_t version = S4_NOT_KEPT;
    DevBuf kfa, kfb, kfs;                         // fused path: pair-ordered spectra [rows][M/2] x 2, [rows][3] (fftconv.h)
    int Lh() const { return Lk / 2 + 1; }
};

// 1. taps forward: the products and the (unnormalised) time-domain taps, ws.ck = [2][rows][Lk].  `version`: the commit the
//    products are kept for, in the chain's own buffers; S4_NOT_KEPT puts them into the workspace's scratch.
int s4_taps_forward(S4Workspace& ws, S4Chain& c, uint64_t version, hipStream_t s);
// 2. fused spectrum: ws.ck (Lt taps per direction) -> c.kfa / kfb / kfs at M = 2^lg, produced by the LDS FFT of the per-step
//    kernel and stored in its pair order
int s4_fused_spectrum(S4Workspace& ws, S4Chain& c, int Lt, int lg, hipStream_t s);
// 3. spectrum adjoint (fused form): dKf [rows][M+1] complex -> ws.dkf = [2][rows][Lk/2+1] and dD [rows]
int s4_spectrum_adjoint(S4Workspace& ws, const S4Chain& c, int lg, float* dKf, float* dD, hipStream_t s);
// 4. taps adjoint: ws.dkf -> the gradients of the six tensors.  Products kept for another commit than `commit` are
//    regenerated first.
int s4_taps_adjoint(S4Workspace& ws, S4Chain& c, uint64_t commit, const S4Tensors& grad, hipStream_t s);

}  // namespace dws
