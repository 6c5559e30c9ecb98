// The S4 kernel-generation chain and its adjoint (s4_kernel_chain.h): the only place its launches are written.
#include "s4_kernel_chain.h"

#include "fftconv.h"
#include "sashimi.h"
#include "sashimi_train.h"

namespace dws {

int S4Workspace::get_tables(int log2m, FftTables** out, hipStream_t s) {
    auto it = tables.find(log2m);
    if (it == tables.end()) {
        auto* t = new FftTables();
        std::vector<float> tw, twn, twp;
        build_fft_tables(log2m, tw, twn, twp);
        DWS_TRY(t->tw.ensure(tw.size() * 4));
        DWS_TRY(t->twn.ensure(twn.size() * 4));
        DWS_TRY(t->twp.ensure(twp.size() * 4));
        DWS_HIP(hipMemcpyAsync(t->tw.p, tw.data(), tw.size() * 4, hipMemcpyHostToDevice, s));
        DWS_HIP(hipMemcpyAsync(t->twn.p, twn.data(), twn.size() * 4, hipMemcpyHostToDevice, s));
        DWS_HIP(hipMemcpyAsync(t->twp.p, twp.data(), twp.size() * 4, hipMemcpyHostToDevice, s));
        DWS_HIP(hipStreamSynchronize(s));
        it = tables.emplace(log2m, t).first;
    }
    *out = it->second;
    return DWS_OK;
}

// parameters -> v, w dt, dt -> r = Cauchy(v, z, w dt), into the chain's own buffers when they are kept for the adjoint, else
// into the workspace's scratch
static int generate_products(S4Workspace& ws, S4Chain& c, uint64_t version, hipStream_t s) {
    const size_t HN = (size_t)c.rows * c.N;
    S4Products& p = version != S4_NOT_KEPT ? c.kept : ws.scratch;
    DWS_TRY(p.v.ensure(6 * HN * 8));
    DWS_TRY(p.wdt.ensure(HN * 8));
    DWS_TRY(p.dt.ensure((size_t)c.rows * 4));
    DWS_TRY(p.r.ensure((size_t)6 * c.rows * c.Lh() * 8));
    DWS_TRY(launch_s4_prep(c.par.C, c.par.B, c.par.P, c.par.inv_w_real, c.par.w_imag, c.par.log_dt, p.v.f(), p.wdt.f(), p.dt.f(),
                           c.rows, c.N, s));
    DWS_TRY(launch_cauchy_sym_fwd_bcast(p.v.f(), c.z, p.wdt.f(), p.r.f(), 6 * c.rows, c.N, c.Lh(), c.rows, s));
    c.version = version;
    return DWS_OK;
}

int s4_taps_forward(S4Workspace& ws, S4Chain& c, uint64_t version, hipStream_t s) {
    DWS_TRY(generate_products(ws, c, version, s));
    const S4Products& p = version != S4_NOT_KEPT ? c.kept : ws.scratch;
    DWS_TRY(ws.ckf.ensure((size_t)2 * c.rows * c.Lh() * 8));
    DWS_TRY(ws.ck.ensure((size_t)2 * c.rows * c.Lk * 4));
    DWS_TRY(launch_s4_woodbury(p.r.f(), c.omega, p.dt.f(), ws.ckf.f(), c.rows, c.Lh(), (c.Lk % 2) == 0, s));
    return ws.fft.exec(1, c.Lk, 2 * c.rows, ws.ckf.p, ws.ck.p, s);
}

int s4_fused_spectrum(S4Workspace& ws, S4Chain& c, int Lt, int lg, hipStream_t s) {
    const int M = 1 << lg, Nf = 2 * M;
    FftTables* t;
    DWS_TRY(ws.get_tables(lg, &t, s));
    DWS_TRY(ws.cK.ensure((size_t)c.rows * Nf * 4));
    DWS_TRY(ws.cKf.ensure((size_t)c.rows * (M + 1) * 8));
    DWS_TRY(c.kfa.ensure((size_t)c.rows * (M / 2) * 8));
    DWS_TRY(c.kfb.ensure((size_t)c.rows * (M / 2) * 8));
    DWS_TRY(c.kfs.ensure((size_t)c.rows * 3 * 8));
    DWS_TRY(launch_s4_twosided_pow2(ws.ck.f(), ws.cK.f(), c.rows, Lt, Nf, c.Lk, s));
    DWS_TRY(launch_rfft_rows(lg, ws.cK.f(), ws.cKf.f(), t->tw.f(), t->twn.f(), c.rows, s));
    return launch_kf_permute(ws.cKf.f(), c.kfa.f(), c.kfb.f(), c.kfs.f(), c.rows, lg, s);
}

int s4_spectrum_adjoint(S4Workspace& ws, const S4Chain& c, int lg, float* dKf, float* dD, hipStream_t s) {
    const int Nf = 2 << lg, Ls = c.Lk;
    DWS_TRY(ws.dKt.ensure((size_t)c.rows * Nf * 4));
    DWS_TRY(ws.dkt.ensure((size_t)2 * c.rows * Ls * 4));
    DWS_TRY(ws.dkf.ensure((size_t)2 * c.rows * c.Lh() * 8));
    DWS_TRY(ws.fft.exec(1, Nf, c.rows, dKf, ws.dKt.p, s));
    // dK_t = C2R / Nf; k enters K as k / L (s4_twosided_pow2); dD[h] = sum u da = dK_t[h][0]
    DWS_TRY(launch_s4_twosided_pow2_bwd(ws.dKt.f(), ws.dkt.f(), dD, c.rows, Ls, Nf, 1.f / ((float)Nf * (float)Ls), 1.f / (float)Nf, s));
    return ws.fft.exec(0, Ls, 2 * c.rows, ws.dkt.p, ws.dkf.p, s);
}

int s4_taps_adjoint(S4Workspace& ws, S4Chain& c, uint64_t commit, const S4Tensors& grad, hipStream_t s) {
    const size_t HN = (size_t)c.rows * c.N;
    const int Lh = c.Lh(), nparts = ceil_div(Lh, 256);
    DWS_TRY(ws.cgr.ensure((size_t)6 * c.rows * Lh * 8));
    DWS_TRY(ws.cgv.ensure(6 * HN * 8));
    DWS_TRY(ws.cgw.ensure(6 * HN * 8));
    DWS_TRY(ws.cpdt.ensure((size_t)c.rows * nparts * 4));
    const bool kept = c.version == commit;
    if (!kept) DWS_TRY(generate_products(ws, c, S4_NOT_KEPT, s));
    const S4Products& p = kept ? c.kept : ws.scratch;
    DWS_TRY(launch_s4_woodbury_bwd(p.r.f(), c.omega, p.dt.f(), ws.dkf.f(), ws.cgr.f(), ws.cpdt.f(), c.rows, Lh, (c.Lk % 2) == 0, s));
    DWS_TRY(launch_cauchy_sym_bwd_bcast(p.v.f(), c.z, p.wdt.f(), ws.cgr.f(), ws.cgv.f(), ws.cgw.f(), 6 * c.rows, c.N, Lh, c.rows, s));
    return launch_s4_prep_bwd(c.par.C, c.par.B, c.par.P, c.par.inv_w_real, c.par.w_imag, c.par.log_dt, ws.cgv.f(), ws.cgw.f(),
                              ws.cpdt.f(), nparts, grad.C, grad.B, grad.P, grad.inv_w_real, grad.w_imag, grad.log_dt, c.rows, c.N, s);
}

}  // namespace dws
