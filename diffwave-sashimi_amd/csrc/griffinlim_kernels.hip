// Mel inversion: the inverse short-time DFT (`dataloaders/stft.py:165-194`, STFT.inverse) and the Griffin-Lim iteration
// (`stft.py:66-82`) on the short-time DFT core of the analysis kernels.  Framing is dws_mel_spectrogram's with a length
// per clip: frames f = 0 .. len_b / hop, centred, reflected about the clip's OWN ends; one workgroup of 256 threads owns
// one frame of one clip.
//
// Sign: the core's DFT is (cos, +sin), Im_core = sum x sin; the public spectrum and phase are torch.stft's e^{-i theta},
// Im_api = -Im_core.  The sign is handled where a phase enters (istft_rows_kernel); the projection never leaves the
// core's convention.
//
// Inverse stage: the real inverse DFT of a Hermitian spectrum is x[i] = sum_k h_k (Re_k cos + Im_core_k sin)(2 pi i k / N)
// over k = 0 .. N/2 with h = 1/N at k = 0 and k = N/2 (whose imaginary part does not enter, as irfft ignores it) and 2/N
// elsewhere: idft_sample on the rows h_k (Re_k, Im_core_k).  1/N is a power of two, so the weight rounds nothing.
//
// One round of the iteration is two launches and no spectrogram goes to memory: gl_project_kernel (frame of the current
// signal -> all K bins -> magnitude replaced, phase kept -> inverse stage -> workspace row) and istft_gather_kernel (the
// overlap-add divided by the window's sum of squares, one thread per sample, ascending frame order).  No atomics: every
// result is bitwise reproducible, and row b depends on clip b's own frames alone.
#include <cfloat>

#include "stft_core.h"

namespace dws {

// Frame f of clip b from (magnitude, phase) [B][K][f_max]; a null phase is phase 0.
__global__ __launch_bounds__(256) void istft_rows_kernel(const float* __restrict__ mag, const float* __restrict__ phase,
                                                         const int* __restrict__ lengths, const float* __restrict__ window,
                                                         float* __restrict__ ws, int T, int n_fft, int hop, int f_max) {
    extern __shared__ float2 gl_lds[];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int half = n_fft / 2, nb = half + 1;
    int len;
    if (f >= centred_clip_frames(lengths, b, T, half + 1, hop, len)) return;   // the whole workgroup, before any barrier
    float2* tab = gl_lds;                                    // [n_fft] (cos, sin)(2 pi j / n_fft)
    float2* d = tab + n_fft;                                 // [nb]    h_k (Re_k, Im_core_k)
#pragma clang loop vectorize(disable)
    for (int i = tid; i < n_fft; i += 256) tab[i] = twiddle(i, n_fft);
    const float inv_n = 1.f / (float)n_fft;
    for (int k = tid; k < nb; k += 256) {
        const size_t at = ((size_t)b * nb + k) * f_max + f;
        const float m = mag[at];
        float s = 0.f, c = 1.f;
        if (phase) sincosf(phase[at], &s, &c);
        d[k] = hermitian_row(k, half, inv_n, m * c, -(m * s));       // Im_core = -Im_api = -M sin(theta)
    }
    __syncthreads();
    inverse_rows(d, tab, window, ws + ((size_t)b * f_max + f) * n_fft, n_fft, tid);
}

// One projection of frame f of clip b: the frame of `cur` [B][T], its K bins, (Re, Im) M / |X| -- (M, 0) where |X| is
// exactly 0, the phase atan2(0, 0) = 0 gives -- and the inverse stage into the workspace.
__global__ __launch_bounds__(256) void gl_project_kernel(const float* __restrict__ cur, const float* __restrict__ mag,
                                                         const int* __restrict__ lengths, const float* __restrict__ window,
                                                         float* __restrict__ ws, int T, int n_fft, int hop, int f_max) {
    extern __shared__ float2 gl_lds[];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int half = n_fft / 2, nb = half + 1;
    int len;
    if (f >= centred_clip_frames(lengths, b, T, half + 1, hop, len)) return;   // the whole workgroup, before any barrier
    float2* tab = gl_lds;                                    // [n_fft]
    float2* d = tab + n_fft;                                 // [nb]
    float* frame = reinterpret_cast<float*>(d + nb);         // [n_fft]
    load_centred_frame<1>(frame, tab, cur + (size_t)b * T, nullptr, window, f * hop - half, len, n_fft, tid);
    __syncthreads();
    const float inv_n = 1.f / (float)n_fft;
    for (int k = tid; k < nb; k += 256) {
        float re[1], im[1];
        dft_bin<1>(frame, tab, k, n_fft, n_fft - 1, re, im);
        const float m = mag[((size_t)b * nb + k) * f_max + f];
        const float a = sqrtf(re[0] * re[0] + im[0] * im[0]);
        const float t = m / a;
        d[k] = a == 0.f ? hermitian_row(k, half, inv_n, m, 0.f) : hermitian_row(k, half, inv_n, re[0] * t, im[0] * t);
    }
    __syncthreads();
    inverse_rows(d, tab, window, ws + ((size_t)b * f_max + f) * n_fft, n_fft, tid);
}

// Normalised overlap-add, one thread per output sample j: padded position p = j + N/2, the frames that cover p in
// ascending order (ola_gather_position's bounds; no reflection terms), divided by wss(p) = sum_f w^2[p - f hop] from the
// same loop wherever wss > FLT_MIN (the reference's `tiny` rule; elsewhere the sum stays undivided).  x [B][T] receives
// the result x_n; y, where not null, x_n + alpha (x_n - x_{n-1}) with x_{n-1} read from x before it is overwritten
// (alpha == 0: y_n = x_n, nothing is read).  Positions at or behind the clip's length are written as exactly 0.
__global__ __launch_bounds__(256) void istft_gather_kernel(const float* __restrict__ ws, const int* __restrict__ lengths,
                                                           const float* __restrict__ window, float* __restrict__ x,
                                                           float* __restrict__ y, int T, int n_fft, int hop, int f_max,
                                                           float alpha) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= T) return;
    const int half = n_fft / 2;
    int len;
    const int nf = centred_clip_frames(lengths, b, T, half + 1, hop, len);
    const size_t at = (size_t)b * T + j;
    if (nf == 0 || j >= len) {
        x[at] = 0.f;
        if (y) y[at] = 0.f;
        return;
    }
    const float* wsb = ws + (size_t)b * f_max * n_fft;
    const int p = j + half;
    int lo = p - n_fft + 1;
    lo = lo <= 0 ? 0 : (lo + hop - 1) / hop;
    int hi = p / hop;
    if (hi > nf - 1) hi = nf - 1;
    float acc = 0.f, wss = 0.f;
    for (int f = lo; f <= hi; ++f) {
        const int i = p - f * hop;
        acc += wsb[(size_t)f * n_fft + i];
        const float w = window[i];
        wss = fmaf(w, w, wss);
    }
    const float v = wss > FLT_MIN ? acc / wss : acc;
    if (y) y[at] = alpha != 0.f ? fmaf(alpha, v - x[at], v) : v;
    x[at] = v;
}

int gl_gather(const float* ws, const int32_t* lengths, const float* window, float* x, float* y, int64_t B, int64_t T,
              int32_t n_fft, int32_t hop, int f_max, float alpha, hipStream_t stream) {
    hipLaunchKernelGGL(istft_gather_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)B), dim3(256), 0, stream, ws, lengths,
                       window, x, y, (int)T, n_fft, hop, f_max, alpha);
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}

}  // namespace dws

extern "C" int64_t dws_griffin_lim_workspace(int64_t B, int64_t f_max, int32_t n_fft, int32_t hop, int32_t momentum) {
    if (B < 1 || B > 65535 || f_max < 2 || hop < 1 || !dws::n_fft_ok(n_fft, 4096) ||
        (f_max - 1) > (INT32_MAX - (int64_t)n_fft) / hop)
        return 0;
    return (B * f_max * (int64_t)n_fft + (momentum ? B * (f_max - 1) * hop : 0)) * (int64_t)sizeof(float);
}

extern "C" int dws_griffin_lim(const float* magnitude, const float* phase0, int64_t B, int64_t f_max, const int32_t* lengths,
                               const int32_t* lengths_host, const float* window, int32_t n_fft, int32_t hop, int32_t n_iters,
                               float momentum, float* out, float* workspace, void* stream) {
    using namespace dws;
    const char* who = "dws_griffin_lim";
    const int rc = gl_check(who, "magnitude", magnitude, B, f_max, lengths, lengths_host, window, n_fft, hop, out, workspace);
    if (rc != DWS_OK) return rc;
    DWS_CHECK(n_iters >= 0 && n_iters <= 4096, DWS_ERR_INVALID, "%s: n_iters = %d (needs 0 .. 4096)", who, n_iters);
    DWS_CHECK(momentum >= 0.f && momentum < 1.f, DWS_ERR_INVALID, "%s: momentum = %g (needs 0 <= momentum < 1)", who,
              (double)momentum);
    hipStream_t st = (hipStream_t)stream;
    const int64_t T = (f_max - 1) * hop;
    const int fm = (int)f_max;
    // the accelerated signal y_n lives behind the rows; without momentum the projection reads x_n itself
    float* y = (momentum != 0.f && n_iters > 0) ? workspace + (size_t)B * f_max * n_fft : nullptr;
    const size_t lds_rows = gl_lds_bytes(n_fft, false), lds_proj = gl_lds_bytes(n_fft, true);
    DWS_HIP(hipFuncSetAttribute((const void*)istft_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_rows));
    hipLaunchKernelGGL(istft_rows_kernel, dim3((unsigned)fm, (unsigned)B), dim3(256), lds_rows, st, magnitude, phase0, lengths,
                       window, workspace, (int)T, n_fft, hop, fm);
    DWS_HIP(hipGetLastError());
    int g = gl_gather(workspace, lengths, window, out, y, B, T, n_fft, hop, fm, 0.f, st);
    if (g != DWS_OK) return g;
    if (n_iters > 0)
        DWS_HIP(hipFuncSetAttribute((const void*)gl_project_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_proj));
    for (int it = 0; it < n_iters; ++it) {
        hipLaunchKernelGGL(gl_project_kernel, dim3((unsigned)fm, (unsigned)B), dim3(256), lds_proj, st, y ? y : out, magnitude,
                           lengths, window, workspace, (int)T, n_fft, hop, fm);
        DWS_HIP(hipGetLastError());
        g = gl_gather(workspace, lengths, window, out, y, B, T, n_fft, hop, fm, momentum, st);
        if (g != DWS_OK) return g;
    }
    return DWS_OK;
}

extern "C" int dws_istft(const float* magnitude, const float* phase, int64_t B, int64_t f_max, const int32_t* lengths,
                         const int32_t* lengths_host, const float* window, int32_t n_fft, int32_t hop, float* out,
                         float* workspace, void* stream) {
    using namespace dws;
    const int rc = gl_check("dws_istft", "magnitude", magnitude, B, f_max, lengths, lengths_host, window, n_fft, hop, out, workspace);
    if (rc != DWS_OK) return rc;
    return dws_griffin_lim(magnitude, phase, B, f_max, lengths, lengths_host, window, n_fft, hop, 0, 0.f, out, workspace,
                           stream);
}
