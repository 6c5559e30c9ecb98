// Time-varying spectral filter of the SpecGrad prior (Koizumi et al., Interspeech 2022): out = G+ (F . G x) with G the
// short-time DFT of dws_mel_spectrogram's framing (centred frames, reflected about the clip's OWN ends), G+ the
// normalised overlap-add inverse of dws_istft and F [B][K][f_max] one complex gain per frame and bin -- and the exact
// transpose of that map, out = G^T (conj F . (G+)^T x).  Both directions are a frame kernel of this file (one workgroup of
// 256 threads per frame: all K bins, the complex product, the inverse stage into the workspace row; no spectrogram goes
// to memory) and a gather that exists: istft_gather_kernel forwards, ola_gather_kernel for the adjoint.
//
// Sign: the core's DFT is (cos, +sin), X_core = conj(X_api).  So Y_api = F X_api is Y_core = conj(F) X_core, and the
// adjoint's dX_api = conj(F) dY_api is dX_core = F dY_core: tv_mul below with the sign of the filter's imaginary part.
// No atomics: every result is bitwise reproducible, and row b depends on clip b alone.
#include <cfloat>

#include "stft_core.h"

namespace dws {

// (fr + i s fi) (a + i c) with s = +1 or -1: four products, each rounded on its own, then one add or subtract per part
// -- re = fr a -/+ fi c, im = fr c +/- fi a -- never contracted, so the result does not depend on the compiler's choice.
template <bool CONJ>
__device__ __forceinline__ float2 tv_mul(float fr, float fi, float a, float c) {
#pragma clang fp contract(off)
    const float p0 = fr * a;
    const float p1 = fi * c;
    const float p2 = fr * c;
    const float p3 = fi * a;
    return CONJ ? make_float2(p0 + p1, p2 - p3) : make_float2(p0 - p1, p2 + p3);
}

// Frame f of clip b.  ADJ = false: the windowed frame of x.  ADJ = true: row[i] = w[i] q[f hop + i], q the cotangent
// divided by the window's sum of squares at its padded position (istft_gather_kernel's loop and `tiny` rule), 0 outside
// the clip.  Then the K bins, the product with the filter, the Hermitian weights (before the product in the adjoint,
// after it forwards) and the inverse stage.
template <bool ADJ>
__global__ __launch_bounds__(256) void tv_filter_frame_kernel(const float* __restrict__ x, const float* __restrict__ filt_re,
                                                              const float* __restrict__ filt_im,
                                                              const int* __restrict__ lengths,
                                                              const float* __restrict__ window, float* __restrict__ ws, int T,
                                                              int n_fft, int hop, int f_max) {
    extern __shared__ float2 tv_lds[];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int half = n_fft / 2, nb = half + 1;
    int len;
    const int nf = centred_clip_frames(lengths, b, T, half + 1, hop, len);
    if (f >= nf) return;                                     // the whole workgroup, before any barrier
    float2* tab = tv_lds;                                    // [n_fft]
    float2* d = tab + n_fft;                                 // [nb]
    float* frame = reinterpret_cast<float*>(d + nb);         // [n_fft]
    const float* xb = x + (size_t)b * T;
    if constexpr (!ADJ) {
        load_centred_frame<1>(frame, tab, xb, nullptr, window, f * hop - half, len, n_fft, tid);
    } else {
#pragma clang loop vectorize(disable)
        for (int i = tid; i < n_fft; i += 256) {
            const int p = f * hop + i, j = p - half;
            float v = 0.f;
            if (j >= 0 && j < len) {
                int lo = p - n_fft + 1;
                lo = lo <= 0 ? 0 : (lo + hop - 1) / hop;
                int hi = p / hop;
                if (hi > nf - 1) hi = nf - 1;
                float wss = 0.f;
                for (int g = lo; g <= hi; ++g) {
                    const float w = window[p - g * hop];
                    wss = fmaf(w, w, wss);
                }
                const float gj = xb[j];
                v = (wss > FLT_MIN ? gj / wss : gj) * window[i];
            }
            frame[i] = v;
            tab[i] = twiddle(i, n_fft);
        }
    }
    __syncthreads();
    const float inv_n = 1.f / (float)n_fft;
    for (int k = tid; k < nb; k += 256) {
        float re[1], im[1];
        dft_bin<1>(frame, tab, k, n_fft, n_fft - 1, re, im);
        const size_t at = ((size_t)b * nb + k) * f_max + f;
        const float fr = filt_re[at], fi = filt_im ? filt_im[at] : 0.f;
        if constexpr (!ADJ) {
            const float2 y = tv_mul<true>(fr, fi, re[0], im[0]);
            d[k] = hermitian_row(k, half, inv_n, y.x, y.y);
        } else {
            const float2 dy = hermitian_row(k, half, inv_n, re[0], im[0]);
            d[k] = tv_mul<false>(fr, fi, dy.x, dy.y);
        }
    }
    __syncthreads();
    inverse_rows(d, tab, window, ws + ((size_t)b * f_max + f) * n_fft, n_fft, tid);
}

template <bool ADJ>
static int tv_launch(const float* x, const float* filt_re, const float* filt_im, const int32_t* lengths, const float* window,
                     float* ws, int64_t B, int64_t T, int32_t n_fft, int32_t hop, int f_max, hipStream_t st) {
    const size_t lds = gl_lds_bytes(n_fft, true);
    DWS_HIP(hipFuncSetAttribute((const void*)tv_filter_frame_kernel<ADJ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(tv_filter_frame_kernel<ADJ>, dim3((unsigned)f_max, (unsigned)B), dim3(256), lds, st, x, filt_re, filt_im,
                       lengths, window, ws, (int)T, n_fft, hop, f_max);
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}

}  // namespace dws

extern "C" int dws_tv_filter(const float* x, int64_t B, int64_t f_max, const int32_t* lengths, const int32_t* lengths_host,
                             const float* filt_re, const float* filt_im, const float* window, int32_t n_fft, int32_t hop,
                             int32_t adjoint, float* out, float* workspace, void* stream) {
    using namespace dws;
    const char* who = "dws_tv_filter";
    const int rc = gl_check(who, "x", x, B, f_max, lengths, lengths_host, window, n_fft, hop, out, workspace);
    if (rc != DWS_OK) return rc;
    DWS_CHECK(filt_re, DWS_ERR_INVALID, "%s: null filt_re", who);
    DWS_CHECK(adjoint == 0 || adjoint == 1, DWS_ERR_INVALID, "%s: adjoint = %d (needs 0 or 1)", who, adjoint);
    hipStream_t st = (hipStream_t)stream;
    const int64_t T = (f_max - 1) * hop;
    const int fm = (int)f_max;
    if (!adjoint) {
        const int g = tv_launch<false>(x, filt_re, filt_im, lengths, window, workspace, B, T, n_fft, hop, fm, st);
        return g != DWS_OK ? g : gl_gather(workspace, lengths, window, out, nullptr, B, T, n_fft, hop, fm, 0.f, st);
    }
    const int g = tv_launch<true>(x, filt_re, filt_im, lengths, window, workspace, B, T, n_fft, hop, fm, st);
    return g != DWS_OK ? g : ola_gather(workspace, lengths, out, B, T, n_fft, hop, fm, 0, st);
}
