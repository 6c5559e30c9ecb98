// Objective spectral distances between two batches of waveforms x (generated) and y (reference), one fused launch per
// STFT resolution: Parallel WaveGAN's multi-resolution STFT terms (spectral convergence, log-magnitude L1), the
// log-spectral distance, and -- where a mel filterbank is passed -- the log-mel L1 and a mel-cepstral distortion.  No
// spectrogram goes to memory: a workgroup owns frame f of clip b of BOTH signals and writes six partial sums.
//
// Framing and transform are stft_core.h's, on two signals: reflect-pad by n_fft/2 about the clip's OWN end len_b (a
// ragged batch: nothing behind len_b is read, so the padding may hold anything), windowed direct DFT, a thread owns bins
// k = tid, tid + 256, ..., the frames of x and y interleaved in LDS.
//
// Reduction, in a fixed order: a thread adds its bins in ascending k (fp32), a wave adds its lanes by wave_sum
// (fp32), thread 0 adds the four waves in wave order (double).  The mel terms take ln() and the cepstral products in
// double: with x = y / 2 the band differences are then ln 2 to the last bit and the distortion cancels to 1e-16, where
// fp32 logs would leave 1e-5 dB of rounding noise.  spectral_clip_sum_kernel adds a clip's frames in ascending order in
// double.  A clip's six numbers depend on its own samples and length alone.
#include "stft_core.h"

namespace dws {

constexpr int SPEC_Q = 6;                 // sc_num, sc_den, mag_abs, lsd, mel_abs, mcd
constexpr float SPEC_FLOOR = 1e-7f;       // Parallel WaveGAN: |X| = sqrt(max(re^2 + im^2, 1e-7))

// What both frame kernels start with: frame f of clip b (len samples) of x and y windowed into fr, the table into tab.
__device__ __forceinline__ void spectral_load(const float* __restrict__ x, const float* __restrict__ y,
                                              const float* __restrict__ window, float2* __restrict__ fr,
                                              float2* __restrict__ tab, int f, int b, int T, int len, int n_fft, int hop) {
    load_centred_frame<2>(fr, tab, x + (size_t)b * T, y + (size_t)b * T, window, f * hop - n_fft / 2, len, n_fft,
                          threadIdx.x);
    __syncthreads();
}

// ... and go on with per bin: Re/Im of X (index 0) and Y (1), and the unfloored powers px = |X|^2, py = |Y|^2 every
// floor decision of the forward and of the adjoint is taken on.  Re/Im are the same bits in both kernels (fmaf only).
// The powers are left to the compiler's contraction, per kernel: today an fma on the rounded re^2 in the forward, two
// rounded products and an add in the adjoint, so at a tie within one rounding of the floor the two can decide
// differently.  Writing the form out would change the results of one of them.
__device__ __forceinline__ void spectral_bin(const float2* __restrict__ fr, const float2* __restrict__ tab, int k, int n_fft,
                                             float (&re)[2], float (&im)[2], float& px, float& py) {
    dft_bin<2>(fr, tab, k, n_fft, n_fft - 1, re, im);
    px = re[0] * re[0] + im[0] * im[0];
    py = re[1] * re[1] + im[1] * im[1];
}

__global__ __launch_bounds__(256) void spectral_frame_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             const int* __restrict__ lengths, const float* __restrict__ window,
                                                             const float* __restrict__ basis, const double* __restrict__ cep,
                                                             double* __restrict__ ws, int T, int n_fft, int hop, int n_mels,
                                                             int n_cep, int f_max, float clip) {
    extern __shared__ double lds64[];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int half = n_fft / 2, nb = half + 1;
    int len;
    if (f >= centred_clip_frames(lengths, b, T, half + 1, hop, len)) return;   // the whole workgroup, before any barrier
    double* red = lds64;                                   // [4 waves][4]
    double* dl = red + 16;                                 // [n_mels] logmel(Y) - logmel(X)
    double* c2 = dl + n_mels;                              // [n_cep]  squared cepstral differences
    float2* fr = reinterpret_cast<float2*>(c2 + n_cep);    // [n_fft]  (x, y) windowed
    float2* tab = fr + n_fft;                              // [n_fft]  (cos, sin)(2 pi j / n_fft)
    float* magx = reinterpret_cast<float*>(tab + n_fft);   // [nb] unfloored |X|, with a filterbank only
    float* magy = magx + nb;                               // [nb]
    spectral_load(x, y, window, fr, tab, f, b, T, len, n_fft, hop);       // len > half keeps every index in [0, len)
    float a_num = 0.f, a_den = 0.f, a_abs = 0.f, a_lsd = 0.f;
    for (int k = tid; k < nb; k += 256) {
        float re[2], im[2], px, py;
        spectral_bin(fr, tab, k, n_fft, re, im, px, py);
        if (basis) {
            magx[k] = sqrtf(px);
            magy[k] = sqrtf(py);
        }
        const float qx = px < SPEC_FLOOR ? SPEC_FLOOR : px;      // (a NaN passes: fmaxf would hide it)
        const float qy = py < SPEC_FLOOR ? SPEC_FLOOR : py;
        const float mx = sqrtf(qx), my = sqrtf(qy);
        const float d = my - mx;
        a_num = fmaf(d, d, a_num);
        a_den = fmaf(my, my, a_den);
        const float l = 0.5f * (logf(qy) - logf(qx));            // ln|Y| - ln|X|
        a_abs += fabsf(l);
        a_lsd = fmaf(l, l, a_lsd);
    }
    const int wave = tid >> 6, lane = tid & 63;
    // wave_sum's tree for the four sums at once: written as one loop the 24 shuffles overlap, as four calls they queue up
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a_num += __shfl_xor(a_num, off);
        a_den += __shfl_xor(a_den, off);
        a_abs += __shfl_xor(a_abs, off);
        a_lsd += __shfl_xor(a_lsd, off);
    }
    if (lane == 0) {
        red[wave * 4 + 0] = (double)a_num;
        red[wave * 4 + 1] = (double)a_den;
        red[wave * 4 + 2] = (double)a_abs;
        red[wave * 4 + 3] = (double)a_lsd;
    }
    __syncthreads();                     // red, and magx / magy
    double* o = ws + ((size_t)b * f_max + f) * SPEC_Q;
    if (tid == 0) {
        double r[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = ((red[q] + red[4 + q]) + red[8 + q]) + red[12 + q];
        o[0] = r[0];
        o[1] = r[1];
        o[2] = r[2];
        // sqrt(mean_k (log10|Y|^2 - log10|X|^2)^2) = (2 / ln 10) sqrt(mean_k (ln|Y| - ln|X|)^2)
        o[3] = 0.86858896380650365530 * sqrt(r[3] / (double)nb);
        if (!basis) {
            o[4] = 0.0;
            o[5] = 0.0;
        }
    }
    if (!basis) return;                  // (a kernel argument: the whole workgroup)
    for (int m = wave; m < n_mels; m += 4) {
        const float* w = basis + (size_t)m * nb;
        float sx = 0.f, sy = 0.f;
        for (int k = lane; k < nb; k += 64) {
            const float wk = w[k];
            sx = fmaf(wk, magx[k], sx);
            sy = fmaf(wk, magy[k], sy);
        }
        sx = wave_sum(sx);
        sy = wave_sum(sy);
        if (lane == 0) dl[m] = log((double)(sy < clip ? clip : sy)) - log((double)(sx < clip ? clip : sx));
    }
    __syncthreads();
    if (tid < n_cep) {
        const double* row = cep + (size_t)tid * n_mels;
        double c = 0.0;
        for (int m = 0; m < n_mels; ++m) c = fma(row[m], dl[m], c);
        c2[tid] = c * c;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int m = 0; m < n_mels; ++m) s += fabs(dl[m]);
        o[4] = s;
        double e = 0.0;
        for (int d = 0; d < n_cep; ++d) e += c2[d];
        o[5] = sqrt(e);
    }
}

// One thread per (clip, quantity): the clip's frames in ascending order, in double.
__global__ __launch_bounds__(64) void spectral_clip_sum_kernel(const double* __restrict__ ws, const int* __restrict__ lengths,
                                                               double* __restrict__ out, int T, int n_fft, int hop, int f_max) {
    const int b = blockIdx.x, q = threadIdx.x;
    if (q >= SPEC_Q) return;
    int len;
    const int nf = centred_clip_frames(lengths, b, T, n_fft / 2 + 1, hop, len);
    const double* p = ws + (size_t)b * f_max * SPEC_Q + q;
    double s = 0.0;
    for (int f = 0; f < nf; ++f) s += p[(size_t)f * SPEC_Q];
    out[(size_t)b * SPEC_Q + q] = s;
}

// Adjoint of the two Parallel WaveGAN terms (sums 0 .. 2) with respect to x, stage 1 of 2: one workgroup per (frame,
// clip).  Re/Im of x and y and the two powers are recomputed by the forward's own spectral_load and spectral_bin, so
// the floor decisions are the forward's (up to the contraction noted there).  With c0, c1 = coef[b][0], coef[b][1]
//   dmag_k = -(c0 (|Y|_k - |X|_k) + c1 sgn(ln|Y|_k - ln|X|_k) / |X|_k)     where p_x >= 1e-7, else 0   (sgn(0) = 0)
//   dRe_k = dmag_k Re_k / |X|_k,   dIm_k = dmag_k Im_k / |X|_k
//   ws[b,f,i] = w[i] sum_k (dRe_k cos(2 pi i k / N) + dIm_k sin(2 pi i k / N))      (k = 0 .. N/2 ascending)
// Nothing is accumulated across workgroups: the overlap-add is ola_gather_kernel's.
//
// LDS: the forward's 16 N bytes and 8 K bytes of (dRe, dIm).  The inverse stage (idft_sample) reads the table at
// (i k) & (N - 1) with a lane stride of k float2 -- conflict-free for odd k, 2^m-way where k = 2^m (odd) until the lanes
// start to share addresses; the same cost profile as the forward's table reads at lane stride i, so the inverse runs at
// the forward's LDS rate with half its FMAs per read pair.
__global__ __launch_bounds__(256) void spectral_frame_backward_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                      const int* __restrict__ lengths,
                                                                      const float* __restrict__ window,
                                                                      const double* __restrict__ coef, float* __restrict__ ws,
                                                                      int T, int n_fft, int hop, int f_max) {
    extern __shared__ double lds64[];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int half = n_fft / 2, nb = half + 1;
    int len;
    if (f >= centred_clip_frames(lengths, b, T, half + 1, hop, len)) return;   // the whole workgroup, before any barrier
    float2* fr = reinterpret_cast<float2*>(lds64);         // [n_fft]  (x, y) windowed
    float2* tab = fr + n_fft;                              // [n_fft]  (cos, sin)(2 pi j / n_fft)
    float2* dri = tab + n_fft;                             // [nb]     (dRe, dIm)
    spectral_load(x, y, window, fr, tab, f, b, T, len, n_fft, hop);
    const float c0 = (float)coef[(size_t)b * 2], c1 = (float)coef[(size_t)b * 2 + 1];
    for (int k = tid; k < nb; k += 256) {
        float re[2], im[2], px, py;
        spectral_bin(fr, tab, k, n_fft, re, im, px, py);
        float2 d = make_float2(0.f, 0.f);
        if (px >= SPEC_FLOOR) {          // the floor passes no gradient below it (the tie counts as passed: clamp_min's rule)
            const float qy = py < SPEC_FLOOR ? SPEC_FLOOR : py;
            const float mx = sqrtf(px), my = sqrtf(qy);
            const float l = 0.5f * (logf(qy) - logf(px));
            const float sg = l > 0.f ? 1.f : (l < 0.f ? -1.f : 0.f);
            const float t = -(c0 * (my - mx) + c1 * sg / mx) / mx;
            d = make_float2(t * re[0], t * im[0]);
        }
        dri[k] = d;
    }
    __syncthreads();
    float* o = ws + ((size_t)b * f_max + f) * n_fft;
    for (int i = tid; i < n_fft; i += 256) o[i] = window[i] * idft_sample(dri, tab, i, nb, n_fft - 1);
}

// Adjoint, stage 2 of 2, of this file's loss and of the mel front-end's (ola_gather): one thread per sample.  Sample j < len_b sits at padded position j + N/2 and, through the
// reflection about the clip's OWN ends, at N/2 - j (j = 1 .. N/2) and at N/2 + 2 (len_b - 1) - j
// (j = len_b - 1 - N/2 .. len_b - 2) -- at len_b <= N/2 + 1 at both at once.  Summed in a fixed order: the direct
// position, the left reflection, the right reflection, each in ascending frame order; a sample no frame covers
// (hop > N) gets exactly 0.  Behind len_b: exactly 0 without `accumulate`, untouched with it.
__global__ __launch_bounds__(256) void ola_gather_kernel(const float* __restrict__ ws, const int* __restrict__ lengths,
                                                         float* __restrict__ dx, int T, int n_fft, int hop, int f_max,
                                                         int accumulate) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= T) return;
    const int half = n_fft / 2;
    int len;
    const int nf = centred_clip_frames(lengths, b, T, half + 1, hop, len);
    float* o = dx + (size_t)b * T + j;
    if (nf == 0 || j >= len) {
        if (!accumulate) *o = 0.f;
        return;
    }
    const float* wsb = ws + (size_t)b * f_max * n_fft;
    float acc = ola_gather_position(wsb, j + half, n_fft, hop, nf, 0.f);
    if (j >= 1 && j <= half) acc = ola_gather_position(wsb, half - j, n_fft, hop, nf, acc);
    if (j <= len - 2 && j >= len - 1 - half) acc = ola_gather_position(wsb, half + 2 * (len - 1) - j, n_fft, hop, nf, acc);
    *o = accumulate ? *o + acc : acc;
}

int ola_gather(const float* ws, const int32_t* lengths, float* dx, int64_t B, int64_t T, int32_t n_fft, int32_t hop,
               int f_max, int32_t accumulate, hipStream_t stream) {
    hipLaunchKernelGGL(ola_gather_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)B), dim3(256), 0, stream, ws, lengths,
                       dx, (int)T, n_fft, hop, f_max, accumulate);
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}

}  // namespace dws

extern "C" int64_t dws_spectral_loss_backward_workspace(int64_t B, int64_t T, int32_t n_fft, int32_t hop) {
    if (B < 1 || T < 1 || hop < 1 || T > INT32_MAX || B > 65535 || !dws::n_fft_ok(n_fft, 2048)) return 0;
    return B * (T / hop + 1) * (int64_t)n_fft * (int64_t)sizeof(float);
}

extern "C" int dws_spectral_loss_backward(const float* x, const float* y, int64_t B, int64_t T, const int32_t* lengths,
                                          const int32_t* lengths_host, const float* window, int32_t n_fft, int32_t hop,
                                          const double* coef, float* dx, int32_t accumulate, float* workspace, void* stream) {
    using namespace dws;
    DWS_CHECK(x && y && window && coef && dx, DWS_ERR_INVALID, "dws_spectral_loss_backward: null argument");
    DWS_CHECK(workspace, DWS_ERR_INVALID,
              "dws_spectral_loss_backward: null workspace (dws_spectral_loss_backward_workspace bytes)");
    DWS_CHECK(n_fft_ok(n_fft, 2048), DWS_ERR_INVALID, "dws_spectral_loss_backward: n_fft = %d (powers of two 64..2048)",
              n_fft);
    DWS_CHECK(B > 0 && B <= 65535 && hop > 0 && T > 0 && T <= INT32_MAX - n_fft, DWS_ERR_INVALID,
              "dws_spectral_loss_backward: bad shape (B = %lld, T = %lld, hop = %d)", (long long)B, (long long)T, hop);
    // reflect padding: a clip holds at least n_fft / 2 + 1 samples
    if (check_clip_lengths("dws_spectral_loss_backward", B, T, lengths, lengths_host, n_fft / 2 + 1) < 0) return DWS_ERR_INVALID;
    const int f_max = (int)(T / hop) + 1;
    const size_t lds = (size_t)n_fft * 16 + (size_t)(n_fft / 2 + 1) * 8;
    DWS_HIP(hipFuncSetAttribute((const void*)spectral_frame_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
    hipLaunchKernelGGL(spectral_frame_backward_kernel, dim3((unsigned)f_max, (unsigned)B), dim3(256), lds, (hipStream_t)stream,
                       x, y, lengths, window, coef, workspace, (int)T, n_fft, hop, f_max);
    DWS_HIP(hipGetLastError());
    return ola_gather(workspace, lengths, dx, B, T, n_fft, hop, f_max, accumulate, (hipStream_t)stream);
}

extern "C" int64_t dws_spectral_distance_workspace(int64_t B, int64_t T, int32_t hop) {
    if (B < 1 || T < 1 || hop < 1 || T > INT32_MAX || B > 65535) return 0;
    return B * (T / hop + 1) * dws::SPEC_Q * (int64_t)sizeof(double);
}

extern "C" int dws_spectral_distance(const float* x, const float* y, int64_t B, int64_t T, const int32_t* lengths,
                                     const int32_t* lengths_host, const float* window, int32_t n_fft, int32_t hop,
                                     const float* mel_basis, int32_t n_mels, float clip, const double* cep, int32_t n_cep,
                                     double* workspace, double* out, void* stream) {
    using namespace dws;
    DWS_CHECK(x && y && window && out, DWS_ERR_INVALID, "dws_spectral_distance: null argument");
    DWS_CHECK(workspace, DWS_ERR_INVALID, "dws_spectral_distance: null workspace (dws_spectral_distance_workspace bytes)");
    DWS_CHECK(n_fft_ok(n_fft, 2048), DWS_ERR_INVALID, "dws_spectral_distance: n_fft = %d (powers of two 64..2048)", n_fft);
    DWS_CHECK(B > 0 && B <= 65535 && hop > 0 && T > 0 && T <= INT32_MAX - n_fft, DWS_ERR_INVALID,
              "dws_spectral_distance: bad shape (B = %lld, T = %lld, hop = %d)", (long long)B, (long long)T, hop);
    // reflect padding: a clip holds at least n_fft / 2 + 1 samples
    if (check_clip_lengths("dws_spectral_distance", B, T, lengths, lengths_host, n_fft / 2 + 1) < 0) return DWS_ERR_INVALID;
    DWS_CHECK(mel_basis ? (n_mels > 0 && n_mels <= 4096) : (n_mels == 0 && cep == nullptr), DWS_ERR_INVALID,
              "dws_spectral_distance: n_mels = %d %s a filterbank (a cepstral table needs one)", n_mels,
              mel_basis ? "with" : "without");
    DWS_CHECK(cep ? (n_cep > 0 && n_cep <= 256) : n_cep == 0, DWS_ERR_INVALID,
              "dws_spectral_distance: n_cep = %d %s a cepstral table (1..256 rows, one thread each)", n_cep,
              cep ? "with" : "without");
    const int f_max = (int)(T / hop) + 1;
    const size_t lds = (size_t)(16 + n_mels + n_cep) * 8 + (size_t)n_fft * 16 + (mel_basis ? (size_t)(n_fft / 2 + 1) * 8 : 0);
    DWS_CHECK(lds <= 160 * 1024, DWS_ERR_INVALID, "dws_spectral_distance: %zu bytes of LDS (160 KiB per workgroup)", lds);
    DWS_HIP(hipFuncSetAttribute((const void*)spectral_frame_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(spectral_frame_kernel, dim3((unsigned)f_max, (unsigned)B), dim3(256), lds, (hipStream_t)stream, x, y,
                       lengths, window, mel_basis, cep, workspace, (int)T, n_fft, hop, n_mels, n_cep, f_max, clip);
    DWS_HIP(hipGetLastError());
    hipLaunchKernelGGL(spectral_clip_sum_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, workspace, lengths, out,
                       (int)T, n_fft, hop, f_max);
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}
