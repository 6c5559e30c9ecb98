// Mel-spectrogram front-end of the vocoding path (`dataloaders/stft.py:100-244`,
// `dataloaders/mel2samp.py:76-82`): reflect-pad by n_fft/2, windowed DFT magnitude at hop
// `hop`, mel filterbank, log(clamp(., clip)).  One workgroup per frame: the windowed frame,
// the (cos, sin) table and the magnitudes live in LDS; a thread owns DFT bins k = tid, tid+256, ...
// (direct O(n_fft^2 / 2) transform: 63 frames of 1024 samples per second of audio is 33 MFLOP,
// not worth an FFT), then 80 mel rows are reduced by one wave each.
#include "stft_core.h"

namespace dws {

// What both mel kernels start with (framing, table and transform: stft_core.h): frame f = blockIdx.x of clip
// b = blockIdx.y windowed into LDS, its magnitudes, and the mel rows s_m = sum_k W[m,k] mag_k, one wave per row (a lane
// adds its bins in ascending k, then wave_sum).  emit(m, s_m) runs on lane 0 of the row's wave; `ri`, where not null,
// keeps (Re_k, Im_k).  The adjoint calls this very function, so its clamp and zero-magnitude decisions are the forward's.
template <typename Emit>
__device__ __forceinline__ void mel_frame_rows(const float* __restrict__ audio, const float* __restrict__ window,
                                               const float* __restrict__ basis, float2* __restrict__ tab,
                                               float* __restrict__ frame, float* __restrict__ mag, float2* __restrict__ ri,
                                               int T, int n_fft, int hop, int n_mels, Emit emit) {
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int half = n_fft / 2, nb = half + 1;
    load_centred_frame<1>(frame, tab, audio + (size_t)b * T, nullptr, window, f * hop - half, T, n_fft, tid);
    __syncthreads();
    for (int k = tid; k < nb; k += 256) {
        float re[1], im[1];
        dft_bin<1>(frame, tab, k, n_fft, n_fft - 1, re, im);
        if (ri) ri[k] = make_float2(re[0], im[0]);
        mag[k] = sqrtf(re[0] * re[0] + im[0] * im[0]);
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int m = wave; m < n_mels; m += 4) {
        const float* w = basis + (size_t)m * nb;
        float s = 0.f;
        for (int k = lane; k < nb; k += 64) s = fmaf(w[k], mag[k], s);
        s = wave_sum(s);
        if (lane == 0) emit(m, s);
    }
}

__global__ __launch_bounds__(256) void mel_frame_kernel(const float* __restrict__ audio, const float* __restrict__ window,
                                                        const float* __restrict__ basis, float* __restrict__ out, int T,
                                                        int n_fft, int hop, int n_mels, int n_frames, float clip) {
    extern __shared__ float2 mel_lds[];
    float2* tab = mel_lds;                                   // [n_fft] (cos, sin)(2 pi j / n_fft)
    float* frame = reinterpret_cast<float*>(tab + n_fft);    // [n_fft]
    float* mag = frame + n_fft;                              // [n_fft/2 + 1]
    const int f = blockIdx.x, b = blockIdx.y;
    mel_frame_rows(audio, window, basis, tab, frame, mag, nullptr, T, n_fft, hop, n_mels, [&](int m, float s) {
        out[((size_t)b * n_mels + m) * n_frames + f] = logf(fmaxf(s, clip));
    });
}

// Adjoint, stage 1 of 2: one workgroup per (frame, clip).  Re/Im of the frame and the mel rows s_m are mel_frame_rows',
// then
//   ds_m = g[m,f] / s_m  (0 where s_m <= clip),   dmag_k = sum_m W[m,k] ds_m  (ascending m),
//   dRe_k = dmag_k Re_k / mag_k,  dIm_k = dmag_k Im_k / mag_k  (both 0 where mag_k == 0),
//   ws[b,f,i] = w[i] sum_k (dRe_k cos(2 pi i k / N) + dIm_k sin(2 pi i k / N))  (ascending k: idft_sample).
// Nothing is accumulated across workgroups here: the overlap-add is ola_gather_kernel's.
__global__ __launch_bounds__(256) void mel_frame_backward_kernel(const float* __restrict__ audio, const float* __restrict__ window,
                                                                 const float* __restrict__ basis, const float* __restrict__ dout,
                                                                 float* __restrict__ ws, int T, int n_fft, int hop, int n_mels,
                                                                 int n_frames, float clip) {
    extern __shared__ float2 mel_lds[];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int nb = n_fft / 2 + 1;
    float2* tab = mel_lds;                                   // [n_fft]
    float2* dri = tab + n_fft;                               // [nb] (Re_k, Im_k), then (dRe_k, dIm_k)
    float* frame = reinterpret_cast<float*>(dri + nb);       // [n_fft]
    float* mag = frame + n_fft;                              // [nb]
    float* ds = mag + nb;                                    // [n_mels]
    mel_frame_rows(audio, window, basis, tab, frame, mag, dri, T, n_fft, hop, n_mels, [&](int m, float s) {
        // the clamp passes no gradient at or below `clip` (the tie s == clip counts as clamped)
        ds[m] = s > clip ? dout[((size_t)b * n_mels + m) * n_frames + f] / s : 0.f;
    });
    __syncthreads();
    for (int k = tid; k < nb; k += 256) {
        float dmag = 0.f;
        for (int m = 0; m < n_mels; ++m) dmag = fmaf(basis[(size_t)m * nb + k], ds[m], dmag);
        const float mk = mag[k];
        const float t = mk > 0.f ? dmag / mk : 0.f;      // |z| has no gradient at 0: a silent bin contributes exactly 0
        const float2 r = dri[k];
        dri[k] = make_float2(t * r.x, t * r.y);
    }
    __syncthreads();
    float* o = ws + ((size_t)b * n_frames + f) * n_fft;
    for (int i = tid; i < n_fft; i += 256) o[i] = window[i] * idft_sample(dri, tab, i, nb, n_fft - 1);
}

// Adaptive prior (PriorGrad, Lee et al., ICLR 2022): the per-sample standard deviation read off the frame energy of a
// log-mel m [B, bands, frames],
//   energy[b, f] = sqrt(sum_k exp(m[b, k, f])),  sigma_f = clamp((energy - e_min) / (e_max - e_min), std_min, 1),
//   sigma[b, 0, l] = sigma_f[b, l / hop]          l = 0 .. L - 1.
// One workgroup per (PRIOR_FRAMES frames, clip).  Lane f of the first wave owns a frame (neighbouring lanes read
// neighbouring frames of a band row) and adds its bands in a fixed order: band k into partial sum k % 8 in ascending k,
// then the tree ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)).  A frame's value so depends on its own column alone,
// not on B or the launch shape.  All 256 threads then write the frames' span of the row: single floats up to the first
// 16-byte border of the output, float4 from there, single floats behind the last whole group.
constexpr int PRIOR_FRAMES = 64;

__global__ __launch_bounds__(256) void prior_std_kernel(const float* __restrict__ mel, float* __restrict__ sigma, int bands,
                                                        int64_t frames, int64_t hop, int64_t L, float e_min, float e_max,
                                                        float std_min) {
    __shared__ float sf[PRIOR_FRAMES];
    const int64_t f0 = (int64_t)blockIdx.x * PRIOR_FRAMES;
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid < PRIOR_FRAMES) {
        float v = 0.f;
        const int64_t f = f0 + tid;
        if (f < frames) {
            const float* col = mel + (size_t)b * bands * frames + f;
            // eight partial sums, band k into partial k % 8 in ascending k, then one fixed tree: for 80 bands a value
            // passes through 13 additions, not the 80 of one running sum, and collects that much less rounding
            float part[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            int k = 0;
            for (; k + 8 <= bands; k += 8) {
#pragma unroll
                for (int j = 0; j < 8; ++j) part[j] += expf(col[(size_t)(k + j) * frames]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (k + j < bands) part[j] += expf(col[(size_t)(k + j) * frames]);
            const float acc = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
            const float e = (sqrtf(acc) - e_min) / (e_max - e_min);
            v = fminf(fmaxf(e, std_min), 1.0f);
        }
        sf[tid] = v;
    }
    __syncthreads();
    const int64_t lo = f0 * hop;                                                   // this block's span [lo, hi) of the row
    const int64_t hi = (f0 + PRIOR_FRAMES) * hop < L ? (f0 + PRIOR_FRAMES) * hop : L;
    if (lo >= hi) return;
    float* row = sigma + (size_t)b * L;
    const bool base16 = ((uintptr_t)sigma & 15) == 0;
    // first element at or behind lo whose address is a 16-byte border (every element when the base is not aligned: no body)
    int64_t head = base16 ? lo + (int64_t)((4 - (((size_t)b * L + lo) & 3)) & 3) : hi;
    if (head > hi) head = hi;
    const int64_t groups = (hi - head) / 4, tail = head + groups * 4;
    for (int64_t i = lo + tid; i < head; i += 256) row[i] = sf[i / hop - f0];
    for (int64_t g = tid; g < groups; g += 256) {
        const int64_t i = head + g * 4;
        *reinterpret_cast<float4*>(row + i) =
            make_float4(sf[i / hop - f0], sf[(i + 1) / hop - f0], sf[(i + 2) / hop - f0], sf[(i + 3) / hop - f0]);
    }
    for (int64_t i = tail + tid; i < hi; i += 256) row[i] = sf[i / hop - f0];
}

}  // namespace dws

extern "C" int dws_prior_std_from_mel(const float* mel, int64_t B, int64_t bands, int64_t frames, int64_t hop, int64_t L,
                                      float e_min, float e_max, float std_min, float* sigma, void* stream) {
    using namespace dws;
    DWS_CHECK(mel && sigma, DWS_ERR_INVALID, "dws_prior_std_from_mel: null argument");
    DWS_CHECK(B > 0 && B <= 65535 && bands > 0 && bands <= INT32_MAX && frames > 0 && hop > 0, DWS_ERR_INVALID,
              "dws_prior_std_from_mel: bad shape (B = %lld, bands = %lld, frames = %lld, hop = %lld)", (long long)B,
              (long long)bands, (long long)frames, (long long)hop);
    DWS_CHECK(frames <= INT64_MAX / hop && L >= 1 && L <= frames * hop, DWS_ERR_INVALID,
              "dws_prior_std_from_mel: L = %lld (needs 1 .. frames * hop = %lld * %lld)", (long long)L, (long long)frames,
              (long long)hop);
    DWS_CHECK(e_min == e_min && e_max - e_max == 0.f && e_min - e_min == 0.f && e_max > e_min, DWS_ERR_INVALID,
              "dws_prior_std_from_mel: energy range %g .. %g (needs finite values, e_max > e_min)", (double)e_min,
              (double)e_max);
    DWS_CHECK(std_min > 0.f && std_min <= 1.f, DWS_ERR_INVALID, "dws_prior_std_from_mel: std_min = %g (needs 0 < std_min <= 1)",
              (double)std_min);
    // frames whose span lies wholly behind L write nothing: launch only the blocks that hold a sample
    const int64_t used = (L + hop - 1) / hop;
    const int64_t blocks = (used + PRIOR_FRAMES - 1) / PRIOR_FRAMES;
    DWS_CHECK(blocks <= INT32_MAX, DWS_ERR_INVALID, "dws_prior_std_from_mel: %lld frames", (long long)used);
    hipLaunchKernelGGL(prior_std_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, (hipStream_t)stream, mel, sigma,
                       (int)bands, frames, hop, L, e_min, e_max, std_min);
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}

extern "C" int dws_mel_spectrogram_backward(const float* audio, int64_t B, int64_t T, const float* window,
                                            const float* mel_basis, int32_t n_fft, int32_t hop, int32_t n_mels, float clip,
                                            const float* dout, float* daudio, float* workspace, void* stream) {
    using namespace dws;
    DWS_CHECK(audio && window && mel_basis && dout && daudio, DWS_ERR_INVALID, "dws_mel_spectrogram_backward: null argument");
    DWS_CHECK(workspace, DWS_ERR_INVALID, "dws_mel_spectrogram_backward: null workspace ([B][T/hop+1][n_fft] floats)");
    DWS_CHECK(B > 0 && hop > 0 && n_mels > 0, DWS_ERR_INVALID, "dws_mel_spectrogram_backward: bad shape");
    DWS_CHECK(n_fft_ok(n_fft, 4096), DWS_ERR_UNSUPPORTED,
              "dws_mel_spectrogram_backward: filter_length %d (powers of two 64..4096 are built)", n_fft);
    DWS_CHECK(T > n_fft / 2, DWS_ERR_INVALID,
              "dws_mel_spectrogram_backward: reflect padding needs T > filter_length/2 (`stft.py:127-131`)");
    const int n_frames = (int)(T / hop) + 1;
    const size_t lds = ((size_t)3 * n_fft + 3 * (size_t)(n_fft / 2 + 1) + (size_t)n_mels) * 4;
    DWS_CHECK(lds <= 160 * 1024, DWS_ERR_UNSUPPORTED, "dws_mel_spectrogram_backward: %d mel bands at filter_length %d need %zu "
              "bytes of LDS (160 KiB per workgroup)", n_mels, n_fft, lds);
    DWS_HIP(hipFuncSetAttribute((const void*)mel_frame_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(mel_frame_backward_kernel, dim3(n_frames, (unsigned)B), dim3(256), lds, (hipStream_t)stream, audio,
                       window, mel_basis, dout, workspace, (int)T, n_fft, hop, n_mels, n_frames, clip);
    DWS_HIP(hipGetLastError());
    return ola_gather(workspace, nullptr, daudio, B, T, n_fft, hop, n_frames, 0, (hipStream_t)stream);
}

extern "C" int dws_mel_spectrogram(const float* audio, int64_t B, int64_t T, const float* window, const float* mel_basis,
                                   int32_t n_fft, int32_t hop, int32_t n_mels, float clip, float* out, void* stream) {
    using namespace dws;
    DWS_CHECK(audio && window && mel_basis && out, DWS_ERR_INVALID, "dws_mel_spectrogram: null argument");
    DWS_CHECK(B > 0 && hop > 0 && n_mels > 0, DWS_ERR_INVALID, "dws_mel_spectrogram: bad shape");
    DWS_CHECK(n_fft_ok(n_fft, 4096), DWS_ERR_UNSUPPORTED,
              "dws_mel_spectrogram: filter_length %d (powers of two 64..4096 are built)", n_fft);
    DWS_CHECK(T > n_fft / 2, DWS_ERR_INVALID, "dws_mel_spectrogram: reflect padding needs T > filter_length/2 (`stft.py:127-131`)");
    const int n_frames = (int)(T / hop) + 1;
    const size_t lds = (size_t)(3 * n_fft + n_fft / 2 + 1) * 4;
    DWS_HIP(hipFuncSetAttribute((const void*)mel_frame_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(mel_frame_kernel, dim3(n_frames, (unsigned)B), dim3(256), lds, (hipStream_t)stream, audio, window,
                       mel_basis, out, (int)T, n_fft, hop, n_mels, n_frames, clip);
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}
