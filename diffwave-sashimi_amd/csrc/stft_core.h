// The short-time DFT core of the analysis kernels (mel_kernels, spectral_kernels, stoi_kernels, pitch_kernels) and of the
// inversion kernels (griffinlim_kernels and tvfilter_kernels, whose frame kernels are a forward and an inverse stage in one
// workgroup): every piece the files share exists here once, so the adjoints recompute the forward's numbers -- and take
// its clamp and floor decisions -- by calling the forward's own code.
//
// Layout: a workgroup of 256 threads owns one frame.  The twiddle table is float2 (cos, sin)(2 pi i / n_fft), i = 0 ..
// n_fft - 1, in LDS on an 8-byte border; the frame sits next to it as float (one signal) or float2 (x, y) (two signals),
// so one 8-byte table read and one frame read (one address for the whole wave: a broadcast) feed 2 or 4 FMAs.
// Loop order: a thread owns bins k = tid, tid + 256, ... and walks the samples in ascending i with the table index
// (i k) & (n_fft - 1) kept as a running sum; per sample Re before Im, x before y.  The inverse stage swaps the roles: a
// thread owns sample i and walks the bins in ascending k, the cos term before the sin term.
// Reduction order: a wave adds its lanes by the xor tree off = 32, 16, ... 1 (wave_sum); what is added across waves or
// frames is each kernel's own and stated there.  No atomics anywhere: every result is bitwise reproducible.
#pragma once
#include <type_traits>

#include "dws_common.h"

namespace dws {

// Index j of a signal padded by reflection without edge repeat: ... s[2] s[1] | s[0] .. s[len - 1] | s[len - 2] ...
// One reflection per side: the caller's minimum length keeps the result in [0, len).
__device__ __forceinline__ int reflect_index(int j, int len) {
    if (j < 0) j = -j;
    if (j >= len) j = 2 * (len - 1) - j;
    return j;
}

__device__ __forceinline__ float2 twiddle(int i, int n_fft) {
    float s, c;
    sincospif(2.f * (float)i / (float)n_fft, &s, &c);
    return make_float2(c, s);
}

template <int NSIG>
using frame_vec = std::conditional_t<NSIG == 2, float2, float>;

// Frame and table in ONE pass over i: the windowed n_fft samples from `start` on (start = f hop - n_fft / 2 for frame f)
// of s0, or of s0 and s1 interleaved, reflected about the clip's own `len`; nothing at or behind len is read.  Not
// vectorised: the loop vectoriser would pair two trips for packed fp32, and at most 16 trips once per workgroup do not
// pay for a second copy of the sincospif body in registers and code.
template <int NSIG>
__device__ __forceinline__ void load_centred_frame(frame_vec<NSIG>* __restrict__ frame, float2* __restrict__ tab,
                                                   const float* __restrict__ s0, const float* __restrict__ s1,
                                                   const float* __restrict__ window, int start, int len, int n_fft,
                                                   int tid) {
#pragma clang loop vectorize(disable)
    for (int i = tid; i < n_fft; i += 256) {
        const int j = reflect_index(start + i, len);
        const float w = window[i];
        if constexpr (NSIG == 1) frame[i] = s0[j] * w;
        else frame[i] = make_float2(s0[j] * w, s1[j] * w);
        tab[i] = twiddle(i, n_fft);
    }
}

// Bin k of the n_fft-point DFT (mask = n_fft - 1, a power of two) of the first n_samples samples of `frame`:
// re[s] + i im[s] = sum_i frame[i][s] (cos + i sin)(2 pi i k / n_fft), direct, in ascending i.
template <int NSIG>
__device__ __forceinline__ void dft_bin(const frame_vec<NSIG>* __restrict__ frame, const float2* __restrict__ tab, int k,
                                        int n_samples, int mask, float (&re)[NSIG], float (&im)[NSIG]) {
    float xr = 0.f, xi = 0.f, yr = 0.f, yi = 0.f;
    int ph = 0;
    for (int i = 0; i < n_samples; ++i) {
        const frame_vec<NSIG> v = frame[i];
        const float2 t = tab[ph];
        if constexpr (NSIG == 1) {
            xr = fmaf(v, t.x, xr);
            xi = fmaf(v, t.y, xi);
        } else {
            xr = fmaf(v.x, t.x, xr);
            xi = fmaf(v.x, t.y, xi);
            yr = fmaf(v.y, t.x, yr);
            yi = fmaf(v.y, t.y, yi);
        }
        ph = (ph + k) & mask;
    }
    re[0] = xr;
    im[0] = xi;
    if constexpr (NSIG == 2) {
        re[1] = yr;
        im[1] = yi;
    }
}

// Sample i of the inverse stage of an adjoint: sum_k (dRe_k cos + dIm_k sin)(2 pi i k / n_fft) over the nb rows
// (dRe, dIm) of `d`, in ascending k.  The row is one address for the whole wave (a broadcast), the table is read at lane
// stride k float2: the transform's access pattern with the roles swapped, and half its FMAs per read pair.
__device__ __forceinline__ float idft_sample(const float2* __restrict__ d, const float2* __restrict__ tab, int i, int nb,
                                             int mask) {
    float acc = 0.f;
    int ph = 0;
    for (int k = 0; k < nb; ++k) {
        const float2 v = d[k];
        const float2 t = tab[ph];
        acc = fmaf(v.x, t.x, acc);
        acc = fmaf(v.y, t.y, acc);
        ph = (ph + i) & mask;
    }
    return acc;
}

// Row k of the inverse stage's input: h_k (re, im) with h = 1/N at k = 0 and k = N/2, whose imaginary part does not
// enter (irfft ignores it), and 2/N elsewhere.
__device__ __forceinline__ float2 hermitian_row(int k, int half, float inv_n, float re, float im) {
    const bool edge = k == 0 || k == half;
    const float h = edge ? inv_n : 2.f * inv_n;
    return make_float2(h * re, edge ? 0.f : h * im);
}

// ws[b][f][i] = w[i] sum_k (d_k.x cos + d_k.y sin)(2 pi i k / N): the windowed frame the overlap-add gathers
__device__ __forceinline__ void inverse_rows(const float2* __restrict__ d, const float2* __restrict__ tab,
                                             const float* __restrict__ window, float* __restrict__ o, int n_fft, int tid) {
    for (int i = tid; i < n_fft; i += 256) o[i] = idft_sample(d, tab, i, n_fft / 2 + 1, n_fft - 1) * window[i];
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Centred frames f = 0 .. len / hop of clip b, and its length: 0 frames where the length is not one the host admitted
// (never the case after check_clip_lengths; the guard keeps every index inside the row whatever the device array holds)
__device__ __forceinline__ int centred_clip_frames(const int* __restrict__ lengths, int b, int T, int min_len, int hop,
                                                   int& len) {
    len = lengths ? lengths[b] : T;
    return (len >= min_len && len <= T) ? len / hop + 1 : 0;
}

// Every frame of a clip of nf frames that covers padded position p, in ascending order, added to acc.
__device__ __forceinline__ float ola_gather_position(const float* __restrict__ wsb, int p, int n_fft, int hop, int nf,
                                                     float acc) {
    int lo = p - n_fft + 1;
    lo = lo <= 0 ? 0 : (lo + hop - 1) / hop;
    int hi = p / hop;
    if (hi > nf - 1) hi = nf - 1;
    for (int f = lo; f <= hi; ++f) acc += wsb[(size_t)f * n_fft + (p - f * hop)];
    return acc;
}

// The overlap-add of an adjoint's per-frame rows ws [B][f_max][n_fft] into dx [B][T] (ola_gather_kernel,
// spectral_kernels.hip); `lengths` may be null (every clip is T samples long).
int ola_gather(const float* ws, const int32_t* lengths, float* dx, int64_t B, int64_t T, int32_t n_fft, int32_t hop,
               int f_max, int32_t accumulate, hipStream_t stream);

static inline bool n_fft_ok(int32_t n_fft, int32_t max) { return n_fft >= 64 && n_fft <= max && (n_fft & (n_fft - 1)) == 0; }

// The ragged-batch contract of an entry point `who`: the device lengths and their host copy come together, and every
// clip (the whole row without lengths) has min_len .. T samples, min_len >= 1.  Returns the longest clip, or the
// (negative) DWS_ERR_* code with the message set.
static inline int64_t check_clip_lengths(const char* who, int64_t B, int64_t T, const int32_t* lengths,
                                         const int32_t* lengths_host, int64_t min_len) {
    DWS_CHECK((lengths == nullptr) == (lengths_host == nullptr), DWS_ERR_INVALID,
              "%s: lengths (device) and lengths_host (the same numbers on the host) come together", who);
    DWS_CHECK(lengths_host || T >= min_len, DWS_ERR_INVALID, "%s: T = %lld (needs at least %lld samples)", who, (long long)T,
              (long long)min_len);
    if (!lengths_host) return T;
    int64_t longest = 0;
    for (int64_t b = 0; b < B; ++b) {
        DWS_CHECK(lengths_host[b] >= min_len && lengths_host[b] <= T, DWS_ERR_INVALID,
                  "%s: clip %lld has %d samples (needs %lld .. T = %lld)", who, (long long)b, lengths_host[b],
                  (long long)min_len, (long long)T);
        if (lengths_host[b] > longest) longest = lengths_host[b];
    }
    return longest;
}

// ---- the inversion family (griffinlim_kernels, tvfilter_kernels): a frame kernel writes rows, a gather adds them up.
// LDS of a frame kernel: the table, the nb rows of the inverse stage and, where it transforms first, the frame.
constexpr size_t gl_lds_bytes(int n_fft, bool frame) { return (size_t)n_fft * 8 + (size_t)(n_fft / 2 + 1) * 8 + (frame ? (size_t)n_fft * 4 : 0); }

// The normalised overlap-add of the rows ws [B][f_max][n_fft] into x [B][T] (istft_gather_kernel, griffinlim_kernels.hip);
// y and alpha are Griffin-Lim's momentum pair (null and 0 elsewhere).
int gl_gather(const float* ws, const int32_t* lengths, const float* window, float* x, float* y, int64_t B, int64_t T,
              int32_t n_fft, int32_t hop, int f_max, float alpha, hipStream_t stream);

// Everything dws_istft, dws_griffin_lim and dws_tv_filter check alike; f_max frames make T = (f_max - 1) hop samples.
// `input` is the entry's first array under the name its message gives it.
static inline int gl_check(const char* who, const char* input_name, const float* input, int64_t B, int64_t f_max,
                           const int32_t* lengths, const int32_t* lengths_host, const float* window, int32_t n_fft,
                           int32_t hop, const float* out, const float* workspace) {
    DWS_CHECK(input, DWS_ERR_INVALID, "%s: null %s", who, input_name);
    DWS_CHECK(window, DWS_ERR_INVALID, "%s: null window", who);
    DWS_CHECK(out, DWS_ERR_INVALID, "%s: null out", who);
    DWS_CHECK(workspace, DWS_ERR_INVALID, "%s: null workspace (dws_griffin_lim_workspace bytes)", who);
    DWS_CHECK(n_fft_ok(n_fft, 4096), DWS_ERR_UNSUPPORTED, "%s: n_fft = %d (powers of two 64..4096 are built)", who, n_fft);
    DWS_CHECK(gl_lds_bytes(n_fft, true) <= 160 * 1024, DWS_ERR_UNSUPPORTED,
              "%s: n_fft = %d needs %zu bytes of LDS (160 KiB per workgroup)", who, n_fft, gl_lds_bytes(n_fft, true));
    DWS_CHECK(B > 0 && B <= 65535, DWS_ERR_INVALID, "%s: B = %lld (needs 1 .. 65535)", who, (long long)B);
    DWS_CHECK(hop > 0, DWS_ERR_INVALID, "%s: hop = %d (needs at least 1)", who, hop);
    DWS_CHECK(f_max >= 2 && (f_max - 1) <= (INT32_MAX - (int64_t)n_fft) / hop, DWS_ERR_INVALID,
              "%s: f_max = %lld (needs 2 frames at least, and (f_max - 1) hop + n_fft below 2^31)", who, (long long)f_max);
    const int64_t T = (f_max - 1) * hop;
    if (check_clip_lengths(who, B, T, lengths, lengths_host, n_fft / 2 + 1) < 0) return DWS_ERR_INVALID;
    for (int64_t b = 0; lengths_host && b < B; ++b)
        DWS_CHECK(lengths_host[b] % hop == 0, DWS_ERR_INVALID, "%s: lengths: clip %lld has %d samples, not a multiple of hop = %d",
                  who, (long long)b, lengths_host[b], hop);
    return DWS_OK;
}

}  // namespace dws
