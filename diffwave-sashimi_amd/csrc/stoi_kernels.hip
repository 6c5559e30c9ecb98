// Short-time objective intelligibility of a generated batch x against a clean reference y (STOI: Taal, Hendriks, Heusdens
// & Jensen 2011; ESTOI: Jensen & Taal 2016; not in the reference).  Both signals are at the rate the band matrix was built
// for (10 kHz); the constants (frame, hop, n_fft, bands, segment, beta, dynamic range) are arguments.  Five launches:
//
//   stoi_energy_kernel    one wave per frame of y: e_j = 20 log10(||w y_j|| + eps), in double
//   stoi_compact_kernel   one workgroup per clip: max_j e_j, the keep flags e_j > max - range and the list of kept frames
//                         (a fixed-order prefix sum: thread t owns a contiguous run of frames, thread 0 adds the 256 counts)
//   stoi_band_kernel      one workgroup per kept frame k: frame k of the compacted (overlap-added) signals, never
//                         materialised -- the kept frames k' around k whose windows reach into it, added in double with k'
//                         ascending -- windowed again, a direct n_fft-point DFT of its `frame` samples in fp32 (one thread
//                         per bin, only bins some band uses), and the band magnitudes sqrt(obm . |.|^2) in double
//   stoi_segment_kernel   one workgroup per segment of N frames: the clipped correlation of every band (STOI) and the
//                         row- and column-normalised inner product (ESTOI), all in double
//   stoi_clip_sum_kernel  one thread per (clip, quantity): the segments in ascending order
//
// The host cannot know K (the kept frames), so the grids cover the largest frame count of the batch and a workgroup behind
// K (behind K - N + 1) leaves before its first barrier.  No atomics; bitwise reproducible; a clip's numbers depend on its own
// len_b samples alone.
#include <cfloat>

#include "stft_core.h"

namespace dws {

constexpr int STOI_Q = 4;
constexpr int STOI_MAX_BANDS = 64;
constexpr int STOI_MAX_SEGMENT = 128;

struct StoiWs {                 // the caller's workspace, cut up (F = the frame count of a clip of T samples)
    double* e;                  // [B][F]            frame energies of y in dB
    double* bands;              // [B][2][F][J]      band magnitudes of x (0) and y (1) per kept frame
    double* seg;                // [B][F][2]         (STOI sum over bands, ESTOI) per segment
    int* idx;                   // [B][F]            kept frames in order
    int* kept;                  // [B]               K
};

static inline int64_t stoi_frames(int64_t T, int32_t frame, int32_t hop) { return (T - frame) / hop + 1; }

static inline StoiWs stoi_cut(void* workspace, int64_t B, int64_t F, int J) {
    StoiWs w;
    w.e = static_cast<double*>(workspace);
    w.bands = w.e + B * F;
    w.seg = w.bands + B * 2 * F * J;
    w.idx = reinterpret_cast<int*>(w.seg + B * F * 2);
    w.kept = w.idx + B * F;
    return w;
}

// frames of clip b: 0 where the length is not one the host admitted
__device__ __forceinline__ int stoi_clip_frames(const int* __restrict__ lengths, int b, int T, int frame, int hop) {
    const int len = lengths ? lengths[b] : T;
    return (len >= frame && len <= T) ? (len - frame) / hop + 1 : 0;
}

// grid (ceil(F / 4), B), 256 threads: wave w of workgroup g takes frame 4 g + w
__global__ __launch_bounds__(256) void stoi_energy_kernel(const float* __restrict__ y, const int* __restrict__ lengths,
                                                          const float* __restrict__ window, double* __restrict__ e, int T,
                                                          int frame, int hop, int F) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= stoi_clip_frames(lengths, b, T, frame, hop)) return;        // a whole wave; there is no barrier
    const float* s = y + (size_t)b * T + (size_t)j * hop;
    double acc = 0.0;
    for (int n = lane; n < frame; n += 64) {
        const double v = (double)window[n] * (double)s[n];
        acc = fma(v, v, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) e[(size_t)b * F + j] = 20.0 * log10(sqrt(acc) + DBL_EPSILON);
}

// grid (B), 256 threads
__global__ __launch_bounds__(256) void stoi_compact_kernel(const double* __restrict__ e, const int* __restrict__ lengths,
                                                           int* __restrict__ idx, int* __restrict__ kept, int T, int frame,
                                                           int hop, int F, double range) {
    __shared__ double wmax[4];
    __shared__ int count[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nf = stoi_clip_frames(lengths, b, T, frame, hop);
    const double* eb = e + (size_t)b * F;
    const int C = (nf + 255) / 256;
    const int j0 = tid * C < nf ? tid * C : nf, j1 = j0 + C < nf ? j0 + C : nf;
    double mx = -1.0e300;
    for (int j = j0; j < j1; ++j) mx = eb[j] > mx ? eb[j] : mx;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(mx, off);
        mx = o > mx ? o : mx;
    }
    if ((tid & 63) == 0) wmax[tid >> 6] = mx;
    __syncthreads();
    mx = wmax[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) mx = wmax[w] > mx ? wmax[w] : mx;
    const double thr = mx - range;
    int n = 0;
    for (int j = j0; j < j1; ++j) n += eb[j] > thr ? 1 : 0;
    count[tid] = n;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) {
            const int c = count[t];
            count[t] = run;
            run += c;
        }
        kept[b] = run;
    }
    __syncthreads();
    int* ib = idx + (size_t)b * F + count[tid];
    for (int j = j0; j < j1; ++j)
        if (eb[j] > thr) *ib++ = j;
}

// grid (F, B), 256 threads; dynamic LDS: n_fft + frame + n_fft/2 + 1 float2
__global__ __launch_bounds__(256) void stoi_band_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                        const float* __restrict__ window, const float* __restrict__ obm,
                                                        const int* __restrict__ idx, const int* __restrict__ kept,
                                                        double* __restrict__ bands, int T, int frame, int hop, int n_fft,
                                                        int J, int F) {
    extern __shared__ double stoi_lds64[];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int K = kept[b];
    if (k >= K) return;                                    // the whole workgroup, before any barrier
    const int nb = n_fft / 2 + 1;
    float2* tab = reinterpret_cast<float2*>(stoi_lds64);   // [n_fft] (cos, sin)(2 pi j / n_fft)
    float2* fr = tab + n_fft;                              // [frame] (x, y): frame k of the compacted signals, windowed
    float2* pw = fr + frame;                               // [nb]    (|X|^2, |Y|^2)
    const int* ib = idx + (size_t)b * F;
    const float* xa = x + (size_t)b * T;
    const float* ya = y + (size_t)b * T;
    const int reach = (frame - 1) / hop;                   // kept frames k - reach .. k + reach overlap frame k
    for (int n = tid; n < frame; n += 256) {
        double sx = 0.0, sy = 0.0;
        int k0 = k - reach, k1 = k + reach;
        if (k0 < 0) k0 = 0;
        if (k1 > K - 1) k1 = K - 1;
        for (int kk = k0; kk <= k1; ++kk) {                // k' ascending
            const int i = n + (k - kk) * hop;              // the sample of kept frame k' that lands on position n
            if (i < 0 || i >= frame) continue;
            const size_t p = (size_t)ib[kk] * hop + i;
            const double w = (double)window[i];
            sx = fma(w, (double)xa[p], sx);
            sy = fma(w, (double)ya[p], sy);
        }
        const double w = (double)window[n];
        fr[n] = make_float2((float)(w * sx), (float)(w * sy));
    }
    for (int i = tid; i < n_fft; i += 256) tab[i] = twiddle(i, n_fft);
    __syncthreads();
    for (int q = tid; q < nb; q += 256) {
        bool used = false;
        for (int j = 0; j < J; ++j) used = used || obm[(size_t)j * nb + q] != 0.f;
        float px = 0.f, py = 0.f;
        if (used) {
            float re[2], im[2];
            dft_bin<2>(fr, tab, q, frame, n_fft - 1, re, im);      // `frame` samples against the n_fft-point table
            // written out: `re re + im im` leaves the contraction (which product is rounded on its own) to the compiler
            px = fmaf(re[0], re[0], im[0] * im[0]);
            py = fmaf(re[1], re[1], im[1] * im[1]);
        }
        pw[q] = make_float2(px, py);
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int j = wave; j < J; j += 4) {
        const float* row = obm + (size_t)j * nb;
        double sx = 0.0, sy = 0.0;
        for (int q = lane; q < nb; q += 64) {
            const double w = (double)row[q];
            sx = fma(w, (double)pw[q].x, sx);
            sy = fma(w, (double)pw[q].y, sy);
        }
        sx = wave_sum(sx);
        sy = wave_sum(sy);
        if (lane == 0) {
            bands[(((size_t)b * 2 + 0) * F + k) * J + j] = sqrt(sx);
            bands[(((size_t)b * 2 + 1) * F + k) * J + j] = sqrt(sy);
        }
    }
}

// grid (F, B), 128 threads; dynamic LDS: 2 N J + N doubles
__global__ __launch_bounds__(128) void stoi_segment_kernel(const double* __restrict__ bands, const int* __restrict__ kept,
                                                           double* __restrict__ seg, int N, int J, int F, double clip) {
    extern __shared__ double stoi_lds64[];
    const int m = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (m > kept[b] - N) return;                           // the whole workgroup, before any barrier
    double* xs = stoi_lds64;                               // [N][J]
    double* ys = xs + N * J;                               // [N][J]
    double* col = ys + N * J;                              // [max(N, J)]
    const double* bx = bands + (((size_t)b * 2 + 0) * F + m) * J;
    const double* by = bands + (((size_t)b * 2 + 1) * F + m) * J;
    for (int i = tid; i < N * J; i += 128) {               // N consecutive frames are N J consecutive doubles
        xs[i] = bx[i];
        ys[i] = by[i];
    }
    __syncthreads();
    const double eps = DBL_EPSILON, inv = 1.0 / (double)N;
    if (tid < J) {                                         // band tid, its N frames in ascending order
        const int j = tid;
        double sxx = 0.0, syy = 0.0, mx0 = 0.0, my = 0.0;
        for (int n = 0; n < N; ++n) {
            const double xv = xs[n * J + j], yv = ys[n * J + j];
            sxx = fma(xv, xv, sxx);
            syy = fma(yv, yv, syy);
            mx0 += xv;
            my += yv;
        }
        // STOI: normalise x to y's energy, clip at (1 + 10^(-beta / 20)) y, correlate the mean-removed rows
        const double alpha = sqrt(syy) / (sqrt(sxx) + eps);
        double mc = 0.0;
        for (int n = 0; n < N; ++n) {
            const double a = alpha * xs[n * J + j], c = clip * ys[n * J + j];
            mc += a < c ? a : c;
        }
        mc *= inv;
        my *= inv;
        mx0 *= inv;
        double cc = 0.0, yy = 0.0, cy = 0.0, xx = 0.0;
        for (int n = 0; n < N; ++n) {
            const double xv = xs[n * J + j], yv = ys[n * J + j] - my;
            const double a = alpha * xv, c = clip * ys[n * J + j];
            const double cv = (a < c ? a : c) - mc;
            const double xz = xv - mx0;
            cc = fma(cv, cv, cc);
            yy = fma(yv, yv, yy);
            xx = fma(xz, xz, xx);
        }
        const double nc = sqrt(cc) + eps, ny = sqrt(yy) + eps, nx = sqrt(xx) + eps;
        for (int n = 0; n < N; ++n) {
            const double xv = xs[n * J + j], yv = (ys[n * J + j] - my) / ny;
            const double a = alpha * xv, c = clip * ys[n * J + j];
            const double cv = ((a < c ? a : c) - mc) / nc;
            cy = fma(cv, yv, cy);
            // ESTOI: the rows zero-mean and unit-norm over time, in place
            xs[n * J + j] = (xv - mx0) / nx;
            ys[n * J + j] = yv;
        }
        col[j] = cy;
    }
    __syncthreads();
    double stoi = 0.0;
    if (tid == 0)
        for (int j = 0; j < J; ++j) stoi += col[j];        // bands in ascending order
    __syncthreads();
    if (tid < N) {                                         // frame tid, its J bands in ascending order
        const int n = tid;
        double mx = 0.0, my = 0.0;
        for (int j = 0; j < J; ++j) {
            mx += xs[n * J + j];
            my += ys[n * J + j];
        }
        mx /= (double)J;
        my /= (double)J;
        double xx = 0.0, yy = 0.0;
        for (int j = 0; j < J; ++j) {
            const double xv = xs[n * J + j] - mx, yv = ys[n * J + j] - my;
            xx = fma(xv, xv, xx);
            yy = fma(yv, yv, yy);
        }
        const double nx = sqrt(xx) + eps, ny = sqrt(yy) + eps;
        double d = 0.0;
        for (int j = 0; j < J; ++j) d = fma((xs[n * J + j] - mx) / nx, (ys[n * J + j] - my) / ny, d);
        col[n] = d;
    }
    __syncthreads();
    if (tid == 0) {
        double d = 0.0;
        for (int n = 0; n < N; ++n) d += col[n];           // frames in ascending order
        double* o = seg + ((size_t)b * F + m) * 2;
        o[0] = stoi;
        o[1] = d * inv;
    }
}

// One thread per (clip, quantity): the clip's segments in ascending order.
__global__ __launch_bounds__(64) void stoi_clip_sum_kernel(const double* __restrict__ seg, const int* __restrict__ kept,
                                                           double* __restrict__ out, int N, int F) {
    const int b = blockIdx.x, q = threadIdx.x;
    if (q >= STOI_Q) return;
    const int K = kept[b], M = K >= N ? K - N + 1 : 0;
    double s = 0.0;
    if (q < 2) {
        const double* p = seg + (size_t)b * F * 2 + q;
        for (int m = 0; m < M; ++m) s += p[2 * m];
    } else {
        s = q == 2 ? (double)M : (double)K;
    }
    out[(size_t)b * STOI_Q + q] = s;
}

static bool stoi_shape_ok(int64_t B, int64_t T, int32_t frame, int32_t hop, int32_t n_bands) {
    return B >= 1 && B <= 65535 && frame >= 1 && hop >= 1 && T >= frame && T <= INT32_MAX - 8192 && n_bands >= 1 &&
           n_bands <= STOI_MAX_BANDS;
}

}  // namespace dws

extern "C" int64_t dws_stoi_workspace(int64_t B, int64_t T, int32_t frame, int32_t hop, int32_t n_bands) {
    if (!dws::stoi_shape_ok(B, T, frame, hop, n_bands)) return 0;
    const int64_t F = dws::stoi_frames(T, frame, hop);
    return B * F * (int64_t)(8 * (1 + 2 * n_bands + 2) + 4) + ((B * 4 + 7) & ~(int64_t)7);
}

extern "C" int dws_stoi(const float* x, const float* y, int64_t B, int64_t T, const int32_t* lengths,
                        const int32_t* lengths_host, const float* window, int32_t frame, int32_t hop, int32_t n_fft,
                        const float* obm, int32_t n_bands, int32_t segment, double beta, double dyn_range, void* workspace,
                        double* out, void* stream) {
    using namespace dws;
    DWS_CHECK(x && y && window && obm && out, DWS_ERR_INVALID, "dws_stoi: null argument");
    DWS_CHECK(workspace, DWS_ERR_INVALID, "dws_stoi: null workspace (dws_stoi_workspace bytes)");
    DWS_CHECK(n_fft_ok(n_fft, 2048), DWS_ERR_INVALID, "dws_stoi: n_fft = %d (powers of two 64..2048)", n_fft);
    DWS_CHECK(frame >= 1 && frame <= n_fft, DWS_ERR_INVALID, "dws_stoi: frame = %d (1 .. n_fft = %d)", frame, n_fft);
    DWS_CHECK(hop >= 1, DWS_ERR_INVALID, "dws_stoi: hop = %d (at least 1)", hop);
    DWS_CHECK(segment >= 2 && segment <= STOI_MAX_SEGMENT, DWS_ERR_INVALID, "dws_stoi: segment = %d frames (2 .. %d)", segment,
              STOI_MAX_SEGMENT);
    DWS_CHECK(n_bands >= 1 && n_bands <= STOI_MAX_BANDS, DWS_ERR_INVALID, "dws_stoi: n_bands = %d (1 .. %d)", n_bands,
              STOI_MAX_BANDS);
    DWS_CHECK(B > 0 && B <= 65535 && T > 0 && T <= INT32_MAX - 8192, DWS_ERR_INVALID,
              "dws_stoi: bad shape (B = %lld, T = %lld)", (long long)B, (long long)T);
    DWS_CHECK(dyn_range > 0.0 && dyn_range < 1e6 && beta > -1e3 && beta < 1e3, DWS_ERR_INVALID,
              "dws_stoi: beta = %g dB, dynamic range = %g dB", beta, dyn_range);
    const int64_t longest = check_clip_lengths("dws_stoi", B, T, lengths, lengths_host, frame);      // one frame at least
    if (longest < 0) return DWS_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int64_t F = stoi_frames(T, frame, hop);          // the workspace's rows
    const int64_t Fb = stoi_frames(longest, frame, hop);   // the most frames a clip of this batch can keep
    const StoiWs w = stoi_cut(workspace, B, F, n_bands);
    hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)ceil_div(Fb, 4), (unsigned)B), dim3(256), 0, s, y, lengths, window,
                       w.e, (int)T, frame, hop, (int)F);
    DWS_HIP(hipGetLastError());
    hipLaunchKernelGGL(stoi_compact_kernel, dim3((unsigned)B), dim3(256), 0, s, w.e, lengths, w.idx, w.kept, (int)T, frame, hop,
                       (int)F, dyn_range);
    DWS_HIP(hipGetLastError());
    const size_t lds_band = (size_t)(n_fft + frame + n_fft / 2 + 1) * sizeof(float2);
    static_assert((2048 + 2048 + 1025) * 8 <= 64 * 1024, "the largest band frame fits the default dynamic LDS limit");
    hipLaunchKernelGGL(stoi_band_kernel, dim3((unsigned)Fb, (unsigned)B), dim3(256), lds_band, s, x, y, window, obm, w.idx,
                       w.kept, w.bands, (int)T, frame, hop, n_fft, n_bands, (int)F);
    DWS_HIP(hipGetLastError());
    const double clip = 1.0 + pow(10.0, -beta / 20.0);
    if (Fb >= segment) {
        const int big = segment > n_bands ? segment : n_bands;
        const size_t lds_seg = (size_t)(2 * segment * n_bands + big) * sizeof(double);
        DWS_HIP(hipFuncSetAttribute((const void*)stoi_segment_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_seg));
        hipLaunchKernelGGL(stoi_segment_kernel, dim3((unsigned)(Fb - segment + 1), (unsigned)B), dim3(128), lds_seg, s, w.bands,
                           w.kept, w.seg, segment, n_bands, (int)F, clip);
        DWS_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(stoi_clip_sum_kernel, dim3((unsigned)B), dim3(64), 0, s, w.seg, w.kept, out, segment, (int)F);
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}
