// Pitch tracks of waveforms and the pitch distances between two batches of them: YIN (de Cheveigne & Kawahara, 2002)
// with a fixed threshold, one workgroup per (frame, clip, signal), and the eight per-clip sums of the pitch metrics
// (F0 RMSE in Hz and cents, gross pitch errors, voicing decision error and F1, periodicity RMSE).
//
// Framing is stft_core.h's: frames f = 0 .. len_b / hop, centred, reflected about the clip's OWN ends (a
// ragged batch: nothing behind len_b is read).  A frame is S = W + M samples (W the integration window, M = tau_hi + 1
// the largest lag computed) in LDS, and
//   d(tau) = sum_{j < W} (u[j] - u[j + tau])^2        tau = 0 .. M
// is the hot loop, in fp32, as the direct sum of squares of exact differences (never as energy - 2 autocorrelation: d
// is a near-zero minimum exactly where it matters, and that form cancels there).
//
// Register tile: a work item owns the four lags 4g .. 4g + 3 and a contiguous run of 4-sample blocks of j.  Per block
// it reads three aligned 16-byte words, u[j .. j+3] (one address per wave: a broadcast) and u[j+4g .. j+4g+7] (lane
// stride 16 bytes: conflict-free), for sixteen difference-squares -- 3/16 LDS words per term where one lag per thread
// reads 2.  With G = ceil((M + 1) / 4) lag groups the W range is cut into P = max(1, 256 / G) parts, so G P <= 256 work
// items where G <= 256 and G items in two or three passes of the workgroup above that.
//
// Order of summation of d(tau): a work item adds its j in ascending order (fmaf of the exact difference), then the P
// parts are added in ascending order (fp32).  Everything after it is double: a fixed-shape prefix sum over tau (thread t
// owns C = ceil(M / 256) consecutive lags serially; an inclusive shuffle scan over the lanes of a wave; the waves in
// wave order), d'(tau) = d(tau) tau / prefix(tau), and the decision as three min reductions (first tau below the
// threshold, first tau at which the descent stops, smallest d' of the search range).  No atomics; bitwise reproducible.
#include "stft_core.h"

namespace dws {

constexpr int PITCH_Q = 8;
typedef float pitch_v4 __attribute__((ext_vector_type(4)));     // a native vector: its LDS loads stay 16-byte loads
// zeros behind the frame: with 4 nblk <= W and 4 G <= M + 4 the block loop reads up to u[4 (nblk - 1) + 4 (G - 1) + 7]
// <= u[S + 3] and the tail up to u[W - 1 + 4 (G - 1) + 3] <= u[S + 2]; what they feed are lags above M, which nobody reads
constexpr int PITCH_PAD = 16;

// the shortest clip a frame of S samples can be reflected about (one reflection per side)
__host__ __device__ __forceinline__ int pitch_min_len(int S) { return (S + 1) / 2 + 1; }

__device__ __forceinline__ int pitch_block_min(int v, int* slot, int wave, int lane) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    __syncthreads();                      // the slots' previous readers
    if (lane == 0) slot[wave] = v;
    __syncthreads();
    int r = slot[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) r = slot[w] < r ? slot[w] : r;
    return r;
}

// grid (f_max, B, signals): signal z is s0 (z = 0) or s1, its track goes to track + z B f_max 2.
__global__ __launch_bounds__(256) void pitch_frame_kernel(const float* __restrict__ s0, const float* __restrict__ s1,
                                                          const int* __restrict__ lengths, float* __restrict__ track, int T,
                                                          int hop, int W, int tau_lo, int tau_hi, double theta, double sr,
                                                          int f_max) {
    extern __shared__ pitch_v4 lds128[];
    const int f = blockIdx.x, b = blockIdx.y, z = blockIdx.z, tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int M = tau_hi + 1, S = W + M;
    float* o = track + (((size_t)z * gridDim.y + b) * f_max + f) * 2;
    int len;
    if (f >= centred_clip_frames(lengths, b, T, pitch_min_len(S), hop, len)) {      // the whole workgroup, before any barrier
        if (tid < 2) o[tid] = 0.f;
        return;
    }
    const int G = (M + 4) / 4;                             // groups of four lags covering 0 .. M
    const int P = G >= 256 ? 1 : 256 / G;                  // parts of the W range
    const int S_pad = (S + PITCH_PAD + 3) & ~3;
    float* u = reinterpret_cast<float*>(lds128);           // [S_pad] the frame, zeros behind S (16-byte aligned rows)
    float* part = u + S_pad;                               // [P][4 G] partial sums
    double* d = reinterpret_cast<double*>(part + P * 4 * G);   // [4 G]   d, then d'
    double* wtot = d + 4 * G;                              // [4]     wave totals of the scan
    double* dslot = wtot + 4;                              // [4]
    int* islot = reinterpret_cast<int*>(dslot + 4);        // [4]
    const float* sa = (z ? s1 : s0) + (size_t)b * T;
    const int start = f * hop - S / 2;
    for (int i = tid; i < S_pad; i += 256) {
        u[i] = i < S ? sa[reflect_index(start + i, len)] : 0.f;      // len >= pitch_min_len(S) keeps the index in [0, len)
    }
    __syncthreads();

    // ---- d(tau), fp32
    const pitch_v4* u4 = lds128;
    const int nblk = W >> 2;                               // whole 4-sample blocks of j; the rest is the last part's tail
    const int chunk = (nblk + P - 1) / P;
    for (int item = tid; item < G * P; item += 256) {
        const int g = item % G, p = item / G;
        int jb0 = p * chunk, jb1 = jb0 + chunk;
        if (jb1 > nblk) jb1 = nblk;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int jb = jb0; jb < jb1; ++jb) {
            const pitch_v4 x = u4[jb];
            const pitch_v4 l = u4[jb + g];
            const pitch_v4 h = u4[jb + g + 1];
            float t;
            t = x.x - l.x; a0 = fmaf(t, t, a0);
            t = x.x - l.y; a1 = fmaf(t, t, a1);
            t = x.x - l.z; a2 = fmaf(t, t, a2);
            t = x.x - l.w; a3 = fmaf(t, t, a3);
            t = x.y - l.y; a0 = fmaf(t, t, a0);
            t = x.y - l.z; a1 = fmaf(t, t, a1);
            t = x.y - l.w; a2 = fmaf(t, t, a2);
            t = x.y - h.x; a3 = fmaf(t, t, a3);
            t = x.z - l.z; a0 = fmaf(t, t, a0);
            t = x.z - l.w; a1 = fmaf(t, t, a1);
            t = x.z - h.x; a2 = fmaf(t, t, a2);
            t = x.z - h.y; a3 = fmaf(t, t, a3);
            t = x.w - l.w; a0 = fmaf(t, t, a0);
            t = x.w - h.x; a1 = fmaf(t, t, a1);
            t = x.w - h.y; a2 = fmaf(t, t, a2);
            t = x.w - h.z; a3 = fmaf(t, t, a3);
        }
        if (p == P - 1) {
            for (int j = nblk * 4; j < W; ++j) {           // W is no multiple of 4: at most three samples
                const float x = u[j];
                const float* q = u + j + 4 * g;            // (j + 4 g + 3 <= W - 1 + M + 3 < S_pad)
                float t;
                t = x - q[0]; a0 = fmaf(t, t, a0);
                t = x - q[1]; a1 = fmaf(t, t, a1);
                t = x - q[2]; a2 = fmaf(t, t, a2);
                t = x - q[3]; a3 = fmaf(t, t, a3);
            }
        }
        reinterpret_cast<pitch_v4*>(part)[p * G + g] = pitch_v4{a0, a1, a2, a3};
    }
    __syncthreads();
    for (int tau = tid; tau < 4 * G; tau += 256) {
        float s = part[tau];
        for (int p = 1; p < P; ++p) s += part[p * 4 * G + tau];
        d[tau] = tau == 0 ? 0.0 : (double)s;
    }                                                      // (d[0] stays d(0) = 0: d'(0) = 1 is never read, tau_lo >= 2)
    __syncthreads();

    // ---- prefix sum over tau = 1 .. M and d', double, in a fixed shape
    const int C = (M + 255) / 256;
    const int t0 = 1 + tid * C;
    int t1 = t0 + C;
    if (t1 > M + 1) t1 = M + 1;
    double own = 0.0;
    for (int tau = t0; tau < t1; ++tau) own += d[tau];
    double incl = own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    double run = 0.0;
    for (int w = 0; w < wave; ++w) run += wtot[w];
    run += incl - own;                                     // the sum of every lag before t0
    for (int tau = t0; tau < t1; ++tau) {
        const double v = d[tau];
        run += v;
        d[tau] = run == 0.0 ? 1.0 : v * (double)tau / run;
    }
    __syncthreads();

    // ---- decision
    int first = INT32_MAX;
    double vmin = 1.0e300;
    for (int tau = tau_lo + tid; tau <= tau_hi; tau += 256) {
        const double v = d[tau];
        if (v < theta && tau < first) first = tau;
        if (v < vmin) vmin = v;
    }
    first = pitch_block_min(first, islot, wave, lane);
    float f0 = 0.f, per;
    if (first == INT32_MAX) {                              // unvoiced (the same value in every thread)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double v = __shfl_xor(vmin, off);
            vmin = v < vmin ? v : vmin;
        }
        if (lane == 0) dslot[wave] = vmin;
        __syncthreads();
        if (tid != 0) return;
        double m = dslot[0];
        for (int w = 1; w < 4; ++w) m = dslot[w] < m ? dslot[w] : m;
        const double p = 1.0 - m;
        per = (float)(p < 0.0 ? 0.0 : (p > 1.0 ? 1.0 : p));
    } else {
        int stop = INT32_MAX;                              // first tau >= first at which the descent stops
        for (int tau = first + tid; tau <= tau_hi; tau += 256) {
            if (tau + 1 > tau_hi || !(d[tau + 1] < d[tau])) {
                stop = tau;
                break;
            }
        }
        stop = pitch_block_min(stop, islot, wave, lane);
        if (tid != 0) return;
        const double a = d[stop - 1], bb = d[stop], c = d[stop + 1];
        const double den = a - 2.0 * bb + c;
        double delta = 0.0;
        if (den > 0.0) {
            delta = 0.5 * (a - c) / den;
            if (!(fabs(delta) <= 1.0)) delta = 0.0;
        }
        f0 = (float)(sr / ((double)stop + delta));
        const double p = 1.0 - bb;
        per = (float)(p < 0.0 ? 0.0 : (p > 1.0 ? 1.0 : p));
    }
    o[0] = f0;
    o[1] = per;
}

// One thread per (clip, quantity): the clip's frames in ascending order, in double, from the two tracks.
__global__ __launch_bounds__(64) void pitch_clip_sum_kernel(const float* __restrict__ tx, const float* __restrict__ ty,
                                                            const int* __restrict__ lengths, double* __restrict__ out, int T,
                                                            int S, int hop, int f_max) {
    const int b = blockIdx.x, q = threadIdx.x;
    if (q >= PITCH_Q) return;
    int len;
    const int nf = centred_clip_frames(lengths, b, T, pitch_min_len(S), hop, len);
    const float2* px = reinterpret_cast<const float2*>(tx) + (size_t)b * f_max;
    const float2* py = reinterpret_cast<const float2*>(ty) + (size_t)b * f_max;
    double s = 0.0;
    for (int f = 0; f < nf; ++f) {
        const float2 x = px[f], y = py[f];
        const bool vx = x.x > 0.f, vy = y.x > 0.f;
        const double fx = (double)x.x, fy = (double)y.x;
        double t = 0.0;
        switch (q) {
            case 0: t = (vx && vy) ? 1.0 : 0.0; break;
            case 1: if (vx && vy) { const double e = fx - fy; t = e * e; } break;
            case 2: if (vx && vy) { const double e = 1200.0 * log2(fx / fy); t = e * e; } break;
            case 3: t = vy ? 1.0 : 0.0; break;
            case 4: t = vx ? 1.0 : 0.0; break;
            case 5: t = (vx != vy) ? 1.0 : 0.0; break;
            case 6: { const double e = (double)x.y - (double)y.y; t = e * e; } break;
            default: t = (vx && vy && fabs(fx / fy - 1.0) > 0.2) ? 1.0 : 0.0; break;
        }
        s += t;
    }
    out[(size_t)b * PITCH_Q + q] = s;
}

static int pitch_check(const char* who, int64_t B, int64_t T, const int32_t* lengths, const int32_t* lengths_host, int32_t hop,
                       int32_t win, int32_t tau_lo, int32_t tau_hi, float threshold, double sampling_rate) {
    DWS_CHECK(win >= 64 && win <= 2048, DWS_ERR_INVALID, "%s: win = %d (64 .. 2048)", who, win);
    DWS_CHECK(tau_lo >= 2 && tau_lo < tau_hi && tau_hi <= 2047, DWS_ERR_INVALID,
              "%s: tau_lo = %d, tau_hi = %d (2 <= tau_lo < tau_hi, tau_hi + 1 <= 2048)", who, tau_lo, tau_hi);
    DWS_CHECK(threshold > 0.f && threshold < 1.f, DWS_ERR_INVALID, "%s: threshold = %g (inside (0, 1))", who, (double)threshold);
    DWS_CHECK(sampling_rate > 0.0 && sampling_rate < 1e12, DWS_ERR_INVALID, "%s: sampling_rate = %g", who, sampling_rate);
    DWS_CHECK(B > 0 && B <= 65535 && hop > 0 && T > 0 && T <= INT32_MAX - 8192, DWS_ERR_INVALID,
              "%s: bad shape (B = %lld, T = %lld, hop = %d)", who, (long long)B, (long long)T, hop);
    return check_clip_lengths(who, B, T, lengths, lengths_host, pitch_min_len(win + tau_hi + 1)) < 0 ? DWS_ERR_INVALID : DWS_OK;
}

static int pitch_launch(const float* s0, const float* s1, int signals, int64_t B, int64_t T, const int32_t* lengths,
                        int32_t hop, int32_t win, int32_t tau_lo, int32_t tau_hi, float threshold, double sampling_rate,
                        float* track, hipStream_t stream) {
    const int f_max = (int)(T / hop) + 1;
    const int M = tau_hi + 1, S = win + M, G = (M + 4) / 4, P = G >= 256 ? 1 : 256 / G;
    const int S_pad = (S + PITCH_PAD + 3) & ~3;
    const size_t lds = (size_t)(S_pad + P * 4 * G) * 4 + (size_t)(4 * G + 10) * 8;
    static_assert((4096 + PITCH_PAD + 4 * 513) * 4 + (4 * 513 + 10) * 8 <= 64 * 1024,
                  "the largest shape (W = M = 2048) fits the default dynamic LDS limit: no attribute call per launch");
    hipLaunchKernelGGL(pitch_frame_kernel, dim3((unsigned)f_max, (unsigned)B, (unsigned)signals), dim3(256), lds, stream, s0,
                       s1, lengths, track, (int)T, hop, win, tau_lo, tau_hi, (double)threshold, sampling_rate, f_max);
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}

}  // namespace dws

extern "C" int dws_pitch_track(const float* s, int64_t B, int64_t T, const int32_t* lengths, const int32_t* lengths_host,
                               int32_t hop, int32_t win, int32_t tau_lo, int32_t tau_hi, float threshold,
                               double sampling_rate, float* track, void* stream) {
    using namespace dws;
    DWS_CHECK(s && track, DWS_ERR_INVALID, "dws_pitch_track: null argument");
    DWS_TRY(pitch_check("dws_pitch_track", B, T, lengths, lengths_host, hop, win, tau_lo, tau_hi, threshold, sampling_rate));
    return pitch_launch(s, s, 1, B, T, lengths, hop, win, tau_lo, tau_hi, threshold, sampling_rate, track,
                        (hipStream_t)stream);
}

extern "C" int64_t dws_pitch_distance_workspace(int64_t B, int64_t T, int32_t hop) {
    if (B < 1 || T < 1 || hop < 1 || T > INT32_MAX - 8192 || B > 65535) return 0;
    return 2 * B * (T / hop + 1) * 2 * (int64_t)sizeof(float);
}

extern "C" int dws_pitch_distance(const float* x, const float* y, int64_t B, int64_t T, const int32_t* lengths,
                                  const int32_t* lengths_host, int32_t hop, int32_t win, int32_t tau_lo, int32_t tau_hi,
                                  float threshold, double sampling_rate, float* workspace, double* out, void* stream) {
    using namespace dws;
    DWS_CHECK(x && y && out, DWS_ERR_INVALID, "dws_pitch_distance: null argument");
    DWS_CHECK(workspace, DWS_ERR_INVALID, "dws_pitch_distance: null workspace (dws_pitch_distance_workspace bytes)");
    DWS_TRY(pitch_check("dws_pitch_distance", B, T, lengths, lengths_host, hop, win, tau_lo, tau_hi, threshold,
                        sampling_rate));
    DWS_TRY(pitch_launch(x, y, 2, B, T, lengths, hop, win, tau_lo, tau_hi, threshold, sampling_rate, workspace,
                         (hipStream_t)stream));
    const int f_max = (int)(T / hop) + 1;
    hipLaunchKernelGGL(pitch_clip_sum_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, workspace,
                       workspace + (size_t)B * f_max * 2, lengths, out, (int)T, win + tau_hi + 1, hop, f_max);
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}
