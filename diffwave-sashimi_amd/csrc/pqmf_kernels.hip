// Pseudo-QMF filter bank of multi-band runs (Multi-band MelGAN, Yang et al. 2020; not in the reference): the analysis
// bank splits a waveform [B][T] into K critically sampled sub-bands [B][K][T/K], the synthesis bank puts it back.  Both
// take the filter table [K][taps + 1] and a gain from the caller, so each also serves as the other's adjoint (with the
// tap-reversed table; include/dws.h).
//
// One workgroup per (tile of PQMF_TILE full-band positions, clip).  The input span of the tile plus taps/2 positions of
// halo on each side (zero outside the clip) and the table are staged in LDS; a sum runs over n ascending (then k
// ascending in the synthesis bank) with fmaf, there are no atomics: a clip's result is bitwise reproducible and does not
// depend on B or on the clip's place in the batch.
//
// LDS layout.  Analysis output t reads x[K t + n - taps/2]: a lane stride of K dwords, a K-way bank conflict on a plain
// staged row (ds_read_b32 banks are dword mod 32 within a 32-lane half).  The span is therefore staged de-interleaved,
// sample i of the span at phase[i % K][i / K]: lane t reads phase[n % K][t + n / K], consecutive dwords across the
// lanes.  A phase row is PQMF_ROW<K> dwords with PQMF_ROW<K> % 32 == 32 / K, so the 32 consecutive samples that a half
// wave writes while staging (K rows, 32 / K dwords in each) fall on 32 different banks as well.  The synthesis bank reads
// s[k][(u + n - taps/2) / K]: K neighbouring lanes share an address (a broadcast), the others read consecutive dwords.
#include "dws_common.h"

namespace dws {

constexpr int PQMF_TILE = 1024;        // full-band positions per workgroup (pqmf.TILE in Python)
constexpr int PQMF_MAX_TAPS = 254;
constexpr int PQMF_THREADS = 256;

// dwords of one staged row: at least (PQMF_TILE + PQMF_MAX_TAPS) / K + 2, and == 32 / K (mod 32)
template <int K> struct PqmfRow;
template <> struct PqmfRow<2> { static constexpr int value = 656; };
template <> struct PqmfRow<4> { static constexpr int value = 328; };
static_assert(PqmfRow<2>::value >= (PQMF_TILE + PQMF_MAX_TAPS) / 2 + 2 && PqmfRow<2>::value % 32 == 16, "row of K = 2");
static_assert(PqmfRow<4>::value >= (PQMF_TILE + PQMF_MAX_TAPS) / 4 + 2 && PqmfRow<4>::value % 32 == 8, "row of K = 4");

template <int K>
__global__ __launch_bounds__(PQMF_THREADS) void pqmf_analysis_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ filt,
                                                                     float* __restrict__ out, int T, int taps, float gain) {
    constexpr int R = PqmfRow<K>::value;
    __shared__ float phase[K * R];
    __shared__ float table[K * (PQMF_MAX_TAPS + 1)];
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int half = taps / 2, ntap = taps + 1;
    const int start = tile * PQMF_TILE;                     // the tile's first full-band position
    const float* xb = x + (size_t)b * T;
    for (int i = tid; i < PQMF_TILE + taps; i += PQMF_THREADS) {
        const int p = start - half + i;
        phase[(i % K) * R + i / K] = (p >= 0 && p < T) ? xb[p] : 0.f;
    }
    for (int i = tid; i < K * ntap; i += PQMF_THREADS) table[i] = filt[i];
    __syncthreads();
    const int Ts = T / K, t0 = start / K;
    for (int tl = tid; tl < PQMF_TILE / K && t0 + tl < Ts; tl += PQMF_THREADS) {
        float acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0.f;
        for (int n = 0; n < ntap; ++n) {                    // one window, all K bands
            const float v = phase[(n % K) * R + tl + n / K];
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = fmaf(table[k * ntap + n], v, acc[k]);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) out[((size_t)b * K + k) * Ts + t0 + tl] = gain * acc[k];
    }
}

template <int K>
__global__ __launch_bounds__(PQMF_THREADS) void pqmf_synthesis_kernel(const float* __restrict__ s,
                                                                      const float* __restrict__ filt,
                                                                      float* __restrict__ out, int Ts, int taps, float gain) {
    constexpr int R = PqmfRow<K>::value;
    __shared__ float band[K * R];
    __shared__ float table[K * (PQMF_MAX_TAPS + 1)];
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int half = taps / 2, ntap = taps + 1;
    const int start = tile * PQMF_TILE;                     // the tile's first full-band (output) position
    const int a = start - half;
    const int q0 = a >= 0 ? a / K : -((-a + K - 1) / K);    // floor(a / K): the first sub-band position any output reads
    const int count = (PQMF_TILE + taps) / K + 2;           // <= R (static_assert above)
    for (int i = tid; i < K * count; i += PQMF_THREADS) {
        const int k = i / count, j = i - k * count, q = q0 + j;
        band[k * R + j] = (q >= 0 && q < Ts) ? s[((size_t)b * K + k) * Ts + q] : 0.f;
    }
    for (int i = tid; i < K * ntap; i += PQMF_THREADS) table[i] = filt[i];
    __syncthreads();
    const int T = Ts * K;
    for (int ul = tid; ul < PQMF_TILE && start + ul < T; ul += PQMF_THREADS) {
        const int u = start + ul;
        const int n0 = (((half - u) % K) + K) % K;          // the smallest n with u + n - half a multiple of K
        int j = (u + n0 - half) / K - q0;                   // exact division; 0 <= j, and j + (taps - n0) / K < count
        float acc = 0.f;
        for (int n = n0; n < ntap; n += K, ++j) {           // polyphase: every K-th tap, no zero-stuffing
#pragma unroll
            for (int k = 0; k < K; ++k) acc = fmaf(table[k * ntap + n], band[k * R + j], acc);
        }
        out[(size_t)b * T + u] = gain * acc;
    }
}

static int pqmf_check(const char* who, int64_t B, int64_t T, int32_t K, int32_t taps) {
    DWS_CHECK(K == 2 || K == 4, DWS_ERR_INVALID, "%s: K = %d (2 or 4)", who, K);
    DWS_CHECK(taps >= 2 && taps <= PQMF_MAX_TAPS && taps % 2 == 0, DWS_ERR_INVALID, "%s: taps = %d (even, 2 .. %d)", who, taps,
              PQMF_MAX_TAPS);
    DWS_CHECK(B > 0 && B <= 65535, DWS_ERR_INVALID, "%s: B = %lld (1 .. 65535)", who, (long long)B);
    DWS_CHECK(T > 0 && T % K == 0 && T <= INT32_MAX - 8192, DWS_ERR_INVALID,
              "%s: the full-band length %lld is not a positive multiple of K = %d (below 2^31 - 8192)", who, (long long)T, K);
    return DWS_OK;
}

}  // namespace dws

extern "C" int dws_pqmf_tile(void) { return dws::PQMF_TILE; }

extern "C" int dws_pqmf_analysis(const float* x, int64_t B, int64_t T, const float* filt, int32_t K, int32_t taps, float gain,
                                 float* out, void* stream) {
    using namespace dws;
    DWS_CHECK(x && filt && out, DWS_ERR_INVALID, "dws_pqmf_analysis: null argument");
    DWS_TRY(pqmf_check("dws_pqmf_analysis", B, T, K, taps));
    const dim3 grid((unsigned)ceil_div(T, PQMF_TILE), (unsigned)B);
    if (K == 2)
        hipLaunchKernelGGL(pqmf_analysis_kernel<2>, grid, dim3(PQMF_THREADS), 0, (hipStream_t)stream, x, filt, out, (int)T, taps,
                           gain);
    else
        hipLaunchKernelGGL(pqmf_analysis_kernel<4>, grid, dim3(PQMF_THREADS), 0, (hipStream_t)stream, x, filt, out, (int)T, taps,
                           gain);
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}

extern "C" int dws_pqmf_synthesis(const float* s, int64_t B, int64_t Ts, const float* filt, int32_t K, int32_t taps, float gain,
                                  float* out, void* stream) {
    using namespace dws;
    DWS_CHECK(s && filt && out, DWS_ERR_INVALID, "dws_pqmf_synthesis: null argument");
    DWS_CHECK(Ts >= 1 && Ts <= INT32_MAX / 4, DWS_ERR_INVALID, "dws_pqmf_synthesis: Ts = %lld (at least 1)", (long long)Ts);
    DWS_TRY(pqmf_check("dws_pqmf_synthesis", B, (K == 2 || K == 4) ? Ts * K : Ts, K, taps));
    const dim3 grid((unsigned)ceil_div(Ts * K, PQMF_TILE), (unsigned)B);
    if (K == 2)
        hipLaunchKernelGGL(pqmf_synthesis_kernel<2>, grid, dim3(PQMF_THREADS), 0, (hipStream_t)stream, s, filt, out, (int)Ts,
                           taps, gain);
    else
        hipLaunchKernelGGL(pqmf_synthesis_kernel<4>, grid, dim3(PQMF_THREADS), 0, (hipStream_t)stream, s, filt, out, (int)Ts,
                           taps, gain);
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}
