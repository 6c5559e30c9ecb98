// Sample-rate conversion by a rational factor U / D (not in the reference): a polyphase FIR resampler with the filter
// table h[0 .. 2 half] (odd length, gain U) from the caller,
//   y[b][m] = sum_i x[b][i] h[m D - i U + half]        0 <= i < len_b, the tap index inside the table,
// for m < out_len_b = ceil(len_b U / D).  Nothing is zero-stuffed: an output takes about (2 half + 1) / U products.
//
// One workgroup per (tile of RESAMPLE_TILE output positions, clip).  The table and the input span the tile reads are staged
// in LDS; an output's sum runs over i ascending with fmaf from 0, there are no atomics: a clip's result is bitwise
// reproducible and depends on its own len_b samples alone (nothing behind len_b is read).
//
// LDS layout of the table: natural order.  With c = m D + half, output m reads h[c - i U] for i = ilo .. ihi, so at its
// t-th product lane m reads h[r_m + (q - t) U] with r_m = c mod U the output's phase: lanes of one phase share an address
// (a broadcast) and the others lie r_m apart inside one window of U dwords.  For U <= 32 (16000 <-> 10000, 2 -> 1) that
// is at most U neighbouring dwords: conflict-free.  For the 441-based ratios the phases (m D) mod U of neighbouring lanes
// step by D mod U and wrap about U, which is odd (441) or has an odd step (41 for 441 mod 200): the banks of a 32-lane
// group are spread.  A phase-major table [U][taps per phase] would put a lane's own taps side by side, which serves a
// lane's consecutive reads and does nothing for the lanes of a group at one t (rows r_m apart times the row length);
// it also needs a padded row per ratio.  It was not built, so there is no A/B.
#include "stft_core.h"      // check_clip_lengths

namespace dws {

constexpr int RESAMPLE_TILE = 1024;            // output positions per workgroup
constexpr int RESAMPLE_THREADS = 256;
constexpr int RESAMPLE_MAX_TAPS = 16384;
constexpr int RESAMPLE_MAX_SPAN = 16384;       // input samples of a tile in LDS

__device__ __forceinline__ int64_t resample_out_len(const int* __restrict__ lengths, int b, int T, int U, int D, int& len) {
    len = lengths ? lengths[b] : T;
    if (len < 1 || len > T) len = 0;           // a length the host did not admit: an empty clip
    return ((int64_t)len * U + D - 1) / D;
}

// grid (ceil(T_out / RESAMPLE_TILE), B); dynamic LDS: (2 half + 1) + span floats
__global__ __launch_bounds__(RESAMPLE_THREADS) void resample_kernel(const float* __restrict__ x, const int* __restrict__ lengths,
                                                                    const float* __restrict__ h, float* __restrict__ y, int T,
                                                                    int T_out, int U, int D, int half) {
    extern __shared__ float resample_lds[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t m0 = (int64_t)blockIdx.x * RESAMPLE_TILE;
    int len;
    const int64_t out_len = resample_out_len(lengths, b, T, U, D, len);
    float* yb = y + (size_t)b * T_out;
    if (m0 >= out_len) {                        // the whole workgroup, before any barrier: padding only
        for (int ml = tid; ml < RESAMPLE_TILE && m0 + ml < T_out; ml += RESAMPLE_THREADS) yb[m0 + ml] = 0.f;
        return;
    }
    const int ntap = 2 * half + 1;
    float* tab = resample_lds;                  // [ntap]
    float* xs = resample_lds + ntap;            // [span] x[i_first ..]
    const int64_t m_last = (m0 + RESAMPLE_TILE < out_len ? m0 + RESAMPLE_TILE : out_len) - 1;
    // i of the tile: m0 D + half - i U <= 2 half  and  m_last D + half - i U >= 0
    const int64_t a = m0 * D - half;
    const int64_t i_first = a <= 0 ? 0 : (a + U - 1) / U;
    int64_t i_last = (m_last * D + half) / U;
    if (i_last > len - 1) i_last = len - 1;
    const int span = (int)(i_last - i_first + 1);           // <= ((TILE - 1) D + 2 half) / U + 1 (the host sized LDS for it)
    const float* xb = x + (size_t)b * T;
    for (int i = tid; i < span; i += RESAMPLE_THREADS) xs[i] = xb[i_first + i];
    for (int i = tid; i < ntap; i += RESAMPLE_THREADS) tab[i] = h[i];
    __syncthreads();
    for (int ml = tid; ml < RESAMPLE_TILE && m0 + ml < T_out; ml += RESAMPLE_THREADS) {
        const int64_t m = m0 + ml;
        float acc = 0.f;
        if (m < out_len) {
            const int64_t c = m * D + half;
            const int64_t lo = c - 2 * (int64_t)half;
            const int64_t ilo = lo <= 0 ? 0 : (lo + U - 1) / U;
            int64_t ihi = c / U;
            if (ihi > len - 1) ihi = len - 1;
            int k = (int)(c - ilo * U);                     // in [0, 2 half] where the loop runs at all
            const float* xp = xs + (ilo - i_first);
            const int n = (int)(ihi - ilo + 1);
            for (int t = 0; t < n; ++t, k -= U) acc = fmaf(xp[t], tab[k], acc);
        }
        yb[m] = acc;
    }
}

// U == D == 1: the copy, bit for bit, whatever the table holds
__global__ __launch_bounds__(RESAMPLE_THREADS) void resample_copy_kernel(const float* __restrict__ x,
                                                                         const int* __restrict__ lengths,
                                                                         float* __restrict__ y, int T, int T_out) {
    const int b = blockIdx.y;
    int len;
    const int64_t out_len = resample_out_len(lengths, b, T, 1, 1, len);
    const int64_t m0 = (int64_t)blockIdx.x * RESAMPLE_TILE;
    for (int ml = threadIdx.x; ml < RESAMPLE_TILE && m0 + ml < T_out; ml += RESAMPLE_THREADS) {
        const int64_t m = m0 + ml;
        y[(size_t)b * T_out + m] = m < out_len ? x[(size_t)b * T + m] : 0.f;
    }
}

}  // namespace dws

extern "C" int dws_resample_tile(void) { return dws::RESAMPLE_TILE; }

extern "C" int dws_resample(const float* x, int64_t B, int64_t T, const int32_t* lengths, const int32_t* lengths_host,
                            const float* h, int32_t taps, int32_t U, int32_t D, float* y, int64_t T_out, void* stream) {
    using namespace dws;
    DWS_CHECK(x && h && y, DWS_ERR_INVALID, "dws_resample: null argument");
    DWS_CHECK(U >= 1 && D >= 1, DWS_ERR_INVALID, "dws_resample: ratio U / D = %d / %d (both at least 1)", U, D);
    DWS_CHECK(taps >= 1 && taps % 2 == 1, DWS_ERR_INVALID, "dws_resample: %d taps at ratio %d / %d (an odd count: h[0 .. 2 half])",
              taps, U, D);
    DWS_CHECK(B > 0 && B <= 65535, DWS_ERR_INVALID, "dws_resample: B = %lld (1 .. 65535)", (long long)B);
    DWS_CHECK(T > 0 && T <= INT32_MAX - 8192, DWS_ERR_INVALID, "dws_resample: T = %lld (1 .. 2^31 - 8193)", (long long)T);
    const int64_t longest = check_clip_lengths("dws_resample", B, T, lengths, lengths_host, 1);
    if (longest < 0) return DWS_ERR_INVALID;
    const int64_t need = (longest * U + D - 1) / D;
    DWS_CHECK(T_out >= need && T_out <= INT32_MAX - 8192, DWS_ERR_INVALID,
              "dws_resample: T_out = %lld at ratio %d / %d (the longest clip, %lld samples, gives %lld; below 2^31 - 8192)",
              (long long)T_out, U, D, (long long)longest, (long long)need);
    const dim3 grid((unsigned)ceil_div(T_out, RESAMPLE_TILE), (unsigned)B);
    if (U == 1 && D == 1) {
        hipLaunchKernelGGL(resample_copy_kernel, grid, dim3(RESAMPLE_THREADS), 0, (hipStream_t)stream, x, lengths, y, (int)T,
                           (int)T_out);
        DWS_HIP(hipGetLastError());
        return DWS_OK;
    }
    DWS_CHECK(taps <= RESAMPLE_MAX_TAPS, DWS_ERR_UNSUPPORTED,
              "dws_resample: ratio %d / %d comes with %d taps (the table in LDS holds at most %d)", U, D, taps, RESAMPLE_MAX_TAPS);
    const int64_t span = ((int64_t)(RESAMPLE_TILE - 1) * D + (taps - 1)) / U + 2;
    DWS_CHECK(span <= RESAMPLE_MAX_SPAN, DWS_ERR_UNSUPPORTED,
              "dws_resample: ratio %d / %d: a tile of %d outputs reads %lld input samples (at most %d fit in LDS)", U, D,
              RESAMPLE_TILE, (long long)span, RESAMPLE_MAX_SPAN);
    const size_t lds = (size_t)(taps + span) * sizeof(float);
    DWS_HIP(hipFuncSetAttribute((const void*)resample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(resample_kernel, grid, dim3(RESAMPLE_THREADS), lds, (hipStream_t)stream, x, lengths, h, y, (int)T,
                       (int)T_out, U, D, (taps - 1) / 2);
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}
