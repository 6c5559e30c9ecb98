// Fused WaveNet residual layer (`models/wavenet.py:82-121`) on the bf16 matrix cores at fp32-equivalent accuracy:
// the Winograd F(2,3) form of wavenet_wino.hip (four K = C products per position PAIR (p, p+d) instead of six) with
// every GEMM operand carried as a 3-term bf16 split and six of the nine partial products accumulated in fp32
// (bf16_split.h: what is dropped is below a quarter of an fp32 ulp of each product).  precision = "bf16x6".
//
// Per tile of 32 pairs (64 positions) and all channels, C/32 waves, a wave owns one (tanh, sigmoid) row-tile pair:
//   * raw x at the four shifts -d, 0, +d, +2d staged by LDS-DMA exactly as in wavenet_wino.hip (16-byte pieces,
//     out-of-range shifts read 0 = the conv's zero padding; one contiguous row piece for d <= 16), two chunks ahead.
//     Eight waves under the 3-term split: a chunk is staged by one half of the workgroup, alternating (waves 0..3 | 4..7 =
//     one wave of every SIMD), so that the other wave of a SIMD has no LDS-DMA piece queued in front of its A fragments;
//     every other instance: all waves stage every chunk;
//   * transform pass, all waves together once per chunk of KC channels: t0..t3 (fp32, the same roundings as the
//     f32 Winograd path), each split into three bf16 terms and stored in the B-fragment order of
//     v_mfma_f32_32x32x16_bf16: 16-byte items [k-octet][product][term][column], one conflict-free ds_read_b128 per
//     fragment.  The pass is branch-free and cut into seven units that stand between the MFMAs of the previous chunk's
//     first step (the one wave's copy of its residual rows is a branch of its own ahead of the second step);
//   * GEMM1: m_j = G_j t_j for the wave's two row tiles; the A fragments of G0..G3 (three bf16 terms each, packed at
//     commit: 6 bytes per weight) stream from L2 one (k-block, product) step ahead, the B fragments from LDS one step
//     ahead inside a chunk; 12 MFMAs per step;
//     step embedding + conv bias enter as one extra k-block per product (A = the fp32 correction row of the f32
//     Winograd path split in registers, B = the Winograd transform of the in-range indicator: exact in bf16; the 16x16x32
//     shape below: as the accumulators' fp32 start values instead);
//   * gate in registers, split, -> LDS gate tile [k-octet][term][64 columns]; the EXTRA instance adds the mel term and, in
//     training (precision = "bf16x6"), saves the pre-activations H [B, 2C, L] for the gate adjoint as wavenet_wino.hip does;
//   * GEMM2 [res; skip] = [Wr; Ws] g with the biases as an extra k-block; the last layer leaves the res row tile out;
//   * epilogue: each wave transposes its row tiles through a private 8 KB LDS slot and moves them as row-major
//     16-byte accesses: x' = (x + res) sqrt(.5) with x re-read (L2-hot: this tile staged it), skip += as load-add-store
//     (one workgroup owns an element per layer, layers are stream-ordered).  The x / skip tiles are requested before
//     the gate stage.  Clips whose rows are not 16-byte aligned take a per-lane dword path.
//
// MFMA shape (template parameter MF; set_option("bx6_mfma") / DWS_BX6_MFMA; SplitBf16x3 at C = S = 256 only -- every other instance
// has the 32x32x16 body above and nothing else).  "16x16x32", the default there: both GEMMs, the gate stage and the epilogue on
// v_mfma_f32_16x16x32_bf16.  No operand is laid out differently: the packed weights, the transformed chunks, the gate tile and the
// transpose slots keep their bytes, a fragment is the same 16-byte items under the lane map (row / column lane & 15, k-octet
// lane >> 4 of a 32-channel block), the transform pass, the staging, the residual copy and every wait count are shared.  A 32 x 32
// tile is four 16 x 16 slices (row half h, column half c) of four registers, row = 16 h + 4 (lane >> 4) + reg, col = 16 c + (lane & 15).
// GEMM1 runs a chunk in eight half-steps (product, row tile) of 24 MFMAs, GEMM2 a 32-channel block in two.  The correction k-blocks
// are not MFMAs on this shape (K = 32 would spend 96 + 48 of them per tile on two non-zero k entries): every accumulator register
// STARTS at the block's value as a rank-1 fp32 expression, one rounding -- GEMM1: correction row x indicator transform (+ conv bias in
// product 1), formed under the first staging wait from 16-byte loads of four consecutive rows; GEMM2: the bias itself (bit-equal to
// the block) (profiles/r09_ab_bx6_accumulator_start.txt, tests/test_bx6_accumulator_start_gpu.py).  The summation order per
// output element is kept (start value, chunks in rotated order, products in P::ia / ib order), but one instruction sums 32
// channels where two summed 16 + 16: results differ in the last bits (tests/test_bx6_mfma_shape_gpu.py), deterministically and
// independently of the clip's place in the batch.  The shape costs cycles (+ 4.9 % tile span) and wins wall time (- 1.8 % of the step):
// the chip is power-capped under this kernel and holds 1970 instead of 1838 MHz on it (profiles/r08_ab_bx6_mfma_shape.txt).
// "gemm2-16x16x32": GEMM2 and the epilogue only (measured: a third of the gain).  "32x32x16": the code as it was, instruction for instruction.
//
// A ring of the 16x16x32 GEMM1 (template parameter AR; set_option("bx6_a_ring") / DWS_BX6_A_RING; no other instance has the parameter's
// second value).  "quarter-step", the default: a half-step runs as its two row halves (disjoint fragments, disjoint accumulators), 12 MFMAs
// on two alternating accumulators each, and the 48 fragment registers are a ring of four sets of three, each requested three quarter-steps =
// 36 MFMAs ahead of its use where "half-step" (the code as it was, instruction for instruction) requests six fragments one half-step = 24
// MFMAs ahead.  Same fragments, L2 bytes, MFMAs and registers; every accumulator keeps its order of summation, so the bits are equal
// (tests/test_bx6_a_ring_gpu.py).  A wave that runs a stretch of a chunk alone goes at the pace of its A-fragment round trips: chunk period
// 8.8 k -> 8.3 k cycles, tile span - 3.0 %, - 1.2 % of the step (profiles/r10_ab_bx6_a_ring.txt, r10_bx6_a_ring_trace.txt).
//
// Work per launch at C = S = 256, B = 16, L = 16000: 204.5 GFLOP of fp32-equivalent GEMM (the f32 Winograd kernel's
// executed flops) = 1.227 PFLOP of bf16 MFMA = 0.49 ms at 2.5 PFLOP/s, against 1.30 ms at the fp32 matrix rate.
#include <cstdlib>
#include <type_traits>

#include "bf16_split.h"
#include "wavenet.h"
#include "wn_trace.h"

namespace dws {

#ifndef BX6_PF3
#define BX6_PF3 1   // A-fragment prefetch distance in (k-block, product) steps: 3-term split (12 MFMAs per step)
#endif
#ifndef BX6_PF2
#define BX6_PF2 2   // 2-term split (6 MFMAs per step)
#endif
#define BX6_PF(NT) ((NT) == 2 ? BX6_PF2 : BX6_PF3)
#ifndef BX6_T_SLOTS
#define BX6_T_SLOTS 0, 2, 3, 4, 6, 7, 9   // the 3-term split's placement of the transform units in a chunk's first step (do_step)
#endif

typedef float bx6_f32x4 __attribute__((ext_vector_type(4)));

// The activation streams (x in, x' out, running skip in / out: each element touched once per launch, 1 GB in all) carry the
// nontemporal policy so that they do not push the weight fragments -- 3.75 MB that every tile re-reads -- out of the
// 4 MB L2 of an XCD.
#ifdef BX6_ABL_NO_NT
#define BX6_NT 0
#else
#define BX6_NT 2
#endif
__device__ __forceinline__ bx6_f32x4 bx6_load_f4(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(bx6_f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, BX6_NT));
}
__device__ __forceinline__ void bx6_store_f4(bx6_f32x4 v, __amdgpu_buffer_rsrc_t r, int voff, int soff) {
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), r, voff, soff, BX6_NT);
}

__device__ __forceinline__ float bx6_gate(float t, float s) {   // tanh(t) * sigmoid(s), see fast_gate (wavenet_kernels.hip)
    const float tc = __builtin_amdgcn_fmed3f(t, -30.f, 30.f);
    const float e2 = __builtin_amdgcn_exp2f(tc * 2.8853900817779268f);
    const float en = __builtin_amdgcn_exp2f(s * -1.4426950408889634f);
    return (e2 - 1.f) * __builtin_amdgcn_rcpf((e2 + 1.f) * (1.f + en));
}

// ---- weight packing (commit time) ----------------------------------------------------------------------------------
// Folded dilated-conv weight [2C][C][3] -> Winograd matrices G0..G3 (the f32 path's formulas and roundings,
// wavenet_wino.hip: wino_dconv_kernel) -> the split's NT terms in A-fragment order:
//   out[((((mt * NKB + kb) * 4 + j) * NT + term) * 64 + lane) * 8 + e] = term of G_j[mt*32 + (lane & 31)][kb*16 + 8*(lane >> 5) + e]
// Scaled splits (fp16 terms) multiply by *scale first: a power of two chosen per matrix by weight_scale_kernel.
template <typename P>
__global__ void pack_a1_bx6_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, int C, const float* __restrict__ scale) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)2 * C * C * 4) return;
    const int e = (int)(i & 7), lane = (int)((i >> 3) & 63), j = (int)((i >> 9) & 3);
    const size_t r = i >> 11;                     // mt * NKB + kb
    const int nkb = C / 16;
    const int kb = (int)(r % nkb), mt = (int)(r / nkb);
    const int o = mt * 32 + (lane & 31), c = kb * 16 + 8 * (lane >> 5) + e;
    const float* wr = w + ((size_t)o * C + c) * 3;
    const float w0 = wr[0], w1 = wr[1], w2 = wr[2];
    float g;
    if (j == 0) g = w0;
    else if (j == 1) g = 0.5f * ((w0 + w2) + w1);
    else if (j == 2) g = 0.5f * ((w0 + w2) - w1);
    else g = w2;
    if (P::SCALED) g *= *scale;
    unsigned short b[P::NT];
    P::bits(g, b);
    const size_t base = ((r * 4 + j) * P::NT) * 512 + (size_t)lane * 8 + e;
#pragma unroll
    for (int t = 0; t < P::NT; ++t) out[base + t * 512] = b[t];
}

// Row-major fp32 W[M][K] -> out[(((mt * NKB + kb) * NT + term) * 64 + lane) * 8 + e]
template <typename P>
__global__ void pack_a_bx6_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, int M, int K, const float* __restrict__ scale) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)M * K) return;
    const int e = (int)(i & 7), lane = (int)((i >> 3) & 63);
    const size_t r = i >> 9;
    const int nkb = K / 16;
    const int kb = (int)(r % nkb), mt = (int)(r / nkb);
    float v = w[(size_t)(mt * 32 + (lane & 31)) * K + kb * 16 + 8 * (lane >> 5) + e];
    if (P::SCALED) v *= *scale;
    unsigned short b[P::NT];
    P::bits(v, b);
    const size_t base = (r * P::NT) * 512 + (size_t)lane * 8 + e;
#pragma unroll
    for (int t = 0; t < P::NT; ++t) out[base + t * 512] = b[t];
}

// *out = the power of two that brings m = max(max|w|, max|bias| / 1024) into [1, 2)  (one workgroup; commit time).  The
// Winograd combinations G1, G2 of three taps then stay below 3, every fp16 high term is normal down to 2^-14 and the low terms
// resolve 2^-25 absolute = 2^-26 of the matrix maximum or better.  The bias rows ride in the same accumulators (correction
// k-block), so they enter the maximum far enough down that a bias 1000 x the weights neither overflows fp16 (< 2^11 scaled)
// nor costs the weights precision in the usual case.
__global__ __launch_bounds__(1024) void weight_scale_kernel(const float* __restrict__ w, size_t n, const float* __restrict__ bias, int nb,
                                                            const float* __restrict__ bias_b, int nb_b, float* __restrict__ out) {
    __shared__ float red[16];
    float m = 0.f;
    for (size_t i = threadIdx.x; i < n; i += 1024) m = fmaxf(m, fabsf(w[i]));
    if (bias)
        for (int i = threadIdx.x; i < nb; i += 1024) m = fmaxf(m, fabsf(bias[i]) * (1.f / 1024.f));
    if (bias_b)
        for (int i = threadIdx.x; i < nb_b; i += 1024) m = fmaxf(m, fabsf(bias_b[i]) * (1.f / 1024.f));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i) m = fmaxf(m, red[i]);
        int ex = 0;
        if (m > 0.f && m < 3.0e38f) {
            frexpf(m, &ex);                         // m = f * 2^ex, f in [0.5, 1)  ->  m * 2^(1 - ex) in [1, 2)
            if (ex > 100) ex = 100;
            if (ex < -100) ex = -100;
        }
        *out = ldexpf(1.f, 1 - ex);
    }
}

int launch_weight_scale(const float* w, size_t n, const float* bias, int nb, const float* bias_b, int nb_b, float* out, hipStream_t s) {
    hipLaunchKernelGGL(weight_scale_kernel, dim3(1), dim3(1024), 0, s, w, n, bias, nb, bias_b, nb_b, out);
    return DWS_OK;
}

int launch_pack_a1_bx6(const float* w, void* out, int C, int split, const float* scale, hipStream_t s) {
    const size_t n = (size_t)2 * C * C * 4;
    if (split == WN_SPLIT_F16X3) {
        DWS_CHECK(scale != nullptr, DWS_ERR_INVALID, "pack_a1: the fp16 split needs the matrix scale");
        hipLaunchKernelGGL(pack_a1_bx6_kernel<SplitF16x2>, dim3(ceil_div(n, 256)), dim3(256), 0, s, w, (unsigned short*)out, C, scale);
    } else {
        hipLaunchKernelGGL(pack_a1_bx6_kernel<SplitBf16x3>, dim3(ceil_div(n, 256)), dim3(256), 0, s, w, (unsigned short*)out, C, scale);
    }
    return DWS_OK;
}

int launch_pack_a_bx6(const float* w, void* out, int M, int K, int split, const float* scale, hipStream_t s) {
    DWS_CHECK(M % 32 == 0 && K % 16 == 0, DWS_ERR_UNSUPPORTED, "pack_a_bx6: M=%d K=%d", M, K);
    const size_t n = (size_t)M * K;
    if (split == WN_SPLIT_F16X3) {
        DWS_CHECK(scale != nullptr, DWS_ERR_INVALID, "pack_a: the fp16 split needs the matrix scale");
        hipLaunchKernelGGL(pack_a_bx6_kernel<SplitF16x2>, dim3(ceil_div(n, 256)), dim3(256), 0, s, w, (unsigned short*)out, M, K, scale);
    } else {
        hipLaunchKernelGGL(pack_a_bx6_kernel<SplitBf16x3>, dim3(ceil_div(n, 256)), dim3(256), 0, s, w, (unsigned short*)out, M, K, scale);
    }
    return DWS_OK;
}

// ---- the layer kernel ----------------------------------------------------------------------------------------------
template <int C, int S, int NT>
struct Bx6Tile {
    static constexpr int WAVES = C / 32;          // one (tanh, sigmoid) tile pair per wave
    static constexpr int NTH = WAVES * 64;
    static constexpr int NP = 32;                 // position pairs per workgroup (64 positions)
    static constexpr int KC = (C >= 256) ? 32 : 16;   // channels per staged chunk (between two workgroup barriers)
    static constexpr int NCB = C / KC;
    static constexpr int NKB = C / 16;            // k-blocks of 16 channels
    static constexpr int MS = S / C;              // skip tiles per wave
    static constexpr int RAW_FLOATS = KC * 4 * NP;          // one raw chunk: [row][shift][32] (or [row][128] contiguous)
    static constexpr int BOP_BYTES = (KC / 8) * 4 * NT * NP * 16;   // one transformed chunk: [octet][product][term][column] items
    static constexpr int STAGE_FLOATS = 2 * RAW_FLOATS + 2 * BOP_BYTES / 4;
    static constexpr int GATE_BYTES = (C / 8) * NT * 64 * 16;       // gate tile: [octet][term][column] items
    static constexpr int MAIN_FLOATS = STAGE_FLOATS > GATE_BYTES / 4 ? STAGE_FLOATS : GATE_BYTES / 4;
    static constexpr int TR_FLOATS = 32 * 64;     // a wave's transpose slot: one row tile x 64 columns
    static constexpr int LDS_FLOATS = MAIN_FLOATS + WAVES * TR_FLOATS;
    static constexpr int TITEMS = (KC / 4) * NP * 2;        // transform items: (4-channel group, column, product pair)
    // 3-term split only: the 2-term instance at C = 256 holds three A-fragment sets in flight and sits at 253 registers, the
    // asymmetric form's second loop body would push it into scratch
    static constexpr bool HALVES = WAVES == 8 && NT == 3;   // raw chunks staged by alternating halves of the workgroup (see the kernel)
    static constexpr int SW = HALVES ? WAVES / 2 : WAVES;   // waves that stage one chunk, a pair of adjacent rows per piece
    static constexpr int NPIECE = KC / (2 * SW);
    static_assert(C % 32 == 0 && S % C == 0 && C % KC == 0 && KC % 16 == 0 && KC % (2 * SW) == 0 && (SW & (SW - 1)) == 0 &&
                  (!HALVES || NCB % 2 == 0) && (TITEMS % NTH == 0) && LDS_FLOATS * 4 <= 163840, "channel counts");
};

// MF: the MFMA shape.  BX6_MF_32: v_mfma_f32_32x32x16 in both GEMMs (every instance has it);  BX6_MF_G2_16: GEMM2 and the
// epilogue on v_mfma_f32_16x16x32;  (SplitBf16x3, C = S = 256 only: the headline instances).
//   BX6_MF_16: GEMM1 and the gate stage on it as well.
enum { BX6_MF_32 = 0, BX6_MF_G2_16 = 1, BX6_MF_16 = 2 };
#ifndef BX6_T16_SLOTS
#define BX6_T16_SLOTS 1, 5, 7, 9, 13, 15, 19   // 16x16x32 GEMM1: the MFMA (of 24) of a chunk's first half-step behind which each transform unit stands
#endif
// AR: the ring of GEMM1's A fragments on the 16x16x32 shape (set_option("bx6_a_ring") / DWS_BX6_A_RING; nothing in any other instance).
//   BX6_AR_HALF: two sets of six fragments (row halves h = 0, 1 x three terms), requested one half-step = 24 MFMAs ahead;
//   BX6_AR_QUARTER: the same 48 registers as four sets of three (one row half), requested BX6_A_LEAD quarter-steps of 12 MFMAs ahead.
enum { BX6_AR_HALF = 0, BX6_AR_QUARTER = 1 };
#ifndef BX6_A_LEAD
#define BX6_A_LEAD 3   // quarter-step ring: lead of an A-fragment request over its first use, in quarter-steps (1..3: the set of quarter q + 4 is still in use)
#endif
struct Bx6Nothing {};
// state of the 16x16x32 GEMM2 (nothing at all in a 32x32x16 instance, so that those compile to the code they had)
template <int MS>
struct Bx6G2State {
    bx_f32x4 bias[1 + MS][2];           // the biases in accumulator layout: rows 16 h + 4 (lane >> 4) + (0..3) of each row tile
    bx_f32x4 acc[1 + MS][2][2][2];      // [row tile][column tile n][row half h][column half c]
};
// the six A fragments of a GEMM1 half-step (row tile, product): [row half h][term], soff = the byte offset of term 0 of the
// first of the block's two k-blocks
template <int NT>
__device__ __forceinline__ int bx6_voff_a1h(int lane) { return ((lane >> 5) * (4 * NT * 64) + ((lane >> 4) & 1) * 32 + (lane & 15)) * 16; }
template <typename V8, int NT>
__device__ __forceinline__ void bx6_load_a1h(V8 (&dst)[2][NT], __amdgpu_buffer_rsrc_t r, int voff, int soff) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int t = 0; t < NT; ++t) dst[h][t] = __builtin_bit_cast(V8, __builtin_amdgcn_raw_buffer_load_b128(r, voff + h * 256, soff + t * 1024, 0));
}
// the three A fragments of a GEMM1 quarter-step (row tile, product, row half h): [term], voff = bx6_voff_a1h + h * 256
template <typename V8, int NT>
__device__ __forceinline__ void bx6_load_a1q(V8 (&dst)[NT], __amdgpu_buffer_rsrc_t r, int voff, int soff) {
#pragma unroll
    for (int t = 0; t < NT; ++t) dst[t] = __builtin_bit_cast(V8, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff + t * 1024, 0));
}
// state of the 16x16x32 GEMM1
template <typename V8, int NT>
struct Bx6G1State {
    // correction rows in accumulator layout, rows 16 h + 4 (lane >> 4) + (0..3) of the two row tiles: [m][h][product], conv bias
    // [m][h].  Dead once the start values are formed (ahead of the first chunk barrier).
    bx_f32x4 av[2][2][4], ab[2][2];
    bx_f32x4 acc[2][4][2][2];           // [row tile m][product j][row half h][column half c]
    // A fragments.  BX6_AR_HALF: ring over the half-steps, [half-step & 1][h][term].  BX6_AR_QUARTER: the same registers as a ring
    // of four sets over the quarter-steps, set s = quarter & 3 is [s >> 1][s & 1][term].
    V8 ar[2][2][NT];
};
template <typename P, int C, int S, bool EXTRA, int MF = BX6_MF_32, int AR = BX6_AR_HALF>
__global__ __launch_bounds__(C * 2, (C >= 128 ? 2 : 1)) void wn_layer_bx6_kernel(WnLayerArgs a, int log2d) {
    using T = Bx6Tile<C, S, P::NT>;
    static_assert(MF == BX6_MF_32 || (P::NT == 3 && !P::SCALED && C == 256 && S == 256), "the 16x16x32 shape: bf16 split, C = S = 256");
    static_assert(AR == BX6_AR_HALF || MF >= BX6_MF_16, "the quarter-step A ring belongs to the 16x16x32 GEMM1");
    static_assert(BX6_A_LEAD >= 1 && BX6_A_LEAD <= 3, "quarter-step ring of four sets: a lead of four would request into the set in use");
    using v8 = typename P::v8;
    using v4 = typename P::v4;
    constexpr int NT = P::NT, NPR = P::NP, NA = 2 * P::NT;   // terms, products per term pair, A fragments per GEMM1 step
    constexpr int KC = T::KC, MS = T::MS, WAVES = T::WAVES, NCB = T::NCB, NTH = T::NTH, NKB = T::NKB;
    __shared__ __attribute__((aligned(16))) float lds[T::LDS_FLOATS];
    float* const Xraw = lds;                                            // 2 raw chunks (LDS-DMA target)
    char* const Bop = reinterpret_cast<char*>(lds + 2 * T::RAW_FLOATS); // 2 transformed chunks (B operands)
    char* const gt = reinterpret_cast<char*>(lds);                      // gate tile (aliases the staging buffers)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lhi = lane >> 5;
    const int L = a.L, dil = 1 << log2d;
    float* const trw = lds + T::MAIN_FLOATS + wave * T::TR_FLOATS;

    const int nblk = (L + 2 * dil - 1) >> (log2d + 1);     // blocks of 2d
    const int ntl = ((nblk << log2d) + 31) >> 5;           // tiles of 32 pairs per batch element
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int b = __builtin_amdgcn_readfirstlane(tile / ntl);
    // Order of the tiles inside a clip.  A tile reads its own 2 x 32 positions AND two halos of 32 (shifts -d and +2d): the
    // second half of the previous block of 2d and the first half of the next one -- the main columns of the tiles d/32 tile
    // numbers away.  d >= 64: the BLOCK index runs fastest (tile t -> block t % nblk, 32-pair slice t / nblk), so that the tiles
    // that share columns are neighbours in launch order = run at the same time on CUs of one XCD and meet in its L2 (4 MB:
    // one round of 32 tiles already moves 6 MB through it); linear order left every x element to be fetched twice.
    const int tic = tile % ntl;                             // tile number inside the clip
#ifdef WN_TILE_ORDER_LINEAR
    const int q0 = __builtin_amdgcn_readfirstlane(tic * 32);
#else
    const int q0 = __builtin_amdgcn_readfirstlane(log2d >= 6 ? ((tic % nblk) << log2d) + (tic / nblk) * 32 : tic * 32);
#endif
    const int q = q0 + l31;                                // first-half position number of this lane's column
    const int p = ((q >> log2d) << (log2d + 1)) + (q & (dil - 1));

    const float* __restrict__ xb = a.x_in + (size_t)b * C * L;
    unsigned long long* __restrict__ trc = a.trace ? a.trace + ((size_t)blockIdx.x * WAVES + wave) * 32 : nullptr;
    auto stamp = [&](int i) {
        if (trc) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            if (lane == 0) trc[i] = t;
        }
    };
    stamp(0);

    // ---- operands of the correction k-blocks, fetched first (their latency hides behind the first staging wait)
    const int mt1[2] = {wave, C / 32 + wave};
    int mt2[1 + MS];
    mt2[0] = wave;
#pragma unroll
    for (int m = 0; m < MS; ++m) mt2[1 + m] = C / 32 + wave * MS + m;
    [[maybe_unused]] std::conditional_t<MF >= BX6_MF_16, Bx6G1State<v8, NT>, Bx6Nothing> gs1;
    if constexpr (MF >= BX6_MF_16) {
        // 16x16x32: the correction rows are the accumulators' start values (below), so they are fetched in accumulator layout,
        // four consecutive rows per 16-byte load.  Every row block starts a multiple of four floats into Abt / bias1, and the
        // launcher checks that both bases and both Abt strides keep 16 bytes (per-clip rows and step-table rows alike).
        const float* Abt = a.Abt + (size_t)b * a.abt_bstride + step_row_off(a.step_idx, a.abt_tstride);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int row = (m ? C / 32 + wave : wave) * 32 + 16 * h + 4 * (lane >> 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) gs1.av[m][h][j] = *reinterpret_cast<const bx_f32x4*>(Abt + j * 2 * C + row);
                gs1.ab[m][h] = *reinterpret_cast<const bx_f32x4*>(a.bias1 + row);
            }
    }
    float av1[2][4], ab1[2], av2[1 + MS];
    if constexpr (MF < BX6_MF_16) {
        const float* Abt = a.Abt + (size_t)b * a.abt_bstride + step_row_off(a.step_idx, a.abt_tstride);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int row = mt1[m] * 32 + l31;
#pragma unroll
            for (int j = 0; j < 4; ++j) av1[m][j] = Abt[j * 2 * C + row];
            ab1[m] = a.bias1[row];
        }
#pragma unroll
        for (int m = 0; m < 1 + MS; ++m) av2[m] = a.bias2[mt2[m] * 32 + l31];
    }
    // scaled splits (fp16 terms): this layer's two weight matrices were packed times a power of two each (wscale[0], [1]);
    // inv1 / inv2 undo weight x operand scale on the fp32 accumulators
    const float ws1 = P::SCALED ? a.wscale[0] : 1.f, ws2 = P::SCALED ? a.wscale[1] : 1.f;
    const float inv1 = 1.f / (ws1 * P::SX), inv2 = 1.f / (ws2 * P::SG);

    // ---- staging of raw x (wavenet_wino.hip: same three forms).  16-byte accesses need every row 16-byte aligned.
    const bool al16 = (L % 4 == 0) && ((((size_t)a.x_in | (size_t)a.x_out | (size_t)a.skip) & 15) == 0);
    const bool contig = al16 && log2d <= 4;
    const bool x4 = contig || (al16 && log2d >= 2);
    __amdgpu_buffer_rsrc_t rXall = __builtin_amdgcn_make_buffer_rsrc((void*)xb, 0, C * L * 4, 0x00020000);
    const int pbase = (q0 >> log2d) << (log2d + 1);          // first position of the tile's block (d < 32: a multiple of 64)
    const int ob = contig ? 32 + (p - pbase) - dil : l31;    // shift s of this lane's column sits at ob + s * os in a staged row
    const int os = contig ? dil : 32;
    // columns of the [res; skip] GEMM: tile n = 0 the first halves, n = 1 the partners (d >= 32: two runs of 32
    // consecutive positions); contiguous staging (d <= 16): positions [pbase, pbase+32) and [pbase+32, pbase+64), the
    // gate tile is written in that order
    const int x0l = p - pbase, x1l = x0l + dil;
    const int gcol0 = contig ? x0l : l31, gcol1 = contig ? x1l : 32 + l31;
    int voffA, voffB;
    if (contig) {
        const int pp = pbase - 32 + 4 * (lane & 31);
        voffA = ((unsigned)pp < (unsigned)L) ? (lhi * L + pp) * 4 : 0x7ffffff0;
        voffB = 0;
    } else if (x4) {
        const int s4 = (lane >> 3) & 3, qq = q0 + 4 * (lane & 7);
        const int pp = ((qq >> log2d) << (log2d + 1)) + (qq & (dil - 1)) + (s4 - 1) * dil;
        voffA = ((unsigned)pp < (unsigned)L) ? (lhi * L + pp) * 4 : 0x7ffffff0;
        voffB = 0;
    } else {
        voffA = (p + (lhi - 1) * dil) * 4;
        voffB = (p + (lhi + 1) * dil) * 4;
    }
    // The K loop visits the channel chunks in an order ROTATED by the tile number: workgroups that run in lockstep on the
    // CUs of an XCD then ask the L2 for different parts of the weight matrices at any moment (every tile streams all of
    // A1 / A2, 3.75 MB at C = 256; worth 3 k of 77 k GEMM1 cycles.  The stream is NOT what bounds GEMM1: with the fragments
    // served from L1 (BX6_ABL_A_HOT) GEMM1 moves by 2-3 %, profiles/r05_split_layer_ablations.txt)
#ifdef BX6_ABL_NO_ROT
    const int rot = 0;
#else
    // Keyed by the tile's number INSIDE its clip (consecutive workgroups of an XCD run consecutive tiles: xcd_remap), never by
    // the batch index: the summation order of a position must not depend on where its clip sits in the batch
    // (tests/test_full_size_gpu.py: equal clips give equal bits, a clip alone == the clip inside a batch of 16).
    const int rot = __builtin_amdgcn_readfirstlane((int)((unsigned)tic % NCB));
#endif
    auto chunk_of = [&](int cb) { const int c = cb + rot; return c >= NCB ? c - NCB : c; };
    // Who stages a chunk.  Eight waves (two per SIMD: waves w and w + 4 share one): chunk cbi is staged by ONE half of the
    // workgroup, waves 0..3 for even cbi and 4..7 for odd, twice the pieces each.  vmcnt retires in order, so the A fragments
    // a wave requests behind its LDS-DMA pieces (x: nontemporal, HBM latency) cannot be consumed before those have landed;
    // the partner wave on the same SIMD has no piece in front of its A stream in that chunk and keeps the matrix pipe busy
    // meanwhile.  With every wave staging, both waves of every SIMD stood in that wait at the same time.  Fewer waves
    // (C <= 128: one wave of a workgroup per SIMD, the neighbour is another workgroup at another point of its tile): all stage.
    constexpr bool HALVES = T::HALVES;
    constexpr int SW = T::SW;                      // waves that stage one chunk
    constexpr int NPIECE = T::NPIECE;              // staging requests (row pairs) per staging wave and chunk
    const int sw = HALVES ? (wave & (SW - 1)) : wave;
    const int shalf = HALVES ? wave / SW : 0;
    auto stages = [&](int cbi) { return !HALVES || (cbi & 1) == shalf; };
    auto stage_piece = [&](int cbi, int i) {
        float* xs = Xraw + (cbi & 1) * T::RAW_FLOATS;
        const int cb = chunk_of(cbi);
        {
            const int cc = 2 * (sw + SW * i);
            if (x4) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rXall, xs + cc * 128, 16, voffA, (cb * KC + cc) * L * 4, 0, BX6_NT);
            } else {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)(xb + (size_t)(cb * KC + cc + h) * L), 0, L * 4, 0x00020000);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, xs + (cc + h) * 128, 4, voffA, 0, 0, 0);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, xs + (cc + h) * 128 + 64, 4, voffB, 0, 0, 0);
                }
            }
        }
    };
    auto stage_dma = [&](int cbi) {
#pragma unroll
        for (int i = 0; i < NPIECE; ++i) stage_piece(cbi, i);
    };

    // ---- transform pass: raw chunk c1 -> t_j = Winograd input transform, three bf16 terms each, in B-fragment order.
    // Item = (column, group of 4 channels, product pair): 12 LDS reads, 8 transforms, 8 splits, six 8-byte writes.
    // No branch in it: the product pair jp of an item is wave-uniform, and a branch on it would cut the pass into basic
    // blocks of its own in front of the MFMAs.  Pair 0 needs shifts (0, 1, 2), pair 1 shifts (1, 2, 3): the third read
    // takes a selected address and the two forms differ by selects of the operands (d1 - d3 == d1 + (-d3) bit for bit).
    // The pass is cut into T_UNITS units that the chunk loop deals out between the MFMAs of a step (do_step), per half
    // h = 0, 1 of the item's four channels:  R_h: the six LDS reads of the half, issued together;  A_h, B_h: t_a, t_b of
    // the half, split;  and last W: the LDS writes.  Order R0 A0 B0 R1 A1 B1 W: six raw values are live at a time.
    constexpr int TK = T::TITEMS / NTH, T_UNITS = 7;
    struct TState {
        float d[TK][2][3];
        v4 pa[TK][NT], pb[TK][NT];
    };
    auto transform_unit = [&](int c1, int u, TState& ts) __attribute__((always_inline)) {
        const float* xs = Xraw + (c1 & 1) * T::RAW_FLOATS;
        char* bo = Bop + (c1 & 1) * T::BOP_BYTES;
#pragma unroll
        for (int k = 0; k < TK; ++k) {
            const int i = tid + NTH * k;
            const int gi = __builtin_amdgcn_readfirstlane(i >> 6);      // wave-uniform part of the item number
            const int g4 = (gi * 2 + lhi) % (KC / 4);
            const int jp = __builtin_amdgcn_readfirstlane((gi * 2) / (KC / 4));   // KC/4 even: both halves of a wave share jp
            const bool p1 = jp != 0;
            const int h = u / 3, w = u % 3;          // half of the item, (R, A, B)
            if (u == T_UNITS - 1) {
                char* dst = bo + ((((g4 >> 1) * 4 + 2 * jp) * NT) * 32 + l31) * 16 + (g4 & 1) * 8;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    *reinterpret_cast<v4*>(dst + t * 512) = ts.pa[k][t];
                    *reinterpret_cast<v4*>(dst + (NT + t) * 512) = ts.pb[k][t];
                }
            } else if (w == 0) {
                const int oa = p1 ? 3 * os : 0;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const float* xr = xs + (g4 * 4 + 2 * h + e) * 128 + ob;
                    ts.d[k][e][0] = xr[oa];          // d0 (pair 0) or d3 (pair 1)
                    ts.d[k][e][1] = xr[os];
                    ts.d[k][e][2] = xr[2 * os];
                }
            } else {
                float t4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const float da = ts.d[k][e][0], d1 = ts.d[k][e][1], d2 = ts.d[k][e][2];
                    if (w == 1) t4[2 * h + e] = (p1 ? d2 : da) - (p1 ? d1 : d2);   // d0 - d2 | d2 - d1
                    else t4[2 * h + e] = d1 + (p1 ? -da : d2);                     // d1 + d2 | d1 - d3
                    if (P::SCALED) t4[2 * h + e] *= P::SX;
                }
                v4 q[NT];
                P::split4(t4, q);                    // (element by element: the two unused ones fold away)
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int e = 2 * h; e < 2 * h + 2; ++e) {
                        if (w == 1) ts.pa[k][t][e] = q[t][e];
                        else ts.pb[k][t][e] = q[t][e];
                    }
            }
        }
    };
    auto transform = [&](int c1) {
        TState ts;
#pragma unroll
        for (int u = 0; u < T_UNITS; ++u) transform_unit(c1, u, ts);
    };
    // The residual x of this wave's 32 output rows passes through the staging buffers exactly once: the wave keeps a
    // copy in its (until the epilogue unused) transpose slot, row-major [row][64 columns] as the epilogue reads it --
    // shifts 0 and +d of a staged row sit at floats 32..95 in both staging forms.  No second read of x from memory.
    // One wave per chunk has work here, so it is a branch, and it stands apart from the transform: in the chunk loop it
    // runs ahead of step 1, where it splits no MFMA block that carries transform work.
    auto keep_residual = [&](int c1) {
        const int ch0 = chunk_of(c1) * KC;
        if (al16 && ch0 / 32 == wave) {
            const float* xs = Xraw + (c1 & 1) * T::RAW_FLOATS;
            const int r0 = ch0 % 32;
#pragma unroll
            for (int i = 0; i < KC / 4; ++i) {
                const int rr = (lane >> 4) + 4 * i;
                const bx6_f32x4 v = *reinterpret_cast<const bx6_f32x4*>(xs + rr * 128 + 32 + 4 * (lane & 15));
                *reinterpret_cast<bx6_f32x4*>(trw + (r0 + rr) * 64 + 4 * (lane & 15)) = v;
            }
        }
    };

    // ---- GEMM1: m_j[2C x 32] = G_j[2C x C] . t_j[C x 32], j = 0..3; this wave: row tiles `wave` and C/32 + wave
    bx_f32x16 acc[2][4];
    __amdgpu_buffer_rsrc_t rA1 = __builtin_amdgcn_make_buffer_rsrc((void*)a.A1, 0, 2 * C * 4 * C * 2 * NT, 0x00020000);
    const int lane16 = lane * 16;
    auto load_a1 = [&](v8 (&dst)[2][NT], int kb, int j) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < NT; ++t)
#ifdef BX6_ABL_A_HOT     // timing ablation only (wrong results): every step re-reads the same fragments -> they come from the CU's L1
                dst[m][t] = __builtin_bit_cast(v8, __builtin_amdgcn_raw_buffer_load_b128(rA1, lane16, ((mt1[m] * NKB * 4) * NT + t) * 1024 + 0 * (kb + j), 0));
#else
                dst[m][t] = __builtin_bit_cast(v8, __builtin_amdgcn_raw_buffer_load_b128(rA1, lane16, (((mt1[m] * NKB + kb) * 4 + j) * NT + t) * 1024, 0));
#endif
    };
    // quarter-step ring (AR == BX6_AR_QUARTER): request the three fragments of quarter-step qq = 4 j + 2 m + h of the chunk with
    // loop index cbi into set qq & 3 -- bx6_load_a1h's addressing for the one row half h
    [[maybe_unused]] auto req_a1q = [&](int cbi, int qq) __attribute__((always_inline)) {
        if constexpr (MF >= BX6_MF_16)
            bx6_load_a1q<v8, NT>(gs1.ar[(qq >> 1) & 1][qq & 1], rA1, bx6_voff_a1h<NT>(lane) + (qq & 1) * 256,
                                 ((mt1[(qq >> 1) & 1] * NKB + 2 * chunk_of(cbi)) * 4 + (qq >> 2)) * NT * 1024);
    };

    if constexpr (MF >= BX6_MF_16) {
        // 16x16x32: the first half-step's six A fragments (product 0 of row tile 0 -- bx6_load_a1h) are requested AHEAD of the
        // wave's LDS-DMA pieces, and the pieces as one sequence (by halves, more than one chunk: every wave stages exactly one of
        // chunks 0 and 1).  The correction rows are then older than six L2-served fragments and the pieces, whatever the staging
        // form: the wait in front of the start values (below) leaves those outstanding and does not wait for the staged x.
        static_assert(T::HALVES && NCB > 1 && BX6_PF(NT) == 1 && KC == 32,
                      "a wave stages chunk 0 or chunk 1; one half-step of six fragments ahead: NAF and the chunk loop's vmcnt counts as in the 32x32x16 form");
        if constexpr (AR == BX6_AR_QUARTER) {
            // quarter-step ring: the sets of the first BX6_A_LEAD quarter-steps of chunk 0 (three fragments each), all of them
            // ahead of the pieces -- the same order of ages: correction rows, L2-served fragments (nine instead of six), pieces
#pragma unroll
            for (int qq = 0; qq < BX6_A_LEAD; ++qq) req_a1q(0, qq);
        } else {
        bx6_load_a1h<v8, NT>(gs1.ar[0], rA1, bx6_voff_a1h<NT>(lane), ((mt1[0] * NKB + 2 * chunk_of(0)) * 4 + 0) * NT * 1024);
        }
        stage_dma(shalf);
    } else {
    if (stages(0)) stage_dma(0);
    if (NCB > 1 && stages(1)) stage_dma(1);
    }
    // A fragments run PF (k-block, product) steps ahead of their use, in a ring of four register sets indexed by the
    // step number (compile time: the steps of a chunk are a multiple of four).  One step is 2 NPR MFMAs = 32 NPR matrix-pipe
    // cycles per wave: six products cover an L2 round trip with one step, three products need two.
    constexpr int PF = BX6_PF(NT);
    v8 a_ring[4][2][NT];
    // 16x16x32 fragments of (32-channel block kk, product j, row tile m): half h takes rows 16 h + r16 of k-blocks 2 kk + (oct >> 1),
    // k half oct & 1 -- the bytes of the two 32x32x16 fragments of those k-blocks; every 16-lane group reads 256 contiguous bytes
    // (16x16x32: requested above)
    if constexpr (MF < BX6_MF_16) {
#pragma unroll
    for (int s0 = 0; s0 < PF; ++s0) load_a1(a_ring[s0], chunk_of(0) * (KC / 16) + (s0 >> 2), s0 & 3);
    }
    constexpr int NAF = PF * NA;              // A fragment loads in flight behind anything older
    // chunk 0 has landed (this wave's part; the barrier makes it everyone's): all but the loads issued after it -- chunk 1
    // and the NAF A fragments.  hipcc does not make a barrier wait for LDS-DMA.  A piece is one request in the 16-byte
    // forms and four dword requests otherwise.  By halves a wave holds pieces of ONE of the two chunks: the half that staged
    // chunk 0 has only the A fragments behind it, the other half has no part in chunk 0 and nothing to wait for yet.
    constexpr int P16 = NPIECE + NAF, P4 = 4 * NPIECE + NAF;
    static_assert(P4 < 64, "vmcnt is a 6-bit counter");
    if constexpr (MF >= BX6_MF_16) {
        // Start values of the accumulators: what the correction k-block summed -- the step-embedding row times the Winograd
        // transform of the in-range indicator of the four shifts (exact small integers, per column half), plus the conv bias in
        // product 1 (m1 enters both outputs of a pair with +1) -- is a rank-1 fp32 expression per register, one rounding each.
        // The rows were the kernel's first requests (vmcnt retires in order: the compiler's waits in front of these FMAs count
        // the six A fragments -- quarter-step ring: nine -- behind them and leave the younger LDS-DMA pieces alone), so this runs under the first staging
        // wait and not behind the chunk barrier.
        float bi[2][4];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int qc = q0 + 16 * c + (lane & 15);
            const int pc = ((qc >> log2d) << (log2d + 1)) + (qc & (dil - 1));   // first-half position of the lane's column 16 c + r16
            const float v0 = ((unsigned)(pc - dil) < (unsigned)L) ? 1.f : 0.f;
            const float v1 = ((unsigned)pc < (unsigned)L) ? 1.f : 0.f;
            const float v2 = ((unsigned)(pc + dil) < (unsigned)L) ? 1.f : 0.f;
            const float v3 = ((unsigned)(pc + 2 * dil) < (unsigned)L) ? 1.f : 0.f;
            bi[c][0] = v0 - v2; bi[c][1] = v1 + v2; bi[c][2] = v2 - v1; bi[c][3] = v1 - v3;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            gs1.acc[m][j][h][c][r] = j == 1 ? __builtin_fmaf(gs1.av[m][h][j][r], bi[c][j], gs1.ab[m][h][r])
                                                            : gs1.av[m][h][j][r] * bi[c][j];
        // (opaque to the optimiser, or it sinks the FMAs to their first use, behind the barrier and transform(0))
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int c = 0; c < 2; ++c) asm volatile("" : "+v"(gs1.acc[m][j][h][c]));
    }
    if constexpr (MF >= BX6_MF_16) {   // (the pieces are this wave's youngest requests here)
        if (stages(0)) __builtin_amdgcn_s_waitcnt(0x0F70);
    } else if (HALVES) {
        if (stages(0)) __builtin_amdgcn_s_waitcnt(0x0F70 | NAF);
    } else if (NCB > 1) {
        if (x4) __builtin_amdgcn_s_waitcnt(0x0F70 | (P16 & 15) | ((P16 >> 4) << 14));
        else __builtin_amdgcn_s_waitcnt(0x0F70 | (P4 & 15) | ((P4 >> 4) << 14));
    } else {
        __builtin_amdgcn_s_waitcnt(0x0F70 | NAF);
    }
    __syncthreads();
    stamp(1);
    if constexpr (MF < BX6_MF_16) {   // correction k-block: k = 0 the step-embedding row (x the Winograd transform of the in-range indicator of the four
        // shifts), k = 1 of product 1 the conv bias (m1 enters both outputs of a pair with +1)
        const float v0 = ((unsigned)(p - dil) < (unsigned)L) ? 1.f : 0.f;
        const float v1 = ((unsigned)p < (unsigned)L) ? 1.f : 0.f;
        const float v2 = ((unsigned)(p + dil) < (unsigned)L) ? 1.f : 0.f;
        const float v3 = ((unsigned)(p + 2 * dil) < (unsigned)L) ? 1.f : 0.f;
        const float bi[4] = {v0 - v2, v1 + v2, v2 - v1, v1 - v3};
        bx_f32x16 zero;
#pragma unroll
        for (int r = 0; r < 16; ++r) zero[r] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // (scaled splits: the indicator operand carries the activation scale, the A rows the weight scale: exact)
            const v8 bf = P::bvals(lhi ? 0.f : bi[j] * P::SX, (lhi || j != 1) ? 0.f : P::SX);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                v8 af[NT];
                P::rank2(av1[m][j] * ws1, j == 1 ? ab1[m] * ws1 : 0.f, lhi == 0, af);
                acc[m][j] = zero;
#pragma unroll
                for (int t = NT - 1; t >= 0; --t) acc[m][j] = P::mfma(af[t], bf, acc[m][j]);
            }
        }
    }
    transform(0);
    keep_residual(0);
    // chunk 1 has landed too (younger: only the NAF A fragments; either half.  16x16x32: nothing is younger than the pieces yet)
    if constexpr (MF >= BX6_MF_16) __builtin_amdgcn_s_waitcnt(0x0F70);
    else __builtin_amdgcn_s_waitcnt(0x0F70 | NAF);
    __syncthreads();                          // transformed chunk 0 visible, raw chunk 1 complete

    constexpr int SPC = (KC / 16) * 4;        // (k-block, product) steps per chunk
    // One (k-block, product) step: prefetch of the next step's A fragments, three B fragments from LDS, 12 MFMAs.
    // WITH_T (step 0 of every chunk but the last): the transform pass of the NEXT chunk rides in this step's MFMA stream.  It
    // has no branch, so it shares the step's basic block, and its seven units stand in program order one behind every
    // few MFMAs (T_SLOTS), each (MFMA, unit) slice fenced by sched_barrier: the reads of half an item go out behind one
    // MFMA and return under the next ones (an MFMA holds the matrix pipe for 32 cycles; the wave issues other work
    // meanwhile), instead of a chain of LDS round trips in front of the MFMAs with the matrix pipe idle (both waves of a
    // SIMD reach it at the same time).  Step 1 starts with the one wave's residual copy of that chunk (keep_residual).
    // the MFMA of the step (of 2 NPR) behind which each unit stands: a half's reads have one MFMA or more to return
    constexpr int T_SLOTS[2][T_UNITS] = {{0, 1, 2, 2, 4, 5, 5}, {BX6_T_SLOTS}};   // [6 | 12 MFMAs per step]
    constexpr bool B_AHEAD = !(C == 256 && NT == 2);   // (the 2-term instance at C = 256 has no registers left for the second set)
    v8 bq_ring[2][NT];
    auto do_step = [&](int cb, auto ST, auto WITH_T) {
        constexpr int st = decltype(ST)::value;
        constexpr bool with_t = decltype(WITH_T)::value;
        constexpr int it = st >> 2, j = st & 3;
        constexpr int sn = (st + PF) % SPC, itn = sn >> 2, jn = sn & 3;
        const int cbn = cb + (st + PF) / SPC;
        const char* tb = Bop + (cb & 1) * T::BOP_BYTES + lhi * (4 * NT * 512) + l31 * 16;
        if (st == 1 && cb + 1 < NCB) keep_residual(cb + 1);
        if (cbn < NCB) load_a1(a_ring[(st + PF) & 3], chunk_of(cbn) * (KC / 16) + itn, jn);   // (no load left in flight behind the last step)
        __builtin_amdgcn_sched_barrier(0);   // keep the prefetch PF whole steps ahead of its use
        // B fragments one step ahead inside a chunk (the first step's cannot be asked for before the chunk barrier)
        v8 (&bq)[NT] = bq_ring[st & 1];
        if (st == 0 || !B_AHEAD) {
#pragma unroll
            for (int t = 0; t < NT; ++t) bq[t] = *reinterpret_cast<const v8*>(tb + ((2 * it * 4 + j) * NT + t) * 512);
        }
        if (B_AHEAD && st + 1 < SPC) {
            constexpr int it1 = (st + 1) >> 2, j1 = (st + 1) & 3;
#pragma unroll
            for (int t = 0; t < NT; ++t) bq_ring[(st + 1) & 1][t] = *reinterpret_cast<const v8*>(tb + ((2 * it1 * 4 + j1) * NT + t) * 512);
            __builtin_amdgcn_sched_barrier(0);
        }
#if defined(BX6_ABL_NO_TRANSFORM)
        constexpr bool ride = false;
#elif defined(BX6_ABL_NO_INTERLEAVE)
        constexpr bool ride = false;
        if (with_t) { transform(cb + 1); __builtin_amdgcn_sched_barrier(0); }
#else
        constexpr bool ride = with_t;
#endif
        TState ts;
#pragma unroll
        for (int t = 0; t < NPR; ++t)
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                acc[m][j] = P::mfma(a_ring[st & 3][m][P::ia(t)], bq[P::ib(t)], acc[m][j]);
                if (ride) {
                    const int i = 2 * t + m;
#pragma unroll
                    for (int u = 0; u < T_UNITS; ++u)
                        if (T_SLOTS[NPR == 3 ? 0 : 1][u] == i) transform_unit(cb + 1, u, ts);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
    };
    auto do_steps_from1 = [&](int cb) {
        if constexpr (SPC == 4) {
            do_step(cb, std::integral_constant<int, 1>{}, std::false_type{});
            do_step(cb, std::integral_constant<int, 2>{}, std::false_type{});
            do_step(cb, std::integral_constant<int, 3>{}, std::false_type{});
        } else {
            do_step(cb, std::integral_constant<int, 1>{}, std::false_type{});
            do_step(cb, std::integral_constant<int, 2>{}, std::false_type{});
            do_step(cb, std::integral_constant<int, 3>{}, std::false_type{});
            do_step(cb, std::integral_constant<int, 4>{}, std::false_type{});
            do_step(cb, std::integral_constant<int, 5>{}, std::false_type{});
            do_step(cb, std::integral_constant<int, 6>{}, std::false_type{});
            do_step(cb, std::integral_constant<int, 7>{}, std::false_type{});
        }
    };
    static_assert((SPC == 4 || SPC == 8) && PF >= 1 && PF <= 3, "steps per chunk, prefetch distance");
    if constexpr (MF >= BX6_MF_16) {
        // The chunk (one 32-channel block) in eight half-steps (product j, row tile m): each requests the six A fragments of the
        // next half-step and issues 24 MFMAs of 16 cycles -- the period, the A ring and the load counts of a 32x32x16 step.  The
        // six B fragments of a product serve its two half-steps; behind the last use of a term in the second one (the products
        // run (2,0) (1,1) (0,2) (1,0) (0,1) (0,0): term 2 is free after the third, term 1 after the fifth) the next product's
        // fragment of that term is read into the same registers; term 0, which the next product's first MFMA needs, alternates
        // between two register sets and is read at the start of the second half-step.  The transform
        // units of the next chunk ride in half-step 0 (T16_SLOTS), the residual copy stands ahead of half-step 2.
        const int r16 = lane & 15, oct = lane >> 4;
        const int voffa = bx6_voff_a1h<NT>(lane);
        constexpr int T16_SLOTS[T_UNITS] = {BX6_T16_SLOTS};
        v8 bq[2][NT], bq0[2][2];   // [column half][term] (terms 1, 2); term 0: [product & 1][column half]
        if constexpr (AR == BX6_AR_QUARTER) {
        // Quarter-step ring.  The two row halves h of a half-step use disjoint fragments and disjoint accumulators, so the half-step
        // runs as two quarter-steps (h outer, then t, then c: 12 MFMAs on two alternating accumulators), a quarter-step needs three
        // fragments, and the 48 registers hold four sets.  Quarter-step q = 4 j + 2 m + h (sixteen per chunk) requests the set of quarter-step
        // q + BX6_A_LEAD (the last BX6_A_LEAD of a chunk: of the next chunk's first ones) into set (q + BX6_A_LEAD) & 3, last read
        // 4 - BX6_A_LEAD quarter-steps ago: a request leads its first use by 12 BX6_A_LEAD MFMAs (36 = 576 matrix-pipe cycles of
        // the wave's own work against 24 = 384 of the half-step ring) at the same registers, L2 bytes and MFMA count.  Every
        // accumulator receives its start value, the chunks and the products in the order of the half-step ring: equal bits.
        // B side: the six fragments of a product serve its four quarter-steps; the refills behind a term's last use and the
        // alternate term-0 set stand in the product's last quarter-step (m = 1, h = 1), where the registers come free.
        // The transform units ride in quarter-steps 0 and 1 (T16_SLOTS counts MFMAs across both), the residual copy stands ahead
        // of quarter-step 4.
        constexpr int LEAD = BX6_A_LEAD, QPC = 16;   // quarter-steps per chunk: four products x two row tiles x two row halves
        auto do_quarter = [&](int cb, auto QS, auto WITH_T, TState& ts) __attribute__((always_inline)) {
            constexpr int qs = decltype(QS)::value, j = qs >> 2, m = (qs >> 1) & 1, h = qs & 1;
            constexpr bool ride = decltype(WITH_T)::value;
            constexpr bool lastq = m == 1 && h == 1;
            const char* tb = Bop + (cb & 1) * T::BOP_BYTES + oct * (4 * NT * 512) + r16 * 16;
            if (qs == 4 && cb + 1 < NCB) keep_residual(cb + 1);
            // (fenced on both sides: with LEAD = 3 the request overwrites the set the previous quarter-step's MFMAs read, and a request
            // moved up between those would need three more registers per fragment)
            __builtin_amdgcn_sched_barrier(0);
            if (qs + LEAD < QPC) req_a1q(cb, qs + LEAD);
            else if (cb + 1 < NCB) req_a1q(cb + 1, qs + LEAD - QPC);   // (no load left in flight behind the last chunk)
            __builtin_amdgcn_sched_barrier(0);   // keep the prefetch LEAD whole quarter-steps ahead of its use
            if (qs == 0) {   // (a chunk's first fragments cannot be asked for before the chunk barrier)
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int c = 0; c < 2; ++c) (t ? bq[c][t] : bq0[0][c]) = *reinterpret_cast<const v8*>(tb + (j * NT + t) * 512 + c * 256);
            }
            if (lastq && j < 3) {   // term 0 of the next product: needed by its first MFMA, so it has a register set of its own
#pragma unroll
                for (int c = 0; c < 2; ++c) bq0[(j + 1) & 1][c] = *reinterpret_cast<const v8*>(tb + ((j + 1) * NT) * 512 + c * 256);
            }
#pragma unroll
            for (int t = 0; t < NPR; ++t) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    gs1.acc[m][j][h][c] = P::mfma16(gs1.ar[m][h][P::ia(t)], P::ib(t) ? bq[c][P::ib(t)] : bq0[j & 1][c], gs1.acc[m][j][h][c]);
                    if (ride) {
                        const int i = 12 * qs + 2 * t + c;
#pragma unroll
                        for (int u = 0; u < T_UNITS; ++u)
                            if (T16_SLOTS[u] == i) transform_unit(cb + 1, u, ts);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                if (lastq && j < 3 && (t == 2 || t == 4)) {   // the next product's fragments of the term that has just had its last use
                    const int term = (t == 2) ? 2 : 1;
#pragma unroll
                    for (int c = 0; c < 2; ++c) bq[c][term] = *reinterpret_cast<const v8*>(tb + ((j + 1) * NT + term) * 512 + c * 256);
                }
            }
        };
        for (int cb = 0; cb < NCB; ++cb) {
            if (cb + 2 < NCB && stages(cb + 2)) stage_dma(cb + 2);
            TState ts;
            if (cb + 1 < NCB) {
                do_quarter(cb, std::integral_constant<int, 0>{}, std::true_type{}, ts);
                do_quarter(cb, std::integral_constant<int, 1>{}, std::true_type{}, ts);
            } else {
                do_quarter(cb, std::integral_constant<int, 0>{}, std::false_type{}, ts);
                do_quarter(cb, std::integral_constant<int, 1>{}, std::false_type{}, ts);
            }
            do_quarter(cb, std::integral_constant<int, 2>{}, std::false_type{}, ts);
            do_quarter(cb, std::integral_constant<int, 3>{}, std::false_type{}, ts);
            do_quarter(cb, std::integral_constant<int, 4>{}, std::false_type{}, ts);
            do_quarter(cb, std::integral_constant<int, 5>{}, std::false_type{}, ts);
            do_quarter(cb, std::integral_constant<int, 6>{}, std::false_type{}, ts);
            do_quarter(cb, std::integral_constant<int, 7>{}, std::false_type{}, ts);
            do_quarter(cb, std::integral_constant<int, 8>{}, std::false_type{}, ts);
            do_quarter(cb, std::integral_constant<int, 9>{}, std::false_type{}, ts);
            do_quarter(cb, std::integral_constant<int, 10>{}, std::false_type{}, ts);
            do_quarter(cb, std::integral_constant<int, 11>{}, std::false_type{}, ts);
            do_quarter(cb, std::integral_constant<int, 12>{}, std::false_type{}, ts);
            do_quarter(cb, std::integral_constant<int, 13>{}, std::false_type{}, ts);
            do_quarter(cb, std::integral_constant<int, 14>{}, std::false_type{}, ts);
            do_quarter(cb, std::integral_constant<int, 15>{}, std::false_type{}, ts);
            stamp(8 + 2 * cb);
            // The LDS-DMA of chunk cb + 2 (requested at the top of this iteration) has landed: younger than the pieces are only
            // the 3 BX6_A_LEAD fragments of the next chunk's first quarter-steps -- every older fragment of this chunk has been
            // waited for by the MFMAs that read it.  (Last chunk: nothing is in flight.)  The count must stay below 16: this form
            // of the immediate carries only the counter's low four bits.
            static_assert(3 * LEAD < 16, "vmcnt immediate: low four bits only");
            __builtin_amdgcn_s_waitcnt(0x0F70 | (NT * LEAD));
            __syncthreads();
            stamp(9 + 2 * cb);
        }
        } else {
        auto do_half = [&](int cb, auto HS, auto WITH_T) {
            constexpr int hs = decltype(HS)::value, j = hs >> 1, m = hs & 1;
            constexpr bool ride = decltype(WITH_T)::value;
            const char* tb = Bop + (cb & 1) * T::BOP_BYTES + oct * (4 * NT * 512) + r16 * 16;
            if (hs == 2 && cb + 1 < NCB) keep_residual(cb + 1);
            if (hs < 7) bx6_load_a1h<v8, NT>(gs1.ar[(hs + 1) & 1], rA1, voffa, ((mt1[(hs + 1) & 1] * NKB + 2 * chunk_of(cb)) * 4 + ((hs + 1) >> 1)) * NT * 1024);
            else if (cb + 1 < NCB) bx6_load_a1h<v8, NT>(gs1.ar[0], rA1, voffa, ((mt1[0] * NKB + 2 * chunk_of(cb + 1)) * 4 + 0) * NT * 1024);
            __builtin_amdgcn_sched_barrier(0);   // keep the prefetch a whole half-step ahead of its use
            if (hs == 0) {   // (a chunk's first fragments cannot be asked for before the chunk barrier)
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int c = 0; c < 2; ++c) (t ? bq[c][t] : bq0[0][c]) = *reinterpret_cast<const v8*>(tb + (j * NT + t) * 512 + c * 256);
            }
            if (m == 1 && j < 3) {   // term 0 of the next product: needed by its first MFMA, so it has a register set of its own
#pragma unroll
                for (int c = 0; c < 2; ++c) bq0[(j + 1) & 1][c] = *reinterpret_cast<const v8*>(tb + ((j + 1) * NT) * 512 + c * 256);
            }
            TState ts;
#pragma unroll
            for (int t = 0; t < NPR; ++t) {
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        gs1.acc[m][j][h][c] = P::mfma16(gs1.ar[hs & 1][h][P::ia(t)], P::ib(t) ? bq[c][P::ib(t)] : bq0[j & 1][c], gs1.acc[m][j][h][c]);
                        if (ride) {
                            const int i = (2 * t + h) * 2 + c;
#pragma unroll
                            for (int u = 0; u < T_UNITS; ++u)
                                if (T16_SLOTS[u] == i) transform_unit(cb + 1, u, ts);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                if (m == 1 && j < 3 && (t == 2 || t == 4)) {   // the next product's fragments of the term that has just had its last use
                    const int term = (t == 2) ? 2 : 1;
#pragma unroll
                    for (int c = 0; c < 2; ++c) bq[c][term] = *reinterpret_cast<const v8*>(tb + ((j + 1) * NT + term) * 512 + c * 256);
                }
            }
        };
        for (int cb = 0; cb < NCB; ++cb) {
            if (cb + 2 < NCB && stages(cb + 2)) stage_dma(cb + 2);
            if (cb + 1 < NCB) do_half(cb, std::integral_constant<int, 0>{}, std::true_type{});
            else do_half(cb, std::integral_constant<int, 0>{}, std::false_type{});
            do_half(cb, std::integral_constant<int, 1>{}, std::false_type{});
            do_half(cb, std::integral_constant<int, 2>{}, std::false_type{});
            do_half(cb, std::integral_constant<int, 3>{}, std::false_type{});
            do_half(cb, std::integral_constant<int, 4>{}, std::false_type{});
            do_half(cb, std::integral_constant<int, 5>{}, std::false_type{});
            do_half(cb, std::integral_constant<int, 6>{}, std::false_type{});
            do_half(cb, std::integral_constant<int, 7>{}, std::false_type{});
            stamp(8 + 2 * cb);
            __builtin_amdgcn_s_waitcnt(0x0F70 | NAF);   // (as below: the LDS-DMA of chunk cb + 2 has landed, only the next half-step's A fragments are younger)
            __syncthreads();
            stamp(9 + 2 * cb);
        }
        }
    } else {
    for (int cb = 0; cb < NCB; ++cb) {
#ifndef BX6_ABL_NO_STAGE
        if (cb + 2 < NCB && stages(cb + 2)) stage_dma(cb + 2);   // into the raw buffer chunk cb occupied (transformed an iteration ago)
#endif
        if (cb + 1 < NCB) do_step(cb, std::integral_constant<int, 0>{}, std::true_type{});
        else do_step(cb, std::integral_constant<int, 0>{}, std::false_type{});
        do_steps_from1(cb);
        stamp(8 + 2 * cb);
        // transformed chunk cb+1 visible after the barrier; the LDS-DMA of chunk cb+2 must have landed too (hipcc does not
        // count LDS-DMA among the accesses a barrier waits for): the only younger loads are the NAF A fragments of the next steps.
        // The same count serves a wave that staged nothing in this chunk: all it has in flight are those A fragments.
#ifndef BX6_ABL_NO_DMA_WAIT     // (timing ablations, wrong results: no wait for the staged chunk / no chunk barrier / no staging)
        __builtin_amdgcn_s_waitcnt(0x0F70 | NAF);
#endif
#ifndef BX6_ABL_NO_BARRIER
        __syncthreads();
#endif
        stamp(9 + 2 * cb);
    }
    }
    stamp(2);
    // The tail's lane number.  The both-GEMM 16x16x32 instances hide it from the optimiser here: whatever the tail derives from
    // it (addresses of the gate tile, the transpose slot, the x / skip rows) is then computed here and not ahead of GEMM1, which
    // has no register to carry it (256 of 256).
    int lane_t = lane;
    if constexpr (MF >= BX6_MF_16) asm volatile("" : "+v"(lane_t));

    // 16x16x32 GEMM2: the biases in accumulator layout (one 16-byte load per row tile and half: rows 16 h + 4 oct + (0..3)), the
    // accumulators' start values.  Asked for here and not with the other correction operands: GEMM1 has no register to carry
    // them, and the gate stage covers the latency.
    [[maybe_unused]] std::conditional_t<MF >= BX6_MF_G2_16, Bx6G2State<MS>, Bx6Nothing> gs2;
    if constexpr (MF >= BX6_MF_G2_16) {
#pragma unroll
        for (int m = 0; m < 1 + MS; ++m)
#pragma unroll
            for (int h = 0; h < 2; ++h) gs2.bias[m][h] = *reinterpret_cast<const bx_f32x4*>(a.bias2 + mt2[m] * 32 + 16 * h + 4 * (lane_t >> 4));
    }
    // ---- x and running-skip tiles of this wave's output rows, requested before the gate stage (row-major 16-byte pieces:
    // lane = (row lane>>4 of a group of four rows, column quad lane&15; quads 0..7 = column tile 0, 8..15 = tile 1)
    const int L4 = L * 4;
    const bool first = a.first_layer, last = a.last_layer;
    __amdgpu_buffer_rsrc_t rXo = __builtin_amdgcn_make_buffer_rsrc((void*)(a.x_out + (size_t)b * C * L), 0, C * L * 4, 0x00020000);
    __amdgpu_buffer_rsrc_t rSk = __builtin_amdgcn_make_buffer_rsrc((void*)(a.skip + (size_t)b * S * L), 0, S * L * 4, 0x00020000);
    const int p0 = ((q0 >> log2d) << (log2d + 1)) + (q0 & (dil - 1));   // position of column 0 of tile 0 (d >= 32: q0 % 32 == 0 keeps it a multiple of 32)
    int voff4;
    {
        const int n4 = (lane_t & 15) >> 3;
        const int pos4 = (contig ? pbase + 32 * n4 : p0 + n4 * dil) + 4 * (lane_t & 7);
        voff4 = (pos4 < L) ? ((lane_t >> 4) * L + pos4) * 4 : 0x7ffffff0;
    }
    // (S = 2C: three row tiles per wave would take 96 registers here -- those instances fetch each tile in the epilogue;
    // they run two workgroups per CU, which cover each other's waits)
    constexpr bool PRELOAD = MS == 1;
    // a tile that is not read (the first layer's skip, the last layer's x) asks for an offset past the buffer: reads 0
    const int voff4s = first ? 0x7ffffff0 : voff4;
    auto load_pre = [&](int m, bx6_f32x4 (&dst)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (m == 0) dst[i] = *reinterpret_cast<const bx6_f32x4*>(trw + ((lane_t >> 4) + 4 * i) * 64 + 4 * (lane_t & 15));
            else dst[i] = bx6_load_f4(rSk, voff4s, ((wave * MS + (m - 1)) * 32 + 4 * i) * L4);
        }
    };
    bx6_f32x4 pre[PRELOAD ? 1 + MS : 1][8];
    if (PRELOAD && al16) {
#pragma unroll
        for (int m = 1; m < 1 + MS; ++m) load_pre(m, pre[PRELOAD ? m : 0]);
    }

    // ---- gate: g = tanh(H_t (+mel_t)) * sigmoid(H_s (+mel_s)) for both outputs of every pair, split -> LDS gate tile
    const float* melb = (EXTRA && a.melc) ? a.melc + (size_t)(a.mel_bstride ? b : 0) * 2 * C * L : nullptr;
    if constexpr (MF >= BX6_MF_16) {
        // a lane_t holds four consecutive channels 16 h + 4 oct + (0..3) of column 16 c + r16: the 8-byte half oct & 1 of item
        // [octet wave * 4 + 2 h + (oct >> 1)][term][column]
        const int r16 = lane_t & 15, oct = lane_t >> 4;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int qc = q0 + 16 * c + r16;
            const int pc = ((qc >> log2d) << (log2d + 1)) + (qc & (dil - 1));
            const int gc0 = contig ? pc - pbase : 16 * c + r16, gc1 = contig ? pc - pbase + dil : 32 + 16 * c + r16;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float ga[4], gb[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int ch = wave * 32 + 16 * h + 4 * oct + e;
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const int pos = pc + n * dil;
                        float ht, hs;
                        if (n == 0) {
                            ht = (gs1.acc[0][0][h][c][e] + gs1.acc[0][1][h][c][e]) + gs1.acc[0][2][h][c][e];
                            hs = (gs1.acc[1][0][h][c][e] + gs1.acc[1][1][h][c][e]) + gs1.acc[1][2][h][c][e];
                        } else {
                            ht = (gs1.acc[0][1][h][c][e] - gs1.acc[0][2][h][c][e]) - gs1.acc[0][3][h][c][e];
                            hs = (gs1.acc[1][1][h][c][e] - gs1.acc[1][2][h][c][e]) - gs1.acc[1][3][h][c][e];
                        }
                        if (EXTRA && melb && pos < L) {
                            ht += melb[(size_t)ch * L + pos];
                            hs += melb[(size_t)(C + ch) * L + pos];
                        }
                        if (EXTRA && a.hsave && pos < L) {   // training: keep the pre-activations for the gate adjoint (dword stores)
                            float* __restrict__ hb = a.hsave + (size_t)b * 2 * C * L;
                            hb[(size_t)ch * L + pos] = ht;
                            hb[(size_t)(C + ch) * L + pos] = hs;
                        }
                        const float g = bx6_gate(ht, hs) * P::SG;
                        if (n == 0) ga[e] = g; else gb[e] = g;
                    }
                }
                v4 s0[NT], s1[NT];
                P::split4(ga, s0);
                P::split4(gb, s1);
                char* dst = gt + ((wave * 4 + 2 * h + (oct >> 1)) * NT * 64) * 16 + (oct & 1) * 8;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    *reinterpret_cast<v4*>(dst + (t * 64 + gc0) * 16) = s0[t];
                    *reinterpret_cast<v4*>(dst + (t * 64 + gc1) * 16) = s1[t];
                }
            }
        }
    } else {
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
        float g0[4], g1[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = qd * 4 + e;
            const int ch = wave * 32 + e + 8 * qd + 4 * lhi;
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int pos = p + n * dil;
                float ht, hs;
                if (n == 0) {
                    ht = (acc[0][0][r] + acc[0][1][r]) + acc[0][2][r];
                    hs = (acc[1][0][r] + acc[1][1][r]) + acc[1][2][r];
                } else {
                    ht = (acc[0][1][r] - acc[0][2][r]) - acc[0][3][r];
                    hs = (acc[1][1][r] - acc[1][2][r]) - acc[1][3][r];
                }
                if (P::SCALED) { ht *= inv1; hs *= inv1; }       // undo the operand scales (powers of two: exact)
                if (EXTRA && melb && pos < L) {
                    ht += melb[(size_t)ch * L + pos];
                    hs += melb[(size_t)(C + ch) * L + pos];
                }
                if (EXTRA && a.hsave && pos < L) {   // training: keep the pre-activations for the gate adjoint (dword stores)
                    float* __restrict__ hb = a.hsave + (size_t)b * 2 * C * L;
                    hb[(size_t)ch * L + pos] = ht;
                    hb[(size_t)(C + ch) * L + pos] = hs;
                }
                const float g = bx6_gate(ht, hs) * P::SG;
                if (n == 0) g0[e] = g; else g1[e] = g;
            }
        }
        v4 s0[NT], s1[NT];
        P::split4(g0, s0);
        P::split4(g1, s1);
        char* dst = gt + ((wave * 4 + qd) * NT * 64) * 16 + lhi * 8;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            *reinterpret_cast<v4*>(dst + (t * 64 + gcol0) * 16) = s0[t];
            *reinterpret_cast<v4*>(dst + (t * 64 + gcol1) * 16) = s1[t];
        }
    }
    }
    stamp(3);

    // ---- GEMM2: [res; skip][(C+S) x 64] = [Wr; Ws][(C+S) x C] . g[C x 64] (+ bias k-block); this wave: res tile `wave`
    // and its skip tiles, both column tiles
    __amdgpu_buffer_rsrc_t rA2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.A2, 0, (C + S) * C * 2 * NT, 0x00020000);
    v8 c_cur[1 + MS][NT], c_nxt[1 + MS][NT];
    auto load_a2 = [&](v8 (&dst)[1 + MS][NT], int kb, int m0) {
#pragma unroll
        for (int m = m0; m < 1 + MS; ++m)
#pragma unroll
            for (int t = 0; t < NT; ++t)
                dst[m][t] = __builtin_bit_cast(v8, __builtin_amdgcn_raw_buffer_load_b128(rA2, lane16, ((mt2[m] * NKB + kb) * NT + t) * 1024, 0));
    };
    const int rot2 = rot * (KC / 16);          // the same rotation of the k-block order in GEMM2
    auto kblock_of = [&](int kb) { const int k = kb + rot2; return k >= NKB ? k - NKB : k; };
    // The last layer's residual output feeds nothing (`wavenet.py:165`; the epilogue does not store it): its row tile
    // m = 0 -- A fragments, MFMAs, bias -- is left out there, by a wave-uniform choice between two instances of the loop.
    bx_f32x16 acc2[1 + MS][2];
    auto gemm2 = [&](auto WITH_RES) {
        constexpr int M0 = decltype(WITH_RES)::value ? 0 : 1;
        load_a2(c_cur, kblock_of(0), M0);
        {
            const v8 bf = P::bvals(lhi ? 0.f : P::SG, 0.f);      // a row of ones, at the gate operand's scale
            bx_f32x16 zero;
#pragma unroll
            for (int r = 0; r < 16; ++r) zero[r] = 0.f;
#pragma unroll
            for (int m = M0; m < 1 + MS; ++m) {
                v8 af[NT];
                P::rank2(av2[m] * ws2, 0.f, lhi == 0, af);
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    acc2[m][n] = zero;
#pragma unroll
                    for (int t = NT - 1; t >= 0; --t) acc2[m][n] = P::mfma(af[t], bf, acc2[m][n]);
                }
            }
        }
        __syncthreads();   // gate tile complete
        stamp(4);
        const char* gb = gt + lhi * (NT * 64 * 16) + l31 * 16;
#pragma unroll 2
        for (int kb = 0; kb < NKB; ++kb) {
            const int kbn = (kb + 1 < NKB) ? kb + 1 : kb;
            load_a2(c_nxt, kblock_of(kbn), M0);
            __builtin_amdgcn_sched_barrier(0);
            const char* gk = gb + kblock_of(kb) * (2 * NT * 64 * 16);
            v8 bq[2][NT];
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int t = 0; t < NT; ++t) bq[n][t] = *reinterpret_cast<const v8*>(gk + (t * 64 + n * 32) * 16);
#pragma unroll
            for (int t = 0; t < NPR; ++t)
#pragma unroll
                for (int m = M0; m < 1 + MS; ++m)
#pragma unroll
                    for (int n = 0; n < 2; ++n)
                        acc2[m][n] = P::mfma(c_cur[m][P::ia(t)], bq[n][P::ib(t)], acc2[m][n]);
#pragma unroll
            for (int m = M0; m < 1 + MS; ++m)
#pragma unroll
                for (int t = 0; t < NT; ++t) c_cur[m][t] = c_nxt[m][t];
        }
    };
    if constexpr (MF >= BX6_MF_G2_16) {
        // The same GEMM on v_mfma_f32_16x16x32_bf16.  A 32 x 32 tile is four slices (row half h, column half c) of four
        // registers: row = 16 h + 4 oct + reg, col = 16 c + r16.  A and B are the same 16-byte items read through another lane_t
        // map: the A fragment of (32-channel block kk, half h) takes rows 16 h + r16 of k-blocks 2 kk + (oct >> 1), k half
        // oct & 1 -- the two halves read exactly the bytes of the two 32x32x16 fragments of those k-blocks; B takes octet
        // 4 kk + oct of the gate tile, columns 32 n + 16 c + r16 (octet stride 3072 B = 0 mod 256: each group of ds_read_b128
        // lanes covers all banks once).  Per output element: the bias as start value, then the 32-channel blocks in the order rotated by
        // `rot`, then the products -- the 32x32x16 order, but one instruction sums 32 channels where two summed 16 + 16
        // (last-bit differences).  A block runs as two half-steps (h = 0, 1) of 8 NPR MFMAs; the (1 + MS) NT A fragments of a
        // half-step are requested one half-step ahead, the B fragments of a block serve both.
        // (The lambda is defined in these instances only: a generic lambda captures what its body names even where the body
        // is discarded, and the 32x32x16 instances compile to exactly the code they had without it.)
        auto gemm2_16 = [&](auto WITH_RES) {
            const int r16 = lane_t & 15, oct = lane_t >> 4;   // row / column of a 16-wide half, k-octet of a 32-channel block
            auto& acc2h = gs2.acc;
            constexpr int M0 = decltype(WITH_RES)::value ? 0 : 1;
            const int voffa = (oct >> 1) * (NT * 1024) + ((oct & 1) * 32 + r16) * 16;
            auto load_a2h = [&](v8 (&dst)[1 + MS][NT], int kk, int h) {
#pragma unroll
                for (int m = M0; m < 1 + MS; ++m)
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        dst[m][t] = __builtin_bit_cast(v8, __builtin_amdgcn_raw_buffer_load_b128(rA2, voffa + h * 256, ((mt2[m] * NKB + 2 * kk) * NT + t) * 1024, 0));
            };
            auto block_of = [&](int kk) { const int k = kk + rot; return k >= NCB ? k - NCB : k; };
            static_assert(KC == 32, "GEMM2's rotation counts 32-channel blocks");
            v8 ah[2][1 + MS][NT];
            load_a2h(ah[0], block_of(0), 0);
            // start values: the bias of the register's row, the same for every column (bit for bit what the bias k-block left:
            // the three terms of a split sum to the fp32 value exactly)
#pragma unroll
            for (int m = M0; m < 1 + MS; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int c = 0; c < 2; ++c) acc2h[m][n][h][c] = gs2.bias[m][h];
            __syncthreads();   // gate tile complete
            stamp(4);
            const char* gb = gt + oct * (NT * 64 * 16) + r16 * 16;
#pragma unroll 1
            for (int kk = 0; kk < NCB; ++kk) {
                const char* gk = gb + block_of(kk) * (4 * NT * 64 * 16);
                v8 bq[2][2][NT];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (h == 0) load_a2h(ah[1], block_of(kk), 1);
                    else load_a2h(ah[0], block_of(kk + 1 < NCB ? kk + 1 : kk), 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if (h == 0) {
#pragma unroll
                        for (int n = 0; n < 2; ++n)
#pragma unroll
                            for (int c = 0; c < 2; ++c)
#pragma unroll
                                for (int t = 0; t < NT; ++t) bq[n][c][t] = *reinterpret_cast<const v8*>(gk + (t * 64 + n * 32 + c * 16) * 16);
                    }
#pragma unroll
                    for (int t = 0; t < NPR; ++t)
#pragma unroll
                        for (int m = M0; m < 1 + MS; ++m)
#pragma unroll
                            for (int n = 0; n < 2; ++n)
#pragma unroll
                                for (int c = 0; c < 2; ++c)
                                    acc2h[m][n][h][c] = P::mfma16(ah[h][m][P::ia(t)], bq[n][c][P::ib(t)], acc2h[m][n][h][c]);
                }
            }
        };
        if (last) gemm2_16(std::false_type{});
        else gemm2_16(std::true_type{});
    } else {
        if (last) gemm2(std::false_type{});
        else gemm2(std::true_type{});
    }
    stamp(5);

    // ---- epilogue
    const float rs = 0.70710678118654752440f;
    if (al16) {
        // row tile by row tile through this wave's own LDS slot (no other wave touches it: no barrier), out as 16-byte rows
#pragma unroll
        for (int m = 0; m < 1 + MS; ++m) {
            if (m == 0 && last) continue;   // the last layer's residual output feeds nothing (`wavenet.py:165`)
            if (!PRELOAD || m == 0) load_pre(m, pre[0]);      // (m = 0: the x rows out of the wave's own slot, before it is overwritten)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if constexpr (MF >= BX6_MF_G2_16) {
                // the four octets of a lane group write rows 4 oct + r, 256 floats = 0 banks apart: the 16-column group of a
                // row is XORed with (row >> 2) & 3 = oct, which spreads them over the 64 banks; the read-back undoes it
                const int r16 = lane_t & 15, oct = lane_t >> 4;
                auto& acc2h = gs2.acc;
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int c = 0; c < 2; ++c)
#pragma unroll
                            for (int r = 0; r < 4; ++r) trw[(16 * h + 4 * oct + r) * 64 + ((n * 32 + 16 * c + r16) ^ (oct << 4))] = acc2h[m][n][h][c][r];
            } else {
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) trw[((r & 3) + 8 * (r >> 2) + 4 * lhi) * 64 + n * 32 + l31] = P::SCALED ? acc2[m][n][r] * inv2 : acc2[m][n][r];
            }
            // one wave, LDS operations of a wave execute in order: only the compiler has to be kept from moving the reads
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const int row0 = (m == 0) ? wave * 32 : (wave * MS + (m - 1)) * 32;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                // (16x16x32: the slot's 16-column groups are XORed with (row >> 2) & 3 = i & 3, see the writes above)
                const bx6_f32x4 v = *reinterpret_cast<const bx6_f32x4*>(trw + ((lane_t >> 4) + 4 * i) * 64 +
                                                                        (MF >= BX6_MF_G2_16 ? (4 * (lane_t & 15)) ^ ((i & 3) << 4) : 4 * (lane_t & 15)));
                bx6_f32x4 o = pre[PRELOAD ? m : 0][i] + v;
                if (m == 0) o = o * rs;
                bx6_store_f4(o, m == 0 ? rXo : rSk, voff4, (row0 + 4 * i) * L4);
                // gfx950 hazard, found by the bit-for-bit determinism test: a VALU write (here the next v_pk_add / v_pk_mul) to
                // the data registers of a 16-byte buffer store in the slot right behind it changes what the store writes
                // for the last lanes of each 16-lane_t group (their last dword) -- hipcc's hazard recognizer leaves the wait
                // state out when the store carries an SGPR offset.  One wait state removes it (measured: 0 -> wrong in
                // 2 of 3 runs, 1 / 2 / 4 / 16 -> never); two are kept.
                asm volatile("s_nop 1" ::: "memory");
            }
            asm volatile("" ::: "memory");   // the next row tile overwrites the slot
        }
    } else if constexpr (MF >= BX6_MF_G2_16) {
        // rows not 16-byte aligned, 16x16x32 accumulators: the lane_t owns columns 16 c + r16 of both column tiles, rows 16 h + 4 oct + reg
        const int r16 = lane_t & 15, oct = lane_t >> 4;
        auto& acc2h = gs2.acc;
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int qc = q0 + 16 * c + r16;
                const int pc = ((qc >> log2d) << (log2d + 1)) + (qc & (dil - 1));
                const int pos = contig ? pbase + 32 * n + 16 * c + r16 : pc + n * dil;
                const int voffc = (pos < L) ? (4 * oct * L + pos) * 4 : 0x7ffffff0;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (!last) {
                        const int s0 = (wave * 32 + 16 * h) * L4;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rXall, voffc, s0 + r * L4, 0));
                            const float v = (x + acc2h[0][n][h][c][r]) * rs;
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rXo, voffc, s0 + r * L4, 0);
                        }
                    }
#pragma unroll
                    for (int m = 0; m < MS; ++m) {
                        const int s0 = ((wave * MS + m) * 32 + 16 * h) * L4;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float old = first ? 0.f : __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rSk, voffc, s0 + r * L4, 0));
                            const float v = old + acc2h[1 + m][n][h][c][r];
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rSk, voffc, s0 + r * L4, 0);
                        }
                    }
                }
            }
    } else {
        // rows not 16-byte aligned: per-lane_t dwords straight from the accumulator layout
        int voffn[2];
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int pos = contig ? pbase + 32 * n + l31 : p + n * dil;
            voffn[n] = (pos < L) ? (4 * lhi * L + pos) * 4 : 0x7ffffff0;
        }
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            if (!last) {
                const int s0 = (wave * 32) * L4;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int so = s0 + ((r & 3) + 8 * (r >> 2)) * L4;
                    const float x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rXall, voffn[n], so, 0));
                    const float v = (x + (P::SCALED ? acc2[0][n][r] * inv2 : acc2[0][n][r])) * rs;
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rXo, voffn[n], so, 0);
                }
            }
#pragma unroll
            for (int m = 0; m < MS; ++m) {
                const int s0 = ((wave * MS + m) * 32) * L4;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int so = s0 + ((r & 3) + 8 * (r >> 2)) * L4;
                    const float old = first ? 0.f : __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rSk, voffn[n], so, 0));
                    const float v = old + (P::SCALED ? acc2[1 + m][n][r] * inv2 : acc2[1 + m][n][r]);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rSk, voffn[n], so, 0);
                }
            }
        }
    }
    stamp(6);
    if (trc) {
        __builtin_amdgcn_s_waitcnt(0);   // everything (stores included) retired
        stamp(7);
    }
}

template <typename P, int C, int S, int MF = BX6_MF_32, int AR = BX6_AR_HALF>
static int launch_bx6_t(const WnLayerArgs& a, int log2d, hipStream_t s) {
    ProfileScope ps(P::NT == 3 ? "wn_layer_bx6" : "wn_layer_f16x3", s);
    using T = Bx6Tile<C, S, P::NT>;
    const int dil = 1 << log2d;
    const int nblk = (a.L + 2 * dil - 1) / (2 * dil);
    const int ntl = (nblk * dil + 31) / 32;
    const int ntiles = a.B * ntl;
    static const bool trace = std::getenv("DWS_BX6_TRACE") != nullptr;
    if (trace && !a.melc && !a.hsave) {
        wino_trace_launch(ntiles, T::WAVES, a, s, [&](const WnLayerArgs& at) {
            hipLaunchKernelGGL((wn_layer_bx6_kernel<P, C, S, false, MF, AR>), dim3(ntiles), dim3(T::NTH), 0, s, at, log2d);
        }, P::NT == 3 ? "bx6" : "f16x3");
        return DWS_OK;
    }
    if (a.melc || a.hsave) hipLaunchKernelGGL((wn_layer_bx6_kernel<P, C, S, true, MF, AR>), dim3(ntiles), dim3(T::NTH), 0, s, a, log2d);
    else hipLaunchKernelGGL((wn_layer_bx6_kernel<P, C, S, false, MF, AR>), dim3(ntiles), dim3(T::NTH), 0, s, a, log2d);
    return DWS_OK;
}

bool wn_layer_bx6_mfma16_supported(int C, int S, int split) { return split == WN_SPLIT_BF16X6 && C == 256 && S == 256; }

bool wn_layer_bx6_supported(int C, int S) {
    return (C == 64 && S == 64) || (C == 128 && S == 128) || (C == 128 && S == 256) || (C == 256 && S == 256);
}

template <typename P>
static int launch_bx6_p(int C, int S, const WnLayerArgs& a, int log2d, hipStream_t s) {
    if (C == 64 && S == 64) return launch_bx6_t<P, 64, 64>(a, log2d, s);
    if (C == 128 && S == 128) return launch_bx6_t<P, 128, 128>(a, log2d, s);
    if (C == 128 && S == 256) return launch_bx6_t<P, 128, 256>(a, log2d, s);
    if (C == 256 && S == 256) return launch_bx6_t<P, 256, 256>(a, log2d, s);
    return set_error(DWS_ERR_UNSUPPORTED, "wn_layer_bx6: (C=%d,S=%d) not instantiated", C, S);
}

int launch_wn_layer_bx6(int C, int S, const WnLayerArgs& a, int split, int mfma, int a_ring, hipStream_t s) {
    int log2d = 0;
    while ((1 << log2d) < a.dilation) ++log2d;
    DWS_CHECK((1 << log2d) == a.dilation, DWS_ERR_UNSUPPORTED, "wn_layer_bx6: dilation %d is not a power of two", a.dilation);
    DWS_CHECK((int64_t)a.L + 4 * (int64_t)a.dilation < ((int64_t)1 << 28), DWS_ERR_UNSUPPORTED, "wn_layer_bx6: L too large");
    DWS_CHECK((int64_t)(C > S ? C : S) * a.L * 4 < ((int64_t)1 << 31), DWS_ERR_UNSUPPORTED,
              "wn_layer_bx6: %d channels x L=%d exceed a 2 GiB tensor per clip", C > S ? C : S, a.L);
    if (split == WN_SPLIT_F16X3) {
        DWS_CHECK(a.hsave == nullptr, DWS_ERR_UNSUPPORTED, "wn_layer_f16x3: the training forward runs with precision=f32 or bf16x6");
        DWS_CHECK(a.wscale != nullptr, DWS_ERR_INVALID, "wn_layer_f16x3: no weight scales");
        return launch_bx6_p<SplitF16x2>(C, S, a, log2d, s);
    }
    // the 16x16x32 instances fetch the correction rows and the biases as 16-byte groups of four rows (accumulator layout)
    if ((mfma == WN_BX6_MFMA_G2_16 || mfma == WN_BX6_MFMA_16) && wn_layer_bx6_mfma16_supported(C, S, split)) {
        DWS_CHECK(((size_t)a.bias2 & 15) == 0, DWS_ERR_UNSUPPORTED, "wn_layer_bx6: bias2 is not 16-byte aligned");
        if (mfma == WN_BX6_MFMA_16)
            DWS_CHECK((((size_t)a.Abt | (size_t)a.bias1) & 15) == 0 && a.abt_bstride % 4 == 0 && a.abt_tstride % 4 == 0, DWS_ERR_UNSUPPORTED,
                      "wn_layer_bx6: Abt / bias1 rows are not 16-byte aligned (strides %d, %d floats)", a.abt_bstride, a.abt_tstride);
    }
    // the 16x16x32 shape exists for the instances it was measured on; every other instance has one shape and keeps it
    if (mfma == WN_BX6_MFMA_G2_16 && wn_layer_bx6_mfma16_supported(C, S, split)) return launch_bx6_t<SplitBf16x3, 256, 256, BX6_MF_G2_16>(a, log2d, s);
    // the A ring is a property of the 16x16x32 GEMM1: every other kernel has no such ring and runs whatever a_ring says
    DWS_CHECK(a_ring == WN_BX6_A_RING_HALF || a_ring == WN_BX6_A_RING_QUARTER, DWS_ERR_INVALID, "wn_layer_bx6: unknown A ring %d", a_ring);
    if (mfma == WN_BX6_MFMA_16 && wn_layer_bx6_mfma16_supported(C, S, split)) {
        if (a_ring == WN_BX6_A_RING_QUARTER) return launch_bx6_t<SplitBf16x3, 256, 256, BX6_MF_16, BX6_AR_QUARTER>(a, log2d, s);
        return launch_bx6_t<SplitBf16x3, 256, 256, BX6_MF_16>(a, log2d, s);
    }
    DWS_CHECK(mfma == WN_BX6_MFMA_32 || mfma == WN_BX6_MFMA_G2_16 || mfma == WN_BX6_MFMA_16, DWS_ERR_INVALID, "wn_layer_bx6: unknown MFMA shape %d", mfma);
    return launch_bx6_p<SplitBf16x3>(C, S, a, log2d, s);
}

// ---- the arithmetic alone, for the GEMM-level accuracy test: C[M][N] = A[M][K] . B[K][N], fp32 in and out, every
// operand split in registers, one wave per 32 x 32 output tile (tests/test_bf16x6_gpu.py; not a fast GEMM).
// Scaled splits: A enters times sa, B times sb (powers of two from the caller), the result leaves times 1/(sa sb).
template <typename P>
__global__ __launch_bounds__(64) void gemm_bx6_kernel(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ Cm,
                                                      int M, int N, int K, float sa, float sb) {
    using v8 = typename P::v8;
    const int lane = threadIdx.x, l31 = lane & 31, lhi = lane >> 5;
    const int mt = blockIdx.y, nt = blockIdx.x;
    bx_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int kb = 0; kb < K / 16; ++kb) {
        v8 af[P::NT], bf[P::NT];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = kb * 16 + 8 * lhi + e;
            P::split1(A[(size_t)(mt * 32 + l31) * K + k] * sa, af, e);
            P::split1(B[(size_t)k * N + nt * 32 + l31] * sb, bf, e);
        }
#pragma unroll
        for (int t = 0; t < P::NP; ++t) acc = P::mfma(af[P::ia(t)], bf[P::ib(t)], acc);
    }
    const float inv = 1.f / (sa * sb);
#pragma unroll
    for (int r = 0; r < 16; ++r)
        Cm[(size_t)(mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi) * N + nt * 32 + l31] = acc[r] * inv;
}

int launch_gemm_bx6(const float* A, const float* B, float* Cm, int M, int N, int K, int split, float sa, float sb, hipStream_t s) {
    DWS_CHECK(M > 0 && N > 0 && K > 0 && M % 32 == 0 && N % 32 == 0 && K % 16 == 0, DWS_ERR_UNSUPPORTED,
              "gemm_bf16x6 / gemm_f16x3: M=%d N=%d must be multiples of 32, K=%d of 16", M, N, K);
    if (split == WN_SPLIT_F16X3) {
        int ea = 0, eb = 0;
        DWS_CHECK(sa > 0.f && sb > 0.f && frexpf(sa, &ea) == 0.5f && frexpf(sb, &eb) == 0.5f, DWS_ERR_INVALID,
                  "gemm_f16x3: the operand scales must be powers of two (%g, %g)", (double)sa, (double)sb);
        hipLaunchKernelGGL(gemm_bx6_kernel<SplitF16x2>, dim3(N / 32, M / 32), dim3(64), 0, s, A, B, Cm, M, N, K, sa, sb);
    } else {
        hipLaunchKernelGGL(gemm_bx6_kernel<SplitBf16x3>, dim3(N / 32, M / 32), dim3(64), 0, s, A, B, Cm, M, N, K, 1.f, 1.f);
    }
    return DWS_OK;
}

}  // namespace dws

extern "C" int dws_gemm_bf16x6(const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K, void* stream) {
    DWS_CHECK(A && B && C, DWS_ERR_INVALID, "dws_gemm_bf16x6: null argument");
    DWS_CHECK(M <= (1 << 20) && N <= (1 << 20) && K <= (1 << 20), DWS_ERR_UNSUPPORTED, "dws_gemm_bf16x6: dimension too large");
    return dws::launch_gemm_bx6(A, B, C, (int)M, (int)N, (int)K, dws::WN_SPLIT_BF16X6, 1.f, 1.f, (hipStream_t)stream);
}

extern "C" int dws_gemm_f16x3(const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K, float scale_a, float scale_b,
                              void* stream) {
    DWS_CHECK(A && B && C, DWS_ERR_INVALID, "dws_gemm_f16x3: null argument");
    DWS_CHECK(M <= (1 << 20) && N <= (1 << 20) && K <= (1 << 20), DWS_ERR_UNSUPPORTED, "dws_gemm_f16x3: dimension too large");
    return dws::launch_gemm_bx6(A, B, C, (int)M, (int)N, (int)K, dws::WN_SPLIT_F16X3, scale_a, scale_b, (hipStream_t)stream);
}
