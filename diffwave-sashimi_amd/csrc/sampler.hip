// Reverse-diffusion sampler (`generate.py:23-55`) as a replayed hipGraph.
//
// Per step t = T-1 .. 0 the reference does (`generate.py:50-54`):
//   eps = net((x, t));  x = (x - (1-a_t)/sqrt(1-abar_t) * eps) / sqrt(a_t);  if t > 0: x += sigma_t * z
// with t, the noise and (partly) the tables crossing the host/device boundary
// every step.  Here the step index lives in device memory, the coefficient
// tables are device resident, and z comes either from an injected tensor
// (parity mode) or from an on-device Philox4x32-10 counter RNG, so that one
// reverse step is a fixed kernel sequence: captured once, replayed T times.
#include <cmath>
#include <type_traits>

#include "model.h"

namespace dws {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t out[4]) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// four N(0,1) samples for element group g of stream `t`
__device__ __forceinline__ void normal4(uint64_t seed, uint32_t t, uint64_t g, float z[4]) {
    uint32_t r[4];
    philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), t, 0x5eedu, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const float k = 2.3283064365386963e-10f;  // 2^-32
    const float u0 = ((float)r[0] + 0.5f) * k, u1 = ((float)r[1] + 0.5f) * k;
    const float u2 = ((float)r[2] + 0.5f) * k, u3 = ((float)r[3] + 0.5f) * k;
    const float ra = sqrtf(-2.f * logf(fminf(u0, 0.99999994f)));
    const float rb = sqrtf(-2.f * logf(fminf(u2, 0.99999994f)));
    float s, c;
    sincospif(2.f * u1, &s, &c);
    z[0] = ra * c; z[1] = ra * s;
    sincospif(2.f * u3, &s, &c);
    z[2] = rb * c; z[3] = rb * s;
}

// sampler state in device memory: [0] the step index t, [1] number of update blocks that have finished this step
__global__ void smp_set_step_kernel(int* t_dev, int t) { t_dev[0] = t; t_dev[1] = 0; }

// the few-step sampler's state also holds the Philox seed ([2..3]): its captured step bakes in no seed.  [5] is the
// history-valid word of the multistep kind (DWS_SAMPLER_DPMPP2M): 0 at the start of every run, 1 once a step of that kind
// has left its data prediction in the history buffer, 0 again behind a jump visit
__global__ void smp_set_state_kernel(int* st, int t, uint64_t seed) {
    st[0] = t;
    st[1] = 0;
    *reinterpret_cast<uint64_t*>(st + 2) = seed;
    st[5] = 0;
}

// a program run (dws_sampler_run_program) also keeps the visit number v in the state ([4]): the noise rows and Philox
// streams of a visit are indexed by v, the step table and the update tables by the step word [0] = step_of[v]
__global__ void smp_set_program_state_kernel(int* st, int t, int v, uint64_t seed) {
    st[0] = t;
    st[1] = 0;
    *reinterpret_cast<uint64_t*>(st + 2) = seed;
    st[4] = v;
    st[5] = 0;
}

// End of a step's kernel (thread 0 of every block, behind a __syncthreads): the last block to arrive moves the step index
// on (s <- s - 1).  Every block has read the state by then, and the next kernel that reads it is stream-ordered behind
// this one -- no separate one-thread launch per step.
// hist_valid >= 0: the new value of the history-valid word (1 behind a multistep step); the plain sampler's two-word
// state passes -1.
// Per-clip seeds (dws_sampler_set_clip_seeds).  A CLIP instance of a drawing kernel runs on a grid with one row per clip:
// row b works on elements b n_c .. (b + 1) n_c - 1 of every array with the Philox key seeds[b] and counts its groups of
// four from the start of the clip -- the launch a B = 1 run with the scalar seed seeds[b] makes, B times side by side
// (n_c = C L elements of a clip; the VEC form needs n_c % 4 == 0, so a group never straddles two clips).  The scalar
// instances (CLIP = false) read neither field and keep their code.
struct ClipSeeds {
    const uint64_t* seeds;       // device [B]
    size_t n_c;
};

// blocks of the whole grid: what the last-block counters below count up to
template <bool CLIP>
__device__ __forceinline__ unsigned smp_grid_blocks() {
    return CLIP ? gridDim.x * gridDim.y : gridDim.x;
}

__device__ __forceinline__ void smp_step_advance(int* __restrict__ st, int s, int hist_valid, unsigned blocks) {
    if (atomicAdd(reinterpret_cast<unsigned*>(st + 1), 1u) == blocks - 1) {
        st[1] = 0;
        st[0] = s - 1;
        if (hist_valid >= 0) st[5] = hist_valid;
    }
}

// The program flavour: the last block moves the program on, visit <- v - 1 and step <- step_of[v - 1] (the row the next
// visit's network reads; -1 behind the last visit).  hist_valid: 1 behind a multistep reverse visit, 0 behind a jump visit.
__device__ __forceinline__ void smp_program_advance(int* __restrict__ st, const int* __restrict__ step_of, int v,
                                                    int hist_valid, unsigned blocks) {
    if (atomicAdd(reinterpret_cast<unsigned*>(st + 1), 1u) == blocks - 1) {
        st[1] = 0;
        st[4] = v - 1;
        st[0] = v > 0 ? step_of[v - 1] : -1;
        if (hist_valid >= 0) st[5] = hist_valid;
    }
}

// Elements 4g .. 4g + 3 of p.  VEC: every group of 4 is in range and p is 16-byte aligned -> one float4; otherwise the
// elements below n one by one (v keeps its value for the others).
template <bool VEC>
__device__ __forceinline__ void smp_load4(const float* __restrict__ p, size_t g, size_t n, float v[4]) {
    if (VEC) {
        const float4 q = reinterpret_cast<const float4*>(p)[g];
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (g * 4 + j < n) v[j] = p[g * 4 + j];
    }
}

template <bool VEC>
__device__ __forceinline__ void smp_store4(float* __restrict__ p, size_t g, size_t n, const float v[4]) {
    if (VEC) {
        reinterpret_cast<float4*>(p)[g] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (g * 4 + j < n) p[g * 4 + j] = v[j];
    }
}

// The mask bytes of a group in one word: byte j is non-zero where element 4g + j is known.  VEC: one 32-bit load.
template <bool VEC>
__device__ __forceinline__ uint32_t smp_mask4(const uint8_t* __restrict__ mask, size_t g, size_t n) {
    if (VEC) return reinterpret_cast<const uint32_t*>(mask)[g];
    uint32_t mk = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (g * 4 + j < n && mask[g * 4 + j]) mk |= 1u << (8 * j);
    return mk;
}

// The arithmetic of the updates, one helper per formula.  Every product, difference, quotient and sum is rounded once, in
// the order written, to match the reference's op-by-op fp32 evaluation (`generate.py:52,54`): each helper switches
// contraction off for itself and uses plain operators -- that survives inlining, whereas the __f*_rn intrinsics are
// inline functions whose operations hipcc fused into FMAs after inlining (found by
// tests/test_sampler_gpu.py::test_step_table_sampler_equals_the_per_step_loop: 1 ulp on most elements once t > 0).

// DDPM: x <- (x - c1 eps) / c2  (+ sigma z if add)
__device__ __forceinline__ float smp_ddpm_elem(float x, float eps, float z, float c1, float c2, float sg, bool add) {
#pragma clang fp contract(off)
    const float p = c1 * eps;
    float v = (x - p) / c2;
    if (add) {
        const float q = sg * z;
        v = v + q;
    }
    return v;
}

// DDIM (Song et al., ICLR 2021, eq. 12) with k1 .. k5 of sampling.ddim_coefficients:
//   u = (x - k1 eps) / k2;  x = k3 u + k4 eps  (+ k5 z if add)
__device__ __forceinline__ float smp_ddim_elem(float x, float eps, float z, float k1, float k2, float k3, float k4,
                                               float k5, bool add) {
#pragma clang fp contract(off)
    const float p = k1 * eps;
    const float d = x - p;
    const float u = d / k2;
    const float a = k3 * u;
    const float b = k4 * eps;
    float v = a + b;
    if (add) {
        const float q = k5 * z;
        v = v + q;
    }
    return v;
}

// DPM-Solver++(2M) (Lu et al., 2022; the multistep solver in the data prediction) with m1 .. m5 of
// sampling.dpmpp_coefficients:
//   p = m1 eps;  d = x - p;  x0 = d / m2;  D = x0;  if second: g = x0 - hist; e = m5 g; D = x0 + e
//   a = m3 x;  b = m4 D;  v = a + b;  hist = x0
// Returns v and leaves x0 in `h`.  With second = false this is DDIM's step at eta = 0 written in the data prediction.
__device__ __forceinline__ float smp_dpmpp_elem(float x, float eps, float& h, float m1, float m2, float m3, float m4,
                                                float m5, bool second) {
#pragma clang fp contract(off)
    const float p = m1 * eps;
    const float d = x - p;
    const float x0 = d / m2;
    float D = x0;
    if (second) {
        const float g = x0 - h;
        const float e = m5 * g;
        D = x0 + e;
    }
    const float a = m3 * x;
    const float b = m4 * D;
    h = x0;
    return a + b;
}

// (a x) + (b z): the known-region replacement, the jump and the q-sample
__device__ __forceinline__ float smp_mix_elem(float a, float x, float b, float z) {
#pragma clang fp contract(off)
    const float p = a * x;
    const float q = b * z;
    return p + q;
}

// adaptive prior (dws_sampler_set_prior): n = sigma z, one product of its own; n then stands where z stood
__device__ __forceinline__ float smp_prior_elem(float sg, float z) {
#pragma clang fp contract(off)
    return sg * z;
}

// PRIOR instances of the drawing kernels: z <- sigma z over a group, sigma at the group's own positions of the table
// [B, C L] (the shape of the state, so it is indexed like x).  Injected and drawn numbers alike.
template <bool VEC>
__device__ __forceinline__ void smp_prior4(const float* __restrict__ prior, size_t g, size_t n, float z[4]) {
    float sg[4] = {0.f, 0.f, 0.f, 0.f};
    smp_load4<VEC>(prior, g, n, sg);
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = smp_prior_elem(sg[j], z[j]);
}

// classifier-free guidance: eps_c + scale (eps_c - eps_u)
__device__ __forceinline__ float smp_cfg_elem(float c, float u, float scale) {
#pragma clang fp contract(off)
    const float d = c - u;
    const float gd = scale * d;
    return c + gd;
}

// PRIOR: x = sigma z with prior [n] (the drawn x_T of a run with an adaptive prior).
template <bool PRIOR>
__global__ void smp_fill_normal_kernel(float* __restrict__ x, size_t n, uint64_t seed, uint32_t stream_id,
                                       const float* __restrict__ prior) {
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n; g += (size_t)gridDim.x * blockDim.x) {
        float z[4];
        normal4(seed, stream_id, g, z);
        if (PRIOR) smp_prior4<false>(prior, g, n, z);
        smp_store4<false>(x, g, n, z);
    }
}

// The per-clip twin: row b = blockIdx.y of x [B, n_c] is smp_fill_normal_kernel(x + b n_c, n_c, seeds[b], stream_id).
// SEEDS: the model's device table, or a chunk of host seeds travelling by value (dws_philox_normal_clips).
struct SeedChunk {
    static constexpr int N = 64;
    uint64_t s[N];
    __device__ uint64_t operator[](unsigned b) const { return s[b]; }
};

template <class SEEDS, bool PRIOR>
__global__ void smp_fill_normal_clips_kernel(float* __restrict__ x, size_t n_c, const SEEDS seeds, uint32_t stream_id,
                                             const float* __restrict__ prior) {
    const uint64_t seed = seeds[blockIdx.y];
    x += (size_t)blockIdx.y * n_c;
    if (PRIOR) prior += (size_t)blockIdx.y * n_c;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n_c; g += (size_t)gridDim.x * blockDim.x) {
        float z[4];
        normal4(seed, stream_id, g, z);
        if (PRIOR) smp_prior4<false>(prior, g, n_c, z);
        smp_store4<false>(x, g, n_c, z);
    }
}

// The full-T sampler's update (dws_sampler_run / dws_sampler_steps) and the plain DDPM kind of the schedule sampler:
// smp_ddpm_elem at step t = *t_dev with tables [3][T] = c1, c2, sigma; z: noise[t] or Philox (seed, t).
// seed_dev non-null (few-step sampler): the Philox seed is read from device memory instead of `seed`.
// CLIP (schedule sampler only): n_all elements in all, this grid row's clip with its own seed (ClipSeeds).
// PRIOR (schedule sampler only): z <- prior z, prior [n_all] (dws_sampler_set_prior).
template <bool CLIP, bool PRIOR>
__global__ void smp_update_kernel(float* __restrict__ x, const float* __restrict__ eps,
                                  const float* __restrict__ tables, int* __restrict__ t_dev,
                                  const float* __restrict__ noise, uint64_t seed, const uint64_t* seed_dev, size_t n_all,
                                  int T, const ClipSeeds cs, const float* __restrict__ prior) {
    const int t = __builtin_amdgcn_readfirstlane(*(volatile int*)t_dev);
    if (CLIP) seed = cs.seeds[blockIdx.y];
    else if (seed_dev) seed = *(const volatile uint64_t*)seed_dev;
    const float c1 = tables[t], c2 = tables[T + t], sg = tables[2 * T + t];
    const float* nz = noise ? noise + (size_t)t * n_all : nullptr;
    const size_t n = CLIP ? cs.n_c : n_all;
    if (CLIP) {
        const size_t off = (size_t)blockIdx.y * cs.n_c;
        x += off; eps += off;
        if (nz) nz += off;
        if (PRIOR) prior += off;
    }
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n; g += (size_t)gridDim.x * blockDim.x) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (t > 0 && !nz) normal4(seed, (uint32_t)t, g, z);
        if (PRIOR && t > 0) {
            if (nz) smp_load4<false>(nz, g, n, z);
            smp_prior4<false>(prior, g, n, z);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t i = g * 4 + j;
            if (i >= n) break;
            x[i] = smp_ddpm_elem(x[i], eps[i], !PRIOR && t > 0 && nz ? nz[i] : z[j], c1, c2, sg, t > 0);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) smp_step_advance(t_dev, t, -1, smp_grid_blocks<CLIP>());
}

// One update of the schedule sampler (dws_sampler_run_schedule / _edit / _program), every flavour of it:
//   KIND  the arithmetic at step s = st[0] with tab = c1, c2, sigma (DDPM), k1 .. k5 (DDIM) or m1 .. m5 (DPM-Solver++(2M)).
//         z: noise[v] or Philox stream v in normal4's layout; the seed comes from the state (st + 2).  The multistep kind
//         draws no update noise; hist [B, C, L] carries its previous x0 across the replays, read only when
//         second = (history-valid word st[5] != 0) && m5[s] != 0 and written by every step.
//   EDIT  inpainting by replacement (Song et al., ICLR 2021, "imputation"; the base case of RePaint): where mask != 0 the
//         element is then overwritten with the known audio y noised to the level the state is at after step s,
//           v = (s > 0) ? (q1[s] * y) + (q2[s] * zk) : y          edit = q1[S], q2[S] (sampling.edit_coefficients)
//         zk: known_noise[v] or Philox stream R + 1 + v, drawn only for groups that hold a known element (no other
//         element reads it).  hist gets the network's prediction x0, before the replacement.
//   PROG  a reverse visit of a program (RePaint's resampling): the visit number v = st[4] names the noise rows and the
//         streams, with R = V (a step that is visited again draws fresh noise), and the last block moves the program on.
//         Otherwise v = s, R = S and the last block counts the step down.
//   VEC   every group of 4 is in range and all pointers are 16-byte aligned -> float4 for the floats and the four mask
//         bytes of a group as one 32-bit load.
//   CLIP  per-clip seeds (ClipSeeds above): the grid row's clip of every array, its seed in the place of the state's.
//   PRIOR adaptive prior (dws_sampler_set_prior): z and zk, injected or drawn, are multiplied by prior [B, C L] at their
//         own positions (smp_prior_elem) before the update reads them.  The other instances never load the field.
// What every flavour reads travels as plain kernel arguments, the rest in one by-value struct whose fields a flavour
// that does not need them never loads.  (Plain arguments are fetched ahead of the ordered reads of the state, fields of a
// struct only behind them; this way the plain DDIM instance is, instruction for instruction, the kernel it took over from.)
struct StepMore {
    float* hist;                 // DWS_SAMPLER_DPMPP2M
    const float* edit;           // EDIT ...
    const float* y;
    const uint8_t* mask;
    const float* known_noise;
    const int* step_of;          // PROG ...
    int V;
    ClipSeeds clip;              // CLIP
    const float* prior;          // PRIOR
};

struct StepArgs {
    float* x;
    const float* eps;
    const float* tab;
    int* st;
    const float* noise;
    size_t n;
    int S;
    int clips;                   // grid rows of a per-clip launch (0: the scalar-seed instances)
    StepMore more;
};

template <int KIND, bool EDIT, bool PROG, bool VEC, bool CLIP, bool PRIOR>
__global__ void smp_step_kernel(float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ tab,
                                int* __restrict__ st, const float* __restrict__ noise, size_t n_all, int S,
                                const StepMore m) {
    constexpr bool MULTI = KIND == DWS_SAMPLER_DPMPP2M;
    const int s = __builtin_amdgcn_readfirstlane(*(volatile int*)st);
    const int v = PROG ? __builtin_amdgcn_readfirstlane(*(volatile int*)(st + 4)) : s;
    const int R = PROG ? m.V : S;
    const uint64_t seed = !(!MULTI || EDIT) ? 0 : CLIP ? m.clip.seeds[blockIdx.y] : *(const volatile uint64_t*)(st + 2);
    const int valid = MULTI ? __builtin_amdgcn_readfirstlane(*(volatile int*)(st + 5)) : 0;
    const float k1 = tab[s], k2 = tab[S + s], k3 = tab[2 * S + s];
    const float k4 = KIND != DWS_SAMPLER_DDPM ? tab[3 * S + s] : 0.f, k5 = KIND != DWS_SAMPLER_DDPM ? tab[4 * S + s] : 0.f;
    const bool add = MULTI ? false : KIND == DWS_SAMPLER_DDIM ? (s > 0 && k5 > 0.f) : s > 0;
    const bool second = MULTI && valid != 0 && k5 != 0.f;
    const float q1 = EDIT ? m.edit[s] : 0.f, q2 = EDIT ? m.edit[S + s] : 0.f;
    const float* nz = noise ? noise + (size_t)v * n_all : nullptr;
    const float* kz = EDIT && m.known_noise ? m.known_noise + (size_t)v * n_all : nullptr;
    // the rows of every array this block works on: all of them, or (CLIP) those of its grid row's clip
    const size_t n = CLIP ? m.clip.n_c : n_all;
    const size_t off = CLIP ? (size_t)blockIdx.y * m.clip.n_c : 0;
    float* hist = MULTI ? m.hist + off : nullptr;
    const float* y = EDIT ? m.y + off : nullptr;
    const uint8_t* mask = EDIT ? m.mask + off : nullptr;
    const float* prior = PRIOR ? m.prior + off : nullptr;
    if (CLIP) {
        x += off; eps += off;
        if (nz) nz += off;
        if (kz) kz += off;
    }
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n; g += (size_t)gridDim.x * blockDim.x) {
        float xv[4] = {0.f, 0.f, 0.f, 0.f}, ev[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f};
        float yv[4] = {0.f, 0.f, 0.f, 0.f}, zk[4] = {0.f, 0.f, 0.f, 0.f}, hv[4] = {0.f, 0.f, 0.f, 0.f};
        smp_load4<VEC>(x, g, n, xv);
        smp_load4<VEC>(eps, g, n, ev);
        if (add && nz) smp_load4<VEC>(nz, g, n, z);
        if (second) smp_load4<VEC>(hist, g, n, hv);
        const uint32_t mk = EDIT ? smp_mask4<VEC>(mask, g, n) : 0;
        if (mk) {
            smp_load4<VEC>(y, g, n, yv);
            if (s > 0 && kz) smp_load4<VEC>(kz, g, n, zk);
        }
        if (add && !nz) normal4(seed, (uint32_t)v, g, z);
        if (mk && s > 0 && !kz) normal4(seed, (uint32_t)(R + 1 + v), g, zk);
        if (PRIOR && (add || (mk && s > 0))) {
            float sg[4] = {0.f, 0.f, 0.f, 0.f};
            smp_load4<VEC>(prior, g, n, sg);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                z[j] = smp_prior_elem(sg[j], z[j]);
                zk[j] = smp_prior_elem(sg[j], zk[j]);
            }
        }
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (MULTI) r[j] = smp_dpmpp_elem(xv[j], ev[j], hv[j], k1, k2, k3, k4, k5, second);     // hv[j] <- x0
            else if (KIND == DWS_SAMPLER_DDIM) r[j] = smp_ddim_elem(xv[j], ev[j], z[j], k1, k2, k3, k4, k5, add);
            else r[j] = smp_ddpm_elem(xv[j], ev[j], z[j], k1, k2, k3, add);
            if ((mk >> (8 * j)) & 0xffu) {
                r[j] = yv[j];
                if (s > 0) r[j] = smp_mix_elem(q1, yv[j], q2, zk[j]);
            }
        }
        smp_store4<VEC>(x, g, n, r);
        if (MULTI) smp_store4<VEC>(hist, g, n, hv);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (PROG) smp_program_advance(st, m.step_of, v, MULTI ? 1 : -1, smp_grid_blocks<CLIP>());
        else smp_step_advance(st, s, MULTI ? 1 : -1, smp_grid_blocks<CLIP>());
    }
}

// Jump visit of dws_sampler_run_program: the whole state, known region included, goes from position k up to k + j in one
// draw of the forward process' exact marginal q(x_{k+j} | x_k),
//   x = (ja * x) + (jb * z)      ja = jump[v], jb = jump[V + v] (sampling.jump_coefficients)
// z: noise[v] or Philox stream v in normal4's layout.  No network runs.  The jump re-noises the state, so the last block
// also clears the history-valid word: the multistep kind's next step is first order.
template <bool VEC, bool CLIP, bool PRIOR>
__global__ void smp_jump_kernel(float* __restrict__ x, const float* __restrict__ jump, int* __restrict__ st,
                                const int* __restrict__ step_of, const float* __restrict__ noise, size_t n_all, int V,
                                const ClipSeeds cs, const float* __restrict__ prior) {
    const int v = __builtin_amdgcn_readfirstlane(*(volatile int*)(st + 4));
    const uint64_t seed = CLIP ? cs.seeds[blockIdx.y] : *(const volatile uint64_t*)(st + 2);
    const float ja = jump[v], jb = jump[V + v];
    const float* nz = noise ? noise + (size_t)v * n_all : nullptr;
    const size_t n = CLIP ? cs.n_c : n_all;
    if (CLIP) {
        const size_t off = (size_t)blockIdx.y * cs.n_c;
        x += off;
        if (nz) nz += off;
        if (PRIOR) prior += off;
    }
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n; g += (size_t)gridDim.x * blockDim.x) {
        float xv[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f};
        smp_load4<VEC>(x, g, n, xv);
        if (nz) smp_load4<VEC>(nz, g, n, z);
        else normal4(seed, (uint32_t)v, g, z);
        if (PRIOR) smp_prior4<VEC>(prior, g, n, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = smp_mix_elem(ja, xv[j], jb, z[j]);
        smp_store4<VEC>(x, g, n, xv);
    }
    __syncthreads();
    if (threadIdx.x == 0) smp_program_advance(st, step_of, v, 0, smp_grid_blocks<CLIP>());
}

// Partial start in q-sample mode: x holds clean audio and becomes the state at step s0,
//   x = (n1 * x) + (n2 * z0)      n1 = sqrt(level[s0]), n2 = sqrt(1 - level[s0])
// z0: the injected tensor or Philox stream `stream_id` (2S + 1).
template <bool CLIP, bool PRIOR>
__global__ void smp_qsample_kernel(float* __restrict__ x, const float* __restrict__ z0, float n1, float n2, size_t n_all,
                                   uint64_t seed, uint32_t stream_id, const ClipSeeds cs, const float* __restrict__ prior) {
    const size_t n = CLIP ? cs.n_c : n_all;
    if (CLIP) {
        const size_t off = (size_t)blockIdx.y * cs.n_c;
        seed = cs.seeds[blockIdx.y];
        x += off;
        if (z0) z0 += off;
        if (PRIOR) prior += off;
    }
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n; g += (size_t)gridDim.x * blockDim.x) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (!z0) normal4(seed, stream_id, g, z);
        if (PRIOR) {
            if (z0) smp_load4<false>(z0, g, n, z);
            smp_prior4<false>(prior, g, n, z);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t i = g * 4 + j;
            if (i >= n) break;
            x[i] = smp_mix_elem(n1, x[i], n2, !PRIOR && z0 ? z0[i] : z[j]);
        }
    }
}

// Classifier-free guidance (Ho & Salimans, 2021) between the network and the update of a guided step: eps [2 n] holds the
// network output of the doubled state, the conditional half first; the first half becomes smp_cfg_elem of the two.  scale
// is word 6 of the sampler state (a float), so a new scale replays the captured step.
__global__ void smp_set_cfg_scale_kernel(int* st, float scale) { reinterpret_cast<float*>(st)[6] = scale; }

template <bool VEC>
__global__ void smp_cfg_kernel(float* __restrict__ eps, const int* __restrict__ st, size_t n) {
    const float scale = *reinterpret_cast<const volatile float*>(st + 6);
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n; g += (size_t)gridDim.x * blockDim.x) {
        float c[4] = {0.f, 0.f, 0.f, 0.f}, u[4] = {0.f, 0.f, 0.f, 0.f};
        smp_load4<VEC>(eps, g, n, c);
        smp_load4<VEC>(eps + n, g, n, u);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = smp_cfg_elem(c[j], u[j], scale);
        smp_store4<VEC>(eps, g, n, c);
    }
}

// ---- host side: what the entry points share ----
static int smp_blocks(size_t n) { return (int)std::min<size_t>(ceil_div(n, 4 * 256), 4096); }

// The grid of a launch over n elements: smp_blocks(n), or -- per-clip seeds, `clips` > 0 rows of n_c elements -- a row of
// blocks per clip with about as many blocks in all.
static dim3 smp_grid(size_t n, int clips, size_t n_c) {
    if (clips == 0) return dim3(smp_blocks(n));
    const size_t per_clip = std::max<size_t>(4096 / (size_t)clips, 1);
    return dim3((unsigned)std::min<size_t>(ceil_div(n_c, 4 * 256), per_clip), (unsigned)clips);
}

// KIND and VEC of a launch as compile-time constants: f(integral_constant<int, kind>, bool_constant<vec>)
template <class F>
static void smp_dispatch(int kind, bool vec, F&& f) {
    const auto with_vec = [&](auto K) {
        if (vec) f(K, std::true_type{});
        else f(K, std::false_type{});
    };
    if (kind == DWS_SAMPLER_DDPM) with_vec(std::integral_constant<int, DWS_SAMPLER_DDPM>{});
    else if (kind == DWS_SAMPLER_DPMPP2M) with_vec(std::integral_constant<int, DWS_SAMPLER_DPMPP2M>{});
    else with_vec(std::integral_constant<int, DWS_SAMPLER_DDIM>{});
}

// The plain flavour has no DDPM instance: that kind's unedited step is smp_update_kernel.
template <bool EDIT, bool PROG>
static void smp_launch_step(int kind, bool vec, const StepArgs& a, hipStream_t s) {
    const dim3 grid = smp_grid(a.n, a.clips, a.more.clip.n_c);
    smp_dispatch(kind, vec, [&](auto K, auto VEC) {
        if constexpr (EDIT || decltype(K)::value != DWS_SAMPLER_DDPM) {
            const auto launch = [&](auto CLIP, auto PRIOR) {
                hipLaunchKernelGGL((smp_step_kernel<decltype(K)::value, EDIT, PROG, decltype(VEC)::value,
                                                    decltype(CLIP)::value, decltype(PRIOR)::value>),
                                   grid, dim3(256), 0, s, a.x, a.eps, a.tab, a.st, a.noise, a.n, a.S, a.more);
            };
            // (the multistep kind draws no update noise: unedited, its prior instance would be the plain one, and is not built)
            constexpr bool HAS_PRIOR = EDIT || decltype(K)::value != DWS_SAMPLER_DPMPP2M;
            bool prior = false;
            if constexpr (HAS_PRIOR) {
                prior = a.more.prior != nullptr;
                if (prior && a.clips) launch(std::true_type{}, std::true_type{});
                else if (prior) launch(std::false_type{}, std::true_type{});
            }
            if (prior) return;
            if (a.clips) launch(std::true_type{}, std::false_type{});
            else launch(std::false_type{}, std::false_type{});
        }
    });
}

// The caller's stream may be the legacy null stream, which cannot be captured: capture and replay on an engine-owned
// stream (*engine) that is ordered after / before the caller's stream with events.
static int engine_after_caller(dws_model* m, hipStream_t s, hipStream_t* engine) {
    DWS_TRY(m->smp.stream.get(engine));
    DWS_TRY(m->smp.ev_in.record(s));
    return m->smp.ev_in.make_wait(*engine);
}

static int caller_after_engine(dws_model* m, hipStream_t s) {
    DWS_TRY(m->smp.ev_out.record(m->smp.stream.s));
    return m->smp.ev_out.make_wait(s);
}

// `exec` becomes the graph of one step: kept when `reuse` says the held one still fits, otherwise captured from what
// `step` enqueues on cs (the stale one is destroyed first; a failing step returns its status and leaves exec null).
template <class Step>
static int capture_step(dws_model* m, hipStream_t cs, hipGraphExec_t& exec, bool reuse, Step&& step) {
    if (exec && reuse) return DWS_OK;
    if (exec) hipGraphExecDestroy(exec);
    exec = nullptr;
    hipGraph_t graph = nullptr;
    DWS_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    const int rc = step();
    hipError_t err = hipStreamEndCapture(cs, &graph);
    if (rc != DWS_OK) {
        if (graph) hipGraphDestroy(graph);
        return rc;
    }
    DWS_HIP(err);
    err = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    DWS_HIP(err);
    ++m->smp.graphs_made;
    return DWS_OK;
}

// Per-clip lengths (dws_model_set_lengths): behind the last step of a run the returned state holds exactly 0.0f past
// every clip's own end.  The steps need nothing: the update is pointwise and the network seals its own padding.
static int seal_result(dws_model* m, float* x, hipStream_t s) {
    if (!m->ragged()) return DWS_OK;
    return launch_wn_mask_tail(x, m->lengths_ptr(), (int)m->B, m->d.out_channels, (int)m->L, -1, nullptr, 0, nullptr, 0, s);
}

// c1 = (1 - alpha) / sqrt(1 - alpha_bar), c2 = sqrt(alpha), sigma: [3][T]
static std::vector<float> ddpm_table(const float* alpha, const float* alpha_bar, const float* sigma, int T) {
    std::vector<float> h(3 * (size_t)T);
    for (int t = 0; t < T; ++t) {
        // fp32 scalar arithmetic in the reference's order (`generate.py:52`)
        const float one_m_a = 1.0f - alpha[t];
        const float den = sqrtf(1.0f - alpha_bar[t]);
        h[t] = one_m_a / den;
        h[T + t] = sqrtf(alpha[t]);
        h[2 * T + t] = sigma[t];
    }
    return h;
}

// ---- the full-T sampler (dws_sampler_run / dws_sampler_steps) ----
static int upload_tables(dws_model* m, const float* alpha, const float* alpha_bar, const float* sigma, int T,
                         hipStream_t s) {
    const std::vector<float> h = ddpm_table(alpha, alpha_bar, sigma, T);
    DWS_TRY(m->smp.state.ensure(8));
    return upload_if_changed(m->smp.tables, m->smp.host_tables, h.data(), h.size(), s);
}

static int one_step(dws_model* m, float* x, const float* noise, uint64_t seed, int T, hipStream_t s) {
    const size_t n = (size_t)m->B * m->d.out_channels * m->L;
    int* t_dev = static_cast<int*>(m->smp.state.p);
    // every clip is at step t (`generate.py:50`): the network reads row t of the step table built at sampler entry
    m->step_idx = t_dev;
    const int st = m->forward(x, nullptr, m->smp.eps.f(), s);
    m->step_idx = nullptr;
    DWS_TRY(st);
    hipLaunchKernelGGL((smp_update_kernel<false, false>), dim3(smp_blocks(n)), dim3(256), 0, s, x, m->smp.eps.f(),
                       m->smp.tables.f(), t_dev, noise, seed, (const uint64_t*)nullptr, n, T, ClipSeeds{}, (const float*)nullptr);
    return DWS_OK;
}

static int run_steps(dws_model* m, float* x, int T, int t_start, int n_steps, const float* noise, uint64_t seed,
                     int use_graph, hipStream_t s) {
    DWS_CHECK(m->B > 0, DWS_ERR_STATE, "sampler before dws_model_prepare");
    DWS_CHECK(m->d.in_channels == m->d.out_channels, DWS_ERR_INVALID,
              "sampler needs in_channels == out_channels (x and eps share a shape, `generate.py:52`)");
    DWS_CHECK(t_start < T && n_steps >= 0 && t_start - n_steps >= -1, DWS_ERR_INVALID, "bad step range");
    if (m->dirty) DWS_TRY(m->commit(s));
    const size_t n = (size_t)m->B * m->d.out_channels * m->L;
    DWS_TRY(m->smp.eps.ensure(n * 4));
    m->smp.eps_B = m->B; m->smp.eps_L = m->L;
    DWS_TRY(m->build_step_table(T, nullptr, s));   // step-only part of the network for t = 0..T-1 (kept while weights and T stay)
    int* t_dev = static_cast<int*>(m->smp.state.p);

    if (!use_graph) {
        hipLaunchKernelGGL(smp_set_step_kernel, dim3(1), dim3(1), 0, s, t_dev, t_start);
        for (int i = 0; i < n_steps; ++i) DWS_TRY(one_step(m, x, noise, seed, T, s));
        DWS_TRY(seal_result(m, x, s));
        DWS_HIP(hipGetLastError());
        return DWS_OK;
    }
    hipStream_t cs = nullptr;
    DWS_TRY(engine_after_caller(m, s, &cs));
    hipLaunchKernelGGL(smp_set_step_kernel, dim3(1), dim3(1), 0, cs, t_dev, t_start);
    const bool reuse = m->smp.graph && m->smp.g_B == m->B && m->smp.g_L == m->L && m->smp.g_T == T && m->smp.g_x == x &&
                       m->smp.g_noise == noise && m->smp.g_seed == seed && m->smp.g_ragged == m->ragged();
    if (!reuse) m->drop_graph();    // this step bakes in x, the noise and the seed: a new one retires every held graph
    DWS_TRY(capture_step(m, cs, m->smp.graph, reuse, [&] { return one_step(m, x, noise, seed, T, cs); }));
    m->smp.g_B = m->B; m->smp.g_L = m->L; m->smp.g_T = T; m->smp.g_x = x; m->smp.g_noise = noise; m->smp.g_seed = seed;
    m->smp.g_ragged = m->ragged();
    for (int i = 0; i < n_steps; ++i) DWS_HIP(hipGraphLaunch(m->smp.graph, cs));
    DWS_TRY(seal_result(m, x, cs));
    return caller_after_engine(m, s);
}

int sampler_run(dws_model* m, float* x, const float* alpha, const float* alpha_bar, const float* sigma, int T,
                const float* noise, uint64_t seed, int init_from_seed, int use_graph, hipStream_t s) {
    DWS_CHECK(T > 0 && alpha && alpha_bar && sigma, DWS_ERR_INVALID, "sampler: bad schedule tables");
    DWS_TRY(upload_tables(m, alpha, alpha_bar, sigma, T, s));
    if (init_from_seed) {
        const size_t n = (size_t)m->B * m->d.in_channels * m->L;
        hipLaunchKernelGGL(smp_fill_normal_kernel<false>, dim3(smp_blocks(n)), dim3(256), 0, s, x, n, seed, (uint32_t)T,
                           (const float*)nullptr);
    }
    return run_steps(m, x, T, T - 1, T, noise, seed, use_graph, s);
}

int sampler_steps(dws_model* m, float* x, const float* alpha, const float* alpha_bar, const float* sigma, int T,
                  int t_start, int n_steps, uint64_t seed, int use_graph, hipStream_t s) {
    DWS_CHECK(T > 0 && alpha && alpha_bar && sigma, DWS_ERR_INVALID, "sampler: bad schedule tables");
    // re-uploaded only when the coefficients differ from the resident ones (3T host flops per call)
    DWS_TRY(upload_tables(m, alpha, alpha_bar, sigma, T, s));
    return run_steps(m, x, T, t_start, n_steps, nullptr, seed, use_graph, s);
}

// ---- few-step samplers (dws_sampler_run_schedule) and their editing modes (dws_sampler_run_edit) ----
// host side of a program: visit_step[V] in execution order, jump_coef[2][V] indexed by the visit number
struct SamplerProgram {
    int V;
    const int32_t* visit_step;
    const float* jump_coef;
};

// One reverse step of the schedule: forward at row *st of the step table, then the update `a` describes -- with the
// replacement of the known region when a.more.mask is given, as a visit of a program when a.more.step_of is given too.
// cfg (neither): a.x is the doubled state [2 Bc, C, L] and a.n the elements of its first half; the guided eps of the first
// half, the update over the first half alone and the mirror of the first half of the state into the second -- one
// linear chain.
static int schedule_step(dws_model* m, int kind, bool vec, const StepArgs& a, bool cfg, hipStream_t s) {
    m->step_idx = a.st;
    const int rc = m->forward(a.x, nullptr, m->smp.eps.f(), s);
    m->step_idx = nullptr;
    DWS_TRY(rc);
    if (cfg) {
        ProfileScope prof("smp_cfg", s);
        if (vec) hipLaunchKernelGGL(smp_cfg_kernel<true>, dim3(smp_blocks(a.n)), dim3(256), 0, s, m->smp.eps.f(), a.st, a.n);
        else hipLaunchKernelGGL(smp_cfg_kernel<false>, dim3(smp_blocks(a.n)), dim3(256), 0, s, m->smp.eps.f(), a.st, a.n);
    }
    // dws_profile_enable("smp_update"): the update kernel of an uncaptured step, by kind
    ProfileScope prof(kind == DWS_SAMPLER_DDPM ? "smp_update_ddpm" : kind == DWS_SAMPLER_DDIM ? "smp_update_ddim"
                                                                                             : "smp_update_dpmpp2m", s);
    if (a.more.mask && a.more.step_of)
        smp_launch_step<true, true>(kind, vec, a, s);
    else if (a.more.mask)
        smp_launch_step<true, false>(kind, vec, a, s);
    else if (kind == DWS_SAMPLER_DDPM) {
        const dim3 grid = smp_grid(a.n, a.clips, a.more.clip.n_c);
        const uint64_t* seed_dev = a.clips ? nullptr : reinterpret_cast<const uint64_t*>(a.st + 2);
        const ClipSeeds cs = a.clips ? a.more.clip : ClipSeeds{};
        const auto launch = [&](auto CLIP, auto PRIOR) {
            hipLaunchKernelGGL((smp_update_kernel<decltype(CLIP)::value, decltype(PRIOR)::value>), grid, dim3(256), 0, s, a.x,
                               a.eps, a.tab, a.st, a.noise, (uint64_t)0, seed_dev, a.n, a.S, cs, a.more.prior);
        };
        if (a.clips && a.more.prior) launch(std::true_type{}, std::true_type{});
        else if (a.clips) launch(std::true_type{}, std::false_type{});
        else if (a.more.prior) launch(std::false_type{}, std::true_type{});
        else launch(std::false_type{}, std::false_type{});
    }
    else
        smp_launch_step<false, false>(kind, vec, a, s);
    if (cfg) DWS_HIP(hipMemcpyAsync(a.x + a.n, a.x, a.n * 4, hipMemcpyDeviceToDevice, s));   // the second half of the state follows the first
    return DWS_OK;
}

// e null: dws_sampler_run_schedule.  e given: dws_sampler_run_edit -- the run starts at e->start_step (the initial value
// of the device step counter, and the number of replays), optionally from a q-sample of x, and with `known` / `mask`
// every step ends in the replacement of the known region (the edited step, a graph of its own).
// pg given (with e, known and mask; checked by sampler_run_program): the host walks the program's V visits in order, a
// reverse visit as a replay of the resampling step (a third graph), a jump visit as a launch of smp_jump_kernel; the
// noise rows and Philox streams are numbered by the visit with V in the place of S.
int sampler_run_schedule(dws_model* m, float* x, int kind, int S, const float* net_steps, const float* coef,
                         const float* noise, uint64_t seed, int init_from_seed, int use_graph,
                         const dws_sampler_edit* e, const SamplerProgram* pg, hipStream_t s) {
    DWS_CHECK(kind == DWS_SAMPLER_DDPM || kind == DWS_SAMPLER_DDIM || kind == DWS_SAMPLER_DPMPP2M, DWS_ERR_INVALID,
              "sampler: unknown kind %d", kind);
    DWS_CHECK(S >= 1, DWS_ERR_INVALID, "sampler: S = %d steps (needs S >= 1)", S);
    DWS_CHECK(net_steps && coef, DWS_ERR_INVALID, "sampler: null net_steps or coefficients");
    for (int i = 0; i < S; ++i)
        DWS_CHECK(std::isfinite(net_steps[i]), DWS_ERR_INVALID, "sampler: net_steps[%d] = %g is not finite", i,
                  (double)net_steps[i]);
    const int rows = kind == DWS_SAMPLER_DDPM ? 3 : 5;
    for (int i = 0; i < rows * S; ++i)
        DWS_CHECK(std::isfinite(coef[i]), DWS_ERR_INVALID, "sampler: coefficient row %d, step %d = %g is not finite",
                  i / S, i % S, (double)coef[i]);
    if (kind == DWS_SAMPLER_DDIM)
        for (int i = 0; i < S; ++i)
            DWS_CHECK(coef[S + i] > 0.f, DWS_ERR_INVALID, "sampler: DDIM k2[%d] = %g (needs k2 > 0)", i, (double)coef[S + i]);
    if (kind == DWS_SAMPLER_DPMPP2M) {
        for (int i = 0; i < S; ++i) {
            DWS_CHECK(coef[S + i] > 0.f, DWS_ERR_INVALID, "sampler: DPM-Solver++ m2[%d] = %g (needs m2 > 0)", i,
                      (double)coef[S + i]);
            DWS_CHECK(coef[4 * (size_t)S + i] >= 0.f, DWS_ERR_INVALID, "sampler: DPM-Solver++ m5[%d] = %g (needs m5 >= 0)", i,
                      (double)coef[4 * (size_t)S + i]);
        }
        DWS_CHECK(!noise || pg, DWS_ERR_INVALID,
                  "sampler: DPM-Solver++ is deterministic; noise is read only by the jump visits of a program run");
    }
    const int start = e ? e->start_step : S - 1;
    const bool masked = e && e->known && e->mask;
    const bool qsample = e && e->start_mode == DWS_START_QSAMPLE;
    if (e) {
        DWS_CHECK(start >= 0 && start < S, DWS_ERR_INVALID, "sampler: start_step = %d (needs 0 .. %d)", start, S - 1);
        DWS_CHECK((e->known != nullptr) == (e->mask != nullptr), DWS_ERR_INVALID,
                  "sampler: known and mask come together (got %s only)", e->known ? "known" : "mask");
        DWS_CHECK(!e->known_noise || masked, DWS_ERR_INVALID, "sampler: known_noise without known / mask");
        DWS_CHECK(e->start_mode == DWS_START_AS_GIVEN || e->start_mode == DWS_START_QSAMPLE, DWS_ERR_INVALID,
                  "sampler: unknown start mode %d", e->start_mode);
        DWS_CHECK(!e->start_noise || qsample, DWS_ERR_INVALID, "sampler: start_noise without the q-sample start mode");
        DWS_CHECK(e->edit_coef, DWS_ERR_INVALID, "sampler: null edit coefficients");
        for (int i = 0; i < 4 * S; ++i)
            DWS_CHECK(std::isfinite(e->edit_coef[i]), DWS_ERR_INVALID,
                      "sampler: edit coefficient row %d, step %d = %g is not finite", i / S, i % S, (double)e->edit_coef[i]);
        DWS_CHECK(!(qsample && init_from_seed), DWS_ERR_INVALID,
                  "sampler: the q-sample start noises the given x; it cannot be combined with init_from_seed");
        DWS_CHECK(!init_from_seed || start == S - 1, DWS_ERR_INVALID,
                  "sampler: init_from_seed draws x_T, the state of step S-1 = %d (start_step = %d)", S - 1, start);
    }
    DWS_CHECK(m->B > 0, DWS_ERR_STATE, "sampler before dws_model_prepare");
    DWS_CHECK(m->d.in_channels == m->d.out_channels, DWS_ERR_INVALID,
              "sampler needs in_channels == out_channels (x and eps share a shape, `generate.py:52`)");
    const bool cfg = m->smp.cfg_on;
    DWS_CHECK(!cfg || (!e && !pg), DWS_ERR_UNSUPPORTED, "classifier-free guidance is not built for editing or program runs");
    DWS_CHECK(!cfg || m->B % 2 == 0, DWS_ERR_UNSUPPORTED,
              "classifier-free guidance needs a model prepared for 2 x Bc clips (prepared batch: %lld)", (long long)m->B);
    // per-clip seeds: one per clip of the sampler state (the first half of a guided run's doubled batch); `seed` is not read
    const int clips = (int)m->smp.clip_B;
    DWS_CHECK(clips == 0 || clips == (cfg ? m->B / 2 : m->B), DWS_ERR_INVALID,
              "sampler: a table of %d clip seeds (dws_sampler_set_clip_seeds) for a sampler state of %lld clips", clips,
              (long long)(cfg ? m->B / 2 : m->B));
    // adaptive prior: a table at the shape of the sampler state; every noise site below scales its z by it
    DWS_CHECK(!cfg || !m->smp.prior_on, DWS_ERR_UNSUPPORTED,
              "classifier-free guidance with an adaptive prior (dws_sampler_set_prior) is not built");
    DWS_CHECK(!m->smp.prior_on || (m->smp.prior_B == m->B && m->smp.prior_n == m->d.out_channels * m->L), DWS_ERR_INVALID,
              "sampler: a prior table of [%lld, %lld] (dws_sampler_set_prior) for a sampler state of [%lld, %lld]",
              (long long)m->smp.prior_B, (long long)m->smp.prior_n, (long long)m->B, (long long)(m->d.out_channels * m->L));
    const float* prior = m->smp.prior_on ? m->smp.prior.f() : nullptr;
    if (m->dirty) DWS_TRY(m->commit(s));
    const size_t nfull = (size_t)m->B * m->d.out_channels * m->L;    // the network's batch
    const size_t n = cfg ? nfull / 2 : nfull;                         // what the caller's x, the noise and the update span
    const ClipSeeds clip{clips ? static_cast<const uint64_t*>(m->smp.clip_seeds.p) : nullptr,
                         clips ? (size_t)m->d.out_channels * m->L : 0};

    // update tables, keyed on their contents; DDIM's and DPM-Solver++'s are used as given
    const std::vector<float> h = kind != DWS_SAMPLER_DDPM ? std::vector<float>(coef, coef + 5 * (size_t)S)
                                                          : ddpm_table(coef, coef + S, coef + 2 * (size_t)S, S);
    DWS_TRY(upload_if_changed(m->smp.sch_tables, m->smp.sch_host_tables, h.data(), h.size(), s));
    if (masked) {   // q1, q2 beside them, keyed the same way (n1, n2 stay on the host: arguments of the q-sample kernel)
        DWS_TRY(upload_if_changed(m->smp.sch_edit, m->smp.sch_host_edit, e->edit_coef, 2 * (size_t)S, s));
        DWS_TRY(m->smp.sch_known.ensure(n * 4));
        DWS_TRY(m->smp.sch_mask.ensure((n + 3) / 4 * 4));
    }
    DWS_TRY(m->smp.eps.ensure(nfull * 4));
    m->smp.eps_B = m->B; m->smp.eps_L = m->L;
    if (kind == DWS_SAMPLER_DPMPP2M) DWS_TRY(m->smp.sch_hist.ensure(nfull * 4));   // the previous step's x0 (first use of this kind)
    DWS_TRY(m->build_step_table(S, net_steps, s));   // the network's step-only part at net_steps (kept while they stay)
    DWS_TRY(m->smp.sch_state.ensure(32));                // step, finished blocks, seed (2 words), visit, history-valid word
    int* st = static_cast<int*>(m->smp.sch_state.p);
    const int V = pg ? pg->V : 0;
    const int R = pg ? V : S;     // streams R (a drawn x_T) and 2R + 1 (the q-sample) lie behind the per-visit ones
    if (pg) {   // step_of[V] and ja[V], jb[V] in one model-owned buffer, keyed on their contents
        std::vector<uint32_t> hp(3 * (size_t)V);
        for (int i = 0; i < V; ++i) {
            const int v = V - 1 - i;      // visit_step is in execution order, the tables are indexed by v
            hp[v] = (uint32_t)std::max(pg->visit_step[i], 0);
            std::memcpy(&hp[V + v], &pg->jump_coef[v], 4);
            std::memcpy(&hp[2 * (size_t)V + v], &pg->jump_coef[V + v], 4);
        }
        DWS_TRY(upload_if_changed(m->smp.sch_prog, m->smp.sch_host_prog, hp.data(), hp.size(), s));
    }
    const int* step_of = pg ? static_cast<const int*>(m->smp.sch_prog.p) : nullptr;
    const float* jump = pg ? m->smp.sch_prog.f() + V : nullptr;
    const float* known_noise = masked ? e->known_noise : nullptr;

    // The state the steps work on: the caller's x on the caller's stream, or -- with a graph, and for the doubled state of
    // a guided run -- the model-owned sch_x: x_T goes in before the steps and x_0 comes out after them, the seed through
    // the state word, so a new x or seed (or known clip, mask, start step) replays the same graph.  Graphs are captured
    // and replayed on the engine's stream.
    const bool staged = use_graph || cfg;
    if (staged) DWS_TRY(m->smp.sch_x.ensure(nfull * 4));
    float* xr = staged ? m->smp.sch_x.f() : x;
    const auto aligned = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    // (the model's buffers come from hipMalloc; per clip every clip must begin on a group border)
    const bool vec = (clips ? clip.n_c : n) % 4 == 0 && aligned(noise) && aligned(known_noise) && (staged || aligned(x));
    const dim3 grid = smp_grid(n, clips, clip.n_c);     // of every launch here that draws
    hipStream_t q = s;
    if (use_graph) DWS_TRY(engine_after_caller(m, s, &q));
    if (init_from_seed && clips && prior)
        hipLaunchKernelGGL((smp_fill_normal_clips_kernel<const uint64_t*, true>), grid, dim3(256), 0, q, xr, clip.n_c,
                           clip.seeds, (uint32_t)R, prior);
    else if (init_from_seed && clips)
        hipLaunchKernelGGL((smp_fill_normal_clips_kernel<const uint64_t*, false>), grid, dim3(256), 0, q, xr, clip.n_c,
                           clip.seeds, (uint32_t)R, prior);
    else if (init_from_seed && prior)
        hipLaunchKernelGGL(smp_fill_normal_kernel<true>, dim3(smp_blocks(n)), dim3(256), 0, q, xr, n, seed, (uint32_t)R, prior);
    else if (init_from_seed)
        hipLaunchKernelGGL(smp_fill_normal_kernel<false>, dim3(smp_blocks(n)), dim3(256), 0, q, xr, n, seed, (uint32_t)R, prior);
    else if (staged)
        DWS_HIP(hipMemcpyAsync(xr, x, n * 4, hipMemcpyDeviceToDevice, q));
    if (cfg) DWS_HIP(hipMemcpyAsync(xr + n, xr, n * 4, hipMemcpyDeviceToDevice, q));    // x_T into both halves
    // what else precedes the steps: the step counter at `start`, the known clip and the mask into their model-owned
    // buffers, the q-sample of the start, the guidance scale
    if (pg)
        hipLaunchKernelGGL(smp_set_program_state_kernel, dim3(1), dim3(1), 0, q, st, start, V - 1, seed);
    else
        hipLaunchKernelGGL(smp_set_state_kernel, dim3(1), dim3(1), 0, q, st, start, seed);
    if (masked) {
        DWS_HIP(hipMemcpyAsync(m->smp.sch_known.p, e->known, n * 4, hipMemcpyDeviceToDevice, q));
        DWS_HIP(hipMemcpyAsync(m->smp.sch_mask.p, e->mask, n, hipMemcpyDeviceToDevice, q));
    }
    if (qsample) {
        const auto launch = [&](auto CLIP, auto PRIOR) {
            hipLaunchKernelGGL((smp_qsample_kernel<decltype(CLIP)::value, decltype(PRIOR)::value>), grid, dim3(256), 0, q, xr,
                               e->start_noise, e->edit_coef[2 * (size_t)S + start], e->edit_coef[3 * (size_t)S + start], n,
                               seed, (uint32_t)(2 * R + 1), clip, prior);
        };
        if (clips && prior) launch(std::true_type{}, std::true_type{});
        else if (clips) launch(std::true_type{}, std::false_type{});
        else if (prior) launch(std::false_type{}, std::true_type{});
        else launch(std::false_type{}, std::false_type{});
    }
    if (cfg) hipLaunchKernelGGL(smp_set_cfg_scale_kernel, dim3(1), dim3(1), 0, q, st, m->smp.cfg_scale);

    StepArgs a{};
    a.x = xr; a.eps = m->smp.eps.f(); a.tab = m->smp.sch_tables.f(); a.st = st; a.noise = noise; a.n = n; a.S = S;
    a.clips = clips;
    StepMore& more = a.more;
    more.V = V;
    more.clip = clip;
    more.prior = prior;
    more.hist = kind == DWS_SAMPLER_DPMPP2M ? m->smp.sch_hist.f() : nullptr;
    if (masked) {
        more.edit = m->smp.sch_edit.f(); more.y = m->smp.sch_known.f(); more.mask = static_cast<const uint8_t*>(m->smp.sch_mask.p);
        more.known_noise = known_noise; more.step_of = step_of;
    }
    const auto jump_launch = [&](auto PRIOR) {
        constexpr bool P = decltype(PRIOR)::value;
        if (clips && vec) hipLaunchKernelGGL((smp_jump_kernel<true, true, P>), grid, dim3(256), 0, q, xr, jump, st, step_of, noise, n, V, clip, prior);
        else if (clips) hipLaunchKernelGGL((smp_jump_kernel<false, true, P>), grid, dim3(256), 0, q, xr, jump, st, step_of, noise, n, V, clip, prior);
        else if (vec) hipLaunchKernelGGL((smp_jump_kernel<true, false, P>), grid, dim3(256), 0, q, xr, jump, st, step_of, noise, n, V, clip, prior);
        else hipLaunchKernelGGL((smp_jump_kernel<false, false, P>), grid, dim3(256), 0, q, xr, jump, st, step_of, noise, n, V, clip, prior);
    };
    // the walk: `reverse` enqueues one reverse step on q; a jump visit is a launch of its own between them
    const auto walk = [&](const auto& reverse) -> int {
        if (!pg) {
            for (int i = 0; i <= start; ++i) DWS_TRY(reverse());
            return DWS_OK;
        }
        for (int i = 0; i < V; ++i) {
            if (pg->visit_step[i] >= 0) DWS_TRY(reverse());
            else if (prior) jump_launch(std::true_type{});
            else jump_launch(std::false_type{});
        }
        return DWS_OK;
    };
    const auto step = [&] { return schedule_step(m, kind, vec, a, cfg, q); };
    if (!use_graph) {
        DWS_TRY(walk(step));
    } else {
        // the edited, the resampling and the guided step have graphs of their own beside the plain one, and each of the
        // four one per form of seed (the per-clip step is other kernel instances on another grid) and per prior on / off
        // (the PRIOR instances; the table sits in a model-owned buffer, so a new one replays the step): the kinds of call
        // may alternate without a new capture
        SamplerState::SchGraph& have = m->smp.sch_graphs[cfg ? SamplerState::SCH_CFG : pg ? SamplerState::SCH_PROG
                                                  : masked ? SamplerState::SCH_EDIT : SamplerState::SCH_PLAIN]
                                                 [(clips ? 1 : 0) + (m->ragged() ? 2 : 0) + (prior ? 4 : 0)];
        const SamplerState::SchKey key{m->B, m->L, S, kind, vec ? 1 : 0, a.tab, noise, a.eps, xr, st, m->step_table_gen,
                                    more.edit, more.y, more.mask, known_noise, V, pg ? m->smp.sch_prog.p : nullptr, more.hist,
                                    clip.seeds, m->ragged() ? m->lengths_dev.p : nullptr, prior};
        DWS_TRY(capture_step(m, q, have.exec, key == have.key, step));
        have.key = key;
        DWS_TRY(walk([&]() -> int {
            DWS_HIP(hipGraphLaunch(have.exec, q));
            return DWS_OK;
        }));
    }
    DWS_TRY(seal_result(m, xr, q));
    if (staged) DWS_HIP(hipMemcpyAsync(x, xr, n * 4, hipMemcpyDeviceToDevice, q));
    if (use_graph) DWS_TRY(caller_after_engine(m, s));
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}

// dws_sampler_run_program: the program must be a walk (see include/dws.h) before anything is enqueued
int sampler_run_program(dws_model* m, float* x, int kind, int S, const float* net_steps, const float* coef, int V,
                        const int32_t* visit_step, const float* jump_coef, const float* noise, uint64_t seed,
                        int init_from_seed, int use_graph, const dws_sampler_edit* e, hipStream_t s) {
    DWS_CHECK(S >= 1, DWS_ERR_INVALID, "sampler: S = %d steps (needs S >= 1)", S);
    DWS_CHECK(e->known && e->mask, DWS_ERR_INVALID, "sampler: a program run needs known and mask");
    DWS_CHECK(V >= 1 && visit_step && jump_coef, DWS_ERR_INVALID, "sampler: empty program or null tables (V = %d)", V);
    const int start = e->start_step;
    DWS_CHECK(start >= 0 && start < S, DWS_ERR_INVALID, "sampler: start_step = %d (needs 0 .. %d)", start, S - 1);
    const int K = start + 1;
    int pos = K;    // the position the state is at: reverse step s takes it from s + 1 to s
    for (int i = 0; i < V; ++i) {
        const int v = V - 1 - i, a = visit_step[i];
        if (a >= 0) {
            DWS_CHECK(a == pos - 1, DWS_ERR_INVALID,
                      "sampler: program entry %d is reverse step %d, but the state is at position %d (step %d is next)", i,
                      a, pos, pos - 1);
            pos = a;
        } else {
            DWS_CHECK(a >= -S && pos - a <= K, DWS_ERR_INVALID,
                      "sampler: program entry %d = %d jumps up from position %d beyond the start position %d", i, a, pos, K);
            const float ja = jump_coef[v], jb = jump_coef[V + v];
            DWS_CHECK(std::isfinite(ja) && std::isfinite(jb) && ja > 0.f, DWS_ERR_INVALID,
                      "sampler: jump coefficients of program entry %d = %g, %g (need finite values, ja > 0)", i, (double)ja,
                      (double)jb);
            pos -= a;
        }
    }
    DWS_CHECK(pos == 0 && visit_step[V - 1] == 0, DWS_ERR_INVALID,
              "sampler: the program ends at position %d (its last visit must be reverse step 0)", pos);
    const SamplerProgram pg{V, visit_step, jump_coef};
    return sampler_run_schedule(m, x, kind, S, net_steps, coef, noise, seed, init_from_seed, use_graph, e, &pg, s);
}

// dws_philox_normal: n values of Philox stream `stream_id` in normal4's layout (group g = elements 4g .. 4g + 3)
int philox_normal(float* x, int64_t n, uint64_t seed, uint32_t stream_id, hipStream_t s) {
    DWS_CHECK(x && n >= 0, DWS_ERR_INVALID, "dws_philox_normal: null x or n = %lld", (long long)n);
    if (n == 0) return DWS_OK;
    hipLaunchKernelGGL(smp_fill_normal_kernel<false>, dim3(smp_blocks((size_t)n)), dim3(256), 0, s, x, (size_t)n, seed, stream_id,
                       (const float*)nullptr);
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}

// dws_philox_normal_clips: row b of x [B, n_per_clip] is dws_philox_normal(n_per_clip, seeds[b], stream_id).  The HOST
// seeds travel as kernel arguments, SeedChunk::N clips per launch: no device table, nothing the host waits for.
int philox_normal_clips(float* x, int64_t B, int64_t n_per_clip, const uint64_t* seeds, uint32_t stream_id, hipStream_t s) {
    DWS_CHECK(x && seeds && B >= 0 && n_per_clip >= 0, DWS_ERR_INVALID,
              "dws_philox_normal_clips: null x or seeds, or B = %lld, n_per_clip = %lld", (long long)B, (long long)n_per_clip);
    if (B == 0 || n_per_clip == 0) return DWS_OK;
    const size_t n_c = (size_t)n_per_clip;
    for (int64_t b0 = 0; b0 < B; b0 += SeedChunk::N) {
        const int rows = (int)std::min<int64_t>(SeedChunk::N, B - b0);
        SeedChunk chunk{};
        std::memcpy(chunk.s, seeds + b0, (size_t)rows * 8);
        hipLaunchKernelGGL((smp_fill_normal_clips_kernel<SeedChunk, false>), smp_grid(n_c * rows, rows, n_c), dim3(256), 0, s,
                           x + (size_t)b0 * n_c, n_c, chunk, stream_id, (const float*)nullptr);
    }
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}

}  // namespace dws
