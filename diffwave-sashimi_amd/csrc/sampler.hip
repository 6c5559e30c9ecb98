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
#include <functional>

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

// End of a visit's kernel: the last block to arrive moves the program on, visit <- v - 1 and step <- step_of[v - 1]
// (the row the next visit's network reads; -1 behind the last visit).  Every block has read the state by then and the
// next kernel that reads it is stream-ordered behind this one, as with the step counter of the kernels above.
// hist_valid >= 0: the new value of the history-valid word (1 behind a multistep reverse visit, 0 behind a jump visit).
__device__ __forceinline__ void smp_program_advance(int* __restrict__ st, const int* __restrict__ step_of, int v,
                                                    int hist_valid) {
    if (atomicAdd(reinterpret_cast<unsigned*>(st + 1), 1u) == gridDim.x - 1) {
        st[1] = 0;
        st[4] = v - 1;
        st[0] = v > 0 ? step_of[v - 1] : -1;
        if (hist_valid >= 0) st[5] = hist_valid;
    }
}

__global__ void smp_fill_normal_kernel(float* __restrict__ x, size_t n, uint64_t seed, uint32_t stream_id) {
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n; g += (size_t)gridDim.x * blockDim.x) {
        float z[4];
        normal4(seed, stream_id, g, z);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (g * 4 + j < n) x[g * 4 + j] = z[j];
    }
}

// x <- (x - c1[t]*eps) / c2[t]  (+ sigma[t]*z if t > 0); products and sums are
// rounded separately to match the reference's op-by-op fp32 evaluation (`generate.py:52,54`): contraction is switched
// off for this kernel and the arithmetic written with plain operators -- the __f*_rn intrinsics are inline functions
// whose operations hipcc fused into FMAs after inlining (found by
// tests/test_sampler_gpu.py::test_step_table_sampler_equals_the_per_step_loop: 1 ulp on most elements once t > 0).
// The last block to finish moves the step index on (t <- t - 1): every block has read t by then, and the next kernel
// that reads it is stream-ordered behind this one -- no separate one-thread launch per step.
// seed_dev non-null (few-step sampler): the Philox seed is read from device memory instead of `seed`.
__global__ void smp_update_kernel(float* __restrict__ x, const float* __restrict__ eps,
                                  const float* __restrict__ tables, int* __restrict__ t_dev,
                                  const float* __restrict__ noise, uint64_t seed, const uint64_t* seed_dev, size_t n,
                                  int T) {
#pragma clang fp contract(off)
    const int t = __builtin_amdgcn_readfirstlane(*(volatile int*)t_dev);
    if (seed_dev) seed = *(const volatile uint64_t*)seed_dev;
    const float c1 = tables[t], c2 = tables[T + t], sg = tables[2 * T + t];
    const float* nz = noise ? noise + (size_t)t * n : nullptr;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n; g += (size_t)gridDim.x * blockDim.x) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (t > 0 && !nz) normal4(seed, (uint32_t)t, g, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t i = g * 4 + j;
            if (i >= n) break;
            // plain operators under `fp contract(off)`: the products, the difference, the quotient and the sum are each
            // rounded once (the __f*_rn intrinsics are inline functions compiled with contraction allowed; after inlining
            // the backend fuses them)
            const float p = c1 * eps[i];
            float v = (x[i] - p) / c2;
            if (t > 0) {
                const float q = sg * (nz ? nz[i] : z[j]);
                v = v + q;
            }
            x[i] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (atomicAdd(reinterpret_cast<unsigned*>(t_dev + 1), 1u) == gridDim.x - 1) {
            t_dev[1] = 0;
            t_dev[0] = t - 1;
        }
    }
}

// DDIM step (Song et al., ICLR 2021, eq. 12) with k[5][S] = k1 .. k5 of sampling.ddim_coefficients, per element:
//   u = (x - k1 eps) / k2;  x = k3 u + k4 eps;  if s > 0 and k5 > 0: x = x + k5 z
// every product, difference, quotient and sum rounded once in this order (contraction off, plain operators, as in
// smp_update_kernel).  z: noise[s] or Philox (seed, s) in normal4's layout; the seed comes from the state (st + 2).
// VEC: every group of 4 is in range and x / eps / noise are 16-byte aligned -> float4 loads and stores.
template <bool VEC>
__global__ void smp_ddim_kernel(float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ k,
                                int* __restrict__ st, const float* __restrict__ noise, size_t n, int S) {
#pragma clang fp contract(off)
    const int s = __builtin_amdgcn_readfirstlane(*(volatile int*)st);
    const uint64_t seed = *(const volatile uint64_t*)(st + 2);
    const float k1 = k[s], k2 = k[S + s], k3 = k[2 * S + s], k4 = k[3 * S + s], k5 = k[4 * S + s];
    const bool add = s > 0 && k5 > 0.f;
    const float* nz = noise ? noise + (size_t)s * n : nullptr;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n; g += (size_t)gridDim.x * blockDim.x) {
        float xv[4] = {0.f, 0.f, 0.f, 0.f}, ev[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {
            const float4 a = reinterpret_cast<const float4*>(x)[g], e = reinterpret_cast<const float4*>(eps)[g];
            xv[0] = a.x; xv[1] = a.y; xv[2] = a.z; xv[3] = a.w;
            ev[0] = e.x; ev[1] = e.y; ev[2] = e.z; ev[3] = e.w;
            if (add && nz) {
                const float4 q = reinterpret_cast<const float4*>(nz)[g];
                z[0] = q.x; z[1] = q.y; z[2] = q.z; z[3] = q.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t i = g * 4 + j;
                if (i >= n) break;
                xv[j] = x[i]; ev[j] = eps[i];
                if (add && nz) z[j] = nz[i];
            }
        }
        if (add && !nz) normal4(seed, (uint32_t)s, g, z);
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float p = k1 * ev[j];
            const float d = xv[j] - p;
            const float u = d / k2;
            const float a = k3 * u;
            const float b = k4 * ev[j];
            float v = a + b;
            if (add) {
                const float q = k5 * z[j];
                v = v + q;
            }
            r[j] = v;
        }
        if (VEC) {
            reinterpret_cast<float4*>(x)[g] = make_float4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t i = g * 4 + j;
                if (i >= n) break;
                x[i] = r[j];
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (atomicAdd(reinterpret_cast<unsigned*>(st + 1), 1u) == gridDim.x - 1) {
            st[1] = 0;
            st[0] = s - 1;
        }
    }
}

// DPM-Solver++(2M) step (Lu et al., 2022; the multistep solver in the data prediction) with m[5][S] = m1 .. m5 of
// sampling.dpmpp_coefficients, per element:
//   p = m1 eps;  d = x - p;  x0 = d / m2;  D = x0;  if second: g = x0 - hist; e = m5 g; D = x0 + e
//   a = m3 x;  b = m4 D;  v = a + b;  hist = x0
// every product, difference, quotient and sum rounded once in this order (contraction off, plain operators).  Returns v
// and leaves x0 in `h`.  With second = false this is DDIM's step at eta = 0 written in the data prediction.
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

// Plain step of DWS_SAMPLER_DPMPP2M.  hist [B, C, L] carries the previous step's x0 across the replays; it is read only
// when second = (history-valid word st[5] != 0) && m5[s] != 0 and written by every step.  No noise: the solver is
// deterministic.  The last block counts the step down and sets the valid word.
// VEC: every group of 4 is in range and x / eps / hist are 16-byte aligned -> float4 loads and stores.
template <bool VEC>
__global__ void smp_dpmpp_kernel(float* __restrict__ x, const float* __restrict__ eps, float* __restrict__ hist,
                                 const float* __restrict__ m, int* __restrict__ st, size_t n, int S) {
#pragma clang fp contract(off)
    const int s = __builtin_amdgcn_readfirstlane(*(volatile int*)st);
    const int valid = __builtin_amdgcn_readfirstlane(*(volatile int*)(st + 5));
    const float m1 = m[s], m2 = m[S + s], m3 = m[2 * S + s], m4 = m[3 * S + s], m5 = m[4 * S + s];
    const bool second = valid != 0 && m5 != 0.f;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n; g += (size_t)gridDim.x * blockDim.x) {
        float xv[4] = {0.f, 0.f, 0.f, 0.f}, ev[4] = {0.f, 0.f, 0.f, 0.f}, hv[4] = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {
            const float4 a = reinterpret_cast<const float4*>(x)[g], e = reinterpret_cast<const float4*>(eps)[g];
            xv[0] = a.x; xv[1] = a.y; xv[2] = a.z; xv[3] = a.w;
            ev[0] = e.x; ev[1] = e.y; ev[2] = e.z; ev[3] = e.w;
            if (second) {
                const float4 q = reinterpret_cast<const float4*>(hist)[g];
                hv[0] = q.x; hv[1] = q.y; hv[2] = q.z; hv[3] = q.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t i = g * 4 + j;
                if (i >= n) break;
                xv[j] = x[i]; ev[j] = eps[i];
                if (second) hv[j] = hist[i];
            }
        }
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = smp_dpmpp_elem(xv[j], ev[j], hv[j], m1, m2, m3, m4, m5, second);
        if (VEC) {
            reinterpret_cast<float4*>(x)[g] = make_float4(r[0], r[1], r[2], r[3]);
            reinterpret_cast<float4*>(hist)[g] = make_float4(hv[0], hv[1], hv[2], hv[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t i = g * 4 + j;
                if (i >= n) break;
                x[i] = r[j];
                hist[i] = hv[j];
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (atomicAdd(reinterpret_cast<unsigned*>(st + 1), 1u) == gridDim.x - 1) {
            st[1] = 0;
            st[0] = s - 1;
            st[5] = 1;
        }
    }
}

// Editing step of dws_sampler_run_edit (inpainting by replacement: Song et al., ICLR 2021, "imputation"; the base case
// of RePaint): the DDPM (tab = c1, c2, sigma) or DDIM (tab = k1 .. k5) update of step s exactly as smp_update_kernel /
// smp_ddim_kernel write it, then, where mask != 0, the element is overwritten with the known audio y noised to the level
// the state is at after step s:
//   v = (s > 0) ? (q1[s] * y) + (q2[s] * zk) : y          edit = q1[S], q2[S] (sampling.edit_coefficients)
// two products and one sum, each rounded once (contraction off, plain operators).  zk: known_noise[s] or Philox stream
// S + 1 + s in normal4's layout, drawn only for groups that hold a known element (no other element reads it).
// KIND = DWS_SAMPLER_DPMPP2M (tab = m1 .. m5): smp_dpmpp_kernel's step -- no update noise; hist gets the network's
// prediction x0, before the replacement; the last block also sets the history-valid word.  hist is null for the others.
// VEC: every group of 4 is in range and all pointers are 16-byte aligned -> float4 for x / eps / y / the noises / hist and
// the four mask bytes of the group as one 32-bit load.
template <int KIND, bool VEC>
__global__ void smp_edit_kernel(float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ tab,
                                const float* __restrict__ edit, int* __restrict__ st, const float* __restrict__ noise,
                                const float* __restrict__ y, const uint8_t* __restrict__ mask,
                                const float* __restrict__ known_noise, float* __restrict__ hist, size_t n, int S) {
#pragma clang fp contract(off)
    const int s = __builtin_amdgcn_readfirstlane(*(volatile int*)st);
    const uint64_t seed = *(const volatile uint64_t*)(st + 2);
    const int valid = KIND == DWS_SAMPLER_DPMPP2M ? __builtin_amdgcn_readfirstlane(*(volatile int*)(st + 5)) : 0;
    const float k1 = tab[s], k2 = tab[S + s], k3 = tab[2 * S + s];
    const float k4 = KIND != DWS_SAMPLER_DDPM ? tab[3 * S + s] : 0.f, k5 = KIND != DWS_SAMPLER_DDPM ? tab[4 * S + s] : 0.f;
    const bool add = KIND == DWS_SAMPLER_DPMPP2M ? false : KIND == DWS_SAMPLER_DDIM ? (s > 0 && k5 > 0.f) : s > 0;
    const bool second = KIND == DWS_SAMPLER_DPMPP2M && valid != 0 && k5 != 0.f;
    const float q1 = edit[s], q2 = edit[S + s];
    const float* nz = noise ? noise + (size_t)s * n : nullptr;
    const float* kz = known_noise ? known_noise + (size_t)s * n : nullptr;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n; g += (size_t)gridDim.x * blockDim.x) {
        float xv[4] = {0.f, 0.f, 0.f, 0.f}, ev[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f};
        float yv[4] = {0.f, 0.f, 0.f, 0.f}, zk[4] = {0.f, 0.f, 0.f, 0.f}, hv[4] = {0.f, 0.f, 0.f, 0.f};
        uint32_t mk = 0;    // byte j: mask of element 4g + j
        if (VEC) {
            const float4 a = reinterpret_cast<const float4*>(x)[g], e = reinterpret_cast<const float4*>(eps)[g];
            xv[0] = a.x; xv[1] = a.y; xv[2] = a.z; xv[3] = a.w;
            ev[0] = e.x; ev[1] = e.y; ev[2] = e.z; ev[3] = e.w;
            if (add && nz) {
                const float4 q = reinterpret_cast<const float4*>(nz)[g];
                z[0] = q.x; z[1] = q.y; z[2] = q.z; z[3] = q.w;
            }
            if (second) {
                const float4 q = reinterpret_cast<const float4*>(hist)[g];
                hv[0] = q.x; hv[1] = q.y; hv[2] = q.z; hv[3] = q.w;
            }
            mk = reinterpret_cast<const uint32_t*>(mask)[g];
            if (mk) {
                const float4 k = reinterpret_cast<const float4*>(y)[g];
                yv[0] = k.x; yv[1] = k.y; yv[2] = k.z; yv[3] = k.w;
                if (s > 0 && kz) {
                    const float4 q = reinterpret_cast<const float4*>(kz)[g];
                    zk[0] = q.x; zk[1] = q.y; zk[2] = q.z; zk[3] = q.w;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t i = g * 4 + j;
                if (i >= n) break;
                xv[j] = x[i]; ev[j] = eps[i];
                if (add && nz) z[j] = nz[i];
                if (second) hv[j] = hist[i];
                if (mask[i]) {
                    mk |= 1u << (8 * j);
                    yv[j] = y[i];
                    if (s > 0 && kz) zk[j] = kz[i];
                }
            }
        }
        if (add && !nz) normal4(seed, (uint32_t)s, g, z);
        if (mk && s > 0 && !kz) normal4(seed, (uint32_t)(S + 1 + s), g, zk);
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v;
            if (KIND == DWS_SAMPLER_DPMPP2M) {          // smp_dpmpp_kernel's order; hv[j] <- x0
                v = smp_dpmpp_elem(xv[j], ev[j], hv[j], k1, k2, k3, k4, k5, second);
            } else if (KIND == DWS_SAMPLER_DDIM) {      // smp_ddim_kernel's order
                const float p = k1 * ev[j];
                const float d = xv[j] - p;
                const float u = d / k2;
                const float a = k3 * u;
                const float b = k4 * ev[j];
                v = a + b;
                if (add) {
                    const float q = k5 * z[j];
                    v = v + q;
                }
            } else {                             // smp_update_kernel's order: k1 = c1, k2 = c2, k3 = sigma
                const float p = k1 * ev[j];
                v = (xv[j] - p) / k2;
                if (add) {
                    const float q = k3 * z[j];
                    v = v + q;
                }
            }
            if ((mk >> (8 * j)) & 0xffu) {
                v = yv[j];
                if (s > 0) {
                    const float a = q1 * yv[j];
                    const float b = q2 * zk[j];
                    v = a + b;
                }
            }
            r[j] = v;
        }
        if (VEC) {
            reinterpret_cast<float4*>(x)[g] = make_float4(r[0], r[1], r[2], r[3]);
            if (KIND == DWS_SAMPLER_DPMPP2M)
                reinterpret_cast<float4*>(hist)[g] = make_float4(hv[0], hv[1], hv[2], hv[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t i = g * 4 + j;
                if (i >= n) break;
                x[i] = r[j];
                if (KIND == DWS_SAMPLER_DPMPP2M) hist[i] = hv[j];
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (atomicAdd(reinterpret_cast<unsigned*>(st + 1), 1u) == gridDim.x - 1) {
            st[1] = 0;
            st[0] = s - 1;
            if (KIND == DWS_SAMPLER_DPMPP2M) st[5] = 1;
        }
    }
}

// Reverse visit of dws_sampler_run_program (RePaint's resampling): smp_edit_kernel's update and replacement at step
// s = st[0], in the same operation order, but the visit number v = st[4] names the noise: noise[v] / known_noise[v], or
// Philox streams v and V + 1 + v (a step that is visited again draws fresh noise).  The last block moves the program on
// (smp_program_advance) instead of counting the step down, and sets the history-valid word for DWS_SAMPLER_DPMPP2M.
template <int KIND, bool VEC>
__global__ void smp_resample_kernel(float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ tab,
                                    const float* __restrict__ edit, int* __restrict__ st,
                                    const int* __restrict__ step_of, const float* __restrict__ noise,
                                    const float* __restrict__ y, const uint8_t* __restrict__ mask,
                                    const float* __restrict__ known_noise, float* __restrict__ hist, size_t n, int S,
                                    int V) {
#pragma clang fp contract(off)
    const int s = __builtin_amdgcn_readfirstlane(*(volatile int*)st);
    const int v = __builtin_amdgcn_readfirstlane(*(volatile int*)(st + 4));
    const uint64_t seed = *(const volatile uint64_t*)(st + 2);
    const int valid = KIND == DWS_SAMPLER_DPMPP2M ? __builtin_amdgcn_readfirstlane(*(volatile int*)(st + 5)) : 0;
    const float k1 = tab[s], k2 = tab[S + s], k3 = tab[2 * S + s];
    const float k4 = KIND != DWS_SAMPLER_DDPM ? tab[3 * S + s] : 0.f, k5 = KIND != DWS_SAMPLER_DDPM ? tab[4 * S + s] : 0.f;
    const bool add = KIND == DWS_SAMPLER_DPMPP2M ? false : KIND == DWS_SAMPLER_DDIM ? (s > 0 && k5 > 0.f) : s > 0;
    const bool second = KIND == DWS_SAMPLER_DPMPP2M && valid != 0 && k5 != 0.f;
    const float q1 = edit[s], q2 = edit[S + s];
    const float* nz = noise ? noise + (size_t)v * n : nullptr;
    const float* kz = known_noise ? known_noise + (size_t)v * n : nullptr;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n; g += (size_t)gridDim.x * blockDim.x) {
        float xv[4] = {0.f, 0.f, 0.f, 0.f}, ev[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f};
        float yv[4] = {0.f, 0.f, 0.f, 0.f}, zk[4] = {0.f, 0.f, 0.f, 0.f}, hv[4] = {0.f, 0.f, 0.f, 0.f};
        uint32_t mk = 0;    // byte j: mask of element 4g + j
        if (VEC) {
            const float4 a = reinterpret_cast<const float4*>(x)[g], e = reinterpret_cast<const float4*>(eps)[g];
            xv[0] = a.x; xv[1] = a.y; xv[2] = a.z; xv[3] = a.w;
            ev[0] = e.x; ev[1] = e.y; ev[2] = e.z; ev[3] = e.w;
            if (add && nz) {
                const float4 q = reinterpret_cast<const float4*>(nz)[g];
                z[0] = q.x; z[1] = q.y; z[2] = q.z; z[3] = q.w;
            }
            if (second) {
                const float4 q = reinterpret_cast<const float4*>(hist)[g];
                hv[0] = q.x; hv[1] = q.y; hv[2] = q.z; hv[3] = q.w;
            }
            mk = reinterpret_cast<const uint32_t*>(mask)[g];
            if (mk) {
                const float4 k = reinterpret_cast<const float4*>(y)[g];
                yv[0] = k.x; yv[1] = k.y; yv[2] = k.z; yv[3] = k.w;
                if (s > 0 && kz) {
                    const float4 q = reinterpret_cast<const float4*>(kz)[g];
                    zk[0] = q.x; zk[1] = q.y; zk[2] = q.z; zk[3] = q.w;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t i = g * 4 + j;
                if (i >= n) break;
                xv[j] = x[i]; ev[j] = eps[i];
                if (add && nz) z[j] = nz[i];
                if (second) hv[j] = hist[i];
                if (mask[i]) {
                    mk |= 1u << (8 * j);
                    yv[j] = y[i];
                    if (s > 0 && kz) zk[j] = kz[i];
                }
            }
        }
        if (add && !nz) normal4(seed, (uint32_t)v, g, z);
        if (mk && s > 0 && !kz) normal4(seed, (uint32_t)(V + 1 + v), g, zk);
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float w;
            if (KIND == DWS_SAMPLER_DPMPP2M) {          // smp_dpmpp_kernel's order; hv[j] <- x0
                w = smp_dpmpp_elem(xv[j], ev[j], hv[j], k1, k2, k3, k4, k5, second);
            } else if (KIND == DWS_SAMPLER_DDIM) {      // smp_ddim_kernel's order
                const float p = k1 * ev[j];
                const float d = xv[j] - p;
                const float u = d / k2;
                const float a = k3 * u;
                const float b = k4 * ev[j];
                w = a + b;
                if (add) {
                    const float q = k5 * z[j];
                    w = w + q;
                }
            } else {                             // smp_update_kernel's order: k1 = c1, k2 = c2, k3 = sigma
                const float p = k1 * ev[j];
                w = (xv[j] - p) / k2;
                if (add) {
                    const float q = k3 * z[j];
                    w = w + q;
                }
            }
            if ((mk >> (8 * j)) & 0xffu) {
                w = yv[j];
                if (s > 0) {
                    const float a = q1 * yv[j];
                    const float b = q2 * zk[j];
                    w = a + b;
                }
            }
            r[j] = w;
        }
        if (VEC) {
            reinterpret_cast<float4*>(x)[g] = make_float4(r[0], r[1], r[2], r[3]);
            if (KIND == DWS_SAMPLER_DPMPP2M)
                reinterpret_cast<float4*>(hist)[g] = make_float4(hv[0], hv[1], hv[2], hv[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t i = g * 4 + j;
                if (i >= n) break;
                x[i] = r[j];
                if (KIND == DWS_SAMPLER_DPMPP2M) hist[i] = hv[j];
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) smp_program_advance(st, step_of, v, KIND == DWS_SAMPLER_DPMPP2M ? 1 : -1);
}

// Jump visit of dws_sampler_run_program: the whole state, known region included, goes from position k up to k + j in one
// draw of the forward process' exact marginal q(x_{k+j} | x_k),
//   x = (ja * x) + (jb * z)      ja = jump[v], jb = jump[V + v] (sampling.jump_coefficients)
// two products and one sum, each rounded once.  z: noise[v] or Philox stream v in normal4's layout.  No network runs.
// The jump re-noises the state, so the last block also clears the history-valid word: the multistep kind's next step is
// first order.
// VEC: every group of 4 is in range and x / noise are 16-byte aligned -> float4 loads and stores.
template <bool VEC>
__global__ void smp_jump_kernel(float* __restrict__ x, const float* __restrict__ jump, int* __restrict__ st,
                                const int* __restrict__ step_of, const float* __restrict__ noise, size_t n, int V) {
#pragma clang fp contract(off)
    const int v = __builtin_amdgcn_readfirstlane(*(volatile int*)(st + 4));
    const uint64_t seed = *(const volatile uint64_t*)(st + 2);
    const float ja = jump[v], jb = jump[V + v];
    const float* nz = noise ? noise + (size_t)v * n : nullptr;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n; g += (size_t)gridDim.x * blockDim.x) {
        float xv[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {
            const float4 a = reinterpret_cast<const float4*>(x)[g];
            xv[0] = a.x; xv[1] = a.y; xv[2] = a.z; xv[3] = a.w;
            if (nz) {
                const float4 q = reinterpret_cast<const float4*>(nz)[g];
                z[0] = q.x; z[1] = q.y; z[2] = q.z; z[3] = q.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t i = g * 4 + j;
                if (i >= n) break;
                xv[j] = x[i];
                if (nz) z[j] = nz[i];
            }
        }
        if (!nz) normal4(seed, (uint32_t)v, g, z);
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = ja * xv[j];
            const float b = jb * z[j];
            r[j] = a + b;
        }
        if (VEC) {
            reinterpret_cast<float4*>(x)[g] = make_float4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t i = g * 4 + j;
                if (i >= n) break;
                x[i] = r[j];
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) smp_program_advance(st, step_of, v, 0);
}

// Partial start in q-sample mode: x holds clean audio and becomes the state at step s0,
//   x = (n1 * x) + (n2 * z0)      n1 = sqrt(level[s0]), n2 = sqrt(1 - level[s0])
// two products and one sum, each rounded once.  z0: the injected tensor or Philox stream `stream_id` (2S + 1).
__global__ void smp_qsample_kernel(float* __restrict__ x, const float* __restrict__ z0, float n1, float n2, size_t n,
                                   uint64_t seed, uint32_t stream_id) {
#pragma clang fp contract(off)
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n; g += (size_t)gridDim.x * blockDim.x) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (!z0) normal4(seed, stream_id, g, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t i = g * 4 + j;
            if (i >= n) break;
            const float a = n1 * x[i];
            const float b = n2 * (z0 ? z0[i] : z[j]);
            x[i] = a + b;
        }
    }
}

// Classifier-free guidance (Ho & Salimans, 2021) between the network and the update of a guided step: eps [2 n] holds the
// network output of the doubled state, the conditional half first; the first half becomes
//   d = eps_c - eps_u;   g = scale * d;   eps = eps_c + g
// each operation rounded once (contraction off, plain operators).  scale is word 6 of the sampler state (a float), so a new
// scale replays the captured step.
__global__ void smp_set_cfg_scale_kernel(int* st, float scale) { reinterpret_cast<float*>(st)[6] = scale; }

template <bool VEC>
__global__ void smp_cfg_kernel(float* __restrict__ eps, const int* __restrict__ st, size_t n) {
#pragma clang fp contract(off)
    const float scale = *reinterpret_cast<const volatile float*>(st + 6);
    const float* __restrict__ eu = eps + n;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n; g += (size_t)gridDim.x * blockDim.x) {
        if (VEC) {
            const float4 c = reinterpret_cast<const float4*>(eps)[g], u = reinterpret_cast<const float4*>(eu)[g];
            float cv[4] = {c.x, c.y, c.z, c.w}, uv[4] = {u.x, u.y, u.z, u.w}, r[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = cv[j] - uv[j];
                const float gd = scale * d;
                r[j] = cv[j] + gd;
            }
            reinterpret_cast<float4*>(eps)[g] = make_float4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t i = g * 4 + j;
                if (i >= n) break;
                const float c = eps[i];
                const float d = c - eu[i];
                const float gd = scale * d;
                eps[i] = c + gd;
            }
        }
    }
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

static int upload_tables(dws_model* m, const float* alpha, const float* alpha_bar, const float* sigma, int T,
                         hipStream_t s) {
    std::vector<float> h = ddpm_table(alpha, alpha_bar, sigma, T);
    // the device copy is keyed on the table CONTENTS (same T with another beta schedule must not reuse it)
    if (m->smp_T == T && m->smp_host_tables == h) return DWS_OK;
    DWS_TRY(m->smp_tables.ensure(h.size() * 4));
    DWS_TRY(m->smp_state.ensure(8));
    DWS_HIP(hipMemcpyAsync(m->smp_tables.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, s));
    DWS_HIP(hipStreamSynchronize(s));
    m->smp_T = T;
    m->smp_host_tables.swap(h);
    return DWS_OK;
}

static int one_step(dws_model* m, float* x, const float* noise, uint64_t seed, int T, hipStream_t s) {
    const size_t n = (size_t)m->B * m->d.out_channels * m->L;
    int* t_dev = static_cast<int*>(m->smp_state.p);
    // every clip is at step t (`generate.py:50`): the network reads row t of the step table built at sampler entry
    m->step_idx = t_dev;
    const int st = m->forward(x, nullptr, m->smp_eps.f(), s);
    m->step_idx = nullptr;
    DWS_TRY(st);
    const int blocks = (int)std::min<size_t>(ceil_div(n, 4 * 256), 4096);
    hipLaunchKernelGGL(smp_update_kernel, dim3(blocks), dim3(256), 0, s, x, m->smp_eps.f(), m->smp_tables.f(), t_dev,
                       noise, seed, (const uint64_t*)nullptr, n, T);
    return DWS_OK;
}

// The caller's stream may be the legacy null stream, which cannot be
// captured: capture and replay on an engine-owned stream that is ordered
// after / before the caller's stream with events.
static int ensure_capture_stream(dws_model* m) {
    if (!m->smp_stream) {
        DWS_HIP(hipStreamCreateWithFlags(&m->smp_stream, hipStreamNonBlocking));
        DWS_HIP(hipEventCreateWithFlags(&m->smp_ev_in, hipEventDisableTiming));
        DWS_HIP(hipEventCreateWithFlags(&m->smp_ev_out, hipEventDisableTiming));
    }
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
    DWS_TRY(m->smp_eps.ensure(n * 4));
    m->smp_eps_B = m->B; m->smp_eps_L = m->L;
    DWS_TRY(m->build_step_table(T, nullptr, s));   // step-only part of the network for t = 0..T-1 (kept while weights and T stay)
    int* t_dev = static_cast<int*>(m->smp_state.p);

    if (!use_graph) {
        hipLaunchKernelGGL(smp_set_step_kernel, dim3(1), dim3(1), 0, s, t_dev, t_start);
        for (int i = 0; i < n_steps; ++i) DWS_TRY(one_step(m, x, noise, seed, T, s));
        DWS_HIP(hipGetLastError());
        return DWS_OK;
    }
    DWS_TRY(ensure_capture_stream(m));
    hipStream_t cs = m->smp_stream;
    DWS_HIP(hipEventRecord(m->smp_ev_in, s));
    DWS_HIP(hipStreamWaitEvent(cs, m->smp_ev_in, 0));
    hipLaunchKernelGGL(smp_set_step_kernel, dim3(1), dim3(1), 0, cs, t_dev, t_start);
    const bool reuse = m->smp_graph && m->g_B == m->B && m->g_L == m->L && m->g_T == T && m->g_x == x &&
                       m->g_noise == noise && m->g_seed == seed;
    if (!reuse) {
        m->drop_graph();
        hipGraph_t graph = nullptr;
        DWS_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
        int st = one_step(m, x, noise, seed, T, cs);
        hipError_t e = hipStreamEndCapture(cs, &graph);
        if (st != DWS_OK) {
            if (graph) hipGraphDestroy(graph);
            return st;
        }
        DWS_HIP(e);
        e = hipGraphInstantiate(&m->smp_graph, graph, nullptr, nullptr, 0);
        hipGraphDestroy(graph);
        DWS_HIP(e);
        ++m->graphs_made;
        m->g_B = m->B; m->g_L = m->L; m->g_T = T; m->g_x = x; m->g_noise = noise; m->g_seed = seed;
    }
    for (int i = 0; i < n_steps; ++i) DWS_HIP(hipGraphLaunch(m->smp_graph, cs));
    DWS_HIP(hipEventRecord(m->smp_ev_out, cs));
    DWS_HIP(hipStreamWaitEvent(s, m->smp_ev_out, 0));
    return DWS_OK;
}

int sampler_run(dws_model* m, float* x, const float* alpha, const float* alpha_bar, const float* sigma, int T,
                const float* noise, uint64_t seed, int init_from_seed, int use_graph, hipStream_t s) {
    DWS_CHECK(T > 0 && alpha && alpha_bar && sigma, DWS_ERR_INVALID, "sampler: bad schedule tables");
    DWS_TRY(upload_tables(m, alpha, alpha_bar, sigma, T, s));
    if (init_from_seed) {
        const size_t n = (size_t)m->B * m->d.in_channels * m->L;
        const int blocks = (int)std::min<size_t>(ceil_div(n, 4 * 256), 4096);
        hipLaunchKernelGGL(smp_fill_normal_kernel, dim3(blocks), dim3(256), 0, s, x, n, seed, (uint32_t)T);
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
// device side of a known-region replacement: the resident q1 / q2 table, the model-owned copies of the known audio and
// the mask, the caller's injected known-region noise (or null)
// host side of a program: visit_step[V] in execution order, jump_coef[2][V] indexed by the visit number
struct SamplerProgram {
    int V;
    const int32_t* visit_step;
    const float* jump_coef;
};

struct EditStep {
    const float* table;
    const float* known;
    const uint8_t* mask;
    const float* known_noise;
};

// device side of a program (dws_sampler_run_program): the resident step_of[V] and jump[2][V] tables
struct ProgStep {
    const int* step_of;
    const float* jump;
    int V;
};

// One reverse step of the schedule: forward at row *st of the step table, then the DDPM, DDIM or DPM-Solver++(2M) update
// (with the replacement of the known region when `ed` is given; as a visit of a program when `pr` is given too).
// cfg (no ed / pr): x is the doubled state [2 Bc, C, L]; the guided eps of the first half, the update over the first half's
// elements alone and the mirror of the first half of the state into the second -- one linear chain.
static int schedule_step(dws_model* m, float* x, int kind, int S, const float* noise, bool vec, const EditStep* ed,
                         const ProgStep* pr, hipStream_t s, bool cfg = false) {
    size_t n = (size_t)m->B * m->d.out_channels * m->L;
    int* st = static_cast<int*>(m->sch_state.p);
    m->step_idx = st;
    const int rc = m->forward(x, nullptr, m->smp_eps.f(), s);
    m->step_idx = nullptr;
    DWS_TRY(rc);
    if (cfg) {
        n /= 2;     // the conditional half: what the update below works on
        ProfileScope prof("smp_cfg", s);
        const int cb = (int)std::min<size_t>(ceil_div(n, 4 * 256), 4096);
        if (vec) hipLaunchKernelGGL(smp_cfg_kernel<true>, dim3(cb), dim3(256), 0, s, m->smp_eps.f(), st, n);
        else hipLaunchKernelGGL(smp_cfg_kernel<false>, dim3(cb), dim3(256), 0, s, m->smp_eps.f(), st, n);
    }
    // dws_profile_enable("smp_update"): the update kernel of an uncaptured step, by kind
    ProfileScope prof(kind == DWS_SAMPLER_DDPM ? "smp_update_ddpm" : kind == DWS_SAMPLER_DDIM ? "smp_update_ddim"
                                                                                             : "smp_update_dpmpp2m", s);
    const int blocks = (int)std::min<size_t>(ceil_div(n, 4 * 256), 4096);
    float* hist = kind == DWS_SAMPLER_DPMPP2M ? m->sch_hist.f() : nullptr;   // the multistep kind's history (allocated by the caller)
    if (ed && pr) {
#define DWS_RESAMPLE_LAUNCH(KIND, VEC)                                                                                 \
    hipLaunchKernelGGL((smp_resample_kernel<KIND, VEC>), dim3(blocks), dim3(256), 0, s, x, m->smp_eps.f(),             \
                       m->sch_tables.f(), ed->table, st, pr->step_of, noise, ed->known, ed->mask, ed->known_noise,     \
                       hist, n, S, pr->V)
        if (kind == DWS_SAMPLER_DDPM) {
            if (vec) DWS_RESAMPLE_LAUNCH(DWS_SAMPLER_DDPM, true); else DWS_RESAMPLE_LAUNCH(DWS_SAMPLER_DDPM, false);
        } else if (kind == DWS_SAMPLER_DPMPP2M) {
            if (vec) DWS_RESAMPLE_LAUNCH(DWS_SAMPLER_DPMPP2M, true); else DWS_RESAMPLE_LAUNCH(DWS_SAMPLER_DPMPP2M, false);
        } else {
            if (vec) DWS_RESAMPLE_LAUNCH(DWS_SAMPLER_DDIM, true); else DWS_RESAMPLE_LAUNCH(DWS_SAMPLER_DDIM, false);
        }
#undef DWS_RESAMPLE_LAUNCH
        return DWS_OK;
    }
    if (ed) {
#define DWS_EDIT_LAUNCH(KIND, VEC)                                                                                     \
    hipLaunchKernelGGL((smp_edit_kernel<KIND, VEC>), dim3(blocks), dim3(256), 0, s, x, m->smp_eps.f(),                 \
                       m->sch_tables.f(), ed->table, st, noise, ed->known, ed->mask, ed->known_noise, hist, n, S)
        if (kind == DWS_SAMPLER_DDPM) {
            if (vec) DWS_EDIT_LAUNCH(DWS_SAMPLER_DDPM, true); else DWS_EDIT_LAUNCH(DWS_SAMPLER_DDPM, false);
        } else if (kind == DWS_SAMPLER_DPMPP2M) {
            if (vec) DWS_EDIT_LAUNCH(DWS_SAMPLER_DPMPP2M, true); else DWS_EDIT_LAUNCH(DWS_SAMPLER_DPMPP2M, false);
        } else {
            if (vec) DWS_EDIT_LAUNCH(DWS_SAMPLER_DDIM, true); else DWS_EDIT_LAUNCH(DWS_SAMPLER_DDIM, false);
        }
#undef DWS_EDIT_LAUNCH
        return DWS_OK;
    }
    if (kind == DWS_SAMPLER_DDPM)
        hipLaunchKernelGGL(smp_update_kernel, dim3(blocks), dim3(256), 0, s, x, m->smp_eps.f(), m->sch_tables.f(), st,
                           noise, (uint64_t)0, reinterpret_cast<const uint64_t*>(st + 2), n, S);
    else if (kind == DWS_SAMPLER_DPMPP2M && vec)
        hipLaunchKernelGGL(smp_dpmpp_kernel<true>, dim3(blocks), dim3(256), 0, s, x, m->smp_eps.f(), hist,
                           m->sch_tables.f(), st, n, S);
    else if (kind == DWS_SAMPLER_DPMPP2M)
        hipLaunchKernelGGL(smp_dpmpp_kernel<false>, dim3(blocks), dim3(256), 0, s, x, m->smp_eps.f(), hist,
                           m->sch_tables.f(), st, n, S);
    else if (vec)
        hipLaunchKernelGGL(smp_ddim_kernel<true>, dim3(blocks), dim3(256), 0, s, x, m->smp_eps.f(), m->sch_tables.f(),
                           st, noise, n, S);
    else
        hipLaunchKernelGGL(smp_ddim_kernel<false>, dim3(blocks), dim3(256), 0, s, x, m->smp_eps.f(), m->sch_tables.f(),
                           st, noise, n, S);
    if (cfg) DWS_HIP(hipMemcpyAsync(x + n, x, n * 4, hipMemcpyDeviceToDevice, s));   // the second half of the state follows the first
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
    const bool cfg = m->cfg_on;
    DWS_CHECK(!cfg || (!e && !pg), DWS_ERR_UNSUPPORTED, "classifier-free guidance is not built for editing or program runs");
    DWS_CHECK(!cfg || m->B % 2 == 0, DWS_ERR_UNSUPPORTED,
              "classifier-free guidance needs a model prepared for 2 x Bc clips (prepared batch: %lld)", (long long)m->B);
    if (m->dirty) DWS_TRY(m->commit(s));
    const size_t nfull = (size_t)m->B * m->d.out_channels * m->L;    // the network's batch
    const size_t n = cfg ? nfull / 2 : nfull;                         // what the caller's x, the noise and the update span

    // update tables, keyed on their contents; DDIM's and DPM-Solver++'s are used as given
    std::vector<float> h = kind != DWS_SAMPLER_DDPM ? std::vector<float>(coef, coef + 5 * (size_t)S)
                                                    : ddpm_table(coef, coef + S, coef + 2 * (size_t)S, S);
    if (!m->sch_tables.p || h.size() != m->sch_host_tables.size() ||
        std::memcmp(h.data(), m->sch_host_tables.data(), h.size() * 4) != 0) {
        DWS_TRY(m->sch_tables.ensure(h.size() * 4));
        DWS_HIP(hipMemcpyAsync(m->sch_tables.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, s));
        DWS_HIP(hipStreamSynchronize(s));
        m->sch_host_tables.swap(h);
    }
    if (masked) {   // q1, q2 beside them, keyed the same way (n1, n2 stay on the host: arguments of the q-sample kernel)
        const size_t nq = 2 * (size_t)S;
        if (!m->sch_edit.p || nq != m->sch_host_edit.size() ||
            std::memcmp(e->edit_coef, m->sch_host_edit.data(), nq * 4) != 0) {
            DWS_TRY(m->sch_edit.ensure(nq * 4));
            DWS_HIP(hipMemcpyAsync(m->sch_edit.p, e->edit_coef, nq * 4, hipMemcpyHostToDevice, s));
            DWS_HIP(hipStreamSynchronize(s));
            m->sch_host_edit.assign(e->edit_coef, e->edit_coef + nq);
        }
        DWS_TRY(m->sch_known.ensure(n * 4));
        DWS_TRY(m->sch_mask.ensure((n + 3) / 4 * 4));
    }
    DWS_TRY(m->smp_eps.ensure(nfull * 4));
    m->smp_eps_B = m->B; m->smp_eps_L = m->L;
    if (kind == DWS_SAMPLER_DPMPP2M) DWS_TRY(m->sch_hist.ensure(nfull * 4));   // the previous step's x0 (first use of this kind)
    DWS_TRY(m->build_step_table(S, net_steps, s));   // the network's step-only part at net_steps (kept while they stay)
    DWS_TRY(m->sch_state.ensure(32));                // step, finished blocks, seed (2 words), visit, history-valid word
    int* st = static_cast<int*>(m->sch_state.p);
    const int V = pg ? pg->V : 0;
    const int R = pg ? V : S;     // streams R (a drawn x_T) and 2R + 1 (the q-sample) lie behind the per-visit ones
    if (pg) {   // step_of[V] and ja[V], jb[V] in one model-owned buffer, keyed on their contents
        std::vector<uint32_t> h(3 * (size_t)V);
        for (int i = 0; i < V; ++i) {
            const int v = V - 1 - i;      // visit_step is in execution order, the tables are indexed by v
            h[v] = (uint32_t)std::max(pg->visit_step[i], 0);
            std::memcpy(&h[V + v], &pg->jump_coef[v], 4);
            std::memcpy(&h[2 * (size_t)V + v], &pg->jump_coef[V + v], 4);
        }
        if (!m->sch_prog.p || h != m->sch_host_prog) {
            DWS_TRY(m->sch_prog.ensure(h.size() * 4));
            DWS_HIP(hipMemcpyAsync(m->sch_prog.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, s));
            DWS_HIP(hipStreamSynchronize(s));
            m->sch_host_prog.swap(h);
        }
    }
    const ProgStep prog{static_cast<const int*>(m->sch_prog.p), m->sch_prog.f() + V, V};
    const ProgStep* pr = pg ? &prog : nullptr;
    const int blocks = (int)std::min<size_t>(ceil_div(n, 4 * 256), 4096);
    const auto aligned = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    const float* known_noise = masked ? e->known_noise : nullptr;
    const EditStep step{m->sch_edit.f(), m->sch_known.f(), static_cast<const uint8_t*>(m->sch_mask.p), known_noise};
    const EditStep* ed = masked ? &step : nullptr;
    // what precedes the steps, on the stream that runs them: the step counter at `start`, the known clip and the mask
    // into their model-owned buffers, the q-sample of the start
    const auto begin = [&](float* xr, hipStream_t q) -> int {
        if (pg)
            hipLaunchKernelGGL(smp_set_program_state_kernel, dim3(1), dim3(1), 0, q, st, start, V - 1, seed);
        else
            hipLaunchKernelGGL(smp_set_state_kernel, dim3(1), dim3(1), 0, q, st, start, seed);
        if (masked) {
            DWS_HIP(hipMemcpyAsync(m->sch_known.p, e->known, n * 4, hipMemcpyDeviceToDevice, q));
            DWS_HIP(hipMemcpyAsync(m->sch_mask.p, e->mask, n, hipMemcpyDeviceToDevice, q));
        }
        if (qsample)
            hipLaunchKernelGGL(smp_qsample_kernel, dim3(blocks), dim3(256), 0, q, xr, e->start_noise,
                               e->edit_coef[2 * (size_t)S + start], e->edit_coef[3 * (size_t)S + start], n, seed,
                               (uint32_t)(2 * R + 1));
        return DWS_OK;
    };
    // the walk: `reverse` enqueues one reverse step on q; a jump visit is a launch of its own between them
    const auto walk = [&](float* xr, bool vec, hipStream_t q, const std::function<int()>& reverse) -> int {
        if (!pg) {
            for (int i = 0; i <= start; ++i) DWS_TRY(reverse());
            return DWS_OK;
        }
        for (int i = 0; i < V; ++i) {
            if (pg->visit_step[i] >= 0) {
                DWS_TRY(reverse());
            } else if (vec) {
                hipLaunchKernelGGL(smp_jump_kernel<true>, dim3(blocks), dim3(256), 0, q, xr, pr->jump, st, pr->step_of,
                                   noise, n, V);
            } else {
                hipLaunchKernelGGL(smp_jump_kernel<false>, dim3(blocks), dim3(256), 0, q, xr, pr->jump, st, pr->step_of,
                                   noise, n, V);
            }
        }
        return DWS_OK;
    };

    if (cfg) {
        // the doubled state lives in the model (sch_x), with and without a graph: x_T goes into both halves, x_0 comes out of
        // the first.  The guided step is a graph of its own (cfg_graph) beside the plain one.
        DWS_TRY(m->sch_x.ensure(nfull * 4));
        float* xs = m->sch_x.f();
        const bool vec = n % 4 == 0 && aligned(noise);
        hipStream_t q = s;
        if (use_graph) {
            DWS_TRY(ensure_capture_stream(m));
            q = m->smp_stream;
            DWS_HIP(hipEventRecord(m->smp_ev_in, s));
            DWS_HIP(hipStreamWaitEvent(q, m->smp_ev_in, 0));
        }
        if (init_from_seed)
            hipLaunchKernelGGL(smp_fill_normal_kernel, dim3(blocks), dim3(256), 0, q, xs, n, seed, (uint32_t)S);
        else
            DWS_HIP(hipMemcpyAsync(xs, x, n * 4, hipMemcpyDeviceToDevice, q));
        DWS_HIP(hipMemcpyAsync(xs + n, xs, n * 4, hipMemcpyDeviceToDevice, q));
        DWS_TRY(begin(xs, q));
        hipLaunchKernelGGL(smp_set_cfg_scale_kernel, dim3(1), dim3(1), 0, q, st, m->cfg_scale);
        if (!use_graph) {
            for (int i = 0; i < S; ++i) DWS_TRY(schedule_step(m, xs, kind, S, noise, vec, nullptr, nullptr, q, true));
        } else {
            const dws_model::SchKey key{m->B, m->L, S, kind, vec ? 1 : 0, m->sch_tables.p, noise, m->smp_eps.p, xs, st,
                                        m->step_table_gen, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                                        kind == DWS_SAMPLER_DPMPP2M ? m->sch_hist.p : nullptr};
            if (!m->cfg_graph || !(key == m->cfg_key)) {
                if (m->cfg_graph) hipGraphExecDestroy(m->cfg_graph);
                m->cfg_graph = nullptr;
                hipGraph_t graph = nullptr;
                DWS_HIP(hipStreamBeginCapture(q, hipStreamCaptureModeThreadLocal));
                int rc = schedule_step(m, xs, kind, S, noise, vec, nullptr, nullptr, q, true);
                hipError_t err = hipStreamEndCapture(q, &graph);
                if (rc != DWS_OK) {
                    if (graph) hipGraphDestroy(graph);
                    return rc;
                }
                DWS_HIP(err);
                err = hipGraphInstantiate(&m->cfg_graph, graph, nullptr, nullptr, 0);
                hipGraphDestroy(graph);
                DWS_HIP(err);
                ++m->graphs_made;
                m->cfg_key = key;
            }
            for (int i = 0; i < S; ++i) DWS_HIP(hipGraphLaunch(m->cfg_graph, q));
        }
        DWS_HIP(hipMemcpyAsync(x, xs, n * 4, hipMemcpyDeviceToDevice, q));
        if (use_graph) {
            DWS_HIP(hipEventRecord(m->smp_ev_out, q));
            DWS_HIP(hipStreamWaitEvent(s, m->smp_ev_out, 0));
        }
        DWS_HIP(hipGetLastError());
        return DWS_OK;
    }
    if (!use_graph) {
        const bool vec = n % 4 == 0 && aligned(x) && aligned(noise) && aligned(known_noise);
        if (init_from_seed)
            hipLaunchKernelGGL(smp_fill_normal_kernel, dim3(blocks), dim3(256), 0, s, x, n, seed, (uint32_t)R);
        DWS_TRY(begin(x, s));
        DWS_TRY(walk(x, vec, s, [&]() { return schedule_step(m, x, kind, S, noise, vec, ed, pr, s); }));
        DWS_HIP(hipGetLastError());
        return DWS_OK;
    }
    // graph: x_T goes into the model-owned state buffer before the replays and x_0 comes out after them, the seed
    // through the state word -- a new x or seed (or known clip, mask, start step) replays the same graph
    DWS_TRY(ensure_capture_stream(m));
    DWS_TRY(m->sch_x.ensure(n * 4));
    float* xs = m->sch_x.f();
    const bool vec = n % 4 == 0 && aligned(noise) && aligned(known_noise);   // (xs, eps, known, mask come from hipMalloc)
    hipStream_t cs = m->smp_stream;
    DWS_HIP(hipEventRecord(m->smp_ev_in, s));
    DWS_HIP(hipStreamWaitEvent(cs, m->smp_ev_in, 0));
    if (init_from_seed)
        hipLaunchKernelGGL(smp_fill_normal_kernel, dim3(blocks), dim3(256), 0, cs, xs, n, seed, (uint32_t)R);
    else
        DWS_HIP(hipMemcpyAsync(xs, x, n * 4, hipMemcpyDeviceToDevice, cs));
    DWS_TRY(begin(xs, cs));
    const dws_model::SchKey key{m->B, m->L, S, kind, vec ? 1 : 0, m->sch_tables.p, noise, m->smp_eps.p, xs, st,
                                m->step_table_gen, ed ? ed->table : nullptr, ed ? ed->known : nullptr,
                                ed ? ed->mask : nullptr, known_noise, V, pr ? m->sch_prog.p : nullptr,
                                kind == DWS_SAMPLER_DPMPP2M ? m->sch_hist.p : nullptr};
    // the edited step and the resampling step have graphs of their own: the three kinds of call may alternate without a
    // new capture
    hipGraphExec_t& exec = pg ? m->prog_graph : masked ? m->edit_graph : m->sch_graph;
    dws_model::SchKey& have = pg ? m->prog_key : masked ? m->edit_key : m->sch_key;
    if (!exec || !(key == have)) {
        if (exec) hipGraphExecDestroy(exec);
        exec = nullptr;
        hipGraph_t graph = nullptr;
        DWS_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
        int rc = schedule_step(m, xs, kind, S, noise, vec, ed, pr, cs);
        hipError_t err = hipStreamEndCapture(cs, &graph);
        if (rc != DWS_OK) {
            if (graph) hipGraphDestroy(graph);
            return rc;
        }
        DWS_HIP(err);
        err = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        hipGraphDestroy(graph);
        DWS_HIP(err);
        ++m->graphs_made;
        have = key;
    }
    DWS_TRY(walk(xs, vec, cs, [&]() -> int {
        DWS_HIP(hipGraphLaunch(exec, cs));
        return DWS_OK;
    }));
    DWS_HIP(hipMemcpyAsync(x, xs, n * 4, hipMemcpyDeviceToDevice, cs));
    DWS_HIP(hipEventRecord(m->smp_ev_out, cs));
    DWS_HIP(hipStreamWaitEvent(s, m->smp_ev_out, 0));
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
    const int blocks = (int)std::min<size_t>(ceil_div((size_t)n, 4 * 256), 4096);
    hipLaunchKernelGGL(smp_fill_normal_kernel, dim3(blocks), dim3(256), 0, s, x, (size_t)n, seed, stream_id);
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}

}  // namespace dws
