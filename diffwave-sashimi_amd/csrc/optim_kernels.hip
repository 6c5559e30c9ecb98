// Fused optimizer step: Adam (torch.optim.Adam, amsgrad=False, maximize=False, L2 weight decay), the EMA shadow, the
// engine's raw mirror of the parameter and global-norm clipping, one pass over a job table of tensors (optim.h).
//
// Per element: 16 bytes read (p, g, m, v) + 12 written (p, m, v); +4 written with a mirror; +4 read +4 written with a
// shadow.  The arithmetic is that of torch's single-tensor Adam, operation by operation (lerp for m, mul + addcmul for v,
// sqrt / sqrt(bc2) + eps, addcdiv), with correctly rounded division and square root.
#include "optim.h"

namespace dws {

namespace {

struct OptimElem { float p, m, v, ema; };

// The tensor pointers come out of the job table, so the compiler only knows them as generic addresses (flat_load / flat_store);
// they are device memory: typed as global they become global_load / global_store.
typedef __attribute__((address_space(1))) float gfloat;
typedef float vec4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) vec4 gvec4;
__device__ __forceinline__ gfloat* as_global(const float* p) { return (gfloat*)p; }
__device__ __forceinline__ vec4 load4(const gfloat* p) { return *(const gvec4*)p; }
__device__ __forceinline__ void store4(gfloat* p, vec4 x) { *(gvec4*)p = x; }

// the job of chunk c: the last one whose first_chunk <= c (c is uniform over the workgroup: scalar loads)
__device__ __forceinline__ int job_of_chunk(const OptimJob* __restrict__ jobs, int njobs, int c) {
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_chunk <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void adam_elem(OptimElem& e, float g, bool has_ema, float coef, float wd, float step_size,
                                          float sqrt_bc2, const OptimHyper& h) {
    g *= coef;                                           // coef == 1 without clipping: exact
    if (wd != 0.f) g = fmaf(wd, e.p, g);
    e.m = fmaf(g - e.m, h.om_beta1, e.m);                // exp_avg.lerp_(g, 1 - beta1)
    e.v = fmaf(h.om_beta2 * g, g, e.v * h.beta2);       // exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    const float denom = sqrtf(e.v) / sqrt_bc2 + h.eps;
    e.p = e.p - step_size * (e.m / denom);               // param.addcdiv_(exp_avg, denom, value=-step_size)
    if (has_ema) e.ema = fmaf(h.ema_w, e.p - e.ema, e.ema);   // ema.lerp_(p, 1 - decay)
}

// clip_grad_norm_'s coefficient: min(1, max_norm / (norm + 1e-6)); a NaN norm stays NaN (torch.clamp propagates it)
__device__ __forceinline__ float clip_coef(const float* __restrict__ norm, float max_norm) {
    if (!norm) return 1.f;
    const float c = max_norm / (*norm + 1e-6f);
    return c > 1.f ? 1.f : c;
}

}  // namespace

__global__ __launch_bounds__(256) void engine_adam_step_kernel(const OptimJob* __restrict__ jobs, int njobs, int nchunks,
                                                               OptimHyper h, const float* __restrict__ norm) {
    const float coef = clip_coef(norm, h.max_norm);
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const OptimJob j = jobs[job_of_chunk(jobs, njobs, c)];
        const int64_t off = (int64_t)(c - j.first_chunk) * OPTIM_CHUNK;
        const int64_t left = j.numel - off;
        const int n = left < OPTIM_CHUNK ? (int)left : OPTIM_CHUNK;     // 1 .. OPTIM_CHUNK elements, all inside the tensor
        gfloat* p = as_global(j.p) + off;
        const gfloat* g = as_global(j.g) + off;
        gfloat* m = as_global(j.m) + off;
        gfloat* v = as_global(j.v) + off;
        gfloat* ema = as_global(j.ema) + off;          // (not dereferenced without a shadow / a mirror)
        gfloat* mir = as_global(j.mirror) + off;
        const bool has_ema = j.ema != nullptr, has_mir = j.mirror != nullptr;
        int done = 0;
        if (j.vec) {
            const int n4 = n & ~3;
            for (int i = tid * 4; i < n4; i += 256 * 4) {
                const vec4 p4 = load4(p + i), g4 = load4(g + i), m4 = load4(m + i), v4 = load4(v + i);
                vec4 e4 = {0.f, 0.f, 0.f, 0.f};
                if (has_ema) e4 = load4(ema + i);
                OptimElem e0{p4.x, m4.x, v4.x, e4.x}, e1{p4.y, m4.y, v4.y, e4.y}, e2{p4.z, m4.z, v4.z, e4.z},
                    e3{p4.w, m4.w, v4.w, e4.w};
                adam_elem(e0, g4.x, has_ema, coef, j.weight_decay, j.step_size, j.sqrt_bc2, h);
                adam_elem(e1, g4.y, has_ema, coef, j.weight_decay, j.step_size, j.sqrt_bc2, h);
                adam_elem(e2, g4.z, has_ema, coef, j.weight_decay, j.step_size, j.sqrt_bc2, h);
                adam_elem(e3, g4.w, has_ema, coef, j.weight_decay, j.step_size, j.sqrt_bc2, h);
                const vec4 po = {e0.p, e1.p, e2.p, e3.p};
                store4(p + i, po);
                store4(m + i, vec4{e0.m, e1.m, e2.m, e3.m});
                store4(v + i, vec4{e0.v, e1.v, e2.v, e3.v});
                if (has_ema) store4(ema + i, vec4{e0.ema, e1.ema, e2.ema, e3.ema});
                if (has_mir) store4(mir + i, po);
            }
            done = n4;       // the scalar tail: at most 3 elements
        }
        for (int i = done + tid; i < n; i += 256) {
            OptimElem e{p[i], m[i], v[i], has_ema ? ema[i] : 0.f};
            adam_elem(e, g[i], has_ema, coef, j.weight_decay, j.step_size, j.sqrt_bc2, h);
            p[i] = e.p;
            m[i] = e.m;
            v[i] = e.v;
            if (has_ema) ema[i] = e.ema;
            if (has_mir) mir[i] = e.p;
        }
    }
}

__global__ __launch_bounds__(256) void engine_adam_norm_kernel(const OptimJob* __restrict__ jobs, int njobs, int nchunks,
                                                               double* __restrict__ partials, unsigned* __restrict__ counter,
                                                               float* __restrict__ norm_out, float* __restrict__ norm_out2) {
    __shared__ double red[4];
    __shared__ bool last;
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const OptimJob j = jobs[job_of_chunk(jobs, njobs, c)];
        const int64_t off = (int64_t)(c - j.first_chunk) * OPTIM_CHUNK;
        const int64_t left = j.numel - off;
        const int n = left < OPTIM_CHUNK ? (int)left : OPTIM_CHUNK;
        const gfloat* g = as_global(j.g) + off;
        int done = 0;
        if (j.vec) {
            const int n4 = n & ~3;
            for (int i = tid * 4; i < n4; i += 256 * 4) {
                const vec4 g4 = load4(g + i);
                acc += (double)g4.x * g4.x;
                acc += (double)g4.y * g4.y;
                acc += (double)g4.z * g4.z;
                acc += (double)g4.w * g4.w;
            }
            done = n4;
        }
        for (int i = done + tid; i < n; i += 256) acc += (double)g[i] * g[i];
    }
    // workgroup sum in a fixed order: butterfly inside a wave, then the four waves in ascending order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
        __threadfence();                                        // the partial is visible device-wide before the ticket
        last = atomicAdd(counter, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();                                            // the other workgroups' partials, not a stale cache line
    double s = 0.0;
    for (int i = tid; i < (int)gridDim.x; i += 256) s += __builtin_nontemporal_load(partials + i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        const float nrm = (float)sqrt(((red[0] + red[1]) + red[2]) + red[3]);
        norm_out[0] = nrm;
        if (norm_out2) norm_out2[0] = nrm;
        *counter = 0u;                                          // ready for the next step (stream order)
    }
}

int launch_optim_norm(const OptimJob* table_dev, int njobs, int nchunks, double* partials, unsigned* counter, float* norm_out,
                      float* norm_out2, hipStream_t s) {
    if (njobs <= 0 || nchunks <= 0) return DWS_OK;
    ProfileScope prof("engine_adam_norm", s);
    const int grid = nchunks < OPTIM_MAX_GRID ? nchunks : OPTIM_MAX_GRID;
    hipLaunchKernelGGL(engine_adam_norm_kernel, dim3(grid), dim3(256), 0, s, table_dev, njobs, nchunks, partials, counter,
                       norm_out, norm_out2);
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}

int launch_optim_step(const OptimJob* table_dev, int njobs, int nchunks, const OptimHyper& h, const float* norm, hipStream_t s) {
    if (njobs <= 0 || nchunks <= 0) return DWS_OK;
    ProfileScope prof("engine_adam_step", s);
    const int grid = nchunks < OPTIM_MAX_GRID ? nchunks : OPTIM_MAX_GRID;
    hipLaunchKernelGGL(engine_adam_step_kernel, dim3(grid), dim3(256), 0, s, table_dev, njobs, nchunks, h, norm);
    DWS_HIP(hipGetLastError());
    return DWS_OK;
}

}  // namespace dws
