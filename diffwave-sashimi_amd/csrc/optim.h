// Fused optimizer step (optim_kernels.hip) behind dws_optim_* (api.hip): job table, launchers and the handle's state.
#pragma once
#include "model.h"

namespace dws {

// Tensors are cut into chunks of OPTIM_CHUNK elements (a multiple of 4: a chunk of a 16-byte aligned tensor starts 16-byte
// aligned); a workgroup of 256 threads walks the chunks c = blockIdx.x, blockIdx.x + gridDim.x, ... of the whole table.
constexpr int OPTIM_CHUNK = 4096;
constexpr int OPTIM_MAX_GRID = 2048;

// One tensor of a step.  mirror (the engine's raw slot of the parameter) and ema (its shadow) may be null.  vec: every
// pointer of the tensor is 16-byte aligned (float4 accesses); otherwise the tensor goes element by element.
struct OptimJob {
    float* p;
    float* mirror;
    const float* g;
    float* m;
    float* v;
    float* ema;
    int64_t numel;
    float step_size;      // lr / (1 - beta1^t)
    float sqrt_bc2;       // sqrt(1 - beta2^t)
    float weight_decay;   // L2: g += weight_decay * p
    int32_t vec;
    int32_t first_chunk;  // number of chunks of the jobs before this one
    int32_t pad;
};

struct OptimHyper {
    float om_beta1;       // 1 - beta1, 1 - beta2 and 1 - ema_decay are formed in double on the host and rounded once
    float beta2, om_beta2, eps;
    float ema_w;          // 1 - ema_decay (the weight of the new parameter in the shadow)
    float max_norm;       // > 0 with a norm pointer: clip to this global L2 norm
};

// Global L2 norm of all gradients of the table: per-workgroup partial sums in double (fixed chunk -> workgroup assignment,
// fixed order inside), then the workgroup that finishes last adds the partials in ascending order and writes
// norm_out[0] (and norm_out2[0] when not null).  `partials`: gridDim.x doubles; `counter`: a zeroed uint32 that the kernel
// leaves zeroed.  No float atomics: the result is the same bits from run to run.
int launch_optim_norm(const OptimJob* table_dev, int njobs, int nchunks, double* partials, unsigned* counter, float* norm_out,
                      float* norm_out2, hipStream_t s);
// The step itself; norm == nullptr: no clipping.
int launch_optim_step(const OptimJob* table_dev, int njobs, int nchunks, const OptimHyper& h, const float* norm, hipStream_t s);

}  // namespace dws

// The handle of dws_optim_create: staging ring of the job table, the device table, the norm scratch.
struct dws_optim {
    dws::StagingRing ring{64};       // (64 slots: the host never waits for the GPU, however far ahead it runs)
    dws::DevBuf table;              // OptimJob[]: written and read in stream order
    dws::DevBuf scratch;             // double partials[OPTIM_MAX_GRID], float norm, uint32 counter
    std::vector<dws::OptimJob> jobs; // host scratch of a call
    double* partials() const { return static_cast<double*>(scratch.p); }
    float* norm() const { return reinterpret_cast<float*>(partials() + dws::OPTIM_MAX_GRID); }
    unsigned* counter() const { return reinterpret_cast<unsigned*>(norm() + 1); }
};
