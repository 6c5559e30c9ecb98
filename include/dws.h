/*
 * dws.h -- flat C ABI of libdws.so, the MI355X (gfx950) DiffWave denoising-loop engine.
 *
 * This is the drop-in boundary.  Everything below is
 * `extern "C"`, plain pointers + explicit sizes + a stream handle; there are no
 * torch types in any signature.  All data pointers are DEVICE pointers unless a
 * parameter is documented as host memory.  Outputs are allocated by the caller
 * (the reference allocates them through torch, `cauchy_cuda.cu:355,462-463`);
 * inputs are borrowed for the duration of the call and never written.
 *
 * Threading / streams: every entry point enqueues on the `stream` it is given
 * (a `hipStream_t` passed as `void*`; NULL = the default stream) and returns
 * without synchronising, exactly like the reference kernels which launch on
 * `at::cuda::getCurrentCUDAStream()` (`cauchy_cuda.cu:124,222,356,464`).
 * One process <-> one device (`generate.py:86`, `distributed_util.py:55`).
 *
 * Errors: every function returns an `int` status: 0 = ok, negative = error
 * class (below).  `dws_last_error()` returns a thread-local message.  The
 * Python host side turns DWS_ERR_UNSUPPORTED into `NotImplementedError`
 * (`extensions/cauchy/cauchy.py:72-77,95-101`) and everything else into
 * `RuntimeError` (the reference's `TORCH_CHECK`s, `cauchy.cpp:6-7,58-64`).
 * Nothing fails silently: an unsupported N raises instead of falling through
 * the `switch` as the reference does (`cauchy_cuda.cu:366-372`).
 *
 * Reference citations are `path:line` relative to albertfgu/diffwave-sashimi.
 */
#ifndef DWS_H_
#define DWS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWS_OK               0
#define DWS_ERR_INVALID     -1   /* bad argument / shape mismatch (reference: TORCH_CHECK -> RuntimeError) */
#define DWS_ERR_UNSUPPORTED -2   /* size the kernels do not cover (reference: NotImplementedError)         */
#define DWS_ERR_HIP         -3   /* a HIP runtime / hipFFT call failed                                      */
#define DWS_ERR_STATE       -4   /* call order violated (e.g. forward before prepare)                       */

/* Thread-local description of the last non-zero status returned on this thread. */
const char* dws_last_error(void);
/* ABI version of the library (bumped when a signature changes). */
int dws_abi_version(void);
/* Name of the GPU architecture the kernels were compiled for ("gfx950"). */
const char* dws_arch(void);

/* ------------------------------------------------------------------------
 * Cauchy multiply -- replaces the pybind module `cauchy_mult`
 * (`extensions/cauchy/cauchy.cpp:86-95`).  Complex64 tensors are passed as
 * interleaved (re,im) float pairs, i.e. the memory of a contiguous
 * torch.cfloat tensor.
 *
 *   v, w : [B, N]   z : [L]   out, dout : [B, L]   dv, dw : [B, N]
 * ------------------------------------------------------------------------ */

/* cauchy_mult_sym_fwd (`cauchy.cpp:55-66`, kernel `cauchy_cuda.cu:242-375`):
 *   out[b,l] = sum_{n<N} v[b,n]/(z[l]-w[b,n]) + conj(v[b,n])/(z[l]-conj(w[b,n]))
 * N is the HALF state size.  Any 1 <= N <= 1024 is accepted (the reference
 * accepts powers of two 2..1024 only, `cauchy.py:95-98`). */
int dws_cauchy_sym_fwd(const float* v, const float* z, const float* w, float* out,
                       int64_t B, int64_t N, int64_t L, void* stream);

/* cauchy_mult_sym_bwd (`cauchy.cpp:68-82`, kernel `cauchy_cuda.cu:377-487`):
 *   dv[b,n] = sum_l dout/(conj z - conj w) + conj(dout)/(z - conj w)
 *   dw[b,n] = conj(v) * sum_l dout/(conj z - conj w)^2 + conj(dout)/(z - conj w)^2 */
int dws_cauchy_sym_bwd(const float* v, const float* z, const float* w, const float* dout,
                       float* dv, float* dw, int64_t B, int64_t N, int64_t L, void* stream);

/* cauchy_mult_fwd (`cauchy.cpp:25-36`, kernel `cauchy_cuda.cu:44-139`), non-symmetric:
 *   out[b,l] = sum_{n<N} v[b,n]/(z[l]-w[b,n]) */
int dws_cauchy_fwd(const float* v, const float* z, const float* w, float* out,
                   int64_t B, int64_t N, int64_t L, void* stream);

/* cauchy_mult_bwd (`cauchy.cpp:38-53`, kernel `cauchy_cuda.cu:141-240`):
 *   dv[b,n] = sum_l dout/conj(z-w),  dw[b,n] = conj(v) * sum_l dout/conj(z-w)^2 */
int dws_cauchy_bwd(const float* v, const float* z, const float* w, const float* dout,
                   float* dv, float* dw, int64_t B, int64_t N, int64_t L, void* stream);

/* ------------------------------------------------------------------------
 * Model -- replaces `models.construct_model(cfg)` + `net((audio, t), mel)`
 * (`models/__init__.py:4-12`, `models/wavenet.py:202-210`,
 * `models/sashimi.py:277-313`).
 * ------------------------------------------------------------------------ */

#define DWS_KIND_WAVENET 1   /* model._name_ == "wavenet" */
#define DWS_KIND_SASHIMI 2   /* model._name_ == "sashimi" */
#define DWS_MAX_POOL 8

/* Field names follow the YAML keys of configs/model/{wavenet,sashimi}.yaml. */
typedef struct dws_model_desc {
    int32_t kind;
    int32_t in_channels, out_channels;
    int32_t diffusion_step_embed_dim_in, diffusion_step_embed_dim_mid, diffusion_step_embed_dim_out;
    int32_t unconditional;            /* 1: no mel path */
    int32_t mel_upsample[2];          /* conditional only; default {16,16} (`wavenet.py:50`) */
    int32_t mel_bands;                /* 80 (`wavenet.py:70`) */
    /* wavenet */
    int32_t res_channels, skip_channels, num_res_layers, dilation_cycle;
    /* sashimi */
    int32_t d_model, n_layers, n_pool, pool[DWS_MAX_POOL], expand, ff, unet, L;
} dws_model_desc;

typedef struct dws_model dws_model;

int dws_model_create(const dws_model_desc* desc, dws_model** out);
int dws_model_destroy(dws_model* m);

/* Number of state-dict entries the model expects and their names/shapes, in
 * the reference's state_dict key layout.  `shape` must
 * hold 8 entries; returns ndim through *ndim.  dtype: 0 = float32, 1 = int64. */
int dws_model_num_params(const dws_model* m);
int dws_model_param_info(const dws_model* m, int index, const char** name,
                         int64_t* shape, int* ndim, int* dtype);

/* Hand one RAW state-dict tensor (weight_g / weight_v / bias / S4 parameters as
 * real (...,2) views, `s4.py:631-638`) to the model.  `data` may be a device or
 * host pointer; it is copied, not retained.  Weight-norm folding, MFMA operand
 * packing and S4 kernel generation happen inside dws_model_commit(). */
int dws_model_set_param(dws_model* m, const char* name, const void* data,
                        const int64_t* shape, int ndim, int dtype, void* stream);

/* Refresh `count` float32 parameters that were set before from device tensors of the same shape, in one launch
 * (a training loop re-sends every parameter after each optimizer step).  Marks the model dirty like set_param. */
int dws_model_update_params(dws_model* m, int32_t count, const char* const* names, const float* const* srcs, void* stream);

/* String options (unknown key/value -> DWS_ERR_INVALID):
 *   "precision" = "f32"    (default) exact-f32 MFMA (v_mfma_f32_32x32x2_f32): bitwise an fmaf chain
 *               = "bf16x3" WaveNet residual layers on the bf16 matrix cores with a 3-term hi/lo split
 *                          (W_hi x_hi + W_hi x_lo + W_lo x_hi, fp32 accumulate): ~1e-5 relative, 5.3x the
 *                          matrix rate.  Not part of the reference surface.
 *               = "bf16x6" WaveNet residual layers on the bf16 matrix cores at fp32-EQUIVALENT accuracy: every GEMM
 *                          operand as an exact 3-term bf16 split (24 significand bits), the six partial products above
 *                          2^-26 accumulated in fp32, Winograd F(2,3) form (the f32 path's algorithm and roundings).
 *                          WaveNet: the residual layers in sampling and in forward_train; in training also the gate
 *                          adjoint, dskip = Wf^T dy and the res / skip / final_conv.0 weight gradients (where L % 4 == 0),
 *                          the dilated conv's data and weight gradients in Winograd form (any L).  SaShiMi: the S4 block tails
 *                          (all H) in sampling; in training the pointwise GEMMs and weight gradients of the step.
 *                          What "fp32-equivalent" was MEASURED to mean (tests/test_bf16x6_gpu.py, test_full_size_gpu.py,
 *                          test_split_trajectory_gpu.py): operands are carried exactly, products are exact, the fp32
 *                          accumulation is the matrix core's own adder, which is NOT an fmaf chain -- fp32-CLASS, not
 *                          bit-compatible.  GEMM level, error relative to sum |a||b|: 2^-24.1 (K = 16) .. 2^-22.4 (K = 256);
 *                          on operands spread over 2^(+-12) up to 7.5e-7, i.e. 2 - 3 x a sequential fp32 sum in the same
 *                          k-block order (torch's own fp32 matmul: 8.7e-7 on the same operands); bound asserted:
 *                          min(2^-20, 4 x sequential fp32).  Network level against float64: 0.73 .. 1.07 x the exact-f32
 *                          path's error (WaveNet and SaShiMi, B = 1 .. 32, L = 16000), T = 200 trajectories within 3e-7
 *                          of the f32 path's.  Results do not depend on the batch position of a clip (bitwise).
 *                          Where no split instance exists (SaShiMi stages whose length is not a multiple of 4, channel
 *                          counts the MFMA tiling does not cover, the pooling GEMMs, 3-tap training GEMMs, WaveNet
 *                          adjoints at L % 4 != 0, the one-channel convolutions, the step-embedding MLP) the f32
 *                          kernels run: the tap "split_launches" reports how many GEMM launches of the last forward ran
 *                          split and how many fell back.
 *               = "f16x3"  the same kernels with a 2-term fp16 split of power-of-two scaled operands (22 significand
 *                          bits per operand, three products: half the matrix work of bf16x6).  Inference only.  Accepted
 *                          by the same float64 criterion; activations beyond 2^11 overflow fp16 and yield NaN, and so
 *                          does a WaveNet step-embedding row fc_t(e) beyond ~40 at C = 256 (it rides in an fp16 k-block
 *                          times the weight scale).  An experiment: narrower than the reference's arithmetic, never a default.
 *   "conv_algo" = "winograd" (default) WaveNet residual layers (precision f32) with the dilated 3-tap convolution in
 *                          Winograd F(2,3) form along the dilation stride: 8 C^2 instead of 12 C^2 flop per position,
 *                          one extra fp32 rounding in the weights and in the inputs (same 1e-6 class error); the
 *                          training step's data and weight gradients of that convolution run the same pairing
 *               = "direct" the direct three-tap form, forward and both adjoints (A/B runs).
 *   "bx6_mfma" = "16x16x32" (default; initial value from the environment variable DWS_BX6_MFMA) WaveNet, precision bf16x6,
 *                          res_channels = skip_channels = 256: both GEMMs of the layer kernel on v_mfma_f32_16x16x32_bf16 (the
 *                          chip holds a higher clock on it); same error class, last bits differ from "32x32x16"
 *              = "gemm2-16x16x32" only the [res; skip] GEMM and the epilogue on that shape
 *              = "32x32x16" the v_mfma_f32_32x32x16_bf16 kernel (every other width runs it whatever this says).
 *   "bx6_a_ring" = "quarter-step" (default; initial value from the environment variable DWS_BX6_A_RING) the "16x16x32" kernel above:
 *                          GEMM1's weight fragments are requested three at a time, three quarter-steps (36 MFMAs) ahead of their use
 *                = "half-step" six at a time, one half-step (24 MFMAs) ahead: the kernel as it was.  The two give equal bits; the
 *                          option has no effect where another kernel runs (bx6_mfma other than "16x16x32", other widths). */
int dws_model_set_option(dws_model* m, const char* key, const char* value);

/* Class conditioning (class-conditional generation; not in the reference).  Call after dws_model_create and before the
 * first set_param / update_params / commit (later: DWS_ERR_STATE).  n_classes = K in 1..65534 adds ONE parameter to num_params /
 * param_info / set_param / update_params / get_grad(s) / gradient sinks: float32 [K+1, diffusion_step_embed_dim_out],
 * "residual_layer.label_embedding.weight" (WaveNet) or "label_embedding.weight" (SaShiMi), beside fc_t1 / fc_t2.  Row K is
 * the null class.  For clip b at step t_b with label y_b in 0..K
 *     e_b = swish(fc_t2(swish(fc_t1(emb(t_b))))) + table[y_b]            (one fp32 add per element)
 * and every block's fc_t runs on e_b: the label enters through the rows the layer kernels already read.  The path sits
 * upstream of every precision switch (exact fp32 under bf16x6 too).  Backward: d table[c] = sum_{b : y_b = c} d e_b in
 * ascending b; rows of classes absent from the batch are exactly zero; a data-only backward does not touch it.
 * A model without this call is unchanged. */
int dws_model_set_classes(dws_model* m, int32_t n_classes);

/* The labels of the prepared batch: HOST int32[B], each in 0..K (checked before anything is enqueued; B must be the
 * prepared batch), or NULL = the null class for every clip.  The upload goes through pinned staging (the host never waits
 * for the GPU on it).  Labels hold until changed; a dws_model_prepare to another shape resets them to the null class.
 * A model without classes -> DWS_ERR_INVALID.
 * Samplers: with labels installed the step table holds rows per (step, clip) (WaveNet's correction fragments then take
 * n_layers x T x B x row floats: 1.9 GB at 36 layers, T = 200, B = 32, C = 256) built from the summed embedding by the
 * row kernels of the per-clip forward, so a labelled run is bit-equal to a loop of labelled forwards.  A new assignment at
 * the same (B, S) rewrites the rows in place and replays the captured graphs (tap "sampler_graphs" does not move). */
int dws_model_set_labels(dws_model* m, const int32_t* labels, int64_t B, void* stream);

/* Ragged batches (both backbones): clip b of the prepared [B, ., L] batch is len_b <= L samples long, the rest is padding.
 * lengths: HOST int32[B] with 1 <= len_b <= L, or NULL = off (every path bit for bit as without this call).  mel_frames:
 * HOST int32[B] or NULL; on a conditional model NULL means ceil(len_b / (s0 s1)); needs 1 <= frames_b and
 * s0 s1 frames_b >= len_b (and frames_b <= Tmel of an installed mel; dws_model_set_condition checks the same).
 * Contract: over [0, len_b) clip b's output is what the network gives for that clip alone at L = len_b, up to the
 * arithmetic of the kernel path; nothing stored at positions >= len_b (audio, mel frames >= frames_b, injected noise,
 * internal buffers, NaN included) reaches a valid position; `out` of dws_model_forward and `x` of every sampler entry hold
 * exactly 0.0f there.  How, WaveNet: behind init_conv and every residual layer but the last a store-only kernel (wn_mask_tail)
 * rewrites x[b, c, len_b .. len_b + d) (d = the next layer's dilation) to -fc_t(e)[b, c] of the next layer, so that the
 * dilated convolution's zero-padded input h = x + fc_t(e) is 0 there as it is past the end of a clip run alone; the
 * conditioner treats mel frames >= frames_b and first-upsampler positions >= s0 frames_b as zero.  A padded position still
 * costs its full layer time.
 * SaShiMi: every op but the S4 convolution is pointwise in the (pooled) position, so the three convolutions seal their own
 * INPUT on the load side: row (b, h) of a stage is convolved as if it were zero on [len_b / div, L_stage), div = the product
 * of the pooling factors above the stage (the fused in-LDS FFT through its load descriptor and a select on the last packed
 * point, the segmented kernel through its segment bounds -- a workgroup whose output segment is wholly padding returns at
 * once --, the rocFFT path through a store-only launch on its input rows); `out` is zeroed behind each clip's end.  Every
 * length must be a multiple of the product of the pooling factors (else DWS_ERR_UNSUPPORTED): len_b / div is an integer.
 * All checks precede any enqueue: B must be the prepared batch (DWS_ERR_INVALID); before dws_model_prepare ->
 * DWS_ERR_STATE; a shared mel (Bm == 1) with lengths -> DWS_ERR_INVALID.  The table goes
 * through pinned staging into a model-owned device buffer (the host never waits for the GPU), holds until changed, and is
 * dropped by a dws_model_prepare to another shape.  With a mel installed the conditioner terms are re-evaluated from the
 * engine's copy of the mel under the new frame counts.  The sampler's captured steps contain the mask launches and read
 * the table from device memory: a new table at the same (B, L) replays them; lengths on / off are graphs of their own.
 * While lengths are on, dws_model_forward_train and dws_sampler_set_cfg(on) return DWS_ERR_UNSUPPORTED. */
int dws_model_set_lengths(dws_model* m, const int32_t* lengths, const int32_t* mel_frames, int64_t B, void* stream);

/* Fold / pack everything that depends only on the weights.  Called implicitly
 * by forward when parameters changed since the last commit. */
int dws_model_commit(dws_model* m, void* stream);

/* Size the workspace for inputs of shape audio[B, in_channels, L]. */
int dws_model_prepare(dws_model* m, int64_t B, int64_t L);

/* Install (or with mel == NULL remove) the mel-spectrogram condition
 * mel[Bm, mel_bands, Tmel], Bm in {1, B} (`generate.py:140,155`).  The
 * upsample + 1x1 terms of every block (`wavenet.py:98-111`,
 * `sashimi.py:160-175`) are evaluated once here, not per step. */
int dws_model_set_condition(dws_model* m, const float* mel, int64_t Bm, int64_t Tmel, void* stream);

/* eps[B, out_channels, L] = net((audio[B, in_channels, L], steps[B]))  (fp32).
 * `steps` holds the diffusion step of every batch element as float32
 * (`generate.py:50`; the int64 steps of `train.py:218` are converted by the host side). */
int dws_model_forward(dws_model* m, const float* audio, const float* steps, float* out, void* stream);

/* Training path (`train.py:198-222`): both backbones, unconditional and mel-conditional, precision f32 or bf16x6
 * (precision=bf16x3 / f16x3 return DWS_ERR_UNSUPPORTED, as does WaveNet bf16x6 where the MFMA adjoints do not run; SaShiMi channel counts that are not multiples of 32 train on a
 * plain-FMA GEMM instead of the MFMA adjoints).
 * forward_train == forward but keeps the activations backward needs inside the model -- of ONE forward:
 * every forward_train must be followed by its backward before the next forward_train.  backward takes dLoss/d(eps)[B, out_channels, L] and produces the gradient of every RAW
 * state-dict tensor (weight_g / weight_v / bias ...), fetched with get_grad (device copy).  The
 * data-parallel exchange of those gradients is the host side's job (RCCL all-reduce,
 * `distributed_util.py:97-149`). */
int dws_model_forward_train(dws_model* m, const float* audio, const float* steps, float* out, void* stream);
int dws_model_backward(dws_model* m, const float* dout, void* stream);
/* backward that can also deliver the gradient w.r.t. the AUDIO input (guided sampling, input-space optimisation):
 * daudio[B, in_channels, L] (device; NULL: not wanted) = d Loss / d audio of the pending forward_train.
 * param_grads = 1: everything dws_model_backward does (it is this call with daudio == NULL), plus daudio.
 * param_grads = 0: DATA-ONLY -- the chain of data adjoints alone, the same kernels in the same order (daudio has the same
 * bits as under param_grads = 1): no weight / bias gradient, no weight-norm adjoint, no S4 kernel adjoint, no LayerNorm
 * parameter sums, no step-embedding or conditioner adjoint.  No gradient buffer is written, nothing is delivered to
 * installed sinks and no group event is recorded.  Needs daudio (else DWS_ERR_INVALID).
 * Preconditions as dws_model_backward: one pending forward_train, precision f32 or bf16x6.  The mel condition and the
 * diffusion steps get no gradient. */
int dws_model_backward_input(dws_model* m, const float* dout, float* daudio, int32_t param_grads, void* stream);
/* The training forward of a DATA-ONLY backward (guided sampling, `audio.grad` of an eval() module): arguments, preconditions
 * (precision f32 or bf16x6, one mel per clip, no per-clip lengths) and output as dws_model_forward_train.
 * Where dws_model_forward_train is accepted this IS that call: the same commit, launches and bits.  A SaShiMi model that
 * dws_model_forward_train refuses only because the run length is not its kernels' own (`L` buffers != stage length) or
 * because a stage runs the segmented convolution is accepted here: the commit stays the sampling path's (per-block kernel
 * chains at min(L, l_max) taps per direction) and every block's S4 convolution runs on the route the sampler takes at this
 * length -- the fused LDS FFT, the segmented kernel (an instance that also stores the pre-activation; its adjoint is the
 * same kernel on the conjugated spectra with the causal' / anti-causal' ones swapped) or rocFFT.  WaveNet: forward_train.
 * Afterwards dws_model_backward_input(param_grads = 0) is valid; dws_model_backward and param_grads = 1 return
 * DWS_ERR_STATE (no parameter gradient is built at another length or on the segmented path, and none is kept for here). */
int dws_model_forward_input(dws_model* m, const float* audio, const float* steps, float* out, void* stream);
int dws_model_get_grad(dws_model* m, const char* name, float* dst, int64_t numel, void* stream);
/* The same for `count` parameters in one launch (the autograd wrapper fetches every gradient after backward). */
int dws_model_get_grads(dws_model* m, int32_t count, const char* const* names, float* const* dsts, const int64_t* numels,
                        void* stream);

/* Staged hand-over of the gradients for the data-parallel exchange (`distributed_util.py:112-142` flattens and all-reduces
 * AFTER backward; here the exchange of a bucket starts while backward still runs).  set_grad_sinks names, for `count`
 * parameters, a device destination and a GROUP (the host's all-reduce bucket) each; it stays in force until it is called
 * again (count == 0 removes it).  With sinks installed, dws_model_backward itself delivers the gradients: as soon as the last
 * gradient of a group has been produced it copies the group to its destinations (one launch) and records the group's
 * event on `stream`; groups left over are delivered at the end, so after backward every destination is written in stream
 * order (no get_grads call is needed for them).  grad_group_wait makes `waiting_stream` wait for a group's event (call it
 * after backward has returned: a collective launched on that stream then depends on the group's gradients only, not on
 * the rest of backward).  When a gradient is final is learnt from the first backward after set_grad_sinks (which delivers
 * everything at its end); grad_ready_seq reports, per parameter, the flush point (block / layer number in backward order,
 * -1 = never written) after which its gradient was final in the last backward -- the order a host should bucket in. */
int dws_model_set_grad_sinks(dws_model* m, int32_t count, const char* const* names, float* const* dsts, const int64_t* numels,
                             const int32_t* groups, int32_t ngroups);
int dws_model_grad_group_wait(dws_model* m, int32_t group, void* waiting_stream);
int dws_model_grad_ready_seq(dws_model* m, int32_t count, const char* const* names, int32_t* seq_out);

/* ---- Fused optimizer step (not in the reference, whose `train.py:91` builds torch.optim.Adam) --------------------------
 * ONE pass over a table of `count` float32 tensors that does, per element,
 *     g'  = coef * g  (+ weight_decay * p)                      coef = 1 without clipping
 *     m  += (g' - m) (1 - beta1)
 *     v   = beta2 v + (1 - beta2) g'^2
 *     p  -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *     ema = ema + (1 - ema_decay) (p - ema)                     where ema[i] is given
 *     mirror = p                                                where a mirror is given
 * i.e. torch.optim.Adam (amsgrad=False, maximize=False, L2 weight decay) operation by operation in fp32 with correctly
 * rounded division and square root, the EMA shadow as `ema.lerp_(p, 1 - ema_decay)`, and the engine's raw copy of the
 * parameter.  16 bytes read + 12 written per element, +4 with a mirror, +8 with a shadow.  The bias corrections are formed
 * in double from the integer step[i]; lr, step and weight_decay are per tensor (parameter groups).
 *
 * The handle owns the pinned staging ring of the job table (a slot is reused only after the event behind its upload has
 * completed; while none is free the ring grows: the host does not wait for the GPU), the device table and the norm scratch.
 * Two corner cases do wait, and nothing else does: a call that needs a larger device table than the handle has (the first
 * call, or more tensors than twice any earlier call) frees and reallocates it, which synchronises the device; and a ring
 * that has grown to 64 slots, all still in flight (the host 64 steps ahead of the GPU), waits for the oldest one.
 * Calls on one handle must be ordered on one stream.  dws_optim_chunk: tensors are cut into chunks of that many elements
 * (the grid is capped at 2048 workgroups of 256 threads that loop over the chunks).  A tensor whose every pointer is 16-byte
 * aligned moves as 16-byte vectors, any other (4-byte aligned views of a flat buffer) element by element.
 *
 * ema, mirrors, weight_decay: NULL tables or NULL entries = none.  ema_decay in (0, 1) is needed with shadows.
 * max_grad_norm > 0: torch.nn.utils.clip_grad_norm_ with the L2 norm over ALL `count` gradients,
 * coef = min(1, max_grad_norm / (norm + 1e-6)), as a second launch BEFORE the step: per-workgroup partial sums in double, a
 * fixed-order final sum by the workgroup that finishes last (no floating-point atomics: same bits from run to run), the
 * norm in a device float the step reads.  The gradients themselves are NOT rewritten (torch scales p.grad in place).  A
 * non-finite norm propagates into every element, as it does in torch.  grad_norm_out (device float, may be NULL) receives
 * the norm; given without clipping, the norm launch runs for it alone.  Nothing synchronises with the host.
 *
 * model (may be NULL) with names[count]: tensor i with names[i] != NULL is the model's parameter of that name -- its raw
 * slot becomes the mirror (mirrors[i] is ignored), and the model is marked as dws_model_update_params marks it (the next
 * forward commits again).  Unknown name, a non-float32 parameter or another element count -> DWS_ERR_INVALID. */
typedef struct dws_optim dws_optim;
int dws_optim_create(dws_optim** out);
int dws_optim_destroy(dws_optim* o);
int dws_optim_chunk(void);
int dws_optim_step(dws_optim* o, int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, float* const* ema, float* const* mirrors, const int64_t* numels, const double* lr,
                   const int64_t* step, const double* weight_decay, double beta1, double beta2, double eps, double ema_decay,
                   double max_grad_norm, float* grad_norm_out, dws_model* model, const char* const* names, void* stream);

/* Debug/parity tap: copy an internal activation into `dst` (device pointer,
 * `capacity` floats).  WaveNet: "pre_final" = ReLU(final_conv[0](skip)) [B,S,L],
 * "skip" [B,S,L], "x" (last residual output) [B,C,L], "hsave" [n_layers,B,2C,L] (the gate
 * pre-activations kept by the last dws_model_forward_train); the step-only terms: "part_t"
 * [B, n_layers*C] / "abt" (per-clip rows of the last forward) and "tab_part_t"
 * [T, n_layers*C] / "tab_abt" (the sampler's step table).  Function-level taps of the last per-clip forward, both
 * models: "emb" [B, embed_dim_in] (`models/utils.py:20-27`), "emb_mlp" [B, embed_dim_out] (the two swish layers), "part_t"
 * (every block's fc_t row); SaShiMi also "nfin" [B, d_model, L] = the final TransposedLayerNorm, "out:<layer prefix>" the
 * output of a layer and "k:<block prefix>" its S4 kernel.  The mel conditioner as the last dws_model_set_condition
 * with a mel left it (Bm = that mel's batch, 1 or B; DWS_ERR_STATE while no mel is installed): WaveNet "melc"
 * [n_layers, Bm, 2C, L] = the term every layer adds to its gate pre-activations, SaShiMi "melc:<block prefix>"
 * [Bm, H, L_stage] of that block; both models "mel_u0" [Bm, mel_bands, T0] / "mel_u1" [Bm, mel_bands, T1] = the two
 * upsampled mels (untruncated) of the layer / block processed last (the last one in execution order).  Both models:
 * "sampler_eps" = the network output of the sampler's last reverse step [B,Cout,L]. */
int dws_model_read_tap(dws_model* m, const char* tap, float* dst, int64_t capacity, void* stream);

/* ------------------------------------------------------------------------
 * Reverse-diffusion sampler -- replaces `generate.sampling`
 * (`generate.py:23-55`).  One reverse step is captured as a hipGraph on first
 * use and replayed T times; step index, schedule coefficients and the RNG
 * counter live in device memory.  Everything of the network that depends on the
 * diffusion step only (embedding, its MLP, every layer's fc_t projection) is
 * evaluated once per (weights, T) for t = 0..T-1 and indexed by the device step
 * counter inside the replays; the update x <- (x - c1 eps) / c2 (+ sigma z) rounds
 * every product, difference, quotient and sum once, as the reference's op-by-op
 * float32 evaluation does.
 *
 *   x          [B, C, L]  in: x_T (or anything when seed-driven, see below); out: x_0
 *   alpha, alpha_bar, sigma  HOST float[T] tables from calc_diffusion_hyperparams
 *                            (`utils.py:121-151`)
 *   noise      optional DEVICE [T, B, C, L]: noise[t] is added after step t
 *              (t > 0).  NULL -> on-device Philox4x32-10 + Box-Muller keyed by
 *              (seed, t, element).
 *   init_from_seed  non-zero: also draw x_T ~ N(0, I) from the Philox stream.
 * ------------------------------------------------------------------------ */
int dws_sampler_run(dws_model* m, float* x, const float* alpha, const float* alpha_bar,
                    const float* sigma, int32_t T, const float* noise, uint64_t seed,
                    int32_t init_from_seed, int32_t use_graph, void* stream);

/* Run `n_steps` reverse steps starting at step index t_start (for benchmarking
 * a bounded number of steps of the T-step loop with the same graph). */
int dws_sampler_steps(dws_model* m, float* x, const float* alpha, const float* alpha_bar,
                      const float* sigma, int32_t T, int32_t t_start, int32_t n_steps,
                      uint64_t seed, int32_t use_graph, void* stream);

/* Few-step samplers (not the reference's loop): S reverse steps s = S-1 .. 0 with the
 * network at net_steps[s] -- any finite float, e.g. the fractional training steps of
 * DiffWave's step alignment or the sub-sequence tau of DDIM.  The step table is built
 * at these values (kept while the values and the weights stay).
 *
 *   kind       DWS_SAMPLER_DDPM: coef = alpha[S], alpha_bar[S], sigma[S] (S-row tables of
 *              calc_diffusion_hyperparams); the update and its c1/c2 arithmetic are those of
 *              dws_sampler_run.
 *              DWS_SAMPLER_DDIM: coef = k1[S] .. k5[S] (sampling.ddim_coefficients, taken as
 *              given); per element, each operation rounded once, in this order:
 *                u = (x - k1 eps) / k2;  x = k3 u + k4 eps;  if s > 0 and k5 > 0: x = x + k5 z
 *              DWS_SAMPLER_DPMPP2M: DPM-Solver++(2M) (Lu et al., 2022), the second-order multistep
 *              solver in the data prediction; coef = m1[S] .. m5[S] (sampling.dpmpp_coefficients,
 *              taken as given).  With a_s the level of step s, p_s = a_{s-1} (p_0 = 1),
 *              lam(v) = log(sqrt(v) / sqrt(1 - v)) and h_s = lam(p_s) - lam(a_s) (h_0 = +inf):
 *                m1 = sqrt(1 - a), m2 = sqrt(a), m3 = sqrt((1 - p) / (1 - a)) (m3[0] = 0),
 *                m4 = sqrt(p) (1 - exp(-h)) (m4[0] = 1), m5[s] = h_s / (2 h_{s+1}) for 1 <= s <= S-2,
 *                else 0 (the first step has no history; the last goes to sigma = 0 and is first order).
 *              Per element, each operation rounded once, in this order:
 *                p = m1 eps;  d = x - p;  x0 = d / m2
 *                D = x0;  if second:  g = x0 - hist;  e = m5 g;  D = x0 + e
 *                a = m3 x;  b = m4 D;  x = a + b;  hist = x0
 *              hist is a model-owned [B, C, L] buffer that holds the previous step's x0 (the network's
 *              prediction, before any known-region replacement).  second = (the history-valid word
 *              of the device state != 0) and m5[s] != 0.  The word is 0 at the start of every run, the
 *              last block of every step of this kind sets it to 1, a jump visit of a program clears
 *              it (the jump re-noises the state, so the step behind it is first order).  With m5 = 0
 *              the step is DDIM's at eta = 0.  The solver is deterministic: no z is drawn or read in a
 *              reverse step, and `noise` must be NULL except in dws_sampler_run_program, where only
 *              the rows of jump visits are read.
 *   net_steps  HOST float[S];  coef  HOST float[3 or 5][S]
 *   noise      optional DEVICE [S, B, C, L]: noise[s] is z of step s.  NULL -> Philox keyed
 *              by (seed, s, element); a seed-driven x_T uses stream S.  With S = T, the
 *              training tables and net_steps = 0..T-1, DDPM is bit-identical to dws_sampler_run.
 *
 * With use_graph the captured step works on a model-owned state buffer and reads the seed
 * from device memory: x_T is copied (or drawn) in before the replays and x_0 copied out
 * after them, so a new seed or a new x needs no new capture.  One graph per (B, L, S, kind,
 * tables, step table, noise pointer); tap "sampler_graphs" counts the graphs a model has
 * instantiated (both entry points).  The multistep kind's history buffer is part of that key; whether a
 * step is second order is decided on the device, so its tables do not depend on the start step.  Bad input
 * (S < 1, non-finite steps or coefficients, DDIM k2 <= 0, DPM-Solver++ m2 <= 0 or m5 < 0 or a non-NULL
 * noise outside a program run) -> DWS_ERR_INVALID, before anything is enqueued. */
#define DWS_SAMPLER_DDPM 0
#define DWS_SAMPLER_DDIM 1
#define DWS_SAMPLER_DPMPP2M 2
int dws_sampler_run_schedule(dws_model* m, float* x, int32_t kind, int32_t S, const float* net_steps,
                             const float* coef, const float* noise, uint64_t seed, int32_t init_from_seed,
                             int32_t use_graph, void* stream);

/* Editing runs on the few-step entry (not the reference's loop): inpainting / continuation by
 * known-region replacement (Song et al., ICLR 2021, "imputation"; the base case of RePaint) and
 * a partial start (DiffWave's zero-shot denoising and latent interpolation, SDEdit).  Everything
 * dws_sampler_run_schedule takes means the same here; `edit` adds:
 *
 *   edit_coef    HOST float[4][S] = q1, q2, n1, n2 (sampling.edit_coefficients).  With level[s]
 *                the cumulative alpha_bar of step s of this run and p_s = level[s-1] (p_0 = 1)
 *                the level the state is at AFTER step s:  q1 = sqrt(p), q2 = sqrt(1 - p)
 *                (q1[0] = 1, q2[0] = 0), n1 = sqrt(level), n2 = sqrt(1 - level).
 *   known, mask  DEVICE float [B, C, L] and uint8 [B, C, L] (non-zero = known), both or neither.
 *                After the ordinary update of step s has produced v for an element:
 *                  if mask:  v = (s > 0) ? (q1[s] * known) + (q2[s] * zk) : known
 *                two products and one sum, each rounded once; at s = 0 the known samples come out
 *                bitwise equal to `known`.  Where mask is zero the element gets exactly the value
 *                dws_sampler_run_schedule would have written.
 *   known_noise  optional DEVICE [S, B, C, L]: known_noise[s] is zk of step s (s > 0).  NULL ->
 *                Philox.
 *   start_step   s0 in 0 .. S-1: steps s0 .. 0 run (s0 + 1 network evaluations).  S-1 = a whole run.
 *   start_mode   DWS_START_AS_GIVEN: x is the state at step s0 (with s0 = S-1: x_T).
 *                DWS_START_QSAMPLE: x holds clean audio and the run first forms
 *                  x = (n1[s0] * x) + (n2[s0] * z0)       (same rounding rule)
 *   start_noise  optional DEVICE [B, C, L]: z0.  NULL -> Philox.  Only with DWS_START_QSAMPLE.
 *
 * Philox streams of a run, normal4(seed, stream, group of four along the flattened [B, C, L]):
 * the update noise of step s is stream s and a drawn x_T stream S, as in dws_sampler_run_schedule;
 * the known-region noise after step s is stream S + 1 + s; the start noise is stream 2S + 1.  No
 * stream is used twice in a run.
 *
 * With use_graph, `known` and `mask` are copied into model-owned buffers before the replays (like
 * x), q1 / q2 sit on the device beside the update tables, keyed on their contents, and
 * start_step only sets the initial value of the device step counter and the number of replays; the
 * q-sample runs once before the replays.  So a new seed, x, known clip, mask or start step REPLAYS
 * the graph captured for that (B, L, S, kind, tables, step table, noise / known_noise pointers,
 * replacement on / off); another of those captures anew.  The step with the replacement is a graph
 * of its own beside the unedited one (a call without known / mask replays dws_sampler_run_schedule's
 * graph), so the two kinds of call alternate without a capture; tap "sampler_graphs" counts both.
 * Bad input -> DWS_ERR_INVALID: start_step outside 0 .. S-1, known without mask or the reverse,
 * known_noise without known, non-finite or missing edit coefficients, DWS_START_QSAMPLE or a
 * start_step other than S-1 together with init_from_seed, start_noise without DWS_START_QSAMPLE. */
#define DWS_START_AS_GIVEN 0
#define DWS_START_QSAMPLE  1
typedef struct dws_sampler_edit {
    const float*   edit_coef;     /* HOST   float[4][S] */
    const float*   known;         /* DEVICE float[B, C, L] or NULL */
    const uint8_t* mask;          /* DEVICE uint8[B, C, L] or NULL */
    const float*   known_noise;   /* DEVICE float[S, B, C, L] ([V, B, C, L] in a program run) or NULL */
    const float*   start_noise;   /* DEVICE float[B, C, L] or NULL */
    int32_t        start_step;
    int32_t        start_mode;
} dws_sampler_edit;
int dws_sampler_run_edit(dws_model* m, float* x, int32_t kind, int32_t S, const float* net_steps,
                         const float* coef, const float* noise, uint64_t seed, int32_t init_from_seed,
                         int32_t use_graph, const dws_sampler_edit* edit, void* stream);

/* Classifier-free guidance (Ho & Salimans, 2021) inside the step of dws_sampler_run_schedule.  on != 0: the model is
 * prepared for 2 Bc clips and carries labels[2 Bc] -- by convention the wanted classes in the first half and the null class
 * in the second (the engine does not look at them) -- while x is [Bc, C, L] and noise [S, Bc, C, L].  The state is doubled
 * inside the model; per step: (1) the network on the doubled state; (2) over the first half of eps, each operation rounded
 * once, no contraction:   d = eps_c - eps_u;   g = scale * d;   eps = eps_c + g;   (3) the update kernel of the kind,
 * unchanged, over the first half's Bc C L elements -- Philox element indices, injected noise rows and the multistep
 * history are those of a plain Bc run (a drawn x_T is stream S over Bc C L elements); (4) a copy of the first half of the
 * state into the second.  One linear chain of nodes; `scale` lives in the device state, so a new scale, seed, x or label
 * set replays the graph (a graph of its own beside the others).  scale = 0 is the conditional run.
 * While on: dws_sampler_run, _steps, _run_edit and _run_program, and an odd prepared batch, return DWS_ERR_UNSUPPORTED.
 * on == 0 restores every other path bit for bit.  A non-finite scale -> DWS_ERR_INVALID. */
int dws_sampler_set_cfg(dws_model* m, int32_t on, float scale);

/* RePaint's resampling (Lugmayr et al., CVPR 2022) on the editing entry: a PROGRAM of V visits in place of the countdown
 * s0 .. 0, so that the chain can walk back up a few steps and down again and the generated part is harmonised with the
 * kept part.  Everything dws_sampler_run_edit takes means the same here; `edit` must carry known and mask.
 *
 * Positions: the state is at position k in 0 .. S with level P[k], P[0] = 1, P[k] = level[k-1] (the p of edit_coef
 * extended by P[S]); reverse step s takes it from position s+1 to s.  The run starts at K = start_step + 1.
 *
 *   visit_step   HOST int32[V] in execution order; entry i is visit number v = V-1-i (visits count down like steps).
 *                  s >= 0  reverse visit at step s: dws_sampler_run_edit's step s unchanged in arithmetic and operation
 *                          order -- the network at step-table row s, the update with tables row s, then where mask
 *                          v = (s > 0) ? (q1[s] * known) + (q2[s] * zk) : known
 *                  -j < 0  jump visit from the position k reached up to k + j: no network; the whole state, known
 *                          region included, becomes   x = (ja * x) + (jb * z)
 *                          two products and one sum, each rounded once -- one draw of the forward process' exact
 *                          marginal q(x_{k+j} | x_k), equal in distribution to j single forward steps.
 *   jump_coef    HOST float[2][V] = ja, jb indexed by v (sampling.jump_coefficients): ja = sqrt(P[k+j] / P[k]),
 *                jb = sqrt(1 - P[k+j] / P[k]) in float64 from the float32 levels, rounded once; zero on reverse visits.
 *   noise        optional DEVICE [V, B, C, L]: row v is the update noise of reverse visit v or z of jump visit v.
 *   edit->known_noise  optional DEVICE [V, B, C, L]: row v is zk of reverse visit v.
 *
 * Philox streams, normal4(seed, stream, group): visit v (update noise of a reverse visit, z of a jump visit) is stream
 * v; the known-region noise after reverse visit v is stream V + 1 + v; a drawn x_T is stream V; the start noise is stream
 * 2V + 1.  No stream is used twice, and a step that is visited again draws fresh noise.  The program s0 .. 0 has v = s
 * and reproduces dws_sampler_run_edit bit for bit; over a whole run (V = S) every stream id coincides too, with a partial
 * start V = s0 + 1 < S numbers the known-region and start streams differently (bit-equal with injected noise).
 *
 * The device state holds the visit number beside the step word; the last block of every visit's kernel writes
 * visit = v - 1 and step = step_of[v - 1] from a device table, so nothing crosses between host and device inside a run
 * and the network reads row *step of the step table as before.  The host enqueues the visits in order: a reverse visit
 * is a replay of the resampling step (forward + update + replacement), a graph of its own beside the unedited and the
 * edited one; a jump visit is one kernel launch between the replays.  step_of and ja / jb sit in a model-owned buffer
 * keyed on their contents: a new seed, x, known clip, mask, start step or program of the same V REPLAYS the graph, and
 * calls of the three kinds alternate on one model without a capture (tap "sampler_graphs" counts all three).
 * use_graph = 0 does the same walk with direct launches.
 * Bad input -> DWS_ERR_INVALID, before anything is enqueued: what dws_sampler_run_edit rejects; known / mask missing;
 * V < 1; a program that is no walk (the first reverse visit is not start_step, a reverse visit is not one below the
 * position reached, a jump lands above K, the last visit is not reverse step 0); ja or jb not finite or ja <= 0. */
int dws_sampler_run_program(dws_model* m, float* x, int32_t kind, int32_t S, const float* net_steps,
                            const float* coef, int32_t V, const int32_t* visit_step, const float* jump_coef,
                            const float* noise, uint64_t seed, int32_t init_from_seed, int32_t use_graph,
                            const dws_sampler_edit* edit, void* stream);

/* x[0 .. n) (DEVICE) = Philox stream `stream_id` of `seed` exactly as the samplers draw it: normal4(seed, stream_id, g)
 * gives elements 4g .. 4g+3.  For checking the stream assignment of a seeded run from outside. */
int dws_philox_normal(float* x, int64_t n, uint64_t seed, uint32_t stream_id, void* stream);

/* Per-clip seeds: a clip's noise depends on (its own seed, the stream, the element's position inside the clip) alone --
 * not on the batch size, the clip's place in the batch or the number of devices a run is spread over.  seeds: HOST
 * uint64[B], or NULL = off (the scalar `seed` of the run entries, every path bit for bit as without this call).  The table
 * goes through pinned staging into a model-owned device buffer on `stream` (the host does not wait for the GPU) and holds
 * until it is changed; dws_model_prepare to another shape drops it.  While it is on, the `seed` argument of
 * dws_sampler_run_schedule, _run_edit and _run_program is ignored, and B must be the number of clips of the sampler state
 * -- the prepared batch, or half of it under dws_sampler_set_cfg (the noise covers the first half's Bc clips) -- else the
 * run entry returns DWS_ERR_INVALID before anything is enqueued.
 *
 * Numbering, with n_c = C L: element e in 0 .. n_c-1 of clip b is component e % 4 of normal4(seeds[b], stream, e / 4);
 * the stream ids are those above (s, S, S + 1 + s, 2S + 1; v, V, V + 1 + v, 2V + 1 in a program run).  So clip b of a
 * per-clip run is bit-equal to the scalar-seed run at B = 1 with seed = seeds[b].  Every kernel that draws (x_T, the
 * update noise, the known-region noise, the jump noise, the start noise) has a per-clip instance that runs on a grid with
 * one row per clip, each row with its clip's seed and its groups counted from the clip's first element; with
 * n_c % 4 == 0 (and 16-byte aligned noise tensors) a group is one float4 per array and the four mask bytes one word as
 * before, otherwise the element-wise path runs bounded by n_c.  The scalar-seed instances are not touched.
 *
 * The captured steps read the table from device memory: a new table replays the graph.  The per-clip step is a graph of
 * its own beside the scalar-seed one of its flavour (still one linear chain of nodes), so calls of the two forms alternate
 * on one model without a new capture once both have run.
 * While on: dws_sampler_run and dws_sampler_steps return DWS_ERR_UNSUPPORTED (dws_sampler_run_schedule with
 * net_steps = 0 .. T-1 is bit-identical to dws_sampler_run).  B outside 1 .. 65535 -> DWS_ERR_INVALID; before
 * dws_model_prepare -> DWS_ERR_STATE. */
int dws_sampler_set_clip_seeds(dws_model* m, const uint64_t* seeds, int64_t B, void* stream);

/* Adaptive prior (PriorGrad: Lee et al., ICLR 2022): the run ends in N(0, diag(sigma^2)) instead of N(0, I).  sigma: DEVICE
 * float[B, n_per_clip] at the shape of the sampler state (n_per_clip = C L; a [B, 1, L] table of a C > 1 model is expanded
 * by the caller), every value finite and > 0 over the positions a run keeps -- or NULL = off, every path bit for bit as
 * without this call.  The table is copied into a model-owned device buffer on `stream` and holds until it is changed;
 * dws_model_prepare to another shape drops it.
 *
 * While it is on, every standard-normal number z a schedule run consumes is replaced by n = sigma * z at its own
 * position -- ONE fp32 product of its own, rounded once, never contracted into what follows -- and n stands exactly where
 * z stood; the update formulas are unchanged.  This holds for numbers drawn from Philox and for INJECTED ones (`noise`,
 * `known_noise`, `start_noise` stay standard normal by contract) at every noise site: the drawn x_T (an injected x_T is a
 * state and is taken as given), the update noise of DDPM and of DDIM with eta > 0, the known-region noise of an edited
 * step, the jump visits of a program and the q-sample start.  DPM-Solver++(2M) draws no update noise: only its drawn x_T
 * (and, edited, its known-region, jump and start noise) changes.  So a run with the table on equals the run without it that
 * is handed x_T = fp32(sigma z_S) and noise[s] = fp32(sigma z_s), bit for bit.  It combines with per-clip seeds (the
 * table's row b belongs to clip b) and per-clip lengths (the update is pointwise: a value past a clip's end reaches no
 * valid position).
 *
 * The scaling kernels are instances of their own (a PRIOR template flag); with no table installed the existing instances
 * run as they are.  The captured steps read the table from the model-owned buffer: a new table of the same shape replays
 * the graph.  The step with a prior is a graph of its own beside the one without, per flavour, form of seed and lengths
 * on / off: the forms alternate on one model without a new capture once each has run.
 * While on: dws_sampler_run and dws_sampler_steps return DWS_ERR_UNSUPPORTED, and so does dws_sampler_set_cfg(on); with
 * guidance on, this call returns DWS_ERR_UNSUPPORTED (guidance with a prior is not built).  B or n_per_clip other than the
 * prepared state's -> DWS_ERR_INVALID; before dws_model_prepare -> DWS_ERR_STATE. */
int dws_sampler_set_prior(dws_model* m, const float* sigma, int64_t B, int64_t n_per_clip, void* stream);

/* The per-clip twin of dws_philox_normal: row b of x[B, n_per_clip] (DEVICE) = dws_philox_normal(n_per_clip, seeds[b],
 * stream_id), seeds HOST uint64[B].  The seeds travel as kernel arguments; the host does not wait for the GPU. */
int dws_philox_normal_clips(float* x, int64_t B, int64_t n_per_clip, const uint64_t* seeds, uint32_t stream_id,
                            void* stream);

/* Mel-spectrogram front-end of the vocoding path: TacotronSTFT.mel_spectrogram
 * (`dataloaders/stft.py:196-244`) as called by Mel2Samp.get_mel (`dataloaders/mel2samp.py:76-82`) and
 * generate.py:147-153.  audio [B][T] in [-1, 1]; window [n_fft] (the Hann window, centre-padded to
 * filter_length, `stft.py:122-129`); mel_basis [n_mels][n_fft/2+1] (`stft.py:203-210`); out
 * [B][n_mels][T/hop + 1] = log(max(mel_basis . |STFT|, clip)).  All pointers are device pointers. */
int dws_mel_spectrogram(const float* audio, int64_t B, int64_t T, const float* window, const float* mel_basis,
                        int32_t n_fft, int32_t hop, int32_t n_mels, float clip, float* out, void* stream);

/* The standard deviation of the adaptive prior from a clip's own conditioning mel (PriorGrad, Lee et al., ICLR 2022, as
 * formulated for a mel-conditional vocoder).  mel [B][bands][frames] is the log-mel above (natural log); with hop samples
 * per frame
 *   energy[b, f]  = sqrt(sum_k exp(mel[b, k, f]))                 (fp32, in a fixed order: band k into partial sum k % 8
 *                                                                  in ascending k, then ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)))
 *   sigma_f[b, f] = clamp((energy[b, f] - e_min) / (e_max - e_min), std_min, 1)
 *   sigma[b, 0, l] = sigma_f[b, l / hop]                          l = 0 .. L-1
 * Each frame is evaluated on its own: no statistic is taken over the batch or the utterance, so a clip's row does not
 * depend on B.  sigma is [B][1][L]; the repeat by hop is written with 16-byte stores where the address allows.  All
 * pointers are device pointers.  L outside 1 .. frames * hop, e_max <= e_min or not finite, std_min outside (0, 1] ->
 * DWS_ERR_INVALID. */
int dws_prior_std_from_mel(const float* mel, int64_t B, int64_t bands, int64_t frames, int64_t hop, int64_t L, float e_min,
                           float e_max, float std_min, float* sigma, void* stream);

/* The adjoint of dws_mel_spectrogram (not in the reference, whose TacotronSTFT detaches its input): daudio [B][T]
 * (overwritten) = d<dout, out>/d audio for a cotangent dout [B][n_mels][T/hop + 1].  With N = n_fft, w the window, W the
 * filterbank, rho the reflect map of the forward (j < 0 -> -j, j >= T -> 2(T-1) - j), the forward is
 *     frame_f[i] = w[i] x[rho(f hop + i - N/2)]
 *     Re_k = sum_i frame_f[i] cos(2 pi i k / N),   Im_k = sum_i frame_f[i] sin(2 pi i k / N),   k = 0 .. N/2
 *     mag_k = sqrt(Re_k^2 + Im_k^2),   s_m = sum_k W[m,k] mag_k,   out[m,f] = log(max(s_m, clip))
 * and the adjoint computed here
 *     ds_m   = dout[m,f] / s_m  if s_m > clip  else 0
 *     dmag_k = sum_m W[m,k] ds_m
 *     dRe_k  = dmag_k Re_k / mag_k,   dIm_k = dmag_k Im_k / mag_k          (both 0 where mag_k == 0)
 *     dframe_f[i] = sum_k (dRe_k cos(2 pi i k / N) + dIm_k sin(2 pi i k / N))
 *     daudio[j] = sum over all (f, i) with rho(f hop + i - N/2) = j  of  w[i] dframe_f[i].
 * Zero magnitude: mag_k == 0 contributes exactly 0 -- a deliberate difference from torch autograd, which returns NaN
 * there (sqrt has no gradient at 0); a silent frame gives a zero gradient, not NaN.  Clamp tie: s_m == clip counts as
 * clamped (gradient 0).  Re, Im and s_m are recomputed with the forward's own arithmetic, so the clamp decision is the
 * forward's.  The overlap-add is a gather in a fixed order (per sample: its direct position, its left reflection, its
 * right reflection, each in ascending frame order) with no atomics: the result is bitwise reproducible, and clip b's
 * gradient does not depend on B or on b.
 * workspace: DEVICE [B][T/hop + 1][n_fft] floats owned by the caller (overwritten; the library allocates nothing per
 * call).  Same limits and error codes as dws_mel_spectrogram (null pointer, workspace included, or B, hop, n_mels < 1 or
 * T <= n_fft/2: DWS_ERR_INVALID; n_fft not a power of two in 64..4096: DWS_ERR_UNSUPPORTED), and DWS_ERR_UNSUPPORTED
 * where 3 n_fft + 3 (n_fft/2 + 1) + n_mels floats exceed the 160 KiB of LDS of a workgroup. */
int dws_mel_spectrogram_backward(const float* audio, int64_t B, int64_t T, const float* window, const float* mel_basis,
                                 int32_t n_fft, int32_t hop, int32_t n_mels, float clip, const float* dout, float* daudio,
                                 float* workspace, void* stream);

/* Objective spectral distances between two batches of waveforms (not in the reference): x (generated) and y
 * (reference), both DEVICE float32 [B][T], compared at ONE STFT resolution in one fused launch -- no spectrogram goes to
 * memory.  Framing is dws_mel_spectrogram's (= torch.stft(center=True, pad_mode="reflect")) with a length per clip: with
 * len_b = lengths[b] (T where lengths is null), N = n_fft, w = window [N] (DEVICE; a periodic Hann window of win <= N
 * points centred in N), rho_b the reflect map about the clip's OWN ends (j < 0 -> -j, j >= len_b -> 2(len_b-1) - j),
 *     frame_f[i] = w[i] s[rho_b(f hop + i - N/2)]          f = 0 .. len_b / hop,   s = x or y
 *     Re_k, Im_k = sum_i frame_f[i] (cos, sin)(2 pi i k / N)                        k = 0 .. N/2   (K = N/2 + 1 bins)
 *     |S|_k = sqrt(max(Re_k^2 + Im_k^2, 1e-7))                                      (Parallel WaveGAN's floor)
 * out [B][6] (DEVICE, double) receives the clip's sums over its frames (and bins):
 *     out[b][0] = sum (|Y| - |X|)^2          out[b][1] = sum |Y|^2                  (spectral convergence = sqrt(0 / 1))
 *     out[b][2] = sum |ln|Y| - ln|X||                                               (log-magnitude L1)
 *     out[b][3] = sum_f sqrt(mean_k (log10|Y|^2 - log10|X|^2)^2)                    (log-spectral distance)
 * With mel_basis [n_mels][K] (DEVICE, float32) and m(S)_f = ln(max(mel_basis . sqrt(Re^2 + Im^2), clip)) -- unfloored
 * magnitudes, the formula of dws_mel_spectrogram --
 *     out[b][4] = sum |m(Y) - m(X)|                                                 (over bands and frames)
 * and with cep [n_cep][n_mels] (DEVICE, DOUBLE; needs mel_basis; n_cep <= 256)
 *     out[b][5] = sum_f || cep . (m(Y)_f - m(X)_f) ||_2 ;
 * out[b][4] / out[b][5] are 0 without the respective table (null pointer, and then n_mels / n_cep = 0).
 * Order of summation: bins within a thread ascending (thread t owns k = t, t + 256, ...), lanes of a wave by an xor tree
 * (fp32), the four waves in wave order, then a clip's frames in ascending order (double); the band logarithms and the
 * cepstral products are taken in double.  The result is bitwise reproducible, and clip b's six numbers depend on its own
 * len_b samples alone: not on B, T, b or on anything stored behind len_b (which is never read and may be NaN).
 * lengths: DEVICE int32 [B] or null; lengths_host: the same numbers on the HOST (both or neither) -- they are checked
 * there, nothing waits for the GPU.  workspace: DEVICE, dws_spectral_distance_workspace(B, T, hop) bytes
 * ([B][T/hop + 1][6] doubles) owned by the caller (overwritten; the library allocates nothing per call).
 * DWS_ERR_INVALID: a null x, y, window, workspace or out; n_fft not a power of two in 64 .. 2048; hop < 1; B outside
 * 1 .. 65535; a len_b outside n_fft/2 + 1 .. T (reflect padding; no length is clamped); tables and counts that do not
 * match as stated above. */
int dws_spectral_distance(const float* x, const float* y, int64_t B, int64_t T, const int32_t* lengths,
                          const int32_t* lengths_host, const float* window, int32_t n_fft, int32_t hop,
                          const float* mel_basis, int32_t n_mels, float clip, const double* cep, int32_t n_cep,
                          double* workspace, double* out, void* stream);

/* Bytes of dws_spectral_distance's workspace; 0 for a shape it refuses. */
int64_t dws_spectral_distance_workspace(int64_t B, int64_t T, int32_t hop);

/* The adjoint of dws_spectral_distance's first three sums with respect to the generated signal x (not in the reference):
 * what a multi-resolution STFT training loss (Parallel WaveGAN's spectral convergence + log-magnitude L1) needs at ONE
 * resolution.  dws_spectral_distance is the forward.  With its notation (frame_f, rho_b, Re / Im with +sin, p = Re^2 +
 * Im^2, |S| = sqrt(max(p, 1e-7)), l = ln|Y| - ln|X|), and for clip b the two numbers coef[b][0], coef[b][1] (DEVICE,
 * DOUBLE [B][2]: the cotangents of out[b][0] and out[b][2] up to the factors the caller's loss puts on them -- for
 * sc = sqrt(out0 / out1) and mag = out2 / (frames K): g_sc / sqrt(out0 out1) and g_mag / (frames K)):
 *     dmag_k   = -(coef[b][0] (|Y|_k - |X|_k) + coef[b][1] sgn(l_k) / |X|_k)      where p_x >= 1e-7, else 0  (sgn(0) = 0)
 *     dRe_k    = dmag_k Re_k / |X|_k,    dIm_k = dmag_k Im_k / |X|_k               (X's Re / Im)
 *     dframe_f[i] = w[i] sum_k (dRe_k cos(2 pi i k / N) + dIm_k sin(2 pi i k / N)) (k = 0 .. N/2 ascending, each bin once)
 *     dx[b][j] = sum over all (f, i) with rho_b(f hop + i - N/2) = j  of  dframe_f[i]          (j < len_b)
 * Floor: a bin of X below the floor passes no gradient, the tie p_x == 1e-7 passes it (clamp_min's rule); Re, Im and the
 * floor decisions are recomputed with the forward's own arithmetic.  A silent x (p_x = 0 everywhere) so has an exactly
 * zero gradient, and so has x == y with coef[b][0] = 0 (the caller's convention where out[b][0] == 0; torch autograd
 * through the square root gives NaN there).
 * dx: DEVICE [B][T].  accumulate == 0: positions j < len_b are overwritten, positions j >= len_b are written as exactly 0;
 * accumulate != 0: positions j < len_b are added to, the others are left untouched.
 * Order of summation: a sample of a frame over k ascending (fp32 fmaf, cos term then sin term); the overlap-add is a
 * gather in a fixed order (per sample: its direct position, its left reflection, its right reflection about len_b, each
 * in ascending frame order) with no atomics.  The result is bitwise reproducible, and row b depends on clip b's own len_b
 * samples and coef[b] alone: not on B, T, b or on anything stored behind len_b (never read; may be NaN).
 * workspace: DEVICE, dws_spectral_loss_backward_workspace(B, T, n_fft, hop) bytes ([B][T/hop + 1][n_fft] floats) owned by
 * the caller (overwritten; the library allocates nothing per call).  LDS per workgroup: 16 n_fft + 8 (n_fft/2 + 1) bytes.
 * DWS_ERR_INVALID: as dws_spectral_distance (a null x, y, window, coef, dx or workspace; n_fft not a power of two in
 * 64 .. 2048; hop < 1; B outside 1 .. 65535; a len_b outside n_fft/2 + 1 .. T; lengths without lengths_host). */
int dws_spectral_loss_backward(const float* x, const float* y, int64_t B, int64_t T, const int32_t* lengths,
                               const int32_t* lengths_host, const float* window, int32_t n_fft, int32_t hop,
                               const double* coef, float* dx, int32_t accumulate, float* workspace, void* stream);

/* Bytes of dws_spectral_loss_backward's workspace; 0 for a shape it refuses. */
int64_t dws_spectral_loss_backward_workspace(int64_t B, int64_t T, int32_t n_fft, int32_t hop);

/* Pitch track of a batch of waveforms (not in the reference): s DEVICE float32 [B][T], YIN (de Cheveigne & Kawahara,
 * 2002) with a fixed threshold, one workgroup per frame.  With len_b = lengths[b] (T where lengths is null), W = win,
 * M = tau_hi + 1 (the largest lag computed: the chosen lag always has a right neighbour), S = W + M, rho_b the reflect map
 * about the clip's OWN ends as in dws_spectral_distance, and frames f = 0 .. len_b / hop (its frame count at that hop):
 *     u_f[i] = s[rho_b(f hop - S/2 + i)]                          i = 0 .. S-1
 *     d(tau) = sum_{j=0}^{W-1} (u_f[j] - u_f[j + tau])^2          tau = 1 .. M,   d(0) = 0
 *     d'(tau) = d(tau) tau / sum_{t=1}^{tau} d(t)                 (1 where the sum is 0; d'(0) = 1)
 * Decision: the smallest tau in [tau_lo, tau_hi] with d'(tau) < threshold, then tau <- tau + 1 while tau + 1 <= tau_hi and
 * d'(tau + 1) < d'(tau); the result is tau*.  If there is one the frame is voiced: with a, b, c = d'(tau* - 1), d'(tau*),
 * d'(tau* + 1), delta = (a - c) / (2 (a - 2b + c)) where a - 2b + c > 0 and |delta| <= 1, else 0:
 *     f0 = sampling_rate / (tau* + delta),    periodicity = clamp(1 - b, 0, 1);
 * otherwise it is unvoiced: f0 = 0, periodicity = clamp(1 - min_{tau_lo..tau_hi} d', 0, 1).  Digital silence is unvoiced
 * with periodicity 0.  track [B][T/hop + 1][2] (DEVICE, float32) receives (f0, periodicity); frames behind a clip's last
 * are written as exactly (0, 0).
 * Arithmetic and order of summation: d(tau) is the direct sum of squares of exact differences in fp32 (never energy -
 * 2 autocorrelation, which cancels at the minimum that decides).  A work item owns lags 4g .. 4g + 3 and one of
 * P = max(1, 256 / G) contiguous parts of the 4-sample blocks of j (G = (M + 4) / 4; the last part also takes the
 * W mod 4 samples that are left); it adds its j in ascending order (fmaf), and the parts are added in ascending order.
 * Everything after that is double -- the prefix sum (thread t of 256 owns ceil(M / 256) consecutive lags serially, an
 * inclusive scan over the lanes of a wave, the four waves in wave order), d', every comparison (threshold is widened
 * from the float32 it travels as) and the interpolation -- and the two outputs are rounded to float32.  The decision is
 * three min reductions; there are no atomics.  The result is bitwise reproducible, and clip b's rows depend on its own
 * len_b samples alone: not on B, T, b or on anything stored behind len_b (never read; may be NaN).  Scaling s by a power
 * of two changes no bit of the track.
 * lengths / lengths_host: as dws_spectral_distance (DEVICE and HOST copies of the same numbers, both or neither; the
 * host copy is checked, nothing waits for the GPU; a device value the host did not admit makes its clip an empty one).
 * LDS per workgroup: 4 (S + 16 .. 19 + 4 G P) + 8 (4G + 10) bytes (at most 41 KiB).
 * DWS_ERR_INVALID: a null s or track; win outside 64 .. 2048; tau_lo < 2, tau_lo >= tau_hi or tau_hi + 1 > 2048;
 * hop < 1; threshold outside (0, 1); sampling_rate <= 0; B outside 1 .. 65535; a len_b outside (S + 1) / 2 + 1 .. T
 * (reflect padding; no length is clamped); lengths without lengths_host. */
int dws_pitch_track(const float* s, int64_t B, int64_t T, const int32_t* lengths, const int32_t* lengths_host, int32_t hop,
                    int32_t win, int32_t tau_lo, int32_t tau_hi, float threshold, double sampling_rate, float* track,
                    void* stream);

/* Pitch distances between two batches of waveforms (not in the reference): the tracks of x (generated) and y (reference)
 * as dws_pitch_track computes them, in one launch, and the sums of a clip over its frames in ascending order in double.
 * With v_x, v_y the voicing flags (f0 > 0), vv = both voiced and p the periodicity, out [B][8] (DEVICE, double):
 *     out[b][0] = #vv                   out[b][1] = sum_vv (f0x - f0y)^2 [Hz^2]   out[b][2] = sum_vv (1200 log2(f0x / f0y))^2
 *     out[b][3] = #v_y                  out[b][4] = #v_x                          out[b][5] = #(v_x != v_y)
 *     out[b][6] = sum (p_x - p_y)^2     out[b][7] = #vv with |f0x / f0y - 1| > 0.2   (gross pitch errors)
 * workspace: DEVICE, dws_pitch_distance_workspace(B, T, hop) bytes (the two tracks, x's then y's, [2][B][T/hop + 1][2]
 * floats) owned by the caller (overwritten; the library allocates nothing per call).  Reproducibility, independence of a
 * clip from its batch and the error codes are dws_pitch_track's (and a null workspace or out: DWS_ERR_INVALID). */
int dws_pitch_distance(const float* x, const float* y, int64_t B, int64_t T, const int32_t* lengths,
                       const int32_t* lengths_host, int32_t hop, int32_t win, int32_t tau_lo, int32_t tau_hi,
                       float threshold, double sampling_rate, float* workspace, double* out, void* stream);

/* Bytes of dws_pitch_distance's workspace; 0 for a shape it refuses. */
int64_t dws_pitch_distance_workspace(int64_t B, int64_t T, int32_t hop);

/* Sample-rate conversion by the rational factor U / D (not in the reference; U = sr_out / g, D = sr_in / g, g their gcd):
 * a polyphase FIR resampler.  x [B][T] (DEVICE float32), h [taps] = h[0 .. 2 half] (DEVICE float32; an odd count, gain U,
 * designed by the caller).  With len_b = lengths[b] (T where lengths is null) clip b has out_len_b = ceil(len_b U / D)
 * output samples
 *     y[b][m] = sum_i x[b][i] h[m D - i U + half]         over the i in 0 .. len_b - 1 whose tap index lies in 0 .. 2 half
 * (about taps / U products per output; nothing is zero-stuffed).  This is scipy.signal.resample_poly(x, U, D,
 * window=h / U).  y is [B][T_out] with T_out >= the largest out_len_b; positions m >= out_len_b are written as exactly 0.
 * Order of summation: fp32 fmaf from 0 with i ascending.  One workgroup per clip and tile of dws_resample_tile() output
 * positions, the table and the tile's input span in LDS, no atomics: the result is bitwise reproducible, and row b
 * depends on clip b's own len_b samples alone: not on B, T, b or on anything stored behind len_b (never read; may be NaN).
 * U == D == 1 copies the len_b samples bit for bit (h is not read).
 * lengths / lengths_host: as dws_spectral_distance (DEVICE and HOST copies of the same numbers, both or neither; the
 * host copy is checked, nothing waits for the GPU; a device value the host did not admit makes its clip an empty one).
 * DWS_ERR_INVALID: a null x, h or y; an even tap count; U or D < 1; B outside 1 .. 65535; T < 1; a len_b outside
 * 1 .. T; T_out below the largest out_len_b; lengths without lengths_host.  DWS_ERR_UNSUPPORTED, with a message naming the
 * ratio: more than 16384 taps, or a D / U so large that the (1023 D + taps - 1) / U + 2 input samples of a tile exceed
 * the 16384 that fit in LDS. */
int dws_resample(const float* x, int64_t B, int64_t T, const int32_t* lengths, const int32_t* lengths_host, const float* h,
                 int32_t taps, int32_t U, int32_t D, float* y, int64_t T_out, void* stream);
/* Output positions per workgroup of dws_resample (tests put shapes on both sides of it). */
int dws_resample_tile(void);

/* Short-time objective intelligibility of x (generated) against y (the clean reference), STOI (Taal et al. 2011) and
 * ESTOI (Jensen & Taal 2016); not in the reference.  x, y [B][T] DEVICE float32 at the rate the band matrix is built for
 * (10 kHz in the papers).  Taal's constants are arguments: frame 256, hop 128, n_fft 512, 15 third-octave bands, segment
 * N = 30 frames, beta = -15 dB, dyn_range = 40 dB.  window [frame] (DEVICE float32; hanning(frame + 2)[1:-1]), obm
 * [n_bands][n_fft/2 + 1] (DEVICE float32, entries >= 0; 0 / 1 for third-octave bands).  eps = DBL_EPSILON.  Per clip, with
 * len_b = lengths[b] (T where lengths is null) and w = window:
 *  1. Silent frames, decided by y alone: frames j = 0 .. (len_b - frame) / hop, e_j = 20 log10(||w y_j|| + eps); frame j
 *     is kept where e_j > max_j e_j - dyn_range.  The kept windowed frames of both signals, K of them, are overlap-added
 *     at `hop` in their order; the compacted signals are never stored -- frame k of one (k = 0 .. K - 1) is
 *         c_k[n] = sum_{k'} w[i] s[idx[k'] hop + i],   i = n + (k - k') hop in 0 .. frame - 1,   |k - k'| <= (frame - 1) / hop
 *     over the list idx of kept frames (a fixed-order prefix sum over the keep flags).
 *  2. Band magnitudes: S_k = the n_fft-point DFT of w c_k (its `frame` samples; only bins some band uses),
 *         X[k][j] = sqrt(sum_q obm[j][q] |S_k[q]|^2)        of x, Y[k][j] of y.
 *  3. For every segment m = 0 .. K - N of N consecutive frames, per band j, with x, y the N values of that band:
 *         alpha = ||y|| / (||x|| + eps),   x' = min(alpha x, (1 + 10^(-beta / 20)) y),
 *         d_mj = sum ((x' - mean x') / (||x' - mean x'|| + eps)) ((y - mean y) / (||y - mean y|| + eps));
 *     ESTOI, no clipping: the rows (bands) of both [n_bands][N] blocks made zero-mean and divided by (norm + eps) over
 *     time, then the columns (frames) over bands, d_m = (1 / N) sum of the N column inner products.
 * out [B][4] (DEVICE, double): sum_{m, j} d_mj, sum_m d_m, the number of segments M = max(K - N + 1, 0) and K.  The caller
 * divides (STOI = out0 / (M n_bands), ESTOI = out1 / M); K < N gives M = 0 and zero sums.
 * Arithmetic and order of summation: the frame energies, the overlap-add, the band sums and everything behind them are
 * double; the DFT is a direct fp32 sum (one thread per bin, fmaf over the samples ascending).  An energy and a band sum
 * are a lane's terms ascending (stride 64) and an xor tree over the wave; the maximum is exact; within a segment a band
 * sums its frames ascending and a frame its bands ascending, the bands and then the frames are added in ascending order,
 * and a clip's segments in ascending order.  No atomics: the result is bitwise reproducible, and clip b's four numbers
 * depend on its own len_b samples alone: not on B, T, b or on anything stored behind len_b (never read; may be NaN).
 * lengths / lengths_host: as dws_spectral_distance.  workspace: DEVICE, dws_stoi_workspace(B, T, frame, hop, n_bands) bytes
 * owned by the caller (overwritten; the library allocates nothing per call): with F = (T - frame) / hop + 1, doubles e
 * [B][F], bands [B][2][F][n_bands] (x then y), segments [B][F][2], then int32 idx [B][F] and kept [B].
 * DWS_ERR_INVALID: a null x, y, window, obm, workspace or out; n_fft not a power of two in 64 .. 2048; frame outside
 * 1 .. n_fft; hop < 1; segment outside 2 .. 128; n_bands outside 1 .. 64; B outside 1 .. 65535; a len_b outside
 * frame .. T; a dyn_range <= 0; lengths without lengths_host. */
int dws_stoi(const float* x, const float* y, int64_t B, int64_t T, const int32_t* lengths, const int32_t* lengths_host,
             const float* window, int32_t frame, int32_t hop, int32_t n_fft, const float* obm, int32_t n_bands,
             int32_t segment, double beta, double dyn_range, void* workspace, double* out, void* stream);

/* Bytes of dws_stoi's workspace; 0 for a shape it refuses. */
int64_t dws_stoi_workspace(int64_t B, int64_t T, int32_t frame, int32_t hop, int32_t n_bands);

/* Inverse short-time Fourier transform, STFT.inverse(magnitude, phase) of `dataloaders/stft.py:165-194` (=
 * torch.istft(center=True) of magnitude e^{i phase}), with a length per clip.  magnitude and phase are DEVICE float32
 * [B][K][f_max], K = n_fft/2 + 1 (the reference's layout); a null phase is phase 0.  The spectrum is the public one,
 * e^{-i theta}: X_k = sum_i frame[i] e^{-2 pi i k / N}, so Re_k = M_k cos(phase_k), Im_k = M_k sin(phase_k).  With
 * N = n_fft, w = window [N] (DEVICE; a periodic Hann window of win <= N points centred in N), len_b = lengths[b]
 * ((f_max - 1) hop where lengths is null; each a multiple of hop) and frames f = 0 .. len_b / hop of clip b:
 *     h_k = 1/N for k = 0 and k = N/2 (whose imaginary part does not enter, as irfft ignores it), 2/N otherwise
 *     row_f[i] = w[i] sum_k h_k (Re_k cos(2 pi i k / N) - Im_k sin(2 pi i k / N))         (k = 0 .. N/2 ascending)
 *     wss(p)   = sum_f w[p - f hop]^2,   s(p) = sum_f row_f[p - f hop]                    (the frames that cover p, ascending)
 *     out[b][j] = s(p) / wss(p) where wss(p) > FLT_MIN, else s(p),   p = j + N/2,  j < len_b
 * (the reference's `tiny` rule; its n_fft / hop factors cancel and do not appear).  out is [B][(f_max - 1) hop];
 * positions j >= len_b are written as exactly 0.  Frames behind a clip's own (f > len_b / hop) are never read and may
 * hold NaN.  No atomics, fixed order: the result is bitwise reproducible, and row b depends on clip b's own frames alone.
 * lengths / lengths_host: as dws_spectral_distance (DEVICE and HOST copies of the same numbers, both or neither; the
 * host copy is checked, nothing waits for the GPU).  workspace: DEVICE, dws_griffin_lim_workspace(B, f_max, n_fft, hop, 0)
 * bytes ([B][f_max][n_fft] floats) owned by the caller (overwritten; the library allocates nothing per call).
 * LDS per workgroup: 8 n_fft + 8 K bytes.
 * DWS_ERR_UNSUPPORTED: n_fft not a power of two in 64 .. 4096 (dws_mel_spectrogram's limits), or more LDS than a
 * workgroup has.  DWS_ERR_INVALID, the message naming the parameter and the clip: a null magnitude, window, out or
 * workspace; B outside 1 .. 65535; hop < 1; f_max < 2; a len_b outside n_fft/2 + 1 .. (f_max - 1) hop or not a multiple of
 * hop; lengths without lengths_host. */
int dws_istft(const float* magnitude, const float* phase, int64_t B, int64_t f_max, const int32_t* lengths,
              const int32_t* lengths_host, const float* window, int32_t n_fft, int32_t hop, float* out, float* workspace,
              void* stream);

/* Griffin-Lim phase reconstruction (`dataloaders/stft.py:66-82`; Griffin & Lim 1984) from the magnitudes M [B][K][f_max]
 * and initial phases phase0 (null: phase 0), shapes, framing, lengths and sign convention as dws_istft:
 *     x_0 = dws_istft(M, phase0),   y_0 = x_0
 *     iteration n = 1 .. n_iters:
 *       projection: X = STFT(y_{n-1}) (dws_mel_spectrogram's framing, reflected about the clip's OWN ends),
 *                   (Re_k, Im_k) <- (Re_k, Im_k) M_k / |X_k|,  (M_k, 0) where |X_k| == 0 exactly (phase atan2(0, 0) = 0),
 *       gather:     x_n = the normalised overlap-add of dws_istft on these rows,   y_n = x_n + momentum (x_n - x_{n-1})
 *     out = x_{n_iters}.
 * momentum = 0 is the reference's loop.  momentum > 0 is Fast Griffin-Lim (Perraudin, Balazs & Sondergaard 2013) stated
 * in the signal domain, which is exact because STFT . iSTFT is linear.  n_iters = 0 is dws_istft(M, phase0), bit for bit.
 * Two launches per iteration; no spectrogram of an iterate goes to memory.  Reproducibility and independence of a clip from
 * its batch are dws_istft's.  workspace: DEVICE, dws_griffin_lim_workspace(B, f_max, n_fft, hop, momentum != 0) bytes (the
 * rows, then y [B][(f_max - 1) hop] with momentum).  LDS per workgroup: 12 n_fft + 8 K bytes.
 * Error codes: dws_istft's, and DWS_ERR_INVALID for n_iters outside 0 .. 4096 or momentum outside [0, 1). */
int dws_griffin_lim(const float* magnitude, const float* phase0, int64_t B, int64_t f_max, const int32_t* lengths,
                    const int32_t* lengths_host, const float* window, int32_t n_fft, int32_t hop, int32_t n_iters,
                    float momentum, float* out, float* workspace, void* stream);

/* Bytes of the workspace of dws_griffin_lim (and, with momentum = 0, of dws_istft); 0 for a shape they refuse. */
int64_t dws_griffin_lim_workspace(int64_t B, int64_t f_max, int32_t n_fft, int32_t hop, int32_t momentum);

/* Time-varying spectral filter (the noise shaping of SpecGrad: Koizumi et al., Interspeech 2022; not in the reference):
 * out = G+ (F . G x), and with adjoint = 1 the exact transpose of that map.  G is the short-time DFT of
 * dws_mel_spectrogram's framing and G+ the normalised overlap-add of dws_istft; framing, lengths / lengths_host, sign
 * convention, window and workspace are dws_istft's.  x and out are DEVICE float32 [B][T], T = (f_max - 1) hop; filt_re and
 * filt_im DEVICE float32 [B][K][f_max], K = n_fft/2 + 1 (the layout of dws_istft's magnitude), one complex gain
 * F = filt_re + i filt_im per clip, bin and frame in the public convention X_k = sum_i frame[i] e^{-2 pi i k / N}; a null
 * filt_im is a real filter.  With N = n_fft, w = window, len_b and frames f = 0 .. len_b / hop as in dws_istft:
 *
 * adjoint = 0, two launches:
 *     frame_f[i] = w[i] x[b][reflect(f hop + i - N/2)]                          (reflected about the clip's OWN ends)
 *     X_k = sum_i frame_f[i] e^{-2 pi i k / N}                                  (k = 0 .. N/2, direct, ascending i)
 *     Re Y_k = fl(fl(Fr Re X_k) - fl(Fi Im X_k)),  Im Y_k = fl(fl(Fr Im X_k) + fl(Fi Re X_k))
 *     row_f, wss, s and out[b][j] = s(p) / wss(p) (the `tiny` rule) exactly as dws_istft on the spectrum Y
 * The complex product is four fp32 products, each rounded on its own, then one subtraction and one addition; nothing of
 * it is contracted into an fma, so the bits do not depend on the compiler.  (The kernel works on the conjugate spectrum,
 * Im_core = -Im; negation is exact, so the statement above holds bit for bit.)
 *
 * adjoint = 1 (x is the cotangent g), two launches:
 *     q(p) = g[b][j] / wss(p) where wss(p) > FLT_MIN, else g[b][j],  p = j + N/2, j < len_b;  q = 0 elsewhere
 *     row_f[i] = w[i] q(f hop + i)
 *     dRe_k = h_k sum_i row_f[i] cos(2 pi i k / N),  dIm_k = -h_k sum_i row_f[i] sin(2 pi i k / N)    (h_k as dws_istft;
 *                                                                                 dIm is exactly 0 at k = 0 and k = N/2)
 *     dX_k = conj(F_k) dY_k       (Re = fl(fl(Fr dRe) + fl(Fi dIm)), Im = fl(fl(Fr dIm) - fl(Fi dRe)), uncontracted)
 *     u_f[i] = w[i] sum_k (Re dX_k cos - Im dX_k sin)(2 pi i k / N)             (k = 0 .. N/2 ascending, no h weights)
 *     out[b][j] = the rows u_f folded back through the reflect map (the overlap-add of dws_spectral_loss_backward:
 *                 direct position, left reflection, right reflection, each in ascending frame order)
 * <dws_tv_filter(x, 0), g> = <x, dws_tv_filter(g, 1)> up to fp32 rounding, for every F.
 *
 * Positions j >= len_b of out are written as exactly 0 in both directions; x behind len_b and filter frames behind a clip's
 * own (f > len_b / hop) are never read and may hold NaN.  No atomics and a fixed summation order: the result is bitwise
 * reproducible, and row b depends on clip b alone, not on B or b.  No spectrogram goes to memory.  One workgroup of 256
 * threads per frame; LDS per workgroup: 12 n_fft + 8 K bytes.  The adjoint's frame kernel recomputes wss(p) for each of its
 * n_fft samples from the window in global memory, ceil(n_fft / hop) reads per sample at most: 4 at hop = n_fft/4, but n_fft
 * of them at hop = 1 (correct, and as slow as that reads).  workspace: DEVICE,
 * dws_griffin_lim_workspace(B, f_max, n_fft, hop, 0) bytes, owned by the caller (overwritten; nothing is allocated per call).
 * Error codes: dws_istft's (with x in the place of magnitude), and DWS_ERR_INVALID for a null filt_re or an adjoint
 * outside {0, 1}. */
int dws_tv_filter(const float* x, int64_t B, int64_t f_max, const int32_t* lengths, const int32_t* lengths_host,
                  const float* filt_re, const float* filt_im, const float* window, int32_t n_fft, int32_t hop,
                  int32_t adjoint, float* out, float* workspace, void* stream);

/* Pseudo-QMF filter bank of multi-band runs (Multi-band MelGAN, Yang et al. 2020; not in the reference).  Both entries
 * take the filter table filt [K][taps + 1] (DEVICE, float32; designed by the caller) and a gain, so that each also serves
 * as the other's adjoint.  K is 2 or 4, taps is even and in 2 .. 254, h = taps / 2.
 *
 * Analysis: x [B][T] -> out [B][K][T/K] (all DEVICE float32), T a positive multiple of K,
 *     out[b][k][t] = gain sum_{n=0}^{taps} filt[k][n] x[b][K t + n - h]              (x read as 0 outside [0, T))
 * Synthesis: s [B][K][Ts] -> out [B][K Ts], Ts >= 1,
 *     out[b][u] = gain sum_k sum_n filt[k][n] s[b][k][q]      over the n in 0 .. taps with u + n - h = K q, 0 <= q < Ts
 * (the polyphase form: about taps + 1 products per output sample; nothing is zero-stuffed).
 * Adjoints (rev(f)[k][n] = f[k][taps - n]): the adjoint of analysis (f, gain g) is synthesis (rev(f), g); the adjoint of
 * synthesis (f, g) is analysis (rev(f), g).
 * Order of summation: fp32 fmaf from 0, n ascending (analysis); n ascending and k ascending within an n (synthesis); the
 * gain multiplies the finished sum.  One workgroup per clip and tile of dws_pqmf_tile() full-band positions, no atomics:
 * the result is bitwise reproducible and clip b's rows depend on clip b alone, not on B or b.  A position outside the clip enters
 * its sum as an explicit product with 0, so zeros appended to every band of s change no output sample u < K Ts.
 * DWS_ERR_INVALID: a null x / s, filt or out; K outside {2, 4}; taps odd or outside 2 .. 254; T not a positive multiple
 * of K; Ts < 1; B outside 1 .. 65535. */
int dws_pqmf_analysis(const float* x, int64_t B, int64_t T, const float* filt, int32_t K, int32_t taps, float gain,
                      float* out, void* stream);
int dws_pqmf_synthesis(const float* s, int64_t B, int64_t Ts, const float* filt, int32_t K, int32_t taps, float gain,
                       float* out, void* stream);
/* Full-band positions per workgroup of the two kernels (tests put shapes on both sides of it). */
int dws_pqmf_tile(void);

/* The arithmetic of precision="bf16x6" alone (accuracy tests; not a tuned GEMM): C[M][N] = A[M][K] . B[K][N], row-major
 * fp32 device tensors, every operand split into three bf16 terms in registers, six bf16 MFMA products per term pair
 * accumulated in fp32 -- exactly what the bf16x6 layer kernels execute per k-block.  M, N multiples of 32, K of 16. */
int dws_gemm_bf16x6(const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K, void* stream);

/* The arithmetic of precision="f16x3" alone, same shapes: every operand is multiplied by its scale (scale_a / scale_b,
 * powers of two: the layer kernels use 2^4 for activations, 2^12 for the gate and a per-matrix power of two that brings
 * the largest weight into (1, 2]), split into two fp16 terms (22 significand bits), three fp16 MFMA products per term
 * pair accumulated in fp32, the result multiplied by 1 / (scale_a scale_b).  Scaled operands beyond 65504 overflow. */
int dws_gemm_f16x3(const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K, float scale_a, float scale_b,
                   void* stream);

/* Timing of the dominant kernel, measured with HIP events on the stream the
 * kernel was launched on (bench.py roofline leg).  Enables per-launch event
 * recording for kernels whose name contains `substr`; query returns the number
 * of launches and their total milliseconds since enable. */
int dws_profile_enable(const char* substr);
int dws_profile_query(int64_t* launches, double* total_ms);
/* the same launches one by one, in launch order: ms[i] for i < min(*launches, capacity) */
int dws_profile_query_each(double* ms, int64_t capacity, int64_t* launches);
int dws_profile_disable(void);

#ifdef __cplusplus
}
#endif
#endif /* DWS_H_ */
