// dws_model: base of the two backbones behind the C ABI (include/dws.h).
#pragma once
#include <cstring>

#include "sampler.h"

namespace dws {

struct CopyJob { const float* src; float* dst; int64_t n; };
int launch_multi_copy(const CopyJob* table_dev, int njobs, hipStream_t s);   // api.hip: one kernel for a job table

// A fixed list of device-to-device copies run as ONE launch (the per-layer fc_t / bias tensors into their stacked
// buffers and the stacked gradients back out: 4-5 hipMemcpyAsync per layer and step otherwise).  The job table is
// uploaded only when it differs from the one already on the device (buffers are allocated once, so: the first time).
struct CopyBatch {
    std::vector<CopyJob> jobs, uploaded;
    DevBuf table;
    void begin() { jobs.clear(); }
    void add(const float* src, float* dst, size_t n) { jobs.push_back({src, dst, (int64_t)n}); }
    int run(hipStream_t s) {
        if (jobs.empty()) return DWS_OK;
        DWS_TRY(upload_if_changed(table, uploaded, jobs.data(), jobs.size(), s));
        return launch_multi_copy((const CopyJob*)table.p, (int)jobs.size(), s);
    }
};

// Weight preparation of a commit as job tables (wavenet_kernels.hip: weight_prep_kernel): the weight-norm folds, MFMA fragment
// packs and row sums of ALL weights in two launches (folds, then everything that reads a folded or raw weight) instead of one
// 4-5 us launch each -- a training step commits once per step: 286 launches = 1.35 ms of a config-5 step.  Each job runs the
// very arithmetic of its single launcher (same block shape, same reduction order): results are bit-identical.
enum { PREP_FOLD = 0, PREP_PACK = 1, PREP_PACK_T = 2, PREP_ROW_SUM = 3 };
struct PrepJob { const float* a; const float* b; float* out; int n0, n1, kind, first_block; };
int prep_job_blocks(int kind, int n0, int n1);
int launch_weight_prep(const PrepJob* table_dev, int njobs, int nblocks, hipStream_t s);

struct PrepBatch {
    std::vector<PrepJob> jobs[2], uploaded[2];    // phase 0: folds; phase 1: packs / row sums (may read a phase-0 output)
    DevBuf table[2];
    int nblocks[2] = {0, 0};
    void begin() { jobs[0].clear(); jobs[1].clear(); nblocks[0] = nblocks[1] = 0; }
    void add(int kind, const float* a, const float* b, float* out, int n0, int n1) {
        const int ph = kind == PREP_FOLD ? 0 : 1;
        jobs[ph].push_back({a, b, out, n0, n1, kind, nblocks[ph]});
        nblocks[ph] += prep_job_blocks(kind, n0, n1);
    }
    void fold(const float* v, const float* g, float* out, int O, int inner) { add(PREP_FOLD, v, g, out, O, inner); }
    void pack(const float* w, float* out, int M, int K) { add(PREP_PACK, w, nullptr, out, M, K); }
    void pack_t(const float* w, float* out, int O, int K) { add(PREP_PACK_T, w, nullptr, out, O, K); }
    void row_sum(const float* w, float* rs, int O, int K) { add(PREP_ROW_SUM, w, nullptr, rs, O, K); }
    int run(hipStream_t s) {
        for (int ph = 0; ph < 2; ++ph) {
            if (jobs[ph].empty()) continue;
            // (buffers are allocated once: the first commit of a model, or a re-shaped one)
            DWS_TRY(upload_if_changed(table[ph], uploaded[ph], jobs[ph].data(), jobs[ph].size(), s));
            DWS_TRY(launch_weight_prep((const PrepJob*)table[ph].p, (int)jobs[ph].size(), nblocks[ph], s));
        }
        return DWS_OK;
    }
};

int launch_iota_f32(float* out, int n, hipStream_t s);   // wavenet_kernels.hip
// ragged batches (wavenet_kernels.hip): x[b, c, len_b .. min(L, len_b + reach)) = v for every row (b, c) of x [B, C, L],
// len_b = lengths[b] (device), stores only; reach < 0: the whole tail.  v = 0.0f, or (pt given) -pt[b * pt_bstride + c
// (+ *step_idx * pt_tstride)]: the value that makes the next layer's h = x + fc_t(e) zero.
int launch_wn_mask_tail(float* x, const int32_t* lengths, int B, int C, int L, int reach, const float* pt, int pt_bstride,
                        const int* step_idx, int pt_tstride, hipStream_t s);
// the same kernel on rows `row_stride` floats apart whose clip ends at lengths[b] / div (a pooled SaShiMi stage; the
// zero-padded rocFFT input rows): x[(b C + c) row_stride + (lengths[b] / div .. L)) = 0.0f
int launch_mask_tail_rows(float* x, const int32_t* lengths, int B, int C, int L, size_t row_stride, int div, hipStream_t s);
// class conditioning (wavenet_kernels.hip): out[r][:] = in[r / rep][:] + table[lab ? lab[r % nlab] : K][:], one fp32 add per
// element (in place when rep == 1 and out == in); and its adjoint dtable[c][:] = sum over b with lab[b] == c of de[b][:], in
// ascending b, rows of absent classes exactly zero
int launch_label_add(const float* in, const float* table, const int32_t* lab, int nlab, int K, float* out, int rows, int rep,
                     int E, hipStream_t s);
int launch_label_grad(const float* de, const int32_t* lab, float* dtable, int B, int K, int E, hipStream_t s);

// Key of a sampler step table: the step values it holds (null steps = t = 0..T-1), compared bit for bit.
struct StepKey {
    std::vector<float> v;
    bool valid = false;
    bool same(int T, const float* steps) const {
        if (!valid || (int)v.size() != T) return false;
        if (steps) return std::memcmp(v.data(), steps, (size_t)T * 4) == 0;
        for (int t = 0; t < T; ++t)
            if (v[t] != (float)t) return false;
        return true;
    }
    // write the step values into the device array `dev` [T] and remember them
    int upload(int T, const float* steps, float* dev, hipStream_t s) {
        valid = false;
        if (steps) {
            v.assign(steps, steps + T);
            DWS_HIP(hipMemcpyAsync(dev, v.data(), (size_t)T * 4, hipMemcpyHostToDevice, s));
            DWS_HIP(hipStreamSynchronize(s));   // `v` is rewritten by the next rebuild
        } else {
            v.resize((size_t)T);
            for (int t = 0; t < T; ++t) v[t] = (float)t;
            DWS_TRY(launch_iota_f32(dev, T, s));
        }
        valid = true;
        return DWS_OK;
    }
};

struct ParamSpec {
    std::string name;
    std::vector<int64_t> shape;
    int dtype = 0;  // 0 float32, 1 int64
    int index = 0;  // place in dws_model::params
    DevBuf buf;     // raw copy of the state-dict tensor
    DevBuf grad;    // gradient w.r.t. the raw tensor (training path; allocated on first backward)
    size_t numel() const {
        size_t n = 1;
        for (auto s : shape) n *= (size_t)s;
        return n;
    }
    size_t nbytes() const { return numel() * (dtype == 1 ? 8 : 4); }
};

}  // namespace dws

struct dws_model {
    dws_model_desc d;
    std::vector<dws::ParamSpec*> params;
    std::map<std::string, int> index;
    bool dirty = true;
    uint64_t int_params_version = 1;  // bumped whenever an int64 tensor (S4 `L` buffers) is (re)set
    int64_t B = 0, L = 0;  // prepared workspace shape

    dws::DevBuf lin_scratch;  // split-O partials of the embedding adjoint
    // batched parameter / gradient copies (api.hip: multi_copy): the job table of a call travels through the pinned
    // staging ring into the device table, so the host can run a training step ahead of the GPU
    dws::DevBuf copy_table;
    dws::StagingRing copy_ring{4};

    dws::SamplerState smp;               // sampler.h
    const int* step_idx = nullptr;       // set by the sampler around forward(): step-table mode, row *step_idx (device memory)
    uint64_t step_table_gen = 0;         // bumped by every step-table rebuild (build_step_table)
    int set_clip_seeds(const uint64_t* seeds, int64_t nB, hipStream_t s);
    int set_prior(const float* sigma, int64_t nB, int64_t n_per_clip, hipStream_t s);

    // ---- class conditioning (dws_model_set_classes / dws_model_set_labels): one parameter "label_embedding.weight"
    // [K+1][Eout] beside fc_t1 / fc_t2 (row K = the null class); a clip's row is added to the output of the embedding MLP,
    // so the label enters the network through the per-block fc_t rows alone.
    int n_classes = 0;                    // K (0: no class conditioning)
    bool params_touched = false;          // a set_param / update_params / commit has run: set_classes comes too late
    std::string label_param;              // the parameter's name in the state_dict layout of the backbone
    dws::DevBuf labels_dev;               // int32 [B]; all K while no labels are installed
    std::vector<int32_t> labels_host;     // what labels_dev holds (empty: the null class everywhere)
    uint64_t labels_version = 0;          // bumped by every change of the assignment (step tables follow it)
    dws::StagingRing label_ring{4};       // pinned staging of the upload
    bool labelled() const { return n_classes > 0 && !labels_host.empty(); }
    const int32_t* labels_ptr() const { return static_cast<const int32_t*>(labels_dev.p); }
    int set_classes(int32_t K);
    int set_labels(const int32_t* labels, int64_t nB, hipStream_t s);
    int reset_labels();                   // after a prepare to another shape: the null class for every clip (blocking)

    // ---- ragged batches (dws_model_set_lengths): per-clip lengths and mel frame counts of the prepared batch in one
    // model-owned device table, int32 [2][B] = lengths, frames.  The kernels that seal the padding read it from device
    // memory, so a new table at the same shape replays a captured step.
    dws::DevBuf lengths_dev;
    std::vector<int32_t> lengths_host, frames_host;   // what lengths_dev holds (empty: off)
    dws::StagingRing length_ring{4};      // pinned staging of the upload
    bool ragged() const { return !lengths_host.empty(); }
    const int32_t* lengths_ptr() const { return static_cast<const int32_t*>(lengths_dev.p); }
    const int32_t* frames_ptr() const { return lengths_ptr() + B; }
    // validation, pinned-ring upload and re-evaluation of the conditioner terms, shared by the backbones (api.hip)
    int set_lengths(const int32_t* lengths, const int32_t* mel_frames, int64_t nB, hipStream_t s);
    // a mel beside per-clip lengths: one mel per clip, and every clip's frames inside it
    int check_ragged_mel(const int32_t* frames, int64_t Bm, int64_t Tmel) const;
    // what set_lengths asks of a backbone: the samples per mel frame (0: unconditional) and the number every length must
    // be a multiple of (SaShiMi: the product of its pooling factors; 1: any length) ...
    virtual int ragged_rule(int64_t* hop, int64_t* multiple) const = 0;
    // ... the installed mel (batch, frames; 0: none) and its conditioner terms evaluated again from the kept copy
    virtual int64_t cond_batch() const = 0;
    virtual int64_t cond_frames() const = 0;
    virtual int reeval_condition(hipStream_t s) = 0;

    // ---- staged gradient hand-over (data-parallel overlap, dws_model_set_grad_sinks): the host names a destination and a
    // GROUP (its all-reduce bucket) per parameter; backward() copies a group's gradients to their destinations (one launch)
    // and records the group's event the moment the group's last gradient has been produced, so the host can start that
    // bucket's all-reduce while the rest of backward still runs.  When a gradient is final is LEARNT: G() stamps every
    // access during a backward with the number of the flush point (grad_point) it precedes; the first backward after the
    // sinks (or the model's graph) changed only records and flushes everything at its end.
    struct GradGroup {
        std::vector<int> params;       // parameter indices
        dws::CopyBatch copy;           // grads -> sinks, table uploaded once
        dws::Event ev;                 // recorded behind the group's copy
        int ready_seq = 0;             // flush point after which every gradient of the group is final (learnt)
        bool flushed = false, touched_after_flush = false;
    };
    std::vector<GradGroup> grad_groups;
    std::vector<int> grad_group_of;        // per parameter: group or -1
    std::vector<float*> grad_sink;         // per parameter: destination or null
    std::vector<int> grad_touch, grad_touch_prev;   // per parameter: flush point of the last G() of this / the previous backward
    bool grad_order_known = false, in_backward = false;
    int grad_seq = 0;
    int set_grad_sinks(int32_t count, const char* const* names, float* const* dsts, const int64_t* numels, const int32_t* groups,
                       int32_t ngroups);
    void grad_begin();                 // start of a backward
    int grad_point(hipStream_t s);     // a flush opportunity inside backward (after a layer / block)
    int grad_end(hipStream_t s);       // end of a backward: flush what is left, learn the order
    int grad_flush(GradGroup& g, hipStream_t s);

    virtual ~dws_model();
    dws::ParamSpec* add_param(const std::string& name, std::vector<int64_t> shape, int dtype = 0);
    float* P(const std::string& name) const;  // raw device pointer of a parameter
    int alloc_params();
    void drop_graph() { smp.drop_graph(); }
    // the parameter `name`, or null with the error set: "unknown parameter" or (state_dict) "unexpected key ... in state_dict"
    dws::ParamSpec* find(const char* name, bool state_dict = false) const;

    virtual int set_option(const std::string& key, const std::string& value);
    virtual int commit(hipStream_t s) = 0;
    virtual int prepare(int64_t B, int64_t L) = 0;
    virtual int set_condition(const float* mel, int64_t Bm, int64_t Tmel, hipStream_t s) = 0;
    // steps may be null only while step_idx is set (sampler): the step-only terms then come from the step table
    virtual int forward(const float* audio, const float* steps, float* out, hipStream_t s) = 0;
    // evaluate everything that depends on the diffusion step only, at T steps: the HOST values `steps` [T], or
    // t = 0..T-1 when null (kept while the weights and the step values stay)
    virtual int build_step_table(int T, const float* steps, hipStream_t s) = 0;
    virtual int read_tap(const char* tap, float* dst, int64_t capacity, hipStream_t s) = 0;
    // training path: forward that keeps what backward needs; backward fills ParamSpec::grad of every parameter
    virtual int forward_train(const float* audio, const float* steps, float* out, hipStream_t s);
    // the training forward of a data-only backward (dws_model_forward_input); a backbone without limits of its own: forward_train
    virtual int forward_input(const float* audio, const float* steps, float* out, hipStream_t s) {
        return forward_train(audio, steps, out, s);
    }
    // daudio (optional): the gradient w.r.t. audio [B, in_channels, L]; param_grads = false (needs daudio): the data path
    // only -- no ParamSpec::grad is touched, nothing is handed to the sinks
    virtual int backward(const float* dout, float* daudio, bool param_grads, hipStream_t s);
    float* G(const std::string& name);  // gradient buffer of a parameter (allocated, zeroed on first use)
};

namespace dws {
dws_model* make_wavenet(const dws_model_desc& d);
dws_model* make_sashimi(const dws_model_desc& d);
}  // namespace dws
