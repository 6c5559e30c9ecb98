// dws_model: base of the two backbones behind the C ABI (include/dws.h).
#pragma once
#include <cstring>

#include "dws_common.h"

namespace dws {

// RAII device buffer.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    ~DevBuf() { release(); }
    void release() {
        if (p) hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // (re)allocate when the request grows; contents are not preserved.
    int ensure(size_t n) {
        if (n <= bytes && p) return DWS_OK;
        release();
        if (n == 0) n = 4;
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) {
            p = nullptr;
            return set_error(DWS_ERR_HIP, "hipMalloc(%zu) failed: %s", n, hipGetErrorString(e));
        }
        bytes = n;
        return DWS_OK;
    }
    float* f() const { return static_cast<float*>(p); }
};

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
        const bool same = jobs.size() == uploaded.size() &&
                          std::memcmp(jobs.data(), uploaded.data(), jobs.size() * sizeof(CopyJob)) == 0;
        if (!same) {
            DWS_HIP(hipStreamSynchronize(s));   // nothing in flight may still read the old table / host copy
            uploaded = jobs;
            DWS_TRY(table.ensure(uploaded.size() * sizeof(CopyJob)));
            DWS_HIP(hipMemcpy(table.p, uploaded.data(), uploaded.size() * sizeof(CopyJob), hipMemcpyHostToDevice));
        }
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
            const bool same = jobs[ph].size() == uploaded[ph].size() &&
                              std::memcmp(jobs[ph].data(), uploaded[ph].data(), jobs[ph].size() * sizeof(PrepJob)) == 0;
            if (!same) {      // (buffers are allocated once: the first commit of a model, or a re-shaped one)
                DWS_HIP(hipStreamSynchronize(s));
                uploaded[ph] = jobs[ph];
                DWS_TRY(table[ph].ensure(uploaded[ph].size() * sizeof(PrepJob)));
                DWS_HIP(hipMemcpy(table[ph].p, uploaded[ph].data(), uploaded[ph].size() * sizeof(PrepJob), hipMemcpyHostToDevice));
            }
            DWS_TRY(launch_weight_prep((const PrepJob*)table[ph].p, (int)jobs[ph].size(), nblocks[ph], s));
        }
        return DWS_OK;
    }
};

int launch_iota_f32(float* out, int n, hipStream_t s);   // wavenet_kernels.hip
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
    // batched parameter / gradient copies (api.hip): device job table, pinned staging, reuse guard
    // multi_copy staging: the job table of a call travels through one of COPY_SLOTS pinned buffers (round robin; an
    // event per slot guards its reuse, so the host only ever waits for the call made COPY_SLOTS calls ago and can run
    // a training step ahead of the GPU)
    static constexpr int COPY_SLOTS = 4;
    dws::DevBuf copy_table;
    void* copy_pinned[COPY_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    size_t copy_pinned_cap[COPY_SLOTS] = {0, 0, 0, 0};
    hipEvent_t copy_consumed[COPY_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    int copy_slot = 0;

    // sampler state (sampler.hip)
    dws::DevBuf smp_tables;   // [3][T] c1, c2, sigma
    std::vector<float> smp_host_tables;  // host copy of what is resident (upload skipped when identical)
    dws::DevBuf smp_state;    // int32 step index
    dws::DevBuf smp_eps;      // eps[B, Cout, L]
    int64_t smp_eps_B = 0, smp_eps_L = 0;   // shape of the sampler step that last wrote it
    const int* step_idx = nullptr;   // set by the sampler around forward(): step-table mode, row *step_idx (device memory)
    hipGraphExec_t smp_graph = nullptr;
    hipStream_t smp_stream = nullptr;  // capture/replay stream (the caller's may be the null stream)
    hipEvent_t smp_ev_in = nullptr, smp_ev_out = nullptr;
    // key of the captured graph
    int64_t g_B = 0, g_L = 0;
    int g_T = 0;
    const void* g_x = nullptr;
    const void* g_noise = nullptr;
    uint64_t g_seed = 0;
    // few-step sampler (dws_sampler_run_schedule): tables, state, x and graph of its own -- the two entry points never
    // replay each other's graph.  Its graph updates sch_x in place and reads the seed from sch_state, so neither the
    // caller's x nor the seed is baked in.
    dws::DevBuf sch_tables;               // DDPM [3][S] c1, c2, sigma; DDIM [5][S] k1 .. k5; DPM-Solver++(2M) [5][S] m1 .. m5
    std::vector<float> sch_host_tables;   // host copy of what is resident (upload skipped when identical)
    dws::DevBuf sch_state;                // int32 step index, int32 finished update blocks, uint64 Philox seed, int32 visit,
                                          // int32 history-valid word (DPM-Solver++(2M): sch_hist holds the last step's x0)
    dws::DevBuf sch_x;                    // [B, C, L]
    dws::DevBuf sch_hist;                 // [B, C, L] the previous step's data prediction (DWS_SAMPLER_DPMPP2M; first use)
    struct SchKey {
        int64_t B, L;
        int S, kind, vec;
        const void *tables, *noise, *eps, *x, *state;
        uint64_t table_gen;
        const void *edit, *known, *mask, *known_noise;   // the edited step's (all null for the unedited one)
        int V = 0;                                       // the resampling step's: visits and the program tables
        const void* prog = nullptr;
        const void* hist = nullptr;                      // the multistep kind's history buffer (null for the others)
        const void* clip_seeds = nullptr;                // the per-clip seed table (null for a scalar-seed step)
        bool operator==(const SchKey& o) const {
            return B == o.B && L == o.L && S == o.S && kind == o.kind && vec == o.vec && tables == o.tables &&
                   noise == o.noise && eps == o.eps && x == o.x && state == o.state && table_gen == o.table_gen &&
                   edit == o.edit && known == o.known && mask == o.mask && known_noise == o.known_noise && V == o.V &&
                   prog == o.prog && hist == o.hist && clip_seeds == o.clip_seeds;
        }
    };
    // One captured step per flavour of call (same state, x, eps and step table), so the flavours alternate without a new
    // capture: the unedited step, the step that ends in the replacement of the known region (dws_sampler_run_edit), the
    // reverse visit of a program (dws_sampler_run_program) and the guided step (dws_sampler_set_cfg) -- each once for the
    // scalar seed ([0]) and once for per-clip seeds ([1]: other kernel instances on a grid row per clip), so the two forms
    // of seed alternate without a new capture as well.
    enum { SCH_PLAIN, SCH_EDIT, SCH_PROG, SCH_CFG, SCH_GRAPHS };
    struct SchGraph {
        hipGraphExec_t exec = nullptr;
        SchKey key{};
    } sch_graphs[SCH_GRAPHS][2];
    // editing: the known clip and the mask are copied into model-owned buffers before the replays, like x into sch_x.
    dws::DevBuf sch_edit;                 // [2][S] q1, q2 of sampling.edit_coefficients
    std::vector<float> sch_host_edit;     // host copy of what is resident
    dws::DevBuf sch_known;                // float [B, C, L]
    dws::DevBuf sch_mask;                 // uint8 [B, C, L] (rounded up to whole groups of four)
    // resampling: the program tables sit in a model-owned buffer keyed on their contents, so a new program of the same V
    // replays the held graph.
    dws::DevBuf sch_prog;                 // int32 step_of[V], float ja[V], jb[V], indexed by the visit number
    std::vector<uint32_t> sch_host_prog;  // host copy of what is resident
    uint64_t step_table_gen = 0;          // bumped by every step-table rebuild (build_step_table)
    // classifier-free guidance in the schedule step: the model is prepared for 2 Bc clips, the first half carries the
    // wanted labels and the second the null class; the update runs on the first half alone.  The scale sits in the
    // device state (word 6).
    bool cfg_on = false;
    float cfg_scale = 0.f;
    // per-clip seeds (dws_sampler_set_clip_seeds): clip b draws from Philox key clip_seeds[b] with groups numbered inside
    // the clip, so its noise does not depend on the batch around it.  The table sits in device memory (a new one replays
    // the captured step) and holds until it is changed or the model is prepared for another shape.
    dws::DevBuf clip_seeds_dev;           // uint64 [clip_B]
    int64_t clip_B = 0;                   // clips the table holds (0: off, the scalar seed of the run entries)
    static constexpr int SEED_SLOTS = 4;  // pinned staging of the upload, as the label assignment (LABEL_SLOTS)
    uint64_t* seed_pinned[SEED_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    size_t seed_pinned_cap[SEED_SLOTS] = {0, 0, 0, 0};
    hipEvent_t seed_consumed[SEED_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    int seed_slot = 0;
    int set_clip_seeds(const uint64_t* seeds, int64_t nB, hipStream_t s);

    // ---- class conditioning (dws_model_set_classes / dws_model_set_labels): one parameter "label_embedding.weight"
    // [K+1][Eout] beside fc_t1 / fc_t2 (row K = the null class); a clip's row is added to the output of the embedding MLP,
    // so the label enters the network through the per-block fc_t rows alone.
    int n_classes = 0;                    // K (0: no class conditioning)
    bool params_touched = false;          // a set_param / update_params / commit has run: set_classes comes too late
    std::string label_param;              // the parameter's name in the state_dict layout of the backbone
    dws::DevBuf labels_dev;               // int32 [B]; all K while no labels are installed
    std::vector<int32_t> labels_host;     // what labels_dev holds (empty: the null class everywhere)
    uint64_t labels_version = 0;          // bumped by every change of the assignment (step tables follow it)
    static constexpr int LABEL_SLOTS = 4; // pinned staging of the upload, as the copy-job tables (COPY_SLOTS)
    int32_t* label_pinned[LABEL_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    size_t label_pinned_cap[LABEL_SLOTS] = {0, 0, 0, 0};
    hipEvent_t label_consumed[LABEL_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    int label_slot = 0;
    bool labelled() const { return n_classes > 0 && !labels_host.empty(); }
    const int32_t* labels_ptr() const { return static_cast<const int32_t*>(labels_dev.p); }
    int set_classes(int32_t K);
    int set_labels(const int32_t* labels, int64_t nB, hipStream_t s);
    int reset_labels();                   // after a prepare to another shape: the null class for every clip (blocking)
    int64_t graphs_made = 0;              // tap "sampler_graphs": graphs instantiated by either entry point

    // ---- staged gradient hand-over (data-parallel overlap, dws_model_set_grad_sinks): the host names a destination and a
    // GROUP (its all-reduce bucket) per parameter; backward() copies a group's gradients to their destinations (one launch)
    // and records the group's event the moment the group's last gradient has been produced, so the host can start that
    // bucket's all-reduce while the rest of backward still runs.  When a gradient is final is LEARNT: G() stamps every
    // access during a backward with the number of the flush point (grad_point) it precedes; the first backward after the
    // sinks (or the model's graph) changed only records and flushes everything at its end.
    struct GradGroup {
        std::vector<int> params;       // parameter indices
        dws::CopyBatch copy;           // grads -> sinks, table uploaded once
        hipEvent_t ev = nullptr;       // recorded behind the group's copy
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
    void drop_graph();

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
    // daudio (optional): the gradient w.r.t. audio [B, in_channels, L]; param_grads = false (needs daudio): the data path
    // only -- no ParamSpec::grad is touched, nothing is handed to the sinks
    virtual int backward(const float* dout, float* daudio, bool param_grads, hipStream_t s);
    float* G(const std::string& name);  // gradient buffer of a parameter (allocated, zeroed on first use)
};

namespace dws {
dws_model* make_wavenet(const dws_model_desc& d);
dws_model* make_sashimi(const dws_model_desc& d);
}  // namespace dws
