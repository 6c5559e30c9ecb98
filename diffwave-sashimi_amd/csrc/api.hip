// extern "C" surface of libdws.so for the model and sampler entry points
// (include/dws.h); the Cauchy entry points live in cauchy_kernels.hip.
#include <cstring>
#include <cmath>
#include "model.h"
#include "optim.h"

namespace dws {
struct SamplerProgram;
int sampler_run(dws_model* m, float* x, const float* alpha, const float* alpha_bar, const float* sigma, int T,
                const float* noise, uint64_t seed, int init_from_seed, int use_graph, hipStream_t s);
int sampler_steps(dws_model* m, float* x, const float* alpha, const float* alpha_bar, const float* sigma, int T,
                  int t_start, int n_steps, uint64_t seed, int use_graph, hipStream_t s);
int sampler_run_schedule(dws_model* m, float* x, int kind, int S, const float* net_steps, const float* coef,
                         const float* noise, uint64_t seed, int init_from_seed, int use_graph,
                         const dws_sampler_edit* e, const SamplerProgram* pg, hipStream_t s);
int sampler_run_program(dws_model* m, float* x, int kind, int S, const float* net_steps, const float* coef, int V,
                        const int32_t* visit_step, const float* jump_coef, const float* noise, uint64_t seed,
                        int init_from_seed, int use_graph, const dws_sampler_edit* e, hipStream_t s);
int philox_normal(float* x, int64_t n, uint64_t seed, uint32_t stream_id, hipStream_t s);
int philox_normal_clips(float* x, int64_t B, int64_t n_per_clip, const uint64_t* seeds, uint32_t stream_id, hipStream_t s);
}  // namespace dws

dws_model::~dws_model() {
    for (auto* p : params) delete p;
}

dws::ParamSpec* dws_model::find(const char* name, bool state_dict) const {
    auto it = index.find(name);
    if (it != index.end()) return params[it->second];
    dws::set_error(DWS_ERR_INVALID, state_dict ? "unexpected key '%s' in state_dict" : "unknown parameter '%s'", name);
    return nullptr;
}

int dws_model::set_classes(int32_t K) {
    // (the table's adjoint runs one grid row per class: K + 1 <= 65535)
    DWS_CHECK(K >= 1 && K <= 65534, DWS_ERR_INVALID, "dws_model_set_classes: n_classes = %d (needs 1 .. 65534)", K);
    DWS_CHECK(!params_touched && n_classes == 0, DWS_ERR_STATE,
              "dws_model_set_classes comes after dws_model_create and before the first set_param / commit, once");
    DWS_CHECK(!label_param.empty(), DWS_ERR_UNSUPPORTED, "this backbone has no class conditioning");
    dws::ParamSpec* p = add_param(label_param, {(int64_t)K + 1, (int64_t)d.diffusion_step_embed_dim_out});
    DWS_TRY(p->buf.ensure(p->nbytes()));
    DWS_HIP(hipMemset(p->buf.p, 0, p->nbytes()));
    n_classes = K;
    if (B > 0) DWS_TRY(reset_labels());
    return DWS_OK;
}

int dws_model::reset_labels() {
    if (n_classes == 0 || B <= 0) return DWS_OK;
    DWS_HIP(hipDeviceSynchronize());      // (a shape change: nothing in flight may still read the old assignment)
    DWS_TRY(labels_dev.ensure((size_t)B * 4));
    std::vector<int32_t> h((size_t)B, n_classes);
    DWS_HIP(hipMemcpy(labels_dev.p, h.data(), (size_t)B * 4, hipMemcpyHostToDevice));
    labels_host.clear();
    ++labels_version;
    return DWS_OK;
}

int dws_model::set_labels(const int32_t* labels, int64_t nB, hipStream_t s) {
    DWS_CHECK(n_classes > 0, DWS_ERR_INVALID, "dws_model_set_labels on a model without classes (dws_model_set_classes)");
    DWS_CHECK(B > 0, DWS_ERR_STATE, "dws_model_set_labels before dws_model_prepare");
    DWS_CHECK(nB == B, DWS_ERR_INVALID, "dws_model_set_labels: %lld labels for a prepared batch of %lld", (long long)nB, (long long)B);
    if (labels)
        for (int64_t b = 0; b < B; ++b)
            DWS_CHECK(labels[b] >= 0 && labels[b] <= n_classes, DWS_ERR_INVALID,
                      "dws_model_set_labels: labels[%lld] = %d (needs 0 .. %d, %d = the null class)", (long long)b, labels[b],
                      n_classes, n_classes);
    if (labels ? (labels_host.size() == (size_t)B && std::memcmp(labels_host.data(), labels, (size_t)B * 4) == 0)
               : (labels_host.empty() && labels_dev.p))
        return DWS_OK;     // the assignment already installed
    DWS_CHECK(labels_dev.p && labels_dev.bytes >= (size_t)B * 4, DWS_ERR_STATE, "dws_model_set_labels: no label buffer");
    int32_t* h = nullptr;
    DWS_TRY(label_ring.acquire((size_t)B * 4, (void**)&h));
    for (int64_t b = 0; b < B; ++b) h[b] = labels ? labels[b] : n_classes;
    DWS_HIP(hipMemcpyAsync(labels_dev.p, h, (size_t)B * 4, hipMemcpyHostToDevice, s));
    DWS_TRY(label_ring.commit(s));
    if (labels) labels_host.assign(labels, labels + B);
    else labels_host.clear();
    ++labels_version;
    return DWS_OK;
}

// Per-clip lengths of the prepared batch (dws_model_set_lengths), for both backbones: host validation, the int32 [2][B]
// device table (lengths, mel frames) through the pinned ring, and the conditioner terms evaluated again from the kept mel
// whenever the table changes -- a forward never runs with terms built for other lengths.
int dws_model::check_ragged_mel(const int32_t* frames, int64_t Bm, int64_t Tmel) const {
    DWS_CHECK(Bm == B, DWS_ERR_INVALID, "a shared mel (Bm = %lld) with per-clip lengths: a ragged batch has a mel per clip",
              (long long)Bm);
    for (int64_t b = 0; b < B; ++b)
        DWS_CHECK(frames[b] <= Tmel, DWS_ERR_INVALID, "mel_frames[%lld] = %d frames, the mel holds %lld", (long long)b,
                  frames[b], (long long)Tmel);
    return DWS_OK;
}

int dws_model::set_lengths(const int32_t* lengths, const int32_t* mel_frames, int64_t nB, hipStream_t s) {
    if (!lengths) {
        if (!ragged()) return DWS_OK;
        lengths_host.clear(); frames_host.clear();
        if (dirty && cond_batch() > 0) DWS_TRY(commit(s));   // (drops the installed mel: nothing to re-evaluate below)
        if (cond_batch() > 0) DWS_TRY(reeval_condition(s));  // the terms were built under the old frame counts
        return DWS_OK;
    }
    DWS_CHECK(B > 0, DWS_ERR_STATE, "dws_model_set_lengths before dws_model_prepare");
    DWS_CHECK(nB == B, DWS_ERR_INVALID, "dws_model_set_lengths: %lld lengths for a prepared batch of %lld", (long long)nB, (long long)B);
    DWS_CHECK(!smp.cfg_on, DWS_ERR_UNSUPPORTED, "per-clip lengths are not built for classifier-free guidance (dws_sampler_set_cfg is on)");
    int64_t hop = 0, mult = 1;
    DWS_TRY(ragged_rule(&hop, &mult));
    std::vector<int32_t> fr((size_t)B, 1);
    for (int64_t b = 0; b < B; ++b) {
        // (SaShiMi: the clip's length at a pooled stage is lengths[b] / the factors above it, an integer only then)
        DWS_CHECK(lengths[b] % mult == 0, DWS_ERR_UNSUPPORTED,
                  "dws_model_set_lengths: lengths[%lld] = %d is not a multiple of %lld, the product of the pooling factors",
                  (long long)b, lengths[b], (long long)mult);
        DWS_CHECK(lengths[b] >= 1 && lengths[b] <= L, DWS_ERR_INVALID, "dws_model_set_lengths: lengths[%lld] = %d (needs 1 .. L = %lld)",
                  (long long)b, lengths[b], (long long)L);
        if (hop == 0) continue;
        const int64_t f = mel_frames ? mel_frames[b] : (lengths[b] + hop - 1) / hop;
        DWS_CHECK(f >= 1 && f <= INT32_MAX && hop * f >= lengths[b], DWS_ERR_INVALID,
                  "dws_model_set_lengths: mel_frames[%lld] = %lld frames of %lld samples for a clip of %d", (long long)b,
                  (long long)f, (long long)hop, lengths[b]);
        fr[b] = (int32_t)f;
    }
    if (cond_batch() > 0) DWS_TRY(check_ragged_mel(fr.data(), cond_batch(), cond_frames()));
    if (lengths_host.size() == (size_t)B && std::memcmp(lengths_host.data(), lengths, (size_t)B * 4) == 0 && frames_host == fr)
        return DWS_OK;     // the table already installed
    if (dirty && cond_batch() > 0) DWS_TRY(commit(s));   // (drops the installed mel: nothing to re-evaluate below)
    DWS_TRY(lengths_dev.ensure((size_t)B * 8));
    int32_t* h = nullptr;
    DWS_TRY(length_ring.acquire((size_t)B * 8, (void**)&h));
    std::memcpy(h, lengths, (size_t)B * 4);
    std::memcpy(h + B, fr.data(), (size_t)B * 4);
    DWS_HIP(hipMemcpyAsync(lengths_dev.p, h, (size_t)B * 8, hipMemcpyHostToDevice, s));
    DWS_TRY(length_ring.commit(s));
    lengths_host.assign(lengths, lengths + B);
    frames_host = fr;
    if (cond_batch() > 0) DWS_TRY(reeval_condition(s));
    return DWS_OK;
}

// The grid of a per-clip launch has one row per clip: at most 65535 clips.
int dws_model::set_clip_seeds(const uint64_t* seeds, int64_t nB, hipStream_t s) {
    if (!seeds) {
        smp.clip_B = 0;
        return DWS_OK;
    }
    DWS_CHECK(B > 0, DWS_ERR_STATE, "dws_sampler_set_clip_seeds before dws_model_prepare");
    DWS_CHECK(nB >= 1 && nB <= 65535, DWS_ERR_INVALID, "dws_sampler_set_clip_seeds: %lld seeds (needs 1 .. 65535)", (long long)nB);
    DWS_TRY(smp.clip_seeds.ensure((size_t)nB * 8));
    void* h = nullptr;
    DWS_TRY(smp.seed_ring.acquire((size_t)nB * 8, &h));
    std::memcpy(h, seeds, (size_t)nB * 8);
    DWS_HIP(hipMemcpyAsync(smp.clip_seeds.p, h, (size_t)nB * 8, hipMemcpyHostToDevice, s));
    DWS_TRY(smp.seed_ring.commit(s));
    smp.clip_B = nB;
    return DWS_OK;
}

// The table of the adaptive prior: device to device into a model-owned buffer at the shape of the sampler state.
int dws_model::set_prior(const float* sigma, int64_t nB, int64_t n_per_clip, hipStream_t s) {
    if (!sigma) {
        smp.prior_on = false;
        return DWS_OK;
    }
    DWS_CHECK(B > 0, DWS_ERR_STATE, "dws_sampler_set_prior before dws_model_prepare");
    DWS_CHECK(!smp.cfg_on, DWS_ERR_UNSUPPORTED, "an adaptive prior with classifier-free guidance (dws_sampler_set_cfg is on) is not built");
    DWS_CHECK(nB == B && n_per_clip == d.out_channels * L, DWS_ERR_INVALID,
              "dws_sampler_set_prior: a table of [%lld, %lld] for a sampler state of [%lld, %lld]", (long long)nB,
              (long long)n_per_clip, (long long)B, (long long)(d.out_channels * L));
    const size_t bytes = (size_t)nB * n_per_clip * 4;
    DWS_TRY(smp.prior.ensure(bytes));
    DWS_HIP(hipMemcpyAsync(smp.prior.p, sigma, bytes, hipMemcpyDeviceToDevice, s));
    smp.prior_B = nB; smp.prior_n = n_per_clip;
    smp.prior_on = true;
    return DWS_OK;
}

dws::ParamSpec* dws_model::add_param(const std::string& name, std::vector<int64_t> shape, int dtype) {
    auto* p = new dws::ParamSpec();
    p->name = name;
    p->shape = std::move(shape);
    p->dtype = dtype;
    p->index = index[name] = (int)params.size();
    params.push_back(p);
    return p;
}

int dws_model::forward_train(const float*, const float*, float*, hipStream_t) {
    return dws::set_error(DWS_ERR_UNSUPPORTED, "the training forward/backward of this backbone is not built yet");
}

int dws_model::backward(const float*, float*, bool, hipStream_t) {
    return dws::set_error(DWS_ERR_UNSUPPORTED, "the training forward/backward of this backbone is not built yet");
}

float* dws_model::G(const std::string& name) {
    auto it = index.find(name);
    if (it == index.end()) return nullptr;
    dws::ParamSpec* p = params[it->second];
    if (!p->grad.p) {
        if (p->grad.ensure(p->nbytes()) != DWS_OK) return nullptr;
        hipMemset(p->grad.p, 0, p->nbytes());
    }
    if (in_backward && !grad_touch.empty()) {      // staged hand-over: this gradient is (still) being produced at flush point grad_seq
        grad_touch[it->second] = grad_seq;
        const int g = grad_group_of[it->second];
        if (g >= 0 && grad_groups[g].flushed) grad_groups[g].touched_after_flush = true;
    }
    return p->grad.f();
}

int dws_model::set_grad_sinks(int32_t count, const char* const* names, float* const* dsts, const int64_t* numels,
                              const int32_t* groups, int32_t ngroups) {
    grad_groups.clear();
    grad_group_of.assign(params.size(), -1);
    grad_sink.assign(params.size(), nullptr);
    grad_touch.assign(params.size(), -1);
    grad_touch_prev.clear();
    grad_order_known = false;
    if (count == 0) { grad_touch.clear(); return DWS_OK; }
    grad_groups.resize((size_t)ngroups);
    for (int i = 0; i < count; ++i) {
        dws::ParamSpec* p = find(names[i]);
        if (!p) return DWS_ERR_INVALID;
        DWS_CHECK(p->dtype == 0 && (int64_t)p->numel() == numels[i] && dsts[i], DWS_ERR_INVALID,
                  "'%s': gradient sink of %lld elements for a tensor of %zu", names[i], (long long)numels[i], p->numel());
        DWS_CHECK(groups[i] >= 0 && groups[i] < ngroups, DWS_ERR_INVALID, "'%s': group %d of %d", names[i], groups[i], ngroups);
        grad_group_of[p->index] = groups[i];
        grad_sink[p->index] = dsts[i];
        grad_groups[groups[i]].params.push_back(p->index);
    }
    return DWS_OK;
}

void dws_model::grad_begin() {
    in_backward = true;
    grad_seq = 0;
    std::fill(grad_touch.begin(), grad_touch.end(), -1);
    for (auto& g : grad_groups) g.flushed = g.touched_after_flush = false;
}

int dws_model::grad_flush(GradGroup& g, hipStream_t s) {
    g.copy.begin();
    for (int pi : g.params) {
        dws::ParamSpec* p = params[pi];
        const bool was = in_backward;
        in_backward = false;               // (fetching the buffer for the copy is not a production of the gradient)
        float* src = G(p->name);
        in_backward = was;
        DWS_CHECK(src, DWS_ERR_HIP, "could not allocate the gradient of '%s'", p->name.c_str());
        g.copy.add(src, grad_sink[pi], p->numel());
    }
    DWS_TRY(g.copy.run(s));
    DWS_TRY(g.ev.record(s));
    g.flushed = true;
    g.touched_after_flush = false;
    return DWS_OK;
}

int dws_model::grad_point(hipStream_t s) {
    if (!in_backward || grad_groups.empty()) return DWS_OK;
    if (grad_order_known)
        for (auto& g : grad_groups)
            if (!g.flushed && g.ready_seq <= grad_seq) DWS_TRY(grad_flush(g, s));
    ++grad_seq;
    return DWS_OK;
}

int dws_model::grad_end(hipStream_t s) {
    if (!in_backward) return DWS_OK;
    // whatever is left, and any group a late write invalidated (the learnt order was wrong for it: re-copied, its event
    // re-recorded -- the host waits on the events only after backward has returned, so it sees this record)
    bool order_held = true;
    for (auto& g : grad_groups) {
        if (g.touched_after_flush) order_held = false;
        if (!g.flushed || g.touched_after_flush) DWS_TRY(grad_flush(g, s));
    }
    in_backward = false;
    if (grad_groups.empty()) return DWS_OK;
    // learn: a group is ready after the flush point of its last-produced gradient.  The order of THIS backward is used by the
    // next one (the graph is static); a backward that disagrees with its predecessor -- new shapes, another config, a late
    // write caught above -- makes the next one a recording-only backward again.
    const bool same = grad_touch_prev.empty() || grad_touch_prev == grad_touch;
    for (auto& g : grad_groups) {
        int r = 0;
        for (int pi : g.params) r = std::max(r, grad_touch[pi] + 1);
        g.ready_seq = r;
    }
    grad_order_known = same && order_held;
    grad_touch_prev = grad_touch;
    return DWS_OK;
}

int dws_model::set_option(const std::string& key, const std::string& value) {
    return dws::set_error(DWS_ERR_INVALID, "unknown option %s=%s for this model", key.c_str(), value.c_str());
}

float* dws_model::P(const std::string& name) const {
    auto it = index.find(name);
    if (it == index.end()) return nullptr;
    return params[it->second]->buf.f();
}

int dws_model::alloc_params() {
    for (auto* p : params) {
        DWS_TRY(p->buf.ensure(p->nbytes()));
        DWS_HIP(hipMemset(p->buf.p, 0, p->nbytes()));
    }
    return DWS_OK;
}

extern "C" {

int dws_model_create(const dws_model_desc* desc, dws_model** out) {
    DWS_CHECK(desc && out, DWS_ERR_INVALID, "dws_model_create: null argument");
    const dws_model_desc& d = *desc;
    DWS_CHECK(d.in_channels > 0 && d.out_channels > 0, DWS_ERR_INVALID, "in/out channels must be positive");
    DWS_CHECK(d.diffusion_step_embed_dim_in > 0 && d.diffusion_step_embed_dim_in % 2 == 0, DWS_ERR_INVALID,
              "diffusion_step_embed_dim_in must be even (`models/utils.py:20`)");
    DWS_CHECK(d.diffusion_step_embed_dim_in <= 1024 && d.diffusion_step_embed_dim_mid <= 1024 &&
                  d.diffusion_step_embed_dim_out <= 1024,
              DWS_ERR_UNSUPPORTED, "embedding dims above 1024 are not supported");
    dws_model* m = nullptr;
    if (d.kind == DWS_KIND_WAVENET) {
        DWS_CHECK(d.res_channels > 0 && d.skip_channels > 0 && d.num_res_layers > 0 && d.dilation_cycle > 0,
                  DWS_ERR_INVALID, "wavenet: bad channel/layer counts");
        DWS_CHECK(d.dilation_cycle <= 24, DWS_ERR_UNSUPPORTED, "dilation_cycle > 24");
        m = dws::make_wavenet(d);
    } else if (d.kind == DWS_KIND_SASHIMI) {
        m = dws::make_sashimi(d);
        if (!m) return DWS_ERR_INVALID;  // message set by make_sashimi
    } else {
        return dws::set_error(DWS_ERR_INVALID, "unknown model kind %d (model._name_ must be wavenet|sashimi, "
                                               "`models/__init__.py:6-9`)", d.kind);
    }
    int st = m->alloc_params();
    if (st != DWS_OK) {
        delete m;
        return st;
    }
    *out = m;
    return DWS_OK;
}

int dws_model_destroy(dws_model* m) {
    delete m;
    return DWS_OK;
}

int dws_model_num_params(const dws_model* m) { return m ? (int)m->params.size() : 0; }

int dws_model_param_info(const dws_model* m, int i, const char** name, int64_t* shape, int* ndim, int* dtype) {
    DWS_CHECK(m && i >= 0 && i < (int)m->params.size(), DWS_ERR_INVALID, "param index %d out of range", i);
    const dws::ParamSpec* p = m->params[i];
    DWS_CHECK(p->shape.size() <= 8, DWS_ERR_INVALID, "rank > 8");
    if (name) *name = p->name.c_str();
    if (ndim) *ndim = (int)p->shape.size();
    if (dtype) *dtype = p->dtype;
    if (shape)
        for (size_t k = 0; k < p->shape.size(); ++k) shape[k] = p->shape[k];
    return DWS_OK;
}

int dws_model_set_param(dws_model* m, const char* name, const void* data, const int64_t* shape, int ndim, int dtype,
                        void* stream) {
    DWS_CHECK(m && name && data && shape, DWS_ERR_INVALID, "dws_model_set_param: null argument");
    if (!m->index.count(name) && name[0] == '_' && name[1] == '_') {
        // host-computed tables ("__omega.<L>", "__z.<L>": FFT nodes of an S4 kernel length the model was not
        // configured with, e.g. a checkpoint trained at another l_max) are registered on first sight
        dws::ParamSpec* np_ = m->add_param(name, std::vector<int64_t>(shape, shape + ndim), dtype);
        DWS_TRY(np_->buf.ensure(np_->nbytes()));
    }
    dws::ParamSpec* p = m->find(name, true);
    if (!p) return DWS_ERR_INVALID;
    DWS_CHECK(dtype == p->dtype, DWS_ERR_INVALID, "'%s': dtype %d, expected %d", name, dtype, p->dtype);
    bool same = (int)p->shape.size() == ndim;
    for (int k = 0; same && k < ndim; ++k) same = p->shape[k] == shape[k];
    if (!same) {
        std::string got = "[", want = "[";
        for (int k = 0; k < ndim; ++k) got += std::to_string(shape[k]) + (k + 1 < ndim ? "," : "");
        for (size_t k = 0; k < p->shape.size(); ++k) want += std::to_string(p->shape[k]) + (k + 1 < p->shape.size() ? "," : "");
        return dws::set_error(DWS_ERR_INVALID, "size mismatch for %s: got %s], expected %s]", name, got.c_str(),
                              want.c_str());
    }
    DWS_HIP(hipMemcpyAsync(p->buf.p, data, p->nbytes(), hipMemcpyDefault, (hipStream_t)stream));
    m->params_touched = true;
    if (dtype == 1) ++m->int_params_version;
    m->dirty = true;
    m->drop_graph();
    return DWS_OK;
}

int dws_model_set_option(dws_model* m, const char* key, const char* value) {
    DWS_CHECK(m && key && value, DWS_ERR_INVALID, "dws_model_set_option: null argument");
    m->drop_graph();
    return m->set_option(key, value);
}

int dws_model_commit(dws_model* m, void* stream) {
    DWS_CHECK(m, DWS_ERR_INVALID, "null model");
    m->params_touched = true;
    return m->commit((hipStream_t)stream);
}

int dws_model_prepare(dws_model* m, int64_t B, int64_t L) {
    DWS_CHECK(m, DWS_ERR_INVALID, "null model");
    const int64_t B0 = m->B, L0 = m->L;
    DWS_TRY(m->prepare(B, L));
    if (m->n_classes > 0 && (B0 != m->B || L0 != m->L)) DWS_TRY(m->reset_labels());   // labels belong to a shape
    if (B0 != m->B || L0 != m->L) m->smp.clip_B = 0;                                        // and so does a seed table
    if (B0 != m->B || L0 != m->L) m->smp.prior_on = false;                                  // and the table of a prior
    return DWS_OK;
}

int dws_model_set_classes(dws_model* m, int32_t n_classes) {
    DWS_CHECK(m, DWS_ERR_INVALID, "null model");
    return m->set_classes(n_classes);
}

int dws_model_set_labels(dws_model* m, const int32_t* labels, int64_t B, void* stream) {
    DWS_CHECK(m, DWS_ERR_INVALID, "null model");
    return m->set_labels(labels, B, (hipStream_t)stream);
}

int dws_model_set_lengths(dws_model* m, const int32_t* lengths, const int32_t* mel_frames, int64_t B, void* stream) {
    DWS_CHECK(m, DWS_ERR_INVALID, "null model");
    return m->set_lengths(lengths, mel_frames, B, (hipStream_t)stream);
}

int dws_sampler_set_cfg(dws_model* m, int32_t on, float scale) {
    DWS_CHECK(m, DWS_ERR_INVALID, "null model");
    DWS_CHECK(!on || (scale == scale && scale - scale == 0.f), DWS_ERR_INVALID, "dws_sampler_set_cfg: scale = %g is not finite",
              (double)scale);
    DWS_CHECK(!on || !m->ragged(), DWS_ERR_UNSUPPORTED, "classifier-free guidance with per-clip lengths (dws_model_set_lengths) is not built");
    DWS_CHECK(!on || !m->smp.prior_on, DWS_ERR_UNSUPPORTED, "classifier-free guidance with an adaptive prior (dws_sampler_set_prior) is not built");
    m->smp.cfg_on = on != 0;
    m->smp.cfg_scale = on ? scale : 0.f;
    return DWS_OK;
}

int dws_sampler_set_clip_seeds(dws_model* m, const uint64_t* seeds, int64_t B, void* stream) {
    DWS_CHECK(m, DWS_ERR_INVALID, "null model");
    return m->set_clip_seeds(seeds, B, (hipStream_t)stream);
}

int dws_sampler_set_prior(dws_model* m, const float* sigma, int64_t B, int64_t n_per_clip, void* stream) {
    DWS_CHECK(m, DWS_ERR_INVALID, "null model");
    return m->set_prior(sigma, B, n_per_clip, (hipStream_t)stream);
}

int dws_model_set_condition(dws_model* m, const float* mel, int64_t Bm, int64_t Tmel, void* stream) {
    DWS_CHECK(m, DWS_ERR_INVALID, "null model");
    m->drop_graph();
    return m->set_condition(mel, Bm, Tmel, (hipStream_t)stream);
}

int dws_model_forward(dws_model* m, const float* audio, const float* steps, float* out, void* stream) {
    DWS_CHECK(m && audio && steps && out, DWS_ERR_INVALID, "dws_model_forward: null argument");
    return m->forward(audio, steps, out, (hipStream_t)stream);
}

int dws_model_forward_train(dws_model* m, const float* audio, const float* steps, float* out, void* stream) {
    DWS_CHECK(m && audio && steps && out, DWS_ERR_INVALID, "dws_model_forward_train: null argument");
    return m->forward_train(audio, steps, out, (hipStream_t)stream);
}

int dws_model_forward_input(dws_model* m, const float* audio, const float* steps, float* out, void* stream) {
    DWS_CHECK(m && audio && steps && out, DWS_ERR_INVALID, "dws_model_forward_input: null argument");
    return m->forward_input(audio, steps, out, (hipStream_t)stream);
}

int dws_model_backward_input(dws_model* m, const float* dout, float* daudio, int32_t param_grads, void* stream) {
    DWS_CHECK(m && dout, DWS_ERR_INVALID, "dws_model_backward: null argument");
    DWS_CHECK(param_grads == 0 || param_grads == 1, DWS_ERR_INVALID, "dws_model_backward_input: param_grads = %d (0 or 1)", param_grads);
    if (!param_grads) {     // data-only: no gradient buffer, sink or group event is involved
        DWS_CHECK(daudio, DWS_ERR_INVALID, "dws_model_backward_input: a data-only backward (param_grads = 0) needs daudio");
        return m->backward(dout, daudio, false, (hipStream_t)stream);
    }
    m->grad_begin();
    const int rc = m->backward(dout, daudio, true, (hipStream_t)stream);
    if (rc != DWS_OK) { m->in_backward = false; return rc; }
    return m->grad_end((hipStream_t)stream);
}

int dws_model_backward(dws_model* m, const float* dout, void* stream) {
    return dws_model_backward_input(m, dout, nullptr, 1, stream);
}

int dws_model_set_grad_sinks(dws_model* m, int32_t count, const char* const* names, float* const* dsts, const int64_t* numels,
                             const int32_t* groups, int32_t ngroups) {
    DWS_CHECK(m && count >= 0 && ngroups >= 0 && (count == 0 || (names && dsts && numels && groups && ngroups > 0)), DWS_ERR_INVALID,
              "dws_model_set_grad_sinks: null argument");
    return m->set_grad_sinks(count, names, dsts, numels, groups, ngroups);
}

int dws_model_grad_group_wait(dws_model* m, int32_t group, void* waiting_stream) {
    DWS_CHECK(m && group >= 0 && (size_t)group < m->grad_groups.size(), DWS_ERR_INVALID, "dws_model_grad_group_wait: group %d of %zu",
              group, m ? m->grad_groups.size() : (size_t)0);
    DWS_CHECK(m->grad_groups[group].flushed, DWS_ERR_STATE, "dws_model_grad_group_wait: no backward has handed group %d over", group);
    DWS_TRY(m->grad_groups[group].ev.make_wait((hipStream_t)waiting_stream));
    return DWS_OK;
}

int dws_model_grad_ready_seq(dws_model* m, int32_t count, const char* const* names, int32_t* seq_out) {
    DWS_CHECK(m && names && seq_out && count >= 0, DWS_ERR_INVALID, "dws_model_grad_ready_seq: null argument");
    DWS_CHECK(!m->grad_touch_prev.empty(), DWS_ERR_STATE, "dws_model_grad_ready_seq: no backward with gradient sinks has run");
    for (int i = 0; i < count; ++i) {
        const dws::ParamSpec* p = m->find(names[i]);
        if (!p) return DWS_ERR_INVALID;
        seq_out[i] = m->grad_touch_prev[p->index];
    }
    return DWS_OK;
}

int dws_model_get_grad(dws_model* m, const char* name, float* dst, int64_t numel, void* stream) {
    DWS_CHECK(m && name && dst, DWS_ERR_INVALID, "dws_model_get_grad: null argument");
    dws::ParamSpec* p = m->find(name);
    if (!p) return DWS_ERR_INVALID;
    DWS_CHECK(p->dtype == 0 && (int64_t)p->numel() == numel, DWS_ERR_INVALID, "'%s': grad has %zu elements, got %lld", name,
              p->numel(), (long long)numel);
    float* g = m->G(name);
    DWS_CHECK(g, DWS_ERR_HIP, "could not allocate the gradient of '%s'", name);
    DWS_HIP(hipMemcpyAsync(dst, g, p->nbytes(), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return DWS_OK;
}

static int multi_copy(dws_model* m, std::vector<dws::CopyJob>& jobs, hipStream_t stream);

int dws_model_update_params(dws_model* m, int32_t count, const char* const* names, const float* const* srcs, void* stream) {
    DWS_CHECK(m && names && srcs && count >= 0, DWS_ERR_INVALID, "dws_model_update_params: null argument");
    if (count == 0) return DWS_OK;
    std::vector<dws::CopyJob> jobs((size_t)count);
    for (int i = 0; i < count; ++i) {
        dws::ParamSpec* p = m->find(names[i], true);
        if (!p) return DWS_ERR_INVALID;
        DWS_CHECK(p->dtype == 0 && srcs[i], DWS_ERR_INVALID, "'%s': update_params takes float32 device tensors", names[i]);
        jobs[i] = {srcs[i], p->buf.f(), (int64_t)p->numel()};
    }
    DWS_TRY(multi_copy(m, jobs, (hipStream_t)stream));
    m->params_touched = true;
    m->dirty = true;
    m->drop_graph();
    return DWS_OK;
}

int dws_model_get_grads(dws_model* m, int32_t count, const char* const* names, float* const* dsts, const int64_t* numels,
                        void* stream) {
    DWS_CHECK(m && names && dsts && numels && count >= 0, DWS_ERR_INVALID, "dws_model_get_grads: null argument");
    if (count == 0) return DWS_OK;
    std::vector<dws::CopyJob> jobs((size_t)count);
    for (int i = 0; i < count; ++i) {
        dws::ParamSpec* p = m->find(names[i]);
        if (!p) return DWS_ERR_INVALID;
        DWS_CHECK(p->dtype == 0 && (int64_t)p->numel() == numels[i], DWS_ERR_INVALID, "'%s': grad has %zu elements, got %lld",
                  names[i], p->numel(), (long long)numels[i]);
        float* g = m->G(names[i]);
        DWS_CHECK(g && dsts[i], DWS_ERR_HIP, "could not allocate the gradient of '%s'", names[i]);
        jobs[i] = {g, dsts[i], numels[i]};
    }
    return multi_copy(m, jobs, (hipStream_t)stream);
}

// One kernel for a list of device-to-device copies.  The job table travels through the pinned staging ring so nothing
// blocks the host.  The device-side table is written and read in stream order.
static int multi_copy(dws_model* m, std::vector<dws::CopyJob>& jobs, hipStream_t stream) {
    const size_t bytes = jobs.size() * sizeof(dws::CopyJob);
    void* h = nullptr;
    DWS_TRY(m->copy_ring.acquire(bytes, &h));
    std::memcpy(h, jobs.data(), bytes);
    dws::DevBuf& table = m->copy_table;
    DWS_TRY(table.ensure(bytes * 2));
    DWS_HIP(hipMemcpyAsync(table.p, h, bytes, hipMemcpyHostToDevice, stream));
    DWS_TRY(m->copy_ring.commit(stream));
    return dws::launch_multi_copy((const dws::CopyJob*)table.p, (int)jobs.size(), stream);
}

// ---- fused optimizer step (optim_kernels.hip) ---------------------------------------------------------------------------
int dws_optim_chunk(void) { return dws::OPTIM_CHUNK; }

int dws_optim_create(dws_optim** out) {
    DWS_CHECK(out, DWS_ERR_INVALID, "dws_optim_create: null argument");
    *out = nullptr;
    dws_optim* o = new dws_optim();
    const size_t bytes = dws::OPTIM_MAX_GRID * sizeof(double) + 2 * sizeof(float);
    int st = o->scratch.ensure(bytes);
    if (st == DWS_OK && hipMemset(o->scratch.p, 0, bytes) != hipSuccess)
        st = dws::set_error(DWS_ERR_HIP, "dws_optim_create: hipMemset failed");
    if (st != DWS_OK) {
        delete o;
        return st;
    }
    *out = o;
    return DWS_OK;
}

int dws_optim_destroy(dws_optim* o) {
    delete o;
    return DWS_OK;
}

int dws_optim_step(dws_optim* o, int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, float* const* ema, float* const* mirrors, const int64_t* numels, const double* lr,
                   const int64_t* step, const double* weight_decay, double beta1, double beta2, double eps, double ema_decay,
                   double max_grad_norm, float* grad_norm_out, dws_model* model, const char* const* names, void* stream) {
    DWS_CHECK(o && count >= 0, DWS_ERR_INVALID, "dws_optim_step: null handle or negative count");
    if (count == 0) return DWS_OK;
    DWS_CHECK(params && grads && exp_avg && exp_avg_sq && numels && lr && step, DWS_ERR_INVALID, "dws_optim_step: null table");
    DWS_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0, DWS_ERR_INVALID,
              "dws_optim_step: betas must lie in [0, 1) and eps must not be negative (got %g, %g, %g)", beta1, beta2, eps);
    DWS_CHECK(!ema || (ema_decay > 0.0 && ema_decay < 1.0), DWS_ERR_INVALID,
              "dws_optim_step: ema_decay must lie in (0, 1) with shadows (got %g)", ema_decay);
    DWS_CHECK(!model || names, DWS_ERR_INVALID, "dws_optim_step: a model needs the parameter names");
    const bool clip = max_grad_norm > 0.0;
    std::vector<dws::OptimJob>& jobs = o->jobs;
    jobs.assign((size_t)count, dws::OptimJob{});
    int64_t chunks = 0;
    bool mirrored = false;
    for (int i = 0; i < count; ++i) {
        dws::OptimJob& j = jobs[i];
        DWS_CHECK(params[i] && grads[i] && exp_avg[i] && exp_avg_sq[i], DWS_ERR_INVALID, "dws_optim_step: tensor %d has a null pointer", i);
        DWS_CHECK(numels[i] > 0 && step[i] >= 1, DWS_ERR_INVALID, "dws_optim_step: tensor %d: numel %lld, step %lld (both must be positive)",
                  i, (long long)numels[i], (long long)step[i]);
        j.p = params[i];
        j.g = grads[i];
        j.m = exp_avg[i];
        j.v = exp_avg_sq[i];
        j.ema = ema ? ema[i] : nullptr;
        j.mirror = mirrors ? mirrors[i] : nullptr;
        j.numel = numels[i];
        if (model && names[i]) {
            dws::ParamSpec* p = model->find(names[i]);
            if (!p) return DWS_ERR_INVALID;
            DWS_CHECK(p->dtype == 0, DWS_ERR_INVALID, "'%s': the optimizer step takes float32 parameters", names[i]);
            DWS_CHECK((int64_t)p->numel() == numels[i], DWS_ERR_INVALID, "'%s': parameter has %zu elements, got %lld", names[i],
                      p->numel(), (long long)numels[i]);
            DWS_CHECK(p->buf.p, DWS_ERR_STATE, "'%s': the model holds no storage for it yet", names[i]);
            j.mirror = p->buf.f();
            mirrored = true;
        }
        // bias corrections in double from the integer step
        const double bc1 = 1.0 - std::pow(beta1, (double)step[i]), bc2 = 1.0 - std::pow(beta2, (double)step[i]);
        j.step_size = (float)(lr[i] / bc1);
        j.sqrt_bc2 = (float)std::sqrt(bc2);
        j.weight_decay = weight_decay ? (float)weight_decay[i] : 0.f;
        const uintptr_t bits = (uintptr_t)j.p | (uintptr_t)j.g | (uintptr_t)j.m | (uintptr_t)j.v | (uintptr_t)j.ema | (uintptr_t)j.mirror;
        j.vec = (bits & 15) == 0;
        DWS_CHECK((bits & 3) == 0, DWS_ERR_INVALID, "dws_optim_step: tensor %d is not 4-byte aligned", i);
        j.first_chunk = (int32_t)chunks;
        chunks += (numels[i] + dws::OPTIM_CHUNK - 1) / dws::OPTIM_CHUNK;
        DWS_CHECK(chunks < (int64_t)1 << 30, DWS_ERR_UNSUPPORTED, "dws_optim_step: more than 2^30 chunks");
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = jobs.size() * sizeof(dws::OptimJob);
    void* staged = nullptr;
    DWS_TRY(o->ring.acquire(bytes, &staged));
    std::memcpy(staged, jobs.data(), bytes);
    DWS_TRY(o->table.ensure(bytes * 2));
    DWS_HIP(hipMemcpyAsync(o->table.p, staged, bytes, hipMemcpyHostToDevice, s));
    DWS_TRY(o->ring.commit(s));
    const dws::OptimJob* table = (const dws::OptimJob*)o->table.p;
    if (clip || grad_norm_out)
        DWS_TRY(dws::launch_optim_norm(table, count, (int)chunks, o->partials(), o->counter(), o->norm(), grad_norm_out, s));
    dws::OptimHyper h;
    h.om_beta1 = (float)(1.0 - beta1);
    h.beta2 = (float)beta2;
    h.om_beta2 = (float)(1.0 - beta2);
    h.eps = (float)eps;
    h.ema_w = ema ? (float)(1.0 - ema_decay) : 0.f;
    h.max_norm = clip ? (float)max_grad_norm : 0.f;
    DWS_TRY(dws::launch_optim_step(table, count, (int)chunks, h, clip ? o->norm() : nullptr, s));
    if (mirrored) {      // as dws_model_update_params: the raw store changed
        model->params_touched = true;
        model->dirty = true;
        model->drop_graph();
    }
    return DWS_OK;
}

int dws_model_read_tap(dws_model* m, const char* tap, float* dst, int64_t capacity, void* stream) {
    DWS_CHECK(m && tap && dst, DWS_ERR_INVALID, "dws_model_read_tap: null argument");
    if (std::strcmp(tap, "sampler_eps") == 0) {     // the network output of the sampler's last reverse step
        const int64_t n = m->B * m->d.out_channels * m->L;
        DWS_CHECK(m->smp.eps.p && capacity >= n, DWS_ERR_INVALID, "tap sampler_eps: no sampler step has run, or capacity %lld < %lld",
                  (long long)capacity, (long long)n);
        // the buffer is sized by the last sampler step: after a prepare() to a larger shape it no longer matches
        DWS_CHECK(m->smp.eps.bytes >= (size_t)n * 4 && m->smp.eps_B == m->B && m->smp.eps_L == m->L, DWS_ERR_STATE,
                  "tap sampler_eps: the last sampler step ran at B=%lld L=%lld, the model is prepared for B=%lld L=%lld",
                  (long long)m->smp.eps_B, (long long)m->smp.eps_L, (long long)m->B, (long long)m->L);
        DWS_HIP(hipMemcpyAsync(dst, m->smp.eps.p, (size_t)n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return DWS_OK;
    }
    if (std::strcmp(tap, "sampler_graphs") == 0) {  // number of sampler graphs this model has instantiated (one float)
        DWS_CHECK(capacity >= 1, DWS_ERR_INVALID, "tap buffer too small");
        const float v = (float)m->smp.graphs_made;
        DWS_HIP(hipMemcpyAsync(dst, &v, 4, hipMemcpyHostToDevice, (hipStream_t)stream));
        DWS_HIP(hipStreamSynchronize((hipStream_t)stream));
        return DWS_OK;
    }
    return m->read_tap(tap, dst, capacity, (hipStream_t)stream);
}

int dws_sampler_run(dws_model* m, float* x, const float* alpha, const float* alpha_bar, const float* sigma,
                    int32_t T, const float* noise, uint64_t seed, int32_t init_from_seed, int32_t use_graph,
                    void* stream) {
    DWS_CHECK(m && x, DWS_ERR_INVALID, "dws_sampler_run: null argument");
    DWS_CHECK(!m->smp.cfg_on, DWS_ERR_UNSUPPORTED, "classifier-free guidance runs on dws_sampler_run_schedule only (dws_sampler_run)");
    DWS_CHECK(m->smp.clip_B == 0, DWS_ERR_UNSUPPORTED, "per-clip seeds run on the schedule entries only (dws_sampler_run)");
    DWS_CHECK(!m->smp.prior_on, DWS_ERR_UNSUPPORTED, "an adaptive prior runs on the schedule entries only (dws_sampler_run)");
    return dws::sampler_run(m, x, alpha, alpha_bar, sigma, T, noise, seed, init_from_seed, use_graph,
                            (hipStream_t)stream);
}

int dws_sampler_steps(dws_model* m, float* x, const float* alpha, const float* alpha_bar, const float* sigma,
                      int32_t T, int32_t t_start, int32_t n_steps, uint64_t seed, int32_t use_graph, void* stream) {
    DWS_CHECK(m && x, DWS_ERR_INVALID, "dws_sampler_steps: null argument");
    DWS_CHECK(!m->smp.cfg_on, DWS_ERR_UNSUPPORTED, "classifier-free guidance runs on dws_sampler_run_schedule only (dws_sampler_steps)");
    DWS_CHECK(m->smp.clip_B == 0, DWS_ERR_UNSUPPORTED, "per-clip seeds run on the schedule entries only (dws_sampler_steps)");
    DWS_CHECK(!m->smp.prior_on, DWS_ERR_UNSUPPORTED, "an adaptive prior runs on the schedule entries only (dws_sampler_steps)");
    return dws::sampler_steps(m, x, alpha, alpha_bar, sigma, T, t_start, n_steps, seed, use_graph,
                              (hipStream_t)stream);
}

int dws_sampler_run_schedule(dws_model* m, float* x, int32_t kind, int32_t S, const float* net_steps,
                             const float* coef, const float* noise, uint64_t seed, int32_t init_from_seed,
                             int32_t use_graph, void* stream) {
    DWS_CHECK(m && x, DWS_ERR_INVALID, "dws_sampler_run_schedule: null argument");
    return dws::sampler_run_schedule(m, x, kind, S, net_steps, coef, noise, seed, init_from_seed, use_graph, nullptr,
                                     nullptr, (hipStream_t)stream);
}

int dws_sampler_run_edit(dws_model* m, float* x, int32_t kind, int32_t S, const float* net_steps, const float* coef,
                         const float* noise, uint64_t seed, int32_t init_from_seed, int32_t use_graph,
                         const dws_sampler_edit* edit, void* stream) {
    DWS_CHECK(m && x && edit, DWS_ERR_INVALID, "dws_sampler_run_edit: null argument");
    DWS_CHECK(!m->smp.cfg_on, DWS_ERR_UNSUPPORTED, "classifier-free guidance runs on dws_sampler_run_schedule only (dws_sampler_run_edit)");
    return dws::sampler_run_schedule(m, x, kind, S, net_steps, coef, noise, seed, init_from_seed, use_graph, edit,
                                     nullptr, (hipStream_t)stream);
}

int dws_sampler_run_program(dws_model* m, float* x, int32_t kind, int32_t S, const float* net_steps, const float* coef,
                            int32_t V, const int32_t* visit_step, const float* jump_coef, const float* noise,
                            uint64_t seed, int32_t init_from_seed, int32_t use_graph, const dws_sampler_edit* edit,
                            void* stream) {
    DWS_CHECK(m && x && edit, DWS_ERR_INVALID, "dws_sampler_run_program: null argument");
    DWS_CHECK(!m->smp.cfg_on, DWS_ERR_UNSUPPORTED, "classifier-free guidance runs on dws_sampler_run_schedule only (dws_sampler_run_program)");
    return dws::sampler_run_program(m, x, kind, S, net_steps, coef, V, visit_step, jump_coef, noise, seed,
                                    init_from_seed, use_graph, edit, (hipStream_t)stream);
}

int dws_philox_normal(float* x, int64_t n, uint64_t seed, uint32_t stream_id, void* stream) {
    return dws::philox_normal(x, n, seed, stream_id, (hipStream_t)stream);
}

int dws_philox_normal_clips(float* x, int64_t B, int64_t n_per_clip, const uint64_t* seeds, uint32_t stream_id,
                            void* stream) {
    return dws::philox_normal_clips(x, B, n_per_clip, seeds, stream_id, (hipStream_t)stream);
}

}  // extern "C"
