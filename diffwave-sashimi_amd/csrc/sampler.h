// Host state of the samplers (sampler.hip), one per model: dws_model::smp.  The backbones read none of it; what they
// share with the sampler -- step_idx and step_table_gen -- sits on dws_model.
#pragma once
#include "host_util.h"

namespace dws {

struct SamplerState {
    // ---- the full-T sampler (dws_sampler_run / dws_sampler_steps)
    DevBuf tables;                   // [3][T] c1, c2, sigma
    std::vector<float> host_tables;  // host copy of what is resident (upload skipped when identical)
    DevBuf state;                    // int32 step index
    DevBuf eps;                      // eps[B, Cout, L]
    int64_t eps_B = 0, eps_L = 0;    // shape of the sampler step that last wrote it
    hipGraphExec_t graph = nullptr;
    Stream stream;                   // capture/replay stream (the caller's may be the null stream)
    Event ev_in, ev_out;
    // key of the captured graph
    int64_t g_B = 0, g_L = 0;
    int g_T = 0;
    const void* g_x = nullptr;
    const void* g_noise = nullptr;
    uint64_t g_seed = 0;
    bool g_ragged = false;           // captured with per-clip lengths on (the step then holds the sealing launches)
    // ---- few-step sampler (dws_sampler_run_schedule): tables, state, x and graph of its own -- the two entry points never
    // replay each other's graph.  Its graph updates sch_x in place and reads the seed from sch_state, so neither the
    // caller's x nor the seed is baked in.
    DevBuf sch_tables;                    // DDPM [3][S] c1, c2, sigma; DDIM [5][S] k1 .. k5; DPM-Solver++(2M) [5][S] m1 .. m5
    std::vector<float> sch_host_tables;   // host copy of what is resident (upload skipped when identical)
    DevBuf sch_state;                     // int32 step index, int32 finished update blocks, uint64 Philox seed, int32 visit,
                                          // int32 history-valid word (DPM-Solver++(2M): sch_hist holds the last step's x0)
    DevBuf sch_x;                         // [B, C, L]
    DevBuf sch_hist;                      // [B, C, L] the previous step's data prediction (DWS_SAMPLER_DPMPP2M; first use)
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
        const void* lengths = nullptr;                   // the per-clip length table (null: lengths off)
        const void* prior = nullptr;                     // the adaptive prior's table (null: N(0, I))
        bool operator==(const SchKey& o) const {
            return prior == o.prior && lengths == o.lengths && B == o.B && L == o.L && S == o.S && kind == o.kind && vec == o.vec && tables == o.tables &&
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
    } sch_graphs[SCH_GRAPHS][8];     // [form of seed + 2 * per-clip lengths on + 4 * adaptive prior on]: a step with lengths on holds the launches
                                     // that seal the padding (it reads the length table from device memory: a new table
                                     // replays it), so lengths on / off alternate without a new capture as the rest does
    // editing: the known clip and the mask are copied into model-owned buffers before the replays, like x into sch_x.
    DevBuf sch_edit;                      // [2][S] q1, q2 of sampling.edit_coefficients
    std::vector<float> sch_host_edit;     // host copy of what is resident
    DevBuf sch_known;                     // float [B, C, L]
    DevBuf sch_mask;                      // uint8 [B, C, L] (rounded up to whole groups of four)
    // resampling: the program tables sit in a model-owned buffer keyed on their contents, so a new program of the same V
    // replays the held graph.
    DevBuf sch_prog;                      // int32 step_of[V], float ja[V], jb[V], indexed by the visit number
    std::vector<uint32_t> sch_host_prog;  // host copy of what is resident
    // classifier-free guidance in the schedule step: the model is prepared for 2 Bc clips, the first half carries the
    // wanted labels and the second the null class; the update runs on the first half alone.  The scale sits in the
    // device state (word 6).
    bool cfg_on = false;
    float cfg_scale = 0.f;
    // per-clip seeds (dws_sampler_set_clip_seeds): clip b draws from Philox key clip_seeds[b] with groups numbered inside
    // the clip, so its noise does not depend on the batch around it.  The table sits in device memory (a new one replays
    // the captured step) and holds until it is changed or the model is prepared for another shape.
    DevBuf clip_seeds;                    // uint64 [clip_B]
    int64_t clip_B = 0;                   // clips the table holds (0: off, the scalar seed of the run entries)
    StagingRing seed_ring{4};             // pinned staging of the table's upload
    // adaptive prior (dws_sampler_set_prior; PriorGrad, Lee et al., ICLR 2022): the run ends in N(0, diag(prior^2)) -- every
    // standard-normal number a schedule run consumes, drawn or injected, is multiplied by the table at its position first
    // (the PRIOR kernel instances).  The table sits in device memory at the shape of the sampler state (a new one replays
    // the captured step) and holds until it is changed or the model is prepared for another shape.
    DevBuf prior;                         // float [prior_B, prior_n]
    int64_t prior_B = 0, prior_n = 0;     // n = C L elements per clip
    bool prior_on = false;
    int64_t graphs_made = 0;              // tap "sampler_graphs": graphs instantiated by either entry point

    SamplerState() = default;
    SamplerState(const SamplerState&) = delete;
    SamplerState& operator=(const SamplerState&) = delete;
    ~SamplerState() { drop_graph(); }
    void drop_graph() {
        if (graph) hipGraphExecDestroy(graph);
        graph = nullptr;
        for (auto& flavour : sch_graphs)
            for (SchGraph& g : flavour) {
                if (g.exec) hipGraphExecDestroy(g.exec);
                g.exec = nullptr;
            }
    }
};

}  // namespace dws
