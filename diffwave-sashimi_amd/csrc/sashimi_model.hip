// SaShiMi backbone behind the C ABI (`models/sashimi.py:187-313`, `models/s4.py`).
//
// Everything that does not depend on x_t is evaluated once per weight load in
// commit(): weight-norm folding, the S4 convolution kernels (Cauchy -> Woodbury
// -> bilinear factor -> irfft -> two-sided kernel -> rfft = K_f per layer; the
// reference regenerates these in all 30 layers on every reverse step,
// `s4.py:1388`) and, in set_condition(), the mel conditioner terms.
// The per-step path is then LN+emb -> rocFFT r2c -> spectrum multiply -> c2r ->
// D-skip+GELU -> 1x1+GLU+residual -> LN -> FF -> residual per block.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "conditioner.h"
#include "fftconv.h"
#include "model.h"
#include "s4_kernel_chain.h"
#include "sashimi.h"
#include "sashimi_mfma.h"
#include "sashimi_train.h"
#include "wavenet.h"
#include "wavenet_backward.h"

namespace dws {

enum { L_BLOCK = 0, L_DOWN = 1, L_UP = 2 };

struct SLayer {
    int kind, H, L, p = 1, Hout = 0, Lout = 0;   // L / Lout: lengths of the CURRENT run (prepare rescales them)
    int L0 = 0, Lout0 = 0;                       // as configured (model L)
    int Lk = 0;                                  // S4 kernel length = the block's `L` buffer
    uint64_t Lk_version = 0;                     // int_params_version at which Lk was read back
    std::string prefix;
    int pt_off = 0;       // offset of this block's fc_t rows in the stacked projection
    int stage = 0;        // index into per-(H,L) workspaces
    DevBuf W1, W2, Wp;    // folded ff / pool weights
    DevBuf Ao, A1, A2, rs1, Ap;  // MFMA-packed copies (+ row sums of W1 for the folded LayerNorm)
    DevBuf Ao_c, A1_c, A2_c;     // H <= 64: the same weights with chain-ordered columns (sashimi_chain.hip)
    DevBuf Ao_c6, A1_c6, A2_c6;  // precision = bf16x6 / f16x3: split fragments in the 16-wide chain order (sashimi_chain6.hip)
    DevBuf wscale_c6;            // f16x3: the three matrices' power-of-two scales
    bool mfma = false, mfma2 = false;
    DevBuf Kf;            // rocFFT path: [H][L+1] complex spectrum of the two-sided kernel (n = 2L)
    S4Chain own;          // the block's kernel generation as a chain of its own (not used while the block belongs to a group);
                          // own.kfa / kfb / kfs also hold the first of the segmented path's three spectra
    const void *kfa_v = nullptr, *kfb_v = nullptr, *kfs_v = nullptr;   // fused path: what the convolution reads -- this block's rows
                                                                       // of its chain's pair-ordered spectra (take_spectra)
    int grp = -1, gidx = 0;   // training: stacked kernel generation -- group (blocks of one shape) and position in it
    int log2m = 0;        // > 0: fused LDS FFT convolution is used for this block
    bool seg = false;     // stage longer than the largest LDS transform: segmented fused path (fftconv_seg_kernel)
    DevBuf kfa_c, kfb_c, kfs_c, kfa_a, kfb_a, kfs_a;   // seg: spectra of the causal / anti-causal kernel half, shifted
    DevBuf melW0, melW1, melWc, melc;
    DevBuf out;           // activation produced by this layer
    // training path: saved activations, gradient w.r.t. `out`, transposed weights in A-fragment order
    DevBuf t_u, t_a, t_g, t_o, t_x1, t_n2, t_f1, t_ge, t_xr, dbuf;   // t_g = gelu(t_a), t_ge = gelu(t_f1): kept so the
                                                                    // weight gradients need no GELU recompute
    DevBuf tAo, tA1, tA2, tAp, tAoT, tA1T, tA2T, tApT;
    const float *pAo = nullptr, *pA1 = nullptr, *pA2 = nullptr, *pAp = nullptr;   // forward operands of the training GEMMs: the
                                                                                 // commit's packs where they exist, else tA*
};

struct Exec {             // one step of Sashimi.forward: out_node = layer(in_node) (+ add_node)
    SLayer* l;
    int in_node, add_node;
};

struct Stage {
    int H, L, L0 = 0;
    bool rocfft = false;  // some block of this stage needs the rocFFT path
    bool seg = false;     // stage runs the segmented fused convolution (L > 16384)
    bool force_rocfft = false;   // resolve_segmented_stages(): a checkpoint's kernels carry more taps than one segment holds, so
                                 // this stage runs on rocFFT whatever prepare() would pick from the configured length; holds
                                 // until the run length changes (the decision depends on L and the `L` buffers only, not on B)
    DevBuf U, Uf, Y, g, x1, n2, ffu, y;
    DevBuf d2, dh, dx1, du;  // training path gradients: [B][max(2,FF) H][L], [B][H][L] x 3
    DevBuf Gf;               // training on rocFFT: the spectrum of the block's input u, recomputed in the backward ([B][H][L+1])
};

// Training: the S4 blocks of one shape (H, L) -- 12 + 12 + 6 in BASELINE config 5 -- generate their kernels, and run the adjoint of
// that generation, STACKED along H: every launch of the chain (s4_prep, Cauchy, Woodbury, rocFFT, re-placement, spectrum, pair
// order; and backwards) is indexed by a row h < H and is launched once over n * H rows.  Per block the chain is ~12 launches of
// 5-80 us each way, latency-bound: 30 blocks x 24 launches = 7.6 ms of a 134 ms step before, three chains each way after.
struct KGroup {
    int H = 0, L = 0, log2m = 0;
    std::vector<SLayer*> layers;
    S4Chain chain;                         // over Ht rows; chain.par points at the stacked parameters below
    DevBuf C, Bp, P, iwr, wim, logdt;      // stacked parameters: [2][Ht][N] complex, [Ht][N] complex x 2, [Ht][N] x 2, [Ht]
    DevBuf dKf, gC, gB, gP, giwr, gwim, glogdt, gD;   // adjoint: stacked spectrum gradient, stacked parameter gradients
    int pending = 0;                       // blocks of this backward whose correlation has not run yet
    CopyBatch stack, unstack;
    int Ht() const { return H * (int)layers.size(); }
};

struct SashimiModel : dws_model, S4Workspace {
    int Cin, Cout, D, NL, E, FF, NS = 32, Ein, Emid, Eout, MB;
    bool cond, unet;
    std::vector<int> pool;
    std::vector<SLayer*> d_layers, c_layers, u_layers, all;
    std::vector<Stage*> stages;
    int pt_total = 0;
    DevBuf Wi, Wt_all, bt_all, Wf, Af, freq;
    CopyBatch stack_fc_t, unstack_fc_t;   // per-layer fc_t tensors <-> their stacked buffers, one launch each
    bool freq_ready = false;
    DevBuf x_init, emb, h1, h2, part_t, nfin, scratch_out;
    int64_t melBm = 0;
    // training path
    std::vector<Exec> plan;
    DevBuf dx_init, ty, ta1, ta2, tAfT, tmp_pack, wpart, dWfold, lnpart, pool_scr, chain_tmp, dpt, dh2, dh1, dWt_all, dbt_all;
    DevBuf bpart, fpart, dKf, dyb, dnf;
    uint64_t commit_version = 0, train_pack_version = ~0ull;
    bool keep_cauchy = false;         // set by the first forward_train: commits then keep every chain's Cauchy products
    std::vector<KGroup*> kgroups;     // training commits: blocks grouped by shape (build_kernels_stacked)
    bool kernels_stacked = false;     // the last commit generated the kernels group by group
    bool trained_fwd = false;
    bool input_only = false;          // the pending training forward came from forward_input: a data-only backward alone may follow
    const float* train_audio = nullptr;
    DevBuf mel_in;                    // copy of the installed mel [Bm][MB][Tmel] (conditioner adjoint)
    DevBuf mel_u0, mel_u1;            // upsampler scratch of set_condition (kept: no allocation / wait per utterance)
    int mel_T = 0;
    CondTrainWs cws;
    DevBuf gW0f, gW1f, gWcf;

    // precision option: the H <= 128 tails on the 16-bit matrix cores (sashimi_chain6.hip): bf16x6 = 3-term bf16 split, six
    // products; f16x3 = 2-term fp16 split of scaled operands, three products
    bool bf16x6 = false, f16x3 = false;
    bool split_tails() const { return bf16x6 || f16x3; }
    int set_option(const std::string& key, const std::string& value) override {
        if (key == "precision") {
            if (value == "f32" || value == "bf16x6" || value == "f16x3") {
                const bool b6 = value == "bf16x6", f3 = value == "f16x3";
                if (b6 != bf16x6 || f3 != f16x3) { bf16x6 = b6; f16x3 = f3; dirty = true; drop_graph(); trained_fwd = false; }
                return DWS_OK;
            }
            return set_error(DWS_ERR_UNSUPPORTED, "sashimi: precision=%s is not built (f32 | bf16x6 | f16x3)", value.c_str());
        }
        if (key == "train_ln_fusion") {     // 0: separate LayerNorm passes in forward_train (parity / A-B runs); default 1
            train_ln_fusion = value != "0";
            return DWS_OK;
        }
        return dws_model::set_option(key, value);
    }

    ~SashimiModel() override {
        for (auto* g : kgroups) delete g;
        for (auto* l : all) delete l;
        for (auto* s : stages) delete s;
    }

    void wn(const std::string& p, std::vector<int64_t> vshape) {
        std::vector<int64_t> g(vshape.size(), 1);
        g[0] = vshape[0];
        add_param(p + ".bias", {vshape[0]});
        add_param(p + ".weight_g", g);
        add_param(p + ".weight_v", vshape);
    }

    int stage_of(int H, int L) {
        for (size_t i = 0; i < stages.size(); ++i)
            if (stages[i]->H == H && stages[i]->L == L) return (int)i;
        auto* s = new Stage();
        s->H = H; s->L = L;
        stages.push_back(s);
        // FFT nodes for this length, computed by the host side with the reference's own
        // complex64 expression (s4.py:561-565) -- rounding-sensitive, SURVEY.md 7.
        add_param("__omega." + std::to_string(L), {L / 2 + 1, 2});
        add_param("__z." + std::to_string(L), {L / 2 + 1, 2});
        return (int)stages.size() - 1;
    }

    SLayer* mk_block(const std::string& prefix, int H, int L) {
        auto* l = new SLayer();
        l->kind = L_BLOCK; l->H = H; l->L = L; l->prefix = prefix;
        l->pt_off = pt_total; pt_total += H;
        l->stage = stage_of(H, L);
        add_param(prefix + ".fc_t.weight", {H, Eout});
        add_param(prefix + ".fc_t.bias", {H});
        add_param(prefix + ".layer.D", {1, H});
        const std::string k = prefix + ".layer.kernel.kernel";
        add_param(k + ".C", {2, H, NS, 2});
        add_param(k + ".log_dt", {H});
        add_param(k + ".B", {1, H, NS, 2});
        add_param(k + ".P", {1, H, NS, 2});
        add_param(k + ".inv_w_real", {H, NS});
        add_param(k + ".w_imag", {H, NS});
        add_param(k + ".L", {}, 1);
        add_param(prefix + ".layer.output_linear.0.weight", {2 * H, H, 1});
        add_param(prefix + ".layer.output_linear.0.bias", {2 * H});
        wn(prefix + ".ff.ff.0.conv", {FF * H, H, 1});
        wn(prefix + ".ff.ff.2.conv", {H, FF * H, 1});
        for (const char* nrm : {".norm1", ".norm2"}) {
            add_param(prefix + nrm + ".m", {1});
            add_param(prefix + nrm + ".s", {1});
        }
        if (cond) {
            for (int i = 0; i < 2; ++i) {
                const std::string u = prefix + ".upsample_conv2d." + std::to_string(i);
                add_param(u + ".bias", {1});
                add_param(u + ".weight_g", {1, 1, 1, 1});
                add_param(u + ".weight_v", {1, 1, 3, 2 * d.mel_upsample[i]});
            }
            wn(prefix + ".mel_conv.conv", {H, MB, 1});
        }
        all.push_back(l);
        return l;
    }

    SLayer* mk_pool(const std::string& prefix, int kind, int Hin, int Lin, int p) {
        auto* l = new SLayer();
        l->kind = kind; l->H = Hin; l->L = Lin; l->p = p; l->prefix = prefix;
        if (kind == L_DOWN) {
            l->Hout = Hin * E; l->Lout = Lin / p;
            wn(prefix + ".linear.conv", {l->Hout, Hin * p, 1});
        } else {
            l->Hout = Hin / E; l->Lout = Lin * p;
            wn(prefix + ".linear.conv", {l->Hout * p, Hin, 1});
        }
        all.push_back(l);
        return l;
    }

    explicit SashimiModel(const dws_model_desc& dd) {
        d = dd;
        Cin = d.in_channels; Cout = d.out_channels; D = d.d_model; NL = d.n_layers; E = d.expand; FF = d.ff;
        Ein = d.diffusion_step_embed_dim_in; Emid = d.diffusion_step_embed_dim_mid; Eout = d.diffusion_step_embed_dim_out;
        MB = d.mel_bands; cond = !d.unconditional; unet = d.unet != 0;
        for (int i = 0; i < d.n_pool; ++i) pool.push_back(d.pool[i]);
        wn("init_conv.0.conv", {D, Cin, 1});
        add_param("fc_t1.weight", {Emid, Ein});
        add_param("fc_t1.bias", {Emid});
        add_param("fc_t2.weight", {Eout, Emid});
        add_param("fc_t2.bias", {Eout});
        label_param = "label_embedding.weight";   // registered by dws_model_set_classes
        // layer plan of `Sashimi.__init__` (sashimi.py:236-268)
        int H = D, L = d.L, idx = 0;
        for (int p : pool) {
            if (unet)
                for (int i = 0; i < NL; ++i) d_layers.push_back(mk_block("d_layers." + std::to_string(idx++), H, L));
            d_layers.push_back(mk_pool("d_layers." + std::to_string(idx++), L_DOWN, H, L, p));
            L /= p; H *= E;
        }
        for (int i = 0; i < NL; ++i) c_layers.push_back(mk_block("c_layers." + std::to_string(i), H, L));
        idx = 0;
        for (auto it = pool.rbegin(); it != pool.rend(); ++it) {
            const int p = *it;
            u_layers.push_back(mk_pool("u_layers." + std::to_string(idx++), L_UP, H, L, p));
            H /= E; L *= p;
            for (int i = 0; i < NL; ++i) u_layers.push_back(mk_block("u_layers." + std::to_string(idx++), H, L));
        }
        for (auto* l : all) { l->L0 = l->L; l->Lout0 = l->Lout; }
        for (auto* st : stages) st->L0 = st->L;
        add_param("norm.m", {1});
        add_param("norm.s", {1});
        wn("final_conv.0.conv", {D, D, 1});
        add_param("final_conv.2.conv.weight", {Cout, D, 1});
        add_param("final_conv.2.conv.bias", {Cout});
    }

    // commit(): the fold joins the commit's batched weight preparation (PrepBatch: run once, before anything reads `out`)
    PrepBatch prep, prep_train;
    int fold(const std::string& p, float* out, int O, int inner, hipStream_t) {
        prep.fold(P(p + ".weight_v"), P(p + ".weight_g"), out, O, inner);
        return DWS_OK;
    }

    // length the kernel of a block was set up for (its `L` buffer): read back only when an int64 buffer was re-sent
    int kernel_len(SLayer* l, hipStream_t s, int64_t* out) {
        int64_t Lbuf = l->Lk;
        if (l->Lk_version != int_params_version) {
            DWS_HIP(hipMemcpyAsync(&Lbuf, P(l->prefix + ".layer.kernel.kernel.L"), 8, hipMemcpyDeviceToHost, s));
            DWS_HIP(hipStreamSynchronize(s));
            l->Lk_version = int_params_version;
            l->Lk = (int)Lbuf;
        }
        *out = Lbuf;
        return DWS_OK;
    }

    // rocFFT path of a stage: zero-padded input rows, spectrum, output rows, and the two plans (allocated here, never
    // inside a stream capture)
    int ensure_rocfft_stage(Stage* st) {
        const size_t rows = (size_t)B * st->H, Ls = st->L;
        const bool fresh = st->U.bytes < rows * 2 * Ls * 4;
        DWS_TRY(st->U.ensure(rows * 2 * Ls * 4));
        if (fresh) DWS_HIP(hipMemset(st->U.p, 0, rows * 2 * Ls * 4));  // zero padding of the FFT input rows
        DWS_TRY(st->Uf.ensure(rows * (Ls + 1) * 8));
        DWS_TRY(st->Y.ensure(rows * 2 * Ls * 4));
        RocfftPlan* plan = nullptr;
        DWS_TRY(fft.get(0, 2 * st->L, (int)B * st->H, &plan));
        DWS_TRY(fft.get(1, 2 * st->L, (int)B * st->H, &plan));
        return DWS_OK;
    }

    // prepare() picks the segmented convolution from the CONFIGURED stage length; a checkpoint whose kernels were set
    // up for a longer l_max (its `L` buffers) can carry more taps than one segment holds: such a stage runs on rocFFT
    int resolve_segmented_stages(hipStream_t s) {
        for (auto* st : stages) {
            if (!st->seg && !st->force_rocfft) continue;
            bool fits = true;
            for (auto* l : all) {
                if (l->kind != L_BLOCK || stages[l->stage] != st) continue;
                int64_t Lk = 0;
                DWS_TRY(kernel_len(l, s, &Lk));
                if (Lk > 0 && !fftconv_seg_supported(st->L, (int)std::min<int64_t>(st->L, Lk))) fits = false;
            }
            if (!fits && st->seg) {
                st->seg = false;
                st->force_rocfft = true;      // prepare() keeps this stage on rocFFT (also for another B) until L changes
                drop_graph();
                DWS_TRY(ensure_rocfft_stage(st));
            } else if (fits && st->force_rocfft) {   // the `L` buffers were re-sent with shorter kernels: back to the segmented path
                st->force_rocfft = false;
                st->rocfft = false;           // (build_kernel sets it again if a block of the stage still needs the fallback)
                st->seg = true;
                drop_graph();
                DWS_TRY(st->y.ensure((size_t)B * st->H * st->L * 4));
            }
        }
        return DWS_OK;
    }

    // the six kernel tensors of a block, or (backward: G() records the access) their gradients
    S4Tensors kernel_tensors(const SLayer* l, bool grad) {
        const std::string k = l->prefix + ".layer.kernel.kernel";
        auto t = [&](const char* name) { return grad ? G(k + name) : P(k + name); };
        return {t(".C"), t(".B"), t(".P"), t(".inv_w_real"), t(".w_imag"), t(".log_dt")};
    }

    // Cauchy products of this commit's chains: kept for the backward in training mode (commit() bumps commit_version when it
    // is done), in the shared scratch otherwise
    uint64_t products_version() const { return keep_cauchy ? commit_version + 1 : S4_NOT_KEPT; }

    // one block as a chain over its own tensors, at the length its kernel was set up for
    int block_chain(SLayer* l, S4Chain& c, hipStream_t s) {
        const std::string k = l->prefix + ".layer.kernel.kernel";
        int64_t Lbuf = 0;
        DWS_TRY(kernel_len(l, s, &Lbuf));
        // the kernel is generated at its own length l_max; a run uses its first min(L, l_max) taps per direction
        // (`L_kernel`, s4.py:1387,805): shorter inputs truncate it, longer inputs keep l_max taps
        DWS_CHECK(Lbuf > 0 && Lbuf < (1 << 28), DWS_ERR_STATE,
                  "%s.L = %lld: C must have been through _setup_C(l_max) (s4.py:524-551) before it is handed to the engine",
                  k.c_str(), (long long)Lbuf);
        l->Lk = (int)Lbuf;
        const std::string zname = "__z." + std::to_string(l->Lk), oname = "__omega." + std::to_string(l->Lk);
        DWS_CHECK(P(zname) && P(oname), DWS_ERR_STATE, "FFT nodes %s / %s were not handed to the engine", zname.c_str(),
                  oname.c_str());
        c.rows = l->H; c.N = NS; c.Lk = l->Lk;
        c.par = kernel_tensors(l, false); c.z = P(zname); c.omega = P(oname);
        return DWS_OK;
    }

    // the blocks of a chain read their H rows of its pair-ordered spectra
    static void take_spectra(const S4Chain& c, SLayer* const* blocks, size_t n, int lg) {
        const size_t half = (size_t)1 << (lg - 1);
        for (size_t i = 0; i < n; ++i) {
            SLayer* l = blocks[i];
            l->kfa_v = c.kfa.f() + i * l->H * half * 2;
            l->kfb_v = c.kfb.f() + i * l->H * half * 2;
            l->kfs_v = c.kfs.f() + i * l->H * 3 * 2;
            l->Lk = c.Lk; l->log2m = lg; l->seg = false;
        }
    }

    // S4 convolution kernel of one block: parameters -> K_f   (s4.py:704-807, 1391-1403)
    int build_kernel(SLayer* l, hipStream_t s) {
        const int H = l->H, L = l->L;
        S4Chain& c = l->own;
        DWS_TRY(block_chain(l, c, s));
        const int Lk = c.Lk, Lt = std::min(L, Lk);
        DWS_TRY(s4_taps_forward(*this, c, products_version(), s));
        int lg = 0;
        if (fftconv_supported(L, &lg) && !getenv("DWS_SASHIMI_ROCFFT")) {
            DWS_TRY(s4_fused_spectrum(*this, c, Lt, lg, s));
            take_spectra(c, &l, 1, lg);
        } else if (stages[l->stage]->seg) {
            // vocoding lengths: three pair-ordered spectra at M = 16384 -- the two-sided kernel, and its causal and
            // anti-causal halves alone shifted by half the transform ((-1)^k), see FftConvSegArgs
            DWS_CHECK(fftconv_seg_supported(L, Lt), DWS_ERR_UNSUPPORTED,
                      "%s: stage of %d samples with %d kernel taps per direction: more taps than one 16384-sample segment",
                      (l->prefix + ".layer.kernel.kernel").c_str(), L, Lt);
            lg = FFTCONV_SEG_LOG2M;
            const int M = 1 << lg, Nf = 2 * M;
            FftTables* t;
            DWS_TRY(get_tables(lg, &t, s));
            DWS_TRY(cK.ensure((size_t)H * Nf * 4));
            DWS_TRY(cKf.ensure((size_t)H * (M + 1) * 8));
            DevBuf* dst[3][3] = {{&c.kfa, &c.kfb, &c.kfs}, {&l->kfa_c, &l->kfb_c, &l->kfs_c}, {&l->kfa_a, &l->kfb_a, &l->kfs_a}};
            for (int which = 0; which < 3; ++which) {
                DWS_TRY(dst[which][0]->ensure((size_t)H * (M / 2) * 8));
                DWS_TRY(dst[which][1]->ensure((size_t)H * (M / 2) * 8));
                DWS_TRY(dst[which][2]->ensure((size_t)H * 3 * 8));
                DWS_TRY(launch_s4_twosided_pow2_part(ck.f(), cK.f(), H, Lt, Nf, Lk, which, s));
                DWS_TRY(launch_rfft_rows(lg, cK.f(), cKf.f(), t->tw.f(), t->twn.f(), H, s));
                DWS_TRY(launch_kf_permute_signed(cKf.f(), dst[which][0]->f(), dst[which][1]->f(), dst[which][2]->f(), H, lg,
                                                 which != 0, s));
            }
            l->log2m = 0;
            l->seg = true;
        } else {
            DWS_TRY(cK.ensure((size_t)H * 2 * L * 4));
            DWS_TRY(l->Kf.ensure((size_t)H * (L + 1) * 8));
            DWS_TRY(launch_s4_twosided(ck.f(), cK.f(), H, L, Lk, Lt, s));
            DWS_TRY(fft.exec(0, 2 * L, H, cK.p, l->Kf.p, s));
            l->log2m = 0;
            l->seg = false;
            stages[l->stage]->rocfft = true;
        }
        return DWS_OK;
    }

    // Can this commit generate the kernels group by group?  Training mode, every block at its kernel's own length (what
    // train_supported() asks for anyway), none on the segmented path, at least one on the fused convolution.  The blocks of
    // stages on rocFFT (odd lengths, more than 16384 samples) keep the per-block chain (build_kernel, rocfft_conv_backward);
    // the fused ones stack.  DWS_S4_KERNELS_PER_BLOCK=1: the per-block chain for every block (same-box A/B).
    static bool stacks(const SLayer* l) {
        int lg = 0;
        return fftconv_supported(l->L, &lg);
    }
    bool stacked_kernels_possible(hipStream_t s) {
        static const bool off = getenv("DWS_S4_KERNELS_PER_BLOCK") != nullptr;
        if (off || !keep_cauchy || getenv("DWS_SASHIMI_ROCFFT")) return false;
        bool any = false;
        for (auto* l : all) {
            if (l->kind != L_BLOCK) continue;
            int64_t Lk = 0;
            if (kernel_len(l, s, &Lk) != DWS_OK || Lk != l->L || stages[l->stage]->seg) return false;
            if (!stacks(l)) continue;
            if (!P("__z." + std::to_string(l->L)) || !P("__omega." + std::to_string(l->L))) return false;
            any = true;
        }
        return any;
    }

    // A block's kernel tensors (or their gradients) <-> its H rows, block i of n, of a group's stack: the C planes of a block
    // go to their plane of the stack
    static void stack_rows(CopyBatch& b, bool unstack, const S4Tensors& blk, const S4Tensors& st, size_t i, int H, int N, int n) {
        const size_t hn = (size_t)H * N, HN = hn * n;
        auto cp = [&](float* pb, float* ps, size_t cnt) { unstack ? b.add(ps, pb, cnt) : b.add(pb, ps, cnt); };
        for (int c = 0; c < 2; ++c) cp(blk.C + c * hn * 2, st.C + (c * HN + i * hn) * 2, hn * 2);
        cp(blk.B, st.B + i * hn * 2, hn * 2);
        cp(blk.P, st.P + i * hn * 2, hn * 2);
        cp(blk.inv_w_real, st.inv_w_real + i * hn, hn);
        cp(blk.w_imag, st.w_imag + i * hn, hn);
        cp(blk.log_dt, st.log_dt + i * H, (size_t)H);
    }

    // parameters -> K_f of every block, one chain per group of same-shaped blocks (s4.py:704-807, 1391-1403)
    int build_kernels_stacked(hipStream_t s) {
        const int N = NS;
        for (auto* g : kgroups) g->layers.clear();      // (the run length may have changed since the last commit)
        for (auto* l : all) {
            if (l->kind != L_BLOCK) continue;
            if (!stacks(l)) { l->grp = -1; continue; }    // rocFFT stage: generated by build_kernel (commit)
            KGroup* g = nullptr;
            for (auto* c : kgroups)
                if (c->H == l->H && c->L == l->L) g = c;
            if (!g) { g = new KGroup(); g->H = l->H; g->L = l->L; kgroups.push_back(g); }
            l->grp = (int)(std::find(kgroups.begin(), kgroups.end(), g) - kgroups.begin());
            l->gidx = (int)g->layers.size();
            g->layers.push_back(l);
        }
        for (auto* g : kgroups) {
            if (g->layers.empty()) continue;
            const int H = g->H, L = g->L, Ht = g->Ht(), n = (int)g->layers.size();
            int lg = 0;
            DWS_CHECK(fftconv_supported(L, &lg), DWS_ERR_STATE, "stacked kernel generation on a stage without the fused convolution");
            g->log2m = lg;
            const size_t HN = (size_t)Ht * N;
            DWS_TRY(g->C.ensure(2 * HN * 8)); DWS_TRY(g->Bp.ensure(HN * 8)); DWS_TRY(g->P.ensure(HN * 8));
            DWS_TRY(g->iwr.ensure(HN * 4)); DWS_TRY(g->wim.ensure(HN * 4)); DWS_TRY(g->logdt.ensure((size_t)Ht * 4));
            S4Chain& c = g->chain;
            c.rows = Ht; c.N = N; c.Lk = L;
            c.par = {g->C.f(), g->Bp.f(), g->P.f(), g->iwr.f(), g->wim.f(), g->logdt.f()};
            c.z = P("__z." + std::to_string(L)); c.omega = P("__omega." + std::to_string(L));
            g->stack.begin();      // the blocks' parameters into the stacked layout (one launch)
            for (int i = 0; i < n; ++i) stack_rows(g->stack, false, kernel_tensors(g->layers[i], false), c.par, i, H, N, n);
            DWS_TRY(g->stack.run(s));
            DWS_TRY(s4_taps_forward(*this, c, products_version(), s));
            DWS_TRY(s4_fused_spectrum(*this, c, L, lg, s));
            take_spectra(c, g->layers.data(), g->layers.size(), lg);
        }
        return DWS_OK;
    }

    int commit(hipStream_t s) override {
        if (B > 0) DWS_TRY(resolve_segmented_stages(s));
        // Pass 1: every fold, fragment pack and row sum of the model as ONE batched preparation (two launches: the folds, then
        // the packs that read them).  Pass 2: what reads the folded weights through its own launches (chain-ordered and
        // split fragments) and the S4 kernel generation.
        prep.begin();
        DWS_TRY(Wi.ensure((size_t)D * Cin * 4));
        DWS_TRY(fold("init_conv.0.conv", Wi.f(), D, Cin, s));
        DWS_TRY(Wt_all.ensure((size_t)pt_total * Eout * 4));
        DWS_TRY(bt_all.ensure((size_t)pt_total * 4));
        stack_fc_t.begin();
        for (auto* l : all) {
            if (l->kind == L_BLOCK) {
                const int H = l->H;
                stack_fc_t.add(P(l->prefix + ".fc_t.weight"), Wt_all.f() + (size_t)l->pt_off * Eout, (size_t)H * Eout);
                stack_fc_t.add(P(l->prefix + ".fc_t.bias"), bt_all.f() + l->pt_off, (size_t)H);
                DWS_TRY(l->W1.ensure((size_t)FF * H * H * 4));
                DWS_TRY(l->W2.ensure((size_t)FF * H * H * 4));
                DWS_TRY(fold(l->prefix + ".ff.ff.0.conv", l->W1.f(), FF * H, H, s));
                DWS_TRY(fold(l->prefix + ".ff.ff.2.conv", l->W2.f(), H, FF * H, s));
                l->mfma = s4_tail_mfma_supported(H, FF) && !getenv("DWS_SASHIMI_GENERIC");
                if (l->mfma) {
                    DWS_TRY(l->Ao.ensure((size_t)2 * H * H * 4));
                    DWS_TRY(l->A1.ensure((size_t)FF * H * H * 4));
                    DWS_TRY(l->A2.ensure((size_t)FF * H * H * 4));
                    DWS_TRY(l->rs1.ensure((size_t)FF * H * 4));
                    prep.pack(P(l->prefix + ".layer.output_linear.0.weight"), l->Ao.f(), 2 * H, H);
                    prep.pack(l->W1.f(), l->A1.f(), FF * H, H);
                    prep.pack(l->W2.f(), l->A2.f(), H, FF * H);
                    prep.row_sum(l->W1.f(), l->rs1.f(), FF * H, H);
                }
                if (cond) {
                    for (int i = 0; i < 2; ++i) {
                        const int sc = d.mel_upsample[i];
                        DevBuf& w = (i == 0) ? l->melW0 : l->melW1;
                        DWS_TRY(w.ensure((size_t)3 * 2 * sc * 4));
                        DWS_TRY(fold(l->prefix + ".upsample_conv2d." + std::to_string(i), w.f(), 1, 3 * 2 * sc, s));
                    }
                    DWS_TRY(l->melWc.ensure((size_t)H * MB * 4));
                    DWS_TRY(fold(l->prefix + ".mel_conv.conv", l->melWc.f(), H, MB, s));
                }
            } else {
                const int O = (l->kind == L_DOWN) ? l->Hout : l->Hout * l->p;
                const int K = (l->kind == L_DOWN) ? l->H * l->p : l->H;
                DWS_TRY(l->Wp.ensure((size_t)O * K * 4));
                DWS_TRY(fold(l->prefix + ".linear.conv", l->Wp.f(), O, K, s));
                l->mfma = pw_mfma_supported(l->kind == L_DOWN ? 0 : 1, K, O, l->p) && !getenv("DWS_SASHIMI_GENERIC");
                // shapes the fused pooling kernel does not cover (e.g. 128 -> 64 channels of unet_d32) still run on MFMA:
                // explicit rearrangement + the position-tile GEMM of the training path
                l->mfma2 = !l->mfma && tapconv_mfma_supported(O, K, 0, 1) && !getenv("DWS_SASHIMI_GENERIC");
                if (l->mfma || l->mfma2) {
                    DWS_TRY(l->Ap.ensure((size_t)O * K * 4));
                    prep.pack(l->Wp.f(), l->Ap.f(), O, K);
                }
            }
        }
        DWS_TRY(Wf.ensure((size_t)D * D * 4));
        DWS_TRY(fold("final_conv.0.conv", Wf.f(), D, D, s));
        if (wn_final_mfma_supported(D)) {
            DWS_TRY(Af.ensure((size_t)D * D * 4));
            prep.pack(Wf.f(), Af.f(), D, D);
        }
        DWS_TRY(prep.run(s));
        kernels_stacked = stacked_kernels_possible(s);
        for (auto* l : all) {
            if (l->kind == L_BLOCK) {
                const int H = l->H;
                if (l->mfma) {
                    // (Wo, W1, W2) of the block's tail, in the order the packed copies below are made
                    struct { const float* w; int rows, cols; const float* bias; int bias_len; } tail[3] = {
                        {P(l->prefix + ".layer.output_linear.0.weight"), 2 * H, H, P(l->prefix + ".layer.output_linear.0.bias"), 2 * H},
                        {l->W1.f(), FF * H, H, P(l->prefix + ".ff.ff.0.conv.bias"), FF * H},
                        {l->W2.f(), H, FF * H, P(l->prefix + ".ff.ff.2.conv.bias"), H}};
                    if (s4_tail_chain_supported(H, FF)) {   // chain-ordered columns for the register-chained tail kernel
                        DWS_TRY(chain_tmp.ensure((size_t)FF * H * H * 4));
                        DevBuf* dst[3] = {&l->Ao_c, &l->A1_c, &l->A2_c};
                        for (int i = 0; i < 3; ++i) {
                            DWS_TRY(dst[i]->ensure((size_t)tail[i].rows * tail[i].cols * 4));
                            DWS_TRY(launch_chain_permute_cols(tail[i].w, chain_tmp.f(), tail[i].rows, tail[i].cols, s));
                            DWS_TRY(launch_pack_a_frag(chain_tmp.f(), dst[i]->f(), tail[i].rows, tail[i].cols, s));
                        }
                    }
                    const int split = f16x3 ? WN_SPLIT_F16X3 : WN_SPLIT_BF16X6;
                    const size_t wb = 2 * (size_t)wn_split_terms(split);            // bytes per packed weight
                    float* sc = nullptr;
                    if (f16x3) {     // (H >= 256: the LDS-tile kernel's split instances scale the fp32 fragments in registers)
                        DWS_TRY(l->wscale_c6.ensure(3 * 4));
                        sc = l->wscale_c6.f();
                        for (int i = 0; i < 3; ++i)
                            DWS_TRY(launch_weight_scale(tail[i].w, (size_t)tail[i].rows * tail[i].cols, tail[i].bias, tail[i].bias_len,
                                                        nullptr, 0, sc + i, s));
                    }
                    if (split_tails() && s4_tail_chain6_supported(H, FF)) {
                        DWS_TRY(chain_tmp.ensure((size_t)FF * H * H * 4));
                        DevBuf* dst[3] = {&l->Ao_c6, &l->A1_c6, &l->A2_c6};
                        for (int i = 0; i < 3; ++i) {
                            DWS_TRY(dst[i]->ensure((size_t)tail[i].rows * tail[i].cols * wb));
                            DWS_TRY(launch_chain16_permute_cols(tail[i].w, chain_tmp.f(), tail[i].rows, tail[i].cols, s));
                            DWS_TRY(launch_pack_a_bx6(chain_tmp.f(), dst[i]->p, tail[i].rows, tail[i].cols, split, sc ? sc + i : nullptr, s));
                        }
                    } else if (split_tails() && s4_tail_wide6_supported(H, FF)) {   // one blob [Wo | W1 | W2], k-block-major fragments
                        DWS_TRY(chain_tmp.ensure((size_t)FF * H * H * 4));
                        DWS_TRY(l->Ao_c6.ensure((size_t)(2 + 2 * FF) * H * H * wb));
                        l->A1_c6.release(); l->A2_c6.release();
                        char* blob = static_cast<char*>(l->Ao_c6.p);
                        for (int i = 0; i < 3; ++i) {
                            DWS_TRY(launch_chain16_permute_cols(tail[i].w, chain_tmp.f(), tail[i].rows, tail[i].cols, s));
                            DWS_TRY(launch_pack_a_bx6_kmajor(chain_tmp.f(), blob, tail[i].rows, tail[i].cols, split, sc ? sc + i : nullptr, s));
                            blob += (size_t)tail[i].rows * tail[i].cols * wb;
                        }
                    } else {
                        l->Ao_c6.release(); l->A1_c6.release(); l->A2_c6.release();
                    }
                }
                if (!kernels_stacked || !stacks(l)) { l->grp = -1; DWS_TRY(build_kernel(l, s)); }
            }
        }
        if (kernels_stacked) DWS_TRY(build_kernels_stacked(s));
        DWS_TRY(stack_fc_t.run(s));
        if (!freq_ready) {   // depends on the embedding width only: uploaded (and waited for) once, not on every commit --
                             // a training step commits once, and a blocking wait there keeps the host from running ahead of the GPU
            const int half = Ein / 2;
            std::vector<float> f(half);
            const float e = (float)(-(std::log(10000.0) / (half - 1)));
            for (int i = 0; i < half; ++i) f[i] = (float)std::exp((double)((float)i * e));
            DWS_TRY(freq.ensure((size_t)half * 4));
            DWS_HIP(hipMemcpyAsync(freq.p, f.data(), (size_t)half * 4, hipMemcpyHostToDevice, s));
            DWS_HIP(hipStreamSynchronize(s));
            freq_ready = true;
        }
        dirty = false;
        ++commit_version;
        melBm = 0;
        return DWS_OK;
    }

    int prepare(int64_t nB, int64_t nL) override {
        DWS_CHECK(nB > 0 && nL > 0, DWS_ERR_INVALID, "prepare: B=%lld L=%lld", (long long)nB, (long long)nL);
        int span = 1;
        for (int p : pool) span *= p;
        DWS_CHECK(nL % span == 0, DWS_ERR_INVALID, "sashimi: input length %lld is not divisible by the pooling factors (%d)",
                  (long long)nL, span);
        if (nB != B || nL != L) { drop_graph(); melBm = 0; trained_fwd = false; lengths_host.clear(); frames_host.clear(); }
        if (nL != L) {
            // variable-length run (s4.py:1387): every stage length scales with the input; the S4 kernels keep their
            // own length (the `L` buffers) and contribute min(run, l_max) taps per direction
            for (auto* l : all) {
                l->L = (int)((int64_t)l->L0 * nL / d.L);
                l->Lout = (int)((int64_t)l->Lout0 * nL / d.L);
            }
            for (auto* st : stages) {
                st->L = (int)((int64_t)st->L0 * nL / d.L);
                st->rocfft = false; st->seg = false; st->force_rocfft = false;
            }
            dirty = true;   // K_f depends on the run length (two-sided assembly, transform size)
        }
        B = nB; L = nL;
        for (auto* st : stages) {
            const size_t rows = (size_t)B * st->H, Ls = st->L;
            int lg = 0;
            const bool no_fused = !fftconv_supported((int)Ls, &lg) || getenv("DWS_SASHIMI_ROCFFT");
            // beyond the largest LDS transform: segmented fused path when the kernels (at most the configured stage
            // length of taps per direction, s4.py:1387) fit one segment
            st->seg = no_fused && !st->force_rocfft && !getenv("DWS_SASHIMI_ROCFFT") &&
                      fftconv_seg_supported((int)Ls, std::min((int)Ls, st->L0));
            const bool need_rocfft = no_fused && !st->seg;
            if (need_rocfft) {
                B = nB;
                DWS_TRY(ensure_rocfft_stage(st));
            } else {
                DWS_TRY(st->y.ensure(rows * Ls * 4));
            }
            DWS_TRY(st->g.ensure(rows * Ls * 4));
            DWS_TRY(st->x1.ensure(rows * Ls * 4));
            DWS_TRY(st->n2.ensure(rows * Ls * 4));
            DWS_TRY(st->ffu.ensure(rows * FF * Ls * 4));
        }
        size_t pool_max = 4;
        for (auto* l : all) {
            const size_t n = (l->kind == L_BLOCK) ? (size_t)B * l->H * l->L : (size_t)B * l->Hout * l->Lout;
            DWS_TRY(l->out.ensure(n * 4));
            if (l->kind != L_BLOCK) pool_max = std::max(pool_max, std::max((size_t)B * l->H * l->L, n) * 4);
        }
        DWS_TRY(pool_scr.ensure(pool_max));
        DWS_TRY(x_init.ensure((size_t)B * D * L * 4));
        DWS_TRY(nfin.ensure((size_t)B * D * L * 4));
        DWS_TRY(emb.ensure((size_t)B * Ein * 4));
        DWS_TRY(h1.ensure((size_t)B * Emid * 4));
        DWS_TRY(h2.ensure((size_t)B * Eout * 4));
        DWS_TRY(part_t.ensure((size_t)B * pt_total * 4));
        if (!zero_row.p) {     // (allocated here, never inside a stream capture)
            DWS_TRY(zero_row.ensure((size_t)D * 4));
            DWS_HIP(hipMemset(zero_row.p, 0, (size_t)D * 4));
        }
        return DWS_OK;
    }

    int set_condition(const float* mel, int64_t Bm, int64_t Tmel, hipStream_t s) override {
        if (mel == nullptr) { melBm = 0; return DWS_OK; }
        DWS_CHECK(cond, DWS_ERR_INVALID, "set_condition on an unconditional model (`sashimi.py:161`)");
        DWS_CHECK(B > 0, DWS_ERR_STATE, "set_condition before prepare");
        DWS_CHECK(Bm == 1 || Bm == B, DWS_ERR_INVALID, "mel batch %lld must be 1 or B=%lld", (long long)Bm, (long long)B);
        if (ragged()) DWS_TRY(check_ragged_mel(frames_host.data(), Bm, Tmel));
        if (dirty) DWS_TRY(commit(s));
        const int T0 = mel_upsampled_len((int)Tmel, d.mel_upsample[0]), T1 = mel_upsampled_len(T0, d.mel_upsample[1]);
        // pooled stages take the FIRST L_stage upsampled frames (sashimi.py:170-172): a truncation
        for (auto* l : all)
            DWS_CHECK(l->kind != L_BLOCK || T1 >= l->L, DWS_ERR_INVALID, "upsampled mel length %d < L=%d (`sashimi.py:169`)", T1, l->L);
        // (the kept copy first: with per-clip lengths on, the terms are evaluated from it, here and again by set_lengths)
        if (mel != mel_in.p) {
            DWS_TRY(mel_in.ensure((size_t)Bm * MB * Tmel * 4));
            DWS_HIP(hipMemcpyAsync(mel_in.p, mel, (size_t)Bm * MB * Tmel * 4, hipMemcpyDeviceToDevice, s));
        }
        mel_T = (int)Tmel;
        melBm = 0;   // (invalid while a launch below can still fail)
        DWS_TRY(eval_condition(mel, Bm, s));
        melBm = Bm;
        return DWS_OK;
    }

    // the conditioner terms of every block from `mel` [Bm][MB][mel_T].  Per-clip lengths on: clip b's mel frames >= frames_b
    // and the first upsampler's output at positions >= s0 frames_b count as zero, as in the WaveNet model -- the second
    // upsampler would otherwise read leaky_relu(bias + ..) != 0 there for the last s1 / 2 samples of the clip.  The 1x1 is
    // pointwise and a pooled stage takes the first L_stage columns: clip b's stage reads columns < len_b / div of the
    // upsampling of its own frames.
    int eval_condition(const float* mel, int64_t Bm, hipStream_t s) {
        const int s0 = d.mel_upsample[0], s1 = d.mel_upsample[1];
        const int T0 = mel_upsampled_len(mel_T, s0), T1 = mel_upsampled_len(T0, s1);
        const int32_t* fr = ragged() ? frames_ptr() : nullptr;
        DevBuf& u0 = mel_u0;
        DevBuf& u1 = mel_u1;
        DWS_TRY(u0.ensure((size_t)Bm * MB * T0 * 4));
        DWS_TRY(u1.ensure((size_t)Bm * MB * T1 * 4));
        for (auto* l : all) {
            if (l->kind != L_BLOCK) continue;
            DWS_TRY(l->melc.ensure((size_t)Bm * l->H * l->L * 4));
            DWS_TRY(launch_mel_upsample(mel, l->melW0.f(), P(l->prefix + ".upsample_conv2d.0.bias"), u0.f(), (int)Bm, MB,
                                        mel_T, T0, s0, 0.4f, s, fr, 1));
            DWS_TRY(launch_mel_upsample(u0.f(), l->melW1.f(), P(l->prefix + ".upsample_conv2d.1.bias"), u1.f(), (int)Bm, MB,
                                        T0, T1, s1, 0.4f, s, fr, s0));
            DWS_TRY(launch_conv1x1_trunc(u1.f(), l->melWc.f(), P(l->prefix + ".mel_conv.conv.bias"), l->melc.f(), (int)Bm,
                                         MB, l->H, T1, l->L, s));
        }
        return DWS_OK;
    }

    // dws_model::set_lengths (api.hip): every length a multiple of the pooling factors' product -- the clip's length at a
    // pooled stage is lengths[b] / (the factors above it); frames of hop samples; the terms again from the kept mel
    int pool_span() const {
        int span = 1;
        for (int p : pool) span *= p;
        return span;
    }
    int ragged_rule(int64_t* hop, int64_t* multiple) const override {
        *hop = cond ? (int64_t)d.mel_upsample[0] * d.mel_upsample[1] : 0;
        *multiple = pool_span();
        return DWS_OK;
    }
    int64_t cond_batch() const override { return melBm; }
    int64_t cond_frames() const override { return mel_T; }
    int reeval_condition(hipStream_t s) override {
        const int64_t Bm = melBm;
        melBm = 0;
        DWS_TRY(eval_condition(mel_in.f(), Bm, s));
        melBm = Bm;
        return DWS_OK;
    }
    // forward(): the length table and a stage's divisor for the S4 convolutions (null while lengths are off)
    const int32_t* conv_lengths() const { return ragged() ? lengths_ptr() : nullptr; }
    int stage_div(const SLayer* l) const { return (int)(L / l->L); }

    // The tail of `l` can also produce the S4 input of the block that runs next (LN1 + step embedding fused into its
    // epilogue) when that block sits on the same stage and both run the fused paths.
    bool feeds_next(const SLayer* l, const SLayer* next) const {
        return next && l->kind == L_BLOCK && next->kind == L_BLOCK && next->stage == l->stage && l->mfma &&
               (next->log2m > 0 || next->seg) && !getenv("DWS_SASHIMI_NO_LN_FUSION");
    }

    // A pooling layer on the fused MFMA kernel whose whole output column sits in one workgroup can emit the LN1 + step
    // embedding of the block that follows it (the first block of the new stage), when that block reads the stage's y buffer.
    bool pool_feeds(const SLayer* l, const SLayer* next) const {
        if (!next || l->kind == L_BLOCK || next->kind != L_BLOCK || !l->mfma || getenv("DWS_SASHIMI_NO_LN_FUSION")) return false;
        const int M = (l->kind == L_DOWN) ? l->Hout : l->Hout * l->p;
        return pw_mfma_ln_supported(M) && (next->log2m > 0 || next->seg);
    }

    // DiffWaveBlock.forward (sashimi.py:143-184).  y_ready: the previous block's tail already wrote this block's S4 input
    // into the stage's y buffer; next: the block whose S4 input this block's tail should write (or null).
    // LayerNorm a tail kernel applies to ITS OUTPUT on the way out (the tile is still in LDS / registers): the next block's
    // LN1 + step-embedding projection into the stage's y buffer, or -- after the last block -- the network's final norm
    // (`sashimi.py:309`) into nfin
    struct OutLN {
        const float *m = nullptr, *s = nullptr, *e = nullptr;
        int e_stride = 0, e_tstride = 0;
        const int* e_step = nullptr;
        float* y = nullptr;
    };
    OutLN next_ln(Stage* st, const SLayer* next) {
        OutLN o;
        o.m = P(next->prefix + ".norm1.m"); o.s = P(next->prefix + ".norm1.s");
        o.e = pt_base() + next->pt_off; o.e_stride = pt_bstride(); o.e_step = step_idx; o.e_tstride = pt_tstride();
        o.y = st->y.f();
        return o;
    }
    DevBuf zero_row;     // [max H] zeros: the "step embedding" of the final norm
    bool final_ln_fused = false;   // set by forward(): the last block's tail wrote norm(x) into nfin

    // a segmented block's tables, three spectra and shape (u, g and the mode's own fields are the caller's)
    FftConvSegArgs seg_args(const SLayer* l) {
        FftTables* t = tables[FFTCONV_SEG_LOG2M];
        FftConvSegArgs fa{};
        fa.D = P(l->prefix + ".layer.D");
        fa.tw = (const c2*)t->tw.p; fa.twp = (const c2*)t->twp.p;
        fa.kfa[0] = (const c2*)l->own.kfa.p; fa.kfb[0] = (const c2*)l->own.kfb.p; fa.kfs[0] = (const c2*)l->own.kfs.p;
        fa.kfa[1] = (const c2*)l->kfa_c.p; fa.kfb[1] = (const c2*)l->kfb_c.p; fa.kfs[1] = (const c2*)l->kfs_c.p;
        fa.kfa[2] = (const c2*)l->kfa_a.p; fa.kfb[2] = (const c2*)l->kfb_a.p; fa.kfs[2] = (const c2*)l->kfs_a.p;
        fa.B = (int)B; fa.H = l->H; fa.L = l->L;
        return fa;
    }

    int run_block(SLayer* l, const float* x, const float* addend, bool y_ready, const OutLN* next, hipStream_t s) {
        Stage* st = stages[l->stage];
        const int H = l->H, Ls = l->L, nB = (int)B;
        const std::string& p = l->prefix;
        if (l->log2m > 0) {
            if (!y_ready)
                DWS_TRY(launch_ln(x, P(p + ".norm1.m"), P(p + ".norm1.s"), pt_base() + l->pt_off, pt_bstride(), st->y.f(), nB,
                                  H, Ls, (size_t)Ls, s, step_idx, pt_tstride()));
            FftTables* t = tables[l->log2m];
            FftConvArgs fa{};
            fa.u = st->y.f(); fa.g = st->g.f(); fa.D = P(p + ".layer.D");
            fa.tw = (const c2*)t->tw.p; fa.twp = (const c2*)t->twp.p;
            fa.kfa = (const c2*)l->kfa_v; fa.kfb = (const c2*)l->kfb_v; fa.kfs = (const c2*)l->kfs_v;
            fa.B = nB; fa.H = H; fa.L = Ls;
            fa.lengths = conv_lengths(); fa.len_div = stage_div(l);
            DWS_TRY(launch_fftconv(l->log2m, fa, s));
            return run_tail(l, st, x, addend, next, s);
        }
        if (l->seg) {
            if (!y_ready)
                DWS_TRY(launch_ln(x, P(p + ".norm1.m"), P(p + ".norm1.s"), pt_base() + l->pt_off, pt_bstride(), st->y.f(), nB,
                                  H, Ls, (size_t)Ls, s, step_idx, pt_tstride()));
            FftConvSegArgs fa = seg_args(l);
            fa.u = st->y.f(); fa.g = st->g.f();
            // (DWS_RAGGED_SEG_NO_SKIP=1: workgroups of wholly padded output segments run too -- the same-box A/B)
            static const bool skip_pad = getenv("DWS_RAGGED_SEG_NO_SKIP") == nullptr;
            fa.lengths = conv_lengths(); fa.len_div = stage_div(l); fa.skip_pad = (fa.lengths && skip_pad) ? 1 : 0;
            DWS_TRY(launch_fftconv_seg(fa, s));
            return run_tail(l, st, x, addend, next, s);
        }
        DWS_TRY(launch_ln(x, P(p + ".norm1.m"), P(p + ".norm1.s"), pt_base() + l->pt_off, pt_bstride(), st->U.f(), nB, H, Ls,
                          (size_t)2 * Ls, s, step_idx, pt_tstride()));
        // ragged batches: the transform's input rows sealed behind each clip's own end (stores: whatever the LayerNorm wrote there)
        if (ragged()) DWS_TRY(launch_mask_tail_rows(st->U.f(), lengths_ptr(), nB, H, Ls, (size_t)2 * Ls, stage_div(l), s));
        {
            ProfileScope ps("rocfft_r2c", s);
            DWS_TRY(fft.exec(0, 2 * Ls, nB * H, st->U.p, st->Uf.p, s));
        }
        DWS_TRY(launch_spec_mul(st->Uf.f(), l->Kf.f(), nB, H, Ls + 1, s));
        {
            ProfileScope ps("rocfft_c2r", s);
            DWS_TRY(fft.exec(1, 2 * Ls, nB * H, st->Uf.p, st->Y.p, s));
        }
        DWS_TRY(launch_s4_post(st->Y.f(), st->U.f(), P(p + ".layer.D"), st->g.f(), nB, H, Ls, s));
        return run_tail(l, st, x, addend, next, s);
    }

    // everything of the block after the S4 convolution (sashimi.py:177-184, s4.py:1435)
    int n_tail_split = 0, n_tail_f32 = 0;     // block-tail launches of the last forward, by arithmetic
    int run_tail(SLayer* l, Stage* st, const float* x, const float* addend, const OutLN* next, hipStream_t s) {
        const int H = l->H, Ls = l->L, nB = (int)B;
        const std::string& p = l->prefix;
        if (l->mfma) {
            S4TailArgs t{};
            t.g = st->g.f(); t.x = x; t.Ao = l->Ao.f(); t.bo = P(p + ".layer.output_linear.0.bias");
            t.mel = melBm ? l->melc.f() : nullptr; t.mel_bstride = melBm > 1 ? 1 : 0;
            t.ln_m = P(p + ".norm2.m"); t.ln_s = P(p + ".norm2.s");
            t.A1 = l->A1.f(); t.b1 = P(p + ".ff.ff.0.conv.bias"); t.rs1 = l->rs1.f();
            t.A2 = l->A2.f(); t.b2 = P(p + ".ff.ff.2.conv.bias");
            t.addend = addend; t.out = l->out.f(); t.B = nB; t.L = Ls;
            t.Ao_c = l->Ao_c.f(); t.A1_c = l->A1_c.f(); t.A2_c = l->A2_c.f();
            if (split_tails()) {
                t.split_on = 1;
                t.Ao_c6 = l->Ao_c6.p; t.A1_c6 = l->A1_c6.p; t.A2_c6 = l->A2_c6.p;
                t.split_c6 = f16x3 ? WN_SPLIT_F16X3 : WN_SPLIT_BF16X6;
                t.wscale_c6 = f16x3 ? l->wscale_c6.f() : nullptr;
            }
            if (next) {     // next block: feeds_next(l, next) holds, the stage's y buffer is free once this block's convolution ran
                t.ynext = next->y;
                t.n1_m = next->m; t.n1_s = next->s;
                t.e_next = next->e; t.e_stride = next->e_stride;
                t.e_step = next->e_step; t.e_tstride = next->e_tstride;
            }
            bool ran_split = false;
            const int rc = launch_s4_tail_mfma(H, t, s, &ran_split);
            ++(ran_split ? n_tail_split : n_tail_f32);
            return rc;
        }
        ++n_tail_f32;          // plain-FMA block (channel counts the MFMA tiling does not cover): no split instance
        DWS_TRY(launch_pw_glu_res(st->g.f(), P(p + ".layer.output_linear.0.weight"), P(p + ".layer.output_linear.0.bias"),
                                  x, melBm ? l->melc.f() : nullptr, melBm > 1 ? 1 : 0, st->x1.f(), nB, H, Ls, s));
        DWS_TRY(launch_ln(st->x1.f(), P(p + ".norm2.m"), P(p + ".norm2.s"), nullptr, 0, st->n2.f(), nB, H, Ls, (size_t)Ls, s));
        DWS_TRY(launch_pw_conv(st->n2.f(), l->W1.f(), P(p + ".ff.ff.0.conv.bias"), st->ffu.f(), nB, H, FF * H, Ls, 1, s));
        DWS_TRY(launch_pw_res(st->ffu.f(), l->W2.f(), P(p + ".ff.ff.2.conv.bias"), st->x1.f(), addend, l->out.f(), nB,
                              FF * H, H, Ls, s));
        return DWS_OK;
    }

    int run_layer(SLayer* l, const float* x, const float* addend, hipStream_t s, bool y_ready = false, const OutLN* next = nullptr) {
        if (l->kind == L_BLOCK) return run_block(l, x, addend, y_ready, next, s);
        if (l->mfma) {
            PwMfmaArgs a{};
            a.in = x; a.A = l->Ap.f(); a.bias = P(l->prefix + ".linear.conv.bias"); a.out = l->out.f();
            a.B = (int)B; a.p = l->p;
            if (l->kind == L_DOWN) { a.K = l->H * l->p; a.M = l->Hout; a.L = l->Lout; a.addend = nullptr; }
            else { a.K = l->H; a.M = l->Hout * l->p; a.L = l->L; a.addend = addend; }
            if (next) {     // pool_feeds(l, next block) holds: the first block of the new stage gets its S4 input from here
                a.ln_y = next->y; a.ln_m = next->m; a.ln_s = next->s;
                a.ln_e = next->e; a.ln_e_stride = next->e_stride; a.ln_step = next->e_step; a.ln_e_tstride = next->e_tstride;
            }
            return launch_pw_mfma(l->kind == L_DOWN ? 0 : 1, a, s);
        }
        if (l->mfma2) {
            const float* bias = P(l->prefix + ".linear.conv.bias");
            if (l->kind == L_DOWN) {
                DWS_TRY(launch_pool_rearrange(x, pool_scr.f(), nullptr, 0, 0, (int)B, l->H, l->p, l->Lout, s));
                return gemm(l->Ap.f(), l->Hout, l->H * l->p, pool_scr.f(), l->out.f(), l->Lout, 2, bias, nullptr, nullptr, nullptr,
                            nullptr, s);
            }
            DWS_TRY(gemm(l->Ap.f(), l->Hout * l->p, l->H, x, pool_scr.f(), l->L, 2, bias, nullptr, nullptr, nullptr, nullptr, s));
            return launch_pool_rearrange(pool_scr.f(), l->out.f(), addend, 1, 0, (int)B, l->Hout, l->p, l->L, s);
        }
        if (l->kind == L_DOWN)
            return launch_pw_downpool(x, l->Wp.f(), P(l->prefix + ".linear.conv.bias"), l->out.f(), (int)B, l->H, l->p,
                                      l->Hout, l->Lout, s);
        return launch_pw_uppool(x, l->Wp.f(), P(l->prefix + ".linear.conv.bias"), addend, l->out.f(), (int)B, l->H, l->p,
                                l->Hout, l->L, s);
    }

    int final_stage(const float* xin, float* out, float* tap, hipStream_t s, bool ln_done = false) {
        if (!ln_done) DWS_TRY(launch_ln(xin, P("norm.m"), P("norm.s"), nullptr, 0, nfin.f(), (int)B, D, (int)L, (size_t)L, s));
        WnFinalArgs f{};
        f.skip = nfin.f(); f.Af = Af.f(); f.Wf = Wf.f(); f.bf = P("final_conv.0.conv.bias");
        f.Wz = P("final_conv.2.conv.weight"); f.bz = P("final_conv.2.conv.bias");
        f.out = out; f.tap = tap; f.scale = 1.f;
        f.B = (int)B; f.L = (int)L; f.Cout = Cout;
        return launch_wn_final(D, f, s);
    }

    const float* last_x = nullptr;

    // everything of the forward that depends on the diffusion step only (`sashimi.py:287-289,151`; a1, a2 of SURVEY 8):
    // embedding -> MLP -> every block's fc_t as one stacked GEMV, for `rows` step values (one wave per output row: a row's
    // result does not depend on how many rows the launch carries)
    // Class conditioning (n_classes > 0): the label row joins h2 = the MLP's output before the fc_t rows are formed --
    // `lab` [nlab] the labels of the clips (null: the null class for every row), in place.
    int embed_rows(const float* steps, int rows, float* emb_, float* h1_, float* h2_, float* pt, hipStream_t s,
                   const int32_t* lab = nullptr, int nlab = 1) {
        DWS_TRY(mlp_rows(steps, rows, emb_, h1_, h2_, s));
        return label_fc_rows(h2_, rows, 1, h2_, lab, nlab, pt, s);
    }

    // embedding -> the two swish layers, for `rows` step values
    int mlp_rows(const float* steps, int rows, float* emb_, float* h1_, float* h2_, hipStream_t s) {
        DWS_TRY(launch_step_embed(steps, freq.f(), emb_, rows, Ein / 2, s));
        DWS_TRY(launch_linear_rows(emb_, P("fc_t1.weight"), P("fc_t1.bias"), h1_, rows, Ein, Emid, 1, s));
        return launch_linear_rows(h1_, P("fc_t2.weight"), P("fc_t2.bias"), h2_, rows, Emid, Eout, 1, s);
    }

    // e[r] = h2[r / rep] + table[label of clip r % nlab] into e_ (rows * rep rows; e_ == h2_ with rep == 1: in place; without
    // classes e is h2 itself), then every block's fc_t row of every e row
    int label_fc_rows(const float* h2_, int rows, int rep, float* e_, const int32_t* lab, int nlab, float* pt, hipStream_t s) {
        if (n_classes == 0) return launch_linear_rows(h2_, Wt_all.f(), bt_all.f(), pt, rows, Eout, pt_total, 0, s);
        DWS_TRY(launch_label_add(h2_, P(label_param), lab, nlab, n_classes, e_, rows * rep, rep, Eout, s));
        return launch_linear_rows(e_, Wt_all.f(), bt_all.f(), pt, rows * rep, Eout, pt_total, 0, s);
    }

    // Step table of a sampler run (sampler.hip): every clip of a reverse step is at the same t (`generate.py:50`), so the
    // projections are evaluated once for t = 0..T-1 -- tab_pt [T][pt_total] -- and the captured step's LayerNorm / tail
    // kernels read row *step_idx: no embedding kernels in a replay.
    // With labels installed (dws_model_set_labels) the rows are per (step, clip): tab_pt [T][B][pt_total], built from
    // e[t, b] = h2[t] + table[y_b] (tab_e) by the same row kernel; the kernels get the matching batch / step strides.  A new
    // assignment rewrites the rows in place: the buffers, and so the captured graphs, stay.
    DevBuf de_raw;                        // class conditioning: d e [B][Eout] before the swish factor
    DevBuf tab_steps, tab_emb, tab_h1, tab_h2, tab_pt, tab_e;
    int tab_rep = 1;                      // rows per step: B with labels installed, else 1
    bool tab_labelled = false;            // the rows carry an installed assignment (B = 1: one row per step as without one)
    uint64_t tab_labels_version = 0;
    int tab_T = 0;
    uint64_t tab_version = ~0ull;
    StepKey tab_key;   // the step VALUES the table holds (same T with other steps must not reuse it)
    const float* pt_base() const { return step_idx ? tab_pt.f() : part_t.f(); }
    int pt_bstride() const { return (step_idx && tab_rep == 1) ? 0 : pt_total; }
    int pt_tstride() const { return tab_rep * pt_total; }
    int build_step_table(int T, const float* steps, hipStream_t s) override {
        if (dirty) DWS_TRY(commit(s));
        const bool per_clip = labelled();
        const int rep = per_clip ? (int)B : 1;
        const int32_t* lab = per_clip ? labels_ptr() : nullptr;
        if (tab_version == commit_version && tab_key.same(T, steps) && tab_rep == rep && tab_labelled == per_clip) {
            if (n_classes == 0 || tab_labels_version == labels_version) return DWS_OK;
            // a new label assignment at the same (B, S): the rows are rewritten in place, the graphs stay
            // (no assignment installed: the rows hold the null class already)
            if (per_clip) DWS_TRY(label_fc_rows(tab_h2.f(), T, rep, tab_e.f(), lab, (int)B, tab_pt.f(), s));
            tab_labels_version = labels_version;
            return DWS_OK;
        }
        drop_graph();   // a captured step holds pointers into the old table
        DWS_CHECK(T > 0 && (size_t)T * rep * ((size_t)pt_total + Eout) * 4 <= ((size_t)4 << 30), DWS_ERR_UNSUPPORTED,
                  "sampler step table: T=%d x %d rows per step exceeds 4 GB", T, rep);
        tab_version = ~0ull;   // invalid until the rebuild has finished
        DWS_TRY(tab_steps.ensure((size_t)T * 4));
        DWS_TRY(tab_emb.ensure((size_t)T * Ein * 4));
        DWS_TRY(tab_h1.ensure((size_t)T * Emid * 4));
        DWS_TRY(tab_h2.ensure((size_t)T * Eout * 4));
        DWS_TRY(tab_pt.ensure((size_t)T * rep * pt_total * 4));
        DWS_TRY(tab_key.upload(T, steps, tab_steps.f(), s));   // steps[t] = float(t) when null, as `generate.py:50` feeds them
        if (n_classes > 0) DWS_TRY(tab_e.ensure((size_t)T * rep * Eout * 4));   // tab_h2 stays label-free for the rewrites
        // the MLP once per step, the label rows and the fc_t rows per step or, with labels, per (step, clip)
        DWS_TRY(mlp_rows(tab_steps.f(), T, tab_emb.f(), tab_h1.f(), tab_h2.f(), s));
        DWS_TRY(label_fc_rows(tab_h2.f(), T, rep, tab_e.f(), lab, (int)B, tab_pt.f(), s));
        tab_labelled = per_clip;
        tab_rep = rep;
        tab_labels_version = labels_version;
        tab_T = T;
        tab_version = commit_version;
        ++step_table_gen;
        return DWS_OK;
    }

    // Sashimi.forward (sashimi.py:277-313)
    int forward(const float* audio, const float* steps, float* out, hipStream_t s) override {
        DWS_CHECK(B > 0, DWS_ERR_STATE, "forward before prepare");
        trained_fwd = false;   // this forward (eval call, or a step of the sampler) overwrites the activations a pending backward needs
        if (dirty) DWS_TRY(commit(s));
        DWS_CHECK(!step_idx || (tab_T > 0 && tab_version == commit_version && (tab_rep == 1 || tab_rep == (int)B)), DWS_ERR_STATE,
                  "step-table forward without a current table");
        DWS_CHECK(step_idx || steps, DWS_ERR_INVALID, "forward: steps == null");
        n_tail_split = n_tail_f32 = 0;     // tap "split_launches": which arithmetic THIS forward's tails ran
        if (!step_idx)
            DWS_TRY(embed_rows(steps, (int)B, emb.f(), h1.f(), h2.f(), part_t.f(), s, n_classes > 0 ? labels_ptr() : nullptr, (int)B));
        std::vector<const float*> stack;  // LIFO skip stack (sashimi.py:293-307)
        const float* x = x_init.f();
        // execution order; a block whose successor is a fused block of the same stage also writes that block's S4 input
        std::vector<SLayer*> order(d_layers);
        order.insert(order.end(), c_layers.begin(), c_layers.end());
        order.insert(order.end(), u_layers.begin(), u_layers.end());
        const bool ln_fusion = getenv("DWS_SASHIMI_NO_LN_FUSION") == nullptr;   // (read per call: tests switch it inside one process)
        // the first block's LN1 + step embedding comes out of the init-conv pass when that block runs a fused convolution
        // (which reads the stage's y buffer); otherwise the block's own LayerNorm launch does it
        SLayer* first = order.empty() ? nullptr : order[0];
        bool y_ready = false;
        if (ln_fusion && first && first->kind == L_BLOCK && (first->log2m > 0 || first->seg) && init_conv_ln_supported(Cin)) {
            DWS_TRY(launch_init_conv_ln(audio, Wi.f(), P("init_conv.0.conv.bias"), P(first->prefix + ".norm1.m"),
                                        P(first->prefix + ".norm1.s"), pt_base() + first->pt_off, pt_bstride(), step_idx, pt_tstride(),
                                        x_init.f(), stages[first->stage]->y.f(), (int)B, Cin, D, (int)L, s));
            y_ready = true;
        } else {
            DWS_TRY(launch_init_conv(audio, Wi.f(), P("init_conv.0.conv.bias"), x_init.f(), (int)B, Cin, D, (int)L, s));
        }
        // the network's final norm (`sashimi.py:309`) comes out of the LAST block's tail the same way (a zero "embedding")
        SLayer* last = order.empty() ? nullptr : order.back();
        final_ln_fused = ln_fusion && last && last->kind == L_BLOCK && last->mfma && last->H == D && zero_row.p;
        size_t oi = 0;
        auto run = [&](SLayer* l, const float* add) -> int {
            SLayer* nxt = oi + 1 < order.size() ? order[oi + 1] : nullptr;
            SLayer* nx = (nxt && (feeds_next(l, nxt) || pool_feeds(l, nxt))) ? nxt : nullptr;
            OutLN o;
            const OutLN* po = nullptr;
            if (nx) { o = next_ln(stages[nx->stage], nx); po = &o; }
            else if (final_ln_fused && l == last) {
                o.m = P("norm.m"); o.s = P("norm.s"); o.e = zero_row.f(); o.y = nfin.f();
                po = &o;
            }
            const int st_ = run_layer(l, x, add, s, y_ready, po);
            y_ready = nx != nullptr;
            ++oi;
            return st_;
        };
        for (auto* l : d_layers) {
            stack.push_back(x);
            DWS_TRY(run(l, nullptr));
            x = l->out.f();
        }
        stack.push_back(x);
        for (size_t i = 0; i < c_layers.size(); ++i) {
            const float* add = nullptr;
            if (i + 1 == c_layers.size()) { add = stack.back(); stack.pop_back(); }
            DWS_TRY(run(c_layers[i], add));
            x = c_layers[i]->out.f();
        }
        for (auto* l : u_layers) {
            const float* add = nullptr;
            if (l->kind == L_UP || unet) { add = stack.back(); stack.pop_back(); }
            DWS_TRY(run(l, add));
            x = l->out.f();
        }
        last_x = x;
        DWS_TRY(final_stage(x, out, nullptr, s, final_ln_fused));
        // ragged batches: exact 0.0f behind every clip's own end, whatever the padded positions computed
        if (ragged()) DWS_TRY(launch_wn_mask_tail(out, lengths_ptr(), (int)B, Cout, (int)L, -1, nullptr, 0, nullptr, 0, s));
        DWS_HIP(hipGetLastError());
        return DWS_OK;
    }


    // ------------------------------------------------------------------ training path
    // Execution plan of Sashimi.forward (sashimi.py:293-307) as nodes: node 0 = init-conv output,
    // node i+1 = output of plan[i].  The skip stack becomes add_node references.
    void build_plan() {
        if (!plan.empty()) return;
        std::vector<int> stack;
        int x = 0;
        auto push = [&](SLayer* l, int add) {
            plan.push_back({l, x, add});
            x = (int)plan.size();
        };
        for (auto* l : d_layers) { stack.push_back(x); push(l, -1); }
        stack.push_back(x);
        for (size_t i = 0; i < c_layers.size(); ++i) {
            int add = -1;
            if (i + 1 == c_layers.size()) { add = stack.back(); stack.pop_back(); }
            push(c_layers[i], add);
        }
        for (auto* l : u_layers) {
            int add = -1;
            if (l->kind == L_UP || unet) { add = stack.back(); stack.pop_back(); }
            push(l, add);
        }
    }
    float* node_act(int i) { return i == 0 ? x_init.f() : plan[i - 1].l->out.f(); }
    float* node_grad(int i) { return i == 0 ? dx_init.f() : plan[i - 1].l->dbuf.f(); }
    size_t node_numel(int i) {
        if (i == 0) return (size_t)B * D * L;
        SLayer* l = plan[i - 1].l;
        return (l->kind == L_BLOCK) ? (size_t)B * l->H * l->L : (size_t)B * l->Hout * l->Lout;
    }

    // Row-major weights behind the packed operands handed to gemm(): shapes the MFMA position-tile GEMM does not tile
    // (rows or contraction not a multiple of 32: test-sized models) run the plain-FMA GEMM on these instead.
    struct RowMajor { const float* w; int M, K; };
    std::map<const float*, RowMajor> row_major;
    DevBuf rAfT;
    std::vector<DevBuf*> row_major_bufs;   // owned transposes

    // A-fragment pack of W [O][K] and of its transpose (the adjoint GEMM).  `packed`: the commit's own pack of W when it
    // made one (same layout) -- reused instead of packing again; *pA receives the operand to hand to gemm().
    int pack_pair(const float* W, int O, int K, DevBuf& A, DevBuf& AT, const float* packed, const float** pA, hipStream_t s) {
        DWS_TRY(A.ensure((size_t)O * K * 4));
        DWS_TRY(AT.ensure((size_t)O * K * 4));
        if (tapconv_mfma_supported(O, K, 0, 1) && tapconv_mfma_supported(K, O, 0, 1)) {
            if (packed) {
                *pA = packed;
            } else {
                prep_train.pack(W, A.f(), O, K);
                *pA = A.f();
            }
            prep_train.pack_t(W, AT.f(), O, K);     // (pack_train runs the batch: one launch for every weight)
            return DWS_OK;
        }
        // generic: A / AT only serve as keys; AT's storage holds the row-major transpose itself
        DWS_TRY(launch_tapconv_pack_transposed(W, AT.f(), O, K, 1, O, 0, 1.f, s));
        row_major[A.f()] = RowMajor{W, O, K};
        row_major[AT.f()] = RowMajor{AT.f(), K, O};
        *pA = A.f();
        return DWS_OK;
    }

    int pack_train(hipStream_t s) {
        row_major.clear();
        prep_train.begin();
        for (auto* l : all) {
            if (l->kind == L_BLOCK) {
                const int H = l->H;
                const bool cp = l->mfma;   // the commit packed Ao / A1 / A2 for the sampling tail kernel
                DWS_TRY(pack_pair(P(l->prefix + ".layer.output_linear.0.weight"), 2 * H, H, l->tAo, l->tAoT, cp ? l->Ao.f() : nullptr,
                                  &l->pAo, s));
                DWS_TRY(pack_pair(l->W1.f(), FF * H, H, l->tA1, l->tA1T, cp ? l->A1.f() : nullptr, &l->pA1, s));
                DWS_TRY(pack_pair(l->W2.f(), H, FF * H, l->tA2, l->tA2T, cp ? l->A2.f() : nullptr, &l->pA2, s));
            } else {
                const int O = (l->kind == L_DOWN) ? l->Hout : l->Hout * l->p;
                const int K = (l->kind == L_DOWN) ? l->H * l->p : l->H;
                DWS_TRY(pack_pair(l->Wp.f(), O, K, l->tAp, l->tApT, (l->mfma || l->mfma2) ? l->Ap.f() : nullptr, &l->pAp, s));
            }
        }
        DWS_TRY(tmp_pack.ensure((size_t)D * D * 4));
        DWS_TRY(tAfT.ensure((size_t)D * D * 4));
        if (tapconv_mfma_supported(D, D, 0, 1)) {
            prep_train.pack_t(Wf.f(), tAfT.f(), D, D);
        } else {
            DWS_TRY(launch_tapconv_pack_transposed(Wf.f(), tAfT.f(), D, D, 1, D, 0, 1.f, s));
            row_major[tAfT.f()] = RowMajor{tAfT.f(), D, D};
        }
        DWS_TRY(prep_train.run(s));
        train_pack_version = commit_version;
        return DWS_OK;
    }

    // out[b, m, l] = epi(sum_k A[m, k] src[b, k, l])   (tapconv_mfma, T = 1)
    // LayerNorm fused into a training GEMM's epilogue (TapConvArgs::ln_*): destination, the norm's scalars, optional fc_t rows
    struct LnFuse { float* out; const float* m; const float* s; const float* pt; int pt_bstride; };
    bool train_ln_fusion = true;
    bool ln_fusable(const float* A, int epi, int M, int Lx) const {
        static const bool off = getenv("DWS_TRAIN_NO_LN_FUSION") != nullptr;     // same-box A/B switch
        return !off && train_ln_fusion && row_major.find(A) == row_major.end() && tapconv_ln_supported(epi, M, Lx);
    }
    int gemm(const float* A, int M, int K, const float* src, float* out, int Lx, int epi, const float* bias,
             const float* res, const float* addend, const float* aux, float* out2, hipStream_t s, const LnFuse* ln = nullptr) {
        auto it = row_major.find(A);
        if (it != row_major.end()) {
            DWS_CHECK(!ln, DWS_ERR_STATE, "gemm: LayerNorm epilogue requested on the plain-FMA path");
            DWS_CHECK(it->second.M == M && it->second.K == K, DWS_ERR_STATE, "gemm: operand registered as %d x %d, used as %d x %d",
                      it->second.M, it->second.K, M, K);
            GemmRowsArgs g{};
            g.W = it->second.w; g.src = src; g.out = out; g.bias = bias; g.res = res; g.addend = addend; g.aux = aux;
            g.addin = (epi == 0) ? aux : nullptr; g.out2 = out2; g.B = (int)B; g.M = M; g.K = K; g.L = Lx; g.epi = epi;
            return launch_gemm_rows_generic(g, s);
        }
        TapConvArgs q{};
        q.src0 = src; q.K0 = K; q.A = A; q.nkg_total = K / 8; q.M = M; q.T = 1; q.dil = 1; q.sign = 1; q.epi = epi;
        q.out = out; q.bias = bias; q.res = res; q.addend = addend; q.aux = aux; q.out2 = out2;
        q.addin = (epi == 0) ? aux : nullptr; q.addscale = 1.f;
        q.B = (int)B; q.L = Lx;
        q.split = bf16x6 ? 1 : 0;      // precision = bf16x6: the pointwise GEMMs of the training step on the bf16 matrix cores
        if (ln) { q.ln_out = ln->out; q.ln_m = ln->m; q.ln_s = ln->s; q.ln_pt = ln->pt; q.ln_pt_bstride = ln->pt_bstride; }
        return launch_tapconv_mfma(q, s);
    }

    // dW[o, c] = sum_{b, l} dY[b, o, l] * act(X[b, c, l]);  db[o] = sum_{b, l} dY[b, o, l] (optional, same pass)
    // wn != nullptr: the weight is the weight-normed tensor `*wn` -- its adjoint runs inside the split-K reduce (dv / dg written
    // directly; dW is not used)
    int wgrad(const float* dY, const float* X, int O, int Cc, int Lx, int xact, float* dW, float* db, hipStream_t s,
              const std::string* wn = nullptr) {
        static const bool wn_separate = getenv("DWS_WN_BWD_SEPARATE") != nullptr;     // same-box A/B switch
        if (wn && (wn_separate || Cc > WGRAD_WN_MAX_INNER)) {
            DWS_TRY(wgrad(dY, X, O, Cc, Lx, xact, dW, db, s));
            return wn_bwd(*wn, dW, O, Cc, s);
        }
        WgradArgs w{};
        if (wn) {
            w.wn_v = P(*wn + ".weight_v"); w.wn_g = P(*wn + ".weight_g");
            w.wn_dv = G(*wn + ".weight_v"); w.wn_dg = G(*wn + ".weight_g");
        }
        w.dY = dY; w.X = X; w.B = (int)B; w.O = O; w.C = Cc; w.L = Lx; w.dil = 1; w.xact = xact;
        w.nsplit = wgrad_mfma_nsplit((int)B, O, Cc, Lx, 1);
        DWS_TRY(wpart.ensure((size_t)w.nsplit * O * Cc * 4));
        w.partial = wpart.f();
        if (db) {
            DWS_TRY(bpart.ensure((size_t)w.nsplit * O * 4));
            w.bias_part = bpart.f(); w.dbias = db; w.bias_scale = 1.f;
        }
        w.split = bf16x6 ? 1 : 0;
        return launch_wgrad_mfma(w, 1, 1.f, dW, s);
    }

    int wn_bwd(const std::string& p, const float* dWf, int O, int inner, hipStream_t s) {
        return launch_weight_norm_bwd(dWf, P(p + ".weight_v"), P(p + ".weight_g"), G(p + ".weight_v"), G(p + ".weight_g"), O,
                                      inner, s);
    }

    // what every training forward asks of the installed condition
    int train_condition_ok() {
        DWS_CHECK(melBm == 0 || melBm == B, DWS_ERR_UNSUPPORTED,
                  "mel-conditional training needs one mel per clip (got %lld for B=%lld)", (long long)melBm, (long long)B);
        DWS_CHECK(!cond || melBm > 0, DWS_ERR_STATE, "conditional model: install the mel (set_condition) before forward_train");
        return DWS_OK;
    }

    // forward_train: every block at its kernel's own length on the fused convolution or rocFFT -- what the PARAMETER gradients
    // are built for (fftcorr, the spectrum / taps adjoints, the stacked groups).  The data-only pair (forward_input) has
    // no such limit.
    int train_supported() {
        DWS_TRY(train_condition_ok());
        for (auto* l : all) {
            if (l->kind == L_BLOCK) {
                // (a stage runs the fused LDS convolution or rocFFT; the segmented path needs kernels shorter than the stage)
                DWS_CHECK(!l->seg, DWS_ERR_UNSUPPORTED,
                          "sashimi training does not run the segmented convolution (stage L=%d): parameter gradients are built "
                          "on the fused and rocFFT stages; input gradients alone (eval() mode, dws_model_forward_input) run here",
                          l->L);
                DWS_CHECK(l->Lk == l->L, DWS_ERR_UNSUPPORTED,
                          "sashimi training runs at the kernels' own length (stage runs at %d, kernel length %d): parameter gradients "
                          "are not built at another; input gradients alone (eval() mode, dws_model_forward_input) run at any length",
                          l->L, l->Lk);
            }
        }
        return DWS_OK;   // channel counts that are not multiples of 32 train on the plain-FMA GEMM (row_major)
    }

    int ensure_train_buffers() {
        build_plan();
        for (auto* st : stages) {
            const size_t rows = (size_t)B * st->H * st->L * 4;
            DWS_TRY(st->d2.ensure(rows * std::max(2, FF)));
            DWS_TRY(st->dh.ensure(rows));
            DWS_TRY(st->dx1.ensure(rows));
            DWS_TRY(st->du.ensure(rows));
            DWS_TRY(st->y.ensure(rows));
        }
        size_t pool_max = 4;
        for (auto* l : all) {
            if (l->kind == L_BLOCK) {
                const size_t n = (size_t)B * l->H * l->L * 4;
                if (l->log2m == 0 && !l->seg) {    // rocFFT stage: padded rows, spectra, plans (prepare() made them for this B already)
                    Stage* st = stages[l->stage];
                    DWS_TRY(ensure_rocfft_stage(st));
                    DWS_TRY(st->Gf.ensure((size_t)B * st->H * (st->L + 1) * 8));
                }
                DWS_TRY(l->t_u.ensure(n)); DWS_TRY(l->t_a.ensure(n)); DWS_TRY(l->t_o.ensure(2 * n));
                DWS_TRY(l->t_g.ensure(n)); DWS_TRY(l->t_ge.ensure((size_t)FF * n));
                DWS_TRY(l->t_x1.ensure(n)); DWS_TRY(l->t_n2.ensure(n)); DWS_TRY(l->t_f1.ensure((size_t)FF * n));
                DWS_TRY(l->dbuf.ensure(n));
            } else {
                const size_t nin = (size_t)B * l->H * l->L * 4, nout = (size_t)B * l->Hout * l->Lout * 4;
                DWS_TRY(l->dbuf.ensure(nout));
                if (l->kind == L_DOWN) DWS_TRY(l->t_xr.ensure(nin));
                pool_max = std::max(pool_max, std::max(nin, nout));
            }
        }
        DWS_TRY(pool_scr.ensure(pool_max));
        DWS_TRY(dx_init.ensure((size_t)B * D * L * 4));
        DWS_TRY(ty.ensure((size_t)B * D * L * 4));
        DWS_TRY(dyb.ensure((size_t)B * D * L * 4));
        DWS_TRY(dnf.ensure((size_t)B * D * L * 4));
        DWS_TRY(ta1.ensure((size_t)B * Emid * 4));
        DWS_TRY(ta2.ensure((size_t)B * Eout * 4));
        ln_slot_floats = (size_t)B * ceil_div(L, 64) * 2;       // a slot per LayerNorm adjoint: two per block + the final norm
        ln_slots = 1;
        for (auto* l : all) ln_slots += (l->kind == L_BLOCK) ? 2 : 0;
        DWS_TRY(lnpart.ensure(ln_slot_floats * ln_slots * 4));
        return DWS_OK;
    }

    int forward_train(const float* audio, const float* steps, float* out, hipStream_t s) override {
        return train_forward(audio, steps, out, false, s);
    }

    // The training forward for a data-only backward (dws_model_forward_input).  Where forward_train runs -- every block at its
    // kernel's own length -- this IS forward_train.  Otherwise (a run shorter or longer than the kernels, a stage on the
    // segmented convolution) the commit stays the sampling path's: per-block chains at Lt = min(L, Lk) taps (build_kernel),
    // and every block's convolution keeps its pre-activation on the route the sampler takes at this length.
    int forward_input(const float* audio, const float* steps, float* out, hipStream_t s) override {
        DWS_CHECK(B > 0, DWS_ERR_STATE, "forward before prepare");
        bool own_length = true;
        for (auto* l : all) {
            if (l->kind != L_BLOCK) continue;
            int64_t Lk = 0;
            DWS_TRY(kernel_len(l, s, &Lk));
            if (Lk != l->L) own_length = false;      // (at Lk == L > 16384 the stage leaves the segmented path: resolve_segmented_stages)
        }
        DWS_TRY(train_forward(audio, steps, out, !own_length, s));
        input_only = true;
        return DWS_OK;
    }

    int train_forward(const float* audio, const float* steps, float* out, bool any_length, hipStream_t s) {
        DWS_CHECK(B > 0, DWS_ERR_STATE, "forward before prepare");
        DWS_CHECK(!ragged(), DWS_ERR_UNSUPPORTED, "training with per-clip lengths (dws_model_set_lengths) is not built");
        DWS_CHECK(!f16x3, DWS_ERR_UNSUPPORTED,
                  "training runs with precision=f32 or bf16x6 (gradients span too many binades for the fixed scales of the fp16 split)");
        if (!any_length) keep_cauchy = true;
        if (dirty) DWS_TRY(commit(s));
        if (any_length) DWS_TRY(train_condition_ok());
        else DWS_TRY(train_supported());
        DWS_TRY(ensure_train_buffers());
        if (train_pack_version != commit_version) DWS_TRY(pack_train(s));
        const int nB = (int)B;
        DWS_TRY(launch_init_conv(audio, Wi.f(), P("init_conv.0.conv.bias"), x_init.f(), nB, Cin, D, (int)L, s));
        DWS_TRY(launch_step_embed(steps, freq.f(), emb.f(), nB, Ein / 2, s));
        DWS_TRY(launch_linear_rows(emb.f(), P("fc_t1.weight"), P("fc_t1.bias"), h1.f(), nB, Ein, Emid, 1, s, ta1.f()));
        DWS_TRY(launch_linear_rows(h1.f(), P("fc_t2.weight"), P("fc_t2.bias"), h2.f(), nB, Emid, Eout, 1, s, ta2.f()));
        if (n_classes > 0) DWS_TRY(launch_label_add(h2.f(), P(label_param), labels_ptr(), nB, n_classes, h2.f(), nB, 1, Eout, s));
        DWS_TRY(launch_linear_rows(h2.f(), Wt_all.f(), bt_all.f(), part_t.f(), nB, Eout, pt_total, 0, s));
        bool ln1_done = false;      // this block's LN1 came out of the previous block's epilogue
        for (size_t i = 0; i < plan.size(); ++i) {
            const Exec& e = plan[i];
            SLayer* l = e.l;
            const float* x = node_act(e.in_node);
            const float* add = e.add_node >= 0 ? node_act(e.add_node) : nullptr;
            if (l->kind == L_BLOCK) {
                Stage* st = stages[l->stage];
                const int H = l->H, Ls = l->L;
                const std::string& p = l->prefix;
                // LN1(x) + fc_t(e): already written by the previous block's last GEMM when that one could fuse it (below)
                if (!ln1_done)
                    DWS_TRY(launch_ln(x, P(p + ".norm1.m"), P(p + ".norm1.s"), part_t.f() + l->pt_off, pt_total, l->t_u.f(), nB, H,
                                      Ls, (size_t)Ls, s));
                ln1_done = false;
                if (l->log2m > 0) {
                    FftTables* t = tables[l->log2m];
                    FftConvArgs fa{};
                    fa.u = l->t_u.f(); fa.g = l->t_g.f(); fa.pre = l->t_a.f(); fa.D = P(p + ".layer.D");
                    fa.tw = (const c2*)t->tw.p; fa.twp = (const c2*)t->twp.p;
                    fa.kfa = (const c2*)l->kfa_v; fa.kfb = (const c2*)l->kfb_v; fa.kfs = (const c2*)l->kfs_v;
                    fa.B = nB; fa.H = H; fa.L = Ls;
                    DWS_TRY(launch_fftconv(l->log2m, fa, s));
                } else if (l->seg) {      // (forward_input only)
                    FftConvSegArgs fa = seg_args(l);
                    fa.u = l->t_u.f(); fa.g = l->t_g.f(); fa.pre = l->t_a.f();
                    DWS_TRY(launch_fftconv_seg_train(fa, s));
                } else {
                    DWS_TRY(rocfft_conv_forward(l, st, s));
                }
                // LN2(x1) out of the epilogue that produces x1 when the tile holds every channel (H = 128): the separate
                // LayerNorm pass (read x1, write n2) becomes one extra store
                bool ln2_done = false;
                if (tapconv_glu_supported(2 * H, H, Ls)) {   // o and x1 = x + GLU(o) (+ mel) from one kernel
                    LnFuse f2{l->t_n2.f(), P(p + ".norm2.m"), P(p + ".norm2.s"), nullptr, 0};
                    ln2_done = ln_fusable(l->pAo, 6, 2 * H, Ls);
                    DWS_TRY(gemm(l->pAo, 2 * H, H, l->t_g.f(), l->t_o.f(), Ls, 6, P(p + ".layer.output_linear.0.bias"), x,
                                 nullptr, melBm ? l->melc.f() : nullptr, l->t_x1.f(), s, ln2_done ? &f2 : nullptr));
                } else {
                    DWS_TRY(gemm(l->pAo, 2 * H, H, l->t_g.f(), l->t_o.f(), Ls, 2, P(p + ".layer.output_linear.0.bias"),
                                 nullptr, nullptr, nullptr, nullptr, s));
                    DWS_TRY(launch_glu_res(l->t_o.f(), x, melBm ? l->melc.f() : nullptr, l->t_x1.f(), nB, H, Ls, s));
                }
                if (!ln2_done)
                    DWS_TRY(launch_ln(l->t_x1.f(), P(p + ".norm2.m"), P(p + ".norm2.s"), nullptr, 0, l->t_n2.f(), nB, H, Ls,
                                      (size_t)Ls, s));
                DWS_TRY(gemm(l->pA1, FF * H, H, l->t_n2.f(), l->t_f1.f(), Ls, 3, P(p + ".ff.ff.0.conv.bias"), nullptr,
                             nullptr, nullptr, l->t_ge.f(), s));
                // the NEXT block's LN1(out) + fc_t(e) out of this block's last epilogue (same stage, H = 128 / 256)
                SLayer* nx = (i + 1 < plan.size() && plan[i + 1].l->kind == L_BLOCK) ? plan[i + 1].l : nullptr;
                LnFuse f1{};
                if (nx && nx->H == H && nx->L == Ls && ln_fusable(l->pA2, 4, H, Ls)) {
                    f1 = LnFuse{nx->t_u.f(), P(nx->prefix + ".norm1.m"), P(nx->prefix + ".norm1.s"), part_t.f() + nx->pt_off, (int)pt_total};
                    ln1_done = true;
                }
                DWS_TRY(gemm(l->pA2, H, FF * H, l->t_ge.f(), l->out.f(), Ls, 4, P(p + ".ff.ff.2.conv.bias"), l->t_x1.f(),
                             add, nullptr, nullptr, s, ln1_done ? &f1 : nullptr));
            } else if (l->kind == L_DOWN) {
                DWS_TRY(launch_pool_rearrange(x, l->t_xr.f(), nullptr, 0, 0, nB, l->H, l->p, l->Lout, s));
                DWS_TRY(gemm(l->pAp, l->Hout, l->H * l->p, l->t_xr.f(), l->out.f(), l->Lout, 2,
                             P(l->prefix + ".linear.conv.bias"), nullptr, nullptr, nullptr, nullptr, s));
            } else {
                DWS_TRY(gemm(l->pAp, l->Hout * l->p, l->H, x, pool_scr.f(), l->L, 2, P(l->prefix + ".linear.conv.bias"),
                             nullptr, nullptr, nullptr, nullptr, s));
                DWS_TRY(launch_pool_rearrange(pool_scr.f(), l->out.f(), add, 1, 0, nB, l->Hout, l->p, l->L, s));
            }
        }
        last_x = node_act((int)plan.size());
        DWS_TRY(final_stage(last_x, out, ty.f(), s));
        DWS_HIP(hipGetLastError());
        train_audio = audio;
        trained_fwd = true;
        input_only = false;      // (forward_input sets it)
        return DWS_OK;
    }

    // The adjoint of a group's stacked kernel generation, once the spectrum gradients of all its blocks are in g->dKf; the
    // stacked parameter gradients leave for the blocks' tensors in one launch.
    int group_backward(KGroup* g, hipStream_t s) {
        const int H = g->H, Ht = g->Ht(), N = NS, n = (int)g->layers.size();
        const size_t HN = (size_t)Ht * N;
        DWS_TRY(g->gC.ensure(2 * HN * 8)); DWS_TRY(g->gB.ensure(HN * 8)); DWS_TRY(g->gP.ensure(HN * 8));
        DWS_TRY(g->giwr.ensure(HN * 4)); DWS_TRY(g->gwim.ensure(HN * 4)); DWS_TRY(g->glogdt.ensure((size_t)Ht * 4));
        DWS_TRY(g->gD.ensure((size_t)Ht * 4));
        const S4Tensors grad{g->gC.f(), g->gB.f(), g->gP.f(), g->giwr.f(), g->gwim.f(), g->glogdt.f()};
        DWS_TRY(s4_spectrum_adjoint(*this, g->chain, g->log2m, g->dKf.f(), g->gD.f(), s));
        DWS_TRY(s4_taps_adjoint(*this, g->chain, commit_version, grad, s));
        g->unstack.begin();
        for (int i = 0; i < n; ++i) {
            stack_rows(g->unstack, true, kernel_tensors(g->layers[i], true), grad, i, H, N, n);
            g->unstack.add(g->gD.f() + (size_t)i * H, G(g->layers[i]->prefix + ".layer.D"), (size_t)H);
        }
        return g->unstack.run(s);
    }

    // gradient of the S4 kernel parameters of one block from u and da (s4.py:704-807 backwards): the block's spectrum gradient
    // dK_f = corr(u, da), then the adjoint of its chain -- at once for a block on its own, once per group when the last of the
    // group's blocks has put its rows into the group's stack
    int kernel_backward(SLayer* l, const float* da, hipStream_t s) {
        KGroup* g = (kernels_stacked && l->grp >= 0) ? kgroups[l->grp] : nullptr;
        const int H = l->H, nB = (int)B, M = 1 << l->log2m;
        const size_t row_floats = (size_t)H * (M + 1) * 2;
        FftTables* t = tables[l->log2m];
        const int nbs = std::max(1, std::min(nB, ceil_div(512, H)));
        const int bchunk = ceil_div(nB, nbs);
        const int nchunks = ceil_div(nB, bchunk);
        DevBuf& dst = g ? g->dKf : dKf;      // the block's rows of its chain's spectrum gradient
        DWS_TRY(fpart.ensure(nchunks * row_floats * 4));
        DWS_TRY(dst.ensure((g ? g->layers.size() : 1) * row_floats * 4));
        FftCorrArgs c{};
        c.u = l->t_u.f(); c.da = da; c.part = (c2*)fpart.p; c.tw = (const c2*)t->tw.p; c.twp = (const c2*)t->twp.p;
        c.B = nB; c.H = H; c.L = l->L; c.bchunk = bchunk;
        DWS_TRY(launch_fftcorr(l->log2m, c, s));
        DWS_TRY(launch_sum_leading(fpart.f(), dst.f() + (g ? l->gidx : 0) * row_floats, row_floats, nchunks, 1.f, s));
        if (g) return --g->pending == 0 ? group_backward(g, s) : DWS_OK;
        DWS_TRY(s4_spectrum_adjoint(*this, l->own, l->log2m, dKf.f(), G(l->prefix + ".layer.D"), s));
        return s4_taps_adjoint(*this, l->own, commit_version, kernel_tensors(l, true), s);
    }

    // S4 convolution of a block whose stage runs on rocFFT (odd length, or more than 16384 samples), training forward: the
    // sampling path's R2C -> spectrum multiply -> C2R (run_block) on the padded rows of u = t_u, whose epilogue also keeps the
    // pre-activation a in t_a.  t_u stays unpadded so that the previous block's epilogue can still write it (ln1_done); the
    // padded rows are a copy.
    int rocfft_conv_forward(SLayer* l, Stage* st, hipStream_t s) {
        ProfileScope ps("long_stage_fwd", s);
        const int H = l->H, Ls = l->L, nB = (int)B, rows = nB * H;
        DWS_TRY(launch_pad_rows(l->t_u.f(), st->U.f(), rows, Ls, s));
        {
            ProfileScope ps("rocfft_r2c", s);
            DWS_TRY(fft.exec(0, 2 * Ls, rows, st->U.p, st->Uf.p, s));
        }
        DWS_TRY(launch_spec_mul(st->Uf.f(), l->Kf.f(), nB, H, Ls + 1, s));
        {
            ProfileScope ps("rocfft_c2r", s);
            DWS_TRY(fft.exec(1, 2 * Ls, rows, st->Uf.p, st->Y.p, s));
        }
        return launch_s4_post_train(st->Y.f(), l->t_u.f(), P(l->prefix + ".layer.D"), l->t_a.f(), l->t_g.f(), nB, H, Ls, s);
    }

    // Its adjoint, given da [B][H][L]: du = C2R(conj(K_f) dA) / 2L + D da into `du`, d fc_t(e) = sum_l du into dpt, dD, and the
    // kernel parameters' gradients through dK_f = sum_b conj(U_b) dA_b -> C2R -> the two-sided assembly backwards -> the taps
    // adjoint of the block's chain.  U_f is recomputed here (one R2C of the padded t_u) instead of being kept from the forward:
    // keeping it would cost B H (L+1) 8 bytes per block for the whole step (90 MB per top-stage block of ljspeech_harder, twelve of them)
    // to save one transform of the same size, and it would need an out-of-place spectrum multiply in the forward.
    // pg = false (data-only backward): du alone -- R2C(da), the product with conj(K_f), C2R and the epilogue without its row sum.
    int rocfft_conv_backward(SLayer* l, Stage* st, const float* da, float* du, bool pg, hipStream_t s) {
        ProfileScope ps("long_stage_bwd", s);
        const int H = l->H, Ls = l->L, Lf = Ls + 1, nB = (int)B, rows = nB * H;
        const int Lk = l->Lk, Lt = std::min(Ls, Lk), Lh = Lk / 2 + 1;
        if (!pg) {
            DWS_TRY(launch_pad_rows(da, st->U.f(), rows, Ls, s));
            DWS_TRY(fft.exec(0, 2 * Ls, rows, st->U.p, st->Uf.p, s));       // dA
            DWS_TRY(launch_conv_adjoint_spec_data(st->Uf.f(), l->Kf.f(), nB, H, Lf, s));
            DWS_TRY(fft.exec(1, 2 * Ls, rows, st->Uf.p, st->Y.p, s));
            return launch_conv_adjoint_epi(st->Y.f(), da, P(l->prefix + ".layer.D"), du, nullptr, 0, nB, H, Ls, s);
        }
        DWS_TRY(dKf.ensure((size_t)H * Lf * 8));
        DWS_TRY(dKt.ensure((size_t)H * 2 * Ls * 4));
        DWS_TRY(dkt.ensure((size_t)2 * H * Lk * 4));
        DWS_TRY(dkf.ensure((size_t)2 * H * Lh * 8));
        DWS_TRY(launch_pad_rows(l->t_u.f(), st->U.f(), rows, Ls, s));
        DWS_TRY(fft.exec(0, 2 * Ls, rows, st->U.p, st->Gf.p, s));       // U
        DWS_TRY(launch_pad_rows(da, st->U.f(), rows, Ls, s));
        DWS_TRY(fft.exec(0, 2 * Ls, rows, st->U.p, st->Uf.p, s));       // dA
        DWS_TRY(launch_conv_adjoint_spec(st->Gf.f(), st->Uf.f(), l->Kf.f(), dKf.f(), nB, H, Lf, s));
        DWS_TRY(fft.exec(1, 2 * Ls, rows, st->Uf.p, st->Y.p, s));
        DWS_TRY(launch_conv_adjoint_epi(st->Y.f(), da, P(l->prefix + ".layer.D"), du, dpt.f() + l->pt_off, (int)pt_total, nB, H, Ls, s));
        // dK = C2R(dK_f) / 2L; K = [k0 | 0 | reversed k1] / Lk (s4_twosided_kernel); dD[h] = sum u da = dK[h][0]
        DWS_TRY(fft.exec(1, 2 * Ls, H, dKf.p, dKt.p, s));
        DWS_TRY(launch_s4_twosided_bwd(dKt.f(), dkt.f(), G(l->prefix + ".layer.D"), H, Ls, Lk, Lt,
                                       1.f / ((float)(2 * Ls) * (float)Lk), 1.f / (float)(2 * Ls), s));
        DWS_TRY(fft.exec(0, Lk, 2 * H, dkt.p, dkf.p, s));
        return s4_taps_adjoint(*this, l->own, commit_version, kernel_tensors(l, true), s);
    }

    // (dm, ds) of a LayerNorm from its adjoint's per-block partials [2][nblk].  Every adjoint of a backward writes its own slot of
    // lnpart and the sums of all of them run as ONE launch at the end of the backward (ln_scalars_flush) -- they were 61 launches
    // of 8 us per config-5 step.  The scalars' gradients are therefore final at the end of backward only (G() is called there:
    // the staged hand-over learns it); they are 122 floats.
    struct LnPending { float* part; std::string name; int nblk; };
    std::vector<LnPending> ln_pending;
    std::vector<SumPairJob> ln_jobs, ln_jobs_uploaded;
    DevBuf ln_table;
    size_t ln_slot_floats = 0;
    int ln_slots = 0;
    bool ln_deferred() const {
        static const bool off = getenv("DWS_LN_SCALARS_SEPARATE") != nullptr;     // same-box A/B switch
        return !off;
    }
    float* ln_slot() {      // partial buffer of the NEXT LayerNorm adjoint of this backward
        if (!ln_deferred() || (int)ln_pending.size() >= ln_slots) return lnpart.f();
        return lnpart.f() + ln_pending.size() * ln_slot_floats;
    }
    int ln_scalars(const std::string& p, int nblk, hipStream_t s) {
        if (!ln_deferred() || (int)ln_pending.size() >= ln_slots)
            return launch_sum_pair(ln_slot(), G(p + ".m"), G(p + ".s"), nblk, s);
        ln_pending.push_back({ln_slot(), p, nblk});
        return DWS_OK;
    }
    int ln_scalars_flush(hipStream_t s) {
        if (ln_pending.empty()) return DWS_OK;
        ln_jobs.clear();
        for (auto& e : ln_pending) ln_jobs.push_back({e.part, G(e.name + ".m"), G(e.name + ".s"), e.nblk, 0});
        ln_pending.clear();
        const bool same = ln_jobs.size() == ln_jobs_uploaded.size() &&
                          std::memcmp(ln_jobs.data(), ln_jobs_uploaded.data(), ln_jobs.size() * sizeof(SumPairJob)) == 0;
        if (!same) {
            DWS_HIP(hipStreamSynchronize(s));
            ln_jobs_uploaded = ln_jobs;
            DWS_TRY(ln_table.ensure(ln_jobs.size() * sizeof(SumPairJob)));
            DWS_HIP(hipMemcpy(ln_table.p, ln_jobs.data(), ln_jobs.size() * sizeof(SumPairJob), hipMemcpyHostToDevice));
        }
        return launch_sum_pair_multi((const SumPairJob*)ln_table.p, (int)ln_jobs.size(), s);
    }

    // Adjoint of forward_train, plan steps in reverse (sashimi.py:143-184,277-313).
    // daudio (optional): the gradient w.r.t. the audio input.  pg = false (data-only, needs daudio): the data path alone, the
    // same kernels in the same order (daudio has the same bits in both modes) -- no weight / bias gradient, no weight-norm
    // adjoint, no S4 kernel adjoint (fftcorr / spectrum adjoint / taps adjoint), no LayerNorm parameter sums, no d fc_t(e),
    // no embedding or conditioner adjoint, no G() access and no flush point.
    int backward(const float* dout, float* daudio, bool pg, hipStream_t s) override {
        DWS_CHECK(trained_fwd, DWS_ERR_STATE, "backward without a preceding forward_train");
        DWS_CHECK(!pg || !input_only, DWS_ERR_STATE,
                  "backward: the pending forward is dws_model_forward_input, which keeps what a data-only backward needs "
                  "(param_grads = 0); parameter gradients need dws_model_forward_train");
        DWS_CHECK(pg || daudio, DWS_ERR_INVALID, "backward: a data-only pass needs a destination for the input gradient");
        const int nB = (int)B, nL = (int)L;
        const int nnodes = (int)plan.size() + 1;
        ln_pending.clear();
        for (auto* g : kgroups) g->pending = (int)g->layers.size();
        std::vector<char> written(nnodes, 0);
        std::vector<float*> gp(nnodes);       // where each node's gradient lives during THIS backward (a skip node may adopt a dy buffer)
        for (int n = 0; n < nnodes; ++n) gp[n] = node_grad(n);
        size_t wmax = (size_t)D * D;
        for (auto* l : all) {
            if (l->kind == L_BLOCK) wmax = std::max(wmax, (size_t)2 * l->H * l->H * std::max(1, FF));
            else wmax = std::max(wmax, (size_t)l->H * l->p * l->Hout * std::max(l->p, 1));
        }
        if (pg) {
            DWS_TRY(dWfold.ensure(wmax * 4));
            DWS_TRY(dpt.ensure((size_t)B * pt_total * 4));
            DWS_TRY(dh2.ensure((size_t)B * Eout * 4)); DWS_TRY(dh1.ensure((size_t)B * Emid * 4));
            DWS_TRY(dWt_all.ensure((size_t)pt_total * Eout * 4)); DWS_TRY(dbt_all.ensure((size_t)pt_total * 4));
        }

        // ---- final stage: out = Wz y + bz, y = relu(Wf LN(x) + bf)
        // (1 x D and D x 1 weight gradients also go through the MFMA kernel: its tile is mostly padding there, but the
        // generic FMA kernel took 2.3 ms per call on [B, ., L] = 512000 positions)
        if (pg) DWS_TRY(wgrad(dout, ty.f(), Cout, D, nL, 0, G("final_conv.2.conv.weight"), G("final_conv.2.conv.bias"), s));
        DWS_TRY(launch_final_dy(dout, P("final_conv.2.conv.weight"), ty.f(), dyb.f(), nB, D, Cout, nL, s));
        if (pg) { const std::string wn_ = "final_conv.0.conv"; DWS_TRY(wgrad(dyb.f(), nfin.f(), D, D, nL, 0, dWfold.f(), G("final_conv.0.conv.bias"), s, &wn_)); }
        DWS_TRY(gemm(tAfT.f(), D, D, dyb.f(), dnf.f(), nL, 2, nullptr, nullptr, nullptr, nullptr, nullptr, s));
        {
            const int last = nnodes - 1;
            DWS_TRY(launch_ln_bwd(node_act(last), dnf.f(), P("norm.m"), P("norm.s"), nullptr, gp[last], 0, pg ? ln_slot() : nullptr,
                                  nB, D, nL, s));
            if (pg) DWS_TRY(ln_scalars("norm", nB * ceil_div(nL, 64), s));
            written[last] = 1;
        }

        for (int i = (int)plan.size() - 1; i >= 0; --i) {
            const Exec& e = plan[i];
            SLayer* l = e.l;
            const float* x = node_act(e.in_node);
            const float* dy = gp[i + 1];
            float* din = gp[e.in_node];
            DWS_CHECK(written[i + 1], DWS_ERR_STATE, "backward: no gradient reached node %d", i + 1);
            const std::string& p = l->prefix;
            if (l->kind == L_BLOCK) {
                Stage* st = stages[l->stage];
                const int H = l->H, Ls = l->L, nblk = nB * ceil_div(Ls, 64);
                // ff: out = x1 + W2 gelu(f1) + b2, f1 = W1 n2 + b1
                DWS_TRY(gemm(l->tA2T.f(), FF * H, H, dy, st->d2.f(), Ls, 5, nullptr, nullptr, nullptr, l->t_f1.f(), nullptr, s));
                if (pg) { const std::string wn_ = p + ".ff.ff.2.conv"; DWS_TRY(wgrad(dy, l->t_ge.f(), H, FF * H, Ls, 0, dWfold.f(), G(p + ".ff.ff.2.conv.bias"), s, &wn_)); }
                DWS_TRY(gemm(l->tA1T.f(), H, FF * H, st->d2.f(), st->dh.f(), Ls, 2, nullptr, nullptr, nullptr, nullptr, nullptr, s));
                if (pg) { const std::string wn_ = p + ".ff.ff.0.conv"; DWS_TRY(wgrad(st->d2.f(), l->t_n2.f(), FF * H, H, Ls, 0, dWfold.f(), G(p + ".ff.ff.0.conv.bias"), s, &wn_)); }
                // norm2: dx1 = dy + LN'(dn2)
                // (the GLU adjoint rides on this kernel when it can: d o is written from the d x1 values in registers)
                const bool glu_fused = ln_bwd_fuses_glu(H);
                DWS_TRY(launch_ln_bwd(l->t_x1.f(), st->dh.f(), P(p + ".norm2.m"), P(p + ".norm2.s"), dy, st->dx1.f(), 0,
                                      pg ? ln_slot() : nullptr, nB, H, Ls, s, glu_fused ? l->t_o.f() : nullptr,
                                      glu_fused ? st->d2.f() : nullptr));
                if (pg) DWS_TRY(ln_scalars(p + ".norm2", nblk, s));
                if (melBm && pg) {  // x1 = ... + melc: the block's conditioner sees d x1 (`sashimi.py:160-175`)
                    const int s0 = d.mel_upsample[0], s1 = d.mel_upsample[1];
                    DWS_TRY(gW0f.ensure((size_t)3 * 2 * s0 * 4)); DWS_TRY(gW1f.ensure((size_t)3 * 2 * s1 * 4));
                    DWS_TRY(gWcf.ensure((size_t)H * MB * 4));
                    DWS_TRY(conditioner_backward(cws, mel_in.f(), nB, MB, mel_T, s0, s1, l->melW0.f(), P(p + ".upsample_conv2d.0.bias"),
                                                 l->melW1.f(), P(p + ".upsample_conv2d.1.bias"), l->melWc.f(), H, Ls, st->dx1.f(),
                                                 gW0f.f(), G(p + ".upsample_conv2d.0.bias"), gW1f.f(),
                                                 G(p + ".upsample_conv2d.1.bias"), gWcf.f(), s));
                    DWS_TRY(wn_bwd(p + ".upsample_conv2d.0", gW0f.f(), 1, 3 * 2 * s0, s));
                    DWS_TRY(wn_bwd(p + ".upsample_conv2d.1", gW1f.f(), 1, 3 * 2 * s1, s));
                    DWS_TRY(wn_bwd(p + ".mel_conv.conv", gWcf.f(), H, MB, s));
                    DWS_TRY(launch_rowsum(st->dx1.f(), G(p + ".mel_conv.conv.bias"), nB, H, Ls, 1.f, 0, s));
                }
                // x1 = x + glu(o), o = Wo gelu(a) + bo
                if (!glu_fused) DWS_TRY(launch_glu_bwd(st->dx1.f(), l->t_o.f(), st->d2.f(), nB, H, Ls, s));
                DWS_TRY(gemm(l->tAoT.f(), H, 2 * H, st->d2.f(), st->dh.f(), Ls, 5, nullptr, nullptr, nullptr, l->t_a.f(), nullptr, s));
                if (pg)
                    DWS_TRY(wgrad(st->d2.f(), l->t_g.f(), 2 * H, H, Ls, 0, G(p + ".layer.output_linear.0.weight"),
                                  G(p + ".layer.output_linear.0.bias"), s));
                // a = conv(u, K) + D u: du = conv^T(da) + D da; kernel parameters from corr(u, da)
                if (l->seg) {           // segmented stage (forward_input: pg is off): the same kernel on the conjugated spectra
                    FftConvSegArgs fa = seg_args(l);
                    fa.u = st->dh.f(); fa.g = st->du.f();
                    DWS_TRY(launch_fftconv_seg_adjoint(fa, s));
                } else if (l->log2m == 0) {    // rocFFT stage (rocfft_conv_backward also writes d fc_t(e) and every S4 kernel gradient)
                    DWS_TRY(rocfft_conv_backward(l, st, st->dh.f(), st->du.f(), pg, s));
                } else {
                    FftTables* t = tables[l->log2m];
                    FftConvArgs fa{};
                    fa.u = st->dh.f(); fa.g = st->du.f(); fa.D = P(p + ".layer.D"); fa.conj_k = 1; fa.no_act = 1;
                    fa.tw = (const c2*)t->tw.p; fa.twp = (const c2*)t->twp.p;
                    fa.kfa = (const c2*)l->kfa_v; fa.kfb = (const c2*)l->kfb_v; fa.kfs = (const c2*)l->kfs_v;
                    fa.B = nB; fa.H = H; fa.L = Ls;
                    // d fc_t(e)[b, h] = sum_l du[b, h, l] leaves with the row (a workgroup owns it) where the plan allows
                    const bool rs_fused = pg && fftconv_rowsum_supported(l->log2m) && getenv("DWS_NO_ROWSUM_FUSION") == nullptr;
                    if (rs_fused) { fa.rowsum = dpt.f() + l->pt_off; fa.rowsum_bstride = (int)pt_total; }
                    DWS_TRY(launch_fftconv(l->log2m, fa, s));
                    if (pg) DWS_TRY(kernel_backward(l, st->dh.f(), s));
                    if (pg && !rs_fused) DWS_TRY(launch_rowsum_bc(st->du.f(), dpt.f() + l->pt_off, pt_total, nB, H, Ls, s));
                }
                // u = LN1(x) + fc_t(e): dx = dx1 + LN'(du)
                DWS_TRY(launch_ln_bwd(x, st->du.f(), P(p + ".norm1.m"), P(p + ".norm1.s"), st->dx1.f(), din, written[e.in_node],
                                      pg ? ln_slot() : nullptr, nB, H, Ls, s));
                if (pg) DWS_TRY(ln_scalars(p + ".norm1", nblk, s));
                written[e.in_node] = 1;
            } else if (l->kind == L_DOWN) {
                const int K = l->H * l->p, O = l->Hout;
                if (pg) { const std::string wn_ = p + ".linear.conv"; DWS_TRY(wgrad(dy, l->t_xr.f(), O, K, l->Lout, 0, dWfold.f(), G(p + ".linear.conv.bias"), s, &wn_)); }
                DWS_TRY(gemm(l->tApT.f(), K, O, dy, pool_scr.f(), l->Lout, 2, nullptr, nullptr, nullptr, nullptr, nullptr, s));
                DWS_TRY(launch_pool_rearrange(pool_scr.f(), din, nullptr, 1, written[e.in_node], nB, l->H, l->p, l->Lout, s));
                written[e.in_node] = 1;
            } else {
                const int K = l->H, O = l->Hout * l->p;   // xl = Wp x + b, [B][O][L_in]
                DWS_TRY(launch_pool_rearrange(dy, pool_scr.f(), nullptr, 0, 0, nB, l->Hout, l->p, l->L, s));
                if (pg) { const std::string wn_ = p + ".linear.conv"; DWS_TRY(wgrad(pool_scr.f(), x, O, K, l->L, 0, dWfold.f(), G(p + ".linear.conv.bias"), s, &wn_)); }
                if (written[e.in_node])
                    DWS_TRY(gemm(l->tApT.f(), K, O, pool_scr.f(), din, l->L, 0, nullptr, nullptr, nullptr, din, nullptr, s));
                else
                    DWS_TRY(gemm(l->tApT.f(), K, O, pool_scr.f(), din, l->L, 2, nullptr, nullptr, nullptr, nullptr, nullptr, s));
                written[e.in_node] = 1;
            }
            if (e.add_node >= 0) {  // the skip connection receives the same gradient
                // The up path runs first in backward, so the skip node has no gradient yet: instead of COPYING dy into its buffer
                // (15 copies of up to 262 MB per C5 step, 1.5 ms) the node ADOPTS this layer's dy buffer -- everything of this
                // layer that reads dy is already enqueued, and the node's own consumer accumulates into it in place later.
                static const bool copy_skip = getenv("DWS_SKIP_GRAD_COPY") != nullptr;      // same-box A/B switch
                if (!written[e.add_node] && !copy_skip && node_numel(e.add_node) == node_numel(i + 1)) {
                    gp[e.add_node] = const_cast<float*>(dy);
                } else {
                    DWS_TRY(launch_add_into(dy, gp[e.add_node], written[e.add_node], node_numel(e.add_node), s));
                }
                written[e.add_node] = 1;
            }
            if (pg) DWS_TRY(grad_point(s));   // staged hand-over: buckets whose last gradient this layer produced leave now
        }

        // ---- init_conv: x0 = relu(Wi audio + bi)
        const size_t nact = (size_t)B * D * L;
        DWS_CHECK(written[0], DWS_ERR_STATE, "backward: no gradient reached the init conv");
        if (!pg) {   // the ReLU gate rides on the data adjoint: the masked gradient is never written
            DWS_TRY(launch_init_conv_bwd_data(gp[0], x_init.f(), Wi.f(), daudio, nB, Cin, D, nL, s));
            DWS_HIP(hipGetLastError());
            return DWS_OK;
        }
        DWS_TRY(launch_relu_bwd(gp[0], x_init.f(), nact, s));      // (node 0 is a skip node too: its gradient may live in an adopted buffer)
        { const std::string wn_ = "init_conv.0.conv"; DWS_TRY(wgrad(gp[0], train_audio, D, Cin, nL, 0, dWfold.f(), G("init_conv.0.conv.bias"), s, &wn_)); }
        if (daudio) DWS_TRY(launch_init_conv_bwd_data(gp[0], nullptr, Wi.f(), daudio, nB, Cin, D, nL, s));

        // ---- step embedding: per-block fc_t (stacked), then the shared swish MLP
        DWS_TRY(launch_lin_bwd_w(dpt.f(), h2.f(), dWt_all.f(), dbt_all.f(), nB, Eout, pt_total, s));
        unstack_fc_t.begin();
        for (auto* l : all) {
            if (l->kind != L_BLOCK) continue;
            unstack_fc_t.add(dWt_all.f() + (size_t)l->pt_off * Eout, G(l->prefix + ".fc_t.weight"), (size_t)l->H * Eout);
            unstack_fc_t.add(dbt_all.f() + l->pt_off, G(l->prefix + ".fc_t.bias"), (size_t)l->H);
        }
        DWS_TRY(unstack_fc_t.run(s));
        // with classes also d e itself (before the swish factor), whose per-class sums are the label table's gradient
        if (n_classes > 0) DWS_TRY(de_raw.ensure((size_t)B * Eout * 4));
        DWS_TRY(launch_lin_bwd_x(dpt.f(), Wt_all.f(), ta2.f(), dh2.f(), nB, Eout, pt_total, lin_scratch, s,
                                 n_classes > 0 ? de_raw.f() : nullptr));
        if (n_classes > 0) DWS_TRY(launch_label_grad(de_raw.f(), labels_ptr(), G(label_param), nB, n_classes, Eout, s));
        DWS_TRY(launch_lin_bwd_w(dh2.f(), h1.f(), G("fc_t2.weight"), G("fc_t2.bias"), nB, Emid, Eout, s));
        DWS_TRY(launch_lin_bwd_x(dh2.f(), P("fc_t2.weight"), ta1.f(), dh1.f(), nB, Emid, Eout, lin_scratch, s));
        DWS_TRY(launch_lin_bwd_w(dh1.f(), emb.f(), G("fc_t1.weight"), G("fc_t1.bias"), nB, Ein, Emid, s));
        DWS_TRY(ln_scalars_flush(s));
        DWS_HIP(hipGetLastError());
        return DWS_OK;
    }

    int read_tap(const char* tap, float* dst, int64_t capacity, hipStream_t s) override {
        DWS_CHECK(B > 0, DWS_ERR_STATE, "read_tap before prepare/forward");
        const std::string t(tap);
        if (t == "split_launches") {   // [block tails of the last forward that ran a split instance, those that ran exact-f32 kernels]
            DWS_CHECK(capacity >= 2, DWS_ERR_INVALID, "tap buffer too small");     // (the pooling GEMMs are exact f32 under every precision)
            const float v[2] = {(float)n_tail_split, (float)n_tail_f32};
            DWS_HIP(hipMemcpyAsync(dst, v, 8, hipMemcpyHostToDevice, s));
            DWS_HIP(hipStreamSynchronize(s));
            return DWS_OK;
        }
        if (t == "pre_final") {
            DWS_CHECK(last_x, DWS_ERR_STATE, "read_tap before forward");
            DWS_CHECK(capacity >= B * D * L, DWS_ERR_INVALID, "tap buffer too small");
            DWS_TRY(scratch_out.ensure((size_t)B * Cout * L * 4));
            return final_stage(last_x, scratch_out.f(), dst, s);
        }
        // function-level taps: the step embedding, the embedding MLP's output and the stacked
        // fc_t rows of the last per-clip forward; the network's final TransposedLayerNorm (`sashimi.py:309`)
        struct { const char* name; const DevBuf* buf; size_t n; } small[] = {
            {"emb", &emb, (size_t)B * Ein}, {"emb_mlp", &h2, (size_t)B * Eout}, {"part_t", &part_t, (size_t)B * pt_total},
            {"nfin", &nfin, last_x ? (size_t)B * D * L : 0}};
        for (auto& e : small)
            if (t == e.name) {
                DWS_CHECK(e.buf->p && e.n > 0 && capacity >= (int64_t)e.n, DWS_ERR_INVALID, "tap '%s': %zu floats, capacity %lld",
                          tap, e.n, (long long)capacity);
                DWS_HIP(hipMemcpyAsync(dst, e.buf->p, e.n * 4, hipMemcpyDeviceToDevice, s));
                return DWS_OK;
            }
        // the conditioner as set_condition left it: "melc:<block prefix>" = that block's [Bm][H][L_stage],
        // "mel_u0" / "mel_u1" = the upsampled mels of the block processed LAST (the scratch is shared)
        if (t == "mel_u0" || t == "mel_u1") {
            DWS_CHECK(melBm > 0, DWS_ERR_STATE, "tap '%s' before a set_condition with a mel", tap);
            const int T0 = mel_upsampled_len(mel_T, d.mel_upsample[0]), T1 = mel_upsampled_len(T0, d.mel_upsample[1]);
            const DevBuf& src = t == "mel_u0" ? mel_u0 : mel_u1;
            const size_t n = (size_t)melBm * MB * (t == "mel_u0" ? T0 : T1);
            DWS_CHECK(src.p && capacity >= (int64_t)n, DWS_ERR_INVALID, "tap '%s': %zu floats, capacity %lld", tap, n,
                      (long long)capacity);
            DWS_HIP(hipMemcpyAsync(dst, src.p, n * 4, hipMemcpyDeviceToDevice, s));
            return DWS_OK;
        }
        if (t.rfind("melc:", 0) == 0) {
            DWS_CHECK(melBm > 0, DWS_ERR_STATE, "tap '%s' before a set_condition with a mel", tap);
            for (auto* l : all)
                if (l->kind == L_BLOCK && l->prefix == t.substr(5)) {
                    const size_t n = (size_t)melBm * l->H * l->L;
                    DWS_CHECK(l->melc.p && capacity >= (int64_t)n, DWS_ERR_INVALID, "tap '%s': %zu floats, capacity %lld", tap, n,
                              (long long)capacity);
                    DWS_HIP(hipMemcpyAsync(dst, l->melc.p, n * 4, hipMemcpyDeviceToDevice, s));
                    return DWS_OK;
                }
        }
        if (t.rfind("k:", 0) == 0) {  // S4 kernel of the block with this prefix: L * k, k = [2][H][L] (s4.py:796-805)
            if (dirty) DWS_TRY(commit(s));
            for (auto* l : all)
                if (l->kind == L_BLOCK && l->prefix == t.substr(2)) {
                    S4Chain c;      // regenerates the (unnormalised) time-domain kernel into scratch; nothing of the commit moves
                    DWS_TRY(block_chain(l, c, s));
                    DWS_TRY(s4_taps_forward(*this, c, S4_NOT_KEPT, s));
                    const size_t n = (size_t)2 * l->H * l->Lk;
                    DWS_CHECK((size_t)capacity >= n, DWS_ERR_INVALID, "tap buffer too small");
                    DWS_HIP(hipMemcpyAsync(dst, ck.p, n * 4, hipMemcpyDeviceToDevice, s));
                    return DWS_OK;
                }
        }
        if (t.rfind("out:", 0) == 0) {  // output activation of the layer with this prefix
            for (auto* l : all)
                if (l->prefix == t.substr(4)) {
                    const size_t n = (l->kind == L_BLOCK) ? (size_t)B * l->H * l->L : (size_t)B * l->Hout * l->Lout;
                    DWS_CHECK((size_t)capacity >= n, DWS_ERR_INVALID, "tap buffer too small");
                    DWS_HIP(hipMemcpyAsync(dst, l->out.p, n * 4, hipMemcpyDeviceToDevice, s));
                    return DWS_OK;
                }
        }
        return set_error(DWS_ERR_INVALID, "unknown tap '%s'", tap);
    }
};

dws_model* make_sashimi(const dws_model_desc& d) {
    if (d.d_model <= 0 || d.n_layers <= 0 || d.n_pool < 0 || d.n_pool > DWS_MAX_POOL || d.expand <= 0 || d.ff <= 0 ||
        d.L <= 0) {
        set_error(DWS_ERR_INVALID, "sashimi: bad d_model/n_layers/pool/expand/ff/L");
        return nullptr;
    }
    int L = d.L;
    for (int i = 0; i < d.n_pool; ++i) {
        if (d.pool[i] <= 0 || L % d.pool[i] != 0) {
            set_error(DWS_ERR_INVALID, "sashimi: L=%d is not divisible by the pooling factors", d.L);
            return nullptr;
        }
        L /= d.pool[i];
    }
    return new SashimiModel(d);
}

}  // namespace dws
