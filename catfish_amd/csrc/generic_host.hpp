// Host side of the any-size inference path (generic.hpp): weight folding / tiling, workspace, launch sequence.
// Included by catfish_hip.hip after cf_model, fail(), HIP_TRY, prof_begin / prof_end.
#pragma once

// W(in, out) accessor (a term, catfish_hip.hip "weight packing") -> A pack emitted into sink e with constant c; inputs in >= k_real
// are zero padding
template <typename E, typename F>
static void gen_pack_a(E& e, size_t off, F w, int k_real, int K16, int M16, int c) {
    for (int mo = 0; mo < M16; ++mo)
        for (int kb = 0; kb < K16; ++kb)
            for (int lane = 0; lane < 64; ++lane)
                for (int i = 0; i < 4; ++i) {
                    const int in = 16 * kb + 4 * (lane >> 4) + i, out = 16 * mo + (lane & 15);
                    e(off + (((size_t)mo * K16 + kb) * 64 + lane) * 4 + i, in < k_real ? cf_scaled(w(in, out), c) : cf_zero());
                }
}

// per-output vector (bias, dense weights; v(o) a term) in accumulator order: [mo][lane][j] = v[16 mo + 4 (lane >> 4) + j] x constant c
template <typename E, typename F>
static void gen_pack_v(E& e, size_t off, F v, int M16, int c) {
    for (int mo = 0; mo < M16; ++mo)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 4; ++j) e(off + ((size_t)mo * 64 + lane) * 4 + j, cf_scaled(v(16 * mo + 4 * (lane >> 4) + j), c));
}

static bool gen_forced() { return cf_knob("CATFISH_GENERIC") && atoi(cf_knob("CATFISH_GENERIC")) != 0; }     // A/B and test knob, read per model

// (the tuned kernels have no bf16x3 form of the plain RNN type: it runs here in that precision)
static bool gen_wanted(const cf_hparams* hp) {
    return gen_forced() || hp->layer_size != CF_H || (hp->n_layers_res > 0 && hp->layer_size_res != CF_C) ||
           (hp->n_layers_res == 0 && hp->precision == CF_PREC_BF16X3);
}

static void gen_destroy(cf_generic* g) {
    if (!g) return;
    for (void* p : g->owned) (void)hipFree(p);
    delete g;
}

static int gen_upload(cf_generic* g, const std::vector<float>& host, f32x4** dev) {
    float* p = nullptr;
    HIP_TRY(hipMalloc((void**)&p, host.size() * sizeof(float)));
    g->owned.push_back(p);
    HIP_TRY(hipMemcpy(p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    *dev = reinterpret_cast<f32x4*>(p);
    return CF_OK;
}

// The fp32 packs of the any-size path, one per device buffer (the bf16x3 weight matrices: gen_pack_a_x3 on host values).
// cf_model_create evaluates them into host blobs, cf_model_load_params records them as its gather map (params_dev.hpp).
template <class E>
static void gen_pack_first(E& e, const ConvTerms& sc, const ConvTerms& f1, int C16) {      // block 0's cin-1 units: [w_sc, b_sc, w_1, b_1]
    gen_pack_v(e, (size_t)0 * C16 * 256, [&](int o) { return sc.w(0, 0, o); }, C16, CF_K_ONE);
    gen_pack_v(e, (size_t)1 * C16 * 256, [&](int o) { return sc.b(o); }, C16, CF_K_ONE);
    gen_pack_v(e, (size_t)2 * C16 * 256, [&](int o) { return f1.w(0, 0, o); }, C16, CF_K_ONE);
    gen_pack_v(e, (size_t)3 * C16 * 256, [&](int o) { return f1.b(o); }, C16, CF_K_ONE);
}
template <class E>
static void gen_pack_conv_w(E& e, const ConvTerms& f) {                                    // [taps][Co16][Ki16][64] f32x4
    const int K16 = f.cin / 16, M16 = f.cout / 16;
    for (int tap = 0; tap < f.k; ++tap)
        gen_pack_a(e, (size_t)tap * M16 * K16 * 256, [&](int in, int out) { return f.w(tap, in, out); }, f.cin, K16, M16, CF_K_ONE);
}
template <class E>
static void gen_pack_conv_b(E& e, const ConvTerms& f) { gen_pack_v(e, 0, [&](int o) { return f.b(o); }, f.cout / 16, CF_K_ONE); }

// biGRU weight of gate 0 = r, 1 = u (gates kernel columns [0, H) and [H, 2H)), 2 = candidate over K = [x blocks (kbx_w) | h blocks]
static cf_term gen_gru_w(const GruTerms& g, int gate, int in, int out, int cin_real, int kbx_w) {
    const int H = g.h, col0 = gate == 1 ? H : 0;
    auto k = [&](int row) { return gate < 2 ? g.gk(row, col0 + out) : g.ck(row, out); };
    if (in < 16 * kbx_w) return in < cin_real ? k(in) : cf_zero();
    return in - 16 * kbx_w < H ? k(cin_real + in - 16 * kbx_w) : cf_zero();
}
static int gen_gru_c(int gate) { return gate < 2 ? CF_K_GATE : CF_K_CAND; }
template <class E>
static void gen_pack_gru_w(E& e, const cf_hparams& hp, int l, int cin_real, int H16) {      // [2 dirs][3 gates][H16][KB][64] (fp32)
    const int kbx = (cin_real + 15) / 16, KB = kbx + H16;
    const size_t mat = (size_t)H16 * KB * 256;
    for (int d = 0; d < 2; ++d) {
        const GruTerms g = gru_terms(cf_tid_gru(hp.n_layers_res, l, d, 0), hp.layer_size);
        for (int gate = 0; gate < 3; ++gate)
            gen_pack_a(e, (size_t)(d * 3 + gate) * mat, [&](int in, int out) { return gen_gru_w(g, gate, in, out, cin_real, kbx); }, 16 * KB, KB,
                       H16, gen_gru_c(gate));
    }
}
template <class E>
static void gen_pack_gru_b(E& e, const cf_hparams& hp, int l, int H16) {                   // [2][3][H16][64]
    const int H = hp.layer_size;
    for (int d = 0; d < 2; ++d) {
        const GruTerms g = gru_terms(cf_tid_gru(hp.n_layers_res, l, d, 0), H);
        for (int gate = 0; gate < 3; ++gate)
            gen_pack_v(e, (size_t)(d * 3 + gate) * H16 * 256, [&](int o) { return gate < 2 ? g.gb((gate == 1 ? H : 0) + o) : g.cb(o); }, H16,
                       gen_gru_c(gate));
    }
}
template <class E>
static void gen_pack_gru_tuned(E& e, const cf_hparams& hp, int l, int cin_real) {           // [2][gru_pack_floats(cin_real)]
    for (int d = 0; d < 2; ++d)
        pack_gru_dir(e, (size_t)d * gru_pack_floats(cin_real), gru_terms(cf_tid_gru(hp.n_layers_res, l, d, 0), CF_H), cin_real, cin_real, -1, 0);
}
template <class E>
static void gen_pack_dense(E& e, const cf_hparams& hp, int H16) {
    const int t = cf_tid_dense(hp.n_layers_res, hp.n_layers, 0);
    gen_pack_v(e, 0, [&](int f) { return cf_raw(t, f); }, 2 * H16, CF_K_ONE);
}
// a 64-unit layer with 16, 32 or 128 inputs runs on the LDS-resident tuned kernel (see gen_build)
static bool gen_layer_tuned(const cf_generic* g, const cf_hparams& hp, int cin_real) {
    return hp.layer_size == CF_H && !gen_forced() && !g->x3 && (cin_real == 16 || cin_real == 32 || cin_real == 128);
}

static int gen_upload_terms(cf_generic* g, size_t n, const cf_host_params& P, f32x4** dev, const std::function<void(HostSink&)>& pack) {
    std::vector<float> host(n, 0.f);
    HostSink e{P, host.data()};
    pack(e);
    return gen_upload(g, host, dev);
}

static int gen_build(cf_model* m, const cf_weights* w) {
    const cf_hparams& hp = m->hp;
    const int H = hp.layer_size, C = hp.n_layers_res > 0 ? hp.layer_size_res : 0;
    if (H < 16 || H > 256 || (H % 16) != 0)
        return fail(CF_ERR_INVALID, "layer_size must be a multiple of 16 between 16 and 256 (the reference draws 16, 32, 64, 128, 256)");
    if (hp.n_layers_res > 0 && (C < 16 || C > 256 || (C % 16) != 0))
        return fail(CF_ERR_INVALID, "layer_size_res must be a multiple of 16 between 16 and 256 (the reference draws 16, 32, 64, 128, 256)");
    if (hp.precision != CF_PREC_FP32 && hp.precision != CF_PREC_BF16X3)
        return fail(CF_ERR_INVALID, "the bf16 kernels are built for layer_size = 64 and layer_size_res = 32 only; other sizes run in CF_PREC_FP32 or CF_PREC_BF16X3");
    cf_generic* g = new cf_generic();
    m->gen = g;
    g->x3 = hp.precision == CF_PREC_BF16X3;
    g->H16 = H / 16;
    g->C16 = C / 16;
    int rc = CF_OK;
    const cf_host_params P = host_params(w, hp, C);
    // residual blocks (resnet_class.py:44-82): conv order per block = shortcut, first, middle (k = 3), last
    for (int b = 0; b < hp.n_layers_res && rc == CF_OK; ++b) {
        const cf_conv_bn* c4 = w->conv + 4 * b;
        const int cin = b == 0 ? 1 : C;
        if (c4[0].ksize != 1 || c4[1].ksize != 1 || c4[2].ksize != 3 || c4[3].ksize != 1 || c4[0].cin != cin || c4[1].cin != cin ||
            c4[2].cin != C || c4[3].cin != C)
            return fail(CF_ERR_INVALID, "residual block geometry not supported (need k = 1,1,3,1)");
        const ConvTerms sc = unit_terms(hp, 4 * b), f1 = unit_terms(hp, 4 * b + 1), f3 = unit_terms(hp, 4 * b + 2), fl = unit_terms(hp, 4 * b + 3);
        auto conv = [&](const ConvTerms& f, f32x4** w_dev, f32x4** b_dev) {
            int r;
            if (g->x3) {
                const int K16 = gen_x3_pad(f.cin / 16), M16 = f.cout / 16;
                std::vector<float> wp((size_t)f.k * M16 * K16 * 256);
                for (int tap = 0; tap < f.k; ++tap)
                    gen_pack_a_x3(wp, (size_t)tap * M16 * K16 * 256, [&](int in, int out) { return in < f.cin ? P.base(f.w(tap, in, out)) : 0.0; },
                                  K16, M16, 1.0);
                r = gen_upload(g, wp, w_dev);
            } else {
                r = gen_upload_terms(g, (size_t)f.k * (f.cout / 16) * (f.cin / 16) * 256, P, w_dev, [&](HostSink& e) { gen_pack_conv_w(e, f); });
            }
            return r != CF_OK ? r : gen_upload_terms(g, (size_t)(f.cout / 16) * 256, P, b_dev, [&](HostSink& e) { gen_pack_conv_b(e, f); });
        };
        cf_generic::Block blk;
        if (b == 0) {
            rc = gen_upload_terms(g, (size_t)4 * g->C16 * 256, P, &blk.first, [&](HostSink& e) { gen_pack_first(e, sc, f1, g->C16); });
        } else {
            rc = conv(sc, &blk.w_sc, &blk.b_sc);
            if (rc == CF_OK) rc = conv(f1, &blk.w_1, &blk.b_1);
        }
        if (rc == CF_OK) rc = conv(f3, &blk.w_3, &blk.b_3);
        if (rc == CF_OK) rc = conv(fl, &blk.w_l, &blk.b_l);
        g->blocks.push_back(blk);
    }
    // biGRU layers: per direction three matrices over K = [x blocks | h blocks]
    for (int l = 0; l < hp.n_layers && rc == CF_OK; ++l) {
        const int cin_real = l == 0 ? (C > 0 ? C : 1) : 2 * H;
        const int kbx = (cin_real + 15) / 16;
        const int kbx_w = g->x3 ? gen_x3_pad(kbx) : kbx, KB = kbx_w + (g->x3 ? gen_x3_pad(g->H16) : g->H16);    // weight blocks: [x | h]
        if (w->gru[2 * l].cin != cin_real || w->gru[2 * l + 1].cin != cin_real) return fail(CF_ERR_INVALID, "GRU layer input width mismatch");
        const size_t mat = (size_t)g->H16 * KB * 256, vec = (size_t)g->H16 * 256;
        cf_generic::Layer L;
        L.kbx = kbx;
        if (g->x3) {
            std::vector<float> wp(2 * 3 * mat);
            for (int d = 0; d < 2; ++d) {
                const GruTerms gd = gru_terms(cf_tid_gru(hp.n_layers_res, l, d, 0), H);
                for (int gate = 0; gate < 3; ++gate)
                    gen_pack_a_x3(wp, (size_t)(d * 3 + gate) * mat, [&](int in, int out) { return P.base(gen_gru_w(gd, gate, in, out, cin_real, kbx_w)); },
                                  KB, g->H16, cf_term_const(gen_gru_c(gate)));
            }
            rc = gen_upload(g, wp, &L.w);
        } else {
            rc = gen_upload_terms(g, 2 * 3 * mat, P, &L.w, [&](HostSink& e) { gen_pack_gru_w(e, hp, l, cin_real, g->H16); });
        }
        if (rc == CF_OK) rc = gen_upload_terms(g, 2 * 3 * vec, P, &L.b, [&](HostSink& e) { gen_pack_gru_b(e, hp, l, g->H16); });
        // 64 units with 16, 32 or 128 input features is what gru_layer_kernel<CIN, false> (weights in LDS, state in registers,
        // 0.78-0.83 of the fp32-MFMA peak) is built for: such layers of an otherwise odd geometry (say 64 units behind 128
        // conv channels) run on it.  Not when CATFISH_GENERIC forces this path: that knob exists to exercise the kernels here.
        // Not in bf16x3 either: the tuned bf16x3 kernels keep their activations in another layout.
        if (rc == CF_OK && gen_layer_tuned(g, hp, cin_real)) {
            f32x4* dev = nullptr;
            rc = gen_upload_terms(g, (size_t)2 * gru_pack_floats(cin_real), P, &dev, [&](HostSink& e) { gen_pack_gru_tuned(e, hp, l, cin_real); });
            L.tuned = reinterpret_cast<float*>(dev);
            L.tuned_cin = cin_real;
        }
        g->layers.push_back(L);
    }
    if (rc == CF_OK) rc = gen_upload_terms(g, (size_t)2 * g->H16 * 256, P, &g->dense, [&](HostSink& e) { gen_pack_dense(e, hp, g->H16); });
    if (rc != CF_OK) return rc;
    // workspace: four conv buffers (input / shortcut / two intermediates), two biGRU output buffers
    int64_t cap = hp.max_windows_per_pass > 0 ? hp.max_windows_per_pass : 32768;
    cap = (cap + CF_TILE - 1) / CF_TILE * CF_TILE;
    m->cap_windows = cap;
    m->cap_tiles = cap / CF_TILE;
    // (+ 16 tiles: the biGRU launch is whole workgroups of up to sixteen tiles; the waves past the last tile own scratch tiles)
    const size_t per_f16 = (size_t)(m->cap_tiles + 16) * CF_T * 64 * sizeof(f32x4);    // bytes of one 16-feature tile plane
    const size_t r_bytes = per_f16 * std::max(1, g->C16), g_bytes = per_f16 * 2 * g->H16;
    const int n_r = g->C16 > 0 ? 4 : 1;
    for (int i = 0; i < n_r; ++i) {
        hipError_t e = hipMalloc((void**)&g->r[i], r_bytes);
        if (e != hipSuccess) return fail(CF_ERR_NOMEM, std::string("workspace allocation: ") + hipGetErrorString(e));
        g->owned.push_back(g->r[i]);
    }
    for (int i = 0; i < 2; ++i) {
        hipError_t e = hipMalloc((void**)&g->g[i], g_bytes);
        if (e != hipSuccess) return fail(CF_ERR_NOMEM, std::string("workspace allocation: ") + hipGetErrorString(e));
        g->owned.push_back(g->g[i]);
    }
    m->ws_bytes = (int64_t)(n_r * r_bytes + 2 * g_bytes);
    // biGRU launch class (csrc/anysize_infer_launch.hpp): the state of a tile takes 3 H 64 B of LDS (h, r.h and h'); as many
    // waves per workgroup as fit (8 at most); when eight waves of that do not fit, h' goes through the output buffer instead
    // (two arrays) and the workgroup is 8 or 4 waves, so that every SIMD carries the same number.  Two tiles per wave
    // (gen_gru2_kernel): two LDS arrays per tile; 8 or 4 waves per workgroup, else not used.  The two knobs are for tools/.
    g->cls = cf_anysize_infer_class_for(g->H16, g->x3, cf_knob("CATFISH_GEN_ONE_TILE") != nullptr,
                                        cf_knob("CATFISH_GEN_WAVES") ? std::max(1, atoi(cf_knob("CATFISH_GEN_WAVES"))) : 0);
    if (g->cls.gru2_waves)
        HIP_TRY(hipFuncSetAttribute((const void*)gen_gru2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g->cls.gru2_lds));
    HIP_TRY(hipFuncSetAttribute(g->x3 ? (const void*)gen_gru_kernel<false, true> : (const void*)gen_gru_kernel<false, false>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)g->cls.gru_lds));
    cf_optin tuned;              // the LDS-resident kernels of gen_layer_tuned layers: the same opt-in as a model on the tuned path
    optin_gru_layer(tuned);
    HIP_TRY(tuned.e);
    return CF_OK;
}

static int gen_run_pass(cf_model* m, const float* x, int64_t n_windows, float* probs, float* logits, hipStream_t s) {
    cf_generic* g = m->gen;
    const int n_tiles = (int)((n_windows + CF_TILE - 1) / CF_TILE);
    const int task_grid = (int)std::min<int64_t>(((int64_t)n_tiles * CF_T + 3) / 4, (int64_t)m->n_cu * 16);
    const cf_knobs knobs = cf_read_knobs();
    int rc;
    size_t pi = 0;
    f32x4* R[4];
    for (int i = 0; i < 4; ++i) R[i] = reinterpret_cast<f32x4*>(g->r[i]);
    f32x4* G[2] = {reinterpret_cast<f32x4*>(g->g[0]), reinterpret_cast<f32x4*>(g->g[1])};
    auto conv = [&](const f32x4* wv, const f32x4* bv, const f32x4* in, const f32x4* res, f32x4* out, int taps, int relu, int slot) -> int {
        int r2;
        if ((r2 = prof_begin(m, slot, s, &pi)) != CF_OK) return r2;
        hipLaunchKernelGGL(g->x3 ? gen_conv_kernel<true> : gen_conv_kernel<false>, dim3(task_grid), dim3(256), 0, s, wv, bv, in, res, out, n_tiles,
                           g->C16, g->C16, taps, relu);
        HIP_TRY(hipGetLastError());
        return prof_end(m, s, pi);
    };
    const f32x4* cur = R[0];
    if (g->C16 > 0) {
        for (size_t b = 0; b < g->blocks.size(); ++b) {
            const cf_generic::Block& k = g->blocks[b];
            const int slot = b == 0 ? SLOT_RES_FIRST : SLOT_RES;
            if (b == 0) {
                if ((rc = prof_begin(m, slot, s, &pi)) != CF_OK) return rc;
                const int64_t n_el = (int64_t)n_tiles * CF_T * g->C16 * 64;
                hipLaunchKernelGGL(gen_first_kernel, dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, s, x, k.first, R[1], R[2], n_windows,
                                   n_tiles, g->C16);
                HIP_TRY(hipGetLastError());
                if ((rc = prof_end(m, s, pi)) != CF_OK) return rc;
            } else {
                if ((rc = conv(k.w_sc, k.b_sc, R[0], nullptr, R[1], 1, 0, slot)) != CF_OK) return rc;       // shortcut: BN(conv1), no relu
                if ((rc = conv(k.w_1, k.b_1, R[0], nullptr, R[2], 1, 1, slot)) != CF_OK) return rc;
            }
            if ((rc = conv(k.w_3, k.b_3, R[2], nullptr, R[3], 3, 1, slot)) != CF_OK) return rc;
            if ((rc = conv(k.w_l, k.b_l, R[3], R[1], R[0], 1, 3, slot)) != CF_OK) return rc;                // relu(relu(BN(conv1)) + shortcut)
        }
    } else {
        // RNN type: the raw sample as feature 0 of a 16-feature tile (the x rows of the first layer are zero-padded to 16)
        if ((rc = prof_begin(m, SLOT_RES_FIRST, s, &pi)) != CF_OK) return rc;
        const int64_t n_el = (int64_t)n_tiles * CF_T * 64;
        hipLaunchKernelGGL(embed_kernel, dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, s, x, R[0], n_windows, n_tiles);
        HIP_TRY(hipGetLastError());
        if ((rc = prof_end(m, s, pi)) != CF_OK) return rc;
    }
    for (size_t l = 0; l < g->layers.size(); ++l) {
        const cf_generic::Layer& L = g->layers[l];
        const int slot = l == 0 ? SLOT_GRU0 : (l + 1 == g->layers.size() ? SLOT_GRU_LAST : SLOT_GRU);
        const cf_anysize_infer_launch sh = cf_anysize_infer_shape_for(g->cls, L.tuned != nullptr, L.kbx, n_tiles, m->n_cu);
        if (sh.kernel == CF_ANYSIZE_INFER_TUNED) {      // a 64-unit layer with 16 / 32 / 128 inputs: the LDS-resident kernel (all its launch regimes)
            const float* x_in = reinterpret_cast<const float*>(cur);
            float* y_out = reinterpret_cast<float*>(G[l & 1]);
            if ((rc = launch_gru(m, knobs, L.tuned_cin, false, L.tuned, x_in, y_out, nullptr, n_tiles, s, slot)) != CF_OK) return rc;
            cur = G[l & 1];
            continue;
        }
        if ((rc = prof_begin(m, slot, s, &pi)) != CF_OK) return rc;
        if (sh.kernel == CF_ANYSIZE_INFER_TWO_TILE) {
            hipLaunchKernelGGL(gen_gru2_kernel, dim3((unsigned)sh.grid_x, 2), dim3(sh.waves * 64), sh.lds_bytes, s,
                               L.w, L.b, cur, G[l & 1], g->H16, L.kbx);
            HIP_TRY(hipGetLastError());
            if ((rc = prof_end(m, s, pi)) != CF_OK) return rc;
            cur = G[l & 1];
            continue;
        }
        hipLaunchKernelGGL((g->x3 ? gen_gru_kernel<false, true> : gen_gru_kernel<false, false>), dim3((unsigned)sh.grid_x, 2), dim3(sh.waves * 64),
                           sh.lds_bytes, s, L.w, L.b, cur, G[l & 1], g->H16, L.kbx, sh.h_via_y, (f32x4*)nullptr, n_tiles);
        HIP_TRY(hipGetLastError());
        if ((rc = prof_end(m, s, pi)) != CF_OK) return rc;
        cur = G[l & 1];
    }
    if ((rc = prof_begin(m, SLOT_HEAD, s, &pi)) != CF_OK) return rc;
    hipLaunchKernelGGL(gen_head_kernel, dim3(task_grid), dim3(256), 0, s, cur, g->dense, m->d_dense_bias, probs, logits, n_windows, n_tiles, 2 * g->H16);
    HIP_TRY(hipGetLastError());
    return prof_end(m, s, pi);
}
