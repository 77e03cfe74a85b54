// cf_model_param_floats / cf_model_load_params (C ABI 9): new weights for an existing fp32 model, from a device flat parameter
// vector in the operator's order (torch_ops.tensor_names, TF layouts, flattened: packed_weights without its header).
//
// The packers of catfish_hip.hip / generic_host.hpp emit every packed element as a term (see "weight packing" there).  The first
// load walks the model's weight buffers in the order cf_model_create filled them, runs the same packers with a recording sink and
// uploads the result as a gather map of 8 bytes per packed float:
//     x = flat index of the term's parameter,   y = kind | constant << 2 | BN channel << 4
// Every load after that is two stream-ordered launches and nothing else (no allocation, no copy, no synchronisation: capturable):
//     cf_bn_fold_kernel     per BN channel s = gamma / sqrt(var + eps), b' = b s + beta - mean s      (double)
//     cf_load_params_kernel one thread per packed float: the term's value, written to its buffer     (coalesced map reads / writes)
// Both use cf_bn_scale / cf_bn_bias / cf_term_value, the functions cf_model_create evaluates on the host, with contraction off,
// so a loaded model computes the bits a freshly created one computes.
// Included by catfish_hip.hip after generic_host.hpp (needs cf_model, the packers, fail, HIP_TRY).
#pragma once

struct cf_pm_seg {                 // one weight buffer: map entries [start, start + count) -> dst[0, count)
    int64_t start, count;
    float* dst;
};

struct cf_param_map {
    void* dev = nullptr;           // one allocation: s, b [n_ch] (double) | map [n_map] | segs [n_segs] | block_seg [n_map / 256] | bias_src [n_ch]
    double* s = nullptr;
    double* b = nullptr;
    const uint2* map = nullptr;
    const cf_pm_seg* segs = nullptr;
    const int32_t* block_seg = nullptr;
    const int32_t* bias_src = nullptr;
    int64_t n_map = 0;             // a multiple of 256: every buffer starts on a workgroup boundary
    int n_ch = 0, C = 0;
};

static void pm_destroy(cf_param_map* pm) {
    if (!pm) return;
    if (pm->dev) (void)hipFree(pm->dev);
    delete pm;
}

__global__ __launch_bounds__(256) void cf_bn_fold_kernel(const float* __restrict__ p, const int32_t* __restrict__ bias_src, int n_ch, int C,
                                                         float eps, double* __restrict__ s, double* __restrict__ b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_ch) return;
    const int64_t j = bias_src[i];                 // a unit's vectors follow its kernel: bias, gamma, beta, moving_mean, moving_variance
    const double sc = cf_bn_scale(p[j + C], p[j + 4 * C], eps);
    s[i] = sc;
    b[i] = cf_bn_bias(p[j], p[j + 2 * C], p[j + 3 * C], sc);
}

__global__ __launch_bounds__(256) void cf_load_params_kernel(const float* __restrict__ p, const uint2* __restrict__ map,
                                                             const double* __restrict__ s, const double* __restrict__ b,
                                                             const cf_pm_seg* __restrict__ segs, const int32_t* __restrict__ block_seg) {
    const cf_pm_seg sg = segs[block_seg[blockIdx.x]];          // uniform: a workgroup never straddles two buffers
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t local = i - sg.start;
    if (local >= sg.count) return;
    const uint2 e = map[i];
    const int kind = (int)(e.y & 3u), c = (int)((e.y >> 2) & 3u), ch = (int)(e.y >> 4);
    const float v = (kind == CF_TERM_RAW || kind == CF_TERM_KERN) ? p[e.x] : 0.f;
    const double sc = kind == CF_TERM_KERN ? s[ch] : 0.0, bb = kind == CF_TERM_BIAS ? b[ch] : 0.0;
    sg.dst[local] = cf_term_value(kind, v, sc, bb, c);
}

// flat offset of every tensor id (cf_tid_*), plus the total at the end
static std::vector<int64_t> pm_tensor_offsets(const cf_hparams& hp) {
    const int64_t H = hp.layer_size, C = hp.n_layers_res > 0 ? hp.layer_size_res : 0;
    std::vector<int64_t> sizes;
    for (int u = 0; u < 4 * hp.n_layers_res; ++u) {
        const ConvTerms f = unit_terms(hp, u);
        sizes.push_back((int64_t)f.k * f.cin * C);
        for (int i = 0; i < 5; ++i) sizes.push_back(C);
    }
    for (int l = 0; l < hp.n_layers; ++l) {
        const int64_t rows = (l == 0 ? (C > 0 ? C : 1) : 2 * H) + H;
        for (int d = 0; d < 2; ++d) {
            sizes.push_back(rows * 2 * H); sizes.push_back(2 * H);
            sizes.push_back(rows * H); sizes.push_back(H);
        }
    }
    sizes.push_back(2 * H);
    sizes.push_back(1);
    std::vector<int64_t> off(sizes.size() + 1, 0);
    for (size_t i = 0; i < sizes.size(); ++i) off[i + 1] = off[i] + sizes[i];
    return off;
}

struct PmBuilder {
    const std::vector<int64_t>& toff;
    std::vector<uint2> map;
    std::vector<cf_pm_seg> segs;
    bool overflow = false;
    struct Sink {                  // records the terms of one buffer
        PmBuilder* B;
        int64_t base, count;
        void operator()(size_t i, const cf_term& t) const {
            if ((int64_t)i >= count) { B->overflow = true; return; }
            uint2 e;
            e.x = (t.kind == CF_TERM_RAW || t.kind == CF_TERM_KERN) ? (uint32_t)(B->toff[t.tensor] + t.elem) : 0u;
            e.y = (uint32_t)t.kind | ((uint32_t)t.c << 2) | ((uint32_t)t.ch << 4);
            B->map[(size_t)(base + (int64_t)i)] = e;
        }
    };
    Sink seg(void* dst, int64_t count) {
        const int64_t start = (int64_t)map.size();
        map.resize((size_t)(start + (count + 255) / 256 * 256), make_uint2(0u, 0u));       // {0, 0}: +0.0f, as the host blobs' fill
        segs.push_back({start, count, reinterpret_cast<float*>(dst)});
        return Sink{this, start, count};
    }
};

// the model's fp32 weight buffers in cf_model_create's order, each with the packer that filled it
static int pm_walk(cf_model* m, PmBuilder& B) {
    const cf_hparams& hp = m->hp;
    int rc = CF_OK;
    if (!m->gen) {
        for (int b = 0; b < hp.n_layers_res && rc == CF_OK; ++b) {
            ConvTerms c4[4];
            for (int u = 0; u < 4; ++u) c4[u] = unit_terms(hp, 4 * b + u);
            auto e = B.seg(m->d_res[b], res_pack_floats(b == 0));
            rc = pack_res_block(e, c4, b == 0);
        }
        for (int l = 0; l < hp.n_layers && rc == CF_OK; ++l) {
            const int cin_real = l == 0 ? (hp.n_layers_res > 0 ? CF_C : 1) : 2 * CF_H, cin = m->gru_cin[l];
            auto e = B.seg(m->d_gru[l], (int64_t)2 * gru_pack_floats(cin));
            for (int d = 0; d < 2; ++d)
                pack_gru_dir(e, (size_t)d * gru_pack_floats(cin), gru_terms(cf_tid_gru(hp.n_layers_res, l, d, 0), CF_H), cin, cin_real,
                             l == hp.n_layers - 1 ? cf_tid_dense(hp.n_layers_res, hp.n_layers, 0) : -1, d * CF_H);
        }
    } else {
        const cf_generic* g = m->gen;
        const int C16 = g->C16, H16 = g->H16;
        for (int b = 0; b < hp.n_layers_res; ++b) {
            const cf_generic::Block& k = g->blocks[b];
            const ConvTerms sc = unit_terms(hp, 4 * b), f1 = unit_terms(hp, 4 * b + 1), f3 = unit_terms(hp, 4 * b + 2), fl = unit_terms(hp, 4 * b + 3);
            auto conv = [&](const ConvTerms& f, f32x4* w, f32x4* bv) {
                auto ew = B.seg(w, (int64_t)f.k * (f.cout / 16) * (f.cin / 16) * 256);
                gen_pack_conv_w(ew, f);
                auto eb = B.seg(bv, (int64_t)(f.cout / 16) * 256);
                gen_pack_conv_b(eb, f);
            };
            if (b == 0) {
                auto e = B.seg(k.first, (int64_t)4 * C16 * 256);
                gen_pack_first(e, sc, f1, C16);
            } else {
                conv(sc, k.w_sc, k.b_sc);
                conv(f1, k.w_1, k.b_1);
            }
            conv(f3, k.w_3, k.b_3);
            conv(fl, k.w_l, k.b_l);
        }
        for (int l = 0; l < hp.n_layers; ++l) {
            const cf_generic::Layer& L = g->layers[l];
            const int cin_real = l == 0 ? (C16 > 0 ? hp.layer_size_res : 1) : 2 * hp.layer_size;
            auto ew = B.seg(L.w, (int64_t)2 * 3 * H16 * (L.kbx + H16) * 256);
            gen_pack_gru_w(ew, hp, l, cin_real, H16);
            auto eb = B.seg(L.b, (int64_t)2 * 3 * H16 * 256);
            gen_pack_gru_b(eb, hp, l, H16);
            if (L.tuned) {
                auto et = B.seg(L.tuned, (int64_t)2 * gru_pack_floats(L.tuned_cin));
                gen_pack_gru_tuned(et, hp, l, L.tuned_cin);
            }
        }
        auto e = B.seg(g->dense, (int64_t)2 * H16 * 256);
        gen_pack_dense(e, hp, H16);
    }
    if (rc != CF_OK) return rc;
    auto e = B.seg(m->d_dense_bias, 1);
    e(0, cf_raw(cf_tid_dense(hp.n_layers_res, hp.n_layers, 1), 0));
    return B.overflow ? fail(CF_ERR_INVALID, "cf_model_load_params: internal error: a packer wrote past its buffer") : CF_OK;
}

static int pm_build(cf_model* m) {
    const cf_hparams& hp = m->hp;
    const std::vector<int64_t> toff = pm_tensor_offsets(hp);
    if (toff.back() >= ((int64_t)1 << 31)) return fail(CF_ERR_INVALID, "cf_model_load_params: too many parameters for a 32-bit gather map");
    PmBuilder B{toff};
    int rc = pm_walk(m, B);
    if (rc != CF_OK) return rc;
    const int C = hp.n_layers_res > 0 ? hp.layer_size_res : 0, n_ch = 4 * hp.n_layers_res * C;
    if ((int64_t)n_ch >= ((int64_t)1 << 28)) return fail(CF_ERR_INVALID, "cf_model_load_params: too many BN channels");
    const int64_t n_map = (int64_t)B.map.size(), n_blocks = n_map / 256;
    std::vector<int32_t> block_seg((size_t)n_blocks), bias_src((size_t)n_ch);
    for (size_t k = 0; k < B.segs.size(); ++k)
        for (int64_t blk = B.segs[k].start / 256; blk < (B.segs[k].start + B.segs[k].count + 255) / 256; ++blk) block_seg[(size_t)blk] = (int32_t)k;
    for (int u = 0; u < 4 * hp.n_layers_res; ++u)
        for (int o = 0; o < C; ++o) bias_src[(size_t)u * C + o] = (int32_t)(toff[cf_tid_conv(u, 1)] + o);
    // one allocation, one upload: [s | b] doubles (written by cf_bn_fold_kernel), then map, segs, block_seg, bias_src
    const size_t sb_bytes = (size_t)2 * n_ch * sizeof(double), map_bytes = (size_t)n_map * sizeof(uint2);
    const size_t seg_bytes = B.segs.size() * sizeof(cf_pm_seg), bs_bytes = (size_t)n_blocks * sizeof(int32_t), src_bytes = (size_t)n_ch * sizeof(int32_t);
    std::vector<char> host(map_bytes + seg_bytes + bs_bytes + src_bytes);
    char* h = host.data();
    memcpy(h, B.map.data(), map_bytes);
    memcpy(h + map_bytes, B.segs.data(), seg_bytes);
    memcpy(h + map_bytes + seg_bytes, block_seg.data(), bs_bytes);
    if (src_bytes) memcpy(h + map_bytes + seg_bytes + bs_bytes, bias_src.data(), src_bytes);
    cf_param_map* pm = new cf_param_map();
    hipError_t e = hipMalloc(&pm->dev, sb_bytes + host.size());
    if (e == hipSuccess) e = hipMemcpy((char*)pm->dev + sb_bytes, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        pm_destroy(pm);
        return fail(CF_ERR_HIP, std::string("cf_model_load_params: gather map upload: ") + hipGetErrorString(e));
    }
    char* d = (char*)pm->dev;
    pm->s = reinterpret_cast<double*>(d);
    pm->b = pm->s + n_ch;
    pm->map = reinterpret_cast<const uint2*>(d + sb_bytes);
    pm->segs = reinterpret_cast<const cf_pm_seg*>(d + sb_bytes + map_bytes);
    pm->block_seg = reinterpret_cast<const int32_t*>(d + sb_bytes + map_bytes + seg_bytes);
    pm->bias_src = reinterpret_cast<const int32_t*>(d + sb_bytes + map_bytes + seg_bytes + bs_bytes);
    pm->n_map = n_map;
    pm->n_ch = n_ch;
    pm->C = C;
    m->pmap = pm;
    return CF_OK;
}

extern "C" int cf_model_param_floats(const cf_model* m, int64_t* n) {
    if (!m || !n) return fail(CF_ERR_INVALID, "cf_model_param_floats: null argument");
    *n = pm_tensor_offsets(m->hp).back();
    return CF_OK;
}

extern "C" int cf_model_load_params(cf_model* m, const float* params, void* stream) {
    if (!m || !params) return fail(CF_ERR_INVALID, "cf_model_load_params: null argument");
    if (m->np != 0)
        return fail(CF_ERR_INVALID, "cf_model_load_params: only models created with CF_PREC_FP32 take device parameters (this one is bf16 / bf16x3)");
    HIP_TRY(hipSetDevice(m->device));
    if (!m->pmap) {
        const int rc = pm_build(m);
        if (rc != CF_OK) return rc;
    }
    const cf_param_map* pm = m->pmap;
    hipStream_t s = (hipStream_t)stream;
    if (pm->n_ch > 0) {
        hipLaunchKernelGGL(cf_bn_fold_kernel, dim3((unsigned)((pm->n_ch + 255) / 256)), dim3(256), 0, s, params, pm->bias_src, pm->n_ch, pm->C,
                           m->hp.bn_epsilon, pm->s, pm->b);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(cf_load_params_kernel, dim3((unsigned)(pm->n_map / 256)), dim3(256), 0, s, params, pm->map, pm->s, pm->b, pm->segs,
                       pm->block_seg);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}
