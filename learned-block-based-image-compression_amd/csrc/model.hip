// liblbic.so host side, the model handle: life cycle and options, state-dict loader and weight packing, entropy
// tables, the per-shape workspace, and the host rANS exports of the C ABI declared in include/lbic.h.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "model.h"

namespace lbic {

static thread_local std::string g_err;

int set_error(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

long long env_int(const char* name, long long dflt) {
    const char* e = getenv(name);
    return e && *e ? strtoll(e, nullptr, 10) : dflt;
}

namespace {

inline int pad16(int x) { return (x + 15) & ~15; }

// workspace set-up stream of handle m, ordered after the caller's stream s (an event recorded on s, waited for by the
// handle's private non-blocking stream): a legacy-stream memset / copy fails while another thread of the process
// captures a graph (decoder handles sizing their workspaces beside each other's captures), and a plain non-blocking
// stream without the event raced the handle's previous encode still running on s (round 5, test_batch_equals_single)
hipStream_t ws_stream(lbc_model* m, hipStream_t s) {
    if (!m->aux) return nullptr;
    if (hipEventRecord(m->aux_ev, s) != hipSuccess || hipStreamWaitEvent(m->aux, m->aux_ev, 0) != hipSuccess) {
        set_error(LBC_E_HIP, "workspace stream ordering failed");
        return nullptr;
    }
    return m->aux;
}

// Pack W[k][n] (row-major K x N, N padded to 16) into [K/16][N/16][4][16][4]: the float4 lane l of
// a wave loads for a 16x16 k-n tile holds W[4*(l>>4) + e][l&15], e = 0..3 -- the A/B operand of four
// v_mfma_f32_16x16x4_f32 (operand maps: cdna_hip_programming.md §3).
int upload_layer(Layer& L, const std::vector<float>& wkn, const std::vector<float>& bias, int K, int N) {
    if (K % 16) return set_error(LBC_E_ARG, "layer K not a multiple of 16");
    const int NB = ((N + 31) / 32) * 2;   // whole 32-column tiles: the widest BN never reads past the end
    std::vector<float> pk((size_t)K * NB * 16, 0.f);
    for (int kb = 0; kb < K / 16; ++kb)
        for (int nb = 0; nb < NB; ++nb)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 4; ++e) {
                    const int k = kb * 16 + 4 * (l >> 4) + e, n = nb * 16 + (l & 15);
                    pk[(((size_t)kb * NB + nb) * 64 + l) * 4 + e] = n < N ? wkn[(size_t)k * N + n] : 0.f;
                }
    std::vector<float> b(NB * 16, 0.f);
    std::copy(bias.begin(), bias.end(), b.begin());
    L.K = K;
    L.N = N;
    L.NB16 = NB;
    int rc = dev_upload(L.W, pk.data(), pk.size() * 4);
    if (rc) return rc;
    return dev_upload(L.bias, b.data(), b.size() * 4);
}

const HostT* get(lbc_model* m, const std::string& n) {
    auto it = m->host.find(n);
    return it == m->host.end() ? nullptr : &it->second;
}

// conv weight [cout][cin][k][k] -> W[k = slot*cin + ci][n] for the listed taps (a 1x1 conv is one slot)
// slot = K stride between taps (>= cin; padded columns keep zero weights)
int conv_to_kn(lbc_model* m, const std::string& name, int cin, int cout, const int (*taps)[2], int ntaps,
               std::vector<float>& wkn, int k_base, int slot, std::vector<float>* bias_acc) {
    const HostT* w = get(m, name + ".weight");
    const HostT* b = get(m, name + ".bias");
    if (!w || !b) return set_error(LBC_E_STATE, "missing tensor " + name);
    const int ks = (int)w->shape[2];
    if ((int)w->shape[0] != cout || (int)w->shape[1] != cin || (int)b->v.size() != cout)
        return set_error(LBC_E_ARG, "bad shape for " + name);
    for (int t = 0; t < ntaps; ++t) {
        const int ky = ks == 1 ? 0 : 1 + taps[t][0], kx = ks == 1 ? 0 : 1 + taps[t][1];
        for (int ci = 0; ci < cin; ++ci)
            for (int co = 0; co < cout; ++co)
                wkn[(size_t)(k_base + t * slot + ci) * cout + co] = w->v[(((size_t)co * cin + ci) * ks + ky) * ks + kx];
    }
    if (bias_acc) {
        if (bias_acc->empty()) bias_acc->assign(b->v.begin(), b->v.end());
        else for (int co = 0; co < cout; ++co) (*bias_acc)[co] += b->v[co];
    }
    return LBC_OK;
}

int pack_conv(lbc_model* m, Layer& L, const std::string& name, int cin, int cout, int ntaps, const int (*taps)[2]) {
    const int slot = pad16(cin);
    std::vector<float> wkn((size_t)ntaps * slot * cout, 0.f), bias;
    int rc = conv_to_kn(m, name, cin, cout, taps, ntaps, wkn, 0, slot, &bias);
    if (rc) return rc;
    return upload_layer(L, wkn, bias, ntaps * slot, cout);
}

// first layer of the encoder / decoder transform: 4 masked taps of prtr_*2 on zhat + the 1x1 prtr_*1
// on x (or y_qnt), one GEMM (K = 4*Cx + cin1); bias = b1 + b2 (net:379-387: out_x + out_zhat).
int pack_first(lbc_model* m, Layer& L, const std::string& n2, const std::string& n1, int cin1) {
    const int K = 4 * m->Cx + cin1;
    std::vector<float> wkn((size_t)K * m->N), bias;
    int rc = conv_to_kn(m, n2, m->Cx, m->N, TAPS_A, 4, wkn, 0, m->Cx, &bias);
    if (rc) return rc;
    static const int one[1][2] = {{0, 0}};
    rc = conv_to_kn(m, n1, cin1, m->N, one, 1, wkn, 4 * m->Cx, cin1, &bias);
    if (rc) return rc;
    return upload_layer(L, wkn, bias, K, m->N);
}

// GDN: norm_i = beta_i + sum_j gamma_ij x_j^2 with the reparametrisation of
// utils/parametrizers.py:45-47: v -> max(v, bound)^2 - pedestal, pedestal = 2^-36,
// bound = sqrt(minimum + pedestal) (beta_min = 1e-6, gdn_compressai.py:43-56).
int pack_gdn(lbc_model* m, Layer& L, const std::string& name, int C) {
    const HostT* be = get(m, name + ".beta");
    const HostT* ga = get(m, name + ".gamma");
    if (!be || !ga) return set_error(LBC_E_STATE, "missing tensor " + name);
    if ((int)be->v.size() != C || (int)ga->v.size() != C * C) return set_error(LBC_E_ARG, "bad GDN shape " + name);
    const float ped = (float)std::pow(2.0, -36.0);
    const float bb = (float)std::sqrt(1e-6 + std::pow(2.0, -36.0));
    const float gb = (float)std::sqrt(0.0 + std::pow(2.0, -36.0));
    std::vector<float> beta(C), wkn((size_t)pad16(C) * C, 0.f);
    for (int i = 0; i < C; ++i) {
        const float t = std::max(be->v[i], bb);
        beta[i] = t * t - ped;
    }
    for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j) {
            const float t = std::max(ga->v[(size_t)i * C + j], gb);
            wkn[(size_t)j * C + i] = t * t - ped;       // W[k = j][n = i]
        }
    return upload_layer(L, wkn, beta, pad16(C), C);
}

// zero a fresh workspace buffer on the handle's set-up stream (ordered after the caller's earlier work on s, ws_stream)
// and wait for it
static int ws_zero(lbc_model* m, hipStream_t s, void* p, size_t b) {
    hipStream_t q = ws_stream(m, s);
    if (!q) return set_error(LBC_E_HIP, "workspace stream unavailable");
    HIPCHK(hipMemsetAsync(p, 0, b, q));
    HIPCHK(hipStreamSynchronize(q));
    return LBC_OK;
}

}  // namespace

int dev_upload(DevBuf& d, const void* src, size_t bytes, lbc_model* m, hipStream_t s) {
    int rc = d.alloc(bytes);
    if (rc) return rc;
    if (!m) {
        HIPCHK(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
        return LBC_OK;
    }
    // on the handle's set-up stream (after the caller's earlier work on s), then waited for
    hipStream_t q = ws_stream(m, s);
    if (!q) return set_error(LBC_E_HIP, "workspace stream unavailable");
    HIPCHK(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, q));
    HIPCHK(hipStreamSynchronize(q));
    return LBC_OK;
}

int ensure_workspace(lbc_model* m, int n_img, int Hb, int Wb, hipStream_t s) {
    if (m->ws_n == n_img && m->ws_Hb == Hb && m->ws_Wb == Wb) return LBC_OK;
    const int T = (Wb - 1) + 2 * (Hb - 1) + 1;
    std::vector<int4> enc;
    m->step_off.assign(T, 0);
    m->step_cnt.assign(T, 0);
    int mmax = n_img;
    for (int t = 0; t < T; ++t) {
        m->step_off[t] = (int)enc.size();
        for (int img = 0; img < n_img; ++img)
            for (int v = 0; v < Hb; ++v) {
                const int h = t - 2 * v;
                if (h >= 0 && h < Wb) enc.push_back(make_int4(img, v, h, 0));
            }
        m->step_cnt[t] = (int)enc.size() - m->step_off[t];
        mmax = std::max(mmax, m->step_cnt[t]);
    }
    std::vector<int4> dec((size_t)Hb * Wb * n_img);
    for (int s = 0; s < Hb * Wb; ++s)
        for (int img = 0; img < n_img; ++img) dec[(size_t)s * n_img + img] = make_int4(img, s / Wb, s % Wb, 0);
    // the GEMM kernels address A rows with unsigned 32-bit float4 offsets from a segment base (kernels.hip, Rows):
    // up to 2^34 floats (64 GB) per buffer
    const double lim = 17179869184.0;
    if ((double)n_img * (Hb + 2) * (Wb + 4) * m->Cx >= lim || (double)n_img * Hb * Wb * m->Cx >= lim ||
        (double)mmax * m->P * std::max({m->C1P, m->NP, m->C2P}) * 5 >= lim)
        return set_error(LBC_E_ARG, "frame batch too large (a workspace buffer above 64 GB); split the batch");
    // Layer-0 map cache (KS[1] = 3).  The context net's second layer reads layer 0 at the five positions (v-1, h-1..h+1),
    // (v, h-1), (v, h) (a 3x3 'B' mask); the value at a position depends only on reconstructions coded
    // before that position's own block (the 'A' taps), so it is computed once -- at its own block's step, position
    // (0,0) -- and read from the cache afterwards, instead of at five positions in every step.  Border cells under
    // compress() (the zero-padded window, net:342-351): row -1 is constant (k_l0_border); column -1 of row v depends
    // on zhat(v-1, 0) and is computed at block (v, 0)'s step, column Wb of row v-1 on zhat(v-2 .. v-1, Wb-1) and is
    // computed at block (v, Wb-1)'s step, the only step that reads it.
    std::vector<int4> cells;
    if (m->l0_on) {
        m->cell_off.assign(T, 0);
        m->cell_cnt.assign(T, 0);
        for (int t = 0; t < T; ++t) {
            m->cell_off[t] = (int)cells.size();
            for (int img = 0; img < n_img; ++img)
                for (int v = 0; v < Hb; ++v) {
                    const int h = t - 2 * v;
                    if (h < 0 || h >= Wb) continue;
                    cells.push_back(make_int4(img, v, h, 0));
                    if (h == 0) cells.push_back(make_int4(img, v, -1, 0));
                    if (h == Wb - 1) cells.push_back(make_int4(img, v - 1, Wb, 0));
                }
            m->cell_cnt[t] = (int)cells.size() - m->cell_off[t];
        }
        if ((double)n_img * (Hb + 2) * (Wb + 4) * m->C1P >= lim)
            return set_error(LBC_E_ARG, "frame batch too large (layer-0 cache above 64 GB); split the batch");
    }
    int rc;
    if ((rc = dev_upload(m->blocks_enc, enc.data(), enc.size() * sizeof(int4), m, s))) return rc;
    if ((rc = dev_upload(m->blocks_dec, dec.data(), dec.size() * sizeof(int4), m, s))) return rc;
    if (m->l0_on) {
        if ((rc = dev_upload(m->cells_enc, cells.data(), cells.size() * sizeof(int4), m, s))) return rc;
        const size_t b = (size_t)n_img * (Hb + 2) * (Wb + 4) * m->C1P * sizeof(float);
        if ((rc = m->l0.alloc(b))) return rc;
        if ((rc = ws_zero(m, s, m->l0.p, b))) return rc;   // pad channels stay 0 (never written; A x 0-weight meets no NaN)
    }
    const size_t F = sizeof(float);
    if ((rc = m->zpad.alloc(zpad_bytes(m, n_img, Hb, Wb)))) return rc;
    Work& w = m->work;
    const size_t rows = (size_t)mmax;       // the largest wavefront step (a raster step has n_img <= mmax rows)
    w.rows = mmax;
    // activation widths are padded to 16 columns; the pad columns are zeroed once and never
    // written, so GEMMs can run K over whole 16-wide k-blocks (their weights are zero there too)
    DevBuf* bufs[] = {&w.ctx0, &w.ctx1, &w.ctx2, &w.ksi, &w.e0, &w.e1, &w.d0, &w.d1, &w.yq, &w.idx};
    const size_t widths[] = {(size_t)m->P * m->C1P, (size_t)m->C2P, (size_t)m->C3P, (size_t)m->C4, (size_t)m->NP,
                             (size_t)m->NP, (size_t)m->NP, (size_t)m->NP, (size_t)m->M, (size_t)m->M};
    for (int i = 0; i < 10; ++i) {
        if ((rc = bufs[i]->alloc(rows * widths[i] * F))) return rc;
        if ((rc = ws_zero(m, s, bufs[i]->p, rows * widths[i] * F))) return rc;
    }
    m->Mmax = mmax;
    m->ws_n = n_img;
    m->ws_Hb = Hb;
    m->ws_Wb = Wb;
    return LBC_OK;
}

// first device use: events and the entropy tables (host copies made by lbc_set_entropy_tables)
int prepare_device(lbc_model* m) {
    HIPCHK(hipSetDevice(m->cfg.device));
    if (!m->ev[0]) {
        for (auto& e : m->ev) HIPCHK(hipEventCreate(&e));
        HIPCHK(hipStreamCreateWithFlags(&m->cap, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&m->cap2, hipStreamNonBlocking));
        for (auto& e : m->fev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHK(hipStreamCreateWithFlags(&m->aux, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&m->aux_ev, hipEventDisableTiming));
    }
    if (m->tabs_dirty) {
        int rc;
        if ((rc = dev_upload(m->table_dev, m->tabs.table.data(), 64 * sizeof(float)))) return rc;
        if ((rc = dev_upload(m->cdf16_dev, m->c16_host.data(), m->c16_host.size() * 2))) return rc;
        if ((rc = dev_upload(m->tmeta_dev, m->meta_host.data(), m->meta_host.size() * sizeof(int)))) return rc;
        m->tabs_dirty = false;
    }
    return LBC_OK;
}

int zero_zpad(lbc_model* m, int n_img, int Hb, int Wb, hipStream_t s) {
    HIPCHK(hipMemsetAsync(m->zpad.p, 0, zpad_bytes(m, n_img, Hb, Wb), s));
    return LBC_OK;
}

// a new closed loop starts: zero reconstruction, and (layer-0 cache) the cache's constant row -1 -- LeakyReLU(bias),
// the layer-0 map of a zero window; frame_pad: zero, forward()'s padding of the map itself
int reset_frame(lbc_model* m, int n_img, int Hb, int Wb, hipStream_t s, bool frame_pad) {
    int rc = zero_zpad(m, n_img, Hb, Wb, s);
    if (rc || !m->l0_on) return rc;
    return launch_l0_border(m->l0.as<float>(), n_img, Hb, Wb, m->C1P, frame_pad ? nullptr : m->net->ctx0.bias.as<float>(), s);
}

// the checks that open the coding entry points, in their fixed order: arguments, lbc_finalize(), update(), frame size
int check_entry(const lbc_model* m, bool args_ok, bool need_tabs, bool dims_ok, const char* empty) {
    if (!m || !args_ok) return set_error(LBC_E_ARG, "null argument");
    if (!m->finalized) return set_error(LBC_E_STATE, "lbc_finalize() not called");
    if (need_tabs && !m->tabs_set) return set_error(LBC_E_NOT_UPDATED, "Uninitialized CDFs. Run update() first");
    return dims_ok ? LBC_OK : set_error(LBC_E_ARG, empty);
}

}  // namespace lbic

using namespace lbic;

extern "C" {

int lbc_create(const lbc_config* cfg, lbc_model** out) {
    if (!cfg || !out) return set_error(LBC_E_ARG, "null argument");
    if (cfg->block_size <= 0 || cfg->n <= 0 || cfg->m <= 0 || cfg->ks[0] != 3 || (cfg->ks[1] != 1 && cfg->ks[1] != 3))
        return set_error(LBC_E_ARG, "unsupported geometry (KS[0] must be 3, KS[1] 1 or 3)");
    if (cfg->ks[2] != 1 && cfg->ks[2] != 3) return set_error(LBC_E_ARG, "bad KS");
    auto* m = new lbc_model();   // no HIP call here: host-only entry points work without a GPU
    m->cfg = *cfg;
    m->B = cfg->block_size;
    m->Cx = 3 * m->B * m->B;
    m->N = cfg->n;
    m->M = cfg->m;
    m->N7 = m->N / 8 * 7;
    m->N6 = m->N / 8 * 6;
    m->C1 = m->N / 8 * 12;
    m->C2 = m->N / 8 * 10;
    m->C3 = m->N / 8 * 8;
    m->C4 = 2 * m->M;
    m->NP = pad16(m->N);
    m->C1P = pad16(m->C1);
    m->C2P = pad16(m->C2);
    m->C3P = pad16(m->C3);
    if (m->Cx % 16 || m->M % 16) {
        delete m;
        return set_error(LBC_E_ARG, "3*B^2 and M must be multiples of 16");
    }
    m->P = cfg->ks[1] == 3 ? 5 : 1;
    m->l0_on = m->P == 5 && env_int("LBIC_L0CACHE", 1) != 0;   // 0: layer 0 at five positions per block (A/B runs)
    *out = m;
    return LBC_OK;
}

int lbc_create_sibling(const lbc_model* src, lbc_model** out) {
    if (!src || !out) return set_error(LBC_E_ARG, "null argument");
    if (!src->finalized) return set_error(LBC_E_STATE, "lbc_finalize() not called on the source handle");
    lbc_model* m = nullptr;
    if (int rc = lbc_create(&src->cfg, &m)) return rc;     // the same geometry
    m->l0_on = src->l0_on;
    m->enc_lds_floor = src->enc_lds_floor;
    m->enc_fork = src->enc_fork;
    m->net = src->net;                    // shared, read-only
    m->finalized = true;
    if (src->tabs_set) {                  // host copies; this handle uploads its own device tables on first use
        m->tabs = src->tabs;
        m->total16 = src->total16;
        m->c16_host = src->c16_host;
        m->meta_host = src->meta_host;
        m->tabs_set = true;
        m->tabs_dirty = true;
    }
    *out = m;
    return LBC_OK;
}

int lbc_set_option(lbc_model* m, int option, long long value) {
    if (!m) return set_error(LBC_E_ARG, "null argument");
    switch (option) {
        case LBC_OPT_ENC_LDS_FLOOR:
            if (value < 0 || value > 160 * 1024) return set_error(LBC_E_ARG, "LDS floor out of range [0, 160 KB]");
            m->enc_lds_floor = (int)value;
            return LBC_OK;
        case LBC_OPT_TEAM_WG_PER_CU:
            if (value < 1 || value > 2) return set_error(LBC_E_ARG, "team workgroups per CU must be 1 or 2");
            m->team_wpc = (int)value;
            return LBC_OK;
        case LBC_OPT_TEAM_SIZE:
            if (value < 0 || value > 32) return set_error(LBC_E_ARG, "team size must be 0 (CUs / 8) .. 32");
            m->team_size = (int)value;
            return LBC_OK;
        case LBC_OPT_ENC_FORK:
            if (value < -1 || value > 1) return set_error(LBC_E_ARG, "encoder fork must be -1 (auto), 0 or 1");
            m->enc_fork = (int)value;
            return LBC_OK;
    }
    return set_error(LBC_E_ARG, "unknown option");
}

void lbc_destroy(lbc_model* m) {
    if (!m) return;
    if (m->prof.slots) (void)hipFree(m->prof.slots);
    if (m->prof.snap) (void)hipHostFree(m->prof.snap);
    for (hipGraphExec_t e : {m->enc_exec, m->dec_exec, m->wf_exec})
        if (e) (void)hipGraphExecDestroy(e);
    for (auto& kv : m->band_exec) (void)hipGraphExecDestroy(kv.second);
    for (hipStream_t st : {m->cap, m->cap2, m->aux})
        if (st) (void)hipStreamDestroy(st);
    for (hipEvent_t e : {m->ev[0], m->ev[1], m->ev[2], m->ev[3], m->fev[0], m->fev[1], m->aux_ev})
        if (e) (void)hipEventDestroy(e);
    delete m;
}

int lbc_set_tensor(lbc_model* m, const char* name, const float* host, const int64_t* shape, int ndim) {
    if (!m || !name || !host || (ndim > 0 && !shape)) return set_error(LBC_E_ARG, "null argument");
    std::string n(name);
    auto ends = [&](const char* suf) {
        const size_t l = strlen(suf);
        return n.size() >= l && n.compare(n.size() - l, l, suf) == 0;
    };
    if (ends(".mask") || ends(".pedestal") || ends(".bound") || n.rfind("conditional_gaussian_model.", 0) == 0)
        return LBC_OK;   // derived constants / entropy buffers (set through lbc_set_entropy_tables)
    HostT t;
    size_t cnt = 1;
    for (int i = 0; i < ndim; ++i) {
        t.shape.push_back(shape[i]);
        cnt *= (size_t)shape[i];
    }
    t.v.assign(host, host + cnt);
    m->host[n] = std::move(t);
    m->finalized = false;
    return LBC_OK;
}

int lbc_finalize(lbc_model* m) {
    if (!m) return set_error(LBC_E_ARG, "null model");
    HIPCHK(hipSetDevice(m->cfg.device));
    // pack into a new set and install it only when every layer packed: a failing call (or one on a sibling, which
    // holds no host tensors) leaves the handle's working weights, graphs and finalized state untouched
    auto net = std::make_shared<Net>();   // a new packed set: siblings made earlier keep theirs
    const int Cx = m->Cx, N = m->N, M = m->M;
    static const int one[1][2] = {{0, 0}};
    int rc;
    // context net: layer 0 = 4 masked taps; layer 1 = 1x1, or 3x3 'B' over the 5 layer-0 positions
    if ((rc = pack_conv(m, net->ctx0, "get_meanscale.0", Cx, m->C1, 4, TAPS_A))) return rc;
    if (m->P == 5) rc = pack_conv(m, net->ctx1, "get_meanscale.2", m->C1, m->C2, 5, TAPS_B);
    else rc = pack_conv(m, net->ctx1, "get_meanscale.2", m->C1, m->C2, 1, one);
    if (rc) return rc;
    if ((rc = pack_conv(m, net->ctx2, "get_meanscale.4", m->C2, m->C3, 1, one))) return rc;
    if ((rc = pack_conv(m, net->ctx3, "get_meanscale.6", m->C3, m->C4, 1, one))) return rc;
    if ((rc = pack_first(m, net->enc0, "prtr_forward2", "prtr_forward1", Cx))) return rc;
    if ((rc = pack_gdn(m, net->g0, "prtr_forward3.0", N))) return rc;
    if ((rc = pack_conv(m, net->e1, "prtr_forward3.1", N, m->N7, 1, one))) return rc;
    if ((rc = pack_gdn(m, net->g1, "prtr_forward3.2", m->N7))) return rc;
    if ((rc = pack_conv(m, net->e2, "prtr_forward3.3", m->N7, m->N6, 1, one))) return rc;
    if ((rc = pack_gdn(m, net->g2, "prtr_forward3.4", m->N6))) return rc;
    if ((rc = pack_conv(m, net->e3, "prtr_forward3.5", m->N6, M, 1, one))) return rc;
    if ((rc = pack_first(m, net->dec0, "prtr_inverse2", "prtr_inverse1", M))) return rc;
    if ((rc = pack_gdn(m, net->ig0, "prtr_inverse3.0", N))) return rc;
    if ((rc = pack_conv(m, net->d1, "prtr_inverse3.1", N, m->N7, 1, one))) return rc;
    if ((rc = pack_gdn(m, net->ig1, "prtr_inverse3.2", m->N7))) return rc;
    if ((rc = pack_conv(m, net->d2, "prtr_inverse3.3", m->N7, m->N6, 1, one))) return rc;
    if ((rc = pack_gdn(m, net->ig2, "prtr_inverse3.4", m->N6))) return rc;
    if ((rc = pack_conv(m, net->d3, "prtr_inverse3.5", m->N6, Cx, 1, one))) return rc;
    // the captured graphs and the recorded team program hold the old weight pointers
    for (hipGraphExec_t* e : {&m->enc_exec, &m->dec_exec, &m->wf_exec})
        if (*e) { (void)hipGraphExecDestroy(*e); *e = nullptr; }
    for (auto& kv : m->band_exec) (void)hipGraphExecDestroy(kv.second);
    m->band_exec.clear();
    m->band_key.clear();
    m->team_key.clear();
    m->net = std::move(net);
    m->finalized = true;
    return LBC_OK;
}

int lbc_pmf_to_quantized_cdf(const float* pmf, int n, int precision, uint32_t* cdf_out) {
    if (!pmf || !cdf_out) return set_error(LBC_E_ARG, "null argument");
    return pmf_to_quantized_cdf(pmf, n, precision, cdf_out);
}

int lbc_set_entropy_tables(lbc_model* m, const float* scale_table, int n_tables, const int32_t* cdf, int cdf_stride,
                           const int32_t* cdf_length, const int32_t* offset) {
    if (!m || !scale_table || !cdf || !cdf_length || !offset) return set_error(LBC_E_ARG, "null argument");
    if (n_tables != 64) return set_error(LBC_E_ARG, "expected the 64-entry scale table (net:13-18)");
    EntropyTables& t = m->tabs;
    t.n_tables = n_tables;
    t.stride = cdf_stride;
    t.table.assign(scale_table, scale_table + n_tables);
    t.cdf.assign(cdf, cdf + (size_t)n_tables * cdf_stride);
    t.length.assign(cdf_length, cdf_length + n_tables);
    t.offset.assign(offset, offset + n_tables);
    // device copies: scale table, and the GPU rANS decoder's LDS image of the CDF rows
    std::vector<uint16_t> c16;
    std::vector<int> meta;
    if (int rc = build_rans_gpu_tables(t, c16, meta)) return rc;
    m->total16 = (int)c16.size();
    m->c16_host = std::move(c16);
    m->meta_host = std::move(meta);
    m->tabs_set = true;
    m->tabs_dirty = true;
    return LBC_OK;
}

int lbc_rans_encode(const lbc_model* m, const int32_t* sym, const int32_t* idx, size_t n, uint8_t** out, size_t* len) {
    if (!m || !sym || !idx || !out || !len) return set_error(LBC_E_ARG, "null argument");
    if (!m->tabs_set) return set_error(LBC_E_NOT_UPDATED, "Uninitialized CDFs. Run update() first");
    std::vector<uint8_t> bytes;
    int rc = rans_encode(m->tabs, sym, idx, n, bytes);
    if (rc) return rc;
    *out = static_cast<uint8_t*>(malloc(std::max<size_t>(bytes.size(), 1)));
    std::memcpy(*out, bytes.data(), bytes.size());
    *len = bytes.size();
    return LBC_OK;
}

int lbc_rans_decode_host(const lbc_model* m, const uint8_t* data, size_t len, const int32_t* idx, size_t n,
                         int32_t* sym_out) {
    if (!m || !data || !idx || !sym_out) return set_error(LBC_E_ARG, "null argument");
    if (!m->tabs_set) return set_error(LBC_E_NOT_UPDATED, "Uninitialized CDFs. Run update() first");
    return rans_decode_host(m->tabs, data, len, idx, n, sym_out);
}

void lbc_free(void* p) { free(p); }

const char* lbc_last_error(void) { return g_err.c_str(); }

}  // extern "C"
