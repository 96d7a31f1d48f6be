// liblbic.so host side, one wavefront / raster step: the context net, the encoder and the decoder transform as GEMM
// launches (run_ctx / run_enc / run_dec) with their launch, record and profile modes, graph capture, the profiler.
//
// Encode (compress, net:319-361): the raster closed loop is replayed as a skewed anti-diagonal
// wavefront.  Block (v, h) needs the reconstructions of (v-1, h-1..h+1), (v, h-1) (and, for KS[1] = 3,
// of (v-2, h-2..h+2), (v-1, h-2), (v, h-2)), so every block with h + 2v = t depends only on steps < t
// and all of them -- across every image of the batch -- are coded in one step of 18 GEMM launches.
// Decode (decompress, net:400-452) keeps the reference's single raster-ordered rANS stream per image:
// each raster step decodes the same block position of every image (ctx GEMMs -> GPU rANS -> decoder
// GEMMs).  Both phases run the same k_gemm arithmetic, so decoder scale indexes equal the encoder's.
#include <cstdio>
#include <cstring>
#include <mutex>

#include "model.h"

namespace lbic {

thread_local Recorder* g_rec = nullptr;

namespace {

// graph captures of different handles are serialised (one-off cost): concurrent first-time captures from
// several host threads failed a kernel launch under rocprofv3's tracer
static std::mutex g_capture_mu;

static const char* kKernelNames[kNClass] = {"k_gemm_s", "k_gemm", "k_rans_decode", "k_copy_interior"};
static thread_local Prof* g_prof = nullptr;

void drop_recs(Prof& p, int r) {
    std::vector<Prof::Rec> keep;
    for (const auto& x : p.recs)
        if (x.slot / kSlotsPerRange != r) keep.push_back(x);
    p.recs.swap(keep);
}

// start capturing sampled launches into slot range r: the range is zeroed by the graph's first node
int prof_range_begin(Prof* p, int r, hipStream_t s) {
    p->range = r;
    p->next = 0;
    for (auto& c : p->per_replay[r]) c = 0;
    for (auto& c : p->work_replay[r]) c[0] = c[1] = 0;
    if (p->sample_every && p->slots)
        return launch_zero_u64(p->slots + kSlotU64 * (size_t)r * kSlotsPerRange, kSlotU64 * kSlotsPerRange, s);
    return LBC_OK;
}

// launch a GEMM; in a sampled step give it a timing slot and record its algorithmic work
static void gemm_work(const GemmArgs& g, double& flops, double& bytes) {
    flops = 2.0 * g.M * g.K * g.N;
    bytes = 4.0 * ((double)g.K * g.N + (double)g.M * g.K + (double)g.M * g.N * (g.square_a ? 2 : 1));
}

int gemm(const GemmArgs& g0, hipStream_t s) {
    if (g_rec) {
        GemmArgs g = g0;
        if (g.M <= 0) return set_error(LBC_E_ARG, "empty GEMM in a recorded step");
        const int rc = prepare_gemm(g);
        if (rc) return rc;
        g_rec->ops.push_back((int)g_rec->gemms.size());
        g_rec->gemms.push_back(g);
        return LBC_OK;
    }
    Prof* p = g_prof;
    if (p) {
        const int c = gemm_class(g0);       // the class launch_gemm will pick
        double f, b;
        gemm_work(g0, f, b);
        p->per_replay[p->range][c] += 1;
        p->work_replay[p->range][c][0] += f;
        p->work_replay[p->range][c][1] += b;
    }
    if (!p || !p->active) return launch_gemm(g0, s);
    GemmArgs g = g0;
    g.ts = p->take();
    if (!g.ts) return launch_gemm(g0, s);
    int cls = 0;
    int rc = launch_gemm(g, s, &cls);
    if (rc) return rc;
    double flops, bytes;
    gemm_work(g, flops, bytes);
    p->add(cls, g.ts, flops, bytes);
    return LBC_OK;
}

void set_layer(GemmArgs& g, const Layer& L, int epi, float* out, int ldo) {
    g.W = L.W.as<float>();
    g.bias = L.bias.as<float>();
    g.NB16 = L.NB16;
    g.K = L.K;
    g.N = L.N;
    g.epi = epi;
    g.out = out;
    g.ldo = ldo;
}

void seg_dense(GemmArgs& g, const float* base, int ld, int k0, int k1) {
    Seg& s = g.seg[g.nseg++];
    s = Seg{base, SEG_DENSE, ld, 0, 0, k0, k1};
}

void segs_ztaps(GemmArgs& g, int Cx) {
    for (int t = 0; t < 4; ++t) {
        Seg& s = g.seg[g.nseg++];
        s = Seg{g.geo.zpad, SEG_ZTAP, 0, TAPS_A[t][0], TAPS_A[t][1], t * Cx, (t + 1) * Cx};
    }
}

int run_dense(GemmArgs g, const Layer& L, const float* in, int ld_in, int epi, float* out, int ldo, hipStream_t s) {
    g.nseg = 0;
    g.square_a = 0;
    set_layer(g, L, epi, out, ldo);
    seg_dense(g, in, ld_in, 0, L.K);
    return gemm(g, s);
}

// ld: row stride of `in` and `out` (the padded activation width)
int run_gdn(GemmArgs g, const Layer& L, const float* in, int ld, bool inverse, float* out, hipStream_t s) {
    g.nseg = 0;
    set_layer(g, L, inverse ? EPI_IGDN : EPI_GDN, out, ld);
    seg_dense(g, in, ld, 0, L.K);
    g.square_a = 1;
    g.gx = in;
    g.ldx = ld;
    return gemm(g, s);
}

}  // namespace

RansArgs rans_args(lbc_model* m) {
    RansArgs r{};
    r.cdf16 = m->cdf16_dev.as<uint16_t>();
    r.tmeta = m->tmeta_dev.as<int>();
    r.total16 = m->total16;
    r.words = m->words.as<uint32_t>();
    r.word_base = m->word_base.as<long long>();
    r.word_count = m->word_count.as<int>();
    r.state_x = m->st_x.as<unsigned long long>();
    r.state_ptr = m->st_ptr.as<int>();
    r.status = m->st_status.as<int>();
    r.ldk = m->C4;
    r.Mlat = m->M;
    r.ldy = m->M;
    r.streams_per_img = 1;
    return r;
}

GemmArgs base_args(lbc_model* m, const int4* blocks, int rows, const float* x, int Hb, int Wb) {
    GemmArgs g{};
    g.M = rows;
    g.P = 1;
    g.blocks = blocks;
    g.pos_dy[0] = g.pos_dx[0] = 0;
    g.geo.zpad = m->zpad.as<float>();
    g.geo.Hp = Hb + 2;
    g.geo.Wp = Wb + 4;
    g.geo.Cx = m->Cx;
    g.geo.x = x;
    g.geo.Hb = Hb;
    g.geo.Wb = Wb;
    g.table = m->table_dev.as<float>();
    g.Mlat = m->M;
    g.HW = Hb * Wb;
    g.lds_floor = m->enc_lds_floor;
    return g;
}

// context net (get_meanscale_fast, net:389-398) for the rows of `g`; the last layer's epilogue is
// plain (encode) or also emits the scale indexes (decode).  frame_pad: forward()'s full-frame semantics
// (get_meanscale as nn.Sequential, net:57-65): the layer-0 map is zero outside the frame.
// cells / ncells: the layer-0 cache cells of this wavefront step (cache mode, encoder and wavefront decoder); a
// raster step (g.raster) computes its own block's cell plus the border cell it owns (column -1 at h = 0, column Wb
// of the row above at h = Wb - 1).  Without either (forward(): every block at once) layer 0 runs at the five
// positions per block as before.
int run_ctx(lbc_model* m, Work& w, GemmArgs g, bool with_idx, hipStream_t s, bool frame_pad,
            const int4* cells, int ncells) {
    int rc;
    if (m->l0_on && (cells || g.raster)) {
        GemmArgs c = g;
        c.nseg = 0;
        c.square_a = 0;
        c.zero_oob = frame_pad;
        c.pos_dy[0] = c.pos_dx[0] = 0;
        if (cells) {
            c.blocks = cells;
            c.M = ncells;
            c.P = 1;
        } else {
            int P = 1;
            if (g.raster_h == 0) { c.pos_dy[P] = 0; c.pos_dx[P] = -1; ++P; }
            if (g.raster_h == g.geo.Wb - 1) { c.pos_dy[P] = -1; c.pos_dx[P] = 1; ++P; }
            c.P = P;
            c.M = g.M * P;
        }
        set_layer(c, m->net->ctx0, EPI_LEAKY_L0, m->l0.as<float>(), m->C1P);
        segs_ztaps(c, m->Cx);
        if ((rc = gemm(c, s))) return rc;
        GemmArgs d = g;
        d.nseg = 0;
        d.square_a = 0;
        set_layer(d, m->net->ctx1, EPI_LEAKY, w.ctx1.as<float>(), m->C2P);
        for (int t = 0; t < 5; ++t) {       // the 3x3 'B' taps of layer 1 = five cache cells, K order as packed
            Seg& sg = d.seg[d.nseg++];
            sg = Seg{m->l0.as<float>(), SEG_L0TAP, m->C1P, TAPS_B[t][0], TAPS_B[t][1], t * m->C1P, (t + 1) * m->C1P};
        }
        if ((rc = gemm(d, s))) return rc;
    } else {
        GemmArgs c = g;
        c.nseg = 0;
        c.square_a = 0;
        c.zero_oob = frame_pad && m->P > 1;
        c.P = m->P;
        c.M = g.M * m->P;
        for (int p = 0; p < m->P; ++p) {
            c.pos_dy[p] = m->P == 1 ? 0 : TAPS_B[p][0];
            c.pos_dx[p] = m->P == 1 ? 0 : TAPS_B[p][1];
        }
        set_layer(c, m->net->ctx0, EPI_LEAKY, w.ctx0.as<float>(), m->C1P);
        segs_ztaps(c, m->Cx);
        if ((rc = gemm(c, s))) return rc;
        rc = run_dense(g, m->net->ctx1, w.ctx0.as<float>(), m->P * m->C1P, EPI_LEAKY, w.ctx1.as<float>(), m->C2P, s);
        if (rc) return rc;
    }
    if ((rc = run_dense(g, m->net->ctx2, w.ctx1.as<float>(), m->C2P, EPI_LEAKY, w.ctx2.as<float>(), m->C3P, s)))
        return rc;
    GemmArgs c = g;
    c.idx = w.idx.as<int32_t>();
    return run_dense(c, m->net->ctx3, w.ctx2.as<float>(), m->C3P, with_idx ? EPI_CTXIDX : EPI_BIAS, w.ksi.as<float>(),
                     m->C4, s);
}

// decoder transform (inverse_prtr_fast, net:384-387) + clamp + write-back into zpad (net:357); with
// xhat: the unclamped output scattered to xhat[img][v][h] instead (forward(), net:104)
int run_dec(lbc_model* m, Work& w, GemmArgs g, hipStream_t s, float* xhat) {
    int rc;
    {
        GemmArgs c = g;
        c.nseg = 0;
        c.square_a = 0;
        set_layer(c, m->net->dec0, EPI_BIAS, w.d0.as<float>(), m->NP);
        segs_ztaps(c, m->Cx);
        seg_dense(c, w.yq.as<float>(), m->M, 4 * m->Cx, 4 * m->Cx + m->M);
        if ((rc = gemm(c, s))) return rc;
    }
    float *d0 = w.d0.as<float>(), *d1 = w.d1.as<float>();
    const int W = m->NP;
    if ((rc = run_gdn(g, m->net->ig0, d0, W, true, d1, s))) return rc;
    if ((rc = run_dense(g, m->net->d1, d1, W, EPI_BIAS, d0, W, s))) return rc;
    if ((rc = run_gdn(g, m->net->ig1, d0, W, true, d1, s))) return rc;
    if ((rc = run_dense(g, m->net->d2, d1, W, EPI_BIAS, d0, W, s))) return rc;
    if ((rc = run_gdn(g, m->net->ig2, d0, W, true, d1, s))) return rc;
    if (xhat) return run_dense(g, m->net->d3, d1, W, EPI_SCATTER, xhat, m->Cx, s);   // forward(): xhat, not clamped
    return run_dense(g, m->net->d3, d1, W, EPI_CLAMPZ, nullptr, 0, s);
}

// encoder transform (forward_prtr_fast, net:379-382) + quantize epilogue.  part: 0 all, 1 the layers before the
// quantising GEMM (they do not read the context net's output), 2 the quantising GEMM only
int run_enc(lbc_model* m, Work& w, GemmArgs g, int32_t* sym, int32_t* idx, float* bits, hipStream_t s, int part) {
    int rc;
    float *e0 = w.e0.as<float>(), *e1 = w.e1.as<float>();
    const int W = m->NP;
    if (part != 2) {
        GemmArgs c = g;
        c.nseg = 0;
        c.square_a = 0;
        set_layer(c, m->net->enc0, EPI_BIAS, e0, m->NP);
        segs_ztaps(c, m->Cx);
        Seg& sx = c.seg[c.nseg++];
        sx = Seg{c.geo.x, SEG_X, 0, 0, 0, 4 * m->Cx, 5 * m->Cx};
        if ((rc = gemm(c, s))) return rc;
        if ((rc = run_gdn(g, m->net->g0, e0, W, false, e1, s))) return rc;
        if ((rc = run_dense(g, m->net->e1, e1, W, EPI_BIAS, e0, W, s))) return rc;
        if ((rc = run_gdn(g, m->net->g1, e0, W, false, e1, s))) return rc;
        if ((rc = run_dense(g, m->net->e2, e1, W, EPI_BIAS, e0, W, s))) return rc;
        if ((rc = run_gdn(g, m->net->g2, e0, W, false, e1, s))) return rc;
        if (part == 1) return LBC_OK;
    }
    GemmArgs c = g;
    c.ksi = w.ksi.as<float>();
    c.ldk = m->C4;
    c.sym = sym;
    c.idx = idx;
    c.bits = bits;
    return run_dense(c, m->net->e3, e1, W, EPI_QUANT, w.yq.as<float>(), m->M, s);
}

// the rANS decode of a raster / wavefront step over `rows` rows of the step workspace; the caller adds what its
// schedule needs (blocks, ctr, streams_per_img)
RansArgs rans_step_args(lbc_model* m, int rows, int sparse) {
    RansArgs r = rans_args(m);
    r.idx = m->work.idx.as<int32_t>();
    r.ksi = m->work.ksi.as<float>();
    r.yq = m->work.yq.as<float>();
    r.rows = rows;
    r.sparse = sparse;
    return r;
}

// launch it inside a capture (capture_graph with a profile range), with its timing slot and record in a sampled step
int rans_step(lbc_model* m, RansArgs r, hipStream_t s) {
    Prof& p = m->prof;
    r.ts = p.active ? p.take() : nullptr;
    p.per_replay[p.range][2] += 1;
    const int rc = launch_rans_decode(r, s);
    // algorithmic bytes: the CDF tables staged into LDS + idx/mean in + y_qnt out
    if (!rc && r.ts) p.add(2, r.ts, 0.0, (double)m->total16 * 2 * ((r.rows + 7) / 8) + 12.0 * r.rows * m->M);
    return rc;
}

// Capture body() on m->cap into a graph and instantiate it as *exec (an earlier *exec is destroyed first).  Captures of
// different handles are serialised (g_capture_mu).  range >= 0: the graph's launches are profiled into that slot range
// (g_prof points at the handle for the body's duration only).  body returns an LBC_* code and must not return early
// past a HIP call that failed inside the capture: the capture is always ended here.
int capture_graph(lbc_model* m, const char* label, int range, hipGraphExec_t* exec, const std::function<int()>& body) {
    std::lock_guard<std::mutex> lk(g_capture_mu);
    if (*exec) { (void)hipGraphExecDestroy(*exec); *exec = nullptr; }
    HIPCHK(hipStreamBeginCapture(m->cap, hipStreamCaptureModeThreadLocal));
    int crc = LBC_OK;
    if (range >= 0) {
        crc = prof_range_begin(&m->prof, range, m->cap);
        drop_recs(m->prof, range);
        g_prof = &m->prof;
    }
    if (!crc) crc = body();
    m->prof.active = false;
    m->prof.nochain = false;
    g_prof = nullptr;
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(m->cap, &graph);
    if (crc) { if (graph) (void)hipGraphDestroy(graph); return crc; }
    if (e != hipSuccess) return set_error(LBC_E_HIP, std::string(label) + " capture: " + hipGetErrorString(e));
    const hipError_t ei = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) {
        *exec = nullptr;
        return set_error(LBC_E_HIP, std::string(label) + " instantiate: " + hipGetErrorString(ei));
    }
    return LBC_OK;
}

}  // namespace lbic

using namespace lbic;

extern "C" {

int lbc_profile_begin(lbc_model* m, int sample_every) {
    if (!m || sample_every < 0) return set_error(LBC_E_ARG, "bad argument");
    Prof& p = m->prof;
    if (sample_every && !p.slots) {
        HIPCHK(hipSetDevice(m->cfg.device));
        HIPCHK(hipMalloc(&p.slots, 8 * kSlotU64 * (size_t)kSlotsPerRange * kRanges));
        if (env_int("LBIC_DEBUG_STAMPS", 0))
            fprintf(stderr, "handle %p slots %p..%p\n", (void*)m, (void*)p.slots,
                    (void*)(p.slots + kSlotU64 * (size_t)kSlotsPerRange * kRanges));
    }
    // sample_every is part of the graph keys: a change re-captures (and re-creates the sample records);
    // an unchanged value only restarts the launch counting.  Every stamp slot is zeroed here, so a graph
    // that is not replayed after this call (a warmup graph, another handle's idle pass) contributes no
    // sample: lbc_profile_end counts only launches executed since lbc_profile_begin.
    if (sample_every != p.sample_every) p.recs.clear();
    p.sample_every = sample_every;
    for (auto& r : p.replays) r = 0;
    if (sample_every && !p.snap)
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&p.snap), (size_t)Prof::kSnaps * kSlotsPerRange * kSlotU64 * 8));
    p.nsnap = 0;
    if (p.slots) {
        HIPCHK(hipSetDevice(m->cfg.device));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemset(p.slots, 0, 8 * kSlotU64 * (size_t)kSlotsPerRange * kRanges));
        HIPCHK(hipDeviceSynchronize());
    }
    return LBC_OK;
}

// Reads the stamps of the sampled launches as of the last replay of every graph (a decoder row graph
// is replayed Hb times: its stamps are those of the last block row).
int lbc_profile_end(lbc_model* m, lbc_kernel_stat* out, int max_out, int* n_out) {
    if (!m || !out || !n_out) return set_error(LBC_E_ARG, "null argument");
    Prof& p = m->prof;
    lbc_kernel_stat acc[kNClass];
    std::memset(acc, 0, sizeof(acc));
    for (int c = 0; c < kNClass; ++c)
        snprintf(acc[c].name, sizeof(acc[c].name), "%s", kKernelNames[c]);
    if (p.slots && !p.recs.empty()) {
        HIPCHK(hipDeviceSynchronize());
        std::vector<unsigned long long> h(kSlotU64 * (size_t)kSlotsPerRange * kRanges);
        HIPCHK(hipMemcpy(h.data(), p.slots, h.size() * 8, hipMemcpyDeviceToHost));
        // latest end stamp of a slot over the XCDs (0: not executed since the last reset)
        auto last_end = [&](int slot) -> unsigned long long {
            const unsigned long long* t = h.data() + kSlotU64 * (size_t)slot;
            unsigned long long e = 0;
            for (int x = 0; x < 8; ++x)
                if (t[2 * x] && t[2 * x + 1]) e = std::max(e, t[2 * x + 1]);
            return e;
        };
        // the launch's span: earliest workgroup start over the XCDs -> latest workgroup end over the XCDs (what a
        // dispatch trace measures; the XCDs do not start a launch at the same moment); -1: not executed
        auto span_of = [](const unsigned long long* t) -> long long {
            unsigned long long s0 = ~0ull, e1 = 0;
            for (int x = 0; x < 8; ++x) {
                if (!t[2 * x] || !t[2 * x + 1]) continue;
                s0 = std::min(s0, ~0ull - t[2 * x]);
                e1 = std::max(e1, t[2 * x + 1]);
            }
            return e1 && e1 >= s0 ? (long long)(e1 - s0) : -1;
        };
        for (const auto& r : p.recs) {
            const unsigned long long* t = h.data() + kSlotU64 * (size_t)r.slot;
            if (r.slot < kSlotsPerRange && p.nsnap > 0 && r.slot < p.used0) {
                // the encoder graph: every replay's copy (stream-ordered D2H after each replay)
                for (int q = 0; q < p.nsnap; ++q) {
                    const long long sp = span_of(p.snap + ((size_t)q * kSlotsPerRange + r.slot) * kSlotU64);
                    if (sp < 0) continue;
                    acc[r.cls].launches += 1;
                    acc[r.cls].total_ms += (double)sp * 1e-5;
                    acc[r.cls].flops += r.flops;
                    acc[r.cls].bytes += r.bytes;
                }
                continue;
            }
            const long long span = span_of(t);
            if (span >= 0 && r.prev >= 0) {    // launch-to-launch period in the stream chain
                const unsigned long long e0 = last_end(r.prev), e1 = last_end(r.slot);
                if (e0 && e1 > e0 && e1 - e0 < 100000000ull) {
                    acc[r.cls].launches_chain += 1;
                    acc[r.cls].total_ms_chain += (double)(e1 - e0) * 1e-5;
                }
            }
            if (span > 10000000 && env_int("LBIC_DEBUG_STAMPS", 0)) {
                fprintf(stderr, "handle %p bad slot %d cls %d:", (void*)m, r.slot, r.cls);
                for (int x = 0; x < 16; ++x) fprintf(stderr, " %llx", t[x]);
                fprintf(stderr, "\n");
            }
            if (span < 0) continue;   // not executed since the last reset
#ifdef LBIC_PHASE_DIAG
            if (r.cls == 0 && t[31]) {
                static double pmax[5], psum[5], nl;
                for (int i = 1; i <= 4; ++i) { pmax[i] += (double)t[16 + i]; psum[i] += (double)t[24 + i] / (double)t[31]; }
                nl += 1;
                static int printed = 0;
                if (++printed % 50 == 0 || &r == &p.recs.back())
                    fprintf(stderr, "[diag k_gemm_s] launches %.0f  critical-WG cycles since start: prologue %.0f "
                            "loads+mfma %.0f reduce %.0f epilogue %.0f | mean WG: %.0f %.0f %.0f %.0f\n", nl,
                            pmax[1] / nl, pmax[2] / nl, pmax[3] / nl, pmax[4] / nl, psum[1] / nl, psum[2] / nl,
                            psum[3] / nl, psum[4] / nl);
            }
#endif
            acc[r.cls].launches += 1;
            acc[r.cls].total_ms += (double)span * 1e-5;     // 100 MHz ticks -> ms
            acc[r.cls].flops += r.flops;
            acc[r.cls].bytes += r.bytes;
        }
    }
    // true launch counts since lbc_profile_begin (the stamps are a sample of them)
    for (int c = 0; c < kNClass; ++c) {
        long long tot = 0;
        for (int r = 0; r < 8; ++r) {
            tot += p.per_replay[r][c] * p.replays[r];
            acc[c].total_flops += p.work_replay[r][c][0] * p.replays[r];
            acc[c].total_bytes += p.work_replay[r][c][1] * p.replays[r];
        }
        acc[c].total_launches = tot;
    }
    int n = 0;
    for (int c = 0; c < kNClass && n < max_out; ++c)
        if (acc[c].launches || acc[c].total_launches) out[n++] = acc[c];
    *n_out = n;
    return LBC_OK;
}

int lbc_last_timing(const lbc_model* m, double* enc_ms, double* dec_ms) {
    if (!m) return set_error(LBC_E_ARG, "null model");
    auto span = [](bool timed, hipEvent_t a, hipEvent_t b) -> double {      // -1: no such call yet, or an error
        float t = 0.f;
        return timed && hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&t, a, b) == hipSuccess ? t : -1.0;
    };
    if (enc_ms) *enc_ms = span(m->enc_timed, m->ev[0], m->ev[1]);
    if (dec_ms) *dec_ms = span(m->dec_timed, m->ev[2], m->ev[3]);
    return LBC_OK;
}

}  // extern "C"
