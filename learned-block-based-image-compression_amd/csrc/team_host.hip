// liblbic.so host side of the team decoder (k_dec_team, team.hip): the recorded raster step, the launch geometry, the
// fallbacks to lbc_decode, and the queries about the last launch.
#include <cstdio>
#include <mutex>

#include "model.h"

using namespace lbic;

// ---------------------------------------------------------------------------------------------- team decode
// lbc_decode_team: T batches (one per handle) decoded by ONE persistent k_dec_team launch, S workgroups per batch.
// The raster step each team replays is recorded from the same run_ctx / run_dec calls that build the graph decoder
// (three column classes: the KS3311 layer-0 cache computes border cells at h = 0 and h = Wb - 1), so the team
// decoder computes exactly what lbc_decode computes.  Falls back to lbc_decode per batch where the team kernel does
// not apply (M > 256, buffers past the 4 GB reach of its buffer loads, LBIC_TEAM=0, an LDS image past 160 KB).
static std::mutex g_team_mu;   // one team launch at a time per process: its grid must be resident as a whole

static int team_fallback(lbc_model* const* ms, int T, const uint8_t* const* streams, const size_t* lens, int n_img,
                         int Hb, int Wb, float* const* zhat, void* stream, bool after_timeout = false) {
    ms[0]->team_mode_last = 0;
    for (int t = 0; t < T; ++t) {
        ms[t]->no_one = after_timeout;
        const int rc = lbc_decode(ms[t], streams + (size_t)t * n_img, lens + (size_t)t * n_img, n_img, Hb, Wb, zhat[t],
                                  stream);
        ms[t]->no_one = false;
        if (rc) return rc;
    }
    return LBC_OK;
}

// The team program (held by ms[0]): every team's raster step recorded from the same run_ctx / run_dec calls that build
// the graph decoder, for the geometry (S, spread); rebuilt when the geometry, any team's buffers or any team's
// weight set (Net::gen) changed.  Sets ms[0]->team_args (without the per-launch fields) and the step's algorithmic work.
static int team_record(lbc_model* const* ms, int T, int n_img, int Hb, int Wb, int S, int spread, int sparse,
                       hipStream_t us) {
    lbc_model* m0 = ms[0];
    int rc;
    std::vector<long long> key = {T, S, spread, n_img, Hb, Wb, sparse};
    for (int t = 0; t < T; ++t) {
        lbc_model* m = ms[t];
        for (long long x : {(long long)m->words.p, (long long)m->zpad.p, (long long)m->work.ctx0.p,
                            (long long)m->work.d0.p, (long long)m->table_dev.p, (long long)m->tmeta_dev.p,
                            (long long)m->st_x.p, (long long)m->l0.p, m->net->gen})
            key.push_back(x);
    }
    if (key == m0->team_key) return LBC_OK;
    std::vector<GemmArgs> gem;
    std::vector<RansArgs> rans;
    std::vector<int> ops;
    int NG = -1;
    for (int t = 0; t < T; ++t) {
        lbc_model* m = ms[t];
        Work& w = m->work;
        for (int c = 0; c < 3; ++c) {
            const int hc = c == 0 ? 0 : c == 1 ? std::min(1, Wb - 1) : Wb - 1;
            Recorder rec;
            GemmArgs g = base_args(m, m->blocks_dec.as<int4>(), n_img, nullptr, Hb, Wb);
            g.ctr = m->ctr.as<int>();
            g.ctr_stride = Wb * n_img;
            g.raster = 1;
            g.raster_img0 = 0;
            g.raster_h = hc;
            g_rec = &rec;
            int crc = run_ctx(m, w, g, true, nullptr);
            rec.ops.push_back(-1);
            if (!crc) crc = run_dec(m, w, g, nullptr);
            g_rec = nullptr;
            if (crc) return crc;
            if (NG < 0) {
                NG = (int)rec.gemms.size();
                ops = rec.ops;
            }
            if ((int)rec.gemms.size() != NG || rec.ops != ops || (int)ops.size() > TEAM_MAXOPS)
                return set_error(LBC_E_STATE, "team decoder: raster steps differ in shape");
            gem.insert(gem.end(), rec.gemms.begin(), rec.gemms.end());
        }
        rans.push_back(rans_step_args(m, n_img, sparse));
    }
    const size_t gb = gem.size() * sizeof(GemmArgs), rb = rans.size() * sizeof(RansArgs);
    if ((rc = m0->team_prog.alloc(gb + rb))) return rc;
    // (on the launch's stream: a legacy-stream copy fails while another thread captures a graph)
    HIPCHK(hipMemcpyAsync(m0->team_prog.p, gem.data(), gb, hipMemcpyHostToDevice, us));
    HIPCHK(hipMemcpyAsync(static_cast<char*>(m0->team_prog.p) + gb, rans.data(), rb, hipMemcpyHostToDevice, us));
    HIPCHK(hipStreamSynchronize(us));
    if ((rc = m0->team_sync.alloc((size_t)(TEAM_MAX + 2) * 32 * sizeof(unsigned)))) return rc;
    if ((rc = m0->team_ts.alloc((size_t)TEAM_MAX * TEAM_TS_WORDS * sizeof(unsigned long long)))) return rc;
    TeamArgs& a = m0->team_args;
    a = TeamArgs{};
    a.gemm = m0->team_prog.as<GemmArgs>();
    a.rans = reinterpret_cast<const RansArgs*>(static_cast<char*>(m0->team_prog.p) + gb);
    for (size_t i = 0; i < ops.size(); ++i) a.opk[i] = ops[i];
    a.nops = (int)ops.size();
    a.NG = NG;
    a.T = T;
    a.S = S;
    a.spread = spread;
    a.sub = T > TEAM_SLOTS ? 2 : 1;
    a.Hb = Hb;
    a.Wb = Wb;
    a.sync = m0->team_sync.as<unsigned>();
    // most tiles per workgroup over the step's GEMMs (the partials' LDS; the slower path needs 2)
    a.ni_max = 2;
    a.tab16 = rans[0].total16;
    for (const GemmArgs& d : gem) {
        const int items = ((d.M + 15) >> 4) * ((d.N + 15) >> 4);
        if (!team_fast_path(d, S)) continue;
        a.ni_max = std::max(a.ni_max, (items + S - 1) / S);
    }
    // rANS waves per workgroup: two once the team has more images than workgroups (each wave then keeps one image's
    // coder state in LDS up to 2 S images; beyond that each wave decodes its rows one after another)
    a.nrw = n_img > S ? 2 : 1;
    a.rows0 = n_img;
    // the GEMM after the rANS decode (the decoder's first layer): its last K segment is y_qnt; the K slices that end
    // before it run beside the rANS decode (on the waves the rANS decode leaves free) when every workgroup takes the
    // fast path for it
    a.split_op = -1;
    a.split_wy = 0;
    for (int i = 0; i + 1 < (int)ops.size(); ++i) {
        if (ops[i] != -1 || ops[i + 1] < 0) continue;
        bool fast = true;
        for (int t = 0; t < T; ++t)
            for (int c = 0; c < 3; ++c) {
                fast = fast && team_fast_path(gem[((size_t)t * 3 + c) * NG + ops[i + 1]], S);
            }
        const GemmArgs& d = gem[ops[i + 1]];
        const Seg& last = d.seg[d.nseg - 1];
        if (last.kind != SEG_DENSE || last.base != ms[0]->work.yq.as<float>() || !fast) continue;
        const int nkb = d.K >> 4, kby = last.k0 >> 4;
        int wy = 0;
        while (wy < KSPLIT && (wy + 1) * nkb / KSPLIT <= kby) ++wy;
        wy = std::min(wy, KSPLIT - a.nrw);
        if (wy >= 1) {
            a.split_op = i + 1;
            a.split_wy = wy;
        }
    }
    // algorithmic work of one raster step (the graph decoder's accounting, gemm(): weights + A rows + outputs [+ the
    // GDN input] once per GEMM; rANS: indexes and means in, y_qnt out, the step's stream words)
    double sb = 0, sf = 0;
    for (int gi = 0; gi < NG; ++gi) {
        const GemmArgs& d = gem[(size_t)1 * NG + gi];     // team 0, inner column class
        sb += 4.0 * ((double)d.K * d.N + (double)d.M * d.K + (double)d.M * d.N * (d.square_a ? 2 : 1));
        sf += 2.0 * d.M * d.K * d.N;
    }
    sb += 12.0 * n_img * m0->M;
    m0->team_step_bytes = sb;
    m0->team_step_flops = sf;
    m0->team_key = key;
    return LBC_OK;
}

extern "C" {

int lbc_decode_team(lbc_model* const* ms, int n_teams, const uint8_t* const* streams, const size_t* lens, int n_img,
                    int Hb, int Wb, float* const* zhat_devs, void* stream) {
    if (!ms || !streams || !lens || !zhat_devs) return set_error(LBC_E_ARG, "null argument");
    if (n_teams < 1 || n_teams > TEAM_MAX) return set_error(LBC_E_ARG, "1 to 16 image sets per team decode");
    if (n_img <= 0 || Hb <= 0 || Wb <= 0) return set_error(LBC_E_ARG, "empty frame");
    const int T = n_teams;
    for (int t = 0; t < T; ++t) {
        lbc_model* m = ms[t];
        if (!m || !zhat_devs[t]) return set_error(LBC_E_ARG, "null handle or output");
        if (int rc = check_entry(m, true, true, true)) return rc;
        for (int u = 0; u < t; ++u)
            if (ms[u] == m) return set_error(LBC_E_ARG, "every batch needs its own handle (lbc_create_sibling)");
        if (m->B != ms[0]->B || m->N != ms[0]->N || m->M != ms[0]->M || m->P != ms[0]->P || m->l0_on != ms[0]->l0_on ||
            m->cfg.device != ms[0]->cfg.device)
            return set_error(LBC_E_ARG, "team decode handles must share one geometry and device");
    }
    const bool team_off = env_int("LBIC_TEAM", 1) == 0;
    if (T == 1 && n_img == 1 && !team_off) {
        // one image: the whole chip is its team -- lbc_decode runs the single-image decoder (k_dec_one) where it
        // applies, else the row graphs (faster than a team of 32 or 64 workgroups for one image: 0.59 vs 0.75 s per
        // 768x768 frame, profiles/r04/r04_c5_b1_s*.log)
        const int rc1 = lbc_decode(ms[0], streams, lens, 1, Hb, Wb, zhat_devs[0], stream);
        if (rc1) return rc1;
        ms[0]->team_mode_last = ms[0]->dec_path_last == 1 ? 3 : 4;
        ms[0]->team_launch_bytes = ms[0]->team_launch_flops = 0;
        ms[0]->team_plain_last = -1;    // no team launch: lbc_team_stats reports the decode's own events (ev[2..3])
        return LBC_OK;
    }
    int sparse = rans_sparse_choice(lens, T * n_img, (double)T * n_img * Hb * Wb * ms[0]->M);
    const double zbytes = (double)n_img * (Hb + 2) * (Wb + 4) * ms[0]->Cx * 4;
    const double lbytes = ms[0]->l0_on ? (double)n_img * (Hb + 2) * (Wb + 4) * ms[0]->C1P * 4 : 0.0;
    if (team_off || ms[0]->M > 256 || zbytes >= 4294967296.0 || lbytes >= 4294967296.0)
        return team_fallback(ms, T, streams, lens, n_img, Hb, Wb, zhat_devs, stream);
    std::lock_guard<std::mutex> team_lock(g_team_mu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    lbc_model* m0 = ms[0];
    int rc;
    int dev = m0->cfg.device, cus = 0;
    HIPCHK(hipSetDevice(dev));
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    for (int t = 0; t < T; ++t) {
        lbc_model* m = ms[t];
        if ((rc = prepare_device(m))) return rc;
        if ((rc = ensure_workspace(m, n_img, Hb, Wb, s))) return rc;
        if ((rc = m->ctr.alloc(sizeof(int)))) return rc;
        std::vector<std::pair<const uint8_t*, size_t>> subs;
        for (int i = 0; i < n_img; ++i) subs.emplace_back(streams[(size_t)t * n_img + i], lens[(size_t)t * n_img + i]);
        if ((rc = upload_streams(m, subs, s))) return rc;
    }
    // team geometry: grid 8 x S, one XCD slot per team, S = one (or, LBC_OPT_TEAM_WG_PER_CU, two) workgroups per CU
    // of an XCD.  The whole grid must be resident (team barriers): the occupancy query below uses the kernel instance
    // and the dynamic LDS of the launch, and a geometry that does not fit is shrunk (two workgroups per CU -> one) or
    // decoded by lbc_decode per batch.
    int wpc = std::max(1, m0->team_wpc);
    int S = 0, spread = 1, sub = 1;
    TeamArgs a{};
    for (;;) {
        // more than 8 teams: two per XCD slot, each half the slot's CUs
        sub = T > TEAM_SLOTS ? 2 : 1;
        S = std::min(32, cus / TEAM_SLOTS) / sub * wpc;
        if (m0->team_size > 0) S = std::min(S, m0->team_size * wpc);
        // at most four batches: each team takes two XCDs (twice the workgroups, write-through hand-offs; 4 batches
        // alone: 0.917 vs 0.969 s per launch, profiles/r02_exp/team_spread.txt); LBIC_TEAM_SPREAD=P (1, 2, 4, 8 with
        // T <= 8 / P) sets the XCD slots per team (A/B runs)
        spread = T <= TEAM_SLOTS / 2 ? 2 : 1;
        const int p = (int)env_int("LBIC_TEAM_SPREAD", 0);
        if ((p == 1 || p == 2 || p == 4 || p == 8) && T <= TEAM_SLOTS / p) spread = p;
        S *= spread;
        if (S < 1) return team_fallback(ms, T, streams, lens, n_img, Hb, Wb, zhat_devs, stream);
        if ((rc = team_record(ms, T, n_img, Hb, Wb, S, spread, sparse, s))) return rc;
        a = m0->team_args;
        // high rates: the tables staged in every workgroup's LDS (rans_row<true>); low rates: rans_row_sparse, its rare
        // far symbols searched in the table image in global memory
        a.dense = sparse ? 0 : 1;
        size_t lds = team_lds_bytes(a);
        if (lds > 160 * 1024 && a.dense) {
            // the dense tables do not fit beside this geometry's partials (high rates with many tiles per workgroup):
            // the sparse coder -- tables read from global memory, any rate, bit-identical -- instead of the row graphs
            sparse = 1;
            if ((rc = team_record(ms, T, n_img, Hb, Wb, S, spread, sparse, s))) return rc;
            a = m0->team_args;
            a.dense = 0;
            lds = team_lds_bytes(a);
        }
        if (lds > 160 * 1024) return team_fallback(ms, T, streams, lens, n_img, Hb, Wb, zhat_devs, stream);
        const int nb = team_blocks_per_cu(a.dense, lds);
        if (nb >= wpc) break;
        if (nb < 1 || wpc == 1) return team_fallback(ms, T, streams, lens, n_img, Hb, Wb, zhat_devs, stream);
        wpc = nb;
    }
    // test hook: s_memrealtime ticks one barrier waits (default 1 s)
    a.tmo = (unsigned long long)std::max(1ll, env_int("LBIC_TEAM_TMO", 100000000ll));
    a.ts = env_int("LBIC_TEAM_STAMPS", 0) ? m0->team_ts.as<unsigned long long>() : nullptr;
    a.sv = Hb / 2;
    a.sh = Wb / 2;
    // plain hand-off stores unless LBIC_TEAM_SC1=1 (or a spread / column-split geometry); a launch that finds a team
    // spread over XCDs stops before its first operation (failure word 2, nothing decoded yet) and is rerun with
    // write-through hand-offs
    a.plain = env_int("LBIC_TEAM_SC1", 0) || a.spread > 1 ? 0 : 1;
    unsigned fail = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        for (int t = 0; t < T; ++t)
            if ((rc = reset_frame(ms[t], n_img, Hb, Wb, s))) return rc;
        HIPCHK(hipMemsetAsync(m0->team_sync.p, 0, (size_t)(TEAM_MAX + 2) * 32 * sizeof(unsigned), s));
        if (a.ts) HIPCHK(hipMemsetAsync(m0->team_ts.p, 0, (size_t)TEAM_MAX * TEAM_TS_WORDS * sizeof(unsigned long long), s));
        HIPCHK(hipEventRecord(m0->ev[2], s));
        if ((rc = launch_dec_team(a, s))) return rc;
        HIPCHK(hipEventRecord(m0->ev[3], s));
        HIPCHK(hipMemcpyAsync(&fail, m0->team_sync.as<unsigned>() + T * 32, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (fail != 2 || !a.plain) break;
        a.plain = 0;
        m0->team_fallbacks += 1;
    }
    if (fail == 1) {
        // a workgroup gave up waiting at a team barrier (the grid was not co-resident in time: another process or
        // stream held CUs past the timeout).  Nothing is wrong with the streams: decode the batches again through
        // lbc_decode one after another (it re-uploads the streams and resets the workspaces), and count the event.
        m0->team_timeouts += 1;
        static std::atomic<bool> noted{false};
        if (!noted.exchange(true) || env_int("LBIC_TEAM_VERBOSE", 0))
            fprintf(stderr, "[lbic] team decode: barrier timeout, decoding through lbc_decode (counted: lbc_team_events)\n");
        return team_fallback(ms, T, streams, lens, n_img, Hb, Wb, zhat_devs, stream, true);
    }
    if (fail)   // any other failure word is a protocol error, not a residency problem: report it
        return set_error(LBC_E_STATE, "team decode: unexpected failure word " + std::to_string(fail));
    m0->team_plain_last = a.plain;
    m0->team_mode_last = a.dense == 1 ? 2 : 1;
    m0->team_launch_bytes = m0->team_step_bytes * T * Hb * Wb;
    m0->team_launch_flops = m0->team_step_flops * T * Hb * Wb;
    m0->dec_timed = true;
    for (int t = 0; t < T; ++t)
        if ((rc = launch_copy_interior(ms[t]->zpad.as<float>(), zhat_devs[t], n_img, Hb, Wb, ms[t]->Cx, s))) return rc;
    if (a.ts) {
        m0->team_ts_host.assign((size_t)T * TEAM_TS_WORDS, 0ull);
        HIPCHK(hipMemcpyAsync(m0->team_ts_host.data(), m0->team_ts.p, (size_t)T * TEAM_TS_WORDS * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (env_int("LBIC_TEAM_VERBOSE", 0))
        fprintf(stderr, "[lbic] team decode: T=%d S=%d plain=%d reruns=%d lds=%zu\n", T, S, a.plain, m0->team_fallbacks,
                team_lds_bytes(a));
    for (int t = 0; t < T; ++t)
        if ((rc = check_status(ms[t], (size_t)n_img, s, true))) return rc;
    return LBC_OK;
}

int lbc_team_stats(const lbc_model* m, double* launch_ms, double* bytes, double* flops, int* plain) {
    if (!m || !launch_ms || !bytes || !flops || !plain) return set_error(LBC_E_ARG, "null argument");
    float ms = 0.f;
    if (m->dec_timed && m->ev[2]) HIPCHK(hipEventElapsedTime(&ms, m->ev[2], m->ev[3]));
    *launch_ms = ms;
    *bytes = m->team_launch_bytes;
    *flops = m->team_launch_flops;
    *plain = m->team_plain_last;
    return LBC_OK;
}

int lbc_team_mode(const lbc_model* m, int* mode) {
    if (!m || !mode) return set_error(LBC_E_ARG, "null argument");
    *mode = m->team_mode_last;
    return LBC_OK;
}

int lbc_team_events(const lbc_model* m, int* sc1_reruns, int* timeouts) {
    if (!m || !sc1_reruns || !timeouts) return set_error(LBC_E_ARG, "null argument");
    *sc1_reruns = m->team_fallbacks;
    *timeouts = m->team_timeouts;
    return LBC_OK;
}

int lbc_team_stamps(const lbc_model* m, unsigned long long* out, int max_out, int* n_out) {
    if (!m || !n_out) return set_error(LBC_E_ARG, "null argument");
    const int n = (int)m->team_ts_host.size();
    *n_out = n;
    if (out)
        for (int i = 0; i < n && i < max_out; ++i) out[i] = m->team_ts_host[i];
    return LBC_OK;
}

}  // extern "C"
