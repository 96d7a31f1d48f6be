// liblbic.so host side, the encoder: lbc_encode(_ex) (the closed loop as one captured wavefront graph), the band
// pipeline for frames split over GPUs, and lbc_forward (teacher-forced, every block at once).
#include "model.h"

using namespace lbic;

static int hip_rc(hipError_t e) {   // for code that must not return early (inside a stream capture)
    return e == hipSuccess ? LBC_OK : set_error(LBC_E_HIP, hipGetErrorString(e));
}

// Encoder graph fork: each wavefront step's context net (4 GEMMs) and the transform's first six GEMMs are independent
// (only the quantising GEMM reads the means / scales), so they are captured as two branches joined before it.
// Encoder alone 98.7 -> 95.0 ms per 32-frame batch, bit-identical; beside the team decoder within noise (+0.3..0.9 %;
// profiles/r02_exp/encoder_fork_team.txt).  Only for passes whose largest wavefront step has at most ENC_FORK_MAX_ROWS
// rows: a 128-frame pass's launches fill the chip for several rounds each, and two branches then only compete (bench,
// four batches per pass: 136.0 / 133.3 Mpix/s with one chain vs 132.9 / 131.5 forked, profiles/r06/exp/fs_*).
// LBIC_ENC_FORK=0 / 1 forces it (with four busy streams, the workers schedule, the branch's extra hardware queue cost
// 5 %: profiles/r02_exp/encoder_fork.txt).
// (LBC_OPT_ENC_FORK: -1 this rule, 0 / 1 forced)
constexpr int ENC_FORK_MAX_ROWS = 2048;
static bool enc_fork_on(int mmax, int opt) {
    const long long e = env_int("LBIC_ENC_FORK", -1);
    if (e >= 0) return e != 0;
    return opt >= 0 ? opt != 0 : mmax <= ENC_FORK_MAX_ROWS;
}

// the encoder's results, from the library-owned buffers the graphs write to the caller's tensors
static int copy_codes_out(lbc_model* m, size_t nsym, int32_t* sym_dev, int32_t* idx_dev, float* bits_dev, hipStream_t s) {
    HIPCHK(hipMemcpyAsync(sym_dev, m->sym_buf.p, nsym * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(idx_dev, m->idx_buf.p, nsym * 4, hipMemcpyDeviceToDevice, s));
    if (bits_dev) HIPCHK(hipMemcpyAsync(bits_dev, m->bits_buf.p, nsym * 4, hipMemcpyDeviceToDevice, s));
    return LBC_OK;
}

extern "C" {

int lbc_encode(lbc_model* m, const float* x_dev, int n_img, int Hb, int Wb, float* zhat_dev, int32_t* sym_dev,
               int32_t* idx_dev, float* bits_dev, void* stream) {
    return lbc_encode_ex(m, x_dev, n_img, Hb, Wb, zhat_dev, sym_dev, idx_dev, bits_dev, 0, stream);
}

int lbc_encode_ex(lbc_model* m, const float* x_dev, int n_img, int Hb, int Wb, float* zhat_dev, int32_t* sym_dev,
                  int32_t* idx_dev, float* bits_dev, int flags, void* stream) {
    if (flags & ~LBC_ENC_FRAME_PAD) return set_error(LBC_E_ARG, "unknown encode flags");
    const bool frame_pad = (flags & LBC_ENC_FRAME_PAD) != 0;
    // the validation loop (frame_pad) uses forward()'s likelihood, not the CDFs: it runs before update()
    // too (scale indexes are then not produced)
    int rc = check_entry(m, x_dev && zhat_dev && sym_dev && idx_dev, !frame_pad, n_img > 0 && Hb > 0 && Wb > 0);
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if ((rc = prepare_device(m))) return rc;
    if ((rc = ensure_workspace(m, n_img, Hb, Wb, s))) return rc;
    const size_t nx = (size_t)n_img * Hb * Wb * m->Cx, nsym = (size_t)n_img * Hb * Wb * m->M;
    if ((rc = m->x_in.alloc(nx * 4)) || (rc = m->sym_buf.alloc(nsym * 4)) || (rc = m->idx_buf.alloc(nsym * 4)) ||
        (rc = m->bits_buf.alloc(nsym * 4)))
        return rc;
    // the graph works on library-owned buffers only, so it survives new caller tensors
    const std::vector<long long> key = {n_img, Hb, Wb, (long long)m->x_in.p, (long long)m->zpad.p,
                                        (long long)m->sym_buf.p, (long long)m->work.ctx0.p,
                                        (long long)m->table_dev.p, m->prof.sample_every, flags,
                                        m->enc_lds_floor, m->enc_fork};
    if (!m->enc_exec || key != m->enc_key) {
        rc = capture_graph(m, "encoder", 0, &m->enc_exec, [&]() -> int {
            int crc = LBC_OK;
            Work& w = m->work;
            int32_t *sym = m->sym_buf.as<int32_t>(), *idx = m->idx_buf.as<int32_t>();
            float* bits = m->bits_buf.as<float>();
            const int4* blocks = m->blocks_enc.as<int4>();
            const bool fork = enc_fork_on(m->Mmax, m->enc_fork);   // (sampled: launch spans only, no launch-to-launch period)
            m->prof.nochain = fork;
            for (size_t t = 0; t < m->step_off.size(); ++t)
                if (m->step_cnt[t] > w.rows) crc = set_error(LBC_E_STATE, "encoder workspace too small");
            for (size_t t = 0; t < m->step_off.size() && !crc; ++t) {
                m->prof.step(m->prof.sample_every > 0 && (t % m->prof.sample_every) == 0);
                GemmArgs g = base_args(m, blocks + m->step_off[t], m->step_cnt[t], m->x_in.as<float>(), Hb, Wb);
                const int4* cells = m->l0_on ? m->cells_enc.as<int4>() + m->cell_off[t] : nullptr;
                const int ncells = m->l0_on ? m->cell_cnt[t] : 0;
                if (fork) {
                    // fork: the context net on cap2, the transform's first layers on cap; join before quantising
                    if (!crc) crc = hip_rc(hipEventRecord(m->fev[0], m->cap));
                    if (!crc) crc = hip_rc(hipStreamWaitEvent(m->cap2, m->fev[0], 0));
                    if (!crc) crc = run_ctx(m, w, g, false, m->cap2, frame_pad, cells, ncells);
                    if (!crc) crc = hip_rc(hipEventRecord(m->fev[1], m->cap2));
                    if (!crc) crc = run_enc(m, w, g, nullptr, nullptr, nullptr, m->cap, 1);
                    if (!crc) crc = hip_rc(hipStreamWaitEvent(m->cap, m->fev[1], 0));
                    if (!crc) crc = run_enc(m, w, g, sym, idx, bits, m->cap, 2);
                } else {
                    if (!crc) crc = run_ctx(m, w, g, false, m->cap, frame_pad, cells, ncells);
                    if (!crc) crc = run_enc(m, w, g, sym, idx, bits, m->cap);
                }
                if (!crc) crc = run_dec(m, w, g, m->cap);
            }
            m->prof.used0 = m->prof.next;   // (the ENCODER graph's range-0 slots: set by this capture only)
            return crc;
        });
        if (rc) return rc;
        m->enc_key = key;
    }
    HIPCHK(hipEventRecord(m->ev[0], s));
    HIPCHK(hipMemcpyAsync(m->x_in.p, x_dev, nx * 4, hipMemcpyDeviceToDevice, s));
    if ((rc = reset_frame(m, n_img, Hb, Wb, s, frame_pad))) return rc;
    HIPCHK(hipGraphLaunch(m->enc_exec, s));
    m->prof.replays[0] += 1;
    if (m->prof.sample_every && m->prof.slots && m->prof.snap && m->prof.used0 > 0 && m->prof.nsnap < Prof::kSnaps) {
        // this replay's stamps, before the next replay zeroes them (stream order)
        HIPCHK(hipMemcpyAsync(m->prof.snap + (size_t)m->prof.nsnap * kSlotsPerRange * kSlotU64, m->prof.slots,
                              (size_t)m->prof.used0 * kSlotU64 * 8, hipMemcpyDeviceToHost, s));
        m->prof.nsnap += 1;
    }
    if ((rc = launch_copy_interior(m->zpad.as<float>(), zhat_dev, n_img, Hb, Wb, m->Cx, s))) return rc;
    if ((rc = copy_codes_out(m, nsym, sym_dev, idx_dev, bits_dev, s))) return rc;
    HIPCHK(hipEventRecord(m->ev[1], s));
    m->enc_timed = true;
    return LBC_OK;
}

// ---------------------------------------------------------------- band pipeline for frames split over GPUs
// Block rows [v0, v0 + Hb_band) of n_img frames.  The workspace is the band's: zpad rows 0..1 (the zero border of a
// whole frame) hold the two block rows above the band, which the caller hands over before every step range.
int lbc_band_begin(lbc_model* m, const float* x_dev, int n_img, int Hb_band, int Wb, int v0, void* stream) {
    int rc = check_entry(m, x_dev, true, n_img > 0 && Hb_band > 0 && Wb > 0 && v0 >= 0, "empty band");
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if ((rc = prepare_device(m))) return rc;
    if ((rc = ensure_workspace(m, n_img, Hb_band, Wb, s))) return rc;
    const size_t nx = (size_t)n_img * Hb_band * Wb * m->Cx, nsym = (size_t)n_img * Hb_band * Wb * m->M;
    if ((rc = m->x_in.alloc(nx * 4)) || (rc = m->sym_buf.alloc(nsym * 4)) || (rc = m->idx_buf.alloc(nsym * 4)) ||
        (rc = m->bits_buf.alloc(nsym * 4)))
        return rc;
    // the step-range graphs hold workspace pointers: rebuilt when any of them (or the band) changed
    const std::vector<long long> key = {n_img, Hb_band, Wb, v0, (long long)m->x_in.p, (long long)m->zpad.p,
                                        (long long)m->sym_buf.p, (long long)m->work.ctx0.p,
                                        (long long)m->table_dev.p, (long long)m->net.get()};
    if (key != m->band_key) {
        m->band_key = key;
        for (auto& kv : m->band_exec) (void)hipGraphExecDestroy(kv.second);
        m->band_exec.clear();
    }
    m->band_v0 = v0;
    HIPCHK(hipMemcpyAsync(m->x_in.p, x_dev, nx * 4, hipMemcpyDeviceToDevice, s));
    return zero_zpad(m, n_img, Hb_band, Wb, s);    // (no layer-0 cache in a band: lbc_band_run)
}

// two block rows [n_img][2][Wb][Cx] <-> zpad rows r0, r0 + 1 (interior columns)
static int band_rows_copy(lbc_model* m, float* rows, int r0, bool to_zpad, hipStream_t s) {
    const size_t w = (size_t)m->ws_Wb * m->Cx * sizeof(float), pitch = (size_t)(m->ws_Wb + 4) * m->Cx * sizeof(float);
    for (int i = 0; i < m->ws_n; ++i) {
        float* z = m->zpad.as<float>() + (((size_t)i * (m->ws_Hb + 2) + r0) * (m->ws_Wb + 4) + 2) * m->Cx;
        float* h = rows + (size_t)i * 2 * m->ws_Wb * m->Cx;
        HIPCHK(to_zpad ? hipMemcpy2DAsync(z, pitch, h, w, w, 2, hipMemcpyDeviceToDevice, s)
                       : hipMemcpy2DAsync(h, w, z, pitch, w, 2, hipMemcpyDeviceToDevice, s));
    }
    return LBC_OK;
}

int lbc_band_run(lbc_model* m, int t0, int t1, const float* halo_dev, float* edge_dev, void* stream) {
    if (!m || m->band_v0 < 0) return set_error(LBC_E_STATE, "lbc_band_begin() not called");
    if (t1 < t0) return set_error(LBC_E_ARG, "bad step range");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc;
    if (halo_dev && (rc = band_rows_copy(m, const_cast<float*>(halo_dev), 0, true, s))) return rc;
    // global step t codes block (v, h) with h + 2 v = t: the band's local step t - 2 v0
    const int T = (int)m->step_off.size();
    const int a = std::max(0, t0 - 2 * m->band_v0), b = std::min(T, t1 - 2 * m->band_v0);
    if (a < b) {
        auto it = m->band_exec.find({a, b});
        if (it == m->band_exec.end()) {
            hipGraphExec_t ex = nullptr;
            rc = capture_graph(m, "band", -1, &ex, [&]() -> int {     // (not profiled)
                int crc = LBC_OK;
                const int4* blocks = m->blocks_enc.as<int4>();
                for (int t = a; t < b && !crc; ++t) {
                    GemmArgs g = base_args(m, blocks + m->step_off[t], m->step_cnt[t], m->x_in.as<float>(), m->ws_Hb, m->ws_Wb);
                    // layer 0 at five positions (no layer-0 cache): the band's row -1 is real data, not the frame border
                    crc = run_ctx(m, m->work, g, false, m->cap);
                    if (!crc) crc = run_enc(m, m->work, g, m->sym_buf.as<int32_t>(), m->idx_buf.as<int32_t>(),
                                            m->bits_buf.as<float>(), m->cap);
                    if (!crc) crc = run_dec(m, m->work, g, m->cap);
                }
                return crc;
            });
            if (rc) return rc;
            it = m->band_exec.emplace(std::make_pair(a, b), ex).first;
        }
        HIPCHK(hipGraphLaunch(it->second, s));
    }
    if (edge_dev && (rc = band_rows_copy(m, edge_dev, m->ws_Hb, false, s))) return rc;
    return LBC_OK;
}

int lbc_band_end(lbc_model* m, float* zhat_dev, int32_t* sym_dev, int32_t* idx_dev, float* bits_dev, void* stream) {
    if (!m || m->band_v0 < 0) return set_error(LBC_E_STATE, "lbc_band_begin() not called");
    if (!zhat_dev || !sym_dev || !idx_dev) return set_error(LBC_E_ARG, "null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc;
    if ((rc = launch_copy_interior(m->zpad.as<float>(), zhat_dev, m->ws_n, m->ws_Hb, m->ws_Wb, m->Cx, s))) return rc;
    if ((rc = copy_codes_out(m, (size_t)m->ws_n * m->ws_Hb * m->ws_Wb * m->M, sym_dev, idx_dev, bits_dev, s))) return rc;
    m->band_v0 = -1;
    return LBC_OK;
}

int lbc_forward(lbc_model* m, const float* x_dev, const float* zhat_dev, int n_img, int Hb, int Wb, float* xhat_dev,
                float* info_dev, void* stream) {
    // (no CDFs needed)
    int rc = check_entry(m, x_dev && zhat_dev && xhat_dev && info_dev, false, n_img > 0 && Hb > 0 && Wb > 0);
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if ((rc = prepare_device(m))) return rc;
    if ((rc = ensure_workspace(m, n_img, Hb, Wb, s))) return rc;
    const size_t nsym = (size_t)n_img * Hb * Wb * m->M;
    if ((rc = m->sym_buf.alloc(nsym * 4)) || (rc = m->idx_buf.alloc(nsym * 4))) return rc;
    // teacher forcing: the given zhat is the reconstruction every block sees (zero border as before)
    if ((rc = zero_zpad(m, n_img, Hb, Wb, s))) return rc;
    if ((rc = launch_fill_interior(zhat_dev, m->zpad.as<float>(), n_img, Hb, Wb, m->Cx, s))) return rc;
    // every block is independent here: chunks of the encoder workspace's row capacity, eager launches
    Work& w = m->work;
    const int total = n_img * Hb * Wb;
    const int4* blocks = m->blocks_enc.as<int4>();    // all blocks (wavefront order; outputs go by block)
    for (int off = 0; off < total && !rc; off += w.rows) {
        const int cnt = std::min(w.rows, total - off);
        GemmArgs g = base_args(m, blocks + off, cnt, x_dev, Hb, Wb);
        if (!rc) rc = run_ctx(m, w, g, false, s, true);
        if (!rc) rc = run_enc(m, w, g, m->sym_buf.as<int32_t>(), m->idx_buf.as<int32_t>(), info_dev, s);
        if (!rc) rc = run_dec(m, w, g, s, xhat_dev);
    }
    return rc;
}

}  // extern "C"
