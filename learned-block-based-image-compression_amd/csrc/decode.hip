// liblbic.so host side, the graph decoders: bitstream upload and the end-of-stream check, lbc_decode (the reference's
// raster order, one block row per graph replay; one image goes to k_dec_one first), lbc_rans_decode_gpu, and the
// sub-stream container with its wavefront decoder (lbc_rans_encode_rows / lbc_decode_rows).
#include <cstdlib>
#include <cstring>

#include "model.h"

namespace lbic {

// Upload rANS (sub-)streams: concatenated words, per-stream base / count, and the initial state of each
// (Rans64DecInit: the first two words).  The word buffer is baked into the decoder graphs, so it grows
// with headroom to stay put across calls.
int upload_streams(lbc_model* m, const std::vector<std::pair<const uint8_t*, size_t>>& subs, hipStream_t s) {
    const size_t n = subs.size();
    std::vector<long long> base(n);
    std::vector<int> cnt(n), ptr(n, 2);
    std::vector<unsigned long long> x0(n);
    size_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!subs[i].first || subs[i].second < 8 || (subs[i].second & 3)) return set_error(LBC_E_STREAM, "invalid bitstream");
        if (subs[i].second / 4 > 0x7fffffff) return set_error(LBC_E_STREAM, "bitstream too long");
        base[i] = (long long)(total / 4);
        cnt[i] = (int)(subs[i].second / 4);
        total += subs[i].second;
        uint32_t w[2];
        std::memcpy(w, subs[i].first, 8);
        x0[i] = (unsigned long long)w[0] | ((unsigned long long)w[1] << 32);
    }
    int rc;
    // every allocation before the first queued copy: an error return below must not leave copies in flight
    // that read the local host arrays or the caller's borrowed buffers
    if (total > m->words.bytes && (rc = m->words.alloc(total + total / 2 + (1 << 20)))) return rc;
    // per-stream arrays: sized by the stream count, pointers kept stable for the graphs
    const size_t cap = std::max<size_t>(n, 64);
    if ((rc = m->word_base.alloc(cap * sizeof(long long))) || (rc = m->word_count.alloc(cap * sizeof(int))) ||
        (rc = m->st_x.alloc(cap * sizeof(unsigned long long))) || (rc = m->st_ptr.alloc(cap * sizeof(int))) ||
        (rc = m->st_status.alloc(cap * sizeof(int))))
        return rc;
    // each stream straight from the caller's buffer to its word offset (no host-side concatenation),
    // stream-ordered on the decoder's stream: the words are rewritten only after that stream's previous
    // graph (which reads them) has drained, whatever the stream's blocking flags.  The local arrays and the
    // borrowed buffers stay alive until the synchronisation below, on the error path as well.
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < n && e == hipSuccess; ++i)
        e = hipMemcpyAsync(static_cast<uint8_t*>(m->words.p) + (size_t)base[i] * 4, subs[i].first, subs[i].second,
                           hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m->word_base.p, base.data(), n * sizeof(long long), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m->word_count.p, cnt.data(), n * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m->st_x.p, x0.data(), n * sizeof(unsigned long long), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m->st_ptr.p, ptr.data(), n * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(m->st_status.p, 0, n * sizeof(int), s);
    const hipError_t es = hipStreamSynchronize(s);      // always: drains whatever was queued
    if (e != hipSuccess) return set_error(LBC_E_HIP, std::string("bitstream upload: ") + hipGetErrorString(e));
    if (es != hipSuccess) return set_error(LBC_E_HIP, std::string("bitstream upload sync: ") + hipGetErrorString(es));
    return LBC_OK;
}

// rANS decoder variant: the sparse one (centre-interval fast path, no LDS table image) when the streams average
// under 1 bit per symbol (LBIC_RANS_SPARSE=0 / 1 forces it)
int rans_sparse_choice(const size_t* lens, int n, double symbols) {
    const long long e = env_int("LBIC_RANS_SPARSE", -1);
    if (e >= 0) return e ? 1 : 0;
    double bytes = 0;
    for (int i = 0; i < n; ++i) bytes += (double)lens[i];
    return symbols > 0 && 8.0 * bytes / symbols < 1.0 ? 1 : 0;
}

// full: the decode consumed every block of every stream, so each rANS stream must end where its encoder began: state
// RANS64_L = 2^31 (Rans64EncInit; the decoder retraces the encoder's states in reverse).  A truncated stream overruns
// (status); a corrupted one ends in another state with near certainty -- both raise.  Words past the last one read
// (trailing padding) are ignored, as CompressAI's RansDecoder ignores them (lbic.h, lbc_decode).
int check_status(lbc_model* m, size_t n, hipStream_t s, bool full) {
    std::vector<int> status(n), ptr(full ? n : 0), cnt(full ? n : 0);
    std::vector<unsigned long long> x(full ? n : 0);
    HIPCHK(hipMemcpyAsync(status.data(), m->st_status.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
    if (full) {
        HIPCHK(hipMemcpyAsync(x.data(), m->st_x.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(ptr.data(), m->st_ptr.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(cnt.data(), m->word_count.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; ++i) {
        if (status[i]) return set_error(LBC_E_STREAM, "corrupt bitstream (stream " + std::to_string(i) + ")");
        if (full && (x[i] != (1ull << 31) || ptr[i] > cnt[i]))
            return set_error(LBC_E_STREAM, "corrupt bitstream (stream " + std::to_string(i) +
                                               ": the decode does not end in the encoder's initial state)");
    }
    return LBC_OK;
}

}  // namespace lbic

using namespace lbic;

// the raster decoder's block row as one captured graph: Wb raster steps (context net -> rANS -> decoder transform, 13
// launches each) whose kernels read the row from the device counter, which the graph's last node advances
static int capture_dec_row(lbc_model* m, int n_img, int Hb, int Wb, int sparse) {
    return capture_graph(m, "decoder", 1, &m->dec_exec, [&]() -> int {
        int crc = LBC_OK;
        RansArgs r = rans_step_args(m, n_img, sparse);
        r.ctr = m->ctr.as<int>();
        r.ctr_stride = Wb * n_img;
        for (int h = 0; h < Wb && !crc; ++h) {
            m->prof.step(m->prof.sample_every > 0 && (h % m->prof.sample_every) == 0);
            const int4* blocks = m->blocks_dec.as<int4>() + (size_t)h * n_img;
            GemmArgs g = base_args(m, blocks, n_img, nullptr, Hb, Wb);
            g.ctr = r.ctr;
            g.ctr_stride = r.ctr_stride;
            g.raster = 1;            // block of row r = (r, row counter, h): computed, not loaded
            g.raster_img0 = 0;
            g.raster_h = h;
            crc = run_ctx(m, m->work, g, true, m->cap);
            r.blocks = blocks;
            if (!crc) crc = rans_step(m, r, m->cap);
            if (!crc) crc = run_dec(m, m->work, g, m->cap);
        }
        if (!crc) crc = launch_ctr_add(m->ctr.as<int>(), 1, m->cap);
        return crc;
    });
}

static const uint32_t kRowsMagic = 0x3157424Cu;   // "LBW1"

extern "C" {

int lbc_decode(lbc_model* m, const uint8_t* const* streams, const size_t* lens, int n_img, int Hb, int Wb,
               float* zhat_dev, void* stream) {
    int rc = check_entry(m, streams && lens && zhat_dev, true, n_img > 0 && Hb > 0 && Wb > 0);
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if ((rc = prepare_device(m))) return rc;
    if ((rc = ensure_workspace(m, n_img, Hb, Wb, s))) return rc;
    std::vector<std::pair<const uint8_t*, size_t>> subs;
    for (int i = 0; i < n_img; ++i) subs.emplace_back(streams[i], lens[i]);
    auto start = [&]() -> int {
        if (int rc_ = upload_streams(m, subs, s)) return rc_;
        HIPCHK(hipEventRecord(m->ev[2], s));
        return reset_frame(m, n_img, Hb, Wb, s);
    };
    if ((rc = start())) return rc;
    m->dec_path_last = 0;
    if (n_img == 1) {     // one image: the persistent single-image decoder (one.hip) where it applies
        int used = 0;
        if ((rc = decode_one(m, Hb, Wb, s, &used))) return rc;
        if (used == 1) m->dec_path_last = 1;
        if (used == -1 && (rc = start())) return rc;    // a timed-out launch advanced the coder state: start again
    }
    if (m->dec_path_last == 0) {
        // the row graphs, on the caller's stream: one block row per replay, Hb replays
        if (n_img > m->work.rows) return set_error(LBC_E_STATE, "decoder workspace too small");
        if ((rc = m->ctr.alloc(sizeof(int)))) return rc;
        const int sparse = rans_sparse_choice(lens, n_img, (double)n_img * Hb * Wb * m->M);
        const std::vector<long long> key = {n_img, Hb, Wb, (long long)m->words.p, (long long)m->zpad.p,
                                            (long long)m->work.ctx0.p, (long long)m->table_dev.p,
                                            (long long)m->st_x.p, m->prof.sample_every, sparse};
        if (!m->dec_exec || key != m->dec_key) {
            if ((rc = capture_dec_row(m, n_img, Hb, Wb, sparse))) return rc;
            m->dec_key = key;
        }
        HIPCHK(hipMemsetAsync(m->ctr.p, 0, sizeof(int), s));
        for (int v = 0; v < Hb; ++v) HIPCHK(hipGraphLaunch(m->dec_exec, s));
        m->prof.replays[1] += Hb;
    }
    if ((rc = launch_copy_interior(m->zpad.as<float>(), zhat_dev, n_img, Hb, Wb, m->Cx, s))) return rc;
    HIPCHK(hipEventRecord(m->ev[3], s));
    m->dec_timed = true;
    return check_status(m, (size_t)n_img, s, true);
}

int lbc_rans_decode_gpu(lbc_model* m, const uint8_t* const* streams, const size_t* lens, int n_streams,
                        const int32_t* idx_dev, int n_chunks, int32_t* sym_dev, void* stream) {
    if (!m || !streams || !lens || !idx_dev || !sym_dev) return set_error(LBC_E_ARG, "null argument");
    if (!m->tabs_set) return set_error(LBC_E_NOT_UPDATED, "Uninitialized CDFs. Run update() first");
    if (n_streams <= 0 || n_chunks < 0) return set_error(LBC_E_ARG, "bad stream / chunk count");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc;
    if ((rc = prepare_device(m))) return rc;
    std::vector<std::pair<const uint8_t*, size_t>> subs;
    for (int i = 0; i < n_streams; ++i) subs.emplace_back(streams[i], lens[i]);
    if ((rc = upload_streams(m, subs, s))) return rc;
    RansArgs r = rans_args(m);
    r.rows = n_streams;
    double nsym = (double)n_streams * n_chunks * m->M;
    r.sparse = rans_sparse_choice(lens, n_streams, nsym);
    for (int c = 0; c < n_chunks && !rc; ++c) {
        r.idx = idx_dev + (size_t)c * n_streams * m->M;
        r.sym_out = sym_dev + (size_t)c * n_streams * m->M;
        rc = launch_rans_decode(r, s);
    }
    if (rc) return rc;
    return check_status(m, (size_t)n_streams, s, false);
}

int lbc_rans_encode_rows(const lbc_model* m, const int32_t* sym, const int32_t* idx, int Hb, int Wb, uint8_t** out,
                         size_t* len) {
    if (!m || !sym || !idx || !out || !len || Hb <= 0 || Wb <= 0) return set_error(LBC_E_ARG, "bad argument");
    if (!m->tabs_set) return set_error(LBC_E_NOT_UPDATED, "Uninitialized CDFs. Run update() first");
    const size_t per_row = (size_t)Wb * m->M;
    std::vector<std::vector<uint8_t>> rows(Hb);
    for (int v = 0; v < Hb; ++v) {
        int rc = rans_encode(m->tabs, sym + v * per_row, idx + v * per_row, per_row, rows[v]);
        if (rc) return rc;
    }
    size_t total = 8 + 4 * (size_t)Hb;
    for (auto& r : rows) total += r.size();
    uint8_t* buf = static_cast<uint8_t*>(malloc(total));
    uint32_t hdr[2] = {kRowsMagic, (uint32_t)Hb};
    std::memcpy(buf, hdr, 8);
    size_t off = 8 + 4 * (size_t)Hb;
    for (int v = 0; v < Hb; ++v) {
        const uint32_t n = (uint32_t)rows[v].size();
        std::memcpy(buf + 8 + 4 * (size_t)v, &n, 4);
        std::memcpy(buf + off, rows[v].data(), n);
        off += n;
    }
    *out = buf;
    *len = total;
    return LBC_OK;
}

int lbc_decode_rows(lbc_model* m, const uint8_t* const* streams, const size_t* lens, int n_img, int Hb, int Wb,
                    float* zhat_dev, void* stream) {
    int rc = check_entry(m, streams && lens && zhat_dev, true, n_img > 0 && Hb > 0 && Wb > 0);
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if ((rc = prepare_device(m))) return rc;
    if ((rc = ensure_workspace(m, n_img, Hb, Wb, s))) return rc;
    std::vector<std::pair<const uint8_t*, size_t>> subs;       // stream (img, v) at img * Hb + v
    for (int i = 0; i < n_img; ++i) {
        uint32_t hdr[2];
        if (!streams[i] || lens[i] < 8 + 4 * (size_t)Hb) return set_error(LBC_E_STREAM, "invalid sub-stream container");
        std::memcpy(hdr, streams[i], 8);
        if (hdr[0] != kRowsMagic || (int)hdr[1] != Hb) return set_error(LBC_E_STREAM, "not a sub-stream container for this frame");
        size_t off = 8 + 4 * (size_t)Hb;
        for (int v = 0; v < Hb; ++v) {
            uint32_t n;
            std::memcpy(&n, streams[i] + 8 + 4 * (size_t)v, 4);
            if (off + n > lens[i]) return set_error(LBC_E_STREAM, "truncated sub-stream container");
            subs.emplace_back(streams[i] + off, (size_t)n);
            off += n;
        }
    }
    if ((rc = upload_streams(m, subs, s))) return rc;
    // the whole anti-diagonal wavefront (the encoder's schedule) as one graph: per step, context net of
    // every block on the diagonal -> one wave per (image, block row) decodes that row's next block ->
    // decoder transform of every block
    std::vector<size_t> sub_lens;
    for (const auto& sb : subs) sub_lens.push_back(sb.second);
    const int sparse = rans_sparse_choice(sub_lens.data(), (int)sub_lens.size(), (double)n_img * Hb * Wb * m->M);
    const std::vector<long long> key = {n_img, Hb, Wb, (long long)m->words.p, (long long)m->zpad.p,
                                        (long long)m->work.ctx0.p, (long long)m->table_dev.p,
                                        (long long)m->st_x.p, m->prof.sample_every, sparse};
    if (!m->wf_exec || key != m->wf_key) {
        rc = capture_graph(m, "wavefront decoder", kRanges - 1, &m->wf_exec, [&]() -> int {
            int crc = LBC_OK;
            const int4* blocks = m->blocks_enc.as<int4>();
            for (size_t t = 0; t < m->step_off.size() && !crc; ++t) {
                m->prof.step(m->prof.sample_every > 0 && (t % m->prof.sample_every) == 0);
                const int rows = m->step_cnt[t];
                GemmArgs g = base_args(m, blocks + m->step_off[t], rows, nullptr, Hb, Wb);
                crc = run_ctx(m, m->work, g, true, m->cap, false,
                              m->l0_on ? m->cells_enc.as<int4>() + m->cell_off[t] : nullptr, m->l0_on ? m->cell_cnt[t] : 0);
                RansArgs r = rans_step_args(m, rows, sparse);
                r.blocks = blocks + m->step_off[t];
                r.streams_per_img = Hb;
                if (!crc) crc = rans_step(m, r, m->cap);
                if (!crc) crc = run_dec(m, m->work, g, m->cap);
            }
            return crc;
        });
        if (rc) return rc;
        m->wf_key = key;
    }
    HIPCHK(hipEventRecord(m->ev[2], s));
    if ((rc = reset_frame(m, n_img, Hb, Wb, s))) return rc;
    HIPCHK(hipGraphLaunch(m->wf_exec, s));
    m->prof.replays[kRanges - 1] += 1;
    if ((rc = launch_copy_interior(m->zpad.as<float>(), zhat_dev, n_img, Hb, Wb, m->Cx, s))) return rc;
    HIPCHK(hipEventRecord(m->ev[3], s));
    m->dec_timed = true;
    return check_status(m, subs.size(), s, true);
}

}  // extern "C"
