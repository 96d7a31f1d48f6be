// Internal types of liblbic.so's host side: the handle (lbc_model) and what the files that work on it share (model.hip,
// step.hip, encode.hip, decode.hip, one_host.hip, team_host.hip; DESIGN.md section 1 says what each holds).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "kernels.h"
#include "lbic_internal.h"

namespace lbic {

#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) return set_error(LBC_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

// The environment's switches (test levers and diagnostics, listed in include/lbic.h) are all read through this: the
// integer value of `name`, dflt when it is absent or empty.  Read at every call: tests set and unset them between calls.
long long env_int(const char* name, long long dflt);

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    int alloc(size_t b) {
        if (b <= bytes && p) return LBC_OK;
        release();
        if (hipMalloc(&p, std::max<size_t>(b, 16)) != hipSuccess) {
            p = nullptr;
            return set_error(LBC_E_HIP, "hipMalloc failed");
        }
        bytes = b;
        return LBC_OK;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

struct Layer {
    DevBuf W, bias;
    int K = 0, N = 0, NB16 = 0;
};

// sampled per-kernel timing (lbc_profile_begin / lbc_profile_end): sampled launches stamp their span
// into a device slot {max(~start), max(end)}; one slot range per graph, zeroed at every replay
constexpr int kSlotsPerRange = 4096;
#ifdef LBIC_PHASE_DIAG
constexpr int kSlotU64 = 32;      // + per-phase max / sum / workgroup count (diagnostic build)
#else
constexpr int kSlotU64 = 16;      // 8 XCDs x {max(~start), max(end)}
#endif
constexpr int kRanges = 6;        // 0 encoder graph, 1 the decoder's row graph, 5 wavefront decoder graph (2..4 unused)
// kernel classes of the profile: gemm_class() (0 k_gemm_s, 1 k_gemm), 2 rANS, 3 copies
constexpr int kNClass = 4;
struct Prof {
    int sample_every = 0;
    bool active = false;          // current step is sampled
    // prev: slot of the launch before this one in the same sampled step of the same stream chain (-1: none),
    // so lbc_profile_end can also report the launch-to-launch period end(prev) -> end(this)
    struct Rec { int cls; int slot; double flops, bytes; int prev; };
    std::vector<Rec> recs;
    int last_slot = -1;
    unsigned long long* slots = nullptr;   // device, kRanges ranges
    int range = 0, next = 0;               // slot allocation inside the range being captured
    long long per_replay[8][kNClass] = {};       // launches of each kernel class per replay of each range's graph
    double work_replay[8][kNClass][2] = {};      // their algorithmic FLOPs and bytes per replay (every launch, sampled or not)
    long long replays[8] = {};             // replays of each range's graph since lbc_profile_begin
    bool nochain = false;                  // capturing a forked graph: no launch-to-launch period (two chains)
    // the encoder graph's slot range (0) copied to the host after EVERY replay since lbc_profile_begin (its stamps are
    // zeroed at the head of each replay): lbc_profile_end averages over all of them, not only the last replay
    int used0 = 0;                         // slots of range 0 the captured encoder graph uses
    unsigned long long* snap = nullptr;    // pinned host ring: kSnaps x kSlotsPerRange x kSlotU64 words
    int nsnap = 0;
    static constexpr int kSnaps = 64;
    unsigned long long* take() {
        if (!slots || next >= kSlotsPerRange) return nullptr;
        return slots + kSlotU64 * ((size_t)range * kSlotsPerRange + next++);
    }
    void step(bool on) {          // a new wavefront / raster step starts (sampled or not)
        active = on;
        last_slot = -1;
    }
    void add(int cls, const unsigned long long* ts, double flops, double bytes) {
        const int slot = (int)((ts - slots) / kSlotU64);
        recs.push_back({cls, slot, flops, bytes, nochain ? -1 : last_slot});
        last_slot = slot;
    }
};

struct HostT {
    std::vector<float> v;
    std::vector<int64_t> shape;
};

// the step workspace: the activations of one wavefront / raster step, shared by the encoder and every decoder
struct Work {
    int rows = 0;
    DevBuf ctx0, ctx1, ctx2, ksi, e0, e1, yq, d0, d1, idx;
};

// The packed device weights of one finalized state dict: shared (read-only) by every handle made from it with
// lbc_create_sibling, so several handles decoding side by side keep one copy in the Infinity Cache.  gen: a
// process-unique id of this packed set (recorded programs key on it: a new set may reuse freed addresses)
struct Net {
    Layer ctx0, ctx1, ctx2, ctx3, enc0, g0, e1, g1, e2, g2, e3, dec0, ig0, d1, ig1, d2, ig2, d3;
    long long gen = next_gen();
    static long long next_gen() {
        static std::atomic<long long> g{0};
        return ++g;
    }
};

inline constexpr int TAPS_A[4][2] = {{-1, -1}, {-1, 0}, {-1, 1}, {0, -1}};       // masked_conv2d.py:9-17 'A'
inline constexpr int TAPS_B[5][2] = {{-1, -1}, {-1, 0}, {-1, 1}, {0, -1}, {0, 0}};  // 'B' adds the centre

}  // namespace lbic

struct lbc_model {
    lbc_config cfg{};
    int B = 0, Cx = 0, N = 0, M = 0, N7 = 0, N6 = 0, C1 = 0, C2 = 0, C3 = 0, C4 = 0, P = 1;
    int NP = 0, C1P = 0, C2P = 0, C3P = 0;   // widths padded to 16 (activation row strides)
    std::map<std::string, lbic::HostT> host;
    bool finalized = false;
    std::shared_ptr<lbic::Net> net = std::make_shared<lbic::Net>();
    lbic::EntropyTables tabs;
    bool tabs_set = false;
    lbic::DevBuf table_dev, cdf16_dev, tmeta_dev;
    int total16 = 0;
    std::vector<uint16_t> c16_host;
    std::vector<int> meta_host;
    bool tabs_dirty = false;
    // per-shape workspace
    int ws_n = 0, ws_Hb = 0, ws_Wb = 0, Mmax = 0;
    lbic::DevBuf zpad, blocks_enc, blocks_dec;
    // layer-0 map cache of the context net (KS[1] = 3): cell (img, v, h) = LeakyReLU(layer 0) at block position
    // (v, h), zpad geometry [n_img][Hb+2][Wb+4][C1P]; cells_enc = the cells each wavefront step computes
    bool l0_on = false;
    lbic::DevBuf l0, cells_enc;
    std::vector<int> cell_off, cell_cnt;
    int enc_lds_floor = 0;      // LBC_OPT_ENC_LDS_FLOOR
    int enc_fork = -1;          // LBC_OPT_ENC_FORK
    int team_wpc = 1;           // LBC_OPT_TEAM_WG_PER_CU
    int team_size = 0;          // LBC_OPT_TEAM_SIZE (0: CUs / 8)
    lbic::Work work;
    std::vector<int> step_off, step_cnt;
    lbic::DevBuf words, word_base, word_count, st_x, st_ptr, st_status;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool enc_timed = false, dec_timed = false;
    lbic::Prof prof;
    // HIP graphs: the whole encoder wavefront (one replay per call), one block row of the raster decoder (replayed
    // Hb times; kernels take the row from the device counter `ctr`) and the whole decoder wavefront
    hipGraphExec_t enc_exec = nullptr, dec_exec = nullptr, wf_exec = nullptr;
    std::vector<long long> enc_key, dec_key, wf_key;
    lbic::DevBuf x_in, sym_buf, idx_buf, bits_buf, ctr;
    hipStream_t cap = nullptr;
    // encoder graph fork (LBIC_ENC_FORK=1): each wavefront step's context net is captured on cap2, beside the
    // encoder transform's first six GEMMs on cap; the quantising GEMM joins both
    hipStream_t cap2 = nullptr;
    hipEvent_t fev[2] = {nullptr, nullptr};
    // workspace set-up (ws_zero / dev_upload with a handle): a private non-blocking stream ordered after the caller's stream by
    // an event, never the legacy stream
    hipStream_t aux = nullptr;
    hipEvent_t aux_ev = nullptr;
    // band pipeline (lbc_band_*): this handle codes block rows [band_v0, band_v0 + ws_Hb) of taller frames;
    // one captured graph per range of global wavefront steps
    int band_v0 = -1;
    std::map<std::pair<int, int>, hipGraphExec_t> band_exec;
    std::vector<long long> band_key;
    // team decoder (lbc_decode_team, held by the first handle of a call): the recorded raster step of every
    // team, the barrier words, and the stamps of the last launch
    lbic::DevBuf team_prog, team_sync, team_ts;
    std::vector<long long> team_key;
    lbic::TeamArgs team_args{};
    std::vector<unsigned long long> team_ts_host;
    int team_fallbacks = 0, team_plain_last = -1;   // launches rerun write-through; mode of the last launch
    int team_timeouts = 0;    // team launches that timed out at a barrier and were decoded through lbc_decode instead
    bool no_one = false;      // lbc_decode skips k_dec_one (set by team_fallback after a residency timeout)
    int team_mode_last = 0;   // the last lbc_decode_team call: 0 lbc_decode per batch (a fallback), 1 team + sparse rANS,
                              // 2 team + dense, one batch of one image through lbc_decode: 3 its single-image decoder
                              // (k_dec_one), 4 its row graphs
    double team_step_bytes = 0, team_step_flops = 0;  // algorithmic work of one team's raster step (inner column)
    double team_launch_bytes = 0, team_launch_flops = 0;
    // single-image decoder (k_dec_one, one.hip; lbc_decode of one image): the step's operations, the weight-tile
    // placement over the grid, the granule buffers and the failure word
    lbic::DevBuf one_ops, one_tiles, one_gran, one_fail, one_rans, one_ts;
    std::vector<unsigned long long> one_ts_host;
    std::vector<long long> one_key;
    lbic::OneArgs one_args{};
    int one_grid = 0;
    int one_ok = 0;             // the placement fits (0: lbc_decode keeps the graph decoder for single images)
    int dec_path_last = 0;      // the last lbc_decode: 0 the row graphs, 1 k_dec_one
    int one_timeouts = 0;       // k_dec_one launches that timed out and were decoded by the row graphs instead
};

namespace lbic {

// ---- model.hip
int dev_upload(DevBuf& d, const void* src, size_t bytes, lbc_model* m = nullptr, hipStream_t s = nullptr);
int ensure_workspace(lbc_model* m, int n_img, int Hb, int Wb, hipStream_t s);
int prepare_device(lbc_model* m);
inline size_t zpad_bytes(const lbc_model* m, int n_img, int Hb, int Wb) {
    return (size_t)n_img * (Hb + 2) * (Wb + 4) * m->Cx * sizeof(float);
}
int zero_zpad(lbc_model* m, int n_img, int Hb, int Wb, hipStream_t s);
int reset_frame(lbc_model* m, int n_img, int Hb, int Wb, hipStream_t s, bool frame_pad = false);
int check_entry(const lbc_model* m, bool args_ok, bool need_tabs, bool dims_ok, const char* empty = "empty frame");

// ---- step.hip
// Recording mode (lbc_decode_team): gemm() prepares the arguments as launch_gemm would and appends them to the
// program instead of launching; the team kernel replays them for every raster step.
struct Recorder {
    std::vector<GemmArgs> gemms;
    std::vector<int> ops;     // >= 0: GEMM index, -1: the rANS decode
};
extern thread_local Recorder* g_rec;
GemmArgs base_args(lbc_model* m, const int4* blocks, int rows, const float* x, int Hb, int Wb);
int run_ctx(lbc_model* m, Work& w, GemmArgs g, bool with_idx, hipStream_t s, bool frame_pad = false,
            const int4* cells = nullptr, int ncells = 0);
int run_dec(lbc_model* m, Work& w, GemmArgs g, hipStream_t s, float* xhat = nullptr);
int run_enc(lbc_model* m, Work& w, GemmArgs g, int32_t* sym, int32_t* idx, float* bits, hipStream_t s, int part = 0);
RansArgs rans_args(lbc_model* m);
RansArgs rans_step_args(lbc_model* m, int rows, int sparse);
int rans_step(lbc_model* m, RansArgs r, hipStream_t s);
int capture_graph(lbc_model* m, const char* label, int range, hipGraphExec_t* exec, const std::function<int()>& body);

// ---- decode.hip
int upload_streams(lbc_model* m, const std::vector<std::pair<const uint8_t*, size_t>>& subs, hipStream_t s);
int rans_sparse_choice(const size_t* lens, int n, double symbols);
int check_status(lbc_model* m, size_t n, hipStream_t s, bool full);

// ---- one_host.hip
int decode_one(lbc_model* m, int Hb, int Wb, hipStream_t s, int* used);

}  // namespace lbic
