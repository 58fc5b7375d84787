// Internal header of the host side (ppg_plan / ppg_engine / ppg_stream / ppg_w2v2_host / ppg_frontend_host .hip): error
// reporting, small helpers, the event flags, the engine's structs, fork/join and launch timing, and the launch
// arguments of the PPG network's kernels, built once per kernel kind for the one-shot encode and the stream step alike.
#pragma once

#include "ppg_launch.h"

#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace ppg {

// Sets the calling thread's ppg_last_error() and returns `code`.  The one thread_local string of the library lives in
// ppg_engine.hip; the kernel files' launchers reach it under this name too.
int fail_message(int code, const char* fmt, ...);
inline int (&fail)(int, const char*, ...) = fail_message;

#define HIP_OK(expr) \
    do { if (hipError_t e_ = (expr); e_ != hipSuccess) return fail(PPG_EDEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)
#define LAUNCH_OK(expr, what) \
    do { if (hipError_t he_ = (expr); he_ != hipSuccess) return fail(PPG_EDEVICE, "%s: %s", what, hipGetErrorString(he_)); } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int round_up(int v, int a) { return (v + a - 1) / a * a; }

inline uint16_t host_bf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
// fp32 -> IEEE half, round to nearest even (subnormals and overflow to inf included)
inline uint16_t host_f16(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
inline float host_f16_to_f32(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }

// The events that fork a batch's pipelines from the caller's stream and join them into it order kernels of ONE device
// that read and write device memory: no system-scope fence (a record otherwise writes the caches back for the host and
// for peer devices to see -- every kernel already ends with the device-scope release that makes its results visible to
// the other XCDs, which is all the other pipeline's kernels need; a copy to the host or a collective behind the join
// brings its own fences).  Step 0.6750 -> 0.6700 ms, four alternations of three builds on one box
// (profiles/r6_fork_join_event_flags_ab.txt; hipEventReleaseToDevice alone: 0.6740).
constexpr unsigned kForkJoinEventFlags = hipEventDisableTiming | hipEventDisableSystemFence;
// ... and the timing events around a launch (the profiling getters) bracket the kernel, not a cache write-back for the host
constexpr unsigned kTimingEventFlags = hipEventDisableSystemFence;

struct EventPair { hipEvent_t a, b; };
// milliseconds between the events of the first `used` pairs (waits for them)
inline int elapsed_total(const std::vector<EventPair>& ev, size_t used, double* total_ms) {
    *total_ms = 0;
    for (size_t i = 0; i < used; ++i) {
        float ms = 0;
        HIP_OK(hipEventSynchronize(ev[i].b));
        HIP_OK(hipEventElapsedTime(&ms, ev[i].a, ev[i].b));
        *total_ms += ms;
    }
    return PPG_OK;
}

// Operand format of a packed weight matrix (ppg_pack.h)
enum class Fmt { F32, BF16, F16, F16X2 };   // F16X2: every 32 elements of a row as [32 fp16 hi | 32 fp16 lo] (PrecX2, ppg_device.h)
inline bool known_precision(int p) { return p == PPG_PRECISION_FP32 || p == PPG_PRECISION_BF16 || p == PPG_PRECISION_FP16 || p == PPG_PRECISION_FP16X2; }
inline Fmt operand_format(int precision) {
    return precision == PPG_PRECISION_FP16X2 ? Fmt::F16X2 : precision == PPG_PRECISION_FP16 ? Fmt::F16 : precision == PPG_PRECISION_BF16 ? Fmt::BF16 : Fmt::F32;
}
// The device of a create call: there must be one (nothing here has a CPU path) and `device` must name it; makes it current.
inline int use_device(int device, const char* what) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PPG_EDEVICE, "no HIP device: the %s has no CPU path", what);
    if (device < 0 || device >= ndev) return fail(PPG_EDEVICE, "device %d of %d", device, ndev);
    HIP_OK(hipSetDevice(device));
    return PPG_OK;
}
// Uploads host data to a device in the element format and fragment order the kernels read (members: ppg_pack.h); owns
// what it allocated.
struct Packer {
    int device = 0;
    Fmt fmt = Fmt::F32;
    std::vector<void*> allocs;
    Packer() = default; Packer(const Packer&) = delete;
    ~Packer() { (void)hipSetDevice(device); for (void* p : allocs) (void)hipFree(p); }
    int sz() const { return fmt == Fmt::BF16 || fmt == Fmt::F16 ? 2 : 4; }   // element bytes of the GEMM operands
    int KG() const { return 64 / sz(); }                                     // elements per 64-byte K-group
    bool split() const { return fmt == Fmt::F16X2; }
    int upload(const void* src, size_t bytes, void** dst);
    int upload_f32(const float* src, size_t n, size_t n_pad, float** dst);
    template <class F> int matrix(Fmt as, int rows, int cols, int rows_pad, int cols_pad, F get, char** dst);
    template <class F> int matrix(int rows, int cols, int rows_pad, int cols_pad, F get, char** dst) { return matrix(fmt, rows, cols, rows_pad, cols_pad, get, dst); }
    template <class F> int image(int frags, F get, char** dst);
    template <class F> int image_hilo(int groups, F get, char** dst);
};

// Chunk planner (ppg_plan.hip).  A group = a contiguous run of computed windows that is executed as one
// independent pipeline on its own HIP stream (windows never interact), with
// its own slice of the workspace and token rows numbered from 0.
struct PlanGroup {
    std::vector<PpgWindow> windows;   // tok_off / vt_off relative to the group
    std::vector<int> blk_win;
    std::vector<AttnItem> items;
    int tokens = 0, vt_tokens = 0;
    size_t ws_offset = 0;
    PpgWindow* d_win = nullptr;
    int* d_blk = nullptr;
    AttnItem* d_items = nullptr;
};
struct Plan {
    std::vector<PpgWindow> all;       // every window, skipped ones with tok_off = -1
    std::vector<PpgWindow> windows;   // computed windows (valid > 0), absolute offsets
    std::vector<PlanGroup> groups;
    PpgPlanInfo info{};
};
void split_groups(Plan* plan, int ngroups, int qtile, int xcd_heads, int narrow_tiles);
int build_plan(int chunk, int overlap, int max_positions, int batch, int frames,
               const int64_t* lengths, int legacy, int qtile, Plan* plan);

// Engine (ppg_engine.hip)
struct DevLayer {
    char* wqkv; float* bqkv;
    char* wo; float* bo;
    char* w1; float* b1;
    char* w2; char* w2p; float* b2;
    char* wqkvk;          // W_qkv for the Q/K/V tail of the previous layer's FFN kernel: fp32 columns in paired order (= wqkv in bf16 mode)
    char* w1k;            // W1 for the out-proj-fused FFN: fp32 columns in paired order (= w1 in bf16 mode)
    float *g1, *e1, *g2, *e2;
    // fragment images of the feature-split layer kernel (ppg_layer32.hip), 16-bit modes with hidden 256
    char* wo_img = nullptr; char* w1_img = nullptr; char* w2_img = nullptr; char* wq_img = nullptr;
    // hi + lo fragment images of the fp16x2 mode's feature-split FFN kernel (ppg_ffn32x2.hip), hidden 256
    char* w1x_img = nullptr; char* w2x_img = nullptr; char* wox_img = nullptr; char* wqx_img = nullptr;
};

struct DevPlan {
    Plan host;
    void* buf = nullptr;
    size_t cap = 0;            // bytes of buf
    uint64_t stamp = 0;
    bool pinned = false;       // used under stream capture: a HIP graph holds its device pointers, never evicted
    hipEvent_t uploaded = nullptr;   // recorded behind the asynchronous upload of the tables
    hipStream_t upload_stream = nullptr;
    bool upload_done = false;
    std::vector<hipStream_t> users;  // every stream a launch reading the tables was queued on (encodes run on several)
    ~DevPlan() { if (uploaded) (void)hipEventDestroy(uploaded); }
};
// a device buffer whose last uses were ordered before `ready` (one event per stream that used it)
struct RetiredBuf { void* buf; size_t cap; std::vector<hipEvent_t> ready; };
// pinned host staging slot of the plan uploads: busy until `done`
struct StageSlot { void* host = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool used = false; };

struct Workspace {
    size_t xw, x, xb, qk, vt, ao, hid, part, total;
    int ffn_nt, ffn_splits;
    int vt_ld, qk_rows;
};

}  // namespace ppg

struct PpgEngine {
    PpgConfig cfg{};
    int device = 0;
    int sz = 4;           // element bytes of the GEMM operands
    int KG = 16;          // elements per 64-byte K-group
    int Cp = 0;           // padded input channels of the gathered features
    int in_groups_per_tap = 0, in_total_groups = 0;
    int out_groups_per_tap = 0, out_total_groups = 0;
    int head_dim = 0;
    int ffn_nt = 0;       // 0 = pick per launch (choose_nt); 1..3 = forced
    int lin_nt = 0;       // same for the linear/conv kernels
    int num_cus = 256;
    bool ffn_fused = true;
    bool qkv_fused = true;   // next layer's Q/K/V projection as the tail of the fused FFN kernel (PPGS_AMD_QKV_FUSED=0: own kernel)
    int ffn_split_max = 0;   // PPGS_AMD_FFN_SPLIT_MAX: cap on the hidden splits (0: half the chunks)
    int ffn_splits_forced = 0;   // PPGS_AMD_FFN_SPLITS: this many hidden splits whatever the tile count (experiments)
    bool ffn_mixed = true;   // allow the mixed 3/3/2/2-block tiling of the fused layer kernel (PPGS_AMD_FFN_MIXED=0 disables)
    bool op_fused = true;    // attention out-projection + LN1 inside the FFN kernel (PPGS_AMD_OP_FUSED=0: own kernel)
    bool attn_xcd = true;    // attention items interleaved so that the query tiles of one (window, head) share an XCD's L2 (PPGS_AMD_ATTN_XCD=0: plain longest-first order)
    bool outconv = true;     // output convolution with LDS-resident weights where it applies (ppg_outconv.hip; PPGS_AMD_OUTCONV=0: linear_kernel)
    bool head32 = true;      // gather + input convolution + layer 0's Q/K/V in one kernel where it applies (with layer32, hidden 256, <= 96 input channels; PPGS_AMD_HEAD32=0: three launches)
    char* win_img = nullptr; // the input convolution as fragment images (ppg_head32.hip)
    int attn_narrow = 1;     // half-width query tiles for the short windows of a batch (PPGS_AMD_ATTN_NARROW=0: one width; 2: half-width tiles for every window)
    unsigned* d_overflow = nullptr;   // sticky device flag: a launch produced a non-finite logit for a valid frame (ppg_engine_nonfinite)
    int ffn32x2 = 3;         // fp16x2 mode, hidden 256, batches of >= half a chip of 96-token tiles: 3 = out-proj + LN1 + FFN + LN2 + the next layer's Q/K/V in ONE feature-split launch per layer (ppg_ffn32x2.hip), 2 = without the Q/K/V tail, 1 = the FFN block only, 0 = the token-split kernels always (PPGS_AMD_FFN32X2)
    bool subtile = true;     // layer32 path, hidden 256: workgroups of two token blocks (three per 160-token tile) when whole tiles would leave two thirds of the CUs idle (PPGS_AMD_SUBTILE=0: whole tiles always)
    bool x16 = false;        // layer32 path: the residual stream between two layer kernels is stored as fp16 (X16 order) instead of fp32 -- default in the bf16 mode (PPGS_AMD_X16=0 / 1 overrides)
    bool layer32 = true;     // feature-split 32x32x16 layer kernel where it applies (16-bit modes, hidden 256, batches that fill the chip; PPGS_AMD_LAYER32=0: token-split kernels everywhere)
    bool ffn_split = true;   // split-hidden FFN for small token counts (PPGS_AMD_FFN_SPLIT=0 disables)
    int num_streams = 2;    // pipelines (HIP streams) a batch of >= 128 x CUs token rows is split into (PPGS_AMD_STREAMS;
                            // 2 = +4..6.5 % at C2 over one pipeline, the same bits there: the half-batches' kernels run beside each
                            // other, every launch on the CUs its one-per-CU workgroups occupy)
    std::vector<hipStream_t> side_streams;
    bool stream_one_pass = false; // PPGS_AMD_STREAM_ONE_PASS=1: KV-cached streams run the split-hidden FFN's reduce + LayerNorm inside the FFN launch (last workgroup of a tile by ticket) -- measured slower: its 64 rows are 4 dependent round trips on 4 waves, 43 us against 18 + 18..30
    int stream_min_rows = 128; // PPGS_AMD_STREAMS_MIN_ROWS: token rows per CU from which a batch is split into pipelines
    hipEvent_t ev_fork = nullptr;
    std::vector<hipEvent_t> ev_join;
    int l32_debug = 0, h32_debug = 0;         // PPGS_AMD_L32_DEBUG / PPGS_AMD_H32_DEBUG: phase-skipping switches of the timing experiments (wrong results), read once
    unsigned long long* ffn_dbg = nullptr;
    unsigned long long* head_dbg = nullptr;
    unsigned long long* attn_dbg = nullptr;  // PPGS_AMD_ATTN_TIMING (PPG_ATTN_TIMING builds)
    unsigned long long* lin_dbg = nullptr;   // PPGS_AMD_LIN_TIMING=<kernel class> (PPG_LIN_TIMING builds): stamps of layer 0
    int lin_dbg_class = -1;
    ppg::Packer pack;        // the weights below: their element format, their device memory
    bool split() const { return pack.split(); }   // PPG_PRECISION_FP16X2: operands as fp16 hi + lo planes in the fp32 path's byte layout (PrecX2)
    float* pe = nullptr;
    char* w_in = nullptr; float* b_in = nullptr;
    char* w_out = nullptr; float* b_out = nullptr;
    std::vector<ppg::DevLayer> layers;
    std::map<std::string, std::unique_ptr<ppg::DevPlan>> plans;
    uint64_t plan_stamp = 0;
    std::vector<ppg::RetiredBuf> retired;      // evicted plans' buffers: reused (or freed) once their event has passed
    ppg::StageSlot stage[4];
    int stage_next = 0;
    std::mutex mu;
    // profiling
    unsigned profiling = 0;          // bitmask of kernel classes to time
    std::vector<ppg::EventPair> events[PPG_K_COUNT];
    size_t events_used[PPG_K_COUNT] = {0};
    int profile_stride = 1;                    // time every stride-th launch of a class
    size_t launch_seq[PPG_K_COUNT] = {0};

    ~PpgEngine();
};

namespace ppg {

#if defined(PPG_FFN_TIMING) || defined(PPG_ATTN_TIMING) || defined(PPG_H32_TIMING) || defined(PPG_LIN_TIMING)
#define PPG_TIMING_BUILD 1
void dump_timing_stamps(const PpgEngine* e);   // ppg_timing.hip: what the engine's stamp buffers hold, when it is destroyed
#endif

int choose_nt(int num_cus, int forced_nt, int M, int max_nt);
// The fused FFN kernel (ppg_ffn.h, ffn_body) walks the hidden features in chunks of one 32 KiB W1 tile; a
// split-hidden launch gives each of its `splits` workgroups per tile chunks / splits of them, so a split count must
// divide the chunk count.
inline int ffn_chunks(int hidden, int ffn, int sz) { return ffn / (32768 / (hidden * sz)); }
// Dynamic LDS of the fused FFN kernel (launch_ffn_t): the weight tiles, b1 and 6 parameter rows of `hidden` floats --
// 9 with the out-projection or the Q/K/V tail fused in; the mixed tiling (launch_ffn_mixed) adds a 16 KiB hand-off to
// the 6.  160 KiB per workgroup on gfx950.
constexpr size_t kLdsBytes = 163840;
inline size_t ffn_lds_bytes(int hidden, int ffn, int rows) { return 131072 + (size_t)ffn * 4 + (size_t)rows * hidden * 4; }
inline bool ffn_fits(int hidden, int ffn, bool op) { return ffn_lds_bytes(hidden, ffn, op ? 9 : 6) <= kLdsBytes; }
inline bool ffn_mixed_fits(int hidden, int ffn) { return ffn_lds_bytes(hidden, ffn, 6) + 16384 <= kLdsBytes; }
Workspace layout(const PpgEngine* e, int tokens, int vt_tokens);
// Queries per attention workgroup of a KV-cached stream's steps: half a tile at head dimension 128 (its items are narrow)
inline int stream_query_tile(int head_dim) { return head_dim == 128 ? attn_query_tile(head_dim) / 2 : attn_query_tile(head_dim); }

// `body` with `n` side streams forked from `s`: each side stream first waits for the work queued on `s` so far, and `s`
// waits for every side stream's work on every exit -- after an error of `body` too (best effort: the body's error is
// what is returned), so that the caller's stream always orders after the work queued on the side streams.
template <class Body>
int fork_join(hipStream_t s, hipEvent_t fork, const hipStream_t* side, const hipEvent_t* join, size_t n, Body&& body) {
    if (n == 0) return body();
    const int rc = [&]() -> int {
        HIP_OK(hipEventRecord(fork, s));
        for (size_t i = 0; i < n; ++i) HIP_OK(hipStreamWaitEvent(side[i], fork, 0));
        return body();
    }();
    if (rc != PPG_OK) {
        for (size_t i = 0; i < n; ++i) {
            (void)hipEventRecord(join[i], side[i]);
            (void)hipStreamWaitEvent(s, join[i], 0);
        }
        return rc;
    }
    for (size_t i = 0; i < n; ++i) {
        HIP_OK(hipEventRecord(join[i], side[i]));
        HIP_OK(hipStreamWaitEvent(s, join[i], 0));
    }
    return PPG_OK;
}

struct Timed {
    PpgEngine* e; int cls; hipStream_t s; EventPair ev{}; bool on = false;
    Timed(PpgEngine* e_, int cls_, hipStream_t s_) : e(e_), cls(cls_), s(s_) {
        if (!(e->profiling & (1u << cls))) return;
        if (e->launch_seq[cls]++ % (size_t)e->profile_stride) return;
        auto& pool = e->events[cls];
        size_t& used = e->events_used[cls];
        if (used == pool.size()) {
            EventPair p;
            if (hipEventCreateWithFlags(&p.a, kTimingEventFlags) != hipSuccess || hipEventCreateWithFlags(&p.b, kTimingEventFlags) != hipSuccess) return;
            pool.push_back(p);
        }
        ev = pool[used++];
        on = hipEventRecord(ev.a, s) == hipSuccess;
    }
    ~Timed() { if (on) (void)hipEventRecord(ev.b, s); }
};

// ----------------------------------------------------------------------------
// Launch arguments of the PPG network's kernels, one builder per kernel kind.  `Rows` is what differs between the
// launches of a one-shot encode (one set per pipeline) and of a stream step: the token rows, their window and block
// tables, the residual stream, and the step's row map.
// ----------------------------------------------------------------------------
struct Rows {
    const int* blk_win; const PpgWindow* win; int M;
    float* X; char* Xb;
    const int* rowmap = nullptr; int map_blocks = 0;
};
// a GEMM over rows of K elements: act [M][K] x W [N][K] + bias
inline LinearArgs gemm_args(const PpgEngine* e, const Rows& t, const char* act, int K, const char* W, const float* bias, int N) {
    LinearArgs a{};
    a.blk_win = t.blk_win; a.win = t.win; a.M = t.M; a.H = e->cfg.hidden_channels;
    a.X = t.X; a.Xb = t.Xb; a.v_start = INT_MAX; a.taps = 1;
    a.rowmap = t.rowmap; a.map_blocks = t.map_blocks;
    a.act = act; a.lda_bytes = K * e->sz;
    a.groups_per_tap = a.real_groups = a.total_groups = K / e->KG;
    a.W = W; a.bias = bias; a.N = N;
    return a;
}
// input convolution (+ positional encoding) of the gathered rows `xw` (EPI_INCONV)
inline LinearArgs inconv_args(const PpgEngine* e, const Rows& t, const char* xw) {
    LinearArgs a = gemm_args(e, t, xw, e->Cp, e->w_in, e->b_in, e->cfg.hidden_channels);
    a.taps = 5; a.groups_per_tap = e->in_groups_per_tap; a.real_groups = 5 * e->in_groups_per_tap; a.total_groups = e->in_total_groups;
    a.pe = e->pe;
    return a;
}
// Q | K rows and V^T columns of a layer (EPI_QKV)
inline LinearArgs qkv_args(const PpgEngine* e, const Rows& t, const DevLayer& d, const char* act_x, char* qk, char* vt, int vt_ld) {
    const int H = e->cfg.hidden_channels;
    LinearArgs a = gemm_args(e, t, act_x, H, d.wqkv, d.bqkv, 3 * H);
    a.out_rows = qk; a.out_ld = 2 * H; a.vt = vt; a.vt_ld = vt_ld; a.v_start = 2 * H;
    return a;
}
// attention out-projection + residual + LayerNorm-1 (EPI_RESLN)
inline LinearArgs outproj_ln_args(const PpgEngine* e, const Rows& t, const DevLayer& d, const char* ao) {
    const int H = e->cfg.hidden_channels;
    LinearArgs a = gemm_args(e, t, ao, H, d.wo, d.bo, H);
    a.gamma = d.g1; a.beta = d.e1;
    return a;
}
// output convolution + mask + softmax into `out` (batch, output_channels, out_T) (EPI_OUTCONV / ppg_outconv.hip)
inline LinearArgs outconv_args(const PpgEngine* e, const Rows& t, const char* act_x, float* out, int out_T, int softmax) {
    LinearArgs a = gemm_args(e, t, act_x, e->cfg.hidden_channels, e->w_out, e->b_out, 48);
    a.taps = 5; a.groups_per_tap = e->out_groups_per_tap; a.real_groups = 5 * e->out_groups_per_tap; a.total_groups = e->out_total_groups;
    a.out = out; a.out_T = out_T; a.out_C = e->cfg.output_channels; a.softmax = softmax;
    a.overflow = e->d_overflow;
    return a;
}
// attention over `items` (query tiles) of the windows `win`; operands of `sz` bytes
inline AttnArgs attn_args(int sz, int H, int heads, int causal, const char* qk, const char* vt, int vt_ld, char* ao,
                          const AttnItem* items, const PpgWindow* win, int M) {
    AttnArgs a{};
    a.qk = qk; a.qk_ld_bytes = 2 * H * sz; a.vt = vt; a.vt_ld_bytes = vt_ld * sz;
    a.ao = ao; a.H = H; a.causal = causal;
    a.items = items; a.win = win; a.M = M; a.heads = heads;
    return a;
}
// token-split FFN + residual + LayerNorm-2, the hidden chunks in `splits` workgroups per tile (partial sums in `partial`) ...
inline FfnArgs ffn_args(const PpgEngine* e, const Rows& t, const DevLayer& d, int splits, float* partial) {
    FfnArgs a{};
    a.X = t.X; a.Xb = t.Xb; a.W1 = d.w1; a.b1 = d.b1; a.W2p = d.w2p; a.b2 = d.b2;
    a.gamma = d.g2; a.beta = d.e2; a.H = e->cfg.hidden_channels; a.F = e->cfg.ffn_channels; a.M = t.M;
    a.splits = splits; a.partial = splits > 1 ? partial : nullptr;
    a.rowmap = t.rowmap; a.map_blocks = t.map_blocks;
    return a;
}
// ... with the attention out-projection + LayerNorm-1 in front (fp32: W1 in the paired K order LN1's accumulators come in) ...
inline void ffn_fuse_outproj(FfnArgs* a, const DevLayer& d, const char* ao) {
    a->ao = ao; a->Wo = d.wo; a->bo = d.bo; a->g1 = d.g1; a->e1 = d.e1; a->W1 = d.w1k;
}
// ... and with the NEXT layer's (`nx`) Q/K/V projection as its tail
inline void ffn_fuse_qkv(FfnArgs* a, const Rows& t, const DevLayer& nx, char* qk, char* vt, int vt_ld) {
    a->Wq = nx.wqkvk; a->bq = nx.bqkv; a->qk_out = qk; a->vt_out = vt; a->vt_ld = vt_ld;
    a->blk_win = t.blk_win; a->win = t.win;
}
// the 64 K rows behind the last of the M token rows of `qk`, which the attention tiles read (masked): GatherArgs, Head32Args
template <class Args>
void set_qk_slack(const PpgEngine* e, char* qk, int M, Args* a) {
    a->qk_slack = qk + (size_t)M * 2 * e->cfg.hidden_channels * e->sz;
    a->qk_slack_bytes = (int)(64 * 2 * e->cfg.hidden_channels * e->sz);
}
// gather of the feature rows into `xw`; the same launch keeps finite what the attention tiles read masked: the V^T
// padding columns of `nwin` windows and the K rows behind the last token
inline GatherArgs gather_args(const PpgEngine* e, const Rows& t, const void* feats, int dtype, int T, char* xw,
                              char* qk, char* vt, int vt_ld, int vt_tokens, int nwin) {
    const int H = e->cfg.hidden_channels;
    GatherArgs g{};
    g.feats = feats; g.dtype = dtype; g.C = e->cfg.input_channels; g.T = T; g.overlap = e->cfg.chunk_overlap;
    g.xw = xw; g.Cp = e->Cp;
    g.blk_win = t.blk_win; g.win = t.win; g.M = t.M;
    g.rowmap = t.rowmap; g.map_blocks = t.map_blocks;
    g.vt = vt; g.vt_ld = vt_ld; g.vt_rows = H; g.vt_tokens = vt_tokens; g.nwin = nwin;
    set_qk_slack(e, qk, t.M, &g);
    return g;
}

}  // namespace ppg
