// The PPG network's engine (include/ppgs_amd.h: ppg_engine_*, ppg_plan_*, ppg_encode): creation and weight packing,
// tiling choices, workspace layout, the plan cache, the launch sequence of one encode, the profiling getters.  Also
// the home of the library's one last-error string.
#include "ppg_pack.h"

#include <stdarg.h>

using namespace ppg;

static thread_local std::string g_error;

int ppg::fail_message(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}

PpgEngine::~PpgEngine() {
    (void)hipSetDevice(device);
#ifdef PPG_TIMING_BUILD
    dump_timing_stamps(this);
#endif
    for (void* p : {(void*)d_overflow, (void*)head_dbg, (void*)ffn_dbg, (void*)attn_dbg, (void*)lin_dbg}) if (p) (void)hipFree(p);
    for (auto& kv : plans) if (kv.second->buf) (void)hipFree(kv.second->buf);
    for (RetiredBuf& r : retired) { (void)hipFree(r.buf); for (hipEvent_t ev : r.ready) (void)hipEventDestroy(ev); }
    for (StageSlot& st : stage) { if (st.host) (void)hipHostFree(st.host); if (st.done) (void)hipEventDestroy(st.done); }
    for (hipStream_t st : side_streams) (void)hipStreamDestroy(st);
    for (hipEvent_t ev : ev_join) (void)hipEventDestroy(ev);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    for (auto& v : events) for (auto& e : v) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
}

// Token blocks (of 16) per wave for the token-tiled kernels: a workgroup
// covers 64*nt tokens; pick the nt that minimises (rounds over the CUs) x
// (per-round cost ~ nt, larger tiles being slightly more efficient because
// each weight fragment read from LDS feeds nt MFMAs).
int ppg::choose_nt(int num_cus, int forced_nt, int M, int max_nt) {
    if (forced_nt >= 1) return std::min(forced_nt, max_nt);
    static const double eff[4] = {0, 0.7, 1.0, 1.1};
    int best = 1;
    double best_cost = 1e30;
    for (int nt = 1; nt <= max_nt; ++nt) {
        const int blocks = (M + 64 * nt - 1) / (64 * nt);
        const int rounds = (blocks + num_cus - 1) / num_cus;
        const double cost = rounds * nt / eff[nt];
        if (cost < best_cost) { best_cost = cost; best = nt; }
    }
    return best;
}

// Fused-FFN tiling for a group of `M` token rows: tokens per wave (16*nt) and,
// when the tiles cannot fill the CUs, how many workgroups share one tile by
// splitting the hidden chunks between them (partial sums + a reduce/LN pass).
// A workgroup streams all of W1/W2 through its CU whatever its tile size, so
// few large tiles x several hidden splits beats many small tiles.
static void choose_ffn_tiling(const PpgEngine* e, int M, int* nt_out, int* splits_out) {
    const int max_nt = (e->sz == 2 && e->cfg.hidden_channels == 256) ? 3
                       : (e->cfg.hidden_channels == 256 ? 2 : 1);
    int nt = choose_nt(e->num_cus, e->ffn_nt, M, max_nt);
    int splits = 1;
    // (a workgroup of a split launch sums chunks / splits hidden chunks, ffn_body's NC: only divisors of the chunk count)
    const int chunks = ppg::ffn_chunks(e->cfg.hidden_channels, e->cfg.ffn_channels, e->sz);
    if (e->ffn_split && e->ffn_fused && e->ffn_nt == 0) {
        const int tiles_max_nt = (M + 64 * max_nt - 1) / (64 * max_nt);
        // only when the tiles would leave 7/8 of the chip idle: the partial-sum
        // round trip costs about as much as it saves above that (measured: 64 x 160
        // frames, 54 tiles: 500 us/step unsplit vs 576 us split)
        if (tiles_max_nt * 8 <= e->num_cus) {
            nt = max_nt;
            const int cap = e->ffn_split_max > 0 ? e->ffn_split_max : chunks / 2;
            while (splits * 2 <= cap && chunks % (splits * 2) == 0 && tiles_max_nt * splits * 2 <= e->num_cus) splits *= 2;
        }
    }
    // 4-byte operand modes (fp32, fp16x2) cannot hold more than 128 tokens in LDS, so a launch whose tiles
    // need a fraction over a whole number of rounds of the chip (C2: 320 tiles on 256 CUs = 2 rounds, the
    // second a quarter full) is cut into hidden splits instead: ceil(tiles * s / CUs) / s rounds of full tiles
    if (splits == 1 && e->sz == 4 && e->ffn_split && e->ffn_fused && e->ffn_nt == 0 && !e->op_fused) {
        const int tiles = (M + 64 * max_nt - 1) / (64 * max_nt);
        auto rounds = [&](int sp) { return (double)((tiles * sp + e->num_cus - 1) / e->num_cus) / sp + 0.08 * (sp > 1 ? 1 + 0.5 * sp : 0); };
        int best = 1;
        for (int sp = 2; sp <= 4 && sp <= chunks / 2 && chunks % sp == 0; sp *= 2)
            if (rounds(sp) < rounds(best)) best = sp;
        if (best > 1) { nt = max_nt; splits = best; }
    }
    if (e->ffn_splits_forced > 0 && e->ffn_fused) { nt = max_nt; splits = e->ffn_splits_forced; }
    // mixed tiling (160-token workgroups, ppg_ffn.h ffn_mixed_kernel): 2.5 blocks of
    // MFMA work per wave and chunk instead of nt; worth it when it saves a round or
    // shortens the one round there is (C2: 256 workgroups on 256 CUs instead of 214 larger ones)
    if (splits == 1 && e->ffn_mixed && e->ffn_fused && e->op_fused && e->ffn_nt == 0 &&
        e->sz == 2 && e->cfg.hidden_channels == 256) {
        const int blocks_nt = (M + 64 * nt - 1) / (64 * nt), blocks_mixed = (M + 159) / 160;
        const double rounds_nt = (blocks_nt + e->num_cus - 1) / e->num_cus;
        const double rounds_mixed = (blocks_mixed + e->num_cus - 1) / e->num_cus;
        if (rounds_mixed * 2.5 < rounds_nt * nt) nt = ppg::kFfnMixedTiling;
    }
    *nt_out = nt;
    *splits_out = splits;
}

Workspace ppg::layout(const PpgEngine* e, int tokens, int vt_tokens) {
    Workspace w{};
    const size_t M = tokens;
    const int H = e->cfg.hidden_channels;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    w.qk_rows = (int)M + 64;
    w.vt_ld = vt_tokens + 64;
    w.xw = take(M * e->Cp * e->sz);
    const size_t Ttile = layer32_tile_tokens(H);        // whole tiles of the layer32 kernel (X32 / AO32 layouts)
    const size_t Mt = (M + Ttile - 1) / Ttile * Ttile;
    w.x = take(Mt * H * 4);
    w.xb = take(e->sz == 2 ? M * H * 2 : (e->split() ? M * H * 4 : 0));
    w.qk = take((size_t)w.qk_rows * 2 * H * e->sz);
    w.vt = take((size_t)H * w.vt_ld * e->sz);
    w.ao = take(Mt * H * e->sz);
    w.hid = take(e->ffn_fused ? 0 : M * e->cfg.ffn_channels * e->sz);
    choose_ffn_tiling(e, tokens, &w.ffn_nt, &w.ffn_splits);
    w.part = take(w.ffn_splits > 1 ? (size_t)w.ffn_splits * M * H * 4 : 0);
    w.total = off;
    return w;
}

namespace {

// Pipelines (HIP streams) a batch is split into: windows are independent, so
// two half-batches on two streams fill the CUs one kernel's last, partly
// filled round of workgroups leaves idle (+8 % at C2).
int group_count(const PpgEngine* e, int tokens) {
    if (e->num_streams <= 1) return 1;
    return tokens >= e->stream_min_rows * e->num_cus ? e->num_streams : 1;
}

size_t finish_plan(const PpgEngine* e, Plan* p) {
    split_groups(p, group_count(e, p->info.tokens), ppg::attn_query_tile(e->head_dim), e->attn_xcd ? e->cfg.heads : 0, e->head_dim == 128 ? e->attn_narrow : 0);
    size_t off = 0;
    for (PlanGroup& grp : p->groups) {
        grp.ws_offset = off;
        off = align_up(off + layout(e, grp.tokens, grp.vt_tokens).total, 256);
    }
    p->info.workspace_bytes = off;
    return off;
}

// The cached (or new) plan of a batch shape, its tables on the device.  A miss costs no device-wide
// synchronisation: the tables go up by hipMemcpyAsync on `stream` from a pinned staging ring, device
// buffers of evicted plans are recycled behind an event.  Under stream capture (Engine.graphed)
// nothing may allocate or copy: the plan must already be cached (graphed() warms it up), and it is
// pinned from then on -- the graph holds its device pointers.
int get_plan(PpgEngine* e, int batch, int frames, const int64_t* lengths, int legacy, hipStream_t stream, DevPlan** out) {
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream, &capture);
    const bool capturing = capture != hipStreamCaptureStatusNone;
    std::string key;
    key.reserve(16 + 8 * (size_t)batch);
    const int hdr[3] = {batch, frames, legacy};
    key.append(reinterpret_cast<const char*>(hdr), sizeof(hdr));
    key.append(reinterpret_cast<const char*>(lengths), sizeof(int64_t) * (size_t)batch);
    auto it = e->plans.find(key);
    if (it != e->plans.end()) {
        DevPlan* hit = it->second.get();
        hit->stamp = ++e->plan_stamp;
        if (capturing) hit->pinned = true;
        if (std::find(hit->users.begin(), hit->users.end(), stream) == hit->users.end()) hit->users.push_back(stream);
        // the tables went up asynchronously on the stream of the first use: another stream waits for them
        if (!hit->upload_done) {
            if (hipEventQuery(hit->uploaded) == hipSuccess) hit->upload_done = true;
            else if (stream != hit->upload_stream) {
                if (capturing) HIP_OK(hipEventSynchronize(hit->uploaded));
                else HIP_OK(hipStreamWaitEvent(stream, hit->uploaded, 0));
            }
        }
        *out = hit;
        return PPG_OK;
    }
    if (capturing)
        return fail(PPG_EINVAL, "ppg_encode under stream capture needs a cached plan: run the same (batch, frames, lengths) once before capturing");
    auto dp = std::make_unique<DevPlan>();
    int rc = build_plan(e->cfg.chunk_length, e->cfg.chunk_overlap, e->cfg.max_positions, batch, frames,
                        lengths, legacy, ppg::attn_query_tile(e->head_dim), &dp->host);
    if (rc) return rc;
    Plan& p = dp->host;
    finish_plan(e, &p);
    // one device buffer: per group windows | blk_win | attention items
    struct Off { size_t win, blk, item; };
    std::vector<Off> offs;
    size_t total = 0;
    for (const PlanGroup& grp : p.groups) {
        Off o;
        o.win = total;
        o.blk = align_up(o.win + std::max<size_t>(grp.windows.size(), 1) * sizeof(PpgWindow), 256);
        o.item = align_up(o.blk + std::max<size_t>(grp.blk_win.size(), 1) * sizeof(int), 256);
        total = align_up(o.item + std::max<size_t>(grp.items.size(), 1) * sizeof(AttnItem), 256);
        offs.push_back(o);
    }
    total = std::max<size_t>(total, 256);
    std::vector<char> staging(total, 0);
    for (size_t gi = 0; gi < p.groups.size(); ++gi) {
        const PlanGroup& grp = p.groups[gi];
        memcpy(staging.data() + offs[gi].win, grp.windows.data(), grp.windows.size() * sizeof(PpgWindow));
        memcpy(staging.data() + offs[gi].blk, grp.blk_win.data(), grp.blk_win.size() * sizeof(int));
        memcpy(staging.data() + offs[gi].item, grp.items.data(), grp.items.size() * sizeof(AttnItem));
    }
    // bound the cache: evict the least recently used plan that no graph refers to; its buffer is retired behind
    // one event per stream that ever used it (kernels queued on ANY of them may still read the tables)
    if (e->plans.size() >= 64) {
        auto victim = e->plans.end();
        for (auto jt = e->plans.begin(); jt != e->plans.end(); ++jt)
            if (!jt->second->pinned && (victim == e->plans.end() || jt->second->stamp < victim->second->stamp)) victim = jt;
        if (victim != e->plans.end()) {
            if (victim->second->buf) {
                RetiredBuf r{victim->second->buf, victim->second->cap, {}};
                std::vector<hipStream_t> streams = victim->second->users;
                if (std::find(streams.begin(), streams.end(), stream) == streams.end()) streams.push_back(stream);
                for (hipStream_t user : streams) {
                    hipEvent_t ev = nullptr;
                    HIP_OK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
                    r.ready.push_back(ev);
                    HIP_OK(hipEventRecord(ev, user));
                }
                e->retired.push_back(std::move(r));
            }
            e->plans.erase(victim);
        }
    }
    // a retired buffer that is large enough and no longer in use, else a new one
    for (size_t i = 0; i < e->retired.size(); ++i) {
        RetiredBuf& r = e->retired[i];
        bool idle = true;
        for (hipEvent_t ev : r.ready) idle = idle && hipEventQuery(ev) == hipSuccess;
        if (!idle) continue;
        if (r.cap >= total && dp->buf == nullptr) {
            dp->buf = r.buf; dp->cap = r.cap;
        } else if (e->retired.size() > 16) {
            (void)hipFree(r.buf);                 // the pool stays small
        } else {
            continue;
        }
        for (hipEvent_t ev : r.ready) (void)hipEventDestroy(ev);
        e->retired.erase(e->retired.begin() + i);
        --i;
    }
    if (dp->buf == nullptr) {
        dp->cap = align_up(total, 4096);
        HIP_OK(hipMalloc(&dp->buf, dp->cap));
    }
    // upload through a pinned staging slot, asynchronously on the encode stream
    StageSlot& slot = e->stage[e->stage_next];
    e->stage_next = (e->stage_next + 1) % 4;
    if (slot.used) HIP_OK(hipEventSynchronize(slot.done));      // four uploads in flight at most
    if (slot.cap < total) {
        if (slot.host) (void)hipHostFree(slot.host);
        slot.cap = align_up(total * 2, 4096);
        HIP_OK(hipHostMalloc(&slot.host, slot.cap, hipHostMallocDefault));
    }
    if (!slot.done) HIP_OK(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
    memcpy(slot.host, staging.data(), total);
    HIP_OK(hipMemcpyAsync(dp->buf, slot.host, total, hipMemcpyHostToDevice, stream));
    HIP_OK(hipEventRecord(slot.done, stream));
    slot.used = true;
    HIP_OK(hipEventCreateWithFlags(&dp->uploaded, hipEventDisableTiming));
    HIP_OK(hipEventRecord(dp->uploaded, stream));
    dp->upload_stream = stream;
    dp->users.push_back(stream);
    for (size_t gi = 0; gi < p.groups.size(); ++gi) {
        char* base = static_cast<char*>(dp->buf);
        p.groups[gi].d_win = reinterpret_cast<PpgWindow*>(base + offs[gi].win);
        p.groups[gi].d_blk = reinterpret_cast<int*>(base + offs[gi].blk);
        p.groups[gi].d_items = reinterpret_cast<AttnItem*>(base + offs[gi].item);
    }
    dp->stamp = ++e->plan_stamp;
    *out = dp.get();
    e->plans.emplace(std::move(key), std::move(dp));
    return PPG_OK;
}

// the windows of a batch as `engine` plans them, or (null) the reference configuration: chunks of 500 with overlap 50, head dimension 128
int plan_for(const PpgEngine* engine, int batch, int frames, const int64_t* lengths, int legacy, Plan* plan) {
    const PpgConfig* c = engine ? &engine->cfg : nullptr;
    return build_plan(c ? c->chunk_length : 500, c ? c->chunk_overlap : 50, c ? c->max_positions : 5000, batch, frames, lengths, legacy,
                      ppg::attn_query_tile(engine ? engine->head_dim : 128), plan);
}

}  // namespace

// ============================================================================
// C ABI
// ============================================================================
extern "C" {

const char* ppg_last_error(void) { return g_error.c_str(); }
int ppg_abi_version(void) { return PPG_ABI_VERSION; }

int ppg_engine_create(const PpgConfig* cfg, const PpgWeights* wts, int device, PpgEngine** out) {
    if (!cfg || !wts || !out) return fail(PPG_EINVAL, "null argument");
    const int H = cfg->hidden_channels, F = cfg->ffn_channels, L = cfg->num_layers, C = cfg->input_channels;
    if (cfg->kernel_size != 5) return fail(PPG_EINVAL, "kernel_size %d unsupported (5 only)", cfg->kernel_size);
    if (L < 0 || L > PPG_MAX_LAYERS) return fail(PPG_EINVAL, "num_layers %d outside [0,%d]", L, PPG_MAX_LAYERS);
    if (H != 256 && H != 512) return fail(PPG_EINVAL, "hidden_channels %d unsupported (256 or 512)", H);
    if (cfg->heads < 1 || H % cfg->heads) return fail(PPG_EINVAL, "heads %d does not divide hidden %d", cfg->heads, H);
    const int dh = H / cfg->heads;
    if (dh != 128 && dh != 256) return fail(PPG_EINVAL, "head dim %d unsupported (128 or 256)", dh);
    if (F % 64 || F < 64) return fail(PPG_EINVAL, "ffn_channels %d must be a multiple of 64", F);
    if (cfg->output_channels < 1 || cfg->output_channels > 48) return fail(PPG_EINVAL, "output_channels %d outside [1,48]", cfg->output_channels);
    if (C < 1) return fail(PPG_EINVAL, "input_channels %d", C);
    if (cfg->chunk_length <= 2 * cfg->chunk_overlap || cfg->chunk_length > 512)
        return fail(PPG_EINVAL, "chunk_length %d / overlap %d unsupported", cfg->chunk_length, cfg->chunk_overlap);
    // a window adds the table's rows 0 .. its length - 1 to its frames (never more than chunk_length of them outside legacy mode,
    // where build_plan holds the frames below max_positions)
    if (cfg->max_positions < cfg->chunk_length)
        return fail(PPG_EINVAL, "max_positions %d below chunk_length %d: a window would read position rows behind the table", cfg->max_positions, cfg->chunk_length);
    if (!known_precision(cfg->precision)) return fail(PPG_EINVAL, "precision %d", cfg->precision);
    if (cfg->precision == PPG_PRECISION_FP16X2 && !((H == 256 && dh == 128) || (H == 512 && dh == 256)))
        return fail(PPG_EINVAL, "the fp16x2 mode covers hidden 256 with head dimension 128 and hidden 512 with head dimension 256 (hidden %d, head dimension %d)", H, dh);
    {   // What the FFN routes can do with this F is settled here, not at the first launch (and before the device is touched).
        // The FFN runs as two GEMMs in the fp16x2 mode at hidden 512 and under PPGS_AMD_FFN_UNFUSED, 256 hidden features per
        // pass of the first; everywhere else the fused kernel must hold b1 in LDS beside its weight tiles.
        const bool split = cfg->precision == PPG_PRECISION_FP16X2;
        const bool two_gemm = split ? H == 512 : ppg::env_switch("PPGS_AMD_FFN_UNFUSED", 0) != 0;
        if (two_gemm && F % 256)
            return fail(PPG_EINVAL, "ffn_channels %d must be a multiple of 256 for the two-GEMM FFN (%s)", F,
                        split ? "the only route of the fp16x2 mode at hidden 512" : "PPGS_AMD_FFN_UNFUSED");
        if (!two_gemm && !ppg::ffn_fits(H, F, false))
            return fail(PPG_EINVAL, "ffn_channels %d above %d, the most the FFN kernel holds in LDS at hidden %d", F,
                        (int)((ppg::kLdsBytes - ppg::ffn_lds_bytes(H, 0, 6)) / 4 / 64 * 64), H);
    }
    if (int rc = use_device(device, "PPG engine")) return rc;

    std::unique_ptr<PpgEngine> e(new PpgEngine());
    e->cfg = *cfg;
    e->device = device;
    Packer& pk = e->pack;
    pk.device = device;
    pk.fmt = operand_format(cfg->precision);
    e->sz = pk.sz(); e->KG = pk.KG();
    e->head_dim = dh;
    e->Cp = round_up(C, e->split() ? 32 : e->KG);      // (split operands: whole [32 hi | 32 lo] blocks)
    e->in_groups_per_tap = e->Cp / e->KG;
    e->in_total_groups = round_up(5 * e->in_groups_per_tap, 2);
    e->out_groups_per_tap = H / e->KG;
    e->out_total_groups = round_up(5 * e->out_groups_per_tap, 2);
    using ppg::env_switch;
    using ppg::env_experiment;
    e->ffn_nt = env_experiment("PPGS_AMD_FFN_NT", e->ffn_nt);
    e->lin_nt = env_experiment("PPGS_AMD_LIN_NT", e->lin_nt);
    e->ffn_fused = env_switch("PPGS_AMD_FFN_UNFUSED", !e->ffn_fused) == 0;
    e->ffn_split = env_experiment("PPGS_AMD_FFN_SPLIT", e->ffn_split) != 0;
    e->ffn32x2 = env_switch("PPGS_AMD_FFN32X2", e->ffn32x2);
    e->num_streams = std::max(1, std::min(env_switch("PPGS_AMD_STREAMS", e->num_streams), 4));
    e->stream_one_pass = env_experiment("PPGS_AMD_STREAM_ONE_PASS", e->stream_one_pass) != 0;
    e->stream_min_rows = std::max(1, env_experiment("PPGS_AMD_STREAMS_MIN_ROWS", e->stream_min_rows));
    HIP_OK(hipEventCreateWithFlags(&e->ev_fork, kForkJoinEventFlags));
    for (int i = 1; i < e->num_streams; ++i) {
        hipStream_t st;
        hipEvent_t ev;
        HIP_OK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        HIP_OK(hipEventCreateWithFlags(&ev, kForkJoinEventFlags));
        e->side_streams.push_back(st);
        e->ev_join.push_back(ev);
    }
    e->op_fused = env_switch("PPGS_AMD_OP_FUSED", e->op_fused) != 0;
    e->ffn_mixed = env_switch("PPGS_AMD_FFN_MIXED", e->ffn_mixed) != 0;
    e->ffn_split_max = env_experiment("PPGS_AMD_FFN_SPLIT_MAX", e->ffn_split_max);
    e->ffn_splits_forced = env_experiment("PPGS_AMD_FFN_SPLITS", e->ffn_splits_forced);
    e->qkv_fused = env_switch("PPGS_AMD_QKV_FUSED", e->qkv_fused) != 0;
    e->layer32 = env_switch("PPGS_AMD_LAYER32", e->layer32) != 0;
    e->attn_xcd = env_experiment("PPGS_AMD_ATTN_XCD", e->attn_xcd) != 0;
    e->attn_narrow = std::max(0, std::min(env_switch("PPGS_AMD_ATTN_NARROW", e->attn_narrow), 2));
    e->head32 = env_switch("PPGS_AMD_HEAD32", e->head32) != 0;
    e->subtile = env_switch("PPGS_AMD_SUBTILE", e->subtile) != 0;
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&e->d_overflow), 256));
    HIP_OK(hipMemset(e->d_overflow, 0, 256));
    e->x16 = env_experiment("PPGS_AMD_X16", cfg->precision == PPG_PRECISION_BF16) != 0;
    e->outconv = env_switch("PPGS_AMD_OUTCONV", e->outconv) != 0;
#ifdef PPG_DEBUG_MODES
    e->l32_debug = env_switch("PPGS_AMD_L32_DEBUG", 0);
    e->h32_debug = env_switch("PPGS_AMD_H32_DEBUG", 0);
#endif
    if (e->split()) {
        // the unfused launch sequence: Q/K/V, attention, out-projection + LayerNorm, FFN as one launch each
        e->op_fused = false; e->qkv_fused = false; e->ffn_mixed = false; e->ffn_fused = true;
        // hidden 512: the FFN as two GEMMs through a [tokens][ffn] buffer of [32 hi | 32 lo] rows (a chunk of the fused
        // kernel cannot hold a 32-wide hidden group of both weight tiles: ppg_linear.h, launch_linear_x2_nt)
        if (H == 512) e->ffn_fused = false;
    }
    // With the out-projection (or the mixed tiling's hand-off) fused in, the FFN kernel has LDS for fewer hidden
    // features: those fusions are switched off where they do not fit (an F that fits no form was refused above).
    if (e->ffn_fused) {
        if (!ppg::ffn_fits(H, F, true)) e->op_fused = false;
        if (!ppg::ffn_mixed_fits(H, F)) e->ffn_mixed = false;
        if (e->ffn_splits_forced > 0 && ppg::ffn_chunks(H, F, e->sz) % e->ffn_splits_forced)
            return fail(PPG_EINVAL, "PPGS_AMD_FFN_SPLITS=%d does not divide the %d hidden chunks of ffn_channels %d", e->ffn_splits_forced,
                        ppg::ffn_chunks(H, F, e->sz), F);
    }
    if (!e->layer32 || H != 256 || e->Cp != 96 || !e->qkv_fused) e->head32 = false;
    if (e->sz != 2 || (H != 256 && H != 512) || F % 128 || F > ppg::layer32_max_ffn(H)) e->layer32 = false;
#ifdef PPG_LIN_TIMING
    if (const char* v = getenv("PPGS_AMD_LIN_TIMING")) {
        e->lin_dbg_class = atoi(v);
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&e->lin_dbg), 16 * 8192 * 8));
        HIP_OK(hipMemset(e->lin_dbg, 0, 16 * 8192 * 8));
    }
#endif
#ifdef PPG_ATTN_TIMING
    if (getenv("PPGS_AMD_ATTN_TIMING")) {
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&e->attn_dbg), 512 + 4096 * 32));
        HIP_OK(hipMemset(e->attn_dbg, 0, 512 + 4096 * 32));
    }
#endif
#ifdef PPG_H32_TIMING
    if (getenv("PPGS_AMD_H32_TIMING")) {
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&e->head_dbg), 512));
        HIP_OK(hipMemset(e->head_dbg, 0, 512));
    }
#endif
#ifdef PPG_FFN_TIMING
    if (getenv("PPGS_AMD_FFN_TIMING")) {
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&e->ffn_dbg), 2048));
        HIP_OK(hipMemset(e->ffn_dbg, 0, 2048));
    }
#endif
    if (e->ffn_nt < 0 || e->ffn_nt > 3) e->ffn_nt = 0;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
            e->num_cus = prop.multiProcessorCount;
    }

    int rc;
    if ((rc = pk.upload_f32(wts->position_encoding, (size_t)cfg->max_positions * H, 0, &e->pe))) return rc;
    {   // in-conv  W'[h][tap*Cp + c] = w[h][c][tap]
        const float* w = wts->input_weight;
        const int Cp = e->Cp;
        rc = pk.matrix(H, 5 * Cp, H, e->in_total_groups * e->KG,
                       [&](int row, int k) { const int h = pair_row(row), tap = k / Cp, c = k % Cp; return c < C ? w[((size_t)h * C + c) * 5 + tap] : 0.f; },
                       &e->w_in);
        if (rc) return rc;
        if ((rc = pk.upload_f32(wts->input_bias, H, 0, &e->b_in))) return rc;
    }
    // Fragment images of the feature-split kernels (ppg_pack.h): wave w owns features 32 RB w .. of a H-wide result
    // (RB = H / 128), in blocks of 32 rows in the accumulator order phi; where a GEMM's K is the previous accumulator
    // (x1, h, x2) the K order follows it.
    const int RB = H / 128, KS = H / 16;
    auto wave_row = [&](int w, int rb, int ln) { return 32 * RB * w + 32 * rb + phi(ln & 31); };
    if (e->head32) {
        // the same convolution as A fragments for ppg_head32.hip: [wave][rb][K-step = tap x 16-channel block], one zero fragment behind
        const float* w = wts->input_weight;
        const int KSI = 5 * e->Cp / 16, frags = 4 * RB * KSI;
        rc = pk.image(frags + 1, [&](int f, int ln, int j) {
            if (f >= frags) return 0.f;
            const int ks = f % KSI, rb = (f / KSI) % RB, wv = f / (KSI * RB);
            const int tap = ks / (e->Cp / 16), c = frag_k(ks % (e->Cp / 16), ln, j);
            return c < C ? w[((size_t)wave_row(wv, rb, ln) * C + c) * 5 + tap] : 0.f;
        }, &e->win_img);
        if (rc) return rc;
    }
    {   // out-conv W'[n][tap*H + c] = w[n][c][tap], rows padded to 48
        const float* w = wts->output_weight;
        rc = pk.matrix(cfg->output_channels, 5 * H, 48, e->out_total_groups * e->KG,
                       [&](int n, int k) { const int tap = k / H, c = k % H; return w[((size_t)n * H + c) * 5 + tap]; },
                       &e->w_out);
        if (rc) return rc;
        if ((rc = pk.upload_f32(wts->output_bias, cfg->output_channels, 48, &e->b_out))) return rc;
    }
    e->layers.resize(L);
    // The attention kernel takes its Q rows already multiplied by log2(e) / sqrt(head_dim) (attn_body's softmax
    // is a bare exp2 of the score accumulator): the factor goes into the Q rows of W_qkv and b_qkv here, before
    // the weights are rounded to the operand type.
    const float qscale = (float)(1.4426950408889634 / sqrt((double)dh));
    std::vector<float> in_w((size_t)3 * H * H), in_b((size_t)3 * H);
    for (int l = 0; l < L; ++l) {
        DevLayer& d = e->layers[l];
        for (size_t i = 0; i < in_w.size(); ++i) in_w[i] = wts->in_proj_weight[l][i] * (i < (size_t)H * H ? qscale : 1.0f);
        for (int i = 0; i < 3 * H; ++i) in_b[i] = wts->in_proj_bias[l][i] * (i < H ? qscale : 1.0f);
        const float *wq = in_w.data(), *wo = wts->out_proj_weight[l], *w1 = wts->linear1_weight[l], *w2 = wts->linear2_weight[l];
        // output features in paired-block order (pair_row, ppg_device.h): tile row r computes feature pair_row(r);
        // pair_k: the K columns in that order too
        auto paired = [&](const float* w, int rows, int cols, bool pair_rows, bool pair_k, char** dst) {
            return pk.matrix(rows, cols, rows, cols, [&](int r, int c) { return w[(size_t)(pair_rows ? pair_row(r) : r) * cols + (pair_k ? pair_row(c) : c)]; }, dst);
        };
        if ((rc = paired(wq, 3 * H, H, true, false, &d.wqkv))) return rc;
        if ((rc = paired(wo, H, H, true, false, &d.wo))) return rc;
        if ((rc = paired(w1, F, H, false, false, &d.w1))) return rc;
        if ((rc = paired(w2, H, F, true, false, &d.w2))) return rc;
        d.wqkvk = d.wqkv;
        d.w1k = d.w1;
        if (pk.fmt == Fmt::F32) {   // the fused kernels hand LN's fp32 accumulators on in paired K order
            if ((rc = paired(wq, 3 * H, H, true, true, &d.wqkvk))) return rc;
            if ((rc = paired(w1, F, H, false, true, &d.w1k))) return rc;
        }
        {   // pack_w2: k-slot order of the fused FFN's phase-B fragments.
            // bf16: inside each 32-wide hidden group, slot 8g + 4e + r holds
            // hidden 16e + 4g + r (the two phase-A accumulators e of lane
            // group g, concatenated).  fp32: natural order.
            const bool bf = pk.fmt != Fmt::F32;
            rc = pk.matrix(H, F, H, F,
                           [&](int row, int c) {
                               const int r = pair_row(row);
                               if (!bf) return w2[(size_t)r * F + c];
                               const int grp = c / 32, s = c % 32, g = s / 8, ee = (s % 8) / 4, rr = s % 4;
                               return w2[(size_t)r * F + grp * 32 + 16 * ee + 4 * g + rr];
                           },
                           &d.w2p);
            if (rc) return rc;
        }
        // the Q | K | V row of step `st` = (kind, rb) of wave w: Q and K rows in the order phi, V rows in attn_kernel's
        // tile order (V^T row r = natural feature pair_row(r))
        auto qkv_row = [&](int w, int st, int ln) {
            const int rb = st % RB, kind = st / RB;
            return kind < 2 ? kind * H + wave_row(w, rb, ln) : 2 * H + pair_row(32 * RB * w + 32 * rb + (ln & 31));
        };
        if (e->layer32) {   // ppg_layer32.hip
            rc = pk.image(4 * RB * KS, [&](int f, int ln, int j) {          // [w][rb][ks], natural K (the attention output's)
                const int ks = f % KS, rb = (f / KS) % RB, w = f / (KS * RB);
                return wo[(size_t)wave_row(w, rb, ln) * H + frag_k(ks, ln, j)];
            }, &d.wo_img);
            if (rc) return rc;
            rc = pk.image(F / 128 * 4 * KS, [&](int f, int ln, int j) {     // [chunk][w][ks], rows natural, K = the x1 panel
                const int ks = f % KS, w = (f / KS) & 3, ch = f / (KS * 4);
                return w1[(size_t)(ch * 128 + 32 * w + (ln & 31)) * H + panel_k(ks, ln, j)];
            }, &d.w1_img);
            if (rc) return rc;
            rc = pk.image(F / 128 * 4 * RB * 8, [&](int f, int ln, int j) { // [chunk][w][rb][ks8], K = the chunk's h in accumulator order
                const int ks = f & 7, rb = (f >> 3) % RB, w = (f / (8 * RB)) & 3, ch = f / (8 * RB * 4);
                return w2[(size_t)wave_row(w, rb, ln) * F + ch * 128 + hidden_k(ks, ln, j)];
            }, &d.w2_img);
            if (rc) return rc;
            // W_qkv of THIS layer (the previous layer's kernel runs it as its tail): per wave 3 RB steps of 32 rows; K = the x2 panel (as W1)
            rc = pk.image(4 * 3 * RB * KS, [&](int f, int ln, int j) {      // [w][step][ks]
                const int ks = f % KS, st = (f / KS) % (3 * RB), w = f / (KS * 3 * RB);
                return wq[(size_t)qkv_row(w, st, ln) * H + panel_k(ks, ln, j)];
            }, &d.wq_img);
            if (rc) return rc;
        }
        if (e->split() && e->ffn32x2 && ppg::ffn32x2_supported(H, F)) {      // (an engine outside it -- F > 3328 -- keeps the token-split kernels)
            // ppg_ffn32x2.hip (hidden 256: RB = 2, a K half = 8 K-steps): every A fragment as its fp16 hi and lo planes.
            // W1: [chunk][wave][plane][ks], rows natural, K natural (the panel is loaded in natural order);
            // W2: [chunk][wave][plane][rb][ks8], rows in the order phi, K = the chunk's h in accumulator order
            rc = pk.image_hilo(F / 128 * 4, [&](int g, int ks, int ln, int j) {
                const int w = g & 3, ch = g >> 2;
                return w1[(size_t)(ch * 128 + 32 * w + (ln & 31)) * H + frag_k(ks, ln, j)];
            }, &d.w1x_img);
            if (rc) return rc;
            rc = pk.image_hilo(F / 128 * 4, [&](int g, int f, int ln, int j) {
                const int w = g & 3, ch = g >> 2, rb = f >> 3, ks = f & 7;
                return w2[(size_t)wave_row(w, rb, ln) * F + ch * 128 + hidden_k(ks, ln, j)];
            }, &d.w2x_img);
            if (rc) return rc;
            // Wo: [wave][K half][plane][rb][ks8], K natural (the attention output's)
            rc = pk.image_hilo(4 * 2, [&](int g, int f, int ln, int j) {
                const int kh = g & 1, w = g >> 1, rb = f >> 3, ks = f & 7;
                return wo[(size_t)wave_row(w, rb, ln) * H + frag_k(8 * kh + ks, ln, j)];
            }, &d.wox_img);
            if (rc) return rc;
            // W_qkv of THIS layer (the previous layer's launch runs it as its tail): [wave][kind][K half][plane][rb][ks8]
            rc = pk.image_hilo(4 * 3 * 2, [&](int g, int f, int ln, int j) {
                const int kh = g & 1, kind = (g >> 1) % 3, w = g / 6, rb = f >> 3, ks = f & 7;
                return wq[(size_t)qkv_row(w, kind * RB + rb, ln) * H + frag_k(8 * kh + ks, ln, j)];
            }, &d.wqx_img);
            if (rc) return rc;
        }
        const struct { const float* src; int n; float** dst; } vectors[] = {
            {in_b.data(), 3 * H, &d.bqkv}, {wts->out_proj_bias[l], H, &d.bo}, {wts->linear1_bias[l], F, &d.b1}, {wts->linear2_bias[l], H, &d.b2},
            {wts->norm1_weight[l], H, &d.g1}, {wts->norm1_bias[l], H, &d.e1}, {wts->norm2_weight[l], H, &d.g2}, {wts->norm2_bias[l], H, &d.e2}};
        for (const auto& v : vectors) if ((rc = pk.upload_f32(v.src, v.n, 0, v.dst))) return rc;
    }
    *out = e.release();
    return PPG_OK;
}

void ppg_engine_destroy(PpgEngine* engine) { delete engine; }

int ppg_plan_windows(const PpgEngine* engine, int batch, int frames, const int64_t* lengths,
                     int legacy_mode, PpgWindow* windows, int max_windows, PpgPlanInfo* info) {
    Plan plan;
    int rc = plan_for(engine, batch, frames, lengths, legacy_mode, &plan);
    if (rc) return rc;
    if (engine) finish_plan(engine, &plan);
    if (info) *info = plan.info;
    const int n = (int)plan.all.size();
    if (windows) for (int i = 0; i < n && i < max_windows; ++i) windows[i] = plan.all[i];
    return n;
}

int ppg_plan_attention_items(const PpgEngine* engine, int batch, int frames, const int64_t* lengths,
                             int legacy_mode, int heads, PpgAttentionItem* items, int max_items) {
    Plan plan;
    const int head_dim = engine ? engine->head_dim : 128, qt = ppg::attn_query_tile(head_dim);
    if (engine) heads = engine->cfg.heads;
    if (heads <= 0) return fail(PPG_EINVAL, "heads=%d", heads);
    int rc = plan_for(engine, batch, frames, lengths, legacy_mode, &plan);
    if (rc) return rc;
    if (engine) finish_plan(engine, &plan);
    else split_groups(&plan, 1, qt, heads, head_dim == 128);
    int n = 0, wbase = 0;
    for (const PlanGroup& grp : plan.groups) {
        for (const AttnItem& it : grp.items) {
            if (items && n < max_items)
                items[n] = PpgAttentionItem{wbase + it.window, it.q0, it.narrow ? qt / 2 : qt, it.frames, it.valid, it.narrow};
            ++n;
        }
        wbase += (int)grp.windows.size();
    }
    return n;
}

int ppg_workspace_bytes(const PpgEngine* engine, int batch, int frames, const int64_t* lengths,
                        int legacy_mode, size_t* bytes) {
    if (!engine || !bytes) return fail(PPG_EINVAL, "null argument");
    PpgPlanInfo info;
    int rc = ppg_plan_windows(engine, batch, frames, lengths, legacy_mode, nullptr, 0, &info);
    if (rc < 0) return rc;
    *bytes = info.workspace_bytes;
    return PPG_OK;
}

int ppg_encode(PpgEngine* e, const void* features, int feature_dtype, const int64_t* lengths,
               int batch, int frames, int softmax, int legacy_mode, float* out,
               void* workspace, size_t workspace_bytes, void* stream_) {
    if (!e || !features || !lengths || !out) return fail(PPG_EINVAL, "null argument");
    if (feature_dtype != PPG_DTYPE_F16 && feature_dtype != PPG_DTYPE_F32) return fail(PPG_EINVAL, "feature dtype %d", feature_dtype);
    std::lock_guard<std::mutex> lock(e->mu);
    HIP_OK(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream_);
    DevPlan* dp = nullptr;
    int rc = get_plan(e, batch, frames, lengths, legacy_mode, s, &dp);
    if (rc) return rc;
    const Plan& plan = dp->host;
    const PpgConfig& c = e->cfg;
    const int H = c.hidden_channels, F = c.ffn_channels, M = plan.info.tokens;
    const int prec = c.precision;
    const size_t out_elems = (size_t)batch * c.output_channels * frames;

    // exhausted windows (all keys masked): reference output there is
    // logits 0 -> uniform posteriors; nothing to compute.
    if (plan.info.skipped_windows > 0 || M == 0) {
        hipError_t he = ppg::launch_fill(out, out_elems, softmax ? 1.0f / c.output_channels : 0.f, s);
        if (he != hipSuccess) return fail(PPG_EDEVICE, "fill: %s", hipGetErrorString(he));
    }
    if (M == 0) return PPG_OK;

    if (!workspace || workspace_bytes < plan.info.workspace_bytes)
        return fail(PPG_EWORKSPACE, "workspace %zu bytes < required %zu", workspace_bytes, plan.info.workspace_bytes);
    if (reinterpret_cast<uintptr_t>(workspace) % 256) return fail(PPG_EINVAL, "workspace not 256-byte aligned");

    // One independent pipeline per plan group, each on its own stream.  A group's route -- its workspace, its tilings,
    // the kernel form of every layer -- is decided once per call; its launch sequence comes in SEGMENTS -- 0: the head
    // (gather, input convolution, layer 0's Q/K/V), 1 + l: layer l, 1 + layers: the output convolution -- and every
    // segment is enqueued once, by the function of its kind below.
    enum Form { kLayer32, kFfn32x2, kFfnFused, kFfnUnfused };
    struct Route {
        const PlanGroup* grp;
        hipStream_t s;
        Workspace ws;
        char *base, *xw, *qk, *vt, *ao, *hid, *Xb;
        float* X;
        const char* act_x;
        int lnt, lnt_ln;
        bool use32, sub32, head, fuse_op;
        Form form[PPG_MAX_LAYERS];
        bool qkv_done[PPG_MAX_LAYERS + 1];   // layer l's Q/K/V came out of the launch before it (layer 0's: out of the head kernel)
    };
    auto route_of = [&](const PlanGroup& grp, hipStream_t gs) {
        Route r{};
        r.grp = &grp; r.s = gs;
        const int M = grp.tokens;
        r.ws = layout(e, grp.tokens, grp.vt_tokens);
        r.base = static_cast<char*>(workspace) + grp.ws_offset;
        r.xw = r.base + r.ws.xw;
        r.X = reinterpret_cast<float*>(r.base + r.ws.x);
        r.Xb = (e->sz == 2 || e->split()) ? r.base + r.ws.xb : nullptr;
        r.qk = r.base + r.ws.qk;
        r.vt = r.base + r.ws.vt;
        r.ao = r.base + r.ws.ao;
        r.hid = r.base + r.ws.hid;
        r.act_x = (e->sz == 2 || e->split()) ? r.Xb : reinterpret_cast<const char*>(r.X);

        const int nt = choose_nt(e->num_cus, e->ffn_nt, M, e->sz == 2 ? 3 : 2);     // linear / conv kernels
        // linear / conv kernels: measured best at C2 (two 256-register workgroups
        // per CU): 32-token waves for the wide projections, 16-token waves where
        // the epilogue dominates (LayerNorm, softmax scatter)
        const bool forced = e->lin_nt >= 1 && e->lin_nt <= 3;
        r.lnt = forced ? e->lin_nt : std::min(nt, 2);
        r.lnt_ln = forced ? e->lin_nt : 1;

        r.use32 = e->layer32 && e->ffn_fused && r.ws.ffn_splits == 1;
        // (one 160-token tile per workgroup: below half a chip of tiles the three launches, with their smaller workgroups, are as fast)
        const int tiles32 = (M + ppg::layer32_tokens(H) - 1) / ppg::layer32_tokens(H);
        // sub-tile workgroups (two token blocks, three per tile) when whole tiles would leave two thirds of the CUs idle
        r.sub32 = r.use32 && e->subtile && H == 256 && (F / 128) % 2 == 0 && 3 * tiles32 <= e->num_cus;
        r.head = r.use32 && e->head32 && (2 * tiles32 >= e->num_cus || r.sub32);
        r.fuse_op = e->ffn_fused && e->op_fused && r.ws.ffn_splits == 1;
        r.qkv_done[0] = r.head;
        for (int l = 0; l < c.num_layers; ++l) {
            const bool more = l + 1 < c.num_layers;
            const bool x2_layer = e->split() && e->ffn32x2 > 0 && e->layers[l].w1x_img && 2 * ((M + ppg::ffn32x2_tokens() - 1) / ppg::ffn32x2_tokens()) >= e->num_cus;
            if (r.use32) { r.form[l] = kLayer32; r.qkv_done[l + 1] = e->qkv_fused && more; }
            else if (x2_layer) { r.form[l] = kFfn32x2; r.qkv_done[l + 1] = e->ffn32x2 >= 3 && more; }
            else if (e->ffn_fused) { r.form[l] = kFfnFused; r.qkv_done[l + 1] = r.fuse_op && e->qkv_fused && more; }
            else { r.form[l] = kFfnUnfused; r.qkv_done[l + 1] = false; }
        }
        return r;
    };
    auto rows_of = [](const Route& r) { return Rows{r.grp->d_blk, r.grp->d_win, r.grp->tokens, r.X, r.Xb}; };
    // a feature-split launch's Q/K/V tail: the projection `img` / `bq` of the layer that follows, into the pipeline's Q|K and V^T
    auto qkv_tail = [](auto* a, const Route& r, const char* img, const float* bq) {
        a->wq_img = img; a->bq = bq; a->qk_out = r.qk; a->vt_out = r.vt; a->vt_ld = r.ws.vt_ld;
        a->blk_win = r.grp->d_blk; a->win = r.grp->d_win;
    };

    auto enqueue_head = [&](const Route& r) -> int {
        const PlanGroup& grp = *r.grp;
        const int M = grp.tokens;
        if (r.head) {
            Timed t(e, PPG_K_INCONV, r.s);
            Head32Args a{};
            a.feats = features; a.dtype = feature_dtype; a.C = c.input_channels; a.T = frames; a.overlap = c.chunk_overlap;
            a.win_img = e->win_img; a.b_in = e->b_in; a.pe = e->pe; a.X = r.X;
            qkv_tail(&a, r, e->layers[0].wq_img, e->layers[0].bqkv);
            a.M = M; a.H = H;
            a.tiles = (M + ppg::layer32_tokens(H) - 1) / ppg::layer32_tokens(H);
            a.nwin = (int)grp.windows.size(); a.vt_rows = H; a.vt_tokens = grp.vt_tokens;
            set_qk_slack(e, r.qk, M, &a);
            a.debug_mode = e->h32_debug;
            a.x_half = e->x16;
            a.sub_tiles = r.sub32;
            a.dbg = e->head_dbg;
            LAUNCH_OK(ppg::launch_head32(prec, a, r.s), "head32");
            return PPG_OK;
        }
        {
            Timed t(e, PPG_K_GATHER, r.s);
            const GatherArgs g = gather_args(e, rows_of(r), features, feature_dtype, frames, r.xw, r.qk, r.vt, r.ws.vt_ld, grp.vt_tokens, (int)grp.windows.size());
            LAUNCH_OK(ppg::launch_gather(prec, g, r.s), "gather");
        }
        Timed t(e, PPG_K_INCONV, r.s);
        LinearArgs a = inconv_args(e, rows_of(r), r.xw);
        a.x_tiled = r.use32 ? (e->x16 ? 2 : 1) : 0;
        if (e->lin_dbg_class == PPG_K_INCONV) a.dbg = e->lin_dbg;
        LAUNCH_OK(ppg::launch_linear(prec, EPI_INCONV, 16, r.lnt, a, H / 256, r.s), "in-conv");
        return PPG_OK;
    };

    auto enqueue_layer = [&](const Route& r, int l) -> int {
        const PlanGroup& grp = *r.grp;
        const int M = grp.tokens;
        const Rows rows = rows_of(r);
        const DevLayer& d = e->layers[l];
        const bool qkv_next = r.qkv_done[l + 1];   // this launch computes the next layer's Q/K/V as its tail
        if (!r.qkv_done[l]) {
            Timed t(e, PPG_K_QKV, r.s);
            LinearArgs a = qkv_args(e, rows, d, r.act_x, r.qk, r.vt, r.ws.vt_ld);
            if (l == 0 && e->lin_dbg_class == PPG_K_QKV) a.dbg = e->lin_dbg;
            LAUNCH_OK(ppg::launch_linear(prec, EPI_QKV, 16, r.lnt, a, 3 * H / 256, r.s), "qkv");
        }
        {
            Timed t(e, PPG_K_ATTENTION, r.s);
            AttnArgs a = attn_args(e->sz, H, c.heads, c.is_causal, r.qk, r.vt, r.ws.vt_ld, r.ao, grp.d_items, grp.d_win, M);
            a.ao_tiled = r.use32;
            a.dbg = l == 0 ? e->attn_dbg : nullptr;
            LAUNCH_OK(ppg::launch_attn(prec, a, (int)grp.items.size(), c.heads, e->head_dim, r.s), "attention");
        }
        if (r.form[l] == kLayer32) {
            Timed t(e, PPG_K_FFN, r.s);
            Layer32Args a{};
            a.ao = r.ao; a.wo_img = d.wo_img; a.w1_img = d.w1_img; a.w2_img = d.w2_img;
            a.bo = d.bo; a.g1 = d.g1; a.e1 = d.e1; a.b1 = d.b1; a.b2 = d.b2; a.g2 = d.g2; a.e2 = d.e2;
            a.X = r.X; a.Xb = r.Xb; a.M = M; a.F = F; a.H = H; a.dbg = l == 0 ? e->ffn_dbg : nullptr;
            a.debug_mode = e->l32_debug;
            a.x_half = e->x16;
            a.sub_tiles = r.sub32;
            a.write_x = l + 1 < c.num_layers;
            if (qkv_next) {
                qkv_tail(&a, r, e->layers[l + 1].wq_img, e->layers[l + 1].bqkv);
                a.Xb = nullptr;              // nobody reads the 16-bit copy: x2 goes straight into the tail
            }
            LAUNCH_OK(ppg::launch_layer32(prec, a, r.s), "layer32");
            return PPG_OK;
        }
        if (!r.fuse_op && !(r.form[l] == kFfn32x2 && e->ffn32x2 >= 2)) {
            Timed t(e, PPG_K_OUTPROJ_LN, r.s);
            LinearArgs a = outproj_ln_args(e, rows, d, r.ao);
            if (l == 0 && e->lin_dbg_class == PPG_K_OUTPROJ_LN) a.dbg = e->lin_dbg;
            LAUNCH_OK(ppg::launch_linear(prec, EPI_RESLN, H / 16, r.lnt_ln, a, 1, r.s), "out-proj+LN");
        }
        Timed t(e, PPG_K_FFN, r.s);
        if (r.form[l] == kFfn32x2) {
            Ffn32X2Args a{};
            a.xb = r.Xb; a.X = r.X; a.xb_out = r.Xb; a.w1_img = d.w1x_img; a.w2_img = d.w2x_img;
            a.b1 = d.b1; a.b2 = d.b2; a.g2 = d.g2; a.e2 = d.e2; a.M = M; a.F = F; a.H = H;
            if (e->ffn32x2 >= 2) { a.ao = r.ao; a.wo_img = d.wox_img; a.bo = d.bo; a.g1 = d.g1; a.e1 = d.e1; }
            a.dbg = l == 0 ? e->ffn_dbg : nullptr;
            if (qkv_next) qkv_tail(&a, r, e->layers[l + 1].wqx_img, e->layers[l + 1].bqkv);
            LAUNCH_OK(ppg::launch_ffn32x2(a, r.s), "ffn32x2");
        } else if (r.form[l] == kFfnFused) {
            FfnArgs a = ffn_args(e, rows, d, r.ws.ffn_splits, reinterpret_cast<float*>(r.base + r.ws.part));
            a.dbg = l == 0 ? e->ffn_dbg : nullptr;
            if (r.fuse_op) ffn_fuse_outproj(&a, d, r.ao);
            if (qkv_next) ffn_fuse_qkv(&a, rows, e->layers[l + 1], r.qk, r.vt, r.ws.vt_ld);
            LAUNCH_OK(ppg::launch_ffn(prec, a, r.ws.ffn_nt, r.s), "ffn");
        } else {   // the FFN as two GEMMs through the [tokens][ffn] buffer
            LinearArgs a = gemm_args(e, rows, r.act_x, H, d.w1, d.b1, F);
            a.out_rows = r.hid; a.out_ld = F;
            LAUNCH_OK(ppg::launch_linear(prec, EPI_RELU, 16, r.lnt, a, F / 256, r.s), "ffn1");
            LinearArgs b = gemm_args(e, rows, r.hid, F, d.w2, d.b2, H);
            b.gamma = d.g2; b.beta = d.e2;
            LAUNCH_OK(ppg::launch_linear(prec, EPI_RESLN, H / 16, r.lnt_ln, b, 1, r.s), "ffn2+LN");
        }
        return PPG_OK;
    };

    auto enqueue_outconv = [&](const Route& r) -> int {
        Timed t(e, PPG_K_OUTCONV_SOFTMAX, r.s);
        LinearArgs a = outconv_args(e, rows_of(r), r.act_x, out, frames, softmax);
        if (e->lin_dbg_class == PPG_K_OUTCONV_SOFTMAX) a.dbg = e->lin_dbg;
        if (e->outconv && ppg::outconv_supported(prec, a)) LAUNCH_OK(ppg::launch_outconv(prec, a, r.s), "out-conv+softmax");
        else LAUNCH_OK(ppg::launch_linear(prec, EPI_OUTCONV, 3, r.lnt_ln, a, 1, r.s), "out-conv+softmax");
        return PPG_OK;
    };

    std::vector<Route> routes;
    routes.reserve(plan.groups.size());
    for (size_t gi = 0; gi < plan.groups.size(); ++gi) routes.push_back(route_of(plan.groups[gi], gi == 0 ? s : e->side_streams[gi - 1]));
    // The pipelines' launches are enqueued segment by segment, alternately: enqueued one whole pipeline after the
    // other, the second one's first kernel reached its queue ~50 us (a dozen launches) behind the first one's -- nothing
    // in a loop of steps, where the host runs ahead of the device, but the first step of a short timed block (and a
    // latency-bound caller's only step) started one pipeline that much late (tools/block_overhead.py).
    return fork_join(s, e->ev_fork, e->side_streams.data(), e->ev_join.data(), routes.size() - 1, [&]() -> int {
        for (int seg = 0; seg < c.num_layers + 2; ++seg)
            for (const Route& r : routes) {
                const int rc = seg == 0 ? enqueue_head(r) : seg <= c.num_layers ? enqueue_layer(r, seg - 1) : enqueue_outconv(r);
                if (rc) return rc;
            }
        return PPG_OK;
    });
}

int ppg_engine_nonfinite(PpgEngine* e, int clear, int* flag) {
    if (!e || !flag) return fail(PPG_EINVAL, "null argument");
    if (!e->d_overflow) { *flag = 0; return PPG_OK; }
    std::lock_guard<std::mutex> lock(e->mu);
    HIP_OK(hipSetDevice(e->device));
    unsigned value = 0;
    HIP_OK(hipMemcpy(&value, e->d_overflow, sizeof(value), hipMemcpyDeviceToHost));      // (synchronises with the device)
    if (value && clear) HIP_OK(hipMemset(e->d_overflow, 0, sizeof(value)));
    *flag = (int)value;
    return PPG_OK;
}

int ppg_engine_pipelines(const PpgEngine* e, int tokens) {
    if (!e || tokens < 0) return 0;
    return group_count(e, tokens);
}

int ppg_engine_profile(PpgEngine* e, int enable) {
    if (!e) return fail(PPG_EINVAL, "null engine");
    e->profiling = (unsigned)enable;
    // a first pool of event pairs per enabled class, so that a short timed region does not pay for creating them
    if (enable) (void)hipSetDevice(e->device);
    for (int cls = 0; enable && cls < PPG_K_COUNT; ++cls) {
        if (!(e->profiling & (1u << cls))) continue;
        while (e->events[cls].size() < 32) {
            EventPair p;
            if (hipEventCreateWithFlags(&p.a, kTimingEventFlags) != hipSuccess || hipEventCreateWithFlags(&p.b, kTimingEventFlags) != hipSuccess) break;
            e->events[cls].push_back(p);
        }
    }
    return PPG_OK;
}

int ppg_engine_profile_reset(PpgEngine* e) {
    if (!e) return fail(PPG_EINVAL, "null engine");
    for (auto& u : e->events_used) u = 0;
    for (auto& q : e->launch_seq) q = 0;
    return PPG_OK;
}

int ppg_engine_profile_stride(PpgEngine* e, int stride) {
    if (!e || stride < 1) return fail(PPG_EINVAL, "profile stride must be >= 1");
    e->profile_stride = stride;
    return PPG_OK;
}

int ppg_engine_profile_read(PpgEngine* e, int cls, double* total_ms, int64_t* launches) {
    if (!e || cls < 0 || cls >= PPG_K_COUNT || !total_ms || !launches) return fail(PPG_EINVAL, "bad argument");
    *launches = (int64_t)e->events_used[cls];
    return elapsed_total(e->events[cls], e->events_used[cls], total_ms);
}

}  // extern "C"
