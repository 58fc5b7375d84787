// KV-cached streaming of the causal model (ppg_stream_*): the stream object, its append kernel, one step's launches.
#include "ppg_host.h"

using namespace ppg;

extern "C" {

// ----------------------------------------------------------------------------
// Streaming causal mode: one utterance, frames arrive in
// chunks, the K / V^T rows and the residual rows of everything seen so far stay
// on the device.  The reference defines no streaming state
// (config/causal_transformer.py:18 only adds the causal mask): what this
// reproduces is the causal forward of the WHOLE utterance (one window, <= the
// chunk length), emitted incrementally.  With a causal mask, row t of every layer
// depends on rows <= t of the layer below -- except for the two k = 5 'same'
// convolutions (+-2 frames each).  After F frames:
//   rows < F - 2 of the residual stream and of every layer are final,
//   posteriors of rows < F - 4 are final (all of them after `flush`).
// A step recomputes from the last 16-row block boundary at or below the previous
// frontier (the kernels work on whole 16-row blocks; recomputing a row gives the
// same bits), on ROW RANGES of the token-split kernels: pointers advanced by
// row0, the window table's tok_off lowered by row0 so that window positions
// (PE, masks, V^T columns) stay absolute.
// ----------------------------------------------------------------------------
// A stream object holds `batch` utterances (ppg_stream_create: one), each ONE window of up to `cap` frames, in one
// token space: item b owns rows b R .. (b + 1) R - 1 of every buffer (R = cap rounded up to 32), its own window
// record (position b R, valid = its frontier) and its own K | Q / V^T rows in the per-layer caches.  A step advances
// all items by their own -- ragged, unaligned -- numbers of frames in ONE launch sequence: the launches of the
// token-split kernels take a ROW MAP (the 16-row blocks the step touches, of any items, one per wave) instead of a
// contiguous row range, the attention launch takes the items' query tiles.  Rows are recomputed from the last block
// boundary at or below an item's previous frontier; a recomputed row gives the same bits (the hidden chunks are
// walked in a fixed order and summed in a fixed number of groups under a row map; attention re-bases a query's softmax
// shift on that query's own sums alone): an item's outputs depend neither on the push cadence nor on what the other
// items do (tests/test_gpu_stream_probe.py holds both, bit for bit).
struct StreamItemMeta { int row0; int received_before; int count; int pad; };
__global__ void stream_append_kernel(const StreamItemMeta* meta, const char* chunk, int nmax, int C, int R, int esz, char* feats) {
    const int b = blockIdx.y;
    const StreamItemMeta m = meta[b];
    const int total = C * m.count;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int c = i / m.count, t = i - c * m.count;
        const char* src = chunk + (((size_t)b * C + c) * nmax + t) * esz;
        char* dst = feats + (((size_t)b * C + c) * R + m.received_before + t) * esz;
        if (esz == 2) *reinterpret_cast<uint16_t*>(dst) = *reinterpret_cast<const uint16_t*>(src);
        else *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(src);
    }
}

struct PpgStream {
    PpgEngine* e = nullptr;
    int batch = 1, cap = 0, rows = 0, dtype = 0;      // rows = R, per item
    Workspace ws{};
    char* buf = nullptr;          // workspace
    char* feats = nullptr;        // (batch, C, rows) in `dtype`
    float* probs = nullptr;       // (batch, output_channels, rows)
    int* d_blk = nullptr;
    char* d_tables = nullptr;     // one step's tables (layout: Tables)
    int* d_tickets = nullptr;     // one-pass split-hidden FFN: a counter per token tile, zero between launches (FfnArgs::tickets)
    size_t qk_bytes = 0, vt_bytes = 0, cache_off = 0, part_off = 0;
    int max_splits = 1;           // hidden splits of the FFN launches (a step's few rows cannot stream the weights through few CUs fast enough)
    int ffn_groups = 1;           // the hidden GROUPS every FFN launch of this stream sums in; fixed for the life of the stream (below)
    std::vector<int> received, x_valid, o_valid;
    std::vector<char> finished;
    std::vector<int> map_scratch;
    // per-step tables, uploaded with ONE copy from a pinned slot (asynchronous: the source must outlive the call)
    struct Tables {
        size_t win = 0, meta = 0, items = 0, maps = 0, bytes = 0;   // byte offsets: win[3][batch], meta[batch], items[max_items], maps[3][max_blocks]
        int max_items = 0, max_blocks = 0;
    } tb;
    static constexpr int kSlots = 8;
    char* staging = nullptr;
    hipEvent_t uploaded[kSlots] = {};
    unsigned step = 0;
    bool fused_layers = false;    // PPGS_AMD_STREAM_FUSED=2 at creation: every step's layers as ONE fused launch each (for streams pushed in whole chunks); fixed for the life of the stream
    ~PpgStream() {
        if (e) (void)hipSetDevice(e->device);
        for (void* p : {(void*)buf, (void*)feats, (void*)probs, (void*)d_blk, (void*)d_tables, (void*)d_tickets}) if (p) (void)hipFree(p);
        if (staging) (void)hipHostFree(staging);
        for (hipEvent_t ev : uploaded) if (ev) (void)hipEventDestroy(ev);
    }
};

int ppg_stream_create_batch(PpgEngine* e, int batch, int max_frames, int feature_dtype, PpgStream** out) {
    if (!e || !out) return fail(PPG_EINVAL, "null argument");
    if (!e->cfg.is_causal) return fail(PPG_EINVAL, "streaming needs a causal engine (is_causal = 1)");
    if (batch < 1 || batch > 4096) return fail(PPG_EINVAL, "batch %d outside [1, 4096]", batch);
    if (max_frames < 1 || max_frames > e->cfg.chunk_length)
        return fail(PPG_ELENGTH, "max_frames %d outside [1, %d] (one window)", max_frames, e->cfg.chunk_length);
    if (feature_dtype != PPG_DTYPE_F16 && feature_dtype != PPG_DTYPE_F32) return fail(PPG_EINVAL, "feature dtype %d", feature_dtype);
    if (e->split() && !e->ffn_fused) return fail(PPG_EINVAL, "the fp16x2 mode has no KV-cached stream at hidden %d", e->cfg.hidden_channels);
    std::lock_guard<std::mutex> lock(e->mu);
    HIP_OK(hipSetDevice(e->device));
    std::unique_ptr<PpgStream> st(new PpgStream);
    st->e = e; st->batch = batch; st->cap = max_frames; st->rows = round_up(max_frames, 32); st->dtype = feature_dtype;
    st->fused_layers = ppg::env_switch("PPGS_AMD_STREAM_FUSED", 0) == 2;
    st->received.assign(batch, 0); st->x_valid.assign(batch, 0); st->o_valid.assign(batch, 0); st->finished.assign(batch, 0);
    const PpgConfig& c = e->cfg;
    const int R = st->rows, MT = batch * R;
    st->ws = layout(e, MT, MT);
    // K | Q rows and V^T per LAYER (the one-shot forward reuses one pair for all layers; here they are the cache)
    st->qk_bytes = align_up((size_t)st->ws.qk_rows * 2 * c.hidden_channels * e->sz, 256);
    st->vt_bytes = align_up((size_t)c.hidden_channels * st->ws.vt_ld * e->sz, 256);
    // partial sums of the split-hidden FFN launches: [splits][batch * R][H] fp32, at most 256 MiB
    {
        const int chunks = ppg::ffn_chunks(c.hidden_channels, c.ffn_channels, e->sz);    // (a split count must divide them)
        // (under a row map a split's rows are slot-dense, ceil(map_blocks / 4) * 64 of them -- ppg_ffn.h, ffn_body's
        // epilogue and the reduce pass: up to MT rounded up to a whole 64-row workgroup, not MT)
        const size_t per_split = (size_t)round_up(MT, 64) * c.hidden_channels * 4;
        st->max_splits = 1;
        while (st->max_splits * 2 <= std::max(1, chunks / 2) && chunks % (st->max_splits * 2) == 0 && (size_t)(st->max_splits * 2) * per_split <= ((size_t)256 << 20)) st->max_splits *= 2;
        st->part_off = align_up(st->ws.total, 256);
        st->cache_off = align_up(st->part_off + (st->max_splits > 1 ? st->max_splits * per_split : 0), 256);
    }
    const size_t bytes = st->cache_off + (size_t)c.num_layers * (st->qk_bytes + st->vt_bytes);
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&st->buf), bytes));
    HIP_OK(hipMemset(st->buf, 0, bytes));
    const size_t esz = feature_dtype == PPG_DTYPE_F16 ? 2 : 4;
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&st->feats), (size_t)batch * c.input_channels * R * esz));
    HIP_OK(hipMemset(st->feats, 0, (size_t)batch * c.input_channels * R * esz));
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&st->probs), (size_t)batch * c.output_channels * R * 4));
    HIP_OK(hipMemset(st->probs, 0, (size_t)batch * c.output_channels * R * 4));
    // block -> window: block k belongs to item k / (R / 16)
    {
        std::vector<int> blk(MT / 16 + 8, -1);
        for (int k = 0; k < MT / 16; ++k) blk[k] = k / (R / 16);
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&st->d_blk), blk.size() * sizeof(int)));
        HIP_OK(hipMemcpy(st->d_blk, blk.data(), blk.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    PpgStream::Tables& tb = st->tb;
    const int tile = stream_query_tile(e->head_dim);
    tb.max_items = batch * (R / tile + 1);
    tb.max_blocks = round_up(MT / 16, 4) + 4;
    size_t off = 0;
    tb.win = off; off = align_up(off + 3 * (size_t)batch * sizeof(PpgWindow), 64);
    tb.meta = off; off = align_up(off + (size_t)batch * sizeof(StreamItemMeta), 64);
    tb.items = off; off = align_up(off + (size_t)tb.max_items * sizeof(AttnItem), 64);
    tb.maps = off; off = align_up(off + 3 * align_up((size_t)tb.max_blocks * sizeof(int), 64), 64) + 256;   // (packed per step, each map 64-byte aligned)
    tb.bytes = off;
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&st->d_tables), tb.bytes));
    HIP_OK(hipMemset(st->d_tables, 0, tb.bytes));
    if (e->stream_one_pass && c.hidden_channels == 256 && e->ffn_fused) {
        const size_t tiles = (size_t)tb.max_blocks / 4 + 4;
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&st->d_tickets), tiles * sizeof(int)));
        HIP_OK(hipMemset(st->d_tickets, 0, tiles * sizeof(int)));
    }
    // The split-hidden FFN sums the hidden chunks in GROUPS: every group from zero, the groups' sums in order, bias + residual
    // last.  The number of groups is a property of the STREAM: chosen per step (as many splits as fill the chip), a step of
    // many row blocks and a step of few summed in different orders, and the final rows of a frontier block -- recomputed by
    // the next step, their X and K / V rows rewritten -- depended on the push cadence in the last bits
    // (tests/test_gpu_stream_probe.py), against "a recomputed row gives the same bits".  The count is what the per-step rule
    // gave a step of 16 frames per item (two row blocks each), the step the four-launch form is for; how the groups are
    // spread over workgroups is still chosen per step (ppg_stream_push_batch) and does not change the arithmetic.
    if (e->ffn_split && st->max_splits > 1) {
        const int wgs = (2 * batch + 3) / 4;
        int cap = e->ffn_split_max > 0 ? std::min(e->ffn_split_max, st->max_splits) : st->max_splits;
        if (st->d_tickets) cap = std::min(cap, e->ffn_split_max > 0 ? 8 : 4);   // (one-pass form: the last workgroup sums the partial rows itself)
        while (st->ffn_groups * 2 <= cap && wgs * st->ffn_groups * 2 <= e->num_cus) st->ffn_groups *= 2;
    }
    HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&st->staging), PpgStream::kSlots * tb.bytes, hipHostMallocDefault));
    for (hipEvent_t& ev : st->uploaded) HIP_OK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIP_OK(hipDeviceSynchronize());
    *out = st.release();
    return PPG_OK;
}

int ppg_stream_create(PpgEngine* e, int max_frames, int feature_dtype, PpgStream** out) {
    return ppg_stream_create_batch(e, 1, max_frames, feature_dtype, out);
}

void ppg_stream_destroy(PpgStream* stream) { delete stream; }

int ppg_stream_rows(const PpgStream* st, int* rows, int* received, int* final_frames) {
    if (!st) return fail(PPG_EINVAL, "null argument");
    if (rows) *rows = st->rows;
    if (received) *received = st->received[0];
    if (final_frames) *final_frames = st->o_valid[0];
    return PPG_OK;
}

int ppg_stream_batch(const PpgStream* st) { return st ? st->batch : 0; }

const float* ppg_stream_posteriors(const PpgStream* st) { return st ? st->probs : nullptr; }

int ppg_stream_push_batch(PpgStream* st, const void* chunk, int nmax, const int* counts, const int* flush, int softmax,
                          int* first_final, int* num_final, void* stream_) {
    if (!st || !counts || nmax < 0) return fail(PPG_EINVAL, "bad argument");
    PpgEngine* e = st->e;
    const int B = st->batch, R = st->rows;
    bool any_frames = false;
    for (int b = 0; b < B; ++b) {
        const int n = counts[b];
        if (n < 0 || n > nmax) return fail(PPG_EINVAL, "item %d: %d frames outside [0, %d]", b, n, nmax);
        if (n > 0 || (flush && flush[b])) {
            if (st->finished[b]) return fail(PPG_EINVAL, "item %d: the stream was flushed", b);
            if (st->received[b] + n > st->cap) return fail(PPG_ELENGTH, "item %d: %d + %d frames > max_frames %d", b, st->received[b], n, st->cap);
        }
        any_frames = any_frames || n > 0;
    }
    if (any_frames && !chunk) return fail(PPG_EINVAL, "null chunk");
    std::lock_guard<std::mutex> lock(e->mu);
    HIP_OK(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const PpgConfig& c = e->cfg;
    const int H = c.hidden_channels, prec = c.precision, MT = B * R;
    const int esz = st->dtype == PPG_DTYPE_F16 ? 2 : 4;
    const PpgStream::Tables& tb = st->tb;

    const unsigned slot_index = st->step++ % PpgStream::kSlots;
    char* stage = st->staging + (size_t)slot_index * tb.bytes;
    HIP_OK(hipEventSynchronize(st->uploaded[slot_index]));               // (its last use, kSlots steps ago, is long done)
    PpgWindow* win = reinterpret_cast<PpgWindow*>(stage + tb.win);       // [0] linear launches, [1] out-conv, [2] gather
    StreamItemMeta* meta = reinterpret_cast<StreamItemMeta*>(stage + tb.meta);
    AttnItem* items = reinterpret_cast<AttnItem*>(stage + tb.items);
    // the three row maps ([0] residual rows, [1] posterior rows, [2] gathered rows) are collected here and packed
    // right behind the items in use: the step uploads what it filled, not the tables' capacity
    std::vector<int>& maps = st->map_scratch;
    maps.assign(3 * (size_t)tb.max_blocks, 0);
    int nmap[3] = {0, 0, 0}, nitems = 0, max_count = 0;
    const int tile = stream_query_tile(e->head_dim);
    // the items' new frontiers are worked out on copies and committed only once every launch of the step is queued:
    // a step that fails half way (too many query tiles, a refused launch) leaves the stream where it was
    std::vector<int> received = st->received, x_valid = st->x_valid, o_valid = st->o_valid;
    std::vector<char> finished = st->finished;
    for (int b = 0; b < B; ++b) {
        const int n = counts[b];
        const bool fl = flush && flush[b];
        const bool active = n > 0 || fl;
        const int f_prev = received[b], x_prev = x_valid[b], o_prev = o_valid[b];
        if (active) received[b] += n;
        const int x_new = !active ? x_prev : (fl ? received[b] : std::max(received[b] - 2, 0));
        const int o_new = !active ? o_prev : (fl ? received[b] : std::max(x_new - 2, 0));
        if (first_final) first_final[b] = o_prev;
        if (num_final) num_final[b] = o_new - o_prev;
        if (fl) finished[b] = 1;
        x_valid[b] = x_new; o_valid[b] = o_new;
        // the item's window as the three kinds of launch see it
        PpgWindow w{};
        w.item = b; w.chunked = 0; w.start = 0; w.frames = R; w.valid = x_new;
        w.keep_lo = 0; w.keep_hi = R; w.out_frame = 0; w.vt_off = b * R; w.tok_off = b * R;
        win[b] = w;
        win[B + b] = w; win[B + b].frames = fl ? received[b] : R;    // out-conv: zero padding at the true end once it is known
        win[2 * B + b] = w;
        meta[b] = StreamItemMeta{b * R, f_prev, active ? n : 0, 0};
        max_count = std::max(max_count, meta[b].count);
        if (!active) continue;
        const int r0 = x_prev / 16 * 16, r1 = round_up(x_new, 16);          // rows of the residual stream to (re)compute
        const int g0 = f_prev / 16 * 16, g1 = round_up(received[b], 16);  // rows whose features changed
        const int o0 = o_prev / 16 * 16, o1 = round_up(o_new, 16);          // posterior rows
        for (int r = r0; r < r1; r += 16) maps[nmap[0]++] = b * R + r;
        for (int r = o0; r < o1; r += 16) maps[tb.max_blocks + nmap[1]++] = b * R + r;
        for (int r = g0; r < g1; r += 16) maps[2 * tb.max_blocks + nmap[2]++] = b * R + r;
        for (int q0 = r0 / tile * tile; q0 < r1; q0 += tile) {
            if (nitems == tb.max_items) return fail(PPG_EINVAL, "more than %d query tiles in one step", tb.max_items);
            items[nitems++] = AttnItem{b, q0, b * R, b * R, R, x_new, e->head_dim == 128 ? 1 : 0, 0};
        }
    }
    size_t map_off[3], used = align_up(tb.items + (size_t)nitems * sizeof(AttnItem), 64);
    for (int k = 0; k < 3; ++k) {
        const int padded = round_up(nmap[k], 4);                           // unused wave slots of the last workgroup: nothing to do
        for (int i = nmap[k]; i < padded; ++i) maps[k * tb.max_blocks + i] = MT;
        map_off[k] = used;
        memcpy(stage + used, maps.data() + (size_t)k * tb.max_blocks, (size_t)padded * sizeof(int));
        used = align_up(used + (size_t)padded * sizeof(int), 64);
    }
    HIP_OK(hipMemcpyAsync(st->d_tables, stage, used, hipMemcpyHostToDevice, s));
    const PpgWindow* d_win = reinterpret_cast<const PpgWindow*>(st->d_tables + tb.win);
    const StreamItemMeta* d_meta = reinterpret_cast<const StreamItemMeta*>(st->d_tables + tb.meta);
    const AttnItem* d_items = reinterpret_cast<const AttnItem*>(st->d_tables + tb.items);

    if (max_count > 0) {
        const int per_item = c.input_channels * max_count;
        hipLaunchKernelGGL(stream_append_kernel, dim3((per_item + 255) / 256, B), dim3(256), 0, s,
                           d_meta, static_cast<const char*>(chunk), nmax, c.input_channels, R, esz, st->feats);
        LAUNCH_OK(hipGetLastError(), "stream append");
    }
    char* base = st->buf;
    const Workspace& ws = st->ws;
    char* xw = base + ws.xw;
    float* X = reinterpret_cast<float*>(base + ws.x);
    char* Xb = (e->sz == 2 || e->split()) ? base + ws.xb : nullptr;
    char* ao = base + ws.ao;
    auto qk_of = [&](int l) { return base + st->cache_off + (size_t)l * (st->qk_bytes + st->vt_bytes); };
    auto vt_of = [&](int l) { return qk_of(l) + st->qk_bytes; };
    const char* act_x = (e->sz == 2 || e->split()) ? Xb : reinterpret_cast<const char*>(X);

    auto rows_of = [&](const PpgWindow* w, float* x, char* xb, int k) {      // the rows of map k
        return Rows{st->d_blk, w, MT, x, xb, reinterpret_cast<const int*>(st->d_tables + map_off[k]), nmap[k]};
    };
    if (nmap[2] > 0) {
        // (no window tails to clear: R is a multiple of 32; the caches were zeroed at creation)
        const GatherArgs g = gather_args(e, rows_of(d_win + 2 * B, nullptr, nullptr, 2), st->feats, st->dtype, R, xw, qk_of(0), vt_of(0), ws.vt_ld, MT, 0);
        LAUNCH_OK(ppg::launch_gather(prec, g, s), "stream gather");
    }
    if (nmap[0] > 0) {
        const Rows t = rows_of(d_win, X, Xb, 0);
        LAUNCH_OK(ppg::launch_linear(prec, EPI_INCONV, 16, 1, inconv_args(e, t, xw), H / 256, s), "stream in-conv");
        // The stream's hidden groups (ffn_groups, fixed at creation) as one workgroup per group and token tile -- hidden
        // splits, each streaming its share of W1 / W2: a step's few rows cannot stream the weights through few CUs fast
        // enough -- while that is at most two rounds of workgroups on the chip.  A bigger step walks all groups in ONE
        // workgroup per token tile, which closes its accumulator at the group boundaries and adds the sums in the reduce
        // pass's order and applies LayerNorm-2 in that pass's arithmetic (FfnArgs::groups, ffn_closed_kernel): the same bits,
        // no partial rows and no reduce launch (hidden 256; the hidden-512 kernel has no registers for the second accumulator
        // and keeps the splits).  Measured: 64 x 160 frames 760 us against 845 us always spread.
        const int ffn_wgs = (nmap[0] + 3) / 4;
        const bool ffn_closed = st->ffn_groups > 1 && H == 256 && ffn_wgs * st->ffn_groups > 2 * e->num_cus;
        const int ffn_splits = ffn_closed ? 1 : st->ffn_groups;
        // One launch per layer besides attention for BIG steps (round 5): out-projection + LayerNorm-1 + FFN + LayerNorm-2
        // + the NEXT layer's Q/K/V in the token-split fused kernel the one-shot forward uses for small batches, here under
        // the step's row map.  Its workgroups stream a whole layer's weights each (no hidden splits: a split would redo
        // the out-projection) -- ~85 us per layer however few they are, so only a step of >= 512 row blocks gains
        // (64 streams x 160 frames: 725 -> 639 us; 64 x 16: 363 -> 491 us, one stream 274 -> 432 us).  The form is a
        // property of the STREAM, fixed at creation (PPGS_AMD_STREAM_FUSED=2; default: the four launches): chosen per
        // step (round 5), a stream whose step sizes straddled the threshold computed a partially filled 16-row block
        // with two kernels of different accumulation order -- its cached K / V rows and the later recomputed X rows then
        // depended on the push cadence, against "a recomputed row gives the same bits wherever it lands".
        const bool fused = st->fused_layers && e->ffn_fused && e->op_fused && e->qkv_fused && !e->split();
        for (int l = 0; l < c.num_layers; ++l) {
            const DevLayer& d = e->layers[l];
            char *qk = qk_of(l), *vt = vt_of(l);
            if (!fused || l == 0)
                LAUNCH_OK(ppg::launch_linear(prec, EPI_QKV, 16, 1, qkv_args(e, t, d, act_x, qk, vt, ws.vt_ld), 3 * H / 256, s), "stream qkv");
            LAUNCH_OK(ppg::launch_attn(prec, attn_args(e->sz, H, c.heads, 1, qk, vt, ws.vt_ld, ao, d_items, d_win, MT), nitems, c.heads, e->head_dim, s), "stream attention");
            if (fused) {
                FfnArgs a = ffn_args(e, t, d, 1, nullptr);
                ffn_fuse_outproj(&a, d, ao);
                if (l + 1 < c.num_layers) ffn_fuse_qkv(&a, t, e->layers[l + 1], qk_of(l + 1), vt_of(l + 1), ws.vt_ld);
                LAUNCH_OK(ppg::launch_ffn(prec, a, 1, s), "stream fused layer");
                continue;
            }
            LAUNCH_OK(ppg::launch_linear(prec, EPI_RESLN, H / 16, 1, outproj_ln_args(e, t, d, ao), 1, s), "stream out-proj+LN");
            FfnArgs a = ffn_args(e, t, d, ffn_splits, reinterpret_cast<float*>(base + st->part_off));
            a.tickets = ffn_splits > 1 ? st->d_tickets : nullptr;
            if (ffn_closed) a.groups = st->ffn_groups;
            LAUNCH_OK(ppg::launch_ffn(prec, a, 1, s), "stream ffn");
        }
    }
    if (nmap[1] > 0) {
        const LinearArgs a = outconv_args(e, rows_of(d_win + B, nullptr, nullptr, 1), act_x, st->probs, R, softmax);
        LAUNCH_OK(ppg::launch_linear(prec, EPI_OUTCONV, 3, 1, a, 1, s), "stream out-conv+softmax");
    }
    HIP_OK(hipEventRecord(st->uploaded[slot_index], s));
    st->received.swap(received); st->x_valid.swap(x_valid); st->o_valid.swap(o_valid); st->finished.swap(finished);
    return PPG_OK;
}

int ppg_stream_push(PpgStream* st, const void* chunk, int n, int flush, int softmax,
                    int* first_final, int* num_final, void* stream_) {
    if (!st || st->batch != 1) return fail(PPG_EINVAL, "ppg_stream_push is the one-utterance form (use ppg_stream_push_batch)");
    if (n < 0 || (n > 0 && !chunk)) return fail(PPG_EINVAL, "bad argument");
    if (st->finished[0]) return fail(PPG_EINVAL, "the stream was flushed");
    return ppg_stream_push_batch(st, chunk, n, &n, &flush, softmax, first_final, num_final, stream_);
}

}  // extern "C"
