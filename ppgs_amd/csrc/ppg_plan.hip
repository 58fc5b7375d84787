// Chunk planner (reference ppgs/model/transformer.py:49-64): the windows of a batch, their split into pipeline groups,
// the attention items of each group.  Pure host code: no HIP call, nothing here needs a device.
#include "ppg_host.h"

namespace ppg {

void split_groups(Plan* plan, int ngroups, int qtile, int xcd_heads, int narrow_tiles) {
    plan->groups.clear();
    const int total = plan->info.tokens;
    size_t w = 0;
    for (int gi = 0; gi < ngroups && w < plan->windows.size(); ++gi) {
        PlanGroup grp;
        const int base_tok = plan->windows[w].tok_off, base_vt = plan->windows[w].vt_off;
        const long long target = (long long)total * (gi + 1) / ngroups;
        while (w < plan->windows.size() &&
               (grp.windows.empty() || gi == ngroups - 1 || plan->windows[w].tok_off + round_up(plan->windows[w].frames, 16) / 2 < target)) {
            PpgWindow win = plan->windows[w++];
            win.tok_off -= base_tok;
            win.vt_off -= base_vt;
            const int wi = (int)grp.windows.size();
            for (int k = 0; k < round_up(win.frames, 16) / 16; ++k) grp.blk_win.push_back(wi);
            grp.tokens = win.tok_off + round_up(win.frames, 16);
            grp.vt_tokens = win.vt_off + round_up(win.frames, 32);
            grp.windows.push_back(win);
        }
        // Query tiles.  A window that fits half a tile, or whose keys are at most half the longest window's, gets
        // tiles of half the width (attn_mixed_kernel): the latter run last, on a chip the long items no longer
        // fill, and a wave's time is its queries x the window's keys.
        int longest = 0;
        for (const PpgWindow& win : grp.windows) longest = std::max(longest, win.valid);
        for (int wi = 0; wi < (int)grp.windows.size(); ++wi) {
            const PpgWindow& win = grp.windows[wi];
            const int narrow = narrow_tiles && (narrow_tiles == 2 || 2 * win.valid <= longest || win.frames <= qtile / 2);
            for (int q0 = 0; q0 < win.frames; q0 += narrow ? qtile / 2 : qtile)
                grp.items.push_back(AttnItem{wi, q0, win.tok_off, win.vt_off, win.frames, win.valid, narrow, 0});
        }
        // Launch order = item order: longest first (keys actually visited; the
        // causal flag only shortens early query tiles, which keeps this order a
        // good proxy).  Workgroups are handed to CU slots in order, so a long item
        // dispatched late would run alone at the end of the kernel (batch 32 x
        // 1000 frames: 500/500/250-frame windows in utterance order finish at 2.0
        // long-item times, sorted at 1.5).
        std::stable_sort(grp.items.begin(), grp.items.end(), [&](const AttnItem& x, const AttnItem& y) {
            return grp.windows[x.window].valid > grp.windows[y.window].valid;
        });
        // XCD affinity: workgroup b of the 1-D attention grid runs (item b / heads, head b % heads) and goes to
        // XCD b % 8, each XCD with its own L2.  Deal the windows (in sorted order) into S = 8 / gcd(8, heads)
        // lanes and interleave the lanes, so that all query tiles of one (window, head) -- which stream the same
        // K and V^T rows -- sit S items apart and land on one XCD instead of four.
        if (xcd_heads > 0) {
            int g = xcd_heads; for (int b = 8; b; ) { const int t = g % b; g = b; b = t; }   // gcd(heads, 8)
            const int S = 8 / g;
            if (S > 1) {
                std::vector<std::vector<AttnItem>> lane(S);
                int rank = -1, last = -1;
                for (const AttnItem& it : grp.items) {
                    if (it.window != last) { ++rank; last = it.window; }
                    lane[rank % S].push_back(it);
                }
                std::vector<size_t> at(S, 0);
                size_t out = 0;
                while (out < grp.items.size())
                    for (int j = 0; j < S; ++j)
                        if (at[j] < lane[j].size()) grp.items[out++] = lane[j][at[j]++];
            }
        }
        plan->groups.push_back(std::move(grp));
    }
}

int build_plan(int chunk, int overlap, int max_positions, int batch, int frames,
               const int64_t* lengths, int legacy, int qtile, Plan* plan) {
    if (batch <= 0 || frames <= 0 || !lengths) return fail(PPG_EINVAL, "empty batch (batch=%d frames=%d)", batch, frames);
    for (int b = 0; b < batch; ++b)
        if (lengths[b] < 0 || lengths[b] > frames)
            return fail(PPG_EINVAL, "lengths[%d]=%lld outside [0, %d]", b, (long long)lengths[b], frames);
    if (legacy && frames >= max_positions)
        return fail(PPG_ELENGTH, "legacy_mode needs frames < %d, got %d", max_positions, frames);
    const int stride = chunk - 2 * overlap;
    const bool chunked = !legacy && frames > chunk;
    const int nchunks = chunked ? (frames + stride - 1) / stride : 1;
    int tok = 0, vt = 0;
    for (int b = 0; b < batch; ++b) {
        int64_t rem = lengths[b];
        for (int i = 0; i < nchunks; ++i) {
            PpgWindow w{};
            w.item = b;
            w.chunked = chunked ? 1 : 0;
            if (chunked) {
                w.start = i * stride;
                const int stop = std::min(w.start + chunk, frames + overlap);
                w.frames = stop - w.start;
                int64_t cl = std::min<int64_t>(std::max<int64_t>(rem + overlap, 0), chunk);
                if (cl == overlap) cl = 0;
                rem = std::max<int64_t>(rem - stride, 0);
                w.valid = (int)cl;
                w.keep_lo = overlap;
                w.keep_hi = std::min(chunk - overlap, w.frames);
                w.out_frame = i * stride;
            } else {
                w.start = 0;
                w.frames = frames;
                w.valid = (int)lengths[b];
                w.keep_lo = 0;
                w.keep_hi = frames;
                w.out_frame = 0;
            }
            // The reference broadcasts a (B, max(valid)) mask against (B, C, Tc):
            // positions >= valid are masked, valid never exceeds the window.
            w.valid = std::min(w.valid, w.frames);
            if (w.valid > 0) {
                w.tok_off = tok;
                w.vt_off = vt;
                tok += round_up(w.frames, 16);
                vt += round_up(w.frames, 32);
                plan->info.processed_frames += w.frames;
                plan->info.attention_pairs += (int64_t)w.frames * w.frames;
                plan->windows.push_back(w);
            } else {
                w.tok_off = -1;
                w.vt_off = -1;
                plan->info.skipped_windows++;
            }
            plan->all.push_back(w);
        }
    }
    plan->info.num_windows = (int)plan->windows.size();
    plan->info.tokens = tok;
    plan->info.vt_tokens = vt;
    return PPG_OK;
}

}  // namespace ppg
