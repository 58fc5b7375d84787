// Host side of the spectral frontend (ppg_frontend.hip): the tables of a device (Hann window, twiddles, the banded mel
// filterbank image and its step program), ppg_frontend, the incremental ppg_frontend_stream_*, the profiling getters.
#include "ppg_pack.h"

using namespace ppg;

namespace {

struct Frontend {
    bool ready = false;
    ppg::FrontendTables tb{};
    std::vector<void*> allocs;
    bool profiling = false;
    std::vector<EventPair> events;
    size_t events_used = 0;
};
std::mutex g_front_mu;
std::map<int, Frontend> g_front;

double slaney_hz_to_mel(double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp;
    const double logstep = log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp;
}
double slaney_mel_to_hz(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp;
    const double logstep = log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : f_sp * m;
}

// Slaney-scale, area-normalised triangular filterbank, the algorithm of
// librosa.filters.mel(sr=16000, n_fft=1024, n_mels=80) called at reference
// ppgs/preprocess/mel.py:61-64; float64 arithmetic, cast to float32.
void mel_filterbank(std::vector<float>* dense) {
    const int n_mels = 80, n_bins = 513;
    const double sr = 16000.0;
    std::vector<double> mel_f(n_mels + 2);
    const double lo = slaney_hz_to_mel(0.0), hi = slaney_hz_to_mel(sr / 2);
    for (int i = 0; i < n_mels + 2; ++i) mel_f[i] = slaney_mel_to_hz(lo + (hi - lo) * i / (n_mels + 1));
    dense->assign((size_t)n_mels * n_bins, 0.f);
    for (int i = 0; i < n_mels; ++i) {
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        for (int k = 0; k < n_bins; ++k) {
            const double f = k * sr / 1024.0;
            const double lower = (f - mel_f[i]) / (mel_f[i + 1] - mel_f[i]);
            const double upper = (mel_f[i + 2] - f) / (mel_f[i + 2] - mel_f[i + 1]);
            const double v = std::max(0.0, std::min(lower, upper)) * enorm;
            (*dense)[(size_t)i * n_bins + k] = (float)v;
        }
    }
}

int frontend_for(int device, Frontend** out) {
    std::lock_guard<std::mutex> lock(g_front_mu);
    Frontend& f = g_front[device];
    if (!f.ready) {
        HIP_OK(hipSetDevice(device));
        std::vector<float> hann(1024);
        for (int n = 0; n < 1024; ++n) hann[n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * n / 1024.0));
        std::vector<float2> tw(1024);
        for (int j = 0; j < 1024; ++j) {
            const double ang = -2.0 * M_PI * j / 1024.0;
            tw[j] = make_float2((float)cos(ang), (float)sin(ang));
        }
        std::vector<float> dense;
        mel_filterbank(&dense);
        // Banded filterbank image (ppg_launch.h, FrontendTables): per block of 16 filters the 32-bin
        // steps from the block's first non-zero bin (rounded down to 32) to its last.
        struct Block { int index, first, steps; };
        std::vector<Block> blocks;
        for (int mb = 0; mb < 5; ++mb) {
            int first = 513, last = -1;
            for (int m = 16 * mb; m < 16 * mb + 16; ++m)
                for (int k = 0; k < 513; ++k)
                    if (dense[(size_t)m * 513 + k] != 0.f) { first = std::min(first, k); last = std::max(last, k); }
            if (last < 0) { first = 0; last = 0; }
            first &= ~31;
            blocks.push_back({mb, first, (last - first) / 32 + 1});
        }
        // A wave runs kMelSteps steps in two segments (kMelSegment + the rest) and can finish a block only at
        // the end of a segment: longest block first, a block longer than the first segment takes a whole
        // wave, the others the smallest free segment they fit (of the wave with the fewest steps so far).
        std::stable_sort(blocks.begin(), blocks.end(), [](const Block& a, const Block& b) { return a.steps > b.steps; });
        std::vector<uint16_t> img;
        auto add_fragments = [&](int mb, int first) {          // -> index of the high fragment
            const int frag = (int)(img.size() / 512);
            img.resize(img.size() + 1024, 0);
            for (int lane = 0; lane < 64 && mb >= 0; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int m = 16 * mb + (lane & 15), k = first + 8 * (lane >> 4) + j;
                    const float w = k < 513 ? dense[(size_t)m * 513 + k] * 65536.0f : 0.f;
                    split_f16(w, &img[(size_t)frag * 512 + lane * 8 + j], &img[(size_t)(frag + 1) * 512 + lane * 8 + j]);
                }
            return frag;
        };
        const int zero_frag = add_fragments(-1, 0);
        const int NS = ppg::kMelSteps, seg_first[2] = {0, ppg::kMelSegment}, seg_size[2] = {ppg::kMelSegment, NS - ppg::kMelSegment};
        std::vector<int> prog(4 * NS * 4, 0);
        for (int i = 0; i < 4 * NS; ++i) { prog[i * 4] = zero_frag; prog[i * 4 + 2] = -1; }
        int used[4] = {0, 0, 0, 0};
        bool taken[4][2] = {};
        for (const Block& blk : blocks) {
            int wave = -1, seg = -1;
            for (int w = 0; w < 4; ++w) {
                if (blk.steps > seg_size[0]) {               // whole wave
                    if (!taken[w][0] && !taken[w][1] && blk.steps <= NS && wave < 0) { wave = w; seg = 2; }
                    continue;
                }
                for (int g = 0; g < 2; ++g) {
                    if (taken[w][g] || blk.steps > seg_size[g]) continue;
                    const bool better = wave < 0 || used[w] < used[wave] || (used[w] == used[wave] && w == wave && seg_size[g] < seg_size[seg]);
                    if (better) { wave = w; seg = g; }
                }
            }
            if (wave < 0 || blk.first + 32 * blk.steps > 544)
                return fail(PPG_EINVAL, "mel filter block %d: %d steps from bin %d do not fit the frontend's program", blk.index, blk.steps, blk.first);
            // the block's steps END at its segment's end (the steps before them stay zero fragments)
            const int last = seg == 2 ? NS - 1 : seg_first[seg] + seg_size[seg] - 1;
            for (int st = 0; st < blk.steps; ++st) {
                int* e = &prog[(wave * NS + last - (blk.steps - 1) + st) * 4];
                e[0] = add_fragments(blk.index, blk.first + 32 * st);
                e[1] = (blk.first + 32 * st) * 2;
            }
            prog[(wave * NS + last) * 4 + 2] = blk.index;
            if (seg == 2) taken[wave][0] = taken[wave][1] = true; else taken[wave][seg] = true;
            used[wave] += blk.steps;
        }
        auto up = [&](const void* src, size_t bytes, const void** dst) -> int {
            void* p = nullptr;
            HIP_OK(hipMalloc(&p, bytes));
            f.allocs.push_back(p);
            HIP_OK(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
            *dst = p;
            return PPG_OK;
        };
        int rc;
        if ((rc = up(hann.data(), hann.size() * 4, (const void**)&f.tb.hann))) return rc;
        if ((rc = up(tw.data(), tw.size() * 8, (const void**)&f.tb.twiddle))) return rc;
        if ((rc = up(img.data(), img.size() * 2, (const void**)&f.tb.mel_img))) return rc;
        if ((rc = up(prog.data(), prog.size() * 4, (const void**)&f.tb.mel_prog))) return rc;
        f.tb.dbg = nullptr;
#ifdef PPG_FE_TIMING
        if (getenv("PPGS_AMD_FE_TIMING")) {
            std::vector<unsigned long long> zeros(64, 0);
            if ((rc = up(zeros.data(), 512, (const void**)&f.tb.dbg))) return rc;
        }
#endif
        f.ready = true;
    }
    *out = &f;
    return PPG_OK;
}

}  // namespace

extern "C" {

int ppg_frontend(int device, const float* audio, int batch, int samples, void* spec, void* mel, void* stream) {
    if (!audio || (!spec && !mel)) return fail(PPG_EINVAL, "null argument");
    if (batch <= 0) return fail(PPG_EINVAL, "batch %d", batch);
    if (samples <= 432)
        return fail(PPG_EINVAL, "samples %d: reflect padding of 432 needs more than 432 samples", samples);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(PPG_EDEVICE, "no HIP device: the PPG frontend has no CPU path");
    Frontend* f = nullptr;
    int rc = frontend_for(device, &f);
    if (rc) return rc;
    HIP_OK(hipSetDevice(device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    EventPair ev{};
    bool on = false;
    if (f->profiling) {
        if (f->events_used == f->events.size()) {
            EventPair p;
            HIP_OK(hipEventCreateWithFlags(&p.a, kTimingEventFlags));
            HIP_OK(hipEventCreateWithFlags(&p.b, kTimingEventFlags));
            f->events.push_back(p);
        }
        ev = f->events[f->events_used++];
        on = hipEventRecord(ev.a, s) == hipSuccess;
    }
    if ((double)batch * 513.0 * (double)(samples / 160) >= 4294967296.0)
        return fail(PPG_EINVAL, "frontend: batch %d x 513 bins x %d frames does not fit the kernel's 32-bit output index", batch, samples / 160);
    hipError_t he = ppg::launch_frontend(f->tb, audio, batch, samples, spec, mel, s);
    if (on) (void)hipEventRecord(ev.b, s);
    if (f->tb.dbg) {
        static int dumps = 0;
        unsigned long long h[64];
        if (dumps++ < 2 && hipStreamSynchronize(s) == hipSuccess &&
            hipMemcpy(h, f->tb.dbg, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess) {
            for (int w = 0; w < 4; ++w) {
                fprintf(stderr, "frontend wave %d (group 2 of workgroup 0):", w);
                for (int k = 1; k < 7; ++k) fprintf(stderr, " [%d] %lld", k, (long long)(h[w * 16 + k] - h[w * 16]));
                fprintf(stderr, "\n");
            }
        }
    }
    if (he != hipSuccess) return fail(PPG_EDEVICE, "frontend: %s", hipGetErrorString(he));
    return PPG_OK;
}

// ----------------------------------------------------------------------------
// Incremental frontend: audio arrives in pieces, mel frames leave as they become computable
// ----------------------------------------------------------------------------
int64_t ppg_audio_stream_frames(int64_t received, int flushed) {
    if (received < 0) return -1;
    if (flushed) return received / 160;
    // frame t reads samples up to 160 t + 591; frames leave in the pairs (2 j, 2 j + 1) the transform forms
    const int64_t computable = received < 592 ? 0 : (received - 592) / 160 + 1;
    return computable & ~(int64_t)1;
}

struct PpgFrontendStream {
    int device = 0, batch = 0, max_push = 0, cap = 0;
    float* carry = nullptr;              // (batch, 2, cap): per item the current carry and the one the next push writes
    struct Item {
        int64_t received = 0, frontier = 0, base = 0;   // samples so far; frames emitted; sample index of carry[0]
        int cur = 0;
        bool flushed = false;
    };
    std::vector<Item> items;
    std::mutex mu;
};

namespace {
// first sample a recording with frame frontier f still needs: frame f starts at 160 f - 432
int64_t carry_base(int64_t frontier) { return std::max<int64_t>(160 * frontier - 432, 0); }
}  // namespace

int ppg_frontend_stream_create(int device, int batch, int max_push_samples, PpgFrontendStream** out) {
    if (!out || batch <= 0 || max_push_samples <= 0) return fail(PPG_EINVAL, "frontend stream: batch %d, max_push_samples %d", batch, max_push_samples);
    if (max_push_samples > (1 << 28)) return fail(PPG_EINVAL, "frontend stream: max_push_samples %d is too large", max_push_samples);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(PPG_EDEVICE, "no HIP device: the PPG frontend has no CPU path");
    Frontend* f = nullptr;
    const int rc = frontend_for(device, &f);
    if (rc) return rc;
    HIP_OK(hipSetDevice(device));
    std::unique_ptr<PpgFrontendStream> st(new PpgFrontendStream);
    st->device = device; st->batch = batch; st->max_push = max_push_samples;
    // before a push an item holds the samples from carry_base(frontier) on: fewer than 432 + 592 + 2 x 160 = 1344
    // (the next pair is not computable yet); a push appends its own
    st->cap = round_up(1344 + max_push_samples, 64);
    st->items.resize(batch);
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&st->carry), (size_t)batch * 2 * st->cap * sizeof(float)));
    *out = st.release();
    return PPG_OK;
}

void ppg_frontend_stream_destroy(PpgFrontendStream* st) {
    if (!st) return;
    if (st->carry) { (void)hipSetDevice(st->device); (void)hipFree(st->carry); }
    delete st;
}

int ppg_frontend_stream_batch(const PpgFrontendStream* st) { return st ? st->batch : fail(PPG_EINVAL, "null frontend stream"); }

int ppg_frontend_stream_state(const PpgFrontendStream* st, int64_t* received, int64_t* emitted) {
    if (!st) return fail(PPG_EINVAL, "null frontend stream");
    for (int b = 0; b < st->batch; ++b) {
        if (received) received[b] = st->items[b].received;
        if (emitted) emitted[b] = st->items[b].frontier;
    }
    return PPG_OK;
}

int ppg_frontend_stream_reset(PpgFrontendStream* st, int item) {
    if (!st || item < -1 || item >= st->batch) return fail(PPG_EINVAL, "frontend stream reset: item %d", item);
    std::lock_guard<std::mutex> lock(st->mu);
    for (int b = 0; b < st->batch; ++b) {
        if (item >= 0 && b != item) continue;
        const int cur = st->items[b].cur;             // (an earlier push may still be writing the other buffer: keep the roles)
        st->items[b] = PpgFrontendStream::Item{};
        st->items[b].cur = cur;
    }
    return PPG_OK;
}

int ppg_frontend_stream_push(PpgFrontendStream* st, const float* audio, int64_t audio_pitch, int n_max, const int* counts_host,
                             const int* flush_host, void* mel, int64_t mel_pitch, int k_max, int64_t* first_frame, int* num_frames,
                             void* stream) {
    if (!st || !counts_host || n_max < 0 || k_max < 0) return fail(PPG_EINVAL, "frontend stream push: bad argument");
    if (n_max > st->max_push) return fail(PPG_EINVAL, "frontend stream push: %d samples, the stream was created for pushes of <= %d", n_max, st->max_push);
    if (n_max > 0 && (!audio || audio_pitch < n_max)) return fail(PPG_EINVAL, "frontend stream push: audio %p with pitch %lld for %d samples", (const void*)audio, (long long)audio_pitch, n_max);
    std::lock_guard<std::mutex> lock(st->mu);
    // everything is checked before any item's state changes
    int most = 0;
    for (int b = 0; b < st->batch; ++b) {
        const PpgFrontendStream::Item& it = st->items[b];
        const int n = counts_host[b], fl = flush_host ? flush_host[b] : 0;
        if (n < 0 || n > n_max) return fail(PPG_EINVAL, "frontend stream push: counts[%d] = %d outside [0, %d]", b, n, n_max);
        if (n == 0 && !fl) continue;
        if (it.flushed) return fail(PPG_EINVAL, "frontend stream push: item %d was flushed (reset it for the next utterance)", b);
        if (fl && it.received + n <= 432)
            return fail(PPG_EINVAL, "frontend stream push: item %d ends after %lld samples: reflect padding of 432 needs more than 432 samples", b, (long long)(it.received + n));
        most = std::max<int64_t>(most, ppg_audio_stream_frames(it.received + n, fl) - it.frontier);
    }
    if (most > k_max) return fail(PPG_EINVAL, "frontend stream push: %d new frames, the output holds %d", most, k_max);
    if (most > 0 && (!mel || mel_pitch < most)) return fail(PPG_EINVAL, "frontend stream push: output %p with pitch %lld for %d frames", mel, (long long)mel_pitch, most);
    if ((double)st->batch * 80.0 * (double)std::max<int64_t>(mel_pitch, 1) >= 4294967296.0)
        return fail(PPG_EINVAL, "frontend stream push: batch %d x 80 x pitch %lld does not fit the kernel's 32-bit output index", st->batch, (long long)mel_pitch);
    Frontend* f = nullptr;
    int rc = frontend_for(st->device, &f);
    if (rc) return rc;
    HIP_OK(hipSetDevice(st->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int b0 = 0; b0 < st->batch; b0 += ppg::kFrontendStreamItems) {
        const int items = std::min(ppg::kFrontendStreamItems, st->batch - b0);
        ppg::FrontendStreamArgs a{};
        a.chunk = audio; a.chunk_pitch = (long)audio_pitch; a.carry = st->carry; a.cap = st->cap; a.item0 = b0;
        a.out_pitch = (int)mel_pitch;
        int frames_most = 0;
        bool any = false;
        for (int l = 0; l < items; ++l) {
            PpgFrontendStream::Item& it = st->items[b0 + l];
            const int n = counts_host[b0 + l], fl = flush_host ? flush_host[b0 + l] : 0;
            ppg::FrontendStreamItem& d = a.item[l];
            if (first_frame) first_frame[b0 + l] = it.frontier;
            if (num_frames) num_frames[b0 + l] = 0;
            if (n == 0 && !fl) continue;                       // (all zero: no frames, nothing carried, no sample read)
            const int64_t origin = 160 * it.frontier, total = it.received + n;
            const int64_t frontier = ppg_audio_stream_frames(total, fl);
            d.lo = (int)std::max<int64_t>(-origin, -(1 << 29));
            d.hi = (int)(total - origin);
            d.cbase = (int)(it.base - origin);
            d.split = (int)(it.received - origin);
            d.frames = (int)(frontier - it.frontier);
            d.keep = fl ? d.hi : (int)(carry_base(frontier) - origin);
            d.cur = it.cur;
            if (d.hi - d.keep > st->cap || d.split - d.cbase > st->cap || d.keep < d.cbase)
                return fail(PPG_EINVAL, "frontend stream push: item %d carry [%d, %d) of [%d, %d) does not fit %d samples (internal)", b0 + l, d.keep, d.hi, d.cbase, d.hi, st->cap);
            if (num_frames) num_frames[b0 + l] = d.frames;
            frames_most = std::max(frames_most, d.frames);
            any = true;
            it.received = total;
            it.frontier = frontier;
            it.flushed = fl != 0;
            if (!fl) { it.base = carry_base(frontier); it.cur ^= 1; }
        }
        if (!any) continue;
        a.groups_per_item = std::max(1, (frames_most + ppg::kFrontendFrames - 1) / ppg::kFrontendFrames);
        const hipError_t he = ppg::launch_frontend_stream(f->tb, a, items, mel, s);
        if (he != hipSuccess) return fail(PPG_EDEVICE, "frontend stream: %s", hipGetErrorString(he));
    }
    return PPG_OK;
}

int ppg_frontend_profile(int device, int enable) {
    Frontend* f = nullptr;
    int rc = frontend_for(device, &f);
    if (rc) return rc;
    f->profiling = enable != 0;
    f->events_used = 0;
    return PPG_OK;
}

int ppg_frontend_profile_read(int device, double* total_ms, int64_t* launches) {
    if (!total_ms || !launches) return fail(PPG_EINVAL, "null argument");
    Frontend* f = nullptr;
    int rc = frontend_for(device, &f);
    if (rc) return rc;
    *launches = (int64_t)f->events_used;
    return elapsed_total(f->events, f->events_used, total_ms);
}

}  // extern "C"
