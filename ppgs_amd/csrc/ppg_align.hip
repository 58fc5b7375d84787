// Forced alignment of a PPG to a phoneme sequence with goodness-of-pronunciation scores, and the free-running
// run-length decode, on the device.  Phrase search (ppg_search) stands at the end, and after
// it the same search carried across the pushes of a stream (ppg_search_stream_*), then the phoneme
// recogniser, the best path through all 40 phonemes under a transition model (ppg_recognize), and last
// that recogniser carried across the pushes of a stream (ppg_recognize_stream_*).  The best path through a
// graph of phoneme states (ppg_viterbi) follows the live recogniser.  The phrase search over such a graph
// (ppg_search_graph) stands at the very end of the file, behind the host entries of all the others, and
// behind it that search carried across the pushes of a stream (ppg_search_graph_stream_*): the two share
// one body, `search_graph_frames`, and their host entries close the file.
//
//   e[t, n] = logf(min(max(P[s[n], t], 1e-8), 1 - 1e-8))                      (the clamp of ppg_distance)
//   D[0, 0] = e[0, 0];  D[0, n > 0] = -inf
//   D[t, n] = e[t, n] + max(D[t-1, n], D[t-1, n-1])                            (fp32, added in order of t)
//   the path advances (takes n-1) only if D[t-1, n-1] > D[t-1, n]; a tie stays.  Comparisons only.
//   total = D[T-1, N-1]; the trace-back starts at (T-1, N-1).
//
// Five kernels (and three for optional phonemes, below), all on the caller's stream, no allocation, no synchronisation:
//   align_prepare    one thread per frame: the 40 clamped log-posteriors and their maximum, frame-major (176 B per
//                    frame).  ONE piece of code for every consumer, so a frame always gives the same bits.
//   align_programme  one wave per utterance.  Lane l keeps a strip of S consecutive states (their phoneme and
//                    D[., n]) in registers, S = 1, 4 or 16 by the utterance's own N, and takes the state below its
//                    strip from lane l - 1 by a cross-lane move.  Time is the serial loop; there is no skew, every
//                    state of frame t needs frame t-1 only.  Emissions are a gather from a chunk of prepared frames
//                    in LDS; the next chunk is in flight while the current one is consumed.  One direction bit per
//                    cell: a 16-bit word per lane and frame.
//   align_traceback  one wave per utterance: direction rows come through LDS 64 frames at a time, the walk itself is
//                    wave-uniform.
//   align_score      one thread per (utterance, phoneme): its segment summed in frame order.
//   decode_runs      one wave per utterance: per-frame argmax (lowest index on ties), run boundaries compacted with
//                    ballot and a popcount prefix.
//
// Optional phonemes (ppg_align_optional): opt[n] != 0 lets the path jump over phoneme n.
//   D[t, n] = e[t, n] + best of  stay D[t-1, n],  advance D[t-1, n-1],  skip D[t-1, n-2] if opt[n-1]
//   strict comparisons in that order: stay beats advance beats skip on ties.  State -1 holds 0 before frame 0.
//   The end is state N-1, or N-2 if opt[N-1] and D[T-1, N-2] > D[T-1, N-1].
// align_prepare is shared; three kernels beside the ones above:
//   align_programme_optional   the same wave, strips and staging; a second value from below the strip (a second
//                              cross-lane move), the states' skip permissions as a bit mask in one register, and two
//                              direction planes (advance, skip) of the 16-bit-per-lane format.
//   align_traceback_optional   both planes through LDS 64 frames at a time; a skip writes two starts.
//   align_score_optional       align_score for transcripts that may be longer than the utterance.
//
// What the kernels share stands once: WALK_FRAMES is the frame loop (staging, double buffering, the gather one frame
// ahead, the barriers) of the five programmes, each of which hands it its recurrence.  `search_strips` is
// the one body of both searches, `recognize_frames` of both recognisers, `traceback` of both trace-backs (one or two
// bit planes), `score_phoneme` of both
// scores, `refused` their test of an utterance the programme refused, `symbols_fine` the phoneme range check,
// `open_runs` the run compression of decode_runs and recognize_runs.  The __global__ entries keep their names and are
// thin where a body is shared.  The host entries share their rungs (check_*, select_device, launched) at the end of
// the file.
#include "../../include/ppgs_amd.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <initializer_list>

namespace ppg {
int fail_message(int code, const char* fmt, ...);
}

namespace {

constexpr int NP = 40;                        // phonemes
constexpr int PREP = 44;                      // floats per prepared frame: 40 log-posteriors, their maximum, 3 zeros
constexpr int PREP_VEC = PREP / 4;            // ... as 16-byte pieces
constexpr int CHUNK = 32;                     // frames staged in LDS at a time
constexpr int CHUNK_VEC = CHUNK * PREP_VEC;   // 352 pieces = 5.5 KiB
constexpr int FETCH = (CHUNK_VEC + 63) / 64;  // pieces per lane and chunk
constexpr int ROW = 64;                       // direction words (16 bit) per frame: one per lane
constexpr int ROW_VEC = ROW * 2 / 16;         // a direction row as 16-byte pieces
constexpr int WALK = 64;                      // frames per LDS refill of the trace-back

struct Layout {
    size_t logp, dirs, skips, ends, bytes;    // byte offsets into the workspace; with optional phonemes also the skip
};                                            // plane and the end state of every utterance

inline size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

// the prepared frames of a call: the first block of every workspace, and the whole workspace of a stream's push
inline size_t prepared_bytes(int items, int frames) { return align256((size_t)items * frames * PREP * sizeof(float)); }

inline Layout layout(int items, int frames, bool optional) {
    Layout w{};
    const size_t plane = (size_t)items * frames * ROW * sizeof(uint16_t);
    size_t at = 0;
    w.logp = at; at += prepared_bytes(items, frames);
    w.dirs = at; at = align256(at + plane);
    if (optional) {
        w.skips = at; at = align256(at + plane);
        w.ends = at; at = align256(at + (size_t)items * sizeof(int));
    }
    w.bytes = at;
    return w;
}

// strip length of an utterance with n phonemes: 64 lanes x S states cover it
__host__ __device__ inline int strip_shift(int n) { return n <= 64 ? 0 : n <= 256 ? 2 : 4; }

// the lengths an utterance may have; everything else yields total = NaN and touches nothing
__device__ __forceinline__ bool plausible(int t, int n, int frames, int max_phonemes) {
    return t >= 1 && t <= frames && n >= 1 && n <= max_phonemes && n <= t;
}

// grid (ceil(frames / 64), items), 64 threads: thread = frame.  src (items, 40, frames); only t < lengths[item] is read
__global__ __launch_bounds__(64) void align_prepare(const float* __restrict__ ppg, int frames,
                                                     const int* __restrict__ lengths, float* __restrict__ logp)
{
    const int item = blockIdx.y;
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= frames || t >= lengths[item]) return;
    const float* src = ppg + (size_t)item * NP * frames + t;
    float4* dst = reinterpret_cast<float4*>(logp + ((size_t)item * frames + t) * PREP);
    float v[PREP];
    float top = -INFINITY;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        v[p] = logf(fminf(fmaxf(src[(size_t)p * frames], 1e-8f), 1.f - 1e-8f));
        top = fmaxf(top, v[p]);
    }
    v[NP] = top;
    v[NP + 1] = v[NP + 2] = v[NP + 3] = 0.f;
#pragma unroll
    for (int q = 0; q < PREP_VEC; ++q) dst[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

// lane l <- lane l - 1; lane 0 <- first.  Call it from wave-uniform control flow only.
__device__ __forceinline__ int lane_up(int v, int first) {
    return __builtin_amdgcn_update_dpp(first, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ float lane_up(float v, float first) {
    return __int_as_float(lane_up(__float_as_int(v), __float_as_int(first)));
}

// the phoneme range check: whether `symbol` is none of the 40
__device__ __forceinline__ bool bad_symbol(int symbol) { return (unsigned)symbol >= (unsigned)NP; }

// whether every phoneme of sym[0 .. N-1] is one of the 40: the same answer in every lane (call it uniformly)
__device__ __forceinline__ bool symbols_fine(const int* __restrict__ sym, int N, int lane) {
    bool bad = false;
    for (int n = lane; n < N; n += 64) bad |= bad_symbol(sym[n]);
    return !__any(bad);
}

// the prepared frames t0 .. t0 + CHUNK - 1 of one utterance, those below T only, one 16-byte piece per lane and u
__device__ __forceinline__ void fetch(const float4* __restrict__ src, int t0, int T, int lane, float4 (&piece)[FETCH]) {
    const int pieces = min(CHUNK, T - t0) * PREP_VEC;          // <= 0 past the end: nothing is read
#pragma unroll
    for (int u = 0; u < FETCH; ++u) {
        const int idx = u * 64 + lane;
        piece[u] = idx < pieces ? src[(size_t)t0 * PREP_VEC + idx] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

__device__ __forceinline__ void stash(float4* __restrict__ stage, int lane, const float4 (&piece)[FETCH]) {
#pragma unroll
    for (int u = 0; u < FETCH; ++u) {
        const int idx = u * 64 + lane;
        if (idx < CHUNK_VEC) stage[idx] = piece[u];
    }
}

// The frame walk of every programme below, once: BODY runs once per frame `t` = 0 .. T-1 in order with `cur`, the
// emissions of the lane's strip (RELATIVE: less the frame's maximum, float NP of the frame: a broadcast).  The prepared
// frames come through LDS CHUNK at a time, double-buffered: the next chunk's loads are in flight while the current one
// is consumed, and the gather itself runs one frame ahead of its use.  It reads `src`, `T`, `s`, `stage` and `lane` of
// the programme it stands in, holds the barriers, so it stands in wave-uniform control flow only; BODY may diverge.
// A macro and not a function taking BODY as a lambda: as a function the same statements built to other schedules and
// other places in the instruction stream (align_programme 6 %, search_programme 7 - 9 % slower, the programme with
// optional phonemes 144 VGPRs for 119), as a macro the compiler sees the written-out loop.
#define WALK_FRAMES(S, RELATIVE, t, cur, ...)                                                                          \
    {                                                                                                                  \
        float4 next[FETCH];                                                                                            \
        fetch(src, 0, T, lane, next);                                                                                  \
        stash(stage[0], lane, next);                                                                                   \
        __syncthreads();                                                                                               \
        int buf = 0;                                                                                                   \
        for (int t0 = 0; t0 < T; t0 += CHUNK, buf ^= 1) {                                                              \
            fetch(src, t0 + CHUNK, T, lane, next);             /* in flight while this chunk is consumed */            \
            const float* e = reinterpret_cast<const float*>(stage[buf]);                                               \
            const int count = min(CHUNK, T - t0);                                                                      \
            float cur[S];                                      /* frame t's, read one frame ahead of their use */      \
            {                                                                                                          \
                const float top = RELATIVE ? e[NP] : 0.f;                                                              \
                _Pragma("unroll") for (int k = 0; k < S; ++k) cur[k] = RELATIVE ? e[s[k]] - top : e[s[k]];             \
            }                                                                                                          \
            for (int u = 0; u < count; ++u) {                                                                          \
                const int t = t0 + u;                                                                                  \
                const float* ahead = e + min(u + 1, CHUNK - 1) * PREP;   /* (the last one re-reads a row: unused) */   \
                const float top = RELATIVE ? ahead[NP] : 0.f;                                                          \
                float coming[S];                                                                                       \
                _Pragma("unroll") for (int k = 0; k < S; ++k) coming[k] = RELATIVE ? ahead[s[k]] - top : ahead[s[k]];  \
                __VA_ARGS__                                                                                            \
                _Pragma("unroll") for (int k = 0; k < S; ++k) cur[k] = coming[k];                                      \
            }                                                                                                          \
            stash(stage[buf ^ 1], lane, next);                 /* its readers passed the barrier below */              \
            __syncthreads();                                                                                           \
        }                                                                                                              \
    }

// The programme of one utterance with S states per lane.  Everything here is wave-uniform control flow.
template <int S>
__device__ __forceinline__ float programme(const float4* __restrict__ src, int T, int N, const int* __restrict__ sym,
                                           uint16_t* __restrict__ dirs, float4 (&stage)[2][CHUNK_VEC], int lane)
{
    int s[S]; float d[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const int n = lane * S + k;
        s[k] = n < N ? sym[n] : 0;                             // states at or above N run along on phoneme 0, unread
        d[k] = -INFINITY;
    }
    WALK_FRAMES(S, false, t, cur,
        // the state below the strip; for the very first cell the virtual origin D[-1, -1] = 0, so D[0, 0] = e + 0
        const float below = lane_up(d[S - 1], t == 0 ? 0.f : -INFINITY);
        uint32_t bits = 0;
        _Pragma("unroll") for (int k = S - 1; k >= 0; --k) {   // downwards: d[k - 1] is still frame t-1's
            const float stay = d[k], from = k ? d[k - 1] : below;
            const bool advance = from > stay;
            d[k] = cur[k] + (advance ? from : stay);           // -inf + finite = -inf: never NaN
            bits |= (uint32_t)advance << k;
        }
        dirs[(size_t)t * ROW + lane] = (uint16_t)bits;)
    const int k = (N - 1) % S;
    float last = d[0];
#pragma unroll
    for (int q = 1; q < S; ++q) last = k == q ? d[q] : last;
    return last;                                               // meaningful in lane (N - 1) / S
}

// grid (items), 64 threads
__global__ __launch_bounds__(64) void align_programme(const float* __restrict__ logp, int frames,
                                                       const int* __restrict__ lengths,
                                                       const int* __restrict__ phonemes, int max_phonemes,
                                                       const int* __restrict__ phoneme_lengths,
                                                       uint16_t* __restrict__ dirs, float* __restrict__ total)
{
    __shared__ float4 stage[2][CHUNK_VEC];
    const int item = blockIdx.x, lane = threadIdx.x;
    const int T = lengths[item], N = phoneme_lengths[item];
    const int* sym = phonemes + (size_t)item * max_phonemes;
    bool fine = plausible(T, N, frames, max_phonemes);
    if (fine) fine = symbols_fine(sym, N, lane);
    if (!fine) {                                               // (uniform)
        if (lane == 0) total[item] = NAN;
        return;
    }
    const float4* src = reinterpret_cast<const float4*>(logp + (size_t)item * frames * PREP);
    uint16_t* out = dirs + (size_t)item * frames * ROW;
    const int shift = strip_shift(N);
    float last;
    if (shift == 0) last = programme<1>(src, T, N, sym, out, stage, lane);
    else if (shift == 2) last = programme<4>(src, T, N, sym, out, stage, lane);
    else last = programme<16>(src, T, N, sym, out, stage, lane);
    if (lane == (N - 1) >> shift) total[item] = last;
}

// What the kernels after a programme ask first: an utterance whose total is NaN was refused by it and stays untouched.
// The plain alignment repeats the programme's test of the lengths; with optional phonemes (N may exceed T) that NaN
// alone says it, so the lengths of a refused utterance are loaded and never used.
template <bool Optional>
__device__ __forceinline__ bool refused(int T, int N, int frames, int max_phonemes, const float* __restrict__ total) {
    return (!Optional && !plausible(T, N, frames, max_phonemes)) || *total != *total;
}

// The trace-back of one utterance over PLANES bit planes of directions: the advance plane and, with Skips, the skip
// plane, whose set bit overrides it; the walk begins in state `end`.  Wave-uniform control flow.
template <bool Skips, int PLANES>
__device__ __forceinline__ void traceback(const uint4* const (&src)[PLANES], int T, int N, int end,
                                          int* __restrict__ out, uint4 (&rows)[PLANES][WALK * ROW_VEC], int lane)
{
    static_assert(PLANES == (Skips ? 2 : 1), "one plane, or two with skips");
    const int shift = strip_shift(N), mask = (1 << shift) - 1;
    uint4 next[PLANES][ROW_VEC];
    auto load = [&](int c) {                                   // rows of frames c * WALK ..., those below T only
        const int pieces = min(WALK, T - c * WALK) * ROW_VEC;
#pragma unroll
        for (int u = 0; u < ROW_VEC; ++u) {
            const int idx = u * 64 + lane;
#pragma unroll
            for (int p = 0; p < PLANES; ++p)
                next[p][u] = idx < pieces ? src[p][(size_t)c * WALK * ROW_VEC + idx] : make_uint4(0, 0, 0, 0);
        }
    };
    int n = end;
    int c = (T - 1) / WALK;
    load(c);
    for (; c >= 0; --c) {
        __syncthreads();                                       // the walk over the previous refill is over
#pragma unroll
        for (int u = 0; u < ROW_VEC; ++u) {
#pragma unroll
            for (int p = 0; p < PLANES; ++p) rows[p][u * 64 + lane] = next[p][u];
        }
        __syncthreads();
        if (c > 0) load(c - 1);
        const uint16_t* row = reinterpret_cast<const uint16_t*>(rows[0]);
        const uint16_t* row_skips = reinterpret_cast<const uint16_t*>(rows[PLANES - 1]);
        const int low = max(c * WALK, 1);
        for (int t = min(T - 1, c * WALK + WALK - 1); t >= low; --t) {
            const int at = (t & (WALK - 1)) * ROW + (n >> shift), bit = n & mask;  // the same address in every lane
            const uint32_t word = row[at], jump = Skips ? row_skips[at] : 0;
            if (Skips && n > 1 && ((jump >> bit) & 1)) {       // over the optional phoneme n - 1: it gets no frame
                if (lane == 0) { out[n] = t; out[n - 1] = t; }
                n -= 2;
            } else if (n > 0 && ((word >> bit) & 1)) {
                if (lane == 0) out[n] = t;
                --n;
            }
        }
    }
    if (lane == 0) {
        if (Skips && n == 1) out[1] = 0;                       // the path began in state 1: phoneme 0 was left out
        out[0] = 0;
        if (Skips && end == N - 2) out[N - 1] = T;             // ... ended in state N - 2: phoneme N - 1 was left out
        out[N] = T;
    }
}

// grid (items), 64 threads
__global__ __launch_bounds__(64) void align_traceback(const uint16_t* __restrict__ dirs, int frames,
                                                       const int* __restrict__ lengths, int max_phonemes,
                                                       const int* __restrict__ phoneme_lengths,
                                                       const float* __restrict__ total, int* __restrict__ starts)
{
    __shared__ uint4 rows[1][WALK * ROW_VEC];
    const int item = blockIdx.x;
    const int T = lengths[item], N = phoneme_lengths[item];
    if (refused<false>(T, N, frames, max_phonemes, total + item)) return;
    const uint4* const src[1] = {reinterpret_cast<const uint4*>(dirs + (size_t)item * frames * ROW)};
    traceback<false>(src, T, N, N - 1, starts + (size_t)item * (max_phonemes + 1), rows, threadIdx.x);
}

// The scores of one phoneme, thread = phoneme of grid (ceil(max_phonemes / 64), items), 64 threads.  Optional: the
// transcript may be longer than its utterance, and a phoneme that was left out has an empty segment: 0 / 0 = NaN.
template <bool Optional>
__device__ __forceinline__ void score_phoneme(const float* __restrict__ logp, int frames,
                                              const int* __restrict__ lengths, const int* __restrict__ phonemes,
                                              int max_phonemes, const int* __restrict__ phoneme_lengths,
                                              const float* __restrict__ total, const int* __restrict__ starts,
                                              float* __restrict__ score, float* __restrict__ gop)
{
    const int item = blockIdx.y, n = blockIdx.x * 64 + threadIdx.x;
    const int T = lengths[item], N = phoneme_lengths[item];
    if (refused<Optional>(T, N, frames, max_phonemes, total + item) || n >= N) return;
    const int* bounds = starts + (size_t)item * (max_phonemes + 1) + n;
    const int first = max(bounds[0], 0), end = min(bounds[1], T);
    const float* row = logp + (size_t)item * frames * PREP + phonemes[(size_t)item * max_phonemes + n];
    const float* top = logp + (size_t)item * frames * PREP + NP;
    float sum = 0.f, below = 0.f;
    for (int t = first; t < end; ++t) {
        const float e = row[(size_t)t * PREP];
        sum += e;
        if (gop) below += e - top[(size_t)t * PREP];           // exactly 0 where the target is the frame's maximum
    }
    const float count = (float)(end - first);
    score[(size_t)item * max_phonemes + n] = sum / count;
    if (gop) gop[(size_t)item * max_phonemes + n] = below / count;
}

// grid (ceil(max_phonemes / 64), items), 64 threads
__global__ __launch_bounds__(64) void align_score(const float* __restrict__ logp, int frames,
                                                   const int* __restrict__ lengths,
                                                   const int* __restrict__ phonemes, int max_phonemes,
                                                   const int* __restrict__ phoneme_lengths,
                                                   const float* __restrict__ total, const int* __restrict__ starts,
                                                   float* __restrict__ score, float* __restrict__ gop)
{
    score_phoneme<false>(logp, frames, lengths, phonemes, max_phonemes, phoneme_lengths, total, starts, score, gop);
}

// Run compression of 64 frames' labels, lane = frame `t` of them (label -2 at or past T): a frame whose label differs
// from the frame before it opens a run; the runs' places come from a ballot and a popcount prefix.  `carry` is the
// label before these frames (-1 before frame 0), `base` the runs so far.  Wave-uniform control flow.
__device__ __forceinline__ void open_runs(int label, int t, int T, int lane, int& carry, int& base,
                                          int* out_phonemes, int* out_starts) {
    const int before = lane_up(label, carry);
    const bool opens = t < T && label != before;
    const unsigned long long mask = __ballot(opens);
    if (opens) {
        const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
        out_phonemes[at] = label;
        out_starts[at] = t;
    }
    base += __popcll(mask);
    carry = __builtin_amdgcn_readlane(label, 63);
}

// grid (items), 64 threads: lane = frame of the current 64
__global__ __launch_bounds__(64) void decode_runs(const float* __restrict__ ppg, int frames,
                                                   const int* __restrict__ lengths, int* __restrict__ phonemes,
                                                   int* __restrict__ starts, int* __restrict__ runs)
{
    const int item = blockIdx.x, lane = threadIdx.x;
    const int T = lengths[item];
    if (T < 1 || T > frames) {                                 // (uniform)
        if (lane == 0) runs[item] = 0;
        return;
    }
    const float* src = ppg + (size_t)item * NP * frames;
    int* out_phonemes = phonemes + (size_t)item * frames;
    int* out_starts = starts + (size_t)item * (frames + 1);
    int carry = -1, base = 0;                                  // the label before this chunk; runs so far
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        int label = -2;
        if (t < T) {
            float best = src[t];
            label = 0;
#pragma unroll 8
            for (int p = 1; p < NP; ++p) {
                const float v = src[(size_t)p * frames + t];
                if (v > best) { best = v; label = p; }         // the lowest index on ties
            }
        }
        open_runs(label, t, T, lane, carry, base, out_phonemes, out_starts);
    }
    if (lane == 0) { runs[item] = base; out_starts[base] = T; }
}

// ---- optional phonemes ----

// The programme with optional phonemes of one utterance with S states per lane: `programme` with a third predecessor.
// Returns the end state; *total is D there.  Everything here is wave-uniform control flow.
template <int S>
__device__ __forceinline__ int programme_optional(const float4* __restrict__ src, int T, int N,
                                                  const int* __restrict__ sym, const int* __restrict__ opt,
                                                  uint16_t* __restrict__ dirs, uint16_t* __restrict__ skips,
                                                  float4 (&stage)[2][CHUNK_VEC], int lane, float* total)
{
    int s[S]; float d[S];
    uint32_t may = 0;                                          // bit k: the state below state k of the strip is optional
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const int n = lane * S + k;
        s[k] = n < N ? sym[n] : 0;                             // states at or above N run along on phoneme 0, unread
        may |= (uint32_t)(n >= 1 && n < N && opt[n - 1] != 0) << k;
        d[k] = -INFINITY;
    }
    WALK_FRAMES(S, false, t, cur,
        // the two states below the strip.  The virtual origin, state -1, holds 0 before frame 0 and -inf after it:
        // it is `below` of state 0 and, where phoneme 0 is optional, `under` of state 1.
        const float below = lane_up(d[S - 1], t == 0 ? 0.f : -INFINITY);
        const float under = S == 1 ? lane_up(below, -INFINITY) : lane_up(d[S > 1 ? S - 2 : 0], -INFINITY);
        uint32_t bits = 0; uint32_t jumps = 0;
        _Pragma("unroll") for (int k = S - 1; k >= 0; --k) {   // downwards: d[k - 1] and d[k - 2] are still frame t-1's
            const float stay = d[k]; const float from = k ? d[k - 1] : below;
            const float over = k >= 2 ? d[k >= 2 ? k - 2 : 0] : k == 1 ? below : under;
            const bool advance = from > stay;
            const float best = advance ? from : stay;
            const bool skip = ((may >> k) & 1) && over > best;
            d[k] = cur[k] + (skip ? over : best);              // -inf + finite = -inf: never NaN
            bits |= (uint32_t)advance << k;                    // (a set skip bit overrides it in the trace-back)
            jumps |= (uint32_t)skip << k;
        }
        dirs[(size_t)t * ROW + lane] = (uint16_t)bits;
        skips[(size_t)t * ROW + lane] = (uint16_t)jumps;)
    const int k = (N - 1) % S, j = (N + S - 2) % S;            // the last state's place in its strip; the one below it
    float last = d[0], before = d[0];
#pragma unroll
    for (int q = 1; q < S; ++q) {
        last = k == q ? d[q] : last;
        before = j == q ? d[q] : before;
    }
    last = __shfl(last, (N - 1) / S);
    before = __shfl(before, max(N - 2, 0) / S);
    const bool shorter = N >= 2 && opt[N - 1] != 0 && before > last;       // (uniform) the last phoneme is left out
    *total = shorter ? before : last;
    return shorter ? N - 2 : N - 1;
}

// grid (items), 64 threads.  An utterance that cannot be aligned gets total = NaN and nothing else.
__global__ __launch_bounds__(64) void align_programme_optional(const float* __restrict__ logp, int frames,
                                                                const int* __restrict__ lengths,
                                                                const int* __restrict__ phonemes,
                                                                const int* __restrict__ optional, int max_phonemes,
                                                                const int* __restrict__ phoneme_lengths,
                                                                uint16_t* __restrict__ dirs,
                                                                uint16_t* __restrict__ skips, int* __restrict__ ends,
                                                                float* __restrict__ total)
{
    __shared__ float4 stage[2][CHUNK_VEC];
    const int item = blockIdx.x, lane = threadIdx.x;
    const int T = lengths[item], N = phoneme_lengths[item];
    const int* sym = phonemes + (size_t)item * max_phonemes;
    const int* opt = optional + (size_t)item * max_phonemes;
    bool fine = T >= 1 && T <= frames && N >= 1 && N <= max_phonemes;
    if (fine) {                                                // one pass over the transcript: phonemes and flags
        bool bad = false;
        int mandatory = 0;
        for (int base = 0; base < N; base += 64) {             // (uniform)
            const int n = base + lane;
            bool needed = false;
            if (n < N) {
                needed = opt[n] == 0;
                bad |= bad_symbol(sym[n]);
                bad |= !needed && n + 1 < N && opt[n + 1] != 0;            // two optional phonemes in a row
            }
            mandatory += __popcll(__ballot(needed));
        }
        fine = !__any(bad) && mandatory >= 1 && mandatory <= T;
    }
    if (!fine) {                                               // (uniform)
        if (lane == 0) total[item] = NAN;
        return;
    }
    const float4* src = reinterpret_cast<const float4*>(logp + (size_t)item * frames * PREP);
    uint16_t* out = dirs + (size_t)item * frames * ROW;
    uint16_t* jumps = skips + (size_t)item * frames * ROW;
    const int shift = strip_shift(N);
    float sum;
    int end;
    if (shift == 0) end = programme_optional<1>(src, T, N, sym, opt, out, jumps, stage, lane, &sum);
    else if (shift == 2) end = programme_optional<4>(src, T, N, sym, opt, out, jumps, stage, lane, &sum);
    else end = programme_optional<16>(src, T, N, sym, opt, out, jumps, stage, lane, &sum);
    if (lane == 0) { total[item] = sum; ends[item] = end; }
}

// grid (items), 64 threads.  Every utterance the programme did not refuse has its end state in `ends`.
__global__ __launch_bounds__(64) void align_traceback_optional(const uint16_t* __restrict__ dirs,
                                                                const uint16_t* __restrict__ skips, int frames,
                                                                const int* __restrict__ lengths, int max_phonemes,
                                                                const int* __restrict__ phoneme_lengths,
                                                                const float* __restrict__ total,
                                                                const int* __restrict__ ends, int* __restrict__ starts)
{
    __shared__ uint4 rows[2][WALK * ROW_VEC];
    const int item = blockIdx.x;
    const int T = lengths[item], N = phoneme_lengths[item];
    if (refused<true>(T, N, frames, max_phonemes, total + item)) return;
    const uint4* const src[2] = {reinterpret_cast<const uint4*>(dirs + (size_t)item * frames * ROW),
                                 reinterpret_cast<const uint4*>(skips + (size_t)item * frames * ROW)};
    traceback<true>(src, T, N, min(max(ends[item], 0), N - 1), starts + (size_t)item * (max_phonemes + 1), rows,
                    threadIdx.x);
}

// grid (ceil(max_phonemes / 64), items), 64 threads
__global__ __launch_bounds__(64) void align_score_optional(const float* __restrict__ logp, int frames,
                                                            const int* __restrict__ lengths,
                                                            const int* __restrict__ phonemes, int max_phonemes,
                                                            const int* __restrict__ phoneme_lengths,
                                                            const float* __restrict__ total,
                                                            const int* __restrict__ starts,
                                                            float* __restrict__ score, float* __restrict__ gop)
{
    score_phoneme<true>(logp, frames, lengths, phonemes, max_phonemes, phoneme_lengths, total, starts, score, gop);
}

// ---- phrase search (ppg_search) ----
//
// Where in a recording is a phoneme sequence said, and how well: the programme above with a free start at every frame
// and a free end.  r[t, n] = logp[t][s[n]] - m[t] (the GOP term: <= 0, exactly 0 at the frame's maximum); before frame
// 0 every state holds -inf.
//   D[t, 0] = r[t, 0] + (0 > D[t-1, 0] ? 0 : D[t-1, 0])     a fresh start, b[t, 0] = t, only if strictly better
//   D[t, n] = r[t, n] + max(D[t-1, n], D[t-1, n-1])          advance only if D[t-1, n-1] > D[t-1, n]
// b[t, n] is the b of the predecessor taken: the first frame of the match that ends in state n at frame t.  The curve
// is D[t, N-1] and b[t, N-1] per end frame, -inf and -1 for t < N-1.  Two kernels beside align_prepare, which is shared:
//   search_programme  grid (queries, items), one wave per pair: the wave, strips (S = 1 or 4 by the query's own N),
//                     staging and gather of align_programme; the emission subtracts the staged maximum, every state
//                     carries its begin, a second cross-lane move brings the begin from lane l - 1, and lane 0 sees the
//                     origin (0, b = t) at every frame.  No direction bits: the lane of state N-1 writes the curve.
//   search_pick       one wave per pair, lanes stride over end frames: per round the largest mean = total / frames, ties
//                     to the largest end frame; end frames whose span meets the hit just taken are struck out of the
//                     workspace's copy of the curve, so a round tests against one hit only.

struct SearchLayout {
    size_t logp, totals, begins, bytes;       // byte offsets into the workspace
};

// (65535 x 65535 pairs of 262144 frames are 9.0e15 bytes: the limits keep this inside a size_t)
inline SearchLayout search_layout(int items, int frames, int queries) {
    SearchLayout w{};
    const size_t curve = (size_t)items * queries * frames * sizeof(float);
    size_t at = 0;
    w.logp = at; at += prepared_bytes(items, frames);
    w.totals = at; at = align256(at + curve);
    w.begins = at; at = align256(at + curve);
    w.bytes = at;
    return w;
}

// The online detector of the live search (its rule stands with the live search below): the search body
// right after it runs it on every frame of a push.
constexpr int DETECTOR = 8;                   // words of a pair's detector
struct Detector {
    int taken, begin, end;                    // begin = -1: nothing is pending
    float total, mean;
    int events;                               // hits emitted since the reset
    int reserved[2];
};
static_assert(sizeof(Detector) == DETECTOR * 4, "the detector is 8 words");

// What a pair hands to its detector and gets back: the outputs of one push.
struct Events {
    int* begin; int* end; float* total; float* mean;           // this pair's `cap` slots
    int cap, count;                                            // count: emitted in this push, written or not
};

__device__ __forceinline__ void emit(Detector& det, Events& out) {
    if (out.count < out.cap) {
        out.begin[out.count] = det.begin;
        out.end[out.count] = det.end;
        out.total[out.count] = det.total;
        out.mean[out.count] = det.mean;
    }
    ++out.count;
    ++det.events;
    det.taken = det.end;
    det.begin = -1;
}

// one frame of the detector: t is the absolute frame, (sum, first) its curve values
__device__ __forceinline__ void detect(Detector& det, Events& out, int t, float sum, int first, float threshold,
                                       int patience) {
    if (det.begin >= 0 && t - (det.end - 1) > patience) emit(det, out);
    if (first < 0 || first < det.taken) return;
    const float value = sum / (float)(t - first + 1);
    if (!(value >= threshold)) return;
    if (det.begin >= 0) {
        if (first < det.end) {                                 // the spans overlap: the better one stays, ties to the later
            if (!(value >= det.mean)) return;
        } else {
            emit(det, out);
        }
    }
    det.begin = first;
    det.end = t + 1;
    det.total = sum;
    det.mean = value;
}

// What a push of a live search carries into the search of one pair and out of it again.
struct Carry {
    float* d; int* b;                         // the pair's strips between pushes: 64 * S words each
    int base;                                 // the stream's position: frame t of the push is frame base + t of the stream
    Detector* det; Events* out;               // the pair's detector, run by the lane of state N-1, and this push's events
    float threshold; int patience;
};

// The search programme of one pair with S states per lane: `programme` with begins.  Live: one push of T frames of a
// stream: the strips come from `live` and go back there (the states at or above N run along as ever), frames count
// from the stream's position, the curve is written only if asked for, and the lane of state N-1 runs the detector.
// Otherwise `live` is unused: every state starts at -inf / -1 and frames count from 0.  One body, so the pushes of a
// stream give the curve of the whole recording bit for bit.  Wave-uniform control flow but for that lane's part.
template <int S, bool Live>
__device__ __forceinline__ void search_strips(const float4* __restrict__ src, int T, int N, const int* __restrict__ sym,
                                              float* __restrict__ totals, int* __restrict__ begins, const Carry& live,
                                              float4 (&stage)[2][CHUNK_VEC], int lane)
{
    int s[S], b[S]; float d[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const int n = lane * S + k;
        s[k] = n < N ? sym[n] : 0;                             // states at or above N run along on phoneme 0, unread
        d[k] = Live ? live.d[n] : -INFINITY;
        b[k] = Live ? live.b[n] : -1;
    }
    const int last = (N - 1) / S, place = (N - 1) % S;         // the lane of state N-1 and its place in the strip
    const int base = Live ? live.base : 0;
    WALK_FRAMES(S, true, t, cur,
        // the state below the strip; below state 0 the origin: 0, beginning at this frame, at every frame
        const float below = lane_up(d[S - 1], 0.f);
        const int origin = lane_up(b[S - 1], base + t);
        _Pragma("unroll") for (int k = S - 1; k >= 0; --k) {   // downwards: d[k - 1] and b[k - 1] are still frame t-1's
            const float stay = d[k]; const float from = k ? d[k - 1] : below;
            const int source = k ? b[k - 1] : origin;
            const bool advance = from > stay;
            d[k] = cur[k] + (advance ? from : stay);           // -inf + finite = -inf: never NaN
            b[k] = advance ? source : b[k];
        }
        if (lane == last) {
            float end = d[0];
            int first = b[0];
            _Pragma("unroll") for (int q = 1; q < S; ++q) {
                end = place == q ? d[q] : end;
                first = place == q ? b[q] : first;
            }
            if (!Live || totals) {
                totals[t] = end;
                begins[t] = first;
            }
            if (Live) detect(*live.det, *live.out, base + t, end, first, live.threshold, live.patience);
        })
    if (Live) {
#pragma unroll
        for (int k = 0; k < S; ++k) {
            live.d[lane * S + k] = d[k];
            live.b[lane * S + k] = b[k];
        }
    }
}

// grid (queries, items), 64 threads.  count = -1 for a pair that cannot be searched, which touches nothing else; 0 for
// every other, whose curve (frames below T) is then in the workspace.
__global__ __launch_bounds__(64) void search_programme(const float* __restrict__ logp, int frames,
                                                        const int* __restrict__ lengths,
                                                        const int* __restrict__ phonemes, int max_phonemes,
                                                        const int* __restrict__ phoneme_lengths,
                                                        float* __restrict__ totals, int* __restrict__ begins,
                                                        int* __restrict__ count)
{
    __shared__ float4 stage[2][CHUNK_VEC];
    const int query = blockIdx.x, item = blockIdx.y, lane = threadIdx.x;
    const size_t pair = (size_t)item * gridDim.x + query;
    const int T = lengths[item], N = phoneme_lengths[query];
    const int* sym = phonemes + (size_t)query * max_phonemes;
    bool fine = T >= 1 && T <= frames && N >= 1 && N <= max_phonemes;
    if (fine) fine = symbols_fine(sym, N, lane);
    if (lane == 0) count[pair] = fine ? 0 : -1;
    if (!fine) return;                                         // (uniform)
    const float4* src = reinterpret_cast<const float4*>(logp + (size_t)item * frames * PREP);
    float* out_totals = totals + pair * frames;
    int* out_begins = begins + pair * frames;
    if (N <= 64) search_strips<1, false>(src, T, N, sym, out_totals, out_begins, Carry{}, stage, lane);
    else search_strips<4, false>(src, T, N, sym, out_totals, out_begins, Carry{}, stage, lane);
}

constexpr int PICK = 4;                       // end frames per lane in flight in the picker

// grid (queries, items), 64 threads.  totals and begins are the workspace's curve: end frames that can no longer be
// taken get begin = -1 there.  Every lane strikes out and later reads its own end frames only.
__global__ __launch_bounds__(64) void search_pick(int frames, const int* __restrict__ lengths,
                                                   const int* __restrict__ phoneme_lengths, int top, float threshold,
                                                   float* __restrict__ totals, int* __restrict__ begins,
                                                   int* __restrict__ begin, int* __restrict__ end,
                                                   float* __restrict__ total, float* __restrict__ mean,
                                                   int* __restrict__ count, float* __restrict__ curve_total,
                                                   int* __restrict__ curve_begin)
{
    const int query = blockIdx.x, item = blockIdx.y, lane = threadIdx.x;
    const size_t pair = (size_t)item * gridDim.x + query;
    if (count[pair] < 0) return;                               // (uniform) refused by the programme
    const int T = lengths[item], N = phoneme_lengths[query];
    float* ct = totals + pair * frames;
    int* cb = begins + pair * frames;
    if (curve_total) {
        for (int t = lane; t < T; t += 64) {
            curve_total[pair * frames + t] = ct[t];
            curve_begin[pair * frames + t] = cb[t];
        }
    }
    int* out_begin = begin + pair * top;
    int* out_end = end + pair * top;
    float* out_total = total + pair * top;
    float* out_mean = mean + pair * top;
    int taken = 0;
    int from = 0, to = 0;                                      // the hit of the round before: frames from .. to - 1
    for (; taken < top; ++taken) {
        float best = -INFINITY;
        int at = -1;
        for (int t0 = N - 1; t0 < T; t0 += PICK * 64) {        // (uniform)
            int b[PICK]; float sum[PICK];
#pragma unroll
            for (int j = 0; j < PICK; ++j) {
                const int t = t0 + j * 64 + lane;
                b[j] = t < T ? cb[t] : -1;
                sum[j] = t < T ? ct[t] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < PICK; ++j) {                   // in order of t: of equal means the later one stays
                const int t = t0 + j * 64 + lane;
                if (b[j] < 0) continue;
                if (b[j] < to && t >= from) { cb[t] = -1; continue; }
                const float value = sum[j] / (float)(t - b[j] + 1);
                if (value >= best) { best = value; at = t; }
            }
        }
#pragma unroll
        for (int step = 1; step < 64; step <<= 1) {
            const float other = __shfl_xor(best, step);
            const int where = __shfl_xor(at, step);
            const bool better = other > best || (other == best && where > at);
            best = better ? other : best;
            at = better ? where : at;
        }
        if (at < 0 || best < threshold) break;                 // (uniform)
        from = cb[at];
        to = at + 1;
        if (lane == 0) {
            out_begin[taken] = from;
            out_end[taken] = to;
            out_total[taken] = ct[at];
            out_mean[taken] = best;
        }
    }
    for (int h = taken + lane; h < top; h += 64) {
        out_begin[h] = out_end[h] = -1;
        out_total[h] = out_mean[h] = NAN;
    }
    if (lane == 0) count[pair] = taken;
}

// ---- live phrase search (ppg_search_stream_*) ----
//
// The search above carried across pushes of a stream.  One pair is a stream of posterior frames and a query
// s[0 .. N-1], 1 <= N <= 256.  A stream has a position p, the number of frames received since its last reset; frame
// indices are absolute: they count from the reset.
//   Curve: the recurrence above, unchanged: the same prepared frame (align_prepare, shared), the same emission
//   r = logp[s[n]] - m, the same strict comparisons, the same fp32 additions in frame order, a fresh origin 0 with b = t
//   at every frame, t the absolute frame index.  A push of F frames at position p computes curve_total[p .. p+F-1] and
//   curve_begin[p .. p+F-1] from the saved (d, b) of every state and saves them again: for any split of a recording into
//   pushes the concatenated curve equals the whole-recording curve bit for bit.
//   Online detector, per pair: threshold (fp32, may be -inf, never NaN) and patience (frames, >= 0); its state is
//   `taken`, the exclusive end of the last emitted hit (initially 0), and at most one pending hit (begin, end, total,
//   mean).  For each frame t in order, after its curve values exist:
//     1. a pending hit with t - (pending.end - 1) > patience is emitted: taken = pending.end, nothing is pending.
//     2. b = curve_begin[t]; if b >= 0 and b >= taken, mean = curve_total[t] / float(t - b + 1) (one fp32 division, as
//        in search_pick); if mean >= threshold, frame t is a candidate (b, t + 1, curve_total[t], mean):
//          nothing pending: the candidate becomes pending;
//          b < pending.end (the spans overlap): the candidate replaces the pending hit when mean >= pending.mean
//          (ties go to the later end frame, as in search_pick);
//          otherwise the spans are disjoint: the pending hit is emitted, taken = pending.end, the candidate is pending.
//   flush emits the pending hit, if any, and sets taken; the curve state and the position are kept.  reset returns a
//   stream to position 0, every state -inf / -1, taken = 0 and nothing pending.  Emitted hits are disjoint, come in
//   stream order and do not depend on how the frames were split into pushes.
// (Detector, Events, emit and detect stand above, in front of search_strips, the one search body, which runs them.)
// The caller owns the state: four blocks, each 256-byte aligned: the position of every stream (int32), the detector of
// every pair (8 words), then d and b of every pair: a whole wave's strips each, 64 words where max_phonemes <= 64 and
// 256 above, so that a strip is loaded and stored without a mask.  Four kernels beside align_prepare:
//   search_stream_programme  grid (queries, streams), one wave per pair: search_strips<S, Live = true>, the body of
//                            search_programme between a load and a store of the strip; the origin's begin is
//                            position + t; the detector runs in the lane of state N-1, in registers, right after that
//                            lane has the frame's two curve values, and stores an event only when it emits one.
//   search_stream_advance    one thread per stream, after the programme: position += length.  The only writer of a
//                            position in a push, so no pair sees it half-done.
//   search_stream_flush      one thread per pair.
//   search_stream_reset      grid (queries, streams), lanes stride over the states.

struct StreamLayout {
    size_t positions, detectors, totals, begins, bytes;        // byte offsets into the state
};

// the saved states of a pair: every lane's strip, for the longest strip a query of this table may have
__host__ __device__ inline int stream_states(int max_phonemes) { return max_phonemes <= 64 ? 64 : 256; }

// (65535 x 65535 pairs of 256 states are 4.4e12 bytes per block: inside a size_t)
inline StreamLayout stream_layout(int streams, int queries, int max_phonemes) {
    StreamLayout w{};
    const size_t pairs = (size_t)streams * queries, states = stream_states(max_phonemes);
    size_t at = 0;
    w.positions = at; at = align256(at + (size_t)streams * sizeof(int));
    w.detectors = at; at = align256(at + pairs * sizeof(Detector));
    w.totals = at; at = align256(at + pairs * states * sizeof(float));
    w.begins = at; at = align256(at + pairs * states * sizeof(int));
    w.bytes = at;
    return w;
}

// grid (queries, streams), 64 threads.  count = -1 for a pair that cannot be pushed, which touches nothing else; every
// other pair gets the events of this push, sentinels behind them, and its state moved on by lengths[stream] frames.
__global__ __launch_bounds__(64) void search_stream_programme(
    const float* __restrict__ logp, int frames, const int* __restrict__ lengths, const int* __restrict__ phonemes,
    int max_phonemes, const int* __restrict__ phoneme_lengths, const int* __restrict__ positions,
    Detector* __restrict__ detectors, float* __restrict__ state_totals, int* __restrict__ state_begins,
    float threshold, int patience, int cap, int* __restrict__ begin, int* __restrict__ end,
    float* __restrict__ total, float* __restrict__ mean, int* __restrict__ count, float* __restrict__ curve_total,
    int* __restrict__ curve_begin)
{
    __shared__ float4 stage[2][CHUNK_VEC];
    const int query = blockIdx.x, item = blockIdx.y, lane = threadIdx.x;
    const size_t pair = (size_t)item * gridDim.x + query;
    const int T = lengths[item], N = phoneme_lengths[query], base = positions[item];
    const int* sym = phonemes + (size_t)query * max_phonemes;
    bool fine = T >= 0 && T <= frames && N >= 1 && N <= max_phonemes && base >= 0 && T <= INT32_MAX - base;
    if (fine) fine = symbols_fine(sym, N, lane);
    if (!fine) {                                               // (uniform)
        if (lane == 0) count[pair] = -1;
        return;
    }
    Events out{begin + pair * cap, end + pair * cap, total + pair * cap, mean + pair * cap, cap, 0};
    const int last = N <= 64 ? N - 1 : (N - 1) >> 2;           // the lane of state N-1
    if (T > 0) {                                               // (uniform) a stream with no frames sits out the step
        const float4* src = reinterpret_cast<const float4*>(logp + (size_t)item * frames * PREP);
        float* out_totals = curve_total ? curve_total + pair * frames : nullptr;
        int* out_begins = curve_total ? curve_begin + pair * frames : nullptr;
        Detector det = detectors[pair];                        // (every lane reads it; the lane of state N-1 uses it)
        const Carry live{state_totals + pair * stream_states(max_phonemes),
                         state_begins + pair * stream_states(max_phonemes), base, &det, &out, threshold, patience};
        if (N <= 64) search_strips<1, true>(src, T, N, sym, out_totals, out_begins, live, stage, lane);
        else search_strips<4, true>(src, T, N, sym, out_totals, out_begins, live, stage, lane);
        if (lane == last) detectors[pair] = det;
    }
    const int events = __shfl(out.count, last);
    if (lane == 0) count[pair] = events;
    for (int h = min(events, cap) + lane; h < cap; h += 64) {
        out.begin[h] = out.end[h] = -1;
        out.total[h] = out.mean[h] = NAN;
    }
}

// grid (ceil(streams / 64)), 64 threads: thread = stream.  The condition is the programme's own.
__global__ __launch_bounds__(64) void search_stream_advance(int streams, int frames, const int* __restrict__ lengths,
                                                             int* __restrict__ positions)
{
    const int item = blockIdx.x * 64 + threadIdx.x;
    if (item >= streams) return;
    const int T = lengths[item], base = positions[item];
    if (T >= 0 && T <= frames && base >= 0 && T <= INT32_MAX - base) positions[item] = base + T;
}

// grid (ceil(streams * queries / 64)), 64 threads: thread = pair
__global__ __launch_bounds__(64) void search_stream_flush(int streams, int queries, const int* __restrict__ which,
                                                           Detector* __restrict__ detectors, int* __restrict__ begin,
                                                           int* __restrict__ end, float* __restrict__ total,
                                                           float* __restrict__ mean, int* __restrict__ count)
{
    const size_t pair = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (pair >= (size_t)streams * queries) return;
    Detector det = detectors[pair];
    const bool hit = (!which || which[pair / queries] != 0) && det.begin >= 0;
    begin[pair] = hit ? det.begin : -1;
    end[pair] = hit ? det.end : -1;
    total[pair] = hit ? det.total : NAN;
    mean[pair] = hit ? det.mean : NAN;
    count[pair] = hit;
    if (hit) {
        ++det.events;
        det.taken = det.end;
        det.begin = -1;
        detectors[pair] = det;
    }
}

// grid (queries, streams), 64 threads
__global__ __launch_bounds__(64) void search_stream_reset(int max_phonemes, const int* __restrict__ which,
                                                           int* __restrict__ positions,
                                                           Detector* __restrict__ detectors,
                                                           float* __restrict__ state_totals,
                                                           int* __restrict__ state_begins)
{
    const int query = blockIdx.x, item = blockIdx.y, lane = threadIdx.x;
    if (which && which[item] == 0) return;                     // (uniform)
    const size_t pair = (size_t)item * gridDim.x + query;
    const int states = stream_states(max_phonemes);
    for (int n = lane; n < states; n += 64) {
        state_totals[pair * states + n] = -INFINITY;
        state_begins[pair * states + n] = -1;
    }
    if (lane == 0) {
        detectors[pair] = Detector{0, -1, 0, 0.f, 0.f, 0, {0, 0}};
        if (query == 0) positions[item] = 0;
    }
}

// ---- phoneme recognition (ppg_recognize) ----
//
// What was said: the best path through the 40 phonemes under a transition model A (40, 40), A[p, q] the weight of going
// from p at frame t-1 to q at frame t, with weights `initial` on the first frame's state and `final` on the last one's.
//   e[t, q] = the prepared frame of align_prepare
//   D[0, q] = e[0, q] + initial[q]
//   c[p]    = D[t-1, p] + A[p, q]                              one fp32 addition per candidate
//   best = c[q], from = q;  for p = 0 .. 39, p != q:  if c[p] > best: best = c[p], from = p
//   D[t, q] = e[t, q] + best                                   fp32, in order of t
//   F[q] = D[T-1, q] + final[q];  last = the first q with the largest F (strict >, ascending q);  total = F[last]
// Comparisons only: staying beats switching and the lowest predecessor beats a higher one on ties; -inf + finite = -inf
// and -inf > -inf is false, so a state nothing reaches never gives NaN.  With the left-to-right chain of a transcript
// as A this is align_programme bit for bit, with A = 0 it is decode_runs.  Three kernels beside align_prepare and
// align_score, which are shared:
//   recognize_programme  one wave per utterance, lane q < 40 = state q: D[q] in a register, column A[., q] in 40
//                        registers, the emission through WALK_FRAMES with S = 1 and the identity as phoneme table.  A
//                        frame is a 40 x 40 max-plus product: every lane needs all 40 D[p], which come as wave-uniform
//                        operands from 40 v_readlane_b32 with constant lane index (DESIGN 4.15 has the comparison with
//                        the broadcast through LDS).  Lanes 40 .. 63 hold -inf and are never a predecessor.  One
//                        back-pointer byte per state and frame; a lane packs four frames into a dword, so the wave
//                        stores 256 contiguous bytes every fourth frame.
//   recognize_traceback  one wave per utterance: back-pointer rows come through LDS 64 frames (4 KiB) at a time, the next
//                        refill in flight; the walk is wave-uniform; lane t % 64 keeps frame t's label and the wave
//                        stores 64 labels at once.
//   recognize_runs       one wave per utterance: decode_runs' run compression (open_runs) on the label row.
// align_score then scores the runs as a transcript of `runs` phonemes among at most `frames`.

constexpr int BACK = 4;                       // frames per back-pointer dword
constexpr int BACK_ROW = 64 * BACK;           // bytes a wave stores per BACK frames
constexpr int BACK_VEC = WALK / BACK * BACK_ROW / 16;          // 16-byte pieces per refill of the trace-back: 256

struct RecognizeLayout {
    size_t logp, back, labels, ends, bytes;   // byte offsets into the workspace
};

// back-pointer bytes of one utterance: whole dwords of BACK frames
__host__ __device__ inline size_t back_bytes(int frames) { return (size_t)((frames + BACK - 1) / BACK) * BACK_ROW; }

// (65535 items of 262144 frames are 4.2e12 bytes: inside a size_t)
inline RecognizeLayout recognize_layout(int items, int frames) {
    RecognizeLayout w{};
    size_t at = 0;
    w.logp = at; at += prepared_bytes(items, frames);
    w.back = at; at = align256(at + (size_t)items * back_bytes(frames));
    w.labels = at; at = align256(at + (size_t)items * frames * sizeof(int));
    w.ends = at; at = align256(at + (size_t)items * sizeof(int));
    w.bytes = at;
    return w;
}

// lane p's value as a wave-uniform operand
__device__ __forceinline__ float from_lane(float v, int p) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), p));
}

// What a push of a live recogniser carries into the frames of one stream and out of it again.
struct Ring {
    float* d;                                 // D of the stream's last frame: a whole wave's lanes, 40 .. 63 at -inf
    int base, window;                         // the stream's position; the frames of its ring
    int* anc; int commit;                     // anc[q] = path(q, c), carried forward; the commit point c
};

// The frames of one utterance, lane q < 40 = state q: D of the last frame is returned.  Live: one push of T frames of a
// stream: D comes from `live` and goes back there, frames count from the stream's position (only absolute frame 0
// takes `initial`), and `out` is the stream's ring of back-pointer dwords, W / BACK rows of 64, where the row of the
// frames at(t) / BACK wraps; a row the push before left partly filled is taken up again; every state's ancestor at the
// commit point goes along (what lets the commit skip a walk that cannot commit).  Otherwise `live` is
// unused:
// D starts at -inf, frames count from 0 and `out` holds the utterance's rows one after the other.  One body, so the
// pushes of a stream give D and the back-pointers of the whole recording bit for bit.  Wave-uniform control flow.
template <bool Live>
__device__ __forceinline__ float recognize_frames(const float4* __restrict__ src, int T,
                                                  const float* __restrict__ transitions,
                                                  const float* __restrict__ initial, uint32_t* __restrict__ out,
                                                  const Ring& live, float4 (&stage)[2][CHUNK_VEC], int lane)
{
    const bool state = lane < NP;
    const int s[1] = {state ? lane : 0};                       // the identity; lanes 40 .. 63 run along on phoneme 0
    float a[NP];                                               // column `lane` of the transitions
#pragma unroll
    for (int p = 0; p < NP; ++p) a[p] = state ? transitions[p * NP + lane] : -INFINITY;
    const float stay = state ? transitions[lane * NP + lane] : -INFINITY;
    const float first = !state ? -INFINITY : initial ? initial[lane] : 0.f;
    const int base = Live ? live.base : 0;
    const int words = Live ? live.window / BACK : 0;           // rows of the ring
    int word = Live ? base % live.window / BACK : 0;           // the row of the frame in hand
    float d = Live ? live.d[lane] : -INFINITY;
    int anc = Live ? live.anc[lane] : 0;
    // this lane's back-pointers of up to BACK frames.  (In a full ring the other bytes of a row that is taken up again
    // or left partly filled are those of the frames W earlier, which are still in use: they are masked out here and
    // left alone at the end.)
    uint32_t packed = Live && base % BACK ? out[(size_t)word * 64 + lane] & ((1u << 8 * (base % BACK)) - 1u) : 0;
    WALK_FRAMES(1, false, t, cur,
        const int at = base + t;                               // the absolute frame
        int from = lane;
        if (at == 0) {                                         // (uniform)
            d = cur[0] + first;
        } else {
            const float before = d;
            float best = before + stay;                        // staying: what a switch has to beat
            _Pragma("unroll") for (int p0 = 0; p0 < NP; p0 += 8) {
                float c[8];                                    // eight at a time: the moves stand ahead of their uses
                _Pragma("unroll") for (int j = 0; j < 8; ++j) c[j] = from_lane(before, p0 + j);
                _Pragma("unroll") for (int j = 0; j < 8; ++j) c[j] += a[p0 + j];
                _Pragma("unroll") for (int j = 0; j < 8; ++j) {    // ascending: the lowest of equal predecessors stays
                    const bool better = c[j] > best;           // (p = lane repeats `best` or less: never taken)
                    best = better ? c[j] : best;
                    from = better ? p0 + j : from;
                }
            }
            d = cur[0] + best;                                 // -inf + finite = -inf: never NaN
        }
        if (Live) anc = at == live.commit ? lane : __builtin_amdgcn_ds_bpermute(from << 2, anc);
        packed |= (uint32_t)from << (8 * (at % BACK));
        if (at % BACK == BACK - 1) {                           // (uniform)
            out[(size_t)(Live ? word : t / BACK) * 64 + lane] = packed;
            packed = 0;
            if (Live) word = word + 1 == words ? 0 : word + 1;
        })
    if (Live) {                                                // the partial dword, its own bytes only
        uint8_t* bytes = reinterpret_cast<uint8_t*>(out + (size_t)word * 64 + lane);
        for (int b = 0; b < (base + T) % BACK; ++b) bytes[b] = (uint8_t)(packed >> 8 * b);
    } else if (T % BACK) {
        out[(size_t)(T / BACK) * 64 + lane] = packed;          // (uniform) the last, partial dword
    }
    if (Live) { live.d[lane] = d; live.anc[lane] = anc; }
    return d;
}

// the first of the largest of the 40 states' `value` (strict >, ascending), wave-uniform: its state; *most is its value
__device__ __forceinline__ int first_largest(float value, float* most) {
    float sum = from_lane(value, 0);
    int end = 0;
#pragma unroll
    for (int q = 1; q < NP; ++q) {
        const float f = from_lane(value, q);
        const bool better = f > sum;
        sum = better ? f : sum;
        end = better ? q : end;
    }
    *most = sum;
    return end;
}

// grid (items), 64 threads.  initial and final_ may be null: all zeros.  An utterance whose length is impossible gets
// total = NaN and runs = 0, one without a path total = -inf and runs = 0; every other its total, its end state in
// `ends` and its back-pointers.
__global__ __launch_bounds__(64) void recognize_programme(const float* __restrict__ logp, int frames,
                                                           const int* __restrict__ lengths,
                                                           const float* __restrict__ transitions,
                                                           const float* __restrict__ initial,
                                                           const float* __restrict__ final_,
                                                           uint32_t* __restrict__ back, int* __restrict__ ends,
                                                           int* __restrict__ runs, float* __restrict__ total)
{
    __shared__ float4 stage[2][CHUNK_VEC];
    const int item = blockIdx.x, lane = threadIdx.x;
    const int T = lengths[item];
    if (T < 1 || T > frames) {                                 // (uniform)
        if (lane == 0) { total[item] = NAN; runs[item] = 0; }
        return;
    }
    const float4* src = reinterpret_cast<const float4*>(logp + (size_t)item * frames * PREP);
    const float d = recognize_frames<false>(src, T, transitions, initial,
                                            back + (size_t)item * (back_bytes(frames) / 4), Ring{}, stage, lane);
    const float last = d + (lane >= NP ? -INFINITY : final_ ? final_[lane] : 0.f);
    float sum;
    const int end = first_largest(last, &sum);
    if (lane == 0) {
        total[item] = sum;
        if (sum > -INFINITY) ends[item] = end;
        else runs[item] = 0;                                   // no path: nothing else is written
    }
}

// whether the programme left a path for this utterance: a plausible length and a total above -inf (NaN is not)
__device__ __forceinline__ bool recognized(int T, int frames, const float* __restrict__ total) {
    return T >= 1 && T <= frames && *total > -INFINITY;
}

// grid (items), 64 threads
__global__ __launch_bounds__(64) void recognize_traceback(const uint32_t* __restrict__ back, int frames,
                                                           const int* __restrict__ lengths,
                                                           const float* __restrict__ total,
                                                           const int* __restrict__ ends, int* __restrict__ labels)
{
    __shared__ uint4 rows[BACK_VEC];
    const int item = blockIdx.x, lane = threadIdx.x;
    const int T = lengths[item];
    if (!recognized(T, frames, total + item)) return;          // (uniform)
    const uint4* src = reinterpret_cast<const uint4*>(back + (size_t)item * (back_bytes(frames) / 4));
    int* out = labels + (size_t)item * frames;
    constexpr int PER = BACK_VEC / 64;
    uint4 next[PER];
    auto load = [&](int c) {                                   // rows of frames c * WALK ..., whole dwords below T only
        const int pieces = (min(WALK, T - c * WALK) + BACK - 1) / BACK * (BACK_ROW / 16);
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int idx = u * 64 + lane;
            next[u] = idx < pieces ? src[(size_t)c * BACK_VEC + idx] : make_uint4(0, 0, 0, 0);
        }
    };
    int n = min(max(ends[item], 0), NP - 1);
    int c = (T - 1) / WALK;
    load(c);
    for (; c >= 0; --c) {
        __syncthreads();                                       // the walk over the previous refill is over
#pragma unroll
        for (int u = 0; u < PER; ++u) rows[u * 64 + lane] = next[u];
        __syncthreads();
        if (c > 0) load(c - 1);
        const uint8_t* row = reinterpret_cast<const uint8_t*>(rows);
        const int high = min(T - 1, c * WALK + WALK - 1);
        int mine = 0;
        for (int t = high; t >= c * WALK; --t) {
            if (lane == (t & (WALK - 1))) mine = n;            // frame t's label
            // frame t's predecessor: the same address in every lane (frame 0 has none; its byte is not used)
            if (t > 0) n = row[((t & (WALK - 1)) / BACK * 64 + n) * BACK + t % BACK] & 63;
        }
        if (c * WALK + lane <= high) out[c * WALK + lane] = mine;
    }
}

// grid (items), 64 threads: lane = frame of the current 64
__global__ __launch_bounds__(64) void recognize_runs(const int* __restrict__ labels, int frames,
                                                      const int* __restrict__ lengths,
                                                      const float* __restrict__ total, int* __restrict__ phonemes,
                                                      int* __restrict__ starts, int* __restrict__ runs)
{
    const int item = blockIdx.x, lane = threadIdx.x;
    const int T = lengths[item];
    if (!recognized(T, frames, total + item)) return;          // (uniform) the programme has set runs = 0
    const int* src = labels + (size_t)item * frames;
    int* out_phonemes = phonemes + (size_t)item * frames;
    int* out_starts = starts + (size_t)item * (frames + 1);
    int carry = -1, base = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        open_runs(t < T ? src[t] : -2, t, T, lane, carry, base, out_phonemes, out_starts);
    }
    if (lane == 0) { runs[item] = base; out_starts[base] = T; }
}

// ---- live phoneme recognition (ppg_recognize_stream_*) ----
//
// The recogniser above carried across the pushes of a stream.  A stream has a position p (frames since its reset, frame
// indices are absolute), a commit point c <= p (frames below c have had their label given out for good), D of frame
// p-1, a ring of W frames (slot t % W) with the back-pointers, the prepared frames and the labels of the frames in
// [c, p), one open run (label, start, fp32 sum and below) and the counter `forced`.
//   Forward: recognize_frames<Live = true>, the body of recognize_programme: D and the back-pointers of every frame are
//   the bits recognize_programme computes for the whole recording, whatever the pushes.
//   Commit, once per stream and push, t = p-1, alive(q) = D[q] > -inf, path(q, u) = the state at frame u of the
//   trace-back from q at t:
//     natural  v = the largest u in [c, t] at which path(q, u) is the same for every alive q (none: v = c-1); frames
//              c .. v get that label, c = v+1.  No state alive: nothing is committed.
//     forced   only if p - c > max_lag = L after that: best = the first alive q with the largest D; frames c .. p-L-1
//              get path(best, .); every q with path(q, p-L-1) != path(best, p-L-1) gets D[q] = -inf; forced grows by
//              the frames committed this way; c = p-L.
//     runs     every newly committed frame, in order, extends the open run (sum += e[t, label], below += e[t, label] -
//              max[t], fp32 from 0.f: the order of align_score) or closes it and opens the next; a closed run is emitted
//              as (phoneme, begin, end, sum / float(end - begin), below / float(end - begin)).
//   A stream with (p - c) + length > W, a length outside [0, frames] or a position that would pass INT32_MAX is
//   impossible: count = -1 and nothing else changes.  flush: F = D + final, last = the first of the largest, total =
//   F[last]; if total > -inf everything up to p is committed along path(last, .); the open run is closed and emitted,
//   total and forced are reported and the stream is reset.  reset: p = c = 0, D = -inf, no open run, forced = 0.
// The caller owns the state: six blocks, each 256-byte aligned: the head of every stream (8 words), D (64 words), the
// ancestors (64 words: anc[q] = path(q, c), see below), the back-pointer ring (64 B per frame, in rows of BACK frames),
// the ring of prepared frames (176 B per frame) and the ring of labels (int32).  Five kernels beside align_prepare, one
// wave per stream:
//   recognize_stream_programme  copies the push's prepared frames into the ring and runs recognize_frames<true>, which
//                               also carries the ancestors forward: anc[q] = q at frame c, else anc[from[q]], one
//                               cross-lane move per frame.  If the alive states' ancestors differ, no u in [c, t] has
//                               all alive paths in one state (paths that meet stay together), so unless a commit has
//                               to be forced the commit kernel has nothing to give out and skips its walk.
//   recognize_stream_commit     lane q walks its own path back from t, the rows through LDS 64 frames at a time as in
//                               recognize_traceback; a ballot per frame finds v, frame p-L-1 forces; lane u % 64 keeps
//                               frame u's label and the wave stores 64 at once; then the new labels 64 at a time, lane =
//                               frame: a ballot finds where runs open, and the sums go in frame order over the lanes.
//   recognize_stream_advance    one thread per stream, after the commit: p += length unless the stream was refused.
//   recognize_stream_flush, recognize_stream_reset

constexpr int HEAD = 8;                       // words of a stream's head
struct RecognizeHead {
    int position, commit, forced;
    int label, start;                         // the open run: label = -1: none
    float sum, below;
    int reserved;
};
static_assert(sizeof(RecognizeHead) == HEAD * 4, "the head is 8 words");

struct RecognizeStreamLayout {
    size_t heads, d, anc, back, kept, labels, bytes;                // byte offsets into the state
};

// (65535 streams of 65536 frames are 1.0e12 bytes: inside a size_t)
inline RecognizeStreamLayout recognize_stream_layout(int streams, int window) {
    RecognizeStreamLayout w{};
    const size_t slots = (size_t)streams * window;
    size_t at = 0;
    w.heads = at; at = align256(at + (size_t)streams * sizeof(RecognizeHead));
    w.d = at; at = align256(at + (size_t)streams * 64 * sizeof(float));
    w.anc = at; at = align256(at + (size_t)streams * 64 * sizeof(int));
    w.back = at; at = align256(at + slots * 64);
    w.kept = at; at = align256(at + slots * PREP * sizeof(float));
    w.labels = at; at = align256(at + slots * sizeof(int));
    w.bytes = at;
    return w;
}

// what a stream may be asked to take; everything else gets count = -1 and touches nothing
__device__ __forceinline__ bool pushable(int T, int frames, int p, int c, int window) {
    return T >= 0 && T <= frames && c >= 0 && c <= p && T <= INT32_MAX - p && p - c <= window &&
           T <= window - (p - c);
}

// grid (streams), 64 threads
__global__ __launch_bounds__(64) void recognize_stream_programme(const float* __restrict__ logp, int frames,
                                                                  const int* __restrict__ lengths,
                                                                  const float* __restrict__ transitions,
                                                                  const float* __restrict__ initial, int window,
                                                                  const RecognizeHead* __restrict__ heads,
                                                                  float* __restrict__ state_d,
                                                                  int* __restrict__ state_anc,
                                                                  uint32_t* __restrict__ back,
                                                                  float4* __restrict__ kept)
{
    __shared__ float4 stage[2][CHUNK_VEC];
    const int item = blockIdx.x, lane = threadIdx.x;
    const int T = lengths[item], p = heads[item].position, c = heads[item].commit;
    if (!pushable(T, frames, p, c, window) || T == 0) return;  // (uniform) refused, or the stream sits out the step
    const float4* src = reinterpret_cast<const float4*>(logp + (size_t)item * frames * PREP);
    float4* ring = kept + (size_t)item * window * PREP_VEC;
    const int slot0 = p % window;
    for (int idx = lane; idx < T * PREP_VEC; idx += 64) {      // T <= window: a slot wraps once at most
        int slot = slot0 + idx / PREP_VEC;
        slot = slot >= window ? slot - window : slot;
        ring[(size_t)slot * PREP_VEC + idx % PREP_VEC] = src[idx];
    }
    recognize_frames<true>(src, T, transitions, initial, back + (size_t)item * window * (64 / 4),
                           Ring{state_d + (size_t)item * 64, p, window, state_anc + (size_t)item * 64, c}, stage, lane);
}

// What a stream hands to its commit and gets back: the run outputs of one push or flush.
struct Runs {
    int* phonemes; int* begin; int* end; float* score; float* gop;         // this stream's `cap` slots; gop may be null
    int cap, count;                                                        // count: closed here, written or not
};

// the open run ends in front of frame `end`.  Wave-uniform; lane 0 writes.
__device__ __forceinline__ void close_run(const RecognizeHead& run, int end, Runs& out, int lane) {
    if (lane == 0 && out.count < out.cap) {
        const float count = (float)(end - run.start);
        out.phonemes[out.count] = run.label;
        out.begin[out.count] = run.start;
        out.end[out.count] = end;
        out.score[out.count] = run.sum / count;
        if (out.gop) out.gop[out.count] = run.below / count;
    }
    ++out.count;
}

// The commit of one stream whose position is p (after the push): `head` holds its commit point, open run and counter
// and gets the new ones.  `lead` is the state whose path gives the labels: the best alive state of a push, the end state
// of a flush, or -1 if there is none (nothing is committed then).  Flush: everything up to p goes along that path and
// nothing is forced.  Otherwise the natural and the forced commit of the text above, and the ancestors at the new commit
// point are left for the next push.  Wave-uniform control flow.
template <bool Flush>
__device__ __forceinline__ void commit(RecognizeHead& head, int p, int lead, bool alive, int max_lag, int window,
                                       float* __restrict__ state_d, int* __restrict__ state_anc,
                                       const uint32_t* __restrict__ back,
                                       const float* __restrict__ kept, int* __restrict__ labels, Runs& out,
                                       uint4 (&rows)[BACK_VEC], int lane)
{
    const int c = head.commit, t = p - 1;
    const int force = Flush ? -1 : p - max_lag - 1;            // the frame a forced commit reaches up to
    int fresh = c, natural = c;                                // the new commit point; what the natural commit gives
    // the alive states' ancestors at c differ, so their paths meet nowhere in [c, t]: nothing to commit unless by force
    bool apart = false;
    if (!Flush && lead >= 0) {
        const int anc = state_anc[lane];
        apart = __ballot(alive && anc != __builtin_amdgcn_readlane(anc, lead)) != 0 && p - c <= max_lag;
    }
    if (lead >= 0 && t >= c && !apart) {                       // (uniform)
        constexpr int PER = BACK_VEC / 64;
        const uint4* src = reinterpret_cast<const uint4*>(back);
        uint4 next[PER];
        auto load = [&](int chunk) {                           // rows of frames chunk * WALK ..., those of [c, t] only
            const int first = chunk * WALK;
            const int low = (max(c, first) - first) / BACK, high = (min(t, first | (WALK - 1)) - first) / BACK;
            const size_t at = (size_t)(first % window / BACK) * (BACK_ROW / 16);
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const int idx = u * 64 + lane, row = idx / (BACK_ROW / 16);
                next[u] = row >= low && row <= high ? src[at + idx] : make_uint4(0, 0, 0, 0);
            }
        };
        bool agreed = Flush, committing = Flush;
        if (Flush) fresh = natural = p;
        int n = lane;                                          // lane q's state at frame u of its own path
        int above = lane, fresh_anc = lane;                    // ... at frame u + 1; ... at the new commit point
        int chunk = t / WALK;
        const int last = c / WALK;
        load(chunk);
        for (; chunk >= last; --chunk) {
            __syncthreads();                                   // the walk over the previous refill is over
#pragma unroll
            for (int u = 0; u < PER; ++u) rows[u * 64 + lane] = next[u];
            __syncthreads();
            if (chunk > last) load(chunk - 1);
            const uint8_t* row = reinterpret_cast<const uint8_t*>(rows);
            const int high = min(t, chunk * WALK | (WALK - 1)), low = max(c, chunk * WALK);
            int mine = -1;
            for (int u = high; u >= low; --u) {
                const int here = __builtin_amdgcn_readlane(n, lead);       // the label of frame u, if it is given out
                if (!agreed && __ballot(alive && n != here) == 0) {        // every alive path is in one state
                    agreed = true;
                    natural = u + 1;
                }
                if (!committing && (agreed || u == force)) {
                    committing = true;
                    fresh = u + 1;
                    fresh_anc = above;
                    if (!agreed && alive && n != here) state_d[lane] = -INFINITY;  // forced: the other paths end
                }
                if (committing && lane == (u & (WALK - 1))) mine = here;
                above = n;
                // frame u's predecessor on this lane's path (frame c's is not needed)
                if (u > c) n = row[((u & (WALK - 1)) / BACK * 64 + n) * BACK + u % BACK] & 63;
            }
            if (mine >= 0) labels[(chunk * WALK + lane) % window] = mine;
        }
        if (!Flush) head.forced += fresh - natural;
        if (!Flush && committing) state_anc[lane] = fresh_anc;
    }
    __threadfence_block();
    __syncthreads();                                           // the labels are there for every lane
    // the newly committed frames c .. fresh-1, 64 at a time: lane = frame
    const int count = fresh - c, slot0 = c % window;
    int carry = head.label;
    for (int k0 = 0; k0 < count; k0 += 64) {                   // (uniform)
        const int k = k0 + lane;
        int slot = slot0 + k;
        slot = slot >= window ? slot - window : slot;
        int label = -2;
        float e = 0.f, top = 0.f;
        if (k < count) {
            label = min(max(labels[slot], 0), NP - 1);
            e = kept[(size_t)slot * PREP + label];
            top = kept[(size_t)slot * PREP + NP];
        }
        const float under = e - top;                           // exactly 0 where the label is the frame's maximum
        const unsigned long long opens = __ballot(k < count && label != lane_up(label, carry));
        const int here = min(64, count - k0);
        for (int j = 0; j < here; ++j) {                       // in frame order: every lane keeps the same sums
            if ((opens >> j) & 1) {
                if (head.label >= 0) close_run(head, c + k0 + j, out, lane);
                head.label = __builtin_amdgcn_readlane(label, j);
                head.start = c + k0 + j;
                head.sum = head.below = 0.f;
            }
            head.sum += from_lane(e, j);
            head.below += from_lane(under, j);
        }
        carry = __builtin_amdgcn_readlane(label, 63);
    }
    head.commit = fresh;
}

// slots at or past the runs written: -1 / NaN
__device__ __forceinline__ void fill_runs(const Runs& out, int lane) {
    for (int h = min(out.count, out.cap) + lane; h < out.cap; h += 64) {
        out.phonemes[h] = out.begin[h] = out.end[h] = -1;
        out.score[h] = NAN;
        if (out.gop) out.gop[h] = NAN;
    }
}

__device__ __forceinline__ Runs runs_of(int item, int cap, int* phonemes, int* begin, int* end, float* score,
                                        float* gop) {
    const size_t at = (size_t)item * cap;
    return Runs{phonemes + at, begin + at, end + at, score + at, gop ? gop + at : nullptr, cap, 0};
}

// grid (streams), 64 threads, after the programme and before the advance: the head still holds the old position.
__global__ __launch_bounds__(64) void recognize_stream_commit(int frames, const int* __restrict__ lengths, int window,
                                                               int max_lag, RecognizeHead* __restrict__ heads,
                                                               float* __restrict__ state_d,
                                                               int* __restrict__ state_anc,
                                                               const uint32_t* __restrict__ back,
                                                               const float* __restrict__ kept,
                                                               int* __restrict__ labels, int cap,
                                                               int* __restrict__ phonemes, int* __restrict__ begin,
                                                               int* __restrict__ end, float* __restrict__ score,
                                                               float* __restrict__ gop, int* __restrict__ count)
{
    __shared__ uint4 rows[BACK_VEC];
    const int item = blockIdx.x, lane = threadIdx.x;
    const int T = lengths[item];
    RecognizeHead head = heads[item];
    if (!pushable(T, frames, head.position, head.commit, window)) {        // (uniform)
        if (lane == 0) count[item] = -1;
        return;
    }
    float* d = state_d + (size_t)item * 64;
    const float mine = d[lane];
    float most;
    const int best = first_largest(mine, &most);
    Runs out = runs_of(item, cap, phonemes, begin, end, score, gop);
    commit<false>(head, head.position + T, most > -INFINITY ? best : -1, mine > -INFINITY, max_lag, window, d,
                  state_anc + (size_t)item * 64,
                  back + (size_t)item * window * (64 / 4), kept + (size_t)item * window * PREP,
                  labels + (size_t)item * window, out, rows, lane);
    if (lane == 0) {
        heads[item] = head;                                    // (the position is the advance's to move)
        count[item] = out.count;
    }
    fill_runs(out, lane);
}

// grid (ceil(streams / 64)), 64 threads: thread = stream.  The commit has said whether the stream took its frames.
__global__ __launch_bounds__(64) void recognize_stream_advance(int streams, const int* __restrict__ lengths,
                                                                const int* __restrict__ count,
                                                                RecognizeHead* __restrict__ heads)
{
    const int item = blockIdx.x * 64 + threadIdx.x;
    if (item >= streams) return;
    if (count[item] >= 0) heads[item].position += lengths[item];
}

// a stream at frame 0.  Wave-uniform; every lane writes its D and its ancestor.
__device__ __forceinline__ void restart(RecognizeHead* head, float* d, int* anc, int lane) {
    d[lane] = -INFINITY;
    anc[lane] = lane;
    if (lane == 0) *head = RecognizeHead{0, 0, 0, -1, 0, 0.f, 0.f, 0};
}

// grid (streams), 64 threads.  A stream `which` leaves out gets count = 0, total = NaN, forced = -1 and keeps its state.
__global__ __launch_bounds__(64) void recognize_stream_flush(int window, const float* __restrict__ final_,
                                                              const int* __restrict__ which,
                                                              RecognizeHead* __restrict__ heads,
                                                              float* __restrict__ state_d,
                                                              int* __restrict__ state_anc,
                                                              const uint32_t* __restrict__ back,
                                                              const float* __restrict__ kept,
                                                              int* __restrict__ labels, int cap,
                                                              int* __restrict__ phonemes, int* __restrict__ begin,
                                                              int* __restrict__ end, float* __restrict__ score,
                                                              float* __restrict__ gop, int* __restrict__ count,
                                                              float* __restrict__ total, int* __restrict__ forced)
{
    __shared__ uint4 rows[BACK_VEC];
    const int item = blockIdx.x, lane = threadIdx.x;
    Runs out = runs_of(item, cap, phonemes, begin, end, score, gop);
    RecognizeHead head = heads[item];
    const bool meant = !which || which[item] != 0;
    // (a head that no reset or push of this library left gives nothing out and is reset)
    const bool sound = head.commit >= 0 && head.commit <= head.position && head.position - head.commit <= window;
    float sum = NAN;
    if (meant && sound) {                                      // (uniform)
        float* d = state_d + (size_t)item * 64;
        const float last = d[lane] + (lane >= NP ? -INFINITY : final_ ? final_[lane] : 0.f);
        const int state = first_largest(last, &sum);
        commit<true>(head, head.position, sum > -INFINITY ? state : -1, false, 0, window, d, nullptr,
                     back + (size_t)item * window * (64 / 4), kept + (size_t)item * window * PREP,
                     labels + (size_t)item * window, out, rows, lane);
        if (head.label >= 0) close_run(head, head.commit, out, lane);
    }
    if (lane == 0) {
        count[item] = out.count;
        total[item] = meant && sound ? sum : NAN;
        forced[item] = meant && sound ? head.forced : -1;
    }
    fill_runs(out, lane);
    if (meant) restart(heads + item, state_d + (size_t)item * 64, state_anc + (size_t)item * 64, lane);
}

// grid (streams), 64 threads
__global__ __launch_bounds__(64) void recognize_stream_reset(const int* __restrict__ which,
                                                              RecognizeHead* __restrict__ heads,
                                                              float* __restrict__ state_d,
                                                              int* __restrict__ state_anc)
{
    const int item = blockIdx.x;
    if (which && which[item] == 0) return;                     // (uniform)
    restart(heads + item, state_d + (size_t)item * 64, state_anc + (size_t)item * 64, threadIdx.x);
}

// ---- Viterbi over a phoneme graph (ppg_viterbi) ----
//
// The best path through a graph whose S <= 1024 states each carry a phoneme: state n has a weight stay[n], an ordered
// list of in-arcs (src[j], w[j]), j < deg(n) <= 255, and weights initial[n] and final[n].
//   e[t, n] = the prepared frame of align_prepare at sym[n]
//   D[0, n] = e[0, n] + initial[n]
//   best = D[t-1, n] + stay[n], from = 0;  for j in list order: c = D[t-1, src[j]] + w[j]; if c > best: best = c, from = j+1
//   D[t, n] = e[t, n] + best                                   fp32, one addition per candidate, in order of t
//   F[n] = D[T-1, n] + final[n];  last = the first n with the largest F (strict >, ascending);  total = F[last]
// A run opens at frame 0 and at every frame of the trace-back whose `from` != 0.  Four kernels beside align_prepare and
// align_score, which are shared:
//   viterbi_check      one wave per GRAPH of the call, not per item: every index and weight of the packed graphs is
//                      tested, each before the read that depends on it, and a verdict is left.  The kernels below trust
//                      a graph with a good verdict and touch no other.
//   viterbi_programme  one wave per utterance.  A state's predecessors are other lanes' states, so D of frame t-1 is read
//                      by index from LDS (two buffers of 1024 floats, one barrier per frame), and what a state keeps
//                      (phoneme, first arc and degree in one word, the stay weight) stands in LDS beside it: nothing of
//                      a state lives in registers across frames, so 1024 states cost no more registers than 64.  If the
//                      call's graphs have at most 64 states, lane n takes state n; else a frame is ceil(S / 256) passes
//                      in which lane l takes the four neighbouring states 4 l .. 4 l + 3 of the pass, whose words move
//                      as 16-byte pieces.  The arcs, 8 bytes each (source, weight), are copied to LDS once if the graph
//                      has at most `held` of them, else they come from the caller's arrays (L2) every frame.  The first
//                      VLEAD arcs of a lane's states are taken in lock step, so their LDS reads are in flight together
//                      (a chain ends there); the rest state by state, four arcs and then eight at a time.  One
//                      back-pointer byte per state and frame, the ordinal `from`: a lane's four are one dword, 256
//                      contiguous bytes a wave.
//   viterbi_traceback  one wave per utterance: back-pointer rows come through LDS 16 KiB at a time, the next refill in
//                      flight, and of a row only what the graph's own passes wrote, whatever the call's largest graph
//                      is; the walk is wave-uniform.  An ordinal becomes its source state through the arcs' sources,
//                      held in LDS on the same condition, and only at the frames where the path changes state.  Frame
//                      t's label is its state with one more bit that flips wherever a run opens, so two neighbouring
//                      labels differ exactly there, also for two runs of one state.
//   viterbi_runs       one wave per utterance: decode_runs' run compression (open_runs) on that label row, then the
//                      states and their phonemes.
// align_score then scores the runs as a transcript of `runs` phonemes among at most `frames`.

constexpr int VSTATES = PPG_VITERBI_MAX_STATES;
constexpr int VLEAD = 2;                      // arcs per state taken in lock step over a lane's slots
constexpr int VAHEAD = 8;                     // arcs of a state read ahead of their compares, past its first six
constexpr int VHELD = 4096;                   // arcs of a graph the programme keeps in LDS (32 KiB) at most
constexpr int VROWS_VEC = 1024;               // 16-byte pieces per refill of the trace-back: 16 KiB
constexpr int VPARITY = 1 << 16;              // the bit of a label that flips where a run opens
static_assert(VSTATES % 256 == 0 && VSTATES <= VPARITY, "a label holds a state below its parity bit");
static_assert(PPG_VITERBI_MAX_ARCS <= 1 << 15 && PPG_VITERBI_MAX_DEGREE == 255, "16 bits of arc index, 8 of degree");

struct ViterbiLayout {
    size_t logp, back, labels, ends, verdict, bytes;           // byte offsets into the workspace
};

// back-pointer bytes of one frame, a byte per state: whole passes of the programme over the call's largest graph
__host__ __device__ inline int viterbi_row(int max_states) { return max_states <= 64 ? 64 : (max_states + 255) & ~255; }

// back-pointer bytes of one utterance
__host__ __device__ inline size_t viterbi_back_bytes(int frames, int max_states) {
    return (size_t)frames * viterbi_row(max_states);
}

// (65535 items of 262144 frames and 1024 states are 1.8e13 bytes: inside a size_t)
inline ViterbiLayout viterbi_layout(int items, int frames, int max_states) {
    ViterbiLayout w{};
    size_t at = 0;
    w.logp = at; at += prepared_bytes(items, frames);
    w.back = at; at = align256(at + (size_t)items * viterbi_back_bytes(frames, max_states));
    w.labels = at; at = align256(at + (size_t)items * frames * sizeof(int));
    w.ends = at; at = align256(at + (size_t)items * sizeof(int));
    w.verdict = at; at = align256(at + (size_t)PPG_VITERBI_MAX_GRAPHS * sizeof(int));
    w.bytes = at;
    return w;
}

// a weight is finite or -inf
__device__ __forceinline__ bool bad_weight(float w) { return w != w || w == INFINITY; }

// grid (graphs), 64 threads: lane = state of the current 64.  Every test stands before the read that depends on it.
__global__ __launch_bounds__(64) void viterbi_check(int n_states, int n_arcs, int max_states,
                                                     const int* __restrict__ state_begin,
                                                     const int* __restrict__ phonemes, const float* __restrict__ stay,
                                                     const float* __restrict__ initial,
                                                     const float* __restrict__ final_,
                                                     const int* __restrict__ arc_begin,
                                                     const int* __restrict__ sources,
                                                     const float* __restrict__ weights, int* __restrict__ verdict)
{
    const int g = blockIdx.x, lane = threadIdx.x;
    const int first = state_begin[g], end = state_begin[g + 1];
    bool fine = first >= 0 && end <= n_states && first < end && end - first <= max_states;
    if (fine) {                                                // (uniform)
        const int S = end - first;
        bool bad = false;
        for (int n = first + lane; n < end; n += 64) {
            const int a0 = arc_begin[n], a1 = arc_begin[n + 1];    // (n + 1 <= n_states: the array has that entry)
            bool wrong = a0 < 0 || a1 > n_arcs || a1 < a0 || a1 - a0 > PPG_VITERBI_MAX_DEGREE ||
                         bad_symbol(phonemes[n]) || bad_weight(stay[n]) || bad_weight(initial[n]) ||
                         bad_weight(final_[n]);
            if (!wrong)
                for (int j = a0; j < a1; ++j) wrong |= (unsigned)sources[j] >= (unsigned)S || bad_weight(weights[j]);
            bad |= wrong;
        }
        fine = !__any(bad);
        // (non-decreasing inside the graph and inside [0, n_arcs] by now)
        if (fine) fine = arc_begin[end] - arc_begin[first] <= PPG_VITERBI_MAX_ARCS;
    }
    if (lane == 0) verdict[g] = fine ? 1 : 0;
}

// The arcs of one graph as the programme and the trace-back read them: Held from LDS, where a piece is (source, the
// weight's bits), else from the caller's arrays.  `i` counts from the graph's first arc.
template <bool Held>
struct ViterbiArcs {
    const uint2* held; const int* sources; const float* weights; int count;
    __device__ __forceinline__ void get(int i, int& source, float& weight) const {
        if (Held) {
            const uint2 piece = held[i];
            source = (int)piece.x; weight = __uint_as_float(piece.y);
        } else {
            source = sources[i]; weight = weights[i];
        }
    }
};

// What the programme keeps of a state in LDS: `meta`, the first arc (counted from the graph's first, 16 bits), the
// degree (8 bits) and the phoneme (above bit 24) in one word, and the weight of staying.
struct ViterbiTable {
    int meta[VSTATES];
    float stay[VSTATES];
};
__device__ __forceinline__ int first_arc(int meta) { return meta & 0xffff; }
__device__ __forceinline__ int degree_of(int meta) { return (meta >> 16) & 0xff; }

// Frame t of G neighbouring states n0 .. n0 + G - 1 of one lane: their D from `before` (frame t-1) into `now`, their
// back-pointers into `row`, the frame's G bytes at n0.  `e` is the prepared frame.  G = 4 moves every per-state word
// as one 16-byte piece.  A lane may diverge inside; call it from wave-uniform control flow.
// `along` is told every state's `meta` and `from` once they stand: the live programme carries its ancestors there.
struct ViterbiAlone {
    template <int G>
    __device__ __forceinline__ void operator()(int, const int (&)[G], const int (&)[G]) const {}
};

template <int G, bool Held, class Along = ViterbiAlone>
__device__ __forceinline__ void viterbi_states(int t, int n0, int S, const float* __restrict__ e,
                                               const ViterbiTable& table, const float* __restrict__ initial,
                                               const ViterbiArcs<Held>& arcs, const float* __restrict__ before,
                                               float* __restrict__ now, uint8_t* __restrict__ row,
                                               const Along& along = Along())
{
    static_assert(G == 1 || G == 4, "a byte or a dword of back-pointers");
    int meta[G], from[G];
    float own[G], d[G], best[G];
    if constexpr (G == 4) {
        const int4 m = *reinterpret_cast<const int4*>(table.meta + n0);
        const float4 o = *reinterpret_cast<const float4*>(table.stay + n0);
        const float4 b = *reinterpret_cast<const float4*>(before + n0);
        meta[0] = m.x; meta[1] = m.y; meta[2] = m.z; meta[3] = m.w;
        own[0] = o.x; own[1] = o.y; own[2] = o.z; own[3] = o.w;
        d[0] = b.x; d[1] = b.y; d[2] = b.z; d[3] = b.w;
    } else {
        meta[0] = table.meta[n0]; own[0] = table.stay[n0]; d[0] = before[n0];
    }
    float cur[G];
#pragma unroll
    for (int k = 0; k < G; ++k) {
        cur[k] = e[meta[k] >> 24];
        from[k] = 0;
    }
    if (t == 0) {                                              // (uniform)
#pragma unroll
        for (int k = 0; k < G; ++k) d[k] = cur[k] + (n0 + k < S ? initial[n0 + k] : -INFINITY);
    } else {
#pragma unroll
        for (int k = 0; k < G; ++k) best[k] = d[k] + own[k];   // staying: what an arc has to beat
        if (arcs.count > 0) {                                  // (uniform) arc 0 stands in where a state has none
#pragma unroll
            for (int j = 0; j < VLEAD; ++j) {                  // the first arcs of the G states in lock step
                int p[G]; float w[G];
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    const bool there = j < degree_of(meta[k]);
                    arcs.get(there ? first_arc(meta[k]) + j : 0, p[k], w[k]);
                    w[k] = there ? w[k] : -INFINITY;           // no such arc: -inf is never better
                }
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    const float c = before[p[k]] + w[k];       // -inf + finite = -inf: never NaN
                    const bool better = c > best[k];
                    best[k] = better ? c : best[k];
                    from[k] = better ? j + 1 : from[k];
                }
            }
#pragma unroll
            for (int k = 0; k < G; ++k) {                      // what lies beyond: state by state, in list order
                const int at = first_arc(meta[k]), degree = degree_of(meta[k]);
                auto batch = [&]<int N>(int j0) {              // arcs j0 .. j0 + N - 1, the loads ahead of the compares
                    int p[N]; float w[N];
#pragma unroll
                    for (int u = 0; u < N; ++u)                // (past the last arc the last one again: never better)
                        arcs.get(at + min(j0 + u, degree - 1), p[u], w[u]);
#pragma unroll
                    for (int u = 0; u < N; ++u) {
                        const float c = before[p[u]] + w[u];
                        const bool better = c > best[k];
                        best[k] = better ? c : best[k];
                        from[k] = better ? j0 + u + 1 : from[k];
                    }
                };
                // four first (a state of a sausage has three or four arcs), then VAHEAD at a time
                if (degree > VLEAD) batch.template operator()<4>(VLEAD);
                for (int j0 = VLEAD + 4; j0 < degree; j0 += VAHEAD) batch.template operator()<VAHEAD>(j0);
            }
        }
#pragma unroll
        for (int k = 0; k < G; ++k) d[k] = cur[k] + best[k];
    }
    along(n0, meta, from);
    if constexpr (G == 4) {
        *reinterpret_cast<float4*>(now + n0) = make_float4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<uint32_t*>(row + n0) =
            (uint32_t)from[0] | (uint32_t)from[1] << 8 | (uint32_t)from[2] << 16 | (uint32_t)from[3] << 24;
    } else {
        now[n0] = d[0];
        row[n0] = (uint8_t)from[0];
    }
}

// grid (items), 64 threads, `held` * 8 bytes of dynamic LDS.  G states per lane and pass: 1 if the call's graphs have
// at most 64 states (a pass is 64 states), else 4 (a pass is 256 states; a graph takes ceil(S / 256) passes per frame).
// `row` = viterbi_row(max_states) back-pointer bytes per frame.  An utterance whose length is impossible, whose `which`
// names no graph or whose graph was refused gets total = NaN and runs = 0, one without a path total = -inf and runs =
// 0; every other its total, its end state in `ends` and its back-pointers.
template <int G>
__global__ __launch_bounds__(64) void viterbi_programme(const float* __restrict__ logp, int frames,
                                                         const int* __restrict__ lengths, int graphs,
                                                         const int* __restrict__ which,
                                                         const int* __restrict__ verdict,
                                                         const int* __restrict__ state_begin,
                                                         const int* __restrict__ phonemes,
                                                         const float* __restrict__ stay,
                                                         const float* __restrict__ initial,
                                                         const float* __restrict__ final_,
                                                         const int* __restrict__ arc_begin,
                                                         const int* __restrict__ sources,
                                                         const float* __restrict__ weights, int held, int row,
                                                         uint8_t* __restrict__ back, int* __restrict__ ends,
                                                         int* __restrict__ runs, float* __restrict__ total)
{
    __shared__ float4 stage[2][CHUNK_VEC];
    __shared__ __attribute__((aligned(16))) float dist[2][VSTATES];
    __shared__ __attribute__((aligned(16))) ViterbiTable table;
    extern __shared__ uint2 held_arcs[];
    const int item = blockIdx.x, lane = threadIdx.x;
    const int T = lengths[item], g = which ? which[item] : 0;
    bool fine = T >= 1 && T <= frames && (unsigned)g < (unsigned)graphs;
    if (fine) fine = verdict[g] != 0;                          // (then S <= max_states <= row)
    if (!fine) {                                               // (uniform)
        if (lane == 0) { total[item] = NAN; runs[item] = 0; }
        return;
    }
    const int first = state_begin[g], S = state_begin[g + 1] - first;
    const int* begin = arc_begin + first;
    const int arc0 = begin[0], count = begin[S] - arc0;
    const int covered = (S + 64 * G - 1) / (64 * G) * (64 * G);    // whole passes: <= row <= VSTATES
    for (int n = lane; n < covered; n += 64) {
        const bool state = n < S;
        // states at or above S run along on phoneme 0 without arcs, at -inf, unread
        table.meta[n] = state ? (begin[n] - arc0) | (begin[n + 1] - begin[n]) << 16 | phonemes[first + n] << 24 : 0;
        table.stay[n] = state ? stay[first + n] : -INFINITY;
        dist[1][n] = -INFINITY;                                // what frame 0 reads as D of the frame before: unused
    }
    const bool keep = count <= held;                           // (uniform)
    if (keep)
        for (int i = lane; i < count; i += 64)
            held_arcs[i] = make_uint2((uint32_t)sources[arc0 + i], __float_as_uint(weights[arc0 + i]));
    const float4* src = reinterpret_cast<const float4*>(logp + (size_t)item * frames * PREP);
    uint8_t* out = back + (size_t)item * frames * row;
    const ViterbiArcs<true> in_lds{held_arcs, nullptr, nullptr, count};
    const ViterbiArcs<false> in_memory{nullptr, sources + arc0, weights + arc0, count};
    // the frame walk of WALK_FRAMES: the prepared frames through LDS CHUNK at a time, the next chunk in flight
    float4 next[FETCH];
    fetch(src, 0, T, lane, next);
    stash(stage[0], lane, next);
    __syncthreads();
    int buf = 0;
    for (int t0 = 0; t0 < T; t0 += CHUNK, buf ^= 1) {
        fetch(src, t0 + CHUNK, T, lane, next);
        const float* e = reinterpret_cast<const float*>(stage[buf]);
        const int chunk = min(CHUNK, T - t0);
        for (int u = 0; u < chunk; ++u) {
            const int t = t0 + u;
            for (int n0 = lane * G; n0 < covered; n0 += 64 * G) {  // (uniform: every lane takes every pass)
                if (keep) viterbi_states<G, true>(t, n0, S, e + u * PREP, table, initial + first, in_lds,
                                                  dist[(t & 1) ^ 1], dist[t & 1], out + (size_t)t * row);
                else viterbi_states<G, false>(t, n0, S, e + u * PREP, table, initial + first, in_memory,
                                              dist[(t & 1) ^ 1], dist[t & 1], out + (size_t)t * row);
            }
            __syncthreads();                                   // frame t+1 reads what this frame wrote
        }
        stash(stage[buf ^ 1], lane, next);                     // its readers passed the barrier above
        __syncthreads();
    }
    // the first of the largest F: ascending n inside a lane, then the lower state of equal values across lanes
    const float* last = dist[(T - 1) & 1];
    float most = -INFINITY;
    int end = VSTATES;
    for (int n = lane; n < S; n += 64) {
        const float f = last[n] + final_[first + n];
        if (f > most || end == VSTATES) { most = f; end = n; }
    }
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) {
        const float other = __shfl_xor(most, step);
        const int state = __shfl_xor(end, step);
        const bool better = other > most || (other == most && state < end);
        most = better ? other : most;
        end = better ? state : end;
    }
    if (lane == 0) {
        total[item] = most;
        if (most > -INFINITY) ends[item] = end;
        else runs[item] = 0;                                   // no path: nothing else is written
    }
}

// grid (items), 64 threads, `held` * 4 bytes of dynamic LDS; `row` = viterbi_row(max_states) back-pointer bytes per frame
__global__ __launch_bounds__(64) void viterbi_traceback(const uint8_t* __restrict__ back, int frames,
                                                         const int* __restrict__ lengths,
                                                         const int* __restrict__ which,
                                                         const int* __restrict__ state_begin,
                                                         const int* __restrict__ arc_begin,
                                                         const int* __restrict__ sources, int held, int row,
                                                         const float* __restrict__ total,
                                                         const int* __restrict__ ends, int* __restrict__ labels)
{
    __shared__ uint4 rows[VROWS_VEC];
    extern __shared__ int held_sources[];
    const int item = blockIdx.x, lane = threadIdx.x;
    const int T = lengths[item];
    if (!recognized(T, frames, total + item)) return;          // (uniform) so `which` and the graph are fine
    const int g = which ? which[item] : 0;
    const int first = state_begin[g], S = state_begin[g + 1] - first;
    const int* begin = arc_begin + first;
    const int arc0 = begin[0], count = begin[S] - arc0;
    const bool keep = count <= held;                           // (uniform)
    if (keep)
        for (int i = lane; i < count; i += 64) held_sources[i] = sources[arc0 + i];   // (the loop's barriers follow)
    // what the programme wrote of a row: the graph's own passes, not the call's largest graph's.  Only that is read.
    const int covered = row == 64 ? 64 : (S + 255) & ~255;     // <= row
    const int per = covered / 16;                              // 16-byte pieces per frame: 4, 16, 32, 48 or 64
    const int span = VROWS_VEC / per;                          // frames per refill: 256, 64, 32, 21 or 16
    const uint4* src = reinterpret_cast<const uint4*>(back + (size_t)item * frames * row);
    int* out = labels + (size_t)item * frames;
    constexpr int PER = VROWS_VEC / 64;
    uint4 next[PER];
    auto load = [&](int c) {                                   // rows of frames c * span ..., those below T only
        const int pieces = min(span, T - c * span) * per;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int idx = u * 64 + lane, frame = idx / per;  // (the refill stands frame by frame, `covered` bytes each)
            next[u] = idx < pieces ? src[(size_t)(c * span + frame) * (row / 16) + idx - frame * per]
                                   : make_uint4(0, 0, 0, 0);
        }
    };
    int n = min(max(ends[item], 0), S - 1);
    int parity = 0;
    int c = (T - 1) / span;
    load(c);
    for (; c >= 0; --c) {
        __syncthreads();                                       // the walk over the previous refill is over
#pragma unroll
        for (int u = 0; u < PER; ++u) rows[u * 64 + lane] = next[u];
        __syncthreads();
        if (c > 0) load(c - 1);
        const uint8_t* bytes = reinterpret_cast<const uint8_t*>(rows);
        for (int t = min(T - 1, c * span + span - 1); t >= c * span; --t) {
            if (lane == 0) out[t] = n | parity;                // frame t's label
            // frame t's ordinal: the same address in every lane (frame 0 has no predecessor; its byte is 0)
            const int from = t > 0 ? bytes[(t - c * span) * covered + n] : 0;
            if (from) {                                        // (uniform) a run opens here: through in-arc from - 1
                const int arc = begin[n] - arc0 + from - 1;
                n = min(max(keep ? held_sources[arc] : sources[arc0 + arc], 0), S - 1);
                parity ^= VPARITY;
            }
        }
    }
}

// grid (items), 64 threads: lane = frame of the current 64
__global__ __launch_bounds__(64) void viterbi_runs(const int* __restrict__ labels, int frames,
                                                    const int* __restrict__ lengths, const int* __restrict__ which,
                                                    const int* __restrict__ state_begin,
                                                    const int* __restrict__ state_phonemes,
                                                    const float* __restrict__ total, int* __restrict__ states,
                                                    int* __restrict__ phonemes, int* __restrict__ starts,
                                                    int* __restrict__ runs)
{
    const int item = blockIdx.x, lane = threadIdx.x;
    const int T = lengths[item];
    if (!recognized(T, frames, total + item)) return;          // (uniform) the programme has set runs = 0
    const int* sym = state_phonemes + state_begin[which ? which[item] : 0];
    const int* src = labels + (size_t)item * frames;
    int* out_states = states + (size_t)item * frames;
    int* out_phonemes = phonemes + (size_t)item * frames;
    int* out_starts = starts + (size_t)item * (frames + 1);
    int carry = -1, base = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        open_runs(t < T ? src[t] : -2, t, T, lane, carry, base, out_states, out_starts);
    }
    if (lane == 0) { runs[item] = base; out_starts[base] = T; }
    __syncthreads();                                           // the labels of the runs are written
    for (int r = lane; r < base; r += 64) {                    // a run's label without its parity bit is its state
        const int state = out_states[r] & (VPARITY - 1);
        out_states[r] = state;
        out_phonemes[r] = sym[state];
    }
}

// ---- live Viterbi over a phoneme graph (ppg_viterbi_stream_*) ----
//
// ppg_viterbi carried across the pushes of a stream, under the stream rules of the live recogniser above with a state n
// of the stream's graph wherever that text has a phoneme q: position p, commit point c, D of frame p-1, a ring of W
// frames (slot t % W) with the back-pointer rows (one byte per state, the ordinal `from`), the prepared frames and the
// labels of the frames in [c, p), one open run, the counter `forced`, and the graph the stream was opened with.
//   Forward: viterbi_states, the body of viterbi_programme, with the absolute frame: D and the back-pointer byte of every
//   frame and state are the bits viterbi_programme computes for the whole recording, whatever the pushes.
//   Commit: natural and forced as above.  A committed frame opens a run if it is absolute frame 0 or its back-pointer
//   byte at its state is not 0; a closed run is emitted as (state, phoneme, begin, end, score, gop).
// The caller owns the state: seven blocks, each 256-byte aligned: the heads (8 words), D (viterbi_row(max_states) words
// per stream), the ancestors (as many 16-bit words: anc[n] = path(n, c)), the back-pointer rings (W rows of
// viterbi_row(max_states) bytes), the rings of prepared frames (176 B per frame) and of labels (int32), and one verdict
// per graph (room for as many graphs as streams).  ppg_viterbi_stream_open runs viterbi_check once and records every
// stream's graph, -1 for a graph that was refused or is not there; such a stream answers -1 to every push.  Push and
// flush read the graph arrays again and trust them as the verdict allows; a source read from them is clamped into
// [0, S) wherever these kernels index with it themselves.  One wave per stream:
//   viterbi_stream_programme  copies the push's prepared frames into the ring, loads D and the ancestors into LDS, runs
//                             viterbi_states per frame and pass, which hands `from` to ViterbiAncestors: anc[n] = n at
//                             frame c, else anc[n] where from = 0, else anc[source of in-arc from - 1], in two more LDS
//                             buffers of 1024 x 16 bits.
//   viterbi_stream_commit     a ballot over the alive states' ancestors: if they differ and nothing has to be forced,
//                             nothing can be committed.  Else the SET of the alive paths' states is walked back from t,
//                             flags in LDS, every lane mapping its states of the set to their predecessors, until the
//                             set is one state: that frame is v.  One wave-uniform walk as in viterbi_traceback, from
//                             that state at v or from the best state at t if a commit is forced, writes the labels: the
//                             state and one more bit where a run opens.  If c moved, a forward pass over the frames
//                             (new c, t] gives every state's ancestor at the new c for the next push, and in the forced
//                             case, through one more look-up at frame p-L, the states whose path left the one given
//                             out: their D becomes -inf.  Then the run pass of the live recogniser on the new labels:
//                             lane = frame, a ballot of the frames that open a run, the sums in frame order.
//                             Back-pointer rows come through LDS 16 KiB at a time, the next refill in flight, and of a
//                             row only the graph's own passes.
//   viterbi_stream_advance, viterbi_stream_flush, viterbi_stream_reset (which also opens) as their namesakes above.

struct ViterbiHead {
    int position, commit, forced;
    int label, start;                         // the open run: its state, -1: none
    float sum, below;
    int graph;                                // the stream's graph; -1: refused or missing when the stream was opened
};
static_assert(sizeof(ViterbiHead) == HEAD * 4, "the head is 8 words");

struct ViterbiStreamLayout {
    size_t heads, d, anc, back, kept, labels, verdict, bytes;      // byte offsets into the state
};

// (65535 streams of 65536 frames and 1024 states are 5.2e12 bytes: inside a size_t)
inline ViterbiStreamLayout viterbi_stream_layout(int streams, int window, int max_states) {
    ViterbiStreamLayout w{};
    const size_t row = (size_t)viterbi_row(max_states), slots = (size_t)streams * window;
    size_t at = 0;
    w.heads = at; at = align256(at + (size_t)streams * sizeof(ViterbiHead));
    w.d = at; at = align256(at + (size_t)streams * row * sizeof(float));
    w.anc = at; at = align256(at + (size_t)streams * row * sizeof(uint16_t));
    w.back = at; at = align256(at + slots * row);
    w.kept = at; at = align256(at + slots * PREP * sizeof(float));
    w.labels = at; at = align256(at + slots * sizeof(int));
    w.verdict = at; at = align256(at + (size_t)streams * sizeof(int));
    w.bytes = at;
    return w;
}

// what a stream may be asked to take; everything else gets count = -1 and touches nothing
__device__ __forceinline__ bool viterbi_pushable(const ViterbiHead& head, int T, int frames, int window) {
    return head.graph >= 0 && pushable(T, frames, head.position, head.commit, window);
}

// The graph of a stream as the live kernels take it from the caller's arrays: S inside [1, row] whatever they hold.
struct ViterbiGraph {
    int first, S, arc0, count;
    const int* begin;                         // arc_begin of the graph's state 0
};
__device__ __forceinline__ ViterbiGraph graph_of(int g, int row, const int* __restrict__ state_begin,
                                                 const int* __restrict__ arc_begin) {
    ViterbiGraph out;
    out.first = state_begin[g];
    out.S = min(max(state_begin[g + 1] - out.first, 1), row);
    out.begin = arc_begin + out.first;
    out.arc0 = out.begin[0];
    out.count = out.begin[out.S] - out.arc0;
    return out;
}

// What viterbi_states tells the live programme at every frame: the ancestors at the commit point move along `from`.
template <bool Held>
struct ViterbiAncestors {
    const ViterbiArcs<Held>& arcs;
    const uint16_t* before; uint16_t* now;    // anc of frame t-1 and of frame t (LDS)
    bool fresh; int S;                        // frame t is the commit point: every state is its own ancestor
    template <int G>
    __device__ __forceinline__ void operator()(int n0, const int (&meta)[G], const int (&from)[G]) const {
        uint16_t a[G];
#pragma unroll
        for (int k = 0; k < G; ++k) {
            int source = n0 + k;
            if (from[k]) {
                float weight;
                arcs.get(first_arc(meta[k]) + from[k] - 1, source, weight);
                source = min(max(source, 0), S - 1);
            }
            a[k] = fresh ? (uint16_t)(n0 + k) : before[source];
        }
        if constexpr (G == 4) {
            *reinterpret_cast<uint2*>(now + n0) = make_uint2((uint32_t)a[0] | (uint32_t)a[1] << 16,
                                                             (uint32_t)a[2] | (uint32_t)a[3] << 16);
        } else {
            now[n0] = a[0];
        }
    }
};

// grid (streams), 64 threads, `held` * 8 bytes of dynamic LDS; G and `row` as for viterbi_programme
template <int G>
__global__ __launch_bounds__(64) void viterbi_stream_programme(const float* __restrict__ logp, int frames,
                                                                const int* __restrict__ lengths, int window,
                                                                const ViterbiHead* __restrict__ heads,
                                                                const int* __restrict__ state_begin,
                                                                const int* __restrict__ phonemes,
                                                                const float* __restrict__ stay,
                                                                const float* __restrict__ initial,
                                                                const int* __restrict__ arc_begin,
                                                                const int* __restrict__ sources,
                                                                const float* __restrict__ weights, int held, int row,
                                                                float* __restrict__ state_d,
                                                                uint16_t* __restrict__ state_anc,
                                                                uint8_t* __restrict__ back, float4* __restrict__ kept)
{
    __shared__ float4 stage[2][CHUNK_VEC];
    __shared__ __attribute__((aligned(16))) float dist[2][VSTATES];
    __shared__ __attribute__((aligned(16))) ViterbiTable table;
    __shared__ __attribute__((aligned(16))) uint16_t anc[2][VSTATES];
    extern __shared__ uint2 held_arcs[];
    const int item = blockIdx.x, lane = threadIdx.x;
    const ViterbiHead head = heads[item];
    const int T = lengths[item], p = head.position, c = head.commit;
    if (!viterbi_pushable(head, T, frames, window) || T == 0) return;  // (uniform) refused, or it sits out the step
    const float4* src = reinterpret_cast<const float4*>(logp + (size_t)item * frames * PREP);
    float4* ring = kept + (size_t)item * window * PREP_VEC;
    const int slot0 = p % window;
    for (int idx = lane; idx < T * PREP_VEC; idx += 64) {      // T <= window: a slot wraps once at most
        int slot = slot0 + idx / PREP_VEC;
        slot = slot >= window ? slot - window : slot;
        ring[(size_t)slot * PREP_VEC + idx % PREP_VEC] = src[idx];
    }
    const ViterbiGraph graph = graph_of(head.graph, row, state_begin, arc_begin);
    const int first = graph.first, S = graph.S, arc0 = graph.arc0, count = graph.count;
    const int covered = (S + 64 * G - 1) / (64 * G) * (64 * G);    // whole passes: <= row <= VSTATES
    float* live_d = state_d + (size_t)item * row;
    uint16_t* live_anc = state_anc + (size_t)item * row;
    for (int n = lane; n < covered; n += 64) {
        const bool state = n < S;
        table.meta[n] = state ? (graph.begin[n] - arc0) | (graph.begin[n + 1] - graph.begin[n]) << 16 |
                                phonemes[first + n] << 24 : 0;
        table.stay[n] = state ? stay[first + n] : -INFINITY;
        dist[(p & 1) ^ 1][n] = live_d[n];                      // D of frame p-1 (-inf at p = 0, and unused there)
        anc[(p & 1) ^ 1][n] = live_anc[n];
    }
    const bool keep = count <= held;                           // (uniform)
    if (keep)
        for (int i = lane; i < count; i += 64)
            held_arcs[i] = make_uint2((uint32_t)min(max(sources[arc0 + i], 0), S - 1),
                                      __float_as_uint(weights[arc0 + i]));
    uint8_t* out = back + (size_t)item * window * row;
    const ViterbiArcs<true> in_lds{held_arcs, nullptr, nullptr, count};
    const ViterbiArcs<false> in_memory{nullptr, sources + arc0, weights + arc0, count};
    float4 next[FETCH];
    fetch(src, 0, T, lane, next);
    stash(stage[0], lane, next);
    __syncthreads();
    int buf = 0, slot = slot0;
    for (int t0 = 0; t0 < T; t0 += CHUNK, buf ^= 1) {
        fetch(src, t0 + CHUNK, T, lane, next);
        const float* e = reinterpret_cast<const float*>(stage[buf]);
        const int chunk = min(CHUNK, T - t0);
        for (int u = 0; u < chunk; ++u) {
            const int t = p + t0 + u;                          // the absolute frame
            uint8_t* bytes = out + (size_t)slot * row;
            for (int n0 = lane * G; n0 < covered; n0 += 64 * G) {  // (uniform: every lane takes every pass)
                if (keep)
                    viterbi_states<G, true>(t, n0, S, e + u * PREP, table, initial + first, in_lds, dist[(t & 1) ^ 1],
                                            dist[t & 1], bytes,
                                            ViterbiAncestors<true>{in_lds, anc[(t & 1) ^ 1], anc[t & 1], t == c, S});
                else
                    viterbi_states<G, false>(t, n0, S, e + u * PREP, table, initial + first, in_memory,
                                             dist[(t & 1) ^ 1], dist[t & 1], bytes,
                                             ViterbiAncestors<false>{in_memory, anc[(t & 1) ^ 1], anc[t & 1], t == c, S});
            }
            slot = slot + 1 == window ? 0 : slot + 1;
            __syncthreads();                                   // frame t+1 reads what this frame wrote
        }
        stash(stage[buf ^ 1], lane, next);                     // its readers passed the barrier above
        __syncthreads();
    }
    const int last = (p + T - 1) & 1;
    for (int n = lane; n < covered; n += 64) {
        live_d[n] = dist[last][n];
        live_anc[n] = anc[last][n];
    }
}

// A wave-uniform pointer kept in vector registers: the commit and the flush run out of scalar registers, and these
// pointers are only ever the address of a vector load or store.
template <class T>
__device__ __forceinline__ T* in_vector_registers(T* pointer) {
    asm volatile("" : "+v"(pointer));
    return pointer;
}

// a pointer known to point into LDS: 32 bits, no flat access.  (As a flat pointer in a struct it drew "Illegal
// instruction detected: Operand has incorrect register class" from the compiler for these kernels.)
#define PPG_LDS __attribute__((address_space(3)))

// What the commit and the flush of one stream share: the graph's arcs for turning an ordinal into its source state,
// and the stream's ring of back-pointer rows, of which a refill of VROWS_VEC pieces holds `span` frames, the graph's
// own `covered` bytes of each.
constexpr int VPER = VROWS_VEC / 64;          // pieces of a refill per lane
struct ViterbiLive {
    int lane, S, covered, count, arc0;
    bool keep;
    const PPG_LDS uint16_t* first;            // a state's first arc, counted from the graph's first
    const PPG_LDS int* held_sources;          // the arcs' sources, clamped, if keep
    const int* sources;
    const uint8_t* back;                      // the stream's ring
    int window, row, per, span;
    int frame[VPER];                          // the frame of a refill this lane's piece u lies in: (u * 64 + lane) / per

    // the state in-arc from - 1 of state n comes from: inside [0, S) whatever the arrays hold
    __device__ __forceinline__ int source_of(int n, int from) const {
        if (count <= 0) return n;
        const int arc = min((int)first[n] + from - 1, count - 1);
        return min(max(keep ? held_sources[arc] : sources[arc0 + arc], 0), S - 1);
    }
    __device__ __forceinline__ int before(int n, int from) const { return from ? source_of(n, from) : n; }

    // the rows of the frames chunk * span ..., those in [low, high] only
    __device__ __forceinline__ void load(int chunk, int low, int high, uint4 (&next)[VPER]) const {
        const uint4* src = reinterpret_cast<const uint4*>(back);
        const int base = chunk * span, start = base % window;
#pragma unroll
        for (int u = 0; u < VPER; ++u) {
            // (relative to the refill's first frame: a position may be INT32_MAX; span <= window: a slot wraps once)
            const int at = frame[u];
            int slot = start + at;
            slot = slot >= window ? slot - window : slot;
            next[u] = at < span && at >= low - base && at <= high - base
                          ? src[(size_t)slot * (row / 16) + u * 64 + lane - at * per] : make_uint4(0, 0, 0, 0);
        }
    }

    // body(u, the bytes of frame u's row) for the frames from `start` to `stop`, descending if Down, until it returns
    // false.  The refills go through `rows`, the next one in flight.  Wave-uniform: so must the body's answer be.
    template <bool Down, class Body>
    __device__ __forceinline__ void walk(int start, int stop, uint4 (&rows)[VROWS_VEC], Body&& body) const {
        if (Down ? start < stop : start > stop) return;        // (uniform)
        const int low = Down ? stop : start, high = Down ? start : stop;
        uint4 next[VPER];
        int chunk = start / span;
        const int last = stop / span;
        load(chunk, low, high, next);
        bool go = true;
        while (go) {
            __syncthreads();                                   // the walk over the previous refill is over
#pragma unroll
            for (int u = 0; u < VPER; ++u) rows[u * 64 + lane] = next[u];
            __syncthreads();
            const bool more = chunk != last;
            if (more) load(Down ? chunk - 1 : chunk + 1, low, high, next);
            const PPG_LDS uint8_t* bytes = (const PPG_LDS uint8_t*)rows;
            const int base = chunk * span;
            const int bottom = max(low - base, 0), top = min(high - base, span - 1);
            if (Down) {
                for (int r = top; go && r >= bottom; --r) go = body(base + r, bytes + r * covered);
            } else {
                for (int r = bottom; go && r <= top; ++r) go = body(base + r, bytes + r * covered);
            }
            if (!more) break;
            chunk += Down ? -1 : 1;
        }
        __syncthreads();
    }

    // the labels of the frames [c, fresh) along the path that is in state n at frame `top` >= fresh - 1: the state and
    // VPARITY where the frame opens a run.  Returns the path's state at frame fresh - 1.  Lane 0 writes.
    __device__ __forceinline__ int label(int n, int top, int c, int fresh, int* __restrict__ labels,
                                         uint4 (&rows)[VROWS_VEC]) const {
        int goal = n;
        walk<true>(top, c, rows, [&](int u, const PPG_LDS uint8_t* bytes) __attribute__((always_inline)) {
            const int from = bytes[n];                         // the same address in every lane (frame 0's byte is 0)
            if (u < fresh && lane == 0) labels[u % window] = n | (from || u == 0 ? VPARITY : 0);
            if (u == fresh - 1) goal = n;
            if (u > c) n = before(n, from);
            return true;
        });
        return goal;
    }
};

// fills `live` and the LDS tables it points to; a barrier must follow before they are read
__device__ __forceinline__ ViterbiLive live_of(const ViterbiGraph& graph, const int* __restrict__ sources, int held,
                                               int row, int window, const uint8_t* back, PPG_LDS uint16_t* first,
                                               PPG_LDS int* held_sources, int lane) {
    ViterbiLive live;
    live.lane = lane; live.S = graph.S; live.count = graph.count; live.arc0 = graph.arc0;
    live.covered = row == 64 ? 64 : (graph.S + 255) & ~255;    // what the programme wrote of a row: <= row
    live.keep = graph.count <= held;
    live.first = first; live.held_sources = held_sources; live.sources = in_vector_registers(sources);
    live.back = in_vector_registers(back); live.window = window; live.row = row;
    live.per = live.covered / 16;
    live.span = min(VROWS_VEC / live.per, window);             // (no more than `window` frames are ever open)
#pragma unroll
    for (int u = 0; u < VPER; ++u) live.frame[u] = (u * 64 + lane) / live.per;
    for (int n = lane; n < live.covered; n += 64)
        first[n] = (uint16_t)(n < graph.S ? min(max(graph.begin[n] - graph.arc0, 0), VPARITY - 1) : 0);
    if (live.keep)
        for (int i = lane; i < graph.count; i += 64)
            held_sources[i] = min(max(sources[graph.arc0 + i], 0), graph.S - 1);
    return live;
}

// the first of the largest of value(n), n < S (strict >, ascending), wave-uniform: its state; *most is its value
template <class Value>
__device__ __forceinline__ int first_largest_state(int S, int lane, float* most, Value&& value) {
    float sum = -INFINITY;
    int end = VSTATES;
    for (int n = lane; n < S; n += 64) {
        const float f = value(n);
        if (f > sum || end == VSTATES) { sum = f; end = n; }
    }
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) {
        const float other = __shfl_xor(sum, step);
        const int state = __shfl_xor(end, step);
        const bool better = other > sum || (other == sum && state < end);
        sum = better ? other : sum;
        end = better ? state : end;
    }
    *most = sum;
    return end;
}

// The run outputs of one stream's push or flush, as `Runs` with the states beside the phonemes.
struct StateRuns {
    int* states; int* phonemes; int* begin; int* end; float* score; float* gop;    // `cap` slots; gop may be null
    int cap, count;
};

__device__ __forceinline__ StateRuns state_runs_of(int item, int cap, int* states, int* phonemes, int* begin, int* end,
                                                   float* score, float* gop) {
    const size_t at = (size_t)item * cap;
    return StateRuns{in_vector_registers(states + at), in_vector_registers(phonemes + at),
                     in_vector_registers(begin + at), in_vector_registers(end + at), in_vector_registers(score + at),
                     gop ? in_vector_registers(gop + at) : nullptr, cap, 0};
}

// the open run ends in front of frame `end`.  Wave-uniform; lane 0 writes.
__device__ __forceinline__ void close_run(const ViterbiHead& run, int end, const int* __restrict__ sym, StateRuns& out,
                                          int lane) {
    if (lane == 0 && out.count < out.cap) {
        const float count = (float)(end - run.start);
        out.states[out.count] = run.label;
        out.phonemes[out.count] = min(max(sym[run.label], 0), NP - 1);
        out.begin[out.count] = run.start;
        out.end[out.count] = end;
        out.score[out.count] = run.sum / count;
        if (out.gop) out.gop[out.count] = run.below / count;
    }
    ++out.count;
}

// slots at or past the runs written: -1 / NaN
__device__ __forceinline__ void fill_runs(const StateRuns& out, int lane) {
    for (int h = min(out.count, out.cap) + lane; h < out.cap; h += 64) {
        out.states[h] = out.phonemes[h] = out.begin[h] = out.end[h] = -1;
        out.score[h] = NAN;
        if (out.gop) out.gop[h] = NAN;
    }
}

// The run pass over the newly committed frames c .. fresh-1, whose labels stand in the ring, 64 at a time: lane =
// frame, a ballot of the frames that open a run, the sums in frame order.  `sym` holds the phonemes of the graph's
// S states.  Leaves head.commit = fresh.  Wave-uniform.
__device__ __forceinline__ void give_runs(ViterbiHead& head, int fresh, int window, int S,
                                          const int* __restrict__ sym, const float* __restrict__ kept,
                                          const int* __restrict__ labels, StateRuns& out, int lane) {
    const int c = head.commit, count = fresh - c, slot0 = c % window;
    for (int k0 = 0; k0 < count; k0 += 64) {                   // (uniform)
        const int k = k0 + lane;
        int slot = slot0 + k;
        slot = slot >= window ? slot - window : slot;
        int state = 0;
        bool opening = false;
        float e = 0.f, top = 0.f;
        if (k < count) {
            const int label = labels[slot];
            state = min(max(label & (VPARITY - 1), 0), S - 1);
            opening = (label & VPARITY) != 0;
            e = kept[(size_t)slot * PREP + min(max(sym[state], 0), NP - 1)];
            top = kept[(size_t)slot * PREP + NP];
        }
        const float under = e - top;                           // exactly 0 where the label is the frame's maximum
        const unsigned long long opens = __ballot(opening);
        const int here = min(64, count - k0);
        for (int j = 0; j < here; ++j) {                       // in frame order: every lane keeps the same sums
            if ((opens >> j) & 1) {
                if (head.label >= 0) close_run(head, c + k0 + j, sym, out, lane);
                head.label = __builtin_amdgcn_readlane(state, j);
                head.start = c + k0 + j;
                head.sum = head.below = 0.f;
            }
            head.sum += from_lane(e, j);
            head.below += from_lane(under, j);
        }
    }
    head.commit = fresh;
}

// grid (streams), 64 threads, `held` * 4 bytes of dynamic LDS; after the programme and before the advance: the head
// still holds the old position.
__global__ __launch_bounds__(64) void viterbi_stream_commit(int frames, const int* __restrict__ lengths, int window,
                                                             int max_lag, ViterbiHead* __restrict__ heads,
                                                             const int* __restrict__ state_begin,
                                                             const int* __restrict__ state_phonemes,
                                                             const int* __restrict__ arc_begin,
                                                             const int* __restrict__ sources, int held, int row,
                                                             float* __restrict__ state_d,
                                                             uint16_t* __restrict__ state_anc,
                                                             const uint8_t* __restrict__ back,
                                                             const float* __restrict__ kept, int* __restrict__ labels,
                                                             int cap, int* __restrict__ states,
                                                             int* __restrict__ phonemes, int* __restrict__ begin,
                                                             int* __restrict__ end, float* __restrict__ score,
                                                             float* __restrict__ gop, int* __restrict__ count)
{
    __shared__ uint4 rows[VROWS_VEC];
    __shared__ uint16_t first[VSTATES];
    __shared__ uint16_t both[2][VSTATES];                      // the set of the walk back; the ancestors of the pass forward
    extern __shared__ int held_sources[];
    const int item = blockIdx.x, lane = threadIdx.x;
    const int T = lengths[item];
    ViterbiHead head = heads[item];
    if (!viterbi_pushable(head, T, frames, window)) {          // (uniform)
        if (lane == 0) count[item] = -1;
        return;
    }
    ViterbiHead* my_head = in_vector_registers(heads + item);  // what is written at the end: out of the scalar file now
    int* my_count = in_vector_registers(count + item);
    StateRuns out = state_runs_of(item, cap, states, phonemes, begin, end, score, gop);
    const float* my_kept = in_vector_registers(kept + (size_t)item * window * PREP);
    const ViterbiGraph graph = graph_of(head.graph, row, state_begin, arc_begin);
    const int* sym = in_vector_registers(state_phonemes + graph.first);
    const ViterbiLive live = live_of(graph, sources, held, row, window, back + (size_t)item * window * row,
                                     (PPG_LDS uint16_t*)first, (PPG_LDS int*)held_sources, lane);
    __syncthreads();
    const int S = graph.S, covered = live.covered;
    PPG_LDS uint16_t* const trail = (PPG_LDS uint16_t*)both;   // side s: trail[s * VSTATES + n]
    float* d = in_vector_registers(state_d + (size_t)item * row);
    uint16_t* anc = in_vector_registers(state_anc + (size_t)item * row);
    int* ring_labels = in_vector_registers(labels + (size_t)item * window);
    const int p = head.position + T, c = head.commit, t = p - 1;
    float most;
    const int best = first_largest_state(S, lane, &most, [&](int n) { return d[n]; });
    int fresh = c;
    if (most > -INFINITY && t >= c) {                          // (uniform) some state is alive and frames are open
        // the alive states' ancestors at c differ, so their paths meet nowhere in [c, t]
        const int lead = anc[best];
        bool other = false;
        for (int n = lane; n < S; n += 64) other |= d[n] > -INFINITY && anc[n] != lead;
        const bool apart = __any(other);
        const bool far = p - c > max_lag;
        if (!apart || far) {                                   // (uniform) else nothing to commit
            int v = c - 1, meet = best;
            if (!apart) {
                // the states of all alive paths at frame u, as flags: back from t until they are one state
                for (int n = lane; n < covered; n += 64) trail[n] = n < S && d[n] > -INFINITY;
                __syncthreads();
                int cur = 0;
                live.walk<true>(t, c, rows, [&](int u, const PPG_LDS uint8_t* bytes) __attribute__((always_inline)) {
                    int members = 0, one = -1;
                    for (int n0 = 0; n0 < covered; n0 += 64) {
                        const unsigned long long in = __ballot(trail[cur * VSTATES + n0 + lane] != 0);
                        members += __popcll(in);
                        if (in && one < 0) one = n0 + __ffsll(in) - 1;
                    }
                    if (members == 1) { v = u; meet = one; return false; }
                    if (u == c) return false;                  // (the ancestors said otherwise: never)
                    for (int n = lane; n < covered; n += 64) trail[(cur ^ 1) * VSTATES + n] = 0;
                    __syncthreads();
                    for (int n = lane; n < covered; n += 64)
                        if (trail[cur * VSTATES + n]) trail[(cur ^ 1) * VSTATES + live.before(n, bytes[n])] = 1;
                    __syncthreads();
                    cur ^= 1;
                    return true;
                });
            }
            const int natural = v + 1;
            const bool force = p - natural > max_lag;
            fresh = force ? p - max_lag : natural;
            if (force) head.forced += fresh - natural;
            if (fresh > c) {                                   // (uniform)
                // from the best state at t if the commit is forced, else from the state the alive paths meet in at v
                const int goal = live.label(force ? best : meet, force ? t : v, c, fresh, ring_labels, rows);
                if (fresh <= t) {
                    // every state's ancestor at the new commit point: a[n] = n there, then a[n] = a[before(n)]
                    for (int n = lane; n < covered; n += 64) trail[n] = (uint16_t)n;
                    __syncthreads();
                    int cur = 0;
                    live.walk<false>(fresh + 1, t, rows, [&](int u, const PPG_LDS uint8_t* bytes) __attribute__((always_inline)) {
                        for (int n = lane; n < covered; n += 64)
                            trail[(cur ^ 1) * VSTATES + n] = trail[cur * VSTATES + live.before(n, bytes[n])];
                        __syncthreads();
                        cur ^= 1;
                        return true;
                    });
                    const uint8_t* edge = live.back + (size_t)(fresh % window) * row;      // frame fresh's row
                    for (int n = lane; n < covered; n += 64) {
                        const int a = trail[cur * VSTATES + n];
                        anc[n] = (uint16_t)a;
                        // forced: the paths that were elsewhere at frame fresh - 1 end
                        if (force && n < S && live.before(a, edge[a]) != goal) d[n] = -INFINITY;
                    }
                } else if (force) {                            // max_lag = 0: only the best state goes on
                    for (int n = lane; n < S; n += 64)
                        if (n != goal) d[n] = -INFINITY;
                }
            }
        }
    }
    __threadfence_block();
    __syncthreads();                                           // the labels are there for every lane
    give_runs(head, fresh, window, S, sym, my_kept, ring_labels, out, lane);
    if (lane == 0) {
        *my_head = head;                                       // (the position is the advance's to move)
        *my_count = out.count;
    }
    fill_runs(out, lane);
}

// grid (ceil(streams / 64)), 64 threads: thread = stream.  The commit has said whether the stream took its frames.
__global__ __launch_bounds__(64) void viterbi_stream_advance(int streams, const int* __restrict__ lengths,
                                                              const int* __restrict__ count,
                                                              ViterbiHead* __restrict__ heads)
{
    const int item = blockIdx.x * 64 + threadIdx.x;
    if (item >= streams) return;
    if (count[item] >= 0) heads[item].position += lengths[item];
}

// a stream at frame 0 with the graph `graph`.  Wave-uniform; the lanes write D and the ancestors of a whole row.
__device__ __forceinline__ void restart(ViterbiHead* head, int graph, float* d, uint16_t* anc, int row, int lane) {
    for (int n = lane; n < row; n += 64) {
        d[n] = -INFINITY;
        anc[n] = (uint16_t)n;
    }
    if (lane == 0) *head = ViterbiHead{0, 0, 0, -1, 0, 0.f, 0.f, graph};
}

// grid (streams), 64 threads, `held` * 4 bytes of dynamic LDS.  A stream `which` leaves out, or one without a graph,
// gets count = 0, total = NaN, forced = -1; the first keeps its state.
__global__ __launch_bounds__(64) void viterbi_stream_flush(int window, const int* __restrict__ which,
                                                            ViterbiHead* __restrict__ heads,
                                                            const int* __restrict__ state_begin,
                                                            const int* __restrict__ state_phonemes,
                                                            const float* __restrict__ final_,
                                                            const int* __restrict__ arc_begin,
                                                            const int* __restrict__ sources, int held, int row,
                                                            float* __restrict__ state_d,
                                                            uint16_t* __restrict__ state_anc,
                                                            const uint8_t* __restrict__ back,
                                                            const float* __restrict__ kept, int* __restrict__ labels,
                                                            int cap, int* __restrict__ states,
                                                            int* __restrict__ phonemes, int* __restrict__ begin,
                                                            int* __restrict__ end, float* __restrict__ score,
                                                            float* __restrict__ gop, int* __restrict__ count,
                                                            float* __restrict__ total, int* __restrict__ forced)
{
    __shared__ uint4 rows[VROWS_VEC];
    __shared__ uint16_t first[VSTATES];
    extern __shared__ int held_sources[];
    const int item = blockIdx.x, lane = threadIdx.x;
    StateRuns out = state_runs_of(item, cap, states, phonemes, begin, end, score, gop);
    ViterbiHead head = heads[item];
    ViterbiHead* my_head = in_vector_registers(heads + item);  // what is written at the end: out of the scalar file now
    int* my_count = in_vector_registers(count + item);
    float* my_total = in_vector_registers(total + item);
    int* my_forced = in_vector_registers(forced + item);
    uint16_t* my_anc = in_vector_registers(state_anc + (size_t)item * row);
    const bool meant = !which || which[item] != 0;
    // (a head that no open, reset or push of this library left gives nothing out and is reset)
    const bool sound = head.graph >= 0 && head.commit >= 0 && head.commit <= head.position &&
                       head.position - head.commit <= window;
    float* d = in_vector_registers(state_d + (size_t)item * row);
    float sum = NAN;
    if (meant && sound) {                                      // (uniform)
        const ViterbiGraph graph = graph_of(head.graph, row, state_begin, arc_begin);
        const ViterbiLive live = live_of(graph, sources, held, row, window, back + (size_t)item * window * row,
                                         (PPG_LDS uint16_t*)first, (PPG_LDS int*)held_sources, lane);
        __syncthreads();
        const float* last = in_vector_registers(final_ + graph.first);
        const int state = first_largest_state(graph.S, lane, &sum, [&](int n) { return d[n] + last[n]; });
        int* ring_labels = in_vector_registers(labels + (size_t)item * window);
        const int p = head.position, c = head.commit;
        int fresh = c;
        if (sum > -INFINITY && p > c) {                        // (uniform) everything up to p along the best path
            live.label(state, p - 1, c, p, ring_labels, rows);
            fresh = p;
        }
        __threadfence_block();
        __syncthreads();                                       // the labels are there for every lane
        const int* sym = in_vector_registers(state_phonemes + graph.first);
        give_runs(head, fresh, window, graph.S, sym, in_vector_registers(kept + (size_t)item * window * PREP),
                  ring_labels, out, lane);
        if (head.label >= 0) close_run(head, head.commit, sym, out, lane);
    }
    if (lane == 0) {
        *my_count = out.count;
        *my_total = meant && sound ? sum : NAN;
        *my_forced = meant && sound ? head.forced : -1;
    }
    fill_runs(out, lane);
    if (meant) restart(my_head, head.graph, d, my_anc, row, lane);
}

// grid (streams), 64 threads.  Open: every stream starts at frame 0 with graph which[item] (null: graph 0), or with
// none (-1) if that names no graph or the graph was refused.  Else the streams `which` flags (null: all) start again
// and keep their graph.
template <bool Open>
__global__ __launch_bounds__(64) void viterbi_stream_reset(const int* __restrict__ which, int graphs,
                                                            const int* __restrict__ verdict,
                                                            ViterbiHead* __restrict__ heads,
                                                            float* __restrict__ state_d,
                                                            uint16_t* __restrict__ state_anc, int row)
{
    const int item = blockIdx.x;
    int graph;
    if (Open) {
        const int g = which ? which[item] : 0;
        graph = (unsigned)g < (unsigned)graphs && verdict[g] != 0 ? g : -1;
    } else {
        if (which && which[item] == 0) return;                 // (uniform)
        graph = heads[item].graph;
    }
    restart(heads + item, graph, state_d + (size_t)item * row, state_anc + (size_t)item * row, row, threadIdx.x);
}

// ---- the rungs the host entries share, in the order every entry takes them.  Each returns PPG_OK or has left its
// message; nothing is launched before the last of an entry's checks has passed. ----

// the table of queries of a search, whole-recording or live
int check_queries(const char* what, int queries, int max_phonemes) {
    if (queries > PPG_SEARCH_MAX_QUERIES)
        return ppg::fail_message(PPG_EINVAL, "%s: %d queries, at most %d per call", what, queries,
                                 PPG_SEARCH_MAX_QUERIES);
    if (max_phonemes > PPG_SEARCH_MAX_PHONEMES)
        return ppg::fail_message(PPG_EINVAL, "%s: %d phonemes, at most %d", what, max_phonemes,
                                 PPG_SEARCH_MAX_PHONEMES);
    return PPG_OK;
}

// the checks the three stream entries share: the state and its geometry
int check_stream_state(const char* what, const void* state, int streams, int queries, int max_phonemes) {
    if (!state || streams <= 0 || queries <= 0 || max_phonemes <= 0)
        return ppg::fail_message(PPG_EINVAL, "%s: bad argument", what);
    if (streams > PPG_SEARCH_MAX_ITEMS)
        return ppg::fail_message(PPG_EINVAL, "%s: %d streams, at most %d per call", what, streams, PPG_SEARCH_MAX_ITEMS);
    if (const int rc = check_queries(what, queries, max_phonemes)) return rc;
    if (reinterpret_cast<uintptr_t>(state) % 16)
        return ppg::fail_message(PPG_EINVAL, "%s: the state must be 16-byte aligned", what);
    return PPG_OK;
}

bool recognize_stream_sizes_fine(int streams, int window) {
    return streams > 0 && streams <= PPG_RECOGNIZE_STREAM_MAX_STREAMS && window >= PPG_RECOGNIZE_STREAM_MIN_WINDOW &&
           window <= PPG_RECOGNIZE_STREAM_MAX_WINDOW && window % 64 == 0;
}

// the checks the three entries of the live recogniser share: the state and its geometry
int check_recognize_stream_state(const char* what, const void* state, int streams, int window) {
    if (!state) return ppg::fail_message(PPG_EINVAL, "%s: bad argument", what);
    if (!recognize_stream_sizes_fine(streams, window))
        return ppg::fail_message(PPG_EINVAL, "%s: %d streams of a window of %d frames: 1 to %d streams, a window that "
                                 "is a multiple of 64 from %d to %d", what, streams, window,
                                 PPG_RECOGNIZE_STREAM_MAX_STREAMS, PPG_RECOGNIZE_STREAM_MIN_WINDOW,
                                 PPG_RECOGNIZE_STREAM_MAX_WINDOW);
    if (reinterpret_cast<uintptr_t>(state) % 16)
        return ppg::fail_message(PPG_EINVAL, "%s: the state must be 16-byte aligned", what);
    return PPG_OK;
}

bool viterbi_stream_sizes_fine(int streams, int window, int max_states) {
    return streams > 0 && streams <= PPG_VITERBI_STREAM_MAX_STREAMS && window >= PPG_VITERBI_STREAM_MIN_WINDOW &&
           window <= PPG_VITERBI_STREAM_MAX_WINDOW && window % 64 == 0 && max_states > 0 &&
           max_states <= PPG_VITERBI_MAX_STATES;
}

// the checks every entry of the live Viterbi shares: the state and its geometry
int check_viterbi_stream_state(const char* what, const void* state, int streams, int window, int max_states) {
    if (!state) return ppg::fail_message(PPG_EINVAL, "%s: bad argument", what);
    if (!viterbi_stream_sizes_fine(streams, window, max_states))
        return ppg::fail_message(PPG_EINVAL, "%s: %d streams of a window of %d frames and %d states: 1 to %d streams, a "
                                 "window that is a multiple of 64 from %d to %d, 1 to %d states", what, streams, window,
                                 max_states, PPG_VITERBI_STREAM_MAX_STREAMS, PPG_VITERBI_STREAM_MIN_WINDOW,
                                 PPG_VITERBI_STREAM_MAX_WINDOW, PPG_VITERBI_MAX_STATES);
    if (reinterpret_cast<uintptr_t>(state) % 16)
        return ppg::fail_message(PPG_EINVAL, "%s: the state must be 16-byte aligned", what);
    return PPG_OK;
}

// the packed graphs of a live Viterbi: as ppg_viterbi takes them, and no more graphs than streams
int check_stream_graphs(const char* what, int streams, int graphs, int n_states, int n_arcs, int max_states,
                        const void* sources, const void* weights) {
    if (graphs <= 0 || n_states <= 0 || n_arcs < 0) return ppg::fail_message(PPG_EINVAL, "%s: bad argument", what);
    if (graphs > streams)
        return ppg::fail_message(PPG_EINVAL, "%s: %d graphs for %d streams, at most one each", what, graphs, streams);
    if (n_states < graphs || (long long)n_states > (long long)graphs * max_states ||
        (long long)n_arcs > (long long)graphs * PPG_VITERBI_MAX_ARCS)
        return ppg::fail_message(PPG_EINVAL, "%s: %d states and %d arcs cannot be %d graphs of 1 to %d states and at "
                                 "most %d arcs", what, n_states, n_arcs, graphs, max_states, PPG_VITERBI_MAX_ARCS);
    if (n_arcs > 0 && (!sources || !weights)) return ppg::fail_message(PPG_EINVAL, "%s: bad argument", what);
    return PPG_OK;
}

// the words a kernel reads and writes: none NULL but those that may be, every one on a 4-byte boundary
int check_words(const char* what, std::initializer_list<const void*> required,
                std::initializer_list<const void*> may_be_null) {
    for (const void* pointer : required)
        if (!pointer) return ppg::fail_message(PPG_EINVAL, "%s: bad argument", what);
    for (const auto& list : {required, may_be_null})
        for (const void* pointer : list)
            if (reinterpret_cast<uintptr_t>(pointer) % 4)
                return ppg::fail_message(PPG_EINVAL, "%s: inputs and outputs must be 4-byte aligned", what);
    return PPG_OK;
}

// the PPGs of a call: alignment and decode take PPG_ALIGN_MAX_*, the search PPG_SEARCH_MAX_*
int check_common(const char* what, const void* ppg, int frames, int items, const void* lengths,
                 int max_frames = PPG_ALIGN_MAX_FRAMES, int max_items = PPG_ALIGN_MAX_ITEMS) {
    if (!ppg || !lengths || items <= 0 || frames <= 0) return ppg::fail_message(PPG_EINVAL, "%s: bad argument", what);
    if (frames > max_frames) return ppg::fail_message(PPG_EINVAL, "%s: %d frames, at most %d", what, frames, max_frames);
    if (items > max_items)
        return ppg::fail_message(PPG_EINVAL, "%s: %d items, at most %d per call", what, items, max_items);
    return PPG_OK;
}

// the sizes ppg_align_workspace_bytes and ppg_align_optional_workspace_bytes answer for
bool align_sizes_fine(int items, int frames, int max_phonemes) {
    return items > 0 && items <= PPG_ALIGN_MAX_ITEMS && frames > 0 && frames <= PPG_ALIGN_MAX_FRAMES &&
           max_phonemes > 0 && max_phonemes <= PPG_ALIGN_MAX_PHONEMES;
}

int check_workspace(const char* what, const void* workspace, size_t bytes, size_t need) {
    if (bytes < need)
        return ppg::fail_message(PPG_EINVAL, "%s: workspace of %zu bytes, %zu needed", what, bytes, need);
    if (reinterpret_cast<uintptr_t>(workspace) % 16)
        return ppg::fail_message(PPG_EINVAL, "%s: workspace must be 16-byte aligned", what);
    return PPG_OK;
}

// the last check of every entry: from here on it launches
int select_device(int device) {
    if (hipSetDevice(device) != hipSuccess)
        return ppg::fail_message(PPG_EDEVICE, "no HIP device: the post-ops have no CPU path");
    return PPG_OK;
}

// what an entry returns after its launches
int launched(const char* what) {
    const hipError_t he = hipGetLastError();
    return he == hipSuccess ? PPG_OK : ppg::fail_message(PPG_EDEVICE, "%s: %s", what, hipGetErrorString(he));
}

}  // namespace

// What ppg_posterior.hip shares with this unit: the prepared frames and the check of the packed graphs'
// in-arc lists, launched from here so that there is one build of either kernel.
namespace ppg {

void launch_align_prepare(void* stream, const float* ppg, int frames, int items, const int32_t* lengths, float* logp) {
    hipLaunchKernelGGL(align_prepare, dim3((frames + 63) / 64, items), dim3(64), 0, static_cast<hipStream_t>(stream),
                       ppg, frames, lengths, logp);
}

void launch_viterbi_check(void* stream, int graphs, int n_states, int n_arcs, int max_states,
                          const int32_t* state_begin, const int32_t* state_phonemes, const float* stay,
                          const float* initial, const float* final_, const int32_t* arc_begin, const int32_t* sources,
                          const float* weights, int32_t* verdict) {
    hipLaunchKernelGGL(viterbi_check, dim3(graphs), dim3(64), 0, static_cast<hipStream_t>(stream), n_states, n_arcs,
                       max_states, state_begin, state_phonemes, stay, initial, final_, arc_begin, sources, weights,
                       verdict);
}

}  // namespace ppg

extern "C" {

size_t ppg_align_workspace_bytes(int items, int frames, int max_phonemes) {
    return align_sizes_fine(items, frames, max_phonemes) ? layout(items, frames, false).bytes : 0;
}

int ppg_align(int device, const float* ppg, int frames, int items, const int32_t* lengths, const int32_t* phonemes,
              int max_phonemes, const int32_t* phoneme_lengths, float* total, int32_t* starts, float* score,
              float* gop, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = check_common("align", ppg, frames, items, lengths)) return rc;
    if (!phonemes || !phoneme_lengths || !total || !starts || !score || !workspace || max_phonemes <= 0)
        return ppg::fail_message(PPG_EINVAL, "align: bad argument");
    if (max_phonemes > PPG_ALIGN_MAX_PHONEMES)
        return ppg::fail_message(PPG_EINVAL, "align: %d phonemes, at most %d", max_phonemes, PPG_ALIGN_MAX_PHONEMES);
    const Layout w = layout(items, frames, false);
    if (const int rc = check_workspace("align", workspace, workspace_bytes, w.bytes)) return rc;
    if (const int rc = select_device(device)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    float* logp = reinterpret_cast<float*>(ws + w.logp);
    uint16_t* dirs = reinterpret_cast<uint16_t*>(ws + w.dirs);
    hipLaunchKernelGGL(align_prepare, dim3((frames + 63) / 64, items), dim3(64), 0, s, ppg, frames, lengths, logp);
    hipLaunchKernelGGL(align_programme, dim3(items), dim3(64), 0, s, logp, frames, lengths, phonemes, max_phonemes,
                       phoneme_lengths, dirs, total);
    hipLaunchKernelGGL(align_traceback, dim3(items), dim3(64), 0, s, dirs, frames, lengths, max_phonemes,
                       phoneme_lengths, total, starts);
    hipLaunchKernelGGL(align_score, dim3((max_phonemes + 63) / 64, items), dim3(64), 0, s, logp, frames, lengths,
                       phonemes, max_phonemes, phoneme_lengths, total, starts, score, gop);
    return launched("align");
}

size_t ppg_align_optional_workspace_bytes(int items, int frames, int max_phonemes) {
    return align_sizes_fine(items, frames, max_phonemes) ? layout(items, frames, true).bytes : 0;
}

int ppg_align_optional(int device, const float* ppg, int frames, int items, const int32_t* lengths,
                       const int32_t* phonemes, const int32_t* optional, int max_phonemes,
                       const int32_t* phoneme_lengths, float* total, int32_t* starts, float* score, float* gop,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = check_common("align_optional", ppg, frames, items, lengths)) return rc;
    if (!phonemes || !optional || !phoneme_lengths || !total || !starts || !score || !workspace || max_phonemes <= 0)
        return ppg::fail_message(PPG_EINVAL, "align_optional: bad argument");
    if (max_phonemes > PPG_ALIGN_MAX_PHONEMES)
        return ppg::fail_message(PPG_EINVAL, "align_optional: %d phonemes, at most %d", max_phonemes,
                                 PPG_ALIGN_MAX_PHONEMES);
    const Layout w = layout(items, frames, true);
    if (const int rc = check_workspace("align_optional", workspace, workspace_bytes, w.bytes)) return rc;
    if (const int rc = select_device(device)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    float* logp = reinterpret_cast<float*>(ws + w.logp);
    uint16_t* dirs = reinterpret_cast<uint16_t*>(ws + w.dirs);
    uint16_t* skips = reinterpret_cast<uint16_t*>(ws + w.skips);
    int* ends = reinterpret_cast<int*>(ws + w.ends);
    hipLaunchKernelGGL(align_prepare, dim3((frames + 63) / 64, items), dim3(64), 0, s, ppg, frames, lengths, logp);
    hipLaunchKernelGGL(align_programme_optional, dim3(items), dim3(64), 0, s, logp, frames, lengths, phonemes, optional,
                       max_phonemes, phoneme_lengths, dirs, skips, ends, total);
    hipLaunchKernelGGL(align_traceback_optional, dim3(items), dim3(64), 0, s, dirs, skips, frames, lengths,
                       max_phonemes, phoneme_lengths, total, ends, starts);
    hipLaunchKernelGGL(align_score_optional, dim3((max_phonemes + 63) / 64, items), dim3(64), 0, s, logp, frames,
                       lengths, phonemes, max_phonemes, phoneme_lengths, total, starts, score, gop);
    return launched("align_optional");
}

int ppg_decode(int device, const float* ppg, int frames, int items, const int32_t* lengths, int32_t* phonemes,
               int32_t* starts, int32_t* runs, void* stream) {
    if (const int rc = check_common("decode", ppg, frames, items, lengths)) return rc;
    if (!phonemes || !starts || !runs) return ppg::fail_message(PPG_EINVAL, "decode: bad argument");
    if (const int rc = select_device(device)) return rc;
    hipLaunchKernelGGL(decode_runs, dim3(items), dim3(64), 0, static_cast<hipStream_t>(stream), ppg, frames, lengths,
                       phonemes, starts, runs);
    return launched("decode");
}

size_t ppg_recognize_workspace_bytes(int items, int frames) {
    if (items <= 0 || items > PPG_RECOGNIZE_MAX_ITEMS || frames <= 0 || frames > PPG_RECOGNIZE_MAX_FRAMES) return 0;
    return recognize_layout(items, frames).bytes;
}

int ppg_recognize(int device, const float* ppg, int frames, int items, const int32_t* lengths,
                  const float* transitions, const float* initial, const float* final_, int32_t* phonemes,
                  int32_t* starts, int32_t* runs, float* total, float* score, float* gop, void* workspace,
                  size_t workspace_bytes, void* stream) {
    if (const int rc = check_common("recognize", ppg, frames, items, lengths, PPG_RECOGNIZE_MAX_FRAMES,
                                    PPG_RECOGNIZE_MAX_ITEMS))
        return rc;
    if (!transitions || !phonemes || !starts || !runs || !total || !score || !workspace)
        return ppg::fail_message(PPG_EINVAL, "recognize: bad argument");
    const RecognizeLayout w = recognize_layout(items, frames);
    if (const int rc = check_workspace("recognize", workspace, workspace_bytes, w.bytes)) return rc;
    if (const int rc = select_device(device)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    float* logp = reinterpret_cast<float*>(ws + w.logp);
    uint32_t* back = reinterpret_cast<uint32_t*>(ws + w.back);
    int* labels = reinterpret_cast<int*>(ws + w.labels);
    int* ends = reinterpret_cast<int*>(ws + w.ends);
    hipLaunchKernelGGL(align_prepare, dim3((frames + 63) / 64, items), dim3(64), 0, s, ppg, frames, lengths, logp);
    hipLaunchKernelGGL(recognize_programme, dim3(items), dim3(64), 0, s, logp, frames, lengths, transitions, initial,
                       final_, back, ends, runs, total);
    hipLaunchKernelGGL(recognize_traceback, dim3(items), dim3(64), 0, s, back, frames, lengths, total, ends, labels);
    hipLaunchKernelGGL(recognize_runs, dim3(items), dim3(64), 0, s, labels, frames, lengths, total, phonemes, starts,
                       runs);
    // the runs as a transcript: at most `frames` phonemes, `runs` of them
    hipLaunchKernelGGL(align_score, dim3((frames + 63) / 64, items), dim3(64), 0, s, logp, frames, lengths, phonemes,
                       frames, runs, total, starts, score, gop);
    return launched("recognize");
}

size_t ppg_viterbi_workspace_bytes(int items, int frames, int max_states) {
    if (items <= 0 || items > PPG_VITERBI_MAX_ITEMS || frames <= 0 || frames > PPG_VITERBI_MAX_FRAMES ||
        max_states <= 0 || max_states > PPG_VITERBI_MAX_STATES)
        return 0;
    return viterbi_layout(items, frames, max_states).bytes;
}

int ppg_viterbi(int device, const float* ppg, int frames, int items, const int32_t* lengths, int graphs, int n_states,
                int n_arcs, int max_states, const int32_t* state_begin, const int32_t* state_phonemes,
                const float* stay, const float* initial, const float* final_, const int32_t* arc_begin,
                const int32_t* sources, const float* weights, const int32_t* which, int32_t* states,
                int32_t* phonemes, int32_t* starts, int32_t* runs, float* total, float* score, float* gop,
                void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = check_common("viterbi", ppg, frames, items, lengths, PPG_VITERBI_MAX_FRAMES,
                                    PPG_VITERBI_MAX_ITEMS))
        return rc;
    if (!workspace || graphs <= 0 || n_states <= 0 || n_arcs < 0 || max_states <= 0)
        return ppg::fail_message(PPG_EINVAL, "viterbi: bad argument");
    if (graphs > PPG_VITERBI_MAX_GRAPHS)
        return ppg::fail_message(PPG_EINVAL, "viterbi: %d graphs, at most %d per call", graphs, PPG_VITERBI_MAX_GRAPHS);
    if (max_states > PPG_VITERBI_MAX_STATES)
        return ppg::fail_message(PPG_EINVAL, "viterbi: %d states, at most %d per graph", max_states,
                                 PPG_VITERBI_MAX_STATES);
    if (n_states < graphs || (long long)n_states > (long long)graphs * max_states ||
        (long long)n_arcs > (long long)graphs * PPG_VITERBI_MAX_ARCS)
        return ppg::fail_message(PPG_EINVAL, "viterbi: %d states and %d arcs cannot be %d graphs of 1 to %d states and "
                                 "at most %d arcs", n_states, n_arcs, graphs, max_states, PPG_VITERBI_MAX_ARCS);
    if (n_arcs > 0 && (!sources || !weights)) return ppg::fail_message(PPG_EINVAL, "viterbi: bad argument");
    if (const int rc = check_words("viterbi", {state_begin, state_phonemes, stay, initial, final_, arc_begin, states,
                                               phonemes, starts, runs, total, score},
                                   {sources, weights, which, gop, ppg, lengths}))
        return rc;
    const ViterbiLayout w = viterbi_layout(items, frames, max_states);
    if (const int rc = check_workspace("viterbi", workspace, workspace_bytes, w.bytes)) return rc;
    if (const int rc = select_device(device)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    float* logp = reinterpret_cast<float*>(ws + w.logp);
    uint8_t* back = reinterpret_cast<uint8_t*>(ws + w.back);
    int* labels = reinterpret_cast<int*>(ws + w.labels);
    int* ends = reinterpret_cast<int*>(ws + w.ends);
    int* verdict = reinterpret_cast<int*>(ws + w.verdict);
    // the arcs a wave keeps in LDS: no graph of the call has more than all of them
    const int held = n_arcs < VHELD ? n_arcs : VHELD;
    hipLaunchKernelGGL(viterbi_check, dim3(graphs), dim3(64), 0, s, n_states, n_arcs, max_states, state_begin,
                       state_phonemes, stay, initial, final_, arc_begin, sources, weights, verdict);
    hipLaunchKernelGGL(align_prepare, dim3((frames + 63) / 64, items), dim3(64), 0, s, ppg, frames, lengths, logp);
    const int row = viterbi_row(max_states);
    hipLaunchKernelGGL(row == 64 ? viterbi_programme<1> : viterbi_programme<4>, dim3(items), dim3(64),
                       (size_t)held * sizeof(uint2), s, logp, frames, lengths, graphs, which, verdict, state_begin,
                       state_phonemes, stay, initial, final_, arc_begin, sources, weights, held, row, back, ends, runs,
                       total);
    hipLaunchKernelGGL(viterbi_traceback, dim3(items), dim3(64), (size_t)held * sizeof(int), s, back, frames, lengths,
                       which, state_begin, arc_begin, sources, held, row, total, ends, labels);
    hipLaunchKernelGGL(viterbi_runs, dim3(items), dim3(64), 0, s, labels, frames, lengths, which, state_begin,
                       state_phonemes, total, states, phonemes, starts, runs);
    // the runs as a transcript: at most `frames` phonemes, `runs` of them
    hipLaunchKernelGGL(align_score, dim3((frames + 63) / 64, items), dim3(64), 0, s, logp, frames, lengths, phonemes,
                       frames, runs, total, starts, score, gop);
    return launched("viterbi");
}

size_t ppg_search_workspace_bytes(int items, int frames, int queries) {
    if (items <= 0 || items > PPG_SEARCH_MAX_ITEMS || frames <= 0 || frames > PPG_SEARCH_MAX_FRAMES || queries <= 0 ||
        queries > PPG_SEARCH_MAX_QUERIES)
        return 0;
    return search_layout(items, frames, queries).bytes;
}

int ppg_search(int device, const float* ppg, int frames, int items, const int32_t* lengths, const int32_t* phonemes,
               int max_phonemes, int queries, const int32_t* phoneme_lengths, int top, float threshold, int32_t* begin,
               int32_t* end, float* total, float* mean, int32_t* count, float* curve_total, int32_t* curve_begin,
               void* workspace, size_t workspace_bytes, void* stream) {
    if (!phonemes || !phoneme_lengths || !begin || !end || !total || !mean || !count || !workspace || queries <= 0 ||
        max_phonemes <= 0)
        return ppg::fail_message(PPG_EINVAL, "search: bad argument");
    if (const int rc = check_common("search", ppg, frames, items, lengths, PPG_SEARCH_MAX_FRAMES, PPG_SEARCH_MAX_ITEMS))
        return rc;
    if (const int rc = check_queries("search", queries, max_phonemes)) return rc;
    if (top < 1 || top > PPG_SEARCH_MAX_HITS)
        return ppg::fail_message(PPG_EINVAL, "search: top = %d, must be 1 .. %d", top, PPG_SEARCH_MAX_HITS);
    if (threshold != threshold) return ppg::fail_message(PPG_EINVAL, "search: the threshold is NaN");
    if (!curve_total != !curve_begin)
        return ppg::fail_message(PPG_EINVAL, "search: curve_total and curve_begin go together");
    const SearchLayout w = search_layout(items, frames, queries);
    if (const int rc = check_workspace("search", workspace, workspace_bytes, w.bytes)) return rc;
    if (const int rc = select_device(device)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    float* logp = reinterpret_cast<float*>(ws + w.logp);
    float* totals = reinterpret_cast<float*>(ws + w.totals);
    int* begins = reinterpret_cast<int*>(ws + w.begins);
    hipLaunchKernelGGL(align_prepare, dim3((frames + 63) / 64, items), dim3(64), 0, s, ppg, frames, lengths, logp);
    hipLaunchKernelGGL(search_programme, dim3(queries, items), dim3(64), 0, s, logp, frames, lengths, phonemes,
                       max_phonemes, phoneme_lengths, totals, begins, count);
    hipLaunchKernelGGL(search_pick, dim3(queries, items), dim3(64), 0, s, frames, lengths, phoneme_lengths, top,
                       threshold, totals, begins, begin, end, total, mean, count, curve_total, curve_begin);
    return launched("search");
}

size_t ppg_search_stream_state_bytes(int streams, int queries, int max_phonemes) {
    if (streams <= 0 || streams > PPG_SEARCH_MAX_ITEMS || queries <= 0 || queries > PPG_SEARCH_MAX_QUERIES ||
        max_phonemes <= 0 || max_phonemes > PPG_SEARCH_MAX_PHONEMES)
        return 0;
    return stream_layout(streams, queries, max_phonemes).bytes;
}

size_t ppg_search_stream_workspace_bytes(int streams, int frames, int queries) {
    if (streams <= 0 || streams > PPG_SEARCH_MAX_ITEMS || frames <= 0 || frames > PPG_SEARCH_MAX_FRAMES ||
        queries <= 0 || queries > PPG_SEARCH_MAX_QUERIES)
        return 0;
    return prepared_bytes(streams, frames);
}

int ppg_search_stream_reset(int device, void* state, int streams, int queries, int max_phonemes, const int32_t* which,
                            void* stream) {
    if (const int rc = check_stream_state("search_stream_reset", state, streams, queries, max_phonemes)) return rc;
    if (const int rc = select_device(device)) return rc;
    const StreamLayout w = stream_layout(streams, queries, max_phonemes);
    char* st = static_cast<char*>(state);
    hipLaunchKernelGGL(search_stream_reset, dim3(queries, streams), dim3(64), 0, static_cast<hipStream_t>(stream),
                       max_phonemes, which, reinterpret_cast<int*>(st + w.positions),
                       reinterpret_cast<Detector*>(st + w.detectors), reinterpret_cast<float*>(st + w.totals),
                       reinterpret_cast<int*>(st + w.begins));
    return launched("search_stream_reset");
}

int ppg_search_stream_push(int device, void* state, const float* ppg, int frames, int streams, const int32_t* lengths,
                           const int32_t* phonemes, int max_phonemes, int queries, const int32_t* phoneme_lengths,
                           float threshold, int patience, int cap, int32_t* begin, int32_t* end, float* total,
                           float* mean, int32_t* count, float* curve_total, int32_t* curve_begin, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (!ppg || !lengths || !phonemes || !phoneme_lengths || !begin || !end || !total || !mean || !count ||
        !workspace || frames <= 0)
        return ppg::fail_message(PPG_EINVAL, "search_stream_push: bad argument");
    if (const int rc = check_stream_state("search_stream_push", state, streams, queries, max_phonemes)) return rc;
    if (frames > PPG_SEARCH_MAX_FRAMES)
        return ppg::fail_message(PPG_EINVAL, "search_stream_push: %d frames, at most %d", frames,
                                 PPG_SEARCH_MAX_FRAMES);
    if (threshold != threshold) return ppg::fail_message(PPG_EINVAL, "search_stream_push: the threshold is NaN");
    if (patience < 0) return ppg::fail_message(PPG_EINVAL, "search_stream_push: patience = %d is negative", patience);
    if (cap < 1) return ppg::fail_message(PPG_EINVAL, "search_stream_push: cap = %d, must be at least 1", cap);
    if (!curve_total != !curve_begin)
        return ppg::fail_message(PPG_EINVAL, "search_stream_push: curve_total and curve_begin go together");
    if (const int rc = check_workspace("search_stream_push", workspace, workspace_bytes,
                                       prepared_bytes(streams, frames)))
        return rc;
    if (const int rc = select_device(device)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const StreamLayout w = stream_layout(streams, queries, max_phonemes);
    char* st = static_cast<char*>(state);
    int* positions = reinterpret_cast<int*>(st + w.positions);
    float* logp = static_cast<float*>(workspace);
    hipLaunchKernelGGL(align_prepare, dim3((frames + 63) / 64, streams), dim3(64), 0, s, ppg, frames, lengths, logp);
    hipLaunchKernelGGL(search_stream_programme, dim3(queries, streams), dim3(64), 0, s, logp, frames, lengths, phonemes,
                       max_phonemes, phoneme_lengths, positions, reinterpret_cast<Detector*>(st + w.detectors),
                       reinterpret_cast<float*>(st + w.totals), reinterpret_cast<int*>(st + w.begins), threshold,
                       patience, cap, begin, end, total, mean, count, curve_total, curve_begin);
    hipLaunchKernelGGL(search_stream_advance, dim3((streams + 63) / 64), dim3(64), 0, s, streams, frames, lengths,
                       positions);
    return launched("search_stream_push");
}

int ppg_search_stream_flush(int device, void* state, int streams, int queries, int max_phonemes, const int32_t* which,
                            int32_t* begin, int32_t* end, float* total, float* mean, int32_t* count, void* stream) {
    if (!begin || !end || !total || !mean || !count)
        return ppg::fail_message(PPG_EINVAL, "search_stream_flush: bad argument");
    if (const int rc = check_stream_state("search_stream_flush", state, streams, queries, max_phonemes)) return rc;
    if (const int rc = select_device(device)) return rc;
    const StreamLayout w = stream_layout(streams, queries, max_phonemes);
    const size_t pairs = (size_t)streams * queries;
    hipLaunchKernelGGL(search_stream_flush, dim3((unsigned)((pairs + 63) / 64)), dim3(64), 0,
                       static_cast<hipStream_t>(stream), streams, queries, which,
                       reinterpret_cast<Detector*>(static_cast<char*>(state) + w.detectors), begin, end, total, mean,
                       count);
    return launched("search_stream_flush");
}

size_t ppg_recognize_stream_state_bytes(int streams, int window) {
    return recognize_stream_sizes_fine(streams, window) ? recognize_stream_layout(streams, window).bytes : 0;
}

size_t ppg_recognize_stream_workspace_bytes(int streams, int frames) {
    if (streams <= 0 || streams > PPG_RECOGNIZE_STREAM_MAX_STREAMS || frames <= 0 || frames > PPG_RECOGNIZE_MAX_FRAMES)
        return 0;
    return prepared_bytes(streams, frames);
}

int ppg_recognize_stream_reset(int device, void* state, int streams, int window, const int32_t* which, void* stream) {
    if (const int rc = check_recognize_stream_state("recognize_stream_reset", state, streams, window)) return rc;
    if (const int rc = check_words("recognize_stream_reset", {}, {which})) return rc;
    if (const int rc = select_device(device)) return rc;
    const RecognizeStreamLayout w = recognize_stream_layout(streams, window);
    char* st = static_cast<char*>(state);
    hipLaunchKernelGGL(recognize_stream_reset, dim3(streams), dim3(64), 0, static_cast<hipStream_t>(stream), which,
                       reinterpret_cast<RecognizeHead*>(st + w.heads), reinterpret_cast<float*>(st + w.d),
                       reinterpret_cast<int*>(st + w.anc));
    return launched("recognize_stream_reset");
}

int ppg_recognize_stream_push(int device, void* state, int streams, int window, const float* ppg, int frames,
                              const int32_t* lengths, const float* transitions, const float* initial, int max_lag,
                              int cap, int32_t* phonemes, int32_t* begin, int32_t* end, float* score, float* gop,
                              int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "recognize_stream_push";
    if (const int rc = check_recognize_stream_state(what, state, streams, window)) return rc;
    if (const int rc = check_words(what, {ppg, lengths, transitions, phonemes, begin, end, score, count, workspace},
                                   {initial, gop}))
        return rc;
    if (frames < 1 || frames > PPG_RECOGNIZE_MAX_FRAMES)
        return ppg::fail_message(PPG_EINVAL, "%s: %d frames, must be 1 .. %d", what, frames, PPG_RECOGNIZE_MAX_FRAMES);
    if (max_lag < 0 || max_lag >= window)
        return ppg::fail_message(PPG_EINVAL, "%s: max_lag = %d, must be 0 .. window - 1 = %d", what, max_lag,
                                 window - 1);
    if (cap < 1) return ppg::fail_message(PPG_EINVAL, "%s: cap = %d, must be at least 1", what, cap);
    if (const int rc = check_workspace(what, workspace, workspace_bytes, prepared_bytes(streams, frames))) return rc;
    if (const int rc = select_device(device)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const RecognizeStreamLayout w = recognize_stream_layout(streams, window);
    char* st = static_cast<char*>(state);
    RecognizeHead* heads = reinterpret_cast<RecognizeHead*>(st + w.heads);
    float* d = reinterpret_cast<float*>(st + w.d);
    uint32_t* back = reinterpret_cast<uint32_t*>(st + w.back);
    float* kept = reinterpret_cast<float*>(st + w.kept);
    float* logp = static_cast<float*>(workspace);
    hipLaunchKernelGGL(align_prepare, dim3((frames + 63) / 64, streams), dim3(64), 0, s, ppg, frames, lengths, logp);
    hipLaunchKernelGGL(recognize_stream_programme, dim3(streams), dim3(64), 0, s, logp, frames, lengths, transitions,
                       initial, window, heads, d, reinterpret_cast<int*>(st + w.anc), back,
                       reinterpret_cast<float4*>(kept));
    hipLaunchKernelGGL(recognize_stream_commit, dim3(streams), dim3(64), 0, s, frames, lengths, window, max_lag, heads,
                       d, reinterpret_cast<int*>(st + w.anc), back, kept, reinterpret_cast<int*>(st + w.labels), cap,
                       phonemes, begin, end, score, gop, count);
    hipLaunchKernelGGL(recognize_stream_advance, dim3((streams + 63) / 64), dim3(64), 0, s, streams, lengths, count,
                       heads);
    return launched(what);
}

int ppg_recognize_stream_flush(int device, void* state, int streams, int window, const float* final_,
                               const int32_t* which, int cap, int32_t* phonemes, int32_t* begin, int32_t* end,
                               float* score, float* gop, int32_t* count, float* total, int32_t* forced, void* stream) {
    const char* what = "recognize_stream_flush";
    if (const int rc = check_recognize_stream_state(what, state, streams, window)) return rc;
    if (const int rc = check_words(what, {phonemes, begin, end, score, count, total, forced}, {final_, which, gop}))
        return rc;
    if (cap < 1) return ppg::fail_message(PPG_EINVAL, "%s: cap = %d, must be at least 1", what, cap);
    if (const int rc = select_device(device)) return rc;
    const RecognizeStreamLayout w = recognize_stream_layout(streams, window);
    char* st = static_cast<char*>(state);
    hipLaunchKernelGGL(recognize_stream_flush, dim3(streams), dim3(64), 0, static_cast<hipStream_t>(stream), window,
                       final_, which, reinterpret_cast<RecognizeHead*>(st + w.heads),
                       reinterpret_cast<float*>(st + w.d), reinterpret_cast<int*>(st + w.anc),
                       reinterpret_cast<const uint32_t*>(st + w.back), reinterpret_cast<const float*>(st + w.kept),
                       reinterpret_cast<int*>(st + w.labels), cap, phonemes, begin, end, score, gop, count, total,
                       forced);
    return launched(what);
}

size_t ppg_viterbi_stream_state_bytes(int streams, int window, int max_states) {
    return viterbi_stream_sizes_fine(streams, window, max_states)
               ? viterbi_stream_layout(streams, window, max_states).bytes : 0;
}

size_t ppg_viterbi_stream_workspace_bytes(int streams, int frames) {
    if (streams <= 0 || streams > PPG_VITERBI_STREAM_MAX_STREAMS || frames <= 0 || frames > PPG_VITERBI_MAX_FRAMES)
        return 0;
    return prepared_bytes(streams, frames);
}

int ppg_viterbi_stream_open(int device, void* state, int streams, int window, int graphs, int n_states, int n_arcs,
                            int max_states, const int32_t* state_begin, const int32_t* state_phonemes,
                            const float* stay, const float* initial, const float* final_, const int32_t* arc_begin,
                            const int32_t* sources, const float* weights, const int32_t* which_graph, void* stream) {
    const char* what = "viterbi_stream_open";
    if (const int rc = check_viterbi_stream_state(what, state, streams, window, max_states)) return rc;
    if (const int rc = check_stream_graphs(what, streams, graphs, n_states, n_arcs, max_states, sources, weights))
        return rc;
    if (const int rc = check_words(what, {state_begin, state_phonemes, stay, initial, final_, arc_begin},
                                   {sources, weights, which_graph}))
        return rc;
    if (const int rc = select_device(device)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const ViterbiStreamLayout w = viterbi_stream_layout(streams, window, max_states);
    char* st = static_cast<char*>(state);
    int* verdict = reinterpret_cast<int*>(st + w.verdict);
    hipLaunchKernelGGL(viterbi_check, dim3(graphs), dim3(64), 0, s, n_states, n_arcs, max_states, state_begin,
                       state_phonemes, stay, initial, final_, arc_begin, sources, weights, verdict);
    hipLaunchKernelGGL(viterbi_stream_reset<true>, dim3(streams), dim3(64), 0, s, which_graph, graphs, verdict,
                       reinterpret_cast<ViterbiHead*>(st + w.heads), reinterpret_cast<float*>(st + w.d),
                       reinterpret_cast<uint16_t*>(st + w.anc), viterbi_row(max_states));
    return launched(what);
}

int ppg_viterbi_stream_reset(int device, void* state, int streams, int window, int max_states, const int32_t* which,
                             void* stream) {
    const char* what = "viterbi_stream_reset";
    if (const int rc = check_viterbi_stream_state(what, state, streams, window, max_states)) return rc;
    if (const int rc = check_words(what, {}, {which})) return rc;
    if (const int rc = select_device(device)) return rc;
    const ViterbiStreamLayout w = viterbi_stream_layout(streams, window, max_states);
    char* st = static_cast<char*>(state);
    hipLaunchKernelGGL(viterbi_stream_reset<false>, dim3(streams), dim3(64), 0, static_cast<hipStream_t>(stream), which,
                       0, static_cast<const int*>(nullptr), reinterpret_cast<ViterbiHead*>(st + w.heads),
                       reinterpret_cast<float*>(st + w.d), reinterpret_cast<uint16_t*>(st + w.anc),
                       viterbi_row(max_states));
    return launched(what);
}

int ppg_viterbi_stream_push(int device, void* state, int streams, int window, const float* ppg, int frames,
                            const int32_t* lengths, int graphs, int n_states, int n_arcs, int max_states,
                            const int32_t* state_begin, const int32_t* state_phonemes, const float* stay,
                            const float* initial, const float* final_, const int32_t* arc_begin,
                            const int32_t* sources, const float* weights, int max_lag, int cap, int32_t* states,
                            int32_t* phonemes, int32_t* begin, int32_t* end, float* score, float* gop, int32_t* count,
                            void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "viterbi_stream_push";
    if (const int rc = check_viterbi_stream_state(what, state, streams, window, max_states)) return rc;
    if (const int rc = check_stream_graphs(what, streams, graphs, n_states, n_arcs, max_states, sources, weights))
        return rc;
    if (const int rc = check_words(what, {ppg, lengths, state_begin, state_phonemes, stay, initial, final_, arc_begin,
                                          states, phonemes, begin, end, score, count, workspace},
                                   {sources, weights, gop}))
        return rc;
    if (frames < 1 || frames > PPG_VITERBI_MAX_FRAMES)
        return ppg::fail_message(PPG_EINVAL, "%s: %d frames, must be 1 .. %d", what, frames, PPG_VITERBI_MAX_FRAMES);
    if (max_lag < 0 || max_lag >= window)
        return ppg::fail_message(PPG_EINVAL, "%s: max_lag = %d, must be 0 .. window - 1 = %d", what, max_lag,
                                 window - 1);
    if (cap < 1) return ppg::fail_message(PPG_EINVAL, "%s: cap = %d, must be at least 1", what, cap);
    if (const int rc = check_workspace(what, workspace, workspace_bytes, prepared_bytes(streams, frames))) return rc;
    if (const int rc = select_device(device)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const ViterbiStreamLayout w = viterbi_stream_layout(streams, window, max_states);
    char* st = static_cast<char*>(state);
    ViterbiHead* heads = reinterpret_cast<ViterbiHead*>(st + w.heads);
    float* d = reinterpret_cast<float*>(st + w.d);
    uint16_t* anc = reinterpret_cast<uint16_t*>(st + w.anc);
    uint8_t* back = reinterpret_cast<uint8_t*>(st + w.back);
    float* kept = reinterpret_cast<float*>(st + w.kept);
    float* logp = static_cast<float*>(workspace);
    const int held = n_arcs < VHELD ? n_arcs : VHELD;         // the arcs a wave keeps in LDS, as in ppg_viterbi
    const int row = viterbi_row(max_states);
    hipLaunchKernelGGL(align_prepare, dim3((frames + 63) / 64, streams), dim3(64), 0, s, ppg, frames, lengths, logp);
    hipLaunchKernelGGL(row == 64 ? viterbi_stream_programme<1> : viterbi_stream_programme<4>, dim3(streams), dim3(64),
                       (size_t)held * sizeof(uint2), s, logp, frames, lengths, window, heads, state_begin,
                       state_phonemes, stay, initial, arc_begin, sources, weights, held, row, d, anc, back,
                       reinterpret_cast<float4*>(kept));
    hipLaunchKernelGGL(viterbi_stream_commit, dim3(streams), dim3(64), (size_t)held * sizeof(int), s, frames, lengths,
                       window, max_lag, heads, state_begin, state_phonemes, arc_begin, sources, held, row, d, anc, back,
                       kept, reinterpret_cast<int*>(st + w.labels), cap, states, phonemes, begin, end, score, gop,
                       count);
    hipLaunchKernelGGL(viterbi_stream_advance, dim3((streams + 63) / 64), dim3(64), 0, s, streams, lengths, count,
                       heads);
    return launched(what);
}

int ppg_viterbi_stream_flush(int device, void* state, int streams, int window, int graphs, int n_states, int n_arcs,
                             int max_states, const int32_t* state_begin, const int32_t* state_phonemes,
                             const float* stay, const float* initial, const float* final_, const int32_t* arc_begin,
                             const int32_t* sources, const float* weights, const int32_t* which, int cap,
                             int32_t* states, int32_t* phonemes, int32_t* begin, int32_t* end, float* score,
                             float* gop, int32_t* count, float* total, int32_t* forced, void* stream) {
    const char* what = "viterbi_stream_flush";
    if (const int rc = check_viterbi_stream_state(what, state, streams, window, max_states)) return rc;
    if (const int rc = check_stream_graphs(what, streams, graphs, n_states, n_arcs, max_states, sources, weights))
        return rc;
    if (const int rc = check_words(what, {state_begin, state_phonemes, stay, initial, final_, arc_begin, states,
                                          phonemes, begin, end, score, count, total, forced},
                                   {sources, weights, which, gop}))
        return rc;
    if (cap < 1) return ppg::fail_message(PPG_EINVAL, "%s: cap = %d, must be at least 1", what, cap);
    if (const int rc = select_device(device)) return rc;
    const ViterbiStreamLayout w = viterbi_stream_layout(streams, window, max_states);
    char* st = static_cast<char*>(state);
    const int held = n_arcs < VHELD ? n_arcs : VHELD;
    hipLaunchKernelGGL(viterbi_stream_flush, dim3(streams), dim3(64), (size_t)held * sizeof(int),
                       static_cast<hipStream_t>(stream), window, which, reinterpret_cast<ViterbiHead*>(st + w.heads),
                       state_begin, state_phonemes, final_, arc_begin, sources, held, viterbi_row(max_states),
                       reinterpret_cast<float*>(st + w.d), reinterpret_cast<uint16_t*>(st + w.anc),
                       reinterpret_cast<const uint8_t*>(st + w.back), reinterpret_cast<const float*>(st + w.kept),
                       reinterpret_cast<int*>(st + w.labels), cap, states, phonemes, begin, end, score, gop, count,
                       total, forced);
    return launched(what);
}

}  // extern "C"

// ---- phrase search over a phoneme graph (ppg_search_graph) ----
//
// ppg_search with a graph of ppg_viterbi in the place of the one chain: pronunciation variants, optional pauses between
// words, a final consonant that may be dropped, all in one query.  One pair is a recording P (40, T) and a graph as in
// ppg_viterbi: S states, sym, stay, ordered in-arcs (src[j], w[j]), initial, final, every weight finite or -inf.  The
// prepared frame is align_prepare's, the emission is the search's: r[t, n] = logp[t][sym[n]] - m[t], one fp32
// subtraction.  Every state carries D (fp32) and a begin b; before frame 0 every D is -inf.  For every t >= 0, frame 0
// included:
//   best = D[t-1, n] + stay[n]; bb = b[t-1, n]
//   for j in list order: c = D[t-1, src[j]] + w[j]; if c > best: best = c, bb = b[t-1, src[j]]
//   if initial[n] > best: best = initial[n], bb = t          a fresh start comes last and only if strictly better
//   D[t, n] = r[t, n] + best; b[t, n] = bb
// Comparisons only, strict >; one fp32 addition per candidate, in order of t; -inf + finite = -inf and -inf > -inf is
// false, so an unreached state never makes a NaN.  Per end frame t, curve_total[t] is the largest D[t, n] + final[n],
// the lowest n on ties (first_largest's rule), curve_begin[t] that state's b, and -1 where the total is -inf.  Hits,
// top, threshold, mean, the tie to the later end frame, the sentinels and count are search_pick's: that kernel runs
// unchanged on the curve with an array of ones for the queries' lengths (it uses a length only to skip the end frames
// below N - 1, whose begin is -1 anyway).  Under chain_graph(s) all weights are 0 and D + 0 is exact; state 0 has the
// candidates stay, then the fresh start, state n > 0 stay, then advance: the search's recurrence candidate for
// candidate, so the curve and the hits are ppg_search's bit for bit.
//   search_graph_programme  grid (graphs, items), one wave per pair, viterbi_programme's structure: D of frame t-1 is
//                           read by index from a double buffer in LDS, a second double buffer holds the begins, the
//                           arcs are copied to LDS once per pair, one barrier per frame, the prepared frames staged
//                           CHUNK at a time with the next chunk in flight.  A graph has at most 256 states here, so a
//                           frame is ONE pass (lane l takes state l if S <= 64, else the four states 4 l .. 4 l + 3)
//                           and a lane's states never change: what viterbi_programme keeps of a state in LDS (the
//                           table word, stay), initial, final and the state's first arcs themselves (four where a
//                           lane has one state, two where it has four) stand in registers for the whole recording,
//                           so D and b at those arcs' sources are read beside the state's own and a frame of a chain
//                           or a phrase is one LDS round trip.  Of the arcs beyond only the SOURCE taken is tracked;
//                           its begin is read once, after the last compare.  No back-pointers.  The curve: per frame
//                           a lane leaves its own largest D + final and that state's b in LDS (a row per frame of
//                           the chunk); after the chunk lane u takes frame u, walks the lanes that hold states in
//                           ascending order with a strict compare (the lowest state of equal values) and the wave
//                           writes the chunk's curve in two coalesced stores.  A 6-step __shfl_xor butterfly per
//                           frame was built first and measured: 742 ns per frame for the chain of 8 against 312 with
//                           the reduction left out; this form costs the same with one final state as
//                           with two, so there is no shortcut for a single final state.
// The legal graphs (256 states, 4096 arcs) always fit the held block, so there is no arcs-from-memory path.

namespace {

constexpr int GSTATES = PPG_SEARCH_GRAPH_MAX_STATES;
static_assert(GSTATES == 256 && PPG_SEARCH_GRAPH_MAX_ARCS == VHELD, "one pass of four states a lane; every graph's arcs are held");

struct SearchGraphLayout {
    size_t logp, totals, begins, verdict, ones, bytes;         // byte offsets into the workspace
};

// (65535 x 65535 pairs of 262144 frames are 9.0e15 bytes: the limits keep this inside a size_t)
inline SearchGraphLayout search_graph_layout(int items, int frames, int graphs) {
    SearchGraphLayout w{};
    const size_t curve = (size_t)items * graphs * frames * sizeof(float);
    size_t at = 0;
    w.logp = at; at += prepared_bytes(items, frames);
    w.totals = at; at = align256(at + curve);
    w.begins = at; at = align256(at + curve);
    w.verdict = at; at = align256(at + (size_t)graphs * sizeof(int));
    w.ones = at; at = align256(at + (size_t)graphs * sizeof(int));
    w.bytes = at;
    return w;
}

// the packed graphs of a search, whole-recording or live: as ppg_viterbi takes them, at most PPG_SEARCH_MAX_QUERIES
int check_search_graphs(const char* what, int graphs, int n_states, int n_arcs, int max_states, const void* sources,
                        const void* weights) {
    if (graphs <= 0 || n_states <= 0 || n_arcs < 0 || max_states <= 0)
        return ppg::fail_message(PPG_EINVAL, "%s: bad argument", what);
    if (graphs > PPG_SEARCH_MAX_QUERIES)
        return ppg::fail_message(PPG_EINVAL, "%s: %d graphs, at most %d per call", what, graphs, PPG_SEARCH_MAX_QUERIES);
    if (max_states > PPG_VITERBI_MAX_STATES)
        return ppg::fail_message(PPG_EINVAL, "%s: %d states, at most %d per graph", what, max_states,
                                 PPG_VITERBI_MAX_STATES);
    if (n_states < graphs || (long long)n_states > (long long)graphs * max_states ||
        (long long)n_arcs > (long long)graphs * PPG_VITERBI_MAX_ARCS)
        return ppg::fail_message(PPG_EINVAL, "%s: %d states and %d arcs cannot be %d graphs of 1 to %d states and at "
                                 "most %d arcs", what, n_states, n_arcs, graphs, max_states, PPG_VITERBI_MAX_ARCS);
    if (n_arcs > 0 && (!sources || !weights)) return ppg::fail_message(PPG_EINVAL, "%s: bad argument", what);
    return PPG_OK;
}

// What the lanes leave per frame of a chunk for the curve: each lane's largest D + final and its begin.  A row has 65
// words, so the lanes that read a row each (lane = frame) meet no bank twice.
struct SearchGraphEnds {
    float total[CHUNK][65];
    int begin[CHUNK][65];
};

// What a push of a live search over a graph carries into the search of one pair and out of it again.
struct GraphCarry {
    float* d; int* b;                         // the pair's D and b between pushes: a row of 64 or 256 words each
    int base;                                 // the stream's position: frame t of the push is frame base + t of the stream
    Detector* det; Events* out;               // the pair's detector, run by lane 0, and this push's events
    float threshold; int patience;
};

// The frames of one pair with G states per lane: 1 for S <= 64, else 4.  `begin` is the graph's own part of arc_begin.
// Live: one push of T >= 1 frames of a stream: D and b come from `live` and go back there (the states at or above S
// run along at -inf / -1 as ever), a fresh start begins at the stream's position + t, the curve is written only if
// asked for, and after every chunk's reduction lane 0 runs the detector over the chunk's frames in order.  Otherwise
// `live` is unused: every state starts at -inf / -1 and frames count from 0.  One body, so the pushes of a stream give
// the curve of the whole recording bit for bit.
// Wave-uniform control flow but for the arcs beyond the first LEAD, the lanes that write the curve and the detector.
template <int G, bool Live>
__device__ __forceinline__ void search_graph_frames(const float4* __restrict__ src, int T, int first, int S,
                                                    const int* __restrict__ phonemes, const float* __restrict__ stay,
                                                    const float* __restrict__ initial,
                                                    const float* __restrict__ final_, const int* __restrict__ begin,
                                                    const ViterbiArcs<true>& arcs, float* __restrict__ totals,
                                                    int* __restrict__ begins, float4 (&stage)[2][CHUNK_VEC],
                                                    float (&dist)[2][GSTATES], int (&began)[2][GSTATES],
                                                    SearchGraphEnds& ends, const GraphCarry& live, int lane)
{
    static_assert(G == 1 || G == 4, "a word or a 16-byte piece per lane");
    const int base = Live ? live.base : 0;
    // arcs per state a lane keeps in registers: four where it has one state (a word's first state takes the pause and
    // three variants of the word before), two where it has four
    constexpr int LEAD = G == 1 ? 4 : VLEAD;
    const int n0 = lane * G, arc0 = begin[0];
    // What the lane keeps of its states for the whole recording: the table word of viterbi_programme, the three
    // weights, and the first LEAD arcs themselves (an arc that is not there: from the state itself at -inf, never
    // better).  States at or above S run along on phoneme 0 without arcs, at -inf, never final.
    int meta[G], lead[G][LEAD]; float own[G], fresh[G], fin[G], heavy[G][LEAD];
#pragma unroll
    for (int k = 0; k < G; ++k) {
        const int n = n0 + k;
        const bool state = n < S;
        meta[k] = state ? (begin[n] - arc0) | (begin[n + 1] - begin[n]) << 16 | phonemes[first + n] << 24 : 0;
        own[k] = state ? stay[first + n] : -INFINITY;
        fresh[k] = state ? initial[first + n] : -INFINITY;
        fin[k] = state ? final_[first + n] : -INFINITY;
#pragma unroll
        for (int j = 0; j < LEAD; ++j) {
            lead[k][j] = n;
            heavy[k][j] = -INFINITY;
            if (j < degree_of(meta[k])) arcs.get(first_arc(meta[k]) + j, lead[k][j], heavy[k][j]);
        }
        // D and b before frame 0, which reads buffer 1: of a push they are the row's words n0 .. n0 + G - 1, which
        // the lane itself stored (or the reset did: the rows are whole, so no lane asks whether n < S)
        dist[1][n] = Live ? live.d[n] : -INFINITY;
        began[1][n] = Live ? live.b[n] : -1;
    }
    float4 next[FETCH];
    fetch(src, 0, T, lane, next);
    stash(stage[0], lane, next);
    __syncthreads();
    const int used = (S + G - 1) / G;                          // the lanes that hold states
    int buf = 0;
    for (int t0 = 0; t0 < T; t0 += CHUNK, buf ^= 1) {
        fetch(src, t0 + CHUNK, T, lane, next);                 // in flight while this chunk is consumed
        const int chunk = min(CHUNK, T - t0);
        for (int u = 0; u < chunk; ++u) {
            const int t = t0 + u;
            const float* e = reinterpret_cast<const float*>(stage[buf]) + u * PREP;
            const float* before = dist[(t & 1) ^ 1];
            const int* origin = began[(t & 1) ^ 1];
            const float top = e[NP];                           // (a broadcast)
            float d[G], cur[G], best[G]; int b[G];
            if constexpr (G == 4) {
                const float4 v = *reinterpret_cast<const float4*>(before + n0);
                const int4 o = *reinterpret_cast<const int4*>(origin + n0);
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
                b[0] = o.x; b[1] = o.y; b[2] = o.z; b[3] = o.w;
            } else {
                d[0] = before[n0];
                b[0] = origin[n0];
            }
            // the first arcs: their D and begins are read beside the state's own, nothing waits for an arc's word
            float came[G][LEAD]; int since[G][LEAD];
#pragma unroll
            for (int k = 0; k < G; ++k) {
#pragma unroll
                for (int j = 0; j < LEAD; ++j) {
                    came[k][j] = before[lead[k][j]];
                    since[k][j] = origin[lead[k][j]];
                }
                cur[k] = e[meta[k] >> 24] - top;
            }
#pragma unroll
            for (int k = 0; k < G; ++k) {
                best[k] = d[k] + own[k];                       // staying: what an arc has to beat
#pragma unroll
                for (int j = 0; j < LEAD; ++j) {
                    const float c = came[k][j] + heavy[k][j];  // -inf + finite = -inf: never NaN
                    const bool better = c > best[k];
                    best[k] = better ? c : best[k];
                    b[k] = better ? since[k][j] : b[k];
                }
            }
#pragma unroll
            for (int k = 0; k < G; ++k) {                      // what lies beyond: state by state, in list order
                const int at = first_arc(meta[k]), degree = degree_of(meta[k]);
                if (degree <= LEAD) continue;
                int via = -1;                                  // the source of the candidate taken here, if any
                auto batch = [&]<int N>(int j0) {              // arcs j0 .. j0 + N - 1, the loads ahead of the compares
                    int p[N]; float w[N];
#pragma unroll
                    for (int q = 0; q < N; ++q)                // (past the last arc the last one again: never better)
                        arcs.get(at + min(j0 + q, degree - 1), p[q], w[q]);
#pragma unroll
                    for (int q = 0; q < N; ++q) {
                        const float c = before[p[q]] + w[q];
                        const bool better = c > best[k];
                        best[k] = better ? c : best[k];
                        via = better ? p[q] : via;
                    }
                };
                batch.template operator()<4>(LEAD);
                for (int j0 = LEAD + 4; j0 < degree; j0 += VAHEAD) batch.template operator()<VAHEAD>(j0);
                if (via >= 0) b[k] = origin[via];
            }
            // the lane's own part of the curve: the first of its largest D + final, ascending n
            float most = -INFINITY; int opened = -1;
#pragma unroll
            for (int k = 0; k < G; ++k) {
                const bool start = fresh[k] > best[k];         // a fresh start: last, and only if strictly better
                d[k] = cur[k] + (start ? fresh[k] : best[k]);
                b[k] = start ? base + t : b[k];
                const float f = d[k] + fin[k];
                const bool better = k == 0 || f > most;
                most = better ? f : most;
                opened = better ? b[k] : opened;
            }
            if constexpr (G == 4) {
                *reinterpret_cast<float4*>(dist[t & 1] + n0) = make_float4(d[0], d[1], d[2], d[3]);
                *reinterpret_cast<int4*>(began[t & 1] + n0) = make_int4(b[0], b[1], b[2], b[3]);
            } else {
                dist[t & 1][n0] = d[0];
                began[t & 1][n0] = b[0];
            }
            ends.total[u][lane] = most;
            ends.begin[u][lane] = opened;
            __syncthreads();                                   // frame t+1 reads what this frame wrote
        }
        // the curve of the chunk, lane = frame: the first of the largest over the lanes in ascending order, which is
        // the lowest state of equal values
        float reach = -INFINITY; int since = -1;               // (Live) frame t0 + lane's two curve values
        if (lane < chunk) {
            float most = ends.total[lane][0];
            int opened = ends.begin[lane][0];
#pragma unroll 4
            for (int j = 1; j < used; ++j) {
                const float f = ends.total[lane][j];
                const int theirs = ends.begin[lane][j];
                const bool better = f > most;
                most = better ? f : most;
                opened = better ? theirs : opened;
            }
            if (!Live || totals) {
                totals[t0 + lane] = most;
                begins[t0 + lane] = most > -INFINITY ? opened : -1;
            }
            if constexpr (Live) {
                reach = most;
                since = most > -INFINITY ? opened : -1;
            }
        }
        if constexpr (Live) {
            // The detector takes the frames in order, and the reduction left frame t0 + u in lane u: lane 0 walks the
            // chunk, each frame's pair read across the lanes with a uniform index (two v_readlane, no LDS, no barrier).
            for (int u = 0; u < chunk; ++u) {                  // (uniform)
                const float sum = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(reach), u));
                const int first = __builtin_amdgcn_readlane(since, u);
                if (lane == 0) detect(*live.det, *live.out, base + t0 + u, sum, first, live.threshold, live.patience);
            }
        }
        stash(stage[buf ^ 1], lane, next);                     // its readers passed the barrier above
        __syncthreads();
    }
    if constexpr (Live) {                                      // the last frame wrote buffer (T - 1) & 1: the lane's own words
#pragma unroll
        for (int k = 0; k < G; ++k) {
            live.d[n0 + k] = dist[(T - 1) & 1][n0 + k];
            live.b[n0 + k] = began[(T - 1) & 1][n0 + k];
        }
    }
}

// grid (graphs, items), 64 threads, `held` * 8 bytes of dynamic LDS.  G states per lane: 1 for S <= 64, else 4.
// count = -1 for a pair that cannot be searched (its graph refused by viterbi_check or beyond 256 states or 4096 arcs,
// its length outside [1, frames]), which touches nothing else; 0 for every other, whose curve (frames below T) is then
// in the workspace.  ones[g] = 1 for search_pick, written here so that the call reads nothing it has not written.
__global__ __launch_bounds__(64) void search_graph_programme(const float* __restrict__ logp, int frames,
                                                              const int* __restrict__ lengths,
                                                              const int* __restrict__ verdict,
                                                              const int* __restrict__ state_begin,
                                                              const int* __restrict__ phonemes,
                                                              const float* __restrict__ stay,
                                                              const float* __restrict__ initial,
                                                              const float* __restrict__ final_,
                                                              const int* __restrict__ arc_begin,
                                                              const int* __restrict__ sources,
                                                              const float* __restrict__ weights,
                                                              float* __restrict__ totals, int* __restrict__ begins,
                                                              int* __restrict__ ones, int* __restrict__ count)
{
    __shared__ float4 stage[2][CHUNK_VEC];
    __shared__ __attribute__((aligned(16))) float dist[2][GSTATES];
    __shared__ __attribute__((aligned(16))) int began[2][GSTATES];
    __shared__ SearchGraphEnds ends;
    extern __shared__ uint2 held_arcs[];
    const int g = blockIdx.x, item = blockIdx.y, lane = threadIdx.x;
    const size_t pair = (size_t)item * gridDim.x + g;
    if (item == 0 && lane == 0) ones[g] = 1;
    const int T = lengths[item];
    bool fine = T >= 1 && T <= frames && verdict[g] != 0;
    int first = 0, S = 0, arc0 = 0, arcs = 0;
    if (fine) {                                                // (uniform) a good verdict: the graph's indices are sound
        first = state_begin[g];
        S = state_begin[g + 1] - first;
        fine = S <= GSTATES;
    }
    if (fine) {
        arc0 = arc_begin[first];
        arcs = arc_begin[first + S] - arc0;
        fine = arcs <= PPG_SEARCH_GRAPH_MAX_ARCS;              // (<= the dynamic LDS: no graph has more than n_arcs)
    }
    if (lane == 0) count[pair] = fine ? 0 : -1;
    if (!fine) return;                                         // (uniform)
    for (int i = lane; i < arcs; i += 64)
        held_arcs[i] = make_uint2((uint32_t)sources[arc0 + i], __float_as_uint(weights[arc0 + i]));
    __syncthreads();                                           // a lane keeps its states' first arcs: it reads them now
    const float4* src = reinterpret_cast<const float4*>(logp + (size_t)item * frames * PREP);
    const ViterbiArcs<true> in_lds{held_arcs, nullptr, nullptr, arcs};
    float* out_totals = totals + pair * frames;
    int* out_begins = begins + pair * frames;
    if (S <= 64)
        search_graph_frames<1, false>(src, T, first, S, phonemes, stay, initial, final_, arc_begin + first, in_lds,
                                      out_totals, out_begins, stage, dist, began, ends, GraphCarry{}, lane);
    else
        search_graph_frames<4, false>(src, T, first, S, phonemes, stay, initial, final_, arc_begin + first, in_lds,
                                      out_totals, out_begins, stage, dist, began, ends, GraphCarry{}, lane);
}

// ---- live phrase search over a phoneme graph (ppg_search_graph_stream_*) ----
//
// ppg_search_graph carried across the pushes of a stream, as ppg_search_stream_* carries ppg_search.  One pair is a
// stream and a graph; every graph runs on every stream.  The curve is the recurrence above, unchanged, with a fresh
// start at frame t of a push at position p beginning at p + t; the detector, flush and reset are the live search's
// (Detector, Events, emit and detect in front of search_strips), word for word.  The caller owns the state: five blocks,
// each 256-byte aligned: the position of every stream (int32), the verdict of viterbi_check on every graph (int32,
// written once, at open), the detector of every pair (8 words), then D and b of every pair: a row of 64 words where
// max_states <= 64 and of 256 above, so that a row is loaded and stored without a mask.  The positions, the detectors
// and the rows lie as the live search's do, so its three small kernels serve here as they are: search_stream_advance
// after the programme (the only writer of a position in a push), search_stream_flush, and search_stream_reset with
// max_states in the place of max_phonemes.  One kernel of its own:
//   search_graph_stream_programme  grid (graphs, streams), one wave per pair: search_graph_frames<G, Live = true>, the
//                                  body of search_graph_programme between a load and a store of the row.  A push goes by
//                                  the verdict stored at open and checks nothing of the graph again, so whatever the
//                                  arrays hold by now, S is held inside [1, row], the arcs inside the held block, and a
//                                  source is clamped into [0, S) where it is copied to LDS: the only place the kernel
//                                  takes one from (ppg_viterbi_stream_push's rule).

struct SearchGraphStreamLayout {
    size_t positions, verdict, detectors, totals, begins, bytes;       // byte offsets into the state
};

// (65535 x 65535 pairs of 256 states are 4.4e12 bytes per block: inside a size_t)
inline SearchGraphStreamLayout search_graph_stream_layout(int streams, int graphs, int max_states) {
    SearchGraphStreamLayout w{};
    const size_t pairs = (size_t)streams * graphs, states = stream_states(max_states);
    size_t at = 0;
    w.positions = at; at = align256(at + (size_t)streams * sizeof(int));
    w.verdict = at; at = align256(at + (size_t)graphs * sizeof(int));
    w.detectors = at; at = align256(at + pairs * sizeof(Detector));
    w.totals = at; at = align256(at + pairs * states * sizeof(float));
    w.begins = at; at = align256(at + pairs * states * sizeof(int));
    w.bytes = at;
    return w;
}

bool search_graph_stream_sizes_fine(int streams, int graphs, int max_states) {
    return streams > 0 && streams <= PPG_SEARCH_MAX_ITEMS && graphs > 0 && graphs <= PPG_SEARCH_MAX_QUERIES &&
           max_states > 0 && max_states <= PPG_VITERBI_MAX_STATES;
}

// the checks every entry of the live search over graphs shares: the state and its geometry
int check_search_graph_stream_state(const char* what, const void* state, int streams, int graphs, int max_states) {
    if (!state || streams <= 0 || graphs <= 0 || max_states <= 0)
        return ppg::fail_message(PPG_EINVAL, "%s: bad argument", what);
    if (!search_graph_stream_sizes_fine(streams, graphs, max_states))
        return ppg::fail_message(PPG_EINVAL, "%s: %d streams, %d graphs and %d states: at most %d streams, %d graphs "
                                 "and %d states per graph", what, streams, graphs, max_states, PPG_SEARCH_MAX_ITEMS,
                                 PPG_SEARCH_MAX_QUERIES, PPG_VITERBI_MAX_STATES);
    if (reinterpret_cast<uintptr_t>(state) % 16)
        return ppg::fail_message(PPG_EINVAL, "%s: the state must be 16-byte aligned", what);
    return PPG_OK;
}

// grid (graphs, streams), 64 threads, `held` * 8 bytes of dynamic LDS; `row` = stream_states(max_states).  count = -1
// for a pair that cannot be pushed (its graph refused at open or beyond 256 states or 4096 arcs, its length outside
// [0, frames], a position that would pass INT32_MAX), which touches nothing else; every other pair gets the events of
// this push, sentinels behind them, and its state moved on by lengths[stream] frames.
__global__ __launch_bounds__(64) void search_graph_stream_programme(
    const float* __restrict__ logp, int frames, const int* __restrict__ lengths, const int* __restrict__ verdict,
    const int* __restrict__ state_begin, const int* __restrict__ phonemes, const float* __restrict__ stay,
    const float* __restrict__ initial, const float* __restrict__ final_, const int* __restrict__ arc_begin,
    const int* __restrict__ sources, const float* __restrict__ weights, int held, int row,
    const int* __restrict__ positions, Detector* __restrict__ detectors, float* __restrict__ state_totals,
    int* __restrict__ state_begins, float threshold, int patience, int cap, int* __restrict__ begin,
    int* __restrict__ end, float* __restrict__ total, float* __restrict__ mean, int* __restrict__ count,
    float* __restrict__ curve_total, int* __restrict__ curve_begin)
{
    __shared__ float4 stage[2][CHUNK_VEC];
    __shared__ __attribute__((aligned(16))) float dist[2][GSTATES];
    __shared__ __attribute__((aligned(16))) int began[2][GSTATES];
    __shared__ SearchGraphEnds ends;
    extern __shared__ uint2 held_arcs[];
    const int g = blockIdx.x, item = blockIdx.y, lane = threadIdx.x;
    const size_t pair = (size_t)item * gridDim.x + g;
    const int T = lengths[item], base = positions[item];
    bool fine = T >= 0 && T <= frames && base >= 0 && T <= INT32_MAX - base && verdict[g] != 0;
    int first = 0, S = 0, arc0 = 0, arcs = 0;
    if (fine) {                                                // (uniform) a good verdict: the graph's indices were sound
        first = state_begin[g];
        S = state_begin[g + 1] - first;
        fine = S >= 1 && S <= row;                             // (row <= GSTATES)
    }
    if (fine) {
        arc0 = arc_begin[first];
        arcs = arc_begin[first + S] - arc0;
        fine = arcs >= 0 && arcs <= held;                      // (held <= PPG_SEARCH_GRAPH_MAX_ARCS: the dynamic LDS)
    }
    if (!fine) {                                               // (uniform)
        if (lane == 0) count[pair] = -1;
        return;
    }
    // what is written now and then by one lane, or once at the end: out of the scalar file, which the frames need
    Events out{in_vector_registers(begin + pair * cap), in_vector_registers(end + pair * cap),
               in_vector_registers(total + pair * cap), in_vector_registers(mean + pair * cap), cap, 0};
    Detector* my_detector = in_vector_registers(detectors + pair);
    int* my_count = in_vector_registers(count + pair);
    if (T > 0) {                                               // (uniform) a stream with no frames sits out the step
        for (int i = lane; i < arcs; i += 64)
            held_arcs[i] = make_uint2((uint32_t)min(max(sources[arc0 + i], 0), S - 1),
                                      __float_as_uint(weights[arc0 + i]));
        __syncthreads();                                       // a lane keeps its states' first arcs: it reads them now
        const float4* src = reinterpret_cast<const float4*>(logp + (size_t)item * frames * PREP);
        const ViterbiArcs<true> in_lds{held_arcs, nullptr, nullptr, arcs};
        float* out_totals = curve_total ? curve_total + pair * frames : nullptr;
        int* out_begins = curve_total ? curve_begin + pair * frames : nullptr;
        Detector det = *my_detector;                           // (every lane reads it; lane 0 uses it)
        const GraphCarry live{in_vector_registers(state_totals + pair * row),
                              in_vector_registers(state_begins + pair * row), base, &det, &out, threshold, patience};
        if (S <= 64)
            search_graph_frames<1, true>(src, T, first, S, phonemes, stay, initial, final_, arc_begin + first, in_lds,
                                         out_totals, out_begins, stage, dist, began, ends, live, lane);
        else
            search_graph_frames<4, true>(src, T, first, S, phonemes, stay, initial, final_, arc_begin + first, in_lds,
                                         out_totals, out_begins, stage, dist, began, ends, live, lane);
        if (lane == 0) *my_detector = det;
    }
    const int events = __builtin_amdgcn_readfirstlane(out.count);
    if (lane == 0) *my_count = events;
    for (int h = min(events, cap) + lane; h < cap; h += 64) {
        out.begin[h] = out.end[h] = -1;
        out.total[h] = out.mean[h] = NAN;
    }
}

}  // namespace

extern "C" {

size_t ppg_search_graph_workspace_bytes(int items, int frames, int graphs) {
    if (items <= 0 || items > PPG_SEARCH_MAX_ITEMS || frames <= 0 || frames > PPG_SEARCH_MAX_FRAMES || graphs <= 0 ||
        graphs > PPG_SEARCH_MAX_QUERIES)
        return 0;
    return search_graph_layout(items, frames, graphs).bytes;
}

int ppg_search_graph(int device, const float* ppg, int frames, int items, const int32_t* lengths, int graphs,
                     int n_states, int n_arcs, int max_states, const int32_t* state_begin,
                     const int32_t* state_phonemes, const float* stay, const float* initial, const float* final_,
                     const int32_t* arc_begin, const int32_t* sources, const float* weights, int top, float threshold,
                     int32_t* begin, int32_t* end, float* total, float* mean, int32_t* count, float* curve_total,
                     int32_t* curve_begin, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "search_graph";
    if (const int rc = check_common(what, ppg, frames, items, lengths, PPG_SEARCH_MAX_FRAMES, PPG_SEARCH_MAX_ITEMS))
        return rc;
    if (!workspace) return ppg::fail_message(PPG_EINVAL, "%s: bad argument", what);
    if (const int rc = check_search_graphs(what, graphs, n_states, n_arcs, max_states, sources, weights)) return rc;
    if (const int rc = check_words(what, {state_begin, state_phonemes, stay, initial, final_, arc_begin, begin, end,
                                          total, mean, count},
                                   {sources, weights, curve_total, curve_begin, ppg, lengths}))
        return rc;
    if (top < 1 || top > PPG_SEARCH_MAX_HITS)
        return ppg::fail_message(PPG_EINVAL, "%s: top = %d, must be 1 .. %d", what, top, PPG_SEARCH_MAX_HITS);
    if (threshold != threshold) return ppg::fail_message(PPG_EINVAL, "%s: the threshold is NaN", what);
    if (!curve_total != !curve_begin)
        return ppg::fail_message(PPG_EINVAL, "%s: curve_total and curve_begin go together", what);
    const SearchGraphLayout w = search_graph_layout(items, frames, graphs);
    if (const int rc = check_workspace(what, workspace, workspace_bytes, w.bytes)) return rc;
    if (const int rc = select_device(device)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    float* logp = reinterpret_cast<float*>(ws + w.logp);
    float* totals = reinterpret_cast<float*>(ws + w.totals);
    int* begins = reinterpret_cast<int*>(ws + w.begins);
    int* verdict = reinterpret_cast<int*>(ws + w.verdict);
    int* ones = reinterpret_cast<int*>(ws + w.ones);
    // the arcs a wave keeps in LDS: no graph of the call has more than all of them, and none it searches more than 4096
    const int held = n_arcs < VHELD ? n_arcs : VHELD;
    hipLaunchKernelGGL(viterbi_check, dim3(graphs), dim3(64), 0, s, n_states, n_arcs, max_states, state_begin,
                       state_phonemes, stay, initial, final_, arc_begin, sources, weights, verdict);
    hipLaunchKernelGGL(align_prepare, dim3((frames + 63) / 64, items), dim3(64), 0, s, ppg, frames, lengths, logp);
    hipLaunchKernelGGL(search_graph_programme, dim3(graphs, items), dim3(64), (size_t)held * sizeof(uint2), s, logp,
                       frames, lengths, verdict, state_begin, state_phonemes, stay, initial, final_, arc_begin, sources,
                       weights, totals, begins, ones, count);
    hipLaunchKernelGGL(search_pick, dim3(graphs, items), dim3(64), 0, s, frames, lengths, ones, top, threshold, totals,
                       begins, begin, end, total, mean, count, curve_total, curve_begin);
    return launched(what);
}

size_t ppg_search_graph_stream_state_bytes(int streams, int graphs, int max_states) {
    return search_graph_stream_sizes_fine(streams, graphs, max_states)
               ? search_graph_stream_layout(streams, graphs, max_states).bytes : 0;
}

size_t ppg_search_graph_stream_workspace_bytes(int streams, int frames, int graphs) {
    if (streams <= 0 || streams > PPG_SEARCH_MAX_ITEMS || frames <= 0 || frames > PPG_SEARCH_MAX_FRAMES ||
        graphs <= 0 || graphs > PPG_SEARCH_MAX_QUERIES)
        return 0;
    return prepared_bytes(streams, frames);
}

int ppg_search_graph_stream_open(int device, void* state, int streams, int graphs, int n_states, int n_arcs,
                                 int max_states, const int32_t* state_begin, const int32_t* state_phonemes,
                                 const float* stay, const float* initial, const float* final_,
                                 const int32_t* arc_begin, const int32_t* sources, const float* weights,
                                 void* stream) {
    const char* what = "search_graph_stream_open";
    if (const int rc = check_search_graph_stream_state(what, state, streams, graphs, max_states)) return rc;
    if (const int rc = check_search_graphs(what, graphs, n_states, n_arcs, max_states, sources, weights)) return rc;
    if (const int rc = check_words(what, {state_begin, state_phonemes, stay, initial, final_, arc_begin},
                                   {sources, weights}))
        return rc;
    if (const int rc = select_device(device)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const SearchGraphStreamLayout w = search_graph_stream_layout(streams, graphs, max_states);
    char* st = static_cast<char*>(state);
    hipLaunchKernelGGL(viterbi_check, dim3(graphs), dim3(64), 0, s, n_states, n_arcs, max_states, state_begin,
                       state_phonemes, stay, initial, final_, arc_begin, sources, weights,
                       reinterpret_cast<int*>(st + w.verdict));
    hipLaunchKernelGGL(search_stream_reset, dim3(graphs, streams), dim3(64), 0, s, max_states,
                       static_cast<const int*>(nullptr), reinterpret_cast<int*>(st + w.positions),
                       reinterpret_cast<Detector*>(st + w.detectors), reinterpret_cast<float*>(st + w.totals),
                       reinterpret_cast<int*>(st + w.begins));
    return launched(what);
}

int ppg_search_graph_stream_reset(int device, void* state, int streams, int graphs, int max_states,
                                  const int32_t* which, void* stream) {
    const char* what = "search_graph_stream_reset";
    if (const int rc = check_search_graph_stream_state(what, state, streams, graphs, max_states)) return rc;
    if (const int rc = check_words(what, {}, {which})) return rc;
    if (const int rc = select_device(device)) return rc;
    const SearchGraphStreamLayout w = search_graph_stream_layout(streams, graphs, max_states);
    char* st = static_cast<char*>(state);
    hipLaunchKernelGGL(search_stream_reset, dim3(graphs, streams), dim3(64), 0, static_cast<hipStream_t>(stream),
                       max_states, which, reinterpret_cast<int*>(st + w.positions),
                       reinterpret_cast<Detector*>(st + w.detectors), reinterpret_cast<float*>(st + w.totals),
                       reinterpret_cast<int*>(st + w.begins));
    return launched(what);
}

int ppg_search_graph_stream_push(int device, void* state, const float* ppg, int frames, int streams,
                                 const int32_t* lengths, int graphs, int n_states, int n_arcs, int max_states,
                                 const int32_t* state_begin, const int32_t* state_phonemes, const float* stay,
                                 const float* initial, const float* final_, const int32_t* arc_begin,
                                 const int32_t* sources, const float* weights, float threshold, int patience, int cap,
                                 int32_t* begin, int32_t* end, float* total, float* mean, int32_t* count,
                                 float* curve_total, int32_t* curve_begin, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    const char* what = "search_graph_stream_push";
    if (!ppg || !lengths || !workspace || frames <= 0) return ppg::fail_message(PPG_EINVAL, "%s: bad argument", what);
    if (const int rc = check_search_graph_stream_state(what, state, streams, graphs, max_states)) return rc;
    if (const int rc = check_search_graphs(what, graphs, n_states, n_arcs, max_states, sources, weights)) return rc;
    if (frames > PPG_SEARCH_MAX_FRAMES)
        return ppg::fail_message(PPG_EINVAL, "%s: %d frames, at most %d", what, frames, PPG_SEARCH_MAX_FRAMES);
    if (const int rc = check_words(what, {state_begin, state_phonemes, stay, initial, final_, arc_begin, begin, end,
                                          total, mean, count},
                                   {sources, weights, curve_total, curve_begin, ppg, lengths}))
        return rc;
    if (threshold != threshold) return ppg::fail_message(PPG_EINVAL, "%s: the threshold is NaN", what);
    if (patience < 0) return ppg::fail_message(PPG_EINVAL, "%s: patience = %d is negative", what, patience);
    if (cap < 1) return ppg::fail_message(PPG_EINVAL, "%s: cap = %d, must be at least 1", what, cap);
    if (!curve_total != !curve_begin)
        return ppg::fail_message(PPG_EINVAL, "%s: curve_total and curve_begin go together", what);
    if (const int rc = check_workspace(what, workspace, workspace_bytes, prepared_bytes(streams, frames))) return rc;
    if (const int rc = select_device(device)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const SearchGraphStreamLayout w = search_graph_stream_layout(streams, graphs, max_states);
    char* st = static_cast<char*>(state);
    int* positions = reinterpret_cast<int*>(st + w.positions);
    float* logp = static_cast<float*>(workspace);
    const int held = n_arcs < VHELD ? n_arcs : VHELD;         // the arcs a wave keeps in LDS, as in ppg_search_graph
    hipLaunchKernelGGL(align_prepare, dim3((frames + 63) / 64, streams), dim3(64), 0, s, ppg, frames, lengths, logp);
    hipLaunchKernelGGL(search_graph_stream_programme, dim3(graphs, streams), dim3(64), (size_t)held * sizeof(uint2), s,
                       logp, frames, lengths, reinterpret_cast<const int*>(st + w.verdict), state_begin, state_phonemes,
                       stay, initial, final_, arc_begin, sources, weights, held, stream_states(max_states), positions,
                       reinterpret_cast<Detector*>(st + w.detectors), reinterpret_cast<float*>(st + w.totals),
                       reinterpret_cast<int*>(st + w.begins), threshold, patience, cap, begin, end, total, mean, count,
                       curve_total, curve_begin);
    hipLaunchKernelGGL(search_stream_advance, dim3((streams + 63) / 64), dim3(64), 0, s, streams, frames, lengths,
                       positions);
    return launched(what);
}

int ppg_search_graph_stream_flush(int device, void* state, int streams, int graphs, int max_states,
                                  const int32_t* which, int32_t* begin, int32_t* end, float* total, float* mean,
                                  int32_t* count, void* stream) {
    const char* what = "search_graph_stream_flush";
    if (const int rc = check_search_graph_stream_state(what, state, streams, graphs, max_states)) return rc;
    if (const int rc = check_words(what, {begin, end, total, mean, count}, {which})) return rc;
    if (const int rc = select_device(device)) return rc;
    const SearchGraphStreamLayout w = search_graph_stream_layout(streams, graphs, max_states);
    const size_t pairs = (size_t)streams * graphs;
    hipLaunchKernelGGL(search_stream_flush, dim3((unsigned)((pairs + 63) / 64)), dim3(64), 0,
                       static_cast<hipStream_t>(stream), streams, graphs, which,
                       reinterpret_cast<Detector*>(static_cast<char*>(state) + w.detectors), begin, end, total, mean,
                       count);
    return launched(what);
}

}  // extern "C"
